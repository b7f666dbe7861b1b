"""CPU proof of tests/fp8_table_ref.py: the table encoder agrees with
oracle/fp8_ref.quant_rows (so torch's e4m3 cast is the same function), and it rounds
ties to the even mantissa at every midpoint, which random data almost never hits."""
import numpy as np
import torch

from oracle import fp8_ref
from tests import fp8_table_ref as F8


def codes_of(q):
    return q.view(torch.uint8).numpy()


def test_code_table():
    assert F8.CODE_VALUES[0x7E] == 448.0 and F8.CODE_VALUES[0xFE] == -448.0
    assert np.isnan(F8.CODE_VALUES[0x7F]) and np.isnan(F8.CODE_VALUES[0xFF])
    assert F8.CODE_VALUES[0x01] == 2.0 ** -9 and F8.CODE_VALUES[0x07] == 7 * 2.0 ** -9
    assert F8.CODE_VALUES[0x08] == 2.0 ** -6 and F8.CODE_VALUES[0x38] == 1.0 and F8.CODE_VALUES[0x3C] == 1.5
    # the same values as torch's decode of every byte
    t = torch.arange(256, dtype=torch.uint8).view(torch.float8_e4m3fn).double().numpy()
    assert np.array_equal(np.nan_to_num(t, nan=1e9), np.nan_to_num(F8.CODE_VALUES, nan=1e9))
    assert np.array_equal(np.signbit(t), np.signbit(F8.CODE_VALUES))
    # every code value encodes to itself
    fin = np.array([c for c in range(256) if (c & 0x7F) != 0x7F], dtype=np.uint8)
    assert np.array_equal(F8.encode(F8.decode(fin).astype(np.float32)), fin)


def test_agrees_with_oracle_on_random_rows():
    g = torch.Generator().manual_seed(3)
    for dtype in (torch.float32, torch.bfloat16):
        for scale in (1.0, 1e-3, 300.0):
            x = (torch.randn(37, 528, generator=g) * scale).to(dtype)
            x[5] = 0
            x[6, 1:] = 0
            q, s = fp8_ref.quant_rows(x)
            cr, sr = F8.quant_rows_ref(x)
            assert np.array_equal(codes_of(q), cr)
            assert np.array_equal(s.numpy(), sr)
            assert sr[5] == 1.0 and not cr[5].any()


def test_ties_round_to_the_even_mantissa():
    x = F8.tie_rows()
    codes, scale = F8.quant_rows_ref(x)
    assert np.array_equal(scale, np.ones(2, dtype=np.float32))  # amax == 448: inv == 1
    n = F8.POS.size
    v = F8.tie_values()
    assert v[0] == 448.0 and codes[0, 0] == 0x7E and codes[1, 0] == 0xFE
    assert codes[0, 1] == 0x00 and codes[1, 1] == 0x80  # +0 and -0
    o = 2
    assert np.array_equal(codes[0, o:o + n], np.arange(n))  # the code values themselves
    lo = np.arange(n - 1)
    even = np.where(lo % 2 == 0, lo, lo + 1)
    mid, up, dn = (codes[0, o + n + k * (n - 1):o + n + (k + 1) * (n - 1)] for k in range(3))
    assert np.array_equal(mid, even)      # a tie goes to the even code
    assert np.array_equal(up, lo + 1)     # one f32 ulp above the midpoint: up
    assert np.array_equal(dn, lo)         # one below: down
    assert v[o + n] == 2.0 ** -10 and mid[0] == 0  # 2^-10 ties to 0
    sub = v[o + n:o + n + 8] / 2.0 ** -10
    assert np.array_equal(sub, np.arange(1, 16, 2))  # subnormal midpoints: odd multiples of 2^-10
    # the negative row mirrors it with the sign bit
    assert np.array_equal(codes[1, :v.size], codes[0, :v.size] | 0x80)
    # torch's cast gives the same answers on these values
    q, _ = fp8_ref.quant_rows(torch.from_numpy(x))
    assert np.array_equal(codes_of(q), codes)


def test_inv_from_the_rounded_scale_differs_on_a_tie_row():
    """The mutant `inv = 1 / scale`: with amax = 448 (1 + 2^-23) style rows the two
    reciprocals differ in the last bit for some amax, and a value that x * inv puts on a
    midpoint moves off it.  The rows the GPU file uses must tell the two apart."""
    x = F8.inv_mutant_rows()
    codes, _ = F8.quant_rows_ref(x)
    amax = np.abs(x).max(axis=1)
    inv2 = (np.float32(1.0) / (amax / np.float32(448.0))).astype(np.float32)
    mutant = F8.encode(np.clip(x * inv2[:, None], np.float32(-448), np.float32(448)).astype(np.float32))
    assert (mutant != codes).any()
