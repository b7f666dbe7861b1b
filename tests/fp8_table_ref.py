"""TEST INFRA: an e4m3fn encoder built from the bit layout, independent of torch's
cast, and the row quantisation of include/nstl.h (nstl_fp8_quant_rows) on top of it,
with no GPU dependency.  tests/test_fp8_table_ref.py proves it (agreement with
oracle/fp8_ref.quant_rows, the tie-to-even results at every midpoint);
tests/test_fp8_parity_gpu.py compares the quantisation kernels with it bit for bit.
Never imported by the package.

e4m3fn: 1 sign, 4 exponent (bias 7), 3 mantissa bits; exponent 0 holds subnormals
m 2^-9; there is no infinity, 0x7F / 0xFF are NaN and the largest value is
0x7E = 1.75 2^8 = 448."""
import numpy as np
import torch

E4M3_MAX = 448.0


def _code_value(c):
    e, m = (c >> 3) & 15, c & 7
    mag = m * 2.0 ** -9 if e == 0 else (1.0 + m / 8.0) * 2.0 ** (e - 7)
    if (c & 0x7F) == 0x7F:
        mag = float("nan")
    return -mag if c & 0x80 else mag


# value of every code byte, and the 127 non-negative finite values in code order
CODE_VALUES = np.array([_code_value(c) for c in range(256)], dtype=np.float64)
POS = CODE_VALUES[:0x7F]
assert POS[0x7E] == E4M3_MAX and np.all(np.diff(POS) > 0) and POS[1] == 2.0 ** -9 and POS[8] == 2.0 ** -6


def decode(codes):
    """float64 numpy values of uint8 code bytes (NaN for 0x7F / 0xFF)."""
    return CODE_VALUES[np.asarray(codes, dtype=np.uint8)]


def encode(v):
    """uint8 codes of f32 values with |v| <= 448: the nearest code value, a tie to the
    even mantissa (the even code byte); the sign bit is kept on a zero result; NaN ->
    0x7F | sign."""
    v = np.asarray(v, dtype=np.float32)
    a = np.abs(v).astype(np.float64)
    nan = np.isnan(a)
    a = np.where(nan, 0.0, a)
    assert np.all(a <= E4M3_MAX), "encode: clamp first"
    hi = np.clip(np.searchsorted(POS, a, side="left"), 1, 0x7E)  # POS[hi-1] < a <= POS[hi] (a > 0)
    lo = hi - 1
    mid = (POS[lo] + POS[hi]) * 0.5  # exact: adjacent codes differ in the last of 4 bits
    code = np.where(a < mid, lo, np.where(a > mid, hi, np.where(lo % 2 == 0, lo, hi)))
    code = np.where(nan, 0x7F, code).astype(np.uint8)
    return code | (np.signbit(v).astype(np.uint8) << 7)


def quant_rows_ref(x):
    """(codes uint8 [rows][cols], scale f32 [rows]) of x [rows][cols] (f32 or bf16
    tensor, or an f32 array) as include/nstl.h states nstl_fp8_quant_rows: amax_i =
    max_j |x_ij|; inv = 448 / amax and scale = amax / 448, both in f32 (1 for an
    all-zero row); x inv in f32; clamp to +-448; encode."""
    if isinstance(x, torch.Tensor):
        x = x.detach().float().cpu().numpy()
    x = np.asarray(x, dtype=np.float32)
    amax = np.abs(x).max(axis=1)
    pos = amax > 0
    safe = np.where(pos, amax, np.float32(1.0)).astype(np.float32)
    inv = np.where(pos, np.float32(E4M3_MAX) / safe, np.float32(1.0)).astype(np.float32)
    scale = np.where(pos, safe / np.float32(E4M3_MAX), np.float32(1.0)).astype(np.float32)
    v = np.clip(x * inv[:, None], np.float32(-E4M3_MAX), np.float32(E4M3_MAX)).astype(np.float32)
    return encode(v), scale


def tie_values():
    """f32 values in [0, 448] at which rounding is decided, with a first entry of 448
    (a row holding them has amax == 448, so inv == 1 exactly): 0, every code value,
    every midpoint of adjacent positive codes (the subnormal ones are the odd multiples
    of 2^-10; 2^-10 itself ties to 0), and the f32 neighbours of each midpoint.  All are
    exact in f32 (at most 5 significant bits, or one ulp beside them)."""
    mids = ((POS[:-1] + POS[1:]) * 0.5).astype(np.float32)
    up = np.nextafter(mids, np.float32(np.inf))
    dn = np.nextafter(mids, np.float32(0.0))
    vals = np.concatenate([[np.float32(E4M3_MAX), np.float32(0.0)], POS.astype(np.float32), mids, up, dn])
    return vals.astype(np.float32)


def tie_rows():
    """[2][cols] f32, cols a multiple of 16: tie_values() and their negatives (with -0
    and -448), zero-padded."""
    v = tie_values()
    cols = -(-v.size // 16) * 16
    x = np.zeros((2, cols), dtype=np.float32)
    x[0, :v.size] = v
    x[1, :v.size] = -v
    return x


def inv_mutant_rows():
    """[8][16] f32 rows that tell inv = 448 / amax from 1 / (amax / 448): amax (the
    first element) is one for which the two f32 values differ, and the other elements x
    are chosen so that x * (448 / amax) is exactly a midpoint of two codes while
    x * (1 / (amax / 448)) is not (a row with amax == 448 cannot: both are 1)."""
    rows = []
    rng = np.random.default_rng(7)
    for amax in rng.uniform(0.5, 4.0, 4000).astype(np.float32):
        inv = np.float32(448.0) / amax
        inv2 = np.float32(1.0) / (amax / np.float32(448.0))
        if inv == inv2:
            continue
        # x = mid / inv rounded; keep those where x * inv lands on the midpoint exactly
        mids = ((POS[40:-1] + POS[41:]) * 0.5).astype(np.float32)
        xs = (mids / inv).astype(np.float32)
        hit = xs[(xs * inv == mids) & (xs * inv2 != mids) & (xs < amax)]
        if hit.size >= 3:
            row = np.zeros(16, dtype=np.float32)
            row[0] = amax
            k = min(hit.size, 15)
            row[1:1 + k] = hit[:k]
            rows.append(row)
        if len(rows) == 8:
            break
    assert len(rows) == 8
    return np.stack(rows)
