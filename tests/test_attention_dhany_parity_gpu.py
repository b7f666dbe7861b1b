"""Per-element float64 parity of the streaming attention kernels at the head widths
other than 64 and 128 (csrc/attention_long.hip, the runtime-width instantiations: any
multiple of 8 below 128, behind NSTL_ATTN_DHANY_OK) against tests/attn_ref.py, and their
exact dropout keep bits.  The cases, buffers (NaN padding columns behind every operand
row, NaN pre-fill, sentinel columns and tails behind every output), the judge and the
launch-counter tuples are tests/test_attention_parity_gpu.py's, which are general in dh
and flags; shapes are its B = 2, H = 3.

c = 1, as at head_dim 64 and 128: the absent columns of an image add exact zeros to the
f32 score accumulators, and P, P_drop and dS still enter the second product through
acc_frag<bf16>: one bf16 rounding between the scores and every output, whatever the
width.  No tolerance of this file's own.

The widths sit at the edges of the 8-column granularity: 8 (one piece, a quarter
k-chunk), 24 (one and a half accumulator tiles), 32 (exactly one k-chunk), 56 (second
k-chunk short of its last piece), 72 (second image with one piece), 96 (a whole second
k-chunk in the second image), 120 (second image short of its last piece).  The padded
layout puts NaN behind the last head of every operand row and the packed layout puts
the next operand there: a read past dh that reached a product would show as NaN or as
an error, an over-wide store or bias sum as the neighbouring head's error or a lost
sentinel.

Fast RoPE^T (rope_tab_fast_w, the frequency divisor dh at run time): the deviation of
the recomputed cos / sin from the float64 value of the f32 tables was measured by
tools/attn_fast_rope_delta.py at head_dim 8, 32 and 120 (T = 300, 8192 heads;
profiles/attention_dhany_parity_errors.txt): largest deviation 1.884e-4 at head_dim 8
(standard error of the solve 1.6e-5), 1.321e-4 at 32 (1.8e-5), 1.508e-4 at 120 (2.1e-5).
At head_dim 8 the largest value sits at angles above 100 rad: a quarter of that table's
pairs have inv_freq 1, so its angles reach t = 299, where the f32 product t * inv_freq
/ 2 pi given to v_sin / v_cos has lost the most; at angle <= 1 it is 1.516e-4, the
head_dim 64 figure.  Twice 1.884e-4 is above FAST_A of
tests/test_attention_parity_gpu.py (3.1e-4, from 1.52e-4 at head_dim 64), so by that
constant's own rule -- twice the measured maximum -- this file carries FAST_A_ANY =
3.8e-4 and judge(fast=True) runs with it in FAST_A's place, otherwise unchanged."""
import pytest
import torch

from tests.test_attention_parity_gpu import BF, F32, GENERIC, MODES, STREAMING, check_words, full_case, run

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from neurosync_trainer_lite_amd import _hip as K

RAG, WIDE, ANY = 1, 2, 4        # K.ATTN_RAGGED_OK, K.ATTN_DH128_OK, K.ATTN_DHANY_OK (tests/test_attn_dhany_sizes.py)
BOTH = RAG | ANY
WIDTHS = [8, 24, 32, 56, 72, 96, 120]
ALL_MODES = [32, 96]            # widths that run every dropout mode; the others run "stored"
CASES = [(dh, mode) for dh in WIDTHS for mode in (MODES if dh in ALL_MODES else ["stored"])]


def flags_for(T):
    return ANY if T % 32 == 0 else BOTH


def test_flag_is_bound():
    assert K.ATTN_DHANY_OK == ANY and K.ATTN_DH128_OK == WIDE and K.ATTN_RAGGED_OK == RAG


# whole tiles, the new flag alone.  32: one active wave, half a tile; 96: a 64 + 32 tile
# pair; 160: two row blocks with a partial last tile and idle waves
@pytest.mark.parametrize("dh,mode", CASES)
@pytest.mark.parametrize("T", [32, 96, 160])
def test_streaming_whole_tiles(T, dh, mode, monkeypatch):
    full_case(monkeypatch, BF, T, mode, STREAMING, 1, dh=dh, flags=ANY)


@pytest.mark.parametrize("dh,mode", CASES)
@pytest.mark.parametrize("T", [7, 100, 300])
def test_streaming_ragged(T, dh, mode, monkeypatch):
    full_case(monkeypatch, BF, T, mode, STREAMING, 1, dh=dh, flags=BOTH)


# one batch: rows past T are not another batch's rows, an overrun lands on the sentinel
@pytest.mark.parametrize("dh,T", [(8, 300), (24, 7), (32, 100), (56, 300), (72, 100), (96, 7), (120, 300)])
def test_streaming_ragged_one_batch(dh, T, monkeypatch):
    full_case(monkeypatch, BF, T, "stored", STREAMING, 1, b=1, dh=dh, flags=BOTH)


# packed qkv [M][3D], o [M][D], dqkv [M][3D]: the columns behind a head are the next
# head's, behind the last head the next operand's
@pytest.mark.parametrize("T", [96, 300])
@pytest.mark.parametrize("dh", [24, 120])
def test_packed_layout(dh, T, monkeypatch):
    full_case(monkeypatch, BF, T, "stored", STREAMING, 1, dh=dh, flags=flags_for(T), packed=True)


@pytest.mark.parametrize("rope", [(1, 0), (0, 1), (0, 0)])
@pytest.mark.parametrize("dh,T", [(24, 300), (96, 96)])
def test_rope_selection(dh, T, rope, monkeypatch):
    full_case(monkeypatch, BF, T, "hashed", STREAMING, 1, dh=dh, flags=flags_for(T), rope=rope)


# ---- interchangeability of stored and re-hashed keep bits
@pytest.mark.parametrize("dh,T", [(32, 96), (32, 300), (72, 96), (72, 300)])
def test_stored_words_are_the_hash_stream(dh, T, monkeypatch):
    monkeypatch.setenv("NSTL_ROPE_BWD", "table")
    s = run(BF, T, dh=dh, mode="stored", flags=flags_for(T))
    assert s["counts"] == STREAMING, s["counts"]
    check_words(s)   # == attn_ref.keep_words of nstl_keep(seed, drop_idx), exactly
    h = run(BF, T, dh=dh, mode="hashed", flags=flags_for(T))
    assert h["counts"] == STREAMING and h["mask"] is None
    for nm in ("o", "lse", "dq", "dk", "dv", "dsum", "part"):
        assert torch.equal(s[nm], h[nm]), "%s: stored vs hashed %s" % (s["what"], nm)


# ---- dispatch
@pytest.mark.parametrize("flags", [0, RAG, RAG | WIDE])
@pytest.mark.parametrize("dh,T", [(32, 96), (96, 300)])
def test_without_the_flag_is_generic(dh, T, flags, monkeypatch):
    r = full_case(monkeypatch, BF, T, "hashed", GENERIC, 0, dh=dh, flags=flags)
    assert r["words"] == 0 and r["rows"] == 0


@pytest.mark.parametrize("dh,T", [(32, 96), (96, 300)])
def test_long_switch_off_is_generic(dh, T, monkeypatch):
    r = full_case(monkeypatch, BF, T, "hashed", GENERIC, 0, dh=dh, flags=BOTH | WIDE, env=(("NSTL_ATTN_LONG", "0"),))
    assert r["words"] == 0 and r["rows"] == 0


def test_f32_is_generic(monkeypatch):
    r = full_case(monkeypatch, F32, 96, "hashed", GENERIC, 0, dh=32, flags=BOTH | WIDE)
    assert r["words"] == 0 and r["rows"] == 0


def test_head_dim_136_is_generic(monkeypatch):
    r = full_case(monkeypatch, BF, 96, "hashed", GENERIC, 0, dh=136, flags=BOTH | WIDE)
    assert r["words"] == 0 and r["rows"] == 0


@pytest.mark.parametrize("dh,T", [(64, 128), (64, 288), (64, 300), (128, 96), (128, 300)])
def test_dh64_and_dh128_do_not_read_the_flag(dh, T, monkeypatch):
    """A head_dim 64 or 128 call with NSTL_ATTN_DHANY_OK added: the same kernels, the same bits."""
    monkeypatch.setenv("NSTL_ROPE_BWD", "table")
    base = (RAG if T % 32 else 0) | (WIDE if dh == 128 else 0)
    a = run(BF, T, dh=dh, mode="stored", flags=base)
    b = run(BF, T, dh=dh, mode="stored", flags=base | ANY)
    assert a["counts"] == b["counts"] and a["counts"] != GENERIC, (a["counts"], b["counts"])
    assert a["words"] == b["words"] > 0 and a["rows"] == b["rows"] > 0
    for nm in ("o", "lse", "dq", "dk", "dv", "dsum", "mask", "part"):
        if nm == "dsum" and not (a["counts"][1] or a["counts"][5]):
            continue    # the fused backward (T = 128) leaves the scratch at its NaN pre-fill
        assert torch.equal(a[nm], b[nm]), "%s: %s differs with the flag" % (a["what"], nm)


def test_dh128_keeps_its_own_bit(monkeypatch):
    r = full_case(monkeypatch, BF, 96, "hashed", GENERIC, 0, dh=128, flags=BOTH)
    assert r["words"] == 0 and r["rows"] == 0


# ---- the production default: cos / sin recomputed in the kernel
FAST_A_ANY = 3.8e-4     # 2 x 1.884e-4, the largest measured deviation (head_dim 8; see the docstring)


@pytest.mark.parametrize("dh,T", [(8, 300), (32, 96), (32, 300), (120, 96), (120, 300)])
def test_fast_rope(dh, T, monkeypatch):
    import tests.test_attention_parity_gpu as P
    monkeypatch.setattr(P, "FAST_A", FAST_A_ANY)    # fast_delta() reads it per call
    full_case(monkeypatch, BF, T, "stored", STREAMING, 1, dh=dh, flags=flags_for(T), rope_mode="fast", twin=False)
