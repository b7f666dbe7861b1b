"""Per-element float64 parity of the streaming attention kernels at head_dim 128
(csrc/attention_long.hip, the <128, ...> instantiations) against tests/attn_ref.py, and
their exact dropout keep bits.  The cases, buffers (NaN pre-fill, sentinel columns and
tails), the judge and the launch-counter tuples are tests/test_attention_parity_gpu.py's,
which are general in dh and flags; shapes are its B = 2, H = 3.

c = 1, as for the head_dim 64 kernels: a 128-wide head is two 64-column halves whose
score products add into the same f32 accumulators (four 32-wide k-chunks instead of
two), and P, P_drop and dS still enter the second product through acc_frag<bf16>: one
bf16 rounding between the scores and every output, whatever the head width.

Fast RoPE^T (rope_tab_fast<128>): the deviation of the recomputed cos / sin from the
float64 value of the f32 tables was measured at head_dim 128 by
tools/attn_fast_rope_delta.py --dh 128 (T = 300, 8192 heads): largest deviation
1.456e-4 at a resolution (standard error of the solve) of 2.1e-5, no slope over the
angle (profiles/attention_dh128_parity_errors.txt).  The bound is twice the largest
deviation, the rule of FAST_A in tests/test_attention_parity_gpu.py: 2.9e-4, not above
that constant (3.1e-4, from 1.52e-4 at head_dim 64), so judge(fast=True) is used
unchanged: this file carries no constant of its own."""
import pytest
import torch

from tests.test_attention_parity_gpu import BF, F32, GENERIC, MODES, STREAMING, check_words, full_case, run

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from neurosync_trainer_lite_amd import _hip as K

DH = 128
RAG, WIDE = 1, 2        # K.ATTN_RAGGED_OK, K.ATTN_DH128_OK (pinned by tests/test_attn_dh128_sizes.py)
BOTH = RAG | WIDE


def flags_for(T):
    return WIDE if T % 32 == 0 else BOTH


def test_flag_is_bound():
    assert K.ATTN_DH128_OK == WIDE and K.ATTN_RAGGED_OK == RAG


# whole tiles, the new flag alone.  32: one active wave, half a tile; 96: a 64 + 32 tile
# pair; 128: the default window, one full block; 160, 288: 2 - 3 row blocks with a
# partial last tile and idle waves
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("T", [32, 64, 96, 128, 160, 288])
def test_streaming_dh128_whole_tiles(T, mode, monkeypatch):
    full_case(monkeypatch, BF, T, mode, STREAMING, 1, dh=DH, flags=WIDE)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("T", [7, 100, 257, 300])
def test_streaming_dh128_ragged(T, mode, monkeypatch):
    full_case(monkeypatch, BF, T, mode, STREAMING, 1, dh=DH, flags=BOTH)


# one batch: rows past T are not another batch's rows, an overrun lands on the sentinel
@pytest.mark.parametrize("T", [7, 100, 257, 300])
def test_streaming_dh128_ragged_one_batch(T, monkeypatch):
    full_case(monkeypatch, BF, T, "stored", STREAMING, 1, b=1, dh=DH, flags=BOTH)


# packed qkv [M][3D], o [M][D], dqkv [M][3D]
@pytest.mark.parametrize("T", [128, 300])
def test_dh128_packed_layout(T, monkeypatch):
    full_case(monkeypatch, BF, T, "stored", STREAMING, 1, dh=DH, flags=flags_for(T), packed=True)


@pytest.mark.parametrize("rope", [(1, 0), (0, 1), (0, 0)])
@pytest.mark.parametrize("T", [96, 300])
def test_dh128_rope_selection(T, rope, monkeypatch):
    full_case(monkeypatch, BF, T, "hashed", STREAMING, 1, dh=DH, flags=flags_for(T), rope=rope)


# ---- dispatch
@pytest.mark.parametrize("flags", [0, RAG])
@pytest.mark.parametrize("T", [128, 300])
def test_dh128_without_the_flag_is_generic(T, flags, monkeypatch):
    r = full_case(monkeypatch, BF, T, "hashed", GENERIC, 0, dh=DH, flags=flags)
    assert r["words"] == 0 and r["rows"] == 0


@pytest.mark.parametrize("T", [128, 300])
def test_dh128_long_switch_off_is_generic(T, monkeypatch):
    r = full_case(monkeypatch, BF, T, "hashed", GENERIC, 0, dh=DH, flags=BOTH, env=(("NSTL_ATTN_LONG", "0"),))
    assert r["words"] == 0 and r["rows"] == 0


def test_dh128_f32_is_generic(monkeypatch):
    r = full_case(monkeypatch, F32, 96, "hashed", GENERIC, 0, dh=DH, flags=BOTH)
    assert r["words"] == 0 and r["rows"] == 0


@pytest.mark.parametrize("T", [128, 288, 300])
def test_dh64_does_not_read_the_flag(T, monkeypatch):
    """A head_dim 64 call with NSTL_ATTN_DH128_OK added: the same kernels, the same bits."""
    monkeypatch.setenv("NSTL_ROPE_BWD", "table")
    base = RAG if T % 32 else 0
    a = run(BF, T, mode="stored", flags=base)
    b = run(BF, T, mode="stored", flags=base | WIDE)
    assert a["counts"] == b["counts"] and a["counts"] != GENERIC, (a["counts"], b["counts"])
    assert a["words"] == b["words"] > 0 and a["rows"] == b["rows"] > 0
    for nm in ("o", "lse", "dq", "dk", "dv", "dsum", "mask", "part"):
        if nm == "dsum" and not (a["counts"][1] or a["counts"][5]):
            continue    # the fused backward (T = 128) leaves the scratch at its NaN pre-fill
        assert torch.equal(a[nm], b[nm]), "%s: %s differs with the flag" % (a["what"], nm)


# ---- interchangeability of stored and re-hashed keep bits
@pytest.mark.parametrize("T", [128, 300])
def test_dh128_stored_words_are_the_hash_stream(T, monkeypatch):
    monkeypatch.setenv("NSTL_ROPE_BWD", "table")
    s = run(BF, T, dh=DH, mode="stored", flags=flags_for(T))
    assert s["counts"] == STREAMING, s["counts"]
    check_words(s)   # == attn_ref.keep_words of nstl_keep(seed, drop_idx), exactly
    h = run(BF, T, dh=DH, mode="hashed", flags=flags_for(T))
    assert h["counts"] == STREAMING and h["mask"] is None
    for nm in ("o", "lse", "dq", "dk", "dv", "dsum", "part"):
        assert torch.equal(s[nm], h[nm]), "%s: stored vs hashed %s" % (s["what"], nm)


# ---- the production default: cos / sin recomputed in the kernel
@pytest.mark.parametrize("T", [128, 300])
def test_dh128_fast_rope(T, monkeypatch):
    full_case(monkeypatch, BF, T, "stored", STREAMING, 1, dh=DH, flags=flags_for(T), rope_mode="fast", twin=False)
