"""Ragged windows (T % 32 != 0) on the streaming MFMA attention kernels: a caller
that sets NSTL_ATTN_RAGGED_OK (and sizes mask_bits / dbias_part by
nstl_attn_mask_words / nstl_attn_bias_rows) gets them for bf16, head_dim 64 and any
T in [1, 4096]; without the flag a ragged T stays on the generic kernels.

Shapes, the smallest that exercise each tail:
  300  third block = two full waves, a wave of 12 rows, five idle waves; fifth key
       tile = a full 32-key chunk and one of 12 keys
  257  odd; the last block and the last tile hold one row / one key
  100  below the one-shot limit: one block, a wave of 4 rows, second tile of 36 keys
  7    odd; one partial wave, one partial tile; every query's row of dropout
       indices starts at alternating parity
  4095 (B = 1, H = 2) the largest LDS request and the longest sweep
Every output buffer carries a sentinel behind it (16 rows / 64 words): rows >= T of
one batch are rows of the next, so each shape also runs with one batch, where an
overrun lands on the sentinel only.  Tolerances are test_attention_long_gpu's."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from neurosync_trainer_lite_amd import _hip as K
    from neurosync_trainer_lite_amd.engine import rotation_tables

DEV = "cuda:0"
B, H, DH = 2, 3, 64
BF = torch.bfloat16
SENT = 7.0                      # sentinel value of the float buffers
SENT_W = 0x0123456789ABCDEF     # ... of the keep-bit words
FILL_W = 0x5A5A5A5A5A5A5A5A     # pre-fill of the words the call must write


def rnd(*shape, dtype=torch.float32, scale=1.0, seed=0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g, dtype=torch.float64) * scale).to(dtype).to(DEV)


def f64(t):
    return t.detach().double().cpu()


def check(got, ref, rel, what):
    got, ref = f64(got), f64(ref)
    scale = ref.abs().max().item() + 1e-30
    err = (got - ref).abs().max().item()
    print("%s: max err %.3e vs scale %.3e (bound %.1e)" % (what, err, scale, rel))
    assert err <= rel * scale, "%s: max err %.3e vs scale %.3e (rel %.1e)" % (what, err, scale, rel)


def attn_ref(q, k, v, scale):
    s = (q @ k.transpose(-1, -2)) * scale
    return torch.softmax(s, -1) @ v, torch.logsumexp(s, -1)


def rope_back_ref(g, cs, sn):
    e, o = g[..., 0::2], g[..., 1::2]
    r = torch.empty_like(g)
    r[..., 0::2] = e * cs + o * sn
    r[..., 1::2] = -e * sn + o * cs
    return r


def guarded(n_rows, cols, extra, dtype, fill):
    """[n_rows + extra][cols] with `fill` in front and the sentinel behind."""
    t = torch.full((n_rows + extra, cols), SENT, dtype=dtype, device=DEV)
    t[:n_rows] = fill
    return t


def run(T, p=0.0, seed=0, stored=True, bias=True, dh=DH, scale=1.0, qseed=20, b=B, h=H, flags=None, dtype=BF):
    """One forward + backward on a packed qkv [M][3D] operand with the flag set
    (flags=0: without).  Checks the sentinels and that no NaN pre-fill remains;
    returns the outputs (views without the sentinel) and the launch counts."""
    flags = K.ATTN_RAGGED_OK if flags is None else flags
    M, D, nan = b * T, h * dh, float("nan")
    qkv = rnd(M, 3 * D, dtype=dtype, scale=scale, seed=qseed)
    do = rnd(M, D, dtype=dtype, seed=qseed + 1)
    o = guarded(M, D, 16, dtype, nan)
    dqkv = guarded(M, 3 * D, 16, dtype, nan)
    lse = guarded(b * h * T, 1, 64, torch.float32, nan)
    dsum = guarded(b * h * T, 1, 64, torch.float32, nan)
    cs, sn = rotation_tables(T, dh, DEV)
    a = K.attn_args(K.dtype_code(dtype), b, T, h, qkv.data_ptr(), 3 * D, qkv[:, D:].data_ptr(), 3 * D,
                    qkv[:, 2 * D:].data_ptr(), 3 * D, o.data_ptr(), D, lse.data_ptr(), p, seed, dh=dh, flags=flags)
    words = K.attn_mask_words(a)
    mask = None
    if stored and words:
        mask = torch.full((words + 64,), SENT_W, dtype=torch.int64, device=DEV)
        mask[:words] = FILL_W
        a.mask_bits = mask.data_ptr()
    K.kernel_counts_reset()
    K.attn_fwd(a)
    a.dout, a.dout_ld = do.data_ptr(), D
    a.dq, a.dq_ld, a.dk, a.dk_ld, a.dv, a.dv_ld = (dqkv.data_ptr(), 3 * D, dqkv[:, D:].data_ptr(), 3 * D,
                                                    dqkv[:, 2 * D:].data_ptr(), 3 * D)
    a.rope_cos, a.rope_sin, a.rope_q, a.rope_k = cs.data_ptr(), sn.data_ptr(), 1, 1
    a.dsum = dsum.data_ptr()
    rows = K.attn_bias_rows(a) if bias else 0
    part = None
    if rows:
        part = guarded(rows, 3 * D, 16, torch.float32, nan)
        a.dbias_part = part.data_ptr()
    K.attn_bwd(a)
    torch.cuda.synchronize()
    counts = K.kernel_counts()
    streaming = counts["attn_bwd_long"] > 0
    for name, t, n in (("o", o, M), ("dqkv", dqkv, M), ("lse", lse, b * h * T), ("dsum", dsum, b * h * T),
                       ("dbias_part", part, rows)):
        if t is None:
            continue
        assert (t[n:].float() == SENT).all(), "%s: sentinel overwritten (T=%d, b=%d)" % (name, T, b)
        if name == "dsum" and not streaming:
            continue  # scratch: only the streaming dQ kernel is required to fill it
        assert not torch.isnan(t[:n].float()).any(), "%s: NaN pre-fill left (T=%d, b=%d)" % (name, T, b)
    if mask is not None:
        assert (mask[words:] == SENT_W).all(), "mask_bits: sentinel overwritten (T=%d, b=%d)" % (T, b)
    return dict(qkv=qkv, do=do, o=o[:M], lse=lse[:b * h * T, 0], dqkv=dqkv[:M], cs=cs, sn=sn, counts=counts,
                mask=None if mask is None else mask[:words], words=words, rows=rows,
                part=None if part is None else part[:rows])


@functools.lru_cache(maxsize=None)
def reference(T, b=B, h=H):
    """float64 forward / backward (RoPE^T applied) of run(T, b=b, h=h)'s inputs, once per shape."""
    M, D = b * T, h * DH
    qkv = rnd(M, 3 * D, dtype=BF, seed=20)
    do = rnd(M, D, dtype=BF, seed=21)
    q = f64(qkv[:, :D]).view(b, T, h, DH).transpose(1, 2).requires_grad_(True)
    k = f64(qkv[:, D:2 * D]).view(b, T, h, DH).transpose(1, 2).requires_grad_(True)
    v = f64(qkv[:, 2 * D:]).view(b, T, h, DH).transpose(1, 2).requires_grad_(True)
    ro, rl = attn_ref(q, k, v, DH ** -0.5)
    ro.backward(f64(do).view(b, T, h, DH).transpose(1, 2))
    cs, sn = rotation_tables(T, DH, DEV)
    c64, s64 = f64(cs), f64(sn)
    return dict(o=ro.detach().transpose(1, 2).reshape(M, D), lse=rl.detach().reshape(-1),
                dq=rope_back_ref(q.grad, c64, s64).transpose(1, 2).reshape(M, D),
                dk=rope_back_ref(k.grad, c64, s64).transpose(1, 2).reshape(M, D),
                dv=v.grad.transpose(1, 2).reshape(M, D))


def counts7(c):
    return (c["attn_fwd_long"], c["attn_bwd_long"], c["attn_fwd_generic"], c["attn_bwd_generic"], c["attn_fwd"],
            c["attn_bwd_split"], c["attn_bwd_fused"])


STREAMING, GENERIC = (1, 1, 0, 0, 0, 0, 0), (0, 0, 1, 1, 0, 0, 0)


def against_f64(r, T, b, h):
    D = h * DH
    assert counts7(r["counts"]) == STREAMING, r["counts"]
    ref = reference(T, b, h)
    tag = " T=%d b=%d" % (T, b)
    check(r["o"], ref["o"], 1e-2, "attn out" + tag)
    check(r["lse"], ref["lse"], 1e-2, "attn lse" + tag)
    check(r["dqkv"][:, :D], ref["dq"], 3e-2, "dq" + tag)
    check(r["dqkv"][:, D:2 * D], ref["dk"], 3e-2, "dk" + tag)
    check(r["dqkv"][:, 2 * D:], ref["dv"], 3e-2, "dv" + tag)


@pytest.mark.parametrize("b", [B, 1])
@pytest.mark.parametrize("T", [300, 257, 100, 7])
def test_ragged_fwd_bwd_against_f64(T, b):
    against_f64(run(T, b=b), T, b, H)


def test_ragged_max_window():
    against_f64(run(4095, b=1, h=2), 4095, 1, 2)


@pytest.mark.parametrize("T", [300, 257])
def test_ragged_dropout_stream_matches_generic(T):
    """The keep decision of (bh, q, k) is nstl_keep(seed, drop_idx(bh, T, q, k)) on
    every path; a different keep pattern would differ at O(1) of the scale."""
    D, p = H * DH, 0.3
    g = run(T, p=p, seed=777, flags=0)
    assert counts7(g["counts"]) == GENERIC, g["counts"]
    n = run(T, p=p, seed=777)
    assert counts7(n["counts"]) == STREAMING, n["counts"]
    check(n["o"], g["o"], 1e-2, "dropout out vs generic")
    check(n["lse"], g["lse"], 1e-2, "dropout lse vs generic")
    check(n["dqkv"][:, :D], g["dqkv"][:, :D], 3e-2, "dropout dq vs generic")
    check(n["dqkv"][:, D:2 * D], g["dqkv"][:, D:2 * D], 3e-2, "dropout dk vs generic")
    check(n["dqkv"][:, 2 * D:], g["dqkv"][:, 2 * D:], 3e-2, "dropout dv vs generic")


@pytest.mark.parametrize("T", [300, 257, 100])
def test_ragged_stored_mask_bits(T):
    p = 0.3
    hashed = run(T, p=p, seed=4242, qseed=70, scale=0.5, stored=False)
    stored = run(T, p=p, seed=4242, qseed=70, scale=0.5, stored=True)
    assert counts7(hashed["counts"]) == STREAMING and counts7(stored["counts"]) == STREAMING
    assert torch.equal(hashed["o"], stored["o"])
    assert torch.equal(hashed["lse"], stored["lse"])
    assert torch.equal(hashed["dqkv"], stored["dqkv"])
    nt = (T + 15) // 16
    assert stored["words"] == B * H * nt * nt * 4
    mask = stored["mask"]
    assert not (mask == FILL_W).any(), "keep-bit words left unwritten"
    # bits of queries / keys past T are 0: the kept fraction of the B*H*T*T real elements
    ones = int(np.unpackbits(mask.cpu().numpy().view(np.uint8)).sum())
    frac = ones / (B * H * T * T)
    print("T=%d kept fraction %.4f" % (T, frac))
    assert abs(frac - (1 - p)) < 0.01, frac


def test_ragged_bias_partials():
    T, b, h = 300, 3, 2
    D = h * DH
    r = run(T, p=0.2, seed=99, qseed=110, scale=0.5, b=b, h=h)
    assert counts7(r["counts"]) == STREAMING, r["counts"]
    assert r["rows"] == 9
    part = r["part"]
    out = torch.full((3 * D,), 5.0, device=DEV)
    K.reduce_rows_strided(part, 3 * D, r["rows"], 3 * D, out, 1.0)
    torch.cuda.synchronize()
    check(out - 5.0, f64(r["dqkv"]).sum(0), 1e-5, "fused q|k|v bias grads")


def test_ragged_reproducible():
    a = run(300, p=0.3, seed=5)
    b = run(300, p=0.3, seed=5)
    assert counts7(a["counts"]) == STREAMING
    assert torch.equal(a["o"], b["o"]) and torch.equal(a["lse"], b["lse"])
    assert torch.equal(a["dqkv"], b["dqkv"])
    assert torch.equal(a["mask"], b["mask"]) and torch.equal(a["part"], b["part"])


def test_ragged_rope_table_vs_fast(monkeypatch):
    T, D = 257, H * DH
    monkeypatch.setenv("NSTL_ROPE_BWD", "table")
    tab = run(T)
    monkeypatch.setenv("NSTL_ROPE_BWD", "fast")
    fast = run(T)
    for r in (tab, fast):
        assert counts7(r["counts"]) == STREAMING, r["counts"]
    assert torch.equal(tab["o"], fast["o"])
    assert torch.equal(tab["dqkv"][:, 2 * D:], fast["dqkv"][:, 2 * D:])
    ref = reference(T)
    for i, nm in enumerate(("dq", "dk")):
        check(fast["dqkv"][:, i * D:(i + 1) * D], tab["dqkv"][:, i * D:(i + 1) * D], 8e-3, "fast vs table RoPE^T " + nm)
        check(tab["dqkv"][:, i * D:(i + 1) * D], ref[nm], 3e-2, "table RoPE^T %s vs f64" % nm)


@pytest.mark.parametrize("T", [128, 256, 288])
def test_flag_changes_nothing_for_whole_tiles(T):
    plain = run(T, p=0.3, seed=11, flags=0)
    flagged = run(T, p=0.3, seed=11)
    assert counts7(plain["counts"]) == counts7(flagged["counts"])
    assert counts7(plain["counts"])[2:4] == (0, 0)
    assert plain["words"] == flagged["words"] == B * H * T * T // 64
    assert plain["rows"] == flagged["rows"]
    for nm in ("o", "lse", "dqkv", "mask", "part"):
        assert torch.equal(plain[nm], flagged[nm]), nm


def test_flag_dispatch(monkeypatch):
    # f32 and head_dim 128 have no streaming kernels, flag or not
    assert counts7(run(300, dtype=torch.float32)["counts"]) == GENERIC
    assert counts7(run(300, dh=128)["counts"]) == GENERIC
    monkeypatch.setenv("NSTL_ATTN_RAGGED", "0")
    r = run(300)
    assert counts7(r["counts"]) == GENERIC and r["words"] == 0 and r["rows"] == 0
    monkeypatch.delenv("NSTL_ATTN_RAGGED")
    monkeypatch.setenv("NSTL_ATTN_LONG", "0")
    assert counts7(run(300)["counts"]) == GENERIC
