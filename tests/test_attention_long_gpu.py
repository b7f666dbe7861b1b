"""The streaming MFMA attention kernels (bf16, head_dim 64, T % 32 == 0,
256 < T <= 4096: csrc/attention_long.hip) against a float64 reference and against
the generic kernels they replace as the default for those shapes.

Shapes: T = 288 = 2 * 128 + 32 has a partial last key tile (32 of 64 keys) and a
partial last 128-row block; 384 has exact tiles and an odd block count; 512 is the
smallest realistic long window.  Tolerances are test_attention_fwd_bwd's bf16 rows
(bf16-rounded inputs shared with the reference; accumulation order and the bf16
output rounding remain)."""
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


def attn_ref(q, k, v, scale, mask=None, p=0.0):
    s = (q @ k.transpose(-1, -2)) * scale
    lse = torch.logsumexp(s, -1)
    P = torch.softmax(s, -1)
    Pd = P * mask / (1 - p) if mask is not None else P
    return Pd @ v, lse


def rope_back_ref(g, cs, sn):
    e, o = g[..., 0::2], g[..., 1::2]
    r = torch.empty_like(g)
    r[..., 0::2] = e * cs + o * sn
    r[..., 1::2] = -e * sn + o * cs
    return r


def run(T, p=0.0, seed=0, stored=False, bias=False, dh=DH, scale=1.0, qseed=20, b=B, h=H):
    """One forward + backward on a packed qkv [M][3D] operand.  Returns a dict of the
    outputs (and the inputs, for a reference)."""
    M, D = b * T, h * dh
    qkv = rnd(M, 3 * D, dtype=BF, scale=scale, seed=qseed)
    do = rnd(M, D, dtype=BF, seed=qseed + 1)
    o = torch.full((M, D), float("nan"), dtype=BF, device=DEV)
    lse = torch.full((b * h * T,), float("nan"), dtype=torch.float32, device=DEV)
    dqkv = torch.full((M, 3 * D), float("nan"), dtype=BF, device=DEV)
    dsum = torch.empty(b * h * T, dtype=torch.float32, device=DEV)
    mask = torch.full((b * h * T * T // 64,), -1, dtype=torch.int64, device=DEV)
    cs, sn = rotation_tables(T, dh, DEV)
    a = K.attn_args(K.BF16, b, T, h, qkv.data_ptr(), 3 * D, qkv[:, D:].data_ptr(), 3 * D, qkv[:, 2 * D:].data_ptr(),
                    3 * D, o.data_ptr(), D, lse.data_ptr(), p, seed, dh=dh)
    if stored:
        a.mask_bits = mask.data_ptr()
    K.kernel_counts_reset()
    K.attn_fwd(a)
    a.dout, a.dout_ld = do.data_ptr(), D
    a.dq, a.dq_ld, a.dk, a.dk_ld, a.dv, a.dv_ld = (dqkv.data_ptr(), 3 * D, dqkv[:, D:].data_ptr(), 3 * D,
                                                    dqkv[:, 2 * D:].data_ptr(), 3 * D)
    a.rope_cos, a.rope_sin, a.rope_q, a.rope_k = cs.data_ptr(), sn.data_ptr(), 1, 1
    a.dsum = dsum.data_ptr()
    rows, part = 0, None
    if bias:
        rows = K.attn_bias_rows(a)
        part = torch.full((max(rows, 1), 3 * D), float("nan"), device=DEV)
        a.dbias_part = part.data_ptr()
    K.attn_bwd(a)
    torch.cuda.synchronize()
    return dict(qkv=qkv, do=do, o=o, lse=lse, dqkv=dqkv, mask=mask, cs=cs, sn=sn, counts=K.kernel_counts(),
                rows=rows, part=part)


@functools.lru_cache(maxsize=None)
def reference(T, B=B, H=H):
    """float64 forward / backward (RoPE^T applied) of run(T, b=B, h=H)'s inputs, computed once per shape."""
    M, D = B * T, H * DH
    qkv = rnd(M, 3 * D, dtype=BF, seed=20)
    do = rnd(M, D, dtype=BF, seed=21)
    q = f64(qkv[:, :D]).view(B, T, H, DH).transpose(1, 2).requires_grad_(True)
    k = f64(qkv[:, D:2 * D]).view(B, T, H, DH).transpose(1, 2).requires_grad_(True)
    v = f64(qkv[:, 2 * D:]).view(B, T, H, DH).transpose(1, 2).requires_grad_(True)
    ro, rl = attn_ref(q, k, v, DH ** -0.5)
    ro.backward(f64(do).view(B, T, H, DH).transpose(1, 2))
    cs, sn = rotation_tables(T, DH, DEV)
    c64, s64 = f64(cs), f64(sn)
    return dict(o=ro.detach().transpose(1, 2).reshape(M, D), lse=rl.detach().reshape(-1),
                dq=rope_back_ref(q.grad, c64, s64).transpose(1, 2).reshape(M, D),
                dk=rope_back_ref(k.grad, c64, s64).transpose(1, 2).reshape(M, D),
                dv=v.grad.transpose(1, 2).reshape(M, D))


def long_counts(c):
    return (c["attn_fwd_long"], c["attn_bwd_long"], c["attn_fwd_generic"], c["attn_bwd_generic"], c["attn_fwd"],
            c["attn_bwd_split"], c["attn_bwd_fused"])


@pytest.mark.parametrize("T", [288, 384, 512])
def test_long_fwd_bwd_against_f64(T):
    D = H * DH
    r = run(T)
    assert long_counts(r["counts"]) == (1, 1, 0, 0, 0, 0, 0), r["counts"]
    ref = reference(T)
    check(r["o"], ref["o"], 1e-2, "attn out T=%d" % T)
    check(r["lse"], ref["lse"], 1e-2, "attn lse T=%d" % T)
    check(r["dqkv"][:, :D], ref["dq"], 3e-2, "dq T=%d" % T)
    check(r["dqkv"][:, D:2 * D], ref["dk"], 3e-2, "dk T=%d" % T)
    check(r["dqkv"][:, 2 * D:], ref["dv"], 3e-2, "dv T=%d" % T)


def test_long_rope_table_vs_fast(monkeypatch):
    """NSTL_ROPE_BWD=table through the long kernels (the switch reaches them in the
    parameter block nstl_attn_bwd fills): RoPE^T from the tables against the
    recomputed angles, at the smallest long shape (partial last tile and block)."""
    T, D = 288, H * DH
    monkeypatch.setenv("NSTL_ROPE_BWD", "table")
    tab = run(T)
    monkeypatch.setenv("NSTL_ROPE_BWD", "fast")
    fast = run(T)
    for r in (tab, fast):
        assert long_counts(r["counts"]) == (1, 1, 0, 0, 0, 0, 0), r["counts"]
    # RoPE does not touch o and dv
    assert torch.equal(tab["o"], fast["o"])
    assert torch.equal(tab["dqkv"][:, 2 * D:], fast["dqkv"][:, 2 * D:])
    ref = reference(T)
    for i, nm in enumerate(("dq", "dk")):
        # recomputed angles vs the tables: the same rotation to well inside bf16 rounding
        check(fast["dqkv"][:, i * D:(i + 1) * D], tab["dqkv"][:, i * D:(i + 1) * D], 8e-3, "fast vs table RoPE^T " + nm)
        check(tab["dqkv"][:, i * D:(i + 1) * D], ref[nm], 3e-2, "table RoPE^T %s vs f64" % nm)


def test_long_max_window():
    """T = 4096, the longest window: 64 tiles per sweep, 32 blocks per head, and the
    dK / dV kernel's largest LDS request (68 KB, past the 64 KB default limit).  One
    batch, two heads; then stored keep bits against re-hashing at the same length."""
    T, b, h = 4096, 1, 2
    D = h * DH
    r = run(T, b=b, h=h)
    assert long_counts(r["counts"]) == (1, 1, 0, 0, 0, 0, 0), r["counts"]
    ref = reference(T, b, h)
    check(r["o"], ref["o"], 1e-2, "attn out T=4096")
    check(r["lse"], ref["lse"], 1e-2, "attn lse T=4096")
    check(r["dqkv"][:, :D], ref["dq"], 3e-2, "dq T=4096")
    check(r["dqkv"][:, D:2 * D], ref["dk"], 3e-2, "dk T=4096")
    check(r["dqkv"][:, 2 * D:], ref["dv"], 3e-2, "dv T=4096")
    hashed = run(T, p=0.3, seed=9, b=b, h=h)
    stored = run(T, p=0.3, seed=9, b=b, h=h, stored=True)
    assert torch.equal(hashed["o"], stored["o"]) and torch.equal(hashed["dqkv"], stored["dqkv"])
    assert not torch.isnan(stored["dqkv"].float()).any()
    frac = np.unpackbits(stored["mask"].cpu().numpy().view(np.uint8)).mean()
    assert abs(frac - 0.7) < 0.01, frac


def test_long_online_softmax_rescale():
    """Inputs scaled so that the row maximum moves by many units from tile to tile:
    every query's running maximum is raised (and O rescaled) at several key tiles."""
    T, D = 288, H * DH
    r = run(T, scale=3.0, qseed=40)
    assert long_counts(r["counts"])[:2] == (1, 1)
    qkv = r["qkv"]
    q = f64(qkv[:, :D]).view(B, T, H, DH).transpose(1, 2)
    k = f64(qkv[:, D:2 * D]).view(B, T, H, DH).transpose(1, 2)
    v = f64(qkv[:, 2 * D:]).view(B, T, H, DH).transpose(1, 2)
    s = (q @ k.transpose(-1, -2)) * DH ** -0.5
    tile_max = torch.stack([s[..., i:i + 64].max(-1).values for i in range(0, T, 64)], -1)
    raised = (tile_max[..., 1:] > torch.cummax(tile_max, -1).values[..., :-1] + 1.0).sum(-1)
    assert (raised >= 1).double().mean() > 0.5  # most rows rescale by more than e at a later tile
    ro, rl = attn_ref(q, k, v, DH ** -0.5)
    check(r["o"], ro.transpose(1, 2).reshape(B * T, D), 1e-2, "attn out (spread scores)")
    check(r["lse"], rl.reshape(-1), 1e-2, "attn lse (spread scores)")


def test_long_dropout_stream_matches_generic(monkeypatch):
    T, D, p = 288, H * DH, 0.3
    monkeypatch.setenv("NSTL_ATTN_LONG", "0")
    g = run(T, p=p, seed=777)
    assert long_counts(g["counts"]) == (0, 0, 1, 1, 0, 0, 0), g["counts"]
    monkeypatch.delenv("NSTL_ATTN_LONG")
    n = run(T, p=p, seed=777)
    assert long_counts(n["counts"]) == (1, 1, 0, 0, 0, 0, 0), n["counts"]
    # a different keep pattern would differ at O(1) of the scale
    check(n["o"], g["o"], 1e-2, "dropout out vs generic")
    check(n["lse"], g["lse"], 1e-2, "dropout lse vs generic")
    check(n["dqkv"][:, :D], g["dqkv"][:, :D], 3e-2, "dropout dq vs generic")
    check(n["dqkv"][:, D:2 * D], g["dqkv"][:, D:2 * D], 3e-2, "dropout dk vs generic")
    check(n["dqkv"][:, 2 * D:], g["dqkv"][:, 2 * D:], 3e-2, "dropout dv vs generic")


@pytest.mark.parametrize("T", [288, 512])
def test_long_stored_mask_bits(T):
    p = 0.3
    hashed = run(T, p=p, seed=4242, qseed=70, scale=0.5)
    stored = run(T, p=p, seed=4242, qseed=70, scale=0.5, stored=True)
    assert long_counts(stored["counts"])[:2] == (1, 1)
    assert torch.equal(hashed["o"], stored["o"])
    assert torch.equal(hashed["lse"], stored["lse"])
    assert torch.equal(hashed["dqkv"], stored["dqkv"])
    assert not torch.isnan(stored["dqkv"].float()).any()
    bits = stored["mask"].cpu().numpy().view(np.uint8)
    frac = np.unpackbits(bits).mean()
    assert abs(frac - (1 - p)) < 0.01, frac


def test_long_bias_partials():
    T, b, h = 288, 3, 2
    D = h * DH
    r = run(T, p=0.2, seed=99, qseed=110, scale=0.5, bias=True, b=b, h=h)
    assert long_counts(r["counts"])[:2] == (1, 1)
    assert r["rows"] == b * 3
    part = r["part"]
    out = torch.full((3 * D,), 5.0, device=DEV)
    K.reduce_rows_strided(part, 3 * D, r["rows"], 3 * D, out, 1.0)
    kpart = torch.zeros(D, device=DEV)
    K.reduce_rows_strided(part[:, D:], 3 * D, r["rows"], D, kpart, 0.0)
    torch.cuda.synchronize()
    ref = f64(r["dqkv"]).sum(0)
    check(out - 5.0, ref, 1e-5, "fused q|k|v bias grads")
    check(kpart, ref[D:2 * D], 1e-5, "k window")


def test_long_backward_reproducible():
    a = run(384, p=0.3, seed=5)
    b = run(384, p=0.3, seed=5)
    assert long_counts(a["counts"])[:2] == (1, 1)
    assert torch.equal(a["o"], b["o"])
    assert torch.equal(a["dqkv"], b["dqkv"])


def test_long_boundary_untouched():
    c = run(256)["counts"]
    assert long_counts(c) == (0, 0, 0, 0, 1, 1, 0), c  # the one-shot kernels, split backward
    c = run(288, dh=128)["counts"]
    assert long_counts(c) == (0, 0, 1, 1, 0, 0, 0), c
    c = run(300)["counts"]
    assert long_counts(c) == (0, 0, 1, 1, 0, 0, 0), c
    a = K.attn_args(K.BF16, 1, 4128, 1, 0, 64, 0, 64, 0, 64, 0, 64, 0, 0.0, 0, dh=64)
    with pytest.raises(RuntimeError, match="T must be"):
        K.attn_fwd(a)
