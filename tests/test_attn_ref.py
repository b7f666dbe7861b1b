"""The float64 attention reference of tests/attn_ref.py against torch autograd, the
scalar port of the dropout hash, the keep-word decode of test_dropout_hash_statistics
and a CPU emulation of the kernels' bf16 roundings, before any kernel is judged by
it (tests/test_attention_parity_gpu.py)."""
import functools

import numpy as np
import pytest
import torch

from neurosync_trainer_lite_amd.engine import rotation_tables
from tests import attn_ref as A
from tests import gemm_ref as G
from tests.test_gemm_ref import SEED, nstl_keep

BF = torch.bfloat16
B, H = 2, 3
# every (dtype, T, dh, c) of tests/test_attention_parity_gpu.py (c: attn_ref's table)
MFMA_T = (32, 64, 96, 128, 160, 192, 224, 256, 288, 320, 7, 100, 257, 300)
SHAPES = ([(BF, T, 64, 1) for T in MFMA_T] + [(torch.float32, T, 64, 0) for T in (32, 64, 96, 128)] +
          [(torch.float32, 7, 24, 0), (torch.float32, 48, 64, 0), (BF, 40, 64, 0), (BF, 100, 128, 0), (BF, 300, 64, 0)])


def rnd(*shape, seed=0, scale=1.0, dtype=torch.float64):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g, dtype=torch.float64) * scale).to(dtype)


def heads(x, b, T, h, dh):
    return x.reshape(b, T, h, dh).transpose(1, 2)


@pytest.mark.parametrize("T,p,rope", [(7, 0.3, (1, 1)), (33, 0.0, (1, 0)), (40, 0.3, (0, 1)), (64, 0.5, (0, 0))])
def test_reference_equals_autograd(T, p, rope):
    dh = 16
    q, k, v = (rnd(B, H, T, dh, seed=s).requires_grad_(True) for s in (1, 2, 3))
    do = rnd(B, H, T, dh, seed=4)
    kp = A.keep(SEED, B * H, T, p)
    cos, sin = rotation_tables(T, dh, "cpu")
    S = (q @ k.transpose(-1, -2)) * dh ** -0.5
    mask = torch.from_numpy(kp).reshape(B, H, T, T).double() * G.inv_keep(p) if p > 0 else 1.0
    o = (torch.softmax(S, -1) * mask) @ v
    o.backward(do)
    f = A.attn_fwd_ref(q, k, v, p, kp)
    assert (f["o"] - o.detach()).abs().max().item() <= 1e-12
    assert (f["lse"] - torch.logsumexp(S.detach(), -1)).abs().max().item() <= 1e-12
    assert (f["mag_o"] >= f["o"].abs() - 1e-15).all() and (f["mag32_o"] >= f["mag_o"]).all()
    r = A.attn_bwd_ref(q, k, v, o.detach(), None, do, p, kp, (cos, sin) + rope)
    want = dict(dq=A.rope_back(q.grad, cos, sin) if rope[0] else q.grad,
                dk=A.rope_back(k.grad, cos, sin) if rope[1] else k.grad, dv=v.grad)
    for nm, w in want.items():
        assert (r[nm] - w).abs().max().item() <= 1e-12, nm
        assert (r["mag_" + nm] >= r[nm].abs() - 1e-13).all(), nm
        assert (r["mag32_" + nm] >= r["mag_" + nm] - 1e-13).all(), nm
    # the stored LSE, when given, is what P is formed from
    r2 = A.attn_bwd_ref(q, k, v, o.detach(), f["lse"].float(), do, p, kp, (cos, sin) + rope)
    assert (r2["dv"] - r["dv"]).abs().max().item() <= 1e-5 * r["mag_dv"].max().item()


@pytest.mark.parametrize("T", [7, 12, 33])
def test_keep_equals_scalar_port(T):
    BH, p = 5, 0.3
    thresh = G.drop_thresh(p)
    assert SEED >> 32
    got = A.keep(SEED, BH, T, p)
    assert got.shape == (BH, T, T) and got.dtype == np.bool_
    want = np.array([[[nstl_keep(SEED, (bh * T + q) * T + k, thresh) for k in range(T)] for q in range(T)]
                     for bh in range(BH)])
    assert np.array_equal(got, want)
    assert A.keep(SEED, BH, T, 0.0).all()


@pytest.mark.parametrize("T", [7, 100, 128])
def test_keep_words_round_trip_and_layout(T):
    BH, nt = 6, (T + 15) // 16
    kp = A.keep(SEED, BH, T, 0.3)
    w = A.keep_words(kp, T)
    assert w.dtype == np.uint64 and w.shape == (BH * nt * nt * 4,)
    assert np.array_equal(A.words_to_keep(w, BH, T), kp)
    # bit by bit, the layout as attention_dev.h states it
    w4 = w.reshape(BH, nt, nt, 4)
    rs = np.random.RandomState(T)
    for _ in range(200):
        bh, qq, kk = rs.randint(BH), rs.randint(nt * 16), rs.randint(nt * 16)
        bit = (int(w4[bh, qq // 16, kk // 16, kk % 4]) >> (16 * ((kk % 16) // 4) + qq % 16)) & 1
        assert bit == (int(kp[bh, qq, kk]) if qq < T and kk < T else 0), (bh, qq, kk)
    # bits of queries / keys at or past T are 0
    assert int(np.unpackbits(w.view(np.uint8)).sum()) == int(kp.sum())
    if T % 16 == 0:
        # the decode of test_kernels_gpu.test_dropout_hash_statistics
        bits = ((w4[..., None] >> np.arange(64, dtype=np.uint64)) & np.uint64(1)).astype(np.uint8)
        dec = bits.reshape(BH, nt, nt, 4, 4, 16).transpose(0, 1, 5, 2, 4, 3).reshape(BH, T, T)
        assert np.array_equal(dec.astype(bool), kp)


# ---------------------------------------------------------------------------
# CPU emulation of the kernels' roundings: f32 arithmetic, one bf16 rounding on P
# (kept, unnormalised), on the kept P of dV, on dS (c = 1: the MFMA kernels; c = 0: the
# generic kernels keep them in f32) and on each stored output.
def emulate(dt, T, dh, c, p, kp, b=B, rope=(1, 1), seed=20):
    st = (lambda x: x.to(BF).float()) if dt == BF else (lambda x: x)
    rr = st if c else (lambda x: x)
    q, k, v, do = (heads(rnd(b * T, H * dh, seed=seed + i, dtype=dt).float(), b, T, H, dh) for i in range(4))
    keepf = torch.from_numpy(kp).reshape(b, H, T, T).float() if p > 0 else torch.ones(b, H, T, T)
    ik, sc = G.f32v(G.inv_keep(p) if p > 0 else 1.0), G.f32v(dh ** -0.5)
    s = q @ k.transpose(-1, -2)
    m = s.amax(-1, keepdim=True)
    e = torch.exp2((s - m) * G.f32v(sc * 1.4426950408889634))
    l = e.sum(-1, keepdim=True)
    o = st((rr(e * keepf) @ v) * (ik / l))
    lse = (m * sc + torch.log(l))[..., 0]
    P = torch.exp(s * sc - lse[..., None])
    D = (do * o).sum(-1, keepdim=True)
    dv = (rr(P * keepf).transpose(-1, -2) @ do) * ik
    dS = rr(P * ((do @ v.transpose(-1, -2)) * keepf * ik - D))
    dq, dk = (dS @ k) * sc, (dS.transpose(-1, -2) @ q) * sc
    cos, sin = rotation_tables(T, dh, "cpu")
    if rope[0]:
        dq = A.rope_back(dq.double(), cos, sin).float()
    if rope[1]:
        dk = A.rope_back(dk.double(), cos, sin).float()
    return dict(q=q, k=k, v=v, do=do, o=o, lse=lse, dq=st(dq), dk=st(dk), dv=st(dv), cos=cos, sin=sin)


def ratios(em, dt, c, p, kp, rope=(1, 1)):
    f = A.attn_fwd_ref(em["q"], em["k"], em["v"], p, kp)
    r = A.attn_bwd_ref(em["q"], em["k"], em["v"], em["o"], None, em["do"], p, kp, (em["cos"], em["sin"]) + rope)
    out = {"o": A.worst(em["o"], f["o"], A.bound(f["o"], f["mag_o"], dt, c, f["mag32_o"])),
           "lse": A.worst(em["lse"], f["lse"], A.lse_bound(f["lse_mag"]))}
    for nm in ("dq", "dk", "dv"):
        out[nm] = A.worst(em[nm], r[nm], A.bound(r[nm], r["mag_" + nm], dt, c, r["mag32_" + nm]))
    return out


@pytest.mark.parametrize("dt,T,dh,c", SHAPES)
@pytest.mark.parametrize("p", [0.0, 0.3])
def test_rounding_emulation_stays_under_the_bound(dt, T, dh, c, p):
    """The condition that the reference alone passes: a correct computation with the
    kernels' roundings sits under the bound at every shape of the GPU file."""
    kp = A.keep(777, B * H, T, p)
    out = ratios(emulate(dt, T, dh, c, p, kp), dt, c, p, kp)
    print("emulation %s T=%d dh=%d p=%.1f: " % (str(dt)[6:], T, dh, p) +
          " ".join("%s %.3f" % (nm, x[0]) for nm, x in out.items()))
    for nm, (ratio, idx) in out.items():
        assert ratio < 1.0, (nm, ratio, idx)


@functools.lru_cache(maxsize=None)
def _t300():
    T, p = 300, 0.3
    kp = A.keep(777, B * H, T, p)
    return T, p, kp, emulate(BF, T, 64, 1, p, kp)


@pytest.mark.parametrize("bh,qq", [(0, 0), (3, 299), (5, 150)])
def test_one_flipped_keep_bit_exceeds_the_bound(bh, qq):
    """A single wrong keep decision (the key of median probability in its row) is
    1 / T of the scale in max-norm; per element it is over the bound."""
    T, p, kp, em = _t300()
    P = torch.softmax((em["q"].double() @ em["k"].double().transpose(-1, -2)) / 8.0, -1).reshape(B * H, T, T)
    kk = int(P[bh, qq].argsort()[T // 2])
    bad = kp.copy()
    bad[bh, qq, kk] = not bad[bh, qq, kk]
    out = ratios(emulate(BF, T, 64, 1, p, bad), BF, 1, p, kp)
    print("flipped keep bit (%d, %d, %d): " % (bh, qq, kk) + " ".join("%s %.2f" % (nm, x[0]) for nm, x in out.items()))
    assert out["o"][0] > 1.0 and out["o"][1][:3] == (bh // H, bh % H, qq)
    assert out["dv"][0] > 1.0 or out["dq"][0] > 1.0
    assert out["lse"][0] < 1.0  # the LSE is taken over the undropped scores


def test_one_dropped_key_exceeds_the_bound():
    """Key 299 left out of query 17's row of one head at T = 300, p = 0."""
    T = 300
    kp = A.keep(0, B * H, T, 0.0)
    good = emulate(BF, T, 64, 1, 0.0, kp)
    assert max(x[0] for x in ratios(good, BF, 1, 0.0, kp).values()) < 1.0
    q, k, v = (good[n][1, 2].double() for n in ("q", "k", "v"))
    s = (q[17] @ k[:299].T) / 8.0
    o_bad = (torch.softmax(s, -1) @ v[:299]).to(BF)
    bad = dict(good, o=good["o"].clone(), lse=good["lse"].clone())
    bad["o"][1, 2, 17] = o_bad.float()
    bad["lse"][1, 2, 17] = torch.logsumexp(s, -1).float()
    out = ratios(bad, BF, 1, 0.0, kp)
    print("dropped key: " + " ".join("%s %.2f" % (nm, x[0]) for nm, x in out.items()))
    # the row's LSE moves by P(17, 299), hundreds of its f32 bound, whatever the key's
    # weight; O moves by P |v - o|, over its bf16 bound only for a key of some weight
    assert out["lse"][0] > 1.0 and out["lse"][1] == (1, 2, 17)
    # in max-norm the same error passes today's checks
    f = A.attn_fwd_ref(good["q"], good["k"], good["v"])
    assert (bad["o"].double() - f["o"]).abs().max() < 1e-2 * f["o"].abs().max()
