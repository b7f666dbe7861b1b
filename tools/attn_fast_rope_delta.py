"""How far the backward's recomputed RoPE^T factors (attention_dev.h rope_tab_fast) stray
from the float64 values of the f32 tables of engine.rotation_tables.

The factors never leave the kernel, so they are read through its outputs: one fast-mode
streaming backward (bf16, head_dim --dh, window T, no dropout) over many heads; the stored
(even, odd) pairs of dq and dk are R(t, i)^T of the unrotated gradient, which
tests/attn_ref.py gives in float64.  Per (t, i), over the heads, the pairs whose
unrotated reference is at least half its row's maximum are solved by least squares for
the implied (cos', sin'):
  cos' = sum(e e' + o o') / sum(e^2 + o^2),  sin' = sum(o e' - e o') / sum(e^2 + o^2)
and delta(t, i) = max(|cos' - cos|, |sin' - sin|).  The outputs are bf16 and carry the
dS rounding, so the solve has a resolution: its standard error is printed beside the
deviations, which mean something only where they exceed it several times.

  python tools/attn_fast_rope_delta.py [--T 300] [--batches 32] [--dh 8..128] [--out FILE]
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from neurosync_trainer_lite_amd import _hip as K  # noqa: E402
from neurosync_trainer_lite_amd.engine import rotation_tables  # noqa: E402
from tests import attn_ref as A  # noqa: E402

DEV, HN, STEP = "cuda:0", 16, 4


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--T", type=int, default=300)
    ap.add_argument("--batches", type=int, default=32, help="heads = 16 x batches (a multiple of 4)")
    ap.add_argument("--dh", type=int, default=64, choices=tuple(range(8, 129, 8)),
                    help="head width of the streaming kernels (a multiple of 8 up to 128)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    T, Bn, DH = args.T, args.batches, args.dh
    assert Bn % STEP == 0
    os.environ["NSTL_ROPE_BWD"] = "fast"
    M, D = Bn * T, HN * DH
    g = torch.Generator().manual_seed(5)
    qkv = torch.randn(M, 3 * D, generator=g).to(torch.bfloat16).to(DEV)
    do = torch.randn(M, D, generator=g).to(torch.bfloat16).to(DEV)
    o = torch.zeros(M, D, dtype=torch.bfloat16, device=DEV)
    dqkv = torch.zeros(M, 3 * D, dtype=torch.bfloat16, device=DEV)
    lse = torch.zeros(Bn * HN * T, device=DEV)
    dsum = torch.zeros(Bn * HN * T, device=DEV)
    cs, sn = rotation_tables(T, DH, DEV)
    a = K.attn_args(K.BF16, Bn, T, HN, qkv.data_ptr(), 3 * D, qkv[:, D:].data_ptr(), 3 * D, qkv[:, 2 * D:].data_ptr(),
                    3 * D, o.data_ptr(), D, lse.data_ptr(), 0.0, 0, dh=DH, flags=K.ATTN_RAGGED_OK | K.ATTN_DH128_OK | K.ATTN_DHANY_OK)
    K.kernel_counts_reset()
    K.attn_fwd(a)
    a.dout, a.dout_ld = do.data_ptr(), D
    a.dq, a.dq_ld, a.dk, a.dk_ld, a.dv, a.dv_ld = (dqkv.data_ptr(), 3 * D, dqkv[:, D:].data_ptr(), 3 * D,
                                                    dqkv[:, 2 * D:].data_ptr(), 3 * D)
    a.rope_cos, a.rope_sin, a.rope_q, a.rope_k = cs.data_ptr(), sn.data_ptr(), 1, 1
    a.dsum = dsum.data_ptr()
    K.attn_bwd(a)
    torch.cuda.synchronize()
    counts = {k: v for k, v in K.kernel_counts().items() if v}

    def hd(x):
        return x.reshape(STEP, T, HN, DH).transpose(1, 2)

    num_c = torch.zeros(T, DH // 2, dtype=torch.float64, device=DEV)
    num_s, den, cnt, yy = (torch.zeros_like(num_c) for _ in range(4))
    for b0 in range(0, Bn, STEP):  # the f64 reference a few batches at a time
        sl = slice(b0 * T, (b0 + STEP) * T)
        q, k, v = (hd(qkv[sl, i * D:(i + 1) * D]) for i in range(3))
        pre = A.attn_bwd_ref(q, k, v, hd(o[sl]), None, hd(do[sl]), 0.0, None, None)
        for i, nm in enumerate(("dq", "dk")):
            st = hd(dqkv[sl, i * D:(i + 1) * D]).double()
            e, od, e1, o1 = pre[nm][..., 0::2], pre[nm][..., 1::2], st[..., 0::2], st[..., 1::2]
            w = (torch.maximum(e.abs(), od.abs()) >= 0.5 * pre[nm].abs().amax(-1, keepdim=True)).double()
            num_c += (w * (e * e1 + od * o1)).sum((0, 1))
            num_s += (w * (od * e1 - e * o1)).sum((0, 1))
            den += (w * (e * e + od * od)).sum((0, 1))
            yy += (w * (e1 * e1 + o1 * o1)).sum((0, 1))
            cnt += w.sum((0, 1))
    c1, s1 = num_c / den, num_s / den
    res2 = (yy - (num_c * num_c + num_s * num_s) / den).clamp_min(0.0)  # the residual at the optimum
    se = torch.sqrt(res2 / (2 * cnt - 2).clamp_min(1)) / torch.sqrt(den)
    delta = torch.maximum((c1 - cs.double()).abs(), (s1 - sn.double()).abs())
    ok = cnt >= 8
    t = torch.arange(T, dtype=torch.float64, device=DEV)[:, None]
    inv = torch.exp(-np.log(10000.0) * torch.arange(0, DH, 2, dtype=torch.float64, device=DEV) / DH)[None, :]
    ang = (t * inv).expand_as(delta)
    small, large = ok & (ang <= 1.0), ok & (ang > 1.0)
    a_half = delta[small].max().item()
    lines = ["launches %s" % counts,
             "T=%d head_dim=%d heads=%d pairs used per (t, i): min %d median %d (entries with < 8, left out: %d)" % (
                 T, DH, Bn * HN, int(cnt.min()), int(cnt.median()), int((~ok).sum())),
             "max delta                          %.3e  (2^-10 = %.3e)" % (delta[ok].max().item(), 2.0 ** -10),
             "A/2: max delta at angle <= 1       %.3e" % a_half,
             "B/2: max (delta - A/2) / angle     %.3e  (angle = t inv_freq_i > 1)" % (
                 ((delta[large] - a_half).clamp_min(0) / ang[large]).max().item()),
             "standard error of the solve: median %.3e max %.3e; max delta / se %.2f" % (
                 se[ok].median().item(), se[ok].max().item(), (delta[ok] / se[ok]).max().item())]
    for lo, hi in ((0, 1), (1, 10), (10, 100), (100, 1000)):
        m = ok & (ang > lo) & (ang <= hi) if lo else ok & (ang <= hi)
        if m.any():
            lines.append("angle in (%d, %d]: max delta %.3e, rms %.3e, rms se %.3e" % (
                lo, hi, delta[m].max().item(), delta[m].pow(2).mean().sqrt().item(), se[m].pow(2).mean().sqrt().item()))
    print("\n".join(lines))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
