"""Times nstl_loss_fwd_bwd (csrc/loss.hip) on both LDS tiles, the arms alternating in one
process: B = 128 sequences, bf16 dpred with dpred_ld = 64 (F <= 64) or 128.
  F61 T128 flag 0   the narrow whole-clip kernel, the call of the default step (yardstick)
  F64 T128          the narrow tile full
  F68 T128          the wide whole-clip kernel, 68 of 128 columns
  F128 T128         the wide tile full
  F68 T256          the wide chunked kernel (126 + 126 + 4 frames)
Each round times every arm once (ITERS calls between two device events); the figure of
an arm is the median over the rounds, with the spread.  The kernel counter shows which
tile ran.  Usage: python tools/bench_loss_wide.py [--rounds 15] [--iters 200] [--out FILE]"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from neurosync_trainer_lite_amd import _hip as K  # noqa: E402

ARMS = [("F61 T128 flag 0", 61, 128, 0), ("F64 T128", 64, 128, K.LOSS_WIDE_OK), ("F68 T128", 68, 128, K.LOSS_WIDE_OK),
        ("F128 T128", 128, 128, K.LOSS_WIDE_OK), ("F68 T256", 68, 256, K.LOSS_WIDE_OK)]
B = 128


def arm(F, T, flags, dev):
    ld = 64 if F <= 64 else 128
    g = torch.Generator(device=dev).manual_seed(F * 1000 + T)
    pred = torch.randn(B * T, ld, generator=g, device=dev)
    trg = torch.randn(B * T, F, generator=g, device=dev) * 20
    keep = dict(pred=pred, trg=trg, dpred=torch.empty(B * T, ld, dtype=torch.bfloat16, device=dev),
                partial=torch.empty(B, 4, device=dev), out=torch.empty(4, device=dev))
    a = K.LossArgs()
    a.B, a.T, a.F = B, T, F
    a.pred, a.pred_ld, a.trg, a.trg_ld = pred.data_ptr(), ld, trg.data_ptr(), F
    a.delta, a.w1, a.w2, a.w3, a.grad_scale = 1.0, 1.0, 1.0, 1.0, 1.0
    a.dpred, a.dpred_dtype, a.dpred_ld = keep["dpred"].data_ptr(), K.BF16, ld
    a.partial, a.loss_out = keep["partial"].data_ptr(), keep["out"].data_ptr()
    a.flags = flags
    return a, keep


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--out", default=None)
    o = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_loss_wide: needs a GPU")
    dev = torch.device("cuda:0")
    os.environ.pop("NSTL_LOSS_CHUNKED", None)
    arms = [(name, F, T) + arm(F, T, flags, dev) for name, F, T, flags in ARMS]
    wide = {}
    for name, F, T, a, keep in arms:  # warm-up of every shape, and which tile it takes
        K.kernel_counts_reset()
        for _ in range(20):
            K.loss_fwd_bwd(a)
        torch.cuda.synchronize()
        wide[name] = K.kernel_counts()["loss_wide"] // 20
        assert torch.isfinite(keep["out"]).all(), name
    times = {name: [] for name, *_ in arms}
    for _ in range(o.rounds):
        for name, F, T, a, keep in arms:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(o.iters):
                K.loss_fwd_bwd(a)
            e1.record()
            e1.synchronize()
            times[name].append(e0.elapsed_time(e1) * 1e3 / o.iters)
    lines = ["# tools/bench_loss_wide.py: nstl_loss_fwd_bwd + loss_final, B = %d, bf16 dpred; us per call, median of %d rounds"
             % (B, o.rounds),
             "# of %d back-to-back calls each, the arms alternating in one process (%s)" % (o.iters, torch.cuda.get_device_name(0)),
             "# %-18s %-6s %9s %9s %9s" % ("arm", "tile", "median", "min", "max")]
    for name, *_ in arms:
        t = times[name]
        lines.append("%-20s %-6s %9.2f %9.2f %9.2f" % (name, "wide" if wide[name] else "narrow", statistics.median(t),
                                                      min(t), max(t)))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if o.out:
        with open(o.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
