"""Training step A/B of the streaming attention kernels against the generic ones at a
head width that has no one-shot kernels (head_dim 128): the default dispatch against
NSTL_ATTN_LONG=0, the same process, the same model, arms alternated (the switch is read
per call), median ms/step per arm.  Also prints the launch counters of one step per arm:
the attention family, and the GEMM families the projections took (at rope_dim 128 the
4-wave GEMM's RoPE table rule T * dim * 4 <= 32 KB fails from T = 64 on, so the q|k|v +
RoPE projections leave it).

  python tools/step_ab_attn_long.py [--hidden 1024] [--heads 8] [--layers 2] [--batch 128]
                                    [--seq 128] [--rounds 5] [--steps 6] [--out FILE]
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from neurosync_trainer_lite_amd import _hip as K  # noqa: E402
from neurosync_trainer_lite_amd.config import training_config  # noqa: E402
from neurosync_trainer_lite_amd.utils.model_utils import build_model, prepare_training_components  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--hidden", type=int, default=1024)
    ap.add_argument("--heads", type=int, default=8)
    ap.add_argument("--layers", type=int, default=2)
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--seq", type=int, default=128)
    ap.add_argument("--rounds", type=int, default=5, help="alternations of the two arms")
    ap.add_argument("--steps", type=int, default=6, help="timed steps per arm and round")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    B, T = args.batch, args.seq
    cfg = dict(training_config)
    cfg.update(hidden_dim=args.hidden, num_heads=args.heads, n_layers=args.layers, micro_batch_size=T, frame_size=T,
               batch_size=B)
    torch.manual_seed(1234)
    model = build_model(cfg, dev)
    model.train()
    crit, opt, _ = prepare_training_components(cfg, model)
    g = torch.Generator(device=dev).manual_seed(100)
    src = torch.randn(B, T, cfg["input_dim"], device=dev, generator=g)
    trg = torch.randn(B, T, cfg["output_dim"], device=dev, generator=g) * 20

    def step():
        opt.zero_grad()
        loss = crit(model(src), trg)
        loss.backward()
        opt.step(max_norm=2.0)

    def arm(name):
        if name == "generic":
            os.environ["NSTL_ATTN_LONG"] = "0"
        else:
            os.environ.pop("NSTL_ATTN_LONG", None)

    def timed(n):
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n)]
        for a, b in ev:
            a.record()
            step()
            b.record()
        torch.cuda.synchronize()
        return [a.elapsed_time(b) for a, b in ev]

    lines = ["hidden_dim %d num_heads %d (head_dim %d) layers %d B %d T %d dropout %.2f amp %s" % (
        args.hidden, args.heads, args.hidden // args.heads, args.layers, B, T, cfg["dropout"], cfg.get("use_amp"))]
    arms = ("streaming", "generic")
    for name in arms:   # warm-up, discarded; then one counted step
        arm(name)
        timed(3)
        K.kernel_counts_reset()
        step()
        torch.cuda.synchronize()
        lines.append("%-9s launches of one step: %s" % (name, {k: v for k, v in K.kernel_counts().items() if v}))
    ms = {name: [] for name in arms}
    for _ in range(args.rounds):
        for name in arms:
            arm(name)
            ms[name] += timed(args.steps)
    arm("streaming")
    for name in arms:
        x = sorted(ms[name])
        lines.append("%-9s ms/step: median %.3f min %.3f max %.3f over %d steps in %d alternated rounds" % (
            name, x[len(x) // 2], x[0], x[-1], len(x), args.rounds))
    med = {name: sorted(ms[name])[len(ms[name]) // 2] for name in arms}
    lines.append("generic / streaming: %.3f" % (med["generic"] / med["streaming"]))
    print("\n".join(lines))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
