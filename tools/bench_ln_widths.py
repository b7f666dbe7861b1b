"""LayerNorm forward / backward at the widths beyond the original four, next to the
D = 1024 instantiation in the same process: bf16, dropout 0.3, as the engine calls
them (forward: x + dropout(y) -> s, out, stats; backward: s, the f32 residual
gradient in place, the bf16 hand-off, two masks, dbranch and its column-sum partials,
256 partial blocks), with rows * D held at 16,384 * 1024 elements.  The arms are
alternated: every round times each width once (median of 5 launches by device
events), after a warm-up of every width; the figure of a width is the median over
the rounds and its ratio is to D = 1024's rate in the same run.
  python tools/bench_ln_widths.py [out.txt]"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from neurosync_trainer_lite_amd import _hip as K  # noqa: E402

ELEMS = 16384 * 1024
WIDTHS = [1024, 768, 1536, 2048, 384, 1152]
ROUNDS, REPS, N_PART = 15, 5, 256
dev = "cuda:0"
bf = torch.bfloat16


class Arm:
    def __init__(self, D):
        self.D, self.R = D, ELEMS // D // 8 * 8
        R = self.R
        self.x = torch.randn(R, D, device=dev).to(bf)
        self.y = torch.randn(R, D, device=dev).to(bf)
        self.s, self.out = torch.empty_like(self.x), torch.empty_like(self.x)
        self.stat = torch.empty(2, R, device=dev)
        self.gamma, self.beta = torch.ones(D, device=dev), torch.zeros(D, device=dev)
        self.dres = torch.randn(R, D, device=dev) * 1e-3
        self.dadd = (torch.randn(R, D, device=dev) * 1e-3).to(bf)
        self.dbranch = torch.empty_like(self.x)
        self.part = torch.empty(3, N_PART, D, device=dev)
        self.bytes = {"fwd": R * D * 2 * 4, "bwd": R * D * 14}
        self.times = {"fwd": [], "bwd": []}

    def args(self, n_masks, **ops):
        a = K.ln_args(K.dtype_code(bf), self.R, self.D, n_masks, 0.3, 11, 12, n_part=N_PART)
        return K.ln_set(a, gamma=self.gamma, beta=self.beta, mean=self.stat[0], rstd=self.stat[1], **ops)

    def fwd(self):
        K.ln_fwd(self.args(1, x=self.x, y=self.y, s_out=self.s, out=self.out))

    def bwd(self):
        K.ln_bwd(self.args(2, s_in=self.s, dout=self.dres, ds=self.dres, dbranch=self.dbranch, dout2=self.dadd,
                           dgamma_part=self.part[0], dbeta_part=self.part[1], dbranch_part=self.part[2]))


def timed(fn):
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(REPS)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return sorted(a.elapsed_time(b) for a, b in ev)[REPS // 2] * 1e-3


def median(v):
    return sorted(v)[len(v) // 2]


def main():
    arms = [Arm(D) for D in WIDTHS]
    for arm in arms:
        for _ in range(3):
            arm.fwd()
            arm.bwd()
    torch.cuda.synchronize()
    for _ in range(ROUNDS):
        for arm in arms:
            arm.times["fwd"].append(timed(arm.fwd))
            arm.times["bwd"].append(timed(arm.bwd))
    lines = ["# tools/bench_ln_widths.py: bf16, rows * D = 16,384 * 1024, %d alternated rounds, %s"
             % (ROUNDS, torch.cuda.get_device_name(0)),
             "# %-6s %6s %6s %10s %8s %10s %10s %10s   %s" % ("kernel", "D", "rows", "median us", "TB/s", "min us", "max us",
                                                             "MB", "rate / D=1024's")]
    for kind in ("fwd", "bwd"):
        base = arms[0].bytes[kind] / median(arms[0].times[kind])
        for arm in arms:
            ts = arm.times[kind]
            rate = arm.bytes[kind] / median(ts)
            lines.append("ln_%-5s %6d %6d %10.1f %8.2f %10.1f %10.1f %10.0f   %.3f"
                         % (kind, arm.D, arm.R, median(ts) * 1e6, rate * 1e-12, min(ts) * 1e6, max(ts) * 1e6,
                            arm.bytes[kind] / 1e6, rate / base))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
