"""Runs tests/loss_ref.CASES (F <= 64) through nstl_loss_fwd_bwd of the library that
NSTL_LIB_PATH names (default: the tree's own) and saves partial, loss_out and dpred of
every case, whole-clip or chunked as the case says, to --save; with --compare OTHER it
then holds them to another run's under torch.equal and writes the verdict to --out.
The two runs are two processes because a process binds one library:
  NSTL_LIB_PATH=.../libnstl_hip_old.so python tools/loss_narrow_identical.py --save old.pt
  python tools/loss_narrow_identical.py --save new.pt --flags 1 --compare old.pt --out report.txt
An old library's nstl_loss_args has no flags field: it reads the struct's first fields
only, which are laid out the same."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from neurosync_trainer_lite_amd import _hip as K  # noqa: E402
from tests import loss_ref as L  # noqa: E402


def run(c, flags):
    dev = "cuda:0"
    B, T, F, ldd = c["B"], c["T"], c["F"], c["ldd"]
    p, y = (x.to(dev) for x in L.case_inputs(c))
    dpred = torch.zeros(B * T, ldd, dtype=torch.bfloat16 if c["bf16"] else torch.float32, device=dev)
    partial, out = torch.zeros(B, 4, device=dev), torch.zeros(4, device=dev)
    a = K.LossArgs()
    a.B, a.T, a.F = B, T, F
    a.pred, a.pred_ld, a.trg, a.trg_ld = p.data_ptr(), p.stride(0), y.data_ptr(), y.stride(0)
    a.delta, (a.w1, a.w2, a.w3), a.grad_scale = c["delta"], c["w"], c["gs"]
    a.dpred, a.dpred_dtype, a.dpred_ld = dpred.data_ptr(), K.BF16 if c["bf16"] else K.F32, ldd
    a.partial, a.loss_out = partial.data_ptr(), out.data_ptr()
    a.flags = flags
    if c["force"]:
        os.environ["NSTL_LOSS_CHUNKED"] = "1"
    else:
        os.environ.pop("NSTL_LOSS_CHUNKED", None)
    K.loss_fwd_bwd(a)
    torch.cuda.synchronize()
    return dict(partial=partial[:, :3].cpu(), loss_out=out.cpu(), dpred=dpred.cpu())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--save", required=True)
    ap.add_argument("--flags", type=int, default=0)
    ap.add_argument("--compare", default=None)
    ap.add_argument("--out", default=None)
    o = ap.parse_args()
    version = K.lib().nstl_version()
    got = {c["name"]: run(c, o.flags) for c in L.CASES}
    torch.save(dict(version=version, flags=o.flags, cases=got), o.save)
    print("library version %d, flags %d: %d cases saved to %s" % (version, o.flags, len(got), o.save))
    if not o.compare:
        return 0
    other = torch.load(o.compare)
    lines = ["# tools/loss_narrow_identical.py: tests/loss_ref.CASES through nstl_loss_fwd_bwd of two builds, torch.equal of",
             "# partial[:, :3], loss_out[0..3] and dpred (pad columns included); %s" % torch.cuda.get_device_name(0),
             "# this build: nstl_version %d, flags %d; the other: nstl_version %d, flags %d"
             % (version, o.flags, other["version"], other["flags"])]
    bad = 0
    for c in L.CASES:
        a, b = got[c["name"]], other["cases"][c["name"]]
        same = {k: torch.equal(a[k], b[k]) and not torch.isnan(a[k].float()).any() for k in a}
        bad += not all(same.values())
        lines.append("%-12s B %3d T %4d F %2d %-10s %-4s  %s" % (
            c["name"], c["B"], c["T"], c["F"], "chunked" if c["chunked"] else "whole-clip", "bf16" if c["bf16"] else "f32",
            "  ".join("%s %s" % (k, "identical" if v else "DIFFERENT") for k, v in same.items())))
    lines.append("%d of %d cases differ" % (bad, len(L.CASES)))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if o.out:
        with open(o.out, "a") as f:
            f.write(text)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
