"""How sharp tests/test_dropout_step_parity_gpu.py is on hardware: give the engine's
BACKWARD wrong site seeds (the forward and the oracle's masks stay right) and count the
figures of a whole step that miss that file's gates.  Wrong masks only: every launch is
the one the right step makes.  Needs an MI355X; run from the repository root:
    python tools/dropout_step_mutants.py
Output of one run: profiles/dropout_step_parity_errors.txt."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from neurosync_trainer_lite_amd import engine as E
from tests import test_dropout_step_parity_gpu as T

orig_seed, orig_bwd = E._seed, E.Seq2SeqEngine.backward
state = {"bwd": False, "mut": None}

def seed(base, enc, layer, site):
    if state["bwd"] and state["mut"] == "drop1<-drop2" and site == "drop1":
        site = "drop2"
    if state["bwd"] and state["mut"] == "layer<-0":
        layer = 0
    if state["bwd"] and state["mut"] == "xresid<-resid" and site == "xresid":
        site = "resid"
    return orig_seed(base, enc, layer, site)

def bwd(self, g, gen):
    state["bwd"] = True
    try:
        return orig_bwd(self, g, gen)
    finally:
        state["bwd"] = False

E._seed = seed
E.Seq2SeqEngine.backward = bwd
for case, amp in ((T.BF16_CASES[0], True), (T.LIFE, True), (T.FP32_CASES[0], False)):
    off = T.off_errors(case) if amp else None
    for mut in (None, "drop1<-drop2", "layer<-0", "xresid<-resid"):
        if mut == "layer<-0" and case[2] == 1:
            continue
        state["mut"] = mut
        errs, x = T.one_step(case, amp, case[5])
        if amp:
            miss = [k for k, e in errs.items() if not e <= min(T.CAPS[T.kind(k)], max(T.FLOOR, T.K_RATIO * off[k]))]
        else:
            miss = [k for k, e in errs.items() if T.kind(k) == "grad" and not e < 1e-4]
        w = max((k for k in errs if T.kind(k) == "grad"), key=errs.get)
        print("%-26s %-5s mutant %-14s figures past their gate %3d / %d; worst gradient %.3e (%s)" % (
            T.tag(case), "bf16" if amp else "fp32", mut, len(miss), len(errs), errs[w], w), flush=True)
