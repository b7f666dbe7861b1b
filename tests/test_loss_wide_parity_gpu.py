"""nstl_loss_fwd_bwd's wide tile (csrc/loss.hip, 64 < F <= 128 with NSTL_LOSS_WIDE_OK)
against tests/loss_ref.py's float64 values under tests/loss_wide_ref.py's bounds, in
the frame of tests/test_loss_parity_gpu.py: through K.loss_fwd_bwd with K.LossArgs
directly, padded pred / trg rows with NaN in the padding, f32 and bf16 dpred with
dpred_ld >= F (pad columns exact zeros), NaN canaries after every output, both wide
kernels at the smallest shapes that reach each path (loss_wide_ref.CASES).  No
element is excluded.  The launch counter loss_wide shows that a wide kernel ran.

run_kernel and check_frame are restated here: the existing file's run_kernel sets no
flags.

NSTL_LOSS_WIDE_PARITY_ERRORS_OUT=<file>: the worst err/bound of every case is appended
(profiles/loss_wide_parity_errors.txt is one such run)."""
import os

import pytest
import torch

from tests import loss_ref as L
from tests import loss_wide_ref as W

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def record(name, what, ratio):
    line = "%-16s %-10s worst err/bound %.4f" % (name, what, ratio)
    print(line)
    path = os.environ.get("NSTL_LOSS_WIDE_PARITY_ERRORS_OUT")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


def run_kernel(c, p, y, monkeypatch, flags=None):
    """One call on NaN-prefilled outputs: (partial [B+1][4], loss_out [5], dpred
    [B*T+2][ldd]) on the CPU, and the loss_wide launches it counted."""
    import neurosync_trainer_lite_amd._hip as K
    B, T, F, ldd = c["B"], c["T"], c["F"], c["ldd"]
    nan = float("nan")
    pd, yd = p.to(DEV), y.to(DEV)
    dpred = torch.full((B * T + 2, ldd), nan, dtype=torch.bfloat16 if c["bf16"] else torch.float32, device=DEV)
    partial = torch.full((B + 1, 4), nan, dtype=torch.float32, device=DEV)
    out = torch.full((5,), nan, dtype=torch.float32, device=DEV)
    a = K.LossArgs()
    a.B, a.T, a.F = B, T, F
    a.pred, a.pred_ld = pd.data_ptr(), pd.stride(0)
    a.trg, a.trg_ld = yd.data_ptr(), yd.stride(0)
    a.delta, (a.w1, a.w2, a.w3), a.grad_scale = c["delta"], c["w"], c["gs"]
    a.dpred, a.dpred_dtype, a.dpred_ld = dpred.data_ptr(), K.BF16 if c["bf16"] else K.F32, ldd
    a.partial, a.loss_out = partial.data_ptr(), out.data_ptr()
    a.flags = K.LOSS_WIDE_OK if flags is None else flags
    if c["force"]:
        monkeypatch.setenv("NSTL_LOSS_CHUNKED", "1")
    else:
        monkeypatch.delenv("NSTL_LOSS_CHUNKED", raising=False)
    K.kernel_counts_reset()
    K.loss_fwd_bwd(a)
    torch.cuda.synchronize()
    return (partial.cpu(), out.cpu(), dpred.cpu()), K.kernel_counts()["loss_wide"]


def check_frame(c, partial, out, dpred):
    """What no case may disturb: canaries, the unwritten partial column, the pad columns."""
    B, T, F = c["B"], c["T"], c["F"]
    assert torch.isnan(partial[B]).all(), "partial row B written"
    assert torch.isnan(partial[:B, 3]).all(), "partial[:, 3] is written by no kernel"
    assert torch.isnan(out[4]), "loss_out[4] written"
    assert torch.isnan(dpred[B * T:].float()).all(), "rows after dpred written"
    pad = dpred[:B * T, F:].float()
    assert torch.equal(pad, torch.zeros_like(pad)), "dpred columns F..dpred_ld-1 are not exact zeros"


def judge_case(c, r, got, tag=""):
    partial, out, dpred = got
    B, T = c["B"], c["T"]
    pb, ob, db = W.bounds(r, c["chunked"], torch.bfloat16 if c["bf16"] else torch.float32)
    bad = []
    for what, g, ref, bound in (("partial", partial[:B, :3], r.partial, pb), ("loss_out", out[:4], r.out, ob),
                                ("dpred", dpred[:B * T], r.dpred, db)):
        ratio, ok = L.judge(g, ref, bound)
        record(c["name"] + tag, what, ratio)
        if not ok:
            bad.append((what, ratio))
    assert not bad, (c["name"], bad)
    return pb, ob, db


@pytest.mark.parametrize("c", W.CASES, ids=[c["name"] for c in W.CASES])
def test_loss_wide_parity(c, monkeypatch):
    p, y = L.case_inputs(c)
    r = L.loss_ref(p, y, c["B"], c["T"], c["F"], **L.case_kw(c))
    assert r.near.sum().item() == 0, "the inputs hold an element whose sign(z) f32 may flip"
    got, wide = run_kernel(c, p, y, monkeypatch)
    assert wide == 1, "loss_wide counted %d launches for one wide call" % wide
    check_frame(c, *got)
    judge_case(c, r, got)


@pytest.mark.parametrize("bf16", [False, True])
def test_whole_clip_and_chunked_kernels_agree_at_T128(bf16, monkeypatch):
    """T = 128 fits the wide whole-clip kernel; NSTL_LOSS_CHUNKED=1 takes the chunked one
    (126 + 2 frames).  Each against f64, and with each other per element under the sum
    of their two bounds."""
    whole = W.case("T128-whole", 3, 128, 68, bf16=bf16, ldd=128, gs=3.0, zp=(124,), zt=(126,))
    forced = dict(whole, name="T128-chunk", chunked=True, force=True)
    p, y = L.case_inputs(whole, seed=1)
    r = L.loss_ref(p, y, 3, 128, 68, **L.case_kw(whole))
    assert r.near.sum().item() == 0
    (g0, n0), (g1, n1) = run_kernel(whole, p, y, monkeypatch), run_kernel(forced, p, y, monkeypatch)
    assert n0 == 1 and n1 == 1
    check_frame(whole, *g0)
    check_frame(forced, *g1)
    tag = "-bf16" if bf16 else "-f32"
    b0, b1 = judge_case(whole, r, g0, tag), judge_case(forced, r, g1, tag)
    for what, x0, x1, bound in (("partial", g0[0][:3, :3], g1[0][:3, :3], b0[0] + b1[0]),
                                ("loss_out", g0[1][:4], g1[1][:4], b0[1] + b1[1]),
                                ("dpred", g0[2][:3 * 128], g1[2][:3 * 128], b0[2] + b1[2])):
        ratio, ok = L.judge(x0, x1, bound)
        record("T128-pair" + tag, what, ratio)
        assert ok, (what, ratio)


@pytest.mark.parametrize("name", ["clip17", "T257"])
def test_flag_changes_nothing_at_narrow_shapes(name, monkeypatch):
    """F <= 64 launches the same kernels with NSTL_LOSS_WIDE_OK set or not."""
    c = next(c for c in L.CASES if c["name"] == name)
    p, y = L.case_inputs(c)
    (g0, n0), (g1, n1) = run_kernel(c, p, y, monkeypatch, flags=0), run_kernel(c, p, y, monkeypatch)
    assert n0 == 0 and n1 == 0, "a narrow call counted as a wide launch"
    B, T = c["B"], c["T"]
    assert torch.equal(g0[0][:B, :3], g1[0][:B, :3]) and torch.equal(g0[1][:4], g1[1][:4])
    assert torch.equal(g0[2][:B * T].float(), g1[2][:B * T].float())
    check_frame(c, *g1)


@pytest.mark.parametrize("change,match", [
    (dict(F=129), "unsupported"), (dict(dpred_ld=64), "ld < F"), (dict(T=4097), "unsupported"),
])
def test_loss_wide_rejections(change, match):
    """Refused before any launch, with the flag set; the buffers would hold a call of
    these sizes anyway."""
    import neurosync_trainer_lite_amd._hip as K
    v = dict(dict(B=1, T=4, F=68, dpred_ld=136, delta=1.0), **change)
    x = torch.zeros(4100, 144, device=DEV)
    dpred, partial, out = torch.zeros(4100, 144, device=DEV), torch.zeros(2, 4, device=DEV), torch.zeros(5, device=DEV)
    a = K.LossArgs()
    a.B, a.T, a.F = v["B"], v["T"], v["F"]
    a.pred, a.pred_ld, a.trg, a.trg_ld = x.data_ptr(), 144, x.data_ptr(), 144
    a.delta, a.w1, a.w2, a.w3, a.grad_scale = v["delta"], 1.0, 1.0, 1.0, 1.0
    a.dpred, a.dpred_dtype, a.dpred_ld = dpred.data_ptr(), K.F32, v["dpred_ld"]
    a.partial, a.loss_out = partial.data_ptr(), out.data_ptr()
    a.flags = K.LOSS_WIDE_OK
    K.kernel_counts_reset()
    with pytest.raises(RuntimeError, match=match):
        K.loss_fwd_bwd(a)
    torch.cuda.synchronize()
    assert K.kernel_counts()["loss_wide"] == 0
    assert not dpred.any() and not partial.any() and not out.any()
