"""CPU proof of tests/loss_wide_ref.py: loss_ref.loss_ref at F = 68 and F = 128 against
f64 autograd of oracle.model_ref.loss_fn; the f32 emulation of the wide kernels stays
under the recounted bounds at every shape the GPU file runs; five wrong kernels each
exceed the same bounds on at least one of those shapes."""
import pytest
import torch

from oracle import model_ref
from tests import loss_ref as L
from tests import loss_wide_ref as W


def autograd(p, y, B, T, F, delta, w, gs):
    pc = L.window(p, B, T, F).requires_grad_(True)
    loss = model_ref.loss_fn(pc, L.window(y, B, T, F), L.G.f32v(delta), *(L.G.f32v(v) for v in w))
    (loss * gs).backward()
    return loss.item(), pc.grad.reshape(B * T, F)


def rel(got, ref):
    return (got - ref).abs().max().item() / (ref.abs().max().item() + 1e-300)


@pytest.mark.parametrize("F", [68, 128])
@pytest.mark.parametrize("w,delta,scale", [((1.0, 1.0, 1.0), 1.0, 30.0), ((0.3, 0.5, 2.0), 0.25, 0.3),
                                           ((0.0, 0.0, 1.0), 1.0, 0.3), ((1.0, 0.0, 0.0), 0.25, 30.0)])
def test_restatement_matches_f64_autograd_wide(F, w, delta, scale):
    B, T = 3, 19
    p, y = L.make_inputs(B, T, F, scale, 1, F + 3, F + 5, zero_pred=(0, 6, 17), zero_trg=(6, 9))
    r = L.loss_ref(p, y, B, T, F, delta=delta, w1=w[0], w2=w[1], w3=w[2], grad_scale=3.0, dpred_ld=136)
    loss, grad = autograd(p, y, B, T, F, delta, w, 3.0)
    assert abs(r.out[0].item() - loss) <= 1e-12 * abs(loss)
    assert rel(r.dpred[:, :F], grad) <= 1e-12
    assert torch.equal(r.dpred[:, F:], torch.zeros(B * T, 136 - F, dtype=torch.float64))
    assert (r.dpred_mag >= r.dpred.abs() * (1 - 1e-12)).all()


def test_sum_roundings_counts():
    # whole clip: ceil(T ldd / 1024) elements per thread, ceil((T-1)/16) steps per wave
    assert W.sum_roundings(128, 128, False) == (3 + 16 + 22, 3 + 16 + 22, 30 + 8 + 22)
    assert W.sum_roundings(2, 68, False) == (26, 26, 53)
    # chunked: per chunk; T = 129 is 126 + 3 frames, staged steps 126 and 3
    assert W.chunks(129) == [(0, 126, 0, 127), (126, 129, 125, 129)]
    assert W.sum_roundings(129, 68, True) == (3 + 9 + 1 + 22, 3 + 9 + 1 + 22, 30 + 8 + 1 + 22)
    assert [c[:2] for c in W.chunks(252)] == [(0, 126), (126, 252)]
    assert len(W.chunks(253)) == 3 and len(W.chunks(379)) == 4
    # no chunk stages more rows than the tile holds
    assert max(hi - lo for T in (127, 128, 129, 379, 4096) for t0, t1, lo, hi in W.chunks(T)) == W.TMAX
    # the derived gradient figure (module docstring) stays under E32
    assert 49 * W.U32 < W.E32
    assert all(c["chunked"] == (c["T"] > W.TMAX or c["force"]) for c in W.CASES)


def run_case(c, **emu):
    B, T, F = c["B"], c["T"], c["F"]
    p, y = L.case_inputs(c)
    r = L.loss_ref(p, y, B, T, F, **L.case_kw(c))
    got = W.loss_emulate(p, y, B, T, F, chunked=c["chunked"], bf16=c["bf16"], **L.case_kw(c), **emu)
    bnd = W.bounds(r, c["chunked"], torch.bfloat16 if c["bf16"] else torch.float32)
    return r, got, bnd


def verdicts(c, **emu):
    """{output: (worst err/bound, within)} of one emulated case."""
    r, (partial, out, dpred), (pb, ob, db) = run_case(c, **emu)
    res = {"near": r.near.sum().item()}
    for what, got, ref, bound in (("partial", partial, r.partial, pb), ("loss_out", out, r.out, ob),
                                  ("dpred", dpred, r.dpred, db)):
        res[what] = L.judge(got, ref, bound)
    res["pad"] = torch.equal(dpred[:, c["F"]:].float(), torch.zeros(c["B"] * c["T"], c["ldd"] - c["F"]))
    return res


@pytest.mark.parametrize("c", W.CASES, ids=[c["name"] for c in W.CASES])
def test_f32_emulation_within_bounds(c):
    v = verdicts(c)
    assert v["near"] == 0, "the inputs hold an element whose sign(z) f32 may flip"
    for what in ("partial", "loss_out", "dpred"):
        ratio, ok = v[what]
        print("%s %s: worst err/bound %.3f" % (c["name"], what, ratio))
        assert ok, (c["name"], what, ratio)
    assert v["pad"]


BY_NAME = {c["name"]: c for c in W.CASES}


# wrong kernel -> (the cases it is tried on, the outputs that must leave their bounds there)
@pytest.mark.parametrize("defect,names,outputs", [
    (dict(cols64=True), ("one-step-68", "F65", "F128", "T128-68"), ("partial", "loss_out", "dpred")),
    (dict(double_halo=True), ("chunked127", "chunked128", "T253-F65"), ("partial", "loss_out")),
    (dict(stride254=True), ("chunked127", "T129", "T253-F65", "T379"), ("partial", "loss_out", "dpred")),
    (dict(norm64=True), ("one-step-68", "F65", "F128", "T129"), ("dpred",)),
    (dict(pad_value=1e-30), ("clip17-68", "F65", "F128", "T129"), ("dpred",)),
], ids=["cols64", "double_halo", "stride254", "norm64", "pad_value"])
def test_wrong_kernels_exceed_bounds(defect, names, outputs):
    caught = []
    for name in names:
        v = verdicts(BY_NAME[name], **defect)
        out = [w for w in outputs if not v[w][1]]
        print("%s on %s: %s" % (list(defect)[0], name, {w: "%.3g" % v[w][0] for w in outputs}))
        if out:
            caught.append((name, out))
    assert caught, "no case catches %s" % defect


def test_defects_show_where_they_should():
    """The sharper statements behind the table above."""
    # a halo step counted twice moves the cosine sum of every sequence and leaves the rest alone
    c = BY_NAME["T253-F65"]
    r, (partial, out, dpred), (pb, ob, db) = run_case(c, double_halo=True)
    assert ((partial[:, 2].double() - r.partial[:, 2]).abs() > pb[:, 2]).all() and not L.judge(out[3], r.out[3], ob[3])[1]
    assert L.judge(partial[:, :2], r.partial[:, :2], pb[:, :2])[1] and L.judge(dpred, r.dpred, db)[1]
    # T129's edge step is a zero step (cos = 0): the same defect hides there, which is why
    # the live edges of the other cases are needed
    assert verdicts(BY_NAME["T129"], double_halo=True)["partial"][1]
    # columns 64.. left out of the step sums: F = 65 drops one of 65 columns and is still caught
    v = verdicts(BY_NAME["F65"], cols64=True)
    assert not v["partial"][1] and not v["dpred"][1]
    # 64 in place of F in the normalisers touches the gradient only
    v = verdicts(BY_NAME["F128"], norm64=True)
    assert v["partial"][1] and v["loss_out"][1] and not v["dpred"][1]
    # a pad column that is not an exact zero has a zero bound
    v = verdicts(BY_NAME["F65"], pad_value=1e-30)
    assert not v["pad"] and not v["dpred"][1] and v["partial"][1] and v["loss_out"][1]
