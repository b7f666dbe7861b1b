"""CPU proof of tests/loss_ref.py: the restatement against f64 autograd of
oracle.model_ref.loss_fn (total and gradient, 1e-12 relative); an f32 emulation of
csrc/loss.hip's arithmetic stays under the derived bounds at every shape the GPU
file runs; a chunked kernel that counted the halo step of every chunk edge twice
exceeds them."""
import pytest
import torch

from oracle import model_ref
from tests import loss_ref as L

WEIGHTS = [(1.0, 1.0, 1.0), (0.0, 0.0, 1.0), (1.0, 0.0, 0.0), (0.3, 0.5, 2.0)]


def autograd(p, y, B, T, F, delta, w, gs):
    pc = L.window(p, B, T, F).requires_grad_(True)
    loss = model_ref.loss_fn(pc, L.window(y, B, T, F), L.G.f32v(delta), *(L.G.f32v(v) for v in w))
    (loss * gs).backward()
    return loss.item(), pc.grad.reshape(B * T, F)


def rel(got, ref):
    return (got - ref).abs().max().item() / (ref.abs().max().item() + 1e-300)


@pytest.mark.parametrize("scale", [30.0, 0.3])
@pytest.mark.parametrize("w", WEIGHTS)
@pytest.mark.parametrize("delta", [1.0, 0.25])
def test_restatement_matches_f64_autograd(scale, w, delta):
    B, T, F = 3, 19, 61
    p, y = L.make_inputs(B, T, F, scale, 1, F + 3, F + 5, zero_pred=(0, 6, 17), zero_trg=(6, 9))
    r = L.loss_ref(p, y, B, T, F, delta=delta, w1=w[0], w2=w[1], w3=w[2], grad_scale=3.0, dpred_ld=72)
    loss, grad = autograd(p, y, B, T, F, delta, w, 3.0)
    assert abs(r.out[0].item() - loss) <= 1e-12 * abs(loss)
    assert rel(r.dpred[:, :F], grad) <= 1e-12
    assert torch.equal(r.dpred[:, F:], torch.zeros(B * T, 72 - F, dtype=torch.float64))
    assert (r.dpred_mag >= r.dpred.abs() * (1 - 1e-12)).all()
    # the parts: loss_out[1..3] and the per-sequence sums add up to them
    w1, w2, w3 = (L.G.f32v(v) for v in w)
    assert abs(w1 * r.out[1] + w2 * r.out[2] + w3 * r.out[3] - r.out[0]) <= 1e-14 * r.out_mag[0]
    assert abs(r.partial[:, 2].sum() / (B * (T - 1)) - (1 - r.out[3])) <= 1e-14


def test_restatement_T2_and_F1():
    for B, T, F in ((2, 2, 61), (2, 33, 1)):
        p, y = L.make_inputs(B, T, F, 30.0, 2)
        r = L.loss_ref(p, y, B, T, F)
        loss, grad = autograd(p, y, B, T, F, 1.0, (1.0, 1.0, 1.0), 1.0)
        assert abs(r.out[0].item() - loss) <= 1e-12 * abs(loss)
        assert rel(r.dpred, grad) <= 1e-12
    # F = 1: every cos_t is +-1 up to eps
    assert ((r.partial_mag[:, 2] - (T - 1)).abs() < 1e-6).all()


def test_sum_roundings_counts():
    # whole clip: ceil(T ldd / 1024) elements per thread, ceil((T-1)/16) steps per wave
    assert L.sum_roundings(256, 72, False) == (3 + 18 + 22, 3 + 18 + 22, 29 + 16 + 22)
    assert L.sum_roundings(2, 61, False) == (26, 26, 52)
    # chunked: per chunk; T = 257 is 254 + 3 frames, staged steps 254 and 3
    assert L.chunks(257) == [(0, 254, 0, 255), (254, 257, 253, 257)]
    assert L.sum_roundings(257, 61, True) == (3 + 16 + 1 + 22, 3 + 16 + 1 + 22, 29 + 16 + 1 + 22)
    assert [c[:2] for c in L.chunks(508)] == [(0, 254), (254, 508)]
    assert len(L.chunks(509)) == 3 and len(L.chunks(763)) == 4


def run_case(c, **emu):
    B, T, F = c["B"], c["T"], c["F"]
    p, y = L.case_inputs(c)
    r = L.loss_ref(p, y, B, T, F, **L.case_kw(c))
    got = L.loss_emulate(p, y, B, T, F, chunked=c["chunked"], bf16=c["bf16"], **L.case_kw(c), **emu)
    bnd = L.bounds(r, c["chunked"], torch.bfloat16 if c["bf16"] else torch.float32)
    return r, got, bnd


@pytest.mark.parametrize("c", L.CASES, ids=[c["name"] for c in L.CASES])
def test_f32_emulation_within_bounds(c):
    r, (partial, out, dpred), (pb, ob, db) = run_case(c)
    assert r.near.sum().item() == 0, "the inputs hold an element whose sign(z) f32 may flip"
    for what, got, ref, bound in (("partial", partial, r.partial, pb), ("loss_out", out, r.out, ob),
                                  ("dpred", dpred, r.dpred, db)):
        ratio, ok = L.judge(got, ref, bound)
        print("%s %s: worst err/bound %.3f" % (c["name"], what, ratio))
        assert ok, (c["name"], what, ratio)
    assert torch.equal(dpred[:, c["F"]:].float(), torch.zeros(c["B"] * c["T"], c["ldd"] - c["F"]))


@pytest.mark.parametrize("T", [257, 513, 1000])
def test_double_counted_halo_step_exceeds_bounds(T):
    c = L.case("halo", 3, T, 61)
    r, (partial, out, dpred), (pb, ob, db) = run_case(c, double_halo=True)
    ratio, ok = L.judge(partial[:, 2], r.partial[:, 2], pb[:, 2])
    print("T=%d partial[:, 2] err/bound %.1f" % (T, ratio))
    assert not ok and ((partial[:, 2].double() - r.partial[:, 2]).abs() > pb[:, 2]).all()
    ratio, ok = L.judge(out[3], r.out[3], ob[3])
    print("T=%d loss_out[3] err/bound %.1f" % (T, ratio))
    assert not ok
    # everything the defect does not touch stays within bound
    assert L.judge(partial[:, :2], r.partial[:, :2], pb[:, :2])[1] and L.judge(dpred, r.dpred, db)[1]
