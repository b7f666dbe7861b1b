"""The fused loss on clips longer than 256 frames (the chunked kernel of
csrc/loss.hip: time chunks of 254 frames with one frame of halo) against
oracle.model_ref.loss_fn in float64.  T = 257 is one frame past one chunk's staging,
513 two whole chunks plus a chunk of 5 frames; bounds are
test_loss_full_batch_shape_and_scale's."""
import pytest
import torch

from oracle import model_ref

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
B, F = 3, 61


def rnd(*shape, dtype=torch.float32, scale=1.0, seed=0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g, dtype=torch.float64) * scale).to(dtype).to(DEV)


def f64(t):
    return t.detach().double().cpu()


def check(got, ref, rel, what):
    got, ref = f64(got), f64(ref)
    scale = ref.abs().max().item() + 1e-30
    err = (got - ref).abs().max().item()
    print("%s: max err %.3e vs scale %.3e (bound %.1e)" % (what, err, scale, rel))
    assert err <= rel * scale, "%s: max err %.3e vs scale %.3e (rel %.1e)" % (what, err, scale, rel)


def loss_and_grad(p0, t):
    from neurosync_trainer_lite_amd.utils.model import Loss
    p = p0.clone().requires_grad_(True)
    loss = Loss()(p, t)
    (loss * 3.0).backward()
    torch.cuda.synchronize()
    return loss.item(), p.grad


def against_oracle(p0, t, what):
    loss, grad = loss_and_grad(p0, t)
    pc = f64(p0).requires_grad_(True)
    lr = model_ref.loss_fn(pc, f64(t))
    (lr * 3.0).backward()
    print("%s: loss %.9g oracle %.9g" % (what, loss, lr.item()))
    assert abs(loss - lr.item()) < 1e-5 * abs(lr.item()), (what, loss, lr.item())
    check(grad, pc.grad, 1e-4, "loss grad " + what)


@pytest.mark.parametrize("T", [257, 288, 513, 1000])
def test_long_loss_matches_oracle(T):
    against_oracle(rnd(B, T, F, scale=30, seed=50), rnd(B, T, F, scale=30, seed=51), "T=%d" % T)


def test_long_loss_zero_difference_run_across_chunk_edge():
    """pred constant over frames 255..257: the steps 255 and 256 have |dp| = 0 (the
    cosine gradient's `np > 0` branch), on either side of the second chunk's first
    owned frame (254) + halo."""
    T = 513
    p = rnd(B, T, F, scale=30, seed=52)
    p[:, 255:258] = p[:, 255:256].clone()
    against_oracle(p, rnd(B, T, F, scale=30, seed=53), "zero-difference run")
    # and a run that straddles the chunk edge itself (frames 253..255; chunk 1 owns 254..)
    p = rnd(B, T, F, scale=30, seed=54)
    p[:, 253:256] = p[:, 253:254].clone()
    against_oracle(p, rnd(B, T, F, scale=30, seed=55), "zero-difference run at the edge")


def test_chunked_kernel_agrees_with_whole_clip_kernel(monkeypatch):
    """T = 256 fits the whole-clip kernel; NSTL_LOSS_CHUNKED=1 forces the chunked one
    (254 + 2 frames).  Same formulas, another summation order: 1e-6."""
    T = 256
    p, t = rnd(B, T, F, scale=30, seed=56), rnd(B, T, F, scale=30, seed=57)
    l0, g0 = loss_and_grad(p, t)
    monkeypatch.setenv("NSTL_LOSS_CHUNKED", "1")
    l1, g1 = loss_and_grad(p, t)
    print("whole %.9g chunked %.9g" % (l0, l1))
    assert abs(l1 - l0) < 1e-6 * abs(l0), (l0, l1)
    check(g1, g0, 1e-6, "chunked vs whole-clip gradient")
    assert not torch.equal(g0, torch.zeros_like(g0))


def test_loss_rejects_past_4096():
    from neurosync_trainer_lite_amd.utils.model import Loss
    with pytest.raises(RuntimeError, match="unsupported"):
        Loss()(rnd(1, 4097, F), rnd(1, 4097, F))
