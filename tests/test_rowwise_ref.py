"""The float64 references of tests/rowwise_ref.py against torch and the CPU oracle,
before any kernel is judged by them (tests/test_rowwise_parity_gpu.py)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import model_ref
from tests import rowwise_ref as R


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g, dtype=torch.float64) * scale


@pytest.mark.parametrize("D", [128, 1024])
def test_ln_bwd_ref_matches_autograd(D):
    """With exact f64 statistics, ln_bwd_ref is the f64 autograd of F.layer_norm."""
    rows, eps = 19, 1e-5
    s = rnd(rows, D, seed=1).requires_grad_(True)
    gamma = (1 + 0.1 * rnd(D, seed=2)).requires_grad_(True)
    beta = (0.1 * rnd(D, seed=3)).requires_grad_(True)
    g = rnd(rows, D, seed=4)
    F.layer_norm(s, (D,), gamma, beta, eps).backward(g)
    sd = s.detach()
    mean = sd.mean(1)
    rstd = 1.0 / torch.sqrt(sd.var(1, unbiased=False) + eps)
    ds, dgamma, dbeta = R.ln_bwd_ref(sd, mean, rstd, g, gamma.detach())
    for got, ref, what in ((ds, s.grad, "ds"), (dgamma, gamma.grad, "dgamma"), (dbeta, beta.grad, "dbeta")):
        assert (got - ref).abs().max().item() <= 1e-10, what


@pytest.mark.parametrize("with_x", [True, False])
def test_ln_fwd_ref_matches_layer_norm(with_x):
    rows, D, eps = 7, 256, 1e-5
    x, y = rnd(rows, D, seed=5), rnd(rows, D, seed=6)
    gamma, beta = 1 + 0.1 * rnd(D, seed=7), 0.1 * rnd(D, seed=8)
    inp = x + y if with_x else y
    # p > 0 with no masks is no dropout either
    for n_masks, p in ((0, 0.0), (2, 0.0), (0, 0.3)):
        s, out, mean, rstd = R.ln_fwd_ref(x if with_x else None, y, gamma, beta, eps, n_masks, p, (11, 22))
        assert torch.equal(s, inp)
        assert (out - F.layer_norm(inp, (D,), gamma, beta, eps)).abs().max().item() <= 1e-12
        assert (mean - inp.mean(1)).abs().max().item() <= 1e-14
        assert (rstd - 1.0 / torch.sqrt(inp.var(1, unbiased=False) + eps)).abs().max().item() <= 1e-12


def test_ln_fwd_ref_dropout_is_the_hash_mask():
    rows, D, p = 6, 128, 0.3
    seeds = ((3 << 32) + 17, (9 << 32) + 5)
    y = torch.ones(rows, D, dtype=torch.float64)
    g, b = torch.ones(D, dtype=torch.float64), torch.zeros(D, dtype=torch.float64)
    k1 = torch.from_numpy(R.keep_pattern(seeds[0], rows, D, p))
    k2 = torch.from_numpy(R.keep_pattern(seeds[1], rows, D, p))
    s1 = R.ln_fwd_ref(None, y, g, b, 1e-5, 1, p, seeds)[0]
    s2 = R.ln_fwd_ref(None, y, g, b, 1e-5, 2, p, seeds)[0]
    assert torch.equal(s1, k1.double() / (1 - p))
    assert torch.equal(s2, (k1 & k2).double() * (1.0 / (1.0 - p)) ** 2)


def test_keep_pattern_rate_and_seed():
    p = 0.3
    a = R.keep_pattern((5 << 32) + 1, 64, 1024, p)
    b = R.keep_pattern((6 << 32) + 1, 64, 1024, p)
    assert a.shape == (64, 1024) and a.dtype == np.bool_
    assert abs(a.mean() - (1 - p)) < 0.01, a.mean()
    assert abs(b.mean() - (1 - p)) < 0.01, b.mean()
    assert (a != b).any()
    # independent seeds agree where both keep or both drop
    assert abs((a == b).mean() - ((1 - p) ** 2 + p ** 2)) < 0.01


def test_adam_ref_matches_oracle_three_steps():
    n = 1000
    p, m, v = rnd(n, seed=10), torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
    po, mo, vo = p.clone(), m.clone(), v.clone()
    for step in range(1, 4):
        g = rnd(n, seed=10 + step, scale=0.01)
        p, m, v = R.adam_ref(p, g, m, v, step, 1e-3, 0.9, 0.999, 1e-8, 1e-2, coef=0.25)
        model_ref.adam_l2_step([po], [g * 0.25], [mo], [vo], step, 1e-3, 0.9, 0.999, 1e-8, 1e-2)
        torch.testing.assert_close(p, po, rtol=1e-13, atol=1e-15)
        torch.testing.assert_close(m, mo, rtol=1e-13, atol=1e-18)
        torch.testing.assert_close(v, vo, rtol=1e-13, atol=1e-20)
    # no weight decay, unclipped
    p2, m2, v2 = R.adam_ref(p, g, m, v, 4, 1e-3)
    model_ref.adam_l2_step([po], [g], [mo], [vo], 4, 1e-3)
    torch.testing.assert_close(p2, po, rtol=1e-13, atol=1e-15)


def test_clip_ref_matches_oracle():
    g = [rnd(100, seed=20), rnd(37, seed=21)]
    parts = torch.stack([(t * t).sum() for t in g])
    for max_norm in (2.0, 1e3):
        norm, coef = R.clip_ref(parts, max_norm)
        gs = [t.clone() for t in g]
        total = model_ref.clip_grad_norm(gs, max_norm).item()
        assert abs(norm - total) <= 1e-12 * total
        assert abs((gs[0] / g[0]).mean().item() - coef) <= 1e-12
    assert R.clip_ref(parts, 1e3)[1] == 1.0


@pytest.mark.parametrize("cols,rope_dim", [(128, 128), (192, 64)])
def test_rope_ref_inverse_undoes_forward(cols, rope_dim):
    T, rows = 7, 17
    cos, sin = model_ref.rotation_tables(T, rope_dim)
    x = rnd(rows, cols, seed=30)
    r = R.rope_ref(x, cos, sin, T, rope_dim)
    assert (r - x).abs().max().item() > 0.1  # it does rotate
    back = R.rope_ref(r, cos, sin, T, rope_dim, inverse=True)
    # the f32 tables' cos^2 + sin^2 is 1 to f32 rounding only
    assert (back - x).abs().max().item() <= 1e-6


def test_rope_ref_matches_oracle_rotation():
    T, D = 5, 8
    cos, sin = model_ref.rotation_tables(T, D)
    x = rnd(T, D, seed=31)
    ref = model_ref.rotate_pairs(x, cos, sin)
    assert (R.rope_ref(x, cos, sin, T, D) - ref).abs().max().item() <= 1e-15
    # two windows stacked: position = row % T; three heads side by side: pair = (col % D) / 2
    x2 = torch.cat([torch.cat([x, 2 * x, 3 * x], 1)] * 2, 0)
    ref2 = torch.cat([torch.cat([ref, 2 * ref, 3 * ref], 1)] * 2, 0)
    assert (R.rope_ref(x2, cos, sin, T, D) - ref2).abs().max().item() <= 1e-14
