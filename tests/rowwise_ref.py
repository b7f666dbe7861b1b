"""TEST INFRA: float64 references of the row-wise kernels (csrc/norm.hip,
csrc/optim.hip), with no GPU dependency.  tests/test_rowwise_ref.py proves them
against torch and the CPU oracle; tests/test_rowwise_parity_gpu.py judges the
kernels by them.  Never imported by the package."""
import math

import numpy as np
import torch


def keep_pattern(seed, rows, cols, p):
    """Keep decision of element (i, j) of a [rows][cols] tensor under common.h's
    dropout hash: nstl_fmix32(pair ^ seed_term) with pair = i * cols/2 + j/2, low /
    high 16 bits against the threshold.  Returns a numpy bool array."""
    seed_term = (seed & 0xFFFFFFFF) ^ (((seed >> 32) * 0x27D4EB2F) & 0xFFFFFFFF)
    thresh = int(p * 65536.0 + 0.5)
    pair = (np.arange(rows, dtype=np.uint64)[:, None] * (cols // 2) + np.arange(cols // 2, dtype=np.uint64)[None, :])
    h = (pair.astype(np.uint32) ^ np.uint32(seed_term)).astype(np.uint64)
    h ^= h >> 16
    h = (h * 0x85EBCA6B) & 0xFFFFFFFF
    h ^= h >> 13
    h = (h * 0xC2B2AE35) & 0xFFFFFFFF
    h ^= h >> 16
    keep = np.empty((rows, cols), dtype=bool)
    keep[:, 0::2] = (h & 0xFFFF) >= thresh
    keep[:, 1::2] = (h >> 16) >= thresh
    return keep


def _f64(t):
    return torch.as_tensor(t).detach().to("cpu", torch.float64)


def branch_mask(rows, D, n_masks, p, seeds):
    """keep1 & keep2 (bool [rows][D]) and the scale 1/(1-p)^n of the LayerNorm
    tail's stacked dropout masks; no dropout (all kept, scale 1) when n_masks = 0
    or p = 0."""
    keep = torch.ones(rows, D, dtype=torch.bool)
    if n_masks <= 0 or p <= 0.0:
        return keep, 1.0
    for k in range(n_masks):
        keep &= torch.from_numpy(keep_pattern(seeds[k], rows, D, p))
    return keep, (1.0 / (1.0 - p)) ** n_masks


def ln_fwd_ref(x, y, gamma, beta, eps, n_masks=0, p=0.0, seeds=(0, 0)):
    """s = x + y * keep1 * keep2 / (1-p)^n (x may be None); out = LayerNorm(s).
    Element (row, col) takes pair index row * D/2 + col/2; the statistics come from
    the unrounded s.  Returns s, out, mean, rstd in f64."""
    y = _f64(y)
    rows, D = y.shape
    keep, scale = branch_mask(rows, D, n_masks, p, seeds)
    s = y * keep.double() * scale
    if x is not None:
        s = s + _f64(x)
    mean = s.mean(1)
    var = ((s - mean[:, None]) ** 2).mean(1)
    rstd = 1.0 / torch.sqrt(var + eps)
    out = (s - mean[:, None]) * rstd[:, None] * _f64(gamma) + _f64(beta)
    return s, out, mean, rstd


def ln_bwd_ref(s_stored, mean, rstd, g, gamma):
    """norm.hip's backward from the stored s and the given row statistics:
    xhat = (s - mean) * rstd;
    ds = rstd * (g*gamma - mean(g*gamma) - xhat * mean(g*gamma*xhat));
    dgamma = sum_rows g * xhat; dbeta = sum_rows g.  Returns ds, dgamma, dbeta."""
    s, g, gamma = _f64(s_stored), _f64(g), _f64(gamma)
    mean, rstd = _f64(mean)[:, None], _f64(rstd)[:, None]
    xhat = (s - mean) * rstd
    gg = g * gamma
    ds = rstd * (gg - gg.mean(1, keepdim=True) - xhat * (gg * xhat).mean(1, keepdim=True))
    return ds, (g * xhat).sum(0), g.sum(0)


def rope_ref(x, cos, sin, T, rope_dim, inverse=False):
    """Pair rotation of a [rows][cols] matrix: element pair (2i, 2i+1) of row r turns
    by the angle of position t = r % T and table pair (col % rope_dim) / 2 (cos / sin
    [T][rope_dim/2]); inverse turns the other way."""
    x, cos, sin = _f64(x), _f64(cos), _f64(sin)
    rows, cols = x.shape
    t = torch.arange(rows) % T
    pr = (torch.arange(0, cols, 2) % rope_dim) // 2
    c, s = cos[t][:, pr], sin[t][:, pr]
    if inverse:
        s = -s
    e, o = x[:, 0::2], x[:, 1::2]
    out = torch.empty_like(x)
    out[:, 0::2] = e * c - o * s
    out[:, 1::2] = e * s + o * c
    return out


def adam_ref(p, g, m, v, step, lr, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0, coef=1.0):
    """One Adam step with coupled L2 on the clipped gradient g * coef: torch's lerp
    form for m, bias corrections in double.  Returns the new p, m, v (f64; the
    inputs are left alone)."""
    p, g, m, v = _f64(p), _f64(g), _f64(m), _f64(v)
    bc1 = 1.0 - beta1 ** step
    bc2_sqrt = math.sqrt(1.0 - beta2 ** step)
    gc = g * coef + weight_decay * p
    m = m + (1.0 - beta1) * (gc - m)
    v = v * beta2 + (1.0 - beta2) * gc * gc
    denom = v.sqrt() / bc2_sqrt + eps
    return p - (lr / bc1) * m / denom, m, v


def clip_ref(partials, max_norm):
    """clip_grad_norm_ from sum-of-squares partials: norm = sqrt(sum), coef =
    min(1, max_norm / (norm + 1e-6)).  Returns norm, coef as python floats."""
    norm = math.sqrt(_f64(partials).sum().item())
    return norm, min(1.0, max_norm / (norm + 1e-6))
