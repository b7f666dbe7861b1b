"""The float64 GEMM reference of tests/gemm_ref.py against torch autograd,
rowwise_ref and a scalar port of the dropout hash, before any kernel is judged by
it (tests/test_gemm_parity_gpu.py)."""
import numpy as np
import pytest
import torch

from oracle import model_ref
from tests import gemm_ref as G
from tests import rowwise_ref as R

SEED = (0x9E3779B9 << 32) | 0x01234567  # nonzero high word


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g, dtype=torch.float64) * scale


def fmix32(h):
    h ^= h >> 16
    h = (h * 0x85EBCA6B) & 0xFFFFFFFF
    h ^= h >> 13
    h = (h * 0xC2B2AE35) & 0xFFFFFFFF
    return h ^ (h >> 16)


def nstl_keep(seed, idx, thresh):
    """Scalar port of common.h nstl_pair_hash / nstl_keep."""
    hi = (idx >> 33) & 0xFFFFFFFF
    s = (seed & 0xFFFFFFFF) ^ (((seed >> 32) * 0x27D4EB2F) & 0xFFFFFFFF) ^ (((hi << 17) | (hi >> 15)) & 0xFFFFFFFF)
    h = fmix32(((idx >> 1) & 0xFFFFFFFF) ^ s)
    return ((h >> 16) if idx & 1 else (h & 0xFFFF)) >= thresh


@pytest.mark.parametrize("M,N", [(5, 72), (33, 1000), (7, 2)])
def test_keep_flat_equals_keep_pattern_for_even_n(M, N):
    for seed, p in ((SEED, 0.3), (77, 0.5), (SEED, 0.0)):
        assert np.array_equal(G.keep_flat(seed, M, N, p), R.keep_pattern(seed, M, N, p)), (seed, p)


@pytest.mark.parametrize("M,N", [(9, 61), (4, 999), (6, 1)])
def test_keep_flat_odd_n_equals_scalar_port(M, N):
    p = 0.3
    thresh = G.drop_thresh(p)
    assert thresh == 19661
    got = G.keep_flat(SEED, M, N, p)
    assert got.shape == (M, N) and got.dtype == np.bool_
    want = np.array([[nstl_keep(SEED, i * N + j, thresh) for j in range(N)] for i in range(M)])
    assert np.array_equal(got, want)


def test_relu_dropout_forward_and_drelu_backward_match_autograd():
    """ffn(x) = mask * relu(x W^T + b) / (1 - p): the forward is the BIAS_RELU_DROP
    reference, its input gradient the DRELU_DROP reference (dh = (g W2) (h > 0) /
    (1 - p) with h the saved forward output) times W."""
    M, N, Kd, p = 11, 61, 24, 0.3
    x = rnd(M, Kd, seed=1).requires_grad_(True)
    W, b = rnd(N, Kd, seed=2), rnd(N, seed=3)
    mask = torch.from_numpy(G.keep_flat(SEED, M, N, p)).double()
    pre = x @ W.T + b
    h = mask * torch.relu(pre) * G.inv_keep(p)
    ref, mag = G.gemm_ref(x.detach(), W, M, N, Kd, epilogue=G.EPI_BIAS_RELU_DROP, bias=b, p_drop=p, seed=SEED)
    assert (ref - h.detach()).abs().max().item() <= 1e-13
    assert (mag >= ref.abs()).all()
    assert ((ref == 0) == ((mask == 0) | (pre.detach() <= 0))).all()
    # backward: the gradient wrt the pre-activation, from dY [M][K2] and W2 [K2][N] (TN)
    K2 = 13
    dY, W2 = rnd(M, K2, seed=4), rnd(K2, N, seed=5)
    g = dY @ W2
    (dpre,) = torch.autograd.grad(h, pre, g)
    dref, dmag = G.gemm_ref(dY, W2, M, N, K2, a_kmajor=True, b_kmajor=False, epilogue=G.EPI_DRELU_DROP,
                            aux=h.detach(), p_drop=p)
    assert (dref - dpre).abs().max().item() <= 1e-13
    assert (dmag >= dref.abs()).all()


def test_rope_branch_is_rope_ref_of_the_plain_product():
    M, N, Kd, T, dim, rc = 50, 72, 16, 25, 24, 48
    A, B, b = rnd(M, Kd, seed=6), rnd(N, Kd, seed=7), rnd(N, seed=8)
    cos, sin = model_ref.rotation_tables(T, dim)
    ref, mag = G.gemm_ref(A, B, M, N, Kd, epilogue=G.EPI_BIAS_ROPE, bias=b, rope=(cos, sin, T, dim), rope_cols=rc)
    z = A @ B.T + b
    want = z.clone()
    want[:, :rc] = R.rope_ref(z[:, :rc], cos, sin, T, dim)
    assert torch.equal(ref, want)
    assert torch.equal(ref[:, rc:], z[:, rc:]) and (ref[:, :rc] - z[:, :rc]).abs().max().item() > 0.1
    assert (mag >= ref.abs()).all()
    # the magnitude goes through the rotation with |cos|, |sin|
    zm = A.abs() @ B.abs().T + b.abs()
    t, pr = torch.arange(M) % T, (torch.arange(0, rc, 2) % dim) // 2
    c, s = cos.double().abs()[t][:, pr], sin.double().abs()[t][:, pr]
    assert (mag[:, 0:rc:2] - (zm[:, 0:rc:2] * c + zm[:, 1:rc:2] * s)).abs().max().item() <= 1e-12
    assert (mag[:, 1:rc:2] - (zm[:, 0:rc:2] * s + zm[:, 1:rc:2] * c)).abs().max().item() <= 1e-12
    assert torch.equal(mag[:, rc:], zm[:, rc:])


@pytest.mark.parametrize("akm,bkm", [(True, True), (True, False), (False, False), (False, True)])
def test_alpha_bias_beta_order_and_layouts(akm, bkm):
    """alpha scales the product only, the bias is added unscaled, beta C0 last; the
    operands are read as stored in each layout, padding columns cut off."""
    M, N, Kd, alpha, beta = 7, 9, 5, 0.5, 0.75
    A, B, b, C0 = rnd(M, Kd, seed=9), rnd(N, Kd, seed=10), rnd(N, seed=11), rnd(M + 2, N + 3, seed=12)
    pad = lambda X: torch.cat([X, torch.full((X.shape[0], 3), float("nan"), dtype=X.dtype)], 1)
    As, Bs = pad(A if akm else A.T.contiguous()), pad(B if bkm else B.T.contiguous())
    ref, mag = G.gemm_ref(As, Bs, M, N, Kd, a_kmajor=akm, b_kmajor=bkm, alpha=alpha, beta=beta, C0=C0,
                          epilogue=G.EPI_BIAS, bias=b)
    acc = A @ B.T
    want = alpha * acc + b + beta * C0[:M, :N]
    assert (ref - want).abs().max().item() <= 1e-14
    wmag = alpha * (A.abs() @ B.abs().T) + b.abs() + (beta * C0[:M, :N]).abs()
    assert (mag - wmag).abs().max().item() <= 1e-14
    assert (mag >= ref.abs()).all()
    # NONE ignores a bias, DRELU_DROP too
    ref0, _ = G.gemm_ref(As, Bs, M, N, Kd, a_kmajor=akm, b_kmajor=bkm, alpha=alpha, bias=b)
    assert (ref0 - alpha * acc).abs().max().item() <= 1e-14


def test_bound_formulas():
    ref, mag = torch.tensor([2.0, -3.0], dtype=torch.float64), torch.tensor([4.0, 8.0], dtype=torch.float64)
    assert torch.equal(G.bound(ref, mag, torch.float32), 1e-5 * mag)
    want = 2.0 ** -8 * ref.abs() + (1 + 2.0 ** -8) * 1e-5 * mag
    assert torch.equal(G.bound(ref, mag, torch.bfloat16), want)
    # one bf16 rounding of an exact value stays inside it; a value one ulp off does not
    x = torch.tensor([1.00390625 + 2.0 ** -9], dtype=torch.float64)  # halfway between two bf16 values
    got = x.float().bfloat16().double()
    assert ((got - x).abs() <= G.bound(x, x.abs(), torch.bfloat16)).all()
    assert ((got + 2.0 ** -7 - x).abs() > G.bound(x, x.abs(), torch.bfloat16)).all()


def test_fp8_call_matches_oracle_fp8_gemm():
    """a_scale / b_scale with e4m3 operands: oracle.fp8_ref.gemm of the same codes
    (padded rows holding 0x7F, the e4m3 NaN, past K; scales followed by NaN), alpha,
    and the bias epilogue on top; mag carries the scales on |qa| @ |qb|."""
    from oracle import fp8_ref
    M, N, Kd = 37, 24, 128
    qa, sa = fp8_ref.quant_rows(rnd(M, Kd, seed=70).float())
    qb, sb = fp8_ref.quant_rows(rnd(N, Kd, seed=71, scale=0.05).float())
    A = torch.full((M, Kd + 16), 0x7F, dtype=torch.uint8).view(torch.float8_e4m3fn)
    B = torch.full((N, Kd + 32), 0x7F, dtype=torch.uint8).view(torch.float8_e4m3fn)
    A.view(torch.uint8)[:, :Kd] = qa.view(torch.uint8)
    B.view(torch.uint8)[:, :Kd] = qb.view(torch.uint8)
    sa_p, sb_p = torch.cat([sa, torch.tensor([float("nan")])]), torch.cat([sb, torch.tensor([float("nan")])])
    want = fp8_ref.gemm(qa, sa, qb, sb)
    ref, mag = G.gemm_ref(A, B, M, N, Kd, a_scale=sa_p, b_scale=sb_p)
    assert torch.allclose(ref, want, rtol=1e-14, atol=0)
    want_mag = (qa.double().abs() @ qb.double().abs().T) * sa.double()[:, None] * sb.double()[None, :]
    assert torch.allclose(mag, want_mag, rtol=1e-14, atol=0) and (mag >= ref.abs()).all()
    bias = rnd(N, seed=72).float()
    ref, mag = G.gemm_ref(A, B, M, N, Kd, a_scale=sa_p, b_scale=sb_p, alpha=0.75, epilogue=G.EPI_BIAS, bias=bias)
    assert ((ref - (0.75 * want + bias.double())).abs() <= 1e-14 * mag).all()
    assert torch.allclose(mag, 0.75 * want_mag + bias.double().abs(), rtol=1e-14, atol=0)
    assert G.e8(192) == G.e8(1024) == G.E32 and G.e8(64) == 2 * 2.299e-5 and G.e8(128) == 2 * 1.417e-5
    assert torch.equal(G.bound(ref, mag, torch.float32, G.e8(64)), G.e8(64) * mag)
