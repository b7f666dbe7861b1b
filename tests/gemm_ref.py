"""TEST INFRA: float64 reference of one nstl_gemm call (csrc/gemm.hip, csrc/gemm4.h)
with its per-element error bound, with no GPU dependency.  tests/test_gemm_ref.py
proves it against torch autograd, rowwise_ref and a scalar port of the dropout hash;
tests/test_gemm_parity_gpu.py judges the kernels by it.  Never imported by the
package.

Tensors may live on any device: the f64 products run where the operands are."""
import numpy as np
import torch

from tests import fp8_table_ref as F8
from tests import rowwise_ref as R

EPI_NONE, EPI_BIAS, EPI_BIAS_RELU_DROP, EPI_BIAS_ROPE, EPI_DRELU_DROP = 0, 1, 2, 3, 4

# The project's per-element bound of an f32-accumulated GEMM, relative to the
# magnitude its roundings act on (tests/test_tight_parity_gpu.py, K up to 16,384).
E32 = 1e-5
BF16_HALF_ULP = 2.0 ** -8  # one rounding to bf16: at most 2^-8 |v|
# fp8 operands: products of two e4m3 values are exact in f32; what is left is how the
# scaled f8f6f4 MFMA adds its 64 or 128 products, and the f32 chain over the K blocks.
# The project's bound E32 is kept wherever the kernels meet it.  They do not at K = 64
# and K = 128 with f32 C (the ring kernel, 1.90 and 1.31 of E32 mag), and neither does
# the instruction alone: tools/fp8_mfma_accum_probe.py (one wave, one chained
# v_mfma_scale_f32_32x32x64_f8f6f4 on register operands, no staging, no epilogue, against
# f64; profiles/fp8_mfma_accum.txt) shows a worst err / mag of 2.299e-5 at K = 64 and
# 1.417e-5 at K = 128 on row-quantised codes.  E8 at those K is twice the probe's
# figure; a kernel that exceeds E8 mag is a finding.  It comes from the probe, not from
# a GEMM kernel's output.
E8_PROBED = {64: 2 * 2.299e-5, 128: 2 * 1.417e-5}


def e8(K):
    """Per-element bound of the fp8 accumulation over K, relative to mag."""
    return E8_PROBED.get(K, E32)


def f32v(x):
    """The value a kernel receives for an f32 argument."""
    return float(np.float32(x))


def drop_thresh(p):
    """common.h nstl_drop_thresh: the threshold on a 16-bit uniform; 0 = no dropout."""
    if p <= 0.0:
        return 0
    return min(int(f32v(p) * 65536.0 + 0.5), 65536)


def inv_keep(p):
    """1 / (1 - p) of the f32 argument."""
    return 1.0 / (1.0 - f32v(p))


def keep_flat(seed, M, N, p):
    """Keep decision of element (i, j) of an [M][N] output from its flat index
    e = i*N + j, for any N (common.h nstl_keep): the hash of pair e >> 1 (indices
    past 2^33 fold their high word into the seed term), low 16 bits for even e, high
    16 for odd e, against the threshold.  Returns a numpy bool array [M][N]."""
    e = np.arange(M, dtype=np.uint64)[:, None] * np.uint64(N) + np.arange(N, dtype=np.uint64)[None, :]
    hi = (e >> np.uint64(33)) & np.uint64(0xFFFFFFFF)
    fold = ((hi << np.uint64(17)) | (hi >> np.uint64(15))) & np.uint64(0xFFFFFFFF)
    seed_term = (seed & 0xFFFFFFFF) ^ (((seed >> 32) * 0x27D4EB2F) & 0xFFFFFFFF)
    h = (((e >> np.uint64(1)) & np.uint64(0xFFFFFFFF)) ^ np.uint64(seed_term) ^ fold)
    h ^= h >> np.uint64(16)
    h = (h * np.uint64(0x85EBCA6B)) & np.uint64(0xFFFFFFFF)
    h ^= h >> np.uint64(13)
    h = (h * np.uint64(0xC2B2AE35)) & np.uint64(0xFFFFFFFF)
    h ^= h >> np.uint64(16)
    u16 = np.where((e & np.uint64(1)) == 0, h & np.uint64(0xFFFF), h >> np.uint64(16))
    return u16 >= np.uint64(drop_thresh(p))


def operand(X, rows, red, kmajor):
    """The [rows][red] f64 matrix of a stored operand: X is [rows][ld] when K-major,
    [red][ld] otherwise (padding columns are cut off).  float8_e4m3fn operands are
    decoded from their code bytes by fp8_table_ref's table, not by torch's cast."""
    if X.dtype == torch.float8_e4m3fn:
        table = torch.from_numpy(F8.CODE_VALUES).to(X.device)
        X = table[X.detach().view(torch.uint8).long()]
    X = X.detach().double()
    return X[:rows, :red] if kmajor else X[:red, :rows].T


def rope_mag(mag, cos, sin, T, rope_dim):
    """rope_ref's map on magnitudes: mag_even |cos| + mag_odd |sin| (even outputs),
    mag_even |sin| + mag_odd |cos| (odd outputs)."""
    rows, cols = mag.shape
    dev = mag.device
    t = torch.arange(rows, device=dev) % T
    pr = (torch.arange(0, cols, 2, device=dev) % rope_dim) // 2
    c = cos.detach().double().to(dev).abs()[t][:, pr]
    s = sin.detach().double().to(dev).abs()[t][:, pr]
    e, o = mag[:, 0::2], mag[:, 1::2]
    out = torch.empty_like(mag)
    out[:, 0::2] = e * c + o * s
    out[:, 1::2] = e * s + o * c
    return out


def gemm_ref(A, B, M, N, K, *, a_kmajor=True, b_kmajor=True, alpha=1.0, beta=0.0, C0=None, epilogue=EPI_NONE,
             bias=None, aux=None, p_drop=0.0, seed=0, rope=None, rope_cols=0, a_scale=None, b_scale=None):
    """(ref, mag), f64 [M][N], of one call described by the K.gemm keywords.

    acc = A(i, :) . B(j, :) of the operands as stored (bf16 values and decoded e4m3
    code bytes are exact in f64); v = alpha acc, for fp8 operands v = alpha a_scale[i]
    b_scale[j] acc with the f32 row scales of A [M] and B [N] (mag carries the same
    factors on |qa| @ |qb|); + bias[j] (every epilogue but NONE and DRELU_DROP); then
      BIAS_RELU_DROP: max(v, 0) keep(i, j) / (1 - p)  (keep_flat)
      BIAS_ROPE:      columns < rope_cols rotated (rowwise_ref.rope_ref; rope =
                      (cos, sin, rope_T, rope_dim))
      DRELU_DROP:     v (aux[i, j] > 0) / (1 - p)
    then + beta C0 (the prior C as stored; only its [M][N] window is read).

    mag is the magnitude the kernel's f32 arithmetic rounds against, carried through
    the same maps: |alpha| (|A| @ |B|) + |bias|; times 1 / (1 - p) where kept and 0
    where dropped (a dropped element is an exact zero); mag_even |cos| + mag_odd |sin|
    for rotated pairs; + |beta C0|.  ReLU leaves it alone (it is 1-Lipschitz, so an
    error of the pre-activation bounds the error after it, also across a sign flip).
    mag >= |ref| everywhere."""
    A64, B64 = operand(A, M, K, a_kmajor), operand(B, N, K, b_kmajor)
    dev = A64.device
    alpha, beta = f32v(alpha), f32v(beta)
    v = alpha * (A64 @ B64.T)
    mag = abs(alpha) * (A64.abs() @ B64.abs().T)
    if a_scale is not None or b_scale is not None:
        sc = a_scale.detach().double().to(dev)[:M, None] * b_scale.detach().double().to(dev)[None, :N]
        v, mag = v * sc, mag * sc.abs()
    if bias is not None and epilogue not in (EPI_NONE, EPI_DRELU_DROP):
        b = bias.detach().double().to(dev)[:N]
        v = v + b
        mag = mag + b.abs()
    if epilogue == EPI_BIAS_RELU_DROP:
        v = v.clamp_min(0.0)
        if drop_thresh(p_drop):
            keep = torch.from_numpy(keep_flat(seed, M, N, p_drop)).to(dev).double()
            v = v * keep * inv_keep(p_drop)
            mag = mag * keep * inv_keep(p_drop)
    elif epilogue == EPI_BIAS_ROPE:
        cos, sin, rope_T, rope_dim = rope
        rc = min(rope_cols, N)
        if rc > 0:
            v = v.clone()
            v[:, :rc] = R.rope_ref(v[:, :rc], cos, sin, rope_T, rope_dim).to(dev)
            mag[:, :rc] = rope_mag(mag[:, :rc], cos, sin, rope_T, rope_dim)
    elif epilogue == EPI_DRELU_DROP:
        pos = (aux.detach().double().to(dev)[:M, :N] > 0).double() * inv_keep(p_drop)
        v = v * pos
        mag = mag * pos
    if beta != 0.0:
        c0 = beta * C0.detach().double().to(dev)[:M, :N]
        v = v + c0
        mag = mag + c0.abs()
    return v, mag


def bound(ref, mag, c_dtype, e=E32):
    """Per-element bound of a stored output: E32 mag for f32; for bf16 the store's
    rounding on top, 2^-8 |ref| + (1 + 2^-8) E32 mag (the rounding acts on the f32
    value, which is within E32 mag of ref).  fp8 operands: e = e8(K) in place of E32."""
    if c_dtype == torch.float32:
        return e * mag
    return BF16_HALF_ULP * ref.abs() + (1.0 + BF16_HALF_ULP) * e * mag
