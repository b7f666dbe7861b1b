"""TEST INFRA: float64 reference of one nstl_attn_fwd / nstl_attn_bwd call
(csrc/attention.hip, csrc/attention_long.hip, csrc/attention_dev.h) with its
per-element error bound, with no GPU dependency.  tests/test_attn_ref.py proves it
against torch autograd, the scalar port of the dropout hash and a CPU emulation of
the kernels' bf16 roundings; tests/test_attention_parity_gpu.py judges the kernels
by it.  Never imported by the package.

Tensors are [B][H][T][dh] and may live on any device: the f64 products run where
the operands are.

The operation.  scale = dh^-1/2, S = scale q k^T, lse = logsumexp_k S (over the
undropped scores), P = exp(S - lse), Pd = P keep / (1 - p), O = Pd v.  Backward,
with D = rowsum(dO * O_stored) formed from the forward's STORED output (what every
dQ / dK kernel does; with the reference's own O the D term alone would carry the
forward's bf16 rounding into the bound): dP = dO v^T, dS = P (dP keep / (1 - p) - D),
dq = RoPE^T(scale dS k), dk = RoPE^T(scale dS^T q), dv = Pd^T dO.

Error model.  `mag` is the magnitude a rounding of the second product's register
operand acts on (every map above on absolute values: Pd |v|, |dS| |k|, ...), `mag32`
the magnitude the f32 arithmetic rounds against.  A score carries an f32 product
error of E32 scale (|q| . |k|) and the exponent also the LSE's error, E32 L_q with
L_q = max_k scale (|q| . |k|) + |lse| + 1 (the LSE bound below: the backward reads
the stored LSE; the forward's own normalisation errs by no more); an absolute error
of the exponent is a relative error of P, so P errs by E32 rho P with
rho = 1 + scale (|q| . |k|) + L_q (the 1: exp, the products and sums that follow).
  mag32_o  = (Pd rho) |v|                     mag32_dv = (Pd rho)^T |dO|
  mag32_dS = P (rho |dP keep/(1-p) - D| + (|dO| |v|^T) keep/(1-p) + rowsum |dO O|)
  mag32_dq = scale (mag32_dS + |dS|) |k|      mag32_dk likewise with |q|
RoPE^T maps a magnitude pair to (m_e |cos| + m_o |sin|, m_e |sin| + m_o |cos|)
(gemm_ref.rope_mag).

bound(): f32 outputs E32 mag32.  bf16 outputs
  2^-8 |ref| + c 2^-8 mag + (1 + 2^-8) E32 mag32
where c counts the bf16 roundings between the scores and the output other than
the store's own.  Read from the kernels (P and dS enter the second product through
acc_frag<bf16>, attention_dev.h:154):
  kernel                                   O    dq   dk   dv
  fwd_queries (one-shot, persistent)       1              attention.hip:264
  attn_fwd_long_kernel                     1              attention_long.hip:229
  attn_bwd_dq_kernel                            1         attention.hip:552
  attn_bwd_dkv_kernel                                1    1   attention.hip:671-672
  attn_bwd_fused_kernel                         1    1    1   attention.hip:919-920 (dQ
                                                          reads the same bf16 dS^T image)
  attn_bwd_dq_long / attn_bwd_dkv_long          1    1    1   attention_long.hip:371, 532-533
  generic kernels (f32 P / dS in LDS)      0    0    0    0   attention.hip:1141, 1187, 1239
The forward rounds the unnormalised e = 2^(s - m) and the dV kernels the kept P
before 1 / (1 - p): a rounding is relative, so the later factor does not change c.
The f32 kernels keep P and dS in f32 (acc_frag<float>): c = 0."""
import numpy as np
import torch

from tests import gemm_ref as G

E32 = G.E32
BF16_HALF_ULP = G.BF16_HALF_ULP


def keep(seed, BH, T, p):
    """bool numpy [BH][T][T]: nstl_keep(seed, drop_idx(bh, T, q, k)) with
    drop_idx = (bh*T + q)*T + k (attention_dev.h:122), i.e. gemm_ref.keep_flat of a
    [BH*T][T] matrix.  Odd T: every other row starts on an odd element."""
    return G.keep_flat(seed, BH * T, T, p).reshape(BH, T, T)


def keep_words(kp, T):
    """The uint64 words the MFMA paths store for keep [BH][T][T] (attention_dev.h
    mask_word): [bh][qt][kt][key % 4] with nt = ceil(T / 16), bit
    16*((key % 16) // 4) + query % 16; bits of queries / keys at or past T are 0.
    Returns a flat numpy uint64 array of BH * nt * nt * 4 words."""
    kp = np.asarray(kp, dtype=bool)
    BH = kp.shape[0]
    nt = (T + 15) // 16
    full = np.zeros((BH, nt * 16, nt * 16), dtype=np.uint64)
    full[:, :T, :T] = kp
    x = full.reshape(BH, nt, 16, nt, 4, 4)          # [bh][qt][qi][kt][kg][kr]
    x = x.transpose(0, 1, 3, 5, 4, 2)               # [bh][qt][kt][kr][kg][qi]
    shift = (16 * np.arange(4, dtype=np.uint64)[:, None] + np.arange(16, dtype=np.uint64)[None, :])
    return (x << shift).sum(axis=(-1, -2), dtype=np.uint64).reshape(-1)


def words_to_keep(words, BH, T):
    """Inverse of keep_words: bool [BH][T][T] (bits past T are cut off)."""
    nt = (T + 15) // 16
    w = np.asarray(words).view(np.uint64).reshape(BH, nt, nt, 4)
    bits = ((w[..., None] >> np.arange(64, dtype=np.uint64)) & np.uint64(1)).astype(bool)
    full = bits.reshape(BH, nt, nt, 4, 4, 16).transpose(0, 1, 5, 2, 4, 3).reshape(BH, nt * 16, nt * 16)
    return full[:, :T, :T].copy()


def _keep_factor(kp, p, like):
    """keep / (1 - p) as an f64 tensor shaped like the scores (1 without dropout)."""
    if kp is None or G.drop_thresh(p) == 0:
        return torch.ones_like(like)
    kp = torch.as_tensor(np.asarray(kp), device=like.device).reshape(like.shape)
    return kp.double() * G.inv_keep(p)


def _scores(q, k):
    q, k = q.detach().double(), k.detach().double()
    scale = float(q.shape[-1]) ** -0.5
    S = scale * (q @ k.transpose(-1, -2))
    A = scale * (q.abs() @ k.abs().transpose(-1, -2))
    return S, A


def _rho(A, lse):
    L = A.amax(-1) + lse.abs() + 1.0
    return 1.0 + A + L[..., None], L


def attn_fwd_ref(q, k, v, p=0.0, kp=None):
    """dict of f64 tensors: o, mag_o, mag32_o [B][H][T][dh]; lse, lse_mag [B][H][T]
    (the LSE bound is E32 lse_mag).  kp: keep() of the call (or None)."""
    S, A = _scores(q, k)
    v = v.detach().double()
    lse = torch.logsumexp(S, -1)
    P = torch.exp(S - lse[..., None])
    rho, L = _rho(A, lse)
    Pd = P * _keep_factor(kp, p, P)
    return dict(o=Pd @ v, mag_o=Pd @ v.abs(), mag32_o=(Pd * rho) @ v.abs(), lse=lse, lse_mag=L)


def rope_back(x, cos, sin):
    """RoPE^T of [..][T][dh] with tables [T][dh/2]: (e c + o s, -e s + o c)."""
    c, s = cos.detach().double().to(x.device), sin.detach().double().to(x.device)
    e, o = x[..., 0::2], x[..., 1::2]
    r = torch.empty_like(x)
    r[..., 0::2] = e * c + o * s
    r[..., 1::2] = -e * s + o * c
    return r


def _rope_mag(m, cos, sin):
    T, dh = m.shape[-2], m.shape[-1]
    return G.rope_mag(m.reshape(-1, dh), cos, sin, T, dh).reshape(m.shape)


def attn_bwd_ref(q, k, v, o_stored, lse, dout, p=0.0, kp=None, rope=None):
    """dict of f64 tensors dq, dk, dv with mag_* and mag32_* (module docstring), and
    dsum = rowsum(dout * o_stored) with mag_dsum.  lse: the stored LSE to form P
    from, or None for the reference's own.  rope = (cos, sin, rope_q, rope_k) with
    the f32 tables of engine.rotation_tables, or None."""
    S, A = _scores(q, k)
    q, k, v = q.detach().double(), k.detach().double(), v.detach().double()
    do, o = dout.detach().double(), o_stored.detach().double()
    scale = float(q.shape[-1]) ** -0.5
    own = torch.logsumexp(S, -1)
    lse = own if lse is None else lse.detach().double().reshape(own.shape)
    P = torch.exp(S - lse[..., None])
    rho, _ = _rho(A, lse)
    kf = _keep_factor(kp, p, P)
    Pd = P * kf
    D = (do * o).sum(-1)
    Dm = (do * o).abs().sum(-1)
    dP = (do @ v.transpose(-1, -2)) * kf
    dPm = (do.abs() @ v.abs().transpose(-1, -2)) * kf
    dS = P * (dP - D[..., None])
    dS32 = P * (rho * (dP - D[..., None]).abs() + dPm + Dm[..., None]) + dS.abs()
    r = dict(dsum=D, mag_dsum=Dm,
             dq=scale * (dS @ k), mag_dq=scale * (dS.abs() @ k.abs()), mag32_dq=scale * (dS32 @ k.abs()),
             dk=scale * (dS.transpose(-1, -2) @ q), mag_dk=scale * (dS.abs().transpose(-1, -2) @ q.abs()),
             mag32_dk=scale * (dS32.transpose(-1, -2) @ q.abs()),
             dv=Pd.transpose(-1, -2) @ do, mag_dv=Pd.transpose(-1, -2) @ do.abs(),
             mag32_dv=(Pd * rho).transpose(-1, -2) @ do.abs())
    if rope is not None:
        cos, sin, rq, rk = rope
        for nm, on in (("dq", rq), ("dk", rk)):
            if on:
                r[nm] = rope_back(r[nm], cos, sin)
                r["mag_" + nm] = _rope_mag(r["mag_" + nm], cos, sin)
                r["mag32_" + nm] = _rope_mag(r["mag32_" + nm], cos, sin)
    return r


def bound(ref, mag, dtype, roundings, mag32=None):
    """Per-element bound of a stored output (module docstring).  roundings: c."""
    mag32 = mag if mag32 is None else mag32
    if dtype == torch.float32:
        return E32 * mag32
    return BF16_HALF_ULP * ref.abs() + roundings * BF16_HALF_ULP * mag + (1.0 + BF16_HALF_ULP) * E32 * mag32


def lse_bound(lse_mag):
    return E32 * lse_mag


def worst(got, ref, bnd):
    """(worst err / bound, its index tuple) of one output; NaN counts as infinite."""
    err = (got.detach().double().to(ref.device) - ref).abs()
    ratio = err / (bnd + 1e-300)
    ratio = torch.where(torch.isnan(ratio), torch.full_like(ratio, float("inf")), ratio)
    i = int(ratio.reshape(-1).argmax())
    return ratio.reshape(-1)[i].item(), tuple(int(x) for x in np.unravel_index(i, tuple(ratio.shape)))
