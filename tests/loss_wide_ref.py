"""TEST INFRA: what differs from tests/loss_ref.py when nstl_loss_fwd_bwd runs its
wide tile (csrc/loss.hip, 64 < F <= 128 with NSTL_LOSS_WIDE_OK): the chunk plan, the
rounding counts, the bounds and an f32 emulation.  The float64 values and magnitudes
are loss_ref.loss_ref's, which is general in F.  tests/test_loss_wide_ref.py proves
this file on the CPU; tests/test_loss_wide_parity_gpu.py judges the kernels by it.
Never imported by the package.

The wide kernels are the narrow ones instantiated on the tile <FMAX 128, TMAX 128>:
P, Y [128][129] f32.  The whole-clip kernel takes T <= 128; longer clips (or
NSTL_LOSS_CHUNKED=1) take the chunked kernel, whose chunks own CH = 126 frames and
stage one halo frame on either side, so a chunk edge lies before frames 126, 252,
378, ...  The per-step loops stride `f += 64`, so with 65..128 columns a lane owns
two elements of each step sum: the accumulator is 0 + e0 (exact) + e1, ONE rounding
in front of wave_sum.

Roundings, recounted from csrc/loss.hip in the manner of loss_ref's table (whole-clip
kernel / chunked kernel lines, the same lines as loss_ref's: the tiles are two
instantiations of one source; only the rows that change are restated, the Huber and
|z| rows are per element and stay 3):
  1 / (|dp| + eps) (52-57 / 161-166)  dp 1, dp*dp 1: a square carries 3; the lane's
                             second element 1; wave_sum 6: 10 under the root, 5
                             after it; sqrtf 1, the f32 constant 1e-8f 1, the add
                             1, the reciprocal 1                                 9
  cos_t (59-63 / 168-172)    (dp inp)(dy iny): 2 (1 + 9 + 1) + 1 = 23, the lane's
                             second element 1, wave_sum 6; relative to
                             sum_f |pn_f tn_f| <= 1                              30
  per-thread accumulation    n_e = ceil(T dpred_ld / 1024) adds (87 / 189); the
                             chunked kernel: the sum of that over its chunks of
                             126 frames.  cos: n_s = ceil((T-1) / 16) steps per
                             wave (49 / 158; per chunk over its staged steps,
                             at most 127)
  wave_sum 6, 16-entry combine 16, as in loss_ref
  g_rec = g_tmp = 3 + n_e + 22,  g_cos = 30 + n_s + 22

The gradient bound stays E32 mag (E32 = 1e-5 = 168 2^-24), with gemm_ref.bound's bf16
store term.  The recounted figure stays under it: the first cosine term is dy 1 +
iny 9 + inp 9 + two products = 21 roundings; the second cos_s 30 (relative to
sum|pn tn| <= 1), dp 1, np 7 (10 under the root is 5 after it, sqrtf 1: 6 <= 7),
np + eps 2, the product, the quotient and the product 3 = 43; w3, / n_dir, the
subtraction from the sign term, g + gd_prev - gd_cur and grad_scale add 6: at most
49 2^-24 = 2.9e-6 of mag."""
import torch

from tests import loss_ref as L

E32, U32, BF16_HALF_ULP = L.E32, L.U32, L.BF16_HALF_ULP
NT, NWAVE = L.NT, L.NWAVE
TMAX, CH, FMAX = 128, 126, 128  # loss.hip, wide tile: whole-clip limit, frames a chunk owns, columns


def chunks(T, stride=CH, own=CH):
    """[(t0, t1, lo, hi)] of the wide chunked kernel: owned frames [t0, t1), staged
    [lo, hi).  stride != own is the defect of a chunk loop that advances by another
    tile's chunk length (test_loss_wide_ref)."""
    out = []
    for t0 in range(0, T, stride):
        t1 = min(T, t0 + own)
        out.append((t0, t1, max(t0 - 1, 0), min(t1 + 1, T)))
    return out


def sum_roundings(T, dpred_ld, chunked):
    """(g_rec, g_tmp, g_cos) of the wide kernels (the table in the module docstring)."""
    cdiv = lambda a, b: -(-a // b)
    if chunked:
        n_e = sum(cdiv((t1 - t0) * dpred_ld, NT) for t0, t1, lo, hi in chunks(T))
        n_s = sum(cdiv(hi - lo - 1, NWAVE) for t0, t1, lo, hi in chunks(T))
    else:
        n_e, n_s = cdiv(T * dpred_ld, NT), cdiv(T - 1, NWAVE)
    return 3 + n_e + 22, 3 + n_e + 22, 30 + n_s + 22


def bounds(r, chunked, d_dtype=torch.float32):
    """loss_ref.bounds with the wide kernels' rounding counts."""
    g = torch.tensor(sum_roundings(r.T, r.ldd, chunked), dtype=torch.float64)
    pb = g * U32 * r.partial_mag
    w1, w2, w3 = (abs(v) for v in r.w)
    e = pb.sum(0) / torch.tensor(r.n, dtype=torch.float64)
    ob = torch.stack([w1 * e[0] + w2 * e[1] + w3 * e[2], e[0], e[1], e[2]]) + U32 * r.out_mag
    db = E32 * r.dpred_mag + r.jump * r.near
    if d_dtype == torch.bfloat16:
        db = BF16_HALF_ULP * r.dpred.abs() + (1.0 + BF16_HALF_ULP) * db
    return pb, ob, db


def _step_sum(x, cols64=False):
    """[steps][F] -> [steps]: a lane's two elements (f, f + 64), then the wave tree."""
    x = torch.nn.functional.pad(x, (0, 2 * 64 - x.shape[-1]))
    lanes = x[..., :64] if cols64 else x[..., :64] + x[..., 64:]
    return L._wave_tree(lanes)


def loss_emulate(pred, trg, B, T, F, *, delta=1.0, w1=1.0, w2=1.0, w3=1.0, grad_scale=1.0, dpred_ld=None,
                 chunked=False, bf16=False, cols64=False, double_halo=False, stride254=False, norm64=False,
                 pad_value=0.0):
    """(partial f32 [B][3], out f32 [4], dpred [B*T][dpred_ld]) as the wide kernels
    compute them (torch f32 on the CPU, the kernels' operation order as far as torch
    allows).  The keywords after bf16 are wrong kernels the bounds must catch:
      cols64       the step norms and the cosine summed over columns 0..63 only
      double_halo  the halo step of a chunk edge counted by both chunks
      stride254    the chunk loop advancing by the narrow tile's 254 frames while a
                   chunk holds 126: frames 126..253 of every stride are never summed,
                   their gradient rows never written (they read NaN, the prefill)
      norm64       n_rec and n_tmp of the gradient formed with 64 in place of F
      pad_value    that value left in the dpred columns F..dpred_ld-1"""
    assert 1 <= F <= FMAX
    ldd = F if dpred_ld is None else dpred_ld
    f = torch.float32
    c = lambda v: torch.tensor(v, dtype=f)
    delta, w1, w2, w3, gs = c(delta), c(w1), c(w2), c(w3), c(grad_scale)
    Fn = 64 if norm64 else F
    n_rec, n_tmp, n_dir = c(float(B * T * Fn)), c(float(B * (T - 1) * Fn)), c(float(B * (T - 1)))
    eps = c(1e-8)
    P, Y = L.window(pred, B, T, F).to(f), L.window(trg, B, T, F).to(f)
    partial = torch.zeros(B, 3, dtype=f)
    dpred = torch.zeros(B * T, ldd, dtype=f)
    dpred[:, F:] = pad_value
    if not chunked:
        spans = [(0, T, 0, T)]
    elif stride254:
        spans = chunks(T, stride=254, own=CH)
    else:
        spans = chunks(T)
    for b in range(B):
        p, y = P[b], Y[b]
        dp, dy = p[1:] - p[:-1], y[1:] - y[:-1]
        npn, nyn = torch.sqrt(_step_sum(dp * dp, cols64)), torch.sqrt(_step_sum(dy * dy, cols64))
        inp, iny = 1.0 / (npn + eps), 1.0 / (nyn + eps)
        cs = _step_sum((dp * inp[:, None]) * (dy * iny[:, None]), cols64)
        gv = dy * iny[:, None] * inp[:, None]
        den = torch.where(npn > 0, npn * (npn + eps), torch.ones_like(npn))
        gv = torch.where((npn > 0)[:, None], gv - cs[:, None] * dp / den[:, None], gv)
        z = dp - dy
        gd = w2 * torch.sign(z) / n_tmp - w3 * gv / n_dir
        d = p - y
        ad = d.abs()
        hub = torch.where(ad < delta, 0.5 * d * d / delta, ad - 0.5 * delta)
        g = w1 * torch.where(ad < delta, d / delta, torch.sign(d)) / n_rec
        gp, gc = torch.zeros_like(g), torch.zeros_like(g)
        gp[1:], gc[:-1] = gd, gd
        rows = (g + gp - gc) * gs
        az = torch.cat([z.abs(), torch.zeros(1, F, dtype=f)])  # frame T-1 owns no step
        rec_acc, tmp_acc = torch.zeros(NWAVE, 64, dtype=f), torch.zeros(NWAVE, 64, dtype=f)
        cos_acc = torch.zeros(NWAVE, dtype=f)
        written = torch.zeros(T, dtype=torch.bool)
        for t0, t1, lo, hi in spans:
            padded = lambda x: torch.nn.functional.pad(x[t0:t1], (0, ldd - F)).reshape(-1)
            rec_acc = rec_acc + L._block_sum(padded(hub))
            tmp_acc = tmp_acc + L._block_sum(padded(az))
            written[t0:t1] = True
            for ls in range(hi - lo - 1):
                if lo + ls >= t0 or double_halo:
                    cos_acc[ls % NWAVE] += cs[lo + ls]
        dpred[b * T:(b + 1) * T, :F] = rows
        dpred[b * T:(b + 1) * T][~written] = float("nan")
        for k, acc in enumerate((L._wave_tree(rec_acc), L._wave_tree(tmp_acc), cos_acc)):
            s = c(0.0)
            for v in acc:
                s = s + v
            partial[b, k] = s
    # loss_final is the narrow kernels' own: it normalises by F whatever the tile
    tot = partial.double().sum(0)
    rec, tmp, dr = tot[0] / (B * T * F), tot[1] / (B * (T - 1) * F), 1.0 - tot[2] / (B * (T - 1))
    out = torch.stack([w1.double() * rec + w2.double() * tmp + w3.double() * dr, rec, tmp, dr]).to(f)
    if bf16:
        dpred = dpred.to(torch.bfloat16)
    return partial, out, dpred


def case(name, B, T, F, *, chunked=False, **kw):
    """loss_ref.case at the wide tile's whole-clip limit."""
    c = L.case(name, B, T, F, chunked=chunked, **kw)
    c.update(chunked=chunked or T > TMAX, force=chunked and T <= TMAX)
    return c


# loss_ref.CASES moved to the wide tile's edges.  A chunk edge lies before frames 126,
# 252, 378, ...; the step that straddles it (125, 251, 377, ...) is evaluated by both
# chunks.  Zero steps sit on either side of it everywhere, and on it in "T129" and at
# the later edges of "T379"; elsewhere it stays live, since a zero step has cos = 0
# and would hide a sum that counted it twice.
CASES = [
    case("one-step-68", 2, 2, 68),
    case("clip17-68", 3, 17, 68, bf16=True, ldd=128, gs=3.0, w=(0.3, 0.5, 2.0), delta=0.25, scale=0.3,
         zp=(0, 5, 15), zt=(5, 7)),
    case("F65", 2, 16, 65, ldd=72, gs=0.125, w=(0.0, 0.0, 1.0)),
    case("F128", 2, 16, 128, ldd=136),
    case("F127", 2, 33, 127, ldd=128, scale=0.3),
    case("T128-68", 2, 128, 68, bf16=True, ldd=128, w=(1.0, 0.0, 0.0), delta=0.25, pad=False, zp=(124, 125, 126),
         zt=(0,)),
    case("B65-100", 65, 4, 100, ldd=128, gs=3.0),
    case("B130-68", 130, 3, 68, bf16=True, scale=0.3),
    case("chunked127", 2, 127, 68, chunked=True, ldd=128, zp=(124,), zt=(123,)),
    case("chunked128", 2, 128, 128, chunked=True, bf16=True, zt=(124, 126)),
    case("T129", 2, 129, 68, ldd=72, w=(0.3, 0.5, 2.0), delta=0.25, zp=(124, 125, 126), zt=(0, 127)),
    case("T252-F128", 2, 252, 128, bf16=True, ldd=128, gs=0.125, scale=0.3),
    case("T253-F65", 2, 253, 65, zp=(126,), zt=(124, 250)),
    case("T379", 2, 379, 68, w=(0.0, 0.0, 1.0), pad=False, zp=(0, 124, 126, 250, 251, 252, 377)),
    case("T4096-F128", 1, 4096, 128, bf16=True, ldd=136),
]
