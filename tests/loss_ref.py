"""TEST INFRA: float64 restatement of one nstl_loss_fwd_bwd call (csrc/loss.hip) with
its error bounds, with no GPU dependency.  tests/test_loss_ref.py proves it against
f64 autograd of oracle.model_ref.loss_fn and an f32 emulation of the kernel's
arithmetic; tests/test_loss_parity_gpu.py judges the kernels by it.  Never imported
by the package.

The operation, from the tensors as stored (f32 values are exact in f64), with
dp_t = p_{t+1} - p_t, dy_t likewise, z = dp - dy, eps = 1e-8 added to the norms:
  partial[b][0] = sum_{t,f} huber_delta(p - y)       n_rec = B T F
  partial[b][1] = sum_{t<T-1,f} |z|                  n_tmp = B (T-1) F
  partial[b][2] = sum_{t<T-1} cos_t                  n_dir = B (T-1)
  cos_t = sum_f pn_f tn_f,  pn = dp / (|dp| + eps),  tn = dy / (|dy| + eps)
  loss_out = (w1 rec + w2 tmp + w3 dir, rec, tmp, dir),  dir = 1 - sum cos / n_dir
  dpred[b T + t][f] = grad_scale (g_rec + gd_{t-1} - gd_t),  exact 0 for f >= F
  g_rec = w1 clamp((p - y) / delta, -1, 1) / n_rec
  gd_s  = w2 sign(z_s) / n_tmp - w3 gcos_s / n_dir
  gcos_s,f = tn_f / (|dp| + eps) - cos_s dp_f / (|dp| (|dp| + eps))
with torch's convention at the origin: the second term is 0 when |dp| == 0.

Bounds.  A sum is held to g 2^-24 sum|term|, g the number of roundings on the
longest path of that sum.  Counted from csrc/loss.hip (whole-clip kernel / chunked
kernel lines; every f32 operation's rounding is relative to its own result):
  Huber term (92 / 194)      d 1, d*d 1, / delta 1 (0.5 * exact); linear branch:
                             d 1 acting on |d| <= 2 term, the subtraction 1     3
  |z| (97-102 / 198-203)     dp and dy 1 each, acting on |dp| + |dy|; the
                             subtraction 1.  With sum(|dp| + |dy|) <= 2 sum|z|
                             (loss_ref asserts it of its inputs) 2 + 1           3
  1 / (|dp| + eps) (52-57 / 161-166)  dp 1, dp*dp 1: a square carries 3; wave_sum
                             6 (common.h:212; F <= 64 is one element per lane):
                             9 under the root, 4.5 after it; sqrtf 1, the f32
                             constant 1e-8f 1, the add 1, the reciprocal 1      9
  cos_t (59-63 / 168-172)    (dp inp)(dy iny): 2 (1 + 9 + 1) + 1 = 23, wave_sum
                             6; relative to sum_f |pn_f tn_f| <= 1              29
  per-thread accumulation    n_e = ceil(T dpred_ld / 1024) adds (87 / 189); the
                             chunked kernel: the sum of that over its chunks of
                             254 frames.  cos: ceil((T-1) / 16) steps per wave
                             (49 / 158; per chunk over its staged steps)
  wave_sum (111-113 / 214-216)                                                   6
  16-entry combine (122 / 225)                                                  16
  g_rec = g_tmp = 3 + n_e + 22,  g_cos = 29 + n_steps + 22
loss_final sums the partials in double (its error is below 2^-50 of them): the
normalised sums inherit the partials' bounds divided by the normaliser, and every
loss_out entry gets one more f32 rounding, 2^-24 of the magnitudes it is cast from.

A gradient element is held to E32 mag (E32 = 1e-5 = 168 2^-24, gemm_ref), mag =
grad_scale (|g_rec| + |g_tmp,t-1| + |g_tmp,t| + sum_{s in {t-1,t}} w3 / n_dir
(|dy_s,f| / ((|dy_s| + eps)(|dp_s| + eps)) + |dp_s,f| / (|dp_s| (|dp_s| + eps)))),
the second cosine term with sum_f |pn tn| <= 1 in place of |cos_s|.  The derived
figure stays under E32: the first cosine term is dy 1 + iny 9 + inp 9 + two
products = 21 roundings; the second cos_s 29 (relative to sum|pn tn| <= 1), dp 1,
np 7, np + eps 2, the product, the quotient and the product 3 = 42; w3, / n_dir,
the subtraction from the sign term, g + gd_prev - gd_cur and grad_scale add 6:
at most 48 2^-24 = 2.9e-6 of mag.  A bf16 dpred adds the store's rounding as
gemm_ref.bound does: 2^-8 |ref| + (1 + 2^-8) E32 mag.

sign(z) is discontinuous: an element whose step s has 0 < |z64| <= 2^-22 (|dp| +
|dy|) may see the other sign in f32 (z's absolute error is at most 2^-24 (|dp| +
|dy| + |z|)); it gets the jump 2 w2 / n_tmp grad_scale added per such step, and
`near` counts these.  z64 == 0 is exact in f32 too (dp == dy as f32 values give 0).
The Huber gradient is continuous across |d| = delta."""
import types

import torch

from tests import gemm_ref as G

E32 = G.E32
BF16_HALF_ULP = G.BF16_HALF_ULP
U32 = 2.0 ** -24
EPS = 1e-8
NT, NWAVE, TMAX, CH = 1024, 16, 256, 254  # loss.hip: threads, waves, whole-clip limit, chunk


def chunks(T):
    """[(t0, t1, lo, hi)] of the chunked kernel: owned frames [t0, t1), staged [lo, hi)."""
    out = []
    for t0 in range(0, T, CH):
        t1 = min(T, t0 + CH)
        out.append((t0, t1, max(t0 - 1, 0), min(t1 + 1, T)))
    return out


def sum_roundings(T, dpred_ld, chunked):
    """(g_rec, g_tmp, g_cos): roundings on the longest path of each partial sum (the
    table in the module docstring)."""
    cdiv = lambda a, b: -(-a // b)
    if chunked:
        n_e = sum(cdiv((t1 - t0) * dpred_ld, NT) for t0, t1, lo, hi in chunks(T))
        n_s = sum(cdiv(hi - lo - 1, NWAVE) for t0, t1, lo, hi in chunks(T))
    else:
        n_e, n_s = cdiv(T * dpred_ld, NT), cdiv(T - 1, NWAVE)
    return 3 + n_e + 22, 3 + n_e + 22, 29 + n_s + 22


def window(x, B, T, F):
    """The [B][T][F] f64 values of a stored [B*T][ld] (or [B][T][ld]) operand."""
    x = x.detach().double().cpu()
    return x.reshape(B * T, -1)[:, :F].reshape(B, T, F)


def loss_ref(pred, trg, B, T, F, *, delta=1.0, w1=1.0, w2=1.0, w3=1.0, grad_scale=1.0, dpred_ld=None):
    """The f64 results of one call and the magnitudes its f32 arithmetic rounds against:
    partial, partial_mag [B][3]; out, out_mag [4] (out_mag[0]: |w1 rec| + |w2 tmp| +
    |w3| (1 + |sum cos| / n_dir), the others their own values likewise); dpred,
    dpred_mag [B*T][dpred_ld]; near [B*T][dpred_ld]: steps (0..2) of the element whose
    z may change sign in f32."""
    ldd = F if dpred_ld is None else dpred_ld
    delta, w1, w2, w3, gs = (G.f32v(v) for v in (delta, w1, w2, w3, grad_scale))
    p, y = window(pred, B, T, F), window(trg, B, T, F)
    n_rec, n_tmp, n_dir = float(B * T * F), float(B * (T - 1) * F), float(B * (T - 1))
    d = p - y
    ad = d.abs()
    hub = torch.where(ad < delta, 0.5 * d * d / delta, ad - 0.5 * delta)
    dp, dy = p[:, 1:] - p[:, :-1], y[:, 1:] - y[:, :-1]
    z = dp - dy
    npn, nyn = dp.norm(dim=-1, keepdim=True), dy.norm(dim=-1, keepdim=True)
    inp, iny = 1.0 / (npn + EPS), 1.0 / (nyn + EPS)
    pntn = (dp * inp) * (dy * iny)
    cos = pntn.sum(-1, keepdim=True)
    inner = (dp.abs() + dy.abs()).sum().item()
    assert inner <= 2.0 * z.abs().sum().item(), "inputs: sum(|dp| + |dy|) > 2 sum|z| (the |z| row of the table)"

    partial = torch.stack([hub.sum((1, 2)), z.abs().sum((1, 2)), cos.sum((1, 2))], 1)
    partial_mag = torch.stack([hub.sum((1, 2)), z.abs().sum((1, 2)), pntn.abs().sum((1, 2))], 1)
    tot = partial.sum(0)
    rec, tmp, cm = tot[0].item() / n_rec, tot[1].item() / n_tmp, tot[2].item() / n_dir
    out = torch.tensor([w1 * rec + w2 * tmp + w3 * (1.0 - cm), rec, tmp, 1.0 - cm], dtype=torch.float64)
    out_mag = torch.tensor([abs(w1) * rec + abs(w2) * tmp + abs(w3) * (1.0 + abs(cm)), rec, tmp, 1.0 + abs(cm)],
                           dtype=torch.float64)

    # gradient with respect to dp_s: sign term and cosine term, and their magnitudes
    safe = torch.where(npn > 0, npn, torch.ones_like(npn))
    second = torch.where(npn > 0, dp / (safe * (npn + EPS)), torch.zeros_like(dp))
    gcos = dy * iny * inp - cos * second
    gd = w2 * torch.sign(z) / n_tmp - w3 * gcos / n_dir
    gd_mag = abs(w2) * (z != 0).double() / n_tmp + abs(w3) / n_dir * ((dy * iny * inp).abs() + second.abs())
    g_rec = w1 * torch.where(ad < delta, d / delta, torch.sign(d)) / n_rec
    g = g_rec.clone()
    mag = g_rec.abs()
    g[:, 1:] += gd
    g[:, :-1] -= gd
    mag[:, 1:] += gd_mag
    mag[:, :-1] += gd_mag
    nz = ((z != 0) & (z.abs() <= 2.0 ** -22 * (dp.abs() + dy.abs()))).double()
    near = torch.zeros_like(g)
    near[:, 1:] += nz
    near[:, :-1] += nz

    def pad(x):
        o = torch.zeros(B * T, ldd, dtype=torch.float64)
        o[:, :F] = x.reshape(B * T, F)
        return o
    return types.SimpleNamespace(
        B=B, T=T, F=F, ldd=ldd, partial=partial, partial_mag=partial_mag, out=out, out_mag=out_mag,
        dpred=pad(g * gs), dpred_mag=pad(mag * abs(gs)), near=pad(near),
        jump=2.0 * abs(w2) / n_tmp * abs(gs), w=(w1, w2, w3), n=(n_rec, n_tmp, n_dir))


def bounds(r, chunked, d_dtype=torch.float32):
    """(partial_bound [B][3], out_bound [4], dpred_bound [B*T][dpred_ld]) of loss_ref's
    result r for the whole-clip (chunked=False) or the chunked kernel."""
    g = torch.tensor(sum_roundings(r.T, r.ldd, chunked), dtype=torch.float64)
    pb = g * U32 * r.partial_mag
    w1, w2, w3 = (abs(v) for v in r.w)
    e = pb.sum(0) / torch.tensor(r.n, dtype=torch.float64)  # of rec, tmp and sum cos / n_dir
    ob = torch.stack([w1 * e[0] + w2 * e[1] + w3 * e[2], e[0], e[1], e[2]]) + U32 * r.out_mag
    db = E32 * r.dpred_mag + r.jump * r.near
    if d_dtype == torch.bfloat16:
        db = BF16_HALF_ULP * r.dpred.abs() + (1.0 + BF16_HALF_ULP) * db
    return pb, ob, db


# ---------------------------------------------------------------------------
# f32 emulation of the kernels' arithmetic (torch f32 on the CPU; the kernel's
# operation order as far as torch allows: its per-thread strided accumulation, a
# halving tree for the wave butterfly, the 16-entry combine in order)
# ---------------------------------------------------------------------------
def _wave_tree(x):
    """[..., 64] -> [...]: six halving steps (wave_sum's rounding depth)."""
    while x.shape[-1] > 1:
        h = x.shape[-1] // 2
        x = x[..., :h] + x[..., h:]
    return x[..., 0]


def _block_sum(terms):
    """Per-thread strided accumulation of a flat f32 vector over 1024 threads, the wave
    tree, then the 16-entry combine in order."""
    n = terms.numel()
    k = -(-n // NT)
    t = torch.zeros(k * NT, dtype=torch.float32)
    t[:n] = terms
    acc = torch.zeros(NT, dtype=torch.float32)
    for row in t.reshape(k, NT):
        acc = acc + row
    return acc.reshape(NWAVE, 64)


def loss_emulate(pred, trg, B, T, F, *, delta=1.0, w1=1.0, w2=1.0, w3=1.0, grad_scale=1.0, dpred_ld=None,
                 chunked=False, double_halo=False, bf16=False):
    """(partial f32 [B][3], out f32 [4], dpred [B*T][dpred_ld]) as the kernels compute
    them.  double_halo: the defect of a chunked kernel without `if (lo + ls >= t0)`."""
    ldd = F if dpred_ld is None else dpred_ld
    f = torch.float32
    c = lambda v: torch.tensor(v, dtype=f)
    delta, w1, w2, w3, gs = c(delta), c(w1), c(w2), c(w3), c(grad_scale)
    n_rec, n_tmp, n_dir = c(float(B * T * F)), c(float(B * (T - 1) * F)), c(float(B * (T - 1)))
    eps = c(1e-8)
    P, Y = window(pred, B, T, F).to(f), window(trg, B, T, F).to(f)
    partial = torch.zeros(B, 3, dtype=f)
    dpred = torch.zeros(B * T, ldd, dtype=f)
    spans = chunks(T) if chunked else [(0, T, 0, T)]
    for b in range(B):
        p, y = P[b], Y[b]
        dp, dy = p[1:] - p[:-1], y[1:] - y[:-1]
        sq = lambda x: _wave_tree(torch.nn.functional.pad(x * x, (0, 64 - F)))
        npn, nyn = torch.sqrt(sq(dp)), torch.sqrt(sq(dy))
        inp, iny = 1.0 / (npn + eps), 1.0 / (nyn + eps)
        cs = _wave_tree(torch.nn.functional.pad((dp * inp[:, None]) * (dy * iny[:, None]), (0, 64 - F)))
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
        dpred[b * T:(b + 1) * T, :F] = (g + gp - gc) * gs
        az = torch.cat([z.abs(), torch.zeros(1, F, dtype=f)])  # frame T-1 owns no step
        rec_acc, tmp_acc = torch.zeros(NWAVE, 64, dtype=f), torch.zeros(NWAVE, 64, dtype=f)
        cos_acc = torch.zeros(NWAVE, dtype=f)
        for t0, t1, lo, hi in spans:
            padded = lambda x: torch.nn.functional.pad(x[t0:t1], (0, ldd - F)).reshape(-1)
            rec_acc = rec_acc + _block_sum(padded(hub))
            tmp_acc = tmp_acc + _block_sum(padded(az))
            for ls in range(hi - lo - 1):
                if lo + ls >= t0 or double_halo:
                    cos_acc[ls % NWAVE] += cs[lo + ls]
        for k, acc in enumerate((_wave_tree(rec_acc), _wave_tree(tmp_acc), cos_acc)):
            s = c(0.0)
            for v in acc:
                s = s + v
            partial[b, k] = s
    tot = partial.double().sum(0)
    rec, tmp, dr = tot[0] / (B * T * F), tot[1] / (B * (T - 1) * F), 1.0 - tot[2] / (B * (T - 1))
    out = torch.stack([w1.double() * rec + w2.double() * tmp + w3.double() * dr, rec, tmp, dr]).to(f)
    if bf16:
        dpred = dpred.to(torch.bfloat16)
    return partial, out, dpred


def judge(got, ref, bound):
    """Worst err / bound over all elements (none excluded; 0 / 0 counts as 0, err > 0
    under a zero bound as inf), and whether every element is within its bound."""
    got, ref, bound = (torch.as_tensor(x).detach().double().cpu().reshape(-1) for x in (got, ref, bound))
    err = (got - ref).abs()
    err = torch.where(torch.isnan(err), torch.full_like(err, float("inf")), err)
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bound.clamp_min(1e-300))
    return ratio.max().item(), bool((err <= bound).all())


def make_inputs(B, T, F, scale, seed, pred_ld=None, trg_ld=None, zero_pred=(), zero_trg=()):
    """f32 pred / trg buffers [B*T][ld] with NaN padding from N(0, scale^2); zero_pred /
    zero_trg list steps s whose difference is exactly 0 (frame s+1 = frame s)."""
    gen = torch.Generator().manual_seed(seed)
    out = []
    for ld, zeros in ((pred_ld or F, zero_pred), (trg_ld or F, zero_trg)):
        x = (torch.randn(B, T, F, generator=gen, dtype=torch.float64) * scale).float()
        for s in sorted(zeros):
            x[:, s + 1] = x[:, s]
        buf = torch.full((B * T, ld), float("nan"), dtype=torch.float32)
        buf[:, :F] = x.reshape(B * T, F)
        out.append(buf)
    return out


def case(name, B, T, F, *, chunked=False, bf16=False, ldd=None, gs=1.0, w=(1.0, 1.0, 1.0), delta=1.0, scale=30.0,
         pad=True, zp=(), zt=()):
    return dict(name=name, B=B, T=T, F=F, chunked=chunked or T > TMAX, force=chunked and T <= TMAX, bf16=bf16,
                ldd=ldd or F, gs=gs, w=w, delta=delta, scale=scale, pred_ld=F + 3 if pad else F,
                trg_ld=F + 5 if pad else F, zp=zp, zt=zt)


# The shapes tests/test_loss_parity_gpu.py runs (and tests/test_loss_ref.py emulates):
# the smallest that reach each path of csrc/loss.hip.  zp / zt: steps with an exactly
# zero difference in pred / trg (step 5 of "clip17" in both: z == 0 on both sides).
# A chunk edge lies before frames 254, 508, ...; the step that straddles it (253, 507,
# ...) is evaluated by both chunks.  Zero steps sit on either side of it everywhere,
# and on it in "T257" and at the later edges of "T763" (the `np > 0` branch in the halo);
# elsewhere it stays live, since a zero step has cos = 0 and would hide a sum that
# counted it twice.
CASES = [
    case("one-step", 2, 2, 61),
    case("clip17", 3, 17, 61, bf16=True, ldd=64, gs=3.0, w=(0.3, 0.5, 2.0), delta=0.25, scale=0.3,
         zp=(0, 5, 15), zt=(5, 7)),
    case("F64", 2, 16, 64, ldd=72, gs=0.125, w=(0.0, 0.0, 1.0)),
    case("F1", 2, 33, 1, ldd=64, scale=0.3),
    case("T256", 2, 256, 61, bf16=True, ldd=72, w=(1.0, 0.0, 0.0), delta=0.25, pad=False, zp=(252, 253, 254),
         zt=(0,)),
    case("B65", 65, 4, 7, ldd=64, gs=3.0),
    case("B130", 130, 3, 61, bf16=True, scale=0.3),
    case("chunked255", 2, 255, 61, chunked=True, ldd=64, zp=(252,), zt=(251,)),
    case("chunked256", 2, 256, 61, chunked=True, bf16=True, zt=(252, 254)),
    case("T257", 2, 257, 61, ldd=72, w=(0.3, 0.5, 2.0), delta=0.25, zp=(252, 253, 254), zt=(0, 255)),
    case("T508", 2, 508, 61, bf16=True, ldd=64, gs=0.125, scale=0.3),
    case("T509-F64", 2, 509, 64, zp=(254,), zt=(252, 506)),
    case("T763", 2, 763, 61, w=(0.0, 0.0, 1.0), pad=False, zp=(0, 252, 254, 506, 507, 508, 761)),
    case("T4096", 1, 4096, 61, bf16=True, ldd=72),
]


def case_inputs(c, seed=0):
    return make_inputs(c["B"], c["T"], c["F"], c["scale"], 1000 + seed, c["pred_ld"], c["trg_ld"], c["zp"], c["zt"])


def case_kw(c):
    w1, w2, w3 = c["w"]
    return dict(delta=c["delta"], w1=w1, w2=w2, w3=w3, grad_scale=c["gs"], dpred_ld=c["ldd"])
