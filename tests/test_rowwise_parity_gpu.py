"""f64 edge parity of the row-wise kernels (csrc/norm.hip, csrc/optim.hip) on the
MI355X: LayerNorm forward / backward, RoPE, cast, copy2d, colsum, the row reducers,
sumsq, shard_sum, clip_coef and Adam against tests/rowwise_ref.py (itself proven in
tests/test_rowwise_ref.py), at the shapes where each kernel changes path.

Bounds (none tuned against a kernel):
  f32 quantities, relative to max|ref|: 2e-6 forward outputs and mean, 1e-5 ds /
  dgamma / dbeta / reducers / colsum; 1e-6 norm, coef and the sumsq partials (per
  element: sums of positives); rtol 1e-5 + atol 1e-6 Adam; rstd 1e-5 per element.
  bf16-stored quantities, per element: 2^-8 |ref| + the f32 bound.  One rounding to
  bf16 is half an ulp, between 2^-9 |v| (top of a binade) and 2^-8 |v| (bottom), so
  a correct kernel reaches this bound from below (measured 0.99 of it) and a second
  rounding, or a value one ulp off, exceeds it.
  bf16 ds / dgamma / dbeta keep the f32 bounds: the kernel computes them in f32
  from the stored s, mean and rstd that the reference takes.
Everything called bit-identical uses torch.equal.

With NSTL_PARITY_ERRORS_OUT=<file> the largest measured error of each quantity is
written next to its bound (profiles/rowwise_parity_errors.txt is such a run)."""
import functools
import os

import numpy as np
import pytest
import torch

from tests import rowwise_ref as R

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from neurosync_trainer_lite_amd import _hip as K
    from neurosync_trainer_lite_amd.engine import rotation_tables

DEV = "cuda:0"
NAN = float("nan")
F32, BF16 = torch.float32, torch.bfloat16
DTYPES = [pytest.param(F32, id="f32"), pytest.param(BF16, id="bf16")]
BF16_REL = 2.0 ** -8

_ERRORS = {}  # quantity -> (fraction of the bound used, bound, measured)


def _note(what, frac, bound, measured):
    if what not in _ERRORS or frac > _ERRORS[what][0]:
        _ERRORS[what] = (frac, bound, measured)


@pytest.fixture(scope="module", autouse=True)
def _error_report():
    yield
    path = os.environ.get("NSTL_PARITY_ERRORS_OUT")
    if path and _ERRORS:
        with open(path, "w") as f:
            f.write("# tests/test_rowwise_parity_gpu.py: largest measured error of each quantity next to its bound\n")
            f.write("# %-34s %-36s %-30s %s\n" % ("quantity", "bound", "measured", "measured / bound"))
            for what in sorted(_ERRORS):
                frac, bound, measured = _ERRORS[what]
                f.write("%-36s %-36s %-30s %.4f\n" % (what, bound, measured, frac))


def rnd(*shape, dtype=F32, scale=1.0, seed=0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g, dtype=torch.float64) * scale).to(dtype).to(DEV)


def f64(t):
    return t.detach().double().cpu()


def f32v(x):
    """The value the kernel receives for an f32 argument."""
    return float(np.float32(x))


def nans(*shape, dtype=F32):
    return torch.full(shape, NAN, dtype=dtype, device=DEV)


def dname(dt):
    return "f32" if dt == F32 else "bf16"


def check(got, ref, rel, what):
    """|got - ref| <= rel * max|ref| (a NaN in got fails)."""
    got, ref = f64(got), f64(ref)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    scale = ref.abs().max().item()
    err = (got - ref).abs().max().item()
    print("%s: max err %.3e, scale %.3e, bound %.1e of it" % (what, err, scale, rel))
    _note(what, err / (rel * scale) if scale > 0 else float(err != 0), "%.0e max|ref|" % rel,
          "%.3e max|ref|" % (err / scale if scale > 0 else err))
    assert err <= rel * scale, "%s: max err %.3e vs scale %.3e (rel %.1e)" % (what, err, scale, rel)


def check_stored(got, ref, rel, what, dt):
    """A quantity stored in dt: the f32 bound, plus one bf16 rounding (2^-8 |ref| per
    element) when dt is bf16."""
    if dt == F32:
        return check(got, ref, rel, what)
    got, ref = f64(got), f64(ref)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    scale = ref.abs().max().item()
    allowed = BF16_REL * ref.abs() + rel * scale
    frac = ((got - ref).abs() / allowed).max().item()
    print("%s: worst element at %.3f of 2^-8|ref| + %.1e max|ref|" % (what, frac, rel))
    _note(what, frac, "2^-8 |ref| + %.0e max|ref|" % rel, "%.3f of the bound" % frac)
    assert frac <= 1.0, "%s: worst element at %.3f of its bound (scale %.3e)" % (what, frac, scale)


def check_rel(got, ref, rel, what, atol=0.0):
    """|got - ref| <= rel * |ref| + atol, per element."""
    got, ref = f64(got), f64(ref)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    frac = ((got - ref).abs() / (rel * ref.abs() + atol)).max().item()
    print("%s: worst element at %.3f of rel %.1e atol %.1e" % (what, frac, rel, atol))
    if atol:  # the bound (and its atol) of the case that came closest to it
        _note(what, frac, "%.0e |ref| + %.0e" % (rel, atol), "%.3f of the bound" % frac)
    else:
        _note(what, frac, "%.0e |ref|" % rel, "%.3e |ref|" % (frac * rel))
    assert frac <= 1.0, "%s: worst element at %.3f of rel %.1e + atol %.1e" % (what, frac, rel, atol)


def check_canary(t, n, what):
    """Rows (elements) 0 .. n-1 of a NaN-prefilled output were written, the rest was not."""
    assert torch.isnan(t[n:].float()).all(), what + ": wrote past its extent"
    assert not torch.isnan(t[:n].float()).any(), what + ": NaN in (or no write to) a written row"


# ---------------------------------------------------------------------------
# LayerNorm
# ---------------------------------------------------------------------------
LN_P, LN_EPS = 0.3, 1e-5
LN_SEEDS = ((0x9E3779B9 << 32) | 0x01234567, (0x7F4A7C15 << 32) | 0x89ABCDEF)  # nonzero high words


@functools.lru_cache(maxsize=None)
def ln_inputs(rows, D, dt):
    """x random; y random with 0.5 <= |y| < 1.5, so that s - x is nonzero exactly
    where the branch is kept (also after s is rounded to bf16: |y| / 0.7 is far above
    half a bf16 ulp of s); gamma, beta; an f32 gradient and a dtype addend."""
    g = torch.Generator().manual_seed(1000 + D)
    sign = torch.randint(0, 2, (rows, D), generator=g).double() * 2 - 1
    y = (sign * (0.5 + torch.rand(rows, D, generator=g, dtype=torch.float64))).to(dt).to(DEV)
    return dict(x=rnd(rows, D, dtype=dt, seed=1), y=y, gamma=1 + 0.1 * rnd(D, seed=2), beta=0.1 * rnd(D, seed=3),
                dout=rnd(rows, D, seed=4), dout2=rnd(rows, D, dtype=dt, seed=5))


def ln_args(dt, rows, D, inp, n_masks, with_x=True):
    a = K.LnArgs()
    a.dtype, a.rows, a.D = K.dtype_code(dt), rows, D
    a.x, a.y = (inp["x"].data_ptr() if with_x else None), inp["y"].data_ptr()
    a.n_masks, a.p_drop, a.seed1, a.seed2 = n_masks, LN_P, LN_SEEDS[0], LN_SEEDS[1]
    a.gamma, a.beta, a.eps = inp["gamma"].data_ptr(), inp["beta"].data_ptr(), LN_EPS
    return a


def ln_forward(dt, rows, D, n_masks, with_x=True, rope=None):
    """One forward into NaN-prefilled outputs with one row to spare each."""
    inp = ln_inputs(rows, D, dt)
    o = dict(s=nans(rows + 1, D, dtype=dt), out=nans(rows + 1, D, dtype=dt), mean=nans(rows + 1), rstd=nans(rows + 1))
    a = ln_args(dt, rows, D, inp, n_masks, with_x)
    a.s_out, a.out, a.mean, a.rstd = o["s"].data_ptr(), o["out"].data_ptr(), o["mean"].data_ptr(), o["rstd"].data_ptr()
    if rope is not None:
        o["rot"] = nans(rows + 1, D, dtype=dt)
        a.rot_out, a.rope_cos, a.rope_sin, a.rope_T = o["rot"].data_ptr(), rope[0].data_ptr(), rope[1].data_ptr(), rope[2]
    K.ln_fwd(a)
    torch.cuda.synchronize()
    for k, t in o.items():
        check_canary(t, rows, "ln_fwd " + k)
    return o


def ln_backward(dt, rows, D, n_masks, n_part, fwd, alias=False, dout2=False, dbranch=True):
    """One backward from the forward's stored s / mean / rstd into NaN-prefilled
    outputs: a spare row for ds and dbranch, a spare partial row for each partial."""
    inp = ln_inputs(rows, D, dt)
    ds = nans(rows + 1, D)
    if alias:
        ds[:rows] = inp["dout"]
    dbr = nans(rows + 1, D, dtype=dt) if dbranch else None
    part = nans(3, n_part + 1, D)
    a = ln_args(dt, rows, D, inp, n_masks)
    a.mean, a.rstd, a.s_in = fwd["mean"].data_ptr(), fwd["rstd"].data_ptr(), fwd["s"].data_ptr()
    a.dout, a.ds, a.dbranch = (ds if alias else inp["dout"]).data_ptr(), ds.data_ptr(), K.ptr(dbr)
    a.dgamma_part, a.dbeta_part, a.n_part = part[0].data_ptr(), part[1].data_ptr(), n_part
    a.dbranch_part = part[2].data_ptr() if dbranch else None
    if dout2:
        a.dout2 = inp["dout2"].data_ptr()
    K.ln_bwd(a)
    torch.cuda.synchronize()
    check_canary(ds, rows, "ln_bwd ds")
    if dbranch:
        check_canary(dbr, rows, "ln_bwd dbranch")
    for k in range(3 if dbranch else 2):
        check_canary(part[k], n_part, "ln_bwd partial %d" % k)
    if not dbranch:
        assert torch.isnan(part[2]).all(), "ln_bwd wrote dbranch_part without being given it"
    return ds, dbr, part


def ln_check_backward(dt, rows, D, n_masks, n_part, fwd, got, g, tag):
    ds, dbr, part = got
    inp = ln_inputs(rows, D, dt)
    rds, rdg, rdb = R.ln_bwd_ref(f64(fwd["s"][:rows]), f64(fwd["mean"][:rows]), f64(fwd["rstd"][:rows]), g,
                                 f64(inp["gamma"]))
    n = dname(dt)
    check(ds[:rows], rds, 1e-5, "ln_bwd ds " + n + tag)
    check(f64(part[0, :n_part]).sum(0), rdg, 1e-5, "ln_bwd dgamma " + n + tag)
    check(f64(part[1, :n_part]).sum(0), rdb, 1e-5, "ln_bwd dbeta " + n + tag)
    if dbr is not None:
        keep, scale = R.branch_mask(rows, D, n_masks, LN_P, LN_SEEDS)
        check_stored(dbr[:rows], rds * keep.double() * scale, 1e-5, "ln_bwd dbranch " + n + tag, dt)
        check(f64(part[2, :n_part]).sum(0), f64(dbr[:rows]).sum(0), 1e-5, "ln_bwd dbranch_part " + n + tag)


LN_CFGS = ["rows53_part3", "rows1_part1", "rows53_partmax"]


@pytest.mark.parametrize("cfg", LN_CFGS)
@pytest.mark.parametrize("n_masks", [0, 1, 2])
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("D", [128, 256, 512, 1024])
def test_layernorm_parity(D, dt, n_masks, cfg):
    """Forward (s_out, out, mean, rstd, the keep pattern; with x and with x = NULL)
    and backward (ds, dgamma, dbeta, dbranch with the hash mask at its position,
    dbranch_part; ds aliasing dout, dout2, dbranch = NULL) of every LayerNorm kernel:
    D = 128 (4 waves, contiguous lanes), 256 (four-column groups), 512 / 1024
    (eight-column groups, NK = 1 / 2).  rows = 53 with 3 partial blocks gives every
    wave 2-3 rows (the prefetch) and a partly empty last pass; the largest legal
    n_part leaves some waves without a row; p_drop > 0 with n_masks = 0 is no
    dropout.  Nothing is written past rows or past n_part."""
    nw = 8 if D % 256 == 0 else 4
    rows, n_part = {"rows53_part3": (53, 3), "rows1_part1": (1, 1), "rows53_partmax": (53, (53 + nw - 1) // nw)}[cfg]
    inp = ln_inputs(rows, D, dt)
    keep, _ = R.branch_mask(rows, D, n_masks, LN_P, LN_SEEDS)
    n = dname(dt)
    fwd = None
    for with_x in (False, True):
        o = ln_forward(dt, rows, D, n_masks, with_x)
        x = inp["x"] if with_x else None
        rs, ro, rm, rr = R.ln_fwd_ref(x, inp["y"], inp["gamma"], inp["beta"], LN_EPS, n_masks, LN_P, LN_SEEDS)
        check_stored(o["s"][:rows], rs, 2e-6, "ln_fwd s_out " + n, dt)
        check_stored(o["out"][:rows], ro, 2e-6, "ln_fwd out " + n, dt)
        check(o["mean"][:rows], rm, 2e-6, "ln_fwd mean " + n)
        check_rel(o["rstd"][:rows], rr, 1e-5, "ln_fwd rstd " + n)
        branch = f64(o["s"][:rows]) - (f64(x) if with_x else 0.0)
        assert torch.equal(branch != 0, keep), "keep pattern is not the dropout hash's (with_x=%s)" % with_x
        fwd = o
    g = f64(inp["dout"])
    plain = ln_backward(dt, rows, D, n_masks, n_part, fwd)
    ln_check_backward(dt, rows, D, n_masks, n_part, fwd, plain, g, "")
    aliased = ln_backward(dt, rows, D, n_masks, n_part, fwd, alias=True)
    assert torch.equal(aliased[0][:rows], plain[0][:rows]), "ds aliasing dout changed ds"
    assert torch.equal(aliased[1][:rows], plain[1][:rows]), "ds aliasing dout changed dbranch"
    assert torch.equal(aliased[2][:, :n_part], plain[2][:, :n_part]), "ds aliasing dout changed the partials"
    with2 = ln_backward(dt, rows, D, n_masks, n_part, fwd, dout2=True)
    ln_check_backward(dt, rows, D, n_masks, n_part, fwd, with2, g + f64(inp["dout2"]), " (dout2)")
    nobr = ln_backward(dt, rows, D, n_masks, n_part, fwd, dbranch=False)
    assert torch.equal(nobr[0][:rows], plain[0][:rows]), "dbranch = NULL changed ds"
    assert torch.equal(nobr[2][:2, :n_part], plain[2][:2, :n_part]), "dbranch = NULL changed dgamma / dbeta partials"


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("D", [256, 1024])
def test_layernorm_rot_out(D, dt):
    """rot_out rotates the stored (rounded) out by position row % rope_T; the rows
    cross the period five times."""
    rows, T, n_masks = 53, 10, 1
    cs, sn = rotation_tables(T, D, DEV)
    inp = ln_inputs(rows, D, dt)
    o = ln_forward(dt, rows, D, n_masks, True, rope=(cs, sn, T))
    ro = R.ln_fwd_ref(inp["x"], inp["y"], inp["gamma"], inp["beta"], LN_EPS, n_masks, LN_P, LN_SEEDS)[1]
    check_stored(o["out"][:rows], ro, 2e-6, "ln_fwd out " + dname(dt), dt)
    check_stored(o["rot"][:rows], R.rope_ref(f64(o["out"][:rows]), cs, sn, T, D), 2e-6, "ln_fwd rot_out " + dname(dt), dt)


# ---------------------------------------------------------------------------
# RoPE
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("inverse", [False, True], ids=["forward", "inverse"])
@pytest.mark.parametrize("dti,dto", [(F32, F32), (BF16, F32), (F32, BF16)], ids=["f32_f32", "bf16_f32", "f32_bf16"])
@pytest.mark.parametrize("cols,rope_dim", [(128, 128), (192, 64)])
def test_rope_parity(cols, rope_dim, dti, dto, inverse):
    """nstl_rope against the f64 rotation: rows cross the period twice (t = row % T),
    per-head tables over three heads (pair = (col % rope_dim) / 2), the input a column
    window of a wider matrix, both directions, and accumulation onto an f32 out with
    a padded row stride."""
    T = 7
    rows = 2 * T + 3
    wide = rnd(rows, 3 * cols, dtype=dti, seed=20)
    x = wide[:, cols:2 * cols]
    cs, sn = rotation_tables(T, rope_dim, DEV)
    ref = R.rope_ref(f64(x), cs, sn, T, rope_dim, inverse)
    out = nans(rows + 1, cols, dtype=dto)
    K.rope(x, 3 * cols, out, cols, rows, cols, cs, sn, T, rope_dim, inverse=inverse)
    torch.cuda.synchronize()
    check_canary(out, rows, "rope out")
    check_stored(out[:rows], ref, 2e-6, "rope " + dname(dto), dto)
    if dto == F32:
        ld = cols + 8
        acc0 = rnd(rows + 1, ld, seed=21)
        acc0[rows:] = NAN
        acc0[:, cols:] = NAN
        acc = acc0.clone()
        K.rope(x, 3 * cols, acc, ld, rows, cols, cs, sn, T, rope_dim, inverse=inverse, accumulate=True)
        torch.cuda.synchronize()
        check_canary(acc[:, :cols], rows, "rope accumulate")
        assert torch.isnan(acc[:, cols:]).all(), "rope wrote into the row padding"
        check(acc[:rows, :cols], f64(acc0[:rows, :cols]) + ref, 2e-6, "rope accumulate f32")


# ---------------------------------------------------------------------------
# cast, copy2d
# ---------------------------------------------------------------------------
CAST_BITS = [
    0x3F808000, 0x3F818000, 0xBF808000, 0xBF818000,  # ties: to even down / up, both signs
    0x3F808001, 0x3F807FFF, 0x3F818001, 0x3F817FFF,  # one f32 ulp either side of a tie
    0x00000000, 0x80000000,                          # +0, -0
    0x7F7FFFFF, 0xFF7FFFFF, 0x7F7F0000, 0x7F7F8000,  # largest finite f32 (rounds to inf), largest bf16, its tie
    0x7F800000, 0xFF800000,                          # +inf, -inf
    0x00000001, 0x00400000, 0x00008000, 0x00018000, 0x807FFFFF,  # subnormals (and their ties)
]


def cast_source(n):
    bits = torch.tensor(CAST_BITS, dtype=torch.int64)
    g = torch.Generator().manual_seed(30)
    body = torch.randn(max(n, 1), generator=g).view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    body[:min(n, len(CAST_BITS))] = bits[:min(n, len(CAST_BITS))]
    body = torch.where(body >= 2 ** 31, body - 2 ** 32, body).to(torch.int32)
    return body[:n].view(torch.float32)


@pytest.mark.parametrize("n", [0, 1, 1027])
def test_cast_bit_exact(n):
    """f32 -> bf16 is torch's round-to-nearest-even on every bit pattern (ties in both
    directions, signed zeros, overflow to inf, inf, subnormals); bf16 -> f32 is exact;
    n elements are written and no more."""
    pad = 8
    src = torch.zeros(n + pad)
    src[:n] = cast_source(n)
    src = src.to(DEV)
    dst = torch.full((n + pad,), 7.0, dtype=BF16, device=DEV)
    K.cast(src, dst, n)
    torch.cuda.synchronize()
    assert (dst[n:] == 7.0).all(), "cast wrote past n"
    want = src[:n].cpu().to(BF16)
    assert torch.equal(dst[:n].cpu().view(torch.int16), want.view(torch.int16))
    back = torch.full((n + pad,), 7.0, device=DEV)
    K.cast(dst, back, n)
    torch.cuda.synchronize()
    assert (back[n:] == 7.0).all(), "cast wrote past n"
    assert torch.equal(back[:n].cpu().view(torch.int32), want.float().view(torch.int32))


@pytest.mark.parametrize("dts,dtd", [(F32, F32), (F32, BF16), (BF16, F32), (BF16, BF16)],
                         ids=["f32_f32", "f32_bf16", "bf16_f32", "bf16_bf16"])
def test_copy2d_exact(dts, dtd):
    """copy2d is one f32 multiply and one rounding per element: bit-identical to torch
    on the CPU, for every dtype pair, with and without a scale, with zero-filled pad
    columns and with dst_cols == cols; the row padding and the rows past `rows` stay."""
    rows, cols, src_ld, dst_ld = 37, 61, 67, 72
    src = rnd(rows, src_ld, dtype=dts, seed=31)
    sc = torch.tensor([0.3], device=DEV)
    for scale, dst_cols in ((sc, 64), (None, 61)):
        dst = torch.full((rows + 1, dst_ld), 7.0, dtype=dtd, device=DEV)
        K.copy2d(src, src_ld, dst, dst_ld, rows, cols, dst_cols, scale=scale)
        torch.cuda.synchronize()
        want = src[:, :cols].cpu().float()
        if scale is not None:
            want = sc.cpu() * want
        assert torch.equal(dst[:rows, :cols].cpu(), want.to(dtd))
        assert (dst[:rows, cols:dst_cols] == 0).all()
        assert (dst[:rows, dst_cols:] == 7.0).all() and (dst[rows:] == 7.0).all(), "copy2d wrote past its extent"
    dst = torch.full((rows + 1, dst_ld), 7.0, dtype=dtd, device=DEV)
    K.copy2d(src, src_ld, dst, dst_ld, 0, cols, 64, scale=sc)
    torch.cuda.synchronize()
    assert (dst == 7.0).all(), "copy2d with rows = 0 touched dst"


# ---------------------------------------------------------------------------
# colsum and the row reducers
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("offset", [0, 1], ids=["aligned", "offset1"])
@pytest.mark.parametrize("rows,cols,ld", [(1, 8, 8), (255, 264, 264), (600, 61, 61), (300, 64, 200), (513, 256, 256)])
@pytest.mark.parametrize("dt", DTYPES)
def test_colsum_parity(dt, rows, cols, ld, offset):
    """nstl_colsum on the vector path (16-byte loads: cols and ld multiples of 8 bf16 /
    4 f32) and the scalar path (cols = 61, or a source one element off alignment): a
    single row, a 255-row chunk (the 4-row unroll's tail), three chunks with one row in
    the last, a second column block of 8 columns, ld > cols with NaN in the padding."""
    buf = rnd(rows * ld + 1, dtype=dt, seed=40)
    x = buf[offset:offset + rows * ld].view(rows, ld)
    x[:, cols:] = NAN
    nchunk = (rows + 255) // 256
    ref = f64(x[:, :cols]).sum(0)
    n = dname(dt)
    for beta in (0.0, 1.0):
        part = nans(nchunk + 1, cols)
        out0 = nans(cols + 1) if beta == 0.0 else torch.cat([rnd(cols, seed=41), nans(1)])
        out = out0.clone()
        K.colsum(x, ld, rows, cols, part, out, beta)
        torch.cuda.synchronize()
        check_canary(part, nchunk, "colsum partial")
        check_canary(out, cols, "colsum out")
        check(out[:cols], ref + (f64(out0[:cols]) if beta else 0.0), 1e-5, "colsum " + n)


@pytest.mark.parametrize("cols", [61, 64, 200])
@pytest.mark.parametrize("n_part", [1, 3, 16, 17, 35, 129, 260])
def test_row_reducers_parity(n_part, cols):
    """reduce_rows / reduce_rows_strided (4 row groups, 4-deep unroll: boundaries at
    n_part = 16 / 17), reduce_rows3 and reduce_rows_batch (16 row groups, 8-deep
    unroll: boundaries at 17, 129) against the f64 column sums: ld > cols with NaN in
    the padding, beta 0 over a NaN-prefilled out, beta 1, one to three matrices."""
    ld = cols + 3
    part = rnd(n_part, ld, seed=50)
    part[:, cols:] = NAN
    contig = part[:, :cols].contiguous()
    ref = f64(contig).sum(0)
    three = torch.cat([rnd(3, n_part, cols, seed=51), nans(3, 1, cols)], 1)  # a spare NaN row per matrix
    small = rnd(3, 5, seed=52)
    for beta in (0.0, 1.0):
        def fresh(seed):
            return nans(cols + 1) if beta == 0.0 else torch.cat([rnd(cols, seed=seed), nans(1)])

        def expect(out0, r):
            return r + (f64(out0[:cols]) if beta else 0.0)

        o0 = fresh(60)
        o = o0.clone()
        K.reduce_rows(contig, n_part, cols, o, beta)
        torch.cuda.synchronize()
        check_canary(o, cols, "reduce_rows out")
        check(o[:cols], expect(o0, ref), 1e-5, "reduce_rows")
        o = o0.clone()
        K.reduce_rows_strided(part, ld, n_part, cols, o, beta)
        torch.cuda.synchronize()
        check_canary(o, cols, "reduce_rows_strided out")
        check(o[:cols], expect(o0, ref), 1e-5, "reduce_rows_strided")
        oa, ob, oc = o0.clone(), o0.clone(), torch.zeros(5, device=DEV)
        K.reduce_rows_batch([(part, ld, n_part, cols, oa, beta), (small, 5, 3, 5, oc, 0.0),
                             (contig, cols, n_part, cols, ob, beta)])
        torch.cuda.synchronize()
        for t in (oa, ob):
            check_canary(t, cols, "reduce_rows_batch out")
            check(t[:cols], expect(o0, ref), 1e-5, "reduce_rows_batch")
        check(oc, f64(small).sum(0), 1e-5, "reduce_rows_batch")
        for n_mat in (1, 2, 3):
            o0s = [fresh(70 + k) for k in range(n_mat)]
            outs = [t.clone() for t in o0s]
            K.reduce_rows3(three, n_part, cols, outs, beta)
            torch.cuda.synchronize()
            for k in range(n_mat):
                check_canary(outs[k], cols, "reduce_rows3 out")
                check(outs[k][:cols], expect(o0s[k], f64(three[k, :n_part]).sum(0)), 1e-5, "reduce_rows3")


# ---------------------------------------------------------------------------
# sumsq, shard_sum, clip_coef
# ---------------------------------------------------------------------------
def slice_sumsq_ref(g, n, n_partial):
    per = (n + n_partial - 1) // n_partial
    g = f64(g)
    return torch.stack([(g[min(n, b * per):min(n, (b + 1) * per)] ** 2).sum() for b in range(n_partial)]), per


@pytest.mark.parametrize("n,n_partial", [(1, 1), (3, 7), (5, 1024), (1023, 7), (4099, 64)])
def test_sumsq_slices(n, n_partial):
    """partial[b] is the sum of squares of slice [b*per, min(n, (b+1)*per)), per =
    ceil(n / n_partial): n < 4 (no vector body), n < n_partial (empty blocks give
    exactly 0), slices that start off 16-byte alignment, one block.  1e-6 per element:
    f32 squares and pair sums (2 roundings), a double accumulator, one rounding out."""
    g = rnd(n, seed=80)
    part = nans(n_partial + 1)
    K.sumsq(g, n, part, n_partial)
    torch.cuda.synchronize()
    check_canary(part, n_partial, "sumsq partial")
    ref, per = slice_sumsq_ref(g, n, n_partial)
    empty = torch.arange(n_partial) * per >= n
    assert (part[:n_partial].cpu()[empty] == 0).all(), "an empty block's partial is not 0"
    check_rel(part[:n_partial].cpu()[~empty], ref[~empty], 1e-6, "sumsq partial")


@pytest.mark.parametrize("n_partial", [1, 7, 64])
@pytest.mark.parametrize("n_slots", [0, 1, 3, 7])
def test_shard_sum_bit_identical(n_slots, n_partial):
    """out is own + slot 0 + slot 1 + ... in f32, in that order, and the partials are
    nstl_sumsq's of that out, bit for bit: n % 4 != 0, a slot stride above n (NaN in
    the padding), blocks that start off 16-byte alignment."""
    n, ld = 4099, 4104
    own = rnd(n, seed=90)
    slots = None
    want = own.cpu().clone()
    if n_slots:
        slots = rnd(n_slots, ld, seed=91)
        slots[:, n:] = NAN
        for k in range(n_slots):
            want = want + slots[k, :n].cpu()
    out = nans(n + 5)
    part = nans(n_partial + 1)
    K.shard_sum(own, slots, n_slots, out, part, n_partial)
    torch.cuda.synchronize()
    check_canary(out, n, "shard_sum out")
    check_canary(part, n_partial, "shard_sum partial")
    assert torch.equal(out[:n].cpu(), want), "out is not own + the slots in slot order"
    part2 = nans(n_partial + 1)
    K.sumsq(out, n, part2, n_partial)
    torch.cuda.synchronize()
    assert torch.equal(part[:n_partial], part2[:n_partial]), "partials differ from nstl_sumsq of the summed shard"
    check_rel(part[:n_partial], slice_sumsq_ref(want, n, n_partial)[0], 1e-6, "shard_sum partial")


def clip_partials(n_partial):
    g = torch.Generator().manual_seed(100 + n_partial)
    part = nans(n_partial + 1)  # a NaN past the end: reading it poisons the norm
    part[:n_partial] = (0.1 + torch.rand(n_partial, generator=g)).to(DEV)
    return part


def run_clip(part, n_partial, max_norm, with_norm=True):
    coef, norm = nans(2), nans(2)
    K.clip_coef(part, n_partial, max_norm, coef, norm if with_norm else None)
    torch.cuda.synchronize()
    check_canary(coef, 1, "clip_coef coef")
    check_canary(norm, 1 if with_norm else 0, "clip_coef norm")
    return coef[:1].cpu(), norm[:1].cpu()


@pytest.mark.parametrize("n_partial", [1, 64, 1000, 1024, 1025, 8191, 8197, 28000])
def test_clip_coef_parity(n_partial):
    """nstl_clip_coef on the one-wave kernel (<= 1024 partials) and the 1024-thread
    kernel (8 x unrolled pass and its tail: 8191 leaves one thread, 8197 five, to the
    tail alone; 28000 is the production count): norm and coef against f64, the
    unclipped branch exactly 1, norm_out = NULL."""
    part = clip_partials(n_partial)
    true_norm = R.clip_ref(part[:n_partial], 1.0)[0]
    for max_norm, clipped in ((f32v(0.5 * true_norm), True), (f32v(2.0 * true_norm), False)):
        coef, norm = run_clip(part, n_partial, max_norm)
        rn, rc = R.clip_ref(part[:n_partial], max_norm)
        check_rel(norm, torch.tensor([rn], dtype=torch.float64), 1e-6, "clip_coef norm")
        if clipped:
            check_rel(coef, torch.tensor([rc], dtype=torch.float64), 1e-6, "clip_coef coef")
        else:
            assert rc == 1.0 and coef.item() == 1.0, coef.item()
        coef2, _ = run_clip(part, n_partial, max_norm, with_norm=False)
        assert torch.equal(coef, coef2), "norm_out = NULL changed coef"


def test_clip_coef_kernels_meet():
    """The same 1024 partials through the one-wave kernel and, with one 0 appended,
    through the 1024-thread kernel: norm and coef bit-identical."""
    part = nans(1026)
    part[:1024] = clip_partials(1024)[:1024]
    part[1024] = 0.0
    max_norm = f32v(0.5 * R.clip_ref(part[:1024], 1.0)[0])
    c1, n1 = run_clip(part, 1024, max_norm)
    c2, n2 = run_clip(part, 1025, max_norm)
    assert torch.equal(n1, n2) and torch.equal(c1, c2), (n1.item(), n2.item(), c1.item(), c2.item())


# ---------------------------------------------------------------------------
# Adam
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("clipped", [True, False], ids=["clipped", "unclipped"])
@pytest.mark.parametrize("step", [1, 1000])
@pytest.mark.parametrize("wd", [0.0, 1e-2])
@pytest.mark.parametrize("lowp", [None, BF16, F32], ids=["nolowp", "lowp_bf16", "lowp_f32"])
@pytest.mark.parametrize("n", [1, 1000, 70001])
def test_adam_parity(n, lowp, wd, step, clipped, monkeypatch):
    """nstl_adam_step on both paths (sumsq partials: adam_kernel; device coef:
    adam_gcoef_kernel with its two-element pass and tail) against adam_ref fed the
    kernel's own coef and the f32 hyperparameters it receives: p at rtol 1e-5 + atol
    1e-6; m and v at rtol 1e-5 + 1e-6 max|ref| (a handful of f32 roundings, each 6e-8
    of the larger operand).  The shadow copy is the rounded new p (or absent), the two
    paths and NSTL_ADAM_NT=0 are bit-identical, nothing is written past n."""
    lr, b1, b2, eps, n_partial, pad = 1e-3, 0.9, 0.999, 1e-8, 64, 3
    g = rnd(n, scale=0.01, seed=110)
    p0 = rnd(n, seed=111)
    if step == 1:
        m0, v0 = torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    else:
        m0, v0 = rnd(n, scale=0.01, seed=112), rnd(n, scale=1e-4, seed=113).abs()
    part = nans(n_partial + 1)
    K.sumsq(g, n, part, n_partial)
    true_norm = f64(g).norm().item()
    max_norm = f32v((0.5 if clipped else 2.0) * true_norm)
    coef, norm = nans(2), nans(2)
    K.clip_coef(part, n_partial, max_norm, coef, norm)
    torch.cuda.synchronize()
    check_rel(norm[:1], torch.tensor([true_norm], dtype=torch.float64), 1e-6, "adam norm")
    assert (coef[0].item() < 1.0) == clipped and (clipped or coef[0].item() == 1.0)
    check_rel(coef[:1], torch.tensor([R.clip_ref(part[:n_partial], max_norm)[1]], dtype=torch.float64), 1e-6, "adam coef")

    def run(path):
        bufs = [torch.cat([t, nans(pad)]) for t in (p0, m0, v0)]
        shadow = None if lowp is None else nans(n + pad, dtype=lowp)
        norm_out = nans(2)
        a = K.AdamArgs()
        a.p, a.g, a.m, a.v = bufs[0].data_ptr(), g.data_ptr(), bufs[1].data_ptr(), bufs[2].data_ptr()
        a.p_lowp, a.lowp_dtype, a.n = K.ptr(shadow), (K.dtype_code(lowp) if lowp is not None else K.F32), n
        a.lr, a.beta1, a.beta2, a.eps, a.weight_decay = lr, b1, b2, eps, wd
        a.step, a.max_norm = step, max_norm
        if path == "sumsq":
            a.sumsq_partial, a.n_partial, a.norm_out = part.data_ptr(), n_partial, norm_out.data_ptr()
        else:
            a.coef = coef.data_ptr()
        K.adam_step(a)
        torch.cuda.synchronize()
        for t, what in zip(bufs, "pmv"):
            check_canary(t, n, "adam " + what)
        if shadow is not None:
            check_canary(shadow, n, "adam shadow")
            assert torch.equal(shadow[:n], bufs[0][:n].to(lowp)), "the shadow copy is not the rounded new p"
        if path == "sumsq":
            assert torch.equal(norm_out[:1], norm[:1]), "adam_kernel's norm differs from nstl_clip_coef's"
        return [t[:n] for t in bufs] + ([shadow[:n]] if shadow is not None else [])

    by_sumsq = run("sumsq")
    by_coef = run("coef")
    monkeypatch.setenv("NSTL_ADAM_NT", "0")
    by_coef_plain = run("coef")
    for name, x, y, z in zip(("p", "m", "v", "shadow"), by_sumsq, by_coef, by_coef_plain):
        assert torch.equal(x, y), "sumsq path vs coef path: " + name
        assert torch.equal(y, z), "NSTL_ADAM_NT=0 changed " + name
    rp, rm, rv = R.adam_ref(p0, g, m0, v0, step, f32v(lr), f32v(b1), f32v(b2), f32v(eps), f32v(wd), coef[0].item())
    check_rel(by_coef[0], rp, 1e-5, "adam p", atol=1e-6)
    check_rel(by_coef[1], rm, 1e-5, "adam m", atol=1e-6 * rm.abs().max().item())
    check_rel(by_coef[2], rv, 1e-5, "adam v", atol=1e-6 * rv.abs().max().item())
