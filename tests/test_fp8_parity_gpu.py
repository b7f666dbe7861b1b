"""The fp8 operand path of config C5 on the MI355X, per element: the quantisation
kernels (csrc/fp8.hip) bit for bit against tests/fp8_table_ref.py, an e4m3 encoder
that does not use torch's cast, on rows that hit every rounding tie; the fp8 ring
kernel (gemm256f8_kernel, csrc/gemm.hip) and the 4-wave persistent kernel
(gemm4f8_kernel, csrc/gemm4.h) against tests/gemm_ref.py's f64 product of the decoded
code bytes, under gemm_ref.bound with e = gemm_ref.e8(K): e mag for f32 C, 2^-8 |ref| +
(1 + 2^-8) e mag for bf16 C; e is E32 = 1e-5 except at K = 64 and 128, where one or two
scaled MFMA instructions alone exceed it and e is twice what the stand-alone probe
tools/fp8_mfma_accum_probe.py shows (profiles/fp8_mfma_accum.txt; see gemm_ref.py).  gemm4f8 holds the C5 T = 256 rotation
table in LDS as bf16: its rotated columns get 2^-8 mag more (one bf16 rounding each of
cos and sin; mag is already rope_mag of the pre-rotation magnitude).

Every GEMM case pads the operand rows with 0x7F bytes (the e4m3 NaN), follows the M /
N scale entries with NaN, gives C as an [M + 2][ldc] NaN-filled buffer and asserts
through the launch counters which kernel ran.  No element is excluded.

The column-sum partials of the dReLU epilogue are compared row by row with the f64
column sums of the stored values of their 128 rows, under n 2^-24 sum|stored| with n
the roundings of the sum read from the code: the ring epilogue adds 16 values per
lane and folds 8 lanes in 3 steps (gemm.hip ring_epi: 19), gemm4f8 adds 8 per lane
and folds 16 lanes in 4 steps (gemm4.h epilogue: 12).

NSTL_FP8_PARITY_ERRORS_OUT=<file>: the worst err / bound of every case is written
(profiles/fp8_parity_errors.txt is such a run)."""
import os

import numpy as np
import pytest
import torch

from oracle import fp8_ref
from tests import fp8_table_ref as F8
from tests import gemm_ref as G
from tests.test_gemm_parity_gpu import BF16, F32, NAN, P, SEED, Out, bias_of, nans

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from neurosync_trainer_lite_amd import _hip as K
    from neurosync_trainer_lite_amd.engine import rotation_tables

DEV = "cuda:0"
E4M3 = torch.float8_e4m3fn
COUNTERS = ("gemm128", "gemm_ring", "gemm4", "gemm_fp8", "gemm4_fp8", "gemm_fp8_rope", "gemm4_tiles")
U32 = 2.0 ** -24

_ERRORS = {}


@pytest.fixture(scope="module", autouse=True)
def _error_report():
    yield
    path = os.environ.get("NSTL_FP8_PARITY_ERRORS_OUT")
    if path and _ERRORS:
        with open(path, "w") as f:
            f.write("# tests/test_fp8_parity_gpu.py: worst |got - ref| / bound of every GEMM case (bound: f32 C e mag;\n")
            f.write("# bf16 C 2^-8 |ref| + (1 + 2^-8) e mag, + 2^-8 mag on columns rotated by a bf16 table; e = 1e-5,\n")
            f.write("# at K = 64 / 128 4.598e-5 / 2.834e-5 from the MFMA probe; tests/gemm_ref.py).  The quantisation cases are bit-exact comparisons and have no ratio.\n")
            f.write("# %-86s %s\n" % ("case", "err / bound"))
            for what in sorted(_ERRORS):
                f.write("%-88s %.4f\n" % (what, _ERRORS[what]))


def rnd_cpu(*shape, seed=0, scale=1.0, dtype=F32):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g, dtype=torch.float64) * scale).to(dtype)


# ---------------------------------------------------------------------------
# quantisation: codes and scales bit for bit
# ---------------------------------------------------------------------------
def row_job(x, ldx=None, ldq=None):
    """Buffers of one nstl_fp8_quant_rows job for the CPU tensor x [rows][cols]: x with
    NaN padding up to ldx, q [rows + 1][ldq] prefilled 0xAA, scale [rows + 1] NaN."""
    rows, cols = x.shape
    ldx, ldq = ldx or cols, ldq or cols
    xb = torch.full((rows, ldx), NAN, dtype=x.dtype, device=DEV)
    xb[:, :cols] = x.to(DEV)
    qb = torch.full((rows + 1, ldq), 0xAA, dtype=torch.uint8, device=DEV)
    sb = nans(rows + 1)
    return (xb, rows, cols, qb.view(E4M3), sb), (x, qb, sb)


def check_row_job(x, qb, sb, what, transposed=False):
    """q, scale against the table reference of x (of x^T for the column kernel); the
    prefill outside the [rows][cols] window of q and after scale survives."""
    ref_q, ref_s = F8.quant_rows_ref(x.T.contiguous() if transposed else x)
    n, w = ref_q.shape
    q, s = qb.cpu().numpy(), sb.cpu().numpy()
    assert np.array_equal(s[:n], ref_s), what + ": scales differ"
    bad = np.argwhere(q[:n, :w] != ref_q)
    assert bad.size == 0, "%s: %d codes differ, first at %s: 0x%02x, reference 0x%02x" % (
        what, len(bad), bad[0].tolist(), q[tuple(bad[0])], ref_q[tuple(bad[0])])
    assert (q[:n, w:] == 0xAA).all() and (q[n:] == 0xAA).all(), what + ": wrote outside the window of q"
    assert np.isnan(s[n:]).all(), what + ": wrote past the scales"


def quant_rows_one(x, what, **ld):
    job, bufs = row_job(x, **ld)
    K.fp8_quant_rows([job])
    torch.cuda.synchronize()
    check_row_job(*bufs, what)


def test_quant_rows_ties_f32():
    """amax == 448 (inv == 1): every midpoint of adjacent codes, the subnormal ones, 2^-10,
    their f32 neighbours, +-0 and +-448; and rows on which 448 / amax differs from
    1 / (amax / 448) with elements that x inv puts exactly on a midpoint."""
    quant_rows_one(torch.from_numpy(F8.tie_rows()), "tie rows f32", ldx=520, ldq=528)
    quant_rows_one(torch.from_numpy(F8.inv_mutant_rows()), "inv rows f32")


def test_quant_rows_ties_bf16():
    """The tie values a bf16 holds exactly (code values and midpoints: at most 5
    significant bits; their f32 neighbours are not representable)."""
    v = F8.tie_values()
    v = v[v == torch.from_numpy(v).bfloat16().float().numpy()]
    assert v.size >= 2 + 127 + 126
    x = np.zeros((2, -(-v.size // 16) * 16), dtype=np.float32)
    x[0, :v.size], x[1, :v.size] = v, -v
    quant_rows_one(torch.from_numpy(x).bfloat16(), "tie rows bf16", ldq=x.shape[1] + 16)


def data_rows(rows, cols, dtype, seed):
    x = rnd_cpu(rows, cols, seed=seed, dtype=dtype)
    x[0] = 0                      # all-zero row: scale 1, codes 0
    if rows > 2:
        x[1] *= 1e-6
        x[2, :cols // 2] *= 1e4   # wide range inside a row: subnormal codes and zeros
    return x


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("cols", [16, 528, 1040, 4096])
def test_quant_rows_widths_strides(cols, dtype):
    """7 rows (not a multiple of the 4 rows per block), ldx > cols with NaN padding,
    ldq > cols.  4096 wide bf16: the register kernel; everything else two passes."""
    quant_rows_one(data_rows(7, cols, dtype, cols), "rows 7x%d" % cols, ldx=cols + 8, ldq=cols + 16)


def test_quant_rows_grid_stride_past_4096_blocks():
    quant_rows_one(data_rows(16388, 16, F32, 5), "rows 16388x16", ldx=24, ldq=32)


@pytest.mark.parametrize("shapes", [[(5, 528), (130, 4096), (64, 16)], [(6, 4096), (131, 4096)]],
                         ids=["mixed-widths-two-pass", "4096-register"])
def test_quant_rows_batches(shapes):
    """Jobs of different row counts in one launch (the grid covers the tallest); widths
    that differ take the two-pass kernel also for the 4096-wide job, two 4096-wide bf16
    jobs the register kernel."""
    jobs, bufs = zip(*(row_job(data_rows(r, c, BF16, r + c), ldx=c + 8, ldq=c + 16) for r, c in shapes))
    K.fp8_quant_rows(list(jobs))
    torch.cuda.synchronize()
    for (r, c), b in zip(shapes, bufs):
        check_row_job(*b, "batch job %dx%d" % (r, c))


def col_job(x, ldx=None, ldq=None):
    rows, cols = x.shape
    ldx, ldq = ldx or cols, ldq or rows
    xb = torch.full((rows, ldx), NAN, dtype=x.dtype, device=DEV)
    xb[:, :cols] = x.to(DEV)
    qb = torch.full((cols + 1, ldq), 0xAA, dtype=torch.uint8, device=DEV)
    sb = nans(cols + 1)
    sb[:cols] = 1e30  # stale large values: the kernel's atomic max must start from its own zeros
    return (xb, rows, cols, qb.view(E4M3), sb), (x, qb, sb)


def data_cols(rows, cols, dtype, seed):
    x = rnd_cpu(rows, cols, seed=seed, dtype=dtype)
    x[:, 0] = 0
    x[:, 1] *= 1e-6
    x[: rows // 2, 2] *= 1e4
    return x


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
def test_quant_cols(dtype):
    """64x64, 128x192 and 192x64 alone and as one batch of three (tiles outside a
    smaller job: the qc_tile guard), ldx > cols NaN padding, ldq = rows + 16."""
    shapes = [(64, 64), (128, 192), (192, 64)]
    for group in [[s] for s in shapes[:2]] + [shapes]:
        jobs, bufs = zip(*(col_job(data_cols(r, c, dtype, r + c), ldx=c + 8, ldq=r + 16) for r, c in group))
        K.fp8_quant_cols(list(jobs))
        torch.cuda.synchronize()
        for (r, c), b in zip(group, bufs):
            check_row_job(*b, "cols job %dx%d of %d" % (r, c, len(group)), transposed=True)


def test_quant_cols_ties():
    """The tie values down the columns (amax 448 in each)."""
    v = F8.tie_values()
    cols = -(-(-(-v.size // 63)) // 64) * 64  # 63 values per column under a first row of 448
    x = np.zeros((64, cols), dtype=np.float32)
    x[0] = 448.0
    body = np.zeros(63 * cols, dtype=np.float32)
    body[:v.size] = v
    x[1:] = body.reshape(63, cols)
    x[:, 1::2] *= -1
    job, bufs = col_job(torch.from_numpy(x), ldq=80)
    K.fp8_quant_cols([job])
    torch.cuda.synchronize()
    check_row_job(*bufs, "cols ties", transposed=True)


def test_quant_rejections():
    x = torch.zeros(64, 64, device=DEV)
    q = torch.zeros(80, 80, dtype=torch.uint8, device=DEV)
    s = torch.zeros(80, device=DEV)
    with pytest.raises(RuntimeError, match="multiple of 16"):
        K.fp8_quant_rows([(x, 64, 24, q.view(E4M3), s)])
    with pytest.raises(RuntimeError, match="multiples of 64"):
        K.fp8_quant_cols([(x, 32, 64, q.view(E4M3), s)])
    off = q.view(-1)[8:8 + 64 * 80].view(64, 80).view(E4M3)  # 8 bytes off the 16-byte alignment
    with pytest.raises(RuntimeError, match="ldq"):
        K.fp8_quant_rows([(x, 64, 64, off, s)])
    with pytest.raises(RuntimeError, match="ldq"):
        K.fp8_quant_cols([(x, 64, 64, off, s)])
    torch.cuda.synchronize()
    assert not q.any() and not s.any()


# ---------------------------------------------------------------------------
# the GEMM kernels
# ---------------------------------------------------------------------------
def f8_operand(rows, Kd, pad, seed, scale=1.0):
    """(codes float8 [rows][Kd + pad] with 0x7F in the padding, scale f32 [rows] followed
    by a NaN) of a random matrix, quantised on the CPU by the oracle's torch code (any
    valid codes and scales make a GEMM input; the quantisers are judged above)."""
    q, s = fp8_ref.quant_rows(rnd_cpu(rows, Kd, seed=seed, scale=scale))
    buf = torch.full((rows, Kd + pad), 0x7F, dtype=torch.uint8)
    buf[:, :Kd] = q.view(torch.uint8)
    sb = torch.full((rows + 1,), NAN)
    sb[:rows] = s
    return buf.to(DEV).view(E4M3), sb.to(DEV)[:rows]


def check_counts(expect, what):
    c = K.kernel_counts()
    for name in COUNTERS:
        assert c[name] == expect.get(name, 0), "%s: %s launches %d, expected %d (%s)" % (
            what, name, c[name], expect.get(name, 0), {n: c[n] for n in COUNTERS})


def ring_counts(epilogue=0):
    return {"gemm_fp8": 1, "gemm_fp8_rope": int(epilogue == G.EPI_BIAS_ROPE)}


def g4_counts(M, N, epilogue=0):
    return dict(ring_counts(epilogue), gemm4_fp8=1, gemm4_tiles=(M // 256) * (N // 256))


def judge(got, ref, mag, c_dtype, what, Kd, extra=None):
    """|got - ref| <= gemm_ref.bound with e8(K) (+ extra) per element; a NaN in got fails."""
    assert got.shape == ref.shape and (mag >= ref.abs()).all(), what
    bnd = G.bound(ref, mag, c_dtype, G.e8(Kd))
    if extra is not None:
        bnd = bnd + extra
    err = (got.double() - ref).abs()
    ratio = (err / bnd.clamp_min(1e-300)).max().item()
    print("%s: worst err / bound %.4f (max |err| %.3e, max |ref| %.3e)" % (what, ratio, err.max().item(),
                                                                         ref.abs().max().item()))
    _ERRORS[what] = ratio
    assert not torch.isnan(got.float()).any(), what + ": NaN in (or no write to) the window of C"
    assert ratio <= 1.0, "%s: worst element at %.4f of its bound" % (what, ratio)
    return bnd


def run8(what, M, N, Kd, expect, *, c_dtype=BF16, pads=(16, 32), ldc=None, c_off=0, alpha=0.75, epilogue=0, bias=None,
         p_drop=0.0, seed=0, rope=None, rope_cols=0, aux=None, ld_aux=0, relu_mask=None, colsum_part=None, in_seed=1,
         bf16_table=False):
    """One fp8 nstl_gemm call judged by the reference.  Returns the Out (stored C), with
    .ref and .bound."""
    A, sa = f8_operand(M, Kd, pads[0], in_seed)
    B, sb = f8_operand(N, Kd, pads[1], in_seed + 1, scale=0.1)
    ldc = N if ldc is None else ldc
    out = Out(M, N, ldc, c_dtype, c_off)
    kw = dict(alpha=alpha, epilogue=epilogue, bias=bias, p_drop=p_drop, seed=seed, rope=rope, rope_cols=rope_cols,
              aux=aux)
    K.kernel_counts_reset()
    K.gemm(A, B, out.C, M, N, Kd, lda=A.stride(0), ldb=B.stride(0), ldc=ldc, ld_aux=ld_aux, relu_mask=relu_mask,
           colsum_part=colsum_part, a_scale=sa, b_scale=sb, **kw)
    torch.cuda.synchronize()
    check_counts(expect, what)
    ref, mag = G.gemm_ref(A, B, M, N, Kd, a_scale=sa, b_scale=sb, **kw)
    out.check_canaries(what)
    extra = None
    if bf16_table:
        extra = torch.zeros_like(mag)
        extra[:, :rope_cols] = G.BF16_HALF_ULP * mag[:, :rope_cols]
    out.ref, out.bound = ref, judge(out.window(), ref, mag, c_dtype, what, Kd, extra)
    return out


def check_keep_pattern(out, what):
    keep = torch.from_numpy(G.keep_flat(SEED, out.M, out.N, P)).to(DEV)
    assert torch.equal(out.window() != 0, keep), what + ": the zero pattern is not keep_flat(seed, M, N, p)"


def mask_of(M, N):
    return torch.zeros(((M + 63) // 64) * 8 * ((N + 7) // 8), dtype=torch.int64, device=DEV)


def check_colsum_rows(part, rows, out, n_round, what):
    """colsum_part [rows + 1][N] (NaN-prefilled: `rows` partial rows and a canary row):
    each partial row against the f64 column sums of the stored values of its 128 rows."""
    assert torch.isnan(part[rows:]).all(), what + ": wrote past its nstl_gemm_colsum_rows rows"
    assert not torch.isnan(part[:rows]).any(), what + ": a partial row was not written"
    st = out.window().double()
    worst = 0.0
    for r in range(rows):
        blk = st[128 * r:128 * (r + 1)]
        bnd = n_round * U32 * blk.abs().sum(0)
        err = (part[r].double() - blk.sum(0)).abs()
        assert (err <= bnd).all(), (what, r, (err / bnd.clamp_min(1e-300)).max().item())
        worst = max(worst, (err / bnd.clamp_min(1e-300)).max().item())
    print("%s: worst partial at %.4f of %d 2^-24 sum|stored|" % (what, worst, n_round))
    _ERRORS["%s (%d 2^-24 sum|stored| per partial)" % (what, n_round)] = worst


RING_MN = [(300, 257), (129, 256), (256, 72)]
RING_K = [64, 128, 192, 256, 320]  # 1..5 K steps through the three-deep staging


@pytest.mark.parametrize("Kd", RING_K)
@pytest.mark.parametrize("M,N", RING_MN)
def test_ring_f8_k_steps_partial_tiles(M, N, Kd):
    """f32 C without epilogue at ldc = N + 3, bf16 C at ldc N, N + 8 and N + 3."""
    run8("ring8 %dx%dx%d ->f32 ldc N+3" % (M, N, Kd), M, N, Kd, ring_counts(), c_dtype=F32, ldc=N + 3)
    for pad in (0, 8, 3):
        run8("ring8 %dx%dx%d ->bf16 ldc N+%d" % (M, N, Kd, pad), M, N, Kd, ring_counts(), ldc=N + pad)


@pytest.mark.parametrize("M,N", RING_MN)
def test_ring_f8_bias_and_unaligned_c(M, N):
    for Kd in (64, 320):
        run8("ring8 %dx%dx%d bias ldc N+8" % (M, N, Kd), M, N, Kd, ring_counts(), ldc=N + 8, epilogue=G.EPI_BIAS,
             bias=bias_of(N, "rand"))
    run8("ring8 %dx%dx192 bias ldc N+8 C one element off" % (M, N), M, N, 192, ring_counts(), ldc=N + 8, c_off=1,
         epilogue=G.EPI_BIAS, bias=bias_of(N, "rand"))


@pytest.mark.parametrize("bias_kind", ["pos", "rand"])
@pytest.mark.parametrize("M,N", [(129, 256), (256, 72), (300, 258)])
def test_ring_f8_relu_dropout_with_and_without_mask(M, N, bias_kind):
    """p = 0.3 with the 64-bit seed, ldc != N; h identical with a relu_mask; with a +50
    bias the zero pattern is keep_flat.  (300, 258): both directions partial, even N."""
    what = "ring8 relu-drop %dx%dx192 bias %s" % (M, N, bias_kind)
    kw = dict(ldc=N + 8, epilogue=G.EPI_BIAS_RELU_DROP, bias=bias_of(N, bias_kind), p_drop=P, seed=SEED)
    h = run8(what, M, N, 192, ring_counts(), **kw)
    hm = run8(what + " +mask", M, N, 192, ring_counts(), relu_mask=mask_of(M, N), **kw)
    assert torch.equal(h.window(), hm.window())
    if bias_kind == "pos":
        check_keep_pattern(h, what)


@pytest.mark.parametrize("M,N,T,dim,rc", [(300, 257, 100, 64, 128), (129, 256, 64, 32, 96), (256, 72, 100, 64, 64)])
def test_ring_f8_rope(M, N, T, dim, rc):
    cs, sn = rotation_tables(T, dim, DEV)
    run8("ring8 rope %dx%dx128 T%d dim%d cols%d" % (M, N, T, dim, rc), M, N, 128, ring_counts(G.EPI_BIAS_ROPE), ldc=N + 8,
         epilogue=G.EPI_BIAS_ROPE, bias=bias_of(N, "rand"), rope=(cs, sn, T, dim), rope_cols=rc)


@pytest.mark.parametrize("M,N", [(1800, 72), (300, 256)])
def test_ring_f8_drelu_aux_mask_colsum(M, N):
    """dReLU from the saved activation (ld_aux = N + 8, NaN padding) and from the
    forward's keep&positive bits: the same output; M % 256 in 1..128: the last tile's
    lower waves hold no row of C and must write no partial row (the canary row)."""
    Kd = 128
    fkw = dict(ldc=N + 8, epilogue=G.EPI_BIAS_RELU_DROP, bias=bias_of(N, "rand"), p_drop=P, seed=SEED)
    mask = mask_of(M, N)
    h = run8("ring8 drelu %dx%d: forward h" % (M, N), M, N, Kd, ring_counts(), relu_mask=mask, **fkw)
    aux = nans(M, N + 8, dtype=BF16)
    aux[:, :N] = h.window()
    bkw = dict(ldc=N + 8, epilogue=G.EPI_DRELU_DROP, aux=aux, ld_aux=N + 8, p_drop=P, in_seed=11)
    d_aux = run8("ring8 drelu %dx%d from aux" % (M, N), M, N, Kd, ring_counts(), **bkw)
    A, sa = f8_operand(M, Kd, 16, 11)
    B, sb = f8_operand(N, Kd, 32, 12, scale=0.1)
    rows = K.gemm_colsum_rows(A, B, d_aux.C, M, N, Kd, lda=A.stride(0), ldb=B.stride(0), ldc=N + 8,
                              epilogue=G.EPI_DRELU_DROP, aux=aux, ld_aux=N + 8, p_drop=P, a_scale=sa, b_scale=sb)
    assert rows == (M + 127) // 128
    part = nans(rows + 1, N)
    d_mask = run8("ring8 drelu %dx%d from mask + colsum" % (M, N), M, N, Kd, ring_counts(), relu_mask=mask,
                  colsum_part=part, **bkw)
    assert torch.equal(d_aux.window(), d_mask.window())
    check_colsum_rows(part, rows, d_mask, 19, "ring8 drelu %dx%d colsum" % (M, N))


def test_ring_f8_refusals():
    M, N, Kd = 300, 257, 64
    A, sa = f8_operand(M, Kd, 16, 1)
    B, sb = f8_operand(N, Kd, 32, 2)
    kw = dict(lda=A.stride(0), ldb=B.stride(0), a_scale=sa, b_scale=sb)
    cb, cf = Out(M, N, N + 3, BF16), Out(M, N, N + 3, F32)
    bias = bias_of(N, "rand")
    with pytest.raises(RuntimeError, match="FP8 supports"):  # odd N with ReLU-dropout
        K.gemm(A, B, cb.C, M, N, Kd, ldc=N + 3, epilogue=G.EPI_BIAS_RELU_DROP, bias=bias, p_drop=P, seed=SEED, **kw)
    with pytest.raises(RuntimeError, match="FP8 supports"):  # f32 C with a bias
        K.gemm(A, B, cf.C, M, N, Kd, ldc=N + 3, epilogue=G.EPI_BIAS, bias=bias, **kw)
    with pytest.raises(RuntimeError, match="FP8 supports"):  # beta != 0 with bf16 C
        K.gemm(A, B, cb.C, M, N, Kd, ldc=N + 3, beta=1.0, **kw)
    with pytest.raises(RuntimeError, match="no split-K"):
        K.gemm(A, B, cf.C, M, N, Kd, ldc=N + 3, split_k=2, workspace=nans(2 * M * N), **kw)
    torch.cuda.synchronize()
    assert torch.isnan(cb.buf.float()).all() and torch.isnan(cf.buf).all()


# gemm4f8: full 256 x 256 tiles, K % 256 == 0, K >= 512
G4_SHAPES = [(256, 256, 512), (512, 256, 768), (256, 512, 1024)]


def both(what, M, N, Kd, monkeypatch, epilogue=0, **kw):
    """The call on gemm4f8 and, with NSTL_GEMM4_F8=0, on the ring kernel: each by the
    reference, and with each other under the sum of their two bounds."""
    monkeypatch.delenv("NSTL_GEMM4_F8", raising=False)
    bf16_table = kw.pop("bf16_table", False)
    masks = [None, None]
    if kw.pop("with_mask", False):
        masks = [mask_of(M, N), mask_of(M, N)]
    o4 = run8("gemm4f8 " + what, M, N, Kd, g4_counts(M, N, epilogue), pads=(16, 16), ldc=N + 8, epilogue=epilogue,
              relu_mask=masks[0], bf16_table=bf16_table, **kw)
    monkeypatch.setenv("NSTL_GEMM4_F8", "0")
    o8 = run8("ring8 " + what, M, N, Kd, ring_counts(epilogue), pads=(16, 16), ldc=N + 8, epilogue=epilogue,
              relu_mask=masks[1], **kw)
    monkeypatch.delenv("NSTL_GEMM4_F8", raising=False)
    err = (o4.window().double() - o8.window().double()).abs()
    ratio = (err / (o4.bound + o8.bound).clamp_min(1e-300)).max().item()
    _ERRORS["pair " + what + " (sum of the two bounds)"] = ratio
    assert ratio <= 1.0, (what, ratio)
    if masks[0] is not None:
        assert torch.equal(masks[0], masks[1]), what + ": the two kernels' keep words differ"
    return o4, o8, masks


@pytest.mark.parametrize("M,N,Kd", G4_SHAPES)
def test_gemm4f8_plain_and_bias(M, N, Kd, monkeypatch):
    both("%dx%dx%d" % (M, N, Kd), M, N, Kd, monkeypatch)
    both("%dx%dx%d bias" % (M, N, Kd), M, N, Kd, monkeypatch, epilogue=G.EPI_BIAS, bias=bias_of(N, "rand"))


@pytest.mark.parametrize("M,N,Kd", G4_SHAPES)
def test_gemm4f8_relu_dropout_then_drelu_colsum(M, N, Kd, monkeypatch):
    """p = 0.3 without and with relu_mask (identical h, identical keep words on both
    kernels, keep_flat with a +50 bias), then dReLU from those bits with column sums."""
    for kind in ("pos", "rand"):
        kw = dict(epilogue=G.EPI_BIAS_RELU_DROP, bias=bias_of(N, kind), p_drop=P, seed=SEED)
        what = "%dx%dx%d relu-drop bias %s" % (M, N, Kd, kind)
        h4, h8, _ = both(what, M, N, Kd, monkeypatch, **kw)
        m4, m8, masks = both(what + " +mask", M, N, Kd, monkeypatch, with_mask=True, **kw)
        assert torch.equal(h4.window(), m4.window()) and torch.equal(h8.window(), m8.window())
        if kind == "pos":
            check_keep_pattern(h4, what)
            check_keep_pattern(h8, what)
    aux = nans(M, N + 8, dtype=BF16)
    aux[:, :N] = m4.window()
    rows = (M + 127) // 128
    for name, env, counts, n_round, mask in (("gemm4f8", None, g4_counts(M, N), 12, masks[0]),
                                             ("ring8", "0", ring_counts(), 19, masks[1])):
        if env is None:
            monkeypatch.delenv("NSTL_GEMM4_F8", raising=False)
        else:
            monkeypatch.setenv("NSTL_GEMM4_F8", env)
        part = nans(rows + 1, N)
        d = run8("%s %dx%dx%d drelu from mask + colsum" % (name, M, N, Kd), M, N, Kd, counts, pads=(16, 16), ldc=N + 8,
                 epilogue=G.EPI_DRELU_DROP, aux=aux, ld_aux=N + 8, p_drop=P, relu_mask=mask, colsum_part=part, in_seed=11)
        check_colsum_rows(part, rows, d, n_round, "%s %dx%dx%d drelu colsum" % (name, M, N, Kd))
    monkeypatch.delenv("NSTL_GEMM4_F8", raising=False)


@pytest.mark.parametrize("T,dim,rc,bf16_table", [(128, 64, 128, False), (256, 64, 192, True)],
                         ids=["f32-table-T128", "bf16-table-T256"])
def test_gemm4f8_rope(T, dim, rc, bf16_table, monkeypatch):
    """T = 128: the f32 table fits the LDS; T = 256 (C5's long clip): held as bf16."""
    M, N, Kd = 512, 256, 768
    cs, sn = rotation_tables(T, dim, DEV)
    both("%dx%dx%d rope T%d dim%d cols%d" % (M, N, Kd, T, dim, rc), M, N, Kd, monkeypatch, epilogue=G.EPI_BIAS_ROPE,
         bias=bias_of(N, "rand"), rope=(cs, sn, T, dim), rope_cols=rc, bf16_table=bf16_table)


def test_gemm4f8_partial_second_round():
    """16 more tiles than the stream has CUs at K = 512: a second, partial round of the
    persistent loop."""
    cus = K.stream_cus()
    M, N, Kd = 256 * (cus // 16 + 1), 4096, 512
    assert (M // 256) * (N // 256) == cus + 16
    run8("gemm4f8 partial second round %dx%dx%d bias" % (M, N, Kd), M, N, Kd, g4_counts(M, N), pads=(16, 16), ldc=N + 8,
         epilogue=G.EPI_BIAS, bias=bias_of(N, "rand"))
