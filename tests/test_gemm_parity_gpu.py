"""Per-element f64 parity of the GEMM kernels (csrc/gemm.hip, csrc/gemm4.h) on the
MI355X against tests/gemm_ref.py (itself proven in tests/test_gemm_ref.py): the
128x128 kernel, the 8-wave 256x256 ring kernel, the 4-wave persistent gemm4 kernel,
split-K with splitk_reduce and the grouped launches, at the tile, K and stride edges
where each changes path.  fp8 operands: tests/test_fp8_parity_gpu.py, by the same reference.

Every case
  - gives C as an [M + 2][ldc] NaN-filled buffer (the live M x N window set to C0
    when beta != 0): after the call every element outside the window is still NaN,
    and every element inside it is within gemm_ref.bound of the f64 reference:
    E32 mag for f32 C, 2^-8 |ref| + (1 + 2^-8) E32 mag for bf16 C, with E32 = 1e-5
    and mag the magnitude the f32 arithmetic rounds against (see gemm_ref.gemm_ref).
    No element is excluded; a dropped element must be an exact zero;
  - pads every operand row past its extent: zeros where the reduction extent is not
    a multiple of the 16-byte chunk (include/nstl.h requires them), NaN everywhere
    else (lda > K, the rows of an MN-major operand, ld_aux > N), so a read of the
    padding shows;
  - asserts through the launch counters which kernel ran.
No bound is tuned against a kernel.  With NSTL_GEMM_PARITY_ERRORS_OUT=<file> the
worst err / bound of every case is written (profiles/gemm_parity_errors.txt is such
a run)."""
import os

import pytest
import torch

from tests import gemm_ref as G

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from neurosync_trainer_lite_amd import _hip as K
    from neurosync_trainer_lite_amd.engine import rotation_tables

DEV = "cuda:0"
NAN = float("nan")
F32, BF16 = torch.float32, torch.bfloat16
TT, TN, NN, NT = (True, True), (True, False), (False, False), (False, True)  # (a_kmajor, b_kmajor)
LAYOUTS = [pytest.param(TT, id="TT"), pytest.param(TN, id="TN"), pytest.param(NN, id="NN"), pytest.param(NT, id="NT")]
DTYPES = [pytest.param(F32, id="f32"), pytest.param(BF16, id="bf16")]
SEED = (0x9E3779B9 << 32) | 0x01234567  # nonzero high word
P = 0.3
COUNTERS = ("gemm128", "gemm_ring", "gemm4", "gemm4_tiles", "gemm_splitk_reduce")

_ERRORS = {}  # case -> worst err / bound


@pytest.fixture(scope="module", autouse=True)
def _error_report():
    yield
    path = os.environ.get("NSTL_GEMM_PARITY_ERRORS_OUT")
    if path and _ERRORS:
        with open(path, "w") as f:
            f.write("# tests/test_gemm_parity_gpu.py: worst |got - ref| / bound of every case (bound: f32 C 1e-5 mag;\n")
            f.write("# bf16 C 2^-8 |ref| + (1 + 2^-8) 1e-5 mag; tests/gemm_ref.py).  No case is widened.\n")
            f.write("# %-86s %s\n" % ("case", "err / bound"))
            for what in sorted(_ERRORS):
                f.write("%-88s %.4f\n" % (what, _ERRORS[what]))


def dname(dt):
    return "f32" if dt == F32 else "bf16"


def lname(lay):
    return {TT: "TT", TN: "TN", NN: "NN", NT: "NT"}[lay]


def rnd(*shape, dtype=BF16, scale=1.0, seed=0):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return (torch.randn(*shape, generator=g, device=DEV, dtype=torch.float32) * scale).to(dtype)


def nans(*shape, dtype=F32):
    return torch.full(shape, NAN, dtype=dtype, device=DEV)


def ceil_to(x, m):
    return (x + m - 1) // m * m


def operand(rows, red, kmajor, dtype, seed, scale=1.0, extra=1):
    """A stored GEMM operand with `extra` 16-byte chunks of padding per row: [rows][ld]
    when K-major, [red][ld] otherwise.  Padding: zeros when K-major and the reduction
    extent is no multiple of the chunk (the 128 kernel reads whole chunks), NaN otherwise."""
    vec = 16 // (4 if dtype == F32 else 2)
    r, c = (rows, red) if kmajor else (red, rows)
    ld = ceil_to(c, vec) + extra * vec
    X = nans(r, ld, dtype=dtype)
    X[:, :c] = rnd(r, c, dtype=dtype, scale=scale, seed=seed)
    if kmajor and c % vec:
        X[:, c:] = 0
    return X


class Out:
    """C as an [M + 2][ldc] window of a NaN-filled buffer that starts c_off elements
    into its allocation (c_off > 0: a C pointer off the 16-byte alignment)."""

    def __init__(self, M, N, ldc, c_dtype, c_off=0, C0=None):
        self.M, self.N, self.ldc = M, N, ldc
        self.buf = nans(c_off + (M + 2) * ldc + 16, dtype=c_dtype)
        self.C = self.buf[c_off:c_off + (M + 2) * ldc].view(M + 2, ldc)
        self.live = torch.zeros_like(self.buf, dtype=torch.bool)
        self.live[c_off:c_off + (M + 2) * ldc].view(M + 2, ldc)[:M, :N] = True
        if C0 is not None:
            self.C[:M, :N] = C0

    def window(self):
        return self.C[:self.M, :self.N]

    def check_canaries(self, what):
        assert torch.isnan(self.buf[~self.live].float()).all(), what + ": wrote outside the M x N window of C"


def judge(got, ref, mag, c_dtype, what):
    """|got - ref| <= bound per element (a NaN in got fails); returns the worst ratio."""
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert (mag >= ref.abs()).all(), what
    err = (got.double() - ref).abs()
    bnd = G.bound(ref, mag, c_dtype)
    ratio = (err / bnd.clamp_min(1e-300)).max().item()
    print("%s: worst err / bound %.4f (max |err| %.3e, max |ref| %.3e)" % (what, ratio, err.max().item(),
                                                                         ref.abs().max().item()))
    _ERRORS[what] = max(ratio, _ERRORS.get(what, 0.0)) if ratio == ratio else ratio
    assert not torch.isnan(got.float()).any(), what + ": NaN in (or no write to) the window of C"
    assert ratio <= 1.0, "%s: worst element at %.4f of its bound" % (what, ratio)
    return ratio


def check_counts(expect, what):
    c = K.kernel_counts()
    for name in COUNTERS:
        assert c[name] == expect.get(name, 0), "%s: %s launches %d, expected %d (%s)" % (
            what, name, c[name], expect.get(name, 0), {n: c[n] for n in COUNTERS})


def run(what, M, N, Kd, expect, *, dtype=BF16, c_dtype=BF16, lay=TT, ldc=None, c_off=0, alpha=1.0, beta=0.0,
        epilogue=0, bias=None, p_drop=0.0, seed=0, rope=None, rope_cols=0, aux=None, ld_aux=0, split_k=1,
        relu_mask=None, colsum_part=None, b_scale=0.1, in_seed=1):
    """One nstl_gemm call judged by the reference.  Returns the Out (stored C)."""
    akm, bkm = lay
    A = operand(M, Kd, akm, dtype, in_seed)
    B = operand(N, Kd, bkm, dtype, in_seed + 1, scale=b_scale)
    ldc = N if ldc is None else ldc
    C0 = rnd(M, N, dtype=c_dtype, seed=in_seed + 2) if beta != 0.0 else None
    out = Out(M, N, ldc, c_dtype, c_off, C0)
    kw = dict(a_kmajor=akm, b_kmajor=bkm, lda=A.stride(0), ldb=B.stride(0), ldc=ldc, alpha=alpha, beta=beta,
              epilogue=epilogue, bias=bias, p_drop=p_drop, seed=seed, rope=rope, rope_cols=rope_cols, aux=aux,
              ld_aux=ld_aux, split_k=split_k, relu_mask=relu_mask, colsum_part=colsum_part)
    if split_k > 1:
        kw["workspace"] = nans(split_k * M * N)
    K.kernel_counts_reset()
    K.gemm(A, B, out.C, M, N, Kd, **kw)
    torch.cuda.synchronize()
    check_counts(expect, what)
    ref, mag = G.gemm_ref(A, B, M, N, Kd, a_kmajor=akm, b_kmajor=bkm, alpha=alpha, beta=beta, C0=C0,
                          epilogue=epilogue, bias=bias, aux=aux, p_drop=p_drop, seed=seed, rope=rope,
                          rope_cols=rope_cols)
    out.check_canaries(what)
    judge(out.window(), ref, mag, c_dtype, what)
    out.ref = ref
    return out


def bias_of(N, kind, seed=9):
    """'rand': ordinary biases; 'pos': all +50, so every pre-activation is positive and
    the zero pattern of a ReLU-dropout output is the keep pattern itself."""
    return torch.full((N,), 50.0, device=DEV) if kind == "pos" else rnd(N, dtype=F32, seed=seed)


def check_keep_pattern(out, seed, what):
    keep = torch.from_numpy(G.keep_flat(seed, out.M, out.N, P)).to(DEV)
    assert torch.equal(out.window() != 0, keep), what + ": the zero pattern is not keep_flat(seed, M, N, p)"


def aux_of(M, N, ld_aux, dtype, seed=7):
    """A saved post-dropout activation [M][ld_aux]: relu of a random matrix (about half
    zeros), NaN in the padding columns."""
    h = nans(M, ld_aux, dtype=dtype)
    h[:, :N] = torch.relu(rnd(M, N, dtype=dtype, seed=seed))
    return h


# ---------------------------------------------------------------------------
# the 128 x 128 kernel: f32 operands, and bf16 below 32 big tiles
# ---------------------------------------------------------------------------
S128 = [(130, 70, 136), (17, 61, 40), (129, 132, 36), (17, 61, 43)]
ONE128 = {"gemm128": 1}


def shapes128(dtype):
    # (129, 132, 36): f32 only (issue); (17, 61, 43): K inside a 16-byte chunk, zero padding
    return [s for s in S128 if dtype == F32 or s != (129, 132, 36)]


@pytest.mark.parametrize("ldc_pad", [3, 8])
@pytest.mark.parametrize("c_dtype", DTYPES)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("lay", LAYOUTS)
def test_gemm128_layouts_ragged(lay, dtype, c_dtype, ldc_pad):
    """Partial tiles in both directions, K tails inside a chunk and inside a BK step,
    every layout, odd ldc (scalar stores) and ldc % 4 == 0 (vector stores)."""
    for M, N, Kd in shapes128(dtype):
        run("128 %s %s->%s %dx%dx%d ldc N+%d" % (lname(lay), dname(dtype), dname(c_dtype), M, N, Kd, ldc_pad),
            M, N, Kd, ONE128, dtype=dtype, c_dtype=c_dtype, lay=lay, ldc=N + ldc_pad, b_scale=1.0)


@pytest.mark.parametrize("ldc_pad,c_off", [(8, 1), (3, 0), (8, 0)])
@pytest.mark.parametrize("c_dtype", DTYPES)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("lay", [pytest.param(TT, id="TT"), pytest.param(NN, id="NN")])
def test_gemm128_alpha_bias_beta_and_unaligned_c(lay, dtype, c_dtype, ldc_pad, c_off):
    """alpha acc, then the bias, then beta C0 (alpha 0.5, beta 0.75), with C one element
    off its allocation (not 16-byte aligned: scalar stores at a vector-friendly ldc)."""
    M, N, Kd = 130, 70, 136
    run("128 %s %s->%s alpha .5 bias beta .75 ldc N+%d off %d" % (lname(lay), dname(dtype), dname(c_dtype), ldc_pad, c_off),
        M, N, Kd, ONE128, dtype=dtype, c_dtype=c_dtype, lay=lay, ldc=N + ldc_pad, c_off=c_off, alpha=0.5, beta=0.75,
        epilogue=K.EPI_BIAS, bias=bias_of(N, "rand"))


@pytest.mark.parametrize("c_dtype", DTYPES)
@pytest.mark.parametrize("dtype", DTYPES)
def test_gemm128_rope_ragged(dtype, c_dtype):
    """bias + RoPE on partial tiles: positions wrap inside a tile (rope_T 25), a head
    dim that is no power of two (24), unrotated columns past rope_cols."""
    M, N, Kd, T, dim, rc = 100, 72, 136, 25, 24, 48
    cs, sn = rotation_tables(T, dim, DEV)
    run("128 rope %s->%s 100x72 T25 dim24 cols48" % (dname(dtype), dname(c_dtype)), M, N, Kd, ONE128, dtype=dtype,
        c_dtype=c_dtype, ldc=N + 4, alpha=0.5, epilogue=K.EPI_BIAS_ROPE, bias=bias_of(N, "rand"), rope=(cs, sn, T, dim),
        rope_cols=rc)


@pytest.mark.parametrize("bias_kind", ["pos", "rand"])
@pytest.mark.parametrize("N", [72, 61])
@pytest.mark.parametrize("dtype", DTYPES)
def test_gemm128_relu_dropout_ragged(dtype, N, bias_kind):
    """bias + ReLU + dropout on partial tiles; odd N hashes single elements of the flat
    index i*N + j (the odd branch of epi_math4) and ldc != N must not enter the index."""
    M, Kd = 100, 136
    what = "128 relu-drop %s N %d bias %s" % (dname(dtype), N, bias_kind)
    out = run(what, M, N, Kd, ONE128, dtype=dtype, c_dtype=dtype, ldc=N + 3, epilogue=K.EPI_BIAS_RELU_DROP,
              bias=bias_of(N, bias_kind), p_drop=P, seed=SEED)
    if bias_kind == "pos":
        check_keep_pattern(out, SEED, what)


@pytest.mark.parametrize("aux_pad", [4, 5])
@pytest.mark.parametrize("N", [72, 61])
@pytest.mark.parametrize("dtype", DTYPES)
def test_gemm128_drelu_ragged(dtype, N, aux_pad):
    """dReLU + dropout from a saved activation in the operands' dtype, ld_aux > N
    (N + 4: the 4-wide aux read when it is aligned; N + 5: the scalar one)."""
    M, Kd = 100, 136
    aux = aux_of(M, N, N + aux_pad, dtype)
    run("128 drelu %s N %d ld_aux N+%d" % (dname(dtype), N, aux_pad), M, N, Kd, ONE128, dtype=dtype, c_dtype=dtype,
        lay=TN, ldc=N + 3, alpha=0.5, epilogue=K.EPI_DRELU_DROP, aux=aux, ld_aux=N + aux_pad, p_drop=P)


@pytest.mark.parametrize("split", [3, 8])
@pytest.mark.parametrize("c_dtype", DTYPES)
@pytest.mark.parametrize("dtype", DTYPES)
def test_gemm128_splitk_bias_beta_strided(dtype, c_dtype, split):
    """split-K partials + splitk_reduce with bias, beta and ldc > N together, odd N."""
    M, N, Kd = 130, 61, 1000
    for lay in (TT, NN):
        run("128 split-K %d %s %s->%s bias beta .5 ldc N+3" % (split, lname(lay), dname(dtype), dname(c_dtype)), M, N, Kd,
            {"gemm128": 1, "gemm_splitk_reduce": 1}, dtype=dtype, c_dtype=c_dtype, lay=lay, ldc=N + 3, beta=0.5,
            epilogue=K.EPI_BIAS, bias=bias_of(N, "rand"), split_k=split)


# ---------------------------------------------------------------------------
# the 8-wave ring kernel: bf16, >= 32 tiles of 256 x 256, kept off gemm4 by shape
# ---------------------------------------------------------------------------
RM, RN = 1800, 1000  # 8 x 4 tiles; the last row tile has 8 rows, the last column tile 232 columns
ONE_RING = {"gemm_ring": 1}


@pytest.mark.parametrize("c_dtype", DTYPES)
@pytest.mark.parametrize("lay", [pytest.param(TT, id="TT"), pytest.param(TN, id="TN")])
@pytest.mark.parametrize("Kd", [64, 128, 192, 320])
def test_ring_short_k(Kd, lay, c_dtype):
    """2, 4, 6 and 10 K-steps through the five-stage ring (three stages of prefetch):
    the prologue and the drain with fewer steps than stages."""
    run("ring %s K %d ->%s 1800x1000 ldc N+8" % (lname(lay), Kd, dname(c_dtype)), RM, RN, Kd, ONE_RING, c_dtype=c_dtype,
        lay=lay, ldc=RN + 8)


@pytest.mark.parametrize("c_dtype", DTYPES)
@pytest.mark.parametrize("lay", [pytest.param(NN, id="NN"), pytest.param(NT, id="NT")])
def test_ring_mn_major_a(lay, c_dtype):
    """The layouts with an MN-major A; a_kmajor=False with b_kmajor=True is launched nowhere else."""
    run("ring %s K 192 ->%s 1800x1000 ldc N+8" % (lname(lay), dname(c_dtype)), RM, RN, 192, ONE_RING, c_dtype=c_dtype,
        lay=lay, ldc=RN + 8)


@pytest.mark.parametrize("bias_kind", ["pos", "rand"])
def test_ring_generic_odd_n_relu_dropout(bias_kind):
    """EM_GENERIC: odd N with ReLU-dropout (ldc = N + 1): single-element hashes."""
    what = "ring generic relu-drop N 999 bias %s" % bias_kind
    out = run(what, RM, 999, 192, ONE_RING, ldc=1000, epilogue=K.EPI_BIAS_RELU_DROP, bias=bias_of(999, bias_kind),
              p_drop=P, seed=SEED)
    if bias_kind == "pos":
        check_keep_pattern(out, SEED, what)


def test_ring_generic_bf16_beta1():
    """EM_GENERIC: bf16 out accumulating into the prior C (beta 1) with a bias."""
    run("ring generic bf16 bias beta 1", RM, RN, 192, ONE_RING, ldc=RN + 8, alpha=0.5, beta=1.0, epilogue=K.EPI_BIAS,
        bias=bias_of(RN, "rand"))


def test_ring_generic_f32_rope():
    """EM_GENERIC: f32 out with the bias + RoPE epilogue."""
    T, dim = 100, 64
    cs, sn = rotation_tables(T, dim, DEV)
    run("ring generic f32 rope", RM, RN, 192, ONE_RING, c_dtype=F32, ldc=RN + 8, alpha=0.5, epilogue=K.EPI_BIAS_ROPE,
        bias=bias_of(RN, "rand"), rope=(cs, sn, T, dim), rope_cols=512)


def test_ring_bias_fused():
    """EM_BF16 with a bias and alpha 0.5: the register-direct epilogue on the full
    tiles, the LDS-staged one on the ragged last row and column tiles."""
    run("ring bias alpha .5 1800x1000 ldc N+8", RM, RN, 192, ONE_RING, ldc=RN + 8, alpha=0.5, epilogue=K.EPI_BIAS,
        bias=bias_of(RN, "rand"))


def test_ring_rope_fused():
    """EM_ROPE at ragged tiles: rope_T 100 (positions wrap inside a 64-row pass),
    rope_cols 512 of 1000, alpha 0.5, ldc N + 8."""
    T, dim = 100, 64
    cs, sn = rotation_tables(T, dim, DEV)
    run("ring rope T100 dim64 cols512", RM, RN, 192, ONE_RING, ldc=RN + 8, alpha=0.5, epilogue=K.EPI_BIAS_ROPE,
        bias=bias_of(RN, "rand"), rope=(cs, sn, T, dim), rope_cols=512)


def ring_relu_kw(bias_kind):
    return dict(ldc=RN + 8, alpha=0.5, epilogue=K.EPI_BIAS_RELU_DROP, bias=bias_of(RN, bias_kind), p_drop=P, seed=SEED)


def mask_words(M, N, Kd, **kw):
    X, W = operand(M, Kd, True, BF16, 1), operand(N, Kd, True, BF16, 2)
    C = torch.empty(M, N + 8, dtype=BF16, device=DEV)
    kw = {k: v for k, v in kw.items() if k != "ldc"}
    return K.gemm_relu_mask_words(X, W, C, M, N, Kd, lda=X.stride(0), ldb=W.stride(0), ldc=N + 8, **kw)


@pytest.mark.parametrize("bias_kind", ["pos", "rand"])
def test_ring_relu_dropout_fused_with_and_without_mask(bias_kind):
    """EM_RELU_DROP at ragged tiles, ldc != N (the hash index is i*N + j, not i*ldc + j):
    the values, the zero pattern against keep_flat, and h the same with a relu_mask."""
    what = "ring relu-drop bias %s" % bias_kind
    kw = ring_relu_kw(bias_kind)
    h = run(what, RM, RN, 192, ONE_RING, **kw)
    words = mask_words(RM, RN, 192, **kw)
    assert words == ((RM + 63) // 64) * 8 * ((RN + 7) // 8)
    mask = torch.zeros(words, dtype=torch.int64, device=DEV)
    hm = run(what + " +mask", RM, RN, 192, ONE_RING, relu_mask=mask, **kw)
    assert torch.equal(h.window(), hm.window())
    if bias_kind == "pos":
        check_keep_pattern(h, SEED, what)


def test_ring_drelu_aux_mask_colsum():
    """EM_DRELU at ragged tiles: from the saved activation (ld_aux = N + 8, NaN padding),
    and from the forward's keep&positive bits, which must give the same output; the
    per-128-row column sums (NaN-prefilled) reduce to the column sums of the stored dh."""
    M, N, Kd = RM, RN, 192
    fkw = ring_relu_kw("rand")
    words = mask_words(M, N, Kd, **fkw)
    mask = torch.zeros(words, dtype=torch.int64, device=DEV)
    h = run("ring drelu: forward h", M, N, Kd, ONE_RING, relu_mask=mask, **fkw)
    aux = nans(M, N + 8, dtype=BF16)
    aux[:, :N] = h.window()
    bkw = dict(lay=TN, ldc=N + 8, alpha=0.5, epilogue=K.EPI_DRELU_DROP, aux=aux, ld_aux=N + 8, p_drop=P, in_seed=11)
    d_aux = run("ring drelu from aux ld_aux N+8", M, N, Kd, ONE_RING, **bkw)
    dY, W2 = operand(M, Kd, True, BF16, 11), operand(N, Kd, False, BF16, 12)
    rows = K.gemm_colsum_rows(dY, W2, d_aux.C, M, N, Kd, a_kmajor=True, b_kmajor=False, lda=dY.stride(0),
                              ldb=W2.stride(0), ldc=N + 8, epilogue=K.EPI_DRELU_DROP, aux=aux, ld_aux=N + 8, p_drop=P)
    assert rows == (M + 127) // 128
    # M % 256 = 8: the last row tile's lower waves (rows 1920 ..) hold no row of C and
    # must write no partial row (row 15 of 15: past the end of colsum_part)
    part = nans(rows + 1, N)
    d_mask = run("ring drelu from mask + colsum", M, N, Kd, ONE_RING, relu_mask=mask, colsum_part=part, **bkw)
    assert torch.equal(d_aux.window(), d_mask.window())
    check_colsum(part, rows, d_mask, "ring drelu colsum")


def check_colsum(part, rows, out, what):
    """colsum_part ([rows + 1][N], NaN-prefilled: rows partial rows and a canary row),
    reduced by nstl_reduce_rows, against the f64 column sums of the stored output,
    within 1e-5 sum_i |stored| per column."""
    assert torch.isnan(part[rows:]).all(), what + ": wrote past its nstl_gemm_colsum_rows rows"
    assert not torch.isnan(part[:rows]).any(), what + ": a partial row was not written"
    total = nans(out.N)
    K.reduce_rows(part, rows, out.N, total, 0.0)
    torch.cuda.synchronize()
    st = out.window().double()
    ratio = ((total.double() - st.sum(0)).abs() / (1e-5 * st.abs().sum(0)).clamp_min(1e-300)).max().item()
    print("%s: worst column at %.4f of 1e-5 sum|stored|" % (what, ratio))
    _ERRORS[what + " (1e-5 sum|stored| per column)"] = ratio
    assert ratio <= 1.0, (what, ratio)


@pytest.mark.parametrize("c_dtype", DTYPES)
def test_ring_splitk_chunk64_beta1(c_dtype):
    """A weight gradient (NN) split 4 ways: K-chunks of 64 = two K-steps per ring pass,
    partials through the workspace, splitk_reduce with beta 1."""
    run("ring split-K 4 NN 2048x1024x256 ->%s beta 1" % dname(c_dtype), 2048, 1024, 256,
        {"gemm_ring": 1, "gemm_splitk_reduce": 1}, c_dtype=c_dtype, lay=NN, ldc=1024 + 8, beta=1.0, split_k=4)


@pytest.mark.parametrize("ldc_pad,c_off", [(8, 4), (4, 0)])
def test_ring_full_tiles_staged_bf16_epilogue(ldc_pad, c_off):
    """Full tiles that gemm4 and the direct bf16 epilogue refuse: C 8 bytes off the
    16-byte alignment, or ldc % 8 != 0: the LDS-staged epilogue with scalar stores."""
    run("ring full tiles bias ldc N+%d off %d" % (ldc_pad, c_off), 2048, 1024, 256, ONE_RING, ldc=1024 + ldc_pad,
        c_off=c_off, alpha=0.5, epilogue=K.EPI_BIAS, bias=bias_of(1024, "rand"))


# ---------------------------------------------------------------------------
# gemm4: the 4-wave persistent kernel (full 256 x 256 tiles, K % 128 == 0, K >= 256)
# ---------------------------------------------------------------------------
def g4(M, N):
    return {"gemm4": 1, "gemm4_tiles": (M // 256) * (N // 256)}


@pytest.mark.parametrize("M,N,Kd", [(256, 256, 256), (512, 256, 384), (512, 512, 2048)])
@pytest.mark.parametrize("lay,c_dtype", [pytest.param(TT, BF16, id="TT-bf16"), pytest.param(TN, BF16, id="TN-bf16"),
                                         pytest.param(TT, F32, id="TT-f32"), pytest.param(TN, F32, id="TN-f32"),
                                         pytest.param(NN, F32, id="NN-f32")])
def test_gemm4_small_and_r3(M, N, Kd, lay, c_dtype):
    """Its smallest legal problem (one tile, K 256), K 384 (three stage pairs) and
    K 2048 (the R3 variant), strided C, lda = K + 8 with NaN padding."""
    ldc = N + (8 if c_dtype == BF16 else 4)
    run("gemm4 %s ->%s %dx%dx%d ldc %d" % (lname(lay), dname(c_dtype), M, N, Kd, ldc), M, N, Kd, g4(M, N),
        c_dtype=c_dtype, lay=lay, ldc=ldc, alpha=0.5, b_scale=0.05)


def test_gemm4_partial_second_round():
    """One more row of tiles than the stream has CUs: a second, partial round of the
    persistent loop, with a strided C."""
    cus = K.stream_cus()
    M, N, Kd = 256 * (cus // 16 + 1), 4096, 256
    assert (M // 256) * (N // 256) == cus + 16
    run("gemm4 partial second round %dx%dx%d ldc N+8" % (M, N, Kd), M, N, Kd, g4(M, N), ldc=N + 8, epilogue=K.EPI_BIAS,
        bias=bias_of(N, "rand"))


@pytest.mark.parametrize("lay", [pytest.param(TT, id="TT"), pytest.param(TN, id="TN")])
def test_gemm4_bias_alpha(lay):
    run("gemm4 %s bias alpha .5 ldc N+8" % lname(lay), 512, 768, 256, g4(512, 768), lay=lay, ldc=768 + 8, alpha=0.5,
        epilogue=K.EPI_BIAS, bias=bias_of(768, "rand"))


@pytest.mark.parametrize("T,dim,rc", [(100, 64, 512), (64, 32, 256)])
def test_gemm4_rope_alpha(T, dim, rc):
    """alpha acc + bias, then the rotation (tables staged in LDS), rope_cols < N."""
    M, N, Kd = 512, 768, 256
    cs, sn = rotation_tables(T, dim, DEV)
    run("gemm4 rope T%d dim%d cols%d alpha .5" % (T, dim, rc), M, N, Kd, g4(M, N), ldc=N + 8, alpha=0.5,
        epilogue=K.EPI_BIAS_ROPE, bias=bias_of(N, "rand"), rope=(cs, sn, T, dim), rope_cols=rc)


def test_gemm4_relu_dropout_mask_then_drelu_colsum():
    """ReLU-dropout + keep bits, then dReLU from those bits + column sums, each by
    the reference (the dReLU reference reads the stored h) and the canaries.  32 tiles:
    nstl_gemm_relu_mask_words answers 0 below that, whichever kernel would run."""
    M, N, Kd = 2048, 1024, 256
    for kind in ("pos", "rand"):
        fkw = dict(ldc=N + 8, alpha=0.5, epilogue=K.EPI_BIAS_RELU_DROP, bias=bias_of(N, kind), p_drop=P, seed=SEED)
        words = mask_words(M, N, Kd, **fkw)
        assert words == (M // 64) * 8 * (N // 8)
        mask = torch.zeros(words, dtype=torch.int64, device=DEV)
        h = run("gemm4 relu-drop +mask bias %s" % kind, M, N, Kd, g4(M, N), relu_mask=mask, **fkw)
        if kind == "pos":
            check_keep_pattern(h, SEED, "gemm4 relu-drop")
    aux = nans(M, N + 8, dtype=BF16)
    aux[:, :N] = h.window()
    part = nans((M + 127) // 128 + 1, N)
    d = run("gemm4 drelu from mask + colsum", M, N, Kd, g4(M, N), lay=TN, ldc=N + 8, alpha=0.5,
            epilogue=K.EPI_DRELU_DROP, aux=aux, ld_aux=N + 8, p_drop=P, relu_mask=mask, colsum_part=part, in_seed=11)
    check_colsum(part, (M + 127) // 128, d, "gemm4 drelu colsum")


# ---------------------------------------------------------------------------
# grouped launches
# ---------------------------------------------------------------------------
GROUP_DW = [(256, 512), (512, 256), (256, 256)]  # (n, k) of three weight gradients dW = dY^T X
# sums of <= 256 squares per lane in f32, then exact: (256 + 1) 2^-24 of a sum of positives
SQ_REL = 257 * 2.0 ** -24


@pytest.mark.parametrize("beta", [0.0, 1.0])
def test_grouped_weight_gradients_column_windows(beta):
    """Three weight gradients of different shapes in one launch, f32 out, each C a
    column window of one wider NaN-filled buffer (ldc > N); sq_part against the stored
    C.  beta 0: one gemm4 launch; beta 1: the ring fallback, one launch per problem."""
    Mt = 256
    width = sum(k + 4 for _, k in GROUP_DW)
    rows = max(n for n, _ in GROUP_DW) + 2
    buf = nans(rows, width)
    live = torch.zeros_like(buf, dtype=torch.bool)
    probs, refs, off = [], [], 0
    for i, (n, k) in enumerate(GROUP_DW):
        dY, X = operand(n, Mt, False, BF16, 20 + i), operand(k, Mt, False, BF16, 30 + i)
        C = buf[:, off:off + k]
        C0 = None
        if beta != 0.0:
            C0 = rnd(n, k, dtype=F32, seed=40 + i)
            C[:n] = C0
        live[:n, off:off + k] = True
        sq = nans((n // 256) * (k // 256) * 8)
        probs.append((dY, X, C, n, k, Mt, dict(a_kmajor=False, b_kmajor=False, lda=dY.stride(0), ldb=X.stride(0),
                                               ldc=width, beta=beta, sq_part=sq)))
        refs.append((G.gemm_ref(dY, X, n, k, Mt, a_kmajor=False, b_kmajor=False, beta=beta, C0=C0), C, n, k, sq))
        off += k + 4
    K.kernel_counts_reset()
    K.gemm_grouped(probs)
    torch.cuda.synchronize()
    tiles = sum((n // 256) * (k // 256) for n, k in GROUP_DW)
    check_counts({"gemm4": 1, "gemm4_tiles": tiles} if beta == 0.0 else {"gemm_ring": len(GROUP_DW)}, "grouped dW")
    assert torch.isnan(buf[~live]).all(), "grouped dW: wrote outside a problem's window"
    for i, ((ref, mag), C, n, k, sq) in enumerate(refs):
        what = "grouped dW beta %g problem %d (%dx%d)" % (beta, i, n, k)
        judge(C[:n], ref, mag, F32, what)
        tot = (C[:n].double() ** 2).sum().item()
        rs = abs(sq.double().sum().item() - tot) / tot
        print("%s: sq_part rel %.3e of the stored C's sum of squares (bound %.2e)" % (what, rs, SQ_REL))
        _ERRORS[what + " sq_part (257 2^-24 relative)"] = rs / SQ_REL
        assert rs <= SQ_REL, (what, rs)


def test_grouped_rope_adjacent_windows():
    """Two bias + RoPE problems writing adjacent column windows of one buffer, as the
    engine's dkv_all is written: one gemm4 launch."""
    M, N, Kd, T, dim, rc = 256, 256, 256, 64, 64, 128
    cs, sn = rotation_tables(T, dim, DEV)
    X = operand(M, Kd, True, BF16, 50)
    buf = nans(M + 2, 2 * N + 8, dtype=BF16)
    probs, refs = [], []
    for i in range(2):
        W, b = operand(N, Kd, True, BF16, 51 + i, scale=0.1), bias_of(N, "rand", seed=60 + i)
        kw = dict(lda=X.stride(0), ldb=W.stride(0), ldc=2 * N + 8, epilogue=K.EPI_BIAS_ROPE, bias=b,
                  rope=(cs, sn, T, dim), rope_cols=rc)
        probs.append((X, W, buf[:, i * N:(i + 1) * N], M, N, Kd, kw))
        refs.append(G.gemm_ref(X, W, M, N, Kd, epilogue=K.EPI_BIAS_ROPE, bias=b, rope=(cs, sn, T, dim), rope_cols=rc))
    K.kernel_counts_reset()
    K.gemm_grouped(probs)
    torch.cuda.synchronize()
    check_counts({"gemm4": 1, "gemm4_tiles": 2}, "grouped rope")
    assert torch.isnan(buf[M:].float()).all() and torch.isnan(buf[:, 2 * N:].float()).all(), "grouped rope: wrote past C"
    for i, (ref, mag) in enumerate(refs):
        judge(buf[:M, i * N:(i + 1) * N], ref, mag, BF16, "grouped rope problem %d" % i)
