"""TEST INFRA: float64 restatement of nstl_features (csrc/features.hip) and of each
of its stages at any sample rate, with per-element error bounds whose roundings are
counted from the kernel source.  numpy only, no GPU.  tests/test_features_ref.py
proves it (against oracle/data_ref.extract_features at 88.2 kHz, the
reference-generated fixtures, an f32 emulation of every stage, and wrong references
that must exceed the bounds); tests/test_features_parity_gpu.py judges the kernels
by it.  Never imported by the package.

Built from the pieces of oracle/data_ref.py that take n_fft / hop / sr.

Bounds, stage by stage (U = 2^-24, one f32 rounding):
  mel power, fused kernels   2e-6 max(frame, pair partner) + 2e-5 |ref|, the
                             project's form (frames 2j, 2j + 1 share one complex FFT),
                             or where it is smaller the per-band bound counted from
                             the FFT's roundings (mel_bound_fft): the project's form
                             is 2e-6 of the frame's peak band, more than a band 57 dB
                             under the peak holds, and the dB stage keeps 80 dB
  X = frames @ DFT basis     (E32 + 3U) (|frames| @ |basis|): gemm_ref's f32 bound at
                             K = kp, and one rounding each of window, product, basis
  power c^2 + s^2            2 (|c| dc + |s| ds) + dc^2 + ds^2 + 3U P
  mel power, GEMM path       W @ dP + (E32 + 2U) W @ (P + dP)  (K = nbp, all >= 0)
  clip max (key)             bits of the max of the GPU's own mel buffer
  dB                         interval image of [mel - d, mel + d] under
                             10 log10(max(1e-10, .)): at least (10 / ln 10) d / mel
                             above the power floor, and the distance the clamp can
                             move below it; + (2 ELOG + 1) U |dB| for log10f and the
                             multiplication; the -80 dB floor the same from the clip
                             max, + U |floor| for the subtraction.  A band that the
                             bounds cannot place on one side of the floor takes the
                             larger of the two
  MFCC                       |dct32| @ d_dB + 129 U |dct32| @ (|dB| + d_dB): 128 fmas
                             and the table's own rounding
  CMVN / deltas / pair mean  from the f32 MFCC rows given: see cmvn_ref
  autocorr lags              rtol 2e-6 / atol 2e-7 for L >= 266, 3e-6 absolute
                             below (tests/test_features_gpu.py says why)
"""
import numpy as np

from oracle import data_ref

U = 2.0 ** -24
E32 = 1e-5            # tests/gemm_ref.E32: f32-accumulated GEMM, relative to |A| @ |B|
N_MELS, N_MFCC, N_AC, SG_W, CMVN_CH = 128, 23, 187, 9, 32
FFT_MAX, SW_MAXN, SW_WAVES, MAX_FRAME = 4096, 1536, 4, 4096
AMIN = float(np.float32(1e-10))   # the kernel's 1e-10f
TOP_DB = 80.0
# log10f on gfx950 against float64, in units of 2^-23 max(|log10 x|, 1): measured by
# tools/log10f_probe.py (profiles/features_parity_errors.txt), times 2.
ELOG_MEASURED = 1.7436
ELOG = 2.0 * ELOG_MEASURED


# sr -> (n_fft, mel path, F of the parity case): F odd at some rates (the last pair
# has one frame), even at others.  The paths are checked by hand: int(0.01667 sr) and
# its factors (tests/test_features_ref.py holds path() to this table).
RATES = {
    12000: (200, "wave", 13),     # 4 2 5 5; nb = 101 < 128 filters: empty ones
    16000: (266, "gemm", 24),     # 2 7 19; kp 268, nbp 192
    22050: (367, "gemm", 15),     # prime, odd; kp 368
    44100: (735, "wave", 21),     # 3 5 7 7, odd; hop 367
    48000: (800, "wave", 16),     # 4 4 2 5 5
    88200: (1470, "wave", 40),    # 2 3 5 7 7, the production rate
    120000: (2000, "wg", 17),     # 4 4 5 5 5: past SW_MAXN
    192000: (3200, "gemm", 12),   # 4 4 4 2 5 5, but 97.7 KB of tables > 64 KB
}


def clip(sr, F, seed, extra=17):
    """A seeded synth_audio clip of (F - 1) hop + extra samples: F STFT frames."""
    from tests.golden.make_goldens_helpers import synth_audio
    hop = frame_params(sr)[1]
    n = (F - 1) * hop + extra
    return synth_audio((n + 8) / sr, seed, sr)[:n].copy()


def cmvn_case(C, F, seed=5):
    """MFCC-like f32 rows [C][F]: row 1 constant, row 2 one large value repeated with a
    single outlier (when there are that many rows)."""
    rng = np.random.default_rng(seed + 1000 * C + F)
    x = (rng.standard_normal((C, F)) * rng.uniform(1, 30, (C, 1)) + rng.uniform(-600, 50, (C, 1))).astype(np.float32)
    if C > 2:
        x[1] = np.float32(-1131.3708)
        x[2] = np.float32(10000.0)
        x[2, F // 2] = np.float32(10001.0)
    return x


# ---------------------------------------------------------------------------
# sizes, plan, path, workspace
# ---------------------------------------------------------------------------
def frame_params(sr):
    n_fft = int(0.01667 * sr)
    return n_fft, n_fft // 2


def fft_radices(n):
    """n over {4, 2, 3, 5, 7}, fours first; [] when another prime factor remains."""
    f = []
    for r in (4, 2, 3, 5, 7):
        while n % r == 0 and len(f) < 16:
            f.append(r)
            n //= r
    return f if n == 1 else []


def mel_bands(sr, n_fft):
    """(first bin, bin count) of each filter's non-zero span, and the total (nnz)."""
    w = data_ref.mel_basis(sr, n_fft)
    bands = []
    for row in w:
        nz = np.nonzero(row)[0]
        bands.append((0, 0) if nz.size == 0 else (int(nz[0]), int(nz[-1] - nz[0] + 1)))
    return bands, sum(c for _, c in bands)


def fused_lds(n_fft, nnz):
    """stft_mel_kernel's dynamic LDS, the 64 KB rule of get_tables."""
    return 3 * n_fft * 8 + n_fft * 4 + 3 * N_MELS * 4 + nnz * 4


def wave_lds(n_fft, nnz):
    tables = (n_fft * 8 + n_fft * 4 + 3 * N_MELS * 4 + nnz * 4 + 15) // 16 * 16
    return tables + SW_WAVES * n_fft * 8


def path(sr, n_samples=0):
    """'gemm' (frames -> DFT GEMM -> power -> mel GEMM), 'wave' (wave-per-pair FFT)
    or 'wg' (workgroup-per-8-frames FFT), as get_tables and launch_stft_mel choose."""
    n_fft, _ = frame_params(sr)
    nf = len(fft_radices(n_fft)) if n_fft <= FFT_MAX else 0
    if nf > 0 and fused_lds(n_fft, mel_bands(sr, n_fft)[1]) > 65536:
        nf = 0
    if nf == 0:
        return "gemm"
    return "wave" if n_fft <= SW_MAXN and n_samples < 1 << 29 else "wg"


def autocorr_kernel(L, n_lags):
    """'mfma' (autocorr3_kernel) or 'valu' (autocorr2_kernel), as nstl_autocorr chooses."""
    steps = (L + 63) // 64
    xlen = max(64 * steps + 16 * 12, 16 * 48)
    return "mfma" if n_lags < 16 * 12 and 4 * xlen * 8 <= 65536 else "valu"


def n_frames(n_samples, n_fft, hop):
    """Centred frames of a clip (librosa's count; nstl_autocorr's as well): 1 + n / hop
    for an even n_fft, one fewer for an odd n_fft when n is a whole number of hops."""
    return (n_samples + 2 * (n_fft // 2) - n_fft) // hop + 1


def _a256(b):
    return (b + 255) // 256 * 256


def feat_layout(n_samples, sr):
    """Byte offsets of the workspace regions (feat_layout in features.hip)."""
    n_fft, hop = frame_params(sr)
    L = dict(n_fft=n_fft, hop=hop, nb=n_fft // 2 + 1, kp=(n_fft + 3) // 4 * 4)
    L["nbp"] = (L["nb"] + 63) // 64 * 64
    L["F"] = n_frames(n_samples, n_fft, hop)
    L["F60"] = (L["F"] + 1) // 2
    off = 0
    for name, size in (("frames", L["F"] * L["kp"] * 4), ("X", L["F"] * 2 * L["nb"] * 4),
                       ("db", L["F"] * N_MELS * 4), ("mfcc", L["F"] * N_MFCC * 4), ("ac", L["F"] * N_AC * 8),
                       ("key", 256), ("cmvn", N_MFCC * CMVN_CH * 2 * 8)):
        L[name] = off
        off += _a256(size)
    L["total"] = off
    return L


# ---------------------------------------------------------------------------
# STFT -> mel power
# ---------------------------------------------------------------------------
def hann_periodic(n):
    return 0.5 - 0.5 * np.cos(2 * np.pi * np.arange(n) / n)


def stft_frames(y, n_fft, hop, F=None):
    """[n_fft][F] f64: frame f starts at f hop - n_fft/2, zeros outside the clip."""
    F = n_frames(len(y), n_fft, hop) if F is None else F
    yp = np.concatenate([np.zeros(n_fft // 2), np.asarray(y, np.float64), np.zeros(n_fft)])
    idx = np.arange(n_fft)[:, None] + hop * np.arange(F)[None, :]
    return yp[idx]


def stft(y, sr, window=None, hop=None):
    """(X [F][nb] complex f64, frames [F][n_fft] f64 unwindowed, window)."""
    n_fft, h = frame_params(sr)
    win = hann_periodic(n_fft) if window is None else window
    fr = stft_frames(y, n_fft, h if hop is None else hop, n_frames(len(y), n_fft, h))
    return np.fft.rfft(fr * win[:, None], axis=0).T, fr.T, win


def mel_power(y, sr, **kw):
    """[F][128] f64 mel power."""
    n_fft, _ = frame_params(sr)
    X = stft(y, sr, **kw)[0]
    return (np.abs(X) ** 2) @ data_ref.mel_basis(sr, n_fft).astype(np.float64).T


def mel_bound_fused(ref):
    """The project's form (tests/test_features_gpu.py)."""
    F = ref.shape[0]
    fmax = ref.max(axis=1)
    pair = np.maximum(fmax, fmax[np.minimum(np.arange(F) ^ 1, F - 1)])
    return 2e-6 * pair[:, None] + 2e-5 * np.abs(ref)


def fft_roundings(n_fft):
    """Relative roundings (in U) a sample meets on its way through the FFT kernels: the
    f32 window and the product (2); per radix-R pass the f32 twiddle (1), the complex
    multiplication by it (2 sqrt 2, rounded up to 3), the f32 root of unity W (1) and a
    chain of 2 (R - 1) fmas per component against it (2 sqrt 2 (R - 1) on the modulus)."""
    return 2 + sum(5 + 2 * np.sqrt(2) * (r - 1) for r in fft_radices(n_fft))


def mel_bound_fft(y, sr):
    """Per-band worst-case bound of the fused kernels' mel power, counted from the
    source.  Every output bin is sum_n z_n w^{nk} with each term perturbed by at most
    fft_roundings() U, so |dZ_k| <= d = fft_roundings U sum_n |z_n| over the pair's
    complex frame z = x_2j + i x_2j+1 (|w| = 1); X0, X1 are half-sums of Z[k] and
    conj Z[n - k] (error d, the halving exact; the add is one more rounding, taken on
    |X| + d).  P = |X|^2 / 4-scaled: dP = 2 |X| d + d^2 + 4U P; the band is a chain of
    cnt fmas of non-negative terms: W @ dP + (cnt + 1) U mel.  Unlike the project's
    form this follows the band's own amplitude: a band 60 dB under the frame's peak
    is bounded to ~1e-2 of itself instead of 2 of itself."""
    n_fft, hop = frame_params(sr)
    X, fr, win = stft(y, sr)
    F = fr.shape[0]
    a = np.abs(fr * win)
    partner = np.minimum(np.arange(F) ^ 1, F - 1)
    z = np.sqrt(a * a + np.where((partner != np.arange(F))[:, None], a[partner] ** 2, 0.0))
    d = (fft_roundings(n_fft) * U * z.sum(axis=1))[:, None]
    d = d + U * (np.abs(X) + d)
    P = np.abs(X) ** 2
    dP = 2 * np.abs(X) * d + d * d + 4 * U * P
    W = data_ref.mel_basis(sr, n_fft).astype(np.float64)
    cnt = max(c for _, c in mel_bands(sr, n_fft)[0])
    return dP @ W.T + (cnt + 1) * U * (P @ W.T)


def gemm_path(y, sr):
    """The DFT-GEMM path's stages: dict of (ref, bound) for 'frames' [F][kp],
    'X' [F][2nb] (cos | sin), 'P' [F][nbp], 'mel' [F][128]."""
    n_fft, hop = frame_params(sr)
    nb, kp = n_fft // 2 + 1, (n_fft + 3) // 4 * 4
    nbp = (nb + 63) // 64 * 64
    Xc, fr, win = stft(y, sr)
    F = fr.shape[0]
    w32 = win.astype(np.float32).astype(np.float64)
    frames = np.zeros((F, kp))
    frames[:, :n_fft] = fr * win
    dframes = np.zeros((F, kp))
    dframes[:, :n_fft] = 2 * U * np.abs(fr * w32)        # window to f32, the product
    ph = 2 * np.pi * ((np.arange(nb)[:, None] * np.arange(n_fft)[None, :]) % n_fft) / n_fft
    mag = np.abs(fr * w32) @ np.concatenate([np.abs(np.cos(ph)), np.abs(np.sin(ph))]).T   # [F][2nb]
    X = np.concatenate([Xc.real, -Xc.imag], axis=1)     # the basis' sin rows are +sin
    # the f64 cos / sin the table is rounded from are within 2^-52 absolute of exact
    dX = (E32 + 3 * U) * mag + 2.0 ** -50 * np.abs(fr * w32).sum(axis=1, keepdims=True)
    c, s, dc, ds = np.abs(X[:, :nb]), np.abs(X[:, nb:]), dX[:, :nb], dX[:, nb:]
    P = np.zeros((F, nbp))
    dP = np.zeros((F, nbp))
    P[:, :nb] = c * c + s * s
    dP[:, :nb] = 2 * (c * dc + s * ds) + dc * dc + ds * ds + 3 * U * P[:, :nb]
    W = data_ref.mel_basis(sr, n_fft).astype(np.float64)
    mel = P[:, :nb] @ W.T
    dmel = dP[:, :nb] @ W.T + (E32 + 2 * U) * ((P[:, :nb] + dP[:, :nb]) @ W.T)
    return dict(frames=(frames, dframes), X=(X, dX), P=(P, dP), mel=(mel, dmel))


def mel_stage(y, sr):
    """(ref, bound) of the mel power [F][128] by the path sr takes."""
    if path(sr, len(y)) == "gemm":
        return gemm_path(y, sr)["mel"]
    ref = mel_power(y, sr)
    return ref, np.minimum(mel_bound_fused(ref), mel_bound_fft(y, sr))


# ---------------------------------------------------------------------------
# dB, floor, DCT
# ---------------------------------------------------------------------------
def dct32():
    """The kernel's table: f64 DCT-II ortho rows rounded to f32."""
    return data_ref.dct_ortho_matrix(N_MELS, N_MFCC).astype(np.float32).astype(np.float64)


def power_db(m):
    return 10.0 * np.log10(np.maximum(AMIN, m))


def _db_f32(db):
    """log10f (ELOG units of 2^-23 max(|log10|, 1)) and the multiplication by 10."""
    return 2 * ELOG * U * np.maximum(np.abs(db), 10.0) + U * np.abs(db)


def _db_range(m, d):
    """(lowest, highest) f32 dB the kernel can hold for a power within d of m (>= 0)."""
    lo, hi = power_db(np.maximum(m - d, 0.0)), power_db(m + d)
    return lo - _db_f32(lo), hi + _db_f32(hi)


def mfcc_ref(mel, dmel=None, top_db=TOP_DB):
    """(mfcc [23][F], bound, floored): mel [F][128] f64 and its per-element bound (None:
    mel is what the kernel read, exactly).  floored: the bands the reference clamps to
    max - top_db.  The clamped dB value is bounded by interval evaluation: the kernel
    holds max(dB, floor) with dB and floor each anywhere in its own range, so the value
    lies between the max of the two low ends and the max of the two high ends,
    whichever side of the floor the band falls on."""
    dmel = np.zeros_like(mel) if dmel is None else dmel
    db = power_db(mel)
    db_lo, db_hi = _db_range(mel, dmel)
    fl_lo, fl_hi = _db_range(mel.max(), dmel.max())
    floor = power_db(mel.max()) - top_db
    fl_lo, fl_hi = fl_lo - top_db - U * abs(floor), fl_hi - top_db + U * abs(floor)
    c = np.maximum(db, floor)
    dc = np.maximum(np.maximum(db_hi, fl_hi) - c, c - np.maximum(db_lo, fl_lo))
    D = dct32()
    ref = (c @ D.T).T
    bound = (dc @ np.abs(D).T + (N_MELS + 1) * U * ((np.abs(c) + dc) @ np.abs(D).T)).T
    return ref, bound, db < floor


# ---------------------------------------------------------------------------
# CMVN, Savitzky-Golay deltas, pair mean
# ---------------------------------------------------------------------------
def savgol_table(width=SG_W):
    """[2][width] f64: tap weights of the order-th derivative of the degree-order
    least-squares fit (order 1, 2).  With polyorder == deriv the derivative is the
    fit's leading coefficient times order!, the same at every position of the window,
    so scipy's mode='interp' edges are the first / last window's fit."""
    t = np.arange(width, dtype=np.float64)
    out = []
    for order in (1, 2):
        A = np.vander(t, order + 1, increasing=True)
        out.append(np.linalg.pinv(A)[order] * (1 if order == 1 else 2))
    return np.array(out)


def reduce_pairs(x):
    """data_ref.reduce_features on [C][F] -> [F60][C]."""
    return data_ref.reduce_features(x).T


def cmvn_ref(x32, ddof=0, width=SG_W):
    """(ref [F60][3C], bound) of nstl_cmvn_delta_reduce on f32 rows x32 [C][F], judged
    from those rows alone.

    The kernel: f64 sums S, Q of x and x^2; mean = f32(S / F); dev = Q - 2 mean S +
    F mean^2 in f64 = sum (x - mean)^2 about the rounded mean, up to f64 rounding of
    terms of size Q (taken as (F + 8) 2^-53 each); sd = sqrtf(f32(dev) / F), inv =
    1 / (sd + 1e-10f): five f32 roundings, two of them under the root.  So
      rho = d(dev) / (2 dev) + 4 U,  d(dev) = F (U mean)^2 + (F + 8) 2^-53 (Q + 2 |mean S| + F mean^2)
    and nv = fl(fl(x - mean) inv) is within
      d(nv) = inv (U |mean| + U |x - mean|) + |x - mean| inv (rho + U)
    of (x - mean64) inv64.  A constant row has x - mean == 0 exactly: ref 0, bound 0.
    Each delta is 9 fmas against the f32-rounded table: sum |sg| d(nv) + 10 U sum
    |sg nv|.  The pair mean is one rounded add (the halving is exact): (da + db +
    U |a + b|) / 2; an odd last frame is stored as it is."""
    x = np.asarray(x32, np.float64)
    C, F = x.shape
    mean = x.mean(axis=1, keepdims=True)
    dev = ((x - mean) ** 2).sum(axis=1, keepdims=True)
    sd = np.sqrt(dev / (F - ddof))
    inv = 1.0 / (sd + AMIN)
    xc = x - mean
    S, Q = np.abs(x.sum(axis=1, keepdims=True)), (x * x).sum(axis=1, keepdims=True)
    ddev = F * (U * mean) ** 2 + (F + 8) * 2.0 ** -53 * (Q + 2 * np.abs(mean) * S + F * mean * mean)
    const = x.max(axis=1, keepdims=True) == x.min(axis=1, keepdims=True)
    with np.errstate(divide="ignore", invalid="ignore"):
        rho = np.where(const, 0.0, ddev / (2 * dev)) + 4 * U
    assert np.all(rho < 0.25), "a row too close to constant for this bound"
    nv = xc * inv
    dnv = np.where(const, 0.0, inv * (U * np.abs(mean) + U * np.abs(xc)) + np.abs(nv) * (rho + U))
    sg = savgol_table(width)
    half = width // 2
    w0 = np.clip(np.arange(F) - half, 0, F - width)
    idx = w0[:, None] + np.arange(width)[None, :]           # [F][width]
    cols, dcols = [nv], [dnv]
    for o in (0, 1):
        cols.append((nv[:, idx] * sg[o]).sum(axis=2))
        dcols.append((dnv[:, idx] * np.abs(sg[o])).sum(axis=2)
                     + (width + 1) * U * (np.abs(nv[:, idx]) * np.abs(sg[o])).sum(axis=2))
    full, dfull = np.vstack(cols), np.vstack(dcols)
    ref = reduce_pairs(full)
    n2 = F // 2 * 2
    bound = reduce_pairs(dfull)
    bound[:n2 // 2] += (U * np.abs(full[:, 0:n2:2] + full[:, 1:n2:2]) / 2).T
    return ref, bound


# ---------------------------------------------------------------------------
# autocorrelation
# ---------------------------------------------------------------------------
def autocorr(y, L, hop, n_lags):
    """[F][n_lags] f64 (data_ref.autocorr_features_120, frame-major)."""
    return data_ref.autocorr_features_120(np.asarray(y, np.float32), L, hop, n_lags).T


def autocorr_tol(L):
    return dict(rtol=2e-6, atol=2e-7) if L >= 266 else dict(rtol=0, atol=3e-6)


def autocorr_bound(ref, L):
    t = autocorr_tol(L)
    return t["atol"] + t["rtol"] * np.abs(ref)


# ---------------------------------------------------------------------------
# the whole pipeline
# ---------------------------------------------------------------------------
def features(y, sr, **kw):
    """f64 [F60][256] of nstl_features at any sr (no bounds): kw reaches stft()."""
    n_fft, hop = frame_params(sr)
    mf = mfcc_ref(mel_power(y, sr, **kw))[0]
    m = data_ref.cmvn(mf)
    full = np.vstack([m, data_ref.savgol_delta(m, 1), data_ref.savgol_delta(m, 2)])
    ac = data_ref.reduce_features(data_ref.autocorr_features_120(np.asarray(y, np.float32), n_fft, hop, N_AC)).T
    return np.hstack([data_ref.reduce_features(full).T, ac])


def cmvn_propagated(mf, dmf):
    """(ref [F60][69], bound) of the MFCC half of the output from reference MFCC rows
    [23][F] known to within dmf: cmvn_ref's own bound at the reference rows (the f32
    rounding of the stored rows is one more U |x|), plus what an input error does to
    each stage, with the cross terms kept as an upper bound:
      mean moves by at most mean(dmf); x - mean by e = dmf + mean(dmf);
      sd by d sd = |e|_2 / sqrt(F)  (the population deviation is 1 / sqrt(F) times
      a 2-norm, 1-Lipschitz in it);
      nv by e inv' + |x - mean| inv (d sd) inv', inv' the inverse at sd - d sd.
    A row whose d sd reaches half its deviation is not constrained by its input
    bound: its bound is inf."""
    C, F = mf.shape
    ref, b0 = cmvn_ref(mf)
    dmf = dmf + U * np.abs(mf)
    e = dmf + dmf.mean(axis=1, keepdims=True)
    mean = mf.mean(axis=1, keepdims=True)
    sd = mf.std(axis=1, keepdims=True)
    dsd = np.sqrt((e * e).sum(axis=1, keepdims=True) / F)
    loose = dsd >= 0.5 * sd
    inv, inv_lo = 1.0 / (sd + AMIN), 1.0 / (np.where(loose, sd, sd - dsd) + AMIN)
    dnv = e * inv_lo + np.abs(mf - mean) * inv * dsd * inv_lo
    sg = np.abs(savgol_table())
    w0 = np.clip(np.arange(F) - SG_W // 2, 0, F - SG_W)
    idx = w0[:, None] + np.arange(SG_W)[None, :]
    dfull = np.vstack([dnv] + [(dnv[:, idx] * sg[o]).sum(axis=2) for o in (0, 1)])
    scale = np.where(loose, np.inf, (1 + 4 * U) * inv_lo / inv)
    return ref, b0 * np.tile(scale, (3, 1)).T + reduce_pairs(dfull)


def features_bounded(y, sr):
    """(ref [F60][256], bound): every stage's bound carried to the output."""
    n_fft, hop = frame_params(sr)
    mel, dmel = mel_stage(y, sr)
    mf, dmf, _ = mfcc_ref(mel, dmel)
    a, da = cmvn_propagated(mf, dmf)
    ac = autocorr(y, n_fft, hop, N_AC)
    r = reduce_pairs(ac.T)
    dr = reduce_pairs(autocorr_bound(ac, n_fft).T) + U * np.abs(r)   # the f32 store
    return np.hstack([a, r]), np.hstack([da, dr])
