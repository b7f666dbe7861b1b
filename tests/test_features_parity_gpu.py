"""The audio feature kernels (csrc/features.hip) against tests/features_ref.py, stage by
stage and end to end, at every path a sample rate can take.

nstl_features runs on a workspace of exactly nstl_features_workspace_bytes, filled
with 0xFF bytes (NaN as f32 and as f64), into an output of row stride 260 prefilled
with NaN, with one canary row after it.  Each stage is read back from the workspace
and judged by its own bound: mel power (db), the clip max (key), MFCC rows (mfcc),
autocorrelation lags (ac), then the output.  Which mel path ran is observed: the fused
kernels leave the frames and X regions untouched, the DFT-GEMM path fills X.

No stage is judged by a tolerance of its own: every bound is features_ref's.

NSTL_FEATURES_PARITY_ERRORS_OUT=<file>: the worst err / bound of every stage of every
case is appended (profiles/features_parity_errors.txt holds one such run)."""
import os

import numpy as np
import pytest
import torch

from tests import features_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NAN = float("nan")


def record(name, stage, ratio):
    line = "%-22s %-14s worst err/bound %.4f" % (name, stage, ratio)
    print(line)
    path = os.environ.get("NSTL_FEATURES_PARITY_ERRORS_OUT")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


def judge(name, stage, got, ref, bound, bad):
    got = np.asarray(got, np.float64)
    assert got.shape == ref.shape, (stage, got.shape, ref.shape)
    err = np.abs(got - ref)
    ok = np.isfinite(got).all() and bool(np.all(err <= bound))
    with np.errstate(invalid="ignore", divide="ignore"):
        q = np.where(err == 0, 0.0, err / bound)
    ratio = float(np.nanmax(q)) if np.isfinite(got).all() else float("inf")
    record(name, stage, ratio)
    if not ok:
        bad.append((stage, ratio))


def untouched(raw):
    return bool((raw == 0xFF).all())


def run_features(y, sr):
    """One nstl_features call; the regions of the workspace and the output, on the CPU."""
    from neurosync_trainer_lite_amd import _hip as K
    n = len(y)
    L = R.feat_layout(n, sr)
    assert L["total"] == K.features_workspace_bytes(n, sr), "the restated layout and the library's disagree"
    assert L["F60"] == K.features_frames(n, sr)
    ws = torch.full((L["total"],), 0xFF, dtype=torch.uint8, device=DEV)
    out = torch.full((L["F60"] + 1, 260), NAN, dtype=torch.float32, device=DEV)
    K.features(torch.tensor(y, dtype=torch.float32, device=DEV), sr, out[:L["F60"]], ws)
    torch.cuda.synchronize()
    raw = ws.cpu().numpy()
    F, nb = L["F"], L["nb"]

    def region(key, count, dtype):
        return raw[L[key]:L[key] + count * np.dtype(dtype).itemsize].view(dtype)
    g = dict(L=L, out=out.cpu().numpy(),
             frames_raw=raw[L["frames"]:L["X"]], X_raw=raw[L["X"]:L["db"]],
             frames=region("frames", F * L["kp"], np.float32), X=region("X", F * 2 * nb, np.float32).reshape(F, 2 * nb),
             mel=region("db", F * 128, np.float32).reshape(F, 128), mfcc=region("mfcc", 23 * F, np.float32).reshape(23, F),
             ac=region("ac", F * 187, np.float64).reshape(F, 187), key=region("key", 1, np.int32)[0])
    return g


def judge_features(name, y, sr, want_path):
    g = run_features(y, sr)
    L = g["L"]
    F, F60, nb, kp, nbp, n_fft, hop = L["F"], L["F60"], L["nb"], L["kp"], L["nbp"], L["n_fft"], L["hop"]
    bad = []
    out = g["out"]
    assert np.isnan(out[F60]).all(), "the row after the output was written"
    assert np.isnan(out[:F60, 256:]).all(), "columns 256..259 were written"
    # which path ran
    assert R.path(sr, len(y)) == want_path
    if want_path == "gemm":
        assert np.isfinite(g["X"]).all(), "DFT-GEMM path: X not filled"
        st = R.gemm_path(y, sr)
        judge(name, "X", g["X"], *st["X"], bad)
        P = g["frames"][:F * nbp].reshape(F, nbp)
        judge(name, "P", P, *st["P"], bad)
        assert np.all(P[:, nb:] == 0), "P's zero tail"
        if nbp < kp:   # the end of the frames buffer that P does not cover still holds frames
            k0 = F * nbp
            fr, dfr = st["frames"]
            judge(name, "frames-tail", g["frames"][k0:], fr.reshape(-1)[k0:], dfr.reshape(-1)[k0:], bad)
            rows = g["frames"].reshape(F, kp)[(k0 + kp - 1) // kp:, n_fft:]
            assert (rows.size > 0) == (kp > n_fft) and np.all(rows == 0), "frames' pad columns"
    else:
        assert untouched(g["X_raw"]) and untouched(g["frames_raw"]), "fused path wrote the frames / X regions"
    ref_mel, dmel = R.mel_stage(y, sr)
    judge(name, "mel", g["mel"], ref_mel, dmel, bad)
    # the clip max: the max of the GPU's own mel values, bit for bit
    assert g["key"] == g["mel"].max().view(np.int32), "key is not the max of the mel buffer"
    judge(name, "key", g["key"].view(np.float32).reshape(1), ref_mel.max().reshape(1), dmel.max().reshape(1), bad)
    # MFCC: the dB / DCT stage alone, from the GPU's own mel; then from the reference
    r, b, _ = R.mfcc_ref(g["mel"].astype(np.float64))
    judge(name, "mfcc|mel", g["mfcc"], r, b, bad)
    r, b, floored = R.mfcc_ref(ref_mel, dmel)
    judge(name, "mfcc", g["mfcc"], r, b, bad)
    # CMVN, deltas, pair mean from the GPU's own MFCC rows
    judge(name, "cmvn|mfcc", out[:F60, :69], *R.cmvn_ref(g["mfcc"]), bad)
    # autocorrelation lags and their reduction
    ac = R.autocorr(y, n_fft, hop, 187)
    judge(name, "ac", g["ac"], ac, R.autocorr_bound(ac, n_fft), bad)
    assert np.array_equal(out[:F60, 69:256], R.reduce_pairs(g["ac"].T).astype(np.float32)), "pair means of the lags"
    # end to end under the propagated bound
    full, fb = R.features_bounded(y, sr)
    judge(name, "out[:, :69]", out[:F60, :69], full[:, :69], fb[:, :69], bad)
    judge(name, "out[:, 69:]", out[:F60, 69:256], full[:, 69:], fb[:, 69:], bad)
    assert not bad, (name, bad)
    return g, floored


@pytest.mark.parametrize("sr", sorted(R.RATES))
def test_features_every_rate(sr):
    n_fft, want_path, F = R.RATES[sr]
    assert R.frame_params(sr)[0] == n_fft
    y = R.clip(sr, F, 100 + sr % 97)
    g, _ = judge_features("features-%d" % sr, y, sr, want_path)
    assert g["L"]["F"] == F
    if sr == 12000:
        empty = [m for m, (_, c) in enumerate(R.mel_bands(sr, n_fft)[0]) if c == 0]
        assert empty and np.all(g["mel"][:, empty] == 0), "12 kHz: filters without a bin"


@pytest.mark.parametrize("sr", [44100, 22050])
def test_features_odd_n_fft_clip_of_whole_hops(sr):
    """An odd n_fft (735, 367) and a clip of exactly 20 hops: n_fft / 2 of padding each
    side is one sample short of n_fft, so the clip has 20 centred frames, not 1 + n / hop
    = 21 (the count every even n_fft has).  Both branches must agree on it."""
    n_fft, want_path, _ = R.RATES[sr]
    y = R.clip(sr, 21, 7, extra=0)
    assert len(y) == 20 * (n_fft // 2) and n_fft % 2 == 1
    g, _ = judge_features("features-%d-20hops" % sr, y, sr, want_path)
    assert g["L"]["F"] == 20


def test_features_floor_active_at_88200():
    """A silent lead-in: the first frames' bands lie under max - 80 dB in the reference."""
    y = R.clip(88200, 40, 12)
    y[:4000] = 0
    _, floored = judge_features("features-88200-silent", y, 88200, "wave")
    assert floored.any() and not floored.all()


@pytest.mark.parametrize("sr,F", [(88200, 30), (16000, 30), (88200, 515)])
def test_features_all_zero_clip(sr, F):
    """Every frame of a silent clip goes through the same arithmetic: mel 0, the MFCC
    rows constant, x - mean exactly 0, every lag 0 (lag 0 == 0: no normalisation).  The
    bound is 0: the output is exact zeros, not NaN from 0 / 0 or sqrt of a negative.
    515 frames: the f64 sums of a constant row's squares no longer come out exact, and
    the expanded deviation Q - 2 mean S + F mean^2 can round to below zero."""
    y = np.zeros((F - 1) * R.frame_params(sr)[1] + 17, np.float32)
    g = run_features(y, sr)
    F60 = g["L"]["F60"]
    assert np.all(g["mel"] == 0) and g["key"] == 0
    assert np.all(g["mfcc"] == g["mfcc"][:, :1]) and np.isfinite(g["mfcc"]).all()
    assert abs(g["mfcc"][0, 0] - R.mfcc_ref(np.zeros((1, 128)))[0][0, 0]) <= R.mfcc_ref(np.zeros((1, 128)))[1][0, 0]
    assert np.all(g["ac"] == 0)
    assert np.isfinite(g["out"][:F60, :256]).all() and np.all(g["out"][:F60, :256] == 0)
    assert np.isnan(g["out"][F60]).all() and np.isnan(g["out"][:F60, 256:]).all()


# ---------------------------------------------------------------------------
# nstl_stft_mel: the key == nullptr arm of both fused kernels
# ---------------------------------------------------------------------------
def run_stft_mel(name, y, sr, F):
    from neurosync_trainer_lite_amd import _hip as K
    yd = torch.tensor(y, dtype=torch.float32, device=DEV)
    mel = torch.full((F + 1, 128), NAN, dtype=torch.float32, device=DEV)
    K.stft_mel(yd, len(y), sr, mel, F)
    torch.cuda.synchronize()
    got = mel.cpu().numpy()
    assert np.isnan(got[F]).all(), "the row after the last frame was written"
    bad = []
    judge(name, "mel", got[:F], *R.mel_stage(y, sr), bad)
    assert not bad, (name, bad)
    with pytest.raises(RuntimeError, match="n_frames"):
        K.stft_mel(yd, len(y), sr, mel, F + 1)


@pytest.mark.parametrize("sr,F", [(44100, 21), (44100, 14), (12000, 13), (120000, 17), (120000, 18), (120000, 23)])
def test_stft_mel(sr, F):
    """120 kHz: the workgroup kernel takes 8 frames per workgroup; F % 8 = 1, 2, 7."""
    y = R.clip(sr, F, 200 + F)
    assert R.n_frames(len(y), *R.frame_params(sr)) == F
    run_stft_mel("stft_mel-%d-F%d" % (sr, F), y, sr, F)


@pytest.mark.parametrize("sr,F", [(88200, 21), (120000, 17)])
def test_stft_mel_odd_last_frame_has_no_partner(sr, F):
    """F odd: the last frame goes through the complex FFT alone, its imaginary part
    zero.  A clip of F hop - 1 samples, nearly silent but for 8 loud samples at its
    very end: the last frame sees them under the window's last 10 taps (weights below
    4e-4), while the frame after it (which does not exist: n_frames = F) would see them
    at the window's peak.  Were those samples loaded as a partner frame, the last
    frame would carry f32 rounding of an energy ~1e4 times its own, far over its bound
    (which knows no partner)."""
    hop = R.frame_params(sr)[1]
    n = F * hop - 1
    rng = np.random.default_rng(F)
    y = (1e-6 * rng.standard_normal(n)).astype(np.float32)
    y[-9:-1] = rng.choice([-1.0, 1.0], 8)
    assert R.n_frames(n, 2 * hop, hop) == F and F % 2 == 1
    run_stft_mel("stft_mel-%d-loud-tail" % sr, y, sr, F)


def test_stft_mel_several_pairs_per_wave():
    """The wave kernel gives each wave ppw = ceil(pairs / (CUs x workgroups per CU x 4))
    pairs in turn; above one, the buffer is refilled while the previous pair's mel
    reads may still be in flight.  Workgroups per CU: the kernel's 78 KB of LDS
    (features_ref.wave_lds) in the CU's 160 KB, which is what the occupancy query of
    the launcher returns when LDS is the limit (it is: 256 threads, < 128 VGPRs)."""
    sr, (n_fft, hop) = 88200, R.frame_params(88200)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    per_cu = 160 * 1024 // R.wave_lds(n_fft, R.mel_bands(sr, n_fft)[1])
    assert per_cu == 2
    F = 2 * cus * per_cu * R.SW_WAVES + 1        # one pair more than the waves: ppw = 2
    assert (F + 1) // 2 > cus * per_cu * R.SW_WAVES and F % 2 == 1
    y = R.clip(sr, F, 31)
    run_stft_mel("stft_mel-ppw2-F%d" % F, y, sr, F)


# ---------------------------------------------------------------------------
# the frame-axis stages on their own
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("C,F", [(1, 9), (23, 10), (23, 31), (23, 33), (64, 513), (23, 515)])
def test_cmvn_delta_reduce(C, F):
    """F = 9: every frame an edge fit; F < 32: chunks of one frame, some empty; F60 >
    256: a second block row; 64 rows: the limit.  Row 1 constant (exact zeros out),
    row 2 one large value with a single outlier; ld_out = 3 C + 5 with the pad checked."""
    from neurosync_trainer_lite_amd import _hip as K
    x = R.cmvn_case(C, F)
    F60, ld = (F + 1) // 2, 3 * C + 5
    out = torch.full((F60 + 1, ld), NAN, dtype=torch.float32, device=DEV)
    K.cmvn_delta_reduce(torch.tensor(x, device=DEV), out[:F60])
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert np.isnan(got[F60]).all() and np.isnan(got[:F60, 3 * C:]).all(), "pad written"
    bad = []
    ref, bound = R.cmvn_ref(x)
    judge("cmvn-%dx%d" % (C, F), "out", got[:F60, :3 * C], ref, bound, bad)
    assert not bad, bad
    if C > 2:
        assert np.all(got[:F60, [1, C + 1, 2 * C + 1]] == 0), "constant row"


def test_cmvn_delta_reduce_rejections():
    from neurosync_trainer_lite_amd import _hip as K
    out = torch.zeros(300, 3 * 65 + 5, device=DEV)
    with pytest.raises(RuntimeError, match="ncoef"):
        K.cmvn_delta_reduce(torch.zeros(65, 20, device=DEV), out)
    with pytest.raises(RuntimeError, match="bad sizes"):
        K.cmvn_delta_reduce(torch.zeros(23, 8, device=DEV), out)
    torch.cuda.synchronize()
    assert not out.any()


@pytest.mark.parametrize("F,cols,col0", [(1, 5, 0), (2, 5, 2), (3, 5, 1), (515, 187, 69)])
def test_reduce_frame_pairs_bit_for_bit(F, cols, col0):
    from neurosync_trainer_lite_amd import _hip as K
    x = np.random.default_rng(F).standard_normal((F, cols))
    F60, ld = (F + 1) // 2, col0 + cols + 4
    out = torch.full((F60 + 1, ld), NAN, dtype=torch.float32, device=DEV)
    K.reduce_frame_pairs(torch.tensor(x, device=DEV), out[:F60], col0=col0)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert np.array_equal(got[:F60, col0:col0 + cols], R.reduce_pairs(x.T).astype(np.float32))
    assert np.isnan(got[F60]).all() and np.isnan(got[:, :col0]).all() and np.isnan(got[:, col0 + cols:]).all()


# ---------------------------------------------------------------------------
# nstl_autocorr
# ---------------------------------------------------------------------------
def run_autocorr(name, y, L, hop, n_lags, rows_after=3):
    from neurosync_trainer_lite_amd import _hip as K
    n = len(y)
    F = (n + 2 * (L // 2) - L) // hop + 1
    out = torch.full((F + rows_after, n_lags), NAN, dtype=torch.float64, device=DEV)
    K.autocorr(torch.tensor(y, dtype=torch.float32, device=DEV), L, hop, n_lags, out, F)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert np.isnan(got[F:]).all(), "rows after the last frame were written"
    ref = R.autocorr(y, L, hop, n_lags)
    assert ref.shape == (F, n_lags)
    bad = []
    judge(name, "ac", got[:F], ref, R.autocorr_bound(ref, L), bad)
    assert not bad, (name, bad)
    return ref


# 191 is the largest lag count either kernel can form: autocorr3 completes lags
# 16 (t - 1) .. 16 t - 1 per tile t = 1..12, autocorr2 has 12 groups of 16 lags (0..191),
# and nstl_autocorr refuses n_lags >= 192 before choosing between them.
@pytest.mark.parametrize("L,hop,n_lags,kernel", [
    (1470, 735, 191, "mfma"), (735, 367, 187, "mfma"), (200, 100, 187, "mfma"), (192, 96, 191, "mfma"),
    (210, 105, 191, "mfma"), (209, 104, 191, "mfma"), (2048, 1024, 191, "valu"), (3200, 1600, 187, "valu")])
@pytest.mark.parametrize("n_frames", [2, 3, 5, 9])
def test_autocorr_lag_and_frame_counts(L, hop, n_lags, kernel, n_frames):
    """Lag counts at the limit, on both kernels; 2, 3, 5 and 9 frames (n_frames % 4 != 0:
    the last workgroup of autocorr3 is partial), with NaN rows after the last frame."""
    assert R.autocorr_kernel(L, n_lags) == kernel
    from tests.golden.make_goldens_helpers import synth_audio
    n = (n_frames - 1) * hop + (1 if L % 2 else 0) + 5
    assert (n + 2 * (L // 2) - L) // hop + 1 == n_frames and n > L // 2
    y = synth_audio((n + 8) / 88200, 40 + n_frames)[:n]
    run_autocorr("ac-%d-%d-F%d" % (L, n_lags, n_frames), y, L, hop, n_lags)


@pytest.mark.parametrize("L,hop", [(1470, 735), (735, 367), (2048, 1024)])
def test_autocorr_zero_frame_in_the_middle(L, hop):
    """2000 (3000 for L = 2048) zero samples inside the clip: a frame with lag 0 == 0
    keeps its unnormalised (zero) lags, and it is not an edge frame."""
    from tests.golden.make_goldens_helpers import synth_audio
    y = synth_audio(0.2, 51)
    z = 2000 if L < 2000 else 3000
    y[6 * hop:6 * hop + z] = 0
    ref = run_autocorr("ac-%d-zero-middle" % L, y, L, hop, 187)
    zero = np.nonzero(np.all(ref == 0, axis=1))[0]
    assert zero.size > 0 and zero.min() > 0 and zero.max() < ref.shape[0] - 1


@pytest.mark.parametrize("n_frames,silence", [(3, "all"), (3, "first"), (2, "first"), (2, "all")])
def test_autocorr_silent_edge_frames_in_short_clips(n_frames, silence):
    """fix_edge_frames_autocorr with 2 or 3 frames.  With hop = L / 2 the first and the
    last of three frames cover the clip between them, so both are silent only when the
    whole clip is: every row stays zero (the copies are of zero rows).  A silent first
    frame alone takes its neighbour's lags; with two frames that neighbour is the last."""
    from tests.golden.make_goldens_helpers import synth_audio
    L, hop = 1470, 735
    n = (n_frames - 1) * hop + 5
    y = synth_audio((n + 8) / 88200, 52)[:n]
    y[:n if silence == "all" else hop + 1] = 0
    ref = run_autocorr("ac-silent-%s-F%d" % (silence, n_frames), y, L, hop, 187)
    assert ref.shape[0] == n_frames
    if silence == "all":
        assert not ref.any()
    else:
        assert ref[1].any() and np.array_equal(ref[0], ref[1])


@pytest.mark.parametrize("L,hop", [(1470, 735), (735, 367), (2048, 1024)])
def test_autocorr_clip_barely_longer_than_half_a_frame(L, hop):
    """n_samples = L/2 + 1, the shortest legal clip: the reflect padding is as long as
    the clip allows on both sides."""
    from tests.golden.make_goldens_helpers import synth_audio
    y = synth_audio(0.05, 53)[:L // 2 + 1]
    run_autocorr("ac-%d-shortest" % L, y, L, hop, 187)


@pytest.mark.parametrize("change,match", [
    (dict(n_lags=1470), "bad lags"), (dict(n_lags=208), "bad lags"), (dict(n_lags=192), "bad lags"),
    (dict(n_frames=11), "n_frames"), (dict(n_frames=9), "n_frames"), (dict(n=735), "bad sizes")])
def test_autocorr_rejections(change, match):
    from neurosync_trainer_lite_amd import _hip as K
    v = dict(dict(n=9 * 735 + 5, n_lags=187, n_frames=10), **change)
    y = torch.zeros(9 * 735 + 5, device=DEV)[:v["n"]]
    out = torch.zeros(12, 1470, dtype=torch.float64, device=DEV)
    with pytest.raises(RuntimeError, match=match):
        K.autocorr(y, 1470, 735, v["n_lags"], out, v["n_frames"])
    torch.cuda.synchronize()
    assert not out.any()
