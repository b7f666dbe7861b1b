"""tests/features_ref.py proved before it judges a kernel (no GPU): against
oracle/data_ref.extract_features at 88.2 kHz, the reference-generated fixtures, scipy's
Savitzky-Golay filter, the sample-rate -> path table checked by hand, an f32 emulation
of every stage that must stay under the stage's bound at every shape the GPU test
uses, and wrong references that must exceed it."""
import numpy as np
import pytest
import scipy.fft

from oracle import data_ref
from tests import features_ref as R
from tests.golden.make_goldens_helpers import synth_audio

f32 = np.float32


def silent_clip():
    y = R.clip(88200, 40, 12)
    y[:4000] = 0
    return y


# ---------------------------------------------------------------------------
# the reference is the oracle and the fixtures
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("seconds,seed", [(0.6, 3), (0.09, 7)])
def test_equals_extract_features_at_88200(seconds, seed):
    y = synth_audio(seconds, seed)
    want = data_ref.extract_features(y)
    got = R.features(y, 88200)
    assert got.shape == want.shape
    # the kernel's 1e-10f and f32 DCT table instead of the f64 ones: 1e-7 of an MFCC
    # of a few hundred, CMVN'd
    np.testing.assert_allclose(got[:, :69], want[:, :69], rtol=0, atol=1e-6)
    assert np.array_equal(got[:, 69:], want[:, 69:])
    ref, bound = R.features_bounded(y, 88200)
    assert np.all(np.abs(ref - want) <= 1e-6) and np.all(np.isfinite(bound))


def test_matches_reference_fixtures(golden):
    g = golden("features_autocorr.npz")
    cases = [(synth_audio(1.0, 3), g["ac_3"]), (synth_audio(0.73, 4), g["ac_4"])]
    y = synth_audio(0.5, 5)
    y[:3000] = 0
    y[-3000:] = 0
    cases.append((y, g["ac_silent_edges"]))
    for y, want in cases:
        np.testing.assert_allclose(R.reduce_pairs(R.autocorr(y, 1470, 735, 187).T), want, rtol=1e-12, atol=1e-15)
    for key, out in (("reduce_in", "reduce_out"), ("reduce_in_even", "reduce_out_even")):
        assert np.array_equal(R.reduce_pairs(g[key]), g[out].T)
    x = g["reduce_in"]
    C = x.shape[0]
    ref, bound = R.cmvn_ref(x)
    np.testing.assert_allclose(ref[:, :C], R.reduce_pairs(g["cmvn_out"]), rtol=1e-9, atol=1e-12)
    for o in (1, 2):
        np.testing.assert_allclose(ref[:, o * C:(o + 1) * C], R.reduce_pairs(data_ref.savgol_delta(g["cmvn_out"], o)),
                                   rtol=1e-9, atol=1e-10)
    assert np.all(bound > 0) and np.all(bound < 1e-4)


def test_savgol_table_is_scipys_filter():
    x = np.random.default_rng(0).standard_normal((3, 31))
    sg = R.savgol_table()
    for o in (1, 2):
        want = data_ref.savgol_delta(x, o)
        w0 = np.clip(np.arange(31) - 4, 0, 31 - 9)
        got = (x[:, w0[:, None] + np.arange(9)[None, :]] * sg[o - 1]).sum(axis=2)
        np.testing.assert_allclose(got, want, rtol=1e-10, atol=1e-12)


# ---------------------------------------------------------------------------
# sizes and paths
# ---------------------------------------------------------------------------
HAND = {  # sr: (int(0.01667 sr), its factors over 4 2 3 5 7 or [] , path)
    12000: (200, [4, 2, 5, 5], "wave"), 16000: (266, [], "gemm"), 22050: (367, [], "gemm"),
    44100: (735, [3, 5, 7, 7], "wave"), 48000: (800, [4, 4, 2, 5, 5], "wave"),
    88200: (1470, [2, 3, 5, 7, 7], "wave"), 120000: (2000, [4, 4, 5, 5, 5], "wg"),
    192000: (3200, [4, 4, 4, 2, 5, 5], "gemm"), 96000: (1600, [4, 4, 4, 5, 5], "wg"), 32000: (533, [], "gemm"),
}


@pytest.mark.parametrize("sr", sorted(HAND))
def test_path_rule(sr):
    n_fft, radices, want = HAND[sr]
    assert R.frame_params(sr) == (n_fft, n_fft // 2)
    assert R.fft_radices(n_fft) == radices
    assert int(np.prod(radices)) == (n_fft if radices else 1)
    assert R.path(sr) == want
    if sr in R.RATES:
        assert R.RATES[sr][:2] == (n_fft, want)


def test_sizes_read_from_the_kernels():
    L = R.feat_layout(24 * 133 - 116, 16000)
    assert (L["kp"], L["nbp"], L["nb"], L["F"]) == (268, 192, 134, 24)
    assert R.feat_layout(1000, 22050)["kp"] == 368
    assert R.fused_lds(3200, R.mel_bands(192000, 3200)[1]) > 65536 >= R.fused_lds(2000, R.mel_bands(120000, 2000)[1])
    assert any(c == 0 for _, c in R.mel_bands(12000, 200)[0]), "12 kHz: no empty mel filter"
    assert all(c > 0 for _, c in R.mel_bands(88200, 1470)[0])
    assert R.path(88200, 1 << 29) == "wg"
    # the wave kernel at 88.2 kHz: two workgroups in a CU's 160 KB of LDS
    assert 160 * 1024 // R.wave_lds(1470, R.mel_bands(88200, 1470)[1]) == 2
    assert R.autocorr_kernel(1470, 187) == "mfma" and R.autocorr_kernel(1470, 191) == "mfma"
    assert R.autocorr_kernel(1856, 187) == "mfma" and R.autocorr_kernel(1857, 187) == "valu"
    assert R.autocorr_kernel(3200, 187) == "valu"


def test_workspace_layout_matches_the_library():
    from neurosync_trainer_lite_amd import _hip as K
    for sr, (_, _, F) in R.RATES.items():
        n = len(R.clip(sr, F, 1))
        assert R.feat_layout(n, sr)["total"] == K.features_workspace_bytes(n, sr), sr
        assert R.feat_layout(n, sr)["F60"] == K.features_frames(n, sr), sr


# ---------------------------------------------------------------------------
# f32 emulation of the kernels' arithmetic, under every bound
# ---------------------------------------------------------------------------
def fma_chain(table, x):
    """acc = fmaf(table[k][m], x[f][m], acc) over m, f32: [F][K]."""
    acc = np.zeros((x.shape[0], table.shape[0]), f32)
    t64, x64 = table.astype(np.float64), x.astype(np.float64)
    for m in range(x.shape[1]):
        acc = (t64[None, :, m] * x64[:, m, None] + acc.astype(np.float64)).astype(f32)
    return acc


def emulate_mel(y, sr):
    n_fft, hop = R.frame_params(sr)
    fr = R.stft_frames(y, n_fft, hop).astype(f32)                      # [n_fft][F]
    fw = fr * R.hann_periodic(n_fft).astype(f32)[:, None]
    W = data_ref.mel_basis(sr, n_fft)
    if R.path(sr) == "gemm":
        nb = n_fft // 2 + 1
        ph = 2 * np.pi * ((np.arange(nb)[:, None] * np.arange(n_fft)[None, :]) % n_fft) / n_fft
        c, s = fw.T @ np.cos(ph).astype(f32).T, fw.T @ np.sin(ph).astype(f32).T
        X = np.concatenate([c, s], axis=1)
        return (c * c + s * s) @ W.T, X
    spec = scipy.fft.rfft(fw, axis=0)
    assert spec.dtype == np.complex64
    return (spec.real ** 2 + spec.imag ** 2).T @ W.T, None


def emulate_mfcc(mel, top_db=80.0):
    db = f32(10) * np.log10(np.maximum(f32(1e-10), mel))
    floor = f32(10) * np.log10(np.maximum(f32(1e-10), mel.max())) - f32(top_db)
    return fma_chain(R.dct32().astype(f32), np.maximum(db, floor)).T


def emulate_cmvn(x):
    C, F = x.shape
    x64 = x.astype(np.float64)
    S, Q = x64.sum(axis=1), (x64 * x64).sum(axis=1)
    mean = (S / F).astype(f32)
    dev = Q - 2.0 * mean.astype(np.float64) * S + F * mean.astype(np.float64) ** 2
    inv = f32(1) / (np.sqrt(dev.astype(f32) / f32(F)) + f32(1e-10))
    nv = (x - mean[:, None]) * inv[:, None]
    sg = R.savgol_table().astype(f32)
    w0 = np.clip(np.arange(F) - 4, 0, F - 9)
    rows = [nv]
    for o in (0, 1):
        d = np.zeros((C, F), f32)
        for t in range(9):
            d = (np.float64(sg[o, t]) * nv[:, w0 + t].astype(np.float64) + d.astype(np.float64)).astype(f32)
        rows.append(d)
    full = np.vstack(rows)
    n2 = F // 2 * 2
    out = (full[:, 0:n2:2] + full[:, 1:n2:2]) * f32(0.5)
    if F % 2:
        out = np.hstack([out, full[:, -1:]])
    return out.T


def worst(got, ref, bound):
    return float(np.max(np.abs(got.astype(np.float64) - ref) / (bound + 1e-300)))


@pytest.mark.parametrize("sr", sorted(R.RATES))
def test_f32_emulation_is_under_every_bound(sr):
    y = R.clip(sr, R.RATES[sr][2], 100 + sr % 97)
    mel32, X32 = emulate_mel(y, sr)
    assert mel32.dtype == f32
    ref, bound = R.mel_stage(y, sr)
    assert worst(mel32, ref, bound) < 1
    if X32 is not None:
        assert worst(X32, *R.gemm_path(y, sr)["X"]) < 1
    # the DCT stage alone (from the f32 mel), and from the reference with the mel bound
    mf32 = emulate_mfcc(mel32)
    r, b, _ = R.mfcc_ref(mel32.astype(np.float64))
    assert worst(mf32, r, b) < 1
    r, b, _ = R.mfcc_ref(ref, bound)
    assert worst(mf32, r, b) < 1
    out32 = emulate_cmvn(mf32)
    assert worst(out32, *R.cmvn_ref(mf32)) < 1
    full, fb = R.features_bounded(y, sr)
    assert worst(out32, full[:, :69], fb[:, :69]) < 1


def test_f32_emulation_with_the_floor_active():
    y = silent_clip()
    ref, bound = R.mel_stage(y, 88200)
    r, b, floored = R.mfcc_ref(ref, bound)
    assert floored.any() and not floored.all()
    mel32 = emulate_mel(y, 88200)[0]
    assert worst(mel32, ref, bound) < 1
    assert worst(emulate_mfcc(mel32), r, b) < 1


@pytest.mark.parametrize("C,F", [(1, 9), (23, 10), (23, 31), (23, 33), (64, 513), (23, 515)])
def test_f32_cmvn_emulation_at_the_stage_shapes(C, F):
    x = R.cmvn_case(C, F)
    ref, bound = R.cmvn_ref(x)
    assert worst(emulate_cmvn(x), ref, bound) < 1
    if C > 2:
        assert np.all(ref[:, [1, C + 1, 2 * C + 1]] == 0) and np.all(bound[:, [1, C + 1, 2 * C + 1]] == 0)


# ---------------------------------------------------------------------------
# wrong references exceed the bounds
# ---------------------------------------------------------------------------
def test_wrong_references_exceed_the_bounds():
    sr, (n_fft, hop) = 88200, R.frame_params(88200)
    y = silent_clip()
    ref, bound = R.mel_stage(y, sr)
    F = ref.shape[0]
    # symmetric window
    assert worst(R.mel_power(y, sr, window=np.hanning(n_fft)), ref, bound) > 1
    # odd frames one sample late
    fr = R.stft_frames(y, n_fft, hop, F)
    fr[:, 1::2] = R.stft_frames(np.concatenate([y[1:], [0.0]]), n_fft, hop, F)[:, 1::2]
    late = (np.abs(np.fft.rfft(fr * R.hann_periodic(n_fft)[:, None], axis=0)) ** 2).T \
        @ data_ref.mel_basis(sr, n_fft).astype(np.float64).T
    assert worst(late, ref, bound) > 1
    # floor at 70 dB: the DCT stage's own bound (mel taken as given)
    r, b, floored = R.mfcc_ref(ref)
    assert floored.any()
    assert worst(R.mfcc_ref(ref, top_db=70.0)[0], r, b) > 1
    # sample deviation, delta width 7: from the f32 MFCC rows
    x = r.astype(f32)
    cr, cb = R.cmvn_ref(x)
    assert worst(R.cmvn_ref(x, ddof=1)[0][:, :23], cr[:, :23], cb[:, :23]) > 1
    assert worst(R.cmvn_ref(x, width=7)[0][:, 23:], cr[:, 23:], cb[:, 23:]) > 1
