"""Audio ingest on the device, end to end: the ``*_device`` loaders of
utils/audio/load_audio.py, ``extract_audio_features(..., device_ingest=True)`` and the
serving helper utils/generate_face_shapes.py against the host forms.

88.2 kHz input needs no resampling: everything must equal the host path exactly.

48 kHz and 16 kHz input is resampled, by scipy on the host and by nstl_resample_poly on
the device: two f32 evaluations of one filter.
  samples  |device - host| <= 2 bound, bound = tests/resample_ref.py's per-element bound
           (one for each side).  After the peak normalisation y / m, with m the peak,
           |m_d - m_h| <= max 2 bound, so the quotients differ by at most
           (2 bound_i + |y_i / m| max 2 bound) / m and two roundings of a value <= 1 (2^-23).
  features the host path itself moves by d_host = max |features(scipy's f32 samples) -
           features(the f64 restatement rounded to f32)| on the same clip; the device
           samples are a second, independent f32 evaluation, so its features may differ
           from the host's by 2 d_host.  Both are computed here, on the clip under test.

NSTL_RESAMPLE_PARITY_ERRORS_OUT=<file>: the figures are appended
(profiles/resample_parity_errors.txt holds one such run)."""
import os

import numpy as np
import pytest
import torch

from tests import resample_ref as R
from tests.golden.make_goldens_helpers import synth_audio

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
TARGET = 88200
_cache = {}


def record(line):
    print(line)
    path = os.environ.get("NSTL_RESAMPLE_PARITY_ERRORS_OUT")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


def wav_bytes(sr, seconds, seed, tmp_path):
    from neurosync_trainer_lite_amd.utils.audio.load_audio import write_wav
    path = str(tmp_path / ("clip_%d.wav" % sr))
    write_wav(path, 0.8 * synth_audio(seconds, seed, sr=sr), sr)
    with open(path, "rb") as f:
        return path, f.read()


def small_model():
    if "model" not in _cache:
        from neurosync_trainer_lite_amd.config import training_config
        from neurosync_trainer_lite_amd.utils.model_utils import build_model
        from oracle import model_ref
        cfg = dict(training_config, hidden_dim=128, num_heads=2, n_layers=1, dropout=0.0, frame_size=32, overlap=8)
        model = build_model(cfg, torch.device(DEV))
        model.load_state_dict(model_ref.seeded_params(model_ref.param_shapes(256, 128, 1, 61), 33), strict=True)
        _cache["model"] = (model, cfg)
    return _cache["model"]


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


# ---------------------------------------------------------------------------
# 88.2 kHz: exact
# ---------------------------------------------------------------------------
def test_88200_loaders_features_and_serving_equal_the_host_path(tmp_path):
    from neurosync_trainer_lite_amd.utils import generate_face_shapes as G
    from neurosync_trainer_lite_amd.utils.audio import load_audio as A
    from neurosync_trainer_lite_amd.utils.audio.extraction.extract_features import extract_audio_features
    from neurosync_trainer_lite_amd.utils.audio.processing.audio_processing import process_audio_features
    path, data = wav_bytes(TARGET, 3.0, 11, tmp_path)
    for host, dev in ((A.load_audio(path), A.load_audio_device(path)),
                      (A.load_and_preprocess_audio(path), A.load_and_preprocess_audio_device(path)),
                      (A.load_audio_from_bytes(data), A.load_audio_from_bytes_device(data))):
        assert dev[1] == host[1] == TARGET and dev[0].is_cuda and dev[0].dtype == torch.float32
        assert same_bits(dev[0].cpu().numpy(), host[0])
    assert np.max(np.abs(A.load_audio_from_bytes(data)[0])) == 1.0
    for src, from_bytes in ((path, False), (data, True)):
        f_host, y_host = extract_audio_features(src, from_bytes=from_bytes)
        f_dev, y_dev = extract_audio_features(src, from_bytes=from_bytes, device_ingest=True)
        assert f_dev.dtype == np.float64 and same_bits(f_dev, f_host) and same_bits(y_dev, y_host)
    model, cfg = small_model()
    want = process_audio_features(extract_audio_features(data, from_bytes=True)[0], model, DEV, cfg)
    got = G.generate_facial_data_from_bytes(data, model, DEV, config=cfg)
    assert got.shape == (f_host.shape[0], 61) and same_bits(got, want)
    # smoothing: the reference's pairwise loop over the unsmoothed rows
    smooth = want.copy()
    for i in range(1, len(want)):
        smooth[i - 1] = (want[i - 1] + want[i]) / 2.0
    assert same_bits(G.generate_facial_data_from_bytes(data, model, DEV, use_smoothing=True, config=cfg), smooth)


def test_process_audio_features_device_at_the_chunk_edges():
    """Frame counts around the chunk plan of frame_size 32, overlap 8: one short chunk
    (reflect padded), exactly one chunk, a last chunk of one frame (25 = 24 + 1), a last
    chunk inside the overlap, several chunks."""
    from neurosync_trainer_lite_amd.utils.audio.processing import audio_processing as P
    model, cfg = small_model()
    feats = torch.randn(100, 256, generator=torch.Generator().manual_seed(3)).to(DEV)
    for n in (9, 17, 25, 32, 33, 49, 56, 57, 100):
        want = P.process_audio_features(feats[:n].double().cpu().numpy(), model, DEV, cfg)
        assert same_bits(P.process_audio_features_device(feats[:n], model, cfg), want), n


# ---------------------------------------------------------------------------
# 48 kHz and 16 kHz: two f32 evaluations of one filter
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("sr,up,down", [(48000, 147, 80), (16000, 441, 80)])
def test_resampled_input_is_within_the_bounds_of_the_host_path(sr, up, down, tmp_path):
    from neurosync_trainer_lite_amd.utils import generate_face_shapes as G
    from neurosync_trainer_lite_amd.utils.audio import load_audio as A
    from neurosync_trainer_lite_amd.utils.audio.extraction.extract_features import (extract_audio_features,
                                                                                    extract_audio_features_device)
    path, data = wav_bytes(sr, 1.0, 12, tmp_path)
    x, file_sr = A._parse_wav(data)
    assert file_sr == sr
    ref, bound = R.resample(x, up, down)
    # the raw loader: no normalisation
    host, dev = A.load_audio(path)[0], A.load_audio_device(path)[0].cpu().numpy()
    assert host.dtype == dev.dtype == np.float32 and host.shape == dev.shape == ref.shape
    assert R.worst(host, ref, bound) <= 1 and R.worst(dev, ref, bound) <= 1
    ratio = R.worst(dev, host.astype(np.float64), bound, sides=2)
    record("ingest-%d samples            worst |device - host| / (2 bound) %.4f" % (sr, ratio))
    assert ratio <= 1
    # the normalising loaders
    m = float(np.max(np.abs(host)))
    tol = (2 * bound + np.abs(host) / m * np.max(2 * bound)) / (m - np.max(2 * bound)) + 2.0 ** -23
    for h, d in ((A.load_and_preprocess_audio(path), A.load_and_preprocess_audio_device(path)),
                 (A.load_audio_from_bytes(data), A.load_audio_from_bytes_device(data))):
        assert h[1] == d[1] == TARGET
        hn, dn = h[0], d[0].cpu().numpy()
        assert np.max(np.abs(dn)) == 1.0 and dn.shape == hn.shape
        assert np.all(np.abs(dn.astype(np.float64) - hn) <= tol)
    # features: the host path's own sensitivity to the f32 evaluation, doubled
    f_host, _ = extract_audio_features(data, from_bytes=True)
    f_dev, _ = extract_audio_features(data, from_bytes=True, device_ingest=True)
    y64 = ref.astype(np.float32)
    f_ref = extract_audio_features_device(A.peak_normalise(y64), TARGET).double().cpu().numpy()
    d_host = float(np.max(np.abs(f_host - f_ref)))
    d_dev = float(np.max(np.abs(f_dev - f_host)))
    record("ingest-%d features           host scipy vs f64 restatement %.3e, device vs host %.3e (allowed %.3e)"
           % (sr, d_host, d_dev, 2 * d_host))
    assert f_dev.shape == f_host.shape and d_host > 0
    assert d_dev <= 2 * d_host
    # the serving helper runs on resampled input and returns one row per feature frame
    model, cfg = small_model()
    out = G.generate_facial_data_from_bytes(data, model, DEV, config=cfg)
    assert out.shape == (f_host.shape[0], 61) and np.isfinite(out).all()


def test_a_clip_under_nine_frames_returns_the_empty_pair(tmp_path):
    from neurosync_trainer_lite_amd.utils import generate_face_shapes as G
    from neurosync_trainer_lite_amd.utils.audio.extraction.extract_features import extract_audio_features
    model, cfg = small_model()
    for sr in (TARGET, 48000):
        _, data = wav_bytes(sr, 0.05, 13, tmp_path)       # 4410 samples at 88.2 kHz: 5 frames
        out = G.generate_facial_data_from_bytes(data, model, DEV, config=cfg)
        assert isinstance(out, tuple) and out[0] == [] and isinstance(out[1], np.ndarray) and out[1].size == 0
        assert extract_audio_features(data, from_bytes=True, device_ingest=True) == (None, None)
