"""The host-side pieces of device audio ingest that need no GPU: the config key and who
reads it, the tap cache's filter, the serving helper's smoothing, and the index form of
the reflect padding that process_audio_features_device gathers with."""
import inspect

import numpy as np
import pytest

from tests import resample_ref as R


def test_config_key_defaults_to_the_host_path():
    from neurosync_trainer_lite_amd.config import training_config
    assert training_config['device_audio_ingest'] is False
    from neurosync_trainer_lite_amd.utils.audio.extraction.extract_features import extract_audio_features
    assert inspect.signature(extract_audio_features).parameters['device_ingest'].default is False


@pytest.mark.parametrize("on", [False, True])
def test_collect_features_and_validation_honour_the_key(on, monkeypatch, tmp_path):
    from neurosync_trainer_lite_amd.dataset import data_processing
    from neurosync_trainer_lite_amd.utils import validation
    seen = []

    class Stop(Exception):
        pass

    def fake(audio_input, sr=88200, from_bytes=False, device_ingest=False):
        seen.append(device_ingest)
        raise Stop

    monkeypatch.setitem(data_processing.training_config, 'device_audio_ingest', on)
    assert validation.training_config is data_processing.training_config
    monkeypatch.setattr(data_processing, 'extract_audio_features', fake)
    monkeypatch.setattr(validation, 'extract_audio_features', fake)
    with pytest.raises(Stop):
        data_processing.collect_features("a.wav", str(tmp_path / "none.csv"), str(tmp_path / "f.csv"), 88200)
    with pytest.raises(Stop):
        validation.generate_and_save_facial_data(0, "a.wav", None, "gt.csv", None, "cpu")
    assert seen == [on, on]


@pytest.mark.parametrize("up,down", [(147, 80), (441, 80), (1, 2), (147, 320)])
def test_cached_taps_are_the_restatements_filter_rounded_once(up, down):
    from neurosync_trainer_lite_amd.utils.audio.load_audio import resample_taps
    h = resample_taps(up, down)
    assert h.dtype == np.float32 and h.shape == (R.plan(up, down)["n_taps"],)
    assert np.array_equal(h, R.taps(up, down).astype(np.float32))


def test_smoothing_is_the_references_pairwise_loop():
    from neurosync_trainer_lite_amd.utils.generate_face_shapes import smooth_by_averaging_pairs
    for n in (0, 1, 2, 7):
        d = np.random.default_rng(n).standard_normal((n, 61)).astype(np.float32)
        want = d.copy()
        for i in range(1, len(d)):
            want[i - 1] = (d[i - 1] + d[i]) / 2.0
        got = smooth_by_averaging_pairs(d)
        assert got.dtype == want.dtype and np.array_equal(got, want) and got is not d


@pytest.mark.parametrize("n", [1, 2, 3, 9, 17, 31, 32])
def test_reflect_rows_index_what_pad_audio_chunk_builds(n):
    from neurosync_trainer_lite_amd.utils.audio.processing import audio_processing as P
    x = np.random.default_rng(n).standard_normal((40 + n, 5))
    rows = P._reflect_rows(40, 40 + n, 32)
    assert rows.shape == (32,) and np.array_equal(x[rows], P.pad_audio_chunk(x[40:40 + n], 32, 5))


def test_the_device_tap_cache_keeps_the_most_recent_ratios():
    from neurosync_trainer_lite_amd.utils.audio import load_audio as A
    A._device_taps.clear()
    first = A._taps_on(2, 1, "cpu")
    for up in range(3, 3 + A.TAPS_CACHE_MAX - 1):
        A._taps_on(up, 1, "cpu")
    assert A._taps_on(2, 1, "cpu") is first and len(A._device_taps) == A.TAPS_CACHE_MAX   # a hit moves it to the back
    A._taps_on(99, 1, "cpu")
    assert len(A._device_taps) == A.TAPS_CACHE_MAX and (3, 1, "cpu") not in A._device_taps
    assert (2, 1, "cpu") in A._device_taps and (99, 1, "cpu") in A._device_taps
    A._device_taps.clear()


def test_a_rate_outside_the_kernels_range_is_refused_with_the_rule():
    """44,101 Hz -> 88,200 Hz is 88200/44101 in lowest terms: past 16384.  Refused on the
    host side of the device path, before anything touches a device."""
    from neurosync_trainer_lite_amd.utils.audio.load_audio import resample_device
    with pytest.raises(ValueError, match=r"88200/44101.*\[1, 16384\]"):
        resample_device(np.zeros(100, np.float32), 44101, 88200, device="cpu")
