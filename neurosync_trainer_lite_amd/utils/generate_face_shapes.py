"""Drop-in for utils/generate_face_shapes.py:1-26 (the serving entry point: audio bytes
-> blendshape frames).

The reference's own call of ``process_audio_features`` omits the config that function
requires (generate_face_shapes.py:15), so its helper cannot run as written; here the
config is one more keyword, ``config=None`` (-> ``training_config``).  This function is
new surface of this package, so the audio takes the device path by default: the bytes
are parsed on the host, resampled and peak-normalised on the GPU
(``load_audio_from_bytes_device``), turned into features there (``nstl_features``),
chunked and decoded there (``process_audio_features_device``); only the decoded chunks
come back to the host.
"""
import numpy as np

from ..config import training_config
from .audio.extraction.extract_features import audio_features_from_device_ingest
from .audio.processing.audio_processing import process_audio_features_device


def generate_facial_data_from_bytes(audio_bytes, model, device, use_smoothing=False, config=None):
    """generate_face_shapes.py:8-20: ([], np.array([])) for a clip under 9 frames."""
    config = training_config if config is None else config
    audio_features, y = audio_features_from_device_ingest(audio_bytes, from_bytes=True, device=device)
    if audio_features is None or y is None:
        return [], np.array([])
    final_decoded_outputs = process_audio_features_device(audio_features, model, config)
    if use_smoothing:
        final_decoded_outputs = smooth_by_averaging_pairs(final_decoded_outputs)
    return final_decoded_outputs


def smooth_by_averaging_pairs(data):
    """generate_face_shapes.py:22-26: row i-1 becomes the mean of rows i-1 and i of the
    input (the last row stays), as the reference's loop over the original rows does."""
    smoothed_data = data.copy()
    if len(data) > 1:
        smoothed_data[:-1] = (data[:-1] + data[1:]) / 2.0
    return smoothed_data
