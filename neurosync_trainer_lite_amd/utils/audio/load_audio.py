"""Audio ingest (drop-in for utils/audio/load_audio.py:6-53).

The reference decodes with ``librosa.load(path, sr=88200)`` (mono mix, soxr
resampling) and peak-normalises.  librosa is not part of this framework: WAV
(RIFF PCM 8/16/24/32-bit, IEEE float 32/64, WAVE_FORMAT_EXTENSIBLE) is parsed
here, channels are averaged to mono (librosa's ``to_mono``), and other sample
rates are resampled with a windowed-sinc polyphase filter
(``scipy.signal.resample_poly``).  That resampler is not soxr: for 88.2 kHz input
(the reference's own capture rate, and every benchmark input) there is no
resampling and the samples are identical; for other rates parity is unpinned
(DESIGN.md).  Other containers (mov/mp4) are decoded by ffmpeg to mono 16-bit
PCM at 88.2 kHz on a pipe, the same samples as the audio.wav the reference
first writes with ffmpeg (utils/video/mov_extraction.py:39-62).

The ``*_device`` forms do the same parse and mono mix on the host, copy the samples
to the GPU at the source rate, and resample (``nstl_resample_poly``: the same filter
as ``scipy.signal.resample_poly``, evaluated in f32 on the device) and peak-normalise
(``nstl_peak_normalise``) there; they return device tensors.  The host forms stay the
default everywhere.
"""
import io
import os
import struct
import subprocess
from collections import OrderedDict
from math import gcd

import numpy as np

TARGET_SR = 88200

_PCM, _FLOAT, _EXTENSIBLE = 1, 3, 0xFFFE


def _parse_wav(buf):
    if len(buf) < 12 or buf[0:4] != b"RIFF" or buf[8:12] != b"WAVE":
        raise ValueError("not a RIFF/WAVE file")
    pos, fmt, data = 12, None, None
    while pos + 8 <= len(buf):
        cid, size = buf[pos:pos + 4], struct.unpack_from("<I", buf, pos + 4)[0]
        body = buf[pos + 8: pos + 8 + size]
        if cid == b"fmt ":
            tag, ch, sr, _, _, bits = struct.unpack_from("<HHIIHH", body, 0)
            if tag == _EXTENSIBLE and len(body) >= 26:
                tag = struct.unpack_from("<H", body, 24)[0]
            fmt = (tag, ch, sr, bits)
        elif cid == b"data":
            data = body
        pos += 8 + size + (size & 1)
    if fmt is None or data is None:
        raise ValueError("WAV without fmt/data chunk")
    tag, ch, sr, bits = fmt
    if tag == _PCM:
        if bits == 8:
            x = (np.frombuffer(data, np.uint8).astype(np.float32) - 128.0) / 128.0
        elif bits == 16:
            x = np.frombuffer(data, "<i2").astype(np.float32) / 32768.0
        elif bits == 24:
            b = np.frombuffer(data[: len(data) // 3 * 3], np.uint8).reshape(-1, 3).astype(np.int32)
            v = b[:, 0] | (b[:, 1] << 8) | (b[:, 2] << 16)
            v = np.where(v >= 1 << 23, v - (1 << 24), v)
            x = v.astype(np.float32) / float(1 << 23)
        elif bits == 32:
            x = (np.frombuffer(data, "<i4").astype(np.float64) / 2147483648.0).astype(np.float32)
        else:
            raise ValueError("unsupported PCM width %d" % bits)
    elif tag == _FLOAT:
        x = np.frombuffer(data, "<f4" if bits == 32 else "<f8").astype(np.float32)
    else:
        raise ValueError("unsupported WAV format tag %d" % tag)
    x = x[: len(x) // ch * ch].reshape(-1, ch)
    return (x.mean(axis=1) if ch > 1 else x[:, 0]).astype(np.float32), sr


def resample(y, orig_sr, target_sr):
    if orig_sr == target_sr:
        return y
    from scipy.signal import resample_poly
    g = gcd(int(orig_sr), int(target_sr))
    return resample_poly(y, target_sr // g, orig_sr // g).astype(np.float32)


def peak_normalise(y):
    """y / max|y| when non-zero (load_audio.py:13-15)."""
    m = np.max(np.abs(y)) if y.size else 0.0
    return y / m if m > 0 else y


def resample_taps(up, down):
    """The f32 prototype filter of ``resample_poly(x, up, down)`` at its defaults:
    firwin(20 max(up, down) + 1, 1 / max(up, down), window=('kaiser', 5.0)) * up, built
    in f64 and rounded once (include/nstl.h: nstl_resample_args.taps)."""
    from scipy.signal import firwin
    max_rate = max(up, down)
    return (firwin(20 * max_rate + 1, 1.0 / max_rate, window=('kaiser', 5.0)) * up).astype(np.float32)


# (up, down, device) -> f32 taps on that device, least recently used first.  A filter is
# up to 20 * 16384 + 1 floats (1.3 MB), and a server sees whatever rates its callers send:
# the cache keeps the TAPS_CACHE_MAX most recent and lets the rest go.
TAPS_CACHE_MAX = 8
_device_taps = OrderedDict()


def _taps_on(up, down, device):
    import torch
    key = (up, down, str(device))
    taps = _device_taps.pop(key, None)
    if taps is None:
        taps = torch.as_tensor(resample_taps(up, down)).to(device)
    _device_taps[key] = taps
    while len(_device_taps) > TAPS_CACHE_MAX:
        _device_taps.popitem(last=False)
    return taps


def _device_of(device):
    import torch
    if device is None:
        return torch.device("cuda", torch.cuda.current_device())
    device = torch.device(device)
    return torch.device("cuda", torch.cuda.current_device()) if device.type == "cuda" and device.index is None else device


def _to_device(y, device):
    import torch
    if not torch.is_tensor(y):
        y = torch.as_tensor(np.ascontiguousarray(y, dtype=np.float32))
    return y.to(device=device, dtype=torch.float32).contiguous()


def resample_device(y, orig_sr, target_sr, device=None, stream=None, peak=False):
    """``resample`` on the GPU: y (numpy or tensor, 1-D) at orig_sr -> f32 device tensor at
    target_sr.  peak=True: returns (samples, f32 [1] device tensor holding max |samples|),
    the peak coming out of the resampling kernel itself."""
    import torch

    from ... import _hip as K
    device = _device_of(device)
    yt = _to_device(y, device)
    if int(orig_sr) == int(target_sr) or yt.numel() == 0:
        if not peak:
            return yt
        return yt, (yt.abs().max().reshape(1) if yt.numel() else torch.zeros(1, device=device))
    g = gcd(int(orig_sr), int(target_sr))
    up, down = int(target_sr) // g, int(orig_sr) // g
    n_out = K.resample_out_len(yt.numel(), up, down)
    if n_out <= 0:
        raise ValueError("resample_device: %d Hz -> %d Hz reduces to %d/%d; nstl_resample_poly takes up and "
                         "down in [1, 16384] (and samples x up < 2^62).  The host loaders (scipy) resample "
                         "such a rate." % (orig_sr, target_sr, up, down))
    with torch.cuda.device(device):
        out = torch.empty(n_out, dtype=torch.float32, device=device)
        pk = torch.empty(1, dtype=torch.float32, device=device) if peak else None
        K.resample_poly(yt, up, down, _taps_on(up, down, device), out, peak=pk, stream=stream)
    return (out, pk) if peak else out


def peak_normalise_device(y, peak=None, stream=None):
    """``peak_normalise`` in place on the device tensor y; peak: f32 [1] on the same
    device (max |y|; computed when not given)."""
    import torch

    from ... import _hip as K
    if y.numel() == 0:
        return y
    if peak is None:
        peak = y.abs().max().reshape(1)
    with torch.cuda.device(y.device):
        K.peak_normalise(y, peak, stream=stream)
    return y


def _host_peak(y, device):
    """max |y| of host samples as the f32 [1] device tensor nstl_peak_normalise reads."""
    import torch
    m = np.float32(np.max(np.abs(y))) if y.size else np.float32(0)
    return torch.as_tensor(np.array([m], np.float32)).to(device)


def _ingest_device(y, file_sr, rates, device, stream, normalise):
    """Host samples at file_sr -> device tensor after resampling to each of `rates` in turn
    (None / equal rates: no resampling), then peak-normalised when `normalise`."""
    device = _device_of(device)
    pk = None
    if normalise and all(r is None or int(r) == int(file_sr) for r in rates):
        pk = _host_peak(y, device)      # nothing resamples: the peak of the parsed samples
    yt, sr = _to_device(y, device), file_sr
    for r in rates:
        if r is not None and int(r) != int(sr):
            yt, pk = resample_device(yt, sr, r, device, stream, peak=True)
            sr = r
    if normalise:
        peak_normalise_device(yt, pk, stream)
    return yt, sr


def _read_file(audio_path, sr):
    if os.path.splitext(audio_path)[1].lower() in ('.mov', '.mp4'):
        return _decode_container(audio_path, sr)
    with open(audio_path, "rb") as f:
        return _parse_wav(f.read())


def load_audio_device(audio_path, sr=TARGET_SR, device=None, stream=None):
    """``load_audio`` with the resampling on the GPU -> (device tensor, sr)."""
    y, file_sr = _read_file(audio_path, sr)
    yt, file_sr = _ingest_device(y, file_sr, [sr], device, stream, normalise=False)
    print(f"Loaded audio file '{audio_path}' with sample rate {file_sr}")
    return yt, file_sr


def load_and_preprocess_audio_device(audio_path, sr=TARGET_SR, device=None, stream=None):
    """``load_and_preprocess_audio`` with resampling and peak normalisation on the GPU."""
    y, file_sr = _read_file(audio_path, sr)
    yt, out_sr = _ingest_device(y, file_sr, [sr, TARGET_SR], device, stream, normalise=True)
    print(f"Loaded audio file '{audio_path}' with sample rate {sr if sr is not None else file_sr}")
    return yt, out_sr


def load_audio_from_bytes_device(audio_bytes, sr=TARGET_SR, device=None, stream=None):
    """``load_audio_from_bytes`` with resampling and peak normalisation on the GPU."""
    y, file_sr = _parse_wav(io.BytesIO(audio_bytes).getvalue())
    return _ingest_device(y, file_sr, [sr], device, stream, normalise=True)


def _decode_container(path, sr):
    """Any container ffmpeg reads -> mono samples at ``sr`` (ffmpeg resamples).
    Decoded as 16-bit PCM and scaled by 1/32768, the samples the reference's
    audio.wav round trip gives (ffmpeg's default WAV codec is pcm_s16le,
    utils/video/mov_extraction.py:39-62, read back by librosa)."""
    from ...config import training_config
    sr = sr or TARGET_SR
    cmd = [training_config['ffmpeg_path'], '-v', 'error', '-i', path, '-vn', '-ac', '1', '-ar', str(sr),
           '-f', 's16le', '-acodec', 'pcm_s16le', '-']
    pcm = subprocess.run(cmd, check=True, stdout=subprocess.PIPE).stdout
    return np.frombuffer(pcm, '<i2').astype(np.float32) / 32768.0, sr


def load_audio(audio_path, sr=TARGET_SR):
    """load_audio.py:18-21: decode, mono, resample to ``sr``."""
    if os.path.splitext(audio_path)[1].lower() in ('.mov', '.mp4'):
        y, file_sr = _decode_container(audio_path, sr)
    else:
        with open(audio_path, "rb") as f:
            y, file_sr = _parse_wav(f.read())
    if sr is not None:
        y, file_sr = resample(y, file_sr, sr), sr
    print(f"Loaded audio file '{audio_path}' with sample rate {file_sr}")
    return y, file_sr


def load_and_preprocess_audio(audio_path, sr=TARGET_SR):
    """load_audio.py:6-16."""
    y, sr = load_audio(audio_path, sr)
    if sr != TARGET_SR:
        y, sr = resample(y, sr, TARGET_SR), TARGET_SR
    return peak_normalise(y), sr


def load_audio_from_bytes(audio_bytes, sr=TARGET_SR):
    """load_audio.py:23-33."""
    y, file_sr = _parse_wav(io.BytesIO(audio_bytes).getvalue())
    if sr is not None:
        y, file_sr = resample(y, file_sr, sr), sr
    return peak_normalise(y), file_sr


def load_audio_file_from_memory(audio_bytes, sr=TARGET_SR):
    """load_audio.py:35-45."""
    y, sr = load_audio_from_bytes(audio_bytes, sr)
    print(f"Loaded audio data with sample rate {sr}")
    return y, sr


def write_wav(path, y, sr, bits=16):
    """16-bit (or 32-bit float) mono WAV writer (test corpora, save_audio)."""
    y = np.asarray(y)
    if bits == 16:
        payload = (np.clip(y, -1.0, 32767 / 32768) * 32768.0).round().astype("<i2").tobytes()
        tag, width = _PCM, 2
    else:
        payload = y.astype("<f4").tobytes()
        tag, width = _FLOAT, 4
    hdr = struct.pack("<4sI4s4sIHHIIHH4sI", b"RIFF", 36 + len(payload), b"WAVE", b"fmt ", 16, tag, 1, sr,
                      sr * width, width, 8 * width, b"data", len(payload))
    with open(path, "wb") as f:
        f.write(hdr + payload)
