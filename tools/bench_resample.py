"""Time the device resampler (nstl_resample_poly) against scipy.signal.resample_poly on
the host of the same machine: 10 s and 60 s clips at 44.1 / 48 / 16 kHz -> 88.2 kHz.

  python tools/bench_resample.py [--rounds 7] [--out profiles/resample_bench.txt]

Per clip, three arms in turn within every round (the first round is warm-up, dropped):
  host     resample_poly(x, up, down).astype(float32), the host loader's call
  kernel   the kernel alone on samples already on the device (device events, peak output on),
           repeated on the same buffers: cache-warm, the clip (5 to 33 MB in and out) stays in
           the L2 / MALL between repetitions
  h2d+k    the copy of the source samples to the device, then the kernel (host clock around
           work that ends in a device synchronise)
and the kernel's memory floor, 4 (n_in + n_out) bytes at HBM_BYTES_PER_S, as a share of
the kernel arm's time.  Medians over the kept rounds; the spread (min .. max) beside
them.  The one condition: h2d+k must not be slower than host on any clip."""
import argparse
import os
import statistics
import sys
import time
from math import gcd

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from neurosync_trainer_lite_amd import _hip as K  # noqa: E402
from neurosync_trainer_lite_amd.utils.audio.load_audio import resample_taps  # noqa: E402

TARGET = 88200
HBM_BYTES_PER_S = 8.0e12   # MI355X HBM3E peak


def clip(sr, seconds):
    rng = np.random.default_rng(sr + int(seconds))
    t = np.arange(int(sr * seconds)) / sr
    y = 0.5 * np.sin(2 * np.pi * 180 * t) * (0.6 + 0.4 * np.sin(2 * np.pi * 4 * t)) + 0.01 * rng.standard_normal(t.size)
    return y.astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--kernel-reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from scipy.signal import resample_poly
    assert torch.cuda.is_available(), "bench_resample needs a GPU"
    dev = torch.device("cuda:0")
    lines = ["# nstl_resample_poly vs scipy.signal.resample_poly, -> 88.2 kHz; ms, median (min .. max) over %d rounds"
             % (a.rounds - 1),
             "# kernel: repeated on the same buffers (cache-warm); h2d+kernel: from host memory every time",
             "# floor: 4 (n_in + n_out) bytes at %.1f TB/s, and its share of the kernel arm's time"
             % (HBM_BYTES_PER_S / 1e12)]
    slower = []
    for sr in (44100, 48000, 16000):
        for seconds in (10, 60):
            g = gcd(sr, TARGET)
            up, down = TARGET // g, sr // g
            x = clip(sr, seconds)
            n_out = K.resample_out_len(len(x), up, down)
            taps = torch.as_tensor(resample_taps(up, down)).to(dev)
            y = torch.empty(n_out, device=dev)
            pk = torch.empty(1, device=dev)
            xd = torch.as_tensor(x).to(dev)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            host, kern, both = [], [], []
            for r in range(a.rounds):
                t0 = time.perf_counter()
                want = resample_poly(x, up, down).astype(np.float32)
                host.append((time.perf_counter() - t0) * 1e3)
                torch.cuda.synchronize()
                e0.record()
                for _ in range(a.kernel_reps):
                    K.resample_poly(xd, up, down, taps, y, peak=pk)
                e1.record()
                torch.cuda.synchronize()
                kern.append(e0.elapsed_time(e1) / a.kernel_reps)
                t0 = time.perf_counter()
                xr = torch.as_tensor(x).to(dev)
                K.resample_poly(xr, up, down, taps, y, peak=pk)
                torch.cuda.synchronize()
                both.append((time.perf_counter() - t0) * 1e3)
            got = y.cpu().numpy()
            err = float(np.max(np.abs(got - want)))
            assert got.shape == want.shape and err < 1e-4, "device and host outputs differ: %g" % err

            def fig(v):
                v = v[1:]
                return "%9.3f (%8.3f .. %8.3f)" % (statistics.median(v), min(v), max(v))
            floor_ms = 4.0 * (len(x) + n_out) / HBM_BYTES_PER_S * 1e3
            k_med, h_med, b_med = (statistics.median(v[1:]) for v in (kern, host, both))
            lines.append("%6d Hz %3d s  %5d/%-4d  host %s  kernel %s  h2d+kernel %s  host/h2d+kernel %6.1fx  "
                         "floor %.4f ms = %4.1f%% of the kernel's time  max|dev-host| %.1e"
                         % (sr, seconds, up, down, fig(host), fig(kern), fig(both), h_med / b_med, floor_ms,
                            100 * floor_ms / k_med, err))
            if b_med > h_med:
                slower.append((sr, seconds))
    lines.append("# h2d+kernel slower than host on: %s" % (slower if slower else "no clip"))
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
