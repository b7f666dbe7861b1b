"""How far the device's log10f is from float64, in the unit tests/features_ref.py counts
the dB stage's rounding in: 2^-23 max(|log10 x|, 1).

dct_kernel (csrc/features.hip) forms 10.f * log10f(fmaxf(1e-10f, mel)); nothing in the
source says how many ulps log10f is good for, so it is measured: one kernel that only
calls log10f, over mel-power-like inputs (2^22 points log-spaced over 1e-10 .. 1e8, the
same number packed around 1 where the result crosses zero, and every f32 within 2^16
ulps of 1).  features_ref.ELOG_MEASURED is the figure printed here; the bound uses
twice it.

  python tools/log10f_probe.py [--lib prebuilt.so] [--keep prebuilt.so]

Without --lib the kernel is compiled with hipcc (gfx950) into a temporary directory;
--keep leaves the shared object at the given path (build once, run elsewhere)."""
import argparse
import ctypes
import os
import subprocess
import tempfile

import numpy as np

SRC = r"""
#include <hip/hip_runtime.h>
__global__ void k(const float* x, float* y, int n) {
  int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) y[i] = log10f(x[i]);
}
extern "C" int log10f_probe(const float* x, float* y, int n) {
  hipLaunchKernelGGL(k, dim3((n + 255) / 256), dim3(256), 0, 0, x, y, n);
  return (int)hipDeviceSynchronize();
}
"""


def build(path):
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "log10f_probe.hip")
        with open(src, "w") as f:
            f.write(SRC)
        hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
        subprocess.check_call([hipcc, "-O3", "-fPIC", "-shared", "--offload-arch=gfx950", src, "-o", path])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib")
    ap.add_argument("--keep")
    a = ap.parse_args()
    if a.keep:
        build(a.keep)
        print("built", a.keep)
        return
    tmp = None
    lib_path = a.lib
    if lib_path is None:
        tmp = tempfile.TemporaryDirectory()
        lib_path = os.path.join(tmp.name, "liblog10f_probe.so")
        build(lib_path)
    import torch
    lib = ctypes.CDLL(os.path.abspath(lib_path))
    lib.log10f_probe.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int]
    one = np.float32(1).view(np.int32)
    x = np.concatenate([
        np.logspace(-10, 8, 1 << 22).astype(np.float32),
        np.logspace(-0.01, 0.01, 1 << 22).astype(np.float32),
        (one + np.arange(-(1 << 16), 1 << 16, dtype=np.int32)).view(np.float32),
        np.array([1e-10, 1.0, 10.0, 0.1], np.float32)])
    xd = torch.tensor(x, device="cuda:0")
    yd = torch.full_like(xd, float("nan"))
    rc = lib.log10f_probe(xd.data_ptr(), yd.data_ptr(), x.size)
    assert rc == 0, rc
    y = yd.cpu().numpy().astype(np.float64)
    ref = np.log10(x.astype(np.float64))
    err = np.abs(y - ref)
    unit = 2.0 ** -23 * np.maximum(np.abs(ref), 1.0)
    i = int(np.argmax(err / unit))
    ulp = np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64)
    print("log10f over %d inputs: worst err %.4f units of 2^-23 max(|log10 x|, 1) at x = %.9g; "
          "worst %.3f ulps of the result" % (x.size, err[i] / unit[i], x[i], float(np.max(err / ulp))))


if __name__ == "__main__":
    main()
