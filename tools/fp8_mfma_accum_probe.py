#!/usr/bin/env python
"""How the scaled f8f6f4 MFMA adds its products: one wave, one instruction of each of
the two shapes the fp8 GEMM kernels use (v_mfma_scale_f32_32x32x64_f8f6f4: the ring
kernel; v_mfma_scale_f32_16x16x128_f8f6f4: gemm4f8), unit E8M0 block scales, chained
over K / 64 or K / 128 blocks on operands loaded straight into registers -- no LDS
staging, no epilogue, no row scales -- against the f64 product of the same e4m3 codes.

Products of two e4m3 values are exact in f32, so everything this prints is the
instruction's own accumulation.  Per shape and K: the worst |got - ref| / mag over
`--tiles` random tiles, mag = |qa| . |qb| (the magnitude tests/gemm_ref.py rounds
against), for codes quantised row-wise from N(0, 1) rows (nstl_fp8_quant_rows' scheme),
and for rows whose codes are spread log-uniformly over the whole e4m3 range.

tests/gemm_ref.py sets E8, the per-element bound of the fp8 GEMM kernels, to twice the
worst figure this shows; profiles/fp8_mfma_accum.txt is a recorded run.

  python tools/fp8_mfma_accum_probe.py [--tiles 64] [--out FILE]
The kernel is compiled once into tools/build/ (hipcc, gfx950)."""
import argparse
import ctypes
import os
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import fp8_ref  # noqa: E402

SRC = r"""
#include <hip/hip_runtime.h>
#include <stdint.h>
typedef int i32x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
#define UNIT 0x7f7f7f7f  // E8M0 127 = 2^0 in every byte

// A [32][K], B [32][K] e4m3 bytes, D [32][32] f32 = A B^T.  Lane l holds row l & 31,
// K bytes 32 (l >> 5) .. + 31 of a 64-byte block; register r of lane l is
// D[8 (r >> 2) + 4 (l >> 5) + (r & 3)][l & 31].  One block of 64 threads per tile.
__global__ __launch_bounds__(64) void probe32(const uint8_t* A, const uint8_t* B, float* D, int K) {
  const int l = threadIdx.x;
  A += (size_t)blockIdx.x * 32 * K;
  B += (size_t)blockIdx.x * 32 * K;
  D += (size_t)blockIdx.x * 32 * 32;
  f32x16 acc;
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
  for (int k0 = 0; k0 < K; k0 += 64) {
    const i32x8 a = *(const i32x8*)(A + (size_t)(l & 31) * K + k0 + 32 * (l >> 5));
    const i32x8 b = *(const i32x8*)(B + (size_t)(l & 31) * K + k0 + 32 * (l >> 5));
    acc = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a, b, acc, 0, 0, 0, UNIT, 0, UNIT);
  }
  for (int r = 0; r < 16; ++r) D[(8 * (r >> 2) + 4 * (l >> 5) + (r & 3)) * 32 + (l & 31)] = acc[r];
}

// A [16][K], B [16][K], D [16][16].  Lane l holds row l & 15, K bytes 32 (l >> 4) .. + 31
// of a 128-byte block; register r of lane l is D[4 (l >> 4) + r][l & 15].
__global__ __launch_bounds__(64) void probe16(const uint8_t* A, const uint8_t* B, float* D, int K) {
  const int l = threadIdx.x;
  A += (size_t)blockIdx.x * 16 * K;
  B += (size_t)blockIdx.x * 16 * K;
  D += (size_t)blockIdx.x * 16 * 16;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  for (int k0 = 0; k0 < K; k0 += 128) {
    const i32x8 a = *(const i32x8*)(A + (size_t)(l & 15) * K + k0 + 32 * (l >> 4));
    const i32x8 b = *(const i32x8*)(B + (size_t)(l & 15) * K + k0 + 32 * (l >> 4));
    acc = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(a, b, acc, 0, 0, 0, UNIT, 0, UNIT);
  }
  for (int r = 0; r < 4; ++r) D[(4 * (l >> 4) + r) * 16 + (l & 15)] = acc[r];
}

extern "C" int probe(int shape, const void* A, const void* B, void* D, int K, int tiles, void* stream) {
  if (shape == 32) hipLaunchKernelGGL(probe32, dim3(tiles), dim3(64), 0, (hipStream_t)stream, (const uint8_t*)A,
                                      (const uint8_t*)B, (float*)D, K);
  else hipLaunchKernelGGL(probe16, dim3(tiles), dim3(64), 0, (hipStream_t)stream, (const uint8_t*)A,
                          (const uint8_t*)B, (float*)D, K);
  return (int)hipGetLastError();
}
"""


def build():
    d = os.path.join(ROOT, "tools", "build")
    src, lib = os.path.join(d, "fp8_mfma_accum_probe.hip"), os.path.join(d, "fp8_mfma_accum_probe.so")
    os.makedirs(d, exist_ok=True)
    if not os.path.exists(src) or open(src).read() != SRC or not os.path.exists(lib):
        with open(src, "w") as f:
            f.write(SRC)
        hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
        subprocess.check_call([hipcc, "-O2", "-std=c++17", "-fPIC", "-shared", "--offload-arch=gfx950", src, "-o", lib])
    return lib


def codes(kind, rows, K, gen):
    """uint8 e4m3 codes [rows][K]: 'rows' = row-wise quantised N(0, 1) (the GEMM tests'
    operands); 'spread' = random sign, exponent field 0..15 and mantissa (no NaN code)."""
    if kind == "rows":
        q, _ = fp8_ref.quant_rows(torch.randn(rows, K, generator=gen))
        return q.view(torch.uint8)
    c = torch.randint(0, 256, (rows, K), generator=gen, dtype=torch.int32)
    c = torch.where((c & 0x7F) == 0x7F, c - 1, c)
    return c.to(torch.uint8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tiles", type=int, default=64)
    ap.add_argument("--build-only", action="store_true")
    ap.add_argument("--out")
    args = ap.parse_args()
    lib = ctypes.CDLL(build())
    if args.build_only:
        return
    lib.probe.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int,
                          ctypes.c_void_p]
    dev = "cuda:0"
    table = torch.arange(256, dtype=torch.uint8).view(torch.float8_e4m3fn).double().to(dev)
    lines = ["# tools/fp8_mfma_accum_probe.py --tiles %d: worst |got - f64| / (|qa| . |qb|) of one chained scaled MFMA" % args.tiles,
             "# per wave (no staging, no epilogue, no row scales); e4m3 products are exact in f32.",
             "# %-12s %-8s %6s %8s %12s %12s" % ("instruction", "codes", "K", "blocks", "worst", "rms")]
    worst_all = 0.0
    for shape, bk, name in ((32, 64, "32x32x64"), (16, 128, "16x16x128")):
        for kind in ("rows", "spread"):
            for K in (64, 128, 192, 256, 320, 512, 768, 1024, 4096):
                if K % bk:
                    continue
                gen = torch.Generator().manual_seed(K + shape)
                A = codes(kind, args.tiles * shape, K, gen).to(dev)
                B = codes(kind, args.tiles * shape, K, gen).to(dev)
                D = torch.full((args.tiles, shape, shape), float("nan"), device=dev)
                rc = lib.probe(shape, A.data_ptr(), B.data_ptr(), D.data_ptr(), K, args.tiles,
                               torch.cuda.current_stream().cuda_stream)
                torch.cuda.synchronize()
                assert rc == 0, rc
                a64 = table[A.long()].view(args.tiles, shape, K)
                b64 = table[B.long()].view(args.tiles, shape, K)
                ref = a64 @ b64.transpose(1, 2)
                mag = a64.abs() @ b64.abs().transpose(1, 2)
                rel = (D.double() - ref).abs() / mag.clamp_min(1e-300)
                w, rms = rel.max().item(), rel.pow(2).mean().sqrt().item()
                assert w < 1e-3, "layout error? %s %s K %d: %.3e" % (name, kind, K, w)
                if kind == "rows":
                    worst_all = max(worst_all, w)
                lines.append("%-14s %-8s %6d %8d %12.3e %12.3e" % (name, kind, K, K // bk, w, rms))
    lines.append("# worst over the row-quantised cases: %.3e" % worst_all)
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
