#include <stdlib.h>
// Post-LN residual tails of the NeuroSync Seq2Seq layers (utils/model.py:175-180,
// :198-207, final norms :228-229/:249-250):
//   forward : s = x + y * m1 * m2 / (1-p)^n ; out = (s - mean) * rstd * gamma + beta
//             (+ optional global-PE rotation of `out`, model.py:246)
//   backward: ds = rstd * (g*gamma - mean(g*gamma) - xhat * mean(g*gamma*xhat));
//             dbranch = ds * masks / (1-p)^n ; per-block dgamma/dbeta partials.
// D = 128 / 256 / 512 / 768 / 1024 (and the forward at every D % 256 == 0): one
// wave per row; each lane owns VPL = D/64 columns: contiguous (D = 128), or when
// D % 256 == 0 four- or eight-column groups 256 / 512 apart (every wave
// instruction then covers one contiguous span).  Every other multiple of 128 up to
// 2048: the row-cooperative kernels (a row split over the waves of a workgroup).
#include <algorithm>

#include "../../include/nstl.h"
#include "common.h"
#include "status.h"

namespace {

constexpr int NT = 256;

template <typename T, int VPL>
NSTL_DEV void load_row(const T* p, float (&v)[VPL]) {
  if constexpr ((VPL * sizeof(T)) % 16 == 0) {
    constexpr int NV = VPL * sizeof(T) / 16;
    constexpr int EPV = 16 / sizeof(T);
#pragma unroll
    for (int k = 0; k < NV; ++k) {
      const uint4 u = ((const uint4*)p)[k];
      const T* e = (const T*)&u;
#pragma unroll
      for (int j = 0; j < EPV; ++j) v[k * EPV + j] = to_f32(e[j]);
    }
  } else {
#pragma unroll
    for (int j = 0; j < VPL; ++j) v[j] = to_f32(p[j]);
  }
}

template <typename T, int VPL>
NSTL_DEV void store_row(T* p, const float (&v)[VPL]) {
  if constexpr ((VPL * sizeof(T)) % 16 == 0) {
    constexpr int NV = VPL * sizeof(T) / 16;
    constexpr int EPV = 16 / sizeof(T);
#pragma unroll
    for (int k = 0; k < NV; ++k) {
      uint4 u;
      T* e = (T*)&u;
#pragma unroll
      for (int j = 0; j < EPV; ++j) e[j] = from_f32<T>(v[k * EPV + j]);
      ((uint4*)p)[k] = u;
    }
  } else {
#pragma unroll
    for (int j = 0; j < VPL; ++j) p[j] = from_f32<T>(v[j]);
  }
}

struct LnParams {
  const char* x; const char* y;
  int rows, D;
  int n_masks; uint32_t thresh; float inv_keep; uint64_t seed1, seed2;
  const float* gamma; const float* beta; float eps;
  char* s_out; char* out; float* mean; float* rstd;
  char* rot_out; const float* rope_cos; const float* rope_sin; int rope_T;
  const char* s_in; const float* dout; float* ds; char* dbranch;
  const char* dout2;  // optional dtype addend of dout
  float* dgp; float* dbp; float* dyp;
  uint8_t* q8; int64_t ldq8; float* q8_scale;  // forward: row-wise e4m3 copy of out (fp8.hip rule)
};

// dropout scale of the element pair (idx, idx+1), idx even: 1 or 2 stacked masks
// (32-bit pair index idx / 2: the launcher checks rows * D <= 2^33)
NSTL_DEV void branch_scale2(const LnParams& p, uint64_t idx, float& m0, float& m1) {
  bool a0, a1, b0 = true, b1 = true;
  const uint32_t pair = (uint32_t)(idx >> 1);
  nstl_keep2_32(nstl_seed_term(p.seed1), pair, p.thresh, a0, a1);
  if (p.n_masks >= 2) nstl_keep2_32(nstl_seed_term(p.seed2), pair, p.thresh, b0, b1);
  const float s = p.n_masks >= 2 ? p.inv_keep * p.inv_keep : p.inv_keep;
  m0 = (a0 && b0) ? s : 0.f;
  m1 = (a1 && b1) ? s : 0.f;
}

template <typename T, int VPL>
__global__ __launch_bounds__(NT) void ln_fwd_kernel(LnParams p) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * (NT / 64) + (threadIdx.x >> 6);
  if (row >= p.rows) return;
  const int c0 = lane * VPL;
  const int64_t base = (int64_t)row * p.D + c0;
  float s[VPL];
  load_row<T, VPL>((const T*)p.y + base, s);
  if (p.thresh && p.n_masks > 0) {
#pragma unroll
    for (int j = 0; j < VPL; j += 2) {
      float m0, m1;
      branch_scale2(p, (uint64_t)base + j, m0, m1);
      s[j] *= m0;
      s[j + 1] *= m1;
    }
  }
  if (p.x) {
    float xv[VPL];
    load_row<T, VPL>((const T*)p.x + base, xv);
#pragma unroll
    for (int j = 0; j < VPL; ++j) s[j] += xv[j];
  }
  float sum = 0.f;
#pragma unroll
  for (int j = 0; j < VPL; ++j) sum += s[j];
  const float mean = wave_sum(sum) / p.D;
  float sq = 0.f;
#pragma unroll
  for (int j = 0; j < VPL; ++j) {
    const float d = s[j] - mean;
    sq += d * d;
  }
  const float rstd = rsqrtf(wave_sum(sq) / p.D + p.eps);
  if (p.s_out) store_row<T, VPL>((T*)p.s_out + base, s);
  float o[VPL];
#pragma unroll
  for (int j = 0; j < VPL; ++j) o[j] = (s[j] - mean) * rstd * p.gamma[c0 + j] + p.beta[c0 + j];
  // round to the storage type first so `rot_out` rotates exactly what `out` holds
#pragma unroll
  for (int j = 0; j < VPL; ++j) o[j] = to_f32(from_f32<T>(o[j]));
  store_row<T, VPL>((T*)p.out + base, o);
  if (lane == 0) {
    p.mean[row] = mean;
    p.rstd[row] = rstd;
  }
  if (p.rot_out) {
    const int t = row % p.rope_T, half = p.D >> 1;
    float r[VPL];
#pragma unroll
    for (int j = 0; j < VPL; j += 2) {
      const int pr = (c0 + j) >> 1;
      const float c = p.rope_cos[t * half + pr], sn = p.rope_sin[t * half + pr];
      r[j] = o[j] * c - o[j + 1] * sn;
      r[j + 1] = o[j] * sn + o[j + 1] * c;
    }
    store_row<T, VPL>((T*)p.rot_out + base, r);
  }
}

template <typename T, int VPL>
__global__ __launch_bounds__(NT) void ln_bwd_kernel(LnParams p) {
  const int lane = threadIdx.x & 63;
  const int c0 = lane * VPL;
  float gam[VPL], dg[VPL], db[VPL], dyb[VPL];
#pragma unroll
  for (int j = 0; j < VPL; ++j) {
    gam[j] = p.gamma[c0 + j];
    dg[j] = 0.f;
    db[j] = 0.f;
    dyb[j] = 0.f;
  }
  for (int row = blockIdx.x * (NT / 64) + (threadIdx.x >> 6); row < p.rows; row += gridDim.x * (NT / 64)) {
    const int64_t base = (int64_t)row * p.D + c0;
    const float mean = p.mean[row], rstd = p.rstd[row];
    float xh[VPL], gy[VPL];
    load_row<T, VPL>((const T*)p.s_in + base, xh);
    load_row<float, VPL>(p.dout + base, gy);
    if (p.dout2) {
      float g2[VPL];
      load_row<T, VPL>((const T*)p.dout2 + base, g2);
#pragma unroll
      for (int j = 0; j < VPL; ++j) gy[j] += g2[j];
    }
    float a1 = 0.f, a2 = 0.f;
#pragma unroll
    for (int j = 0; j < VPL; ++j) {
      xh[j] = (xh[j] - mean) * rstd;
      dg[j] += gy[j] * xh[j];
      db[j] += gy[j];
      const float gg = gy[j] * gam[j];
      a1 += gg;
      a2 += gg * xh[j];
    }
    const float m1 = wave_sum(a1) / p.D, m2 = wave_sum(a2) / p.D;
    float d[VPL];
#pragma unroll
    for (int j = 0; j < VPL; ++j) d[j] = rstd * (gy[j] * gam[j] - m1 - xh[j] * m2);
    store_row<float, VPL>(p.ds + base, d);
    if (p.dbranch) {
      if (p.thresh && p.n_masks > 0) {
#pragma unroll
        for (int j = 0; j < VPL; j += 2) {
          float m0, m1;
          branch_scale2(p, (uint64_t)base + j, m0, m1);
          d[j] *= m0;
          d[j + 1] *= m1;
        }
      }
#pragma unroll
      for (int j = 0; j < VPL; ++j) d[j] = to_f32(from_f32<T>(d[j]));  // sum what is stored
      store_row<T, VPL>((T*)p.dbranch + base, d);
#pragma unroll
      for (int j = 0; j < VPL; ++j) dyb[j] += d[j];
    }
  }
  // per-block partials: reduce the 4 waves through LDS
  __shared__ float red[3][NT / 64][1024];
  const int w = threadIdx.x >> 6;
#pragma unroll
  for (int j = 0; j < VPL; ++j) {
    red[0][w][c0 + j] = dg[j];
    red[1][w][c0 + j] = db[j];
    red[2][w][c0 + j] = dyb[j];
  }
  __syncthreads();
  for (int c = threadIdx.x; c < p.D; c += NT) {
    float a = 0.f, b = 0.f, y = 0.f;
#pragma unroll
    for (int k = 0; k < NT / 64; ++k) {
      a += red[0][k][c];
      b += red[1][k][c];
      y += red[2][k][c];
    }
    p.dgp[(int64_t)blockIdx.x * p.D + c] = a;
    p.dbp[(int64_t)blockIdx.x * p.D + c] = b;
    if (p.dyp) p.dyp[(int64_t)blockIdx.x * p.D + c] = y;
  }
}

// Backward for D % 256 == 0 (the step's D = 1024): 8 waves per block, lane l
// owns columns k*256 + 4l .. +3 (k < D/256), so every load/store instruction of
// a wave covers one contiguous 512 B (bf16) / 1 KB (f32) span, and the next
// row's inputs are loaded before the current row is reduced (two rows in flight
// per wave: ~100 KB per CU, what HBM latency needs).
constexpr int NTB = 512;

template <typename T>
NSTL_DEV void load4(const T* p, float (&v)[4]) {
  if constexpr (sizeof(T) == 2) {
    const uint2 u = *(const uint2*)p;
    const T* e = (const T*)&u;
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = to_f32(e[j]);
  } else {
    const float4 u = *(const float4*)p;
    v[0] = u.x; v[1] = u.y; v[2] = u.z; v[3] = u.w;
  }
}
// G consecutive columns of a row (G = 8: one 16-byte bf16 access, two for f32)
template <typename T, int G>
NSTL_DEV void loadG(const T* p, float (&v)[G]) {
  if constexpr (G == 4) {
    load4<T>(p, v);
  } else if constexpr (sizeof(T) == 2) {
    const uint4 u = *(const uint4*)p;
    const T* e = (const T*)&u;
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = to_f32(e[j]);
  } else {
    const float4 a = *(const float4*)p, b = *(const float4*)(p + 4);
    v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
  }
}
template <typename T>
NSTL_DEV void store4(T* p, const float* v);
template <typename T, int G>
NSTL_DEV void storeG(T* p, const float* v) {
  if constexpr (G == 4) {
    store4<T>(p, v);
  } else if constexpr (sizeof(T) == 2) {
    uint4 u;
    T* e = (T*)&u;
#pragma unroll
    for (int j = 0; j < 8; ++j) e[j] = from_f32<T>(v[j]);
    *(uint4*)p = u;
  } else {
    *(float4*)p = make_float4(v[0], v[1], v[2], v[3]);
    *(float4*)(p + 4) = make_float4(v[4], v[5], v[6], v[7]);
  }
}

template <typename T>
NSTL_DEV void store4(T* p, const float* v) {
  if constexpr (sizeof(T) == 2) {
    uint2 u;
    T* e = (T*)&u;
#pragma unroll
    for (int j = 0; j < 4; ++j) e[j] = from_f32<T>(v[j]);
    *(uint2*)p = u;
  } else {
    *(float4*)p = make_float4(v[0], v[1], v[2], v[3]);
  }
}

// The row-wise e4m3 copy of a stored row v (already rounded to the storage type),
// the same arithmetic as nstl_fp8_quant_rows: the forward's LN output (the next fp8
// projection's operand) or, in the backward, dbranch (the fp8 input-gradient GEMM's
// A operand).  Interleaved column map: lane l owns columns k*64G + G*l .. +G-1.
template <int VPL, int G>
NSTL_DEV void q8_row(const LnParams& p, int row, int lane, const float (&v)[VPL]) {
  constexpr int NK = VPL / G, SPAN = 64 * G;
  float am = 0.f;
#pragma unroll
  for (int j = 0; j < VPL; ++j) am = fmaxf(am, fabsf(v[j]));
  am = wave_max(am);
  const float inv = am > 0.f ? 448.f / am : 1.f;
  if (lane == 0) p.q8_scale[row] = am > 0.f ? am / 448.f : 1.f;
#pragma unroll
  for (int k = 0; k < NK; ++k) {
    float x[G];
#pragma unroll
    for (int e = 0; e < G; ++e) x[e] = fminf(fmaxf(v[G * k + e] * inv, -448.f), 448.f);
    uint32_t b[G / 4];
#pragma unroll
    for (int h = 0; h < G / 4; ++h)
      b[h] = ((uint32_t)__builtin_amdgcn_cvt_pk_fp8_f32(x[4 * h], x[4 * h + 1], 0, false) & 0xffffu) |
             (((uint32_t)__builtin_amdgcn_cvt_pk_fp8_f32(x[4 * h + 2], x[4 * h + 3], 0, false) & 0xffffu) << 16);
    uint8_t* q = p.q8 + (int64_t)row * p.ldq8 + k * SPAN + G * lane;
    if constexpr (G == 8) *(uint2*)q = make_uint2(b[0], b[1]);
    else *(uint32_t*)q = b[0];
  }
}

template <typename T, int VPL, int G>
__global__ __launch_bounds__(NTB) void ln_bwd_kernel_il(LnParams p) {
  constexpr int NK = VPL / G;  // G-column groups per lane
  constexpr int SPAN = 64 * G;
  constexpr int NWB = NTB / 64;
  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  float gam[VPL], dg[VPL], db[VPL], dyb[VPL];
#pragma unroll
  for (int k = 0; k < NK; ++k)
#pragma unroll
    for (int e = 0; e < G; ++e) {
      gam[G * k + e] = p.gamma[k * SPAN + G * lane + e];
      dg[G * k + e] = db[G * k + e] = dyb[G * k + e] = 0.f;
    }
  const int stride = gridDim.x * NWB;
  int row = blockIdx.x * NWB + w;
  float xh[VPL], gy[VPL], mean = 0.f, rstd = 0.f;
  auto load = [&](int r, float (&x)[VPL], float (&g)[VPL], float& mu, float& rs) {
    const int64_t base = (int64_t)r * p.D + G * lane;
#pragma unroll
    for (int k = 0; k < NK; ++k) {
      float t4[G], g4[G], a4[G];
#pragma unroll
      for (int e = 0; e < G; ++e) a4[e] = 0.f;
      loadG<T, G>((const T*)p.s_in + base + k * SPAN, t4);
      loadG<float, G>(p.dout + base + k * SPAN, g4);
      if (p.dout2) loadG<T, G>((const T*)p.dout2 + base + k * SPAN, a4);
#pragma unroll
      for (int e = 0; e < G; ++e) {
        x[G * k + e] = t4[e];
        g[G * k + e] = g4[e] + a4[e];
      }
    }
    mu = p.mean[r];
    rs = p.rstd[r];
  };
  if (row < p.rows) load(row, xh, gy, mean, rstd);
  for (; row < p.rows; row += stride) {
    const int nxt = row + stride;
    float xn[VPL], gn[VPL], mn = 0.f, rn = 0.f;
    if (nxt < p.rows) load(nxt, xn, gn, mn, rn);
    const int64_t base = (int64_t)row * p.D + G * lane;
    float a1 = 0.f, a2 = 0.f;
#pragma unroll
    for (int j = 0; j < VPL; ++j) {
      xh[j] = (xh[j] - mean) * rstd;
      dg[j] += gy[j] * xh[j];
      db[j] += gy[j];
      const float gg = gy[j] * gam[j];
      a1 += gg;
      a2 += gg * xh[j];
    }
    const float m1 = wave_sum(a1) / p.D, m2 = wave_sum(a2) / p.D;
    float d[VPL];
#pragma unroll
    for (int j = 0; j < VPL; ++j) d[j] = rstd * (gy[j] * gam[j] - m1 - xh[j] * m2);
#pragma unroll
    for (int k = 0; k < NK; ++k) storeG<float, G>(p.ds + base + k * SPAN, d + G * k);
    if (p.dbranch) {
      if (p.thresh && p.n_masks > 0) {
#pragma unroll
        for (int k = 0; k < NK; ++k)
#pragma unroll
          for (int e = 0; e < G; e += 2) {
            float s0, s1;
            branch_scale2(p, (uint64_t)base + k * SPAN + e, s0, s1);
            d[G * k + e] *= s0;
            d[G * k + e + 1] *= s1;
          }
      }
#pragma unroll
      for (int j = 0; j < VPL; ++j) d[j] = to_f32(from_f32<T>(d[j]));  // sum what is stored
#pragma unroll
      for (int k = 0; k < NK; ++k) storeG<T, G>((T*)p.dbranch + base + k * SPAN, d + G * k);
#pragma unroll
      for (int j = 0; j < VPL; ++j) dyb[j] += d[j];
      if (p.q8) q8_row<VPL, G>(p, row, lane, d);  // fp8 backward: the e4m3 copy of dbranch
    }
#pragma unroll
    for (int j = 0; j < VPL; ++j) {
      xh[j] = xn[j];
      gy[j] = gn[j];
    }
    mean = mn;
    rstd = rn;
  }
  // per-block partials: reduce the waves through LDS, column order
  __shared__ float red[3][NWB][1024];
#pragma unroll
  for (int k = 0; k < NK; ++k)
#pragma unroll
    for (int e = 0; e < G; ++e) {
      const int c = k * SPAN + G * lane + e;
      red[0][w][c] = dg[G * k + e];
      red[1][w][c] = db[G * k + e];
      red[2][w][c] = dyb[G * k + e];
    }
  __syncthreads();
  for (int c = threadIdx.x; c < p.D; c += NTB) {
    float a = 0.f, b = 0.f, y = 0.f;
#pragma unroll
    for (int k = 0; k < NWB; ++k) {
      a += red[0][k][c];
      b += red[1][k][c];
      y += red[2][k][c];
    }
    p.dgp[(int64_t)blockIdx.x * p.D + c] = a;
    p.dbp[(int64_t)blockIdx.x * p.D + c] = b;
    if (p.dyp) p.dyp[(int64_t)blockIdx.x * p.D + c] = y;
  }
}

// Forward with the interleaved column map of ln_bwd_kernel_il (D % 256 == 0):
// lane l owns columns k*256 + 4l .. +3, one row per wave.
template <typename T, int VPL, int G>
__global__ __launch_bounds__(NT) void ln_fwd_kernel_il(LnParams p) {
  constexpr int NK = VPL / G;
  constexpr int SPAN = 64 * G;
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * (NT / 64) + (threadIdx.x >> 6);
  if (row >= p.rows) return;
  const int64_t base = (int64_t)row * p.D + G * lane;
  float s[VPL], xv[VPL];
#pragma unroll
  for (int k = 0; k < NK; ++k) {
    float y4[G], x4[G];
#pragma unroll
    for (int e = 0; e < G; ++e) x4[e] = 0.f;
    loadG<T, G>((const T*)p.y + base + k * SPAN, y4);
    if (p.x) loadG<T, G>((const T*)p.x + base + k * SPAN, x4);
#pragma unroll
    for (int e = 0; e < G; ++e) {
      s[G * k + e] = y4[e];
      xv[G * k + e] = x4[e];
    }
  }
  if (p.thresh && p.n_masks > 0) {
#pragma unroll
    for (int k = 0; k < NK; ++k)
#pragma unroll
      for (int e = 0; e < G; e += 2) {
        float m0, m1;
        branch_scale2(p, (uint64_t)base + k * SPAN + e, m0, m1);
        s[G * k + e] *= m0;
        s[G * k + e + 1] *= m1;
      }
  }
  float sum = 0.f;
#pragma unroll
  for (int j = 0; j < VPL; ++j) {
    s[j] += xv[j];
    sum += s[j];
  }
  const float mean = wave_sum(sum) / p.D;
  float sq = 0.f;
#pragma unroll
  for (int j = 0; j < VPL; ++j) {
    const float d = s[j] - mean;
    sq += d * d;
  }
  const float rstd = rsqrtf(wave_sum(sq) / p.D + p.eps);
  float o[VPL];
#pragma unroll
  for (int k = 0; k < NK; ++k) {
    if (p.s_out) storeG<T, G>((T*)p.s_out + base + k * SPAN, s + G * k);
#pragma unroll
    for (int e = 0; e < G; ++e) {
      const int c = k * SPAN + G * lane + e;
      // round to the storage type first so `rot_out` rotates exactly what `out` holds
      o[G * k + e] = to_f32(from_f32<T>((s[G * k + e] - mean) * rstd * p.gamma[c] + p.beta[c]));
    }
    storeG<T, G>((T*)p.out + base + k * SPAN, o + G * k);
  }
  if (lane == 0) {
    p.mean[row] = mean;
    p.rstd[row] = rstd;
  }
  if (p.q8) q8_row<VPL, G>(p, row, lane, o);
  if (p.rot_out) {
    const int t = row % p.rope_T, half = p.D >> 1;
#pragma unroll
    for (int k = 0; k < NK; ++k) {
      float r[G];
#pragma unroll
      for (int e = 0; e < G; e += 2) {
        const int pr = (k * SPAN + G * lane + e) >> 1;
        const float c = p.rope_cos[t * half + pr], sn = p.rope_sin[t * half + pr];
        r[e] = o[G * k + e] * c - o[G * k + e + 1] * sn;
        r[e + 1] = o[G * k + e] * sn + o[G * k + e + 1] * c;
      }
      storeG<T, G>((T*)p.rot_out + base + k * SPAN, r);
    }
  }
}

// Row-cooperative kernels for every other width (D % 128 == 0, D <= 2048): a
// row is split over the waves of a workgroup, thread t of them owns columns
// 4t .. 4t+3 in the forward (8-byte bf16 / 16-byte f32 accesses) and 8t .. 8t+7 in
// the backward (16-byte accesses); a wave instruction covers one contiguous span,
// and where D is no multiple of a wave's span the top lanes of a row's last wave idle.
// The row statistics go through LDS (wave sums added in wave order).  In the
// backward RCR rows are in flight per row group and pass, so one barrier serves
// RCR rows and a thread has 8 * RCR elements of every stream outstanding.  Every
// wave of a block runs the same number of passes (rows past the end are skipped
// by predicate, not by leaving), so no wave is missing at a barrier.
constexpr int NTR = 512;
constexpr int RCR = 4;  // backward
constexpr int RCF = 1;  // forward: many short blocks stream faster than fewer with more rows each

// Forward: one row group per block, rows blockIdx.x * RCF .. + RCF - 1.
template <typename T>
__global__ __launch_bounds__(NTR) void ln_fwd_kernel_rc(LnParams p) {
  __shared__ float red[2][RCF][NTR / 64];
  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), nwv = blockDim.x >> 6;
  const int c = 4 * threadIdx.x;
  const bool act = c < p.D;
  const int row0 = blockIdx.x * RCF;
  float s[RCF][4], g[4], b[4];
  if (act) {
    load4<float>(p.gamma + c, g);
    load4<float>(p.beta + c, b);
  }
#pragma unroll
  for (int r = 0; r < RCF; ++r) {
#pragma unroll
    for (int e = 0; e < 4; ++e) s[r][e] = 0.f;
    if (act && row0 + r < p.rows) load4<T>((const T*)p.y + (int64_t)(row0 + r) * p.D + c, s[r]);
  }
  if (p.x) {
    float xv[RCF][4];
#pragma unroll
    for (int r = 0; r < RCF; ++r) {
#pragma unroll
      for (int e = 0; e < 4; ++e) xv[r][e] = 0.f;
      if (act && row0 + r < p.rows) load4<T>((const T*)p.x + (int64_t)(row0 + r) * p.D + c, xv[r]);
    }
    if (p.thresh && p.n_masks > 0) {
#pragma unroll
      for (int r = 0; r < RCF; ++r)
#pragma unroll
        for (int e = 0; e < 4; e += 2) {
          float m0, m1;
          branch_scale2(p, (uint64_t)((int64_t)(row0 + r) * p.D + c + e), m0, m1);
          s[r][e] *= m0;
          s[r][e + 1] *= m1;
        }
    }
#pragma unroll
    for (int r = 0; r < RCF; ++r)
#pragma unroll
      for (int e = 0; e < 4; ++e) s[r][e] += xv[r][e];
  } else if (p.thresh && p.n_masks > 0) {
#pragma unroll
    for (int r = 0; r < RCF; ++r)
#pragma unroll
      for (int e = 0; e < 4; e += 2) {
        float m0, m1;
        branch_scale2(p, (uint64_t)((int64_t)(row0 + r) * p.D + c + e), m0, m1);
        s[r][e] *= m0;
        s[r][e + 1] *= m1;
      }
  }
  float mean[RCF], rstd[RCF];
#pragma unroll
  for (int r = 0; r < RCF; ++r) {
    const float t = wave_sum((s[r][0] + s[r][1]) + (s[r][2] + s[r][3]));
    if (lane == 0) red[0][r][w] = t;
  }
  __syncthreads();
#pragma unroll
  for (int r = 0; r < RCF; ++r) {
    float t = 0.f;
    for (int k = 0; k < nwv; ++k) t += red[0][r][k];
    mean[r] = t / p.D;
    float sq = 0.f;
    if (act) {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float d = s[r][e] - mean[r];
        sq += d * d;
      }
    }
    sq = wave_sum(sq);
    if (lane == 0) red[1][r][w] = sq;
  }
  __syncthreads();
#pragma unroll
  for (int r = 0; r < RCF; ++r) {
    float t = 0.f;
    for (int k = 0; k < nwv; ++k) t += red[1][r][k];
    rstd[r] = rsqrtf(t / p.D + p.eps);
    if (threadIdx.x == 0 && row0 + r < p.rows) {
      p.mean[row0 + r] = mean[r];
      p.rstd[row0 + r] = rstd[r];
    }
  }
  if (!act) return;  // past the last barrier
#pragma unroll
  for (int r = 0; r < RCF; ++r) {
    const int row = row0 + r;
    if (row >= p.rows) break;
    const int64_t base = (int64_t)row * p.D + c;
    if (p.s_out) store4<T>((T*)p.s_out + base, s[r]);
    float o[4];
    // round to the storage type first so `rot_out` rotates exactly what `out` holds
#pragma unroll
    for (int e = 0; e < 4; ++e) o[e] = to_f32(from_f32<T>((s[r][e] - mean[r]) * rstd[r] * g[e] + b[e]));
    store4<T>((T*)p.out + base, o);
    if (p.rot_out) {
      const int t = row % p.rope_T, half = p.D >> 1;
      const float2 cs = *(const float2*)(p.rope_cos + (int64_t)t * half + (c >> 1));
      const float2 sn = *(const float2*)(p.rope_sin + (int64_t)t * half + (c >> 1));
      float rr[4];
      rr[0] = o[0] * cs.x - o[1] * sn.x;
      rr[1] = o[0] * sn.x + o[1] * cs.x;
      rr[2] = o[2] * cs.y - o[3] * sn.y;
      rr[3] = o[2] * sn.y + o[3] * cs.y;
      store4<T>((T*)p.rot_out + base, rr);
    }
  }
}

// Backward: a thread owns CB = 8 columns (one 16-byte bf16 access, two for f32), so
// a row takes WPRB = ceil(D / 512) waves and the per-row work outside the element
// loop (two wave sums, the LDS round, addresses) is spread over twice the elements.
// A block is NG = max(1, 8 / WPRB) row groups; group g of block b takes rows
// (b * NG + g) + i * gridDim.x * NG, RCR of them per pass, with the next pass's rows
// loaded before the current ones are reduced.  A thread keeps its columns over all
// of its rows, so the per-block partials come straight from registers, summed over
// the row groups (in group order) through LDS when NG > 1.
constexpr int CB = 8;
constexpr int RC_PART_LDS = 7 * 3 * 512;  // (NG - 1) * 3 * D floats at most: D = 512, NG = 8

template <typename T>
__global__ __launch_bounds__(NTR) void ln_bwd_kernel_rc(LnParams p) {
  __shared__ float red[2][RCR][2][NTR / 64];  // [pass parity][row][a1 | a2][wave]: one barrier per pass
  __shared__ float pr[RC_PART_LDS];
  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int wpr = (p.D + 64 * CB - 1) / (64 * CB), ng = (int)(blockDim.x >> 6) / wpr;
  const int g = w / wpr, w0 = g * wpr;
  const int c = CB * ((w - w0) * 64 + lane);
  const bool act = c < p.D;
  const int stride = gridDim.x * ng;
  const int first = blockIdx.x * ng + g;
  const float inv_d = 1.0f / p.D;
  float gam[CB], dg[CB], db[CB], dyb[CB];
#pragma unroll
  for (int e = 0; e < CB; ++e) gam[e] = dg[e] = db[e] = dyb[e] = 0.f;
  if (act) loadG<float, CB>(p.gamma + c, gam);
  float xh[RCR][CB], gy[RCR][CB], mean[RCR], rstd[RCR];
  // rows first + (i0 + r) * stride, r < RCR; zeros where there is no such row
  auto load = [&](int i0, float (&x)[RCR][CB], float (&gr)[RCR][CB], float (&mu)[RCR], float (&rs)[RCR]) {
#pragma unroll
    for (int r = 0; r < RCR; ++r) {
      const int row = first + (i0 + r) * stride;
      const bool ok = row < p.rows;
#pragma unroll
      for (int e = 0; e < CB; ++e) x[r][e] = gr[r][e] = 0.f;
      mu[r] = rs[r] = 0.f;
      if (ok) {
        mu[r] = p.mean[row];
        rs[r] = p.rstd[row];
      }
      if (ok && act) {
        const int64_t base = (int64_t)row * p.D + c;
        loadG<T, CB>((const T*)p.s_in + base, x[r]);
        loadG<float, CB>(p.dout + base, gr[r]);
        if (p.dout2) {
          float a8[CB];
          loadG<T, CB>((const T*)p.dout2 + base, a8);
#pragma unroll
          for (int e = 0; e < CB; ++e) gr[r][e] += a8[e];
        }
      }
    }
  };
  load(0, xh, gy, mean, rstd);
  // Block-uniform trip count: group 0 has the block's lowest rows, so it decides.
  int par = 0;
  for (int i0 = 0; blockIdx.x * ng + i0 * stride < p.rows; i0 += RCR, par ^= 1) {
    float xn[RCR][CB], gn[RCR][CB], mn[RCR], rn[RCR];
    load(i0 + RCR, xn, gn, mn, rn);
#pragma unroll
    for (int r = 0; r < RCR; ++r) {
      float a1 = 0.f, a2 = 0.f;
#pragma unroll
      for (int e = 0; e < CB; ++e) {
        xh[r][e] = (xh[r][e] - mean[r]) * rstd[r];
        dg[e] += gy[r][e] * xh[r][e];
        db[e] += gy[r][e];
        const float gg = gy[r][e] * gam[e];
        a1 += gg;
        a2 += gg * xh[r][e];
      }
      a1 = wave_sum(a1);
      a2 = wave_sum(a2);
      if (lane == 0) {
        red[par][r][0][w] = a1;
        red[par][r][1][w] = a2;
      }
    }
    // the buffer of this parity was last read two passes back, ahead of the
    // previous pass's barrier
    __syncthreads();
#pragma unroll
    for (int r = 0; r < RCR; ++r) {
      const int row = first + (i0 + r) * stride;
      float m1 = 0.f, m2 = 0.f;
      for (int k = 0; k < wpr; ++k) {
        m1 += red[par][r][0][w0 + k];
        m2 += red[par][r][1][w0 + k];
      }
      m1 *= inv_d;
      m2 *= inv_d;
      if (act && row < p.rows) {
        const int64_t base = (int64_t)row * p.D + c;
        float d[CB];
#pragma unroll
        for (int e = 0; e < CB; ++e) d[e] = rstd[r] * (gy[r][e] * gam[e] - m1 - xh[r][e] * m2);
        storeG<float, CB>(p.ds + base, d);
        if (p.dbranch) {
          if (p.thresh && p.n_masks > 0) {
#pragma unroll
            for (int e = 0; e < CB; e += 2) {
              float s0, s1;
              branch_scale2(p, (uint64_t)base + e, s0, s1);
              d[e] *= s0;
              d[e + 1] *= s1;
            }
          }
#pragma unroll
          for (int e = 0; e < CB; ++e) d[e] = to_f32(from_f32<T>(d[e]));  // sum what is stored
          storeG<T, CB>((T*)p.dbranch + base, d);
#pragma unroll
          for (int e = 0; e < CB; ++e) dyb[e] += d[e];
        }
      }
    }
#pragma unroll
    for (int r = 0; r < RCR; ++r) {
#pragma unroll
      for (int e = 0; e < CB; ++e) {
        xh[r][e] = xn[r][e];
        gy[r][e] = gn[r][e];
      }
      mean[r] = mn[r];
      rstd[r] = rn[r];
    }
  }
  if (ng > 1) {  // block-uniform
    if (g > 0 && act) {
#pragma unroll
      for (int e = 0; e < CB; ++e) {
        pr[((g - 1) * 3 + 0) * p.D + c + e] = dg[e];
        pr[((g - 1) * 3 + 1) * p.D + c + e] = db[e];
        pr[((g - 1) * 3 + 2) * p.D + c + e] = dyb[e];
      }
    }
    __syncthreads();
    if (g == 0 && act) {
      for (int k = 0; k < ng - 1; ++k)
#pragma unroll
        for (int e = 0; e < CB; ++e) {
          dg[e] += pr[(k * 3 + 0) * p.D + c + e];
          db[e] += pr[(k * 3 + 1) * p.D + c + e];
          dyb[e] += pr[(k * 3 + 2) * p.D + c + e];
        }
    }
  }
  if (g != 0 || !act) return;  // past the last barrier
  const int64_t o = (int64_t)blockIdx.x * p.D + c;
  storeG<float, CB>(p.dgp + o, dg);
  storeG<float, CB>(p.dbp + o, db);
  if (p.dyp) storeG<float, CB>(p.dyp + o, dyb);
}

// Host side: the one decision "which kernel does this call run?", the table above
// nstl_ln_args in nstl.h.  The entry points and nstl_ln_route_describe read the LnRoute
// of a call; nothing else looks at D, dtype or q8 to choose a kernel.
// wave-il: V = D / 64 columns per lane, in lane groups of eight columns (16-byte bf16
// accesses) when D % 512 == 0, else of four; up to the V that still fits the registers
constexpr int IL_MAX_V_FWD = 32, IL_MAX_V_BWD = 16;
constexpr int il_group(int V) { return V % 8 == 0 ? 8 : 4; }
static_assert(NTR == 512, "RC_PART_LDS is sized for at most 8 row groups");

struct LnRoute {
  enum Family { REJECTED, WAVE, WAVE_IL, ROWCOOP } family;
  bool bf16, q8;
  int V, G;            // WAVE: ln_*_kernel<T, V>; WAVE_IL: ln_*_kernel_il<T, V, G>
  int waves, groups;   // ROWCOOP: ln_*_kernel_rc<T>, waves per row and row groups per block
  int block, grid;     // the launch
  int rows_per_block;  // forward: grid = ceil(rows / it); backward: n_part <= ceil(rows / it)
  char why[128];       // REJECTED: the error text of the entry points
};

// Validates the shape half of the arguments (the null-pointer checks on tensors are the
// entry points' and fill()'s) and routes them.
LnRoute ln_route(const nstl_ln_args* a, bool bwd) {
  LnRoute r = {};
  r.family = LnRoute::REJECTED;
  const char* fn = bwd ? "nstl_ln_bwd" : "nstl_ln_fwd";
#define NSTL_ROUTE_CHECK(cond, ...) \
  if (!(cond)) return snprintf(r.why, sizeof(r.why), __VA_ARGS__), r
  NSTL_ROUTE_CHECK(a != nullptr, "nstl_ln: null args");
  NSTL_ROUTE_CHECK(a->dtype == NSTL_F32 || a->dtype == NSTL_BF16, "nstl_ln: bad dtype");
  NSTL_ROUTE_CHECK(a->rows > 0, "nstl_ln: bad shape (rows=%d)", a->rows);
  const int D = a->D, V = D / 64;
  NSTL_ROUTE_CHECK(D >= 128 && D % 128 == 0 && D <= 2048,
                   "nstl_ln: D=%d unsupported (a multiple of 128, 128 <= D <= 2048)", D);
  r.bf16 = a->dtype == NSTL_BF16;
  r.q8 = a->q8 != nullptr;
  NSTL_ROUTE_CHECK(!r.q8 || D == 256 || D == 512 || D == 1024,
                   "nstl_ln: the q8 / q8_scale copy (fp8) needs D in 256/512/1024 (got %d)", D);
  NSTL_ROUTE_CHECK(a->n_masks >= 0 && a->n_masks <= 2 && a->p_drop >= 0.f && a->p_drop < 1.f, "nstl_ln: dropout");
  NSTL_ROUTE_CHECK(a->p_drop == 0.f || nstl_pair_index32_ok((uint64_t)a->rows * D),
                   "nstl_ln: rows*D past 2^33 dropout elements (32-bit pair index)");
  NSTL_ROUTE_CHECK(!r.q8 || (r.bf16 && a->q8_scale && (!bwd || a->dbranch) && a->ldq8 >= D && a->ldq8 % 16 == 0 &&
                             (uintptr_t)a->q8 % 16 == 0),
                   "%s: q8 needs %sbf16, q8_scale and a 16-byte aligned ldq8 >= D", fn, bwd ? "dbranch, " : "");
  const bool wave = V == 2, il = D % 256 == 0 && V <= (bwd ? IL_MAX_V_BWD : IL_MAX_V_FWD);
  r.rows_per_block = bwd ? (D % 256 == 0 ? NTB / 64 : NT / 64) : (wave || il ? NT / 64 : RCF);
  r.grid = (a->rows + r.rows_per_block - 1) / r.rows_per_block;
  if (bwd) {  // n_part blocks, each with at least one row per wave
    NSTL_ROUTE_CHECK(a->n_part > 0, "nstl_ln_bwd: partials");
    NSTL_ROUTE_CHECK(a->n_part <= r.grid, "nstl_ln_bwd: n_part (%d) must be <= rows/%d", a->n_part, r.rows_per_block);
    r.grid = a->n_part;
  }
  // the widths at which a direction runs row-cooperative (their float4 / float2 table reads)
  NSTL_ROUTE_CHECK(wave || (D % 256 == 0 && V <= IL_MAX_V_BWD) ||
                       (((uintptr_t)a->gamma | (uintptr_t)a->beta) % 16 == 0 &&
                        ((uintptr_t)a->rope_cos | (uintptr_t)a->rope_sin) % 8 == 0),
                   "nstl_ln: D=%d needs 16-byte aligned gamma/beta and 8-byte aligned rope tables", D);
#undef NSTL_ROUTE_CHECK
  if (wave || il) {
    r.family = wave ? LnRoute::WAVE : LnRoute::WAVE_IL;
    r.V = V;
    r.G = wave ? 0 : il_group(V);
    r.block = wave || !bwd ? NT : NTB;
  } else {
    r.family = LnRoute::ROWCOOP;  // forward: 4 columns per thread; backward: CB, in 8 / waves row groups
    r.waves = bwd ? (D + 64 * CB - 1) / (64 * CB) : (D + 255) / 256;
    r.groups = bwd ? NTR / 64 / r.waves : 1;
    r.block = r.groups * r.waves * 64;
  }
  return r;
}

// p filled from the arguments r routed; exactly the reachable kernels are instantiated
template <typename T, bool BWD>
int launch(const LnParams& p, const LnRoute& r, hipStream_t st) {
  const dim3 grid(r.grid), block(r.block);
  bool found = true;
  if (r.family == LnRoute::WAVE) {
    if constexpr (BWD) hipLaunchKernelGGL((ln_bwd_kernel<T, 2>), grid, block, 0, st, p);
    else hipLaunchKernelGGL((ln_fwd_kernel<T, 2>), grid, block, 0, st, p);
  } else if (r.family == LnRoute::ROWCOOP) {
    if constexpr (BWD) hipLaunchKernelGGL((ln_bwd_kernel_rc<T>), grid, block, 0, st, p);
    else hipLaunchKernelGGL((ln_fwd_kernel_rc<T>), grid, block, 0, st, p);
  } else if constexpr (BWD) {
    found = nstl::with_const<4, 8, 12, IL_MAX_V_BWD>(r.V, [&](auto V) {
      hipLaunchKernelGGL((ln_bwd_kernel_il<T, V(), il_group(V())>), grid, block, 0, st, p);
    });
  } else {
    found = nstl::with_const<4, 8, 12, 16, 20, 24, 28, IL_MAX_V_FWD>(r.V, [&](auto V) {
      hipLaunchKernelGGL((ln_fwd_kernel_il<T, V(), il_group(V())>), grid, block, 0, st, p);
    });
  }
  if (!found) return nstl::fail((int)hipErrorInvalidValue, "nstl_ln: no kernel for D=%d", p.D);
  NSTL_LAUNCH_CHECK(BWD ? "nstl_ln_bwd" : "nstl_ln_fwd");
  return 0;
}

int fill(LnParams& p, const nstl_ln_args* a) {
  NSTL_CHECK_ARG(a->gamma && a->beta, "nstl_ln: gamma/beta missing");
  p.x = (const char*)a->x; p.y = (const char*)a->y;
  p.rows = a->rows; p.D = a->D;
  p.n_masks = a->n_masks;
  p.thresh = nstl_drop_thresh(a->p_drop);
  p.inv_keep = 1.0f / (1.0f - a->p_drop);
  p.seed1 = a->seed1; p.seed2 = a->seed2;
  p.gamma = a->gamma; p.beta = a->beta; p.eps = a->eps;
  p.s_out = (char*)a->s_out; p.out = (char*)a->out; p.mean = a->mean; p.rstd = a->rstd;
  p.rot_out = (char*)a->rot_out; p.rope_cos = a->rope_cos; p.rope_sin = a->rope_sin; p.rope_T = a->rope_T;
  p.s_in = (const char*)a->s_in; p.dout = a->dout; p.ds = a->ds; p.dbranch = (char*)a->dbranch;
  p.dgp = a->dgamma_part; p.dbp = a->dbeta_part; p.dyp = a->dbranch_part;
  p.dout2 = (const char*)a->dout2;
  p.q8 = (uint8_t*)a->q8; p.ldq8 = a->ldq8; p.q8_scale = a->q8_scale;
  return 0;
}

}  // namespace

extern "C" int nstl_ln_fwd(const nstl_ln_args* a, void* stream) {
  const LnRoute r = ln_route(a, false);
  if (r.family == LnRoute::REJECTED) return nstl::fail((int)hipErrorInvalidValue, "%s", r.why);
  NSTL_CHECK_ARG(a->y && a->out && a->mean && a->rstd, "nstl_ln_fwd: null tensor");
  NSTL_CHECK_ARG(!a->rot_out || (a->rope_cos && a->rope_sin && a->rope_T > 0), "nstl_ln_fwd: rope tables");
  LnParams p;
  int rc = fill(p, a);
  if (rc) return rc;
  return r.bf16 ? launch<bf16, false>(p, r, (hipStream_t)stream) : launch<float, false>(p, r, (hipStream_t)stream);
}

extern "C" int nstl_ln_bwd(const nstl_ln_args* a, void* stream) {
  const LnRoute r = ln_route(a, true);
  if (r.family == LnRoute::REJECTED) return nstl::fail((int)hipErrorInvalidValue, "%s", r.why);
  NSTL_CHECK_ARG(a->s_in && a->dout && a->ds && a->mean && a->rstd, "nstl_ln_bwd: null tensor");
  NSTL_CHECK_ARG(a->dgamma_part && a->dbeta_part, "nstl_ln_bwd: partials");
  LnParams p;
  int rc = fill(p, a);
  if (rc) return rc;
  return r.bf16 ? launch<bf16, true>(p, r, (hipStream_t)stream) : launch<float, true>(p, r, (hipStream_t)stream);
}

extern "C" int nstl_ln_route_describe(const nstl_ln_args* a, int backward, char* buf, int n) {
  const LnRoute r = ln_route(a, backward != 0);
  const size_t cap = buf && n > 0 ? (size_t)n : 0;
  const char *dir = backward ? "bwd" : "fwd", *ty = r.bf16 ? "bf16" : "f32";
  switch (r.family) {
    case LnRoute::REJECTED: return snprintf(buf, cap, "rejected: %s", r.why);
    case LnRoute::WAVE: return snprintf(buf, cap, "wave %s %s V=%d", dir, ty, r.V);
    case LnRoute::WAVE_IL: return snprintf(buf, cap, "wave-il %s %s V=%d G=%d%s", dir, ty, r.V, r.G, r.q8 ? " q8" : "");
    case LnRoute::ROWCOOP:
      return backward ? snprintf(buf, cap, "rowcoop bwd %s waves=%d groups=%d", ty, r.waves, r.groups)
                      : snprintf(buf, cap, "rowcoop fwd %s waves=%d", ty, r.waves);
  }
  return -1;
}
