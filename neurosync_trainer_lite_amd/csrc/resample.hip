// Audio ingest kernels: the rational-ratio polyphase FIR resampler and the peak
// normalisation that follow the host's WAV parse (utils/audio/load_audio.py).
//
// nstl_resample_poly restates scipy.signal.resample_poly(x, up, down) at its
// defaults (window ('kaiser', 5.0), padtype 'constant').  With max_rate =
// max(up, down), half = 10 max_rate and the prototype h (2 half + 1 taps, built
// and scaled by `up` on the host):
//   pre = down - half % down zeros go in front of h (hp), rem = (half + pre) / down,
//   n_out = ceil(n_in up / down), and for output m, t0 = (m + rem) down:
//   y[m] = sum over k == t0 (mod up), 0 <= k < len(hp), of hp[k] x[(t0 - k) / up],
// terms whose sample index falls outside [0, n_in) dropped.  With p = t0 % up and
// q = t0 / up that is sum_j hp[p + j up] x[q - j], j = 0 .. J - 1,
// J = ceil(len(hp) / up) taps per phase: ascending j is ascending k.  One thread
// forms one output with one f32 FMA per tap in that order, so the result is a
// function of the inputs only.
//
// A workgroup computes runs of RS_RUN consecutive outputs (run = blockIdx.x,
// + gridDim.x, ...; the grid is capped at what the device holds at once so a
// workgroup builds its tap table once for several runs).  Per run it stages the
// input span the run reads, x[q_lo .. q_lo + span), zero outside [0, n_in), in
// LDS.  The tap table lives in LDS as rows of one phase each: row r holds phase
// (r down) % up, so output m reads row (m + rem) % up and consecutive outputs
// read consecutive rows; the row stride is odd (J | 1), which puts the 32 lanes
// of a ds_read_b32 group on 32 different banks.  (Rows, not phases, index the
// table, so a ratio that is not in lowest terms only repeats some phases.)
// Two template flags take the same arithmetic to global memory where LDS does not
// hold it: TG reads the taps from h (tables past the 64 KB a workgroup may take,
// e.g. 11025/5507), XG reads the samples from x (spans past it: strong decimation).
#include <algorithm>

#include "../../include/nstl.h"
#include "common.h"
#include "status.h"

namespace {
constexpr int RS_NT = 256;            // threads per workgroup
constexpr int RS_PER = 4;             // outputs per thread and run
constexpr int RS_RUN = RS_NT * RS_PER;
constexpr int RS_MAX_RATE = 16384;
constexpr int64_t RS_LDS_BYTES = 64 * 1024 - 64;  // dynamic LDS of one workgroup (+ the 4 wave maxima)

struct RsParams {
  const float* x;
  int64_t n_in;
  int up, down;
  const float* h;
  int n_taps;
  int pre;       // zeros in front of h
  int64_t rem;   // outputs of the full convolution dropped at the front
  int J, S;      // taps per phase, table row stride (floats)
  float* y;
  int64_t n_out, n_runs;
  int span;      // staged samples per run
  unsigned* peak;
};

template <bool TG, bool XG>
__global__ __launch_bounds__(RS_NT) void resample_kernel(const RsParams P) {
  extern __shared__ __attribute__((aligned(16))) float rs_smem[];
  __shared__ float red[RS_NT / 64];
  float* T = rs_smem;                                // [up][S], absent with TG
  float* xs = rs_smem + (TG ? 0 : P.up * P.S);       // [span], absent with XG
  const int tid = threadIdx.x;
  const int up = P.up, down = P.down, J = P.J, S = P.S, pre = P.pre;
  if constexpr (!TG) {
    // j-major over the table: the threads of one j read one window of `up` taps
    // and write LDS S floats apart (odd: no bank conflict)
    for (int idx = tid; idx < up * J; idx += RS_NT) {
      const int j = idx / up, r = idx - j * up;
      const int k = (int)(((int64_t)r * down) % up) + j * up - pre;
      T[r * S + j] = (k >= 0 && k < P.n_taps) ? P.h[k] : 0.f;
    }
  }
  float pk = 0.f;
  for (int64_t run = blockIdx.x; run < P.n_runs; run += gridDim.x) {
    const int64_t m0 = run * RS_RUN;
    const int cnt = (int)std::min<int64_t>(RS_RUN, P.n_out - m0);
    const int64_t M0 = m0 + P.rem;
    const int64_t t_base = M0 * down;            // < 2^63: n_in up < 2^62
    const int64_t qb = t_base / up;
    const int pb = (int)(t_base - qb * up);
    const int rb = (int)(M0 % up);
    const int64_t q_lo = qb - (J - 1);
    if constexpr (!XG) {
      __syncthreads();                           // the previous run's readers are done
      for (int i = tid; i < P.span; i += RS_NT) {
        const int64_t s = q_lo + i;
        xs[i] = (s >= 0 && s < P.n_in) ? P.x[s] : 0.f;
      }
    }
    __syncthreads();
    // output m0 + l: t0 = t_base + l down, so p and q follow from 32-bit arithmetic
    // (pb + l down < 2^14 + 2^24)
    int row[RS_PER], ph[RS_PER], xo[RS_PER];
    float acc[RS_PER];
#pragma unroll
    for (int i = 0; i < RS_PER; ++i) {
      const int l = tid + i * RS_NT < cnt ? tid + i * RS_NT : 0;
      const int tl = pb + l * down;
      const int dq = tl / up;
      ph[i] = tl - dq * up;
      xo[i] = dq + J - 1;                        // x[q] in xs; x[q - j] at xo - j >= 0
      row[i] = ((rb + l) % up) * S;
      acc[i] = 0.f;
    }
    for (int j = 0; j < J; ++j) {
#pragma unroll
      for (int i = 0; i < RS_PER; ++i) {
        float tap, v;
        if constexpr (TG) {
          const int k = ph[i] + j * up - pre;
          tap = (k >= 0 && k < P.n_taps) ? P.h[k] : 0.f;
        } else {
          tap = T[row[i] + j];
        }
        if constexpr (XG) {
          const int64_t s = q_lo + xo[i] - j;
          v = (s >= 0 && s < P.n_in) ? P.x[s] : 0.f;
        } else {
          v = xs[xo[i] - j];
        }
        acc[i] = fmaf(tap, v, acc[i]);
      }
    }
#pragma unroll
    for (int i = 0; i < RS_PER; ++i) {
      const int l = tid + i * RS_NT;
      if (l < cnt) {
        P.y[m0 + l] = acc[i];
        pk = fmaxf(pk, fabsf(acc[i]));
      }
    }
  }
  if (P.peak != nullptr) {
    pk = wave_max(pk);
    if ((tid & 63) == 0) red[tid >> 6] = pk;
    __syncthreads();
    // non-negative floats order as their bit patterns do
    if (tid == 0) atomicMax(P.peak, __float_as_uint(fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]))));
  }
}

__global__ __launch_bounds__(256) void peak_normalise_kernel(float* y, int64_t n, const float* peak) {
  const float p = *peak;
  if (!(p > 0.f)) return;
  const int64_t step = (int64_t)gridDim.x * 256;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += step) y[i] = __fdiv_rn(y[i], p);
}

bool rs_rate_ok(int64_t n_in, int up, int down) {
  return n_in >= 1 && up >= 1 && up <= RS_MAX_RATE && down >= 1 && down <= RS_MAX_RATE &&
         n_in <= ((int64_t(1) << 62) - 1) / up;
}
}  // namespace

extern "C" int64_t nstl_resample_out_len(int64_t n_in, int up, int down) {
  if (!rs_rate_ok(n_in, up, down)) return 0;
  return (n_in * up + down - 1) / down;
}

extern "C" int nstl_resample_poly(const nstl_resample_args* a, void* stream) {
  NSTL_CHECK_ARG(a != nullptr, "nstl_resample_poly: null args");
  NSTL_CHECK_ARG(a->x && a->taps && a->y, "nstl_resample_poly: null pointer (x, taps and y are required)");
  NSTL_CHECK_ARG(a->n_in >= 1, "nstl_resample_poly: n_in %lld < 1", (long long)a->n_in);
  NSTL_CHECK_ARG(a->up >= 1 && a->up <= RS_MAX_RATE && a->down >= 1 && a->down <= RS_MAX_RATE,
                 "nstl_resample_poly: up %d / down %d outside [1, %d]", a->up, a->down, RS_MAX_RATE);
  const int max_rate = std::max(a->up, a->down);
  NSTL_CHECK_ARG(a->n_taps == 20 * max_rate + 1, "nstl_resample_poly: n_taps %d != 20 max(up, down) + 1 = %d",
                 a->n_taps, 20 * max_rate + 1);
  NSTL_CHECK_ARG(a->n_in <= ((int64_t(1) << 62) - 1) / a->up, "nstl_resample_poly: n_in up = %lld x %d >= 2^62",
                 (long long)a->n_in, a->up);
  const int64_t n_out = nstl_resample_out_len(a->n_in, a->up, a->down);
  NSTL_CHECK_ARG(a->n_out == n_out, "nstl_resample_poly: n_out %lld != nstl_resample_out_len = %lld",
                 (long long)a->n_out, (long long)n_out);
  hipStream_t st = (hipStream_t)stream;
  RsParams P;
  P.x = a->x;
  P.n_in = a->n_in;
  P.up = a->up;
  P.down = a->down;
  P.h = a->taps;
  P.n_taps = a->n_taps;
  const int half = 10 * max_rate;
  P.pre = a->down - half % a->down;
  P.rem = (half + P.pre) / a->down;
  const int len_hp = P.pre + a->n_taps;
  P.J = (len_hp + a->up - 1) / a->up;
  P.S = P.J | 1;
  P.y = a->y;
  P.n_out = n_out;
  P.n_runs = (n_out + RS_RUN - 1) / RS_RUN;
  const int64_t span = ((int64_t)(RS_RUN - 1) * a->down) / a->up + 2 + P.J;
  P.peak = (unsigned*)a->peak;
  const int64_t table_bytes = (int64_t)a->up * P.S * 4, span_bytes = span * 4;
  const bool xg = span_bytes > RS_LDS_BYTES;
  const bool tg = table_bytes + (xg ? 0 : span_bytes) > RS_LDS_BYTES;
  P.span = xg ? 0 : (int)span;
  const size_t lds = (size_t)((tg ? 0 : table_bytes) + (xg ? 0 : span_bytes));
  if (a->peak != nullptr) {
    const hipError_t e = hipMemsetAsync(a->peak, 0, sizeof(float), st);
    if (e != hipSuccess) return nstl::fail((int)e, "nstl_resample_poly: zeroing peak: %s", hipGetErrorString(e));
  }
  // as many workgroups as the device holds at once: a CU's 160 KB of LDS, 8 at most
  const int per_cu = (int)std::max<int64_t>(1, std::min<int64_t>(8, (160 * 1024) / std::max<size_t>(lds + 64, 1)));
  const int cus = std::max(1, nstl::stream_cus(st));
  const unsigned grid = (unsigned)std::min<int64_t>(P.n_runs, (int64_t)cus * per_cu);
  if (tg && xg) hipLaunchKernelGGL((resample_kernel<true, true>), dim3(grid), dim3(RS_NT), lds, st, P);
  else if (tg) hipLaunchKernelGGL((resample_kernel<true, false>), dim3(grid), dim3(RS_NT), lds, st, P);
  else if (xg) hipLaunchKernelGGL((resample_kernel<false, true>), dim3(grid), dim3(RS_NT), lds, st, P);
  else hipLaunchKernelGGL((resample_kernel<false, false>), dim3(grid), dim3(RS_NT), lds, st, P);
  NSTL_LAUNCH_CHECK("nstl_resample_poly");
  return 0;
}

extern "C" int nstl_peak_normalise(float* y, int64_t n, const float* peak, void* stream) {
  NSTL_CHECK_ARG(y != nullptr && peak != nullptr, "nstl_peak_normalise: null pointer");
  NSTL_CHECK_ARG(n >= 0, "nstl_peak_normalise: n %lld < 0", (long long)n);
  if (n == 0) return 0;
  const unsigned grid = (unsigned)std::min<int64_t>((n + 255) / 256, 4096);
  hipLaunchKernelGGL(peak_normalise_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, y, n, peak);
  NSTL_LAUNCH_CHECK("nstl_peak_normalise");
  return 0;
}
