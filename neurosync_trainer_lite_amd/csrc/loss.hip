// Fused Loss forward + backward (replaces Loss.forward, utils/model.py:278-291,
// and its autograd graph: SmoothL1 + L1 of first differences + directional
// cosine of first differences, eps 1e-8 added to the difference norms).
//
//   rec  = mean_{b,t,f} huber_delta(p - y)
//   temp = mean_{b,t<T-1,f} |dp - dy|                   dp_t = p_{t+1} - p_t
//   dir  = 1 - mean_{b,t<T-1} <dp_t/(|dp_t|+eps), dy_t/(|dy_t|+eps)>
//   loss = w1 rec + w2 temp + w3 dir
// One workgroup per sequence b: the clip is staged in LDS, per-step norms are
// wave reductions, the gradient is written straight into the (zero-padded)
// dpred operand of the output-head backward GEMMs.
#include <stdlib.h>

#include "../../include/nstl.h"
#include "common.h"
#include "status.h"

namespace {
// 16 waves per sequence: the per-step cosine chain (3 wave reductions per step)
// runs T/16 steps deep instead of T/4 (58 -> ~20 us at B=128, T=128)
constexpr int NT = 1024;
constexpr int TMAX_NARROW = 256, FMAX_NARROW = 64, TMAX_WIDE = 128, FMAX_WIDE = 128;  // the two tiles <FMAX, TMAX>

struct LossParams {
  int B, T, F;
  const float* pred; int64_t pred_ld;
  const float* trg; int64_t trg_ld;
  float delta, w1, w2, w3, gscale;
  char* dpred; int d_f32; int64_t dpred_ld;
  float* partial; float* out;
};

template <int FMAX, int TMAX> __global__ __launch_bounds__(NT) void loss_kernel(LossParams p) {
  __shared__ float P[TMAX][FMAX + 1];
  __shared__ float Y[TMAX][FMAX + 1];
  // per-step scalars: 1/(|dp|+eps), 1/(|dy|+eps), cos_t, |dp|
  __shared__ float s_inp[TMAX], s_iny[TMAX], s_cos[TMAX], s_np[TMAX];
  __shared__ float red[3][NT / 64];
  const int b = blockIdx.x, T = p.T, F = p.F;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  for (int e = tid; e < T * F; e += NT) {
    const int t = e / F, f = e % F;
    P[t][f] = p.pred[((int64_t)b * T + t) * p.pred_ld + f];
    Y[t][f] = p.trg[((int64_t)b * T + t) * p.trg_ld + f];
  }
  __syncthreads();
  // per-step cosine terms (one wave per step)
  float cos_acc = 0.f;
  for (int t = w; t < T - 1; t += NT / 64) {
    float np2 = 0.f, ny2 = 0.f;
    for (int f = lane; f < F; f += 64) {
      const float dp = P[t + 1][f] - P[t][f], dy = Y[t + 1][f] - Y[t][f];
      np2 += dp * dp;
      ny2 += dy * dy;
    }
    const float np = sqrtf(wave_sum(np2)), ny = sqrtf(wave_sum(ny2));
    const float inp = 1.f / (np + 1e-8f), iny = 1.f / (ny + 1e-8f);
    float dot = 0.f;
    for (int f = lane; f < F; f += 64) {
      const float dp = P[t + 1][f] - P[t][f], dy = Y[t + 1][f] - Y[t][f];
      dot += (dp * inp) * (dy * iny);
    }
    const float cs = wave_sum(dot);  // cos_t = sum_f pn * tn (same value in every lane)
    if (lane == 0) cos_acc += cs;
    if (lane == 0) {
      s_inp[t] = inp;
      s_iny[t] = iny;
      s_cos[t] = cs;
      s_np[t] = np;
    }
  }
  __syncthreads();
  const float n_rec = (float)p.B * T * F;
  const float n_tmp = (float)p.B * (T - 1) * F;
  const float n_dir = (float)p.B * (T - 1);
  float rec_acc = 0.f, tmp_acc = 0.f;
  const int ldd = (int)p.dpred_ld;
  // d cos_t / d dp_{t,f} = tn_f/(|dp|+eps) - cos_t * dp_f / (|dp| (|dp|+eps))  (2nd term 0 if |dp| == 0,
  // torch's norm backward at the origin)
  auto gcos = [&](int t, int f) {
    const float dp = P[t + 1][f] - P[t][f], dy = Y[t + 1][f] - Y[t][f];
    float gv = dy * s_iny[t] * s_inp[t];
    const float np = s_np[t];
    if (np > 0.f) gv -= s_cos[t] * dp / (np * (np + 1e-8f));
    return gv;
  };
  for (int e = tid; e < T * ldd; e += NT) {
    const int t = e / ldd, f = e % ldd;
    float g = 0.f;
    if (f < F) {
      const float d = P[t][f] - Y[t][f], ad = fabsf(d);
      rec_acc += ad < p.delta ? 0.5f * d * d / p.delta : ad - 0.5f * p.delta;
      g = p.w1 * (ad < p.delta ? d / p.delta : (d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f))) / n_rec;
      // gradient w.r.t. dp_{t-1} (+) and dp_t (-)
      float gd_prev = 0.f, gd_cur = 0.f;
      if (t >= 1) {
        const float z = (P[t][f] - P[t - 1][f]) - (Y[t][f] - Y[t - 1][f]);
        gd_prev = p.w2 * (z > 0.f ? 1.f : (z < 0.f ? -1.f : 0.f)) / n_tmp - p.w3 * gcos(t - 1, f) / n_dir;
      }
      if (t < T - 1) {
        const float z = (P[t + 1][f] - P[t][f]) - (Y[t + 1][f] - Y[t][f]);
        tmp_acc += fabsf(z);
        gd_cur = p.w2 * (z > 0.f ? 1.f : (z < 0.f ? -1.f : 0.f)) / n_tmp - p.w3 * gcos(t, f) / n_dir;
      }
      g = (g + gd_prev - gd_cur) * p.gscale;
    }
    const int64_t o = ((int64_t)b * T + t) * p.dpred_ld + f;
    if (p.d_f32) ((float*)p.dpred)[o] = g;
    else ((bf16*)p.dpred)[o] = (bf16)g;
  }
  rec_acc = wave_sum(rec_acc);
  tmp_acc = wave_sum(tmp_acc);
  cos_acc = wave_sum(cos_acc);
  if (lane == 0) {
    red[0][w] = rec_acc;
    red[1][w] = tmp_acc;
    red[2][w] = cos_acc;
  }
  __syncthreads();
  if (tid < 3) {
    float s = 0.f;
    for (int k = 0; k < NT / 64; ++k) s += red[tid][k];
    p.partial[b * 4 + tid] = s;
  }
}

// Clips longer than TMAX frames: the same sums over time chunks of CH = TMAX - 2 frames, each
// staged with one frame of halo on either side (the first differences, and the
// cosine gradient's t-1 and t terms, reach one frame across a chunk edge).  The
// step s = t0 - 1 that straddles two chunks is evaluated in both with identical
// values, and counted in the cosine sum by the chunk that owns frame s.
template <int TMAX> constexpr int CH = TMAX - 2;  // frames a chunk owns: 254 (narrow tile), 126 (wide tile)
constexpr int TMAX_LONG = 4096;

template <int FMAX, int TMAX> __global__ __launch_bounds__(NT) void loss_long_kernel(LossParams p) {
  __shared__ float P[TMAX][FMAX + 1];
  __shared__ float Y[TMAX][FMAX + 1];
  __shared__ float s_inp[TMAX], s_iny[TMAX], s_cos[TMAX], s_np[TMAX];
  __shared__ float red[3][NT / 64];
  const int b = blockIdx.x, T = p.T, F = p.F;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const float n_rec = (float)p.B * T * F;
  const float n_tmp = (float)p.B * (T - 1) * F;
  const float n_dir = (float)p.B * (T - 1);
  const int ldd = (int)p.dpred_ld;
  float cos_acc = 0.f, rec_acc = 0.f, tmp_acc = 0.f;
  for (int t0 = 0; t0 < T; t0 += CH<TMAX>) {
    const int t1 = min(T, t0 + CH<TMAX>);                      // frames this chunk owns: [t0, t1)
    const int lo = max(t0 - 1, 0), hi = min(t1 + 1, T);  // staged frames [lo, hi), row = t - lo
    const int n = hi - lo;
    for (int e = tid; e < n * F; e += NT) {
      const int lt = e / F, f = e % F;
      P[lt][f] = p.pred[((int64_t)b * T + lo + lt) * p.pred_ld + f];
      Y[lt][f] = p.trg[((int64_t)b * T + lo + lt) * p.trg_ld + f];
    }
    __syncthreads();
    // steps lo .. hi-2 (one wave per step), row ls = step - lo
    for (int ls = w; ls < n - 1; ls += NT / 64) {
      float np2 = 0.f, ny2 = 0.f;
      for (int f = lane; f < F; f += 64) {
        const float dp = P[ls + 1][f] - P[ls][f], dy = Y[ls + 1][f] - Y[ls][f];
        np2 += dp * dp;
        ny2 += dy * dy;
      }
      const float np = sqrtf(wave_sum(np2)), ny = sqrtf(wave_sum(ny2));
      const float inp = 1.f / (np + 1e-8f), iny = 1.f / (ny + 1e-8f);
      float dot = 0.f;
      for (int f = lane; f < F; f += 64) {
        const float dp = P[ls + 1][f] - P[ls][f], dy = Y[ls + 1][f] - Y[ls][f];
        dot += (dp * inp) * (dy * iny);
      }
      const float cs = wave_sum(dot);
      if (lane == 0) {
        if (lo + ls >= t0) cos_acc += cs;  // the halo step belongs to the previous chunk
        s_inp[ls] = inp;
        s_iny[ls] = iny;
        s_cos[ls] = cs;
        s_np[ls] = np;
      }
    }
    __syncthreads();
    auto gcos = [&](int ls, int f) {
      const float dp = P[ls + 1][f] - P[ls][f], dy = Y[ls + 1][f] - Y[ls][f];
      float gv = dy * s_iny[ls] * s_inp[ls];
      const float np = s_np[ls];
      if (np > 0.f) gv -= s_cos[ls] * dp / (np * (np + 1e-8f));
      return gv;
    };
    for (int e = tid; e < (t1 - t0) * ldd; e += NT) {
      const int t = t0 + e / ldd, f = e % ldd, lt = t - lo;
      float g = 0.f;
      if (f < F) {
        const float d = P[lt][f] - Y[lt][f], ad = fabsf(d);
        rec_acc += ad < p.delta ? 0.5f * d * d / p.delta : ad - 0.5f * p.delta;
        g = p.w1 * (ad < p.delta ? d / p.delta : (d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f))) / n_rec;
        float gd_prev = 0.f, gd_cur = 0.f;
        if (t >= 1) {
          const float z = (P[lt][f] - P[lt - 1][f]) - (Y[lt][f] - Y[lt - 1][f]);
          gd_prev = p.w2 * (z > 0.f ? 1.f : (z < 0.f ? -1.f : 0.f)) / n_tmp - p.w3 * gcos(lt - 1, f) / n_dir;
        }
        if (t < T - 1) {
          const float z = (P[lt + 1][f] - P[lt][f]) - (Y[lt + 1][f] - Y[lt][f]);
          tmp_acc += fabsf(z);
          gd_cur = p.w2 * (z > 0.f ? 1.f : (z < 0.f ? -1.f : 0.f)) / n_tmp - p.w3 * gcos(lt, f) / n_dir;
        }
        g = (g + gd_prev - gd_cur) * p.gscale;
      }
      const int64_t o = ((int64_t)b * T + t) * p.dpred_ld + f;
      if (p.d_f32) ((float*)p.dpred)[o] = g;
      else ((bf16*)p.dpred)[o] = (bf16)g;
    }
    __syncthreads();  // the next chunk restages P / Y and the step scalars
  }
  rec_acc = wave_sum(rec_acc);
  tmp_acc = wave_sum(tmp_acc);
  cos_acc = wave_sum(cos_acc);
  if (lane == 0) {
    red[0][w] = rec_acc;
    red[1][w] = tmp_acc;
    red[2][w] = cos_acc;
  }
  __syncthreads();
  if (tid < 3) {
    float s = 0.f;
    for (int k = 0; k < NT / 64; ++k) s += red[tid][k];
    p.partial[b * 4 + tid] = s;
  }
}

__global__ void loss_final(LossParams p) {
  // deterministic combine over the sequences in double: lane l sums sequences
  // l, l + 64, ... in order, then a fixed butterfly over the wave
  const int l = threadIdx.x;
  double r = 0, t = 0, c = 0;
  for (int b = l; b < p.B; b += 64) {
    r += p.partial[b * 4 + 0];
    t += p.partial[b * 4 + 1];
    c += p.partial[b * 4 + 2];
  }
  r = wave_sum_d(r);
  t = wave_sum_d(t);
  c = wave_sum_d(c);
  if (l != 0) return;
  const double rec = r / ((double)p.B * p.T * p.F);
  const double tmp = t / ((double)p.B * (p.T - 1) * p.F);
  const double dir = 1.0 - c / ((double)p.B * (p.T - 1));
  p.out[0] = (float)(p.w1 * rec + p.w2 * tmp + p.w3 * dir);
  p.out[1] = (float)rec;
  p.out[2] = (float)tmp;
  p.out[3] = (float)dir;
}
}  // namespace

// Two LDS tiles, both with an odd row stride and one workgroup per CU (160 KiB of LDS):
//   narrow  F <= 64:   P, Y [256][65]  f32 = 133,120 B; 137,408 B with the step scalars and red
//   wide    F <= 128:  P, Y [128][129] f32 = 132,096 B; 134,336 B likewise (NSTL_LOSS_WIDE_OK)
// Both kernels are templates on the tile.  The per-step loops stride f += 64, so a lane
// of the wide form owns up to two elements of each step sum; the chunked form stages at
// most CH + 2 = TMAX rows.  Everything a tile needs (F <= FMAX, the T range) is checked
// here, and the chunk loop's bound comes from T alone.
extern "C" int nstl_loss_fwd_bwd(const nstl_loss_args* a, void* stream) {
  NSTL_CHECK_ARG(a != nullptr, "nstl_loss: null args");
  // flags 0: the limits of version 5; NSTL_LOSS_WIDE_OK: 64 < F <= 128 takes the wide tile
  const int fmax = (a->flags & NSTL_LOSS_WIDE_OK) ? FMAX_WIDE : FMAX_NARROW;
  NSTL_CHECK_ARG(a->B > 0 && a->T >= 2 && a->T <= TMAX_LONG && a->F > 0 && a->F <= fmax,
                 "nstl_loss: shape B=%d T=%d F=%d unsupported (T in [2,%d], F <= %d)", a->B, a->T, a->F, TMAX_LONG,
                 fmax);
  NSTL_CHECK_ARG(a->pred && a->trg && a->dpred && a->partial && a->loss_out, "nstl_loss: null tensor");
  NSTL_CHECK_ARG(a->dpred_ld >= a->F && a->pred_ld >= a->F && a->trg_ld >= a->F, "nstl_loss: ld < F");
  NSTL_CHECK_ARG(a->delta > 0.f, "nstl_loss: delta must be > 0");
  LossParams p;
  p.B = a->B; p.T = a->T; p.F = a->F;
  p.pred = a->pred; p.pred_ld = a->pred_ld;
  p.trg = a->trg; p.trg_ld = a->trg_ld;
  p.delta = a->delta; p.w1 = a->w1; p.w2 = a->w2; p.w3 = a->w3; p.gscale = a->grad_scale;
  p.dpred = (char*)a->dpred; p.d_f32 = a->dpred_dtype == NSTL_F32; p.dpred_ld = a->dpred_ld;
  p.partial = a->partial; p.out = a->loss_out;
  hipStream_t st = (hipStream_t)stream;
  // NSTL_LOSS_CHUNKED=1: the chunked kernel also where the whole clip fits (tests; read per call)
  const char* e = getenv("NSTL_LOSS_CHUNKED");
  const bool forced = e && e[0] == '1';
  if (a->F > FMAX_NARROW) {  // only with NSTL_LOSS_WIDE_OK (checked above); F <= FMAX_WIDE
    if (a->T > TMAX_WIDE || forced)
      hipLaunchKernelGGL((loss_long_kernel<FMAX_WIDE, TMAX_WIDE>), dim3(a->B), dim3(NT), 0, st, p);
    else
      hipLaunchKernelGGL((loss_kernel<FMAX_WIDE, TMAX_WIDE>), dim3(a->B), dim3(NT), 0, st, p);
    NSTL_LAUNCH_CHECK("nstl_loss_fwd_bwd");
    nstl::count(NSTL_K_LOSS_WIDE);
  } else {
    if (a->T > TMAX_NARROW || forced)
      hipLaunchKernelGGL((loss_long_kernel<FMAX_NARROW, TMAX_NARROW>), dim3(a->B), dim3(NT), 0, st, p);
    else
      hipLaunchKernelGGL((loss_kernel<FMAX_NARROW, TMAX_NARROW>), dim3(a->B), dim3(NT), 0, st, p);
    NSTL_LAUNCH_CHECK("nstl_loss_fwd_bwd");
  }
  hipLaunchKernelGGL(loss_final, dim3(1), dim3(64), 0, st, p);
  NSTL_LAUNCH_CHECK("nstl_loss_fwd_bwd final");
  return 0;
}
