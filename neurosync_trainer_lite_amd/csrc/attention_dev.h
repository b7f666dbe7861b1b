// What attention.hip (one-shot kernels, T <= 256) and attention_long.hip (streaming
// kernels, 256 < T <= 4096) share, stated once: the parameter block, the
// 128-byte-row operand image and its inline-asm reads, the dropout element index
// and keep-bit words, the register-operand fragment order, the staged tile store,
// RoPE^T and the bias partial sums.  These are the conventions that make the two
// paths interchangeable (a forward of one, stored keep bits included, feeds the
// backward of the other).  Tile and workgroup sizes (NT, NW, ROWS, KT, ...) are
// each file's own.  AttnParams crosses from attention.hip's entry points to
// attention_long.hip's launchers, so it has a name (nstl::); everything else sits
// in the including file's anonymous namespace, next to its kernels.
// DH = 64 is the width of one operand image and of one result tile.  The streaming
// kernels also take head_dim 128 as two such halves, and reuse every helper here per
// half; only RoPE^T knows the head's width (the pair index offset of the half and the
// frequency divisor: rope_tab's i0, rope_tab_fast<DHT>, rope_back_tile<DHT>).
#pragma once
#include "common.h"
#include "status.h"

namespace nstl {
// filled once per call by nstl_attn_fwd / nstl_attn_bwd (attention.hip: fill) and
// passed by value to every kernel of both files
struct AttnParams {
  const char* q; int64_t q_ld;
  const char* k; int64_t k_ld;
  const char* v; int64_t v_ld;
  char* o; int64_t o_ld;
  float* lse;
  float* dsum;
  uint64_t* mask;  // dropout keep bits (fast path), see mask_word()
  float* dbias;    // optional [B * nblk][3 * H * dh] column sums of dq | dk | dv (fast path)
  const char* dout; int64_t dout_ld;
  char* dq; int64_t dq_ld;
  char* dk; int64_t dk_ld;
  char* dv; int64_t dv_ld;
  const float* rope_cos; const float* rope_sin; int rope_q, rope_k;
  int rope_fast;  // bf16 backward: RoPE^T angles recomputed with v_sin / v_cos instead of the tables
  int B, T, H, dh;
  float scale;
  uint32_t thresh; float inv_keep; uint64_t seed;
};
}  // namespace nstl

namespace {

using nstl::AttnParams;
constexpr int DH = 64;
constexpr float LOG2E = 1.4426950408889634f;

// nt threads per workgroup, lds bytes of dynamic LDS (raised past the 64 KB default where needed)
template <typename K, typename... X>
int launch(K kern, dim3 grid, size_t lds, hipStream_t st, const AttnParams& p, const char* what, int nt, X... extra) {
  hipError_t e = hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (e != hipSuccess) return nstl::fail((int)e, "%s: LDS request %zu: %s", what, lds, hipGetErrorString(e));
  hipLaunchKernelGGL(kern, grid, dim3(nt), lds, st, p, extra...);
  NSTL_LAUNCH_CHECK(what);
  return 0;
}

// 2^x as one v_exp_f32 (exp2f adds a denormal-range fix-up: 4 more vector
// instructions per call; every argument here is <= 0 and a probability below
// 2^-126 is 0 either way)
NSTL_DEV float fast_exp2(float x) { return __builtin_amdgcn_exp2f(x); }

template <int N>
NSTL_DEV void vmcnt_wait() {
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}

// The 128-byte-row (bf16) K / V / Q / dO images of both files: 16-byte chunk c
// of row r at c ^ att_x(r).  They are read both ways: by rows (ds_read_b128, 16
// rows at one chunk per lane group) and transposed (ds_read_b64_tr_b16, 8 rows x
// 32 bytes per 32-lane group).  ImgK<128>'s x = (r >> 1) & 7 serves the row reads
// but puts rows r and r + 2 of a transposed read on the same banks (2 LDS cycles
// per 32-lane group instead of 1: the backward's largest bank-conflict term).
// This x -- row bit 1 to chunk bit 2, row bit 2 to chunk bit 1 -- is
// conflict-free for both (checked for every read pattern of the kernels by a
// bank simulation of the ds_read_b128 / ds_read_b64_tr_b16 lane groups).
// 256-byte rows (f32) keep ImgK<256>.
NSTL_DEV int att_x(int row) { return (((row >> 2) & 1) << 1) | (((row >> 1) & 1) << 2); }
template <int RB> struct ImgAtt {
  static NSTL_DEV int off(int row, int byte) {
    const int chunk = byte >> 4;
    const int x = RB == 128 ? att_x(row) : (row & 15);
    return row * RB + (((chunk ^ x) << 4) | (byte & 15));
  }
};

// one wave instruction of LDS-DMA: 16 bytes per lane, 1 KB = 8 rows of an
// ImgAtt<128> image (the caller applies the swizzle to the per-lane source chunk)
NSTL_DEV void dma1k(const char* src, char* dst) {
  __builtin_amdgcn_global_load_lds((const void __attribute__((address_space(1)))*)src,
                                   (void __attribute__((address_space(3)))*)dst, 16, 0, 0);
}

// ImgAtt<128> fragment reads as inline asm (bf16): with a prefetch DMA in flight
// into another buffer the compiler would put vmcnt(0) in front of its own LDS
// reads (it cannot tell the images apart), draining the prefetch; the caller
// orders them with lgkm_fence() before the MFMAs.
NSTL_DEV uint32_t lds_addr(const char* p) { return (uint32_t)(uintptr_t)(const __attribute__((address_space(3))) char*)p; }
typedef int i32x4a __attribute__((ext_vector_type(4)));
typedef int i32x2a __attribute__((ext_vector_type(2)));
// fragment (row, elements r .. r + 7)
NSTL_DEV void asm_row128(bf16x8& f, const char* img, int row, int r) {
  i32x4a v;
  asm volatile("ds_read_b128 %0, %1" : "=v"(v) : "v"(lds_addr(img + ImgAtt<128>::off(row, r * 2))));
  f = __builtin_bit_cast(bf16x8, v);
}
// column col16 + (lane & 15) of an image whose rows are the reduction index, rows
// r0 + 4g + 0..3 then r0 + 16 + 4g + 0..3 (acc_frag's order): two gfx950 transpose reads
NSTL_DEV void asm_col2_128(bf16x8& f, const char* img, int col16, int r0, int lane) {
  const int g = lane >> 4, q = (lane & 15) >> 2, pp = lane & 3;
  const int byte = (col16 + 4 * pp) * 2;
  i32x2a v0, v1;
  asm volatile("ds_read_b64_tr_b16 %0, %1" : "=v"(v0) : "v"(lds_addr(img + ImgAtt<128>::off(r0 + 4 * g + q, byte))));
  asm volatile("ds_read_b64_tr_b16 %0, %1" : "=v"(v1) : "v"(lds_addr(img + ImgAtt<128>::off(r0 + 16 + 4 * g + q, byte))));
  const bf16x4 b0 = __builtin_bit_cast(bf16x4, v0), b1 = __builtin_bit_cast(bf16x4, v1);
  f = (bf16x8){b0[0], b0[1], b0[2], b0[3], b1[0], b1[1], b1[2], b1[3]};
}
NSTL_DEV void lgkm_fence() {
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_sched_barrier(0);
}

// dropout element index: query-major, so the key pair (k, k+1) of one query
// shares a hash (the MFMA kernels hold 4 consecutive keys of a query per lane)
NSTL_DEV uint64_t drop_idx(int bh, int T, int q, int k) { return ((uint64_t)bh * T + q) * T + k; }

// Stored keep bits (MFMA paths): one 64-bit word per (query tile qt, key tile kt,
// key % 4) of a head, bit 16 * ((key % 16) / 4) + query % 16 -- the ballot of
// one score register r over a wave in the forward / dQ layout (lane 16g + c:
// query c, key 4g + r).  A head's words are [qt][kt][4] with nt = ceil(T / 16)
// tiles a side (T*T/64 of them for T % 16 == 0; the streaming kernels' ragged T:
// bits of queries / keys past T are 0).
NSTL_DEV int64_t mask_word(int bh, int nt, int qt, int kt, int r) {
  return (((int64_t)bh * nt + qt) * nt + kt) * 4 + r;
}
NSTL_DEV uint64_t shfl64(uint64_t v, int src) {
  const uint32_t lo = __shfl((uint32_t)v, src), hi = __shfl((uint32_t)(v >> 32), src);
  return ((uint64_t)hi << 32) | lo;
}
NSTL_DEV uint64_t readlane64(uint64_t v, int src) {
  const uint32_t lo = __builtin_amdgcn_readlane((uint32_t)v, src);
  const uint32_t hi = __builtin_amdgcn_readlane((uint32_t)(v >> 32), src);
  return ((uint64_t)hi << 32) | lo;
}

// ---------------------------------------------------------------------------
// Register-operand layout.  Scores are computed TRANSPOSED where the next
// product reduces over them: mma16(acc, X, Y) gives lane (g, c = lane & 15)
// the elements (row 4g + r, column c), so with X = keys and Y = queries a lane
// owns keys 16kt + 4g + r of ITS query c -- exactly what it must supply as the
// A operand (row c) of a product that sums over keys.  Two score registers
// (tiles 2j, 2j+1) form one A fragment whose 8 reduction slots are the keys
// {32j + 4g + 0..3, 32j + 16 + 4g + 0..3}; the B operand is read from its LDS
// image in that same order (frag_col2 / asm_col2_128), so P / dS never go
// through LDS.
template <typename T> NSTL_DEV typename FragT<T>::type acc_frag(const f32x4& a, const f32x4& b);
template <> NSTL_DEV bf16x8 acc_frag<bf16>(const f32x4& a, const f32x4& b) {
  return (bf16x8){(bf16)a[0], (bf16)a[1], (bf16)a[2], (bf16)a[3], (bf16)b[0], (bf16)b[1], (bf16)b[2], (bf16)b[3]};
}
template <> NSTL_DEV f32x8 acc_frag<float>(const f32x4& a, const f32x4& b) {
  return (f32x8){a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]};
}

// A wave's 16 x 64 result tile (lane: rows 4g+r, column dt*16 + (lane&15)) to
// global memory through the wave's LDS scratch: element writes into a dense
// [16][64] image, then 16-byte row chunks (2-byte scattered stores write
// 32-byte pieces of 4 rows per instruction).
template <typename T>
NSTL_DEV void store_tile16x64(const float (&v)[4][4], char* scr, char* gbase, int64_t ld_elems, int lane) {
  constexpr int ESZ = (int)sizeof(T), RB = DH * ESZ, CPR = RB / 16;
  const int g = lane >> 4;
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) *(T*)(scr + (4 * g + r) * RB + (dt * 16 + (lane & 15)) * ESZ) = from_f32<T>(v[dt][r]);
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
  for (int c = lane; c < 16 * CPR; c += 64) {
    const int row = c / CPR, ch = c % CPR;
    *(uint4*)(gbase + (int64_t)row * ld_elems * ESZ + ch * 16) = *(const uint4*)(scr + row * RB + ch * 16);
  }
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
}
// The same with a row limit (a wave whose 16 rows straddle the end of a ragged
// head): rows >= nrows are staged but not stored.
template <typename T>
NSTL_DEV void store_tile16x64(const float (&v)[4][4], char* scr, char* gbase, int64_t ld_elems, int lane, int nrows) {
  constexpr int ESZ = (int)sizeof(T), RB = DH * ESZ, CPR = RB / 16;
  const int g = lane >> 4;
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) *(T*)(scr + (4 * g + r) * RB + (dt * 16 + (lane & 15)) * ESZ) = from_f32<T>(v[dt][r]);
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
  for (int c = lane; c < 16 * CPR; c += 64) {
    const int row = c / CPR, ch = c % CPR;
    if (row < nrows)
      *(uint4*)(gbase + (int64_t)row * ld_elems * ESZ + ch * 16) = *(const uint4*)(scr + row * RB + ch * 16);
  }
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
}

// RoPE^T: rotate (row t, col d) accumulator elements back by -theta
// partner element of a RoPE pair: lane c <-> c ^ 1 (DPP quad_perm [1,0,3,2], no LDS)
NSTL_DEV float swap_pair(float v) {
  return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0xB1, 0xF, 0xF, false));
}
// RoPE^T over a lane's 16 x 64 tile elements v[dt][r] = (row0 + r, d = 16 dt + c):
// the 32 table reads are issued together (rope_tab), the pair swaps are DPP
// moves (the per-element form waited on one ds_bpermute and two table reads at
// a time).  Tables [T][RS] with row stride RS floats (32 in global memory, 36
// in the fused kernel's LDS copy: the rows 4g + r of a wave's four lane groups
// then fall on distinct banks).  The sin table comes out with the lane's sign
// folded in (ts = -sin on odd lanes), so every element is x cos + partner ts:
// one multiply and one FMA.  rope_apply needs every lane of the wave active.
template <int RS>
NSTL_DEV void rope_tab(float (&tc)[4][4], float (&ts)[4][4], int row0, int c, const float* cs, const float* sn,
                       int i0 = 0) {
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) {
      const int i = (row0 + r) * RS + i0 + dt * 8 + (c >> 1);
      tc[dt][r] = cs[i];
      ts[dt][r] = (c & 1) ? -sn[i] : sn[i];
    }
}
// rope_tab with the table row clamped to row_last (a ragged head's last wave: its
// rows past the head hold zeros, but the tables end at row T - 1)
template <int RS>
NSTL_DEV void rope_tab_clamped(float (&tc)[4][4], float (&ts)[4][4], int row0, int c, const float* cs, const float* sn,
                               int row_last, int i0 = 0) {
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) {
      const int i = min(row0 + r, row_last) * RS + i0 + dt * 8 + (c >> 1);
      tc[dt][r] = cs[i];
      ts[dt][r] = (c & 1) ? -sn[i] : sn[i];
    }
}
NSTL_DEV void rope_apply(float (&v)[4][4], const float (&tc)[4][4], const float (&ts)[4][4]) {
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) {
      const float x = v[dt][r], partner = swap_pair(x);
      v[dt][r] = fmaf(partner, ts[dt][r], x * tc[dt][r]);
    }
}
// The same cos / sin values recomputed: angle = float(t) * inv_freq_i as
// rotation_tables() forms it (f32 product; inv_freq by the hardware exp), then
// the hardware sin / cos (v_sin_f32 / v_cos_f32 on angle / 2pi).  Against the
// f32 tables the error is ~1e-6 absolute, far below the bf16 rounding of the
// dQ / dK it rotates.
// The angle goes to v_sin / v_cos in revolutions, t * (inv_freq / 2pi), with the
// lane's sign folded into the factor (sin is odd, cos even): one multiply per
// angle instead of three (angle, 1/2pi for each of sin and cos, the sign).
// DHT: the head width (the divisor of the frequency exponent); i0: the first pair
// index of the tile (32 for columns 64..127 of a 128-wide head).
template <int DHT = DH>
NSTL_DEV void rope_tab_fast(float (&tc)[4][4], float (&ts)[4][4], int row0, int c, int i0 = 0) {
  const float sgn_rev = ((c & 1) ? -1.f : 1.f) * 0.15915494309189535f;  // +-1/(2pi)
#pragma unroll
  for (int dt = 0; dt < 4; ++dt) {
    const float two_i = (float)(2 * (i0 + dt * 8 + (c >> 1)));
    const float inv_freq = __expf(-9.21034049987793f * two_i / (float)DHT);  // f32(ln 10000)
    const float f = inv_freq * sgn_rev;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float a = (float)(row0 + r) * f;
      ts[dt][r] = __builtin_amdgcn_sinf(a);
      tc[dt][r] = __builtin_amdgcn_cosf(a);
    }
  }
}
// fast: the angles recomputed (rope_tab_fast) instead of per-element table reads
// from global memory (16 dependent L2 round trips per wave at the end of the split
// kernels; bf16 only -- the f32 parity mode keeps the tables' exact values)
// The tile is columns 64 hf .. 64 hf + 63 of a DHT-wide head: pair indices
// 32 hf + 8 dt + (c >> 1) of the head's DHT / 2, table row stride DHT / 2.
template <int DHT = DH>
NSTL_DEV void rope_back_tile(float (&v)[4][4], int row0, int c, const float* cs, const float* sn, bool fast = false,
                             int hf = 0) {
  float tc[4][4], ts[4][4];
  if (fast) rope_tab_fast<DHT>(tc, ts, row0, c, 32 * hf);
  else rope_tab<DHT / 2>(tc, ts, row0, c, cs, sn, 32 * hf);
  rope_apply(v, tc, ts);
}
// ... with the table row clamped to row_last (rope_tab_clamped)
template <int DHT = DH>
NSTL_DEV void rope_back_tile_clamped(float (&v)[4][4], int row0, int c, const float* cs, const float* sn, bool fast,
                                     int row_last, int hf = 0) {
  float tc[4][4], ts[4][4];
  if (fast) rope_tab_fast<DHT>(tc, ts, row0, c, 32 * hf);
  else rope_tab_clamped<DHT / 2>(tc, ts, row0, c, cs, sn, row_last, 32 * hf);
  rope_apply(v, tc, ts);
}

// Bias gradients fused into the backward stores: column sums of a wave's stored
// 16 x 64 tile (rounded to T, as colsum() of the stored tensor would see it) go
// to red[w][64]; the LAST wave to finish (an LDS arrival counter, no barrier,
// so early waves leave at once) adds the block's waves in fixed order and
// writes one partial row: deterministic, no float atomics.
template <typename T>
NSTL_DEV void wave_colsum16x64(const float (&v)[4][4], float* red, int w, int lane) {
  if constexpr (sizeof(T) == 2) {
    // bf16: one v_mfma_f32_16x16x16_bf16 per 16 columns, ones x tile: the lane's
    // four rows 4g + r of column 16 dt + c are exactly its B operand, and every
    // result row is the column sum of the stored (bf16) values -- lane c of lane
    // group 0 holds column 16 dt + c, no cross-lane reduction
    const s16x4 ones = __builtin_bit_cast(s16x4, (bf16x4){(bf16)1.f, (bf16)1.f, (bf16)1.f, (bf16)1.f});
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) {
      const bf16x4 x = {(bf16)v[dt][0], (bf16)v[dt][1], (bf16)v[dt][2], (bf16)v[dt][3]};
      const f32x4 d = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(ones, __builtin_bit_cast(s16x4, x),
                                                                (f32x4){0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
      if (lane < 16) red[w * 64 + dt * 16 + lane] = d[0];
    }
    return;
  }
#pragma unroll
  for (int dt = 0; dt < 4; ++dt) {
    float cs = 0.f;
#pragma unroll
    for (int r = 0; r < 4; ++r) cs += to_f32(from_f32<T>(v[dt][r]));
    cs = sum_xor16(cs);
    cs = sum_xor32(cs);
    if (lane < 16) red[w * 64 + dt * 16 + lane] = cs;
  }
}
NSTL_DEV bool last_to_arrive(unsigned* cnt, int nw, int lane) {
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // this wave's red[] writes are done
  unsigned old = 0;
  if (lane == 0) old = atomicAdd(cnt, 1u);
  return __shfl(old, 0) == (unsigned)(nw - 1);
}
NSTL_DEV void wave_sum_out(const float* red, int nw, float* out, int lane) {
  float cs = 0.f;
  for (int k = 0; k < nw; ++k) cs += red[k * 64 + lane];
  out[lane] = cs;
}

// ---------------------------------------------------------------------------
// The epilogue helpers for a head of RUNTIME width (the streaming kernels' head
// widths other than 64 and 128: any multiple of 8).  A result tile is still 16 x 64
// in registers and in the staging image; ncols = min(64, dh - 64 hf) of its columns
// exist.  Nothing is stored to, summed into or read from (RoPE tables) a column at or
// past ncols: those belong to the next head, the next operand or nobody.
//
// store_tile16x64 with a column limit as well: 16-byte chunks at or past ncols (a
// multiple of 8) and rows >= nrows are staged but not stored.
template <typename T>
NSTL_DEV void store_tile16xw(const float (&v)[4][4], char* scr, char* gbase, int64_t ld_elems, int lane, int nrows,
                             int ncols) {
  constexpr int ESZ = (int)sizeof(T), RB = DH * ESZ, CPR = RB / 16;
  const int g = lane >> 4;
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) *(T*)(scr + (4 * g + r) * RB + (dt * 16 + (lane & 15)) * ESZ) = from_f32<T>(v[dt][r]);
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
  for (int c = lane; c < 16 * CPR; c += 64) {
    const int row = c / CPR, ch = c % CPR;
    if (row < nrows && ch * (16 / ESZ) < ncols)
      *(uint4*)(gbase + (int64_t)row * ld_elems * ESZ + ch * 16) = *(const uint4*)(scr + row * RB + ch * 16);
  }
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
}
// rope_tab_clamped for tables of row stride dh / 2: the pair index is clamped to the
// head's last pair, so a lane whose column is absent reads (and then rotates garbage
// by) an angle inside its own table row; its result is never stored
NSTL_DEV void rope_tab_w(float (&tc)[4][4], float (&ts)[4][4], int row0, int c, const float* cs, const float* sn,
                         int row_last, int i0, int dh) {
  const int rs = dh >> 1;
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) {
      const int i = min(row0 + r, row_last) * rs + min(i0 + dt * 8 + (c >> 1), rs - 1);
      tc[dt][r] = cs[i];
      ts[dt][r] = (c & 1) ? -sn[i] : sn[i];
    }
}
// rope_tab_fast with the head width (the divisor of the frequency exponent) at run time
NSTL_DEV void rope_tab_fast_w(float (&tc)[4][4], float (&ts)[4][4], int row0, int c, int i0, int dh) {
  const float sgn_rev = ((c & 1) ? -1.f : 1.f) * 0.15915494309189535f;  // +-1/(2pi)
  const float fdh = (float)dh;
#pragma unroll
  for (int dt = 0; dt < 4; ++dt) {
    const float two_i = (float)(2 * (i0 + dt * 8 + (c >> 1)));
    const float inv_freq = __expf(-9.21034049987793f * two_i / fdh);  // f32(ln 10000)
    const float f = inv_freq * sgn_rev;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float a = (float)(row0 + r) * f;
      ts[dt][r] = __builtin_amdgcn_sinf(a);
      tc[dt][r] = __builtin_amdgcn_cosf(a);
    }
  }
}
// rope_back_tile_clamped for columns 64 hf .. of a dh-wide head (pairs are adjacent
// columns, so a pair is wholly present or wholly absent)
NSTL_DEV void rope_back_tile_w(float (&v)[4][4], int row0, int c, const float* cs, const float* sn, bool fast,
                               int row_last, int hf, int dh) {
  float tc[4][4], ts[4][4];
  if (fast) rope_tab_fast_w(tc, ts, row0, c, 32 * hf, dh);
  else rope_tab_w(tc, ts, row0, c, cs, sn, row_last, 32 * hf, dh);
  rope_apply(v, tc, ts);
}
// wave_sum_out for the first ncols columns only
NSTL_DEV void wave_sum_out_w(const float* red, int nw, float* out, int lane, int ncols) {
  float cs = 0.f;
  for (int k = 0; k < nw; ++k) cs += red[k * 64 + lane];
  if (lane < ncols) out[lane] = cs;
}

}  // namespace
