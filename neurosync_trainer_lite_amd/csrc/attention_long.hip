// Streaming MFMA attention (bf16): the shapes past the one-shot kernels of
// attention.hip, whose score rows live in registers and whose K / V of a whole head
// live in LDS.  Which calls come here: the table above nstl_attn_args in nstl.h
// (decided by nstl::attn_route, attention_route.h).
//
// The head width is the template parameter DHT of the three kernels (64 or 128).  A
// 128-wide head is two 64-column halves: every K / V / Q / dO tile is two
// 128-byte-row images (columns 0..63 and 64..127) with the swizzle, the DMA pieces
// and the reads of the 64-wide case; scores and dP sum four 32-wide k-chunks instead
// of two; O, dQ, dK and dV are two groups of four 16-column accumulator tiles, stored,
// rotated (RoPE^T pair index 32 half + ...) and column-summed one half at a time.  The
// <64, ...> instantiations are the kernels as they were before DHT.
//
// Every other width dh % 8 == 0 below 128 runs the ANY instantiations: DHT is then
// the image class (64: dh <= 56 in one image, 128:
// 72 <= dh <= 120 in two) and the width is p.dh.  Columns at and past dh are absent:
// their DMA pieces are fetched from piece 0 of the same head's row (TileDmaW), the
// wave's own-row fragments are exact zeros there (row_frag_w), nothing is stored,
// summed or looked up (RoPE tables) for them (attention_dev.h: store_tile16xw,
// wave_sum_out_w, rope_tab_w).  HI (compile time) says whether the upper 32 columns of
// the last image hold anything; without it that k-chunk and its two accumulator tiles
// are not compiled in.  It is not a run-time branch because the inline-asm LDS reads
// must reach their lgkm_fence() in straight-line code: a read in a conditional block
// had its result register moved at the merge, before the data had landed.
//
// Here nothing of size T x T or T per lane is held.  Every kernel owns a block of
// 128 rows of one (batch, head) -- 8 waves, 16 rows each, the wave's own rows
// loaded from global memory straight into MFMA fragments -- and walks the other
// sequence index in tiles of 64 rows that go through LDS by LDS-DMA, two
// buffers: tile t+1 is in flight while tile t is computed.
//   forward : 128 queries; K / V tiles; S^T = K Q^T per tile, online softmax
//             (running max and running sum per query in f32, O accumulators
//             rescaled when the max moves), O += V^T P^T from the score registers.
//   dQ      : 128 queries; K / V tiles; P recomputed from the saved LSE;
//             also writes D = rowsum(dO * O).
//   dK / dV : 128 keys; Q / dO tiles; accumulators in registers over the sweep.
// No atomics on global memory and no cross-workgroup sums: every output element
// has one writer and a fixed summation order.
// Conventions (scale, LSE, dropout on the normalised probabilities, the
// nstl_keep(seed, drop_idx) stream, RoPE^T on dq / dk, bias partial rows) are
// those of attention.hip, so the paths are interchangeable: the parameter block
// (filled by attention.hip's entry points), the operand image and its reads, the
// keep-bit words, the fragment order and the epilogue helpers (tile store, RoPE^T,
// bias partials) are the one definition of each in attention_dev.h.
//
// Tails: T % 32 == 0, so a wave's 16 rows are all in range or all out, and a
// tile holds 64 or (the last one) 32 valid rows.  The backward kernels only
// touch a tile's valid 32-row chunks.  The forward computes the whole tile: its
// DMA clamps the row index to T - 1 (nothing is read past the head's T rows) and
// the out-of-range scores are set to -inf, i.e. probability exactly 0.
//
// Ragged T is the template parameter RAG of the three kernels (the T % 32 == 0
// instantiations are unchanged by it).  A wave whose 16 rows straddle T loads its
// rows past the head from row T - 1 (finite, inside the head), makes their
// contribution exactly zero (dQ: lse = +inf, D = 0; dK / dV: P selected to 0) and
// stores nothing for them; a tile's 32-row chunks count while they hold one valid
// row; the dK / dV kernel's LSE / D rows in LDS are padded to whole tiles with
// +inf / 0; keep bits of rows and keys past T are stored as 0; the keep-bit words
// have ceil(T / 16) tiles a side.
#include "../../include/nstl.h"
#include "attention_dev.h"
#include "attention_route.h"
#include "common.h"
#include "status.h"

namespace {

constexpr int LNT = 512, NW = LNT / 64, ROWS = 16 * NW;  // 8 waves, 128 rows per workgroup
constexpr int KT = 64;                                    // streamed rows per tile
constexpr int TILE_B = KT * 64 * 2;                       // one 64-column image: 8 KB
// A DHT-wide operand tile is NH = DHT / 64 images side by side (columns 64 hf ..
// 64 hf + 63 in image hf), each an ImgAtt<128> of its own; a buffer holds two
// operands: [A images][B images].
template <int DHT> struct Geo {
  static_assert(DHT == 64 || DHT == 128, "head widths of the streaming kernels");
  static constexpr int NH = DHT / 64, OP_B = NH * TILE_B, BUF_B = 2 * OP_B;
  // waves per SIMD the forward and dQ kernels are compiled for
  static constexpr int OCC = DHT == 64 ? 4 : 2;
};

// f(half 0), then f(half 1) of a 128-wide head, the half a compile-time constant (the
// backward epilogues).  In the backward tile loops the second half is instead an
// `if constexpr (NH == 2)` block behind the 64-wide statements: as a loop over halves
// or through this helper the 64-wide kernels came out with other register counts
// (DESIGN.md section 4), as written they have the counts they had before DHT.
template <int V> struct HalfC { static constexpr int value = V; };
template <int NH, typename F>
NSTL_DEV void for_halves(F&& f) {
  f(HalfC<0>{});
  if constexpr (NH == 2) f(HalfC<1>{});
}

NSTL_DEV f32x4 asm_f32x4(const float* p) {
  f32x4 v;
  asm volatile("ds_read_b128 %0, %1" : "=v"(v) : "v"(lds_addr((const char*)p)));
  return v;
}
// This wave's 1 KB pieces (rows 8w .. 8w + 7 of every image) of tile t of two operands
// into buffer buf: A's images at the buffer's start, B's behind them.  The source row
// is clamped
// to the head's last row (a partial last tile re-reads row T - 1: finite data, never
// past the head).
template <int DHT> struct TileDma {
  static constexpr int NH = Geo<DHT>::NH, OP_B = Geo<DHT>::OP_B, BUF_B = Geo<DHT>::BUF_B;
  const char* a; int64_t a_ldb;
  const char* b; int64_t b_ldb;
  int lrow, lc, T;
  NSTL_DEV void issue(char* smem, int t, int buf, int w) const {
    const int row = min(t * KT + lrow, T - 1);
#pragma unroll
    for (int hf = 0; hf < NH; ++hf)
      dma1k(a + row * a_ldb + hf * 128 + lc * 16, smem + buf * BUF_B + hf * TILE_B + w * 1024);
#pragma unroll
    for (int hf = 0; hf < NH; ++hf)
      dma1k(b + row * b_ldb + hf * 128 + lc * 16, smem + buf * BUF_B + OP_B + hf * TILE_B + w * 1024);
  }
};
template <int DHT>
NSTL_DEV TileDma<DHT> tile_dma(const char* a, int64_t a_ld, const char* b, int64_t b_ld, int64_t tok0, int h, int T,
                               int w, int lane) {
  TileDma<DHT> d;
  d.a = a + (tok0 * a_ld + h * DHT) * 2; d.a_ldb = a_ld * 2;
  d.b = b + (tok0 * b_ld + h * DHT) * 2; d.b_ldb = b_ld * 2;
  d.lrow = w * 8 + (lane >> 3);
  d.lc = (lane & 7) ^ att_x(d.lrow);
  d.T = T;
  return d;
}
// The same for a head of runtime width dh (a multiple of 8, 64 (NH - 1) < dh < 64 NH):
// the lane's 16-byte source piece of image hf is columns 64 hf + 8 lc .. + 7, and a
// piece at or past dh is fetched from piece 0 of the same row of the same head
// instead -- no byte outside row * ld + h * dh + [0, dh) is read, and the absent
// columns of an image hold finite data (a copy of columns 0 .. 7).
template <int DHT> struct TileDmaW {
  static constexpr int NH = Geo<DHT>::NH, OP_B = Geo<DHT>::OP_B, BUF_B = Geo<DHT>::BUF_B;
  const char* a; int64_t a_ldb;
  const char* b; int64_t b_ldb;
  int lrow, T, off[NH];  // off[hf]: byte offset of the lane's piece in the head's row
  NSTL_DEV void issue(char* smem, int t, int buf, int w) const {
    const int row = min(t * KT + lrow, T - 1);
#pragma unroll
    for (int hf = 0; hf < NH; ++hf) dma1k(a + row * a_ldb + off[hf], smem + buf * BUF_B + hf * TILE_B + w * 1024);
#pragma unroll
    for (int hf = 0; hf < NH; ++hf)
      dma1k(b + row * b_ldb + off[hf], smem + buf * BUF_B + OP_B + hf * TILE_B + w * 1024);
  }
};
template <int DHT>
NSTL_DEV TileDmaW<DHT> tile_dma_w(const char* a, int64_t a_ld, const char* b, int64_t b_ld, int64_t tok0, int h, int dh,
                                  int T, int w, int lane) {
  TileDmaW<DHT> d;
  d.a = a + (tok0 * a_ld + h * dh) * 2; d.a_ldb = a_ld * 2;
  d.b = b + (tok0 * b_ld + h * dh) * 2; d.b_ldb = b_ld * 2;
  d.lrow = w * 8 + (lane >> 3);
  const int lc = (lane & 7) ^ att_x(d.lrow);
#pragma unroll
  for (int hf = 0; hf < Geo<DHT>::NH; ++hf) d.off[hf] = 64 * hf + 8 * lc < dh ? (64 * hf + 8 * lc) * 2 : 0;
  d.T = T;
  return d;
}
// ANY selects the runtime-width form of a kernel's operand stream and head width
template <int DHT, bool ANY> struct DmaSel { using type = TileDma<DHT>; };
template <int DHT> struct DmaSel<DHT, true> { using type = TileDmaW<DHT>; };
template <int DHT, bool ANY>
NSTL_DEV typename DmaSel<DHT, ANY>::type tile_dma_sel(const char* a, int64_t a_ld, const char* b, int64_t b_ld,
                                                      int64_t tok0, int h, int dh, int T, int w, int lane) {
  if constexpr (ANY) return tile_dma_w<DHT>(a, a_ld, b, b_ld, tok0, h, dh, T, w, lane);
  else return tile_dma<DHT>(a, a_ld, b, b_ld, tok0, h, T, w, lane);
}
template <int DHT, bool ANY>
NSTL_DEV int head_width(const AttnParams& p) {
  if constexpr (ANY) return p.dh;
  else return DHT;
}
// own-row fragment u of a head of runtime width dh: elements 32 u + 8 g .. + 7 of the
// row, an exact zero (and no read) where that piece is at or past dh
NSTL_DEV bf16x8 row_frag_w(const bf16* row, int u, int g, int dh) {
  bf16x8 z = {};
  return 32 * u + 8 * g < dh ? *(const bf16x8*)(row + 32 * u + 8 * g) : z;
}

// ---------------------------------------------------------------------------
// Forward.  s[kt][r] = score(query q0 + c, key 64 t + 16 kt + 4g + r): a lane holds
// 16 scores of ITS query per tile, the rest are in the lanes c + 16 g' (two
// permlane swaps for the tile maximum).  The running sum stays a per-lane partial
// (the four lanes of a query rescale by the same factor) and is reduced once at
// the end.  LDS: 2 x (K | V) = 32 KB (head_dim 64) / 64 KB (128).
template <int DHT, bool DROP, bool RAG = false, bool ANY = false, bool HI = true>
__global__ __launch_bounds__(LNT, Geo<DHT>::OCC) void attn_fwd_long_kernel(AttnParams p) {
  constexpr int NH = Geo<DHT>::NH, OP_B = Geo<DHT>::OP_B, BUF_B = Geo<DHT>::BUF_B;
  static_assert((!ANY || RAG) && (ANY || HI), "the runtime-width kernels are the ragged ones");
  const int dh = head_width<DHT, ANY>(p);  // ANY: 64 (NH - 1) < dh < 64 NH, dh % 8 == 0
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int T_ = p.T, nt16 = (T_ + 15) / 16, ntile = (T_ + KT - 1) / KT;
  const int tid = threadIdx.x, lane = tid & 63, g = lane >> 4, c = lane & 15;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int bh = blockIdx.y, b = bh / p.H, h = bh % p.H;
  const int64_t tok0 = (int64_t)b * T_;
  const int q0 = blockIdx.x * ROWS + w * 16;
  const bool act = q0 < T_;
  const auto dma = tile_dma_sel<DHT, ANY>(p.k, p.k_ld, p.v, p.v_ld, tok0, h, dh, T_, w, lane);
  dma.issue(smem, 0, 0, w);
  // RAG: a wave that straddles T reads its rows past the head from row T - 1 and
  // stores nothing for them
  const int qr = RAG ? min(q0 + c, T_ - 1) : q0 + c;
  const bool qok = !RAG || q0 + c < T_;
  bf16x8 fq[2 * NH] = {};  // elements 32 u + 8g .. + 7 of the query's row, u = 0 .. 2 NH - 1
  if (act) {
    const bf16* qrow = (const bf16*)p.q + (tok0 + qr) * p.q_ld + h * dh;
#pragma unroll
    for (int u = 0; u < 2 * NH; ++u) {
      if constexpr (ANY) fq[u] = row_frag_w(qrow, u, g, dh);
      else fq[u] = *(const bf16x8*)(qrow + 32 * u + 8 * g);
    }
  }
  // ANY: 32-column k-chunks 0 .. 2 NH - 2 hold at least one present piece, the last one
  // only if dh > DHT - 32, which is HI; with it go accumulator tiles 2 and 3 of the last
  // half.  Without HI their LDS reads and MFMAs are not compiled in.
  constexpr bool last_kc = !ANY || HI;
  const float c2 = p.scale * LOG2E;
  float m = -INFINITY, lsum = 0.f;
  f32x4 o[4 * NH];
#pragma unroll
  for (int dt = 0; dt < 4 * NH; ++dt) o[dt] = (f32x4){0.f, 0.f, 0.f, 0.f};
  const uint32_t st = nstl_seed_term(p.seed);
  for (int t = 0; t < ntile; ++t) {
    vmcnt_wait<0>();          // this wave's piece of tile t (and its stores of tile t-1)
    __syncthreads();   // tile t has landed; every wave is done with tile t-1's buffer
    if (t + 1 < ntile) dma.issue(smem, t + 1, (t + 1) & 1, w);
    if (!act) continue;
    const char* Kimg = smem + (t & 1) * BUF_B;
    const char* Vimg = Kimg + OP_B;
    const int kb = t * KT;
    f32x4 s[4];
#pragma unroll
    for (int kt = 0; kt < 4; kt += 2) {
      bf16x8 fk[4 * NH];
#pragma unroll
      for (int hf = 0; hf < NH; ++hf)
#pragma unroll
        for (int u = 0; u < 4; ++u)
          if (!ANY || 2 * hf + (u & 1) < 2 * NH - 1 || last_kc)
            asm_row128(fk[4 * hf + u], Kimg + hf * TILE_B, (kt + (u >> 1)) * 16 + c, 32 * (u & 1) + 8 * g);
      lgkm_fence();
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        s[kt + u] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int hf = 0; hf < NH; ++hf) {
          mma16(s[kt + u], fk[4 * hf + 2 * u], fq[2 * hf]);
          if (!ANY || hf < NH - 1 || last_kc) mma16(s[kt + u], fk[4 * hf + 2 * u + 1], fq[2 * hf + 1]);
        }
      }
    }
    if (kb + KT > T_) {  // the partial last tile: keys past T get probability 0
#pragma unroll
      for (int kt = 0; kt < 4; ++kt)
#pragma unroll
        for (int r = 0; r < 4; ++r)
          if (kb + kt * 16 + 4 * g + r >= T_) s[kt][r] = -INFINITY;
    }
    float mt = -INFINITY;
#pragma unroll
    for (int kt = 0; kt < 4; ++kt) mt = fmaxf(fmaxf(mt, fmaxf(fmaxf(s[kt][0], s[kt][1]), s[kt][2])), s[kt][3]);
    mt = max_xor16(mt);
    mt = max_xor32(mt);
    // every tile has a valid key (>= 32 of them unless RAG), so mn is finite; the first tile's factor is 2^-inf = 0
    const float mn = fmaxf(m, mt);
    const float alpha = fast_exp2((m - mn) * c2);
    m = mn;
    lsum *= alpha;
#pragma unroll
    for (int dt = 0; dt < 4 * NH; ++dt) o[dt] *= alpha;
    const float nmc = -mn * c2;
#pragma unroll
    for (int kt = 0; kt < 4; ++kt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float e = fast_exp2(fmaf(s[kt][r], c2, nmc));
        s[kt][r] = e;
        lsum += e;  // the row sum is taken over the undropped p
      }
    if constexpr (DROP) {
      // keys (r, r+1) of this lane's query share one hash; pair index of
      // drop_idx(bh, T, q, kb + 4g) (even): 32-bit, checked by the launcher.  Lane
      // kt * 4 + r collects the ballot of (kt, r): the tile's 16 keep words.
      uint32_t pair0;
      if (RAG && (T_ & 1)) pair0 = (uint32_t)(drop_idx(bh, T_, qr, kb + 4 * g) >> 1);
      else pair0 = ((uint32_t)bh * T_ + qr) * (uint32_t)(T_ >> 1) + (kb >> 1) + 2 * g;
      uint32_t hs[4][2];
#pragma unroll
      for (int kt = 0; kt < 4; ++kt) {
        hs[kt][0] = nstl_pair_hash32(st, pair0 + kt * 8);
        hs[kt][1] = nstl_pair_hash32(st, pair0 + kt * 8 + 1);
      }
      if constexpr (RAG) {
        // odd T: a query's row of element indices starts odd for every other query,
        // and its four keys are then the high half of pair0, pair0 + 1 and the low
        // half of pair0 + 2: the per-element definition nstl_keep(seed, drop_idx)
        if ((T_ & 1) && ((bh + qr) & 1)) {
#pragma unroll
          for (int kt = 0; kt < 4; ++kt) {
            const uint32_t h2 = nstl_pair_hash32(st, pair0 + kt * 8 + 2);
            hs[kt][0] = (hs[kt][0] >> 16) | (hs[kt][1] << 16);
            hs[kt][1] = (hs[kt][1] >> 16) | (h2 << 16);
          }
        }
      }
      uint32_t mlo = 0, mhi = 0;
#pragma unroll
      for (int kt = 0; kt < 4; ++kt) {
        const uint32_t h0 = hs[kt][0], h1 = hs[kt][1];
        const bool k[4] = {(h0 & 0xFFFFu) >= p.thresh, (h0 >> 16) >= p.thresh, (h1 & 0xFFFFu) >= p.thresh,
                           (h1 >> 16) >= p.thresh};
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          s[kt][r] = k[r] ? s[kt][r] : 0.f;  // 1/(1-p): in the normalisation
          const uint64_t bal = __builtin_amdgcn_ballot_w64(k[r]);
          mlo = nstl_writelane_i32((int)(uint32_t)bal, kt * 4 + r, (int)mlo);
          mhi = nstl_writelane_i32((int)(uint32_t)(bal >> 32), kt * 4 + r, (int)mhi);
        }
        __builtin_amdgcn_sched_barrier(0);
      }
      if constexpr (RAG) {
        // bits of queries / keys past T are stored as 0 (their p is 0 or unstored, so
        // only the words need it): lane L holds word (kt, r) = (L >> 2, L & 3), whose
        // bit 16 g + c is (key 16 kt + 4 g + r, query q0 + c)
        const int ng = min(4, max(0, (T_ - kb - 16 * (lane >> 2) - (lane & 3) + 3) >> 2));  // valid g
        const int nq = min(16, T_ - q0);
        uint64_t vm = ng >= 4 ? ~0ull : (1ull << (16 * ng)) - 1;
        vm &= ((1ull << nq) - 1) * 0x0001000100010001ull;
        mlo &= (uint32_t)vm;
        mhi &= (uint32_t)(vm >> 32);
      }
      // words of key tiles past T are not written (they would be another query tile's)
      if (p.mask && lane < 4 * min(4, nt16 - (kb >> 4)))
        p.mask[mask_word(bh, nt16, q0 >> 4, kb >> 4, 0) + lane] = ((uint64_t)mhi << 32) | mlo;
    }
    // O^T += V^T P^T over the tile's two 32-key chunks: o[dt][r] = O(query q0 + c, d = 16 dt + 4g + r)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const bf16x8 fp = acc_frag<bf16>(s[2 * j], s[2 * j + 1]);
#pragma unroll
      for (int hf = 0; hf < NH; ++hf) {
        bf16x8 fv[4];
#pragma unroll
        for (int dt = 0; dt < 4; ++dt)
          if (hf < NH - 1 || dt < 2 || last_kc) asm_col2_128(fv[dt], Vimg + hf * TILE_B, dt * 16, 32 * j, lane);
        lgkm_fence();
#pragma unroll
        for (int dt = 0; dt < 4; ++dt)
          if (hf < NH - 1 || dt < 2 || last_kc) mma16(o[4 * hf + dt], fv[dt], fp);
      }
    }
  }
  if (!act) return;
  float sum = sum_xor16(lsum);
  sum = sum_xor32(sum);
  const float inv = (DROP ? p.inv_keep : 1.f) * __builtin_amdgcn_rcpf(sum);
  if (!qok) return;
  bf16* orow = (bf16*)p.o + (tok0 + q0 + c) * p.o_ld + h * dh + 4 * g;
#pragma unroll
  for (int dt = 0; dt < 4 * NH; ++dt) {
    const f32x4 x = o[dt] * inv;
    // ANY: dh % 8 == 0, so the lane's four columns 16 dt + 4g .. + 3 are all present or all absent
    if (!ANY || 16 * dt + 4 * g < dh)
      *(bf16x4*)(orow + 16 * dt) = (bf16x4){(bf16)x[0], (bf16)x[1], (bf16)x[2], (bf16)x[3]};
  }
  if (g == 0) p.lse[(int64_t)bh * T_ + q0 + c] = m * p.scale + logf(sum);
}

// ---------------------------------------------------------------------------
// dQ.  Workgroup = (b, h, 128 queries); K / V tiles stream.  DM: dropout mode
// (0 none, 1 the forward's stored keep bits, 2 re-hashed).  LDS: 2 x (K | V) =
// 32 KB (the output staging reuses it after the sweep), bias partials, counter.
// (head_dim 128: 64 KB, and one bias partial array [NW][64] per 64-column half.)
template <int DHT> struct DqLds {
  static constexpr int RED_OFF = 2 * Geo<DHT>::BUF_B, ARR_OFF = RED_OFF + Geo<DHT>::NH * NW * 64 * 4;
  static constexpr size_t BYTES = ARR_OFF + 16;
};

template <int DHT, int DM, bool RAG = false, bool ANY = false, bool HI = true>
__global__ __launch_bounds__(LNT, Geo<DHT>::OCC) void attn_bwd_dq_long_kernel(AttnParams p) {
  constexpr int NH = Geo<DHT>::NH, OP_B = Geo<DHT>::OP_B, BUF_B = Geo<DHT>::BUF_B;
  static_assert((!ANY || RAG) && (ANY || HI), "the runtime-width kernels are the ragged ones");
  const int dh = head_width<DHT, ANY>(p);  // ANY: 64 (NH - 1) < dh < 64 NH, dh % 8 == 0
  constexpr bool last_kc = !ANY || HI;  // the last 32-column k-chunk (accumulator tiles 2, 3 of the last half) exists
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* red = (float*)(smem + DqLds<DHT>::RED_OFF);  // [NH][NW][64]
  unsigned* arrived = (unsigned*)(smem + DqLds<DHT>::ARR_OFF);
  const int T_ = p.T, nt16 = (T_ + 15) / 16, ntile = (T_ + KT - 1) / KT;
  const int tid = threadIdx.x, lane = tid & 63, g = lane >> 4, c = lane & 15;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int bh = blockIdx.y, b = bh / p.H, h = bh % p.H;
  const int64_t tok0 = (int64_t)b * T_;
  const int q0 = blockIdx.x * ROWS + w * 16;
  const bool act = q0 < T_;
  const auto dma = tile_dma_sel<DHT, ANY>(p.k, p.k_ld, p.v, p.v_ld, tok0, h, dh, T_, w, lane);
  dma.issue(smem, 0, 0, w);
  // stored keep bits of this wave's 16 queries against tile t: lane kt * 4 + r holds word (kt, r)
  auto load_mask = [&](int t) -> uint64_t {
    const int kt0 = t * (KT / 16);
    if (lane < 4 * min(4, nt16 - kt0)) return p.mask[mask_word(bh, nt16, q0 >> 4, kt0, 0) + lane];
    return 0;
  };
  bf16x8 fq[2 * NH] = {}, fo[2 * NH] = {};
  float lq = 0.f, dqv = 0.f;  // LSE (log2 units) and D of this lane's query q0 + c
  uint64_t mcur = 0, mnext = 0;
  // RAG: queries past T of a straddling wave read row T - 1, carry lq = +inf (P = 0)
  // and D = 0, so their dQ rows are exactly 0; they store nothing
  const int qr = RAG ? min(q0 + c, T_ - 1) : q0 + c;
  const bool qok = !RAG || q0 + c < T_;
  if (act) {
    const bf16* qrow = (const bf16*)p.q + (tok0 + qr) * p.q_ld + h * dh;
    const bf16* drow = (const bf16*)p.dout + (tok0 + qr) * p.dout_ld + h * dh;
    const bf16* orow = (const bf16*)p.o + (tok0 + qr) * p.o_ld + h * dh;
    bf16x8 oo[2 * NH];
#pragma unroll
    for (int u = 0; u < 2 * NH; ++u) {
      if constexpr (ANY) {  // pieces at or past dh: exact zeros, nothing read
        fq[u] = row_frag_w(qrow, u, g, dh);
        fo[u] = row_frag_w(drow, u, g, dh);
        oo[u] = row_frag_w(orow, u, g, dh);
      } else {
        fq[u] = *(const bf16x8*)(qrow + 32 * u + 8 * g);
        fo[u] = *(const bf16x8*)(drow + 32 * u + 8 * g);
        oo[u] = *(const bf16x8*)(orow + 32 * u + 8 * g);
      }
    }
    float dpart = 0.f;
#pragma unroll
    for (int u = 0; u < 2 * NH; ++u)
#pragma unroll
      for (int e = 0; e < 8; ++e) dpart += (float)fo[u][e] * (float)oo[u][e];
    dpart = sum_xor16(dpart);
    dpart = sum_xor32(dpart);
    if (g == 0 && qok) p.dsum[(int64_t)bh * T_ + qr] = dpart;
    dqv = qok ? dpart : 0.f;
    lq = qok ? p.lse[(int64_t)bh * T_ + qr] * LOG2E : INFINITY;
    if (DM == 1) mcur = load_mask(0);
  }
  if (tid == 0) *arrived = 0u;
  const float c2 = p.scale * LOG2E;
  f32x4 dq[4 * NH];
#pragma unroll
  for (int dt = 0; dt < 4 * NH; ++dt) dq[dt] = (f32x4){0.f, 0.f, 0.f, 0.f};
  for (int t = 0; t < ntile; ++t) {
    vmcnt_wait<0>();
    __syncthreads();
    if (t + 1 < ntile) {
      if (DM == 1 && act) mnext = load_mask(t + 1);  // ahead of the DMA: its wait leaves the DMA in flight
      dma.issue(smem, t + 1, (t + 1) & 1, w);
    }
    if (!act) continue;
    const char* Kimg = smem + (t & 1) * BUF_B;
    const char* Vimg = Kimg + OP_B;
    const int nc = min(2, (T_ - t * KT + (RAG ? 31 : 0)) / 32);  // 32-key chunks with a valid key
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      if (j < nc) {
        // fb[8 hf + 4 u + x]: x = 0, 1: K elements 64 hf + 32 x + 8g ..; x = 2, 3: V's
        bf16x8 fb[8 * NH];
#pragma unroll
        for (int u = 0; u < 2; ++u) {
          const int row = (2 * j + u) * 16 + c;
          asm_row128(fb[4 * u + 0], Kimg, row, 8 * g);
          if (NH == 2 || last_kc) asm_row128(fb[4 * u + 1], Kimg, row, 32 + 8 * g);
          asm_row128(fb[4 * u + 2], Vimg, row, 8 * g);
          if (NH == 2 || last_kc) asm_row128(fb[4 * u + 3], Vimg, row, 32 + 8 * g);
          if constexpr (NH == 2) {
            asm_row128(fb[8 + 4 * u + 0], Kimg + TILE_B, row, 8 * g);
            if (last_kc) asm_row128(fb[8 + 4 * u + 1], Kimg + TILE_B, row, 32 + 8 * g);
            asm_row128(fb[8 + 4 * u + 2], Vimg + TILE_B, row, 8 * g);
            if (last_kc) asm_row128(fb[8 + 4 * u + 3], Vimg + TILE_B, row, 32 + 8 * g);
          }
        }
        lgkm_fence();
        f32x4 dsv[2];
#pragma unroll
        for (int u = 0; u < 2; ++u) {
          const int ktl = 2 * j + u, kt = t * (KT / 16) + ktl;
          f32x4 sc = {0.f, 0.f, 0.f, 0.f}, dp = {0.f, 0.f, 0.f, 0.f};
          mma16(sc, fb[4 * u + 0], fq[0]);
          if (NH == 2 || last_kc) mma16(sc, fb[4 * u + 1], fq[1]);
          if constexpr (NH == 2) {
            mma16(sc, fb[8 + 4 * u + 0], fq[2]);
            if (last_kc) mma16(sc, fb[8 + 4 * u + 1], fq[3]);
          }
          mma16(dp, fb[4 * u + 2], fo[0]);
          if (NH == 2 || last_kc) mma16(dp, fb[4 * u + 3], fo[1]);
          if constexpr (NH == 2) {
            mma16(dp, fb[8 + 4 * u + 2], fo[2]);
            if (last_kc) mma16(dp, fb[8 + 4 * u + 3], fo[3]);
          }
          // sc[r] / dp[r]: S^T / dP^T at (key 16 kt + 4g + r, query q0 + c)
          bool keep[4] = {true, true, true, true};
          if constexpr (DM == 1) {
#pragma unroll
            for (int r = 0; r < 4; ++r) keep[r] = (readlane64(mcur, ktl * 4 + r) >> lane) & 1;
          } else if constexpr (DM == 2) {
            const uint64_t idx = drop_idx(bh, T_, qr, kt * 16 + 4 * g);
            if (RAG && (T_ & 1)) {  // idx may be odd: the per-element form
#pragma unroll
              for (int r = 0; r < 4; ++r) keep[r] = nstl_keep(p.seed, idx + r, p.thresh);
            } else {
              nstl_keep2(p.seed, idx, p.thresh, keep[0], keep[1]);
              nstl_keep2(p.seed, idx + 2, p.thresh, keep[2], keep[3]);
            }
          }
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            float pv = fast_exp2(sc[r] * c2 - lq);
            if constexpr (RAG) pv = kt * 16 + 4 * g + r < T_ ? pv : 0.f;  // the clamped K rows are finite
            float dpd = dp[r];
            if constexpr (DM != 0) dpd = keep[r] ? dpd * p.inv_keep : 0.f;
            dsv[u][r] = pv * (dpd - dqv);
          }
        }
        const bf16x8 fa = acc_frag<bf16>(dsv[0], dsv[1]);  // dS, row = query q0 + c
        bf16x8 fc[4];
#pragma unroll
        for (int dt = 0; dt < 4; ++dt)
          if (NH == 2 || dt < 2 || last_kc) asm_col2_128(fc[dt], Kimg, dt * 16, 32 * j, lane);
        lgkm_fence();
#pragma unroll
        for (int dt = 0; dt < 4; ++dt)
          if (NH == 2 || dt < 2 || last_kc) mma16(dq[dt], fa, fc[dt]);
        if constexpr (NH == 2) {  // columns 64 .. 127
#pragma unroll
          for (int dt = 0; dt < 4; ++dt)
            if (dt < 2 || last_kc) asm_col2_128(fc[dt], Kimg + TILE_B, dt * 16, 32 * j, lane);
          lgkm_fence();
#pragma unroll
          for (int dt = 0; dt < 4; ++dt)
            if (dt < 2 || last_kc) mma16(dq[4 + dt], fa, fc[dt]);
        }
      }
    }
    mcur = mnext;
  }
  __syncthreads();  // every wave is done with the tiles: the buffers become output staging
  float* bias_row = p.dbias ? p.dbias + (int64_t)(b * gridDim.x + blockIdx.x) * 3 * p.H * dh : nullptr;
  if (!act) {
    if (bias_row) {
#pragma unroll
      for (int hf = 0; hf < NH; ++hf) red[hf * NW * 64 + w * 64 + lane] = 0.f;
      if (last_to_arrive(arrived, NW, lane)) {
#pragma unroll
        for (int hf = 0; hf < NH; ++hf) {
          if constexpr (ANY) wave_sum_out_w(red + hf * NW * 64, NW, bias_row + h * dh + 64 * hf, lane, dh - 64 * hf);
          else wave_sum_out(red + hf * NW * 64, NW, bias_row + h * DHT + 64 * hf, lane);
        }
      }
    }
    return;
  }
  // the wave's 16 x DHT result, one 16 x 64 tile per half through the same staging
  for_halves<NH>([&](auto HF) __attribute__((always_inline)) {
    constexpr int hf = decltype(HF)::value;
    float vq[4][4];
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
      for (int dt = 0; dt < 4; ++dt) vq[dt][r] = dq[4 * hf + dt][r] * p.scale;
    char* dq_dst = p.dq + ((tok0 + q0) * p.dq_ld + h * dh + 64 * hf) * 2;
    if constexpr (ANY) {  // dh - 64 hf columns of this half exist: tables, stores and sums stop there
      if (p.rope_q) rope_back_tile_w(vq, q0 + 4 * g, c, p.rope_cos, p.rope_sin, p.rope_fast, T_ - 1, hf, dh);
      store_tile16xw<bf16>(vq, smem + w * 2048, dq_dst, p.dq_ld, lane, T_ - q0, dh - 64 * hf);
    } else if constexpr (RAG) {
      if (p.rope_q)
        rope_back_tile_clamped<DHT>(vq, q0 + 4 * g, c, p.rope_cos, p.rope_sin, p.rope_fast, T_ - 1, hf);
      store_tile16x64<bf16>(vq, smem + w * 2048, dq_dst, p.dq_ld, lane, T_ - q0);
    } else {
      if (p.rope_q) rope_back_tile<DHT>(vq, q0 + 4 * g, c, p.rope_cos, p.rope_sin, p.rope_fast, hf);
      store_tile16x64<bf16>(vq, smem + w * 2048, dq_dst, p.dq_ld, lane);
    }
    if (bias_row) {
      wave_colsum16x64<bf16>(vq, red + hf * NW * 64, w, lane);
      if (hf == NH - 1 && last_to_arrive(arrived, NW, lane)) {
#pragma unroll
        for (int h2 = 0; h2 < NH; ++h2) {
          if constexpr (ANY) wave_sum_out_w(red + h2 * NW * 64, NW, bias_row + h * dh + 64 * h2, lane, dh - 64 * h2);
          else wave_sum_out(red + h2 * NW * 64, NW, bias_row + h * DHT + 64 * h2, lane);
        }
      }
    }
  });
}

// ---------------------------------------------------------------------------
// dK / dV.  Workgroup = (b, h, 128 keys); Q / dO tiles stream; the head's LSE and
// D rows sit in LDS for the whole sweep.  st[r] / dpt[r]: S / dP at (query
// 64 t + 16 qt + 4g + r, key k0 + c).  LDS: 2 x (Q | dO) = 32 KB (later the output
// staging), lse | D (8 T bytes), bias partials, counter.
// rows of each of the LSE / D arrays: T, or (ragged T) T rounded up to whole
// 64-query tiles -- the padding rows hold lse = +inf / D = 0, and both arrays stay
// 16-byte aligned for ds_read_b128.  head_dim 128: the tile buffers are 64 KB and
// the bias partials [dk | dv][half][NW][64]; 104 KB at T = 4096.  rag: the kernel's
// RAG (a runtime-width call is ragged at every T, so it pads at T % 32 == 0 too).
int dkv_rows(int T, bool rag) { return rag ? (T + KT - 1) / KT * KT : T; }
template <int DHT> NSTL_DEV int dkv_red_off(int rows) { return 2 * Geo<DHT>::BUF_B + 2 * rows * 4; }
template <int DHT> size_t dkv_lds_bytes(int T, bool rag) {
  return (size_t)2 * Geo<DHT>::BUF_B + (size_t)2 * dkv_rows(T, rag) * 4 + 2 * Geo<DHT>::NH * NW * 64 * 4 + 16;
}

template <int DHT, int DM, bool RAG = false, bool ANY = false, bool HI = true>
__global__ __launch_bounds__(LNT) void attn_bwd_dkv_long_kernel(AttnParams p) {
  constexpr int NH = Geo<DHT>::NH, OP_B = Geo<DHT>::OP_B, BUF_B = Geo<DHT>::BUF_B;
  static_assert((!ANY || RAG) && (ANY || HI), "the runtime-width kernels are the ragged ones");
  const int dh = head_width<DHT, ANY>(p);  // ANY: 64 (NH - 1) < dh < 64 NH, dh % 8 == 0
  constexpr bool last_kc = !ANY || HI;  // the last 32-column k-chunk (accumulator tiles 2, 3 of the last half) exists
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int T_ = p.T, nt16 = (T_ + 15) / 16, ntile = (T_ + KT - 1) / KT;
  const int Tp = RAG ? ntile * KT : T_;  // dkv_rows(T, RAG)
  float* lse_s = (float*)(smem + 2 * BUF_B);
  float* dq_s = lse_s + Tp;
  float* red = (float*)(smem + dkv_red_off<DHT>(Tp));  // [2][NH][NW][64]
  unsigned* arrived = (unsigned*)(red + 2 * NH * NW * 64);
  const int tid = threadIdx.x, lane = tid & 63, g = lane >> 4, c = lane & 15;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int bh = blockIdx.y, b = bh / p.H, h = bh % p.H;
  const int64_t tok0 = (int64_t)b * T_;
  const int k0 = blockIdx.x * ROWS + w * 16;
  const bool act = k0 < T_;
  const auto dma = tile_dma_sel<DHT, ANY>(p.q, p.q_ld, p.dout, p.dout_ld, tok0, h, dh, T_, w, lane);
  dma.issue(smem, 0, 0, w);
  if constexpr (RAG) {  // queries past T: P = 2^(s - inf) = 0 and dS = 0 * (dP - 0) = 0
    for (int i = tid; i < Tp; i += LNT) {
      lse_s[i] = i < T_ ? p.lse[(int64_t)bh * T_ + i] * LOG2E : INFINITY;
      dq_s[i] = i < T_ ? p.dsum[(int64_t)bh * T_ + i] : 0.f;
    }
  } else {
    for (int i = tid; i < T_; i += LNT) {
      lse_s[i] = p.lse[(int64_t)bh * T_ + i] * LOG2E;
      dq_s[i] = p.dsum[(int64_t)bh * T_ + i];
    }
  }
  // stored keep bits of this wave's 16 keys against query tile t: lane 4 * qtl + r holds word (qtl, r)
  auto load_mask = [&](int t) -> uint64_t {
    const int qt = t * (KT / 16) + (lane >> 2);
    if (lane < 16 && qt < nt16) return p.mask[mask_word(bh, nt16, qt, k0 >> 4, lane & 3)];
    return 0;
  };
  bf16x8 fk[2 * NH] = {}, fv[2 * NH] = {};
  uint64_t mcur = 0, mnext = 0;
  // RAG: keys past T of a straddling wave read row T - 1 and get P = 0 below, so
  // their dK / dV rows are exactly 0; they store nothing
  const int kr = RAG ? min(k0 + c, T_ - 1) : k0 + c;
  const bool kok = !RAG || k0 + c < T_;
  if (act) {
    const bf16* krow = (const bf16*)p.k + (tok0 + kr) * p.k_ld + h * dh;
    const bf16* vrow = (const bf16*)p.v + (tok0 + kr) * p.v_ld + h * dh;
#pragma unroll
    for (int u = 0; u < 2 * NH; ++u) {
      if constexpr (ANY) {  // pieces at or past dh: exact zeros, nothing read
        fk[u] = row_frag_w(krow, u, g, dh);
        fv[u] = row_frag_w(vrow, u, g, dh);
      } else {
        fk[u] = *(const bf16x8*)(krow + 32 * u + 8 * g);
        fv[u] = *(const bf16x8*)(vrow + 32 * u + 8 * g);
      }
    }
    if (DM == 1) mcur = load_mask(0);
  }
  if (tid == 0) *arrived = 0u;
  const float c2 = p.scale * LOG2E;
  f32x4 dk[4 * NH], dv[4 * NH];
#pragma unroll
  for (int dt = 0; dt < 4 * NH; ++dt) dk[dt] = dv[dt] = (f32x4){0.f, 0.f, 0.f, 0.f};
  for (int t = 0; t < ntile; ++t) {
    vmcnt_wait<0>();
    __syncthreads();
    if (t + 1 < ntile) {
      if (DM == 1 && act) mnext = load_mask(t + 1);
      dma.issue(smem, t + 1, (t + 1) & 1, w);
    }
    if (!act) continue;
    const char* Qimg = smem + (t & 1) * BUF_B;
    const char* Dimg = Qimg + OP_B;
    const int nc = min(2, (T_ - t * KT + (RAG ? 31 : 0)) / 32);  // 32-query chunks with a valid query
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      if (j < nc) {
        // fb[8 hf + 4 u + x]: x = 0, 1: Q elements 64 hf + 32 x + 8g ..; x = 2, 3: dO's
        bf16x8 fb[8 * NH];
        f32x4 l4[2], d4[2];
#pragma unroll
        for (int u = 0; u < 2; ++u) {
          const int row = (2 * j + u) * 16 + c;
          asm_row128(fb[4 * u + 0], Qimg, row, 8 * g);
          if (NH == 2 || last_kc) asm_row128(fb[4 * u + 1], Qimg, row, 32 + 8 * g);
          asm_row128(fb[4 * u + 2], Dimg, row, 8 * g);
          if (NH == 2 || last_kc) asm_row128(fb[4 * u + 3], Dimg, row, 32 + 8 * g);
          if constexpr (NH == 2) {
            asm_row128(fb[8 + 4 * u + 0], Qimg + TILE_B, row, 8 * g);
            if (last_kc) asm_row128(fb[8 + 4 * u + 1], Qimg + TILE_B, row, 32 + 8 * g);
            asm_row128(fb[8 + 4 * u + 2], Dimg + TILE_B, row, 8 * g);
            if (last_kc) asm_row128(fb[8 + 4 * u + 3], Dimg + TILE_B, row, 32 + 8 * g);
          }
          const int qb = t * KT + (2 * j + u) * 16 + 4 * g;  // this lane's four queries
          l4[u] = asm_f32x4(lse_s + qb);
          d4[u] = asm_f32x4(dq_s + qb);
        }
        lgkm_fence();
        f32x4 pdv[2], dsv[2];
#pragma unroll
        for (int u = 0; u < 2; ++u) {
          const int qtl = 2 * j + u;
          f32x4 st = {0.f, 0.f, 0.f, 0.f}, dpt = {0.f, 0.f, 0.f, 0.f};
          mma16(st, fb[4 * u + 0], fk[0]);
          if (NH == 2 || last_kc) mma16(st, fb[4 * u + 1], fk[1]);
          if constexpr (NH == 2) {
            mma16(st, fb[8 + 4 * u + 0], fk[2]);
            if (last_kc) mma16(st, fb[8 + 4 * u + 1], fk[3]);
          }
          mma16(dpt, fb[4 * u + 2], fv[0]);
          if (NH == 2 || last_kc) mma16(dpt, fb[4 * u + 3], fv[1]);
          if constexpr (NH == 2) {
            mma16(dpt, fb[8 + 4 * u + 2], fv[2]);
            if (last_kc) mma16(dpt, fb[8 + 4 * u + 3], fv[3]);
          }
          // keep bits of (queries 4g + r, key k0 + c): 4 consecutive bits of word (qtl, key % 4)
          uint32_t nib = 0;
          if (DM == 1) nib = (uint32_t)(shfl64(mcur, 4 * qtl + (lane & 3)) >> (16 * (c >> 2) + 4 * g));
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            float pv = fast_exp2(st[r] * c2 - l4[u][r]);
            if constexpr (RAG) pv = kok ? pv : 0.f;
            float pdr = pv, dpd = dpt[r];
            if constexpr (DM != 0) {  // P_drop's 1/(1-p) goes onto dV at the end
              const int q = t * KT + qtl * 16 + 4 * g + r;
              const bool keep = DM == 1 ? ((nib >> r) & 1) : nstl_keep(p.seed, drop_idx(bh, T_, q, kr), p.thresh);
              pdr = keep ? pv : 0.f;
              dpd = keep ? dpd * p.inv_keep : 0.f;
            }
            pdv[u][r] = pdr;
            dsv[u][r] = pv * (dpd - d4[u][r]);
          }
        }
        const bf16x8 fa1 = acc_frag<bf16>(pdv[0], pdv[1]);  // P_drop^T, row = key k0 + c
        const bf16x8 fa2 = acc_frag<bf16>(dsv[0], dsv[1]);  // dS^T
        bf16x8 fc[8];
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) {
          if (NH == 2 || dt < 2 || last_kc) {
            asm_col2_128(fc[2 * dt], Dimg, dt * 16, 32 * j, lane);
            asm_col2_128(fc[2 * dt + 1], Qimg, dt * 16, 32 * j, lane);
          }
        }
        lgkm_fence();
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) {
          if (NH == 2 || dt < 2 || last_kc) {
            mma16(dv[dt], fa1, fc[2 * dt]);
            mma16(dk[dt], fa2, fc[2 * dt + 1]);
          }
        }
        if constexpr (NH == 2) {  // columns 64 .. 127
#pragma unroll
          for (int dt = 0; dt < 4; ++dt) {
            if (dt < 2 || last_kc) {
              asm_col2_128(fc[2 * dt], Dimg + TILE_B, dt * 16, 32 * j, lane);
              asm_col2_128(fc[2 * dt + 1], Qimg + TILE_B, dt * 16, 32 * j, lane);
            }
          }
          lgkm_fence();
#pragma unroll
          for (int dt = 0; dt < 4; ++dt) {
            if (dt < 2 || last_kc) {
              mma16(dv[4 + dt], fa1, fc[2 * dt]);
              mma16(dk[4 + dt], fa2, fc[2 * dt + 1]);
            }
          }
        }
      }
    }
    mcur = mnext;
  }
  __syncthreads();  // every wave is done with the tiles: the buffers become output staging
  float* bias_row = p.dbias ? p.dbias + (int64_t)(b * gridDim.x + blockIdx.x) * 3 * p.H * dh : nullptr;
  float* red_v = red + NH * NW * 64;
  if (!act) {
    if (bias_row) {
#pragma unroll
      for (int hf = 0; hf < NH; ++hf) {
        red[hf * NW * 64 + w * 64 + lane] = 0.f;
        red_v[hf * NW * 64 + w * 64 + lane] = 0.f;
      }
      if (last_to_arrive(arrived, NW, lane)) {
#pragma unroll
        for (int hf = 0; hf < NH; ++hf) {
          if constexpr (ANY) {
            wave_sum_out_w(red + hf * NW * 64, NW, bias_row + p.H * dh + h * dh + 64 * hf, lane, dh - 64 * hf);
            wave_sum_out_w(red_v + hf * NW * 64, NW, bias_row + 2 * p.H * dh + h * dh + 64 * hf, lane, dh - 64 * hf);
          } else {
            wave_sum_out(red + hf * NW * 64, NW, bias_row + p.H * DHT + h * DHT + 64 * hf, lane);
            wave_sum_out(red_v + hf * NW * 64, NW, bias_row + 2 * p.H * DHT + h * DHT + 64 * hf, lane);
          }
        }
      }
    }
    return;
  }
  // the wave's two 16 x DHT results, one 16 x 64 tile per half through the same staging
  char* scr = smem + w * 2048;
  for_halves<NH>([&](auto HF) __attribute__((always_inline)) {
    constexpr int hf = decltype(HF)::value;
    float vk[4][4], vv[4][4];
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
      for (int dt = 0; dt < 4; ++dt) {
        vk[dt][r] = dk[4 * hf + dt][r] * p.scale;
        vv[dt][r] = DM != 0 ? dv[4 * hf + dt][r] * p.inv_keep : dv[4 * hf + dt][r];
      }
    char* dk_dst = p.dk + ((tok0 + k0) * p.dk_ld + h * dh + 64 * hf) * 2;
    char* dv_dst = p.dv + ((tok0 + k0) * p.dv_ld + h * dh + 64 * hf) * 2;
    if constexpr (ANY) {  // dh - 64 hf columns of this half exist: tables, stores and sums stop there
      if (p.rope_k) rope_back_tile_w(vk, k0 + 4 * g, c, p.rope_cos, p.rope_sin, p.rope_fast, T_ - 1, hf, dh);
      store_tile16xw<bf16>(vk, scr, dk_dst, p.dk_ld, lane, T_ - k0, dh - 64 * hf);
      store_tile16xw<bf16>(vv, scr, dv_dst, p.dv_ld, lane, T_ - k0, dh - 64 * hf);
    } else if constexpr (RAG) {
      if (p.rope_k)
        rope_back_tile_clamped<DHT>(vk, k0 + 4 * g, c, p.rope_cos, p.rope_sin, p.rope_fast, T_ - 1, hf);
      store_tile16x64<bf16>(vk, scr, dk_dst, p.dk_ld, lane, T_ - k0);
      store_tile16x64<bf16>(vv, scr, dv_dst, p.dv_ld, lane, T_ - k0);
    } else {
      if (p.rope_k) rope_back_tile<DHT>(vk, k0 + 4 * g, c, p.rope_cos, p.rope_sin, p.rope_fast, hf);
      store_tile16x64<bf16>(vk, scr, dk_dst, p.dk_ld, lane);
      store_tile16x64<bf16>(vv, scr, dv_dst, p.dv_ld, lane);
    }
    if (bias_row) {
      wave_colsum16x64<bf16>(vk, red + hf * NW * 64, w, lane);
      wave_colsum16x64<bf16>(vv, red_v + hf * NW * 64, w, lane);
      if (hf == NH - 1 && last_to_arrive(arrived, NW, lane)) {
#pragma unroll
        for (int h2 = 0; h2 < NH; ++h2) {
          if constexpr (ANY) {
            wave_sum_out_w(red + h2 * NW * 64, NW, bias_row + p.H * dh + h * dh + 64 * h2, lane, dh - 64 * h2);
            wave_sum_out_w(red_v + h2 * NW * 64, NW, bias_row + 2 * p.H * dh + h * dh + 64 * h2, lane, dh - 64 * h2);
          } else {
            wave_sum_out(red + h2 * NW * 64, NW, bias_row + p.H * DHT + h * DHT + 64 * h2, lane);
            wave_sum_out(red_v + h2 * NW * 64, NW, bias_row + 2 * p.H * DHT + h * DHT + 64 * h2, lane);
          }
        }
      }
    }
  });
}

// The route's run-time fields as the template arguments <DHT, M, RAG, ANY, HI> of a
// generic lambda, M (one of MS...) the forward's DROP or the backward's DM.  The four
// branches are the forms that exist: a runtime width (ANY) is always ragged and is the
// only one with a lower half (!HI).
template <int... MS, class F>
int with_kernel_args(const nstl::AttnRoute& r, int m, const char* what, F&& f) {
  using Y = std::true_type;
  using N = std::false_type;
  int rc = 0;
  const bool found = nstl::with_const<64, 128>(r.dht, [&](auto DHT) {
    nstl::with_const<MS...>(m, [&](auto M) {
      if (r.any) rc = r.hi ? f(DHT, M, Y{}, Y{}, Y{}) : f(DHT, M, Y{}, Y{}, N{});
      else rc = r.rag ? f(DHT, M, Y{}, N{}, Y{}) : f(DHT, M, N{}, N{}, Y{});
    });
  });
  return found ? rc : nstl::fail((int)hipErrorInvalidValue, "%s: no streaming kernel of image class %d", what, r.dht);
}
dim3 long_grid(const AttnParams& p) { return dim3((p.T + ROWS - 1) / ROWS, p.B * p.H); }
template <int DHT> constexpr size_t fwd_lds_bytes() { return 2 * Geo<DHT>::BUF_B; }

}  // namespace

int nstl::attn_long_fwd(const AttnParams& p, const AttnRoute& r, hipStream_t st) {
  nstl::count(NSTL_K_ATTN_FWD_LONG);
  return with_kernel_args<0, 1>(r, r.drop, "nstl_attn_fwd long", [&](auto DHT, auto DROP, auto RAG, auto ANY, auto HI) {
    return launch(attn_fwd_long_kernel<DHT(), DROP() != 0, RAG(), ANY(), HI()>, long_grid(p), fwd_lds_bytes<DHT()>(), st, p,
                  "nstl_attn_fwd long", LNT);
  });
}

int nstl::attn_long_bwd(const AttnParams& p, const AttnRoute& r, hipStream_t st) {
  nstl::count(NSTL_K_ATTN_BWD_LONG);
  return with_kernel_args<0, 1, 2>(r, r.dm, "nstl_attn_bwd long", [&](auto DHT, auto DM, auto RAG, auto ANY, auto HI) {
    int rc = launch(attn_bwd_dq_long_kernel<DHT(), DM(), RAG(), ANY(), HI()>, long_grid(p), DqLds<DHT()>::BYTES, st, p,
                    "nstl_attn_bwd long dq", LNT);
    if (rc) return rc;
    return launch(attn_bwd_dkv_long_kernel<DHT(), DM(), RAG(), ANY(), HI()>, long_grid(p), dkv_lds_bytes<DHT()>(p.T, RAG()),
                  st, p, "nstl_attn_bwd long dkv", LNT);
  });
}
