// Host side of the 4-wave persistent GEMM (gemm4.h): the stream-K space, the
// stream-K plan, and the launch of a finished decision.  Which calls come here,
// with which epilogue and instantiation traits, is decided by route() in
// gemm.hip (the one place that evaluates eligibility and reads NSTL_GEMM4 /
// NSTL_GEMM4_F8); nothing here falls back to another kernel.
#include <stdlib.h>
#include <string.h>

#include <map>
#include <mutex>
#include <vector>

#include "../../include/nstl.h"
#include "common.h"
#include "gemm_host.h"
#include "status.h"

namespace {

// NSTL_GEMM4_SK=1: a stream-K tail when the grid does not divide the tiles
// (default 0: a partial last round of whole tiles, measured faster on every
// shape but the long-K weight gradients, profiles/r4_sk_bench_v2.txt); 2: the
// stream-K instantiation also when the grid divides the tiles (every tail range
// one whole tile: its cost without hand-offs; timing only)
int sk_env() {
  const char* e = getenv("NSTL_GEMM4_SK");
  return e ? atoi(e) : 0;
}

// the stream-K slabs and tickets, per (device, stream): launches on different
// streams never share them.  Tickets start at zero (hipMemset once) and every
// tile's second arriver resets its own.
struct SkSpace {
  float* slab = nullptr;
  unsigned* cnt = nullptr;
  int G = 0;
};
// At most SK_SPACES of them (2 G x 256 KB each, 128 MB at G = 256).  Nothing
// is ever freed on the launch path: a space handed out may still be waiting
// for its launch on another host thread, and a free there would also break
// stream capture.  So a new stream past SK_SPACES gets no space (its launches
// run whole tiles), and a space outgrown by a larger grid is retired, not
// freed (grids change only with a stream's CU mask; stream-K is opt-in).
constexpr size_t SK_SPACES = 4;
bool sk_space(hipStream_t st, int G, g4::StreamK& sk) {
  static std::mutex mu;
  static std::map<std::pair<int, hipStream_t>, SkSpace> spaces;
  static std::vector<SkSpace> retired;
  const int dev = nstl::stream_device(st);  // the stream's device, not the current one
  std::lock_guard<std::mutex> lk(mu);
  if (spaces.find({dev, st}) == spaces.end() && spaces.size() >= SK_SPACES) return false;
  SkSpace& s = spaces[{dev, st}];
  if (s.G < G) {
    nstl::DeviceGuard on(dev);
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(st, &cs) != hipSuccess || cs != hipStreamCaptureStatusNone) return false;
    if (s.slab) retired.push_back(s);
    s = SkSpace();
    if (hipMalloc((void**)&s.slab, (size_t)2 * G * 262144) != hipSuccess) return false;
    if (hipMalloc((void**)&s.cnt, (size_t)8 * G * sizeof(unsigned)) != hipSuccess) return false;
    if (hipMemset(s.cnt, 0, (size_t)8 * G * sizeof(unsigned)) != hipSuccess) return false;
    s.G = G;
  }
  sk.slab = s.slab;
  sk.cnt = s.cnt;
  sk.slab_bytes = (uint32_t)((size_t)2 * G * 262144);
  return true;
}

// whole tiles for the first T / G - 1 rounds, stream-K over the rest, when T is
// not a multiple of G (and every problem's K splits into 256-deep units)
void plan_sk(g4::GroupParams& gp, int G, hipStream_t st) {
  memset(&gp.sk, 0, sizeof(gp.sk));
  const int T = gp.tile_end[gp.n - 1];
  const int mode = sk_env();  // 2: the stream-K instantiation even when G divides T (timing only)
  if (T < G || !mode || (T % G == 0 && mode != 2)) return;
  const int K = gp.g[0].K;
  for (int i = 0; i < gp.n; ++i)
    if (gp.g[i].K != K) return;
  if (K % (4 * g4::BK)) return;
  g4::StreamK sk;
  if (!sk_space(st, G, sk)) {
    (void)hipGetLastError();
    return;
  }
  sk.dp_tiles = (T / G - 1) * G;
  sk.units = K / (4 * g4::BK);
  gp.sk = sk;
}

// one launch of the instantiation (r.ak, r.bk, r.em, GROUPED, SK, R3); false when nstl::g4_has has none
template <bool GROUPED, bool SK, int R3>
bool launch_as(const nstl::Gemm4Route& r, dim3 grid, hipStream_t st, const g4::GroupParams& gp) {
  bool done = false;
  nstl::with_layout(r.ak, r.bk, [&](auto AK, auto BKM) {
    nstl::with_const<g4::EM_BF16, g4::EM_RELU_DROP, g4::EM_ROPE, g4::EM_DRELU, g4::EM_F32>(r.em, [&](auto EM) {
      constexpr bool ak = decltype(AK)::value, bkm = decltype(BKM)::value;
      constexpr int em = decltype(EM)::value;
      if constexpr (nstl::g4_has(ak, bkm, em, GROUPED, SK, R3)) {
        hipLaunchKernelGGL((g4::gemm4_kernel<ak, bkm, em, GROUPED, 0, SK, R3>), grid, dim3(g4::NT), 0, st, gp);
        done = true;
      }
    });
  });
  return done;
}

}  // namespace

int nstl::gemm4_launch(g4::GroupParams& gp, const Gemm4Route& r, hipStream_t st) {
  const int tiles = gp.tile_end[gp.n - 1];
  const dim3 grid(tiles < r.G ? tiles : r.G);
  bool done;
  if (r.f8) {
    done = with_const<g4::EM_BF16, g4::EM_RELU_DROP, g4::EM_ROPE, g4::EM_DRELU>(r.em, [&](auto EM) {
      hipLaunchKernelGGL((g4::gemm4f8_kernel<decltype(EM)::value>), grid, dim3(g4::NT), 0, st, gp);
    });
  } else {
    if (r.sk_ok) plan_sk(gp, r.G, st);
    const bool sk = gp.sk.slab != nullptr;
    auto go = [&](auto GROUPED) {
      constexpr bool g = decltype(GROUPED)::value;
      return sk ? launch_as<g, true, 0>(r, grid, st, gp)
                : r.r3 ? launch_as<g, false, 1>(r, grid, st, gp) : launch_as<g, false, 0>(r, grid, st, gp);
    };
    done = r.grouped ? go(std::true_type{}) : go(std::false_type{});
    if (done && sk) count(NSTL_K_GEMM4_SK);
  }
  NSTL_CHECK_ARG(done, "nstl_gemm: no 4-wave kernel for epilogue mode %d, layout %d%d (routing error)", r.em, r.ak,
                 r.bk);
  NSTL_LAUNCH_CHECK(r.f8 ? "nstl_gemm (fp8, 4-wave persistent)"
                         : r.grouped ? "nstl_gemm_grouped (4-wave persistent)" : "nstl_gemm (4-wave persistent)");
  if (r.f8) {
    count(NSTL_K_GEMM_FP8);  // every fp8 launch, either kernel
    count(NSTL_K_GEMM4F8);
    if (r.em == g4::EM_ROPE) count(NSTL_K_GEMM_FP8_ROPE);
  } else {
    count(NSTL_K_GEMM4);
  }
  count(NSTL_K_GEMM4_TILES, tiles);
  return 0;
}
