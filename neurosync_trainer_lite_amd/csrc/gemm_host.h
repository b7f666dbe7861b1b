// Host-side pieces the two GEMM translation units share: the one layout /
// epilogue dispatch helper, and what gemm.hip's routing hands to gemm4.hip.
#pragma once
#include <type_traits>

#include "gemm4.h"

namespace nstl {

// Runtime (a_kmajor, b_kmajor) as the two std::bool_constant arguments of a generic lambda.
template <class F>
void with_layout(bool ak, bool bk, F&& f) {
  if (ak && bk) f(std::true_type{}, std::true_type{});
  else if (ak) f(std::true_type{}, std::false_type{});
  else if (!bk) f(std::false_type{}, std::false_type{});
  else f(std::false_type{}, std::true_type{});
}

// The gemm4_kernel<AK, BKM, EM, GROUPED, 0, SK, R3> instantiations that exist;
// routing asks it at run time, the launch at compile time.  Forward and dX (A
// K-major) take every epilogue, RoPE only with a K-major B and never R3; NN (the
// weight gradients) has f32 output only; there is no NT; grouped launches are NN
// + f32 or TT + RoPE (the cross-attention k|v projections of all decoder
// layers), the latter without a stream-K tail.
constexpr bool g4_has(bool ak, bool bkm, int em, bool grouped, bool sk, int r3) {
  if (em == g4::EM_ROPE && (!bkm || r3)) return false;
  if (!ak) return !bkm && em == g4::EM_F32;
  if (grouped) return bkm && em == g4::EM_ROPE && !sk;
  return true;
}

// A finished decision for the 4-wave persistent kernels (route() in gemm.hip).
struct Gemm4Route {
  int em;        // g4::EM_*
  bool f8;       // gemm4f8_kernel (K-major e4m3 operands): none of the traits below
  bool ak, bk;   // a_kmajor, b_kmajor
  bool grouped;  // the GROUPED instantiation (nstl_gemm_grouped)
  bool r3;       // the 3 + 2 slot stage ring, when no stream-K tail is planned
  bool sk_ok;    // a stream-K instantiation exists: plan_sk may plan a tail
  int G;         // persistent grid: nstl::stream_cus(st) > 0
};
// Launches gp as `r` says (gemm4.hip).  gp.sk comes in zeroed.
int gemm4_launch(g4::GroupParams& gp, const Gemm4Route& r, hipStream_t st);

}  // namespace nstl
