// Host side of attention: the one decision "which kernel does this call run?".  The
// entry points, the two size queries and nstl_attn_route_describe (attention.hip) and
// the streaming launchers (attention_long.hip) read the AttnRoute of a call; nothing
// else looks at dtype, dh, T, flags or the switches.  The rule is the table above
// nstl_attn_args in nstl.h.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/nstl.h"

namespace nstl {

// the limits the rule reads; the kernels they size take the values from here
namespace attn {
constexpr int ONESHOT_DH = 64, ONESHOT_MAX_T_BF16 = 256, ONESHOT_MAX_T_F32 = 128;
constexpr int PF_T = 128;          // the persistent forward's only T
constexpr int FUSED_MAX_T = 128;   // the fused backward: T <= this
constexpr int LONG_MAX_DH = 128, LONG_MAX_T = 4096, G_MAX_DH = 512, G_MAX_T = 4096;  // streaming, generic
static_assert(LONG_MAX_T <= G_MAX_T && LONG_MAX_DH <= G_MAX_DH, "the generic limits are the entry points' limits");
}  // namespace attn

struct AttnRoute {
  enum Family { REJECTED, GENERIC, ONESHOT, STREAMING } family;
  bool bf16;       // the element type (streaming: always)
  // ONESHOT: attn_fwd_kernel<T, nkt> or attn_fwd_persist_kernel<dm == 1>;
  // attn_bwd_fused_kernel<dm, tc> or the attn_bwd_dq / dkv_kernel<T, dm> pair
  int nkt;         // T / 16
  bool persist, fused;
  int tc;          // fused: FUSED_MAX_T when T is, else 0 (T at run time)
  // STREAMING: attn_fwd_long_kernel<dht, drop, rag, any, hi>, attn_bwd_*_long_kernel<dht, dm, rag, any, hi>
  int dht;         // image class: 64 (dh <= 64) or 128
  bool any;        // dh is neither: the runtime-width kernels, always in their ragged form
  bool hi;         // the upper 32 columns of the last image hold something (!any: always)
  bool rag;        // any || T % 32 != 0
  // every family
  int dm;          // dropout mode: 0 off, 1 the stored keep bits (mask_bits), 2 hashed
  bool drop;       // the forward's DROP: dm != 0
  int rope_fast;   // AttnParams::rope_fast (NSTL_ROPE_BWD=table: 0)
  char why[104];   // REJECTED: the error text of the entry points
};
// Validates the shape half of the arguments (null args, dtype, dh, T, B, H, p_drop; the
// pointers, strides and alignment are fill()'s, attention.hip) and routes them.  Reads
// the five switches, once each per call.
AttnRoute attn_route(const nstl_attn_args* a);
inline bool attn_mfma(const AttnRoute& r) { return r.family >= AttnRoute::ONESHOT; }

struct AttnParams;  // attention_dev.h
// r.family == STREAMING; p validated and filled by attention.hip (attention_long.hip)
int attn_long_fwd(const AttnParams& p, const AttnRoute& r, hipStream_t st);
int attn_long_bwd(const AttnParams& p, const AttnRoute& r, hipStream_t st);

}  // namespace nstl
