// Streaming (online-softmax) MFMA attention for long windows: bf16, head_dim 64,
// T % 32 == 0, 256 < T <= 4096, and with NSTL_ATTN_RAGGED_OK every T % 32 != 0 up
// to 4096; with NSTL_ATTN_DH128_OK also head_dim 128, at every T % 32 == 0 up to
// 4096 and (both flags) every ragged T (attention_long.hip).  Called from
// nstl_attn_fwd / nstl_attn_bwd with the parameter block they validated and filled.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/nstl.h"

namespace nstl {
struct AttnParams;  // attention_dev.h
// whether these (already validated) arguments take the streaming kernels;
// NSTL_ATTN_LONG=0 sends them to the generic kernels (head_dim 128 at every T: its
// A/B arm), NSTL_ATTN_RAGGED=0 the ragged ones only (read per call)
bool attn_long_takes(const nstl_attn_args* a);
int attn_long_fwd(const AttnParams& p, hipStream_t st);
int attn_long_bwd(const AttnParams& p, hipStream_t st);
}  // namespace nstl
