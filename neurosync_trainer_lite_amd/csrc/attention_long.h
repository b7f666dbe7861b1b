// Streaming (online-softmax) MFMA attention for long windows: bf16, head_dim 64,
// T % 32 == 0, 256 < T <= 4096 (attention_long.hip).  Called from nstl_attn_fwd /
// nstl_attn_bwd after their argument checks.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/nstl.h"

namespace nstl {
// whether these (already validated) arguments take the streaming kernels;
// NSTL_ATTN_LONG=0 sends them to the generic kernels (read per call)
bool attn_long_takes(const nstl_attn_args* a);
int attn_long_fwd(const nstl_attn_args* a, hipStream_t st);
// rope_fast: RoPE^T angles recomputed instead of read from the tables (NSTL_ROPE_BWD)
int attn_long_bwd(const nstl_attn_args* a, int rope_fast, hipStream_t st);
}  // namespace nstl
