// Helpers of the kernels that select from a row of bf16 logits with one 256-thread workgroup per
// row: the sampler (attn_decode.hip) and the beam search's top-W (beam.hip).
#pragma once

#include "common.h"

namespace jdt {

// 8 logits from column i0 (a multiple of 8) of a row; columns >= V read as -inf
__device__ __forceinline__ void logits8(const bf16_t* row, int i0, int V, bool vec, float (&x)[8]) {
  if (vec) {   // V % 8 == 0 and a 16-byte aligned row: i0 < V covers all 8
    unpack8(*reinterpret_cast<const u32x4*>(row + i0), x);
    return;
  }
#pragma unroll
  for (int e = 0; e < 8; ++e) x[e] = i0 + e < V ? bf2f(row[i0 + e]) : -INFINITY;
}

// Order-preserving 16-bit key of a bf16 value held in a float: a larger value has a larger
// key.  -0 shares the key of +0 and a NaN gets key 0 (below -inf), so it is never kept.
__device__ __forceinline__ unsigned key16(float x) {
  unsigned h = __float_as_uint(x) >> 16;
  if ((h & 0x7fffu) > 0x7f80u) return 0u;
  if (h == 0x8000u) h = 0u;
  return (h & 0x8000u) ? (~h & 0xffffu) : (h | 0x8000u);
}

// inclusive prefix sum of v over the workgroup's 256 threads (every thread calls it)
__device__ __forceinline__ int block_scan_incl(int v, int* s_tmp) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
  for (int o = 1; o < WAVE; o <<= 1) {
    const int t = __shfl_up(v, o, WAVE);
    if (lane >= o) v += t;
  }
  __syncthreads();   // the previous call's readers are done with s_tmp
  if (lane == WAVE - 1) s_tmp[w] = v;
  __syncthreads();
  int off = 0;
#pragma unroll
  for (int k = 0; k < 3; ++k)
    if (k < w) off += s_tmp[k];
  return v + off;
}

}  // namespace jdt
