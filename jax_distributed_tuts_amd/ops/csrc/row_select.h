// Helpers of the kernels that select from a row of bf16 logits with one 256-thread workgroup per
// row: the sampler (attn_decode.hip), the beam search's top-W (beam.hip) and the speculative
// judge (spec.hip).  The sampler and the judge share the argmax, the top-k / top-p threshold and
// the inverse-CDF draw, so a judged row with no draft gets exactly the sampler's token.
#pragma once

#include "common.h"

#include <limits.h>

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

// the sampling weight of a logit; FILT: 0 below the threshold key
template <bool FILT>
__device__ __forceinline__ float weight(float x, float gmx, float inv_t, unsigned thr) {
  if (FILT && key16(x) < thr) return 0.f;
  return __expf((x - gmx) * inv_t);
}

// The threshold key max(key_k, key_p) of a row (every thread of the workgroup calls it and
// gets the same value).  top-k: bf16 has 65,536 values, so two 256-bin histograms of integer
// counts (high byte of the key, then the low byte inside the selected bin) give the key of
// the k-th largest logit exactly.  top-p: a binary search over the key in [key_k, key(max)];
// each probe sums the weights at or above the key in a fixed order (the thread's chunk in
// column order, the wave, the four waves), so a row always gives the same threshold.
__device__ __forceinline__ unsigned filter_threshold(const bf16_t* row, int V, int vec, int beg, int end, float gmx,
                                                     float inv_t, int top_k, float top_p) {
  __shared__ int s_hist[256], s_scan[4], s_sel[2];
  __shared__ float s_mass[2][4];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  unsigned key_k = 0;
  if (top_k > 0 && top_k < V) {
    int want = top_k;   // rank still to go, counted from the top of the current bin range
    unsigned hi_bin = 0;
    for (int level = 0; level < 2; ++level) {
      s_hist[tid] = 0;
      __syncthreads();
      for (int i0 = beg; i0 < end; i0 += 8) {
        float x[8];
        logits8(row, i0, V, vec, x);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const unsigned key = key16(x[e]);
          if (i0 + e < V && (level == 0 || (key >> 8) == hi_bin))
            atomicAdd(&s_hist[level == 0 ? key >> 8 : key & 255u], 1);   // integer counts: order-free
        }
      }
      __syncthreads();
      const int bin = 255 - tid, h = s_hist[bin];   // descending: thread 0 has the top bin
      const int inc = block_scan_incl(h, s_scan);
      if (inc >= want && inc - h < want) {   // exactly one thread: the counts sum to >= want
        s_sel[0] = bin;
        s_sel[1] = want - (inc - h);
      }
      __syncthreads();
      if (level == 0) hi_bin = (unsigned)s_sel[0];
      else key_k = (hi_bin << 8) | (unsigned)s_sel[0];
      want = s_sel[1];
    }
  }
  if (!(top_p < 1.f)) return key_k;
  int probe = 0;
  auto mass = [&](unsigned thr) {
    float m = 0.f;
    for (int i0 = beg; i0 < end; i0 += 8) {
      float x[8];
      logits8(row, i0, V, vec, x);
#pragma unroll
      for (int e = 0; e < 8; ++e) m += weight<true>(x[e], gmx, inv_t, thr);
    }
    m = wave_sum_dpp(m);
    float* s = s_mass[probe++ & 1];   // two buffers: one barrier per probe
    if (lane == 0) s[w] = m;
    __syncthreads();
    return (s[0] + s[1]) + (s[2] + s[3]);
  };
  const float target = top_p * mass(key_k);   // <= the top-k mass, so key_k always qualifies
  unsigned lo = key_k, hi = max(key16(gmx), key_k);
  while (lo < hi) {   // uniform: every thread sees the same masses
    const unsigned mid = (lo + hi + 1) >> 1;
    if (mass(mid) >= target) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

// The row's maximum (``gmx``) and its argmax, lowest index on ties (0 for a row with no finite
// maximum).  Thread t owns the contiguous columns [beg, end); every thread calls it and gets both.
__device__ __forceinline__ int row_argmax(const bf16_t* row, int V, int vec, int beg, int end, float& gmx) {
  __shared__ float s_mx[4];
  __shared__ int s_am[4];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  float mx = -INFINITY;
  int am = INT_MAX;
  for (int i0 = beg; i0 < end; i0 += 8) {
    float x[8];
    logits8(row, i0, V, vec, x);
#pragma unroll
    for (int e = 0; e < 8; ++e)
      if (x[e] > mx) { mx = x[e]; am = i0 + e; }
  }
  const float wmx = wave_max_dpp(mx);
  const int wam = wave_min_dpp(mx == wmx ? am : INT_MAX);
  if (lane == 0) { s_mx[w] = wmx; s_am[w] = wam; }
  __syncthreads();
  gmx = fmaxf(fmaxf(s_mx[0], s_mx[1]), fmaxf(s_mx[2], s_mx[3]));
  int gam = INT_MAX;
#pragma unroll
  for (int k = 0; k < 4; ++k)
    if (s_mx[k] == gmx) gam = min(gam, s_am[k]);
  return gam >= V ? 0 : gam;
}

// The inverse-CDF draw of one column of a row: weights w_i = weight<FILT>(x_i) in fp32 (EXCL: the
// weight of column ``excl`` is 0), a fixed-order prefix sum over the threads' chunk sums, target =
// u * total with u = ``word`` >> 8 as a 24-bit uniform; the first thread whose inclusive prefix
// exceeds the target walks its chunk to the first column whose running sum does.  Every thread of
// the workgroup calls it; exactly one gets the drawn column back, the others -1.  A target that
// no prefix exceeds (no weight left, or u * total rounded up to total): thread 0 gets ``gam``.
template <bool FILT, bool EXCL>
__device__ __forceinline__ int row_draw(const bf16_t* row, int V, int vec, int beg, int end, float gmx, int gam,
                                        float inv_t, unsigned thr, unsigned word, int excl) {
  __shared__ float s_w[4];
  __shared__ int s_own[4];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  float tsum = 0.f;
  for (int i0 = beg; i0 < end; i0 += 8) {
    float x[8];
    logits8(row, i0, V, vec, x);
#pragma unroll
    for (int e = 0; e < 8; ++e) tsum += (EXCL && i0 + e == excl) ? 0.f : weight<FILT>(x[e], gmx, inv_t, thr);
  }
  float inc = tsum;   // inclusive scan over the wave's threads
#pragma unroll
  for (int o = 1; o < WAVE; o <<= 1) {
    const float t = __shfl_up(inc, o, WAVE);
    if (lane >= o) inc += t;
  }
  const float prev = __shfl_up(inc, 1, WAVE);
  if (lane == WAVE - 1) s_w[w] = inc;
  __syncthreads();
  float woff = 0.f, total = 0.f;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    if (k == w) woff = total;
    total += s_w[k];
  }
  const float target = (float)(word >> 8) * (1.0f / 16777216.0f) * total;
  const int own = wave_min_dpp(woff + inc > target ? tid : INT_MAX);
  if (lane == 0) s_own[w] = own;
  __syncthreads();
  const int owner = min(min(s_own[0], s_own[1]), min(s_own[2], s_own[3]));
  if (owner == INT_MAX) return tid == 0 ? gam : -1;
  if (tid != owner) return -1;
  float run = woff + (lane > 0 ? prev : 0.f);
  int pick = -1, last = -1;
  for (int i0 = beg; i0 < end && pick < 0; i0 += 8) {
    float x[8];
    logits8(row, i0, V, vec, x);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const float wt = (EXCL && i0 + e == excl) ? 0.f : weight<FILT>(x[e], gmx, inv_t, thr);
      run += wt;
      if (wt > 0.f && pick < 0) {
        last = i0 + e;
        if (run > target) pick = i0 + e;
      }
    }
  }
  return pick >= 0 ? pick : (last >= 0 ? last : gam);
}

}  // namespace jdt
