// Speculative decoding on the KV cache: the launches a verify round adds around the append pass.
//
// A round scores C = k + 1 tokens per sequence in one append slice (the last processed token and up
// to k drafts behind it, already in ``tokens``) and keeps the longest prefix of the drafts the target
// agrees with, plus one token of the target's own.  The state is the per-row cache state (pos int32[B],
// end int32[B]) plus count int32[B] (tokens the row appends this round: 1 + its drafts), the scratch
// acc / repl int32 [B, C] and the counters drafted / accepted / emitted / last_accept int32[B].  Every
// kernel reads it on the device, so one captured round replays with no host bookkeeping.
//
// With p = pos[b], lim = min(end[b], S_max), n = count[b] - 1 drafts d_(i+1) = tokens[b, p + 1 + i] and
// logits row b * C + i the target's prediction after token index p + i:
//
// spec_count:   count[b] = 0 if p < 0 or p + 1 >= lim, else 1 + min(n_drafted[b], k, lim - p - 2): the
//               append never passes the end of the cache and the last emitted index stays below lim.
// spec_judge:   grid (C, B), one 256-thread workgroup per logits row i < count[b].  Temperature 0:
//               g = argmax (lowest index on ties), acc = (i < n and d == g), repl = g.  Otherwise, with
//               the sampler's weights w (top-k / top-p filter included), W their fixed-order sum and
//               u0, u1 = words 0, 1 of philox4x32(seed, b, ((p + i) << 32) | stream) as 24-bit uniforms:
//               i < n: acc = (0 <= d < V and u1 * W < w_d), repl = the inverse-CDF draw with u0 over w
//               with w_d zeroed (nothing left: the argmax); i == n: acc = 0, repl = the plain draw with
//               u0 -- the sampler's token for that row and position (row_select.h: the same code).
//               The drafts are a point mass, so "accept with probability p(d), else redraw from p
//               without d" is the exact speculative-sampling rule.
// spec_commit:  one wave per row.  a = the first i with acc[b, i] == 0.  An accepted draft d_j == eos_id
//               (smallest j in 1..a): pos = p + j, end = p + j + 1, j tokens emitted.  Otherwise
//               tokens[b, p + a + 1] = repl[b, a], pos = p + a + 1 and, for that token == eos_id, end =
//               p + a + 2 (the per-row sampler's convention).  Adds to the counters and, if given,
//               resynchronises the drafter's state: dpos[b] = pos[b], dend[b] = max(min(end[b], S_max) - 1, 0)
//               (for every row, from whatever pos / end hold after the round).
//
// A row takes part iff 0 <= p, 1 <= count[b] <= C and p + count[b] < lim; any other row is left
// untouched.  The hand-off between the kernels is the kernel boundary: no ticket, flag or wait here.
#include "common.h"
#include "row_select.h"

namespace jdt {

constexpr int SP_MAXC = 16;   // tokens per row of a round: up to 15 drafts and the token before them

// whether row b takes part in the round (the three kernels' common test, no overflow)
__device__ __forceinline__ bool spec_live(int p, int cnt, int C, int lim) {
  return p >= 0 && cnt >= 1 && cnt <= C && (long)p + cnt < (long)lim;
}

__global__ void __launch_bounds__(256) spec_count_kernel(const int* __restrict__ pos, const int* __restrict__ end,
                                                        const int* __restrict__ n_drafted, int* __restrict__ count,
                                                        int B, int k, int S_max) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b >= B) return;
  const int p = pos[b], lim = min(end[b], S_max);
  int c = 0;
  if (p >= 0 && (long)p + 1 < (long)lim) c = 1 + max(min(min(n_drafted[b], k), lim - p - 2), 0);
  count[b] = c;
}

// the fixed-order sum of a row's weights: the thread's chunk in column order, the wave, the four waves
template <bool FILT>
__device__ __forceinline__ float row_mass(const bf16_t* row, int V, int vec, int beg, int end, float gmx, float inv_t,
                                          unsigned thr) {
  __shared__ float s_m[4];
  float m = 0.f;
  for (int i0 = beg; i0 < end; i0 += 8) {
    float x[8];
    logits8(row, i0, V, vec, x);
#pragma unroll
    for (int e = 0; e < 8; ++e) m += weight<FILT>(x[e], gmx, inv_t, thr);
  }
  m = wave_sum_dpp(m);
  if ((threadIdx.x & 63) == 0) s_m[threadIdx.x >> 6] = m;
  __syncthreads();
  return (s_m[0] + s_m[1]) + (s_m[2] + s_m[3]);
}

template <bool FILT>
__global__ void __launch_bounds__(256) spec_judge_kernel(const bf16_t* __restrict__ logits, long ld, int V, int C,
                                                        float temperature, unsigned long long seed,
                                                        unsigned stream_id, const int* __restrict__ tokens,
                                                        int S_max, const int* __restrict__ pos_ptr,
                                                        const int* __restrict__ end_ptr,
                                                        const int* __restrict__ count, int* __restrict__ acc,
                                                        int* __restrict__ repl, int vec, int top_k, float top_p) {
  const int tid = threadIdx.x, i = blockIdx.x, b = blockIdx.y;
  const int p = pos_ptr[b], cnt = count[b];
  if (!spec_live(p, cnt, C, min(end_ptr[b], S_max)) || i >= cnt) return;   // uniform over the workgroup
  const int n = cnt - 1;
  const long slot = (long)b * C + i;
  const int d = i < n ? tokens[(long)b * S_max + p + 1 + i] : -1;   // p + 1 + i <= p + n < lim <= S_max
  const bf16_t* row = logits + slot * ld;
  const int per = (((V + 255) / 256) + 7) & ~7;
  const int beg = tid * per, end = min(beg + per, V);
  float gmx;
  const int gam = row_argmax(row, V, vec, beg, end, gmx);
  if (temperature <= 0.f) {
    if (tid == 0) {
      acc[slot] = (i < n && d == gam) ? 1 : 0;
      repl[slot] = gam;
    }
    return;
  }
  const float inv_t = 1.f / temperature;
  unsigned thr = 0;
  if (FILT) thr = filter_threshold(row, V, vec, beg, end, gmx, inv_t, top_k, top_p);
  const u32x4 r = philox4x32(seed, (uint64_t)b, ((uint64_t)(unsigned)(p + i) << 32) | (uint64_t)stream_id);
  if (i < n) {   // uniform
    const bool in_v = d >= 0 && d < V;
    const float total = row_mass<FILT>(row, V, vec, beg, end, gmx, inv_t, thr);
    const float wd = in_v ? weight<FILT>(bf2f(row[in_v ? d : 0]), gmx, inv_t, thr) : 0.f;
    const bool ok = in_v && (float)(r.y >> 8) * (1.0f / 16777216.0f) * total < wd;
    const int tok = row_draw<FILT, true>(row, V, vec, beg, end, gmx, gam, inv_t, thr, r.x, in_v ? d : -1);
    if (tok >= 0) {   // one thread
      acc[slot] = ok ? 1 : 0;
      repl[slot] = tok;
    }
  } else {
    const int tok = row_draw<FILT, false>(row, V, vec, beg, end, gmx, gam, inv_t, thr, r.x, -1);
    if (tok >= 0) {
      acc[slot] = 0;
      repl[slot] = tok;
    }
  }
}

__global__ void __launch_bounds__(WAVE) spec_commit_kernel(const int* __restrict__ acc, const int* __restrict__ repl,
                                                          int C, int* tokens, int S_max, int* pos_ptr, int* end_ptr,
                                                          const int* __restrict__ count, int eos_id,
                                                          int* __restrict__ drafted, int* __restrict__ accepted,
                                                          int* __restrict__ emitted, int* __restrict__ last_accept,
                                                          int* __restrict__ dpos, int* __restrict__ dend) {
  const int lane = threadIdx.x, b = blockIdx.x;
  const int p = pos_ptr[b], cnt = count[b], e0 = end_ptr[b];
  int np = p, ne = e0;   // the row's position and end after the round
  if (spec_live(p, cnt, C, min(e0, S_max))) {   // uniform over the wave
    const int n = cnt - 1;
    const bool rej = lane < n && acc[(long)b * C + lane] == 0;
    const unsigned long long rm = __ballot(rej);
    const int a = rm ? __ffsll((long long)rm) - 1 : n;   // first rejected index; acc[b, n] counts as 0
    // lane j - 1 looks at accepted draft d_j = tokens[b, p + j], j in 1..a (p + a <= p + n < lim)
    const bool is_eos = eos_id >= 0 && lane < a && tokens[(long)b * S_max + p + 1 + lane] == eos_id;
    const unsigned long long em = __ballot(is_eos);
    if (lane == 0) {
      int kept, out;
      if (em) {
        const int j = __ffsll((long long)em);
        np = p + j;
        ne = p + j + 1;
        kept = j;
        out = j;
      } else {
        const int tok = repl[(long)b * C + a];
        tokens[(long)b * S_max + p + a + 1] = tok;   // p + a + 1 <= p + cnt < lim <= S_max
        np = p + a + 1;
        if (eos_id >= 0 && tok == eos_id) ne = p + a + 2;
        kept = a;
        out = a + 1;
      }
      pos_ptr[b] = np;
      if (ne != e0) end_ptr[b] = ne;
      drafted[b] += n;
      accepted[b] += kept;
      emitted[b] += out;
      last_accept[b] = kept;
    }
  }
  if (lane == 0 && dpos) {
    dpos[b] = np;
    dend[b] = max(min(ne, S_max) - 1, 0);
  }
}

}  // namespace jdt
using namespace jdt;

// Codes of the three launchers, returned before anything is launched: -2 a null pointer, -4 S_max < 1,
// -5 a bad size (V < 1, ld < V, B < 0, a grid past the launch limits), -7 a temperature that is not
// >= 0, -8 top_k < 0, -9 top_p outside (0, 1], -16 C outside 1..16 (spec_count: k outside 1..15).
// B == 0: nothing to do, 0.

// pos / end / n_drafted / count: int32[B]
JDT_API int jdt_spec_count(const int* pos, const int* end, const int* n_drafted, int* count, int B, int k, int S_max,
                           void* stream) {
  if (!pos || !end || !n_drafted || !count) return -2;
  if (k < 1 || k > SP_MAXC - 1) return -16;
  if (S_max < 1) return -4;
  if (B < 0) return -5;
  if (B == 0) return 0;
  hipLaunchKernelGGL(spec_count_kernel, dim3((B + 255) / 256), dim3(256), 0, static_cast<hipStream_t>(stream), pos,
                     end, n_drafted, count, B, k, S_max);
  return HIP_LAUNCH_CHECK();
}

// logits [B * C, V] bf16 (row stride ld); tokens int32 [B, S_max]; pos / end / count int32[B]; acc / repl
// int32 [B, C].  top_k = 0 (or >= V) and top_p = 1 are "off", as in the sampler.
JDT_API int jdt_spec_judge(const void* logits, long ld, int B, int C, int V, float temperature,
                           unsigned long long seed, unsigned stream_id, const int* tokens, int S_max, const int* pos,
                           const int* end, const int* count, int* acc, int* repl, int top_k, float top_p,
                           void* stream) {
  if (!logits || !tokens || !pos || !end || !count || !acc || !repl) return -2;
  if (C < 1 || C > SP_MAXC) return -16;
  if (V < 1 || ld < V || B < 0 || B > 65535) return -5;
  if (S_max < 1) return -4;
  if (!(temperature >= 0.f)) return -7;
  if (top_k < 0) return -8;
  if (!(top_p > 0.f && top_p <= 1.f)) return -9;
  if (B == 0) return 0;
  const int vec = (V % 8 == 0) && (ld % 8 == 0) && !misaligned16(logits);
  const bool filt = temperature > 0.f && ((top_k > 0 && top_k < V) || top_p < 1.f);
  auto kernel = filt ? spec_judge_kernel<true> : spec_judge_kernel<false>;
  hipLaunchKernelGGL(kernel, dim3(C, B), dim3(256), 0, static_cast<hipStream_t>(stream),
                     static_cast<const bf16_t*>(logits), ld, V, C, temperature, seed, stream_id, tokens, S_max, pos,
                     end, count, acc, repl, vec, top_k, top_p);
  return HIP_LAUNCH_CHECK();
}

// drafted / accepted / emitted / last_accept: int32[B]; dpos / dend: int32[B] or both null
JDT_API int jdt_spec_commit(const int* acc, const int* repl, int B, int C, int* tokens, int S_max, int* pos, int* end,
                            const int* count, int eos_id, int* drafted, int* accepted, int* emitted,
                            int* last_accept, int* dpos, int* dend, void* stream) {
  if (!acc || !repl || !tokens || !pos || !end || !count || !drafted || !accepted || !emitted || !last_accept)
    return -2;
  if ((dpos == nullptr) != (dend == nullptr)) return -2;
  if (C < 1 || C > SP_MAXC) return -16;
  if (S_max < 1) return -4;
  if (B < 0) return -5;
  if (B == 0) return 0;
  hipLaunchKernelGGL(spec_commit_kernel, dim3(B), dim3(WAVE), 0, static_cast<hipStream_t>(stream), acc, repl, C,
                     tokens, S_max, pos, end, count, eos_id, drafted, accepted, emitted, last_accept, dpos, dend);
  return HIP_LAUNCH_CHECK();
}
