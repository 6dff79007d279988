// Beam search on the KV cache: the two launches a beam step adds after the decode step.
//
// Batch row g * W + j is beam slot j of group g (W <= 8 beams per group).  Per slot the search
// keeps ``score`` (fp32 sum of log-probabilities), ``done`` and ``length`` (generated tokens).
// Both kernels READ the shared position word ``pos`` like the rest of the decode step, and the
// second one advances it, so one captured step replays for every token.  pos + 1 >= S_max (or a
// negative pos): neither kernel writes anything.
//
// beam_topw:    stage 1, one workgroup per batch row: fp32 max and log-sum-exp of the row's bf16
//               logits in a fixed order and the row's W largest logits, exact on the bf16 values,
//               ties to the lower token index.  Writes W (token, score[w] + log_softmax) pairs in
//               that order into the candidate scratch [B, 8]; unused entries get token -1.  A done
//               row writes the single candidate (eos_id, score[w]).
// beam_reorder: stage 2 and the history re-routing in ONE launch (so a step is two launches, no
//               separate merge launch): every workgroup re-derives its group's W best of the
//               <= W * W candidates from the scratch (score descending, then source slot, then
//               stage-1 rank; one wave, a candidate per lane), so all of them see the same
//               parent[].  Grid (ceil(S_max / 128), G * H, n_caches + 1): slice z < n_caches
//               permutes rows <= pos of cache tensor z in place, slice n_caches the token
//               histories, and its first workgroup of each group writes the new beam state and
//               tokens[:, pos + 1].  The grid depends on the cache's shape only.
//
// In-place permutation without a second buffer: a thread owns the same 16-byte piece (row, column
// slice) of every slot of its group, nobody else touches those addresses, and it loads the piece of
// every destination's parent into registers (at most 8 u32x4) before it stores the first one.  The
// loads are per destination slot, so a parent two children share is read twice (an L2 hit); the
// accesses go through one plain (non-restrict) pointer per tensor, which keeps them in program order.
//
// The last workgroup to take an arrival ticket stores pos + 1 and re-arms the ticket (the
// sampler's scheme, csrc/attn_decode.hip: every workgroup has read pos by then).
//
// logits8 / key16 / block_scan_incl are the sampler's too: csrc/row_select.h.
#include "common.h"
#include "row_select.h"

#include <limits.h>

namespace jdt {

constexpr int BM_MAXW = 8;       // beams per group, and entries per row of the candidate scratch
constexpr int BM_DH = 64;        // head dim: a cache row is 8 pieces of 16 bytes
constexpr int BM_ROWS = 128;     // cache rows (token columns) per workgroup of the reorder
constexpr int BM_PASS = 32;      // rows per pass: 256 threads / 8 pieces per row
constexpr int BM_SMAX = 32768;   // cache rows per head the decode kernels cover

// One workgroup per batch row; thread t owns the contiguous columns [t * per, (t + 1) * per) (the
// sampler's chunking).  gmx = max x; lse = logf(sum expf(x - gmx)) with libm's expf / logf (not the
// fast intrinsics), the sum in a fixed order: the thread's columns in order, the wave (DPP), the four
// waves.  A candidate's score is score[w] + ((x - gmx) - lse): no product, so nothing contracts.
// The W-th largest key comes from two 256-bin histograms of integer counts (high byte, then the
// low byte inside the selected bin), exactly; everything above it is taken, and of the columns at it
// the ``need`` lowest indices (a prefix count over the threads, whose chunks ascend).  The W entries
// are then ranked by (key descending, index ascending), so the order they were collected in drops out.
// A row whose logits are all -inf has no finite lse; its scores are NaN.
__global__ void __launch_bounds__(256) beam_topw_kernel(const bf16_t* __restrict__ logits, long ld, int V, int W,
                                                       const float* __restrict__ score,
                                                       const int* __restrict__ done, int eos_id,
                                                       int* __restrict__ cand_tok, float* __restrict__ cand_score,
                                                       const int* __restrict__ pos_ptr, int S_max, int vec) {
  __shared__ float s_mx[4], s_sum[4], s_x[BM_MAXW];
  __shared__ int s_hist[256], s_scan[4], s_sel[2], s_i[BM_MAXW], s_n;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, b = blockIdx.x;
  const int pos = pos_ptr[0];
  if (pos < 0 || pos + 1 >= S_max) return;   // uniform over the grid
  int* ct = cand_tok + (long)b * BM_MAXW;
  float* cs = cand_score + (long)b * BM_MAXW;
  const float sc = score[b];
  if (done[b]) {   // uniform over the workgroup
    if (tid < BM_MAXW) {
      ct[tid] = tid == 0 ? eos_id : -1;
      cs[tid] = tid == 0 ? sc : -INFINITY;
    }
    return;
  }
  const bf16_t* row = logits + (long)b * ld;
  const int per = (((V + 255) / 256) + 7) & ~7;
  const int beg = tid * per, end = min(beg + per, V);
  float mx = -INFINITY;
  for (int i0 = beg; i0 < end; i0 += 8) {
    float x[8];
    logits8(row, i0, V, vec, x);
#pragma unroll
    for (int e = 0; e < 8; ++e) mx = fmaxf(mx, x[e]);
  }
  mx = wave_max_dpp(mx);
  if (lane == 0) s_mx[w] = mx;
  if (tid == 0) s_n = 0;
  if (tid < BM_MAXW) { s_x[tid] = -INFINITY; s_i[tid] = 0; }
  __syncthreads();
  const float gmx = fmaxf(fmaxf(s_mx[0], s_mx[1]), fmaxf(s_mx[2], s_mx[3]));
  float ts = 0.f;
  for (int i0 = beg; i0 < end; i0 += 8) {
    float x[8];
    logits8(row, i0, V, vec, x);
#pragma unroll
    for (int e = 0; e < 8; ++e) ts += expf(x[e] - gmx);   // a column past V is -inf: adds an exact 0
  }
  ts = wave_sum_dpp(ts);
  if (lane == 0) s_sum[w] = ts;
  __syncthreads();
  const float lse = logf((s_sum[0] + s_sum[1]) + (s_sum[2] + s_sum[3]));

  // key of the W-th largest logit, and how many of the columns at that key are wanted
  int want = W;
  unsigned hi_bin = 0, key_w = 0;
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
    if (inc >= want && inc - h < want) {   // exactly one thread: the counts sum to V >= W
      s_sel[0] = bin;
      s_sel[1] = want - (inc - h);
    }
    __syncthreads();
    if (level == 0) hi_bin = (unsigned)s_sel[0];
    else key_w = (hi_bin << 8) | (unsigned)s_sel[0];
    want = s_sel[1];
  }
  const int need = want;   // columns at key_w to take; the W - need columns above it are all taken

  int neq = 0;
  for (int i0 = beg; i0 < end; i0 += 8) {
    float x[8];
    logits8(row, i0, V, vec, x);
#pragma unroll
    for (int e = 0; e < 8; ++e) neq += (i0 + e < V && key16(x[e]) == key_w) ? 1 : 0;
  }
  int eq_rank = block_scan_incl(neq, s_scan) - neq;   // columns at key_w left of this thread's chunk
  for (int i0 = beg; i0 < end; i0 += 8) {
    float x[8];
    logits8(row, i0, V, vec, x);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      if (i0 + e >= V) continue;
      const unsigned key = key16(x[e]);
      if (key > key_w || (key == key_w && eq_rank++ < need)) {
        const int slot = atomicAdd(&s_n, 1);
        if (slot < BM_MAXW) { s_x[slot] = x[e]; s_i[slot] = i0 + e; }
      }
    }
  }
  __syncthreads();
  if (tid < BM_MAXW) {
    if (tid < W) {
      const float x = s_x[tid];
      const int i = s_i[tid];
      const unsigned key = key16(x);
      int r = 0;
      for (int j = 0; j < W; ++j) {
        const unsigned kj = key16(s_x[j]);
        r += (kj > key || (kj == key && s_i[j] < i)) ? 1 : 0;
      }
      ct[r] = i;
      cs[r] = sc + ((x - gmx) - lse);
    } else {
      ct[tid] = -1;
      cs[tid] = -INFINITY;
    }
  }
}

struct BeamArgs {
  const int* cand_tok;     // [B, 8] stage-1 candidates
  const float* cand_score;
  bf16_t* const* caches;   // device table of n_caches base pointers, each [B, H, S_max, 64] bf16
  int* tokens;             // [B, S_max]
  float* score;            // [B] beam state ...
  int* done;
  int* length;
  int* parent;             // [B] this step's parent slot (0..W-1 inside the group) and token
  int* token;
  int n_caches, W, H, S_max, eos_id;
};

// everything a workgroup does before it takes its ticket
__device__ __forceinline__ void beam_reorder_body(const BeamArgs& a, int pos) {
  __shared__ int s_par[BM_MAXW], s_tok[BM_MAXW];
  __shared__ float s_sc[BM_MAXW];
  const int tid = threadIdx.x, W = a.W, H = a.H, S_max = a.S_max;
  const int g = blockIdx.y / H, h = blockIdx.y % H, z = blockIdx.z, r0 = blockIdx.x * BM_ROWS;
  if (r0 > pos) return;                      // nothing of this chunk is history yet
  if (z == a.n_caches && h != 0) return;     // the token slice needs one workgroup per (chunk, group)
  if (tid < BM_MAXW) { s_par[tid] = tid; s_tok[tid] = 0; s_sc[tid] = -INFINITY; }
  __syncthreads();
  if (tid < WAVE) {
    // stage 2: lane = source slot * 8 + stage-1 rank, so the tie order is the lane order
    const int slot = tid >> 3, rank = tid & 7;
    int tok = -1;
    float sc = -INFINITY;
    if (slot < W && rank < W) {
      const long i = (long)(g * W + slot) * BM_MAXW + rank;
      tok = a.cand_tok[i];
      sc = a.cand_score[i];
    }
    const int valid = tok >= 0 ? 1 : 0;
    int better = 0;   // valid candidates that come before this one
#pragma unroll
    for (int j = 0; j < WAVE; ++j) {
      const float sj = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, sc), j));
      const int vj = __builtin_amdgcn_readlane(valid, j);
      better += (vj && (!valid || sj > sc || (sj == sc && j < tid))) ? 1 : 0;
    }
    if (valid && better < W) { s_par[better] = slot; s_tok[better] = tok; s_sc[better] = sc; }
  }
  __syncthreads();
  int par[BM_MAXW];
  bool ident = true;
#pragma unroll
  for (int j = 0; j < BM_MAXW; ++j) {
    par[j] = j < W ? s_par[j] : j;
    ident = ident && par[j] == j;
  }
  if (z < a.n_caches) {
    if (ident) return;
    u32x4* p = reinterpret_cast<u32x4*>(a.caches[z]);   // 8 pieces per cache row
    const int rr = tid >> 3, c = tid & 7;
    for (int pass = 0; pass < BM_ROWS / BM_PASS; ++pass) {
      const int r = r0 + pass * BM_PASS + rr;
      if (r > pos) break;   // pos < S_max
      u32x4 v[BM_MAXW];
#pragma unroll
      for (int j = 0; j < BM_MAXW; ++j)
        if (j < W && par[j] != j) v[j] = p[(((long)(g * W + par[j]) * H + h) * S_max + r) * 8 + c];
#pragma unroll
      for (int j = 0; j < BM_MAXW; ++j)
        if (j < W && par[j] != j) p[(((long)(g * W + j) * H + h) * S_max + r) * 8 + c] = v[j];
    }
    return;
  }
  int* tokens = a.tokens;
  const int col = r0 + tid;
  if (!ident && tid < BM_ROWS && col <= pos) {
    int v[BM_MAXW];
#pragma unroll
    for (int j = 0; j < BM_MAXW; ++j)
      if (j < W && par[j] != j) v[j] = tokens[(long)(g * W + par[j]) * S_max + col];
#pragma unroll
    for (int j = 0; j < BM_MAXW; ++j)
      if (j < W && par[j] != j) tokens[(long)(g * W + j) * S_max + col] = v[j];
  }
  if (blockIdx.x != 0) return;
  // the group's state: the parents' done / length are read by every lane before any is overwritten
  int pd = 0, pl = 0;
  if (tid < W) {
    pd = a.done[g * W + s_par[tid]];
    pl = a.length[g * W + s_par[tid]];
  }
  __syncthreads();
  if (tid < W) {
    const int b = g * W + tid, tok = s_tok[tid];
    a.score[b] = s_sc[tid];
    a.done[b] = (pd || (a.eos_id >= 0 && tok == a.eos_id)) ? 1 : 0;
    a.length[b] = pl + (pd ? 0 : 1);
    a.parent[b] = s_par[tid];
    a.token[b] = tok;
    tokens[(long)b * S_max + pos + 1] = tok;   // pos + 1 < S_max
  }
}

__global__ void __launch_bounds__(256) beam_reorder_kernel(BeamArgs a, int* pos_ptr, unsigned* ticket) {
  const int pos = pos_ptr[0];
  if (pos < 0 || pos + 1 >= a.S_max) return;   // uniform over the grid: the ticket stays armed at 0
  beam_reorder_body(a, pos);
  __syncthreads();
  if (threadIdx.x == 0) {
    const unsigned t = atomicAdd(ticket, 1u);
    if (t == gridDim.x * gridDim.y * gridDim.z - 1) {
      pos_ptr[0] = pos + 1;
      __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
}

}  // namespace jdt
using namespace jdt;

// Shape codes of both launchers, returned before anything is launched: -2 a null pointer, -3 a head
// dim other than 64, -4 S_max outside 1..32768, -5 a bad size (V < 1, ld < V, B < 0, H < 1, a grid past
// the launch limits), -6 a cache base that is not 16-byte aligned, -12 W outside 1..8, -13 B % W != 0,
// -14 W > V, -15 eos_id >= V.

// logits [B, V] bf16 (row stride ld); score fp32 [B], done int32 [B]; cand_tok int32 [B, 8] and
// cand_score fp32 [B, 8]; pos int32[1]; eos_id < 0: no EOS (no row may be done then)
JDT_API int jdt_beam_topw(const void* logits, long ld, int B, int V, int W, const float* score, const int* done,
                          int eos_id, int* cand_tok, float* cand_score, const int* pos, int S_max, void* stream) {
  if (!logits || !score || !done || !cand_tok || !cand_score || !pos) return -2;
  if (W < 1 || W > BM_MAXW) return -12;
  if (V < 1 || ld < V || B < 0) return -5;
  if (B % W) return -13;
  if (W > V) return -14;
  if (eos_id >= V) return -15;
  if (S_max < 1 || S_max > BM_SMAX) return -4;
  if (B == 0) return 0;
  const int vec = (V % 8 == 0) && (ld % 8 == 0) && !misaligned16(logits);
  hipLaunchKernelGGL(beam_topw_kernel, dim3(B), dim3(256), 0, static_cast<hipStream_t>(stream),
                     static_cast<const bf16_t*>(logits), ld, V, W, score, done, eos_id, cand_tok, cand_score, pos,
                     S_max, vec);
  return HIP_LAUNCH_CHECK();
}

// caches_dev: device table of n_caches base pointers (every layer's K, then V: [B, H, S_max, Dh] bf16);
// caches_host: the same pointers in host memory, read here for the null / alignment checks only.
// tokens int32 [B, S_max]; score / done / length / parent / token: [B]; ticket: a zeroed uint32 the
// kernel leaves zero again.
JDT_API int jdt_beam_reorder(const int* cand_tok, const float* cand_score, void* const* caches_dev,
                             void* const* caches_host, int n_caches, int* tokens, float* score, int* done,
                             int* length, int* parent, int* token, int* pos, unsigned* ticket, int B, int W, int H,
                             int Dh, int S_max, int eos_id, void* stream) {
  if (!cand_tok || !cand_score || !tokens || !score || !done || !length || !parent || !token || !pos || !ticket)
    return -2;
  if (n_caches < 0 || (n_caches > 0 && (!caches_dev || !caches_host))) return -2;
  if (W < 1 || W > BM_MAXW) return -12;
  if (B < 0 || H < 1) return -5;
  if (B % W) return -13;
  if (Dh != BM_DH) return -3;
  if (S_max < 1 || S_max > BM_SMAX) return -4;
  for (int i = 0; i < n_caches; ++i) {
    if (!caches_host[i]) return -2;
    if (misaligned16(caches_host[i])) return -6;
  }
  if (B == 0) return 0;
  const long gy = (long)(B / W) * H, gx = (S_max + BM_ROWS - 1) / BM_ROWS, gz = (long)n_caches + 1;
  if (gy > 65535 || gz > 65535 || gx * gy * gz > INT_MAX) return -5;
  BeamArgs a;
  a.cand_tok = cand_tok;
  a.cand_score = cand_score;
  a.caches = reinterpret_cast<bf16_t* const*>(caches_dev);
  a.tokens = tokens;
  a.score = score;
  a.done = done;
  a.length = length;
  a.parent = parent;
  a.token = token;
  a.n_caches = n_caches;
  a.W = W;
  a.H = H;
  a.S_max = S_max;
  a.eos_id = eos_id;
  hipLaunchKernelGGL(beam_reorder_kernel, dim3((unsigned)gx, (unsigned)gy, (unsigned)gz), dim3(256), 0,
                     static_cast<hipStream_t>(stream), a, pos, ticket);
  return HIP_LAUNCH_CHECK();
}
