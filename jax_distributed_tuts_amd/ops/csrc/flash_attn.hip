// Fused (flash-style) causal self-attention for the transformer tutorial model,
// head dim 64, bf16 in/out, fp32 softmax statistics.  q/k/v are read in place
// from the fused [B*S, 3*H*64] QKV projection; O is written in place into the
// [B*S, H*64] attention output; nothing of size S x S ever reaches HBM.
//
// The tile bodies live in attn_tile.h (shared with attn_append.hip, and between the two
// backward kernels here); this file holds the kernels' loops and what differs between them.
//
// forward  grid (S/64 query blocks, B*H); 4 waves x 16 query rows.
//   Per 64-key tile: K (row-major) and V (transposed) staged in LDS,
//   S = Q K^T on MFMA (Q fragments in registers), online softmax in registers
//   (row stats reduced over the 16 lanes that share a row), P -> per-wave LDS
//   tile (bf16) -> O += P V on MFMA.  Saves LSE (of the scaled scores) per row.
// backward  ONE launch, grid (S/64 key blocks, B*H), each wave owns 16 keys:
//   per 64-query tile delta = rowsum(dO * O) (recomputed, cheaper than a launch),
//   P^T = exp(scale K Q^T - LSE), dP^T = V dO^T, dS^T = P^T (dP^T - delta),
//   dV += P^T dO, dK += dS^T Q (fp32 accumulators in registers for the whole
//   sweep), dQ += dS K summed across key blocks with fp32 atomics into a
//   persistent zeroed workspace; the key block that arrives last for its
//   (batch, head) (ticket) converts that head's dQ to bf16 into the QKV
//   gradient and re-zeroes the workspace -- no memset, delta or convert launch.
#include "attn_tile.h"

namespace jdt {

__global__ void __launch_bounds__(256) flash_fwd_kernel(const bf16_t* __restrict__ qkv, bf16_t* __restrict__ out,
                                                        float* __restrict__ lse, int S, int H, float scale,
                                                        int causal) {
  __shared__ __attribute__((aligned(16))) bf16_t Ks[AT_T * AT_LD];
  __shared__ __attribute__((aligned(16))) bf16_t Vt[AT_D * AT_LD];
  __shared__ __attribute__((aligned(16))) bf16_t Ps[4][16 * AT_LD];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int bh = blockIdx.y, b = bh / H, h = bh % H;
  const int d = H * AT_D, ld3 = 3 * d;
  const int q0 = blockIdx.x * AT_T, qw = q0 + w * 16;
  const bf16_t* base = qkv + (long)b * S * ld3;

  bf16x8 qf[2];
  float m[4], l[4];
  f32x4 o[4];
  {
    const int row = qw + (lane & 15);
    fwd_begin(base + (long)row * ld3 + h * AT_D, row < S, qf, m, l, o);
  }
  int last[4];   // the last key each of the lane's rows sees
#pragma unroll
  for (int e = 0; e < 4; ++e) last[e] = causal ? min(qw + (lane >> 4) * 4 + e, S - 1) : S - 1;

  const int kend = causal ? min(S, q0 + AT_T) : S;
  for (int k0 = 0; k0 < kend; k0 += AT_T) {
    __syncthreads();
    stage_tile<256>(base + (long)k0 * ld3 + d + h * AT_D, ld3, S - k0, Ks, nullptr);
    stage_tile<256>(base + (long)k0 * ld3 + 2 * d + h * AT_D, ld3, S - k0, nullptr, Vt);
    __syncthreads();
    fwd_tile_step(Ks, Vt, Ps[w], qf, scale, k0, last, m, l, o);
  }
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int row = qw + (lane >> 4) * 4 + e;
    if (row >= S) continue;
    fwd_store_row(out + ((long)b * S + row) * d + h * AT_D, o, e, l[e]);
    if ((lane & 15) == 0) lse[(long)bh * S + row] = m[e] + __logf(l[e]);
  }
}

__global__ void __launch_bounds__(256) flash_bwd_kernel(const bf16_t* __restrict__ qkv, const bf16_t* __restrict__ o,
                                                        const bf16_t* __restrict__ dout, const float* __restrict__ lse,
                                                        bf16_t* __restrict__ dqkv, float* __restrict__ dq_acc,
                                                        unsigned* __restrict__ tickets, float* __restrict__ dbias,
                                                        int S, int H, float scale, int causal) {
  __shared__ __attribute__((aligned(16))) bf16_t Qs[AT_T * AT_LD];
  __shared__ __attribute__((aligned(16))) bf16_t Qt[AT_D * AT_LD];
  __shared__ __attribute__((aligned(16))) bf16_t dOs[AT_T * AT_LD];
  __shared__ __attribute__((aligned(16))) bf16_t dOt[AT_D * AT_LD];
  __shared__ __attribute__((aligned(16))) bf16_t Kt[AT_D * AT_LD];
  __shared__ __attribute__((aligned(16))) bf16_t Pw[4][16 * AT_LD];
  __shared__ __attribute__((aligned(16))) bf16_t dSw[4][16 * AT_LD];
  __shared__ __attribute__((aligned(16))) bf16_t dSq[AT_T * AT_LD];   // dS[q][key] for dQ
  __shared__ float lse_s[AT_T], delta_s[AT_T];
  __shared__ int last_s;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int bh = blockIdx.y, b = bh / H, h = bh % H;
  const int d = H * AT_D, ld3 = 3 * d;
  const int k0 = blockIdx.x * AT_T, kw = k0 + w * 16;
  const bf16_t* base = qkv + (long)b * S * ld3;
  const bf16_t* dbase = dout + (long)b * S * d;
  const bf16_t* obase = o + (long)b * S * d;

  bf16x8 kf[2], vf[2];
  {
    const int key = kw + (lane & 15);
    bwd_load_kv(base + (long)key * ld3 + d + h * AT_D, d, key < S, kf, vf);
  }
  stage_tile<256>(base + (long)k0 * ld3 + d + h * AT_D, ld3, S - k0, nullptr, Kt);
  f32x4 dk[4], dv[4];
#pragma unroll
  for (int nt = 0; nt < 4; ++nt) { dk[nt] = (f32x4){0.f, 0.f, 0.f, 0.f}; dv[nt] = dk[nt]; }

  for (int q0 = causal ? k0 : 0; q0 < S; q0 += AT_T) {
    __syncthreads();
    stage_tile<256>(base + (long)q0 * ld3 + h * AT_D, ld3, S - q0, Qs, Qt);
    stage_tile<256>(dbase + (long)q0 * d + h * AT_D, d, S - q0, dOs, dOt);
    bwd_stage_stats(dbase, obase, lse + (long)bh * S, d, h, q0, S, lse_s, delta_s);
    __syncthreads();
    bwd_tile_scores(kf, vf, Qs, dOs, lse_s, delta_s, scale, q0, kw, S, causal, Pw[w], dSw[w], dSq + w * 16, AT_LD);
    __syncthreads();
    bwd_accum_dkdv(Pw[w], dSw[w], dOt, Qt, dk, dv);
    // dQ[q0 + w*16 .. +16][:] += dS K  (K-dim = this block's 64 keys), fp32 atomics across key blocks
    f32x4 dq[4];
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) dq[nt] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      const bf16x8 sa = ld8(&dSq[(w * 16 + (lane & 15)) * AT_LD + ks * 32 + 8 * (lane >> 4)]);
#pragma unroll
      for (int nt = 0; nt < 4; ++nt)
        dq[nt] = mfma16x16x32(sa, ld8(&Kt[(nt * 16 + (lane & 15)) * AT_LD + ks * 32 + 8 * (lane >> 4)]), dq[nt]);
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int q = q0 + w * 16 + (lane >> 4) * 4 + e;
      if (q >= S) continue;
#pragma unroll
      for (int nt = 0; nt < 4; ++nt)
        atomicAdd(dq_acc + ((long)b * S + q) * d + h * AT_D + nt * 16 + (lane & 15), dq[nt][e] * scale);
    }
  }
  bwd_store_dkdv(dk, dv, scale, kw, S, d, h, dqkv + (long)b * S * ld3, dbias);
  // last key block of this (batch, head): dQ fp32 -> bf16, workspace re-zeroed.
  // The dQ atomics are device-scope (performed past the per-XCD L2s); drain
  // them (vmcnt) before the ticket; the last arriver acquires at agent scope
  // (invalidating its XCD's L2) and then reads the head's dQ with plain
  // 16-byte loads, all in flight at once.
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (threadIdx.x == 0) {
    const unsigned t = __hip_atomic_fetch_add(tickets + bh, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const int last = t == gridDim.x - 1;
    if (last) __hip_atomic_store(tickets + bh, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    last_s = last;
  }
  __syncthreads();
  if (!last_s) return;
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
  constexpr int QV = AT_D / 4;  // float4 per row; thread t always owns columns 4 (t % QV) .. +3
  float sq[4] = {0.f, 0.f, 0.f, 0.f};
  for (int i0 = 0; i0 < S * QV; i0 += 256 * 8) {
    float4 v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int i = i0 + u * 256 + threadIdx.x;
      v[u] = i < S * QV ? *reinterpret_cast<const float4*>(dq_acc + ((long)b * S + i / QV) * d + h * AT_D + (i % QV) * 4)
                        : make_float4(0.f, 0.f, 0.f, 0.f);
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int i = i0 + u * 256 + threadIdx.x;
      if (i >= S * QV) continue;
      const int q = i / QV, c = (i % QV) * 4;
      *reinterpret_cast<float4*>(dq_acc + ((long)b * S + q) * d + h * AT_D + c) = make_float4(0.f, 0.f, 0.f, 0.f);
      const bf16_t h0 = f2bf(v[u].x), h1 = f2bf(v[u].y), h2 = f2bf(v[u].z), h3 = f2bf(v[u].w);
      uint2 pk;
      pk.x = (unsigned)h0 | ((unsigned)h1 << 16);
      pk.y = (unsigned)h2 | ((unsigned)h3 << 16);
      *reinterpret_cast<uint2*>(dqkv + ((long)b * S + q) * ld3 + h * AT_D + c) = pk;
      sq[0] += bf2f(h0); sq[1] += bf2f(h1); sq[2] += bf2f(h2); sq[3] += bf2f(h3);
    }
  }
  if (dbias) {  // q bias gradient: lanes t, t+16, t+32, t+48 of a wave share columns
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      sq[j] += __shfl_xor(sq[j], 16, 64);
      sq[j] += __shfl_xor(sq[j], 32, 64);
    }
    if (lane < 16) {
#pragma unroll
      for (int j = 0; j < 4; ++j) atomicAdd(dbias + h * AT_D + lane * 4 + j, sq[j]);
    }
  }
}

// ---------------------------------------------------------------------------
// Whole-head backward (S <= 128, the tutorial LM's sequence length): ONE
// workgroup of 8 waves per (batch, head), wave w owns keys 16w .. 16w + 15.
// The key-block kernel above splits a head over S/64 workgroups, so dQ (a sum
// over key blocks) needs fp32 atomics into a workspace and a last-arriver
// conversion pass; at S = 128 that atomic / ticket tail and the half-empty
// causal blocks dominated (35 us per launch, 19 TFLOP/s, rocprofv3
// profiles/r2_transformer_merged_tuned_kernel_stats.csv).  Here every key of the
// head is in the workgroup, so per 64-query tile dQ = dS K is one more MFMA
// pass over the shared dS image, written straight to dQKV as bf16: no atomics,
// no workspace, no ticket, and a fixed summation order (deterministic).
constexpr int FS = 128;          // keys per head handled by one workgroup
constexpr int KLD = FS + 8;      // padded [64][128] image row (bf16)

__global__ void __launch_bounds__(512) flash_bwd_head_kernel(const bf16_t* __restrict__ qkv,
                                                             const bf16_t* __restrict__ o,
                                                             const bf16_t* __restrict__ dout,
                                                             const float* __restrict__ lse, bf16_t* __restrict__ dqkv,
                                                             float* __restrict__ dbias, int S, int H, float scale,
                                                             int causal) {
  __shared__ __attribute__((aligned(16))) bf16_t Qs[AT_T * AT_LD];
  __shared__ __attribute__((aligned(16))) bf16_t Qt[AT_D * AT_LD];
  __shared__ __attribute__((aligned(16))) bf16_t dOs[AT_T * AT_LD];
  __shared__ __attribute__((aligned(16))) bf16_t dOt[AT_D * AT_LD];
  __shared__ __attribute__((aligned(16))) bf16_t Kt[AT_D * KLD];     // K^T [dim][key]
  __shared__ __attribute__((aligned(16))) bf16_t Pw[8][16 * AT_LD];
  __shared__ __attribute__((aligned(16))) bf16_t dSw[8][16 * AT_LD];
  __shared__ __attribute__((aligned(16))) bf16_t dSq[AT_T * KLD];    // dS[q][key]
  __shared__ float lse_s[AT_T], delta_s[AT_T];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int bh = blockIdx.x, b = bh / H, h = bh % H;
  const int d = H * AT_D, ld3 = 3 * d;
  const int kw = w * 16;
  const bf16_t* base = qkv + (long)b * S * ld3;
  const bf16_t* dbase = dout + (long)b * S * d;
  const bf16_t* obase = o + (long)b * S * d;

  bf16x8 kf[2], vf[2];
  {
    const int key = kw + (lane & 15);
    bwd_load_kv(base + (long)key * ld3 + d + h * AT_D, d, key < S, kf, vf);
  }
  stage_tile<512>(base + d + h * AT_D, ld3, S, nullptr, Kt, KLD);
  stage_tile<512>(base + (long)AT_T * ld3 + d + h * AT_D, ld3, S - AT_T, nullptr, Kt + AT_T, KLD);
  f32x4 dk[4], dv[4];
#pragma unroll
  for (int nt = 0; nt < 4; ++nt) { dk[nt] = (f32x4){0.f, 0.f, 0.f, 0.f}; dv[nt] = dk[nt]; }
  // dQ role of this wave: 16 query rows (w & 3) x 32 dims (w >> 2) of each tile
  const int qr = (w & 3) * 16, nt0 = (w >> 2) * 2;
  float sq[2] = {0.f, 0.f};

  for (int q0 = 0; q0 < S; q0 += AT_T) {
    __syncthreads();
    stage_tile<512>(base + (long)q0 * ld3 + h * AT_D, ld3, S - q0, Qs, Qt);
    stage_tile<512>(dbase + (long)q0 * d + h * AT_D, d, S - q0, dOs, dOt);
    bwd_stage_stats(dbase, obase, lse + (long)bh * S, d, h, q0, S, lse_s, delta_s);
    __syncthreads();
    // this wave's keys see any query of the tile (uniform per wave)
    const bool active = kw < S && !(causal && kw > q0 + AT_T - 1);
    if (active) {
      bwd_tile_scores(kf, vf, Qs, dOs, lse_s, delta_s, scale, q0, kw, S, causal, Pw[w], dSw[w], dSq + kw, KLD);
    } else {
#pragma unroll
      for (int nt = 0; nt < 4; ++nt)
#pragma unroll
        for (int e = 0; e < 4; ++e) dSq[(nt * 16 + (lane & 15)) * KLD + kw + (lane >> 4) * 4 + e] = 0;
    }
    __syncthreads();
    if (active) bwd_accum_dkdv(Pw[w], dSw[w], dOt, Qt, dk, dv);
    // dQ[q0 + qr .. +16][32 dims] = scale * dS K over every key that can be unmasked
    const int kmax = causal ? min(S, q0 + AT_T) : S;
    f32x4 dq[2];
    dq[0] = (f32x4){0.f, 0.f, 0.f, 0.f};
    dq[1] = dq[0];
    for (int ks = 0; ks < (kmax + 31) / 32; ++ks) {
      const bf16x8 sa = ld8(&dSq[(qr + (lane & 15)) * KLD + ks * 32 + 8 * (lane >> 4)]);
#pragma unroll
      for (int j = 0; j < 2; ++j)
        dq[j] = mfma16x16x32(sa, ld8(&Kt[((nt0 + j) * 16 + (lane & 15)) * KLD + ks * 32 + 8 * (lane >> 4)]), dq[j]);
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int q = q0 + qr + (lane >> 4) * 4 + e;
      if (q >= S) continue;
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const bf16_t qb = f2bf(dq[j][e] * scale);
        dqkv[((long)b * S + q) * ld3 + h * AT_D + (nt0 + j) * 16 + (lane & 15)] = qb;
        sq[j] += bf2f(qb);
      }
    }
  }
  bwd_store_dkdv(dk, dv, scale, kw, S, d, h, dqkv + (long)b * S * ld3, dbias);
  if (dbias) {  // q bias gradient
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      sq[j] += __shfl_xor(sq[j], 16, 64);
      sq[j] += __shfl_xor(sq[j], 32, 64);
    }
    if (lane < 16) {
#pragma unroll
      for (int j = 0; j < 2; ++j) atomicAdd(dbias + h * AT_D + (nt0 + j) * 16 + lane, sq[j]);
    }
  }
}

}  // namespace jdt
using namespace jdt;

// S <= 128: the whole-head kernels of attn128.hip (JDT_ATTN128=0 or
// jdt_flash_set_attn128(0): these tile-streaming kernels at every S, for A/B runs)
JDT_API int jdt_attn128_fwd(const void* qkv, void* out, float* lse, int B, int S, int H, float scale, int causal,
                            void* stream);
JDT_API int jdt_attn128_bwd(const void* qkv, const void* out, const void* dout, const float* lse, void* dqkv,
                            float* dbias, int B, int S, int H, float scale, int causal, void* stream);
static int g_attn128 = -1;
static bool attn128_on(int S) {
  if (g_attn128 < 0) {
    const char* e = getenv("JDT_ATTN128");
    g_attn128 = (e && e[0] == '0') ? 0 : 1;
  }
  return g_attn128 && S <= 128;
}
JDT_API void jdt_flash_set_attn128(int on) { g_attn128 = on; }

JDT_API int jdt_flash_fwd(const void* qkv, void* out, float* lse, int B, int S, int H, float scale, int causal,
                          void* stream) {
  if (attn128_on(S)) return jdt_attn128_fwd(qkv, out, lse, B, S, H, scale, causal, stream);
  dim3 grid((S + AT_T - 1) / AT_T, B * H);
  hipLaunchKernelGGL(flash_fwd_kernel, grid, dim3(256), 0, static_cast<hipStream_t>(stream),
                     static_cast<const bf16_t*>(qkv), static_cast<bf16_t*>(out), lse, S, H, scale, causal);
  return HIP_LAUNCH_CHECK();
}

static bool g_flash_head = true;
JDT_API void jdt_flash_set_head(int on) { g_flash_head = on; }  // A/B: 0 = key-block kernel at every S

// dq_acc: fp32 [B*S, H*64] workspace, all zero on entry and left zero on exit;
// tickets: B*H counters, zero on entry and on exit.
// dbias (optional, fp32 [3*H*64]): += column sums of dQKV (the QKV bias gradient).
JDT_API int jdt_flash_bwd(const void* qkv, const void* out, const void* dout, const float* lse, float* dq_acc,
                          unsigned* tickets, void* dqkv, float* dbias, int B, int S, int H, float scale, int causal,
                          void* stream) {
  if (attn128_on(S)) return jdt_attn128_bwd(qkv, out, dout, lse, dqkv, dbias, B, S, H, scale, causal, stream);
  if (S <= FS && g_flash_head) {  // whole head in one workgroup: dq_acc / tickets untouched (stay zero)
    hipLaunchKernelGGL(flash_bwd_head_kernel, dim3(B * H), dim3(512), 0, static_cast<hipStream_t>(stream),
                       static_cast<const bf16_t*>(qkv), static_cast<const bf16_t*>(out),
                       static_cast<const bf16_t*>(dout), lse, static_cast<bf16_t*>(dqkv), dbias, S, H, scale, causal);
    return HIP_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(flash_bwd_kernel, dim3((S + AT_T - 1) / AT_T, B * H), dim3(256), 0, static_cast<hipStream_t>(stream),
                     static_cast<const bf16_t*>(qkv), static_cast<const bf16_t*>(out),
                     static_cast<const bf16_t*>(dout), lse, static_cast<bf16_t*>(dqkv), dq_acc, tickets, dbias, S, H, scale,
                     causal);
  return HIP_LAUNCH_CHECK();
}
