// Append attention: causal attention of a block of C new query rows per sequence against a KV
// cache in the cache's own layout -- the case between attn_decode.hip (one query against the
// cache) and flash_attn.hip (a whole sequence in the packed qkv layout).  Chunked prefill,
// teacher forcing a block of tokens and scoring a continuation all run through it.
//
// qkv [B*C, 3*H*64] bf16 (row b*C + i is token i of sequence b; columns q | k | v), caches
// [B, H, S_max, 64] bf16 (one layer), pos int32[1] (shared) or int32[B] (ROWS), read on the
// device like every decode kernel; ROWS also takes count int32[B], the tokens row b appends
// (0..C; shared: every row appends C).  For sequence b with p = pos[b], n = count[b]:
//   cache rows p + i (i < n) receive token i's k / v bit for bit,
//   o[b*C + i] (i < n) = attention of q_i over keys 0..p+i; rows i >= n of o are left alone,
//   p < 0, p + n > S_max or n outside 0..C: nothing at all is written for the sequence.
//
// Grid (ceil(C/64) query tiles, B*H), 4 waves x 16 query rows; the tile body is attn_tile.h's,
// the one flash_fwd_kernel runs (K row-major and V transposed in LDS, Q K^T and P V on
// mfma16x16x32, online softmax in registers, a per-wave P tile; fp32 scores and statistics, p
// rounded to bf16 before P V, fp32 accumulate).  One launch and no hand-off between workgroups:
//   * a workgroup writes only its own query tile's k / v rows into the cache;
//   * it reads every key >= p from qkv and only keys < p from the cache, so it never depends
//     on another workgroup's stores;
//   * key tiles are absolute, k0 = 0, 64, 128, ... in cache-row index up to the tile that holds
//     the workgroup's last query; the staging picks each row's source (at most one tile mixes
//     the two) and zero-fills rows past the workgroup's last query, so a masked key contributes
//     p = 0 times a finite v.  A fully masked tile is an exact no-op (alpha = 1, p = 0).
// Hence the bits of o for the token at absolute index t depend only on (q_t, K[0..t], V[0..t]):
// not on how the sequence was cut into calls, on C, or on the query tile the token fell into.
//
// The next key tile's global loads are issued into registers before the current tile's MFMA
// work and stored to LDS after it, so their latency overlaps the compute; the LDS store of a
// chunk is attn_tile.h's (transposed V: scalar LDS writes).
#include "attn_tile.h"

#include <limits.h>

namespace jdt {

constexpr int AP_SMAX = 32768;      // cache rows per head the launchers accept
constexpr int AP_CMAX = 1024;       // new tokens per sequence and call

template <bool ROWS>
__global__ void __launch_bounds__(256) attn_append_kernel(const bf16_t* __restrict__ qkv, bf16_t* __restrict__ kc,
                                                         bf16_t* __restrict__ vc, bf16_t* __restrict__ out,
                                                         const int* __restrict__ pos_ptr,
                                                         const int* __restrict__ count, int C, int H, int S_max,
                                                         float scale) {
  __shared__ __attribute__((aligned(16))) bf16_t Ks[AT_T * AT_LD];
  __shared__ __attribute__((aligned(16))) bf16_t Vt[AT_D * AT_LD];
  __shared__ __attribute__((aligned(16))) bf16_t Ps[4][16 * AT_LD];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int bh = blockIdx.y, b = bh / H, h = bh % H;
  const int p = pos_ptr[ROWS ? b : 0];
  const int n = ROWS ? count[b] : C;
  // out of range: nothing is written (uniform over the sequence's workgroups); S_max - n cannot overflow
  if (n < 0 || n > C || p < 0 || p > S_max - n) return;
  const int q0 = blockIdx.x * AT_T;
  if (q0 >= n) return;
  const int qn = min(q0 + AT_T, n);   // one past this workgroup's last token (chunk index)
  const int kend = p + qn;            // one past the last key any of its queries sees (<= S_max)
  const int d = H * AT_D;
  const long ld3 = 3L * d;
  const bf16_t* base = qkv + (long)b * C * ld3 + h * AT_D;   // token 0's q; + d: k; + 2 d: v
  bf16_t* Kh = kc + (long)bh * S_max * AT_D;
  bf16_t* Vh = vc + (long)bh * S_max * AT_D;

  // this query tile's k / v rows -> cache rows p + q0 .. p + qn - 1
  for (int c = threadIdx.x; c < AT_T * AT_D / 8; c += 256) {
    const int i = q0 + (c >> 3), dc = (c & 7) * 8;
    if (i < qn) {
      const bf16_t* src = base + (long)i * ld3 + dc;
      *reinterpret_cast<u32x4*>(Kh + (long)(p + i) * AT_D + dc) = *reinterpret_cast<const u32x4*>(src + d);
      *reinterpret_cast<u32x4*>(Vh + (long)(p + i) * AT_D + dc) = *reinterpret_cast<const u32x4*>(src + 2 * d);
    }
  }

  // key tile k0 -> registers: thread t owns 16-byte chunks t and t + 256 of the [64][64] tile
  u32x4 kr[2], vr[2];
  auto fetch = [&](int k0) {
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int c = threadIdx.x + 256 * j, key = k0 + (c >> 3), dc = (c & 7) * 8;
      kr[j] = (u32x4){0u, 0u, 0u, 0u};
      vr[j] = kr[j];
      if (key < p) {   // < p <= S_max: from the cache
        kr[j] = *reinterpret_cast<const u32x4*>(Kh + (long)key * AT_D + dc);
        vr[j] = *reinterpret_cast<const u32x4*>(Vh + (long)key * AT_D + dc);
      } else if (key < kend) {   // chunk token key - p < qn <= C: from qkv, never from the cache
        const bf16_t* src = base + (long)(key - p) * ld3 + dc;
        kr[j] = *reinterpret_cast<const u32x4*>(src + d);
        vr[j] = *reinterpret_cast<const u32x4*>(src + 2 * d);
      }
    }
  };
  auto stage = [&]() {
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int c = threadIdx.x + 256 * j, r = c >> 3, dc = (c & 7) * 8;
      lds_store_chunk(kr[j], r, dc, Ks);
      lds_store_chunk_t(vr[j], r, dc, Vt);
    }
  };

  bf16x8 qf[2];
  float m[4], l[4];
  f32x4 o[4];
  {
    const int i = q0 + w * 16 + (lane & 15);
    fwd_begin(base + (long)i * ld3, i < qn, qf, m, l, o);
  }
  int last[4];   // the last key each of the lane's rows sees: the query's absolute index
#pragma unroll
  for (int e = 0; e < 4; ++e) last[e] = p + q0 + w * 16 + (lane >> 4) * 4 + e;

  fetch(0);
  for (int k0 = 0; k0 < kend; k0 += AT_T) {
    __syncthreads();   // the previous tile's readers are done with Ks / Vt
    stage();
    __syncthreads();
    if (k0 + AT_T < kend) fetch(k0 + AT_T);
    fwd_tile_step(Ks, Vt, Ps[w], qf, scale, k0, last, m, l, o);
  }
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int i = q0 + w * 16 + (lane >> 4) * 4 + e;
    if (i >= qn) continue;
    fwd_store_row(out + ((long)b * C + i) * d + h * AT_D, o, e, l[e]);
  }
}

}  // namespace jdt
using namespace jdt;

// Everything is checked before anything is launched.  -11: C outside 1..1024; -5: a batch or
// head count the grid cannot hold (B * H is the grid's y extent).
template <bool ROWS>
static int attn_append_launch(const void* qkv, void* k_cache, void* v_cache, void* o, const int* pos, const int* count,
                              int B, int C, int H, int Dh, int S_max, float scale, void* stream) {
  if (Dh != AT_D) return -3;
  if (S_max < 1 || S_max > AP_SMAX) return -4;
  if (C < 1 || C > AP_CMAX) return -11;
  if (B < 0 || H < 1 || (long)B * H > 65535) return -5;
  if (!qkv || !k_cache || !v_cache || !o || !pos || (ROWS && !count)) return -2;
  if (misaligned16(qkv) || misaligned16(k_cache) || misaligned16(v_cache)) return -6;
  if (B == 0) return 0;
  hipLaunchKernelGGL(attn_append_kernel<ROWS>, dim3((C + AT_T - 1) / AT_T, B * H), dim3(256), 0,
                     static_cast<hipStream_t>(stream), static_cast<const bf16_t*>(qkv), static_cast<bf16_t*>(k_cache),
                     static_cast<bf16_t*>(v_cache), static_cast<bf16_t*>(o), pos, count, C, H, S_max, scale);
  return HIP_LAUNCH_CHECK();
}

// qkv [B*C, 3*H*Dh] bf16 (q | k | v), caches [B, H, S_max, Dh] bf16, o [B*C, H*Dh] bf16, pos int32[1]:
// every sequence appends C tokens at rows pos .. pos + C - 1
JDT_API int jdt_attn_append(const void* qkv, void* k_cache, void* v_cache, void* o, const int* pos, int B, int C,
                            int H, int Dh, int S_max, float scale, void* stream) {
  return attn_append_launch<false>(qkv, k_cache, v_cache, o, pos, nullptr, B, C, H, Dh, S_max, scale, stream);
}

// one position and one token count (0..C) per sequence: pos int32[B], count int32[B]
JDT_API int jdt_attn_append_rows(const void* qkv, void* k_cache, void* v_cache, void* o, const int* pos,
                                 const int* count, int B, int C, int H, int Dh, int S_max, float scale, void* stream) {
  return attn_append_launch<true>(qkv, k_cache, v_cache, o, pos, count, B, C, H, Dh, S_max, scale, stream);
}
