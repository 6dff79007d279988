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
// Grid (ceil(C/64) query tiles, B*H), 4 waves x 16 query rows; the tile body is
// flash_fwd_kernel's (K row-major and V transposed in LDS, Q K^T and P V on mfma16x16x32, online
// softmax in registers, a per-wave P tile; fp32 scores and statistics, p rounded to bf16 before
// P V, fp32 accumulate).  One launch and no hand-off between workgroups:
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
// work and stored to LDS after it, so their latency overlaps the compute; the transposed V
// staging is flash_attn.hip's (scalar LDS writes).
#include "common.h"

#include <limits.h>

namespace jdt {

constexpr int AP_D = 64;            // head dim
constexpr int AP_T = 64;            // query / key tile
constexpr int AP_LD = AP_T + 8;     // padded LDS row (bf16 elements)
constexpr int AP_SMAX = 32768;      // cache rows per head the launchers accept
constexpr int AP_CMAX = 1024;       // new tokens per sequence and call

__device__ __forceinline__ bf16x8 ap_ld8(const bf16_t* p) { return *reinterpret_cast<const bf16x8*>(p); }

template <bool ROWS>
__global__ void __launch_bounds__(256) attn_append_kernel(const bf16_t* __restrict__ qkv, bf16_t* __restrict__ kc,
                                                         bf16_t* __restrict__ vc, bf16_t* __restrict__ out,
                                                         const int* __restrict__ pos_ptr,
                                                         const int* __restrict__ count, int C, int H, int S_max,
                                                         float scale) {
  __shared__ __attribute__((aligned(16))) bf16_t Ks[AP_T * AP_LD];
  __shared__ __attribute__((aligned(16))) bf16_t Vt[AP_D * AP_LD];
  __shared__ __attribute__((aligned(16))) bf16_t Ps[4][16 * AP_LD];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int bh = blockIdx.y, b = bh / H, h = bh % H;
  const int p = pos_ptr[ROWS ? b : 0];
  const int n = ROWS ? count[b] : C;
  // out of range: nothing is written (uniform over the sequence's workgroups); S_max - n cannot overflow
  if (n < 0 || n > C || p < 0 || p > S_max - n) return;
  const int q0 = blockIdx.x * AP_T;
  if (q0 >= n) return;
  const int qn = min(q0 + AP_T, n);   // one past this workgroup's last token (chunk index)
  const int kend = p + qn;            // one past the last key any of its queries sees (<= S_max)
  const int d = H * AP_D;
  const long ld3 = 3L * d;
  const bf16_t* base = qkv + (long)b * C * ld3 + h * AP_D;   // token 0's q; + d: k; + 2 d: v
  bf16_t* Kh = kc + (long)bh * S_max * AP_D;
  bf16_t* Vh = vc + (long)bh * S_max * AP_D;

  // this query tile's k / v rows -> cache rows p + q0 .. p + qn - 1
  for (int c = threadIdx.x; c < AP_T * AP_D / 8; c += 256) {
    const int i = q0 + (c >> 3), dc = (c & 7) * 8;
    if (i < qn) {
      const bf16_t* src = base + (long)i * ld3 + dc;
      *reinterpret_cast<u32x4*>(Kh + (long)(p + i) * AP_D + dc) = *reinterpret_cast<const u32x4*>(src + d);
      *reinterpret_cast<u32x4*>(Vh + (long)(p + i) * AP_D + dc) = *reinterpret_cast<const u32x4*>(src + 2 * d);
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
        kr[j] = *reinterpret_cast<const u32x4*>(Kh + (long)key * AP_D + dc);
        vr[j] = *reinterpret_cast<const u32x4*>(Vh + (long)key * AP_D + dc);
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
      *reinterpret_cast<u32x4*>(Ks + r * AP_LD + dc) = kr[j];
      const unsigned q[4] = {vr[j].x, vr[j].y, vr[j].z, vr[j].w};
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        Vt[(dc + 2 * u) * AP_LD + r] = (bf16_t)(q[u] & 0xffff);
        Vt[(dc + 2 * u + 1) * AP_LD + r] = (bf16_t)(q[u] >> 16);
      }
    }
  };

  bf16x8 qf[2];
  {
    const int i = q0 + w * 16 + (lane & 15);
#pragma unroll
    for (int ks = 0; ks < 2; ++ks)
      qf[ks] = i < qn ? ap_ld8(base + (long)i * ld3 + ks * 32 + 8 * (lane >> 4)) : (bf16x8){0, 0, 0, 0, 0, 0, 0, 0};
  }
  float m[4], l[4];
  f32x4 o[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) { m[e] = -INFINITY; l[e] = 0.f; }
#pragma unroll
  for (int nt = 0; nt < 4; ++nt) o[nt] = (f32x4){0.f, 0.f, 0.f, 0.f};

  fetch(0);
  for (int k0 = 0; k0 < kend; k0 += AP_T) {
    __syncthreads();   // the previous tile's readers are done with Ks / Vt
    stage();
    __syncthreads();
    if (k0 + AP_T < kend) fetch(k0 + AP_T);
    // S = Q K^T (16 x 64 per wave)
    f32x4 s[4];
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) {
      s[nt] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < 2; ++ks)
        s[nt] = mfma16x16x32(qf[ks], ap_ld8(&Ks[(nt * 16 + (lane & 15)) * AP_LD + ks * 32 + 8 * (lane >> 4)]), s[nt]);
    }
    // online softmax over this tile (row r = (lane>>4)*4 + e; key column nt*16 + (lane&15))
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int qabs = p + q0 + w * 16 + (lane >> 4) * 4 + e;   // the query's absolute index
      float mx = -INFINITY;
#pragma unroll
      for (int nt = 0; nt < 4; ++nt) {
        const int key = k0 + nt * 16 + (lane & 15);
        float v = s[nt][e] * scale;
        if (key > qabs) v = -INFINITY;
        s[nt][e] = v;
        mx = fmaxf(mx, v);
      }
#pragma unroll
      for (int off = 1; off < 16; off <<= 1) mx = fmaxf(mx, __shfl_xor(mx, off, 64));
      const float mnew = fmaxf(m[e], mx);
      const float alpha = (mnew == -INFINITY) ? 1.f : __expf(m[e] - mnew);
      float rs = 0.f;
#pragma unroll
      for (int nt = 0; nt < 4; ++nt) {
        const float pe = (mnew == -INFINITY) ? 0.f : __expf(s[nt][e] - mnew);
        s[nt][e] = pe;
        rs += pe;
      }
#pragma unroll
      for (int off = 1; off < 16; off <<= 1) rs += __shfl_xor(rs, off, 64);
      l[e] = l[e] * alpha + rs;
      m[e] = mnew;
#pragma unroll
      for (int nt = 0; nt < 4; ++nt) o[nt][e] *= alpha;
    }
    // P (bf16) -> per-wave LDS tile [row][key] so it can be the A operand of P V
#pragma unroll
    for (int nt = 0; nt < 4; ++nt)
#pragma unroll
      for (int e = 0; e < 4; ++e) Ps[w][((lane >> 4) * 4 + e) * AP_LD + nt * 16 + (lane & 15)] = f2bf(s[nt][e]);
    __builtin_amdgcn_s_waitcnt(0xC07F);  // lgkmcnt(0): this wave's P writes land before its reads
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      const bf16x8 pa = ap_ld8(&Ps[w][(lane & 15) * AP_LD + ks * 32 + 8 * (lane >> 4)]);
#pragma unroll
      for (int nt = 0; nt < 4; ++nt)
        o[nt] = mfma16x16x32(pa, ap_ld8(&Vt[(nt * 16 + (lane & 15)) * AP_LD + ks * 32 + 8 * (lane >> 4)]), o[nt]);
    }
  }
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int i = q0 + w * 16 + (lane >> 4) * 4 + e;
    if (i >= qn) continue;
    const float inv = 1.f / l[e];
#pragma unroll
    for (int nt = 0; nt < 4; ++nt)
      out[((long)b * C + i) * d + h * AP_D + nt * 16 + (lane & 15)] = f2bf(o[nt][e] * inv);
  }
}

}  // namespace jdt
using namespace jdt;

static bool ap_misaligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) != 0; }

// Everything is checked before anything is launched.  -11: C outside 1..1024; -5: a batch or
// head count the grid cannot hold (B * H is the grid's y extent).
template <bool ROWS>
static int attn_append_launch(const void* qkv, void* k_cache, void* v_cache, void* o, const int* pos, const int* count,
                              int B, int C, int H, int Dh, int S_max, float scale, void* stream) {
  if (Dh != AP_D) return -3;
  if (S_max < 1 || S_max > AP_SMAX) return -4;
  if (C < 1 || C > AP_CMAX) return -11;
  if (B < 0 || H < 1 || (long)B * H > 65535) return -5;
  if (!qkv || !k_cache || !v_cache || !o || !pos || (ROWS && !count)) return -2;
  if (ap_misaligned16(qkv) || ap_misaligned16(k_cache) || ap_misaligned16(v_cache)) return -6;
  if (B == 0) return 0;
  hipLaunchKernelGGL(attn_append_kernel<ROWS>, dim3((C + AP_T - 1) / AP_T, B * H), dim3(256), 0,
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
