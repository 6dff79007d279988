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
//
// Split-KV (the ``_split`` launchers, opt-in): at B = 1 the grid above is a handful of workgroups
// that each walk the whole cache below their query tile.  The split pair spreads one query tile's
// keys over workgroups instead, as attn_decode.hip does for one query: two launches on one stream,
// the kernel boundary is the hand-off (no in-launch tickets, flags or waits).
//   * split launch (attn_append_kernel<ROWS, true>: the same kernel text, as attn_decode_kernel's
//     SPLIT), grid (ceil(C/64), B*H, ceil(S_max/AP_SPAN)): workgroup (qt, bh, s) runs the
//     body over the key tiles of span s only, the ABSOLUTE cache rows [s*AP_SPAN, (s+1)*AP_SPAN)
//     below p + qn, and instead of normalising stores each row's (m, l, unnormalised o[64]) into
//     workspace slot (bh, qt, s, row).  A span that starts at or past p + qn has no workgroup work
//     and no partial.  Only the s == 0 workgroup (it always exists) writes the tile's k / v rows
//     into the cache; nobody reads what another workgroup of the launch writes.
//   * combine launch, grid (ceil(C/64), B*H): row i with t = p + i folds the partials of spans
//     0 .. t / AP_SPAN in increasing order with the decode combine's expressions: M = max m_s,
//     L = sum l_s e^(m_s - M), o = (sum o_s e^(m_s - M)) * (1 / L) as bf16.  Exactly those slots are
//     read -- each was written by this call's split launch, so stale (even NaN) workspace contents
//     are harmless.  One span: e^0 = 1 and o_0 * (1 / l_0), the bits of the one-launch kernel.
// The spans are absolute and a fully masked tile is an exact no-op, so the cut invariance above
// holds for the split pair too; the caches come out bit for bit as from the one-launch kernel.
#include "attn_tile.h"
#include "kv_fp8.h"

#include <limits.h>

#include <type_traits>

namespace jdt {

constexpr int AP_SMAX = 32768;      // cache rows per head the launchers accept
constexpr int AP_CMAX = 1024;       // new tokens per sequence and call
constexpr int AP_SPAN = 512;        // keys per workgroup of the split launch: 8 key tiles, absolute cache rows
constexpr int AP_SLOT = 2 + AT_D;   // fp32 words of a row's partial: max, sum, unnormalised o[64]
constexpr int AP_CB = 8;            // spans the combine loads at a time

// One body for both launches, as attn_decode_kernel.  SPLIT (the split launch): blockIdx.z is the
// span and ``out`` is the fp32 workspace instead of o, so <ROWS, false> keeps the one-launch
// kernel's arguments and instruction stream.
//
// FP8 (the ``_fp8`` launchers, one launch only; kv_fp8.h has the format): the caches are e4m3 bytes with
// one fp32 scale per row in ``ksc`` / ``vsc`` [B, H, S_max].  The 8 consecutive threads that own a row's
// eight chunks are an aligned lane octet: they quantize the row together.  The cache write stores the
// tile's rows quantized; a key below p is fetched as 8 bytes plus its scale and a key of the chunk as its
// qkv row, and both become the bf16x8 image of the DEQUANTIZED row (exact) just before staging -- the
// chunk's keys through the quantizer, so a query sees them as every later call will read them back.
// Staging, the tile body and the epilogue are the bf16 kernel's, and FP8 = false is that kernel (``ksc`` /
// ``vsc`` are null and unused): every FP8 statement is under ``if constexpr``.
template <bool ROWS, bool SPLIT, bool FP8>
__global__ void __launch_bounds__(256)
attn_append_kernel(const bf16_t* __restrict__ qkv, std::conditional_t<FP8, uint8_t, bf16_t>* __restrict__ kc,
                   std::conditional_t<FP8, uint8_t, bf16_t>* __restrict__ vc,
                   std::conditional_t<SPLIT, float, bf16_t>* __restrict__ out, const int* __restrict__ pos_ptr,
                   const int* __restrict__ count, int C, int H, int S_max, float scale, float* __restrict__ ksc,
                   float* __restrict__ vsc) {
  static_assert(!(FP8 && SPLIT), "the split launchers take bf16 caches only");
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
  // SPLIT: the span's key tiles [kbeg, kstop) only; a span at or past kend: no partial, its slot is never read
  const int kbeg = SPLIT ? (int)blockIdx.z * AP_SPAN : 0;
  if (SPLIT && kbeg >= kend) return;
  const int kstop = SPLIT ? min(kbeg + AP_SPAN, kend) : kend;
  const int d = H * AT_D;
  const long ld3 = 3L * d;
  const bf16_t* base = qkv + (long)b * C * ld3 + h * AT_D;   // token 0's q; + d: k; + 2 d: v
  auto* Kh = kc + (long)bh * S_max * AT_D;
  auto* Vh = vc + (long)bh * S_max * AT_D;
  // FP8: the scales of this head's rows
  float* Ksc = nullptr;
  float* Vsc = nullptr;
  if constexpr (FP8) {
    Ksc = ksc + (long)bh * S_max;
    Vsc = vsc + (long)bh * S_max;
  }

  // this query tile's k / v rows -> cache rows p + q0 .. p + qn - 1 (SPLIT: span 0's workgroup alone)
  for (int c = threadIdx.x; c < AT_T * AT_D / 8; c += 256) {
    const int i = q0 + (c >> 3), dc = (c & 7) * 8;
    if constexpr (FP8) {
      // every lane runs the quantizer (the loop's trip count is the same for all): a row past qn is zeros
      const bool own = i < qn;   // the same in the row's octet
      const bf16_t* src = base + (long)i * ld3 + dc;
      u32x4 kx = {0u, 0u, 0u, 0u}, vx = kx;
      if (own) {
        kx = *reinterpret_cast<const u32x4*>(src + d);
        vx = *reinterpret_cast<const u32x4*>(src + 2 * d);
      }
      float ksv, vsv;
      const u32x2 kq = kv_quantize8(kx, ksv), vq = kv_quantize8(vx, vsv);
      if (own) {
        *reinterpret_cast<u32x2*>(Kh + (long)(p + i) * AT_D + dc) = kq;
        *reinterpret_cast<u32x2*>(Vh + (long)(p + i) * AT_D + dc) = vq;
        if (dc == 0) {
          Ksc[p + i] = ksv;
          Vsc[p + i] = vsv;
        }
      }
    } else if (i < qn && (!SPLIT || blockIdx.z == 0)) {
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
        if constexpr (FP8) {   // the raw image: 8 bytes, then the row's scale; dequant() below opens it
          const u32x2 k8 = *reinterpret_cast<const u32x2*>(Kh + (long)key * AT_D + dc);
          const u32x2 v8 = *reinterpret_cast<const u32x2*>(Vh + (long)key * AT_D + dc);
          kr[j] = (u32x4){k8[0], k8[1], __float_as_uint(Ksc[key]), 0u};
          vr[j] = (u32x4){v8[0], v8[1], __float_as_uint(Vsc[key]), 0u};
        } else {
          kr[j] = *reinterpret_cast<const u32x4*>(Kh + (long)key * AT_D + dc);
          vr[j] = *reinterpret_cast<const u32x4*>(Vh + (long)key * AT_D + dc);
        }
      } else if (key < kend) {   // chunk token key - p < qn <= C: from qkv, never from the cache
        const bf16_t* src = base + (long)(key - p) * ld3 + dc;
        kr[j] = *reinterpret_cast<const u32x4*>(src + d);
        vr[j] = *reinterpret_cast<const u32x4*>(src + 2 * d);
      }
    }
  };
  // FP8: what fetch(k0) left -> the bf16x8 images of the dequantized rows.  Kept apart from fetch so
  // that the loads stay in flight over the previous tile's MFMA work.  Every lane runs the quantizer
  // (a row that is not a chunk key goes through as zeros); the case is the same in a row's octet.
  auto dequant = [&](int k0) {
    const bool below = k0 + AT_T <= p;   // the whole tile comes from the cache (uniform): no quantizer
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int key = k0 + ((threadIdx.x + 256 * j) >> 3);
      const bool cached = key < p, fresh = !cached && key < kend;
      const u32x4 zero = {0u, 0u, 0u, 0u};
      u32x4 kd = zero, vd = zero;
      if (!below) {
        float ksv, vsv;
        const u32x2 kq = kv_quantize8(fresh ? kr[j] : zero, ksv), vq = kv_quantize8(fresh ? vr[j] : zero, vsv);
        kd = kv_dequantize8(kq, ksv);
        vd = kv_dequantize8(vq, vsv);
      }
      if (cached) {
        kr[j] = kv_dequantize8((u32x2){kr[j][0], kr[j][1]}, __uint_as_float(kr[j][2]));
        vr[j] = kv_dequantize8((u32x2){vr[j][0], vr[j][1]}, __uint_as_float(vr[j][2]));
      } else {
        kr[j] = kd;   // zeros past kend
        vr[j] = vd;
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

  fetch(kbeg);
  for (int k0 = kbeg; k0 < kstop; k0 += AT_T) {
    __syncthreads();   // the previous tile's readers are done with Ks / Vt
    if constexpr (FP8) dequant(k0);
    stage();
    __syncthreads();
    if (k0 + AT_T < kstop) fetch(k0 + AT_T);
    fwd_tile_step(Ks, Vt, Ps[w], qf, scale, k0, last, m, l, o);
  }
  // SPLIT: the query tile's 64 slots of span blockIdx.z; a row whose queries all lie below the span
  // leaves (-inf, 0, 0), which the combine never reads
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int i = q0 + w * 16 + (lane >> 4) * 4 + e;
    if (i >= qn) continue;
    if constexpr (SPLIT) {
      float* slot = out + (((long)bh * gridDim.x + blockIdx.x) * gridDim.z + blockIdx.z) * (AT_T * AP_SLOT) +
                    (i - q0) * AP_SLOT;
      if ((lane & 15) == 0) {   // m and l are the same in the row's 16 lanes
        slot[0] = m[e];
        slot[1] = l[e];
      }
#pragma unroll
      for (int nt = 0; nt < 4; ++nt) slot[2 + nt * 16 + (lane & 15)] = o[nt][e];
    } else {
      fwd_store_row(out + ((long)b * C + i) * d + h * AT_D, o, e, l[e]);
    }
  }
}

// The combine launch: grid (ceil(C/64), B*H), 1024 threads = 64 rows x 16 lanes; lane j of row r owns
// columns 2j, 2j + 1, 32 + 2j and 33 + 2j (two 8-byte loads per partial: a slot is 8-byte aligned).
// Row i of the chunk (t = p + i) folds spans 0 .. t / AP_SPAN in increasing order, AP_CB spans' loads
// in flight at a time (a block's tail past the last span re-reads that span and is not folded); the
// expressions are attn_decode_combine_kernel's.  Rows i >= n of o and out-of-range sequences are
// left alone.
template <bool ROWS>
__global__ void __launch_bounds__(1024) attn_append_combine_kernel(const float* __restrict__ ws,
                                                                  bf16_t* __restrict__ out,
                                                                  const int* __restrict__ pos_ptr,
                                                                  const int* __restrict__ count, int C, int H,
                                                                  int S_max, int n_spans) {
  const int bh = blockIdx.y, b = bh / H, h = bh % H;
  const int p = pos_ptr[ROWS ? b : 0];
  const int n = ROWS ? count[b] : C;
  if (n < 0 || n > C || p < 0 || p > S_max - n) return;
  const int r = threadIdx.x >> 4, j = threadIdx.x & 15;
  const int i = blockIdx.x * AT_T + r;
  if (i >= n) return;   // the 16 lanes of a row leave together; no barrier below
  const int last = (p + i) / AP_SPAN;   // < n_spans: p + i < S_max
  constexpr long SPAN_STRIDE = AT_T * AP_SLOT;
  const float* slot = ws + ((long)bh * gridDim.x + blockIdx.x) * n_spans * SPAN_STRIDE + r * AP_SLOT;
  float M = -INFINITY;
  for (int s = j; s <= last; s += 16) M = fmaxf(M, slot[s * SPAN_STRIDE]);
#pragma unroll
  for (int off = 1; off < 16; off <<= 1) M = fmaxf(M, __shfl_xor(M, off, 64));   // a max does not depend on the order
  const int c0 = 2 + 2 * j, c1 = 2 + 32 + 2 * j;
  float wgt = __expf(slot[0] - M);
  float L = slot[1] * wgt;
  float2 a0 = *reinterpret_cast<const float2*>(slot + c0), a1 = *reinterpret_cast<const float2*>(slot + c1);
  float acc[4] = {a0.x * wgt, a0.y * wgt, a1.x * wgt, a1.y * wgt};
  for (int s0 = 1; s0 <= last; s0 += AP_CB) {
    float pm[AP_CB], pl[AP_CB];
    float2 po0[AP_CB], po1[AP_CB];
#pragma unroll
    for (int k = 0; k < AP_CB; ++k) {
      const float* s = slot + min(s0 + k, last) * SPAN_STRIDE;
      pm[k] = s[0];
      pl[k] = s[1];
      po0[k] = *reinterpret_cast<const float2*>(s + c0);
      po1[k] = *reinterpret_cast<const float2*>(s + c1);
    }
#pragma unroll
    for (int k = 0; k < AP_CB; ++k) {
      if (s0 + k <= last) {
        wgt = __expf(pm[k] - M);
        L += pl[k] * wgt;
        acc[0] += po0[k].x * wgt;
        acc[1] += po0[k].y * wgt;
        acc[2] += po1[k].x * wgt;
        acc[3] += po1[k].y * wgt;
      }
    }
  }
  const float inv = 1.f / L;
  bf16_t* row = out + ((long)b * C + i) * (H * AT_D) + h * AT_D;
  row[2 * j] = f2bf(acc[0] * inv);
  row[2 * j + 1] = f2bf(acc[1] * inv);
  row[32 + 2 * j] = f2bf(acc[2] * inv);
  row[33 + 2 * j] = f2bf(acc[3] * inv);
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
  hipLaunchKernelGGL((attn_append_kernel<ROWS, false, false>), dim3((C + AT_T - 1) / AT_T, B * H), dim3(256), 0,
                     static_cast<hipStream_t>(stream), static_cast<const bf16_t*>(qkv), static_cast<bf16_t*>(k_cache),
                     static_cast<bf16_t*>(v_cache), static_cast<bf16_t*>(o), pos, count, C, H, S_max, scale,
                     static_cast<float*>(nullptr), static_cast<float*>(nullptr));
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

// The FP8 launchers: attn_append_launch's checks and codes, with -2 also for a null scale pointer and -6
// for caches off an 8-byte or scales off a 4-byte boundary.
template <bool ROWS>
static int attn_append_fp8_launch(const void* qkv, void* k_cache, void* v_cache, float* k_scale, float* v_scale,
                                  void* o, const int* pos, const int* count, int B, int C, int H, int Dh, int S_max,
                                  float scale, void* stream) {
  if (Dh != AT_D) return -3;
  if (S_max < 1 || S_max > AP_SMAX) return -4;
  if (C < 1 || C > AP_CMAX) return -11;
  if (B < 0 || H < 1 || (long)B * H > 65535) return -5;
  if (!qkv || !k_cache || !v_cache || !k_scale || !v_scale || !o || !pos || (ROWS && !count)) return -2;
  if (misaligned16(qkv) || misaligned8(k_cache) || misaligned8(v_cache) || misaligned4(k_scale) ||
      misaligned4(v_scale))
    return -6;
  if (B == 0) return 0;
  hipLaunchKernelGGL((attn_append_kernel<ROWS, false, true>), dim3((C + AT_T - 1) / AT_T, B * H), dim3(256), 0,
                     static_cast<hipStream_t>(stream), static_cast<const bf16_t*>(qkv),
                     static_cast<uint8_t*>(k_cache), static_cast<uint8_t*>(v_cache), static_cast<bf16_t*>(o), pos,
                     count, C, H, S_max, scale, k_scale, v_scale);
  return HIP_LAUNCH_CHECK();
}

// jdt_attn_append on an FP8 cache: caches [B, H, S_max, Dh] e4m3 bytes, k_scale / v_scale fp32 [B, H, S_max]
JDT_API int jdt_attn_append_fp8(const void* qkv, void* k_cache, void* v_cache, float* k_scale, float* v_scale,
                                void* o, const int* pos, int B, int C, int H, int Dh, int S_max, float scale,
                                void* stream) {
  return attn_append_fp8_launch<false>(qkv, k_cache, v_cache, k_scale, v_scale, o, pos, nullptr, B, C, H, Dh, S_max,
                                       scale, stream);
}

// one position and one token count (0..C) per sequence: pos int32[B], count int32[B]
JDT_API int jdt_attn_append_fp8_rows(const void* qkv, void* k_cache, void* v_cache, float* k_scale, float* v_scale,
                                     void* o, const int* pos, const int* count, int B, int C, int H, int Dh,
                                     int S_max, float scale, void* stream) {
  return attn_append_fp8_launch<true>(qkv, k_cache, v_cache, k_scale, v_scale, o, pos, count, B, C, H, Dh, S_max,
                                      scale, stream);
}

// Split-KV: the split launch, then the combine on the same stream.  The checks and codes of
// attn_append_launch, plus -2 for a null ws and -10 for a workspace below B * H * ceil(C / 64) *
// ceil(S_max / 512) * 64 * 66 floats; everything is checked before anything is launched.
template <bool ROWS>
static int attn_append_split_launch(const void* qkv, void* k_cache, void* v_cache, void* o, const int* pos,
                                    const int* count, float* ws, long ws_floats, int B, int C, int H, int Dh, int S_max,
                                    float scale, void* stream) {
  if (Dh != AT_D) return -3;
  if (S_max < 1 || S_max > AP_SMAX) return -4;
  if (C < 1 || C > AP_CMAX) return -11;
  if (B < 0 || H < 1 || (long)B * H > 65535) return -5;
  if (!qkv || !k_cache || !v_cache || !o || !pos || (ROWS && !count) || !ws) return -2;
  if (misaligned16(qkv) || misaligned16(k_cache) || misaligned16(v_cache)) return -6;
  const int n_qt = (C + AT_T - 1) / AT_T, n_spans = (S_max + AP_SPAN - 1) / AP_SPAN;
  if (ws_floats < (long)B * H * n_qt * n_spans * AT_T * AP_SLOT) return -10;
  if (B == 0) return 0;
  hipLaunchKernelGGL((attn_append_kernel<ROWS, true, false>), dim3(n_qt, B * H, n_spans), dim3(256), 0,
                     static_cast<hipStream_t>(stream), static_cast<const bf16_t*>(qkv), static_cast<bf16_t*>(k_cache),
                     static_cast<bf16_t*>(v_cache), ws, pos, count, C, H, S_max, scale, static_cast<float*>(nullptr),
                     static_cast<float*>(nullptr));
  const int rc = HIP_LAUNCH_CHECK();
  if (rc) return rc;
  hipLaunchKernelGGL(attn_append_combine_kernel<ROWS>, dim3(n_qt, B * H), dim3(1024), 0,
                     static_cast<hipStream_t>(stream), static_cast<const float*>(ws), static_cast<bf16_t*>(o), pos,
                     count, C, H, S_max, n_spans);
  return HIP_LAUNCH_CHECK();
}

// jdt_attn_append through the split-KV pair: ws is fp32 scratch of ws_floats >= B * H * ceil(C / 64) *
// ceil(S_max / 512) * 64 * 66 words (any contents; one slot per row of a workgroup of the split launch)
JDT_API int jdt_attn_append_split(const void* qkv, void* k_cache, void* v_cache, void* o, const int* pos, float* ws,
                                  long ws_floats, int B, int C, int H, int Dh, int S_max, float scale, void* stream) {
  return attn_append_split_launch<false>(qkv, k_cache, v_cache, o, pos, nullptr, ws, ws_floats, B, C, H, Dh, S_max,
                                         scale, stream);
}

// as jdt_attn_append_split with one position and one token count per sequence: pos int32[B], count int32[B]
JDT_API int jdt_attn_append_split_rows(const void* qkv, void* k_cache, void* v_cache, void* o, const int* pos,
                                       const int* count, float* ws, long ws_floats, int B, int C, int H, int Dh,
                                       int S_max, float scale, void* stream) {
  return attn_append_split_launch<true>(qkv, k_cache, v_cache, o, pos, count, ws, ws_floats, B, C, H, Dh, S_max,
                                        scale, stream);
}
