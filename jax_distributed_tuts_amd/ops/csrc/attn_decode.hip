// Autoregressive decode kernels: one new token per sequence against a KV cache.
//
// The three launchers of a decode step share one device word, ``pos`` (int32[1]): the
// number of tokens already in the cache == the index of the token being processed.
// Every kernel READS it from memory, so a captured step replays with no host
// bookkeeping (like the trainers' device step counter); jdt_sample, the last launch
// of a step, advances it.  A position outside the cache makes every kernel a no-op.
//
// Per-row variants (the ``_rows`` launchers, the same kernel bodies with ROWS = true): the
// state is one word per sequence, ``pos`` int32[B], plus ``end`` int32[B], one past the last
// token index row b may hold.  Workgroup (b, ...) reads pos[b]; a row out of range is a
// no-op for its own workgroups only.  jdt_sample_rows writes tokens[b, pos[b] + 1] and
// advances pos[b] while pos[b] + 1 < min(end[b], S_max); a written token equal to
// ``eos_id`` sets end[b] = pos[b] + 2, which finishes the row: later steps re-process the
// token at the frozen pos[b] (the same bits again) and the sampler skips the row.
// For a row whose position equals the shared one both variants give the same bits.
//
// attn_decode:  single-query attention.  M = 1: latency / memory bound, no MFMA and no
//               LDS staging -- each cached K / V row goes straight to VGPRs with one
//               16-byte load per 8 lanes' slice and is read exactly once.  Caches of up to
//               AD_SMAX rows: one launch.  Longer caches (the ``_long`` launchers, up to
//               AD_LONG_SMAX rows): the same body once per 128-key chunk (split-KV), each
//               workgroup leaving an unnormalised partial in a workspace slot, then a second
//               launch that folds the partials -- the kernel boundary is the hand-off.
// embed_decode: x[b] = wte[tokens[b, pos]] + wpe[pos]   (the bits embed_fwd_kernel stores)
// embed_append: the same for a block of C tokens per sequence from pos on (attn_append.hip's input)
// sample:       argmax (temperature 0) or inverse-CDF sampling of softmax(logits / T),
//               optionally restricted to the top-k / top-p set (FILT = true); the argmax, the
//               threshold and the draw are row_select.h's, shared with the speculative judge
#include "common.h"
#include "kv_fp8.h"
#include "row_select.h"

#include <limits.h>

#include <type_traits>

namespace jdt {

constexpr int AD_DH = 64;      // head dim (8 lanes x 8 bf16 = one 128-byte row)
constexpr int AD_SMAX = 128;   // cache rows per head the kernel covers
constexpr int AD_KPP = 32;     // keys per pass: 256 threads / 8 lanes per key
constexpr int AD_NP = AD_SMAX / AD_KPP;
constexpr int AD_CHUNK = AD_KPP * AD_NP;   // keys per workgroup of the split-KV launch
constexpr int AD_LONG_SMAX = 32768;        // cache rows per head the split-KV launchers cover
constexpr int AD_SLOT = 2 + AD_DH;         // fp32 words of a partial: max, sum, unnormalised o[64]
constexpr int AD_CB = 8;                   // partials the combine loads at a time

// sum over the 8 lanes of an aligned lane octet (all lanes active): the first three
// steps of wave_sum_dpp; every lane of the octet gets the same value
__device__ __forceinline__ float oct_sum_dpp(float v) {
  v += dpp_mov<0xB1>(v);   // quad_perm [1,0,3,2]
  v += dpp_mov<0x4E>(v);   // quad_perm [2,3,0,1]
  v += dpp_mov<0x141>(v);  // row_half_mirror
  return v;
}

// One workgroup per (batch, head).  Thread t: key group g = t / 8 (keys g, g + 32, ...),
// column slice c = t % 8 (8 bf16 = 16 bytes of the 64-wide row).  Order: the token's k / v
// rows go to the cache at row pos (and are used from registers, not read back), scores
// over keys 0..pos, fp32 softmax statistics, p = exp(s - max) rounded to bf16 before P.V and
// the fp32 sum scaled by 1 / l at the end (the rounding points of the training forward,
// attn128.hip), o stored as bf16.
//
// SPLIT: workgroup (bh, blockIdx.y = ch) does the same over the keys of chunk ch, rows
// [128 ch, min(128 ch + 128, pos + 1)), and returns at once when the chunk starts past the
// position.  Below, ``pos`` is the position relative to the chunk's first row: >= AD_CHUNK for a
// chunk that is full (every row comes from the cache, nothing is appended), else the chunk holds
// the token itself.  Instead of normalising, the workgroup stores its partial into workspace
// slot (bh, ch): the chunk's max m, l = sum exp(s - m) and the unnormalised fp32 o[64].
// The grid, (B * H, ceil(S_max / AD_CHUNK)), depends on the cache's shape only, never on pos.
// ``o`` is unused with SPLIT and ``ws`` without it.
//
// FP8 (the ``_fp8`` launchers; kv_fp8.h has the format): the caches are e4m3 bytes, 64 per row, with one
// fp32 power-of-two scale per row in ``ksc`` / ``vsc`` [B, H, S_max].  A lane's slice of a cached row is one
// 8-byte load plus the row's scale word; the token's k / v are quantized in registers (amax over the key's
// lane octet), one octet stores the 64 bytes and one lane each scale, and the workgroup itself uses the
// token as it will be read back.  The bytes stay packed until their use; a row's scale goes on its score
// and on its p instead of on its 8 values -- a power of two, so the same bits.  FP8 = false is the bf16
// kernel (``ksc`` / ``vsc`` are null and unused): every FP8 statement is under ``if constexpr``.
template <bool ROWS, bool SPLIT, bool FP8>
__global__ void __launch_bounds__(256)
attn_decode_kernel(const bf16_t* __restrict__ qkv, std::conditional_t<FP8, uint8_t, bf16_t>* __restrict__ kc,
                   std::conditional_t<FP8, uint8_t, bf16_t>* __restrict__ vc, bf16_t* __restrict__ o,
                   const int* __restrict__ pos_ptr, int H, int S_max, float scale, float* __restrict__ ws,
                   float* __restrict__ ksc, float* __restrict__ vsc) {
  using row_t = std::conditional_t<FP8, u32x2, u32x4>;   // a lane's 8 values of a row: 8 e4m3 or 8 bf16
  __shared__ float red_m[4], red_l[4], red_o[4][AD_DH];
  const int bh = blockIdx.x, b = bh / H, h = bh % H;
  const int tok_pos = pos_ptr[ROWS ? b : 0];
  if (tok_pos < 0 || tok_pos >= S_max) return;   // past the end: nothing is written (uniform over the workgroup)
  const int row0 = SPLIT ? (int)blockIdx.y * AD_CHUNK : 0;
  if (SPLIT && row0 > tok_pos) return;   // a chunk past the position: no partial, its slot is never read
  const int pos = tok_pos - row0;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, c = tid & 7, g = tid >> 3;
  const long d = (long)H * AD_DH;
  const bf16_t* row = qkv + (long)b * 3 * d + h * AD_DH + c * 8;
  const u32x4 qv = *reinterpret_cast<const u32x4*>(row);
  const u32x4 kn = *reinterpret_cast<const u32x4*>(row + d);
  const u32x4 vn = *reinterpret_cast<const u32x4*>(row + 2 * d);
  auto* Kh = kc + (long)bh * S_max * AD_DH + c * 8;   // SPLIT: the chunk's first row
  auto* Vh = vc + (long)bh * S_max * AD_DH + c * 8;
  if (SPLIT) {
    Kh += (long)row0 * AD_DH;
    Vh += (long)row0 * AD_DH;
  }
  // FP8: the scales of this head's rows (SPLIT: from the chunk's first row on)
  float* Ksc = nullptr;
  float* Vsc = nullptr;
  if constexpr (FP8) {
    Ksc = ksc + (long)bh * S_max + row0;
    Vsc = vsc + (long)bh * S_max + row0;
  }
  // every load of the step is issued before the first use; rows past pos are never read
  row_t kr[AD_NP], vr[AD_NP];
  float ks[FP8 ? AD_NP : 1], vs[FP8 ? AD_NP : 1];   // FP8: the rows' scales
  if constexpr (FP8) {
    // the cache loads go out first; quantizing the token then waits for kn / vn (issued before them) only
#pragma unroll
    for (int i = 0; i < AD_NP; ++i) {
      const int j = g + AD_KPP * i;
      if (j < pos) {
        kr[i] = *reinterpret_cast<const row_t*>(Kh + (long)j * AD_DH);
        vr[i] = *reinterpret_cast<const row_t*>(Vh + (long)j * AD_DH);
        ks[i] = Ksc[j];
        vs[i] = Vsc[j];
      }
    }
    // the token's rows as the cache will hold them: every octet has the whole row and quantizes it
    float kts, vts;
    const row_t kt = kv_quantize8(kn, kts), vt = kv_quantize8(vn, vts);
#pragma unroll
    for (int i = 0; i < AD_NP; ++i) {
      if (g + AD_KPP * i >= pos) {   // j == pos: the token itself; j > pos: masked below
        kr[i] = kt;
        vr[i] = vt;
        ks[i] = kts;
        vs[i] = vts;
      }
    }
    if ((!SPLIT || pos < AD_CHUNK) && g == (pos & (AD_KPP - 1))) {
      *reinterpret_cast<row_t*>(Kh + (long)pos * AD_DH) = kt;
      *reinterpret_cast<row_t*>(Vh + (long)pos * AD_DH) = vt;
      if (c == 0) {
        Ksc[pos] = kts;
        Vsc[pos] = vts;
      }
    }
  } else {
#pragma unroll
    for (int i = 0; i < AD_NP; ++i) {
      const int j = g + AD_KPP * i;
      if (j < pos) {
        kr[i] = *reinterpret_cast<const u32x4*>(Kh + (long)j * AD_DH);
        vr[i] = *reinterpret_cast<const u32x4*>(Vh + (long)j * AD_DH);
      } else {
        kr[i] = kn;   // j == pos: the token itself; j > pos: masked below
        vr[i] = vn;
      }
    }
    if ((!SPLIT || pos < AD_CHUNK) && g == (pos & (AD_KPP - 1))) {
      *reinterpret_cast<u32x4*>(Kh + (long)pos * AD_DH) = kn;
      *reinterpret_cast<u32x4*>(Vh + (long)pos * AD_DH) = vn;
    }
  }
  float qf[8];
  unpack8(qv, qf);
  float s[AD_NP], m = -INFINITY;
#pragma unroll
  for (int i = 0; i < AD_NP; ++i) {
    float kf[8], dot = 0.f;
    if constexpr (FP8) fp8_unpack8(kr[i], kf);
    else unpack8(kr[i], kf);
#pragma unroll
    for (int e = 0; e < 8; ++e) dot += qf[e] * kf[e];
    dot = oct_sum_dpp(dot);
    if constexpr (FP8) dot *= ks[i];   // exact: a power of two
    s[i] = (g + AD_KPP * i <= pos) ? dot * scale : -INFINITY;
    m = fmaxf(m, s[i]);
  }
  m = wave_max_dpp(m);
  if (lane == 0) red_m[w] = m;
  __syncthreads();
  m = fmaxf(fmaxf(red_m[0], red_m[1]), fmaxf(red_m[2], red_m[3]));   // finite: key 0 is always valid
  float l = 0.f;
#pragma unroll
  for (int i = 0; i < AD_NP; ++i) {
    s[i] = (g + AD_KPP * i <= pos) ? __expf(s[i] - m) : 0.f;
    l += s[i];
  }
  l = wave_sum_dpp(c == 0 ? l : 0.f);   // one lane per key
  if (lane == 0) red_l[w] = l;
  __syncthreads();
  l = (red_l[0] + red_l[1]) + (red_l[2] + red_l[3]);
  float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int i = 0; i < AD_NP; ++i) {
    float p = round_bf(s[i]);   // exp(s - m) as bf16; 1 / l goes on the fp32 sum, as in attn128.hip
    float vf[8];
    if constexpr (FP8) {
      fp8_unpack8(vr[i], vf);
      p *= vs[i];   // exact: a power of two
    } else {
      unpack8(vr[i], vf);
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[e] += p * vf[e];
  }
  // the 8 key groups of a wave (lanes c, c + 8, ...), then the 4 waves through LDS
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    float a = acc[e];
    a += __shfl_xor(a, 8, WAVE);
    a += __shfl_xor(a, 16, WAVE);
    a += __shfl_xor(a, 32, WAVE);
    if (lane < 8) red_o[w][lane * 8 + e] = a;
  }
  __syncthreads();
  if (tid < AD_DH) {
    if (SPLIT) {
      float* slot = ws + ((long)bh * gridDim.y + blockIdx.y) * AD_SLOT;
      if (tid == 0) {
        slot[0] = m;
        slot[1] = l;
      }
      slot[2 + tid] = (red_o[0][tid] + red_o[1][tid]) + (red_o[2][tid] + red_o[3][tid]);
    } else {
      const float inv = 1.f / l;
      o[(long)b * d + h * AD_DH + tid] =
          f2bf(((red_o[0][tid] + red_o[1][tid]) + (red_o[2][tid] + red_o[3][tid])) * inv);
    }
  }
}

// The second launch of the split-KV path: one wave per (batch, head), lane t owns column t.
// Folds the partials of chunks 0..pos / 128 in increasing order: M = max m_c, L = sum l_c e^(m_c - M),
// o = (sum o_c e^(m_c - M)) * (1 / L), stored as bf16.  Slots past pos / 128 are never read (stale
// workspace contents are harmless) and a position outside the cache leaves o as it is.  One chunk:
// e^0 = 1, so this is o_0 * (1 / l_0) -- the expression and the bits of attn_decode_kernel.
template <bool ROWS>
__global__ void __launch_bounds__(WAVE) attn_decode_combine_kernel(const float* __restrict__ ws,
                                                                  bf16_t* __restrict__ o,
                                                                  const int* __restrict__ pos_ptr, int H, int S_max,
                                                                  int n_chunks) {
  const int bh = blockIdx.x, b = bh / H, h = bh % H, t = threadIdx.x;
  const int pos = pos_ptr[ROWS ? b : 0];
  if (pos < 0 || pos >= S_max) return;
  const int last = pos / AD_CHUNK;   // < n_chunks: pos < S_max
  const float* slot = ws + (long)bh * n_chunks * AD_SLOT;
  float M = -INFINITY;
  for (int ch = t; ch <= last; ch += WAVE) M = fmaxf(M, slot[(long)ch * AD_SLOT]);
  M = wave_max_dpp(M);   // every lane gets the same value; a max does not depend on the order
  float wgt = __expf(slot[0] - M);
  float L = slot[1] * wgt, acc = slot[2 + t] * wgt;
  // eight chunks' loads in flight at a time (a load per iteration would pay its latency pos / 128
  // times in a row); the fold itself stays in increasing chunk order.  A block's tail past
  // ``last`` re-reads slot ``last`` and is not folded.
  for (int c0 = 1; c0 <= last; c0 += AD_CB) {
    float pm[AD_CB], pl[AD_CB], po[AD_CB];
#pragma unroll
    for (int k = 0; k < AD_CB; ++k) {
      const float* s = slot + (long)min(c0 + k, last) * AD_SLOT;
      pm[k] = s[0];
      pl[k] = s[1];
      po[k] = s[2 + t];
    }
#pragma unroll
    for (int k = 0; k < AD_CB; ++k) {
      if (c0 + k <= last) {
        wgt = __expf(pm[k] - M);
        L += pl[k] * wgt;
        acc += po[k] * wgt;
      }
    }
  }
  o[((long)b * H + h) * AD_DH + t] = f2bf(acc * (1.f / L));
}

// one thread per 8 columns, as embed_fwd_kernel (same bf16x8_add -> same bits)
template <bool ROWS>
__global__ void __launch_bounds__(256) embed_decode_kernel(const int* __restrict__ tokens,
                                                          const bf16_t* __restrict__ wte,
                                                          const bf16_t* __restrict__ wpe, bf16_t* __restrict__ out,
                                                          const int* __restrict__ pos_ptr, int B, int S_max, int d,
                                                          int vocab) {
  const int i = blockIdx.x * 256 + threadIdx.x, per_row = d / 8;
  if (i >= B * per_row) return;
  const int b = i / per_row, c = (i % per_row) * 8;
  const int pos = pos_ptr[ROWS ? b : 0];
  if (pos < 0 || pos >= S_max) return;
  const int v = tokens[(long)b * S_max + pos];
  if ((unsigned)v >= (unsigned)vocab) return;   // never read outside the table
  const u32x4 a = *reinterpret_cast<const u32x4*>(wte + (long)v * d + c);
  const u32x4 p = *reinterpret_cast<const u32x4*>(wpe + (long)pos * d + c);
  *reinterpret_cast<u32x4*>(out + (long)b * d + c) = bf16x8_add(a, p);
}

// embed_decode for a block of C tokens per sequence (the input of attn_append.hip's step):
// out[b*C + i] = wte[tokens[b, p + i]] + wpe[p + i] for i < n, with p = pos[b] and n = count[b]
// (shared position: pos[0] and n = C).  Rows i >= n keep their contents; p < 0, p + n > S_max or
// n outside 0..C: nothing is written for the sequence.  One thread per 8 columns, as above.
template <bool ROWS>
__global__ void __launch_bounds__(256) embed_append_kernel(const int* __restrict__ tokens,
                                                          const bf16_t* __restrict__ wte,
                                                          const bf16_t* __restrict__ wpe, bf16_t* __restrict__ out,
                                                          const int* __restrict__ pos_ptr,
                                                          const int* __restrict__ count, int B, int C, int S_max,
                                                          int d, int vocab) {
  const int per_row = d / 8;
  const long t = (long)blockIdx.x * 256 + threadIdx.x;
  if (t >= (long)B * C * per_row) return;
  const int row = (int)(t / per_row), c = (int)(t % per_row) * 8;   // row = b * C + i < B * C <= INT_MAX
  const int b = row / C, i = row % C;
  const int p = pos_ptr[ROWS ? b : 0], n = ROWS ? count[b] : C;
  if (n < 0 || n > C || p < 0 || p > S_max - n || i >= n) return;
  const int v = tokens[(long)b * S_max + p + i];
  if ((unsigned)v >= (unsigned)vocab) return;   // never read outside the table
  const u32x4 a = *reinterpret_cast<const u32x4*>(wte + (long)v * d + c);
  const u32x4 e = *reinterpret_cast<const u32x4*>(wpe + (long)(p + i) * d + c);
  *reinterpret_cast<u32x4*>(out + (long)row * d + c) = bf16x8_add(a, e);
}

// One workgroup per row; thread t owns the contiguous columns [t * per, (t + 1) * per).
// temperature == 0: argmax, lowest index on ties.  Otherwise inverse-CDF sampling: weights
// w_i = exp((x_i - max) / T) in fp32, a fixed-order prefix sum over the threads' chunk sums,
// target = u * total with u = word 0 of philox4x32(seed, b, (pos << 32) | stream) as 24 bits;
// the first thread whose inclusive prefix exceeds the target walks its chunk to the first
// column whose running sum does.  The token goes to tokens[b, pos + 1]; the workgroup that
// takes the last arrival ticket (optim.hip's scheme: every workgroup has read pos by then)
// stores pos + 1 and re-arms the ticket.  pos + 1 >= S_max: nothing is written at all.
//
// ROWS: the position is pos[b] and the row is live while pos[b] + 1 < min(end[b], S_max).  Only
// workgroup b touches pos[b] / end[b], so there is no ticket: the thread that stores the token
// also stores pos[b] + 1 and, for a token equal to eos_id >= 0, end[b] = pos[b] + 2.
//
// FILT (temperature > 0 and top-k or top-p on): the weights of columns below the threshold
// key max(key_k, key_p) are 0 and everything else runs as above.  key_k is the key of the
// k-th largest logit (ties kept), key_p the largest key whose mass over {key >= key_p} is
// >= top_p * (mass of the top-k set) (ties kept).
template <bool ROWS, bool FILT>
__global__ void __launch_bounds__(256) sample_kernel(const bf16_t* __restrict__ logits, long ld, int V,
                                                    float temperature, unsigned long long seed, unsigned stream_id,
                                                    int* __restrict__ tokens, int S_max, int* pos_ptr,
                                                    unsigned* ticket, int vec, int* end_ptr, int eos_id, int top_k,
                                                    float top_p) {
  const int tid = threadIdx.x, b = blockIdx.x;
  const int pos = pos_ptr[ROWS ? b : 0];
  if (ROWS) {
    if (pos < 0 || pos + 1 >= min(end_ptr[b], S_max)) return;   // finished or full: uniform over the workgroup
  } else {
    if (pos < 0 || pos + 1 >= S_max) return;   // uniform over the grid: the ticket stays armed at 0
  }
  // the one thread that stores the row's token; ROWS: it also advances / finishes the row
  // (every thread has read pos[b] and end[b] before the first barrier, all stores come after it)
  auto emit = [&](int tok) {
    tokens[(long)b * S_max + pos + 1] = tok;
    if (ROWS) {
      pos_ptr[b] = pos + 1;
      if (eos_id >= 0 && tok == eos_id) end_ptr[b] = pos + 2;
    }
  };
  const bf16_t* row = logits + (long)b * ld;
  const int per = (((V + 255) / 256) + 7) & ~7;
  const int beg = tid * per, end = min(beg + per, V);
  float gmx;
  const int gam = row_argmax(row, V, vec, beg, end, gmx);
  if (temperature <= 0.f) {
    if (tid == 0) emit(gam);
  } else {
    const float inv_t = 1.f / temperature;
    unsigned thr = 0;   // FILT: columns whose key is below it weigh 0
    if (FILT) thr = filter_threshold(row, V, vec, beg, end, gmx, inv_t, top_k, top_p);
    const u32x4 r = philox4x32(seed, (uint64_t)b, ((uint64_t)(unsigned)pos << 32) | (uint64_t)stream_id);
    const int tok = row_draw<FILT, false>(row, V, vec, beg, end, gmx, gam, inv_t, thr, r.x, -1);
    if (tok >= 0) emit(tok);   // one thread
  }
  if (ROWS) return;
  __syncthreads();
  if (tid == 0) {
    const unsigned t = atomicAdd(ticket, 1u);
    if (t == gridDim.x - 1) {
      pos_ptr[0] = pos + 1;
      __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
}

}  // namespace jdt
using namespace jdt;

template <bool ROWS>
static int attn_decode_launch(const void* qkv, void* k_cache, void* v_cache, void* o, const int* pos, int B, int H,
                              int Dh, int S_max, float scale, void* stream) {
  if (Dh != AD_DH) return -3;
  if (S_max < 1 || S_max > AD_SMAX) return -4;
  if (B < 0 || H < 1) return -5;
  if (!qkv || !k_cache || !v_cache || !o || !pos) return -2;
  if (misaligned16(qkv) || misaligned16(k_cache) || misaligned16(v_cache)) return -6;
  if (B == 0) return 0;
  hipLaunchKernelGGL((attn_decode_kernel<ROWS, false, false>), dim3(B * H), dim3(256), 0,
                     static_cast<hipStream_t>(stream), static_cast<const bf16_t*>(qkv),
                     static_cast<bf16_t*>(k_cache), static_cast<bf16_t*>(v_cache), static_cast<bf16_t*>(o), pos, H,
                     S_max, scale, static_cast<float*>(nullptr), static_cast<float*>(nullptr),
                     static_cast<float*>(nullptr));
  return HIP_LAUNCH_CHECK();
}

// qkv [B, 3*H*Dh] bf16 (q | k | v), caches [B, H, S_max, Dh] bf16, o [B, H*Dh] bf16, pos int32[1]
JDT_API int jdt_attn_decode(const void* qkv, void* k_cache, void* v_cache, void* o, const int* pos, int B, int H,
                            int Dh, int S_max, float scale, void* stream) {
  return attn_decode_launch<false>(qkv, k_cache, v_cache, o, pos, B, H, Dh, S_max, scale, stream);
}

// as jdt_attn_decode with one position per sequence: pos int32[B]
JDT_API int jdt_attn_decode_rows(const void* qkv, void* k_cache, void* v_cache, void* o, const int* pos, int B, int H,
                                 int Dh, int S_max, float scale, void* stream) {
  return attn_decode_launch<true>(qkv, k_cache, v_cache, o, pos, B, H, Dh, S_max, scale, stream);
}

// Split-KV: the split launch, then the combine on the same stream.  Everything is checked
// before anything is launched; -10: a workspace below B * H * ceil(S_max / 128) * 66 floats.
template <bool ROWS>
static int attn_decode_long_launch(const void* qkv, void* k_cache, void* v_cache, void* o, const int* pos, float* ws,
                                   long ws_floats, int B, int H, int Dh, int S_max, float scale, void* stream) {
  if (Dh != AD_DH) return -3;
  if (S_max < 1 || S_max > AD_LONG_SMAX) return -4;
  if (B < 0 || H < 1 || (long)B * H > INT_MAX) return -5;
  if (!qkv || !k_cache || !v_cache || !o || !pos || !ws) return -2;
  if (misaligned16(qkv) || misaligned16(k_cache) || misaligned16(v_cache)) return -6;
  const int n_chunks = (S_max + AD_CHUNK - 1) / AD_CHUNK;
  if (ws_floats < (long)B * H * n_chunks * AD_SLOT) return -10;
  if (B == 0) return 0;
  hipLaunchKernelGGL((attn_decode_kernel<ROWS, true, false>), dim3(B * H, n_chunks), dim3(256), 0,
                     static_cast<hipStream_t>(stream), static_cast<const bf16_t*>(qkv),
                     static_cast<bf16_t*>(k_cache), static_cast<bf16_t*>(v_cache), static_cast<bf16_t*>(nullptr), pos,
                     H, S_max, scale, ws, static_cast<float*>(nullptr), static_cast<float*>(nullptr));
  const int rc = HIP_LAUNCH_CHECK();
  if (rc) return rc;
  hipLaunchKernelGGL(attn_decode_combine_kernel<ROWS>, dim3(B * H), dim3(WAVE), 0, static_cast<hipStream_t>(stream),
                     static_cast<const float*>(ws), static_cast<bf16_t*>(o), pos, H, S_max, n_chunks);
  return HIP_LAUNCH_CHECK();
}

// jdt_attn_decode for caches of 1 <= S_max <= 32768 rows: ws is fp32 scratch of ws_floats >=
// B * H * ceil(S_max / 128) * 66 words (any contents; one slot per workgroup of the split launch)
JDT_API int jdt_attn_decode_long(const void* qkv, void* k_cache, void* v_cache, void* o, const int* pos, float* ws,
                                 long ws_floats, int B, int H, int Dh, int S_max, float scale, void* stream) {
  return attn_decode_long_launch<false>(qkv, k_cache, v_cache, o, pos, ws, ws_floats, B, H, Dh, S_max, scale, stream);
}

// as jdt_attn_decode_long with one position per sequence: pos int32[B]
JDT_API int jdt_attn_decode_long_rows(const void* qkv, void* k_cache, void* v_cache, void* o, const int* pos,
                                      float* ws, long ws_floats, int B, int H, int Dh, int S_max, float scale,
                                      void* stream) {
  return attn_decode_long_launch<true>(qkv, k_cache, v_cache, o, pos, ws, ws_floats, B, H, Dh, S_max, scale, stream);
}

// The FP8 launchers: the bf16 ones' checks and codes, with -2 also for a null scale pointer and -6 for
// caches off an 8-byte or scales off a 4-byte boundary.
template <bool ROWS>
static int attn_decode_fp8_launch(const void* qkv, void* k_cache, void* v_cache, float* k_scale, float* v_scale,
                                  void* o, const int* pos, int B, int H, int Dh, int S_max, float scale,
                                  void* stream) {
  if (Dh != AD_DH) return -3;
  if (S_max < 1 || S_max > AD_SMAX) return -4;
  if (B < 0 || H < 1) return -5;
  if (!qkv || !k_cache || !v_cache || !k_scale || !v_scale || !o || !pos) return -2;
  if (misaligned16(qkv) || misaligned8(k_cache) || misaligned8(v_cache) || misaligned4(k_scale) ||
      misaligned4(v_scale))
    return -6;
  if (B == 0) return 0;
  hipLaunchKernelGGL((attn_decode_kernel<ROWS, false, true>), dim3(B * H), dim3(256), 0,
                     static_cast<hipStream_t>(stream), static_cast<const bf16_t*>(qkv),
                     static_cast<uint8_t*>(k_cache), static_cast<uint8_t*>(v_cache), static_cast<bf16_t*>(o), pos, H,
                     S_max, scale, static_cast<float*>(nullptr), k_scale, v_scale);
  return HIP_LAUNCH_CHECK();
}

// jdt_attn_decode on an FP8 cache: caches [B, H, S_max, Dh] e4m3 bytes, k_scale / v_scale fp32 [B, H, S_max]
JDT_API int jdt_attn_decode_fp8(const void* qkv, void* k_cache, void* v_cache, float* k_scale, float* v_scale,
                                void* o, const int* pos, int B, int H, int Dh, int S_max, float scale,
                                void* stream) {
  return attn_decode_fp8_launch<false>(qkv, k_cache, v_cache, k_scale, v_scale, o, pos, B, H, Dh, S_max, scale,
                                       stream);
}

// as jdt_attn_decode_fp8 with one position per sequence: pos int32[B]
JDT_API int jdt_attn_decode_fp8_rows(const void* qkv, void* k_cache, void* v_cache, float* k_scale, float* v_scale,
                                     void* o, const int* pos, int B, int H, int Dh, int S_max, float scale,
                                     void* stream) {
  return attn_decode_fp8_launch<true>(qkv, k_cache, v_cache, k_scale, v_scale, o, pos, B, H, Dh, S_max, scale,
                                      stream);
}

// Split-KV on an FP8 cache: the same 128-key chunks, workspace and combine as the bf16 pair.
template <bool ROWS>
static int attn_decode_fp8_long_launch(const void* qkv, void* k_cache, void* v_cache, float* k_scale, float* v_scale,
                                       void* o, const int* pos, float* ws, long ws_floats, int B, int H, int Dh,
                                       int S_max, float scale, void* stream) {
  if (Dh != AD_DH) return -3;
  if (S_max < 1 || S_max > AD_LONG_SMAX) return -4;
  if (B < 0 || H < 1 || (long)B * H > INT_MAX) return -5;
  if (!qkv || !k_cache || !v_cache || !k_scale || !v_scale || !o || !pos || !ws) return -2;
  if (misaligned16(qkv) || misaligned8(k_cache) || misaligned8(v_cache) || misaligned4(k_scale) ||
      misaligned4(v_scale))
    return -6;
  const int n_chunks = (S_max + AD_CHUNK - 1) / AD_CHUNK;
  if (ws_floats < (long)B * H * n_chunks * AD_SLOT) return -10;
  if (B == 0) return 0;
  hipLaunchKernelGGL((attn_decode_kernel<ROWS, true, true>), dim3(B * H, n_chunks), dim3(256), 0,
                     static_cast<hipStream_t>(stream), static_cast<const bf16_t*>(qkv),
                     static_cast<uint8_t*>(k_cache), static_cast<uint8_t*>(v_cache), static_cast<bf16_t*>(nullptr),
                     pos, H, S_max, scale, ws, k_scale, v_scale);
  const int rc = HIP_LAUNCH_CHECK();
  if (rc) return rc;
  hipLaunchKernelGGL(attn_decode_combine_kernel<ROWS>, dim3(B * H), dim3(WAVE), 0, static_cast<hipStream_t>(stream),
                     static_cast<const float*>(ws), static_cast<bf16_t*>(o), pos, H, S_max, n_chunks);
  return HIP_LAUNCH_CHECK();
}

// jdt_attn_decode_long on an FP8 cache
JDT_API int jdt_attn_decode_fp8_long(const void* qkv, void* k_cache, void* v_cache, float* k_scale, float* v_scale,
                                     void* o, const int* pos, float* ws, long ws_floats, int B, int H, int Dh,
                                     int S_max, float scale, void* stream) {
  return attn_decode_fp8_long_launch<false>(qkv, k_cache, v_cache, k_scale, v_scale, o, pos, ws, ws_floats, B, H, Dh,
                                            S_max, scale, stream);
}

// as jdt_attn_decode_fp8_long with one position per sequence: pos int32[B]
JDT_API int jdt_attn_decode_fp8_long_rows(const void* qkv, void* k_cache, void* v_cache, float* k_scale,
                                          float* v_scale, void* o, const int* pos, float* ws, long ws_floats, int B,
                                          int H, int Dh, int S_max, float scale, void* stream) {
  return attn_decode_fp8_long_launch<true>(qkv, k_cache, v_cache, k_scale, v_scale, o, pos, ws, ws_floats, B, H, Dh,
                                           S_max, scale, stream);
}

template <bool ROWS>
static int embed_decode_launch(const int* tokens, const void* wte, const void* wpe, void* out, const int* pos, int B,
                               int S_max, int d, int vocab, void* stream) {
  if (d < 8 || d % 8) return -3;
  if (S_max < 1 || vocab < 1 || B < 0) return -5;
  if (!tokens || !wte || !wpe || !out || !pos) return -2;
  if (misaligned16(wte) || misaligned16(wpe) || misaligned16(out)) return -6;
  if (B == 0) return 0;
  const long n = (long)B * (d / 8);
  if (n > INT_MAX) return -5;
  hipLaunchKernelGGL(embed_decode_kernel<ROWS>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0,
                     static_cast<hipStream_t>(stream), tokens, static_cast<const bf16_t*>(wte),
                     static_cast<const bf16_t*>(wpe), static_cast<bf16_t*>(out), pos, B, S_max, d, vocab);
  return HIP_LAUNCH_CHECK();
}

// out [B, d] bf16 = wte[tokens[b, pos]] + wpe[pos]; tokens int32 [B, S_max]; wpe has >= S_max rows
JDT_API int jdt_embed_decode(const int* tokens, const void* wte, const void* wpe, void* out, const int* pos, int B,
                             int S_max, int d, int vocab, void* stream) {
  return embed_decode_launch<false>(tokens, wte, wpe, out, pos, B, S_max, d, vocab, stream);
}

// as jdt_embed_decode with one position per sequence: pos int32[B]
JDT_API int jdt_embed_decode_rows(const int* tokens, const void* wte, const void* wpe, void* out, const int* pos,
                                  int B, int S_max, int d, int vocab, void* stream) {
  return embed_decode_launch<true>(tokens, wte, wpe, out, pos, B, S_max, d, vocab, stream);
}

// -11: C outside 1..1024 (the envelope of jdt_attn_append)
template <bool ROWS>
static int embed_append_launch(const int* tokens, const void* wte, const void* wpe, void* out, const int* pos,
                               const int* count, int B, int C, int S_max, int d, int vocab, void* stream) {
  if (d < 8 || d % 8) return -3;
  if (C < 1 || C > 1024) return -11;
  if (S_max < 1 || vocab < 1 || B < 0 || (long)B * C > INT_MAX) return -5;
  if (!tokens || !wte || !wpe || !out || !pos || (ROWS && !count)) return -2;
  if (misaligned16(wte) || misaligned16(wpe) || misaligned16(out)) return -6;
  if (B == 0) return 0;
  const long blocks = ((long)B * C * (d / 8) + 255) / 256;
  if (blocks > INT_MAX) return -5;
  hipLaunchKernelGGL(embed_append_kernel<ROWS>, dim3((unsigned)blocks), dim3(256), 0, static_cast<hipStream_t>(stream),
                     tokens, static_cast<const bf16_t*>(wte), static_cast<const bf16_t*>(wpe),
                     static_cast<bf16_t*>(out), pos, count, B, C, S_max, d, vocab);
  return HIP_LAUNCH_CHECK();
}

// out [B*C, d] bf16: row b*C + i = wte[tokens[b, pos + i]] + wpe[pos + i]; tokens int32 [B, S_max]; pos int32[1]
JDT_API int jdt_embed_append(const int* tokens, const void* wte, const void* wpe, void* out, const int* pos, int B,
                             int C, int S_max, int d, int vocab, void* stream) {
  return embed_append_launch<false>(tokens, wte, wpe, out, pos, nullptr, B, C, S_max, d, vocab, stream);
}

// one position and one token count (0..C) per sequence: pos int32[B], count int32[B]
JDT_API int jdt_embed_append_rows(const int* tokens, const void* wte, const void* wpe, void* out, const int* pos,
                                  const int* count, int B, int C, int S_max, int d, int vocab, void* stream) {
  return embed_append_launch<true>(tokens, wte, wpe, out, pos, count, B, C, S_max, d, vocab, stream);
}

// The checks and the launch of the three sampler entry points.  ROWS: ``end`` in the place of
// ``ticket``.  top_k = 0 (or >= V) and top_p = 1 are "off"; with both off, or at temperature 0
// (greedy), the unfiltered kernel runs.
template <bool ROWS>
static int sample_launch(const void* logits, long ld, int B, int V, float temperature, unsigned long long seed,
                         unsigned stream_id, int* tokens, int S_max, int* pos, unsigned* ticket, int* end, int eos_id,
                         int top_k, float top_p, void* stream) {
  if (V < 1 || ld < V || S_max < 1 || B < 0) return -5;
  if (!(temperature >= 0.f)) return -7;
  if (top_k < 0) return -8;
  if (!(top_p > 0.f && top_p <= 1.f)) return -9;
  if (!logits || !tokens || !pos || (ROWS ? !end : !ticket)) return -2;
  if (B == 0) return 0;
  const int vec = (V % 8 == 0) && (ld % 8 == 0) && !misaligned16(logits);
  const bool filt = temperature > 0.f && ((top_k > 0 && top_k < V) || top_p < 1.f);
  auto kernel = filt ? sample_kernel<ROWS, true> : sample_kernel<ROWS, false>;
  hipLaunchKernelGGL(kernel, dim3(B), dim3(256), 0, static_cast<hipStream_t>(stream),
                     static_cast<const bf16_t*>(logits), ld, V, temperature, seed, stream_id, tokens, S_max, pos,
                     ticket, vec, end, eos_id, top_k, top_p);
  return HIP_LAUNCH_CHECK();
}

// logits [B, V] bf16 (row stride ld); tokens int32 [B, S_max]; pos int32[1]; ticket: a zeroed
// uint32 the kernel leaves zero again
JDT_API int jdt_sample(const void* logits, long ld, int B, int V, float temperature, unsigned long long seed,
                       unsigned stream_id, int* tokens, int S_max, int* pos, unsigned* ticket, void* stream) {
  return sample_launch<false>(logits, ld, B, V, temperature, seed, stream_id, tokens, S_max, pos, ticket, nullptr, -1,
                              0, 1.f, stream);
}

// jdt_sample restricted to the top-k / top-p set: top_k >= 0 (0: off), top_p in (0, 1] (1: off)
JDT_API int jdt_sample_filtered(const void* logits, long ld, int B, int V, float temperature, unsigned long long seed,
                                unsigned stream_id, int* tokens, int S_max, int* pos, unsigned* ticket, int top_k,
                                float top_p, void* stream) {
  return sample_launch<false>(logits, ld, B, V, temperature, seed, stream_id, tokens, S_max, pos, ticket, nullptr, -1,
                              top_k, top_p, stream);
}

// one position per sequence: pos int32[B], end int32[B] (one past the last token index a row
// may hold); eos_id >= 0: a row that draws it is finished (end[b] = its length); no ticket
JDT_API int jdt_sample_rows(const void* logits, long ld, int B, int V, float temperature, unsigned long long seed,
                            unsigned stream_id, int* tokens, int S_max, int* pos, int* end, int eos_id, int top_k,
                            float top_p, void* stream) {
  return sample_launch<true>(logits, ld, B, V, temperature, seed, stream_id, tokens, S_max, pos, nullptr, end, eos_id,
                             top_k, top_p, stream);
}
