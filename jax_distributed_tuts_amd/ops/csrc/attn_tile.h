// The tile-streaming attention core shared by flash_attn.hip (training forward and both backward
// kernels) and attn_append.hip (chunked prefill): head dim 64, 64 x 64 tiles, a wave owns 16 rows.
//
// Written once here, so the kernels agree bit for bit by construction: fp32 scores and softmax
// statistics, p rounded to bf16 before P V, 1 / l applied to the fp32 sum, and the
// ``mnew == -inf`` guards that make a fully masked tile an exact no-op.  The kernels keep what
// differs between them: which rows a tile is staged from and when (direct or register prefetch),
// the mask's last visible key, the LSE store, how dQ is formed.
#pragma once

#include "common.h"

namespace jdt {

constexpr int AT_D = 64;          // head dim
constexpr int AT_T = 64;          // query / key tile
constexpr int AT_LD = AT_T + 8;   // padded LDS row (bf16 elements)

__device__ __forceinline__ bf16x8 ld8(const bf16_t* p) { return *reinterpret_cast<const bf16x8*>(p); }

// ---------------------------------------------------------------- staging
// One 16-byte chunk (row r, columns dc .. dc + 7 of a [64][64] tile) -> LDS, row-major (row stride
// AT_LD) ...
__device__ __forceinline__ void lds_store_chunk(const u32x4& v, int r, int dc, bf16_t* row_major) {
  *reinterpret_cast<u32x4*>(row_major + r * AT_LD + dc) = v;
}
// ... and transposed (row stride tld, scalar writes)
__device__ __forceinline__ void lds_store_chunk_t(const u32x4& v, int r, int dc, bf16_t* transposed, int tld = AT_LD) {
  const unsigned q[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    transposed[(dc + 2 * j) * tld + r] = (bf16_t)(q[j] & 0xffff);
    transposed[(dc + 2 * j + 1) * tld + r] = (bf16_t)(q[j] >> 16);
  }
}

// stage a [64 rows][64 cols] bf16 tile (global row stride ld) into LDS with NT threads, row-major
// and/or transposed; rows >= nrows are zero
template <int NT>
__device__ __forceinline__ void stage_tile(const bf16_t* g, long ld, int nrows, bf16_t* row_major,
                                           bf16_t* transposed, int tld = AT_LD) {
  for (int c = threadIdx.x; c < AT_T * AT_D / 8; c += NT) {
    const int r = c >> 3, dc = (c & 7) * 8;
    u32x4 v = {0u, 0u, 0u, 0u};
    if (r < nrows) v = *reinterpret_cast<const u32x4*>(g + (long)r * ld + dc);
    if (row_major) lds_store_chunk(v, r, dc, row_major);
    if (transposed) lds_store_chunk_t(v, r, dc, transposed, tld);
  }
}

// ---------------------------------------------------------------- forward
// This lane's Q fragments (row lane & 15 of the wave's 16; q_row: that row's 64 columns) and the
// empty online-softmax state.  Lane layout of m / l / o: row (lane >> 4) * 4 + e.
__device__ __forceinline__ void fwd_begin(const bf16_t* q_row, bool valid, bf16x8 (&qf)[2], float (&m)[4],
                                          float (&l)[4], f32x4 (&o)[4]) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int ks = 0; ks < 2; ++ks)
    qf[ks] = valid ? ld8(q_row + ks * 32 + 8 * (lane >> 4)) : (bf16x8){0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
  for (int e = 0; e < 4; ++e) { m[e] = -INFINITY; l[e] = 0.f; }
#pragma unroll
  for (int nt = 0; nt < 4; ++nt) o[nt] = (f32x4){0.f, 0.f, 0.f, 0.f};
}

// One 64-key tile (keys k0 .. k0 + 63: Ks row-major, Vt transposed, both staged) folded into the
// wave's state.  last[e]: the last key row (lane >> 4) * 4 + e may see; Ps: this wave's P tile.
__device__ __forceinline__ void fwd_tile_step(const bf16_t* Ks, const bf16_t* Vt, bf16_t* Ps, const bf16x8 (&qf)[2],
                                              float scale, int k0, const int (&last)[4], float (&m)[4],
                                              float (&l)[4], f32x4 (&o)[4]) {
  const int lane = threadIdx.x & 63;
  // this lane's row and k-slice of an MFMA operand tile: one base per image, so the tile reads
  // below differ by compile-time offsets only
  const int frag = (lane & 15) * AT_LD + 8 * (lane >> 4);
  // S = Q K^T (16 x 64 per wave)
  f32x4 s[4];
#pragma unroll
  for (int nt = 0; nt < 4; ++nt) {
    s[nt] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ks = 0; ks < 2; ++ks)
      s[nt] = mfma16x16x32(qf[ks], ld8(Ks + frag + nt * 16 * AT_LD + ks * 32), s[nt]);
  }
  // online softmax over this tile (row r = (lane>>4)*4 + e; key column nt*16 + (lane&15))
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    float mx = -INFINITY;
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) {
      const int key = k0 + nt * 16 + (lane & 15);
      float v = s[nt][e] * scale;
      if (key > last[e]) v = -INFINITY;
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
      const float p = (mnew == -INFINITY) ? 0.f : __expf(s[nt][e] - mnew);
      s[nt][e] = p;
      rs += p;
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
    for (int e = 0; e < 4; ++e) Ps[((lane >> 4) * 4 + e) * AT_LD + nt * 16 + (lane & 15)] = f2bf(s[nt][e]);
  __builtin_amdgcn_s_waitcnt(0xC07F);  // lgkmcnt(0): this wave's P writes land before its reads
  __builtin_amdgcn_wave_barrier();
#pragma unroll
  for (int ks = 0; ks < 2; ++ks) {
    const bf16x8 pa = ld8(Ps + frag + ks * 32);
#pragma unroll
    for (int nt = 0; nt < 4; ++nt)
      o[nt] = mfma16x16x32(pa, ld8(Vt + frag + nt * 16 * AT_LD + ks * 32), o[nt]);
  }
}

// row e of the lane's state, normalised, -> out_row (that row's 64 output columns)
__device__ __forceinline__ void fwd_store_row(bf16_t* out_row, const f32x4 (&o)[4], int e, float l) {
  const int lane = threadIdx.x & 63;
  const float inv = 1.f / l;
#pragma unroll
  for (int nt = 0; nt < 4; ++nt) out_row[nt * 16 + (lane & 15)] = f2bf(o[nt][e] * inv);
}

// ---------------------------------------------------------------- backward
// (a wave owns 16 keys, kw .. kw + 15, and sweeps 64-query tiles)

// this lane's K and V fragments (key lane & 15 of the wave's 16; k_row: the key's 64 K columns,
// its V columns are d elements further)
__device__ __forceinline__ void bwd_load_kv(const bf16_t* k_row, int d, bool valid, bf16x8 (&kf)[2],
                                            bf16x8 (&vf)[2]) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int ks = 0; ks < 2; ++ks) {
    const int c = ks * 32 + 8 * (lane >> 4);
    kf[ks] = valid ? ld8(k_row + c) : (bf16x8){0, 0, 0, 0, 0, 0, 0, 0};
    vf[ks] = valid ? ld8(k_row + d + c) : (bf16x8){0, 0, 0, 0, 0, 0, 0, 0};
  }
}

// threads 0..63: delta[q] = dO[q, h, :] . O[q, h, :] and LSE of the tile's queries q0 .. q0 + 63
// (dout_b / o_b: row 0 of the sequence, row stride d, head h's columns; lse_h: the head's LSE)
__device__ __forceinline__ void bwd_stage_stats(const bf16_t* dout_b, const bf16_t* o_b, const float* lse_h, int d,
                                                int h, int q0, int S, float* lse_s, float* delta_s) {
  if (threadIdx.x < AT_T) {
    const int q = q0 + threadIdx.x;
    float dl = 0.f;
    if (q < S) {
      const long off = (long)q * d + h * AT_D;
#pragma unroll
      for (int c = 0; c < AT_D; c += 8)
        dl = dot8(*reinterpret_cast<const u32x4*>(dout_b + off + c), *reinterpret_cast<const u32x4*>(o_b + off + c),
                  dl);
    }
    lse_s[threadIdx.x] = q < S ? lse_h[q] : 0.f;
    delta_s[threadIdx.x] = dl;
  }
}

// S^T = K Q^T, dP^T = V dO^T (rows: this wave's 16 keys; cols: the tile's 64 queries), then
// P^T = exp(scale S^T - LSE), dS^T = P^T (dP^T - delta) as bf16 -> this wave's [key][q] tiles Pw
// and dSw, and dS -> the shared [q][key] image: dSq_w is its column of this wave's first key,
// dsq_ld its row stride.
__device__ __forceinline__ void bwd_tile_scores(const bf16x8 (&kf)[2], const bf16x8 (&vf)[2], const bf16_t* Qs,
                                                const bf16_t* dOs, const float* lse_s, const float* delta_s,
                                                float scale, int q0, int kw, int S, int causal, bf16_t* Pw,
                                                bf16_t* dSw, bf16_t* dSq_w, int dsq_ld) {
  const int lane = threadIdx.x & 63;
  f32x4 st[4], dpt[4];
#pragma unroll
  for (int nt = 0; nt < 4; ++nt) {
    st[nt] = (f32x4){0.f, 0.f, 0.f, 0.f};
    dpt[nt] = st[nt];
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      const int c = (nt * 16 + (lane & 15)) * AT_LD + ks * 32 + 8 * (lane >> 4);
      st[nt] = mfma16x16x32(kf[ks], ld8(&Qs[c]), st[nt]);
      dpt[nt] = mfma16x16x32(vf[ks], ld8(&dOs[c]), dpt[nt]);
    }
  }
#pragma unroll
  for (int nt = 0; nt < 4; ++nt) {
    const int ql = nt * 16 + (lane & 15), q = q0 + ql;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int kl = (lane >> 4) * 4 + e, key = kw + kl;
      const bool ok = q < S && key < S && !(causal && key > q);
      const float p = ok ? __expf(st[nt][e] * scale - lse_s[ql]) : 0.f;
      const float ds = p * (dpt[nt][e] - delta_s[ql]);
      Pw[kl * AT_LD + ql] = f2bf(p);
      const bf16_t dsb = f2bf(ds);
      dSw[kl * AT_LD + ql] = dsb;
      dSq_w[ql * dsq_ld + kl] = dsb;
    }
  }
}

// dV += P^T dO ; dK += dS^T Q   (K-dim = the tile's 64 queries)
__device__ __forceinline__ void bwd_accum_dkdv(const bf16_t* Pw, const bf16_t* dSw, const bf16_t* dOt,
                                               const bf16_t* Qt, f32x4 (&dk)[4], f32x4 (&dv)[4]) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int ks = 0; ks < 2; ++ks) {
    const int ca = (lane & 15) * AT_LD + ks * 32 + 8 * (lane >> 4);
    const bf16x8 pa = ld8(&Pw[ca]), sa = ld8(&dSw[ca]);
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) {
      const int cb = (nt * 16 + (lane & 15)) * AT_LD + ks * 32 + 8 * (lane >> 4);
      dv[nt] = mfma16x16x32(pa, ld8(&dOt[cb]), dv[nt]);
      dk[nt] = mfma16x16x32(sa, ld8(&Qt[cb]), dk[nt]);
    }
  }
}

// dK, dV -> the K and V column blocks of head h of dQKV (dqkv_b: row 0 of the sequence, row stride
// 3 d); with dbias, their column sums (the k/v bias gradient, over exactly the stored bf16 values)
// go out with one atomic per column per wave
__device__ __forceinline__ void bwd_store_dkdv(const f32x4 (&dk)[4], const f32x4 (&dv)[4], float scale, int kw, int S,
                                               int d, int h, bf16_t* dqkv_b, float* dbias) {
  const int lane = threadIdx.x & 63;
  float sk[4] = {0.f, 0.f, 0.f, 0.f}, sv[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int key = kw + (lane >> 4) * 4 + e;
    if (key >= S) continue;
    bf16_t* row = dqkv_b + (long)key * (3 * d) + h * AT_D + (lane & 15);
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) {
      const bf16_t kb = f2bf(dk[nt][e] * scale), vb = f2bf(dv[nt][e]);
      row[d + nt * 16] = kb;
      row[2 * d + nt * 16] = vb;
      sk[nt] += bf2f(kb);
      sv[nt] += bf2f(vb);
    }
  }
  if (dbias) {
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) {
      sk[nt] += __shfl_xor(sk[nt], 16, 64);
      sk[nt] += __shfl_xor(sk[nt], 32, 64);
      sv[nt] += __shfl_xor(sv[nt], 16, 64);
      sv[nt] += __shfl_xor(sv[nt], 32, 64);
    }
    if (lane < 16) {
#pragma unroll
      for (int nt = 0; nt < 4; ++nt) {
        atomicAdd(dbias + d + h * AT_D + nt * 16 + lane, sk[nt]);
        atomicAdd(dbias + 2 * d + h * AT_D + nt * 16 + lane, sv[nt]);
      }
    }
  }
}

}  // namespace jdt
