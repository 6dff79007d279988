// The FP8 KV-cache row format, written once for the kernels that quantize (attn_decode.hip,
// attn_append.hip, kv_quantize.hip) -- ops/kernels.py kv_quantize / kv_dequantize is the definition
// they are tested against, byte for byte.
//
// One cache row is the 64 values of one (batch, head, token) of K or of V: 64 OCP e4m3 (fn) bytes and
// one fp32 scale.  amax = max |x|, e = floor(log2(amax)) from amax's exponent bits, clamped to
// [-120, 127] (amax == 0: e = 7); scale = 2^(e - 7), a power of two; q = e4m3(x * 2^(7 - e)), round to
// nearest even.  The product is exact and the row's largest scaled magnitude lies in [128, 256), so
// nothing saturates.  float(q) * scale is exact in fp32 and exactly a bf16, so a consumer of
// dequantized rows rounds nowhere and scaling a dot product or a P.V weight by the row's scale gives
// the bits of scaling the row.
//
// A row is owned by an aligned lane octet, lane c holding columns 8c .. 8c + 7 (16 bytes of bf16 in,
// 8 bytes of e4m3 out); every lane of the octet must be active in kv_quantize8.
#pragma once

#include "common.h"

namespace jdt {

typedef __attribute__((ext_vector_type(2))) unsigned u32x2;
typedef __attribute__((ext_vector_type(2))) float f32x2;

constexpr int KV_ROW = 64;   // values, and bytes, of a quantized cache row

// max over the 8 lanes of an aligned lane octet (all lanes active): the three steps of
// attn_decode.hip's oct_sum_dpp; every lane of the octet gets the same value
__device__ __forceinline__ float oct_max_dpp(float v) {
  v = fmaxf(v, dpp_mov<0xB1>(v));   // quad_perm [1,0,3,2]
  v = fmaxf(v, dpp_mov<0x4E>(v));   // quad_perm [2,3,0,1]
  v = fmaxf(v, dpp_mov<0x141>(v));  // row_half_mirror
  return v;
}

// 8 e4m3 bytes -> 8 floats, unscaled (byte i is element i)
__device__ __forceinline__ void fp8_unpack8(const u32x2& q, float (&x)[8]) {
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const f32x2 lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)q[j], false);
    const f32x2 hi = __builtin_amdgcn_cvt_pk_f32_fp8((int)q[j], true);
    x[4 * j] = lo[0];
    x[4 * j + 1] = lo[1];
    x[4 * j + 2] = hi[0];
    x[4 * j + 3] = hi[1];
  }
}

// this lane's 8 bf16 of a row -> its 8 e4m3 bytes; ``scale``: the row's, the same in the octet's 8 lanes
__device__ __forceinline__ u32x2 kv_quantize8(const u32x4& x, float& scale) {
  float f[8];
  unpack8(x, f);
  float amax = 0.f;
#pragma unroll
  for (int e = 0; e < 8; ++e) amax = fmaxf(amax, fabsf(f[e]));
  amax = oct_max_dpp(amax);
  int e = (int)(__float_as_uint(amax) >> 23) - 127;   // amax >= 0: the sign bit is clear
  e = amax == 0.f ? 7 : min(max(e, -120), 127);
  scale = ldexpf(1.f, e - 7);
  const float inv = __uint_as_float((unsigned)(134 - e) << 23);   // 2^(7 - e), 7 - e in [-120, 127]: normal
  u32x2 q;
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    int w = __builtin_amdgcn_cvt_pk_fp8_f32(f[4 * j] * inv, f[4 * j + 1] * inv, 0, false);
    w = __builtin_amdgcn_cvt_pk_fp8_f32(f[4 * j + 2] * inv, f[4 * j + 3] * inv, w, true);
    q[j] = (unsigned)w;
  }
  return q;
}

// 8 e4m3 bytes and the row's scale -> the 8 bf16 of the dequantized row (exact)
__device__ __forceinline__ u32x4 kv_dequantize8(const u32x2& q, float scale) {
  float f[8];
  fp8_unpack8(q, f);
  u32x4 o;
#pragma unroll
  for (int j = 0; j < 4; ++j)
    o[j] = (unsigned)f2bf(f[2 * j] * scale) | ((unsigned)f2bf(f[2 * j + 1] * scale) << 16);
  return o;
}

}  // namespace jdt

// host: the launchers' checks of the quantized caches (8-byte loads) and their scales
static inline bool misaligned8(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 7) != 0; }
static inline bool misaligned4(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3) != 0; }
