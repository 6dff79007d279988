// Prefill copy into an FP8 KV cache: the k / v columns of the training forward's qkv, quantized row by
// row (kv_fp8.h) into one layer's caches in the cache's own layout -- the FP8 counterpart of the two
// permute-copies Generator.prefill does for a bf16 cache.  One launch per layer.
#include "kv_fp8.h"

#include <limits.h>

namespace jdt {

// qkv [B * Sp, 3 * H * 64] bf16 (row b * Sp + i is token i of sequence b; q | k | v), caches
// [B, H, S_max, 64] e4m3 bytes, scales fp32 [B, H, S_max].  Lane octet r = (b, i, h) with i < n owns cache
// row (b, h, i) of K and of V; lane c of it holds columns 8c .. 8c + 7.  Rows >= n are left alone.  An
// octet past the last row runs the quantizer on zeros (every lane must be active in it) and stores nothing.
__global__ void __launch_bounds__(256) kv_quantize_rows_kernel(const bf16_t* __restrict__ qkv,
                                                              uint8_t* __restrict__ kc, uint8_t* __restrict__ vc,
                                                              float* __restrict__ ksc, float* __restrict__ vsc,
                                                              long rows, int H, int S_max, int Sp, int n) {
  const long t = (long)blockIdx.x * 256 + threadIdx.x;
  const long r = t >> 3;
  const int dc = (int)(t & 7) * 8;
  const bool own = r < rows;   // the same in the octet
  const int h = (int)(r % H), i = (int)((r / H) % n), b = (int)(r / ((long)H * n));
  const long d = (long)H * KV_ROW;
  u32x4 kx = {0u, 0u, 0u, 0u}, vx = kx;
  if (own) {
    const bf16_t* src = qkv + ((long)b * Sp + i) * 3 * d + h * KV_ROW + dc;
    kx = *reinterpret_cast<const u32x4*>(src + d);
    vx = *reinterpret_cast<const u32x4*>(src + 2 * d);
  }
  float ksv, vsv;
  const u32x2 kq = kv_quantize8(kx, ksv), vq = kv_quantize8(vx, vsv);
  if (own) {
    const long row = ((long)b * H + h) * S_max + i;
    *reinterpret_cast<u32x2*>(kc + row * KV_ROW + dc) = kq;
    *reinterpret_cast<u32x2*>(vc + row * KV_ROW + dc) = vq;
    if (dc == 0) {
      ksc[row] = ksv;
      vsc[row] = vsv;
    }
  }
}

}  // namespace jdt
using namespace jdt;

// Rows i < n of every (sequence, head) of one layer's K and V caches <- the quantized k / v of qkv's token
// i.  -3: Dh != 64; -5: a shape out of range (0 <= n <= min(Sp, S_max)); -2: a null pointer; -6: qkv off a
// 16-byte, a cache off an 8-byte or a scale tensor off a 4-byte boundary.
JDT_API int jdt_kv_quantize_rows(const void* qkv, void* k_cache, void* v_cache, float* k_scale, float* v_scale, int B,
                                 int H, int Dh, int S_max, int Sp, int n, void* stream) {
  if (Dh != KV_ROW) return -3;
  if (B < 0 || H < 1 || S_max < 1 || Sp < 1 || n < 0 || n > Sp || n > S_max) return -5;
  if (!qkv || !k_cache || !v_cache || !k_scale || !v_scale) return -2;
  if (misaligned16(qkv) || misaligned8(k_cache) || misaligned8(v_cache) || misaligned4(k_scale) ||
      misaligned4(v_scale))
    return -6;
  const long rows = (long)B * n * H;
  if (rows == 0) return 0;
  const long blocks = (rows * 8 + 255) / 256;
  if (blocks > INT_MAX) return -5;
  hipLaunchKernelGGL(kv_quantize_rows_kernel, dim3((unsigned)blocks), dim3(256), 0, static_cast<hipStream_t>(stream),
                     static_cast<const bf16_t*>(qkv), static_cast<uint8_t*>(k_cache), static_cast<uint8_t*>(v_cache),
                     k_scale, v_scale, rows, H, S_max, Sp, n);
  return HIP_LAUNCH_CHECK();
}
