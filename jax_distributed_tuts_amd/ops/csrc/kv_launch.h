// Host side of the KV-cache attention launchers (attn_decode.hip, attn_append.hip): the arguments
// of every variant in one struct and the one ladder of checks their extern "C" entry points share.
// No device code.
#pragma once

#include "kv_fp8.h"

// What an entry point received; a pointer its variant does not take is null.  ``split``: the pair of
// launches through the workspace (decode: the ``_long`` entry points; append: ``_split``).
struct KvAttnArgs {
  const void* qkv;
  void *k_cache, *v_cache;
  float *k_scale, *v_scale;   // fp8
  void* o;
  const int* pos;
  const int* count;           // append with rows
  float* ws;                  // split
  long ws_floats;
  int B, C, H, Dh, S_max;     // C: append only
  float scale;
  bool rows, split, fp8;
};

// the launch of one kernel instantiation (a file's table of them is indexed by the three flags)
using KvAttnLaunch = int (*)(const KvAttnArgs&, hipStream_t);

// The envelope of a family of launchers and the shape of its split workspace.
struct KvAttnLimits {
  int s_top;       // most cache rows per head
  int c_top;       // most new tokens per sequence and call; 0: decode (one token, no C and no count)
  long bh_top;     // most B * H the grid holds
  int ws_tile;     // split: query rows per tile (decode: 1), keys per span and fp32 words of the
  int ws_span;     //   partials of one (batch, head, query tile, span)
  int ws_partial;
};

// Everything is checked before anything is launched, in this order (the codes are the entry points'
// contract): -3 head dim, -4 S_max, -11 C, -5 a batch or head count the grid cannot hold, -2 a null
// pointer the variant needs, -6 alignment (qkv 16 bytes; caches 16, FP8 caches 8 and scales 4),
// -10 a workspace below B * H * query tiles * spans * ws_partial floats.  0: valid (B == 0 included).
static inline int kv_attn_check(const KvAttnArgs& a, const KvAttnLimits& lim) {
  const bool append = lim.c_top > 0;
  if (a.Dh != 64) return -3;
  if (a.S_max < 1 || a.S_max > lim.s_top) return -4;
  if (append && (a.C < 1 || a.C > lim.c_top)) return -11;
  if (a.B < 0 || a.H < 1 || (long)a.B * a.H > lim.bh_top) return -5;
  if (!a.qkv || !a.k_cache || !a.v_cache || !a.o || !a.pos || (append && a.rows && !a.count) ||
      (a.fp8 && (!a.k_scale || !a.v_scale)) || (a.split && !a.ws))
    return -2;
  if (misaligned16(a.qkv)) return -6;
  if (a.fp8 ? misaligned8(a.k_cache) || misaligned8(a.v_cache) || misaligned4(a.k_scale) || misaligned4(a.v_scale)
            : misaligned16(a.k_cache) || misaligned16(a.v_cache))
    return -6;
  if (a.split) {
    const long tiles = append ? (a.C + lim.ws_tile - 1) / lim.ws_tile : 1;
    const long spans = (a.S_max + lim.ws_span - 1) / lim.ws_span;
    if (a.ws_floats < (long)a.B * a.H * tiles * spans * lim.ws_partial) return -10;
  }
  return 0;
}
