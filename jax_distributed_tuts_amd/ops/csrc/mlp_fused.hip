// Whole-step fused kernels for the tutorial classifier (784 -> H -> C, SiLU,
// dropout, softmax-CE, AdamW) -- the reference's DP/FSDP hot loop
// (data_paral.py:171-238, util.py:41-78) in TWO launches per step on 1 GPU.
//
// Measured on MI355X, each dependent kernel of this tiny model costs ~4-6 us
// end to end regardless of its work (profiles/README.md), so the step is
// organised around the two global data dependencies of the maths:
//
// mlp2_fwd  grid (row blocks of 32) x (hidden blocks of 16), 8 waves
//   Z1 = X W1 + b1 (fp32 X converted in-register, W1 column block staged
//   transposed in LDS, K split over the 8 waves, partials reduced in LDS),
//   H = dropout(silu(Z1)) plus the backward factor G1 = silu'(Z1) * mask/keep,
//   and the block's partial logits H[:,blk] W2[blk,:]
//   (+ b2 from block 0) accumulated with fp32 atomics into logits[M][C].
//   (All rows of all minibatches at once: every row carries its minibatch's
//   1/mb loss weight, so the summed gradient equals util.accum_grads_loop's.)
//
// mlp2_bwd  grid (hidden blocks of 16) x (input chunks of KC), 8 waves
//   every workgroup recomputes CE from the summed logits (M x C, tiny) ->
//   dlogits; its dZ1 block = (dlogits W2[blk]^T) * G1 (one MFMA per wave);
//   dW1[chunk, blk] = X[:,chunk]^T dZ1[:,blk] on MFMA with both operands
//   staged K(=row)-contiguous in LDS; chunk-0 blocks also emit db1, dW2[blk]
//   and block (0,0) db2 + metrics.  Each gradient element is produced by
//   exactly ONE workgroup, so
//     mode 0 (DP over N>1 GPUs): plain-store grads into the flat bucket for
//            the RCCL all-reduce, AdamW follows;
//     mode 1 (single GPU): apply AdamW right in the epilogue (no grad buffer
//            round trip, no optimizer launch).  W2's bf16 shadow is double
//            buffered by step parity because other workgroups of the same
//            launch still read the old W2 for dZ1; b2 is only read by mlp2_fwd.
//
// Latency structure (tools/stamp_mlp2.py, s_memrealtime phase stamps): every
// global load of a workgroup -- including the AdamW state of its outputs -- is
// issued before its first LDS write or MFMA; each thread owns whole 4-row
// dropout groups so one Philox call serves 4 elements; 8 waves per workgroup so
// the dependent VALU chains (Philox, exp, f32->bf16) overlap across waves.
#include "common.h"

namespace jdt {

constexpr int NT = 512;  // threads per workgroup (8 waves)
constexpr int NW = NT / 64;

// Input chunk of one backward workgroup (= the X^T columns one forward hidden block
// writes) for an input width K_IN: 112 for the tutorial's 784 (7 chunks), 64 for
// power-of-two widths (1024: 16 chunks).  At most 7 dW1 tiles of 16 rows per chunk
// (wave 7 is the aux wave: dW2 / db1 / db2), a multiple of 16.
template <int K_IN>
constexpr int mlp2_kc() {
  return K_IN % 112 == 0 ? 112 : (K_IN % 64 == 0 ? 64 : (K_IN % 32 == 0 ? 32 : 16));
}

struct Mlp2Args {
  int M, H;
  float inv_mb;                     // CE grad scale: 1 / rows per minibatch
  const float* X; const int* labels;
  const bf16_t* W1s; const bf16_t* b1s; const bf16_t* W2s0; const bf16_t* W2s1; const bf16_t* b2s;
  // G1: the backward factor silu'(Z1) * mask / keep, fp32 [ceil(M/4)][H][4] (the
  // dropout-group layout both kernels use), written by mlp2_fwd so mlp2_bwd needs
  // neither Z1 nor the dropout bits
  float* G1; bf16_t* H1; float* logits;   // logits: [2][M][C] (step parity)
  float keep; unsigned long long seed, offset;
  int* step; unsigned* ticket;
  // mode 0 outputs
  float* gW1; float* gb1; float* gW2; float* gb2; float* mslot;
  // mode 1 (fused AdamW)
  int fuse_opt;
  float* pW1; float* pb1; float* pW2; float* pb2;
  float* mW1; float* mb1; float* mW2; float* mb2;
  float* vW1; float* vb1; float* vW2; float* vb2;
  bf16_t* sW1; bf16_t* sb1; bf16_t* sW2_0; bf16_t* sW2_1; bf16_t* sb2;
  float lr, beta1, beta2, eps, wd, gscale;
  float* running;
  unsigned long long* stamps;   // diagnostic: per-workgroup s_memrealtime (100 MHz) at phase ends (null = off)
  // K-contiguous bf16 operand copies that let both kernels load MFMA fragments
  // straight from global memory (no LDS transposition on the critical path):
  bf16_t* W1T;   // [H][ldw1t] = W1^T, written by mlp2_bwd's AdamW epilogue (mode 1); null -> LDS path
  int ldw1t;     // >= KP (zero-padded K tail)
  bf16_t* XT;    // [K_IN][ldxt] = X^T (rows of all minibatches), written by mlp2_fwd
  int ldxt;      // >= Mp, zero-padded sample tail
  // mlp2_fwd's copy of the step it ran (block (0,0) writes it); mlp2_bwd reads the
  // copy, so its lead block may advance `step` itself without an arrival ticket
  int* step_copy;
  // loop kernel only: fp32 snapshot of W2 [H][C] taken by the forward (row block 0)
  // for the same step's backward, whose chunk-0 workgroups update W2 concurrently
  float* W2snap;
  // mode 0, N > 1: the gradient bucket lives in this rank's xGMI staging buffer
  // (comm/csrc/xgmi.hip, staged all-reduce): grads and metric slots are written at
  // + (step & 1) * stage_stride floats, the half the collective of this step reads
  long stage_stride;
  // deterministic mode (JDT_DETERMINISTIC=1): each column block of mlp2_fwd stores its
  // partial logits to det_logits[H/16][M][C] instead of fp32-atomically adding them;
  // mlp2_bwd sums the partials in column-block order -> bitwise-reproducible steps.  The
  // run-ahead / persistent step (lg3) keeps one such set per step % 3: [3][H/16][M][C]
  float* det_logits;
  // run-ahead step (mlp2_bwd_kernel<..., AHEAD>): the backward launch of step t also runs
  // step t+1's forward, so a step is ONE launch.  XR: row-major bf16 copy of X written by
  // mlp2_fwd; zslab: per-(hidden block, input chunk) partial Z1 = X[:, chunk] W1[chunk, blk]
  // fp32 [H/16][K_IN/KC][MPM/4][16][4]; ztick (32-word = 128-byte lines, no line is
  // shared by two XCDs' L2s): line 0 = step ticket, error word, launch counter; line
  // 1 + blk = column block blk's barrier counter; then one line per XCD with a counter
  // per tile it runs (== the launch counter when every tile ran exactly once per
  // launch); hand: fp32 updated b1 [H], W2 [H][C], b2 [C]
  // handed from the chunk-0 / lead workgroups to each column block's last arriver.
  // lg3: logits accumulators indexed by step % 3 (forward of t+1 accumulates into one
  // buffer while the backward of t reads another and re-arms the third).
  bf16_t* XR; float* zslab; unsigned* ztick; float* hand;
  int lg3;
  // fused optimizer = plain SGD (p -= lr * (g * gscale + wd * p), no momentum) instead
  // of AdamW: the m / v pointers then alias p and are neither used nor written
  int opt_sgd;
  // mode 0, FSDP N > 1: gradients + metric slots go straight into the xGMI staging
  // buffer in the fused FSDP collective's packed layout (common.h StageMap; leaves W1,
  // b1, W2, b2, metrics), half = step parity; null = plain stores at g* (+ goff)
  const StageMap* smap;
  // run-ahead backward only: bit 0 = the W1 AdamW state (p, m, v) and the W1^T copy are
  // stored write-through (sc1), bit 1 = the Z1 partials and G1 / H1 too.  A plain store
  // leaves its line dirty in this XCD's L2 and the kernel boundary writes every dirty
  // line back before the next launch starts (~B / 6 TB/s on the boundary, guide
  // "boundary" row); written through, those bytes drain during the kernel's own
  // latency-bound run-ahead phases instead.
  int wt;
  // N > 1 run-ahead step: the per-tile gradient exchange with the other ranks' launches
  // (common.h TxArgs, device memory; null = one GPU)
  const TxArgs* tx;
  // with tx: 1 = FSDP (the optimizer state pointers are this rank's local shards; the
  // tile's partials go to their rows' owners, which hand back updated values)
  int tx_fsdp;
};

// Persistent multi-step launch (mlp2_loop_kernel): n steps, grid barriers between
// the phases.  ctr counts barrier arrivals across launches (never reset); base is
// its value at the start of the next launch (advanced by block 0 at the end);
// err is raised by a barrier that timed out (every workgroup then leaves).
struct Mlp2Loop {
  int n;
  unsigned* ctr;
  unsigned* base;
  int* err;
  long long timeout;   // s_memrealtime ticks (100 MHz) per barrier
  unsigned long long* stamps;   // diagnostic: [G][n][5] s_memrealtime per phase edge (null = off)
};

// 16 slots per workgroup.  Slots 0-4: s_memrealtime at phase ends; slots 5/6:
// s_memtime (core clock) at phases 0/4, so (slot6 - slot5) / (slot4 - slot0) * 100 MHz
// is the shader clock; slots 8-11: run-ahead phases (mlp2_bwd AHEAD); 12/13: the N > 1
// tile exchange's start / end.
#define STAMP(i)                                                                              \
  do {                                                                                        \
    if (a.stamps && threadIdx.x == 0) {                                                       \
      unsigned long long* s_ = a.stamps + (long)(blockIdx.y * gridDim.x + blockIdx.x) * 16; \
      s_[(i)] = __builtin_amdgcn_s_memrealtime();                                             \
      if ((i) == 0) s_[5] = __builtin_amdgcn_s_memtime();                                     \
      if ((i) == 4) s_[6] = __builtin_amdgcn_s_memtime();                                     \
    }                                                                                         \
  } while (0)

struct AdamK { float b1, b2, eps, wd, lr, gs, rbc1, rbc2; int sgd; };

template <class AT>
__device__ __forceinline__ AdamK adam_consts(AT& a, int step) {
  AdamK k;
  k.b1 = a.beta1; k.b2 = a.beta2; k.eps = a.eps; k.wd = a.wd; k.lr = a.lr; k.gs = a.gscale; k.sgd = a.opt_sgd;
  const float t = (float)(step + 1);
  k.rbc1 = 1.f / (1.f - powf(a.beta1, t));
  k.rbc2 = 1.f / (1.f - powf(a.beta2, t));
  return k;
}

// the same constants with the bias corrections supplied (persistent launch)
template <class AT>
__device__ __forceinline__ AdamK adam_consts_pre(AT& a, float rbc1, float rbc2) {
  AdamK k;
  k.b1 = a.beta1; k.b2 = a.beta2; k.eps = a.eps; k.wd = a.wd; k.lr = a.lr; k.gs = a.gscale; k.sgd = a.opt_sgd;
  k.rbc1 = rbc1;
  k.rbc2 = rbc2;
  return k;
}

// AdamW on one element whose (p, m, v) were loaded earlier; writes them back.
__device__ __forceinline__ float adam_apply(float p, float m, float v, float g, const AdamK& k, float* pp, float* mp,
                                            float* vp) {
  g *= k.gs;
  if (k.sgd) {   // fused SGD (SGD without momentum, utils/train_state.SGD)
    p = p - k.lr * (g + k.wd * p);
    *pp = p;
    return p;
  }
  m = k.b1 * m + (1.f - k.b1) * g;
  v = k.b2 * v + (1.f - k.b2) * g * g;
  // v_rcp_f32 (1 ulp) instead of the IEEE divide's scale/fma/fixup sequence
  p = p - k.lr * ((m * k.rbc1) * __builtin_amdgcn_rcpf(sqrtf(v * k.rbc2) + k.eps) + k.wd * p);
  *pp = p; *mp = m; *vp = v;
  return p;
}
__device__ __forceinline__ float adam_elem(float* p, float* m, float* v, long i, float g, const AdamK& k) {
  return adam_apply(p[i], m[i], v[i], g, k, p + i, m + i, v + i);
}

// ---------------------------------------------------------------------------- in-launch hand-offs
// mlp2_loop_kernel hands data between workgroups inside one launch WITHOUT
// agent-scope release/acquire fences (on this multi-XCD part they write back /
// invalidate a whole XCD L2 per workgroup, ~1.7-6.5 us each): every handed-off
// byte is stored AND loaded with sc1 (global_store/load ... sc1: written through
// to / read from the cross-XCD coherence point, never from a stale L1), 4- or
// 8-byte accesses; a grid barrier orders them (each wave drains its stores with
// s_waitcnt vmcnt(0), workgroup barrier, ONE lane adds to the arrival counter and
// polls it with sc1 loads, workgroup barrier).  SC1 = false: plain accesses (the
// two-launch path, where the kernel boundary orders everything).
typedef __attribute__((address_space(1))) unsigned long long gu64_t;
typedef __attribute__((address_space(1))) float gf32_t;
typedef __attribute__((address_space(1))) unsigned gu32_t;
typedef __attribute__((address_space(1))) int gi32_t;

template <bool SC1> __device__ __forceinline__ float ld_f(const float* p) {
  if constexpr (SC1) return __hip_atomic_load((gf32_t*)p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  else return *p;
}
template <bool SC1> __device__ __forceinline__ void st_f(float* p, float v) {
  if constexpr (SC1) __hip_atomic_store((gf32_t*)p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  else *p = v;
}
template <bool SC1> __device__ __forceinline__ unsigned long long ld_u64(const void* p) {
  if constexpr (SC1) return __hip_atomic_load((gu64_t*)p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  else return *reinterpret_cast<const unsigned long long*>(p);
}
template <bool SC1> __device__ __forceinline__ void st_u64(void* p, unsigned long long v) {
  if constexpr (SC1) __hip_atomic_store((gu64_t*)p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  else *reinterpret_cast<unsigned long long*>(p) = v;
}
// 16 bytes: one dwordx4 (plain) or two sc1 dwordx2
template <bool SC1> __device__ __forceinline__ u32x4 ld_b128(const void* p) {
  if constexpr (SC1) {
    const unsigned long long lo = ld_u64<true>(p), hi = ld_u64<true>(static_cast<const char*>(p) + 8);
    return (u32x4){(unsigned)lo, (unsigned)(lo >> 32), (unsigned)hi, (unsigned)(hi >> 32)};
  } else {
    return *reinterpret_cast<const u32x4*>(p);
  }
}
template <bool SC1> __device__ __forceinline__ void st_b128(void* p, u32x4 v) {
  if constexpr (SC1) {
    st_u64<true>(p, (unsigned long long)v.x | ((unsigned long long)v.y << 32));
    st_u64<true>(static_cast<char*>(p) + 8, (unsigned long long)v.z | ((unsigned long long)v.w << 32));
  } else {
    *reinterpret_cast<u32x4*>(p) = v;
  }
}
// AdamW whose updated parameter is handed to other workgroups (sc1 store of p)
template <bool SC1>
__device__ __forceinline__ float adam_apply_h(float p, float m, float v, float g, const AdamK& k, float* pp, float* mp,
                                              float* vp) {
  float tp, tm = m, tv = v;
  const float r = adam_apply(p, m, v, g, k, &tp, &tm, &tv);
  st_f<SC1>(pp, tp);
  if (!k.sgd) { *mp = tm; *vp = tv; }   // SGD: m / v alias p (unused)
  return r;
}

// Grid barrier of the loop kernel: true when every workgroup has arrived (target
// arrivals counted since the counter's creation), false on timeout / a raised err.
__device__ __forceinline__ bool grid_sync(const Mlp2Loop& l, unsigned target, int* flag_lds) {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // every wave drains its hand-off stores
  __syncthreads();
  if (threadIdx.x == 0) {
    __hip_atomic_fetch_add((gu32_t*)l.ctr, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
    int ok = 1;
    for (unsigned spins = 0;; ++spins) {
      if ((int)(__hip_atomic_load((gu32_t*)l.ctr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) - target) >= 0) break;
      if ((spins & 63) == 63 &&
          (__hip_atomic_load((gi32_t*)l.err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0 ||
           (long long)(__builtin_amdgcn_s_memrealtime() - t0) > l.timeout)) {
        __hip_atomic_store((gi32_t*)l.err, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        ok = 0;
        break;
      }
      __builtin_amdgcn_s_sleep(1);
    }
    flag_lds[0] = ok;
  }
  __syncthreads();
  return flag_lds[0] != 0;
}

// ---------------------------------------------------------------------------- forward
// RB rows per workgroup (16 or 32): 16-row blocks halve each workgroup's X
// bytes and double the grid (256 workgroups at M = 128), which the load-latency
// bound phase 1 prefers.
// DIRECT: the W1^T copy exists (mode 1), B fragments come straight from global;
// otherwise the W1 column block is transposed through LDS.  (A compile-time
// switch: with a runtime branch the two paths' loads share registers and the
// waitcnt pass, which is path-insensitive, drains one path's loads at the join.)
template <int K_IN, int C, int RB, bool DIRECT, bool LOOP, class AT>
__device__ __forceinline__ void mlp2_fwd_body(AT& a, const int bx, const int by, const int step_in) {
  static_assert(!LOOP || DIRECT, "the loop kernel reads W1^T");
  static_assert(RB == 16 || RB == 32, "row block");
  constexpr int KS = (K_IN + 31) / 32;  // 32-deep MFMA k-steps
  constexpr int KP = KS * 32;
  constexpr int WCH = (K_IN * 2 + NT - 1) / NT;  // 16-byte W1 chunks per thread
  constexpr int MAXT = (KS + NW - 1) / NW;       // k-steps per wave
  constexpr int XTC = mlp2_kc<K_IN>();           // X^T features written per hidden block
  constexpr int LDXS = K_IN + 8;                 // padded row of the X image (bf16)
  static_assert(K_IN % XTC == 0 && XTC % 8 == 0 && K_IN % 8 == 0, "X^T chunking");
  // !DIRECT: the W1 column block as loaded, a k-row image [KP][16] (32 bytes per row);
  // B fragments come out of it with the gfx950 transposing ds_read_b64_tr_b16
  __shared__ __attribute__((aligned(16))) bf16_t w1k[DIRECT ? 8 : KP * 16];
  __shared__ __attribute__((aligned(16))) bf16_t xs[RB * LDXS];
  __shared__ float part[NW][RB][17];
  __shared__ float htile[RB][17];
  __shared__ float w2s[16][C];
  __shared__ float b1sh[16];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int M = a.M, H = a.H;
  const int r0 = bx * RB, j0 = by * 16;
  STAMP(0);
  const int ks0 = (w * KS) / NW, ks1 = ((w + 1) * KS) / NW;

  constexpr bool direct = DIRECT;

  // ---- 1. issue all global loads.  Every load is unconditional (clamped address,
  // value selected afterwards) and nothing waits on the step counter: a load under
  // a divergent guard makes the compiler wait for it at the join (asm: this phase
  // was ~8 serial round trips), and the parity-dependent W2 shadow is loaded from
  // both buffers.  The step counter is loaded FIRST through a lane-varying address
  // (an asm-produced zero), so it stays a per-lane value: a uniform load is read
  // back into a scalar register (readfirstlane), which would wait for every load
  // in flight.  The dropout bits, which depend only on it, are then computed while
  // the operand loads are still in flight.
  int step = step_in;
  if constexpr (!LOOP) {
    int lz;
    asm volatile("v_mov_b32 %0, 0" : "=v"(lz));
    step = a.step[lz];
  }
  u32x4 wv[WCH];
  bf16x8 bg[MAXT];
  if constexpr (!DIRECT) {
#pragma unroll
    for (int t = 0; t < WCH; ++t) {
      const int idx = min(tid + t * NT, K_IN * 2 - 1);
      wv[t] = *reinterpret_cast<const u32x4*>(a.W1s + (long)(idx >> 1) * H + j0 + (idx & 1) * 8);
    }
  } else {
#pragma unroll
    for (int t = 0; t < MAXT; ++t) {
      const int ks = min(ks0 + t, ks1 - 1);
      const u32x4 q = ld_b128<LOOP>(a.W1T + (long)(j0 + (lane & 15)) * a.ldw1t + ks * 32 + 8 * (lane >> 4));
      bg[t] = __builtin_bit_cast(bf16x8, q);
    }
  }
  // X row block [RB][K_IN] fp32: fully coalesced float4 loads (consecutive lanes,
  // consecutive 16 B), converted to bf16 into a row-major LDS image the MFMA A
  // fragments are read from (a fragment-shaped global load touches 16 rows/instr).
  constexpr int XF4 = RB * K_IN / 4;                 // float4 per row block
  constexpr int XPT = (XF4 + NT - 1) / NT;           // per thread
  float4 xv[XPT];
#pragma unroll
  for (int e = 0; e < XPT; ++e) {
    const int f = min(tid + e * NT, XF4 - 1), rl = f / (K_IN / 4), k4 = f % (K_IN / 4);
    xv[e] = *reinterpret_cast<const float4*>(a.X + (long)min(r0 + rl, M - 1) * K_IN + 4 * k4);
  }
  const int wi = min(tid, 16 * C - 1);
  const long wo = (long)(j0 + wi / C) * C + wi % C;
  // loop kernel: the fp32 masters (the bf16 shadows are not handed off in-launch)
  bf16_t w2a, w2b, b1b, b2b;
  float w2f = 0.f;
  if constexpr (LOOP) {
    w2f = ld_f<true>(a.pW2 + wo);
    w2a = w2b = f2bf(w2f);
    b1b = f2bf(ld_f<true>(a.pb1 + j0 + (tid & 15)));
    b2b = f2bf(ld_f<true>(a.pb2 + tid % C));
  } else {
    w2a = a.W2s0[wo]; w2b = a.W2s1[wo];
    b1b = a.b1s[j0 + (tid & 15)];
    b2b = a.b2s[tid % C];   // read by the by == 0 logit partials
  }
  __builtin_amdgcn_sched_barrier(0);
  const int par = step & 1;
  const unsigned long long doff = a.offset + ((unsigned long long)(unsigned)step << 32);
  if constexpr (LOOP) {
    if (bx == 0 && tid < 16 * C) st_f<true>(a.W2snap + wo, w2f);   // this step's W2 for the backward
  } else {
    if (a.step_copy && bx == 0 && by == 0 && tid == 0) a.step_copy[0] = step;
  }
  // dropout bits of this thread's 4-row group (phase 4 threads only)
  const int g4 = tid >> 4, gc = tid & 15, rowg = r0 + g4 * 4;
  u32x4 db = {0u, 0u, 0u, 0u};
  if (tid < (RB / 4) * 16 && a.keep < 1.f && rowg < M) db = dropout_bits(a.seed, doff, dropout_group(0, rowg, j0 + gc, M, H));

  // ---- 2. (LDS path) W1 block -> LDS as loaded (k-row image w1k[k][16]), zero the K padding
  if constexpr (!DIRECT) {
#pragma unroll
    for (int t = 0; t < WCH; ++t) {
      const int idx = tid + t * NT;
      if (idx < K_IN * 2) *reinterpret_cast<u32x4*>(&w1k[(idx >> 1) * 16 + (idx & 1) * 8]) = wv[t];
    }
    for (int idx = tid; idx < 2 * (KP - K_IN); idx += NT)
      *reinterpret_cast<u32x4*>(&w1k[(K_IN + (idx >> 1)) * 16 + (idx & 1) * 8]) = (u32x4){0u, 0u, 0u, 0u};
  }
  if (tid < 16 * C) w2s[tid / C][tid % C] = bf2f(par ? w2b : w2a);
  if (tid < 16) b1sh[tid] = bf2f(b1b);
#pragma unroll
  for (int e = 0; e < XPT; ++e) {
    const int f = tid + e * NT, rl = f / (K_IN / 4), k4 = f % (K_IN / 4);
    if (f < XF4) {
      const bool ok = r0 + rl < M;   // rows past M stay zero (X^T tail is read by mlp2_bwd)
      *reinterpret_cast<uint2*>(&xs[rl * LDXS + 4 * k4]) =
          ok ? make_uint2((unsigned)f2bf(xv[e].x) | ((unsigned)f2bf(xv[e].y) << 16),
                          (unsigned)f2bf(xv[e].z) | ((unsigned)f2bf(xv[e].w) << 16))
             : make_uint2(0u, 0u);
    }
  }
  __syncthreads();
  STAMP(1);
  // X^T side output for mlp2_bwd: hidden block y < K_IN/XTC writes input features
  // [y*XTC, (y+1)*XTC) of this row block (16-byte stores of 8 consecutive samples)
  if (a.XT && by < K_IN / XTC && tid < XTC * (RB / 8)) {
    const int i = tid / (RB / 8), h = (tid % (RB / 8)) * 8, xk = by * XTC + i;
    unsigned q[4];
#pragma unroll
    for (int e = 0; e < 4; ++e)
      q[e] = (unsigned)xs[(h + 2 * e) * LDXS + xk] | ((unsigned)xs[(h + 2 * e + 1) * LDXS + xk] << 16);
    u32x4 o; o.x = q[0]; o.y = q[1]; o.z = q[2]; o.w = q[3];
    st_b128<LOOP>(a.XT + (long)xk * a.ldxt + r0 + h, o);
  }
  // row-major bf16 X side output (run-ahead backward: the next step's forward operand)
  if constexpr (!LOOP) {
    if (a.XR && by < K_IN / XTC && tid < RB * (XTC / 8)) {
      const int rl = tid / (XTC / 8), q = tid % (XTC / 8);
      if (r0 + rl < M)
        *reinterpret_cast<u32x4*>(a.XR + (long)(r0 + rl) * K_IN + by * XTC + 8 * q) =
            *reinterpret_cast<const u32x4*>(&xs[rl * LDXS + by * XTC + 8 * q]);
    }
  }

  // ---- 3. K split over the 8 waves
  constexpr int MT = RB / 16;
  f32x4 acc[MT];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) acc[mt] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int t = 0; t < MAXT; ++t) {
    if (ks0 + t < ks1) {
      const int k = (ks0 + t) * 32 + 8 * (lane >> 4);
      bf16x8 b;
      if constexpr (DIRECT) {
        b = bg[t];
      } else {
        // lane 4q+p of each 16-lane group addresses k-row k + q (then + 4 + q),
        // columns 4p..4p+3; after the transposing read it holds column (lane & 15)
        typedef __attribute__((ext_vector_type(4))) short s4;
        const int i16 = lane & 15;
        const unsigned a0 = (unsigned)(uintptr_t)(
            (__attribute__((address_space(3))) const bf16_t*)(w1k + (k + (i16 >> 2)) * 16 + 4 * (i16 & 3)));
        s4 lo, hi;
        asm volatile("ds_read_b64_tr_b16 %0, %1" : "=v"(lo) : "v"(a0));
        asm volatile("ds_read_b64_tr_b16 %0, %1 offset:128" : "=v"(hi) : "v"(a0));
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        b[0] = lo[0]; b[1] = lo[1]; b[2] = lo[2]; b[3] = lo[3];
        b[4] = hi[0]; b[5] = hi[1]; b[6] = hi[2]; b[7] = hi[3];
      }
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) {
        // K tail: W1^T / w1t are zero past K_IN, the X image row is clamped in bounds
        const bf16x8 af = *reinterpret_cast<const bf16x8*>(&xs[(mt * 16 + (lane & 15)) * LDXS + min(k, K_IN - 8)]);
        acc[mt] = mfma16x16x32(af, b, acc[mt]);
      }
    }
  }
#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
#pragma unroll
    for (int e = 0; e < 4; ++e) part[w][mt * 16 + (lane >> 4) * 4 + e][lane & 15] = acc[mt][e];
  __syncthreads();
  STAMP(2);

  // ---- 4. bias + silu + dropout per 4-row group; H tile kept in LDS
  if (tid < (RB / 4) * 16) {
    const int c = gc, col = j0 + c;
    float gf[4];
    unsigned long long hpk = 0ull;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int rl = g4 * 4 + e, row = r0 + rl;
      float hv = 0.f;
      gf[e] = 0.f;
      if (row < M) {
        float v = b1sh[c];
#pragma unroll
        for (int q = 0; q < NW; ++q) v += part[q][rl][c];
        const float z = bf2f(f2bf(v));           // Z1 as the bf16 Dense output
        const float ez = __expf(-z);
        hv = z / (1.0f + ez);                    // act_fwd(ACT_SILU)
        const float sg = 1.0f / (1.0f + ez);
        float gd = sg * (1.0f + z * (1.0f - sg));  // act_grad(ACT_SILU)
        if (a.keep < 1.f) {
          const bool kp = keep_word(db, e, a.keep);
          hv = kp ? hv / a.keep : 0.f;
          gd = kp ? gd / a.keep : 0.f;
        }
        gf[e] = gd;
        const bf16_t hb = f2bf(hv);
        hpk |= (unsigned long long)hb << (16 * e);
        hv = bf2f(hb);
      }
      htile[rl][c] = hv;
    }
    // G1 and H1 in the dropout-group layout [row group][H][4]: one 16-/8-byte store each
    const long go = ((long)(rowg >> 2) * H + col) * 4;
    st_b128<LOOP>(a.G1 + go, (u32x4){__float_as_uint(gf[0]), __float_as_uint(gf[1]), __float_as_uint(gf[2]),
                                     __float_as_uint(gf[3])});
    st_u64<LOOP>(a.H1 + go, hpk);
  }
  __syncthreads();
  STAMP(3);
  float* lg = a.logits + (long)(a.lg3 ? step % 3 : par) * M * C;
  if (tid < RB * C) {
    const int rl = tid / C, c = tid % C, row = r0 + rl;
    if (row < M) {
      float s = (by == 0) ? bf2f(b2b) : 0.f;
#pragma unroll
      for (int n = 0; n < 16; ++n) s += htile[rl][n] * w2s[n][c];
      if (a.det_logits) {
        // run-ahead (lg3): one [H/16][M][C] partial set per step % 3, like the accumulators
        a.det_logits[(((long)(a.lg3 ? step % 3 : 0) * (H / 16) + by) * M + row) * C + c] = s;
      } else if constexpr (LOOP) {
        // read after a grid barrier in this launch: a returning add proves it was performed
        const float old = __hip_atomic_fetch_add((gf32_t*)(lg + (long)row * C + c), s, __ATOMIC_RELAXED,
                                                 __HIP_MEMORY_SCOPE_AGENT);
        asm volatile("" ::"v"(old));
      } else {
        atomicAdd(lg + (long)row * C + c, s);
      }
    }
  }
  __syncthreads();
  STAMP(4);
}

// ---------------------------------------------------------------------------- backward
// Start-up self-test of the tile exchange (comm/tile_exchange.py): workgroup T < tiles
// exchanges, with the payload positions of mlp2_bwd AHEAD's waves (tile T % 7 == 0 with
// the spare wave's dW2 / db1 slots, tile 0 with db2 and the metric slots), values that
// are an exact function of (rank, tile, position), and counts every result that is not
// bit-identical to the rank-ordered sum.  Small grid: the W ranks' grids fit one GPU.
__device__ __forceinline__ float tx_probe_value(int rank, int T, int pos) {
  unsigned h = (unsigned)rank * 0x9E3779B1u ^ (unsigned)T * 0x85EBCA77u ^ (unsigned)pos * 0xC2B2AE3Du;
  h ^= h >> 15; h *= 0x2C1B3C6Du; h ^= h >> 12;
  return (float)((int)(h & 0xFFFFu) - 32768) * (1.f / 4096.f);   // exact in fp32, exact sums
}

__global__ void __launch_bounds__(NT) tx_selftest_kernel(const TxArgs* X, unsigned epoch, unsigned* bad,
                                                        unsigned* err) {
  constexpr int NTILE = 7;
  const int T = blockIdx.x, tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
  const bool chunk0 = T % 7 == 0, lead = T == 0;
  float4 v4[2];
  int p4[2] = {0, 0}, n4 = 0, ps = -1;
  float vs = 0.f;
  if (w < NTILE) {
    p4[0] = w * 256 + lane * 4;
    n4 = 1;
    if (lead && tid < 4) ps = (NTILE + 2) * 256 + 64 + tid;
  } else if (chunk0) {
    p4[0] = NTILE * 256 + lane * 4;
    p4[1] = (NTILE + 1) * 256 + lane * 4;
    n4 = 2;
    if (lead && lane < 10) ps = (NTILE + 2) * 256 + lane;
  }
  const int R = X->rank, W = X->world;
#pragma unroll
  for (int k = 0; k < 2; ++k)
    v4[k] = make_float4(tx_probe_value(R, T, p4[k]), tx_probe_value(R, T, p4[k] + 1),
                        tx_probe_value(R, T, p4[k] + 2), tx_probe_value(R, T, p4[k] + 3));
  if (ps >= 0) vs = tx_probe_value(R, T, ps);
  tx_tile(X, T, epoch, n4, v4, p4, vs, ps, err);
  unsigned nbad = 0;
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    if (k >= n4) continue;
    const float* got = &v4[k].x;
    for (int e = 0; e < 4; ++e) {
      float want = 0.f;
      for (int q = 0; q < W; ++q) want = q == 0 ? tx_probe_value(q, T, p4[k] + e) : want + tx_probe_value(q, T, p4[k] + e);
      nbad += __float_as_uint(got[e]) != __float_as_uint(want);
    }
  }
  if (ps >= 0) {
    float want = 0.f;
    for (int q = 0; q < W; ++q) want = q == 0 ? tx_probe_value(q, T, ps) : want + tx_probe_value(q, T, ps);
    nbad += __float_as_uint(vs) != __float_as_uint(want);
  }
  if (nbad) atomicAdd(bad, nbad);
}

// Persistent run-ahead (PST, mlp2_pst_kernel): what a workgroup's lanes carry from step
// to step in registers -- the AdamW state (p, m, v) of the lane's four W1 elements (aux
// lanes: W2 / b1; block (0,0)'s first lanes: b2 too).  Only the last step of a launch
// stores it; every step still hands its updated values to the other workgroups.
struct PstRegs {
  float op[4], om[4], ov[4];
  float qp, qm, qv;
  float rbc1, rbc2;   // the step's AdamW bias corrections (computed during the previous barrier)
  float l_loss, l_corr;   // block (0,0): this thread's row loss / hit, folded into the metrics
};
// What a persistent launch reads once (pst_x_load) instead of every step: the batch does not
// change inside a launch (the forward wrote X^T and the row-major copy before it), so the
// lane's dW1 A fragments (xf), its next-forward A fragments (xa) and the label of its CE row
// (row tid >> 2: four lanes per row) stay in registers.  Loaded by EVERY launch: a replay may
// find a new batch in the same buffers.
struct PstX {
  bf16x8 xf[4], xa[4];
  int lab;
};
// position of a step inside a persistent launch: step `it` of `n`, the launch counter
// (Mlp2Args::ztick[2]) when the launch started
struct PstPos {
  int it, n;
  unsigned launch0;
  // column-block completion counters (mlp2_pst_kernel CBW): after its forward epilogue
  // every workgroup adds 1 to done[32 * column block]; null = the grid barrier form
  unsigned* done = nullptr;
};
// mlp2_bwd_body's batch operands (one step's phase 0, or once per persistent launch):
// k-step ks of the A fragments of this wave's dW1 tile straight from X^T (written by
// mlp2_fwd, zero-padded to Mp rows) ...
template <int KC, bool SC1, class AT>
__device__ __forceinline__ bf16x8 mlp2_xf_frag(AT& a, const int kc0, const int ks) {
  const int lane = threadIdx.x & 63, wt_ = min((int)threadIdx.x >> 6, KC / 16 - 1), Mp = (a.M + 31) & ~31;
  return __builtin_bit_cast(bf16x8, ld_b128<SC1>(a.XT + (long)(kc0 + wt_ * 16 + (lane & 15)) * a.ldxt +
                                                 min(ks, Mp / 32 - 1) * 32 + 8 * (lane >> 4)));
}
// ... and of the A fragments of X[16w.., chunk] (row-major bf16 copy) for the next forward;
// k past the chunk is multiplied by w1n's zero padding, so the address is only clamped
template <int K_IN, class AT>
__device__ __forceinline__ bf16x8 mlp2_xa_frag(AT& a, const int kc0, const int ks) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  return __builtin_bit_cast(bf16x8, *reinterpret_cast<const u32x4*>(
             a.XR + (long)min(w * 16 + (lane & 15), a.M - 1) * K_IN + min(kc0 + ks * 32 + 8 * (lane >> 4), K_IN - 8)));
}
// lane j (a constant after unrolling) of this lane's quad, every lane active
__device__ __forceinline__ float quad_lane(float v, int j) {
  return j == 0 ? dpp_mov<0x00>(v) : j == 1 ? dpp_mov<0x55>(v) : j == 2 ? dpp_mov<0xAA>(v) : dpp_mov<0xFF>(v);
}

// AHEAD (single GPU, fused AdamW, W1^T copy): after its AdamW epilogue every
// workgroup (blk, chunk) also computes the partial Z1 = X[:, chunk] W1'[chunk, blk]
// of the NEXT step from the W1' tile it just produced (phase 5); the last of a
// column block's K_IN/KC workgroups to arrive sums the partials in chunk order and
// runs the forward epilogue (bias, SiLU, dropout of step t+1, G1/H1, partial logits).
// So one launch per step: the kernel boundary the forward needed (W1' complete) is
// replaced by a per-column-block arrival ticket among workgroups that share an XCD
// (xcd_contiguous_tile), and the one global dependency left -- complete logits for
// the next CE -- is the launch boundary.
//
// PST (persistent run-ahead, mlp2_pst_kernel): the same step, n of them per launch with an
// XCD-hierarchical grid barrier between steps in place of the launch boundary.  The AdamW
// state stays in registers (PstRegs); every byte another workgroup wrote during the launch
// is read with sc1 loads (never served by a stale L1; logits, re-armed write-through and
// accumulated by atomics, come from the cross-XCD coherence point).
template <int K_IN, int C, int KC, bool LOOP, bool AHEAD = false, bool TX = false, bool P3S = false,
          bool FX = false, bool PST = false, bool HX = false, class AT>
__device__ __forceinline__ void mlp2_bwd_body(AT& a, const int bx, const int by, const int step_in,
                                              PstRegs* R = nullptr, const PstPos pp = PstPos{0, 1, 0u},
                                              const PstX* PX = nullptr) {
  static_assert(!PST || (AHEAD && !P3S && !LOOP), "persistent: the run-ahead step (one GPU, or TX / FX exchange)");
  static_assert(PST || !HX, "HX: a persistent launch's batch fragments held in registers (PstX)");
  constexpr bool SCX = LOOP || PST;        // in-launch hand-offs: sc1 loads / stores
  // phase stamps: a persistent launch records step n-2 (a steady step: the last one also
  // stores the optimizer state)
  unsigned long long* const stamps_ = (!PST || pp.it + 2 == pp.n) ? a.stamps : nullptr;
#pragma push_macro("STAMP")
#undef STAMP
#define STAMP(i)                                                                              \
  do {                                                                                        \
    if (stamps_ && threadIdx.x == 0) {                                                        \
      unsigned long long* s_ = stamps_ + (long)(blockIdx.y * gridDim.x + blockIdx.x) * 16;    \
      s_[(i)] = __builtin_amdgcn_s_memrealtime();                                             \
      if (!PST && (i) == 0) s_[5] = __builtin_amdgcn_s_memtime();                             \
      if (!PST && (i) == 4) s_[6] = __builtin_amdgcn_s_memtime();                             \
    }                                                                                         \
  } while (0)
  // persistent launches: sub-phase stamps of one lane (slot k), after `dep` is computed
#define PSTAMP(k, dep)                                                                        \
  do {                                                                                        \
    if (PST && stamps_ && lane == 0) {                                                        \
      const unsigned d_ = __builtin_amdgcn_readfirstlane(__float_as_uint(dep));              \
      stamps_[(long)(blockIdx.y * gridDim.x + blockIdx.x) * 16 + (k)] =                       \
          __builtin_amdgcn_s_memrealtime() + (d_ == 0x7fc00001u ? 1ull : 0ull);               \
    }                                                                                         \
  } while (0)
  constexpr int MPM = 128;                 // max rows per device (fused path)
  constexpr int LDM = MPM + 8;             // padded row (bf16 elements)
  constexpr int NTILE = KC / 16;           // dW1 output tiles (one per wave)
  static_assert(KC % 4 == 0 && K_IN % KC == 0 && NTILE < NW, "tile plan (every dW1 row in range)");
  static_assert((MPM / 4) * 16 == NT, "one 4-row dropout group per thread");
  constexpr int LDB = 40;                  // [row][32 classes] bf16 rows (classes zero-padded), +8 spread
  static_assert(C < 16 && MPM == NW * 16, "dZ1: one 16-row MFMA tile per wave, classes padded to K = 32");
  __shared__ __attribute__((aligned(16))) bf16_t dlB[MPM * LDB];   // dlogits, row-major
  __shared__ __attribute__((aligned(16))) bf16_t w2B[16 * LDB];    // W2[blk, :] (B operand: col = hidden unit)
  __shared__ __attribute__((aligned(16))) bf16_t dzT[16 * LDM];
  __shared__ __attribute__((aligned(16))) bf16_t h1T[16 * LDM];    // H1[:, blk]^T   (chunk-0 blocks)
  __shared__ __attribute__((aligned(16))) bf16_t dlT[16 * LDM];    // dlogits^T, classes padded to 16
  __shared__ float red[2][NW];
  __shared__ float cel[2][PST ? MPM : 1];   // persistent lead: row loss / hit, from the CE's lanes to thread = row
  static_assert(!AHEAD || (!LOOP && KC <= 128 && KC % 16 == 0), "run-ahead: K chunk within 4 k-steps");
  constexpr int LDW1 = 128 + 8;            // w1n row: one hidden unit's KC inputs, zero-padded to 128
  constexpr int NCH = K_IN / KC;           // workgroups per column block
  __shared__ __attribute__((aligned(16))) bf16_t w1n[AHEAD ? 16 * LDW1 : 8];   // W1'[chunk, blk]^T
  __shared__ float htA[AHEAD ? MPM : 1][17];                                   // next H tile
  __shared__ float w2A[AHEAD ? 16 : 1][C];
  __shared__ float b2A[C];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int M = a.M, H = a.H, Mp = (M + 31) & ~31;
  const int j0 = bx * 16, kc0 = by * KC;
  const bool chunk0 = by == 0;
  STAMP(0);
  const bool lead = bx == 0 && by == 0;
  const int rg = tid >> 4, gn = tid & 15;   // this thread's dropout group: rows 4rg..4rg+3, column j0+gn

  // ---- 0. issue all global loads (incl. the AdamW state of this wave's outputs).
  // Every load is unconditional -- clamped address, value selected afterwards -- and
  // none waits on the step counter (both logits / W2-shadow parities are loaded):
  // a load under a divergent guard makes the compiler wait for it at the join,
  // which serialised this phase into ~6 round trips (asm).  The step counter is
  // loaded last (its scalar read-back waits for every earlier load).  Run-ahead: it is
  // loaded FIRST through a lane-varying address instead (a per-lane value, as in the
  // forward), so step t+1's dropout bits are computed while the other loads fly.
  int step_lane = 0;
  if constexpr (AHEAD && !PST) {
    int lz;
    asm volatile("v_mov_b32 %0, 0" : "=v"(lz));
    step_lane = a.step[lz];
  }
  float lr0[C], lr1[C], lr2[AHEAD ? C : 1];
  // persistent: the CE runs on the whole workgroup, four lanes per row -- lane cq of row
  // crow loads, rounds and exponentiates the classes cq + 4k only (CK of them at most)
  constexpr int CK = (C + 3) / 4;
  const int crow = tid >> 2, cq = tid & 3;
  float lown[CK];
  if constexpr (PST) {
    const long lo = (long)min(crow, M - 1) * C;
    if (a.det_logits) {
      // deterministic: this step's per-column-block partial logits (written through by the
      // previous forward epilogues) summed in column-block order, per class as the one-step kernel
      const float* pb = a.det_logits + (long)(step_in % 3) * (H / 16) * M * C + lo;
#pragma unroll
      for (int k = 0; k < CK; ++k) lown[k] = 0.f;
      for (int q = 0; q < H / 16; ++q) {
#pragma unroll
        for (int k = 0; k < CK; ++k) lown[k] += ld_f<true>(pb + (long)q * M * C + min(cq + 4 * k, C - 1));
      }
    } else {
      // accumulated by other XCDs' atomics during the previous step: sc1 loads of this
      // step's buffer only (the step is known: no load waits on the counter)
      const float* lg = a.logits + (long)(step_in % 3) * M * C + lo;
#pragma unroll
      for (int k = 0; k < CK; ++k) lown[k] = ld_f<true>(lg + min(cq + 4 * k, C - 1));
    }
  } else {
    const long lo = (long)min(tid, M - 1) * C;
    if (AHEAD && a.det_logits) {
      // deterministic run-ahead: this step's per-column-block partial logits (step % 3 set,
      // written by the previous forward epilogues) summed in column-block order; waits for
      // the step (det mode only)
      const int p3 = step_lane % 3;
      const float* pb = a.det_logits + (long)p3 * (H / 16) * M * C + lo;
#pragma unroll
      for (int c = 0; c < C; ++c) lr0[c] = 0.f;
      for (int q = 0; q < H / 16; ++q) {
#pragma unroll
        for (int c = 0; c < C; ++c) lr0[c] += pb[(long)q * M * C + c];
      }
#pragma unroll
      for (int c = 0; c < C; ++c) {
        lr1[c] = lr0[c];
        if constexpr (AHEAD) lr2[c] = lr0[c];
      }
    } else if constexpr (AHEAD) {   // step % 3 buffers, all three loaded (no wait on the step)
#pragma unroll
      for (int c = 0; c < C; ++c) {
        lr0[c] = a.logits[lo + c]; lr1[c] = a.logits[(long)M * C + lo + c]; lr2[c] = a.logits[2l * M * C + lo + c];
      }
    } else if constexpr (LOOP) {   // step known: this step's parity only
      const float* lg = a.logits + (long)(step_in & 1) * M * C;
#pragma unroll
      for (int c = 0; c < C; ++c) lr1[c] = lr0[c] = ld_f<true>(lg + lo + c);
    } else if (a.det_logits) {
      // partial logits of the H/16 column blocks, summed in block order (deterministic)
#pragma unroll
      for (int c = 0; c < C; ++c) lr0[c] = 0.f;
      for (int q = 0; q < a.H / 16; ++q) {
        const float* pq = a.det_logits + (long)q * M * C + lo;
#pragma unroll
        for (int c = 0; c < C; ++c) lr0[c] += pq[c];
      }
#pragma unroll
      for (int c = 0; c < C; ++c) lr1[c] = lr0[c];
    } else {
#pragma unroll
      for (int c = 0; c < C; ++c) { lr0[c] = a.logits[lo + c]; lr1[c] = a.logits[(long)M * C + lo + c]; }
    }
  }
  int lab;
  if constexpr (PST) lab = PX->lab;   // of row crow
  else lab = a.labels[min(tid, M - 1)];
  // G1 / H1: this thread's dropout group (rows 4rg..4rg+3, column j0+gn)
  const long go = ((long)min(rg, (M - 1) >> 2) * H + j0 + gn) * 4;
  const u32x4 g1q = ld_b128<SCX>(a.G1 + go);
  const unsigned long long hq = ld_u64<SCX>(a.H1 + go);
  bf16_t hv[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) hv[e] = (bf16_t)(hq >> (16 * e));
  // A fragments of this wave's dW1 tile straight from X^T (written by mlp2_fwd, zero-padded to Mp)
  const int wt_ = min(w, NTILE - 1);
  bf16x8 xf[MPM / 32];
#pragma unroll
  for (int ks = 0; ks < MPM / 32; ++ks) {
    if constexpr (HX) xf[ks] = PX->xf[ks];   // the launch's batch: loaded once (pst_x_load)
    else xf[ks] = mlp2_xf_frag<KC, LOOP>(a, kc0, ks);
  }
  const long wo = (long)(j0 + (tid >> 5)) * C + min(tid & 31, C - 1);   // w2B[tid >> 5][tid & 31]
  bf16_t w2a, w2b;
  if constexpr (LOOP) {
    w2a = w2b = f2bf(ld_f<true>(a.W2snap + wo));   // the forward's snapshot of this step's W2
  } else if constexpr (PST) {
    // written by the column block's chunk-0 workgroup during the previous step: the
    // aligned 4-byte word holding the element, sc1
    const unsigned sh = 16u * (unsigned)(wo & 1);
    w2a = (bf16_t)(__hip_atomic_load((const gu32_t*)(a.W2s0 + (wo & ~1l)), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >> sh);
    w2b = (bf16_t)(__hip_atomic_load((const gu32_t*)(a.W2s1 + (wo & ~1l)), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >> sh);
  } else {
    w2a = a.W2s0[wo]; w2b = a.W2s1[wo];
  }
  const int trow0 = kc0 + wt_ * 16 + (lane >> 4) * 4;   // this lane's 4 dW1 rows (tile = wave)
  const int tcol = j0 + (lane & 15);
  // wave NW-1 owns no dW1 tile; in chunk-0 blocks it reduces dW2 / db1 (/ db2) on MFMA,
  // so it prefetches the AdamW state of those outputs instead.  (Mode 0 has no
  // optimizer state: the loads then read the gradient buffers, values unused.)
  const bool aux = chunk0 && w == NW - 1;
  const int ac = lane & 15;                        // aux: class column
  const bool fo = a.fuse_opt != 0;
  // aux lanes: class column ac < C -> W2[j0+n][ac]; ac >= C -> b1[j0+n] (lane C applies it)
  const bool w2l = aux && ac < C;
  const float* sp = aux ? (w2l ? sgpr_ptr(fo ? a.pW2 : a.gW2) : sgpr_ptr(fo ? a.pb1 : a.gb1)) : sgpr_ptr(fo ? a.pW1 : a.gW1);
  const float* sm = aux ? (w2l ? sgpr_ptr(fo ? a.mW2 : a.gW2) : sgpr_ptr(fo ? a.mb1 : a.gb1)) : sgpr_ptr(fo ? a.mW1 : a.gW1);
  const float* sv = aux ? (w2l ? sgpr_ptr(fo ? a.vW2 : a.gW2) : sgpr_ptr(fo ? a.vb1 : a.gb1)) : sgpr_ptr(fo ? a.vW1 : a.gW1);
  // FSDP one-launch (FX): the AdamW state is this rank's LOCAL shard (W1 rows in K_IN / W
  // blocks, W2 / b1 rows in H / W blocks); other ranks' elements read a clamped index
  int fx_R = 0, fx_rpq = 1, fx_hpq = 1;
  if constexpr (FX) {
    fx_R = __builtin_amdgcn_readfirstlane(a.tx->rank);   // scalar (common.h tx_tile)
    const int fx_W = __builtin_amdgcn_readfirstlane(a.tx->world);
    fx_rpq = K_IN / fx_W;
    fx_hpq = H / fx_W;
  }
  float op[4], om[4], ov[4];
  if constexpr (PST) {   // loaded by the launch's prologue (pst_state_io), carried in registers
#pragma unroll
    for (int e = 0; e < 4; ++e) { op[e] = R->op[e]; om[e] = R->om[e]; ov[e] = R->ov[e]; }
  } else {
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int n = (lane >> 4) * 4 + e;
    long idx = aux ? (w2l ? (long)(j0 + n) * C + ac : (long)(j0 + n)) : (long)(trow0 + e) * H + tcol;
    if constexpr (FX) {
      const int lr = aux ? min(max(j0 + n - fx_R * fx_hpq, 0), fx_hpq - 1)
                         : min(max(trow0 + e - fx_R * fx_rpq, 0), fx_rpq - 1);
      idx = aux ? (w2l ? (long)lr * C + ac : (long)lr) : (long)lr * H + tcol;
    }
    op[e] = ld_global(sp + idx); om[e] = ld_global(sm + idx); ov[e] = ld_global(sv + idx);
  }
  }
  // lead: metric accumulators (persistent N > 1: its own store of the previous step, sc1 so
  // no stale L1 line is read)
  float run_pre;
  if constexpr (PST && TX) run_pre = ld_f<true>(a.running + (lane & 3));
  else run_pre = (a.running ? a.running : a.logits)[lane & 3];
  const int lq = min(lane, C - 1);
  float qp, qm, qv;
  if constexpr (PST) {
    qp = R->qp; qm = R->qm; qv = R->qv;
  } else {
    qp = (fo ? a.pb2 : a.gb2)[lq]; qm = (fo ? a.mb2 : a.gb2)[lq]; qv = (fo ? a.vb2 : a.gb2)[lq];
  }
  // run-ahead: A fragments of X[16w.., chunk] (row-major bf16 copy) for the next
  // forward (in flight through CE, dZ1 and dW1); k past the chunk is multiplied by
  // w1n's zero padding, so the address is only clamped.  dbn: step t+1's dropout bits
  // of this thread's element of the epilogue share (phase 6: workgroup `by` of the
  // column block finishes row groups [g_lo, g_hi)), computed in phase 5.
  bf16x8 xa[AHEAD ? 4 : 1];
  u32x4 dbn = {0u, 0u, 0u, 0u};
  const int g_lo = (by * (MPM / 4)) / NCH, g_hi = ((by + 1) * (MPM / 4)) / NCH;
  // phase 6: this thread's element -- row group eg, row eg*4 + ee, column j0 + gn
  // (tid < 64 * (g_hi - g_lo): one element per thread spreads the epilogue over 5 waves)
  const int eg = g_lo + (tid >> 6), ee = (tid >> 4) & 3;
  if constexpr (AHEAD) {
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      if constexpr (HX) xa[ks] = PX->xa[ks];
      else xa[ks] = mlp2_xa_frag<K_IN>(a, kc0, ks);
    }
  }
  __builtin_amdgcn_sched_barrier(0);
  int step = step_in;
  if constexpr (PST) step = step_in;    // the launch's first step + it
  else if constexpr (AHEAD) step = step_lane;   // advanced by the step ticket once every workgroup has read it
  else if constexpr (!LOOP) step = (a.step_copy ? a.step_copy : a.step)[0];
  const int par = step & 1;
  float lrow[C];
  if constexpr (PST) {
    // the row's rounded logits gathered from its four lanes (every lane active)
#pragma unroll
    for (int k = 0; k < CK; ++k) lown[k] = round_bf(lown[k]);
#pragma unroll
    for (int c = 0; c < C; ++c) lrow[c] = quad_lane(lown[c >> 2], c & 3);
  } else if constexpr (AHEAD) {
    const int p3 = step % 3;
#pragma unroll
    for (int c = 0; c < C; ++c) lrow[c] = p3 == 0 ? lr0[c] : (p3 == 1 ? lr1[c] : lr2[c]);
  } else {
#pragma unroll
    for (int c = 0; c < C; ++c) lrow[c] = par ? lr1[c] : lr0[c];
  }

  // persistent: the bias corrections (two powf + two divides per lane, ~0.4 us of VALU at
  // two waves per SIMD on the step's critical path) were computed while this workgroup
  // waited in the previous grid barrier
  AdamK ak;
  if constexpr (PST) {
    ak = adam_consts_pre(a, R->rbc1, R->rbc2);
  } else {
    // (pinning these early, as md_bwd does, measured no gain here: 77.7-77.9k per-step
    // headline, N = 2 shared 44.5k vs 46.8k; the compiler's placement stays)
    ak = adam_consts(a, step);
  }
  const long goff = (!fo && a.stage_stride) ? (long)par * a.stage_stride : 0;   // staged bucket half

  // ---- 1. CE from the summed logits (rounded like the bf16 Dense output) -> dlogits
  float l_loss = 0.f, l_corr = 0.f;
  if constexpr (PST) {
    // Four lanes per row: every lane repeats the row's cheap serial parts (max / argmax over
    // the gathered logits, the sum in class order, one log) and computes the transcendentals
    // and bf16 dlogits of its own classes only -- the one-step kernel's values bit for bit
    // (same operations on the same operands, sums in the same order).  The zero padding
    // of dlB / dlT (classes >= C, rows >= M) is written by the launch's first step only:
    // M does not change in a launch and no later phase writes these arrays.
    float mx = -INFINITY;
    int am = 0;
#pragma unroll
    for (int c = 0; c < C; ++c) {
      if (lrow[c] > mx) { mx = lrow[c]; am = c; }
    }
    float ex[CK];
#pragma unroll
    for (int k = 0; k < CK; ++k) ex[k] = __expf(lown[k] - mx);
    float s = 0.f;
#pragma unroll
    for (int c = 0; c < C; ++c) s += quad_lane(ex[c >> 2], c & 3);
    const float lse = mx + __logf(s);
    if (crow < M) {
#pragma unroll
      for (int k = 0; k < CK; ++k) {
        const int c = cq + 4 * k;
        if (c < C) {
          const bf16_t gb = f2bf((__expf(lown[k] - lse) - (c == lab ? 1.f : 0.f)) * a.inv_mb);
          dlT[c * LDM + crow] = gb;
          dlB[crow * LDB + c] = gb;
        }
      }
      // the row's loss / hit go to thread = row (pst_metrics, the metric slots) after the barrier
      if (lead && cq == 0) { cel[0][crow] = lse - lrow[lab]; cel[1][crow] = (am == lab) ? 1.f : 0.f; }
    }
    if (pp.it == 0) {
      for (int idx = tid; idx < MPM * 32; idx += NT) {
        const int r = idx >> 5, c = idx & 31;
        if (r >= M || c >= C) dlB[r * LDB + c] = 0;
      }
      for (int idx = tid; idx < 16 * MPM; idx += NT) {
        const int c = idx / MPM, r = idx % MPM;
        if (r >= M || c >= C) dlT[c * LDM + r] = 0;
      }
    }
    if ((tid & 31) < C) w2B[(tid >> 5) * LDB + (tid & 31)] = par ? w2b : w2a;
    else if (pp.it == 0) w2B[(tid >> 5) * LDB + (tid & 31)] = 0;
  } else {
  if (tid < M) {
    float mx = -INFINITY;
    int am = 0;
#pragma unroll
    for (int c = 0; c < C; ++c) {
      lrow[c] = round_bf(lrow[c]);
      if (lrow[c] > mx) { mx = lrow[c]; am = c; }
    }
    float s = 0.f;
#pragma unroll
    for (int c = 0; c < C; ++c) s += __expf(lrow[c] - mx);
    const float lse = mx + __logf(s);
    l_loss = lse - lrow[lab];
    l_corr = (am == lab) ? 1.f : 0.f;
    unsigned row[16];
#pragma unroll
    for (int q = 0; q < 16; ++q) row[q] = 0u;
#pragma unroll
    for (int c = 0; c < C; ++c) {
      const bf16_t gb = f2bf((__expf(lrow[c] - lse) - (c == lab ? 1.f : 0.f)) * a.inv_mb);
      row[c >> 1] |= (unsigned)gb << (16 * (c & 1));
      dlT[c * LDM + tid] = gb;
    }
#pragma unroll
    for (int q = 0; q < 4; ++q)
      *reinterpret_cast<u32x4*>(&dlB[tid * LDB + 8 * q]) = (u32x4){row[4 * q], row[4 * q + 1], row[4 * q + 2], row[4 * q + 3]};
  } else if (tid < MPM) {
#pragma unroll
    for (int c = 0; c < C; ++c) dlT[c * LDM + tid] = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) *reinterpret_cast<u32x4*>(&dlB[tid * LDB + 8 * q]) = (u32x4){0u, 0u, 0u, 0u};
  }
  for (int idx = tid; idx < (16 - C) * MPM; idx += NT) dlT[(C + idx / MPM) * LDM + idx % MPM] = 0;
  w2B[(tid >> 5) * LDB + (tid & 31)] = (tid & 31) < C ? (par ? w2b : w2a) : (bf16_t)0;
  }
  if (lead && !PST) {
    l_loss = wave_sum(l_loss);
    l_corr = wave_sum(l_corr);
    if (lane == 0) { red[0][w] = l_loss; red[1][w] = l_corr; }
  }
  if (lead) {
    // re-arm the accumulator of the step after next (run-ahead: step t+1's forward
    // accumulates into buffer (t+1) % 3 during this launch)
    float* nxt = a.logits + (long)(AHEAD ? (step + 2) % 3 : (par ^ 1)) * M * C;
    if constexpr (!PST)
      for (int i = tid; i < M * C; i += NT) st_f<SCX>(nxt + i, 0.f);
  }
  if constexpr (PST) {
    // persistent: every workgroup re-arms 8 words (write-through), so the lead workgroup
    // -- and with it its column block, which everyone then waits for at the grid barrier --
    // does not drain 1,280 sc1 stores before its column barrier (stamps: column block 0
    // was the step's last by ~0.5 us)
    float* nxt = a.logits + (long)((step + 2) % 3) * M * C;
    const int G = (int)(gridDim.x * gridDim.y), t = by * (int)gridDim.x + bx;
    if (tid < 8)
      for (int i = t * 8 + tid; i < M * C; i += G * 8) st_f<true>(nxt + i, 0.f);
  }
  if constexpr (AHEAD) {   // K padding of the W1' tile image (persistent: the first step's stays)
    if (!PST || pp.it == 0)
      for (int idx = tid; idx < 16 * (128 - KC); idx += NT) w1n[(idx / (128 - KC)) * LDW1 + KC + idx % (128 - KC)] = 0;
  }
  __syncthreads();
  STAMP(1);
  if constexpr (PST) {
    // the lead's rows' loss / hit, thread = row: folded into the metrics while waiting in
    // the grid barrier (pst_metrics); N > 1: the metric slots ride the exchange
    if (lead) {
      l_loss = tid < M ? cel[0][tid] : 0.f;
      l_corr = tid < M ? cel[1][tid] : 0.f;
      R->l_loss = l_loss;
      R->l_corr = l_corr;
      if constexpr (TX) {
        l_loss = wave_sum(l_loss);
        l_corr = wave_sum(l_corr);
        if (lane == 0) { red[0][w] = l_loss; red[1][w] = l_corr; }
      }
    }
  }

  // ---- 2. dZ1 = (dlogits W2[blk]^T) * G1: one MFMA per wave (rows 16w.., K = classes);
  // the output lane layout (rows 4*(lane>>4)+e, column lane&15) is this thread's
  // dropout group (rg, gn), so G1's float4 multiplies in place.  H1 -> LDS.
  {
    const bf16x8 af = *reinterpret_cast<const bf16x8*>(&dlB[(w * 16 + (lane & 15)) * LDB + 8 * (lane >> 4)]);
    const bf16x8 bw = *reinterpret_cast<const bf16x8*>(&w2B[(lane & 15) * LDB + 8 * (lane >> 4)]);
    const f32x4 dh = mfma16x16x32(af, bw, (f32x4){0.f, 0.f, 0.f, 0.f});
    const float gv[4] = {__uint_as_float(g1q.x), __uint_as_float(g1q.y), __uint_as_float(g1q.z),
                         __uint_as_float(g1q.w)};
    unsigned packed[2] = {0u, 0u};
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float v = rg * 4 + e < M ? dh[e] * gv[e] : 0.f;
      packed[e >> 1] |= (unsigned)f2bf(v) << (16 * (e & 1));
    }
    *reinterpret_cast<uint2*>(&dzT[gn * LDM + rg * 4]) = make_uint2(packed[0], packed[1]);
    if (chunk0)
      *reinterpret_cast<uint2*>(&h1T[gn * LDM + rg * 4]) =
          make_uint2((unsigned)hv[0] | ((unsigned)hv[1] << 16), (unsigned)hv[2] | ((unsigned)hv[3] << 16));
  }
  __syncthreads();
  STAMP(2);

  // mval: lead, tid < 4 -- the all-reduced metric slot of the N > 1 exchange (TX)
  float mval = 0.f;
  if constexpr (!TX && !P3S) {
    // one GPU: each tile's MFMA result goes straight into its epilogue
    // ---- 3. dW1[chunk, blk] = X[:, chunk]^T dZ1[:, blk]   (K = rows) on MFMA; one tile per wave
    if (w < NTILE) {
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  #pragma unroll
      for (int ks = 0; ks < MPM / 32; ++ks) {
        if (ks < Mp / 32) {
          const int kk = ks * 32 + 8 * (lane >> 4);
          const bf16x8 bfr = *reinterpret_cast<const bf16x8*>(&dzT[(lane & 15) * LDM + kk]);
          acc = mfma16x16x32(xf[ks], bfr, acc);
        }
      }
      if (w == 0) PSTAMP(15, acc[0]);   // wave 0: dW1 tile on MFMA done
      unsigned wt[2] = {0u, 0u};
  #pragma unroll
      for (int e = 0; e < 4; ++e) {
        const long idx = (long)(trow0 + e) * H + tcol;   // K_IN % KC == 0: always in range
        if (a.fuse_opt) {
          float tp, tm = om[e], tv = ov[e];
          const bf16_t pb = f2bf(adam_apply(op[e], om[e], ov[e], acc[e], ak, &tp, &tm, &tv));
          if constexpr (PST) {
            // persistent launch: the state stays in registers (stored after the last step)
            R->op[e] = tp; R->om[e] = tm; R->ov[e] = tv;
          } else if (AHEAD && (a.wt & 1)) {
            st_f<true>(a.pW1 + idx, tp);
            if (!ak.sgd) { st_f<true>(a.mW1 + idx, tm); st_f<true>(a.vW1 + idx, tv); }
          } else {
            a.pW1[idx] = tp;
            if (!ak.sgd) { a.mW1[idx] = tm; a.vW1[idx] = tv; }   // SGD: m / v alias p (unused)
          }
          // with the W1^T copy, the [in,out] bf16 shadow is rebuilt from it by
          // FusedMLP2.finalize() instead of being written every step (0.8 MB of HBM writes)
          if (!a.W1T) a.sW1[idx] = pb;
          wt[e >> 1] |= (unsigned)pb << (16 * (e & 1));
        } else if (a.smap) {
          stage_store(a.smap, par, 0, trow0 + e, tcol, acc[e]);
        } else {
          a.gW1[goff + idx] = acc[e];
        }
      }
      // the lane's 4 rows are 4 consecutive K elements of W1^T: one 8-byte store
      if (!PST && a.fuse_opt && a.W1T) {   // persistent: the next steps read w1n (LDS), not W1^T
        const unsigned long long w8 = (unsigned long long)wt[0] | ((unsigned long long)wt[1] << 32);
        if (LOOP || (AHEAD && (a.wt & 1))) st_u64<true>(a.W1T + (long)tcol * a.ldw1t + trow0, w8);
        else st_u64<false>(a.W1T + (long)tcol * a.ldw1t + trow0, w8);
      }
      if constexpr (AHEAD)
        *reinterpret_cast<uint2*>(&w1n[(lane & 15) * LDW1 + (trow0 - kc0)]) = make_uint2(wt[0], wt[1]);
      if (w == 0) PSTAMP(14, __uint_as_float(wt[0]));   // wave 0: AdamW + W1' tile done
    } else if (aux) {
      // chunk-0 blocks, concurrently with the dW1 tiles:
      //   dW2[blk, :] = H1[:, blk]^T dlogits ; db1[blk] = dZ1[:, blk]^T 1 ; db2 = 1^T dlogits (block (0,0))
      bf16x8 ones;
  #pragma unroll
      for (int q = 0; q < 8; ++q) ones[q] = (short)0x3f80;  // bf16 1.0
      f32x4 aw = {0.f, 0.f, 0.f, 0.f}, ab1 = {0.f, 0.f, 0.f, 0.f}, ab2 = {0.f, 0.f, 0.f, 0.f};
  #pragma unroll
      for (int ks = 0; ks < MPM / 32; ++ks) {
        if (ks >= Mp / 32) break;
        const int kk = ks * 32 + 8 * (lane >> 4);
        const bf16x8 hT = *reinterpret_cast<const bf16x8*>(&h1T[(lane & 15) * LDM + kk]);
        const bf16x8 dT = *reinterpret_cast<const bf16x8*>(&dlT[(lane & 15) * LDM + kk]);
        const bf16x8 zT = *reinterpret_cast<const bf16x8*>(&dzT[(lane & 15) * LDM + kk]);
        aw = mfma16x16x32(hT, dT, aw);
        ab1 = mfma16x16x32(zT, ones, ab1);
        if (lead && !PST) ab2 = mfma16x16x32(ones, dT, ab2);
      }
      bf16_t* sW2n = par ? a.sW2_0 : a.sW2_1;   // next step's parity buffer
  #pragma unroll
      for (int e = 0; e < 4; ++e) {
        // lanes ac < C: W2[j0+n][ac]; lane ac == C: b1[j0+n] (every column of ab1 holds
        // db1, B = ones) -- one AdamW code path for both, its state loaded in phase 0
        const int n = (lane >> 4) * 4 + e;
        if (ac <= C) {
          const bool isb = ac == C;
          const long o = isb ? (long)(j0 + n) : (long)(j0 + n) * C + ac;
          const float gr = isb ? ab1[e] : aw[e];
          if (a.fuse_opt) {
            float pn;
            if constexpr (PST) {
              float tp, tm = om[e], tv = ov[e];
              pn = adam_apply(op[e], om[e], ov[e], gr, ak, &tp, &tm, &tv);
              R->op[e] = tp; R->om[e] = tm; R->ov[e] = tv;
            } else {
              pn = adam_apply_h<LOOP>(op[e], om[e], ov[e], gr, ak, (isb ? a.pb1 : a.pW2) + o,
                                      (isb ? a.mb1 : a.mW2) + o, (isb ? a.vb1 : a.vW2) + o);
            }
            (isb ? a.sb1 : sW2n)[o] = f2bf(pn);
            if constexpr (AHEAD) a.hand[(isb ? 0 : H) + o] = pn;   // same XCD as the reader (L2)
          } else if (a.smap) {
            if (isb) stage_store(a.smap, par, 1, j0 + n, 0, gr);
            else stage_store(a.smap, par, 2, j0 + n, ac, gr);
          } else {
            (isb ? a.gb1 : a.gW2)[goff + o] = gr;
          }
        }
      }
      if (!PST && lead && lane < C) {
        if (a.fuse_opt) {
          const float pn = adam_apply_h<LOOP>(qp, qm, qv, ab2[0], ak, a.pb2 + lane, a.mb2 + lane, a.vb2 + lane);
          a.sb2[lane] = f2bf(pn);
          if constexpr (AHEAD) a.hand[H + (long)H * C + lane] = pn;
        } else if (a.smap) {
          stage_store(a.smap, par, 3, lane, 0, ab2[0]);
        } else {
          a.gb2[goff + lane] = ab2[0];
        }
      }
      PSTAMP(5, aw[0]);   // aux wave: dW2 / db1 / db2 + their AdamW done
    } else if (PST && bx == 0 && by == 1 && w == NW - 1) {
      // persistent: db2 = 1^T dlogits and b2's AdamW on the otherwise idle last wave of
      // block (0,1) instead of the lead's aux wave (the lead's extra work held its column
      // block -- and so the grid barrier -- back by ~0.5 us); the same MFMA sum and AdamW,
      // handed to the column block's forward epilogues like the lead's was
      bf16x8 ones;
  #pragma unroll
      for (int q = 0; q < 8; ++q) ones[q] = (short)0x3f80;  // bf16 1.0
      f32x4 ab2 = {0.f, 0.f, 0.f, 0.f};
  #pragma unroll
      for (int ks = 0; ks < MPM / 32; ++ks) {
        if (ks >= Mp / 32) break;
        const int kk = ks * 32 + 8 * (lane >> 4);
        const bf16x8 dT = *reinterpret_cast<const bf16x8*>(&dlT[(lane & 15) * LDM + kk]);
        ab2 = mfma16x16x32(ones, dT, ab2);
      }
      if (lane < C) {
        float tp, tm = qm, tv = qv;
        const float pn = adam_apply(qp, qm, qv, ab2[0], ak, &tp, &tm, &tv);
        R->qp = tp; R->qm = tm; R->qv = tv;
        a.sb2[lane] = f2bf(pn);
        a.hand[H + (long)H * C + lane] = pn;
      }
    }
  } else {
    // N > 1 (TX): all MFMAs, then the tile exchange, then the epilogues
    // ---- 3. dW1[chunk, blk] = X[:, chunk]^T dZ1[:, blk]   (K = rows) on MFMA; one tile per wave
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    // chunk-0 blocks' spare wave, concurrently with the dW1 tiles:
    //   dW2[blk, :] = H1[:, blk]^T dlogits ; db1[blk] = dZ1[:, blk]^T 1 ; db2 = 1^T dlogits (block (0,0))
    f32x4 aw = {0.f, 0.f, 0.f, 0.f}, ab1 = {0.f, 0.f, 0.f, 0.f}, ab2 = {0.f, 0.f, 0.f, 0.f};
    if (w < NTILE) {
  #pragma unroll
      for (int ks = 0; ks < MPM / 32; ++ks) {
        if (ks < Mp / 32) {
          const int kk = ks * 32 + 8 * (lane >> 4);
          const bf16x8 bfr = *reinterpret_cast<const bf16x8*>(&dzT[(lane & 15) * LDM + kk]);
          acc = mfma16x16x32(xf[ks], bfr, acc);
        }
      }
    } else if (aux) {
      bf16x8 ones;
  #pragma unroll
      for (int q = 0; q < 8; ++q) ones[q] = (short)0x3f80;  // bf16 1.0
  #pragma unroll
      for (int ks = 0; ks < MPM / 32; ++ks) {
        if (ks >= Mp / 32) break;
        const int kk = ks * 32 + 8 * (lane >> 4);
        const bf16x8 hT = *reinterpret_cast<const bf16x8*>(&h1T[(lane & 15) * LDM + kk]);
        const bf16x8 dT = *reinterpret_cast<const bf16x8*>(&dlT[(lane & 15) * LDM + kk]);
        const bf16x8 zT = *reinterpret_cast<const bf16x8*>(&dzT[(lane & 15) * LDM + kk]);
        aw = mfma16x16x32(hT, dT, aw);
        ab1 = mfma16x16x32(zT, ones, ab1);
        if (lead) ab2 = mfma16x16x32(ones, dT, ab2);
      }
    }
    if constexpr (FX) {
      // FSDP at N > 1 (the reference's dim-0 shards: W1 rows in K_IN / W blocks, W2 / b1 rows
      // in H / W blocks; b2 replicated): every element's partial goes to the rank that owns
      // its row, the owner sums in rank order, applies the SHARDED AdamW (its local state)
      // and pushes the updated fp32 value to every rank; replicated b2 and the metric slots
      // are summed by rank T % W and pushed back as sums (every rank updates its own copy).
      // Then every rank holds the whole updated tile and runs the next forward from it.
      const TxArgs* X = a.tx;
      PstRegs* const R_ = R;   // the persistent launch's registers (R names the rank here)
      const int R = fx_R, W = __builtin_amdgcn_readfirstlane(X->world);
      const int T = bx * NCH + by;
      const long pay = __builtin_amdgcn_readfirstlane(X->pay), tiles = __builtin_amdgcn_readfirstlane(X->tiles);
      const unsigned long long tb = (unsigned long long)pay * 4ull;
      const unsigned epoch = (unsigned)step + 1u;
      const long AG = tiles * TX_MAX_RANKS + tiles;   // flag base of the updated-value hand-back
      const int o_lo = kc0 / fx_rpq, o_hi = (kc0 + KC - 1) / fx_rpq, ob = j0 / fx_hpq, orep = T % W;
      auto owner_of = [&](int q) { return (q >= o_lo && q <= o_hi) || (chunk0 && q == ob) || (lead && q == orep); };
      if (lead && tid < 4) {
        float L = 0.f, Cr = 0.f;
        for (int q = 0; q < NW; ++q) { L += red[0][q]; Cr += red[1][q]; }
        mval = tid == 0 ? L : tid == 2 ? Cr : (float)M;   // {loss sum, n, correct, n}
      }
      float ev[4];          // waves < NTILE: this lane's 4 W1 elements; aux: dW2 (ac < C) / db1 (ac == C)
      int eo[4];            // their owners
      int epos[4];          // payload positions
      int ne = 0;
      if (w < NTILE) {
#pragma unroll
        for (int e = 0; e < 4; ++e) { ev[e] = acc[e]; eo[e] = (trow0 + e) / fx_rpq; epos[e] = w * 256 + lane * 4 + e; }
        ne = 4;
      } else if (aux && ac <= C) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          ev[e] = ac == C ? ab1[e] : aw[e];
          eo[e] = ob;
          epos[e] = (ac == C ? 8 * 256 : 7 * 256) + lane * 4 + e;
        }
        ne = 4;
      }
      // replicated scalar of this thread: lead's db2 (aux lanes < C) or metric slot (tid < 4)
      int rpos = -1;
      float rv = 0.f;
      if (lead && aux && lane < C) { rpos = 9 * 256 + lane; rv = ab2[0]; }
      if (lead && tid < 4) { rpos = 9 * 256 + 64 + tid; rv = mval; }
      // 1. partials to their owners: one uniform resource per candidate owner (a W1 chunk's
      // rows have at most two, o_lo / o_hi; the aux rows one, ob); a lane whose element
      // belongs elsewhere stores out of range (offset pay: dropped by the bounds check), so
      // no resource is lane-dependent (that compiled into readfirstlane waterfall loops)
      {
        const int cand[3] = {o_lo, o_hi, ob};
#pragma unroll
        for (int ci = 0; ci < 3; ++ci) {
          const int c = cand[ci];
          if (c == R || (ci >= 1 && c == cand[0]) || (ci == 2 && c == cand[1]) || (ci == 2 && !chunk0)) continue;
          const __amdgpu_buffer_rsrc_t rr = sys_rsrc_u(sgpr_ptr(X->part[c]) + ((long)T * TX_MAX_RANKS + R) * pay, tb);
#pragma unroll
          for (int e = 0; e < 4; ++e) sys_store1(rr, (e < ne && eo[e] == c) ? (long)epos[e] : pay, ev[e]);
        }
      }
      if (rpos >= 0 && orep != R)
        sys_store1(sys_rsrc_u(sgpr_ptr(X->part[orep]) + ((long)T * TX_MAX_RANKS + R) * pay, tb), rpos, rv);
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __syncthreads();
      if (tid < W && tid != R && owner_of(tid))
        tx_flag_store(X->flag[tid] + (long)T * TX_MAX_RANKS + R, epoch);
      // 2. this rank's owned elements: rank-ordered sums, sharded AdamW, hand-back
      float pnew[4] = {0.f, 0.f, 0.f, 0.f};
      if (owner_of(R)) {
        if (tid < W && tid != R) tx_wait(X->flag[R] + (long)T * TX_MAX_RANKS + tid, epoch, X->timeout, a.ztick + 1);
        __syncthreads();
        const float* inbox = sgpr_ptr(X->part[R]) + (long)T * TX_MAX_RANKS * pay;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          if (e >= ne || eo[e] != R) continue;
          float sacc = 0.f;
          for (int q = 0; q < W; ++q) {
            const float x = q == R ? ev[e] : sys_load1(sys_rsrc_u(inbox + (long)q * pay, tb), epos[e]);
            sacc = q == 0 ? x : sacc + x;
          }
          ev[e] = sacc;
        }
        if (rpos >= 0 && orep == R) {
          float sacc = 0.f;
          for (int q = 0; q < W; ++q) {
            const float x = q == R ? rv : sys_load1(sys_rsrc_u(inbox + (long)q * pay, tb), rpos);
            sacc = q == 0 ? x : sacc + x;
          }
          rv = sacc;
        }
        // sharded AdamW on the owned elements (state prefetched at local indices in phase 0)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          if (e >= ne || eo[e] != R) continue;
          if (w < NTILE) {
            const long li = (long)(trow0 + e - R * fx_rpq) * H + tcol;
            float tp, tm = om[e], tv = ov[e];
            adam_apply(op[e], om[e], ov[e], ev[e], ak, &tp, &tm, &tv);
            if constexpr (PST) {   // persistent: the owned shard's state stays in registers
              R_->op[e] = tp; R_->om[e] = tm; R_->ov[e] = tv;
            } else {
              a.pW1[li] = tp; a.mW1[li] = tm; a.vW1[li] = tv;
            }
            pnew[e] = tp;
          } else {
            const int n = (lane >> 4) * 4 + e;
            const bool isb = ac == C;
            const long li = isb ? (long)(j0 + n - R * fx_hpq) : (long)(j0 + n - R * fx_hpq) * C + ac;
            float tp, tm = om[e], tv = ov[e];
            adam_apply(op[e], om[e], ov[e], ev[e], ak, &tp, &tm, &tv);
            if constexpr (PST) {
              R_->op[e] = tp; R_->om[e] = tm; R_->ov[e] = tv;
            } else {
              (isb ? a.pb1 : a.pW2)[li] = tp; (isb ? a.mb1 : a.mW2)[li] = tm; (isb ? a.vb1 : a.vW2)[li] = tv;
            }
            pnew[e] = tp;
          }
        }
        for (int q = 0; q < W; ++q) {
          if (q == R) continue;
          const __amdgpu_buffer_rsrc_t dst = sys_rsrc_u(sgpr_ptr(X->red[q]) + (long)T * pay, tb);
#pragma unroll
          for (int e = 0; e < 4; ++e)
            if (e < ne && eo[e] == R) sys_store1(dst, epos[e], pnew[e]);
          if (rpos >= 0 && orep == R) sys_store1(dst, rpos, rv);
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if (tid < W && tid != R)
          tx_flag_store(X->flag[tid] + AG + (long)T * TX_MAX_RANKS + R, epoch);
      }
      // 3. the other owners' updated values
      if (tid < W && tid != R && owner_of(tid)) tx_wait(X->flag[R] + AG + (long)T * TX_MAX_RANKS + tid, epoch, X->timeout, a.ztick + 1);
      __syncthreads();
      {
        const __amdgpu_buffer_rsrc_t src = sys_rsrc_u(sgpr_ptr(X->red[R]) + (long)T * pay, tb);
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (e < ne && eo[e] != R) pnew[e] = sys_load1(src, epos[e]);
        if (rpos >= 0 && orep != R) rv = sys_load1(src, rpos);
      }
      if (lead && tid < 4) mval = rv;
      // 4. the whole updated tile: W1^T copy + the next forward's LDS image; W2 / b1 shadows
      // and hand-offs; b2 (replicated) updated by every rank from the summed gradient
      if (w < NTILE) {
        unsigned wt[2] = {0u, 0u};
#pragma unroll
        for (int e = 0; e < 4; ++e) wt[e >> 1] |= (unsigned)f2bf(pnew[e]) << (16 * (e & 1));
        st_u64<true>(a.W1T + (long)tcol * a.ldw1t + trow0, (unsigned long long)wt[0] | ((unsigned long long)wt[1] << 32));
        *reinterpret_cast<uint2*>(&w1n[(lane & 15) * LDW1 + (trow0 - kc0)]) = make_uint2(wt[0], wt[1]);
      } else if (aux) {
        bf16_t* sW2n = par ? a.sW2_0 : a.sW2_1;   // next step's parity buffer
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int n = (lane >> 4) * 4 + e;
          if (ac <= C) {
            const bool isb = ac == C;
            const long o = isb ? (long)(j0 + n) : (long)(j0 + n) * C + ac;
            (isb ? a.sb1 : sW2n)[o] = f2bf(pnew[e]);
            a.hand[(isb ? 0 : H) + o] = pnew[e];
          }
        }
        if (lead && lane < C) {
          float pn;
          if constexpr (PST) {   // b2 (replicated): every rank's own copy, in registers
            float tp, tm = qm, tv = qv;
            pn = adam_apply(qp, qm, qv, rv, ak, &tp, &tm, &tv);
            R_->qp = tp; R_->qm = tm; R_->qv = tv;
          } else {
            pn = adam_apply_h<LOOP>(qp, qm, qv, rv, ak, a.pb2 + lane, a.mb2 + lane, a.vb2 + lane);
          }
          a.sb2[lane] = f2bf(pn);
          a.hand[H + (long)H * C + lane] = pn;
        }
      }
    } else {
      // N > 1 (Mlp2Args::tx): this tile's gradients -- and the lead's db2 and metric slots --
      // all-reduced with the same tile of the other ranks' launches before the optimizer
      if constexpr (AHEAD && TX) {
        {
          if (lead && tid < 4) {
            float L = 0.f, Cr = 0.f;
            for (int q = 0; q < NW; ++q) { L += red[0][q]; Cr += red[1][q]; }
            mval = tid == 0 ? L : tid == 2 ? Cr : (float)M;   // {loss sum, n, correct, n}
          }
          float4 v4[2];
          int p4[2], n4 = 0, ps = -1;
          float vs = 0.f;
          if (w < NTILE) {
            v4[0] = make_float4(acc[0], acc[1], acc[2], acc[3]);
            p4[0] = w * 256 + lane * 4;
            n4 = 1;
            if (lead && tid < 4) { vs = mval; ps = (NTILE + 2) * 256 + 64 + tid; }
          } else if (aux) {
            v4[0] = make_float4(aw[0], aw[1], aw[2], aw[3]);
            v4[1] = make_float4(ab1[0], ab1[1], ab1[2], ab1[3]);
            p4[0] = NTILE * 256 + lane * 4;
            p4[1] = (NTILE + 1) * 256 + lane * 4;
            n4 = 2;
            if (lead && lane < C) { vs = ab2[0]; ps = (NTILE + 2) * 256 + lane; }
          }
          STAMP(12);
          tx_tile(a.tx, bx * NCH + by, (unsigned)step + 1u, n4, v4, p4, vs, ps, a.ztick + 1);
          STAMP(13);
          if (w < NTILE) {
            acc = (f32x4){v4[0].x, v4[0].y, v4[0].z, v4[0].w};
            if (lead && tid < 4) mval = vs;
          } else if (aux) {
            aw = (f32x4){v4[0].x, v4[0].y, v4[0].z, v4[0].w};
            ab1 = (f32x4){v4[1].x, v4[1].y, v4[1].z, v4[1].w};
            if (lead && lane < C) ab2[0] = vs;
          }
        }
      }
      if (w < NTILE) {
        unsigned wt[2] = {0u, 0u};
    #pragma unroll
        for (int e = 0; e < 4; ++e) {
          const long idx = (long)(trow0 + e) * H + tcol;   // K_IN % KC == 0: always in range
          if (a.fuse_opt) {
            float tp, tm = om[e], tv = ov[e];
            const bf16_t pb = f2bf(adam_apply(op[e], om[e], ov[e], acc[e], ak, &tp, &tm, &tv));
            if constexpr (PST) {
              // persistent N > 1: the state stays in registers (stored after the last step)
              R->op[e] = tp; R->om[e] = tm; R->ov[e] = tv;
            } else if (AHEAD && (a.wt & 1)) {
              st_f<true>(a.pW1 + idx, tp);
              if (!ak.sgd) { st_f<true>(a.mW1 + idx, tm); st_f<true>(a.vW1 + idx, tv); }
            } else {
              a.pW1[idx] = tp;
              if (!ak.sgd) { a.mW1[idx] = tm; a.vW1[idx] = tv; }   // SGD: m / v alias p (unused)
            }
            // with the W1^T copy, the [in,out] bf16 shadow is rebuilt from it by
            // FusedMLP2.finalize() instead of being written every step (0.8 MB of HBM writes)
            if (!a.W1T) a.sW1[idx] = pb;
            wt[e >> 1] |= (unsigned)pb << (16 * (e & 1));
          } else if (a.smap) {
            stage_store(a.smap, par, 0, trow0 + e, tcol, acc[e]);
          } else {
            a.gW1[goff + idx] = acc[e];
          }
        }
        // the lane's 4 rows are 4 consecutive K elements of W1^T: one 8-byte store
        // (persistent: the next steps read w1n; W1^T is stored after the last one)
        if (!PST && a.fuse_opt && a.W1T) {
          const unsigned long long w8 = (unsigned long long)wt[0] | ((unsigned long long)wt[1] << 32);
          if (LOOP || (AHEAD && (a.wt & 1))) st_u64<true>(a.W1T + (long)tcol * a.ldw1t + trow0, w8);
          else st_u64<false>(a.W1T + (long)tcol * a.ldw1t + trow0, w8);
        }
        if constexpr (AHEAD)
          *reinterpret_cast<uint2*>(&w1n[(lane & 15) * LDW1 + (trow0 - kc0)]) = make_uint2(wt[0], wt[1]);
      } else if (aux) {
        bf16_t* sW2n = par ? a.sW2_0 : a.sW2_1;   // next step's parity buffer
    #pragma unroll
        for (int e = 0; e < 4; ++e) {
          // lanes ac < C: W2[j0+n][ac]; lane ac == C: b1[j0+n] (every column of ab1 holds
          // db1, B = ones) -- one AdamW code path for both, its state loaded in phase 0
          const int n = (lane >> 4) * 4 + e;
          if (ac <= C) {
            const bool isb = ac == C;
            const long o = isb ? (long)(j0 + n) : (long)(j0 + n) * C + ac;
            const float gr = isb ? ab1[e] : aw[e];
            if (a.fuse_opt) {
              float pn;
              if constexpr (PST) {
                float tp, tm = om[e], tv = ov[e];
                pn = adam_apply(op[e], om[e], ov[e], gr, ak, &tp, &tm, &tv);
                R->op[e] = tp; R->om[e] = tm; R->ov[e] = tv;
              } else {
                pn = adam_apply_h<LOOP>(op[e], om[e], ov[e], gr, ak, (isb ? a.pb1 : a.pW2) + o,
                                        (isb ? a.mb1 : a.mW2) + o, (isb ? a.vb1 : a.vW2) + o);
              }
              (isb ? a.sb1 : sW2n)[o] = f2bf(pn);
              if constexpr (AHEAD) a.hand[(isb ? 0 : H) + o] = pn;   // same XCD as the reader (L2)
            } else if (a.smap) {
              if (isb) stage_store(a.smap, par, 1, j0 + n, 0, gr);
              else stage_store(a.smap, par, 2, j0 + n, ac, gr);
            } else {
              (isb ? a.gb1 : a.gW2)[goff + o] = gr;
            }
          }
        }
        if (lead && lane < C) {
          if (a.fuse_opt) {
            float pn;
            if constexpr (PST) {   // persistent N > 1: b2 stays with the lead's aux wave
              float tp, tm = qm, tv = qv;
              pn = adam_apply(qp, qm, qv, ab2[0], ak, &tp, &tm, &tv);
              R->qp = tp; R->qm = tm; R->qv = tv;
            } else {
              pn = adam_apply_h<LOOP>(qp, qm, qv, ab2[0], ak, a.pb2 + lane, a.mb2 + lane, a.vb2 + lane);
            }
            a.sb2[lane] = f2bf(pn);
            if constexpr (AHEAD) a.hand[H + (long)H * C + lane] = pn;
          } else if (a.smap) {
            stage_store(a.smap, par, 3, lane, 0, ab2[0]);
          } else {
            a.gb2[goff + lane] = ab2[0];
          }
        }
      }
    }
  }
  __syncthreads();
  STAMP(3);

  if ((!PST || TX) && lead && tid < 4) {
    float val = mval;   // N > 1 run-ahead: the all-reduced slot
    if (!(AHEAD && TX)) {
      float L = 0.f, Cr = 0.f;
      for (int q = 0; q < NW; ++q) { L += red[0][q]; Cr += red[1][q]; }
      val = tid == 0 ? L : tid == 2 ? Cr : (float)M;   // {loss sum, n, correct, n}
    }
    if (fo && a.running) a.running[tid] = run_pre + val;
    else if (a.smap) stage_store(a.smap, par, 4, tid, 0, val);
    else if (a.mslot) a.mslot[goff + tid] = val;
    // advance the device step: every other workgroup of this launch reads the
    // forward's copy (step_copy), so no arrival ticket is needed
    if (!LOOP && !AHEAD && fo && tid == 0) a.step[0] = step + 1;   // the loop kernel advances it at its end
  }
  if constexpr (AHEAD) {
    // tile-map check (xcd_column_tile): this tile's counter, only touched on this XCD,
    // must read the launch number
    unsigned tile_seen = 0u, launch_no = 0u;
    if (tid == 0) {
      launch_no = PST ? pp.launch0 + (unsigned)pp.it : a.ztick[2];
      const int tpx = (H / 16) * NCH / 8, t = bx * NCH + by;   // tiles per XCD, this tile
      tile_seen = __hip_atomic_fetch_add((gu32_t*)(a.ztick + 32 * (1 + H / 16) + 32 * ((tpx + 31) / 32) * (t / tpx) + t % tpx),
                                         1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
    // ---- 5. step t+1's partial Z1 for (chunk, blk): wave w -> rows 16w.., K = this chunk
    f32x4 z = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      if (ks * 32 < KC) {
        const bf16x8 bw = *reinterpret_cast<const bf16x8*>(&w1n[(lane & 15) * LDW1 + ks * 32 + 8 * (lane >> 4)]);
        z = mfma16x16x32(xa[ks], bw, z);
      }
    }
    // lane: rows 16w + 4(lane>>4) + e of column j0 + (lane & 15) = one 4-row dropout group.
    // The column block's workgroups run on ONE XCD (xcd_column_tile), so the hand-off
    // lives in that XCD's L2: plain stores (L1 is write-through) drained by vmcnt, an
    // L2 counter (workgroup-scope atomics), loads with sc1 (never served by the L1).
    float* const zb = sgpr_ptr(a.zslab + (long)bx * NCH * (MPM / 4) * 64);   // scalar: a buffer resource base
    {
      const long zo = ((long)by * (MPM / 4) + w * 4 + (lane >> 4)) * 64 + (lane & 15) * 4;
      const u32x4 zv = {__float_as_uint(z[0]), __float_as_uint(z[1]), __float_as_uint(z[2]), __float_as_uint(z[3])};
      if (a.wt & 2) st_b128<true>(zb + zo, zv);
      else *reinterpret_cast<u32x4*>(zb + zo) = zv;
    }
    // step t+1's dropout bits of this thread's epilogue element, computed while the
    // partial store drains (off the phase-0 critical path)
    if (a.keep < 1.f && eg < g_hi && eg * 4 < M)
      dbn = dropout_bits(a.seed, a.offset + ((unsigned long long)(unsigned)(step + 1) << 32),
                         dropout_group(0, eg * 4, j0 + gn, M, H));
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // partials, hand-offs, launch_no: in the L2 / read
    STAMP(8);
    __syncthreads();
    // ---- column-block barrier: all NCH workgroups of the column block are resident
    // (one launch of H/16 * NCH <= CU-count workgroups); monotonic counter, so no reset.
    // A wall-clock timeout (s_memrealtime) raises the error word instead of hanging.
    if (tid == 0) {
      unsigned* cnt = sgpr_ptr(a.ztick + 32 * (1 + bx));
      __hip_atomic_fetch_add((gu32_t*)cnt, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      const unsigned target = (unsigned)NCH * (launch_no + 1u);
      const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
      // poll with sc1 loads (never served by this CU's L1, which is coherent only
      // within a workgroup; an idempotent atomic such as +0 is folded into a plain load)
      const __amdgpu_buffer_rsrc_t cr = __builtin_amdgcn_make_buffer_rsrc(cnt, (short)0, 4, 0x00020000);
      while ((int)((unsigned)__builtin_amdgcn_raw_buffer_load_b32(cr, 0, 0, 16) - target) < 0) {
        if ((long long)(__builtin_amdgcn_s_memrealtime() - t0) > 2000000ll) {   // 20 ms
          atomicOr(a.ztick + 1, 2u);
          break;
        }
        __builtin_amdgcn_s_sleep(1);
        asm volatile("" ::: "memory");
      }
      if (tile_seen != launch_no) atomicOr(a.ztick + 1, 1u);   // a tile ran twice / not at all
    }
    __syncthreads();
    STAMP(9);
    // ---- 6. step t+1's forward epilogue, row groups [g_lo, g_hi) of column block blk
    const int ng = g_hi - g_lo;
    const __amdgpu_buffer_rsrc_t zr = __builtin_amdgcn_make_buffer_rsrc(zb, (short)0, NCH * (MPM / 4) * 64 * 4, 0x00020000);
    const __amdgpu_buffer_rsrc_t hr =
        __builtin_amdgcn_make_buffer_rsrc(sgpr_ptr(a.hand), (short)0, (int)((H + H * C + C) * 4), 0x00020000);
    float zp[NCH];
    const int egc = min(eg, g_hi - 1);
#pragma unroll
    for (int q = 0; q < NCH; ++q)
      zp[q] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(
                                            zr, (int)((((long)q * (MPM / 4) + egc) * 64 + gn * 4 + ee) * 4), 0, 16));
    const float b1v = round_bf(__builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(hr, (j0 + gn) * 4, 0, 16)));
    if (tid < 16 * C)
      w2A[tid / C][tid % C] =
          round_bf(__builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(hr, (H + j0 * C + tid) * 4, 0, 16)));
    if (tid < C)
      b2A[tid] = bx == 0 ? round_bf(__builtin_bit_cast(
                               float, __builtin_amdgcn_raw_buffer_load_b32(hr, (H + H * C + tid) * 4, 0, 16)))
                         : 0.f;
    if (a.stamps) {   // diagnostic: wait for the partials before stamping
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      STAMP(10);
    }
    if (tid < 64 * ng) {
      const int row = eg * 4 + ee;
      float hvn = 0.f;
      if (row < M) {
        float v = b1v;   // + the NCH chunk partials in chunk order
#pragma unroll
        for (int q = 0; q < NCH; ++q) v += zp[q];
        const float zz = bf2f(f2bf(v));           // Z1 as the bf16 Dense output
        const float ez = __expf(-zz);
        hvn = zz / (1.0f + ez);                    // act_fwd(ACT_SILU)
        const float sg = 1.0f / (1.0f + ez);
        float gd = sg * (1.0f + zz * (1.0f - sg));  // act_grad(ACT_SILU)
        if (a.keep < 1.f) {
          const bool kp = keep_word(dbn, ee, a.keep);
          hvn = kp ? hvn / a.keep : 0.f;
          gd = kp ? gd / a.keep : 0.f;
        }
        const bf16_t hb = f2bf(hvn);
        hvn = bf2f(hb);
        // G1 / H1 element (row group eg, column j0+gn, slot ee) of the dropout-group layout
        const long gq = ((long)eg * H + j0 + gn) * 4 + ee;
        if (a.wt & 2) st_f<true>(a.G1 + gq, gd);
        else a.G1[gq] = gd;
        a.H1[gq] = hb;
      }
      htA[(tid >> 6) * 4 + ee][gn] = hvn;
    }
    __syncthreads();
    STAMP(11);
    float* lgn = a.logits + (long)((step + 1) % 3) * M * C;
    const int r0 = g_lo * 4, nr = min(ng * 4, M - r0);
    if (tid < nr * C) {
      const int rl = tid / C, c = tid % C;
      float sacc = b2A[c];
#pragma unroll
      for (int n = 0; n < 16; ++n) sacc += htA[rl][n] * w2A[n][c];
      if (a.det_logits) {
        // deterministic: this column block's partial (b2 in block 0's, as the forward
        // kernel), summed in block order by the next step's backward
        float* const dp = a.det_logits + (((long)((step + 1) % 3) * (H / 16) + bx) * M + r0 + rl) * C + c;
        if constexpr (PST) st_f<true>(dp, sacc);   // read on other XCDs after the grid barrier
        else *dp = sacc;
      } else if constexpr (PST) {
        // returning atomics: the wait for the returned value is the proof that the add was
        // PERFORMED at the memory side (a no-return add's vmcnt acknowledgement is not), so
        // the grid barrier's arrival orders it before every reader of the next step; without
        // it the XCD-local release let a reader see 99 % of the parameters ~1e-6 off
        const float old = __hip_atomic_fetch_add((gf32_t*)(lgn + (long)(r0 + rl) * C + c), sacc, __ATOMIC_RELAXED,
                                                 __HIP_MEMORY_SCOPE_AGENT);
        asm volatile("" ::"v"(old));
      } else {
        atomicAdd(lgn + (long)(r0 + rl) * C + c, sacc);
      }
    }
    // every workgroup read the step counter before the column barrier; one workgroup
    // per column block reports, the last of them advances the step and launch counters
    if (!PST && by == 0 && tid == 0 &&
        __hip_atomic_fetch_add((gu32_t*)a.ztick, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) ==
            (unsigned)(H / 16 - 1)) {
      __hip_atomic_store((gu32_t*)a.ztick, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      a.step[0] = step + 1;
      a.ztick[2] = launch_no + 1u;
    }
    if (PST && pp.done) {
      // column-block completion (persistent CBW form): this workgroup's epilogue is in
      // memory -- its logit adds returned (performed at the memory side), its G1 / H1 and
      // its step-start logits re-arm drained -- then one agent-scope add on the column
      // block's own line; the next step waits for all of them instead of a grid barrier
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __syncthreads();
      if (tid == 0)
        __hip_atomic_fetch_add((gu32_t*)(pp.done + 32 * bx), 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
  STAMP(4);
#pragma pop_macro("STAMP")
#undef PSTAMP
}

// ---------------------------------------------------------------------------- kernels
template <int K_IN, int C, int RB, bool DIRECT, bool XCD>
__global__ void __launch_bounds__(NT) mlp2_fwd_kernel(Mlp2Args a) {
  int bx = blockIdx.x, by = blockIdx.y;
  // XCD-contiguous: each XCD takes whole column blocks (1/8 of W1) over all row blocks
  if constexpr (XCD) xcd_contiguous_tile(bx, by);
  mlp2_fwd_body<K_IN, C, RB, DIRECT, false>(static_cast<const Mlp2Args&>(a), bx, by, 0);
}
template <int K_IN, int C, int KC, bool XCD, bool AHEAD = false, bool TX = false, bool P3S = false, bool FX = false>
__global__ void __launch_bounds__(NT) mlp2_bwd_kernel(Mlp2Args a) {
  int bx = blockIdx.x, by = blockIdx.y;
  if constexpr (AHEAD) xcd_column_tile(bx, by);
  else if constexpr (XCD) xcd_contiguous_tile(bx, by);
  mlp2_bwd_body<K_IN, C, KC, false, AHEAD, TX, P3S, FX>(static_cast<const Mlp2Args&>(a), bx, by, 0);
}

// n complete training steps in ONE launch (single GPU, fused AdamW, W1^T copy):
// every workgroup plays a forward role (16-row block x hidden block) and a
// backward role (hidden block x input chunk) per step, with a grid barrier after
// each phase instead of a kernel boundary (the boundary measured 2.36 us from the
// forward's last store to the backward's first instruction: tools/stamp_mlp2.py).
// Requires every workgroup resident at once (checked by the launcher).
template <int K_IN, int C, int KC>
__global__ void __launch_bounds__(NT) mlp2_loop_kernel(Mlp2Args a, Mlp2Loop l) {
  __shared__ int sync_flag[1];
  const int b = blockIdx.x, G = gridDim.x;
  const int nrb = (a.M + 15) / 16, nhb = a.H / 16;
  const int nfwd = nrb * nhb, nbwd = nhb * (K_IN / KC);
  // both written only by block 0 after its last barrier (every block has read them by then)
  const int step0 = a.step[0];
  const unsigned base = l.base[0];
  int it = 0;
  // The bodies read their arguments through a kernarg-segment pointer laundered
  // per phase (an empty asm), so the ~50 argument words are scalar-loaded next to
  // their uses instead of being hoisted out of the loop and kept live across both
  // phases (that spilled 127 SGPRs and 24 VGPRs to scratch).
  typedef const __attribute__((address_space(4))) Mlp2Args KArgs;
  KArgs* const kbase = (KArgs*)(__builtin_amdgcn_kernarg_segment_ptr());
#define LSTAMP(k)                                                                                   \
  do {                                                                                              \
    if (l.stamps && threadIdx.x == 0) l.stamps[((long)b * l.n + it) * 5 + (k)] = __builtin_amdgcn_s_memrealtime(); \
  } while (0)
  for (; it < l.n; ++it) {
    const int step = step0 + it;
    KArgs* kf = kbase;
    asm volatile("" : "+s"(kf));
    LSTAMP(0);
    if (b < nfwd) mlp2_fwd_body<K_IN, C, 16, true, true>(*kf, b % nrb, b / nrb, step);
    LSTAMP(1);
    if (!grid_sync(l, base + (2u * it + 1u) * (unsigned)G, sync_flag)) break;
    LSTAMP(2);
    KArgs* kb = kbase;
    asm volatile("" : "+s"(kb));
    if (b < nbwd) mlp2_bwd_body<K_IN, C, KC, true>(*kb, b % nhb, b / nhb, step);
    LSTAMP(3);
    if (it + 1 < l.n && !grid_sync(l, base + (2u * it + 2u) * (unsigned)G, sync_flag)) break;
    LSTAMP(4);
  }
#undef LSTAMP
  if (b == 0 && threadIdx.x == 0 && it == l.n) {
    a.step[0] = step0 + l.n;
    l.base[0] = base + (2u * l.n - 1u) * (unsigned)G;
  }
}

// XCD-hierarchical grid barrier of the persistent run-ahead launch (profiles/r5_barrier_lab.txt:
// 1.92 us, the cost of the kernel boundary it replaces).  ws: 128-byte lines -- 0: the
// generation count of completed barriers (advanced by the host-visible end of a launch),
// 1: top counter, 2 + x: XCD x's arrival counter, 10 + x: XCD x's release word (the grid is
// dealt round-robin over the 8 XCDs, probed: G / 8 workgroups each).  Every wave drains its
// stores and atomics first (vmcnt), so the step's hand-offs (sc1 / atomic for cross-XCD
// bytes, L2 for the column block's own XCD) are complete before anyone passes.  A
// wall-clock timeout (the launch's `tmo` ticks: 20 ms by default, scaled by the host like
// the other in-kernel waits) raises bit 8 of the error word and every workgroup leaves;
// the counters are then out of step and the host re-zeroes them (FusedMLP2.finalize).
// Arrival: every wave drains, then one lane adds to its XCD's counter (an L2 atomic: the
// line is only touched by that XCD's workgroups); the XCD's last arriver -- told by the
// value its add returned -- adds 1 to the cross-XCD top counter.  The caller may compute
// between arrival and the wait.  Returns (to lane 0) whether this workgroup arrived last.
__device__ __forceinline__ bool pst_arrive(unsigned* ws, unsigned& xcc) {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  bool last = false;
  // read by every lane (a scalar register): set inside the lane-0 branch it would come out
  // of the branch as a vector value, and the poll's buffer resource with it
  asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID, 0, 4)" : "=s"(xcc));
  xcc &= 7u;
  if (threadIdx.x == 0) {
    const unsigned per = (gridDim.x * gridDim.y) / 8u;
    const unsigned old =
        __hip_atomic_fetch_add((gu32_t*)(ws + 32 * (2 + xcc)), 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    // scalar: the poll's buffer resource is chosen by it (a lane value would compile into a
    // readfirstlane waterfall loop, tests/test_isa_waterfalls.py)
    last = __builtin_amdgcn_readfirstlane(old % per == per - 1 ? 1u : 0u) != 0u;
    if (last) __hip_atomic_fetch_add((gu32_t*)(ws + 32), 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  return last;
}
// bounded poll of one word until it reaches `target` (sc1 loads: never an L1 copy)
__device__ __forceinline__ bool pst_poll(unsigned* word, unsigned target, unsigned* errw, long long tmo) {
  const __amdgpu_buffer_rsrc_t r = __builtin_amdgcn_make_buffer_rsrc(word, (short)0, 4, 0x00020000);
  const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
  while ((int)((unsigned)__builtin_amdgcn_raw_buffer_load_b32(r, 0, 0, 16) - target) < 0) {
    if ((long long)(__builtin_amdgcn_s_memrealtime() - t0) > tmo) {
      atomicOr(errw + 1, 8u);
      return false;
    }
    __builtin_amdgcn_s_sleep(1);
    asm volatile("" ::: "memory");
  }
  return true;
}
// Wait: each XCD's last arriver polls the top counter (8 arrivals per generation, at the
// cross-XCD coherence point) and then releases its XCD through a word in that XCD's L2
// (line 10 + x), which the XCD's other workgroups poll -- 8 pollers of the shared counter
// instead of every workgroup, the rest served by their own L2.
__device__ __forceinline__ bool pst_wait(unsigned* ws, unsigned gen, bool last, unsigned xcc, int* ok_lds,
                                         unsigned* errw, long long tmo) {
  if (threadIdx.x == 0) {
    int ok = 1;
    unsigned* rel = sgpr_ptr(ws + 32 * (10 + xcc));
    if (__builtin_amdgcn_readfirstlane(last ? 1u : 0u)) {
      ok = pst_poll(ws + 32, 8u * gen, errw, tmo);
      __hip_atomic_store((gu32_t*)rel, gen, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    } else {
      ok = pst_poll(rel, gen, errw, tmo);
    }
    ok_lds[0] = ok;
  }
  __syncthreads();
  return ok_lds[0] != 0;
}

// Column-block wait (mlp2_pst_kernel CBW): step it's backward needs step it's logits -- the
// sum of every column block's partials -- and, from its own column block, G1 / H1 and the
// W2 shadow; all of them are in memory once every column block's NCH workgroups have added
// to their completion counter (PstPos::done).  Lanes 0 .. nb-1 of wave 0 poll one counter
// each (sc1) until it reaches `target`; bounded like pst_poll (error bit 8).
__device__ __forceinline__ bool cb_wait(const unsigned* done, int nb, unsigned target, int* ok_lds, unsigned* errw,
                                        long long tmo) {
  if (threadIdx.x < 64) {
    const int lane = threadIdx.x;
    const __amdgpu_buffer_rsrc_t r = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<unsigned*>(done), (short)0, 32 * 4 * 64, 0x00020000);
    const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
    int ok = 1;
    while (true) {
      // every lane loads (lanes past nb re-read the last line): no branch around the load
      const unsigned v = (unsigned)__builtin_amdgcn_raw_buffer_load_b32(r, 32 * 4 * min(lane, nb - 1), 0, 16);
      if (__builtin_amdgcn_ballot_w64((int)(v - target) < 0) == 0ull) break;
      if ((long long)(__builtin_amdgcn_s_memrealtime() - t0) > tmo) {
        if (lane == 0) atomicOr(errw + 1, 8u);
        ok = 0;
        break;
      }
      __builtin_amdgcn_s_sleep(1);
      asm volatile("" ::: "memory");
    }
    if (lane == 0) ok_lds[0] = ok;
  }
  __syncthreads();
  return ok_lds[0] != 0;
}

// The AdamW state a persistent launch carries in registers (PstRegs), loaded before its
// first step and stored after its last: the elements each lane owns in mlp2_bwd_body's
// phase-3 epilogues (same indices) -- tile waves 4 W1 elements (plus their W1^T bf16
// copy), the chunk-0 aux wave W2 / b1 (lanes ac <= C) and, in block (0,0), b2.
template <int K_IN, int C, int KC, bool TX, class AT, bool FX = false>
__device__ __forceinline__ void pst_state_io(AT& a, const int bx, const int by, PstRegs& R, const bool store) {
  constexpr int NTILE = KC / 16;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, H = a.H;
  const int j0 = bx * 16, kc0 = by * KC;
  const bool aux = by == 0 && w == NW - 1;
  const int ac = lane & 15;
  const bool w2l = aux && ac < C;
  const int trow0 = kc0 + min(w, NTILE - 1) * 16 + (lane >> 4) * 4, tcol = j0 + (lane & 15);
  const bool sgd = a.opt_sgd != 0;
  if constexpr (FX) {
    // FSDP (mlp2_bwd FX): this rank's LOCAL shards -- W1 rows [R K/W, (R+1) K/W), W2 / b1
    // rows [R H/W, (R+1) H/W) -- indexed as the body's phase 0 does; only owned elements are
    // stored back (the others' registers hold clamped, unused values); b2 is replicated.
    // W1^T is written by the body every step (its non-owned elements come from the owners).
    const int Rk = __builtin_amdgcn_readfirstlane(a.tx->rank), Wk = __builtin_amdgcn_readfirstlane(a.tx->world);
    const int rpq = K_IN / Wk, hpq = H / Wk;
    float* const pW1 = sgpr_ptr(a.pW1); float* const mW1 = sgpr_ptr(a.mW1); float* const vW1 = sgpr_ptr(a.vW1);
    float* const pW2 = sgpr_ptr(a.pW2); float* const mW2 = sgpr_ptr(a.mW2); float* const vW2 = sgpr_ptr(a.vW2);
    float* const pb1 = sgpr_ptr(a.pb1); float* const mb1 = sgpr_ptr(a.mb1); float* const vb1 = sgpr_ptr(a.vb1);
    float* const pb2 = sgpr_ptr(a.pb2); float* const mb2 = sgpr_ptr(a.mb2); float* const vb2 = sgpr_ptr(a.vb2);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int n = (lane >> 4) * 4 + e;
      const int lr = aux ? min(max(j0 + n - Rk * hpq, 0), hpq - 1) : min(max(trow0 + e - Rk * rpq, 0), rpq - 1);
      const long idx = aux ? (w2l ? (long)lr * C + ac : (long)lr) : (long)lr * H + tcol;
      float* const sp = aux ? (w2l ? pW2 : pb1) : pW1;
      float* const sm = aux ? (w2l ? mW2 : mb1) : mW1;
      float* const sv = aux ? (w2l ? vW2 : vb1) : vW1;
      if (!store) {
        R.op[e] = ld_global(sp + idx); R.om[e] = ld_global(sm + idx); R.ov[e] = ld_global(sv + idx);
      } else {
        const bool owned = aux ? (ac <= C && (j0 + n) / hpq == Rk) : (w < NTILE && (trow0 + e) / rpq == Rk);
        if (owned) {
          sp[idx] = R.op[e];
          if (!sgd) { sm[idx] = R.om[e]; sv[idx] = R.ov[e]; }
        }
      }
    }
    const int lq = min(lane, C - 1);
    if (!store) {
      R.qp = ld_global(pb2 + lq); R.qm = ld_global(mb2 + lq); R.qv = ld_global(vb2 + lq);
    } else if (bx == 0 && by == 0 && w == NW - 1 && lane < C) {
      pb2[lane] = R.qp;
      if (!sgd) { mb2[lane] = R.qm; vb2[lane] = R.qv; }
    }
    return;
  }
  // argument words as scalar values first, then per-lane selects between those values
  // (a select between two fields of the by-value argument block made the compiler give
  // the kernel a private copy of it: a scratch segment, set up at the first launch)
  float* const pW1 = sgpr_ptr(a.pW1); float* const mW1 = sgpr_ptr(a.mW1); float* const vW1 = sgpr_ptr(a.vW1);
  float* const pW2 = sgpr_ptr(a.pW2); float* const mW2 = sgpr_ptr(a.mW2); float* const vW2 = sgpr_ptr(a.vW2);
  float* const pb1 = sgpr_ptr(a.pb1); float* const mb1 = sgpr_ptr(a.mb1); float* const vb1 = sgpr_ptr(a.vb1);
  float* const pb2 = sgpr_ptr(a.pb2); float* const mb2 = sgpr_ptr(a.mb2); float* const vb2 = sgpr_ptr(a.vb2);
  if (!store) {
    float* const sp = aux ? (w2l ? pW2 : pb1) : pW1;
    float* const sm = aux ? (w2l ? mW2 : mb1) : mW1;
    float* const sv = aux ? (w2l ? vW2 : vb1) : vW1;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int n = (lane >> 4) * 4 + e;
      const long idx = aux ? (w2l ? (long)(j0 + n) * C + ac : (long)(j0 + n)) : (long)(trow0 + e) * H + tcol;
      R.op[e] = ld_global(sp + idx); R.om[e] = ld_global(sm + idx); R.ov[e] = ld_global(sv + idx);
    }
    const int lq = min(lane, C - 1);   // b2: block (0,1)'s last wave (mlp2_bwd_body PST)
    R.qp = ld_global(pb2 + lq); R.qm = ld_global(mb2 + lq); R.qv = ld_global(vb2 + lq);
    return;
  }
  if (w < NTILE) {
    unsigned wt[2] = {0u, 0u};
    const bool wt1 = (a.wt & 1) != 0;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const long idx = (long)(trow0 + e) * H + tcol;
      if (wt1) {
        st_f<true>(pW1 + idx, R.op[e]);
        if (!sgd) { st_f<true>(mW1 + idx, R.om[e]); st_f<true>(vW1 + idx, R.ov[e]); }
      } else {
        pW1[idx] = R.op[e];
        if (!sgd) { mW1[idx] = R.om[e]; vW1[idx] = R.ov[e]; }
      }
      wt[e >> 1] |= (unsigned)f2bf(R.op[e]) << (16 * (e & 1));
    }
    const unsigned long long w8 = (unsigned long long)wt[0] | ((unsigned long long)wt[1] << 32);
    bf16_t* const W1T = sgpr_ptr(a.W1T);
    if (wt1) st_u64<true>(W1T + (long)tcol * a.ldw1t + trow0, w8);
    else st_u64<false>(W1T + (long)tcol * a.ldw1t + trow0, w8);
  } else if (aux) {
    if (ac <= C) {
      const bool isb = ac == C;
      float* const dp = isb ? pb1 : pW2;
      float* const dm = isb ? mb1 : mW2;
      float* const dv = isb ? vb1 : vW2;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int n = (lane >> 4) * 4 + e;
        const long o = isb ? (long)(j0 + n) : (long)(j0 + n) * C + ac;
        dp[o] = R.op[e];
        if (!sgd) { dm[o] = R.om[e]; dv[o] = R.ov[e]; }
      }
    }
  }
  // b2's state: block (0,1)'s last wave on one GPU, the lead's aux wave with the exchange
  if (bx == 0 && by == (TX ? 0 : 1) && w == NW - 1 && lane < C) {
    pb2[lane] = R.qp;
    if (!sgd) { mb2[lane] = R.qm; vb2[lane] = R.qv; }
  }
}

// The batch operands a persistent launch keeps in registers (PstX): mlp2_bwd_body's phase-0
// fragments at the same addresses, and the label of the lane's CE row.  by: the tile's chunk.
template <int K_IN, int KC, bool HX, class AT>
__device__ __forceinline__ void pst_x_load(AT& a, const int by, PstX& X) {
  if constexpr (HX) {
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      X.xf[ks] = mlp2_xf_frag<KC, false>(a, by * KC, ks);
      X.xa[ks] = mlp2_xa_frag<K_IN>(a, by * KC, ks);
    }
  }
  X.lab = a.labels[min((int)threadIdx.x >> 2, a.M - 1)];
}

// Block (0,0), persistent launch: the step's loss sum / hits folded into the running metrics
// ({loss sum, n, correct, n}: the per-step kernel's metric slot), between arriving at the grid
// barrier and waiting on it (or after the last step) -- off the step's critical path.
__device__ __forceinline__ void pst_metrics(float* running, int M, const PstRegs& R, float (*red)[NW]) {
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const float L = wave_sum(R.l_loss), Cr = wave_sum(R.l_corr);
  if (lane == 0) { red[0][w] = L; red[1][w] = Cr; }
  __syncthreads();
  if (tid < 4) {
    float Ls = 0.f, Cs = 0.f;
    for (int q = 0; q < NW; ++q) { Ls += red[0][q]; Cs += red[1][q]; }
    running[tid] += tid == 0 ? Ls : tid == 2 ? Cs : (float)M;
  }
}

// n run-ahead steps in ONE launch (single GPU, fused AdamW, W1^T copy): step i's CE,
// backward and AdamW plus step i+1's forward, then the grid barrier, n times.  The AdamW
// state of every workgroup's tile stays in registers across the steps (PstRegs) -- the
// per-step reload and write-back of p / m / v (9.6 MB of L2 / HBM traffic a step) and the
// launch ramp are gone; the last step stores the state, W1^T and the shadows as the
// one-step kernel does.  The batch is the launch's too: each lane's X fragments and CE label
// are loaded before the first step (PstX; WPE = 4 keeps the per-step fragment loads, its
// 128 VGPRs already spill), the zero padding of the step's LDS images is written by the
// first step only, and the CE runs on four lanes per row.  Same arithmetic as n launches of mlp2_bwd_kernel<..., AHEAD>, up
// to the arrival order of the memory-side logit atomics (fp32 sums in a different order):
// tests/test_mlp2_persistent_gpu.py bounds the difference (median <= 1e-5 x the update
// scale, p99.9 <= 1e-4 x).  Requires every workgroup
// resident at once and round-robin XCD dispatch (the run-ahead's own conditions).
//
// TX (N > 1 data parallel, Mlp2Args::tx): every step's gradient tiles are all-reduced with
// the same tiles of the other ranks' persistent launches inside the step (the one-launch
// step's tile exchange, common.h tx_tile: epochs = optimizer step + 1, single-buffered
// inboxes -- a rank pushes step t+1's partial only after it read step t's reduced tile,
// which the owner sends only after it has read step t's partials), so the n steps of a
// replay are one launch per rank.  The metric slots ride the exchange (every rank folds
// the all-reduced sums); b2 stays with the lead's aux wave.  Requires every workgroup of
// every rank resident (one rank per GPU; two ranks sharing one only while both grids fit:
// the WPE = 4 variant, <= 128 VGPRs, two workgroups per CU).
//
// CBW (column-block wait): between steps, instead of the grid barrier, every workgroup
// waits until every column block's NCH workgroups have finished the step's forward
// epilogue (PstPos::done: one counter line per column block, monotonic, base ws[1] = the
// persistent steps run so far) -- one agent-scope add per workgroup and a poll of H/16
// lines, against the barrier's XCD counter, cross-XCD counter and per-XCD release.
//
// FX (with TX): the FSDP form -- every gradient element goes to the rank owning its row,
// the owner applies the sharded AdamW to its LOCAL state (carried in registers across the
// steps like the replicated form's) and hands the value back (mlp2_bwd_body FX).
template <int K_IN, int C, int KC, bool TX = false, int WPE = 1, bool CBW = false, bool FX = false>
__global__ void __launch_bounds__(NT) __attribute__((amdgpu_waves_per_eu(WPE)))
mlp2_pst_kernel(Mlp2Args a, int n, unsigned* ws, long long tmo) {
  __shared__ int ok_lds[1];
  __shared__ float red_lds[2][NW];
  if (n <= 0) return;   // warm-up launch (jdt_mlp2_pst n = 0): touches nothing
  int bx = blockIdx.x, by = blockIdx.y;
  xcd_column_tile(bx, by);
  // read before the first barrier; block (0,0) rewrites them only after the last one
  const int step0 = a.step[0];
  const unsigned launch0 = a.ztick[2];
  const unsigned gen0 = ws[0];
  const unsigned cb0 = ws[1];   // CBW: persistent steps before this launch
  unsigned* const done = CBW ? ws + 32 * 18 : nullptr;
  // the body's ~50 argument words re-read from the kernarg segment each step (laundered
  // pointer) instead of being held live across the loop (by value: 107 SGPRs spilled)
  typedef const __attribute__((address_space(4))) Mlp2Args KArgs;
  KArgs* const kbase = (KArgs*)(__builtin_amdgcn_kernarg_segment_ptr());
  PstRegs R;
  pst_state_io<K_IN, C, KC, TX, Mlp2Args, FX>(a, bx, by, R, false);
  R.l_loss = R.l_corr = 0.f;   // the lead's threads set them every step
  PstX PX;
  pst_x_load<K_IN, KC, WPE == 1>(a, by, PX);
  {
    const AdamK k0 = adam_consts(*kbase, step0);
    R.rbc1 = k0.rbc1;
    R.rbc2 = k0.rbc2;
  }
  int it = 0;
  // diagnostic stamps (Mlp2Args::stamps; the body stamps the phases of step n-2, sub-phases
  // in slots 5, 14, 15): slot 7 = start of step n-1, 12 / 13 = before / after the barrier
  // between them, 6 = the tile (bx + 256 * by) this workgroup plays
  unsigned long long* const stw =
      a.stamps && threadIdx.x == 0 ? a.stamps + (long)(blockIdx.y * gridDim.x + blockIdx.x) * 16 : nullptr;
  for (; it < n; ++it) {
    KArgs* k = kbase;
    asm volatile("" : "+s"(k));
    if (stw && it == n - 1) stw[7] = __builtin_amdgcn_s_memrealtime();
    // the tile coordinates re-made scalar each step: carried across the loop they may sit
    // in VGPRs, and the buffer resources built from them would become waterfall loops
    mlp2_bwd_body<K_IN, C, KC, false, true, TX, false, FX, true, WPE == 1>(
        *k, __builtin_amdgcn_readfirstlane(bx), __builtin_amdgcn_readfirstlane(by), step0 + it, &R,
        PstPos{it, n, launch0, done}, &PX);
    if (stw && it == n - 2) stw[12] = __builtin_amdgcn_s_memrealtime();
    if (it + 1 < n) {
      if constexpr (CBW) {
        if (!TX && bx == 0 && by == 0) pst_metrics(a.running, a.M, R, red_lds);
        const AdamK kn = adam_consts(*kbase, step0 + it + 1);
        R.rbc1 = kn.rbc1;
        R.rbc2 = kn.rbc2;
        constexpr int NCH_ = K_IN / KC;
        if (!cb_wait(done, a.H / 16, (unsigned)NCH_ * (cb0 + (unsigned)it + 1u), ok_lds, a.ztick, tmo)) break;
      } else {
        unsigned xcc = 0u;
        const bool last = pst_arrive(ws, xcc);
        if (!TX && bx == 0 && by == 0) pst_metrics(a.running, a.M, R, red_lds);
        // the next step's bias corrections, while the other workgroups arrive
        const AdamK kn = adam_consts(*kbase, step0 + it + 1);
        R.rbc1 = kn.rbc1;
        R.rbc2 = kn.rbc2;
        if (!pst_wait(ws, gen0 + (unsigned)it + 1u, last, xcc, ok_lds, a.ztick, tmo)) break;
      }
    }
    if (stw && it == n - 2) stw[13] = __builtin_amdgcn_s_memrealtime();
  }
  if (it == n) {
    if (!TX && bx == 0 && by == 0) pst_metrics(a.running, a.M, R, red_lds);
    pst_state_io<K_IN, C, KC, TX, Mlp2Args, FX>(a, bx, by, R, true);
  }
  if (stw) stw[6] = (unsigned long long)(bx + 256 * by);
  if (bx == 0 && by == 0 && threadIdx.x == 0 && it == n) {
    a.step[0] = step0 + n;
    a.ztick[2] = launch0 + (unsigned)n;
    ws[0] = gen0 + (unsigned)(n - 1);
    ws[1] = cb0 + (unsigned)n;   // every step of the launch added NCH to every done line
  }
}

}  // namespace jdt
using namespace jdt;

JDT_API int jdt_mlp2_args_size() { return (int)sizeof(Mlp2Args); }

static int g_mlp2_rb = 16;  // forward rows per workgroup (jdt_mlp2_set_rows: 16 or 32, A/B tests)
JDT_API void jdt_mlp2_set_rows(int rb) { g_mlp2_rb = rb == 32 ? 32 : 16; }
// workgroup -> tile map (A/B: JDT_XCD_TILES): 1 = XCD-contiguous (xcd_contiguous_tile) in the
// forward and backward kernels, 2 = backward only, 0 = identity everywhere
static int g_xcd_tiles = -1;
int xcd_tiles_enabled() {
  if (g_xcd_tiles < 0) {
    const char* e = getenv("JDT_XCD_TILES");
    g_xcd_tiles = (e && (e[0] == '0' || e[0] == '2')) ? e[0] - '0' : 1;
  }
  return g_xcd_tiles;
}

// phase 0: forward, 1: backward.  Supported: K_IN = 784, C = 10, H % 16 == 0, M <= 128.
static int mlp2_loop_grid(int M, int H) { return max(((M + 15) / 16) * (H / 16), (H / 16) * (784 / 112)); }

// workgroups of mlp2_loop_kernel the device holds at once (0 if unknown)
static int mlp2_loop_resident() {
  static int resident = -1;
  if (resident < 0) {
    int dev = 0, cus = 0, per = 0;
    if (hipGetDevice(&dev) != hipSuccess ||
        hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess ||
        hipOccupancyMaxActiveBlocksPerMultiprocessor(&per, mlp2_loop_kernel<784, 10, 112>, NT, 0) != hipSuccess)
      return 0;
    resident = cus * per;
  }
  return resident;
}

// 1 if the loop kernel can run M rows x H hidden units on this device (every
// workgroup resident at once); called before graph capture.
JDT_API int jdt_mlp2_loop_ok(int M, int H) {
  return (H % 16 == 0 && M > 0 && M <= 128 && mlp2_loop_grid(M, H) <= mlp2_loop_resident()) ? 1 : 0;
}

// Persistent n-step launch; -4 if the grid cannot be fully resident (caller then
// uses the two-launch path).
JDT_API int jdt_mlp2_loop(const Mlp2Args* args, int n, unsigned* ctr, unsigned* base, int* err, long long timeout,
                          unsigned long long* stamps, void* stream) {
  const Mlp2Args& a = *args;
  if (a.H % 16 || a.M <= 0 || a.M > 128 || n <= 0 || !a.fuse_opt || !a.W1T || !a.W2snap || !ctr || !base || !err)
    return -3;
  const int grid = mlp2_loop_grid(a.M, a.H);
  if (grid > mlp2_loop_resident()) return -4;
  Mlp2Loop l;
  l.n = n; l.ctr = ctr; l.base = base; l.err = err; l.timeout = timeout; l.stamps = stamps;
  hipLaunchKernelGGL((mlp2_loop_kernel<784, 10, 112>), dim3(grid), dim3(NT), 0, static_cast<hipStream_t>(stream), a, l);
  return HIP_LAUNCH_CHECK();
}

// ---------------------------------------------------------------- XCD dispatch probe
// The run-ahead tile map (common.h xcd_column_tile) is a bijection only when the
// device deals workgroups round-robin over exactly 8 XCDs (linear id L -> XCD
// (L + o) % 8).  A partitioned device (CPX / DPX mode: fewer XCDs per logical GPU)
// or another part would run some tiles twice and others never.  This probe
// launches a grid of G workgroups that each record HW_REG_XCC_ID, and the host
// checks the assumption the tile map makes: the 8 residues L % 8 land on 8
// distinct XCC ids, every workgroup of a residue on the same one.
__global__ void xcd_probe_kernel(int* out) {
  unsigned xcc;
  asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID, 0, 4)" : "=s"(xcc));
  if (threadIdx.x == 0) out[blockIdx.x] = (int)xcc;
}

// 1 if a G-workgroup launch is dealt round-robin over 8 XCDs (checked on 3 launches).
int xcd_roundrobin_ok(int G) {
  static int cached_g = -1, cached = 0;
  if (G == cached_g) return cached;
  if (G <= 0 || G % 8) return 0;
  int ok = 1;
  int* d = nullptr;
  hipStream_t st = nullptr;
  if (hipMalloc(&d, sizeof(int) * G) != hipSuccess) return 0;
  if (hipStreamCreateWithFlags(&st, hipStreamNonBlocking) != hipSuccess) { hipFree(d); return 0; }
  int* h = static_cast<int*>(malloc(sizeof(int) * G));
  for (int rep = 0; rep < 3 && ok; ++rep) {
    hipLaunchKernelGGL(xcd_probe_kernel, dim3(G), dim3(64), 0, st, d);
    if (hipStreamSynchronize(st) != hipSuccess || hipMemcpy(h, d, sizeof(int) * G, hipMemcpyDeviceToHost) != hipSuccess) {
      ok = 0;
      break;
    }
    unsigned seen = 0;
    for (int r = 0; r < 8 && ok; ++r) {
      const int x = h[r];
      if (x < 0 || x > 7 || (seen >> x) & 1u) ok = 0;
      seen |= 1u << (x & 7);
      for (int L = r; L < G && ok; L += 8) ok = h[L] == x;
    }
  }
  free(h);
  hipStreamDestroy(st);
  hipFree(d);
  cached_g = G;
  cached = ok;
  return ok;
}
JDT_API int jdt_xcd_roundrobin_ok(int G) { return xcd_roundrobin_ok(G); }

// 1 if the run-ahead backward can run M rows x H hidden units of input width K_IN here:
// its column-block barrier needs every workgroup of the launch resident at once, its tile
// map needs round-robin dispatch over 8 XCDs (probed), and the forward's X^T side output
// one input chunk per hidden block.  Called before capture.
template <int K_IN>
static int mlp2_ahead_ok_k(int M, int H, int nshare, bool tx) {
  constexpr int NCH = K_IN / mlp2_kc<K_IN>();
  if (H % 128 || M <= 0 || M > 128 || H / 16 < NCH || nshare < 1) return 0;
  if (!xcd_roundrobin_ok((H / 16) * NCH)) return 0;
  int dev = 0, cus = 0, per = 0;
  if (hipGetDevice(&dev) != hipSuccess ||
      hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess)
    return 0;
  const hipError_t e = tx ? hipOccupancyMaxActiveBlocksPerMultiprocessor(
                                &per, mlp2_bwd_kernel<K_IN, 10, mlp2_kc<K_IN>(), true, true, true>, NT, 0)
                          : hipOccupancyMaxActiveBlocksPerMultiprocessor(
                                &per, mlp2_bwd_kernel<K_IN, 10, mlp2_kc<K_IN>(), true, true>, NT, 0);
  if (e != hipSuccess) return 0;
  return (long)nshare * (H / 16) * NCH <= (long)cus * per ? 1 : 0;
}

// 1 if the persistent run-ahead launch can run M rows x H hidden units of input width
// K_IN here: the run-ahead's conditions, a grid of whole XCD shares (G % 8 == 0) and every
// workgroup of the persistent kernel resident at once.
// nshare > 0: the N > 1 form (tile exchange) with `nshare` ranks' grids on this GPU -- every
// workgroup of every sharing rank's persistent launch resident at once.
template <int K_IN>
static int mlp2_pst_ok_k(int M, int H, int nshare, bool fx = false) {
  constexpr int KC = mlp2_kc<K_IN>(), NCH = K_IN / KC;
  if (!mlp2_ahead_ok_k<K_IN>(M, H, nshare > 0 ? nshare : 1, nshare > 0)) return 0;
  const int G = (H / 16) * NCH;
  if (G % 8) return 0;
  int dev = 0, cus = 0, per = 0;
  if (hipGetDevice(&dev) != hipSuccess ||
      hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess)
    return 0;
  const hipError_t e =
      fx ? (nshare > 1 ? hipOccupancyMaxActiveBlocksPerMultiprocessor(
                             &per, mlp2_pst_kernel<K_IN, 10, KC, true, 4, false, true>, NT, 0)
                       : hipOccupancyMaxActiveBlocksPerMultiprocessor(
                             &per, mlp2_pst_kernel<K_IN, 10, KC, true, 1, false, true>, NT, 0))
      : nshare > 1 ? hipOccupancyMaxActiveBlocksPerMultiprocessor(&per, mlp2_pst_kernel<K_IN, 10, KC, true, 4>, NT, 0)
      : nshare == 1 ? hipOccupancyMaxActiveBlocksPerMultiprocessor(&per, mlp2_pst_kernel<K_IN, 10, KC, true>, NT, 0)
                    : hipOccupancyMaxActiveBlocksPerMultiprocessor(&per, mlp2_pst_kernel<K_IN, 10, KC>, NT, 0);
  if (e != hipSuccess) return 0;
  return (long)(nshare > 0 ? nshare : 1) * G <= (long)cus * per ? 1 : 0;
}

JDT_API int jdt_mlp2_pst_ok(int M, int H, int k_in) {
  if (k_in == 784) return mlp2_pst_ok_k<784>(M, H, 0);
  if (k_in == 1024) return mlp2_pst_ok_k<1024>(M, H, 0);
  return 0;
}
// the persistent launch with the tile exchange (N > 1 DP; fx: the FSDP owner exchange),
// `nshare` ranks per GPU
JDT_API int jdt_mlp2_pst_tx_ok(int M, int H, int k_in, int nshare, int fx) {
  if (nshare < 1) return 0;
  if (k_in == 784) return mlp2_pst_ok_k<784>(M, H, nshare, fx != 0);
  if (k_in == 1024) return mlp2_pst_ok_k<1024>(M, H, nshare, fx != 0);
  return 0;
}

// n >= 2 run-ahead steps in one persistent launch (mlp2_pst_kernel); ws: >= 18 x 32 words,
// zeroed once, never reset (monotonic barrier counters).  -3 outside the run-ahead's
// argument envelope (the caller then launches the one-step kernel n times).  n = 0: a
// launch that returns at once -- done once before any timed or captured use, so the
// kernel's first-dispatch setup (its private segment, ~100 us) is not paid inside one
// (bench.py's 20-step driver form measured 51.6k steps/s without it).
// ranks sharing this GPU (jdt_mlp2_pst_set_share): > 1 selects the two-workgroups-per-CU
// build of the exchanging persistent kernel
static int g_pst_share = 1;
JDT_API void jdt_mlp2_pst_set_share(int n) { g_pst_share = n < 1 ? 1 : n; }
// between-step synchronisation of the persistent launch: 0 = XCD-hierarchical grid barrier,
// 1 = column-block completion counters (CBW); ws then needs 32 * (18 + H/16) words
static int g_pst_cbw = 0;
JDT_API void jdt_mlp2_pst_set_cbw(int on) { g_pst_cbw = on ? 1 : 0; }
JDT_API int jdt_mlp2_pst(const Mlp2Args* args, int n, int k_in, unsigned* ws, long long timeout, void* stream) {
  const long long tmo = timeout > 0 ? timeout : 2000000ll;   // s_memrealtime ticks (100 MHz): 20 ms
  const Mlp2Args& a = *args;
  if (n == 1 || n < 0 || !ws || (a.tx_fsdp && !a.tx) || !a.fuse_opt || !a.W1T || !a.XR || !a.zslab || !a.ztick || !a.hand ||
      !a.lg3 || a.M <= 0 || a.M > 128 || a.H % 128 || (a.tx && !a.running))
    return -3;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const bool tx = a.tx != nullptr;
  if (tx && a.tx_fsdp) {   // FSDP owner exchange (mlp2_bwd_body FX)
    if (k_in == 784) {
      const dim3 g(a.H / 16, 784 / mlp2_kc<784>());
      if (g_pst_share > 1)
        hipLaunchKernelGGL((mlp2_pst_kernel<784, 10, mlp2_kc<784>(), true, 4, false, true>), g, dim3(NT), 0, st, a, n,
                           ws, tmo);
      else
        hipLaunchKernelGGL((mlp2_pst_kernel<784, 10, mlp2_kc<784>(), true, 1, false, true>), g, dim3(NT), 0, st, a, n,
                           ws, tmo);
    } else if (k_in == 1024) {
      const dim3 g(a.H / 16, 1024 / mlp2_kc<1024>());
      if (g_pst_share > 1)
        hipLaunchKernelGGL((mlp2_pst_kernel<1024, 10, mlp2_kc<1024>(), true, 4, false, true>), g, dim3(NT), 0, st, a,
                           n, ws, tmo);
      else
        hipLaunchKernelGGL((mlp2_pst_kernel<1024, 10, mlp2_kc<1024>(), true, 1, false, true>), g, dim3(NT), 0, st, a,
                           n, ws, tmo);
    } else {
      return -3;
    }
    return HIP_LAUNCH_CHECK();
  }
  if (k_in == 784 && g_pst_cbw && !tx) {
    const dim3 g(a.H / 16, 784 / mlp2_kc<784>());
    hipLaunchKernelGGL((mlp2_pst_kernel<784, 10, mlp2_kc<784>(), false, 1, true>), g, dim3(NT), 0, st, a, n, ws, tmo);
  } else if (k_in == 784) {
    const dim3 g(a.H / 16, 784 / mlp2_kc<784>());
    if (tx && g_pst_share > 1)
      hipLaunchKernelGGL((mlp2_pst_kernel<784, 10, mlp2_kc<784>(), true, 4>), g, dim3(NT), 0, st, a, n, ws, tmo);
    else if (tx) hipLaunchKernelGGL((mlp2_pst_kernel<784, 10, mlp2_kc<784>(), true>), g, dim3(NT), 0, st, a, n, ws, tmo);
    else hipLaunchKernelGGL((mlp2_pst_kernel<784, 10, mlp2_kc<784>()>), g, dim3(NT), 0, st, a, n, ws, tmo);
  } else if (k_in == 1024) {
    const dim3 g(a.H / 16, 1024 / mlp2_kc<1024>());
    if (tx && g_pst_share > 1)
      hipLaunchKernelGGL((mlp2_pst_kernel<1024, 10, mlp2_kc<1024>(), true, 4>), g, dim3(NT), 0, st, a, n, ws, tmo);
    else if (tx) hipLaunchKernelGGL((mlp2_pst_kernel<1024, 10, mlp2_kc<1024>(), true>), g, dim3(NT), 0, st, a, n, ws, tmo);
    else hipLaunchKernelGGL((mlp2_pst_kernel<1024, 10, mlp2_kc<1024>()>), g, dim3(NT), 0, st, a, n, ws, tmo);
  } else {
    return -3;
  }
  return HIP_LAUNCH_CHECK();
}

// input widths the fused classifier kernels are instantiated for
static bool mlp2_width_ok(int k_in) { return k_in == 784 || k_in == 1024; }

JDT_API int jdt_mlp2_ahead_ok(int M, int H, int k_in) {
  if (k_in == 784) return mlp2_ahead_ok_k<784>(M, H, 1, false);
  if (k_in == 1024) return mlp2_ahead_ok_k<1024>(M, H, 1, false);
  return 0;
}

// 1 if the N > 1 run-ahead backward (tile exchange, Mlp2Args::tx) can run here with
// `nshare` ranks' grids on this GPU (1 = a GPU per rank): every workgroup of every
// sharing rank's launch must be resident at once -- a tile waits for the same tile of
// the other ranks' launches, and a column block for its own workgroups.
JDT_API int jdt_mlp2_ahead_tx_ok(int M, int H, int k_in, int nshare) {
  if (!jdt_mlp2_ahead_ok(M, H, k_in)) return 0;
  if (k_in == 784) return mlp2_ahead_ok_k<784>(M, H, nshare, true);
  return mlp2_ahead_ok_k<1024>(M, H, nshare, true);
}

// input chunk (rows of W1 per backward workgroup) for an input width, 0 if unsupported
JDT_API int jdt_mlp2_chunk(int k_in) {
  if (k_in == 784) return mlp2_kc<784>();
  if (k_in == 1024) return mlp2_kc<1024>();
  return 0;
}

// The tile exchange's self-test (above): `tiles` workgroups, epoch `epoch`; words[0] gets
// the number of wrong results, words[1] the timeout bits.  The caller resets the flags
// afterwards (jdt_tx_reset) before the step kernels use epochs from 1.
JDT_API int jdt_tx_selftest(const void* tx_args_dev, int tiles, unsigned epoch, unsigned* words, void* stream) {
  if (!tx_args_dev || tiles <= 0) return -2;
  hipLaunchKernelGGL(tx_selftest_kernel, dim3(tiles), dim3(NT), 0, static_cast<hipStream_t>(stream),
                     static_cast<const TxArgs*>(tx_args_dev), epoch, words, words + 1);
  return HIP_LAUNCH_CHECK();
}

// A/B switch (JDT_MLP2_P3S=1): the one-GPU run-ahead backward compiled with the N > 1
// kernel's phase-3 structure (all MFMAs, then all epilogues) instead of its own
static int g_mlp2_p3s = 0;
JDT_API void jdt_mlp2_set_p3s(int on) { g_mlp2_p3s = on; }

// phase 0: mlp2_fwd, 1: mlp2_bwd, 2: run-ahead mlp2_bwd (backward of t + forward of t+1)
template <int K_IN>
static int mlp2_launch(const Mlp2Args& a, int phase, hipStream_t st) {
  constexpr int KC = mlp2_kc<K_IN>(), NCH = K_IN / KC;
  // the forward's X^T / X side outputs: hidden block y < NCH writes input chunk y
  if (a.H / 16 < NCH) return -3;
  if (phase == 0) {
    const bool direct = a.W1T != nullptr;
    const bool xf = xcd_tiles_enabled() == 1;
    if (g_mlp2_rb == 32) {
      const dim3 g((a.M + 31) / 32, a.H / 16);
      if (direct && xf) hipLaunchKernelGGL((mlp2_fwd_kernel<K_IN, 10, 32, true, true>), g, dim3(NT), 0, st, a);
      else if (direct) hipLaunchKernelGGL((mlp2_fwd_kernel<K_IN, 10, 32, true, false>), g, dim3(NT), 0, st, a);
      else hipLaunchKernelGGL((mlp2_fwd_kernel<K_IN, 10, 32, false, false>), g, dim3(NT), 0, st, a);
    } else {
      const dim3 g((a.M + 15) / 16, a.H / 16);
      if (direct && xf) hipLaunchKernelGGL((mlp2_fwd_kernel<K_IN, 10, 16, true, true>), g, dim3(NT), 0, st, a);
      else if (direct) hipLaunchKernelGGL((mlp2_fwd_kernel<K_IN, 10, 16, true, false>), g, dim3(NT), 0, st, a);
      else hipLaunchKernelGGL((mlp2_fwd_kernel<K_IN, 10, 16, false, false>), g, dim3(NT), 0, st, a);
    }
  } else if (phase == 1) {
    const dim3 g(a.H / 16, NCH);
    if (xcd_tiles_enabled()) hipLaunchKernelGGL((mlp2_bwd_kernel<K_IN, 10, KC, true>), g, dim3(NT), 0, st, a);
    else hipLaunchKernelGGL((mlp2_bwd_kernel<K_IN, 10, KC, false>), g, dim3(NT), 0, st, a);
  } else {
    // run-ahead backward: step t's backward + AdamW + step t+1's forward (needs the
    // fused optimizer, the W1^T copy, the X copy written by mlp2_fwd and lg3 logits)
    if (!a.fuse_opt || !a.W1T || !a.XR || !a.zslab || !a.ztick || !a.hand || !a.lg3 || a.M > 128 || a.H % 128)
      return -3;
    const dim3 g(a.H / 16, NCH);
    if (a.tx && a.tx_fsdp)
      hipLaunchKernelGGL((mlp2_bwd_kernel<K_IN, 10, KC, true, true, true, false, true>), g, dim3(NT), 0, st, a);
    else if (a.tx) hipLaunchKernelGGL((mlp2_bwd_kernel<K_IN, 10, KC, true, true, true>), g, dim3(NT), 0, st, a);
    else if (g_mlp2_p3s) hipLaunchKernelGGL((mlp2_bwd_kernel<K_IN, 10, KC, true, true, false, true>), g, dim3(NT), 0, st, a);
    else hipLaunchKernelGGL((mlp2_bwd_kernel<K_IN, 10, KC, true, true>), g, dim3(NT), 0, st, a);
  }
  return HIP_LAUNCH_CHECK();
}

JDT_API int jdt_mlp2(const Mlp2Args* args, int phase, int k_in, int c, void* stream) {
  const Mlp2Args& a = *args;
  if (!mlp2_width_ok(k_in) || c != 10 || a.H % 16 || a.M <= 0 || a.M > 128) return -3;
  hipStream_t st = static_cast<hipStream_t>(stream);
  return k_in == 784 ? mlp2_launch<784>(a, phase, st) : mlp2_launch<1024>(a, phase, st);
}
