// Host-side AddressSanitizer check of the kernel library's extern "C" entry points
// (SURVEY §5.2 "optional ASan builds of the C++ extension (host side)").
//
// Built by `python -m jax_distributed_tuts_amd.ops.build --asan-check`: every
// csrc/*.hip object is recompiled with `-Xarch_host -fsanitize=address` (device
// code unchanged -- GPU sanitizers are not used on this pool), linked with this
// driver and run on the CPU.  It exercises the host code that needs no GPU: the
// argument validation of every launcher (each rejects before touching the
// device), the struct-layout probes the ctypes mirrors check, the grouped-GEMM
// planner's early exits and the collectives' rank/world checks.  ASan aborts the
// run on any out-of-bounds / use-after-free in that code.
#include <cstdio>
#include <cstring>
#include <vector>

extern "C" {
int jdt_gemm_args_size();
int jdt_mlp2_args_size();
int jdt_md_args_size();
int jdt_xgmi_adam_size();
int jdt_xgmi_segs_size();
int jdt_gemm(const void* ga, int batch, int cfg, int splits, float* ws, long ws_floats, unsigned* counters,
             long n_counters, void* stream);
int jdt_gemm_group(const void* gs, int n, float* ws, long ws_floats, unsigned* counters, long n_counters,
                   void* stream);
int jdt_mlp2(const void* args, int phase, int k_in, int c, void* stream);
int jdt_md_layer(const void* args, int phase, int head, void* stream);
int jdt_xgmi_create(int rank, int world, long cap_floats, void** ctx_out, void* handles_out);
int jdt_p2p_create(int rank, int world, long slot_bytes, int n_slots, void** ctx_out, void* handles_out);
int jdt_adamw(float* p, float* g, float* m, float* v, void* shadow, long n, float lr, float b1, float b2, float eps,
              float wd, float grad_scale, int* step, unsigned* ticket, int zero_grad, void* stream);
int jdt_sgd(float* p, float* g, float* buf, void* shadow, long n, float lr, float momentum, float wd,
            float grad_scale, int* step, unsigned* ticket, int zero_grad, void* stream);
int jdt_colsum(const void* x, long ld, int M, int N, float* out, void* stream);
int jdt_attn_decode(const void* qkv, void* k_cache, void* v_cache, void* o, const int* pos, int B, int H, int Dh,
                    int S_max, float scale, void* stream);
int jdt_embed_decode(const int* tokens, const void* wte, const void* wpe, void* out, const int* pos, int B, int S_max,
                     int d, int vocab, void* stream);
int jdt_sample(const void* logits, long ld, int B, int V, float temperature, unsigned long long seed,
               unsigned stream_id, int* tokens, int S_max, int* pos, unsigned* ticket, void* stream);
int jdt_attn_decode_rows(const void* qkv, void* k_cache, void* v_cache, void* o, const int* pos, int B, int H, int Dh,
                         int S_max, float scale, void* stream);
int jdt_attn_decode_long(const void* qkv, void* k_cache, void* v_cache, void* o, const int* pos, float* ws,
                         long ws_floats, int B, int H, int Dh, int S_max, float scale, void* stream);
int jdt_attn_decode_long_rows(const void* qkv, void* k_cache, void* v_cache, void* o, const int* pos, float* ws,
                              long ws_floats, int B, int H, int Dh, int S_max, float scale, void* stream);
int jdt_embed_decode_rows(const int* tokens, const void* wte, const void* wpe, void* out, const int* pos, int B,
                          int S_max, int d, int vocab, void* stream);
int jdt_sample_filtered(const void* logits, long ld, int B, int V, float temperature, unsigned long long seed,
                        unsigned stream_id, int* tokens, int S_max, int* pos, unsigned* ticket, int top_k, float top_p,
                        void* stream);
int jdt_sample_rows(const void* logits, long ld, int B, int V, float temperature, unsigned long long seed,
                    unsigned stream_id, int* tokens, int S_max, int* pos, int* end, int eos_id, int top_k, float top_p,
                    void* stream);
int jdt_attn_append(const void* qkv, void* k_cache, void* v_cache, void* o, const int* pos, int B, int C, int H, int Dh,
                    int S_max, float scale, void* stream);
int jdt_attn_append_rows(const void* qkv, void* k_cache, void* v_cache, void* o, const int* pos, const int* count,
                         int B, int C, int H, int Dh, int S_max, float scale, void* stream);
int jdt_attn_append_split(const void* qkv, void* k_cache, void* v_cache, void* o, const int* pos, float* ws,
                          long ws_floats, int B, int C, int H, int Dh, int S_max, float scale, void* stream);
int jdt_attn_append_split_rows(const void* qkv, void* k_cache, void* v_cache, void* o, const int* pos,
                               const int* count, float* ws, long ws_floats, int B, int C, int H, int Dh, int S_max,
                               float scale, void* stream);
int jdt_embed_append(const int* tokens, const void* wte, const void* wpe, void* out, const int* pos, int B, int C,
                     int S_max, int d, int vocab, void* stream);
int jdt_embed_append_rows(const int* tokens, const void* wte, const void* wpe, void* out, const int* pos,
                          const int* count, int B, int C, int S_max, int d, int vocab, void* stream);
int jdt_attn_decode_fp8(const void* qkv, void* k_cache, void* v_cache, float* k_scale, float* v_scale, void* o,
                        const int* pos, int B, int H, int Dh, int S_max, float scale, void* stream);
int jdt_attn_decode_fp8_rows(const void* qkv, void* k_cache, void* v_cache, float* k_scale, float* v_scale, void* o,
                             const int* pos, int B, int H, int Dh, int S_max, float scale, void* stream);
int jdt_attn_decode_fp8_long(const void* qkv, void* k_cache, void* v_cache, float* k_scale, float* v_scale, void* o,
                             const int* pos, float* ws, long ws_floats, int B, int H, int Dh, int S_max, float scale,
                             void* stream);
int jdt_attn_decode_fp8_long_rows(const void* qkv, void* k_cache, void* v_cache, float* k_scale, float* v_scale,
                                  void* o, const int* pos, float* ws, long ws_floats, int B, int H, int Dh, int S_max,
                                  float scale, void* stream);
int jdt_attn_append_fp8(const void* qkv, void* k_cache, void* v_cache, float* k_scale, float* v_scale, void* o,
                        const int* pos, int B, int C, int H, int Dh, int S_max, float scale, void* stream);
int jdt_attn_append_fp8_rows(const void* qkv, void* k_cache, void* v_cache, float* k_scale, float* v_scale, void* o,
                             const int* pos, const int* count, int B, int C, int H, int Dh, int S_max, float scale,
                             void* stream);
int jdt_kv_quantize_rows(const void* qkv, void* k_cache, void* v_cache, float* k_scale, float* v_scale, int B, int H,
                         int Dh, int S_max, int Sp, int n, void* stream);
}

static int failures = 0;
#define EXPECT(cond, what)                                   \
  do {                                                       \
    if (!(cond)) {                                           \
      std::fprintf(stderr, "FAIL: %s\n", what);              \
      ++failures;                                            \
    }                                                        \
  } while (0)

int main() {
  // layout probes (the Python ctypes mirrors compare against these)
  EXPECT(jdt_gemm_args_size() > 0 && jdt_mlp2_args_size() > 0 && jdt_md_args_size() > 0, "struct sizes");
  EXPECT(jdt_xgmi_adam_size() > 0 && jdt_xgmi_segs_size() > 0, "xgmi struct sizes");

  // every launcher rejects bad arguments on the host, before any device call
  std::vector<unsigned char> gemm(jdt_gemm_args_size(), 0);
  EXPECT(jdt_gemm(gemm.data(), 1, -1, -1, nullptr, 0, nullptr, 0, nullptr) == 0, "gemm M = N = 0 is a no-op");
  EXPECT(jdt_gemm_group(gemm.data(), 0, nullptr, 0, nullptr, 0, nullptr) == 1, "empty group declined");
  std::vector<unsigned char> mlp2(jdt_mlp2_args_size(), 0);
  EXPECT(jdt_mlp2(mlp2.data(), 0, 784, 10, nullptr) == -3, "mlp2 rejects M = 0");
  EXPECT(jdt_mlp2(mlp2.data(), 0, 100, 10, nullptr) == -3, "mlp2 rejects an input width it is not built for");
  std::vector<unsigned char> md(jdt_md_args_size(), 0);
  EXPECT(jdt_md_layer(md.data(), 0, 0, nullptr) == -3, "md rejects N != 512");
  void* ctx = nullptr;
  unsigned char handles[3 * 64];
  EXPECT(jdt_xgmi_create(0, 1, 1024, &ctx, handles) == -4 && ctx == nullptr, "xgmi rejects world 1");
  EXPECT(jdt_xgmi_create(3, 2, 1024, &ctx, handles) == -4, "xgmi rejects rank >= world");
  EXPECT(jdt_xgmi_create(0, 9, 1024, &ctx, handles) == -4, "xgmi rejects world > 8");
  EXPECT(jdt_p2p_create(0, 1, 4096, 2, &ctx, handles) == -4, "p2p rejects world 1");
  EXPECT(jdt_p2p_create(0, 2, 4096, 0, &ctx, handles) == -2, "p2p rejects 0 slots");
  EXPECT(jdt_p2p_create(0, 2, 0, 2, &ctx, handles) == -2, "p2p rejects empty slots");
  EXPECT(jdt_adamw(nullptr, nullptr, nullptr, nullptr, nullptr, 0, 1e-3f, .9f, .999f, 1e-8f, 0.f, 1.f, nullptr,
                   nullptr, 1, nullptr) == 0, "adamw n = 0 is a no-op");
  float* mis = reinterpret_cast<float*>(reinterpret_cast<char*>(handles) + 4);  // misaligned
  EXPECT(jdt_adamw(mis, mis, mis, mis, nullptr, 16, 1e-3f, .9f, .999f, 1e-8f, 0.f, 1.f, nullptr, nullptr, 1,
                   nullptr) == -2, "adamw rejects misaligned buffers");
  EXPECT(jdt_sgd(nullptr, nullptr, nullptr, nullptr, 0, .1f, 0.f, 0.f, 1.f, nullptr, nullptr, 1, nullptr) == 0,
         "sgd n = 0 is a no-op");
  EXPECT(jdt_colsum(handles, 7, 4, 7, nullptr, nullptr) == -3, "colsum rejects N % 8");
  // decode launchers (attn_decode.hip): the envelope is checked before anything is launched
  alignas(16) unsigned char buf[64];
  int* ip = reinterpret_cast<int*>(buf);
  unsigned* up = reinterpret_cast<unsigned*>(buf);
  EXPECT(jdt_attn_decode(buf, buf, buf, buf, ip, 1, 2, 32, 128, .125f, nullptr) == -3, "attn_decode rejects head dim 32");
  EXPECT(jdt_attn_decode(buf, buf, buf, buf, ip, 1, 2, 64, 129, .125f, nullptr) == -4, "attn_decode rejects S_max > 128");
  EXPECT(jdt_attn_decode(buf, buf, buf, buf, ip, 1, 2, 64, 0, .125f, nullptr) == -4, "attn_decode rejects S_max 0");
  EXPECT(jdt_attn_decode(buf, nullptr, buf, buf, ip, 1, 2, 64, 128, .125f, nullptr) == -2, "attn_decode rejects null");
  EXPECT(jdt_attn_decode(buf + 4, buf, buf, buf, ip, 1, 2, 64, 128, .125f, nullptr) == -6,
         "attn_decode rejects a misaligned qkv");
  EXPECT(jdt_attn_decode(buf, buf, buf, buf, ip, 0, 2, 64, 128, .125f, nullptr) == 0, "attn_decode B = 0 is a no-op");
  EXPECT(jdt_embed_decode(ip, buf, buf, buf, ip, 1, 128, 60, 8, nullptr) == -3, "embed_decode rejects d % 8");
  EXPECT(jdt_embed_decode(ip, buf, buf, buf, ip, 0, 128, 64, 8, nullptr) == 0, "embed_decode B = 0 is a no-op");
  EXPECT(jdt_sample(buf, 8, 1, 0, 0.f, 0, 0, ip, 128, ip, up, nullptr) == -5, "sample rejects V = 0");
  EXPECT(jdt_sample(buf, 8, 1, 8, -1.f, 0, 0, ip, 128, ip, up, nullptr) == -7, "sample rejects temperature < 0");
  EXPECT(jdt_sample(buf, 8, 1, 8, 1.f, 0, 0, ip, 128, ip, nullptr, nullptr) == -2, "sample rejects a null ticket");
  EXPECT(jdt_sample(buf, 8, 0, 8, 1.f, 0, 0, ip, 128, ip, up, nullptr) == 0, "sample B = 0 is a no-op");
  // per-row and filtered variants: the same envelope, plus top_k / top_p
  EXPECT(jdt_attn_decode_rows(buf, buf, buf, buf, ip, 1, 2, 32, 128, .125f, nullptr) == -3,
         "attn_decode_rows rejects head dim 32");
  EXPECT(jdt_attn_decode_rows(buf, buf, buf, buf, ip, 1, 2, 64, 129, .125f, nullptr) == -4,
         "attn_decode_rows rejects S_max > 128");
  EXPECT(jdt_attn_decode_rows(buf, buf, buf, buf, ip, 1, 2, 64, 0, .125f, nullptr) == -4,
         "attn_decode_rows rejects S_max 0");
  EXPECT(jdt_attn_decode_rows(buf, buf, buf, buf, nullptr, 1, 2, 64, 128, .125f, nullptr) == -2,
         "attn_decode_rows rejects a null pos");
  EXPECT(jdt_attn_decode_rows(buf, buf, buf, buf, ip, 0, 2, 64, 128, .125f, nullptr) == 0,
         "attn_decode_rows B = 0 is a no-op");
  EXPECT(jdt_embed_decode_rows(ip, buf, buf, buf, nullptr, 1, 128, 64, 8, nullptr) == -2,
         "embed_decode_rows rejects a null pos");
  EXPECT(jdt_embed_decode_rows(ip, buf, buf, buf, ip, 1, 0, 64, 8, nullptr) == -5, "embed_decode_rows rejects S_max 0");
  EXPECT(jdt_embed_decode_rows(ip, buf, buf, buf, ip, 0, 128, 64, 8, nullptr) == 0,
         "embed_decode_rows B = 0 is a no-op");
  EXPECT(jdt_sample_filtered(buf, 8, 1, 8, 1.f, 0, 0, ip, 128, ip, up, -1, 1.f, nullptr) == -8,
         "sample_filtered rejects top_k < 0");
  EXPECT(jdt_sample_filtered(buf, 8, 1, 8, 1.f, 0, 0, ip, 128, ip, up, 0, 0.f, nullptr) == -9,
         "sample_filtered rejects top_p = 0");
  EXPECT(jdt_sample_filtered(buf, 8, 1, 8, 1.f, 0, 0, ip, 128, ip, up, 0, 1.5f, nullptr) == -9,
         "sample_filtered rejects top_p > 1");
  EXPECT(jdt_sample_filtered(buf, 8, 1, 8, 1.f, 0, 0, ip, 0, ip, up, 3, .9f, nullptr) == -5,
         "sample_filtered rejects S_max 0");
  EXPECT(jdt_sample_filtered(buf, 8, 1, 8, 1.f, 0, 0, ip, 128, ip, nullptr, 3, .9f, nullptr) == -2,
         "sample_filtered rejects a null ticket");
  EXPECT(jdt_sample_filtered(buf, 8, 0, 8, 1.f, 0, 0, ip, 128, ip, up, 3, .9f, nullptr) == 0,
         "sample_filtered B = 0 is a no-op");
  EXPECT(jdt_sample_rows(buf, 8, 1, 8, 1.f, 0, 0, ip, 128, ip, ip, -1, -1, 1.f, nullptr) == -8,
         "sample_rows rejects top_k < 0");
  EXPECT(jdt_sample_rows(buf, 8, 1, 8, 1.f, 0, 0, ip, 128, ip, ip, -1, 0, 0.f, nullptr) == -9,
         "sample_rows rejects top_p = 0");
  EXPECT(jdt_sample_rows(buf, 8, 1, 8, 1.f, 0, 0, ip, 128, ip, ip, -1, 0, 1.5f, nullptr) == -9,
         "sample_rows rejects top_p > 1");
  EXPECT(jdt_sample_rows(buf, 8, 1, 8, 1.f, 0, 0, ip, 0, ip, ip, -1, 0, 1.f, nullptr) == -5,
         "sample_rows rejects S_max 0");
  EXPECT(jdt_sample_rows(buf, 8, 1, 8, 1.f, 0, 0, ip, 128, ip, nullptr, -1, 0, 1.f, nullptr) == -2,
         "sample_rows rejects a null end");
  EXPECT(jdt_sample_rows(buf, 8, 1, 8, 1.f, 0, 0, ip, 128, nullptr, ip, -1, 0, 1.f, nullptr) == -2,
         "sample_rows rejects a null pos");
  EXPECT(jdt_sample_rows(buf, 8, 0, 8, 1.f, 0, 0, ip, 128, ip, ip, 3, 50, .9f, nullptr) == 0,
         "sample_rows B = 0 is a no-op");
  // split-KV launchers: the same envelope up to 32768 rows, plus the workspace (1 x 2 x 3 chunks x 66 floats)
  float* fp = reinterpret_cast<float*>(buf);
  EXPECT(jdt_attn_decode_long(buf, buf, buf, buf, ip, fp, 396, 1, 2, 32, 320, .125f, nullptr) == -3,
         "attn_decode_long rejects head dim 32");
  EXPECT(jdt_attn_decode_long(buf, buf, buf, buf, ip, fp, 396, 1, 2, 64, 0, .125f, nullptr) == -4,
         "attn_decode_long rejects S_max 0");
  EXPECT(jdt_attn_decode_long(buf, buf, buf, buf, ip, fp, 1L << 30, 1, 2, 64, 32769, .125f, nullptr) == -4,
         "attn_decode_long rejects S_max 32769");
  EXPECT(jdt_attn_decode_long(buf, buf, buf, buf, ip, nullptr, 396, 1, 2, 64, 320, .125f, nullptr) == -2,
         "attn_decode_long rejects a null ws");
  EXPECT(jdt_attn_decode_long(buf, buf, buf, buf, ip, fp, 395, 1, 2, 64, 320, .125f, nullptr) == -10,
         "attn_decode_long rejects a short ws");
  EXPECT(jdt_attn_decode_long(buf, buf, buf, buf, ip, fp, 0, 0, 2, 64, 320, .125f, nullptr) == 0,
         "attn_decode_long B = 0 is a no-op");
  EXPECT(jdt_attn_decode_long_rows(buf, buf, buf, buf, ip, fp, 396, 1, 2, 32, 320, .125f, nullptr) == -3,
         "attn_decode_long_rows rejects head dim 32");
  EXPECT(jdt_attn_decode_long_rows(buf, buf, buf, buf, ip, fp, 396, 1, 2, 64, 0, .125f, nullptr) == -4,
         "attn_decode_long_rows rejects S_max 0");
  EXPECT(jdt_attn_decode_long_rows(buf, buf, buf, buf, ip, fp, 1L << 30, 1, 2, 64, 32769, .125f, nullptr) == -4,
         "attn_decode_long_rows rejects S_max 32769");
  EXPECT(jdt_attn_decode_long_rows(buf, buf, buf, buf, ip, nullptr, 396, 1, 2, 64, 320, .125f, nullptr) == -2,
         "attn_decode_long_rows rejects a null ws");
  EXPECT(jdt_attn_decode_long_rows(buf, buf, buf, buf, ip, fp, 395, 1, 2, 64, 320, .125f, nullptr) == -10,
         "attn_decode_long_rows rejects a short ws");
  EXPECT(jdt_attn_decode_long_rows(buf, buf, buf, buf, ip, fp, 0, 0, 2, 64, 320, .125f, nullptr) == 0,
         "attn_decode_long_rows B = 0 is a no-op");
  // append launchers (attn_append.hip, embed_append): Dh = 64, S_max in 1..32768, C in 1..1024
  EXPECT(jdt_attn_append(buf, buf, buf, buf, ip, 1, 64, 2, 32, 320, .125f, nullptr) == -3,
         "attn_append rejects head dim 32");
  EXPECT(jdt_attn_append(buf, buf, buf, buf, ip, 1, 64, 2, 64, 0, .125f, nullptr) == -4, "attn_append rejects S_max 0");
  EXPECT(jdt_attn_append(buf, buf, buf, buf, ip, 1, 64, 2, 64, 32769, .125f, nullptr) == -4,
         "attn_append rejects S_max 32769");
  EXPECT(jdt_attn_append(buf, buf, buf, buf, ip, 1, 0, 2, 64, 320, .125f, nullptr) == -11, "attn_append rejects C 0");
  EXPECT(jdt_attn_append(buf, buf, buf, buf, ip, 1, 1025, 2, 64, 320, .125f, nullptr) == -11,
         "attn_append rejects C 1025");
  EXPECT(jdt_attn_append(buf, buf, nullptr, buf, ip, 1, 64, 2, 64, 320, .125f, nullptr) == -2,
         "attn_append rejects null");
  EXPECT(jdt_attn_append(buf, buf + 4, buf, buf, ip, 1, 64, 2, 64, 320, .125f, nullptr) == -6,
         "attn_append rejects a misaligned cache");
  EXPECT(jdt_attn_append(buf, buf, buf, buf, ip, 65536, 64, 1, 64, 320, .125f, nullptr) == -5,
         "attn_append rejects B * H past the grid");
  EXPECT(jdt_attn_append(buf, buf, buf, buf, ip, 0, 64, 2, 64, 320, .125f, nullptr) == 0, "attn_append B = 0 is a no-op");
  EXPECT(jdt_attn_append_rows(buf, buf, buf, buf, ip, ip, 1, 64, 2, 128, 320, .125f, nullptr) == -3,
         "attn_append_rows rejects head dim 128");
  EXPECT(jdt_attn_append_rows(buf, buf, buf, buf, ip, ip, 1, 64, 2, 64, 32769, .125f, nullptr) == -4,
         "attn_append_rows rejects S_max 32769");
  EXPECT(jdt_attn_append_rows(buf, buf, buf, buf, ip, ip, 1, 1025, 2, 64, 320, .125f, nullptr) == -11,
         "attn_append_rows rejects C 1025");
  EXPECT(jdt_attn_append_rows(buf, buf, buf, buf, ip, nullptr, 1, 64, 2, 64, 320, .125f, nullptr) == -2,
         "attn_append_rows rejects a null count");
  EXPECT(jdt_attn_append_rows(buf, buf, buf, buf, nullptr, ip, 1, 64, 2, 64, 320, .125f, nullptr) == -2,
         "attn_append_rows rejects a null pos");
  EXPECT(jdt_attn_append_rows(buf + 4, buf, buf, buf, ip, ip, 1, 64, 2, 64, 320, .125f, nullptr) == -6,
         "attn_append_rows rejects a misaligned qkv");
  EXPECT(jdt_attn_append_rows(buf, buf, buf, buf, ip, ip, 0, 64, 2, 64, 320, .125f, nullptr) == 0,
         "attn_append_rows B = 0 is a no-op");
  // split-KV append launchers: the same envelope, plus the workspace (1 x 2 x 1 query tile x 1 span x 64 x 66 floats)
  const long big = 1L << 40;   // a workspace size no shape here exceeds
  EXPECT(jdt_attn_append_split(buf, buf, buf, buf, ip, fp, 8448, 1, 64, 2, 32, 320, .125f, nullptr) == -3,
         "attn_append_split rejects head dim 32");
  EXPECT(jdt_attn_append_split(buf, buf, buf, buf, ip, fp, 8448, 1, 64, 2, 64, 0, .125f, nullptr) == -4,
         "attn_append_split rejects S_max 0");
  EXPECT(jdt_attn_append_split(buf, buf, buf, buf, ip, fp, big, 1, 64, 2, 64, 32769, .125f, nullptr) == -4,
         "attn_append_split rejects S_max 32769");
  EXPECT(jdt_attn_append_split(buf, buf, buf, buf, ip, fp, 8448, 1, 0, 2, 64, 320, .125f, nullptr) == -11,
         "attn_append_split rejects C 0");
  EXPECT(jdt_attn_append_split(buf, buf, buf, buf, ip, fp, big, 1, 1025, 2, 64, 320, .125f, nullptr) == -11,
         "attn_append_split rejects C 1025");
  EXPECT(jdt_attn_append_split(buf, buf, nullptr, buf, ip, fp, 8448, 1, 64, 2, 64, 320, .125f, nullptr) == -2,
         "attn_append_split rejects null");
  EXPECT(jdt_attn_append_split(buf, buf, buf, buf, ip, nullptr, 8448, 1, 64, 2, 64, 320, .125f, nullptr) == -2,
         "attn_append_split rejects a null ws");
  EXPECT(jdt_attn_append_split(buf, buf + 4, buf, buf, ip, fp, 8448, 1, 64, 2, 64, 320, .125f, nullptr) == -6,
         "attn_append_split rejects a misaligned cache");
  EXPECT(jdt_attn_append_split(buf, buf, buf, buf, ip, fp, big, 65536, 64, 1, 64, 320, .125f, nullptr) == -5,
         "attn_append_split rejects B * H past the grid");
  EXPECT(jdt_attn_append_split(buf, buf, buf, buf, ip, fp, 8447, 1, 64, 2, 64, 320, .125f, nullptr) == -10,
         "attn_append_split rejects a short ws");
  EXPECT(jdt_attn_append_split(buf, buf, buf, buf, ip, fp, 2 * 8448 - 1, 1, 65, 2, 64, 320, .125f, nullptr) == -10,
         "attn_append_split rejects a ws short of the second query tile");
  EXPECT(jdt_attn_append_split(buf, buf, buf, buf, ip, fp, 2 * 8448 - 1, 1, 64, 2, 64, 513, .125f, nullptr) == -10,
         "attn_append_split rejects a ws short of the second span");
  EXPECT(jdt_attn_append_split(buf, buf, buf, buf, ip, fp, 0, 0, 64, 2, 64, 320, .125f, nullptr) == 0,
         "attn_append_split B = 0 is a no-op");
  EXPECT(jdt_attn_append_split_rows(buf, buf, buf, buf, ip, ip, fp, 8448, 1, 64, 2, 128, 320, .125f, nullptr) == -3,
         "attn_append_split_rows rejects head dim 128");
  EXPECT(jdt_attn_append_split_rows(buf, buf, buf, buf, ip, ip, fp, big, 1, 64, 2, 64, 32769, .125f, nullptr) == -4,
         "attn_append_split_rows rejects S_max 32769");
  EXPECT(jdt_attn_append_split_rows(buf, buf, buf, buf, ip, ip, fp, big, 1, 1025, 2, 64, 320, .125f, nullptr) == -11,
         "attn_append_split_rows rejects C 1025");
  EXPECT(jdt_attn_append_split_rows(buf, buf, buf, buf, ip, nullptr, fp, 8448, 1, 64, 2, 64, 320, .125f, nullptr) == -2,
         "attn_append_split_rows rejects a null count");
  EXPECT(jdt_attn_append_split_rows(buf, buf, buf, buf, ip, ip, nullptr, 8448, 1, 64, 2, 64, 320, .125f, nullptr) == -2,
         "attn_append_split_rows rejects a null ws");
  EXPECT(jdt_attn_append_split_rows(buf + 4, buf, buf, buf, ip, ip, fp, 8448, 1, 64, 2, 64, 320, .125f, nullptr) == -6,
         "attn_append_split_rows rejects a misaligned qkv");
  EXPECT(jdt_attn_append_split_rows(buf, buf, buf, buf, ip, ip, fp, big, 65536, 64, 1, 64, 320, .125f, nullptr) == -5,
         "attn_append_split_rows rejects B * H past the grid");
  EXPECT(jdt_attn_append_split_rows(buf, buf, buf, buf, ip, ip, fp, 8447, 1, 64, 2, 64, 320, .125f, nullptr) == -10,
         "attn_append_split_rows rejects a short ws");
  EXPECT(jdt_attn_append_split_rows(buf, buf, buf, buf, ip, ip, fp, 0, 0, 64, 2, 64, 320, .125f, nullptr) == 0,
         "attn_append_split_rows B = 0 is a no-op");
  EXPECT(jdt_embed_append(ip, buf, buf, buf, ip, 1, 64, 128, 60, 8, nullptr) == -3, "embed_append rejects d % 8");
  EXPECT(jdt_embed_append(ip, buf, buf, buf, ip, 1, 0, 128, 64, 8, nullptr) == -11, "embed_append rejects C 0");
  EXPECT(jdt_embed_append(ip, buf, buf, buf, ip, 1, 64, 0, 64, 8, nullptr) == -5, "embed_append rejects S_max 0");
  EXPECT(jdt_embed_append(ip, buf, buf, nullptr, ip, 1, 64, 128, 64, 8, nullptr) == -2, "embed_append rejects null");
  EXPECT(jdt_embed_append(ip, buf, buf, buf + 4, ip, 1, 64, 128, 64, 8, nullptr) == -6,
         "embed_append rejects a misaligned out");
  EXPECT(jdt_embed_append(ip, buf, buf, buf, ip, 0, 64, 128, 64, 8, nullptr) == 0, "embed_append B = 0 is a no-op");
  EXPECT(jdt_embed_append_rows(ip, buf, buf, buf, ip, nullptr, 1, 64, 128, 64, 8, nullptr) == -2,
         "embed_append_rows rejects a null count");
  EXPECT(jdt_embed_append_rows(ip, buf, buf, buf, ip, ip, 1, 1025, 128, 64, 8, nullptr) == -11,
         "embed_append_rows rejects C 1025");
  EXPECT(jdt_embed_append_rows(ip, buf, buf, buf, ip, ip, 0, 64, 128, 64, 8, nullptr) == 0,
         "embed_append_rows B = 0 is a no-op");
  // FP8 KV cache launchers: the bf16 envelopes, null scales, 8-byte caches and 4-byte scales
  float* sp = reinterpret_cast<float*>(buf);
  float* sp_mis = reinterpret_cast<float*>(buf + 2);
  EXPECT(jdt_attn_decode_fp8(buf, buf, buf, sp, sp, buf, ip, 1, 2, 32, 128, .125f, nullptr) == -3,
         "attn_decode_fp8 rejects head dim 32");
  EXPECT(jdt_attn_decode_fp8(buf, buf, buf, sp, sp, buf, ip, 1, 2, 64, 129, .125f, nullptr) == -4,
         "attn_decode_fp8 rejects S_max > 128");
  EXPECT(jdt_attn_decode_fp8(buf, buf, buf, nullptr, sp, buf, ip, 1, 2, 64, 128, .125f, nullptr) == -2,
         "attn_decode_fp8 rejects a null k_scale");
  EXPECT(jdt_attn_decode_fp8(buf, buf, buf, sp, nullptr, buf, ip, 1, 2, 64, 128, .125f, nullptr) == -2,
         "attn_decode_fp8 rejects a null v_scale");
  EXPECT(jdt_attn_decode_fp8(buf, buf + 4, buf, sp, sp, buf, ip, 1, 2, 64, 128, .125f, nullptr) == -6,
         "attn_decode_fp8 rejects a cache off an 8-byte boundary");
  EXPECT(jdt_attn_decode_fp8(buf, buf, buf, sp, sp_mis, buf, ip, 1, 2, 64, 128, .125f, nullptr) == -6,
         "attn_decode_fp8 rejects a misaligned scale");
  EXPECT(jdt_attn_decode_fp8(buf, buf, buf, sp, sp, buf, ip, 0, 2, 64, 128, .125f, nullptr) == 0,
         "attn_decode_fp8 B = 0 is a no-op");
  EXPECT(jdt_attn_decode_fp8_rows(buf, buf, buf, sp, sp, buf, nullptr, 1, 2, 64, 128, .125f, nullptr) == -2,
         "attn_decode_fp8_rows rejects null");
  EXPECT(jdt_attn_decode_fp8_rows(buf, buf, buf, sp, sp, buf, ip, 0, 2, 64, 128, .125f, nullptr) == 0,
         "attn_decode_fp8_rows B = 0 is a no-op");
  EXPECT(jdt_attn_decode_fp8_long(buf, buf, buf, sp, sp, buf, ip, fp, 1L << 30, 1, 2, 64, 32769, .125f, nullptr) == -4,
         "attn_decode_fp8_long rejects S_max > 32768");
  EXPECT(jdt_attn_decode_fp8_long(buf, buf, buf, sp, nullptr, buf, ip, fp, 396, 1, 2, 64, 320, .125f, nullptr) == -2,
         "attn_decode_fp8_long rejects a null v_scale");
  EXPECT(jdt_attn_decode_fp8_long(buf, buf, buf, sp, sp, buf, ip, fp, 395, 1, 2, 64, 320, .125f, nullptr) == -10,
         "attn_decode_fp8_long rejects a short ws");
  EXPECT(jdt_attn_decode_fp8_long(buf, buf, buf, sp, sp, buf, ip, fp, 0, 0, 2, 64, 320, .125f, nullptr) == 0,
         "attn_decode_fp8_long B = 0 is a no-op");
  EXPECT(jdt_attn_decode_fp8_long_rows(buf, buf, buf + 4, sp, sp, buf, ip, fp, 396, 1, 2, 64, 320, .125f, nullptr) == -6,
         "attn_decode_fp8_long_rows rejects a cache off an 8-byte boundary");
  EXPECT(jdt_attn_decode_fp8_long_rows(buf, buf, buf, sp, sp, buf, ip, fp, 395, 1, 2, 64, 320, .125f, nullptr) == -10,
         "attn_decode_fp8_long_rows rejects a short ws");
  EXPECT(jdt_attn_append_fp8(buf, buf, buf, sp, sp, buf, ip, 1, 64, 2, 32, 320, .125f, nullptr) == -3,
         "attn_append_fp8 rejects head dim 32");
  EXPECT(jdt_attn_append_fp8(buf, buf, buf, sp, sp, buf, ip, 1, 1025, 2, 64, 320, .125f, nullptr) == -11,
         "attn_append_fp8 rejects C 1025");
  EXPECT(jdt_attn_append_fp8(buf, buf, buf, nullptr, sp, buf, ip, 1, 64, 2, 64, 320, .125f, nullptr) == -2,
         "attn_append_fp8 rejects a null k_scale");
  EXPECT(jdt_attn_append_fp8(buf, buf + 4, buf, sp, sp, buf, ip, 1, 64, 2, 64, 320, .125f, nullptr) == -6,
         "attn_append_fp8 rejects a cache off an 8-byte boundary");
  EXPECT(jdt_attn_append_fp8(buf, buf, buf, sp, sp, buf, ip, 0, 64, 2, 64, 320, .125f, nullptr) == 0,
         "attn_append_fp8 B = 0 is a no-op");
  EXPECT(jdt_attn_append_fp8_rows(buf, buf, buf, sp, sp, buf, ip, nullptr, 1, 64, 2, 64, 320, .125f, nullptr) == -2,
         "attn_append_fp8_rows rejects a null count");
  EXPECT(jdt_attn_append_fp8_rows(buf, buf, buf, sp, sp_mis, buf, ip, ip, 1, 64, 2, 64, 320, .125f, nullptr) == -6,
         "attn_append_fp8_rows rejects a misaligned scale");
  EXPECT(jdt_kv_quantize_rows(buf, buf, buf, sp, sp, 1, 2, 32, 128, 128, 16, nullptr) == -3,
         "kv_quantize_rows rejects head dim 32");
  EXPECT(jdt_kv_quantize_rows(buf, buf, buf, sp, sp, 1, 2, 64, 128, 64, 65, nullptr) == -5,
         "kv_quantize_rows rejects n > Sp");
  EXPECT(jdt_kv_quantize_rows(buf, buf, buf, sp, nullptr, 1, 2, 64, 128, 128, 16, nullptr) == -2,
         "kv_quantize_rows rejects null");
  EXPECT(jdt_kv_quantize_rows(buf, buf + 4, buf, sp, sp, 1, 2, 64, 128, 128, 16, nullptr) == -6,
         "kv_quantize_rows rejects a cache off an 8-byte boundary");
  EXPECT(jdt_kv_quantize_rows(buf, buf, buf, sp, sp, 1, 2, 64, 128, 128, 0, nullptr) == 0,
         "kv_quantize_rows n = 0 is a no-op");
  std::printf("asan host check: %d failure(s)\n", failures);
  return failures ? 1 : 0;
}
