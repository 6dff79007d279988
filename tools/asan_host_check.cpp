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

alignas(16) static unsigned char buf[64];

// The 14 KV-cache attention launchers (attn_decode.hip, attn_append.hip) share one ladder of checks, so one
// list of cases runs over every variant: KvArgs holds every argument any of them takes, a variant's ``call``
// passes on the ones its entry point has.
struct KvArgs {
  const void* qkv;
  void *k_cache, *v_cache;
  float *k_scale, *v_scale;
  void* o;
  const int *pos, *count;
  float* ws;
  long ws_floats;
  int B, C, H, Dh, S_max;
};
struct KvVariant {
  const char* name;
  int (*call)(const KvArgs&);
  bool rows, split, fp8;
};
#define KV_DECODE(fn, ...) [](const KvArgs& a) { return fn(__VA_ARGS__, a.B, a.H, a.Dh, a.S_max, .125f, nullptr); }
#define KV_APPEND(fn, ...) [](const KvArgs& a) { return fn(__VA_ARGS__, a.B, a.C, a.H, a.Dh, a.S_max, .125f, nullptr); }
static const KvVariant kv_decode[] = {
    {"attn_decode", KV_DECODE(jdt_attn_decode, a.qkv, a.k_cache, a.v_cache, a.o, a.pos), false, false, false},
    {"attn_decode_rows", KV_DECODE(jdt_attn_decode_rows, a.qkv, a.k_cache, a.v_cache, a.o, a.pos), true, false, false},
    {"attn_decode_long", KV_DECODE(jdt_attn_decode_long, a.qkv, a.k_cache, a.v_cache, a.o, a.pos, a.ws, a.ws_floats),
     false, true, false},
    {"attn_decode_long_rows",
     KV_DECODE(jdt_attn_decode_long_rows, a.qkv, a.k_cache, a.v_cache, a.o, a.pos, a.ws, a.ws_floats), true, true,
     false},
    {"attn_decode_fp8", KV_DECODE(jdt_attn_decode_fp8, a.qkv, a.k_cache, a.v_cache, a.k_scale, a.v_scale, a.o, a.pos),
     false, false, true},
    {"attn_decode_fp8_rows",
     KV_DECODE(jdt_attn_decode_fp8_rows, a.qkv, a.k_cache, a.v_cache, a.k_scale, a.v_scale, a.o, a.pos), true, false,
     true},
    {"attn_decode_fp8_long", KV_DECODE(jdt_attn_decode_fp8_long, a.qkv, a.k_cache, a.v_cache, a.k_scale, a.v_scale, a.o,
                                       a.pos, a.ws, a.ws_floats),
     false, true, true},
    {"attn_decode_fp8_long_rows", KV_DECODE(jdt_attn_decode_fp8_long_rows, a.qkv, a.k_cache, a.v_cache, a.k_scale,
                                            a.v_scale, a.o, a.pos, a.ws, a.ws_floats),
     true, true, true},
};
static const KvVariant kv_append[] = {
    {"attn_append", KV_APPEND(jdt_attn_append, a.qkv, a.k_cache, a.v_cache, a.o, a.pos), false, false, false},
    {"attn_append_rows", KV_APPEND(jdt_attn_append_rows, a.qkv, a.k_cache, a.v_cache, a.o, a.pos, a.count), true, false,
     false},
    {"attn_append_split", KV_APPEND(jdt_attn_append_split, a.qkv, a.k_cache, a.v_cache, a.o, a.pos, a.ws, a.ws_floats),
     false, true, false},
    {"attn_append_split_rows",
     KV_APPEND(jdt_attn_append_split_rows, a.qkv, a.k_cache, a.v_cache, a.o, a.pos, a.count, a.ws, a.ws_floats), true,
     true, false},
    {"attn_append_fp8", KV_APPEND(jdt_attn_append_fp8, a.qkv, a.k_cache, a.v_cache, a.k_scale, a.v_scale, a.o, a.pos),
     false, false, true},
    {"attn_append_fp8_rows",
     KV_APPEND(jdt_attn_append_fp8_rows, a.qkv, a.k_cache, a.v_cache, a.k_scale, a.v_scale, a.o, a.pos, a.count), true,
     false, true},
};

static void kv_expect(const KvVariant& v, const KvArgs& a, int want, const char* what) {
  const int got = v.call(a);
  if (got != want) {
    std::fprintf(stderr, "FAIL: %s %s: returned %d, expected %d\n", v.name, what, got, want);
    ++failures;
  }
}

// Every variant of a family against the whole ladder, in the ladder's order: head dim 64 (-3), S_max in 1..top
// with top = 128 for the one-launch decode and 32768 otherwise (-4), append: C in 1..1024 (-11), B >= 0, H >= 1
// and B * H within the grid: INT_MAX for decode, 65535 for append (-5), the pointers the variant takes (-2),
// alignment (-6), split: the workspace (-10), and B = 0 as a no-op.  Each case changes ``ok``, arguments the
// variant accepts (and would launch with: never passed as they are), in the one way it names.
static void kv_check_family(const KvVariant* variants, int n, bool append) {
  int* ip = reinterpret_cast<int*>(buf);
  float* fp = reinterpret_cast<float*>(buf);
  const long big = 1L << 40;   // a workspace size no shape here exceeds
  for (int i = 0; i < n; ++i) {
    const KvVariant& v = variants[i];
    const int s_top = append || v.split ? 32768 : 128;
    // B = 1, H = 2; decode: 3 chunks of 128 keys x 66 floats; append: 1 query tile x 1 span of 512 keys x 64 x 66
    const long need = append ? 2 * 64 * 66 : 2 * 3 * 66;
    const KvArgs ok = {buf, buf, buf, fp, fp, buf, ip, ip, fp, need, 1, 64, 2, 64, s_top == 128 ? 128 : 320};
#define KV_CASE(edit, want, what) \
  do {                            \
    KvArgs c = ok;                \
    edit;                         \
    kv_expect(v, c, want, what);  \
  } while (0)
    KV_CASE(c.Dh = 32, -3, "rejects head dim 32");
    KV_CASE(c.Dh = 128, -3, "rejects head dim 128");
    KV_CASE((c.Dh = 32, c.S_max = 0, c.B = -1, c.qkv = nullptr), -3, "checks the head dim first");
    KV_CASE(c.S_max = 0, -4, "rejects S_max 0");
    KV_CASE((c.S_max = s_top + 1, c.ws_floats = big), -4, "rejects S_max past its envelope");
    if (append) {
      KV_CASE(c.C = 0, -11, "rejects C 0");
      KV_CASE((c.C = 1025, c.ws_floats = big), -11, "rejects C 1025");
    }
    KV_CASE((c.B = 65536, c.H = append ? 1 : 65536, c.ws_floats = big), -5, "rejects B * H past the grid");
    KV_CASE(c.B = -1, -5, "rejects B < 0");
    KV_CASE(c.H = 0, -5, "rejects H 0");
    KV_CASE(c.qkv = nullptr, -2, "rejects a null qkv");
    KV_CASE(c.k_cache = nullptr, -2, "rejects a null k_cache");
    KV_CASE(c.v_cache = nullptr, -2, "rejects a null v_cache");
    KV_CASE(c.o = nullptr, -2, "rejects a null o");
    KV_CASE(c.pos = nullptr, -2, "rejects a null pos");
    KV_CASE(c.qkv = buf + 4, -6, "rejects a misaligned qkv");
    KV_CASE(c.k_cache = buf + 4, -6, "rejects a misaligned k_cache");
    KV_CASE(c.v_cache = buf + 4, -6, "rejects a misaligned v_cache");
    KV_CASE((c.k_cache = c.v_cache = buf + 8, c.B = 0), v.fp8 ? 0 : -6, "takes 8-byte aligned caches as FP8 only");
    KV_CASE((c.B = 0, c.ws_floats = 0), 0, "B = 0 is a no-op");
    if (append && v.rows) KV_CASE(c.count = nullptr, -2, "rejects a null count");
    if (v.fp8) {
      KV_CASE(c.k_scale = nullptr, -2, "rejects a null k_scale");
      KV_CASE(c.v_scale = nullptr, -2, "rejects a null v_scale");
      KV_CASE(c.k_scale = reinterpret_cast<float*>(buf + 2), -6, "rejects a misaligned k_scale");
      KV_CASE(c.v_scale = reinterpret_cast<float*>(buf + 2), -6, "rejects a misaligned v_scale");
    }
    if (v.split) {
      KV_CASE(c.ws = nullptr, -2, "rejects a null ws");
      KV_CASE(c.ws_floats = need - 1, -10, "rejects a short ws");
      KV_CASE((c.S_max = append ? 513 : 385, c.ws_floats = append ? 2 * need - 1 : need + 2 * 66 - 1), -10,
              "rejects a ws short of one more span");
      if (append) KV_CASE((c.C = 65, c.ws_floats = 2 * need - 1), -10, "rejects a ws short of the second query tile");
    }
#undef KV_CASE
  }
}

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
  // the KV-cache attention launchers: the envelope is checked before anything is launched
  kv_check_family(kv_decode, 8, false);
  kv_check_family(kv_append, 6, true);
  // the other decode launchers (attn_decode.hip): embedding and samplers
  int* ip = reinterpret_cast<int*>(buf);
  unsigned* up = reinterpret_cast<unsigned*>(buf);
  EXPECT(jdt_embed_decode(ip, buf, buf, buf, ip, 1, 128, 60, 8, nullptr) == -3, "embed_decode rejects d % 8");
  EXPECT(jdt_embed_decode(ip, buf, buf, buf, ip, 0, 128, 64, 8, nullptr) == 0, "embed_decode B = 0 is a no-op");
  EXPECT(jdt_sample(buf, 8, 1, 0, 0.f, 0, 0, ip, 128, ip, up, nullptr) == -5, "sample rejects V = 0");
  EXPECT(jdt_sample(buf, 8, 1, 8, -1.f, 0, 0, ip, 128, ip, up, nullptr) == -7, "sample rejects temperature < 0");
  EXPECT(jdt_sample(buf, 8, 1, 8, 1.f, 0, 0, ip, 128, ip, nullptr, nullptr) == -2, "sample rejects a null ticket");
  EXPECT(jdt_sample(buf, 8, 0, 8, 1.f, 0, 0, ip, 128, ip, up, nullptr) == 0, "sample B = 0 is a no-op");
  // per-row and filtered variants: the same envelope, plus top_k / top_p
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
  // embed_append: d % 8, C in 1..1024, S_max >= 1
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
  // the FP8 prefill copy: null scales, 8-byte caches
  float* sp = reinterpret_cast<float*>(buf);
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
