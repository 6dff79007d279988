"""FP8 KV cache on the MI355X: the quantizing decode, append and prefill-copy kernels
(csrc/attn_decode.hip and csrc/attn_append.hip with FP8 = true, csrc/kv_quantize.hip) against the
reference quantizer of ops/kernels.py -- cache bytes and scales exactly -- and against the existing
bf16 kernels run on the dequantized values, which are exactly representable in bf16.

Shapes: B = 3, H in {2, 8}, caches of 128 rows (one launch) and 320 rows (split-KV: two full 128-key
chunks and a ragged third), positions on both sides of every chunk seam and of the 32-key passes."""
import ctypes

import pytest
import torch

from jax_distributed_tuts_amd.generation import Generator
from jax_distributed_tuts_amd.ops import _lib
from jax_distributed_tuts_amd.ops import kernels as kern

from . import test_generate as T
from . import test_generate_append as TA
from . import test_generate_long as TL

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0) if torch.cuda.is_available() else None
B, CPU, CFG_LONG = T.B, T.CPU, TL.CFG_LONG
POSITIONS = {128: [0, 1, 31, 32, 127], 320: [0, 127, 128, 129, 255, 256, 257, 319]}
posr = TA.posr


class Cache:
    """One layer's quantized caches on the CPU (from bf16 rows) with device copies to run on."""

    def __init__(self, kc, vc):
        (self.k, self.ks), (self.v, self.vs) = kern.kv_quantize(kc), kern.kv_quantize(vc)
        self.dev = [t.to(DEV).clone() for t in (self.k, self.v, self.ks, self.vs)]

    def dequantized(self):
        return kern.kv_dequantize(self.k, self.ks), kern.kv_dequantize(self.v, self.vs)

    def fresh(self):
        self.dev = [t.to(DEV).clone() for t in (self.k, self.v, self.ks, self.vs)]
        return self

    def unchanged(self):
        return all(torch.equal(d.cpu(), h) for d, h in zip(self.dev, (self.k, self.v, self.ks, self.vs)))


def decode(qkv, c, pos, H, **kw):
    k, v, ks, vs = c.dev
    return kern.attention_decode(qkv.to(DEV), k, v, pos, H, k_scale=ks, v_scale=vs, **kw)


def token_qdq(qkv, H):
    """(qkv with its k / v columns quantized and dequantized, (kq, ks), (vq, vs)) of a decode step's qkv."""
    v4 = qkv.clone().view(-1, 3, H, 64)
    kq, vq = kern.kv_quantize(v4[:, 1]), kern.kv_quantize(v4[:, 2])
    v4[:, 1], v4[:, 2] = kern.kv_dequantize(*kq), kern.kv_dequantize(*vq)
    return v4.view(qkv.shape[0], -1).contiguous(), kq, vq


CASES = [(S, p, H) for S in (128, 320) for p in POSITIONS[S] for H in (2, 8)]


# ----------------------------------------------------------------------------- 1. bytes, 2. values
@pytest.mark.parametrize("S_max,pos,H", CASES)
def test_decode_bytes_and_values(S_max, pos, H):
    """Row pos of K, V and both scales equals kv_quantize of the token's k / v exactly and every other byte
    and scale is unchanged.  Values: e_fp8 <= 2 e_ref, where both errors are against fp64 attention over
    the dequantized cache and token, and e_ref is the existing bf16 kernel's on those same values."""
    qkv, kc, vc = T.decode_inputs(B, H, S_max, seed=1000 * H + S_max + pos)
    c = Cache(kc, vc)
    got = decode(qkv, c, T.posw(pos, DEV), H)
    qdq, (kq, ks), (vq, vs) = token_qdq(qkv, H)
    wk, wv, wks, wvs = c.k.clone(), c.v.clone(), c.ks.clone(), c.vs.clone()
    wk[:, :, pos], wv[:, :, pos], wks[:, :, pos], wvs[:, :, pos] = kq, vq, ks, vs
    for name, d, w in zip(("k", "v", "k_scale", "v_scale"), c.dev, (wk, wv, wks, wvs)):
        assert torch.equal(d.cpu(), w), name
    dk, dv = c.dequantized()
    want, _ = T.attn_decode_fp64(qdq, dk, dv, pos, H)
    ref = kern.attention_decode(qdq.to(DEV), dk.to(DEV), dv.to(DEV), T.posw(pos, DEV), H)
    e_ref = float((ref.cpu().double() - want).abs().max())
    e_fp8 = float((got.cpu().double() - want).abs().max())
    T.log_errors(name="attention_decode_fp8", S_max=S_max, pos=pos, H=H, e_fp8=e_fp8, e_ref=e_ref)
    assert e_fp8 <= 2 * e_ref, (e_fp8, e_ref)
    c2 = Cache(kc, vc)
    cpu = kern.attention_decode(qkv, c2.k, c2.v, T.posw(pos, CPU), H, k_scale=c2.ks, v_scale=c2.vs)
    T.close(got, cpu)
    assert torch.equal(c2.k, wk) and torch.equal(c2.vs, wvs)   # the composed path writes the same row


# ----------------------------------------------------------------------------- 3. bitwise
@pytest.mark.parametrize("H", [2, 8])
def test_decode_per_row_has_the_bits_of_the_shared_position(H):
    for S_max, pos in ((128, [0, 32, 127]), (320, [0, 128, 319])):
        qkv, kc, vc = T.decode_inputs(B, H, S_max, seed=60 + H)
        c = Cache(kc, vc)
        got = decode(qkv, c, posr(pos, DEV), H)
        rows = [t.clone() for t in c.dev]
        for b, p in enumerate(pos):
            ref = decode(qkv, c.fresh(), T.posw(p, DEV), H)
            assert torch.equal(got[b], ref[b])
            assert all(torch.equal(r[b], d[b]) for r, d in zip(rows, c.dev))


@pytest.mark.parametrize("H", [2, 8])
def test_decode_one_chunk_has_the_bits_of_the_one_launch_kernel(H):
    """S_max = 129 at pos < 128 is the split pair with one live chunk: o and row pos as from S_max = 128."""
    for pos in (0, 63, 127):
        qkv, kc, vc = T.decode_inputs(B, H, 129, seed=50 * H + pos)
        short, long_ = Cache(kc[:, :, :128].contiguous(), vc[:, :, :128].contiguous()), Cache(kc, vc)
        want = decode(qkv, short, T.posw(pos, DEV), H)
        got = decode(qkv, long_, T.posw(pos, DEV), H)
        assert torch.equal(got, want)
        for a, b in zip(long_.dev, short.dev):
            assert torch.equal(a[:, :, :128], b)


def test_decode_two_calls_same_bits_and_stale_workspace():
    H, S_max = 8, 320
    qkv, kc, vc = T.decode_inputs(B, H, S_max, seed=70)
    c = Cache(kc, vc)
    for pos in (T.posw(200, DEV), posr([17, 128, 300], DEV)):
        a = decode(qkv, c.fresh(), pos, H)
        ka = [t.clone() for t in c.dev]
        b = decode(qkv, c.fresh(), pos, H)
        assert torch.equal(a, b) and all(torch.equal(x, y) for x, y in zip(ka, c.dev))
        nan = torch.full((B * H, 3, 66), float("nan"), device=DEV)
        n = decode(qkv, c.fresh(), pos, H, ws=nan)
        assert torch.equal(n, a) and all(torch.equal(x, y) for x, y in zip(ka, c.dev))
    last = 200 // 128
    nan = torch.full((B * H, 3, 66), float("nan"), device=DEV)
    decode(qkv, c.fresh(), T.posw(200, DEV), H, ws=nan)
    assert not bool(nan[:, :last + 1].isnan().any()) and bool(nan[:, last + 1:].isnan().all())


# ----------------------------------------------------------------------------- 4. out of range, codes
@pytest.mark.parametrize("S_max", [128, 320])
def test_decode_out_of_range(S_max):
    H = 2
    qkv, kc, vc = T.decode_inputs(B, H, S_max, seed=3)
    c = Cache(kc, vc)
    for pos in (-1, S_max, 2 ** 30):
        o = torch.full((B, H * 64), 7.0, dtype=torch.bfloat16, device=DEV)
        decode(qkv, c, T.posw(pos, DEV), H, out=o)
        assert c.unchanged() and bool((o == 7.0).all())
        o = torch.full((B, H * 64), 7.0, dtype=torch.bfloat16, device=DEV)
        ps = [5, pos, S_max - 1]
        decode(qkv, c.fresh(), posr(ps, DEV), H, out=o)
        ref = decode(qkv, Cache(kc, vc), posr([5, 5, S_max - 1], DEV), H)
        assert bool((o[1] == 7.0).all()) and torch.equal(o[0], ref[0]) and torch.equal(o[2], ref[2])
        assert all(torch.equal(d[1].cpu(), h[1]) for d, h in zip(c.dev, (c.k, c.v, c.ks, c.vs)))
        c.fresh()


@pytest.mark.parametrize("rows", [False, True])
@pytest.mark.parametrize("long_", [False, True])
def test_decode_return_codes(rows, long_):
    """Every rejection comes before anything is launched: the buffers keep their sentinels."""
    H = 2
    name = "jdt_attn_decode_fp8" + ("_long" if long_ else "") + ("_rows" if rows else "")
    top = 32768 if long_ else 128

    def case(Dh=64, S_max=None, Bq=B, null=(), off=(), short=False):
        S_max = (320 if long_ else 128) if S_max is None else S_max
        rows_alloc = min(max(S_max, 1), 512)
        t = dict(qkv=torch.zeros(B, 3 * H * Dh + 16, dtype=torch.bfloat16, device=DEV),
                 kc=torch.full((B * H * rows_alloc * Dh + 16,), 3, dtype=torch.uint8, device=DEV),
                 ks=torch.full((B * H * rows_alloc + 4,), 5.0, device=DEV),
                 o=torch.full((B, H * Dh), 7.0, dtype=torch.bfloat16, device=DEV),
                 pos=posr([0] * B, DEV) if rows else T.posw(0, DEV),
                 ws=torch.full((kern.attention_decode_ws_floats(B, H, rows_alloc),), 9.0, device=DEV))
        t["vc"], t["vs"] = t["kc"].clone(), t["ks"].clone()
        p = {k: (None if k in null else ctypes.c_void_p(v.data_ptr() + (off[1] if off and off[0] == k else 0)))
             for k, v in t.items()}
        args = [p["qkv"], p["kc"], p["vc"], p["ks"], p["vs"], p["o"], p["pos"]]
        if long_:
            args += [p["ws"], kern.attention_decode_ws_floats(Bq, H, S_max) - 1 if short else t["ws"].numel()]
        rc = getattr(_lib.lib(), name)(*args, Bq, H, Dh, S_max, 0.125, _lib.stream_ptr())
        torch.cuda.synchronize()
        assert bool((t["o"] == 7.0).all()) and bool((t["kc"] == 3).all()) and bool((t["vc"] == 3).all())
        assert bool((t["ks"] == 5.0).all()) and bool((t["vs"] == 5.0).all()) and bool((t["ws"] == 9.0).all())
        return rc

    assert case(Dh=32) == -3 and case(Dh=128) == -3
    assert case(S_max=0) == -4 and case(S_max=top + 1) == -4
    for arg in ("qkv", "kc", "vc", "ks", "vs", "o", "pos") + (("ws",) if long_ else ()):
        assert case(null=(arg,)) == -2, arg
    for arg, by in (("qkv", 8), ("kc", 4), ("vc", 4), ("kc", 1), ("ks", 2), ("vs", 2)):
        assert case(off=(arg, by)) == -6, (arg, by)
    if long_:
        assert case(short=True) == -10 and case(S_max=129, short=True) == -10
    assert case(Bq=0) == 0   # a no-op


# ----------------------------------------------------------------------------- 5. append
def append_fp8(qkv, c, pos, H, C, count=None, o=None):
    k, v, ks, vs = c.dev
    return kern.attention_append(qkv.to(DEV), k, v, pos, H, C, count=count, out=o, k_scale=ks, v_scale=vs)


def chunk_qdq(qkv, Bq, C, H):
    """(qkv with k / v quantized and dequantized, the chunk's (kq, ks), (vq, vs) in the cache's layout)."""
    v5 = qkv.clone().view(Bq, C, 3, H, 64)
    kq, vq = kern.kv_quantize(v5[:, :, 1]), kern.kv_quantize(v5[:, :, 2])
    v5[:, :, 1], v5[:, :, 2] = kern.kv_dequantize(*kq), kern.kv_dequantize(*vq)
    lay = lambda q, s: (q.permute(0, 2, 1, 3), s.permute(0, 2, 1))  # noqa: E731
    return v5.view(Bq * C, -1).contiguous(), lay(*kq), lay(*vq)


@pytest.mark.parametrize("H", [2, 8])
@pytest.mark.parametrize("p,C", [(0, 1), (0, 64), (5, 7), (63, 65), (64, 130), (200, 64)])
def test_append_bytes_and_bits(p, C, H):
    """Cache rows p..p+C-1 and their scales equal kv_quantize exactly, everything else is unchanged, and o is
    bit for bit the bf16 kernel's on a bf16 cache of the dequantized values with the chunk's k / v columns
    quantized and dequantized: the staging and the tile body are shared and dequantization is exact."""
    qkv, kc, vc = TA.append_inputs(H, C, seed=10 * p + C + H)
    c = Cache(kc, vc)
    got = append_fp8(qkv, c, T.posw(p, DEV), H, C)
    qdq, (kq, ks), (vq, vs) = chunk_qdq(qkv, B, C, H)
    wk, wv, wks, wvs = c.k.clone(), c.v.clone(), c.ks.clone(), c.vs.clone()
    wk[:, :, p:p + C], wv[:, :, p:p + C], wks[:, :, p:p + C], wvs[:, :, p:p + C] = kq, vq, ks, vs
    for name, d, w in zip(("k", "v", "k_scale", "v_scale"), c.dev, (wk, wv, wks, wvs)):
        assert torch.equal(d.cpu(), w), name
    dk, dv = c.dequantized()
    ref, _, _ = TA.run_append(DEV, qdq, dk, dv, T.posw(p, DEV), H, C)
    assert torch.equal(got, ref)
    c2 = Cache(kc, vc)
    cpu = kern.attention_append(qkv, c2.k, c2.v, T.posw(p, CPU), H, C, k_scale=c2.ks, v_scale=c2.vs)
    T.close(got, cpu)
    assert torch.equal(c2.k, wk) and torch.equal(c2.ks, wks)


def test_append_per_row_counts():
    H, C = 2, 64
    pos, count = [0, 70, 130], [0, 3, C]
    qkv, kc, vc = TA.append_inputs(H, C, seed=5)
    c = Cache(kc, vc)
    o = torch.full((B * C, H * 64), 7.0, dtype=torch.bfloat16, device=DEV)
    append_fp8(qkv, c, posr(pos, DEV), H, C, count=posr(count, DEV), o=o)
    qdq, (kq, ks), (vq, vs) = chunk_qdq(qkv, B, C, H)
    wk, wv, wks, wvs = c.k.clone(), c.v.clone(), c.ks.clone(), c.vs.clone()
    for b, (p, n) in enumerate(zip(pos, count)):
        wk[b, :, p:p + n], wv[b, :, p:p + n] = kq[b, :, :n], vq[b, :, :n]
        wks[b, :, p:p + n], wvs[b, :, p:p + n] = ks[b, :, :n], vs[b, :, :n]
    for name, d, w in zip(("k", "v", "k_scale", "v_scale"), c.dev, (wk, wv, wks, wvs)):
        assert torch.equal(d.cpu(), w), name
    dk, dv = c.dequantized()
    ro = torch.full((B * C, H * 64), 7.0, dtype=torch.bfloat16, device=DEV)
    TA.run_append(DEV, qdq, dk, dv, posr(pos, DEV), H, C, count=posr(count, DEV), o=ro)
    assert torch.equal(o, ro) and bool((o.view(B, C, -1)[0] == 7.0).all()) and bool((o.view(B, C, -1)[1, 3:] == 7.0).all())


def test_append_cut_invariance():
    """The same 130 tokens appended as 130, 64 + 66 and 7 x 18 + 4: identical bytes, scales and o."""
    H, N, p0 = 2, 130, 37
    qkv, kc, vc = TA.append_inputs(H, N, seed=77)
    q3 = qkv.view(B, N, -1)
    results = []
    for cuts in ([130], [64, 66], [18] * 7 + [4]):
        c, p, outs = Cache(kc, vc), p0, []
        for n in cuts:
            part = q3[:, p - p0:p - p0 + n].reshape(B * n, -1).contiguous()
            outs.append(append_fp8(part, c, T.posw(p, DEV), H, n).view(B, n, -1))
            p += n
        results.append((torch.cat(outs, 1), [t.clone() for t in c.dev]))
    o0, c0 = results[0]
    for o, cc in results[1:]:
        assert torch.equal(o, o0) and all(torch.equal(a, b) for a, b in zip(cc, c0))


@pytest.mark.parametrize("H", [2, 8])
def test_append_c1_agrees_with_decode(H):
    for p in (0, 63, 64, 200, 319):
        qkv, kc, vc = T.decode_inputs(B, H, 320, seed=40 + p)
        a, d = Cache(kc, vc), Cache(kc, vc)
        got = append_fp8(qkv, a, T.posw(p, DEV), H, 1)
        dec = decode(qkv, d, T.posw(p, DEV), H)
        T.close(got, dec)
        assert all(torch.equal(x, y) for x, y in zip(a.dev, d.dev))


def test_append_out_of_range_and_codes():
    H, C = 2, 64
    qkv, kc, vc = TA.append_inputs(H, C, seed=3)
    c = Cache(kc, vc)
    for p in (-1, 320 - C + 1, 320):
        o = torch.full((B * C, H * 64), 7.0, dtype=torch.bfloat16, device=DEV)
        append_fp8(qkv, c, T.posw(p, DEV), H, C, o=o)
        assert c.unchanged() and bool((o == 7.0).all())
    k, v, ks, vs = c.dev
    o = torch.full((B * C, H * 64), 7.0, dtype=torch.bfloat16, device=DEV)
    P = lambda t, off=0: ctypes.c_void_p(t.data_ptr() + off)  # noqa: E731
    pos, q = T.posw(0, DEV), qkv.to(DEV)

    def call(a, Dh=64, S_max=320, Cc=C):
        return _lib.lib().jdt_attn_append_fp8(*a, B, Cc, H, Dh, S_max, 0.125, _lib.stream_ptr())

    good = [P(q), P(k), P(v), P(ks), P(vs), P(o), P(pos)]
    for i in range(7):
        assert call(good[:i] + [None] + good[i + 1:]) == -2, i
    assert call([P(q), P(k, 4), P(v), P(ks), P(vs), P(o), P(pos)]) == -6
    assert call([P(q), P(k), P(v), P(ks), P(vs, 2), P(o), P(pos)]) == -6
    assert call(good, Dh=32) == -3 and call(good, S_max=32769) == -4 and call(good, Cc=1025) == -11
    torch.cuda.synchronize()
    assert c.unchanged() and bool((o == 7.0).all())
    with pytest.raises(ValueError, match="split"):
        kern.attention_append(q, k, v, pos, H, C, ws=torch.zeros(8, device=DEV), k_scale=ks, v_scale=vs)


# ----------------------------------------------------------------------------- 6. prefill copy
@pytest.mark.parametrize("seq_len,Pn", [(128, 1), (128, 17), (128, 128), (320, 200)])
def test_prefill_copy(seq_len, Pn):
    """An fp8 and a bf16 Generator prefill the same prompt through the training forward: the FP8 cache holds
    kv_quantize of the bf16 cache's rows < P exactly, and rows >= P are untouched."""
    cfg = T.CFG if seq_len == 128 else CFG_LONG
    model, P = T.make_model(cfg, DEV, 1)
    prompt = torch.randint(0, cfg.vocab_size, (B, Pn), generator=torch.Generator().manual_seed(Pn)).to(torch.int32)
    gen, bf = Generator(model, P, B, DEV, kv_dtype="fp8"), Generator(model, P, B, DEV)
    for l in range(cfg.n_layers):
        gen.kv.k[l].fill_(9), gen.kv.v[l].fill_(9), gen.kv.k_scale[l].fill_(3.0), gen.kv.v_scale[l].fill_(3.0)
    gen.prefill(prompt.to(DEV))
    bf.prefill(prompt.to(DEV))
    assert int(gen.kv.pos.item()) == Pn - 1 and gen.prefill_rows == bf.prefill_rows
    for l in range(cfg.n_layers):
        for cache, sc, src in ((gen.kv.k[l], gen.kv.k_scale[l], bf.kv.k[l]), (gen.kv.v[l], gen.kv.v_scale[l], bf.kv.v[l])):
            wq, wsc = kern.kv_quantize(src[:, :, :Pn].cpu())
            assert torch.equal(cache[:, :, :Pn].cpu(), wq) and torch.equal(sc[:, :, :Pn].cpu(), wsc), l
            assert bool((cache[:, :, Pn:] == 9).all()) and bool((sc[:, :, Pn:] == 3.0).all())


def test_kv_quantize_rows_codes():
    H, Sp, S_max = 2, 16, 32
    qkv = torch.zeros(B * Sp, 3 * H * 64, dtype=torch.bfloat16, device=DEV)
    kc = torch.full((B, H, S_max, 64), 9, dtype=torch.uint8, device=DEV)
    vc, ks = kc.clone(), torch.full((B, H, S_max), 3.0, device=DEV)
    vs = ks.clone()
    P = lambda t, off=0: ctypes.c_void_p(t.data_ptr() + off)  # noqa: E731

    def call(a, Dh=64, n=8, Sp_=Sp):
        return _lib.lib().jdt_kv_quantize_rows(*a, B, H, Dh, S_max, Sp_, n, _lib.stream_ptr())

    good = [P(qkv), P(kc), P(vc), P(ks), P(vs)]
    for i in range(5):
        assert call(good[:i] + [None] + good[i + 1:]) == -2, i
    assert call([P(qkv), P(kc, 4), P(vc), P(ks), P(vs)]) == -6 and call([P(qkv, 8)] + good[1:]) == -6
    assert call(good, Dh=32) == -3 and call(good, n=Sp + 1) == -5 and call(good, n=S_max + 1, Sp_=64) == -5
    assert call(good, n=0) == 0
    torch.cuda.synchronize()
    assert bool((kc == 9).all()) and bool((vc == 9).all()) and bool((ks == 3.0).all()) and bool((vs == 3.0).all())
    kern.kv_cache_fill(qkv, kc, vc, ks, vs, 8, Sp)   # zero rows: bytes 0, scale 1
    assert bool((kc[:, :, :8] == 0).all()) and bool((vs[:, :, :8] == 1.0).all()) and bool((kc[:, :, 8:] == 9).all())


# ----------------------------------------------------------------------------- 7. end to end
@pytest.mark.parametrize("cfg", [T.CFG, CFG_LONG], ids=["128", "320"])
@pytest.mark.parametrize("temperature", [0.0, 0.8])
def test_captured_equals_eager(cfg, temperature):
    model, P = T.make_model(cfg, DEV, 3)
    gen = Generator(model, P, B, DEV, kv_dtype="fp8")
    S = cfg.seq_len
    prompt = torch.randint(0, cfg.vocab_size, (B, S - 60), generator=torch.Generator().manual_seed(4))
    prompt = prompt.to(torch.int32).to(DEV)
    for pr, kw in ((prompt[:, :S - 70], {}), (prompt, dict(prompt_lens=[5, S // 2, S - 60], eos_id=7)),
                   (prompt[:, :S - 70], dict(prefill_chunk=64, top_k=40, top_p=0.9))):
        eager = gen.generate(pr, 12, temperature=temperature, seed=11, capture=False, **kw)
        eager_logits, eager_lengths = gen.logits.clone(), gen.lengths.clone()
        for _ in range(2):   # the call that captures, then one that only replays
            graph = gen.generate(pr, 12, temperature=temperature, seed=11, capture=True, **kw)
            assert torch.equal(graph, eager)
            assert torch.equal(gen.logits, eager_logits) and torch.equal(gen.lengths, eager_lengths)
        assert gen._graphs[gen._graph_key()][0] is not None   # the step really was captured


@pytest.mark.parametrize("cfg", [T.CFG, CFG_LONG], ids=["128", "320"])
def test_teacher_forced_logits_agree_with_cpu(cfg):
    """Chunked prefill, extend and teacher-forced steps on the GPU against the same calls on CPU tensors."""
    model, P = T.make_model(cfg, CPU, 4)
    S = cfg.seq_len
    tok = torch.randint(0, cfg.vocab_size, (B, S), generator=torch.Generator().manual_seed(5)).to(torch.int32)
    gens = []
    for dev in (CPU, DEV):
        Pd = P if dev is CPU else T.make_model(cfg, DEV, 4)[1]
        g = Generator(model, Pd, B, dev, kv_dtype="fp8")
        g.prefill(tok[:, :S - 40].to(dev), chunk=64)
        out = [g.extend(tok[:, S - 40:S - 8].to(dev), chunk=13, logits=True)]
        g.kv.tokens.copy_(tok.to(dev))
        out += [g.step(sample=False).clone() for _ in range(7)]
        gens.append((g, out))
    (gc, oc), (gg, og) = gens
    assert int(gg.kv.pos.item()) == int(gc.kv.pos.item()) == S - 2
    for a, b in zip(og, oc):
        T.close(a, b)


def test_prefill_cuts_agree_gpu():
    """Chunk 7, chunk 64 and token by token on the kernels: the next step's logits agree.  (The GEMMs that
    produce k / v may round differently at another row count, so the bytes are compared at the kernel level,
    test_append_cut_invariance, and on CPU tensors.)"""
    cfg, Pn = CFG_LONG, 150
    model, P = T.make_model(cfg, DEV, 4)
    tok = torch.randint(0, cfg.vocab_size, (B, Pn), generator=torch.Generator().manual_seed(5)).to(torch.int32).to(DEV)
    gens = [Generator(model, P, B, DEV, kv_dtype="fp8") for _ in range(3)]
    gens[0].prefill(tok, chunk=7)
    gens[1].prefill(tok, chunk=64)
    gens[2].prefill(tok[:, :1])
    gens[2].kv.tokens[:, :Pn] = tok
    for _ in range(Pn - 1):
        gens[2].step(sample=False)
    logits = [g.step(sample=False).clone() for g in gens]
    T.close(logits[1], logits[0])
    T.close(logits[2], logits[0])
    assert all(int(g.kv.pos.item()) == Pn for g in gens)


def test_needle_fp8():
    """test_needle_long's construction on the quantized cache: one cached key aligned with q carries softmax
    weight > 1 - 1e-4 after dequantization, so o must be that key's dequantized value row."""
    H, S_max = 2, 320
    for pos in (256, 319):
        for j in sorted({0, 127, 128, 255, 256, pos}):
            qkv, kc, vc = T.decode_inputs(B, H, S_max, seed=2000 + pos + j)
            q = qkv.float().view(B, 3, H, 64)[:, 0]
            needle = (20.0 * q / q.norm(dim=-1, keepdim=True)).to(torch.bfloat16)
            kc = (kc.float() * 0.05).to(torch.bfloat16)
            new = qkv.clone().view(B, 3, H, 64)
            new[:, 1] = (new[:, 1].float() * 0.05).to(torch.bfloat16)
            if j == pos:
                new[:, 1] = needle
            else:
                kc[:, :, j] = needle
            qkv = new.view(B, -1).contiguous()
            c = Cache(kc, vc)
            qdq, _, _ = token_qdq(qkv, H)
            dk, dv = c.dequantized()
            want, p = T.attn_decode_fp64(qdq, dk, dv, pos, H)
            assert float(p[:, :, j].min()) > 1 - 1e-4
            vj = (qdq.view(B, 3, H, 64)[:, 2] if j == pos else dv[:, :, j]).reshape(B, -1)
            got = decode(qkv, c, T.posw(pos, DEV), H)
            T.close(got, vj)
            T.close(got, want)


def test_longest_cache_accepted():
    """S_max = 32768, the top of the envelope, at its last position and at the first."""
    H, S_max = 1, 32768
    qkv, kc, vc = T.decode_inputs(1, H, S_max, seed=4)
    c = Cache(kc, vc)
    qdq, (kq, ks), _ = token_qdq(qkv, H)
    dk, dv = c.dequantized()
    for pos in (S_max - 1, 0):
        got = decode(qkv, c.fresh(), T.posw(pos, DEV), H)
        want, _ = T.attn_decode_fp64(qdq, dk, dv, pos, H)
        T.close(got, want)
        assert torch.equal(c.dev[0][:, :, pos].cpu(), kq) and torch.equal(c.dev[2][:, :, pos].cpu(), ks)
