"""FP8 KV cache on CPU tensors: the reference quantizer (ops/kernels.py ``kv_quantize`` /
``kv_dequantize``, the definition the HIP kernels are tested against) and ``Generator(...,
kv_dtype="fp8")`` through the composed torch paths.  The helpers are tests/test_generate.py's."""
import pytest
import torch

from jax_distributed_tuts_amd.generation import Generator, KVCache
from jax_distributed_tuts_amd.ops import kernels as kern

from . import test_generate as T

B, CPU, CFG = T.B, T.CPU, T.CFG


def quantizer_rows():
    """randn rows times magnitudes 2^-20 .. 2^20 (one magnitude per row), and an all-zero last row."""
    g = torch.Generator().manual_seed(0)
    mag = torch.exp2(torch.linspace(-20, 20, 410))
    x = (torch.randn(410, 64, generator=g) * mag[:, None]).to(torch.bfloat16)
    return torch.cat([x, torch.zeros(1, 64, dtype=torch.bfloat16)])


# ----------------------------------------------------------------------------- the quantizer
def test_quantizer_properties():
    x = quantizer_rows()
    q, scale = kern.kv_quantize(x)
    assert q.dtype == torch.uint8 and q.shape == x.shape and scale.dtype == torch.float32 and scale.shape == (411,)
    mant, _ = torch.frexp(scale)
    assert bool((mant == 0.5).all())                       # a power of two
    amax = x.float().abs().amax(-1)
    top = amax[:-1] / scale[:-1]                           # exact: a division by a power of two
    assert bool((top >= 128).all()) and bool((top < 256).all())
    f = q.view(torch.float8_e4m3fn).float()
    assert bool(torch.isfinite(f).all()) and float(f.abs().max()) <= 256
    exact = f.double() * scale.double()[:, None]           # float(q) * scale without any rounding
    dq = kern.kv_dequantize(q, scale)
    assert dq.dtype == torch.bfloat16 and torch.equal(dq.double(), exact)   # exact in bf16
    err = (dq.double() - x.double()).abs().amax(-1)
    assert bool((err <= amax.double() / 16).all())
    assert float(scale[-1]) == 1.0 and bool((q[-1] == 0).all()) and bool((dq[-1] == 0).all())


def test_quantizer_rounds_to_nearest_even():
    """Scaled values 128 + 8 k lie half way between two e4m3 values (the step in [128, 256) is 16): ties go
    to the even mantissa.  The row's 240 pins the scale to 1."""
    x = torch.zeros(1, 64)
    x[0, :8] = torch.tensor([240.0, 136.0, 152.0, 168.0, -136.0, -152.0, 129.0, 143.0])
    q, scale = kern.kv_quantize(x.to(torch.bfloat16))
    assert float(scale) == 1.0
    assert kern.kv_dequantize(q, scale)[0, :8].tolist() == [240.0, 128.0, 160.0, 160.0, -128.0, -160.0, 128.0, 144.0]


def test_quantizer_shapes():
    """Leading dims are free, and rows do not see each other."""
    x = quantizer_rows()[:408].view(2, 3, 68, 64)
    q, scale = kern.kv_quantize(x)
    assert q.shape == (2, 3, 68, 64) and scale.shape == (2, 3, 68)
    q1, s1 = kern.kv_quantize(x[1, 2, 5])
    assert s1.shape == () and torch.equal(q1, q[1, 2, 5]) and torch.equal(s1, scale[1, 2, 5])
    with pytest.raises(AssertionError):
        kern.kv_quantize(x.float())


# ----------------------------------------------------------------------------- ops on CPU tensors
def test_attention_decode_fp8_cpu():
    """The composed path: row pos of the caches and scales receives kv_quantize of the token's k / v, nothing
    else changes, and o is attention over the dequantized rows."""
    H, S_max, pos = 2, 128, 77
    qkv, kc, vc = T.decode_inputs(B, H, S_max, seed=5)
    (kq, ks), (vq, vs) = kern.kv_quantize(kc), kern.kv_quantize(vc)
    k2, v2, ks2, vs2 = kq.clone(), vq.clone(), ks.clone(), vs.clone()
    got = kern.attention_decode(qkv, k2, v2, T.posw(pos, CPU), H, k_scale=ks2, v_scale=vs2)
    tk, tv = qkv.view(B, 3, H, 64)[:, 1], qkv.view(B, 3, H, 64)[:, 2]
    kq[:, :, pos], ks[:, :, pos] = kern.kv_quantize(tk)
    vq[:, :, pos], vs[:, :, pos] = kern.kv_quantize(tv)
    assert torch.equal(k2, kq) and torch.equal(v2, vq) and torch.equal(ks2, ks) and torch.equal(vs2, vs)
    dq = qkv.clone().view(B, 3, H, 64)
    dq[:, 1], dq[:, 2] = kern.kv_dequantize(kq[:, :, pos], ks[:, :, pos]), kern.kv_dequantize(vq[:, :, pos],
                                                                                              vs[:, :, pos])
    want, _ = T.attn_decode_fp64(dq.view(B, -1), kern.kv_dequantize(kq, ks), kern.kv_dequantize(vq, vs), pos, H)
    T.close(got, want)
    with pytest.raises(AssertionError):   # uint8 caches need their scales
        kern.attention_decode(qkv, k2, v2, T.posw(pos, CPU), H)


def test_kv_cache_fill_cpu():
    H, S_max, Sp, n = 2, 96, 64, 37
    g = torch.Generator().manual_seed(3)
    qkv = torch.randn(B * Sp, 3 * H * 64, generator=g).to(torch.bfloat16)
    kc = torch.full((B, H, S_max, 64), 9, dtype=torch.uint8)
    vc, ks = kc.clone(), torch.full((B, H, S_max), 3.0)
    vs = ks.clone()
    kern.kv_cache_fill(qkv, kc, vc, ks, vs, n, Sp)
    q5 = qkv.view(B, Sp, 3, H, 64)
    for j, cache, sc in ((1, kc, ks), (2, vc, vs)):
        wq, wsc = kern.kv_quantize(q5[:, :n, j].permute(0, 2, 1, 3))
        assert torch.equal(cache[:, :, :n], wq) and torch.equal(sc[:, :, :n], wsc)
        assert bool((cache[:, :, n:] == 9).all()) and bool((sc[:, :, n:] == 3.0).all())


# ----------------------------------------------------------------------------- Generator
def test_kv_dtype_tensors():
    c = CFG
    kv = KVCache(c, B, CPU, kv_dtype="fp8")
    H, L, S = c.n_heads, c.n_layers, c.seq_len
    assert kv.k[0].dtype == kv.v[0].dtype == torch.uint8 and kv.k[0].shape == (B, H, S, 64)
    assert len(kv.k_scale) == len(kv.v_scale) == L and kv.k_scale[0].shape == (B, H, S)
    assert kv.k_scale[0].dtype == torch.float32 and bool((kv.k_scale[0] == 1).all()) and bool((kv.v_scale[1] == 1).all())
    assert kv.cache_bytes() == 2 * L * B * H * S * 68
    for ref in (KVCache(c, B, CPU), KVCache(c, B, CPU, kv_dtype="bf16")):   # today's object
        assert ref.k[0].dtype == ref.v[0].dtype == torch.bfloat16 and ref.k[0].shape == (B, H, S, 64)
        assert ref.k_scale is None and ref.v_scale is None and ref.kv_dtype == "bf16"
        assert ref.cache_bytes() == 2 * L * B * H * S * 128
        assert ref.tokens.shape == (B, S) and ref.pos.shape == (1,) and ref.split_ws is None
    with pytest.raises(ValueError, match="kv_dtype"):
        KVCache(c, B, CPU, kv_dtype="e5m2")
    model, P = T.make_model(c, CPU, 1)
    assert Generator(model, P, B, CPU).kv.k[0].dtype == torch.bfloat16
    assert Generator(model, P, B, CPU, kv_dtype="fp8").kv.k[0].dtype == torch.uint8


def test_fp8_refuses_split_draft_beams():
    model, P = T.make_model(CFG, CPU, 1)
    with pytest.raises(ValueError, match="split_append"):
        Generator(model, P, B, CPU, split_append=True, kv_dtype="fp8")
    with pytest.raises(ValueError, match="draft"):
        Generator(model, P, B, CPU, draft=(model, P), kv_dtype="fp8")
    gen = Generator(model, P, 4, CPU, kv_dtype="fp8")
    prompt = torch.ones(2, 5, dtype=torch.int32)
    with pytest.raises(ValueError, match="beam"):
        gen.beam_begin(prompt, 2)
    with pytest.raises(ValueError, match="beam"):
        gen.beam_search(prompt, 3, num_beams=2)


def test_prefill_cuts_leave_the_same_cache():
    """prefill(chunk=7), prefill(chunk=64) and token-by-token steps: identical cache bytes and scales below
    the position, and teacher-forced logits that agree."""
    model, P = T.make_model(CFG, CPU, 4)
    Pn = 100
    tok = torch.randint(0, CFG.vocab_size, (B, Pn), generator=torch.Generator().manual_seed(5)).to(torch.int32)
    gens = [Generator(model, P, B, CPU, kv_dtype="fp8") for _ in range(3)]
    gens[0].prefill(tok, chunk=7)
    gens[1].prefill(tok, chunk=64)
    gens[2].prefill(tok[:, :1])
    gens[2].kv.tokens[:, :Pn] = tok
    for _ in range(Pn - 1):
        gens[2].step(sample=False)
    logits = []
    for g in gens:
        assert int(g.kv.pos.item()) == Pn - 1
        logits.append(g.step(sample=False).clone())
    ref = gens[0].kv
    for g in gens[1:]:
        for l in range(CFG.n_layers):
            for a, b in ((g.kv.k[l], ref.k[l]), (g.kv.v[l], ref.v[l])):
                assert torch.equal(a[:, :, :Pn], b[:, :, :Pn]), l
            for a, b in ((g.kv.k_scale[l], ref.k_scale[l]), (g.kv.v_scale[l], ref.v_scale[l])):
                assert torch.equal(a[:, :, :Pn], b[:, :, :Pn]), l
    T.close(logits[1], logits[0])
    T.close(logits[2], logits[0])
    # and close to the bf16 cache's logits: the quantization error of the keys and values, not a bug's
    bf = Generator(model, P, B, CPU)
    bf.prefill(tok, chunk=64)
    T.close(logits[0], bf.step(sample=False), rtol=0.1, atol=0.1)


def test_default_prefill_quantizes_the_forward_rows():
    """The default prefill: the prompt rows attend over unquantized keys in the training forward, and the
    cache receives kv_quantize of the rows a bf16 cache receives."""
    model, P = T.make_model(CFG, CPU, 4)
    tok = torch.randint(0, CFG.vocab_size, (B, 33), generator=torch.Generator().manual_seed(6)).to(torch.int32)
    gen, bf = Generator(model, P, B, CPU, kv_dtype="fp8"), Generator(model, P, B, CPU)
    gen.prefill(tok)
    bf.prefill(tok)
    for l in range(CFG.n_layers):
        for cache, sc, src in ((gen.kv.k[l], gen.kv.k_scale[l], bf.kv.k[l]), (gen.kv.v[l], gen.kv.v_scale[l], bf.kv.v[l])):
            wq, wsc = kern.kv_quantize(src[:, :, :33])
            assert torch.equal(cache[:, :, :33], wq) and torch.equal(sc[:, :, :33], wsc)
            assert bool((cache[:, :, 33:] == 0).all()) and bool((sc[:, :, 33:] == 1).all())


def test_ragged_generate_with_eos():
    """The documented ragged format: int32 [B, max(len) + new], pad_id at and past each row's final length,
    a row that draws the EOS ends with it."""
    model, P = T.make_model(CFG, CPU, 2)
    gen = Generator(model, P, B, CPU, kv_dtype="fp8")
    prompt = torch.randint(0, CFG.vocab_size, (B, 20), generator=torch.Generator().manual_seed(7)).to(torch.int32)
    lens, new = [4, 11, 20], 10
    free = gen.generate(prompt, new, prompt_lens=lens, pad_id=-1)
    assert free.shape == (B, 20 + new) and free.dtype == torch.int32 and gen.lengths.tolist() == [14, 21, 30]
    eos = int(free[1, lens[1] + 3])   # the fourth new token of row 1
    out = gen.generate(prompt, new, prompt_lens=lens, eos_id=eos, pad_id=-1, top_k=0)
    for b, n in enumerate(lens):
        L = int(gen.lengths[b])
        assert torch.equal(out[b, :n], prompt[b, :n]) and bool((out[b, L:] == -1).all())
        assert n < L <= n + new and bool((out[b, :L] >= 0).all())
        body = out[b, n:L].tolist()
        assert eos not in body[:-1] and (body[-1] == eos or L == n + new)
        assert torch.equal(out[b, :L], free[b, :L])   # greedy: the same tokens up to the stop
    assert int(gen.lengths[1]) <= lens[1] + 4
    # sampling with filters runs too, and the seed fixes the draw
    a = gen.generate(prompt, 6, temperature=0.8, seed=3, top_k=20, top_p=0.9, prompt_lens=lens)
    assert torch.equal(a, gen.generate(prompt, 6, temperature=0.8, seed=3, top_k=20, top_p=0.9, prompt_lens=lens))


def test_extend_fp8_cpu():
    """extend appends to a live FP8 cache and leaves the rows one chunked prefill of all tokens leaves."""
    model, P = T.make_model(CFG, CPU, 4)
    tok = torch.randint(0, CFG.vocab_size, (B, 60), generator=torch.Generator().manual_seed(8)).to(torch.int32)
    a, b = Generator(model, P, B, CPU, kv_dtype="fp8"), Generator(model, P, B, CPU, kv_dtype="fp8")
    a.prefill(tok[:, :25], chunk=64)
    la = a.extend(tok[:, 25:], chunk=16, logits=True)
    b.prefill(tok, chunk=64)
    assert int(a.kv.pos.item()) == int(b.kv.pos.item()) == 59
    for l in range(CFG.n_layers):
        assert torch.equal(a.kv.k[l][:, :, :59], b.kv.k[l][:, :, :59])
        assert torch.equal(a.kv.v_scale[l][:, :, :59], b.kv.v_scale[l][:, :, :59])
    assert la.shape == (B, CFG.vocab_size)


def test_generate_cli_kv_dtype(capsys):
    import generate

    assert generate.parse_args([]).kv_dtype == "bf16"
    generate.main(generate.parse_args(["--kv-dtype", "fp8", "--prompt-len", "12", "--max-new-tokens", "4", "--batch",
                                       "2"]))
    rows = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("[generate] seq ")]
    assert len(rows) == 2 and all(len(ln.split(": ", 1)[1].split()) == 16 for ln in rows)
