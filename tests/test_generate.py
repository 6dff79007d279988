"""KV-cache generation on CPU tensors (the torch reference paths), and the device-agnostic
test bodies that tests/test_generate_gpu.py runs again on the HIP kernels.

Yardsticks: a float64 forward of the LM built from the weights the kernels see (bf16
shadow for matmul weights / biases / embeddings, fp32 LayerNorm parameters) and float64
single-query attention.  The decode path may be at most twice as far from fp64 as the
existing full forward is on the same positions (both are bf16 pipelines with the same
rounding points; the factor covers the different summation order)."""
import json
import math
import os

import numpy as np
import pytest
import torch

from jax_distributed_tuts_amd.generation import Generator, KVCache
from jax_distributed_tuts_amd.models.transformer import TransformerConfig, TransformerLM, lm_stage
from jax_distributed_tuts_amd.ops import kernels as kern
from jax_distributed_tuts_amd.utils.flat import FlatParams

CFG = TransformerConfig(vocab_size=512, d_model=128, n_heads=2, d_ff=512, seq_len=128, n_layers=2)
B = 3
CPU = torch.device("cpu")


def log_errors(**kw):
    """Append measured errors to JDT_ORACLE_LOG (how the bounds were checked)."""
    log = os.environ.get("JDT_ORACLE_LOG")
    print(json.dumps(kw))
    if log:
        with open(log, "a") as f:
            f.write(json.dumps({"test": os.environ.get("PYTEST_CURRENT_TEST", "").split(" ")[0], **kw}) + "\n")


def close(a, b, rtol=2e-2, atol=2e-2):
    a, b = a.double().cpu(), b.double().cpu()
    err = (a - b).abs().max().item()
    scale = b.abs().max().item() + 1e-6
    assert err <= atol + rtol * scale, f"max err {err} (scale {scale})"


# ----------------------------------------------------------------------------- fp64 yardsticks
def make_model(cfg, dev, seed=0):
    """A full model whose every parameter (biases and LayerNorm included) is random."""
    model = TransformerLM(cfg)
    P = FlatParams(model.param_specs(), device=dev).init_(seed)
    g = torch.Generator().manual_seed(seed + 100)
    for n in P.names():
        P.p(n).add_((0.05 * torch.randn(P.p(n).shape, generator=g)).to(dev))
    P.sync_shadow()
    return model, P


def lm_logits_fp64(P, cfg, tok):
    """float64 logits [B, S, V] of the LM on ``tok`` [B, S] from the weights the kernels read."""
    ps = {n: (P.p(n) if "/ln" in n or n.startswith("ln_f") else P.s(n)).detach().cpu().double() for n in P.names()}
    tok = tok.cpu().long()
    Bq, S = tok.shape
    d, H = cfg.d_model, cfg.n_heads
    Dh = d // H

    def ln(x, g, b):
        return torch.nn.functional.layer_norm(x, (d,), g, b, eps=cfg.ln_eps)

    x = (ps["embed/wte"][tok] + ps["embed/wpe"][None, :S]).reshape(Bq * S, d)
    for l in range(cfg.n_layers):
        b = f"block_{l}"
        h = ln(x, ps[f"{b}/ln1/scale"], ps[f"{b}/ln1/bias"])
        qkv = h @ ps[f"{b}/attn/qkv/kernel"] + ps[f"{b}/attn/qkv/bias"]
        q, k, v = qkv.view(Bq, S, 3, H, Dh).permute(2, 0, 3, 1, 4)
        sc = (q @ k.transpose(-1, -2)) / math.sqrt(Dh)
        sc = sc.masked_fill(torch.triu(torch.ones(S, S, dtype=torch.bool), 1), float("-inf"))
        o = (torch.softmax(sc, -1) @ v).permute(0, 2, 1, 3).reshape(Bq * S, d)
        x = x + o @ ps[f"{b}/attn/out/kernel"] + ps[f"{b}/attn/out/bias"]
        h2 = ln(x, ps[f"{b}/ln2/scale"], ps[f"{b}/ln2/bias"])
        u = torch.nn.functional.gelu(h2 @ ps[f"{b}/mlp/fc1/kernel"] + ps[f"{b}/mlp/fc1/bias"], approximate="tanh")
        x = x + u @ ps[f"{b}/mlp/fc2/kernel"] + ps[f"{b}/mlp/fc2/bias"]
    hf = ln(x, ps["ln_f/scale"], ps["ln_f/bias"])
    return (hf @ ps["head/kernel"] + ps["head/bias"]).view(Bq, S, cfg.vocab_size)


def full_logits(model, P, tok):
    """The existing forward's logits [B, S, V] (fp64 copy on the CPU)."""
    out, _ = model.forward(P, tok.to(P.device))
    return out.detach().cpu().double().view(tok.shape[0], model.cfg.seq_len, model.cfg.vocab_size)


def attn_decode_fp64(qkv, kc, vc, pos, H):
    """float64 single-query attention of the bf16 inputs: the token's k / v are row ``pos``."""
    Bq, d3 = qkv.shape
    Dh = d3 // 3 // H
    q, k, v = qkv.double().cpu().view(Bq, 3, H, Dh).unbind(1)
    K_ = torch.cat([kc.double().cpu()[:, :, :pos], k[:, :, None]], 2)
    V_ = torch.cat([vc.double().cpu()[:, :, :pos], v[:, :, None]], 2)
    p = torch.softmax(torch.einsum("bhd,bhjd->bhj", q, K_) / math.sqrt(Dh), -1)
    return torch.einsum("bhj,bhjd->bhd", p, V_).reshape(Bq, H * Dh), p


def decode_inputs(Bq, H, S_max=128, seed=0):
    g = torch.Generator().manual_seed(seed)
    bf = lambda *s: torch.randn(*s, generator=g).to(torch.bfloat16)  # noqa: E731
    return bf(Bq, 3 * H * 64), bf(Bq, H, S_max, 64), bf(Bq, H, S_max, 64)


def posw(p, dev):
    return torch.tensor([p], dtype=torch.int32, device=dev)


# ----------------------------------------------------------------------------- shared bodies
def body_needle(dev):
    """One key j carries softmax weight > 1 - 1e-4: o must be v_j.  j at both ends, at the
    64-key seams and at the current token (appended before it is used)."""
    H = 2
    for pos in (64, 127):
        for j in sorted({0, 63, 64, pos}):
            qkv, kc, vc = decode_inputs(B, H, seed=1000 + pos + j)
            q = qkv.float().view(B, 3, H, 64)[:, 0]
            needle = (16.0 * q / q.norm(dim=-1, keepdim=True)).to(torch.bfloat16)
            kc = (kc.float() * 0.05).to(torch.bfloat16)
            new = qkv.clone().view(B, 3, H, 64)
            new[:, 1] = (new[:, 1].float() * 0.05).to(torch.bfloat16)
            if j == pos:
                new[:, 1] = needle
            else:
                kc[:, :, j] = needle
            qkv = new.view(B, -1).contiguous()
            want, p = attn_decode_fp64(qkv, kc, vc, pos, H)
            assert float(p[:, :, j].min()) > 1 - 1e-4
            vj = (qkv.view(B, 3, H, 64)[:, 2] if j == pos else vc[:, :, j]).reshape(B, -1)
            got = kern.attention_decode(qkv.to(dev), kc.to(dev).clone(), vc.to(dev).clone(), posw(pos, dev), H)
            close(got, vj)
            close(got, want)


def body_cache_append(dev):
    H = 2
    for pos in (0, 63, 64, 127):
        qkv, kc, vc = decode_inputs(B, H, seed=7 + pos)
        k2, v2 = kc.to(dev).clone(), vc.to(dev).clone()
        kern.attention_decode(qkv.to(dev), k2, v2, posw(pos, dev), H)
        wk, wv = kc.clone(), vc.clone()
        wk[:, :, pos] = qkv.view(B, 3, H, 64)[:, 1]
        wv[:, :, pos] = qkv.view(B, 3, H, 64)[:, 2]
        assert torch.equal(k2.cpu(), wk) and torch.equal(v2.cpu(), wv)


def body_out_of_range(dev):
    H, S_max = 2, 128
    for pos in (S_max, S_max + 5):
        qkv, kc, vc = decode_inputs(B, H, seed=3)
        k2, v2 = kc.to(dev).clone(), vc.to(dev).clone()
        o = torch.full((B, H * 64), 7.0, dtype=torch.bfloat16, device=dev)
        kern.attention_decode(qkv.to(dev), k2, v2, posw(pos, dev), H, out=o)
        assert torch.equal(k2.cpu(), kc) and torch.equal(v2.cpu(), vc) and bool((o == 7.0).all())
        x = torch.full((B, 64), 7.0, dtype=torch.bfloat16, device=dev)
        tok = torch.zeros(B, S_max, dtype=torch.int32, device=dev)
        kern.embed_decode(tok, vc[0, 0, :16].contiguous().to(dev), kc[0, 0].to(dev), posw(pos, dev), out=x)
        assert bool((x == 7.0).all())
    logits = torch.randn(B, 64).to(torch.bfloat16).to(dev)
    for pos in (S_max - 1, S_max, S_max + 5):
        tok = torch.full((B, S_max), 5, dtype=torch.int32, device=dev)
        pw = posw(pos, dev)
        for t in (0.0, 1.0):
            kern.sample_tokens(logits, tok, pw, temperature=t)
        assert bool((tok == 5).all()) and int(pw.item()) == pos


def body_embed_decode(dev):
    V, S, d = 100, 128, 64
    g = torch.Generator().manual_seed(5)
    wte, wpe = torch.randn(V, d, generator=g).to(torch.bfloat16), torch.randn(S, d, generator=g).to(torch.bfloat16)
    tok = torch.randint(0, V, (B, S), generator=g).to(torch.int32)
    full = kern.embed_fwd(tok.reshape(-1).to(dev), wte.to(dev), wpe.to(dev), S).view(B, S, d)
    for pos in (0, 1, 127):
        got = kern.embed_decode(tok.to(dev), wte.to(dev), wpe.to(dev), posw(pos, dev))
        assert torch.equal(got, full[:, pos])


def _sample(logits, pos, dev, S_max=128, **kw):
    tok = torch.full((logits.shape[0], S_max), -1, dtype=torch.int32, device=dev)
    pw = posw(pos, dev)
    kern.sample_tokens(logits.to(dev), tok, pw, **kw)
    assert int(pw.item()) == pos + 1
    keep = torch.ones(S_max, dtype=torch.bool)
    keep[pos + 1] = False
    assert bool((tok.cpu()[:, keep] == -1).all())   # only column pos + 1 is written
    return tok[:, pos + 1].cpu().long()


def body_sample_greedy(dev):
    g = torch.Generator().manual_seed(11)
    for V in (512, 2048, 1000, 37):    # 16-byte rows, and odd widths (scalar loads, ragged chunks)
        vals = (torch.arange(V) + 0x3000).to(torch.int16).view(torch.bfloat16)   # V distinct bf16 values
        x = torch.stack([vals[torch.randperm(V, generator=g)] for _ in range(5)])
        assert x.float().unique(dim=1).shape[1] == V
        assert torch.equal(_sample(x, 3, dev), x.float().argmax(-1))
    x = torch.zeros(4, 2048)
    x[0, [700, 9, 1999]] = 3.0     # exact ties: the lowest index wins
    x[1, [2047, 256]] = 3.0
    x[2, [255, 256]] = 3.0
    assert _sample(x.to(torch.bfloat16), 0, dev).tolist() == [9, 256, 255, 0]


def body_sample_certain(dev):
    g = torch.Generator().manual_seed(12)
    x = torch.randn(64, 512, generator=g)
    hot = torch.randint(0, 512, (64,), generator=g)
    x[torch.arange(64), hot] = x.max() + 40.0
    x = x.to(torch.bfloat16)
    for t in (0.5, 1.0, 2.0):
        for pos in (0, 1, 64, 126):
            assert torch.equal(_sample(x, pos, dev, temperature=t, seed=3), hot)


def live8(N, V=2048):
    x = torch.full((N, V), -60.0)
    cols = torch.arange(8) * 251 + 17   # spread over the row: several threads' chunks
    x[:, cols] = torch.arange(8).float() * 0.5
    return x.to(torch.bfloat16), cols


def body_sample_distribution(dev):
    """8 live logits: every token's frequency over 8192 rows within 6 sigma of its fp64
    softmax probability (false-fail probability < 1e-8 per bin)."""
    N = 8192
    x, cols = live8(N)
    p = torch.softmax(x[0].double(), -1)
    tok = _sample(x, 5, dev, temperature=1.0, seed=1234)
    assert bool(torch.isin(tok, cols).all())
    for c in cols.tolist():
        pc = float(p[c])
        freq = float((tok == c).double().mean())
        assert abs(freq - pc) <= 6 * math.sqrt(pc * (1 - pc) / N), (c, freq, pc)


def body_sample_deterministic(dev):
    x, _ = live8(256)
    a = _sample(x, 9, dev, temperature=1.0, seed=77)
    assert torch.equal(a, _sample(x, 9, dev, temperature=1.0, seed=77))
    assert not torch.equal(a, _sample(x, 10, dev, temperature=1.0, seed=77))
    assert not torch.equal(a, _sample(x, 9, dev, temperature=1.0, seed=78))
    assert not torch.equal(a, _sample(x, 9, dev, temperature=1.0, seed=77, stream_id=1))


def teacher_forced_errors(dev, cfg, Bq, cases, seed=0):
    """(E_full, E_dec): max |logits - fp64| of the existing forward and of the decode path
    over the decoded positions of ``cases`` = [(P, positions)], true tokens fed."""
    model, P = make_model(cfg, dev, seed)
    tok = torch.randint(0, cfg.vocab_size, (Bq, cfg.seq_len), generator=torch.Generator().manual_seed(seed + 1))
    tok = tok.to(torch.int32)
    F = lm_logits_fp64(P, cfg, tok)
    f = full_logits(model, P, tok)
    gen = Generator(model, P, Bq, dev)
    e_full = e_dec = 0.0
    for Pn, positions in cases:
        gen.prefill(tok[:, :Pn].to(dev))
        gen.kv.tokens.copy_(tok.to(dev))
        assert int(gen.kv.pos.item()) == Pn - 1
        for p in range(Pn - 1, positions[-1] + 1):
            d = gen.step(sample=False).detach().cpu().double()
            assert int(gen.kv.pos.item()) == p + 1
            if p in positions:
                e_full = max(e_full, float((f[:, p] - F[:, p]).abs().max()))
                e_dec = max(e_dec, float((d - F[:, p]).abs().max()))
        assert torch.equal(gen.kv.tokens.cpu(), tok)   # teacher forcing leaves the tokens alone
    return e_full, e_dec


SMALL_CASES = [(1, [1, 2, 3]), (62, [62, 63, 64, 65, 66]), (126, [126, 127])]


def body_teacher_forced(dev, cfg=CFG, Bq=B, cases=SMALL_CASES):
    e_full, e_dec = teacher_forced_errors(dev, cfg, Bq, cases)
    log_errors(name="teacher_forced", device=str(dev), d_model=cfg.d_model, E_full=e_full, E_dec=e_dec)
    assert e_full > 0
    assert e_dec <= 2 * e_full, (e_dec, e_full)


def body_greedy_consistent(dev, capture=True):
    """Every greedily generated token is, in fp64, within 4 E_full of its row's maximum:
    decode is allowed 2 E_full of elementwise error, so d[tok] >= d[j] implies
    F[tok] >= F[j] - 4 E_full."""
    model, P = make_model(CFG, dev, 2)
    Pn, new = 60, 8
    prompt = torch.randint(0, CFG.vocab_size, (B, Pn), generator=torch.Generator().manual_seed(9)).to(torch.int32)
    seq = Generator(model, P, B, dev).generate(prompt.to(dev), new, temperature=0.0, capture=capture).cpu()
    assert seq.shape == (B, Pn + new) and seq.dtype == torch.int32 and torch.equal(seq[:, :Pn], prompt)
    padded = torch.zeros(B, CFG.seq_len, dtype=torch.int32)
    padded[:, :Pn + new] = seq
    F = lm_logits_fp64(P, CFG, padded)[:, :Pn + new]
    f = full_logits(model, P, padded)[:, :Pn + new]
    e_full = float((f - F).abs().max())
    worst = 0.0
    for t in range(Pn, Pn + new):
        row = F[:, t - 1]
        gap = row.max(-1).values - row.gather(1, seq[:, t].long()[:, None])[:, 0]
        worst = max(worst, float(gap.max()))
    log_errors(name="greedy_consistent", device=str(dev), E_full=e_full, worst_gap=worst)
    assert worst <= 4 * e_full, (worst, e_full)


# ----------------------------------------------------------------------------- CPU tests
def test_needle_cpu():
    body_needle(CPU)


def test_cache_append_cpu():
    body_cache_append(CPU)


def test_out_of_range_cpu():
    body_out_of_range(CPU)


def test_embed_decode_cpu():
    body_embed_decode(CPU)


def test_sample_greedy_cpu():
    body_sample_greedy(CPU)


def test_sample_certain_cpu():
    body_sample_certain(CPU)


def test_sample_distribution_cpu():
    body_sample_distribution(CPU)


def test_sample_deterministic_cpu():
    body_sample_deterministic(CPU)


def test_sample_uniform_is_philox():
    """The CPU sampler draws exactly ``philox_uniform(seed, (pos << 32) | stream, row)``: two
    equal logits split at u = 0.5."""
    x = torch.full((64, 16), -60.0)
    x[:, [3, 11]] = 0.0
    tok = _sample(x.to(torch.bfloat16), 6, CPU, temperature=1.0, seed=21, stream_id=2)
    u = kern.philox_uniform(21, (6 << 32) | 2, np.arange(64), 0)
    assert tok.tolist() == [3 if v < 0.5 else 11 for v in u]


def test_attention_decode_composed_head_dim():
    """Head dims other than 64 run the composed torch path: equal to row ``pos`` of attention_fwd."""
    H, Dh, S, pos = 2, 32, 16, 9
    g = torch.Generator().manual_seed(4)
    full = torch.randn(B * S, 3 * H * Dh, generator=g).to(torch.bfloat16)
    o_full, _ = kern.attention_fwd(full, B, S, H)
    v5 = full.view(B, S, 3, H, Dh)
    kc = torch.zeros(B, H, S, Dh, dtype=torch.bfloat16)
    vc = torch.zeros_like(kc)
    kc[:, :, :pos] = v5[:, :pos, 1].permute(0, 2, 1, 3)
    vc[:, :, :pos] = v5[:, :pos, 2].permute(0, 2, 1, 3)
    got = kern.attention_decode(full.view(B, S, -1)[:, pos].contiguous(), kc, vc, posw(pos, CPU), H)
    close(got, o_full.view(B, S, -1)[:, pos], rtol=1e-2, atol=1e-2)


def test_teacher_forced_cpu():
    body_teacher_forced(CPU)


def test_greedy_consistent_cpu():
    body_greedy_consistent(CPU)


def test_api_edges():
    model, P = make_model(CFG, CPU, 1)
    gen = Generator(model, P, B, CPU)
    prompt = torch.randint(0, CFG.vocab_size, (B, 120), generator=torch.Generator().manual_seed(2)).to(torch.int32)
    with pytest.raises(ValueError, match="seq_len"):
        gen.generate(prompt, 9)
    out = gen.generate(prompt, 8, temperature=0.7, seed=5)
    assert out.shape == (B, 128) and out.dtype == torch.int32 and torch.equal(out[:, :120], prompt)
    assert int(out.min()) >= 0 and int(out.max()) < CFG.vocab_size
    assert torch.equal(out, gen.generate(prompt, 8, temperature=0.7, seed=5))       # the seed fixes the draw
    assert not torch.equal(out, gen.generate(prompt, 8, temperature=0.7, seed=6))
    assert gen.generate(prompt[:, :1], 0).shape == (B, 1)
    with pytest.raises(ValueError):
        gen.prefill(prompt[:2])                     # wrong batch
    with pytest.raises(ValueError):
        gen.prefill(prompt.clamp(min=0) + CFG.vocab_size)   # token outside the vocabulary
    kv = KVCache(CFG, B, CPU)
    assert kv.k[0].shape == (B, CFG.n_heads, CFG.seq_len, 64) and kv.tokens.shape == (B, CFG.seq_len)
    assert kv.pos.dtype == torch.int32 and kv.pos.shape == (1,) and len(kv.k) == len(kv.v) == CFG.n_layers
    stage = lm_stage(CFG, 2, 0)
    Ps = FlatParams(stage.param_specs()).init_(0)
    with pytest.raises(ValueError, match="full model"):
        Generator(stage, Ps, B, CPU)
    with pytest.raises(ValueError, match="full model"):
        stage.decode_step(Ps, kv, torch.zeros(B, CFG.d_model, dtype=torch.bfloat16))
