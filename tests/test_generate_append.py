"""Append attention over the KV cache, chunked prefill and ``Generator.extend`` on CPU tensors (the
composed torch paths), and the device-agnostic bodies that tests/test_generate_append_gpu.py runs
again on the HIP kernels (csrc/attn_append.hip, embed_append).

Yardsticks and bounds are those of tests/test_generate.py: float64 attention of the bf16 inputs,
the float64 LM, E_dec <= 2 E_full for teacher-forced logits and a worst greedy gap of 4 E_full.
Kernel shapes: B = 3, H in {2, 8}, a 320-row cache; the model is test_generate_long's CFG_LONG."""
import math

import pytest
import torch

from jax_distributed_tuts_amd.generation import Generator
from jax_distributed_tuts_amd.ops import kernels as kern

from . import test_generate as T
from . import test_generate_long as TL

CFG_LONG, LONG_CASES = TL.CFG_LONG, TL.LONG_CASES
B, CPU = T.B, T.CPU
S_MAX = 320


# ----------------------------------------------------------------------------- helpers
def append_inputs(H, C, seed, Bq=B, S_max=S_MAX):
    """qkv [Bq*C, 3*H*64] (row b*C + i: token i of sequence b) and one layer's caches."""
    g = torch.Generator().manual_seed(seed)
    bf = lambda *s: torch.randn(*s, generator=g).to(torch.bfloat16)  # noqa: E731
    return bf(Bq * C, 3 * H * 64), bf(Bq, H, S_max, 64), bf(Bq, H, S_max, 64)


def posr(ps, dev):
    return torch.tensor(list(ps), dtype=torch.int32, device=dev)


def attn_append_fp64(qkv, kc, vc, p, n, H):
    """float64 attention of the bf16 inputs: tokens 0..n-1 of the chunk are rows p..p+n-1, keys < p
    come from the cache.  Returns (o [B, n, H*64], probabilities [B, H, n, p + n])."""
    Bq = kc.shape[0]
    C = qkv.shape[0] // Bq
    q, k, v = qkv.double().cpu().view(Bq, C, 3, H, 64)[:, :n].permute(2, 0, 3, 1, 4)   # [B, H, n, 64]
    K_ = torch.cat([kc.double().cpu()[:, :, :p], k], 2)
    V_ = torch.cat([vc.double().cpu()[:, :, :p], v], 2)
    s = q @ K_.transpose(-1, -2) / math.sqrt(64)
    s = s.masked_fill(torch.arange(p + n)[None, :] > (p + torch.arange(n))[:, None], float("-inf"))
    pr = torch.softmax(s, -1)
    return (pr @ V_).permute(0, 2, 1, 3).reshape(Bq, n, H * 64), pr


def run_append(dev, qkv, kc, vc, pos, H, C, count=None, o=None):
    """attention_append on device copies: (o, k_cache, v_cache) after the call."""
    k2, v2 = kc.to(dev).clone(), vc.to(dev).clone()
    got = kern.attention_append(qkv.to(dev), k2, v2, pos, H, C, count=count, out=o)
    return got, k2, v2


def chunk_kv(qkv, Bq, C, H):
    """The chunk's k and v in the cache's layout [B, H, C, 64]."""
    v5 = qkv.view(Bq, C, 3, H, 64)
    return v5[:, :, 1].permute(0, 2, 1, 3), v5[:, :, 2].permute(0, 2, 1, 3)


# ----------------------------------------------------------------------------- kernel-level bodies
def body_append_close_to_fp64(dev):
    H = 2
    for p, C in ((0, 1), (0, 65), (63, 17), (65, 128), (200, 64)):
        qkv, kc, vc = append_inputs(H, C, seed=10 * p + C)
        want, _ = attn_append_fp64(qkv, kc, vc, p, C, H)
        got, _, _ = run_append(dev, qkv, kc, vc, T.posw(p, dev), H, C)
        T.close(got.view(B, C, -1), want)


def body_cache_writes(dev):
    """In a 3-layer sandwich exactly rows p..p+n-1 of the middle layer change, and they hold the
    chunk's k / v bit for bit; p and n straddle 64 and 128."""
    H = 2
    for p, n in ((0, 1), (60, 10), (63, 2), (100, 64), (120, 70), (37, 192), (128, 64), (300, 20)):
        qkv, kc, vc = append_inputs(H, n, seed=p + n)
        g = torch.Generator().manual_seed(p)
        layers_k = torch.randn(3, B, H, S_MAX, 64, generator=g).to(torch.bfloat16)
        layers_v = torch.randn(3, B, H, S_MAX, 64, generator=g).to(torch.bfloat16)
        layers_k[1], layers_v[1] = kc, vc
        dk, dv = layers_k.to(dev), layers_v.to(dev)
        kern.attention_append(qkv.to(dev), dk[1], dv[1], T.posw(p, dev), H, n)
        layers_k[1, :, :, p:p + n], layers_v[1, :, :, p:p + n] = chunk_kv(qkv, B, n, H)
        assert torch.equal(dk.cpu(), layers_k) and torch.equal(dv.cpu(), layers_v), (p, n)
    # per row: each sequence its own rows, a count of 0 none
    pos, count, C = [0, 70, 130], [64, 10, 0], 64
    qkv, kc, vc = append_inputs(H, C, seed=5)
    _, k2, v2 = run_append(dev, qkv, kc, vc, posr(pos, dev), H, C, count=posr(count, dev))
    ck, cv = chunk_kv(qkv, B, C, H)
    for b, (p, n) in enumerate(zip(pos, count)):
        kc[b, :, p:p + n], vc[b, :, p:p + n] = ck[b, :, :n], cv[b, :, :n]
    assert torch.equal(k2.cpu(), kc) and torch.equal(v2.cpu(), vc)


def body_out_of_range(dev):
    """p = -1 and p + n = S_max + 1 write nothing: shared, for any row; per row, for the bad row
    alone (the good rows are checked against their solo calls on the GPU)."""
    H, C = 2, 64
    qkv, kc, vc = append_inputs(H, C, seed=3)
    for p in (-1, S_MAX - C + 1, S_MAX):
        o = torch.full((B * C, H * 64), 7.0, dtype=torch.bfloat16, device=dev)
        _, k2, v2 = run_append(dev, qkv, kc, vc, T.posw(p, dev), H, C, o=o)
        assert torch.equal(k2.cpu(), kc) and torch.equal(v2.cpu(), vc) and bool((o == 7.0).all())
    for bad_p, bad_n in ((-1, 5), (S_MAX - 4, 5), (0, C + 1), (0, -1)):
        for b_bad in range(B):
            pos, count = [5, 100, 250], [64, 7, 1]
            pos[b_bad], count[b_bad] = bad_p, bad_n
            o = torch.full((B * C, H * 64), 7.0, dtype=torch.bfloat16, device=dev)
            _, k2, v2 = run_append(dev, qkv, kc, vc, posr(pos, dev), H, C, count=posr(count, dev), o=o)
            o3 = o.view(B, C, -1)
            for b in range(B):
                if b == b_bad:
                    assert torch.equal(k2[b].cpu(), kc[b]) and torch.equal(v2[b].cpu(), vc[b])
                    assert bool((o3[b] == 7.0).all())
                else:
                    want, _ = attn_append_fp64(qkv, kc, vc, pos[b], count[b], H)
                    T.close(o3[b, :count[b]], want[b])
                    assert bool((o3[b, count[b]:] == 7.0).all())


def body_needle(dev):
    """body_needle's construction (needle length 20): for query token i one key j carries softmax
    weight > 1 - 1e-4, so row i of o must be v_j -- j at 0, p - 1, p, the query's own index and a
    64-seam."""
    H, C, p, i = 2, 40, 100, 39
    for j in (0, p - 1, p, p + i, 64, 128):
        qkv, kc, vc = append_inputs(H, C, seed=3000 + j)
        v5 = qkv.clone().view(B, C, 3, H, 64)
        q = v5[:, i, 0].float()
        needle = (20.0 * q / q.norm(dim=-1, keepdim=True)).to(torch.bfloat16)   # [B, H, 64]
        kc = (kc.float() * 0.05).to(torch.bfloat16)
        v5[:, :, 1] = (v5[:, :, 1].float() * 0.05).to(torch.bfloat16)
        if j >= p:
            v5[:, j - p, 1] = needle
        else:
            kc[:, :, j] = needle
        qkv = v5.view(B * C, -1).contiguous()
        want, pr = attn_append_fp64(qkv, kc, vc, p, C, H)
        assert float(pr[:, :, i, j].min()) > 1 - 1e-4
        vj = (v5[:, j - p, 2] if j >= p else vc[:, :, j]).reshape(B, -1)
        got, _, _ = run_append(dev, qkv, kc, vc, T.posw(p, dev), H, C)
        T.close(got.view(B, C, -1)[:, i], vj)
        T.close(got.view(B, C, -1), want)


def body_c1_agrees_with_decode(dev):
    """C = 1 is the decode step's case (another algorithm: not bit for bit)."""
    for H in (2, 8):
        for p in (0, 63, 64, 200, 319):
            qkv, kc, vc = T.decode_inputs(B, H, S_MAX, seed=40 + p)
            got, k2, v2 = run_append(dev, qkv, kc, vc, T.posw(p, dev), H, 1)
            dk, dv = kc.to(dev).clone(), vc.to(dev).clone()
            dec = kern.attention_decode(qkv.to(dev), dk, dv, T.posw(p, dev), H)
            T.close(got, dec)
            assert torch.equal(k2, dk) and torch.equal(v2, dv)


def body_embed_append(dev):
    """Rows are bit-equal to embed_decode at the same positions; uncounted rows and out-of-range
    sequences keep their contents."""
    V, S, d, C = 100, 128, 64, 20
    g = torch.Generator().manual_seed(5)
    wte, wpe = torch.randn(V, d, generator=g).to(torch.bfloat16).to(dev), torch.randn(S, d, generator=g).to(torch.bfloat16).to(dev)
    tok = torch.randint(0, V, (B, S), generator=g).to(torch.int32).to(dev)
    at = lambda p: kern.embed_decode(tok, wte, wpe, T.posw(p, dev))   # noqa: E731
    for p in (0, 1, 100, S - C):
        got = kern.embed_append(tok, wte, wpe, T.posw(p, dev), C).view(B, C, d)
        for i in range(C):
            assert torch.equal(got[:, i], at(p + i))
    pos, count = [0, 50, 120], [20, 3, 0]
    out = torch.full((B * C, d), 7.0, dtype=torch.bfloat16, device=dev)
    got = kern.embed_append(tok, wte, wpe, posr(pos, dev), C, count=posr(count, dev), out=out).view(B, C, d)
    for b, (p, n) in enumerate(zip(pos, count)):
        for i in range(n):
            assert torch.equal(got[b, i], at(p + i)[b])
        assert bool((got[b, n:] == 7.0).all())
    for ps, cs in (([-1], None), ([S - C + 1], None), ([0, -1, S - 2], [20, 3, 3])):
        out = torch.full((B * C, d), 7.0, dtype=torch.bfloat16, device=dev)
        kern.embed_append(tok, wte, wpe, posr(ps, dev), C, count=None if cs is None else posr(cs, dev), out=out)
        keep = out.view(B, C, d)[1:] if cs is not None else out
        assert bool((keep == 7.0).all())
        if cs is not None:
            assert torch.equal(out.view(B, C, d)[0, 0], at(0)[0])


# ----------------------------------------------------------------------------- model-level bodies
def lm_setup(dev, seed=0):
    """(model, P, true tokens [B, 320], fp64 logits, the existing forward's logits)."""
    cfg = CFG_LONG
    model, P = T.make_model(cfg, dev, seed)
    tok = torch.randint(0, cfg.vocab_size, (B, cfg.seq_len), generator=torch.Generator().manual_seed(seed + 1))
    tok = tok.to(torch.int32)
    return model, P, tok, T.lm_logits_fp64(P, cfg, tok), T.full_logits(model, P, tok)


_LM: dict = {}


def lm_shared(dev):
    """One model and its references per device, shared by the tests (never modified)."""
    key = str(dev)
    if key not in _LM:
        _LM[key] = lm_setup(dev)
    return _LM[key]


def body_teacher_forced_chunked(dev, Pn, chunk):
    """prefill(chunk=) then teacher-forced steps over the positions of LONG_CASES that follow P:
    E_dec <= 2 E_full (teacher_forced_errors' bound and yardsticks).  After the prefill the
    position, the tokens and the cache rows < P - 1 are the existing prefill's."""
    model, P, tok, F, f = lm_shared(dev)
    gen = Generator(model, P, B, dev)
    gen.prefill(tok[:, :Pn].to(dev), chunk=chunk)
    assert int(gen.kv.pos.item()) == Pn - 1 and gen.prefill_rows == 0 and not gen.kv.per_row
    ref = Generator(model, P, B, dev)
    ref.prefill(tok[:, :Pn].to(dev))
    assert torch.equal(gen.kv.tokens, ref.kv.tokens)
    for l in range(CFG_LONG.n_layers):
        if Pn > 1:
            T.close(gen.kv.k[l][:, :, :Pn - 1], ref.kv.k[l][:, :, :Pn - 1])
            T.close(gen.kv.v[l][:, :, :Pn - 1], ref.kv.v[l][:, :, :Pn - 1])
    gen.kv.tokens.copy_(tok.to(dev))
    positions = [p for _, ps in LONG_CASES for p in ps if p >= Pn - 1]
    e_full = e_dec = 0.0
    for p in range(Pn - 1, positions[-1] + 1):
        d = gen.step(sample=False)
        if p in positions:
            e_full = max(e_full, float((f[:, p] - F[:, p]).abs().max()))
            e_dec = max(e_dec, float((d.detach().cpu().double() - F[:, p]).abs().max()))
    assert int(gen.kv.pos.item()) == positions[-1] + 1
    T.log_errors(name="teacher_forced_chunked", device=str(dev), P=Pn, chunk=chunk, E_full=e_full, E_dec=e_dec)
    assert e_full > 0
    assert e_dec <= 2 * e_full, (e_dec, e_full)


def body_extend_logits(dev):
    """Prefill 100 tokens, extend by 70 true tokens, then by 150 more in chunks of 64: each returned
    row is within 2 E_full of the fp64 logits at its position and pos advances by exactly n."""
    model, P, tok, F, f = lm_shared(dev)
    gen = Generator(model, P, B, dev)
    gen.prefill(tok[:, :100].to(dev), chunk=64)
    got1 = gen.extend(tok[:, 100:170].to(dev), logits=True)
    assert int(gen.kv.pos.item()) == 169 and got1.shape == (B, CFG_LONG.vocab_size)
    got2 = gen.extend(tok[:, 170:320].to(dev), chunk=64, logits=True)
    assert int(gen.kv.pos.item()) == 319 and torch.equal(gen.kv.tokens.cpu(), tok)
    assert gen.extend(tok[:, :0].to(dev)) is None and int(gen.kv.pos.item()) == 319
    e_full = max(float((f[:, p] - F[:, p]).abs().max()) for p in (168, 318))
    e_ext = max(float((g.detach().cpu().double() - F[:, p]).abs().max()) for g, p in ((got1, 168), (got2, 318)))
    T.log_errors(name="extend_logits", device=str(dev), E_full=e_full, E_ext=e_ext)
    assert e_full > 0
    assert e_ext <= 2 * e_full, (e_ext, e_full)
    # the last token is still unprocessed: a decode step continues from it
    d = gen.step(sample=False).detach().cpu().double()
    e319 = float((f[:, 319] - F[:, 319]).abs().max())
    assert float((d - F[:, 319]).abs().max()) <= 2 * max(e_full, e319)


def body_ragged(dev):
    """prefill(lens, chunk=64), a per-row extend that moves each row by its own count, then greedy
    steps that meet body_greedy_consistent_long's 4 E_full gap bound."""
    cfg = CFG_LONG
    model, P, tok, _, _ = lm_shared(dev)
    gen = Generator(model, P, B, dev)
    lens, more, new = [5, 130, 200], [0, 3, 64], 8
    gen.prefill(tok[:, :200].to(dev), torch.tensor(lens), chunk=64)
    assert gen.kv.per_row and gen.kv.pos_rows.tolist() == [n - 1 for n in lens] and gen.prefill_rows == 0
    assert gen.kv.end.tolist() == [cfg.seq_len] * B
    ext = torch.zeros(B, 64, dtype=torch.int32)
    for b, (n, m) in enumerate(zip(lens, more)):
        ext[b, :m] = tok[b, n:n + m]
    ext[0, :] = 77   # padding past a row's count is ignored
    logits = gen.extend(ext.to(dev), torch.tensor(more), chunk=64, logits=True)
    total = [n + m for n, m in zip(lens, more)]
    assert gen.kv.pos_rows.tolist() == [n - 1 for n in total] and logits.shape == (B, cfg.vocab_size)
    for b, n in enumerate(total):
        assert torch.equal(gen.kv.tokens[b, :n].cpu(), tok[b, :n]) and bool((gen.kv.tokens[b, n:] == 0).all())
    for _ in range(new):
        gen.step()
    assert gen.kv.pos_rows.tolist() == [n - 1 + new for n in total]
    seq = gen.kv.tokens.cpu()
    F = T.lm_logits_fp64(P, cfg, seq)
    f = T.full_logits(model, P, seq)
    e_full = worst = 0.0
    for b, n in enumerate(total):
        assert torch.equal(seq[b, :n], tok[b, :n])
        e_full = max(e_full, float((f[b, :n + new] - F[b, :n + new]).abs().max()))
        for t in range(n, n + new):
            worst = max(worst, float(F[b, t - 1].max() - F[b, t - 1, seq[b, t].long()]))
    T.log_errors(name="ragged_append", device=str(dev), E_full=e_full, worst_gap=worst)
    assert worst <= 4 * e_full, (worst, e_full)


def body_greedy_chunked(dev, capture):
    """body_greedy_consistent_long with generate(prefill_chunk=64); returns (generator, tokens)."""
    cfg = CFG_LONG
    model, P = T.make_model(cfg, dev, 2)
    Pn, new = 250, 12
    prompt = torch.randint(0, cfg.vocab_size, (B, Pn), generator=torch.Generator().manual_seed(9)).to(torch.int32)
    gen = Generator(model, P, B, dev)
    seq = gen.generate(prompt.to(dev), new, temperature=0.0, capture=capture, prefill_chunk=64).cpu()
    assert gen.prefill_rows == 0
    assert seq.shape == (B, Pn + new) and seq.dtype == torch.int32 and torch.equal(seq[:, :Pn], prompt)
    padded = torch.zeros(B, cfg.seq_len, dtype=torch.int32)
    padded[:, :Pn + new] = seq
    F = T.lm_logits_fp64(P, cfg, padded)[:, :Pn + new]
    f = T.full_logits(model, P, padded)[:, :Pn + new]
    e_full = float((f - F).abs().max())
    worst = 0.0
    for t in range(Pn, Pn + new):
        row = F[:, t - 1]
        gap = row.max(-1).values - row.gather(1, seq[:, t].long()[:, None])[:, 0]
        worst = max(worst, float(gap.max()))
    T.log_errors(name="greedy_chunked", device=str(dev), capture=capture, E_full=e_full, worst_gap=worst)
    assert worst <= 4 * e_full, (worst, e_full)
    return gen, seq


def body_edges(dev):
    cfg = CFG_LONG
    model, P, tok, _, _ = lm_shared(dev)
    gen = Generator(model, P, B, dev)
    t = tok.to(dev)
    with pytest.raises(ValueError, match="live cache"):
        gen.extend(t[:, :4])
    for bad in (0, -3):
        with pytest.raises(ValueError, match="chunk"):
            gen.prefill(t[:, :10], chunk=bad)
    gen.prefill(t[:, :300], chunk=100)
    with pytest.raises(ValueError, match="chunk"):
        gen.extend(t[:, 300:304], chunk=0)
    with pytest.raises(ValueError, match="chunk"):
        gen.advance(1, chunk=0)
    with pytest.raises(ValueError, match="seq_len"):
        gen.extend(t[:, :21])               # 299 + 21 = 320 > 319
    with pytest.raises(ValueError, match="per-row"):
        gen.extend(t[:, 300:304], torch.tensor([1, 2, 3]))
    assert int(gen.kv.pos.item()) == 299 and torch.equal(gen.kv.tokens[:, :300], t[:, :300])
    gen.extend(t[:, 300:320])               # up to the last row of the cache
    assert int(gen.kv.pos.item()) == 319
    gen.prefill(t[:, :200], torch.tensor([5, 130, 200]), chunk=64)
    with pytest.raises(ValueError, match="seq_len"):
        gen.extend(t[:, :121], torch.tensor([0, 3, 121]))   # 199 + 120 = 319 is the limit
    with pytest.raises(ValueError, match="lens"):
        gen.extend(t[:, :4], torch.tensor([0, 3, 5]))
    assert gen.kv.pos_rows.tolist() == [4, 129, 199]
    TL.body_prefill_rows(dev)               # prefill(chunk=None) is today's path


# ----------------------------------------------------------------------------- CPU tests
def test_append_close_to_fp64_cpu():
    body_append_close_to_fp64(CPU)


def test_cache_writes_cpu():
    body_cache_writes(CPU)


def test_out_of_range_cpu():
    body_out_of_range(CPU)


def test_needle_cpu():
    body_needle(CPU)


def test_c1_agrees_with_decode_cpu():
    body_c1_agrees_with_decode(CPU)


def test_embed_append_cpu():
    body_embed_append(CPU)


def test_append_composed_head_dim():
    """Head dims other than 64 run the composed torch path: rows p..p+C-1 of attention_fwd."""
    H, Dh, S, p, C = 2, 32, 24, 9, 7
    full = torch.randn(B * S, 3 * H * Dh, generator=torch.Generator().manual_seed(4)).to(torch.bfloat16)
    o_full, _ = kern.attention_fwd(full, B, S, H)
    v5 = full.view(B, S, 3, H, Dh)
    kc = torch.zeros(B, H, S, Dh, dtype=torch.bfloat16)
    vc = torch.zeros_like(kc)
    kc[:, :, :p], vc[:, :, :p] = v5[:, :p, 1].permute(0, 2, 1, 3), v5[:, :p, 2].permute(0, 2, 1, 3)
    chunk = full.view(B, S, -1)[:, p:p + C].reshape(B * C, -1).contiguous()
    got = kern.attention_append(chunk, kc, vc, T.posw(p, CPU), H, C)
    T.close(got.view(B, C, -1), o_full.view(B, S, -1)[:, p:p + C], rtol=1e-2, atol=1e-2)
    assert torch.equal(kc[:, :, :p + C], v5[:, :p + C, 1].permute(0, 2, 1, 3))


@pytest.mark.parametrize("chunk", [64, 100])
@pytest.mark.parametrize("Pn", [1, 2, 65, 250])
def test_teacher_forced_chunked_cpu(Pn, chunk):
    body_teacher_forced_chunked(CPU, Pn, chunk)


def test_extend_logits_cpu():
    body_extend_logits(CPU)


def test_ragged_cpu():
    body_ragged(CPU)


def test_greedy_chunked_cpu():
    body_greedy_chunked(CPU, False)


def test_edges_cpu():
    body_edges(CPU)


def test_generate_cli_prefill_chunk(capsys):
    """generate.py --prefill-chunk 64: 140 prompt tokens + 8 new ones per row in a 160-row cache."""
    import generate

    generate.main(generate.parse_args(["--seq-len", "160", "--prompt-len", "140", "--prefill-chunk", "64",
                                       "--max-new-tokens", "8", "--batch", "2"]))
    rows = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("[generate] seq ")]
    assert len(rows) == 2
    for ln in rows:
        ids = ln.split(": ", 1)[1].split()
        assert len(ids) == 148 and all(0 <= int(t) < 2048 for t in ids)
    assert generate.parse_args([]).prefill_chunk is None
