"""Ragged prompts (per-row positions), top-k / top-p and EOS stopping on CPU tensors (the
torch reference paths), and the device-agnostic bodies tests/test_generate_rows_gpu.py runs
again on the HIP kernels.

Yardsticks: the shared-position kernels (a row at the shared position must give the same
bits), the kept set of the top-k / top-p definition evaluated in float64 from the bf16
logits, the float64 LM of tests/test_generate.py, and the uniform ``generate`` (the rows of
a decode step do not interact and the Philox counter depends on row, position and seed
only, so a ragged batch must reproduce it bit for bit)."""
import math

import pytest
import torch

from jax_distributed_tuts_amd.generation import Generator, KVCache
from jax_distributed_tuts_amd.ops import kernels as kern

from . import test_generate as T

CFG, CPU = T.CFG, T.CPU
S_MAX = 128


def posr(ps, dev):
    return torch.tensor(list(ps), dtype=torch.int32, device=dev)


# ----------------------------------------------------------------------------- kernels, per row
def _attn_rows_case(dev, H, pos, seed):
    """Per-row attention at ``pos`` against the shared-position kernel at each pos[b]; rows out
    of range must leave their cache rows and their ``out`` row (sentinel 7) alone."""
    Bq = len(pos)
    qkv, kc, vc = T.decode_inputs(Bq, H, seed=seed)
    k2, v2 = kc.to(dev).clone(), vc.to(dev).clone()
    out = torch.full((Bq, H * 64), 7.0, dtype=torch.bfloat16, device=dev)
    kern.attention_decode(qkv.to(dev), k2, v2, posr(pos, dev), H, out=out)
    wk, wv = kc.clone(), vc.clone()
    for b, p in enumerate(pos):
        if not 0 <= p < S_MAX:
            assert bool((out[b] == 7.0).all())
            continue
        ref = kern.attention_decode(qkv.to(dev), kc.to(dev).clone(), vc.to(dev).clone(), T.posw(p, dev), H)
        assert torch.equal(out[b], ref[b]), (H, b, p)
        wk[b, :, p] = qkv.view(Bq, 3, H, 64)[b, 1]
        wv[b, :, p] = qkv.view(Bq, 3, H, 64)[b, 2]
    assert torch.equal(k2.cpu(), wk) and torch.equal(v2.cpu(), wv)   # exactly row pos[b] of row b
    return qkv, kc, vc, out


def body_attn_rows(dev):
    for H in (2, 8):
        qkv, kc, vc, out = _attn_rows_case(dev, H, [0, 31, 64, 127], seed=40 + H)   # both ends, the 32-key seams
        if H == 2:
            for b, p in enumerate([0, 31, 64, 127]):
                want, _ = T.attn_decode_fp64(qkv[b:b + 1], kc[b:b + 1], vc[b:b + 1], p, H)
                T.close(out[b:b + 1], want)
        _attn_rows_case(dev, H, [5, 128, 17, 200], seed=50 + H)


def body_embed_rows(dev):
    V, S, d = 100, 128, 64
    g = torch.Generator().manual_seed(5)
    wte, wpe = torch.randn(V, d, generator=g).to(torch.bfloat16), torch.randn(S, d, generator=g).to(torch.bfloat16)
    tok = torch.randint(0, V, (3, S), generator=g).to(torch.int32)
    full = kern.embed_fwd(tok.reshape(-1).to(dev), wte.to(dev), wpe.to(dev), S).view(3, S, d)
    pos = [0, 1, 127]
    got = kern.embed_decode(tok.to(dev), wte.to(dev), wpe.to(dev), posr(pos, dev))
    for b, p in enumerate(pos):
        assert torch.equal(got[b], full[b, p])
    for pos in ([1, 128, 127], [-1, 5, 300]):
        x = torch.full((3, d), 7.0, dtype=torch.bfloat16, device=dev)
        kern.embed_decode(tok.to(dev), wte.to(dev), wpe.to(dev), posr(pos, dev), out=x)
        for b, p in enumerate(pos):
            assert torch.equal(x[b], full[b, p]) if 0 <= p < S else bool((x[b] == 7.0).all())


def _hot_rows(n, hot):
    x = torch.randn(n, 512, generator=torch.Generator().manual_seed(12))
    x[torch.arange(n), torch.tensor(hot)] = x.max() + 40.0
    return x.to(torch.bfloat16)


def body_sample_state(dev):
    pos, end, hot = [3, 60, 126, 127], [128, 61, 128, 128], [7, 9, 13, 11]
    x = _hot_rows(4, hot).to(dev)
    for t in (0.0, 1.0):
        tok = torch.full((4, S_MAX), -1, dtype=torch.int32, device=dev)
        pw, ew = posr(pos, dev), posr(end, dev)
        kern.sample_tokens(x, tok, pw, end=ew, temperature=t, seed=3)
        want = torch.full((4, S_MAX), -1, dtype=torch.int32)
        want[0, 4], want[2, 127] = hot[0], hot[2]   # row 1 is at its end, row 3 at the cache end
        assert torch.equal(tok.cpu(), want)
        assert pw.tolist() == [4, 60, 127, 127] and ew.tolist() == end
    # a row that draws eos_id is finished: end = its length; the next call skips it
    tok = torch.full((4, S_MAX), -1, dtype=torch.int32, device=dev)
    pw, ew = posr(pos, dev), posr(end, dev)
    kern.sample_tokens(x, tok, pw, end=ew, eos_id=hot[0], temperature=1.0, seed=3)
    assert torch.equal(tok.cpu(), want) and pw.tolist() == [4, 60, 127, 127]
    assert ew.tolist() == [5, 61, 128, 128]    # pos_old + 2 for row 0 only (row 2 drew another token)
    kern.sample_tokens(x, tok, pw, end=ew, eos_id=hot[0], temperature=1.0, seed=3)
    assert torch.equal(tok.cpu(), want) and pw.tolist() == [4, 60, 127, 127] and ew.tolist() == [5, 61, 128, 128]


def _sample_rows(logits, pos, dev, **kw):
    """Per-row sampler on fresh tokens: every row must write column pos[b] + 1 only and advance."""
    n = logits.shape[0]
    tok = torch.full((n, S_MAX), -1, dtype=torch.int32, device=dev)
    pw = posr(pos, dev)
    ew = torch.full((n,), S_MAX, dtype=torch.int32, device=dev)
    kern.sample_tokens(logits.to(dev), tok, pw, end=ew, **kw)
    col = torch.tensor(list(pos)) + 1
    assert torch.equal(pw.cpu().long(), col) and bool((ew == S_MAX).all())
    tok = tok.cpu()
    got = tok[torch.arange(n), col].long()
    tok[torch.arange(n), col] = -1
    assert bool((tok == -1).all())
    return got


def draw(x, pos, dev, rows, **kw):
    """One draw per row at the shared position ``pos``: the shared or the per-row sampler."""
    return _sample_rows(x, [pos] * x.shape[0], dev, **kw) if rows else T._sample(x, pos, dev, **kw)


def body_draw_identity(dev):
    x, _ = T.live8(256)
    a9 = T._sample(x, 9, dev, temperature=1.0, seed=77)
    a10 = T._sample(x, 10, dev, temperature=1.0, seed=77)
    assert torch.equal(_sample_rows(x, [9] * 256, dev, temperature=1.0, seed=77, top_k=0, top_p=1.0), a9)
    mixed = _sample_rows(x, [9, 10] * 128, dev, temperature=1.0, seed=77)
    assert torch.equal(mixed[0::2], a9[0::2]) and torch.equal(mixed[1::2], a10[1::2])
    assert not torch.equal(a9, a10)


# ----------------------------------------------------------------------------- top-k / top-p
def body_topk_argmax(dev, rows):
    g = torch.Generator().manual_seed(11)
    for V in (512, 2048, 1000, 37):
        vals = (torch.arange(V) + 0x3000).to(torch.int16).view(torch.bfloat16)   # V distinct bf16 values
        x = torch.stack([vals[torch.randperm(V, generator=g)] for _ in range(5)])
        assert torch.equal(draw(x, 3, dev, rows, temperature=1.0, seed=5, top_k=1), x.float().argmax(-1))


def _check_freq(tok, cols, probs, N):
    """Only ``cols`` occur, each within 6 sigma of its probability (false fail < 1e-8 per bin)."""
    assert bool(torch.isin(tok, torch.tensor(cols)).all()), sorted(set(tok.tolist()) - set(cols))
    for c, pc in zip(cols, probs):
        freq = float((tok == c).double().mean())
        assert freq > 0 and abs(freq - pc) <= 6 * math.sqrt(pc * (1 - pc) / N), (c, freq, pc)


def body_topk_ties(dev, rows):
    """Three equal logits at the top and top_k = 2: the tie at the threshold is kept whole."""
    N = 8192
    x = torch.full((N, 1000), -60.0)
    x[:, [5, 300, 900]] = 2.0
    tok = draw(x.to(torch.bfloat16), 5, dev, rows, temperature=1.0, seed=99, top_k=2)
    _check_freq(tok, [5, 300, 900], [1 / 3] * 3, N)


def body_filter_distribution(dev, rows):
    """live8 at T = 1: top-k, top-p, and k before p over the renormalised set."""
    N = 8192
    x, cols = T.live8(N)
    order = torch.argsort(x[0, cols].double(), descending=True)
    cols = cols[order].tolist()                       # descending logits
    p = torch.softmax(x[0].double(), -1)[cols]        # fp64 from the bf16 values
    cum = torch.cumsum(p, 0)
    assert torch.allclose(cum, torch.tensor([0.4008, 0.6439, 0.7914, 0.8808, 0.9350, 0.9679, 0.9879, 1.0],
                                            dtype=torch.float64), atol=1e-4)
    cum4 = torch.cumsum(p[:4] / p[:4].sum(), 0)       # 0.4551, 0.7311, 0.8985, 1
    for thr, masses in ((0.7, cum), (0.8, cum), (0.8, cum4)):
        assert float((masses - thr).abs().min()) > 1e-3
    assert cum[1] < 0.7 <= cum[2] and cum[2] < 0.8 <= cum[3] and cum4[1] < 0.8 <= cum4[2]
    cases = [(dict(top_k=3), 3), (dict(top_p=0.7), 3), (dict(top_k=4, top_p=0.8), 3), (dict(top_p=0.8), 4)]
    for i, (kw, n) in enumerate(cases):
        tok = draw(x, 5, dev, rows, temperature=1.0, seed=1234 + i, **kw)
        _check_freq(tok, cols[:n], (p[:n] / p[:n].sum()).tolist(), N)


def kept_fp64(x, top_k, top_p, margin=1e-4):
    """(kept [V] bool, near): the kept set of one row of logits from the definition in float64
    at T = 1, and whether a cumulative mass lies within ``margin`` of top_p (fp32 sums may then
    fall on either side)."""
    x = x.double()
    V = x.numel()
    w = torch.exp(x - x.max())
    keep = torch.ones(V, dtype=torch.bool)
    if 0 < top_k < V:
        keep = x >= torch.sort(x, descending=True).values[top_k - 1]
    near = False
    if top_p < 1.0:
        vals = torch.unique(x[keep]).flip(0)                                  # descending
        mass = torch.stack([w[keep & (x >= v)].sum() for v in vals]) / w[keep].sum()
        near = bool(((mass - top_p).abs() < margin).any())
        keep = keep & (x >= vals[int((mass >= top_p).nonzero()[0])])
    return keep, near


def body_filter_random(dev, rows):
    N, draws = 256, 64
    for V, top_p in ((37, 0.5), (37, 0.9), (512, 0.5), (37, 1.0), (512, 1.0)):
        for top_k in (0, 7):
            if top_k == 0 and top_p == 1.0:
                continue
            x = (2 * torch.randn(N, V, generator=torch.Generator().manual_seed(31))).to(torch.bfloat16)
            kept, near = zip(*(kept_fp64(x[i], top_k, top_p) for i in range(N)))
            kept, ok = torch.stack(kept), ~torch.tensor(near)
            assert float((~ok).double().mean()) <= 0.05, (V, top_p, top_k, int((~ok).sum()))
            if top_p == 1.0:
                assert bool(ok.all())   # the top-k threshold alone is exact
            toks = torch.stack([draw(x, pos, dev, rows, temperature=1.0, seed=8, top_k=top_k, top_p=top_p)
                                for pos in range(draws)], 1)   # [N, draws]
            inside = kept.gather(1, toks)
            assert bool(inside[ok].all()), (V, top_p, top_k, int((~inside[ok]).sum()))
            assert bool((toks != x.float().argmax(-1)[:, None]).any())   # it does sample, not only argmax


def body_filter_deterministic(dev, rows):
    x, _ = T.live8(256)
    kw = dict(temperature=1.0, top_k=3, top_p=0.9)
    a = draw(x, 9, dev, rows, seed=77, **kw)
    assert torch.equal(a, draw(x, 9, dev, rows, seed=77, **kw))
    assert not torch.equal(a, draw(x, 10, dev, rows, seed=77, **kw))
    assert not torch.equal(a, draw(x, 9, dev, rows, seed=78, **kw))
    assert not torch.equal(a, draw(x, 9, dev, rows, seed=77, stream_id=1, **kw))


# ----------------------------------------------------------------------------- end to end
LENS, NEW = [1, 30, 62, 122], 6   # the rows cross key 32, key 64 and end exactly at index 127
SETTINGS = [dict(temperature=0.0), dict(temperature=0.8, seed=11, top_k=20, top_p=0.9)]


def ragged_prompt(lens, seed=4):
    prompt = torch.randint(0, CFG.vocab_size, (len(lens), max(lens)), generator=torch.Generator().manual_seed(seed))
    return prompt.to(torch.int32)


def body_ragged_equals_uniform(dev, capture=False):
    """Row b of the ragged batch against the uniform ``generate`` of a batch in which every
    prompt has length len_b and row b holds the same prompt: bit-equal tokens."""
    model, P = T.make_model(CFG, dev, 3)
    gen = Generator(model, P, len(LENS), dev)
    prompt = ragged_prompt(LENS).to(dev)
    lens = torch.tensor(LENS)
    for kw in SETTINGS:
        ragged = gen.generate(prompt, NEW, capture=capture, prompt_lens=lens, **kw)
        assert ragged.shape == (len(LENS), max(LENS) + NEW) and ragged.dtype == torch.int32
        assert gen.lengths.tolist() == [n + NEW for n in LENS] and gen.lengths.dtype == torch.int32
        for b, n in enumerate(LENS):
            uni = gen.generate(prompt[:, :n], NEW, capture=False, **kw)
            assert torch.equal(ragged[b, :n + NEW], uni[b]), (kw, b, ragged[b, n:n + NEW].tolist(), uni[b, n:].tolist())
            assert torch.equal(ragged[b, :n], prompt[b, :n]) and bool((ragged[b, n + NEW:] == 0).all())
        if capture:
            eager = gen.generate(prompt, NEW, capture=False, prompt_lens=lens, **kw)
            assert torch.equal(ragged, eager)
            n_graphs = len(gen._graphs)
            assert torch.equal(gen.generate(prompt, NEW, capture=True, prompt_lens=lens, **kw), eager)
            assert len(gen._graphs) == n_graphs and all(g is not None for g, _ in gen._graphs.values())
    return gen


def body_teacher_forced_ragged(dev):
    """E_dec <= 2 E_full over the decoded positions of every row (the yardstick and the factor
    of test_generate.body_teacher_forced), with ragged prompt lengths."""
    model, P = T.make_model(CFG, dev, 0)
    Bq = len(LENS)
    tok = torch.randint(0, CFG.vocab_size, (Bq, CFG.seq_len), generator=torch.Generator().manual_seed(1))
    tok = tok.to(torch.int32)
    F = T.lm_logits_fp64(P, CFG, tok)   # causal: row b's logits at p depend on its own tokens <= p only
    f = T.full_logits(model, P, tok)
    gen = Generator(model, P, Bq, dev)
    gen.prefill(tok[:, :max(LENS)].to(dev), torch.tensor(LENS))
    assert gen.kv.per_row and gen.kv.pos_rows.tolist() == [n - 1 for n in LENS]
    gen.kv.tokens.copy_(tok.to(dev))
    e_full = e_dec = 0.0
    for s in range(NEW):
        d = gen.step(sample=False).detach().cpu().double()
        for b, n in enumerate(LENS):
            p = n - 1 + s
            e_full = max(e_full, float((f[b, p] - F[b, p]).abs().max()))
            e_dec = max(e_dec, float((d[b] - F[b, p]).abs().max()))
    assert gen.kv.pos_rows.tolist() == [n - 1 + NEW for n in LENS] and torch.equal(gen.kv.tokens.cpu(), tok)
    T.log_errors(name="teacher_forced_ragged", device=str(dev), E_full=e_full, E_dec=e_dec)
    assert e_full > 0
    assert e_dec <= 2 * e_full, (e_dec, e_full)


def body_eos(dev, capture=False):
    """Greedy decoding; eos_id is the token one row emits at its third new step (taken from a
    run without eos_id).  That row stops there, the others are untouched, and a finished
    row's further steps change nothing."""
    model, P = T.make_model(CFG, dev, 2)
    lens, new, pad = [5, 20, 40, 60], 8, -1
    gen = Generator(model, P, len(lens), dev)
    prompt = ragged_prompt(lens, seed=9).to(dev)
    first = gen.generate(prompt, new, capture=capture, prompt_lens=torch.tensor(lens), pad_id=pad).cpu()
    assert gen.lengths.tolist() == [n + new for n in lens]
    # a row whose third new token is new to it and that no other row emits
    pick = [r for r, n in enumerate(lens)
            if first[r, n + 2] not in first[r, n:n + 2]
            and all(first[r, n + 2] not in first[b, m:m + new] for b, m in enumerate(lens) if b != r)]
    assert pick, "no row emits a token at its third step that is unique to it: choose other seeds"
    r = pick[0]
    eos = int(first[r, lens[r] + 2])
    out = gen.generate(prompt, new, capture=capture, prompt_lens=torch.tensor(lens), eos_id=eos, pad_id=pad).cpu()
    want_len = [n + new for n in lens]
    want_len[r] = lens[r] + 3
    assert gen.lengths.tolist() == want_len
    assert torch.equal(out[r, :want_len[r]], first[r, :want_len[r]]) and bool((out[r, want_len[r]:] == pad).all())
    for b in range(len(lens)):
        if b != r:
            assert torch.equal(out[b], first[b])
    # row r's steps since it finished were post-finish steps: one more changes nothing of row r.
    # That step is the first post-finish step of the rows that ran to their end (it caches their
    # last token), so a second one changes nothing at all.
    kv = gen.kv
    state = lambda: [kv.tokens, kv.pos_rows, kv.end] + kv.k + kv.v  # noqa: E731
    assert int(kv.end[r]) == want_len[r] and int(kv.pos_rows[r]) == want_len[r] - 1
    snap = [t[r].clone() for t in state()]
    gen.step()
    for a, b in zip(snap, state()):
        assert torch.equal(a, b[r])
    snap = [t.clone() for t in state()]
    gen.step()
    for a, b in zip(snap, state()):
        assert torch.equal(a, b)


def body_eos_early_stop(dev):
    """Once every row has finished the loop ends at the next 16-step check instead of running
    all max_new_tokens steps; the result is that of the full run.  B = 1: the per-row state
    of a single sequence."""
    model, P = T.make_model(CFG, dev, 2)
    gen = Generator(model, P, 1, dev)
    prompt = ragged_prompt([20], seed=9).to(dev)
    first = gen.generate(prompt, 3, capture=False, prompt_lens=torch.tensor([20])).cpu()
    eos = int(first[0, 22])
    assert eos not in first[0, 20:22]
    steps, real = [0], gen.step

    def counted(*a, **kw):
        steps[0] += 1
        return real(*a, **kw)

    gen.step = counted
    out = gen.generate(prompt, 40, capture=False, eos_id=eos, pad_id=-1).cpu()
    assert steps[0] == 16 and out.shape == (1, 60) and gen.lengths.tolist() == [23]
    assert torch.equal(out[0, :23], first[0]) and bool((out[0, 23:] == -1).all())


# ----------------------------------------------------------------------------- CPU tests
def test_attn_rows_cpu():
    body_attn_rows(CPU)


def test_embed_rows_cpu():
    body_embed_rows(CPU)


def test_sample_state_cpu():
    body_sample_state(CPU)


def test_draw_identity_cpu():
    body_draw_identity(CPU)


ROWS = pytest.mark.parametrize("rows", [False, True], ids=["shared", "rows"])


@ROWS
def test_topk_argmax_cpu(rows):
    body_topk_argmax(CPU, rows)


@ROWS
def test_topk_ties_cpu(rows):
    body_topk_ties(CPU, rows)


@ROWS
def test_filter_distribution_cpu(rows):
    body_filter_distribution(CPU, rows)


@ROWS
def test_filter_random_cpu(rows):
    body_filter_random(CPU, rows)


@ROWS
def test_filter_deterministic_cpu(rows):
    body_filter_deterministic(CPU, rows)


def test_attention_decode_rows_composed_head_dim():
    """Head dims other than 64 take the composed torch path in per-row mode too."""
    H, Dh, S = 2, 32, 16
    g = torch.Generator().manual_seed(4)
    qkv = torch.randn(3, 3 * H * Dh, generator=g).to(torch.bfloat16)
    kc, vc = (torch.randn(3, H, S, Dh, generator=g).to(torch.bfloat16) for _ in range(2))
    pos = [9, 16, 0]
    k2, v2 = kc.clone(), vc.clone()
    out = torch.full((3, H * Dh), 7.0, dtype=torch.bfloat16)
    kern.attention_decode(qkv, k2, v2, posr(pos, CPU), H, out=out)
    for b, p in enumerate(pos):
        if p >= S:
            assert bool((out[b] == 7.0).all()) and torch.equal(k2[b], kc[b]) and torch.equal(v2[b], vc[b])
            continue
        ref = kern.attention_decode(qkv, kc.clone(), vc.clone(), T.posw(p, CPU), H)
        assert torch.equal(out[b], ref[b])


def test_ragged_equals_uniform_cpu():
    body_ragged_equals_uniform(CPU)


def test_teacher_forced_ragged_cpu():
    body_teacher_forced_ragged(CPU)


def test_eos_cpu():
    body_eos(CPU)


def test_eos_early_stop_cpu():
    body_eos_early_stop(CPU)


def test_api_edges_rows():
    model, P = T.make_model(CFG, CPU, 1)
    gen = Generator(model, P, 3, CPU)
    prompt = ragged_prompt([100, 100, 100], seed=2)
    for bad in ([5, 6], [[5, 6, 7]], [0, 5, 6], [5, 101, 6]):   # wrong shape, a length of 0, one above the width
        with pytest.raises(ValueError):
            gen.generate(prompt, 4, prompt_lens=torch.tensor(bad))
    with pytest.raises(ValueError, match="seq_len"):
        gen.generate(prompt, 29, prompt_lens=torch.tensor([5, 100, 6]))
    with pytest.raises(ValueError):
        gen.generate(prompt, 4, top_k=-1)
    for top_p in (0.0, 1.5):
        with pytest.raises(ValueError):
            gen.generate(prompt, 4, temperature=1.0, top_p=top_p)
    out = gen.generate(prompt, 28, prompt_lens=torch.tensor([5, 100, 6]), pad_id=7)
    assert out.shape == (3, 128) and gen.lengths.tolist() == [33, 128, 34]
    assert bool((out[0, 33:] == 7).all()) and bool((out[2, 34:] == 7).all())
    # the default sampler setting keeps its graph-cache key; any other setting has a longer one
    gen.generate(prompt, 2, temperature=0.7, seed=5)
    assert gen._graph_key() == (0.7, 5) and not gen.kv.per_row
    gen.generate(prompt, 2, temperature=0.7, seed=5, top_k=4)
    assert gen._graph_key()[:2] == (0.7, 5) and len(gen._graph_key()) > 2
    kv = KVCache(CFG, 3, CPU)
    assert kv.pos.shape == (1,) and kv.live_pos is kv.pos and not kv.per_row
    assert kv.pos_rows.shape == kv.end.shape == (3,) and kv.pos_rows.dtype == kv.end.dtype == torch.int32
