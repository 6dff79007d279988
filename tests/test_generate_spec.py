"""Speculative decoding on CPU tensors (the torch reference paths), and the device-agnostic bodies
tests/test_generate_spec_gpu.py runs again on the HIP kernels (csrc/spec.hip).

Yardsticks.  Kernel level: a plain-Python statement of the rules of ``ops.kernels.spec_judge`` /
``spec_commit`` (exact), ``sample_tokens`` (a judged row with no draft must give its token) and the
fp64 softmax of the bf16 logits with ``body_sample_distribution``'s 6 sigma bound.  Model level: the
fp64 LM of tests/test_generate.py and E_full, the training forward's own error against it, measured in
the test: the decode logits are held to 2 E_full (``body_teacher_forced``) and so are the append
logits (``body_extend_logits``), hence a greedily emitted token lies within 4 E_full of its row's fp64
maximum, and a draft (decode path) the target (append path) rejects sits at a top-2 gap <= 4 E_full."""
import dataclasses
import math

import pytest
import torch

from jax_distributed_tuts_amd.generation import SPEC_CHECK_ROUNDS, Generator, SpecState
from jax_distributed_tuts_amd.ops import kernels as kern

from . import test_generate as T
from . import test_generate_long as TL

CFG, CPU, B = T.CFG, T.CPU, T.B
S_MAX = 128


def i32(v, dev):
    return torch.tensor(v, dtype=torch.int32, device=dev)


# ----------------------------------------------------------------------------- kernel level
class Round:
    """The device state of one judge + commit call on hand-made logits ``x`` [B*C, V]."""

    def __init__(self, dev, x, tokens, pos, end, count, C, sentinel=0):
        Bq = len(pos)
        self.dev, self.C, self.Bq = dev, C, Bq
        self.x = x.to(torch.bfloat16).to(dev)
        self.tokens = tokens.clone().to(torch.int32).to(dev)
        self.pos, self.end, self.count = i32(pos, dev), i32(end, dev), i32(count, dev)
        self.acc = torch.full((Bq, C), -7, dtype=torch.int32, device=dev)
        self.repl = torch.full((Bq, C), -7, dtype=torch.int32, device=dev)
        self.ctr = [torch.full((Bq,), sentinel, dtype=torch.int32, device=dev) for _ in range(4)]
        self.dpos = torch.full((Bq,), -9, dtype=torch.int32, device=dev)
        self.dend = torch.full((Bq,), -9, dtype=torch.int32, device=dev)

    def run(self, eos_id=-1, draft_state=False, **kw):
        kern.spec_judge(self.x, self.tokens, self.pos, self.end, self.count, self.acc, self.repl, **kw)
        kern.spec_commit(self.acc, self.repl, self.tokens, self.pos, self.end, self.count, *self.ctr, eos_id=eos_id,
                         dpos=self.dpos if draft_state else None, dend=self.dend if draft_state else None)
        return self

    def state(self):
        return dict(tokens=self.tokens.cpu(), pos=self.pos.tolist(), end=self.end.tolist(), acc=self.acc.cpu(),
                    repl=self.repl.cpu(), drafted=self.ctr[0].tolist(), accepted=self.ctr[1].tolist(),
                    emitted=self.ctr[2].tolist(), last_accept=self.ctr[3].tolist())


def argmax_low(row):
    """Index of the maximum of a 1-D tensor, the lowest on ties."""
    row = row.float()
    return int((row == row.max()).nonzero()[0])


def greedy_rules(x, tokens, pos, end, count, C, eos_id=-1, sentinel=0):
    """The rules of the issue at temperature 0, in plain Python, on the state ``Round`` starts from."""
    Bq, S = tokens.shape
    x = x.to(torch.bfloat16).float().view(Bq, C, -1)
    tokens = tokens.clone().to(torch.int32)
    pos, end = list(pos), list(end)
    acc = torch.full((Bq, C), -7, dtype=torch.int32)
    repl = torch.full((Bq, C), -7, dtype=torch.int32)
    drafted, accepted, emitted, last = ([sentinel] * Bq for _ in range(4))
    for b in range(Bq):
        p, cnt, lim = pos[b], count[b], min(end[b], S)
        if not (0 <= p and 1 <= cnt <= C and p + cnt < lim):
            continue
        n = cnt - 1
        for i in range(cnt):
            g = argmax_low(x[b, i])
            acc[b, i] = int(i < n and int(tokens[b, p + 1 + i]) == g)
            repl[b, i] = g
        a = next(i for i in range(cnt) if acc[b, i] == 0)
        j = next((j for j in range(1, a + 1) if eos_id >= 0 and int(tokens[b, p + j]) == eos_id), 0)
        if j:
            pos[b], end[b], kept, out = p + j, p + j + 1, j, j
        else:
            tokens[b, p + a + 1] = repl[b, a]
            pos[b], kept, out = p + a + 1, a, a + 1
            if eos_id >= 0 and int(repl[b, a]) == eos_id:
                end[b] = p + a + 2
        drafted[b] += n
        accepted[b] += kept
        emitted[b] += out
        last[b] = kept
    return dict(tokens=tokens, pos=pos, end=end, acc=acc, repl=repl, drafted=drafted, accepted=accepted,
                emitted=emitted, last_accept=last)


def assert_state(got, want, what=""):
    for key, w in want.items():
        g = got[key]
        same = torch.equal(g, w) if isinstance(w, torch.Tensor) else g == w
        assert same, (what, key, g, w)


def distinct_rows(n, V, g):
    vals = (torch.arange(V) + 0x3000).to(torch.int16).view(torch.bfloat16)   # V distinct bf16 values
    return torch.stack([vals[torch.randperm(V, generator=g)] for _ in range(n)])


def body_greedy_judge_commit(dev):
    """Row w of a call has its first wrong draft at index w (w = n: all right); drafts behind the first
    wrong one are right again, which must not matter."""
    g = torch.Generator().manual_seed(21)
    for V in (512, 2048, 1000, 37):
        for k in (1, 4, 15):
            C, Bq = k + 1, k + 1
            x = distinct_rows(Bq * C, V, g)
            best = x.float().argmax(-1).view(Bq, C)
            pos = [(7 * b + 3) % 100 for b in range(Bq)]
            tokens = torch.randint(0, V, (Bq, S_MAX), generator=g).to(torch.int32)
            for b in range(Bq):
                for i in range(k):
                    tokens[b, pos[b] + 1 + i] = best[b, i] if i != b else (best[b, i] + 1) % V
            end, count = [S_MAX] * Bq, [C] * Bq
            want = greedy_rules(x, tokens, pos, end, count, C, sentinel=5)
            got = Round(dev, x, tokens, pos, end, count, C, sentinel=5).run().state()
            assert_state(got, want, (V, k))
            for b in range(Bq):   # the literal expectation, and nothing but column p + a + 1 changes
                a = b
                assert got["pos"][b] == pos[b] + a + 1 and got["last_accept"][b] == a
                assert got["emitted"][b] == 5 + a + 1 and got["drafted"][b] == 5 + k and got["accepted"][b] == 5 + a
                assert int(got["tokens"][b, pos[b] + a + 1]) == int(best[b, a])
                keep = torch.ones(S_MAX, dtype=torch.bool)
                keep[pos[b] + a + 1] = False
                assert torch.equal(got["tokens"][b, keep], tokens[b, keep])
            assert got["end"] == end
    # exact ties: the lowest index wins, for accepting and for the replacement
    x = torch.zeros(2 * 3, 2048)
    x[0, [700, 9, 1999]] = 3.0
    x[1, [2047, 256]] = 3.0
    x[3, [255, 256]] = 3.0
    x[4, [30, 31]] = 3.0
    tokens = torch.zeros(2, S_MAX, dtype=torch.int32)
    tokens[0, 11:13] = torch.tensor([9, 2047])     # lowest tie index: kept; a higher one: rejected, repl 256
    tokens[1, 21:23] = torch.tensor([256, 30])     # the higher index of the tie: rejected at once, repl 255
    got = Round(dev, x, tokens, [10, 20], [S_MAX] * 2, [3, 3], 3).run().state()
    assert_state(got, greedy_rules(x, tokens, [10, 20], [S_MAX] * 2, [3, 3], 3), "ties")
    assert got["pos"] == [12, 21] and got["last_accept"] == [1, 0]
    assert int(got["tokens"][0, 12]) == 256 and int(got["tokens"][1, 21]) == 255
    assert got["acc"][0].tolist() == [1, 0, 0] and got["repl"][0].tolist() == [9, 256, 0]


def body_range_liveness(dev):
    k, C, V = 4, 5, 512
    g = torch.Generator().manual_seed(22)
    #        count 0, count > C, p < 0, p + count >= lim, finished, live, live (short count)
    pos = [10, 20, -1, 124, 50, 60, 122]
    end = [S_MAX, S_MAX, S_MAX, S_MAX, 51, S_MAX, 126]
    count = [0, C + 1, 3, 4, 2, 5, 3]
    Bq = len(pos)
    x = distinct_rows(Bq * C, V, g)
    best = x.float().argmax(-1).view(Bq, C)
    tokens = torch.randint(0, V, (Bq, S_MAX), generator=g).to(torch.int32)
    tokens[5, 61:63] = best[5, :2]      # row 5 keeps two drafts, row 6 its only two
    tokens[5, 63] = (best[5, 2] + 1) % V
    tokens[6, 123:125] = best[6, :2]
    for kw in (dict(), dict(temperature=1.0, seed=5, top_k=50, top_p=0.9)):
        got = Round(dev, x, tokens, pos, end, count, C, sentinel=3).run(draft_state=True, **kw)
        st = got.state()
        for b in range(5):   # untouched: every sentinel stands
            assert torch.equal(st["tokens"][b], tokens[b]) and st["pos"][b] == pos[b] and st["end"][b] == end[b]
            assert bool((st["acc"][b] == -7).all()) and bool((st["repl"][b] == -7).all())
            assert [st[c][b] for c in ("drafted", "accepted", "emitted", "last_accept")] == [3] * 4
        # the drafter's state follows whatever pos / end hold after the round, for every row
        assert got.dpos.tolist() == st["pos"]
        assert got.dend.tolist() == [max(min(e, S_MAX) - 1, 0) for e in st["end"]]
        if not kw:
            assert_state(st, greedy_rules(x, tokens, pos, end, count, C, sentinel=3), "mixed")
            assert st["pos"][5:] == [63, 125] and st["last_accept"][5:] == [2, 2]
            for b in (5, 6):   # the bits of the row's solo call
                solo = Round(dev, x[b * C:(b + 1) * C], tokens[b:b + 1], pos[b:b + 1], end[b:b + 1], count[b:b + 1], C,
                             sentinel=3).run().state()
                for key in ("tokens", "acc", "repl"):
                    assert torch.equal(solo[key][0], st[key][b]), (b, key)
                for key in ("pos", "end", "drafted", "accepted", "emitted", "last_accept"):
                    assert solo[key][0] == st[key][b], (b, key)
        else:   # sampling draws depend on the row index: the same call with the other rows switched off
            only = [c if b >= 5 else 0 for b, c in enumerate(count)]
            alone = Round(dev, x, tokens, pos, end, only, C, sentinel=3).run(**kw).state()
            assert_state({key: v for key, v in st.items()}, alone, "sampled")
    # entries i >= count[b] of a live row stay as they were
    assert bool((st["acc"][6, 3:] == -7).all()) and bool((st["repl"][6, 3:] == -7).all())


def body_spec_count(dev):
    k = 4
    rows = []   # (p, end, n_drafted, want)
    for room, wants in ((-1, (0, 0)), (0, (1, 1)), (1, (1, 2)), (k, (1, 1 + k))):
        for nd, want in zip((0, k), wants):
            rows.append((40, 40 + room + 2, nd, want))
    rows += [(-1, S_MAX, k, 0), (S_MAX - 1, 400, k, 0), (S_MAX - 2, 400, k, 1), (S_MAX - 3, 400, k, 2),
             (5, S_MAX, k + 9, 1 + k), (5, S_MAX, -2, 1)]
    p, e, nd, want = (list(v) for v in zip(*rows))
    out = torch.full((len(rows),), -7, dtype=torch.int32, device=dev)
    got = kern.spec_count(i32(p, dev), i32(e, dev), i32(nd, dev), k, S_MAX, out=out)
    assert got is out and out.tolist() == want
    for b, c in enumerate(want):   # the guarantee: the append stays inside the cache, the last index below lim
        if c:
            assert p[b] + c <= min(e[b], S_MAX) - 1
    with pytest.raises(ValueError):
        kern.spec_count(i32(p, dev), i32(e, dev), i32(nd, dev), 16, S_MAX)
    with pytest.raises(ValueError):
        kern.spec_count(i32(p, dev), i32(e, dev), i32(nd, dev), 0, S_MAX)


def body_eos(dev):
    k, C, V, EOS = 4, 5, 37, 30
    hot = [[3, 4, 5, 6, 7]] * 4 + [[3, EOS, 5, 6, 7]]
    drafts = [[EOS, 4, 5, 6],    # accepted EOS at j = 1 (its logits row must say EOS: see below)
              [3, EOS, 5, 6],    # in the middle, everything accepted
              [3, EOS, 9, 6],    # at j = a = 2 (draft 3 is wrong)
              [3, EOS, 5, 6],    # a rejected draft equal to EOS: no effect
              [3, 9, 5, 6]]      # the replacement is EOS
    hot[0], hot[1], hot[2] = [EOS, 4, 5, 6, 7], [3, EOS, 5, 6, 7], [3, EOS, 5, 6, 7]
    Bq = len(drafts)
    x = torch.zeros(Bq * C, V)
    for b in range(Bq):
        for i in range(C):
            x[b * C + i, hot[b][i]] = 5.0
    pos = [10, 20, 30, 40, 50]
    tokens = torch.full((Bq, S_MAX), 1, dtype=torch.int32)
    for b in range(Bq):
        tokens[b, pos[b] + 1:pos[b] + 1 + k] = torch.tensor(drafts[b], dtype=torch.int32)
    end, count = [S_MAX] * Bq, [C] * Bq
    got = Round(dev, x, tokens, pos, end, count, C).run(eos_id=EOS).state()
    assert_state(got, greedy_rules(x, tokens, pos, end, count, C, eos_id=EOS), "eos")
    assert got["pos"] == [11, 22, 32, 42, 52]
    assert got["end"] == [12, 23, 33, S_MAX, 53]
    assert got["emitted"] == [1, 2, 2, 2, 2] and got["last_accept"] == [1, 2, 2, 1, 1]
    for b in range(3):   # an accepted EOS writes nothing to tokens
        assert torch.equal(got["tokens"][b], tokens[b])
    assert int(got["tokens"][3, 42]) == 4 and int(got["tokens"][4, 52]) == EOS
    # the same call without eos_id: the rows run on
    free = Round(dev, x, tokens, pos, end, count, C).run().state()
    assert free["pos"] == [15, 25, 33, 42, 52] and free["end"] == end


FILTERS = [dict(), dict(top_k=50, top_p=0.9)]


def body_sample_no_drafts(dev):
    """count = 1: the round's token is ``sample_tokens``' token for the row, position, seed and filter."""
    N, C = 64, 2
    x, _ = T.live8(N)
    pos = [(b * 5) % 126 for b in range(N)]
    x2 = torch.zeros(N * C, x.shape[1], dtype=torch.bfloat16)
    x2[0::C] = x
    for filt in FILTERS:
        for seed in (1234, 77):
            tok = torch.full((N, S_MAX), -1, dtype=torch.int32, device=dev)
            pw = i32(pos, dev)
            kern.sample_tokens(x.to(dev), tok, pw, end=i32([S_MAX] * N, dev), temperature=1.0, seed=seed, **filt)
            r = Round(dev, x2, torch.full((N, S_MAX), -1), pos, [S_MAX] * N, [1] * N, C).run(temperature=1.0, seed=seed,
                                                                                           **filt)
            assert torch.equal(r.tokens, tok) and torch.equal(r.pos, pw)
            st = r.state()
            assert st["emitted"] == [1] * N and st["drafted"] == [0] * N and bool((st["acc"][:, 0] == 0).all())


def _within(freq, p, N):
    return abs(freq - p) <= 6 * math.sqrt(p * (1 - p) / N)


def _draft_round(dev, N, draft, pos=5, seed=1234, **filt):
    x, cols = T.live8(N)
    x2 = torch.zeros(N * 2, x.shape[1], dtype=torch.bfloat16)
    x2[0::2] = x
    tokens = torch.full((N, S_MAX), -1)
    tokens[:, pos + 1] = draft
    r = Round(dev, x2, tokens, [pos] * N, [S_MAX] * N, [2] * N, 2).run(temperature=1.0, seed=seed, **filt)
    return x, cols, r.acc[:, 0].cpu().bool(), r.repl[:, 0].cpu().long(), r.tokens[:, pos + 1].cpu().long()


def body_sample_distribution(dev):
    """One draft per row on live8 at T = 1: it is accepted with its fp64 probability and the first
    emitted token (the draft, or the replacement) follows the fp64 softmax, 6 sigma per bin
    (``body_sample_distribution``'s bound: false fail < 1e-8 per bin)."""
    N = 8192
    x, cols, acc, repl, first = _draft_round(dev, N, int(T.live8(1)[1][3]))
    c0 = int(cols[3])
    p = torch.softmax(x[0].double(), -1)
    assert _within(float(acc.double().mean()), float(p[c0]), N), (float(acc.double().mean()), float(p[c0]))
    assert bool((first[acc] == c0).all()) and bool((first[~acc] == repl[~acc]).all()) and bool((repl != c0).all())
    assert bool(torch.isin(first, cols).all())
    for c in cols.tolist():
        assert _within(float((first == c).double().mean()), float(p[c]), N), c
    # a draft on a dead column is never accepted and the replacement is the plain sampler's distribution
    x, cols, acc, repl, first = _draft_round(dev, N, 5)
    assert not bool(acc.any()) and torch.equal(first, repl) and bool(torch.isin(first, cols).all())
    for c in cols.tolist():
        assert _within(float((first == c).double().mean()), float(p[c]), N), c
    # top_k = 4 keeps the four largest live columns: a draft on the smallest one is outside the set
    x, cols, acc, repl, first = _draft_round(dev, N, int(cols[0]), top_k=4)
    assert not bool(acc.any()) and bool(torch.isin(first, cols[4:]).all())
    p4 = p[cols[4:]] / p[cols[4:]].sum()
    for c, pc in zip(cols[4:].tolist(), p4.tolist()):
        assert _within(float((first == c).double().mean()), pc, N), c


def body_sample_deterministic(dev):
    N = 256
    c0 = int(T.live8(1)[1][3])
    a = _draft_round(dev, N, c0, pos=9, seed=77)
    b = _draft_round(dev, N, c0, pos=9, seed=77)
    assert torch.equal(a[2], b[2]) and torch.equal(a[3], b[3]) and torch.equal(a[4], b[4])
    for other in (_draft_round(dev, N, c0, pos=10, seed=77), _draft_round(dev, N, c0, pos=9, seed=78)):
        assert not torch.equal(a[2], other[2]) and not torch.equal(a[3], other[3])


# ----------------------------------------------------------------------------- model level
def make_pair(cfg, dev, seed, kind, batch=B, **kw):
    """(generator with a draft, its model, P).  ``kind`` "self": the target's own weights as the draft;
    "small": a 1-layer draft with another seed."""
    model, P = T.make_model(cfg, dev, seed)
    draft = (model, P) if kind == "self" else T.make_model(dataclasses.replace(cfg, n_layers=1), dev, seed + 7)
    return Generator(model, P, batch, dev, draft=draft, **kw), model, P


def fp64_of(model, P, cfg, out):
    """(F, E_full) over the tokens ``out`` [B, n] padded to seq_len: the fp64 logits [B, n, V] and the
    training forward's largest error against them."""
    n = out.shape[1]
    padded = torch.zeros(out.shape[0], cfg.seq_len, dtype=torch.int32)
    padded[:, :n] = out.cpu()
    F = T.lm_logits_fp64(P, cfg, padded)[:, :n]
    f = T.full_logits(model, P, padded)[:, :n]
    return F, float((f - F).abs().max())


def check_greedy(F, e_full, out, lens, new):
    worst = 0.0
    for b, n in enumerate(lens):
        for t in range(n, n + new):
            row = F[b, t - 1]
            worst = max(worst, float(row.max() - row[int(out[b, t])]))
    assert worst <= 4 * e_full, (worst, e_full)
    return worst


GREEDY_CASES = [(CFG, 60, [58, 60, 62]), (TL.CFG_LONG, 124, [122, 124, 126])]   # rounds cross rows 63..65 / 127..129


def body_greedy_is_greedy(dev, cfg, Pn, ragged, kind, k, capture=False):
    new = 8
    gen, model, P = make_pair(cfg, dev, 2, "self" if kind == "self" else "small")
    lens = ragged if kind == "ragged" else [Pn] * B
    prompt = torch.randint(0, cfg.vocab_size, (B, max(lens)), generator=torch.Generator().manual_seed(9)).to(torch.int32)
    kw = dict(prompt_lens=torch.tensor(lens)) if kind == "ragged" else {}
    out = gen.generate(prompt.to(dev), new, speculative=k, capture=capture, pad_id=0, **kw).cpu()
    assert out.shape == (B, max(lens) + new) and out.dtype == torch.int32
    assert gen.lengths.tolist() == [n + new for n in lens]
    for b, n in enumerate(lens):
        assert torch.equal(out[b, :n], prompt[b, :n]) and bool((out[b, n + new:] == 0).all())
    assert gen.spec_emitted.tolist() == [new] * B and 1 <= gen.spec_rounds <= new
    assert bool((gen.spec_accepted <= gen.spec_drafted).all())
    F, e_full = fp64_of(model, P, cfg, out)
    worst = check_greedy(F, e_full, out, lens, new)
    T.log_errors(name="spec_greedy", device=str(dev), seq_len=cfg.seq_len, kind=kind, k=k, E_full=e_full,
                 worst_gap=worst, rounds=gen.spec_rounds, accepted=int(gen.spec_accepted.sum()),
                 drafted=int(gen.spec_drafted.sum()))
    if kind == "self":   # some position has a top-2 gap no rounding can bridge: its draft is kept
        assert int(gen.spec_accepted.sum()) > 0
    return gen


def record_rounds(gen, k):
    """Wrap ``gen.spec_step``: per round (pos before, count, last_accept, pos after, logits), host copies."""
    log, real = [], gen.spec_step

    def step(kk):
        before = gen.kv.pos_rows.tolist()
        logits = real(kk)
        st = gen.spec_state(kk)
        log.append((before, st.count.tolist(), st.last_accept.tolist(), gen.kv.pos_rows.tolist(),
                    logits.detach().float().cpu()))
        return logits

    gen.spec_step = step
    return log


def body_acceptance_teeth(dev, model_seed):
    """Self-draft: the drafter (decode path) and the target (append path) are each within 2 E_full of
    fp64, so they can disagree only where the fp64 top-2 gap is <= 4 E_full.  Not vacuous: at least a
    quarter of the judged draft positions have a wider gap (CPU, plain greedy, prompt seed 9, Pn = 60, 40
    new tokens: 70 of 120 positions at model seed 2, E_full 0.050; 65 of 120 at seed 5, E_full 0.055)."""
    k, Pn, new = 4, 60, 40
    gen, model, P = make_pair(CFG, dev, model_seed, "self")
    log = record_rounds(gen, k)
    prompt = torch.randint(0, CFG.vocab_size, (B, Pn), generator=torch.Generator().manual_seed(9)).to(torch.int32)
    out = gen.generate(prompt.to(dev), new, speculative=k, capture=False).cpu()
    assert gen.lengths.tolist() == [Pn + new] * B and len(log) == gen.spec_rounds
    F, e_full = fp64_of(model, P, CFG, out)
    check_greedy(F, e_full, out, [Pn] * B, new)
    top2 = torch.topk(F, 2, dim=-1).values
    gap = top2[..., 0] - top2[..., 1]   # [B, n]
    judged = wide = rejected = 0
    for before, count, kept, after, _ in log:
        for b in range(B):
            n = count[b] - 1
            if count[b] == 0 or after[b] == before[b]:
                continue
            assert after[b] == before[b] + kept[b] + 1   # no EOS here
            for i in range(min(kept[b] + 1, n)):   # draft i was judged on the logits at index p + i
                judged += 1
                wide += float(gap[b, before[b] + i]) > 4 * e_full
            if kept[b] < n:
                rejected += 1
                g = float(gap[b, before[b] + kept[b]])
                assert g <= 4 * e_full, (b, before[b], kept[b], g, e_full)
    T.log_errors(name="spec_teeth", device=str(dev), model_seed=model_seed, E_full=e_full, judged=judged, wide=wide,
                 rejected=rejected, rounds=gen.spec_rounds)
    assert judged > 0 and 4 * wide >= judged, (wide, judged)


def body_small_draft(dev):
    """A 1-layer draft with other weights: most drafts are rejected, the output is still greedy."""
    k, Pn, new = 4, 60, 40
    gen, model, P = make_pair(CFG, dev, 2, "small")
    prompt = torch.randint(0, CFG.vocab_size, (B, Pn), generator=torch.Generator().manual_seed(9)).to(torch.int32)
    out = gen.generate(prompt.to(dev), new, speculative=k, capture=False).cpu()
    F, e_full = fp64_of(model, P, CFG, out)
    check_greedy(F, e_full, out, [Pn] * B, new)
    acc, dr = int(gen.spec_accepted.sum()), int(gen.spec_drafted.sum())
    T.log_errors(name="spec_small_draft", device=str(dev), accepted=acc, drafted=dr, rounds=gen.spec_rounds)
    assert dr > 0 and 2 * acc < dr, (acc, dr)   # unrelated weights over 512 tokens: agreement is chance


def body_caches_consistent(dev):
    k, new = 4, 12
    lens = [56, 60, 61]
    gen, model, P = make_pair(CFG, dev, 2, "small")
    prompt = torch.randint(0, CFG.vocab_size, (B, max(lens)), generator=torch.Generator().manual_seed(9)).to(torch.int32)
    out = gen.generate(prompt.to(dev), new, speculative=k, capture=False, prompt_lens=torch.tensor(lens)).cpu()
    assert int(gen.spec_accepted.sum()) < int(gen.spec_drafted.sum())   # there were rejections
    final = [n + new for n in lens]
    assert gen.lengths.tolist() == final and gen.kv.pos_rows.tolist() == [n - 1 for n in final]
    assert gen.draft.kv.pos_rows.tolist() == gen.kv.pos_rows.tolist()
    for g, (m, p) in ((gen, (model, P)), (gen.draft, (gen.draft.model, gen.draft.P))):
        cfg = m.cfg
        F, e_full = fp64_of(m, p, cfg, out)
        fresh = Generator(m, p, B, dev)
        fresh.prefill(out.to(dev), torch.tensor(final), chunk=64)
        a = g.step(sample=False).detach().cpu().double()
        f = fresh.step(sample=False).detach().cpu().double()
        for b, n in enumerate(final):
            for got in (a, f):
                err = float((got[b] - F[b, n - 1]).abs().max())
                assert err <= 2 * e_full, (b, err, e_full)
            for l in range(cfg.n_layers):
                T.close(g.kv.k[l][b, :, :n - 1], fresh.kv.k[l][b, :, :n - 1])
                T.close(g.kv.v[l][b, :, :n - 1], fresh.kv.v[l][b, :, :n - 1])


def body_edges(dev):
    model, P = T.make_model(CFG, dev, 1)
    small = T.make_model(dataclasses.replace(CFG, n_layers=1), dev, 8)
    prompt = torch.randint(0, CFG.vocab_size, (B, 20), generator=torch.Generator().manual_seed(3)).to(torch.int32).to(dev)
    plain = Generator(model, P, B, dev)
    with pytest.raises(ValueError, match="draft"):
        plain.generate(prompt, 4, speculative=2)
    with pytest.raises(ValueError, match="draft"):
        plain.prefill(prompt, torch.tensor([20] * B)) or plain.spec_step(2)
    for bad in (dataclasses.replace(CFG, n_layers=1, vocab_size=256), dataclasses.replace(CFG, n_layers=1, seq_len=64)):
        with pytest.raises(ValueError):
            Generator(model, P, B, dev, draft=T.make_model(bad, dev, 8))
    gen = Generator(model, P, B, dev, draft=small)
    assert gen.draft.kv.tokens is gen.kv.tokens
    for k in (0, 16, -1):
        with pytest.raises(ValueError):
            gen.generate(prompt, 4, speculative=k)
    with pytest.raises(ValueError, match="prefill"):   # before any prefill
        gen.spec_step(2)
    with pytest.raises(ValueError, match="prefill"):
        gen.verify(torch.ones(B, dtype=torch.int32), k=2)
    gen.prefill(prompt)                                # a shared-position cache
    with pytest.raises(ValueError, match="per-row"):
        gen.spec_step(2)
    with pytest.raises(ValueError, match="per-row"):
        gen.verify(torch.ones(B, dtype=torch.int32), k=2)
    gen.prefill(prompt, torch.tensor([20] * B))        # per-row, but the draft was not prefilled
    with pytest.raises(ValueError, match="sync"):
        gen.spec_step(2)
    out = gen.generate(prompt, 4, speculative=2, capture=False)
    gen.spec_step(2)                                   # in sync after a speculative generate (rows finished: a no-op)
    assert torch.equal(gen.kv.tokens[:, :24], out)
    gen.extend(torch.zeros(B, 2, dtype=torch.int32))
    with pytest.raises(ValueError, match="sync"):
        gen.spec_step(2)
    # max_new_tokens = 0
    out = gen.generate(prompt, 0, speculative=2, capture=False)
    assert torch.equal(out, prompt) and gen.lengths.tolist() == [20] * B and gen.spec_rounds == 0
    assert gen.spec_emitted.tolist() == [0] * B
    assert SPEC_CHECK_ROUNDS == 4 and isinstance(gen.spec_state(2), SpecState)


def body_cache_end(dev):
    """Prompts that end at seq_len - 1 and seq_len - 2 (and one with room): no round passes the end of the
    cache, and ``tokens`` at and past a row's limit is never written."""
    S = CFG.seq_len
    gen, model, P = make_pair(CFG, dev, 2, "self")
    lens = [S - 1, S - 2, S - 9]
    prompt = torch.randint(1, CFG.vocab_size, (B, S - 1), generator=torch.Generator().manual_seed(3)).to(torch.int32)
    out = gen.generate(prompt.to(dev), 1, speculative=4, capture=False, prompt_lens=torch.tensor(lens)).cpu()
    assert out.shape == (B, S) and gen.lengths.tolist() == [S, S - 1, S - 8]
    toks = gen.kv.tokens.cpu()
    for b, n in enumerate(lens):
        assert torch.equal(toks[b, :n], prompt[b, :n]) and bool((toks[b, n + 1:] == 0).all()), b
    assert gen.spec_emitted.tolist() == [1] * B and gen.spec_drafted.tolist() == [0] * B
    # with room for new tokens up to the end of the cache: every row ends exactly at seq_len
    out = gen.generate(prompt.to(dev), 9, speculative=4, capture=False, prompt_lens=torch.tensor([S - 9] * B)).cpu()
    assert gen.lengths.tolist() == [S] * B and gen.kv.pos_rows.tolist() == [S - 1] * B
    F, e_full = fp64_of(model, P, CFG, out)
    check_greedy(F, e_full, out, [S - 9] * B, 9)


def body_eos_rows(dev, capture=False):
    """EOS stops one row while the others go on: the token a row emits third becomes ``eos_id``."""
    lens, new, k = [5, 20, 40, 60], 8, 4   # the lengths of test_generate_rows.body_eos
    gen, _, _ = make_pair(CFG, dev, 2, "self", batch=len(lens))
    prompt = torch.randint(0, CFG.vocab_size, (len(lens), max(lens)), generator=torch.Generator().manual_seed(9)).to(torch.int32)
    kw = dict(speculative=k, capture=capture, prompt_lens=torch.tensor(lens), pad_id=-1)
    first = gen.generate(prompt.to(dev), new, **kw).cpu()
    pick = [r for r, n in enumerate(lens)
            if first[r, n + 2] not in first[r, n:n + 2]
            and all(first[r, n + 2] not in first[b, m:m + new] for b, m in enumerate(lens) if b != r)]
    assert pick, "no row emits a token at its third step that is unique to it: choose other seeds"
    r = pick[0]
    eos = int(first[r, lens[r] + 2])
    out = gen.generate(prompt.to(dev), new, eos_id=eos, **kw).cpu()
    want = [n + new for n in lens]
    want[r] = lens[r] + 3
    assert gen.lengths.tolist() == want and int(gen.kv.end[r]) == want[r]
    assert gen.spec_emitted.tolist() == [w - n for w, n in zip(want, lens)]
    assert torch.equal(out[r, :want[r]], first[r, :want[r]]) and bool((out[r, want[r]:] == -1).all())
    for b in range(len(lens)):
        if b != r:
            assert torch.equal(out[b], first[b])


def body_sampling_mode(dev):
    """T = 0.8, top_k 50, top_p 0.9: reproducible per seed, and every emitted token lies in the kept set
    of the logits row that judged it (``_filter_weights`` on the round's own logits)."""
    k, Pn, new = 4, 30, 12
    kw = dict(speculative=k, capture=False, temperature=0.8, top_k=50, top_p=0.9)
    gen, _, _ = make_pair(CFG, dev, 2, "self")
    prompt = torch.randint(0, CFG.vocab_size, (B, Pn), generator=torch.Generator().manual_seed(9)).to(torch.int32).to(dev)
    a = gen.generate(prompt, new, seed=11, **kw).cpu()
    log = record_rounds(gen, k)
    b_ = gen.generate(prompt, new, seed=11, **kw).cpu()
    assert torch.equal(a, b_) and gen.lengths.tolist() == [Pn + new] * B
    checked = 0
    for before, count, kept, after, logits in log:
        x = logits.to(torch.bfloat16).float().view(B, k + 1, -1)
        for b in range(B):
            for i in range(after[b] - before[b]):
                row = x[b, i][None]
                w = torch.exp((row - row.max()) / 0.8)
                keep = kern._filter_weights(row, w, 50, 0.9)[0] > 0
                assert bool(keep[int(b_[b, before[b] + i + 1])]), (b, before[b], i)
                checked += 1
    assert checked == B * new
    c = gen.generate(prompt, new, seed=12, **kw).cpu()
    assert not torch.equal(a, c)


def body_verify_hook(dev):
    """``verify`` on drafts the caller wrote: the target's own greedy continuation is accepted whole, a
    wrong draft is replaced by the token the plain greedy step emits."""
    k, Pn = 3, 62
    gen, model, P = make_pair(CFG, dev, 2, "self")
    prompt = torch.randint(0, CFG.vocab_size, (B, Pn), generator=torch.Generator().manual_seed(9)).to(torch.int32).to(dev)
    ref = gen.generate(prompt, 6, speculative=k, capture=False).cpu()
    gen.prefill(prompt, torch.tensor([Pn] * B))
    gen.kv.tokens[:, Pn:Pn + k] = ref[:, Pn:Pn + k].to(dev)
    gen.kv.tokens[1, Pn + 1] = (ref[1, Pn + 1] + 1) % CFG.vocab_size
    logits = gen.verify(torch.tensor([k + 1, k + 1, 1]), k=k)
    assert logits.shape == (B * (k + 1), CFG.vocab_size)
    st = gen.spec_state(k)
    # row 0: everything kept, plus one token; row 1: one draft kept, then the target's own; row 2: no drafts
    assert st.last_accept.tolist() == [k, 1, 0] and gen.kv.pos_rows.tolist() == [Pn + k, Pn + 1, Pn]
    got = gen.kv.tokens.cpu()
    F, e_full = fp64_of(model, P, CFG, got[:, :Pn + k + 1])
    for b, n in enumerate([k + 1, 2, 1]):
        for t in range(Pn, Pn + n):
            row = F[b, t - 1]
            assert float(row.max() - row[int(got[b, t])]) <= 4 * e_full


# ----------------------------------------------------------------------------- CPU tests
def test_greedy_judge_commit_cpu():
    body_greedy_judge_commit(CPU)


def test_range_liveness_cpu():
    body_range_liveness(CPU)


def test_spec_count_cpu():
    body_spec_count(CPU)


def test_eos_kernel_cpu():
    body_eos(CPU)


def test_sample_no_drafts_cpu():
    body_sample_no_drafts(CPU)


def test_sample_distribution_cpu():
    body_sample_distribution(CPU)


def test_sample_deterministic_cpu():
    body_sample_deterministic(CPU)


KINDS = pytest.mark.parametrize("kind", ["self", "small", "ragged"])
KS = pytest.mark.parametrize("k", [1, 4])
SHAPES = pytest.mark.parametrize("case", GREEDY_CASES, ids=["s128", "s320"])


@SHAPES
@KINDS
@KS
def test_greedy_is_greedy_cpu(case, kind, k):
    body_greedy_is_greedy(CPU, *case, kind, k)


@pytest.mark.parametrize("model_seed", [2, 5])
def test_acceptance_teeth_cpu(model_seed):
    body_acceptance_teeth(CPU, model_seed)


def test_small_draft_cpu():
    body_small_draft(CPU)


def test_caches_consistent_cpu():
    body_caches_consistent(CPU)


def test_edges_cpu():
    body_edges(CPU)


def test_cache_end_cpu():
    body_cache_end(CPU)


def test_eos_rows_cpu():
    body_eos_rows(CPU)


def test_sampling_mode_cpu():
    body_sampling_mode(CPU)


def test_verify_hook_cpu():
    body_verify_hook(CPU)
