"""Beam search on CPU tensors (the torch paths of ops.kernels.beam_topw / beam_reorder), and the
device-agnostic test bodies that tests/test_generate_beam_gpu.py runs again on csrc/beam.hip.

Yardsticks: a float64 log-softmax / merge built from the bf16 logits and fp32 scores the kernel read
(``check_select``), exact permutations of position-encoded caches, and the fp64 LM of
tests/test_generate.py for the search as a whole."""
import os
import subprocess
import sys

import pytest
import torch

from jax_distributed_tuts_amd.generation import Generator
from jax_distributed_tuts_amd.models.transformer import TransformerConfig
from jax_distributed_tuts_amd.ops import kernels as kern

from . import test_generate as T
from .rowcheck import U32, _log

CFG = T.CFG
CPU = T.CPU
G = 2
NEG = float("-inf")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ----------------------------------------------------------------------------- select (topw + merge)
def run_select(dev, logits, score, done, W, eos_id):
    """beam_topw, then the merge through beam_reorder on a cache-less state (pos 0 of 4 columns).
    Returns (parent, token, new score, cand_tok, cand_score) on the CPU."""
    Bq = logits.shape[0]
    pos = T.posw(0, dev)
    tokens = torch.zeros(Bq, 4, dtype=torch.int32, device=dev)
    sc, dn = score.to(dev).clone(), done.to(dev).clone()
    ln, par, tok = (torch.zeros(Bq, dtype=torch.int32, device=dev) for _ in range(3))
    cand = kern.beam_topw(logits.to(dev), sc, dn, pos, W, eos_id, seq_len=4)
    ct, cs = cand[0].cpu().clone(), cand[1].cpu().clone()
    kern.beam_reorder(cand, [], [], tokens, sc, dn, ln, par, tok, pos, W, eos_id)
    assert int(pos.item()) == 1 and torch.equal(tokens[:, 1].cpu(), tok.cpu())
    return par.cpu(), tok.cpu(), sc.cpu(), ct, cs


def select_fp64(logits, score, done, W, eos_id):
    """The spec in float64 from the bf16 logits and fp32 scores.  Per group a list of candidates
    (score, slot, rank, token, bound) sorted by (score descending, slot, rank); ``bound`` is
    ``check_select``'s bound of that candidate's fp32 score."""
    x = logits.double()
    Bq, V = x.shape
    gmx = x.max(-1, keepdim=True).values
    d = x - gmx
    S = torch.exp(d).sum(-1, keepdim=True)
    lse = torch.log(S)
    # x - gmx in fp32 is exact unless the two exponents are > 16 binades apart; what its rounding does to S
    inexact = ((d - d.float().double()).abs() * torch.exp(d)).sum(-1, keepdim=True) / S
    order = torch.sort(x, dim=-1, descending=True, stable=True).indices[:, :W]
    groups = []
    for g in range(Bq // W):
        cands = []
        for j in range(W):
            b = g * W + j
            s = float(score[b])
            if int(done[b]):
                cands.append((s, j, 0, eos_id, 0.0))
                continue
            for r, t in enumerate(order[b].tolist()):
                dd, ll = float(d[b, t]), float(lse[b])
                mag = (0.0 if s == NEG else abs(s)) + abs(dd) + abs(ll)
                cands.append((s + (dd - ll), j, r, t, U32 * (V + 4) + float(inexact[b]) + 4 * U32 * mag))
        cands.sort(key=lambda c: (-c[0], c[1], c[2]))
        groups.append(cands)
    return groups


def select_precondition(groups, W):
    """Among the fp64 top W + 1, finite scores from different slots differ by more than twice the bound."""
    for cands in groups:
        top = cands[:W + 1]
        for i, a in enumerate(top):
            for b in top[i + 1:]:
                if a[1] != b[1] and a[0] != NEG and b[0] != NEG and abs(a[0] - b[0]) <= 2 * max(a[4], b[4]):
                    return False
    return True


def check_select(variant, dev, logits, score, done, W, eos_id):
    """``beam_topw`` + the merge against float64.  Exact: parent, token and their order.  Scores: within

        bound = 2^-24 (V + 4) + r + 4 * 2^-24 (|score| + |x - gmx| + |lse|)

    of score + ((x - gmx) - lse) evaluated in fp64 from the same bf16 logits and fp32 score.  Derivation,
    u = 2^-24: the sum S of V positive terms in any order is within (V - 1) u of exact, relatively;
    each term comes from expf (<= 1 ulp = 2 u); products of the (1 + u) factors add second-order terms,
    below 3 u here: (V + 4) u relative on S is (V + 4) u absolute on lse = logf(S).  r covers the
    argument of expf: x - gmx is exact in fp32 unless the exponents of x and gmx lie > 16 binades apart;
    r = sum |d_i - fl32(d_i)| exp(d_i) / S is what those roundings do to S (0 for most rows).  Then logf
    (<= 1 ulp: 2 u |lse|), and the three roundings of x - gmx, (.) - lse and score + (.), each at most u times
    the sum of the magnitudes involved: at most 3 u |x - gmx|, 4 u |lse|, u |score|, rounded up to 4 u of
    each.  A done slot's score is copied: exact.  The kernel uses libm expf / logf (1 ulp), not the fast
    intrinsics.  Returns the worst err / bound."""
    groups = select_fp64(logits, score, done, W, eos_id)
    assert select_precondition(groups, W), "the fp64 candidates are too close for an exact comparison"
    par, tok, sc, _, _ = run_select(dev, logits, score, done, W, eos_id)
    worst = 0.0
    for g, cands in enumerate(groups):
        for j, (s, slot, _, t, bound) in enumerate(cands[:W]):
            b = g * W + j
            assert (int(par[b]), int(tok[b])) == (slot, t), (variant, g, j, int(par[b]), int(tok[b]), slot, t)
            got = float(sc[b])
            if s == NEG or bound == 0.0:
                assert got == s, (variant, g, j, got, s)
                continue
            err = abs(got - s)
            assert err <= bound, (variant, g, j, got, s, err, bound)
            worst = max(worst, err / bound)
    _log(variant, "score", worst)
    return worst


def select_inputs(V, W, seed):
    """G = 2 groups.  Group 0: the first-step pattern (0, -inf, ...).  Group 1: finite scores, and with
    W > 1 its last slot done.  Logits: bf16 of 3 * randn."""
    g = torch.Generator().manual_seed(seed)
    logits = (3.0 * torch.randn(G * W, V, generator=g)).to(torch.bfloat16)
    score = torch.full((G * W,), NEG)
    score[0] = 0.0
    score[W:] = -5.0 * torch.rand(W, generator=g) - 1.0
    done = torch.zeros(G * W, dtype=torch.int32)
    if W > 1:
        done[-1] = 1
    return logits, score, done


SELECT_SHAPES = [(V, W) for V in (8, 50, 512, 2048) for W in (1, 2, 3, 8) if W <= V]


def body_select(dev, V, W):
    eos_id = V - 3
    for seed in range(100 * V + W, 100 * V + W + 50):   # the first seed whose fp64 candidates are well apart
        logits, score, done = select_inputs(V, W, seed)
        if select_precondition(select_fp64(logits, score, done, W, eos_id), W):
            break
    name = "cpu" if dev.type == "cpu" else "hip"
    ratio = check_select(f"beam_select<{name},V={V},W={W}>", dev, logits, score, done, W, eos_id)
    assert ratio <= 1.0
    return ratio


def body_ties(dev):
    """The same bf16 logit at several columns: the lower token index first.  Two slots with equal
    scores and identical rows: the lower slot first.  W = 1: the sampler's argmax."""
    V, W = 2048, 3
    x = torch.zeros(G * W, V)
    x[:, [700, 9]] = 3.0
    x[:, [1999, 1030]] = 2.0     # the W-th largest value twice: the lower index is taken
    x[:, 5] = 1.0
    x = x.to(torch.bfloat16)
    score = torch.tensor([-1.0, -1.0, -2.0, -0.5, -3.0, -0.5])
    done = torch.zeros(G * W, dtype=torch.int32)
    par, tok, sc, ct, _ = run_select(dev, x, score, done, W, -1)
    assert ct[:, :W].tolist() == [[9, 700, 1030]] * (G * W) and bool((ct[:, W:] == -1).all())
    assert par.tolist() == [0, 0, 1, 0, 0, 2] and tok.tolist() == [9, 700, 9, 9, 700, 9]
    assert sc[0] == sc[1] == sc[2] and sc[3] == sc[4] == sc[5]
    # scalar path (odd V), ties across the threads' chunks, and W = 1 against the sampler
    for V in (2048, 1000, 37):
        y = torch.zeros(4, V)
        y[0, [V - 1, V // 3, 9]] = 3.0
        y[1, [V - 1, V // 2]] = 3.0
        y[2, [min(255, V - 2), min(256, V - 1)]] = 3.0
        y = y.to(torch.bfloat16)
        _, tok1, _, _, _ = run_select(dev, y, torch.zeros(4), torch.zeros(4, dtype=torch.int32), 1, -1)
        assert tok1.long().tolist() == T._sample(y, 0, dev, S_max=4).tolist() == y.float().argmax(-1).tolist()
        assert tok1.tolist() == [9, V // 2, min(255, V - 2), 0]


# ----------------------------------------------------------------------------- reorder
def forced_cand(maps, W, dev):
    """A candidate scratch whose merge gives ``maps[g][j]`` as the parent of new slot j, with token
    1000 + 10 g + j: new slot j's candidate sits at the next free rank of its parent, score -j."""
    Gq = len(maps)
    ct = torch.full((Gq * W, 8), -1, dtype=torch.int32)
    cs = torch.full((Gq * W, 8), NEG)
    for g, m in enumerate(maps):
        used = [0] * W
        for j, p in enumerate(m):
            ct[g * W + p, used[p]] = 1000 + 10 * g + j
            cs[g * W + p, used[p]] = -float(j)
            used[p] += 1
    return ct.to(dev), cs.to(dev)


REORDER_MAPS = [
    ("identity", 2, [[0, 1], [0, 1]]),
    ("swap", 2, [[1, 0], [1, 0]]),
    ("all_from_one", 4, [[2, 2, 2, 2], [2, 2, 2, 2]]),
    ("cycle3", 3, [[1, 2, 0], [1, 2, 0]]),
    ("rotate8", 8, [[1, 2, 3, 4, 5, 6, 7, 0], [7, 0, 1, 2, 3, 4, 5, 6]]),
    ("per_group", 4, [[0, 1, 2, 3], [3, 3, 0, 1]]),
]
REORDER_POS = (0, 31, 32, 127, 128, 200)
GUARD = 2048   # int32 words of sentinel on either side of every tensor


def guarded(words, dev, base):
    """A tensor of ``words`` int32 holding base + arange between two sentinel guards."""
    flat = torch.full((words + 2 * GUARD,), -7, dtype=torch.int32, device=dev)
    flat[GUARD:GUARD + words] = torch.arange(words, dtype=torch.int32, device=dev) + base
    return flat, flat[GUARD:GUARD + words]


def body_reorder(dev, H, S):
    """Every int32 word of every cache tensor and of ``tokens`` is distinct (it encodes tensor, slot,
    head, row, piece), so any misplaced 16-byte piece shows."""
    L = 2
    for name, W, maps in REORDER_MAPS:
        Bq = G * W
        n = Bq * H * S * 32
        for pos in list(REORDER_POS) + [S - 1]:
            if pos >= S:
                continue
            flats, caches = [], []
            for t in range(2 * L):
                f, body = guarded(n, dev, t * n)
                flats.append(f)
                caches.append(body.view(torch.bfloat16).view(Bq, H, S, 64))
            tf, tbody = guarded(Bq * S, dev, 1 << 30)
            tokens = tbody.view(Bq, S)
            want_c = [c.view(torch.int32).view(Bq, H, S, 32).clone() for c in caches]
            want_t = tokens.clone()
            src = torch.tensor([g * W + p for g, m in enumerate(maps) for p in m], device=dev)
            score = torch.arange(Bq, dtype=torch.float32, device=dev)
            done = torch.zeros(Bq, dtype=torch.int32, device=dev)
            length = torch.arange(Bq, dtype=torch.int32, device=dev)
            done[1] = 1
            par, tok = (torch.full((Bq,), -1, dtype=torch.int32, device=dev) for _ in range(2))
            pw = T.posw(pos, dev)
            cand = forced_cand(maps, W, dev)
            state0 = [t.clone() for t in (score, done, length, par, tok)]
            kern.beam_reorder(cand, caches[:L], caches[L:], tokens, score, done, length, par, tok, pw, W, 1001)
            what = (name, H, S, pos)
            if pos + 1 >= S:   # past the end: nothing changes at all
                assert int(pw.item()) == pos, what
                for t, t0 in zip((score, done, length, par, tok), state0):
                    assert torch.equal(t, t0), what
            else:
                for w in want_c:
                    w[:, :, :pos + 1] = w.index_select(0, src)[:, :, :pos + 1]
                want_t[:, :pos + 1] = want_t.index_select(0, src)[:, :pos + 1]
                new_tok = torch.tensor([1000 + 10 * g + j for g in range(G) for j in range(W)], dtype=torch.int32)
                want_t[:, pos + 1] = new_tok.to(dev)
                assert int(pw.item()) == pos + 1, what
                assert torch.equal(tok.cpu(), new_tok) and torch.equal(par.cpu(), (src.cpu() % W).to(torch.int32)), what
                assert torch.equal(score.cpu(), -(torch.arange(Bq) % W).float()), what
                d0, l0 = state0[1].index_select(0, src), state0[2].index_select(0, src)
                assert torch.equal(done, ((d0 != 0) | (tok == 1001)).to(torch.int32)), what
                assert torch.equal(length, l0 + (d0 == 0).to(torch.int32)), what
            for c, w, f in zip(caches, want_c, flats):
                assert torch.equal(c.view(torch.int32).view(Bq, H, S, 32), w), what
                assert bool((f[:GUARD] == -7).all()) and bool((f[-GUARD:] == -7).all()), what
            assert torch.equal(tokens, want_t), what
            assert bool((tf[:GUARD] == -7).all()) and bool((tf[-GUARD:] == -7).all()), what
            if dev.type == "cuda":
                assert int(kern._SAMPLE_TICKET[str(dev)].item()) == 0, what   # the ticket is re-armed


# ----------------------------------------------------------------------------- the search
def beam_prompt(Pn, seed=9):
    return torch.randint(0, CFG.vocab_size, (G, Pn), generator=torch.Generator().manual_seed(seed)).to(torch.int32)


def body_w1_is_greedy(dev, capture):
    model, P = T.make_model(CFG, dev, 2)
    prompt = beam_prompt(60).to(dev)
    gen = Generator(model, P, G, dev)
    greedy = gen.generate(prompt, 8, temperature=0.0, capture=capture)
    beams = gen.beam_search(prompt, 8, 1, capture=capture)
    assert beams.shape == (G, 1, 68) and beams.dtype == torch.int32
    assert torch.equal(beams[:, 0], greedy)


def body_history(dev, cfg, W, Pn, steps):
    """After each step: the cache row the step filled (row pos of every layer's K / V, every slot, as the
    reorder left it) and the step's parent / token.  At the end every slot's ancestry is followed back:
    its tokens are the ancestry's tokens and its cache row of step t is the row its ancestor held then;
    the prompt's rows are those of the slot the ancestry starts in."""
    model, P = T.make_model(cfg, dev, 2)
    Bq = G * W
    gen = Generator(model, P, Bq, dev)
    prompt = torch.randint(0, cfg.vocab_size, (G, Pn), generator=torch.Generator().manual_seed(5)).to(torch.int32)
    st = gen.beam_begin(prompt.to(dev), W)
    kv = gen.kv
    tensors = kv.k + kv.v
    pre = [t[:, :, :Pn - 1].cpu().clone() for t in tensors]
    rec = []
    for s in range(steps):
        pos = Pn - 1 + s
        gen.beam_step()
        assert int(kv.pos.item()) == pos + 1
        rec.append(([t[:, :, pos].cpu().clone() for t in tensors], st.parent.cpu().long(), st.token.cpu().clone()))
    final_tok = kv.tokens.cpu()
    final = [t.cpu() for t in tensors]
    anc = torch.arange(Bq)   # final slot b's ancestor: its slot after step s
    moved = False
    for s in range(steps - 1, -1, -1):
        rows, par, tok = rec[s]
        assert torch.equal(final_tok[:, Pn + s], tok[anc]), (W, Pn, s)
        for r, t in zip(rows, final):
            assert torch.equal(t[:, :, Pn - 1 + s], r[anc]), (W, Pn, s)
        moved = moved or s > 0 and not torch.equal(par, torch.arange(Bq) % W)
        anc = torch.arange(Bq) // W * W + par[anc]
    assert moved, "no step after the first re-routed a history: the case checks nothing"
    assert torch.equal(anc, torch.arange(Bq) // W * W)   # everything descends from slot 0
    for p0, t in zip(pre, final):
        assert torch.equal(t[:, :, :Pn - 1], p0[anc]), (W, Pn)
    assert torch.equal(final_tok[:, :Pn], prompt.repeat_interleave(W, 0))


def body_search_consistent(dev, W=3):
    """The search against the fp64 LM, step by step.  E_full = max |full_logits - lm_logits_fp64| on the
    final sequences; the decode path's logits may be 2 E_full from fp64, so a step's log-probability (a
    logit minus the lse) may be off by 4 E_full, and ``check_select``'s bound B_sel (V = 512, |score|,
    |x - gmx|, |lse| <= 64, asserted) comes on top: after s steps a score is within acc(s) =
    s (4 E_full + B_sel) of the fp64 score of its history.  Before every step the fp64 log-probabilities of
    every slot's actual history are computed; every chosen candidate's fp64 score must be no worse than the
    fp64 W-th best of the group's W x V candidates minus 2 acc(s) (the kernel's W-th best is within acc of
    it, and so is the chosen one's own score), and the fp32 scores equal the fp64 ones within acc(s)."""
    model, P = T.make_model(CFG, dev, 2)
    Pn, new, V = 60, 8, CFG.vocab_size
    Bq = G * W
    prompt = beam_prompt(Pn)
    gen = Generator(model, P, Bq, dev)
    st = gen.beam_begin(prompt.to(dev), W)
    hist = prompt.repeat_interleave(W, 0).long()
    sc64 = torch.full((Bq,), NEG, dtype=torch.float64)
    sc64[::W] = 0.0
    base = torch.arange(Bq) // W * W
    checks = []   # (step, chosen fp64 score, fp64 W-th best, |fp32 - fp64| of the new score)
    for s in range(new):
        lp = torch.log_softmax(T.lm_logits_fp64(P, CFG, hist)[:, -1], -1)   # [Bq, V] from the actual histories
        logits = gen.beam_step().float().cpu()
        assert float(logits.abs().max()) <= 32.0
        par, tok = st.parent.cpu().long(), st.token.cpu().long()
        src = base + par
        cand = (sc64[:, None] + lp).view(G, W * V)
        kth = torch.sort(cand, dim=1, descending=True).values[:, W - 1].repeat_interleave(W)
        chosen = sc64[src] + lp[src, tok]
        hist = torch.cat([hist[src], tok[:, None]], 1)
        sc64 = chosen
        got = st.score.cpu().double()
        assert float(got.abs().max()) <= 64.0
        checks.append((s + 1, chosen, kth, (got - sc64).abs()))
    assert torch.equal(hist.to(torch.int32), gen.kv.tokens[:, :Pn + new].cpu())
    padded = torch.zeros(Bq, CFG.seq_len, dtype=torch.int32)
    padded[:, :Pn + new] = hist.to(torch.int32)
    F = T.lm_logits_fp64(P, CFG, padded)[:, :Pn + new]
    f = T.full_logits(model, P, padded)[:, :Pn + new]
    e_full = float((f - F).abs().max())
    per_step = 4 * e_full + U32 * (V + 4) + 4 * U32 * (64.0 + 64.0 + 64.0)
    worst_gap = worst_sum = 0.0
    for s, chosen, kth, err in checks:
        worst_gap = max(worst_gap, float((kth - chosen).max()))
        worst_sum = max(worst_sum, float(err.max()))
    T.log_errors(name="beam_search_consistent", device=str(dev), W=W, E_full=e_full, worst_gap=worst_gap,
                 worst_sum_err=worst_sum, per_step=per_step)
    assert e_full > 0
    for s, chosen, kth, err in checks:
        assert bool((chosen >= kth - 2 * s * per_step).all()), (s, float((kth - chosen).max()), per_step)
        assert bool((err <= s * per_step).all()), (s, float(err.max()), per_step)


def body_eos(dev, capture=False):
    model, P = T.make_model(CFG, dev, 2)
    W, Pn, new = 3, 60, 8
    gen = Generator(model, P, G * W, dev)
    prompt = beam_prompt(Pn).to(dev)
    first = gen.beam_search(prompt, new, W, capture=capture)
    eos = int(first[0, 0, Pn])
    # step by step: the beam that emits eos is done at length 1 and its score never changes again
    st = gen.beam_begin(prompt, W, eos_id=eos)
    gen.beam_step()
    hit = (st.token.cpu()[:W] == eos).nonzero()[:, 0]
    assert hit.numel() == 1 and int(st.done[hit[0]]) == 1 and int(st.length[hit[0]]) == 1
    frozen = st.score[hit[0]].clone()
    for _ in range(new - 1):
        gen.beam_step()
        fin = (st.done.cpu()[:W] != 0) & (st.length.cpu()[:W] == 1)
        assert int(fin.sum()) == 1 and torch.equal(st.score[:W][fin.to(dev)][0], frozen)
    assert int((st.done.cpu()[:W] == 0).sum()) >= 1 and int(st.length.cpu()[:W].max()) == new   # the others go on
    for lp_ in (0.0, 1.0):
        out = gen.beam_search(prompt, new, W, eos_id=eos, length_penalty=lp_, pad_id=-5, capture=capture)
        raw, length = st.score.view(G, W).cpu(), st.length.view(G, W).cpu()
        rank = raw / length.clamp(min=1).float() ** lp_
        order = torch.sort(rank, dim=1, descending=True, stable=True).indices
        assert torch.equal(gen.beam_scores.cpu(), rank.gather(1, order))
        assert torch.equal(gen.beam_logprobs.cpu(), raw.gather(1, order))
        assert torch.equal(gen.lengths.cpu(), (Pn + length).gather(1, order).to(torch.int32))
        toks = gen.kv.tokens[:, :Pn + new].view(G, W, -1).cpu()
        for g in range(G):
            for r in range(W):
                n = int(gen.lengths[g, r])
                assert torch.equal(out[g, r, :n].cpu(), toks[g, order[g, r], :n])
                assert bool((out[g, r, n:] == -5).all())
        k = (gen.lengths[0].cpu() == Pn + 1).nonzero()[:, 0]
        assert k.numel() == 1 and int(out[0, k[0], Pn]) == eos
        assert gen.beam_scores[0, k[0]] == frozen
    # every slot finishes: W = 1 and eos = the greedy first token of a prompt both groups share, so every
    # slot is done after step 1 and the loop stops at the first look, after step 16
    gen1 = Generator(model, P, G, dev)
    g0 = gen1.beam_search(prompt, 1, 1, capture=capture)
    e0 = int(g0[0, 0, Pn])
    both = prompt.clone()
    both[1] = both[0]                      # both groups emit e0 first
    out = gen1.beam_search(both, 40, 1, eos_id=e0, capture=capture)
    assert gen1.beam_steps == 16 and gen1.lengths.cpu().tolist() == [[Pn + 1], [Pn + 1]]
    assert bool((out[:, 0, Pn] == e0).all()) and bool((out[:, 0, Pn + 1:] == 0).all())


# ----------------------------------------------------------------------------- CPU tests
@pytest.mark.parametrize("V,W", SELECT_SHAPES)
def test_select_vs_fp64_cpu(V, W):
    body_select(CPU, V, W)


def test_ties_cpu():
    body_ties(CPU)


@pytest.mark.parametrize("S", [128, 384])
def test_reorder_permutation_cpu(S):
    body_reorder(CPU, 2, S)


def test_w1_is_greedy_cpu():
    body_w1_is_greedy(CPU, False)


@pytest.mark.parametrize("W", [3, 4])
def test_history_cpu(W):
    body_history(CPU, CFG, W, 60, 8)


def test_history_long_cpu():
    cfg = TransformerConfig(vocab_size=512, d_model=128, n_heads=2, d_ff=512, seq_len=256, n_layers=2)
    body_history(CPU, cfg, 3, 125, 6)


def test_search_consistent_cpu():
    body_search_consistent(CPU)


def test_eos_cpu():
    body_eos(CPU)


def test_api_edges():
    model, P = T.make_model(CFG, CPU, 1)
    gen = Generator(model, P, 6, CPU)
    prompt = beam_prompt(120)
    for W in (0, 9):
        with pytest.raises(ValueError, match="num_beams"):
            gen.beam_search(prompt, 4, W)
    with pytest.raises(ValueError, match="divide"):
        gen.beam_search(prompt, 4, 4)
    with pytest.raises(ValueError, match="prompt must be"):
        gen.beam_search(prompt[:1], 4, 3)            # G * W != batch
    with pytest.raises(ValueError, match="seq_len"):
        gen.beam_search(prompt, 9, 3)
    for eos in (-1, CFG.vocab_size):
        with pytest.raises(ValueError, match="eos_id"):
            gen.beam_search(prompt, 4, 3, eos_id=eos)
    tiny = TransformerConfig(vocab_size=4, d_model=128, n_heads=2, d_ff=512, seq_len=128, n_layers=1)
    m4, P4 = T.make_model(tiny, CPU, 1)
    with pytest.raises(ValueError, match="vocabulary"):
        Generator(m4, P4, 8, CPU).beam_search(prompt[:1] % 4, 2, 8)
    with pytest.raises(ValueError, match="beam_begin"):
        Generator(model, P, 6, CPU).beam_step()
    out = gen.beam_search(prompt, 8, 3)
    assert out.shape == (G, 3, 128) and out.dtype == torch.int32
    assert torch.equal(out[:, :, :120], prompt[:, None].expand(-1, 3, -1))
    assert gen.beam_scores.shape == gen.beam_logprobs.shape == gen.lengths.shape == (G, 3)
    assert bool((gen.beam_scores[:, :-1] >= gen.beam_scores[:, 1:]).all()) and bool((gen.lengths == 128).all())
    assert gen.beam_search(prompt[:, :1], 0, 3).shape == (G, 3, 1)


def test_generate_script_beams_cpu():
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", CUDA_VISIBLE_DEVICES="")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "generate.py"), "--beams", "3", "--max-new-tokens", "4",
                        "--prompt-len", "8", "--length-penalty", "1.0"], capture_output=True, text=True, env=env,
                       cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("[generate] group")]
    assert len(lines) == 2 * 3 and "score" in lines[0]
