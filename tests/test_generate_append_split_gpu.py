"""Split-KV append attention on the MI355X (csrc/attn_append.hip, ``jdt_attn_append_split`` /
``_rows``: one workgroup per (query tile, 512-key span) and a combine launch) against fp64, against
the one-launch kernel and bit for bit across every way of cutting a sequence into calls, then
``Generator(split_append=True)`` at the model level.

Kernel shapes: B = 3, H in {2, 8}, a cache of 2 * SPAN + 69 rows -- two full spans and a third whose
last key tile is partial -- with chunks that start and end on both sides of the span seams.  Bounds
are the project's own: e <= 2 e_ref against fp64 at the kernel level (e_ref: the one-launch kernel on
the same inputs), E_dec <= 2 E_full and a worst greedy gap of 4 E_full at the model level."""
import ctypes
import dataclasses

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
B = TA.B
SPAN = kern.AP_SPAN_ROWS
S = 2 * SPAN + 69
posr = TA.posr


def ws_for(H, C, S_max=S, Bq=B, fill=0.0, extra=0):
    n = kern.attention_append_ws_floats(Bq, H, C, S_max)
    return torch.full((n + extra,), fill, dtype=torch.float32, device=DEV)


def run_split(qkv, kc, vc, pos, H, C, count=None, o=None, ws=None):
    """attention_append through the split pair on device copies: (o, k_cache, v_cache)."""
    k2, v2 = kc.to(DEV).clone(), vc.to(DEV).clone()
    if ws is None:
        ws = ws_for(H, C, S_max=kc.shape[2], Bq=kc.shape[0])
    got = kern.attention_append(qkv.to(DEV), k2, v2, pos, H, C, count=count, out=o, ws=ws)
    return got, k2, v2


def run_one(qkv, kc, vc, pos, H, C, count=None, o=None):
    return TA.run_append(DEV, qkv, kc, vc, pos, H, C, count=count, o=o)


def rows_of(qkv, Bq, C, lo, hi):
    """Tokens lo..hi-1 of every sequence of a [Bq*C, w] chunk as a chunk of their own."""
    return qkv.view(Bq, C, -1)[:, lo:hi].reshape(Bq * (hi - lo), -1).contiguous()


# ----------------------------------------------------------------------------- 1. against fp64
@pytest.mark.parametrize("H", [2, 8])
@pytest.mark.parametrize("p,C", [(p, C) for p in (0, SPAN - 1, SPAN, SPAN + 1, SPAN - 70, 2 * SPAN - 64, 2 * SPAN + 1)
                                 for C in (1, 17, 64, 65, 130) if p + C <= S])
def test_split_vs_fp64(p, C, H):
    """e_split <= 2 e_ref with e_ref the fp64 error of the one-launch kernel on the same inputs; rows
    below the first seam have the one-launch bits, and so do the caches."""
    qkv, kc, vc = TA.append_inputs(H, C, seed=1000 * H + 10 * p + C, S_max=S)
    want, _ = TA.attn_append_fp64(qkv, kc, vc, p, C, H)
    got, k2, v2 = run_split(qkv, kc, vc, T.posw(p, DEV), H, C)
    ref, k1, v1 = run_one(qkv, kc, vc, T.posw(p, DEV), H, C)
    got, ref = got.view(B, C, -1), ref.view(B, C, -1)
    e_ref = float((ref.cpu().double() - want).abs().max())
    e_split = float((got.cpu().double() - want).abs().max())
    T.log_errors(name="attention_append_split", p=p, C=C, H=H, e_split=e_split, e_ref=e_ref)
    assert e_split <= 2 * e_ref, (e_split, e_ref)
    one_span = max(0, min(C, SPAN - p))   # rows i with p + i < SPAN
    assert torch.equal(got[:, :one_span], ref[:, :one_span])
    assert torch.equal(k2, k1) and torch.equal(v2, v1)


# ----------------------------------------------------------------------------- 2. one span
@pytest.mark.parametrize("H", [2, 8])
@pytest.mark.parametrize("p,C", [(p, C) for p in (0, 63, 200) for C in (1, 64, 65)])
def test_one_span_has_the_one_launch_bits(p, C, H):
    """A 320-row cache is one span: o and both caches equal the one-launch kernel's bit for bit."""
    qkv, kc, vc = TA.append_inputs(H, C, seed=7000 + 100 * H + 10 * p + C)
    got, k2, v2 = run_split(qkv, kc, vc, T.posw(p, DEV), H, C)
    ref, k1, v1 = run_one(qkv, kc, vc, T.posw(p, DEV), H, C)
    assert torch.equal(got, ref) and torch.equal(k2, k1) and torch.equal(v2, v1)


# ----------------------------------------------------------------------------- 3. cutting leaves the bits alone
@pytest.mark.parametrize("H", [2, 8])
def test_cutting_leaves_the_bits_alone(H):
    """192 tokens from p0 = SPAN - 100 in one call, as 64 + 64 + 64 and as 1 + 100 + 91: the same o
    rows and caches bit for bit; two identical calls are bit-equal; the result is close to fp64."""
    p0, N = SPAN - 100, 192
    qkv, kc, vc = TA.append_inputs(H, N, seed=20 + H, S_max=S)
    one, k1, v1 = run_split(qkv, kc, vc, T.posw(p0, DEV), H, N)
    again, k1b, v1b = run_split(qkv, kc, vc, T.posw(p0, DEV), H, N)
    assert torch.equal(one, again) and torch.equal(k1, k1b) and torch.equal(v1, v1b)
    want, _ = TA.attn_append_fp64(qkv, kc, vc, p0, N, H)
    T.close(one.view(B, N, -1), want)
    for cuts in ((64, 64, 64), (1, 100, 91)):
        k2, v2 = kc.to(DEV).clone(), vc.to(DEV).clone()
        outs, lo = [], 0
        for C in cuts:
            part = rows_of(qkv, B, N, lo, lo + C).to(DEV)
            outs.append(kern.attention_append(part, k2, v2, T.posw(p0 + lo, DEV), H, C,
                                              ws=ws_for(H, C)).view(B, C, -1))
            lo += C
        assert torch.equal(torch.cat(outs, 1), one.view(B, N, -1)), cuts
        assert torch.equal(k2, k1) and torch.equal(v2, v1), cuts


# ----------------------------------------------------------------------------- 4. dirty workspace
@pytest.mark.parametrize("p,C", [(SPAN - 70, 130), (2 * SPAN + 1, 64)])
def test_dirty_workspace(p, C):
    """A NaN-filled workspace and one larger than needed give the bits of a zeroed exact-size one:
    the combine reads only what the split launch of the same call wrote."""
    H = 2
    qkv, kc, vc = TA.append_inputs(H, C, seed=40 + C, S_max=S)
    clean, k1, v1 = run_split(qkv, kc, vc, T.posw(p, DEV), H, C, ws=ws_for(H, C))
    assert not bool(clean.isnan().any())
    for ws in (ws_for(H, C, fill=float("nan")), ws_for(H, C, extra=1000), ws_for(H, C, fill=float("nan"), extra=77)):
        got, k2, v2 = run_split(qkv, kc, vc, T.posw(p, DEV), H, C, ws=ws)
        assert torch.equal(got, clean) and torch.equal(k2, k1) and torch.equal(v2, v1)


# ----------------------------------------------------------------------------- 5. per row
@pytest.mark.parametrize("H", [2, 8])
def test_per_row_has_the_bits_of_the_shared_position(H):
    pos, count, C = [0, SPAN - 10, 2 * SPAN + 3], [64, 40, 0], 64
    qkv, kc, vc = TA.append_inputs(H, C, seed=30 + H, S_max=S)
    o = torch.full((B * C, H * 64), 7.0, dtype=torch.bfloat16, device=DEV)
    got, k2, v2 = run_split(qkv, kc, vc, posr(pos, DEV), H, C, count=posr(count, DEV), o=o)
    got = got.view(B, C, -1)
    for b, (p, n) in enumerate(zip(pos, count)):
        assert bool((got[b, n:] == 7.0).all())
        if n == 0:
            assert torch.equal(k2[b].cpu(), kc[b]) and torch.equal(v2[b].cpu(), vc[b])
            continue
        ref, rk, rv = run_split(rows_of(qkv, B, C, 0, n), kc, vc, T.posw(p, DEV), H, n)
        assert torch.equal(got[b, :n], ref.view(B, n, -1)[b])
        assert torch.equal(k2[b], rk[b]) and torch.equal(v2[b], rv[b])


# ----------------------------------------------------------------------------- 6. out of range
def test_out_of_range():
    """p = -1 and p + n = S + 1 write nothing, shared and per row; a bad row among good rows leaves
    the good rows the bits of their solo calls."""
    H, C = 2, 64
    qkv, kc, vc = TA.append_inputs(H, C, seed=3, S_max=S)
    for p in (-1, S - C + 1):
        o = torch.full((B * C, H * 64), 7.0, dtype=torch.bfloat16, device=DEV)
        _, k2, v2 = run_split(qkv, kc, vc, T.posw(p, DEV), H, C, o=o)
        assert torch.equal(k2.cpu(), kc) and torch.equal(v2.cpu(), vc) and bool((o == 7.0).all())
    for bad_p, bad_n in ((-1, 5), (S - 4, 5)):
        for b_bad in range(B):
            pos, count = [5, SPAN - 3, 2 * SPAN + 3], [64, 7, 1]
            pos[b_bad], count[b_bad] = bad_p, bad_n
            o = torch.full((B * C, H * 64), 7.0, dtype=torch.bfloat16, device=DEV)
            got, k2, v2 = run_split(qkv, kc, vc, posr(pos, DEV), H, C, count=posr(count, DEV), o=o)
            o3 = got.view(B, C, -1)
            for b in range(B):
                n = count[b]
                if b == b_bad:
                    assert torch.equal(k2[b].cpu(), kc[b]) and torch.equal(v2[b].cpu(), vc[b])
                    assert bool((o3[b] == 7.0).all())
                    continue
                ref, rk, rv = run_split(rows_of(qkv, B, C, 0, n), kc, vc, T.posw(pos[b], DEV), H, n)
                assert torch.equal(o3[b, :n], ref.view(B, n, -1)[b]) and bool((o3[b, n:] == 7.0).all())
                assert torch.equal(k2[b], rk[b]) and torch.equal(v2[b], rv[b])


# ----------------------------------------------------------------------------- 7. return codes
def call_split(qkv, kc, vc, o, pos, count, ws, ws_floats, H, C, *, Bq=B, Dh=64, S_max=None, qkv_ptr=None, kc_ptr=None,
               null=()):
    """The raw launcher (per-row when ``count`` is given); returns its code.  ``null``: names of
    pointer arguments passed as NULL."""
    ptr = {k: (None if k in null or t is None else ctypes.c_void_p(t.data_ptr()))
           for k, t in dict(qkv=qkv, kc=kc, vc=vc, o=o, pos=pos, count=count, ws=ws).items()}
    if qkv_ptr is not None:
        ptr["qkv"] = ctypes.c_void_p(qkv_ptr)
    if kc_ptr is not None:
        ptr["kc"] = ctypes.c_void_p(kc_ptr)
    tail = (ptr["ws"], ws_floats, Bq, C, H, Dh, kc.shape[2] if S_max is None else S_max, 0.125, _lib.stream_ptr())
    if count is None:
        return _lib.lib().jdt_attn_append_split(ptr["qkv"], ptr["kc"], ptr["vc"], ptr["o"], ptr["pos"], *tail)
    return _lib.lib().jdt_attn_append_split_rows(ptr["qkv"], ptr["kc"], ptr["vc"], ptr["o"], ptr["pos"], ptr["count"],
                                                 *tail)


@pytest.mark.parametrize("rows", [False, True])
def test_split_return_codes(rows):
    """Every rejection comes before anything is launched: o, the caches and the workspace keep their
    sentinels (every buffer is large enough for the shape named anyway)."""
    H = 2

    def case(Dh=64, S_max=S, C=64, Bq=B, short=0, **kw):
        Cb = min(max(C, 1), 1025)
        qkv = torch.zeros(B * Cb, 3 * H * Dh + 8, dtype=torch.bfloat16, device=DEV)
        kc = torch.full((B, H, max(min(max(S_max, 1), S), Cb) + 1, Dh), 3.0, dtype=torch.bfloat16, device=DEV)
        vc = kc.clone()
        o = torch.full((B * Cb, H * Dh), 7.0, dtype=torch.bfloat16, device=DEV)
        need = kern.attention_append_ws_floats(B, H, Cb, max(min(S_max, S), 1))
        ws = torch.full((need,), 5.0, dtype=torch.float32, device=DEV)
        pos = posr([0] * B, DEV) if rows else T.posw(0, DEV)
        count = posr([1] * B, DEV) if rows else None
        if kw.pop("misaligned", None) == "qkv":
            kw["qkv_ptr"] = qkv.data_ptr() + 8
        elif "kc_mis" in kw:
            kw.pop("kc_mis")
            kw["kc_ptr"] = kc.data_ptr() + 8
        rc = call_split(qkv, kc, vc, o, pos, count, ws, need - short, H, C, Bq=Bq, Dh=Dh, S_max=S_max, **kw)
        torch.cuda.synchronize()
        assert bool((o == 7.0).all()) and bool((kc == 3.0).all()) and bool((vc == 3.0).all())
        assert bool((ws == 5.0).all())
        return rc

    name = "jdt_attn_append_split_rows" if rows else "jdt_attn_append_split"
    assert case(Dh=32) == -3 and case(Dh=128) == -3
    assert case(S_max=0) == -4 and case(S_max=32769) == -4
    for arg in ("qkv", "kc", "vc", "o", "pos", "ws") + (("count",) if rows else ()):
        assert case(null=(arg,)) == -2, arg
    assert case(misaligned="qkv") == -6 and case(kc_mis=True) == -6
    assert case(C=0) == -11 and case(C=1025) == -11
    assert case(Bq=65536) == -5
    assert case(short=1) == -10 and case(short=1, C=130) == -10 and case(short=1, S_max=SPAN) == -10
    for rc in (-2, -3, -4, -5, -6, -10, -11):
        with pytest.raises(RuntimeError):
            _lib.check(rc, name)
    assert case(Bq=0) == 0   # a no-op


# ----------------------------------------------------------------------------- 8. top of the envelope
def test_longest_cache_accepted():
    """S_max = 32768, 64 spans: the last 64 rows appended at once; one row further writes nothing."""
    H, S_max, C = 1, 32768, 64
    p = S_max - C
    qkv, kc, vc = TA.append_inputs(H, C, seed=4, Bq=1, S_max=S_max)
    got, k2, v2 = run_split(qkv, kc, vc, T.posw(p, DEV), H, C)
    want, _ = TA.attn_append_fp64(qkv, kc, vc, p, C, H)
    T.close(got.view(1, C, -1), want)
    kc[:, :, p:], vc[:, :, p:] = TA.chunk_kv(qkv, 1, C, H)
    assert torch.equal(k2.cpu(), kc) and torch.equal(v2.cpu(), vc)
    o = torch.full((C, 64), 7.0, dtype=torch.bfloat16, device=DEV)
    _, k3, v3 = run_split(qkv, k2, v2, T.posw(p + 1, DEV), H, C, o=o)   # one row too far: nothing is written
    assert bool((o == 7.0).all()) and torch.equal(k3, k2) and torch.equal(v3, v2)


# ----------------------------------------------------------------------------- 9. model level
CFG = dataclasses.replace(TL.CFG_LONG, seq_len=2 * SPAN + 64)
_LM: dict = {}


def lm_shared():
    """One model and its references, shared by the tests (never modified): (model, P, true tokens
    [B, seq_len], fp64 logits, the existing forward's logits)."""
    if not _LM:
        model, P = T.make_model(CFG, DEV, 0)
        tok = torch.randint(0, CFG.vocab_size, (B, CFG.seq_len), generator=torch.Generator().manual_seed(1))
        tok = tok.to(torch.int32)
        _LM["lm"] = (model, P, tok, T.lm_logits_fp64(P, CFG, tok), T.full_logits(model, P, tok))
    return _LM["lm"]


@pytest.mark.parametrize("chunk", [64, 100])
@pytest.mark.parametrize("Pn", [SPAN + 70, 2 * SPAN + 3])
def test_teacher_forced_split(Pn, chunk):
    """body_teacher_forced_chunked's construction with split_append: prefill(chunk=), then
    teacher-forced steps at the next three positions, E_dec <= 2 E_full; the position and the tokens
    are the plain chunked generator's, and so is layer 0's cache (its inputs are the same bits)."""
    model, P, tok, F, f = lm_shared()
    gen = Generator(model, P, B, DEV, split_append=True)
    gen.prefill(tok[:, :Pn].to(DEV), chunk=chunk)
    H = CFG.n_heads
    assert gen.kv.append_ws.numel() >= kern.attention_append_ws_floats(B, H, chunk, CFG.seq_len)
    ref = Generator(model, P, B, DEV)
    ref.prefill(tok[:, :Pn].to(DEV), chunk=chunk)
    assert ref.kv.append_ws is None
    assert int(gen.kv.pos.item()) == int(ref.kv.pos.item()) == Pn - 1 and not gen.kv.per_row
    assert torch.equal(gen.kv.tokens, ref.kv.tokens)
    assert torch.equal(gen.kv.k[0], ref.kv.k[0]) and torch.equal(gen.kv.v[0], ref.kv.v[0])
    for l in range(1, CFG.n_layers):
        T.close(gen.kv.k[l][:, :, :Pn - 1], ref.kv.k[l][:, :, :Pn - 1])
        T.close(gen.kv.v[l][:, :, :Pn - 1], ref.kv.v[l][:, :, :Pn - 1])
    gen.kv.tokens.copy_(tok.to(DEV))
    e_full = e_dec = 0.0
    for p in range(Pn - 1, Pn + 2):
        d = gen.step(sample=False)
        e_full = max(e_full, float((f[:, p] - F[:, p]).abs().max()))
        e_dec = max(e_dec, float((d.detach().cpu().double() - F[:, p]).abs().max()))
    assert int(gen.kv.pos.item()) == Pn + 2
    T.log_errors(name="teacher_forced_split", P=Pn, chunk=chunk, E_full=e_full, E_dec=e_dec)
    assert e_full > 0
    assert e_dec <= 2 * e_full, (e_dec, e_full)


def test_extend_logits_split():
    """60 tokens from P = SPAN - 30 in one extend (its rows cross the first seam): the returned
    logits are within 2 E_full of fp64 at their position."""
    model, P, tok, F, f = lm_shared()
    P0, n = SPAN - 30, 60
    gen = Generator(model, P, B, DEV, split_append=True)
    gen.prefill(tok[:, :P0].to(DEV), chunk=64)
    got = gen.extend(tok[:, P0:P0 + n].to(DEV), logits=True)
    at = P0 + n - 2   # the last processed token
    assert int(gen.kv.pos.item()) == at + 1 and got.shape == (B, CFG.vocab_size)
    assert torch.equal(gen.kv.tokens[:, :P0 + n].cpu(), tok[:, :P0 + n])
    e_full = float((f[:, at] - F[:, at]).abs().max())
    e_ext = float((got.detach().cpu().double() - F[:, at]).abs().max())
    T.log_errors(name="extend_logits_split", E_full=e_full, E_ext=e_ext)
    assert e_full > 0
    assert e_ext <= 2 * e_full, (e_ext, e_full)


def greedy_gap(P, model, seq, starts, new):
    """(E_full, worst gap) of body_greedy_chunked / body_ragged: rows b generated tokens starts[b] ..
    starts[b] + new - 1 of ``seq`` [B, <= seq_len]."""
    padded = torch.zeros(B, CFG.seq_len, dtype=torch.int32)
    padded[:, :seq.shape[1]] = seq
    F = T.lm_logits_fp64(P, CFG, padded)
    f = T.full_logits(model, P, padded)
    e_full = worst = 0.0
    for b, n in enumerate(starts):
        e_full = max(e_full, float((f[b, :n + new] - F[b, :n + new]).abs().max()))
        for t in range(n, n + new):
            worst = max(worst, float(F[b, t - 1].max() - F[b, t - 1, padded[b, t].long()]))
    return e_full, worst


def test_greedy_split_captured_equals_eager():
    """generate(prefill_chunk=64) with split_append, prompt SPAN + 20 and 8 new tokens: eager and
    captured runs give the same tokens and last logits bit for bit, the step really was captured, and
    the worst greedy gap is within 4 E_full."""
    model, P = T.make_model(CFG, DEV, 2)
    Pn, new = SPAN + 20, 8
    prompt = torch.randint(0, CFG.vocab_size, (B, Pn), generator=torch.Generator().manual_seed(9)).to(torch.int32)
    runs = []
    for capture in (False, True):
        gen = Generator(model, P, B, DEV, split_append=True)
        seq = gen.generate(prompt.to(DEV), new, temperature=0.0, capture=capture, prefill_chunk=64).cpu()
        assert gen.prefill_rows == 0 and gen.kv.append_ws is not None
        assert seq.shape == (B, Pn + new) and seq.dtype == torch.int32 and torch.equal(seq[:, :Pn], prompt)
        runs.append((gen, seq, gen.logits.clone()))
    (gen_e, eager, logits_e), (gen_c, graph, logits_c) = runs
    assert torch.equal(graph, eager) and torch.equal(logits_c, logits_e)
    assert gen_c._graphs[gen_c._graph_key()][0] is not None
    assert not gen_e._graphs
    e_full, worst = greedy_gap(P, model, eager, [Pn] * B, new)
    T.log_errors(name="greedy_split", E_full=e_full, worst_gap=worst)
    assert worst <= 4 * e_full, (worst, e_full)


def test_ragged_generate_split():
    """A ragged generate with prompt lengths on both sides of the first seam meets the same gap bound."""
    model, P, tok, _, _ = lm_shared()
    lens, new = [SPAN - 5, SPAN + 40, 2 * SPAN + 10], 8
    gen = Generator(model, P, B, DEV, split_append=True)
    seq = gen.generate(tok[:, :max(lens)].to(DEV), new, temperature=0.0, prompt_lens=torch.tensor(lens),
                       prefill_chunk=64).cpu()
    assert gen.kv.per_row and gen.lengths.tolist() == [n + new for n in lens]
    for b, n in enumerate(lens):
        assert torch.equal(seq[b, :n], tok[b, :n])
    e_full, worst = greedy_gap(P, model, seq, lens, new)
    T.log_errors(name="ragged_split", E_full=e_full, worst_gap=worst)
    assert worst <= 4 * e_full, (worst, e_full)
