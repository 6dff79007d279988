"""Beam search on the MI355X: the test bodies of tests/test_generate_beam.py on the HIP kernels of
csrc/beam.hip, plus the kernel-level cases (launcher return codes, the captured beam step)."""
import ctypes

import pytest
import torch

from jax_distributed_tuts_amd.generation import Generator
from jax_distributed_tuts_amd.models.transformer import TransformerConfig
from jax_distributed_tuts_amd.ops import _lib
from jax_distributed_tuts_amd.ops import kernels as kern

from . import test_generate as T
from . import test_generate_beam as TB

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0) if torch.cuda.is_available() else None
G = TB.G
LONG_CFG = TransformerConfig(vocab_size=512, d_model=128, n_heads=2, d_ff=512, seq_len=256, n_layers=2)


@pytest.mark.parametrize("V,W", TB.SELECT_SHAPES)
def test_select_vs_fp64(V, W):
    TB.body_select(DEV, V, W)


def test_select_matches_cpu_path():
    """The HIP kernels and the torch path agree on the candidates' tokens and the merge exactly."""
    logits, score, done = TB.select_inputs(512, 3, 51203)
    assert TB.select_precondition(TB.select_fp64(logits, score, done, 3, 509), 3)
    a =TB.run_select(DEV, logits, score, done, 3, 509)
    b = TB.run_select(T.CPU, logits, score, done, 3, 509)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[3], b[3])


def test_ties():
    TB.body_ties(DEV)


def test_topw_past_the_end():
    logits, score, done = TB.select_inputs(512, 2, 1)
    ct = torch.full((4, 8), 77, dtype=torch.int32, device=DEV)
    cs = torch.full((4, 8), 7.0, device=DEV)
    for pos in (3, 9, -1):
        kern.beam_topw(logits.to(DEV), score.to(DEV), done.to(DEV), T.posw(pos, DEV), 2, 509, seq_len=4, out=(ct, cs))
    torch.cuda.synchronize()
    assert bool((ct == 77).all()) and bool((cs == 7.0).all())


@pytest.mark.parametrize("S", [128, 384])
@pytest.mark.parametrize("H", [2, 8])
def test_reorder_permutation(H, S):
    TB.body_reorder(DEV, H, S)


def test_bad_shapes_return_codes():
    """Every bad shape: a non-zero code before anything is launched, sentinel buffers unchanged."""
    L = _lib.lib()
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    B, V, W, H, S = 4, 64, 2, 2, 16
    logits = torch.zeros(B, V, dtype=torch.bfloat16, device=DEV)
    score = torch.full((B,), 3.0, device=DEV)
    done, length, par, tok = (torch.full((B,), 5, dtype=torch.int32, device=DEV) for _ in range(4))
    ct = torch.full((B, 8), 77, dtype=torch.int32, device=DEV)
    cs = torch.full((B, 8), 7.0, device=DEV)
    tokens = torch.full((B, S), 5, dtype=torch.int32, device=DEV)
    pw = T.posw(0, DEV)
    ticket = torch.zeros(1, dtype=torch.int32, device=DEV)
    big = torch.full((B * H * S * 64 + 8,), 3.0, dtype=torch.bfloat16, device=DEV)
    kc = big[:B * H * S * 64].view(B, H, S, 64)
    off = big[4:4 + B * H * S * 64].view(B, H, S, 64)   # 8 bytes past a 16-byte boundary
    st = _lib.stream_ptr()

    def topw(logits_=p(logits), ld=V, B_=B, V_=V, W_=W, eos=-1, S_=S):
        return L.jdt_beam_topw(logits_, ld, B_, V_, W_, p(score), p(done), eos, p(ct), p(cs), p(pw), S_, st)

    assert topw(logits_=None) != 0
    assert topw(W_=0) != 0 and topw(W_=9) != 0
    assert topw(B_=3) != 0                       # B % W
    assert topw(V_=1, ld=1) != 0                 # W > V
    assert topw(ld=V - 1) != 0
    assert topw(eos=V) != 0
    assert topw(S_=0) != 0 and topw(S_=32769) != 0

    def reorder(caches=(kc, kc), B_=B, W_=W, Dh=64, S_=S, tokens_=p(tokens)):
        dev_tab, host_tab = kern.cache_ptr_table(list(caches))
        return L.jdt_beam_reorder(p(ct), p(cs), p(dev_tab), host_tab, len(caches), tokens_, p(score), p(done),
                                  p(length), p(par), p(tok), p(pw), p(ticket), B_, W_, H, Dh, S_, -1, st)

    assert reorder(tokens_=None) != 0
    assert reorder(W_=0) != 0 and reorder(W_=9) != 0
    assert reorder(B_=3) != 0
    assert reorder(Dh=32) != 0 and reorder(Dh=128) != 0
    assert reorder(S_=0) != 0 and reorder(S_=32769) != 0
    assert reorder(caches=(kc, off)) != 0        # a misaligned cache
    with pytest.raises(RuntimeError):
        _lib.check(reorder(Dh=32), "jdt_beam_reorder")
    torch.cuda.synchronize()
    assert bool((ct == 77).all()) and bool((cs == 7.0).all()) and bool((tokens == 5).all()) and bool((big == 3.0).all())
    assert bool((score == 3.0).all()) and int(pw.item()) == 0 and int(ticket.item()) == 0
    for t in (done, length, par, tok):
        assert bool((t == 5).all())


@pytest.mark.parametrize("capture", [False, True])
def test_w1_is_greedy(capture):
    TB.body_w1_is_greedy(DEV, capture)


@pytest.mark.parametrize("W", [3, 4])
def test_history(W):
    TB.body_history(DEV, TB.CFG, W, 60, 8)


def test_history_long():
    """seq_len 256, P = 125: the split-KV decode path, and the steps cross the 128-row chunk edge."""
    TB.body_history(DEV, LONG_CFG, 3, 125, 6)


def test_search_consistent():
    TB.body_search_consistent(DEV)


@pytest.mark.parametrize("eos", [False, True])
def test_captured_equals_eager(eos):
    model, P = T.make_model(TB.CFG, DEV, 3)
    W = 4
    gen = Generator(model, P, G * W, DEV)
    prompt = TB.beam_prompt(60, seed=4).to(DEV)
    eos_id = None
    if eos:
        eos_id = int(gen.beam_search(prompt, 8, W, capture=False)[0, 0, 60])
    eager = gen.beam_search(prompt, 8, W, eos_id=eos_id, length_penalty=0.5, capture=False)
    want = (eager, gen.beam_scores.clone(), gen.lengths.clone(), gen.beam_logprobs.clone())
    for _ in range(2):   # the call that captures, then one that only replays
        got = gen.beam_search(prompt, 8, W, eos_id=eos_id, length_penalty=0.5, capture=True)
        for a, b in zip((got, gen.beam_scores, gen.lengths, gen.beam_logprobs), want):
            assert torch.equal(a, b)
    assert gen._graphs[("beam", W, -1 if eos_id is None else eos_id)][0] is not None   # really captured


@pytest.mark.parametrize("capture", [False, True])
def test_eos(capture):
    TB.body_eos(DEV, capture)
