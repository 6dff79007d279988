"""Speculative decoding on the MI355X: the test bodies of tests/test_generate_spec.py on the HIP kernels
of csrc/spec.hip, plus the GPU-only cases (launcher return codes, HIP against the torch path, the
captured round)."""
import ctypes

import pytest
import torch

from jax_distributed_tuts_amd.ops import _lib
from jax_distributed_tuts_amd.ops import kernels as kern

from . import test_generate as T
from . import test_generate_spec as SP

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0) if torch.cuda.is_available() else None
B = SP.B


def test_greedy_judge_commit():
    SP.body_greedy_judge_commit(DEV)


def test_range_liveness():
    SP.body_range_liveness(DEV)


def test_spec_count():
    SP.body_spec_count(DEV)


def test_eos_kernel():
    SP.body_eos(DEV)


def test_sample_no_drafts():
    SP.body_sample_no_drafts(DEV)


def test_sample_distribution():
    SP.body_sample_distribution(DEV)


def test_sample_deterministic():
    SP.body_sample_deterministic(DEV)


def test_sampled_judge_matches_cpu_path():
    """Greedy: the HIP kernels and the torch path agree exactly.  Sampled: both draw from the same Philox
    words; the fp32 sums differ in order, so a handful of draws near a boundary may differ."""
    N = 512
    c0 = int(T.live8(1)[1][3])
    a = SP._draft_round(DEV, N, c0, pos=9, seed=77, top_k=50, top_p=0.9)
    b = SP._draft_round(T.CPU, N, c0, pos=9, seed=77, top_k=50, top_p=0.9)
    for x, y in zip(a[2:], b[2:]):
        assert float((x != y).double().mean()) <= 0.01


def test_return_codes():
    """Every rejection has its own code, before anything is launched: the buffers keep their sentinels."""
    L, st = _lib.lib(), _lib.stream_ptr()
    p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())  # noqa: E731
    C, V, S = 3, 64, 16
    logits = torch.zeros(B * C, V, dtype=torch.bfloat16, device=DEV)
    i32 = lambda n, v: torch.full((n,), v, dtype=torch.int32, device=DEV)  # noqa: E731
    tok = torch.full((B, S), 5, dtype=torch.int32, device=DEV)
    pos, end, count, nd = i32(B, 2), i32(B, S), i32(B, 2), i32(B, 1)
    acc, repl = i32(B * C, -7).view(B, C), i32(B * C, -7).view(B, C)
    ctr = [i32(B, 3) for _ in range(4)]
    dpos, dend = i32(B, -9), i32(B, -9)

    def judge(logits=logits, Bq=B, C=C, V=V, t=1.0, S=S, top_k=0, top_p=1.0, acc=acc):
        return L.jdt_spec_judge(p(logits), V, Bq, C, V, t, 0, 0, p(tok), S, p(pos), p(end), p(count), p(acc), p(repl),
                                top_k, top_p, st)

    def commit(Bq=B, C=C, S=S, acc=acc, dpos=dpos, dend=dend):
        return L.jdt_spec_commit(p(acc), p(repl), Bq, C, p(tok), S, p(pos), p(end), p(count), -1, *map(p, ctr),
                                 p(dpos), p(dend), st)

    def cnt(k=2, Bq=B, S=S, out=count):
        return L.jdt_spec_count(p(pos), p(end), p(nd), p(out), Bq, k, S, st)

    codes = {"null": judge(acc=None), "V": judge(V=0), "C0": judge(C=0), "C17": judge(C=17), "T": judge(t=-1.0),
             "T_nan": judge(t=float("nan")), "top_k": judge(top_k=-1), "top_p0": judge(top_p=0.0),
             "top_p": judge(top_p=1.5), "S": judge(S=0)}
    assert all(rc < 0 for rc in codes.values()), codes
    assert codes["C0"] == codes["C17"] and codes["T"] == codes["T_nan"] and codes["top_p0"] == codes["top_p"]
    assert len({codes[key] for key in ("null", "V", "C0", "T", "top_k", "top_p", "S")}) == 7, codes
    cc = {"null": commit(acc=None), "half": commit(dend=None), "C0": commit(C=0), "C17": commit(C=17), "S": commit(S=0)}
    assert all(rc < 0 for rc in cc.values()) and cc["null"] == cc["half"] == codes["null"], cc
    assert cc["C0"] == cc["C17"] == codes["C0"] and cc["S"] == codes["S"]
    kc = {"null": cnt(out=None), "k0": cnt(k=0), "k16": cnt(k=16), "S": cnt(S=0)}
    assert all(rc < 0 for rc in kc.values()) and kc["null"] == codes["null"] and kc["k0"] == kc["k16"] == codes["C0"]
    for rc in (codes["null"], codes["C0"]):
        with pytest.raises(RuntimeError):
            _lib.check(rc, "jdt_spec_judge")
    assert judge(Bq=0) == 0 and commit(Bq=0) == 0 and cnt(Bq=0) == 0
    torch.cuda.synchronize()
    assert bool((tok == 5).all()) and pos.tolist() == [2] * B and end.tolist() == [S] * B and count.tolist() == [2] * B
    assert bool((acc == -7).all()) and bool((repl == -7).all()) and all(c.tolist() == [3] * B for c in ctr)
    assert dpos.tolist() == [-9] * B and dend.tolist() == [-9] * B
    # and the Python entry points reject before they reach the launcher
    with pytest.raises(ValueError):
        kern.spec_judge(logits, tok, pos, end, count, acc, repl, top_p=0.0)


@SP.SHAPES
@SP.KINDS
@SP.KS
def test_greedy_is_greedy(case, kind, k):
    SP.body_greedy_is_greedy(DEV, *case, kind, k, capture=True)


@pytest.mark.parametrize("model_seed", [2, 5])
def test_acceptance_teeth(model_seed):
    SP.body_acceptance_teeth(DEV, model_seed)


def test_small_draft():
    SP.body_small_draft(DEV)


def test_caches_consistent():
    SP.body_caches_consistent(DEV)


def test_edges():
    SP.body_edges(DEV)


def test_cache_end():
    SP.body_cache_end(DEV)


@pytest.mark.parametrize("capture", [False, True])
def test_eos_rows(capture):
    SP.body_eos_rows(DEV, capture)


def test_sampling_mode():
    SP.body_sampling_mode(DEV)


def test_verify_hook():
    SP.body_verify_hook(DEV)


@pytest.mark.parametrize("kw", [dict(), dict(temperature=0.8, seed=11, top_k=50, top_p=0.9)], ids=["greedy", "sampled"])
@pytest.mark.parametrize("split", [False, True], ids=["one", "split"])
def test_captured_equals_eager(kw, split):
    """Tokens, lengths, the counters and the final logits are bit-equal between the captured round and
    the eager one, and a second generate replays the graph it has."""
    k, new, lens = 4, 12, [58, 60, 62]
    gen, _, _ = SP.make_pair(SP.CFG, DEV, 2, "self", split_append=split)
    prompt = torch.randint(0, SP.CFG.vocab_size, (B, max(lens)), generator=torch.Generator().manual_seed(9))
    prompt = prompt.to(torch.int32).to(DEV)
    run = lambda capture: gen.generate(prompt, new, speculative=k, capture=capture, prompt_lens=torch.tensor(lens),  # noqa: E731
                                       eos_id=None, **kw)

    def result(out):
        return [out.clone(), gen.lengths.clone(), gen.spec_drafted, gen.spec_accepted, gen.spec_emitted,
                gen.spec_state(k).last_accept.clone(), gen.logits.clone()]

    eager = result(run(False))
    rounds = gen.spec_rounds
    assert not gen._graphs
    captured = result(run(True))
    key = ("spec", k, kw.get("temperature", 0.0), kw.get("seed", 0), kw.get("top_k", 0), kw.get("top_p", 1.0), -1)
    assert list(gen._graphs) == [key] and gen._graphs[key][0] is not None
    assert gen.spec_rounds == rounds
    for a, b in zip(eager, captured):
        assert torch.equal(a, b)
    graph = gen._graphs[key][0]
    again = result(run(True))
    assert list(gen._graphs) == [key] and gen._graphs[key][0] is graph
    for a, b in zip(eager, again):
        assert torch.equal(a, b)
    assert gen.lengths.tolist() == [n + new for n in lens]
