"""Ragged prompts, top-k / top-p and EOS stopping on the MI355X: the bodies of
tests/test_generate_rows.py on the HIP kernels (csrc/attn_decode.hip, the ``_rows`` and
filtered entry points), captured steps included."""
import ctypes

import pytest
import torch

from jax_distributed_tuts_amd.ops import _lib

from . import test_generate as T
from . import test_generate_rows as R

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0) if torch.cuda.is_available() else None


def test_attn_rows():
    R.body_attn_rows(DEV)


def test_embed_rows():
    R.body_embed_rows(DEV)


def test_sample_state():
    R.body_sample_state(DEV)


def test_draw_identity():
    R.body_draw_identity(DEV)


@R.ROWS
def test_topk_argmax(rows):
    R.body_topk_argmax(DEV, rows)


@R.ROWS
def test_topk_ties(rows):
    R.body_topk_ties(DEV, rows)


@R.ROWS
def test_filter_distribution(rows):
    R.body_filter_distribution(DEV, rows)


@R.ROWS
def test_filter_random(rows):
    R.body_filter_random(DEV, rows)


@R.ROWS
def test_filter_deterministic(rows):
    R.body_filter_deterministic(DEV, rows)


def test_filter_return_codes():
    """A bad top_k / top_p: a non-zero code before anything is launched, on both entry points."""
    B = 3
    L = _lib.lib()
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    logits = torch.zeros(B, 64, dtype=torch.bfloat16, device=DEV)
    tok = torch.full((B, 16), 5, dtype=torch.int32, device=DEV)
    ticket = torch.zeros(1, dtype=torch.int32, device=DEV)
    for top_k, top_p in ((-1, 1.0), (0, 0.0), (0, 1.5)):
        pw, pr = T.posw(0, DEV), R.posr([0] * B, DEV)
        end = R.posr([16] * B, DEV)
        rcs = {"jdt_sample_filtered": L.jdt_sample_filtered(p(logits), 64, B, 64, 1.0, 0, 0, p(tok), 16, p(pw),
                                                             p(ticket), top_k, top_p, _lib.stream_ptr()),
               "jdt_sample_rows": L.jdt_sample_rows(p(logits), 64, B, 64, 1.0, 0, 0, p(tok), 16, p(pr), p(end), -1,
                                                     top_k, top_p, _lib.stream_ptr())}
        for name, rc in rcs.items():
            assert rc != 0, (name, top_k, top_p)
            with pytest.raises(RuntimeError):
                _lib.check(rc, name)
        torch.cuda.synchronize()
        assert bool((tok == 5).all()) and int(pw.item()) == 0 and pr.tolist() == [0] * B and end.tolist() == [16] * B
        assert int(ticket.item()) == 0
    rc = L.jdt_sample_rows(p(logits), 64, B, 64, 1.0, 0, 0, p(tok), 0, p(pr), p(end), -1, 0, 1.0, _lib.stream_ptr())
    assert rc != 0   # S_max 0


@pytest.mark.parametrize("capture", [False, True])
def test_ragged_equals_uniform(capture):
    gen = R.body_ragged_equals_uniform(DEV, capture)
    if capture:   # one graph per ragged sampler setting, under the longer key
        assert len(gen._graphs) == len(R.SETTINGS) and all(len(k) > 2 for k in gen._graphs)


def test_default_key_stays():
    """A call with none of the new options still caches its graph under (temperature, seed)."""
    model, P = T.make_model(T.CFG, DEV, 3)
    gen = R.Generator(model, P, 2, DEV)
    prompt = R.ragged_prompt([20, 20]).to(DEV)
    gen.generate(prompt, 3, temperature=0.8, seed=11)
    assert list(gen._graphs) == [(0.8, 11)] and gen._graphs[(0.8, 11)][0] is not None
    plain = gen.generate(prompt, 3, temperature=0.8, seed=11)
    gen.generate(prompt, 3, temperature=0.8, seed=11, top_k=5)
    assert len(gen._graphs) == 2
    assert torch.equal(gen.generate(prompt, 3, temperature=0.8, seed=11), plain)


def test_teacher_forced_ragged():
    R.body_teacher_forced_ragged(DEV)


@pytest.mark.parametrize("capture", [False, True])
def test_eos(capture):
    R.body_eos(DEV, capture)


def test_eos_early_stop():
    R.body_eos_early_stop(DEV)
