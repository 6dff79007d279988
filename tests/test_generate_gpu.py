"""KV-cache generation on the MI355X: the HIP decode kernels (csrc/attn_decode.hip) against
fp64, and the test bodies of tests/test_generate.py on the GPU."""
import ctypes

import pytest
import torch

from jax_distributed_tuts_amd.generation import Generator
from jax_distributed_tuts_amd.models.transformer import TransformerConfig
from jax_distributed_tuts_amd.ops import _lib
from jax_distributed_tuts_amd.ops import kernels as kern

from . import test_generate as T

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0) if torch.cuda.is_available() else None
B = T.B


@pytest.mark.parametrize("H", [2, 8])
@pytest.mark.parametrize("pos", [0, 1, 62, 63, 64, 65, 126, 127])
def test_attention_decode_vs_fp64(pos, H):
    """e_dec <= 2 e_ref: the decode kernel against fp64, measured with the error of row
    ``pos`` of the existing attention_fwd kernel on the equivalent full sequence (same bf16
    inputs, same rounding points; the factor covers the different summation order)."""
    S, d = 128, H * 64
    qkv, kc, vc = T.decode_inputs(B, H, seed=100 * H + pos)
    want, _ = T.attn_decode_fp64(qkv, kc, vc, pos, H)
    got = kern.attention_decode(qkv.to(DEV), kc.to(DEV).clone(), vc.to(DEV).clone(), T.posw(pos, DEV), H)
    # the same problem as row pos of a full causal sequence (rows > pos cannot reach row pos)
    full = torch.randn(B, S, 3, H, 64, generator=torch.Generator().manual_seed(1)).to(torch.bfloat16)
    full[:, :pos, 1] = kc[:, :, :pos].permute(0, 2, 1, 3)
    full[:, :pos, 2] = vc[:, :, :pos].permute(0, 2, 1, 3)
    full[:, pos] = qkv.view(B, 3, H, 64)
    o_full, _ = kern.attention_fwd(full.view(B * S, 3 * d).to(DEV), B, S, H)
    e_ref = float((o_full.view(B, S, d)[:, pos].cpu().double() - want).abs().max())
    e_dec = float((got.cpu().double() - want).abs().max())
    T.log_errors(name="attention_decode", pos=pos, H=H, e_dec=e_dec, e_ref=e_ref)
    assert e_dec <= 2 * e_ref, (e_dec, e_ref)
    cpu = kern.attention_decode(qkv, kc.clone(), vc.clone(), T.posw(pos, T.CPU), H)
    T.close(got, cpu)


def test_needle():
    T.body_needle(DEV)


def test_cache_append():
    T.body_cache_append(DEV)
    for H in (8,):   # more workgroups than one batch row's heads
        qkv, kc, vc = T.decode_inputs(B, H, seed=5)
        k2, v2 = kc.to(DEV), vc.to(DEV)
        kern.attention_decode(qkv.to(DEV), k2, v2, T.posw(33, DEV), H)
        kc[:, :, 33] = qkv.view(B, 3, H, 64)[:, 1]
        vc[:, :, 33] = qkv.view(B, 3, H, 64)[:, 2]
        assert torch.equal(k2.cpu(), kc) and torch.equal(v2.cpu(), vc)


def test_out_of_range():
    T.body_out_of_range(DEV)


def test_bad_shapes_return_codes():
    """A head dim or cache length outside the kernel's envelope: a non-zero code before
    anything is launched (every buffer is large enough for the shape named anyway)."""
    H = 2
    L = _lib.lib()
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    for Dh, S_max in ((32, 128), (128, 128), (64, 256), (64, 0)):
        qkv = torch.zeros(B, 3 * H * Dh, dtype=torch.bfloat16, device=DEV)
        kc = torch.full((B, H, max(S_max, 1), Dh), 3.0, dtype=torch.bfloat16, device=DEV)
        vc = kc.clone()
        o = torch.full((B, H * Dh), 7.0, dtype=torch.bfloat16, device=DEV)
        rc = L.jdt_attn_decode(p(qkv), p(kc), p(vc), p(o), p(T.posw(0, DEV)), B, H, Dh, S_max, 0.125,
                               _lib.stream_ptr())
        assert rc != 0
        with pytest.raises(RuntimeError):
            _lib.check(rc, "jdt_attn_decode")
        torch.cuda.synchronize()
        assert bool((o == 7.0).all()) and bool((kc == 3.0).all()) and bool((vc == 3.0).all())
    tok = torch.full((B, 16), 5, dtype=torch.int32, device=DEV)
    pw = T.posw(0, DEV)
    logits = torch.zeros(B, 64, dtype=torch.bfloat16, device=DEV)
    ticket = torch.zeros(1, dtype=torch.int32, device=DEV)
    rc = L.jdt_sample(p(logits), 64, B, 0, 0.0, 0, 0, p(tok), 16, p(pw), p(ticket), _lib.stream_ptr())
    assert rc != 0
    rc = L.jdt_embed_decode(p(tok), p(logits), p(logits), p(logits), p(pw), B, 16, 60, 3, _lib.stream_ptr())
    assert rc != 0
    torch.cuda.synchronize()
    assert bool((tok == 5).all()) and int(pw.item()) == 0


def test_embed_decode():
    T.body_embed_decode(DEV)


def test_sample_greedy():
    T.body_sample_greedy(DEV)


def test_sample_certain():
    T.body_sample_certain(DEV)


def test_sample_distribution():
    T.body_sample_distribution(DEV)


def test_sample_deterministic():
    T.body_sample_deterministic(DEV)


def test_sample_matches_cpu_draws():
    """Same Philox uniform on both sides: two equal live logits split at u = 0.5 identically."""
    x = torch.full((256, 512), -60.0)
    x[:, [3, 300]] = 0.0
    x = x.to(torch.bfloat16)
    for pos in (0, 77):
        a = T._sample(x, pos, DEV, temperature=1.0, seed=21, stream_id=2)
        assert torch.equal(a, T._sample(x, pos, T.CPU, temperature=1.0, seed=21, stream_id=2))


def test_teacher_forced():
    T.body_teacher_forced(DEV)


def test_teacher_forced_default_config():
    T.body_teacher_forced(DEV, TransformerConfig(), 2, [(60, [60, 61, 62, 63, 64, 65, 66])])


@pytest.mark.parametrize("capture", [False, True])
def test_greedy_consistent(capture):
    T.body_greedy_consistent(DEV, capture)


@pytest.mark.parametrize("temperature", [0.0, 0.8])
def test_captured_equals_eager(temperature):
    model, P = T.make_model(T.CFG, DEV, 3)
    gen = Generator(model, P, B, DEV)
    prompt = torch.randint(0, T.CFG.vocab_size, (B, 60), generator=torch.Generator().manual_seed(4))
    prompt = prompt.to(torch.int32).to(DEV)
    eager = gen.generate(prompt, 8, temperature=temperature, seed=11, capture=False)
    eager_logits = gen.logits.clone()
    for _ in range(2):   # the call that captures, then one that only replays
        graph = gen.generate(prompt, 8, temperature=temperature, seed=11, capture=True)
        assert torch.equal(graph, eager)
        assert torch.equal(gen.logits, eager_logits)
    assert gen._graphs[(temperature, 11)][0] is not None   # the step really was captured
