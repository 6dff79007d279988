"""Split-KV append attention, the parts that need no GPU: the workspace formula, the ``ws``
argument on the composed torch path (ignored), ``Generator(split_append=True)`` on CPU tensors
(the same tokens, position and caches, and a workspace of the documented size) and the
``generate.py --split-append`` switch.  tests/test_generate_append_split_gpu.py checks the kernels."""
import pytest
import torch

from jax_distributed_tuts_amd.generation import Generator, KVCache
from jax_distributed_tuts_amd.ops import kernels as kern

from . import test_generate as T
from . import test_generate_append as TA
from . import test_generate_long as TL

B, CPU = T.B, T.CPU
SPAN, SLOT = kern.AP_SPAN_ROWS, kern.AP_SLOT_FLOATS


def test_ws_floats_formula():
    """One (max, sum, o[64]) partial per (batch x head, 64-row query tile, span, row of the tile)."""
    assert SLOT == 66
    f = kern.attention_append_ws_floats
    assert f(1, 8, 64, 32768) == 8 * 1 * (32768 // SPAN) * 64 * SLOT
    assert f(3, 2, 65, 2 * SPAN + 69) == 3 * 2 * 2 * 3 * 64 * SLOT
    assert f(16, 8, 1024, SPAN) == 16 * 8 * 16 * 1 * 64 * SLOT
    assert f(2, 2, 1, 1) == 2 * 2 * 1 * 1 * 64 * SLOT
    assert f(0, 8, 64, 4096) == 0
    # the documented size: 16.5 KiB per (batch x head, query tile, span), 8.3 MiB at B = 1, H = 8, chunk 64, 32768 rows
    assert 64 * SLOT * 4 == 16.5 * 1024
    assert f(1, 8, 64, 32768) * 4 == 8.25 * 2 ** 20


@pytest.mark.parametrize("rows", [False, True])
def test_ws_is_ignored_on_cpu(rows):
    """The composed torch path ignores ws: the same o and caches, and ws is left alone."""
    H, C, p = 2, 65, 63
    qkv, kc, vc = TA.append_inputs(H, C, seed=11)
    pos = TA.posr([p, 0, 200], CPU) if rows else T.posw(p, CPU)
    count = TA.posr([65, 3, 0], CPU) if rows else None
    ref, k1, v1 = TA.run_append(CPU, qkv, kc, vc, pos, H, C, count=count)
    for ws in (torch.full((kern.attention_append_ws_floats(B, H, C, TA.S_MAX),), 5.0), torch.full((3,), 5.0)):
        k2, v2 = kc.clone(), vc.clone()
        got = kern.attention_append(qkv, k2, v2, pos, H, C, count=count, ws=ws)
        assert torch.equal(got, ref) and torch.equal(k2, k1) and torch.equal(v2, v1)
        assert bool((ws == 5.0).all())


def test_generator_split_append_cpu():
    """prefill(chunk=) and extend with split_append give the tokens, position and caches of the
    plain generator, and kv.append_ws has at least the documented size; it grows on demand and a
    larger buffer is kept."""
    cfg = TL.CFG_LONG
    H = cfg.n_heads
    model, P, tok, _, _ = TA.lm_shared(CPU)
    gen, ref = Generator(model, P, B, CPU, split_append=True), Generator(model, P, B, CPU)
    assert gen.split_append and not ref.split_append and gen.kv.append_ws is None
    for g in (gen, ref):
        g.prefill(tok[:, :150], chunk=64)
    need64 = kern.attention_append_ws_floats(B, H, 64, cfg.seq_len)
    ws = gen.kv.append_ws
    assert ws.dtype == torch.float32 and ws.is_contiguous() and ws.numel() >= need64
    for g in (gen, ref):
        g.extend(tok[:, 150:180], chunk=16)
    assert gen.kv.append_ws is ws   # the larger buffer is kept
    la, lb = (g.extend(tok[:, 180:310], chunk=130, logits=True) for g in (gen, ref))
    assert gen.kv.append_ws.numel() >= kern.attention_append_ws_floats(B, H, 130, cfg.seq_len) > need64
    assert torch.equal(la, lb)
    assert int(gen.kv.pos.item()) == int(ref.kv.pos.item()) == 309
    assert torch.equal(gen.kv.tokens, ref.kv.tokens)
    for l in range(cfg.n_layers):
        assert torch.equal(gen.kv.k[l], ref.kv.k[l]) and torch.equal(gen.kv.v[l], ref.kv.v[l])
    assert ref.kv.append_ws is None


def test_generator_split_append_per_row_cpu():
    model, P, tok, _, _ = TA.lm_shared(CPU)
    gen, ref = Generator(model, P, B, CPU, split_append=True), Generator(model, P, B, CPU)
    for g in (gen, ref):
        g.prefill(tok[:, :200], torch.tensor([5, 130, 200]), chunk=64)
        g.extend(tok[:, 200:264], torch.tensor([0, 3, 64]), chunk=64)
    assert gen.kv.pos_rows.tolist() == ref.kv.pos_rows.tolist()
    for l in range(TL.CFG_LONG.n_layers):
        assert torch.equal(gen.kv.k[l], ref.kv.k[l]) and torch.equal(gen.kv.v[l], ref.kv.v[l])
    assert gen.kv.append_ws.numel() >= kern.attention_append_ws_floats(B, TL.CFG_LONG.n_heads, 64, 320)


def test_default_generator_has_no_append_ws():
    model, P, tok, _, _ = TA.lm_shared(CPU)
    gen = Generator(model, P, B, CPU)
    assert gen.kv.append_ws is None and KVCache(TL.CFG_LONG, B, CPU).append_ws is None
    gen.prefill(tok[:, :100], chunk=64)
    gen.extend(tok[:, 100:120])
    assert gen.kv.append_ws is None


def test_generate_cli_split_append(capsys):
    """--split-append is valid only with --prefill-chunk: a clear error (exit 2) without it."""
    import generate

    with pytest.raises(SystemExit) as e:
        generate.parse_args(["--split-append"])
    assert e.value.code == 2 and "--prefill-chunk" in capsys.readouterr().err
    assert generate.parse_args([]).split_append is False
    generate.main(generate.parse_args(["--seq-len", "160", "--prompt-len", "140", "--prefill-chunk", "64",
                                       "--split-append", "--max-new-tokens", "8", "--batch", "2"]))
    rows = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("[generate] seq ")]
    assert len(rows) == 2
    for ln in rows:
        ids = ln.split(": ", 1)[1].split()
        assert len(ids) == 148 and all(0 <= int(t) < 2048 for t in ids)
