"""KV caches longer than 128 rows (split-KV decode attention) on CPU tensors, and the
device-agnostic bodies that tests/test_generate_long_gpu.py runs again on the HIP kernels.

Yardsticks and bounds are those of tests/test_generate.py: the float64 LM, E_dec <= 2 E_full
for teacher-forced decoding and a worst greedy gap of 4 E_full.  The model's cache has 320 rows:
two full 128-key chunks and a ragged third, so the decoded positions cross both chunk seams."""
import torch

from jax_distributed_tuts_amd.generation import Generator, KVCache
from jax_distributed_tuts_amd.models.transformer import TransformerConfig
from jax_distributed_tuts_amd.ops import kernels as kern

from . import test_generate as T

CFG_LONG = TransformerConfig(vocab_size=512, d_model=128, n_heads=2, d_ff=512, seq_len=320, n_layers=2)
B, CPU = T.B, T.CPU
LONG_CASES = [(126, [126, 127, 128, 129, 130]), (254, [254, 255, 256, 257, 258]), (318, [318, 319])]


# ----------------------------------------------------------------------------- shared bodies
def body_teacher_forced_long(dev):
    T.body_teacher_forced(dev, CFG_LONG, B, LONG_CASES)


def body_greedy_consistent_long(dev, capture=True):
    """tests/test_generate.py body_greedy_consistent on the 320-row cache: a 250-token prompt
    (prefilled over 256 rows) and 12 new tokens, which cross the seam at 256."""
    cfg = CFG_LONG
    model, P = T.make_model(cfg, dev, 2)
    Pn, new = 250, 12
    prompt = torch.randint(0, cfg.vocab_size, (B, Pn), generator=torch.Generator().manual_seed(9)).to(torch.int32)
    gen = Generator(model, P, B, dev)
    seq = gen.generate(prompt.to(dev), new, temperature=0.0, capture=capture).cpu()
    assert gen.prefill_rows == 256
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
    T.log_errors(name="greedy_consistent_long", device=str(dev), E_full=e_full, worst_gap=worst)
    assert worst <= 4 * e_full, (worst, e_full)


def body_prefill_rows(dev):
    """The prefill's forward runs over the prompt padded to a multiple of 128 (at most seq_len),
    and leaves the cache rows < P and the position of the full-length convention."""
    model, P = T.make_model(CFG_LONG, dev, 1)
    gen = Generator(model, P, B, dev)
    assert gen.prefill_rows == 0
    prompt = torch.randint(0, CFG_LONG.vocab_size, (B, 310), generator=torch.Generator().manual_seed(3))
    prompt = prompt.to(torch.int32).to(dev)
    for Pn, rows in ((250, 256), (16, 128), (129, 256), (310, 320)):
        gen.prefill(prompt[:, :Pn])
        assert gen.prefill_rows == rows, (Pn, gen.prefill_rows)
        assert int(gen.kv.pos.item()) == Pn - 1
        assert torch.equal(gen.kv.tokens[:, :Pn], prompt[:, :Pn]) and bool((gen.kv.tokens[:, Pn:] == 0).all())
    gen.prefill(prompt[:, :200], torch.tensor([5, 130, 200]))
    assert gen.prefill_rows == 256 and gen.kv.pos_rows.tolist() == [4, 129, 199]


# ----------------------------------------------------------------------------- CPU tests
def test_teacher_forced_long_cpu():
    body_teacher_forced_long(CPU)


def test_greedy_consistent_long_cpu():
    body_greedy_consistent_long(CPU)


def test_prefill_rows_cpu():
    body_prefill_rows(CPU)


def test_prefill_rows_short_cache_unchanged():
    """seq_len <= 128: the forward still runs over the whole cache."""
    model, P = T.make_model(T.CFG, CPU, 1)
    gen = Generator(model, P, B, CPU)
    gen.prefill(torch.ones(B, 16, dtype=torch.int32))
    assert gen.prefill_rows == T.CFG.seq_len == 128


def test_split_ws_shape():
    H = CFG_LONG.n_heads
    kv = KVCache(CFG_LONG, B, CPU)
    assert kv.split_ws.shape == (B * H, 3, 66) and kv.split_ws.dtype == torch.float32
    assert kv.split_ws.numel() == kern.attention_decode_ws_floats(B, H, CFG_LONG.seq_len)
    assert kern.AD_CHUNK_ROWS == 128 and kern.AD_LONG_MAX_ROWS == 32768
    for seq_len, chunks in ((129, 2), (256, 2), (257, 3), (1024, 8)):
        cfg = TransformerConfig(vocab_size=64, d_model=128, n_heads=2, d_ff=128, seq_len=seq_len, n_layers=1)
        assert KVCache(cfg, 2, CPU).split_ws.shape == (4, chunks, 66)
    for seq_len in (1, 127, 128):
        cfg = TransformerConfig(vocab_size=64, d_model=128, n_heads=2, d_ff=128, seq_len=seq_len, n_layers=1)
        assert KVCache(cfg, 2, CPU).split_ws is None
    assert KVCache(T.CFG, B, CPU).split_ws is None


def test_attention_decode_ws_ignored_on_cpu():
    """CPU tensors take the composed path whatever ``ws`` is, and leave it alone."""
    H, S_max, pos = 2, 320, 200
    qkv, kc, vc = T.decode_inputs(B, H, S_max, seed=1)
    want = kern.attention_decode(qkv, kc.clone(), vc.clone(), T.posw(pos, CPU), H)
    ref, _ = T.attn_decode_fp64(qkv, kc, vc, pos, H)
    T.close(want, ref)
    for ws in (torch.full((7,), float("nan")), torch.zeros(0), torch.full((B * H, 3, 66), 5.0)):
        before = ws.clone()
        got = kern.attention_decode(qkv, kc.clone(), vc.clone(), T.posw(pos, CPU), H, ws=ws)
        assert torch.equal(got, want)
        assert torch.equal(ws.isnan(), before.isnan()) and torch.equal(ws.nan_to_num(), before.nan_to_num())


def test_generate_cli_seq_len(capsys):
    """generate.py --seq-len 160: 140 prompt tokens + 8 new ones per row in a 160-row cache."""
    import generate

    generate.main(generate.parse_args(["--seq-len", "160", "--prompt-len", "140", "--max-new-tokens", "8",
                                       "--batch", "2"]))
    rows = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("[generate] seq ")]
    assert len(rows) == 2
    for ln in rows:
        ids = ln.split(": ", 1)[1].split()
        assert len(ids) == 148 and all(0 <= int(t) < 2048 for t in ids)
    assert generate.parse_args([]).seq_len == 128
