"""Split-KV decode attention on the MI355X (csrc/attn_decode.hip, ``jdt_attn_decode_long`` and
``_long_rows``: caches of 129..32768 rows) against fp64, bit for bit against the one-launch
kernel where both apply, and the bodies of tests/test_generate_long.py on the GPU.

Shapes: caches of 129 rows (one full 128-key chunk and a chunk of one row) and 320 rows (two
full chunks and a ragged third), positions on both sides of every chunk seam."""
import ctypes

import pytest
import torch

from jax_distributed_tuts_amd.generation import Generator, KVCache
from jax_distributed_tuts_amd.ops import _lib
from jax_distributed_tuts_amd.ops import kernels as kern

from . import test_generate as T
from . import test_generate_long as TL

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0) if torch.cuda.is_available() else None
B, CFG_LONG = T.B, TL.CFG_LONG
POSITIONS = [0, 127, 128, 129, 255, 256, 257, 319]


def posr(ps, dev):
    return torch.tensor(list(ps), dtype=torch.int32, device=dev)


def call_long(qkv, kc, vc, o, pos, ws, H, *, ws_floats=None, Bq=None, Dh=64, S_max=None, qkv_ptr=None, null=()):
    """The raw launcher (shared or per-row by ``pos.numel()``); returns its code.  ``null``:
    names of pointer arguments passed as NULL."""
    Bq = qkv.shape[0] if Bq is None else Bq
    name = "jdt_attn_decode_long" if pos.numel() == 1 else "jdt_attn_decode_long_rows"
    ptr = {k: (None if k in null else ctypes.c_void_p(t.data_ptr()))
           for k, t in dict(qkv=qkv, kc=kc, vc=vc, o=o, pos=pos, ws=ws).items()}
    if qkv_ptr is not None:
        ptr["qkv"] = ctypes.c_void_p(qkv_ptr)
    return getattr(_lib.lib(), name)(ptr["qkv"], ptr["kc"], ptr["vc"], ptr["o"], ptr["pos"], ptr["ws"],
                                     ws.numel() if ws_floats is None else ws_floats, Bq, H, Dh,
                                     kc.shape[2] if S_max is None else S_max, 0.125, _lib.stream_ptr())


def decode(qkv, kc, vc, pos, H, ws=None, o=None):
    """attention_decode on device copies: (o, k_cache, v_cache) after the call."""
    k2, v2 = kc.to(DEV).clone(), vc.to(DEV).clone()
    got = kern.attention_decode(qkv.to(DEV), k2, v2, pos, H, out=o, ws=ws)
    return got, k2, v2


# ----------------------------------------------------------------------------- 1. against fp64
@pytest.mark.parametrize("H", [2, 8])
@pytest.mark.parametrize("S_max,pos", [(S, p) for S in (129, 320) for p in POSITIONS if p < S])
def test_attention_decode_long_vs_fp64(S_max, pos, H):
    """e_dec <= 2 e_ref, the bound and the construction of test_attention_decode_vs_fp64: e_ref is
    the fp64 error of row ``pos`` of attention_fwd on the equivalent S_max-long causal sequence."""
    d = H * 64
    qkv, kc, vc = T.decode_inputs(B, H, S_max, seed=1000 * H + S_max + pos)
    want, _ = T.attn_decode_fp64(qkv, kc, vc, pos, H)
    got, _, _ = decode(qkv, kc, vc, T.posw(pos, DEV), H)
    full = torch.randn(B, S_max, 3, H, 64, generator=torch.Generator().manual_seed(1)).to(torch.bfloat16)
    full[:, :pos, 1] = kc[:, :, :pos].permute(0, 2, 1, 3)
    full[:, :pos, 2] = vc[:, :, :pos].permute(0, 2, 1, 3)
    full[:, pos] = qkv.view(B, 3, H, 64)
    o_full, _ = kern.attention_fwd(full.view(B * S_max, 3 * d).to(DEV), B, S_max, H)
    e_ref = float((o_full.view(B, S_max, d)[:, pos].cpu().double() - want).abs().max())
    e_dec = float((got.cpu().double() - want).abs().max())
    T.log_errors(name="attention_decode_long", S_max=S_max, pos=pos, H=H, e_dec=e_dec, e_ref=e_ref)
    assert e_dec <= 2 * e_ref, (e_dec, e_ref)
    cpu = kern.attention_decode(qkv, kc.clone(), vc.clone(), T.posw(pos, T.CPU), H)
    T.close(got, cpu)


# ----------------------------------------------------------------------------- 2. bitwise
@pytest.mark.parametrize("H", [2, 8])
def test_one_chunk_has_the_bits_of_the_one_launch_kernel(H):
    """S_max = 128 is one chunk: the split launch + combine give jdt_attn_decode's o and caches."""
    for pos in (0, 63, 127):
        qkv, kc, vc = T.decode_inputs(B, H, 128, seed=50 * H + pos)
        want, wk, wv = decode(qkv, kc, vc, T.posw(pos, DEV), H)   # S_max <= 128: jdt_attn_decode
        k2, v2 = kc.to(DEV).clone(), vc.to(DEV).clone()
        o = torch.full((B, H * 64), 7.0, dtype=torch.bfloat16, device=DEV)
        ws = torch.full((kern.attention_decode_ws_floats(B, H, 128),), float("nan"), device=DEV)
        assert call_long(qkv.to(DEV), k2, v2, o, T.posw(pos, DEV), ws, H) == 0
        assert torch.equal(o, want) and torch.equal(k2, wk) and torch.equal(v2, wv)


@pytest.mark.parametrize("H", [2, 8])
def test_per_row_has_the_bits_of_the_shared_position(H):
    pos = [0, 128, 319]
    qkv, kc, vc = T.decode_inputs(B, H, 320, seed=60 + H)
    got, k2, v2 = decode(qkv, kc, vc, posr(pos, DEV), H)
    for b, p in enumerate(pos):
        ref, rk, rv = decode(qkv, kc, vc, T.posw(p, DEV), H)
        assert torch.equal(got[b], ref[b]) and torch.equal(k2[b], rk[b]) and torch.equal(v2[b], rv[b])


def test_two_calls_same_bits():
    H = 8
    qkv, kc, vc = T.decode_inputs(B, H, 320, seed=70)
    for pos in (T.posw(300, DEV), posr([17, 128, 300], DEV)):
        a, ak, av = decode(qkv, kc, vc, pos, H)
        b, bk, bv = decode(qkv, kc, vc, pos, H)
        assert torch.equal(a, b) and torch.equal(ak, bk) and torch.equal(av, bv)


# ----------------------------------------------------------------------------- 3. stale workspace
@pytest.mark.parametrize("pos", [5, 128, 200])
def test_stale_workspace_is_harmless(pos):
    """Slots of chunks past pos / 128 are neither written nor read: a NaN-filled workspace gives
    the bits of a zeroed one and keeps its NaNs there."""
    H, S_max = 2, 320
    qkv, kc, vc = T.decode_inputs(B, H, S_max, seed=80 + pos)
    zero = torch.zeros(B * H, 3, 66, device=DEV)
    nan = torch.full((B * H, 3, 66), float("nan"), device=DEV)
    want, wk, wv = decode(qkv, kc, vc, T.posw(pos, DEV), H, ws=zero)
    got, gk, gv = decode(qkv, kc, vc, T.posw(pos, DEV), H, ws=nan)
    assert torch.equal(got, want) and torch.equal(gk, wk) and torch.equal(gv, wv)
    last = pos // 128
    assert not bool(nan[:, :last + 1].isnan().any()) and bool(nan[:, last + 1:].isnan().all())
    assert torch.equal(nan[:, :last + 1], zero[:, :last + 1]) and bool((zero[:, last + 1:] == 0).all())
    ref, _ = T.attn_decode_fp64(qkv, kc, vc, pos, H)
    T.close(got, ref)


# ----------------------------------------------------------------------------- 4. needle
def test_needle_long():
    """body_needle's construction in a 320-row cache: one key j carries softmax weight > 1 - 1e-4,
    so o must be v_j -- j at both ends of every chunk and at the token itself.  The needle's
    length is 20 where body_needle has 16: 319 other keys share the rest here, not 127."""
    H, S_max = 2, 320
    for pos in (256, 319):
        for j in sorted({0, 127, 128, 255, 256, pos}):
            qkv, kc, vc = T.decode_inputs(B, H, S_max, seed=2000 + pos + j)
            q = qkv.float().view(B, 3, H, 64)[:, 0]
            needle = (20.0 * q / q.norm(dim=-1, keepdim=True)).to(torch.bfloat16)
            kc = (kc.float() * 0.05).to(torch.bfloat16)
            new = qkv.clone().view(B, 3, H, 64)
            new[:, 1] = (new[:, 1].float() * 0.05).to(torch.bfloat16)
            if j == pos:
                new[:, 1] = needle
            else:
                kc[:, :, j] = needle
            qkv = new.view(B, -1).contiguous()
            want, p = T.attn_decode_fp64(qkv, kc, vc, pos, H)
            assert float(p[:, :, j].min()) > 1 - 1e-4
            vj = (qkv.view(B, 3, H, 64)[:, 2] if j == pos else vc[:, :, j]).reshape(B, -1)
            got, _, _ = decode(qkv, kc, vc, T.posw(pos, DEV), H)
            T.close(got, vj)
            T.close(got, want)


# ----------------------------------------------------------------------------- 5. append and bounds
@pytest.mark.parametrize("S_max", [129, 320])
@pytest.mark.parametrize("H", [2, 8])
def test_append_touches_one_row_of_one_layer(S_max, H):
    """After a call, cache row pos holds the token's k / v bit for bit; every other row, and the
    neighbouring layers' buffers on both sides, are untouched."""
    for pos in (p for p in (0, 127, 128, 129, 255, 256, 319) if p < S_max):
        qkv, kc, vc = T.decode_inputs(B, H, S_max, seed=90 + pos)
        g = torch.Generator().manual_seed(pos)
        layers_k = torch.randn(3, B, H, S_max, 64, generator=g).to(torch.bfloat16)
        layers_v = torch.randn(3, B, H, S_max, 64, generator=g).to(torch.bfloat16)
        layers_k[1], layers_v[1] = kc, vc
        dk, dv = layers_k.to(DEV), layers_v.to(DEV)
        kern.attention_decode(qkv.to(DEV), dk[1], dv[1], T.posw(pos, DEV), H)
        layers_k[1, :, :, pos] = qkv.view(B, 3, H, 64)[:, 1]
        layers_v[1, :, :, pos] = qkv.view(B, 3, H, 64)[:, 2]
        assert torch.equal(dk.cpu(), layers_k) and torch.equal(dv.cpu(), layers_v)


@pytest.mark.parametrize("S_max", [129, 320])
def test_out_of_range_long(S_max):
    H = 2
    qkv, kc, vc = T.decode_inputs(B, H, S_max, seed=3)
    for pos in (-1, S_max):   # the shared word: nothing changes for any row
        o = torch.full((B, H * 64), 7.0, dtype=torch.bfloat16, device=DEV)
        ws = torch.full((B * H, (S_max + 127) // 128, 66), 9.0, device=DEV)
        _, k2, v2 = decode(qkv, kc, vc, T.posw(pos, DEV), H, ws=ws, o=o)
        assert torch.equal(k2.cpu(), kc) and torch.equal(v2.cpu(), vc)
        assert bool((o == 7.0).all()) and bool((ws == 9.0).all())
    for bad in (-1, S_max):   # per row: nothing changes for that row only
        for b_bad in range(B):
            pos = [5, 128, S_max - 1]
            pos[b_bad] = bad
            o = torch.full((B, H * 64), 7.0, dtype=torch.bfloat16, device=DEV)
            _, k2, v2 = decode(qkv, kc, vc, posr(pos, DEV), H, o=o)
            for b, p in enumerate(pos):
                if b == b_bad:
                    assert torch.equal(k2[b].cpu(), kc[b]) and torch.equal(v2[b].cpu(), vc[b])
                    assert bool((o[b] == 7.0).all())
                else:
                    ref, rk, rv = decode(qkv, kc, vc, T.posw(p, DEV), H)
                    assert torch.equal(o[b], ref[b]) and torch.equal(k2[b], rk[b]) and torch.equal(v2[b], rv[b])


# ----------------------------------------------------------------------------- 6. return codes
@pytest.mark.parametrize("rows", [False, True])
def test_long_return_codes(rows):
    """Every rejection comes before anything is launched: o, the caches and the workspace keep
    their sentinels (every buffer is large enough for the shape named anyway)."""
    H = 2

    def case(Dh=64, S_max=320, Bq=B, **kw):
        qkv = torch.zeros(B, 3 * H * Dh + 8, dtype=torch.bfloat16, device=DEV)
        kc = torch.full((B, H, max(S_max, 1), Dh), 3.0, dtype=torch.bfloat16, device=DEV)
        vc = kc.clone()
        o = torch.full((B, H * Dh), 7.0, dtype=torch.bfloat16, device=DEV)
        ws = torch.full((kern.attention_decode_ws_floats(B, H, max(S_max, 1)),), 9.0, device=DEV)
        pos = posr([0] * B, DEV) if rows else T.posw(0, DEV)
        if kw.pop("misaligned", False):
            kw["qkv_ptr"] = qkv.data_ptr() + 8
        if kw.pop("short", False):   # one float less than this call's B * H * chunks * 66
            kw["ws_floats"] = kern.attention_decode_ws_floats(Bq, H, S_max) - 1
        rc = call_long(qkv, kc, vc, o, pos, ws, H, Bq=Bq, Dh=Dh, S_max=S_max, **kw)
        torch.cuda.synchronize()
        assert bool((o == 7.0).all()) and bool((kc == 3.0).all()) and bool((vc == 3.0).all())
        assert bool((ws == 9.0).all())
        return rc

    name = "jdt_attn_decode_long_rows" if rows else "jdt_attn_decode_long"
    assert case(Dh=32) == -3 and case(Dh=128) == -3
    assert case(S_max=0) == -4 and case(S_max=32769) == -4
    for arg in ("qkv", "kc", "vc", "o", "pos", "ws"):
        assert case(null=(arg,)) == -2, arg
    assert case(misaligned=True) == -6
    short = case(short=True)
    assert short not in (0, -2, -3, -4, -5, -6)   # a code of its own
    assert case(S_max=129, short=True) == short and case(S_max=32768, Bq=1, short=True) == short
    with pytest.raises(RuntimeError):
        _lib.check(short, name)
    assert case(Bq=0) == 0   # a no-op


def test_longest_cache_accepted():
    """S_max = 32768, the top of the envelope (256 chunks), at its last position and at the first."""
    H, S_max = 1, 32768
    qkv, kc, vc = T.decode_inputs(1, H, S_max, seed=4)
    for pos in (S_max - 1, 0):
        got, k2, v2 = decode(qkv, kc, vc, T.posw(pos, DEV), H)
        want, _ = T.attn_decode_fp64(qkv, kc, vc, pos, H)
        T.close(got, want)
        kc2, vc2 = kc.clone(), vc.clone()
        kc2[:, :, pos], vc2[:, :, pos] = qkv.view(1, 3, H, 64)[:, 1], qkv.view(1, 3, H, 64)[:, 2]
        assert torch.equal(k2.cpu(), kc2) and torch.equal(v2.cpu(), vc2)


# ----------------------------------------------------------------------------- 7. model level
def test_teacher_forced_long():
    TL.body_teacher_forced_long(DEV)


@pytest.mark.parametrize("capture", [False, True])
def test_greedy_consistent_long(capture):
    TL.body_greedy_consistent_long(DEV, capture)


def test_prefill_rows():
    TL.body_prefill_rows(DEV)


def test_decode_step_uses_the_cache_workspace():
    """The model's decode step hands KVCache.split_ws to the kernel: its slots up to pos / 128 are
    rewritten and the later ones keep what they held."""
    model, P = T.make_model(CFG_LONG, DEV, 1)
    gen = Generator(model, P, B, DEV)
    assert isinstance(gen.kv, KVCache) and gen.kv.split_ws.shape == (B * CFG_LONG.n_heads, 3, 66)
    gen.prefill(torch.ones(B, 130, dtype=torch.int32, device=DEV))
    gen.kv.split_ws.fill_(float("nan"))
    logits = gen.step(sample=False)
    assert bool(torch.isfinite(logits.float()).all())
    assert not bool(gen.kv.split_ws[:, :2].isnan().any()) and bool(gen.kv.split_ws[:, 2].isnan().all())


# ----------------------------------------------------------------------------- 8. capture
@pytest.mark.parametrize("temperature", [0.0, 0.8])
def test_captured_equals_eager_long(temperature):
    """The decode step of a 320-row cache is captured (no host read of pos) and its replays give
    the eager tokens and logits bit for bit, uniform and ragged with an EOS."""
    model, P = T.make_model(CFG_LONG, DEV, 3)
    gen = Generator(model, P, B, DEV)
    prompt = torch.randint(0, CFG_LONG.vocab_size, (B, 260), generator=torch.Generator().manual_seed(4))
    prompt = prompt.to(torch.int32).to(DEV)
    for pr, kw in ((prompt[:, :250], {}), (prompt, dict(prompt_lens=[5, 130, 260], eos_id=7))):
        eager = gen.generate(pr, 12, temperature=temperature, seed=11, capture=False, **kw)
        eager_logits, eager_lengths = gen.logits.clone(), gen.lengths.clone()
        for _ in range(2):   # the call that captures, then one that only replays
            graph = gen.generate(pr, 12, temperature=temperature, seed=11, capture=True, **kw)
            assert torch.equal(graph, eager)
            assert torch.equal(gen.logits, eager_logits) and torch.equal(gen.lengths, eager_lengths)
        assert gen._graphs[gen._graph_key()][0] is not None   # the step really was captured
