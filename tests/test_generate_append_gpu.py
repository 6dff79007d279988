"""Append attention on the MI355X (csrc/attn_append.hip, ``jdt_attn_append`` / ``_rows``, and
``embed_append``) against fp64 and bit for bit across every way of cutting a sequence into calls,
and the bodies of tests/test_generate_append.py on the GPU.

Shapes: B = 3, H in {2, 8}, a 320-row cache; chunks of 1..192 rows that start on both sides of the
64-key tile seams, so a workgroup's key tiles come from the cache, from the chunk and from both."""
import ctypes

import pytest
import torch

from jax_distributed_tuts_amd.ops import _lib
from jax_distributed_tuts_amd.ops import kernels as kern

from . import test_generate as T
from . import test_generate_append as TA

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0) if torch.cuda.is_available() else None
B, S_MAX = TA.B, TA.S_MAX
posr = TA.posr


def run(qkv, kc, vc, pos, H, C, count=None, o=None):
    return TA.run_append(DEV, qkv, kc, vc, pos, H, C, count=count, o=o)


def rows_of(qkv, Bq, C, lo, hi):
    """Tokens lo..hi-1 of every sequence of a [Bq*C, w] chunk as a chunk of their own."""
    return qkv.view(Bq, C, -1)[:, lo:hi].reshape(Bq * (hi - lo), -1).contiguous()


# ----------------------------------------------------------------------------- 1. against fp64
_FULL: dict = {}


def full_filler(H):
    """The rows past p + C of the equivalent 320-row sequence (one draw per H, never modified)."""
    if H not in _FULL:
        _FULL[H] = torch.randn(B, S_MAX, 3, H, 64, generator=torch.Generator().manual_seed(1)).to(torch.bfloat16)
    return _FULL[H]


@pytest.mark.parametrize("H", [2, 8])
@pytest.mark.parametrize("p,C", [(p, C) for p in (0, 1, 63, 64, 65, 127, 200) for C in (1, 17, 64, 65, 128)
                                 if p + C <= S_MAX])
def test_attention_append_vs_fp64(p, C, H):
    """e_app <= 2 e_ref, the construction of test_attention_decode_long_vs_fp64: e_ref is the fp64
    error of rows p..p+C-1 of attention_fwd on the equivalent 320-row causal sequence."""
    d = H * 64
    qkv, kc, vc = TA.append_inputs(H, C, seed=1000 * H + 10 * p + C)
    want, _ = TA.attn_append_fp64(qkv, kc, vc, p, C, H)
    got, _, _ = run(qkv, kc, vc, T.posw(p, DEV), H, C)
    full = full_filler(H).clone()
    full[:, :p, 1] = kc[:, :, :p].permute(0, 2, 1, 3)
    full[:, :p, 2] = vc[:, :, :p].permute(0, 2, 1, 3)
    full[:, p:p + C] = qkv.view(B, C, 3, H, 64)
    o_full, _ = kern.attention_fwd(full.view(B * S_MAX, 3 * d).to(DEV), B, S_MAX, H)
    e_ref = float((o_full.view(B, S_MAX, d)[:, p:p + C].cpu().double() - want).abs().max())
    e_app = float((got.view(B, C, d).cpu().double() - want).abs().max())
    T.log_errors(name="attention_append", p=p, C=C, H=H, e_app=e_app, e_ref=e_ref)
    assert e_app <= 2 * e_ref, (e_app, e_ref)
    cpu = kern.attention_append(qkv, kc.clone(), vc.clone(), T.posw(p, T.CPU), H, C)
    T.close(got, cpu)


# ----------------------------------------------------------------------------- 2. chunking leaves the bits alone
@pytest.mark.parametrize("H", [2, 8])
def test_chunking_leaves_the_bits_alone(H):
    """192 tokens from p = 37 in one call, in three calls of 64 and in calls of 1, 100 and 91: the
    same o rows and the same caches, bit for bit; and two identical calls give the same bits."""
    p0, N = 37, 192
    qkv, kc, vc = TA.append_inputs(H, N, seed=20 + H)
    one, k1, v1 = run(qkv, kc, vc, T.posw(p0, DEV), H, N)
    again, k1b, v1b = run(qkv, kc, vc, T.posw(p0, DEV), H, N)
    assert torch.equal(one, again) and torch.equal(k1, k1b) and torch.equal(v1, v1b)
    want, _ = TA.attn_append_fp64(qkv, kc, vc, p0, N, H)
    T.close(one.view(B, N, -1), want)
    for cuts in ((64, 64, 64), (1, 100, 91)):
        k2, v2 = kc.to(DEV).clone(), vc.to(DEV).clone()
        outs, lo = [], 0
        for C in cuts:
            part = rows_of(qkv, B, N, lo, lo + C).to(DEV)
            outs.append(kern.attention_append(part, k2, v2, T.posw(p0 + lo, DEV), H, C).view(B, C, -1))
            lo += C
        assert torch.equal(torch.cat(outs, 1), one.view(B, N, -1)), cuts
        assert torch.equal(k2, k1) and torch.equal(v2, v1), cuts


# ----------------------------------------------------------------------------- 3. per row == shared
@pytest.mark.parametrize("H", [2, 8])
def test_per_row_has_the_bits_of_the_shared_position(H):
    pos, count, C = [0, 70, 130], [64, 10, 0], 64
    qkv, kc, vc = TA.append_inputs(H, C, seed=30 + H)
    o = torch.full((B * C, H * 64), 7.0, dtype=torch.bfloat16, device=DEV)
    got, k2, v2 = run(qkv, kc, vc, posr(pos, DEV), H, C, count=posr(count, DEV), o=o)
    got = got.view(B, C, -1)
    for b, (p, n) in enumerate(zip(pos, count)):
        assert bool((got[b, n:] == 7.0).all())
        if n == 0:
            assert torch.equal(k2[b].cpu(), kc[b]) and torch.equal(v2[b].cpu(), vc[b])
            continue
        ref, rk, rv = run(rows_of(qkv, B, C, 0, n), kc, vc, T.posw(p, DEV), H, n)
        assert torch.equal(got[b, :n], ref.view(B, n, -1)[b])
        assert torch.equal(k2[b], rk[b]) and torch.equal(v2[b], rv[b])


# ----------------------------------------------------------------------------- 4. cache writes
def test_cache_writes():
    TA.body_cache_writes(DEV)


# ----------------------------------------------------------------------------- 5. out of range
def test_out_of_range():
    TA.body_out_of_range(DEV)


def test_out_of_range_good_rows_have_their_solo_bits():
    """Per row, one bad row among good ones: the good rows have the bits of their solo calls."""
    H, C = 2, 64
    qkv, kc, vc = TA.append_inputs(H, C, seed=3)
    for bad_p, bad_n in ((-1, 5), (S_MAX - 4, 5)):
        for b_bad in range(B):
            pos, count = [5, 100, 250], [64, 7, 1]
            pos[b_bad], count[b_bad] = bad_p, bad_n
            got, k2, v2 = run(qkv, kc, vc, posr(pos, DEV), H, C, count=posr(count, DEV))
            for b in (b for b in range(B) if b != b_bad):
                n = count[b]
                ref, rk, rv = run(rows_of(qkv, B, C, 0, n), kc, vc, T.posw(pos[b], DEV), H, n)
                assert torch.equal(got.view(B, C, -1)[b, :n], ref.view(B, n, -1)[b])
                assert torch.equal(k2[b], rk[b]) and torch.equal(v2[b], rv[b])


# ----------------------------------------------------------------------------- 6. needle, 7. C = 1
def test_needle():
    TA.body_needle(DEV)


def test_append_close_to_fp64_body():
    TA.body_append_close_to_fp64(DEV)


def test_c1_agrees_with_decode():
    TA.body_c1_agrees_with_decode(DEV)


# ----------------------------------------------------------------------------- 8. return codes
def call_append(qkv, kc, vc, o, pos, count, H, C, *, Bq=B, Dh=64, S_max=None, qkv_ptr=None, kc_ptr=None, null=()):
    """The raw launcher (per-row when ``count`` is given); returns its code.  ``null``: names of
    pointer arguments passed as NULL."""
    ptr = {k: (None if k in null or t is None else ctypes.c_void_p(t.data_ptr()))
           for k, t in dict(qkv=qkv, kc=kc, vc=vc, o=o, pos=pos, count=count).items()}
    if qkv_ptr is not None:
        ptr["qkv"] = ctypes.c_void_p(qkv_ptr)
    if kc_ptr is not None:
        ptr["kc"] = ctypes.c_void_p(kc_ptr)
    tail = (Bq, C, H, Dh, kc.shape[2] if S_max is None else S_max, 0.125, _lib.stream_ptr())
    if count is None:
        return _lib.lib().jdt_attn_append(ptr["qkv"], ptr["kc"], ptr["vc"], ptr["o"], ptr["pos"], *tail)
    return _lib.lib().jdt_attn_append_rows(ptr["qkv"], ptr["kc"], ptr["vc"], ptr["o"], ptr["pos"], ptr["count"], *tail)


@pytest.mark.parametrize("rows", [False, True])
def test_append_return_codes(rows):
    """Every rejection comes before anything is launched: o and the caches keep their sentinels
    (every buffer is large enough for the shape named anyway)."""
    H = 2

    def case(Dh=64, S_max=320, C=64, Bq=B, **kw):
        Cb = min(max(C, 1), 1025)
        qkv = torch.zeros(B * Cb, 3 * H * Dh + 8, dtype=torch.bfloat16, device=DEV)
        kc = torch.full((B, H, max(min(max(S_max, 1), 400), Cb) + 1, Dh), 3.0, dtype=torch.bfloat16, device=DEV)
        vc = kc.clone()
        o = torch.full((B * Cb, H * Dh), 7.0, dtype=torch.bfloat16, device=DEV)
        pos = posr([0] * B, DEV) if rows else T.posw(0, DEV)
        count = posr([1] * B, DEV) if rows else None
        if kw.pop("misaligned", None) == "qkv":
            kw["qkv_ptr"] = qkv.data_ptr() + 8
        elif "kc_mis" in kw:
            kw.pop("kc_mis")
            kw["kc_ptr"] = kc.data_ptr() + 8
        rc = call_append(qkv, kc, vc, o, pos, count, H, C, Bq=Bq, Dh=Dh, S_max=S_max, **kw)
        torch.cuda.synchronize()
        assert bool((o == 7.0).all()) and bool((kc == 3.0).all()) and bool((vc == 3.0).all())
        return rc

    name = "jdt_attn_append_rows" if rows else "jdt_attn_append"
    assert case(Dh=32) == -3 and case(Dh=128) == -3
    assert case(S_max=0) == -4 and case(S_max=32769) == -4
    for arg in ("qkv", "kc", "vc", "o", "pos") + (("count",) if rows else ()):
        assert case(null=(arg,)) == -2, arg
    assert case(misaligned="qkv") == -6 and case(kc_mis=True) == -6
    bad_c = case(C=0)
    assert bad_c not in (0, -2, -3, -4, -5, -6) and case(C=1025) == bad_c   # a code of its own
    with pytest.raises(RuntimeError):
        _lib.check(bad_c, name)
    assert case(Bq=0) == 0   # a no-op


def test_longest_cache_accepted():
    """S_max = 32768, the top of the envelope: the last 64 rows appended at once."""
    H, S_max, C = 1, 32768, 64
    p = S_max - C
    qkv, kc, vc = TA.append_inputs(H, C, seed=4, Bq=1, S_max=S_max)
    got, k2, v2 = run(qkv, kc, vc, T.posw(p, DEV), H, C)
    want, _ = TA.attn_append_fp64(qkv, kc, vc, p, C, H)
    T.close(got.view(1, C, -1), want)
    kc[:, :, p:], vc[:, :, p:] = TA.chunk_kv(qkv, 1, C, H)
    assert torch.equal(k2.cpu(), kc) and torch.equal(v2.cpu(), vc)
    o = torch.full((C, 64), 7.0, dtype=torch.bfloat16, device=DEV)
    _, k3, v3 = run(qkv, k2, v2, T.posw(p + 1, DEV), H, C, o=o)   # one row too far: nothing is written
    assert bool((o == 7.0).all()) and torch.equal(k3, k2) and torch.equal(v3, v2)


# ----------------------------------------------------------------------------- 9. embed_append
def test_embed_append():
    TA.body_embed_append(DEV)


# ----------------------------------------------------------------------------- 10-14. model level
@pytest.mark.parametrize("chunk", [64, 100])
@pytest.mark.parametrize("Pn", [1, 2, 65, 250])
def test_teacher_forced_chunked(Pn, chunk):
    TA.body_teacher_forced_chunked(DEV, Pn, chunk)


def test_extend_logits():
    TA.body_extend_logits(DEV)


def test_ragged():
    TA.body_ragged(DEV)


def test_greedy_chunked_captured_equals_eager():
    """generate(prefill_chunk=64) meets the 4 E_full bound eagerly and captured, the captured run
    equals the eager one bit for bit, and the step really was captured."""
    gen_e, eager = TA.body_greedy_chunked(DEV, False)
    eager_logits = gen_e.logits.clone()
    gen_c, graph = TA.body_greedy_chunked(DEV, True)
    assert torch.equal(graph, eager) and torch.equal(gen_c.logits, eager_logits)
    assert gen_c._graphs[gen_c._graph_key()][0] is not None
    assert not gen_e._graphs


def test_edges():
    TA.body_edges(DEV)
