"""The ctypes signatures of the 14 KV-cache attention launchers are generated (``ops/_lib.py``
``_kv_attn_name`` / ``_kv_attn_argtypes``).  A wrong entry does not fail at the call: it corrupts the
arguments on the GPU.  So the lists are pinned here as literals, spelled out from the ``extern "C"``
declarations of csrc/attn_decode.hip and csrc/attn_append.hip; the library is not loaded."""
from ctypes import c_float, c_int, c_long, c_void_p

from jax_distributed_tuts_amd.ops import _lib

P, I, L, F = c_void_p, c_int, c_long, c_float

EXPECTED = {
    # (qkv, k_cache, v_cache, o, pos, B, H, Dh, S_max, scale, stream)
    "jdt_attn_decode": [P, P, P, P, P, I, I, I, I, F, P],
    "jdt_attn_decode_rows": [P, P, P, P, P, I, I, I, I, F, P],
    # (qkv, k_cache, v_cache, o, pos, ws, ws_floats, B, H, Dh, S_max, scale, stream)
    "jdt_attn_decode_long": [P, P, P, P, P, P, L, I, I, I, I, F, P],
    "jdt_attn_decode_long_rows": [P, P, P, P, P, P, L, I, I, I, I, F, P],
    # (qkv, k_cache, v_cache, o, pos, B, C, H, Dh, S_max, scale, stream); per row: (..., pos, count, B, ...)
    "jdt_attn_append": [P, P, P, P, P, I, I, I, I, I, F, P],
    "jdt_attn_append_rows": [P, P, P, P, P, P, I, I, I, I, I, F, P],
    # (qkv, k_cache, v_cache, o, pos, ws, ws_floats, B, C, H, Dh, S_max, scale, stream); per row: (..., pos, count,
    # ws, ...)
    "jdt_attn_append_split": [P, P, P, P, P, P, L, I, I, I, I, I, F, P],
    "jdt_attn_append_split_rows": [P, P, P, P, P, P, P, L, I, I, I, I, I, F, P],
    # (qkv, k_cache, v_cache, k_scale, v_scale, o, pos, B, H, Dh, S_max, scale, stream)
    "jdt_attn_decode_fp8": [P, P, P, P, P, P, P, I, I, I, I, F, P],
    "jdt_attn_decode_fp8_rows": [P, P, P, P, P, P, P, I, I, I, I, F, P],
    # (qkv, k_cache, v_cache, k_scale, v_scale, o, pos, ws, ws_floats, B, H, Dh, S_max, scale, stream)
    "jdt_attn_decode_fp8_long": [P, P, P, P, P, P, P, P, L, I, I, I, I, F, P],
    "jdt_attn_decode_fp8_long_rows": [P, P, P, P, P, P, P, P, L, I, I, I, I, F, P],
    # (qkv, k_cache, v_cache, k_scale, v_scale, o, pos, B, C, H, Dh, S_max, scale, stream); per row: (..., pos,
    # count, B, ...)
    "jdt_attn_append_fp8": [P, P, P, P, P, P, P, I, I, I, I, I, F, P],
    "jdt_attn_append_fp8_rows": [P, P, P, P, P, P, P, P, I, I, I, I, I, F, P],
}


def test_generated_signatures_match_the_declarations():
    generated = {name: sig for name, sig in _lib._SIGS.items() if name.startswith("jdt_attn_decode")
                 or name.startswith("jdt_attn_append")}
    assert sorted(generated) == sorted(EXPECTED)
    for name, argtypes in EXPECTED.items():
        restype, got = generated[name]
        assert restype is c_int, name
        assert got == argtypes, name
