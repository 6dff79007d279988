"""GPU half of the row-kernel value checks: the HIP kernels of csrc/layernorm.hip, csrc/xent.hip and
the row kernels of csrc/attention.hip against float64, element by element, with the bounds derived in
tests/rowcheck.py.  Every case is tiny and sits at a dispatch edge; every case that claims a kernel
variant asserts, through the launchers' own predicates (jdt_ln_bwd_variant, jdt_xent_variant), that it
ran on that variant."""
import pytest
import torch

from jax_distributed_tuts_amd.ops import _lib

from . import rowcheck as rc

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
BF = torch.bfloat16


def _dt(dt):
    return "bf16" if dt == BF else "f32"


# ----------------------------------------------------------------------------- LayerNorm
@pytest.mark.parametrize("xcd", [1, 0])
@pytest.mark.parametrize("d", rc.LN_D)
@pytest.mark.parametrize("T", rc.LN_T)
def test_ln_fwd(T, d, xcd):
    lib = _lib.lib()
    nv = {1: 1, 2: 2}.get((d // 8 + 63) // 64, 4)
    try:
        lib.jdt_ln_set_xcd(xcd)
        assert rc.body_ln_fwd(DEV, T, d, f"ln_fwd<NV={nv}>") <= 1.0
    finally:
        lib.jdt_ln_set_xcd(1)


@pytest.mark.parametrize("T,S,d", rc.LN_EMBED)
def test_ln_fwd_embed(T, S, d):
    nv = {1: 1, 2: 2}.get((d // 8 + 63) // 64, 4)
    assert rc.body_ln_embed(DEV, T, S, d, f"ln_fwd_embed<NV={nv}>") <= 1.0


def _ln_bwd_forced(NV, R, W, d, T, **kw):
    lib = _lib.lib()
    try:
        lib.jdt_ln_set_waves(W)
        lib.jdt_ln_set_rows(R)
        assert lib.jdt_ln_bwd_variant(T, d) == NV | R << 8 | W << 16, "the case does not reach the variant it claims"
        return rc.body_ln_bwd(DEV, T, d, f"ln_bwd<NV={NV},R={R},W={W}>", **kw)
    finally:
        lib.jdt_ln_set_waves(0)
        lib.jdt_ln_set_rows(0)


@pytest.mark.parametrize("xcd", [1, 0])
@pytest.mark.parametrize("NV,R,W,d,T", rc.ln_bwd_cases())
def test_ln_bwd_every_variant(NV, R, W, d, T, xcd):
    lib = _lib.lib()
    try:
        lib.jdt_ln_set_xcd(xcd)
        assert _ln_bwd_forced(NV, R, W, d, T) <= 1.0
    finally:
        lib.jdt_ln_set_xcd(1)


@pytest.mark.parametrize("d", rc.LN_BWD_OPTIONAL)
@pytest.mark.parametrize("with_dres,with_dsum", [(True, True), (True, False), (False, True), (False, False)])
def test_ln_bwd_optional_arguments(d, with_dres, with_dsum):
    NV = {1: 1, 2: 2}.get((d // 8 + 63) // 64, 4)
    assert _ln_bwd_forced(NV, 2, 4, d, 37, with_dres=with_dres, with_dsum=with_dsum) <= 1.0


@pytest.mark.parametrize("NV,R,W,d", [(1, 2, 16, 72), (2, 4, 8, 520), (4, 2, 4, 2048)])
def test_ln_bwd_integer_dy_exact_dbeta(NV, R, W, d):
    assert _ln_bwd_forced(NV, R, W, d, 37, integer_dy=True) <= 1.0


def test_ln_bwd_heuristic_shape():
    """Knobs at 0: T = 1024, d = 512 is the heuristic's 16 waves x 2 rows."""
    assert _lib.lib().jdt_ln_bwd_variant(1024, 512) == 1 | 2 << 8 | 16 << 16
    assert rc.body_ln_bwd(DEV, 1024, 512, "ln_bwd<NV=1,R=2,W=16>") <= 1.0


# ----------------------------------------------------------------------------- softmax cross-entropy
def _xent(M, C, dt, layout="contig", rpw=0, **kw):
    nv = rc.xent_expected_variant(C, dt, layout)
    name = f"xent<narrow,{_dt(dt)}>" if nv == 0 else f"xent<wide NV={nv},rpw={rpw or 'auto'}>"
    lib = _lib.lib()
    try:
        lib.jdt_xent_set_rpw(rpw)
        return rc.body_xent(DEV, M, C, dt, name, layout=layout, expect=nv, **kw)
    finally:
        lib.jdt_xent_set_rpw(0)


@pytest.mark.parametrize("dt", [BF, torch.float32], ids=_dt)
@pytest.mark.parametrize("C", rc.XENT_C)
def test_xent_widths(C, dt):
    assert _xent(9, C, dt) <= 1.0


@pytest.mark.parametrize("slab", [False, True])
@pytest.mark.parametrize("C", rc.XENT_RPW_C)
@pytest.mark.parametrize("rpw,M", [(r, M) for r in rc.XENT_RPW for M in rc.xent_rpw_rows(r)])
def test_xent_rows_per_wave(rpw, M, C, slab):
    assert _xent(M, C, BF, rpw=rpw, slab=slab) <= 1.0


def test_xent_heuristic_rows_per_wave_4():
    """Knob at 0: M = 2048 is the heuristic's rpw = 4 (its dlogits were never value-checked)."""
    assert _xent(2048, 256, BF, slab=True) <= 1.0


@pytest.mark.parametrize("C,dt,layout", rc.XENT_LAYOUTS, ids=lambda v: _dt(v) if isinstance(v, torch.dtype) else str(v))
def test_xent_layouts(C, dt, layout):
    assert _xent(9, C, dt, layout=layout) <= 1.0


@pytest.mark.parametrize("slab", [False, True])
@pytest.mark.parametrize("C", (70, 520))
def test_xent_without_dlogits(C, slab):
    assert _xent(9, C, BF, with_dlogits=False, slab=slab) <= 1.0


@pytest.mark.parametrize("C,dt", rc.XENT_NEG_INF, ids=lambda v: _dt(v) if isinstance(v, torch.dtype) else str(v))
def test_xent_neg_inf_logits(C, dt):
    """-inf logits away from the label, among them a lane's first logit: xent_kernel's per-lane
    online update needs the same -inf guard as its cross-lane merge."""
    assert _xent(9, C, dt, neg_inf=True) <= 1.0


# ----------------------------------------------------------------------------- attention.hip row kernels
@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("Sk", rc.SOFTMAX_SK)
def test_row_softmax(Sk, causal):
    assert rc.body_softmax(DEV, Sk, causal, "attn_softmax") <= 1.0


@pytest.mark.parametrize("M,N", rc.COLSUM_MN)
def test_colsum(M, N):
    assert rc.body_colsum(DEV, M, N, "colsum") <= 1.0
