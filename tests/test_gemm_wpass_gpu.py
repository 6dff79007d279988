"""Value checks of the one-launch weight-gradient pass (csrc/gemm.hip ``gemm_wpass_kernel``,
``ops.kernels.gemm_wpass``) against an fp64 reference, for every selectable tile config.

Two kinds of operands:

* integer-valued bf16 operands sized so that every product and every partial sum is an
  integer below 2^24: fp32 accumulation is then exact in ANY order (MFMA order, K-tile
  order, split-K combine order) and the outputs must be *equal* to the fp64 reference;
* Gaussian operands with the worst-case bound of K fp32 accumulations,
  ``K * 2^-23 * (|A|^T |B|)_ij + 2^-23 * |C0_ij|`` (K * 2^-24 * sum|a||b|, doubled because
  the rounding mode inside the MFMA is not documented as round-to-nearest).

Every test that claims to cover the kernel observes its launch (a spy on the library's
``jdt_gemm_wpass_launch``) and the workgroup count, written here as a literal derived by
hand from the planner rule above ``wpass_plan``: sum of (M/BM)*(N/BN) workgroups, each
problem's K split in two while sp < 8, tiles_all*sp < 512, K/(2sp) % 64 == 0 and
K/(2sp) >= 512.  ``_launch_wpass`` falls back to per-problem launches when a plan is
refused, so values alone would not prove the kernel ran.
"""
import math
import types

import numpy as np
import pytest
import torch

from jax_distributed_tuts_amd.ops import _lib
from jax_distributed_tuts_amd.ops import kernels as kern
from jax_distributed_tuts_amd.utils.train_state import adamw

pytestmark = pytest.mark.gpu

DEV = "cuda"
# BM x BN of the configs of jdt_gemm_wpass_launch
TILES = {0: (64, 64), 1: (64, 64), 2: (128, 128), 3: (32, 64), 4: (64, 128), 5: (128, 64)}
CFGS = sorted(TILES)
SENTINEL = 7.0
C0MAX = 1000        # |C0| of the integer-valued initial accumulators
COUNT = 3           # AdamW step counter: the epilogue computes step t = COUNT + 1
GS = 0.25           # grad_scale (a power of two: exact)
TX = adamw(1e-3)
# the kernel receives its hyper-parameters as fp32: the reference does its arithmetic in
# fp64 on those fp32 values (1 - fp32(0.999) is 6e-5 away from 1e-3 relatively)
LR, B1, B2, EPS, WD = (float(np.float32(x)) for x in (TX.learning_rate, TX.b1, TX.b2, TX.eps, TX.weight_decay))
U24 = 2.0 ** -24


class Spy:
    def __init__(self):
        self.totals = []   # workgroup count of every one-launch W pass
        self.gemms = 0     # per-problem launches (the fallback)


@pytest.fixture
def spy(monkeypatch):
    s = Spy()
    L = _lib.lib()
    launch = L.jdt_gemm_wpass_launch
    launch_gemm = kern._launch_gemm

    def wpass_launch(table, total, cfg, stream):
        s.totals.append(int(total))
        return launch(table, total, cfg, stream)

    def one_gemm(*a, **k):
        s.gemms += 1
        return launch_gemm(*a, **k)

    monkeypatch.setattr(L, "jdt_gemm_wpass_launch", wpass_launch)
    monkeypatch.setattr(kern, "_launch_gemm", one_gemm)
    return s


def _mag(n_launches, K, c0max=0):
    """Largest operand magnitude m (<= 127: exact in bf16) with n_launches*K*m^2 + c0max < 2^24."""
    m = min(127, math.isqrt(((1 << 24) - 1 - c0max) // (n_launches * K)))
    assert m >= 1 and n_launches * K * m * m + c0max < (1 << 24)
    return m


def _operand(gen, K, X, mag, pad):
    """bf16 [K, X] operand (integer-valued in [-mag, mag], or Gaussian when mag is None);
    pad: the column slice [:, 8:8+X] of a [K, X+24] buffer (row stride > row, 16-byte
    aligned offset).  Returns (device view, fp64 host copy)."""
    w = X + 24 if pad else X
    full = (torch.randn(K, w, generator=gen) if mag is None
            else torch.randint(-mag, mag + 1, (K, w), generator=gen).float()).to(torch.bfloat16)
    dev = full.to(DEV)
    if pad:
        return dev[:, 8:8 + X], full[:, 8:8 + X].double()
    return dev, full.double()


def _make(gen, M, N, K, mode, *, mag, alpha=1.0, a_pad=False, b_pad=False, out_pad=False, dbias=False, count=None):
    """One problem dW (+)= alpha * A^T B.  mode: "store", "acc" (onto an integer-valued
    C0), "adamw" (accumulate=False: the gradient never goes to memory) or "adamw_acc"
    (gradient = C0 + A^T B, C re-zeroed).  The fp64 references are computed once, here."""
    q = types.SimpleNamespace(M=M, N=N, K=K, mode=mode, alpha=alpha, out_pad=out_pad)
    q.a, ha = _operand(gen, K, M, mag, a_pad)
    q.b, hb = _operand(gen, K, N, mag, b_pad)
    q.AtB = alpha * (ha.T @ hb)
    q.absAtB = ha.abs().T @ hb.abs()
    q.acc = mode in ("acc", "adamw_acc")
    q.C0 = torch.randint(-C0MAX, C0MAX + 1, (M, N), generator=gen).double() if q.acc else None
    if out_pad:
        q.buf = torch.full((M, N + 16), SENTINEL, dtype=torch.float32, device=DEV)
        q.out = q.buf[:, 8:8 + N]
    elif q.acc:
        q.out = q.C0.float().to(DEV)
    else:
        q.out = torch.full((M, N), SENTINEL, dtype=torch.float32, device=DEV)
    q.dbias = torch.zeros(N, dtype=torch.float32, device=DEV) if dbias else None
    q.opt = None
    if mode.startswith("adamw"):
        # not a zero state: from one, step-1 AdamW is lr * sign(g) and hides |g|
        g0 = GS * (q.AtB + (q.C0 if q.acc else 0.0))
        ms = float((g0 * g0).mean())
        q.p = torch.randn(M, N, generator=gen).to(DEV)
        q.m = (torch.randn(M, N, generator=gen) * math.sqrt(ms)).to(DEV)
        q.v = ((0.5 + torch.rand(M, N, generator=gen)) * ms).to(DEV)
        q.s = torch.zeros(M, N, dtype=torch.bfloat16, device=DEV)
        q.count = count
        q.opt = (q.p, q.m, q.v, q.s, types.SimpleNamespace(o={"count": count}, tx=TX, grad_scale=GS))
    return q


def _state(q):
    return types.SimpleNamespace(p=q.p.cpu().double(), m=q.m.cpu().double(), v=q.v.cpu().double())


def _issue(probs):
    for q in probs:
        kern.gemm(q.a, q.b, a_layout="km", b_layout="kn", out=q.out, accumulate=q.acc, alpha=q.alpha,
                  dbias=q.dbias, opt=q.opt)


def _tol_g(q):
    """Worst case of K fp32 accumulations of exact products (+ the add onto C0), doubled."""
    t = q.K * 2.0 ** -23 * q.absAtB
    return t + 2.0 ** -23 * q.C0.abs() if q.C0 is not None else t


def _check_out(q, runs=1, exact=True, ratios=None):
    """A store / accumulate problem after `runs` passes."""
    ref = q.AtB if q.mode == "store" else q.C0 + runs * q.AtB
    got = q.out.cpu().double()
    if exact:
        same = torch.equal(got, ref)
        assert same, f"{q.mode} {q.M}x{q.N}x{q.K}: max |err| {float((got - ref).abs().max())}"
    else:
        assert runs == 1
        err, bound = (got - ref).abs(), _tol_g(q)
        ratios.append(float((err / bound).max()))
        assert bool((err <= bound).all()), f"{q.mode} {q.M}x{q.N}x{q.K}: max err/bound {ratios[-1]}"
    if q.out_pad:   # the columns on both sides of the slice are untouched
        buf = q.buf.cpu()
        assert bool((buf[:, :8] == SENTINEL).all()) and bool((buf[:, 8 + q.N:] == SENTINEL).all())
    if q.dbias is not None:
        assert runs == 1
        dref, dgot = q.AtB.sum(0), q.dbias.cpu().double()
        if exact:
            assert torch.equal(dgot, dref)
        else:
            # every summand within its bound, then an fp32 sum of M terms (any order)
            dtol = _tol_g(q).sum(0) + q.M * 2.0 ** -23 * q.AtB.abs().sum(0)
            assert bool(((dgot - dref).abs() <= dtol).all())


def _check_adamw(q, G, prev, tol_g=None):
    """One epilogue AdamW step from state `prev` with exact fp64 gradient G (tol_g: the
    elementwise bound of the kernel's own gradient for Gaussian operands, else exact)."""
    tol_g = torch.zeros_like(G) if tol_g is None else tol_g
    gr = GS * G
    m1, m2 = B1 * prev.m, (1.0 - B1) * gr
    v1, v2 = B2 * prev.v, (1.0 - B2) * gr * gr
    m, v, p = q.m.cpu().double(), q.v.cpu().double(), q.p.cpu().double()
    # three fp32 roundings (two products, one sum)
    tol_m = 4 * U24 * (m1.abs() + m2.abs()) + (1.0 - B1) * GS * tol_g
    assert bool(((m - (m1 + m2)).abs() <= tol_m).all()), "AdamW m"
    tol_v = 6 * U24 * (v1.abs() + v2) + 2 * (1.0 - B2) * GS * GS * G.abs() * tol_g
    assert bool(((v - (v1 + v2)).abs() <= tol_v).all()), "AdamW v"
    # the update from the kernel's own stored m and v (no gradient error propagates).  powf
    # within a few ulp is amplified by b2^t / (1 - b2^t) ~ 250 at t = 4: < 1e-4 relative in
    # the bias correction, 1e-3 leaves a tenfold margin (no bias correction: a factor 2.9)
    t = COUNT + 1
    u_ref = -LR * ((m / (1.0 - B1 ** t)) / ((v / (1.0 - B2 ** t)).sqrt() + EPS) + WD * prev.p)
    u = p - prev.p
    assert bool(((u - u_ref).abs() <= 1e-3 * u_ref.abs() + 2.0 ** -22 * prev.p.abs()).all()), "AdamW p"
    assert torch.equal(q.s, q.p.to(torch.bfloat16)), "bf16 shadow"
    out = q.out.cpu()
    if q.acc:
        assert bool((out == 0).all()), "accumulated gradient re-zeroed"
    else:
        assert bool((out == SENTINEL).all()), "the fused gradient never goes to memory"
    assert int(q.count.item()) == COUNT, "the epilogue does not advance the step"


# --------------------------------------------------------------------------- the mixed set
def _mixed(cfg, gen, gaussian=False, p1_m=None):
    """Five problems, 1 + 2 + 3 + 6 + 1 = 13 tiles, every K < 1024 (no split-K).  The ring
    has 3 slots: P0 has one K-tile, P1 two (depth - 1), P2 three (depth), P3 five."""
    BM, BN = TILES[cfg]
    count = torch.tensor([COUNT], dtype=torch.int32, device=DEV)

    def mag(K, c0=0):
        return None if gaussian else _mag(1, K, c0)

    return [
        _make(gen, BM, BN, 64, "store", mag=mag(64), out_pad=True),
        _make(gen, 2 * BM if p1_m is None else p1_m, BN, 128, "acc", mag=mag(128, C0MAX), a_pad=True),
        # dbias: BM (<= 128) * 192 * 15^2 * 0.5 = 2.8e6 half-integers, exact in fp32
        _make(gen, BM, 3 * BN, 192, "store", mag=None if gaussian else 15, alpha=0.5, dbias=True),
        _make(gen, 3 * BM, 2 * BN, 320, "adamw", mag=mag(320), b_pad=True, count=count),
        _make(gen, BM, BN, 256, "adamw_acc", mag=mag(256, C0MAX), count=count),
    ]


def _check_mixed(probs, prev, exact=True, ratios=None):
    for q in probs[:3]:
        _check_out(q, exact=exact, ratios=ratios)
    for q, pv in zip(probs[3:], prev):
        G = q.AtB + q.C0 if q.acc else q.AtB
        _check_adamw(q, G, pv, None if exact else _tol_g(q))


@pytest.mark.parametrize("cfg", CFGS)
def test_mixed_set_exact(cfg, spy):
    probs = _mixed(cfg, torch.Generator().manual_seed(100 + cfg))
    prev = [_state(q) for q in probs[3:]]
    with kern.gemm_wpass(cfg):
        _issue(probs)
    torch.cuda.synchronize()
    # 13 workgroups: not a multiple of 8, the remainder branch of the XCD remap runs
    assert spy.totals == [13] and spy.gemms == 0
    _check_mixed(probs, prev)


@pytest.mark.parametrize("cfg", CFGS)
def test_mixed_set_gaussian(cfg, spy):
    probs = _mixed(cfg, torch.Generator().manual_seed(7), gaussian=True)
    prev = [_state(q) for q in probs[3:]]
    with kern.gemm_wpass(cfg):
        _issue(probs)
    torch.cuda.synchronize()
    assert spy.totals == [13] and spy.gemms == 0
    ratios = []
    try:
        _check_mixed(probs, prev, exact=False, ratios=ratios)
    finally:
        print(f"[wpass gaussian cfg {cfg}] max err/bound {max(ratios):.4f} (per problem: "
              + ", ".join(f"{r:.4f}" for r in ratios) + ")")


# --------------------------------------------------------------------------- split-K
def _splitk(cfg, gen, launches):
    """Q0 sp 2, Q1 sp 8, Q2 sp 4, Q3 sp 1 (K/2 = 96 is no multiple of 64): 2*2 + 8 + 4 + 1
    = 17 workgroups, each split problem with its own workspace and counter offsets."""
    BM, BN = TILES[cfg]
    count = torch.tensor([COUNT], dtype=torch.int32, device=DEV)
    return [
        _make(gen, BM, 2 * BN, 1024, "acc", mag=_mag(launches, 1024, C0MAX)),
        _make(gen, BM, BN, 4096, "adamw_acc", mag=_mag(launches, 4096, C0MAX), count=count),
        _make(gen, BM, BN, 2048, "adamw", mag=_mag(launches, 2048), count=count),
        _make(gen, BM, BN, 192, "store", mag=_mag(launches, 192)),
    ]


@pytest.mark.parametrize("cfg", CFGS)
def test_split_k_set_twice(cfg, spy):
    q0, q1, q2, q3 = probs = _splitk(cfg, torch.Generator().manual_seed(200 + cfg), launches=2)
    prev1, prev2 = _state(q1), _state(q2)
    with kern.gemm_wpass(cfg):
        _issue(probs)
    torch.cuda.synchronize()
    assert spy.totals == [17] and spy.gemms == 0
    _check_out(q0, runs=1)
    _check_out(q3)
    _check_adamw(q1, q1.C0 + q1.AtB, prev1)
    _check_adamw(q2, q2.AtB, prev2)
    # the second step of each AdamW problem starts from the state the kernel stored
    prev1, prev2 = _state(q1), _state(q2)
    # the same plan key again: a cache hit, and the arrival counters re-armed by the first pass
    with kern.gemm_wpass(cfg):
        _issue(probs)
    torch.cuda.synchronize()
    assert spy.totals == [17, 17] and spy.gemms == 0
    _check_out(q0, runs=2)
    _check_out(q3)
    _check_adamw(q1, q1.AtB, prev1)   # its accumulator was re-zeroed: C0 = 0
    _check_adamw(q2, q2.AtB, prev2)


# --------------------------------------------------------------------------- table boundary, fallbacks
def _small(gen, n):
    return [_make(gen, 64, 64, 64, "store", mag=127) for _ in range(n)]


def test_table_full(spy):
    probs = _small(torch.Generator().manual_seed(40), 40)   # WP_MAX
    with kern.gemm_wpass(0):
        _issue(probs)
    torch.cuda.synchronize()
    assert spy.totals == [40] and spy.gemms == 0
    for q in probs:
        _check_out(q)


def test_table_overflow_falls_back(spy):
    probs = _small(torch.Generator().manual_seed(41), 41)
    with kern.gemm_wpass(0):
        _issue(probs)
    torch.cuda.synchronize()
    assert spy.totals == [] and spy.gemms == 41
    for q in probs:
        _check_out(q)


def test_outside_envelope_falls_back(spy):
    # M = 128 + 32 is no multiple of config 2's tile: the plan is refused
    probs = _mixed(2, torch.Generator().manual_seed(42), p1_m=128 + 32)
    prev = [_state(q) for q in probs[3:]]
    with kern.gemm_wpass(2):
        _issue(probs)
    torch.cuda.synchronize()
    assert spy.totals == [] and spy.gemms == len(probs)
    _check_mixed(probs, prev)


def test_graph_replay(spy):
    q0, q1, q2, q3 = probs = _splitk(0, torch.Generator().manual_seed(43), launches=3)
    with kern.gemm_wpass(0):   # eager: plans the set
        _issue(probs)
    torch.cuda.synchronize()
    assert spy.totals == [17] and spy.gemms == 0
    kern.workspace(torch.device(DEV, torch.cuda.current_device()))   # (pre-creates the capture stream's buffers)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        with kern.gemm_wpass(0):
            _issue(probs)
    assert spy.totals == [17, 17] and spy.gemms == 0   # the captured pass is the one launch too
    graph.replay()
    graph.replay()
    torch.cuda.synchronize()
    _check_out(q0, runs=3)
    _check_out(q3)
    assert bool((q1.out == 0).all()) and bool((q2.out == SENTINEL).all())


def test_set_first_seen_in_capture(spy):
    probs = _mixed(0, torch.Generator().manual_seed(44))
    prev = [_state(q) for q in probs[3:]]
    kern.workspace(torch.device(DEV, torch.cuda.current_device()))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        with kern.gemm_wpass(0):
            _issue(probs)
    assert spy.totals == [] and spy.gemms == len(probs)   # no plan upload inside a capture
    graph.replay()
    torch.cuda.synchronize()
    _check_mixed(probs, prev)
