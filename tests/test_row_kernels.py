"""CPU half of the row-kernel value checks (tests/rowcheck.py): the test bodies of
tests/test_row_kernels_gpu.py run on CPU tensors through the torch path of ops/kernels.py -- the
reference alone must sit inside every bound at every shape -- and one rejection test per checker:
wrong formulas, written in torch and rounded to bf16, must fail at every shape."""
import pytest
import torch

from jax_distributed_tuts_amd.ops import kernels as kern

from . import rowcheck as rc

CPU = torch.device("cpu")
BF = torch.bfloat16
XENT_SHAPES = [(9, C) for C in rc.XENT_C] + sorted({(M, C) for r in rc.XENT_RPW for M in rc.xent_rpw_rows(r)
                                                     for C in rc.XENT_RPW_C})


# ----------------------------------------------------------------------------- the reference passes
@pytest.mark.parametrize("d", rc.LN_D)
@pytest.mark.parametrize("T", rc.LN_T)
def test_ln_fwd(T, d):
    assert rc.body_ln_fwd(CPU, T, d, "ln_fwd<cpu>") <= 1.0


@pytest.mark.parametrize("T,S,d", rc.LN_EMBED)
def test_ln_fwd_embed(T, S, d):
    assert rc.body_ln_embed(CPU, T, S, d, "ln_fwd_embed<cpu>") <= 1.0


@pytest.mark.parametrize("d,T", sorted({(d, T) for _, _, _, d, T in rc.ln_bwd_cases()}))
def test_ln_bwd(d, T):
    assert rc.body_ln_bwd(CPU, T, d, "ln_bwd<cpu>") <= 1.0


@pytest.mark.parametrize("d", rc.LN_BWD_OPTIONAL)
@pytest.mark.parametrize("with_dres,with_dsum", [(True, True), (True, False), (False, True), (False, False)])
def test_ln_bwd_optional_arguments(d, with_dres, with_dsum):
    assert rc.body_ln_bwd(CPU, 37, d, "ln_bwd<cpu>", with_dres=with_dres, with_dsum=with_dsum) <= 1.0


@pytest.mark.parametrize("d", (72, 520, 2048))
def test_ln_bwd_integer_dy_exact_dbeta(d):
    assert rc.body_ln_bwd(CPU, 37, d, "ln_bwd<cpu>", integer_dy=True) <= 1.0


def test_ln_bwd_heuristic_shape():
    assert rc.body_ln_bwd(CPU, 1024, 512, "ln_bwd<cpu>") <= 1.0


@pytest.mark.parametrize("dt", [BF, torch.float32], ids=["bf16", "f32"])
@pytest.mark.parametrize("M,C", XENT_SHAPES)
def test_xent(M, C, dt):
    assert rc.body_xent(CPU, M, C, dt, "xent<cpu>") <= 1.0


@pytest.mark.parametrize("M,C", [(9, 520), (145, 1544)])
def test_xent_slab_fold(M, C):
    assert rc.body_xent(CPU, M, C, BF, "xent<cpu>", slab=True) <= 1.0


@pytest.mark.parametrize("C,dt,layout", rc.XENT_LAYOUTS)
def test_xent_layouts(C, dt, layout):
    assert rc.body_xent(CPU, 9, C, dt, "xent<cpu>", layout=layout) <= 1.0


@pytest.mark.parametrize("C", (70, 520))
def test_xent_without_dlogits(C):
    assert rc.body_xent(CPU, 9, C, BF, "xent<cpu>", with_dlogits=False) <= 1.0


@pytest.mark.parametrize("C,dt", rc.XENT_NEG_INF)
def test_xent_neg_inf_logits(C, dt):
    assert rc.body_xent(CPU, 9, C, dt, "xent<cpu>", neg_inf=True) <= 1.0


@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("Sk", rc.SOFTMAX_SK)
def test_row_softmax(Sk, causal):
    assert rc.body_softmax(CPU, Sk, causal, "attn_softmax<cpu>") <= 1.0


@pytest.mark.parametrize("M,N", rc.COLSUM_MN)
def test_colsum(M, N):
    assert rc.body_colsum(CPU, M, N, "colsum<cpu>") <= 1.0


def test_reduction_depth():
    assert [rc.red(n) for n in (1, 8, 15, 16, 512, 520, 1544, 2048, 2056)] == [1, 8, 15, 15, 15, 23, 39, 39, 47]


# ----------------------------------------------------------------------------- the mutants fail
def _ln_bwd_pieces(T, d):
    x, gamma, beta, dy, dres = rc.ln_inputs(T, d)
    _, mean, rstd = kern.layernorm_fwd(x, gamma, beta)
    xh = (x.float() - mean[:, None]) * rstd[:, None]
    g = dy.float() * gamma
    return x, gamma, dy, dres, mean, rstd, xh, g


@pytest.mark.parametrize("d", rc.LN_D)
@pytest.mark.parametrize("T", rc.LN_T)
def test_rejects_ln_dx_without_xh_s2(T, d):
    x, gamma, dy, dres, mean, rstd, xh, g = _ln_bwd_pieces(T, d)
    dx = (dres.float() + rstd[:, None] * (g - g.mean(-1, keepdim=True))).to(BF)
    with pytest.raises(AssertionError, match="dx"):
        rc.check_ln_bwd(dy, x, mean, rstd, gamma, dx, dres=dres, variant="mutant")


@pytest.mark.parametrize("d", rc.LN_D)
@pytest.mark.parametrize("T", rc.LN_T)
def test_rejects_ln_dx_means_over_padded_width(T, d):
    x, gamma, dy, dres, mean, rstd, xh, g = _ln_bwd_pieces(T, d)
    s1, s2 = g.sum(-1, keepdim=True) / (d + 8), (g * xh).sum(-1, keepdim=True) / (d + 8)
    dx = (dres.float() + rstd[:, None] * (g - s1 - xh * s2)).to(BF)
    with pytest.raises(AssertionError, match="dx"):
        rc.check_ln_bwd(dy, x, mean, rstd, gamma, dx, dres=dres, variant="mutant")


@pytest.mark.parametrize("d", rc.LN_D)
@pytest.mark.parametrize("T", rc.LN_T)
def test_rejects_ln_y_without_beta(T, d):
    x, gamma, beta, _, _ = rc.ln_inputs(T, d)
    _, mean, rstd = kern.layernorm_fwd(x, gamma, beta)
    y = ((x.float() - mean[:, None]) * rstd[:, None] * gamma).to(BF)
    with pytest.raises(AssertionError, match="/y"):
        rc.check_ln_fwd(x, gamma, beta, y, mean, rstd, variant="mutant")


def _xent_pieces(M, C, dt):
    z, y = rc.xent_inputs(M, C, dt)
    zf = z.float()
    valid = ((y >= 0) & (y < C))[:, None]
    lab = y.clamp(0, C - 1).long()
    return z, y, zf, valid, lab, 1.0 / M


@pytest.mark.parametrize("dt", [BF, torch.float32], ids=["bf16", "f32"])
@pytest.mark.parametrize("M,C", XENT_SHAPES)
def test_rejects_xent_gradient_from_row_max(M, C, dt):
    z, y, zf, valid, lab, gs = _xent_pieces(M, C, dt)
    p = torch.exp(zf - zf.max(-1, keepdim=True).values)   # the row max where the LSE belongs
    d = torch.where(valid, (p - torch.nn.functional.one_hot(lab, C)) * gs, torch.zeros_like(p)).to(BF)
    with pytest.raises(AssertionError, match="dlogits"):
        rc.check_xent(z, y, gs, dlogits=d, variant="mutant")


@pytest.mark.parametrize("dt", [BF, torch.float32], ids=["bf16", "f32"])
@pytest.mark.parametrize("M,C", XENT_SHAPES)
def test_rejects_xent_onehot_at_next_class(M, C, dt):
    z, y, zf, valid, lab, gs = _xent_pieces(M, C, dt)
    oh = torch.nn.functional.one_hot((lab + 1) % C, C)
    d = torch.where(valid, (torch.softmax(zf, -1) - oh) * gs, torch.zeros_like(zf)).to(BF)
    with pytest.raises(AssertionError, match="dlogits"):
        rc.check_xent(z, y, gs, dlogits=d, variant="mutant")


@pytest.mark.parametrize("dt", [BF, torch.float32], ids=["bf16", "f32"])
@pytest.mark.parametrize("M,C", XENT_SHAPES)
def test_rejects_accuracy_with_ties_to_the_highest_index(M, C, dt):
    z, y, zf, valid, lab, gs = _xent_pieces(M, C, dt)
    assert bool(((zf == zf.max(-1, keepdim=True).values).sum(-1) > 1).any()), "the inputs hold no tie"
    last = torch.where(zf == zf.max(-1, keepdim=True).values, torch.arange(C)[None, :], -1).max(-1).values
    n = valid.sum().float()
    loss = torch.where(valid[:, 0], torch.logsumexp(zf, -1) - zf.gather(1, lab[:, None])[:, 0], torch.zeros(M))
    metrics = torch.stack([loss.sum(), n, ((last == lab) & valid[:, 0]).sum().float(), n])
    with pytest.raises(AssertionError, match="metrics_counts"):
        rc.check_xent(z, y, gs, metrics=metrics, variant="mutant")


@pytest.mark.parametrize("Sk", rc.SOFTMAX_SK)
def test_rejects_causal_limit_off_by_one(Sk):
    S, _ = rc.softmax_inputs(Sk, True)
    rows = S.shape[0]
    vis = torch.arange(Sk)[None, :] < (torch.arange(rows) % Sk)[:, None]   # q keys where q + 1 belong
    P = torch.softmax(torch.where(vis, S, torch.full_like(S, float("-inf"))), -1)
    P = torch.where(vis, P, torch.zeros_like(P)).to(BF)   # a row with no key: zeros
    with pytest.raises(AssertionError, match="/P"):
        rc.check_softmax_fwd(S, P, Sk, True, variant="mutant")


@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("Sk", rc.SOFTMAX_SK)
def test_rejects_ds_without_rowsum(Sk, causal):
    S, dP = rc.softmax_inputs(Sk, causal)
    P = rc.row_softmax_fwd(S, Sk, causal)
    dS = (P.float() * dP).to(BF)
    with pytest.raises(AssertionError, match="dS"):
        rc.check_softmax_bwd(P, dP, dS, variant="mutant")


@pytest.mark.parametrize("M,N", rc.COLSUM_MN)
def test_rejects_colsum_that_forgets_its_previous_content(M, N):
    x = torch.randn(M, N, generator=torch.Generator().manual_seed(M * N)).to(BF)
    with pytest.raises(AssertionError, match="colsum"):
        rc.check_colsum(x, x.float().sum(0), out0=0.5, variant="mutant")


def test_rejects_nan_and_written_ignored_rows():
    z, y = rc.xent_inputs(9, 70, BF)
    gs = 1.0 / 9
    d = torch.empty(9, 70, dtype=BF)
    kern.softmax_xent(z, y, grad_scale=gs, dlogits=d)
    assert rc.check_xent(z, y, gs, dlogits=d, variant="xent<cpu>") <= 1.0
    bad = d.clone()
    bad[0, 3] = float("nan")
    with pytest.raises(AssertionError, match="dlogits"):
        rc.check_xent(z, y, gs, dlogits=bad, variant="mutant")
    bad = d.clone()
    bad[1, 3] = 2.0 ** -20   # row 1 is ignored (label -1): its gradient is exactly zero
    with pytest.raises(AssertionError, match="dlogits"):
        rc.check_xent(z, y, gs, dlogits=bad, variant="mutant")


def test_summary_has_one_row_per_variant_and_output(tmp_path, monkeypatch):
    log = tmp_path / "ratios.jsonl"
    monkeypatch.setenv("JDT_ORACLE_LOG", str(log))
    rc.body_colsum(CPU, 31, 8, "colsum<cpu>")
    rc.body_colsum(CPU, 33, 8, "colsum<cpu>")
    rc.body_softmax(CPU, 63, True, "attn_softmax<cpu>")
    rows = rc.summarize(str(log)).splitlines()
    assert len(rows) == 4 and rows[1].startswith("attn_softmax<cpu>_bwd/dS") and rows[3].split()[-1] == "2"
