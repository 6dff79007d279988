"""What the persistent run-ahead launch (ops/csrc/mlp_fused.hip mlp2_pst_kernel) does once
per launch or spreads over the workgroup instead of repeating per step -- the batch
fragments and labels in registers (PstX), the constant zero padding of its dlogits / W2
LDS images, the CE on four lanes per row -- against one launch per step (JDT_MLP2_PST=0),
which loads, fills and computes all of it every step with one lane per row.

Bounds: tests/test_mlp2_persistent_gpu.py's (the two forms differ only in the arrival
order of the forward's fp32 logit atomics: AdamW median |d| <= 1e-5 x scale and 99.9th
percentile <= 1e-4 x scale, SGD max |d| <= 1e-5 x scale); bitwise with
JDT_DETERMINISTIC=1, where the logits are summed in column-block order.

Shapes: 32 rows (96 padded rows), 100 (clamped rows, padding inside a 32-row k step of the
dW1 MFMA and inside a wave's 16-row CE tile) and 128; 128 hidden units (the smallest the
persistent launch accepts: jdt_mlp2_pst_ok needs H % 128 == 0, so 64 is refused) and 512."""
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)


def _batch(rows, seed):
    from jax_distributed_tuts_amd.utils.train_state import Batch

    g = torch.Generator().manual_seed(seed)
    return Batch(torch.randn(rows, 784, generator=g).to(DEV),
                 torch.randint(0, 10, (rows,), generator=g).to(torch.int32).to(DEV))


def _trainer(opt, hidden, pst, det, monkeypatch):
    from jax_distributed_tuts_amd.models.mlp import Classifier
    from jax_distributed_tuts_amd.parallel.dp import DataParallelTrainer, DPConfig, init_dp

    monkeypatch.setenv("JDT_MLP2_PST", pst)
    monkeypatch.setenv("JDT_DETERMINISTIC", "1" if det else "0")
    st = init_dp(Classifier(hidden_size=hidden), opt, 69, DEV)
    return st, DataParallelTrainer(st, None, DPConfig(4, "kernel"))


def _result(st, tr):
    tr.finalize()
    torch.cuda.synchronize()
    o = st.opt_state
    out = {"p": st.params.master.clone(), "metrics": tr.metrics.clone(), "count": int(o["count"].item())}
    if "m" in o:
        out["m"], out["v"] = o["m"].clone(), o["v"].clone()
    assert int(tr.fused.ztick[1]) == 0   # no tile-map / barrier error word
    return out


def _compare(ref, got, det, sgd, tag):
    assert ref["count"] == got["count"]
    keys = [k for k in ("p", "m", "v") if k in ref]
    if det:
        for k in keys + ["metrics"]:
            assert torch.equal(ref[k], got[k]), (tag, k, float((ref[k] - got[k]).abs().max()))
        return
    for k in keys:
        d = (ref[k] - got[k]).abs().flatten().float().cpu()
        scale = float(ref[k].abs().max())
        ds = d.sort().values
        q50, q999 = float(ds[len(ds) // 2]), float(ds[int(0.999 * (len(ds) - 1))])
        print(f"[{tag}] {k}: max |d| {float(ds[-1]):.3e} (scale {scale:.3e}) median {q50:.3e} p99.9 {q999:.3e}")
        if sgd:
            assert float(ds[-1]) <= 1e-5 * scale, (tag, k, "max", float(ds[-1]))
        else:
            assert q50 <= 1e-5 * scale, (tag, k, "median", q50)
            assert q999 <= 1e-4 * scale, (tag, k, "p99.9", q999)
    torch.testing.assert_close(got["metrics"], ref["metrics"], rtol=1e-5, atol=1e-3)


def _opt(name):
    from jax_distributed_tuts_amd.utils.train_state import adamw, sgd

    return adamw(1e-3) if name == "adamw" else sgd(0.05)


def _replays(rows, hidden, n, opt, pst, det, monkeypatch, second=None):
    """One eager step, then replays of the captured n-step graph (a persistent launch each
    with pst = "1").  Deterministic: cold then primed (the second launch reloads what the
    first kept in registers).  With ``second``: that batch copied into the captured tensors
    between two replays (both then start with their forward).  Otherwise one replay: every
    further step on the logit atomics is another chance that the two forms' arrival orders
    round a logit to different bf16 values, which AdamW's first steps carry on."""
    st, tr = _trainer(_opt(opt), hidden, pst, det, monkeypatch)
    b = _batch(rows, 11)
    tr.step(b)
    assert tr.fused.ahead_ok and tr.fused.pst_ok == (pst == "1")
    tr.capture(b, steps_per_graph=n)
    replays = 2 if (det or second is not None) else 1
    tr.run_steps(b, n)
    if second is not None:
        tr.set_batch(second)
    if replays == 2:
        tr.run_steps(b, n)
    assert tr.multi is not None and tr.multi[0] == n
    out = _result(st, tr)
    assert out["count"] == 1 + replays * n
    return out


@pytest.mark.parametrize("det", [True, False], ids=["det", "atomics"])
@pytest.mark.parametrize("opt", ["adamw", "sgd"])
@pytest.mark.parametrize("n", [2, 3])
@pytest.mark.parametrize("hidden", [128, 512])
@pytest.mark.parametrize("rows", [32, 100, 128])
def test_persistent_replay_matches_per_step_launches(rows, hidden, n, opt, det, monkeypatch):
    """Measured (six runs of the file): every deterministic case bitwise equal every time; the
    SGD and the H = 128 atomics cases bit-identical; the AdamW atomics cases at H = 512 are
    bit-identical in some runs and in others differ by one recurring set of figures per case,
    which for n = 3 is outside the p99.9 bound: [128-512-3-adamw-atomics] p: max |d|
    1.154e-4, median 2.217e-7, p99.9 1.218e-5 against 1e-4 x scale = 1.040e-5 (failed in 3 of
    6 runs, once with two replays: p99.9 2.465e-5), [32-512-3-adamw-atomics] failed in 1 of 6;
    [128-512-2-adamw-atomics] p99.9 7.864e-6, inside.  The parent commit's kernels give the
    same figures to every printed digit ([128-512-3]: 4 of 5 runs; [128-512-2] likewise), so
    the miss is the two forms' usual arrival orders rounding a logit of this batch to
    different bf16 neighbours, carried on by AdamW's first steps -- not the work this file
    checks.  The bounds and cases stand as set; the atomics cases fail in such runs."""
    ref = _replays(rows, hidden, n, opt, "0", det, monkeypatch)
    got = _replays(rows, hidden, n, opt, "1", det, monkeypatch)
    _compare(ref, got, det, opt == "sgd", f"pst rows {rows} H {hidden} n {n} {opt}")


@pytest.mark.parametrize("det", [True, False], ids=["det", "atomics"])
@pytest.mark.parametrize("opt", ["adamw", "sgd"])
@pytest.mark.parametrize("rows,hidden,n", [(100, 128, 2), (128, 512, 3), (32, 512, 2)])
def test_new_batch_between_launches(rows, hidden, n, opt, det, monkeypatch):
    """The same captured graph replayed on a second batch written into the captured
    tensors: a launch that kept the first batch's X fragments or labels gives another
    result than the per-step launches, which read both every step.  Deterministic cases:
    bitwise equal in every run.  [128-512-3-adamw-atomics] missed the p99.9 bound in 2 of 6
    runs (p99.9 2.023e-5 against 1e-4 x scale ~ 1.04e-5): the arrival-order effect described
    in test_persistent_replay_matches_per_step_launches, over two replays."""
    second = _batch(rows, 12)
    ref = _replays(rows, hidden, n, opt, "0", det, monkeypatch, second=second)
    got = _replays(rows, hidden, n, opt, "1", det, monkeypatch, second=second)
    _compare(ref, got, det, opt == "sgd", f"pst new batch rows {rows} H {hidden} n {n} {opt}")
    # the second batch did reach the steps: the same two replays on the first batch's values differ
    same = _replays(rows, hidden, n, opt, "1", det, monkeypatch, second=_batch(rows, 11))
    assert not torch.equal(same["p"], got["p"])


def _ce_case(rows, hidden, pst, monkeypatch):
    """Two steps from an init whose first-step logits have ties in the maximum and a wide
    spread: W2's columns 3 and 7 equal and scaled (rows whose largest logit is class 3 tie
    with class 7), the first 10 rows of X zero with zero biases (all ten logits equal)."""
    st, tr = _trainer(_opt("adamw"), hidden, pst, True, monkeypatch)
    P = st.params
    w2 = P.p("output_dense/kernel")
    w2.mul_(60.0)
    w2[:, 7] = w2[:, 3]
    P.p("input_dense/bias").zero_()
    P.p("output_dense/bias").zero_()
    P.sync_shadow()
    b = _batch(rows, 21)
    b.inputs[:10].zero_()
    r = torch.arange(rows, device=DEV)
    b.labels.copy_(torch.where(r % 3 == 0, 3, torch.where(r % 3 == 1, 7, b.labels)).to(torch.int32))
    eng = tr._fused_engine(b)
    assert eng.ahead_ok and eng.pst_ok == (pst == "1")
    eng.run_ahead(b, 2)   # the first step's forward, then one 2-step launch / two launches
    out = _result(st, tr)
    # step 0's logits: its per-column-block partials (set 0 of 3) summed in block order
    lg = torch.zeros(rows, 10, device=DEV)
    for q in range(hidden // 16):
        lg = lg + eng.det_logits[0, q]
    out["logits0"] = lg.bfloat16().float()
    return out


@pytest.mark.parametrize("rows,hidden", [(100, 128), (128, 512)])
def test_ce_ties_and_spread_bitwise(rows, hidden, monkeypatch):
    """The four-lanes-per-row CE against the one-lane-per-row CE of the per-step kernel on
    logits with two equal largest classes (argmax = the lower), all-equal rows and a spread
    past +-80, deterministic mode: loss sum, hit count, parameters and moments bitwise.  (A
    persistent launch has at least two steps, so the comparison is after two; the second
    step starts from the first's parameters, so a difference in the first shows.)"""
    ref = _ce_case(rows, hidden, "0", monkeypatch)
    got = _ce_case(rows, hidden, "1", monkeypatch)
    lg = ref["logits0"]
    assert torch.equal(lg, got["logits0"])
    top = lg.max(dim=1).values
    ties = ((lg == top[:, None]).sum(dim=1) >= 2)
    assert int(ties[10:].sum()) >= 3, "rows with two equal largest classes"
    assert bool((lg[:10] == lg[:10, :1]).all()), "all-equal rows"
    assert float(lg.max()) >= 80.0 and float(lg.min()) <= -80.0, (float(lg.min()), float(lg.max()))
    assert ref["count"] == got["count"] == 2
    for k in ("metrics", "p", "m", "v"):
        assert torch.equal(ref[k], got[k]), (k, float((ref[k] - got[k]).abs().max()))
