"""Elementwise fp64 checks of the one-wave-per-row kernels (csrc/layernorm.hip, csrc/xent.hip and
the row kernels of csrc/attention.hip), plus the test bodies that tests/test_row_kernels.py (CPU
tensors, the torch path of ops/kernels.py) and tests/test_row_kernels_gpu.py (the HIP kernels) share.

Every checker takes the tensors a kernel consumed and produced, moves them to the CPU, rebuilds the
operation in float64 from exactly the inputs the kernel read, asserts a bound per element and returns
the worst ``err / bound``.  Nothing here is fitted to an observed error; the bounds are:

* bf16 outputs: ``|got - ref| <= 2^-8 |ref| + e32``.  2^-8 is one round-to-nearest bf16 rounding
  (8 significand bits); ``e32`` bounds the error of the fp32 value v that was rounded, times
  (1 + 2^-8) because the rounding is relative to v, not to ref, plus 2^-125 for results that
  underflow (flushed subnormals).  ``e32 = 2^-24 * n_ops * A`` (+ terms named in the checker): A sums
  the absolute values of the addends of the element's expression, n_ops counts the fp32 roundings on
  its longest dependency chain.  A row reduction over n elements counts as ``red(n)``, the additions
  one addend passes through in these kernels: a lane first adds its own elements serially (8 per
  16-byte chunk, at most ceil(n / 512) chunks; the scalar kernels ceil(n / 64) <= that), then the
  wave's 64 partial sums are combined in at most 7 further additions (DPP or butterfly), and never
  more than n: red(n) = min(n, 8 ceil(n / 512) + 7).  A sum errs by at most that depth times 2^-24
  sum|addends|.  (Counting the reduction as n instead would let a wrong divisor d + 8 pass at
  d = 2048; the depth is what the code does.)  Fused multiply-adds only remove roundings.
* fp32 sums built with atomics: ``|got - ref| <= (n + 8) 2^-24 sum|addends|`` for n addends in any
  order; the 8 covers the few roundings inside each addend (e.g. dy * xh: 3).
* fp32 per-row outputs keep the tolerances of tests/test_kernels_gpu.py (1e-5 mean, 1e-4 rstd,
  1e-4 row loss) but per row, against that row's own scale.
* counts, ignored rows, masked columns and the fused embedding are exact.

With ``JDT_ORACLE_LOG`` set (the convention of tests/oracle.py) every checker appends its worst ratio
per output; ``python -m tests.rowcheck LOG`` folds such a log into one row per (variant, output).
"""
from __future__ import annotations

import json
import os
import sys
from typing import Optional

import torch

from jax_distributed_tuts_amd.ops import kernels as kern

U32 = 2.0 ** -24     # fp32 unit roundoff
UBF = 2.0 ** -8      # bf16 unit roundoff
TINY = 2.0 ** -125   # underflow floor


def _log(variant: str, name: str, ratio: float):
    path = os.environ.get("JDT_ORACLE_LOG")
    if path:
        with open(path, "a") as f:
            f.write(json.dumps({"test": os.environ.get("PYTEST_CURRENT_TEST", "").split(" ")[0],
                                "name": f"{variant}/{name}", "ratio": ratio}) + "\n")


def _bounded(variant: str, name: str, got: torch.Tensor, ref: torch.Tensor, bound: torch.Tensor) -> float:
    """assert |got - ref| <= bound elementwise (a NaN fails); returns max err / bound."""
    got, ref, bound = got.detach().cpu().double(), ref.double(), bound.double().expand_as(ref)
    assert got.shape == ref.shape, f"{variant}/{name}: shape {tuple(got.shape)} vs {tuple(ref.shape)}"
    err = (got - ref).abs()
    ok = err <= bound
    ratio = torch.where(ok & (err == 0), torch.zeros_like(err), err / bound)
    ratio = torch.where(torch.isnan(ratio), torch.full_like(ratio, float("inf")), ratio)
    worst = float(ratio.max()) if ratio.numel() else 0.0
    _log(variant, name, worst)
    if not bool(ok.all()):
        i = int(ratio.flatten().argmax())
        idx = tuple(int(v) for v in torch.unravel_index(torch.tensor(i), ref.shape)) if ref.dim() else ()
        raise AssertionError(f"{variant}/{name}: {int((~ok).sum())} of {ok.numel()} elements outside the bound; worst at "
                             f"{idx}: got {float(got.flatten()[i])!r} ref {float(ref.flatten()[i])!r} "
                             f"bound {float(bound.flatten()[i]):.3e} (err / bound = {worst:.3g})")
    return worst


def _exact(variant: str, name: str, got: torch.Tensor, ref: torch.Tensor) -> float:
    got = got.detach().cpu()
    same = torch.equal(got.double(), ref.double())
    _log(variant, name, 0.0 if same else float("inf"))
    assert same, f"{variant}/{name}: not exact: got {got.flatten()[:8].tolist()} want {ref.flatten()[:8].tolist()}"
    return 0.0


def _bf16_bound(ref: torch.Tensor, e32: torch.Tensor) -> torch.Tensor:
    return UBF * ref.abs() + (1 + UBF) * e32 + TINY


def red(n: int) -> int:
    """Additions one addend of an n-element row reduction passes through (module docstring)."""
    return min(n, 8 * ((n + 511) // 512) + 7)


def _c64(t):
    return None if t is None else t.detach().cpu().double()


# ----------------------------------------------------------------------------- LayerNorm
def check_ln_fwd(x, gamma, beta, y, mean, rstd, eps: float = 1e-6, variant: str = "ln_fwd") -> float:
    """ln_fwd_kernel: mean = sum(x) / d; rstd = rsqrt(sum((x - mean)^2) / d + eps);
    y = bf16(fma((x - mean) * rstd, gamma, beta)), everything in fp32 from bf16 x.

    mean, rstd (per row): the existing tolerances, against mean|x_row| and rstd.

    y: A = |xh gamma| + |beta|.  Roundings on the chain of one element: x - mean (1), * rstd (1), the
    fma (1), and rstd's own relative error -- the variance reduction (red(d), halved by the square root
    but counted whole), its squares, the division, + eps and rsqrtf (<= 2 ulp): n_ops = red(d) + 8.
    One term is not relative to A: x - mean cancels, so the error of ``mean`` itself, dm =
    (red(d) + 1) 2^-24 mean|x_row| (the row reduction and the division), reaches y amplified by
    rstd |gamma|; squared it also shifts the variance (sum(x - mean) = 0 kills the first order):
        e32 = 2^-24 ((red(d) + 8) A + (red(d) + 1) rstd |gamma| mean|x|) + (dm rstd)^2 / 2 |xh gamma|."""
    X, G, B = _c64(x), _c64(gamma), _c64(beta)
    d = X.shape[1]
    m = X.mean(-1)
    r = 1.0 / torch.sqrt(((X - m[:, None]) ** 2).mean(-1) + eps)
    absx = X.abs().mean(-1)
    worst = _bounded(variant, "mean", mean, m, 1e-5 * absx + TINY)
    worst = max(worst, _bounded(variant, "rstd", rstd, r, 1e-4 * r))
    xhg = (X - m[:, None]) * r[:, None] * G
    dm = U32 * (red(d) + 1) * absx
    e32 = U32 * ((red(d) + 8) * (xhg.abs() + B.abs()) + (red(d) + 1) * (r * absx)[:, None] * G.abs()) \
        + 0.5 * ((dm * r) ** 2)[:, None] * xhg.abs()
    ref = xhg + B
    return max(worst, _bounded(variant, "y", y, ref, _bf16_bound(ref, e32)))


def check_embed_bits(tok, wte, wpe, S: int, x_out, variant: str = "ln_fwd_embed") -> float:
    """x_out = bf16(wte[tok] + wpe[row % S]): one IEEE fp32 add of two bf16 values and one rounding to
    bf16, both correctly rounded and so reproducible bit for bit (the definition, not an estimate)."""
    T = tok.shape[0]
    pos = torch.arange(T) % S
    ref = (wte.detach().cpu().float()[tok.cpu().long()] + wpe.detach().cpu().float()[pos]).to(torch.bfloat16)
    return _exact(variant, "embed", x_out.detach().cpu().view(torch.int16), ref.view(torch.int16))


def ln_bwd_ref(dy, x, mean, rstd, gamma, dres=None):
    """fp64 (dx, A, xh, g) of the LayerNorm backward from the kernel's own inputs."""
    DY, X, M, R, G = _c64(dy), _c64(x), _c64(mean), _c64(rstd), _c64(gamma)
    xh = (X - M[:, None]) * R[:, None]
    g = DY * G
    s1, s2 = g.mean(-1, keepdim=True), (g * xh).mean(-1, keepdim=True)
    dx = R[:, None] * (g - s1 - xh * s2)
    # the row reductions cancel: their error is relative to mean|g| and mean|g xh|, not |s1|, |s2|
    A = R[:, None] * (g.abs() + g.abs().mean(-1, keepdim=True) + xh.abs() * (g * xh).abs().mean(-1, keepdim=True))
    if dres is not None:
        dx, A = dx + _c64(dres), A + _c64(dres).abs()
    return dx, A, xh, g


def check_ln_bwd(dy, x, mean, rstd, gamma, dx, dres=None, dgamma=None, dbeta=None, dsum=None, dgamma0=0.0,
                 dbeta0=0.0, dsum0=0.0, exact_dbeta: bool = False, variant: str = "ln_bwd") -> float:
    """ln_bwd_kernel, from the fp32 mean / rstd it was given:
    xh = (x - mean) rstd; g = dy gamma; s1 = sum(g) / d; s2 = sum(g xh) / d;
    dx = bf16(dres + rstd (g - s1 - xh s2)).

    dx: A = |dres| + rstd (|g| + mean|g| + |xh| mean|g xh|) (the means of absolute values: the row
    reductions' addends).  Longest chain, through xh s2: xh (2), g (1), g xh (1), the reduction (red(d)),
    / d (<= 2 ulp), xh s2 (1), two subtractions, * rstd, + dres: n_ops = red(d) + 12.
    dgamma / dbeta: atomic sums of dy xh / dy over the T rows on top of their previous content.
    dsum: the atomic sum of the bf16 dx the kernel stored (its definition in the code)."""
    T, d = x.shape
    ref, A, xh, _ = ln_bwd_ref(dy, x, mean, rstd, gamma, dres)
    worst = _bounded(variant, "dx", dx, ref, _bf16_bound(ref, U32 * (red(d) + 12) * A))
    DY = _c64(dy)
    if dgamma is not None:
        t = DY * xh
        worst = max(worst, _bounded(variant, "dgamma", dgamma, t.sum(0) + dgamma0,
                                    (T + 9) * U32 * (t.abs().sum(0) + abs(dgamma0)) + TINY))
    if dbeta is not None:
        if exact_dbeta:
            worst = max(worst, _exact(variant, "dbeta_exact", dbeta, DY.sum(0) + dbeta0))
        else:
            worst = max(worst, _bounded(variant, "dbeta", dbeta, DY.sum(0) + dbeta0,
                                        (T + 9) * U32 * (DY.abs().sum(0) + abs(dbeta0)) + TINY))
    if dsum is not None:
        own = _c64(dx)
        worst = max(worst, _bounded(variant, "dsum", dsum, own.sum(0) + dsum0,
                                    (T + 9) * U32 * (own.abs().sum(0) + abs(dsum0)) + TINY))
    return worst


# ----------------------------------------------------------------------------- softmax cross-entropy
def xent_ref(logits, labels, grad_scale):
    """fp64 pieces of the softmax-CE from the logits the kernel read (fp32 or bf16)."""
    Z = _c64(logits)
    M, C = Z.shape
    lab = labels.detach().cpu().long()
    valid = (lab >= 0) & (lab < C)
    lc = lab.clamp(0, C - 1)
    lse = torch.logsumexp(Z, -1)
    p = torch.exp(Z - lse[:, None])
    oh = torch.nn.functional.one_hot(lc, C).double()
    zl = Z.gather(1, lc[:, None])[:, 0]
    loss = torch.where(valid, lse - zl, torch.zeros_like(lse))
    d = torch.where(valid[:, None], (p - oh) * grad_scale, torch.zeros_like(p))
    # argmax with ties to the lowest index (xent.hip: `z > best`, then the lowest index across lanes)
    first = torch.where(Z == Z.max(-1, keepdim=True).values, torch.arange(C)[None, :], C).min(-1).values
    correct = (first == lc) & valid
    return dict(Z=Z, valid=valid, lab=lc, lse=lse, p=p, oh=oh, zl=zl, loss=loss, d=d, correct=correct)


def check_xent(logits, labels, grad_scale, dlogits=None, dbias=None, metrics=None, row_loss=None, dbias0=0.0,
               metrics0=(0.0, 0.0, 0.0, 0.0), variant: str = "xent") -> float:
    """xent_kernel / xent_vec_kernel: lse = mx + log(sum exp(z - mx)); loss = lse - z_label;
    dlogits = bf16((exp(z - lse) - onehot) grad_scale); rows with label < 0 or >= C give zeros.

    dlogits: A = grad_scale (p + onehot).  n_ops = 4 red(C) + 12: the sum of the exponentials is at
    most red(C) deep, and in the online form of xent_kernel every step (rescale by a 2-ulp exp,
    multiply, add) costs up to 4 roundings; then the 2-ulp log, mx + log s, z - lse, the 2-ulp exp, the
    subtraction of the one-hot, the multiply by grad_scale (12 with some slack for grad_scale's own
    fp32 rounding).  Terms relative to p alone, from the fast exponential and logarithm
    (__expf(a) = exp2(a log2e): a's rounding and the product's, 2^-23 |a| relative):
      its own argument, 2 |z - lse|; lse = mx + log(s) rounded once, |lse|; __logf(s) = log2(s) ln2,
      2 |log s|; the arguments inside the sum (or along the rescale chain, which telescopes), at
      most 2 (max z - min z) over the row's finite logits.
        e32 = 2^-24 grad_scale ((4 red(C) + 12) (p + onehot) + p (2 |z - lse| + |lse| + 2 |log s| + 2 range)).
    row_loss: 1e-4 (|lse| + |z_label| + 1) per row.  metrics[0]: the atomic sum of the row losses the
    kernel stored (of the fp64 losses with their tolerance when row_loss was not requested);
    metrics[1..3] = (n, correct, n) exact.  dbias: the atomic sum of the stored bf16 dlogits."""
    R = xent_ref(logits, labels, grad_scale)
    Z, valid, p = R["Z"], R["valid"], R["p"]
    M, C = Z.shape
    n = int(valid.sum())
    worst = 0.0
    row_tol = 1e-4 * (R["lse"].abs() + torch.where(valid, R["zl"].abs(), torch.zeros_like(R["zl"])) + 1)
    if row_loss is not None:
        worst = max(worst, _bounded(variant, "row_loss", row_loss, R["loss"], torch.where(valid, row_tol, 0 * row_tol)))
    if dlogits is not None:
        fin = torch.isfinite(Z)
        zmax = torch.where(fin, Z, torch.full_like(Z, -1e300)).max(-1).values
        zmin = torch.where(fin, Z, torch.full_like(Z, 1e300)).min(-1).values
        arg = 2 * torch.nan_to_num((Z - R["lse"][:, None]).abs(), posinf=0.0) \
            + (R["lse"].abs() + 2 * (R["lse"] - zmax).abs() + 2 * (zmax - zmin))[:, None]
        e32 = U32 * grad_scale * ((4 * red(C) + 12) * (p + R["oh"]) + p * arg)
        e32 = torch.where(valid[:, None], e32, torch.zeros_like(e32))
        bound = torch.where(valid[:, None], _bf16_bound(R["d"], e32), torch.zeros_like(e32))   # ignored rows: exact 0
        worst = max(worst, _bounded(variant, "dlogits", dlogits, R["d"], bound))
        if dbias is not None:
            own = _c64(dlogits)[valid]
            worst = max(worst, _bounded(variant, "dbias", dbias, own.sum(0) + dbias0,
                                        (n + 9) * U32 * (own.abs().sum(0) + abs(dbias0)) + TINY))
    if metrics is not None:
        m = metrics.detach().cpu().double()
        m0 = torch.tensor(metrics0, dtype=torch.float64)
        if row_loss is not None:
            add, slack = _c64(row_loss)[valid], 0.0
        else:
            add, slack = R["loss"][valid], float(row_tol[valid].sum())
        worst = max(worst, _bounded(variant, "metrics_loss", m[0], add.sum() + m0[0],
                                    (n + 9) * U32 * (add.abs().sum() + m0[0].abs()) + slack + TINY))
        want = torch.tensor([n, int(R["correct"].sum()), n], dtype=torch.float64) + m0[1:]
        worst = max(worst, _exact(variant, "metrics_counts", m[1:], want))
    return worst


# ----------------------------------------------------------------------------- attention row softmax, colsum
def softmax_visible(rows: int, Sq: int, Sk: int, causal: bool) -> torch.Tensor:
    """[rows, Sk] bool: key k is visible to row r (query r % Sq sees keys [0, q + 1 + Sk - Sq))."""
    q = torch.arange(rows) % Sq
    lim = torch.clamp(q + 1 + (Sk - Sq), max=Sk) if causal else torch.full((rows,), Sk)
    return torch.arange(Sk)[None, :] < lim[:, None]


def check_softmax_fwd(S, P, Sq: int, causal: bool, variant: str = "attn_softmax_fwd") -> float:
    """attn_softmax_fwd_kernel: P = bf16(exp(s - mx) / sum exp(s - mx)) over the visible keys, 0 elsewhere.
    A = p.  n_ops = red(Sk) + 16: s - mx, the 2-ulp exp, the sum (red(Sk) deep, each term with those
    roundings), 1 / sum (<= 2 ulp), the product.  The fast exponential's argument error, relative to
    p: its own 2 |s - mx|, and inside the sum at most 2 (max s - min s) over the visible keys.
    Masked columns are exact zeros."""
    Sc = _c64(S)
    rows, Sk = Sc.shape
    vis = softmax_visible(rows, Sq, Sk, causal)
    zm = torch.where(vis, Sc, torch.full_like(Sc, float("-inf")))
    mx = zm.max(-1, keepdim=True).values
    p = torch.where(vis, torch.exp(zm - mx), torch.zeros_like(Sc))
    p = p / p.sum(-1, keepdim=True)
    rng = mx - torch.where(vis, Sc, torch.full_like(Sc, float("inf"))).min(-1, keepdim=True).values
    e32 = U32 * p * ((red(Sk) + 16) + 2 * torch.where(vis, (Sc - mx).abs(), torch.zeros_like(Sc)) + 2 * rng)
    bound = torch.where(vis, _bf16_bound(p, e32), torch.zeros_like(p))
    return _bounded(variant, "P", P, p, bound)


def check_softmax_bwd(P, dP, dS, variant: str = "attn_softmax_bwd") -> float:
    """attn_softmax_bwd_kernel: dS = bf16(P (dP - sum_k P dP)) from the bf16 P and fp32 dP it read.
    A = |P| (|dP| + sum|P dP|); n_ops = red(Sk) + 8: the products (1), the reduction (red(Sk)), the
    subtraction and the final product."""
    Pc, D = _c64(P), _c64(dP)
    Sk = Pc.shape[1]
    dot = (Pc * D).sum(-1, keepdim=True)
    ref = Pc * (D - dot)
    A = Pc.abs() * (D.abs() + (Pc * D).abs().sum(-1, keepdim=True))
    return _bounded(variant, "dS", dS, ref, _bf16_bound(ref, U32 * (red(Sk) + 8) * A))


def check_colsum(x, out, out0=0.0, variant: str = "colsum") -> float:
    """colsum_kernel: out += sum over the M rows of bf16 x (registers, LDS, one atomic per workgroup)."""
    X = _c64(x)
    M = X.shape[0]
    return _bounded(variant, "colsum", out, X.sum(0) + out0, (M + 9) * U32 * (X.abs().sum(0) + abs(out0)) + TINY)


# ----------------------------------------------------------------------------- shared inputs and test bodies
def _gen(*key) -> torch.Generator:
    seed = 0
    for k in key:
        seed = (seed * 1000003 + int(k) + 1) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(seed)


def _is_gpu(dev) -> bool:
    return torch.device(dev).type == "cuda"


def _lib():
    from jax_distributed_tuts_amd.ops import _lib as L

    return L.lib()


def ln_inputs(T: int, d: int, integer_dy: bool = False):
    """x: Gaussian rows (scale 2, offset 0.7); from T >= 3 on, row 1 and the last row sit at 300 +- 1
    (a large row offset: x - mean cancels) and row 2 is constant (variance 0)."""
    g = _gen(1, T, d)
    x = torch.randn(T, d, generator=g) * 2 + 0.7
    if T >= 3:
        x[1] = 300 + torch.randn(d, generator=g)
        x[T - 1] = 300 + torch.randn(d, generator=g)
        x[2] = 1.5
    gamma = 1 + 0.3 * torch.randn(d, generator=g)
    beta = 0.3 * torch.randn(d, generator=g)
    # dy with a row mean and a component along x - mean, so that neither s1 nor s2 is small by chance
    up = (x > x.mean(-1, keepdim=True)).float()
    if integer_dy:
        dy = torch.randint(-2, 3, (T, d), generator=g).float() + up
    else:
        dy = torch.randn(T, d, generator=g) + 0.5 + (up - 0.5)
    dres = torch.randn(T, d, generator=g)
    return x.to(torch.bfloat16), gamma, beta, dy.to(torch.bfloat16), dres.to(torch.bfloat16)


def body_ln_fwd(dev, T: int, d: int, variant: str) -> float:
    x, gamma, beta, _, _ = ln_inputs(T, d)
    y, mean, rstd = kern.layernorm_fwd(x.to(dev), gamma.to(dev), beta.to(dev))
    return check_ln_fwd(x, gamma, beta, y, mean, rstd, variant=variant)


def body_ln_embed(dev, T: int, S: int, d: int, variant: str) -> float:
    g = _gen(2, T, S, d)
    V = 50
    wte = torch.randn(V, d, generator=g).to(torch.bfloat16)
    wpe = torch.randn(S, d, generator=g).to(torch.bfloat16)
    tok = torch.randint(0, V, (T,), generator=g).to(torch.int32)
    gamma, beta = 1 + 0.3 * torch.randn(d, generator=g), 0.3 * torch.randn(d, generator=g)
    x = torch.full((T, d), 7.0, dtype=torch.bfloat16, device=dev)
    y, mean, rstd = kern.layernorm_fwd(x, gamma.to(dev), beta.to(dev), embed=(tok.to(dev), wte.to(dev), wpe.to(dev), S))
    worst = check_embed_bits(tok, wte, wpe, S, x, variant=variant)
    return max(worst, check_ln_fwd(x, gamma, beta, y, mean, rstd, variant=variant))


def body_ln_bwd(dev, T: int, d: int, variant: str, with_dres: bool = True, with_dsum: bool = True,
                integer_dy: bool = False) -> float:
    """mean / rstd come from the fp32 torch forward: the backward is checked against what it is given."""
    x, gamma, beta, dy, dres = ln_inputs(T, d, integer_dy)
    _, mean, rstd = kern.layernorm_fwd(x, gamma, beta)
    dg0, db0, ds0 = 0.75, -1.25, 0.5   # the column sums accumulate on top of what is there
    dg, db = torch.full((d,), dg0, device=dev), torch.full((d,), db0, device=dev)
    ds = torch.full((d,), ds0, device=dev) if with_dsum else None
    dx = kern.layernorm_bwd(dy.to(dev), x.to(dev), mean.to(dev), rstd.to(dev), gamma.to(dev), dg, db,
                            dres=dres.to(dev) if with_dres else None, dsum=ds)
    return check_ln_bwd(dy, x, mean, rstd, gamma, dx, dres=dres if with_dres else None, dgamma=dg, dbeta=db, dsum=ds,
                        dgamma0=dg0, dbeta0=db0, dsum0=ds0, exact_dbeta=integer_dy, variant=variant)


# two tie_lower rows for every tie_higher one: a kernel that resolves ties the other way miscounts one
# row up and one down per pair, which would cancel in the `correct` count
XENT_KINDS = ("tie_lower", "ignore_neg", "tie_lower", "tie_higher", "ignore_C", "first", "last", "ignore_C5",
              "last_chunk", "random")
TIE = 14.0   # above every Gaussian logit (3 sigma = 3 -> |z| < 14), exact in bf16


def xent_inputs(M: int, C: int, dt, neg_inf: bool = False):
    """Gaussian logits (sigma 3) and one label kind per row, cycling through XENT_KINDS: a label tied
    for the row maximum with a lower index (counts as incorrect) / a higher index (correct), ignored
    labels -1, C and C + 5, the first and last class, a class inside the last 8-wide chunk.
    ``neg_inf``: every row also gets -inf logits away from its label, columns 0..2 (a lane's first
    logit) and a later stretch."""
    g = _gen(3, M, C)
    z = (torch.randn(M, C, generator=g) * 3).clamp(-13, 13)
    y = torch.randint(0, C, (M,), generator=g)
    for r in range(M):
        kind = XENT_KINDS[r % len(XENT_KINDS)]
        if kind == "tie_lower":
            y[r] = max(1, int(y[r]))
            z[r, int(y[r])] = z[r, int(y[r]) // 2] = TIE
        elif kind == "tie_higher":
            y[r] = min(C - 2, int(y[r]))
            z[r, int(y[r])] = z[r, (int(y[r]) + C) // 2] = TIE
            if (int(y[r]) + C) // 2 == int(y[r]):
                z[r, C - 1] = TIE
        elif kind == "ignore_neg":
            y[r] = -1
        elif kind == "ignore_C":
            y[r] = C
        elif kind == "ignore_C5":
            y[r] = C + 5
        elif kind == "first":
            y[r] = 0
        elif kind == "last":
            y[r] = C - 1
        elif kind == "last_chunk":
            y[r] = C - 3
    if neg_inf:
        for r in range(M):
            lab = int(y[r])
            cols = [c for c in list(range(0, min(3, C))) + list(range(C // 2, min(C, C // 2 + 70))) if c != lab]
            z[r, cols] = float("-inf")
    return z.to(dt), y.to(torch.int32)


def xent_buffers(dev, z, layout: str):
    """(logits view, dlogits view, dlogits backing buffer) on ``dev``.  contig; slice8: columns [8, 8 + C)
    of buffers C + 16 wide (ld % 8 == 0, 16-byte aligned); slice_odd: columns [0, C) of C + 3 wide
    buffers (ld % 8 != 0); misaligned: a contiguous dlogits one element (2 bytes) into its buffer."""
    M, C = z.shape
    if layout == "contig":
        back = torch.full((M, C), 7.0, dtype=torch.bfloat16, device=dev)
        return z.to(dev), back, back
    if layout == "misaligned":
        back = torch.full((M * C + 8,), 7.0, dtype=torch.bfloat16, device=dev)
        return z.to(dev), back[1:1 + M * C].view(M, C), back
    off, ld = (8, C + 16) if layout == "slice8" else (0, C + 3)
    zb = torch.full((M, ld), 5.0, dtype=z.dtype, device=dev)
    zb[:, off:off + C] = z.to(dev)
    back = torch.full((M, ld), 7.0, dtype=torch.bfloat16, device=dev)
    return zb[:, off:off + C], back[:, off:off + C], back


def xent_expected_variant(C: int, dt, layout: str) -> int:
    """The kernel each case claims: 0 = narrow, else the wide kernel's NV."""
    if dt != torch.bfloat16 or C < 256 or C > 2048 or C % 8 or layout in ("slice_odd", "misaligned"):
        return 0
    return 1 if C <= 512 else (2 if C <= 1024 else 4)


def body_xent(dev, M: int, C: int, dt, variant: str, layout: str = "contig", with_dlogits: bool = True,
              slab: bool = False, neg_inf: bool = False, expect: Optional[int] = None) -> float:
    z, y = xent_inputs(M, C, dt, neg_inf)
    gs = float(torch.tensor(1.0 / M, dtype=torch.float32))   # the fp32 value the launcher receives
    zv, dv, back = xent_buffers(dev, z, layout)
    if not with_dlogits:
        dv = None
    if expect is not None and _is_gpu(dev):
        got = _lib().jdt_xent_variant(zv.data_ptr(), int(dt == torch.float32), zv.stride(0), C,
                                      dv.data_ptr() if dv is not None else 0, dv.stride(0) if dv is not None else 0)
        assert got == expect, f"case claims kernel variant {expect}, the launcher takes {got}"
    db0, m0 = 0.5, (3.0, 2.0, 1.0, 2.0)
    dbias = torch.full((C,), db0, device=dev) if with_dlogits else None
    metrics = torch.tensor(m0, device=dev)
    row_loss = torch.full((M,), 9.0, device=dev)
    mslab = torch.zeros(256, 4, device=dev) if slab else None
    kern.softmax_xent(zv, y.to(dev), grad_scale=gs, dlogits=dv, dbias=dbias, metrics=metrics, row_loss=row_loss,
                      mslab=mslab)
    if slab:
        # the per-workgroup rows hold (loss, n, correct, 0) partial sums; the fold adds slot and slab
        # into the running totals and zeroes both
        assert float(mslab[:, 3].abs().sum()) == 0.0
        if _is_gpu(dev) and expect:
            assert float(metrics.cpu().sub(torch.tensor(m0)).abs().sum()) == 0.0, "the slab route touched the slot"
            assert float(mslab[:, 1].max()) <= 16.0   # at most 4 waves x rpw <= 4 rows per workgroup
        running = torch.tensor((10.0, 20.0, 30.0, 20.0), device=dev)
        kern.metrics_fold_(running, metrics, slab=mslab)
        assert float(mslab.abs().sum()) == 0.0 and float(metrics.abs().sum()) == 0.0
        metrics, m0 = running, tuple(a + b for a, b in zip(m0, (10.0, 20.0, 30.0, 20.0)))
    worst = check_xent(z, y, gs, dlogits=dv, dbias=dbias, metrics=metrics, row_loss=row_loss, dbias0=db0, metrics0=m0,
                       variant=variant)
    if with_dlogits and layout != "contig":   # nothing outside the view was written
        keep = torch.ones(back.shape, dtype=torch.bool)
        if layout == "misaligned":
            keep[1:1 + M * C] = False
        else:
            off = 8 if layout == "slice8" else 0
            keep[:, off:off + C] = False
        assert bool((back.cpu()[keep] == 7.0).all()), "dlogits written outside its view"
    return worst


def row_softmax_fwd(S: torch.Tensor, Sq: int, causal: bool) -> torch.Tensor:
    """GPU: jdt_attn_softmax_fwd.  CPU: the same formula in fp32 torch, rounded to bf16."""
    rows, Sk = S.shape
    if _is_gpu(S.device):
        from jax_distributed_tuts_amd.ops import _lib as L

        P = torch.full((rows, Sk), 7.0, dtype=torch.bfloat16, device=S.device)
        L.check(L.lib().jdt_attn_softmax_fwd(S.data_ptr(), P.data_ptr(), rows, Sq, Sk, int(causal), L.stream_ptr()),
                "jdt_attn_softmax_fwd")
        return P
    vis = softmax_visible(rows, Sq, Sk, causal)
    return torch.softmax(torch.where(vis, S, torch.full_like(S, float("-inf"))), -1).to(torch.bfloat16)


def row_softmax_bwd(P: torch.Tensor, dP: torch.Tensor) -> torch.Tensor:
    rows, Sk = P.shape
    if _is_gpu(P.device):
        from jax_distributed_tuts_amd.ops import _lib as L

        dS = torch.full((rows, Sk), 7.0, dtype=torch.bfloat16, device=P.device)
        L.check(L.lib().jdt_attn_softmax_bwd(P.data_ptr(), dP.data_ptr(), dS.data_ptr(), rows, Sk, L.stream_ptr()),
                "jdt_attn_softmax_bwd")
        return dS
    p = P.float()
    return (p * (dP - (p * dP).sum(-1, keepdim=True))).to(torch.bfloat16)


def softmax_inputs(Sk: int, causal: bool):
    """Two heads of Sq = Sk rows of fp32 scores; the last visible key of the middle and the last row of
    each head dominates (+30)."""
    g = _gen(4, Sk, causal)
    rows = 2 * Sk
    S = torch.randn(rows, Sk, generator=g) * 2
    for r in range(rows):
        q = r % Sk
        if q in (Sk // 2, Sk - 1):
            S[r, q if causal else Sk - 1] += 30.0
    dP = torch.randn(rows, Sk, generator=g)
    return S, dP


def body_softmax(dev, Sk: int, causal: bool, variant: str) -> float:
    S, dP = softmax_inputs(Sk, causal)
    P = row_softmax_fwd(S.to(dev), Sk, causal)
    worst = check_softmax_fwd(S, P, Sk, causal, variant=variant + "_fwd")
    dS = row_softmax_bwd(P, dP.to(dev))
    return max(worst, check_softmax_bwd(P, dP, dS, variant=variant + "_bwd"))


def body_colsum(dev, M: int, N: int, variant: str) -> float:
    g = _gen(5, M, N)
    wide = torch.randn(M, N + 24, generator=g).to(torch.bfloat16)
    x = wide.to(dev)[:, 8:8 + N]   # ld = N + 24 (% 8 == 0), 16-byte aligned
    out = torch.full((N,), 0.5, device=dev)
    kern.colsum_(x, out)
    return check_colsum(wide[:, 8:8 + N], out, out0=0.5, variant=variant)


# ----------------------------------------------------------------------------- shapes (dispatch edges, not workload sizes)
# LayerNorm widths: NV = 1, 2 and 4 chunks of 512 columns, full and partial last chunk; 1032 and 1544
# have 3 chunks and take the NV = 4 kernels.  Rows: 1, and grids of 8 (XCD remap) and 10 (none, ragged)
LN_D = (8, 72, 512, 520, 1024, 1032, 1544, 2048)
LN_T = (1, 30, 37)
LN_EMBED = ((37, 5, 8), (30, 7, 520), (37, 16, 1544), (9, 4, 2048))   # (T, S, d): S never divides T
LN_BWD_RW = ((1, 4), (2, 4), (4, 4), (8, 4), (1, 8), (2, 8), (4, 8), (1, 16), (2, 16))


def ln_bwd_cases():
    """(NV, R, W, d, T) for every ln_bwd_kernel instantiation: T = 8 W R - 1 (grid 8, the last
    workgroup one row short) and 9 W R + 1 (grid 10: no remap, one row in the last workgroup)."""
    out = []
    for nv, d in ((1, 72), (2, 520)):
        out += [(nv, r, w, d, t) for r, w in LN_BWD_RW for t in (8 * w * r - 1, 9 * w * r + 1)]
    out += [(4, r, 4, d, t) for r, d in ((1, 1032), (2, 2048)) for t in (8 * 4 * r - 1, 9 * 4 * r + 1)]
    return out


LN_BWD_OPTIONAL = (8, 1024, 1544)   # widths of the optional-argument cases (T = 37)
# classes: narrow; wide NV = 1, 2, 4, each full and partial; narrow again above 2048 and at C % 8 != 0
XENT_C = (10, 63, 64, 65, 255, 256, 264, 512, 520, 1001, 1024, 1032, 2048, 2056)
XENT_M = (1, 5, 31, 33)
XENT_RPW = (1, 2, 4)
XENT_RPW_C = (264, 520, 1544)   # NV = 1, 2 and 4, each with a partial last chunk


def xent_rpw_rows(rpw: int):
    """M of the rows-per-wave cases: 32 rpw - 1 gives a grid of 8 (block remap), 36 rpw + 1 a grid of
    10 with a ragged last wave."""
    return XENT_M + (32 * rpw - 1, 36 * rpw + 1)


XENT_LAYOUTS = ((512, torch.bfloat16, "slice8"), (1032, torch.bfloat16, "slice8"), (264, torch.float32, "slice8"),
                (512, torch.bfloat16, "slice_odd"), (1032, torch.bfloat16, "slice_odd"),
                (512, torch.bfloat16, "misaligned"), (2048, torch.bfloat16, "misaligned"))
XENT_NEG_INF = ((10, torch.float32), (70, torch.bfloat16), (200, torch.float32), (520, torch.bfloat16),
                (2056, torch.bfloat16))
SOFTMAX_SK = (1, 63, 64, 65, 200)
COLSUM_MN = tuple((m, n) for m in (1, 31, 33) for n in (8, 520, 1032))


# ----------------------------------------------------------------------------- log summary
def summarize(path: str) -> str:
    """One row per (variant/output): the worst ratio over the log and the number of checks."""
    worst: dict = {}
    with open(path) as f:
        for line in f:
            rec = json.loads(line)
            if "ratio" not in rec or rec["name"].startswith("mutant/"):   # rejection tests, tests/test_row_kernels.py
                continue
            w, n = worst.get(rec["name"], (0.0, 0))
            worst[rec["name"]] = (max(w, rec["ratio"]), n + 1)
    width = max(len(k) for k in worst)
    rows = [f"{'kernel variant / output':<{width}}  worst err/bound  checks"]
    rows += [f"{k:<{width}}  {w:15.4f}  {n:6d}" for k, (w, n) in sorted(worst.items())]
    return "\n".join(rows)


if __name__ == "__main__":
    print(summarize(sys.argv[1]))
