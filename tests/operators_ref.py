"""The yardstick of the sparse-operator tests (include/enf_hip.h, "Sparse linear observations"), in fp64, on the DENSE operator:

    obs[b,m,o]   = sum_n A[m,n] out[b,n,o]
    loss         = 1/(B M O) sum_{b,m,o} w (obs - target)^2              w == 0 is a select: that target is never used
    d out[b,n,o] = grad_scale 2/(B M O) sum_m A[m,n] (w (obs - target))[b,m,o]
    err_a[b,m]   = sum_o w (obs - target)^2            loss_b[b] = sum_m err_a[b,m] / (M O)

``dense_loss`` works on a decode that exists (numpy einsum); ``operator_loss`` decodes with the oracle and takes d loss / d(p, a, sigma)
times grad_scale by its autograd, as tests/cells_ref.py does; ``fit_loop`` is fit_linear_observations written on it.  Cases are seeded
here, computed once per process and never modified."""
from types import SimpleNamespace as NS

import numpy as np
import torch

from oracle import enf_ref_np as R
from oracle import enf_ref_torch as T
from tests.cells_ref import B, Z, f32, rel      # noqa: F401  (re-exported: one batch shape and one error measure for both yardsticks)
from tests.gn_ref import sgd_rule
from tests.helpers import make_cfg, make_inputs

_CASES = {}


def _weights(w, shape):
    """w None, (B, M) or (B, M, O) -> (B, M, O) fp64"""
    if w is None:
        return np.ones(shape)
    w = np.asarray(w, dtype=np.float64)
    return np.broadcast_to(w[..., None] if w.ndim == 2 else w, shape).copy()


def dense_loss(A, out, target, w=None, grad_scale=1.0):
    """NS(obs, r = w dd, dd = the selected residual, dout, err_a, loss_b, loss) of a decode ``out`` (B, N, O) in fp64 numpy."""
    A, out = np.asarray(A, dtype=np.float64), np.asarray(out, dtype=np.float64)
    obs = np.einsum("mn,bno->bmo", A, out)
    Bn, M, O = obs.shape
    wt = _weights(w, obs.shape)
    live = wt > 0
    dd = np.where(live, obs - np.where(live, np.asarray(target, dtype=np.float64), 0.0), 0.0)
    r = wt * dd
    err_a = (r * dd).sum(-1)
    loss_b = err_a.sum(1) / (M * O)
    dout = grad_scale * 2.0 / (Bn * M * O) * np.einsum("mn,bmo->bno", A, r)
    return NS(obs=obs, r=r, dd=dd, dout=dout, err_a=err_a, loss_b=loss_b, loss=float(loss_b.sum() / Bn))


def operator_loss(cfg, prm, x, p, a, s, A, target, w=None, grad_scale=1.0, grads=True):
    """NS(obs, dd, err_a, loss_b, loss, g = (gp, ga, gs) or None, out) in fp64: the oracle's decode, the dense operator, autograd."""
    tp = T.to_torch(prm, torch.float64)
    leaves = tuple(torch.tensor(np.asarray(u, dtype=np.float64), requires_grad=grads) for u in (p, a, s))
    out = T.nef_apply(tp, cfg, torch.tensor(np.asarray(x, dtype=np.float64)), *leaves)
    At = torch.tensor(np.asarray(A, dtype=np.float64))
    obs = torch.einsum("mn,bno->bmo", At, out)
    Bn, M, On = obs.shape
    wt = torch.tensor(_weights(w, tuple(obs.shape)))
    live = wt > 0
    tgt = torch.where(live, torch.tensor(np.asarray(target, dtype=np.float64)), torch.zeros_like(obs))
    dd = torch.where(live, obs - tgt, torch.zeros_like(obs))
    err_a = (wt * dd * dd).sum(-1)
    loss_b = err_a.sum(1) / (M * On)
    loss = loss_b.sum() / Bn
    g = None
    if grads:
        g = torch.autograd.grad(loss * grad_scale, leaves, allow_unused=True)
        g = tuple((torch.zeros_like(u) if gi is None else gi).numpy() for u, gi in zip(leaves, g))
    return NS(obs=obs.detach().numpy(), dd=dd.detach().numpy(), err_a=err_a.detach().numpy(), loss_b=loss_b.detach().numpy(),
              loss=float(loss.detach()), g=g, out=out.detach().numpy())


def ragged_entries(lengths, N, seed, unsorted=True, spare=0):
    """(rows, cols, vals) of an operator with the given row lengths on N columns: every row draws its columns without repetition from
    the first N - spare columns (so rows overlap, and the last `spare` columns are in no row), in random -- unsorted -- order; factors of
    both signs in [-1.5, -0.2] u [0.2, 1.5], scaled by 1 / sqrt(length), rounded to fp32."""
    rng = np.random.default_rng(seed)
    rows, cols, vals = [], [], []
    for m, n in enumerate(lengths):
        c = rng.permutation(N - spare)[:n] if n <= N - spare else rng.integers(0, N - spare, n)      # (a longer row repeats columns)
        if not unsorted:
            c = np.sort(c)
        rows += [m] * len(c)
        cols += c.tolist()
        vals += (rng.uniform(0.2, 1.5, len(c)) * rng.choice([-1.0, 1.0], len(c)) / np.sqrt(max(len(c), 1))).tolist()
    return np.asarray(rows, dtype=np.int64), np.asarray(cols, dtype=np.int64), f32(vals)


def case(inv, lengths, N, D=64, H=2, seed=171, O=2, weights="obs", Bn=B, Zn=Z, spare=3):
    """One problem and its reference: Bn signals, Zn latents, O channels, N points per signal (x per signal), a ragged operator with the
    given row lengths, random targets (residuals are O(1)); weights "obs": w (B, M) with about a third exact zeros, "value": (B, M, O)
    alike, None: none.  `poisoned` puts NaN / Inf under every zero weight."""
    key = (inv, tuple(lengths), N, D, H, seed, O, weights, Bn, Zn, spare)
    if key not in _CASES:
        cfg = make_cfg(inv, D=D, H=H, C=12, O=O, freq=(0.3, 0.6))
        prm = R.init_params(seed, cfg, jitter=0.1)
        x, p, a, s = (f32(v) for v in make_inputs(cfg, Bn, N, Zn, seed + 1))
        rng = np.random.default_rng(seed + 2)
        M = len(lengths)
        rows, cols, vals = ragged_entries(lengths, N, seed + 3, spare=spare)
        A = np.zeros((M, N))
        np.add.at(A, (rows, cols), vals)
        y = f32(rng.standard_normal((Bn, M, O)))
        w = None
        if weights is not None:
            shape = (Bn, M) if weights == "obs" else (Bn, M, O)
            w = f32(rng.uniform(0.2, 2.0, shape))
            w[rng.uniform(size=shape) < 0.3] = 0.0
            w[(1, 0) if weights == "obs" else (1, 0, 0)] = 0.0
        gs = float(Bn)
        ref = operator_loss(cfg, prm, x, p, a, s, A, y, w, gs)
        _CASES[key] = NS(cfg=cfg, prm=prm, x=x, p=p, a=a, s=s, rows=rows, cols=cols, vals=vals, A=A, y=y, w=w, N=N, M=M, O=O, gs=gs, ref=ref,
                         B=Bn, Z=Zn, weights=weights)
    return _CASES[key]


def poisoned(y, w):
    """the targets with NaN / +-Inf under every zero weight (w (B, M) or (B, M, O))"""
    y = np.array(y, dtype=np.float64)
    gone = np.broadcast_to((np.asarray(w) == 0)[..., None] if np.asarray(w).ndim == 2 else np.asarray(w) == 0, y.shape)
    bad = np.array([np.nan, np.inf, -np.inf])
    y[gone] = bad[np.arange(int(gone.sum())) % 3]
    return y


def fit_loop(cfg, prm, x, A, targets, w, lat0, lrs, steps):
    """fit_linear_observations in fp64 on shared points x (N, dx): (losses (steps + 1,), latents).  lat0 = (p, a, s) with leading
    dimension 1; lrs = (lr_p, lr_a (C,)); the window does not move.  The gradient of the batch-mean loss times B, as inner_loop."""
    Bn = targets.shape[0]
    p, a, s = (np.repeat(np.asarray(u, dtype=np.float64), Bn, 0) for u in lat0)
    xb = np.repeat(x[None], Bn, 0)

    def loss(cur, grads):
        r = operator_loss(cfg, prm, xb, *cur, A, targets, w, float(Bn), grads=grads)
        return r.loss, r.g
    losses, lat = sgd_rule(loss, p, a, s, steps, lrs[0], lrs[1])           # (tests/gn_ref.py: the one copy of the rule)
    return np.array(losses), tuple(lat)
