"""The yardstick of the grouped-observation tests (include/enf_hip.h, "Grouped observations"), on the oracle in fp64:

    obs[b,m,o] = sum_{k<G} q[b, mG+k] out[b, mG+k, o]
    loss       = 1/(B M O) sum_{b,m} w[b,m] sum_o (obs - target)^2            w == 0 is a select: that target is never used
    err_g[b,m] = w[b,m] sum_o (obs - target)^2            loss_b[b] = sum_m err_g[b,m] / (M O)

and d loss / d(p, a, sigma) times grad_scale by autograd, plus the meta-SGD loop of fitting/cells.py: fit_cell_averages written on it.
Cases are seeded here, computed once per process and never modified."""
from types import SimpleNamespace as NS

import numpy as np
import torch

from oracle import enf_ref_np as R
from oracle import enf_ref_torch as T
from tests.gn_ref import sgd_rule
from tests.helpers import make_cfg, make_inputs

B, Z = 3, 7
_CASES = {}


def f32(v):
    """rounded to fp32 and back: the oracle sees the numbers the kernels get"""
    return np.asarray(v, dtype=np.float32).astype(np.float64)


def rel(u, v):
    u, v = np.asarray(u, dtype=np.float64), np.asarray(v, dtype=np.float64)
    return float(np.linalg.norm(u - v) / np.linalg.norm(v))


def cell_loss(cfg, prm, x, p, a, s, target, G, q=None, w=None, grad_scale=1.0, grads=True):
    """NS(obs (B, M, O), dd = the selected residual, err_g (B, M), loss_b (B,), loss, g = (gp, ga, gs) or None, out_max = max |out|) in
    fp64 numpy.  q None: 1 / G; w None: 1."""
    tp = T.to_torch(prm, torch.float64)
    leaves = tuple(torch.tensor(np.asarray(u, dtype=np.float64), requires_grad=grads) for u in (p, a, s))
    out = T.nef_apply(tp, cfg, torch.tensor(np.asarray(x, dtype=np.float64)), *leaves)
    Bn, N, On = out.shape
    M = N // G
    assert M * G == N
    qt = torch.full((Bn, N), 1.0 / G, dtype=torch.float64) if q is None else torch.tensor(np.asarray(q, dtype=np.float64))
    wt = torch.ones((Bn, M), dtype=torch.float64) if w is None else torch.tensor(np.asarray(w, dtype=np.float64))
    obs = (qt[..., None] * out).reshape(Bn, M, G, On).sum(2)
    live = (wt > 0)[..., None]
    tgt = torch.where(live, torch.tensor(np.asarray(target, dtype=np.float64)), torch.zeros_like(obs))     # the select
    dd = torch.where(live, obs - tgt, torch.zeros_like(obs))
    err_g = wt * (dd * dd).sum(-1)
    loss_b = err_g.sum(1) / (M * On)
    loss = loss_b.sum() / Bn
    g = None
    if grads:
        g = torch.autograd.grad(loss * grad_scale, leaves, allow_unused=True)
        g = tuple((torch.zeros_like(u) if gi is None else gi).numpy() for u, gi in zip(leaves, g))
    return NS(obs=obs.detach().numpy(), dd=dd.detach().numpy(), err_g=err_g.detach().numpy(), loss_b=loss_b.detach().numpy(), loss=float(loss.detach()),
              g=g, out_max=float(out.detach().abs().max()))


def case(inv, G, N, D=64, H=2, seed=71, O=2):
    """One problem and its reference: B = 3 signals, Z = 7 latents, O channels, N = M G points per signal; random q > 0, random
    targets (residuals are O(1)), w with about a third exact zeros.  `target` is clean; `poisoned(kind)` puts NaN / Inf under w == 0."""
    key = (inv, G, N, D, H, seed, O)
    if key not in _CASES:
        cfg = make_cfg(inv, D=D, H=H, C=12, O=O, freq=(0.3, 0.6))
        prm = R.init_params(seed, cfg, jitter=0.1)
        x, p, a, s = (f32(v) for v in make_inputs(cfg, B, N, Z, seed + 1))
        rng = np.random.default_rng(seed + 2)
        M = N // G
        q = f32(rng.uniform(0.2, 2.0, (B, N)) / G)
        y = f32(rng.standard_normal((B, M, O)))
        w = f32(rng.uniform(0.2, 2.0, (B, M)))
        w[rng.uniform(size=(B, M)) < 0.3] = 0.0
        w[1, 0] = 0.0
        gs = float(B)
        ref = cell_loss(cfg, prm, x, p, a, s, y, G, q, w, gs)
        _CASES[key] = NS(cfg=cfg, prm=prm, x=x, p=p, a=a, s=s, q=q, y=y, w=w, G=G, N=N, M=M, O=O, gs=gs, ref=ref)
    return _CASES[key]


def poisoned(c, kind="mixed"):
    """the targets with NaN / +-Inf ("mixed") or +Inf only ("inf") under every zero weight"""
    y = c.y.copy()
    gone = c.w == 0
    vals = np.array([np.nan, np.inf, -np.inf]) if kind == "mixed" else np.array([np.inf])
    y[gone] = vals[np.arange(int(gone.sum())) % len(vals)][:, None]
    return y


def fit_loop(cfg, prm, x, q, G, targets, w, lat0, lrs, steps):
    """fit_cell_averages in fp64 on shared cells x (N, dx), q (N,): (losses (steps + 1,), latents).  lat0 = (p, a, s) with leading
    dimension 1; lrs = (lr_p, lr_a (C,)); the window does not move.  The gradient of the batch-mean loss times B, as inner_loop."""
    Bn = targets.shape[0]
    p, a, s = (np.repeat(np.asarray(u, dtype=np.float64), Bn, 0) for u in lat0)
    xb, qb = np.repeat(x[None], Bn, 0), np.repeat(q[None], Bn, 0)

    def loss(cur, grads):
        r = cell_loss(cfg, prm, xb, *cur, targets, G, qb, w, float(Bn), grads=grads)
        return r.loss, r.g
    losses, lat = sgd_rule(loss, p, a, s, steps, lrs[0], lrs[1])           # (tests/gn_ref.py: the one copy of the rule)
    return np.array(losses), tuple(lat)
