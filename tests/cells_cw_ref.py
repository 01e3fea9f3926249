"""The yardstick of the per-value weights on grouped observations (include/enf_hip.h, "Grouped observations": the _gc calls), on the
oracle in fp64 -- tests/cells_ref.cell_loss with w (B, M, O) and the select per VALUE:

    loss       = 1/(B M O) sum_{b,m,o} cw[b,m,o] (obs - target)^2             cw == 0 is a select: that target is never used
    d out[b, mG+k, o] = 2 q[b,mG+k] cw[b,m,o] (obs - target) / (B M O) * grad_scale
    err_g[b,m] = sum_o cw[b,m,o] (obs - target)^2          loss_b[b] = sum_m err_g[b,m] / (M O)

Cases are seeded here, computed once per process and never modified."""
from types import SimpleNamespace as NS

import numpy as np
import torch

from oracle import enf_ref_torch as T
from tests import cells_ref as CR
from tests.cells_ref import B, Z, f32

_CASES = {}


def group_loss(out, target, G, q=None, cw=None, grad_scale=1.0):
    """The definitions above on a decode ``out`` (B, N, O) that exists, fp64 torch: NS(obs, dd = the selected residual, err_g, loss_b,
    loss (a tensor: differentiable w.r.t. out), dout = d (loss grad_scale) / d out in closed form).  q None: 1 / G; cw None: 1."""
    Bn, N, On = out.shape
    M = N // G
    assert M * G == N
    qt = torch.full((Bn, N), 1.0 / G, dtype=torch.float64) if q is None else torch.as_tensor(np.asarray(q, dtype=np.float64))
    wt = torch.ones((Bn, M, On), dtype=torch.float64) if cw is None else torch.as_tensor(np.asarray(cw, dtype=np.float64))
    assert tuple(wt.shape) == (Bn, M, On)
    obs = (qt[..., None] * out).reshape(Bn, M, G, On).sum(2)
    live = wt > 0
    tgt = torch.where(live, torch.as_tensor(np.asarray(target, dtype=np.float64)), torch.zeros_like(obs))     # the select, per value
    dd = torch.where(live, obs - tgt, torch.zeros_like(obs))
    err_g = (wt * dd * dd).sum(-1)
    loss_b = err_g.sum(1) / (M * On)
    loss = loss_b.sum() / Bn
    dout = qt[..., None] * (2.0 * wt * dd.detach() / (Bn * M * On) * grad_scale).repeat_interleave(G, dim=1)
    return NS(obs=obs, dd=dd, err_g=err_g, loss_b=loss_b, loss=loss, dout=dout)


def cell_loss(cfg, prm, x, p, a, s, target, G, q=None, w=None, grad_scale=1.0, grads=True):
    """tests/cells_ref.cell_loss with w (B, M, O): NS(obs, dd, err_g (B, M), loss_b (B,), loss, g = (gp, ga, gs) or None, out_max, dout
    (B, N, O)) in fp64 numpy."""
    tp = T.to_torch(prm, torch.float64)
    leaves = tuple(torch.tensor(np.asarray(u, dtype=np.float64), requires_grad=grads) for u in (p, a, s))
    out = T.nef_apply(tp, cfg, torch.tensor(np.asarray(x, dtype=np.float64)), *leaves)
    r = group_loss(out, target, G, q, w, grad_scale)
    g = None
    if grads:
        g = torch.autograd.grad(r.loss * grad_scale, leaves, allow_unused=True)
        g = tuple((torch.zeros_like(u) if gi is None else gi).numpy() for u, gi in zip(leaves, g))
    n = lambda v: v.detach().numpy()
    return NS(obs=n(r.obs), dd=n(r.dd), err_g=n(r.err_g), loss_b=n(r.loss_b), loss=float(r.loss.detach()), g=g,
              out_max=float(out.detach().abs().max()), dout=n(r.dout), out=n(out))


def weights(rng, Bn, M, O):
    """cw (B, M, O) in [0.2, 2) with about a third exact zeros; observation (0, 1) has channel 0 live and channel 1 dead, observation
    (1, 0) has every channel dead, observation (2, M - 1) has only its LAST channel live (channel 16 at O = 17: the second accumulator)."""
    cw = f32(rng.uniform(0.2, 2.0, (Bn, M, O)))
    cw[rng.uniform(size=(Bn, M, O)) < 0.3] = 0.0
    cw[0, 1, 0], cw[0, 1, 1] = 1.25, 0.0
    cw[1, 0, :] = 0.0
    cw[2, M - 1, :] = 0.0
    cw[2, M - 1, O - 1] = 0.75
    return cw


def _smooth_point(c):
    """Is the yardstick differentiable enough at this point to judge fp32 kernels?  The decoder has relu units, and the fp64 gradient is
    the derivative on ONE side of every kink.  Where a pre-activation lies within fp32 rounding of zero, any fp32 evaluation -- the
    oracle's own code run in fp32 included -- may take the other side, and differs from the fp64 gradient by that unit's whole
    contribution, whatever the kernel does.  So the ORACLE is run once more in fp32 on the same inputs: a point is kept when its fp32
    gradients agree with its fp64 gradients within 2e-5 relative L2, a tenth of the f32 gradient tolerance of the tests.  The code
    under test takes no part in this."""
    tp = T.to_torch(c.prm, torch.float32)
    leaves = tuple(torch.tensor(np.asarray(u, dtype=np.float32), requires_grad=True) for u in (c.p, c.a, c.s))
    out = T.nef_apply(tp, c.cfg, torch.tensor(np.asarray(c.x, dtype=np.float32)), *leaves)
    g = torch.autograd.grad(group_loss(out.double(), c.y, c.G, c.q, c.cw).loss * c.gs, leaves)
    return all(np.linalg.norm(gi.numpy() - r) <= 2e-5 * np.linalg.norm(r) for gi, r in zip(g, c.ref.g))


def case(inv, G, N, D=64, H=2, seed=71, O=2):
    """One problem and its reference: the problem of tests/cells_ref.case -- the same decoder, points, latents, factors q and targets
    (B = 3 signals, Z = 7 latents, O channels, N = M G points per signal) -- with cw from ``weights`` in place of its w.  `y` is clean;
    `poisoned(c)` puts NaN / Inf under every dead value.  The seed advances by 1000 until the point is one the yardstick can judge
    at (_smooth_point)."""
    key = (inv, G, N, D, H, seed, O)
    while key not in _CASES:
        c = _case(inv, G, N, D, H, seed, O)
        if _smooth_point(c):
            _CASES[key] = c
        seed += 1000
    return _CASES[key]


def _case(inv, G, N, D, H, seed, O):
    c = CR.case(inv, G, N, D=D, H=H, seed=seed, O=O)
    cw = weights(np.random.default_rng(seed + 3), B, c.M, O)
    ref = cell_loss(c.cfg, c.prm, c.x, c.p, c.a, c.s, c.y, G, c.q, cw, c.gs)
    return NS(cfg=c.cfg, prm=c.prm, x=c.x, p=c.p, a=c.a, s=c.s, q=c.q, y=c.y, cw=cw, G=G, N=N, M=c.M, O=O, gs=c.gs, ref=ref, seed=seed)


def poisoned(c, kind="mixed"):
    """the targets with NaN / +-Inf ("mixed") or +Inf only ("inf") under every zero weight"""
    y = c.y.copy()
    gone = c.cw == 0
    vals = np.array([np.nan, np.inf, -np.inf]) if kind == "mixed" else np.array([np.inf])
    y[gone] = vals[np.arange(int(gone.sum())) % len(vals)]
    return y
