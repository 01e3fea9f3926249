"""The yardstick of the grouped Gauss-Newton tests (include/enf_hip.h, "Gauss-Newton product on grouped observations"), on the
oracle in fp64:

    obs_tan[b,m,o] = sum_{k<G} q[b, mG+k] tan[b, mG+k, o]                 tan = J v, by torch.autograd.functional.jvp (tests/gn_ref.py)
    seed[b, mG+k, o] = coef q[b, mG+k] (w[b,m] > 0 ? w[b,m] : 0) obs_tan[b,m,o]        coef = grad_scale 2 / (B M O)
    gv = J^T seed                                                         one backward

and the Levenberg-Marquardt loop and the SGD rule of tests/gn_ref.py written on tests/cells_ref.cell_loss and this product.  The
problems are those of tests/cells_ref.case (B = 3, Z = 7, O = 2, random q > 0, w with about a third exact zeros) with the tangents of
tests/tangent_ref.case for the same (inv, N); where a test needs another B or Z the problem is tests/tangent_ref.case's and q, w are
seeded here in the same way.  Inputs are rounded to fp32 (cells_ref.f32).  Everything is computed once per process and never modified."""
from types import SimpleNamespace as NS

import numpy as np
import torch

from oracle import enf_ref_torch as T
from tests import cells_ref, gn_ref, tangent_ref
from tests.cells_ref import cell_loss, f32, rel  # noqa: F401

_CASES, _FIT = {}, {}


def oracle_gn_cells(cfg, prm, x, p, a, s, v, G, q=None, w=None, grad_scale=1.0):
    """((gp, ga, gs), tan (B, N, O), obs_tan (B, M, O)) in fp64 numpy: v = (vp, va, vs), a None entry is zero; q None: 1 / G; w None: 1."""
    tp = T.to_torch(prm, torch.float64)
    tx = torch.tensor(np.asarray(x, dtype=np.float64))
    prim = tuple(torch.tensor(np.asarray(u, dtype=np.float64)) for u in (p, a, s))
    tang = tuple(torch.zeros_like(u) if d is None else torch.tensor(np.asarray(d, dtype=np.float64)) for u, d in zip(prim, v))
    f = lambda p_, a_, s_: T.nef_apply(tp, cfg, tx, p_, a_, s_)
    out, tan = torch.autograd.functional.jvp(f, prim, tang)
    tan = tan.detach()
    B, N, O = out.shape
    M = N // G
    assert M * G == N
    qt = torch.full((B, N), 1.0 / G, dtype=torch.float64) if q is None else torch.tensor(np.asarray(q, dtype=np.float64))
    wt = torch.ones((B, M), dtype=torch.float64) if w is None else torch.tensor(np.asarray(w, dtype=np.float64))
    obs_tan = (qt[..., None] * tan).reshape(B, M, G, O).sum(2)
    coef = grad_scale * 2.0 / (B * M * O)
    ws = torch.where(wt > 0, wt, torch.zeros_like(wt))
    seed = coef * qt[..., None] * (ws[..., None] * obs_tan).repeat_interleave(G, dim=1)
    leaves = tuple(u.clone().requires_grad_(True) for u in prim)
    g = torch.autograd.grad(f(*leaves), leaves, grad_outputs=seed, allow_unused=True)
    g = tuple(torch.zeros_like(u) if gi is None else gi for u, gi in zip(leaves, g))
    return tuple(gi.numpy() for gi in g), tan.numpy(), obs_tan.numpy()


def case(inv, G, N, D=64, H=2, B=3, Z=7, grad_scale=3.0, weights=True):
    """NS(cfg, prm, x, p, a, s, q, w, v = (vp, va, vs), G, N, M, O, gs, ref = (gp, ga, gs), tan, obs_tan).  B = 3, Z = 7: the problem of
    cells_ref.case(inv, G, N, D=, H=) with the tangents of tangent_ref.case(inv, D=, H=, C=12, N=); another B or Z: the problem and
    the tangents of tangent_ref.case(inv, D=, H=, B=, N=, Z=) with q = U(0.2, 2) / G and w = U(0.2, 2) with about a third exact zeros,
    default_rng(73).  `weights` False: the reference for qweight = None, obs_weight = None (q and w are then None)."""
    key = (inv, G, N, D, H, B, Z, grad_scale, weights)
    if key not in _CASES:
        if (B, Z) == (cells_ref.B, cells_ref.Z):
            c = cells_ref.case(inv, G, N, D=D, H=H)
            cfg, prm, x, p, a, s, q, w = c.cfg, c.prm, c.x, c.p, c.a, c.s, c.q, c.w
            v = tangent_ref.case(inv, D=D, H=H, C=12, N=N)[3]
        else:
            cfg, prm, xpas, v = tangent_ref.case(inv, D=D, H=H, B=B, N=N, Z=Z)[:4]
            x, p, a, s = (f32(u) for u in xpas)
            rng = np.random.default_rng(73)
            q = f32(rng.uniform(0.2, 2.0, (B, N)) / G)
            w = f32(rng.uniform(0.2, 2.0, (B, N // G)))
            w[rng.uniform(size=w.shape) < 0.3] = 0.0
            w[B - 1, 0] = 0.0
        v = tuple(f32(u) for u in v)
        assert all(u.shape == t.shape for u, t in zip(v, (p, a, s)))
        if not weights:
            q = w = None
        ref, tan, obs_tan = oracle_gn_cells(cfg, prm, x, p, a, s, v, G, q, w, grad_scale)
        _CASES[key] = NS(cfg=cfg, prm=prm, x=x, p=p, a=a, s=s, q=q, w=w, v=v, G=G, N=N, M=N // G, O=cfg["num_out"], gs=grad_scale, ref=ref,
                         tan=tan, obs_tan=obs_tan)
    return _CASES[key]


def fit_case(inv, G=4, N=80, seed=21, scale_p=0.05, scale_a=0.5):
    """The end-to-end fit on cells: NS(cfg, prm, x, p, a, s, q, G, target).  The (G, N) rows of tangent_ref.case(inv, N=N), rounded to
    fp32, q = U(0.2, 2) normalised to sum 1 per group (default_rng(seed + 1)), target = the fp64 group sums of the oracle's decode at
    p + scale_p N(0,1), a + scale_a N(0,1), default_rng(seed)."""
    key = (inv, G, N, seed, scale_p, scale_a)
    if key not in _FIT:
        cfg, prm, xpas = tangent_ref.case(inv, N=N)[:3]
        x, p, a, s = (f32(u) for u in xpas)
        B = p.shape[0]
        rng = np.random.default_rng(seed)
        ps, as_ = p + scale_p * rng.standard_normal(p.shape), a + scale_a * rng.standard_normal(a.shape)
        q = np.random.default_rng(seed + 1).uniform(0.2, 2.0, (B, N // G, G))
        q = f32((q / q.sum(-1, keepdims=True)).reshape(B, N))
        target = cell_loss(cfg, prm, x, ps, as_, s, np.zeros((B, N // G, cfg["num_out"])), G, q, grads=False).obs
        _FIT[key] = NS(cfg=cfg, prm=prm, x=x, p=p, a=a, s=s, q=q, G=G, target=target)
    return _FIT[key]


def _loss(cfg, prm, x, q, G, target, w, B):
    """cells_ref.cell_loss at gradient scale B as tests/gn_ref.lm_loop and sgd_rule take a loss: (loss_b, g)"""
    def loss(cur, grads):
        r = cell_loss(cfg, prm, x, *cur, target, G, q, w, float(B), grads=grads)
        return r.loss_b, r.g
    return loss


def oracle_lm_cells(cfg, prm, x, q, G, target, p, a, s, steps, w=None, cg_iters=8, damping=1e-2, down=1.0 / 3.0, up=4.0, which=(0, 1)):
    """lm_fit_cell_averages on the oracle (tests/gn_ref.lm_loop on the grouped loss and product): loss_b (steps + 1, B) and the
    acceptance masks (steps, B).  `which`: the moving components (0 = p, 1 = a, 2 = sigma)."""
    B = p.shape[0]
    return gn_ref.lm_loop(_loss(cfg, prm, x, q, G, target, w, B), lambda cur, v: oracle_gn_cells(cfg, prm, x, *cur, v, G, q, w, float(B))[0],
                          p, a, s, steps, cg_iters, damping, down, up, which)


def oracle_sgd_cells(cfg, prm, x, q, G, target, p, a, s, steps, w=None, lr_p=1.0, lr_a=5.0):
    """`steps` of the inner loop's SGD rule on (p, a) with gradient scale B against the grouped loss: the final per-signal losses"""
    return gn_ref.sgd_rule(_loss(cfg, prm, x, q, G, target, w, p.shape[0]), p, a, s, steps, lr_p, lr_a)[0][-1]
