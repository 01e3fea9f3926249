"""The yardstick of the Gauss-Newton tests: the product  gv = coef * J^T (w * (J v)),  coef = grad_scale * 2 / (B N O),  of the
oracle's decode in fp64 -- torch.autograd.functional.jvp followed by one backward with the seed coef * w * tan -- and the
Levenberg-Marquardt loop of fitting/gauss_newton.py written on it (dense per-signal CG in fp64).  The cases are those of
tests/tangent_ref.py; weights and targets are seeded here, computed once per process and never modified."""
import numpy as np
import torch

from oracle import enf_ref_torch as T
from tests.tangent_ref import INVARIANTS, case, rel  # noqa: F401

_W, _FIT = {}, {}


def weights(shape, seed=7):
    """U(0.2, 2) with every seventh value (in memory order) set to 0: points, or values, that do not exist"""
    key = (tuple(shape), seed)
    if key not in _W:
        w = np.random.default_rng(seed).uniform(0.2, 2.0, size=shape)
        w.reshape(-1)[::7] = 0.0
        _W[key] = w
    return _W[key]


def _seed_weight(w, shape):
    if w is None:
        return torch.ones(shape, dtype=torch.float64)
    w = torch.tensor(np.asarray(w, dtype=np.float64))
    return (w[..., None] if w.dim() == 2 else w).expand(shape)


def oracle_gn(cfg, prm, x, p, a, s, v, w, grad_scale=1.0):
    """((gp, ga, gs), tan) in fp64 numpy: v = (vp, va, vs), a None entry is zero; w None, (B, N) or (B, N, O)."""
    tp = T.to_torch(prm, torch.float64)
    tx = torch.tensor(x)
    prim = tuple(torch.tensor(u) for u in (p, a, s))
    tang = tuple(torch.zeros_like(u) if d is None else torch.tensor(np.asarray(d, dtype=np.float64)) for u, d in zip(prim, v))
    f = lambda p_, a_, s_: T.nef_apply(tp, cfg, tx, p_, a_, s_)
    out, tan = torch.autograd.functional.jvp(f, prim, tang)
    B, N, O = out.shape
    coef = grad_scale * 2.0 / (B * N * O)
    leaves = tuple(u.clone().requires_grad_(True) for u in prim)
    seed = coef * _seed_weight(w, out.shape) * tan.detach()
    g = torch.autograd.grad(f(*leaves), leaves, grad_outputs=seed, allow_unused=True)
    g = tuple(torch.zeros_like(u) if gi is None else gi for u, gi in zip(leaves, g))
    return tuple(gi.numpy() for gi in g), tan.detach().numpy()


def oracle_loss_grad(cfg, prm, x, p, a, s, target, w=None, grad_scale=1.0):
    """(loss_b (B,), (gp, ga, gs)) of the weighted mean squared error, the gradient scaled by grad_scale: the fit step in fp64"""
    tp = T.to_torch(prm, torch.float64)
    leaves = tuple(torch.tensor(u, requires_grad=True) for u in (p, a, s))
    out = T.nef_apply(tp, cfg, torch.tensor(x), *leaves)
    B, N, O = out.shape
    err = _seed_weight(w, out.shape) * (out - torch.tensor(target)) ** 2
    loss_b = err.sum(dim=(1, 2)) / (N * O)
    g = torch.autograd.grad(loss_b.sum() / B * grad_scale, leaves, allow_unused=True)
    g = tuple(torch.zeros_like(u) if gi is None else gi for u, gi in zip(leaves, g))
    return loss_b.detach().numpy(), tuple(gi.numpy() for gi in g)


def fit_case(inv, seed=21):
    """The end-to-end fit: (cfg, prm, x, (p, a, s), target) with target = the oracle's decode of p + 0.05 N(0,1), a + 0.5 N(0,1)"""
    if (inv, seed) not in _FIT:
        cfg, prm, (x, p, a, s) = case(inv)[:3]
        rng = np.random.default_rng(seed)
        ps, as_ = p + 0.05 * rng.standard_normal(p.shape), a + 0.5 * rng.standard_normal(a.shape)
        tp = T.to_torch(prm, torch.float64)
        with torch.no_grad():
            target = T.nef_apply(tp, cfg, torch.tensor(x), torch.tensor(ps), torch.tensor(as_), torch.tensor(s)).numpy()
        _FIT[(inv, seed)] = (cfg, prm, x, (p, a, s), target)
    return _FIT[(inv, seed)]


def lm_loop(loss, product, p, a, s, steps, cg_iters=8, damping=1e-2, down=1.0 / 3.0, up=4.0, which=(0, 1)):
    """The Levenberg-Marquardt loop of fitting/gauss_newton.py in fp64, dense per-signal CG, on ANY loss, written once.  Two callables on
    the current latents ``cur`` = [p, a, s] say which:
      loss(cur, grads)  -> (loss_b (B,), (gp, ga, gs) at gradient scale B -- or anything without ``grads``)
      product(cur, v)   -> (gp, ga, gs), the Gauss-Newton product at gradient scale B along v = [vp, va, vs], a None entry is zero
    Returns loss_b (steps + 1, B) and the acceptance masks (steps, B).  `which`: the moving components (0 = p, 1 = a, 2 = sigma)."""
    B = p.shape[0]
    cur = [p.copy(), a.copy(), s.copy()]
    lam = np.full(B, damping)
    hist, accs = [], []
    bdot = lambda u, v: sum((ui * vi).reshape(B, -1).sum(1) for ui, vi in zip(u, v))
    for _ in range(steps):
        lb, g = loss(cur, True)
        hist.append(lb)
        r = [-g[c] for c in which]
        xs = [np.zeros_like(v) for v in r]
        d = [v.copy() for v in r]
        rho = bdot(r, r)
        for _ in range(cg_iters):
            v = [None, None, None]
            for c, dc in zip(which, d):
                v[c] = dc
            gv = product(cur, v)
            q = [gv[c] + lam.reshape(B, 1, 1) * dc for c, dc in zip(which, d)]
            kappa = bdot(d, q)
            live = (rho > 0) & np.isfinite(rho) & (kappa > 0) & np.isfinite(kappa)
            alpha = np.where(live, rho / np.where(live, kappa, 1.0), 0.0).reshape(B, 1, 1)
            xs = [xi + alpha * di for xi, di in zip(xs, d)]
            r = [ri - alpha * qi for ri, qi in zip(r, q)]
            rho2 = np.where(live, bdot(r, r), rho)
            beta = np.where(live, rho2 / np.where(live, rho, 1.0), 0.0).reshape(B, 1, 1)
            lv = live.reshape(B, 1, 1)
            d = [np.where(lv, ri + beta * di, di) for ri, di in zip(r, d)]
            rho = rho2
        trial = [v.copy() for v in cur]
        for c, dx in zip(which, xs):
            trial[c] = cur[c] + dx
        lb_t = loss(trial, False)[0]
        acc = lb_t < lb
        for c in which:
            cur[c] = np.where(acc.reshape(B, 1, 1), trial[c], cur[c])
        lam = np.where(acc, lam * down, lam * up)
        accs.append(acc)
        last = np.where(acc, lb_t, lb)
    hist.append(last)
    return np.stack(hist), np.stack(accs)


def sgd_rule(loss, p, a, s, steps, lr_p, lr_a):
    """The inner loop's SGD rule on (p, a) in fp64, written once: ``loss(cur, grads)`` -> (a value, (gp, ga, gs) at gradient scale B) as
    for lm_loop.  Returns (the values before every step and after the last one (steps + 1), the latents [p, a, s])."""
    cur = [p, a, s]
    vals = []
    for _ in range(steps):
        val, g = loss(cur, True)
        vals.append(val)
        cur = [cur[0] - lr_p * g[0], cur[1] - lr_a * g[1], s]
    vals.append(loss(cur, False)[0])
    return vals, cur


def oracle_lm(cfg, prm, x, target, p, a, s, steps, cg_iters=8, damping=1e-2, down=1.0 / 3.0, up=4.0, which=(0, 1)):
    """lm_fit_latents on the oracle (lm_loop on oracle_loss_grad and oracle_gn): loss_b (steps + 1, B) and the acceptance masks
    (steps, B).  `which`: the moving components (0 = p, 1 = a, 2 = sigma)."""
    B = float(p.shape[0])
    return lm_loop(lambda cur, grads: oracle_loss_grad(cfg, prm, x, *cur, target, grad_scale=B),
                   lambda cur, v: oracle_gn(cfg, prm, x, *cur, v, None, grad_scale=B)[0], p, a, s, steps, cg_iters, damping, down, up, which)


def oracle_sgd(cfg, prm, x, target, p, a, s, steps, lr_p=1.0, lr_a=5.0):
    """`steps` of the inner loop's SGD rule on (p, a) with gradient scale B: the final per-signal losses"""
    loss = lambda cur, grads: oracle_loss_grad(cfg, prm, x, *cur, target, grad_scale=float(p.shape[0]))
    return sgd_rule(loss, p, a, s, steps, lr_p, lr_a)[0][-1]


_GN = {}


def gn_case(inv, mode="none", grad_scale=3.0, **shape):
    """(case, w, (gp, ga, gs), tan) of tests/tangent_ref.case(inv, **shape) along its own tangents; mode: "none", "point" (w (B, N)) or
    "channel" (w (B, N, O))"""
    key = (inv, mode, grad_scale, tuple(sorted(shape.items())))
    if key not in _GN:
        c = case(inv, **shape)
        cfg, prm, (x, p, a, s), v = c[:4]
        B, N, O = c[4].shape
        w = None if mode == "none" else weights((B, N) if mode == "point" else (B, N, O))
        _GN[key] = (c, w) + oracle_gn(cfg, prm, x, p, a, s, v, w, grad_scale)
    return _GN[key]
