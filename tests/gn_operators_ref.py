"""The yardstick of the Gauss-Newton tests on sparse observation operators (include/enf_hip.h, "Gauss-Newton product on sparse
observations"), on the oracle in fp64 and the DENSE operator:

    tan = J v                                       by torch.autograd.functional.jvp, as tests/gn_cells_ref.py
    obs_tan[b,m,o] = sum_n A[m,n] tan[b,n,o]
    seed[b,n,o] = coef sum_m A[m,n] ((w > 0 ? w : 0) obs_tan)[b,m,o]              coef = grad_scale 2 / (B M O)
    gv = J^T seed                                   one backward

and the Levenberg-Marquardt loop and the SGD rule of tests/gn_cells_ref.py written on tests/operators_ref.operator_loss and this
product.  The problems are those of tests/operators_ref.case (ragged rows, unsorted columns, spare columns, w (B, M) or (B, M, O) with
about a third exact zeros) with the tangents of tests/tangent_ref.case for the same (inv, N).  Everything is computed once per process
and never modified."""
from types import SimpleNamespace as NS

import numpy as np
import torch

from oracle import enf_ref_torch as T
from tests import gn_cells_ref, gn_ref, operators_ref, tangent_ref
from tests.operators_ref import _weights, f32, operator_loss, ragged_entries, rel  # noqa: F401

_CASES, _FIT = {}, {}


def oracle_gn_operator(cfg, prm, x, p, a, s, v, A, w=None, grad_scale=1.0):
    """((gp, ga, gs), tan (B, N, O), obs_tan (B, M, O)) in fp64 numpy: v = (vp, va, vs), a None entry is zero; A dense (M, N); w None,
    (B, M) or (B, M, O)."""
    tp = T.to_torch(prm, torch.float64)
    tx = torch.tensor(np.asarray(x, dtype=np.float64))
    prim = tuple(torch.tensor(np.asarray(u, dtype=np.float64)) for u in (p, a, s))
    tang = tuple(torch.zeros_like(u) if d is None else torch.tensor(np.asarray(d, dtype=np.float64)) for u, d in zip(prim, v))
    f = lambda p_, a_, s_: T.nef_apply(tp, cfg, tx, p_, a_, s_)
    out, tan = torch.autograd.functional.jvp(f, prim, tang)
    tan = tan.detach()
    At = torch.tensor(np.asarray(A, dtype=np.float64))
    obs_tan = torch.einsum("mn,bno->bmo", At, tan)
    Bn, M, O = obs_tan.shape
    wt = torch.tensor(_weights(w, (Bn, M, O)))
    ws = torch.where(wt > 0, wt, torch.zeros_like(wt))
    seed = grad_scale * 2.0 / (Bn * M * O) * torch.einsum("mn,bmo->bno", At, ws * obs_tan)
    leaves = tuple(u.clone().requires_grad_(True) for u in prim)
    g = torch.autograd.grad(f(*leaves), leaves, grad_outputs=seed, allow_unused=True)
    g = tuple(torch.zeros_like(u) if gi is None else gi for u, gi in zip(leaves, g))
    return tuple(gi.numpy() for gi in g), tan.numpy(), obs_tan.numpy()


def case(inv, lengths, N, D=64, H=2, O=2, weights="obs", Bn=operators_ref.B, Zn=operators_ref.Z, spare=3, grad_scale=3.0):
    """operators_ref.case(inv, lengths, N, ...) with v = the tangents of tangent_ref.case(inv, D=, H=, C=12, B=, N=, Z=) rounded to fp32,
    gs = grad_scale and ref = (gp, ga, gs), tan, obs_tan of the product."""
    key = (inv, tuple(lengths), N, D, H, O, weights, Bn, Zn, spare, grad_scale)
    if key not in _CASES:
        c = operators_ref.case(inv, lengths, N, D=D, H=H, O=O, weights=weights, Bn=Bn, Zn=Zn, spare=spare)
        v = tuple(f32(u) for u in tangent_ref.case(inv, D=D, H=H, C=12, B=Bn, N=N, Z=Zn)[3])
        assert all(u.shape == t.shape for u, t in zip(v, (c.p, c.a, c.s)))
        ref, tan, obs_tan = oracle_gn_operator(c.cfg, c.prm, c.x, c.p, c.a, c.s, v, c.A, c.w, grad_scale)
        _CASES[key] = NS(cfg=c.cfg, prm=c.prm, x=c.x, p=c.p, a=c.a, s=c.s, rows=c.rows, cols=c.cols, vals=c.vals, A=c.A, w=c.w, N=N, M=c.M,
                         O=O, B=Bn, Z=Zn, weights=weights, v=v, gs=grad_scale, ref=ref, tan=tan, obs_tan=obs_tan)
    return _CASES[key]


def fit_case(inv, seed=21, scale_p=0.05, scale_a=0.5):
    """The end-to-end fit on an operator: NS(cfg, prm, x, p, a, s, rows, cols, vals, A, M, N, target).  The rows (p, a, s, x) of
    gn_cells_ref.fit_case(inv) (N = 80); the operator's rows from ragged_entries([1, 3, 9, 27, 5, 70] * 4, 80, 301, spare=0), their
    factors made positive and normalised to row sum 1, rounded to fp32; target = the fp64 A out of the oracle's decode at
    p + scale_p N(0,1), a + scale_a N(0,1), default_rng(seed)."""
    key = (inv, seed, scale_p, scale_a)
    if key not in _FIT:
        f = gn_cells_ref.fit_case(inv)
        N = f.x.shape[1]
        lengths = [1, 3, 9, 27, 5, 70] * 4
        rows, cols, vals = ragged_entries(lengths, N, 301, spare=0)
        vals = np.abs(np.asarray(vals, dtype=np.float64))
        vals = f32(vals / np.bincount(rows, weights=vals, minlength=len(lengths))[rows])
        A = np.zeros((len(lengths), N))
        np.add.at(A, (rows, cols), vals)
        rng = np.random.default_rng(seed)
        ps, as_ = f.p + scale_p * rng.standard_normal(f.p.shape), f.a + scale_a * rng.standard_normal(f.a.shape)
        target = operator_loss(f.cfg, f.prm, f.x, ps, as_, f.s, A, np.zeros((f.p.shape[0], len(lengths), f.cfg["num_out"])), grads=False).obs
        _FIT[key] = NS(cfg=f.cfg, prm=f.prm, x=f.x, p=f.p, a=f.a, s=f.s, rows=rows, cols=cols, vals=vals, A=A, M=len(lengths), N=N,
                       target=target)
    return _FIT[key]


def _loss(cfg, prm, x, A, target, w, B):
    """operators_ref.operator_loss at gradient scale B as tests/gn_ref.lm_loop and sgd_rule take a loss: (loss_b, g)"""
    def loss(cur, grads):
        r = operator_loss(cfg, prm, x, *cur, A, target, w, float(B), grads=grads)
        return r.loss_b, r.g
    return loss


def oracle_lm_operator(cfg, prm, x, A, target, p, a, s, steps, w=None, cg_iters=8, damping=1e-2, down=1.0 / 3.0, up=4.0, which=(0, 1)):
    """lm_fit_linear_observations on the oracle (tests/gn_ref.lm_loop on the operator's loss and product): loss_b (steps + 1, B) and the
    acceptance masks (steps, B).  `which`: the moving components (0 = p, 1 = a, 2 = sigma)."""
    B = p.shape[0]
    return gn_ref.lm_loop(_loss(cfg, prm, x, A, target, w, B), lambda cur, v: oracle_gn_operator(cfg, prm, x, *cur, v, A, w, float(B))[0],
                          p, a, s, steps, cg_iters, damping, down, up, which)


def oracle_sgd_operator(cfg, prm, x, A, target, p, a, s, steps, w=None, lr_p=1.0, lr_a=5.0):
    """`steps` of the inner loop's SGD rule on (p, a) with gradient scale B against the operator's loss: the final per-signal losses"""
    return gn_ref.sgd_rule(_loss(cfg, prm, x, A, target, w, p.shape[0]), p, a, s, steps, lr_p, lr_a)[0][-1]
