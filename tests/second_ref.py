"""The yardstick of the second-derivative tests: nested forward mode on the fp64 oracle -- torch.func.jvp of torch.func.jvp of
oracle.enf_ref_torch.nef_apply over x, both along the same direction -- which gives (out, J_x xdot, xdot^T H_x xdot) "exactly" as
autograd means it: almost everywhere, relu'' = 0.  The cases are tests/tangent_x_ref.case's, inputs and xdot included; a case is
computed once per process and never modified."""
import numpy as np
import torch

from oracle import enf_ref_torch as T
from tests.tangent_x_ref import INVARIANTS, CASES_3D, case as case_x, oracle_jvp_x, rel  # noqa: F401

_CASES = {}


def oracle_second_x(cfg, prm, x, p, a, s, xdot):
    """(out, tan, tan2) of the oracle in fp64 (numpy): tan = J_x xdot, tan2 = xdot^T (d^2 out / d x^2) xdot per (b, n, o)"""
    tp = T.to_torch(prm, torch.float64)
    X, P, A, S, V = (torch.tensor(np.asarray(v, dtype=np.float64)) for v in (x, p, a, s, xdot))
    f = lambda x_: T.nef_apply(tp, cfg, x_, P, A, S)
    first = lambda x_: torch.func.jvp(f, (x_,), (V,))            # (out, tan) as a function of x
    (out, tan), (tan_again, tan2) = torch.func.jvp(first, (X,), (V,))
    assert torch.equal(tan, tan_again)
    return out.detach().numpy(), tan.detach().numpy(), tan2.detach().numpy()


def oracle_hessian_x(cfg, prm, x, p, a, s):
    """d^2 out[b, n, o] / d x[b, n, i] d x[b, n, j] of the oracle by reverse over reverse: (B, N, O, dx, dx).  A query's output depends on
    its own coordinates only, so the gradient of sum_{b, n} grad_i is the per-query second derivative."""
    tp = T.to_torch(prm, torch.float64)
    X = torch.tensor(np.asarray(x, dtype=np.float64), requires_grad=True)
    P, A, S = (torch.tensor(np.asarray(v, dtype=np.float64)) for v in (p, a, s))
    out = T.nef_apply(tp, cfg, X, P, A, S)
    dx = X.shape[-1]
    H = np.zeros(tuple(out.shape) + (dx, dx))
    for o in range(out.shape[-1]):
        g = torch.autograd.grad(out[..., o].sum(), X, create_graph=True)[0]
        for i in range(dx):
            H[:, :, o, i, :] = torch.autograd.grad(g[..., i].sum(), X, retain_graph=True)[0].numpy()
    return H


def case(inv, **kw):
    """(cfg, prm, (x, p, a, s), xdot, out_ref, tan_ref, tan2_ref) on tests/tangent_x_ref.case's inputs (its keywords)"""
    key = (inv, tuple(sorted((k, tuple(v) if isinstance(v, (list, tuple)) else v) for k, v in kw.items())))
    if key not in _CASES:
        c = case_x(inv, **kw)
        _CASES[key] = c[:4] + oracle_second_x(c[0], c[1], *c[2], c[3])
    return _CASES[key]
