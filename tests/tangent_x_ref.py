"""The yardstick of the directional-derivative tests: the Jacobian-vector product of the oracle's decode over (x, p, a, sigma) in fp64
(torch.autograd.functional.jvp of oracle.enf_ref_torch.nef_apply), with a seeded query direction xdot ~ N(0, 1) in the shape of x beside
the latent tangents of tests/tangent_ref.py, and the seeded cases the CPU and GPU tests share.  A case is computed once per process and
never modified."""
import numpy as np
import torch

from oracle import enf_ref_np as R
from oracle import enf_ref_torch as T
from tests.helpers import make_cfg, make_inputs
from tests.tangent_ref import INVARIANTS, make_tangents, rel  # noqa: F401

CASES_3D = ["rel_pos", "abs_pos", "norm_rel_pos"]          # the invariants that also take num_in = 3
_CASES = {}


def oracle_jvp_x(cfg, prm, x, p, a, s, xdot, dp, da, ds):
    """(out, tan) of the oracle in fp64 (numpy) along (xdot, dp, da, ds); a None tangent is zero."""
    tp = T.to_torch(prm, torch.float64)
    prim = tuple(torch.tensor(np.asarray(v, dtype=np.float64)) for v in (x, p, a, s))
    tang = tuple(torch.zeros_like(v) if d is None else torch.tensor(np.asarray(d, dtype=np.float64)) for v, d in zip(prim, (xdot, dp, da, ds)))
    out, tan = torch.autograd.functional.jvp(lambda x_, p_, a_, s_: T.nef_apply(tp, cfg, x_, p_, a_, s_), prim, tang)
    return out.detach().numpy(), tan.detach().numpy()


def oracle_jacobian_x(cfg, prm, x, p, a, s):
    """d out[b, n, o] / d x[b, n, :] of the oracle by reverse-mode autograd, one backward per channel: (B, N, O, dx)"""
    tp = T.to_torch(prm, torch.float64)
    X = torch.tensor(x, requires_grad=True)
    out = T.nef_apply(tp, cfg, X, torch.tensor(p), torch.tensor(a), torch.tensor(s))
    cols = [torch.autograd.grad(out[..., o].sum(), X, retain_graph=True)[0].numpy() for o in range(out.shape[-1])]
    return np.stack(cols, axis=2)


def make_xdot(x, seed):
    """N(0, 1) in the shape of x.  (`case` seeds it with seed + 400: at the base shape no central difference of the ten cases of
    tests/test_tangent_x_host.py then straddles a relu kink.  The 3-D rel_pos inputs have a pre-activation within ~1e-6 of zero, and
    with the offsets 200, 300, 500 the h = 1e-6 difference crosses it: 3.4e-3, 7.0e-5, 1.9e-3 against the JVP, which agrees with the
    oracle's reverse-mode Jacobian to 1.6e-15 for every one of them.  That is the difference's limit, not the JVP's.)"""
    return np.random.default_rng(seed).standard_normal(x.shape)


def case(inv, D=64, H=2, C=8, O=2, B=3, N=50, Z=7, seed=1, num_in=2, use_window=True, freq=(0.05, 0.1)):
    """(cfg, prm, (x, p, a, s), xdot, (dp, da, ds), out_ref, tan_x_ref, tan_all_ref): tan_x_ref along xdot alone, tan_all_ref along all
    four tangents.  The defaults are tests/tangent_ref.py's shape (a partial 16-query tile, a wave without a latent) with its inputs and
    latent tangents."""
    key = (inv, D, H, C, O, B, N, Z, seed, num_in, use_window, tuple(freq))
    if key not in _CASES:
        cfg = make_cfg(inv, D=D, H=H, C=C, O=O, num_in=num_in, use_window=use_window, freq=freq)
        prm = R.init_params(0, cfg, jitter=0.1)
        xpas = make_inputs(cfg, B, N, Z, seed)
        tang = make_tangents(*xpas[1:], seed + 100)
        xdot = make_xdot(xpas[0], seed + 400)
        out, tan_x = oracle_jvp_x(cfg, prm, *xpas, xdot, None, None, None)
        _, tan_all = oracle_jvp_x(cfg, prm, *xpas, xdot, *tang)
        _CASES[key] = (cfg, prm, xpas, xdot, tang, out, tan_x, tan_all)
    return _CASES[key]
