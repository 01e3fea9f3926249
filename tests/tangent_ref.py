"""The yardstick of the tangent tests: the Jacobian-vector product of the oracle's decode with respect to its latents, by fp64
autograd (torch.autograd.functional.jvp of oracle.enf_ref_torch.nef_apply), and the seeded cases the CPU and GPU tests share.  A case
is computed once per process and never modified."""
import numpy as np
import torch

from oracle import enf_ref_np as R
from oracle import enf_ref_torch as T
from tests.helpers import make_cfg, make_inputs
from tests.test_gpu_backward import rel  # noqa: F401  (the relative Frobenius error the gradient tests use)

INVARIANTS = ["rel_pos_periodic", "latitude_periodic", "polar_periodic", "ponita", "abs_pos", "rel_pos", "norm_rel_pos"]
_CASES = {}


def oracle_jvp(cfg, prm, x, p, a, s, dp, da, ds):
    """(out, tan) of the oracle in fp64 (numpy); a None tangent is zero."""
    tp = T.to_torch(prm, torch.float64)
    tx = torch.tensor(x)
    prim = tuple(torch.tensor(v) for v in (p, a, s))
    tang = tuple(torch.zeros_like(v) if d is None else torch.tensor(np.asarray(d, dtype=np.float64)) for v, d in zip(prim, (dp, da, ds)))
    out, tan = torch.autograd.functional.jvp(lambda p_, a_, s_: T.nef_apply(tp, cfg, tx, p_, a_, s_), prim, tang)
    return out.detach().numpy(), tan.detach().numpy()


def make_tangents(p, a, s, seed):
    """0.3 N(0,1), N(0,1), 0.1 N(0,1) in the shapes of p, a, sigma"""
    rng = np.random.default_rng(seed)
    return 0.3 * rng.standard_normal(p.shape), rng.standard_normal(a.shape), 0.1 * rng.standard_normal(s.shape)


def case(inv, D=64, H=2, C=8, O=2, B=3, N=50, Z=7, seed=1, use_window=True, freq=(0.05, 0.1)):
    """(cfg, prm, (x, p, a, s), (dp, da, ds), out_ref, tan_ref); the defaults are the shape the reference was validated at: N = 50
    leaves a partial 16-query tile, Z = 7 leaves a wave without a latent."""
    key = (inv, D, H, C, O, B, N, Z, seed, use_window, tuple(freq))
    if key not in _CASES:
        cfg = make_cfg(inv, D=D, H=H, C=C, O=O, use_window=use_window, freq=freq)
        prm = R.init_params(0, cfg, jitter=0.1)
        xpas = make_inputs(cfg, B, N, Z, seed)
        tang = make_tangents(*xpas[1:], seed + 100)
        _CASES[key] = (cfg, prm, xpas, tang) + oracle_jvp(cfg, prm, *xpas, *tang)
    return _CASES[key]

