"""Cases and fp64 references of the coordinate-dimension and latent-width tests (tests/test_gpu_coord_dims.py,
tests/test_coord_dims_host.py): dx = 1 and 3 for the three translation invariants, and latent_dim 1 .. 130 at dx = 2.

Shapes.  A: make_cfg(inv, D=64, H=2, C=8, O=2, num_in=dx, freq=(0.5, 1.0)) at (B, N, Z) = (3, 50, 7) -- 150 rows: nine 16-query tiles and
a ragged tenth, signals start in mid-tile, a wave without a latent -- and (2, 130, 9): a partial query tile and a second 128-query
workgroup.  Grouped observations need N = M G: (3, 52, 7) with G = 4.  B: rel_pos_periodic (and one ponita case) at (2, 40, 9) and
(2, 40, 37), latent_dim from C_LIST.

Windows.  make_inputs gives sigma ~ dx / round(Z^(1/dx)): 0.14 at dx = 1, Z = 7 and 1.5 at dx = 3.  Every case here passes the
sigma_scale that puts the window where the 2-D suite has it at Z = 7 and Z = 9, sigma = 2/3 (1 +- 0.1), and `problem` asserts that the
mean lies in [0.5, 1.5]: these tests are about dx and C, not about sharp windows.

Inputs are rounded to fp32 (the oracle sees the numbers the kernels get).  Every reference is the fp64 oracle, computed once per
process and never modified."""
from types import SimpleNamespace as NS

import numpy as np
import torch

from oracle import enf_ref_np as R
from oracle import enf_ref_torch as T
from tests.helpers import make_cfg, make_inputs
from tests.test_gpu_backward import rel  # noqa: F401

INVS = ("rel_pos", "abs_pos", "norm_rel_pos")
DXS = (1, 3)
BASE, TILES, CELLS = (3, 50, 7), (2, 130, 9), (3, 52, 7)
FREQ = (0.5, 1.0)
SIGMA = 2.0 / 3.0
C_LIST = (1, 3, 17, 33, 64, 100, 130)
C_DEEP = (1, 33, 130)                    # the widths that also run at Z = 37 and through the forward-mode and update kernels
G = 4
_CACHE = {}


def f32(v):
    """rounded to fp32 and back"""
    return np.asarray(v, dtype=np.float32).astype(np.float64)


def _once(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def sigma_scale(inv, num_in, Z):
    """the factor that turns make_inputs' sigma = z_pos / round(Z^(1 / z_pos)) into SIGMA"""
    zp = R.invariant_spec(inv, num_in)["z_pos"]
    return SIGMA / (zp / max(1.0, round(Z ** (1.0 / zp))))


def problem(inv, dx, shape=BASE, D=64, H=2, C=8, O=2, seed=11):
    """NS(cfg, prm, x, p, a, s, w, out, ...): one decode problem, a cotangent w ~ N(0, 1) in the shape of out, the oracle's out"""
    key = ("problem", inv, dx, tuple(shape), D, H, C, O, seed)

    def make():
        B, N, Z = shape
        cfg = make_cfg(inv, D=D, H=H, C=C, O=O, num_in=dx, freq=FREQ)
        prm = R.init_params(seed, cfg, jitter=0.1)
        x, p, a, s = (f32(v) for v in make_inputs(cfg, B, N, Z, seed + 1, sigma_scale=sigma_scale(inv, dx, Z)))
        assert 0.5 <= float(s.mean()) <= 1.5, (inv, dx, shape, float(s.mean()))
        assert x.shape == (B, N, dx) and a.shape == (B, Z, C)
        w = f32(np.random.default_rng(seed + 2).standard_normal((B, N, O)))
        return NS(cfg=cfg, prm=prm, x=x, p=p, a=a, s=s, w=w, out=R.nef_apply(prm, cfg, x, p, a, s), key=key, inv=inv, dx=dx, B=B, N=N,
                  Z=Z, C=C, O=O, D=D, H=H)
    return _once(key, make)


def latent_problem(C, Z=9, inv="rel_pos_periodic"):
    """section B: dx = 2, (B, N) = (2, 40), latent_dim C"""
    # (seed: with 31, as everywhere else, the C = 33, Z = 37 case has the relu pre-activation of feature 28 of the value embedding at
    #  the pair (b, n, z) = (0, 31, 24) at -4.98e-7, 8.2e-8 of the sum of its terms' magnitudes: within fp32 rounding of zero.  The
    #  kernels' mask differs from the fp64 oracle's there, and that one flip moves d/dp by 6.247e-4 of its norm in the oracle itself
    #  (d/da by 3e-10) -- the 6.246e-4 both backward variants measured; the reason tests/test_gpu_layers.py:42-43 records.  With 35
    #  the smallest ratio of the case is 1.4e-6.)
    return problem(inv, 2, shape=(2, 40, Z), C=C, seed=35 if (C, Z, inv) == (33, 37, "rel_pos_periodic") else 31)


def all_cases():
    """every problem the GPU file builds: (label, problem) -- the sigma condition is checked on each"""
    for inv in INVS:
        for dx in DXS:
            for shape in (BASE, TILES, CELLS):
                yield f"{inv} dx={dx} {shape}", problem(inv, dx, shape)
            yield f"{inv} dx={dx} 128x2", problem(inv, dx, BASE, D=128, H=2)
            yield f"{inv} dx={dx} 64x4", problem(inv, dx, BASE, D=64, H=4)
        yield f"{inv} dx=2", problem(inv, 2)
    for C in C_LIST:
        yield f"C={C}", latent_problem(C)
    for C in C_DEEP:
        yield f"C={C} Z=37", latent_problem(C, 37)
    yield "ponita C=130", latent_problem(130, 9, "ponita")


# ---- reverse mode: one backward gives d x, d p, d a, d sigma and every weight gradient
def backward(c):
    """NS(gx, gp, ga, gs, gw): gradients of sum(out * c.w); gw in the order of enf_pde_amd.enf.models.TENSOR_PATHS"""
    def make():
        from enf_pde_amd.enf.models import TENSOR_PATHS
        tp = T.to_torch(c.prm, torch.float64, requires_grad=True)
        leaves = [torch.tensor(v, requires_grad=True) for v in (c.x, c.p, c.a, c.s)]
        out = T.nef_apply(tp, c.cfg, *leaves)
        (out * torch.tensor(c.w)).sum().backward()
        g = lambda t: np.zeros(tuple(t.shape)) if t.grad is None else t.grad.numpy()

        def get(path):
            tree = tp["params"]
            for k in path:
                tree = tree[k]
            return tree
        return NS(gx=g(leaves[0]), gp=g(leaves[1]), ga=g(leaves[2]), gs=g(leaves[3]), gw=[g(get(path)) for path in TENSOR_PATHS])
    return _once(("backward", c.key), make)


def shared_grid(c):
    """NS(out, gx (N, dx)): signal 0's points for every signal (a stride-0 batch); the gradient w.r.t. the grid sums over the signals"""
    def make():
        tp = T.to_torch(c.prm, torch.float64)
        x0 = torch.tensor(c.x[0], requires_grad=True)
        out = T.nef_apply(tp, c.cfg, x0[None].expand(c.B, -1, -1), torch.tensor(c.p), torch.tensor(c.a), torch.tensor(c.s))
        (out * torch.tensor(c.w)).sum().backward()
        return NS(out=out.detach().numpy(), gx=x0.grad.numpy())
    return _once(("shared", c.key), make)


def jacobian(c):
    """d out / d x, (B, N, O, dx): tests/tangent_x_ref.oracle_jacobian_x"""
    from tests.tangent_x_ref import oracle_jacobian_x
    return _once(("jac", c.key), lambda: oracle_jacobian_x(c.cfg, c.prm, c.x, c.p, c.a, c.s))


# ---- the fused fit step
def fit(c):
    """NS(y, wt, loss_b, loss, g): targets N(0, 1), per-point weights U(0.2, 2) with about a third exact zeros, and the weighted mean
    squared error with its gradients times B (tests/gn_ref.oracle_loss_grad)"""
    def make():
        from tests.gn_ref import oracle_loss_grad
        rng = np.random.default_rng(41)
        y = f32(rng.standard_normal((c.B, c.N, c.O)))
        wt = f32(rng.uniform(0.2, 2.0, (c.B, c.N)))
        wt[rng.uniform(size=wt.shape) < 0.33] = 0.0
        wt[c.B - 1, 0] = 0.0
        loss_b, g = oracle_loss_grad(c.cfg, c.prm, c.x, c.p, c.a, c.s, y, wt, float(c.B))
        return NS(y=y, wt=wt, loss_b=loss_b, loss=float(loss_b.mean()), g=g)
    return _once(("fit", c.key), make)


def cells(c):
    """NS(q, y, wt, ref): G = 4 consecutive rows per observation, factors U(0.2, 2) / G, observation weights with exact zeros; ref =
    tests/cells_ref.cell_loss (gradients times B)"""
    def make():
        from tests.cells_ref import cell_loss
        assert c.N % G == 0
        rng = np.random.default_rng(43)
        M = c.N // G
        q = f32(rng.uniform(0.2, 2.0, (c.B, c.N)) / G)
        y = f32(rng.standard_normal((c.B, M, c.O)))
        wt = f32(rng.uniform(0.2, 2.0, (c.B, M)))
        wt[rng.uniform(size=wt.shape) < 0.3] = 0.0
        wt[1, 0] = 0.0
        return NS(q=q, y=y, wt=wt, M=M, ref=cell_loss(c.cfg, c.prm, c.x, c.p, c.a, c.s, y, G, q, wt, float(c.B)))
    return _once(("cells", c.key), make)


# ---- forward mode
def tangents(c):
    """(dp, da, ds) of tests/tangent_ref.make_tangents and xdot of tests/tangent_x_ref.make_xdot, rounded to fp32"""
    def make():
        from tests.tangent_ref import make_tangents
        from tests.tangent_x_ref import make_xdot
        return NS(v=tuple(f32(u) for u in make_tangents(c.p, c.a, c.s, 151)), xdot=f32(make_xdot(c.x, 451)))
    return _once(("tangents", c.key), make)


def tangent(c, which="latent"):
    """the oracle's tangent: "latent" along (dp, da, ds); "da" along da alone; "xdot" along xdot alone; "all" along all four"""
    def make():
        from tests.tangent_x_ref import oracle_jvp_x
        tg = tangents(c)
        dirs = {"latent": (None,) + tg.v, "da": (None, None, tg.v[1], None), "xdot": (tg.xdot, None, None, None), "all": (tg.xdot,) + tg.v}[which]
        return oracle_jvp_x(c.cfg, c.prm, c.x, c.p, c.a, c.s, *dirs)[1]
    return _once(("tangent", which, c.key), make)


def second(c):
    """(tan, tan2) along xdot: tests/second_ref.oracle_second_x"""
    from tests.second_ref import oracle_second_x
    return _once(("second", c.key), lambda: oracle_second_x(c.cfg, c.prm, c.x, c.p, c.a, c.s, tangents(c).xdot)[1:])


def gn(c, grad_scale=3.0):
    """NS(wt, ref): the Gauss-Newton product along the latent tangents with tests/gn_ref.weights per point"""
    def make():
        from tests.gn_ref import oracle_gn, weights
        wt = f32(weights((c.B, c.N)))
        return NS(wt=wt, gs=grad_scale, ref=oracle_gn(c.cfg, c.prm, c.x, c.p, c.a, c.s, tangents(c).v, wt, grad_scale)[0])
    return _once(("gn", c.key, grad_scale), make)


def gn_cells(c, grad_scale=3.0):
    """the grouped product on cells(c)'s factors and weights: tests/gn_cells_ref.oracle_gn_cells"""
    def make():
        from tests.gn_cells_ref import oracle_gn_cells
        k = cells(c)
        return NS(gs=grad_scale, ref=oracle_gn_cells(c.cfg, c.prm, c.x, c.p, c.a, c.s, tangents(c).v, G, k.q, k.wt, grad_scale)[0])
    return _once(("gn_cells", c.key, grad_scale), make)


def cg_step(c, lam=(0.05, 0.5, 2.0)):
    """One CG iteration from x = 0 on (G + lam I) x = -g in fp64, the formulas of tests/gn_ref.oracle_lm's inner loop on the components
    (p, a): NS(y, rhs, lam, x).  g is the fit step's gradient at grad_scale B for targets N(0, 1)."""
    def make():
        from tests.gn_ref import oracle_gn, oracle_loss_grad
        B = c.B
        y = f32(np.random.default_rng(47).standard_normal((B, c.N, c.O)))
        lm = np.asarray(lam[:B], dtype=np.float64)
        _, g = oracle_loss_grad(c.cfg, c.prm, c.x, c.p, c.a, c.s, y, None, float(B))
        r = [f32(-g[0]), f32(-g[1])]
        bdot = lambda u, v: sum((ui * vi).reshape(B, -1).sum(1) for ui, vi in zip(u, v))
        gv, _ = oracle_gn(c.cfg, c.prm, c.x, c.p, c.a, c.s, (r[0], r[1], None), None, float(B))
        q = [gv[k] + lm.reshape(B, 1, 1) * r[k] for k in range(2)]
        alpha = (bdot(r, r) / bdot(r, q)).reshape(B, 1, 1)
        return NS(y=y, rhs=r, lam=lm, x=[alpha * rk for rk in r])
    return _once(("cg", c.key, tuple(lam)), make)


# ---- the inner loop
def inner(c, S=2, Ns=24, lr_p=0.3, lr_a=2.0):
    """The problem of the inner-loop tests on c's grid: coords = c.x[0], the meta-init = signal 0's latents, targets = the oracle's
    decode of latents moved by 0.05 N(0, 1) in p and 0.5 N(0, 1) in a, learning rates (lr_p, lr_a per channel, 0 for the window).
    NS(coords, img, lat0, lrs, masks (Ns, S + 1), masks_b (B, Ns, S + 1), shared = (loss, fit), per_signal = (loss, fit)): the
    references are oracle.enf_ref_torch.inner_loop in fp64, for per-signal masks once per signal (tests/test_gpu_signal_masks.py)."""
    def make():
        rng = np.random.default_rng(53)
        B, N, Z = c.B, c.N, c.Z
        coords = c.x[0]
        lat0 = {"p_pos": c.p[:1], "a": c.a[:1], "gaussian_window": c.s[:1]}
        xb = np.repeat(coords[None], B, 0)
        img = f32(R.nef_apply(c.prm, c.cfg, xb, f32(np.repeat(c.p[:1], B, 0) + 0.05 * rng.standard_normal((B, Z, c.p.shape[-1]))),
                              f32(np.repeat(c.a[:1], B, 0) + 0.5 * rng.standard_normal((B, Z, c.C))), np.repeat(c.s[:1], B, 0)))
        masks = np.stack([rng.permutation(N)[:Ns] for _ in range(S + 1)], 1)
        masks_b = np.stack([np.stack([rng.permutation(N)[:Ns] for _ in range(S + 1)], 1) for _ in range(B)])
        lrs = {"p_pos": np.array([lr_p]), "a": np.full((c.C,), lr_a), "gaussian_window": np.array([0.0])}
        tp = T.to_torch(c.prm, torch.float64)
        tl = {k: torch.tensor(v) for k, v in lat0.items()}
        tr = {k: torch.tensor(v) for k, v in lrs.items()}
        n = lambda fit: {k: v.detach().numpy() for k, v in fit.items()}
        loss, fit = T.inner_loop(tp, c.cfg, tl, tr, torch.tensor(coords), torch.tensor(img), torch.tensor(masks))
        shared = (float(loss.detach()), n(fit))
        losses, fits = [], []
        for b in range(B):
            lb, fb = T.inner_loop(tp, c.cfg, tl, tr, torch.tensor(coords), torch.tensor(img[b:b + 1]), torch.tensor(masks_b[b]))
            losses.append(float(lb.detach()) / B)
            fits.append(n(fb))
        per_signal = (sum(losses), {k: np.concatenate([f[k] for f in fits], 0) for k in fits[0]})
        return NS(coords=coords, img=img, lat0=lat0, lrs=lrs, masks=masks, masks_b=masks_b, shared=shared, per_signal=per_signal, S=S)
    return _once(("inner", c.key, S, Ns, lr_p, lr_a), make)


def inner_cells(c, S=2, Ms=6, lr_p=0.3, lr_a=2.0):
    """inner_loop_cells on c's grid (N = M G rows, shared cells): NS(x, q, y, wt, lat0, lrs, masks (Ms, S + 1), ref = (loss, fit)) with
    tests/cells_train_ref.inner_loop_cells in fp64 as the reference"""
    def make():
        from tests.cells_train_ref import inner_loop_cells
        rng = np.random.default_rng(59)
        B, M = c.B, c.N // G
        x, q = c.x[0], f32(rng.uniform(0.2, 2.0, (c.N,)) / G)
        lat0 = {"p_pos": c.p[:1], "a": c.a[:1], "gaussian_window": c.s[:1]}
        out = R.nef_apply(c.prm, c.cfg, np.repeat(x[None], B, 0), f32(np.repeat(c.p[:1], B, 0) + 0.05 * rng.standard_normal((B, c.Z, c.p.shape[-1]))),
                          f32(np.repeat(c.a[:1], B, 0) + 0.5 * rng.standard_normal((B, c.Z, c.C))), np.repeat(c.s[:1], B, 0))
        y = f32((q[None, :, None] * out).reshape(B, M, G, c.O).sum(2))
        wt = f32(rng.uniform(0.2, 2.0, (B, M)))
        wt[rng.uniform(size=wt.shape) < 0.3] = 0.0
        masks = np.stack([rng.permutation(M)[:Ms] for _ in range(S + 1)], 1)
        lrs = {"p_pos": np.array([lr_p]), "a": np.full((c.C,), lr_a), "gaussian_window": np.array([0.0])}
        loss, fit = inner_loop_cells(T.to_torch(c.prm, torch.float64), c.cfg, {k: torch.tensor(v) for k, v in lat0.items()},
                                     {k: torch.tensor(v) for k, v in lrs.items()}, torch.tensor(x), torch.tensor(q), G, torch.tensor(y),
                                     torch.tensor(masks), torch.tensor(wt))
        return NS(x=x, q=q, y=y, wt=wt, lat0=lat0, lrs=lrs, masks=masks, ref=(float(loss.detach()), {k: v.detach().numpy() for k, v in fit.items()}))
    return _once(("inner_cells", c.key, S, Ms, lr_p, lr_a), make)


# ---- lifting: a dx-dimensional problem is the (dx + 1)-dimensional one whose extra coordinate is 0 in every x and p
def lift(c):
    """The lifted twin of c: cfg with num_in = dx + 1, x and p with a zero column appended, the same a, sigma and cotangent.
    norm_rel_pos has one invariant row whatever dx: the parameters are the same tensors.  rel_pos, abs_pos: one row N(0, freq) is appended
    to both RFF coefficient matrices; it multiplies the zero.  `out` is the oracle's, from the lifted problem itself."""
    def make():
        import copy
        dx = c.dx + 1
        cfg = make_cfg(c.inv, D=c.D, H=c.H, C=c.C, O=c.O, num_in=dx, freq=FREQ)
        prm = copy.deepcopy(c.prm)
        if c.inv != "norm_rel_pos":
            rng = np.random.default_rng(61)
            attn = prm["params"]["cross_attention_blocks_0"]["attn"]
            for branch, f in zip(("query", "value"), FREQ):
                enc = attn["invariant_embedding_" + branch]["encoding"]
                enc["coefficients"] = np.concatenate([enc["coefficients"], f * rng.standard_normal((1, c.D // 2))], 0)
                assert enc["coefficients"].shape == (dx, c.D // 2)
        pad = lambda v: np.concatenate([v, np.zeros(v.shape[:-1] + (1,))], -1)
        x, p = pad(c.x), pad(c.p)
        return NS(cfg=cfg, prm=prm, x=x, p=p, a=c.a, s=c.s, w=c.w, out=R.nef_apply(prm, cfg, x, p, c.a, c.s), key=("lift", c.key), inv=c.inv,
                  dx=dx, B=c.B, N=c.N, Z=c.Z, C=c.C, O=c.O, D=c.D, H=c.H)
    return _once(("lift", c.key), make)


# ---- group actions
def translation(dx):
    return np.array([0.37, -0.21, 0.55])[:dx]


def rotation():
    """a proper 3-D rotation: Rodrigues' formula about (1, 2, 3) / sqrt(14) by 0.9 rad"""
    k = np.array([1.0, 2.0, 3.0]) / np.sqrt(14.0)
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    Rm = np.eye(3) + np.sin(0.9) * K + (1 - np.cos(0.9)) * K @ K
    assert np.allclose(Rm @ Rm.T, np.eye(3), atol=1e-14) and abs(np.linalg.det(Rm) - 1) < 1e-14
    return Rm
