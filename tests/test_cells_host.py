"""Grouped observations without a GPU (include/enf_hip.h, "Grouped observations"): the yardstick itself (tests/cells_ref.py against
central differences, against the oracle's weighted loss at G = 1, and under poisoned targets), the quadrature rules of
fitting/cells.py, the header and the bindings, the refusals of enf_fit_step_g / enf_eval_loss_g (every call here fails its checks, so
nothing is launched) and the Python mirror's."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from enf_pde_amd import _lib
from enf_pde_amd.fitting import cell_quadrature, draw_cell_samples, fit_cell_averages
from tests.cells_ref import case, cell_loss, poisoned
from tests.gn_ref import oracle_loss_grad
from tests.helpers import build_nef, make_cfg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, EUNSUPPORTED, EWORKSPACE = -1, -3, -4
DET, SHARED = _lib.ENF_FIT_DETERMINISTIC, _lib.ENF_FIT_SHARED_LATENTS


# ---- 1. the yardstick
@pytest.mark.parametrize("inv,G,N", [("rel_pos_periodic", 4, 16), ("latitude_periodic", 2, 10)])
def test_reference_gradients_match_central_differences(inv, G, N):
    """d loss / d(p, a, sigma) along a random direction against (L(+h) - L(-h)) / 2h in fp64: h = 1e-6 leaves truncation ~ h^2 = 1e-12
    and rounding ~ 1e-16 / h = 1e-10 relative to the loss, so 1e-7 on the directional derivative (tests/test_gn_host.py)."""
    c = case(inv, G, N)
    rng = np.random.default_rng(3)
    v = [rng.standard_normal(u.shape) * sc for u, sc in zip((c.p, c.a, c.s), (0.3, 1.0, 0.1))]
    want = sum(float((gi * vi).sum()) for gi, vi in zip(c.ref.g, v)) / c.gs
    h = 1e-6
    f = lambda sg: cell_loss(c.cfg, c.prm, c.x, c.p + sg * h * v[0], c.a + sg * h * v[1], c.s + sg * h * v[2], c.y, G, c.q, c.w,
                             grads=False).loss
    cd = (f(1.0) - f(-1.0)) / (2 * h)
    print(inv, G, N, "directional derivative", want, "central difference", cd)
    assert abs(cd - want) <= 1e-7 * abs(want)


def test_group_of_one_with_unit_factors_is_the_weighted_loss():
    """G = 1, q = 1: the oracle's weighted mean squared error and its gradients (tests/gn_ref.py), to 1e-12"""
    c = case("rel_pos_periodic", 1, 11)
    ones = np.ones_like(c.q)
    for q in (ones, None):
        r = cell_loss(c.cfg, c.prm, c.x, c.p, c.a, c.s, c.y, 1, q, c.w, c.gs)
        lb, g = oracle_loss_grad(c.cfg, c.prm, c.x, c.p, c.a, c.s, c.y, c.w, c.gs)
        assert np.allclose(r.loss_b, lb, rtol=1e-12, atol=0) and abs(r.loss - lb.mean()) <= 1e-12 * lb.mean()
        for u, v in zip(r.g, g):
            assert np.linalg.norm(u - v) <= 1e-12 * np.linalg.norm(v)


def test_poisoned_targets_under_zero_weights_change_nothing():
    c = case("rel_pos_periodic", 4, 16)
    assert (c.w == 0).any()
    for kind in ("mixed", "inf"):
        y = poisoned(c, kind)
        assert not np.isfinite(y).all()
        r = cell_loss(c.cfg, c.prm, c.x, c.p, c.a, c.s, y, c.G, c.q, c.w, c.gs)
        assert r.loss == c.ref.loss and np.array_equal(r.err_g, c.ref.err_g) and np.array_equal(r.loss_b, c.ref.loss_b)
        assert all(np.array_equal(u, v) for u, v in zip(r.g, c.ref.g))
        assert (r.err_g[c.w == 0] == 0).all()


# ---- 2. the quadrature rules
def test_quadrature_weights_sum_to_one_and_points_lie_in_their_cells():
    edges = [np.array([-1.0, -0.2, 0.1, 1.0]), np.array([0.0, 0.5, 2.0])]
    for cells, kind in ((edges, "cartesian"), ((-1.0, 1.0, (3, 2)), "cartesian"), ([edges[0] + 1.0, edges[1] + 0.3], "sphere")):
        for k, rule in ((1, "gauss"), (2, "gauss"), (2, "midpoint"), (4, "midpoint")):
            x, q = cell_quadrature(cells, k, rule=rule, kind=kind, dtype=torch.float64)
            G = k * k
            assert x.shape == (6 * G, 2) and q.shape == (6 * G,) and bool((q > 0).all())
            assert torch.allclose(q.reshape(6, G).sum(1), torch.ones(6, dtype=torch.float64), rtol=1e-14, atol=0)
            if isinstance(cells, list):                 # cell m = (i, j) in C order owns rows m G ..
                xc = x.reshape(3, 2, G, 2)
                for i in range(3):
                    for j in range(2):
                        assert bool(((xc[i, j, :, 0] > cells[0][i]) & (xc[i, j, :, 0] < cells[0][i + 1])).all())
                        assert bool(((xc[i, j, :, 1] > cells[1][j]) & (xc[i, j, :, 1] < cells[1][j + 1])).all())
    x1, q1 = cell_quadrature([np.linspace(0, 1, 5)], 8, dtype=torch.float64)             # one axis: G = k
    assert x1.shape == (32, 1) and torch.allclose(q1.reshape(4, 8).sum(1), torch.ones(4, dtype=torch.float64))
    assert cell_quadrature((0.0, 1.0, 4), 2)[0].dtype == torch.float32


def test_gauss_rule_integrates_cubics_per_axis_exactly():
    """k = 2 Gauss-Legendre is exact to degree 3 per axis: the cell mean of x^3 y^3 + x^2 y - 2 y^3 + 1 against its antiderivative"""
    ex, ey = np.array([-1.0, -0.3, 0.4, 1.0]), np.array([0.2, 0.9, 1.0])
    x, q = cell_quadrature([ex, ey], 2, dtype=torch.float64)
    f = lambda u, v: u ** 3 * v ** 3 + u ** 2 * v - 2 * v ** 3 + 1
    got = (q * f(x[:, 0], x[:, 1])).reshape(6, 4).sum(1).numpy()
    mean = lambda e, n: (e[1:] ** (n + 1) - e[:-1] ** (n + 1)) / ((n + 1) * (e[1:] - e[:-1]))       # the mean of t^n over every cell
    want = (np.outer(mean(ex, 3), mean(ey, 3)) + np.outer(mean(ex, 2), mean(ey, 1)) - 2 * np.outer(mean(ex, 0), mean(ey, 3)) + 1).reshape(-1)
    assert np.allclose(got, want, rtol=1e-13, atol=1e-14)
    xm, qm = cell_quadrature([ex, ey], 2, rule="midpoint", dtype=torch.float64)          # (the midpoint rule is not)
    assert not np.allclose((qm * f(xm[:, 0], xm[:, 1])).reshape(6, 4).sum(1).numpy(), want, rtol=1e-6, atol=0)


def test_sphere_weights_match_the_area_integrals():
    """kind = "sphere": the factors carry sin(theta), normalised per cell.  Against fp64 cell integrals: the unnormalised Gauss factors
    half-width * w_k sin(theta_k) sum to cos(theta_0) - cos(theta_1), and the area mean of cos(theta) is (sin^2 theta_1 - sin^2
    theta_0) / (2 (cos theta_0 - cos theta_1)).  k = 4 Gauss points on cells of pi / 12: the rule's error is below
    (h / 2)^8 / 8! * 2 h of a unit-size eighth derivative, ~ 1e-12 relative; asserted at 1e-10."""
    phi, th = np.linspace(0, 2 * np.pi, 4), np.linspace(0.0, np.pi, 13)
    x, q = cell_quadrature([phi, th], 4, kind="sphere", dtype=torch.float64)
    x, q = x.reshape(3, 12, 16, 2).numpy(), q.reshape(3, 12, 16).numpy()
    area = np.cos(th[:-1]) - np.cos(th[1:])
    want = (np.sin(th[1:]) ** 2 - np.sin(th[:-1]) ** 2) / (2 * area)
    got = (q * np.cos(x[..., 1])).sum(-1)
    assert np.allclose(got, want[None].repeat(3, 0), rtol=0, atol=1e-10)
    # the theta factors alone: proportional to w_k sin(theta_k), summing to 1; their unnormalised sum is the cell's area integral
    t, w = np.polynomial.legendre.leggauss(4)
    for j in range(12):
        mid, half = 0.5 * (th[j] + th[j + 1]), 0.5 * (th[j + 1] - th[j])
        raw = half * w * np.sin(mid + half * t)
        assert abs(raw.sum() - area[j]) <= 1e-10 * area[j]
        assert np.allclose(q[0, j].reshape(4, 4).sum(0), raw / raw.sum(), rtol=1e-13, atol=0)
    xm, qm = cell_quadrature([phi, th], 2, rule="midpoint", kind="sphere", dtype=torch.float64)
    assert torch.allclose(qm.reshape(36, 4).sum(1), torch.ones(36, dtype=torch.float64), rtol=1e-14, atol=0)


def test_quadrature_refuses_group_sizes_the_tail_does_not_serve():
    for cells, k in (((0.0, 1.0, (2, 2)), 3), ((0.0, 1.0, (2, 2)), 5), ((0.0, 1.0, 4), 3), ((0.0, 1.0, 4), 32), ((0.0, 1.0, (2, 2, 2)), 3)):
        with pytest.raises(ValueError, match="serves"):
            cell_quadrature(cells, k)
    with pytest.raises(ValueError):
        cell_quadrature((0.0, 1.0, 4), 2, rule="simpson")
    with pytest.raises(ValueError):
        cell_quadrature((0.0, 1.0, 4), 2, kind="sphere")                 # one axis
    with pytest.raises(ValueError):
        cell_quadrature([np.array([0.0, 1.0, 0.5])], 2)                  # edges that do not increase
    with pytest.raises(ValueError):
        cell_quadrature((1.0, 0.0, 4), 2)
    assert cell_quadrature((0.0, 1.0, (2, 2, 2)), 2)[0].shape == (64, 3)  # G = 8


# ---- 3. header, exports, argument types
def test_symbols_header_and_abi():
    with open(os.path.join(ROOT, "include", "enf_hip.h")) as f:
        h = f.read()
    assert re.search(r"#define\s+ENF_ABI_VERSION\s+2\b", h)
    lib = _lib.load()
    assert lib.enf_abi_version() == 2
    for name in ("enf_fit_step_g", "enf_eval_loss_g"):
        assert re.search(rf"\bint\s+{name}\s*\(", h), name
        assert name in _lib.EXPORTS and hasattr(lib, name) and hasattr(_lib.load_test(), name)
    assert len(lib.enf_fit_step_g.argtypes) == 22 and lib.enf_fit_step_g.argtypes[8] is ctypes.c_int32
    assert lib.enf_fit_step_g.argtypes[11] is ctypes.c_float
    assert len(lib.enf_eval_loss_g.argtypes) == 18 and lib.enf_eval_loss_g.argtypes[8] is ctypes.c_int32
    assert "Grouped observations" in h and "ENF_FIT_SHARED_LATENTS is ENF_EINVAL" in h


# ---- 4. the refusals, without a launch
def _descs():
    dummy = ctypes.create_string_buffer(64)
    P = ctypes.cast(dummy, ctypes.c_void_p)
    mk = lambda N=48, O=2, window=1, B=3: _lib.make_desc(B, N, 7, 2, 64, 12, O, 2, 0, window, 0)
    return dummy, P, mk


def test_fit_step_g_refusals_and_their_order():
    lib = _lib.load()
    dummy, P, mk = _descs()
    big = 1 << 40

    def call(desc=None, x=P, p=P, a=P, sigma=P, blob=P, y=P, G=4, q=P, w=P, loss=P, dp=P, da=P, ds=P, err=P, lb=P, ws=P, nbytes=big, flags=0,
             xb=0):
        desc = mk() if desc is None else desc
        return lib.enf_fit_step_g(ctypes.byref(desc), x, xb, p, a, sigma, blob, y, G, q, w, 1.0, loss, dp, da, ds, err, lb, ws, nbytes, flags, None)
    # the descriptor's own error comes first, whatever else is wrong
    assert call(desc=mk(O=33)) == EUNSUPPORTED
    assert call(desc=mk(O=33), G=3, y=None, flags=SHARED, nbytes=0) == EUNSUPPORTED
    bad_dim = _lib.make_desc(3, 48, 7, 2, 64, 12, 2, 3, 0, 1, 0)            # rel_pos_periodic with three coordinates
    assert call(desc=bad_dim, G=5, x=None) == -6
    # G outside the set, N % G != 0 -- before the workspace size is looked at
    for G in (0, -1, 3, 5, 6, 7, 12, 32, 64):
        assert call(G=G) == EINVAL and call(G=G, nbytes=0) == EINVAL, G
    for G in (1, 2, 4, 8, 16):
        assert call(G=G, nbytes=0) == EWORKSPACE, G                          # legal: the next check is the workspace's
    assert call(desc=mk(N=50), G=4, nbytes=0) == EINVAL and call(desc=mk(N=50), G=16, nbytes=0) == EINVAL
    assert call(desc=mk(N=50), G=2, nbytes=0) == EWORKSPACE
    # NULL target and the other required pointers; q, w, err_g, loss_b are optional
    for k in ("y", "x", "p", "a", "sigma", "blob", "loss", "dp", "da", "ds", "ws"):
        assert call(**{k: None}, nbytes=0) == EINVAL, k
    assert call(q=None, w=None, err=None, lb=None, nbytes=0) == EWORKSPACE
    assert call(err=None, lb=P, nbytes=0) == EINVAL                          # loss_b needs err_g in the fit step
    assert call(desc=mk(window=0), sigma=None, nbytes=0) == EWORKSPACE
    # flags: 0 or ENF_FIT_DETERMINISTIC; the shared-latent permission is refused, with and without a batch stride
    assert call(flags=SHARED, nbytes=0) == EINVAL and call(flags=SHARED | DET, nbytes=0) == EINVAL and call(flags=SHARED, xb=96) == EINVAL
    assert call(desc=mk(B=1), flags=SHARED, nbytes=0) == EINVAL
    for flags in (1, 2, 4, 8, 32, 64, DET | 2):
        assert call(flags=flags, nbytes=0) == EINVAL, flags
    # the workspace sizes are those of enf_fit_step_w
    d = mk()
    for flags in (0, DET):
        need = lib.enf_workspace_bytes_ex(ctypes.byref(d), flags)
        assert call(flags=flags, nbytes=need - 1) == EWORKSPACE
    assert call(flags=DET, nbytes=lib.enf_workspace_bytes_ex(ctypes.byref(d), 0)) == EWORKSPACE


def test_eval_loss_g_refusals_and_their_order():
    lib = _lib.load()
    dummy, P, mk = _descs()
    big = 1 << 40

    def call(desc=None, x=P, p=P, a=P, sigma=P, blob=P, y=P, G=4, q=P, w=P, loss=P, err=P, lb=P, ws=P, nbytes=big, flags=0):
        desc = mk() if desc is None else desc
        return lib.enf_eval_loss_g(ctypes.byref(desc), x, 0, p, a, sigma, blob, y, G, q, w, loss, err, lb, ws, nbytes, flags, None)
    assert call(desc=mk(O=33)) == EUNSUPPORTED and call(desc=mk(O=33), G=3, y=None, loss=None, err=None, lb=None) == EUNSUPPORTED
    for G in (0, -4, 3, 6, 17, 32):
        assert call(G=G, nbytes=0) == EINVAL, G
    for G in (1, 2, 4, 8, 16):
        assert call(G=G, nbytes=0) == EWORKSPACE, G
    assert call(desc=mk(N=50), G=4, nbytes=0) == EINVAL and call(desc=mk(N=50), G=2, nbytes=0) == EWORKSPACE
    for k in ("y", "x", "p", "a", "sigma", "blob", "ws"):
        assert call(**{k: None}, nbytes=0) == EINVAL, k
    assert call(loss=None, err=None, lb=None, nbytes=0) == EINVAL            # all three outputs NULL
    for kw in ({"loss": None}, {"err": None}, {"lb": None}, {"loss": None, "err": None}, {"err": None, "lb": None}, {"q": None, "w": None}):
        assert call(**kw, nbytes=0) == EWORKSPACE, kw                        # every output alone is legal, loss_b without err_g too
    for flags in (1, 2, 8, 32, SHARED, SHARED | DET):
        assert call(flags=flags, nbytes=0) == EINVAL, flags
    d = mk()
    for flags in (0, DET):
        assert call(flags=flags, nbytes=lib.enf_workspace_bytes_ex(ctypes.byref(d), flags) - 1) == EWORKSPACE


# ---- 5. the Python mirror's refusals: shapes are checked before anything touches the device
def test_python_mirror_checks_shapes_first():
    from tests.test_gpu_layers import _nef as layered
    Bn, N, Zn, G = 2, 8, 3, 4
    x, p, a, s = torch.zeros(Bn, N, 2), torch.zeros(Bn, Zn, 2), torch.ones(Bn, Zn, 8), torch.ones(Bn, Zn, 1)
    y = torch.zeros(Bn, N // G, 2)
    nef = build_nef(make_cfg("rel_pos_periodic", D=64, H=2, C=8, O=2), "f32")
    deep = layered(dict(make_cfg("rel_pos_periodic", D=64, H=2, C=8, O=2), num_layers=1), "f32")
    for fn, dfn in ((nef.mse_value_and_cell_grads, deep.mse_value_and_cell_grads), (nef.eval_cell_loss, deep.eval_cell_loss)):
        with pytest.raises(NotImplementedError, match="num_layers"):
            dfn(None, x, p, a, s, y, G)
        for bad in (3, 0, 32, 5):
            with pytest.raises(ValueError, match="group"):
                fn(None, x, p, a, s, y, bad)
        with pytest.raises(ValueError, match="multiple"):
            fn(None, x[:, :7], p, a, s, y, G)
        with pytest.raises(ValueError, match="target"):
            fn(None, x, p, a, s, torch.zeros(Bn, N, 2), G)
        with pytest.raises(ValueError, match="qweight"):
            fn(None, x, p, a, s, y, G, qweight=torch.ones(Bn, N // G))
        with pytest.raises(ValueError, match="obs_weight"):
            fn(None, x, p, a, s, y, G, obs_weight=torch.ones(Bn, N))
        with pytest.raises(_lib.EnfError):                                   # host tensors: there is no CPU path
            fn(None, x, p, a, s, y, G)
    lat0 = {"p_pos": p[:1], "a": a[:1], "gaussian_window": s[:1]}
    with pytest.raises(ValueError, match="group"):
        fit_cell_averages(nef, None, lat0, None, x[0], None, 3, y, 1)
    with pytest.raises(ValueError, match="cells"):
        fit_cell_averages(nef, None, lat0, None, x[0], None, 2, y, 1)
    with pytest.raises(ValueError, match="obs_weight"):
        fit_cell_averages(nef, None, lat0, None, x[0], None, G, y, 1, obs_weight=torch.ones(Bn, N))
    with pytest.raises(ValueError, match="sample"):
        fit_cell_averages(nef, None, lat0, None, x[0], None, G, y, 1, sample=3)
    idx = draw_cell_samples(10, 4, 2, generator=torch.Generator().manual_seed(1))
    assert idx.shape == (3, 4) and idx.dtype == torch.int64 and all(len(set(r.tolist())) == 4 for r in idx) and int(idx.max()) < 10
    assert torch.equal(idx, draw_cell_samples(10, 4, 2, generator=torch.Generator().manual_seed(1)))
