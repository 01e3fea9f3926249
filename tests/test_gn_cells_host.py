"""The Gauss-Newton product on grouped observations without a GPU (include/enf_hip.h, "Gauss-Newton product on grouped observations"):
the yardstick itself (tests/gn_cells_ref.py: symmetry, the central difference of the grouped loss's gradients at zero residual, G = 1
against the per-point yardstick), the header and the binding, the refusals of enf_gn_product_g and their order (every call here fails
its checks, so nothing is launched), the Python mirror's refusals, and the call sequences of lm_fit_cell_averages and lm_fit_latents
against a stand-in model that records them."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from enf_pde_amd import _lib
from tests.helpers import make_cfg, build_nef
from tests import cells_ref, gn_ref
from tests.gn_cells_ref import case, oracle_gn_cells
from tests.test_gn_host import _LinearNef, _cg_update_torch, _descs, _dot

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, EUNSUPPORTED, EWORKSPACE = -1, -3, -4
DET, REUSE = _lib.ENF_BWD_DETERMINISTIC, _lib.ENF_GN_REUSE_POINT


# ---- 1. the yardstick
@pytest.mark.parametrize("inv,G,N,h", [("rel_pos_periodic", 4, 80, 1e-7), ("latitude_periodic", 2, 50, 1e-6), ("ponita", 16, 48, 1e-6)])
def test_reference_product_is_symmetric_and_matches_the_gradient_difference(inv, G, N, h):
    """The bounds of tests/test_gn_host.py for the per-point yardstick: G = coef Jg^T W Jg is symmetric and equals its quadratic form up
    to fp64 summation (1e-12), and at zero residual (target = obs) it IS the Hessian of the grouped loss, so G v equals the central
    difference of cells_ref.cell_loss's gradients along v (h = 1e-6: 1e-7, the argument is there).  The difference assumes that no relu
    of the query branch changes sign between the two points.  In the (4, 80) case one does within 1e-6 |v| -- its error is 1.2e-4 at
    h = 1e-6 and 1.4e-9 at h = 1e-7, a jump no truncation term makes -- so that case steps by 1e-7: truncation ~ 1e-14, rounding
    ~ 1e-16 / h = 1e-9, the bound stays 1e-7."""
    c = case(inv, G, N)
    rng = np.random.default_rng(13)
    u = tuple(rng.standard_normal(t.shape) * sc for t, sc in zip(c.v, (0.3, 1.0, 0.1)))
    Gv, obs_tan = c.ref, c.obs_tan
    Gu = oracle_gn_cells(c.cfg, c.prm, c.x, c.p, c.a, c.s, u, G, c.q, c.w, c.gs)[0]
    e_sym = abs(_dot(u, Gv) - _dot(Gu, c.v)) / abs(_dot(u, Gv))
    coef = c.gs * 2.0 / (3 * c.M * c.O)
    quad = coef * float((c.w[..., None] * obs_tan ** 2).sum())
    e_quad = abs(_dot(c.v, Gv) - quad) / quad
    obs = cells_ref.cell_loss(c.cfg, c.prm, c.x, c.p, c.a, c.s, np.zeros((3, c.M, c.O)), G, c.q, grads=False).obs
    grad = lambda sg: cells_ref.cell_loss(c.cfg, c.prm, c.x, c.p + sg * h * c.v[0], c.a + sg * h * c.v[1], c.s + sg * h * c.v[2], obs, G,
                                          c.q, c.w, c.gs).g
    cd = [(a_ - b_) / (2 * h) for a_, b_ in zip(grad(1.0), grad(-1.0))]
    e_cd = float(np.sqrt(sum(((d - g) ** 2).sum() for d, g in zip(cd, Gv))) / np.sqrt(sum((g ** 2).sum() for g in Gv)))
    print(f"{inv} G={G} N={N} h={h:.0e}: symmetry {e_sym:.2e}, quadratic form {e_quad:.2e}, central difference of the gradients {e_cd:.2e}")
    assert _dot(c.v, Gv) > 0 and e_sym < 1e-12 and e_quad < 1e-12 and e_cd < 1e-7


def test_reference_product_with_groups_of_one_is_the_per_point_product():
    """G = 1, q = 1: Jg = J and the observation weights are point weights -- oracle_gn(w = (B, N)) of tests/gn_ref.py, to fp64 rounding"""
    c = case("rel_pos_periodic", 1, 50)
    ones = np.ones((3, 50))
    for q in (ones, None):
        got = oracle_gn_cells(c.cfg, c.prm, c.x, c.p, c.a, c.s, c.v, 1, q, c.w, c.gs)[0]
        want = gn_ref.oracle_gn(c.cfg, c.prm, c.x, c.p, c.a, c.s, c.v, c.w, c.gs)[0]
        for g, r in zip(got, want):
            assert cells_ref.rel(g, r) < 1e-13
    assert (c.w == 0).any()


# ---- 2. header, export, argument types
def test_symbol_header_and_binding():
    with open(os.path.join(ROOT, "include", "enf_hip.h")) as f:
        h = f.read()
    assert re.search(r"#define\s+ENF_ABI_VERSION\s+2\b", h)
    lib = _lib.load()
    assert lib.enf_abi_version() == 2
    assert re.search(r"\bint\s+enf_gn_product_g\s*\(", h)
    assert "enf_gn_product_g" in _lib.EXPORTS and hasattr(lib, "enf_gn_product_g") and hasattr(_lib.load_test(), "enf_gn_product_g")
    at = lib.enf_gn_product_g.argtypes
    assert len(at) == 21 and at[2] is ctypes.c_int64 and at[10] is ctypes.c_int32 and at[13] is ctypes.c_float
    assert at[18] is ctypes.c_size_t and at[19] is ctypes.c_uint
    assert all(at[i] is ctypes.c_void_p for i in (1, 3, 4, 5, 6, 7, 8, 9, 11, 12, 14, 15, 16, 17, 20))
    # the declaration's parameters, in order
    decl = re.sub(r"/\*.*?\*/", "", h[h.index("int enf_gn_product_g("):].split(";")[0], flags=re.S)
    names = [a.split()[-1].lstrip("*") for a in decl[decl.index("(") + 1:decl.rindex(")")].split(",")]
    assert names == ["d", "x", "x_bstride", "p", "a", "sigma", "vp", "va", "vsigma", "packed", "G", "qweight", "oweight", "grad_scale",
                     "gp", "ga", "gsigma", "workspace", "workspace_bytes", "flags", "stream"]
    assert "enf_gn_product_g" in h[h.index("ENF_GN_REUSE_POINT --"):h.index("#define ENF_GN_REUSE_POINT")]      # the flag's statement


# ---- 3. the refusals and their order, without a launch
def test_gn_product_g_error_order_without_a_launch():
    lib = _lib.load()
    dummy, P, mk0, unserved = _descs()
    mk = lambda N=80, **kw: _with_n(mk0(**kw), N)
    d = mk()
    big = 1 << 40

    def call(desc=d, x=P, p=P, a=P, sigma=P, vp=P, va=P, vs=P, blob=P, G=4, q=P, w=P, gp=P, ga=P, gs=P, ws=P, nbytes=big, flags=0):
        return lib.enf_gn_product_g(ctypes.byref(desc), x, 0, p, a, sigma, vp, va, vs, blob, G, q, w, 1.0, gp, ga, gs, ws, nbytes, flags, None)
    # 1. the descriptor's own error comes first, whatever else is wrong
    assert call(desc=mk(O=33)) == EUNSUPPORTED and call(desc=mk(O=33), gp=None, flags=2, G=3) == EUNSUPPORTED
    bad_dim = _lib.make_desc(2, 80, 9, 2, 128, 16, 2, 3, 0, 1, 0)            # rel_pos_periodic with three coordinates
    assert call(desc=bad_dim, x=None, G=3) == -6
    # 2. what the call does not serve, before any pointer or the group size is looked at
    for bad in unserved:
        assert call(desc=bad) == EUNSUPPORTED
        assert call(desc=bad, gp=None, vp=None, va=None, vs=None, flags=2, nbytes=0, G=3) == EUNSUPPORTED
    # 3. ENF_EINVAL: what enf_gn_product refuses, and the group size -- before the workspace size
    for k in ("x", "p", "a", "sigma", "blob", "gp", "ga", "gs", "ws"):
        assert call(**{k: None}) == EINVAL and call(**{k: None}, nbytes=0) == EINVAL, k
    assert call(desc=mk(window=0), sigma=None, nbytes=0) == EWORKSPACE     # sigma is required with a window only
    assert call(vp=None, va=None, vs=None, nbytes=0) == EINVAL
    for flags in (2, 4, 8, 32, 64, 128, DET | 2):
        assert call(flags=flags, nbytes=0) == EINVAL, flags
    for G in (0, -1, -4, 3, 5, 6, 12, 32, 80):
        assert call(G=G) == EINVAL and call(G=G, nbytes=0) == EINVAL, G
    assert call(desc=mk(N=50), G=4) == EINVAL and call(desc=mk(N=50), G=4, nbytes=0) == EINVAL      # N % G != 0
    assert call(desc=mk(N=50), G=2, nbytes=0) == EWORKSPACE and call(desc=mk(N=72), G=16, nbytes=0) == EINVAL
    # 4. ENF_EWORKSPACE, for every legal group size, combination of tangents, factors, weights and flags
    for flags in (0, DET, REUSE, DET | REUSE):
        need = lib.enf_gn_workspace_bytes(ctypes.byref(d), flags)
        for kw in ({}, {"vp": None}, {"vp": None, "va": None}, {"q": None}, {"w": None}, {"q": None, "w": None}):
            for G in (1, 2, 4, 8, 16):
                assert call(flags=flags, nbytes=need - 1, G=G, **kw) == EWORKSPACE, (flags, kw, G)
    assert call(flags=DET, nbytes=lib.enf_gn_workspace_bytes(ctypes.byref(d), 0)) == EWORKSPACE


def _with_n(desc, N):
    desc.N = N
    return desc


# ---- 4. the Python mirror's refusals
def test_python_mirror_refuses_what_it_does_not_serve():
    from tests.test_gpu_layers import _nef as layered
    from tests.ffn_ref import build_nef_ffn
    B, N, Z = 2, 8, 3
    x, p, a, s = torch.zeros(B, N, 2), torch.zeros(B, Z, 2), torch.ones(B, Z, 8), torch.ones(B, Z, 1)
    va = torch.zeros_like(a)
    nef = layered(dict(make_cfg("rel_pos_periodic", D=64, H=2, C=8, O=2), num_layers=1), "f32")
    with pytest.raises(NotImplementedError, match="num_layers"):
        nef.gn_cell_product(None, x, p, a, s, 4, va=va)
    with pytest.raises(NotImplementedError, match="ffn"):
        build_nef_ffn(make_cfg("rel_pos_periodic", D=64, H=2, C=8, O=2), "f32").gn_cell_product(None, x, p, a, s, 4, va=va)
    for inv in ("ball", "ball_lat"):
        with pytest.raises(NotImplementedError, match=inv):
            build_nef(make_cfg(inv, D=64, H=2, C=8, O=2), "f32").gn_cell_product(None, torch.zeros(B, N, 3), torch.zeros(B, Z, 4), a, s, 4, va=va)
    flat = build_nef(make_cfg("rel_pos_periodic", D=64, H=2, C=8, O=2), "f32")
    with pytest.raises(ValueError, match="at least one"):
        flat.gn_cell_product(None, x, p, a, s, 4)                           # all three directions None
    for group in (0, 3, 5, 32):
        with pytest.raises(ValueError, match="group must be"):
            flat.gn_cell_product(None, x, p, a, s, group, va=va)
    with pytest.raises(ValueError, match="not a multiple"):
        flat.gn_cell_product(None, x, p, a, s, 16, va=va)                   # N % group != 0
    for bad in (torch.ones(B, N // 4), torch.ones(N), torch.ones(B, N, 1)):
        with pytest.raises(ValueError, match="qweight"):
            flat.gn_cell_product(None, x, p, a, s, 4, qweight=bad, va=va)
    for bad in (torch.ones(B, N), torch.ones(N // 4), torch.ones(B, N // 4, 1)):
        with pytest.raises(ValueError, match="obs_weight"):
            flat.gn_cell_product(None, x, p, a, s, 4, obs_weight=bad, va=va)
    with pytest.raises(_lib.EnfError):                                     # host tensors: there is no CPU path
        flat.gn_cell_product(None, x, p, a, s, 4, qweight=torch.ones(B, N), obs_weight=torch.ones(B, N // 4), va=va)
    from enf_pde_amd.fitting import lm_fit_cell_averages
    with pytest.raises(ValueError):
        lm_fit_cell_averages(flat, None, x, None, 4, torch.zeros(B, N // 4, 2), p, a, s, 1, components=("p", "q"))
    with pytest.raises(ValueError):
        lm_fit_cell_averages(flat, None, x, None, 4, torch.zeros(B, N // 4, 2), p, a, None, 1, components=("window",))


# ---- 5. the call sequences of both front ends of the LM loop
class _LinearCellNef(_LinearNef):
    """_LinearNef of tests/test_gn_host.py observed through groups: obs[b,m] = sum_k q[b, m G + k] out[b, m G + k], so Jg = Q A with Q
    the (M O) x (N O) matrix of the factors and G = 2 / (M O) (Q A)^T W (Q A) exactly.  N = 12 here, G = 4; records every call."""
    N, GROUP = 12, 4

    def _obs(self, out, q):
        B, N, O = out.shape
        qb = torch.full((B, N), 1.0 / self.GROUP) if q is None else q
        return (qb[..., None] * out).reshape(B, N // self.GROUP, self.GROUP, O).sum(2), qb

    def _jt(self, res, qb):
        """A^T Q^T res: res (B, M, O) back to the rows, times the factors, through A"""
        rows = qb[..., None] * res.repeat_interleave(self.GROUP, dim=1)
        return torch.einsum("bij,bi->bj", self.A, rows.reshape(self.B, -1))

    def mse_value_and_cell_grads(self, params, x, p, a, window, target, group, qweight=None, obs_weight=None, grad_scale=1.0,
                                 return_errors=False):
        assert return_errors and window is None and group == self.GROUP and tuple(x.shape) == (self.B, self.N, 2)
        obs, qb = self._obs(self.out(p, a), qweight)
        M = self.N // self.GROUP
        w = torch.ones(self.B, M) if obs_weight is None else obs_weight
        res = obs - target
        err = w * (res ** 2).sum(2)
        g = grad_scale / self.B * 2.0 / (M * self.O) * self._jt(w[..., None] * res, qb)
        self._touch()
        self.log.append(("cell_fit", grad_scale, x.stride(0), None if qweight is None else tuple(qweight.shape)))
        lb = err.sum(1) / (M * self.O)
        return (lb.mean().reshape(1), *self._split(g), None, err, lb)

    def gn_cell_product(self, params, x, p, a, window, group, qweight=None, obs_weight=None, vp=None, va=None, vwindow=None, grad_scale=1.0,
                        reuse=None):
        assert group == self.GROUP
        self.log.append(("cell_gn", vp is None, va is None, vwindow is None, reuse == self.workspace_tag(None)))
        v = self._z(torch.zeros(self.B, self.Z, self.WP) if vp is None else vp, torch.zeros(self.B, self.Z, self.WA) if va is None else va)
        tan = torch.einsum("bij,bj->bi", self.A, v).reshape(self.B, self.N, self.O)
        obs_tan, qb = self._obs(tan, qweight)
        M = self.N // self.GROUP
        w = torch.ones(self.B, M) if obs_weight is None else obs_weight
        g = grad_scale / self.B * 2.0 / (M * self.O) * self._jt(w[..., None] * obs_tan, qb)
        self._touch()
        return (*self._split(g), None)

    def eval_cell_loss(self, params, x, p, a, window, target, group, qweight=None, obs_weight=None):
        self._touch()
        self.log.append(("cell_eval",))
        obs, _ = self._obs(self.out(p, a), qweight)
        M = self.N // self.GROUP
        w = torch.ones(self.B, M) if obs_weight is None else obs_weight
        err = w * ((obs - target) ** 2).sum(2)
        return err.sum(1) / (M * self.O), err


def test_lm_front_ends_issue_their_call_sequences(monkeypatch):
    from enf_pde_amd.fitting import gauss_newton as GN
    monkeypatch.setattr(GN, "_cg_update", _cg_update_torch)
    B = 3
    nef = _LinearCellNef(B)
    g = torch.Generator().manual_seed(5)
    n = nef.Z * (nef.WP + nef.WA)
    M = nef.N // nef.GROUP
    p0, a0 = torch.randn((B, nef.Z, nef.WP), generator=g), torch.randn((B, nef.Z, nef.WA), generator=g)
    ps, as_ = p0 + 0.3 * torch.randn(p0.shape, generator=g), a0 + 0.3 * torch.randn(a0.shape, generator=g)
    q = torch.rand((nef.N,), generator=g) + 0.2
    w = torch.rand((B, M), generator=g) + 0.2
    x = torch.zeros(nef.N, 2)                                   # (N, dx) and q (N,): shared cells, expanded with stride 0
    target, _ = nef._obs(nef.out(ps, as_), q[None].expand(B, -1))
    # the cell front end: reserve, then per step one grouped fit step at gradient scale B, cg_iters grouped products that reuse its
    # point, one grouped evaluation.  M O = 6 observations for n = 15 unknowns per signal: G + lam I has at most 7 distinct eigenvalues,
    # so 8 CG iterations solve the damped system and one step fits the linear model up to (lam / sigma^2)^2 and fp32 rounding.
    (p1, a1, w1), loss_b, lam1, acc = GN.lm_fit_cell_averages(nef, None, x, q, nef.GROUP, target, p0, a0, None, steps=2, cg_iters=8,
                                                             damping=1e-6, obs_weight=w)
    assert w1 is None and loss_b.shape == (3, B) and acc.shape == (2, B) and acc.dtype == torch.bool and lam1.shape == (B,)
    assert bool(acc[0].all()) and bool((loss_b[1] < 1e-3 * loss_b[0]).all()) and bool((loss_b[2] <= loss_b[1]).all())
    assert nef.log[0] == ("reserve", B, nef.N, nef.Z)
    step = [("cell_fit", float(B), 0, (B, nef.N))] + [("cell_gn", False, False, True, True)] * 8 + [("cell_eval",)]
    assert nef.log[1:] == step * 2
    # q = None, x (B, N, dx), one component: the unused one passes None and stays
    nef.log.clear()
    tgt0, _ = nef._obs(nef.out(ps, as_), None)
    (p2, a2, _), lb2, _, acc2 = GN.lm_fit_cell_averages(nef, None, x[None].repeat(B, 1, 1), None, nef.GROUP, tgt0, p0, a0, None, steps=1,
                                                        cg_iters=4, components=("a",))
    assert torch.equal(p2, p0) and not torch.equal(a2, a0) and bool(acc2.all()) and bool((lb2[1] < lb2[0]).all())
    assert nef.log[1] == ("cell_fit", float(B), nef.N * 2, None)
    assert [e[0] for e in nef.log] == ["reserve", "cell_fit"] + ["cell_gn"] * 4 + ["cell_eval"]
    assert all(e[1:] == (True, False, True, True) for e in nef.log if e[0] == "cell_gn")
    # steps = 0: one evaluation and nothing else
    nef.log.clear()
    _, lb0, _, acc0 = GN.lm_fit_cell_averages(nef, None, x, q, nef.GROUP, target, p0, a0, None, steps=0)
    assert lb0.shape == (1, B) and acc0.shape == (0, B) and [e[0] for e in nef.log] == ["reserve", "cell_eval"]
    # the per-point front end issues what it issued: reserve, fit step, products with the point reused, evaluation
    nef.log.clear()
    tp = nef.out(ps, as_)
    xb = torch.zeros(B, nef.N, 2)
    _, lbp, _, accp = GN.lm_fit_latents(nef, None, xb, tp, p0, a0, None, steps=2, cg_iters=2 * n, damping=1e-6)
    assert nef.log[0] == ("reserve", B, nef.N, nef.Z)
    assert nef.log[1:] == ([("fit", float(B))] + [("gn", False, False, True, True)] * (2 * n) + [("eval",)]) * 2
    assert bool(accp[0].all()) and bool((lbp[1] < 1e-6 * lbp[0]).all())
