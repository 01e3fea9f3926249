"""The Gauss-Newton product and the batched CG step without a GPU (include/enf_hip.h, "Gauss-Newton product"): the yardstick itself
(symmetry, the quadratic form, and the central difference of the oracle's loss gradients at zero residual), the header and the
bindings, the size query, the argument checks of enf_gn_product and enf_cg_update (every call here fails its checks, so nothing is
launched), the Python mirror's refusals, and cg_solve / lm_fit_latents against a stand-in model with a known linear Jacobian (the CG
step itself replaced by the same arithmetic in torch: the kernel is tested on the GPU)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from enf_pde_amd import _lib
from oracle import enf_ref_torch as T
from tests.helpers import make_cfg, build_nef
from tests.gn_ref import case, oracle_gn, oracle_loss_grad, weights

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, EUNSUPPORTED, EWORKSPACE = -1, -3, -4
DET, REUSE = _lib.ENF_BWD_DETERMINISTIC, _lib.ENF_GN_REUSE_POINT


def _dot(u, v):
    return float(sum((ui * vi).sum() for ui, vi in zip(u, v)))


# ---- 1. the yardstick
@pytest.mark.parametrize("inv", ["rel_pos_periodic", "ponita", "latitude_periodic"])
def test_reference_product_is_symmetric_matches_its_quadratic_form_and_the_gradient_difference(inv):
    """Exact identities of  G = coef J^T W J  up to fp64 summation (1e-12), and at zero residual (target = out) the Gauss-Newton matrix
    IS the Hessian of the loss, so G v equals the central difference of the loss gradients along v: h = 1e-6 leaves truncation
    ~ h^2 = 1e-12 and rounding ~ 1e-16 / h = 1e-10 relative (tests/test_tangent_host.py has the argument for the small step): 1e-7."""
    cfg, prm, (x, p, a, s), v = case(inv)[:4]
    w = weights((3, 50))
    rng = np.random.default_rng(13)
    u = tuple(rng.standard_normal(t.shape) * sc for t, sc in zip(v, (0.3, 1.0, 0.1)))
    gs = 3.0
    coef = gs * 2.0 / (3 * 50 * 2)
    Gv, tan_v = oracle_gn(cfg, prm, x, p, a, s, v, w, gs)
    Gu, _ = oracle_gn(cfg, prm, x, p, a, s, u, w, gs)
    e_sym = abs(_dot(u, Gv) - _dot(Gu, v)) / abs(_dot(u, Gv))
    quad = coef * float((w[..., None] * tan_v ** 2).sum())
    e_quad = abs(_dot(v, Gv) - quad) / quad
    tp = T.to_torch(prm, torch.float64)
    with torch.no_grad():
        out = T.nef_apply(tp, cfg, torch.tensor(x), torch.tensor(p), torch.tensor(a), torch.tensor(s)).numpy()
    h = 1e-6
    hi = oracle_loss_grad(cfg, prm, x, p + h * v[0], a + h * v[1], s + h * v[2], out, w, gs)[1]
    lo = oracle_loss_grad(cfg, prm, x, p - h * v[0], a - h * v[1], s - h * v[2], out, w, gs)[1]
    cd = [(a_ - b_) / (2 * h) for a_, b_ in zip(hi, lo)]
    e_cd = float(np.sqrt(sum(((c - g) ** 2).sum() for c, g in zip(cd, Gv))) / np.sqrt(sum((g ** 2).sum() for g in Gv)))
    print(f"{inv}: symmetry {e_sym:.2e}, quadratic form {e_quad:.2e}, central difference of the gradients {e_cd:.2e}")
    assert _dot(v, Gv) > 0 and e_sym < 1e-12 and e_quad < 1e-12 and e_cd < 1e-7


# ---- 2. header, exports, argument types
def test_symbols_header_and_abi():
    with open(os.path.join(ROOT, "include", "enf_hip.h")) as f:
        h = f.read()
    assert re.search(r"#define\s+ENF_ABI_VERSION\s+2\b", h)
    lib = _lib.load()
    assert lib.enf_abi_version() == 2
    for name in ("enf_gn_workspace_bytes", "enf_gn_product", "enf_cg_update"):
        assert re.search(rf"\b(int|size_t)\s+{name}\s*\(", h), name
        assert name in _lib.EXPORTS and hasattr(lib, name) and hasattr(_lib.load_test(), name)
        assert getattr(lib, name).argtypes is not None, name
    assert len(lib.enf_gn_product.argtypes) == 20 and lib.enf_gn_product.argtypes[12] is ctypes.c_float
    assert lib.enf_gn_workspace_bytes.restype is ctypes.c_size_t
    assert len(lib.enf_cg_update.argtypes) == 7
    assert int(re.search(r"#define\s+ENF_GN_REUSE_POINT\s+(\d+)u", h).group(1)) == REUSE and not (REUSE & DET)
    # the segment struct field by field
    body = h[h.index("typedef struct EnfCgSegment {"):h.index("} EnfCgSegment;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for kind, names in re.findall(r"\b(const float\*|float\*|int32_t)\s+([^;]+);", body):
        fields += [(n.strip(), kind) for n in names.split(",")]
    assert [n for n, _ in fields] == [f[0] for f in _lib.EnfCgSegment._fields_] == ["x", "r", "d", "q", "width", "reserved"]
    assert ctypes.sizeof(_lib.EnfCgSegment) == 4 * 8 + 8 and _lib.ENF_CG_MAX_SEGMENTS == 3
    assert "Gauss-Newton product" in h and "FROZEN" in h and "each may be NULL" in h


# ---- 3. + 4. the size query and the error order, without a launch
def _descs():
    dummy = ctypes.create_string_buffer(64)
    P = ctypes.cast(dummy, ctypes.c_void_p)
    mk = lambda inv=0, O=2, window=1, emb=0, D=128, H=2: _lib.make_desc(2, 70, 9, H, D, 16, O, 2 if inv < 7 else 3, inv, window, 0, embedding=emb)
    masked = mk()
    masked.relu_masks, masked.mask_mode, masked.mask_signals = P.value, _lib.MASK_MODE["read"], 2
    unserved = (mk(inv=7, D=64), mk(inv=8, D=64), mk(inv=9), mk(emb=1), masked)      # ball, ball_lat, ponita_full, ffn, masks
    return dummy, P, mk, unserved


def test_workspace_size_query():
    lib = _lib.load()
    dummy, P, mk, unserved = _descs()
    size = lambda desc, flags=0: lib.enf_gn_workspace_bytes(ctypes.byref(desc), flags)
    for d in (mk(), mk(D=64, H=4), mk(window=0)):
        for flags in (0, DET, REUSE, DET | REUSE):
            n = size(d, flags)
            assert n >= lib.enf_workspace_bytes_ex(ctypes.byref(d), flags & DET) > 0
            assert n >= lib.enf_field_tangent_workspace_bytes(ctypes.byref(d)) > 0
            assert n == size(d, flags & DET)                                # the reuse bit changes no size
        assert size(d, DET) > size(d, 0)
        # the plain (or deterministic) regions, then the table's tangent and d ybar's tangent
        assert size(d, 0) == lib.enf_field_tangent_workspace_bytes(ctypes.byref(d))
        assert size(d, DET) - lib.enf_workspace_bytes_ex(ctypes.byref(d), DET) == size(d, 0) - lib.enf_workspace_bytes(ctypes.byref(d))
    for bad in unserved:
        assert lib.enf_check_desc(ctypes.byref(bad)) == 0 and size(bad) == 0 and size(bad, DET) == 0
    assert size(mk(O=33)) == 0                                              # a bad descriptor
    for flags in (2, 4, 8, 32, 64, 128, DET | 2, 1 << 31):                  # an unknown flag bit
        assert size(mk(), flags) == 0, flags


def test_gn_product_error_order_without_a_launch():
    lib = _lib.load()
    dummy, P, mk, unserved = _descs()
    d = mk()
    big = 1 << 40

    def call(desc=d, x=P, p=P, a=P, sigma=P, vp=P, va=P, vs=P, blob=P, w=None, cw=None, gp=P, ga=P, gs=P, ws=P, nbytes=big, flags=0):
        return lib.enf_gn_product(ctypes.byref(desc), x, 0, p, a, sigma, vp, va, vs, blob, w, cw, 1.0, gp, ga, gs, ws, nbytes, flags, None)
    # 1. the descriptor's own error comes first, whatever else is wrong
    assert call(desc=mk(O=33)) == EUNSUPPORTED and call(desc=mk(O=33), gp=None, flags=2) == EUNSUPPORTED
    bad_dim = _lib.make_desc(2, 70, 9, 2, 128, 16, 2, 3, 0, 1, 0)            # rel_pos_periodic with three coordinates
    assert call(desc=bad_dim, x=None) == -6
    # 2. what the call does not serve, before any pointer is looked at
    for bad in unserved:
        assert call(desc=bad) == EUNSUPPORTED and call(desc=bad, gp=None, vp=None, va=None, vs=None, flags=2, nbytes=0) == EUNSUPPORTED
    # 3. ENF_EINVAL: required pointers, all tangents NULL, both weights, unknown flags -- before the workspace size
    for k in ("x", "p", "a", "sigma", "blob", "gp", "ga", "gs", "ws"):
        assert call(**{k: None}) == EINVAL and call(**{k: None}, nbytes=0) == EINVAL, k
    assert call(desc=mk(window=0), sigma=None, nbytes=0) == EWORKSPACE     # sigma is required with a window only
    assert call(vp=None, va=None, vs=None, nbytes=0) == EINVAL
    assert call(w=P, cw=P, nbytes=0) == EINVAL
    for flags in (2, 4, 8, 32, 64, 128, DET | 2):
        assert call(flags=flags, nbytes=0) == EINVAL, flags
    # 4. ENF_EWORKSPACE, for every legal combination of tangents, weights and flags
    for flags in (0, DET, REUSE, DET | REUSE):
        need = lib.enf_gn_workspace_bytes(ctypes.byref(d), flags)
        for kw in ({}, {"vp": None}, {"vp": None, "va": None}, {"w": P}, {"cw": P}):
            assert call(flags=flags, nbytes=need - 1, **kw) == EWORKSPACE, (flags, kw)
    assert lib.enf_gn_workspace_bytes(ctypes.byref(d), DET) > lib.enf_gn_workspace_bytes(ctypes.byref(d), 0)
    assert call(flags=DET, nbytes=lib.enf_gn_workspace_bytes(ctypes.byref(d), 0)) == EWORKSPACE


def test_cg_update_argument_checks_without_a_launch():
    lib = _lib.load()
    dummy = ctypes.create_string_buffer(64)
    P = ctypes.cast(dummy, ctypes.c_void_p).value

    def segs(over=None, n=2):
        arr = (_lib.EnfCgSegment * _lib.ENF_CG_MAX_SEGMENTS)()
        for k in range(n):
            arr[k].x, arr[k].r, arr[k].d, arr[k].q, arr[k].width = P, P, P, P, 4
        for (k, field), val in (over or {}).items():
            setattr(arr[k], field, val)
        return arr
    call = lambda arr, nseg=2, B=3, Z=7, rho=P: lib.enf_cg_update(nseg, arr, B, Z, None, rho, None)
    assert call(segs(), nseg=0) == EINVAL and call(segs(), nseg=4) == EINVAL and call(None) == EINVAL
    assert call(segs(), B=0) == EINVAL and call(segs(), Z=0) == EINVAL and call(segs(), rho=None) == EINVAL
    for field in ("x", "r", "d"):
        assert call(segs({(1, field): None})) == EINVAL, field
    assert call(segs({(0, "width"): 0})) == EINVAL and call(segs({(1, "width"): -3})) == EINVAL
    assert call(segs({(1, "q"): None})) == EINVAL and call(segs({(0, "q"): None})) == EINVAL      # q in some segments only


# ---- 5. the Python mirror's refusals
def test_python_mirror_refuses_what_it_does_not_serve():
    from tests.test_gpu_layers import _nef as layered
    from tests.ffn_ref import build_nef_ffn
    B, N, Z = 2, 5, 3
    x, p, a, s = torch.zeros(B, N, 2), torch.zeros(B, Z, 2), torch.ones(B, Z, 8), torch.ones(B, Z, 1)
    nef = layered(dict(make_cfg("rel_pos_periodic", D=64, H=2, C=8, O=2), num_layers=1), "f32")
    with pytest.raises(NotImplementedError, match="num_layers"):
        nef.gn_product(None, x, p, a, s, va=torch.zeros_like(a))
    with pytest.raises(NotImplementedError, match="ffn"):
        build_nef_ffn(make_cfg("rel_pos_periodic", D=64, H=2, C=8, O=2), "f32").gn_product(None, x, p, a, s, va=torch.zeros_like(a))
    for inv in ("ball", "ball_lat"):
        with pytest.raises(NotImplementedError, match=inv):
            build_nef(make_cfg(inv, D=64, H=2, C=8, O=2), "f32").gn_product(None, torch.zeros(B, N, 3), torch.zeros(B, Z, 4), a, s,
                                                                             va=torch.zeros_like(a))
    flat = build_nef(make_cfg("rel_pos_periodic", D=64, H=2, C=8, O=2), "f32")
    with pytest.raises(ValueError):
        flat.gn_product(None, x, p, a, s)                                  # all three directions None
    with pytest.raises(_lib.EnfError):                                     # host tensors: there is no CPU path
        flat.gn_product(None, x, p, a, s, va=torch.zeros_like(a))
    from enf_pde_amd.fitting import cg_solve, lm_fit_latents
    with pytest.raises(_lib.EnfError):                                     # the CG step is a kernel
        cg_solve(lambda d: d, (torch.zeros(B, Z, 2),), None, 1)
    with pytest.raises(ValueError):
        cg_solve(lambda d: d, (), None, 1)
    with pytest.raises(ValueError):
        cg_solve(lambda d: d, (torch.zeros(B, Z, 2).double(),), None, 1)
    with pytest.raises(ValueError):
        lm_fit_latents(flat, None, x, torch.zeros(B, N, 2), p, a, s, 1, components=("p", "q"))
    with pytest.raises(ValueError):
        lm_fit_latents(flat, None, x, torch.zeros(B, N, 2), p, a, None, 1, components=("window",))


# ---- 6. cg_solve and lm_fit_latents on a stand-in with a known linear Jacobian
def _cg_update_torch(segs, B, Z, lam, rho, q=None):
    """enf_cg_update's arithmetic in torch (fp32), signal by signal"""
    flat = lambda ts: torch.cat([t.reshape(B, -1) for t in ts], dim=1)
    if q is None:
        for x, r, d in segs:
            x.zero_()
            d.copy_(r)
        rho.copy_((flat([r for _, r, _ in segs]) ** 2).sum(1))
        return
    lam = torch.zeros(B) if lam is None else lam
    qd = [qi + lam[:, None, None] * d for qi, (_, _, d) in zip(q, segs)]
    kappa = (flat([d for _, _, d in segs]) * flat(qd)).sum(1)
    live = (rho > 0) & torch.isfinite(rho) & (kappa > 0) & torch.isfinite(kappa)
    alpha = torch.where(live, rho / torch.where(live, kappa, torch.ones_like(kappa)), torch.zeros_like(rho))[:, None, None]
    for (x, r, d), qi in zip(segs, qd):
        x.add_(alpha * d)
        r.sub_(alpha * qi)
    rho2 = torch.where(live, (flat([r for _, r, _ in segs]) ** 2).sum(1), rho)
    beta = torch.where(live, rho2 / torch.where(live, rho, torch.ones_like(rho)), torch.zeros_like(rho))[:, None, None]
    for x, r, d in segs:
        d.copy_(torch.where(live[:, None, None], r + beta * d, d))
    rho.copy_(rho2)


class _LinearNef:
    """out[b] = A_b [p_b ; a_b] (flattened latents), a per-signal (N O) x (Z (2 + 3)) matrix: J = A, G = 2 / (N O) A^T A exactly.
    Records every call and the reuse tags it was handed."""
    Z, WP, WA, N, O = 3, 2, 3, 11, 2

    def __init__(self, B):
        g = torch.Generator().manual_seed(4)
        self.A = torch.randn((B, self.N * self.O, self.Z * (self.WP + self.WA)), generator=g)
        self.B, self.gen, self.log = B, 0, []

    def _z(self, p, a):
        return torch.cat([p.reshape(self.B, -1), a.reshape(self.B, -1)], dim=1)

    def _split(self, g):
        n = self.Z * self.WP
        return g[:, :n].reshape(self.B, self.Z, self.WP), g[:, n:].reshape(self.B, self.Z, self.WA)

    def out(self, p, a):
        return torch.einsum("bij,bj->bi", self.A, self._z(p, a)).reshape(self.B, self.N, self.O)

    def gn_reserve(self, B, N, Z, dev):
        self.log.append(("reserve", B, N, Z))

    def workspace_tag(self, dev):
        return ("ws", self.gen)

    def _touch(self):
        self.gen += 1

    def mse_value_and_latent_grads(self, params, x, p, a, window, target, grad_scale=1.0, weight=None, channel_weight=None,
                                   return_errors=False):
        assert return_errors and window is None
        res = (self.out(p, a) - target).reshape(self.B, -1)
        lb = (res ** 2).sum(1) / (self.N * self.O)
        g = grad_scale / self.B * 2.0 / (self.N * self.O) * torch.einsum("bij,bi->bj", self.A, res)
        self._touch()
        self.log.append(("fit", grad_scale))
        return (lb.mean().reshape(1), *self._split(g), None, (res ** 2).reshape(self.B, self.N, self.O).sum(2), lb)

    def gn_product(self, params, x, p, a, window, vp=None, va=None, vwindow=None, weight=None, channel_weight=None, grad_scale=1.0, reuse=None):
        self.log.append(("gn", vp is None, va is None, vwindow is None, reuse == self.workspace_tag(None)))
        v = self._z(torch.zeros(self.B, self.Z, self.WP) if vp is None else vp, torch.zeros(self.B, self.Z, self.WA) if va is None else va)
        g = grad_scale / self.B * 2.0 / (self.N * self.O) * torch.einsum("bij,bi->bj", self.A, torch.einsum("bij,bj->bi", self.A, v))
        self._touch()
        return (*self._split(g), None)

    def eval_loss(self, params, x, p, a, window, target, weight=None, channel_weight=None):
        self._touch()
        self.log.append(("eval",))
        err = ((self.out(p, a) - target) ** 2).sum(2)
        return err.sum(1) / (self.N * self.O), err


def test_cg_solve_and_lm_fit_latents_on_a_linear_stand_in(monkeypatch):
    from enf_pde_amd.fitting import gauss_newton as GN
    monkeypatch.setattr(GN, "_cg_update", _cg_update_torch)
    B = 3
    nef = _LinearNef(B)
    g = torch.Generator().manual_seed(5)
    # cg_solve: n iterations solve an n-dimensional SPD system; lam as given per signal; a zero right-hand side stays frozen at x = 0
    n = nef.Z * (nef.WP + nef.WA)
    G = 2.0 / (nef.N * nef.O) * torch.einsum("bij,bik->bjk", nef.A, nef.A).double()
    rhs = torch.randn((B, n), generator=g)
    rhs[2] = 0.0
    lam = torch.tensor([0.0, 0.5, 2.0])
    mv = lambda d: nef.gn_product(None, None, None, None, None, vp=d[0], va=d[1], grad_scale=float(B))[:2]
    xs = GN.cg_solve(mv, nef._split(rhs), lam, 2 * n)
    want = torch.linalg.solve(G + lam.double()[:, None, None] * torch.eye(n, dtype=torch.float64), rhs.double())
    got = nef._z(*xs).double()
    assert torch.equal(got[2], torch.zeros(n, dtype=torch.float64))
    assert float((got - want).norm() / want.norm()) < 1e-4
    # lm_fit_latents: a linear model is fitted by ONE undamped Gauss-Newton step; tiny damping, enough CG iterations
    nef.log.clear()
    p0, a0 = torch.randn((B, nef.Z, nef.WP), generator=g), torch.randn((B, nef.Z, nef.WA), generator=g)
    ps, as_ = p0 + 0.3 * torch.randn(p0.shape, generator=g), a0 + 0.3 * torch.randn(a0.shape, generator=g)
    target = nef.out(ps, as_)
    x = torch.zeros(B, nef.N, 2)
    (p1, a1, w1), loss_b, lam1, acc = GN.lm_fit_latents(nef, None, x, target, p0, a0, None, steps=2, cg_iters=2 * n, damping=1e-6)
    assert w1 is None and loss_b.shape == (3, B) and acc.shape == (2, B) and acc.dtype == torch.bool and lam1.shape == (B,)
    assert bool(acc[0].all()) and bool((loss_b[1] < 1e-6 * loss_b[0]).all()) and bool((loss_b[2] <= loss_b[1]).all())
    want_lam = torch.where(acc[1], torch.full((B,), 1e-6 / 9), torch.full((B,), 4e-6 / 3))
    assert torch.allclose(lam1, want_lam, rtol=1e-5)
    # the sequence per step: one fit step at gradient scale B, cg_iters products that reuse its point, one evaluation
    assert nef.log[0] == ("reserve", B, nef.N, nef.Z)
    step = [("fit", float(B))] + [("gn", False, False, True, True)] * (2 * n) + [("eval",)]
    assert nef.log[1:] == step * 2
    # components: an unused component passes None and stays where it was
    nef.log.clear()
    (p2, a2, _), lb2, _, acc2 = GN.lm_fit_latents(nef, None, x, target, p0, a0, None, steps=1, cg_iters=4, components=("a",))
    assert torch.equal(p2, p0) and not torch.equal(a2, a0) and bool(acc2.all()) and bool((lb2[1] < lb2[0]).all())
    assert all(e[1:4] == (True, False, True) for e in nef.log if e[0] == "gn")
    # a rejected signal keeps its latents and its damping grows: a target nobody can improve on (already fitted exactly)
    exact = nef.out(p0, a0)
    (p3, a3, _), lb3, lam3, acc3 = GN.lm_fit_latents(nef, None, x, exact, p0, a0, None, steps=1, cg_iters=3, damping=1e-2)
    assert not bool(acc3.any()) and torch.equal(p3, p0) and torch.equal(a3, a0) and torch.allclose(lam3, torch.full((B,), 4e-2))
    assert torch.equal(lb3[1], lb3[0])
