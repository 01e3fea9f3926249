"""The Gauss-Newton product on sparse observation operators without a GPU (include/enf_hip.h, "Gauss-Newton product on sparse
observations"): the yardstick itself (tests/gn_operators_ref.py: symmetry, its quadratic form, the central difference of
operators_ref.operator_loss's gradients at zero residual, equal groups against the grouped yardstick), the header and the bindings, the
size query, the refusals of enf_gn_product_a and their order (every call here fails its checks, so nothing is launched), the Python
mirror's refusals and the argument checks of lm_fit_linear_observations."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from enf_pde_amd import _lib
from enf_pde_amd.fitting import SparseObservations, lm_fit_linear_observations
from tests import gn_cells_ref
from tests.helpers import build_nef, make_cfg
from tests.gn_operators_ref import case, oracle_gn_operator
from tests.operators_ref import operator_loss, rel
from tests.test_gn_host import _descs, _dot
from tests.test_operators_host import _setup

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, EUNSUPPORTED, EWORKSPACE = -1, -3, -4
DET, REUSE = _lib.ENF_BWD_DETERMINISTIC, _lib.ENF_GN_REUSE_POINT
LENGTHS = [0, 1, 3, 9, 5, 30]


# ---- 1. the yardstick
@pytest.mark.parametrize("inv,weights,h", [("rel_pos_periodic", "obs", 1e-6), ("latitude_periodic", "value", 1e-6), ("ponita", None, 1e-6)])
def test_reference_product_is_symmetric_and_matches_the_gradient_difference(inv, weights, h):
    """The bounds of tests/test_gn_cells_host.py: G = coef J^T A^T W A J is symmetric and equals its quadratic form up to fp64
    summation (1e-12), and at zero residual (target = A out) it IS the Hessian of the operator's loss, so G v equals the central
    difference of operator_loss's gradients along v: h = 1e-6 leaves truncation ~ 1e-12 and rounding ~ 1e-16 / h = 1e-10, bound 1e-7.
    The difference assumes that no relu of the query branch changes sign between the two points."""
    c = case(inv, LENGTHS, 24, weights=weights)
    rng = np.random.default_rng(13)
    u = tuple(rng.standard_normal(t.shape) * sc for t, sc in zip(c.v, (0.3, 1.0, 0.1)))
    Gv = c.ref
    Gu = oracle_gn_operator(c.cfg, c.prm, c.x, c.p, c.a, c.s, u, c.A, c.w, c.gs)[0]
    e_sym = abs(_dot(u, Gv) - _dot(Gu, c.v)) / abs(_dot(u, Gv))
    coef = c.gs * 2.0 / (c.B * c.M * c.O)
    wt = np.ones((c.B, c.M, c.O)) if c.w is None else (c.w[..., None] if c.w.ndim == 2 else c.w)
    quad = coef * float((wt * c.obs_tan ** 2).sum())
    e_quad = abs(_dot(c.v, Gv) - quad) / quad
    obs = operator_loss(c.cfg, c.prm, c.x, c.p, c.a, c.s, c.A, np.zeros((c.B, c.M, c.O)), grads=False).obs
    grad = lambda sg: operator_loss(c.cfg, c.prm, c.x, c.p + sg * h * c.v[0], c.a + sg * h * c.v[1], c.s + sg * h * c.v[2], c.A, obs, c.w,
                                    c.gs).g
    cd = [(a_ - b_) / (2 * h) for a_, b_ in zip(grad(1.0), grad(-1.0))]
    e_cd = float(np.sqrt(sum(((d - g) ** 2).sum() for d, g in zip(cd, Gv))) / np.sqrt(sum((g ** 2).sum() for g in Gv)))
    print(f"{inv} weights={weights} h={h:.0e}: symmetry {e_sym:.2e}, quadratic form {e_quad:.2e}, central difference of the gradients {e_cd:.2e}")
    assert _dot(c.v, Gv) > 0 and e_sym < 1e-12 and e_quad < 1e-12 and e_cd < 1e-7
    assert (c.obs_tan[:, 0] == 0).all()                                       # the empty row


def test_reference_product_at_equal_groups_is_the_grouped_one():
    """an operator of groups of 4 with signal 0's factors against gn_cells_ref.oracle_gn_cells with those factors for every signal"""
    c = gn_cells_ref.case("rel_pos_periodic", 4, 16)
    q0 = c.q[0]
    A = SparseObservations.from_groups(np.full(c.M, 4), q0).to_dense()
    got = oracle_gn_operator(c.cfg, c.prm, c.x, c.p, c.a, c.s, c.v, A, c.w, c.gs)[0]
    want = gn_cells_ref.oracle_gn_cells(c.cfg, c.prm, c.x, c.p, c.a, c.s, c.v, 4, np.repeat(q0[None], 3, 0), c.w, c.gs)[0]
    for g, r in zip(got, want):
        assert rel(g, r) < 1e-12
    assert (c.w == 0).any()


# ---- 2. header, exports, argument types
def test_symbols_header_and_binding():
    with open(os.path.join(ROOT, "include", "enf_hip.h")) as f:
        h = f.read()
    assert re.search(r"#define\s+ENF_ABI_VERSION\s+2\b", h) and "Gauss-Newton product on sparse observations" in h
    lib = _lib.load()
    assert lib.enf_abi_version() == 2
    assert re.search(r"\bint\s+enf_gn_product_a\s*\(", h) and re.search(r"\bsize_t\s+enf_gn_a_workspace_bytes\s*\(", h)
    for name in ("enf_gn_product_a", "enf_gn_a_workspace_bytes"):
        assert name in _lib.EXPORTS and hasattr(lib, name) and hasattr(_lib.load_test(), name) and hasattr(_lib.load_f32r(), name)
    at = lib.enf_gn_product_a.argtypes
    assert len(at) == 21 and at[2] is ctypes.c_int64 and at[10] is ctypes.POINTER(_lib.EnfSparseObs) and at[13] is ctypes.c_float
    assert at[18] is ctypes.c_size_t and at[19] is ctypes.c_uint
    assert all(at[i] is ctypes.c_void_p for i in (1, 3, 4, 5, 6, 7, 8, 9, 11, 12, 14, 15, 16, 17, 20))
    assert lib.enf_gn_a_workspace_bytes.restype is ctypes.c_size_t and len(lib.enf_gn_a_workspace_bytes.argtypes) == 3
    decl = re.sub(r"/\*.*?\*/", "", h[h.index("int enf_gn_product_a("):].split(";")[0], flags=re.S)
    names = [a.split()[-1].lstrip("*") for a in decl[decl.index("(") + 1:decl.rindex(")")].split(",")]
    assert names == ["d", "x", "x_bstride", "p", "a", "sigma", "vp", "va", "vsigma", "packed", "op", "oweight", "cweight", "grad_scale",
                     "gp", "ga", "gsigma", "workspace", "workspace_bytes", "flags", "stream"]


# ---- 3. the size query
def test_workspace_size_query():
    lib = _lib.load()
    dummy, P, mk, unserved = _descs()
    size = lambda desc, M=5, flags=0: lib.enf_gn_a_workspace_bytes(ctypes.byref(desc), M, flags)
    for d in (mk(), mk(D=64, H=4), mk(window=0), mk(O=5)):
        O = d.O
        for flags in (0, DET, REUSE, DET | REUSE):
            for M in (1, 5, 500, 100000):
                need = size(d, M, flags)
                gn = lib.enf_gn_workspace_bytes(ctypes.byref(d), flags)
                # tan and d out (B, N, O) and r (B, M, O) behind the product's own regions, and never below the deterministic fit step's
                assert need % 256 == 0 and need >= gn + 4 * (2 * 2 * 70 * O + 2 * M * O)
                assert need >= lib.enf_obs_workspace_bytes(ctypes.byref(d), M, _lib.ENF_FIT_DETERMINISTIC) > 0
        assert size(d, 500) > size(d, 5) and size(d, 5, DET) > size(d, 5, 0) and size(d, 5, REUSE) == size(d, 5, 0)
    d = mk()
    assert size(d, 0) == 0 and size(d, -1) == 0
    for flags in (2, 4, 8, 32, 64, DET | 2):
        assert size(d, 5, flags) == 0, flags
    for bad in unserved + (mk(O=33),):
        assert size(bad) == 0 and size(bad, 5, DET) == 0


# ---- 4. the refusals and their order, without a launch
def test_gn_product_a_error_order_without_a_launch():
    lib = _lib.load()
    dummy, P, mk, unserved = _descs()
    _, _, _, op = _setup()
    d = mk()
    big = 1 << 40

    def call(desc=d, x=P, p=P, a=P, sigma=P, vp=P, va=P, vs=P, blob=P, o=None, w=None, cw=None, gp=P, ga=P, gs=P, ws=P, nbytes=big, flags=0):
        o = ctypes.byref(op()) if o is None else (None if o == "null" else ctypes.byref(o))
        return lib.enf_gn_product_a(ctypes.byref(desc), x, 0, p, a, sigma, vp, va, vs, blob, o, w, cw, 1.0, gp, ga, gs, ws, nbytes, flags, None)
    # 1. the descriptor's own error comes first, whatever else is wrong
    assert call(desc=mk(O=33)) == EUNSUPPORTED and call(desc=mk(O=33), gp=None, flags=2, o="null") == EUNSUPPORTED
    bad_dim = _lib.make_desc(2, 80, 9, 2, 128, 16, 2, 3, 0, 1, 0)            # rel_pos_periodic with three coordinates
    assert call(desc=bad_dim, x=None, o="null") == -6
    # 2. what the call does not serve, before any pointer or the operator is looked at
    for bad in unserved:
        assert call(desc=bad) == EUNSUPPORTED
        assert call(desc=bad, gp=None, vp=None, va=None, vs=None, flags=2, nbytes=0, o="null") == EUNSUPPORTED
    # 3. ENF_EINVAL: what enf_gn_product refuses, and the operator -- before the workspace size
    for k in ("x", "p", "a", "sigma", "blob", "gp", "ga", "gs", "ws"):
        assert call(**{k: None}) == EINVAL and call(**{k: None}, nbytes=0) == EINVAL, k
    assert call(desc=mk(window=0), sigma=None, nbytes=0) == EWORKSPACE     # sigma is required with a window only
    assert call(vp=None, va=None, vs=None) == EINVAL and call(vp=None, va=None, vs=None, nbytes=0) == EINVAL      # no tangent
    for flags in (2, 4, 8, 32, 64, 128, DET | 2):
        assert call(flags=flags) == EINVAL and call(flags=flags, nbytes=0) == EINVAL, flags
    assert call(o="null") == EINVAL and call(o="null", nbytes=0) == EINVAL
    # the product reads the CSR and the CSC
    for bad in (op(M=0), op(M=-3), op(nnz=-1), op(nnz=1 << 31), op(row_ptr=True), op(col=True), op(val=True), op(col_ptr=True), op(trow=True),
                op(tval=True)):
        assert call(o=bad) == EINVAL and call(o=bad, nbytes=0) == EINVAL
    assert call(o=op(nnz=0, col=True, val=True, trow=True, tval=True), nbytes=0) == EWORKSPACE      # an operator of empty rows is legal
    assert call(w=P, cw=P) == EINVAL and call(w=P, cw=P, nbytes=0) == EINVAL                        # both weight kinds
    # 4. ENF_EWORKSPACE, for every combination of tangents, weights and flags: below the operator's size, the product's own included
    for flags in (0, DET, REUSE, DET | REUSE):
        need = lib.enf_gn_a_workspace_bytes(ctypes.byref(d), 5, flags)
        for kw in ({}, {"vp": None}, {"vp": None, "va": None}, {"w": P}, {"cw": P}):
            assert call(flags=flags, nbytes=need - 1, **kw) == EWORKSPACE, (flags, kw)
            assert call(flags=flags, nbytes=lib.enf_gn_workspace_bytes(ctypes.byref(d), flags), **kw) == EWORKSPACE, (flags, kw)
    assert call(flags=DET, nbytes=lib.enf_gn_a_workspace_bytes(ctypes.byref(d), 5, 0)) == EWORKSPACE


# ---- 5. the Python mirror's refusals
def test_python_mirror_refuses_what_it_does_not_serve():
    """the refusals, error types and their order are gn_cell_product's (tests/test_gn_cells_host.py)"""
    from tests.test_gpu_layers import _nef as layered
    from tests.ffn_ref import build_nef_ffn
    B, N, Z = 2, 8, 3
    x, p, a, s = torch.zeros(B, N, 2), torch.zeros(B, Z, 2), torch.ones(B, Z, 8), torch.ones(B, Z, 1)
    va = torch.zeros_like(a)
    op = SparseObservations.from_groups([3, 0, 5], None)
    nef = layered(dict(make_cfg("rel_pos_periodic", D=64, H=2, C=8, O=2), num_layers=1), "f32")
    with pytest.raises(NotImplementedError, match="num_layers"):
        nef.gn_operator_product(None, x, p, a, s, op, va=va)
    with pytest.raises(NotImplementedError, match="ffn"):
        build_nef_ffn(make_cfg("rel_pos_periodic", D=64, H=2, C=8, O=2), "f32").gn_operator_product(None, x, p, a, s, op, va=va)
    for inv in ("ball", "ball_lat"):
        with pytest.raises(NotImplementedError, match=inv):
            build_nef(make_cfg(inv, D=64, H=2, C=8, O=2), "f32").gn_operator_product(None, torch.zeros(B, N, 3), torch.zeros(B, Z, 4), a, s, op,
                                                                                      va=va)
    flat = build_nef(make_cfg("rel_pos_periodic", D=64, H=2, C=8, O=2), "f32")
    with pytest.raises(ValueError, match="at least one"):
        flat.gn_operator_product(None, x, p, a, s, op)                      # all three directions None
    with pytest.raises(ValueError, match="at least one"):                   # ... ahead of the shape checks
        flat.gn_operator_product(None, x[:, :7], p, a, s, op)
    with pytest.raises(ValueError, match="columns"):
        flat.gn_operator_product(None, x[:, :7], p, a, s, op, va=va)
    for bad in (torch.ones(B, N), torch.ones(3), torch.ones(B, 3, 1)):
        with pytest.raises(ValueError, match="obs_weight"):
            flat.gn_operator_product(None, x, p, a, s, op, obs_weight=bad, va=va)
    for bad in (torch.ones(B, 3), torch.ones(B, N, 2), torch.ones(B, 3, 1)):
        with pytest.raises(ValueError, match="obs_channel_weight"):
            flat.gn_operator_product(None, x, p, a, s, op, obs_channel_weight=bad, va=va)
    with pytest.raises(ValueError, match="not both"):
        flat.gn_operator_product(None, x, p, a, s, op, obs_weight=torch.ones(B, 3), obs_channel_weight=torch.ones(B, 3, 2), va=va)
    with pytest.raises(_lib.EnfError):                                     # host tensors: there is no CPU path
        flat.gn_operator_product(None, x, p, a, s, op, obs_weight=torch.ones(B, 3), va=va)


def test_lm_fit_linear_observations_checks_its_arguments():
    B, N, Z = 2, 8, 3
    x, p, a, s = torch.zeros(B, N, 2), torch.zeros(B, Z, 2), torch.ones(B, Z, 8), torch.ones(B, Z, 1)
    op = SparseObservations.from_groups([3, 0, 5], None)
    y = torch.zeros(B, 3, 2)
    flat = build_nef(make_cfg("rel_pos_periodic", D=64, H=2, C=8, O=2), "f32")
    with pytest.raises(ValueError, match="columns"):
        lm_fit_linear_observations(flat, None, x[0, :7], op, y, p, a, s, 1)
    with pytest.raises(ValueError, match="columns"):
        lm_fit_linear_observations(flat, None, x[:, :7], op, y, p, a, s, 1)
    with pytest.raises(ValueError, match="signals"):
        lm_fit_linear_observations(flat, None, x[:1], op, y, p, a, s, 1)
    with pytest.raises(ValueError, match="x must be"):
        lm_fit_linear_observations(flat, None, x[0, 0], op, y, p, a, s, 1)
    with pytest.raises(ValueError, match="target"):
        lm_fit_linear_observations(flat, None, x[0], op, torch.zeros(B, 4, 2), p, a, s, 1)
    with pytest.raises(ValueError, match="components"):
        lm_fit_linear_observations(flat, None, x[0], op, y, p, a, s, 1, components=("p", "q"))
    with pytest.raises(ValueError, match="window"):
        lm_fit_linear_observations(flat, None, x, op, y, p, a, None, 1, components=("window",))
    from enf_pde_amd import fitting
    assert "lm_fit_linear_observations" in fitting.__all__ and fitting.lm_fit_linear_observations is lm_fit_linear_observations
