"""Sparse linear observations without a GPU (include/enf_hip.h, "Sparse linear observations"): the operator value of
fitting/operators.py (CSC = the transpose of the CSR, the stable sort, the constructors and their refusals), the rules of cell_operator
and line_integrals in fp64, the yardstick itself (tests/operators_ref.py against tests/cells_ref.py at equal groups and against central
differences), the header and the bindings, and the refusals of the entry points (every call here fails its checks: nothing is launched)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from enf_pde_amd import _lib
from enf_pde_amd.fitting import SparseObservations, cell_operator, cell_quadrature, fit_linear_observations, line_integrals
from enf_pde_amd.fitting.observations import LinearObservations, observed
from tests import cells_ref
from tests.helpers import build_nef, make_cfg
from tests.operators_ref import case, dense_loss, operator_loss, ragged_entries

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, EUNSUPPORTED, EWORKSPACE = -1, -3, -4
DET, SHARED = _lib.ENF_FIT_DETERMINISTIC, _lib.ENF_FIT_SHARED_LATENTS


# ---- 1. the operator value
def _random_operator(seed, M=13, N=17):
    """ragged: empty rows, empty columns (the last three), overlaps, unsorted columns, one repeated (row, column)"""
    rng = np.random.default_rng(seed)
    lengths = rng.integers(0, 8, M)
    lengths[[2, 5]] = 0
    rows, cols, vals = ragged_entries(lengths, N, seed + 1, spare=3)
    rows, cols, vals = np.append(rows, rows[0]), np.append(cols, cols[0]), np.append(vals, 0.25)       # a duplicate entry
    perm = rng.permutation(rows.size)                                                                  # COO order is arbitrary
    return rows[perm], cols[perm], vals[perm], M, N


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_csc_is_the_transpose_of_the_csr(seed):
    rows, cols, vals, M, N = _random_operator(seed)
    op = SparseObservations.from_coo(rows, cols, vals, M, N)
    want = np.zeros((M, N))
    np.add.at(want, (rows, cols), vals)
    assert (op.M, op.N, op.nnz) == (M, N, rows.size)
    assert np.array_equal(op.to_dense(), want) or np.allclose(op.to_dense(), want, rtol=1e-15, atol=0)
    assert np.array_equal(op.to_dense(transposed=True), op.to_dense().T)
    assert np.array_equal(op.to_dense(transposed=True, dtype=np.float32), op.to_dense(dtype=np.float32).T)
    rp, cp = op.row_ptr.numpy(), op.col_ptr.numpy()
    assert rp[0] == 0 and rp[-1] == op.nnz and cp[0] == 0 and cp[-1] == op.nnz and (np.diff(rp) >= 0).all() and (np.diff(cp) >= 0).all()
    assert (np.diff(rp) == 0).sum() >= 2 and (np.diff(cp)[-3:] == 0).all()                # empty rows and empty columns are there
    assert any((np.diff(op.col.numpy()[rp[m]:rp[m + 1]]) < 0).any() for m in range(M))   # unsorted columns inside a row
    # from_coo keeps a row's entries in the order given, and nothing is summed
    for m in range(M):
        assert np.array_equal(op.col.numpy()[rp[m]:rp[m + 1]], cols[rows == m])
        assert np.array_equal(op.val.numpy()[rp[m]:rp[m + 1]], vals[rows == m].astype(np.float32))
    # the stable sort: a column's entries come in CSR order (by row, and within a row by position)
    erow = np.repeat(np.arange(M), np.diff(rp))
    for n in range(N):
        src = np.flatnonzero(op.col.numpy() == n)                                         # CSR positions of column n, increasing
        assert np.array_equal(op.trow.numpy()[cp[n]:cp[n + 1]], erow[src])
        assert np.array_equal(op.tval.numpy()[cp[n]:cp[n + 1]], op.val.numpy()[src])
    assert op.row_ptr.dtype == torch.int32 and op.trow.dtype == torch.int32 and op.val.dtype == torch.float32


def test_from_groups_with_equal_sizes_is_the_grouped_layout():
    x, q = cell_quadrature((-1.0, 1.0, (3, 2)), 2)
    op = SparseObservations.from_groups(np.full(6, 4), q)
    assert np.array_equal(op.row_ptr.numpy(), np.arange(7) * 4) and np.array_equal(op.col.numpy(), np.arange(24))
    assert torch.equal(op.val, q) and np.array_equal(op.col_ptr.numpy(), np.arange(25)) and np.array_equal(op.trow.numpy(), np.arange(24) // 4)
    dense = op.to_dense(dtype=np.float32)
    assert np.array_equal(dense[np.arange(24) // 4, np.arange(24)], q.numpy()) and np.count_nonzero(dense) == 24
    mean = SparseObservations.from_groups([2, 0, 3], None)                                 # ragged, the plain mean, an empty group
    assert np.array_equal(mean.to_dense(), np.array([[.5, .5, 0, 0, 0], [0] * 5, [0, 0, 1 / 3, 1 / 3, 1 / 3]]))


def test_constructor_refusals():
    ok = dict(row_ptr=[0, 2, 3], col=[0, 1, 1], val=[1.0, 2.0, 3.0], N=2)
    SparseObservations(**ok)
    for change in (dict(row_ptr=[1, 2, 3]), dict(row_ptr=[0, 3, 2]), dict(row_ptr=[0, 2, 4]), dict(row_ptr=[0]), dict(N=0),
                   dict(col=[0, 2, 1]), dict(col=[0, -1, 1]), dict(val=[1.0, np.nan, 3.0]), dict(val=[1.0, np.inf, 3.0]), dict(val=[1.0, 1e39, 3.0]),
                   dict(val=[1.0, 2.0]), dict(col=[0.0, 1.0, 1.0]), dict(row_ptr=[[0, 2, 3]])):
        with pytest.raises(ValueError):
            SparseObservations(**dict(ok, **change))
    for bad in (dict(rows=[0, 2]), dict(rows=[0, -1]), dict(M=0), dict(cols=[0]), dict(cols=[0, 5]), dict(rows=[0.0, 1.0]), dict(cols=[0.0, 1.0]),
                dict(cols=[0.5, 1.0])):
        with pytest.raises(ValueError):
            SparseObservations.from_coo(**dict(dict(rows=[0, 1], cols=[0, 1], vals=[1.0, 1.0], M=2, N=2), **bad))
    for sizes, q in (([], None), ([2, -1], None), ([2, 2], [1.0, 1.0, 1.0]), ([[2, 2]], None)):
        with pytest.raises(ValueError):
            SparseObservations.from_groups(sizes, q)
    with pytest.raises(_lib.EnfError):
        SparseObservations(**ok).struct()                                                 # host arrays: there is no CPU path


# ---- 2. the rules
EX, EY, EZ = np.array([-1.0, -0.3, 0.4, 1.0]), np.array([0.2, 0.9, 1.0]), np.array([0.0, 0.25, 1.5])


def _cell_means_of_monomials(edges, degrees):
    """the exact mean of prod_ax t_ax^n_ax over every cell, cells in C order"""
    mean = lambda e, n: (e[1:] ** (n + 1) - e[:-1] ** (n + 1)) / ((n + 1) * (e[1:] - e[:-1]))
    out = np.ones(())
    for e, n in zip(edges, degrees):
        out = np.multiply.outer(out, mean(e, n))
    return out.reshape(-1)


def _check_exact(edges, k, rule, degree, tol=1e-12):
    x, op = cell_operator(edges, k, rule=rule, dtype=torch.float64)
    A, xs = op.to_dense(), x.numpy()
    worst = 0.0
    for degs in np.ndindex(*([degree + 1] * len(edges))):
        got = A @ np.prod([xs[:, ax] ** n for ax, n in enumerate(degs)], axis=0)
        worst = max(worst, float(np.abs(got - _cell_means_of_monomials(edges, degs)).max()))
    assert worst <= tol, (rule, k, worst)
    return x, op, A


def test_cell_operator_equals_cell_quadrature_where_it_serves_k():
    for cells, k, rule, kind in (([EX, EY], 2, "gauss", "cartesian"), ((-1.0, 1.0, (3, 2)), 4, "midpoint", "cartesian"),
                                 ([EX + 1.0, EY + 0.3], 2, "gauss", "sphere"), ([EX, EY, EZ], 2, "gauss", "cartesian"), ([EX], 8, "gauss", "cartesian")):
        x, q = cell_quadrature(cells, k, rule=rule, kind=kind)
        xo, op = cell_operator(cells, k, rule=rule, kind=kind)
        G = k ** x.shape[1]
        assert torch.equal(x, xo) and torch.equal(q, op.val) and np.array_equal(op.col.numpy(), np.arange(x.shape[0]))
        assert np.array_equal(op.row_ptr.numpy(), np.arange(op.M + 1) * G)


def test_gauss_3_is_exact_to_degree_5_per_axis_in_2d_and_3d():
    x, op, A = _check_exact([EX, EY], 3, "gauss", 5)
    assert x.shape == (6 * 9, 2) and op.M == 6 and (np.diff(op.row_ptr.numpy()) == 9).all()          # the 9-point rule the tail cannot group
    x3, op3, _ = _check_exact([EX, EY, EZ], 3, "gauss", 5)
    assert x3.shape == (12 * 27, 3) and (np.diff(op3.row_ptr.numpy()) == 27).all()
    with pytest.raises(AssertionError):
        _check_exact([EX, EY], 3, "gauss", 6)                                                        # (degree 6 is not)


def test_closed_rules_share_nodes_and_hold_their_degree():
    x, op, A = _check_exact([EX, EY], 3, "simpson", 3)
    assert x.shape == ((2 * 3 + 1) * (2 * 2 + 1), 2) and op.M == 6 and op.nnz == 6 * 9                # (2c + 1)^dx nodes
    assert (np.count_nonzero(A, axis=0) > 1).any() and np.allclose(A.sum(1), 1.0, rtol=1e-14)         # neighbours share nodes
    x3, op3, _ = _check_exact([EX, EY, EZ], 3, "simpson", 3)
    assert x3.shape == (7 * 5 * 5, 3)
    with pytest.raises(AssertionError):
        _check_exact([EX, EY], 3, "simpson", 4)
    xt, opt, At = _check_exact([EX, EY], 2, "trapezoid", 1)
    assert xt.shape == (4 * 3, 2) and np.array_equal(np.unique(xt[:, 0].numpy()), EX) and np.allclose(At.sum(1), 1.0, rtol=1e-14)
    with pytest.raises(AssertionError):
        _check_exact([EX, EY], 2, "trapezoid", 2)
    _check_exact([EX, EY], 4, "trapezoid", 1)                                                         # three sub-intervals per cell
    assert cell_operator([EX, EY], 4, rule="trapezoid")[0].shape == (10 * 7, 2)
    _check_exact([EX], 5, "simpson", 3)


def test_sphere_rows_sum_to_one():
    phi, th = np.linspace(0, 2 * np.pi, 4), np.linspace(0.0, np.pi, 7)
    for k, rule in ((3, "gauss"), (3, "simpson"), (2, "trapezoid"), (5, "midpoint")):
        x, op = cell_operator([phi, th], k, rule=rule, kind="sphere", dtype=torch.float64)
        assert np.allclose(op.to_dense().sum(1), 1.0, rtol=1e-13, atol=0) and op.M == 18
    # the area mean of cos(theta): (sin^2 t1 - sin^2 t0) / (2 (cos t0 - cos t1)); 3 Gauss points on cells of pi / 6, error ~ 1e-7
    x, op = cell_operator([phi, th], 3, kind="sphere", dtype=torch.float64)
    want = (np.sin(th[1:]) ** 2 - np.sin(th[:-1]) ** 2) / (2 * (np.cos(th[:-1]) - np.cos(th[1:])))
    assert np.allclose((op.to_dense() @ np.cos(x[:, 1].numpy())).reshape(3, 6), want[None].repeat(3, 0), rtol=0, atol=1e-5)


def test_cell_operator_refusals():
    for kw in (dict(k=0), dict(k=2, rule="simpson"), dict(k=1, rule="simpson"), dict(k=1, rule="trapezoid"), dict(k=2, rule="boole"),
               dict(k=2, kind="torus")):
        with pytest.raises(ValueError):
            cell_operator([EX, EY], **kw)
    with pytest.raises(ValueError):
        cell_operator([EX], 2, kind="sphere")
    with pytest.raises(ValueError):
        cell_operator((1.0, 0.0, 4), 2)


def test_line_integrals_are_exact_for_a_linear_field():
    rng = np.random.default_rng(5)
    s, e = rng.uniform(-1, 1, (7, 3)), rng.uniform(-1, 1, (7, 3))
    g, c0 = np.array([0.7, -1.1, 0.4]), 0.3
    want = np.linalg.norm(e - s, axis=1) * (c0 + 0.5 * (s + e) @ g)                        # length * the field at the midpoint
    for k, rule in ((1, "gauss"), (4, "gauss"), (3, "midpoint"), (2, "trapezoid"), (5, "simpson")):
        x, op = line_integrals(s, e, k, rule=rule, dtype=torch.float64)
        assert x.shape == (7 * k, 3) and op.M == 7 and (np.diff(op.row_ptr.numpy()) == k).all()
        assert np.allclose(op.to_dense() @ (c0 + x.numpy() @ g), want, rtol=1e-13, atol=1e-14), rule
    x, op = line_integrals(s, e, 3, dtype=torch.float64)                                   # and for a quintic along the ray
    ua, ub = s @ g, e @ g                                                                  # u = g . x runs linearly from ua to ub
    assert np.allclose(op.to_dense() @ (x.numpy() @ g) ** 5, np.linalg.norm(e - s, axis=1) * (ub ** 6 - ua ** 6) / (6 * (ub - ua)),
                       rtol=1e-11, atol=1e-13)
    for bad in (dict(starts=s[:, :2]), dict(starts=s[0]), dict(k=0), dict(rule="boole"), dict(k=2, rule="simpson")):
        with pytest.raises(ValueError):
            line_integrals(**dict(dict(starts=s, ends=e, k=2), **bad))


# ---- 3. the yardstick itself
def test_yardstick_equals_the_grouped_one_at_equal_groups():
    c = cells_ref.case("rel_pos_periodic", 4, 16)
    q0 = c.q[0]                                                    # one operator for all signals: signal 0's factors
    qb = np.repeat(q0[None], cells_ref.B, 0)
    ref = cells_ref.cell_loss(c.cfg, c.prm, c.x, c.p, c.a, c.s, c.y, 4, qb, c.w, c.gs)
    A = SparseObservations.from_groups(np.full(c.M, 4), q0).to_dense()
    got = operator_loss(c.cfg, c.prm, c.x, c.p, c.a, c.s, A, c.y, c.w, c.gs)
    assert abs(got.loss - ref.loss) <= 1e-14 * ref.loss and np.allclose(got.err_a, ref.err_g, rtol=1e-13, atol=1e-16)
    assert np.allclose(got.obs, ref.obs, rtol=1e-13, atol=1e-15) and np.allclose(got.loss_b, ref.loss_b, rtol=1e-13)
    for u, v in zip(got.g, ref.g):
        assert np.linalg.norm(u - v) <= 1e-12 * np.linalg.norm(v)


@pytest.mark.parametrize("weights", ["obs", "value", None])
def test_yardstick_dout_is_the_central_difference_of_its_loss(weights):
    """along a random direction of out: the loss is quadratic in out, so the central difference is exact up to rounding, ~ 1e-16 / h
    relative with h = 1e-4: asserted at 1e-9"""
    c = case("rel_pos_periodic", [0, 1, 3, 9, 5], 12, weights=weights)
    rng = np.random.default_rng(4)
    out, v = c.ref.out, rng.standard_normal(c.ref.out.shape)
    r = dense_loss(c.A, out, c.y, c.w, c.gs)
    assert abs(r.loss - c.ref.loss) <= 1e-14 * c.ref.loss and np.allclose(r.err_a, c.ref.err_a, rtol=1e-13, atol=1e-16)
    h = 1e-4
    cd = (dense_loss(c.A, out + h * v, c.y, c.w).loss - dense_loss(c.A, out - h * v, c.y, c.w).loss) / (2 * h)
    want = float((r.dout * v).sum()) / c.gs
    assert abs(cd - want) <= 1e-9 * abs(want), (cd, want)
    assert (r.dout[:, -3:] == 0).all() and (r.obs[:, 0] == 0).all()                       # unreferenced columns, the empty row
    if weights is not None:
        from tests.operators_ref import poisoned
        p = dense_loss(c.A, out, poisoned(c.y, c.w), c.w, c.gs)
        assert p.loss == r.loss and np.array_equal(p.dout, r.dout) and np.array_equal(p.err_a, r.err_a)


# ---- 4. header, exports, argument types
NAMES = ("enf_obs_apply", "enf_mse_value_grad_a", "enf_fit_step_a", "enf_eval_loss_a")


def test_symbols_header_and_abi():
    with open(os.path.join(ROOT, "include", "enf_hip.h")) as f:
        h = f.read()
    assert re.search(r"#define\s+ENF_ABI_VERSION\s+2\b", h) and "Sparse linear observations" in h
    lib = _lib.load()
    for name in NAMES + ("enf_obs_workspace_bytes", "enf_mse_a_scratch_bytes"):
        assert re.search(rf"\b(int|size_t)\s+{name}\s*\(", h), name
        assert name in _lib.EXPORTS and hasattr(lib, name) and hasattr(_lib.load_test(), name) and hasattr(_lib.load_f32r(), name)
    assert len(lib.enf_fit_step_a.argtypes) == 22 and len(lib.enf_eval_loss_a.argtypes) == 18 and len(lib.enf_mse_value_grad_a.argtypes) == 16
    # the struct, field by field against the header
    body = re.sub(r"/\*.*?\*/", "", h[h.index("typedef struct EnfSparseObs {"):h.index("} EnfSparseObs;")], flags=re.S)
    fields = re.findall(r"\b(int32_t|int64_t|const int32_t\*|const float\*)\s+(\w+);", body)
    assert [n for _, n in fields] == [f[0] for f in _lib.EnfSparseObs._fields_]
    kinds = {"int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64}
    assert all(ct is kinds.get(k, ctypes.c_void_p) for (k, _), (_, ct) in zip(fields, _lib.EnfSparseObs._fields_))
    assert _lib.EnfSparseObs.nnz.offset == 8 and ctypes.sizeof(_lib.EnfSparseObs) == 64


# ---- 5. the refusals, without a launch
def _setup():
    dummy = ctypes.create_string_buffer(64)
    P = ctypes.cast(dummy, ctypes.c_void_p)
    mk = lambda N=48, O=2, window=1, B=3: _lib.make_desc(B, N, 7, 2, 64, 12, O, 2, 0, window, 0)

    def op(M=5, nnz=9, **null):
        s = _lib.EnfSparseObs()
        s.M, s.nnz = M, nnz
        for f in ("row_ptr", "col", "val", "col_ptr", "trow", "tval"):
            setattr(s, f, None if null.get(f, False) else P.value)
        return s
    return dummy, P, mk, op


def test_fit_step_a_refusals_and_their_order():
    lib = _lib.load()
    dummy, P, mk, op = _setup()
    big = 1 << 40

    def call(desc=None, x=P, p=P, a=P, sigma=P, blob=P, y=P, o=None, w=None, cw=None, loss=P, dp=P, da=P, ds=P, err=P, lb=P, ws=P, nbytes=big,
             flags=0, xb=0):
        desc = mk() if desc is None else desc
        o = ctypes.byref(op()) if o is None else (None if o == "null" else ctypes.byref(o))
        return lib.enf_fit_step_a(ctypes.byref(desc), x, xb, p, a, sigma, blob, y, o, w, cw, 1.0, loss, dp, da, ds, err, lb, ws, nbytes, flags, None)
    # the descriptor's own error comes first, whatever else is wrong
    assert call(desc=mk(O=33)) == EUNSUPPORTED and call(desc=mk(O=33), o="null", y=None, flags=SHARED, nbytes=0) == EUNSUPPORTED
    assert call(desc=_lib.make_desc(3, 48, 7, 2, 64, 12, 2, 3, 0, 1, 0), o=op(M=0), x=None) == -6
    # the operator: NULL, M < 1, nnz < 0 or beyond int32, a missing array of the CSR or the CSC -- before the workspace is looked at
    assert call(o="null", nbytes=0) == EINVAL
    for bad in (op(M=0), op(M=-3), op(nnz=-1), op(nnz=1 << 31), op(row_ptr=True), op(col=True), op(val=True), op(col_ptr=True), op(trow=True),
                op(tval=True)):
        assert call(o=bad) == EINVAL and call(o=bad, nbytes=0) == EINVAL
    assert call(o=op(nnz=0, col=True, val=True, trow=True, tval=True), nbytes=0) == EWORKSPACE      # an operator of empty rows is legal
    assert call(w=P, cw=P) == EINVAL and call(w=P, cw=P, nbytes=0) == EINVAL                        # both weight kinds
    assert call(w=P, nbytes=0) == EWORKSPACE and call(cw=P, nbytes=0) == EWORKSPACE
    for k in ("y", "x", "p", "a", "sigma", "blob", "loss", "dp", "da", "ds", "ws"):
        assert call(**{k: None}, nbytes=0) == EINVAL, k
    assert call(err=None, lb=None, nbytes=0) == EWORKSPACE
    assert call(err=None, lb=P, nbytes=0) == EWORKSPACE                      # loss_b without err_a is allowed: the workspace has room
    assert call(desc=mk(window=0), sigma=None, nbytes=0) == EWORKSPACE
    for flags in (SHARED, SHARED | DET, 1, 2, 4, 8, 32, 64, DET | 2):
        assert call(flags=flags, nbytes=0) == EINVAL, flags
    assert call(desc=mk(B=1), flags=SHARED) == EINVAL
    # the workspace: the plain (deterministic) one first, then regions that grow with M
    d = mk()
    for flags in (0, DET):
        need = lib.enf_obs_workspace_bytes(ctypes.byref(d), 5, flags)
        base = lib.enf_workspace_bytes_ex(ctypes.byref(d), flags)
        assert need > base + 4 * (2 * 3 * 48 * 2 + 3 * 5 * 2 + 3 * 5) and need % 256 == 0
        assert call(flags=flags, nbytes=need - 1) == EWORKSPACE and call(flags=flags, nbytes=base) == EWORKSPACE
        assert lib.enf_obs_workspace_bytes(ctypes.byref(d), 500, flags) > need
    assert lib.enf_obs_workspace_bytes(ctypes.byref(d), 0, 0) == 0 and lib.enf_obs_workspace_bytes(ctypes.byref(d), 5, SHARED) == 0
    assert lib.enf_obs_workspace_bytes(ctypes.byref(mk(O=33)), 5, 0) == 0


def test_eval_loss_a_refusals_and_their_order():
    lib = _lib.load()
    dummy, P, mk, op = _setup()
    big = 1 << 40

    def call(desc=None, x=P, p=P, a=P, sigma=P, blob=P, y=P, o=None, w=None, cw=None, loss=P, err=P, lb=P, ws=P, nbytes=0, flags=0):
        desc = mk() if desc is None else desc
        o = ctypes.byref(op()) if o is None else (None if o == "null" else ctypes.byref(o))
        return lib.enf_eval_loss_a(ctypes.byref(desc), x, 0, p, a, sigma, blob, y, o, w, cw, loss, err, lb, ws, nbytes, flags, None)
    assert call(desc=mk(O=33), nbytes=big) == EUNSUPPORTED and call(desc=mk(O=33), o="null", y=None, loss=None, err=None, lb=None) == EUNSUPPORTED
    assert call(o="null") == EINVAL
    for bad in (op(M=0), op(nnz=-1), op(row_ptr=True), op(col=True), op(val=True)):
        assert call(o=bad) == EINVAL and call(o=bad, nbytes=big) == EINVAL
    assert call(o=op(col_ptr=True, trow=True, tval=True)) == EWORKSPACE       # the evaluation needs no CSC
    assert call(w=P, cw=P) == EINVAL
    for k in ("y", "x", "p", "a", "sigma", "blob", "ws"):
        assert call(**{k: None}) == EINVAL, k
    assert call(loss=None, err=None, lb=None) == EINVAL                        # all three outputs NULL
    for kw in ({"loss": None}, {"err": None}, {"lb": None}, {"loss": None, "err": None}, {"err": None, "lb": None}, {"w": P}, {"cw": P}):
        assert call(**kw) == EWORKSPACE, kw
    for flags in (1, 2, 8, 32, SHARED, SHARED | DET):
        assert call(flags=flags) == EINVAL, flags
    d = mk()
    for flags in (0, DET):
        assert call(flags=flags, nbytes=lib.enf_obs_workspace_bytes(ctypes.byref(d), 5, flags) - 1) == EWORKSPACE


def test_unfused_entry_points_refuse_before_any_launch():
    lib = _lib.load()
    dummy, P, mk, op = _setup()
    good = op()
    ref = ctypes.byref(good)
    assert lib.enf_obs_apply(None, 3, 48, 2, ref, P, None) == EINVAL and lib.enf_obs_apply(P, 3, 48, 2, ref, None, None) == EINVAL
    assert lib.enf_obs_apply(P, 3, 48, 2, None, P, None) == EINVAL
    for B, N, O in ((0, 48, 2), (3, 0, 2), (3, 48, 0)):
        assert lib.enf_obs_apply(P, B, N, O, ref, P, None) == EINVAL
    for bad in (op(M=0), op(nnz=-1), op(row_ptr=True), op(col=True), op(val=True)):
        assert lib.enf_obs_apply(P, 3, 48, 2, ctypes.byref(bad), P, None) == EINVAL

    def mse(out=P, y=P, B=3, N=48, O=2, o=ref, w=None, cw=None, dout=P, loss=P, err=P, scr=P, nbytes=1 << 40, flags=0):
        return lib.enf_mse_value_grad_a(out, y, B, N, O, o, w, cw, 1.0, dout, loss, err, scr, nbytes, flags, None)
    for kw in (dict(out=None), dict(y=None), dict(loss=None), dict(o=None), dict(B=0), dict(N=0), dict(O=0), dict(w=P, cw=P), dict(flags=1),
               dict(flags=DET | 2), dict(scr=None), dict(scr=None, dout=None, flags=DET)):
        assert mse(**kw) == EINVAL, kw
    for bad in (op(M=0), op(nnz=-1), op(col_ptr=True), op(trow=True), op(tval=True), op(val=True)):
        assert mse(o=ctypes.byref(bad)) == EINVAL
    # the size query: r (B M O) where d out is wanted, the partials in deterministic mode
    q = lib.enf_mse_a_scratch_bytes
    assert q(3, 5, 2, 0, 0) == 0 and q(3, 5, 2, 1, 0) == 256 and q(3, 5, 2, 0, DET) == 4096 and q(3, 5, 2, 1, DET) == 4352
    assert q(0, 5, 2, 1, 0) == 0 and q(3, 5, 2, 1, 2) == 0
    assert mse(nbytes=255) == EWORKSPACE and mse(flags=DET, nbytes=4351) == EWORKSPACE and mse(dout=None, flags=DET, nbytes=4095) == EWORKSPACE


# ---- 6. the Python layers: shapes are checked before anything touches the device
def test_python_layers_check_shapes_first():
    from tests.test_gpu_layers import _nef as layered
    Bn, N, Zn = 2, 8, 3
    x, p, a, s = torch.zeros(Bn, N, 2), torch.zeros(Bn, Zn, 2), torch.ones(Bn, Zn, 8), torch.ones(Bn, Zn, 1)
    op = SparseObservations.from_groups([3, 0, 5], None)
    y = torch.zeros(Bn, 3, 2)
    nef = build_nef(make_cfg("rel_pos_periodic", D=64, H=2, C=8, O=2), "f32")
    deep = layered(dict(make_cfg("rel_pos_periodic", D=64, H=2, C=8, O=2), num_layers=1), "f32")
    for fn, dfn in ((nef.mse_value_and_operator_grads, deep.mse_value_and_operator_grads), (nef.eval_operator_loss, deep.eval_operator_loss)):
        with pytest.raises(NotImplementedError, match="num_layers"):
            dfn(None, x, p, a, s, y, op)
        with pytest.raises(ValueError, match="columns"):
            fn(None, x[:, :7], p, a, s, y, op)
        with pytest.raises(ValueError, match="target"):
            fn(None, x, p, a, s, torch.zeros(Bn, 4, 2), op)
        with pytest.raises(ValueError, match="obs_weight"):
            fn(None, x, p, a, s, y, op, obs_weight=torch.ones(Bn, N))
        with pytest.raises(ValueError, match="obs_channel_weight"):
            fn(None, x, p, a, s, y, op, obs_channel_weight=torch.ones(Bn, 3))
        with pytest.raises(ValueError, match="not both"):
            fn(None, x, p, a, s, y, op, obs_weight=torch.ones(Bn, 3), obs_channel_weight=torch.ones(Bn, 3, 2))
        with pytest.raises(_lib.EnfError):                                   # host tensors: there is no CPU path
            fn(None, x, p, a, s, y, op)
    out = torch.zeros(Bn, N, 2)
    for kw, match in ((dict(out=out[:, :7]), "operator"), (dict(target=torch.zeros(Bn, 4, 2)), "target"), (dict(obs_weight=torch.ones(Bn, N)), "obs_weight"),
                      (dict(obs_weight=torch.ones(Bn, 3), obs_channel_weight=torch.ones(Bn, 3, 2)), "not both")):
        with pytest.raises(ValueError, match=match):
            nef.operator_mse(**dict(dict(out=out, target=y, op=op), **kw))
    with pytest.raises(_lib.EnfError):
        nef.operator_mse(out, y, op)
    # the fitting layer: the observation value, and who does not take it yet
    with pytest.raises(ValueError, match="operator"):
        LinearObservations(x[0, :7], op)
    with pytest.raises(NotImplementedError, match="fit_linear_observations"):
        observed(x[0], None, None, LinearObservations(x[0], op), None, Bn, 3, 2)
    with pytest.raises(NotImplementedError, match="fit_linear_observations"):
        observed(x[0], None, None, (x[0], op), None, Bn, 3, 2)
    lat0 = {"p_pos": p[:1], "a": a[:1], "gaussian_window": s[:1]}
    with pytest.raises(ValueError, match="observations"):
        fit_linear_observations(nef, None, lat0, lat0, x[0], op, torch.zeros(Bn, 4, 2), 1)
    with pytest.raises(ValueError, match="not both"):
        fit_linear_observations(nef, None, lat0, lat0, x[0], op, y, 1, obs_weight=torch.ones(Bn, 3), obs_channel_weight=torch.ones(Bn, 3, 2))
