"""The Gauss-Newton product on sparse observation operators and the Levenberg-Marquardt fit on one, on the GPU (include/enf_hip.h,
"Gauss-Newton product on sparse observations"): EquivariantCrossAttentionNeF.gn_operator_product against the fp64 product of the oracle
on the dense operator (tests/gn_operators_ref.py, pinned by tests/test_gn_operators_host.py), against the composed route through the
shipped entry points (nef.tangent, A, the weights and A^T in torch, apply().backward), against nef.gn_cell_product on an operator of
equal groups and nef.gn_product on the identity; lm_fit_linear_observations against the inner loop's SGD rule.

Error measure and bounds are those of tests/test_gpu_gn.py: the relative Frobenius norm per component gp, ga, gsigma; 7e-4 (f32) and
1.4e-1 (bf16) against the oracle; 1e-5 against a composed route in f32 (the same fp32 sums in another order)."""
import ctypes

import numpy as np
import pytest
import torch

from enf_pde_amd import _lib
from enf_pde_amd.fitting import SparseObservations, lm_fit_linear_observations
from tests import gn_cells_ref
from tests.helpers import build_nef
from tests.gn_operators_ref import case, fit_case, oracle_lm_operator
from tests.test_gpu_gn import NAMES, TOL, _check, _t

pytestmark = pytest.mark.gpu

# the lane form (0 .. 64 entries), both sides of ENF_OBS_TREE_MIN = 65, a row longer than N = 80 (repeated columns), an empty row
LENGTHS = ([0, 1, 2, 3, 9, 27, 63, 64, 65, 70, 100] * 2)[:22]
SHORT = [0, 1, 2, 3, 9, 5, 4, 2] * 2          # rows that leave many columns to one row only
_LM = {}


def _model(cuda, c, precision, deterministic=None, variants=None):
    nef = build_nef(c.cfg, precision)
    nef.deterministic = deterministic
    if variants is not None:
        nef.pair_variants = variants
    return nef, nef.load_params(c.prm, device=cuda)


def _op(cuda, c, vals=None):
    return SparseObservations.from_coo(c.rows, c.cols, c.vals if vals is None else vals, c.M, c.N, device=cuda)


def _gno(cuda, c, nef, P, op, v=None, x=None, w="case", reuse=None):
    """nef.gn_operator_product on a case of tests/gn_operators_ref.py: its own tangents and weights unless given; w (B, M) or (B, M, O)"""
    t = _t(cuda)
    vp, va, vs = c.v if v is None else v
    w = c.w if isinstance(w, str) else w
    kw = {} if w is None else ({"obs_weight": t(w)} if np.asarray(w).ndim == 2 else {"obs_channel_weight": t(w)})
    return nef.gn_operator_product(P, t(c.x) if x is None else x, t(c.p), t(c.a), t(c.s) if c.cfg["use_gaussian_window"] else None, op,
                                   vp=t(vp), va=t(va), vwindow=t(vs), grad_scale=c.gs, reuse=reuse, **kw)


def _equal(r0, r1):
    return all(torch.equal(a_, b_) for a_, b_ in zip(r0, r1))


def _composed(cuda, c, nef, P, op):
    """nef.tangent -> fp32 A, the weights' select and A^T as elementwise torch sums -> the latent backward of nef.apply"""
    t = _t(cuda)
    _, tan = nef.tangent(P, t(c.x), t(c.p), t(c.a), t(c.s), dp=t(c.v[0]), da=t(c.v[1]), dwindow=t(c.v[2]))
    A = torch.tensor(op.to_dense(dtype=np.float32), dtype=torch.float32, device=cuda)             # (M, N): the factors the kernels read
    obs_tan = (A[None, :, :, None] * tan[:, None, :, :]).sum(2)
    w = torch.ones_like(obs_tan) if c.w is None else (t(c.w)[..., None] if c.w.ndim == 2 else t(c.w)).expand_as(obs_tan)
    r = torch.where(w > 0, w * obs_tan, torch.zeros_like(obs_tan))
    gs = (torch.tensor(2.0 * c.gs, dtype=torch.float32) / (float(c.B) * c.M * c.O)).to(cuda)
    seed = (A[None, :, :, None] * r[:, :, None, :]).sum(1) * gs
    hp, ha, hs = (t(u).requires_grad_(True) for u in (c.p, c.a, c.s))
    nef.apply(P, t(c.x), hp, ha, hs).backward(seed)
    return [h.grad.double().cpu().numpy() for h in (hp, ha, hs)], tan


# ---- 1. oracle parity
@pytest.mark.parametrize("O", [1, 2, 4, 5])
@pytest.mark.parametrize("precision", ["f32", "bf16"])
@pytest.mark.parametrize("inv", ["rel_pos_periodic", "latitude_periodic"])
def test_gn_operator_product_matches_oracle(cuda, inv, precision, O):
    """N = 80: the second 64-query tail block is partial and B N = 240 clamps rows.  M = 22 rows of LENGTHS, columns unsorted, three
    spare columns in no row (their d out is written as zero: the product would otherwise carry what the workspace held).  Weights per
    observation, per value, none.  O = 1: the scalar pass; 4: the 16-byte pass; 2, 5: four channels per pass, the last one short."""
    nef = P = None
    for weights in ("obs", "value", None):
        c = case(inv, LENGTHS, 80, O=O, weights=weights)
        if nef is None:
            nef, P = _model(cuda, c, precision)
        assert c.M == 22 and (c.A[:, -3:] == 0).all()
        _check(_gno(cuda, c, nef, P, _op(cuda, c)), c.ref, TOL[precision], f"{inv} {precision} O={O} weights={weights}")


# ---- 2. the composed route through public entry points, f32, in both variants of the backward pair kernel
@pytest.mark.parametrize("variant", ["z_fold", "latent_split"])
@pytest.mark.parametrize("inv,weights", [("rel_pos_periodic", "obs"), ("latitude_periodic", "value")])
def test_gn_operator_product_equals_tangent_operator_then_latent_backward(cuda, inv, weights, variant):
    c = case(inv, LENGTHS, 80, weights=weights)
    nef, P = _model(cuda, c, "f32", variants=("auto", variant))
    desc = nef._desc(3, 80, 7)
    assert _lib.load().enf_pair_variant(ctypes.byref(desc), 1) == _lib.VARIANT[variant]
    op = _op(cuda, c)
    got = _gno(cuda, c, nef, P, op)
    ref, _ = _composed(cuda, c, nef, P, op)
    _check(got, ref, 1e-5, f"{inv} weights={weights} {variant}: against tangent -> A^T w A tan coef -> latent backward")


# ---- 3. operators that are cells, and the identity
def test_gn_operator_product_on_equal_groups_is_the_cell_product(cuda):
    """from_groups(G = 4, q) with signal 0's factors against gn_cell_product with those factors for every signal and the same w: the
    same sums through other kernels -- 1e-5; equal bits are not promised (printed)."""
    c = gn_cells_ref.case("rel_pos_periodic", 4, 80)
    nef = build_nef(c.cfg, "f32")
    nef.deterministic = True
    P = nef.load_params(c.prm, device=cuda)
    t = _t(cuda)
    q0 = c.q[0]
    op = SparseObservations.from_groups(np.full(c.M, 4), q0, device=cuda)
    args = (P, t(c.x), t(c.p), t(c.a), t(c.s))
    kw = dict(vp=t(c.v[0]), va=t(c.v[1]), vwindow=t(c.v[2]), grad_scale=c.gs)
    ref = nef.gn_cell_product(*args, 4, qweight=t(np.repeat(q0[None], 3, 0)), obs_weight=t(c.w), **kw)
    got = nef.gn_operator_product(*args, op, obs_weight=t(c.w), **kw)
    _check(got, [r.double().cpu().numpy() for r in ref], 1e-5, "from_groups(4, q) against gn_cell_product")
    print("from_groups(4, q): equal bits " + ", ".join(f"{n} {torch.equal(g, r)}" for n, g, r in zip(NAMES, got, ref)))


def test_gn_operator_product_on_the_identity_is_the_per_point_product(cuda):
    c = gn_cells_ref.case("ponita", 1, 50)
    nef = build_nef(c.cfg, "f32")
    nef.deterministic = True
    P = nef.load_params(c.prm, device=cuda)
    t = _t(cuda)
    op = SparseObservations.from_groups(np.ones(50, dtype=np.int64), np.ones(50), device=cuda)
    args = (P, t(c.x), t(c.p), t(c.a), t(c.s))
    kw = dict(vp=t(c.v[0]), va=t(c.v[1]), vwindow=t(c.v[2]), grad_scale=c.gs)
    ref = nef.gn_product(*args, weight=t(c.w), **kw)
    got = nef.gn_operator_product(*args, op, obs_weight=t(c.w), **kw)
    _check(got, [r.double().cpu().numpy() for r in ref], 1e-5, "the identity against gn_product(weight=w)")
    print("identity: equal bits " + ", ".join(f"{n} {torch.equal(g, r)}" for n, g, r in zip(NAMES, got, ref)))


# ---- 4. symmetry and the quadratic form
@pytest.mark.parametrize("precision", ["f32", "bf16"])
@pytest.mark.parametrize("inv", ["rel_pos_periodic", "latitude_periodic"])
def test_gn_operator_product_is_symmetric_and_positive(cuda, inv, precision):
    """the bounds of test_gn_cell_product_is_symmetric_and_positive: 7e-4 in f32, printed in bf16"""
    c = case(inv, LENGTHS, 80)
    rng = np.random.default_rng(13)
    u = tuple(rng.standard_normal(q.shape) * sc for q, sc in zip(c.v, (0.3, 1.0, 0.1)))
    nef, P = _model(cuda, c, precision)
    t = _t(cuda)
    op = _op(cuda, c)
    Gv = [g.double() for g in _gno(cuda, c, nef, P, op)]
    Gu = [g.double() for g in _gno(cuda, c, nef, P, op, v=u)]
    dot = lambda A, B_: float(sum((a_ * b_).sum() for a_, b_ in zip(A, B_)))
    nrm = lambda A: float(np.sqrt(sum(float((a_ * a_).sum()) for a_ in A)))
    vt, ut = [t(q).double() for q in c.v], [t(q).double() for q in u]
    asym = abs(dot(ut, Gv) - dot(Gu, vt))
    scale = nrm(ut) * nrm(Gv) + nrm(vt) * nrm(Gu)
    _, tan = nef.tangent(P, t(c.x), t(c.p), t(c.a), t(c.s), dp=t(c.v[0]), da=t(c.v[1]), dwindow=t(c.v[2]))
    obs_tan = torch.einsum("mn,bno->bmo", torch.tensor(op.to_dense(), dtype=torch.float64, device=cuda), tan.double())
    quad = c.gs * 2.0 / (3 * c.M * c.O) * float((t(c.w).double()[..., None] * obs_tan ** 2).sum())
    vGv = dot(vt, Gv)
    print(f"{inv} {precision}: |<u,Gv> - <Gu,v>| / (|u||Gv| + |v||Gu|) = {asym / scale:.3e}, <v,Gv> = {vGv:.6e} against "
          f"coef sum w obs_tan^2 = {quad:.6e}: {abs(vGv - quad) / quad:.3e} (bounds 7.0e-04, f32 only)")
    if precision == "f32":
        assert asym <= 7e-4 * scale and abs(vGv - quad) <= 7e-4 * quad and vGv >= 0


# ---- 5. the other instantiations
@pytest.mark.parametrize("name,inv,shape,precision", [
    ("128x2", "rel_pos_periodic", dict(D=128, H=2), "f32"),
    ("128x2", "rel_pos_periodic", dict(D=128, H=2), "bf16"),
    ("128x1", "rel_pos_periodic", dict(D=128, H=1), "f32"),
    ("128x1", "rel_pos_periodic", dict(D=128, H=1), "bf16"),
    ("64x4", "rel_pos_periodic", dict(D=64, H=4), "f32"),
    ("64x4", "rel_pos_periodic", dict(D=64, H=4), "bf16"),
    ("64x1", "rel_pos_periodic", dict(D=64, H=1), "f32"),
    ("64x1", "rel_pos_periodic", dict(D=64, H=1), "bf16"),
    ("16x2 padded", "polar_periodic", dict(D=16, H=2), "f32")])
def test_gn_operator_product_other_instantiations(cuda, name, inv, shape, precision):
    """B Z = 2 x 96 = 192: the descriptor resolves to the z-fold backward by itself.  N = 40: one partial tail block."""
    c = case(inv, [0, 1, 3, 9, 27, 45, 5, 2], 40, Bn=2, Zn=96, **shape)
    assert (c.w == 0).any() and (c.w > 0).any()
    nef, P = _model(cuda, c, precision)
    desc = nef._desc(2, 40, 96)
    assert _lib.load().enf_pair_variant(ctypes.byref(desc), 1) == _lib.VARIANT["z_fold"]
    _check(_gno(cuda, c, nef, P, _op(cuda, c)), c.ref, TOL[precision], f"{name} {precision} N=40 Z=96")


# ---- 6. what has weight zero does not exist
@pytest.mark.parametrize("weights", ["obs", "value"])
def test_gn_operator_product_ignores_what_has_weight_zero(cuda, weights):
    """Deterministic mode, f32.  The rows `dead` have weight 0 in every signal (every value of them with per-value weights) beside the
    case's own scattered zeros.  Moving x at the columns that only dead rows touch, or replacing the dead rows' factors by other
    finite values, changes no bit; moving the other columns does change ga."""
    c = case("rel_pos_periodic", SHORT, 80, weights=weights)
    dead = np.array([3, 4, 9, 12])
    w = c.w.copy()
    w[:, dead] = 0.0
    in_dead = np.isin(c.rows, dead)
    only_dead = np.setdiff1d(c.cols[in_dead], c.cols[~in_dead])               # columns no live row touches
    live_cols = np.unique(c.cols[~in_dead])
    assert only_dead.size >= 3 and live_cols.size >= 3 and (w > 0).any()
    nef, P = _model(cuda, c, "f32", deterministic=True)
    t = _t(cuda)
    op = _op(cuda, c)
    shift = lambda cols_: t(c.x + np.where(np.isin(np.arange(80), cols_)[None, :, None], 0.37, 0.0))
    g0 = _gno(cuda, c, nef, P, op, w=w)
    g1 = _gno(cuda, c, nef, P, op, w=w, x=shift(only_dead))
    g2 = _gno(cuda, c, nef, P, _op(cuda, c, vals=np.where(in_dead, -3.0 * c.vals + 0.5, c.vals).astype(np.float32)), w=w)
    assert _equal(g0, g1) and _equal(g0, g2) and float(g0[1].abs().max()) > 0
    g3 = _gno(cuda, c, nef, P, op, w=w, x=shift(live_cols))
    assert not torch.equal(g0[1], g3[1])


# ---- 7. determinism
@pytest.mark.parametrize("precision", ["f32", "bf16"])
@pytest.mark.parametrize("variant", ["z_fold", "latent_split"])
def test_gn_operator_product_deterministic_mode_equal_bits(cuda, precision, variant):
    c = case("rel_pos_periodic", LENGTHS, 80)
    nef, P = _model(cuda, c, precision, deterministic=True, variants=("auto", variant))
    op = _op(cuda, c)
    runs = [_gno(cuda, c, nef, P, op), _gno(cuda, c, nef, P, op)]
    assert len(nef._ws_cache) == 1
    for byte in (0x00, 0xFF):
        for ws in nef._ws_cache.values():
            ws.fill_(byte)
        runs.append(_gno(cuda, c, nef, P, op))
    for r in runs[1:]:
        assert _equal(r, runs[0])
    assert all(torch.isfinite(g).all() for g in runs[0]) and float(runs[0][1].abs().max()) > 0


# ---- 8. reuse of the point
@pytest.mark.parametrize("variant", ["z_fold", "latent_split"])
def test_gn_operator_product_reuse_point_after_an_operator_fit_step_gives_the_same_bits(cuda, variant):
    c = case("ponita", LENGTHS, 80)
    nef, P = _model(cuda, c, "f32", deterministic=True, variants=("auto", variant))
    t = _t(cuda)
    op = _op(cuda, c)
    plain = _gno(cuda, c, nef, P, op)
    tag0 = nef.gn_reserve(3, 80, 7, cuda, op=op)
    target = t(np.random.default_rng(3).standard_normal((3, c.M, c.O)))
    nef.mse_value_and_operator_grads(P, t(c.x), t(c.p), t(c.a), t(c.s), target, op, obs_weight=t(c.w), grad_scale=3.0)
    tag = nef.workspace_tag(cuda)                               # enf_fit_step_a ran on that buffer
    assert tag != tag0 and len(nef._ws_cache) == 1
    reused = _gno(cuda, c, nef, P, op, reuse=tag)
    again = _gno(cuda, c, nef, P, op, reuse=nef.workspace_tag(cuda))                                   # behind an earlier product
    stale = _gno(cuda, c, nef, P, op, reuse=tag)                                                       # a stale tag recomputes
    assert len(nef._ws_cache) == 1
    for r in (reused, again, stale):
        assert _equal(r, plain)


# ---- 9. a broadcast grid
def test_gn_operator_product_broadcast_grid_equals_materialised(cuda):
    c = case("ponita", LENGTHS, 80)
    nef, P = _model(cuda, c, "f32", deterministic=True)
    op = _op(cuda, c)
    x = _t(cuda)(c.x[0])
    g0 = _gno(cuda, c, nef, P, op, x=x[None].expand(3, -1, -1))
    g1 = _gno(cuda, c, nef, P, op, x=x[None].repeat(3, 1, 1))
    assert _equal(g0, g1) and float(g0[0].abs().max()) > 0


# ---- 10. end to end
def _sgd(nef, P, x, op, tgt, p, a, s, steps):
    B = p.shape[0]
    for _ in range(steps):
        _, gp, ga, _ = nef.mse_value_and_operator_grads(P, x, p, a, s, tgt, op, grad_scale=float(B))
        p, a = p - gp, a - 5.0 * ga
    return nef.eval_operator_loss(P, x, p, a, s, tgt, op)[0]


@pytest.mark.parametrize("precision", ["f32", "bf16"])
@pytest.mark.parametrize("inv", ["rel_pos_periodic", "ponita"])
def test_lm_fit_linear_observations_end_to_end(cuda, inv, precision):
    """The rows (p, a, s, x) of tests/gn_cells_ref.fit_case(inv) (N = 80); the operator's rows from
    ragged_entries([1, 3, 9, 27, 5, 70] * 4, 80, 301, spare=0), their factors made positive and normalised to row sum 1.
    default_rng(21): p* = p + 0.05 N(0,1), a* = a + 0.5 N(0,1), target = the fp64 A out of the oracle's decode at (p*, a*, s); four LM
    steps of eight CG iterations from (p, a, s).  Both precisions: shapes, finite, the window untouched, no signal's loss ever increases.
    f32: every signal ends below 48 steps of the inner loop's SGD rule (p -= g_p, a -= 5 g_a at gradient scale B) run on the GPU
    through mse_value_and_operator_grads.
    The fp64 reference alone (oracle_lm_operator against oracle_sgd_operator) leaves, per signal, the factors 5.0, 3.9, 5.2
    (rel_pos_periodic) and 11.1, 17.6, 10.5 (ponita) between the two, every LM step accepted: at least 2, with room."""
    f = fit_case(inv)
    nef = build_nef(f.cfg, precision)
    P = nef.load_params(f.prm, device=cuda)
    t = _t(cuda)
    op = SparseObservations.from_coo(f.rows, f.cols, f.vals, f.M, f.N, device=cuda)
    (p1, a1, s1), loss_b, lam, acc = lm_fit_linear_observations(nef, P, t(f.x), op, t(f.target), t(f.p), t(f.a), t(f.s), steps=4, cg_iters=8)
    lb = loss_b.double().cpu().numpy()
    if inv not in _LM:
        _LM[inv] = oracle_lm_operator(f.cfg, f.prm, f.x, f.A, f.target, f.p, f.a, f.s, 4)
    ref, ref_acc = _LM[inv]
    for k in range(5):
        print(f"{inv} {precision} step {k}: GPU " + " ".join(f"{v:.3e}" for v in lb[k]) + "   fp64 " + " ".join(f"{v:.3e}" for v in ref[k]))
    print(f"accepted: GPU {acc.cpu().numpy().astype(int).tolist()}  fp64 {ref_acc.astype(int).tolist()}; damping {lam.cpu().numpy()}")
    assert lb.shape == (5, 3) and acc.shape == (4, 3) and p1.shape == f.p.shape and a1.shape == f.a.shape
    assert np.isfinite(lb).all() and bool(torch.isfinite(p1).all()) and bool(torch.isfinite(a1).all()) and torch.equal(s1, t(f.s))
    assert (lb[1:] <= lb[:-1]).all()
    if precision == "f32":
        sgd = _sgd(nef, P, t(f.x), op, t(f.target), t(f.p), t(f.a), t(f.s), 48).double().cpu().numpy()
        print("48 SGD steps: " + " ".join(f"{v:.3e}" for v in sgd))
        assert (lb[-1] < sgd).all()
