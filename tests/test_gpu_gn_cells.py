"""The Gauss-Newton product on grouped observations and the Levenberg-Marquardt fit on cell averages on the GPU (include/enf_hip.h,
"Gauss-Newton product on grouped observations"): EquivariantCrossAttentionNeF.gn_cell_product against the fp64 product of the oracle
(tests/gn_cells_ref.py, pinned by tests/test_gn_cells_host.py), against the composed route through the shipped entry points
(nef.tangent, the group sum and the seed in torch, apply().backward) and against nef.gn_product at G = 1; lm_fit_cell_averages against
the inner loop's SGD rule.

Error measure and bounds are those of tests/test_gpu_gn.py: the relative Frobenius norm per component gp, ga, gsigma; 7e-4 (f32) and
1.4e-1 (bf16) against the oracle; 1e-5 against a composed route in f32 (the same fp32 sums in another order)."""
import ctypes

import numpy as np
import pytest
import torch

from enf_pde_amd import _lib
from tests.helpers import build_nef
from tests.gn_cells_ref import case, fit_case, oracle_lm_cells
from tests.test_gpu_gn import NAMES, TOL, _check, _t

pytestmark = pytest.mark.gpu

BIG = dict(D=128, H=2, B=2, Z=9)          # with G = 8, N = 128 + 16: the f32 instantiation that fills the register file, two workgroups


def _model(cuda, c, precision, deterministic=None, variants=None):
    nef = build_nef(c.cfg, precision)
    nef.deterministic = deterministic
    if variants is not None:
        nef.pair_variants = variants
    return nef, nef.load_params(c.prm, device=cuda)


def _gnc(cuda, c, nef, P, v=None, x=None, q="case", w="case", reuse=None):
    """nef.gn_cell_product on a case of tests/gn_cells_ref.py: its own tangents, factors and weights unless given"""
    t = _t(cuda)
    vp, va, vs = c.v if v is None else v
    return nef.gn_cell_product(P, t(c.x) if x is None else x, t(c.p), t(c.a), t(c.s) if c.cfg["use_gaussian_window"] else None, c.G,
                               qweight=t(c.q) if isinstance(q, str) else q, obs_weight=t(c.w) if isinstance(w, str) else w, vp=t(vp),
                               va=t(va), vwindow=t(vs), grad_scale=c.gs, reuse=reuse)


def _pair_tree(s):
    """(B, M, G, O) -> (B, M, O) in the order of the tail's xor tree: neighbours at distance 1, then 2, 4, 8"""
    while s.shape[2] > 1:
        s = s[:, :, 0::2] + s[:, :, 1::2]
    return s[:, :, 0]


def _equal(r0, r1):
    return all(torch.equal(a_, b_) for a_, b_ in zip(r0, r1))


# ---- 1. oracle parity
@pytest.mark.parametrize("precision", ["f32", "bf16"])
@pytest.mark.parametrize("inv", ["rel_pos_periodic", "latitude_periodic"])
def test_gn_cell_product_matches_oracle(cuda, inv, precision):
    """(G, N): (4, 80); (16, 48) a group that fills a tile; (2, 50) and (8, 24) tiles that straddle signals; B N = 150, 72 a clamped
    last tile.  Then (4, 80) with the plain mean and no weights."""
    nef = P = None
    for G, N in ((4, 80), (16, 48), (2, 50), (8, 24)):
        c = case(inv, G, N)
        if nef is None:
            nef, P = _model(cuda, c, precision)
        _check(_gnc(cuda, c, nef, P), c.ref, TOL[precision], f"{inv} {precision} G={G} N={N}")
    c = case(inv, 4, 80, weights=False)
    _check(_gnc(cuda, c, nef, P, q=None, w=None), c.ref, TOL[precision], f"{inv} {precision} G=4 N=80 qweight=None obs_weight=None")


# ---- 2. the composed route through public entry points, f32, in both variants of the backward pair kernel
@pytest.mark.parametrize("variant", ["z_fold", "latent_split"])
@pytest.mark.parametrize("inv,G,N", [("rel_pos_periodic", 4, 80), ("latitude_periodic", 8, 24)])
def test_gn_cell_product_equals_tangent_group_sum_then_latent_backward(cuda, inv, G, N, variant):
    c = case(inv, G, N)
    nef, P = _model(cuda, c, "f32", variants=("auto", variant))
    desc = nef._desc(3, N, 7)
    assert _lib.load().enf_pair_variant(ctypes.byref(desc), 1) == _lib.VARIANT[variant]
    t = _t(cuda)
    got = _gnc(cuda, c, nef, P)
    _, tan = nef.tangent(P, t(c.x), t(c.p), t(c.a), t(c.s), dp=t(c.v[0]), da=t(c.v[1]), dwindow=t(c.v[2]))
    q, w = t(c.q)[..., None], t(c.w)[..., None]
    obs_tan = _pair_tree((q * tan).reshape(3, c.M, G, c.O))
    gs = torch.tensor(2.0 * c.gs, dtype=torch.float32) / (3.0 * c.M * c.O)
    wo = torch.where(w > 0, w * obs_tan, torch.zeros_like(obs_tan)).repeat_interleave(G, dim=1)
    seed = (q * wo) * gs.to(cuda)
    hp, ha, hs = (t(u).requires_grad_(True) for u in (c.p, c.a, c.s))
    nef.apply(P, t(c.x), hp, ha, hs).backward(seed)
    ref = [h.grad.double().cpu().numpy() for h in (hp, ha, hs)]
    _check(got, ref, 1e-5, f"{inv} G={G} N={N} {variant}: against tangent -> q w sum_k q tan coef -> latent backward")


# ---- 3. groups of one
@pytest.mark.parametrize("inv", ["rel_pos_periodic", "ponita"])
def test_gn_cell_product_with_groups_of_one_is_the_per_point_product(cuda, inv):
    """G = 1 with q = 1 or None against nef.gn_product(weight = w): another instantiation, the same arithmetic up to the order of two
    products -- 1e-5; equal bits are not promised (printed)."""
    c = case(inv, 1, 50)
    nef, P = _model(cuda, c, "f32", deterministic=True)
    t = _t(cuda)
    ref = nef.gn_product(P, t(c.x), t(c.p), t(c.a), t(c.s), vp=t(c.v[0]), va=t(c.v[1]), vwindow=t(c.v[2]), weight=t(c.w), grad_scale=c.gs)
    refn = [r.double().cpu().numpy() for r in ref]
    for label, q in (("ones", torch.ones((3, 50), device=cuda)), ("None", None)):
        got = _gnc(cuda, c, nef, P, q=q)
        _check(got, refn, 1e-5, f"{inv} G=1 q={label} against gn_product(weight=w)")
        print(f"{inv} G=1 q={label}: equal bits " + ", ".join(f"{n} {torch.equal(g, r)}" for n, g, r in zip(NAMES, got, ref)))


# ---- 4. symmetry and the quadratic form
@pytest.mark.parametrize("precision", ["f32", "bf16"])
@pytest.mark.parametrize("inv", ["rel_pos_periodic", "latitude_periodic"])
def test_gn_cell_product_is_symmetric_and_positive(cuda, inv, precision):
    c = case(inv, 4, 80)
    rng = np.random.default_rng(13)
    u = tuple(rng.standard_normal(q.shape) * sc for q, sc in zip(c.v, (0.3, 1.0, 0.1)))
    nef, P = _model(cuda, c, precision)
    t = _t(cuda)
    Gv = [g.double() for g in _gnc(cuda, c, nef, P)]
    Gu = [g.double() for g in _gnc(cuda, c, nef, P, v=u)]
    dot = lambda A, B_: float(sum((a_ * b_).sum() for a_, b_ in zip(A, B_)))
    nrm = lambda A: float(np.sqrt(sum(float((a_ * a_).sum()) for a_ in A)))
    vt, ut = [t(q).double() for q in c.v], [t(q).double() for q in u]
    asym = abs(dot(ut, Gv) - dot(Gu, vt))
    scale = nrm(ut) * nrm(Gv) + nrm(vt) * nrm(Gu)
    _, tan = nef.tangent(P, t(c.x), t(c.p), t(c.a), t(c.s), dp=t(c.v[0]), da=t(c.v[1]), dwindow=t(c.v[2]))
    obs_tan = (t(c.q).double()[..., None] * tan.double()).reshape(3, c.M, c.G, c.O).sum(2)
    quad = c.gs * 2.0 / (3 * c.M * c.O) * float((t(c.w).double()[..., None] * obs_tan ** 2).sum())
    vGv = dot(vt, Gv)
    print(f"{inv} {precision}: |<u,Gv> - <Gu,v>| / (|u||Gv| + |v||Gu|) = {asym / scale:.3e}, <v,Gv> = {vGv:.6e} against "
          f"coef sum w obs_tan^2 = {quad:.6e}: {abs(vGv - quad) / quad:.3e} (bounds 7.0e-04, f32 only)")
    if precision == "f32":
        assert asym <= 7e-4 * scale and abs(vGv - quad) <= 7e-4 * quad and vGv >= 0


# ---- 5. the other instantiations and the edges
@pytest.mark.parametrize("name,inv,G,N,shape,precision", [
    ("128x2", "rel_pos_periodic", 8, 144, BIG, "f32"),
    ("128x2", "rel_pos_periodic", 8, 144, BIG, "bf16"),
    ("128x1", "rel_pos_periodic", 4, 40, dict(D=128, H=1, B=2, Z=5), "f32"),
    ("128x1", "rel_pos_periodic", 4, 40, dict(D=128, H=1, B=2, Z=5), "bf16"),
    ("64x4", "rel_pos_periodic", 4, 40, dict(D=64, H=4, B=2, Z=5), "f32"),
    ("64x4", "rel_pos_periodic", 4, 40, dict(D=64, H=4, B=2, Z=5), "bf16"),
    ("64x1", "rel_pos_periodic", 4, 40, dict(D=64, H=1, B=2, Z=5), "f32"),
    ("64x1", "rel_pos_periodic", 4, 40, dict(D=64, H=1, B=2, Z=5), "bf16"),
    ("16x2 padded", "polar_periodic", 4, 40, dict(D=16, H=2, B=2, Z=5), "f32"),
    ("one latent", "rel_pos_periodic", 4, 20, dict(D=64, H=2, B=2, Z=1), "f32"),
    ("one observation per signal", "rel_pos_periodic", 16, 16, dict(), "f32")])
def test_gn_cell_product_other_instantiations(cuda, name, inv, G, N, shape, precision):
    c = case(inv, G, N, **shape)
    assert (c.w == 0).any() and (c.w > 0).any()
    nef, P = _model(cuda, c, precision)
    _check(_gnc(cuda, c, nef, P), c.ref, TOL[precision], f"{name} {precision} G={G} N={N}")


# ---- 6. observations of weight zero do not exist
def test_gn_cell_product_ignores_observations_of_weight_zero(cuda):
    """Deterministic mode, f32, (4, 80): moving x on all rows of the zero-weight observations, or replacing their factors by other
    positive finite values, changes no bit; moving the other rows does change ga."""
    c = case("rel_pos_periodic", 4, 80)
    nef, P = _model(cuda, c, "f32", deterministic=True)
    t = _t(cuda)
    gone = np.repeat(c.w == 0, c.G, axis=1)                     # (B, N): the rows of the observations that do not exist
    assert gone.any() and not gone.all()
    g0 = _gnc(cuda, c, nef, P)
    g1 = _gnc(cuda, c, nef, P, x=t(c.x + np.where(gone[..., None], 0.37, 0.0)))
    g2 = _gnc(cuda, c, nef, P, q=t(np.where(gone, 3.0 * c.q + 0.5, c.q)))
    assert _equal(g0, g1) and _equal(g0, g2) and float(g0[1].abs().max()) > 0
    g3 = _gnc(cuda, c, nef, P, x=t(c.x + np.where(gone[..., None], 0.0, 0.37)))
    assert not torch.equal(g0[1], g3[1])


# ---- 7. determinism
@pytest.mark.parametrize("precision", ["f32", "bf16"])
@pytest.mark.parametrize("variant", ["z_fold", "latent_split"])
def test_gn_cell_product_deterministic_mode_equal_bits(cuda, precision, variant):
    c = case("rel_pos_periodic", 8, 144, **BIG)
    nef, P = _model(cuda, c, precision, deterministic=True, variants=("auto", variant))
    runs = [_gnc(cuda, c, nef, P), _gnc(cuda, c, nef, P)]
    assert len(nef._ws_cache) == 1
    for byte in (0x00, 0xFF):
        for ws in nef._ws_cache.values():
            ws.fill_(byte)
        runs.append(_gnc(cuda, c, nef, P))
    for r in runs[1:]:
        assert _equal(r, runs[0])
    assert all(torch.isfinite(g).all() for g in runs[0]) and float(runs[0][1].abs().max()) > 0


# ---- 8. reuse of the point
@pytest.mark.parametrize("variant", ["z_fold", "latent_split"])
def test_gn_cell_product_reuse_point_after_a_cell_fit_step_gives_the_same_bits(cuda, variant):
    c = case("ponita", 4, 80)
    nef, P = _model(cuda, c, "f32", deterministic=True, variants=("auto", variant))
    t = _t(cuda)
    plain = _gnc(cuda, c, nef, P)
    tag0 = nef.gn_reserve(3, 80, 7, cuda)
    target = t(np.random.default_rng(3).standard_normal((3, c.M, c.O)))
    nef.mse_value_and_cell_grads(P, t(c.x), t(c.p), t(c.a), t(c.s), target, c.G, qweight=t(c.q), obs_weight=t(c.w), grad_scale=3.0)
    tag = nef.workspace_tag(cuda)                               # enf_fit_step_g ran on that buffer
    assert tag != tag0 and len(nef._ws_cache) == 1
    reused = _gnc(cuda, c, nef, P, reuse=tag)
    again = _gnc(cuda, c, nef, P, reuse=nef.workspace_tag(cuda))                                       # behind an earlier product
    stale = _gnc(cuda, c, nef, P, reuse=tag)                                                           # a stale tag recomputes
    for r in (reused, again, stale):
        assert _equal(r, plain)


# ---- 9. a broadcast grid
def test_gn_cell_product_broadcast_grid_equals_materialised(cuda):
    c = case("ponita", 4, 80)
    nef, P = _model(cuda, c, "f32", deterministic=True)
    x = _t(cuda)(c.x[0])
    g0 = _gnc(cuda, c, nef, P, x=x[None].expand(3, -1, -1))
    g1 = _gnc(cuda, c, nef, P, x=x[None].repeat(3, 1, 1))
    assert _equal(g0, g1) and float(g0[0].abs().max()) > 0


# ---- 10. end to end
def _sgd(nef, P, x, q, G, tgt, p, a, s, steps):
    B = p.shape[0]
    for _ in range(steps):
        _, gp, ga, _ = nef.mse_value_and_cell_grads(P, x, p, a, s, tgt, G, qweight=q, grad_scale=float(B))
        p, a = p - gp, a - 5.0 * ga
    return nef.eval_cell_loss(P, x, p, a, s, tgt, G, qweight=q)[0]


@pytest.mark.parametrize("precision", ["f32", "bf16"])
@pytest.mark.parametrize("inv", ["rel_pos_periodic", "ponita"])
def test_lm_fit_cell_averages_end_to_end(cuda, inv, precision):
    """Cells: groups of 4 over the 80 rows of tests/tangent_ref.case(inv, N=80), q = U(0.2, 2) normalised to sum 1 per group.
    default_rng(21): p* = p + 0.05 N(0,1), a* = a + 0.5 N(0,1), target = the fp64 group sums of the oracle's decode at (p*, a*, s); four
    LM steps of eight CG iterations from (p, a, s).  Both precisions: shapes, finite, the window untouched, no signal's loss ever
    increases.  f32: every signal ends below 48 steps of the inner loop's SGD rule (p -= g_p, a -= 5 g_a at gradient scale B) run on the
    GPU through mse_value_and_cell_grads.
    The fp64 reference alone (oracle_lm_cells against oracle_sgd_cells, seed 21 and the scales above as first chosen) leaves, per
    signal, the factors 10.0, 3.8, 4.8 (rel_pos_periodic) and 14.3, 9.6, 5.1 (ponita) between the two: at least 2, nothing was changed."""
    from enf_pde_amd.fitting import lm_fit_cell_averages
    f = fit_case(inv)
    nef = build_nef(f.cfg, precision)
    P = nef.load_params(f.prm, device=cuda)
    t = _t(cuda)
    (p1, a1, s1), loss_b, lam, acc = lm_fit_cell_averages(nef, P, t(f.x), t(f.q), f.G, t(f.target), t(f.p), t(f.a), t(f.s), steps=4, cg_iters=8)
    lb = loss_b.double().cpu().numpy()
    ref, ref_acc = oracle_lm_cells(f.cfg, f.prm, f.x, f.q, f.G, f.target, f.p, f.a, f.s, 4)
    for k in range(5):
        print(f"{inv} {precision} step {k}: GPU " + " ".join(f"{v:.3e}" for v in lb[k]) + "   fp64 " + " ".join(f"{v:.3e}" for v in ref[k]))
    print(f"accepted: GPU {acc.cpu().numpy().astype(int).tolist()}  fp64 {ref_acc.astype(int).tolist()}; damping {lam.cpu().numpy()}")
    assert lb.shape == (5, 3) and acc.shape == (4, 3) and p1.shape == f.p.shape and a1.shape == f.a.shape
    assert np.isfinite(lb).all() and bool(torch.isfinite(p1).all()) and bool(torch.isfinite(a1).all()) and torch.equal(s1, t(f.s))
    assert (lb[1:] <= lb[:-1]).all()
    if precision == "f32":
        sgd = _sgd(nef, P, t(f.x), t(f.q), f.G, t(f.target), t(f.p), t(f.a), t(f.s), 48).double().cpu().numpy()
        print("48 SGD steps: " + " ".join(f"{v:.3e}" for v in sgd))
        assert (lb[-1] < sgd).all()
