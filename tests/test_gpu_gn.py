"""The Gauss-Newton product, the batched CG step and the Levenberg-Marquardt fit on the GPU (include/enf_hip.h, "Gauss-Newton
product"): EquivariantCrossAttentionNeF.gn_product against the fp64 product of the oracle (tests/gn_ref.py, pinned by
tests/test_gn_host.py) and against the composed route through the shipped entry points; enf_cg_update against numpy; cg_solve against a
dense solve; lm_fit_latents against the inner loop's SGD rule.

Error measure: the relative Frobenius norm per component gp, ga, gsigma.  Bounds against the oracle: the sum of the project's two
contracts, for the derivative of ``out`` through the chain (5e-4 / 7e-2) and for latent gradients (2e-4 / 7e-2): 7e-4 in f32, 1.4e-1 in
bf16 -- the bound tests/test_gpu_tangent.py::test_tangent_is_dual_to_the_latent_backward uses.  Against the composed route (the same fp32
sums in another order): 1e-5."""
import ctypes

import numpy as np
import pytest
import torch

from enf_pde_amd import _lib
from tests.helpers import build_nef
from tests.gn_ref import INVARIANTS, case, fit_case, gn_case, oracle_gn, oracle_lm, rel, weights

pytestmark = pytest.mark.gpu

TOL = {"f32": 7e-4, "bf16": 1.4e-1}
NAMES = ("gp", "ga", "gsigma")
GS = 3.0


def _t(cuda):
    return lambda v: None if v is None else torch.tensor(np.asarray(v), dtype=torch.float32, device=cuda)


def _model(cuda, c, precision, deterministic=None, variants=None):
    nef = build_nef(c[0], precision)
    nef.deterministic = deterministic
    if variants is not None:
        nef.pair_variants = variants
    return nef, nef.load_params(c[1], device=cuda)


def _gn(cuda, c, nef, P, v=None, w=None, gs=GS, x=None, reuse=None):
    """nef.gn_product on a case of tests/tangent_ref.py (its own tangents unless `v`); w: None, (B, N) or (B, N, O)"""
    cfg, prm, (x0, p, a, s), tg = c[:4]
    t = _t(cuda)
    vp, va, vs = tg if v is None else v
    w = None if w is None else np.asarray(w)
    kw = {} if w is None else ({"weight": t(w)} if w.ndim == 2 else {"channel_weight": t(w)})
    return nef.gn_product(P, t(x0) if x is None else x, t(p), t(a), t(s) if cfg["use_gaussian_window"] else None, vp=t(vp), va=t(va),
                          vwindow=t(vs), grad_scale=gs, reuse=reuse, **kw)


def _errs(got, ref):
    """Per component.  A component whose exact value is zero (the window of a single latent: its logit shift cancels in a one-term
    softmax) has no norm of its own to be relative to: it is measured against the norm of the whole product."""
    whole = float(np.sqrt(sum(float((r ** 2).sum()) for r in ref)))
    return [rel(g.double().cpu().numpy().reshape(r.shape), r) if np.any(r) else float(np.linalg.norm(g.double().cpu().numpy())) / whole
            for g, r in zip(got, ref)]


def _check(got, ref, tol, what):
    es = _errs(got, ref)
    print(f"{what}: " + ", ".join(f"{n} {e:.3e}" for n, e in zip(NAMES, es)) + f" (bound {tol:.1e})")
    for g, e, n in zip(got, es, NAMES):
        assert torch.isfinite(g).all() and e <= tol, (what, n, e)
    return es


# ---- 1. oracle parity: seven invariants x two precisions, with per-point weights, per-channel weights and neither
@pytest.mark.parametrize("precision", ["f32", "bf16"])
@pytest.mark.parametrize("inv", INVARIANTS)
def test_gn_product_matches_oracle_for_every_invariant(cuda, inv, precision):
    nef = P = None
    for mode in ("point", "channel", "none"):
        c, w, ref, _ = gn_case(inv, mode)
        if nef is None:
            nef, P = _model(cuda, c, precision)
        _check(_gn(cuda, c, nef, P, w=w), ref, TOL[precision], f"{inv} {precision} weights={mode}")


# ---- 2. the composed route through public entry points, f32, in both variants of the backward pair kernel
@pytest.mark.parametrize("variant", ["z_fold", "latent_split"])
@pytest.mark.parametrize("inv", ["rel_pos_periodic", "ponita", "latitude_periodic"])
def test_gn_product_equals_tangent_then_latent_backward(cuda, inv, variant):
    c, w, _, _ = gn_case(inv, "point")
    cfg, prm, (x, p, a, s), (vp, va, vs) = c[:4]
    nef, P = _model(cuda, c, "f32", variants=("auto", variant))
    desc = nef._desc(3, 50, 7)
    assert _lib.load().enf_pair_variant(ctypes.byref(desc), 1) == _lib.VARIANT[variant]
    t = _t(cuda)
    got = _gn(cuda, c, nef, P, w=w)
    _, tan = nef.tangent(P, t(x), t(p), t(a), t(s), dp=t(vp), da=t(va), dwindow=t(vs))
    wt = t(w)[..., None]
    coef = GS * 2.0 / tan.numel()
    seed = torch.where(wt > 0, wt * tan, torch.zeros_like(tan)) * coef
    hp, ha, hs = (t(u).requires_grad_(True) for u in (p, a, s))
    nef.apply(P, t(x), hp, ha, hs).backward(seed)
    ref = [h.grad.double().cpu().numpy() for h in (hp, ha, hs)]
    _check(got, ref, 1e-5, f"{inv} {variant}: against tangent -> w tan coef -> latent backward")


# ---- 3. symmetry and the quadratic form
@pytest.mark.parametrize("precision", ["f32", "bf16"])
@pytest.mark.parametrize("inv", ["rel_pos_periodic", "ponita", "polar_periodic"])
def test_gn_product_is_symmetric_and_positive(cuda, inv, precision):
    c, w, _, _ = gn_case(inv, "point")
    cfg, prm, (x, p, a, s), v = c[:4]
    rng = np.random.default_rng(13)
    u = tuple(rng.standard_normal(q.shape) * sc for q, sc in zip(v, (0.3, 1.0, 0.1)))
    nef, P = _model(cuda, c, precision)
    t = _t(cuda)
    Gv = [g.double() for g in _gn(cuda, c, nef, P, w=w)]
    Gu = [g.double() for g in _gn(cuda, c, nef, P, v=u, w=w)]
    dot = lambda A, B_: float(sum((a_ * b_).sum() for a_, b_ in zip(A, B_)))
    nrm = lambda A: float(np.sqrt(sum(float((a_ * a_).sum()) for a_ in A)))
    vt, ut = [t(q).double() for q in v], [t(q).double() for q in u]
    asym = abs(dot(ut, Gv) - dot(Gu, vt))
    scale = nrm(ut) * nrm(Gv) + nrm(vt) * nrm(Gu)
    _, tan = nef.tangent(P, t(x), t(p), t(a), t(s), dp=t(v[0]), da=t(v[1]), dwindow=t(v[2]))
    quad = GS * 2.0 / tan.numel() * float((t(w).double()[..., None] * tan.double() ** 2).sum())
    vGv = dot(vt, Gv)
    print(f"{inv} {precision}: |<u,Gv> - <Gu,v>| / (|u||Gv| + |v||Gu|) = {asym / scale:.3e}, <v,Gv> = {vGv:.6e} against "
          f"coef sum w tan^2 = {quad:.6e}: {abs(vGv - quad) / quad:.3e} (bounds 7.0e-04, f32 only)")
    if precision == "f32":
        assert asym <= 7e-4 * scale and abs(vGv - quad) <= 7e-4 * quad and vGv >= 0


# ---- 4. the other instantiations and the edges
@pytest.mark.parametrize("name,inv,D,H,B,N,Z,precision", [
    ("128x2", "rel_pos_periodic", 128, 2, 2, 130, 9, "f32"),
    ("128x2", "rel_pos_periodic", 128, 2, 2, 130, 9, "bf16"),
    ("128x1", "rel_pos_periodic", 128, 1, 2, 40, 5, "f32"),
    ("64x4", "rel_pos_periodic", 64, 4, 2, 40, 5, "f32"),
    ("64x1", "rel_pos_periodic", 64, 1, 2, 20, 7, "f32"),          # with the rows above and the default 64x2: every (D, H) pair of the
    ("64x1", "rel_pos_periodic", 64, 1, 2, 20, 7, "bf16"),         # dispatch in both precisions
    ("128x1", "rel_pos_periodic", 128, 1, 2, 20, 7, "bf16"),
    ("64x4", "rel_pos_periodic", 64, 4, 2, 20, 7, "bf16"),
    ("16x2 padded", "polar_periodic", 16, 2, 2, 40, 5, "f32"),
    ("32x3 padded", "rel_pos", 32, 3, 2, 40, 5, "f32"),
    ("one latent", "rel_pos_periodic", 64, 2, 2, 20, 1, "f32"),
    ("one query", "rel_pos_periodic", 64, 2, 2, 1, 7, "f32")])
def test_gn_product_other_instantiations(cuda, name, inv, D, H, B, N, Z, precision):
    c, w, ref, _ = gn_case(inv, "point", D=D, H=H, B=B, N=N, Z=Z)
    nef, P = _model(cuda, c, precision)
    _check(_gn(cuda, c, nef, P, w=w), ref, TOL[precision], f"{name} {precision}")


# ---- 5. each direction alone, exact zeros, linearity, points of weight zero
@pytest.mark.parametrize("which", [0, 1, 2])
def test_gn_product_each_direction_alone(cuda, which):
    c = case("latitude_periodic")
    cfg, prm, xpas, tg = c[:4]
    alone = tuple(v if i == which else None for i, v in enumerate(tg))
    w = weights((3, 50))
    ref, _ = oracle_gn(cfg, prm, *xpas, alone, w, GS)
    nef, P = _model(cuda, c, "f32")
    _check(_gn(cuda, c, nef, P, v=alone, w=w), ref, TOL["f32"], ("vp", "va", "vwindow")[which] + " alone")


def test_gn_product_window_direction_without_a_window_is_exactly_zero(cuda):
    nw = case("rel_pos_periodic", use_window=False)
    for det in (False, True):
        nef, P = _model(cuda, nw, "f32", deterministic=det)
        got = _gn(cuda, nw, nef, P, v=(None, None, nw[3][2]))
        assert got[2] is None
        assert torch.equal(got[0], torch.zeros_like(got[0])) and torch.equal(got[1], torch.zeros_like(got[1]))


def test_gn_product_is_linear_in_the_direction(cuda):
    c = case("polar_periodic")
    v1 = c[3]
    rng = np.random.default_rng(11)
    v2 = tuple(rng.standard_normal(v.shape) * sc for v, sc in zip(v1, (0.3, 1.0, 0.1)))
    alpha = 0.7
    w = weights((3, 50))
    nef, P = _model(cuda, c, "f32", deterministic=True)
    g1 = _gn(cuda, c, nef, P, w=w)
    g2 = _gn(cuda, c, nef, P, v=v2, w=w)
    g12 = _gn(cuda, c, nef, P, v=tuple(alpha * a + b for a, b in zip(v1, v2)), w=w)
    for n, a_, b_, ab in zip(NAMES, g1, g2, g12):
        e = float((ab - (alpha * a_ + b_)).norm() / ab.norm())
        print(f"linearity {n}: {e:.3e} (bound 1.0e-05)")
        assert e < 1e-5


@pytest.mark.parametrize("mode", ["point", "channel"])
def test_gn_product_ignores_points_of_weight_zero(cuda, mode):
    """Moving x at the points whose weight is 0 changes no bit (deterministic mode).  Per-channel weights: a point counts as absent
    where all its channels are."""
    c, w, _, _ = gn_case("ponita", mode)
    nef, P = _model(cuda, c, "f32", deterministic=True)
    t = _t(cuda)
    wz = w == 0 if w.ndim == 2 else (w == 0).all(-1)
    if mode == "channel":                      # make some whole points absent
        w = w.copy()
        w[:, ::5, :] = 0.0
        wz = (w == 0).all(-1)
    assert wz.any() and not wz.all()
    x = c[2][0]
    moved = x + np.where(wz[..., None], 0.37, 0.0)
    g0 = _gn(cuda, c, nef, P, w=w)
    g1 = _gn(cuda, c, nef, P, w=w, x=t(moved))
    assert all(torch.equal(a_, b_) for a_, b_ in zip(g0, g1)) and float(g0[1].abs().max()) > 0
    g2 = _gn(cuda, c, nef, P, w=w, x=t(x + 0.37))             # (moving the other points does change it)
    assert not torch.equal(g0[1], g2[1])


# ---- 6. determinism
@pytest.mark.parametrize("precision", ["f32", "bf16"])
@pytest.mark.parametrize("variant", ["z_fold", "latent_split"])
def test_gn_product_deterministic_mode_equal_bits(cuda, precision, variant):
    c, w, _, _ = gn_case("rel_pos_periodic", "point", D=128, H=2, B=2, N=130, Z=9)
    nef, P = _model(cuda, c, precision, deterministic=True, variants=("auto", variant))
    runs = [_gn(cuda, c, nef, P, w=w), _gn(cuda, c, nef, P, w=w)]
    assert len(nef._ws_cache) == 1
    for byte in (0x00, 0xFF):
        for ws in nef._ws_cache.values():
            ws.fill_(byte)
        runs.append(_gn(cuda, c, nef, P, w=w))
    for r in runs[1:]:
        assert all(torch.equal(a_, b_) for a_, b_ in zip(r, runs[0]))
    assert all(torch.isfinite(g).all() for g in runs[0]) and float(runs[0][1].abs().max()) > 0


@pytest.mark.parametrize("variant", ["z_fold", "latent_split"])
def test_gn_product_reuse_point_after_a_fit_step_gives_the_same_bits(cuda, variant):
    c, w, _, _ = gn_case("ponita", "point")
    cfg, prm, (x, p, a, s), v = c[:4]
    nef, P = _model(cuda, c, "f32", deterministic=True, variants=("auto", variant))
    t = _t(cuda)
    plain = _gn(cuda, c, nef, P, w=w)
    tag0 = nef.gn_reserve(3, 50, 7, cuda)
    target = t(np.random.default_rng(3).standard_normal((3, 50, 2)))
    nef.mse_value_and_latent_grads(P, t(x), t(p), t(a), t(s), target, grad_scale=3.0, weight=t(w))      # enf_fit_step_w on that buffer
    tag = nef.workspace_tag(cuda)
    assert tag != tag0 and len(nef._ws_cache) == 1
    reused = _gn(cuda, c, nef, P, w=w, reuse=tag)
    again = _gn(cuda, c, nef, P, w=w, reuse=nef.workspace_tag(cuda))                                   # behind an earlier product
    stale = _gn(cuda, c, nef, P, w=w, reuse=tag)                                                       # a stale tag recomputes
    for r in (reused, again, stale):
        assert all(torch.equal(a_, b_) for a_, b_ in zip(r, plain))


def test_gn_product_broadcast_grid_equals_materialised(cuda):
    c, w, _, _ = gn_case("ponita", "point")
    nef, P = _model(cuda, c, "f32", deterministic=True)
    x = _t(cuda)(c[2][0][0])
    g0 = _gn(cuda, c, nef, P, w=w, x=x[None].expand(3, -1, -1))
    g1 = _gn(cuda, c, nef, P, w=w, x=x[None].repeat(3, 1, 1))
    assert all(torch.equal(a_, b_) for a_, b_ in zip(g0, g1)) and float(g0[0].abs().max()) > 0


# ---- 7. enf_cg_update
def _cg_call(cuda, segs, B, Z, lam, rho, q):
    arr = (_lib.EnfCgSegment * _lib.ENF_CG_MAX_SEGMENTS)()
    for k, (x, r, d) in enumerate(segs):
        arr[k].x, arr[k].r, arr[k].d, arr[k].width = x.data_ptr(), r.data_ptr(), d.data_ptr(), x.shape[2]
        arr[k].q = None if q is None else q[k].data_ptr()
    _lib.launch(cuda, _lib.load().enf_cg_update, len(segs), arr, B, Z, _lib.ptr(lam), _lib.ptr(rho), _lib.stream(cuda))
    torch.cuda.synchronize()


def test_cg_update_one_step_against_numpy_and_frozen_signals(cuda):
    """B = 3, Z = 7, widths (2, 8, 1), distinct damping.  Signal 0 takes a step; signal 1 has r = 0 (rho = 0) and signal 2 a negative
    curvature (q = -d, lam < 1): both stay untouched bit for bit.  1e-5: fp32 sums of 77 terms against float64."""
    B, Z, widths = 3, 7, (2, 8, 1)
    rng = np.random.default_rng(17)
    X, R, D, Q = ([rng.standard_normal((B, Z, w)) for w in widths] for _ in range(4))
    for k in range(3):
        Q[k][0] = 2.0 * D[k][0] + 0.1 * Q[k][0]               # kappa > 0
        R[k][1] = 0.0
        Q[k][2] = -D[k][2]
    lam = np.array([0.1, 0.5, 0.3])
    flat = lambda L: np.concatenate([v.reshape(B, -1) for v in L], axis=1)
    rho = (flat(R) ** 2).sum(1)
    t = _t(cuda)
    run = lambda: ([(t(x), t(r), t(d)) for x, r, d in zip(X, R, D)], [t(q) for q in Q], t(rho), t(lam))
    segs, q, rho_t, lam_t = run()
    before = [[v.clone() for v in s] for s in segs]
    _cg_call(cuda, segs, B, Z, lam_t, rho_t, q)
    # float64 reference of signal 0
    qd = flat(Q) + lam[:, None] * flat(D)
    kappa = (flat(D) * qd).sum(1)
    assert kappa[0] > 0 and rho[1] == 0 and kappa[2] < 0
    alpha = rho[0] / kappa[0]
    x_ref = flat(X)[0] + alpha * flat(D)[0]
    r_ref = flat(R)[0] - alpha * qd[0]
    rho2 = (r_ref ** 2).sum()
    d_ref = r_ref + rho2 / rho[0] * flat(D)[0]
    got = lambda i: np.concatenate([s[i][0].double().cpu().numpy().reshape(-1) for s in segs])
    for name, g, r in (("x", got(0), x_ref), ("r", got(1), r_ref), ("d", got(2), d_ref)):
        e = float(np.linalg.norm(g - r) / np.linalg.norm(r))
        print(f"cg step {name}: {e:.3e} (bound 1.0e-05)")
        assert e <= 1e-5
    assert abs(float(rho_t[0]) - rho2) <= 1e-5 * rho2
    for b in (1, 2):                                          # frozen: x, r, d, rho exactly as they were
        for s, s0 in zip(segs, before):
            assert all(torch.equal(v[b], v0[b]) for v, v0 in zip(s, s0))
        assert float(rho_t[b]) == float(t(rho)[b])
    # equal bits run to run
    segs2, q2, rho2_t, lam2_t = run()
    _cg_call(cuda, segs2, B, Z, lam2_t, rho2_t, q2)
    assert torch.equal(rho_t, rho2_t) and all(torch.equal(v, v2) for s, s2 in zip(segs, segs2) for v, v2 in zip(s, s2))
    # INIT: x = 0, d = r, rho = r . r; a NaN signal stays alone in the next step
    segs3, q3, rho3, lam3 = run()
    segs3[0][1][2] = float("nan")
    _cg_call(cuda, segs3, B, Z, None, rho3, None)
    assert all(torch.equal(s[0], torch.zeros_like(s[0])) for s in segs3)
    assert all(torch.equal(s[2][:2], s[1][:2]) for s in segs3)
    assert abs(float(rho3[0]) - rho[0]) <= 1e-5 * rho[0] and float(rho3[1]) == 0.0 and bool(torch.isnan(rho3[2]))
    _cg_call(cuda, segs3, B, Z, None, rho3, q3)
    assert all(torch.isfinite(s[i][:2]).all() for s in segs3 for i in range(3)) and bool(torch.isfinite(rho3[:2]).all())


# ---- 8. cg_solve on a dense operator
def test_cg_solve_against_a_dense_solve(cuda):
    """Batched SPD matrices with eigenvalues in [1, 10], lam = (0, 0.5, 2), 30 iterations: the CG bound 2 ((sqrt 10 - 1) / (sqrt 10 +
    1))^30 ~ 6e-9 leaves the error to fp32 rounding: 1e-4 against torch.linalg.solve in fp64."""
    from enf_pde_amd.fitting import cg_solve
    B, Z, widths = 3, 7, (2, 8, 1)
    n = Z * sum(widths)
    g = torch.Generator().manual_seed(19)
    Qm, _ = torch.linalg.qr(torch.randn((B, n, n), generator=g, dtype=torch.float64))
    ev = 1.0 + 9.0 * torch.rand((B, n), generator=g, dtype=torch.float64)
    ev[:, 0], ev[:, 1] = 1.0, 10.0
    G = (Qm * ev[:, None, :]) @ Qm.transpose(1, 2)
    rhs = torch.randn((B, n), generator=g, dtype=torch.float64)
    lam = torch.tensor([0.0, 0.5, 2.0], dtype=torch.float64)
    want = torch.linalg.solve(G + lam[:, None, None] * torch.eye(n, dtype=torch.float64), rhs)
    Gd = G.float().to(cuda)
    sizes = [Z * w for w in widths]

    def split(vec):
        return tuple(part.reshape(B, Z, w).contiguous() for part, w in zip(vec.split(sizes, dim=1), widths))

    def matvec(d):
        return split(torch.einsum("bij,bj->bi", Gd, torch.cat([t.reshape(B, -1) for t in d], dim=1)))
    xs = cg_solve(matvec, split(rhs.float().to(cuda)), lam.float().to(cuda), 30)
    got = torch.cat([t.reshape(B, -1) for t in xs], dim=1).double().cpu()
    for b in range(B):
        e = float((got[b] - want[b]).norm() / want[b].norm())
        print(f"cg_solve signal {b} (lam {float(lam[b])}): {e:.3e} (bound 1.0e-04)")
        assert e <= 1e-4


# ---- 9. end to end
def _sgd(nef, P, x, tgt, p, a, s, steps):
    B = p.shape[0]
    for _ in range(steps):
        _, gp, ga, _ = nef.mse_value_and_latent_grads(P, x, p, a, s, tgt, grad_scale=float(B))
        p, a = p - gp, a - 5.0 * ga
    return nef.eval_loss(P, x, p, a, s, tgt)[0]


@pytest.mark.parametrize("precision", ["f32", "bf16"])
@pytest.mark.parametrize("inv", ["rel_pos_periodic", "ponita"])
def test_lm_fit_latents_end_to_end(cuda, inv, precision):
    """default_rng(21): p* = p + 0.05 N(0,1), a* = a + 0.5 N(0,1), target = the oracle's fp64 decode of (p*, a*, s); four LM steps of
    eight CG iterations from (p, a, s).  f32: no signal's loss ever increases and every signal ends below 48 steps of the inner loop's
    SGD rule (p -= g_p, a -= 5 g_a at gradient scale B) run on the GPU in the same precision -- the fp64 reference leaves a factor 2.6
    (rel_pos_periodic) and 13 (ponita) between the two.  bf16: finite and non-increasing."""
    from enf_pde_amd.fitting import lm_fit_latents
    cfg, prm, x, (p, a, s), target = fit_case(inv)
    nef = build_nef(cfg, precision)
    P = nef.load_params(prm, device=cuda)
    t = _t(cuda)
    (p1, a1, s1), loss_b, lam, acc = lm_fit_latents(nef, P, t(x), t(target), t(p), t(a), t(s), steps=4, cg_iters=8)
    lb = loss_b.double().cpu().numpy()
    ref, ref_acc = oracle_lm(cfg, prm, x, target, p, a, s, 4)
    for k in range(5):
        print(f"{inv} {precision} step {k}: GPU " + " ".join(f"{v:.3e}" for v in lb[k]) + "   fp64 " + " ".join(f"{v:.3e}" for v in ref[k]))
    print(f"accepted: GPU {acc.cpu().numpy().astype(int).tolist()}  fp64 {ref_acc.astype(int).tolist()}; damping {lam.cpu().numpy()}")
    assert lb.shape == (5, 3) and np.isfinite(lb).all() and torch.equal(s1, t(s))
    assert (lb[1:] <= lb[:-1]).all()
    if precision == "f32":
        sgd = _sgd(nef, P, t(x), t(target), t(p), t(a), t(s), 48).double().cpu().numpy()
        print(f"48 SGD steps: " + " ".join(f"{v:.3e}" for v in sgd))
        assert (lb[-1] < sgd).all()
