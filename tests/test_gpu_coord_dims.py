"""Coordinate dimension dx = 1 and 3 for rel_pos, abs_pos and norm_rel_pos, and latent_dim 1 .. 130, on the GPU against the fp64 oracle.

enf_check_desc takes dx 1 .. 3 for the three translation invariants and any latent_dim > 0; the rest of the suite runs dx = 2 (dx = 3 only
through the f32 forward-mode calls) and latent_dim 2 .. 32.  Cases, shapes and references: tests/coord_dims_ref.py (windows kept at
sigma = 2/3, where the 2-D suite has them); what needs no GPU: tests/test_coord_dims_host.py.

Which test reaches what (A: dx in {1, 3}, three invariants, f32 and bf16; 64x2 at (3, 50, 7) and (2, 130, 9) unless said otherwise):
    test_forward                  load_query and pair_invariant's default: branch under the three forward variants; x_bstride = 0 and
                                  N dx with rows 1 and 3 floats wide; the zero-padded invariant rows of the packed first layer
    test_latent_backward          pair_invariant_bwd and its dpose[1], dpose[2] updates under both backward variants; the dp_dim loop of
                                  the prologue backward (d p is (B, Z, dx)); 128x2: in bf16 the generic INV = -1 instantiation
    test_query_gradient           the dxq[0..2] stores, the atomic and the deterministic stores of d x at o[1], o[2],
                                  enf_dxq_reduce_kernel's (B, Z, N, dx) and (B, N, dx) indexing, enf_field_grad's (O, B, N, dx) buffer;
                                  apply() with x.requires_grad, nef.query_vjp and nef.jacobian agree with one another
    test_weight_gradients         enf_backward_all with enf_inv_dim = 1 and 3 rows in the embeddings' first layer (rff: frozen
                                  coefficients; ffn: Dense_0 has enf_inv_dim rows and gets a gradient)
    test_fit_step                 the fused step with per-point weights at 64x2, 128x2 and 64x4
    test_fit_step_on_cells        enf_fit_step_g, G = 4, (3, 52, 7)
    test_inner_loop               enf_fit_inputs (coords (N, dx), shared masks, the shared first step), enf_fit_inputs_b (per-signal
                                  masks) and enf_fit_inputs_g (inner_loop_cells): the three gather kernels with rows dx floats wide
    test_forward_mode             nef.tangent along the latents and with xdot, nef.second_derivative: dx = 1 for the first time, dx = 3
                                  in bf16 for the first time
    test_gauss_newton             nef.gn_product and nef.gn_cell_product
    test_lifting                  no oracle: the dx-dimensional problem against the (dx + 1)-dimensional one with a zero coordinate,
                                  1 -> 2 and 2 -> 3, which holds the 1-D and 3-D paths to the 2-D one
    test_translation_and_rotation no oracle: joint translations (rel_pos, norm_rel_pos) and a joint 3-D rotation (norm_rel_pos)
B: latent_dim in {1, 3, 17, 33, 64, 100, 130}, dx = 2, rel_pos_periodic (one ponita case at 130), (2, 40, 9); 1, 33, 130 also at Z = 37:
    test_latent_width             the prologues' LDS sized by C; the prologue backward's loop over 16-row tiles of C, one per wave:
                                  17 and 33 end in a tile of one row, 100 is 7 tiles, 130 is 9 tiles on 8 waves -- the loop's second
                                  trip; Z = 37: three workgroups of 16 latents, the last with 10 real rows
    test_latent_width_weight_gradients   the stem's X^T Y with C rows, and every other tensor
    test_latent_width_forward_mode       nef.tangent along da, nef.gn_product's ga, enf_cg_update through fitting.cg_solve
    test_latent_width_inner_loop         enf_meta_sgd_update with C per-channel rates
    test_latent_width_fit_latents_step   enf_table_adam_update on rows C wide, through the auto-decoder trainer's fit_latents_step

Bounds, all borrowed from the 2-D test of the same quantity against the same oracle, none taken from these kernels:
    out                  max |err| / max |ref|: 2e-5 / 3e-2        tests/test_gpu_backward.py:102 (= tests/test_gpu_forward.TOL)
    d p, d a, d sigma    relative L2: 2e-4 / 7e-2                  tests/test_gpu_backward.TOL; a reference that vanishes (abs_pos: d p comes
                                                                   from the window alone and may) on the scale of d a, as its check()
    d x                  relative L2: 5e-4 / 7e-2                  tests/test_gpu_layers.py:96
    weight gradients     5e-4 per tensor                           tests/test_gpu_weight_grads.TOL; layers_0/linear (the tensors that feed a
                         1e-2 for the relu-fed tensors             relu): tests/test_gpu_layers.py:70
    fit step             loss 1e-5 / 3e-2, gradients 2e-4 / 7e-2   tests/test_gpu_cells.TOL (tests/test_gpu_wide_out.py uses it the same way)
    inner loop           loss 5e-4 / 5e-2, updates 20 times that   tests/test_gpu_signal_masks.LOSS_TOL
    tangent, out         5e-4 / 7e-2, 2e-5 / 3e-2                  tests/test_gpu_tangent.TOL, TOL_OUT (= tests/test_gpu_tangent_x's)
    second derivative    5e-4; bf16: 2 BF16_ER of the invariant    tests/test_gpu_second.TOL2_F32, BF16_ER
    GN products          7e-4 / 1.4e-1                             tests/test_gpu_gn.TOL
    three routes to d x  1e-3                                      tests/test_gpu_tangent_x.py section 3: two f32 contracts
    lifting              each quantity's own f32 bound above       two f32 runs of the same arithmetic
    translation, rotation  5e-4                                    tests/test_gpu_forward.test_full_size_invariances: coordinates moved
                                                                   in fp32
Every figure is printed before it is asserted.

Measured (MI355X; the table is in DESIGN.md 2).  f32: out 6e-7 .. 2.7e-6; d p, d a, d sigma 1e-6 .. 1.6e-5 (abs_pos at 128x2 the largest);
d x 1.3e-6 .. 1.7e-6 and the routes within 7.5e-7 of one another; weight gradients at most 6.5e-5 over dx and 3.1e-4 over latent_dim (a
bias of the query embedding at latent_dim 1), the stem kernel 1.3e-6 .. 2.9e-6 in every row; tangents, second derivatives, GN products and
the CG step 1.2e-6 .. 9.2e-6; lifting: equal bits in all six quantities.  bf16: out at most 1.7e-2, derivatives 1e-2 .. 6.5e-2 except the
two cases of BF16_OPERAND_ROUNDING below; GN products at most 8.0e-2 of 1.4e-1."""
import numpy as np
import pytest
import torch

from enf_pde_amd.fitting import cg_solve, default_meta_sgd_lrs
from enf_pde_amd.fitting.cells import inner_loop_cells
from enf_pde_amd.fitting.inner_loop import inner_loop
from tests import coord_dims_ref as CD
from tests import test_gpu_gn as GN
from tests import test_gpu_second as SEC
from tests import test_gpu_tangent as TT
from tests import test_gpu_weight_grads as WG
from tests.ffn_ref import build_nef_ffn, ffn_oracle, init_params_ffn  # noqa: F401  (fixture)
from tests.helpers import build_nef
from tests.test_gpu_backward import TOL as TOL_GRAD, hip_grads, rel
from tests.test_gpu_cells import TOL as TOL_FIT
from tests.test_gpu_forward import TOL as TAU
from tests.test_gpu_signal_masks import LOSS_TOL

pytestmark = pytest.mark.gpu

PRECISIONS = ("f32", "bf16")
TOL_DX = {"f32": 5e-4, "bf16": 7e-2}                 # tests/test_gpu_layers.py:96
TOL_RELU_FED = 1e-2                                  # tests/test_gpu_layers.py:70
TOL_ROUTES = 1e-3                                    # tests/test_gpu_tangent_x.py, section 3
TOL_MOVED = 5e-4                                     # tests/test_gpu_forward.py:135
A_CASES = [(inv, dx) for inv in CD.INVS for dx in CD.DXS]
# bf16 cases over the borrowed 7e-2 whose f32 twins sit at 1e-5: decided with the rounding build libenf_hip_f32r.so (precision f32 with
# every operand rounded where bf16 rounds it, tests/test_gpu_bf16_faithful.py).  Its error against the oracle is the same -- d p 9.384e-2,
# d sigma 7.354e-2 for the backward case, d p 9.522e-2 for the fit step -- and bf16 - f32r is 1.1e-3 .. 1.8e-3 of the reference's norm,
# as in every case that keeps 7e-2 (the 2-D twins: 6.835e-2 / 5.948e-2 and 5.387e-2 on f32r), so the excess is operand rounding and the
# bound is twice the f32r error.  abs_pos takes d p and d sigma from the window's logit alone, where the terms cancel over z.
BF16_OPERAND_ROUNDING = {
    "backward z_fold abs_pos dx=3 (3, 50, 7) 128x2 bf16": {"d p": 2 * 9.384e-2, "d sigma": 2 * 7.354e-2},
    "fit step norm_rel_pos dx=3 64x4 bf16": {"d p": 2 * 9.522e-2},
}


def _t(cuda):
    return lambda v, g=False: None if v is None else torch.tensor(np.asarray(v), dtype=torch.float32, device=cuda, requires_grad=g)


def _np(v):
    return v.detach().double().cpu().numpy()


def _model(cuda, c, precision, deterministic=None):
    nef = build_nef(c.cfg, precision)
    nef.deterministic = deterministic
    return nef, nef.load_params(c.prm, device=cuda)


def _max_rel(got, ref):
    return float(np.abs(np.asarray(got, dtype=np.float64) - ref).max() / np.abs(ref).max())


def _check_out(got, ref, tol, what):
    got = np.asarray(got, dtype=np.float64)
    e = _max_rel(got, ref)
    print(f"{what}: out {e:.3e} of max|ref| (bound {tol:.1e})")
    assert got.shape == ref.shape and np.isfinite(got).all() and e < tol, (what, e)
    return e


def _check_rel(pairs, tol, what, scale=None):
    """relative L2 error of every (name, got, ref); a reference below 1e-9 of `scale` is compared on that scale
    (tests/test_gpu_backward.check)"""
    es = {}
    for name, g, r in pairs:
        g = np.asarray(g, dtype=np.float64).reshape(r.shape)
        assert np.isfinite(g).all(), (what, name)
        if scale is not None and np.linalg.norm(r) <= 1e-9 * scale:
            es[name + " (vanishing reference, of |d a|)"] = float(np.linalg.norm(g) / scale)
        else:
            es[name] = float(rel(g, r))
    own = BF16_OPERAND_ROUNDING.get(what, {})
    print(f"{what}: " + ", ".join(f"{k} {v:.3e}" for k, v in es.items()) + f" (bound {tol:.1e}"
          + "".join(f", {k} {v:.3e}: twice the rounding build's error" for k, v in own.items()) + ")")
    bad = {k: v for k, v in es.items() if not v < own.get(k, tol)}
    assert not bad, (what, bad)
    return es


def _latent_pairs(got, g):
    return (("d p", got[0], g.gp), ("d a", got[1], g.ga), ("d sigma", got[2], g.gs))


# ======================================================================= A. dx = 1 and 3
# ---- 1. forward
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("inv,dx", A_CASES)
def test_forward(cuda, pair_variant, inv, dx, precision):
    t = _t(cuda)
    for shape in (CD.BASE, CD.TILES):
        c = CD.problem(inv, dx, shape)
        nef, P = _model(cuda, c, precision)
        with torch.no_grad():
            out = nef.apply(P, t(c.x), t(c.p), t(c.a), t(c.s))
            grid = nef.apply(P, t(c.x[0])[None].expand(c.B, -1, -1), t(c.p), t(c.a), t(c.s))
        torch.cuda.synchronize()
        what = f"forward {pair_variant} {inv} dx={dx} {shape} {precision}"
        _check_out(_np(out), c.out, TAU[precision], what)
        _check_out(_np(grid), CD.shared_grid(c).out, TAU[precision], what + ", stride-0 grid")


# ---- 2. backward to the latents
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("inv,dx", A_CASES)
def test_latent_backward(cuda, bwd_variant, inv, dx, precision):
    for shape, D in ((CD.BASE, 64), (CD.TILES, 64), (CD.BASE, 128)):
        c = CD.problem(inv, dx, shape, D=D)
        g = CD.backward(c)
        out, gp, ga, gs = hip_grads(cuda, build_nef(c.cfg, precision), c.prm, c.x, c.p, c.a, c.s, c.w)
        what = f"backward {bwd_variant} {inv} dx={dx} {shape} {D}x2 {precision}"
        assert gp.shape == (c.B, c.Z, dx)
        _check_out(out, c.out, TAU[precision], what)
        _check_rel(_latent_pairs((gp, ga, gs), g), TOL_GRAD[precision], what, scale=float(np.linalg.norm(g.ga)))


# ---- 3. the gradient with respect to the query coordinates, three routes
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("inv,dx", A_CASES)
def test_query_gradient(cuda, inv, dx, precision):
    t = _t(cuda)
    tol = TOL_DX[precision]
    for shape in (CD.BASE, CD.TILES):
        c = CD.problem(inv, dx, shape)
        g = CD.backward(c)
        what = f"query gradient {inv} dx={dx} {shape} {precision}"
        routes = {}
        for det in (None, True):
            nef, P = _model(cuda, c, precision, deterministic=det)
            x = t(c.x, True)
            (nef.apply(P, x, t(c.p), t(c.a), t(c.s)) * t(c.w)).sum().backward()
            routes["apply, deterministic" if det else "apply"] = x.grad
            routes["query_vjp, deterministic" if det else "query_vjp"] = nef.query_vjp(P, t(c.x), t(c.p), t(c.a), t(c.s), t(c.w))
        out, jac = nef.jacobian(P, t(c.x), t(c.p), t(c.a), t(c.s))
        torch.cuda.synchronize()
        assert jac.shape == (c.B, c.N, c.O, dx)
        routes["jacobian . w"] = (jac * t(c.w)[..., None]).sum(2)
        _check_out(_np(out), c.out, TAU[precision], what + ", jacobian's")
        _check_rel([(k, _np(v), g.gx) for k, v in routes.items()], tol, what)
        _check_rel([("jacobian", _np(jac), CD.jacobian(c))], tol, what)
        if precision == "f32":
            ref = routes["query_vjp, deterministic"]
            ds = {k: float((v - ref).norm() / ref.norm()) for k, v in routes.items()}
            print(f"{what}: the routes against query_vjp (deterministic): " + ", ".join(f"{k} {v:.3e}" for k, v in ds.items()) + f" (bound {TOL_ROUTES:.1e})")
            assert all(v < TOL_ROUTES for v in ds.values()), ds
    # one grid shared by the signals: the gradient with respect to it sums over them
    c = CD.problem(inv, dx)
    sg = CD.shared_grid(c)
    for det in (None, True):
        nef, P = _model(cuda, c, precision, deterministic=det)
        x0 = t(c.x[0], True)
        (nef.apply(P, x0[None].expand(c.B, -1, -1), t(c.p), t(c.a), t(c.s)) * t(c.w)).sum().backward()
        per_signal = nef.query_vjp(P, t(c.x[0])[None].expand(c.B, -1, -1), t(c.p), t(c.a), t(c.s), t(c.w))
        torch.cuda.synchronize()
        _check_rel([("apply", _np(x0.grad), sg.gx), ("query_vjp summed", _np(per_signal.sum(0)), sg.gx)], tol,
                   f"query gradient {inv} dx={dx} {precision}, shared grid{', deterministic' if det else ''}")


# ---- 4. weight gradients
def _check_weight_grads(paths, got, ref, what, frozen="coefficients"):
    gmax = max(np.linalg.norm(r) for r in ref if r is not None)
    es, bad = {}, []
    for path, g, r in zip(paths, got, ref):
        if path is None:
            continue
        name = "/".join(path)
        if path[-1] == frozen:                                # stop_gradient (tests/test_gpu_weight_grads.check)
            assert np.all(g == 0) and not np.any(r), name
            continue
        nr = np.linalg.norm(r)
        e = float(np.linalg.norm(g - r) / (nr if nr > 1e-6 * gmax else gmax))
        tol = TOL_RELU_FED if "layers_0/linear" in name else WG.TOL["f32"]
        es[name] = e
        if not (np.isfinite(e) and e < tol):
            bad.append((name, e, tol))
    relu = {k: v for k, v in es.items() if "layers_0/linear" in k}
    rest = {k: v for k, v in es.items() if k not in relu}
    worst = max(rest, key=rest.get)
    print(f"{what}: {len(es)} tensors, worst {worst} {rest[worst]:.3e} (bound {WG.TOL['f32']:.1e})"
          + (f"; relu-fed worst {max(relu.values()):.3e} (bound {TOL_RELU_FED:.1e})" if relu else ""))
    assert not bad, (what, bad)
    return es


@pytest.mark.parametrize("inv,dx", A_CASES)
def test_weight_gradients(cuda, inv, dx):
    c = CD.problem(inv, dx)
    g = CD.backward(c)
    out, hg, hp, ha, hs = WG.hip(cuda, build_nef(c.cfg, "f32"), c.prm, c.x, c.p, c.a, c.s, c.w)
    what = f"weight gradients {inv} dx={dx}"
    _check_out(out, c.out, TAU["f32"], what)
    es = _check_weight_grads(WG.TENSOR_PATHS, hg, g.gw, what)
    assert len(es) == 44
    _check_rel(_latent_pairs((hp, ha, hs), g), WG.TOL["f32"], what, scale=float(np.linalg.norm(g.ga)))


@pytest.mark.parametrize("dx", CD.DXS)
def test_weight_gradients_ffn(cuda, ffn_oracle, dx):
    """the ffn embedding, rel_pos: Dense_0 of both embeddings is (dx, D) and trained"""
    from enf_pde_amd.enf.models import FFN_TENSOR_PATHS
    from oracle import enf_ref_torch as T
    c = CD.problem("rel_pos", dx)
    prm = init_params_ffn(13, c.cfg, jitter=0.1)
    tp = T.to_torch(prm, torch.float64, requires_grad=True)
    ref_out = T.nef_apply(tp, c.cfg, *(torch.tensor(v) for v in (c.x, c.p, c.a, c.s)))
    (ref_out * torch.tensor(c.w)).sum().backward()

    def get(path):
        tree = tp["params"]
        for k in path:
            tree = tree[k]
        return tree
    ref = [None if path is None else get(path).grad.numpy() for path in FFN_TENSOR_PATHS]
    nef = build_nef_ffn(c.cfg, "f32")
    P = nef.load_params(prm, device=cuda)
    ts = nef.param_tensors(P)
    for v in ts:
        v.requires_grad_(True)
    t = _t(cuda)
    out = nef.apply(P, t(c.x), t(c.p), t(c.a), t(c.s))
    (out * t(c.w)).sum().backward()
    torch.cuda.synchronize()
    what = f"weight gradients ffn rel_pos dx={dx}"
    _check_out(_np(out), ref_out.detach().numpy(), TAU["f32"], what)
    first = [i for i, path in enumerate(FFN_TENSOR_PATHS) if path is not None and path[-2:] == ("Dense_0", "kernel") and "invariant_embedding" in path[-3]]
    assert len(first) == 2 and all(tuple(ts[i].shape) == (dx, c.D) and float(np.linalg.norm(ref[i])) > 0 for i in first)
    got = [None if path is None else _np(v.grad) for path, v in zip(FFN_TENSOR_PATHS, ts)]
    _check_weight_grads(FFN_TENSOR_PATHS, got, ref, what, frozen=None)
    for i in first:
        print(f"{what}: {'/'.join(FFN_TENSOR_PATHS[i][-3:])} {rel(got[i], ref[i]):.3e}")


# ---- 5. the fused fit step
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("D,H", [(64, 2), (128, 2), (64, 4)])
@pytest.mark.parametrize("inv,dx", A_CASES)
def test_fit_step(cuda, inv, dx, D, H, precision):
    """mse_value_and_latent_grads with per-point weights (about a third exact zeros, NaN targets under them) against autograd of the
    oracle's weighted mean squared error"""
    c = CD.problem(inv, dx, D=D, H=H)
    r = CD.fit(c)
    nef, P = _model(cuda, c, precision)
    t = _t(cuda)
    y = r.y.copy()
    y[r.wt == 0] = np.nan
    loss, dp, da, ds = nef.mse_value_and_latent_grads(P, t(c.x), t(c.p), t(c.a), t(c.s), t(y), grad_scale=float(c.B), weight=t(r.wt))
    torch.cuda.synchronize()
    tol_l, tol_g = TOL_FIT[precision]
    what = f"fit step {inv} dx={dx} {D}x{H} {precision}"
    e = abs(float(loss) - r.loss) / r.loss
    print(f"{what}: loss {e:.3e} (bound {tol_l:.1e})")
    assert e <= tol_l
    _check_rel((("d p", _np(dp), r.g[0]), ("d a", _np(da), r.g[1]), ("d sigma", _np(ds), r.g[2])), tol_g, what, scale=float(np.linalg.norm(r.g[1])))


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("inv,dx", A_CASES)
def test_fit_step_on_cells(cuda, inv, dx, precision):
    """mse_value_and_cell_grads, G = 4, random factors, observation weights with exact zeros (NaN targets under them)"""
    c = CD.problem(inv, dx, CD.CELLS)
    k = CD.cells(c)
    nef, P = _model(cuda, c, precision)
    t = _t(cuda)
    y = k.y.copy()
    y[k.wt == 0] = np.nan
    loss, dp, da, ds, err, loss_b = nef.mse_value_and_cell_grads(P, t(c.x), t(c.p), t(c.a), t(c.s), t(y), CD.G, qweight=t(k.q), obs_weight=t(k.wt),
                                                                 grad_scale=float(c.B), return_errors=True)
    torch.cuda.synchronize()
    tol_l, tol_g = TOL_FIT[precision]
    what = f"fit step on cells {inv} dx={dx} {precision}"
    e, eb = abs(float(loss) - k.ref.loss) / k.ref.loss, float(np.abs(_np(loss_b) - k.ref.loss_b).max() / k.ref.loss_b.max())
    print(f"{what}: loss {e:.3e}, loss_b {eb:.3e} (bound {tol_l:.1e})")
    assert e <= tol_l and eb <= tol_l and bool((err[t(k.wt) == 0] == 0).all())
    _check_rel((("d p", _np(dp), k.ref.g[0]), ("d a", _np(da), k.ref.g[1]), ("d sigma", _np(ds), k.ref.g[2])), tol_g, what,
               scale=float(np.linalg.norm(k.ref.g[1])))


# ---- 6. the inner loop, three ways
def _check_inner(loss, fit, ref, lat0, B, precision, what):
    tol = LOSS_TOL[precision]
    ref_loss, ref_fit = ref
    e = abs(float(loss) - ref_loss) / ref_loss
    es = {}
    for k in ("p_pos", "a"):
        init = np.repeat(lat0[k], B, 0)
        assert np.abs(ref_fit[k] - init).max() > 0
        es[k] = float(rel(_np(fit[k]) - init, ref_fit[k] - init))
    print(f"{what}: loss {float(loss):.6e} against {ref_loss:.6e}: {e:.3e} (bound {tol:.1e}); updates "
          + ", ".join(f"{k} {v:.3e}" for k, v in es.items()) + f" (bound {20 * tol:.1e})")
    assert e < tol and all(v < 20 * tol for v in es.values()), (what, e, es)
    assert np.array_equal(_np(fit["gaussian_window"]), np.repeat(lat0["gaussian_window"], B, 0).astype(np.float32).astype(np.float64))


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("inv,dx", A_CASES)
def test_inner_loop(cuda, inv, dx, precision):
    t = _t(cuda)
    c = CD.problem(inv, dx)
    q = CD.inner(c)
    nef, P = _model(cuda, c, precision)
    lat0 = {k: t(v) for k, v in q.lat0.items()}
    lrs = {k: t(v) for k, v in q.lrs.items()}
    what = f"inner loop {inv} dx={dx} {precision}"
    loss, fit = inner_loop(nef, P, lat0, lrs, t(q.coords), t(q.img), torch.tensor(q.masks, device=cuda))
    torch.cuda.synchronize()
    assert fit["p_pos"].shape == (c.B, c.Z, dx)
    _check_inner(loss, fit, q.shared, q.lat0, c.B, precision, what + ", shared masks")
    loss, fit = inner_loop(nef, P, lat0, lrs, t(q.coords), t(q.img), torch.tensor(q.masks_b, device=cuda))
    torch.cuda.synchronize()
    _check_inner(loss, fit, q.per_signal, q.lat0, c.B, precision, what + ", per-signal masks")
    c = CD.problem(inv, dx, CD.CELLS)
    k = CD.inner_cells(c)
    nef, P = _model(cuda, c, precision)
    y = k.y.copy()
    y[k.wt == 0] = np.nan
    loss, fit = inner_loop_cells(nef, P, {n: t(v) for n, v in k.lat0.items()}, {n: t(v) for n, v in k.lrs.items()}, t(k.x), t(k.q), CD.G, t(y),
                                 torch.tensor(k.masks, device=cuda), obs_weights=t(k.wt))
    torch.cuda.synchronize()
    _check_inner(loss, fit, k.ref, k.lat0, c.B, precision, what + ", cells")


# ---- 7. forward mode and Gauss-Newton
def _check_tangent(out, tan, c, which, precision, what):
    _check_out(_np(out), c.out, TT.TOL_OUT[precision], what)
    ref = CD.tangent(c, which)
    assert tan.shape == ref.shape and float(np.linalg.norm(ref)) > 0
    _check_rel([("tangent", _np(tan), ref)], TT.TOL[precision], what)


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("inv,dx", A_CASES)
def test_forward_mode(cuda, inv, dx, precision):
    t = _t(cuda)
    for shape in (CD.BASE, CD.TILES):
        c = CD.problem(inv, dx, shape)
        tg = CD.tangents(c)
        nef, P = _model(cuda, c, precision)
        args = (P, t(c.x), t(c.p), t(c.a), t(c.s))
        kw = dict(dp=t(tg.v[0]), da=t(tg.v[1]), dwindow=t(tg.v[2]))
        what = f"{inv} dx={dx} {shape} {precision}"
        _check_tangent(*nef.tangent(*args, **kw), c, "latent", precision, f"tangent, latent directions, {what}")
        _check_tangent(*nef.tangent(*args, xdot=t(tg.xdot)), c, "xdot", precision, f"tangent, xdot alone, {what}")
        _check_tangent(*nef.tangent(*args, xdot=t(tg.xdot), **kw), c, "all", precision, f"tangent, all four, {what}")
    c = CD.problem(inv, dx)
    tg = CD.tangents(c)
    nef, P = _model(cuda, c, precision)
    out, tan, tan2 = nef.second_derivative(P, t(c.x), t(c.p), t(c.a), t(c.s), t(tg.xdot))
    torch.cuda.synchronize()
    tan_ref, tan2_ref = CD.second(c)
    what = f"second derivative {inv} dx={dx} {precision}"
    _check_out(_np(out), c.out, TT.TOL_OUT[precision], what)
    _check_rel([("tan", _np(tan), tan_ref)], TT.TOL[precision], what)
    _check_rel([("tan2", _np(tan2), tan2_ref)], SEC.TOL2_F32 if precision == "f32" else 2 * SEC.BF16_ER[inv], what)


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("inv,dx", A_CASES)
def test_gauss_newton(cuda, inv, dx, precision):
    t = _t(cuda)
    c = CD.problem(inv, dx)
    tg, r = CD.tangents(c), CD.gn(c)
    nef, P = _model(cuda, c, precision)
    got = nef.gn_product(P, t(c.x), t(c.p), t(c.a), t(c.s), vp=t(tg.v[0]), va=t(tg.v[1]), vwindow=t(tg.v[2]), grad_scale=r.gs, weight=t(r.wt))
    torch.cuda.synchronize()
    GN._check(got, r.ref, GN.TOL[precision], f"gn_product {inv} dx={dx} {precision}")
    c = CD.problem(inv, dx, CD.CELLS)
    tg, k, r = CD.tangents(c), CD.cells(c), CD.gn_cells(c)
    nef, P = _model(cuda, c, precision)
    got = nef.gn_cell_product(P, t(c.x), t(c.p), t(c.a), t(c.s), CD.G, qweight=t(k.q), obs_weight=t(k.wt), vp=t(tg.v[0]), va=t(tg.v[1]),
                              vwindow=t(tg.v[2]), grad_scale=r.gs)
    torch.cuda.synchronize()
    GN._check(got, r.ref, GN.TOL[precision], f"gn_cell_product {inv} dx={dx} {precision}")


# ---- 8. lifting
def _f32_run(cuda, c, y):
    """out, d x, d p, d a, d sigma of sum(out * w) through apply() and the fused step's loss, f32, deterministic"""
    t = _t(cuda)
    nef, P = _model(cuda, c, "f32", deterministic=True)
    x, p, a, s = t(c.x, True), t(c.p, True), t(c.a, True), t(c.s, True)
    out = nef.apply(P, x, p, a, s)
    (out * t(c.w)).sum().backward()
    loss = nef.mse_value_and_latent_grads(P, t(c.x), t(c.p), t(c.a), t(c.s), t(y))[0]
    torch.cuda.synchronize()
    return _np(out), _np(x.grad), _np(p.grad), _np(a.grad), _np(s.grad), float(loss)


@pytest.mark.parametrize("dx", [1, 2])
@pytest.mark.parametrize("inv", CD.INVS)
def test_lifting(cuda, inv, dx):
    c = CD.problem(inv, dx)
    up = CD.lift(c)
    y = CD.fit(c).y
    lo, hi = _f32_run(cuda, c, y), _f32_run(cuda, up, y)
    what = f"lifting {inv} {dx} -> {dx + 1}"
    assert hi[1].shape == (c.B, c.N, dx + 1) and hi[2].shape == (c.B, c.Z, dx + 1)
    _check_out(hi[0], lo[0], TAU["f32"], what)
    _check_rel([("d x", hi[1][..., :dx], lo[1])], TOL_DX["f32"], what)
    _check_rel([("d p", hi[2][..., :dx], lo[2]), ("d a", hi[3], lo[3]), ("d sigma", hi[4], lo[4])], TOL_GRAD["f32"], what, scale=float(np.linalg.norm(lo[3])))
    e = abs(hi[5] - lo[5]) / lo[5]
    print(f"{what}: fused loss {e:.3e} (bound {TOL_FIT['f32'][0]:.1e})")
    assert e <= TOL_FIT["f32"][0]


# ---- 9. group invariances
@pytest.mark.parametrize("inv,dx", [(inv, dx) for inv in ("rel_pos", "norm_rel_pos") for dx in CD.DXS])
def test_translation_and_rotation(cuda, inv, dx):
    t = _t(cuda)
    c = CD.problem(inv, dx, CD.TILES)
    nef, P = _model(cuda, c, "f32")
    moves = {"translation": (c.x + CD.translation(dx), c.p + CD.translation(dx))}
    if inv == "norm_rel_pos" and dx == 3:
        moves["rotation"] = (c.x @ CD.rotation().T, c.p @ CD.rotation().T)
    with torch.no_grad():
        base = nef.apply(P, t(c.x), t(c.p), t(c.a), t(c.s))
        for name, (x, p) in moves.items():
            out = nef.apply(P, t(x), t(p), t(c.a), t(c.s))
            e = float((out - base).abs().max() / base.abs().max())
            print(f"{name} {inv} dx={dx}: {e:.3e} of max|out| (bound {TOL_MOVED:.1e})")
            assert e < TOL_MOVED
    _check_out(_np(base), c.out, TAU["f32"], f"{inv} dx={dx}")


# ======================================================================= B. latent_dim
B_CASES = [(C, 9, "rel_pos_periodic") for C in CD.C_LIST] + [(C, 37, "rel_pos_periodic") for C in CD.C_DEEP] + [(130, 9, "ponita")]


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("C,Z,inv", B_CASES)
def test_latent_width(cuda, bwd_variant, C, Z, inv, precision):
    c = CD.latent_problem(C, Z, inv)
    g = CD.backward(c)
    out, gp, ga, gs = hip_grads(cuda, build_nef(c.cfg, precision), c.prm, c.x, c.p, c.a, c.s, c.w)
    what = f"latent_dim {C} Z={Z} {inv} {bwd_variant} {precision}"
    assert ga.shape == (2, Z, C)
    _check_out(out, c.out, TAU[precision], what)
    _check_rel(_latent_pairs((gp, ga, gs), g), TOL_GRAD[precision], what)
    rows = np.linalg.norm((ga - g.ga).reshape(-1, C), axis=0) / max(np.linalg.norm(g.ga.reshape(-1, C), axis=0).max(), 1e-300)
    print(f"{what}: d a per channel, worst {int(np.argmax(rows))} at {rows.max():.3e} of the largest channel; channels >= 128: "
          f"{rows[128:].max() if C > 128 else 0.0:.3e}")
    assert (rows < TOL_GRAD[precision]).all()


@pytest.mark.parametrize("C,Z", [(C, 9) for C in CD.C_LIST] + [(130, 37)])
def test_latent_width_weight_gradients(cuda, C, Z):
    c = CD.latent_problem(C, Z)
    g = CD.backward(c)
    out, hg, hp, ha, hs = WG.hip(cuda, build_nef(c.cfg, "f32"), c.prm, c.x, c.p, c.a, c.s, c.w)
    what = f"weight gradients latent_dim {C} Z={Z}"
    _check_out(out, c.out, TAU["f32"], what)
    es = _check_weight_grads(WG.TENSOR_PATHS, hg, g.gw, what)
    stem = [i for i, path in enumerate(WG.TENSOR_PATHS) if path[0] == "latent_stem"]
    assert len(stem) == 2 and sorted((hg[i].shape for i in stem), key=len) == [(64,), (C, 64)]
    for i in stem:
        name = "/".join(WG.TENSOR_PATHS[i])
        print(f"{what}: {name} {hg[i].shape} {es[name]:.3e} (bound {WG.TOL['f32']:.1e})")
        if hg[i].ndim == 2:                                   # every one of the C rows, not their norm alone
            rows = np.linalg.norm(hg[i] - g.gw[i], axis=1) / np.linalg.norm(g.gw[i], axis=1).max()
            print(f"{what}: {name} per row, worst {int(np.argmax(rows))} at {rows.max():.3e} of the largest row")
            assert (rows < WG.TOL["f32"]).all()


@pytest.mark.parametrize("C,Z", [(C, Z) for C in CD.C_DEEP for Z in (9, 37)])
def test_latent_width_forward_mode(cuda, C, Z):
    """f32: nef.tangent along da alone, nef.gn_product (its ga per channel), and one CG iteration through fitting.cg_solve against the
    fp64 formulas of tests/gn_ref.py (alpha = r . r / r . (G + lam) r, x = alpha r; the GN bound: alpha carries the product's error)"""
    t = _t(cuda)
    c = CD.latent_problem(C, Z)
    tg, r = CD.tangents(c), CD.gn(c)
    nef, P = _model(cuda, c, "f32")
    args = (P, t(c.x), t(c.p), t(c.a), t(c.s))
    what = f"latent_dim {C} Z={Z}"
    _check_tangent(*nef.tangent(*args, da=t(tg.v[1])), c, "da", "f32", f"tangent along da, {what}")
    got = nef.gn_product(*args, vp=t(tg.v[0]), va=t(tg.v[1]), vwindow=t(tg.v[2]), grad_scale=r.gs, weight=t(r.wt))
    torch.cuda.synchronize()
    GN._check(got, r.ref, GN.TOL["f32"], f"gn_product {what}")
    rows = np.linalg.norm((_np(got[1]) - r.ref[1]).reshape(-1, C), axis=0) / np.linalg.norm(r.ref[1].reshape(-1, C), axis=0).max()
    print(f"gn_product {what}: ga per channel, worst {int(np.argmax(rows))} at {rows.max():.3e} of the largest channel")
    assert (rows < GN.TOL["f32"]).all()
    k = CD.cg_step(c)
    B = c.B
    matvec = lambda d: nef.gn_product(*args, vp=d[0], va=d[1], grad_scale=float(B))[:2]
    xs = cg_solve(matvec, (t(k.rhs[0]), t(k.rhs[1])), t(k.lam), 1)
    torch.cuda.synchronize()
    _check_rel([("x_p", _np(xs[0]), k.x[0]), ("x_a", _np(xs[1]), k.x[1])], GN.TOL["f32"], f"cg_solve, one iteration, {what}")


@pytest.mark.parametrize("C", CD.C_DEEP)
def test_latent_width_fit_latents_step(cuda, monkeypatch, C):
    """the auto-decoder's latent-only step (enf_fit_step_w + enf_table_adam_update on rows C wide): the problem and every assertion of
    tests/test_gpu_autodec_fit.py::test_one_step_from_a_zero_adam_state with its latent_dim set to C"""
    from tests import test_gpu_autodec_fit as ADF
    monkeypatch.setattr(ADF, "C", C)
    monkeypatch.setattr(ADF, "_ORACLE", {})
    pb = ADF._problem("rel_pos_periodic")
    assert pb.table["a"].shape == (ADF.S, ADF.Z, C) and 0.5 <= float(pb.table["gaussian_window"].mean()) <= 1.5
    ADF._check_step(cuda, pb, "plain", "f32")


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("C", CD.C_DEEP)
def test_latent_width_inner_loop(cuda, C, precision):
    """two steps with default_meta_sgd_lrs(C): C per-channel rates into enf_meta_sgd_update"""
    t = _t(cuda)
    c = CD.latent_problem(C)
    q = CD.inner(c, Ns=20)
    nef, P = _model(cuda, c, precision)
    lrs = default_meta_sgd_lrs(C, lr_p=0.3, lr_a=2.0, device=cuda)
    assert lrs["a"].shape == (C,) and all(np.array_equal(_np(lrs[k]), CD.f32(q.lrs[k])) for k in q.lrs)
    loss, fit = inner_loop(nef, P, {k: t(v) for k, v in q.lat0.items()}, lrs, t(q.coords), t(q.img), torch.tensor(q.masks, device=cuda))
    torch.cuda.synchronize()
    assert fit["a"].shape == (c.B, c.Z, C)
    _check_inner(loss, fit, q.shared, q.lat0, c.B, precision, f"inner loop latent_dim {C} {precision}")
