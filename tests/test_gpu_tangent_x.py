"""Directional derivatives on the GPU (include/enf_hip.h, "Directional derivatives"): EquivariantCrossAttentionNeF.tangent with
``xdot`` and fitting.decode_directional / decode_material_derivative against the fp64 Jacobian-vector product of the oracle over
(x, p, a, sigma) (tests/tangent_x_ref.py, pinned by tests/test_tangent_x_host.py), against the shipped reverse-mode calls
(nef.jacobian, nef.query_vjp) and against identities that need no oracle.

Error measure: the relative Frobenius norm over the whole (B, N, O) tangent.  Bounds: the project's contracts for a derivative of
``out`` through this chain (tests/test_gpu_tangent.py): 5e-4 in f32, 7e-2 in bf16; ``out`` of the same call against the
oracle: 2e-5 in f32, 3e-2 in bf16 on max|err| / max|ref|.
Measured (MI355X): f32 2.3e-7 .. 1.8e-6 in every case; bf16 1.3e-2 .. 4.8e-2 (ponita with xdot alone is the closest to the bound);
against nef.jacobian 5.8e-7 .. 1.5e-6, against nef.query_vjp 7.5e-8 .. 8.9e-6; the translation sums 0 exactly, abs_pos 1.02."""
import ctypes
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

from enf_pde_amd import _lib
from tests.helpers import build_nef
from tests.tangent_x_ref import INVARIANTS, CASES_3D, case, oracle_jvp_x, rel

pytestmark = pytest.mark.gpu

TOL = {"f32": 5e-4, "bf16": 7e-2}
TOL_OUT = {"f32": 2e-5, "bf16": 3e-2}


def _t(cuda):
    return lambda v: None if v is None else torch.tensor(np.asarray(v), dtype=torch.float32, device=cuda)


def _model(cuda, c, precision):
    nef = build_nef(c[0], precision)
    return nef, nef.load_params(c[1], device=cuda)


def _run(cuda, c, precision, latent=True, xdot="case", x=None, model=None):
    """nef.tangent on a case of tests/tangent_x_ref.py: its xdot (or the tensor / None given), with its latent tangents or without"""
    cfg, prm, (x0, p, a, s), xd, (dp, da, ds) = c[:5]
    nef, P = model or _model(cuda, c, precision)
    t = _t(cuda)
    kw = dict(dp=t(dp), da=t(da), dwindow=t(ds)) if latent else {}
    return nef.tangent(P, t(x0) if x is None else x, t(p), t(a), t(s), xdot=t(xd) if isinstance(xdot, str) else xdot, **kw)


def _check(out, tan, out_ref, tan_ref, precision, what):
    e = rel(tan.double().cpu().numpy(), tan_ref)
    eo = float(np.abs(out.double().cpu().numpy() - out_ref).max() / np.abs(out_ref).max())
    print(f"{what} {precision}: relative tangent error {e:.3e} (bound {TOL[precision]:.1e}), out {eo:.3e} (bound {TOL_OUT[precision]:.1e})")
    assert tan.shape == tan_ref.shape and out.shape == out_ref.shape
    assert torch.isfinite(tan).all() and e < TOL[precision], (what, e)
    assert eo < TOL_OUT[precision], (what, eo)
    return e


# ---- 1. oracle parity, every served invariant, at the shape the reference was validated at
@pytest.mark.parametrize("precision", ["f32", "bf16"])
@pytest.mark.parametrize("latent", [False, True], ids=["xdot alone", "all four"])
@pytest.mark.parametrize("inv", INVARIANTS)
def test_tangent_x_matches_oracle_for_every_invariant(cuda, inv, latent, precision):
    c = case(inv)
    out, tan = _run(cuda, c, precision, latent=latent)
    _check(out, tan, c[5], c[7] if latent else c[6], precision, f"{inv} {'all four' if latent else 'xdot alone'}")


# ---- 2. the other instantiations, xdot together with the latent tangents
@pytest.mark.parametrize("name,inv,D,H,B,N,Z,num_in,precision", [
    ("128x2", "rel_pos_periodic", 128, 2, 2, 130, 9, 2, "f32"),    # three query tiles per signal and a partial one, three latent rounds
    ("128x2", "rel_pos_periodic", 128, 2, 2, 130, 9, 2, "bf16"),
    ("128x1", "rel_pos_periodic", 128, 1, 2, 40, 5, 2, "f32"),
    ("128x1", "rel_pos_periodic", 128, 1, 2, 20, 7, 2, "bf16"),
    ("64x4", "rel_pos_periodic", 64, 4, 2, 40, 5, 2, "f32"),
    ("64x4", "rel_pos_periodic", 64, 4, 2, 20, 7, 2, "bf16"),
    ("64x1", "rel_pos_periodic", 64, 1, 2, 20, 7, 2, "f32"),
    ("64x1", "rel_pos_periodic", 64, 1, 2, 20, 7, 2, "bf16"),
    ("16x2 padded", "polar_periodic", 16, 2, 2, 40, 5, 2, "f32"),  # zero-padded to 64 wide: d_true
    ("32x3 padded", "rel_pos", 32, 3, 2, 40, 5, 2, "f32"),         # 3 -> 4 heads: h_true
    ("3-D rel_pos", "rel_pos", 64, 2, 3, 50, 7, 3, "f32"),         # dx = 3: the third component of xdot
    ("3-D abs_pos", "abs_pos", 64, 2, 3, 50, 7, 3, "f32"),
    ("3-D norm_rel_pos", "norm_rel_pos", 64, 2, 3, 50, 7, 3, "f32"),
    ("Z=1", "rel_pos_periodic", 64, 2, 2, 20, 1, 2, "f32"),        # one latent: the softmax has one term, only the value path moves
    ("N=1", "rel_pos_periodic", 64, 2, 2, 1, 7, 2, "f32")])        # one query: 15 clamped columns read row 0 of x and of xdot
def test_tangent_x_other_instantiations(cuda, name, inv, D, H, B, N, Z, num_in, precision):
    c = case(inv, D=D, H=H, B=B, N=N, Z=Z, num_in=num_in)
    out, tan = _run(cuda, c, precision)
    _check(out, tan, c[5], c[7], precision, name)
    if num_in == 3:
        out, tan = _run(cuda, c, precision, latent=False)
        _check(out, tan, c[5], c[6], precision, name + " xdot alone")


# ---- 3. forward mode against reverse mode on the GPU: unit directions against the columns of nef.jacobian
@pytest.mark.parametrize("inv", INVARIANTS)
def test_tangent_x_unit_directions_are_the_columns_of_the_jacobian(cuda, inv):
    """1e-3 = the sum of the two f32 contracts (5e-4 each for a derivative of out through the chain)."""
    c = case(inv)
    x = _t(cuda)(c[2][0])
    nef, P = _model(cuda, c, "f32")
    nef.deterministic = True
    t = _t(cuda)
    _, jac = nef.jacobian(P, x, *(t(v) for v in c[2][1:]))
    for i in range(x.shape[-1]):
        e = torch.zeros_like(x)
        e[..., i] = 1.0
        _, tan = _run(cuda, c, "f32", latent=False, xdot=e, model=(nef, P))
        err = float((tan - jac[..., i]).norm() / jac[..., i].norm())
        print(f"{inv}: tangent(xdot = e_{i}) against jac[..., {i}]: {err:.3e} (bound 1.0e-03)")
        assert float(jac[..., i].norm()) > 0 and err < 1e-3


# ---- 4. duality with the query backward, no oracle: <w, J_x xdot> against <J_x^T w, xdot>
@pytest.mark.parametrize("inv", INVARIANTS)
def test_tangent_x_is_dual_to_query_vjp(cuda, inv):
    """1e-3 = the sum of the two f32 contracts."""
    c = case(inv)
    t = _t(cuda)
    x, p, a, s = (t(v) for v in c[2])
    xd = t(c[3])
    nef, P = _model(cuda, c, "f32")
    w = t(np.random.default_rng(9).standard_normal(c[5].shape))
    _, tan = nef.tangent(P, x, p, a, s, xdot=xd)
    g = nef.query_vjp(P, x, p, a, s, w)
    lhs, rhs = float((w.double() * tan.double()).sum()), float((g.double() * xd.double()).sum())
    e = abs(lhs - rhs) / abs(rhs)
    print(f"{inv}: <w, tan> = {lhs:.6e}, <query_vjp(w), xdot> = {rhs:.6e}, relative difference {e:.3e} (bound 1.0e-03)")
    assert e < 1e-3


# ---- 5. translation: moving every query and every latent position by the same e changes nothing where only x - p enters
@pytest.mark.parametrize("inv", ["rel_pos", "norm_rel_pos", "rel_pos_periodic", "ponita", "abs_pos"])
def test_tangent_x_translation_identity(cuda, inv):
    """tan(xdot = e on every query) + tan(dp = e on every latent's position) = 0 for the invariants of x - p; the oracle gives exactly
    0 in fp64 (asserted: 1e-12).  f32 bound 1e-3 relative to |tan| (the sum of two f32 contracts); the kernel forms the pair's pose
    tangent as tp - tq, so the two calls are each other's negation bit for bit and the measured sum is exactly 0.
    abs_pos sees x itself: there the sum is as large as the tangents (the oracle's ratio is asserted to exceed 0.1) and the GPU's sum
    must match the oracle's sum, not vanish."""
    c = case(inv)
    cfg, prm, (x, p, a, s) = c[:3]
    e = np.array([0.6, -0.8])
    xd = np.broadcast_to(e, x.shape).copy()
    dp = np.zeros_like(p)
    dp[..., :2] = e
    _, ref_x = oracle_jvp_x(cfg, prm, x, p, a, s, xd, None, None, None)
    _, ref_p = oracle_jvp_x(cfg, prm, x, p, a, s, None, dp, None, None)
    ratio_ref = float(np.linalg.norm(ref_x + ref_p) / np.linalg.norm(ref_x))
    t = _t(cuda)
    nef, P = _model(cuda, c, "f32")
    args = (P, t(x), t(p), t(a), t(s))
    _, tan_x = nef.tangent(*args, xdot=t(xd))
    _, tan_p = nef.tangent(*args, dp=t(dp))
    ratio = float((tan_x + tan_p).norm() / tan_x.norm())
    print(f"{inv}: |tan_x + tan_p| / |tan_x| = {ratio:.3e} on the GPU, {ratio_ref:.3e} in the oracle")
    assert float(tan_x.norm()) > 0
    if inv == "abs_pos":
        assert ratio_ref > 0.1 and ratio > 0.1
        assert rel((tan_x + tan_p).double().cpu().numpy(), ref_x + ref_p) < 1e-3
    else:
        assert ratio_ref < 1e-12 and ratio < 1e-3


# ---- 6. exact zeros
def test_tangent_x_exact_zeros(cuda):
    c = case("rel_pos_periodic")
    zero = torch.zeros(c[2][0].shape, device=cuda)
    for precision in ("f32", "bf16"):
        out, tan = _run(cuda, c, precision, latent=False, xdot=zero)
        assert torch.equal(tan, torch.zeros_like(tan))
        assert float(np.abs(out.double().cpu().numpy() - c[5]).max() / np.abs(c[5]).max()) < TOL_OUT[precision]


# ---- 7. bits
def _raw(cuda, nef, P, fn_name, x, xstride, xdot, xdstride, p, a, s, tang, poison=0xFF):
    """one C-ABI call on caller-owned buffers and a poisoned workspace: (out, tan)"""
    from enf_pde_amd.enf.models import _ptr
    lib = _lib.load()
    B, Z, N = p.shape[0], p.shape[1], x.shape[-2]
    desc = nef._desc(B, N, Z)
    nbytes = int(lib.enf_field_tangent_workspace_bytes(ctypes.byref(desc)))
    assert nbytes > 0
    ws = torch.full((nbytes,), poison, device=cuda, dtype=torch.uint8)
    out = torch.full((B, N, nef.num_out), float("nan"), device=cuda)
    tan = torch.full((B, N, nef.num_out), float("nan"), device=cuda)
    packed = nef.pack(P)
    st = _lib.stream(cuda)
    dp, da, ds = tang
    if fn_name == "enf_field_tangent":
        _lib.launch(cuda, lib.enf_field_tangent, ctypes.byref(desc), _ptr(x), xstride, _ptr(p), _ptr(a), _ptr(s), _ptr(dp), _ptr(da),
                    _ptr(ds), _ptr(packed), _ptr(out), _ptr(tan), _ptr(ws), st)
    else:
        _lib.launch(cuda, lib.enf_field_tangent_x, ctypes.byref(desc), _ptr(x), xstride, _ptr(xdot), xdstride, _ptr(p), _ptr(a), _ptr(s),
                    _ptr(dp), _ptr(da), _ptr(ds), _ptr(packed), _ptr(out), _ptr(tan), _ptr(ws), st)
    torch.cuda.synchronize()
    return out, tan


@pytest.mark.parametrize("precision", ["f32", "bf16"])
def test_c_abi_null_xdot_is_enf_field_tangent_and_xdot_alone_is_served(cuda, precision):
    c = case("ponita")
    t = _t(cuda)
    x, p, a, s = (t(v) for v in c[2])
    xd, tang = t(c[3]), tuple(t(v) for v in c[4])
    nef, P = _model(cuda, c, precision)
    B, N, dx = x.shape
    o0, t0 = _raw(cuda, nef, P, "enf_field_tangent", x, N * dx, None, 0, p, a, s, tang)
    o1, t1 = _raw(cuda, nef, P, "enf_field_tangent_x", x, N * dx, None, 0, p, a, s, tang, poison=0x55)
    assert torch.equal(o0, o1) and torch.equal(t0, t1) and torch.isfinite(t0).all() and float(t0.abs().max()) > 0
    # xdot alone passes the pointer checks (three NULL latent tangents); on a NaN workspace the table's tangent must have been zeroed
    o2, t2 = _raw(cuda, nef, P, "enf_field_tangent_x", x, N * dx, xd, N * dx, p, a, s, (None, None, None))
    _check(o2, t2, c[5], c[6], precision, "C-ABI, xdot alone")


@pytest.mark.parametrize("precision", ["f32", "bf16"])
def test_tangent_x_equal_bits_on_differently_poisoned_workspaces(cuda, precision):
    c = case("rel_pos_periodic", D=128, H=2, B=2, N=130, Z=9)
    model = _model(cuda, c, precision)
    for latent in (False, True):
        runs = [_run(cuda, c, precision, latent=latent, model=model)]
        assert len(model[0]._ws_cache) == 1
        for byte in (0xFF, 0x55):                                        # NaNs, then ordinary positive numbers
            for ws in model[0]._ws_cache.values():
                ws.fill_(byte)
            runs.append(_run(cuda, c, precision, latent=latent, model=model))
        for o, tn in runs[1:]:
            assert torch.equal(o, runs[0][0]) and torch.equal(tn, runs[0][1])
        assert torch.isfinite(runs[0][1]).all() and float(runs[0][1].abs().max()) > 0


def test_tangent_x_broadcast_direction_and_broadcast_grid(cuda):
    c = case("ponita")
    t = _t(cuda)
    cfg, prm, (x, p, a, s), xd = c[:4]
    model = _model(cuda, c, "f32")
    d0 = t(xd[0])                                                        # (N, dx): signal 0's direction for everybody
    o0, t0 = _run(cuda, c, "f32", xdot=d0[None].expand(3, -1, -1), model=model)       # stride-0 batch
    o1, t1 = _run(cuda, c, "f32", xdot=d0[None].repeat(3, 1, 1), model=model)
    assert torch.equal(o0, o1) and torch.equal(t0, t1) and float(t0.abs().max()) > 0
    # a stride-0 x with a per-signal xdot: the two batch strides are independent
    xs = np.broadcast_to(x[0], x.shape).copy()
    out_ref, tan_ref = oracle_jvp_x(cfg, prm, xs, p, a, s, xd, *c[4])
    o2, t2 = _run(cuda, c, "f32", x=t(x[0])[None].expand(3, -1, -1), model=model)
    _check(o2, t2, out_ref, tan_ref, "f32", "stride-0 x, per-signal xdot")
    o3, t3 = _run(cuda, c, "f32", x=t(xs), model=model)
    assert torch.equal(o2, o3) and torch.equal(t2, t3)


# ---- 8. the helpers
def test_decode_directional_chunked_equals_unchunked(cuda):
    from enf_pde_amd.fitting import decode_directional
    c = case("latitude_periodic")
    t = _t(cuda)
    x, p, a, s = (t(v) for v in c[2])
    nef, P = _model(cuda, c, "f32")
    for coords, direction in ((x, t(c[3])), (x[0], t(c[3][0]))):        # per-signal, then one grid and one direction for the batch
        u, du = decode_directional(nef, P, coords, p, a, s, direction)
        u1, du1 = decode_directional(nef, P, coords, p, a, s, direction, chunk=32)   # 32, 18
        assert torch.equal(u, u1) and torch.equal(du, du1) and float(du.abs().max()) > 0
    _check(*decode_directional(nef, P, x, p, a, s, t(c[3]), chunk=32), c[5], c[6], "f32", "decode_directional")


def test_decode_material_derivative_with_a_ponita_ode(cuda):
    """Du/Dt from ONE tangent pass against the composed route on the GPU: decode_tendency plus nef.jacobian contracted with the
    velocity.  Both sides carry the f32 contract; bound 5e-4 relative to |Du/Dt|."""
    from enf_pde_amd.enf.steerable_attention.invariant import get_sa_invariant
    from enf_pde_amd.fitting import decode_material_derivative, decode_tendency, PonitaODEGen
    from oracle import ode_ref_np as O
    from tests.test_ode_oracle import ode_cfg
    B, N, Z, C = 2, 50, 9, 32
    c = case("ponita", C=C, B=B, N=N, Z=Z)
    ocfg = ode_cfg("ponita", num_hidden=128, basis_dim=128, num_layers=3, kernel_size=0.2)      # the ODE of tests/test_gpu_tangent.py
    ode = PonitaODEGen(num_hidden=128, num_layers=3, scalar_num_out=C, vec_num_out=1,
                       invariant=get_sa_invariant(NS(invariant_type="ponita", num_in=2)), basis_dim=128, degree=ocfg["degree"],
                       widening_factor=ocfg["widening_factor"], global_pool=False, kernel_size=ocfg["kernel_size"])
    oprm = ode.load_params(O.init_ponita_ode(3, ocfg, latent_dim=C, jitter=0.1, readout_scale=1.0), device=cuda)
    t = _t(cuda)
    x, p, a, s = (t(v) for v in c[2])
    vel = t(c[3])
    nef, P = _model(cuda, c, "f32")
    nef.deterministic = True
    coords = x[0]                                                        # one grid for the batch, a velocity per signal
    u, dudt = decode_material_derivative(nef, P, ode, oprm, coords, p, a, s, vel)
    u0, ut = decode_tendency(nef, P, ode, oprm, coords, p, a, s)
    _, jac = nef.jacobian(P, coords[None].expand(B, -1, -1), p, a, s)
    want = ut + (jac * vel[:, :, None, :]).sum(-1)
    e = float((dudt - want).norm() / want.norm())
    print(f"material derivative: one pass against tendency + jacobian . velocity: {e:.3e} (bound 5.0e-04); "
          f"|u_t| = {float(ut.norm()):.3e}, |c . grad u| = {float((want - ut).norm()):.3e}")
    assert float((u - u0).abs().max() / u0.abs().max()) < TOL_OUT["f32"] and float(ut.norm()) > 0 and float((want - ut).norm()) > 0
    assert e < 5e-4
    u1, d1 = decode_material_derivative(nef, P, ode, oprm, coords, p, a, s, vel, chunk=32)
    assert torch.equal(u, u1) and torch.equal(dudt, d1)
