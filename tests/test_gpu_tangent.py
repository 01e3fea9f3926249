"""Tendency fields on the GPU (include/enf_hip.h, "Tendency fields"): EquivariantCrossAttentionNeF.tangent and
fitting.decode_tangent / decode_tendency against the fp64 Jacobian-vector product of the oracle (tests/tangent_ref.py, pinned by
tests/test_tangent_host.py).

Error measure: the relative Frobenius norm over the whole (B, N, O) tangent.  Bounds: the project's contracts for the derivative of
``out`` through this chain ("Derivative fields"): 5e-4 in f32, 7e-2 in bf16.  ``out`` of the same call against the
oracle: the forward's tolerances on max|err| / max|ref| (tests/test_gpu_forward.py): 2e-5 in f32, 3e-2 in bf16."""
import ctypes
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

from enf_pde_amd import _lib
from tests.helpers import make_cfg, build_nef
from tests.tangent_ref import INVARIANTS, case, oracle_jvp, rel

pytestmark = pytest.mark.gpu

TOL = {"f32": 5e-4, "bf16": 7e-2}
TOL_OUT = {"f32": 2e-5, "bf16": 3e-2}


def _t(cuda):
    return lambda v: None if v is None else torch.tensor(np.asarray(v), dtype=torch.float32, device=cuda)


def _run(cuda, c, precision, tang=None, x=None):
    """nef.tangent on a case of tests/tangent_ref.py (its own tangents unless `tang` is given)"""
    cfg, prm, (x0, p, a, s), tg = c[:4]
    dp, da, ds = tg if tang is None else tang
    nef = build_nef(cfg, precision)
    t = _t(cuda)
    return nef.tangent(nef.load_params(prm, device=cuda), t(x0) if x is None else x, t(p), t(a), t(s) if cfg["use_gaussian_window"] else None,
                       dp=t(dp), da=t(da), dwindow=t(ds))


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
@pytest.mark.parametrize("inv", INVARIANTS)
def test_tangent_matches_oracle_for_every_invariant(cuda, inv, precision):
    c = case(inv)
    out, tan = _run(cuda, c, precision)
    _check(out, tan, c[4], c[5], precision, inv)


# ---- 2. duality with the shipped backward, no oracle: <w, J v> against <J^T w, v>, both sides on the GPU in f32
@pytest.mark.parametrize("inv", INVARIANTS)
def test_tangent_is_dual_to_the_latent_backward(cuda, inv):
    """7e-4 = the sum of the two f32 contracts (5e-4 for the derivative of out through the chain, 2e-4 for the latent gradients)."""
    cfg, prm, (x, p, a, s), (dp, da, ds) = case(inv)[:4]
    nef = build_nef(cfg, "f32")
    P = nef.load_params(prm, device=cuda)
    t = _t(cuda)
    w = t(np.random.default_rng(9).standard_normal((3, 50, 2)))
    _, tan = nef.tangent(P, t(x), t(p), t(a), t(s), dp=t(dp), da=t(da), dwindow=t(ds))
    hp, ha, hs = (t(v).requires_grad_(True) for v in (p, a, s))
    (nef.apply(P, t(x), hp, ha, hs) * w).sum().backward()
    lhs = float((w.double() * tan.double()).sum())
    rhs = float((hp.grad.double() * t(dp).double()).sum() + (ha.grad.double() * t(da).double()).sum() + (hs.grad.double() * t(ds).double()).sum())
    e = abs(lhs - rhs) / abs(rhs)
    print(f"{inv}: <w, tan> = {lhs:.6e}, <grad, v> = {rhs:.6e}, relative difference {e:.3e} (bound 7.0e-04)")
    assert e <= 7e-4


# ---- 3. the other instantiations
@pytest.mark.parametrize("name,inv,D,H,B,N,Z,precision", [
    ("128x2", "rel_pos_periodic", 128, 2, 2, 130, 9, "f32"),       # three query tiles per signal and a partial one, three latent rounds
    ("128x2", "rel_pos_periodic", 128, 2, 2, 130, 9, "bf16"),
    ("128x1", "rel_pos_periodic", 128, 1, 2, 40, 5, "f32"),
    ("64x4", "rel_pos_periodic", 64, 4, 2, 40, 5, "f32"),
    ("64x1", "rel_pos_periodic", 64, 1, 2, 20, 7, "f32"),          # with the rows above and the default 64x2: every (D, H) pair of the
    ("64x1", "rel_pos_periodic", 64, 1, 2, 20, 7, "bf16"),         # dispatch in both precisions
    ("128x1", "rel_pos_periodic", 128, 1, 2, 20, 7, "bf16"),
    ("64x4", "rel_pos_periodic", 64, 4, 2, 20, 7, "bf16"),
    ("16x2 padded", "polar_periodic", 16, 2, 2, 40, 5, "f32"),     # zero-padded to 64 wide: d_true
    ("32x3 padded", "rel_pos", 32, 3, 2, 40, 5, "f32")])           # 3 -> 4 heads: h_true
def test_tangent_other_instantiations(cuda, name, inv, D, H, B, N, Z, precision):
    c = case(inv, D=D, H=H, B=B, N=N, Z=Z)
    out, tan = _run(cuda, c, precision)
    _check(out, tan, c[4], c[5], precision, name)


# ---- 4. edge cases, f32
@pytest.mark.parametrize("B,N,Z", [(2, 20, 1), (2, 1, 7)])        # one latent: the softmax has one term, only the value path moves; one query
def test_tangent_single_latent_and_single_query(cuda, B, N, Z):
    c = case("rel_pos_periodic", B=B, N=N, Z=Z)
    out, tan = _run(cuda, c, "f32")
    _check(out, tan, c[4], c[5], "f32", f"Z={Z} N={N}")


def test_tangent_broadcast_grid_equals_materialised(cuda):
    c = case("ponita")
    x = _t(cuda)(c[2][0][0])                                         # (N, dx): signal 0's points for everybody
    o0, t0 = _run(cuda, c, "f32", x=x[None].expand(3, -1, -1))       # stride-0 batch
    o1, t1 = _run(cuda, c, "f32", x=x[None].repeat(3, 1, 1))
    assert torch.equal(o0, o1) and torch.equal(t0, t1) and float(t0.abs().max()) > 0


@pytest.mark.parametrize("which", [0, 1, 2])
def test_tangent_each_direction_alone(cuda, which):
    c = case("latitude_periodic")
    cfg, prm, xpas, tg = c[:4]
    alone = tuple(v if i == which else None for i, v in enumerate(tg))
    out_ref, tan_ref = oracle_jvp(cfg, prm, *xpas, *alone)
    out, tan = _run(cuda, c, "f32", tang=alone)
    _check(out, tan, out_ref, tan_ref, "f32", ("dp", "da", "dwindow")[which] + " alone")


def test_tangent_exact_zeros(cuda):
    c = case("rel_pos_periodic")
    zeros = tuple(np.zeros_like(v) for v in c[3])
    _, tan = _run(cuda, c, "f32", tang=zeros)
    assert torch.equal(tan, torch.zeros_like(tan))                   # a zero tangent
    nw = case("rel_pos_periodic", use_window=False)
    out, tan = _run(cuda, nw, "f32", tang=(None, None, nw[3][2]))
    assert torch.equal(tan, torch.zeros_like(tan))                   # the window's tangent of a model without a window
    assert float(np.abs(out.double().cpu().numpy() - nw[4]).max() / np.abs(nw[4]).max()) < TOL_OUT["f32"]


def test_tangent_is_linear_in_the_direction(cuda):
    c = case("polar_periodic")
    v1 = c[3]
    rng = np.random.default_rng(11)
    v2 = tuple(rng.standard_normal(v.shape) * sc for v, sc in zip(v1, (0.3, 1.0, 0.1)))
    alpha = 0.7
    _, t1 = _run(cuda, c, "f32")
    _, t2 = _run(cuda, c, "f32", tang=v2)
    _, t12 = _run(cuda, c, "f32", tang=tuple(alpha * a + b for a, b in zip(v1, v2)))
    e = float((t12 - (alpha * t1 + t2)).norm() / t12.norm())
    print(f"linearity: {e:.3e} (bound 1.0e-05)")
    assert e < 1e-5


# ---- 5. no dependence on what the workspace held
@pytest.mark.parametrize("precision", ["f32", "bf16"])
def test_tangent_equal_bits_on_differently_poisoned_workspaces(cuda, precision):
    cfg, prm, (x, p, a, s), (dp, da, ds) = case("rel_pos_periodic", D=128, H=2, B=2, N=130, Z=9)[:4]
    nef = build_nef(cfg, precision)
    P = nef.load_params(prm, device=cuda)
    t = _t(cuda)
    args = (P, t(x), t(p), t(a), t(s))
    kw = dict(dp=t(dp), da=t(da), dwindow=t(ds))
    runs = [nef.tangent(*args, **kw)]
    assert len(nef._ws_cache) == 1
    for byte in (0xFF, 0x55):                                        # NaNs, then ordinary positive numbers
        for ws in nef._ws_cache.values():
            ws.fill_(byte)
        runs.append(nef.tangent(*args, **kw))
    for o, tn in runs[1:]:
        assert torch.equal(o, runs[0][0]) and torch.equal(tn, runs[0][1])
    assert torch.isfinite(runs[0][1]).all()


# ---- 6. what the call does not serve
def test_tangent_refusals(cuda):
    from tests.ffn_ref import build_nef_ffn
    lib = _lib.load()
    z = lambda *shape: torch.zeros(*shape, device=cuda)
    B, N, Z = 2, 20, 5
    a, s = z(B, Z, 8), torch.ones(B, Z, 1, device=cuda)
    for inv in ("ball", "ball_lat"):
        with pytest.raises(NotImplementedError):
            build_nef(make_cfg(inv, D=64, H=2, C=8, O=2), "f32").tangent(None, z(B, N, 3), z(B, Z, 4), a, s, da=a)
    with pytest.raises(NotImplementedError):
        build_nef_ffn(make_cfg("rel_pos_periodic", D=64, H=2, C=8, O=2), "f32").tangent(None, z(B, N, 2), z(B, Z, 2), a, s, da=a)
    nef = build_nef(make_cfg("rel_pos_periodic", D=64, H=2, C=8, O=2), "f32")
    buf = nef.relu_mask_buffer(B, N, Z, cuda)
    with nef.relu_masks(buf, "write", B):
        with pytest.raises(NotImplementedError):
            nef.tangent(None, z(B, N, 2), z(B, Z, 2), a, s, da=a)
    # the C-ABI says the same, whatever the pointers: ENF_EUNSUPPORTED before anything is launched
    ws = torch.empty(1 << 20, device=cuda, dtype=torch.uint8)
    ptr = ctypes.c_void_p(ws.data_ptr())
    for desc in (_lib.make_desc(B, N, Z, 2, 64, 8, 2, 3, 7, 1, 0), _lib.make_desc(B, N, Z, 2, 64, 8, 2, 3, 8, 1, 0),
                 _lib.make_desc(B, N, Z, 2, 64, 8, 2, 2, 0, 1, 0, embedding=1),
                 _lib.make_desc(B, N, Z, 2, 64, 8, 2, 2, 0, 1, 0, masks=(buf, "read", B))):
        assert lib.enf_field_tangent(ctypes.byref(desc), ptr, 0, ptr, ptr, ptr, ptr, ptr, ptr, ptr, ptr, ptr, ptr, None) == -3
    # argument checks of the Python call that need device tensors
    x, p = z(B, N, 2), z(B, Z, 2)
    with pytest.raises(AssertionError):
        nef.tangent(None, x, p, a, s, da=z(B, Z, 9))
    with pytest.raises(ValueError):
        nef.tangent(None, x, p, a, s, da=a.double())
    with pytest.raises(ValueError):
        nef.tangent(None, x, p, a, s, dp=z(B, 2, Z).transpose(1, 2))


# ---- 7. d u / d t under a latent ODE
def test_decode_tendency_with_a_ponita_ode(cuda):
    from enf_pde_amd.enf.steerable_attention.invariant import get_sa_invariant
    from enf_pde_amd.fitting import decode_tendency, PonitaODEGen
    from oracle import ode_ref_np as O
    from tests.test_ode_oracle import ode_cfg
    B, N, Z, C = 2, 130, 9, 32
    cfg, prm, (x, p, a, s) = case("ponita", C=C, B=B, N=N, Z=Z)[:3]
    ocfg = ode_cfg("ponita", num_hidden=128, basis_dim=128, num_layers=3, kernel_size=0.2)      # the ODE of tests/test_gpu_ode.py at Z = 9
    ode = PonitaODEGen(num_hidden=128, num_layers=3, scalar_num_out=C, vec_num_out=1,
                       invariant=get_sa_invariant(NS(invariant_type="ponita", num_in=2)), basis_dim=128, degree=ocfg["degree"],
                       widening_factor=ocfg["widening_factor"], global_pool=False, kernel_size=ocfg["kernel_size"])
    oprm = ode.load_params(O.init_ponita_ode(3, ocfg, latent_dim=C, jitter=0.1, readout_scale=1.0), device=cuda)
    nef = build_nef(cfg, "f32")
    P = nef.load_params(prm, device=cuda)
    t = _t(cuda)
    coords = t(x[0])                                                  # one grid for the batch
    lat = (t(p), t(a), t(s))
    with torch.no_grad():
        dz = ode.apply(oprm, lat)
    n = lambda v: None if v is None else v.double().cpu().numpy().reshape(v.shape[0], v.shape[1], -1)
    xs = np.broadcast_to(x[0], (B, N, 2)).copy()
    out_ref, tan_ref = oracle_jvp(cfg, prm, xs, p, a, s, n(dz[0]), n(dz[1]), n(dz[2]))
    u, ut = decode_tendency(nef, P, ode, oprm, coords, *lat)
    assert float(np.linalg.norm(tan_ref)) > 0
    _check(u, ut, out_ref, tan_ref, "f32", "tendency")
    u1, ut1 = decode_tendency(nef, P, ode, oprm, coords, *lat, chunk=48)     # 48, 48, 34: chunked equals unchunked bit for bit
    assert torch.equal(u, u1) and torch.equal(ut, ut1)
