"""Directional derivatives without a GPU (include/enf_hip.h, "Directional derivatives"): the yardstick itself (the oracle's fp64
Jacobian-vector product along the query coordinates against central differences, against the oracle's reverse-mode Jacobian and
against the latent half of tests/tangent_ref.py), the header and the bindings, the argument checks of enf_field_tangent_x (every call
here fails its checks, so nothing is launched), the Python mirror's refusals and its checks of ``xdot``, and decode_directional /
decode_material_derivative against a stand-in model whose tangent is a known linear map.

That ``xdot`` alone PASSES the pointer checks cannot be shown here: a call that passes them launches.  tests/test_gpu_tangent_x.py
makes that call through the C-ABI on real buffers."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from enf_pde_amd import _lib
from oracle import enf_ref_torch as T
from tests.helpers import make_cfg, build_nef
from tests import tangent_ref
from tests.tangent_x_ref import INVARIANTS, CASES_3D, case, oracle_jacobian_x, oracle_jvp_x, rel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, EUNSUPPORTED = -1, -3
ALL_CASES = [(inv, 2) for inv in INVARIANTS] + [(inv, 3) for inv in CASES_3D]


@pytest.mark.parametrize("inv,num_in", ALL_CASES)
def test_reference_jvp_along_x(inv, num_in):
    """The reference every GPU test compares with, at the base shape.
    Central differences in fp64 with h = 1e-6 (the step and the bound 1e-7 of tests/test_tangent_host.py, for its reasons: truncation
    ~1e-12, rounding ~1e-10 times the cancellation, a small step because of the relu kinks).  Measured 3.4e-10 .. 3.6e-9.
    The contraction of the oracle's reverse-mode Jacobian d out / d x with xdot: exact up to fp64 summation over dx <= 3 terms, bound
    1e-12 (measured 1.0e-15 .. 2.1e-15).
    Linearity: the joint JVP along (xdot, dp, da, dsigma) equals the sum of the two separate ones to fp64 rounding, bound 1e-12
    (measured 1.2e-15 .. 1.8e-15).
    Neither half hides the other in the joint cases: |J_x xdot| / |J_z zdot| within a factor 10 of one (measured 0.37 .. 3.8)."""
    cfg, prm, (x, p, a, s), xdot, (dp, da, ds), out_ref, tan_x, tan_all = case(inv, num_in=num_in)
    tp = T.to_torch(prm, torch.float64)
    f = lambda X: T.nef_apply(tp, cfg, torch.tensor(X), torch.tensor(p), torch.tensor(a), torch.tensor(s)).numpy()
    h = 1e-6
    with torch.no_grad():
        hi, lo, mid = f(x + h * xdot), f(x - h * xdot), f(x)
    e_cd = rel((hi - lo) / (2 * h), tan_x)
    assert np.array_equal(mid, out_ref) and tan_x.shape == tan_all.shape == out_ref.shape == (3, 50, 2) and x.shape[-1] == num_in
    jac = oracle_jacobian_x(cfg, prm, x, p, a, s)
    assert jac.shape == (3, 50, 2, num_in)
    e_jac = rel(np.einsum("bnoi,bni->bno", jac, xdot), tan_x)
    if num_in == 2:
        tan_z = tangent_ref.case(inv)[5]
        assert np.array_equal(tangent_ref.case(inv)[2][0], x)             # the same inputs as the latent tangent's cases
    else:
        tan_z = oracle_jvp_x(cfg, prm, x, p, a, s, None, dp, da, ds)[1]
    e_sum = rel(tan_x + tan_z, tan_all)
    ratio = float(np.linalg.norm(tan_x) / np.linalg.norm(tan_z))
    print(f"{inv} num_in={num_in}: central differences {e_cd:.2e}, Jacobian contraction {e_jac:.2e}, joint vs sum {e_sum:.2e}, "
          f"|J_x xdot| / |J_z zdot| = {ratio:.2f}")
    assert np.linalg.norm(tan_x) > 0 and e_cd < 1e-7 and e_jac < 1e-12 and e_sum < 1e-12
    assert 0.1 < ratio < 10


def test_symbols_header_and_abi():
    with open(os.path.join(ROOT, "include", "enf_hip.h")) as f:
        h = f.read()
    assert re.search(r"#define\s+ENF_ABI_VERSION\s+2\b", h)
    lib = _lib.load()
    assert lib.enf_abi_version() == 2
    assert re.search(r"\bint\s+enf_field_tangent_x\s*\(", h)
    assert "enf_field_tangent_x" in _lib.EXPORTS and hasattr(lib, "enf_field_tangent_x")
    assert len(lib.enf_field_tangent.argtypes) == 14                      # the existing call keeps its signature
    at = lib.enf_field_tangent_x.argtypes
    assert len(at) == 16 and at[2] is ctypes.c_int64 and at[4] is ctypes.c_int64 and at[3] is ctypes.c_void_p
    decl = re.search(r"int\s+enf_field_tangent_x\s*\((.*?)\);", h, re.S).group(1)
    assert len(re.sub(r"/\*.*?\*/", "", decl, flags=re.S).split(",")) == 16
    # what the header has to say: the definition, the convention on the sphere, that xdot is only read, NULL tangents
    assert "d out[b,n,o] / d x[b,n,i]  xdot[b,n,i]" in h
    assert "no metric" in h and "never written" in h and "not all four" in h


def _mk(inv=0, O=2, window=1, emb=0, D=128, H=2):
    return _lib.make_desc(2, 70, 9, H, D, 16, O, 2 if inv < 7 else 3, inv, window, 0, embedding=emb)


def test_argument_checks_without_a_launch():
    lib = _lib.load()
    dummy = ctypes.create_string_buffer(64)
    P = ctypes.cast(dummy, ctypes.c_void_p)
    d = _mk()
    masked = _mk()
    masked.relu_masks, masked.mask_mode, masked.mask_signals = P.value, _lib.MASK_MODE["read"], 2

    def call(desc=d, x=P, xdot=P, p=P, a=P, sigma=P, dp=P, da=P, ds=P, blob=P, out=P, tan=P, ws=P):
        return lib.enf_field_tangent_x(ctypes.byref(desc), x, 0, xdot, 0, p, a, sigma, dp, da, ds, blob, out, tan, ws, None)
    for k in ("x", "p", "a", "sigma", "blob", "tan", "ws"):
        assert call(**{k: None}) == EINVAL, k
        assert call(**{k: None}, dp=None, da=None, ds=None) == EINVAL, k   # ... also when xdot is the only direction
    assert call(xdot=None, dp=None, da=None, ds=None) == EINVAL           # not all four
    unserved = (_mk(inv=7, D=64), _mk(inv=8, D=64), _mk(inv=9), _mk(emb=1), masked)      # ball, ball_lat, ponita_full, ffn, masks
    for bad in unserved:
        assert lib.enf_check_desc(ctypes.byref(bad)) == 0
        assert call(desc=bad) == EUNSUPPORTED and call(desc=bad, tan=None) == EUNSUPPORTED
        assert call(desc=bad, xdot=None, dp=None, da=None, ds=None) == EUNSUPPORTED
    bad = _mk(O=33)                                                       # the descriptor's error comes first
    assert lib.enf_check_desc(ctypes.byref(bad)) != 0
    assert call(desc=bad) == call(desc=bad, tan=None) == lib.enf_check_desc(ctypes.byref(bad))


def test_python_mirror_refusals_and_xdot_checks():
    from tests.test_gpu_layers import _nef as layered
    from tests.ffn_ref import build_nef_ffn
    B, N, Z = 2, 5, 3
    x, p, a, s = torch.zeros(B, N, 2), torch.zeros(B, Z, 2), torch.ones(B, Z, 8), torch.ones(B, Z, 1)
    xd = torch.zeros(B, N, 2)
    nef = layered(dict(make_cfg("rel_pos_periodic", D=64, H=2, C=8, O=2), num_layers=1), "f32")
    with pytest.raises(NotImplementedError, match="num_layers"):
        nef.tangent(None, x, p, a, s, xdot=xd)
    with pytest.raises(NotImplementedError, match="ffn"):
        build_nef_ffn(make_cfg("rel_pos_periodic", D=64, H=2, C=8, O=2), "f32").tangent(None, x, p, a, s, xdot=xd)
    for inv in ("ball", "ball_lat"):
        with pytest.raises(NotImplementedError, match=inv):
            build_nef(make_cfg(inv, D=64, H=2, C=8, O=2), "f32").tangent(None, torch.zeros(B, N, 3), torch.zeros(B, Z, 4), a, s,
                                                                          xdot=torch.zeros(B, N, 3))
    flat = build_nef(make_cfg("rel_pos_periodic", D=64, H=2, C=8, O=2), "f32")
    with pytest.raises(ValueError, match="xdot"):
        flat.tangent(None, x, p, a, s, xdot=None)                         # all four tangents None
    for wrong in (torch.zeros(B, N, 3), torch.zeros(B, N + 1, 2), torch.zeros(N, 2), torch.zeros(1, N, 2)):
        with pytest.raises(AssertionError, match="xdot"):
            flat.tangent(None, x, p, a, s, xdot=wrong)
    with pytest.raises(ValueError, match="xdot"):
        flat.tangent(None, x, p, a, s, xdot=xd.double())
    with pytest.raises(ValueError, match="xdot"):
        flat.tangent(None, x, p, a, s, xdot=torch.zeros(B, N, 2, device="meta"))
    # a well-formed xdot alone passes every check of the arguments: what stops the call is that there is no CPU path
    for good in (xd, xd[:1].expand(B, -1, -1), torch.zeros(B, 2, N).transpose(1, 2)):
        with pytest.raises(_lib.EnfError):
            flat.tangent(None, x, p, a, s, xdot=good)


class _StubNef:
    """out[b, n, o] = (o + 1) |x_n|^2,  tan[b, n, o] = (o + 1) ((sum dp_b + 2 sum da_b + 3 sum dw_b) x_n0 + xdot_n . (1, 10)): linear in
    the tangents; records the slices and the tangents it was handed"""

    def __init__(self):
        self.calls = []

    def tangent(self, params, x, p, a, window, dp=None, da=None, dwindow=None, xdot=None):
        self.calls.append((x.shape[1], x.stride(0), dp is None, da is None, dwindow is None,
                           None if xdot is None else (tuple(xdot.shape), xdot.stride(0))))
        ch = torch.tensor([1.0, 2.0])
        z = lambda t, k: 0.0 if t is None else k * t.sum(dim=(1, 2))
        lin = z(dp, 1.0) + z(da, 2.0) + z(dwindow, 3.0) + torch.zeros(x.shape[0])
        along = 0.0 if xdot is None else (xdot * torch.tensor([1.0, 10.0])).sum(-1, keepdim=True)
        out = (x * x).sum(-1, keepdim=True) * ch
        return out, (lin[:, None, None] * x[:, :, :1] + along) * ch


class _ThreeKeywordNef:
    """the stub of tests/test_tangent_host.py: accepts the three latent keywords and no others"""

    def __init__(self):
        self.calls = 0

    def tangent(self, params, x, p, a, window, dp=None, da=None, dwindow=None):
        self.calls += 1
        return x[..., :1] * 1.0, x[..., :1] * 2.0


class _StubOde:
    def __init__(self, window):
        self.window, self.seen = window, []

    def apply(self, params, latents):
        p, a, w = latents
        self.seen.append(torch.is_grad_enabled())
        return 0.5 * p, a * params, (None if self.window is None else torch.full_like(w, self.window))


@pytest.mark.parametrize("shared_grid,shared_dir", [(True, True), (True, False), (False, True), (False, False)])
def test_decode_directional_slices_the_direction_with_the_grid(shared_grid, shared_dir):
    from enf_pde_amd.fitting import decode_directional
    g = torch.Generator().manual_seed(0)
    B, N, Z = 3, 23, 4
    coords = torch.randn((N, 2), generator=g) if shared_grid else torch.randn((B, N, 2), generator=g)
    c = torch.randn((N, 2), generator=g) if shared_dir else torch.randn((B, N, 2), generator=g)
    p, a, w = torch.randn((B, Z, 2), generator=g), torch.randn((B, Z, 8), generator=g), torch.ones(B, Z, 1)
    whole, chunked = _StubNef(), _StubNef()
    o0, t0 = decode_directional(whole, None, coords, p, a, w, c)
    o1, t1 = decode_directional(chunked, None, coords, p, a, w, c, chunk=10)
    # the latent tangents pass through as None; the direction arrives as (B, N, dx), a stride-0 expansion when it is shared
    assert whole.calls == [(N, 0 if shared_grid else N * 2, True, True, True, ((B, N, 2), 0 if shared_dir else N * 2))]
    assert [k[0] for k in chunked.calls] == [10, 10, 3] and [k[5][0][1] for k in chunked.calls] == [10, 10, 3]
    assert all((k[1] == 0) == shared_grid and (k[5][1] == 0) == shared_dir and k[2:5] == (True, True, True) for k in chunked.calls)
    assert o1.shape == t1.shape == (B, N, 2) and torch.equal(o0, o1) and torch.equal(t0, t1)
    cd = c[None].expand(B, -1, -1) if shared_dir else c
    assert torch.equal(t1[..., 1], 2 * (cd[..., 0] + 10 * cd[..., 1]))   # each chunk got ITS slice of the direction
    with pytest.raises(ValueError):
        decode_directional(_StubNef(), None, coords, p, a, w, c[..., :1])
    with pytest.raises(ValueError):
        decode_directional(_StubNef(), None, coords, p, a, w, c[..., :N - 1, :])


@pytest.mark.parametrize("window", [None, 0.25])
def test_decode_material_derivative_evaluates_the_ode_once_without_autograd(window):
    from enf_pde_amd.fitting import decode_material_derivative
    g = torch.Generator().manual_seed(1)
    B, N, Z = 2, 17, 3
    coords, vel = torch.randn((N, 2), generator=g), torch.randn((B, N, 2), generator=g)
    p, a, w = torch.randn((B, Z, 2), generator=g), torch.randn((B, Z, 8), generator=g, requires_grad=True), torch.ones(B, Z, 1)
    nef, ode = _StubNef(), _StubOde(window)
    u, dudt = decode_material_derivative(nef, None, ode, 3.0, coords, p, a, w, vel, chunk=8)
    assert ode.seen == [False]                                            # once, under no_grad, however many chunks
    assert [k[0] for k in nef.calls] == [8, 8, 1] and [k[5][0][1] for k in nef.calls] == [8, 8, 1]
    assert all(k[2:5] == (False, False, window is None) for k in nef.calls)   # ONE pass carries both halves; a None entry stays None
    lin = 0.5 * p.sum(dim=(1, 2)) + 2 * 3.0 * a.detach().sum(dim=(1, 2)) + (0.0 if window is None else 3 * window * Z)
    want = lin[:, None] * coords[None, :, 0] + vel[..., 0] + 10 * vel[..., 1]
    assert u.shape == dudt.shape == (B, N, 2) and not dudt.requires_grad
    assert torch.allclose(dudt[..., 0], want, rtol=1e-5, atol=1e-5)
    u0, d0 = decode_material_derivative(_StubNef(), None, _StubOde(window), 3.0, coords, p, a, w, vel)
    assert torch.equal(u, u0) and torch.equal(dudt, d0)


def test_decode_tangent_keeps_its_three_keywords():
    from enf_pde_amd.fitting import decode_tangent, decode_tendency
    B, N, Z = 2, 9, 3
    coords, p, a, w = torch.ones(N, 2), torch.ones(B, Z, 2), torch.ones(B, Z, 8), torch.ones(B, Z, 1)
    nef = _ThreeKeywordNef()
    decode_tangent(nef, None, coords, p, a, w, p, a, None)
    decode_tangent(nef, None, coords, p, a, w, p, a, None, chunk=4)
    decode_tendency(nef, None, _StubOde(None), 1.0, coords, p, a, w)
    assert nef.calls == 1 + 3 + 1
