"""Second directional derivatives without a GPU (include/enf_hip.h, "Second directional derivatives"): the yardstick itself
(tests/second_ref.py: nested forward mode on the fp64 oracle, against a central difference of the oracle's first-order JVP, against a
reverse-over-reverse Hessian and against identities that hold exactly), that the error measure of tests/test_gpu_second.py rejects
plausible defects of a second-order kernel at its f32 and bf16 bounds, the header and the bindings, the argument checks of
enf_field_second_x (every call here fails its checks, so nothing is launched), the size queries, and the signatures of the decode_*
functions."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

from enf_pde_amd import _lib
from oracle import enf_ref_torch as T
from tests.second_ref import INVARIANTS, CASES_3D, case, oracle_second_x, oracle_hessian_x, rel
from tests.tangent_x_ref import oracle_jvp_x
from tests.test_gpu_second import BF16_ER, TOL2_F32

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, EUNSUPPORTED = -1, -3
ALL_CASES = [(inv, 2) for inv in INVARIANTS] + [(inv, 3) for inv in CASES_3D]


# ---- the reference
@pytest.mark.parametrize("inv,num_in", ALL_CASES)
def test_reference_against_a_central_difference_of_the_first_order_jvp(inv, num_in):
    """(JVP(x + h xdot) - JVP(x - h xdot)) / 2h of the oracle's first-order JVP along xdot, h = 1e-6: truncation ~1e-12, rounding ~1e-16 / h
    times the cancellation; a small step because of the relu kinks (at 1e-4 and 1e-5 the difference crosses kinks and is off by more than
    1).  Measured over the ten cases 1.8e-10 .. 3.4e-9; bound 1e-7.  out and tan are tests/tangent_x_ref.py's to fp64 rounding."""
    cfg, prm, (x, p, a, s), xd, out, tan, tan2 = case(inv, num_in=num_in)
    h = 1e-6
    hi = oracle_jvp_x(cfg, prm, x + h * xd, p, a, s, xd, None, None, None)[1]
    lo = oracle_jvp_x(cfg, prm, x - h * xd, p, a, s, xd, None, None, None)[1]
    e = rel((hi - lo) / (2 * h), tan2)
    o1, t1 = oracle_jvp_x(cfg, prm, x, p, a, s, xd, None, None, None)
    print(f"{inv} num_in={num_in}: central difference of the JVP {e:.2e}; |tan2| max {np.abs(tan2).max():.3g}; out {rel(out, o1):.1e}, "
          f"tan {rel(tan, t1):.1e} against the first-order reference")
    assert tan2.shape == tan.shape == out.shape == (3, 50, 2) and x.shape[-1] == num_in
    assert np.linalg.norm(tan2) > 0 and e < 1e-7 and rel(out, o1) < 1e-14 and rel(tan, t1) < 1e-14


def test_reference_against_a_reverse_mode_hessian_and_exact_identities():
    """xdot^T H xdot from a reverse-over-reverse autograd Hessian on a small case (N = 6): bound 1e-10.  Then what holds exactly or to
    fp64 rounding: tan2(2 xdot) = 4 tan2(xdot) (a power of two: 0 difference), the polarisation identity
    H_ij = (D2(e_i + e_j) - D2 e_i - D2 e_j) / 2, and trace(hess) = the sum of the unit passes."""
    cfg, prm, (x, p, a, s), xd, out, tan, tan2 = case("rel_pos_periodic", B=2, N=6, Z=5)
    H = oracle_hessian_x(cfg, prm, x, p, a, s)
    e = rel(np.einsum("bni,bnoij,bnj->bno", xd, H, xd), tan2)
    print(f"reverse-over-reverse Hessian contracted with xdot: {e:.2e}")
    assert H.shape == (2, 6, 2, 2, 2) and e < 1e-10 and rel(H, np.swapaxes(H, -1, -2)) < 1e-12
    assert np.array_equal(oracle_second_x(cfg, prm, x, p, a, s, 2 * xd)[2], 4 * tan2)
    unit = lambda *ax: np.broadcast_to(np.isin(np.arange(2), ax).astype(np.float64), x.shape).copy()
    d0, d1, d01 = (oracle_second_x(cfg, prm, x, p, a, s, unit(*ax))[2] for ax in ((0,), (1,), (0, 1)))
    assert rel((d01 - d0 - d1) / 2, H[..., 0, 1]) < 1e-12
    assert rel(d0 + d1, np.trace(H, axis1=-2, axis2=-1)) < 1e-12


# ---- the metric rejects plausible defects
class _TorchWith:
    """the torch module as oracle/enf_ref_torch.py sees it, with another softmax"""

    def __init__(self, softmax):
        self.softmax = softmax

    def __getattr__(self, name):
        return getattr(torch, name)


def _defective(monkeypatch, c, kind):
    """tan2 of the oracle with one term of the second-order rules dropped, by linearising a function at the primal point (its first
    derivative stays, its second is zero): "gelu": every gelu -> no g'' da^2 term anywhere; "softmax_denominator": exp in the softmax's
    DENOMINATOR only -> R = sum e d2l without dl^2, U keeps it."""
    cfg, prm, (x, p, a, s), xd = c[:4]
    tp = T.to_torch(prm, torch.float64)
    seen, gelu, softmax = [], T.gelu, torch.softmax

    def record_gelu(z):
        zr = z.detach().clone().requires_grad_(True)
        g = gelu(zr)
        seen.append((z.detach(), g.detach(), torch.autograd.grad(g.sum(), zr)[0]))
        return gelu(z)

    def record_softmax(l, dim):
        seen.append(l.detach())
        return softmax(l, dim=dim)
    if kind == "gelu":
        monkeypatch.setattr(T, "gelu", record_gelu)
    else:
        monkeypatch.setattr(T, "torch", _TorchWith(record_softmax))
    T.nef_apply(tp, cfg, *(torch.tensor(v) for v in (x, p, a, s)))          # pass 1: the primal points, in call order
    points = iter(seen)

    def linear_gelu(z):
        z0, g0, gp = next(points)
        return g0 + gp * (z - z0)

    def softmax_linear_denominator(l, dim):
        l0 = next(points)
        m = l0.max(dim=dim, keepdim=True).values
        return torch.exp(l - m) / (torch.exp(l0 - m) * (1.0 + l - l0)).sum(dim=dim, keepdim=True)
    if kind == "gelu":
        monkeypatch.setattr(T, "gelu", linear_gelu)
    else:
        monkeypatch.setattr(T, "torch", _TorchWith(softmax_linear_denominator))
    out, tan, tan2 = oracle_second_x(cfg, prm, x, p, a, s, xd)
    assert rel(out, c[4]) < 1e-12 and rel(tan, c[5]) < 1e-12                 # value and first derivative are untouched
    return tan2


@pytest.mark.parametrize("kind", ["softmax_denominator", "gelu", "first_order"])
def test_the_metric_rejects_plausible_defects(monkeypatch, kind):
    """A dropped dl^2 term in R, a dropped g'' da^2 term, a tan2 that is the first-order value: each must miss the f32 bound (5e-4) and
    the bf16 bound of its class (twice the class's measured E_r) by the relative Frobenius norm the GPU tests use."""
    c = case("rel_pos_periodic")
    tan2 = c[5] if kind == "first_order" else _defective(monkeypatch, c, kind)
    e, bf16_bound = rel(tan2, c[6]), 2 * BF16_ER["rel_pos_periodic"]
    print(f"defect '{kind}': relative error of tan2 {e:.3e} (f32 bound {TOL2_F32:.1e}, bf16 bound {bf16_bound:.2e})")
    assert e > TOL2_F32 and e > bf16_bound


# ---- header, bindings, argument checks, sizes
def test_symbols_header_and_abi():
    with open(os.path.join(ROOT, "include", "enf_hip.h")) as f:
        h = f.read()
    assert re.search(r"#define\s+ENF_ABI_VERSION\s+2\b", h)
    lib = _lib.load()
    assert lib.enf_abi_version() == 2
    assert re.search(r"\bint\s+enf_field_second_x\s*\(", h) and re.search(r"\bsize_t\s+enf_field_second_workspace_bytes\s*\(", h)
    for name in ("enf_field_second_workspace_bytes", "enf_field_second_x"):
        assert name in _lib.EXPORTS and hasattr(lib, name)
    assert lib.enf_field_second_workspace_bytes.restype is ctypes.c_size_t and len(lib.enf_field_second_workspace_bytes.argtypes) == 1
    at = lib.enf_field_second_x.argtypes
    assert len(at) == 14 and at[2] is ctypes.c_int64 and at[4] is ctypes.c_int64 and at[3] is ctypes.c_void_p
    assert len(lib.enf_field_tangent_x.argtypes) == 16 and len(lib.enf_field_tangent.argtypes) == 14      # the existing calls keep theirs
    decl = re.search(r"int\s+enf_field_second_x\s*\((.*?)\);", h, re.S).group(1)
    assert len(re.sub(r"/\*.*?\*/", "", decl, flags=re.S).split(",")) == 14
    # what the header has to say: the definition, the convention on the sphere, that xdot is only read, the workspace's layout
    assert "d^2 out[b,n,o] / d x[b,n,i] d x[b,n,j]" in h
    assert "no metric factors -- a sum of second angle" in h and "never\n * written" in h and "followed by d2 ybar" in h


def _mk(inv=0, O=2, window=1, emb=0, D=128, H=2, prec=0):
    return _lib.make_desc(2, 70, 9, H, D, 16, O, 2 if inv < 7 else 3, inv, window, prec, embedding=emb)


def _unserved():
    dummy = ctypes.create_string_buffer(64)
    masked = _mk()
    masked.relu_masks, masked.mask_mode, masked.mask_signals = ctypes.cast(dummy, ctypes.c_void_p).value, _lib.MASK_MODE["read"], 2
    return (_mk(inv=7, D=64), _mk(inv=8, D=64), _mk(inv=9), _mk(emb=1), masked), dummy     # ball, ball_lat, ponita_full, ffn, masks


def test_argument_checks_without_a_launch():
    lib = _lib.load()
    dummy = ctypes.create_string_buffer(64)
    P = ctypes.cast(dummy, ctypes.c_void_p)
    d = _mk()

    def call(desc=d, x=P, xdot=P, p=P, a=P, sigma=P, blob=P, out=P, tan=P, tan2=P, ws=P):
        return lib.enf_field_second_x(ctypes.byref(desc), x, 0, xdot, 0, p, a, sigma, blob, out, tan, tan2, ws, None)
    for k in ("x", "xdot", "p", "a", "sigma", "blob", "tan2", "ws"):
        assert call(**{k: None}) == EINVAL, k
        assert call(**{k: None}, out=None, tan=None) == EINVAL, k
    unserved, keep = _unserved()
    for bad in unserved:                                                  # ENF_EUNSUPPORTED comes before a NULL pointer
        assert lib.enf_check_desc(ctypes.byref(bad)) == 0
        assert call(desc=bad) == EUNSUPPORTED and call(desc=bad, tan2=None) == EUNSUPPORTED and call(desc=bad, xdot=None) == EUNSUPPORTED
    bad = _mk(O=33)                                                       # the descriptor's error comes first
    assert lib.enf_check_desc(ctypes.byref(bad)) != 0
    assert call(desc=bad) == call(desc=bad, tan2=None) == lib.enf_check_desc(ctypes.byref(bad))


def test_size_queries():
    lib = _lib.load()
    second = lambda desc: lib.enf_field_second_workspace_bytes(ctypes.byref(desc))
    tangent = lambda desc: lib.enf_field_tangent_workspace_bytes(ctypes.byref(desc))
    for D, H in ((128, 2), (64, 2), (128, 1), (64, 1), (64, 4)):
        for prec in (0, 1):
            d = _mk(D=D, H=H, prec=prec)
            # the tangent workspace's regions at their offsets, then d2 ybar: (B, N, H D) floats, 256-aligned
            assert second(d) >= tangent(d) + 4 * 2 * 70 * H * D > tangent(d) > 0, (D, H, prec)
            assert second(d) - tangent(d) < 4 * 2 * 70 * H * D + 256
    unserved, keep = _unserved()
    for bad in unserved + (_mk(O=33),):
        assert second(bad) == 0


def test_python_mirror_refusals_and_xdot_checks():
    from tests.helpers import make_cfg, build_nef
    from tests.ffn_ref import build_nef_ffn
    B, N, Z = 2, 5, 3
    x, p, a, s = torch.zeros(B, N, 2), torch.zeros(B, Z, 2), torch.ones(B, Z, 8), torch.ones(B, Z, 1)
    xd = torch.zeros(B, N, 2)
    with pytest.raises(NotImplementedError, match="ffn"):
        build_nef_ffn(make_cfg("rel_pos_periodic", D=64, H=2, C=8, O=2), "f32").second_derivative(None, x, p, a, s, xd)
    with pytest.raises(NotImplementedError, match="ball"):
        build_nef(make_cfg("ball", D=64, H=2, C=8, O=2), "f32").second_derivative(None, torch.zeros(B, N, 3), torch.zeros(B, Z, 4), a, s,
                                                                                 torch.zeros(B, N, 3))
    flat = build_nef(make_cfg("rel_pos_periodic", D=64, H=2, C=8, O=2), "f32")
    with pytest.raises(ValueError, match="xdot"):
        flat.second_derivative(None, x, p, a, s, None)
    for wrong in (torch.zeros(B, N, 3), torch.zeros(B, N + 1, 2), torch.zeros(N, 2)):
        with pytest.raises(AssertionError, match="xdot"):
            flat.second_derivative(None, x, p, a, s, wrong)
    with pytest.raises(ValueError, match="xdot"):
        flat.second_derivative(None, x, p, a, s, xd.double())
    with pytest.raises(_lib.EnfError):                                    # well-formed: what stops the call is that there is no CPU path
        flat.second_derivative(None, x, p, a, s, xd[:1].expand(B, -1, -1))


# ---- the decode_* functions
def test_signatures():
    from enf_pde_amd import fitting
    from enf_pde_amd.enf.models import EquivariantCrossAttentionNeF as NeF
    sig = lambda f: list(inspect.signature(f).parameters)
    base = ["nef", "nef_params", "coords", "p", "a", "window"]
    assert sig(fitting.decode_second_directional) == base + ["direction", "chunk"]
    assert sig(fitting.decode_laplacian) == base + ["chunk"] and sig(fitting.decode_hessian) == base + ["chunk"]
    assert sig(fitting.decode_diffusion_residual) == ["nef", "nef_params", "ode_model", "ode_params", "coords", "p", "a", "window",
                                                      "diffusivity", "chunk"]
    for f in (fitting.decode_second_directional, fitting.decode_laplacian, fitting.decode_hessian, fitting.decode_diffusion_residual):
        assert inspect.signature(f).parameters["chunk"].default is None and f.__name__ in fitting.__all__
    assert sig(NeF.second_derivative) == ["self", "params", "x", "p", "a", "gaussian_window_size", "xdot", "return_out", "return_first"]
    # the existing ones are unchanged
    assert sig(fitting.decode_tangent) == base + ["dp", "da", "dwindow", "chunk"]
    assert sig(fitting.decode_directional) == base + ["direction", "chunk"]
    assert sig(NeF.tangent) == ["self", "params", "x", "p", "a", "gaussian_window_size", "dp", "da", "dwindow", "return_out", "xdot"]


class _StubNef:
    """out = |x|^2 (o + 1), tan = 2 x . xdot (o + 1), tan2 = 2 |xdot|^2 (o + 1) + 6 x_0 xdot_0 xdot_1: a field whose Hessian is
    [[2 (o + 1), 3 x_0], [3 x_0, 2 (o + 1)]] + ... with a known mixed term; records the slices it was handed"""

    def __init__(self, name="rel_pos"):
        from types import SimpleNamespace as NS
        self.cross_attn_invariant, self.calls = NS(name=name), []

    def second_derivative(self, params, x, p, a, window, xdot, return_out=True, return_first=True):
        self.calls.append((x.shape[1], x.stride(0), tuple(xdot.shape), xdot.stride(0), return_out))
        ch = torch.tensor([1.0, 2.0])
        out = (x * x).sum(-1, keepdim=True) * ch
        tan = 2 * (x * xdot).sum(-1, keepdim=True) * ch
        tan2 = 2 * (xdot * xdot).sum(-1, keepdim=True) * ch + 6 * (x[..., :1] * xdot[..., :1] * xdot[..., 1:2])
        return (out if return_out else None), (tan if return_first else None), tan2


@pytest.mark.parametrize("shared_grid", [True, False])
def test_decode_functions_on_a_field_with_a_known_hessian(shared_grid):
    from enf_pde_amd.fitting import decode_second_directional, decode_laplacian, decode_hessian
    g = torch.Generator().manual_seed(0)
    B, N, Z = 3, 23, 4
    coords = torch.randn((N, 2), generator=g) if shared_grid else torch.randn((B, N, 2), generator=g)
    c = torch.randn((B, N, 2), generator=g)
    p, a, w = torch.randn((B, Z, 2), generator=g), torch.randn((B, Z, 8), generator=g), torch.ones(B, Z, 1)
    xs = coords[None].expand(B, -1, -1) if shared_grid else coords
    whole, chunked = _StubNef(), _StubNef()
    r0 = decode_second_directional(whole, None, coords, p, a, w, c)
    r1 = decode_second_directional(chunked, None, coords, p, a, w, c, chunk=10)
    assert whole.calls == [(N, 0 if shared_grid else 2 * N, (B, N, 2), 2 * N, True)] and [k[0] for k in chunked.calls] == [10, 10, 3]
    assert all(torch.equal(u, v) for u, v in zip(r0, r1)) and r0[2].shape == (B, N, 2)
    nef = _StubNef()
    u, grad, hess = decode_hessian(nef, None, coords, p, a, w, chunk=10)
    assert [k[4] for k in nef.calls] == [True] * 3 + [False] * 6 and len(nef.calls) == 9      # e_0 (with the decode), e_1, e_0 + e_1
    ch = torch.tensor([1.0, 2.0])
    assert torch.equal(u, (xs * xs).sum(-1, keepdim=True) * ch) and torch.equal(grad, 2 * xs[:, :, None, :] * ch[:, None])
    assert hess.shape == (B, N, 2, 2, 2) and torch.equal(hess, hess.transpose(-1, -2))
    assert torch.allclose(hess[..., 0, 0], (2 * ch).expand(B, N, 2)) and torch.allclose(hess[..., 0, 1], 3 * xs[..., :1].expand(B, N, 2), atol=1e-5)
    u2, grad2, lap = decode_laplacian(_StubNef(), None, coords, p, a, w)
    assert torch.equal(u2, u) and torch.equal(grad2, grad) and torch.equal(lap, hess[..., 0, 0] + hess[..., 1, 1])
    for name in ("latitude_periodic", "polar_periodic"):
        with pytest.raises(ValueError, match=name):
            decode_laplacian(_StubNef(name), None, coords, p, a, w)
        assert decode_hessian(_StubNef(name), None, coords, p, a, w)[2].shape == (B, N, 2, 2, 2)
    with pytest.raises(ValueError):
        decode_second_directional(_StubNef(), None, coords, p, a, w, c[..., :1])


def test_decode_diffusion_residual_composes_tendency_and_laplacian():
    from enf_pde_amd.fitting import decode_diffusion_residual
    B, N, Z = 2, 9, 3
    coords, p, a, w = torch.randn(N, 2), torch.ones(B, Z, 2), torch.ones(B, Z, 8), torch.ones(B, Z, 1)

    class Nef(_StubNef):
        def tangent(self, params, x, p, a, window, dp=None, da=None, dwindow=None):
            return x[..., :1] * torch.ones(2), x[..., 1:] * torch.tensor([1.0, -1.0]) * float(dp.sum())

    class Ode:
        def apply(self, params, latents):
            return latents[0] * params, None, None
    u, res = decode_diffusion_residual(Nef(), None, Ode(), 0.5, coords, p, a, w, 0.25, chunk=4)
    xs = coords[None].expand(B, -1, -1)
    lap = (4 * torch.tensor([1.0, 2.0])).expand(B, N, 2)
    ut = xs[..., 1:] * torch.tensor([1.0, -1.0]) * (0.5 * B * Z * 2)
    assert torch.equal(u, (xs * xs).sum(-1, keepdim=True) * torch.tensor([1.0, 2.0])) and torch.allclose(res, ut - 0.25 * lap)
