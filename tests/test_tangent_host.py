"""Tendency fields without a GPU (include/enf_hip.h, "Tendency fields"): the yardstick itself (the oracle's fp64 Jacobian-vector
product against central differences and against its own vector-Jacobian product), the header and the bindings, the size query, the
argument checks of enf_field_tangent (every call here fails its checks, so nothing is launched), the Python mirror's refusals, and
decode_tangent / decode_tendency against a stand-in model whose tangent is a known linear map."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from enf_pde_amd import _lib
from oracle import enf_ref_torch as T
from tests.helpers import make_cfg, build_nef
from tests.tangent_ref import INVARIANTS, case, rel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, EUNSUPPORTED = -1, -3


@pytest.mark.parametrize("inv", INVARIANTS)
def test_reference_jvp_against_central_differences_and_the_vjp(inv):
    """The reference every GPU test compares with.  Central differences in fp64 with h = 1e-6: truncation ~ h^2 = 1e-12 times the
    third directional derivative, rounding ~ 1e-16 / h = 1e-10 times the cancellation in out(z + h v) - out(z - h v), so 1e-7 relative
    leaves three orders for both and is three and a half below the tightest bound a GPU test applies (5e-4).  (The step is small because
    the chain has relu layers: a difference that straddles one kink of one pair is wrong by ~5e-5, as h = 1e-5 is for rel_pos_periodic.)
    The dot-product identity <w, J v> = <J^T w, v> is exact up to fp64 summation: 1e-12."""
    cfg, prm, (x, p, a, s), (dp, da, ds), out_ref, tan_ref = case(inv)
    tp = T.to_torch(prm, torch.float64)
    f = lambda P, A, S: T.nef_apply(tp, cfg, torch.tensor(x), P, A, S)
    h = 1e-6
    with torch.no_grad():
        hi = f(torch.tensor(p + h * dp), torch.tensor(a + h * da), torch.tensor(s + h * ds)).numpy()
        lo = f(torch.tensor(p - h * dp), torch.tensor(a - h * da), torch.tensor(s - h * ds)).numpy()
        mid = f(torch.tensor(p), torch.tensor(a), torch.tensor(s)).numpy()
    e_cd = rel((hi - lo) / (2 * h), tan_ref)
    assert np.array_equal(mid, out_ref) and tan_ref.shape == out_ref.shape == (3, 50, 2)
    w = np.random.default_rng(5).standard_normal(tan_ref.shape)
    P, A, S = (torch.tensor(v, requires_grad=True) for v in (p, a, s))
    (f(P, A, S) * torch.tensor(w)).sum().backward()
    rhs = float((P.grad.numpy() * dp).sum() + (A.grad.numpy() * da).sum() + (S.grad.numpy() * ds).sum())
    lhs = float((w * tan_ref).sum())
    e_id = abs(lhs - rhs) / abs(rhs)
    print(f"{inv}: central differences {e_cd:.2e}, dot-product identity {e_id:.2e}")
    assert np.linalg.norm(tan_ref) > 0 and e_cd < 1e-7 and e_id < 1e-12


def test_symbols_header_and_abi():
    with open(os.path.join(ROOT, "include", "enf_hip.h")) as f:
        h = f.read()
    assert re.search(r"#define\s+ENF_ABI_VERSION\s+2\b", h)
    lib = _lib.load()
    assert lib.enf_abi_version() == 2
    for name in ("enf_field_tangent_workspace_bytes", "enf_field_tangent"):
        assert re.search(rf"\b(int|size_t)\s+{name}\s*\(", h), name
        assert name in _lib.EXPORTS and hasattr(lib, name)
        assert getattr(lib, name).argtypes is not None, name
    assert len(lib.enf_field_tangent.argtypes) == 14
    assert lib.enf_field_tangent_workspace_bytes.restype is ctypes.c_size_t
    # what the header has to say: the definition, the NULL tangents, reproducibility by construction
    assert "tan[b,n,o] = sum_z" in h and "each may be NULL" in h
    assert "no atomics" in h and "bit-reproducible" in h


def test_workspace_size_and_argument_checks_without_a_launch():
    lib = _lib.load()
    dummy = ctypes.create_string_buffer(64)
    P = ctypes.cast(dummy, ctypes.c_void_p)
    mk = lambda inv=0, O=2, window=1, emb=0, D=128, H=2: _lib.make_desc(2, 70, 9, H, D, 16, O, 2 if inv < 7 else 3, inv, window, 0, embedding=emb)
    d = mk()
    size = lambda desc: lib.enf_field_tangent_workspace_bytes(ctypes.byref(desc))
    plain = lib.enf_workspace_bytes(ctypes.byref(d))
    # the plain workspace is what it was (lt, an, kv, ybar, lse, dybar, delta, tail_act, dlt at this shape: the latent-split kernels)
    al = lambda n: (n + 255) & ~255
    stride = (2 * 256 + 32 + 128 + 63) & ~63
    BZ, BN, HD, Dm = 18, 140, 256, 128
    want = (al(4 * BZ * stride) + al(4 * BZ * (2 * Dm + 2)) + al(4 * BZ * 2 * HD) + al(4 * BN * HD) + al(4 * BN * 2) + al(4 * BN * HD) +
            al(4 * BN * 2) + al(4 * BN * (2 * HD + 2 * Dm + 2)) + al(4 * BZ * stride))
    assert plain == want
    # its own buffer: the plain regions, then the table's tangent and d ybar
    assert size(d) == plain + al(4 * BZ * stride) + al(4 * BN * HD) > plain
    assert size(mk(O=33)) == 0                                           # a bad descriptor
    for bad in (mk(inv=7, D=64), mk(inv=8, D=64), mk(inv=9), mk(emb=1)):   # ball, ball_lat, ponita_full, ffn
        assert lib.enf_check_desc(ctypes.byref(bad)) == 0 and size(bad) == 0
    masked = mk()
    masked.relu_masks, masked.mask_mode, masked.mask_signals = P.value, _lib.MASK_MODE["read"], 2
    assert size(masked) == 0

    def call(desc=d, x=P, p=P, a=P, sigma=P, dp=P, da=P, ds=P, blob=P, out=P, tan=P, ws=P):
        return lib.enf_field_tangent(ctypes.byref(desc), x, 0, p, a, sigma, dp, da, ds, blob, out, tan, ws, None)
    for k in ("x", "p", "a", "sigma", "blob", "tan", "ws"):
        assert call(**{k: None}) == EINVAL, k
    assert call(dp=None, da=None, ds=None) == EINVAL                      # not all three
    for bad in (mk(inv=7, D=64), mk(inv=8, D=64), mk(inv=9), mk(emb=1), masked):
        assert call(desc=bad) == EUNSUPPORTED and call(desc=bad, tan=None) == EUNSUPPORTED
    assert call(desc=mk(O=33)) == EUNSUPPORTED and call(desc=mk(O=33), tan=None) == EUNSUPPORTED   # the descriptor's error comes first


def test_python_mirror_refuses_what_it_does_not_serve():
    from tests.test_gpu_layers import _nef as layered
    from tests.ffn_ref import build_nef_ffn
    B, N, Z = 2, 5, 3
    x, p, a, s = torch.zeros(B, N, 2), torch.zeros(B, Z, 2), torch.ones(B, Z, 8), torch.ones(B, Z, 1)
    nef = layered(dict(make_cfg("rel_pos_periodic", D=64, H=2, C=8, O=2), num_layers=1), "f32")
    with pytest.raises(NotImplementedError, match="num_layers"):
        nef.tangent(None, x, p, a, s, da=torch.zeros_like(a))
    with pytest.raises(NotImplementedError, match="ffn"):
        build_nef_ffn(make_cfg("rel_pos_periodic", D=64, H=2, C=8, O=2), "f32").tangent(None, x, p, a, s, da=torch.zeros_like(a))
    for inv in ("ball", "ball_lat"):
        with pytest.raises(NotImplementedError, match=inv):
            build_nef(make_cfg(inv, D=64, H=2, C=8, O=2), "f32").tangent(None, torch.zeros(B, N, 3), torch.zeros(B, Z, 4), a, s,
                                                                          da=torch.zeros_like(a))
    flat = build_nef(make_cfg("rel_pos_periodic", D=64, H=2, C=8, O=2), "f32")
    with pytest.raises(ValueError):
        flat.tangent(None, x, p, a, s)                                    # all three tangents None
    with pytest.raises(_lib.EnfError):                                    # host tensors: there is no CPU path
        flat.tangent(None, x, p, a, s, da=torch.zeros_like(a))


class _StubNef:
    """out[b, n, o] = (o + 1) |x_n|^2,  tan[b, n, o] = (o + 1) (sum dp_b + 2 sum da_b + 3 sum dw_b) x_n0: linear in the tangents;
    records the slices and the tangents it was handed"""

    def __init__(self):
        self.calls = []

    def tangent(self, params, x, p, a, window, dp=None, da=None, dwindow=None):
        self.calls.append((x.shape[1], x.stride(0), dp is None, da is None, dwindow is None))
        ch = torch.tensor([1.0, 2.0])
        z = lambda t, k: 0.0 if t is None else k * t.sum(dim=(1, 2))
        lin = z(dp, 1.0) + z(da, 2.0) + z(dwindow, 3.0) + torch.zeros(x.shape[0])
        out = (x * x).sum(-1, keepdim=True) * ch
        return out, lin[:, None, None] * x[:, :, :1] * ch


class _StubOde:
    def __init__(self, window):
        self.window, self.seen = window, []

    def apply(self, params, latents):
        p, a, w = latents
        self.seen.append(torch.is_grad_enabled())
        return 0.5 * p, a * params, (None if self.window is None else torch.full_like(w, self.window))


@pytest.mark.parametrize("shared_grid", [True, False])
def test_decode_tangent_chunks_by_slicing_and_passes_none_through(shared_grid):
    from enf_pde_amd.fitting import decode_tangent
    g = torch.Generator().manual_seed(0)
    B, N, Z = 3, 23, 4
    coords = torch.randn((N, 2), generator=g) if shared_grid else torch.randn((B, N, 2), generator=g)
    p, a, w = torch.randn((B, Z, 2), generator=g), torch.randn((B, Z, 8), generator=g), torch.ones(B, Z, 1)
    dp, da = torch.randn((B, Z, 2), generator=g), torch.randn((B, Z, 8), generator=g)
    whole, chunked = _StubNef(), _StubNef()
    o0, t0 = decode_tangent(whole, None, coords, p, a, w, dp, da, None)
    o1, t1 = decode_tangent(chunked, None, coords, p, a, w, dp, da, None, chunk=10)
    assert whole.calls == [(N, 0 if shared_grid else N * 2, False, False, True)]
    assert [c[0] for c in chunked.calls] == [10, 10, 3]
    assert all((c[1] == 0) == shared_grid and c[2:] == (False, False, True) for c in chunked.calls)
    assert o1.shape == t1.shape == (B, N, 2) and torch.equal(o0, o1) and torch.equal(t0, t1)
    x = coords[None].expand(B, -1, -1) if shared_grid else coords
    want = (dp.sum(dim=(1, 2)) + 2 * da.sum(dim=(1, 2)))[:, None] * x[:, :, 0]
    assert torch.allclose(t1[..., 1], 2 * want)


@pytest.mark.parametrize("window", [None, 0.25])
def test_decode_tendency_evaluates_the_ode_once_without_autograd(window):
    from enf_pde_amd.fitting import decode_tendency
    g = torch.Generator().manual_seed(1)
    B, N, Z = 2, 17, 3
    coords = torch.randn((N, 2), generator=g)
    p, a, w = torch.randn((B, Z, 2), generator=g), torch.randn((B, Z, 8), generator=g, requires_grad=True), torch.ones(B, Z, 1)
    nef, ode = _StubNef(), _StubOde(window)
    u, ut = decode_tendency(nef, None, ode, 3.0, coords, p, a, w, chunk=8)
    assert ode.seen == [False]                                            # once, under no_grad, however many chunks
    assert [c[0] for c in nef.calls] == [8, 8, 1]
    assert all(c[2:] == (False, False, window is None) for c in nef.calls)   # a None entry stays None: zero
    lin = 0.5 * p.sum(dim=(1, 2)) + 2 * 3.0 * a.detach().sum(dim=(1, 2)) + (0.0 if window is None else 3 * window * Z)
    assert u.shape == ut.shape == (B, N, 2) and not ut.requires_grad
    assert torch.allclose(ut[..., 0], lin[:, None] * coords[None, :, 0], rtol=1e-5, atol=1e-6)
    u0, ut0 = decode_tendency(_StubNef(), None, _StubOde(window), 3.0, coords, p, a, w)
    assert torch.equal(u, u0) and torch.equal(ut, ut0)
