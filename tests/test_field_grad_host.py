"""Derivative fields without a GPU (include/enf_hip.h, "Derivative fields"): the header, the bindings, the argument checks of
enf_field_grad / enf_query_vjp (every call here fails its checks, so nothing is launched), the size query, the operators of
fitting/derivatives.py on a hand-made Jacobian, decode_jacobian's chunking against a stub model, and the Python mirror's refusals."""
import ctypes
import os
import re

import pytest
import torch

from enf_pde_amd import _lib
from tests.helpers import make_cfg, build_nef

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, EUNSUPPORTED, EWORKSPACE = -1, -3, -4
DET = _lib.ENF_BWD_DETERMINISTIC


def test_symbols_header_and_abi():
    with open(os.path.join(ROOT, "include", "enf_hip.h")) as f:
        h = f.read()
    assert re.search(r"#define\s+ENF_ABI_VERSION\s+2\b", h)
    assert ctypes.sizeof(_lib.EnfDesc) == 80
    lib = _lib.load()
    assert lib.enf_abi_version() == 2
    for name in ("enf_field_grad_workspace_bytes", "enf_field_grad", "enf_query_vjp"):
        assert re.search(rf"\b(int|size_t)\s+{name}\s*\(", h), name
        assert name in _lib.EXPORTS and hasattr(lib, name)
        assert getattr(lib, name).argtypes is not None, name
    assert len(lib.enf_field_grad.argtypes) == 13 and len(lib.enf_query_vjp.argtypes) == 14
    assert lib.enf_field_grad_workspace_bytes.restype is ctypes.c_size_t
    # what the documentation has to say: the layout, the coordinates, the atomics
    assert "jac[o,b,n,i] = d out[b,n,o] / d x[b,n,i]" in h and "(O, B, N, dx)" in h
    assert "no metric factors" in h and "float atomics" in h


def test_argument_checks_without_a_launch():
    lib = _lib.load()
    dummy = ctypes.create_string_buffer(64)
    P = ctypes.cast(dummy, ctypes.c_void_p)
    d = _lib.make_desc(2, 70, 9, 2, 128, 16, 3, 2, 0, 1, 0)
    bad = _lib.make_desc(2, 70, 9, 2, 128, 16, 33, 2, 0, 1, 0)          # O > 32
    masked = _lib.make_desc(2, 70, 9, 2, 128, 16, 3, 2, 0, 1, 0)
    masked.relu_masks, masked.mask_mode, masked.mask_signals = P.value, _lib.MASK_MODE["read"], 2
    size = lambda desc, flags: lib.enf_field_grad_workspace_bytes(ctypes.byref(desc), flags)
    plain, det = size(d, 0), size(d, DET)
    # one buffer for everything: the plain workspace; deterministic = the deterministic workspace + the query-gradient shares
    assert plain == lib.enf_workspace_bytes(ctypes.byref(d)) > 0
    assert det >= lib.enf_workspace_bytes_ex(ctypes.byref(d), DET) + 4 * 2 * 9 * 70 * 2 > plain
    assert size(bad, 0) == 0 and size(bad, DET) == 0
    assert size(d, 1) == 0 and size(d, DET | 32) == 0                    # ENF_BWD_QUERY_GRAD is not a flag of this call
    assert size(masked, 0) == 0

    def jac(x=P, p=P, a=P, sigma=P, packed=P, out=P, jac=P, ws=P, nbytes=plain, flags=0, desc=d):
        return lib.enf_field_grad(ctypes.byref(desc), x, 0, p, a, sigma, packed, out, jac, ws, nbytes, flags, None)

    def vjp(x=P, p=P, a=P, sigma=P, packed=P, dout=P, out=P, dx=P, ws=P, nbytes=plain, flags=0, desc=d):
        return lib.enf_query_vjp(ctypes.byref(desc), x, 0, p, a, sigma, packed, dout, out, dx, ws, nbytes, flags, None)
    for call, dst in ((jac, "jac"), (vjp, "dx")):
        for k in ("x", "p", "a", "sigma", "packed", "ws", dst):
            assert call(**{k: None}) == EINVAL, (call.__name__, k)
        for flags in (1, 2, 8, 32, DET | 64):
            assert call(flags=flags) == EINVAL, flags                    # only ENF_BWD_DETERMINISTIC is known
        assert call(nbytes=plain - 1) == EWORKSPACE
        assert call(flags=DET) == EWORKSPACE and call(flags=DET, nbytes=det - 1) == EWORKSPACE
        assert call(desc=masked) == EUNSUPPORTED and call(desc=masked, **{dst: None}) == EUNSUPPORTED
        # the descriptor's error comes first, ENF_EINVAL before ENF_EWORKSPACE
        assert call(desc=bad) == EUNSUPPORTED and call(desc=bad, **{dst: None}) == EUNSUPPORTED
        assert call(nbytes=0, **{dst: None}) == EINVAL
    assert vjp(dout=None) == EINVAL
    assert jac(out=None, nbytes=plain - 1) == EWORKSPACE                 # out == NULL passes the argument checks
    assert vjp(out=None, nbytes=plain - 1) == EWORKSPACE
    nowin = _lib.make_desc(2, 70, 9, 2, 128, 16, 3, 2, 0, 0, 0)
    assert jac(desc=nowin, sigma=None, nbytes=0) == EWORKSPACE           # no window: sigma is not needed


def test_operators_on_a_hand_made_jacobian():
    from enf_pde_amd.fitting import divergence, curl_2d, gradient_norm
    # u = (x^2 y, x + 3 y) at (x, y): jac = [[2 x y, x^2], [1, 3]]
    pts = torch.tensor([[1.0, 2.0], [-0.5, 4.0], [3.0, -1.0]])
    x, y = pts[:, 0], pts[:, 1]
    jac = torch.stack([torch.stack([2 * x * y, x * x], -1), torch.stack([torch.ones(3), torch.full((3,), 3.0)], -1)], -2)[None]   # (1, 3, 2, 2)
    assert torch.allclose(divergence(jac), (2 * x * y + 3)[None])
    assert torch.allclose(curl_2d(jac), (1 - x * x)[None])
    want = torch.stack([(4 * x * x * y * y + x ** 4).sqrt(), torch.full((3,), 10.0 ** 0.5)], -1)[None]
    assert torch.allclose(gradient_norm(jac), want)
    assert divergence(jac).shape == (1, 3) and curl_2d(jac).shape == (1, 3) and gradient_norm(jac).shape == (1, 3, 2)
    j3 = torch.arange(18.0).reshape(2, 3, 3)                              # three channels on three coordinates
    assert divergence(j3).tolist() == [0 + 4 + 8, 9 + 13 + 17]
    with pytest.raises(ValueError):
        divergence(torch.zeros(4, 2, 3))
    with pytest.raises(ValueError):
        curl_2d(j3)
    for fn in (divergence, curl_2d, gradient_norm):
        assert "artesian" in fn.__doc__.lower() or "CARTESIAN" in fn.__doc__, fn.__name__


class _Stub:
    """u_o(x) = (o + 1) * sum_i x_i^2 * (b + 1): jacobian known in closed form; records the slices it was handed"""

    def __init__(self):
        self.calls = []

    def jacobian(self, params, x, p, a, window):
        self.calls.append((x.shape[1], x.stride(0)))
        B, N, dx = x.shape
        scale = torch.arange(1, B + 1, dtype=x.dtype)[:, None, None]
        ch = torch.tensor([1.0, 2.0])
        out = (x * x).sum(-1, keepdim=True) * ch * scale
        jac = 2 * x[:, :, None, :] * ch[None, None, :, None] * scale[..., None]
        return out, jac


@pytest.mark.parametrize("shared_grid", [True, False])
def test_decode_jacobian_chunks_by_slicing(shared_grid):
    from enf_pde_amd.fitting import decode_jacobian
    g = torch.Generator().manual_seed(0)
    B, N = 3, 23
    coords = torch.randn((N, 2), generator=g) if shared_grid else torch.randn((B, N, 2), generator=g)
    p = torch.zeros(B, 4, 2)
    whole, chunked = _Stub(), _Stub()
    o0, j0 = decode_jacobian(whole, None, coords, p, None, None)
    o1, j1 = decode_jacobian(chunked, None, coords, p, None, None, chunk=10)
    assert whole.calls == [(N, 0 if shared_grid else N * 2)]
    assert [n for n, _ in chunked.calls] == [10, 10, 3]
    assert all((s == 0) == shared_grid for _, s in chunked.calls)        # a shared grid stays a stride-0 batch in every chunk
    assert o1.shape == (B, N, 2) and j1.shape == (B, N, 2, 2)
    assert torch.equal(o0, o1) and torch.equal(j0, j1)
    x = coords[None].expand(B, -1, -1) if shared_grid else coords
    assert torch.allclose(j1[2, :, 1, :], 2 * x[2] * 2.0 * 3.0)


def test_python_mirror_refuses_what_it_does_not_serve():
    from tests.test_gpu_layers import _nef as layered
    cfg = dict(make_cfg("rel_pos_periodic", D=64, H=2, C=8, O=2), num_layers=1)
    nef = layered(cfg, "f32")
    B, N, Z = 2, 5, 3
    x, p, a, s = torch.zeros(B, N, 2), torch.zeros(B, Z, 2), torch.ones(B, Z, 8), torch.ones(B, Z, 1)
    with pytest.raises(NotImplementedError):
        nef.jacobian(None, x, p, a, s)
    with pytest.raises(NotImplementedError):
        nef.query_vjp(None, x, p, a, s, torch.zeros(B, N, 2))
    flat = build_nef(make_cfg("rel_pos_periodic", D=64, H=2, C=8, O=2), "f32")
    with pytest.raises(_lib.EnfError):                                    # host tensors: there is no CPU path
        flat.jacobian(None, x, p, a, s)
    with pytest.raises(_lib.EnfError):
        flat.query_vjp(None, x, p, a, s, torch.zeros(B, N, 2))
