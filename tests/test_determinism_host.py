"""Deterministic mode, host side (no GPU): the header declares the flags and entry points and _lib binds them, the size
queries, the argument checks of the new entry points (nothing is launched), the unchanged ABI, and how the model resolves
its ``deterministic`` setting."""
import ctypes
import os
import re
from types import SimpleNamespace as NS

import pytest
import torch

from enf_pde_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRY_POINTS = ["enf_workspace_bytes_ex", "enf_fit_step_ex", "enf_mse_value_grad_ex", "enf_mse_scratch_bytes",
                    "enf_pair_backward_ex2", "enf_pair_backward_scratch_bytes", "enf_backward_all_scratch_bytes_ex",
                    "enf_backward_weights_ex", "enf_backward_weights_scratch_bytes_ex"]
DET, QGRAD = 16, 32


def _header():
    with open(os.path.join(ROOT, "include", "enf_hip.h")) as f:
        return f.read()


def _desc(B, N, Z, D=128, H=2, inv=0, dx=2, prec=1, variants=(0, 0)):
    return _lib.make_desc(B, N, Z, H, D, 16, 1, dx, inv, 1, prec, variants=variants)


def test_header_declares_and_lib_binds():
    h = _header()
    for name, value in (("ENF_BWD_DETERMINISTIC", "16u"), ("ENF_FIT_DETERMINISTIC", "16u"), ("ENF_MSE_DETERMINISTIC", "16u"),
                        ("ENF_BWD_QUERY_GRAD", "32u")):
        assert re.search(rf"#define\s+{name}\s+{value}\b", h), name
    assert re.search(r"#define\s+ENF_ABI_VERSION\s+2\b", h)
    lib = _lib.load()
    for name in NEW_ENTRY_POINTS:
        assert re.search(rf"\b{name}\s*\(", h), name
        assert name in _lib.EXPORTS
        assert getattr(lib, name).argtypes is not None, name
    assert _lib.ENF_BWD_DETERMINISTIC == _lib.ENF_FIT_DETERMINISTIC == _lib.ENF_MSE_DETERMINISTIC == DET
    assert _lib.ENF_BWD_QUERY_GRAD == QGRAD
    # the sentence about enf_backward_all no longer carries the caveat as the only truth
    assert "up to the float atomics of d lt" not in h


def test_abi_is_unchanged():
    assert _lib.load().enf_abi_version() == 2
    assert ctypes.sizeof(_lib.EnfDesc) == 80


@pytest.mark.parametrize("B,N,Z,variants,grows", [
    (1, 200, 5, (0, 0), True),        # 13 query tiles on one workgroup of latents: the backward splits the queries 8 ways
    (1, 200, 5, (0, 2), True),        # the same with the z-fold backward forced
    (64, 256, 16, (0, 0), True),      # the fit shape of the bench: nsplit = 1, one more gradient table and the loss partials
    (3, 50, 9, (0, 0), True)])
def test_workspace_bytes_ex(B, N, Z, variants, grows):
    lib = _lib.load()
    d = _desc(B, N, Z, variants=variants)
    plain = lib.enf_workspace_bytes(ctypes.byref(d))
    assert plain > 0
    assert lib.enf_workspace_bytes_ex(ctypes.byref(d), 0) == plain
    det = lib.enf_workspace_bytes_ex(ctypes.byref(d), DET)
    assert det >= plain and (det > plain) == grows
    assert lib.enf_workspace_bytes_ex(ctypes.byref(d), DET | QGRAD) == det
    assert lib.enf_workspace_bytes_ex(ctypes.byref(d), DET | 64) == 0          # unknown bit
    assert lib.enf_workspace_bytes_ex(ctypes.byref(d), 1) == 0
    # the partial rows: nsplit x B Z rows of the latent table's stride (13 tiles over < 256 workgroups: 8 splits; 64 x 16
    # latents fill the chip: 1)
    stride = ctypes.c_int(0)
    assert lib.enf_lt_layout(ctypes.byref(d), ctypes.byref(stride), None, None, None, None, None) == 0
    nsplit = 8 if B == 1 else (1 if B == 64 else 4)
    if B != 3:
        assert det - plain >= nsplit * B * Z * stride.value * 4
        assert det - plain < nsplit * B * Z * stride.value * 4 + 4096 + 4 * ((B * N + 127) // 128) * 8


def test_scratch_size_queries():
    lib = _lib.load()
    d = _desc(2, 100, 8)
    assert lib.enf_pair_backward_scratch_bytes(ctypes.byref(d), 0) == 0
    a = lib.enf_pair_backward_scratch_bytes(ctypes.byref(d), DET)
    b = lib.enf_pair_backward_scratch_bytes(ctypes.byref(d), DET | QGRAD)
    assert 0 < a < b and b - a >= 2 * 8 * 100 * 2 * 4
    assert lib.enf_pair_backward_scratch_bytes(ctypes.byref(d), DET | 1) == 0
    for q, q_ex in ((lib.enf_backward_all_scratch_bytes, lib.enf_backward_all_scratch_bytes_ex),
                    (lib.enf_backward_weights_scratch_bytes, lib.enf_backward_weights_scratch_bytes_ex)):
        plain = q(ctypes.byref(d), 2)
        assert plain > 0 and q_ex(ctypes.byref(d), 2, 0) == plain
        assert plain < q_ex(ctypes.byref(d), 2, DET) < q_ex(ctypes.byref(d), 2, DET | QGRAD)
        assert q_ex(ctypes.byref(d), 2, 4) == 0 and q_ex(ctypes.byref(d), 3, DET) == 0
    assert lib.enf_mse_scratch_bytes(1000, 0) == 0
    assert lib.enf_mse_scratch_bytes(1000, DET) >= 4 * 4
    assert lib.enf_mse_scratch_bytes(10 ** 7, DET) >= 4 * 1024
    assert lib.enf_mse_scratch_bytes(1000, 2) == 0


def _zeros(fn, **over):
    out = []
    for t in fn.argtypes[1:]:
        if t in (ctypes.c_float, ctypes.c_double):
            out.append(0.0)
        elif t in (ctypes.c_int, ctypes.c_int32, ctypes.c_int64, ctypes.c_uint, ctypes.c_size_t, ctypes.c_longlong):
            out.append(0)
        else:
            out.append(None)
    return out


def test_argument_checks_without_a_launch():
    """Unknown flag bits are ENF_EINVAL and a workspace / scratch shorter than the deterministic size query asks for is
    ENF_EWORKSPACE, decided from the arguments alone: the buffers are NULL or (where a NULL pointer would be reported first)
    dummy host addresses that are never dereferenced."""
    lib = _lib.load()
    d = _desc(1, 200, 5)
    EINVAL, EWORKSPACE = -1, -4
    dummy = ctypes.create_string_buffer(64)
    P = ctypes.cast(dummy, ctypes.c_void_p)
    plain = lib.enf_workspace_bytes(ctypes.byref(d))

    # enf_fit_step_ex(d, x, xs, p, a, sigma, packed, target, gscale, loss, dp, da, dsigma, ws, ws_bytes, flags, stream)
    def fit(ws_bytes, flags, ptr):
        return lib.enf_fit_step_ex(ctypes.byref(d), ptr, 0, ptr, ptr, ptr, ptr, ptr, 1.0, ptr, ptr, ptr, ptr, ptr, ws_bytes, flags, None)
    assert fit(0, DET, None) == EINVAL                       # NULL buffers, as enf_fit_step
    assert fit(plain, DET | 1, P) == EINVAL                  # unknown bit
    assert fit(plain, 64, None) == EINVAL
    assert fit(plain, DET, P) == EWORKSPACE                  # the plain size is too small for the deterministic form
    assert fit(plain - 1, 0, P) == EWORKSPACE

    # enf_backward_latents_ex(d, x, xs, p, a, sigma, packed, ybar, lse, dout, dp, da, dsigma, ws, ws_bytes, flags, stream)
    def bwd(ws_bytes, flags, ptr):
        return lib.enf_backward_latents_ex(ctypes.byref(d), ptr, 0, ptr, ptr, ptr, ptr, ptr, ptr, ptr, ptr, ptr, ptr, ptr, ws_bytes, flags, None)
    assert bwd(plain, DET | 64, P) == EINVAL
    assert bwd(plain, DET, P) == EWORKSPACE
    assert bwd(plain, DET, None) == EINVAL

    # enf_pair_backward_ex2(d, x, xs, lt, packed, lse, dybar, delta, dlt, store, dx, scratch, scratch_bytes, flags, stream)
    def pair(scratch, n, flags, dx):
        return lib.enf_pair_backward_ex2(ctypes.byref(d), P, 0, P, P, P, P, P, P, None, dx, scratch, n, flags, None)
    need = lib.enf_pair_backward_scratch_bytes(ctypes.byref(d), DET)
    assert pair(P, need, DET | 2, None) == EINVAL
    assert pair(None, need, DET, None) == EINVAL
    assert pair(P, need - 1, DET, None) == EWORKSPACE
    assert pair(P, need, DET, P) == EWORKSPACE               # with dx the query-gradient shares are needed too

    # enf_mse_value_grad_ex(out, target, n, gscale, dout, loss, scratch, scratch_bytes, flags, stream)
    assert lib.enf_mse_value_grad_ex(P, P, 1000, 1.0, None, P, P, 64, DET | 1, None) == EINVAL
    assert lib.enf_mse_value_grad_ex(P, P, 1000, 1.0, None, P, None, 0, DET, None) == EINVAL
    assert lib.enf_mse_value_grad_ex(P, P, 1000, 1.0, None, P, P, 8, DET, None) == EWORKSPACE
    assert lib.enf_mse_value_grad_ex(None, None, 0, 1.0, None, None, None, 0, 0, None) == EINVAL

    # enf_backward_all: unknown bits with everything else NULL
    z = _zeros(lib.enf_backward_all)
    z[-2] = 64
    assert lib.enf_backward_all(ctypes.byref(d), *z) == EINVAL
    z = _zeros(lib.enf_backward_weights_ex)
    z[-2] = DET | 64
    assert lib.enf_backward_weights_ex(ctypes.byref(d), *z) == EINVAL


def _nef(deterministic="unset", precision="bf16"):
    from enf_pde_amd.enf.models import EquivariantCrossAttentionNeF
    from enf_pde_amd.enf.steerable_attention.invariant import get_ca_invariant
    inv = get_ca_invariant(NS(invariant_type="rel_pos_periodic", num_in=2))
    kw = {} if deterministic == "unset" else {"deterministic": deterministic}
    return EquivariantCrossAttentionNeF(num_hidden=64, num_heads=2, num_layers=0, num_out=1, latent_dim=8, cross_attn_invariant=inv,
                                        precision=precision, **kw)


def test_model_resolves_the_setting():
    prev = torch.are_deterministic_algorithms_enabled()
    prev_warn = torch.is_deterministic_algorithms_warn_only_enabled()
    try:
        for glob in (False, True):
            torch.use_deterministic_algorithms(glob)
            assert _nef().is_deterministic() is glob                     # the default is None: torch's switch at call time
            assert _nef(None).is_deterministic() is glob
            assert _nef(True).is_deterministic() is True
            assert _nef(False).is_deterministic() is False
            assert _nef(None)._det_flag() == (DET if glob else 0)
        m = _nef(None)
        torch.use_deterministic_algorithms(False)
        assert not m.is_deterministic()
        torch.use_deterministic_algorithms(True)
        assert m.is_deterministic()                                      # resolved per call, not at construction
    finally:
        torch.use_deterministic_algorithms(prev, warn_only=prev_warn)
    with pytest.raises(ValueError):
        _nef("yes")


def test_with_precision_keeps_the_setting():
    for det in (True, False, None):
        m = _nef(det, "bf16").with_precision("f32")
        assert m.deterministic is det and m.precision == "f32"


def test_get_model_pde_reads_the_config_key():
    from enf_pde_amd.fitting.model import get_model_pde
    base = dict(num_hidden=64, num_heads=2, num_layers=0, num_out=1, latent_dim=8, num_latents=16, invariant_type="rel_pos_periodic",
                num_in=2, embedding_type="rff", embedding_freq_multiplier_invariant=0.05, embedding_freq_multiplier_value=0.1,
                condition_value_transform=True, use_gaussian_window=True)
    nef, _ = get_model_pde(NS(nef=NS(**base)))
    assert nef.deterministic is None
    nef, _ = get_model_pde(NS(nef=NS(deterministic=True, **base)))
    assert nef.deterministic is True
