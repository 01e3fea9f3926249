"""Per-point loss weights, host side (no GPU): fitting/weights.py, the C-ABI contract of the three weighted entry points
(nothing is launched) and the inner loop's framework route for gathering the weights."""
import ctypes
import importlib
import math
import os
import re
from types import SimpleNamespace as NS

import pytest
import torch

from enf_pde_amd import _lib
from enf_pde_amd.fitting.weights import (normalize_point_weights, quadrature_weights, valid_weights, gather_point_weights,
                                         prepare_point_weights, weighted_mse)

IL = importlib.import_module("enf_pde_amd.fitting.inner_loop")      # (the package's attribute of that name is the function)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRY_POINTS = ["enf_fit_step_w", "enf_mse_value_grad_w", "enf_fit_inputs_w"]
EINVAL = -1


def test_normalize_point_weights():
    g = torch.Generator().manual_seed(0)
    w = torch.rand((3, 50), generator=g, dtype=torch.float64) * 2
    w[w < 0.5] = 0
    w[2] = 0                                               # an all-zero signal
    n = normalize_point_weights(w)
    assert torch.allclose(n[:2].mean(-1), torch.ones(2, dtype=torch.float64), atol=1e-14)
    assert torch.equal(n == 0, w == 0)                      # zeros stay zero, nothing else becomes zero
    assert torch.equal(n[2], torch.zeros(50, dtype=torch.float64))
    assert torch.allclose(n[0] * w[0].mean(), w[0], atol=1e-14)   # a rescaling, nothing else
    for dt in (torch.float32, torch.float64):
        ones = torch.ones((2, 777), dtype=dt)
        assert torch.equal(normalize_point_weights(ones), ones)
    with pytest.raises(ValueError):
        normalize_point_weights(torch.tensor([[1.0, -1.0]]))
    with pytest.raises(ValueError):
        normalize_point_weights(torch.tensor([[1.0, float("nan")]]))
    assert prepare_point_weights(None, 2, 5) is None
    assert torch.equal(prepare_point_weights(torch.ones(5), 2, 5), torch.ones(2, 5))
    with pytest.raises(ValueError):
        prepare_point_weights(torch.ones(2, 4), 2, 5)


@pytest.mark.parametrize("n_lat", [16, 48])
def test_quadrature_weights_on_an_equiangular_grid(n_lat):
    """Cell-centred latitudes lat_i = -pi/2 + (i + 1/2) h, h = pi / n_lat, n_lon longitudes.  The normalised weighted mean of
    f(lat) is sum_i cos(lat_i) f(lat_i) / sum_i cos(lat_i): the midpoint rule for int f cos / int cos (= int f cos / 2).
    Midpoint rule on [a, b]: |error| <= (b - a) h^2 / 24 * max |g''|.  For g = sin^2 cos, g'' = 2 cos - 9 sin^2 cos = 9 c^3 - 7 c
    with c = cos(lat) in [0, 1]: its extrema are 2 (c = 1) and -2.38 (c^2 = 7 / 27), so |g''| <= 2.4 and
    |sum_i h g(lat_i) - 2/3| <= pi h^2 / 10; for g = cos, |g''| <= 1: |sum_i h cos(lat_i) - 2| <= pi h^2 / 24.
    With num = 2/3 + e1 and den = 2 + e2, |num / den - 1/3| <= (|e1| + |e2| / 3) / (2 - |e2|)
    <= (pi h^2 / 10 + pi h^2 / 72) / (2 - pi h^2 / 24)."""
    n_lon = 8
    h = math.pi / n_lat
    lat = -math.pi / 2 + (torch.arange(n_lat, dtype=torch.float64) + 0.5) * h
    lon = torch.arange(n_lon, dtype=torch.float64) * (2 * math.pi / n_lon)
    coords = torch.stack(torch.meshgrid(lon, lat, indexing="ij"), -1).reshape(-1, 2)       # (N, 2): (lon, lat)
    w = quadrature_weights(coords, 1, "latitude")
    assert w.shape == (n_lon * n_lat,) and bool((w > 0).all())
    wn = normalize_point_weights(w[None])[0]
    const = torch.full_like(wn, 3.25)
    assert abs(float((wn * const).mean()) - 3.25) < 1e-13
    got = float((wn * torch.sin(coords[:, 1]) ** 2).mean())
    bound = (math.pi * h * h / 10 + math.pi * h * h / 72) / (2 - math.pi * h * h / 24)
    assert abs(got - 1.0 / 3) <= bound, (got, bound)
    assert abs(float(torch.sin(coords[:, 1]).pow(2).mean()) - 1.0 / 3) > bound       # the unweighted mean (1/2) is not it
    # the two conventions agree under lat = pi/2 - colat
    colat = coords.clone()
    colat[:, 1] = math.pi / 2 - coords[:, 1]
    assert torch.allclose(quadrature_weights(colat, 1, "colatitude"), w, atol=1e-15)
    # ball: r^2 sin(colat)
    ball = torch.cat([colat, torch.linspace(0.1, 1.0, colat.shape[0], dtype=torch.float64)[:, None]], -1)
    assert torch.allclose(quadrature_weights(ball, 1, "ball", radius_column=2), w * ball[:, 2] ** 2, atol=1e-15)
    with pytest.raises(ValueError):
        quadrature_weights(coords, 1, "latitude_periodic")           # an invariant's name is not a convention
    with pytest.raises(ValueError):
        quadrature_weights(ball, 1, "ball")


def test_valid_weights():
    f = torch.zeros((2, 5, 3))
    f[0, 1, 2] = float("nan")
    f[1, 0, 0] = float("inf")
    f[1, 4, 1] = -float("inf")
    w = valid_weights(f)
    assert w.dtype == torch.float32 and w.shape == (2, 5)
    expect = torch.ones((2, 5))
    expect[0, 1] = expect[1, 0] = expect[1, 4] = 0
    assert torch.equal(w, expect)


def test_weighted_mse_ignores_what_a_zero_weight_covers():
    g = torch.Generator().manual_seed(1)
    out = torch.randn((2, 7, 3), generator=g, dtype=torch.float64, requires_grad=True)
    tgt = torch.randn((2, 7, 3), generator=g, dtype=torch.float64)
    w = torch.rand((2, 7), generator=g, dtype=torch.float64)
    w[0, 2] = w[1, 5] = 0
    ref = (w[..., None] * (out - tgt) ** 2).sum() / out.numel()
    bad = tgt.clone()
    bad[0, 2] = float("nan")
    bad[1, 5, 1] = float("inf")
    loss = weighted_mse(out, bad, w)
    assert torch.allclose(loss, ref, atol=1e-15)
    (grad,) = torch.autograd.grad(loss, out)
    assert bool(torch.isfinite(grad).all()) and bool((grad[0, 2] == 0).all()) and bool((grad[1, 5] == 0).all())
    assert torch.allclose(grad, 2 * w[..., None] * torch.nan_to_num(out.detach() - bad, posinf=0, neginf=0) / out.numel(), atol=1e-15)
    assert torch.equal(weighted_mse(out, tgt, None), ((out - tgt) ** 2).mean())
    assert torch.allclose(weighted_mse(out, tgt, torch.ones_like(w)), ((out - tgt) ** 2).mean(), atol=1e-15)


def test_header_declares_and_lib_binds():
    with open(os.path.join(ROOT, "include", "enf_hip.h")) as f:
        h = f.read()
    assert re.search(r"#define\s+ENF_ABI_VERSION\s+2\b", h)
    lib = _lib.load()
    assert lib.enf_abi_version() == 2
    for name in NEW_ENTRY_POINTS:
        assert re.search(rf"\b{name}\s*\(", h), name
        assert name in _lib.EXPORTS
        assert getattr(lib, name).argtypes is not None, name
    assert "weight == 0 does not exist" in h


def test_argument_checks_without_a_launch():
    lib = _lib.load()
    dummy = ctypes.create_string_buffer(64)
    P = ctypes.cast(dummy, ctypes.c_void_p)
    d = _lib.make_desc(2, 70, 9, 2, 128, 16, 3, 2, 0, 1, 0)
    plain = lib.enf_workspace_bytes(ctypes.byref(d))

    def fit(flags, ptr, weight):
        return lib.enf_fit_step_w(ctypes.byref(d), ptr, 0, ptr, ptr, ptr, ptr, ptr, 1.0, ptr, ptr, ptr, ptr, ptr, plain, weight, flags, None)
    for weight in (None, P):
        assert fit(0, None, weight) == EINVAL                   # NULL buffers, as enf_fit_step
        assert fit(1, P, weight) == EINVAL                      # unknown flag bits
        assert fit(16 | 64, P, weight) == EINVAL
    assert fit(16, P, P) == -4                                  # the deterministic call's workspace size holds with a weight

    def mse(n, O, flags, weight=P, scratch=P, nbytes=1 << 20):
        return lib.enf_mse_value_grad_w(P, P, weight, n, O, 1.0, P, P, scratch, nbytes, flags, None)
    assert mse(10, 3, 0) == EINVAL                              # n % O != 0
    assert mse(10, 3, 0, weight=None) == EINVAL
    assert mse(12, 0, 0) == EINVAL
    assert mse(0, 3, 0) == EINVAL
    assert mse(12, 3, 1) == EINVAL and mse(12, 3, 16 | 32) == EINVAL      # unknown flag bits
    assert mse(12, 3, 16, scratch=None) == EINVAL
    assert mse(12, 3, 16, nbytes=0) == -4
    assert lib.enf_mse_value_grad_w(None, P, P, 12, 3, 1.0, P, P, None, 0, 0, None) == EINVAL

    comps = (_lib.EnfFitComponent * _lib.ENF_SGD_MAX_SEGMENTS)()
    comps[0] = _lib.EnfFitComponent(P.value, P.value, 2, 0)

    def inputs(weight, ws, ncomp=1, xs=P):
        return lib.enf_fit_inputs_w(ncomp, comps, 3, 4, 50, 17, 4, 2, 1, P, P, P, xs, P, P, weight, ws, None)
    assert inputs(P, None) == EINVAL and inputs(None, P) == EINVAL         # given together or not at all
    assert inputs(P, P, ncomp=0) == EINVAL and inputs(None, None, ncomp=0) == EINVAL
    assert inputs(P, P, xs=None) == EINVAL


class _Stop(Exception):
    pass


def test_framework_route_gathers_the_weights(monkeypatch):
    """The inner loop's route without enf_fit_inputs_w (CPU tensors never take it): every step is handed
    weights[:, masks[:, s]] next to targets whose NaN (under zero weights) passed through the gather untouched."""
    g = torch.Generator().manual_seed(2)
    B, N, Ns, S, Z = 2, 30, 11, 2, 3
    img = torch.randn((B, N, 2), generator=g)
    w = torch.rand((B, N), generator=g)
    w[torch.rand((B, N), generator=g) < 0.3] = 0
    img[w == 0] = float("nan")
    coords = torch.randn((N, 2), generator=g)
    masks = torch.stack([torch.randperm(N, generator=g)[:Ns] for _ in range(S + 1)], 1)
    assert torch.equal(gather_point_weights(w, masks), w[:, masks.t()].transpose(0, 1))
    lat0 = {"p_pos": torch.zeros(1, Z, 2), "a": torch.ones(1, Z, 4), "gaussian_window": torch.ones(1, Z, 1)}
    seen = []

    class Nef:
        cross_attn_invariant = NS(num_z_ori_dims=0)

        def mse_value_and_latent_grads(self, params, x, p, a, window, target, grad_scale=1.0, loss_out=None, weight=None):
            seen.append((x, target, weight))
            return loss_out, torch.zeros_like(p), torch.zeros_like(a), torch.zeros_like(window)

        def apply(self, *a):
            raise _Stop             # (the final loss is a library call on device memory)

    monkeypatch.setattr(IL, "meta_sgd_update", lambda lat, grads, lrs, scale: lat)
    with pytest.raises(_Stop):
        IL.inner_loop(Nef(), None, lat0, None, coords, img, masks, weights=w)
    assert len(seen) == S
    for s, (x, target, weight) in enumerate(seen):
        assert torch.equal(weight, w[:, masks[:, s]])
        assert torch.equal(x, coords[masks[:, s]][None].expand(B, -1, -1))
        assert torch.equal(torch.isnan(target).any(-1), weight == 0)
        assert torch.equal(torch.nan_to_num(target), torch.nan_to_num(img[:, masks[:, s]]))
    seen.clear()
    with pytest.raises(_Stop):
        IL.inner_loop(Nef(), None, lat0, None, coords, torch.nan_to_num(img), masks)
    assert all(weight is None for _, _, weight in seen)
    with pytest.raises(ValueError):
        IL.inner_loop(Nef(), None, lat0, None, coords, img, masks, weights=w[:, :-1])
