"""Per-channel loss weights without a GPU (include/enf_hip.h, "Weighted loss"; fitting/weights.py): the helpers, the C-ABI's new
entry points and their argument checks, and the inner loop's framework route with a stub model."""
import ctypes
import importlib
import os
import re
from types import SimpleNamespace as NS

import pytest
import torch

from enf_pde_amd import _lib
from enf_pde_amd.fitting.weights import (valid_channel_weights, prepare_channel_weights, normalize_channel_weights, point_support,
                                         observed_channel_sampling_weights, observed_sampling_weights, weighted_mse,
                                         gather_point_weights, valid_weights, prepare_point_weights)

IL = importlib.import_module("enf_pde_amd.fitting.inner_loop")      # (the package re-exports the function under the same name)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1
NEW_ENTRY_POINTS = ("enf_fit_step_cw", "enf_mse_value_grad_cw", "enf_fit_inputs_cw")


def _cw(g, B, N, O, zeros=0.3):
    cw = 2 * torch.rand((B, N, O), generator=g)
    cw[torch.rand((B, N, O), generator=g) < zeros] = 0
    return cw


def test_valid_channel_weights_is_per_value():
    f = torch.tensor([[[1.0, float("nan")], [float("inf"), 2.0], [3.0, 4.0], [float("nan"), float("-inf")]]])
    cw = valid_channel_weights(f)
    assert cw.shape == f.shape and cw.dtype == torch.float32
    assert cw.tolist() == [[[1, 0], [0, 1], [1, 1], [0, 0]]]
    assert torch.equal(valid_weights(f), cw.prod(-1))                   # the per-point mask drops what one missing value touches
    assert torch.equal(point_support(cw) > 0, torch.tensor([[True, True, True, False]]))


def test_normalisation_identities():
    g = torch.Generator().manual_seed(0)
    B, N, O = 3, 20, 3
    cw = _cw(g, B, N, O)
    cw[2] = 0                                                            # a signal that observes nothing
    cw[1, :, 0] = 0                                                      # a channel that is never observed
    n = prepare_channel_weights(cw, B, N, O)
    assert n.shape == (B, N, O) and n.dtype == torch.float32 and n.is_contiguous()
    assert torch.allclose(n[:2].mean(dim=(1, 2)), torch.ones(2), atol=1e-6)
    assert bool((n[2] == 0).all()) and bool((n[1, :, 0] == 0).all())
    assert torch.equal(n == 0, cw == 0)                                  # zeros stay exactly zero, nothing else becomes zero
    assert torch.allclose(n[0] * cw[0].mean(), cw[0], atol=1e-6)         # one factor per signal
    ones = torch.ones(B, N, O)
    assert torch.equal(prepare_channel_weights(ones, B, N, O), ones)     # all ones come back exactly
    assert torch.equal(normalize_channel_weights(ones), ones)
    assert torch.equal(prepare_channel_weights(cw, B, N, O, normalize=False), cw)
    shared = prepare_channel_weights(cw[0], B, N, O)                     # (N, O) is broadcast over the signals
    assert shared.shape == (B, N, O) and torch.equal(shared[0], shared[2]) and torch.allclose(shared[0], n[0], atol=1e-6)
    assert prepare_channel_weights(None, B, N, O) is None
    # the per-point weight broadcast over the channels normalises like the per-point weight
    w = cw[..., 0] + 0.1
    assert torch.allclose(prepare_channel_weights(w[..., None].expand(B, N, O), B, N, O)[..., 1], prepare_point_weights(w, B, N), atol=1e-6)


@pytest.mark.parametrize("normalize", [True, False])
def test_bad_channel_weights_are_rejected(normalize):
    B, N, O = 2, 5, 3
    ok = torch.ones(B, N, O)
    for bad in (-1.0, float("nan"), float("inf")):
        w = ok.clone()
        w[1, 2, 0] = bad
        with pytest.raises(ValueError):
            prepare_channel_weights(w, B, N, O, normalize=normalize)
    for shape in ((B, N), (B, N, O + 1), (B, N + 1, O), (B + 1, N, O), (N,), (B, N, O, 1)):
        with pytest.raises(ValueError):
            prepare_channel_weights(torch.ones(shape), B, N, O, normalize=normalize)


def test_point_support_and_observed_sampling_weights():
    g = torch.Generator().manual_seed(1)
    B, N, O, Ns = 3, 40, 2, 16
    cw = _cw(g, B, N, O, zeros=0.5)
    cw[1, 10:] = 0                                                       # signal 1 observes 10 points at most: fewer than Ns
    cw[2] = 0
    sup = point_support(cw)
    assert sup.shape == (B, N) and torch.equal(sup > 0, (cw > 0).any(-1))
    got = observed_channel_sampling_weights(cw, Ns)
    nb = (sup > 0).sum(-1).float()
    c = nb / N * Ns / nb.clamp(min=1).clamp(max=Ns)
    assert torch.allclose(got, cw * c[:, None, None]) and bool((got[2] == 0).all())
    # the same factor as the per-point rule gives for the support, on every channel
    assert torch.allclose(got[..., 1], observed_sampling_weights(sup, Ns) / sup.clamp(min=1e-30) * cw[..., 1])
    masks = IL.make_signal_masks(sup, Ns, 1, generator=torch.Generator().manual_seed(3), device="cpu")
    assert masks.shape == (B, Ns, 2)
    for b in range(B):
        idx = masks[b][masks[b] >= 0]
        assert bool((sup[b][idx] > 0).all())                             # drawn from points that carry an observed value
    assert bool((masks[2] == -1).all())


def test_weighted_mse_with_channel_weights_and_nan_targets():
    g = torch.Generator().manual_seed(2)
    B, N, O = 2, 7, 3
    out = torch.randn((B, N, O), generator=g, dtype=torch.float64, requires_grad=True)
    tgt = torch.randn((B, N, O), generator=g, dtype=torch.float64)
    cw = _cw(g, B, N, O).double()
    cw[0, 2] = 0
    cw[1, :, 1] = 0
    bad = tgt.clone()
    bad[cw == 0] = float("nan")
    bad[0, 2, 1] = float("inf")
    loss = weighted_mse(out, bad, cw)
    ref = (cw * (out.detach() - tgt) ** 2).mean()
    assert bool(torch.isfinite(loss)) and torch.allclose(loss, ref, atol=1e-15)
    (grad,) = torch.autograd.grad(loss, out)
    assert bool(torch.isfinite(grad).all()) and bool((grad[cw == 0] == 0).all())
    assert torch.allclose(grad, 2 * cw * (out.detach() - tgt) / out.numel(), atol=1e-15)
    # the shapes accepted before keep their meaning
    w = cw[..., 0]
    assert torch.allclose(weighted_mse(out, tgt, w), weighted_mse(out, tgt, w[..., None].expand(B, N, O)), atol=1e-15)
    assert torch.equal(weighted_mse(out, tgt, None), ((out - tgt) ** 2).mean())
    with pytest.raises(ValueError):
        weighted_mse(out, tgt, cw[..., :2])


def test_header_declares_and_lib_binds():
    with open(os.path.join(ROOT, "include", "enf_hip.h")) as f:
        h = f.read()
    assert re.search(r"#define\s+ENF_ABI_VERSION\s+2\b", h)
    assert ctypes.sizeof(_lib.EnfDesc) == 80
    lib = _lib.load()
    assert lib.enf_abi_version() == 2
    for name in NEW_ENTRY_POINTS:
        assert re.search(rf"\b{name}\s*\(", h), name
        assert name in _lib.EXPORTS
        assert getattr(lib, name).argtypes is not None, name
    assert len(lib.enf_fit_step_cw.argtypes) == len(lib.enf_fit_step_w.argtypes) == 18
    assert len(lib.enf_mse_value_grad_cw.argtypes) == 11
    assert len(lib.enf_fit_inputs_cw.argtypes) == 19
    assert "cweight[b,n,o]" in h and "(B, N, O)" in h and "per VALUE" in h


def test_argument_checks_without_a_launch():
    lib = _lib.load()
    dummy = ctypes.create_string_buffer(64)
    P = ctypes.cast(dummy, ctypes.c_void_p)
    d = _lib.make_desc(2, 70, 9, 2, 128, 16, 3, 2, 0, 1, 0)
    plain = lib.enf_workspace_bytes(ctypes.byref(d))

    def fit(flags, ptr, cweight, nbytes=plain):
        return lib.enf_fit_step_cw(ctypes.byref(d), ptr, 0, ptr, ptr, ptr, ptr, ptr, 1.0, ptr, ptr, ptr, ptr, ptr, nbytes, cweight, flags, None)
    assert fit(0, P, None) == EINVAL                            # a caller without channel weights uses the existing calls
    assert fit(16, P, None) == EINVAL
    assert fit(0, None, P) == EINVAL
    assert fit(1, P, P) == EINVAL and fit(16 | 64, P, P) == EINVAL      # unknown flag bits
    assert fit(16, P, P) == -4                                  # the deterministic call needs enf_workspace_bytes_ex, as enf_fit_step_w
    assert fit(0, P, P, nbytes=plain - 1) == -4
    bad = _lib.make_desc(2, 70, 9, 2, 128, 16, 33, 2, 0, 1, 0)  # O > 32: the descriptor's error comes first
    assert lib.enf_fit_step_cw(ctypes.byref(bad), P, 0, P, P, P, P, P, 1.0, P, P, P, P, P, plain, P, 0, None) == -3

    def mse(n, flags, cweight=P, scratch=P, nbytes=1 << 20, out=P):
        return lib.enf_mse_value_grad_cw(out, P, cweight, n, 1.0, P, P, scratch, nbytes, flags, None)
    assert mse(12, 0, cweight=None) == EINVAL
    assert mse(0, 0) == EINVAL
    assert mse(12, 1) == EINVAL and mse(12, 16 | 32) == EINVAL
    assert mse(12, 16, scratch=None) == EINVAL
    assert mse(12, 16, nbytes=0) == -4
    assert mse(12, 0, out=None) == EINVAL

    comps = (_lib.EnfFitComponent * _lib.ENF_SGD_MAX_SEGMENTS)()
    comps[0] = _lib.EnfFitComponent(P.value, P.value, 2, 0)

    def inputs(cweight, ws, ncomp=1, xs=P, O=3, layout=0):
        return lib.enf_fit_inputs_cw(ncomp, comps, 3, 4, 50, 17, 4, 2, O, P, P, P, xs, P, P, cweight, ws, layout, None)
    for layout in (0, 1):
        assert inputs(None, P, layout=layout) == EINVAL and inputs(P, None, layout=layout) == EINVAL
        assert inputs(None, None, layout=layout) == EINVAL
        assert inputs(P, P, ncomp=0, layout=layout) == EINVAL and inputs(P, P, xs=None, layout=layout) == EINVAL
        assert inputs(P, P, O=0, layout=layout) == -6


class _Stop(Exception):
    pass


class _Nef:
    cross_attn_invariant = NS(num_z_ori_dims=0)

    def __init__(self):
        self.seen = []

    def mse_value_and_latent_grads(self, params, x, p, a, window, target, grad_scale=1.0, loss_out=None, weight=None, channel_weight=None):
        self.seen.append((x, target, weight, channel_weight))
        return loss_out, torch.zeros_like(p), torch.zeros_like(a), torch.zeros_like(window)

    def apply(self, *a):
        raise _Stop             # (the final loss is a library call on device memory)


def _fit_problem():
    g = torch.Generator().manual_seed(2)
    B, N, O, Ns, S, Z = 2, 30, 3, 11, 2, 3
    img = torch.randn((B, N, O), generator=g)
    cw = _cw(g, B, N, O)
    img[cw == 0] = float("nan")
    coords = torch.randn((N, 2), generator=g)
    lat0 = {"p_pos": torch.zeros(1, Z, 2), "a": torch.ones(1, Z, 4), "gaussian_window": torch.ones(1, Z, 1)}
    return g, B, N, O, Ns, S, img, cw, coords, lat0


def test_inner_loop_hands_every_step_its_gathered_channel_weights(monkeypatch):
    """The framework route (CPU tensors never take enf_fit_inputs_cw), shared masks: step s gets cw[:, masks[:, s]], (B, Ns, O),
    next to targets whose NaN passed through the gather untouched, and no per-point weight."""
    g, B, N, O, Ns, S, img, cw, coords, lat0 = _fit_problem()
    masks = torch.stack([torch.randperm(N, generator=g)[:Ns] for _ in range(S + 1)], 1)
    assert torch.equal(gather_point_weights(cw, masks), cw[:, masks.t()].transpose(0, 1))
    monkeypatch.setattr(IL, "meta_sgd_update", lambda lat, grads, lrs, scale: lat)
    nef = _Nef()
    with pytest.raises(_Stop):
        IL.inner_loop(nef, None, lat0, None, coords, img, masks, channel_weights=cw)
    assert len(nef.seen) == S
    for s, (x, target, weight, cwt) in enumerate(nef.seen):
        assert weight is None and cwt.shape == (B, Ns, O)
        assert torch.equal(cwt, cw[:, masks[:, s]])
        assert torch.equal(x, coords[masks[:, s]][None].expand(B, -1, -1))
        assert torch.equal(torch.isnan(target), cwt == 0)
        assert torch.equal(torch.nan_to_num(target), torch.nan_to_num(img[:, masks[:, s]]))
    # normalize_weights: mean 1 over every signal's Ns * O sampled values
    nef = _Nef()
    with pytest.raises(_Stop):
        IL.inner_loop(nef, None, lat0, None, coords, img, masks, channel_weights=cw, normalize_weights=True)
    for s, (_, _, _, cwt) in enumerate(nef.seen):
        raw = cw[:, masks[:, s]]
        assert torch.allclose(cwt.mean(dim=(1, 2)), torch.ones(B), atol=1e-6)
        assert torch.allclose(cwt, raw / raw.mean(dim=(1, 2), keepdim=True), atol=1e-6)
    # None takes the path it took before
    nef = _Nef()
    with pytest.raises(_Stop):
        IL.inner_loop(nef, None, lat0, None, coords, torch.nan_to_num(img), masks)
    assert all(w is None and c is None for _, _, w, c in nef.seen)


def test_inner_loop_with_per_signal_masks_and_padding(monkeypatch):
    g, B, N, O, Ns, S, img, cw, coords, lat0 = _fit_problem()
    cw[1, 6:] = 0                                                        # signal 1 observes at most 6 points: padded with -1
    masks = IL.make_signal_masks(point_support(cw), Ns, S, generator=g, device="cpu")
    assert bool((masks[1] == -1).any()) and not bool((masks[0] == -1).any())
    monkeypatch.setattr(IL, "meta_sgd_update", lambda lat, grads, lrs, scale: lat)
    nef = _Nef()
    with pytest.raises(_Stop):
        IL.inner_loop(nef, None, lat0, None, coords, img, masks, channel_weights=cw)
    assert len(nef.seen) == S
    for s, (x, target, weight, cwt) in enumerate(nef.seen):
        assert weight is None and cwt.shape == (B, Ns, O) and x.shape == (B, Ns, 2)
        for b in range(B):
            m = masks[b, :, s]
            ok = m >= 0
            assert torch.equal(cwt[b][ok], cw[b][m[ok]]) and bool((cwt[b][~ok] == 0).all())
            assert torch.equal(x[b][ok], coords[m[ok]]) and bool((x[b][~ok] == coords[0]).all())
            assert bool((target[b][~ok] == 0).all())
            assert torch.equal(torch.nan_to_num(target[b][ok]), torch.nan_to_num(img[b][m[ok]]))


def test_inner_loop_rejects_wrong_shapes_and_both_kinds_of_weights():
    g, B, N, O, Ns, S, img, cw, coords, lat0 = _fit_problem()
    masks = torch.stack([torch.randperm(N, generator=g)[:Ns] for _ in range(S + 1)], 1)
    for bad in (cw[..., 0], cw[..., :2], cw[:, :-1], cw[:1], cw[..., None]):
        with pytest.raises(ValueError):
            IL.inner_loop(_Nef(), None, lat0, None, coords, img, masks, channel_weights=bad)
    with pytest.raises(ValueError):
        IL.inner_loop(_Nef(), None, lat0, None, coords, img, masks, weights=cw[..., 0], channel_weights=cw)


# ---- the auto-decoder trainer on the host, with a differentiable two-channel stand-in for the decoder (which has no CPU path)
def _two_channel_trainer():
    from tests.test_table_adam_host import _ToyNef, _val_trainer

    class Toy2(_ToyNef):
        def _out(self, x, p, a, window):
            one = super()._out(x, p, a, window)
            return torch.cat((one, 0.3 - 0.5 * one), -1)

        def mse_value_and_latent_grads(self, params, x, p, a, window, target, grad_scale=1.0, loss_out=None, weight=None,
                                       channel_weight=None):
            assert weight is None or channel_weight is None
            self.seen.append(("fit", x.detach().clone(), x.stride(0), channel_weight))
            with torch.enable_grad():
                leaves = [t.detach().clone().requires_grad_(True) for t in (p, a, window)]
                loss = weighted_mse(self._out(x, *leaves), target, weight if channel_weight is None else channel_weight)
                g = torch.autograd.grad(loss, leaves)
            return loss.detach().reshape(1), g[0], g[1], g[2]

    tr, st, _, _, val_ad = _val_trainer(train_until=3)
    tr.nef = Toy2(16, tr.nef.cross_attn_invariant)
    g = torch.Generator().manual_seed(9)

    def traj(n):
        f = torch.randn(n, 12, 64, 2, generator=g)
        f[..., 1] = torch.where(torch.rand(n, 12, 64, generator=g) < 0.5, torch.full_like(f[..., 1], float("nan")), f[..., 1])
        return f.reshape(n, 12, 8, 8, 2)
    train = [(traj(3), None, torch.tensor(i)) for i in ([4, 0, 5], [1, 2, 3])]
    val = [(traj(2), torch.tensor(i)) for i in ([0, 1], [3, 2])]
    return tr, st, train, val, val_ad


def _filled(loader, value):
    return [(torch.nan_to_num(b[0], nan=value),) + tuple(b[1:]) for b in loader]


@pytest.mark.parametrize("step", ["nef_train_step_autodec_only", "fit_latents_step"])
def test_autodecoder_steps_take_channel_weights(step):
    """a two-channel field whose second channel is NaN on half the points: the loss is finite, the table moves, and the step equals
    the same step with the NaN replaced by a number; together with weights= it is a ValueError"""
    tr, st, train, _, _ = _two_channel_trainer()
    results = []
    for fill in (None, 0.0, -3e4):
        frames, idx = train[0][0][:, 0], train[0][-1]
        cw = valid_channel_weights(frames.reshape(3, 64, 2))
        assert 0.7 < float(cw.mean()) < 0.8
        batch = frames if fill is None else torch.nan_to_num(frames, nan=fill)
        st.rng.manual_seed(11)
        loss, new = getattr(tr, step)(st, (batch, idx), channel_weights=cw)
        P0, P1 = st.params["autodecoder"]["params"], new.params["autodecoder"]["params"]
        assert bool(torch.isfinite(loss)) and float(loss) > 0 and all(bool(torch.isfinite(v).all()) for v in P1.values())
        assert not torch.equal(P1["a"][idx], P0["a"][idx])
        results.append((loss, P1))
    for loss, P in results[1:]:
        assert torch.allclose(loss, results[0][0], rtol=1e-6)
        assert all(torch.equal(P[k], results[0][1][k]) for k in P)
    if step == "fit_latents_step":
        fits = [s for s in tr.nef.seen if s[0] == "fit"]
        assert len(fits) == 3 and all(s[3] is not None and s[3].shape == (3, 24, 2) for s in fits)      # 64 -> 24 sampled points
    with pytest.raises(ValueError):
        getattr(tr, step)(st, (frames, idx), weights=cw[..., 0], channel_weights=cw)


def test_validate_epoch_with_channel_weights_on_the_host():
    tr, st, train, val, val_ad = _two_channel_trainer()
    cw_of = lambda batch: valid_channel_weights(batch[0].flatten(2, 3))                  # (B, T, N, O)
    runs = []
    for loaders in ((train, val), (_filled(train, 7.0), _filled(val, 7.0))):
        st.rng.manual_seed(12)
        weights = {id(b[0]): cw_of(s) for ld, src in zip(loaders, (train, val)) for b, s in zip(ld, src)}
        metrics, last = tr.validate_epoch(st, loaders[0], loaders[1], val_ad, drop_rates=(0.0, 0.5), channel_weights=lambda b: weights[id(b[0])])
        assert all(type(v) is float and torch.isfinite(torch.tensor(v)) for v in metrics.values()), metrics
        assert {"val_mse_in_t", "val_mse_out_t_dp0.5", "train_mse_in_t_sc"} <= set(metrics)
        runs.append((metrics, last.params["autodecoder"]["params"]))
    for k, v in runs[0][0].items():
        assert abs(v - runs[1][0][k]) <= 1e-6 * abs(v), k                                   # the NaN were never used
    assert all(torch.equal(v, runs[1][1][k]) for k, v in runs[0][1].items())
    plain, _ = tr.validate_epoch(st, _filled(train, 7.0), _filled(val, 7.0), val_ad, drop_rates=(0.0,), fit_train=False)
    assert plain["val_mse_in_t"] != runs[0][0]["val_mse_in_t"]                              # without weights the fill value counts
