"""Per-signal and per-point errors without a GPU (include/enf_hip.h, "Per-signal and per-point errors"): the header, the bindings,
the argument checks of enf_fit_step_e / enf_eval_loss / enf_signal_sum (every call here fails its checks, so nothing is launched),
the new keywords of the Python mirror and its refusal of host tensors."""
import ctypes
import importlib
import inspect
import os
import re
from types import SimpleNamespace as NS

import pytest
import torch

from enf_pde_amd import _lib
from tests.helpers import make_cfg, build_nef

IL = importlib.import_module("enf_pde_amd.fitting.inner_loop")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, EUNSUPPORTED, EWORKSPACE = -1, -3, -4
NEW_ENTRY_POINTS = ("enf_fit_step_e", "enf_eval_loss")


def test_header_declares_and_lib_binds():
    with open(os.path.join(ROOT, "include", "enf_hip.h")) as f:
        h = f.read()
    assert re.search(r"#define\s+ENF_ABI_VERSION\s+2\b", h)
    assert ctypes.sizeof(_lib.EnfDesc) == 80
    lib = _lib.load()
    assert lib.enf_abi_version() == 2
    for name in NEW_ENTRY_POINTS + ("enf_signal_sum",):
        assert re.search(rf"\bint\s+{name}\s*\(", h), name
        assert name in _lib.EXPORTS
        assert getattr(lib, name).argtypes is not None, name
    assert len(lib.enf_fit_step_e.argtypes) == len(lib.enf_fit_step_w.argtypes) + 3 == 21
    assert len(lib.enf_eval_loss.argtypes) == 17
    assert "err[b,n]" in h and "loss_b[b]" in h and "OVERWRITTEN" in h


def test_argument_checks_without_a_launch():
    lib = _lib.load()
    dummy = ctypes.create_string_buffer(64)
    P = ctypes.cast(dummy, ctypes.c_void_p)
    d = _lib.make_desc(2, 70, 9, 2, 128, 16, 3, 2, 0, 1, 0)
    bad = _lib.make_desc(2, 70, 9, 2, 128, 16, 33, 2, 0, 1, 0)          # O > 32
    plain = lib.enf_workspace_bytes(ctypes.byref(d))
    det = lib.enf_workspace_bytes_ex(ctypes.byref(d), _lib.ENF_FIT_DETERMINISTIC)
    assert det > plain > 0                                               # additive: the sizes are those of enf_fit_step_w

    def fit(weight=None, cweight=None, err=P, loss_b=P, flags=0, nbytes=plain, x=P, desc=d):
        return lib.enf_fit_step_e(ctypes.byref(desc), x, 0, P, P, P, P, P, 1.0, P, P, P, P, P, nbytes, weight, cweight, err, loss_b, flags, None)
    assert fit(weight=P, cweight=P) == EINVAL                            # one kind of weight
    for w in ({}, {"weight": P}, {"cweight": P}):
        assert fit(err=None, **w) == EINVAL                              # err is required ...
        assert fit(err=None, loss_b=None, **w) == EINVAL
        assert fit(flags=1, **w) == EINVAL and fit(flags=16 | 64, **w) == EINVAL      # unknown flag bits
        assert fit(x=None, **w) == EINVAL
        assert fit(flags=16, **w) == EWORKSPACE                          # the deterministic call needs enf_workspace_bytes_ex
        assert fit(nbytes=plain - 1, **w) == EWORKSPACE
        assert fit(desc=bad, **w) == EUNSUPPORTED                        # the descriptor's error comes first
    assert fit(weight=P, cweight=P, desc=bad) == EUNSUPPORTED

    def ev(weight=None, cweight=None, loss=P, err=P, loss_b=P, flags=0, nbytes=plain, x=P, desc=d):
        return lib.enf_eval_loss(ctypes.byref(desc), x, 0, P, P, P, P, P, weight, cweight, loss, err, loss_b, P, nbytes, flags, None)
    assert ev(loss=None, err=None, loss_b=None) == EINVAL                # nothing asked for
    assert ev(weight=P, cweight=P) == EINVAL
    assert ev(flags=1) == EINVAL and ev(flags=16 | 32) == EINVAL
    assert ev(x=None) == EINVAL
    assert ev(nbytes=plain - 1) == EWORKSPACE
    assert ev(flags=16) == EWORKSPACE and ev(flags=16, loss=None) == EWORKSPACE
    assert ev(loss=None, err=None, nbytes=plain - 1) == EWORKSPACE       # loss_b alone passes the argument checks (it is allowed)
    assert ev(desc=bad) == EUNSUPPORTED and ev(loss=None, err=None, loss_b=None, desc=bad) == EUNSUPPORTED

    assert lib.enf_signal_sum(None, 2, 5, 1.0, P, None) == EINVAL
    assert lib.enf_signal_sum(P, 2, 5, 1.0, None, None) == EINVAL
    assert lib.enf_signal_sum(P, 0, 5, 1.0, P, None) == EINVAL and lib.enf_signal_sum(P, 2, 0, 1.0, P, None) == EINVAL


def test_new_keywords_exist_and_default_to_off():
    from enf_pde_amd.enf.models import EquivariantCrossAttentionNeF as NeF
    from enf_pde_amd.fitting.trainers import MetaSGDPDETrainer, NonMetaPDETrainer
    for fn, kw in ((IL.inner_loop, "per_signal_loss"), (NonMetaPDETrainer.fit_latents_step, "per_signal_loss"),
                   (NeF.mse_value_and_latent_grads, "return_errors")):
        assert inspect.signature(fn).parameters[kw].default is False, (fn, kw)
    ev = inspect.signature(NeF.eval_loss).parameters
    assert list(ev)[:9] == ["self", "params", "x", "p", "a", "gaussian_window_size", "target", "weight", "channel_weight"]
    assert ev["weight"].default is None and ev["channel_weight"].default is None
    fe = inspect.signature(MetaSGDPDETrainer.fit_errors).parameters
    assert list(fe)[:7] == ["self", "state", "batch", "masks", "weights", "normalize", "channel_weights"]
    assert fe["masks"].default is None and fe["normalize"].default is True


def test_host_tensors_raise():
    cfg = make_cfg("rel_pos_periodic", D=64, H=2, C=8, O=2)
    nef = build_nef(cfg, "f32")
    B, N, Z = 2, 5, 3
    x, p, a, s, y = torch.zeros(B, N, 2), torch.zeros(B, Z, 2), torch.ones(B, Z, 8), torch.ones(B, Z, 1), torch.zeros(B, N, 2)
    with pytest.raises(_lib.EnfError):
        nef.eval_loss(None, x, p, a, s, y)
    with pytest.raises(_lib.EnfError):
        nef.mse_value_and_latent_grads(None, x, p, a, s, y, return_errors=True)
    with pytest.raises(_lib.EnfError):
        nef.signal_losses(torch.zeros(B, N))
    from tests.test_signal_masks_host import _maml_trainer
    tr, state = _maml_trainer(False)
    with pytest.raises(_lib.EnfError):
        tr.fit_errors(state, torch.zeros(2, 30, 1))


class _Nef:
    """records what the inner loop hands to the model; no device"""
    cross_attn_invariant = NS(num_z_ori_dims=0)

    def __init__(self):
        self.steps, self.evals = [], []

    def mse_value_and_latent_grads(self, params, x, p, a, window, target, grad_scale=1.0, loss_out=None, weight=None, channel_weight=None,
                                   return_errors=False):
        self.steps.append((return_errors, weight, channel_weight))
        B, N = target.shape[:2]
        res = (loss_out, torch.zeros_like(p), torch.zeros_like(a), torch.zeros_like(window))
        return res + (torch.zeros(B, N), torch.full((B,), float(len(self.steps)))) if return_errors else res

    def eval_loss(self, params, x, p, a, window, target, weight=None, channel_weight=None, loss_out=None, per_signal=True):
        self.evals.append((x, target, weight, channel_weight))
        loss_out += 7.0
        return torch.full((target.shape[0],), -1.0), torch.zeros(target.shape[:2])

    def apply(self, *a):
        raise AssertionError("per_signal_loss=True decodes nothing")


@pytest.mark.parametrize("form", ["none", "weights", "channel_weights"])
@pytest.mark.parametrize("per_signal", [False, True])
def test_inner_loop_routes_steps_and_final_loss(monkeypatch, form, per_signal):
    """per_signal_loss=True on the framework route (CPU tensors): every step asks for the errors, the final loss is ONE eval_loss on
    the last mask's points with that mask's weights, nothing is decoded, and loss_b is (S + 1, B) in step order."""
    g = torch.Generator().manual_seed(2)
    B, N, O, Ns, S, Z = 2, 30, 3, 11, 2, 3
    img, coords = torch.randn((B, N, O), generator=g), torch.randn((N, 2), generator=g)
    lat0 = {"p_pos": torch.zeros(1, Z, 2), "a": torch.ones(1, Z, 4), "gaussian_window": torch.ones(1, Z, 1)}
    if per_signal:
        masks = torch.stack([torch.stack([torch.randperm(N, generator=g)[:Ns] for _ in range(S + 1)], 1) for _ in range(B)])
        masks[1, Ns - 3:] = -1
    else:
        masks = torch.stack([torch.randperm(N, generator=g)[:Ns] for _ in range(S + 1)], 1)
    kw = {"weights": {"weights": torch.rand((B, N), generator=g)}, "channel_weights": {"channel_weights": torch.rand((B, N, O), generator=g)},
          "none": {}}[form]
    monkeypatch.setattr(IL, "meta_sgd_update", lambda lat, grads, lrs, scale: lat)
    nef = _Nef()
    loss, lat, loss_b = IL.inner_loop(nef, None, lat0, None, coords, img, masks, per_signal_loss=True, **kw)
    assert float(loss) == 7.0 and set(lat) == set(lat0)
    assert loss_b.shape == (S + 1, B) and loss_b[:, 0].tolist() == [1.0, 2.0, -1.0]
    assert len(nef.steps) == S and all(r for r, _, _ in nef.steps) and len(nef.evals) == 1
    x, target, w, cw = nef.evals[0]
    assert x.shape == (B, Ns, 2) and target.shape == (B, Ns, O)
    if form == "channel_weights":
        assert w is None and cw.shape == (B, Ns, O)
    elif form == "weights" or per_signal:
        assert cw is None and w.shape == (B, Ns)
    else:
        assert w is None and cw is None
    if per_signal:
        pad = (cw if form == "channel_weights" else w)[1, Ns - 3:]
        assert bool((pad == 0).all()) and bool((target[1, Ns - 3:] == 0).all())      # a padded index has weight 0: err == 0 there
