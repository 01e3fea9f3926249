"""The shared-latent forward without a GPU (include/enf_hip.h: ENF_FIT_SHARED_LATENTS / ENF_STAGE_SHARED_LATENTS): the header and the
bindings, the argument checks of the flagged entry points (every call here fails its checks, so nothing is launched), the unchanged
workspace sizes, the part count of enf_shared_forward_parts, and which inner steps are handed the hint."""
import ctypes
import importlib
import inspect
import os
import re
from types import SimpleNamespace as NS

import pytest
import torch

from enf_pde_amd import _lib

IL = importlib.import_module("enf_pde_amd.fitting.inner_loop")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, EINVAL, EWORKSPACE = 0, -1, -4
SHARED, DET = 128, 16


def _desc(B, N, Z, H=2, D=128, C=16, O=1, variants=(0, 0)):
    d = _lib.make_desc(B, N, Z, H, D, C, O, 2, 0, 1, 0)
    d.pair_fwd_variant, d.pair_bwd_variant = variants
    return d


def test_header_declares_and_lib_binds():
    with open(os.path.join(ROOT, "include", "enf_hip.h")) as f:
        h = f.read()
    assert re.search(r"#define\s+ENF_ABI_VERSION\s+2\b", h)                      # additive
    assert re.search(r"#define\s+ENF_FIT_SHARED_LATENTS\s+128u", h) and re.search(r"#define\s+ENF_STAGE_SHARED_LATENTS\s+128u", h)
    stage_bits = [int(v) for v in re.findall(r"#define\s+ENF_STAGE_\w+\s+(\d+)u", h)]
    assert len(stage_bits) == len(set(stage_bits)) and all(b & (b - 1) == 0 for b in stage_bits)      # no collision
    assert _lib.ENF_FIT_SHARED_LATENTS == _lib.ENF_STAGE_SHARED_LATENTS == SHARED
    assert re.search(r"\bint\s+enf_shared_forward_parts\s*\(", h) and "enf_shared_forward_parts" in _lib.EXPORTS
    assert _lib.load().enf_abi_version() == 2


def test_argument_checks_without_a_launch():
    lib = _lib.load()
    dummy = ctypes.create_string_buffer(64)
    P = ctypes.cast(dummy, ctypes.c_void_p)
    d, one = _desc(2, 70, 9, O=3), _desc(1, 70, 9, O=3)
    plain = lib.enf_workspace_bytes(ctypes.byref(d))

    def w(flags, stride, desc=d, nbytes=0):
        return lib.enf_fit_step_w(ctypes.byref(desc), P, stride, P, P, P, P, P, 1.0, P, P, P, P, P, nbytes, None, flags, None)

    def ex(flags, stride, desc=d, nbytes=0):
        return lib.enf_fit_step_ex(ctypes.byref(desc), P, stride, P, P, P, P, P, 1.0, P, P, P, P, P, nbytes, flags, None)

    def cw(flags, stride, desc=d, nbytes=0):
        return lib.enf_fit_step_cw(ctypes.byref(desc), P, stride, P, P, P, P, P, 1.0, P, P, P, P, P, nbytes, P, flags, None)

    def e(flags, stride, desc=d, nbytes=0):
        return lib.enf_fit_step_e(ctypes.byref(desc), P, stride, P, P, P, P, P, 1.0, P, P, P, P, P, nbytes, None, None, P, P, flags, None)

    def fwd(stages, stride, desc=d, nbytes=0):
        return lib.enf_forward_stages(ctypes.byref(desc), P, stride, P, P, P, P, P, P, P, P, nbytes, stages, None)

    for call in (w, ex, cw, e):
        # a workspace of 0 bytes: a call that passes its argument checks stops at ENF_EWORKSPACE, before any launch
        assert call(SHARED, 0) == EWORKSPACE and call(SHARED | DET, 0) == EWORKSPACE, call.__name__        # the bit is known
        assert call(SHARED, 140) == EINVAL and call(SHARED | DET, 140) == EINVAL, call.__name__            # signals with their own points
        assert call(0, 140) == EWORKSPACE, call.__name__                                                   # (not an error without the flag)
        assert call(SHARED, 140, desc=one) == EWORKSPACE, call.__name__                                    # B == 1: the flag says nothing
        for unknown in (1, 64, 256):
            assert call(SHARED | unknown, 0) == EINVAL, (call.__name__, unknown)
    assert fwd(15 | SHARED, 0) == EWORKSPACE and fwd(15, 140) == EWORKSPACE
    assert fwd(15 | SHARED, 140) == EINVAL and fwd(15 | SHARED, 140, desc=one) == EWORKSPACE
    assert plain > 0


@pytest.mark.parametrize("B,N,Z,variants", [(16, 512, 64, (0, 0)), (2, 70, 9, (0, 0)), (4, 4608, 128, (0, 0)), (3, 100, 70, (1, 1))])
def test_workspace_sizes_do_not_change(B, N, Z, variants):
    lib = _lib.load()
    d = _desc(B, N, Z, variants=variants)
    plain = lib.enf_workspace_bytes(ctypes.byref(d))
    det = lib.enf_workspace_bytes_ex(ctypes.byref(d), DET)
    assert plain > 0 and det > plain
    assert lib.enf_workspace_bytes_ex(ctypes.byref(d), SHARED) == plain == lib.enf_workspace_bytes_ex(ctypes.byref(d), 0)
    assert lib.enf_workspace_bytes_ex(ctypes.byref(d), SHARED | DET) == det
    assert lib.enf_workspace_bytes_ex(ctypes.byref(d), SHARED | 64) == 0                               # an unknown bit still is one


def _parts(B, N, Z, H=2, D=128, variants=(0, 0)):
    n = ctypes.c_int32(-7)
    rc = _lib.load().enf_shared_forward_parts(ctypes.byref(_desc(B, N, Z, H=H, D=D, variants=variants)), ctypes.byref(n))
    return rc, n.value


def test_part_count():
    """P is the largest power of two with P ZS <= Z (every wave of every part gets a latent), tiles P <= 256 and
    P (HD + 3 H) <= B (HD + H) (the parts fit the borrowed d ybar | delta region)."""
    assert _parts(16, 512, 64) == (1, 8)                   # the headline fit shape: 32 tiles x 8 parts = 256 workgroups
    assert _parts(2, 512, 64) == (1, 1)                    # 2 x 262 floats per query do not fit 2 x 258: signal 0 once, then the broadcast
    assert _parts(2, 64, 64) == (1, 1)
    for Z in (1, 2, 3, 5, 7, 8, 9, 15):                    # fewer than two full parts of 8 (or ZS) latents
        assert _parts(16, 512, Z) == (1, 1), Z
    assert _parts(16, 512, 16) == (1, 2) and _parts(16, 512, 31) == (1, 2) and _parts(16, 512, 32) == (1, 4)
    assert _parts(16, 33, 64) == (1, 8) and _parts(5, 40, 9) == (1, 1) and _parts(4, 32, 3) == (1, 1)
    assert _parts(3, 100, 70) == (1, 2)                    # the region: 2 x 262 <= 3 x 258 < 4 x 262
    assert _parts(16, 1024, 64) == (1, 4)                  # 64 tiles: 4 parts fill the 256 compute units
    assert _parts(16, 16 * 256, 64, variants=(1, 0)) == (1, 1)         # 256 tiles already do
    assert _parts(16, 33, 65) == (1, 8) and _parts(6, 40, 33) == (1, 4)          # short last parts: 2 of 9 and 6 of 9 latents
    assert _parts(17, 33, 129) == (1, 16)                  # parts of 9: the 16th starts at 135 > Z -- a whole part can be empty from P = 16 on
    assert _parts(6, 48, 24, H=2, D=64) == (1, 2) and _parts(6, 48, 24, H=1, D=128) == (1, 2)
    assert _parts(1, 512, 64) == (0, 1)                    # one signal: nothing is shared
    assert _parts(16, 4096, 64) == (0, 1)                  # the decode shape resolves to the z-fold forward
    assert _parts(16, 512, 64, variants=(2, 0)) == (0, 1) and _parts(16, 512, 64, variants=(1, 0)) == (1, 8)
    n = ctypes.c_int32(0)
    bad = _lib.make_desc(2, 70, 9, 2, 128, 16, 33, 2, 0, 1, 0)
    assert _lib.load().enf_shared_forward_parts(ctypes.byref(bad), ctypes.byref(n)) < 0
    assert _lib.load().enf_shared_forward_parts(ctypes.byref(_desc(2, 70, 9)), None) == EINVAL


def test_keyword_exists_and_defaults_to_off():
    from enf_pde_amd.enf.models import EquivariantCrossAttentionNeF as NeF
    assert inspect.signature(NeF.mse_value_and_latent_grads).parameters["shared_latents"].default is False


class _Nef:
    """records what the inner loop hands to the model; no device"""
    cross_attn_invariant = NS(num_z_ori_dims=0)

    def __init__(self):
        self.hints = []

    def mse_value_and_latent_grads(self, params, x, p, a, window, target, grad_scale=1.0, loss_out=None, weight=None, channel_weight=None,
                                   return_errors=False, shared_latents=False):
        self.hints.append(shared_latents)
        B, N = target.shape[:2]
        res = (loss_out, torch.zeros_like(p), torch.zeros_like(a), torch.zeros_like(window))
        return res + (torch.zeros(B, N), torch.zeros(B)) if return_errors else res

    def eval_loss(self, params, x, p, a, window, target, weight=None, channel_weight=None, loss_out=None, per_signal=True):
        return torch.zeros(target.shape[0]), torch.zeros(target.shape[:2])

    def apply(self, params, x, p, a, window):
        raise _Stop()


class _Stop(Exception):
    pass


@pytest.mark.parametrize("form", ["none", "weights", "channel_weights", "per_signal_loss"])
@pytest.mark.parametrize("per_signal,noise,want", [(False, 0.0, [True, False, False]), (True, 0.0, [False] * 3), (False, 0.1, [False] * 3)])
def test_inner_loop_hands_the_hint_to_step_0_only(monkeypatch, form, per_signal, noise, want):
    g = torch.Generator().manual_seed(2)
    B, N, O, Ns, S, Z = 2, 30, 3, 11, 3, 3
    img, coords = torch.randn((B, N, O), generator=g), torch.randn((N, 2), generator=g)
    lat0 = {"p_pos": torch.zeros(1, Z, 2), "a": torch.ones(1, Z, 4), "gaussian_window": torch.ones(1, Z, 1)}
    if per_signal:
        masks = torch.stack([torch.stack([torch.randperm(N, generator=g)[:Ns] for _ in range(S + 1)], 1) for _ in range(B)])
    else:
        masks = torch.stack([torch.randperm(N, generator=g)[:Ns] for _ in range(S + 1)], 1)
    kw = {"weights": {"weights": torch.rand((B, N), generator=g)}, "channel_weights": {"channel_weights": torch.rand((B, N, O), generator=g)},
          "none": {}, "per_signal_loss": {"per_signal_loss": True}}[form]
    monkeypatch.setattr(IL, "meta_sgd_update", lambda lat, grads, lrs, scale: lat)
    nef = _Nef()
    try:
        IL.inner_loop(nef, None, lat0, None, coords, img, masks, noise_pos=noise, generator=g, **kw)
    except _Stop:                                          # (the final-loss decode of the plain loops: the steps are behind us)
        pass
    assert nef.hints == want


def test_a_decoder_in_deterministic_mode_is_not_given_the_hint(monkeypatch):
    """deterministic mode keeps a fit on shared masks bit-equal to the fit on per-signal masks that repeat them
    (tests/test_gpu_signal_masks.py), so the re-ordered forward is not asked for there"""
    class Det(_Nef):
        mode = True

        def is_deterministic(self):
            return self.mode
    g = torch.Generator().manual_seed(4)
    img, coords = torch.randn((2, 20, 1), generator=g), torch.randn((20, 2), generator=g)
    lat0 = {"p_pos": torch.zeros(1, 3, 2), "a": torch.ones(1, 3, 4), "gaussian_window": torch.ones(1, 3, 1)}
    masks = torch.stack([torch.randperm(20, generator=g)[:7] for _ in range(3)], 1)
    monkeypatch.setattr(IL, "meta_sgd_update", lambda lat, grads, lrs, scale: lat)
    for mode, want in ((True, [False, False]), (False, [True, False])):
        nef = Det()
        nef.mode = mode
        with pytest.raises(_Stop):
            IL.inner_loop(nef, None, lat0, None, coords, img, masks)
        assert nef.hints == want, mode


def test_a_decoder_that_does_not_know_the_hint_is_not_given_it(monkeypatch):
    class Old(_Nef):
        def mse_value_and_latent_grads(self, params, x, p, a, window, target, grad_scale=1.0, loss_out=None, weight=None):
            self.hints.append(None)
            return loss_out, torch.zeros_like(p), torch.zeros_like(a), torch.zeros_like(window)
    g = torch.Generator().manual_seed(3)
    img, coords = torch.randn((2, 20, 1), generator=g), torch.randn((20, 2), generator=g)
    lat0 = {"p_pos": torch.zeros(1, 3, 2), "a": torch.ones(1, 3, 4), "gaussian_window": torch.ones(1, 3, 1)}
    masks = torch.stack([torch.randperm(20, generator=g)[:7] for _ in range(3)], 1)
    monkeypatch.setattr(IL, "meta_sgd_update", lambda lat, grads, lrs, scale: lat)
    nef = Old()
    with pytest.raises(_Stop):
        IL.inner_loop(nef, None, lat0, None, coords, img, masks)
    assert nef.hints == [None, None]
