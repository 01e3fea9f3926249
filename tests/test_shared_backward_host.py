"""The shared-latent backward without a GPU (include/enf_hip.h: ENF_FIT_SHARED_LATENTS, "The shared backward"): the header and the
binding, and enf_shared_backward_applies -- the one rule (enf_layout.h: enf_shared_backward_rule) the fit step asks -- over a table
of descriptors and flags: every exclusion the header lists, the five shapes of bench.py, and bad descriptors.  Nothing is launched."""
import ctypes
import os
import re

import pytest

from enf_pde_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHARED, DET = _lib.ENF_FIT_SHARED_LATENTS, _lib.ENF_FIT_DETERMINISTIC
EINVAL = -1
INV = _lib.INVARIANT_IDS
AUTO, LSPLIT, ZFOLD = _lib.VARIANT["auto"], _lib.VARIANT["latent_split"], _lib.VARIANT["z_fold"]


def _applies(flags=SHARED, B=16, N=512, Z=64, H=2, D=128, C=16, O=1, inv="rel_pos_periodic", prec="bf16", variants=(AUTO, AUTO), **kw):
    d = _lib.make_desc(B, N, Z, H, D, C, O, 3 if inv in ("ball", "ball_lat") else 2, INV[inv], 1, _lib.PREC[prec], variants=variants, **kw)
    return _lib.load().enf_shared_backward_applies(ctypes.byref(d), flags)


def test_header_declares_and_lib_binds():
    with open(os.path.join(ROOT, "include", "enf_hip.h")) as f:
        h = f.read()
    assert re.search(r"\bint\s+enf_shared_backward_applies\s*\(\s*const\s+EnfDesc\s*\*\s*d\s*,\s*unsigned\s+flags\s*\)", h)
    assert "enf_shared_backward_applies" in _lib.EXPORTS
    assert re.search(r"#define\s+ENF_ABI_VERSION\s+2\b", h)                      # additive


def test_the_headline_shape_takes_it_in_both_precisions():
    assert _applies(prec="bf16") == 1 and _applies(prec="f32") == 1


@pytest.mark.parametrize("why,kw", [
    ("the flag is not set", dict(flags=0)),
    ("deterministic mode", dict(flags=SHARED | DET)),
    ("one signal: nothing is shared", dict(B=1, Z=256)),
    ("more than one output channel", dict(O=2)),
    ("the forward resolves to the z-fold kernel: no shared forward", dict(variants=(ZFOLD, AUTO))),
    ("the decode shape: 512 query tiles, the z-fold forward", dict(N=4096)),
    ("the backward resolves to the latent-split kernel (B Z < 192)", dict(B=2)),
    ("the latent-split backward is forced", dict(variants=(AUTO, LSPLIT))),
    ("the ffn embedding", dict(embedding=1)),
    ("ball: per-latent phases", dict(inv="ball", D=64)),
    ("ball_lat: per-latent phases", dict(inv="ball_lat", D=64)),
    ("no instantiation at (64, 1)", dict(D=64, H=1)),
    ("no instantiation at (64, 4)", dict(D=64, H=4)),
])
def test_every_exclusion(why, kw):
    assert _applies(**kw) == 0, why


def test_relu_masks_exclude_it():
    class Buf:                                   # (make_desc only asks for the address; nothing is launched)
        @staticmethod
        def data_ptr():
            return 4096
    assert _applies(masks=(Buf, "read", 16)) == 0
    assert _applies(masks=(Buf, "write", 16)) == 0


def test_forced_variants_and_the_other_instantiations():
    assert _applies(B=5, N=40, Z=9, variants=(LSPLIT, ZFOLD)) == 1              # small shapes with the z-fold backward forced
    assert _applies(B=5, N=40, Z=9, variants=(LSPLIT, AUTO)) == 0
    for D, H in ((128, 2), (128, 1), (64, 2)):
        for prec in ("f32", "bf16"):
            assert _applies(B=6, N=48, Z=24, D=D, H=H, prec=prec, variants=(LSPLIT, ZFOLD)) == 1, (D, H, prec)
    for inv in ("latitude_periodic", "polar_periodic", "ponita", "abs_pos", "rel_pos", "norm_rel_pos"):
        assert _applies(inv=inv) == 1, inv


def test_the_shapes_of_the_benchmark():
    """bench.py CONFIGS 1-5 at their fit shapes (B signals, N_s sampled points)"""
    assert _applies(B=32, N=1024, Z=16, D=64, inv="ponita") == 0               # 1: 256 query tiles, the z-fold forward
    assert _applies(B=16, N=512, Z=64) == 1                                     # 2: the headline
    assert _applies(B=4, N=4096, Z=128, C=32, O=3, inv="latitude_periodic") == 0        # 3: three fields
    assert _applies(B=8, N=512, Z=128) == 1                                     # 4
    assert _applies(B=2, N=512, Z=64) == 0                                      # 5: 128 latent rows, the latent-split backward


def test_bad_descriptors_and_flags():
    assert _applies(O=33) < 0 and _applies(D=96) < 0 and _applies(B=0) < 0
    for unknown in (1, 64, 256):
        assert _applies(flags=SHARED | unknown) == EINVAL
