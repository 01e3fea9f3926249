"""Resident weight panels of the forward pair kernel (enf_pair_fwd.hip: PairSmem's resident set): the kernel keeps some of the shared
D x D panels in LDS for a workgroup's lifetime and streams only the others through the ring.

The reference is the same kernel with an EMPTY resident set -- every panel through the ring, the kernel as it was before --, which only
the test library has (libenf_hip_test.so: enf_test_pair_fwd_streamed).  The fragments a GEMM reads are the same bytes and its MFMAs run
in the same order, so ybar, lse and out of the resident kernel must equal the streamed kernel's BIT FOR BIT; each case also stays within
tests/test_gpu_forward.py's TOL (max|err| / max|ref|) of the fp64 oracle.  Every figure is printed before it is asserted.

Shapes (B, N, Z), at D, H = 128, 2, bf16, rel_pos_periodic (the compile-time-invariant instantiation) unless said:
  z-fold          (2, 16, 1) one latent step; (2, 40, 9) ragged query tile; (2, 130, 5) a nearly empty second workgroup
  z-fold, split   (2, 300, 40) runs of latent steps that cross query-tile boundaries: a workgroup walks two segments, the resident
                  panels are loaded once
  latent-split    (2, 17, 65) idle waves in the last pass; (4, 32, 3) Z < 8: four query groups; (3, 33, 16) with
                  ENF_STAGE_SHARED_LATENTS: the parts grid
and (2, 40, 9) in both variants for: rel_pos (the run-time-invariant instantiation), (D, H) = (128, 1), (64, 2), (64, 4), the ffn
embedding, relu masks written and then read, and precision f32 (at D = 128 its resident set is empty: the two kernels are one)."""
import ctypes
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

from oracle import enf_ref_np as R
from tests.helpers import make_cfg, make_inputs, build_nef
from tests.ffn_ref import ffn_oracle, init_params_ffn, build_nef_ffn  # noqa: F401  (fixture)
from tests.test_gpu_forward import TOL
from enf_pde_amd import _lib

pytestmark = pytest.mark.gpu

_REF = {}


def _case(invariant, D, H, B, N, Z, ffn=False, shared=False):
    """weights, fp32-rounded inputs and the fp64 oracle's output, once per session"""
    key = (invariant, D, H, B, N, Z, ffn, shared)
    if key not in _REF:
        cfg = make_cfg(invariant, D=D, H=H, C=12, O=2, freq=(0.3, 0.6))
        prm = (init_params_ffn if ffn else R.init_params)(D + Z, cfg, jitter=0.1)
        f32 = lambda v: np.asarray(v, dtype=np.float32).astype(np.float64)
        x, p, a, s = (f32(v) for v in make_inputs(cfg, B, N, Z, D + Z + 1))
        if shared:            # one signal's latents and points for all of them
            x, p, a, s = (np.repeat(v[:1], B, 0) for v in (x, p, a, s))
        _REF[key] = NS(cfg=cfg, prm=prm, x=x, p=p, a=a, s=s, ref=R.nef_apply(prm, cfg, x, p, a, s), shape=(B, N, Z), shared=shared)
    return _REF[key]


def _ptr(v):
    return ctypes.c_void_p(v.data_ptr()) if v is not None else None


def _forward(cuda, lib, nef, packed, c, streamed, masks=None):
    """enf_forward_stages of the test library on caller-owned, NaN-filled ybar / lse / out, with the resident set or without"""
    B, N, Z = c.shape
    t = lambda v: torch.tensor(np.asarray(v), dtype=torch.float32, device=cuda)
    desc = nef._desc(B, N, Z, masks=masks)
    nbytes = int(lib.enf_workspace_bytes_ex(ctypes.byref(desc), 0))
    ws = torch.zeros((nbytes,), device=cuda, dtype=torch.uint8)
    x = t(c.x[0] if c.shared else c.x)
    p, a, s = t(c.p), t(c.a), t(c.s)
    HD, H = nef._Hp * nef._Dp, nef._Hp
    out = torch.full((B, N, nef.num_out), float("nan"), device=cuda)
    ybar, lse = torch.full((B, N, HD), float("nan"), device=cuda), torch.full((B, N, H), float("nan"), device=cuda)
    stages = _lib.ENF_STAGES_FORWARD | (_lib.ENF_STAGE_SHARED_LATENTS if c.shared else 0)
    lib.enf_test_pair_fwd_streamed(1 if streamed else 0)
    try:
        _lib.launch(cuda, lib.enf_forward_stages, ctypes.byref(desc), _ptr(x), 0 if c.shared else N * c.x.shape[2], _ptr(p), _ptr(a), _ptr(s),
                    _ptr(packed), _ptr(out), _ptr(ybar), _ptr(lse), _ptr(ws), nbytes, stages, ctypes.c_void_p(torch.cuda.current_stream(cuda).cuda_stream))
        torch.cuda.synchronize()
    finally:
        lib.enf_test_pair_fwd_streamed(0)
    return NS(out=out, ybar=ybar, lse=lse)


def _check(cuda, c, variant, precision, ffn=False, with_masks=False):
    lib = _lib.load_test()
    nef = (build_nef_ffn if ffn else build_nef)(c.cfg, precision)
    nef.pair_variants = (variant, "auto")
    B, N, Z = c.shape
    assert lib.enf_pair_variant(ctypes.byref(nef._desc(B, N, Z)), 0) == _lib.VARIANT[variant]
    packed = nef.pack(nef.load_params(c.prm, device=cuda))
    runs = [None]
    if with_masks:            # the masks are written by each kernel's own first pass and read back by its second
        runs = ["write", "read"]
    for mode in runs:
        got = {}
        for streamed in (True, False):
            masks = (nef.relu_mask_buffer(B, N, Z, cuda).zero_(), "write", B) if mode else None
            if mode == "read":
                _forward(cuda, lib, nef, packed, c, streamed, masks)
                masks = (masks[0], "read", B)
            got[streamed] = _forward(cuda, lib, nef, packed, c, streamed, masks)
        res, stm = got[False], got[True]
        diff = {k: float((getattr(res, k).double() - getattr(stm, k).double()).abs().max()) for k in ("ybar", "lse", "out")}
        o = res.out.cpu().numpy().astype(np.float64)
        err = float(np.abs(o - c.ref).max() / max(np.abs(c.ref).max(), 1e-6))
        print("resident panels", c.cfg["invariant"], (c.cfg["num_hidden"], c.cfg["num_heads"]), c.shape, variant, precision,
              "ffn" if ffn else "rff", "masks " + str(mode), "max|resident - streamed|", diff, "against the oracle", err)
        for k in ("ybar", "lse", "out"):
            assert bool(torch.isfinite(getattr(res, k)).all()), k
            assert torch.equal(getattr(res, k), getattr(stm, k)), (k, diff)
        assert err < TOL[precision], err


MAIN = [("z_fold", 2, 16, 1, False), ("z_fold", 2, 40, 9, False), ("z_fold", 2, 130, 5, False),
        ("z_fold_zsplit", 2, 300, 40, False),
        ("latent_split", 2, 17, 65, False), ("latent_split", 4, 32, 3, False), ("latent_split", 3, 33, 16, True)]


@pytest.mark.parametrize("variant,B,N,Z,shared", MAIN)
def test_resident_equals_streamed(cuda, variant, B, N, Z, shared):
    _check(cuda, _case("rel_pos_periodic", 128, 2, B, N, Z, shared=shared), variant, "bf16")


BOTH = ["z_fold", "latent_split"]


@pytest.mark.parametrize("variant", BOTH)
def test_run_time_invariant_instantiation(cuda, variant):
    _check(cuda, _case("rel_pos", 128, 2, 2, 40, 9), variant, "bf16")


@pytest.mark.parametrize("variant", BOTH)
@pytest.mark.parametrize("D,H", [(128, 1), (64, 2), (64, 4)])
def test_other_widths_and_heads(cuda, variant, D, H):
    _check(cuda, _case("rel_pos_periodic", D, H, 2, 40, 9), variant, "bf16")


@pytest.mark.parametrize("variant", BOTH)
def test_ffn_embedding(cuda, ffn_oracle, variant):
    _check(cuda, _case("rel_pos_periodic", 128, 2, 2, 40, 9, ffn=True), variant, "bf16", ffn=True)


@pytest.mark.parametrize("variant", BOTH)
def test_relu_masks_write_then_read(cuda, variant):
    _check(cuda, _case("rel_pos_periodic", 128, 2, 2, 40, 9), variant, "bf16", with_masks=True)


@pytest.mark.parametrize("variant", BOTH)
def test_fp32(cuda, variant):
    _check(cuda, _case("rel_pos_periodic", 128, 2, 2, 40, 9), variant, "f32")
