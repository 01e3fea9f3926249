"""The tail's active-wave forms (csrc/enf_tail.hip: AW) and the one-launch seeded forward + backward.

A tail launch whose grid would be far below the CU count runs workgroups in which only AW of the eight waves carry queries; the others
keep the weight staging and the barrier cadence.  The arithmetic of a wave does not depend on AW, so every AW in {1, 2, 4} must give the
bits of AW = 8 -- equality, not a tolerance -- on everything a form writes: `out`, the stash, d ybar, delta, err, and the loss in
deterministic mode (where the launcher keeps the 8-wave geometry and its partial-sum slots; outside it the loss is a sum of float
atomics whose order is free, so it is compared within 1e-6 relative).  The test library forces AW (enf_test_tail_active_waves) and
launches one tail form on the test's buffers (enf_test_tail).

Forms: forward, forward with the stash (SAVE), evaluation (EVAL), seeded backward from the stash, the new seeded forward + backward,
the fused loss; with O = 3 also the per-value weights of the evaluation and the fused loss.  The seeded forward + backward is also
compared, bit for bit, with the forward-with-stash launch followed by the seeded backward on the same inputs.

Queries NQ in {16, 40, 130, 519}: one tile; a ragged tile; more tiles than one workgroup holds; 33 tiles with a ragged last one and a
last workgroup whose active waves are partly idle.  (D, H) in {(128, 2), (64, 2), (128, 1)}, f32 and bf16, O in {1, 3}."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import enf_ref_np as R
from tests.helpers import make_cfg, build_nef
from enf_pde_amd import _lib

pytestmark = pytest.mark.gpu

FWD, SAVE, EVAL, SEED, FWD_SEED, LOSS = range(6)
_NEF = {}


def _setup(cuda, D, H, O, precision):
    key = (D, H, O, precision)
    if key not in _NEF:
        cfg = make_cfg("rel_pos_periodic", D=D, H=H, C=12, O=O)
        nef = build_nef(cfg, precision)
        params = nef.load_params(R.init_params(3, cfg, jitter=0.1), device=cuda)
        _NEF[key] = (nef, nef.pack(params))
    return _NEF[key]


def _ptr(v):
    return ctypes.c_void_p(v.data_ptr()) if v is not None else None


def _launch(cuda, lib, nef, packed, NQ, form, aw, inp, act=None, seed=0, weight=None, per_value=False, det=False):
    """one tail launch with `aw` active waves on 0xFF-filled outputs; returns what the form writes, as int32 words (and the loss)"""
    HD, D, O = nef._Hp * nef._Dp, nef._Dp, nef.num_out
    desc = nef._desc(1, NQ, 1)
    fill = lambda *shape: torch.full(shape, -1, device=cuda, dtype=torch.int32)
    out, dybar, delta, err = fill(NQ, O), fill(NQ, HD), fill(NQ, nef._Hp), fill(NQ)
    act = act.clone() if act is not None else fill(NQ, 2 * HD + 2 * D + 2)
    loss = torch.zeros(1, device=cuda)
    part = fill(int(lib.enf_test_tail_parts(ctypes.byref(desc)))) if det else None
    st = ctypes.c_void_p(torch.cuda.current_stream(cuda).cuda_stream)
    lib.enf_test_tail_active_waves(aw)
    try:
        _lib.launch(cuda, lib.enf_test_tail, ctypes.byref(desc), _ptr(packed), form, seed, _ptr(inp["ybar"]), _ptr(inp["target"]),
                    _ptr(weight), int(per_value), _ptr(out), _ptr(act), _ptr(dybar), _ptr(delta), _ptr(err), _ptr(loss), _ptr(part), st)
        torch.cuda.synchronize()
    finally:
        lib.enf_test_tail_active_waves(0)
    wrote = {FWD: dict(out=out), SAVE: dict(out=out, act=act), EVAL: dict(err=err), SEED: dict(dybar=dybar, delta=delta),
             FWD_SEED: dict(out=out, act=act, dybar=dybar, delta=delta), LOSS: dict(act=act, dybar=dybar, delta=delta, err=err)}[form]
    return wrote, float(loss)


@pytest.mark.parametrize("NQ", [16, 40, 130, 512 + 7])
@pytest.mark.parametrize("O", [1, 3])
@pytest.mark.parametrize("precision", ["f32", "bf16"])
@pytest.mark.parametrize("D,H", [(128, 2), (64, 2), (128, 1)])
def test_active_waves_bit_equal(cuda, D, H, precision, O, NQ):
    lib = _lib.load_test()
    nef, packed = _setup(cuda, D, H, O, precision)
    g = torch.Generator(device="cpu").manual_seed(NQ + O)
    rnd = lambda *shape: torch.randn(shape, generator=g).to(cuda)
    inp = dict(ybar=rnd(NQ, H * D), target=rnd(NQ, O))
    wq = (torch.rand((NQ,), generator=g) * 2).to(cuda)
    wq[::5] = 0.0                                            # a weight of 0: the query does not exist
    wv = (torch.rand((NQ, O), generator=g) * 2).to(cuda)
    seed = O - 1
    runs = [("forward", FWD, {}), ("save", SAVE, {}), ("eval", EVAL, {}), ("eval weighted", EVAL, dict(weight=wq)),
            ("seeded backward", SEED, dict(seed=seed)), ("seeded forward + backward", FWD_SEED, dict(seed=seed)),
            ("fused loss", LOSS, {}), ("fused loss weighted", LOSS, dict(weight=wq))]
    if O > 1:
        runs += [("eval per value", EVAL, dict(weight=wv, per_value=True)), ("fused loss per value", LOSS, dict(weight=wv, per_value=True))]
    checked = 0
    for name, form, kw in runs:
        ref = {}
        for aw in (8, 1, 2, 4):
            stash = None
            if form == SEED:                                 # its input: the stash of a forward with the same number of active waves
                stash = _launch(cuda, lib, nef, packed, NQ, SAVE, aw, inp)[0]["act"]
            got, loss = _launch(cuda, lib, nef, packed, NQ, form, aw, inp, act=stash, **kw)
            det_loss = None
            if form in (EVAL, LOSS):
                got_det, det_loss = _launch(cuda, lib, nef, packed, NQ, form, aw, inp, det=True, **kw)
                assert all(torch.equal(got[k], got_det[k]) for k in got), (name, aw, "deterministic mode")
            if aw == 8:
                ref[name] = (got, loss, det_loss)
                if form == FWD_SEED:                         # one launch against the two it replaces
                    two = dict(_launch(cuda, lib, nef, packed, NQ, SAVE, 8, inp)[0])
                    two.update(_launch(cuda, lib, nef, packed, NQ, SEED, 8, inp, act=two["act"], seed=seed)[0])
                    same = {k: bool(torch.equal(got[k], two[k])) for k in got}
                    print("tail", (D, H, precision, O, NQ), "one seeded launch against forward + seeded backward, bit-equal:", same)
                    assert all(same.values()), same
                continue
            want, wloss, wdet = ref[name]
            same = {k: bool(torch.equal(got[k], want[k])) for k in got}
            print("tail", (D, H, precision, O, NQ), name, "AW", aw, "against 8, bit-equal:", same, "loss", loss, wloss, "deterministic", det_loss, wdet)
            assert all(same.values()), (name, aw, same)
            assert all(not bool((v == -1).all()) for v in got.values()), (name, aw)          # the form did write
            if form in (EVAL, LOSS):
                assert det_loss == wdet and np.isfinite(det_loss), (name, aw, det_loss, wdet)
                assert abs(loss - wloss) <= 1e-6 * abs(wloss), (name, aw, loss, wloss)
            checked += 1
    assert checked == 3 * len(runs)
