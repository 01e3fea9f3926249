"""The forward's permission flags across the per-call modes (include/enf_hip.h: ENF_STAGE_YBAR_HALF, with ENF_STAGE_SHARED_LATENTS and
ENF_STAGE_TAIL_SAVE beside it).  A permission is "ignored where it does not apply"; whether it applies is decided in enf_forward_stages
and must hold for the pair kernel that writes `ybar` and for the tail that reads it.  Each cell of the matrix below runs ONE descriptor
twice through the raw C-ABI -- without ENF_STAGE_YBAR_HALF and with it -- on a 0xFF-filled workspace, `ybar` = `lse` = NULL unless the
cell says otherwise, `out` NaN-filled, and asserts

  * both calls return ENF_OK and the flagged `out` is finite,
  * torch.equal(out_flagged, out_unflagged): the header's promise of the same bits,
  * max|out - ref| / max|ref| < TOL[precision] of tests/test_gpu_forward.py against the fp64 oracle on the fp32-rounded inputs,
  * liveness, read off the workspace: with `written` = the 32-bit words that do not hold the fill after the call(s), a cell where the
    hand-off APPLIES has written_unflagged - written_flagged == B N H D / 2 exactly (H, D the padded values: bf16 rows are half the
    words of fp32 rows), a cell where it is IGNORED has 0.  (No finite fp32 word has the fill's pattern, nor has a pair of finite bf16
    values: the fill is a NaN in both formats.)

Default cell: (B, N, Z) = (2, 40, 9) -- a ragged 16-query tile, two latent rounds --, D, H = 128, 2, C = 12, O = 2, frequencies
(0.3, 0.6), rel_pos_periodic, bf16 (the resident-panel cases); the padded models are tests/test_gpu_tangent.py's configurations.

  live      bf16, masks off, ybar NULL, variants latent_split and z_fold: the invariants' instantiations, the widths, the padded models
            (h_true, d_true), the ffn embedding, other shapes, a call without ENF_STAGE_PROLOGUE, and ENF_STAGE_SHARED_LATENTS beside
            the flag ("that hand-off runs instead")
  ignored   f32; the split z-fold; ENF_STAGE_TAIL_SAVE; a caller-owned ybar; PAIR and TAIL in two calls; RELU MASKS written and read
            (rff): the masked pair kernels store fp32 rows only, so the tail must read fp32
  free      ffn with relu masks (the masks do nothing there): liveness unconstrained, everything else required

The call without ENF_STAGE_PROLOGUE follows a full FLAGGED call on the same workspace and inputs (that call leaves half of the ybar
region at the fill, so the difference of the two follow-up calls still measures the hand-off).  A relu-mask "read" cell replays the masks
an unflagged "write" call took on the same inputs: at that point the linearised relu IS the relu, so the oracle and the tolerance are the
unmasked ones.

Behind the matrix: the same crossing through nef.apply inside relu_masks() under no_grad, and the other entry points that run the
forward pair kernel -- enf_fit_step_ex (deterministic) and enf_eval_loss -- with masks off, written and read at the same point.
Every figure is printed before it is asserted."""
import ctypes
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

from oracle import enf_ref_np as R
from tests import ffn_ref
from tests.helpers import make_cfg, make_inputs, build_nef
from tests.test_gpu_forward import TOL
from tests.test_gpu_resident_panels import _case as resident_case
from enf_pde_amd import _lib

pytestmark = pytest.mark.gpu

YHALF, SHARED, TSAVE = _lib.ENF_STAGE_YBAR_HALF, _lib.ENF_STAGE_SHARED_LATENTS, _lib.ENF_STAGE_TAIL_SAVE
FULL = _lib.ENF_STAGES_FORWARD
DET = _lib.ENF_FIT_DETERMINISTIC
BOTH = ("latent_split", "z_fold")
RES = NS(C=12, freq=(0.3, 0.6), seed=None)            # the resident-panel cases' decoder
TAN = NS(C=8, freq=(0.05, 0.1), seed=0)               # tests/test_gpu_tangent.py's


def cell(kind, what, variant, precision="bf16", inv="rel_pos_periodic", D=128, H=2, shape=(2, 40, 9), ffn=False, model=RES, mode="full",
         masks=None, mask_signals=0):
    """kind: "live" | "ignored" | "free"; mode: "full" (one call of every stage) | "tail_save" | "own" (caller-owned ybar, lse) |
    "two_calls" | "no_prologue" | "shared"; masks: None | "write" | "read"; mask_signals: 0 = B"""
    return NS(kind=kind, what=what, variant=variant, precision=precision, inv=inv, D=D, H=H, shape=shape, ffn=ffn, model=model, mode=mode,
              masks=masks, mask_signals=mask_signals)


CELLS = []
for v in BOTH:
    # ---- live
    CELLS += [cell("live", "compile-time invariant", v),
              cell("live", "run-time invariant", v, inv="rel_pos"),
              cell("live", "latitude_periodic", v, inv="latitude_periodic"),
              cell("live", "ponita 64x2", v, inv="ponita", D=64, H=2),
              cell("live", "128x1", v, D=128, H=1),
              cell("live", "64x2", v, D=64, H=2),
              cell("live", "64x4", v, D=64, H=4),
              cell("live", "32x3 padded (h_true)", v, inv="rel_pos", D=32, H=3, model=TAN),
              cell("live", "16x2 padded (d_true)", v, inv="polar_periodic", D=16, H=2, model=TAN),
              cell("live", "ffn", v, ffn=True),
              cell("live", "nearly empty second tile", v, shape=(2, 130, 5)),
              cell("live", "one latent", v, shape=(2, 16, 1)),
              cell("live", "without the prologue", v, mode="no_prologue"),
              cell("live", "with shared latents", v, shape=(3, 33, 16), mode="shared")]
    # ---- ignored
    CELLS += [cell("ignored", "f32", v, precision="f32"),
              cell("ignored", "tail save", v, mode="tail_save"),
              cell("ignored", "caller-owned ybar", v, mode="own"),
              cell("ignored", "pair and tail in two calls", v, mode="two_calls")]
    for D_ in (128, 64):
        CELLS += [cell("ignored", f"masks write {D_}x2", v, D=D_, masks="write"),
                  cell("ignored", f"masks read {D_}x2", v, D=D_, masks="read")]
    # ---- liveness unconstrained
    CELLS += [cell("free", "ffn masks write", v, ffn=True, masks="write"),
              cell("free", "ffn masks read", v, ffn=True, masks="read")]
CELLS += [cell("ignored", "split z-fold", "z_fold_zsplit", shape=(2, 300, 40)),
          cell("ignored", "masks read, two signals per mask set", "latent_split", shape=(4, 40, 9), masks="read", mask_signals=2)]


def _id(c):
    return "-".join([c.kind, c.what.replace(" ", "_"), c.variant])


_REF = {}
_SEEN = {}          # cell id -> what the cell measured (test_the_matrix_as_a_whole)


def _case(c):
    """weights, fp32-rounded inputs and the fp64 oracle's output, once per session and never modified.  With `mask_signals` the second
    half of the batch is a copy of the first; with mode "shared" every signal holds signal 0's latents and points.  (The caller has
    patched the oracle's embedding for an ffn cell: the key carries it.)"""
    B, N, Z = c.shape
    dup = bool(c.mask_signals)
    if c.model is RES and not dup:          # the resident-panel cases themselves: one oracle run for both files
        return resident_case(c.inv, c.D, c.H, B, N, Z, ffn=c.ffn, shared=c.mode == "shared")
    key =(c.inv, c.D, c.H, c.shape, c.ffn, c.model.C, c.mode == "shared", dup)
    if key not in _REF:
        cfg = make_cfg(c.inv, D=c.D, H=c.H, C=c.model.C, O=2, freq=c.model.freq)
        seed = c.D + Z if c.model.seed is None else c.model.seed
        prm = (ffn_ref.init_params_ffn if c.ffn else R.init_params)(seed, cfg, jitter=0.1)
        f32 = lambda v: np.asarray(v, dtype=np.float32).astype(np.float64)
        x, p, a, s = (f32(v) for v in make_inputs(cfg, B // 2 if dup else B, N, Z, seed + 1))
        if dup:
            x, p, a, s = (np.concatenate([v, v], 0) for v in (x, p, a, s))
        if c.mode == "shared":
            x, p, a, s = (np.repeat(v[:1], B, 0) for v in (x, p, a, s))
        _REF[key] = NS(cfg=cfg, prm=prm, x=x, p=p, a=a, s=s, ref=R.nef_apply(prm, cfg, x, p, a, s), shape=c.shape)
    return _REF[key]


def _ptr(v):
    return ctypes.c_void_p(v.data_ptr()) if v is not None else None


def _rc(cuda, fn, *args):
    """the entry point's return code, with `cuda` as the calling thread's device"""
    with torch.cuda.device(cuda):
        return int(fn(*args))


def _dev(cuda, nef, params, k, signals=None):
    """device copies of a case's inputs (the first `signals` signals), the packed weights and the stream argument"""
    t = lambda v: torch.tensor(np.asarray(v if signals is None else v[:signals]), dtype=torch.float32, device=cuda)
    return NS(lib=_lib.load(), x=t(k.x), p=t(k.p), a=t(k.a), s=t(k.s), packed=nef.pack(params),
              st=ctypes.c_void_p(torch.cuda.current_stream(cuda).cuda_stream))


def _workspace(cuda, lib, desc, flags=0):
    nbytes = int(lib.enf_workspace_bytes_ex(ctypes.byref(desc), flags))
    assert nbytes > 0 and nbytes % 4 == 0
    return torch.full((nbytes,), 255, device=cuda, dtype=torch.uint8)


def _stages(cuda, nef, v, desc, ws, stages, own=None, shared_x=False):
    """one enf_forward_stages on workspace `ws`; `out` NaN-filled; own = (ybar, lse) or None for NULL"""
    B, N = desc.B, desc.N
    out = torch.full((B, N, nef.num_out), float("nan"), device=cuda)
    x = v.x[0].contiguous() if shared_x else v.x
    rc = _rc(cuda, v.lib.enf_forward_stages, ctypes.byref(desc), _ptr(x), 0 if shared_x else N * v.x.shape[2], _ptr(v.p), _ptr(v.a), _ptr(v.s),
             _ptr(v.packed), _ptr(out), _ptr(own[0]) if own else None, _ptr(own[1]) if own else None, _ptr(ws), ws.numel(), stages, v.st)
    torch.cuda.synchronize()
    return rc, out


def _written(ws):
    return int((ws.view(torch.int32) != -1).sum())          # words of the 0xFF-filled workspace that were overwritten


def _run(cuda, c, nef, v, flag, masks=None, signals=None):
    """the cell's call sequence without (flag = 0) or with (flag = ENF_STAGE_YBAR_HALF) the flag on every call that can carry it"""
    B, N, Z = c.shape
    B = signals or B
    desc = nef._desc(B, N, Z, masks=masks)
    ws = _workspace(cuda, v.lib, desc)
    HD, H = nef._Hp * nef._Dp, nef._Hp
    own = None
    rcs = []
    if c.mode == "own":
        own = (torch.full((B, N, HD), float("nan"), device=cuda), torch.full((B, N, H), float("nan"), device=cuda))
    if c.mode == "two_calls":
        rc, _ = _stages(cuda, nef, v, desc, ws, (FULL & ~_lib.ENF_STAGE_TAIL) | flag)
        rcs.append(rc)
        rc, out = _stages(cuda, nef, v, desc, ws, _lib.ENF_STAGE_TAIL | flag)
    elif c.mode == "no_prologue":
        rc, _ = _stages(cuda, nef, v, desc, ws, FULL | YHALF)
        rcs.append(rc)
        rc, out = _stages(cuda, nef, v, desc, ws, (FULL & ~_lib.ENF_STAGE_PROLOGUE) | flag)
    elif c.mode == "shared":            # the unflagged call is also the unshared one
        rc, out = _stages(cuda, nef, v, desc, ws, FULL | ((SHARED | YHALF) if flag else 0), shared_x=True)
    else:
        rc, out = _stages(cuda, nef, v, desc, ws, FULL | flag | (TSAVE if c.mode == "tail_save" else 0), own=own)
    rcs.append(rc)
    return NS(rcs=rcs, out=out, own=own, written=_written(ws))


def _nef(cuda, c, k):
    nef = (ffn_ref.build_nef_ffn if c.ffn else build_nef)(k.cfg, c.precision)
    nef.pair_variants = (c.variant, "auto")
    B, N, Z = c.shape
    assert _lib.load().enf_pair_variant(ctypes.byref(nef._desc(B, N, Z)), 0) == _lib.VARIANT[c.variant]
    return nef, nef.load_params(k.prm, device=cuda)


@pytest.mark.parametrize("c", CELLS, ids=_id)
def test_hand_off_matrix(cuda, monkeypatch, c):
    if c.ffn:           # tests/ffn_ref.py: the oracle with its embedding replaced, for the duration of this test
        monkeypatch.setattr(R, "rff_net", ffn_ref.ffn_net_np)
    k = _case(c)
    nef, params = _nef(cuda, c, k)
    B, N, Z = c.shape
    v = _dev(cuda, nef, params, k)
    sig = c.mask_signals or B
    bufs = [None, None]
    if c.masks == "write":              # each call writes a zeroed buffer of its own
        bufs = [nef.relu_mask_buffer(B, N, Z, cuda).zero_() for _ in range(2)]
    elif c.masks == "read":             # both calls replay what an UNFLAGGED write call took on the same inputs (its first `sig` signals)
        buf = nef.relu_mask_buffer(sig, N, Z, cuda).zero_()
        vw = _dev(cuda, nef, params, k, signals=sig)
        w = _run(cuda, NS(**{**vars(c), "mode": "full"}), nef, vw, 0, masks=(buf, "write", sig), signals=sig)
        assert w.rcs == [0]
        bufs = [buf, buf]
    plain = _run(cuda, c, nef, v, 0, masks=(bufs[0], c.masks, sig) if c.masks else None)
    flagged = _run(cuda, c, nef, v, YHALF, masks=(bufs[1], c.masks, sig) if c.masks else None)
    half = B * N * nef._Hp * nef._Dp // 2
    diff = plain.written - flagged.written
    ref_max = max(np.abs(k.ref).max(), 1e-6)
    err = {n: float(np.abs(r.out.double().cpu().numpy() - k.ref).max() / ref_max) for n, r in (("plain", plain), ("flagged", flagged))}
    finite = bool(torch.isfinite(flagged.out).all())
    same = torch.equal(flagged.out, plain.out)
    print("hand-off cell", _id(c), c.precision, c.inv, (c.D, c.H), c.shape, "ffn" if c.ffn else "rff", "masks", c.masks, "| rc", plain.rcs,
          flagged.rcs, "| finite", finite, "| equal bits", same, "| against the oracle", err, "| written", plain.written, flagged.written,
          "difference", diff, "(half the ybar words:", half, ")")
    _SEEN[_id(c)] = NS(cell=c, live=diff == half, ignored=diff == 0, err=err["flagged"])
    assert plain.rcs == [0] * len(plain.rcs) and flagged.rcs == [0] * len(flagged.rcs)          # ENF_OK
    assert finite
    assert same
    assert err["flagged"] < TOL[c.precision] and err["plain"] < TOL[c.precision], err
    if c.kind == "live":
        assert diff == half, (diff, half)
    elif c.kind == "ignored":
        assert diff == 0, (diff, half)
    if c.mode == "own":
        for got, want in zip(flagged.own, plain.own):
            assert bool(torch.isfinite(got).all()) and torch.equal(got, want)
    if c.mode == "shared":              # every signal's rows are signal 0's, bit for bit
        assert bool((flagged.out == flagged.out[:1]).all())
    if c.masks == "write" and not c.ffn:
        assert torch.equal(bufs[0], bufs[1])            # the masks the flagged call took are the unflagged call's
        assert bool((bufs[0] != 0).any())


def test_the_matrix_as_a_whole():
    """No cell is skipped or xfailed; at least 20 cells are live; every masked rff bf16 cell is ignored -- by the cell list, whose
    liveness each cell asserts for itself, and, where the whole matrix ran in this session, by what the cells measured."""
    assert 50 <= len(CELLS) <= 70 and len({_id(c) for c in CELLS}) == len(CELLS)
    live = [c for c in CELLS if c.kind == "live"]
    masked = [c for c in CELLS if c.masks and not c.ffn and c.precision == "bf16"]
    assert len(live) >= 20
    assert len(masked) >= 9 and all(c.kind == "ignored" for c in masked)
    assert all(c.kind == "free" for c in CELLS if c.masks and c.ffn)
    ran = [_SEEN[_id(c)] for c in CELLS if _id(c) in _SEEN]
    print("hand-off matrix:", len(CELLS), "cells,", len(ran), "ran;", sum(r.live for r in ran), "live and", sum(r.ignored for r in ran),
          "ignored by the workspace measure; largest error against the oracle",
          {p: max([r.err for r in ran if r.cell.precision == p], default=None) for p in ("f32", "bf16")})
    if len(ran) == len(CELLS):
        assert sum(r.live for r in ran) >= 20
        assert all(_SEEN[_id(c)].ignored for c in masked)


# ---- the same crossing through Python: a no_grad forward inside relu_masks()
@pytest.mark.parametrize("variant", BOTH)
@pytest.mark.parametrize("precision", ["bf16", "f32"])
def test_no_grad_apply_inside_relu_masks(cuda, precision, variant):
    """`with torch.no_grad(), nef.relu_masks(buf, "write" | "read", B): nef.apply(...)`: the mirror passes ENF_STAGE_YBAR_HALF (no input
    needs a gradient) on a masked call.  `out` must be the oracle's within TOL and equal, bit for bit, to the same call with a
    gradient-requiring p in the same context -- the same pair-kernel instantiation with the fp32 hand-off, which the tail rounds anyway."""
    c = cell("ignored", "python", variant, precision=precision)
    k = _case(c)
    nef, params = _nef(cuda, c, k)
    B, N, Z = c.shape
    t = lambda v: torch.tensor(v, dtype=torch.float32, device=cuda)
    x, p, a, s = t(k.x), t(k.p), t(k.a), t(k.s)
    buf = nef.relu_mask_buffer(B, N, Z, cuda).zero_()
    lib = _lib.load()
    orig = lib.enf_forward_stages
    calls = []

    class Spy:                                   # records the `stages` argument of every forward
        def __call__(self, *args):
            calls.append(int(args[-2]))
            return orig(*args)
    got = {}
    try:
        lib.enf_forward_stages = Spy()
        for mode in ("write", "read"):
            with torch.no_grad(), nef.relu_masks(buf, mode, B):
                got[mode] = nef.apply(params, x, p, a, s)
            with nef.relu_masks(buf, mode, B):
                got[mode + " grad"] = nef.apply(params, x, p.clone().requires_grad_(True), a, s).detach()
        torch.cuda.synchronize()
    finally:
        lib.enf_forward_stages = orig
    ref_max = np.abs(k.ref).max()
    err = {m: float(np.abs(o.double().cpu().numpy() - k.ref).max() / ref_max) for m, o in got.items()}
    print("no_grad apply inside relu_masks", precision, variant, "stages", calls, "against the oracle", err, "equal bits",
          {m: torch.equal(got[m], got[m + " grad"]) for m in ("write", "read")})
    assert [bool(s_ & YHALF) for s_ in calls] == [True, False, True, False], calls
    for m in ("write", "read"):
        assert bool(torch.isfinite(got[m]).all()), m
        assert err[m] < TOL[precision], (m, err)
        assert torch.equal(got[m], got[m + " grad"]), m


# ---- the other entry points that run the forward pair kernel, under masks
def _fit_or_eval(cuda, nef, v, k, which, y, masks):
    B, N, Z = k.shape
    desc = nef._desc(B, N, Z, masks=masks)
    ws = _workspace(cuda, v.lib, desc, DET)
    loss = torch.zeros(1, device=cuda)
    head = (ctypes.byref(desc), _ptr(v.x), N * v.x.shape[2], _ptr(v.p), _ptr(v.a), _ptr(v.s), _ptr(v.packed), _ptr(y))
    if which == "fit":
        r = NS(loss=loss, dp=torch.full_like(v.p, float("nan")), da=torch.full_like(v.a, float("nan")), ds=torch.full_like(v.s, float("nan")))
        rc = _rc(cuda, v.lib.enf_fit_step_ex, *head, float(B), _ptr(loss), _ptr(r.dp), _ptr(r.da), _ptr(r.ds), _ptr(ws), ws.numel(), DET, v.st)
    else:
        r = NS(loss=loss, err=torch.full((B, N), float("nan"), device=cuda), loss_b=torch.full((B,), float("nan"), device=cuda))
        rc = _rc(cuda, v.lib.enf_eval_loss, *head, None, None, _ptr(loss), _ptr(r.err), _ptr(r.loss_b), _ptr(ws), ws.numel(), DET, v.st)
    torch.cuda.synchronize()
    assert rc == 0, rc
    return r


@pytest.mark.parametrize("variant", BOTH)
@pytest.mark.parametrize("precision", ["bf16", "f32"])
@pytest.mark.parametrize("which", ["fit", "eval"])
def test_fit_step_and_eval_loss_under_relu_masks(cuda, which, precision, variant):
    """enf_fit_step_ex (ENF_FIT_DETERMINISTIC: no float atomics blur the comparison) and enf_eval_loss with masks off, written, and read
    at the point they were written at -- where the masked forward computes what the unmasked one does, in another instantiation: the
    loss within TOL (relative), the latent gradients within 20 TOL (relative to max), the bounds tests/test_gpu_shared_forward.py uses
    for "same arithmetic, other instantiation"."""
    c = cell("ignored", "entry points", variant, precision=precision)
    k = _case(c)
    nef, params = _nef(cuda, c, k)
    B, N, Z = c.shape
    v = _dev(cuda, nef, params, k)
    y = torch.tensor(np.random.default_rng(5).standard_normal((B, N, nef.num_out)), dtype=torch.float32, device=cuda)
    buf = nef.relu_mask_buffer(B, N, Z, cuda).zero_()
    off = _fit_or_eval(cuda, nef, v, k, which, y, None)
    assert all(bool(torch.isfinite(t).all()) for t in vars(off).values())
    for mode in ("write", "read"):
        r = _fit_or_eval(cuda, nef, v, k, which, y, (buf, mode, B))
        rel = lambda g, g0: float((g.double() - g0.double()).abs().max() / g0.double().abs().max())
        devs = {n: rel(t, getattr(off, n)) for n, t in vars(r).items()}
        print(which, "under relu masks", mode, precision, variant, "loss", float(r.loss), "unmasked", float(off.loss),
              "max|masked - unmasked| / max|unmasked|", devs)
        assert all(bool(torch.isfinite(t).all()) for t in vars(r).values())
        assert devs["loss"] < TOL[precision], devs
        for n in ("dp", "da", "ds"):
            if which == "fit":
                assert devs[n] < 20 * TOL[precision], (n, devs)
