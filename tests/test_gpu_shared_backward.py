"""The shared-latent backward on the GPU (include/enf_hip.h: ENF_FIT_SHARED_LATENTS, "The shared backward"): with equal latents and
points, one output channel and the z-fold backward, a flagged fit step runs tail, loss and the backward pair kernel ONCE, on signal 0
with a unit-seeded tail backward, and contracts the pair kernel's sums over queries with d out (B, N) on fp32 matrix instructions.

Flagged against unflagged enf_fit_step_w (both with float atomics: the shared path has no deterministic form).  The per-pair arithmetic
is the same; what differs is the fp32 order of the sums over queries and latents (and, in bf16 mode, that d out is multiplied in fp32
instead of being rounded to a bf16 operand per signal: measured 4e-6 of the maximum in fp32, 1.4e-2 in bf16), so the bounds are those of
tests/test_gpu_shared_forward.py: the forward tolerance tau (tests/test_gpu_forward.py: TOL, max|err| / max|ref|) on the loss and
20 tau on the latent gradients behind a re-ordered sum.  Every figure is printed before it is asserted.

Shapes (B, N, Z), with O = 1 and pair_variants = ("latent_split", "z_fold") so that the small shapes take the z-fold backward:
(5, 40, 9) B < 16 leaves zero rows in the A operand, the query tile is ragged, fewer tiles than waves; (16, 33, 64); (17, 130, 6) two
groups of signals, the second holding one signal, 9 tiles in two query splits; (2, 16, 3); (6, 48, 24) at (D, H) = (64, 2) and (128, 1).

That the flagged call took the shared path: enf_shared_backward_applies returns 1, and the floats [N H, B N H) of the workspace's delta
region -- which only the ordinary backward writes (the header's workspace paragraph) -- still hold the 0xFF fill after the call."""
import ctypes
import importlib
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

from oracle import enf_ref_np as R
from oracle import enf_ref_torch as T
from tests.helpers import make_cfg, make_inputs, build_nef
from tests.test_gpu_forward import TOL
from tests.test_gpu_backward import TOL as GTOL, rel
from enf_pde_amd import _lib

IL = importlib.import_module("enf_pde_amd.fitting.inner_loop")

pytestmark = pytest.mark.gpu

SHARED, DET = _lib.ENF_FIT_SHARED_LATENTS, _lib.ENF_FIT_DETERMINISTIC
VARIANTS = ("latent_split", "z_fold")
CASES = [(5, 40, 9, 128, 2), (16, 33, 64, 128, 2), (17, 130, 6, 128, 2), (2, 16, 3, 128, 2), (6, 48, 24, 64, 2), (6, 48, 24, 128, 1)]
_REF = {}


def _case(B, N, Z, D, H, O=1, seed=71, C=12, freq=(0.3, 0.6)):
    """weights and inputs, once per session: one signal's latents and points (fp32-rounded), per-signal targets and weights"""
    key = (B, N, Z, D, H, O, seed, C, freq)
    if key not in _REF:
        cfg = make_cfg("rel_pos_periodic", D=D, H=H, C=C, O=O, freq=freq)
        prm = R.init_params(seed, cfg, jitter=0.1)
        f32 = lambda v: np.asarray(v, dtype=np.float32).astype(np.float64)
        x, p, a, s = (f32(v[:1]) for v in make_inputs(cfg, 1, N, Z, seed + 1))
        rng = np.random.default_rng(seed + 2)
        y = f32(rng.standard_normal((B, N, O)))
        w = f32(rng.uniform(0.2, 2, (B, N)))
        _REF[key] = NS(cfg=cfg, prm=prm, x=x[0], p=np.repeat(p, B, 0), a=np.repeat(a, B, 0), s=np.repeat(s, B, 0), y=y, w=w,
                       shape=(B, N, Z))
    return _REF[key]


def _t(cuda):
    return lambda v: torch.tensor(np.asarray(v), dtype=torch.float32, device=cuda)


def _ptr(v):
    return ctypes.c_void_p(v.data_ptr()) if v is not None else None


def _fit(cuda, nef, params, c, flags, weighted=True, grad_scale=None, err=False):
    """one raw fit step on NaN-filled outputs and a 0xFF-filled workspace: enf_fit_step_w, or enf_fit_step_e with the error outputs"""
    B, N, Z = c.shape
    lib = _lib.load()
    t = _t(cuda)
    desc = nef._desc(B, N, Z)
    nbytes = int(lib.enf_workspace_bytes_ex(ctypes.byref(desc), flags & DET))
    ws = torch.full((nbytes,), 255, device=cuda, dtype=torch.uint8)
    x, p, a, s, y, w = t(c.x), t(c.p), t(c.a), t(c.s), t(c.y), (t(c.w) if weighted else None)
    packed = nef.pack(params)
    st = ctypes.c_void_p(torch.cuda.current_stream(cuda).cuda_stream)
    loss = torch.zeros(1, device=cuda)
    dp, da, ds = (torch.full_like(g, float("nan")) for g in (p, a, s))
    head = (ctypes.byref(desc), _ptr(x), 0, _ptr(p), _ptr(a), _ptr(s), _ptr(packed), _ptr(y),
            float(B if grad_scale is None else grad_scale), _ptr(loss), _ptr(dp), _ptr(da), _ptr(ds), _ptr(ws), nbytes)
    if err:
        e, lb = torch.empty((B, N), device=cuda), torch.empty((B,), device=cuda)
        _lib.launch(cuda, lib.enf_fit_step_e, *head, _ptr(w), None, _ptr(e), _ptr(lb), flags, st)
    else:
        _lib.launch(cuda, lib.enf_fit_step_w, *head, _ptr(w), flags, st)
    torch.cuda.synchronize()
    return NS(loss=loss, dp=dp, da=da, ds=ds, ws=ws, applies=int(lib.enf_shared_backward_applies(ctypes.byref(desc), flags)))


def _dev_rel(got, ref):
    return float((got.double() - ref.double()).abs().max() / ref.double().abs().max())


def _delta_tail(nef, ws, B, N, Z):
    """the floats [N H, B N H) of the workspace's delta region (enf_layout.h: EnfWorkspace, every region 256-byte aligned)"""
    H, D = nef._Hp, nef._Dp
    al = lambda v: (v + 255) & ~255
    stride = ((2 * H * D + 32 + D) + 63) & ~63
    o = 0
    for nb in (4 * B * Z * stride, 4 * B * Z * (2 * D + 2), 4 * B * Z * 2 * H * D, 4 * B * N * H * D, 4 * B * N * H, 4 * B * N * H * D):
        o = al(o + nb)                                           # lt, an, kv, ybar, lse, dybar -> delta
    return ws[o:o + 4 * B * N * H].view(torch.int32)[N * H:]


@pytest.mark.parametrize("weighted", [True, False])
@pytest.mark.parametrize("precision", ["f32", "bf16"])
@pytest.mark.parametrize("B,N,Z,D,H", CASES)
def test_fit_step_flagged_against_unflagged(cuda, B, N, Z, D, H, precision, weighted):
    c = _case(B, N, Z, D, H)
    nef = build_nef(c.cfg, precision)
    nef.pair_variants = VARIANTS
    params = nef.load_params(c.prm, device=cuda)
    plain, flagged = _fit(cuda, nef, params, c, 0, weighted), _fit(cuda, nef, params, c, SHARED, weighted)
    devs = {k: _dev_rel(getattr(flagged, k), getattr(plain, k)) for k in ("loss", "dp", "da", "ds")}
    tail_p, tail_f = _delta_tail(nef, plain.ws, B, N, Z), _delta_tail(nef, flagged.ws, B, N, Z)
    print("shared backward", (B, N, Z, D, H), precision, "weighted" if weighted else "unweighted", "applies", flagged.applies,
          "max|flagged - plain| / max|plain|", devs, "delta words of signals 1.. still filled:", int((tail_f == -1).sum()), "of", tail_f.numel(),
          "(unflagged:", int((tail_p == -1).sum()), ")")
    assert flagged.applies == 1 and plain.applies == 0
    # the launch, not only the query: the ordinary backward writes every signal's delta, the shared one signal 0's alone
    assert bool((tail_f == -1).all()) and not bool((tail_p == -1).any())
    assert all(bool(torch.isfinite(getattr(flagged, k)).all()) for k in devs)
    assert devs["loss"] < TOL[precision], devs
    for k in ("dp", "da", "ds"):
        assert devs[k] < 20 * TOL[precision], (k, devs)


@pytest.mark.parametrize("precision", ["f32", "bf16"])
def test_fit_step_flagged_against_the_oracle(cuda, precision):
    """(B, N, Z) = (5, 40, 9): the flagged step's loss and latent gradients against fp64 autograd of the oracle, with the tolerances of
    tests/test_gpu_backward.py (relative L2 per gradient tensor) and the forward tolerance on the loss, on that file's rel_pos_periodic
    decoder (latent_dim 16, frequencies (0.5, 1.0), seed 0) with one output.  The step without the flag is measured beside it."""
    B, N, Z = 5, 40, 9
    c = _case(B, N, Z, 128, 2, O=1, seed=0, C=16, freq=(0.5, 1.0))
    tp = T.to_torch(c.prm, torch.float64)
    qp, qa, qs = (torch.tensor(v, requires_grad=True) for v in (c.p, c.a, c.s))
    xb = torch.tensor(np.broadcast_to(c.x[None], (B,) + c.x.shape).copy())
    lref = ((T.nef_apply(tp, c.cfg, xb, qp, qa, qs) - torch.tensor(c.y)) ** 2).mean()
    lref.backward()
    nef = build_nef(c.cfg, precision)
    nef.pair_variants = VARIANTS
    params = nef.load_params(c.prm, device=cuda)
    lref = float(lref.detach())
    for flags in (0, SHARED):                             # (the step without the flag is measured beside it, the flagged one asserted)
        r = _fit(cuda, nef, params, c, flags, weighted=False, grad_scale=1.0)
        el = abs(float(r.loss) - lref) / lref
        errs = {k: rel(g.double().cpu().numpy(), q.grad.numpy()) for k, g, q in (("p", r.dp, qp), ("a", r.da, qa), ("sigma", r.ds, qs))}
        print("fit step against the oracle", precision, "flagged" if flags & SHARED else "plain", "applies", r.applies, "loss", el, errs)
    assert r.applies == 1
    assert el < TOL[precision], el
    for k, e in errs.items():
        assert np.isfinite(e) and e < GTOL[precision], (k, errs)


@pytest.mark.parametrize("precision", ["f32", "bf16"])
def test_the_permission_falls_back(cuda, precision):
    """deterministic mode, two output channels, the per-point errors asked for, the latent-split backward: the flagged call is the call
    with the shared forward alone.  There is no second entry point that runs "the shared forward alone" to compare bits with -- where the
    rule says 0 the flagged call IS that sequence -- and outside deterministic mode the ordinary backward's float atomics make two runs
    of one call differ in their last bits.  So: in deterministic mode the flagged call equals the deterministic shared-forward call bit
    for bit; for the other exclusions the rule says 0, every signal's delta is written (the ordinary backward ran: the shared one leaves
    signals 1.. untouched) and loss and gradients agree with the deterministic shared-forward call within the bounds of this file."""
    B, N, Z = 5, 40, 9
    for why, O, variants, flags, err in (("deterministic", 1, VARIANTS, DET | SHARED, False), ("two outputs", 2, VARIANTS, SHARED, False),
                                         ("errors asked for", 1, VARIANTS, SHARED, True),
                                         ("latent-split backward", 1, ("latent_split", "latent_split"), SHARED, False)):
        c = _case(B, N, Z, 128, 2, O=O)
        nef = build_nef(c.cfg, precision)
        nef.pair_variants = variants
        params = nef.load_params(c.prm, device=cuda)
        r = _fit(cuda, nef, params, c, flags, err=err)
        tail = _delta_tail(nef, r.ws, B, N, Z)
        print("fallback", why, precision, "applies", r.applies, "delta words of signals 1.. still filled:", int((tail == -1).sum()))
        if not err:
            assert r.applies == 0, why
        assert not bool((tail == -1).any()), why
        assert all(bool(torch.isfinite(getattr(r, k)).all()) for k in ("loss", "dp", "da", "ds")), why
        # against the same call in deterministic mode (fixed-order sums: the shared forward alone, same bits run to run)
        a, b = _fit(cuda, nef, params, c, DET | SHARED, err=err), _fit(cuda, nef, params, c, DET | SHARED, err=err)
        assert all(torch.equal(getattr(a, k), getattr(b, k)) for k in ("loss", "dp", "da", "ds")), why
        devs = {k: _dev_rel(getattr(r, k), getattr(a, k)) for k in ("loss", "dp", "da", "ds")}
        print("fallback", why, precision, "against the deterministic shared-forward call", devs)
        if flags & DET:
            assert all(torch.equal(getattr(r, k), getattr(a, k)) for k in devs), why
        else:                                            # float atomics in the ordinary backward: equal up to their order
            assert devs["loss"] < TOL[precision] and all(devs[k] < 20 * TOL[precision] for k in ("dp", "da", "ds")), (why, devs)


def test_inner_loop_with_the_hint_against_without(cuda, monkeypatch):
    """inner_loop on B = 16 signals, an 8 x 8 grid, 32 sampled points, 16 latents (B Z = 256: the z-fold backward is chosen
    automatically, and with it the shared backward at step 0), S = 2: the fitted latents with the hint on against a run with it off."""
    B, side, Ns, Z, S, C = 16, 8, 32, 16, 2, 12
    c = _case(B, Ns, Z, 128, 2, O=1)
    rng = np.random.default_rng(5)
    lin = np.linspace(-1, 1, side, endpoint=False)
    t = _t(cuda)
    coords = t(np.stack(np.meshgrid(lin, lin), -1).reshape(-1, 2))
    img = t(rng.standard_normal((B, side * side, 1)))
    lat0 = {"p_pos": t(R.init_positions_grid(1, Z, 2) + 0.02 * rng.standard_normal((1, Z, 2))),
            "a": t(1 + 0.1 * rng.standard_normal((1, Z, C))), "gaussian_window": t(np.full((1, Z, 1), 0.5))}
    lrs = {"p_pos": t([0.5]), "a": t(np.full((C,), 2.0)), "gaussian_window": t([0.0])}
    masks = torch.tensor(np.stack([rng.permutation(side * side)[:Ns] for _ in range(S + 1)], 1), device=cuda)
    nef = build_nef(c.cfg, "f32")
    params = nef.load_params(c.prm, device=cuda)
    assert _lib.load().enf_shared_backward_applies(ctypes.byref(nef._desc(B, Ns, Z)), SHARED) == 1

    def run():
        gen = torch.Generator().manual_seed(9)
        loss, fit = IL.inner_loop(nef, params, lat0, lrs, coords, img, masks, generator=gen)
        torch.cuda.synchronize()
        return float(loss), fit
    loss, fit = run()
    monkeypatch.setattr(IL, "_shared_kw", lambda *a, **k: {})
    loss_off, fit_off = run()
    devs = {k: _dev_rel(fit[k], fit_off[k]) for k in fit}
    print("inner loop, hint on against off: loss", loss, loss_off, devs)
    assert abs(loss - loss_off) <= TOL["f32"] * abs(loss_off)
    for k, d in devs.items():
        assert d < 20 * TOL["f32"], (k, devs)
