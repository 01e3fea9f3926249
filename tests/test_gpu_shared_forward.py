"""The shared-latent forward on the GPU (include/enf_hip.h: ENF_FIT_SHARED_LATENTS / ENF_STAGE_SHARED_LATENTS): with the flag the
latent-split pair kernel runs once, for signal 0, its latents in P parts (enf_shared_forward_parts), and a merge kernel writes the row
to all B signals.  Inputs: latents replicated over B, x one point set expanded with stride 0.

The flagged call is compared with the call without the flag.  The per-pair arithmetic is the same; what differs is the fp32 order in
which a query's partial sums over the latents are added, so the bound is the project's forward tolerance tau (tests/test_gpu_forward.py:
TOL, max|err| / max|ref|) for ybar, lse, out and the loss, and 20 tau for the latent gradients behind the re-ordered forward (the factor
of test_config3_decode_shape_picks_the_split_z_fold_and_agrees).  Every figure is printed before it is asserted.

Shapes (D, H = 128, 2 unless said): (5, 40, 9) ragged query tile, second latent pass with seven idle waves, P = 1; (16, 33, 64) P = 8;
(3, 100, 70) P = 2 with parts of 35 latents (not a multiple of 8: idle waves in the last pass of a part); (4, 32, 3) Z < 8: four query
groups per workgroup, P = 1; (2, 64, 64) the borrowed region holds one part only; (1, 48, 16) one signal: the flag is a no-op;
(6, 48, 24) at (64, 2) and (128, 1): P = 2.
Short last parts -- what the unshared kernel never has (there ZS <= Z gives every wave a latent): (16, 33, 65) P = 8, parts of 9, the
last part holds 2 latents, so six of its waves reach the combine at m = -inf; (6, 40, 33) P = 4, parts of 9, the last holds 6;
(17, 33, 129) P = 16, parts of 9: part 14 holds 3 latents and part 15 NONE (15 x 9 > 129: with P >= 16 a whole part can be empty),
so a whole workgroup stores m* = -inf, L = C = 0, Y = 0 and the merge skips it.

That the flagged forward really took the shared path is read off the workspace: filled with 0xFF before the call, it must hold exactly
P N (HD + 3 H) more overwritten words than after the call without the flag (the parts in the borrowed d ybar | delta region)."""
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

IL = importlib.import_module("enf_pde_amd.fitting.inner_loop")      # (the package exports the function under the module's name)

pytestmark = pytest.mark.gpu

SHARED, DET = _lib.ENF_FIT_SHARED_LATENTS, _lib.ENF_FIT_DETERMINISTIC
#        B   N   Z    D   H  (runs shared, P)
CASES = [(5, 40, 9, 128, 2, (1, 1)),
         (16, 33, 64, 128, 2, (1, 8)),
         (3, 100, 70, 128, 2, (1, 2)),
         (4, 32, 3, 128, 2, (1, 1)),
         (2, 64, 64, 128, 2, (1, 1)),
         (1, 48, 16, 128, 2, (0, 1)),
         (6, 48, 24, 64, 2, (1, 2)),
         (6, 48, 24, 128, 1, (1, 2)),
         (16, 33, 65, 128, 2, (1, 8)),
         (6, 40, 33, 128, 2, (1, 4)),
         (17, 33, 129, 128, 2, (1, 16))]
_REF = {}


def _case(B, N, Z, D, H, O=2, seed=71, C=12, freq=(0.3, 0.6)):
    """weights and inputs, once per session: one signal's latents and points (fp32-rounded), per-signal targets and weights"""
    key = (B, N, Z, D, H, O, seed, C, freq)
    if key not in _REF:
        cfg = make_cfg("rel_pos_periodic", D=D, H=H, C=C, O=O, freq=freq)
        prm = R.init_params(seed, cfg, jitter=0.1)
        f32 = lambda v: np.asarray(v, dtype=np.float32).astype(np.float64)
        x, p, a, s = (f32(v[:1]) for v in make_inputs(cfg, 1, N, Z, seed + 1))
        rng = np.random.default_rng(seed + 2)
        y = f32(rng.standard_normal((B, N, O)))
        w, cw = f32(rng.uniform(0.2, 2, (B, N))), f32(rng.uniform(0.2, 2, (B, N, O)))
        _REF[key] = NS(cfg=cfg, prm=prm, x=x[0], p=np.repeat(p, B, 0), a=np.repeat(a, B, 0), s=np.repeat(s, B, 0), y=y, w=w, cw=cw,
                       shape=(B, N, Z))
    return _REF[key]


def _t(cuda):
    return lambda v: torch.tensor(np.asarray(v), dtype=torch.float32, device=cuda)


def _ptr(v):
    return ctypes.c_void_p(v.data_ptr()) if v is not None else None


def _dev(cuda, nef, params, c, flags=0):
    B, N, Z = c.shape
    lib = _lib.load()
    t = _t(cuda)
    desc = nef._desc(B, N, Z)
    nbytes = int(lib.enf_workspace_bytes_ex(ctypes.byref(desc), flags & DET))
    return NS(lib=lib, desc=desc, nbytes=nbytes, ws=torch.full((nbytes,), 255, device=cuda, dtype=torch.uint8), packed=nef.pack(params),
              x=t(c.x), p=t(c.p), a=t(c.a), s=t(c.s), st=ctypes.c_void_p(torch.cuda.current_stream(cuda).cuda_stream))


def _forward(cuda, nef, params, c, shared):
    """enf_forward_stages on caller-owned, NaN-filled ybar and lse; x_bstride = 0"""
    B, N, Z = c.shape
    v = _dev(cuda, nef, params, c)
    HD, H = nef._Hp * nef._Dp, nef._Hp
    out = torch.full((B, N, nef.num_out), float("nan"), device=cuda)
    ybar, lse = torch.full((B, N, HD), float("nan"), device=cuda), torch.full((B, N, H), float("nan"), device=cuda)
    _lib.launch(cuda, v.lib.enf_forward_stages, ctypes.byref(v.desc), _ptr(v.x), 0, _ptr(v.p), _ptr(v.a), _ptr(v.s), _ptr(v.packed), _ptr(out),
                _ptr(ybar), _ptr(lse), _ptr(v.ws), v.nbytes, 15 | (_lib.ENF_STAGE_SHARED_LATENTS if shared else 0), v.st)
    torch.cuda.synchronize()
    written = int((v.ws.view(torch.int32) != -1).sum())          # words of the 0xFF-filled workspace the call overwrote
    return NS(out=out, ybar=ybar, lse=lse, written=written)


def _dev_rel(got, ref):
    return float((got.double() - ref.double()).abs().max() / ref.double().abs().max())


@pytest.mark.parametrize("precision", ["f32", "bf16"])
@pytest.mark.parametrize("B,N,Z,D,H,parts", CASES)
def test_forward_flagged_against_unflagged(cuda, B, N, Z, D, H, parts, precision):
    c = _case(B, N, Z, D, H)
    nef = build_nef(c.cfg, precision)
    nef.pair_variants = ("latent_split", "auto")
    params = nef.load_params(c.prm, device=cuda)
    n = ctypes.c_int32(0)
    assert (_lib.load().enf_shared_forward_parts(ctypes.byref(nef._desc(B, N, Z)), ctypes.byref(n)), n.value) == parts
    plain, flagged = _forward(cuda, nef, params, c, False), _forward(cuda, nef, params, c, True)
    devs = {k: _dev_rel(getattr(flagged, k), getattr(plain, k)) for k in ("ybar", "lse", "out")}
    print("shared forward", (B, N, Z, D, H), precision, "parts", parts, "max|flagged - plain| / max|plain|", devs)
    # the launch, not only the query: the parts' slots (no stored value has the fill's bit pattern, a NaN with every bit set)
    assert flagged.written - plain.written == (parts[1] * N * (H * D + 3 * H) if parts[0] else 0), (flagged.written, plain.written)
    for k in ("ybar", "lse", "out"):
        got = getattr(flagged, k)
        assert bool(torch.isfinite(got).all()), k
        assert bool((got == got[:1]).all()), k                      # every signal's rows are signal 0's, bit for bit
        assert devs[k] < TOL[precision], (k, devs)
    if B == 1:                                                      # no-op: the ordinary sequence
        assert all(torch.equal(getattr(flagged, k), getattr(plain, k)) for k in ("ybar", "lse", "out"))


def _fit(cuda, nef, params, c, kind, flags, grad_scale=None):
    """one raw fit step: kind "w" (per-point weights), "cw" (per-channel weights), "e" (unweighted, with the error outputs)"""
    B, N, Z = c.shape
    v = _dev(cuda, nef, params, c, flags)
    t = _t(cuda)
    y = t(c.y)
    loss = torch.zeros(1, device=cuda)
    dp, da, ds = (torch.full_like(g, float("nan")) for g in (v.p, v.a, v.s))
    head = (ctypes.byref(v.desc), _ptr(v.x), 0, _ptr(v.p), _ptr(v.a), _ptr(v.s), _ptr(v.packed), _ptr(y),
            float(B if grad_scale is None else grad_scale), _ptr(loss), _ptr(dp), _ptr(da), _ptr(ds), _ptr(v.ws), v.nbytes)
    if kind == "w":
        w = t(c.w)
        _lib.launch(cuda, v.lib.enf_fit_step_w, *head, _ptr(w), flags, v.st)
    elif kind == "cw":
        cw = t(c.cw)
        _lib.launch(cuda, v.lib.enf_fit_step_cw, *head, _ptr(cw), flags, v.st)
    else:
        err, lb = torch.empty((B, N), device=cuda), torch.empty((B,), device=cuda)
        _lib.launch(cuda, v.lib.enf_fit_step_e, *head, None, None, _ptr(err), _ptr(lb), flags, v.st)
    torch.cuda.synchronize()
    return NS(loss=loss, dp=dp, da=da, ds=ds)


@pytest.mark.parametrize("precision", ["f32", "bf16"])
@pytest.mark.parametrize("B,N,Z", [(5, 40, 9), (16, 33, 64), (3, 100, 70), (16, 33, 65), (6, 40, 33), (17, 33, 129)])
def test_fit_step_flagged_against_unflagged(cuda, B, N, Z, precision):
    """enf_fit_step_w / _cw / _e in deterministic mode (no float atomics blur the comparison)"""
    c = _case(B, N, Z, 128, 2)
    nef = build_nef(c.cfg, precision)
    nef.pair_variants = ("latent_split", "auto")
    params = nef.load_params(c.prm, device=cuda)
    for kind in ("w", "cw", "e"):
        plain, flagged = _fit(cuda, nef, params, c, kind, DET), _fit(cuda, nef, params, c, kind, DET | SHARED)
        devs = {k: _dev_rel(getattr(flagged, k), getattr(plain, k)) for k in ("loss", "dp", "da", "ds")}
        print("shared fit step", (B, N, Z), precision, kind, devs)
        assert all(bool(torch.isfinite(getattr(flagged, k)).all()) for k in devs)
        assert devs["loss"] < TOL[precision], (kind, devs)
        for k in ("dp", "da", "ds"):
            assert devs[k] < 20 * TOL[precision], (kind, k, devs)


@pytest.mark.parametrize("precision", ["f32", "bf16"])
def test_fit_step_flagged_against_the_oracle(cuda, precision):
    """(B, N, Z) = (5, 40, 9): the flagged step's loss and latent gradients against fp64 autograd of the oracle, with the tolerances of
    tests/test_gpu_backward.py (relative L2 per gradient tensor) and the forward tolerance on the loss.  Those tolerances are stated for
    that file's decoders, so this comparison runs on one of them -- test_backward_invariants' rel_pos_periodic configuration (latent_dim
    16, three outputs, frequencies (0.5, 1.0), seed 0) at Z = 9 -- not on this file's other configuration, where the bf16 pose gradient
    of the step WITHOUT the flag already misses that file's bound.  The step without the flag is measured beside the flagged one."""
    B, N, Z = 5, 40, 9
    c = _case(B, N, Z, 128, 2, O=3, seed=0, C=16, freq=(0.5, 1.0))
    tp = T.to_torch(c.prm, torch.float64)
    qp, qa, qs = (torch.tensor(v, requires_grad=True) for v in (c.p, c.a, c.s))
    xb = torch.tensor(np.broadcast_to(c.x[None], (B,) + c.x.shape).copy())
    lref = ((T.nef_apply(tp, c.cfg, xb, qp, qa, qs) - torch.tensor(c.y)) ** 2).mean()
    lref.backward()
    nef = build_nef(c.cfg, precision)
    nef.pair_variants = ("latent_split", "auto")
    params = nef.load_params(c.prm, device=cuda)
    lref = float(lref.detach())
    for flags in (DET, DET | SHARED):                     # (the step without the flag is measured beside it, the flagged one asserted)
        r = _fit(cuda, nef, params, c, "e", flags, grad_scale=1.0)
        el = abs(float(r.loss) - lref) / lref
        errs = {k: rel(g.double().cpu().numpy(), q.grad.numpy()) for k, g, q in (("p", r.dp, qp), ("a", r.da, qa), ("sigma", r.ds, qs))}
        print("fit step against the oracle", precision, "flagged" if flags & SHARED else "plain", "loss", el, errs)
    assert el < TOL[precision], el
    for k, e in errs.items():
        assert np.isfinite(e) and e < GTOL[precision], (k, errs)


@pytest.mark.parametrize("precision", ["f32", "bf16"])
def test_flag_is_a_permission_only_where_the_forward_is_the_z_fold(cuda, precision):
    c = _case(4, 64, 16, 128, 2)
    nef = build_nef(c.cfg, precision)
    nef.pair_variants = ("z_fold", "auto")
    params = nef.load_params(c.prm, device=cuda)
    n = ctypes.c_int32(0)
    assert _lib.load().enf_shared_forward_parts(ctypes.byref(nef._desc(4, 64, 16)), ctypes.byref(n)) == 0
    for kind in ("w", "cw", "e"):
        plain, flagged = _fit(cuda, nef, params, c, kind, DET), _fit(cuda, nef, params, c, kind, DET | SHARED)
        assert all(torch.equal(getattr(flagged, k), getattr(plain, k)) for k in ("loss", "dp", "da", "ds")), kind
    a, b = _forward(cuda, nef, params, c, False), _forward(cuda, nef, params, c, True)
    assert all(torch.equal(getattr(a, k), getattr(b, k)) for k in ("ybar", "lse", "out"))


@pytest.mark.parametrize("noise,det", [(0.0, False), (0.05, False), (0.0, True)])
def test_inner_loop_passes_the_hint_at_step_0_only(cuda, monkeypatch, noise, det):
    """inner_loop on B = 4 signals, an 8 x 8 grid, 32 sampled points, 16 latents, S = 2: the launched flags, and the fitted latents
    against a run with the hint forced off.  The hint is not passed with noise_pos > 0, nor in deterministic mode (which keeps shared
    masks bit-equal to repeated per-signal masks, tests/test_gpu_signal_masks.py): those runs take the one path twice, and in
    deterministic mode must give the same bits."""
    B, side, Ns, Z, S, C = 4, 8, 32, 16, 2, 12
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
    nef.pair_variants = ("latent_split", "auto")
    nef.deterministic = det
    params = nef.load_params(c.prm, device=cuda)
    lib = _lib.load()
    orig = lib.enf_fit_step_w
    flags = []

    class Spy:                                   # records the `flags` argument of every one-call inner step
        def __call__(self, *args):
            flags.append(int(args[-2]))
            return orig(*args)

    def run():
        gen = torch.Generator().manual_seed(9)
        flags.clear()
        loss, fit = IL.inner_loop(nef, params, lat0, lrs, coords, img, masks, noise_pos=noise, generator=gen)
        torch.cuda.synchronize()
        return float(loss), fit, list(flags)
    try:
        lib.enf_fit_step_w = Spy()
        loss, fit, seen = run()
        monkeypatch.setattr(IL, "_shared_kw", lambda *a, **k: {})
        loss_off, fit_off, seen_off = run()
    finally:
        lib.enf_fit_step_w = orig
    assert [f & SHARED for f in seen_off] == [0] * S
    assert [f & SHARED for f in seen] == ([SHARED] + [0] * (S - 1) if not noise and not det else [0] * S)
    devs = {k: _dev_rel(fit[k], fit_off[k]) for k in fit}
    print("inner loop, hint on against off", "noise", noise, "deterministic", det, "loss", loss, loss_off, devs)
    assert abs(loss - loss_off) <= TOL["f32"] * abs(loss_off)
    for k, d in devs.items():
        assert d < 20 * TOL["f32"], (k, devs)
        if det:
            assert torch.equal(fit[k], fit_off[k]), k
