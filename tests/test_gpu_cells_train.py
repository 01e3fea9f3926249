"""Training on cell averages on the GPU (include/enf_hip.h, "Grouped observations"): the gather of sampled cells (enf_fit_inputs_g), the
unfused grouped loss (enf_mse_value_grad_g; nef.cell_mse), the first inner step on shared latents (enf_fit_step_gs), inner_loop_cells,
and cells= in meta_gradients and in both trainers.

Bounds.  The gather copies: equal bits with its torch-op mirror.  d out and err_g of the loss kernel: fp32 rounding of the group sum,
derived in test_grouped_loss_kernel.  Its scalar loss: 1e-5 relative, what tests/test_gpu_weighted_fit.py holds enf_mse_value_grad_w to.
The composed route (apply -> cell_mse -> backward) against the fused step: 1e-5 relative L2 in f32 (tests/test_gpu_cells.py).  The flagged
step against the unflagged one: the bounds of tests/test_gpu_shared_backward.py (tau on the loss, 20 tau on the gradients); against fp64:
the fit-step contract of tests/test_gpu_cells.py (TOL).  The meta-gradient, the trainers: the bounds of tests/test_gpu_trainer.py and
tests/test_gpu_autodec_fit.py, named where they are used.  Every figure is printed before it is asserted."""
import ctypes
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

from oracle import enf_ref_torch as T
from oracle import optim_ref_np as OP
from tests import cells_train_ref as CT
from tests import test_gpu_autodec_fit as AF
from tests.cells_ref import case, cell_loss, poisoned, rel
from tests.helpers import build_nef
from tests.test_gpu_backward import TOL as GRAD_TOL
from tests.test_gpu_cells import LOSS_TOL, PAIRS, TOL, _fit_problem, _fit_reference
from tests.test_gpu_forward import TOL as TAU
from tests.test_gpu_shared_backward import VARIANTS, _case as shared_case, _delta_tail
from tests.test_gpu_trainer import _problem
from enf_pde_amd import _lib
from enf_pde_amd.enf.models import TENSOR_PATHS
from enf_pde_amd.enf.latents.autodecoder_meta import PositionOrientationFeatureAutodecoderMeta
from enf_pde_amd.fitting import cell_mse_torch, cell_quadrature, fit_cell_averages, gather_cell_samples, inner_loop_cells
from enf_pde_amd.fitting import cells as CELLS
from enf_pde_amd.fitting.trainers import MetaSGDPDETrainer, meta_gradients

pytestmark = pytest.mark.gpu

GUARD = 16
U = 2.0 ** -24
DET, SHARED = _lib.ENF_FIT_DETERMINISTIC, _lib.ENF_FIT_SHARED_LATENTS


def _t(cuda):
    return lambda v: torch.tensor(np.asarray(v), dtype=torch.float32, device=cuda)


def _ptr(v):
    return ctypes.c_void_p(v.data_ptr()) if v is not None else None


def _stream(cuda):
    return ctypes.c_void_p(torch.cuda.current_stream(cuda).cuda_stream)


# ---- 1. the gather
def _gather(cuda, G, dx, per_signal, with_q, with_w, O=2, B=3, Z=5, M=30, Ms=11, S1=3):
    """enf_fit_inputs_g on NaN-filled outputs with GUARD floats behind each, against gather_cell_samples: every output bit for bit"""
    rng = np.random.default_rng(100 * G + 10 * dx + per_signal)
    t = _t(cuda)
    x, q, obs, w = t(rng.standard_normal((M * G, dx))), t(rng.uniform(0.1, 1.0, M * G)), t(rng.standard_normal((B, M, O))), t(rng.uniform(0, 2, (B, M)))
    q, w = (q if with_q else None), (w if with_w else None)
    cols = lambda: np.stack([rng.permutation(M)[:Ms] for _ in range(S1)], 1)
    masks = np.stack([cols() for _ in range(B)]) if per_signal else cols()
    if per_signal:
        masks[1, Ms - 4:, :] = -1
        masks[2, 0, 1], masks[0, 3, 2] = M, M + 7
    masks = torch.tensor(masks, device=cuda)
    lat0 = {"p_pos": t(rng.standard_normal((1, Z, 2))), "a": t(rng.standard_normal((1, Z, 6))), "gaussian_window": t(rng.uniform(0.5, 1, (1, Z, 1)))}
    lead = (S1, B, Ms * G) if per_signal else (S1, Ms * G)
    shapes = {"xs": lead + (dx,), "qs": lead, "ys": (S1, B, Ms, O), "ws": (S1, B, Ms), "losses": (S1,), "p_pos": (B, Z, 2), "a": (B, Z, 6),
              "gaussian_window": (B, Z, 1)}
    if not with_q:
        del shapes["qs"]
    if not with_w and not per_signal:
        del shapes["ws"]
    bufs = {k: torch.full((int(np.prod(s)) + GUARD,), float("nan"), device=cuda) for k, s in shapes.items()}
    comps = (_lib.EnfFitComponent * _lib.ENF_SGD_MAX_SEGMENTS)()
    for i, k in enumerate(lat0):
        comps[i] = _lib.EnfFitComponent(lat0[k].data_ptr(), bufs[k].data_ptr(), lat0[k].shape[2], 0)
    _lib.launch(cuda, _lib.load().enf_fit_inputs_g, 3, comps, B, Z, M, Ms, S1, G, dx, O, _ptr(x), _ptr(q), _ptr(obs), _ptr(masks), _ptr(bufs["xs"]),
                _ptr(bufs.get("qs")), _ptr(bufs["ys"]), _ptr(bufs["losses"]), _ptr(w), _ptr(bufs.get("ws")), int(per_signal), _stream(cuda))
    torch.cuda.synchronize()
    xs, qs, ys, ws = gather_cell_samples(x, q, G, obs, masks, w)
    want = {"xs": xs, "qs": qs, "ys": ys, "ws": ws, "losses": torch.zeros(S1, device=cuda), **{k: v.expand(B, -1, -1) for k, v in lat0.items()}}
    for k, s in shapes.items():
        n = int(np.prod(s))
        assert torch.equal(bufs[k][:n].view(s), want[k]), (k, G, dx, per_signal, with_q, with_w)
        assert bool(torch.isnan(bufs[k][n:]).all()), ("guard", k)
    assert bool(torch.isfinite(xs).all()) and (qs is None or bool(torch.isfinite(qs).all()))
    if per_signal:
        assert float(ws[:, 1, Ms - 4:].abs().max()) == 0.0 and float(ys[:, 1, Ms - 4:].abs().max()) == 0.0 and float(ws[1, 2, 0]) == 0.0
    # and the package's own route takes the launch and returns the same tensors
    fused = CELLS._cell_inputs(lat0, x, q, G, obs, masks, w)
    assert fused is not None
    torch.cuda.synchronize()
    for got, k in zip(fused[1:], ("xs", "qs", "ys", "losses", "ws")):
        assert (got is None and want[k] is None) or torch.equal(got, want[k]), k
    assert all(torch.equal(fused[0][k], want[k]) for k in lat0)


@pytest.mark.parametrize("per_signal", [False, True])
@pytest.mark.parametrize("dx", [2, 3])
@pytest.mark.parametrize("G", [1, 2, 4, 8, 16])
def test_gather_of_sampled_cells(cuda, G, dx, per_signal):
    """M = 30, Ms = 11 (Ms G is no multiple of 16), S1 = 3; both mask layouts, per-signal masks holding -1, M and M + 7; with and without
    q and the observation weights; NaN guard bands behind every output"""
    for with_q, with_w in ((True, True), (False, False), (True, False), (False, True)):
        _gather(cuda, G, dx, per_signal, with_q, with_w)


def test_gather_with_seventeen_channels(cuda):
    _gather(cuda, 4, 2, True, True, True, O=17)
    _gather(cuda, 8, 3, False, True, False, O=17)


# ---- 2. the unfused grouped loss
def _mse_g(cuda, out, y, G, q, w, gscale, flags=0, want_dout=True, want_err=True):
    lib = _lib.load()
    B, N, O = out.shape
    M = N // G
    nb = int(lib.enf_mse_scratch_bytes(B * M * O, flags))
    scr = torch.full((max(nb, 1),), 255, device=cuda, dtype=torch.uint8)
    dbuf = torch.full((B * N * O + GUARD,), float("nan"), device=cuda)
    ebuf = torch.full((B * M + GUARD,), float("nan"), device=cuda)
    loss = torch.zeros(1, device=cuda)
    _lib.launch(cuda, lib.enf_mse_value_grad_g, _ptr(out), _ptr(y), B, N, O, G, _ptr(q), _ptr(w), float(gscale), _ptr(dbuf) if want_dout else None,
                _ptr(loss), _ptr(ebuf) if want_err else None, _ptr(scr) if nb else None, nb, flags, _stream(cuda))
    torch.cuda.synchronize()
    assert bool(torch.isnan(dbuf[B * N * O:]).all()) and bool(torch.isnan(ebuf[B * M:]).all())
    return NS(loss=loss, dout=dbuf[:B * N * O].view(B, N, O), err=ebuf[:B * M].view(B, M))


@pytest.mark.parametrize("G,N", PAIRS)
def test_grouped_loss_kernel(cuda, G, N):
    """enf_mse_value_grad_g, O = 2, against fp64 on the fp32 inputs.  With u = 2^-24 and S = sum_k |q out| + |target|: the G products and
    the tree of G - 1 additions (depth log2 G) put at most (1 + log2 G) u sum|q out| <= G u S on the group sum; the subtraction adds u S;
    the three products w dd, q (w dd), (..) gs add 3 u |dd| <= 3 u S: (G + 4) u S times the factors |q w gs| on d out, gs being the fp32
    number the kernel multiplies with.  err_g = w sum_o dd^2 in the manner of ebound (tests/test_gpu_cells.py): eps = (G + 4) u S on dd
    gives w sum_o (2 |dd| eps + eps^2), which also covers the O + 1 roundings of the products and of the sum over o ((O + 1) u dd^2 <=
    3 u |dd| S at O = 2, against the 2 * 3 u |dd| S that eps holds beyond the G + 1 roundings of dd itself)."""
    c = case("rel_pos_periodic", G, N)
    B, M, O, gsc = 3, c.M, c.O, 3.0
    f32 = lambda v: np.asarray(v, dtype=np.float32).astype(np.float64)
    out64 = f32(np.random.default_rng(G).standard_normal((B, N, O)))
    t = _t(cuda)
    out, q, w, y_bad, y_clean = t(out64), t(c.q), t(c.w), t(poisoned(c)), t(c.y)
    v = c.q[..., None] * out64
    obs = v.reshape(B, M, G, O).sum(2)
    S = np.abs(v).reshape(B, M, G, O).sum(2) + np.abs(c.y)
    live = (c.w > 0)[..., None]
    dd = np.where(live, obs - c.y, 0.0)
    inv_n = np.float32(1.0) / (np.float32(B) * np.float32(M) * np.float32(O))
    gs = float(np.float32(2.0) * inv_n * np.float32(gsc))
    fac = c.q.reshape(B, M, G, 1) * (c.w[..., None, None] * gs)                                   # (B, M, G, 1): q w gs
    ref_dout = (fac * dd[:, :, None, :]).reshape(B, N, O)
    bound_dout = (np.abs(fac) * ((G + 4) * U * np.where(live, S, 0.0))[:, :, None, :]).reshape(B, N, O)
    ref_err = c.w * (dd * dd).sum(-1)
    eps = (G + 4) * U * S
    bound_err = c.w * (2 * np.abs(dd) * eps + eps * eps).sum(-1)
    ref_loss = float(ref_err.sum() / (B * M * O))
    runs = [_mse_g(cuda, out, y_bad, G, q, w, gsc, flags) for flags in (0, DET, DET)]
    for r in runs:
        d_dout, d_err = np.abs(r.dout.double().cpu().numpy() - ref_dout), np.abs(r.err.double().cpu().numpy() - ref_err)
        el = abs(float(r.loss) - ref_loss) / ref_loss
        print(f"grouped loss G={G} N={N}: d out / bound {float((d_dout / np.maximum(bound_dout, 1e-300))[bound_dout > 0].max()):.2e} "
              f"err_g / bound {float((d_err / np.maximum(bound_err, 1e-300))[bound_err > 0].max()):.2e} loss {el:.2e}")
        assert (d_dout <= bound_dout).all() and (d_err <= bound_err).all()
        assert el < 1e-5
        assert bool(torch.isfinite(r.dout).all()) and bool(torch.isfinite(r.err).all())
        gone = torch.tensor(c.w == 0, device=cuda)
        assert bool((r.err[gone] == 0).all()) and bool((r.dout.view(B, M, G, O)[gone] == 0).all())
    assert all(torch.equal(runs[0].dout, r.dout) and torch.equal(runs[0].err, r.err) for r in runs[1:])
    assert torch.equal(runs[1].loss, runs[2].loss)
    clean = _mse_g(cuda, out, y_clean, G, q, w, gsc, DET)                     # what lies under a zero weight changes no bit
    assert torch.equal(clean.loss, runs[1].loss) and torch.equal(clean.dout, runs[1].dout) and torch.equal(clean.err, runs[1].err)
    only = _mse_g(cuda, out, y_bad, G, q, w, gsc, DET, want_dout=False, want_err=False)
    assert torch.equal(only.loss, runs[1].loss) and bool(torch.isnan(only.dout).all()) and bool(torch.isnan(only.err).all())
    # NULL factors are 1 / G, NULL weights 1
    plain = _mse_g(cuda, out, y_clean, G, None, None, gsc, DET)
    ones = _mse_g(cuda, out, y_clean, G, torch.full((B, N), 1.0 / G, device=cuda), torch.ones(B, M, device=cuda), gsc, DET)
    assert torch.equal(plain.loss, ones.loss) and torch.equal(plain.dout, ones.dout) and torch.equal(plain.err, ones.err)
    # nef.cell_mse: the kernel's loss, and out.grad is its d out at grad_scale 1; the torch-op mirror agrees to rounding
    nef = build_nef(c.cfg, "f32")
    nef.deterministic = True
    o = out.clone().requires_grad_(True)
    loss = nef.cell_mse(o, y_bad, G, q, w)
    loss.backward()
    one = _mse_g(cuda, out, y_bad, G, q, w, 1.0, DET)
    assert loss.shape == () and torch.equal(loss.detach().reshape(1), one.loss) and torch.equal(o.grad, one.dout)
    o2 = out.clone().requires_grad_(True)
    mirror = cell_mse_torch(o2, y_bad, G, q, w)
    mirror.backward()
    assert abs(float(mirror.detach()) - float(loss.detach())) <= 1e-5 * float(loss.detach()) and rel(o2.grad.cpu().numpy(), o.grad.cpu().numpy()) <= 1e-6
    with pytest.raises(_lib.EnfError):
        nef.cell_mse(out.cpu(), y_bad.cpu(), G)


@pytest.mark.parametrize("G,N", PAIRS)
def test_composed_route_against_the_fused_step(cuda, G, N):
    """apply -> nef.cell_mse -> backward to the latents against nef.mse_value_and_cell_grads at the same inputs: 1e-5 relative L2, f32"""
    c = case("latitude_periodic", G, N)
    nef = build_nef(c.cfg, "f32")
    params = nef.load_params(c.prm, device=cuda)
    t = _t(cuda)
    x, q, w, y = t(c.x), t(c.q), t(c.w), t(poisoned(c))
    fused = nef.mse_value_and_cell_grads(params, x, t(c.p), t(c.a), t(c.s), y, G, qweight=q, obs_weight=w, grad_scale=c.gs)
    leaves = [t(v).requires_grad_(True) for v in (c.p, c.a, c.s)]
    loss = nef.cell_mse(nef.apply(params, x, *leaves), y, G, q, w)
    (loss * c.gs).backward()
    torch.cuda.synchronize()
    errs = [rel(g.cpu().numpy(), l.grad.cpu().numpy()) for g, l in zip(fused[1:4], leaves)]
    e_loss = abs(float(fused[0]) - float(loss.detach())) / float(loss.detach())
    print(f"composed against fused G={G} N={N}: loss {e_loss:.2e} dp {errs[0]:.2e} da {errs[1]:.2e} dsigma {errs[2]:.2e}")
    assert e_loss <= 1e-5 and all(e <= 1e-5 for e in errs), (e_loss, errs)


# ---- 3. enf_fit_step_gs
def _cells_of(c, G, O):
    """the shared-latent case of tests/test_gpu_shared_backward.py as cells: the first M targets and weights, factors q (N,) for all"""
    B, N, Z = c.shape
    M = N // G
    rng = np.random.default_rng(G)
    q = np.asarray(rng.uniform(0.2, 2.0, N) / G, dtype=np.float32).astype(np.float64)
    return NS(M=M, q=np.repeat(q[None], B, 0), y=c.y[:, :M], w=c.w[:, :M])


def _step(cuda, nef, params, c, g, G, flags, fn="enf_fit_step_gs", err=False, poison=255, grad_scale=None):
    B, N, Z = c.shape
    lib = _lib.load()
    t = _t(cuda)
    desc = nef._desc(B, N, Z)
    nbytes = int(lib.enf_workspace_bytes_ex(ctypes.byref(desc), flags & DET))
    ws = torch.full((nbytes,), poison, device=cuda, dtype=torch.uint8)
    x, p, a, s, y, q, w = t(c.x), t(c.p), t(c.a), t(c.s), t(g.y), t(g.q), t(g.w)
    packed = nef.pack(params)
    loss = torch.zeros(1, device=cuda)
    dp, da, ds = (torch.full_like(v, float("nan")) for v in (p, a, s))
    e = torch.full((B, g.M), float("nan"), device=cuda) if err else None
    lb = torch.full((B,), float("nan"), device=cuda) if err else None
    _lib.launch(cuda, getattr(lib, fn), ctypes.byref(desc), _ptr(x), 0, _ptr(p), _ptr(a), _ptr(s), _ptr(packed), _ptr(y), G, _ptr(q), _ptr(w),
                float(B if grad_scale is None else grad_scale), _ptr(loss), _ptr(dp), _ptr(da), _ptr(ds), _ptr(e), _ptr(lb), _ptr(ws), nbytes, flags,
                _stream(cuda))
    torch.cuda.synchronize()
    return NS(loss=loss, dp=dp, da=da, ds=ds, err=e, loss_b=lb, ws=ws, applies=int(lib.enf_shared_backward_applies(ctypes.byref(desc), flags)))


def _dev_rel(got, ref):
    return float((got.double() - ref.double()).abs().max() / ref.double().abs().max())


def _same(u, v, names=("loss", "dp", "da", "ds")):
    return [n for n in names if not torch.equal(getattr(u, n), getattr(v, n))]


_ORACLE = {}


def _oracle_step(c, g, G):
    key = (c.shape, G, g.y.shape[-1])
    if key not in _ORACLE:
        B = c.shape[0]
        _ORACLE[key] = cell_loss(c.cfg, c.prm, np.repeat(c.x[None], B, 0), c.p, c.a, c.s, g.y, G, g.q, g.w, float(B))
    return _ORACLE[key]


@pytest.mark.parametrize("precision", ["f32", "bf16"])
@pytest.mark.parametrize("G", [4, 8])
def test_flag_clear_is_the_grouped_step(cuda, G, precision):
    """under ENF_FIT_DETERMINISTIC: loss, gradients, err_g and loss_b of enf_fit_step_gs(flags without the permission) are
    enf_fit_step_g's bits; B = 1 with the permission is the call without it, bit for bit"""
    c = shared_case(5, 40, 9, 128, 2, O=2)
    g = _cells_of(c, G, 2)
    nef = build_nef(c.cfg, precision)
    nef.pair_variants = VARIANTS
    params = nef.load_params(c.prm, device=cuda)
    old, new = _step(cuda, nef, params, c, g, G, DET, "enf_fit_step_g", err=True), _step(cuda, nef, params, c, g, G, DET, err=True, poison=0)
    assert _same(old, new, ("loss", "dp", "da", "ds", "err", "loss_b")) == [] and bool(torch.isfinite(new.dp).all())
    c1 = shared_case(1, 40, 9, 128, 2, O=1)
    g1 = _cells_of(c1, G, 1)
    nef1 = build_nef(c1.cfg, precision)
    nef1.pair_variants = VARIANTS
    params1 = nef1.load_params(c1.prm, device=cuda)
    plain, flagged = _step(cuda, nef1, params1, c1, g1, G, DET), _step(cuda, nef1, params1, c1, g1, G, DET | SHARED, poison=0)
    assert _same(plain, flagged) == [] and flagged.applies == 0


@pytest.mark.parametrize("precision", ["f32", "bf16"])
@pytest.mark.parametrize("G", [4, 8])
@pytest.mark.parametrize("O", [1, 2])
def test_flag_set_against_unflagged_and_the_oracle(cuda, O, G, precision):
    """(B, N, Z) = (5, 40, 9), pair_variants as tests/test_gpu_shared_backward.py so that the z-fold backward runs.  O = 1: the shared
    backward applies -- the query says so, and the delta rows of signals 1.. still hold the fill, which only the ordinary backward
    overwrites.  O = 2: only the forward is shared.  Against the unflagged call: tau on the loss, 20 tau on the gradients.  Against fp64:
    the fit-step contract.  The flagged call on a 0x00-filled and on a 0xFF-filled workspace: equal results (at N = 40 the shared
    backward has one query split, so every element of the gradient table has one adder; with O = 2 in deterministic mode)."""
    B, N, Z = 5, 40, 9
    c = shared_case(B, N, Z, 128, 2, O=O)
    g = _cells_of(c, G, O)
    nef = build_nef(c.cfg, precision)
    nef.pair_variants = VARIANTS
    params = nef.load_params(c.prm, device=cuda)
    plain, flagged = _step(cuda, nef, params, c, g, G, 0), _step(cuda, nef, params, c, g, G, SHARED)
    tail = _delta_tail(nef, flagged.ws, B, N, Z)
    devs = {k: _dev_rel(getattr(flagged, k), getattr(plain, k)) for k in ("loss", "dp", "da", "ds")}
    ref = _oracle_step(c, g, G)
    e_loss = abs(float(flagged.loss) - ref.loss) / ref.loss
    e_g = [rel(v.cpu().numpy(), r) for v, r in zip((flagged.dp, flagged.da, flagged.ds), ref.g)]
    print(f"enf_fit_step_gs O={O} G={G} {precision}: applies {flagged.applies}, delta words still filled {int((tail == -1).sum())} of {tail.numel()}, "
          f"against unflagged {devs}, against fp64 loss {e_loss:.2e} grads {e_g}")
    if O == 1:
        assert flagged.applies == 1 and plain.applies == 0 and bool((tail == -1).all())
    else:
        assert flagged.applies == 0 and not bool((tail == -1).any())
    assert not bool((_delta_tail(nef, plain.ws, B, N, Z) == -1).any())
    assert all(bool(torch.isfinite(getattr(flagged, k)).all()) for k in devs)
    assert devs["loss"] < TAU[precision] and all(devs[k] < 20 * TAU[precision] for k in ("dp", "da", "ds")), devs
    assert e_loss <= TOL[precision][0] and all(e <= TOL[precision][1] for e in e_g), (e_loss, e_g)
    flags = SHARED if O == 1 else SHARED | DET
    zero, ones = _step(cuda, nef, params, c, g, G, flags, poison=0), _step(cuda, nef, params, c, g, G, flags, poison=255)
    assert _same(zero, ones) == []
    # err_g asked for: the ordinary grouped tail behind the shared forward, err_g and loss_b as the unflagged call forms them
    with_err, base = _step(cuda, nef, params, c, g, G, SHARED, err=True), _step(cuda, nef, params, c, g, G, DET, err=True)
    d_err = _dev_rel(with_err.err, base.err)
    print(f"  err_g behind the shared forward against the unflagged call {d_err:.2e}")
    assert d_err < 20 * TAU[precision] and bool(torch.isfinite(with_err.loss_b).all())
    assert not bool((_delta_tail(nef, with_err.ws, B, N, Z) == -1).any())


# ---- 4. the inner loop
def test_inner_loop_cells_equals_fit_cell_averages(cuda):
    """shared masks, the same sampled indices: in deterministic mode (no shared route) inner_loop_cells is fit_cell_averages bit for bit;
    in the default mode step 0 takes the shared route and the two agree to rounding (tau on the loss, 20 tau on the latents)"""
    pb = _fit_problem(cuda, "f32")
    S, Ms, G = 2, 12, 4
    gen = torch.Generator().manual_seed(3)
    idx = torch.stack([torch.randperm(30, generator=gen)[:Ms] for _ in range(S + 1)]).to(cuda)
    masks = idx.t().contiguous()
    args = (pb.nef, pb.params, pb.lat0_t, pb.lrs, pb.xt, pb.qt, G, pb.yt)
    a_loss, a_lat, a_lb = fit_cell_averages(*args, S, obs_weight=pb.wt, sample=idx, per_signal_loss=True)
    b_loss, b_lat, b_lb = inner_loop_cells(*args, masks, obs_weights=pb.wt, per_signal_loss=True)
    torch.cuda.synchronize()
    assert torch.equal(a_loss, b_loss) and torch.equal(a_lb, b_lb) and all(torch.equal(a_lat[k], b_lat[k]) for k in a_lat)
    nef = build_nef(pb.cfg, "f32")                                   # the default mode: the hint is passed at step 0
    assert CELLS._shared_kw(nef, 0, False, 0.0, step="mse_value_and_cell_grads") == {"shared_latents": True}
    c_loss, c_lat = inner_loop_cells(nef, *args[1:], masks, obs_weights=pb.wt)
    torch.cuda.synchronize()
    devs = {k: _dev_rel(c_lat[k], a_lat[k]) for k in ("p_pos", "a")}
    print("inner_loop_cells with the shared first step against fit_cell_averages: loss", float(c_loss), float(a_loss), devs)
    assert abs(float(c_loss) - float(a_loss)) <= TAU["f32"] * float(a_loss) and all(d < 20 * TAU["f32"] for d in devs.values())


@pytest.mark.parametrize("precision", ["f32", "bf16"])
def test_inner_loop_cells_follows_the_reference_loop(cuda, precision):
    """every cell at every step against tests/cells_ref.py: fit_loop in fp64 (the reference of tests/test_gpu_cells.py, computed once):
    every step's loss and the final one within LOSS_TOL, NaN targets under the zero weights"""
    pb = _fit_problem(cuda, precision)
    ref_losses, _ = _fit_reference(pb)
    y = pb.yt.clone()
    y[pb.wt == 0] = float("nan")
    masks = torch.arange(30, device=cuda)[:, None].expand(-1, 4).contiguous()
    loss, lat, loss_b = inner_loop_cells(pb.nef, pb.params, pb.lat0_t, pb.lrs, pb.xt, pb.qt, 4, y, masks, obs_weights=pb.wt, per_signal_loss=True)
    torch.cuda.synchronize()
    got = loss_b.double().mean(1).cpu().numpy()
    print("inner_loop_cells", precision, "losses", got.tolist(), "reference", ref_losses.tolist())
    assert np.all(np.abs(got - ref_losses) <= LOSS_TOL[precision] * ref_losses), (got, ref_losses)
    assert abs(float(loss) - ref_losses[3]) <= LOSS_TOL[precision] * ref_losses[3] and np.all(np.diff(got) < 0)


def test_inner_loop_cells_on_per_signal_masks_with_a_padded_signal(cuda):
    """deterministic mode.  Signal 1 holds 7 cells and 5 entries of -1: the fit equals, bit for bit, the fit in which those entries name a
    cell that signal 1 does not otherwise sample and whose weight is zero -- an observation that does not exist either way; and per-signal
    masks that repeat shared ones give the shared fit's bits."""
    pb = _fit_problem(cuda, "f32")
    S, Ms, G, Bn = 2, 12, 4, 3
    gen = torch.Generator().manual_seed(5)
    masks = torch.stack([torch.stack([torch.randperm(29, generator=gen)[:Ms] for _ in range(S + 1)], 1) for _ in range(Bn)])     # cells 0..28
    padded = masks.clone()
    padded[1, 7:, :] = -1
    named = masks.clone()
    named[1, 7:, :] = 29
    w = pb.wt.clone()
    w[1, 29] = 0.0
    args = (pb.nef, pb.params, pb.lat0_t, pb.lrs, pb.xt, pb.qt, G, pb.yt)
    a = inner_loop_cells(*args, padded.to(cuda), obs_weights=w, per_signal_loss=True)
    b = inner_loop_cells(*args, named.to(cuda), obs_weights=w, per_signal_loss=True)
    torch.cuda.synchronize()
    assert torch.equal(a[0], b[0]) and torch.equal(a[2], b[2]) and all(torch.equal(a[1][k], b[1][k]) for k in a[1])
    assert bool(torch.isfinite(a[2]).all()) and float(a[0]) > 0
    shared = masks[0].to(cuda).contiguous()
    c = inner_loop_cells(*args, shared, obs_weights=w, per_signal_loss=True)
    d = inner_loop_cells(*args, shared[None].expand(Bn, -1, -1).contiguous(), obs_weights=w, per_signal_loss=True)
    torch.cuda.synchronize()
    assert torch.equal(c[0], d[0]) and torch.equal(c[2], d[2]) and all(torch.equal(c[1][k], d[1][k]) for k in c[1])


# ---- 5. the meta-gradient
def _tensor_errs(got, want):
    want = [b if isinstance(b, np.ndarray) else b.cpu().numpy() for b in want]
    gmax = max(np.linalg.norm(x) for x in want)
    out = []
    for path, a, b in zip(TENSOR_PATHS, got, want):
        nb = np.linalg.norm(b)
        out.append(("/".join(path[-3:]), np.linalg.norm(a.cpu().numpy() - b) / (nb if nb > 1e-3 * gmax else gmax)))
    return out


def test_meta_gradient_on_cells_matches_exact_second_order(cuda):
    """tests/test_gpu_trainer.py's problem (B = 8, Z = 16) as 8 x 8 cells on [-1, 1]^2 with 2 x 2 Gauss points, 16 sampled cells = 64 rows
    per step, S = 2, per-observation weights: every weight tensor, the latent initialisation and the inner rates against double backward
    of tests/cells_train_ref.py in fp64 at that file's bounds -- 2e-3 for the weights, `a` and the rates, 5e-3 for p_pos."""
    cfg, prm, x, q, G, obs, lat0, lrs, masks = CT.cell_problem(_problem(B=8, Ns=64, Z=16), side=8, k=2, Ms=16)
    w = np.asarray(np.random.default_rng(6).uniform(0.5, 1.5, obs.shape[:2]), dtype=np.float32).astype(np.float64)
    w[2, int(masks[3, 1])] = 0.0
    loss_r, gw_r, gl_r, gr_r = CT.meta_grads(prm, cfg, lat0, lrs, x, q, G, obs, masks, w)
    nef = build_nef(cfg, "f32")
    params = nef.load_params(prm, device=cuda)
    t = _t(cuda)
    y = t(obs)
    y[2, int(masks[3, 1])] = float("nan")
    loss, g = meta_gradients(nef, params, {k: t(v) for k, v in lat0.items()}, {k: t(v) for k, v in lrs.items()}, None, y,
                             torch.tensor(masks, device=cuda), second_order="fd", weights=t(w), normalize=False, cells=(t(x), t(q), G))
    errs = _tensor_errs(g["nef"], gw_r)
    e_lat = {k: rel(g["autodecoder"][k].cpu().numpy(), gl_r[k]) for k in ("a", "p_pos")}
    e_lr = {k: rel(g["meta_sgd_lrs"][k].cpu().numpy(), gr_r[k]) for k in ("a", "p_pos")}
    print("meta-gradient on cells: loss", float(loss), loss_r, "worst weight tensor", max(errs, key=lambda e: e[1]), "lat0", e_lat, "lrs", e_lr)
    assert abs(float(loss) - loss_r) < 1e-5 * max(1.0, abs(loss_r))
    assert not [e for e in errs if not e[1] < 2e-3], [e for e in errs if not e[1] < 2e-3]
    assert e_lat["a"] < 2e-3 and e_lat["p_pos"] < 5e-3 and all(e < 2e-3 for e in e_lr.values())
    assert all(bool(torch.isfinite(v).all()) for v in g["nef"])


def test_meta_gradient_on_cells_of_one_point_is_the_point_meta_gradient(cuda):
    """cells with G = 1 and q = None on the point problem against meta_gradients without cells: 1e-5 relative per tensor"""
    cfg, prm, coords, img, lat0, lrs, masks = _problem(B=8, Ns=64, Z=16)
    nef = build_nef(cfg, "f32")
    params = nef.load_params(prm, device=cuda)
    t = _t(cuda)
    args = (nef, params, {k: t(v) for k, v in lat0.items()}, {k: t(v) for k, v in lrs.items()}, t(coords), t(img), torch.tensor(masks, device=cuda))
    loss_p, gp = meta_gradients(*args, second_order="fd")
    loss_c, gc = meta_gradients(*args, second_order="fd", cells=(t(coords), None, 1))
    errs = _tensor_errs(gc["nef"], gp["nef"])
    e_lat = {k: rel(gc["autodecoder"][k].cpu().numpy(), gp["autodecoder"][k].cpu().numpy()) for k in ("a", "p_pos")}
    e_lr = {k: rel(gc["meta_sgd_lrs"][k].cpu().numpy(), gp["meta_sgd_lrs"][k].cpu().numpy()) for k in ("a", "p_pos")}
    print("G = 1 cells against points: loss", float(loss_c), float(loss_p), "worst weight tensor", max(errs, key=lambda e: e[1]), e_lat, e_lr)
    assert abs(float(loss_c) - float(loss_p)) <= 1e-5 * float(loss_p)
    assert all(e[1] <= 1e-5 for e in errs), [e for e in errs if e[1] > 1e-5]
    assert all(e <= 1e-5 for e in e_lat.values()) and all(e <= 1e-5 for e in e_lr.values())


# ---- 6. the trainers
def test_meta_trainer_step_on_cells_follows_optax_rules(cuda):
    """tests/test_gpu_trainer.py: test_nef_train_step_follows_optax_rules with cells=: the step's loss is meta_gradients', the parameters
    move by clip_by_global_norm + AdamW (nef) and Adam + clip (rates) applied to those gradients; a step that draws its own masks samples
    max_num_sampled_points // G cells; the loss goes down over steps"""
    cfg, prm, x, q, G, obs, lat0, lrs, masks = CT.cell_problem(_problem(seed=3), side=8, k=2, Ms=8)
    nef = build_nef(cfg, "f32")
    conf = NS(optimizer=NS(learning_rate_enf=1e-3, learning_rate_codes=1e-3), meta=NS(learning_rate_meta_sgd=1e-2,
              num_inner_steps=2, inner_learning_rate_p=0.5, inner_learning_rate_a=2.0, inner_learning_rate_window=0.0,
              noise_pos_inner_loop=0.0), nef=NS(optimize_gaussian_window=False), training=NS(max_num_sampled_points=32))
    t = _t(cuda)
    cells = (t(x), t(q), G)
    ad = PositionOrientationFeatureAutodecoderMeta(1, 9, 8, 2, 0, gaussian_window_size=-1)
    tr = MetaSGDPDETrainer(conf, nef, ad, t(x), seed=0, second_order="fd")
    state = tr.init_train_state(nef.load_params(prm, device=cuda))
    batch, mk = t(obs), torch.tensor(masks, device=cuda)
    w0 = [w.clone() for w in nef.param_tensors(state.params["nef"])]
    lat0_t = {k: v.clone() for k, v in tr._latents0(state).items()}
    lrs0 = {k: v.clone() for k, v in state.params["meta_sgd_lrs"].items()}
    loss0, g = meta_gradients(nef, state.params["nef"], lat0_t, lrs0, None, batch, mk, second_order="fd", cells=cells)
    loss, new = tr.nef_train_step(state, batch, masks=mk, cells=cells)
    assert abs(float(loss) - float(loss0)) < 1e-6
    gn = [v.cpu().numpy().astype(np.float64) for v in g["nef"]]
    ref_w, _ = OP.adam_step([w.cpu().numpy().astype(np.float64) for w in w0], OP.clip_by_global_norm(gn, 1.0), OP.init_state(gn), lr=1e-3,
                            weight_decay=1e-4)
    for a, b in zip(nef.param_tensors(new.params["nef"]), ref_w):
        np.testing.assert_allclose(a.cpu().numpy(), b, rtol=2e-4, atol=2e-6)
    for k in lrs0:
        ref, _ = OP.adam_step([lrs0[k].cpu().numpy().astype(np.float64)], [g["meta_sgd_lrs"][k].cpu().numpy().astype(np.float64)],
                              OP.init_state([lrs0[k].cpu().numpy()]), lr=1e-2)
        np.testing.assert_allclose(new.params["meta_sgd_lrs"][k].cpu().numpy(), np.clip(ref[0], 1e-6, 10), rtol=2e-4, atol=1e-6)
    losses, st = [float(loss)], new
    for _ in range(6):
        l, st = tr.nef_train_step(st, batch, masks=mk, cells=cells)
        losses.append(float(l))
    assert losses[-1] < losses[0], losses
    drawn, _ = tr._draw_masks(st, 64, None, group=G)
    assert tuple(drawn.shape) == (32 // G, 3) and int(drawn.max()) < 64
    l, _ = tr.nef_train_step(st, batch, cells=cells, weights=torch.ones(64, device=cuda))
    assert np.isfinite(float(l))
    with pytest.raises(ValueError, match="channel_weights"):
        tr.nef_train_step(st, batch, cells=cells, channel_weights=torch.ones(64, 1, device=cuda))


def _autodec_cells(cuda):
    """tests/test_gpu_autodec_fit.py's problem on 8 x 8 cells of 2 x 2 Gauss points: max_num_sampled_points = 37 gives 9 cells, drawn as
    the step draws them; per-observation weights with exact zeros, taken as they are"""
    pb = AF._problem("rel_pos_periodic")
    x, q = cell_quadrature((-1.0, 1.0, (AF.SIDE, AF.SIDE)), 2)
    G, M = 4, AF.SIDE * AF.SIDE
    obs = torch.tensor(pb.img).reshape(3, M, AF.O)
    w = torch.rand(3, M, generator=torch.Generator().manual_seed(13)) + 0.5
    w[torch.rand(3, M, generator=torch.Generator().manual_seed(14)) < 0.25] = 0.0
    pick = torch.randperm(M, generator=torch.Generator().manual_seed(AF.SEED))[:AF.N_S // G]
    rows = (pick[:, None] * G + torch.arange(G)).reshape(-1)
    n = lambda v: v.double().numpy()
    pose, a, s = (v[AF.IDX].astype(np.float64) for v in (pb.table["p_pos"], pb.table["a"], pb.table["gaussian_window"]))
    ref = cell_loss(pb.cfg, pb.prm, np.repeat(n(x[rows])[None], 3, 0), pose, a, s, n(obs[:, pick]), G, np.repeat(n(q[rows])[None], 3, 0),
                    n(w[:, pick]), 1.0)
    return pb, (x.to(cuda), q.to(cuda), G), obs, w, ref


@pytest.mark.parametrize("precision", ["f32", "bf16"])
def test_autodecoder_fit_latents_step_on_cells(cuda, precision):
    """NonMetaPDETrainer.fit_latents_step(cells=): the loss and the gradient the table update took (read back from its first moments)
    against fp64 autograd of the oracle at the bounds of tests/test_gpu_autodec_fit.py; rows outside the batch stay where they were"""
    pb, cells, obs, w, ref = _autodec_cells(cuda)
    tr, nef_params = AF._trainer(cuda, pb, precision)
    state = AF._state(cuda, tr, nef_params, pb)
    y = obs.clone()
    y[w == 0] = float("nan")
    loss, new, loss_b = tr.fit_latents_step(state, (y.reshape(3, AF.SIDE, AF.SIDE, AF.O).to(cuda), torch.tensor(AF.IDX, device=cuda)),
                                            weights=w.to(cuda), normalize=False, cells=cells, per_signal_loss=True)
    torch.cuda.synchronize()
    el = abs(float(loss) - ref.loss) / ref.loss
    g = AF._own_gradient(new, pb)
    errs = {"p": AF._rel(g["p_pos"][AF.IDX], ref.g[0]), "a": AF._rel(g["a"][AF.IDX], ref.g[1]), "sigma": AF._rel(g["gaussian_window"][AF.IDX], ref.g[2])}
    print(f"fit_latents_step on cells {precision}: loss rel err {el:.2e}, gradient rel errs {errs}")
    assert el < TAU[precision], el
    assert all(np.isfinite(e) and e < GRAD_TOL[precision] for e in errs.values()), errs
    assert np.allclose(loss_b.double().cpu().numpy(), ref.loss_b, rtol=LOSS_TOL[precision], atol=0)        # (tests/test_gpu_cells.py)
    P0, P1 = state.params["autodecoder"]["params"], new.params["autodecoder"]["params"]
    assert all(torch.equal(P1[k][AF.ROWS_OUT], P0[k][AF.ROWS_OUT]) for k in pb.names) and new.step == 1
    with pytest.raises(ValueError, match="channel_weights"):
        tr.fit_latents_step(state, (y.to(cuda), torch.tensor(AF.IDX, device=cuda)), cells=cells, channel_weights=torch.ones(64, AF.O, device=cuda))


def test_autodecoder_train_step_on_cells(cuda):
    """NonMetaPDETrainer.loss_and_grads / nef_train_step(cells=), every cell: the loss and the weight gradients against fp64 autograd of
    the oracle within 1e-3 (tests/test_gpu_trainer.py: test_nonmeta_train_step), the latent rows alike; then steps lower the loss"""
    from enf_pde_amd.fitting.trainers import NonMetaPDETrainer
    from enf_pde_amd.enf.latents.autodecoder import PositionOrientationFeatureAutodecoder
    cfg, prm, x, q, G, obs, _, _, _ = CT.cell_problem(_problem(seed=5, B=3, Z=9), side=8, k=2, Ms=8)
    nef = build_nef(cfg, "f32")
    conf = NS(optimizer=NS(learning_rate_enf=1e-3, learning_rate_codes=1e-2), training=NS(max_num_sampled_points=10 ** 6))
    ad = PositionOrientationFeatureAutodecoder(6, 9, 8, 2, 0, gaussian_window_size=-1)
    t = _t(cuda)
    cells = (t(x), t(q), G)
    tr = NonMetaPDETrainer(conf, nef, ad, t(x), seed=0)
    state = tr.init_train_state(nef.load_params(prm, device=cuda))
    P0 = {k: v.clone() for k, v in state.params["autodecoder"]["params"].items()}
    P0["a"] = P0["a"] + 0.1 * torch.randn(P0["a"].shape, generator=torch.Generator().manual_seed(1)).to(cuda)
    state.params["autodecoder"]["params"] = {k: v.clone() for k, v in P0.items()}
    idx = torch.tensor([4, 0, 2], device=cuda)
    loss, gw, ga = tr.loss_and_grads(state, t(obs), idx, cells=cells)
    tp = T.to_torch(prm, torch.float64, requires_grad=True)
    lat = {k: torch.tensor(v.cpu().numpy().astype(np.float64), requires_grad=True) for k, v in P0.items()}
    out = T.nef_apply(tp, cfg, torch.tensor(x)[None].expand(3, -1, -1), lat["p_pos"][idx.cpu()], lat["a"][idx.cpu()], lat["gaussian_window"][idx.cpu()])
    lref = cell_mse_torch(out, torch.tensor(obs), G, torch.tensor(q)[None].expand(3, -1))
    leaves = [CT._get(tp["params"], p) for p in TENSOR_PATHS]
    g = torch.autograd.grad(lref, leaves + [lat[k] for k in ("p_pos", "a")], allow_unused=True)
    assert abs(float(loss) - float(lref.detach())) < 1e-5 * max(1.0, float(lref.detach()))
    gmax = max(float(v.norm()) for v in g[:len(leaves)] if v is not None)
    for path, a, b in zip(TENSOR_PATHS, gw, g[:len(leaves)]):
        if b is None:
            assert float(a.abs().max()) == 0
            continue
        nb = float(b.norm())
        e = float((a.cpu().double() - b).norm()) / (nb if nb > 1e-3 * gmax else gmax)
        assert e < 1e-3, ("/".join(path), e)
    for k, b in zip(("p_pos", "a"), g[len(leaves):]):
        assert float((ga[k].cpu().double() - b).norm() / b.norm()) < 1e-3, k
        assert float(ga[k][[1, 3, 5]].abs().max()) == 0
    batch = (t(obs), idx)
    l0, new = tr.nef_train_step(state, batch, cells=cells)
    for _ in range(8):
        l, new = tr.nef_train_step(new, batch, cells=cells)
    assert float(l) < float(l0)
    w_before = [v.clone() for v in nef.param_tensors(new.params["nef"])]
    l2, only = tr.nef_train_step_autodec_only(new, batch, cells=cells)
    assert all(torch.equal(u, v) for u, v in zip(w_before, nef.param_tensors(only.params["nef"]))) and np.isfinite(float(l2))
