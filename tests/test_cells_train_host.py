"""Training on cell averages without a GPU (include/enf_hip.h, "Grouped observations": enf_fit_inputs_g, enf_mse_value_grad_g,
enf_fit_step_gs): the torch-op mirrors of the two new kernels against fp64 statements written here, inner_loop_cells on a stand-in decoder
against tests/cells_ref.py: fit_loop, the refusals of the three C calls (every call here fails its checks, so nothing is launched), and
the yardstick of the grouped meta-gradient (tests/cells_train_ref.py) against central differences of its own loss."""
import copy
import importlib
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from enf_pde_amd import _lib
from enf_pde_amd.enf.models import TENSOR_PATHS
from enf_pde_amd.fitting import cell_mse_torch, gather_cell_samples, inner_loop_cells
from enf_pde_amd.fitting import cells as CELLS
from tests import cells_train_ref as CT
from tests.cells_ref import case, cell_loss, fit_loop

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, EUNSUPPORTED, EWORKSPACE = -1, -3, -4
DET, SHARED = _lib.ENF_FIT_DETERMINISTIC, _lib.ENF_FIT_SHARED_LATENTS


# ---- 1. the mirrors
@pytest.mark.parametrize("per_signal", [False, True])
@pytest.mark.parametrize("with_q,with_w", [(True, True), (False, False), (True, False)])
def test_gather_mirror_matches_the_statement(per_signal, with_q, with_w):
    """row i G + k of a sampled set is row m G + k of cell m; ys = obs[b, m]; ws = w[b, m]; an index outside [0, M) gives cell 0's rows,
    zero targets and weight 0 -- element by element in numpy"""
    B, M, Ms, S1, G, dx, O = 3, 9, 5, 3, 4, 2, 2
    rng = np.random.default_rng(5)
    x, q = rng.standard_normal((M * G, dx)), rng.uniform(0.1, 1.0, M * G)
    obs, w = rng.standard_normal((B, M, O)), rng.uniform(0.0, 2.0, (B, M))
    masks = np.stack([rng.permutation(M)[:Ms] for _ in range(S1 * (B if per_signal else 1))], 1)
    masks = masks.reshape(Ms, B, S1).transpose(1, 0, 2).copy() if per_signal else masks
    if per_signal:
        masks[1, 3:, :] = -1
        masks[2, 0, 1] = M
    idx = masks if per_signal else np.repeat(masks[None], B, 0)
    xs = np.zeros((S1, B, Ms * G, dx)); qs = np.zeros((S1, B, Ms * G)); ys = np.zeros((S1, B, Ms, O)); ws = np.zeros((S1, B, Ms))
    for s in range(S1):
        for b in range(B):
            for i in range(Ms):
                m = int(idx[b, i, s])
                ok = 0 <= m < M
                for k in range(G):
                    xs[s, b, i * G + k], qs[s, b, i * G + k] = x[(m if ok else 0) * G + k], q[(m if ok else 0) * G + k]
                if ok:
                    ys[s, b, i], ws[s, b, i] = obs[b, m], (w[b, m] if with_w else 1.0)
    t = torch.tensor
    got = gather_cell_samples(t(x), t(q) if with_q else None, G, t(obs), t(masks), t(w) if with_w else None)
    want_x, want_q = (xs, qs) if per_signal else (xs[:, 0], qs[:, 0])
    assert np.array_equal(got[0].numpy(), want_x)
    assert (got[1] is None) if not with_q else np.array_equal(got[1].numpy(), want_q)
    assert np.array_equal(got[2].numpy(), ys.astype(np.float32))
    if not with_w and not per_signal:
        assert got[3] is None
    else:
        assert np.array_equal(got[3].numpy(), ws.astype(np.float32))
    assert all(v is None or v.is_contiguous() for v in got)


@pytest.mark.parametrize("G,N,with_q,with_w", [(4, 16, True, True), (1, 5, False, True), (16, 32, True, False), (2, 6, False, False)])
def test_loss_mirror_and_its_gradient(G, N, with_q, with_w):
    """cell_mse_torch and its autograd d out against the header's formulas in numpy fp64, NaN / Inf targets under the zero weights"""
    B, O = 3, 2
    M = N // G
    rng = np.random.default_rng(G)
    out, q, y = rng.standard_normal((B, N, O)), rng.uniform(-1.0, 2.0, (B, N)), rng.standard_normal((B, M, O))
    w = rng.uniform(0.2, 2.0, (B, M))
    w[0, 0] = w[2, M - 1] = 0.0
    qn, wn = (q if with_q else np.full((B, N), 1.0 / G)), (w if with_w else np.ones((B, M)))
    obs = (qn[..., None] * out).reshape(B, M, G, O).sum(2)
    dd = np.where((wn > 0)[..., None], obs - y, 0.0)
    loss = (wn[..., None] * dd * dd).sum() / (B * M * O)
    dout = qn[..., None] * np.repeat(2.0 * wn[..., None] * dd / (B * M * O), G, axis=1)
    yp = y.copy()
    if with_w:
        yp[0, 0], yp[2, M - 1] = np.nan, np.inf
    t = torch.tensor
    o = t(out, requires_grad=True)
    got = cell_mse_torch(o, t(yp), G, t(q) if with_q else None, t(w) if with_w else None)
    got.backward()
    assert abs(float(got.detach()) - loss) <= 1e-14 * loss
    assert np.allclose(o.grad.numpy(), dout, rtol=1e-13, atol=1e-16) and bool(torch.isfinite(o.grad).all())
    if with_w:
        assert float(o.grad[0, :G].abs().max()) == 0.0


class _Oracle:
    """A decoder on the fp64 oracle with the grouped calls inner_loop_cells makes; no device.  It names ``shared_latents``."""

    def __init__(self, c):
        self.c, self.cross_attn_invariant, self.hints = c, type("I", (), {"num_z_ori_dims": 0})(), []

    def _loss(self, x, p, a, s, y, G, q, w, grads):
        n = lambda v: None if v is None else v.double().numpy()
        return cell_loss(self.c.cfg, self.c.prm, n(x), n(p), n(a), n(s), n(y), G, n(q), n(w), 1.0, grads=grads)

    def mse_value_and_cell_grads(self, params, x, p, a, window, target, group, qweight=None, obs_weight=None, loss_out=None,
                                 return_errors=False, shared_latents=False):
        self.hints.append(shared_latents)
        r = self._loss(x, p, a, window, target, group, qweight, obs_weight, True)
        loss_out += r.loss
        res = (loss_out,) + tuple(torch.tensor(g) for g in r.g)
        return res + (torch.tensor(r.err_g), torch.tensor(r.loss_b)) if return_errors else res

    def eval_cell_loss(self, params, x, p, a, window, target, group, qweight=None, obs_weight=None, loss_out=None, per_signal=True):
        r = self._loss(x, p, a, window, target, group, qweight, obs_weight, False)
        loss_out += r.loss
        return (torch.tensor(r.loss_b) if per_signal else None), torch.tensor(r.err_g)


def test_inner_loop_cells_reproduces_the_reference_loop(monkeypatch):
    """every cell at every step, in order, on a stand-in decoder that is the oracle: the losses and the fitted latents of
    tests/cells_ref.py: fit_loop (fp64; the loop's loss accumulators are float32, so 1e-6 on the losses, 1e-12 on the latents), the
    per-signal rows, and the shared-latent hint at step 0 only"""
    c = case("rel_pos_periodic", 4, 16)
    S, M = 2, c.M
    lr_p, lr_a = 0.7, np.linspace(1.0, 3.0, c.a.shape[-1])
    monkeypatch.setattr(importlib.import_module("enf_pde_amd.fitting.inner_loop"), "meta_sgd_update", lambda lat, g, lrs, scale: {k: (lat[k] - lrs[k] * (scale * g[k]) if k in g else lat[k]) for k in lat})
    t = torch.tensor
    lat0 = {"p_pos": t(c.p[:1]), "a": t(c.a[:1]), "gaussian_window": t(c.s[:1])}
    lrs = {"p_pos": t([lr_p], dtype=torch.float64), "a": t(lr_a), "gaussian_window": t([0.0], dtype=torch.float64)}
    masks = torch.arange(M)[:, None].expand(-1, S + 1).contiguous()
    ref_losses, ref_lat = fit_loop(c.cfg, c.prm, c.x[0], c.q[0], 4, c.y, c.w, (c.p[:1], c.a[:1], c.s[:1]), (lr_p, lr_a), S)
    nef = _Oracle(c)
    loss, lat, loss_b = inner_loop_cells(nef, None, lat0, lrs, t(c.x[0]), t(c.q[0]), 4, t(c.y), masks, obs_weights=t(c.w), per_signal_loss=True)
    assert nef.hints == [True, False]
    assert abs(float(loss) - ref_losses[S]) <= 1e-6 * ref_losses[S]
    assert np.allclose(loss_b.double().mean(1).numpy(), ref_losses, rtol=1e-6, atol=0)
    for k, r in zip(("p_pos", "a", "gaussian_window"), ref_lat):
        assert np.linalg.norm(lat[k].numpy() - r) <= 1e-12 * np.linalg.norm(r), k
    # per-signal masks that repeat the shared ones: the same fit, no hint
    nef2 = _Oracle(c)
    loss2, lat2 = inner_loop_cells(nef2, None, lat0, lrs, t(c.x[0]), t(c.q[0]), 4, t(c.y), masks[None].expand(3, -1, -1).contiguous(),
                                   obs_weights=t(c.w))
    assert nef2.hints == [False, False] and abs(float(loss2) - float(loss)) <= 1e-6 * float(loss)
    assert all(torch.allclose(lat2[k], lat[k], rtol=1e-12, atol=0) for k in lat)
    with pytest.raises(ValueError, match="group"):
        inner_loop_cells(nef, None, lat0, lrs, t(c.x[0]), None, 3, t(c.y), masks)
    with pytest.raises(ValueError, match="normalize_weights"):
        inner_loop_cells(nef, None, lat0, lrs, t(c.x[0]), None, 4, t(c.y), masks, normalize_weights=True)


# ---- 2. header, exports, refusals
def test_symbols_and_header():
    with open(os.path.join(ROOT, "include", "enf_hip.h")) as f:
        h = f.read()
    lib = _lib.load()
    assert re.search(r"#define\s+ENF_ABI_VERSION\s+2\b", h) and lib.enf_abi_version() == 2
    for name in ("enf_fit_step_gs", "enf_mse_value_grad_g", "enf_fit_inputs_g"):
        assert re.search(rf"\bint\s+{name}\s*\(", h), name
        assert name in _lib.EXPORTS and hasattr(lib, name) and hasattr(_lib.load_test(), name) and hasattr(_lib.load_f32r(), name)
    assert len(lib.enf_fit_step_gs.argtypes) == 22 and len(lib.enf_mse_value_grad_g.argtypes) == 16 and len(lib.enf_fit_inputs_g.argtypes) == 22


def _P():
    dummy = ctypes.create_string_buffer(64)
    return dummy, ctypes.cast(dummy, ctypes.c_void_p)


def test_fit_step_gs_refusals_and_their_order():
    lib = _lib.load()
    dummy, P = _P()
    mk = lambda N=48, O=2, window=1, B=3: _lib.make_desc(B, N, 7, 2, 64, 12, O, 2, 0, window, 0)
    big = 1 << 40

    def call(fn=None, desc=None, x=P, p=P, a=P, sigma=P, blob=P, y=P, G=4, q=P, w=P, loss=P, dp=P, da=P, ds=P, err=P, lb=P, ws=P, nbytes=big,
             flags=0, xb=0):
        desc = mk() if desc is None else desc
        return (fn or lib.enf_fit_step_gs)(ctypes.byref(desc), x, xb, p, a, sigma, blob, y, G, q, w, 1.0, loss, dp, da, ds, err, lb, ws, nbytes,
                                           flags, None)
    assert call(desc=mk(O=33)) == EUNSUPPORTED and call(desc=mk(O=33), G=3, y=None, flags=SHARED, nbytes=0) == EUNSUPPORTED
    for G in (0, -1, 3, 5, 12, 32):
        assert call(G=G, nbytes=0) == EINVAL and call(G=G, flags=SHARED, nbytes=0) == EINVAL, G
    for G in (1, 2, 4, 8, 16):
        assert call(G=G, nbytes=0) == EWORKSPACE and call(G=G, flags=SHARED, nbytes=0) == EWORKSPACE, G
    assert call(desc=mk(N=50), G=4, nbytes=0) == EINVAL and call(desc=mk(N=50), G=2, flags=SHARED, nbytes=0) == EWORKSPACE
    for k in ("y", "x", "p", "a", "sigma", "blob", "loss", "dp", "da", "ds", "ws"):
        assert call(**{k: None}, nbytes=0, flags=SHARED) == EINVAL, k
    assert call(q=None, w=None, err=None, lb=None, nbytes=0, flags=SHARED) == EWORKSPACE
    assert call(err=None, lb=P, nbytes=0) == EINVAL
    # the shared-latent statement: legal here, with the deterministic bit too; a batch stride contradicts it unless B == 1
    assert call(flags=SHARED | DET, nbytes=0) == EWORKSPACE
    assert call(flags=SHARED, xb=96, nbytes=0) == EINVAL and call(flags=SHARED, xb=96) == EINVAL
    assert call(desc=mk(B=1), flags=SHARED, xb=96, nbytes=0) == EWORKSPACE and call(xb=96, nbytes=0) == EWORKSPACE
    for flags in (1, 2, 4, 8, 32, 64, SHARED | 2):
        assert call(flags=flags, nbytes=0) == EINVAL, flags
    d = mk()
    for flags in (0, DET, SHARED, SHARED | DET):        # the workspace sizes are enf_fit_step_g's
        assert call(flags=flags, nbytes=lib.enf_workspace_bytes_ex(ctypes.byref(d), flags & DET) - 1) == EWORKSPACE
    # and enf_fit_step_g still refuses the flag
    g = lib.enf_fit_step_g
    assert call(g, flags=SHARED, nbytes=0) == EINVAL and call(g, flags=SHARED | DET) == EINVAL and call(g, desc=mk(B=1), flags=SHARED) == EINVAL
    assert call(g, nbytes=0) == EWORKSPACE


def test_mse_value_grad_g_refusals():
    lib = _lib.load()
    dummy, P = _P()

    def call(out=P, y=P, B=3, N=48, O=2, G=4, q=P, w=P, dout=P, loss=P, err=P, scr=P, nbytes=1 << 40, flags=0):
        return lib.enf_mse_value_grad_g(out, y, B, N, O, G, q, w, 1.0, dout, loss, err, scr, nbytes, flags, None)
    for k in ("out", "y", "loss"):
        assert call(**{k: None}) == EINVAL, k
    for k in ("B", "N", "O"):
        assert call(**{k: 0}) == EINVAL and call(**{k: -2}) == EINVAL, k
    for G in (0, -4, 3, 6, 32):
        assert call(G=G) == EINVAL, G
    assert call(N=50, G=4) == EINVAL
    for flags in (1, 2, 128, DET | 1):
        assert call(flags=flags) == EINVAL, flags
    assert call(flags=DET, scr=None) == EINVAL
    need = lib.enf_mse_scratch_bytes(3 * 12 * 2, DET)
    assert need > 0 and call(flags=DET, nbytes=need - 1) == EWORKSPACE and call(flags=DET, nbytes=0) == EWORKSPACE


def test_fit_inputs_g_refusals():
    lib = _lib.load()
    dummy, P = _P()
    comps = (_lib.EnfFitComponent * _lib.ENF_SGD_MAX_SEGMENTS)()
    comps[0] = _lib.EnfFitComponent(P.value, P.value, 2, 0)

    def call(ncomp=1, cs=comps, B=3, Z=7, M=30, Ms=11, S1=3, G=4, dx=2, O=2, xq=P, q=P, obs=P, masks=P, xs=P, qs=P, ys=P, losses=P, ow=P, ws=P,
             per_signal=0):
        return lib.enf_fit_inputs_g(ncomp, cs, B, Z, M, Ms, S1, G, dx, O, xq, q, obs, masks, xs, qs, ys, losses, ow, ws, per_signal, None)
    for k in ("xq", "obs", "masks", "xs", "ys", "losses", "cs"):
        assert call(**{k: None}) == EINVAL and call(**{k: None}, per_signal=1) == EINVAL, k
    for k in ("B", "Z", "M", "Ms", "S1", "dx", "O"):
        assert call(**{k: 0}) == EINVAL and call(**{k: -1}) == EINVAL, k
    for G in (0, -1, 3, 6, 17, 32):
        assert call(G=G) == EINVAL, G
    assert call(ncomp=0) == EINVAL and call(ncomp=_lib.ENF_SGD_MAX_SEGMENTS + 1) == EINVAL
    assert call(q=None) == EINVAL and call(qs=None) == EINVAL                                 # q and qs: together or not at all
    assert call(ow=None) == EINVAL and call(ws=None) == EINVAL                                # shared masks: oweight and ws alike
    assert call(ws=None, per_signal=1) == EINVAL and call(ow=None, ws=None, per_signal=1) == EINVAL     # per-signal masks: ws required
    bad = (_lib.EnfFitComponent * _lib.ENF_SGD_MAX_SEGMENTS)()
    bad[0] = _lib.EnfFitComponent(P.value, P.value, 0, 0)
    assert call(cs=bad) == EINVAL


# ---- 3. the yardstick of the grouped meta-gradient
def _small():
    from tests.test_gpu_trainer import _problem
    return CT.cell_problem(_problem(seed=2, Z=4, side=4, B=2, S=2, Ns=6), side=4, k=2, Ms=6)


def test_reference_meta_gradient_matches_central_differences():
    """the double-backward meta-gradient of tests/cells_train_ref.py along random directions in two weight tensors and in the latent
    initialisation `a` and the inner rates, against (L(+h) - L(-h)) / 2h of its own loss in fp64.  h = 1e-6: truncation ~ h^2 = 1e-12
    and rounding ~ 1e-16 / h = 1e-10 relative to the loss, and the directional derivatives are within two decades of the loss: 1e-6
    relative.  (The step is small on purpose: the inner steps' gradients jump where a relu unit changes sign, so the meta-loss is only
    piecewise smooth -- at h = 1e-5 one such jump lies inside the interval of the first direction.)"""
    cfg, prm, x, q, G, obs, lat0, lrs, masks = _small()
    rng = np.random.default_rng(4)
    w = rng.uniform(0.5, 1.5, obs.shape[:2])
    w[0, int(masks[0, 0])] = 0.0
    loss, gw, gl, gr = CT.meta_grads(prm, cfg, lat0, lrs, x, q, G, obs, masks, w)
    assert abs(loss - CT.meta_loss(prm, cfg, lat0, lrs, x, q, G, obs, masks, w)) <= 1e-14 * loss
    h = 1e-6
    names = [p[-2:] for p in TENSOR_PATHS]
    for i in (names.index(("a_to_v", "kernel")), [p[-3:] for p in TENSOR_PATHS].index(("layers_0", "linear", "kernel"))):
        v = rng.standard_normal(gw[i].shape)

        def at(sg):
            pr = copy.deepcopy(prm)
            leaf = CT._get(pr["params"], TENSOR_PATHS[i][:-1])
            leaf[TENSOR_PATHS[i][-1]] = leaf[TENSOR_PATHS[i][-1]] + sg * h * v
            return CT.meta_loss(pr, cfg, lat0, lrs, x, q, G, obs, masks, w)
        want, cd = float((gw[i] * v).sum()), (at(1.0) - at(-1.0)) / (2 * h)
        print("/".join(TENSOR_PATHS[i][-3:]), "directional derivative", want, "central difference", cd, "loss", loss)
        assert abs(cd - want) <= 1e-6 * abs(want)
    v = rng.standard_normal(gl["a"].shape)
    at = lambda sg: CT.meta_loss(prm, cfg, dict(lat0, a=lat0["a"] + sg * h * v), lrs, x, q, G, obs, masks, w)
    want, cd = float((gl["a"] * v).sum()), (at(1.0) - at(-1.0)) / (2 * h)
    print("lat0/a directional derivative", want, "central difference", cd)
    assert abs(cd - want) <= 1e-6 * abs(want)
    v = rng.standard_normal(gr["a"].shape)
    at = lambda sg: CT.meta_loss(prm, cfg, lat0, dict(lrs, a=lrs["a"] + sg * h * v), x, q, G, obs, masks, w)
    want, cd = float((gr["a"] * v).sum()), (at(1.0) - at(-1.0)) / (2 * h)
    print("lr/a directional derivative", want, "central difference", cd)
    assert abs(cd - want) <= 1e-6 * abs(want)


def test_trainers_refuse_channel_weights_on_cells():
    from enf_pde_amd.fitting.trainers import meta_gradients
    x, img = torch.zeros(16, 2), torch.zeros(2, 4, 1)
    with pytest.raises(ValueError, match="channel_weights"):
        meta_gradients(None, None, {}, {}, None, img, torch.zeros(2, 3, dtype=torch.long), channel_weights=torch.ones(4, 1), cells=(x, None, 4))
    with pytest.raises(ValueError, match="group"):
        meta_gradients(None, None, {}, {}, None, img, torch.zeros(2, 3, dtype=torch.long), cells=(x, None, 3))
    with pytest.raises(ValueError, match="cells hold"):
        meta_gradients(None, None, {}, {}, None, img, torch.zeros(2, 3, dtype=torch.long), cells=(x, None, 2))
