"""Per-channel loss weights on the GPU path (include/enf_hip.h, "Weighted loss": enf_fit_step_cw, enf_mse_value_grad_cw,
enf_fit_inputs_cw):

    loss = 1 / (B N O) * sum_{b,n,o} cw[b,n,o] (out - target)^2,     d out = 2 cw (out - target) / (B N O) * grad_scale

The oracle is oracle.enf_ref_torch.nef_apply in fp64; the weighted loss is formed here around it.  Shapes are the smallest at which
the tail's lane-to-channel mapping and its partial tiles can go wrong: O in {1, 3, 5, 32} (one lane, part of a quad, two quads, both
16-output tiles full), N = 70 (no multiple of the 16-query tile: B N = 140 / 210 queries end inside a wave, the second workgroup is
partial), B = 2 and 3, Z = 9, num_hidden 128 with 2 heads and once 64 with 3 heads (padded to 4).

Tolerances are tests/test_gpu_weighted_fit.py's for the same quantities: gradients tests/test_gpu_backward.TOL, a loss value against
fp64 5e-4 (f32) / 5e-2 (bf16) of max(1, loss); the inner loop 5e-4 on the loss and 20 times that on the latent updates."""
import ctypes
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

from oracle import enf_ref_np as R
from oracle import enf_ref_torch as T
from tests.helpers import make_cfg, make_inputs, build_nef
from tests.test_gpu_backward import TOL, ref_grads, rel
from tests.test_gpu_weighted_fit import LOSS_TOL
from enf_pde_amd import _lib
from enf_pde_amd.fitting.inner_loop import _fit_inputs, gather_signal_points, inner_loop, make_signal_masks
from enf_pde_amd.fitting.weights import valid_channel_weights, point_support, gather_point_weights

pytestmark = pytest.mark.gpu

N, Z = 70, 9


def _t(cuda):
    return lambda v: torch.tensor(np.asarray(v), dtype=torch.float32, device=cuda)


def _cweights(rng, B, N, O):
    """random in [0, 2] with about 30 % exact zeros; for signal 0 the whole last channel is zero (where there is more than one);
    the last signal is all zero.  Rounded to fp32 so that the product sees the reference's numbers."""
    cw = rng.uniform(0, 2, (B, N, O))
    cw[rng.uniform(size=(B, N, O)) < 0.3] = 0.0
    if O > 1:
        cw[0, :, O - 1] = 0.0
    cw[B - 1] = 0.0
    return cw.astype(np.float32).astype(np.float64)


_REF = {}


def _case(D, H, O, B, seed=41):
    """inputs and fp64 reference of one fit step with channel weights, computed once per session and left unchanged"""
    key = (D, H, O, B, seed)
    if key not in _REF:
        cfg = make_cfg("rel_pos_periodic", D=D, H=H, C=12, O=O, freq=(0.3, 0.6))
        prm = R.init_params(seed, cfg, jitter=0.1)
        x, p, a, s = make_inputs(cfg, B, N, Z, seed + 1)
        rng = np.random.default_rng(seed + 2)
        y = rng.standard_normal((B, N, O))
        cw = _cweights(rng, B, N, O)
        out = T.nef_apply(T.to_torch(prm, torch.float64), cfg, *(torch.tensor(v) for v in (x, p, a, s))).numpy()
        loss = float((cw * (out - y) ** 2).sum() / (B * N * O))
        _, rp, ra, rs = ref_grads(prm, cfg, x, p, a, s, 2 * cw * (out - y) / (B * N * O))
        _REF[key] = (cfg, prm, (x, p, a, s, y, cw), (loss, rp, ra, rs))
    return _REF[key]


CASES = [(128, 2, 1, 2), (128, 2, 3, 2), (128, 2, 3, 3), (128, 2, 5, 3), (128, 2, 32, 2), (64, 3, 3, 3)]


# ---- 1. the fit step against fp64
@pytest.mark.parametrize("precision", ["f32", "bf16"])
@pytest.mark.parametrize("D,H,O,B", CASES)
def test_fit_step_matches_oracle(cuda, bwd_variant, D, H, O, B, precision):
    cfg, prm, (x, p, a, s, y, cw), (loss, rp, ra, rs) = _case(D, H, O, B)
    nef = build_nef(cfg, precision)
    t = _t(cuda)
    res = nef.mse_value_and_latent_grads(nef.load_params(prm, device=cuda), t(x), t(p), t(a), t(s), t(y), channel_weight=t(cw))
    got = float(res[0])
    errs = {k: rel(g.cpu().numpy().astype(np.float64), r) for k, g, r in (("p", res[1], rp), ("a", res[2], ra), ("sigma", res[3], rs))}
    print((D, H, O, B), precision, "loss", got, "ref", loss, "gradient errors", errs)
    assert np.isfinite(got) and abs(got - loss) < LOSS_TOL[precision] * max(1.0, loss), (got, loss)
    for k, e in errs.items():
        assert np.isfinite(e) and e < TOL[precision], (precision, k, e)
    # the last signal's weights are all zero: its gradients are exact zeros, not small numbers
    for g in res[1:]:
        assert bool((g[B - 1] == 0).all())


def test_wrong_shapes_and_both_keywords_are_value_errors(cuda):
    cfg, prm, (x, p, a, s, y, cw), _ = _case(128, 2, 3, 2)
    nef = build_nef(cfg, "f32")
    t = _t(cuda)
    args = (nef.load_params(prm, device=cuda), t(x), t(p), t(a), t(s), t(y))
    for bad in (t(cw)[..., 0], t(cw)[..., :2], t(cw)[:, :-1], t(cw)[..., None]):
        with pytest.raises(ValueError):
            nef.mse_value_and_latent_grads(*args, channel_weight=bad)
    with pytest.raises(ValueError):
        nef.mse_value_and_latent_grads(*args, weight=t(cw)[..., 0], channel_weight=t(cw))
    with pytest.raises(ValueError):                                     # weight= keeps its meaning: (B, N) only
        nef.mse_value_and_latent_grads(*args, weight=t(cw)[..., :1])


# ---- 2. missing values do not exist
@pytest.mark.parametrize("precision", ["f32", "bf16"])
@pytest.mark.parametrize("D,H,O,B", [(128, 2, 3, 3), (128, 2, 32, 2), (64, 3, 3, 3)])
def test_targets_under_zero_weights_are_never_used(cuda, D, H, O, B, precision):
    """deterministic mode: NaN / Inf exactly where the weight is 0 gives finite results with the bits of the runs whose targets
    hold 0 and 1e30 there"""
    cfg, prm, (x, p, a, s, y, cw), _ = _case(D, H, O, B)
    nef = build_nef(cfg, precision)
    nef.deterministic = True
    assert nef.is_deterministic()
    t = _t(cuda)
    params = nef.load_params(prm, device=cuda)
    gone = cw == 0
    assert 0.3 < gone.mean() < 1
    runs = []
    for fill in ("naninf", 0.0, 1e30):
        yy = y.copy()
        if fill == "naninf":
            yy[gone] = np.array([np.inf, -np.inf, np.nan])[np.arange(int(gone.sum())) % 3]
        else:
            yy[gone] = fill
        runs.append(nef.mse_value_and_latent_grads(params, t(x), t(p), t(a), t(s), t(yy), grad_scale=float(B), channel_weight=t(cw)))
    for v in runs[0]:
        assert bool(torch.isfinite(v).all())
    assert float(runs[0][0]) > 0
    for other in runs[1:]:
        for name, u, v in zip(("loss", "dp", "da", "dsigma"), runs[0], other):
            assert torch.equal(u, v), (name, float((u - v).abs().max()))
    again = nef.mse_value_and_latent_grads(params, t(x), t(p), t(a), t(s), t(y), grad_scale=float(B), channel_weight=t(cw))
    assert all(torch.equal(u, v) for u, v in zip(again, runs[1]))        # ENF_FIT_DETERMINISTIC: same inputs, same bits


# ---- 3. reduction to per-point weights
@pytest.mark.parametrize("D,H,O,B", [(128, 2, 1, 2), (128, 2, 3, 3), (128, 2, 32, 2), (64, 3, 3, 3)])
def test_broadcast_point_weights_are_the_per_point_loss(cuda, D, H, O, B):
    """f32: cw = w[..., None] against enf_fit_step_w on w, and all ones against the unweighted call: gradients at the f32
    latent-gradient tolerance, the loss to 1e-6 relative (the fp32 rounding of an O-term sum)."""
    cfg, prm, (x, p, a, s, y, cw), _ = _case(D, H, O, B)
    nef = build_nef(cfg, "f32")
    t = _t(cuda)
    params = nef.load_params(prm, device=cuda)
    args = (params, t(x), t(p), t(a), t(s), t(y))
    w = t(cw[..., 0] + 0.25 * (cw[..., 0] == 0) * (np.arange(N)[None] % 2))       # zeros and positive values, no all-zero signal
    point = nef.mse_value_and_latent_grads(*args, weight=w)
    chan = nef.mse_value_and_latent_grads(*args, channel_weight=w[..., None].expand(B, N, O).contiguous())
    plain = nef.mse_value_and_latent_grads(*args)
    ones = nef.mse_value_and_latent_grads(*args, channel_weight=torch.ones((B, N, O), device=cuda))
    for what, got, ref in (("per-point", chan, point), ("unweighted", ones, plain)):
        print(what, (D, H, O, B), float(got[0]), float(ref[0]))
        assert abs(float(got[0]) - float(ref[0])) < 1e-6 * float(ref[0]), (what, float(got[0]), float(ref[0]))
        for name, u, v in zip(("dp", "da", "dsigma"), got[1:], ref[1:]):
            e = rel(u.cpu().numpy().astype(np.float64), v.cpu().numpy().astype(np.float64))
            assert e < TOL["f32"], (what, name, e)


# ---- 4. the loss kernel
def test_mse_value_grad_cw(cuda):
    """n = 2 * 333 * 3 = 1998 elements, no multiple of 256, eight blocks; float64 numpy is the reference.  fp32 bounds as in
    tests/test_gpu_weighted_fit.py::test_mse_value_grad_w: every dout is three roundings from exact (asserted at 1e-6 of the
    largest), the loss is a sum of 1998 non-negative terms (1e-5 relative)."""
    lib = _lib.load()
    rng = np.random.default_rng(3)
    B, Nn, O = 2, 333, 3
    out, y = rng.standard_normal((B, Nn, O)), rng.standard_normal((B, Nn, O))
    cw = _cweights(rng, B + 1, Nn, O)[:B]                        # (no all-zero signal here; the last channel of signal 0 is zero)
    y[cw == 0] = np.nan
    y[0, 0, O - 1] = np.inf
    t = _t(cuda)
    o_, y_, w_ = t(out), t(y), t(cw)
    o64, y64, w64 = (v.double().cpu().numpy() for v in (o_, y_, w_))
    d = np.where(w64 > 0, o64 - np.nan_to_num(y64, posinf=0.0, neginf=0.0), 0.0)
    n = B * Nn * O
    ref_loss = float((w64 * d * d).sum() / n)
    ref_dout = 2 * w64 * d / n * 1.5
    st = ctypes.c_void_p(torch.cuda.current_stream(cuda).cuda_stream)
    runs = []
    for flags in (0, _lib.ENF_MSE_DETERMINISTIC, _lib.ENF_MSE_DETERMINISTIC):
        nb = int(lib.enf_mse_scratch_bytes(n, flags))
        scr = torch.full((max(nb, 1),), 255, device=cuda, dtype=torch.uint8)
        dout, loss = torch.full_like(o_, 7.0), torch.zeros(1, device=cuda)
        _lib.launch(cuda, lib.enf_mse_value_grad_cw, o_.data_ptr(), y_.data_ptr(), w_.data_ptr(), n, 1.5, dout.data_ptr(),
                    loss.data_ptr(), scr.data_ptr() if nb else None, nb, flags, st)
        torch.cuda.synchronize()
        runs.append((loss.clone(), dout.clone()))
        print("mse_cw", flags, float(loss), ref_loss)
        assert abs(float(loss) - ref_loss) < 1e-5 * ref_loss
        assert bool((dout[w_ == 0] == 0).all()) and bool(torch.isfinite(dout).all())
        assert float(np.abs(dout.double().cpu().numpy() - ref_dout).max()) < 1e-6 * float(np.abs(ref_dout).max())
    assert torch.equal(runs[1][0], runs[2][0]) and torch.equal(runs[1][1], runs[2][1])
    # no dout asked for: the value alone
    loss = torch.zeros(1, device=cuda)
    _lib.launch(cuda, lib.enf_mse_value_grad_cw, o_.data_ptr(), y_.data_ptr(), w_.data_ptr(), n, 1.0, None, loss.data_ptr(), None, 0, 0, st)
    assert abs(float(loss) - ref_loss) < 1e-5 * ref_loss


# ---- 5. the gathers
def _lat0(rng, t, Zl):
    return {"p_pos": t(rng.standard_normal((1, Zl, 2))), "a": t(rng.standard_normal((1, Zl, 6)))}


@pytest.mark.parametrize("O", [1, 3, 5, 17])
@pytest.mark.parametrize("per_signal", [False, True])
def test_gather_parity(cuda, per_signal, O):
    rng = np.random.default_rng(11)
    B, Ng, Ns, S1, Zl, dx = 3, 50, 17, 4, 5, 2
    t = _t(cuda)
    lat0 = _lat0(rng, t, Zl)
    coords, img, cw = t(rng.standard_normal((Ng, dx))), t(rng.standard_normal((B, Ng, O))), t(_cweights(rng, B, Ng, O))
    img[cw == 0] = float("nan")
    if per_signal:
        masks = torch.tensor(np.stack([np.stack([rng.permutation(Ng)[:Ns] for _ in range(S1)], 1) for _ in range(B)]), device=cuda)
        idx = masks.permute(2, 0, 1)                                                          # (S1, B, Ns)
        ref_x = coords[idx]
        ref_y = torch.gather(img[None].expand(S1, -1, -1, -1), 2, idx[..., None].expand(-1, -1, -1, O))
        ref_w = torch.gather(cw[None].expand(S1, -1, -1, -1), 2, idx[..., None].expand(-1, -1, -1, O))
    else:
        masks = torch.tensor(np.stack([rng.permutation(Ng)[:Ns] for _ in range(S1)], 1), device=cuda)
        ref_x, ref_y = coords[masks.t()], img[:, masks.t()].transpose(0, 1)
        ref_w = gather_point_weights(cw, masks)
    lat, xs, ys, losses, ws = _fit_inputs(lat0, coords, img, masks, cw, channel=True)
    assert ws.shape == (S1, B, Ns, O) and torch.equal(ws, ref_w)
    assert xs.shape == ref_x.shape and torch.equal(xs, ref_x)
    assert torch.equal(torch.isnan(ys), torch.isnan(ref_y)) and torch.equal(torch.nan_to_num(ys), torch.nan_to_num(ref_y))
    assert torch.equal(torch.isnan(ys), ws == 0)                         # the NaN of missing values pass through the gather
    assert losses.shape == (S1,) and bool((losses == 0).all())
    for k in lat0:
        assert torch.equal(lat[k], lat0[k].expand(B, -1, -1))
    if per_signal:
        comp = gather_signal_points(coords, torch.nan_to_num(img), masks, cw)               # the composed route gathers the same
        assert torch.equal(xs, comp[0]) and torch.equal(torch.nan_to_num(ys), comp[1]) and torch.equal(ws, comp[2])


@pytest.mark.parametrize("per_signal", [False, True])
def test_index_contract(cuda, per_signal):
    """-1 and indices >= N give coords[0], zero targets and O zero weights.  The three inputs sit at the very END of buffers whose
    front is filled with a sentinel (an index >= N used as an offset would leave the buffer; a negative one would bring the sentinel
    or a neighbouring signal's values into the outputs): the outputs are compared with the torch reference only."""
    SENTINEL = 12345.678
    rng = np.random.default_rng(12)
    B, Ng, Ns, S1, dx, O, Zl, pad = 3, 50, 16, 4, 2, 3, 5, 64
    t = _t(cuda)

    def at_end(values):
        buf = torch.full((pad + values.size,), SENTINEL, device=cuda, dtype=torch.float32)
        view = buf[pad:].view(values.shape)
        view.copy_(t(values))
        return view
    coords, img, cw = at_end(rng.standard_normal((Ng, dx))), at_end(rng.standard_normal((B, Ng, O))), at_end(rng.uniform(0.5, 2, (B, Ng, O)))
    if per_signal:
        m = np.stack([np.stack([rng.permutation(Ng)[:Ns] for _ in range(S1)], 1) for _ in range(B)])
    else:
        m = np.stack([rng.permutation(Ng)[:Ns] for _ in range(S1)], 1)
    bad = rng.uniform(size=m.shape) < 0.3
    m[bad] = rng.choice([-1, Ng, Ng + 7, -Ng, 2 ** 40], size=int(bad.sum()))
    m[..., 0, 0], m[..., Ns - 1, S1 - 1], m[..., 1, 1] = -1, Ng + 7, Ng
    masks = torch.tensor(m, device=cuda)
    lat, xs, ys, losses, ws = _fit_inputs(_lat0(rng, t, Zl), coords, img, masks, cw, channel=True)
    torch.cuda.synchronize()
    for out in (xs, ys, ws, losses):
        assert bool(torch.isfinite(out).all()) and not bool((out == SENTINEL).any())
    full = masks if per_signal else masks[None].expand(B, -1, -1).contiguous()
    ref = gather_signal_points(coords, img, full, cw)
    idx = full.permute(2, 0, 1)
    ok = (idx >= 0) & (idx < Ng)
    assert bool((~ok).any()) and bool(ok.any())
    assert bool((ws[~ok] == 0).all()) and bool((ys[~ok] == 0).all()) and bool((ws[ok] > 0).all())
    assert torch.equal(ys, ref[1]) and torch.equal(ws, ref[2]) and ws.shape == (S1, B, Ns, O)
    assert torch.equal(xs, ref[0] if per_signal else ref[0][:, 0])       # shared masks: one (S1, Ns, dx) set, coords[0] for a bad index


# ---- 6. the inner loop against the oracle's loop with the weighted loss
def _oracle_inner_loop(params, cfg, lat0, lrs, coords, img, masks, cw):
    """oracle/enf_ref_torch.py's inner loop with the per-channel weighted loss; masks (Ns, S+1) or (B, Ns, S+1), -1 = no point"""
    spec = T.invariant_spec(cfg["invariant"], cfg.get("num_in", 2))
    B, S = img.shape[0], masks.shape[-1] - 1
    O = img.shape[-1]
    full = masks if masks.dim() == 3 else masks[None].expand(B, -1, -1)
    lat = {k: v.repeat_interleave(B, dim=0).detach().clone().requires_grad_(True) for k, v in lat0.items()}

    def loss_fn(lat, s):
        m = full[:, :, s]
        ok = m >= 0
        ic = torch.where(ok, m, torch.zeros_like(m))
        xs = coords[ic]
        ys = torch.gather(img, 1, ic[..., None].expand(-1, -1, O))
        ws = torch.gather(cw, 1, ic[..., None].expand(-1, -1, O)) * ok[..., None]
        out = T.nef_apply(params, cfg, xs, T.split_pose(lat, spec), lat["a"], lat["gaussian_window"])
        d = torch.where(ws > 0, out - ys, torch.zeros_like(out))
        return (ws * d * d).mean()

    for s in range(S):
        keys = list(lat.keys())
        g = torch.autograd.grad(loss_fn(lat, s), [lat[k] for k in keys], allow_unused=True)
        new = {}
        for k, gk in zip(keys, g):
            gk = torch.zeros_like(lat[k]) if (gk is None or k == "gaussian_window") else gk * B     # pde_trainer.py:206-212
            new[k] = (lat[k] - lrs[k] * gk).detach().requires_grad_(True)                            # pde_trainer.py:215-219
        lat = new
    return loss_fn(lat, S).detach(), lat


@pytest.mark.parametrize("per_signal", [False, True])
def test_inner_loop_matches_fp64_trace(cuda, per_signal):
    """S = 3, B = 2, an 8 x 8 grid, Ns = 40, Z = 4, two channels, f32.  The second channel is NaN on half the points of signal 0 and
    signal 1 observes 30 points in all (per-signal rows padded with -1); the weights are valid_channel_weights of the field."""
    C, B, side, Ns, Zl, S = 8, 2, 8, 40, 4, 3
    cfg = make_cfg("rel_pos_periodic", D=64, H=2, C=C, O=2)
    prm = R.init_params(7, cfg, jitter=0.1)
    rng = np.random.default_rng(8)
    lin = np.linspace(-1, 1, side)
    coords = np.stack(np.meshgrid(lin, lin), -1).reshape(-1, 2)
    Ng = side * side
    img = rng.standard_normal((B, Ng, 2))
    img[0, rng.permutation(Ng)[:Ng // 2], 1] = np.nan
    img[1, rng.permutation(Ng)[30:]] = np.nan
    img[1, rng.uniform(size=Ng) < 0.3, 0] = np.nan
    cw = valid_channel_weights(torch.tensor(img)).double()
    lat0 = {"p_pos": R.init_positions_grid(1, Zl, 2) + 0.02 * rng.standard_normal((1, Zl, 2)),
            "a": 1 + 0.1 * rng.standard_normal((1, Zl, C)), "gaussian_window": np.full((1, Zl, 1), 2.0 / 3)}
    lrs = {"p_pos": np.array([0.5]), "a": np.full((C,), 2.0) * (1 + 0.1 * rng.standard_normal(C)), "gaussian_window": np.array([0.0])}
    if per_signal:
        masks = make_signal_masks(point_support(cw), Ns, S, generator=torch.Generator().manual_seed(3), device="cpu")
        assert bool((masks[1] == -1).any())
    else:
        masks = torch.tensor(np.stack([rng.permutation(Ng)[:Ns] for _ in range(S + 1)], 1))
    t64 = lambda v: torch.tensor(v, dtype=torch.float64)
    ref_loss, ref_fit = _oracle_inner_loop(T.to_torch(prm, torch.float64), cfg, {k: t64(v) for k, v in lat0.items()},
                                           {k: t64(v) for k, v in lrs.items()}, t64(coords), torch.nan_to_num(t64(img)), masks, cw)
    t = _t(cuda)
    nef = build_nef(cfg, "f32")
    loss, fit = inner_loop(nef, nef.load_params(prm, device=cuda), {k: t(v) for k, v in lat0.items()}, {k: t(v) for k, v in lrs.items()},
                           t(coords), t(img), masks.to(cuda), channel_weights=cw.float().to(cuda))
    tol = LOSS_TOL["f32"]
    print("inner loop", per_signal, float(loss), float(ref_loss))
    assert np.isfinite(float(loss)) and abs(float(loss) - float(ref_loss)) < tol * max(1.0, float(ref_loss))
    for k, v in fit.items():
        ref, init = ref_fit[k].detach().numpy(), np.repeat(lat0[k], B, 0)
        if np.abs(ref - init).max() == 0:
            assert np.abs(v.cpu().numpy() - init.astype(np.float32)).max() == 0, k      # gaussian_window frozen
        else:
            e = rel(v.cpu().numpy().astype(np.float64) - init, ref - init)
            print("inner loop", per_signal, k, e)
            assert e < tol * 20, (k, e)


# ---- 7. the trainers: a two-channel field whose second channel is NaN on half the points
def _maml(cuda, sample_observed=False):
    from enf_pde_amd.fitting.trainers import MetaSGDPDETrainer
    from enf_pde_amd.enf.latents.autodecoder_meta import PositionOrientationFeatureAutodecoderMeta
    cfg = make_cfg("rel_pos_periodic", D=64, H=2, C=8, O=2)
    prm = R.init_params(0, cfg, jitter=0.1)
    lin = np.linspace(-1, 1, 8)
    coords = np.stack(np.meshgrid(lin, lin), -1).reshape(-1, 2)
    conf = NS(optimizer=NS(learning_rate_enf=1e-3, learning_rate_codes=1e-3),
              meta=NS(learning_rate_meta_sgd=1e-2, num_inner_steps=2, inner_learning_rate_p=0.5, inner_learning_rate_a=2.0,
                      inner_learning_rate_window=0.0, noise_pos_inner_loop=0.0),
              nef=NS(optimize_gaussian_window=False), training=NS(max_num_sampled_points=32))
    nef = build_nef(cfg, "f32")
    nef.deterministic = True
    ad = PositionOrientationFeatureAutodecoderMeta(1, 9, 8, 2, 0, gaussian_window_size=-1)
    tr = MetaSGDPDETrainer(conf, nef, ad, _t(cuda)(coords), seed=0, second_order="fd", sample_observed=sample_observed)
    return tr, nef.load_params(prm, device=cuda)


def _half_missing(rng, shape):
    """a field (B, ..., 2) whose second channel is NaN on half the points of every signal"""
    f = rng.standard_normal(shape).astype(np.float32)
    flat = f.reshape(shape[0], -1, 2)
    for b in range(shape[0]):
        flat[b, rng.permutation(flat.shape[1])[:flat.shape[1] // 2], 1] = np.nan
    return flat.reshape(shape)


@pytest.mark.parametrize("sample_observed", [False, True])
def test_maml_nef_step_on_a_field_with_a_missing_variable(cuda, sample_observed):
    rng = np.random.default_rng(21)
    field = _half_missing(rng, (2, 8, 8, 2))
    results = []
    for fill in (None, 0.0, -7.5):
        tr, params = _maml(cuda, sample_observed)
        state = tr.init_train_state(params)
        batch = torch.tensor(field, device=cuda)
        cw = valid_channel_weights(batch.reshape(2, 64, 2))
        if fill is not None:
            batch = torch.nan_to_num(batch, nan=fill)
        before = [x.clone() for x in tr.nef.param_tensors(state.params["nef"])]
        loss, new = tr.nef_train_step(state, batch, channel_weights=cw)
        after = tr.nef.param_tensors(new.params["nef"])
        assert np.isfinite(float(loss)) and float(loss) > 0
        assert all(bool(torch.isfinite(x).all()) for x in after)
        assert any(not torch.equal(a, b) for a, b in zip(before, after))
        results.append((loss, after, list(new.params["autodecoder"]["params"].values()), list(new.params["meta_sgd_lrs"].values())))
    for other in results[1:]:
        assert torch.equal(results[0][0], other[0])
        for group in (1, 2, 3):
            assert all(torch.equal(a, b) for a, b in zip(results[0][group], other[group]))
    with pytest.raises(ValueError):
        tr.nef_train_step(state, batch, weights=cw[..., 0], channel_weights=cw)


def _autodec(cuda, sample_observed=False, ode_model=None, shell=None):
    from tests.test_gpu_autodec_fit import _problem, _trainer, _state
    pb = _problem("rel_pos_periodic")
    tr, nef_params = _trainer(cuda, pb, "f32", sample_observed=sample_observed, ode_model=ode_model, shell=shell)
    tr.nef.deterministic = True
    return pb, tr, nef_params, _state


@pytest.mark.parametrize("sample_observed", [False, True])
@pytest.mark.parametrize("step", ["nef_train_step", "fit_latents_step"])
def test_autodecoder_steps_on_a_field_with_a_missing_variable(cuda, step, sample_observed):
    rng = np.random.default_rng(22)
    field = _half_missing(rng, (3, 8, 8, 2))
    idx = torch.tensor([4, 0, 2], device=cuda)
    results = []
    for fill in (None, 0.0, 3e4):
        pb, tr, nef_params, _state = _autodec(cuda, sample_observed)
        state = _state(cuda, tr, nef_params, pb)
        state.nef_opt_state = tr.nef_opt.init(tr.nef.param_tensors(nef_params))           # (nef_train_step updates the decoder too)
        batch = torch.tensor(field, device=cuda)
        cw = valid_channel_weights(batch.reshape(3, 64, 2))
        if fill is not None:
            batch = torch.nan_to_num(batch, nan=fill)
        before = {k: v.clone() for k, v in state.params["autodecoder"]["params"].items()}
        calls = []
        if step == "fit_latents_step":          # still one fit call and one table update
            from enf_pde_amd.fitting.trainers import nonmaml_pde_trainer as NT
            real_fit, real_adam = tr.nef.mse_value_and_latent_grads, NT.table_adam_update
            tr.nef.mse_value_and_latent_grads = lambda *a, **k: (calls.append(("fit", sorted(k))), real_fit(*a, **k))[1]
            NT.table_adam_update = lambda *a, **k: (calls.append(("adam", None)), real_adam(*a, **k))[1]
        try:
            loss, new = getattr(tr, step)(state, (batch, idx), channel_weights=cw)
        finally:
            if step == "fit_latents_step":
                NT.table_adam_update = real_adam
        if step == "fit_latents_step":
            assert calls == [("fit", ["channel_weight"]), ("adam", None)], calls
        after = new.params["autodecoder"]["params"]
        assert np.isfinite(float(loss)) and float(loss) > 0
        assert all(bool(torch.isfinite(v).all()) for v in after.values())
        assert not torch.equal(after["a"][idx], before["a"][idx])
        results.append((loss, list(after.values()), tr.nef.param_tensors(new.params["nef"])))
    for other in results[1:]:
        assert torch.equal(results[0][0], other[0])
        for group in (1, 2):
            assert all(torch.equal(a, b) for a, b in zip(results[0][group], other[group]))


def test_validate_epoch_with_channel_weights(cuda):
    """tests/test_gpu_autodec_fit.py::test_validate_epoch's set-up; the second channel of every frame is NaN on half the points.
    Every metric is finite, and the fitted validation table reconstructs the OBSERVED values of frame 0 better than its
    initialisation does."""
    from tests.test_gpu_autodec_fit import _FiveLatents, S, C, O, SIDE
    from enf_pde_amd.fitting.inner_loop import decode
    from enf_pde_amd.fitting.ode_models import MLPODE
    from enf_pde_amd.fitting.weights import weighted_mse
    ode = MLPODE(num_hidden=16, num_layers=3, scalar_num_out=C, vec_num_out=1)
    pb, tr, nef_params, _ = _autodec(cuda, ode_model=ode, shell=_FiveLatents(S, 5, C, 2, 0, gaussian_window_size=-1))
    val_shell = _FiveLatents(4, 5, C, 2, 0, gaussian_window_size=-1)
    state = tr.init_train_state(nef_params)
    state.params["autodecoder"]["params"] = {k: torch.tensor(v, device=cuda) for k, v in pb.table.items()}
    xy = torch.tensor(pb.coords, device=cuda)

    def fields(n, seed):
        g = torch.Generator().manual_seed(seed)
        amp, ph = torch.rand(n, 1, 1, O, generator=g).to(cuda), (6.28 * torch.rand(n, 4, 1, O, generator=g)).to(cuda)
        f = 0.6 + 0.4 * amp * torch.sin(2.0 * xy[None, None, :, :1] + 1.5 * xy[None, None, :, 1:] + ph)
        gone = torch.rand(n, 4, SIDE * SIDE, generator=g).to(cuda) < 0.5
        f[..., 1] = torch.where(gone, torch.full_like(f[..., 1], float("nan")), f[..., 1])
        return f.reshape(n, 4, SIDE, SIDE, O)

    t = lambda i: torch.tensor(i, device=cuda)
    train = [(fields(3, 1), None, t([4, 0, 2])), (fields(2, 2), None, t([1, 3]))]
    val = [(fields(2, 3), t([0, 1])), (fields(2, 4), t([3, 2]))]
    cw_of = lambda batch: valid_channel_weights(batch[0].flatten(2, 3))             # (B, T, N, O)
    metrics, last = tr.validate_epoch(state, train, val, val_shell, epochs=3, drop_rates=(0.0, 0.5), channel_weights=cw_of)
    torch.cuda.synchronize()
    assert set(metrics) == {"train_mse_in_t_sc", "train_mse_out_t_sc"} | {f"{s}_mse_{io}_t{d}" for s in ("val", "train")
                                                                          for io in ("in", "out") for d in ("", "_dp0.5")}
    assert all(type(v) is float and np.isfinite(v) for v in metrics.values()), metrics
    assert last.autodecoder_opt_state["count"] == 3 * 2

    def frame0_error(table):
        err = 0.0
        for traj, idx in val:
            rec = decode(tr.nef, state.params["nef"], tr.coords, *val_shell.apply(table, idx))
            f0 = traj[:, 0].reshape(2, -1, O)
            err += float(weighted_mse(rec, f0, valid_channel_weights(f0)))
        return err / len(val)

    e0, e1 = frame0_error(val_shell.init(device=cuda)), frame0_error(last.params["autodecoder"])
    print(f"frame-0 error on the observed values: {e0:.4f} at initialisation, {e1:.4f} after 3 epochs; metrics {metrics}")
    assert np.isfinite(e0) and e1 < e0
