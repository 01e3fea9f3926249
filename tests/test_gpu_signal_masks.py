"""Per-signal point masks on the GPU: enf_fit_inputs_b against torch gathers (pure copies: equal bits) and its index contract, the
inner loop with masks (B, N_s, S+1) against the shared-mask path and against the fp64 oracle run signal by signal, rows padded
with -1, normalize_weights, and the trainer's sample_observed / val_step(drop_rate=)."""
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

from oracle import enf_ref_np as R
from oracle import enf_ref_torch as T
from tests.helpers import make_cfg, make_inputs, build_nef
from tests.test_gpu_backward import TOL, rel
from enf_pde_amd.fitting.inner_loop import (_fit_inputs, inner_loop, make_masks, make_signal_masks, gather_signal_points,
                                            normalize_sampled_weights, default_meta_sgd_lrs)
from enf_pde_amd.fitting.weights import valid_weights

pytestmark = pytest.mark.gpu

LOSS_TOL = {"f32": 5e-4, "bf16": 5e-2}          # tests/test_gpu_ffn.py::test_ffn_inner_loop_matches_oracle, tests/test_gpu_golden.py
SENTINEL = 12345.678


def _t(cuda):
    return lambda v: torch.tensor(np.asarray(v), dtype=torch.float32, device=cuda)


def _lat0(rng, t, Z):
    return {"p_pos": t(rng.standard_normal((1, Z, 2))), "a": t(rng.standard_normal((1, Z, 6)))}       # two latent components


# ---- 1. the gather
@pytest.mark.parametrize("Ns,dx,O", [(16, 2, 2), (16, 3, 1), (1, 2, 2), (16, 2, 17)])
@pytest.mark.parametrize("weighted", [True, False])
def test_gather_parity(cuda, Ns, dx, O, weighted):
    rng = np.random.default_rng(11)
    B, N, S1, Z = 3, 50, 4, 5
    t = _t(cuda)
    lat0 = _lat0(rng, t, Z)
    coords, img = t(rng.standard_normal((N, dx))), t(rng.standard_normal((B, N, O)))
    w = t(rng.uniform(0, 2, (B, N))) if weighted else None
    masks = torch.tensor(np.stack([np.stack([rng.permutation(N)[:Ns] for _ in range(S1)], 1) for _ in range(B)]), device=cuda)
    assert masks.shape == (B, Ns, S1)
    lat, xs, ys, losses, ws = _fit_inputs(lat0, coords, img, masks, w)
    idx = masks.permute(2, 0, 1)                                                            # (S1, B, Ns)
    assert xs.shape == (S1, B, Ns, dx) and torch.equal(xs, coords[idx])
    assert torch.equal(ys, torch.gather(img[None].expand(S1, -1, -1, -1), 2, idx[..., None].expand(-1, -1, -1, O)))
    assert torch.equal(ws, torch.gather(w[None].expand(S1, -1, -1), 2, idx) if weighted else torch.ones_like(ws))
    assert losses.shape == (S1,) and bool((losses == 0).all())
    for k in lat0:
        assert torch.equal(lat[k], lat0[k].expand(B, -1, -1))
    ref = gather_signal_points(coords, img, masks, w)                                       # the composed route gathers the same
    assert torch.equal(xs, ref[0]) and torch.equal(ys, ref[1]) and torch.equal(ws, ref[2])


# ---- 2. indices outside [0, N)
@pytest.mark.parametrize("weighted", [True, False])
def test_index_contract(cuda, weighted):
    """coords, img and weight are interior slices of buffers filled with a sentinel: an index that was used as an offset would
    bring the sentinel (or a neighbouring signal's values) into the outputs."""
    rng = np.random.default_rng(12)
    B, N, Ns, S1, dx, O, Z, pad = 3, 50, 16, 4, 2, 2, 5, 64
    t = _t(cuda)

    def interior(values):
        buf = torch.full((values.size + 2 * pad,), SENTINEL, device=cuda, dtype=torch.float32)
        view = buf[pad:pad + values.size].view(values.shape)
        view.copy_(t(values))
        return view
    coords, img = interior(rng.standard_normal((N, dx))), interior(rng.standard_normal((B, N, O)))
    w = interior(rng.uniform(0.5, 2, (B, N))) if weighted else None
    m = np.stack([np.stack([rng.permutation(N)[:Ns] for _ in range(S1)], 1) for _ in range(B)])
    bad = rng.uniform(size=m.shape) < 0.3
    m[bad] = rng.choice([-1, N, N + 7, -N, 2 ** 40], size=int(bad.sum()))
    m[0, :, 0], m[B - 1, Ns - 1, S1 - 1], m[1, 0, 1], m[1, 1, 1] = -1, N + 7, N, -1        # a whole column, the last row, both ends
    masks = torch.tensor(m, device=cuda)
    lat, xs, ys, losses, ws = _fit_inputs(_lat0(rng, t, Z), coords, img, masks, w)
    torch.cuda.synchronize()
    for out in (xs, ys, ws, losses):
        assert bool(torch.isfinite(out).all()) and not bool((out == SENTINEL).any())
    idx = masks.permute(2, 0, 1)
    ok = (idx >= 0) & (idx < N)
    assert bool((~ok).any()) and bool(ok.any())
    assert torch.equal(xs[~ok], coords[0].expand(int((~ok).sum()), dx))
    assert bool((ys[~ok] == 0).all()) and bool((ws[~ok] == 0).all())
    ic = idx.clamp(0, N - 1)
    assert torch.equal(xs[ok], coords[ic][ok])
    assert torch.equal(ys[ok], torch.gather(img[None].expand(S1, -1, -1, -1), 2, ic[..., None].expand(-1, -1, -1, O))[ok])
    assert torch.equal(ws[ok], torch.gather(w[None].expand(S1, -1, -1), 2, ic)[ok] if weighted else torch.ones_like(ws[ok]))
    ref = gather_signal_points(coords, img, masks, w)
    assert torch.equal(xs, ref[0]) and torch.equal(ys, ref[1]) and torch.equal(ws, ref[2])


# ---- 3-6. the inner loop: D=128, H=2, C=16, Z=16, a 12 x 12 grid, Ns=48, S=3, B=3
_PROBLEM = {}


def _problem():
    if not _PROBLEM:
        cfg = make_cfg("rel_pos_periodic", D=128, H=2, C=16, O=1, freq=(0.5, 1.0))
        prm = R.init_params(5, cfg, jitter=0.1)
        B, Z = 3, 16
        lin = np.linspace(-1, 1, 12)
        coords = np.stack(np.meshgrid(lin, lin), -1).reshape(-1, 2)
        img = np.sin(np.pi * coords[None, :, :1]) * np.linspace(0.5, 1.5, B)[:, None, None] + 0.3 * coords[None, :, 1:] ** 2
        _, p, a, s = make_inputs(cfg, 1, 4, Z, 6)
        lat0 = {k: v.astype(np.float32).astype(np.float64) for k, v in (("p_pos", p), ("a", a), ("gaussian_window", s))}
        lrs = default_meta_sgd_lrs(16, lr_p=0.3, lr_a=2.0, device="cpu")
        _PROBLEM.update(cfg=cfg, prm=prm, coords=coords, img=img, lat0=lat0, lrs=lrs, B=B, Z=Z, Ns=48, S=3)
    return NS(**_PROBLEM)


def _run(P, cuda, precision, masks, img=None, deterministic=False, **kw):
    nef = build_nef(P.cfg, precision)
    nef.deterministic = deterministic
    t = _t(cuda)
    img = P.img if img is None else img
    return inner_loop(nef, nef.load_params(P.prm, device=cuda), {k: t(v) for k, v in P.lat0.items()},
                      {k: v.to(cuda) for k, v in P.lrs.items()}, t(P.coords), t(img), masks.to(cuda), **kw)


def test_repeated_shared_masks_are_the_shared_path_bit_for_bit(cuda):
    """deterministic f32: per-signal masks that repeat one shared mask give the bits of the 2-D call -- without weights (the
    per-signal path's unit weights are the unweighted arithmetic) and with weights."""
    P = _problem()
    masks = make_masks(144, P.Ns, P.S, generator=torch.Generator().manual_seed(0), device="cpu")
    rep = masks[None].expand(P.B, -1, -1).contiguous()
    w = _t(cuda)(np.random.default_rng(1).uniform(0.2, 2, (P.B, 144)))
    for kw in ({}, {"weights": w}, {"weights": w, "normalize_weights": True}):
        loss2, fit2 = _run(P, cuda, "f32", masks, deterministic=True, **kw)
        loss3, fit3 = _run(P, cuda, "f32", rep, deterministic=True, **kw)
        assert torch.equal(loss2, loss3), (list(kw), float(loss2), float(loss3))
        for k in fit2:
            assert torch.equal(fit2[k], fit3[k]), (list(kw), k, float((fit2[k] - fit3[k]).abs().max()))
        assert bool(torch.isfinite(loss3)) and float(loss3) > 0


@pytest.mark.parametrize("precision", ["f32", "bf16"])
def test_default_mode_agrees_with_the_shared_path(cuda, precision):
    """the default (atomic) mode, same construction: the inner-loop oracle tolerances"""
    P = _problem()
    masks = make_masks(144, P.Ns, P.S, generator=torch.Generator().manual_seed(0), device="cpu")
    loss2, fit2 = _run(P, cuda, precision, masks)
    loss3, fit3 = _run(P, cuda, precision, masks[None].expand(P.B, -1, -1).contiguous())
    tol = LOSS_TOL[precision]
    assert abs(float(loss2) - float(loss3)) < tol * max(1.0, float(loss2))
    for k in ("p_pos", "a"):
        init = _t(cuda)(np.repeat(P.lat0[k], P.B, 0))
        e = rel((fit3[k] - init).cpu().numpy(), (fit2[k] - init).cpu().numpy())
        assert e < tol * 20, (k, e)


_ORACLE = {}


def _half_observed():
    """every signal observes its own half of the 144 points; NaN elsewhere.  The fp64 reference is the unchanged oracle run once
    per signal (B = 1) on that signal's masks; the batch-mean loss is the mean of the per-signal losses."""
    if not _ORACLE:
        P = _problem()
        rng = np.random.default_rng(21)
        img = P.img.copy()
        for b in range(P.B):
            img[b, rng.permutation(144)[:72]] = np.nan
        w = valid_weights(torch.tensor(img))
        assert w.sum(-1).tolist() == [72.0] * P.B and not torch.equal(w[0], w[1]) and not torch.equal(w[1], w[2])
        masks = make_signal_masks(w, P.Ns, P.S, generator=torch.Generator().manual_seed(3), device="cpu")
        assert bool((masks >= 0).all()) and not torch.equal(masks[0], masks[1])
        tp = T.to_torch(P.prm, torch.float64)
        lat0 = {k: torch.tensor(v) for k, v in P.lat0.items()}
        lrs = {k: v.double() for k, v in P.lrs.items()}
        losses, fits = [], []
        for b in range(P.B):
            lb, fb = T.inner_loop(tp, P.cfg, lat0, lrs, torch.tensor(P.coords), torch.tensor(img[b:b + 1]), masks[b])
            losses.append(float(lb.detach()) / P.B)
            fits.append({k: v.detach().numpy() for k, v in fb.items()})
        assert all(np.isfinite(l) for l in losses)
        _ORACLE.update(img=img, w=w, masks=masks, loss=sum(losses), fit={k: np.concatenate([f[k] for f in fits], 0) for k in fits[0]})
    return NS(**_ORACLE)


@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("precision", ["f32", "bf16"])
def test_inner_loop_on_per_signal_points_matches_oracle(cuda, precision, fused, monkeypatch):
    import importlib
    IL = importlib.import_module("enf_pde_amd.fitting.inner_loop")
    monkeypatch.setattr(IL, "FUSED_FIT_INPUTS", fused)             # enf_fit_inputs_b, or the same gathers in torch ops
    P, Q = _problem(), _half_observed()
    loss, fit = _run(P, cuda, precision, Q.masks, img=Q.img, weights=Q.w.to(cuda))
    tol = LOSS_TOL[precision]
    print("per-signal inner loop", precision, fused, float(loss), Q.loss)
    assert abs(float(loss) - Q.loss) < tol * max(1.0, Q.loss)
    for k, v in fit.items():
        init = np.repeat(P.lat0[k], P.B, 0)
        upd = Q.fit[k] - init
        if np.abs(upd).max() == 0:
            assert np.abs(v.cpu().numpy() - init).max() == 0, k
        else:
            e = rel(v.cpu().numpy() - init, upd)
            print("per-signal inner loop", precision, fused, k, e)
            assert e < tol * 20, (k, e)


def test_short_rows(cuda):
    """signal 2 has 5 observed points and Ns = 16: its row is 5 indices and eleven -1.  Everything stays finite, and its fit is
    that of a call given only this signal, its 5 points and the padding, with no weights at all (the gradient of the batch-mean
    loss times B does not depend on B).  One step, so the latent update is -lr * gradient; the f32 gradient tolerance."""
    P = _problem()
    rng = np.random.default_rng(31)
    img = P.img.copy()
    for b, n_obs in enumerate((72, 40, 5)):
        img[b, rng.permutation(144)[n_obs:]] = np.nan
    w = valid_weights(torch.tensor(img))
    masks = make_signal_masks(w, 16, 1, generator=torch.Generator().manual_seed(4), device="cpu")
    assert bool((masks[2, 5:] == -1).all()) and bool((masks[2, :5] >= 0).all()) and bool((masks[:2] >= 0).all())
    loss, fit = _run(P, cuda, "f32", masks, img=img, weights=w.to(cuda))
    assert bool(torch.isfinite(loss)) and all(bool(torch.isfinite(v).all()) for v in fit.values())
    loss1, fit1 = _run(P, cuda, "f32", masks[2:], img=np.nan_to_num(img[2:]))
    assert bool(torch.isfinite(loss1))
    for k in ("p_pos", "a"):
        init = _t(cuda)(P.lat0[k])
        upd = (fit1[k] - init).cpu().numpy()
        assert np.abs(upd).max() > 0
        e = rel((fit[k][2:] - init).cpu().numpy(), upd)
        print("short rows", k, e)
        assert e < TOL["f32"], (k, e)


def test_normalize_weights(cuda):
    """mean 1 over a signal's Ns samples.  A signal that is 25 % observed through padded masks -- 12 indices, 36 times -1 -- gets
    weights 48 / 12 = 4, so its loss is sum_i 4 d_i^2 / 48 = sum_i d_i^2 / 12: that of the same 12 points given four times each
    with weight 1.  One step; the f32 gradient tolerance on the latent updates."""
    ws = torch.tensor([[[1.0] * 12 + [0.0] * 36, [0.5] * 48, [0.0] * 48]])
    n = normalize_sampled_weights(ws)
    assert torch.equal(n[0, 0], torch.tensor([4.0] * 12 + [0.0] * 36)) and torch.equal(n[0, 1], torch.ones(48))
    assert torch.equal(n[0, 2], torch.zeros(48))
    P = _problem()
    rng = np.random.default_rng(41)
    img = P.img[:1]
    pts = np.stack([rng.permutation(144)[:12] for _ in range(2)], 1)                      # (12, S1): step 0 and the final loss
    padded = torch.tensor(np.concatenate([pts, np.full((36, 2), -1)], 0))[None]           # (1, 48, 2)
    repeated = torch.tensor(np.tile(pts, (4, 1)))[None]
    loss_p, fit_p = _run(P, cuda, "f32", padded, img=img, normalize_weights=True)
    loss_r, fit_r = _run(P, cuda, "f32", repeated, img=img, normalize_weights=True)
    loss_u, fit_u = _run(P, cuda, "f32", padded, img=img)                  # un-normalised: from the same start, a quarter of the step
    assert bool(torch.isfinite(loss_p)) and all(bool(torch.isfinite(v).all()) for v in fit_p.values())
    assert abs(float(loss_p) - float(loss_r)) < LOSS_TOL["f32"] * max(1.0, float(loss_r))
    for k in ("p_pos", "a"):
        init = _t(cuda)(P.lat0[k])
        upd = (fit_r[k] - init).cpu().numpy()
        e = rel((fit_p[k] - init).cpu().numpy(), upd)
        e4 = rel(4 * (fit_u[k] - init).cpu().numpy(), upd)
        print("normalize_weights", k, e, e4)
        assert e < TOL["f32"] and e4 < TOL["f32"], (k, e, e4)


# ---- 7. the trainer
def _trainer(cuda, sample_observed, n_s=48):
    from tests.test_ode_oracle import ode_cfg
    from tests.test_gpu_ode import _model
    from oracle import ode_ref_np as O
    from enf_pde_amd.fitting.trainers import MetaSGDPDETrainer
    from enf_pde_amd.enf.latents.autodecoder_meta import PositionOrientationFeatureAutodecoderMeta
    cfg = make_cfg("rel_pos_periodic", D=64, H=2, C=8, O=1)
    prm = R.init_params(0, cfg, jitter=0.1)
    ocfg = ode_cfg("rel_pos_periodic", num_hidden=16, basis_dim=16, num_layers=2)
    oprm = O.init_ponita_ode(1, ocfg, latent_dim=8, jitter=0.1, readout_scale=0.02)
    lin = np.linspace(-1, 1, 12)
    coords = np.stack(np.meshgrid(lin, lin), -1).reshape(-1, 2)
    conf = NS(optimizer=NS(learning_rate_enf=1e-3, learning_rate_codes=1e-3, learning_rate_ode=1e-3),
              meta=NS(learning_rate_meta_sgd=1e-2, num_inner_steps=2, inner_learning_rate_p=0.5, inner_learning_rate_a=2.0,
                      inner_learning_rate_window=0.0, noise_pos_inner_loop=0.0),
              nef=NS(optimize_gaussian_window=False), training=NS(max_num_sampled_points=n_s),
              node=NS(dt=1, method="euler"), dataset=NS(traj_len_train=3, traj_len_out_horizon=2))
    nef, ode = build_nef(cfg, "f32"), _model(ocfg, 8)
    t = _t(cuda)
    ad = PositionOrientationFeatureAutodecoderMeta(1, 9, 8, 2, 0, gaussian_window_size=-1)
    tr = MetaSGDPDETrainer(conf, nef, ad, t(coords), seed=0, second_order="fd", ode_model=ode, sample_observed=sample_observed)
    state = tr.init_train_state(nef.load_params(prm, device=cuda), ode_params=ode.load_params(oprm, device=cuda))
    return tr, state


def test_trainer_samples_observed_points(cuda, monkeypatch):
    from enf_pde_amd.fitting.trainers import pde_trainer as PT
    rng = np.random.default_rng(51)
    traj = rng.standard_normal((2, 5, 12, 12, 1))
    traj[0][rng.uniform(size=traj[0].shape) < 0.5] = np.nan                # half observed
    flat = traj[1].reshape(5, 144, 1)
    flat[:, rng.permutation(144)[20:]] = np.nan                           # 20 points of 144: rows padded with -1 at Ns = 48
    t = _t(cuda)
    batch = t(traj[:, 0])
    w = valid_weights(batch.reshape(2, 144, 1))
    assert w.sum(-1).tolist()[1] == 20.0
    drawn = []
    real = PT.make_signal_masks
    monkeypatch.setattr(PT, "make_signal_masks", lambda *a, **k: drawn.append(real(*a, **k)) or drawn[-1])
    losses = []
    for _ in range(2):
        tr, state = _trainer(cuda, True)
        before = [x.clone() for x in tr.nef.param_tensors(state.params["nef"]) if x is not None]
        lat_before = {k: v.clone() for k, v in state.params["autodecoder"]["params"].items()}
        lr_before = {k: v.clone() for k, v in state.params["meta_sgd_lrs"].items()}
        loss, new = tr.nef_train_step(state, batch, weights=w)
        losses.append(float(loss))
    assert len(drawn) == 2 and drawn[0].shape == (2, 48, 3) and torch.equal(drawn[0], drawn[1])
    assert bool((drawn[0][1, 20:] == -1).all()) and bool((drawn[0][0] >= 0).all())
    assert bool((w.cpu()[0][drawn[0][0].cpu().flatten()] > 0).all())
    assert np.isfinite(losses[0]) and losses[0] > 0
    assert abs(losses[0] - losses[1]) <= 1e-6 * abs(losses[0])            # same seed, same loss
    after = [x for x in tr.nef.param_tensors(new.params["nef"]) if x is not None]
    assert len(after) == len(before) and all(not torch.equal(a, b) for a, b in zip(before, after))       # every parameter moves
    assert all(bool(torch.isfinite(a).all()) for a in after)
    for k in ("p_pos", "a"):
        assert not torch.equal(lat_before[k], new.params["autodecoder"]["params"][k]), k
        assert not torch.equal(lr_before[k], new.params["meta_sgd_lrs"][k]), k
    # validation under point drop-out: two finite positive errors over all valid points; the masks are per signal
    tj = t(traj)
    wt = valid_weights(tj.reshape(2, 5, 144, 1))
    mse_in, mse_out = tr.val_step(new, tj, weights=wt, drop_rate=0.5)
    assert np.isfinite(float(mse_in)) and np.isfinite(float(mse_out)) and float(mse_in) > 0 and float(mse_out) > 0
    assert drawn[-1].shape == (2, 48, 3)
    # a fully observed trajectory needs no weights
    full = t(rng.standard_normal((2, 5, 12, 12, 1)))
    mse_in, mse_out = tr.val_step(new, full, drop_rate=0.5)
    assert np.isfinite(float(mse_in)) and np.isfinite(float(mse_out)) and float(mse_in) > 0 and float(mse_out) > 0
    assert drawn[-1].shape == (2, 48, 3) and bool((drawn[-1] >= 0).all())
    with pytest.raises(ValueError):
        tr.val_step(new, full, drop_rate=1.0)


def test_trainer_loss_keeps_its_scale_under_sample_observed(cuda, monkeypatch):
    """Pins the scale of the per-signal path against the shared one on the same observed points.  Every signal observes its own 48
    of the 144 points.  Trainer A, shared masks of all 144 points per step: its loss is the full-grid weighted mean,
    1 / 144 * sum over the 48 observed points of 3 d^2.  Trainer B, sample_observed with 48 points per signal, meets exactly the
    observed points in every step: with observed_sampling_weights the same sums, 1 / 48 * sum d^2 -- not 3 times them.  The two
    differ by fp32 summation order carried through two inner steps: 1e-4 relative on the loss (tests/test_gpu_weighted_fit.py's
    bound for a fit re-run in another order); the outer gradients by the tolerance of the meta-gradient tests, 2e-3 per tensor
    relative to the tensor's norm (to the largest norm for tensors below 1e-3 of it)."""
    from enf_pde_amd.fitting.trainers import pde_trainer as PT
    rng = np.random.default_rng(61)
    frame = rng.standard_normal((2, 144, 1))
    for b in range(2):
        frame[b, rng.permutation(144)[48:]] = np.nan
    batch = _t(cuda)(frame).reshape(2, 12, 12, 1)
    w = valid_weights(batch.reshape(2, 144, 1))
    assert w.sum(-1).tolist() == [48.0, 48.0]
    seen = []
    real = PT.meta_gradients

    def spy(*a, **k):
        seen.append(real(*a, **k))
        return seen[-1]
    monkeypatch.setattr(PT, "meta_gradients", spy)
    losses = []
    for sample_observed, n_s in ((False, 144), (True, 48)):
        tr, state = _trainer(cuda, sample_observed, n_s=n_s)
        loss, _ = tr.nef_train_step(state, batch, weights=w)
        losses.append(float(loss))
    print("loss scale", losses)
    assert np.isfinite(losses[0]) and losses[0] > 0
    assert abs(losses[1] - losses[0]) < 1e-4 * losses[0], losses
    (_, ga), (_, gb) = seen
    gmax = max(float(t.norm()) for t in ga["nef"] if t is not None)
    for i, (a, b) in enumerate(zip(ga["nef"], gb["nef"])):
        if a is None:
            continue
        na = float(a.norm())
        e = float((a - b).norm()) / (na if na > 1e-3 * gmax else gmax)
        assert e < 2e-3, (i, e)
    for group in ("autodecoder", "meta_sgd_lrs"):
        for k in ("p_pos", "a"):
            e = float((ga[group][k] - gb[group][k]).norm()) / max(float(ga[group][k].norm()), 1e-12)
            print("loss scale", group, k, e)
            assert e < 5e-3 if k == "p_pos" else e < 2e-3, (group, k, e)
