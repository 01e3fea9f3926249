"""The trainers' loss weights on the host: fitting/weights.py: LossWeights against the public helpers it stands for, what every step
hands to the layer below for {no, per-point, per-channel} weights x sample_observed, and the steps that stay in torch with
per-point 0/1 weights against the same weights broadcast over the channels (bit for bit: every intermediate is exact).

Everything but the first section states behaviour the trainers had before the class existed, in terms of the public helpers only."""
from types import SimpleNamespace as NS

import pytest
import torch

from enf_pde_amd.fitting import weights as W
from enf_pde_amd.fitting.inner_loop import gather_signal_points, make_masks, make_signal_masks
from enf_pde_amd.fitting.trainers import latent_ode as LO
from enf_pde_amd.fitting.trainers import nonmaml_pde_trainer as NT
from enf_pde_amd.fitting.trainers import pde_trainer as PT
from tests.test_nonmaml_ode_host import _ToyDecoder, _toy

LossWeights = getattr(W, "LossWeights", None)
frame_weights = getattr(W, "frame_weights", None) or LO.frame_weights
frame_channel_weights = getattr(W, "frame_channel_weights", None) or LO.frame_channel_weights
needs_class = pytest.mark.skipif(LossWeights is None, reason="this tree has no LossWeights")

KINDS = ("none", "point", "channel")
B, N, O, T = 2, 6, 2, 3


# ---------------------------------------------------------------------------------------------- the class against the helpers
def _point_cases():
    """Every accepted shape of ``weights``: zeros inside, signal 1 of the batched forms all zero."""
    g = torch.Generator().manual_seed(0)
    w = torch.rand((B, T, N), generator=g) + 0.5
    w[0, :, 1] = 0
    w[0, 1, 4] = 0
    w[1] = 0
    return {"N": w[0, 0].clone(), "BN": w[:, 0].clone(), "BTN": w}


def _channel_cases():
    g = torch.Generator().manual_seed(1)
    cw = torch.rand((B, T, N, O), generator=g) + 0.5
    cw[0, :, 1] = 0                                                        # a point nobody observes
    cw[0, :, 2, 1] = 0                                                     # a point that lacks one variable
    cw[1] = 0
    return {"NO": cw[0, 0].clone(), "BNO": cw[:, 0].clone(), "BTNO": cw}


@needs_class
@pytest.mark.parametrize("normalize", [True, False])
def test_construction_equals_the_prepare_and_frame_helpers(normalize):
    assert LossWeights.build(None, None, B, N, O) is None and LossWeights.build(None, None, B, N, O, T=T, frames=0) is None
    for name, w in _point_cases().items():
        framed = LossWeights.build(w, None, B, N, O, T=T, normalize=normalize)
        assert not framed.channel and framed.w.dtype == torch.float32
        assert torch.equal(framed.w, frame_weights(w, B, T, N, normalize))
        w0 = w[:, 0] if name == "BTN" else w
        first = LossWeights.build(w, None, B, N, O, normalize=normalize, frames=0)
        assert not first.channel and torch.equal(first.w, W.prepare_point_weights(w0, B, N, normalize)) and first.w.is_contiguous()
        if name != "BTN":
            assert torch.equal(LossWeights.build(w, None, B, N, O, normalize=normalize).w, first.w)
    for name, cw in _channel_cases().items():
        framed = LossWeights.build(None, cw, B, N, O, T=T, normalize=normalize)
        assert framed.channel and torch.equal(framed.w, frame_channel_weights(cw, B, T, N, O, normalize))
        c0 = cw[:, 0] if name == "BTNO" else cw
        first = LossWeights.build(None, cw, B, N, O, normalize=normalize, frames=0)
        assert first.channel and torch.equal(first.w, W.prepare_channel_weights(c0, B, N, O, normalize)) and first.w.is_contiguous()
        if name != "BTNO":
            assert torch.equal(LossWeights.build(None, cw, B, N, O, normalize=normalize).w, first.w)


@needs_class
def test_frames_subsets_and_rescaling_equal_the_helper_pairs():
    w, cw = _point_cases()["BTN"], _channel_cases()["BTNO"]
    index = torch.tensor([4, 0, 2, 5])
    keep = torch.tensor([[1, 1, 0, 1, 1, 0], [1, 0, 1, 1, 0, 1]], dtype=torch.bool)
    # a frame range of the caller's weights, cut before they are prepared (what val_step does for its T frames)
    assert torch.equal(LossWeights.build(w, None, B, N, O, T=2, frames=slice(2)).w, frame_weights(w[:, :2], B, 2, N))
    assert torch.equal(LossWeights.build(None, cw, B, N, O, T=2, frames=slice(2)).w, frame_channel_weights(cw[:, :2], B, 2, N, O))
    assert W.cut_frames(w[:, 0], slice(2)) is not None and W.cut_frames(w[:, 0], slice(2)).shape == (B, N)       # no frame axis: kept
    assert W.cut_frames(cw[:, 0], slice(2), channel=True).shape == (B, N, O) and W.cut_frames(None, 0) is None
    for lw, ref, support, observed, renorm, per_point in (
            (LossWeights.build(w, None, B, N, O, frames=0), W.prepare_point_weights(w[:, 0], B, N), lambda t: t,
             W.observed_sampling_weights, W.normalize_point_weights, lambda t: t),
            (LossWeights.build(None, cw, B, N, O, frames=0), W.prepare_channel_weights(cw[:, 0], B, N, O), W.point_support,
             W.observed_channel_sampling_weights, W.normalize_channel_weights, lambda t: t[..., None])):
        assert torch.equal(lw.support(), support(ref)) and lw.support().shape == (B, N)
        assert torch.equal(lw.points(index).w, ref[:, index]) and lw.points(index).channel == lw.channel
        assert torch.equal(lw.keep(keep).w, ref * per_point(keep))
        assert torch.equal(lw.keep(keep).renormalized().w, renorm(ref * per_point(keep)))
        for n_s in (2, 4, 6):                                               # below, at and above signal 0's five (four) observed points
            assert torch.equal(lw.observed_draw(n_s).w, observed(ref, n_s))
        shared, per_signal = torch.zeros((4, 3), dtype=torch.long), torch.zeros((B, 4, 3), dtype=torch.long)
        assert lw.drawn_on(shared) is lw and torch.equal(lw.drawn_on(per_signal).w, observed(ref, 4))
    # a range of prepared frames (the two horizons of val_step) is a slice of them
    fw = LossWeights.build(w, None, B, N, O, T=T)
    assert torch.equal(fw.frame_range(0, 2).w, fw.w[:, :2]) and torch.equal(fw.frame_range(2, T).w, fw.w[:, 2:])


@needs_class
def test_hand_over_keywords():
    lw, lc = LossWeights.build(torch.ones(N), None, B, N, O), LossWeights.build(None, torch.ones(N, O), B, N, O)
    assert W.loop_kw(None) == {} and W.nef_kw(None) == {} and W.loss_tensor(None) is None
    assert list(W.loop_kw(lw)) == ["weights"] and W.loop_kw(lw)["weights"] is lw.w and W.loss_tensor(lw) is lw.w
    assert list(W.loop_kw(lc)) == ["channel_weights"] and W.loop_kw(lc)["channel_weights"] is lc.w
    assert list(W.nef_kw(lw)) == ["weight"] and W.nef_kw(lw)["weight"] is lw.w
    assert list(W.nef_kw(lc)) == ["channel_weight"] and W.nef_kw(lc)["channel_weight"] is lc.w
    with pytest.raises(Exception):                                         # immutable
        lw.channel = True


@needs_class
def test_errors_and_the_validation_asymmetry():
    w, cw = _point_cases(), _channel_cases()
    with pytest.raises(ValueError, match="^pass weights= or channel_weights=, not both$"):
        LossWeights.build(w["BN"], cw["BNO"], B, N, O)

    def same_error(build, helper):
        with pytest.raises(ValueError) as want:
            helper()
        with pytest.raises(ValueError) as got:
            build()
        assert str(got.value) == str(want.value)

    bad = torch.ones(B, N + 1)
    same_error(lambda: LossWeights.build(bad, None, B, N, O), lambda: W.prepare_point_weights(bad, B, N))
    same_error(lambda: LossWeights.build(bad, None, B, N, O, T=T), lambda: frame_weights(bad, B, T, N))
    same_error(lambda: LossWeights.build(torch.ones(N + 1), None, B, N, O), lambda: W.prepare_point_weights(torch.ones(N + 1), B, N))
    bad = torch.ones(B, T + 1, N)
    same_error(lambda: LossWeights.build(bad, None, B, N, O, T=T), lambda: frame_weights(bad, B, T, N))
    same_error(lambda: LossWeights.build(bad, None, B, N, O), lambda: W.prepare_point_weights(bad, B, N))
    bad = torch.ones(B, N, O + 1)
    same_error(lambda: LossWeights.build(None, bad, B, N, O), lambda: W.prepare_channel_weights(bad, B, N, O))
    same_error(lambda: LossWeights.build(None, bad, B, N, O, T=T), lambda: frame_channel_weights(bad, B, T, N, O))
    bad = torch.ones(B, T + 1, N, O)
    same_error(lambda: LossWeights.build(None, bad, B, N, O, T=T), lambda: frame_channel_weights(bad, B, T, N, O))
    # not finite and >= 0: an error wherever the weights are normalised; without that only channel weights are looked at
    neg, cneg = w["BN"].clone(), cw["BNO"].clone()
    neg[0, 0], cneg[0, 0, 0] = -1.0, -1.0
    assert torch.equal(LossWeights.build(neg, None, B, N, O, normalize=False).w, neg)
    assert torch.equal(LossWeights.build(neg, None, B, N, O, T=T, normalize=False).w, neg[:, None].expand(B, T, N))
    fneg = neg[:, None].expand(B, T, N).contiguous()
    assert torch.equal(LossWeights.build(fneg, None, B, N, O, T=T, normalize=False).w, fneg)
    same_error(lambda: LossWeights.build(neg, None, B, N, O), lambda: W.prepare_point_weights(neg, B, N))
    for normalize in (True, False):
        same_error(lambda: LossWeights.build(None, cneg, B, N, O, normalize=normalize),
                   lambda: W.prepare_channel_weights(cneg, B, N, O, normalize))
        fcneg = cneg[:, None].expand(B, T, N, O)
        same_error(lambda: LossWeights.build(None, fcneg, B, N, O, T=T, normalize=normalize),
                   lambda: frame_channel_weights(fcneg, B, T, N, O, normalize))
    with pytest.raises(ValueError, match="^channel weights must be finite and >= 0$"):
        LossWeights.build(None, cneg, B, N, O, normalize=False)


# ---------------------------------------------------------------------------------------------- what each step hands on
class _Stop(Exception):
    pass


GRID, N_S, STEPS, SIGNALS = 30, 8, 2, 2            # 30 grid points, 8 sampled; signal 1 observes 5 of them: padded rows


def _field(channels, frames=None):
    g = torch.Generator().manual_seed(3)
    return torch.rand((SIGNALS, GRID, channels) if frames is None else (SIGNALS, frames, GRID, channels), generator=g)


def _weights(kind, channels, frames=None):
    """The caller's weights of ``kind``, not normalised, with zeros; with ``frames`` one set per frame."""
    if kind == "none":
        return None
    g = torch.Generator().manual_seed(5)
    w = torch.rand((SIGNALS, frames or 1, GRID, channels), generator=g) + 0.5
    w[0, :, :12] = 0
    w[1, :, 5:] = 0
    if channels > 1:
        w[0, :, 12:20, 1] = 0                                              # observed in the first variable only
    w = w if kind == "channel" else w[..., 0]
    return w if frames else w[:, 0]


def _given(kind, w):
    return {} if kind == "none" else {"weights" if kind == "point" else "channel_weights": w}


def _prepared(kind, w, channels, normalize=True):
    if kind == "none":
        return None
    return W.prepare_point_weights(w, SIGNALS, w.shape[1], normalize) if kind == "point" else \
        W.prepare_channel_weights(w, SIGNALS, w.shape[1], channels, normalize)


def _support(kind, p):
    return p if kind == "point" else W.point_support(p)


def _observed(kind, p, n_s):
    return W.observed_sampling_weights(p, n_s) if kind == "point" else W.observed_channel_sampling_weights(p, n_s)


def _expected_fit(kind, w, channels, sample_observed, seed, steps):
    """(masks, weights, generator state) of a fit that draws its own masks from a generator seeded with ``seed``."""
    g = torch.Generator().manual_seed(seed)
    p = _prepared(kind, w, channels)
    if sample_observed and p is not None:
        masks = make_signal_masks(_support(kind, p), N_S, steps, generator=g, device="cpu")
        return masks, _observed(kind, p, N_S), g.get_state()
    return make_masks(GRID, N_S, steps, generator=g, device="cpu"), p, g.get_state()


def _fitted_with(kind, kw, channels, normalize=None):
    """The weights the layer below fits with, from the keywords it was handed: inner_loop takes them as they are, meta_gradients
    prepares them once more as its ``normalize`` keyword says."""
    assert kw.get("channel_weights" if kind != "channel" else "weights") is None
    w = kw.get("weights" if kind != "channel" else "channel_weights")
    if kind == "none":
        assert w is None
        return None
    return w if normalize is None else _prepared(kind, w, channels, normalize)


def _same(a, b):
    return (a is None and b is None) or (a is not None and b is not None and a.shape == b.shape and torch.equal(a, b))


def _maml_trainer(sample_observed):
    conf = NS(optimizer=NS(learning_rate_enf=1e-3, learning_rate_codes=0.0), meta=NS(learning_rate_meta_sgd=1e-2, num_inner_steps=STEPS),
              nef=NS(optimize_gaussian_window=False), training=NS(max_num_sampled_points=N_S),
              dataset=NS(traj_len_train=2, traj_len_out_horizon=1))
    tr = PT.MetaSGDPDETrainer(conf, None, NS(num_ori_dims=0), torch.rand(GRID, 2, generator=torch.Generator().manual_seed(2)),
                              sample_observed=sample_observed)
    lat = {"p_pos": torch.zeros(1, 3, 2), "a": torch.ones(1, 3, 4), "gaussian_window": torch.ones(1, 3, 1)}
    state = PT.TrainState(params={"nef": None, "autodecoder": {"params": lat}, "meta_sgd_lrs": {}}, nef_opt_state=None,
                          autodecoder_opt_state=None, meta_sgd_opt_state=None, rng=torch.Generator().manual_seed(11))
    return tr, state


@pytest.mark.parametrize("sample_observed", [False, True])
@pytest.mark.parametrize("kind", KINDS)
def test_maml_nef_train_step_hands_on(monkeypatch, kind, sample_observed):
    got = {}

    def stop(nef, params, lat0, lrs, coords, img, masks, **kw):
        got.update(masks=masks, kw=kw, img=img)
        raise _Stop
    monkeypatch.setattr(PT, "meta_gradients", stop)
    tr, state = _maml_trainer(sample_observed)
    batch, w = _field(2), _weights(kind, 2)
    with pytest.raises(_Stop):
        tr.nef_train_step(state, batch, **_given(kind, w))
    masks, fit_w, rng = _expected_fit(kind, w, 2, sample_observed, 11, STEPS)
    assert _same(got["masks"], masks) and torch.equal(got["img"], batch)
    assert _same(_fitted_with(kind, got["kw"], 2, got["kw"].get("normalize", True)), fit_w)
    assert got["kw"]["generator"] is state.rng and torch.equal(state.rng.get_state(), rng)


@pytest.mark.parametrize("drop_rate", [None, 0.5])
@pytest.mark.parametrize("sample_observed", [False, True])
@pytest.mark.parametrize("kind", KINDS)
def test_maml_val_step_hands_on(monkeypatch, kind, sample_observed, drop_rate):
    """The fit of val_step: frame 0's weights of per-frame input, the masks, and under drop-out the keep-mask drawn BEFORE them."""
    got = {}

    def stop(nef, params, lat0, lrs, coords, img, masks, **kw):
        got.update(masks=masks, kw=kw, img=img)
        raise _Stop
    monkeypatch.setattr(PT, "inner_loop", stop)
    tr, state = _maml_trainer(sample_observed)
    traj, w = _field(2, frames=4), _weights(kind, 2, frames=4)             # 4 frames given, 3 used
    with pytest.raises(_Stop):
        tr.val_step(state, traj, drop_rate=drop_rate, **_given(kind, w))
    w0 = None if w is None else w[:, 0]
    if drop_rate is None:
        masks, fit_w, rng = _expected_fit(kind, w0, 2, sample_observed, 11, STEPS)
    else:
        g = torch.Generator().manual_seed(11)
        kept = torch.rand((SIGNALS, GRID), generator=g) >= drop_rate
        p = _prepared(kind, w0, 2)
        if p is not None:
            kept &= _support(kind, p) > 0
        masks = make_signal_masks(kept, min(N_S, int((1.0 - drop_rate) * GRID)), STEPS, generator=g, device="cpu")
        rng = g.get_state()
        if kind == "channel":
            fit_w = W.observed_channel_sampling_weights(W.normalize_channel_weights(p * kept[..., None]), N_S)
        else:
            fit_w = W.observed_sampling_weights(W.normalize_point_weights(kept.float() if p is None else p * kept), N_S)
        kind = "point" if kind == "none" else kind                         # what was kept is what is observed: point weights
    assert _same(got["masks"], masks) and torch.equal(got["img"], traj[:, 0])
    assert _same(_fitted_with(kind, got["kw"], 2), fit_w)
    assert torch.equal(state.rng.get_state(), rng)


class _RecordingNef:
    """Stops at the first call of the decoder; ``apply`` returns zeros that depend on the latents so that a step can finish."""

    def __init__(self, stop_at):
        self.stop_at, self.seen = stop_at, {}

    def param_tensors(self, params):
        return []

    def tensor_paths(self):
        return []

    def apply(self, params, xs, p, a, window):
        self.seen.update(xs=xs)
        if self.stop_at == "apply":
            raise _Stop
        return (p.sum() + a.sum()) * 0 + torch.zeros(xs.shape[0], xs.shape[1], 1)

    def mse_value_and_latent_grads(self, params, xs, p, a, window, target, **kw):
        self.seen.update(xs=xs, target=target, kw=kw)
        raise _Stop


def _autodec_trainer(sample_observed, stop_at):
    coords = torch.rand(GRID, 2, generator=torch.Generator().manual_seed(2))
    lat = {"p_pos": torch.zeros(4, 3, 2), "a": torch.ones(4, 3, 4)}
    ad = NS(apply=lambda params, idx: (params["params"]["p_pos"][idx], params["params"]["a"][idx], None))
    conf = NS(optimizer=NS(learning_rate_enf=1e-3, learning_rate_codes=1e-3), training=NS(max_num_sampled_points=N_S))
    tr = NT.NonMetaPDETrainer(conf, _RecordingNef(stop_at), ad, coords, sample_observed=sample_observed)
    state = NT.NonMetaTrainState(params={"nef": None, "autodecoder": {"params": lat}}, nef_opt_state=None, autodecoder_opt_state=None,
                                 rng=torch.Generator().manual_seed(7))
    return tr, state


def _expected_points(kind, w, img, coords, sample_observed):
    """(xs (B, n, dx), targets, weights, generator state) of the one draw of an auto-decoder nef step."""
    g = torch.Generator().manual_seed(7)
    p = _prepared(kind, w, 1)
    if sample_observed and p is not None:
        m = make_signal_masks(_support(kind, p), N_S, 0, generator=g, device="cpu")
        xs, ys, ws = (t[0] for t in gather_signal_points(coords, img, m, _observed(kind, p, N_S)))
        return xs, ys, ws, g.get_state()
    sub = torch.randperm(GRID, generator=g)[:N_S]
    return coords[sub][None].expand(SIGNALS, -1, -1), img[:, sub], None if p is None else p[:, sub], g.get_state()


@pytest.mark.parametrize("sample_observed", [False, True])
@pytest.mark.parametrize("kind", KINDS)
def test_autodecoder_loss_and_grads_hands_on(monkeypatch, kind, sample_observed):
    tr, state = _autodec_trainer(sample_observed, stop_at=None)
    got = {}

    def record(out, target, weights=None):
        got.update(target=target, weights=weights)
        raise _Stop
    monkeypatch.setattr(NT, "weighted_mse", record)
    img, w = _field(1), _weights(kind, 1)
    if kind == "none":                                                     # the plain mean: the step finishes, nothing weighted is formed
        loss, gw, ga = tr.loss_and_grads(state, img, torch.tensor([0, 2]))
        assert got == {} and gw == [] and set(ga) == {"p_pos", "a"}
    else:
        with pytest.raises(_Stop):
            tr.loss_and_grads(state, img, torch.tensor([0, 2]), **_given(kind, w))
    xs, ys, ws, rng = _expected_points(kind, w, img, tr.coords, sample_observed)
    assert _same(tr.nef.seen["xs"], xs) and torch.equal(state.rng.get_state(), rng)
    if kind != "none":
        assert _same(got["target"], ys) and _same(got["weights"], ws)


@pytest.mark.parametrize("sample_observed", [False, True])
@pytest.mark.parametrize("kind", KINDS)
def test_autodecoder_fit_latents_step_hands_on(kind, sample_observed):
    tr, state = _autodec_trainer(sample_observed, stop_at="fit")
    img, w = _field(1), _weights(kind, 1)
    with pytest.raises(_Stop):
        tr.fit_latents_step(state, (img, torch.tensor([0, 2])), **_given(kind, w))
    xs, ys, ws, rng = _expected_points(kind, w, img, tr.coords, sample_observed)
    seen = tr.nef.seen
    assert _same(seen["xs"], xs) and _same(seen["target"], ys) and torch.equal(state.rng.get_state(), rng)
    assert set(seen["kw"]) <= {"weight", "channel_weight"}                  # (no return_errors without per_signal_loss)
    assert _same(seen["kw"].get("channel_weight" if kind == "channel" else "weight"), ws)
    assert seen["kw"].get("weight" if kind == "channel" else "channel_weight") is None


# ---------------------------------------------------------------------------------------------- broadcast equivalence in torch
class _Toy(_ToyDecoder):
    def tensor_paths(self):
        return self._nef.tensor_paths()


def _toy_problem():
    cfg, tr, st, traj, idx = _toy(n_s=24, grid=8)
    tr.nef = _Toy(tr.nef._nef)
    g = torch.Generator().manual_seed(9)
    w = (torch.rand((3, 64), generator=g) < 0.6).float()                   # 0/1, per signal
    nan = torch.full((), float("nan"))
    traj = torch.where(w[:, None, :, None] > 0, traj.reshape(3, 22, 64, 1), nan).reshape(traj.shape)       # NaN under the zeros
    return tr, st, traj, idx, w


def _tensors(tree):
    if isinstance(tree, torch.Tensor):
        return [tree]
    if isinstance(tree, dict):
        return [t for k in sorted(tree) for t in _tensors(tree[k])]
    if isinstance(tree, (list, tuple)):
        return [t for v in tree for t in _tensors(v)]
    return []


def _state_tensors(st):
    return _tensors([st.params, st.nef_opt_state, st.autodecoder_opt_state, st.ode_opt_state]) + [st.rng.get_state()]


def test_broadcast_point_weights_in_the_torch_only_steps():
    """0/1 weights (B, N) against the same weights repeated over the channels, (B, N, O): NonMetaPDETrainer.nef_train_step, val_step
    and rollout_loss agree bit for bit (NaN under the zeros)."""
    results = []
    for form in ("point", "channel"):
        tr, st, traj, idx, w = _toy_problem()
        kw = {"weights": w} if form == "point" else {"channel_weights": w[..., None].expand(3, 64, 1)}
        loss, new = tr.nef_train_step(st, (traj[:, 0], idx), **kw)
        e_in, e_out = tr.val_step(new, (traj, idx), **kw)
        pm = LO.draw_point_masks(64, 24, 10, torch.Generator().manual_seed(1))
        z0 = tr.autodecoder.apply(new.params["autodecoder"], idx)
        roll = tr.rollout_loss(new.params["nef"], new.params["ode_params"], z0, traj[:, :10], pm, **kw)
        assert all(bool(torch.isfinite(v)) for v in (loss, e_in, e_out, roll)) and float(loss) > 0 and float(roll) > 0
        results.append([loss, e_in, e_out, roll.detach()] + _state_tensors(new))
    assert len(results[0]) == len(results[1]) > 10
    for i, (a, b) in enumerate(zip(*results)):
        assert torch.equal(a, b), i
