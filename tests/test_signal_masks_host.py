"""Per-signal point masks, host side (no GPU): the C-ABI declaration of enf_fit_inputs_b and its argument checks (nothing is
launched), the sampler make_signal_masks, the torch restatement of the gather, and that the shared-mask defaults of inner_loop
and of both trainers are what they were."""
import ctypes
import importlib
import os
import re
from types import SimpleNamespace as NS

import pytest
import torch

from enf_pde_amd import _lib

IL = importlib.import_module("enf_pde_amd.fitting.inner_loop")      # (the package's attribute of that name is the function)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, EDIM = -1, -6


def test_header_declares_and_lib_binds():
    with open(os.path.join(ROOT, "include", "enf_hip.h")) as f:
        h = f.read()
    assert re.search(r"\benf_fit_inputs_b\s*\(", h)
    assert "enf_fit_inputs_b" in _lib.EXPORTS
    assert re.search(r"#define\s+ENF_ABI_VERSION\s+2\b", h)
    assert ctypes.sizeof(_lib.EnfDesc) == 80
    lib = _lib.load()
    assert lib.enf_abi_version() == 2
    assert lib.enf_fit_inputs_b.argtypes is not None and len(lib.enf_fit_inputs_b.argtypes) == 18
    assert "never dereferenced" in h                         # the index contract is written down next to the declaration


def test_argument_checks_without_a_launch():
    lib = _lib.load()
    dummy = ctypes.create_string_buffer(64)
    P = ctypes.cast(dummy, ctypes.c_void_p)
    comps = (_lib.EnfFitComponent * _lib.ENF_SGD_MAX_SEGMENTS)()
    comps[0] = _lib.EnfFitComponent(P.value, P.value, 2, 0)

    def inputs(weight, ws, ncomp=1, xs=P, masks=P, N=50):
        return lib.enf_fit_inputs_b(ncomp, comps, 3, 4, N, 17, 4, 2, 1, P, P, masks, xs, P, P, weight, ws, None)
    assert inputs(P, None) == EINVAL and inputs(None, None) == EINVAL      # ws is required: it marks the indices outside [0, N)
    assert inputs(P, P, ncomp=0) == EINVAL and inputs(None, None, ncomp=5) == EINVAL
    assert inputs(P, P, xs=None) == EINVAL and inputs(None, P, masks=None) == EINVAL
    assert inputs(None, P, N=0) == EDIM


def _weights():
    g = torch.Generator().manual_seed(3)
    B, N = 3, 40
    w = torch.rand((B, N), generator=g)
    w[0, torch.randperm(N, generator=g)[:10]] = 0              # 30 observed points
    w[1, torch.randperm(N, generator=g)[:24]] = 0              # 16: exactly Ns
    w[2] = 0
    w[2, torch.tensor([3, 11, 17, 22, 39])] = 0.5              # 5: fewer than Ns
    return w


def test_make_signal_masks():
    w = _weights()
    B, N, Ns, S = 3, 40, 16, 2
    m = IL.make_signal_masks(w, Ns, S, generator=torch.Generator().manual_seed(5), device="cpu")
    assert m.shape == (B, Ns, S + 1) and m.dtype == torch.int64 and m.is_contiguous()
    n_valid = (w > 0).sum(-1)
    assert n_valid.tolist() == [30, 16, 5]
    for b in range(B):
        for s in range(S + 1):
            col = m[b, :, s]
            k = min(Ns, int(n_valid[b]))
            assert bool((col[:k] >= 0).all()) and bool((col[k:] == -1).all())           # -1 exactly when short, only at the end
            assert bool((col[:k] < N).all()) and bool((w[b, col[:k]] > 0).all())        # observed points only
            assert col[:k].unique().numel() == k                                        # no duplicates
    assert set(m[2, :5, 0].tolist()) == {3, 11, 17, 22, 39}                             # a short signal gets all it has
    assert not torch.equal(m[0, :, 0], m[0, :, 1])                                      # the steps are drawn independently
    again = IL.make_signal_masks(w, Ns, S, generator=torch.Generator().manual_seed(5), device="cpu")
    assert torch.equal(m, again)
    other = IL.make_signal_masks(w, Ns, S, generator=torch.Generator().manual_seed(6), device="cpu")
    assert not torch.equal(m, other)
    # a boolean validity pattern is taken like weights; more samples than grid points pad as well
    assert torch.equal(IL.make_signal_masks(w > 0, Ns, S, generator=torch.Generator().manual_seed(5), device="cpu"), m)
    big = IL.make_signal_masks(torch.ones(2, 6), 9, 0, generator=torch.Generator().manual_seed(0), device="cpu")
    assert big.shape == (2, 9, 1) and bool((big[:, 6:] == -1).all()) and sorted(big[0, :6, 0].tolist()) == list(range(6))
    with pytest.raises(ValueError):
        IL.make_signal_masks(torch.ones(6), 3, 0)


def test_make_signal_masks_is_uniform_over_the_observed_set():
    """Ns = 2 of 4 observed points, 3000 independent columns: every point is drawn with probability 1/2.  The count of one point is
    Binomial(3000, 1/2), sigma = 27.4; 6 sigma = 165."""
    w = torch.tensor([[1.0, 0.0, 2.0, 0.0, 3.0, 0.5]])
    m = IL.make_signal_masks(w, 2, 2999, generator=torch.Generator().manual_seed(1), device="cpu")
    counts = torch.bincount(m.flatten(), minlength=6)
    assert counts[1] == 0 and counts[3] == 0
    assert all(abs(int(counts[i]) - 1500) < 165 for i in (0, 2, 4, 5)), counts


def test_gather_signal_points_and_normalisation():
    g = torch.Generator().manual_seed(2)
    w = _weights()
    B, N, Ns, S1, O = 3, 40, 16, 3, 2
    coords, img = torch.randn((N, 2), generator=g), torch.randn((B, N, O), generator=g)
    img[w == 0] = float("nan")
    m = IL.make_signal_masks(w, Ns, S1 - 1, generator=g, device="cpu")
    m[0, 0, 0], m[0, 1, 0] = N, N + 7                                   # beyond the grid: treated like -1
    xs, ys, ws = IL.gather_signal_points(coords, img, m, w)
    assert xs.shape == (S1, B, Ns, 2) and ys.shape == (S1, B, Ns, O) and ws.shape == (S1, B, Ns)
    for s in range(S1):
        for b in range(B):
            for i in range(Ns):
                j = int(m[b, i, s])
                if 0 <= j < N:
                    assert torch.equal(xs[s, b, i], coords[j]) and torch.equal(ys[s, b, i], img[b, j]) and ws[s, b, i] == w[b, j]
                else:
                    assert torch.equal(xs[s, b, i], coords[0]) and bool((ys[s, b, i] == 0).all()) and ws[s, b, i] == 0
    assert not bool(torch.isnan(ys).any())                              # the sampler never picks an unobserved point
    _, _, unit = IL.gather_signal_points(coords, img, m, None)
    assert torch.equal(unit, ((m >= 0) & (m < N)).permute(2, 0, 1).float())
    # mean 1 over a signal's Ns samples: 5 valid samples of weight 0.5 become 16 / 5 each; a zero row stays zero
    n = IL.normalize_sampled_weights(ws)
    assert torch.allclose(n[1, 2, :5], torch.full((5,), 16 / 5)) and bool((n[1, 2, 5:] == 0).all())
    assert torch.allclose(n.mean(-1), torch.ones(S1, B), atol=1e-6)
    assert torch.equal(IL.normalize_sampled_weights(torch.zeros(2, 3, 4)), torch.zeros(2, 3, 4))


def _nef():
    from enf_pde_amd.enf.models import EquivariantCrossAttentionNeF
    from enf_pde_amd.enf.steerable_attention.invariant import get_ca_invariant
    inv = get_ca_invariant(NS(invariant_type="rel_pos_periodic", num_in=2))
    return EquivariantCrossAttentionNeF(num_hidden=128, num_heads=2, num_layers=0, num_out=1, latent_dim=16, cross_attn_invariant=inv,
                                        self_attn_invariant=inv, embedding_type="rff", embedding_freq_multiplier=(0.05, 0.1),
                                        condition_value_transform=True, use_gaussian_window=True, precision="f32")


def test_inner_loop_without_gpu_fails_loudly_for_both_mask_forms():
    nef = _nef()
    prm = nef.init(0, device="cpu")
    B, N, Z = 2, 20, 4
    lat0 = {"p_pos": torch.zeros(1, Z, 2), "a": torch.ones(1, Z, 16), "gaussian_window": torch.ones(1, Z, 1)}
    lrs = IL.default_meta_sgd_lrs(16, device="cpu")
    coords, img = torch.rand(N, 2), torch.rand(B, N, 1)
    shared = IL.make_masks(N, 8, 1, generator=torch.Generator().manual_seed(0), device="cpu")
    errors = []
    for masks in (shared, shared[None].expand(B, -1, -1).contiguous()):
        with pytest.raises(_lib.EnfError) as e:
            IL.inner_loop(nef, prm, lat0, lrs, coords, img, masks)
        errors.append(str(e.value))
    assert errors[0] == errors[1] and ("no CPU path" in errors[0] or "CUDA" in errors[0])
    with pytest.raises(ValueError):                                     # per-signal masks of another batch size
        IL.inner_loop(nef, prm, lat0, lrs, coords, img, shared[None].expand(B + 1, -1, -1).contiguous())


class _Stop(Exception):
    pass


def test_framework_route_with_per_signal_masks(monkeypatch):
    """The inner loop's route without enf_fit_inputs_b (CPU tensors never take it): every step is handed that step's per-signal
    points, targets and weights, x with a real batch stride; normalize_weights rescales the weights and nothing else."""
    g = torch.Generator().manual_seed(4)
    w = _weights()
    B, N, Ns, S, Z = 3, 40, 16, 2, 3
    coords, img = torch.randn((N, 2), generator=g), torch.randn((B, N, 1), generator=g)
    m = IL.make_signal_masks(w, Ns, S, generator=g, device="cpu")
    lat0 = {"p_pos": torch.zeros(1, Z, 2), "a": torch.ones(1, Z, 4), "gaussian_window": torch.ones(1, Z, 1)}
    seen = []

    class Nef:
        cross_attn_invariant = NS(num_z_ori_dims=0)

        def mse_value_and_latent_grads(self, params, x, p, a, window, target, grad_scale=1.0, loss_out=None, weight=None):
            seen.append((x, target, weight))
            return loss_out, torch.zeros_like(p), torch.zeros_like(a), torch.zeros_like(window)

        def apply(self, *a):
            raise _Stop

    monkeypatch.setattr(IL, "meta_sgd_update", lambda lat, grads, lrs, scale: lat)
    xs, ys, ws = IL.gather_signal_points(coords, img, m, w)
    for normalize in (False, True):
        seen.clear()
        with pytest.raises(_Stop):
            IL.inner_loop(Nef(), None, lat0, None, coords, img, m, weights=w, normalize_weights=normalize)
        assert len(seen) == S
        for s, (x, target, weight) in enumerate(seen):
            assert x.shape == (B, Ns, 2) and x.stride(0) == Ns * 2
            assert torch.equal(x, xs[s]) and torch.equal(target, ys[s])
            assert torch.equal(weight, IL.normalize_sampled_weights(ws)[s] if normalize else ws[s])
    with pytest.raises(ValueError):                                     # nothing to normalise: shared masks, no weights
        IL.inner_loop(Nef(), None, lat0, None, coords, img, IL.make_masks(N, Ns, S, device="cpu"), normalize_weights=True)


def _maml_trainer(sample_observed, N=30, n_s=8, S=2):
    from enf_pde_amd.fitting.trainers import MetaSGDPDETrainer, TrainState
    conf = NS(optimizer=NS(learning_rate_enf=1e-3, learning_rate_codes=0.0), meta=NS(learning_rate_meta_sgd=1e-2, num_inner_steps=S),
              nef=NS(optimize_gaussian_window=False), training=NS(max_num_sampled_points=n_s))
    tr = MetaSGDPDETrainer(conf, None, NS(num_ori_dims=0), torch.rand(N, 2), sample_observed=sample_observed)
    lat = {"p_pos": torch.zeros(1, 3, 2), "a": torch.ones(1, 3, 4), "gaussian_window": torch.ones(1, 3, 1)}
    state = TrainState(params={"nef": None, "autodecoder": {"params": lat}, "meta_sgd_lrs": {}}, nef_opt_state=None,
                       autodecoder_opt_state=None, meta_sgd_opt_state=None, rng=torch.Generator().manual_seed(11))
    return tr, state


def test_trainers_draw_the_shared_masks_they_drew(monkeypatch):
    """sample_observed=False (the default), with or without weights: nef_train_step and the fit of the ODE-phase steps hand on
    make_masks' draw from the state's generator.  sample_observed=True without weights does too; with weights the masks are
    make_signal_masks' draw."""
    from enf_pde_amd.fitting.trainers import pde_trainer as PT
    N, n_s, S, B = 30, 8, 2, 2
    w = torch.ones(B, N)
    w[0, :20] = 0
    w[1, 5:] = 0                                                         # 5 observed points: padded rows
    batch = torch.rand(B, N, 1)
    got = {}

    def stop(nef, params, lat0, lrs, coords, img, masks, **kw):
        got["masks"] = masks
        raise _Stop
    monkeypatch.setattr(PT, "meta_gradients", stop)
    expect = IL.make_masks(N, n_s, S, generator=torch.Generator().manual_seed(11), device="cpu")
    for sample_observed, weights in ((False, None), (False, w), (True, None)):
        tr, state = _maml_trainer(sample_observed)
        with pytest.raises(_Stop):
            tr.nef_train_step(state, batch, weights=weights)
        assert torch.equal(got["masks"], expect), (sample_observed, weights is None)
        tr, state = _maml_trainer(sample_observed)
        assert torch.equal(tr._fit_initial_latents(state, batch, weights=weights)[2], expect)
    tr, state = _maml_trainer(True)
    with pytest.raises(_Stop):
        tr.nef_train_step(state, batch, weights=w)
    assert torch.equal(got["masks"], IL.make_signal_masks(w, n_s, S, generator=torch.Generator().manual_seed(11), device="cpu"))
    assert got["masks"].shape == (B, n_s, S + 1) and bool((got["masks"][1, 5:] == -1).all())


def test_nonmaml_trainer_samples_as_before_by_default():
    from enf_pde_amd.fitting.trainers import NonMetaPDETrainer, NonMetaTrainState
    N, n_s, B = 30, 8, 2
    coords, img = torch.rand(N, 2), torch.rand(B, N, 1)
    w = torch.ones(B, N)
    w[0, :20] = 0
    w[1, 5:] = 0
    seen = {}

    class Nef:
        def param_tensors(self, params):
            return []

        def tensor_paths(self):
            return []

        def apply(self, params, xs, p, a, window):
            seen["xs"] = xs
            raise _Stop

    lat = {"p_pos": torch.zeros(4, 3, 2), "a": torch.ones(4, 3, 4)}
    ad = NS(apply=lambda params, idx: (params["params"]["p_pos"][idx], params["params"]["a"][idx], None))
    conf = NS(optimizer=NS(learning_rate_enf=1e-3, learning_rate_codes=1e-3), training=NS(max_num_sampled_points=n_s))

    def run(sample_observed, weights):
        tr = NonMetaPDETrainer(conf, Nef(), ad, coords, sample_observed=sample_observed)
        state = NonMetaTrainState(params={"nef": None, "autodecoder": {"params": lat}}, nef_opt_state=None, autodecoder_opt_state=None,
                                  rng=torch.Generator().manual_seed(7))
        with pytest.raises(_Stop):
            tr.loss_and_grads(state, img, torch.tensor([0, 2]), weights=weights, normalize=False)
        return seen["xs"]

    sub = torch.randperm(N, generator=torch.Generator().manual_seed(7))[:n_s]
    for sample_observed, weights in ((False, None), (False, w), (True, None)):
        xs = run(sample_observed, weights)
        assert xs.stride(0) == 0 and torch.equal(xs[0], coords[sub])
    xs = run(True, w)
    m = IL.make_signal_masks(w, n_s, 0, generator=torch.Generator().manual_seed(7), device="cpu")
    assert torch.equal(xs, IL.gather_signal_points(coords, img, m, w)[0][0]) and xs.stride(0) == n_s * 2


def test_observed_sampling_weights():
    """c_b = n_b / N * Ns / min(Ns, n_b).  With every observed point of signal b drawn with probability min(Ns, n_b) / n_b, the
    expectation of 1 / Ns * sum_i (c w)_i d_i^2 is 1 / N * sum_n w_n d_n^2, the full-grid weighted mean: checked in closed form
    (fp64, 1e-12) for a signal with more observed points than samples, one with exactly as many, a padded one and an empty one."""
    from enf_pde_amd.fitting.weights import observed_sampling_weights, normalize_point_weights
    g = torch.Generator().manual_seed(8)
    N, Ns = 40, 16
    w = torch.rand((4, N), generator=g, dtype=torch.float64) + 0.1
    for b, n_obs in enumerate((30, 16, 5, 0)):
        w[b, torch.randperm(N, generator=g)[n_obs:]] = 0
    d2 = torch.rand((4, N), generator=g, dtype=torch.float64)
    ws = observed_sampling_weights(w, Ns)
    assert torch.equal(ws == 0, w == 0) and bool((ws[3] == 0).all())
    for b, n_obs in enumerate((30, 16, 5)):
        prob = min(Ns, n_obs) / n_obs
        expect = float((prob * ws[b] * d2[b]).sum() / Ns)
        assert abs(expect - float((w[b] * d2[b]).sum() / N)) < 1e-12, b
    # 0/1 weights of mean 1 on the grid (1 / f on the observed points) become 1 where a signal has at least Ns points
    v = (w > 0).double()
    out = observed_sampling_weights(normalize_point_weights(v), Ns)
    assert torch.allclose(out[:2], v[:2], atol=1e-14)
    assert torch.allclose(out[2], v[2] * Ns / 5, atol=1e-14)              # padded: 5 samples stand for Ns
    # the drawn estimate itself, where it is exact (n_b <= Ns: every observed point is met once)
    m = IL.make_signal_masks(w, Ns, 0, generator=g, device="cpu")
    _, _, gathered = IL.gather_signal_points(torch.zeros(N, 2), d2[..., None].float(), m, ws.float())
    _, d2s, _ = IL.gather_signal_points(torch.zeros(N, 2), d2[..., None].float(), m, None)
    for b in (1, 2):
        got = float((gathered[0, b].double() * d2s[0, b, :, 0].double()).sum() / Ns)
        assert abs(got - float((w[b] * d2[b]).sum() / N)) < 1e-6, b


def test_nonmaml_loss_keeps_its_scale_under_sample_observed():
    """Every signal observes its own 10 of 30 points.  The shared subset is the whole grid (max_num_sampled_points = 30): the loss
    is the full-grid weighted mean.  sample_observed with 10 points per signal meets exactly the observed points: the same sum, so
    the same loss (fp32 sums in another order: 1e-6 relative) -- not 30 / 10 times it."""
    from enf_pde_amd.fitting.trainers import NonMetaPDETrainer, NonMetaTrainState
    g = torch.Generator().manual_seed(9)
    N, B = 30, 2
    coords, img = torch.rand((N, 2), generator=g), torch.rand((B, N, 1), generator=g)
    w = torch.zeros(B, N)
    for b in range(B):
        w[b, torch.randperm(N, generator=g)[:10]] = 1
    img[w == 0] = float("nan")

    class Nef:
        def param_tensors(self, params):
            return []

        def tensor_paths(self):
            return []

        def apply(self, params, xs, p, a, window):
            return xs.sum(-1, keepdim=True) * a.mean(dim=(1, 2))[:, None, None] + p.sum(dim=(1, 2))[:, None, None]

    lat = {"p_pos": torch.rand((4, 3, 2), generator=g), "a": torch.rand((4, 3, 4), generator=g)}
    ad = NS(apply=lambda params, idx: (params["params"]["p_pos"][idx], params["params"]["a"][idx], None))
    losses = {}
    for sample_observed, n_s in ((False, N), (True, 10)):
        conf = NS(optimizer=NS(learning_rate_enf=1e-3, learning_rate_codes=1e-3), training=NS(max_num_sampled_points=n_s))
        tr = NonMetaPDETrainer(conf, Nef(), ad, coords, sample_observed=sample_observed)
        state = NonMetaTrainState(params={"nef": None, "autodecoder": {"params": lat}}, nef_opt_state=None, autodecoder_opt_state=None,
                                  rng=torch.Generator().manual_seed(7))
        loss, _, ga = tr.loss_and_grads(state, img, torch.tensor([0, 2]), weights=w)
        losses[sample_observed] = (float(loss), ga["a"])
    assert losses[False][0] > 0
    assert abs(losses[True][0] - losses[False][0]) < 1e-6 * losses[False][0], losses
    assert torch.allclose(losses[True][1], losses[False][1], rtol=1e-5, atol=1e-8)
