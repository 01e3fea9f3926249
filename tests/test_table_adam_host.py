"""Host side of the latent-only fit path (nonmaml_pde_trainer.py:139-171, 399-548): the binding of enf_table_adam_update and its
rejection cases (they return before any launch), table_adam_update on CPU tensors against float64 optax adam, and -- with a small
differentiable stand-in for the decoder, which has no CPU path -- the bookkeeping of fit_latents_step and validate_epoch."""
import ctypes
import os
import re
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

from enf_pde_amd import _lib
from enf_pde_amd.enf.latents.autodecoder import PositionOrientationFeatureAutodecoder
from enf_pde_amd.fitting.ode_models import MLPODE
from enf_pde_amd.fitting.optim import Adam, AdamW, scatter_rows, table_adam_update
from enf_pde_amd.fitting.trainers import NonMetaPDETrainer, NonMetaTrainState
from enf_pde_amd.fitting.weights import weighted_mse
from tests import table_adam_ref as TA

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, EDIM = -1, -6


def test_segment_struct_matches_header():
    hdr = open(os.path.join(ROOT, "include", "enf_hip.h")).read()
    body = hdr[hdr.index("typedef struct EnfAdamSegment {"):hdr.index("} EnfAdamSegment;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for kind, names in re.findall(r"\b(const float\*|float\*|int32_t)\s+([^;]+);", body):
        fields += [(n.strip(), kind) for n in names.split(",")]
    assert [n for n, _ in fields] == [f[0] for f in _lib.EnfAdamSegment._fields_]
    assert [n for n, _ in fields] == ["x", "mu", "nu", "g", "x_out", "mu_out", "nu_out", "width", "g_stride"]
    for (n, kind), (_, ctype) in zip(fields, _lib.EnfAdamSegment._fields_):
        assert ctype is (ctypes.c_int32 if kind == "int32_t" else ctypes.c_void_p), n
    assert ctypes.sizeof(_lib.EnfAdamSegment) == 7 * 8 + 2 * 4
    assert _lib.EnfAdamSegment.width.offset == 56 and _lib.EnfAdamSegment.g_stride.offset == 60
    assert re.search(r"#define ENF_ADAM_MAX_SEGMENTS (\d)", hdr).group(1) == str(_lib.ENF_ADAM_MAX_SEGMENTS)
    assert "enf_table_adam_update" in _lib.EXPORTS and hasattr(_lib.load(), "enf_table_adam_update")
    assert _lib.load().enf_abi_version() == 2                      # additive: the ABI version stays


def test_entry_point_rejects_bad_arguments_before_any_launch():
    lib = _lib.load()
    buf = (ctypes.c_float * 64)()                                  # host memory: only its address is looked at
    ptr = ctypes.addressof(buf)
    idx = (ctypes.c_int64 * 3)(4, 0, 2)

    def call(nseg=1, segs="default", S=5, Z=5, idx=ctypes.addressof(idx), nidx=3, c1=0.1, c2=0.001, **field):
        arr = (_lib.EnfAdamSegment * _lib.ENF_ADAM_MAX_SEGMENTS)()
        for k in range(_lib.ENF_ADAM_MAX_SEGMENTS):
            arr[k] = _lib.EnfAdamSegment(ptr, ptr, ptr, ptr, ptr, ptr, ptr, 2, 3)
        for name, val in field.items():
            setattr(arr[0], name, val)
        return lib.enf_table_adam_update(nseg, arr if segs == "default" else segs, S, Z, idx, nidx, 1e-3, 0.9, 0.999, 1e-8, c1, c2, None)

    for kw in (dict(nseg=0), dict(nseg=5), dict(nseg=-1), dict(segs=None), dict(S=0), dict(S=-3), dict(Z=0), dict(nidx=0), dict(nidx=-1),
               dict(width=0), dict(width=-2), dict(c1=0.0), dict(c2=0.0), dict(c1=-0.5), dict(c2=float("nan")),
               dict(x=None), dict(mu=None), dict(nu=None), dict(g=None), dict(x_out=None), dict(mu_out=None), dict(nu_out=None)):
        assert call(**kw) == EINVAL, kw
    assert call(g_stride=1) == EDIM                                # rows of g would overlap
    assert call(idx=None, nidx=3) == EDIM                          # a dense gradient has S rows
    assert call(idx=None, nidx=5, g_stride=1) == EDIM
    # ENF_EINVAL comes first
    assert call(g_stride=1, c1=0.0) == EINVAL and call(idx=None, nidx=3, nu_out=None) == EINVAL
    assert call(nseg=2, g_stride=1) == EDIM                        # every segment of the call is looked at ...
    assert call(nseg=4, Z=0) == EINVAL
    assert lib.enf_strerror(EDIM) and lib.enf_strerror(EINVAL)


@pytest.mark.parametrize("count", [1, 7])
@pytest.mark.parametrize("idx", [[4, 0, 2], [1, 1, 3], [2, -1, 9], None])
def test_table_adam_update_on_cpu_tensors_is_optax_adam(idx, count):
    lr = 1e-2
    tables, mu, nu, grads = TA.problem(idx, count)
    opt = Adam(lr)
    state = {"count": count - 1, "mu": mu, "nu": nu}
    before = [t.clone() for t in tables + mu + nu]
    new, st = table_adam_update(opt, state, tables, grads, idx=None if idx is None else torch.tensor(idx))
    assert st["count"] == count and state["count"] == count - 1
    assert all(torch.equal(a, b) for a, b in zip(tables + mu + nu, before))            # out of place by default
    ref = TA.reference(tables, mu, nu, grads, idx, count, lr)
    TA.check(new, st["mu"], st["nu"], ref, lr, label=f"cpu idx={idx} count={count}")
    if idx is not None:                                                                # rows outside the batch: momentum only
        out = [s for s in range(5) if s not in idx]
        b1 = torch.tensor(TA.B1)
        for k in range(4):
            assert torch.equal(st["mu"][k][out], b1 * mu[k][out])
            assert bool((new[k][out] == tables[k][out]).all()) == (count == 1)          # zero moments: they stay where they are
    if idx == [1, 1, 3]:                                                               # duplicates equal the sum
        summed = [torch.stack((g[0] + g[1], g[2])) for g in grads]
        new2, st2 = table_adam_update(opt, state, tables, summed, idx=torch.tensor([1, 3]))
        assert all(torch.equal(a, b) for a, b in zip(new + st["mu"] + st["nu"], new2 + st2["mu"] + st2["nu"]))
    # in place
    t2, m2, n2 = ([t.clone() for t in ts] for ts in (tables, mu, nu))
    new3, st3 = table_adam_update(opt, {"count": count - 1, "mu": m2, "nu": n2}, t2, grads,
                                  idx=None if idx is None else torch.tensor(idx), inplace=True)
    assert all(a is b for a, b in zip(new3 + st3["mu"] + st3["nu"], t2 + m2 + n2))
    assert all(torch.equal(a, b) for a, b in zip(new3 + st3["mu"] + st3["nu"], new + st["mu"] + st["nu"]))


def test_table_adam_update_follows_adam_update_and_refuses_what_it_is_not():
    """The existing dense rule (Adam.update on scattered gradients) and the table update agree over several steps; the bias
    corrections come from the float32 decay rates (optim._table_adam_scalars)."""
    tables, _, _, _ = TA.problem([4, 0, 2], 1)
    opt = Adam(3e-3)
    s_old, s_new = opt.init(tables), opt.init(tables)
    x_old, x_new = tables, tables
    for step, idx in enumerate(([4, 0, 2], [1, 1, 3], [0, 3, 4])):
        _, _, _, grads = TA.problem(idx, 1, seed=step + 1)
        x_old, s_old = opt.update(scatter_rows(grads, idx, 5), s_old, x_old)
        x_new, s_new = table_adam_update(opt, s_new, x_new, grads, idx=torch.tensor(idx))
    for a, b in zip(x_new + s_new["mu"] + s_new["nu"], x_old + s_old["mu"] + s_old["nu"]):
        torch.testing.assert_close(a, b, rtol=2e-5, atol=1e-7)
    assert s_new["count"] == 3
    with pytest.raises(ValueError, match="weight decay"):
        table_adam_update(AdamW(1e-3), opt.init(tables), tables, grads, idx=torch.tensor([0, 3, 4]))
    with pytest.raises(ValueError, match="expected"):
        table_adam_update(opt, opt.init(tables), tables, [g[:2] for g in grads], idx=torch.tensor([0, 3, 4]))
    with pytest.raises(ValueError, match="expected"):
        table_adam_update(opt, opt.init(tables), tables, grads, idx=None)                  # dense needs S rows


# ---------------------------------------------------------------------------------------------------------------------
class _ToyNef:
    """A differentiable stand-in with the decoder's calling convention (the HIP decoder raises on host tensors): gaussian bumps at
    the latent positions, weighted by a projection of ``a`` and, where the pose carries one, the cosine of the orientation.
    ``mse_value_and_latent_grads`` is what the product's returns: the loss (1,) and its gradient w.r.t. (p, a, window)."""

    def __init__(self, latent_dim, cross_attn_invariant=None):
        self.w = torch.linspace(-1, 1, latent_dim)
        self.cross_attn_invariant = cross_attn_invariant
        self.seen = []

    def param_tensors(self, params):
        return []

    def tensor_paths(self):
        return []

    def apply(self, params, x, p, a, window):
        self.seen.append(("apply", x.detach().clone(), x.stride(0), None))
        return self._out(x, p, a, window)

    def _out(self, x, p, a, window):
        d2 = ((x[:, :, None, :] - p[:, None, :, :2]) ** 2).sum(-1)
        amp = a @ self.w.to(a.dtype)
        if p.shape[-1] > 2:
            amp = amp * torch.cos(p[..., 2])
        return (torch.exp(-d2 / window[:, None, :, 0] ** 2) * amp[:, None, :]).sum(-1, keepdim=True)

    def mse_value_and_latent_grads(self, params, x, p, a, window, target, grad_scale=1.0, loss_out=None, weight=None):
        assert not torch.is_grad_enabled()                                             # the step builds no autograd graph
        self.seen.append(("fit", x.detach().clone(), x.stride(0), weight))
        with torch.enable_grad():
            leaves = [t.detach().clone().requires_grad_(True) for t in (p, a, window)]
            loss = weighted_mse(self._out(x, *leaves), target, weight)
            g = torch.autograd.grad(loss, leaves)
        return loss.detach().reshape(1), g[0], g[1], g[2]


def _grid(side=8):
    lin = torch.linspace(-1, 1, side)
    return torch.stack(torch.meshgrid(lin, lin, indexing="xy"), -1).reshape(-1, 2)


def _fit_trainer(n_s, sample_observed=False, ori=1, seed=5):
    conf = NS(optimizer=NS(learning_rate_enf=1e-4, learning_rate_codes=1e-2), training=NS(max_num_sampled_points=n_s))
    ad = PositionOrientationFeatureAutodecoder(6, 4, 8, 2, ori, gaussian_window_size=-1)
    tr = NonMetaPDETrainer(conf, _ToyNef(8), ad, _grid(), seed=0, sample_observed=sample_observed)
    g = torch.Generator().manual_seed(seed)
    table = ad.init(device="cpu")
    P = table["params"]
    P["a"] = P["a"] + 0.2 * torch.randn(P["a"].shape, generator=g)
    opt_state = tr.autodecoder_opt.init(list(P.values()))
    opt_state = {"count": 2, "mu": [0.01 * torch.randn(t.shape, generator=g) for t in opt_state["mu"]],
                 "nu": [1e-4 * torch.rand(t.shape, generator=g) + 1e-6 for t in opt_state["nu"]]}
    state = lambda: NonMetaTrainState(params={"nef": None, "autodecoder": table, "ode_params": "ode"}, nef_opt_state="nef-opt",
                                      autodecoder_opt_state=opt_state, ode_opt_state="ode-opt", step=11,
                                      rng=torch.Generator().manual_seed(7))
    img = torch.randn(3, 8, 8, 1, generator=g)
    return tr, state, img, torch.tensor([4, 0, 2])


@pytest.mark.parametrize("case", ["whole grid", "subset", "mask", "mask and subset", "weights", "sample_observed"])
def test_fit_latents_step_draws_and_steps_like_the_autodec_only_step(case):
    """Same generator consumption, same points, same loss and -- the toy decoder being differentiable -- the same Adam step as
    nef_train_step_autodec_only, to float32 rounding; everything else of the state is handed on."""
    n_s = 64 if case in ("whole grid", "mask") else 37
    tr, state, img, idx = _fit_trainer(n_s, sample_observed=case == "sample_observed")
    kw = {}
    if case.startswith("mask"):
        kw["mask"] = torch.randperm(64, generator=torch.Generator().manual_seed(1))[:50]
    if case in ("weights", "sample_observed"):
        img = img.clone()
        holes = torch.rand(3, 64, generator=torch.Generator().manual_seed(2)) < 0.3
        img.reshape(3, 64, 1)[holes] = float("nan")
        kw["weights"] = torch.isfinite(img.reshape(3, 64, 1)).all(-1).float()
    old_state, new_state = state(), state()
    loss_old, old = tr.nef_train_step_autodec_only(old_state, (img, idx), **kw)
    loss_new, new = tr.fit_latents_step(new_state, (img, idx), **kw)
    assert torch.equal(old_state.rng.get_state(), new_state.rng.get_state())
    drew = not torch.equal(new_state.rng.get_state(), torch.Generator().manual_seed(7).get_state())
    assert drew == (case not in ("whole grid", "mask"))
    (kind_a, x_a, stride_a, _), (kind_b, x_b, stride_b, w_b) = tr.nef.seen
    assert (kind_a, kind_b) == ("apply", "fit") and torch.equal(x_a, x_b) and stride_a == stride_b
    n = min(n_s, 50 if case.startswith("mask") else 64)
    assert x_b.shape == (3, n, 2) and stride_b == (n * 2 if case == "sample_observed" else 0)      # x_bstride: per signal or shared
    assert (w_b is None) == (case not in ("weights", "sample_observed")) and (w_b is None or w_b.shape == (3, n))
    assert np.isfinite(float(loss_new)) and loss_new.shape == ()
    assert abs(float(loss_new) - float(loss_old)) <= 1e-6 * abs(float(loss_old))
    P_old, P_new = old.params["autodecoder"]["params"], new.params["autodecoder"]["params"]
    assert list(P_new) == ["p_pos", "p_ori", "a", "gaussian_window"] == list(P_old)
    lr = tr.autodecoder_opt.lr
    for k in P_new:
        torch.testing.assert_close(P_new[k], P_old[k], rtol=1e-6, atol=1e-3 * lr)          # an update is at most ~lr per element
        assert not torch.equal(P_new[k], new_state.params["autodecoder"]["params"][k])
    for part, tol in (("mu", 1e-5), ("nu", 2e-5)):
        for a, b in zip(new.autodecoder_opt_state[part], old.autodecoder_opt_state[part]):
            assert float((a - b).abs().max()) <= tol * float(b.abs().max()), part
    assert new.autodecoder_opt_state["count"] == 3 and new_state.autodecoder_opt_state["count"] == 2
    assert new.params["nef"] is None and new.params["ode_params"] == "ode" and new.nef_opt_state == "nef-opt"
    assert new.ode_opt_state == "ode-opt" and new.step == 12 and new.rng is new_state.rng
    # rows outside the batch moved by momentum only: the same for both, and not by a gradient
    b1 = torch.tensor(TA.B1)
    for k, m0 in zip(range(4), new_state.autodecoder_opt_state["mu"]):
        assert torch.equal(new.autodecoder_opt_state["mu"][k][[1, 3, 5]], b1 * m0[[1, 3, 5]])


def test_fit_latents_step_without_an_orientation_or_a_window_gradient():
    tr, state, img, idx = _fit_trainer(37, ori=0)
    st = state()
    inner = tr.nef.mse_value_and_latent_grads
    tr.nef.mse_value_and_latent_grads = lambda *a, **k: inner(*a, **k)[:3] + (None,)     # a decoder without a gaussian window
    loss, new = tr.fit_latents_step(st, (img, idx))
    P0, P1 = st.params["autodecoder"]["params"], new.params["autodecoder"]["params"]
    assert list(P1) == ["p_pos", "a", "gaussian_window"] and P1["p_pos"].shape == (6, 4, 2)
    assert not torch.equal(P1["a"][idx], P0["a"][idx])
    i = list(P1).index("gaussian_window")
    assert torch.equal(new.autodecoder_opt_state["mu"][i], torch.tensor(TA.B1) * st.autodecoder_opt_state["mu"][i])   # zero gradient


# ---------------------------------------------------------------------------------------------------------------------
def _val_trainer(train_until=4, n_s=24):
    from tests.test_nonmaml_ode_host import _cfg
    from enf_pde_amd.fitting import get_model_pde
    cfg = _cfg(n_s=n_s, nef=(0, train_until))
    nef, _ = get_model_pde(cfg)
    ode = MLPODE(num_hidden=16, num_layers=3, scalar_num_out=16, vec_num_out=1)
    ad = PositionOrientationFeatureAutodecoder(6, 4, 16, 2, 0, gaussian_window_size=-1)
    val_ad = PositionOrientationFeatureAutodecoder(4, 4, 16, 2, 0, gaussian_window_size=-1)
    tr = NonMetaPDETrainer(cfg, nef, ad, _grid(), seed=0, ode_model=ode)
    st = tr.init_train_state()
    tr.nef = _ToyNef(16, nef.cross_attn_invariant)
    g = torch.Generator().manual_seed(8)
    P = st.params["autodecoder"]["params"]
    P["a"] = P["a"] + 0.2 * torch.randn(P["a"].shape, generator=g)
    train = [(torch.randn(3, 12, 8, 8, 1, generator=g), None, torch.tensor(i)) for i in ([4, 0, 5], [1, 2, 3])]
    val = [(torch.randn(2, 12, 8, 8, 1, generator=g), torch.tensor(i)) for i in ([0, 1], [3, 2])]   # the two-element batch form
    return tr, st, train, val, val_ad


KEYS = {"train_mse_in_t_sc", "train_mse_out_t_sc"} | {f"{s}_mse_{io}_t{d}" for s in ("val", "train") for io in ("in", "out")
                                                      for d in ("", "_dp0.05", "_dp0.1", "_dp0.5")}


def test_validate_epoch_protocol():
    """Which fits and roll-outs validate_epoch runs: the reference's keys, train_until_epoch - 1 passes, a fresh table and Adam
    state per fit, frame 0 as the target, and a drop-out mask that KEEPS int(N * rate) points, shared by the two fits of a rate."""
    tr, st, train, val, val_ad = _val_trainer(train_until=4)
    fits, rolls = [], []

    def fit_step(state, batch, mask=None, **kw):
        fits.append(NS(state=state, batch=batch, mask=mask))
        table = {k: v + 1 for k, v in state.params["autodecoder"]["params"].items()}
        opt = dict(state.autodecoder_opt_state, count=state.autodecoder_opt_state["count"] + 1)
        return torch.tensor(0.5), NonMetaTrainState(params=dict(state.params, autodecoder={"params": table}), nef_opt_state=state.nef_opt_state,
                                                    autodecoder_opt_state=opt, ode_opt_state=state.ode_opt_state, step=state.step + 1, rng=state.rng)

    def val_step(state, batch, autodecoder=None, **kw):
        rolls.append(NS(state=state, batch=batch, shell=autodecoder))
        return torch.tensor(float(len(rolls))), torch.tensor(10.0 * len(rolls))

    tr.fit_latents_step, tr.val_step = fit_step, val_step
    metrics, last = tr.validate_epoch(st, train, val, val_ad)
    assert set(metrics) == KEYS and all(type(v) is float for v in metrics.values())
    # 1 stored-table pass over the train loader, then per rate a validation and a training roll-out pass: 2 + 4 * (2 + 2) calls
    assert len(rolls) == 2 + 4 * 4 and len(fits) == 4 * (3 * 2 + 3 * 2)                    # train_until_epoch - 1 = 3 passes
    assert metrics["train_mse_in_t_sc"] == 1.5 and metrics["train_mse_out_t_sc"] == 15.0   # the mean over the loader
    assert metrics["val_mse_in_t"] == 3.5 and metrics["train_mse_out_t"] == 55.0 and metrics["val_mse_in_t_dp0.05"] == 7.5
    assert rolls[0].state is st and rolls[0].shell is tr.autodecoder
    per_rate = [fits[12 * r:12 * r + 12] for r in range(4)]
    for rate, calls in zip((0.0, 0.05, 0.1, 0.5), per_rate):
        keep = int(64 * rate)
        for c in calls:
            assert (c.mask is None) if rate == 0 else (c.mask.shape == (keep,) and len(set(c.mask.tolist())) == keep)
            assert c.mask is calls[0].mask                                                 # drawn once per rate, shared by both fits
            assert c.state.params["nef"] is st.params["nef"] and c.state.params["ode_params"] is st.params["ode_params"]
            assert c.state.rng is st.rng and c.state.ode_opt_state is st.ode_opt_state
        for first, shell, loader in ((calls[0], val_ad, val), (calls[6], tr.autodecoder, train)):
            fresh = shell.init(device="cpu")["params"]
            P = first.state.params["autodecoder"]["params"]
            assert list(P) == list(fresh) and all(torch.equal(P[k], fresh[k]) for k in fresh)
            s = first.state.autodecoder_opt_state
            assert s["count"] == 0 and not any(bool(t.any()) for t in s["mu"] + s["nu"])
            assert [t.shape for t in s["mu"]] == [v.shape for v in fresh.values()]
        for j, c in enumerate(calls):                                                      # frame 0 of the loader's batches, in order
            src = (val if j < 6 else train)[j % 2]
            assert torch.equal(c.batch[0], src[0][:, 0]) and c.batch[1] is src[-1] and len(c.batch) == 2
        assert calls[5].state.autodecoder_opt_state["count"] == 5                          # one state threaded through the fit
    assert (per_rate[1][0].mask.shape[0], per_rate[2][0].mask.shape[0], per_rate[3][0].mask.shape[0]) == (3, 6, 32)
    # the roll-outs of a rate read the FITTED tables through the right shell
    assert rolls[2].shell is val_ad and rolls[2].state.autodecoder_opt_state["count"] == 6 and rolls[4].shell is tr.autodecoder
    assert last is rolls[-3].state                                                         # the last validation state
    # explicit epochs, rates, no training fit
    fits.clear(), rolls.clear()
    metrics, _ = tr.validate_epoch(st, train, val, val_ad, drop_rates=(0.0, 0.5), epochs=1, fit_train=False)
    assert set(metrics) == {"train_mse_in_t_sc", "train_mse_out_t_sc", "val_mse_in_t", "val_mse_out_t", "val_mse_in_t_dp0.5",
                            "val_mse_out_t_dp0.5"}
    assert len(fits) == 2 * 2 and len(rolls) == 2 + 2 * 2
    cfg, plain = NS(), NonMetaPDETrainer(tr.config, tr.nef, tr.autodecoder, tr.coords)
    with pytest.raises(ValueError, match="ode_model"):
        plain.validate_epoch(st, train, val, val_ad)


def test_validate_epoch_runs_end_to_end_on_the_host_and_only_reads_the_state():
    tr, st, train, val, val_ad = _val_trainer(train_until=3)
    before = {k: v.clone() for k, v in st.params["autodecoder"]["params"].items()}
    opt_before = [t.clone() for t in st.autodecoder_opt_state["mu"] + st.autodecoder_opt_state["nu"]]
    metrics, last = tr.validate_epoch(st, train, val, val_ad, drop_rates=(0.0, 0.5))
    assert set(metrics) == {k for k in KEYS if "dp0.05" not in k and "dp0.1" not in k}
    assert all(np.isfinite(v) for v in metrics.values())
    fit_calls = [s for s in tr.nef.seen if s[0] == "fit"]
    assert len(fit_calls) == 2 * 2 * (2 + 2)                                               # 2 rates x 2 passes x (2 + 2) batches
    assert {tuple(s[1].shape[1:]) for s in fit_calls} == {(24, 2)}                          # 64 -> 24 points; the kept 32 -> 24
    assert all(torch.equal(v, before[k]) for k, v in st.params["autodecoder"]["params"].items())
    assert all(torch.equal(a, b) for a, b in zip(st.autodecoder_opt_state["mu"] + st.autodecoder_opt_state["nu"], opt_before))
    assert st.autodecoder_opt_state["count"] == 0 and st.step == 0
    P = last.params["autodecoder"]["params"]
    assert P["a"].shape == (4, 4, 16) and last.autodecoder_opt_state["count"] == 2 * 2 and last.params["nef"] is st.params["nef"]
    assert not torch.equal(P["a"], val_ad.init(device="cpu")["params"]["a"])
