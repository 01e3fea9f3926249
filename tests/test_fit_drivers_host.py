"""What the fits beside inner_loop ask of a decoder, without a GPU: the call sequences of fit_cell_averages and fit_linear_observations
(the step body of fitting/inner_loop.py on inputs of their own choosing, never with the shared-latent hint), the operator front end of
the Levenberg-Marquardt loop on a linear stand-in, and the one switch between the fused gathers and their torch-op mirrors."""
import importlib
from types import SimpleNamespace as NS

import pytest
import torch

from enf_pde_amd.fitting import SparseObservations, draw_cell_samples, fit_cell_averages, fit_linear_observations
from tests.test_gn_host import _LinearNef, _cg_update_torch
from tests.test_inner_loop_calls_host import _RecCells, _cell_problem, _UNSET

IL = importlib.import_module("enf_pde_amd.fitting.inner_loop")
CELLS = importlib.import_module("enf_pde_amd.fitting.cells")
B, M, G, O, Z, S = 3, 6, 4, 2, 4, 3
MS = 4                      # observations per step of a sampled fit


class _RecFit(_RecCells):
    """_RecCells whose steps also hand back a window gradient's worth of zeros, plus the operator's two calls."""

    def mse_value_and_operator_grads(self, params, x, p, a, window, target, op, shared_latents=_UNSET, **kw):
        return self.mse_value_and_cell_grads(params, x, p, a, window, target, op, shared_latents=shared_latents, **kw)

    def eval_operator_loss(self, params, x, p, a, window, target, op, **kw):
        return self.eval_cell_loss(params, x, p, a, window, target, op, **kw)


def _updates(monkeypatch):
    updates = []

    def update(lat, grads, lrs, scale):
        updates.append((sorted(grads), scale))
        return {k: v + 1.0 for k, v in lat.items()}           # (every step then sees other latents than the one before)
    monkeypatch.setattr(IL, "meta_sgd_update", update)
    return updates


def _latents(g):
    return {"p_pos": torch.randn((1, Z, 2), generator=g), "a": torch.randn((1, Z, 4), generator=g), "gaussian_window": torch.ones(1, Z, 1)}


def _weights(form, g, num):
    full = {"none": None, "obs": torch.rand((B, num), generator=g) + 0.1, "value": torch.rand((B, num, O), generator=g) + 0.1}[form]
    return full, {"none": {}, "obs": {"obs_weight": full}, "value": {"obs_channel_weight": full}}[form]


def _check_fit(nef, res, updates, lat0, weight_kw, per_signal_loss, window, extra, inputs):
    """What both stand-alone fits share: S steps with today's keywords and never the hint, the update at scale B, one evaluation on the
    last set into the last slot, and the shape of the returns.  ``inputs(s)`` -> (x (N_s, dx), target, weights or None) of step s."""
    keys = ["a", "gaussian_window", "p_pos"] if window else ["a", "p_pos"]
    assert len(nef.steps) == S and updates == [(keys, B)] * S
    poses = [lat0["p_pos"].expand(B, -1, -1)]
    for _ in range(S):
        poses.append(poses[-1] + 1.0)
    base = nef.steps[0].kw["loss_out"].data_ptr()
    for s, c in enumerate(nef.steps + nef.evals):
        x, ys, ws = inputs(s)
        last = s == S
        assert set(c.kw) == {"loss_out", weight_kw, "per_signal" if last else "return_errors"} | extra, s
        assert "shared_latents" not in c.kw
        assert c.kw["per_signal" if last else "return_errors"] is per_signal_loss
        assert c.x.shape == (B, *x.shape) and c.x.stride(0) == 0 and torch.equal(c.x[0], x), s          # one set, a stride-0 batch
        assert torch.equal(c.target, ys) and c.target.dtype == torch.float32, s
        assert c.kw[weight_kw] is None if ws is None else torch.equal(c.kw[weight_kw], ws), s
        lo = c.kw["loss_out"]                                  # slot s of one zeroed (S + 1,) buffer
        assert lo.shape == (1,) and float(lo) == 0.0 and lo.data_ptr() == base + 4 * s
        assert torch.equal(c.p, poses[s]) and c.p.shape == (B, Z, 2)
    assert len(nef.evals) == 1
    loss, lat = res[:2]
    assert loss.dim() == 0 and loss.data_ptr() == base + 4 * S and torch.equal(lat["p_pos"], poses[S])
    assert set(lat) == set(lat0) and all(lat[k].shape == (B, *lat0[k].shape[1:]) for k in lat0)
    if per_signal_loss:
        assert len(res) == 3 and torch.equal(res[2], torch.tensor([[1.0] * B, [2.0] * B, [3.0] * B, [-1.0] * B]))
    else:
        assert len(res) == 2


@pytest.mark.parametrize("window", [False, True])
@pytest.mark.parametrize("with_q", [True, False])
@pytest.mark.parametrize("per_signal_loss", [False, True])
@pytest.mark.parametrize("form", ["none", "obs", "value"])
@pytest.mark.parametrize("sample", ["all", "int", "tensor"])
def test_what_fit_cell_averages_asks_of_a_decoder(monkeypatch, sample, form, per_signal_loss, with_q, window):
    g = torch.Generator().manual_seed(17)
    obs, x = torch.randn((B, M, O), generator=g), torch.randn((M * G, 2), generator=g)
    q = torch.rand((M * G,), generator=g) if with_q else None
    lat0 = _latents(g)
    full, wkw = _weights(form, g, M)
    if sample == "all":
        idx, skw = torch.arange(M)[None].expand(S + 1, -1), {}
    elif sample == "int":
        idx = draw_cell_samples(M, MS, S, torch.Generator().manual_seed(3))
        skw = {"sample": MS, "generator": torch.Generator().manual_seed(3)}
    else:
        idx = torch.stack([torch.randperm(M, generator=g)[:MS] for _ in range(S + 1)])
        skw = {"sample": idx}
    updates = _updates(monkeypatch)
    nef = _RecFit()
    res = fit_cell_averages(nef, None, lat0, None, x, q, G, obs, S, per_signal_loss=per_signal_loss, optimize_gaussian_window=window, **wkw, **skw)
    rows = (idx[..., None] * G + torch.arange(G)).reshape(S + 1, -1)        # rows m G + k of every cell m of a set, in order
    weight_kw = "obs_channel_weight" if form == "value" else "obs_weight"
    _check_fit(nef, res, updates, lat0, weight_kw, per_signal_loss, window, {"qweight"},
               lambda s: (x[rows[s]], obs[:, idx[s]], None if full is None else full[:, idx[s]]))
    for s, c in enumerate(nef.steps + nef.evals):
        qw = c.kw["qweight"]
        assert c.group == G
        if q is None:
            assert qw is None
        else:
            assert qw.shape == (B, rows.shape[1]) and qw.stride(0) == 0 and torch.equal(qw[0], q[rows[s]]), s


@pytest.mark.parametrize("window", [False, True])
@pytest.mark.parametrize("per_signal_loss", [False, True])
@pytest.mark.parametrize("form", ["none", "obs", "value"])
def test_what_fit_linear_observations_asks_of_a_decoder(monkeypatch, form, per_signal_loss, window):
    g = torch.Generator().manual_seed(19)
    op = SparseObservations.from_groups([3, 0, 5], None)                  # ragged rows, one of them empty
    y, x = torch.randn((B, op.M, O), generator=g), torch.randn((op.N, 2), generator=g)
    lat0 = _latents(g)
    full, wkw = _weights(form, g, op.M)
    updates = _updates(monkeypatch)
    nef = _RecFit()
    res = fit_linear_observations(nef, None, lat0, None, x, op, y, S, per_signal_loss=per_signal_loss, optimize_gaussian_window=window, **wkw)
    weight_kw = "obs_channel_weight" if form == "value" else "obs_weight"
    _check_fit(nef, res, updates, lat0, weight_kw, per_signal_loss, window, set(), lambda s: (x, y, full))
    assert all(c.group is op for c in nef.steps + nef.evals)              # (the operator stands where the group size does)


# ---------------------------------------------------------------------------------------------- the operator front end of the LM loop
class _LinearOpNef(_LinearNef):
    """_LinearNef of tests/test_gn_host.py observed through a sparse operator: obs[b] = A out[b] with the dense A (M, N) of the
    operator it is handed, so J = A J_out and G = 2 / (M O) (A J_out)^T W (A J_out) exactly.  Records every call."""
    N = 8

    def gn_reserve(self, B, N, Z, dev, op=None):
        self.log.append(("reserve", B, N, Z, op))

    def _obs(self, out, op):
        return torch.einsum("mn,bno->bmo", torch.tensor(op.to_dense(dtype="float32")), out)

    def _jt(self, res, op):
        """J_out^T A^T res"""
        rows = torch.einsum("mn,bmo->bno", torch.tensor(op.to_dense(dtype="float32")), res)
        return torch.einsum("bij,bi->bj", self.A, rows.reshape(self.B, -1))

    def mse_value_and_operator_grads(self, params, x, p, a, window, target, op, obs_weight=None, obs_channel_weight=None, grad_scale=1.0,
                                     return_errors=False):
        assert return_errors and window is None and obs_channel_weight is None and tuple(x.shape) == (self.B, self.N, 2)
        w = torch.ones(self.B, op.M) if obs_weight is None else obs_weight
        res = self._obs(self.out(p, a), op) - target
        err = w * (res ** 2).sum(2)
        g = grad_scale / self.B * 2.0 / (op.M * self.O) * self._jt(w[..., None] * res, op)
        self._touch()
        self.log.append(("op_fit", grad_scale, x.stride(0), op))
        lb = err.sum(1) / (op.M * self.O)
        return (lb.mean().reshape(1), *self._split(g), None, err, lb)

    def gn_operator_product(self, params, x, p, a, window, op, obs_weight=None, obs_channel_weight=None, vp=None, va=None, vwindow=None,
                            grad_scale=1.0, reuse=None):
        self.log.append(("op_gn", vp is None, va is None, vwindow is None, reuse == self.workspace_tag(None), x.stride(0)))
        v = self._z(torch.zeros(self.B, self.Z, self.WP) if vp is None else vp, torch.zeros(self.B, self.Z, self.WA) if va is None else va)
        tan = torch.einsum("bij,bj->bi", self.A, v).reshape(self.B, self.N, self.O)
        w = torch.ones(self.B, op.M) if obs_weight is None else obs_weight
        g = grad_scale / self.B * 2.0 / (op.M * self.O) * self._jt(w[..., None] * self._obs(tan, op), op)
        self._touch()
        return (*self._split(g), None)

    def eval_operator_loss(self, params, x, p, a, window, target, op, obs_weight=None, obs_channel_weight=None):
        self._touch()
        self.log.append(("op_eval", x.stride(0)))
        w = torch.ones(self.B, op.M) if obs_weight is None else obs_weight
        err = w * ((self._obs(self.out(p, a), op) - target) ** 2).sum(2)
        return err.sum(1) / (op.M * self.O), err


def test_lm_operator_front_end_issues_its_call_sequence(monkeypatch):
    """The third leg of tests/test_gn_cells_host.py: test_lm_front_ends_issue_their_call_sequences."""
    from enf_pde_amd.fitting import gauss_newton as GN
    monkeypatch.setattr(GN, "_cg_update", _cg_update_torch)
    nef = _LinearOpNef(B)
    op = SparseObservations.from_groups([3, 0, 5], None)
    g = torch.Generator().manual_seed(5)
    p0, a0 = torch.randn((B, nef.Z, nef.WP), generator=g), torch.randn((B, nef.Z, nef.WA), generator=g)
    ps, as_ = p0 + 0.3 * torch.randn(p0.shape, generator=g), a0 + 0.3 * torch.randn(a0.shape, generator=g)
    w = torch.rand((B, op.M), generator=g) + 0.2
    x = torch.zeros(nef.N, 2)                                   # (N, dx): shared query points, expanded with stride 0
    target = nef._obs(nef.out(ps, as_), op)
    # reserve for this operator, then per step one operator fit step at gradient scale B, cg_iters products that reuse its point, one
    # evaluation.  M O = 6 observations (two of them of the empty row) for 15 unknowns per signal: 8 CG iterations solve the damped system.
    (p1, a1, w1), loss_b, lam1, acc = GN.lm_fit_linear_observations(nef, None, x, op, target, p0, a0, None, steps=2, cg_iters=8, damping=1e-6,
                                                                   obs_weight=w)
    assert w1 is None and loss_b.shape == (3, B) and acc.shape == (2, B) and acc.dtype == torch.bool and lam1.shape == (B,)
    assert bool(acc[0].all()) and bool((loss_b[1] < 1e-3 * loss_b[0]).all()) and bool((loss_b[2] <= loss_b[1]).all())
    assert nef.log[0] == ("reserve", B, nef.N, nef.Z, op) and nef.log[0][4] is op
    step = [("op_fit", float(B), 0, op)] + [("op_gn", False, False, True, True, 0)] * 8 + [("op_eval", 0)]
    assert nef.log[1:] == step * 2
    # x (B, N, dx) arrives as given; one component: the unused one passes None and stays
    nef.log.clear()
    xb = x[None].repeat(B, 1, 1)
    (p2, a2, _), lb2, _, acc2 = GN.lm_fit_linear_observations(nef, None, xb, op, target, p0, a0, None, steps=1, cg_iters=4, components=("a",))
    assert torch.equal(p2, p0) and not torch.equal(a2, a0) and bool(acc2.all()) and bool((lb2[1] < lb2[0]).all())
    assert [e[0] for e in nef.log] == ["reserve", "op_fit"] + ["op_gn"] * 4 + ["op_eval"]
    assert nef.log[1] == ("op_fit", float(B), nef.N * 2, op) and nef.log[-1] == ("op_eval", nef.N * 2)
    assert all(e[1:] == (True, False, True, True, nef.N * 2) for e in nef.log if e[0] == "op_gn")
    # steps = 0: one evaluation and nothing else
    nef.log.clear()
    _, lb0, _, acc0 = GN.lm_fit_linear_observations(nef, None, x, op, target, p0, a0, None, steps=0)
    assert lb0.shape == (1, B) and acc0.shape == (0, B) and [e[0] for e in nef.log] == ["reserve", "op_eval"]


# ---------------------------------------------------------------------------------------------- one switch for both gathers
@pytest.mark.parametrize("fused", [False, True])
def test_the_cell_gather_honours_the_inner_loops_switch(monkeypatch, fused):
    """inner_loop.FUSED_FIT_INPUTS is the one switch between the fused gather launches and their torch-op mirrors: turned off there,
    inner_loop_cells does not even ask for the launch (off the GPU the launch declines and both routes end in gather_cell_samples)."""
    pr = _cell_problem(False, "obs")
    asked = []
    inputs = CELLS._cell_inputs
    monkeypatch.setattr(CELLS, "_cell_inputs", lambda *a, **k: asked.append(1) or inputs(*a, **k))
    monkeypatch.setattr(IL, "FUSED_FIT_INPUTS", fused)
    monkeypatch.setattr(IL, "meta_sgd_update", lambda lat, grads, lrs, scale: lat)
    nef = _RecCells()
    CELLS.inner_loop_cells(nef, None, pr.lat0, None, pr.x, pr.q, 4, pr.obs, pr.masks, **pr.kw)
    assert len(asked) == (1 if fused else 0)
    assert len(nef.steps) == 3 and all(torch.equal(c.x, pr.xs[s]) and torch.equal(c.target, pr.ys[s]) for s, c in enumerate(nef.steps))
