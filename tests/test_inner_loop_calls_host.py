"""What fitting/inner_loop.py: inner_loop asks of a decoder, without a GPU: for every form of the fit -- shared or per-signal masks, no,
point or channel weights, with or without per-signal losses -- the keywords of each step, the points, targets and weights step s is
handed, the form of the last loss, and the one draw of the pose jitter.  One loop serves all forms; these are the properties that
have to hold in each of them."""
import importlib
from types import SimpleNamespace as NS

import pytest
import torch

IL = importlib.import_module("enf_pde_amd.fitting.inner_loop")
B, N, O, NS_, S, Z = 3, 30, 2, 11, 3, 4
PAD = 4                     # signal 1 of the per-signal masks has only N_s - PAD observed points: -1 in its last rows
_UNSET = object()


class _Stop(Exception):
    pass


class _Rec:
    """A decoder that records what it is handed; no device.  ``shared_latents`` is named, so the loop may pass the hint."""
    cross_attn_invariant = NS(num_z_ori_dims=0)

    def __init__(self):
        self.steps, self.evals, self.applies = [], [], []

    def mse_value_and_latent_grads(self, params, x, p, a, window, target, shared_latents=_UNSET, **kw):
        if shared_latents is not _UNSET:
            kw["shared_latents"] = shared_latents
        self.steps.append(NS(x=x, p=p.clone(), a=a, window=window, target=target, kw=kw))
        res = (kw["loss_out"], torch.zeros_like(p), torch.zeros_like(a), torch.zeros_like(window))
        k = float(len(self.steps))
        return res + (torch.zeros(target.shape[:2]), torch.full((target.shape[0],), k)) if kw.get("return_errors") else res

    def eval_loss(self, params, x, p, a, window, target, **kw):
        self.evals.append(NS(x=x, p=p.clone(), target=target, kw=kw))
        return torch.full((target.shape[0],), -1.0), torch.zeros(target.shape[:2])

    def apply(self, params, x, p, a, window):
        self.applies.append(NS(x=x, p=p.clone()))
        raise _Stop()         # (the launch of the loss kernel that follows needs a device)


def _problem(per_signal, form):
    g = torch.Generator().manual_seed(11)
    img, coords = torch.randn((B, N, O), generator=g), torch.randn((N, 2), generator=g)
    lat0 = {"p_pos": torch.randn((1, Z, 2), generator=g), "a": torch.randn((1, Z, 4), generator=g), "gaussian_window": torch.ones(1, Z, 1)}
    cols = lambda: torch.stack([torch.randperm(N, generator=g)[:NS_] for _ in range(S + 1)], 1)
    if per_signal:
        masks = torch.stack([cols() for _ in range(B)])
        masks[1, NS_ - PAD:, :] = -1
    else:
        masks = cols()
    full = {"none": None, "point": torch.rand((B, N), generator=g) + 0.1, "channel": torch.rand((B, N, O), generator=g) + 0.1}[form]
    # the sampled inputs of step s, element by element (an index outside the grid: the first coordinate, zero target, zero weight)
    idx = masks if per_signal else masks[None].expand(B, -1, -1)
    xs, ys = torch.zeros(S + 1, B, NS_, 2), torch.zeros(S + 1, B, NS_, O)
    ws = torch.zeros((S + 1, B, NS_, O) if form == "channel" else (S + 1, B, NS_))
    for s in range(S + 1):
        for b in range(B):
            for i in range(NS_):
                n = int(idx[b, i, s])
                xs[s, b, i] = coords[n if n >= 0 else 0]
                if n >= 0:
                    ys[s, b, i] = img[b, n]
                    ws[s, b, i] = 1.0 if full is None else full[b, n]
    if form == "none" and not per_signal:
        ws = None
    kw = {"none": {}, "point": {"weights": full}, "channel": {"channel_weights": full}}[form]
    return NS(img=img, coords=coords, lat0=lat0, masks=masks, kw=kw, xs=xs, ys=ys, ws=ws)


def _run(monkeypatch, pr, **kw):
    updates = []

    def update(lat, grads, lrs, scale):
        updates.append((sorted(grads), scale))
        return {k: v + 1.0 for k, v in lat.items()}           # (every step then sees other latents than the one before)
    monkeypatch.setattr(IL, "meta_sgd_update", update)
    nef, res = _Rec(), None
    try:
        res = IL.inner_loop(nef, None, pr.lat0, None, pr.coords, pr.img, pr.masks, **pr.kw, **kw)
    except _Stop:
        pass
    return nef, res, updates


@pytest.mark.parametrize("per_signal_loss", [False, True])
@pytest.mark.parametrize("form", ["none", "point", "channel"])
@pytest.mark.parametrize("per_signal", [False, True])
def test_what_the_loop_asks_of_a_decoder(monkeypatch, per_signal, form, per_signal_loss):
    pr = _problem(per_signal, form)
    nef, res, updates = _run(monkeypatch, pr, per_signal_loss=per_signal_loss)
    weight_kw = "channel_weight" if form == "channel" else "weight"
    assert len(nef.steps) == S and updates == [(["a", "p_pos"], B)] * S
    poses = [pr.lat0["p_pos"].expand(B, -1, -1)]              # the stand-in update adds one to every latent
    for _ in range(S):
        poses.append(poses[-1] + 1.0)
    for s, c in enumerate(nef.steps):
        want = {"loss_out", weight_kw} | ({"return_errors"} if per_signal_loss else set()) | ({"shared_latents"} if s == 0 and not per_signal else set())
        assert set(c.kw) == want, s
        assert c.kw.get("return_errors", True) is True and c.kw.get("shared_latents", True) is True
        assert c.x.shape == (B, NS_, 2) and c.x.stride(0) == (NS_ * 2 if per_signal else 0), s       # every signal's own points, or one set
        assert torch.equal(c.x, pr.xs[s]) and torch.equal(c.target, pr.ys[s]), s
        assert c.target.is_contiguous() and c.target.dtype == torch.float32
        if pr.ws is None:
            assert c.kw[weight_kw] is None
        else:
            assert torch.equal(c.kw[weight_kw], pr.ws[s]) and c.kw[weight_kw].is_contiguous(), s
        lo = c.kw["loss_out"]                                  # step s's own zeroed accumulator of one (S + 1,) buffer
        assert lo.shape == (1,) and float(lo) == 0.0 and lo.data_ptr() == nef.steps[0].kw["loss_out"].data_ptr() + 4 * s
        assert torch.equal(c.p, poses[s]) and c.p.shape == (B, Z, 2)  # the latents of the update before
    if per_signal_loss:
        assert not nef.applies and len(nef.evals) == 1
        e = nef.evals[0]
        assert set(e.kw) == {"loss_out", weight_kw}
        assert torch.equal(e.x, pr.xs[S]) and torch.equal(e.target, pr.ys[S]) and torch.equal(e.p, poses[S])
        assert e.kw[weight_kw] is None if pr.ws is None else torch.equal(e.kw[weight_kw], pr.ws[S])
        assert e.kw["loss_out"].shape == (1,) and e.kw["loss_out"].data_ptr() == nef.steps[0].kw["loss_out"].data_ptr() + 4 * S
        loss, lat, loss_b = res
        assert loss.dim() == 0 and loss.data_ptr() == e.kw["loss_out"].data_ptr()
        assert torch.equal(loss_b, torch.tensor([[1.0] * B, [2.0] * B, [3.0] * B, [-1.0] * B]))     # every step's row, then the last mask's
        assert torch.equal(lat["p_pos"], e.p)
    else:
        assert res is None and not nef.evals and len(nef.applies) == 1                            # a decode on the points of mask column S
        c = nef.applies[0]
        assert torch.equal(c.x, pr.xs[S]) and c.x.stride(0) == (NS_ * 2 if per_signal else 0)
        assert torch.equal(c.p, poses[S])


@pytest.mark.parametrize("per_signal_loss", [False, True])
@pytest.mark.parametrize("form", ["none", "point", "channel"])
def test_the_pose_jitter_is_one_draw(monkeypatch, form, per_signal_loss):
    pr = _problem(False, form)
    g, twin = torch.Generator().manual_seed(5), torch.Generator().manual_seed(5)
    nef, _, _ = _run(monkeypatch, pr, per_signal_loss=per_signal_loss, noise_pos=0.25, generator=g)
    noise = torch.randn((B, Z, 2), generator=twin)
    assert torch.equal(g.get_state(), twin.get_state())                                          # one draw of (B, Z, 2), nothing else
    p0 = nef.steps[0].p
    assert torch.equal(p0, pr.lat0["p_pos"] + noise * 0.25)
    assert not torch.equal(p0[0], p0[1]) and not torch.equal(p0[1], p0[2])
    assert all("shared_latents" not in c.kw for c in nef.steps)                                  # the signals no longer share their latents


# ---------------------------------------------------------------------------------------------- the same loop on cell averages
CELLS = importlib.import_module("enf_pde_amd.fitting.cells")
M, G, MS = 10, 4, 5
PAD_G = 2                   # signal 1 of the per-signal masks has only MS - PAD_G observed cells: -1 in its last rows


class _RecCells:
    """The grouped calls of a decoder, recorded; no device.  ``shared_latents`` is named, so the loop may pass the hint."""
    cross_attn_invariant = NS(num_z_ori_dims=0)

    def __init__(self):
        self.steps, self.evals = [], []

    def mse_value_and_cell_grads(self, params, x, p, a, window, target, group, shared_latents=_UNSET, **kw):
        if shared_latents is not _UNSET:
            kw["shared_latents"] = shared_latents
        self.steps.append(NS(x=x, p=p.clone(), target=target, group=group, kw=kw))
        res = (kw["loss_out"], torch.zeros_like(p), torch.zeros_like(a), torch.zeros_like(window))
        k = float(len(self.steps))
        return res + (torch.zeros(target.shape[:2]), torch.full((target.shape[0],), k)) if kw.get("return_errors") else res

    def eval_cell_loss(self, params, x, p, a, window, target, group, **kw):
        self.evals.append(NS(x=x, p=p.clone(), target=target, group=group, kw=kw))
        return (torch.full((target.shape[0],), -1.0) if kw["per_signal"] else None), torch.zeros(target.shape[:2])

    def apply(self, *a):
        raise AssertionError("the loop on cells decodes nothing")


def _cell_problem(per_signal, form):
    g = torch.Generator().manual_seed(13)
    obs, x, q = torch.randn((B, M, O), generator=g), torch.randn((M * G, 2), generator=g), torch.rand((M * G,), generator=g)
    lat0 = {"p_pos": torch.randn((1, Z, 2), generator=g), "a": torch.randn((1, Z, 4), generator=g), "gaussian_window": torch.ones(1, Z, 1)}
    cols = lambda: torch.stack([torch.randperm(M, generator=g)[:MS] for _ in range(S + 1)], 1)
    if per_signal:
        masks = torch.stack([cols() for _ in range(B)])
        masks[1, MS - PAD_G:, :] = -1
    else:
        masks = cols()
    full = {"none": None, "obs": torch.rand((B, M), generator=g) + 0.1, "value": torch.rand((B, M, O), generator=g) + 0.1}[form]
    # the sampled inputs of step s, element by element (an index outside: cell 0's rows, zero target, zero weight)
    idx = masks if per_signal else masks[None].expand(B, -1, -1)
    xs, qs, ys = torch.zeros(S + 1, B, MS * G, 2), torch.zeros(S + 1, B, MS * G), torch.zeros(S + 1, B, MS, O)
    ws = torch.zeros((S + 1, B, MS, O) if form == "value" else (S + 1, B, MS))
    for s in range(S + 1):
        for b in range(B):
            for i in range(MS):
                m = int(idx[b, i, s])
                for k in range(G):
                    xs[s, b, i * G + k], qs[s, b, i * G + k] = x[max(m, 0) * G + k], q[max(m, 0) * G + k]
                if m >= 0:
                    ys[s, b, i] = obs[b, m]
                    ws[s, b, i] = 1.0 if full is None else full[b, m]
    if form == "none" and not per_signal:
        ws = None
    kw = {"none": {}, "obs": {"obs_weights": full}, "value": {"obs_channel_weight": full}}[form]
    return NS(obs=obs, x=x, q=q, lat0=lat0, masks=masks, kw=kw, xs=xs, qs=qs, ys=ys, ws=ws)


def _run_cells(monkeypatch, pr, **kw):
    updates = []

    def update(lat, grads, lrs, scale):
        updates.append((sorted(grads), scale))
        return {k: v + 1.0 for k, v in lat.items()}
    monkeypatch.setattr(IL, "meta_sgd_update", update)            # (the loop on cells is inner_loop's: it looks the update up there)
    nef = _RecCells()
    return nef, CELLS.inner_loop_cells(nef, None, pr.lat0, None, pr.x, pr.q, G, pr.obs, pr.masks, **pr.kw, **kw), updates


@pytest.mark.parametrize("per_signal_loss", [False, True])
@pytest.mark.parametrize("form", ["none", "obs", "value"])
@pytest.mark.parametrize("per_signal", [False, True])
def test_what_the_loop_on_cells_asks_of_a_decoder(monkeypatch, per_signal, form, per_signal_loss):
    pr = _cell_problem(per_signal, form)
    nef, res, updates = _run_cells(monkeypatch, pr, per_signal_loss=per_signal_loss)
    weight_kw = "obs_channel_weight" if form == "value" else "obs_weight"
    assert len(nef.steps) == S and updates == [(["a", "p_pos"], B)] * S
    poses = [pr.lat0["p_pos"].expand(B, -1, -1)]
    for _ in range(S):
        poses.append(poses[-1] + 1.0)
    rows = MS * G
    for s, c in enumerate(nef.steps):
        hint = s == 0 and not per_signal and form != "value"           # per-value weights run every step unshared
        want = {"qweight", "loss_out", weight_kw} | ({"return_errors"} if per_signal_loss else set()) | ({"shared_latents"} if hint else set())
        assert set(c.kw) == want and c.group == G, s
        assert c.kw.get("return_errors", True) is True and c.kw.get("shared_latents", True) is True
        assert c.x.shape == (B, rows, 2) and c.x.stride(0) == (rows * 2 if per_signal else 0), s      # rows m G + k of every sampled cell m
        qw = c.kw["qweight"]
        assert qw.shape == (B, rows) and qw.stride(0) == (rows if per_signal else 0), s
        assert torch.equal(c.x, pr.xs[s]) and torch.equal(qw, pr.qs[s]) and torch.equal(c.target, pr.ys[s]), s
        assert c.target.is_contiguous() and c.target.dtype == torch.float32
        if pr.ws is None:
            assert c.kw[weight_kw] is None
        else:
            assert torch.equal(c.kw[weight_kw], pr.ws[s]) and c.kw[weight_kw].is_contiguous(), s
        lo = c.kw["loss_out"]                                  # step s's own zeroed accumulator of one (S + 1,) buffer
        assert lo.shape == (1,) and float(lo) == 0.0 and lo.data_ptr() == nef.steps[0].kw["loss_out"].data_ptr() + 4 * s
        assert torch.equal(c.p, poses[s]) and c.p.shape == (B, Z, 2)
    assert len(nef.evals) == 1                                  # the final loss always comes from eval_cell_loss: nothing is decoded
    e = nef.evals[0]
    assert set(e.kw) == {"qweight", "loss_out", "per_signal", weight_kw} and e.kw["per_signal"] is per_signal_loss and e.group == G
    assert torch.equal(e.x, pr.xs[S]) and torch.equal(e.kw["qweight"], pr.qs[S]) and torch.equal(e.target, pr.ys[S]) and torch.equal(e.p, poses[S])
    assert e.x.stride(0) == (rows * 2 if per_signal else 0)
    assert e.kw[weight_kw] is None if pr.ws is None else torch.equal(e.kw[weight_kw], pr.ws[S])
    assert e.kw["loss_out"].shape == (1,) and e.kw["loss_out"].data_ptr() == nef.steps[0].kw["loss_out"].data_ptr() + 4 * S
    loss, lat = res[:2]
    assert loss.dim() == 0 and loss.data_ptr() == e.kw["loss_out"].data_ptr() and torch.equal(lat["p_pos"], e.p)
    if per_signal_loss:
        assert torch.equal(res[2], torch.tensor([[1.0] * B, [2.0] * B, [3.0] * B, [-1.0] * B]))      # every step's row, then the last mask's
    else:
        assert len(res) == 2


@pytest.mark.parametrize("form", ["none", "obs", "value"])
def test_the_pose_jitter_on_cells_is_one_draw(monkeypatch, form):
    pr = _cell_problem(False, form)
    g, twin = torch.Generator().manual_seed(5), torch.Generator().manual_seed(5)
    nef, _, _ = _run_cells(monkeypatch, pr, noise_pos=0.25, generator=g)
    noise = torch.randn((B, Z, 2), generator=twin)
    assert torch.equal(g.get_state(), twin.get_state())                                          # one draw of (B, Z, 2), nothing else
    assert torch.equal(nef.steps[0].p, pr.lat0["p_pos"] + noise * 0.25)
    assert all("shared_latents" not in c.kw for c in nef.steps)
