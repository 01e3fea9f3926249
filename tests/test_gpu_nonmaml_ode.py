"""Latent-ODE phase and validation roll-out of the auto-decoder trainer (nonmaml_pde_trainer.py:173-307) against the oracle:
table latents -> oracle solver (fp64 autograd through the oracle ODE model) -> oracle decoder at the same points -> mean
squared error.  Sizes and tolerances are those of the MAML trainer's equivalents (tests/test_gpu_ode_trainer.py): from the
latents on it is the same arithmetic."""
import os
import socket
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from oracle import enf_ref_np as R
from oracle import enf_ref_torch as T
from oracle import ode_ref_np as O
from oracle import ode_ref_torch as OT
from oracle import optim_ref_np as OP
from tests.helpers import make_cfg, build_nef
from tests.test_ode_oracle import ode_cfg
from tests.test_gpu_ode import _flat, _model, rel
from enf_pde_amd.fitting.trainers import NonMetaPDETrainer
from enf_pde_amd.enf.latents.autodecoder import PositionOrientationFeatureAutodecoder

pytestmark = pytest.mark.gpu

IDX = [4, 1]


def make_problem(n_s=32, method="euler", frames=22):
    """Everything but the device: oracle trees, a jittered 6-signal latent table, an 8 x 8 grid and 2 trajectories."""
    cfg = make_cfg("rel_pos_periodic", D=64, H=2, C=8, O=1)
    prm = R.init_params(0, cfg, jitter=0.1)
    ocfg = ode_cfg("rel_pos_periodic", num_hidden=16, basis_dim=16, num_layers=2)
    oprm = O.init_ponita_ode(1, ocfg, latent_dim=8, jitter=0.1, readout_scale=0.02)
    rng = np.random.default_rng(2)
    lin = np.linspace(-1, 1, 8)
    coords = np.stack(np.meshgrid(lin, lin), -1).reshape(-1, 2)
    traj = 10.0 * rng.standard_normal((2, frames, 8, 8, 1))              # (large targets: a gradient norm above 1, so the clip acts)
    table = {"p_pos": R.init_positions_grid(6, 9, 2) + 0.05 * rng.standard_normal((6, 9, 2)),
             "a": 1 + 0.2 * rng.standard_normal((6, 9, 8)), "gaussian_window": np.full((6, 9, 1), 2.0 / 3)}
    conf = NS(optimizer=NS(learning_rate_enf=1e-3, learning_rate_codes=1e-2, learning_rate_ode=1e-1),
              nef=NS(optimize_gaussian_window=False), training=NS(max_num_sampled_points=n_s), node=NS(dt=1, method=method))
    return NS(cfg=cfg, prm=prm, ocfg=ocfg, oprm=oprm, coords=coords, traj=traj, table=table, conf=conf, method=method)


def make_trainer(cuda, precision="f32", **kw):
    pb = make_problem(**kw)
    t = lambda v: torch.tensor(v, dtype=torch.float32, device=cuda)
    nef = build_nef(pb.cfg, precision)
    ode = _model(pb.ocfg, 8)
    ad = PositionOrientationFeatureAutodecoder(6, 9, 8, 2, 0, gaussian_window_size=-1)
    tr = NonMetaPDETrainer(pb.conf, nef, ad, t(pb.coords), seed=0, ode_model=ode)
    state = tr.init_train_state(nef.load_params(pb.prm, device=cuda), ode_params=ode.load_params(pb.oprm, device=cuda))
    state.params["autodecoder"]["params"] = {k: t(v) for k, v in pb.table.items()}
    return pb, tr, state, t


def point_masks(frames=10, n_s=32, seed=5):
    rng = np.random.default_rng(seed)
    return np.stack([rng.permutation(64)[:n_s] for _ in range(frames)])


def oracle_rollout(pb, oprm_t, idx, frames):
    z0 = tuple(torch.tensor(pb.table[k][idx]) for k in ("p_pos", "a", "gaussian_window"))
    sol = OT.solve_latent_ode(lambda z, _: OT.ponita_ode(oprm_t, pb.ocfg, z), z0, 0, frames - 1, 1, pb.method)
    return tuple(v.reshape(len(idx) * frames, *v.shape[2:]) for v in sol)


def oracle_ode_loss(pb, oprm_t, idx, traj, pm):
    """nonmaml_pde_trainer.py:244-307 in fp64: 10 frames; ``pm`` (10, n_s) or None for the full grid."""
    B, F = len(idx), 10
    p_fl, a_fl, w_fl = oracle_rollout(pb, oprm_t, idx, F)
    tj = torch.tensor(traj[:, :F]).reshape(B, F, 64, 1)
    if pm is None:
        xs, ys = torch.tensor(pb.coords)[None].expand(B * F, -1, -1), tj.reshape(B * F, 64, 1)
    else:
        xs = torch.tensor(pb.coords)[torch.tensor(pm)][None].expand(B, -1, -1, -1).reshape(B * F, pm.shape[1], 2)
        ys = torch.stack([torch.stack([tj[b, k, pm[k]] for k in range(F)]) for b in range(B)]).reshape(B * F, pm.shape[1], 1)
    out = T.nef_apply(T.to_torch(pb.prm, torch.float64), pb.cfg, xs, p_fl, a_fl, w_fl)
    return ((out - ys) ** 2).mean(), out


def oracle_step(pb, idx, traj, pm, lr=1e-3):
    """(loss, {name: gradient}, {name: parameter after clip_by_global_norm(1) + adamw(lr) from a zero state}, the AdamW state
    after that step: mu = 0.1 clip(g), nu = 0.001 clip(g)^2 in the order of ``_flat``)."""
    rp = T.to_torch(pb.oprm, torch.float64, requires_grad=True)
    loss, _ = oracle_ode_loss(pb, rp, idx, traj, pm)
    loss.backward()
    leaves = dict(_flat(rp))
    names = list(leaves)
    g = [leaves[k].grad.numpy() for k in names]
    new, opt = OP.adam_step([leaves[k].detach().numpy() for k in names], OP.clip_by_global_norm(g, 1.0), OP.init_state(g),
                            lr=lr, weight_decay=1e-4)
    return float(loss.detach()), dict(zip(names, g)), dict(zip(names, new)), opt


@pytest.mark.parametrize("method", ["euler", "rk4"])
def test_ode_train_step_loss_gradient_and_update_match_oracle(cuda, method):
    pb, tr, state, t = make_trainer(cuda, method=method)
    pm = point_masks()
    ref_loss, ref_g, ref_new, ref_opt = oracle_step(pb, IDX, pb.traj, pm)
    batch = (t(pb.traj), torch.tensor(IDX, device=cuda))
    # the gradient the step takes: ode_loss differentiated w.r.t. the ODE leaves
    leaves = {k: v.detach().clone().requires_grad_(True) for k, v in _flat(state.params["ode_params"])}
    from enf_pde_amd.fitting.trainers.latent_ode import _unflatten
    params = dict(state.params, ode_params=_unflatten(state.params["ode_params"], list(leaves.values())))
    l0 = tr.ode_loss(params, batch[0], batch[1], torch.tensor(pm, device=cuda))
    g = torch.autograd.grad(l0, list(leaves.values()))
    l0 = l0.detach()
    print("loss", float(l0), "oracle", ref_loss)
    assert abs(float(l0) - ref_loss) < 1e-4 * ref_loss
    assert set(leaves) == set(ref_g)
    assert sum(float((x ** 2).sum()) for x in ref_g.values()) ** 0.5 > 1.5          # clip_by_global_norm(1.0) is not a no-op here
    for (k, _), gi in zip(leaves.items(), g):
        e = rel(gi.cpu().double().numpy(), ref_g[k])
        print("grad", k, e)
        assert e < 5e-3, k
    # the step: same loss, only the ODE parameters move, by clip_by_global_norm(1) + AdamW(learning_rate_enf) (:68-69)
    w0 = [w.clone() for w in tr.nef.param_tensors(state.params["nef"])]
    tab0 = {k: v.clone() for k, v in state.params["autodecoder"]["params"].items()}
    loss, new = tr.ode_train_step(state, batch, point_masks=torch.tensor(pm, device=cuda))
    assert abs(float(loss) - float(l0)) < 1e-6 * max(1.0, float(l0))
    after = dict(_flat(new.params["ode_params"]))
    before = dict(_flat(state.params["ode_params"]))
    for k, r in ref_new.items():
        np.testing.assert_allclose(after[k].detach().cpu().numpy(), r, rtol=2e-4, atol=2e-6, err_msg=k)
        assert not torch.equal(after[k], before[k]) or float(before[k].abs().max()) == 0
    # The first AdamW step from zero moments is lr g / (|g| + eps) + lr wd p, the same for g and for any rescaled g, so the
    # parameters above would not show a missing clip.  The moments do: mu = 0.1 clip(g), nu = 0.001 clip(g)^2 with clip(g) =
    # g / |g|_global (the norm is above 1.5).  Bounds from the gradient's: every leaf is within 5e-3 of the oracle's in norm, so
    # is the global norm, hence clip(g) within 1e-2 and its square within 2e-2; without the clip mu would be off by the factor
    # |g|_global > 1.5.
    assert list(ref_new) == list(after) and len(new.ode_opt_state["mu"]) == len(ref_new)
    for part, bound in (("mu", 1e-2), ("nu", 2e-2)):
        for k, got, want in zip(ref_new, new.ode_opt_state[part], ref_opt[part]):
            e = rel(got.cpu().double().numpy(), want)
            print(part, k, e)
            assert e < bound, (part, k)
    assert new.params["nef"] is state.params["nef"] and new.params["autodecoder"] is state.params["autodecoder"]
    assert new.nef_opt_state is state.nef_opt_state and new.autodecoder_opt_state is state.autodecoder_opt_state
    for a, b in zip(tr.nef.param_tensors(new.params["nef"]), w0):
        assert torch.equal(a, b)
    for k, v in tab0.items():
        assert torch.equal(new.params["autodecoder"]["params"][k], v)
    assert new.ode_opt_state["count"] == 1 and new.step == state.step + 1
    assert not any(v.requires_grad for v in after.values())


def test_steps_in_a_row_decrease_the_loss(cuda):
    """Consecutive steps on a fixed batch and fixed masks: the loss after one update and after three is below the first.  (The
    targets are noise no roll-out can fit, so the gain is small -- the same steps taken by the oracle in fp64 give 95.881, 95.792,
    95.775, 95.751, a thousand times the fp32 rounding of the loss -- and the oracle's own sequence is not monotone further on.)"""
    pb, tr, state, t = make_trainer(cuda)
    batch = (t(pb.traj), torch.tensor(IDX, device=cuda))
    pm = torch.tensor(point_masks(), device=cuda)
    losses = []
    for _ in range(4):
        l, state = tr.ode_train_step(state, batch, point_masks=pm)
        losses.append(float(l))
    print(losses)
    assert state.ode_opt_state["count"] == 4 and state.step == 4
    assert losses[1] < losses[0] and losses[-1] < losses[0], losses


def test_without_point_masks_on_a_small_grid_the_loss_is_the_full_grid_loss(cuda):
    pb, tr, state, t = make_trainer(cuda, n_s=64)                          # max_num_sampled_points == the grid: no subsampling
    ref_loss, _, _, _ = oracle_step(pb, IDX, pb.traj, None)
    rng0 = state.rng.get_state().clone()
    loss, _ = tr.ode_train_step(state, (t(pb.traj), torch.tensor(IDX, device=cuda)))
    print("loss", float(loss), "oracle", ref_loss)
    assert abs(float(loss) - ref_loss) < 1e-4 * ref_loss
    assert torch.equal(state.rng.get_state(), rng0)                 # and no permutation was drawn


def test_random_point_masks_come_from_the_state_generator(cuda):
    pb, tr, state, t = make_trainer(cuda)
    from enf_pde_amd.fitting.trainers import draw_point_masks
    gen = torch.Generator()
    gen.set_state(state.rng.get_state())
    pm = draw_point_masks(64, 32, 10, gen)
    ref_loss, _, _, _ = oracle_step(pb, IDX, pb.traj, pm.numpy())
    loss, _ = tr.ode_train_step(state, (t(pb.traj), torch.tensor(IDX, device=cuda)))
    assert abs(float(loss) - ref_loss) < 1e-4 * ref_loss
    assert torch.equal(state.rng.get_state(), gen.get_state())


def test_val_step_matches_oracle(cuda):
    """20 frames on the full grid, decoded in chunks of 24 of the 64 points (three chunks)."""
    pb, tr, state, t = make_trainer(cuda, n_s=24)
    idx = torch.tensor(IDX, device=cuda)
    mse_in, mse_out = tr.val_step(state, (t(pb.traj), idx))
    p_fl, a_fl, w_fl = oracle_rollout(pb, T.to_torch(pb.oprm, torch.float64), IDX, 20)
    rec = T.nef_apply(T.to_torch(pb.prm, torch.float64), pb.cfg, torch.tensor(pb.coords)[None].expand(40, -1, -1), p_fl, a_fl, w_fl)
    err = (rec.reshape(2, 20, 8, 8, 1).numpy() - pb.traj[:, :20]) ** 2
    print("val", float(mse_in), err[:, :10].mean(), float(mse_out), err[:, 10:].mean())
    assert abs(float(mse_in) - err[:, :10].mean()) < 1e-4 * err[:, :10].mean()
    assert abs(float(mse_out) - err[:, 10:].mean()) < 1e-4 * err[:, 10:].mean()
    assert "_ode_graph" in tr.__dict__                              # the roll-out replayed a captured derivative evaluation
    # 12 frames: the second error over frames 10, 11; 10 frames: zero.  (The first ten frames of a roll-out do not depend on its length.)
    a, b = tr.val_step(state, (t(pb.traj[:, :12]), idx))
    assert abs(float(a) - err[:, :10].mean()) < 1e-4 * err[:, :10].mean() and abs(float(b) - err[:, 10:12].mean()) < 1e-4 * err[:, 10:12].mean()
    a, b = tr.val_step(state, (t(pb.traj[:, :10]), idx))
    assert abs(float(a) - err[:, :10].mean()) < 1e-4 * err[:, :10].mean() and float(b) == 0.0
    # a validation table read through its own shell (:209-210: the shell given, the table of the state)
    val_ad = PositionOrientationFeatureAutodecoder(2, 9, 8, 2, 0, gaussian_window_size=-1)
    P = state.params["autodecoder"]["params"]
    vstate = type(state)(params=dict(state.params, autodecoder={"params": {k: v[IDX].clone() for k, v in P.items()}}),
                         nef_opt_state=state.nef_opt_state, autodecoder_opt_state=None, ode_opt_state=state.ode_opt_state)
    c, d = tr.val_step(vstate, (t(pb.traj), torch.tensor([0, 1], device=cuda)), autodecoder=val_ad)
    assert abs(float(c) - float(mse_in)) < 1e-6 * float(mse_in) and abs(float(d) - float(mse_out)) < 1e-6 * float(mse_out)


def test_bf16_decoder_gives_a_finite_loss_near_the_f32_loss(cuda):
    """bf16-mode kernels change the decoder only (the latent ODE runs in fp32 either way), and the project bounds a bf16-mode field
    by 3e-2 of the largest reference value (tests/test_gpu_forward.py: TOL).  With out = ref + e, |e| <= d = 3e-2 max|ref|, and
    targets y, the loss mean((ref + e - y)^2) differs from mean((ref - y)^2) by 2 mean(e ref) - 2 mean(e y) + mean(e^2).
      * |mean(e ref)| <= d max|ref| and mean(e^2) <= d^2;
      * the targets are 10 N(0, 1) noise drawn independently of everything the decoder reads, so given e, mean(e y) over the
        n = 2 x 10 x 32 sampled values is normal with standard deviation <= 10 d / sqrt(n); six of them are allowed.
    Here max|ref| = 0.347 and the loss is 95.9, so the bound is 0.057.  (Cauchy-Schwarz, 2 d sqrt(loss) + d^2 = 0.204, is the case of an
    error aligned with the residual.)  Measured difference: OBSERVED."""
    from tests.test_gpu_forward import TOL
    pm = point_masks()
    losses = {}
    for prec in ("f32", "bf16"):
        pb, tr, state, t = make_trainer(cuda, precision=prec)
        loss, new = tr.ode_train_step(state, (t(pb.traj), torch.tensor(IDX, device=cuda)), point_masks=torch.tensor(pm, device=cuda))
        assert np.isfinite(float(loss)) and all(bool(torch.isfinite(v).all()) for _, v in _flat(new.params["ode_params"]))
        losses[prec] = float(loss)
    _, out = oracle_ode_loss(pb, T.to_torch(pb.oprm, torch.float64), IDX, pb.traj, pm)
    top = float(out.abs().max())
    d = TOL["bf16"] * top
    bound = 2 * d * top + 2 * 6 * 10.0 * d / out.numel() ** 0.5 + d * d
    print(losses, "difference", abs(losses["bf16"] - losses["f32"]), "bound", bound, "max|ref|", top)
    assert out.numel() == 2 * 10 * 32
    assert abs(losses["bf16"] - losses["f32"]) <= bound, (losses, bound)


# ------------------------------------------------------------------------------------------------ two ranks on one GPU
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _worker(rank, world, port, q):
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK="0", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import torch.distributed as dist
    from enf_pde_amd.fitting import init_distributed, shard_range
    from tests.test_gpu_nonmaml_ode import make_trainer, point_masks, IDX
    from tests.test_gpu_ode import _flat
    init_distributed(backend="gloo")
    cuda = torch.device("cuda:0")
    pb, tr, state, t = make_trainer(cuda)
    lo, hi = shard_range(2, rank, world)                          # 2 trajectories: one per rank
    batch = (t(pb.traj)[lo:hi], torch.tensor(IDX[lo:hi], device=cuda))
    loss, new = tr.ode_train_step(state, batch, point_masks=torch.tensor(point_masks(), device=cuda))
    o = torch.cat([v.reshape(-1) for _, v in _flat(new.params["ode_params"])]).cpu()
    q.put((rank, float(loss), o.numpy()))                         # plain arrays: no shared-memory handles to outlive us
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_take_the_single_process_step(cuda):
    world, port = 2, _free_port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    try:
        res = sorted((q.get(timeout=300) for _ in range(world)), key=lambda r: r[0])
        for p in procs:
            p.join(timeout=120)
            assert p.exitcode == 0
    finally:
        for p in procs:
            if p.is_alive():
                p.kill()
    (_, la, oa), (_, lb, ob) = res
    assert la == lb and np.array_equal(oa, ob)                    # the all-reduced loss, identical parameters on both ranks
    pb, tr, state, t = make_trainer(cuda)
    loss, new = tr.ode_train_step(state, (t(pb.traj), torch.tensor(IDX, device=cuda)), point_masks=torch.tensor(point_masks(), device=cuda))
    o = torch.cat([v.reshape(-1) for _, v in _flat(new.params["ode_params"])]).cpu().numpy()
    o0 = torch.cat([v.reshape(-1) for _, v in _flat(state.params["ode_params"])]).cpu().numpy()
    assert abs(float(loss) - la) < 1e-4 * abs(la)
    assert np.abs(o - o0).max() > 5e-4                            # the step moved the parameters (by ~lr = 1e-3 per entry)
    # the first Adam step is lr * sign-ish(g): entries whose gradient is within rounding noise of zero may move the other way;
    # the rest agree (the criterion of tests/test_gpu_dist.py)
    assert (np.abs(o - oa) < 2e-4).mean() > 0.97
