"""The yardstick of training on cell averages (include/enf_hip.h, "Grouped observations"), on the oracle in fp64: the MAML inner loop
of oracle/enf_ref_torch.py: inner_loop with every step's loss taken against GROUPED observations,

    obs[b,i,o] = sum_{k<G} q[m G + k] out[b, i G + k, o]         m = masks[i, s], the cell sampled as observation i of step s
    loss_s     = 1/(B Ms O) sum_{b,i} w[b,m] sum_o (obs - target[b,m])^2          (w == 0 is a select)

differentiable through the inner steps (create_graph), so that torch.autograd gives the exact meta-gradient w.r.t. the weights, the
latent initialisation and the inner rates.  tests/test_cells_train_host.py checks it against central differences of its own loss."""
import numpy as np
import torch

from oracle import enf_ref_torch as T
from enf_pde_amd.enf.models import TENSOR_PATHS


def _get(tree, path):
    for k in path:
        tree = tree[k]
    return tree


def cell_rows(masks_s, G):
    """query rows of the sampled cells, in order: row i G + k of the set is row m G + k of cell m"""
    return (masks_s[:, None] * G + torch.arange(G)).reshape(-1)


def inner_loop_cells(params, cfg, latents0, lrs, x, q, G, obs, masks, w=None, optimize_gaussian_window=False, create_graph=False):
    """x (M G, dx), q (M G,) or None (1 / G), obs (B, M, O), masks long (Ms, S + 1) cell indices, w (B, M) or None.
    Returns (loss at step S on masks[:, S], fitted latents)."""
    spec = T.invariant_spec(cfg["invariant"], cfg.get("num_in", 2))
    B, M, O = obs.shape
    S = masks.shape[1] - 1
    qf = torch.full((M * G,), 1.0 / G, dtype=x.dtype) if q is None else q
    lat = {k: v.repeat_interleave(B, dim=0) for k, v in latents0.items()}
    if not create_graph:
        lat = {k: v.detach().clone().requires_grad_(True) for k, v in lat.items()}

    def loss_fn(lat, s):
        m = masks[:, s]
        rows = cell_rows(m, G)
        out = T.nef_apply(params, cfg, x[rows][None].expand(B, -1, -1), T.split_pose(lat, spec), lat["a"], lat["gaussian_window"])
        o = (qf[rows][None, :, None] * out).reshape(B, m.shape[0], G, O).sum(2)
        ws = torch.ones((B, m.shape[0]), dtype=x.dtype) if w is None else w[:, m]
        live = (ws > 0)[..., None]
        dd = torch.where(live, o - torch.where(live, obs[:, m], torch.zeros_like(o)), torch.zeros_like(o))
        return (ws[..., None] * dd * dd).sum() / (B * m.shape[0] * O)

    for s in range(S):
        keys = list(lat.keys())
        g = torch.autograd.grad(loss_fn(lat, s), [lat[k] for k in keys], create_graph=create_graph, allow_unused=True)
        new = {}
        for k, gk in zip(keys, g):
            gk = torch.zeros_like(lat[k]) if gk is None else gk * B
            if k == "gaussian_window" and not optimize_gaussian_window:
                gk = torch.zeros_like(gk)
            new[k] = lat[k] - lrs[k] * gk
            if not create_graph:
                new[k] = new[k].detach().requires_grad_(True)
        lat = new
    return loss_fn(lat, S), lat


def meta_loss(prm, cfg, lat0, lrs, x, q, G, obs, masks, w=None):
    """the meta-objective as a float, from numpy inputs (for finite differences)"""
    tp = T.to_torch(prm, torch.float64)
    tt = lambda v: None if v is None else torch.tensor(np.asarray(v, dtype=np.float64))
    loss, _ = inner_loop_cells(tp, cfg, {k: tt(v) for k, v in lat0.items()}, {k: tt(v) for k, v in lrs.items()}, tt(x), tt(q), G, tt(obs),
                               torch.tensor(np.asarray(masks)), tt(w), create_graph=False)
    return float(loss.detach())


def meta_grads(prm, cfg, lat0, lrs, x, q, G, obs, masks, w=None):
    """(loss, [d / d weight tensor in TENSOR_PATHS order], {d / d lat0}, {d / d lrs}) by double backward in fp64"""
    tp = T.to_torch(prm, torch.float64, requires_grad=True)
    tt = lambda v: None if v is None else torch.tensor(np.asarray(v, dtype=np.float64))
    tl = {k: tt(v).requires_grad_(True) for k, v in lat0.items()}
    tr = {k: tt(v).requires_grad_(True) for k, v in lrs.items()}
    loss, _ = inner_loop_cells(tp, cfg, tl, tr, tt(x), tt(q), G, tt(obs), torch.tensor(np.asarray(masks)), tt(w), create_graph=True)
    leaves = [_get(tp["params"], p) for p in TENSOR_PATHS]
    g = torch.autograd.grad(loss, leaves + list(tl.values()) + list(tr.values()), allow_unused=True)
    z = lambda gi, t: np.zeros(tuple(t.shape)) if gi is None else gi.numpy()
    gw = [z(a, b) for a, b in zip(g[:len(leaves)], leaves)]
    gl = {k: z(a, tl[k]) for k, a in zip(tl, g[len(leaves):len(leaves) + len(tl)])}
    gr = {k: z(a, tr[k]) for k, a in zip(tr, g[len(leaves) + len(tl):])}
    return float(loss.detach()), gw, gl, gr


def cell_problem(problem, side=8, k=2, Ms=16, seed=11):
    """tests/test_gpu_trainer.py: _problem turned into side x side cells on [-1, 1]^2 with k Gauss points per axis: (cfg, prm, x (M G, 2),
    q (M G,), G, obs (B, M, 1), lat0, lrs, masks (Ms, S + 1))."""
    from enf_pde_amd.fitting import cell_quadrature
    cfg, prm, _, img, lat0, lrs, masks = problem
    x, q = cell_quadrature((-1.0, 1.0, (side, side)), k, dtype=torch.float64)
    M = side * side
    assert img.shape[1] == M
    rng = np.random.default_rng(seed)
    cm = np.stack([rng.permutation(M)[:Ms] for _ in range(masks.shape[1])], 1)
    f32 = lambda v: np.asarray(v, dtype=np.float32).astype(np.float64)
    return cfg, prm, f32(x.numpy()), f32(q.numpy()), k * k, f32(img), lat0, lrs, cm
