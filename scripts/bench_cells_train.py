"""Cost of the three pieces that carry cell averages into the trainers (include/enf_hip.h, "Grouped observations"), at the bench's fit
shape with G = 4: 16 signals, 64 latents, 128 sampled cells = 512 query rows per step, D = 128, H = 2, O = 1, bf16; the cells are 32 x 32
on [-1, 1]^2 with 2 x 2 Gauss points, S = 3 inner steps (four sampled sets).

  gather     the setup of inner_loop_cells: ONE enf_fit_inputs_g launch (latent broadcast, the four sampled sets of points, factors,
             targets and weights, zeroed losses) against the same in torch ops (gather_cell_samples, the broadcast, the zero fill)
  step0      the first inner step on shared latents: nef.mse_value_and_cell_grads(shared_latents=True) (enf_fit_step_gs with
             ENF_FIT_SHARED_LATENTS: one forward and, here, one backward for all signals) against the unflagged call (enf_fit_step_g)
  cell_mse   the unfused grouped loss and its d out on a decode in memory: nef.cell_mse forward + backward (ONE
             enf_mse_value_grad_g launch and a scale) against cell_mse_torch forward + backward (torch ops with autograd)

hipEvent pairs on the launch stream, median of --iters single calls after --warmup, --rounds interleaved rounds (every leg in every
round).  Prints one JSON line; with --out FILE also writes it there.

  python scripts/bench_cells_train.py [--iters 100] [--warmup 10] [--rounds 3] [--out profiles/cells_train.json]
"""
import argparse
import json
import os
import sys
from types import SimpleNamespace as NS

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

D, H, C, O = 128, 2, 16, 1
B, Z, MS, G, S = 16, 64, 128, 4, 3
SIDE = 32


def median_ms(fn, iters, warmup):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2 * iters)]
    for i in range(iters):
        ev[2 * i].record()
        fn()
        ev[2 * i + 1].record()
    torch.cuda.synchronize()
    ts = sorted(ev[2 * i].elapsed_time(ev[2 * i + 1]) for i in range(iters))
    return ts[iters // 2]


def legs():
    import torch
    from enf_pde_amd.enf.models import EquivariantCrossAttentionNeF
    from enf_pde_amd.enf.steerable_attention.invariant import get_ca_invariant
    from enf_pde_amd.fitting import cell_mse_torch, cell_quadrature, gather_cell_samples
    from enf_pde_amd.fitting import cells as CELLS
    dev = torch.device("cuda:0")
    inv = get_ca_invariant(NS(invariant_type="rel_pos_periodic", num_in=2))
    g = torch.Generator().manual_seed(0)
    x, q = (t.to(dev) for t in cell_quadrature((-1.0, 1.0, (SIDE, SIDE)), 2))
    M, N = SIDE * SIDE, MS * G
    obs = torch.randn(B, M, O, generator=g).to(dev)
    w = (torch.rand(B, M, generator=g) * 2).to(dev)
    w[w < 0.5] = 0
    masks = torch.stack([torch.randperm(M, generator=g)[:MS] for _ in range(S + 1)], 1).to(dev).contiguous()
    lat0 = {"p_pos": (torch.rand(1, Z, 2, generator=g) * 2 - 1).to(dev), "a": (1 + 0.1 * torch.randn(1, Z, C, generator=g)).to(dev),
            "gaussian_window": torch.full((1, Z, 1), 0.25, device=dev)}
    nef = EquivariantCrossAttentionNeF(num_hidden=D, num_heads=H, num_layers=0, num_out=O, latent_dim=C, cross_attn_invariant=inv,
                                       precision="bf16")
    params = nef.init(1, device=dev)

    def gather_launch():
        CELLS._cell_inputs(lat0, x, q, G, obs, masks, w)

    def gather_torch():
        lat = {k: v.detach().repeat_interleave(B, dim=0) for k, v in lat0.items()}
        losses = torch.zeros(S + 1, device=dev)
        return lat, losses, gather_cell_samples(x, q, G, obs, masks, w)
    assert CELLS._cell_inputs(lat0, x, q, G, obs, masks, w) is not None
    lat, xs_all, qs_all, ys_all, _, ws_all = CELLS._cell_inputs(lat0, x, q, G, obs, masks, w)
    xb, qb = xs_all[0][None].expand(B, -1, -1), qs_all[0][None].expand(B, -1).contiguous()
    loss = torch.zeros(1, device=dev)
    step = lambda shared: nef.mse_value_and_cell_grads(params, xb, lat["p_pos"], lat["a"], lat["gaussian_window"], ys_all[0], G, qweight=qb,
                                                       obs_weight=ws_all[0], grad_scale=B, loss_out=loss, shared_latents=shared)
    with torch.no_grad():
        out = nef.apply(params, xb, lat["p_pos"], lat["a"], lat["gaussian_window"]).float().contiguous()

    def mse_kernel():
        o = out.detach().requires_grad_(True)
        nef.cell_mse(o, ys_all[0], G, qb, ws_all[0]).backward()

    def mse_torch():
        o = out.detach().requires_grad_(True)
        cell_mse_torch(o, ys_all[0], G, qb, ws_all[0]).backward()
    import ctypes
    from enf_pde_amd import _lib
    applies = int(_lib.load().enf_shared_backward_applies(ctypes.byref(nef._desc(B, N, Z)), _lib.ENF_FIT_SHARED_LATENTS))
    return {"gather_launch": gather_launch, "gather_torch": gather_torch, "step0_flagged": lambda: step(True), "step0_unflagged": lambda: step(False),
            "cell_mse_kernel": mse_kernel, "cell_mse_torch": mse_torch}, applies


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    own, applies = legs()
    ms = {k: [] for k in own}
    for _ in range(args.rounds):
        for k, fn in own.items():
            ms[k].append(round(median_ms(fn, args.iters, args.warmup), 4))
    med = lambda v: sorted(v)[len(v) // 2]
    res = {"D": D, "H": H, "precision": "bf16", "B,Z,Ms,G": [B, Z, MS, G], "rows_per_step": MS * G, "sampled_sets": S + 1, "iters": args.iters,
           "rounds": args.rounds, "clock": "hipEvent pair around each call, median per round", "ms": ms,
           "shared_backward_applies": applies,
           "gather_launch_over_torch": round(med(ms["gather_launch"]) / med(ms["gather_torch"]), 4),
           "step0_flagged_over_unflagged": round(med(ms["step0_flagged"]) / med(ms["step0_unflagged"]), 4),
           "cell_mse_kernel_over_torch": round(med(ms["cell_mse_kernel"]) / med(ms["cell_mse_torch"]), 4)}
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
