"""The latent-only step of the auto-decoder trainer, old and new (fitting/trainers/nonmaml_pde_trainer.py):

  autodec_only   nef_train_step_autodec_only: the training step with the weight update switched off (autograd graph, `out`
                 materialised, enf_backward_all with its 46 unused weight gradients, dense index backward, foreach Adam)
  fit_latents    fit_latents_step: enf_fit_step_w + enf_table_adam_update, no autograd

at the shape validate_epoch runs for config_navier_stokes_nonmaml.yaml: batch 8, 64 latents, a 64 x 64 grid, 2048 sampled points,
num_hidden 128, 2 heads, latent_dim 16, bf16, a table of --signals rows (512: num_signals_test).  ONE process, interleaved rounds;
per leg the median of --iters hipEvent pairs around single steps after --warmup (the protocol of scripts/bench_determinism.py),
and the wall time per step of the same number of steps issued back to back with one synchronisation at the end (what a fit loop
of validate_epoch pays, host side included).  Every step starts from the same state.  Prints one JSON line.

  python scripts/bench_autodec_fit.py [--iters 100] [--warmup 10] [--rounds 3] [--signals 512]
"""
import argparse
import json
import os
import sys
import time
from types import SimpleNamespace as NS

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from enf_pde_amd.enf.models import EquivariantCrossAttentionNeF  # noqa: E402
from enf_pde_amd.enf.steerable_attention.invariant import get_ca_invariant  # noqa: E402
from enf_pde_amd.enf.latents.autodecoder import PositionOrientationFeatureAutodecoder  # noqa: E402
from enf_pde_amd.fitting.trainers import NonMetaPDETrainer  # noqa: E402
from bench_determinism import median_ms  # noqa: E402

D, H, C, O = 128, 2, 16, 1
B, Z, SIDE, N_S = 8, 64, 64, 2048


def wall_ms(fn, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--signals", type=int, default=512)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    inv = get_ca_invariant(NS(invariant_type="rel_pos_periodic", num_in=2))
    nef = EquivariantCrossAttentionNeF(num_hidden=D, num_heads=H, num_layers=0, num_out=O, latent_dim=C, cross_attn_invariant=inv,
                                       precision="bf16")
    conf = NS(optimizer=NS(learning_rate_enf=1e-4, learning_rate_codes=1e-3), training=NS(max_num_sampled_points=N_S))
    ad = PositionOrientationFeatureAutodecoder(args.signals, Z, C, 2, 0, gaussian_window_size=-1)
    lin = torch.linspace(-1, 1, SIDE)
    coords = torch.stack(torch.meshgrid(lin, lin, indexing="xy"), -1).reshape(-1, 2).to(dev)
    tr = NonMetaPDETrainer(conf, nef, ad, coords, seed=0)
    state = tr.init_train_state(nef.init(1, device=dev))
    g = torch.Generator().manual_seed(0)
    batch = (torch.randn(B, SIDE, SIDE, O, generator=g).to(dev), torch.randperm(args.signals, generator=g)[:B].to(dev))
    legs = {"autodec_only": lambda: tr.nef_train_step_autodec_only(state, batch), "fit_latents": lambda: tr.fit_latents_step(state, batch)}
    event, wall = {k: [] for k in legs}, {k: [] for k in legs}
    for _ in range(args.rounds):                     # interleaved: both legs see the same box state
        for k, fn in legs.items():
            event[k].append(round(median_ms(fn, args.iters, args.warmup), 4))
            wall[k].append(round(wall_ms(fn, args.iters), 4))
    res = {"D": D, "H": H, "precision": "bf16", "B,Z,grid,N_s": [B, Z, SIDE * SIDE, N_S], "table_rows": args.signals, "iters": args.iters,
           "rounds": args.rounds, "clock": "hipEvent pair around each step, median per round; wall: back-to-back steps, one sync",
           "step_ms_event": event, "step_ms_wall": wall,
           "old_over_new_event": round(min(event["autodec_only"]) / min(event["fit_latents"]), 3),
           "old_over_new_wall": round(min(wall["autodec_only"]) / min(wall["fit_latents"]), 3)}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
