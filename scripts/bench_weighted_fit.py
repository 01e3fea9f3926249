"""Cost of the per-point loss weights (include/enf_hip.h, "Weighted loss"): the one-call inner step at the bench's fit shape
(BASELINE config 2: 16 signals, 64 latents, 512 sampled points, D = 128, H = 2, bf16) without a weight (enf_fit_step_w with
weight == NULL: what bench.py and every unweighted caller run) and with one, in ONE process, interleaved rounds, hipEvent
pairs on the launch stream, median of --iters single calls after --warmup (the protocol of scripts/bench_determinism.py).
Prints one JSON line.

  python scripts/bench_weighted_fit.py [--iters 100] [--warmup 10] [--rounds 3]
"""
import argparse
import json
import os
import sys
from types import SimpleNamespace as NS

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from enf_pde_amd.enf.models import EquivariantCrossAttentionNeF  # noqa: E402
from enf_pde_amd.enf.steerable_attention.invariant import get_ca_invariant  # noqa: E402
from bench_determinism import median_ms  # noqa: E402

D, H, C, O = 128, 2, 16, 1
B, Z, N = 16, 64, 512


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    inv = get_ca_invariant(NS(invariant_type="rel_pos_periodic", num_in=2))
    g = torch.Generator().manual_seed(0)
    x = (torch.rand(B, N, 2, generator=g) * 2 - 1).to(dev)
    p = (torch.rand(B, Z, 2, generator=g) * 2 - 1).to(dev)
    a = (1 + 0.1 * torch.randn(B, Z, C, generator=g)).to(dev)
    s = torch.full((B, Z, 1), 0.25, device=dev)
    target = torch.randn(B, N, O, generator=g).to(dev)
    weight = (torch.rand(B, N, generator=g) * 2).to(dev)
    weight[weight < 0.5] = 0
    nef = EquivariantCrossAttentionNeF(num_hidden=D, num_heads=H, num_layers=0, num_out=O, latent_dim=C, cross_attn_invariant=inv,
                                       precision="bf16")
    params = nef.init(1, device=dev)
    loss = torch.zeros(1, device=dev)

    def step(w):
        def fn():
            with torch.no_grad():
                nef.mse_value_and_latent_grads(params, x, p, a, s, target, grad_scale=B, loss_out=loss, weight=w)
        return fn
    legs = {"unweighted": step(None), "weighted": step(weight)}
    out = {k: [] for k in legs}
    for _ in range(args.rounds):                     # interleaved: both legs see the same box state
        for k, fn in legs.items():
            out[k].append(round(median_ms(fn, args.iters, args.warmup), 4))
    res = {"D": D, "H": H, "precision": "bf16", "B,Z,N": [B, Z, N], "iters": args.iters, "rounds": args.rounds,
           "clock": "hipEvent pair around each call, median per round", "fit_step_ms": out,
           "weighted_over_unweighted": round(min(out["weighted"]) / min(out["unweighted"]), 4)}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
