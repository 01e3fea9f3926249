"""Decode and one inner step (enf_fit_step) with the rff and the ffn invariant embedding at BASELINE config 2 (16 signals,
64^2 grid, 64 latents, rel_pos_periodic, D = 128, H = 2, bf16; the inner step on 512 sampled points), timed with hipEvent
pairs on the launch stream: median of --iters single calls after --warmup.  Prints one JSON line.

  python scripts/bench_ffn.py [--iters 100] [--warmup 10]
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

B, GRID, Z, NS_FIT, D, H, C, O = 16, 64, 64, 512, 128, 2, 16, 1


def median_ms(fn, iters, warmup):
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
    return round(ts[iters // 2], 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    lin = torch.linspace(-1, 1, GRID)
    coords = torch.stack(torch.meshgrid(lin, lin, indexing="xy"), -1).reshape(-1, 2).to(dev)
    x = coords[None].expand(B, -1, -1)
    xs = coords[torch.randperm(GRID * GRID, generator=g)[:NS_FIT].to(dev)][None].expand(B, -1, -1)
    p = (torch.rand(B, Z, 2, generator=g) * 2 - 1).to(dev)
    a = (1 + 0.1 * torch.randn(B, Z, C, generator=g)).to(dev)
    s = torch.full((B, Z, 1), 0.25, device=dev)
    target = torch.randn(B, NS_FIT, O, generator=g).to(dev)
    inv = get_ca_invariant(NS(invariant_type="rel_pos_periodic", num_in=2))
    res = {"config": 2, "B": B, "N_decode": GRID * GRID, "N_fit": NS_FIT, "Z": Z, "D": D, "H": H, "precision": "bf16",
           "clock": "hipEvent pair around each call, median", "iters": args.iters}
    for emb in ("rff", "ffn"):
        nef = EquivariantCrossAttentionNeF(num_hidden=D, num_heads=H, num_layers=0, num_out=O, latent_dim=C, cross_attn_invariant=inv,
                                           embedding_type=emb, precision="bf16")
        params = nef.init(1, device=dev)
        with torch.no_grad():
            dec = median_ms(lambda: nef.apply(params, x, p, a, s), args.iters, args.warmup)
            loss = torch.zeros(1, device=dev)
            fit = median_ms(lambda: nef.mse_value_and_latent_grads(params, xs, p, a, s, target, grad_scale=B, loss_out=loss),
                            args.iters, args.warmup)
        res[emb] = {"decode_ms": dec, "fit_step_ms": fit}
    res["ffn_over_rff"] = {k: round(res["ffn"][k] / res["rff"][k], 4) for k in ("decode_ms", "fit_step_ms")}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
