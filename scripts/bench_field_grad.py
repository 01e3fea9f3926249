"""Cost of a derivative field (include/enf_hip.h, "Derivative fields") at bench config 2's DECODE shape (16 signals, 64 latents, the
64 x 64 grid shared by the signals, D = 128, H = 2, bf16) with O = 1 and with O = 2, in ONE process, interleaved rounds, hipEvent pairs
on the launch stream, median of single calls after a warm-up; the best of the rounds is reported.  Three routes per shape:

  jacobian   nef.jacobian (enf_field_grad: one forward, O seeded tail backwards + backward pair kernels)
  existing   nef.apply with x.requires_grad (the training path: activation-store K3 + K4, all weight gradients formed and dropped),
             one forward and one autograd backward per output channel
  decode     nef.apply under no_grad (the plain decode, for scale)

Prints one JSON line; --out FILE also writes it there (profiles/field_grad.json).

  python scripts/bench_field_grad.py [--iters 30] [--warmup 3] [--rounds 3] [--out profiles/field_grad.json]
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
from scripts.bench_determinism import median_ms  # noqa: E402

D, H, C = 128, 2, 16
B, Z, GRID = 16, 64, 64


def routes(O, dev):
    inv = get_ca_invariant(NS(invariant_type="rel_pos_periodic", num_in=2))
    nef = EquivariantCrossAttentionNeF(num_hidden=D, num_heads=H, num_layers=0, num_out=O, latent_dim=C, cross_attn_invariant=inv,
                                       precision="bf16", deterministic=False)
    params = nef.init(1, device=dev)
    g = torch.Generator().manual_seed(0)
    lin = torch.linspace(-1, 1, GRID)
    coords = torch.stack(torch.meshgrid(lin, lin, indexing="xy"), -1).reshape(-1, 2).to(dev)     # (4096, 2), one grid for the batch
    p = (torch.rand(B, Z, 2, generator=g) * 2 - 1).to(dev)
    a = (1 + 0.1 * torch.randn(B, Z, C, generator=g)).to(dev)
    s = torch.full((B, Z, 1), 0.25, device=dev)
    grid = coords[None].expand(B, -1, -1)

    def jacobian():
        nef.jacobian(params, grid, p, a, s)

    def existing():
        leaf = coords.detach().requires_grad_(True)
        out = nef.apply(params, leaf[None].expand(B, -1, -1), p, a, s)
        for o in range(O):
            torch.autograd.grad(out[..., o].sum(), leaf, retain_graph=o + 1 < O)

    def decode():
        with torch.no_grad():
            nef.apply(params, grid, p, a, s)
    return {"jacobian": jacobian, "existing": existing, "decode": decode}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    res = {"shape": {"B": B, "Z": Z, "N": GRID * GRID, "D": D, "H": H, "precision": "bf16", "grid": "shared by the signals (x_bstride = 0)"},
           "clock": "hipEvent pair around each call, median; best of the rounds", "iters": args.iters, "rounds": args.rounds}
    for O in (1, 2):
        fns = routes(O, dev)
        times = {k: [] for k in fns}
        for _ in range(args.rounds):                 # interleaved: the routes see the same box state
            for k, fn in fns.items():
                times[k].append(median_ms(fn, args.iters, args.warmup))
        best = {k: min(v) for k, v in times.items()}
        res[f"O{O}"] = {"jacobian_ms": round(best["jacobian"], 4), "existing_ms": round(best["existing"], 4), "decode_ms": round(best["decode"], 4),
                        "existing_over_jacobian": round(best["existing"] / best["jacobian"], 3),
                        "jacobian_over_decode": round(best["jacobian"] / best["decode"], 3),
                        "rounds_ms": {k: [round(t, 4) for t in v] for k, v in times.items()}}
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
