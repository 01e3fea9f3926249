"""Cost of the deterministic mode (include/enf_hip.h, "Deterministic mode"): the one-call inner step (enf_fit_step_ex) and the
training backward (forward + enf_backward_all through apply / backward with the weights requiring gradients) on the default
(atomic) and on the deterministic path, in ONE process, interleaved rounds, hipEvent pairs on the launch stream, median of
--iters single calls after --warmup.  Shapes: BASELINE config 2 (16 signals, 64 latents, 512 sampled points, D = 128, H = 2,
bf16: the z-fold backward with nsplit = 1) and a small batch where the backward pair kernel splits the queries (1 signal,
5 latents, 4096 queries: nsplit = 256).  Prints one JSON line.

  python scripts/bench_determinism.py [--iters 100] [--warmup 10] [--rounds 3]
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
from enf_pde_amd.fitting.trainers.pde_trainer import _tree_from_tensors  # noqa: E402

D, H, C, O = 128, 2, 16, 1
SHAPES = {"config2_fit": (16, 64, 512), "small_batch": (1, 5, 4096)}       # B, Z, N


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
    return ts[iters // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    inv = get_ca_invariant(NS(invariant_type="rel_pos_periodic", num_in=2))
    res = {"D": D, "H": H, "precision": "bf16", "clock": "hipEvent pair around each call, median; best of the rounds",
           "iters": args.iters, "rounds": args.rounds}
    for name, (B, Z, N) in SHAPES.items():
        g = torch.Generator().manual_seed(0)
        x = (torch.rand(B, N, 2, generator=g) * 2 - 1).to(dev)
        p = (torch.rand(B, Z, 2, generator=g) * 2 - 1).to(dev)
        a = (1 + 0.1 * torch.randn(B, Z, C, generator=g)).to(dev)
        s = torch.full((B, Z, 1), 0.25, device=dev)
        target = torch.randn(B, N, O, generator=g).to(dev)
        w = torch.randn(B, N, O, generator=g).to(dev)
        legs = {}
        for mode in ("default", "deterministic"):
            nef = EquivariantCrossAttentionNeF(num_hidden=D, num_heads=H, num_layers=0, num_out=O, latent_dim=C, cross_attn_invariant=inv,
                                               precision="bf16", deterministic=mode == "deterministic")
            params = nef.init(1, device=dev)
            loss = torch.zeros(1, device=dev)
            ws = [t.detach().clone().requires_grad_(t.numel() > 0) for t in nef.param_tensors(params)]
            tree = _tree_from_tensors(ws)

            def fit(nef=nef, params=params, loss=loss):
                with torch.no_grad():
                    nef.mse_value_and_latent_grads(params, x, p, a, s, target, grad_scale=B, loss_out=loss)

            def train(nef=nef, tree=tree, ws=ws):
                out = nef.apply(tree, x, p, a, s)
                torch.autograd.grad((out * w).sum(), [t for t in ws if t.requires_grad], allow_unused=True)
            legs[mode] = {"fit_step_ms": fit, "train_fwd_bwd_all_ms": train}
        out = {m: {k: [] for k in legs[m]} for m in legs}
        for _ in range(args.rounds):                     # interleaved: both paths see the same box state
            for leg in ("fit_step_ms", "train_fwd_bwd_all_ms"):
                for mode in legs:
                    out[mode][leg].append(median_ms(legs[mode][leg], args.iters, args.warmup))
        best = {m: {k: round(min(v), 4) for k, v in out[m].items()} for m in out}
        best["deterministic_over_default"] = {k: round(best["deterministic"][k] / best["default"][k], 4) for k in best["default"]}
        best["B,Z,N"] = [B, Z, N]
        res[name] = best
    print(json.dumps(res))


if __name__ == "__main__":
    main()
