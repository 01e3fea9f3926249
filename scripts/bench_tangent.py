"""Cost and accuracy of a tendency field (include/enf_hip.h, "Tendency fields") against the only route there was before it, a central
difference of two decodes.

Time: bench config 2's DECODE shape (16 signals, 64 latents, the 64 x 64 grid shared by the signals, D = 128, H = 2, O = 1), ONE
process, interleaved rounds, hipEvent pairs on the launch stream, median of single calls after a warm-up; every round is recorded.
  tangent    nef.tangent (enf_field_tangent), bf16 and f32
  decode     nef.apply under no_grad in the same precision
  cdiff      (apply(z + h v) - apply(z - h v)) / (2 h) with two f32 decodes
Accuracy: the test shape of tests/tangent_ref.py (rel_pos_periodic, D = 64, H = 2, B = 3, N = 50, Z = 7) against the fp64 oracle: the
relative Frobenius error of nef.tangent and of the central difference for a range of steps h, in f32 and in bf16.

Prints one JSON line; --out FILE also writes it there (profiles/tangent.json).

  python scripts/bench_tangent.py [--iters 30] [--warmup 3] [--rounds 3] [--out profiles/tangent.json]
"""
import argparse
import json
import os
import sys
from types import SimpleNamespace as NS

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from enf_pde_amd.enf.models import EquivariantCrossAttentionNeF  # noqa: E402
from enf_pde_amd.enf.steerable_attention.invariant import get_ca_invariant  # noqa: E402
from scripts.bench_determinism import median_ms  # noqa: E402

D, H, C, O = 128, 2, 16, 1
B, Z, GRID = 16, 64, 64
STEPS = (1e-1, 3e-2, 1e-2, 3e-3, 1e-3, 1e-4)


def routes(dev):
    inv = get_ca_invariant(NS(invariant_type="rel_pos_periodic", num_in=2))
    g = torch.Generator().manual_seed(0)
    lin = torch.linspace(-1, 1, GRID)
    coords = torch.stack(torch.meshgrid(lin, lin, indexing="xy"), -1).reshape(-1, 2).to(dev)     # (4096, 2), one grid for the batch
    p = (torch.rand(B, Z, 2, generator=g) * 2 - 1).to(dev)
    a = (1 + 0.1 * torch.randn(B, Z, C, generator=g)).to(dev)
    s = torch.full((B, Z, 1), 0.25, device=dev)
    dp, da = (0.3 * torch.randn(B, Z, 2, generator=g)).to(dev), torch.randn(B, Z, C, generator=g).to(dev)
    ds = (0.02 * torch.randn(B, Z, 1, generator=g)).to(dev)
    grid = coords[None].expand(B, -1, -1)
    fns = {}
    for prec in ("bf16", "f32"):
        nef = EquivariantCrossAttentionNeF(num_hidden=D, num_heads=H, num_layers=0, num_out=O, latent_dim=C, cross_attn_invariant=inv,
                                           precision=prec, deterministic=False)
        params = nef.init(1, device=dev)

        def tangent(nef=nef, params=params):
            nef.tangent(params, grid, p, a, s, dp=dp, da=da, dwindow=ds)

        def decode(nef=nef, params=params):
            with torch.no_grad():
                nef.apply(params, grid, p, a, s)
        fns[f"tangent_{prec}"], fns[f"decode_{prec}"] = tangent, decode
        if prec == "f32":
            def cdiff(nef=nef, params=params, h=1e-2):
                with torch.no_grad():
                    hi = nef.apply(params, grid, p + h * dp, a + h * da, s + h * ds)
                    lo = nef.apply(params, grid, p - h * dp, a - h * da, s - h * ds)
                    return (hi - lo) / (2 * h)
            fns["cdiff_f32"] = cdiff
    return fns


def accuracy(dev):
    from tests.helpers import build_nef
    from tests.tangent_ref import case, rel
    cfg, prm, (x, p, a, s), (dp, da, ds), _, tan_ref = case("rel_pos_periodic")
    t = lambda v: torch.tensor(v, dtype=torch.float32, device=dev)
    res = {"shape": "rel_pos_periodic, D = 64, H = 2, C = 8, O = 2, B = 3, N = 50, Z = 7 (tests/tangent_ref.py)", "steps_h": list(STEPS)}
    for prec in ("f32", "bf16"):
        nef = build_nef(cfg, prec)
        P = nef.load_params(prm, device=dev)
        _, tan = nef.tangent(P, t(x), t(p), t(a), t(s), dp=t(dp), da=t(da), dwindow=t(ds))
        errs = []
        with torch.no_grad():
            for h in STEPS:
                hi = nef.apply(P, t(x), t(p + h * dp), t(a + h * da), t(s + h * ds))
                lo = nef.apply(P, t(x), t(p - h * dp), t(a - h * da), t(s - h * ds))
                errs.append(rel(((hi - lo) / (2 * h)).double().cpu().numpy(), tan_ref))
        res[prec] = {"tangent_rel_err": float(f"{rel(tan.double().cpu().numpy(), tan_ref):.3e}"),
                     "cdiff_rel_err_by_h": [float(f"{e:.3e}") for e in errs], "cdiff_best_rel_err": float(f"{min(errs):.3e}"),
                     "cdiff_best_h": STEPS[int(np.argmin(errs))]}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    res = {"shape": {"B": B, "Z": Z, "N": GRID * GRID, "D": D, "H": H, "O": O, "grid": "shared by the signals (x_bstride = 0)"},
           "clock": "hipEvent pair around each call, median of the calls; medians of all rounds listed, the best reported",
           "iters": args.iters, "rounds": args.rounds}
    fns = routes(dev)
    times = {k: [] for k in fns}
    for _ in range(args.rounds):                     # interleaved: the routes see the same box state
        for k, fn in fns.items():
            times[k].append(median_ms(fn, args.iters, args.warmup))
    best = {k: min(v) for k, v in times.items()}
    res["ms"] = {k: round(v, 4) for k, v in best.items()}
    res["rounds_ms"] = {k: [round(t, 4) for t in v] for k, v in times.items()}
    res["ratios"] = {"tangent_over_decode_bf16": round(best["tangent_bf16"] / best["decode_bf16"], 3),
                     "tangent_over_decode_f32": round(best["tangent_f32"] / best["decode_f32"], 3),
                     "cdiff_f32_over_tangent_bf16": round(best["cdiff_f32"] / best["tangent_bf16"], 3),
                     "cdiff_f32_over_tangent_f32": round(best["cdiff_f32"] / best["tangent_f32"], 3)}
    res["accuracy"] = accuracy(dev)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
