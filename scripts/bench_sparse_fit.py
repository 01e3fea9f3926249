"""What per-signal point masks buy on partially observed fields (include/enf_hip.h: enf_fit_inputs_b; fitting/inner_loop.py:
make_signal_masks).  BASELINE config 2's fit shape -- 16 signals, 64 latents, a 64 x 64 grid, 512 sampled points, 3 inner steps,
D = 128, H = 2, bf16 -- on fields of which every signal observes its own random fraction f of the grid, f in {1, 0.5, 0.25}:

  shared    one index set of N_s points for the whole batch plus ``weights`` (the zero-weight samples are computed and discarded)
  observed  per-signal masks of N_s * f points, all of them observed: the same expected number of informative samples per step,
            fitted with observed_sampling_weights (fitting/weights.py), so both arms' losses estimate the same full-grid weighted
            mean and their steps have the same length in expectation

For both arms: the inner loop (hipEvent pair around each call on the launch stream, median of --iters calls after --warmup, the
arms interleaved over --rounds rounds in ONE process), one inner step alone at the arm's point count, the gather kernel alone,
and the weighted MSE of the fitted latents' full-grid decode over all observed points (mean over --fits mask draws; the decoder
is randomly initialised, so the errors compare the arms and say nothing about a trained model).  Prints one JSON line.

  python scripts/bench_sparse_fit.py [--iters 50] [--warmup 5] [--rounds 3] [--fits 8]
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
from enf_pde_amd.fitting.inner_loop import (inner_loop, decode, make_masks, make_signal_masks, default_meta_sgd_lrs, _fit_inputs,  # noqa: E402
                                            _pose)
from enf_pde_amd.fitting.weights import normalize_point_weights, observed_sampling_weights, weighted_mse  # noqa: E402
from bench_determinism import median_ms  # noqa: E402

D, H, C, O = 128, 2, 16, 1
B, Z, SIDE, NS_FULL, S = 16, 64, 64, 512, 3
FRACTIONS = (1.0, 0.5, 0.25)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--fits", type=int, default=8)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    inv = get_ca_invariant(NS(invariant_type="rel_pos_periodic", num_in=2))
    nef = EquivariantCrossAttentionNeF(num_hidden=D, num_heads=H, num_layers=0, num_out=O, latent_dim=C, cross_attn_invariant=inv,
                                       precision="bf16")
    params = nef.init(1, device=dev)
    g = torch.Generator().manual_seed(0)
    lin = torch.linspace(-1, 1, SIDE)
    coords = torch.stack(torch.meshgrid(lin, lin, indexing="xy"), -1).reshape(-1, 2).to(dev)
    N = coords.shape[0]
    phase = torch.rand(B, 1, 2, generator=g).to(dev) * 6.283
    img = (torch.sin(3.1416 * coords[None, :, :1] + phase[..., :1]) * torch.cos(3.1416 * coords[None, :, 1:] + phase[..., 1:])).contiguous()
    k = round(Z ** 0.5)
    cell = (torch.arange(k, dtype=torch.float32) + 0.5) / k * 2 - 1
    lat0 = {"p_pos": torch.stack(torch.meshgrid(cell, cell, indexing="xy"), -1).reshape(1, Z, 2).to(dev),
            "a": torch.ones(1, Z, C, device=dev), "gaussian_window": torch.full((1, Z, 1), 2.0 / k, device=dev)}
    lrs = default_meta_sgd_lrs(C, lr_p=0.3, lr_a=2.0, device=dev)
    res = {"D": D, "H": H, "precision": "bf16", "B,Z,N,Ns,S": [B, Z, N, NS_FULL, S], "iters": args.iters, "rounds": args.rounds,
           "clock": "hipEvent pair around each call, median per round", "fractions": {}}
    for f in FRACTIONS:
        valid = (torch.rand(B, N, generator=g) < f) if f < 1 else torch.ones(B, N, dtype=torch.bool)
        w = normalize_point_weights(valid.float()).to(dev)                 # mean 1 on the full grid: 1 / f where observed
        field = torch.where(valid.to(dev)[..., None], img, torch.full_like(img, float("nan")))
        ns_b = max(1, int(NS_FULL * f))
        draw = {"shared": lambda gen: make_masks(N, NS_FULL, S, generator=gen, device=dev),
                "observed": lambda gen: make_signal_masks(valid, ns_b, S, generator=gen, device=dev)}
        masks = {k_: fn(torch.Generator().manual_seed(1)) for k_, fn in draw.items()}
        fit_w = {"shared": w, "observed": observed_sampling_weights(w, ns_b).contiguous()}         # matched normalisation

        def loop(m, w):
            return lambda: inner_loop(nef, params, lat0, lrs, coords, field, m, weights=w)

        def gather(m, w):
            return lambda: _fit_inputs(lat0, coords, field, m, w)

        def step(m, w):
            lat, xs, ys, losses, ws = _fit_inputs(lat0, coords, field, m, w)
            x = xs[0] if m.dim() == 3 else xs[0][None].expand(B, -1, -1)
            return lambda: nef.mse_value_and_latent_grads(params, x, _pose(lat, 0), lat["a"], lat["gaussian_window"], ys[0], grad_scale=B,
                                                          loss_out=losses[:1], weight=ws[0])
        legs = {(what, arm): fn(masks[arm], fit_w[arm]) for what, fn in (("inner_loop_ms", loop), ("fit_step_ms", step), ("gather_ms", gather))
                for arm in draw}
        out = {what: {arm: [] for arm in draw} for what in ("inner_loop_ms", "fit_step_ms", "gather_ms")}
        for _ in range(args.rounds):                  # interleaved: both arms see the same box state
            for (what, arm), fn in legs.items():
                out[what][arm].append(round(median_ms(fn, args.iters, args.warmup), 4))
        mse = {arm: [] for arm in draw}
        for seed in range(args.fits):
            for arm, fn in draw.items():
                _, fit = inner_loop(nef, params, lat0, lrs, coords, field, fn(torch.Generator().manual_seed(100 + seed)), weights=fit_w[arm])
                rec = decode(nef, params, coords, _pose(fit, 0), fit["a"], fit["gaussian_window"]).float()
                mse[arm].append(float(weighted_mse(rec, field, w)))
        out["points_per_signal"] = {"shared": NS_FULL, "observed": ns_b}
        out["valid_mse_after_fit"] = {arm: round(sum(v) / len(v), 6) for arm, v in mse.items()}
        out["valid_mse_at_init"] = round(float(weighted_mse(decode(nef, params, coords, lat0["p_pos"].repeat(B, 1, 1),
                                                                   lat0["a"].repeat(B, 1, 1), lat0["gaussian_window"].repeat(B, 1, 1)).float(),
                                                            field, w)), 6)
        out["observed_over_shared"] = {what: round(min(out[what]["observed"]) / min(out[what]["shared"]), 4)
                                       for what in ("inner_loop_ms", "fit_step_ms", "gather_ms")}
        res["fractions"][str(f)] = out
    print(json.dumps(res))


if __name__ == "__main__":
    main()
