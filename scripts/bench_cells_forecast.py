"""Cost of the per-value weights on grouped observations and of the decode-free roll-out loss on cells (include/enf_hip.h, "Grouped
observations": the _gc calls; nef.cell_fit_loss) at the bench's fit shape with groups of 4 (16 signals, 64 latents, 512 quadrature
rows = 128 cells per signal, D = 128, H = 2, bf16), in ONE process, interleaved rounds, hipEvent pairs on the launch stream, median
of --iters single calls after --warmup; the best of the rounds is reported.  Two pairs:

  step      enf_fit_step_g (one weight per observation)   against  enf_fit_step_gc (one weight per observed value)
  rollout   the roll-out loss of ode_train_step(cells=) over T = 10 frames (160 signal-frames) and its gradient w.r.t. the rolled-out
            latents: the composed route (nef.apply, nef.cell_mse, backward)   against   nef.cell_fit_loss (one enf_fit_step_gc over
            the signal-frames, the backward scales its gradients).  The solver and the ODE model are the same on both sides and
            are left out.

Prints one JSON line; --out FILE also writes it there (profiles/cells_forecast.json).

  python scripts/bench_cells_forecast.py [--iters 100] [--warmup 10] [--rounds 5] [--out profiles/cells_forecast.json]
"""
import argparse
import ctypes
import json
import os
import sys
from types import SimpleNamespace as NS

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from enf_pde_amd import _lib  # noqa: E402
from enf_pde_amd.enf.models import EquivariantCrossAttentionNeF  # noqa: E402
from enf_pde_amd.enf.steerable_attention.invariant import get_ca_invariant  # noqa: E402
from scripts.bench_determinism import median_ms  # noqa: E402

D, H, C, O = 128, 2, 16, 1
B, Z, N, G, T = 16, 64, 512, 4, 10


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    lib = _lib.load()
    inv = get_ca_invariant(NS(invariant_type="rel_pos_periodic", num_in=2))
    nef = EquivariantCrossAttentionNeF(num_hidden=D, num_heads=H, num_layers=0, num_out=O, latent_dim=C, cross_attn_invariant=inv,
                                       precision="bf16", deterministic=False)
    params = nef.init(1, device=dev)
    g = torch.Generator().manual_seed(0)
    M = N // G
    x = (torch.rand(N, 2, generator=g) * 2 - 1).to(dev)                    # shared by the signals: x_bstride = 0, as the fit passes it
    q = (torch.rand(B, N, generator=g) / G + 0.5 / G).to(dev)
    p = (torch.rand(B, Z, 2, generator=g) * 2 - 1).to(dev)
    a = (1 + 0.1 * torch.randn(B, Z, C, generator=g)).to(dev)
    s = torch.full((B, Z, 1), 0.25, device=dev)
    y = torch.randn(B, M, O, generator=g).to(dev)
    w = (2 * torch.rand(B, M, generator=g)).to(dev)
    cw = (2 * torch.rand(B, M, O, generator=g)).to(dev)
    desc = nef._desc(B, N, Z)
    nbytes = int(lib.enf_workspace_bytes(ctypes.byref(desc)))
    ws = torch.empty(nbytes, device=dev, dtype=torch.uint8)
    packed = nef.pack(params)
    loss = torch.zeros(1, device=dev)
    dp, da, ds = torch.empty_like(p), torch.empty_like(a), torch.empty_like(s)
    st = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    head = (ctypes.byref(desc), P(x), 0, P(p), P(a), P(s), P(packed), P(y), G, P(q))
    tail = (float(B), P(loss), P(dp), P(da), P(ds), None, None, P(ws), nbytes, 0, st)

    def step_g():
        _lib.check(lib.enf_fit_step_g(*head, P(w), *tail))

    def step_gc():
        _lib.check(lib.enf_fit_step_gc(*head, P(cw), *tail))

    # the roll-out loss over B T signal-frames, every frame at its own sampled cells
    F = B * T
    xs = (torch.rand(F, N, 2, generator=g) * 2 - 1).to(dev)
    qs = (torch.rand(F, N, generator=g) / G + 0.5 / G).to(dev)
    ys = torch.randn(F, M, O, generator=g).to(dev)
    cws = (2 * torch.rand(F, M, O, generator=g)).to(dev)
    lat = [t.requires_grad_(True) for t in ((torch.rand(F, Z, 2, generator=g) * 2 - 1).to(dev),
                                            (1 + 0.1 * torch.randn(F, Z, C, generator=g)).to(dev), torch.full((F, Z, 1), 0.25, device=dev))]

    def composed():
        out = nef.apply(params, xs, *lat)
        torch.autograd.grad(nef.cell_mse(out, ys, G, qs, obs_channel_weight=cws), lat)

    def fused():
        torch.autograd.grad(nef.cell_fit_loss(params, xs, *lat, ys, G, qweight=qs, obs_channel_weight=cws), lat)

    pairs = {"step": (step_g, step_gc), "rollout": (composed, fused)}
    times = {k: ([], []) for k in pairs}
    for _ in range(args.rounds):                     # interleaved: both sides of a pair see the same box state
        for k, fns in pairs.items():
            for side, fn in enumerate(fns):
                times[k][side].append(median_ms(fn, args.iters, args.warmup))
    res = {"shape": {"B": B, "Z": Z, "N": N, "G": G, "D": D, "H": H, "O": O, "precision": "bf16", "rollout_frames": T, "signal_frames": F},
           "clock": "hipEvent pair around each call, median; best of the rounds", "iters": args.iters, "rounds": args.rounds}
    for k, (old, new) in times.items():
        res[k] = {"existing_ms": round(min(old), 4), "new_ms": round(min(new), 4), "new_over_existing": round(min(new) / min(old), 4),
                  "existing_rounds_ms": [round(v, 4) for v in old], "new_rounds_ms": [round(v, 4) for v in new]}
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
