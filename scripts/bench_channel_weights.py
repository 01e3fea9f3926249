"""Cost of the per-channel loss weights (include/enf_hip.h, "Weighted loss": enf_fit_step_cw): the one-call inner step at the
bench's fit shape (BASELINE config 2: 16 signals, 64 latents, 512 sampled points, D = 128, H = 2, bf16) with per-point weights
(enf_fit_step_w) and with per-channel weights (enf_fit_step_cw), at O = 1 and O = 3, in ONE process, interleaved rounds, hipEvent
pairs on the launch stream, median of --iters single calls after --warmup (the protocol of scripts/bench_determinism.py).
With --parent-tree DIR (a checkout of the parent commit with its library built) the per-point leg is also measured on the parent's
code, in a child process of its own before and after the rounds: the existing path must not have moved.  Prints one JSON line; with
--out FILE also writes it there.

  python scripts/bench_channel_weights.py [--iters 100] [--warmup 10] [--rounds 3] [--parent-tree DIR] [--out profiles/channel_weights.json]
"""
import argparse
import json
import os
import subprocess
import sys
from types import SimpleNamespace as NS

HERE = os.path.dirname(os.path.abspath(__file__))

D, H, C = 128, 2, 16
B, Z, N = 16, 64, 512


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


def measure(args, channel):
    """{"O=1": {"point": [...], "channel": [...]}, "O=3": ...}: medians per round, ms; ``channel`` False: the per-point leg only"""
    import torch
    from enf_pde_amd.enf.models import EquivariantCrossAttentionNeF
    from enf_pde_amd.enf.steerable_attention.invariant import get_ca_invariant
    dev = torch.device("cuda:0")
    inv = get_ca_invariant(NS(invariant_type="rel_pos_periodic", num_in=2))
    legs = {}
    for O in (1, 3):
        g = torch.Generator().manual_seed(0)
        x = (torch.rand(B, N, 2, generator=g) * 2 - 1).to(dev)
        p = (torch.rand(B, Z, 2, generator=g) * 2 - 1).to(dev)
        a = (1 + 0.1 * torch.randn(B, Z, C, generator=g)).to(dev)
        s = torch.full((B, Z, 1), 0.25, device=dev)
        target = torch.randn(B, N, O, generator=g).to(dev)
        cw = (torch.rand(B, N, O, generator=g) * 2).to(dev)
        cw[cw < 0.5] = 0
        w = cw[..., 0].contiguous()
        nef = EquivariantCrossAttentionNeF(num_hidden=D, num_heads=H, num_layers=0, num_out=O, latent_dim=C, cross_attn_invariant=inv,
                                           precision="bf16")
        params = nef.init(1, device=dev)
        loss = torch.zeros(1, device=dev)

        def step(kw, nef=nef, params=params, loss=loss, x=x, p=p, a=a, s=s, target=target):
            def fn():
                with torch.no_grad():
                    nef.mse_value_and_latent_grads(params, x, p, a, s, target, grad_scale=B, loss_out=loss, **kw)
            return fn
        legs[f"O={O}"] = {"point": step({"weight": w})}
        if channel:
            legs[f"O={O}"]["channel"] = step({"channel_weight": cw})
    out = {o: {k: [] for k in legs[o]} for o in legs}
    for _ in range(args.rounds):                     # interleaved: all legs see the same box state
        for o in legs:
            for k, fn in legs[o].items():
                out[o][k].append(round(median_ms(fn, args.iters, args.warmup), 4))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--parent-tree", default=None, help="a checkout of the parent commit, library built: its enf_fit_step_w is measured too")
    ap.add_argument("--tree", default=None, help=argparse.SUPPRESS)          # child mode: import the package from this checkout
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.tree is not None:                        # the child: the parent's package and library, the per-point leg only
        sys.path.insert(0, os.path.abspath(args.tree))
        print("RESULT " + json.dumps(measure(args, channel=False)))
        return
    sys.path.insert(0, os.path.dirname(HERE))

    def parent_leg():
        if args.parent_tree is None:
            return None
        cmd = [sys.executable, os.path.abspath(__file__), "--tree", args.parent_tree, "--iters", str(args.iters), "--warmup", str(args.warmup),
               "--rounds", str(args.rounds)]
        env = {k: v for k, v in os.environ.items() if k != "ENF_HIP_LIB"}      # the child loads the library of its own tree
        txt = subprocess.run(cmd, check=True, capture_output=True, text=True, env=env, timeout=300).stdout
        return json.loads([ln for ln in txt.splitlines() if ln.startswith("RESULT ")][-1][len("RESULT "):])
    before = parent_leg()
    own = measure(args, channel=True)
    after = parent_leg()
    res = {"D": D, "H": H, "precision": "bf16", "B,Z,N": [B, Z, N], "iters": args.iters, "rounds": args.rounds,
           "clock": "hipEvent pair around each call, median per round", "fit_step_ms": own,
           "channel_over_point": {o: round(min(v["channel"]) / min(v["point"]), 4) for o, v in own.items()},
           "extra_bytes_read": {o: 4 * B * N * (int(o[2:]) - 1) for o in own}}
    if before is not None:
        res["parent_commit_point_fit_step_ms"] = {"before": {o: v["point"] for o, v in before.items()},
                                                  "after": {o: v["point"] for o, v in after.items()}}
        res["point_over_parent_point"] = {o: round(min(own[o]["point"]) / min(before[o]["point"] + after[o]["point"]), 4) for o in own}
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
