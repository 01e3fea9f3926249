"""Cost of the per-signal / per-point errors (include/enf_hip.h, "Per-signal and per-point errors") at the bench's fit shape
(16 signals, 64 latents, 512 sampled points, D = 128, H = 2, bf16, per-point weights), in ONE process, interleaved rounds, hipEvent
pairs on the launch stream, median of --iters single calls after --warmup; the best of the rounds is reported.  Three pairs:

  step          enf_fit_step_w                        against  enf_fit_step_e with err alone
  step_loss_b   enf_fit_step_w                        against  enf_fit_step_e with err and loss_b (one more small launch)
  final_loss    enf_forward + enf_mse_value_grad_w    against  enf_eval_loss (err, loss_b and the scalar loss)

Prints one JSON line; --out FILE also writes it there (profiles/fit_errors.json).

  python scripts/bench_fit_errors.py [--iters 200] [--warmup 20] [--rounds 5] [--out profiles/fit_errors.json]
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
B, Z, N = 16, 64, 512


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
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
    x = (torch.rand(N, 2, generator=g) * 2 - 1).to(dev)                    # shared by the signals: x_bstride = 0, as the fit passes it
    p = (torch.rand(B, Z, 2, generator=g) * 2 - 1).to(dev)
    a = (1 + 0.1 * torch.randn(B, Z, C, generator=g)).to(dev)
    s = torch.full((B, Z, 1), 0.25, device=dev)
    y = torch.randn(B, N, O, generator=g).to(dev)
    w = (2 * torch.rand(B, N, generator=g)).to(dev)
    desc = nef._desc(B, N, Z)
    nbytes = int(lib.enf_workspace_bytes(ctypes.byref(desc)))
    ws = torch.empty(nbytes, device=dev, dtype=torch.uint8)
    packed = nef.pack(params)
    loss = torch.zeros(1, device=dev)
    dp, da, ds = torch.empty_like(p), torch.empty_like(a), torch.empty_like(s)
    err, loss_b, out = torch.empty(B, N, device=dev), torch.empty(B, device=dev), torch.empty(B, N, O, device=dev)
    st = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    head = (ctypes.byref(desc), P(x), 0, P(p), P(a), P(s), P(packed))

    def step_w():
        _lib.check(lib.enf_fit_step_w(*head, P(y), float(B), P(loss), P(dp), P(da), P(ds), P(ws), nbytes, P(w), 0, st))

    def step_e():
        _lib.check(lib.enf_fit_step_e(*head, P(y), float(B), P(loss), P(dp), P(da), P(ds), P(ws), nbytes, P(w), None, P(err), None, 0, st))

    def step_e_b():
        _lib.check(lib.enf_fit_step_e(*head, P(y), float(B), P(loss), P(dp), P(da), P(ds), P(ws), nbytes, P(w), None, P(err), P(loss_b), 0, st))

    def final_old():
        _lib.check(lib.enf_forward(*head, P(out), None, None, P(ws), nbytes, st))
        _lib.check(lib.enf_mse_value_grad_w(P(out), P(y), P(w), out.numel(), O, 1.0, None, P(loss), None, 0, 0, st))

    def final_new():
        _lib.check(lib.enf_eval_loss(*head, P(y), P(w), None, P(loss), P(err), P(loss_b), P(ws), nbytes, 0, st))

    pairs = {"step": (step_w, step_e), "step_loss_b": (step_w, step_e_b), "final_loss": (final_old, final_new)}
    times = {k: ([], []) for k in pairs}
    for _ in range(args.rounds):                     # interleaved: both sides of a pair see the same box state
        for k, fns in pairs.items():
            for side, fn in enumerate(fns):
                times[k][side].append(median_ms(fn, args.iters, args.warmup))
    res = {"shape": {"B": B, "Z": Z, "N": N, "D": D, "H": H, "O": O, "precision": "bf16", "weights": "per point"},
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
