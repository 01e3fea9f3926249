"""The auto-decoder trainer's latent-ODE phase at config_navier_stokes_nonmaml.yaml's shapes: 4 latents of width 16 per signal,
decoder width 128 with 2 heads, a 64 x 64 grid, max_num_sampled_points 2048, batch 8, PonitaODEGen with 3 layers of 128
(basis 64, degree 3), Euler with dt 1.  Times NonMetaPDETrainer.ode_train_step (8 x 10 signal-frames at 2048 points each,
latent backward, 9 derivative evaluations; eager, and with training.graph_ode_training) and val_step (8 x 20 signal-frames on the full grid in chunks of 2048).
5 warm-up steps, then the median of 20 steps timed one by one with hipEvents.

Every step runs under its own time limit, and the limit is real: this process never opens the GPU.  It starts one child per
phase (train, train_graphed, val; one after the other), the child reports every finished step on a line of its standard
output, and a child whose next line does not arrive within --step-timeout seconds (--setup-timeout for the first: imports,
initialisation, kernel loading) is killed, whatever it hangs in -- a kernel, a synchronize, the interpreter.  After a child
that failed or was killed no further one is started.  Prints one JSON line.
Usage: python scripts/bench_nonmaml_ode.py [--precision bf16|f32] [--steps 20] [--warmup 5] [--step-timeout 60] [--setup-timeout 300]"""
import argparse
import json
import os
import queue
import statistics
import subprocess
import sys
import threading

PHASES = ("train", "train_graphed", "val")
ap = argparse.ArgumentParser()
ap.add_argument("--precision", default="bf16")
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--step-timeout", type=int, default=60)
ap.add_argument("--setup-timeout", type=int, default=300)
ap.add_argument("--signals", type=int, default=64, help="rows of the latent table (the config's 8192 only make the table larger)")
ap.add_argument("--phase", choices=PHASES, help="(internal) run this phase in this process, one JSON line per step")
args = ap.parse_args()
B, Z, C, GRID, FRAMES = 8, 4, 16, 64, 20


def run_phase(phase):
    """The child: build the trainer, run warmup + steps of ``phase``, print {"step": i, "ms": ...} after each and the value last."""
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from types import SimpleNamespace as NS

    import torch

    from enf_pde_amd.fitting import get_model_pde
    from enf_pde_amd.fitting.trainers import NonMetaPDETrainer
    from enf_pde_amd.enf.latents.autodecoder import PositionOrientationFeatureAutodecoder

    dev = torch.device("cuda:0")
    cfg = NS(nef=NS(num_in=2, num_out=1, num_layers=0, num_hidden=128, num_heads=2, condition_value_transform=True, latent_dim=C,
                    num_latents=Z, use_gaussian_window=True, embedding_type="rff", embedding_freq_multiplier_invariant=0.05,
                    embedding_freq_multiplier_value=0.2, invariant_type="rel_pos_periodic"),
             node=NS(name="ponita", num_layers=3, num_hidden=128, widening_factor=2, kernel_size="global", degree=3, basis_dim=64,
                     dt=1, method="euler"),
             training=NS(max_num_sampled_points=2048, graph_ode_training=phase == "train_graphed"),
             optimizer=NS(learning_rate_enf=1e-4, learning_rate_codes=1e-3))
    nef, ode = get_model_pde(cfg, precision=args.precision)
    lin = torch.linspace(-1, 1, GRID)
    coords = torch.stack(torch.meshgrid(lin, lin, indexing="xy"), -1).reshape(-1, 2).to(dev)
    ad = PositionOrientationFeatureAutodecoder(args.signals, Z, C, 2, 0, gaussian_window_size=-1)
    tr = NonMetaPDETrainer(cfg, nef, ad, coords, seed=0, ode_model=ode)
    state = [tr.init_train_state()]
    g = torch.Generator().manual_seed(0)
    # a table as the nef phase leaves it: features away from their initial value of exactly 1, poses off the grid.  (From an
    # untouched table ode_train_step raises: a - 1 == 0 puts every LayerNorm of the ODE model at a constant vector, and the
    # roll-out's gradient leaves the fp32 range -- DESIGN.md section 5b.)
    P = state[0].params["autodecoder"]["params"]
    P["a"] = P["a"] + 0.1 * torch.randn(P["a"].shape, generator=g).to(dev)
    P["p_pos"] = P["p_pos"] + 0.02 * torch.randn(P["p_pos"].shape, generator=g).to(dev)
    # smooth travelling waves: (B, FRAMES, 64, 64, 1)
    k, ph = torch.randint(1, 4, (B, 2), generator=g).float(), torch.rand(B, generator=g) * 6.28
    tt = torch.arange(FRAMES).float()
    x, y = coords[:, 0].cpu(), coords[:, 1].cpu()
    traj = torch.sin(3.14159 * (k[:, None, None, 0] * x + k[:, None, None, 1] * y) + ph[:, None, None] + 0.2 * tt[None, :, None])
    traj = traj.reshape(B, FRAMES, GRID, GRID, 1).to(dev)
    idx = torch.randperm(args.signals, generator=g)[:B].to(dev)

    def train():
        loss, state[0] = tr.ode_train_step(state[0], (traj, idx))
        return [loss]

    fn = (lambda: list(tr.val_step(state[0], (traj, idx)))) if phase == "val" else train
    for i in range(args.warmup + args.steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        e1.synchronize()
        print(json.dumps({"step": i, "ms": e0.elapsed_time(e1)}), flush=True)
    print(json.dumps({"values": [float(v) for v in out]}), flush=True)


def watch(phase):
    """The parent's side of one phase: (timed milliseconds, last values); ends the script when the child fails or goes silent."""
    cmd = [sys.executable, os.path.abspath(__file__), "--phase", phase, "--precision", args.precision, "--steps", str(args.steps),
           "--warmup", str(args.warmup), "--signals", str(args.signals)]
    child = subprocess.Popen(cmd, stdout=subprocess.PIPE, text=True)
    lines = queue.Queue()
    threading.Thread(target=lambda: [lines.put(ln) for ln in child.stdout] + [lines.put(None)], daemon=True).start()
    ms, values, limit = [], None, args.setup_timeout
    try:
        while True:
            try:
                ln = lines.get(timeout=limit)
            except queue.Empty:
                sys.exit(f"{phase}: no step finished within {limit} s; the child was killed and nothing further is started")
            if ln is None:
                break
            rec = json.loads(ln)
            if "values" in rec:
                values = rec["values"]
            elif rec["step"] >= args.warmup:
                ms.append(rec["ms"])
            limit = args.step_timeout
        if child.wait(timeout=args.step_timeout) != 0 or values is None or len(ms) != args.steps:
            sys.exit(f"{phase}: the child ended with status {child.returncode} after {len(ms)} timed steps; nothing further is started")
    finally:
        if child.poll() is None:
            child.kill()
            child.wait()
    return ms, values


if args.phase:
    run_phase(args.phase)
else:
    (ms_train, (loss,)), (ms_train_graphed, _), (ms_val, (mse_in, mse_out)) = (watch(ph) for ph in PHASES)
    print(json.dumps({"workload": f"auto-decoder trainer, ODE phase: B={B} Z={Z} C={C} D=128 H=2 grid={GRID}^2 n_s=2048 ponita 3x128 basis 64 "
                                  f"euler, {args.precision} decoder",
                      "ms_ode_train_step_median": round(statistics.median(ms_train), 3), "ms_ode_train_step_min": round(min(ms_train), 3),
                      "ms_ode_train_step_max": round(max(ms_train), 3),
                      "ms_ode_train_step_graphed_evals_median": round(statistics.median(ms_train_graphed), 3),
                      "ms_val_step_median": round(statistics.median(ms_val), 3), "ms_val_step_min": round(min(ms_val), 3),
                      "ms_val_step_max": round(max(ms_val), 3), "steps": args.steps, "warmup": args.warmup,
                      "loss": loss, "val_mse_in": mse_in, "val_mse_out": mse_out}))
