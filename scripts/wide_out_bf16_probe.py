"""The bf16 derivative cases of tests/test_gpu_wide_out.py that exceed 7e-2 in the per-channel metric, decided with the rounding build:
the Jacobian w.r.t. x, the latent tangent and the tangent with xdot at num_out 17 and at num_out 2 (B = 3, N = 50, Z = 7, 64x2,
rel_pos_periodic), each through the plain f32 library, libenf_hip_f32r.so and the bf16 kernels.  Per pair (bf16 - f32r, oracle - f32r,
oracle - bf16, oracle - f32): the worst channel's max |difference| over max |oracle|, and the relative Frobenius norm.

  python scripts/wide_out_bf16_probe.py [--out profiles/wide_out_bf16.json]
"""
import argparse
import contextlib
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from enf_pde_amd import _lib  # noqa: E402
from tests import wide_out as WO, tangent_ref, tangent_x_ref  # noqa: E402
from tests import test_gpu_tangent as TT, test_gpu_tangent_x as TX  # noqa: E402
from tests.helpers import build_nef  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
args = ap.parse_args()

cuda = torch.device("cuda:0")
t = lambda v: torch.tensor(np.asarray(v), dtype=torch.float32, device=cuda)
npf = lambda v: v.detach().double().cpu().numpy()
res = {}

def three(run):
    out = {}
    for tag, prec, lib in (("f32", "f32", None), ("f32r", "f32", _lib.load_f32r()), ("bf16", "bf16", None)):
        with (_lib.using(lib) if lib is not None else contextlib.nullcontext()):
            out[tag] = run(prec)
            torch.cuda.synchronize()
    return out

def report(name, r, ref, axis=-1):
    row = {}
    for a, b, key in (("bf16", "f32r", "bf16-f32r"), ("f32r", None, "oracle-f32r"), ("bf16", None, "oracle-bf16"), ("f32", None, "oracle-f32")):
        other = ref if b is None else r[b]
        d = np.moveaxis(np.abs(r[a] - other), axis, -1)
        e = d.reshape(-1, d.shape[-1]).max(0) / np.abs(ref).max()
        row[key] = {"max_channel": float(e.max()), "argmax": int(e.argmax()), "frobenius": float(np.linalg.norm(r[a] - other) / np.linalg.norm(ref))}
    res[name] = row
    print(name, json.dumps(row), flush=True)

for O in (2, 17):
    c = WO.problem(O)
    def jac(prec):
        nef = build_nef(c.cfg, prec)
        return npf(nef.jacobian(nef.load_params(c.prm, device=cuda), t(c.x), t(c.p), t(c.a), t(c.s))[1])
    report(f"jacobian O={O}", three(jac), WO.jacobian_x(c), axis=2)
    ct = tangent_ref.case("rel_pos_periodic", O=O, freq=WO.FREQ)
    report(f"tangent O={O}", three(lambda prec: npf(TT._run(cuda, ct, prec)[1])), ct[5])
    cx = tangent_x_ref.case("rel_pos_periodic", O=O, freq=WO.FREQ)
    report(f"tangent with xdot O={O}", three(lambda prec: npf(TX._run(cuda, cx, prec)[1])), cx[7])
if args.out:
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
