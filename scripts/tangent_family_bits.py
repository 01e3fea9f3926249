"""Bits of the first-order forward-mode family, for a comparison of two builds of the library: nef.tangent without and with xdot and
nef.gn_product in deterministic mode, on the base inputs of tests/tangent_x_ref.py (rel_pos_periodic, B = 3, N = 50, Z = 7) for the five
compiled (D, H) shapes and both precisions.  Prints one line per result with the SHA-256 of its bytes.  Run it once per build in a fresh
process (an argument names the root of another built checkout, whose package and library then run) and diff the two outputs: every line
must be equal.

  python scripts/tangent_family_bits.py /path/to/parent/checkout > parent.txt
  python scripts/tangent_family_bits.py > new.txt && diff parent.txt new.txt
"""
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(128, 2), (64, 2), (128, 1), (64, 1), (64, 4)]


def main():
    import numpy as np
    import torch
    sys.path.insert(0, os.path.abspath(sys.argv[1]) if len(sys.argv) > 1 else ROOT)
    from tests.helpers import build_nef
    from tests.tangent_x_ref import case
    dev = torch.device("cuda:0")
    t = lambda v: torch.tensor(np.asarray(v), dtype=torch.float32, device=dev)
    sha = lambda v: hashlib.sha256(v.detach().cpu().contiguous().numpy().tobytes()).hexdigest()
    for D, H in SHAPES:
        cfg, prm, xpas, xd, tang = case("rel_pos_periodic", D=D, H=H)[:5]
        x, p, a, s = (t(v) for v in xpas)
        dp, da, ds = (t(v) for v in tang)
        for prec in ("f32", "bf16"):
            nef = build_nef(cfg, prec)
            nef.deterministic = True
            P = nef.load_params(prm, device=dev)
            res = dict(zip(("out", "tan"), nef.tangent(P, x, p, a, s, dp=dp, da=da, dwindow=ds)))
            res.update(zip(("out_x", "tan_x"), nef.tangent(P, x, p, a, s, dp=dp, da=da, dwindow=ds, xdot=t(xd))))
            res["tan_x_alone"] = nef.tangent(P, x, p, a, s, xdot=t(xd), return_out=False)[1]
            res.update(zip(("gp", "ga", "gwindow"), nef.gn_product(P, x, p, a, s, vp=dp, va=da, vwindow=ds)))
            torch.cuda.synchronize()
            for k, v in res.items():
                print(f"{D}x{H} {prec} {k} {sha(v)}")


if __name__ == "__main__":
    main()
