"""The shared-latent backward's cross-wave reduce (enf_pair_bwd.hip, SHARED: the eight waves of a workgroup own one latent, park their
result tiles in LDS and add them there, so a gradient element gets one float atomic per workgroup instead of one per wave).

Flagged against unflagged enf_fit_step_w in the manner and with the bounds of tests/test_gpu_shared_backward.py -- the loss within the
forward tolerance tau (tests/test_gpu_forward.py: TOL, max|diff| / max|ref|), dp, da, ds within 20 tau -- at the shapes (B, N, Z) that
file does not reach.  The bounds are that file's, not this kernel's: the per-pair arithmetic is unchanged and the reduce only moves
where the fp32 sums over a workgroup's eight query tiles are taken.  Every figure is printed before it is asserted.

(3, 260, 130) at (D, H) = (64, 2): Z ceil(N / 128) = 390 > 256 selects the launcher's other nsplit rule (the sweep of
enf_pair_bwd_nsplit on Z latents: nsplit 2 for 17 query tiles), so split 0 holds 9 tiles -- wave 0 runs two, the other seven a tile past
the end on their second step, which must contribute zeros -- and split 1 holds 8.
(16, 512, 64) at (128, 2), bf16 only: the benchmark's own instantiation (rel_pos_periodic as a compile-time invariant), 32 tiles in 4
splits, every wave one tile.
(2, 8, 1), bf16 only: one ragged tile, seven waves without one, two signals in the 16-row A operand.

The same comparisons on the parent commit's library (direct float atomics from every wave), as max|flagged - plain| / max|plain| of
(loss, dp, da, ds), one MI355X (profiles/step0.json has this build's beside them, equal to two digits everywhere):
(3, 260, 130) f32 1.1e-7, 1.7e-6, 4.1e-6, 2.3e-6; bf16 2.4e-6, 4.6e-3, 4.8e-3, 6.8e-3; (16, 512, 64) bf16 1.2e-6, 7.0e-3, 5.3e-3, 6.1e-3;
(2, 8, 1) bf16 0, 6.0e-3, 6.7e-3, 2.7e-3; (2, 8, 1) f32 0, 1.9e-6, 1.1e-6, 0.414.
(2, 8, 1) in f32 is therefore NOT a case here: the parent itself exceeds 20 tau = 4e-4 on ds there, with the same 0.414 as this build.
With one latent the softmax weight is 1 and d logit = att (d ybar . n~ - delta) is the difference of two equal numbers, so d sigma is
rounding noise in both the flagged and the unflagged step and its relative deviation says nothing about either; dp and da of that
case agree to 2e-6.  The bounds stay the project's."""
import pytest
import torch

from tests.helpers import build_nef
from tests.test_gpu_forward import TOL
from tests.test_gpu_shared_backward import SHARED, VARIANTS, _case, _fit, _dev_rel, _delta_tail

pytestmark = pytest.mark.gpu

CASES = [(3, 260, 130, 64, 2, "f32"), (3, 260, 130, 64, 2, "bf16"), (16, 512, 64, 128, 2, "bf16"), (2, 8, 1, 128, 2, "bf16")]


def _nsplit(N, Z):
    """enf_launch.h: enf_pair_bwd_shared_nsplit (the kernel's own B is 1)"""
    ntiles = (N + 15) // 16
    if Z * ((N + 127) // 128) <= 256:
        return (ntiles + 7) // 8
    ns = 1
    while Z * ns < 256 and ns * 2 <= ntiles:
        ns *= 2
    return ns


@pytest.mark.parametrize("B,N,Z,D,H,precision", CASES)
def test_reduced_sums_flagged_against_unflagged(cuda, B, N, Z, D, H, precision):
    c = _case(B, N, Z, D, H)
    nef = build_nef(c.cfg, precision)
    nef.pair_variants = VARIANTS
    params = nef.load_params(c.prm, device=cuda)
    plain, flagged = _fit(cuda, nef, params, c, 0), _fit(cuda, nef, params, c, SHARED)
    devs = {k: _dev_rel(getattr(flagged, k), getattr(plain, k)) for k in ("loss", "dp", "da", "ds")}
    ns, ntiles = _nsplit(N, Z), (N + 15) // 16
    per_split = [(ntiles - s + ns - 1) // ns for s in range(ns)]
    tail_f = _delta_tail(nef, flagged.ws, B, N, Z)
    print("shared backward reduce", (B, N, Z, D, H), precision, "applies", flagged.applies, "nsplit", ns, "tiles per split", per_split,
          "tile steps per wave", [(t + 7) // 8 for t in per_split], "waves with a tile in the last step", [(t - 1) % 8 + 1 for t in per_split],
          "max|flagged - plain| / max|plain|", devs)
    assert flagged.applies == 1 and plain.applies == 0
    assert bool((tail_f == -1).all())                      # the shared backward ran: signals 1.. have no delta
    assert all(bool(torch.isfinite(getattr(flagged, k)).all()) for k in devs)
    assert devs["loss"] < TOL[precision], devs
    for k in ("dp", "da", "ds"):
        assert devs[k] < 20 * TOL[precision], (k, devs)
