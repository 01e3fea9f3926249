"""Host-side half of tests/test_gpu_stage_flags.py (no GPU): where ENF_STAGE_YBAR_HALF is ignored is written down, and the forward pair
launcher refuses -- instead of answering with fp32 rows -- a bf16 hand-off on a call it routes to the masked kernels."""
import os
import re
import shutil
import subprocess

from enf_pde_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "enf-pde_amd", "csrc")


def _read(*path):
    with open(os.path.join(ROOT, *path)) as f:
        return f.read()


def test_header_and_documents_name_relu_masks_among_the_ignored_cases():
    hdr = _read("include", "enf_hip.h")
    note = re.search(r"#define ENF_STAGE_YBAR_HALF 64u /\*(.*?)\*/", hdr, re.S).group(1)
    ignored = note[note.index("Ignored where it does not apply"):]
    for case in ("f32 mode", "ENF_STAGE_TAIL_SAVE", "split z-fold", "caller-owned `ybar`", "relu masks", "ENF_MASK_OFF"):
        assert case in ignored, case
    for doc in ("INTEGRATION.md", "DESIGN.md"):
        text = _read(doc)
        at = text.index("ENF_STAGE_YBAR_HALF")
        assert "relu masks" in text[at:at + 1200], doc


PROGRAM = r"""
#include <cstdio>
#include "enf_launch.h"
int main() {
  EnfDesc d{};
  d.B = 2; d.N = 40; d.Z = 9; d.H = 2; d.D = 128; d.C = 12; d.O = 2; d.dx = 2;
  d.invariant_id = 0; d.use_window = 1; d.precision = 1;                        // bf16
  unsigned word = 0;
  int bad = 0;
  for (int variant = 1; variant <= 2; ++variant)                                // latent-split, z-fold
    for (int mode = ENF_MASK_WRITE; mode <= ENF_MASK_READ; ++mode) {
      d.relu_masks = &word; d.mask_mode = mode; d.pair_fwd_variant = variant;
      if (enf_check_desc(&d) != ENF_OK) return 100;
      const EnfDims m = enf_dims(&d);
      const EnfLayout L = enf_layout(m);
      // no scratch of the z-fold: the launcher resolves to the latent-split kernel; both return before any launch
      const int both = enf_launch_pair_fwd(m, L, nullptr, nullptr, 0, nullptr, nullptr, nullptr, EnfFoldFwd{}, ENF_PAIR_PAIR | ENF_PAIR_YBAR_HALF, nullptr);
      const int fold = enf_launch_pair_fwd(m, L, nullptr, nullptr, 0, nullptr, nullptr, nullptr, EnfFoldFwd{}, ENF_PAIR_YBAR_HALF, nullptr);
      printf("variant %d mask_mode %d: run_pair 3 -> %d, run_pair 2 -> %d\n", variant, mode, both, fold);
      bad += both != ENF_EINVAL || fold != 0;
    }
  return bad;
}
"""


def test_pair_launcher_refuses_the_hand_off_on_a_masked_call(tmp_path):
    """enf_launch_pair_fwd(ENF_PAIR_PAIR | ENF_PAIR_YBAR_HALF, "run_pair 3" below) with relu masks on: ENF_EINVAL, before anything is
    launched (so this runs without a GPU); the hand-off bit on the fold alone (ENF_PAIR_YBAR_HALF, "run_pair 2": no pair stage, no masked
    kernel) is not an error.  A small program of its own,
    linked against the built library."""
    hipcc = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    assert os.path.exists(hipcc) and os.path.exists(_lib.LIB_PATH), "build the library first"
    src, exe = tmp_path / "pair_launcher.cpp", tmp_path / "pair_launcher"
    src.write_text(PROGRAM)
    libdir = os.path.dirname(_lib.LIB_PATH)
    r = subprocess.run([hipcc, "-O1", "-std=c++17", "-Wno-unused-function", "-Wno-unknown-pragmas", "-I", CSRC, str(src), "-o", str(exe),
                        "-L", libdir, "-l:" + os.path.basename(_lib.LIB_PATH), "-Wl,-rpath," + libdir], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    print(r.stdout)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr[-500:])
    assert r.stdout.count("run_pair 3 -> -1, run_pair 2 -> 0") == 4
