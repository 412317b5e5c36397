"""CPU test: what the compiler made of k_rollout_quad in the product build (make -C cafe-mpc_amd/csrc resources-quad: hsddp_quad.hip with the Makefile's
flags, device code only).  The kernel's candidate loop wraps a knot program that fills the register file; that it needs no scratch rests on the
compiler NOT moving loop-invariant work in front of the loop (hsddp_quad.hip, Makefile QUAD_FLAGS).  A compiler that starts doing so again shows
here, not as a slower probe launch nobody looks at.

The target compiles the device code of that one file: about five seconds.  It covers the Makefile's build only: a one-command build of
hsddp_hip.hip (tests/test_refs_host.py, tests/test_ensemble_host.py) includes the kernel without QUAD_FLAGS and gets about 90 B of scratch per lane."""
import os
import re
import subprocess

from conftest import ROOT


def test_quad_kernel_has_no_scratch_and_fits_four_workgroups_per_cu():
    out = subprocess.run(["make", "--no-print-directory", "-C", os.path.join(ROOT, "cafe-mpc_amd", "csrc"), "resources-quad"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    block = out.stdout[out.stdout.index("k_rollout_quad"):]
    val = lambda key: int(re.search(re.escape(key) + r"\D*?(\d+)", block).group(1))
    print(block[:900])
    assert val("ScratchSize [bytes/lane]:") == 0
    assert val("Occupancy [waves/SIMD]:") == 1
    assert val("LDS Size [bytes/block]:") <= 40 * 1024      # four workgroups (one wave per SIMD) in a CU's 160 KiB
