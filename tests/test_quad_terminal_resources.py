"""CPU test: what the compiler made of k_rollout_quad_term, the lane-quad kernel of the terminal knots, in the product build (make -C cafe-mpc_amd/csrc
resources-quad-term: hsddp_quad.hip with the Makefile's flags, device code only, about five seconds).  It is held to the limits of the running-knot
kernel beside it (tests/test_quad_kernel_resources.py): at most 256 VGPR and 210 AGPR, nothing in scratch, one wave per SIMD, four workgroups'
worth of LDS per CU - its candidate loop wraps a knot program with the same block contact solve, and the same compiler switch keeps it free of scratch."""
import os
import re
import subprocess

from conftest import ROOT


def test_quad_terminal_kernel_keeps_the_running_knot_kernels_limits():
    out = subprocess.run(["make", "--no-print-directory", "-C", os.path.join(ROOT, "cafe-mpc_amd", "csrc"), "resources-quad-term"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    block = out.stdout[out.stdout.index("k_rollout_quad_term"):]
    assert block.count("Function Name") == 1      # the last kernel of the file: its figures and nothing else
    val = lambda key: int(re.search(re.escape(key) + r"\D*?(\d+)", block).group(1))
    print(block[:900])
    assert val("VGPRs:") <= 256
    assert val("AGPRs:") <= 210
    assert val("ScratchSize [bytes/lane]:") == 0
    assert val("Occupancy [waves/SIMD]:") == 1
    assert val("LDS Size [bytes/block]:") <= 40 * 1024
