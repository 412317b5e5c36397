"""Shared by tests/test_quad_terminal_host.py: the host build of the lane-quad terminal knot (tests/_emu/term_emu.cpp: the lane emulator plus the two
terminal programs as entry points) behind numpy arguments."""
import ctypes as C

import numpy as np

import walk_ref as wr
from conftest import pkg

DP = C.POINTER(C.c_double)
WAVE, QUAD = 0, 1      # program of term_emu_terminal


def build_emu(tmpdir):
    raw = wr.build_so(tmpdir, "term_emu.cpp", "libhsddp_term_emu.so")
    raw.term_emu_terminal.argtypes = [C.c_void_p, C.c_int, DP, C.c_void_p, C.c_int, DP]
    raw.term_emu_records.argtypes = [C.c_void_p, C.c_int, DP]
    raw.term_emu_set_al.argtypes = [C.c_void_p, C.c_int, C.c_double, C.c_double, C.c_double, C.c_double]
    return pkg._abi.bind(raw), raw


def terminal(raw, s, program, eps, opt, wr):
    """One evaluation of every terminal slot the quad path owns; eps: [batch].  Returns [batch, nph, 4] = cost, defect^2, max |h|, min g."""
    eps = np.ascontiguousarray(eps, dtype=np.float64)
    assert eps.shape == (s.batch,)
    out = np.zeros((s.batch, len(s.phases), 4))
    assert raw.term_emu_terminal(s.h, program, eps.ctypes.data_as(DP), C.byref(opt), 1 if wr else 0, out.ctypes.data_as(DP)) == 0
    return out


def records(raw, s, phase):
    """[batch, 6] = Phibase, Phi, th[0..3]."""
    out = np.zeros((s.batch, 6))
    assert raw.term_emu_records(s.h, phase, out.ctypes.data_as(DP)) == 0
    return out


def state(raw, s):
    """Everything a terminal knot may write, per phase: X, XSIM, DEFECT and the terminal records."""
    return [dict(X=s.field(i, "X"), XSIM=s.field(i, "XSIM"), DEFECT=s.field(i, "DEFECT"), REC=records(raw, s, i)) for i in range(len(s.phases))]
