"""Shared by tests/test_touchdown_host.py and tests/test_touchdown_gpu.py: the host build of the terminal programs with per-problem touchdown heights
(tests/_emu/tdh_emu.cpp) behind numpy arguments, and the inputs both files use for the terrain lookup."""
import ctypes as C

import numpy as np

import walk_ref as wr
from conftest import pkg

DP = C.POINTER(C.c_double)
IP = C.POINTER(C.c_int)
WAVE, QUAD = 0, 1      # program of tdh_emu_terminal


def build_emu(tmpdir):
    raw = wr.build_so(tmpdir, "tdh_emu.cpp", "libhsddp_tdh_emu.so")
    raw.term_emu_records.argtypes = [C.c_void_p, C.c_int, DP]
    raw.term_emu_set_al.argtypes = [C.c_void_p, C.c_int, C.c_double, C.c_double, C.c_double, C.c_double]
    raw.tdh_emu_terminal.argtypes = [C.c_void_p, C.c_int, DP, C.c_void_p, C.c_int, DP, DP]
    raw.tdh_emu_get_al.argtypes = [C.c_void_p, C.c_int, DP, DP]
    raw.tdh_emu_terrain.argtypes = [DP, IP, C.c_int, C.c_int, C.c_int, C.c_int] + [C.c_double] * 5 + [C.c_int, C.c_int, C.POINTER(DP), IP, IP, IP, DP]
    raw.tdh_emu_check_set.argtypes = [C.c_int, C.c_int, C.c_int, IP, IP, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int]
    raw.tdh_emu_check_terrain.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int] + [C.c_double] * 5 + [C.c_void_p, C.c_void_p, C.c_int]
    return pkg._abi.bind(raw), raw


def terminal(raw, s, program, eps, opt, wr, heights=None):
    """One evaluation of every terminal slot; eps [batch]; heights [batch, nph, 4] by leg or None (the programs without the switch).
    Returns [batch, nph, 4] = cost, defect^2, max |h|, min g."""
    eps = np.ascontiguousarray(eps, dtype=np.float64)
    hp = None
    if heights is not None:
        heights = np.ascontiguousarray(heights, dtype=np.float64)
        assert heights.shape == (s.batch, len(s.phases), 4)
        hp = heights.ctypes.data_as(DP)
    out = np.zeros((s.batch, len(s.phases), 4))
    assert raw.tdh_emu_terminal(s.h, program, eps.ctypes.data_as(DP), C.byref(opt), 1 if wr else 0, hp, out.ctypes.data_as(DP)) == 0
    return out


def records(raw, s, phase):
    """[batch, 6] = Phibase, Phi, th[0..3]."""
    out = np.zeros((s.batch, 6))
    assert raw.term_emu_records(s.h, phase, out.ctypes.data_as(DP)) == 0
    return out


def al_params(raw, s, phase):
    sg, lm = np.zeros((s.batch, 4)), np.zeros((s.batch, 4))
    raw.tdh_emu_get_al(s.h, phase, sg.ctypes.data_as(DP), lm.ctypes.data_as(DP))
    return sg, lm


def state(raw, s):
    return [dict(X=s.field(i, "X"), XSIM=s.field(i, "XSIM"), DEFECT=s.field(i, "DEFECT"), REC=records(raw, s, i)) for i in range(len(s.phases))]


def td_legs(phases):
    """[nph, 4] bool: the touchdown legs of each phase."""
    return np.array([pkg.problems.touchdown_legs(p["desc"]) for p in phases])


def mixed_heights(batch, nph, seed=7):
    """Heights within +-0.05 m that differ per problem, per phase AND between the legs of one problem."""
    r = np.random.default_rng(seed)
    return np.round(r.uniform(-0.05, 0.05, size=(batch, nph, 4)), 4)


def al_sum(th, sg, lm, nt):
    """sum over the touchdown feet in foot order of 0.5 sigma h^2 + lambda h, added term by term as the kernels do."""
    c = np.zeros(th.shape[0])
    for i in range(nt):
        c = c + 0.5 * sg[:, i] * th[:, i] * th[:, i]
        c = c + lm[:, i] * th[:, i]
    return c


# ---- the terrain lookup's inputs (CPU test 3, GPU test 5): 3 maps of 5 x 4 cells, B = 17
def lookup_terrain():
    r = np.random.default_rng(11)
    H = np.round(r.uniform(-0.05, 0.05, size=(3, 4, 5)), 4)
    return pkg.sim.Terrain(H, x0=-0.3, y0=-0.25, cx=0.2, cy=0.15)


def lookup_map(batch=17):
    return (np.arange(batch) * 2 % 3).astype(np.int32)


def lookup_footholds(batch, h1, seed):
    """foot_pos [batch, h1, 12] whose terminal rows lie inside the grid, outside it on every side, and hold one NaN."""
    r = np.random.default_rng(seed)
    fp = r.uniform(-0.25, 0.65, size=(batch, h1, 12))
    fp[:, :, 1::3] = r.uniform(-0.2, 0.3, size=(batch, h1, 4))
    t = fp[:, -1].reshape(batch, 4, 3)
    t[0, 0, 0] = -5.0; t[1 % batch, 1, 0] = 7.0; t[2 % batch, 2, 1] = -3.0; t[3 % batch, 3, 1] = 4.0; t[4 % batch, 0, :2] = (-9.0, 9.0); t[5 % batch, 1, 0] = np.nan
    t[6 % batch, 2, 0] = -0.3; t[7 % batch, 3, 0] = 0.7      # on the grid's first edge / on its far edge
    fp[:, -1] = t.reshape(batch, 12)
    return fp


def emu_terrain(raw, terrain, map_of, z_ground, batch, feet):
    """k_td_terrain's loop on the host.  feet: per phase None (off) or (foot_pos rows [*, 12] as [batch, h1, 12] or [h1, 12]).  Returns [nph, batch, 4]."""
    H = terrain.grid()
    nph = len(feet)
    keep, ptrs, pb, hz, on = [], (DP * nph)(), np.zeros(nph, dtype=np.int32), np.zeros(nph, dtype=np.int32), np.zeros(nph, dtype=np.int32)
    for i, f in enumerate(feet):
        if f is None:
            continue
        f = np.ascontiguousarray(f, dtype=np.float64); keep.append(f)
        ptrs[i] = f.ctypes.data_as(DP); on[i] = 1
        hz[i] = f.shape[-2] - 1; pb[i] = f.shape[-2] if f.ndim == 3 else 0
    mo = None if map_of is None else np.ascontiguousarray(map_of, dtype=np.int32)
    out = np.full((nph, batch, 4), np.nan)
    raw.tdh_emu_terrain(H.ctypes.data_as(DP), None if mo is None else mo.ctypes.data_as(IP), 1, H.shape[2], H.shape[1], H.shape[0], terrain.x0, terrain.y0, terrain.cx, terrain.cy,
                        float(z_ground), nph, batch, ptrs, pb.ctypes.data_as(IP), hz.ctypes.data_as(IP), on.ctypes.data_as(IP), out.ctypes.data_as(DP))
    return out
