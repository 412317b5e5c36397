"""CPU tests of per-problem tracking references (include/hsddp_refs.h): the symbols, the packing of k_pack_refs (csrc/refs.hpp compiled for
the host) against a numpy statement, problems.stack_references / translate_references, and the C++ wrapper."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import pkg, ROOT

CSRC = os.path.join(ROOT, "cafe-mpc_amd", "csrc")
P = pkg.problems
NAMES = ("xr", "ur", "yr", "foot_pos", "foot_vel", "body_pos", "ref_contact")


def test_refs_header_symbols_match_binding_list():
    hdr = open(os.path.join(ROOT, "include", "hsddp_refs.h")).read()
    assert sorted(set(re.findall(r"\b(hsddp_[a-zA-Z_]+)\s*\(", hdr))) == sorted(pkg._abi.REFS_EXPORTS)
    others = set(pkg._abi.EXPORTS) | set(pkg._abi.ENSEMBLE_EXPORTS) | set(pkg._abi.HKD_EXPORTS)
    assert not set(pkg._abi.REFS_EXPORTS) & others
    assert "hsddp_set_references" not in open(os.path.join(ROOT, "include", "hsddp.h")).read()


LLVM_BIN = "/opt/rocm/lib/llvm/bin"


def gfx950_kernels(so, tmp):
    """Mangled names of the kernels in the gfx950 code objects of a library: its .hip_fatbin section is one offload bundle per translation unit (magic, entry
    count, then offset / size / triple of each entry); a kernel is a symbol with a kernel descriptor NAME.kd in an entry for gfx950."""
    fat = os.path.join(str(tmp), os.path.basename(str(so)) + ".fatbin")
    subprocess.check_call([os.path.join(LLVM_BIN, "llvm-objcopy"), "--dump-section", ".hip_fatbin=" + fat, str(so), os.devnull])
    data, magic, names, n = open(fat, "rb").read(), b"__CLANG_OFFLOAD_BUNDLE__", set(), 0
    assert data.startswith(magic)
    for m in re.finditer(magic, data):
        at, pos = m.start(), m.start() + len(magic) + 8
        for _ in range(int.from_bytes(data[pos - 8:pos], "little")):
            off, size, tl = (int.from_bytes(data[pos + 8 * i:pos + 8 * i + 8], "little") for i in range(3))
            triple = data[pos + 24:pos + 24 + tl].decode(); pos += 24 + tl
            if not triple.endswith("gfx950"):
                continue
            co = os.path.join(str(tmp), "%s.%d.co" % (os.path.basename(str(so)), n)); n += 1
            open(co, "wb").write(data[at + off:at + off + size])
            syms = subprocess.run([os.path.join(LLVM_BIN, "llvm-readelf"), "-sW", co], capture_output=True, text=True, check=True).stdout
            names |= {line.split()[-1][:-3] for line in syms.splitlines() if line.endswith(".kd") and " OBJECT " in line}
    return names


def test_fresh_hip_build_exports_the_refs_symbols(tmp_path):
    """A fresh one-command hipcc --offload-arch=gfx950 build of libhsddp_hip.so from hsddp_hip.hip alone (the product Makefile's flags, into a scratch
    directory): it exports the symbols, and its device code defines every kernel the product build of the Makefile defines - the files that build
    compiles on their own are included where the device pass sees them."""
    so = tmp_path / "libhsddp_hip.so"
    subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared", "-I", os.path.join(ROOT, "include"),
                           "-Wno-unused-value", "-DROLL_WPE=2", os.path.join(CSRC, "hsddp_hip.hip"), "-o", str(so)], timeout=1800)
    lib = ctypes.CDLL(str(so))
    for s in pkg._abi.REFS_EXPORTS + pkg._abi.EXPORTS:
        assert hasattr(lib, s), s
    pkg._abi.bind_refs(lib)
    subprocess.check_call(["make", "-C", CSRC], stdout=subprocess.DEVNULL)      # the product library (what build() makes; nothing to do if it is current)
    product, fresh = gfx950_kernels(os.path.join(ROOT, "cafe-mpc_amd", "libhsddp_hip.so"), tmp_path), gfx950_kernels(so, tmp_path)
    assert len([k for k in product if "k_sim_quad" in k]) == 27 and any("k_episode_impact_plant" in k for k in product) and any("k_rollout_quad_term" in k for k in product)
    assert sorted(product - fresh) == [], "kernels of the product build without device code in the one-command build"


def test_bind_refs_refuses_a_library_without_it(oracle_lib):
    with pytest.raises(RuntimeError):
        pkg._abi.bind_refs(oracle_lib)


# ------------------------------------------------------------------------------------------------ k_pack_refs on the host
DRIVER = r"""
#include <cstdio>
#include <string>
#include <vector>
#include "refs.hpp"
// argv[1]: directory.  meta.txt: n m p wb B h1 cur_pb b0 nb p0 np, then 7 flags (source given); files cur_<s>.bin, src_<s>.bin, dst_<s>.bin
// (s = segment index; int32 for segment 6); dst files are rewritten with the packed result
static std::vector<char> rd(const std::string& f) { std::vector<char> v; FILE* p = fopen(f.c_str(), "rb"); if (!p) return v; int c; while ((c = fgetc(p)) != EOF) v.push_back((char)c); fclose(p); return v; }
int main(int argc, char** argv) {
    std::string d = argv[1];
    FILE* m = fopen((d + "/meta.txt").c_str(), "r");
    int n, mm, p, wb, B, h1, pb, b0, nb, p0, np_, fl[7];
    if (fscanf(m, "%d %d %d %d %d %d %d %d %d %d %d", &n, &mm, &p, &wb, &B, &h1, &pb, &b0, &nb, &p0, &np_) != 11) return 1;
    for (int s = 0; s < 7; s++) if (fscanf(m, "%d", &fl[s]) != 1) return 2;
    fclose(m);
    hs::RefsPack R{};
    const int w[8] = {n, mm, p, 12, 12, 3, 4, wb ? 80 : 0};
    std::vector<std::vector<char>> cur(7), src(7), dst(8);
    for (int s = 0; s < 8; s++) {
        R.w[s] = w[s];
        if (s < 7) { cur[s] = rd(d + "/cur_" + std::to_string(s) + ".bin"); R.cur[s] = (const double*)cur[s].data();
                     if (fl[s]) { src[s] = rd(d + "/src_" + std::to_string(s) + ".bin"); R.src[s] = (const double*)src[s].data(); } }
        if (w[s]) { dst[s] = rd(d + "/dst_" + std::to_string(s) + ".bin"); R.dst[s] = (double*)dst[s].data(); }
    }
    R.h1 = h1; R.cur_pb = pb; R.b0 = b0; R.nb = nb; R.p0 = p0; R.np = np_;
    hs::refs_pack_host(R);
    for (int s = 0; s < 8; s++) if (w[s]) { FILE* f = fopen((d + "/dst_" + std::to_string(s) + ".bin").c_str(), "wb"); fwrite(dst[s].data(), 1, dst[s].size(), f); fclose(f); }
    return 0;
}
"""


@pytest.fixture(scope="module")
def host_pack(tmp_path_factory):
    d = tmp_path_factory.mktemp("refs")
    (d / "drv.cpp").write_text(DRIVER)
    exe = d / "drv"
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-DREFS_PACK_ONLY", "-I", CSRC, str(d / "drv.cpp"), "-o", str(exe)])
    calls = [0]

    def run(model, B, h1, cur, cur_pb, src, b0, nb, dst):
        """cur / dst: dicts name -> array (dst also 'rref' on whole-body phases); returns the packed dst."""
        calls[0] += 1
        w = d / f"call{calls[0]}"; w.mkdir()
        n, m, p = pkg._abi.MODEL_DIMS[model]
        first = cur_pb == 0
        p0, np_ = (0, B) if first else (b0, nb)
        (w / "meta.txt").write_text(" ".join(map(str, [n, m, p, int(model == pkg.MODEL_WB), B, h1, cur_pb, b0, nb, p0, np_] +
                                                   [int(src.get(k) is not None) for k in NAMES])))
        for s, k in enumerate(NAMES):
            cur[k].tofile(w / f"cur_{s}.bin")
            if src.get(k) is not None:
                src[k].tofile(w / f"src_{s}.bin")
        segs = list(NAMES) + ["rref"]
        for s, k in enumerate(segs):
            if k in dst:
                dst[k].tofile(w / f"dst_{s}.bin")
        subprocess.check_call([str(exe), str(w)])
        return {k: np.fromfile(w / f"dst_{s}.bin", dtype=dst[k].dtype).reshape(dst[k].shape) for s, k in enumerate(segs) if k in dst}
    return run


def pack_spec(model, B, h1, cur, cur_pb, src, b0, nb):
    """numpy statement of a hsddp_set_references call: every problem's raw rows afterwards, and the whole-body record built from them
    exactly as setup_phase builds the shared one (hs_host.hpp)."""
    w = pkg._abi.ref_widths(model)
    raw = {}
    for k in NAMES:
        if w[k] == 0:
            continue
        a = cur[k].reshape(-1, h1, w[k])
        raw[k] = np.repeat(a[:1], B, axis=0) if cur_pb == 0 else a.copy()
        if src.get(k) is not None:
            raw[k][b0:b0 + nb] = src[k].reshape(nb, h1, w[k])
    if model == pkg.MODEL_WB:
        rr = np.zeros((B, h1, 80))
        rr[..., 0:36] = raw["xr"]; rr[..., 36:48] = raw["ur"]; rr[..., 48:60] = raw["foot_vel"]
        rr[..., 60:64] = raw["ref_contact"].astype(np.float64)
        rr[..., 64:76] = raw["foot_pos"] - np.tile(raw["body_pos"], 4)
        raw["rref"] = rr
    return raw


@pytest.mark.parametrize("model", [0, 1, 2])
def test_pack_matches_numpy_statement(host_pack, model):
    rng = np.random.default_rng(11 + model)
    B, h1 = 5, 7
    w = pkg._abi.ref_widths(model)

    def rand(k, lead):
        if k == "ref_contact":
            return rng.integers(0, 2, (lead, h1, 4)).astype(np.int32)
        return rng.standard_normal((lead, h1, max(w[k], 1))) if w[k] or k != "yr" else np.zeros((lead, h1, 1))
    keys = [k for k in NAMES if w[k] > 0] + (["rref"] if model == pkg.MODEL_WB else [])
    shared = {k: rand(k, 1) for k in NAMES}
    # first call: all problems from the shared rows, [1, 4) from the sources (foot_vel kept)
    src = {k: (rand(k, 3) if k != "foot_vel" and w[k] > 0 else None) for k in NAMES}
    dst0 = {k: np.full((B, h1, w[k] if k != "rref" else 80), -7, dtype=np.int32 if k == "ref_contact" else np.float64) for k in keys}
    got = host_pack(model, B, h1, shared, 0, src, 1, 3, dst0)
    want = pack_spec(model, B, h1, shared, 0, src, 1, 3)
    for k in keys:
        assert got[k].tobytes() == want[k].tobytes(), ("first call", k)
    # later call in place: problems [3, 5) get new body_pos and ref_contact, everything else keeps its values
    cur = {k: (got[k] if k in got else shared[k]) for k in NAMES}
    src2 = {k: None for k in NAMES}; src2["body_pos"] = rand("body_pos", 2); src2["ref_contact"] = rand("ref_contact", 2)
    got2 = host_pack(model, B, h1, cur, h1, src2, 3, 2, {k: got[k].copy() for k in keys})
    want2 = pack_spec(model, B, h1, cur, h1, src2, 3, 2)
    for k in keys:
        assert got2[k].tobytes() == want2[k].tobytes(), ("later call", k)
    assert np.array_equal(got2["xr"][:3], got["xr"][:3])


# ------------------------------------------------------------------------------------------------ helpers
def test_stack_references_shapes_and_values():
    lists = [P.hkd_trot_problem(vx=v) for v in (0.0, 0.3, 0.6)]
    st = P.stack_references(lists)
    assert len(st) == len(lists[0])
    for i, r in enumerate(st):
        assert set(r) == {"xr", "ur", "foot_pos", "foot_vel", "body_pos", "ref_contact"}
        for k, v in r.items():
            assert v.shape == (3,) + lists[0][i]["bufs"][k].shape
            assert np.array_equal(v[2], lists[2][i]["bufs"][k])
    assert "yr" in P.stack_references([P.wb_trot_problem(vx=0.1), P.wb_trot_problem(vx=0.2)])[0]


def test_stack_references_refuses_mismatched_lists():
    base = P.wb_trot_problem(horizons=(10, 10, 10, 10))
    P.stack_references([base, P.wb_trot_problem(horizons=(10, 10, 10, 10), vx=0.1)])      # references only: fine
    bad = {
        "horizon": P.wb_trot_problem(horizons=(10, 10, 10, 11)),
        "dt": P.wb_trot_problem(horizons=(10, 10, 10, 10), dt=0.02),
        "contact": P.wb_trot_problem(schedule=((1, 1, 1, 1), (1, 0, 0, 1), (0, 1, 1, 0), (1, 0, 0, 1)), horizons=(10, 10, 10, 10)),
        "phase count": P.wb_trot_problem(schedule=((1, 1, 1, 1), (0, 1, 1, 0), (1, 0, 0, 1)), horizons=(10, 10, 10)),
        "model": P.mhpc_problem(wb_horizons=(10, 10), srb_horizons=(10, 10)),
    }
    w = P.wb_trot_problem(horizons=(10, 10, 10, 10)); w[2]["desc"].q[4] = 7.0
    bad["cost weight"] = w
    c = P.wb_trot_problem(horizons=(10, 10, 10, 10)); c[1]["desc"].c_torque = 0
    bad["constraint"] = c
    for name, pl in bad.items():
        with pytest.raises(ValueError):
            P.stack_references([base, pl])
        with pytest.raises(ValueError):
            P.stack_references([pl, base])


def _moved_mask(model, rc):
    """Entries translate_references moves: {name: (mask_x, mask_y)} for a phase of `model` with per-knot reference contacts rc."""
    h1 = rc.shape[0]
    n = pkg._abi.MODEL_DIMS[model][0]
    xm = np.zeros((h1, n), dtype=int)
    if model == pkg.MODEL_HKD:
        xm[:, 3] = 1; xm[:, 4] = 2
        for l in range(4):
            xm[rc[:, l] > 0, 12 + 3 * l] = 1; xm[rc[:, l] > 0, 13 + 3 * l] = 2
    else:
        xm[:, 0] = 1; xm[:, 1] = 2
    fm = np.tile(np.array([1, 2, 0] * 4), (h1, 1)); bm = np.tile(np.array([1, 2, 0]), (h1, 1))
    return {"xr": xm, "Xbar": xm, "foot_pos": fm, "body_pos": bm}


@pytest.mark.parametrize("which", ["wb", "mhpc", "hkd"])
def test_translate_references_moves_exactly_the_listed_entries(which):
    phases = {"wb": lambda: P.wb_trot_problem(horizons=(6, 6, 6, 6)), "mhpc": lambda: P.mhpc_problem(wb_horizons=(6, 6), srb_horizons=(3, 3)),
              "hkd": lambda: P.hkd_trot_problem(horizons=(4, 4, 4, 4))}[which]()
    dx, dy = 0.75, -2.5
    moved = P.translate_references(phases, dx, dy)
    for p, q in zip(phases, moved):
        model = p["desc"].model
        mask = _moved_mask(model, p["bufs"]["ref_contact"])
        for k in list(p["bufs"]) + ["Xbar"]:
            a = p["Xbar"] if k == "Xbar" else p["bufs"][k]
            b = q["Xbar"] if k == "Xbar" else q["bufs"][k]
            mk = mask.get(k, np.zeros(a.shape, dtype=int))
            want = a + np.where(mk == 1, dx, 0.0) + np.where(mk == 2, dy, 0.0) if a.dtype == np.float64 else a
            assert np.array_equal(b, want), (which, k)
            if k != "Xbar":      # the copy's descriptor points at the moved arrays; the original is untouched
                assert ctypes.addressof(getattr(q["desc"], k).contents) == b.ctypes.data
                assert ctypes.addressof(getattr(p["desc"], k).contents) == a.ctypes.data
        assert P._structure_bytes(p["desc"]) == P._structure_bytes(q["desc"])
    assert any((_moved_mask(p["desc"].model, p["bufs"]["ref_contact"])["xr"] > 0).any() for p in phases)


def test_multiphase_ddp_header_compiles_with_references(tmp_path):
    src = tmp_path / "w.cpp"
    src.write_text('#include "MultiPhaseDDP.hpp"\n'
                   'void f(hsddp::MultiPhaseDDP<double>& s, const double* xr) {\n'
                   '    hsddp_refs_t r{}; r.xr = xr; s.set_references(0, 1, 2, r); s.set_references(0, 0, 1, r, 1);\n'
                   '    std::vector<double> o(10); std::vector<int> c(4); s.get_references(0, 0, 1, o.data(), nullptr, nullptr, nullptr, nullptr, nullptr, c.data());\n'
                   '}\n')
    subprocess.check_call(["g++", "-std=c++17", "-c", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "cafe-mpc_amd", "host"),
                           str(src), "-o", str(tmp_path / "w.o")])
