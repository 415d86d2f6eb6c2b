"""VectorCorrelation (gr_vcorr_*; groan_rs_amd.VectorCorrelation): what can be checked without a device -- that the header's section is
mirrored in _lib.py (parameter counts), include/groan_hip.hpp and the Rust shim, the flags, stat keys and caps, the export and its
methods, and that the numpy restatement the GPU tests compare with (tests/vcorr_ref.py) itself gives the analytic curves of a rigid rotor.

THE BOUND of the rotor's curves (vcorr_ref.unit_error, vcorr_ref.curve_bounds).  The generator's coordinates are f64, stored as f32:
each stored coordinate is within ulp32(X) / 2 of the exact one (X the largest coordinate), so a component of d = x_j - x_i, whose f32
subtraction rounds by ulp32(b) / 2 at most (b the bond), is within ulp32(X) + ulp32(b) / 2 of the exact one and |delta d| within
sqrt(3) of that.  Normalising moves the unit vector by at most 2 |delta d| / b, the rule's own roundings add less than 4 * 2^-24:
eps = 2 sqrt(3) (ulp32(X) + ulp32(b) / 2) / b + 4 * 2^-24.  Then |delta (u . u')| <= 2 eps + eps^2 = e bounds C1, and
1.5 (2 + e) e + 8 * 2^-24 bounds C2 (the rank-2 entries are f32 products, scaled by an f32 sqrt 2).  With X = 3 nm and b = 0.1 nm:
eps = 8.6e-6.  Measured share of the bound: 0.011 (C1), 0.007 (C2) (the coordinate errors are of random sign and average over the vectors)."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np

import vcorr_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["gr_vcorr_append_batch", "gr_vcorr_capacity", "gr_vcorr_clear", "gr_vcorr_compute", "gr_vcorr_compute_each", "gr_vcorr_count", "gr_vcorr_create",
         "gr_vcorr_destroy", "gr_vcorr_frames", "gr_vcorr_read", "gr_vcorr_read_vectors", "gr_vcorr_set_launch", "gr_vcorr_stat"]


def _header():
    txt = open(os.path.join(ROOT, "include", "groan_hip.h")).read()
    return re.sub(r"/\*.*?\*/", " ", txt, flags=re.S)


def _header_prototypes():
    return {m.group(1): [p for p in m.group(2).split(",") if p.strip()]
            for m in re.finditer(r"\b(gr_vcorr_[a-z_]+)\s*\(([^;{]*?)\)\s*;", _header(), flags=re.S)}


def test_header_section_is_mirrored_in_lib_hpp_and_rust():
    from groan_rs_amd import _lib
    protos = _header_prototypes()
    assert sorted(protos) == NAMES
    hpp = open(os.path.join(ROOT, "include", "groan_hip.hpp")).read()
    rs = re.sub(r"//[^\n]*", " ", open(os.path.join(ROOT, "rust", "src", "groan_hip.rs")).read())
    for name, params in protos.items():
        assert name in _lib.SIGNATURES, name
        assert len(_lib.SIGNATURES[name][1]) == len(params), (name, len(_lib.SIGNATURES[name][1]), len(params))
        assert re.search(r"\b%s\s*\(" % name, hpp), name
        m = re.search(r"pub\s+fn\s+%s\s*\((.*?)\)\s*(?:->[^;]*)?;" % name, rs, flags=re.S)
        assert m, name
        assert len([p for p in m.group(1).split(",") if ":" in p]) == len(params), name
    assert _lib.SIGNATURES["gr_vcorr_create"][0] is C.c_void_p and _lib.SIGNATURES["gr_vcorr_destroy"][0] is None
    assert all(_lib.SIGNATURES["gr_vcorr_" + n][0] is C.c_uint64 for n in ("frames", "count", "capacity"))
    assert len(protos["gr_vcorr_create"]) == 6 and len(protos["gr_vcorr_set_launch"]) == 4 and len(protos["gr_vcorr_read"]) == 4
    assert "class VectorCorrelation {" in hpp and "pub struct gr_vcorr" in rs
    # the header states the rule, the order of the sums and what is not promised; the kernel header states the rule and the caps
    section = open(os.path.join(ROOT, "include", "groan_hip.h")).read().split("VectorCorrelation: P1/P2 reorientation curves")[1].split("#define")[0]
    flat = re.sub(r"\s*\n \*\s*", " ", section)
    for phrase in ("THE RULE", "ORDER OF THE SUMS", "STILL COUNTS IN THE DENOMINATOR", "NOT promised", "A FAILED FRAME STILL TAKES A TIME INDEX", "CLAMPED",
                   "GR_MSD_MAX_PANEL_BYTES", "GR_VCORR_MAX_EACH_BYTES", "Out of scope"):
        assert phrase in flat, phrase
    src = open(os.path.join(ROOT, "groan_rs_amd", "csrc", "gr_vcorr.h")).read()
    for phrase in ("THE RULE", "STILL", "GR_MSD_MAX_PANEL_BYTES", "GR_VCORR_MAX_EACH_BYTES", "k_band_lags", "k_band_gram", "k_vc_walk", "k_vc_each"):
        assert phrase in src, phrase
    api = open(os.path.join(ROOT, "groan_rs_amd", "csrc", "gr_api.hip")).read()
    assert api.index('#include "gr_internals.h"') < api.index('#include "gr_vcorr.h"')


def test_cpp_mirror_compiles_without_a_warning():
    """tests/cpp/vcorr_mirror.cpp calls every public method of groan::VectorCorrelation"""
    src = os.path.join(ROOT, "tests", "cpp", "vcorr_mirror.cpp")
    hpp = open(os.path.join(ROOT, "include", "groan_hip.hpp")).read()
    cls = hpp.split("class VectorCorrelation {")[1].split("  private:")[0]
    text = open(src).read()
    for name in ("append", "clear", "correlate", "correlate_each", "vectors", "set_launch", "stat", "raw_handle", "frames", "count", "capacity"):
        assert re.search(r"\b%s\(" % name, cls) and re.search(r"\.%s\(" % name, text), name
    p = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"), src], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    assert "detail::batch_status" in hpp.split("class VectorCorrelation {")[1]         # a refused call throws, like the other batch objects


def test_flags_stat_keys_and_caps_are_the_header_s():
    from groan_rs_amd import _lib
    enums = {m.group(1): int(m.group(2)) for m in re.finditer(r"\bGR_(VCORR_STAT_[A-Z_]+)\s*=\s*(\d+)", _header())}
    assert sorted(enums) == ["VCORR_STAT_COUNTED", "VCORR_STAT_LAGS", "VCORR_STAT_LAST_BLOCKS", "VCORR_STAT_LAST_EACH_GROUPS", "VCORR_STAT_LAST_GRAM_GROUPS",
                             "VCORR_STAT_LAST_WALK_GROUPS", "VCORR_STAT_LAUNCHES", "VCORR_STAT_N_PAD"]
    assert sorted(enums.values()) == list(range(1, 9))
    rs = open(os.path.join(ROOT, "rust", "src", "groan_hip.rs")).read()
    for name, v in enums.items():
        assert getattr(_lib, name) == v, name
        assert re.search(r"pub const GR_%s: c_int = %d;" % (name, v), rs), name
    defs = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define\s+GR_(VCORR_[A-Z_0-9]+)\s+(\d+)u?\b", _header())}
    assert defs == {"VCORR_PBC": _lib.VCORR_PBC, "VCORR_UNIT": _lib.VCORR_UNIT, "VCORR_P1": _lib.VCORR_P1, "VCORR_P2": _lib.VCORR_P2,
                    "VCORR_MAX_EACH_BYTES": _lib.VCORR_MAX_EACH_BYTES}
    assert (defs["VCORR_PBC"], defs["VCORR_UNIT"], defs["VCORR_P1"], defs["VCORR_P2"], defs["VCORR_MAX_EACH_BYTES"]) == (1, 2, 4, 8, 2 ** 30)
    for name, v in defs.items():
        assert re.search(r"pub const GR_%s: u(32|64) = %d;" % (name, v), rs), name


def test_vector_correlation_is_exported():
    import groan_rs_amd as G
    from groan_rs_amd import vcorr
    assert G.VectorCorrelation is vcorr.VectorCorrelation and "VectorCorrelation" in G.__all__
    for method in ("append", "clear", "correlate", "correlate_each", "vectors", "set_launch", "stat", "close", "__enter__", "__exit__"):
        assert callable(getattr(G.VectorCorrelation, method)), method
    assert isinstance(G.VectorCorrelation.n_frames, property)
    sig = inspect.signature(G.VectorCorrelation.__init__).parameters
    assert list(sig)[1:] == ["system", "pairs", "capacity", "rank", "pbc", "unit"]
    assert sig["rank"].default == (1, 2) and sig["pbc"].default is False and sig["unit"].default is True
    assert "_plans.append(self)" in inspect.getsource(vcorr.VectorCorrelation.__init__)


def test_panel_rule_of_the_restatement():
    pos = np.array([[0, 0, 0], [3, 4, 0], [1, 1, 1], [1, 1, 1], [0.1, 0.2, 0.3]], R.F)
    u = R.vectors32(pos, [[0, 1], [2, 3], [1, 4]])
    assert u.dtype == R.F and u[0].tolist() == [R.F(3) * (R.F(1) / R.F(5)), R.F(4) * (R.F(1) / R.F(5)), 0.0]
    assert u[1].tolist() == [0.0, 0.0, 0.0]                           # a vector of length zero: u = 0, no NaN
    assert R.same_bits(R.vectors32(pos, [[0, 1]], unit=False), np.array([[3, 4, 0]], R.F))
    e = R.rank2(u)
    assert e.shape == (3, 6) and R.same_bits(e[:, 3], R.SQRT2_F * (u[:, 0] * u[:, 1])) and R.same_bits(e[:, 1], u[:, 1] * u[:, 1])
    # the rank-2 product is the square of the rank-1 product, up to the f32 rounding of the entries
    rng = np.random.default_rng(1)
    p = rng.standard_normal((400, 3)).astype(R.F)
    w = R.vectors32(p, np.arange(400).reshape(-1, 2))
    a, b = w[:100].astype(np.float64), w[100:].astype(np.float64)
    ea, eb = R.rank2(w[:100]).astype(np.float64), R.rank2(w[100:]).astype(np.float64)
    assert np.abs((ea * eb).sum(1) - (a * b).sum(1) ** 2).max() <= 8 * R.EPS32
    # failed frames: a named atom without position (the lowest), an atom no pair names, with pbc a frame without a box first
    frames = [pos.copy() for _ in range(4)]
    frames[1][4] = np.nan; frames[1][2] = np.nan; frames[2][0, 1] = np.nan
    q = R.Panels([[1, 4], [2, 3]])
    st, bad = q.append(frames)
    assert st.tolist() == [0, R.E_NO_POSITION, 0, 0] and bad.tolist() == [-1, 2, -1, -1] and q.ok == [True, False, True, True] and not q.x1()[1].any()
    qb = R.Panels([[1, 4], [2, 3]], pbc=True)
    assert qb.append(frames, [None, None, [3.0] * 3 + [0.0] * 6, [3.0] * 3 + [0.0] * 6])[0].tolist() == [R.E_NO_BOX, R.E_NO_BOX, 0, 0]
    assert R.pair_counts(q.ok).tolist() == [3, 1, 1, 1] and R.pair_counts(q.ok, 1).tolist() == [3, 1]


def test_restatement_gives_the_rigid_rotor_s_curves():
    worst = [0.0, 0.0]
    for theta, omega, seed in ((0.6, 0.11, 1), (np.pi / 2, 0.05, 2), (1.2, 0.4, 3)):
        V, T = 40, 90
        frames, pairs = R.rotor(V, T, theta, omega, seed)
        q = R.Panels(pairs)
        st, bad = q.append(frames)
        assert not st.any()
        den = R.pair_counts(q.ok).astype(np.float64) * V
        c1 = R.close(np.asarray(R.direct(q.x1(), q.ok)[0], np.float64), den, 1)
        c2 = R.close(np.asarray(R.direct(q.x2(), q.ok)[0], np.float64), den, 2)
        w1, w2 = R.rotor_curves(theta, omega, T)
        b1, b2 = R.curve_bounds(R.unit_error(max(float(np.abs(x).max()) for x in frames), 0.1))
        s1, s2 = np.abs(c1 - w1).max() / b1, np.abs(c2 - w2).max() / b2
        worst = [max(worst[0], s1), max(worst[1], s2)]
        assert s1 <= 1.0 and s2 <= 1.0, (theta, omega, s1, s2)
        # every vector on its own follows the same curve: the chains, closed per vector
        e1, e2 = R.each(q.x1(), q.ok, 1), R.each(q.x2(), q.ok, 2)
        assert e1.shape == (V, T) and np.abs(e1 - w1).max() <= b1 and np.abs(e2 - w2).max() <= b2
    print("rotor: C1 within %.3f of its bound, C2 within %.3f" % tuple(worst))


def test_mean_of_the_per_vector_curves_is_the_all_vector_curve():
    """the two closings differ by the order of f64 sums only: (T V C + 2) 2^-53 of the sum of the |products| per lag and pair count"""
    frames, boxes, pairs, straddle = R.bonded_world(37, 70, 5, "ortho")
    frames = [x.copy() for x in frames]
    frames[9][4] = np.nan
    q = R.Panels(pairs)
    st, bad = q.append(frames)
    assert st[9] == R.E_NO_POSITION and bad[9] == 4 and st.sum() == R.E_NO_POSITION
    V, T = 37, 70
    cnt = R.pair_counts(q.ok)
    assert cnt[0] == T - 1 and cnt[T - 1] == 1
    for rank, panel in ((1, q.x1()), (2, q.x2())):
        S, A = R.direct(panel, q.ok)
        want = R.close(np.asarray(S, np.float64), cnt.astype(np.float64) * V, rank)
        got = R.each(panel, q.ok, rank).mean(0)
        C = panel.shape[2]
        bound = (T * V * C + 2) * 2.0 ** -53 * np.asarray(A, np.float64) / (cnt * V) * (1.5 if rank == 2 else 1.0) + 8 * 2.0 ** -53
        assert (np.abs(got - want) <= bound).all(), (np.abs(got - want) / bound).max()
    # lag 0 of unit vectors is 1 within the normalisation's rounding
    assert np.abs(R.each(q.x1(), q.ok, 1)[:, 0] - 1.0).max() <= 8 * R.EPS32 and np.abs(R.each(q.x2(), q.ok, 2)[:, 0] - 1.0).max() <= 16 * R.EPS32
    # a shorter band is a prefix
    assert R.same_bits(R.each(q.x2(), q.ok, 2, 12), R.each(q.x2(), q.ok, 2)[:, :13])
