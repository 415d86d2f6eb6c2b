"""MSD (gr_msd_*; groan_rs_amd.MSD): what can be checked without a device -- that the header's section is mirrored in _lib.py (parameter
counts), include/groan_hip.hpp and the Rust shim, the flags and stat keys, the export and its methods, and that the numpy restatement
the GPU tests compare with (tests/msd_ref.py) itself unwraps the walks it is fed and gives the MSD of a random walk.

THE BOUND of the unwrapped walk against the walk the generator cut the frames from, per atom: (1 + 2 c) ulp(L) + T ulp(0.25), with
ulp(L) the f32 spacing at the longest box edge, c the number of times the atom changed its image and T the number of frames.  The two
end frames are stored as f32 (half an ulp(L) each); a step without a crossing is a difference of neighbours |d| < 0.25 nm, rounded to
half an ulp(0.25) at most (up to four roundings in the triclinic reduction: 2 ulp(0.25) -- counted as T ulp(0.25) with the f64 chain's
own rounding, which is far below); a step with a crossing forms d = x - w of size L and reduces it through up to three more f32
roundings at that size: 2 ulp(L).  Measured on the inputs below: at most 4.7 ulp(L), 0.075 of the bound.

THE SAMPLING ERROR of the direct MSD against n_dims sigma^2 tau: the squared displacement of one atom and component over tau steps is
sigma^2 tau chi^2_1, variance 2 (sigma^2 tau)^2; the mean over S atoms, n_dims components and the T - tau overlapping windows has at
least S n_dims (T - tau) / tau independent terms, so its relative standard error is at most sqrt(2 tau / (S n_dims (T - tau))); the test
allows five of them (the steps are clipped at 4 sigma, which lowers the variance of a step by 0.1 %: inside the allowance)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

import msd_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["gr_msd_append_batch", "gr_msd_capacity", "gr_msd_clear", "gr_msd_compute", "gr_msd_create", "gr_msd_destroy", "gr_msd_frames", "gr_msd_n_atoms",
         "gr_msd_read", "gr_msd_read_displacements", "gr_msd_read_from_origin", "gr_msd_set_launch", "gr_msd_stat"]


def _header():
    txt = open(os.path.join(ROOT, "include", "groan_hip.h")).read()
    return re.sub(r"/\*.*?\*/", " ", txt, flags=re.S)


def _header_prototypes():
    return {m.group(1): [p for p in m.group(2).split(",") if p.strip()]
            for m in re.finditer(r"\b(gr_msd_[a-z_]+)\s*\(([^;{]*?)\)\s*;", _header(), flags=re.S)}


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
    assert _lib.SIGNATURES["gr_msd_create"][0] is C.c_void_p and _lib.SIGNATURES["gr_msd_destroy"][0] is None
    assert all(_lib.SIGNATURES["gr_msd_" + n][0] is C.c_uint64 for n in ("frames", "n_atoms", "capacity"))
    assert "class Msd" in hpp and "pub struct gr_msd" in rs
    # the header states the rule, the order of the sums, what msd[0] is, the ambiguity of long steps and what is not promised
    section = open(os.path.join(ROOT, "include", "groan_hip.h")).read().split("MSD: nojump unwrapping")[1].split("enum {")[0]
    flat = re.sub(r"\s*\n \*\s*", " ", section)
    for phrase in ("THE RULE", "ORDER OF THE SUMS", "D2(t, t) IS DEFINED AS 0", "ambiguous by nature", "NOT promised", "A FAILED FRAME STILL TAKES A TIME INDEX", "CLAMPED",
                   "GR_MSD_MAX_PANEL_BYTES"):
        assert phrase in flat, phrase
    src = open(os.path.join(ROOT, "groan_rs_amd", "csrc", "gr_msd.h")).read()
    assert "GR_MSD_MAX_PANEL_BYTES" in src and "ambiguous by nature" in src and "IS DEFINED AS 0" in src


def test_cpp_mirror_compiles_without_a_warning():
    """tests/cpp/msd_mirror.cpp calls every public method of groan::Msd"""
    src = os.path.join(ROOT, "tests", "cpp", "msd_mirror.cpp")
    hpp = open(os.path.join(ROOT, "include", "groan_hip.hpp")).read()
    cls = hpp.split("class Msd {")[1].split("  private:")[0]
    text = open(src).read()
    for name in ("append", "clear", "msd", "from_origin", "displacements", "set_launch", "stat", "raw_handle", "frames", "n_atoms", "capacity"):
        assert re.search(r"\b%s\(" % name, cls) and re.search(r"\.%s\(" % name, text), name
    p = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"), src], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    assert "detail::batch_status" in hpp.split("class Msd {")[1]                      # a refused call throws, like the other batch objects


def test_flags_stat_keys_and_cap_are_the_header_s():
    from groan_rs_amd import _lib
    enums = {m.group(1): int(m.group(2)) for m in re.finditer(r"\bGR_(MSD_STAT_[A-Z_]+)\s*=\s*(\d+)", _header())}
    assert sorted(enums) == ["MSD_STAT_BLOCK_EDGE", "MSD_STAT_COUNTED", "MSD_STAT_LAGS", "MSD_STAT_LAST_BLOCKS", "MSD_STAT_LAST_GRAM_GROUPS", "MSD_STAT_LAST_WALK_GROUPS",
                             "MSD_STAT_LAUNCHES", "MSD_STAT_N_PAD", "MSD_STAT_TRIP_VALUES"]
    assert sorted(enums.values()) == list(range(1, 10))
    for name, v in enums.items():
        assert getattr(_lib, name) == v, name
    defs = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define\s+GR_(MSD_[A-Z_]+)\s+(\d+)u?\b", _header())}
    assert defs == {"MSD_X": _lib.MSD_X, "MSD_Y": _lib.MSD_Y, "MSD_Z": _lib.MSD_Z, "MSD_NOJUMP": _lib.MSD_NOJUMP, "MSD_MAX_PANEL_BYTES": _lib.MSD_MAX_PANEL_BYTES}
    assert (defs["MSD_X"], defs["MSD_Y"], defs["MSD_Z"], defs["MSD_NOJUMP"]) == (1, 2, 4, 8)
    rs = open(os.path.join(ROOT, "rust", "src", "groan_hip.rs")).read()
    assert "GR_MSD_NOJUMP" in rs


def test_msd_is_exported():
    import groan_rs_amd as G
    from groan_rs_amd import msd
    assert G.MSD is msd.MSD and "MSD" in G.__all__
    for method in ("append", "msd", "from_origin", "displacements", "clear", "close", "set_launch", "stat", "__enter__", "__exit__"):
        assert callable(getattr(G.MSD, method)), method
    assert isinstance(G.MSD.n_frames, property)
    import inspect
    assert list(inspect.signature(G.MSD.__init__).parameters)[1:] == ["system", "group", "capacity", "dims", "nojump"]
    assert inspect.signature(G.MSD.__init__).parameters["dims"].default == "xyz" and inspect.signature(G.MSD.__init__).parameters["nojump"].default is True


def test_fma32_is_the_fused_operation():
    """against exact rational arithmetic, on likely and on unlikely inputs (a tiny addend beside a product of order 1)"""
    from fractions import Fraction
    rng = np.random.default_rng(5)
    k = rng.integers(-3, 4, 4000).astype(R.F)
    L = (rng.random(4000) * 4 + 0.5).astype(R.F)
    d = np.concatenate([(rng.standard_normal(2000) * 2).astype(R.F), (rng.standard_normal(2000) * 2.0 ** rng.integers(-60, -20, 2000)).astype(R.F)])
    got = R.fma32(k, L, d)

    def exact(a, b, c):
        x = Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c))
        lo = np.float32(float(x))                                   # (float(Fraction) rounds once to f64; decide by comparing neighbours exactly)
        cands = [lo, np.nextafter(lo, np.float32(np.inf)), np.nextafter(lo, np.float32(-np.inf))]
        best = min(cands, key=lambda v: (abs(Fraction(float(v)) - x), int(np.float32(v).view(np.uint32)) & 1))
        return best
    want = np.array([exact(a, b, c) for a, b, c in zip(k, L, d)], R.F)
    assert R.same_bits(got + R.F(0), want + R.F(0))                  # (+0: -0.0 and 0.0 are the same result)


def _inputs():
    for cell in sorted(R.CELLS):
        yield cell, R.walk(200, 240, 20261022 + len(cell), cell)


def test_inputs_stay_clear_of_half_a_box_edge_and_of_ties():
    for cell, (frames, boxes, U, crossings) in _inputs():
        worst, tie = 0.0, 1.0
        for t in range(1, len(frames)):
            seen = []
            d = R.reduce_step(frames[t] - frames[t - 1], boxes[t], seen)
            edges = np.asarray(boxes[t], R.F)[:3]
            worst = max(worst, float((np.abs(d) / edges).max()))
            raw = np.stack(seen)                                     # what rint was given along c, b and a: a tie is a fraction of exactly 0.5
            tie = min(tie, float(np.abs(np.abs(raw - np.rint(raw)) - 0.5).min()))
        print("%s: largest |d| / edge %.3f, nearest to a tie of rint %.3f, crossings per atom up to %d" % (cell, worst, tie, crossings.max()))
        assert worst < 0.15 and tie > 0.3 and crossings.max() >= 3
        assert min(np.asarray(b)[:3].min() for b in boxes) >= 2.9


def test_restatement_unwraps_the_walk_it_is_fed():
    for cell, (frames, boxes, U, crossings) in _inputs():
        idx = np.arange(3, 190)
        w = R.Walk(len(idx))
        st, bad = w.append(frames, boxes, idx)
        assert not st.any() and len(w.us) == len(frames)
        err = np.abs(np.stack(w.us) - U[:, idx]).max(axis=(0, 2))
        ulp_l = float(np.spacing(R.F(max(np.asarray(b)[:3].max() for b in boxes))))
        bound = (1 + 2 * crossings[idx]) * ulp_l + len(frames) * float(np.spacing(R.F(0.25)))
        print("%s: unwrapped walk within %.2f ulp(L) of the generator's, %.3f of the bound at worst" % (cell, err.max() / ulp_l, (err / bound).max()))
        assert (err <= bound).all()
        # the panel is the unwrapped displacement from the first frame, rounded to f32; without nojump it is the wrapped one
        assert np.abs(w.panel() - (U[:, idx] - U[0, idx])).max() <= bound.max() + 2.0 ** -24 * np.abs(U[:, idx] - U[0, idx]).max()
        raw = R.Walk(len(idx), nojump=False)
        raw.append(frames, boxes, idx)
        assert R.same_bits(raw.panel()[5], (frames[5][idx].astype(R.D) - frames[0][idx].astype(R.D)).astype(R.F))
        assert crossings[idx].max() >= 3 and np.abs(raw.panel() - w.panel()).max() > 2.9      # (atoms did cross the cell: there a whole box vector lies between the two)
        if cell == "rescaled":
            assert len({np.asarray(b).tobytes() for b in boxes}) == len(boxes)


def test_direct_msd_is_the_random_walk_s():
    frames, boxes, U, crossings = R.walk(300, 400, 99, "tric")
    idx = np.arange(300)
    for dims in ("xyz", "xy", "z"):
        w = R.Walk(300, dims=dims)
        w.append(frames, boxes, idx)
        msd, pairs, qsum = R.direct_msd(w.panel(), w.ok, max_lag=100)
        nd, T = len(dims), len(frames)
        assert msd[0] == 0.0 and pairs.tolist() == [T - tau for tau in range(101)]
        tau = np.arange(1, 101)
        rel = np.abs(msd[1:] / (nd * R.SIGMA ** 2 * tau) - 1.0)
        allow = 5.0 * np.sqrt(2.0 * tau / (300 * nd * (T - tau)))
        print("dims %s: direct MSD within %.2f of the allowance (5 standard errors) at worst" % (dims, (rel / allow).max()))
        assert (rel <= allow).all()
    # long double and double agree far below the device's bound
    w = R.Walk(300); w.append(frames[:40], boxes[:40], idx)
    a, b = R.direct_msd(w.panel(), w.ok)[0], R.direct_msd(w.panel(), w.ok, dtype=np.longdouble)[0]
    assert np.abs(a - b).max() <= 1e-15


def test_restatement_of_failed_frames():
    frames, boxes, U, crossings = R.walk(40, 12, 3, "ortho")
    frames = [x.copy() for x in frames]
    boxes = list(boxes)
    frames[0][5, :] = np.nan; frames[4][[9, 7], :] = np.nan; frames[6][1, :] = np.nan; boxes[8] = None
    idx = np.arange(3, 40)
    w = R.Walk(len(idx))
    st, bad = w.append(frames, boxes, idx)
    assert st.tolist() == [R.E_NO_POSITION, 0, 0, 0, R.E_NO_POSITION, 0, 0, 0, R.E_NO_BOX, 0, 0, 0] and bad[0] == 5 and bad[4] == 7 and bad[6] == -1
    assert R.same_bits(w.o, frames[1][idx]) and not w.panel()[[0, 1, 4, 8]].any() and w.panel()[2].any()
    # the walk continues across the gap: the same as the walk over the good frames alone
    good = [k for k in range(12) if k not in (0, 4, 8)]
    v = R.Walk(len(idx))
    v.append([frames[k] for k in good], [boxes[k] for k in good], idx)
    assert R.same_bits(w.panel()[good], v.panel())
    msd, pairs, qsum = R.direct_msd(w.panel(), w.ok)
    ok = np.array(w.ok)
    assert pairs.tolist() == [int((ok[:12 - t] & ok[t:]).sum()) for t in range(12)] and pairs[0] == 9 and pairs[11] == 0 and np.isnan(msd[11])
    free = R.Walk(len(idx), nojump=False)                            # without nojump a frame needs no box
    assert free.append(frames, boxes, idx)[0].tolist() == [R.E_NO_POSITION, 0, 0, 0, R.E_NO_POSITION, 0, 0, 0, 0, 0, 0, 0]
