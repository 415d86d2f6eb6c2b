"""Fluctuations (gr_fluct_*; groan_rs_amd.Fluctuations): what can be checked without a device -- that the header's section is mirrored
in _lib.py (parameter counts), include/groan_hip.hpp and the Rust shim, the export and its methods, the look-ahead constant the edge
tests are written around, and that the numpy restatement the GPU tests compare bits with (tests/fluct_ref.py) itself agrees with an
independent two-pass reference on the GPU tests' inputs."""
import ctypes as C
import os
import re

import numpy as np

import fluct_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["gr_fluct_accumulate_batch", "gr_fluct_clear", "gr_fluct_create", "gr_fluct_destroy", "gr_fluct_frames", "gr_fluct_merge", "gr_fluct_n_atoms",
         "gr_fluct_read", "gr_fluct_read_raw", "gr_fluct_set_launch", "gr_fluct_stat", "gr_fluct_store_mean"]


def _header():
    txt = open(os.path.join(ROOT, "include", "groan_hip.h")).read()
    return re.sub(r"/\*.*?\*/", " ", txt, flags=re.S)


def _header_prototypes():
    return {m.group(1): [p for p in m.group(2).split(",") if p.strip()]
            for m in re.finditer(r"\b(gr_fluct_[a-z_]+)\s*\(([^;{]*?)\)\s*;", _header(), flags=re.S)}


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
    assert _lib.SIGNATURES["gr_fluct_create"][0] is C.c_void_p and _lib.SIGNATURES["gr_fluct_destroy"][0] is None
    assert _lib.SIGNATURES["gr_fluct_frames"][0] is C.c_uint64 and _lib.SIGNATURES["gr_fluct_n_atoms"][0] is C.c_uint64
    assert "class Fluctuations" in hpp and "pub struct gr_fluct" in rs
    # the header says what a merge does to the order of the sums
    section = open(os.path.join(ROOT, "include", "groan_hip.h")).read().split("Fluctuations: mean structure")[1].split("enum {")[0]
    assert "NO LONGER THOSE OF A SEQUENTIAL WALK" in section


def test_stat_keys_are_the_header_s():
    from groan_rs_amd import _lib
    enums = {m.group(1): int(m.group(2)) for m in re.finditer(r"\bGR_(FL_STAT_[A-Z_]+)\s*=\s*(\d+)", _header())}
    assert sorted(enums) == ["FL_STAT_AHEAD", "FL_STAT_FORM", "FL_STAT_LAST_CHECK_GROUPS", "FL_STAT_LAST_RANGE_GROUPS", "FL_STAT_LAUNCHES"]
    for name, v in enums.items():
        assert getattr(_lib, name) == v, name


def test_fluctuations_is_exported():
    import groan_rs_amd as G
    from groan_rs_amd import fluct
    assert G.Fluctuations is fluct.Fluctuations and "Fluctuations" in G.__all__
    for method in ("accumulate", "mean", "variance", "rmsf", "raw", "merge", "store_mean", "clear", "set_launch", "stat", "close", "__enter__", "__exit__"):
        assert callable(getattr(G.Fluctuations, method)), method
    assert isinstance(G.Fluctuations.n_frames, property)


def test_look_ahead_is_read_from_the_source():
    """the edge tests place their frame counts and failing frames around GR_FL_AHEAD: it must be there to be read, and a real look-ahead"""
    ahead = R.source_ahead()
    assert 3 <= ahead <= 64
    src = open(os.path.join(ROOT, "groan_rs_amd", "csrc", "gr_fluct.h")).read()
    assert re.search(r"ring\[GR_FL_AHEAD\]", src)


def _worst(state, frames, idx):
    mean, var, rmsf = state.close()
    m2, v2, r2 = R.two_pass(frames, idx)
    return max(np.abs(mean - m2).max(), np.abs(rmsf - r2).max())


def test_restatement_agrees_with_the_two_pass_reference():
    """on the inputs of the GPU tests (tests/test_gpu_fluct.py): fitted frames, frames jumping across the box, rigid copies; <= 1e-6 nm"""
    n = 1000
    idx = np.arange(n)
    for frames in (R.fitted_frames(n, 37, 20261020), R.jumping_frames(n, 37, 7), R.fitted_frames(700, 1100, 3)):
        st = R.State(len(frames[0]))
        ix = idx[:len(frames[0])]
        status, bad = st.accumulate(frames, ix)
        assert not status.any() and st.n == len(frames)
        assert _worst(st, frames, ix) <= 1e-6
    rigid = [R.fitted_frames(n, 1, 5)[0]] * 9
    st = R.State(n)
    st.accumulate(rigid, idx)
    mean, var, rmsf = st.close()
    assert np.array_equal(mean, rigid[0].astype(np.float64)) and not rmsf.any() and not st.s.any() and not st.q.any()


def test_restatement_of_failed_frames_and_merge():
    n = 64
    frames = R.fitted_frames(n, 9, 11)
    frames[0][5, 0] = np.nan; frames[4][[9, 7], 0] = np.nan
    idx = np.arange(3, 40)
    st = R.State(len(idx))
    status, bad = st.accumulate(frames, idx)
    assert status.tolist() == [R.E_NO_POSITION, 0, 0, 0, R.E_NO_POSITION, 0, 0, 0, 0] and bad[0] == 5 and bad[4] == 7 and st.n == 7
    assert np.array_equal(st.o, frames[1][idx])                                  # the origin: the first COUNTED frame
    a, b = R.State(len(idx)), R.State(len(idx))
    a.accumulate(frames[:4], idx); b.accumulate(frames[4:], idx)
    a.merge(b)
    assert a.n == 7
    for x, y in zip(a.close(), st.close()):                                      # (two origins: the f32 subtractions round differently, each within
        assert np.abs(x - y).max() <= 1e-6                                       #  the restatement's own 1e-6 of the two-pass reference)
    e = R.State(len(idx)); e.merge(st)
    assert R.same_bits(e.s, st.s) and R.same_bits(e.q, st.q) and R.same_bits(e.o, st.o) and e.n == 7
    st.merge(R.State(len(idx)))
    assert R.same_bits(e.s, st.s) and st.n == 7
    empty = R.State(4)
    assert all(np.isnan(x).all() for x in empty.close())
