"""Covariance (gr_covar_*; groan_rs_amd.Covariance): what can be checked without a device -- that the header's section is mirrored in
_lib.py (parameter counts), include/groan_hip.hpp and the Rust shim, the stat keys, the export and its methods, and that the numpy
restatement the GPU tests compare with (tests/covar_ref.py) itself agrees with an independent two-pass reference on the GPU tests'
inputs.

The bound of that agreement, per entry: 2^-22 sd_i sd_j.  The restatement differs from the two-pass covariance through the rounding of
the f32 subtraction d = x - o (relative 2^-24 of |d|, |d| a few sd): measured on the inputs below at most 5.8e-8 sd_i sd_j = 0.24 of the bound."""
import ctypes as C
import os
import re

import numpy as np

import covar_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["gr_covar_accumulate_batch", "gr_covar_clear", "gr_covar_create", "gr_covar_destroy", "gr_covar_frames", "gr_covar_merge", "gr_covar_n_atoms",
         "gr_covar_read", "gr_covar_read_dccm", "gr_covar_read_raw", "gr_covar_set_launch", "gr_covar_stat"]
REL = 2.0 ** -22


def _header():
    txt = open(os.path.join(ROOT, "include", "groan_hip.h")).read()
    return re.sub(r"/\*.*?\*/", " ", txt, flags=re.S)


def _header_prototypes():
    return {m.group(1): [p for p in m.group(2).split(",") if p.strip()]
            for m in re.finditer(r"\b(gr_covar_[a-z_]+)\s*\(([^;{]*?)\)\s*;", _header(), flags=re.S)}


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
    assert _lib.SIGNATURES["gr_covar_create"][0] is C.c_void_p and _lib.SIGNATURES["gr_covar_destroy"][0] is None
    assert _lib.SIGNATURES["gr_covar_frames"][0] is C.c_uint64 and _lib.SIGNATURES["gr_covar_n_atoms"][0] is C.c_uint64
    assert "class Covariance" in hpp and "pub struct gr_covar" in rs
    # the header says what a merge does to the order of the sums, and what is not promised across cuts
    section = open(os.path.join(ROOT, "include", "groan_hip.h")).read().split("Covariance: positional covariance")[1].split("enum {")[0]
    assert "NO LONGER THOSE OF ONE WALK" in re.sub(r"\s*\n \*\s*", " ", section)
    assert "NOT guaranteed" in section and "GR_CV_MAX_ATOMS" in section


def test_stat_keys_flags_and_cap_are_the_header_s():
    from groan_rs_amd import _lib
    enums = {m.group(1): int(m.group(2)) for m in re.finditer(r"\bGR_(CV_STAT_[A-Z_]+)\s*=\s*(\d+)", _header())}
    assert sorted(enums) == ["CV_STAT_BLOCKS", "CV_STAT_BLOCK_EDGE", "CV_STAT_LAST_CHECK_GROUPS", "CV_STAT_LAST_PRODUCT_GROUPS", "CV_STAT_LAUNCHES", "CV_STAT_TRIP_FRAMES"]
    for name, v in enums.items():
        assert getattr(_lib, name) == v, name
    defs = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define\s+GR_(CV_[A-Z_]+)\s+(\d+)u?\b", _header())}
    assert defs == {"CV_MAX_ATOMS": _lib.CV_MAX_ATOMS, "CV_MASS_WEIGHTED": _lib.CV_MASS_WEIGHTED}


def test_covariance_is_exported():
    import groan_rs_amd as G
    from groan_rs_amd import covar
    assert G.Covariance is covar.Covariance and "Covariance" in G.__all__
    for method in ("accumulate", "clear", "merge", "mean", "matrix", "dccm", "raw", "set_launch", "stat", "close", "__enter__", "__exit__"):
        assert callable(getattr(G.Covariance, method)), method
    assert isinstance(G.Covariance.n_frames, property)


def _inputs():
    yield R.fitted_frames(1000, 37, 20261020), np.arange(3, 104)
    yield R.jumping_frames(1000, 37, 7), np.arange(0, 1000, 9)
    yield R.fitted_frames(700, 1100, 3), np.arange(40)
    yield R.fitted_frames(40, 1030, 5), np.arange(40)


def _worst(cov, frames, idx):
    m2, c2, sd = R.two_pass(frames, idx)
    return (np.abs(cov - c2) / np.outer(sd, sd)).max()


def test_restatement_agrees_with_the_two_pass_reference():
    """on the inputs of the GPU tests: fitted frames, frames jumping across the box, long runs; per entry within 2^-22 sd_i sd_j"""
    for frames, idx in _inputs():
        st = R.State(len(idx))
        status, bad = st.accumulate(frames, idx)
        assert not status.any() and st.n == len(frames)
        mean, cov = R.close(st.o, st.s, st.Q, st.n)
        worst = _worst(cov, frames, idx)
        print("restatement vs two-pass: %.3g of sd_i sd_j (bound %.3g)" % (worst, REL))
        assert worst <= REL
        assert np.abs(mean - R.two_pass(frames, idx)[0]).max() <= 1e-6
        assert np.array_equal(st.Q, st.Q.T)


def test_restatement_of_failed_frames_and_merge():
    frames = R.fitted_frames(64, 9, 11)
    frames[0][5, 0] = np.nan; frames[4][[9, 7], 0] = np.nan
    idx = np.arange(3, 40)
    st = R.State(len(idx))
    status, bad = st.accumulate(frames, idx)
    assert status.tolist() == [R.E_NO_POSITION, 0, 0, 0, R.E_NO_POSITION, 0, 0, 0, 0] and bad[0] == 5 and bad[4] == 7 and st.n == 7
    assert np.array_equal(st.o, frames[1][idx].reshape(-1))                      # the origin: the first COUNTED frame
    a, b = R.State(len(idx)), R.State(len(idx))
    a.accumulate(frames[:4], idx); b.accumulate(frames[4:], idx)
    a.merge(b)
    assert a.n == 7
    # two origins: the f32 subtractions round differently, each within the bound of the two-pass reference; the merge agrees with one walk within it
    clean = [x for k, x in enumerate(frames) if k not in (0, 4)]
    m2, c2, sd = R.two_pass(clean, idx)
    for s in (a, st):
        mean, cov = R.close(s.o, s.s, s.Q, s.n)
        assert (np.abs(cov - c2) / np.outer(sd, sd)).max() <= REL and np.abs(mean - m2).max() <= 1e-6
    ca, cs = R.close(a.o, a.s, a.Q, a.n)[1], R.close(st.o, st.s, st.Q, st.n)[1]
    assert (np.abs(ca - cs) / np.outer(sd, sd)).max() <= REL
    e = R.State(len(idx)); e.merge(st)
    assert R.same_bits(e.s, st.s) and R.same_bits(e.Q, st.Q) and R.same_bits(e.o, st.o) and e.n == 7
    st.merge(R.State(len(idx)))
    assert R.same_bits(e.s, st.s) and R.same_bits(e.Q, st.Q) and st.n == 7
    empty = R.State(4)
    assert all(np.isnan(x).all() for x in R.close(empty.o, empty.s, empty.Q, empty.n))


def test_merge_of_long_halves_agrees_with_one_walk():
    frames = R.fitted_frames(40, 1030, 5)
    idx = np.arange(40)
    one, a, b = R.State(40), R.State(40), R.State(40)
    one.accumulate(frames, idx); a.accumulate(frames[:515], idx); b.accumulate(frames[515:], idx)
    a.merge(b)
    sd = R.two_pass(frames, idx)[2]
    c1, c2 = R.close(one.o, one.s, one.Q, one.n)[1], R.close(a.o, a.s, a.Q, a.n)[1]
    assert a.n == 1030 and (np.abs(c1 - c2) / np.outer(sd, sd)).max() <= REL


def test_dccm_of_the_restatement():
    frames = R.fitted_frames(50, 37, 8)
    frames = [x.copy() for x in frames]
    for x in frames:
        x[7] = frames[0][7]                                                      # an atom that does not move
    idx = np.arange(2, 30)
    st = R.State(len(idx)); st.accumulate(frames, idx)
    corr = R.dccm(R.close(st.o, st.s, st.Q, st.n)[1])
    k = 5                                                                         # atom 7 in group order
    moving = np.delete(np.arange(len(idx)), k)
    sub = corr[np.ix_(moving, moving)]
    assert np.abs(np.diagonal(sub) - 1.0).max() <= 1e-12 and np.abs(sub - sub.T).max() <= 1e-12
    assert sub.min() >= -1.0 - 1e-12 and sub.max() <= 1.0 + 1e-12
    assert corr[k, k] == 1.0 and np.isnan(corr[k, moving]).all() and np.isnan(corr[moving, k]).all()
    assert np.isnan(R.dccm(np.full((6, 6), np.nan))).all()
