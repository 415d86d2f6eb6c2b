"""Contacts (gr_contacts_*; groan_rs_amd.Contacts): what can be checked without a device -- that the header's section is mirrored in
_lib.py (parameter counts), include/groan_hip.hpp and the Rust shim, that the stat keys agree, the export, and the Python mirror's
argument handling (the nbins range, max_pairs)."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["gr_contacts_count_batch", "gr_contacts_create", "gr_contacts_destroy", "gr_contacts_hist_batch", "gr_contacts_pairs_batch", "gr_contacts_read",
         "gr_contacts_read_device", "gr_contacts_set_piece_frames", "gr_contacts_set_walk_groups", "gr_contacts_sizes", "gr_contacts_stat"]


def _header_prototypes():
    txt = open(os.path.join(ROOT, "include", "groan_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", " ", txt, flags=re.S)
    return {m.group(1): [p for p in m.group(2).split(",") if p.strip()] for m in re.finditer(r"\b(gr_contacts_[a-z_]+)\s*\(([^;{]*?)\)\s*;", txt, flags=re.S)}


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
    assert _lib.SIGNATURES["gr_contacts_create"][0] is C.c_void_p and _lib.SIGNATURES["gr_contacts_destroy"][0] is None
    assert _lib.SIGNATURES["gr_contacts_create"][1][3] is C.c_float          # the cut-off travels as f32
    assert "class Contacts" in hpp and "pub struct gr_contacts" in rs


def test_stat_keys_are_equal_everywhere():
    from groan_rs_amd import _lib
    txt = open(os.path.join(ROOT, "include", "groan_hip.h")).read()
    keys = {m.group(1): int(m.group(2)) for m in re.finditer(r"\bGR_CT_STAT_([A-Z_]+)\s*=\s*(\d+)", txt)}
    assert keys == {"LAST_LAUNCHES": _lib.CT_STAT_LAST_LAUNCHES, "LAST_PIECES": _lib.CT_STAT_LAST_PIECES, "LAST_TOTAL": _lib.CT_STAT_LAST_TOTAL,
                    "TILE": _lib.CT_STAT_TILE, "LAST_RUNS": _lib.CT_STAT_LAST_RUNS, "LAST_CELLS": _lib.CT_STAT_LAST_CELLS,
                    "LAST_RUN_CELLS_MIN": _lib.CT_STAT_LAST_RUN_CELLS_MIN, "LAST_RUN_CELLS_MAX": _lib.CT_STAT_LAST_RUN_CELLS_MAX,
                    "LAST_WALK_GROUPS": _lib.CT_STAT_LAST_WALK_GROUPS}
    rs = open(os.path.join(ROOT, "rust", "src", "groan_hip.rs")).read()
    rkeys = {m.group(1): int(m.group(2)) for m in re.finditer(r"pub\s+const\s+GR_CT_STAT_([A-Z_]+)\s*:\s*c_int\s*=\s*(\d+)", rs)}
    assert rkeys == keys
    src = open(os.path.join(ROOT, "groan_rs_amd", "csrc", "gr_contacts.h")).read()
    assert int(re.search(r"#define\s+GR_CT_MAX_BINS\s+(\d+)", src).group(1)) == _lib.CT_MAX_BINS == 4096


def test_contacts_is_exported():
    import groan_rs_amd as G
    assert G.Contacts is G.contacts.Contacts and "Contacts" in G.__all__
    for method in ("pairs", "lists", "frame", "lists_device", "counts", "hist", "set_piece_frames", "set_walk_groups", "stat", "close", "__enter__", "__exit__"):
        assert callable(getattr(G.Contacts, method)), method


def test_nbins_range():
    from groan_rs_amd.contacts import check_nbins
    assert [check_nbins(n) for n in (1, 7, 4096)] == [1, 7, 4096]
    for bad in (0, 4097, -1, 2.5, 10 ** 12):
        with pytest.raises(ValueError):
            check_nbins(bad)


def test_max_pairs():
    from groan_rs_amd.contacts import check_max_pairs, NO_LIMIT
    assert NO_LIMIT == 2 ** 64 - 1
    assert check_max_pairs(None) == NO_LIMIT
    assert check_max_pairs(0) == 0 and check_max_pairs(12345) == 12345 and check_max_pairs(NO_LIMIT) == NO_LIMIT
    for bad in (-1, 2 ** 64, 1.5):
        with pytest.raises(ValueError):
            check_max_pairs(bad)


def test_hist_refuses_its_bins_before_any_device_call():
    """the mirror checks nbins before it touches the object: `_lib` and `_ct` are never read"""
    import groan_rs_amd as G

    class Bare(G.Contacts):
        def __init__(self):
            pass

        def __getattr__(self, name):
            raise AssertionError("the mirror touched %s before refusing its arguments" % name)

    c = Bare()
    for bad in (0, 4097):
        with pytest.raises(ValueError):
            c.hist(0, 1, bad)
    with pytest.raises(ValueError):
        c.pairs(0, 1, max_pairs=-5)
