"""RMSDPanel / rmsd_matrix (gr_rmsd_panel_*, gr_rmsd_matrix*; groan_rs_amd.RMSDPanel): what can be checked without a device -- that the
header's section is mirrored in _lib.py (parameter counts), include/groan_hip.hpp and the Rust shim, that the limits agree between the
kernel source and the Python mirror, the export, and the mirror's argument handling (capacity, the size of a device-side matrix)."""
import ctypes as C
import importlib
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["gr_rmsd_matrix", "gr_rmsd_matrix_device", "gr_rmsd_panel_append_batch", "gr_rmsd_panel_clear", "gr_rmsd_panel_create", "gr_rmsd_panel_destroy",
         "gr_rmsd_panel_frames", "gr_rmsd_panel_n_atoms", "gr_rmsd_panel_set_block_entries", "gr_rmsd_panel_status"]


def _header_prototypes():
    txt = open(os.path.join(ROOT, "include", "groan_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", " ", txt, flags=re.S)
    return {m.group(1): [p for p in m.group(2).split(",") if p.strip()]
            for m in re.finditer(r"\b(gr_rmsd_(?:panel_[a-z_]+|matrix(?:_device)?))\s*\(([^;{]*?)\)\s*;", txt, flags=re.S)}


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
    assert _lib.SIGNATURES["gr_rmsd_panel_create"][0] is C.c_void_p and _lib.SIGNATURES["gr_rmsd_panel_destroy"][0] is None
    assert _lib.SIGNATURES["gr_rmsd_panel_frames"][0] is C.c_uint32 and _lib.SIGNATURES["gr_rmsd_panel_n_atoms"][0] is C.c_uint64
    assert "class RmsdPanel" in hpp and "pub struct gr_rmsd_panel" in rs


def test_limits_are_equal_in_the_source_and_the_mirror():
    M = importlib.import_module("groan_rs_amd.rmsd_matrix")       # (the package exports the function of the same name)
    src = open(os.path.join(ROOT, "groan_rs_amd", "csrc", "gr_rmsd_panel.h")).read()
    shift = lambda name: int(re.search(r"#define\s+%s\s+\(1u?l?l?\s*<<\s*(\d+)\)" % name, src).group(1))
    assert 1 << shift("GR_RP_MAX_FRAMES") == M.MAX_FRAMES == 1 << 20
    assert 1 << shift("GR_RP_MAX_DEVICE_ENTRIES") == M.MAX_DEVICE_ENTRIES == 1 << 28
    # the tile the edge tests are written around: 8 row frames x 16 column frames, 16 atoms per trip of a wave
    tile = {k: int(re.search(r"#define\s+GR_RP_%s\s+(\d+)u" % k, src).group(1)) for k in ("ROW_FRAMES", "COL_FRAMES", "KSTEP")}
    assert tile == {"ROW_FRAMES": 8, "COL_FRAMES": 16, "KSTEP": 16}


def test_panel_is_exported():
    import groan_rs_amd as G
    M = importlib.import_module("groan_rs_amd.rmsd_matrix")
    assert G.RMSDPanel is M.RMSDPanel and G.rmsd_matrix is M.rmsd_matrix and "RMSDPanel" in G.__all__ and "rmsd_matrix" in G.__all__
    assert callable(G.rmsd_matrix)
    for method in ("append", "clear", "set_block_entries", "close", "__len__", "__enter__", "__exit__"):
        assert callable(getattr(G.RMSDPanel, method)), method
    assert isinstance(G.RMSDPanel.status, property)


def test_capacity_range():
    from groan_rs_amd.rmsd_matrix import check_capacity
    assert [check_capacity(n) for n in (1, 21, 1 << 20)] == [1, 21, 1 << 20]
    for bad in (0, -1, 2.5, (1 << 20) + 1):
        with pytest.raises(ValueError):
            check_capacity(bad)


def test_device_matrix_size():
    from groan_rs_amd.rmsd_matrix import check_device_size
    check_device_size(1 << 14, 1 << 14)
    with pytest.raises(ValueError):
        check_device_size((1 << 14) + 1, 1 << 14)


def test_panel_refuses_its_capacity_before_any_device_call():
    """the mirror checks the capacity before it loads the library or touches the system"""
    import groan_rs_amd as G

    class NoSystem:
        def __getattr__(self, name):
            raise AssertionError("the mirror touched the system (%s) before refusing its arguments" % name)

    for bad in (0, (1 << 20) + 1):
        with pytest.raises(ValueError):
            G.RMSDPanel(NoSystem(), "Protein", bad)
