"""Region (gr_region_*; groan_rs_amd.Region): what can be checked without a device -- the Python mirror's argument handling (shape
packing, the anchor array's shape and dtype) and that the header's new section is mirrored in _lib.py and include/groan_hip.hpp."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header_prototypes():
    txt = open(os.path.join(ROOT, "include", "groan_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", " ", txt, flags=re.S)
    return {m.group(1): [p for p in m.group(2).split(",") if p.strip()] for m in re.finditer(r"\b(gr_region_[a-z_]+)\s*\(([^;{]*?)\)\s*;", txt, flags=re.S)}


def test_header_section_is_mirrored_in_lib_and_hpp():
    from groan_rs_amd import _lib
    protos = _header_prototypes()
    assert sorted(protos) == ["gr_region_create", "gr_region_destroy", "gr_region_group", "gr_region_read", "gr_region_read_device",
                              "gr_region_select_batch", "gr_region_set_piece_frames", "gr_region_stat"]
    hpp = open(os.path.join(ROOT, "include", "groan_hip.hpp")).read()
    for name, params in protos.items():
        assert name in _lib.SIGNATURES, name
        assert len(_lib.SIGNATURES[name][1]) == len(params), (name, len(_lib.SIGNATURES[name][1]), len(params))
        assert re.search(r"\b%s\s*\(" % name, hpp), name
    assert _lib.SIGNATURES["gr_region_create"][0] is C.c_void_p and _lib.SIGNATURES["gr_region_destroy"][0] is None
    # the stat keys of the header are the module's
    txt = open(os.path.join(ROOT, "include", "groan_hip.h")).read()
    keys = {m.group(1): int(m.group(2)) for m in re.finditer(r"\bGR_RG_STAT_([A-Z_]+)\s*=\s*(\d+)", txt)}
    assert keys == {"LAST_LAUNCHES": _lib.RG_STAT_LAST_LAUNCHES, "LAST_PIECES": _lib.RG_STAT_LAST_PIECES, "LAST_TOTAL": _lib.RG_STAT_LAST_TOTAL,
                    "CHUNK": _lib.RG_STAT_CHUNK}
    assert int(re.search(r"#define\s+GR_MAX_SHAPES\s+(\d+)", txt).group(1)) == _lib.MAX_SHAPES


def test_region_is_exported():
    import groan_rs_amd as G
    assert G.Region is G.region.Region and "Region" in G.__all__
    for method in ("select", "lists", "frame", "to_group", "close"):
        assert callable(getattr(G.Region, method))


def test_anchor_array_shape_and_dtype():
    from groan_rs_amd.region import pack_anchors
    assert pack_anchors(None, 5) is None
    a = np.arange(12, dtype=np.float32).reshape(4, 3)
    out = pack_anchors(a, 4)
    assert out.dtype == np.float32 and out.flags["C_CONTIGUOUS"] and np.array_equal(out, a)
    strided = np.zeros((4, 6), np.float32)[:, ::2]                       # not contiguous: copied, same values
    strided[:] = a
    out = pack_anchors(strided, 4)
    assert out.flags["C_CONTIGUOUS"] and np.array_equal(out, a)
    for bad in (a.astype(np.float64), a.astype(np.int32), a.tolist()):   # only float32: the bits that are added are the caller's
        with pytest.raises(TypeError):
            pack_anchors(bad, 4)
    for bad, n in ((a, 3), (a, 5), (a.ravel(), 4), (a.T.copy(), 4), (a[:, :2].copy(), 4), (np.zeros((0, 3), np.float32), 1)):
        with pytest.raises(ValueError):
            pack_anchors(bad, n)


def test_shape_packing_and_refusals_before_any_device_call():
    """packing is groan_rs_amd.shapes.pack (gr_shape records in order); too many shapes and a naive prism are refused by the mirror
    before it asks for a context -- `system` is never touched"""
    import groan_rs_amd as G
    from groan_rs_amd.shapes import GrShape, pack
    shapes = [G.Sphere([1, 2, 3], 0.5), G.Cylinder([0, 0, -2], 2.0, 4.0, G.Dimension.Z), G.Rectangular([1, 1, 1], 2, 3, 4),
              G.TriangularPrism([3, 4, 2], [7, 5, 2], [4, 3, 2], 4.3)]
    arr, n = pack(shapes)
    assert n == 4 and C.sizeof(arr) == 4 * C.sizeof(GrShape) and C.sizeof(GrShape) == 60
    assert [arr[k].kind for k in range(4)] == [1, 3, 2, 4]
    assert list(arr[1].position) == [0.0, 0.0, -2.0] and list(arr[1].size)[:2] == [2.0, 4.0] and arr[1].orientation == int(G.Dimension.Z)
    assert list(arr[3].base2) == [7.0, 5.0, 2.0] and list(arr[3].base3) == [4.0, 3.0, 2.0]
    arr0, n0 = pack([])
    assert n0 == 0 and len(arr0) == 1                                    # (a pointer to hand over)

    class NoSystem:
        def __getattr__(self, name):
            raise AssertionError("the mirror touched the system (%s) before refusing its arguments" % name)

    with pytest.raises(ValueError):
        G.Region(NoSystem(), [G.Sphere([0, 0, 0], 1.0)] * (G._lib.MAX_SHAPES + 1))
    with pytest.raises(TypeError):
        G.Region(NoSystem(), [shapes[0], shapes[3]], naive=True)
