"""What the Region tests share (test_gpu_region.py, test_gpu_region_edges.py): shapes from their specs, a spec moved by a float32
anchor as the library moves it, and the oracle's per-frame lists (oracle_lib.group_from_geometries) in the form a Region call returns
them -- counts, offsets, one flat list.  Everything compared is an integer and every comparison is np.array_equal."""
import numpy as np

import oracle_lib as O

F = np.float32
E_NO_BOX, E_NOT_ORTHOGONAL, E_GROUP_NOT_FOUND, E_INVALID_ARG, E_UNSUPPORTED_BOX = 1, 2, 8, 10, 14


def build(G, spec):
    k = spec["kind"]
    if k == "sphere": return G.Sphere(spec["position"], spec["radius"])
    if k == "rectangular": return G.Rectangular(spec["position"], *spec["size"])
    if k == "cylinder": return G.Cylinder(spec["position"], spec["radius"], spec["height"], G.Dimension[spec["orientation"].upper()])
    return G.TriangularPrism(spec["base1"], spec["base2"], spec["base3"], spec["height"])


def moved(specs, a):
    """the specs moved by the float32 vector a: stored + a in float32, component by component"""
    a = np.asarray(a, F)
    out = []
    for sp in specs:
        sp = dict(sp)
        for key in ("position", "base1", "base2", "base3"):
            if key in sp:
                sp[key] = [float(v) for v in (np.asarray(sp[key], F) + a).astype(F)]
        out.append(sp)
    return out


def expect(frames, boxes, idx, specs, naive=False, anchors=None, failed=()):
    """-> (counts, offsets, flat list) of the oracle, frame by frame; frames in `failed` are empty"""
    lists = []
    for f, pos in enumerate(frames):
        if f in failed:
            lists.append(np.zeros(0, np.uint64))
            continue
        sp = specs if anchors is None else moved(specs, anchors[f])
        lists.append(O.group_from_geometries(pos, idx, boxes[f], sp, naive=naive))
    counts = np.array([l.size for l in lists], np.uint64)
    offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64)
    return counts, offsets, np.concatenate(lists).astype(np.uint64) if lists else np.zeros(0, np.uint64)


def check(region, got_counts, want):
    counts, offsets, flat = want
    off, atoms = region.lists()
    assert np.array_equal(got_counts, counts), (got_counts.tolist(), counts.tolist())
    assert off.dtype == np.uint64 and atoms.dtype == np.uint64
    assert np.array_equal(off, offsets) and np.array_equal(atoms, flat)
