"""The batch objects of the C++ mirror (include/groan_hip.hpp: HBondPlan, GridMap, Segments, Region, Contacts, RmsdPanel, Fluctuations,
Covariance) on the GPU: tests/cpp/test_objects.cpp runs once over the world of cpp_objects_world.py and writes every array its calls
return; each test compares one class's arrays with

  1. that object's own reference -- the restatement or oracle call, the tolerance and the checking helper of its own GPU test, and
  2. the Python class of the same name, run here on a fresh System through the same calls in the same order: bit for bit.  Both mirrors
     go through one C ABI and every object's result is documented not to depend on the context, so any difference is a layout, size or
     argument error in one of the two.

The program itself has already checked the sizes of what it got, the moves, the errors and the repeated calls (its exit code).  No
case is left out of a comparison: test_cpp_objects_world.py shows that no atom of the world sits on a decision point."""
import os
import subprocess
import time

import numpy as np
import pytest

import covar_ref
import cpp_objects_world as W
import fluct_ref
import gridmap_ref
import hbond_ref
import oracle_lib as O
import region_ref
import rmsd_matrix_ref
import segments_ref
import test_gpu_contacts as TC
import test_gpu_covar as TV
import test_gpu_fluct as TF

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
NS, N = W.NS, W.N
DTYPES = {"f32": "<f4", "f64": "<f8", "u32": "<u4", "u64": "<u8", "i32": "<i4", "i64": "<i8"}
CLOSING = 1e-12         # test_gpu_fluct.py / test_gpu_covar.py: the library's closing step against the restatement's
MERGED = 1e-9           # test_gpu_fluct.py test_merge: the merged sums against the restatement's merge
MERGED_ULPS = 8.0       # test_gpu_covar.py test_merge: ulps of the absolute sums on top of the halves' bounds


@pytest.fixture(scope="module")
def G():
    import groan_rs_amd as g
    g._lib.load()
    return g


@pytest.fixture(scope="module")
def world():
    return W.build()


@pytest.fixture(scope="module")
def cpp(world, tmp_path_factory):
    """{file name: array}: what one run of the program wrote"""
    fixtures, out = tmp_path_factory.mktemp("cpp_objects_world"), tmp_path_factory.mktemp("cpp_objects_out")
    W.write(world, str(fixtures))
    exe = os.path.join(ROOT, "tests", "cpp", "test_objects")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "tests", "cpp"), "test_objects"])
    env = dict(os.environ)
    env["LD_LIBRARY_PATH"] = os.path.join(ROOT, "groan_rs_amd") + ":/opt/rocm/lib:" + env.get("LD_LIBRARY_PATH", "")
    t0 = time.perf_counter()
    p = subprocess.run([exe, str(fixtures), str(out)], capture_output=True, text=True, env=env, timeout=120)
    print("test_objects: %.2f s" % (time.perf_counter() - t0))
    print(p.stdout, p.stderr)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "all passed" in p.stdout
    return {name: np.fromfile(os.path.join(str(out), name), DTYPES[name.rsplit(".", 1)[1]]) for name in sorted(os.listdir(str(out)))}


# ------------------------------------------------------------------ the same calls through the Python classes
def _system(G, world):
    s = G.System(N, masses=world["masses"], n_slots=NS)
    for f in range(NS):
        s.set_frame(world["frames"][f], world["boxes"][f], slot=f)
    for name, idx in W.GROUPS.items():
        if name in W.RANGES:
            s.group_create_from_ranges(name, [W.RANGES[name]])
        else:
            s.group_create_from_indices(name, idx)
    s.add_bonds(W.BONDS)
    return s


def _py_hbonds(G, s, out):
    chains = [G.HBondChain(*c) for c in W.CHAINS]

    def put(name, r, status=True):
        don, hyd, acc, dist, ang, offsets, st = r
        out[name + ".atoms.u32"] = np.stack([don, hyd, acc], 1).ravel()
        out[name + ".values.f32"] = np.stack([dist, ang], 1).ravel()
        out[name + ".n.u64"] = np.diff(offsets)
        if status:
            out[name + ".status.i32"] = st

    an = G.HBondAnalysis(s, chains, W.HB_PAIRS, W.HB_DIST, W.HB_ANGLE, W.BONDS)
    put("hbond.all", an.batch(0, NS, raise_on_error=False))
    an.batch(0, NS, raise_on_error=False)
    with pytest.raises(G.GroanError):
        an.batch(0, NS)
    put("hbond.one", an.batch(3, 1), status=False)
    put("hbond.tail", an.batch(7, 3, raise_on_error=False))
    none = G.HBondAnalysis(s, chains, W.HB_PAIRS, W.HB_DIST_NONE, W.HB_ANGLE, W.BONDS)
    put("hbond.none", none.batch(0, 3, raise_on_error=False))
    an.close(); none.close()


def _py_gridmap(G, s, out):
    def read(m, name):
        cnt, sq, mean = m._read(True)
        out[name + ".counts.u64"], out[name + ".sums_q.i64"], out[name + ".mean.f32"] = cnt.ravel(), sq.ravel(), mean.ravel()

    m = G.GridMap(s, *W.MAP1)
    out["gridmap.m1.dims.u64"] = np.array([m.n_tiles_x, m.n_tiles_y], np.uint64)
    tiles = [m.get_tile(x, y) for x, y in W.GM_POINTS]
    out["gridmap.m1.inside.i32"] = np.array([t is not None for t in tiles], np.int32)
    out["gridmap.m1.tiles.f32"] = np.array([t if t is not None else (np.nan, np.nan) for t in tiles], F).ravel()
    out["gridmap.count.outside.u64"], out["gridmap.count.status.i32"] = m.accumulate("rng", 0, NS, raise_on_error=False)
    read(m, "gridmap.count")
    with pytest.raises(G.GroanError):
        m.accumulate("rng", 0, NS)
    m.clear()
    m.accumulate("rng", 0, NS, raise_on_error=False)
    out["gridmap.z.outside.u64"] = m.accumulate("lst", 3, 1, value=G.Dimension.Z, offset=[W.GM_OFFSET_Z])[0]
    read(m, "gridmap.z")
    out["gridmap.x.outside.u64"] = m.accumulate("hyd", 0, 4, value=G.Dimension.X)[0]
    read(m, "gridmap.x")
    m.clear()
    read(m, "gridmap.cleared")
    fb = G.GridMap.from_box(s, W.MAP2_TILE, W.MAP2_SLOT)
    out["gridmap.m2.dims.u64"] = np.array([fb.n_tiles_x, fb.n_tiles_y], np.uint64)
    out["gridmap.wrap.outside.u64"], out["gridmap.wrap.status.i32"] = fb.accumulate("hyd", 0, NS, value=G.Dimension.Y, wrap=True, raise_on_error=False)
    read(fb, "gridmap.wrap")
    fb.clear(); fb.set_launch(1, 1, 1)                                      # (the launch caps never change a result)
    fb.accumulate("hyd", 0, NS, value=G.Dimension.Y, wrap=True, raise_on_error=False)
    m.close(); fb.close()


def _py_segments(G, s, out):
    L = G._lib
    s1, s2, s3 = G.Segments.from_lists(s, W.SEG_LISTS), G.Segments.by_resid(s, W.LABELS, "rng"), G.Segments.from_molecules(s)
    for name, sg in (("seg1", s1), ("seg2", s2), ("seg3", s3)):
        out[name + ".sizes.u64"] = sg.sizes
        out[name + ".atoms.u64"] = np.concatenate([sg.atoms(k) for k in range(len(sg))])
    c, st = s1.centers(0, NS, L.CENTER_PBC, True, raise_on_error=False)
    out["seg1.pbc_w.centers.f32"], out["seg1.pbc_w.status.i32"] = c.ravel(), st
    with pytest.raises(G.GroanError):
        s1.centers(0, NS, L.CENTER_PBC, True)
    c, st = s1.centers(0, NS, L.CENTER_NAIVE, False, raise_on_error=False)
    out["seg1.naive.centers.f32"], out["seg1.naive.status.i32"] = c.ravel(), st
    out["seg2.com_one.centers.f32"] = s2.get_com(2, 1)[0].ravel()
    c, st = s2.centers(0, NS, L.CENTER_ESTIMATE, True, raise_on_error=False)
    out["seg2.est_w.centers.f32"], out["seg2.est_w.status.i32"] = c.ravel(), st
    out["seg3.center_tail.centers.f32"] = s3.get_center(7, 3)[0].ravel()
    for sg in (s1, s2, s3):
        sg.close()


def _py_region(G, s, out):
    rg = G.Region(s, [region_ref.build(G, sp) for sp in W.SHAPES_A])
    counts, st = rg.select("hyd", 0, NS, raise_on_error=False)
    off, atoms = rg.lists()
    out["region.a_all.counts.u64"], out["region.a_all.status.i32"], out["region.a_all.offsets.u64"], out["region.a_all.atoms.u64"] = counts, st, off, atoms
    out["region.a_all.frame_first.u64"], out["region.a_all.frame_last.u64"] = rg.frame(0), rg.frame(NS - 1)
    with pytest.raises(IndexError):
        rg.frame(NS)
    assert rg.to_group(0, "picked") is False and rg.to_group(NS - 1, "picked") is True
    with pytest.raises(G.GroanError):
        rg.select("hyd", 0, NS)
    counts, st = rg.select("rng", 2, 1, anchors=W.ANCHOR_ONE)
    off, atoms = rg.lists()
    out["region.a_one.counts.u64"], out["region.a_one.offsets.u64"], out["region.a_one.atoms.u64"] = counts, off, atoms
    counts, st = rg.select("hyd", 7, 3, anchors=W.ANCHORS_3, raise_on_error=False)
    off, atoms = rg.lists()
    out["region.a_anch.counts.u64"], out["region.a_anch.status.i32"], out["region.a_anch.offsets.u64"], out["region.a_anch.atoms.u64"] = counts, st, off, atoms
    rg.select("hyd", 7, 3, anchors=W.ANCHORS_3)
    rg.set_piece_frames(1)
    rg.select("hyd", 7, 3, anchors=W.ANCHORS_3)
    empty = G.Region(s, [region_ref.build(G, sp) for sp in W.SHAPES_EMPTY])
    counts, st = empty.select(None, 0, 3)
    off, atoms = empty.lists()
    out["region.empty.counts.u64"], out["region.empty.offsets.u64"], out["region.empty.atoms.u64"] = counts, off, atoms
    rg.close(); empty.close()


def _py_contacts(G, s, out):
    ct = G.Contacts(s, "rng", "hyd", W.CT_CUT)
    out["contacts.all.n.u64"], out["contacts.all.status.i32"] = ct.pairs(0, NS, raise_on_error=False)
    out["contacts.all.offsets.u64"], out["contacts.all.i.u32"], out["contacts.all.j.u32"], out["contacts.all.d.f32"] = ct.lists()
    with pytest.raises(G.GroanError):
        ct.pairs(0, NS)
    out["contacts.counts.per_atom.u32"], out["contacts.counts.n.u64"], out["contacts.counts.status.i32"] = ct.counts(0, NS, raise_on_error=False)
    out["contacts.counts.per_atom.u32"] = out["contacts.counts.per_atom.u32"].ravel()
    h, st = ct.hist(0, NS, W.CT_NBINS, raise_on_error=False)
    out["contacts.hist.hist.u64"], out["contacts.hist.status.i32"] = h.ravel(), st
    out["contacts.one.n.u64"] = ct.pairs(5, 1)[0]
    _, out["contacts.one.i.u32"], out["contacts.one.j.u32"], out["contacts.one.d.f32"] = ct.lists()
    out["contacts.counts_tail.per_atom.u32"] = ct.counts(7, 3)[0].ravel()
    out["contacts.hist_one.hist.u64"] = ct.hist(8, 1, 5)[0].ravel()
    out["contacts.count_only.n.u64"] = ct.pairs(0, 3, max_pairs=W.CT_MAX_PAIRS, raise_on_error=False)[0]
    with pytest.raises(G.GroanError):
        ct.lists()
    ct.pairs(5, 1)
    ct.set_piece_frames(1); ct.set_walk_groups(1)
    ct.pairs(7, 3); ct.counts(7, 3)
    none = G.Contacts(s, "oxy", "oxy", W.CT_CUT_NONE)
    out["contacts.none.n.u64"] = none.pairs(0, 3)[0]
    out["contacts.none.offsets.u64"] = none.lists()[0]
    ct.close(); none.close()


def _py_rmsd(G, s, out):
    rows, cols = G.RMSDPanel(s, "rng", NS), G.RMSDPanel(s, "rng", 4)
    out["rmsd.rows.append.i32"] = rows.append(0, NS, raise_on_error=False)
    out["rmsd.rows.status.i32"] = rows.status
    cols.append(7, 3); cols.append(2, 1)
    out["rmsd.cols.status.i32"] = cols.status
    out["rmsd.self.matrix.f32"] = G.rmsd_matrix(rows).ravel()
    out["rmsd.rows_cols.matrix.f32"] = G.rmsd_matrix(rows, cols).ravel()
    out["rmsd.cols_rows.matrix.f32"] = G.rmsd_matrix(cols, rows).ravel()
    rows.close(); cols.close()


def _py_fluct(G, s, one, out):
    def read(fl, name):
        o, sm, sq, n = fl.raw()
        out[name + ".mean.f64"], out[name + ".variance.f64"], out[name + ".rmsf.f64"] = fl.mean().ravel(), fl.variance().ravel(), fl.rmsf()
        out[name + ".origin.f32"], out[name + ".sum.f64"], out[name + ".sumsq.f64"], out[name + ".n.u64"] = o.ravel(), sm.ravel(), sq.ravel(), np.array([n], np.uint64)

    fl, part = G.Fluctuations(s, "rng"), G.Fluctuations(s, "rng")
    out["fluct.all.status.i32"] = fl.accumulate(0, NS, raise_on_error=False)
    read(fl, "fluct.all")
    part.accumulate(7, 3); part.accumulate(2, 1)
    read(part, "fluct.part")
    fl.merge(part)
    read(fl, "fluct.merged")
    fl.store_mean(one, 0)
    out["fluct.merged.stored.f32"] = one.get_positions(0).ravel()
    with G.Fluctuations(s, "rng") as cut:
        cut.set_launch(3, 1)
        cut.accumulate(0, NS, raise_on_error=False)
    fl.clear()
    read(fl, "fluct.cleared")
    fl.close(); part.close()


def _py_covar(G, s, out):
    def read(cv, name):
        o, sm, Q, n = cv.raw()
        out[name + ".mean.f64"], out[name + ".cov.f64"], out[name + ".cov_mw.f64"], out[name + ".dccm.f64"] = cv.mean().ravel(), cv.matrix().ravel(), cv.matrix(True).ravel(), cv.dccm().ravel()
        out[name + ".origin.f32"], out[name + ".sum.f64"], out[name + ".Q.f64"], out[name + ".n.u64"] = o.ravel(), sm.ravel(), Q.ravel(), np.array([n], np.uint64)

    cv, part = G.Covariance(s, "lst"), G.Covariance(s, "lst")
    out["covar.all.status.i32"] = cv.accumulate(0, NS, raise_on_error=False)
    read(cv, "covar.all")
    part.accumulate(7, 3); part.accumulate(2, 1)
    read(part, "covar.part")
    cv.merge(part)
    read(cv, "covar.merged")
    with G.Covariance(s, "lst") as capped:
        capped.set_launch(1, 1)
        capped.accumulate(0, NS, raise_on_error=False)
    cv.clear()
    read(cv, "covar.cleared")
    cv.close(); part.close()


@pytest.fixture(scope="module")
def py(G, world):
    """{file name: array}: the Python classes through the calls of the program, in its order, on a fresh System"""
    s = _system(G, world)
    one = G.System(N, masses=world["masses"], n_slots=1)
    one.set_frame(np.zeros((N, 3), F), world["boxes"][0])
    out = {}
    _py_hbonds(G, s, out)
    _py_gridmap(G, s, out)
    _py_segments(G, s, out)
    _py_region(G, s, out)
    _py_contacts(G, s, out)
    _py_rmsd(G, s, out)
    _py_fluct(G, s, one, out)
    _py_covar(G, s, out)
    one.close()
    yield out, s
    s.close()


def same_as_python(cpp, py, prefix):
    """every array of the class, bit for bit; both sides hold the same set of arrays"""
    names = sorted(n for n in cpp if n.startswith(prefix))
    assert names and names == sorted(n for n in py[0] if n.startswith(prefix))
    for n in names:
        want = np.ascontiguousarray(py[0][n])
        assert want.dtype == np.dtype(DTYPES[n.rsplit(".", 1)[1]]), (n, want.dtype)
        assert cpp[n].shape == want.shape and cpp[n].tobytes() == want.tobytes(), n


def expected_status(needs_box=True, needs_position=True, first=0, n=NS):
    st = np.zeros(NS, np.int32)
    if needs_position:
        st[W.NAN_SLOT] = W.E_NO_POSITION
    if needs_box:
        st[W.NOBOX_SLOT] = W.E_NO_BOX
    return st[first:first + n]


def test_every_array_belongs_to_a_test(cpp):
    prefixes = ("hbond.", "gridmap.", "seg", "region.", "contacts.", "rmsd.", "fluct.", "covar.")
    assert all(n.startswith(prefixes) for n in cpp) and len(cpp) > 100


# ------------------------------------------------------------------ HBondPlan
def test_hbond_plan(cpp, py, world):
    same_as_python(cpp, py, "hbond.")
    for call, first, n, dist in (("all", 0, NS, W.HB_DIST), ("one", 3, 1, W.HB_DIST), ("tail", 7, 3, W.HB_DIST), ("none", 0, 3, W.HB_DIST_NONE)):
        atoms, values, counts = cpp["hbond.%s.atoms.u32" % call].reshape(-1, 3), cpp["hbond.%s.values.f32" % call].reshape(-1, 2), cpp["hbond.%s.n.u64" % call]
        assert counts.size == n * len(W.HB_PAIRS) and int(counts.sum()) == len(atoms) == len(values)
        k, total, status = 0, 0, []
        for f in range(first, first + n):
            want, st = W.hbonds_of(world["frames"][f], world["boxes"][f], dist, W.HB_ANGLE)
            status.append(st)
            for p, key in enumerate(W.HB_PAIRS):                                    # [f][p] order
                m = int(counts[(f - first) * len(W.HB_PAIRS) + p])
                assert m == len(want[key]), (call, f, key)
                for g_a, g_v, w in zip(atoms[k:k + m], values[k:k + m], want[key]):
                    assert hbond_ref.close((g_a[0], g_a[1], g_a[2], g_v[0], g_v[1]), w), (call, f, key, g_a, g_v, w)
                k += m; total += m
        if call != "one":
            assert cpp["hbond.%s.status.i32" % call].tolist() == status
        assert (total == 0) == (call == "none")
    assert cpp["hbond.all.status.i32"][W.NOBOX_SLOT] == W.E_NO_BOX


# ------------------------------------------------------------------ GridMap
def test_gridmap(cpp, py, world):
    same_as_python(cpp, py, "gridmap.")
    R, fr, bx = gridmap_ref, world["frames"], world["boxes"]

    def same(name, ref):
        shape = (ref.nx, ref.ny)
        assert np.array_equal(cpp[name + ".counts.u64"].reshape(shape), ref.count) and np.array_equal(cpp[name + ".sums_q.i64"].reshape(shape), ref.sum_q)
        assert np.array_equal(cpp[name + ".mean.f32"].reshape(shape).view(np.uint32), ref.mean().view(np.uint32))

    ref = R.Map(*W.MAP1)
    assert cpp["gridmap.m1.dims.u64"].tolist() == [ref.nx, ref.ny]
    sx, sy, td = W.MAP1
    ix, iy = R.coord2index(W.GM_POINTS[:, 0], sx[0], td[0]), R.coord2index(W.GM_POINTS[:, 1], sy[0], td[1])
    inside = (ix >= 0) & (ix < ref.nx) & (iy >= 0) & (iy < ref.ny)
    assert cpp["gridmap.m1.inside.i32"].tolist() == inside.astype(int).tolist() and inside.tolist() == [True, True, False, False, False, False, False]
    tiles = np.where(inside[:, None], np.stack([R.index2coord(ix, sx[0], td[0]), R.index2coord(iy, sy[0], td[1])], 1), F(np.nan)).astype(F)
    assert np.array_equal(cpp["gridmap.m1.tiles.f32"].view(np.uint32), tiles.ravel().view(np.uint32))
    n_out, st, _ = ref.accumulate(fr, bx, W.GROUPS["rng"], R.COUNT)
    assert cpp["gridmap.count.outside.u64"].tolist() == n_out.tolist() and cpp["gridmap.count.status.i32"].tolist() == st.tolist()
    assert st.tolist() == expected_status(needs_box=False).tolist()
    same("gridmap.count", ref)
    n_out, st, _ = ref.accumulate(fr[3:4], bx[3:4], W.GROUPS["lst"], R.Z, np.array([W.GM_OFFSET_Z], F))
    assert cpp["gridmap.z.outside.u64"].tolist() == n_out.tolist()
    same("gridmap.z", ref)
    n_out, st, _ = ref.accumulate(fr[0:4], bx[0:4], W.GROUPS["hyd"], R.X)
    assert cpp["gridmap.x.outside.u64"].tolist() == n_out.tolist() and ref.sum_q.any()
    same("gridmap.x", ref)
    ref.clear()
    same("gridmap.cleared", ref)
    ref2 = R.Map(*W.map2_spans(bx), W.MAP2_TILE)
    assert cpp["gridmap.m2.dims.u64"].tolist() == [ref2.nx, ref2.ny]
    n_out, st, _ = ref2.accumulate(fr, bx, W.GROUPS["hyd"], R.Y, None, True, lambda p, box: O.wrap_atoms(p, np.arange(len(p)), box))
    assert cpp["gridmap.wrap.outside.u64"].tolist() == n_out.tolist() and cpp["gridmap.wrap.status.i32"].tolist() == st.tolist()
    assert st.tolist() == expected_status().tolist()
    same("gridmap.wrap", ref2)
    assert int(ref2.count.sum()) == 8 * len(W.GROUPS["hyd"])              # the wrap brought the molecules outside the box into the map


# ------------------------------------------------------------------ Segments
def test_segments(cpp, py, world):
    same_as_python(cpp, py, "seg")
    S, fr, bx = segments_ref, world["frames"], world["boxes"]
    lists = W.segment_lists()
    calls = {"seg1": [("pbc_w", (S.PBC, 1), 0, NS, True), ("naive", (S.NAIVE, 0), 0, NS, True)],
             "seg2": [("com_one", (S.PBC, 1), 2, 1, False), ("est_w", (S.ESTIMATE, 1), 0, NS, True)],
             "seg3": [("center_tail", (S.PBC, 0), 7, 3, False)]}
    for seg, seg_calls in calls.items():
        L = lists[seg]
        assert cpp[seg + ".sizes.u64"].tolist() == [len(a) for a in L] and np.array_equal(cpp[seg + ".atoms.u64"], np.concatenate(L))
        ref = S._reference(fr, bx, world["masses"], L)
        for call, key, first, n, has_status in seg_calls:
            got = cpp["%s.%s.centers.f32" % (seg, call)].reshape(n, len(L), 3)
            status = cpp["%s.%s.status.i32" % (seg, call)] if has_status else np.zeros(n, np.int32)
            cen, errs, flags = ref[key]
            part = {key: (cen[first:first + n], errs[first:first + n], None if flags is None else flags[first:first + n])}
            assert flags is None or not flags.any()                                 # no centre near a cell face: nothing is compared modulo the box
            S._check_against(got, status, part, key, bx[first:first + n])
    assert len(set(len(a) for L in lists.values() for a in L)) >= 5 and sum(len(L) for L in lists.values()) >= 5
    assert cpp["seg1.pbc_w.status.i32"].tolist() == expected_status().tolist()
    assert cpp["seg1.naive.status.i32"].tolist() == expected_status(needs_box=False).tolist()


# ------------------------------------------------------------------ Region
def test_region(cpp, py, world):
    same_as_python(cpp, py, "region.")
    for name, specs, group, first, n, anchors in W.region_calls():
        idx = np.arange(N) if group is None else W.GROUPS[group]
        bx = world["boxes"][first:first + n]
        failed = [k for k in range(n) if bx[k] is None]
        counts, offsets, flat = region_ref.expect(world["frames"][first:first + n], bx, idx, specs, anchors=anchors, failed=failed)
        pre = "region.%s." % name
        assert np.array_equal(cpp[pre + "counts.u64"], counts) and np.array_equal(cpp[pre + "offsets.u64"], offsets) and np.array_equal(cpp[pre + "atoms.u64"], flat)
        if pre + "status.i32" in cpp:
            assert cpp[pre + "status.i32"].tolist() == expected_status(needs_position=False, first=first, n=n).tolist()
        assert (flat.size == 0) == (name == "empty")
    off, atoms = cpp["region.a_all.offsets.u64"], cpp["region.a_all.atoms.u64"]
    assert np.array_equal(cpp["region.a_all.frame_first.u64"], atoms[:int(off[1])]) and np.array_equal(cpp["region.a_all.frame_last.u64"], atoms[int(off[NS - 1]):])


# ------------------------------------------------------------------ Contacts
def test_contacts(cpp, py, world):
    same_as_python(cpp, py, "contacts.")
    fr, bx = world["frames"], world["boxes"]
    idx1, idx2 = W.GROUPS["rng"], W.GROUPS["hyd"]
    want_st = expected_status()
    off, i, j, d = (cpp["contacts.all.%s" % k] for k in ("offsets.u64", "i.u32", "j.u32", "d.f32"))
    assert off.size == NS + 1 and np.array_equal(np.diff(off), cpp["contacts.all.n.u64"])
    for key in ("all", "counts", "hist"):
        assert cpp["contacts.%s.status.i32" % key].tolist() == want_st.tolist()
    assert [TC.slot_status(py[1], "rng", "hyd", W.CT_CUT, f)[0] for f in range(NS)] == want_st.tolist()      # ... which is what the per-slot call reports
    good = [f for f in range(NS) if want_st[f] == 0]
    assert all(off[f] == off[f + 1] for f in range(NS) if want_st[f] != 0)
    # the oracle, on the frames that did not fail: indices identical, d within the margin of test_gpu_contacts.py
    parts = [slice(int(off[f]), int(off[f + 1])) for f in good]
    packed = (np.concatenate([[0], np.cumsum([p.stop - p.start for p in parts])]), *(np.concatenate([a[p] for p in parts]) for a in (i, j, d)))
    TC.check_oracle(packed, [fr[f] for f in good], [bx[f] for f in good], idx1, idx2, W.CT_CUT)
    # counts and hist: numpy on the lists
    per_atom, hist = cpp["contacts.counts.per_atom.u32"].reshape(NS, idx1.size), cpp["contacts.hist.hist.u64"].reshape(NS, W.CT_NBINS)
    lookup = np.full(N, -1, np.int64); lookup[idx1] = np.arange(idx1.size)
    for f in range(NS):
        a, b = int(off[f]), int(off[f + 1])
        assert np.array_equal(per_atom[f], np.bincount(lookup[i[a:b]], minlength=idx1.size).astype(np.uint32))
        assert np.array_equal(hist[f], TC.numpy_hist(d[a:b], W.CT_CUT, W.CT_NBINS))
    assert np.array_equal(cpp["contacts.counts.n.u64"], cpp["contacts.all.n.u64"]) and len(set(per_atom[0].tolist())) > 2
    # the single frame and the tails are the batch's
    a, b = int(off[5]), int(off[6])
    assert cpp["contacts.one.n.u64"].tolist() == [b - a]
    assert np.array_equal(cpp["contacts.one.i.u32"], i[a:b]) and np.array_equal(cpp["contacts.one.j.u32"], j[a:b]) and np.array_equal(cpp["contacts.one.d.f32"].view(np.uint32), d[a:b].view(np.uint32))
    assert np.array_equal(cpp["contacts.counts_tail.per_atom.u32"].reshape(3, -1), per_atom[7:10])
    assert np.array_equal(cpp["contacts.hist_one.hist.u64"], TC.numpy_hist(d[int(off[8]):int(off[9])], W.CT_CUT, 5))
    assert np.array_equal(cpp["contacts.count_only.n.u64"], cpp["contacts.all.n.u64"][:3])
    for f in range(3):
        assert O.pairs_within(fr[f], W.GROUPS["oxy"], W.GROUPS["oxy"], bx[f], W.CT_CUT_NONE)[0].size == 0
    assert not cpp["contacts.none.n.u64"].any() and cpp["contacts.none.offsets.u64"].tolist() == [0, 0, 0, 0]


# ------------------------------------------------------------------ RmsdPanel
def test_rmsd_panel(cpp, py, world):
    same_as_python(cpp, py, "rmsd.")
    fr, bx, m, idx = world["frames"], world["boxes"], world["masses"], W.GROUPS["rng"]

    def oracle_status(f):
        try:
            O.calc_rmsd(fr[f], m, idx, bx[f], fr[f], m, idx, bx[f])
            return 0
        except O.OracleError as e:
            return e.status

    row_slots, col_slots = list(range(NS)), [7, 8, 9, 2]
    st = [oracle_status(f) for f in range(NS)]
    assert st == expected_status().tolist()
    assert cpp["rmsd.rows.append.i32"].tolist() == st == cpp["rmsd.rows.status.i32"].tolist() and cpp["rmsd.cols.status.i32"].tolist() == [st[f] for f in col_slots]
    for name, rs, cs in (("self", row_slots, row_slots), ("rows_cols", row_slots, col_slots), ("cols_rows", col_slots, row_slots)):
        got = cpp["rmsd.%s.matrix.f32" % name].reshape(len(rs), len(cs))
        ok_r, ok_c = [k for k, f in enumerate(rs) if st[f] == 0], [k for k, f in enumerate(cs) if st[f] == 0]
        want = rmsd_matrix_ref.oracle_matrix([fr[rs[k]] for k in ok_r], [bx[rs[k]] for k in ok_r], [fr[cs[k]] for k in ok_c], [bx[cs[k]] for k in ok_c], m, idx)
        valid = np.zeros(got.shape, bool); valid[np.ix_(ok_r, ok_c)] = True
        assert np.isnan(got[~valid]).all() and not np.isnan(got[valid]).any()
        err = np.abs(got[np.ix_(ok_r, ok_c)] - want).max()
        print("rmsd %s: max |error| %.3g nm" % (name, err))
        assert err <= rmsd_matrix_ref.TOL and want.max() > 0.01


# ------------------------------------------------------------------ Fluctuations
def _fluct(cpp, name, S):
    g = lambda field: cpp["fluct.%s.%s" % (name, field)]
    return (g("origin.f32").reshape(S, 3), g("sum.f64").reshape(S, 3), g("sumsq.f64").reshape(S, 3), int(g("n.u64")[0]),
            g("mean.f64").reshape(S, 3), g("variance.f64").reshape(S, 3), g("rmsf.f64"))


def test_fluctuations(cpp, py, world):
    same_as_python(cpp, py, "fluct.")
    R, fr, idx = fluct_ref, world["frames"], W.GROUPS["rng"]
    S = idx.size
    full, part = R.State(S), R.State(S)
    st, _ = full.accumulate(fr, idx)
    assert cpp["fluct.all.status.i32"].tolist() == st.tolist() == expected_status(needs_box=False).tolist()
    part.accumulate(fr[7:10], idx); part.accumulate(fr[2:3], idx)
    for name, ref, used in (("all", full, fr), ("part", part, fr[7:10] + fr[2:3])):
        o, s, q, n, mean, var, rmsf = _fluct(cpp, name, S)
        assert n == ref.n and R.same_bits(o, ref.o) and R.same_bits(s, ref.s) and R.same_bits(q, ref.q)              # the raw state: bit for bit
        m2, v2, r2 = R.two_pass(used, idx)
        assert np.abs(mean - m2).max() <= TF.TOL and np.abs(var - v2).max() <= TF.TOL and np.abs(rmsf - r2).max() <= TF.TOL
        cm, cv, cr = ref.close()
        assert np.abs(mean - cm).max() <= CLOSING and np.abs(var - cv).max() <= CLOSING and np.abs(rmsf - cr).max() <= CLOSING
        assert rmsf.mean() > 1e-3                                                   # (the frames do move)
    full.merge(part)
    o, s, q, n, mean, var, rmsf = _fluct(cpp, "merged", S)
    assert n == full.n == NS - 1 + 4 and R.same_bits(o, full.o) and np.abs(s - full.s).max() <= MERGED and np.abs(q - full.q).max() <= MERGED
    m2, v2, r2 = R.two_pass(fr + fr[7:10] + fr[2:3], idx)
    assert np.abs(mean - m2).max() <= TF.TOL and np.abs(var - v2).max() <= TF.TOL and np.abs(rmsf - r2).max() <= TF.TOL
    # store_mean: the mean rounded to f32 in the group's atoms, nothing else of the slot touched
    stored, want = cpp["fluct.merged.stored.f32"].reshape(N, 3), np.zeros((N, 3), F)
    want[idx] = mean.astype(F)
    assert R.same_bits(stored, want)
    o, s, q, n, mean, var, rmsf = _fluct(cpp, "cleared", S)
    assert n == 0 and np.isnan(mean).all() and np.isnan(var).all() and np.isnan(rmsf).all()


# ------------------------------------------------------------------ Covariance
class _Stored:
    """the arrays of one read-out in the form test_gpu_covar.within_bounds takes a Covariance object"""

    def __init__(self, cpp, name, S):
        g = lambda field: cpp["covar.%s.%s" % (name, field)]
        D = 3 * S
        self.n_atoms, self.n_frames = S, int(g("n.u64")[0])
        self._raw = (g("origin.f32").reshape(S, 3), g("sum.f64").reshape(S, 3), g("Q.f64").reshape(D, D), self.n_frames)
        self.mean, self.cov, self.cov_mw, self.corr = g("mean.f64").reshape(S, 3), g("cov.f64").reshape(D, D), g("cov_mw.f64").reshape(D, D), g("dccm.f64").reshape(S, S)

    def raw(self):
        return self._raw


def test_covariance(cpp, py, world):
    same_as_python(cpp, py, "covar.")
    R, fr, idx = covar_ref, world["frames"], W.GROUPS["lst"]
    S = idx.size
    assert 3 * S + 1 > 64                                                           # Q spans more than one stored block
    full, part = R.State(S), R.State(S)
    st, _ = full.accumulate(fr, idx)
    assert cpp["covar.all.status.i32"].tolist() == st.tolist() == expected_status(needs_box=False).tolist()
    part.accumulate(fr[7:10], idx); part.accumulate(fr[2:3], idx)
    rm = np.sqrt(np.repeat(world["masses"][idx].astype(np.float64), 3))
    checks = [("all", full, fr, 0.0), ("part", part, fr[7:10] + fr[2:3], 0.0)]
    for name, ref, used, extra in checks + [("merged", None, fr + fr[7:10] + fr[2:3], MERGED_ULPS)]:
        if ref is None:
            full.merge(part); ref = full
        got = _Stored(cpp, name, S)
        TV.within_bounds(got, ref, extra=extra)                                     # o and n exactly, s and Q within the rounding bounds, Q == Q.T
        o, s, Q, n = got.raw()
        cm, cc = R.close(o, s, Q, n)                                                # the closing step, applied to the device's own raw state
        assert TV.ulps(got.mean, cm).max() <= 2 and TV.ulps(got.cov, cc).max() <= 2
        assert TV.ulps(got.cov_mw, got.cov * np.outer(rm, rm)).max() <= 2 and not np.array_equal(got.cov_mw, got.cov)
        m2, c2, sd = R.two_pass(used, idx)
        assert (np.abs(got.cov - c2) / np.outer(sd, sd)).max() <= TV.REL and np.abs(got.mean - m2).max() <= 1e-6
        assert np.array_equal(got.cov, got.cov.T)
        rc = R.dccm(R.close(ref.o, ref.s, ref.Q, ref.n)[1])
        assert np.abs(got.corr - rc).max() <= CLOSING and np.array_equal(got.corr, got.corr.T)
    got = _Stored(cpp, "cleared", S)
    assert got.n_frames == 0 and np.isnan(got.mean).all() and np.isnan(got.cov).all() and np.isnan(got.cov_mw).all() and np.isnan(got.corr).all()
