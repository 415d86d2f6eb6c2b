"""A call's result does not depend on what its context did before.

tests/history_world.py builds one world and a table of call kinds over every family of the library (centres, RMSD, pair distances,
topology with gyration, trajectory I/O, failing calls, redefinitions, and "series": RMSDPanel, Fluctuations, Covariance, MSD, Internals,
VectorCorrelation on long-lived objects).  Every kind runs on two fresh worlds of its own: those two results must
agree, bit for bit wherever the project documents determinism (everything but the RMSD calls); an RMSD kind whose fresh results differ
is held to the margins of tests/test_gpu_resident.py (RMSD 2e-6 nm, fitted coordinates 2e-5 nm; rotation elements 2e-6 as in
tests/test_gpu_rmsd_fast.py) from then on.  The fresh result is checked once against the reference the suite uses for that call.
Then ONE long-lived world walks the mandatory adjacencies (each behind a shortcut of the library: an elided reset, a shared
sequence word, a grow-only buffer, a cache; 11-19 behind those of the series objects and gyration: the verdict block and its tail,
the context's state words behind a panel append, the epoch check, group snapshots, the words gyration shares with centers, the
grow-only gyration block, the band scratch, rewritten slots, device ingest) and two seeded schedules, and every step must give its
kind's fresh result.  The series kinds are compared as their objects' own suites compare (cited where used): bit for bit for the
Fluctuations and Internals sums, MSD displacements and VectorCorrelation vectors inside the cell, within the reference modules'
derived bounds elsewhere.  (test_gpu_internals.py holds `values` to internals_ref.bounds of the f64 values, not to values32's bits:
so does this file.)"""
import itertools
import os
import time
import traceback

import numpy as np
import pytest

import covar_ref
import fluct_ref
import gridmap_ref
import gyration_ref
import hbond_ref
import history_world as HW
import internals_ref
import msd_ref
import oracle_lib as O
import rmsd_matrix_ref
import vcorr_ref
import whole_ref

pytestmark = pytest.mark.gpu
F = np.float32
TOL_RMSD, TOL_FIT, TOL_ROT = 2e-6, 2e-5, 2e-6            # between two runs of the library (test_gpu_resident.py, test_gpu_rmsd_fast.py)
REF_CENTRE, REF_RMSD, REF_FIT, REF_DIST = 1e-5, 1e-5, 5e-5, 1e-5     # against the oracle (test_gpu_masked_selections.py, test_gpu_pairdist.py, smoke)
REF_ROT = 1e-5           # rotation elements against the oracle: the fitted coordinates' 5e-5 nm over the 5 nm an atom lies from the centre at the most
E_NO_BOX, E_NO_POSITION, E_UNSUPPORTED_BOX = HW.E_NO_BOX, HW.E_NO_POSITION, HW.E_UNSUPPORTED_BOX


@pytest.fixture(scope="module")
def G():
    import groan_rs_amd as g
    return g


# ------------------------------------------------------------------ comparing two results
def may_differ(name):
    """kinds with an RMSD in them: the only ones whose determinism the project does not document"""
    return HW.META[name]["family"] == "rmsd" or name in ("fail_redefined_small_plan", "restored_small_plan", "tune_masked0")


def _tolerance(name, label):
    if not may_differ(name):
        return 0.0
    if label.startswith("pos"): return TOL_FIT
    if label.startswith("r"): return TOL_RMSD
    if label == "R": return TOL_ROT
    return 0.0


def difference(name, got, want, exact):
    """None, or (label, what) of the first entry of `got` that is not `want`'s: bit for bit when `exact`, else within the RMSD margins"""
    if sorted(got) != sorted(want):
        return "keys", (sorted(got), sorted(want))
    for label in sorted(want):
        a, b = got[label], want[label]
        if isinstance(b, np.ndarray) or isinstance(b, np.generic):
            a, b = np.asarray(a), np.asarray(b)
            if a.shape != b.shape or a.dtype != b.dtype:
                return label, "shape %r %s, expected %r %s" % (a.shape, a.dtype, b.shape, b.dtype)
            if np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8)):
                continue
            tol = 0.0 if exact else _tolerance(name, label)
            if a.dtype.kind == "f":
                nan = np.isnan(a)
                with np.errstate(invalid="ignore"):
                    d = np.abs(a.astype(np.float64) - b.astype(np.float64))
                worst = float(np.nanmax(d)) if d.size and not np.isnan(d).all() else 0.0
                if np.array_equal(nan, np.isnan(b)) and worst <= tol:
                    continue
                return label, "%d of %d values differ, largest difference %.3g (allowed %.3g), first at %r" % (
                    int((a != b).sum()), a.size, worst, tol, tuple(int(v) for v in np.argwhere(a != b)[0]))
            return label, "%d of %d values differ, first at %r" % (int((a != b).sum()), a.size, tuple(int(v) for v in np.argwhere(a != b)[0]))
        elif a != b:
            return label, "%r, expected %r" % (a, b)
    return None


# ------------------------------------------------------------------ fresh results: computed once
class Fresh:
    def __init__(self):
        self.result, self.exact, self.second_differs, self.seconds = {}, {}, {}, 0.0


@pytest.fixture(scope="module")
def fresh(G, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("history")
    fr = Fresh()
    t0 = time.time()
    for name in sorted(HW.KINDS):
        res = []
        for k in range(2):
            w = HW.make_world(G, tmp)
            res.append(HW.KINDS[name](w))
            w.close()
        fr.result[name] = res[0]
        d = difference(name, res[1], res[0], exact=True)
        fr.exact[name] = d is None
        if d is not None:
            fr.second_differs[name] = (d, difference(name, res[1], res[0], exact=False))
    fr.seconds = time.time() - t0
    print("history: %d kinds on two fresh worlds each in %.1f s" % (len(HW.KINDS), fr.seconds))
    return fr


def test_fresh_contexts_agree(fresh):
    for name, (bits, within) in sorted(fresh.second_differs.items()):
        print("history: two fresh contexts differ in %s: %s: %s" % (name, bits[0], bits[1]))
    wrong = {n: d for n, d in fresh.second_differs.items() if not may_differ(n) or d[1] is not None}
    assert not wrong, wrong
    for name, meta in HW.META.items():
        r = fresh.result[name]
        if meta["lean"]:                                     # a forced resident launch over good frames is lean, on a fresh context already
            assert r["lean"] == 1 and r["launches"] == 1, (name, r["lean"], r["launches"])
        if meta["failing"]:
            assert r["raised"] is not None or (np.asarray(r.get("st", 0)) != 0).any(), name
        else:
            assert r["raised"] is None and ("st" not in r or (np.asarray(r["st"]) == 0).all()), (name, r["raised"])


# ------------------------------------------------------------------ the long-lived world
def _brief(st):
    return None if st is None else np.asarray(st).ravel()[:16].tolist()


def _walk(G, tmp, fresh, names):
    w = HW.make_world(G, tmp)
    try:
        done = []
        for step, name in enumerate(names):
            got = HW.KINDS[name](w)
            d = difference(name, got, fresh.result[name], exact=fresh.exact[name])
            assert d is None, "step %d, kind %s, behind %s: %s: %s (statuses %s, fresh %s; raised %s, fresh %s)" % (
                step, name, done[-3:], d[0], d[1], _brief(got.get("st")), _brief(fresh.result[name].get("st")), got.get("raised"), fresh.result[name].get("raised"))
            if HW.META[name]["lean"]:                        # a forced resident launch over good frames: it started, and no state was zeroed or uploaded for it
                assert got["launches"] == 1 and got["lean"] == 1, (step, name, got["launches"], got["lean"])
            done.append(name)
        for key in ("res_aborts", "res_handshake_misses", "res_sync_fallbacks", "small_sync_fallbacks"):
            assert w.s.stat(key) == 0, (key, w.s.stat(key))
    finally:
        w.close()


@pytest.mark.parametrize("k", sorted(HW.ADJACENCIES))
def test_history_adjacencies(G, fresh, tmp_path, k):
    _walk(G, tmp_path, fresh, HW.ADJACENCIES[k])


@pytest.mark.parametrize("seed", [0, 1])
def test_history_schedule(G, fresh, tmp_path, seed):
    t0 = time.time()
    names = HW.schedule(seed)
    _walk(G, tmp_path, fresh, names)
    print("history: schedule %d, %d steps in %.1f s" % (seed, len(names), time.time() - t0))


# ------------------------------------------------------------------ the fresh results against the suite's references
def _lattice_error(got, want, box):
    """largest component of got - want after taking off the nearest lattice vector (an atom or a centre on a cell face may come out on either side)"""
    H = HW.cell(box)
    d = np.asarray(got, np.float64) - np.asarray(want, np.float64)
    d -= np.round(d @ np.linalg.inv(H)) @ H
    return float(np.abs(d).max()) if d.size else 0.0


def _idx(name):
    return HW.host_world()["groups"][name].astype(np.uint64)


def _centre(pos, box, group, kind, weighted):
    m = HW.host_world()["masses"] if weighted else None
    if kind == HW.NAIVE: return O.center_naive(pos, _idx(group), m)
    if kind == HW.ESTIMATE: return O.estimate_center(pos, _idx(group), box, m)
    return O.get_center(pos, _idx(group), box, m)


def _check_centres(fresh, h):
    for g, (kind, wt) in itertools.product(("small", "big", "masked"), HW.CENTRES):
        one, many = fresh.result["center_%s_%d%d" % (g, kind, wt)], fresh.result["center_batch_%s_%d%d" % (g, kind, wt)]
        assert one["raised"] is None and many["raised"] is None and (many["st"] == 0).all()
        for f in range(16):
            want = _centre(h["frames"][f], h["boxes"][f], g, kind, wt)
            err = np.abs(many["c"][f] - want).max() if kind == HW.NAIVE else _lattice_error(many["c"][f], want, h["boxes"][f])
            assert err <= REF_CENTRE, (g, kind, wt, f, err)
            if f in (3, 11):
                assert np.array_equal(one["c%d" % f].view(np.uint32), many["c"][f].view(np.uint32)) or np.abs(one["c%d" % f] - many["c"][f]).max() <= REF_CENTRE, (g, kind, wt, f)
    r = fresh.result["group_distance"]
    for label, slot, dim, other in (("d", 3, "xyz", "b400"), ("dxy", 11, "xy", "big")):
        a, b = (O.get_center(h["frames"][slot], _idx(g), h["boxes"][slot]) for g in ("small", other))
        assert abs(float(r[label]) - O.distance(a, b, dim, h["boxes"][slot])) <= 2 * REF_CENTRE, label


def _check_moves(fresh, h):
    big, masses = _idx("big"), h["masses"]
    def each(name, slots, fn, tol=TOL_FIT):
        r = fresh.result[name]
        assert r["raised"] is None and ("st" not in r or (np.asarray(r["st"]) == 0).all()), name
        for f in slots:
            want = fn(h["frames"][f], h["boxes"][f])
            assert _lattice_error(r["pos%d" % f], want, h["boxes"][f]) <= tol, (name, f)
            assert np.array_equal(r["box%d" % f][:3], np.asarray(h["boxes"][f][:3], F)), (name, f)
    for rows in ("ortho_rows1", "ortho_rows0", "tric"):
        slots = HW.TRIC8 if rows == "tric" else HW.ORTHO8
        each("translate_batch_" + rows, slots, lambda x, b: O.translate(x, big, [1.7, -2.9, 0.45], b))
        each("wrap_batch_" + rows, slots, lambda x, b: O.wrap_atoms(x, big, b))
    each("group_translate_small", (3,), lambda x, b: O.translate(x, _idx("small"), [4.0, -7.0, 0.3], b))
    each("group_wrap_all", (3,), lambda x, b: O.wrap_atoms(O.translate(x, _idx("all"), [-0.4, 0.3, 9.0], b), _idx("all"), b))
    each("atoms_center_small", (3,), lambda x, b: O.atoms_center(x, _idx("small"), "xyz", b))
    each("atoms_center_mass_big", (11,), lambda x, b: O.atoms_center(x, big, "xy", b, mass=masses))
    for name in ("atoms_center_batch_res", "atoms_center_batch_two"):
        each(name, HW.ORTHO8, lambda x, b: O.atoms_center(x, big, "xyz", b))
    for name in ("atoms_center_mass_batch_res", "atoms_center_mass_batch_two"):
        each(name, HW.TRIC8, lambda x, b: O.atoms_center(x, big, "xyz", b, mass=masses))
    for a, b in (("atoms_center_batch_res", "atoms_center_batch_two"), ("atoms_center_mass_batch_res", "atoms_center_mass_batch_two")):
        for label in fresh.result[a]:                                         # (test_gpu_center_resident.py: the one pass gives the two passes' bits)
            if label.startswith("pos"):
                assert np.array_equal(fresh.result[a][label].view(np.uint32), fresh.result[b][label].view(np.uint32)), (a, label)
        assert fresh.result[b]["launches"] == 0


def _check_rmsd(fresh, h):
    m, ref = h["masses"], h["frames"][HW.REF_SLOT]
    want = {}
    def oracle(group, f):
        if (group, f) not in want:
            i = _idx(group)
            want[(group, f)] = O.calc_rmsd_and_fit(ref, m, i, HW.BOX, h["frames"][f], m, i, h["boxes"][f])
        return want[(group, f)]
    with O.acc64():
        r = fresh.result["calc_rmsd_small"]
        assert r["raised"] is None and abs(float(r["r"]) - oracle("small", 3)[0]) <= REF_RMSD
        i = _idx("small")
        assert np.abs(r["R"] - O.calc_rmsd(ref, m, i, HW.BOX, h["frames"][3], m, i, HW.BOX)[1]).max() <= REF_ROT
        r = fresh.result["calc_rmsd_fit_small"]
        assert abs(float(r["r"]) - oracle("small", 11)[0]) <= REF_RMSD and np.abs(r["pos11"] - oracle("small", 11)[1]).max() <= REF_FIT
        for g in ("all", "big", "masked", "listbig"):
            r = fresh.result["plan_rmsd_%s" % g]
            assert r["raised"] is None and (r["st"] == 0).all()
            for f in range(16):
                assert abs(float(r["r"][f]) - oracle(g, f)[0]) <= REF_RMSD, (g, f)
            for f in (0, 7, 8, 15):                                             # the rotations, at both ends of both cells
                i = _idx(g)
                assert np.abs(r["R"][f] - O.calc_rmsd(ref, m, i, HW.BOX, h["frames"][f], m, i, h["boxes"][f])[1]).max() <= REF_ROT, (g, f)
            for fuse in (0, 1):
                r = fresh.result["plan_fit_%s_fuse%d" % (g, fuse)]
                assert r["raised"] is None and (r["st"] == 0).all()
                for f in range(16):
                    assert abs(float(r["r"][f]) - oracle(g, f)[0]) <= REF_RMSD, (g, fuse, f)
                    assert np.abs(r["pos%d" % f] - oracle(g, f)[1]).max() <= REF_FIT, (g, fuse, f)
        for nf in (3, 9, 2):
            r = fresh.result["res_fit_%d" % nf]
            assert r["raised"] is None and (r["st"] == 0).all()
            for f in range(nf):
                assert abs(float(r["r"][f]) - oracle("all", f)[0]) <= REF_RMSD and np.abs(r["pos%d" % f] - oracle("all", f)[1]).max() <= REF_FIT, (nf, f)
        r = fresh.result["plan_begin_end"]
        for f in range(8):
            assert abs(float(r["r"][f]) - oracle("big", f)[0]) <= REF_RMSD and np.abs(r["pos%d" % f] - oracle("big", f)[1]).max() <= REF_FIT, f
        # the mixed batch: the good frames are fitted, the others untouched
        r = fresh.result["fail_fit_mixed_fused"]
        assert r["st"].tolist() == [0, 0, E_NO_BOX, 0, 0, E_NO_POSITION, 0, 0, 0]
        for f in range(9):
            if f in (2, 5):
                assert np.array_equal(np.nan_to_num(r["pos%d" % f], nan=-1.0), np.nan_to_num(HW.nan_frame(f, 4321) if f == 5 else h["frames"][f], nan=-1.0)) and np.isnan(r["r"][f])
            else:
                assert abs(float(r["r"][f]) - oracle("all", f)[0]) <= REF_RMSD and np.abs(r["pos%d" % f] - oracle("all", f)[1]).max() <= REF_FIT, f
        r = fresh.result["restored_small_plan"]
        assert abs(float(r["r"][0]) - oracle("small", 3)[0]) <= REF_RMSD and abs(float(r["r11"][0]) - oracle("small", 11)[0]) <= REF_RMSD


def _check_pairs(G, fresh, h, aux):
    r = fresh.result["atoms_distance"]
    want = [O.distance(h["frames"][3][3], h["frames"][3][11777], "xyz", HW.BOX), O.distance(h["frames"][11][0], h["frames"][11][HW.N - 1], "xyz", HW.TRIC),
            O.distance(h["frames"][11][5000], h["frames"][11][77], "yz", HW.TRIC)]
    assert np.abs(r["d"] - np.array(want, F)).max() <= REF_DIST
    for name, g1, g2, f in (("alldist_40x50", "a40", "b50", 3), ("alldist_300x400", "a300", "b400", 11), ("alldist_small_self", "small", "small", 3),
                            ("tune_pairsym0", "small", "small", 3), ("iter_all_distances", "a40", "list", 11)):
        want = O.group_all_distances(h["frames"][f], _idx(g1), _idx(g2), "xyz", h["boxes"][f])
        assert fresh.result[name]["raised"] is None and np.abs(fresh.result[name]["d"] - want).max() <= REF_DIST, name
    assert np.array_equal(fresh.result["tune_pairsym0"]["d"], fresh.result["alldist_small_self"]["d"])      # (test_gpu_pairdist_self.py: the bits of the plain kernel)
    d = fresh.result["alldist_masked_self"]["d"]
    rows = np.arange(0, 5000, 79)                                               # 64 rows of the 5 000 against the oracle, the matrix against its transpose
    want = O.group_all_distances(h["frames"][11], _idx("masked")[rows], _idx("masked"), "xyz", HW.TRIC)
    assert d.shape == (5000, 5000) and np.abs(d[rows] - want).max() <= REF_DIST and np.array_equal(d, d.T)
    r = fresh.result["alldist_batch_device_40x50"]
    assert (r["st"] == 0).all()
    for k, f in enumerate((6, 7, 8, 9)):
        assert np.abs(r["d"][k] - O.group_all_distances(h["frames"][f], _idx("a40"), _idx("b50"), "xyz", h["boxes"][f])).max() <= REF_DIST, f
    # the reducers: equal to the reduction of the full matrices (test_gpu_pairdist_reduce.py), which are the oracle's
    full = np.stack([aux.s.group_all_distances("a300", "b400", slot=f) for f in (6, 7, 8, 9)])
    for k, f in enumerate((6, 7, 8, 9)):
        assert np.abs(full[k] - O.group_all_distances(h["frames"][f], _idx("a300"), _idx("b400"), "xyz", h["boxes"][f])).max() <= REF_DIST
    assert np.array_equal(fresh.result["reduce_max"]["v"][:, 0], full.max(axis=(1, 2)))
    assert np.array_equal(fresh.result["reduce_min_rows"]["v"], full.min(axis=2))
    assert np.array_equal(fresh.result["reduce_count_rows"]["v"], (full < F(1.5)).sum(axis=2).astype(np.uint64))
    s = F(97) / F(3.0)                                                          # bin = (uint32)(d * s), counted iff d >= 0 and d * s < nbins (groan_hip.h)
    t = (full * s).astype(F)
    hist = np.stack([np.bincount(t[k][(full[k] >= 0) & (t[k] < F(97))].astype(np.uint32), minlength=97) for k in range(4)])
    assert hist.sum() > 100_000 and np.array_equal(fresh.result["reduce_hist"]["v"], hist.astype(np.uint64))
    r = fresh.result["pairs_within"]
    i, j, d = O.pairs_within(h["frames"][3], _idx("small"), _idx("big"), HW.BOX, 0.9)
    assert len(i) > 1000 and np.array_equal(r["i"], i.astype(np.uint32)) and np.array_equal(r["j"], j.astype(np.uint32)) and np.abs(r["d"] - d).max() <= REF_DIST
    r = fresh.result["geometries_small_all_small"]
    spec = [dict(kind="sphere", position=[0.3, 0.2, 0.2], radius=1.4)]
    for k, src in enumerate(("small", "all", "small")):
        want = O.group_from_geometries(h["frames"][3], _idx(src), HW.BOX, spec)
        got = np.concatenate([np.arange(a, b + 1) for a, b in r["blocks%d" % k]]) if len(r["blocks%d" % k]) else np.zeros(0)
        assert len(want) > 10 and np.array_equal(got, want), (k, len(got), len(want))
    assert np.array_equal(r["blocks0"], r["blocks2"])
    # Contacts: the per-slot call, bit for bit (test_gpu_contacts.py)
    def slot_pairs(f):
        return aux.s.group_pairs_within("oxy", "hyd", HW.CT_CUTOFF, slot=f)
    r = fresh.result["contacts_pairs_8"]
    assert r["raised"] is None and (r["st"] == 0).all() and r["off"].size == 9 and np.array_equal(np.diff(r["off"]), r["n"])
    for f in range(8):
        a, b = int(r["off"][f]), int(r["off"][f + 1])
        i, j, d = slot_pairs(f)
        assert i.size >= 2 * HW.N_MOL and np.array_equal(r["i"][a:b], i) and np.array_equal(r["j"][a:b], j) and np.array_equal(r["d"][a:b].view(np.uint32), d.view(np.uint32)), f
    r = fresh.result["contacts_hist_tric_8"]
    s = F(HW.CT_BINS) / F(HW.CT_CUTOFF)                                         # bin = (uint32)(d * s), counted iff d * s < nbins (groan_hip.h)
    for k, f in enumerate(HW.TRIC8):
        t = (slot_pairs(f)[2] * s).astype(F)
        want = np.bincount(t[t < F(HW.CT_BINS)].astype(np.uint32), minlength=HW.CT_BINS).astype(np.uint64)
        assert want.sum() >= 2 * HW.N_MOL and np.array_equal(r["h"][k], want), f
    r = fresh.result["contacts_counts_1"]
    i, j, d = slot_pairs(11)
    assert np.array_equal(r["per_atom"][0], np.bincount(i // 3, minlength=HW.N_MOL).astype(np.uint32)) and int(r["n"][0]) == i.size      # oxygen k is atom 3 k
    # Region: the geometry selection, frame by frame (test_gpu_region.py)
    r = fresh.result["region_select_16"]
    assert r["raised"] is None and (r["st"] == 0).all() and np.array_equal(np.diff(r["off"]), r["n"])
    for f in range(16):
        want = O.group_from_geometries(h["frames"][f], _idx("all"), h["boxes"][f], HW.REGION_SPECS)
        assert len(want) > 100 and np.array_equal(r["atoms"][int(r["off"][f]):int(r["off"][f + 1])], want), (f, int(r["n"][f]), len(want))
    r = fresh.result["region_anchored_8"]
    assert r["raised"] is None and (r["st"] == 0).all() and (r["cst"] == 0).all() and r["anchors"].dtype == F
    for k, f in enumerate(range(4, 12)):
        assert _lattice_error(r["anchors"][k], O.get_center(h["frames"][f], _idx("small"), h["boxes"][f]), h["boxes"][f]) <= REF_CENTRE, f
        specs = [dict(sp, position=[float(v) for v in (np.asarray(sp["position"], F) + r["anchors"][k]).astype(F)]) for sp in HW.REGION_SPECS]     # stored + anchor in float32
        want = O.group_from_geometries(h["frames"][f], _idx("big"), h["boxes"][f], specs)
        assert len(want) > 100 and np.array_equal(r["atoms"][int(r["off"][k]):int(r["off"][k + 1])], want), (f, int(r["n"][k]), len(want))


def _check_topology(G, fresh, h):
    nbrs = whole_ref.neighbours(HW.N, h["bonds"])
    refs, orders = whole_ref.molecules(nbrs)
    ref_of = whole_ref.ref_of(HW.N, refs, orders)
    r = fresh.result["whole_mols"]
    assert r["raised"] is None and (r["st"] == 0).all()
    for f in range(16):
        got = r["pos%d" % f]
        if f < 8:                                                               # (test_gpu_whole.py: the reference's arithmetic, bit for bit)
            want, bad = whole_ref.make_molecules_whole(h["frames"][f], HW.BOX, ref_of, orders)
            assert bad is None and np.array_equal(got.view(np.uint32), want.view(np.uint32)), f
        else:                                                                   # triclinic: whole, and every atom a lattice image of itself
            assert np.linalg.norm(got - np.repeat(got[0::3], 3, axis=0), axis=1).max() <= 0.2, f
            assert _lattice_error(got, h["frames"][f], HW.TRIC) <= REF_CENTRE, f
    r = fresh.result["rebond_whole"]
    assert r["raised"] is None and r["no_bonds"] == 0 and (r["st"] == 0).all()
    nb_alt = whole_ref.neighbours(HW.N, h["bonds_alt"])
    refs_a, orders_a = whole_ref.molecules(nb_alt)
    ref_a = whole_ref.ref_of(HW.N, refs_a, orders_a)
    for f in range(8):
        want, bad = whole_ref.make_molecules_whole(h["frames"][f], HW.BOX, ref_a, orders_a)
        assert np.array_equal(r["pos%d" % f].view(np.uint32), want.view(np.uint32)), f
    r = fresh.result["whole_group_big"]
    assert (r["st"] == 0).all()
    big = _idx("big").astype(np.int64)
    other = np.setdiff1d(np.arange(HW.N), big)
    for f in range(16):
        got = r["pos%d" % f]
        assert np.array_equal(got[other], h["frames"][f][other]) and _lattice_error(got[big], h["frames"][f][big], h["boxes"][f]) <= REF_CENTRE, f
        if f < 8:                                                               # every atom the image nearest to the group's estimated centre
            c = O.estimate_center(h["frames"][f], _idx("big"), HW.BOX)
            assert (np.abs(got[big] - c) <= np.asarray(HW.BOX) / 2 + 1e-4).all(), f
    # segments: the oracle, segment by segment as a group
    lists = {"mol": [np.arange(3 * k, 3 * k + 3, dtype=np.uint64) for k in range(HW.N_MOL)],
             "resid": [np.arange(7 * k, min(7 * k + 7, HW.N), dtype=np.uint64) for k in range((HW.N + 6) // 7)]}
    with O.acc64():
        for which, (first, nf) in itertools.product(("mol", "resid"), ((7, 2), (4, 9), (11, 1))):
            r = fresh.result["seg_%s_%d" % (which, nf)]
            assert r["raised"] is None and (r["st"] == 0).all() and r["c"].shape == (nf, len(lists[which]), 3)
            for k in range(nf):
                f = first + k
                if nf == 9 and k not in (0, 4, 8):                               # (the frames of the batch of 9 are those of the other batches: three of them)
                    continue
                want = np.stack([O.get_center(h["frames"][f], l, h["boxes"][f], h["masses"]) for l in lists[which]])
                assert _lattice_error(r["c"][k], want, h["boxes"][f]) <= REF_CENTRE, (which, nf, f)
    r = fresh.result["fail_seg_nobox"]
    assert r["st"].tolist() == [0, E_NO_BOX, 0, 0] and np.isnan(r["c"][1]).all() and not np.isnan(r["c"][[0, 2, 3]]).any()
    # hydrogen bonds: the orthorhombic frames in full; the triclinic ones among the 800 molecules placed in pairs (the oracle's triclinic
    # all-pairs search over all oxygens takes 16 s a frame)
    nb = hbond_ref.bonded(h["bonds"], HW.N)
    full = hbond_ref.resolve_chain(h["groups"]["oxy"], h["groups"]["oxy"], h["groups"]["hyd"], nb)
    placed_o = 3 * np.sort(np.concatenate([h["donors"], h["donors"] + 1]))
    placed = hbond_ref.resolve_chain(placed_o, placed_o, h["groups"]["hyd"], nb)
    seen = {}
    for name, first, nf in (("hbond_2", 7, 2), ("hbond_8", 4, 8), ("hbond_1", 3, 1)):
        r = fresh.result[name]
        assert r["raised"] is None and (r["st"] == 0).all()
        for k in range(nf):
            f = first + k
            a, b = int(r["offsets"][k]), int(r["offsets"][k + 1])
            got = [(int(r["donor"][q]), int(r["hydrogen"][q]), int(r["acceptor"][q]), float(r["distance"][q]), float(r["angle"][q])) for q in range(a, b)]
            assert len(got) >= 100, (name, f, len(got))
            if f not in seen:
                want = hbond_ref.analyze(h["frames"][f], h["boxes"][f], [full if f < 8 else placed], [(0, 0)], HW.HB_DISTANCE, HW.HB_ANGLE)[(0, 0)]
                seen[f] = [(int(w[0]), int(w[1]), int(w[2]), float(w[3]), float(w[4])) for w in want]
            if f >= 8:
                inside = set(placed_o.tolist())
                got = [g for g in got if g[0] in inside and g[2] in inside]
            # (test_gpu_hbonds.py compare_hbonds: indices exact, distance and angle within 1e-3; a pair within that of a threshold may be on either side)
            edge = lambda g: abs(g[3] - HW.HB_DISTANCE) <= 1e-3 or abs(g[4] - HW.HB_ANGLE) <= 1e-3
            gk, wk = {g[:3]: g for g in got}, {g[:3]: g for g in seen[f]}
            assert all(edge(gk[key]) for key in set(gk) - set(wk)) and all(edge(wk[key]) for key in set(wk) - set(gk)), (name, f)
            assert all(hbond_ref.close(gk[key], wk[key]) for key in set(gk) & set(wk)), (name, f)
    r = fresh.result["gridmap"]
    ref = gridmap_ref.Map((0.0, 6.0), (0.0, 6.4), (0.25, 0.25))
    n_out, st, _ = ref.accumulate(h["frames"][:8], [HW.BOX] * 8, np.arange(HW.N), value=gridmap_ref.Z)
    assert r["raised"] is None and np.array_equal(r["outside"], n_out) and np.array_equal(r["st"], st)
    assert np.array_equal(r["counts"], ref.count) and np.array_equal(r["sums_q"], ref.sum_q) and np.array_equal(r["mean"].view(np.uint32), ref.mean().view(np.uint32))


def _check_gyration(fresh, h):
    t = HW.series_tuples()
    lists = {"mol": [np.arange(3 * k, 3 * k + 3) for k in range(HW.N_MOL)], "resid": [np.arange(7 * k, min(7 * k + 7, HW.N)) for k in range((HW.N + 6) // 7)],
             "sizes": [l.astype(np.int64) for l in t["sizes"]]}
    flat = {which: gyration_ref.flatten(l) for which, l in lists.items()}

    def frame(what, which, r, k, f, pos=None, box=None, axes=True):
        """frame k of the result r = slot f: the moments against the reference (gyration_ref's derived margin), the axes against the
        returned tensor, and their directions where the reference's eigenvalues stand apart (test_gpu_gyration.py; for `sizes` that
        is one axis per segment, test_history_schedule.py says which)"""
        pos, box = h["frames"][f] if pos is None else pos, h["boxes"][f] if box is None else box
        S_ref, margin = gyration_ref.reference(pos, box, h["masses"], flat[which], r["moments"][k, :, 0:3], HW.PBC, True)
        gyration_ref.check_moments(what, r["moments"][k], S_ref, margin)
        if axes:
            gyration_ref.check_axes(what, r["moments"][k], r["raw_axes"][k], S_ref)

    r = fresh.result["gyr_mol_9_axes"]
    assert r["raised"] is None and (r["st"] == 0).all() and r["moments"].shape == (9, HW.N_MOL, 10) and r["raw_axes"].shape == (9, HW.N_MOL, 12)
    assert np.array_equal(r["moments"][..., 0:3].view(np.uint32), fresh.result["seg_mol_9"]["c"].view(np.uint32))     # the centre is `centers`' own, bit for bit
    for k in range(9):                                                          # (the directions in three frames, both cells among them)
        frame("mol slot %d" % (4 + k), "mol", r, k, 4 + k, axes=k in (0, 4, 8))
    p = fresh.result["gyr_mol_9_pieces"]                                        # results do not depend on the piece size
    assert p["raised"] is None and all(np.array_equal(p[label].view(np.uint32), r[label].view(np.uint32)) for label in ("moments", "raw_axes", "st"))
    r = fresh.result["gyr_resid_2"]
    assert r["raised"] is None and (r["st"] == 0).all() and "raw_axes" not in r
    assert np.array_equal(r["moments"][..., 0:3].view(np.uint32), fresh.result["seg_resid_2"]["c"].view(np.uint32))
    for k in range(2):
        frame("resid slot %d" % (7 + k), "resid", r, k, 7 + k, axes=False)
    r = fresh.result["gyr_sizes_16_axes"]
    assert r["raised"] is None and (r["st"] == 0).all() and r["moments"].shape == (16, len(HW.SIZES), 10)
    assert (r["moments"][:, 0, 3:] == 0).all() and np.array_equal(r["raw_axes"][:, 0, 3:], np.broadcast_to(np.eye(3, dtype=F).ravel(), (16, 9)))    # one atom
    for k in range(16):
        frame("sizes slot %d" % k, "sizes", r, k, k)
        want = np.stack([O.get_center(h["frames"][k], l.astype(np.uint64), h["boxes"][k], h["masses"]) for l in lists["sizes"]])     # no `centers` kind runs on these segments
        assert _lattice_error(r["moments"][k, :, 0:3], want, h["boxes"][k]) <= REF_CENTRE, k
    d = fresh.result["gyr_sizes_device_4"]                                      # the device form: the host form's bits
    assert d["raised"] is None and (d["st"] == 0).all()
    assert np.array_equal(d["moments"].view(np.uint32), r["moments"][6:10].view(np.uint32)) and np.array_equal(d["raw_axes"].view(np.uint32), r["raw_axes"][6:10].view(np.uint32))
    # the mixed batch: a frame without box is NaN throughout, a missing position costs its own molecule only; the good frames are the good call's
    r, good = fresh.result["fail_gyr_mixed"], fresh.result["gyr_mol_9_axes"]
    assert r["raised"] is None and r["st"].tolist() == [0, E_NO_BOX, E_NO_POSITION, 0, 0]
    assert np.isnan(r["moments"][1]).all() and np.isnan(r["raw_axes"][1]).all()
    hit = np.zeros(HW.N_MOL, bool); hit[HW.NAN_BIG // 3] = True
    assert np.isnan(r["moments"][2][hit]).all() and np.isnan(r["raw_axes"][2][hit]).all() and not np.isnan(r["moments"][2][~hit]).any()
    for label in ("moments", "raw_axes"):
        assert np.array_equal(r[label][[0, 3, 4]].view(np.uint32), good[label][[0, 3, 4]].view(np.uint32)), label
        assert np.array_equal(r[label][2][~hit].view(np.uint32), good[label][2][~hit].view(np.uint32)), label


def _box9(box):
    b = np.zeros(9, F); b[:len(box)] = box
    return b


def _check_series(G, fresh, h):
    t = HW.series_tuples()
    frames, boxes = h["frames"], [_box9(b) for b in h["boxes"]]
    bits = fluct_ref.same_bits

    # -- Fluctuations: the raw state is the restatement's walk bit for bit, the closing within 1e-12 of its closing (test_gpu_fluct.py)
    def fluct_state(r, tag, group, fr):
        idx = h["groups"][group]
        ref = fluct_ref.State(len(idx))
        st, bad = ref.accumulate(fr, idx)
        assert r["n" + tag] == ref.n == r["n_frames" + tag], (group, tag)
        assert bits(r["origin" + tag], ref.o) and bits(r["sum" + tag], ref.s) and bits(r["sq" + tag], ref.q), (group, tag)
        mean, var, rmsf = ref.close()
        assert np.abs(r["mean" + tag] - mean).max() <= 1e-12 and np.abs(r["rmsf" + tag] - rmsf).max() <= 1e-12, (group, tag)
        return st
    for name, group, slots in (("fluct_small_8", "small", range(8)), ("fluct_masked_16", "masked", range(16)), ("fluct_list_tric_8", "list", range(8, 16)),
                               ("fluct_two_calls", "list", range(16))):
        r = fresh.result[name]
        assert r["raised"] is None and r["cleared_n"] == 0 and not r["cleared_origin"].any(), name
        assert np.array_equal(r["st"], fluct_state(r, "", group, [frames[f] for f in slots])), name
    r = fresh.result["fail_fluct_nan"]
    bad = [HW.nan_frame(4, HW.NAN_SMALL) if f == 4 else frames[f] for f in range(1, 9)]
    st = fluct_state(r, "", "small", bad)
    assert r["raised"] is None and np.array_equal(r["st"], st) and st.tolist() == [0, 0, 0, E_NO_POSITION, 0, 0, 0, 0] and r["n"] == 7
    fluct_state(r, "_without", "small", [frames[f] for f in (1, 2, 3, 5, 6, 7, 8)])
    for label in ("origin", "sum", "sq", "mean", "rmsf"):                        # the failed frame is counted for no atom
        assert bits(r[label], r[label + "_without"]), label

    # -- Covariance: origin and count exactly, sums within the bound of any summation order, the closings as test_gpu_covar.py holds them
    def ulps(a, b):
        with np.errstate(invalid="ignore"):
            return np.abs(a - b) / np.spacing(np.maximum(np.abs(a), np.abs(b)))
    def covar_state(r, group, fr):
        idx = h["groups"][group]
        ref = covar_ref.State(len(idx))
        st, bad = ref.accumulate(fr, idx)
        assert r["n"] == ref.n and bits(r["origin"].reshape(-1), ref.o), group
        assert (np.abs(r["q"] - ref.Q) <= ref.q_bound()).all() and (np.abs(r["sum"].reshape(-1) - ref.s) <= ref.s_bound()).all() and np.array_equal(r["q"], r["q"].T), group
        mean, cov = covar_ref.close(r["origin"], r["sum"], r["q"], r["n"])             # the library's closing step, applied to the device's own raw state
        assert ulps(r["mean"], mean).max() <= 2 and ulps(r["cov"], cov).max() <= 2, group
        rm = np.sqrt(np.repeat(h["masses"][idx].astype(np.float64), 3))
        assert ulps(r["cov_mw"], r["cov"] * np.outer(rm, rm)).max() <= 2, group
        want = covar_ref.dccm(covar_ref.close(ref.o, ref.s, ref.Q, ref.n)[1])
        assert np.abs(r["dccm"] - want).max() <= 1e-12 and np.array_equal(r["dccm"], r["dccm"].T), group
        return st
    for name, group, slots in (("covar_small_16", "small", range(16)), ("covar_a300_tric_8", "a300", range(8, 16))):
        r = fresh.result[name]
        assert r["raised"] is None and np.array_equal(r["st"], covar_state(r, group, [frames[f] for f in slots])), name
    r = fresh.result["fail_covar_all_bad"]
    assert r["raised"] is None and r["st"].tolist() == [E_NO_POSITION, E_NO_POSITION] and r["n_bad"] == 0 and not r["st_good"].any() and r["n"] == 4
    covar_state(r, "a300", [frames[f] for f in range(4, 8)])
    assert bits(r["origin"], frames[4][h["groups"]["a300"]])                     # the origin comes from the good call

    # -- MSD: the displacements are the restatement's walk bit for bit, the curves within msd_ref.msd_bound of the direct evaluation (test_gpu_msd.py)
    def msd_state(r, tag, group, dims, nojump, fr, bx, n_frames):
        idx = h["groups"][group]
        ref = msd_ref.Walk(len(idx), dims, nojump)
        st, bad = ref.append(fr, bx, idx)
        panel, S, n_pad = ref.panel(), len(idx), r["n_pad"]
        assert n_pad % 64 == 0 and 0 <= n_pad - S < 64 and len(panel) == n_frames
        assert bits(r["disp" + tag], panel), (group, tag)
        for label, lag in (("", None), ("3", 3)):
            msd, pairs = r["msd" + label + tag], r["pairs" + label + tag]
            want, wpairs, qsum = msd_ref.direct_msd(panel, ref.ok, lag, dtype=np.longdouble)
            assert np.array_equal(pairs, wpairs) and np.array_equal(np.isnan(msd), pairs == 0) and (not pairs[0] or (msd[0] == 0.0 and not np.signbit(msd[0])))
            have = pairs > 0
            assert (np.abs(msd[have] - want[have]) <= msd_ref.msd_bound(qsum, pairs, n_pad, S)[have]).all(), (group, tag, label)
        X = panel.reshape(len(panel), -1).astype(np.longdouble)
        q, ok = np.asarray((X * X).sum(1), np.float64), np.asarray(ref.ok, bool)
        fo = r["from_origin" + tag]
        assert np.isnan(fo[~ok]).all() and (np.abs(fo[ok] - q[ok] / S) <= 3 * n_pad * 2.0 ** -53 * q[ok] / S).all(), (group, tag)
        return st
    r = fresh.result["msd_small_ortho_8"]
    assert r["raised"] is None and np.array_equal(r["st"], msd_state(r, "", "small", "xyz", True, frames[0:8], boxes[0:8], 8)) and not r["st"].any()
    assert np.abs(r["disp"]).max() < 0.1                                         # (unwrapped: no jump of a box length is left)
    again = fresh.result["msd_appended_in_three"]                                # however the frames were cut into calls
    assert again["raised"] is None and all(bits(again[label], r[label]) for label in ("disp", "from_origin", "msd", "pairs", "msd3", "pairs3", "st"))
    r = fresh.result["msd_masked_tric_8"]
    assert r["raised"] is None and np.array_equal(r["st"], msd_state(r, "", "masked", "xy", False, frames[8:16], boxes[8:16], 8)) and not r["st"].any()
    assert not r["disp"][..., 2].any() and np.abs(r["disp"]).max() > 1.0          # (as the positions stand: the jumps are in)
    r = fresh.result["fail_msd_nobox"]
    st = msd_state(r, "", "small", "xyz", True, frames[0:4], [boxes[0], boxes[1], None, boxes[3]], 4)
    assert r["raised"] is None and np.array_equal(r["st"], st) and st.tolist() == [0, 0, E_NO_BOX, 0] and not r["disp"][2].any()
    r = fresh.result["fail_msd_capacity"]
    assert r["raised"] is None and r["st"].tolist() == [0] * 16 + [HW.LIB.E_INVALID_ARG] and r["refused"][0] == "DeviceError" and r["n_frames"] == 16
    msd_state(r, "_before", "small", "xyz", True, frames[0:8] + frames[0:8], boxes[0:8] + boxes[0:8], 16)
    for label in ("disp", "from_origin", "msd", "pairs", "msd3", "pairs3"):      # the refused call changed nothing
        assert bits(r[label], r[label + "_before"]), label

    # -- VectorCorrelation (test_gpu_vcorr.py): a vector inside the cell is the panel rule bit for bit, one that straddles it within the
    #    derived bound of the f64 minimum image; correlate_each is the chains over the device's own panel bit for bit, correlate within
    #    vcorr_ref.sum_bound of the long-double direct sum
    U = 2.0 ** -53
    pairs_t = t["pairs"].astype(np.int64)
    def vcorr_state(r, fr, bx):
        ref = vcorr_ref.Panels(pairs_t, unit=True, pbc=True)
        st, bad = ref.append(fr, bx)
        x, ok, V, n_pad = r["vectors"], np.asarray(ref.ok, bool), len(pairs_t), r["n_pad"]
        assert n_pad % 64 == 0 and 0 <= n_pad - V < 64 and x.shape == (len(fr), V, 3)
        coord = max(float(np.nanmax(np.abs(f))) for f in fr)
        for k in range(len(fr)):
            if not ok[k]:
                assert not x[k].any()
                continue
            raw = fr[k][pairs_t[:, 1]].astype(np.float64) - fr[k][pairs_t[:, 0]].astype(np.float64)
            d = vcorr_ref.vectors64(fr[k], pairs_t, bx[k], unit=False)
            straddle = np.abs(raw - d).max(1) > 0
            assert bits(x[k][~straddle], ref.rows[k][~straddle]), k
            shortest = float(np.sqrt((d * d).sum(1)).min())
            eps = vcorr_ref.unit_error(coord, shortest, steps=5.0, size=2.0 * coord, stored=False)
            assert np.abs(x[k].astype(np.float64) - vcorr_ref.vectors64(fr[k], pairs_t, bx[k])).max() <= eps, k
        assert bits(r["each1"], vcorr_ref.each(x, ok, 1, 4)) and bits(r["each2"], vcorr_ref.each(vcorr_ref.rank2(x), ok, 2, 4))
        want_pairs = vcorr_ref.pair_counts(ok)
        assert np.array_equal(r["pairs"], want_pairs)
        den, have = want_pairs.astype(np.float64) * V, want_pairs > 0
        for rank, got, panel in ((1, r["c1"], x), (2, r["c2"], vcorr_ref.rank2(x))):
            S, A = vcorr_ref.direct(panel, ok)
            want = vcorr_ref.close(np.asarray(S, np.float64), den, rank)
            assert np.array_equal(np.isnan(got), ~have)
            bound = vcorr_ref.sum_bound(A, want_pairs, panel.shape[2] * n_pad)[have] / den[have] * (1.5 if rank == 2 else 1.0) + 4 * U * (np.abs(want[have]) + 1.0)
            assert (np.abs(got[have] - want[have]) <= bound).all(), rank
        return st
    for name, lo in (("vcorr_ortho_8", 0), ("vcorr_tric_8", 8)):
        r = fresh.result[name]
        assert r["raised"] is None and np.array_equal(r["st"], vcorr_state(r, frames[lo:lo + 8], boxes[lo:lo + 8])) and not r["st"].any(), name
        assert abs(r["c1"][0] - 1.0) <= 9 * vcorr_ref.EPS32 and abs(r["c2"][0] - 1.0) <= 35 * vcorr_ref.EPS32
    r = fresh.result["fail_vcorr_nan"]
    st = vcorr_state(r, frames[0:2] + [HW.nan_frame(2, HW.NAN_SERIES), frames[3]], boxes[0:4])
    assert r["raised"] is None and np.array_equal(r["st"], st) and st.tolist() == [0, 0, E_NO_POSITION, 0] and r["pairs"].tolist() == [3, 1, 1, 1]

    # -- Internals (test_gpu_internals.py): the values within internals_ref.bounds of the f64 values, the accumulator the restatement's
    #    sums over the rows `values` returns, bit for bit
    tuples = {"distance": t["pairs"], "angle": t["angles"], "dihedral": t["dihedrals"]}
    def values(which, v, k, pos, box):
        bound = internals_ref.bounds(which, pos, tuples[which], box)
        err = internals_ref.error(which, v[k], internals_ref.values64(which, pos, tuples[which], box))
        assert bound.max() < 1e-3 and (err <= bound).all(), (which, k, float((err / bound).max()))
    for name, which, nf in (("internals_distance_16", "distance", 16), ("internals_angle_16", "angle", 16), ("internals_dihedral_8", "dihedral", 8)):
        r = fresh.result[name]
        assert r["raised"] is None and not r["st"].any() and r["v"].shape == (nf, len(tuples[which])) and r["v"].dtype == F, name
        for k in range(nf):
            values(which, r["v"], k, frames[k], boxes[k])
    def accumulated(r, which, rows):
        ref = internals_ref.State(which, len(tuples[which])).add(rows)
        assert r["n_" + which] == ref.n and bits(r["origin_" + which], ref.o) and bits(r["sum_" + which], ref.s) and bits(r["sq_" + which], ref.q), which
        mean, var = ref.close()
        assert np.abs(r["mean_" + which] - mean).max() <= 1e-12 and np.abs(r["var_" + which] - var).max() <= 1e-12, which
    r = fresh.result["internals_accumulate_16"]
    assert r["raised"] is None and not r["st"].any()
    accumulated(r, "angle", fresh.result["internals_angle_16"]["v"])
    assert bits(r["v_dihedral"][:8], fresh.result["internals_dihedral_8"]["v"])
    for k in range(8, 16):
        values("dihedral", r["v_dihedral"], k, frames[k], boxes[k])
    accumulated(r, "dihedral", r["v_dihedral"])
    r = fresh.result["fail_internals_nan"]
    assert r["raised"] is None and r["st"].tolist() == r["st_values"].tolist() == [0, E_NO_POSITION, 0] and np.isnan(r["v"][1]).all() and r["n_dihedral"] == 2
    for k, f in ((0, 4), (2, 6)):
        values("dihedral", r["v"], k, frames[f], boxes[f])
        assert bits(r["v"][k], fresh.result["internals_dihedral_8"]["v"][f])
    accumulated(r, "dihedral", r["v"])                                           # the failed frame is counted for no tuple

    # -- RMSDPanel: the oracle's matrix within 1e-5 nm (rmsd_matrix_ref.TOL, test_gpu_rmsd_matrix.py), the forms of one matrix bit for bit
    m = h["masses"]
    def matrix(got, group, rows, cols, what):
        idx = h["groups"][group].astype(np.uint64)
        want = rmsd_matrix_ref.oracle_matrix([frames[f] for f in rows], [h["boxes"][f] for f in rows], [frames[f] for f in cols], [h["boxes"][f] for f in cols], m, idx)
        assert got.shape == want.shape and got.dtype == F and np.abs(got - want).max() <= rmsd_matrix_ref.TOL, (what, float(np.abs(got - want).max()))
    r = fresh.result["panel_big_16"]
    assert r["raised"] is None and not r["st"].any() and not r["status"].any() and np.array_equal(r["m"], r["m"].T)
    matrix(r["m"], "big", range(16), range(16), "panel_big_16")
    r2 = fresh.result["panel_big_small_cols"]
    assert r2["raised"] is None and not r2["st"].any() and rmsd_matrix_ref.same_bits(r2["m_big"], r["m"][8:, 8:])
    assert r2["m"].shape == (16, 8) and rmsd_matrix_ref.same_bits(r2["m"], r2["m_again"])
    matrix(r2["m"], "small", range(16), range(4, 12), "small rows and columns")
    matrix(r2["m_t"], "small", range(4, 12), range(16), "small columns and rows")
    assert r2["refused"][:2] == ("RMSDError", "InconsistentGroup") and r2["refused"][2][1:] == (len(h["groups"]["small"]), len(h["groups"]["big"]))
    r3 = fresh.result["panel_device"]
    assert r3["raised"] is None and not r3["st"].any() and r3["shape"] == (8, 8) and rmsd_matrix_ref.same_bits(r3["m"], r["m"][8:, 8:])
    r = fresh.result["fail_panel_nan"]
    assert r["raised"] is None and r["st"].tolist() == r["status"].tolist() == [0, E_NO_POSITION, 0] and r["len"] == 3
    assert np.isnan(r["m"][1]).all() and np.isnan(r["m"][:, 1]).all()            # the failed frame took a row, and its entries are NaN
    assert rmsd_matrix_ref.same_bits(r["m"][np.ix_([0, 2], [0, 2])], fresh.result["panel_big_16"]["m"][np.ix_([2, 4], [2, 4])])
    r = fresh.result["fail_panel_masses"]
    assert r["raised"] is None and r["st"].tolist() == [HW.LIB.E_INVALID_ARG, 0, 0, 0, 0] and r["len_refused"] == 0 and not r["status"].any()
    assert r["refused"][0] == "DeviceError" and "the masses of its atoms have changed" in str(r["refused"][2])
    assert rmsd_matrix_ref.same_bits(r["m"], fresh.result["panel_big_16"]["m"][:4, :4])


def _check_io(G, fresh, h, aux, tmp):
    # the writers: the host encoder's bytes (test_gpu_xtc_encoder_device.py)
    for count, repeat in ((4, 5), (12, 2)):
        r = fresh.result["xtc_write_%d" % count]
        nf = count * repeat
        assert r["raised"] is None and r["device_frames"] == nf
        for k in range(nf):
            aux.s.copy_frame(HW.SPOOL + k, k % count)
        aux.s.set_tuning(xtc_device_encode=0)
        path = os.path.join(str(tmp), "host_%d.xtc" % count)
        with G.XtcWriter(path) as wr:
            wr.write_slots(aux.s, HW.SPOOL, nf, steps=np.arange(nf, dtype=np.int64) * 10, times=np.arange(nf, dtype=F) * 0.5, host_threads=2)
        aux.s.set_tuning(xtc_device_encode=1)
        assert r["bytes"] == open(path, "rb").read(), count
    # the readers: the host readers' frames bit for bit, a group-limited read leaves the other atoms alone
    host_x = [aux.xtc.read_frame(f) for f in range(HW.N_XTC)]
    host_t = [aux.trr.read_frame(f) for f in range(HW.N_XTC)]
    def check(name, first, nf, atoms, reader="xtc"):
        r = fresh.result[name]
        assert r["raised"] is None, (name, r["raised"])
        inside = np.zeros(HW.N, bool)
        inside[atoms] = True
        for k in range(nf):
            x = host_x[first + k][0] if reader == "xtc" else host_t[first + k][0]
            want = np.where(inside[:, None], x, h["frames"][k])
            assert np.array_equal(r["pos%d" % k].view(np.uint32), want.view(np.uint32)), (name, k)
            assert np.array_equal(r["box%d" % k][:3], np.asarray(HW.BOX, F)) and int(r["steps"][k]) == 10 * (first + k) and r["times"][k] == F(0.5 * (first + k)), (name, k)
    every = np.arange(HW.N)
    check("xtc_read_small", 0, 4, h["groups"]["small"])
    check("xtc_read_small_redefined", 0, 4, np.arange(HW.SMALL_XTC[0], HW.SMALL_XTC[1] + 1))
    check("xtc_read_full", 1, 5, every)
    check("xtc_read_masked", 3, 3, h["groups"]["masked"])
    check("xtc_read_full_again", 4, 2, every)
    check("trr_read", 0, 6, every, reader="trr")
    assert fresh.result["fail_xtc_range"]["raised"] == ("XtcError", None, None, HW.E_OUT_OF_RANGE)
    assert fresh.result["fail_xtc_nogroup"]["raised"] == ("XtcError", None, None, HW.E_GROUP_NOT_FOUND)
    for name, slots in (("fail_xtc_range", (0, 1)), ("fail_xtc_nogroup", (0,))):          # a refused read writes no slot
        for k in slots:
            assert np.array_equal(fresh.result[name]["pos%d" % k].view(np.uint32), h["frames"][k].view(np.uint32)), (name, k)


def _check_failures(fresh, h):
    want = {"fail_translate_nan_small": ("GroupError", "InvalidPosition", HW.NAN_SMALL), "fail_com_nan_big": ("GroupError", "InvalidPosition", HW.NAN_BIG),
            "fail_translate_nan_tail": ("GroupError", "InvalidPosition", HW.NAN_TAIL), "fail_center_nogroup": ("GroupError", "NotFound", None),
            "fail_rmsd_nan_small": ("RMSDError", "InvalidPosition", HW.NAN_SMALL), "fail_rmsd_nogroup": ("RMSDError", "NonexistentGroup", None),
            "fail_alldist_nan": ("GroupError", "InvalidPosition", HW.NAN_A40), "fail_pairs_nogroup": ("GroupError", "NotFound", None),
            "fail_whole_nan": ("AtomError", "InvalidPosition", HW.NAN_BIG), "fail_redef_nogroup": ("GroupError", "NotFound", None),
            "fail_center_nobox": ("GroupError", "InvalidSimBox", None), "fail_redefined_small_plan": ("RMSDError", "InconsistentGroup", None)}
    for name, (cls, variant, detail) in want.items():
        got = fresh.result[name]["raised"]
        assert got is not None and got[:2] == (cls, variant) and (detail is None or got[2] == detail), (name, got)
    assert fresh.result["fail_redefined_small_plan"]["raised"][2][1:] == (363, 394)
    other = np.arange(HW.SMALL_OTHER[0], HW.SMALL_OTHER[1] + 1, dtype=np.uint64)       # the centre of mass of the redefined group, in front of the plan's refusal
    assert np.abs(fresh.result["fail_redefined_small_plan"]["c"] - O.get_center(h["frames"][3], other, HW.BOX, h["masses"])).max() <= REF_CENTRE
    got = fresh.result["fail_alldist_skewed"]["raised"]                                # (test_gpu_pin_triclinic.py: a DeviceError that says "skewed")
    assert got is not None and got[0] == "DeviceError" and got[3] == E_UNSUPPORTED_BOX and "skewed" in str(got[1]) + str(got[2]) and "d" not in fresh.result["fail_alldist_skewed"], got
    for name in ("fail_translate_nan_small", "fail_translate_nan_tail", "fail_whole_nan"):
        got = fresh.result[name]["pos3"]
        assert np.array_equal(np.isnan(got).any(axis=1).nonzero()[0], [want[name][2]]), name
    got = fresh.result["fail_whole_nan"]["pos3"]                                      # (groan_hip.h: a frame that fails make-whole is left bit for bit untouched)
    assert np.array_equal(np.nan_to_num(got, nan=-1.0), np.nan_to_num(HW.nan_frame(3, HW.NAN_BIG), nan=-1.0))
    r = fresh.result["fail_center_batch_mixed"]
    assert r["st"].tolist() == [0, 0, E_NO_BOX, 0, E_NO_POSITION, 0] and np.isnan(r["c"][[2, 4]]).all() and not np.isnan(r["c"][[0, 1, 3, 5]]).any()
    r = fresh.result["fail_reduce_mixed"]
    assert r["st"].tolist() == [0, E_NO_BOX, E_NO_POSITION, 0] and np.array_equal(r["v"][[0, 3]], fresh.result["reduce_hist"]["v"][[0, 3]])
    r = fresh.result["fail_contacts_nan"]                                              # the failed frame is empty, the others are what they are without it
    good = fresh.result["contacts_pairs_8"]
    assert r["raised"] is None and r["st"].tolist() == [0, E_NO_POSITION, 0, 0] and r["n"][1] == 0 and np.array_equal(r["n"][[0, 2, 3]], good["n"][[2, 4, 5]])
    for k, f in ((0, 2), (2, 4), (3, 5)):
        for label in ("i", "j", "d"):
            assert np.array_equal(r[label][int(r["off"][k]):int(r["off"][k + 1])].view(np.uint32), good[label][int(good["off"][f]):int(good["off"][f + 1])].view(np.uint32)), (f, label)
    r = fresh.result["fail_hbond_mixed"]
    assert r["st"].tolist() == [0, E_NO_BOX, E_NO_POSITION] and int(r["offsets"][1]) >= 100 and int(r["offsets"][3]) == int(r["offsets"][1])
    r = fresh.result["masses_changed"]
    other = (h["masses"][::-1] * F(1.5)).astype(F)
    with O.acc64():
        assert np.abs(r["c_other"] - O.get_center(h["frames"][3], _idx("big"), HW.BOX, other)).max() <= REF_CENTRE
        assert np.abs(r["c"] - O.get_center(h["frames"][3], _idx("big"), HW.BOX, h["masses"])).max() <= REF_CENTRE
        assert np.abs(r["s"] - O.get_center(h["frames"][3], _idx("small"), HW.BOX, h["masses"])).max() <= REF_CENTRE
    r = fresh.result["tune_small_calls0"]
    assert r["small_calls"] == 0 and np.abs(r["c"] - fresh.result["center_small_21"]["c3"]).max() <= REF_CENTRE and np.array_equal(r["c_again"], fresh.result["center_small_21"]["c3"])
    r = fresh.result["tune_masked0"]
    assert np.abs(r["c"] - fresh.result["center_batch_masked_21"]["c"]).max() <= REF_CENTRE and np.abs(r["r"] - fresh.result["plan_rmsd_masked"]["r"][:4]).max() <= TOL_RMSD


def test_fresh_results_are_right(G, fresh, tmp_path):
    h = HW.host_world()
    aux = HW.make_world(G, tmp_path)
    checks = [lambda: _check_centres(fresh, h), lambda: _check_moves(fresh, h), lambda: _check_rmsd(fresh, h), lambda: _check_pairs(G, fresh, h, aux),
              lambda: _check_topology(G, fresh, h), lambda: _check_gyration(fresh, h), lambda: _check_series(G, fresh, h), lambda: _check_io(G, fresh, h, aux, tmp_path), lambda: _check_failures(fresh, h)]
    failed = []
    try:
        for k, check in enumerate(checks):                   # every family is checked, whatever the ones before it found
            try:
                with O.acc64():
                    check()
            except Exception:
                failed.append(traceback.format_exc())
    finally:
        aux.close()
    assert not failed, "\n".join(failed)
