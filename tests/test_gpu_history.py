"""A call's result does not depend on what its context did before.

tests/history_world.py builds one world and a table of call kinds over every family of the library (centres, RMSD, pair distances,
topology, trajectory I/O, failing calls, redefinitions).  Every kind runs on two fresh worlds of its own: those two results must
agree, bit for bit wherever the project documents determinism (everything but the RMSD calls); an RMSD kind whose fresh results differ
is held to the margins of tests/test_gpu_resident.py (RMSD 2e-6 nm, fitted coordinates 2e-5 nm; rotation elements 2e-6 as in
tests/test_gpu_rmsd_fast.py) from then on.  The fresh result is checked once against the reference the suite uses for that call.
Then ONE long-lived world walks the mandatory adjacencies (each behind a shortcut of the library: an elided reset, a shared
sequence word, a grow-only buffer, a cache) and two seeded schedules, and every step must give its kind's fresh result."""
import itertools
import os
import time
import traceback

import numpy as np
import pytest

import gridmap_ref
import hbond_ref
import history_world as HW
import oracle_lib as O
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
              lambda: _check_topology(G, fresh, h), lambda: _check_io(G, fresh, h, aux, tmp_path), lambda: _check_failures(fresh, h)]
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
