"""The single-wave kernels (gr_small.h) at the boundaries their loops are written around: one lane, one 4-atom group, one row of lanes,
a half trip and a full trip of either kernel, two trips, the threshold GR_TUNE_SMALL_CALLS and -- with the threshold raised -- 8 192
atoms; every `start % 4`, starts just below, at and above a 256-atom tile boundary, a selection that ends on the system's last atom
(4 357 atoms: inside a ragged 4-atom group and a ragged tile); gather lists with a ragged tail.  The reference system carries a mass
vector of its own, so the plan's weights are NOT the target's masses (GrPlanDev::w_is_mass = 0; one selection is repeated with equal
masses).  Checked: values against the oracle summing in double (1e-5 nm) and against the batched kernels (2e-6 nm), the path that ran
(GR_STAT_SMALL_CALLS) and that no call fell back to a stream synchronisation; that no atom outside the selection reaches a sum (NaN
neighbours, bit for bit); the reference's error order at the edges; the literal redo of a frame whose image proof fails; a batch
against its per-frame calls bit for bit, also around a failed frame; group_distance's two waves; atoms_center's estimate that starts
the frame's state itself (fresh_bad); independence from the atoms around the group.  small_ref.py holds what is shared."""
import numpy as np
import pytest

import oracle_lib as O
import small_ref as R
from small_ref import CELLS, N_ATOMS, N_BIG, N_FRAMES, PATHS, TOL, bits, sel_id, sel_indices

pytestmark = pytest.mark.gpu

SIZES = [1, 2, 3, 4, 5, 7, 8, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 4095, 4096]
ALL_CELLS = (5, 257, 513)          # sizes run in all three cells; every other size in one (by turns)
STARTS = (2, 3, 253, 254, 255, 256, 257, 259)


@pytest.fixture(scope="module")
def G():
    import groan_rs_amd as g
    g._lib.load()
    return g


@pytest.fixture(scope="module", autouse=True)
def warm_single_wave_kernels(G):
    R.warm(G)
    yield
    R.WORST.report()


@pytest.fixture(scope="module")
def worlds(G):
    made = {}

    def get(cell, n=N_ATOMS, equal_masses=False):
        key = (cell, n, equal_masses)
        if key not in made:
            made[key] = R.World(G, cell, n=n, equal_masses=equal_masses)
        return made[key]
    yield get
    for w in made.values():
        w.close()


def _atoms_needed(sel):
    """the smallest of the systems used here that holds the selection"""
    last = int(sel_indices(sel)[-1])
    return N_ATOMS if last < N_ATOMS else N_BIG if last < N_BIG else 16400


def _value_cases():
    contiguous = [(("block", start, n), "") for n in SIZES for start in (0, 1)]
    contiguous += [(("block", start, n), "") for n in (5, 64, 257, 513) for start in STARTS]
    contiguous += [(("block", N_ATOMS - n, n), "-system-end") for n in (1, 3, 5, 257)]
    # every third atom from 2 while that fits the system; the two largest sizes as every other atom from 2 of the 8 600-atom system
    gathered = [((("third", 2, n) if 2 + 3 * (n - 1) < N_ATOMS else ("other", 2, n)), "") for n in SIZES]
    gathered += [(("hole", 1, n), "") for n in (5, 256, 257, 513)]
    out = []
    for sel, tag in contiguous + gathered:
        n = sel[2]
        for cell in (CELLS if n in ALL_CELLS else [CELLS[SIZES.index(n) % 3]]):
            for family in ("centres", "rmsd"):
                out.append(pytest.param(family, cell, sel, id="%s-%s-%s%s" % (family, cell, sel_id(sel), tag)))
    return out


def _check(family, W, sel, **kw):
    return (R.check_centres if family == "centres" else R.check_rmsd)(W, sel, **kw)


# ------------------------------------------------------------------ 1. values
@pytest.mark.parametrize("family,cell,sel", _value_cases())
def test_values_with_different_masses(worlds, family, cell, sel):
    """every size and start against the oracle and the batched kernels; the reference's masses are not the target's"""
    _check(family, worlds(cell, n=_atoms_needed(sel)), sel)


@pytest.mark.parametrize("sel", [("block", 255, 257), ("third", 2, 257)], ids=sel_id)
@pytest.mark.parametrize("family", ["centres", "rmsd"])
def test_values_with_equal_masses(worlds, family, sel):
    """the same atoms with the reference's masses equal to the target's: one load serves mass and weight (w_is_mass = 1)"""
    _check(family, worlds("triclinic", equal_masses=True), sel)
    _check(family, worlds("triclinic"), sel)


@pytest.mark.parametrize("sel", [("block", 1, 4097), ("block", 1, 8192), ("other", 2, 4097), ("other", 2, 8192)], ids=sel_id)
@pytest.mark.parametrize("family", ["centres", "rmsd"])
def test_above_the_threshold_with_small_calls_8192(worlds, family, sel):
    """GR_TUNE_SMALL_CALLS raised to 8 192: up to 16 outer trips per lane of a centre stage, 64 trips of the RMSD kernel.  (get_com /
    get_center of such a group stay the one-pass centre's: small_ref.one_pass_centre.  Every other atom of 8 192 needs 16 384 atoms: that
    one case has a system of 16 400.)"""
    W = worlds("orthorhombic", n=_atoms_needed(sel))
    W.tune(8192)
    try:
        _check(family, W, sel)
    finally:
        W.tune(4096)


# ------------------------------------------------------------------ 2. nothing outside the selection is read into a sum
POISONED = [("block", 0, 5), ("block", 1, 64), ("block", 2, 257), ("block", 3, 513), ("block", 253, 5), ("block", 254, 2), ("block", 255, 257),
            ("block", 256, 64), ("block", 257, 513), ("block", 259, 63), ("block", 1, 1023), ("block", 2, 3), ("block", N_ATOMS - 257, 257),
            ("third", 2, 7), ("third", 2, 65), ("third", 2, 1022), ("hole", 1, 257)]


@pytest.mark.parametrize("sel", POISONED, ids=lambda s: sel_id(s) + "-poisoned-neighbours")
@pytest.mark.parametrize("family", ["centres", "rmsd"])
def test_atoms_outside_the_selection_do_not_enter(worlds, family, sel):
    """every atom that is not in the selection has a NaN position and a NaN mass in the target (the reference system is clean: only the
    group's atoms enter the plan): the straddling 4-atom groups, the clamped loads of a ragged tail and the rows of the tile around the
    selection must leave no trace -- the same bits as the clean run, which is itself checked as in (1)"""
    W = worlds(CELLS[POISONED.index(sel) % 3])
    _, idx = W.group(sel)
    clean = _check(family, W, sel)
    frames = []
    for f in range(N_FRAMES):
        pos = np.full_like(W.frames[f], np.nan); pos[idx] = W.frames[f][idx]; frames.append(pos)
    m = np.full_like(W.m, np.nan); m[idx] = W.m[idx]
    twin = W.twin([sel], frames, m)
    try:
        dirty = _check(family, W, sel, s=twin)
    finally:
        twin.close()
    assert clean.keys() == dirty.keys()
    for k in clean:
        assert np.array_equal(bits(clean[k]), bits(dirty[k])), (sel, k, clean[k], dirty[k])


# ------------------------------------------------------------------ 3. errors in the reference's order
# (ordinals without position, ordinals without mass); negative: from the end
ERRORS = {"position-first": ([0], []), "position-last": ([-1], []), "position-ordinal-600": ([600], []), "position-two": ([1, -2], []),
          "mass": ([], ["mid"]), "mass-and-lower-position": ([1], ["mid"]), "mass-and-higher-position": ([-1], ["mid"])}


@pytest.mark.parametrize("case,n,layout", [pytest.param(c, n, layout, id="%s-%s-n%d" % (c, layout, n)) for c in ERRORS for n in (5, 257, 1025) for layout in ("block", "third")
                                           if c != "position-ordinal-600" or n > 600])
def test_errors_in_the_reference_order(G, worlds, case, n, layout):
    """a missing position at the selection's first atom (the RMSD kernel's provisional centre), at its last (the ragged tail), in an
    unchecked interior group of a later trip, two at once; a missing mass alone and beside a missing position: variant and atom of the
    oracle's error, from the single wave and from the batched kernels"""
    W = worlds("orthorhombic")
    sel = (layout, 255 if layout == "block" else 2, n)
    name, idx = W.group(sel)
    no_pos, no_mass = ERRORS[case]
    pos, m = W.frames[0].copy(), W.m.copy()
    pos[idx[no_pos]] = np.nan
    m[idx[[n // 2 for _ in no_mass]]] = np.nan
    try:
        W.s.set_frame(pos, W.box, slot=0); W.s.set_masses(m)
        plan = G.RMSDPlan(W.ref, W.s, name)
        calls = [(c, (lambda c=c: getattr(W.s, c)(name, slot=0)), (lambda c=c: W.oracle_centre(c, idx, 0, pos, m))) for c in ("group_get_com", "group_estimate_com", "group_get_com_naive")]
        calls.append(("rmsd", lambda: plan.rmsd(0, 1), lambda: W.oracle_rmsd(idx, 0, pos, m)))
        for call, fn, oracle in calls:
            want = R.expected_error(oracle)
            assert want is not None, (case, call)
            got, got0, ran, ran0 = W.both_paths(lambda: R.raised(G, fn))
            print(case, sel_id(sel), call, "oracle", want, "single wave", got, "batched", got0)
            assert got == want and got0 == want, (case, sel, call, want, got, got0)
            assert ran == 1 and ran0 == 0, (case, sel, call, ran, ran0)
        assert W.s.stat("small_sync_fallbacks") == 0
        plan.close()
    finally:
        W.restore()


# ------------------------------------------------------------------ 4. the literal redo
@pytest.mark.parametrize("layout", ["block", "third"])
@pytest.mark.parametrize("start", [1, 255])
@pytest.mark.parametrize("n", [5, 257, 513, 1025])
def test_the_redo_of_a_frame_whose_image_proof_fails(G, worlds, n, start, layout):
    """the selection's x spread over 0.75 of the cell: the single pass's image proof fails and the frame is redone by k_center_small_pbc
    + k_rmsd_small<1>, the literal sums about the frame's own centre of mass -- with the plan's weights, not the target's masses"""
    W = worlds("orthorhombic")
    sel = (layout, start, n)
    name, idx = W.group(sel)
    wide = W.frames[1].copy()
    wide[idx, 0] = np.linspace(0.2, W.box[0] * 0.75, n).astype(np.float32)
    try:
        W.s.set_frame(wide, W.box, slot=1)
        plan = G.RMSDPlan(W.ref, W.s, name)
        before = W.s.stat("small_calls")
        r, st = plan.rmsd(1, 1)
        assert W.s.stat("small_calls") == before + 1 and st[0] == 0
        assert plan.last_fallbacks() == 1
        want = W.oracle_rmsd(idx, 1, wide)
        d = abs(float(r[0]) - want)
        print("redo %s: %.7g oracle %.7g |gpu - oracle| %.3g" % (sel_id(sel), float(r[0]), want, d))
        R.WORST.note("|rmsd redo - oracle|", d, sel_id(sel))
        assert d <= TOL, (sel, float(r[0]), want)
        assert W.s.stat("small_sync_fallbacks") == 0
        plan.close()
    finally:
        W.restore()


# ------------------------------------------------------------------ 5. a batch equals its per-frame calls
def _status_of(G, fn):
    try:
        return fn(), 0
    except G.GroanError as e:
        return None, e.status


@pytest.mark.parametrize("middle", ["clean", "middle-frame-fails"])
@pytest.mark.parametrize("sel", [("block", 1, 3), ("block", 1, 65), ("block", 255, 257), ("block", 3, 513), ("block", 1, 4096), ("third", 2, 3), ("third", 2, 65),
                                 ("third", 2, 257), ("third", 2, 513)], ids=sel_id)
def test_a_batch_equals_its_per_frame_calls(G, worlds, sel, middle):
    """k_center_small_pbc / k_center_small_stage / k_rmsd_small with one wave per frame against the one-frame kernels: the same bits.  With a
    NaN inside the selection of the middle frame, that frame's status is the per-frame call's and its neighbours' values do not move.
    (4 096 contiguous atoms: get_com is the one-pass centre's by default -- here that centre is switched off, so the batch and the
    per-frame call are both the single wave's at its threshold.)"""
    W = worlds("orthorhombic")
    name, idx = W.group(sel)
    n = sel[2]
    frames = [p.copy() for p in W.frames]
    if middle != "clean":
        frames[1][idx[n // 2]] = np.nan
    twin = plan = plan2 = None
    try:
        W.s.set_center_onepass_min(0)
        W.s.set_frame(frames[1], W.box, slot=1)
        for batch, single in (("group_get_com_batch", "group_get_com"), ("group_estimate_com_batch", "group_estimate_com")):
            got, st = getattr(W.s, batch)(name, 0, N_FRAMES, raise_on_error=False)
            before = W.s.stat("small_calls")
            for f in range(N_FRAMES):
                one, s1 = _status_of(G, lambda: getattr(W.s, single)(name, slot=f))
                assert st[f] == s1 and (s1 != 0) == (middle != "clean" and f == 1), (batch, f, st, s1)
                if s1 == 0: assert np.array_equal(bits(got[f]), bits(one)), (batch, f, got[f], one)
                else: assert np.isnan(got[f]).all()
            assert W.s.stat("small_calls") == before + N_FRAMES
        plan = G.RMSDPlan(W.ref, W.s, name)
        rb, st = plan.rmsd(0, N_FRAMES, raise_on_error=False)
        singles = []
        before = W.s.stat("small_calls")
        for f in range(N_FRAMES):
            r1, s1 = plan.rmsd(f, 1, raise_on_error=False)
            assert st[f] == s1[0] and (s1[0] != 0) == (middle != "clean" and f == 1), (f, st, s1)
            if s1[0] == 0: assert np.array_equal(bits(rb[f]), bits(r1[0])), (f, rb, r1)
            singles.append((r1[0], s1[0]))
        assert W.s.stat("small_calls") == before + N_FRAMES
        # the fit: one frame per call on a twin system, the batch here -- the same rmsd, statuses and coordinates
        twin = W.twin([sel], frames)
        plan2 = G.RMSDPlan(W.ref, twin, name)
        for f in range(N_FRAMES):
            r1, s1 = plan2.rmsd_fit(f, 1, raise_on_error=False)
            assert s1[0] == singles[f][1]
            if s1[0] == 0: assert np.array_equal(bits(r1[0]), bits(singles[f][0]))
        rb2, st2 = plan.rmsd_fit(0, N_FRAMES, raise_on_error=False)
        assert np.array_equal(st2, st)
        for f in range(N_FRAMES):
            if st[f] == 0: assert np.array_equal(bits(rb2[f]), bits(rb[f]))
            assert np.array_equal(bits(twin.get_positions(f)), bits(W.s.get_positions(f))), f
        assert W.s.stat("small_sync_fallbacks") == 0 and twin.stat("small_sync_fallbacks") == 0
    finally:
        for x in (plan, plan2, twin):
            if x is not None: x.close()
        W.s.set_center_onepass_min(4096)
        W.restore()


# ------------------------------------------------------------------ 6. group_distance
@pytest.mark.parametrize("na,nb", [(1, 4096), (4096, 1), (65, 513), (3, 257)])
def test_group_distance_two_waves_in_one_dispatch(G, worlds, na, nb):
    """k_center_small with two workgroups, a block and a list, of very different lengths: the wave that ends first publishes first, the
    host waits for both words.  (A contiguous or dense group of 4 096 atoms would take the one-pass centre: it is switched off for those
    pairs, which then are one dispatch of two waves, one of them at the threshold; the list of 4 096 is every other atom of 8 600.)"""
    big = max(na, nb) >= 4096
    W = worlds("orthorhombic", n=N_BIG if big else N_ATOMS)
    sa, sb = ("block", 1, na), (("other", 2, nb) if nb >= 4096 else ("third", 2, nb))
    (a, ia), (b, ib) = W.group(sa), W.group(sb)
    try:
        if big: W.s.set_center_onepass_min(0)
        for f in range(N_FRAMES):
            ca, cb = W.s.group_get_center(a, slot=f), W.s.group_get_center(b, slot=f)
            for dim in (G.Dimension.XYZ, G.Dimension.X, G.Dimension.YZ):
                d, d0, ran, ran0 = W.both_paths(lambda: W.s.group_distance(a, b, dim, slot=f))
                assert ran == 1 and ran0 == 0, (na, nb, ran, ran0)
                with O.acc64():
                    want = O.distance(O.get_center(W.frames[f], ia, W.box), O.get_center(W.frames[f], ib, W.box), dim.name.lower(), W.box)
                print("distance %d / %d frame %d %s: %.7g oracle %.7g batched %.7g" % (na, nb, f, dim.name, d, want, d0))
                R.WORST.note("|distance - oracle|", abs(d - want), (na, nb, f, dim.name)); R.WORST.note("|distance small - batched|", abs(d - d0), (na, nb, f, dim.name))
                assert abs(d - want) <= 2e-5, (na, nb, f, dim, d, want)
                assert abs(d - d0) <= PATHS
                assert abs(d - O.distance(ca, cb, dim.name.lower(), W.box)) <= PATHS
        assert W.s.stat("small_sync_fallbacks") == 0
    finally:
        W.s.set_center_onepass_min(4096)


# ------------------------------------------------------------------ 7. atoms_center
@pytest.mark.parametrize("dim", ["XYZ", "XY"])
@pytest.mark.parametrize("call", ["atoms_center", "atoms_center_mass"])
@pytest.mark.parametrize("layout", ["block", "third"])
@pytest.mark.parametrize("n", [1, 65, 513])
def test_atoms_center_about_a_small_group_fresh_bad(G, worlds, n, layout, call, dim):
    """k_center_small_stage with fresh_bad: no reset launch in front of it, the translate kernel's words set by the wave.  An atom the
    oracle leaves within 2e-5 nm of a cell face is compared modulo that box vector (at most 2 per call: 4 357 atoms in a cell of 6.5 nm
    or more put 0.01 there)"""
    W = worlds(CELLS[[1, 65, 513].index(n)])
    sel = (layout, 255 if layout == "block" else 2, n)
    name, idx = W.group(sel)
    try:
        for f in range(N_FRAMES):
            getattr(W.s, call)(name, G.Dimension[dim], slot=f)
            with O.acc64():
                want = O.atoms_center(W.frames[f], idx, dim.lower(), W.box, mass=W.m if call == "atoms_center_mass" else None)
            err, at_face = R.wrapped_error(W.s.get_positions(f), want, W.box)
            print("%s %s %s frame %d: max |error| %.3g nm, %d atoms at a cell face" % (call, dim, sel_id(sel), f, err.max(), at_face))
            R.WORST.note("|atoms_center - oracle|", err.max(), (W.cell, call, dim, sel_id(sel), f))
            assert at_face <= 2
            assert err.max() <= TOL, (call, dim, sel, f, float(err.max()), int(err.argmax()))
    finally:
        W.restore()


@pytest.mark.parametrize("call", ["atoms_center", "atoms_center_mass"])
def test_atoms_center_reports_the_group_first_atom_and_leaves_the_frame(G, worlds, call):
    W = worlds("orthorhombic")
    sel = ("block", 255, 65)
    name, idx = W.group(sel)
    pos = W.frames[0].copy(); pos[idx[0]] = np.nan
    try:
        W.s.set_frame(pos, W.box, slot=0)
        want = R.expected_error(lambda: O.atoms_center(pos, idx, "xyz", W.box, mass=W.m if call == "atoms_center_mass" else None))
        got = R.raised(G, lambda: getattr(W.s, call)(name, G.Dimension.XYZ, slot=0))
        assert want == ("InvalidPosition", int(idx[0])) and got == want, (want, got)
        assert np.array_equal(bits(W.s.get_positions(0)), bits(pos))
    finally:
        W.restore()


# ------------------------------------------------------------------ 8. independence from the neighbours
def test_the_same_atoms_among_other_neighbours(G):
    """257 atoms -- positions, masses, reference -- at start 0, 255 and 4 100 of a system of 8 600 other atoms, as the list "every third atom
    from 2" there, and as the same list in a system of different other atoms.
    Bit for bit: start 0 against start 4 100, and the list against itself.  A centre stage gives ordinal j to lane j % 64 whatever the
    atoms' indices are; k_rmsd_small walks a block by the 4-atom groups of the FRAME, lane = group - (start >> 2) (mod 64) and the group's
    members decided by start % 4 -- so two starts with the same start % 4 put the same atoms into the same groups on the same lanes in the
    same order (the reference rows are the plan's, stored by ordinal + start % 256 and read back from the tile's origin: the same rows),
    and the neighbours in the straddling groups are masked out.  A list is walked by position, four entries per lane.
    Start 255 (start % 4 = 3) and the list against the blocks group the atoms differently: 2e-6 nm, the limit between two orders of the
    same fp64 sums."""
    box = O.box_from_lengths_angles(*R.BOXES["triclinic"])
    n = 257
    bases = []
    for seed in (77, 78):
        s0, frames, m, _ = R.make(G, N_BIG, N_FRAMES, box, seed, spread=R.SPREAD)
        s0.close()
        bases.append((frames, m, np.random.default_rng(seed + 1000).uniform(1.0, 16.0, N_BIG).astype(np.float32)))
    P = [bases[0][0][f][1000:1000 + n].copy() for f in range(N_FRAMES + 1)]
    pm, pm_ref = bases[0][1][1000:1000 + n].copy(), bases[0][2][1000:1000 + n].copy()
    places = {"start-0": (0, ("block", 0, n)), "start-255": (0, ("block", 255, n)), "start-4100": (0, ("block", 4100, n)), "list": (0, ("third", 2, n)),
              "list-elsewhere": (1, ("third", 2, n))}
    res = {}
    for key, (base, sel) in places.items():
        frames, m, m_ref = [p.copy() for p in bases[base][0]], bases[base][1].copy(), bases[base][2].copy()
        idx = sel_indices(sel)
        for f in range(N_FRAMES + 1):
            frames[f][idx] = P[f]
        m[idx] = pm; m_ref[idx] = pm_ref
        s = G.System(N_BIG, masses=m, n_slots=N_FRAMES)
        for f in range(N_FRAMES):
            s.set_frame(frames[f], box, slot=f)
        ref = G.System(N_BIG, masses=m_ref, box=box, positions=frames[N_FRAMES])
        R.sel_create(s, "g", sel); R.sel_create(ref, "g", sel)
        plan = G.RMSDPlan(ref, s, "g")
        before = s.stat("small_calls")
        out = {}
        for f in range(N_FRAMES):
            for call, _, _ in R.CENTRES:
                out[(call, f)] = getattr(s, call)("g", slot=f)
            r, st = plan.rmsd(f, 1)
            assert st[0] == 0
            out[("rmsd", f)] = r[:1].copy()
        assert s.stat("small_calls") == before + N_FRAMES * (len(R.CENTRES) + 1) and s.stat("small_sync_fallbacks") == 0
        res[key] = out
        plan.close(); ref.close(); s.close()
    same_bits = {frozenset(("start-0", "start-4100")), frozenset(("list", "list-elsewhere"))}
    keys = list(places)
    for i, a in enumerate(keys):
        for b in keys[i + 1:]:
            for k in res[a]:
                d = float(np.abs(res[a][k].astype(np.float64) - res[b][k]).max())
                R.WORST.note("|placement - placement|", d, (a, b, k))
                if frozenset((a, b)) in same_bits: assert np.array_equal(bits(res[a][k]), bits(res[b][k])), (a, b, k, res[a][k], res[b][k])
                else: assert d <= PATHS, (a, b, k, res[a][k], res[b][k])
