"""What the tests of the single-wave kernels share (test_gpu_small_calls.py, test_gpu_small_edges.py; gr_small.h): the cells, the
seeded blob systems, the warm-up of every single-wave kernel, selections named by (layout, start, n), a pair of systems -- target and
reference, the reference with a mass vector of its own -- with the oracle's answers for them, and the comparisons.

Margins: TOL = 1e-5 nm against the oracle summing in double (the project's parity margin; the oracle's own f32 loop stays within
9e-7 nm of that for the rmsd and 4.8e-6 nm for the centres on these inputs), PATHS = 2e-6 nm between the single-wave and the batched
kernels (the same per-atom arithmetic, fp64 sums in another order)."""
import numpy as np

import oracle_lib as O

F = np.float32
TOL = 1e-5
PATHS = 2e-6
N_ATOMS = 4357          # neither a multiple of 4 nor of 256: a selection can end inside a ragged 4-atom group and a ragged tile
N_BIG = 8600            # the selections above the threshold, and the placements of one group among different neighbours
N_FRAMES = 3
SPREAD = 0.35           # nm: narrow enough that the image proof of the single pass holds

BOXES = {
    "orthorhombic": ([6.44, 6.76, 7.26], [90.0, 90.0, 90.0]),
    "dodecahedron": ([7.0, 7.0, 7.0], [60.0, 60.0, 90.0]),
    "triclinic": ([7.5, 7.0, 6.5], [75.0, 80.0, 70.0]),
}
CELLS = list(BOXES)

# (call, the oracle's function, weighted)
CENTRES = (("group_get_com", O.get_center, True), ("group_get_center", O.get_center, False), ("group_estimate_com", O.estimate_center, True),
           ("group_estimate_center", O.estimate_center, False), ("group_get_com_naive", lambda pos, idx, box, mass=None: O.center_naive(pos, idx, mass=mass), True))
VARIANT = {O.E_NO_POSITION: "InvalidPosition", O.E_NO_MASS: "InvalidMass"}


def make(G, n, nf, box, seed, spread=0.5):
    rng = np.random.default_rng(seed)
    masses = rng.uniform(1.0, 16.0, n).astype(np.float32)
    s = G.System(n, masses=masses, n_slots=nf + 1)
    frames = []
    for f in range(nf + 1):
        blob = rng.normal(0, spread, (n, 3)) + rng.uniform(0.1, 0.9, 3) * np.array([box[0], box[1], box[2]])
        pos = O.wrap_atoms(blob.astype(np.float32), np.arange(n), box)
        s.set_frame(pos, box, slot=f); frames.append(pos)
    return s, frames, masses, rng


_WARM = False


def warm(G):
    """Every single-wave kernel variant once, untimed, on a throwaway context: the FIRST launch of a kernel in a process (code-object load
    on a cold box) can outlast the 20 ms the host polls for a small call's result -- the call then synchronises the stream instead and
    counts it (GR_STAT_SMALL_SYNC_FALLBACKS).  With the kernels loaded, the tests assert that counter stays 0 on their own
    contexts: the polling path must be the one the tests exercise (round 4 had dropped the assertion instead).
    Once per process: a second call returns at once."""
    global _WARM
    if _WARM:
        return
    box = O.box_from_lengths_angles([6.0, 6.0, 6.0], [60.0, 60.0, 90.0])
    s, frames, m, rng = make(G, 2000, 2, box, 1)
    s.group_create_from_ranges("a", [(10, 300)]); s.group_create_from_indices("b", np.unique(rng.integers(0, 2000, 200)))
    ref = G.System(2000, masses=m, box=box, positions=frames[2])
    ref.group_create_from_ranges("a", [(10, 300)]); ref.group_create_from_indices("b", np.unique(rng.integers(0, 2000, 200)))
    for name in ("a", "b"):
        for fn in ("group_get_com", "group_get_center", "group_estimate_com", "group_estimate_center", "group_get_com_naive", "group_get_center_naive"):
            if hasattr(s, fn):
                getattr(s, fn)(name, slot=0)
        s.group_get_com_batch(name, 0, 2)
    s.group_distance("a", "b", G.Dimension.XYZ, slot=0)
    plan = G.RMSDPlan(ref, s, "a")
    plan.rmsd(0, 1); plan.rmsd(0, 2); plan.rmsd_fit(0, 1); plan.rmsd_fit(0, 2)
    plan.close(); ref.close(); s.close()
    _WARM = True


# ------------------------------------------------------------------ selections
def sel_indices(sel):
    """sel = (layout, start, n): "block" atoms start .. start + n - 1; "third" every third atom from start; "other" every other atom
    from start; "hole" two blocks from start with 300 atoms left out between them (the first holds n // 2 atoms)"""
    layout, start, n = sel
    if layout == "block": return np.arange(start, start + n)
    if layout == "third": return start + 3 * np.arange(n)
    if layout == "other": return start + 2 * np.arange(n)
    assert layout == "hole" and n >= 2
    h = n // 2
    return np.concatenate([np.arange(start, start + h), np.arange(start + h + 300, start + 300 + n)])


def sel_id(sel):
    return "%s-start%d-n%d" % sel


def sel_create(system, name, sel):
    layout, start, n = sel
    idx = sel_indices(sel)
    assert int(idx[-1]) < system.n_atoms, (sel, system.n_atoms)
    if layout == "block": system.group_create_from_ranges(name, [(start, start + n - 1)])
    elif layout == "hole": system.group_create_from_ranges(name, [(start, start + n // 2 - 1), (start + n // 2 + 300, start + 300 + n - 1)])
    else: system.group_create_from_indices(name, idx)
    return idx


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


# ------------------------------------------------------------------ a target system and its reference
class World:
    """A target system of n atoms with N_FRAMES frames and a reference system holding one more frame of the same blob.  The reference
    carries a second, independently seeded mass vector unless equal_masses: the plan's weights are then not the target's masses
    (GrPlanDev::w_is_mass = 0: `ww = w4[pg]` / `plan.w[jj]` and the separate sums of w v)."""

    def __init__(self, G, cell, n=N_ATOMS, seed=41, equal_masses=False):
        self.G, self.cell, self.n = G, cell, n
        self.box = O.box_from_lengths_angles(*BOXES[cell])
        self.s, frames, self.m, _ = make(G, n, N_FRAMES, self.box, seed, spread=SPREAD)
        self.frames, self.ref_pos = frames[:N_FRAMES], frames[N_FRAMES]
        self.m_ref = self.m if equal_masses else np.random.default_rng(seed + 1000).uniform(1.0, 16.0, n).astype(F)
        self.ref = G.System(n, masses=self.m_ref, box=self.box, positions=self.ref_pos)
        self.small = 4096
        self._groups = {}

    def close(self):
        self.ref.close(); self.s.close()

    def tune(self, small):
        self.small = small
        self.s.set_tuning(small_calls=small)

    def group(self, sel):
        """-> (name, indices): the selection as a group of both systems"""
        if sel not in self._groups:
            name = "%s_%d_%d" % sel
            idx = sel_create(self.s, name, sel)
            sel_create(self.ref, name, sel)
            self._groups[sel] = (name, idx)
        return self._groups[sel]

    def restore(self):
        """frames and masses as they were made (after a test that poisoned some)"""
        for f in range(N_FRAMES):
            self.s.set_frame(self.frames[f], self.box, slot=f)
        self.s.set_masses(self.m)

    def twin(self, sels, frames=None, masses=None):
        """another target system with the groups of `sels`: these frames and masses (default: this world's)"""
        t = self.G.System(self.n, masses=self.m if masses is None else masses, n_slots=N_FRAMES + 1)
        for f in range(N_FRAMES):
            t.set_frame((self.frames if frames is None else frames)[f], self.box, slot=f)
        t.set_tuning(small_calls=self.small)
        for sel in sels:
            sel_create(t, self.group(sel)[0], sel)
        return t

    # -- calls
    def both_paths(self, fn, s=None):
        """fn() by the single-wave kernels and by the batched ones (of target system s, default this world's)
        -> (small, batched, single-wave calls counted, single-wave calls counted with the path switched off)"""
        s = self.s if s is None else s
        before = s.stat("small_calls")
        a = fn()
        ran = s.stat("small_calls") - before
        s.set_tuning(small_calls=0)
        try:
            before = s.stat("small_calls")
            b = fn()
            ran0 = s.stat("small_calls") - before
        finally:
            s.set_tuning(small_calls=self.small)
        return a, b, ran, ran0

    def oracle_centre(self, call, idx, f, pos=None, mass=None):
        _, orc, w = next(c for c in CENTRES if c[0] == call)
        with O.acc64():
            return orc(self.frames[f] if pos is None else pos, idx, self.box, mass=(self.m if mass is None else mass) if w else None)

    def oracle_rmsd(self, idx, f, pos=None, mass=None):
        with O.acc64():
            return O.calc_rmsd(self.ref_pos, self.m_ref, idx, self.box, self.frames[f] if pos is None else pos, self.m if mass is None else mass, idx, self.box)[0]


def one_pass_centre(call, sel):
    """get_com / get_center of a contiguous group of at least 4 096 atoms is the one-pass centre's, not a single wave's (center_onepass_ok,
    gr_api.hip) -- and so is that of a DENSE list of that many atoms (at least 1/8 of its span: the masked walk of its span)"""
    return call in ("group_get_com", "group_get_center") and sel[2] >= 4096 and sel[0] in ("block", "other")


class Worst:
    """the largest differences seen, per family: printed at the end of the module (what the tests measured, beside what they assert)"""

    def __init__(self):
        self.d = {}

    def note(self, key, value, what):
        if value > self.d.get(key, (-1.0, None))[0]:
            self.d[key] = (float(value), what)

    def report(self):
        print()
        for key in sorted(self.d):
            print("largest %-40s %.3g nm  (%s)" % (key, self.d[key][0], self.d[key][1]))


WORST = Worst()


def check_centres(W, sel, frames=range(N_FRAMES), calls=None, s=None):
    """the five centre calls of one selection: against the oracle (TOL), against the batched kernels (PATHS), the path that ran
    -> {(call, frame): centre}.  s: a twin of the world's target system whose atoms INSIDE the selection are the world's (the oracle
    is asked about the world's own frames)"""
    name, idx = W.group(sel)
    s = W.s if s is None else s
    out = {}
    for f in frames:
        for call, _, _ in CENTRES:
            if calls is not None and call not in calls:
                continue
            got, ref, ran, ran0 = W.both_paths(lambda: getattr(s, call)(name, slot=f), s)
            assert ran == (0 if one_pass_centre(call, sel) else 1) and ran0 == 0, (sel, call, ran, ran0)
            want = W.oracle_centre(call, idx, f)
            d, d0 = float(np.abs(got - want).max()), float(np.abs(got.astype(np.float64) - ref).max())
            print("%s %s frame %d: |gpu - oracle| %.3g  |small - batched| %.3g" % (sel_id(sel), call, f, d, d0))
            if ran:
                WORST.note("|centre - oracle|", d, (W.cell, sel_id(sel), call, f)); WORST.note("|centre small - batched|", d0, (W.cell, sel_id(sel), call, f))
            assert d <= TOL, (sel, call, f, got, want)
            assert d0 <= PATHS, (sel, call, f, got, ref)
            out[(call, f)] = got
    assert s.stat("small_sync_fallbacks") == 0
    return out


def check_rmsd(W, sel, frames=range(N_FRAMES), s=None):
    """plan.rmsd(f, 1) of one selection: one single-wave call, against the oracle with the two mass vectors (TOL; one or two atoms:
    finite, the oracle's value printed) and against the batched kernels (PATHS; one or two atoms: TOL) -> {frame: rmsd}.  s: as in
    check_centres"""
    name, idx = W.group(sel)
    s = W.s if s is None else s
    plan = W.G.RMSDPlan(W.ref, s, name)
    out = {}
    try:
        for f in frames:
            (r, st), (r0, st0), ran, ran0 = W.both_paths(lambda: plan.rmsd(f, 1), s)
            assert ran == 1 and ran0 == 0, (sel, f, ran, ran0)
            assert st[0] == 0 and st0[0] == 0 and np.isfinite(r[0]), (sel, f, st, st0, r)
            want = W.oracle_rmsd(idx, f)
            d, d0 = abs(float(r[0]) - want), abs(float(r[0]) - float(r0[0]))
            # (redone: a thousand atoms or more of the blob, wrapped about a face of the dodecahedron, can reach past what the image proof
            #  about the first atom allows -- such a frame takes the literal redo on both paths and is compared like any other)
            print("%s rmsd frame %d: %.7g oracle %.7g  |gpu - oracle| %.3g  |small - batched| %.3g  redone %d" % (sel_id(sel), f, float(r[0]), want, d, d0, plan.last_fallbacks()))
            if sel[2] > 2:      # (one or two atoms do not determine a rotation: the Kabsch problem is rank-deficient)
                WORST.note("|rmsd - oracle|", d, (W.cell, sel_id(sel), f)); WORST.note("|rmsd small - batched|", d0, (W.cell, sel_id(sel), f))
                assert d <= TOL, (sel, f, float(r[0]), want)
                assert d0 <= PATHS, (sel, f, float(r[0]), float(r0[0]))
            else:
                assert d0 <= TOL, (sel, f, float(r[0]), float(r0[0]))
            out[f] = r[0]
    finally:
        plan.close()
    assert s.stat("small_sync_fallbacks") == 0
    return out


# ------------------------------------------------------------------ errors
def expected_error(fn):
    """fn() of the oracle -> (variant, atom) of the error it raises, None when it raises none"""
    try:
        with O.acc64():
            fn()
    except O.OracleError as e:
        return VARIANT[e.status], int(e.index)
    return None


def raised(G, fn):
    try:
        fn()
    except G.GroanError as e:
        return e.variant, e.detail
    return None


# ------------------------------------------------------------------ atoms at a cell face
def cell_rows(box):
    """rows = the box vectors (gromacs order xx yy zz xy xz yx yz zx zy)"""
    b = np.zeros(9); b[:len(box)] = box
    return np.array([[b[0], b[3], b[4]], [b[5], b[1], b[6]], [b[7], b[8], b[2]]], np.float64)


def wrapped_error(got, want, box, seam=2e-5, dims=(0, 1, 2)):
    """-> (largest component error per atom, number of atoms compared modulo a box vector): an atom that `want` leaves within `seam` nm of
    a cell face along an axis of `dims` (the axes that were wrapped) may come out at either face and is compared modulo that box vector"""
    H = cell_rows(box)
    u = np.asarray(want, np.float64) @ np.linalg.inv(H)
    L = np.diag(H)
    near = (np.abs(u) * L < seam) | (np.abs(1.0 - u) * L < seam)
    near[:, [k for k in range(3) if k not in dims]] = False
    d = np.asarray(got, np.float64) - np.asarray(want, np.float64)
    err = np.abs(d).max(axis=1)
    rows = np.nonzero(near.any(axis=1))[0]
    for a in rows:
        best = err[a]
        for k in np.nonzero(near[a])[0]:
            for sgn in (-1.0, 1.0):
                best = min(best, np.abs(d[a] - sgn * H[k]).max())
        err[a] = best
    return err, len(rows)
