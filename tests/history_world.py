"""One deterministic world, a table of call kinds and seeded schedules over them: the material of tests/test_gpu_history.py, which
checks that a call's result does not depend on what its context did before (test_history_schedule.py checks this module on the CPU).

The world: 12 003 atoms (no multiple of 4 or 256; three resident workgroups, the last one ragged) as 4 001 water-like molecules O H H,
frames = one base configuration plus a little noise, every atom wrapped into its cell on its own (so the molecules on a cell face are
broken), 400 donor-acceptor pairs placed 0.28 nm apart with the hydrogen on the line.  Slots 0-7 orthorhombic, 8-15 triclinic (the
cells of test_gpu_segments.py), slot 16 the noise-free RMSD reference (also slot 0 of a reference System of its own).  Slots 17-40
are the xtc writer's spool: write_slots takes consecutive slots and the device encoder needs 200 000 atoms in a call, so the frames
to write are repeated there with copy_frame, as test_gpu_xtc_encoder_device.py repeats its frames.

A kind is a function (world) -> result.  It first puts back, from the pristine host frames, every slot it reads or writes that an
earlier kind has changed (`World.need`; by set_frame or by upload_async + upload_wait, fixed per kind), makes its calls and returns
everything they handed back: arrays, statuses, the exception if one was raised (with its atom index), and positions and box of every slot
it may write.  A kind leaves groups, bonds, masses and tuning as it found them.

The family "series" holds the objects that keep state over the frames handed to them -- Fluctuations (groups of all three snapshot
forms), Covariance, MSD, VectorCorrelation, Internals, RMSDPanel -- and the topology family `Segments.gyration` on the segments of
`centers` plus `sizes` (1 to 4 097 consecutive atoms: every team class of the moments kernel).  The world makes each of them on
first use (`World.fluct`, `.covar`, `.msd`, `.vcorr`, `.internals`, `.panel`, `.segments`), so a fresh world of another kind pays nothing
for them and the order of creation differs between a fresh world and the long-lived one.  Every kind on such an object starts with
clear() and returns statuses, the raw state and the closed results; MSD and VectorCorrelation kinds stay inside one cell (the
whole configuration moves between slot 7 and slot 8).  A call that is refused outright (capacity, changed masses) puts its status
in front of the frames' statuses in `st` and its exception in `refused`.  rmsd_matrix(rows, cols) needs panels of equally many
atoms, so the columns panel on `small` (capacity 8) meets a rows panel on `small`; `big` against it is the refused call.
ADJACENCIES 11-19 stand behind the shortcuts of these objects; each says which."""
import functools
import os

import numpy as np

from groan_rs_amd import _lib as LIB
from groan_rs_amd._lib import E_GROUP_NOT_FOUND, E_HIP, E_NO_BOX, E_NO_POSITION, E_OUT_OF_RANGE, E_UNSUPPORTED_BOX     # the status codes of include/groan_hip.h, for the tests too

F = np.float32
N, N_MOL, N_FRAMES, REF_SLOT, SPOOL, N_SPOOL = 12003, 4001, 16, 16, 17, 24
N_SLOTS = SPOOL + N_SPOOL
BOX = [6.0, 6.4, 5.0]
TRIC = [6.0, 6.4, 5.0, 0, 0, 1.0, 0, -1.5, 0.8]
FLAT = [12.8942, 29.4173, 3.27353, 0, 0, -4.28403, 0, -1.85917, -4.05997]      # test_gpu_pin_triclinic.py "flat_a": too skewed for the image table
GRID = (18, 20, 15)              # lattice sites per cell vector, 0.32 to 0.33 nm apart
USED = (16, 18, 15)              # ... of which the molecules fill these: a gap along x and y (and the unfilled last planes along z) keeps the periodic centre of
                                 # every group well conditioned -- a group that covers a cell vector evenly has no centre along it
N_HB_PAIRS = 400
HB_DISTANCE, HB_ANGLE = 0.3, 150.0
NAN_SMALL, NAN_BIG, NAN_TAIL, NAN_A40 = 100, 3000, N - 1, 20
SMALL, SMALL_OTHER, SMALL_XTC = (5, 367), (7, 400), (400, 700)
RANGES = {"all": (0, N - 1), "small": SMALL, "big": (1003, 6002), "a40": (10, 49), "b50": (1000, 1049), "a300": (300, 599), "b400": (1500, 1899)}
DEFAULT_TUNING = dict(resident=1, center_resident=1, fuse=1, two_pass=1, small_calls=4096, pairdist_symmetric=1, masked_selections=1, translate_rows=1,
                      xtc_device_encode=1)
N_XTC = 6
CT_CUTOFF, CT_BINS = 0.3, 40
REGION_SPECS = [dict(kind="sphere", position=[2.6, 2.8, 2.2], radius=1.6),                       # a sphere and a cylinder along z, both inside the filled part of the cell
                dict(kind="cylinder", position=[2.4, 2.6, 0.8], radius=1.2, height=3.0, orientation="z")]
SERIES_CAPACITY, PANEL_SMALL_CAPACITY = 16, 8
SERIES_MOLS = tuple(range(0, N_MOL, 10))                                                         # the molecules whose O-H1 vectors and internal coordinates are followed
SIZES = (1, 5, 17, 65, 257, 4097)                                                                # the segments of seg["sizes"], cut from consecutive atoms: every team class of k_segment_moments
NAN_SERIES = 3 * 200 + 1                                                                         # H1 of a followed molecule
DIHEDRAL_MIN_SINE = 0.3
NAIVE, ESTIMATE, PBC = 0, 1, 2
CENTRES = [(NAIVE, 0), (NAIVE, 1), (ESTIMATE, 0), (ESTIMATE, 1), (PBC, 0), (PBC, 1)]


def cell(box):
    """rows = the box vectors (gromacs order xx yy zz xy xz yx yz zx zy)"""
    b = np.zeros(9); b[:len(box)] = box
    return np.array([[b[0], b[3], b[4]], [b[5], b[1], b[6]], [b[7], b[8], b[2]]], np.float64)


def box_of(slot):
    return BOX if slot < 8 or slot == REF_SLOT else TRIC


# ------------------------------------------------------------------ the host side
@functools.lru_cache(maxsize=None)
def host_world():
    """-> dict: frames [17] float32 [N, 3], boxes [17], masses, bonds, bonds_alt, groups {name: indices}, resid, xtc_frames [N_XTC]"""
    rng = np.random.default_rng(20261019)
    nx, ny, nz = USED
    k, j, i = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    site = np.stack([i.ravel(), j.ravel(), k.ravel()], 1)[:N_MOL]                   # i runs fastest
    frac = site / np.array(GRID, np.float64) + rng.uniform(-0.002, 0.002, (N_MOL, 3))
    # a water molecule in a random orientation: O-H 0.1 nm, H-O-H 104.5 degrees
    def unit(v):
        return v / np.linalg.norm(v, axis=1)[:, None]
    e1 = unit(rng.normal(size=(N_MOL, 3)))
    e2 = unit(np.cross(e1, rng.normal(size=(N_MOL, 3))))
    # donors: an even site of the row with its right-hand neighbour, 400 of them spread over the system
    cand = np.nonzero((site[:, 0] % 2 == 0) & (site[:, 0] + 1 < nx) & (np.arange(N_MOL) + 1 < N_MOL))[0]
    donors = cand[np.linspace(0, len(cand) - 1, N_HB_PAIRS).astype(int)]
    assert len(set(donors.tolist())) == N_HB_PAIRS
    e1[donors] = [1.0, 0.0, 0.0]
    e2[donors] = unit(np.cross(e1[donors], rng.normal(size=(N_HB_PAIRS, 3))))
    a = np.deg2rad(104.5)
    h1, h2 = 0.1 * e1, 0.1 * (np.cos(a) * e1 + np.sin(a) * e2)
    masses = np.array([1.008, 12.011, 14.007, 15.999], F)[np.arange(N) % 4]

    def frame(box, noise):
        H = cell(box)
        o = frac @ H
        o[donors + 1] = o[donors] + [0.28, 0.0, 0.0]                               # the acceptor, on the line O-H1
        pos = np.empty((N, 3))
        pos[0::3], pos[1::3], pos[2::3] = o, o + h1, o + h2
        if noise is not None:
            pos += np.repeat(noise.normal(0.0, 0.004, (N_MOL, 3)), 3, axis=0) + noise.normal(0.0, 0.002, (N, 3))
        u = pos @ np.linalg.inv(H)
        return ((u - np.floor(u)) @ H).astype(F)                                   # every atom into the cell on its own

    frames = [frame(box_of(f), np.random.default_rng(1000 + f)) for f in range(N_FRAMES)] + [frame(BOX, None)]
    boxes = [box_of(f) for f in range(N_FRAMES + 1)]
    xtc_frames = [frame(BOX, np.random.default_rng(2000 + f)) for f in range(N_XTC)]
    ox = np.arange(0, N, 3)
    bonds = np.concatenate([np.stack([ox, ox + 1], 1), np.stack([ox, ox + 2], 1)]).astype(np.uint64)
    bonds_alt = np.concatenate([np.stack([ox, ox + 1], 1), np.stack([ox[:-1] + 2, ox[1:]], 1)[::5]]).astype(np.uint64)      # O-H1 only, and every fifth molecule tied to the next
    groups = {name: np.arange(a, b + 1) for name, (a, b) in RANGES.items()}
    groups["masked"] = np.arange(0, 10000, 2)
    groups["listbig"] = groups["masked"]
    groups["list"] = np.arange(0, N, 7)
    groups["oxy"] = ox
    groups["hyd"] = np.sort(np.concatenate([ox + 1, ox + 2]))
    return dict(frames=frames, boxes=boxes, masses=masses, bonds=bonds, bonds_alt=bonds_alt, groups=groups, resid=(np.arange(N) // 7).astype(np.uint64),
                xtc_frames=xtc_frames, donors=donors)


def bend_sines(tuples, frames=range(N_FRAMES)):
    """[len(frames), T, 2]: the sines of the two bend angles i-j-k and j-k-l of the dihedral tuples, minimum image, in f64"""
    h = host_world()
    t = np.asarray(tuples, np.int64)
    out = []
    for f in frames:
        x, H = h["frames"][f].astype(np.float64), cell(h["boxes"][f])
        def d(a, b):
            v = x[b] - x[a]
            return v - np.round(v @ np.linalg.inv(H)) @ H
        def sine(u, v):
            return np.linalg.norm(np.cross(u, v), axis=1) / (np.linalg.norm(u, axis=1) * np.linalg.norm(v, axis=1))
        out.append(np.stack([sine(d(t[:, 1], t[:, 0]), d(t[:, 1], t[:, 2])), sine(d(t[:, 2], t[:, 1]), d(t[:, 2], t[:, 3]))], 1))
    return np.stack(out)


@functools.lru_cache(maxsize=None)
def series_tuples():
    """-> dict: pairs [401, 2] O-H1 and angles [401, 3] H1-O-H2 of every 10th molecule; dihedrals [<= 400, 4] H2-O...O'-H2' of the placed
    donor-acceptor pairs (not H1: it lies on the line O...O'), without those whose bend angles come near 0 or 180 degrees in some
    frame; sizes: the atom lists of the segments of SIZES"""
    h = host_world()
    o = 3 * np.array(SERIES_MOLS, np.int64)
    d = 3 * h["donors"].astype(np.int64)
    dih = np.stack([d + 2, d, d + 3, d + 5], 1)
    dih = dih[(bend_sines(dih) >= DIHEDRAL_MIN_SINE).all(axis=(0, 2))]
    off = np.concatenate([[0], np.cumsum(SIZES)])
    return dict(pairs=np.stack([o, o + 1], 1).astype(np.uint64), angles=np.stack([o + 1, o, o + 2], 1).astype(np.uint64), dihedrals=dih.astype(np.uint64),
                sizes=[np.arange(off[k], off[k + 1], dtype=np.uint64) for k in range(len(SIZES))])


def nan_frame(slot, atom):
    x = host_world()["frames"][slot].copy()
    x[atom] = np.nan
    return x


# ------------------------------------------------------------------ the device side
class World:
    def __init__(self, G, tmp_dir):
        self.G, self.tmp, self.host = G, str(tmp_dir), host_world()
        h = self.host
        self.s = G.System(N, masses=h["masses"], n_slots=N_SLOTS)
        self.ref = G.System(N, masses=h["masses"], n_slots=1)
        self.ref.set_frame(h["frames"][REF_SLOT], BOX, slot=0)
        self.pin, self._pin_ptr = G.pinned_array((N, 3))
        self.dirty = set()
        for slot in range(N_FRAMES + 1):
            self.load(slot, "set_frame")
        for s in (self.s, self.ref):
            for name, r in RANGES.items():
                s.group_create_from_ranges(name, [r])
            s.group_create_from_indices("masked", h["groups"]["masked"])
            s.group_create_from_indices("list", h["groups"]["list"])
            s.group_create_from_indices("oxy", h["groups"]["oxy"])
            s.group_create_from_indices("hyd", h["groups"]["hyd"])
            s.set_tuning(masked_selections=0)
            s.group_create_from_indices("listbig", h["groups"]["listbig"])
            s.set_tuning(masked_selections=1)
        self.s.add_bonds(h["bonds"])
        self.plans = {g: G.RMSDPlan(self.ref, self.s, g) for g in ("all", "big", "masked", "listbig", "small")}
        self.seg = {"mol": G.Segments.from_molecules(self.s), "resid": G.Segments.by_resid(self.s, h["resid"])}
        self.hb = G.HBondAnalysis(self.s, [G.HBondChain("oxy", "oxy", "hyd")], [(0, 0)], HB_DISTANCE, HB_ANGLE, h["bonds"])
        self.map = G.GridMap(self.s, (0.0, 6.0), (0.0, 6.4), (0.25, 0.25))
        self.ct = G.Contacts(self.s, "oxy", "hyd", CT_CUTOFF)
        self.region = G.Region(self.s, [G.Sphere(s["position"], s["radius"]) if s["kind"] == "sphere" else
                                        G.Cylinder(s["position"], s["radius"], s["height"], G.Dimension[s["orientation"].upper()]) for s in REGION_SPECS])
        # the trajectories the readers read: written by the host writers
        self.xtc_path, self.trr_path = os.path.join(self.tmp, "world.xtc"), os.path.join(self.tmp, "world.trr")
        if not os.path.isfile(self.xtc_path):
            box9 = np.array(BOX + [0] * 6, F)
            with G.XtcWriter(self.xtc_path) as wx, G.TrrWriter(self.trr_path) as wt:
                for f, x in enumerate(h["xtc_frames"]):
                    wx.write_frame(x, box9, step=10 * f, time=0.5 * f)
                    wt.write_frame(x[::-1].copy(), box9, step=10 * f, time=0.5 * f)
        self.xtc, self.trr = G.XtcFile(self.xtc_path), G.TrrFile(self.trr_path)
        self.n_written = 0
        self.made = {}            # the series objects, made on first use: a fresh world of another kind pays nothing for them
        self.s.sync()

    def _once(self, key, make):
        if key not in self.made:
            self.made[key] = make()
        return self.made[key]

    def fluct(self, group):
        return self._once(("fluct", group), lambda: self.G.Fluctuations(self.s, group))

    def covar(self, group):
        return self._once(("covar", group), lambda: self.G.Covariance(self.s, group))

    def msd(self, group):
        """`small` with nojump, `masked` lateral and as the positions stand"""
        kw = dict(dims="xyz", nojump=True) if group == "small" else dict(dims="xy", nojump=False)
        return self._once(("msd", group), lambda: self.G.MSD(self.s, group, SERIES_CAPACITY, **kw))

    def vcorr(self):
        return self._once(("vcorr",), lambda: self.G.VectorCorrelation(self.s, series_tuples()["pairs"], SERIES_CAPACITY, rank=(1, 2), pbc=True))

    def internals(self, which):
        tuples = series_tuples()[{"distance": "pairs", "angle": "angles", "dihedral": "dihedrals"}[which]]
        return self._once(("internals", which), lambda: self.G.Internals(self.s, which, tuples))

    def panel(self, which):
        group, capacity = {"big": ("big", SERIES_CAPACITY), "small": ("small", PANEL_SMALL_CAPACITY), "small16": ("small", SERIES_CAPACITY)}[which]
        return self._once(("panel", which), lambda: self.G.RMSDPanel(self.s, group, capacity))

    def segments(self, which):
        if which == "sizes" and which not in self.seg:
            self.seg[which] = self.G.Segments.from_lists(self.s, series_tuples()["sizes"])
        return self.seg[which]

    def close(self):
        for obj in self.made.values():
            obj.close()
        self.xtc.close(); self.trr.close()
        self.s.close(); self.ref.close()
        self.G.pinned_free(self._pin_ptr)

    # -- slots
    def load(self, slot, how, frame=None, box="pristine"):
        x = self.host["frames"][slot] if frame is None else frame
        b = self.host["boxes"][slot] if isinstance(box, str) else box
        if how == "set_frame":
            self.s.set_frame(x, b, slot=slot)
        else:
            self.pin[:] = x
            self.s.upload_async(self.pin, b, slot)
            self.s.upload_wait(slot)
        if frame is None and isinstance(box, str):
            self.dirty.discard(slot)
        else:
            self.dirty.add(slot)

    def need(self, slots, how):
        for slot in slots:
            if slot in self.dirty:
                self.load(slot, how)

    def tune(self, **kw):
        self.s.set_tuning(**kw)

    def untune(self, *keys):
        self.s.set_tuning(**{k: DEFAULT_TUNING[k] for k in keys})


def make_world(G, tmp_dir):
    return World(G, tmp_dir)


# ------------------------------------------------------------------ kinds
KINDS, META = {}, {}          # META[name] = dict(family, failing, lean)


def _exc(e):
    d = getattr(e, "detail", None)
    if isinstance(d, Exception):
        d = (type(d).__name__, getattr(d, "variant", None), repr(getattr(d, "detail", None)))
    elif d is not None and not isinstance(d, (int, str, tuple)):
        d = repr(d)
    return (type(e).__name__, getattr(e, "variant", None), d, getattr(e, "status", None))


def kind(name, family, slots=(), writes=(), failing=False, how="set_frame", lean=False):
    """register body(w, out) under `name`: `slots` are put back before it, `writes` (a subset) are read back after it"""
    def deco(body):
        def run(w):
            import groan_rs_amd as G
            w.need(slots, how)
            out = {}
            try:
                body(w, out)
                out["raised"] = None
            except (G.GroanError, G.XtcError) as e:
                if getattr(e, "status", None) == E_HIP:          # the device or the runtime failed: no result to compare, and nothing more to run
                    raise
                out["raised"] = _exc(e)                                 # (an atom index is the exception's detail)
            for slot in writes:
                out["pos%d" % slot] = w.s.get_positions(slot)
                b = w.s.get_box(slot)
                out["box%d" % slot] = None if b is None else np.array(b)
            w.dirty.update(writes)
            return out
        KINDS[name] = run
        META[name] = dict(family=family, failing=failing, lean=lean)
        return body
    return deco


R16 = tuple(range(16))
ORTHO8, TRIC8 = tuple(range(8)), tuple(range(8, 16))

# -- centres
_CALL = {(NAIVE, 0): "group_get_center_naive", (NAIVE, 1): "group_get_com_naive", (ESTIMATE, 0): "group_estimate_center", (ESTIMATE, 1): "group_estimate_com",
         (PBC, 0): "group_get_center", (PBC, 1): "group_get_com"}
for _g in ("small", "big", "masked"):
    for _k, _w in CENTRES:
        def _one(w, out, g=_g, k=_k, wt=_w):
            out["c3"] = getattr(w.s, _CALL[(k, wt)])(g, slot=3)
            out["c11"] = getattr(w.s, _CALL[(k, wt)])(g, slot=11)
        kind("center_%s_%d%d" % (_g, _k, _w), "centres", slots=(3, 11))(_one)

        def _batch(w, out, g=_g, k=_k, wt=_w):
            out["c"], out["st"] = w.s.group_center_batch(g, k, wt, 0, 16)
        kind("center_batch_%s_%d%d" % (_g, _k, _w), "centres", slots=R16, how="upload")(_batch)


@kind("group_distance", "centres", slots=(3, 11))
def _(w, out):
    D = w.G.Dimension
    out["d"] = F(w.s.group_distance("small", "b400", D.XYZ, slot=3))                # both small: one dispatch, two words
    out["dxy"] = F(w.s.group_distance("small", "big", D.XY, slot=11))


@kind("atoms_center_small", "centres", slots=(3,), writes=(3,))
def _(w, out):
    w.s.atoms_center("small", w.G.Dimension.XYZ, slot=3)


@kind("atoms_center_mass_big", "centres", slots=(11,), writes=(11,), how="upload")
def _(w, out):
    w.s.atoms_center_mass("big", w.G.Dimension.XY, slot=11)


def _center_batch(resident, weighted, slots):
    def body(w, out):
        w.tune(center_resident=resident, resident=2 if resident else 0)
        try:
            before = (w.s.stat("center_res_launches"), w.s.stat("res_lean_segments"))
            out["st"] = w.s.atoms_center_batch("big", slots[0], len(slots), w.G.Dimension.XYZ, weighted=weighted)
            out["launches"] = w.s.stat("center_res_launches") - before[0]
            out["lean"] = w.s.stat("res_lean_segments") - before[1]
        finally:
            w.untune("center_resident", "resident")
    return body


kind("atoms_center_batch_res", "centres", slots=ORTHO8, writes=ORTHO8, lean=True)(_center_batch(1, False, ORTHO8))
kind("atoms_center_mass_batch_res", "centres", slots=TRIC8, writes=TRIC8, how="upload", lean=True)(_center_batch(1, True, TRIC8))
kind("atoms_center_batch_two", "centres", slots=ORTHO8, writes=ORTHO8)(_center_batch(0, False, ORTHO8))
kind("atoms_center_mass_batch_two", "centres", slots=TRIC8, writes=TRIC8)(_center_batch(0, True, TRIC8))


def _move_batch(call, slots, rows):
    def body(w, out):
        w.tune(translate_rows=rows)
        try:
            if call == "translate":
                out["st"] = w.s.group_translate_batch("big", [1.7, -2.9, 0.45], slots[0], len(slots))
            else:
                out["st"] = w.s.group_wrap_batch("big", slots[0], len(slots))
        finally:
            w.untune("translate_rows")
    return body


for _call in ("translate", "wrap"):
    kind("%s_batch_ortho_rows1" % _call, "centres", slots=ORTHO8, writes=ORTHO8)(_move_batch(_call, ORTHO8, 1))
    kind("%s_batch_ortho_rows0" % _call, "centres", slots=ORTHO8, writes=ORTHO8, how="upload")(_move_batch(_call, ORTHO8, 0))
    kind("%s_batch_tric" % _call, "centres", slots=TRIC8, writes=TRIC8)(_move_batch(_call, TRIC8, 1))


@kind("group_translate_small", "centres", slots=(3,), writes=(3,))
def _(w, out):
    w.s.group_translate("small", [4.0, -7.0, 0.3], slot=3)


@kind("group_wrap_all", "centres", slots=(3,), writes=(3,))
def _(w, out):
    w.s.group_translate("all", [-0.4, 0.3, 9.0], slot=3)
    w.s.group_wrap("all", slot=3)


@kind("fail_translate_nan_small", "centres", writes=(3,), failing=True)
def _(w, out):
    w.load(3, "set_frame", frame=nan_frame(3, NAN_SMALL))
    w.s.group_translate("small", [0.1, 0.2, 0.3], slot=3)


@kind("fail_com_nan_big", "centres", writes=(11,), failing=True)
def _(w, out):
    w.load(11, "upload", frame=nan_frame(11, NAN_BIG))
    out["c"] = w.s.group_get_com("big", slot=11)


@kind("fail_translate_nan_tail", "centres", writes=(3,), failing=True)
def _(w, out):
    w.load(3, "set_frame", frame=nan_frame(3, NAN_TAIL))
    w.s.group_translate("all", [0.1, 0.2, 0.3], slot=3)


@kind("fail_center_nobox", "centres", slots=(3,), writes=(3,), failing=True)
def _(w, out):
    w.s.reset_box(slot=3)
    w.dirty.add(3)
    out["c"] = w.s.group_get_center("big", slot=3)


@kind("fail_center_nogroup", "centres", slots=(3,), failing=True)
def _(w, out):
    out["c"] = w.s.group_get_com("nobody", slot=3)


@kind("fail_center_batch_mixed", "centres", writes=(0, 1, 2, 3, 4, 5), failing=True)
def _(w, out):
    w.need((0, 1, 3, 4, 5), "set_frame")
    w.load(2, "set_frame", box=None)
    w.load(4, "set_frame", frame=nan_frame(4, NAN_BIG))
    out["c"], out["st"] = w.s.group_get_com_batch("big", 0, 6, raise_on_error=False)


# -- RMSD
@kind("calc_rmsd_small", "rmsd", slots=(3,))
def _(w, out):
    out["r"], out["R"] = w.s.calc_rmsd(w.ref, "small", slot=3, return_rotation=True)
    out["r"] = F(out["r"])


@kind("calc_rmsd_fit_small", "rmsd", slots=(11,), writes=(11,), how="upload")
def _(w, out):
    out["r"] = F(w.s.calc_rmsd_and_fit(w.ref, "small", slot=11))


def _plan_rmsd(group):
    def body(w, out):
        w.tune(resident=0)
        try:
            out["r"], out["st"], out["R"] = w.plans[group].rmsd(0, 16, return_rotation=True)
        finally:
            w.untune("resident")
    return body


def _plan_fit(group, fuse):
    def body(w, out):
        w.tune(resident=0, fuse=fuse)
        try:
            out["r"], out["st"] = w.plans[group].rmsd_fit(0, 16)
        finally:
            w.untune("resident", "fuse")
    return body


for _g in ("all", "big", "masked", "listbig"):
    kind("plan_rmsd_%s" % _g, "rmsd", slots=R16)(_plan_rmsd(_g))
    kind("plan_fit_%s_fuse1" % _g, "rmsd", slots=R16, writes=R16)(_plan_fit(_g, 1))
    kind("plan_fit_%s_fuse0" % _g, "rmsd", slots=R16, writes=R16, how="upload")(_plan_fit(_g, 0))


def _res_fit(nf):
    def body(w, out):
        w.tune(resident=2)
        try:
            before = (w.s.stat("res_launches"), w.s.stat("res_lean_segments"))
            out["r"], out["st"] = w.plans["all"].rmsd_fit(0, nf)
            out["launches"] = w.s.stat("res_launches") - before[0]
            out["lean"] = w.s.stat("res_lean_segments") - before[1]
        finally:
            w.untune("resident")
    return body


for _nf in (3, 9, 2):
    kind("res_fit_%d" % _nf, "rmsd", slots=tuple(range(_nf)), writes=tuple(range(_nf)), lean=True)(_res_fit(_nf))


@kind("plan_begin_end", "rmsd", slots=ORTHO8, writes=ORTHO8)
def _(w, out):
    w.plans["big"].begin(0, 8, True)
    out["r"], out["st"] = w.plans["big"].end()


@kind("fail_fit_mixed_fused", "rmsd", writes=tuple(range(9)), failing=True)
def _(w, out):
    w.need((0, 1, 3, 4, 6, 7, 8), "set_frame")
    w.load(2, "set_frame", box=None)
    w.load(5, "set_frame", frame=nan_frame(5, 4321))
    w.tune(resident=0, fuse=1)
    try:
        out["r"], out["st"] = w.plans["all"].rmsd_fit(0, 9, raise_on_error=False)
    finally:
        w.untune("resident", "fuse")


@kind("fail_rmsd_nan_small", "rmsd", writes=(3,), failing=True)
def _(w, out):
    w.load(3, "set_frame", frame=nan_frame(3, NAN_SMALL))
    out["r"] = F(w.s.calc_rmsd(w.ref, "small", slot=3))


@kind("fail_rmsd_nogroup", "rmsd", slots=(3,), failing=True)
def _(w, out):
    out["r"] = F(w.s.calc_rmsd(w.ref, "nobody", slot=3))


# -- pair distances
@kind("atoms_distance", "pairs", slots=(3, 11))
def _(w, out):
    D = w.G.Dimension
    out["d"] = np.array([w.s.atoms_distance(3, 11777, D.XYZ, slot=3), w.s.atoms_distance(0, N - 1, D.XYZ, slot=11), w.s.atoms_distance(5000, 77, D.YZ, slot=11)], F)


def _alldist(g1, g2, slot):
    def body(w, out):
        out["d"] = w.s.group_all_distances(g1, g2, slot=slot)
    return body


kind("alldist_40x50", "pairs", slots=(3,))(_alldist("a40", "b50", 3))
kind("alldist_300x400", "pairs", slots=(11,))(_alldist("a300", "b400", 11))
kind("alldist_masked_self", "pairs", slots=(11,))(_alldist("masked", "masked", 11))
kind("alldist_small_self", "pairs", slots=(3,))(_alldist("small", "small", 3))


@kind("alldist_batch_device_40x50", "pairs", slots=(6, 7, 8, 9))
def _(w, out):
    dev, n1, n2, out["st"] = w.s.group_all_distances_batch_device("a40", "b50", 6, 4)
    out["d"] = w.s.device_read(dev, 0, (4, n1, n2))


def _reduce(op, **kw):
    def body(w, out):
        out["v"], out["st"] = w.s.group_all_distances_reduce("a300", "b400", op, first_slot=6, n_frames=4, **kw)
    return body


kind("reduce_max", "pairs", slots=(6, 7, 8, 9))(_reduce("max"))
kind("reduce_min_rows", "pairs", slots=(6, 7, 8, 9))(_reduce("min", per_row=True))
kind("reduce_count_rows", "pairs", slots=(6, 7, 8, 9))(_reduce("count_below", per_row=True, param=1.5))
kind("reduce_hist", "pairs", slots=(6, 7, 8, 9))(_reduce("hist", param=3.0, nbins=97))


@kind("iter_all_distances", "pairs", slots=(11,))
def _(w, out):
    out["d"] = w.s.group_iter("a40", slot=11).all_distances(w.s.group_iter("list", slot=11))


@kind("pairs_within", "pairs", slots=(3,))
def _(w, out):
    out["i"], out["j"], out["d"] = w.s.group_pairs_within("small", "big", 0.9, slot=3)


@kind("geometries_small_all_small", "pairs", slots=(3,))
def _(w, out):
    G = w.G
    shapes = [G.Sphere([0.3, 0.2, 0.2], 1.4)]
    try:
        for k, src in enumerate(("small", "all", "small")):
            w.s.group_create_from_geometries("geo", src, shapes, slot=3)
            out["blocks%d" % k] = np.array(w.s.group_container("geo").blocks, np.uint64)
            w.s.group_remove("geo")
    finally:
        if w.s.group_exists("geo"):
            w.s.group_remove("geo")


def _contacts_lists(w, out):
    out["off"], out["i"], out["j"], out["d"] = w.ct.lists()


@kind("contacts_pairs_8", "pairs", slots=ORTHO8)
def _(w, out):
    out["n"], out["st"] = w.ct.pairs(0, 8)
    _contacts_lists(w, out)


@kind("contacts_hist_tric_8", "pairs", slots=TRIC8)
def _(w, out):
    out["h"], out["st"] = w.ct.hist(8, 8, CT_BINS)


@kind("contacts_counts_1", "pairs", slots=(11,))
def _(w, out):
    out["per_atom"], out["n"], out["st"] = w.ct.counts(11, 1)


def _region_lists(w, out):
    out["off"], out["atoms"] = w.region.lists()


@kind("region_select_16", "pairs", slots=R16, how="upload")
def _(w, out):
    out["n"], out["st"] = w.region.select("all", 0, 16)
    _region_lists(w, out)


@kind("region_anchored_8", "pairs", slots=tuple(range(4, 12)))
def _(w, out):
    out["anchors"], out["cst"] = w.s.group_center_batch("small", PBC, 0, 4, 8)      # the shapes are moved by the centre of `small`, frame by frame
    out["n"], out["st"] = w.region.select("big", 4, 8, anchors=out["anchors"])
    _region_lists(w, out)


@kind("fail_contacts_nan", "pairs", writes=(3,), failing=True)
def _(w, out):
    w.need((2, 4, 5), "set_frame")
    w.load(3, "set_frame", frame=nan_frame(3, NAN_A40))                             # atom 20: a hydrogen, in group 2 of the search
    out["n"], out["st"] = w.ct.pairs(2, 4, raise_on_error=False)
    _contacts_lists(w, out)


@kind("fail_alldist_skewed", "pairs", slots=(3,), writes=(3,), failing=True)
def _(w, out):
    w.s.set_box(FLAT, slot=3)
    w.dirty.add(3)
    out["d"] = w.s.group_all_distances("a40", "b50", slot=3)


@kind("fail_alldist_nan", "pairs", writes=(3,), failing=True)
def _(w, out):
    w.load(3, "upload", frame=nan_frame(3, NAN_A40))
    out["d"] = w.s.group_all_distances("a40", "b50", slot=3)


@kind("fail_reduce_mixed", "pairs", writes=(6, 7, 8, 9), failing=True)
def _(w, out):
    w.need((6, 9), "set_frame")
    w.load(7, "set_frame", box=None)
    w.load(8, "set_frame", frame=nan_frame(8, 350))
    out["v"], out["st"] = w.s.group_all_distances_reduce("a300", "b400", "hist", param=3.0, nbins=97, first_slot=6, n_frames=4, raise_on_error=False)


@kind("fail_pairs_nogroup", "pairs", slots=(3,), failing=True)
def _(w, out):
    out["d"] = w.s.group_all_distances("a40", "nobody", slot=3)


# -- topology
@kind("whole_mols", "topology", slots=R16, writes=R16)
def _(w, out):
    out["st"] = w.s.make_molecules_whole_batch(0, 16)


@kind("whole_group_big", "topology", slots=R16, writes=R16, how="upload")
def _(w, out):
    out["st"] = w.s.make_group_whole_batch("big", 0, 16)


@kind("rebond_whole", "topology", slots=R16, writes=R16)
def _(w, out):
    try:
        w.s.clear_bonds()
        out["no_bonds"] = int(w.s.has_bonds())
        w.s.add_bonds(w.host["bonds_alt"])
        out["st"] = w.s.make_molecules_whole_batch(0, 16)
    finally:
        w.s.clear_bonds()
        w.s.add_bonds(w.host["bonds"])


def _segments(which, first, nf):
    def body(w, out):
        out["c"], out["st"] = w.seg[which].centers(first, nf, PBC, 1)
    return body


for _which in ("mol", "resid"):
    kind("seg_%s_2" % _which, "topology", slots=(7, 8))(_segments(_which, 7, 2))
    kind("seg_%s_9" % _which, "topology", slots=tuple(range(4, 13)))(_segments(_which, 4, 9))
    kind("seg_%s_1" % _which, "topology", slots=(11,))(_segments(_which, 11, 1))


def _hbonds(first, nf):
    def body(w, out):
        r = w.hb.batch(first, nf)
        for name, a in zip(("donor", "hydrogen", "acceptor", "distance", "angle", "offsets", "st"), r):
            out[name] = a
    return body


kind("hbond_2", "topology", slots=(7, 8))(_hbonds(7, 2))
kind("hbond_8", "topology", slots=tuple(range(4, 12)))(_hbonds(4, 8))
kind("hbond_1", "topology", slots=(3,))(_hbonds(3, 1))


@kind("gridmap", "topology", slots=ORTHO8)
def _(w, out):
    w.map.clear()
    out["outside"], out["st"] = w.map.accumulate("all", 0, 8, value=w.G.Dimension.Z)
    out["counts"], out["sums_q"], out["mean"] = w.map.counts, w.map.sums_q, w.map.mean()


@kind("fail_seg_nobox", "topology", writes=(4, 5, 6, 7), failing=True)
def _(w, out):
    w.need((4, 6, 7), "set_frame")
    w.load(5, "set_frame", box=None)
    out["c"], out["st"] = w.seg["mol"].centers(4, 4, PBC, 1, raise_on_error=False)


@kind("fail_whole_nan", "topology", writes=(3,), failing=True)
def _(w, out):
    w.load(3, "set_frame", frame=nan_frame(3, NAN_BIG))
    w.s.make_molecules_whole(slot=3)


@kind("fail_hbond_mixed", "topology", writes=(4, 5, 6), failing=True)
def _(w, out):
    w.need((4,), "set_frame")
    w.load(5, "set_frame", box=None)
    w.load(6, "set_frame", frame=nan_frame(6, NAN_BIG))
    r = w.hb.batch(4, 3, raise_on_error=False)
    for name, a in zip(("donor", "hydrogen", "acceptor", "distance", "angle", "offsets", "st"), r):
        out[name] = a


def _gyration(which, first, nf, axes, piece=0):
    def body(w, out):
        seg = w.segments(which)
        if piece:                                          # (sticky: put back below; a kind without a piece size takes the object as it finds it)
            seg.set_piece_frames(piece)
        try:
            g = seg.gyration(first, nf, axes=axes)
        finally:
            if piece:
                seg.set_piece_frames(0)
        out["moments"], out["st"] = g.moments, g.status
        if axes:
            out["raw_axes"] = g.raw_axes
    return body


kind("gyr_mol_9_axes", "topology", slots=tuple(range(4, 13)))(_gyration("mol", 4, 9, True))
kind("gyr_resid_2", "topology", slots=(7, 8), how="upload")(_gyration("resid", 7, 2, False))
kind("gyr_sizes_16_axes", "topology", slots=R16, how="upload")(_gyration("sizes", 0, 16, True))
kind("gyr_mol_9_pieces", "topology", slots=tuple(range(4, 13)))(_gyration("mol", 4, 9, True, piece=2))


@kind("gyr_sizes_device_4", "topology", slots=(6, 7, 8, 9), how="upload")
def _(w, out):
    seg = w.segments("sizes")
    mom, ax, out["st"] = seg.gyration_device(6, 4, axes=True)
    out["moments"], out["raw_axes"] = w.s.device_read(mom, 0, (4, len(seg), 10)), w.s.device_read(ax, 0, (4, len(seg), 12))


@kind("fail_gyr_mixed", "topology", writes=(5, 6), failing=True)
def _(w, out):
    w.need((4, 7, 8), "set_frame")
    w.load(5, "set_frame", box=None)                                                # the pieces are slots 4-5, 6-7 and 8: one failure on either side of the first boundary
    w.load(6, "set_frame", frame=nan_frame(6, NAN_BIG))
    seg = w.segments("mol")
    seg.set_piece_frames(2)
    try:
        g = seg.gyration(4, 5, axes=True, raise_on_error=False)
    finally:
        seg.set_piece_frames(0)
    out["moments"], out["raw_axes"], out["st"] = g.moments, g.raw_axes, g.status


# -- series: the objects that keep state over the frames handed to them.  Every kind starts with clear()
def _fluct_state(f, out, tag=""):
    out["origin" + tag], out["sum" + tag], out["sq" + tag], out["n" + tag] = f.raw()
    out["mean" + tag], out["rmsf" + tag], out["n_frames" + tag] = f.mean(), f.rmsf(), f.n_frames


def _fluct(group, calls):
    def body(w, out):
        f = w.fluct(group)
        f.clear()
        out["cleared_origin"], out["cleared_n"] = f.raw()[0], f.n_frames
        out["st"] = np.concatenate([f.accumulate(first, nf) for first, nf in calls])
        _fluct_state(f, out)
    return body


kind("fluct_small_8", "series", slots=ORTHO8)(_fluct("small", [(0, 8)]))
kind("fluct_masked_16", "series", slots=R16, how="upload")(_fluct("masked", [(0, 16)]))
kind("fluct_list_tric_8", "series", slots=TRIC8, how="upload")(_fluct("list", [(8, 8)]))
kind("fluct_two_calls", "series", slots=R16)(_fluct("list", [(0, 5), (5, 11)]))


@kind("fail_fluct_nan", "series", writes=(4,), failing=True)
def _(w, out):
    w.need((1, 2, 3, 5, 6, 7, 8), "set_frame")
    w.load(4, "set_frame", frame=nan_frame(4, NAN_SMALL))
    f = w.fluct("small")
    f.clear()
    f.accumulate(1, 3); f.accumulate(5, 4)                                          # the call below without its failed frame
    _fluct_state(f, out, "_without")
    f.clear()
    out["st"] = f.accumulate(1, 8, raise_on_error=False)                            # the object's last call: 8 frames, one of them failed
    _fluct_state(f, out)


def _covar_state(cv, out):
    out["origin"], out["sum"], out["q"], out["n"] = cv.raw()
    out["cov"], out["cov_mw"], out["dccm"], out["mean"] = cv.matrix(), cv.matrix(mass_weighted=True), cv.dccm(), cv.mean()


def _covar(group, first, nf):
    def body(w, out):
        cv = w.covar(group)
        cv.clear()
        out["st"] = cv.accumulate(first, nf)
        _covar_state(cv, out)
    return body


kind("covar_small_16", "series", slots=R16)(_covar("small", 0, 16))
kind("covar_a300_tric_8", "series", slots=TRIC8, how="upload")(_covar("a300", 8, 8))


@kind("fail_covar_all_bad", "series", writes=(2, 3), failing=True)
def _(w, out):
    w.need((4, 5, 6, 7), "set_frame")
    w.load(2, "set_frame", frame=nan_frame(2, 310))
    w.load(3, "set_frame", frame=nan_frame(3, 599))
    cv = w.covar("a300")
    cv.clear()
    out["st"] = cv.accumulate(2, 2, raise_on_error=False)
    out["n_bad"] = cv.n_frames
    out["st_good"] = cv.accumulate(4, 4)                                            # the origin is this call's first frame
    _covar_state(cv, out)


def _msd_state(m, out, tag=""):
    out["disp" + tag], out["from_origin" + tag] = m.displacements(0, m.n_frames), m.from_origin()
    out["msd" + tag], out["pairs" + tag] = m.msd()
    out["msd3" + tag], out["pairs3" + tag] = m.msd(3)
    out["n_pad"] = m.stat(LIB.MSD_STAT_N_PAD)


def _msd(group, calls):
    def body(w, out):
        m = w.msd(group)
        m.clear()
        out["st"] = np.concatenate([m.append(first, nf) for first, nf in calls])
        _msd_state(m, out)
    return body


kind("msd_small_ortho_8", "series", slots=ORTHO8)(_msd("small", [(0, 8)]))
kind("msd_masked_tric_8", "series", slots=TRIC8, how="upload")(_msd("masked", [(8, 8)]))
kind("msd_appended_in_three", "series", slots=ORTHO8)(_msd("small", [(0, 3), (3, 1), (4, 4)]))


@kind("fail_msd_nobox", "series", writes=(2,), failing=True)
def _(w, out):
    w.need((0, 1, 3), "set_frame")
    w.load(2, "set_frame", box=None)
    m = w.msd("small")
    m.clear()
    out["st"] = m.append(0, 4, raise_on_error=False)                                # nojump needs the frame's box
    _msd_state(m, out)


@kind("fail_msd_capacity", "series", slots=ORTHO8, failing=True)
def _(w, out):
    m = w.msd("small")
    m.clear()
    st = [m.append(0, 8), m.append(0, 8)]                                           # full
    _msd_state(m, out, "_before")
    try:
        m.append(0, 1)
        refused = 0
    except w.G.GroanError as e:
        out["refused"], refused = _exc(e), e.status
    out["st"] = np.concatenate(st + [[refused]]).astype(np.int32)                   # the frames' statuses, then the refused call's
    out["n_frames"] = m.n_frames
    _msd_state(m, out)


def _vcorr_state(v, out):
    out["vectors"] = v.vectors(0, v.n_frames)
    out["c1"], out["c2"], out["pairs"] = v.correlate()
    out["each1"], out["each2"] = v.correlate_each(4)
    out["n_pad"] = v.stat(LIB.VCORR_STAT_N_PAD)


def _vcorr(first, nf):
    def body(w, out):
        v = w.vcorr()
        v.clear()
        out["st"] = v.append(first, nf)
        _vcorr_state(v, out)
    return body


kind("vcorr_ortho_8", "series", slots=ORTHO8, how="upload")(_vcorr(0, 8))
kind("vcorr_tric_8", "series", slots=TRIC8)(_vcorr(8, 8))


@kind("fail_vcorr_nan", "series", writes=(2,), failing=True)
def _(w, out):
    w.need((0, 1, 3), "set_frame")
    w.load(2, "upload", frame=nan_frame(2, NAN_SERIES))
    v = w.vcorr()
    v.clear()
    out["st"] = v.append(0, 4, raise_on_error=False)
    _vcorr_state(v, out)


def _internals(which, first, nf):
    def body(w, out):
        out["v"], out["st"] = w.internals(which).values(first, nf)
    return body


kind("internals_distance_16", "series", slots=R16)(_internals("distance", 0, 16))
kind("internals_angle_16", "series", slots=R16, how="upload")(_internals("angle", 0, 16))
kind("internals_dihedral_8", "series", slots=ORTHO8, how="upload")(_internals("dihedral", 0, 8))


def _internals_state(ic, out, tag):
    out["mean_" + tag], out["var_" + tag] = ic.read()
    out["origin_" + tag], out["sum_" + tag], out["sq_" + tag], out["n_" + tag] = ic.read_raw()


@kind("internals_accumulate_16", "series", slots=R16)
def _(w, out):
    st = []
    for which in ("angle", "dihedral"):
        ic = w.internals(which)
        ic.clear()
        st.append(ic.accumulate(0, 16))
        _internals_state(ic, out, which)
    out["st"] = np.concatenate(st)
    out["v_dihedral"] = w.internals("dihedral").values(0, 16)[0]                    # the rows the sums are made of (slots 8-15: no other kind returns them)


@kind("fail_internals_nan", "series", writes=(5,), failing=True)
def _(w, out):
    w.need((4, 6), "set_frame")
    w.load(5, "set_frame", frame=nan_frame(5, int(series_tuples()["dihedrals"][3, 3])))
    ic = w.internals("dihedral")
    out["v"], out["st_values"] = ic.values(4, 3, raise_on_error=False)
    ic.clear()
    out["st"] = ic.accumulate(4, 3, raise_on_error=False)
    _internals_state(ic, out, "dihedral")


def _panel_state(w, p, out):
    out["status"], out["m"] = p.status, w.G.rmsd_matrix(p)


@kind("panel_big_16", "series", slots=R16)
def _(w, out):
    p = w.panel("big")
    p.clear()
    out["st"] = p.append(0, 16)
    _panel_state(w, p, out)


@kind("panel_big_small_cols", "series", slots=R16, how="upload")
def _(w, out):
    big, rows, cols = w.panel("big"), w.panel("small16"), w.panel("small")
    for p in (big, rows, cols):
        p.clear()
    out["st"] = np.concatenate([big.append(8, 8), rows.append(0, 16), cols.append(4, 8)])
    out["m_big"] = w.G.rmsd_matrix(big)
    out["m"] = w.G.rmsd_matrix(rows, cols)
    out["m_t"] = w.G.rmsd_matrix(cols, rows)
    try:                                                                            # panels of different groups are refused, and nothing changes
        w.G.rmsd_matrix(big, cols)
    except w.G.GroanError as e:
        out["refused"] = _exc(e)
    out["m_again"] = w.G.rmsd_matrix(rows, cols)


@kind("panel_device", "series", slots=TRIC8)
def _(w, out):
    p = w.panel("big")
    p.clear()
    out["st"] = p.append(8, 8)
    dev, nr, nc = w.G.rmsd_matrix(p, device=True)
    out["shape"], out["m"] = (nr, nc), w.s.device_read(dev, 0, (nr, nc))
    out["status"] = p.status


@kind("fail_panel_nan", "series", writes=(3,), failing=True)
def _(w, out):
    w.need((2, 4), "set_frame")
    w.load(3, "set_frame", frame=nan_frame(3, NAN_BIG))
    p = w.panel("big")
    p.clear()
    out["st"] = p.append(2, 3, raise_on_error=False)                                # the failed frame takes a row all the same
    out["len"] = len(p)
    _panel_state(w, p, out)


@kind("fail_panel_masses", "series", slots=(0, 1, 2, 3), failing=True)
def _(w, out):
    p = w.panel("big")
    p.clear()
    other = (w.host["masses"][::-1] * F(1.5)).astype(F)
    refused = 0
    try:
        w.s.set_masses(other)
        p.append(0, 2)
    except w.G.GroanError as e:
        out["refused"], refused = _exc(e), e.status
    finally:
        w.s.set_masses(w.host["masses"])
    out["len_refused"] = len(p)
    out["st"] = np.concatenate([[refused], p.append(0, 4)]).astype(np.int32)        # the refused call's status, then the frames of the good one
    _panel_state(w, p, out)


# -- trajectory I/O
def _xtc_write(count, repeat):
    def body(w, out):
        for k in range(count * repeat):
            w.s.copy_frame(SPOOL + k, k % count)
        w.tune(xtc_device_encode=1)
        took = w.s.stat("xtc_device_frames")
        w.n_written += 1
        path = os.path.join(w.tmp, "out_%d_%d.xtc" % (id(w), w.n_written))
        nf = count * repeat
        with w.G.XtcWriter(path) as wr:
            wr.write_slots(w.s, SPOOL, nf, steps=np.arange(nf, dtype=np.int64) * 10, times=np.arange(nf, dtype=F) * 0.5, host_threads=2)
        out["device_frames"] = w.s.stat("xtc_device_frames") - took
        out["bytes"] = open(path, "rb").read()
        os.remove(path)
    return body


kind("xtc_write_4", "io", slots=(0, 1, 2, 3))(_xtc_write(4, 5))
kind("xtc_write_12", "io", slots=tuple(range(12)), how="upload")(_xtc_write(12, 2))


def _xtc_read(group, first, nf):
    def body(w, out):
        out["steps"], out["times"] = w.xtc.read_frames_device(w.s, first, nf, first_slot=0, group=group)
    return body


kind("xtc_read_small", "io", slots=(0, 1, 2, 3), writes=(0, 1, 2, 3))(_xtc_read("small", 0, 4))
kind("xtc_read_full", "io", slots=(0, 1, 2, 3, 4), writes=(0, 1, 2, 3, 4), how="upload")(_xtc_read(None, 1, 5))
kind("xtc_read_masked", "io", slots=(0, 1, 2), writes=(0, 1, 2))(_xtc_read("masked", 3, 3))
kind("xtc_read_full_again", "io", slots=(0, 1), writes=(0, 1))(_xtc_read(None, 4, 2))


@kind("xtc_read_small_redefined", "io", slots=(0, 1, 2, 3), writes=(0, 1, 2, 3))
def _(w, out):
    try:
        w.s.group_remove("small")
        w.s.group_create_from_ranges("small", [SMALL_XTC])
        out["steps"], out["times"] = w.xtc.read_frames_device(w.s, 0, 4, first_slot=0, group="small")
    finally:
        if w.s.group_exists("small"):
            w.s.group_remove("small")
        w.s.group_create_from_ranges("small", [SMALL])


@kind("trr_read", "io", slots=(0, 1, 2, 3, 4, 5), writes=(0, 1, 2, 3, 4, 5))
def _(w, out):
    out["steps"], out["times"] = w.trr.read_frames_device(w.s, 0, 6, first_slot=0)


@kind("fail_xtc_range", "io", slots=(0, 1), writes=(0, 1), failing=True)
def _(w, out):
    out["steps"], out["times"] = w.xtc.read_frames_device(w.s, N_XTC - 1, 2, first_slot=0)


@kind("fail_xtc_nogroup", "io", slots=(0,), writes=(0,), failing=True)
def _(w, out):
    out["steps"], out["times"] = w.xtc.read_frames_device(w.s, 0, 1, first_slot=0, group="nobody")


# -- redefinitions
@kind("fail_redefined_small_plan", "redef", slots=(3,), failing=True)
def _(w, out):
    try:
        w.s.group_remove("small")
        w.s.group_create_from_ranges("small", [SMALL_OTHER])
        out["c"] = w.s.group_get_com("small", slot=3)
        out["r"], out["st"] = w.plans["small"].rmsd(3, 1)
    finally:
        if w.s.group_exists("small"):
            w.s.group_remove("small")
        w.s.group_create_from_ranges("small", [SMALL])


@kind("fail_redef_nogroup", "redef", slots=(3,), failing=True)
def _(w, out):
    w.s.group_remove("nobody")


@kind("restored_small_plan", "redef", slots=(3, 11))
def _(w, out):
    w.s.group_remove("small")
    w.s.group_create_from_ranges("small", [SMALL_OTHER])
    w.s.group_remove("small")
    w.s.group_create_from_ranges("small", [SMALL])
    out["r"], out["st"] = w.plans["small"].rmsd(3, 1)
    out["r11"], out["st11"] = w.plans["small"].rmsd(11, 1)
    out["c"] = w.s.group_get_com("small", slot=3)


@kind("masses_changed", "redef", slots=(3,))
def _(w, out):
    other = (w.host["masses"][::-1] * F(1.5)).astype(F)
    try:
        w.s.set_masses(other)
        out["c_other"] = w.s.group_get_com("big", slot=3)
        out["s_other"] = w.s.group_get_com("small", slot=3)
    finally:
        w.s.set_masses(w.host["masses"])
    out["c"] = w.s.group_get_com("big", slot=3)
    out["s"] = w.s.group_get_com("small", slot=3)


@kind("tune_small_calls0", "redef", slots=(3,))
def _(w, out):
    w.tune(small_calls=0)
    try:
        before = w.s.stat("small_calls")
        out["c"] = w.s.group_get_com("small", slot=3)
        out["d"] = F(w.s.group_distance("small", "a40", slot=3))
        out["small_calls"] = w.s.stat("small_calls") - before
    finally:
        w.untune("small_calls")
    out["c_again"] = w.s.group_get_com("small", slot=3)


@kind("tune_pairsym0", "redef", slots=(3,))
def _(w, out):
    w.tune(pairdist_symmetric=0)
    try:
        out["d"] = w.s.group_all_distances("small", "small", slot=3)
    finally:
        w.untune("pairdist_symmetric")


@kind("tune_masked0", "redef", slots=R16)
def _(w, out):
    w.tune(masked_selections=0)
    try:
        out["c"], out["st"] = w.s.group_get_com_batch("masked", 0, 16)
        out["r"], out["rst"] = w.plans["masked"].rmsd(0, 4)
    finally:
        w.untune("masked_selections")


# ------------------------------------------------------------------ schedules
ADJACENCIES = {
    1: ["fail_translate_nan_small", "atoms_center_small", "group_wrap_all", "fail_translate_nan_small"],
    2: ["fail_fit_mixed_fused", "plan_fit_all_fuse1", "res_fit_9", "atoms_center_batch_res"],
    3: ["group_distance", "center_small_21", "calc_rmsd_small", "group_distance"],
    4: ["atoms_distance", "reduce_hist", "alldist_300x400", "alldist_batch_device_40x50", "reduce_count_rows", "alldist_40x50"],
    5: ["xtc_read_small", "xtc_read_small_redefined", "trr_read", "xtc_read_full"],
    6: ["fail_seg_nobox", "seg_mol_9", "seg_mol_1"],
    7: ["hbond_2", "hbond_8", "hbond_1"],
    8: ["whole_mols", "rebond_whole", "whole_mols"],
    9: ["res_fit_3", "plan_rmsd_masked", "res_fit_9", "plan_rmsd_masked", "res_fit_2"],
    10: ["fail_contacts_nan", "contacts_pairs_8", "region_select_16", "contacts_pairs_8"],
    # 11: the verdict block of an object and its "skip" tail, reused by every call (GrVerdicts): a call of as many frames as the failed
    #     one before it on the same object; clear() behind a failed call gives the origin back
    11: ["fail_fluct_nan", "fluct_masked_16", "fluct_small_8", "fluct_masked_16"],
    # 12: RMSDPanel.append packs through the context's shared state words (states_from_prechecks, pbc_center_stages, fetch_states):
    #     the resident kinds behind it must still start lean, the plans still read their own states
    12: ["res_fit_9", "panel_big_16", "res_fit_3", "plan_rmsd_big", "panel_big_16", "atoms_center_batch_res"],
    # 13: the panel looks at its weights again only when the context's epoch has moved; Covariance keeps the masses it was made with
    13: ["masses_changed", "panel_big_16", "fail_panel_masses", "panel_big_16", "covar_small_16"],
    # 14: every series object keeps a snapshot (GrSnapshot) of its group, which is replaced and put back around it
    14: ["fail_redefined_small_plan", "fluct_small_8", "msd_small_ortho_8", "restored_small_plan", "covar_small_16"],
    # 15: gyration and centers share key_dev, ok_dev, ok_host and the launch statistics of one Segments object; piece_frames is sticky
    15: ["seg_mol_9", "gyr_mol_9_pieces", "seg_mol_1", "gyr_mol_9_axes", "fail_seg_nobox", "gyr_mol_9_axes", "fail_gyr_mixed", "seg_mol_9"],
    # 16: the grow-only gyr block grows and is then reused by a smaller call
    16: ["gyr_sizes_16_axes", "gyr_sizes_device_4", "gyr_resid_2", "gyr_sizes_16_axes"],
    # 17: the band scratch of the Gram kernel and the panels of the two band objects (MSD, VectorCorrelation)
    17: ["msd_masked_tric_8", "vcorr_tric_8", "msd_appended_in_three", "vcorr_ortho_8"],
    # 18: slots rewritten by another call and put back; the accumulator of Internals behind a failed call
    18: ["whole_mols", "internals_dihedral_8", "fail_internals_nan", "internals_accumulate_16", "internals_dihedral_8"],
    # 19: device ingest into the slots straight in front of an object's walk (SlotUse)
    19: ["xtc_read_full", "fluct_small_8", "trr_read", "panel_big_16"],
}


def mandatory():
    return [k for a in sorted(ADJACENCIES) for k in ADJACENCIES[a]]


def schedule(seed):
    """the mandatory adjacencies in order, then a seeded shuffle of (failing kind, kind) pairs: every non-failing kind once directly
    behind a failing kind of its own family and once behind one of another family, every failing kind at least twice"""
    rng = np.random.default_rng(seed)
    fails = {}
    for name in sorted(KINDS):
        if META[name]["failing"]:
            fails.setdefault(META[name]["family"], []).append(name)
    all_fails = [f for fam in sorted(fails) for f in fails[fam]]
    turn = {"own": {fam: 0 for fam in fails}, "other": 0}
    pairs = []
    for name in sorted(KINDS):
        if META[name]["failing"]:
            continue
        fam = META[name]["family"]
        own = fails[fam][turn["own"][fam] % len(fails[fam])]; turn["own"][fam] += 1
        while META[all_fails[turn["other"] % len(all_fails)]]["family"] == fam:
            turn["other"] += 1
        other = all_fails[turn["other"] % len(all_fails)]; turn["other"] += 1
        pairs += [(own, name), (other, name)]
    order = rng.permutation(len(pairs))
    return mandatory() + [k for p in order for k in pairs[p]]
