"""Segments: the centres of every residue / molecule / listed part of a system, for a block of resident frames, in one C call.

The reference's loop is `for part in group_split_by_resid(..) { group_get_com(part) }` (src/system/groups.rs:344-435, :514-558) or the
same over `molecule_iter` (iterating.rs:238-245), once per frame.  Here the parts are one object (gr_segments_*): made once, then
`centers` returns all of them for n_frames slots, and `gyration` their shape: radius of gyration, gyration tensor and principal axes
(gmx gyrate / gmx principal for every part at once).  No arithmetic on atoms happens in Python.
"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import OK, CENTER_ESTIMATE, CENTER_NAIVE, CENTER_PBC
from .system import _ptr


class Gyration:
    """what Segments.gyration returns, as views of the call's two blocks (F frames, M segments):
    center [F, M, 3] nm, rg [F, M] nm, tensor [F, M, 3, 3] nm^2 (symmetric), status [F]; with axes: eigenvalues [F, M, 3] nm^2
    (descending) and axes [F, M, 3, 3] (rows v1, v2, v3), else both None.  `moments` [F, M, 10] and `raw_axes` [F, M, 12] are the blocks"""

    def __init__(self, moments, raw_axes, status):
        self.moments, self.raw_axes, self.status = moments, raw_axes, status
        self.center, self.rg = moments[..., 0:3], moments[..., 3]
        self.tensor = moments[..., [4, 7, 8, 7, 5, 9, 8, 9, 6]].reshape(moments.shape[:-1] + (3, 3))
        self.eigenvalues = raw_axes[..., 0:3] if raw_axes is not None else None
        self.axes = raw_axes[..., 3:12].reshape(raw_axes.shape[:-1] + (3, 3)) if raw_axes is not None else None


def shape_descriptors(eigenvalues):
    """eigenvalues [..., 3] of a gyration tensor (descending) -> (asphericity l1 - (l2 + l3) / 2, acylindricity l2 - l3, relative shape
    anisotropy 1.5 sum l^2 / (sum l)^2 - 0.5, which is 0 where sum l = 0), float64"""
    lam = np.asarray(eigenvalues, np.float64)
    l1, l2, l3 = lam[..., 0], lam[..., 1], lam[..., 2]
    tr = l1 + l2 + l3
    with np.errstate(invalid="ignore", divide="ignore"):
        kappa2 = np.where(tr == 0.0, 0.0, 1.5 * (l1 * l1 + l2 * l2 + l3 * l3) / np.where(tr == 0.0, 1.0, tr * tr) - 0.5)
    return l1 - 0.5 * (l2 + l3), l2 - l3, kappa2


class Segments:
    """an ordered list of M non-empty, strictly ascending atom lists over the atoms of `system`"""

    def __init__(self, system, handle):
        self._lib = _lib.load()
        self.system, self._seg = system, handle
        system._plans.append(self)

    # -- constructors
    @classmethod
    def _make(cls, system, call):
        lib = _lib.load()
        st = C.c_int(0)
        handle = call(lib, C.byref(st))
        if not handle:
            system._raise_group(st.value)
        return cls(system, handle)

    @classmethod
    def from_lists(cls, system, lists):
        """explicit atom lists, each strictly ascending; they may overlap"""
        lists = [np.asarray(a, np.uint64).ravel() for a in lists]
        off = np.zeros(len(lists) + 1, np.uint64)
        if lists:
            off[1:] = np.cumsum([a.size for a in lists])
        atoms = np.ascontiguousarray(np.concatenate(lists) if lists else np.zeros(0, np.uint64), np.uint64)
        if atoms.size == 0:
            atoms = np.zeros(1, np.uint64)      # (a pointer to hand over: the call refuses empty segments itself)
        return cls._make(system, lambda lib, st: lib.gr_segments_create(system._ctx, _ptr(off), _ptr(atoms), len(lists), st))

    @classmethod
    def _from_labels(cls, system, labels, group):
        lab = np.ascontiguousarray(labels, np.uint64)
        if lab.shape != (system.n_atoms,):
            raise ValueError("one label per atom of the system")
        return cls._make(system, lambda lib, st: lib.gr_segments_from_labels(system._ctx, group.encode() if group is not None else None, _ptr(lab), st))

    @classmethod
    def by_resid(cls, system, resid, group=None):
        """group_split_by_resid: one segment per residue number of `group` (None: all atoms), in order of first appearance"""
        return cls._from_labels(system, resid, group)

    @classmethod
    def by_resname(cls, system, resnames, group=None):
        """group_split_by_resname: one segment per residue name; names become labels by first appearance"""
        names = np.asarray(resnames)
        _, first, inverse = np.unique(names, return_index=True, return_inverse=True)
        rank = np.empty(first.size, np.uint64)
        rank[np.argsort(first, kind="stable")] = np.arange(first.size, dtype=np.uint64)
        return cls._from_labels(system, rank[inverse.ravel()], group)

    @classmethod
    def from_group(cls, system, name):
        """ONE segment holding the group `name`: from_group(s, "Protein").gyration(0, nf).rg[:, 0] is the gmx gyrate curve"""
        return cls._from_labels(system, np.zeros(system.n_atoms, np.uint64), name)

    @classmethod
    def from_molecules(cls, system):
        """one segment per molecule of the system's bonds as they are now; an atom without bonds is a segment of its own"""
        return cls._make(system, lambda lib, st: lib.gr_segments_from_molecules(system._ctx, st))

    # -- lifetime: close() (or `with`) frees the device buffers now; System.close() closes what is still open, before its context goes
    def close(self):
        if getattr(self, "_seg", None):
            self._lib.gr_segments_destroy(self._seg)
            self._seg = None

    def __enter__(self): return self
    def __exit__(self, *a): self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- the partition
    def __len__(self):
        return int(self._lib.gr_segments_count(self._seg))

    @property
    def sizes(self):
        out = np.zeros(len(self), np.uint64)
        self._lib.gr_segments_sizes(self._seg, _ptr(out))
        return out

    def atoms(self, s):
        n = C.c_uint64(0)
        st = self._lib.gr_segments_atoms(self._seg, int(s), None, 0, C.byref(n))
        if st != OK:
            raise IndexError("segment %r out of range" % (s,))
        out = np.zeros(n.value, np.uint64)
        self._lib.gr_segments_atoms(self._seg, int(s), _ptr(out), n.value, C.byref(n))
        return out

    def stat(self, key):
        v = C.c_uint64(0)
        if self._lib.gr_segments_stat(self._seg, int(key), C.byref(v)) != OK:
            raise ValueError("unknown segments stat %r" % (key,))
        return int(v.value)

    # -- centres
    def centers(self, first_slot, n_frames, kind, weighted, raise_on_error=True):
        """-> (float32 [n_frames, M, 3], status int32 [n_frames]): NaN rows for a segment with an atom without position / mass (the
        frame's status is that of its first such segment) and for every segment of a frame that fails its box check"""
        out = np.zeros((n_frames, len(self), 3), np.float32); st_arr = np.zeros(n_frames, np.int32)
        st = self._lib.gr_segments_center_batch(self._seg, first_slot, n_frames, int(kind), int(bool(weighted)), _ptr(out), _ptr(st_arr))
        if st != OK and raise_on_error:
            self.system._raise_group(st)
        return out, st_arr

    def centers_device(self, first_slot, n_frames, kind, weighted, raise_on_error=True):
        """the same, left on the device: -> (device pointer to [n_frames, M, 3] float32, valid until the next call on this object, status)"""
        dev = C.c_void_p(0); st_arr = np.zeros(n_frames, np.int32)
        st = self._lib.gr_segments_center_batch_device(self._seg, first_slot, n_frames, int(kind), int(bool(weighted)), C.byref(dev), None, _ptr(st_arr))
        if st != OK and raise_on_error:
            self.system._raise_group(st)
        return dev, st_arr

    # -- shape: gyration tensor, radius of gyration, principal axes (gr_segments_gyration_batch)
    def gyration(self, first_slot, n_frames, kind=CENTER_PBC, weighted=True, axes=False, raise_on_error=True):
        """-> Gyration: centre, Rg, gyration tensor (and, with `axes`, eigenvalues and principal axes) of every segment in every frame.
        NaN rows where `centers` has them; the centre is `centers`' own, bit for bit"""
        m = len(self)
        mom = np.zeros((n_frames, m, 10), np.float32); st_arr = np.zeros(n_frames, np.int32)
        ax = np.zeros((n_frames, m, 12), np.float32) if axes else None
        st = self._lib.gr_segments_gyration_batch(self._seg, first_slot, n_frames, int(kind), int(bool(weighted)), _ptr(mom), _ptr(ax), _ptr(st_arr))
        if st != OK and raise_on_error:
            self.system._raise_group(st)
        return Gyration(mom, ax, st_arr)

    def gyration_device(self, first_slot, n_frames, kind=CENTER_PBC, weighted=True, axes=False, raise_on_error=True):
        """the same, left on the device: -> (pointer to [n_frames, M, 10] float32, pointer to [n_frames, M, 12] float32 or None, status);
        valid until the next call on this object; at most one piece of frames (set_piece_frames)"""
        mom, ax = C.c_void_p(0), C.c_void_p(0)
        st_arr = np.zeros(n_frames, np.int32)
        st = self._lib.gr_segments_gyration_batch_device(self._seg, first_slot, n_frames, int(kind), int(bool(weighted)), int(bool(axes)), C.byref(mom), C.byref(ax),
                                                         None, _ptr(st_arr))
        if st != OK and raise_on_error:
            self.system._raise_group(st)
        return mom, (ax if axes else None), st_arr

    def set_piece_frames(self, n):
        """frames per piece of a gyration call (0: as many as 256 MiB of moments and axes hold); results do not depend on it"""
        self._lib.gr_segments_set_piece_frames(self._seg, int(n))

    def moments_of_inertia(self, eigenvalues, masses):
        """principal moments of inertia I_k = W (Rg^2 - lambda_k) = W (sum of the two other eigenvalues), W = the segment's total mass
        from `masses` [n_atoms] and its atom list: eigenvalues [..., M, 3] of a mass-weighted gyration call -> float64 [..., M, 3]"""
        lam = np.asarray(eigenvalues, np.float64)
        masses = np.asarray(masses, np.float64)
        if lam.shape[-2:] != (len(self), 3):
            raise ValueError("eigenvalues [..., M, 3]")
        total = np.array([masses[self.atoms(s).astype(np.int64)].sum() for s in range(len(self))], np.float64)
        return total[:, None] * (lam.sum(axis=-1, keepdims=True) - lam)

    def get_com(self, first_slot=0, n_frames=1, **kw): return self.centers(first_slot, n_frames, CENTER_PBC, 1, **kw)
    def get_center(self, first_slot=0, n_frames=1, **kw): return self.centers(first_slot, n_frames, CENTER_PBC, 0, **kw)
    def estimate_com(self, first_slot=0, n_frames=1, **kw): return self.centers(first_slot, n_frames, CENTER_ESTIMATE, 1, **kw)
    def get_com_naive(self, first_slot=0, n_frames=1, **kw): return self.centers(first_slot, n_frames, CENTER_NAIVE, 1, **kw)
