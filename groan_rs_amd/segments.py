"""Segments: the centres of every residue / molecule / listed part of a system, for a block of resident frames, in one C call.

The reference's loop is `for part in group_split_by_resid(..) { group_get_com(part) }` (src/system/groups.rs:344-435, :514-558) or the
same over `molecule_iter` (iterating.rs:238-245), once per frame.  Here the parts are one object (gr_segments_*): made once, then
`centers` returns all of them for n_frames slots.  No arithmetic on atoms happens in Python.
"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import OK, CENTER_ESTIMATE, CENTER_NAIVE, CENTER_PBC
from .system import _ptr


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

    def get_com(self, first_slot=0, n_frames=1, **kw): return self.centers(first_slot, n_frames, CENTER_PBC, 1, **kw)
    def get_center(self, first_slot=0, n_frames=1, **kw): return self.centers(first_slot, n_frames, CENTER_PBC, 0, **kw)
    def estimate_com(self, first_slot=0, n_frames=1, **kw): return self.centers(first_slot, n_frames, CENTER_ESTIMATE, 1, **kw)
    def get_com_naive(self, first_slot=0, n_frames=1, **kw): return self.centers(first_slot, n_frames, CENTER_NAIVE, 1, **kw)
