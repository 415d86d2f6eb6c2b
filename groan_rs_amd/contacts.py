"""Contacts: which atoms of group 2 are within a cut-off of an atom of group 1, for every frame of a block of resident frames, in one C call.

The reference's loop is `CellGrid::new` + `neighbors_iter` + a distance filter (src/structures/cellgrid.rs:301-409, :434-476,
src/system/hbonds.rs:248-265), once per frame.  Here the two groups and the cut-off are one object (gr_contacts_*): made once -- the
groups' atoms are snapshotted -- then `pairs` searches n slots and leaves the per-frame (i, j, d) lists on the device; `lists` / `frame`
copy them to the host; `counts` and `hist` run the same walk without the lists.  A frame's result is exactly
`System.group_pairs_within` of that slot.  No arithmetic on atoms happens in Python.
"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import OK
from .system import _ptr

NO_LIMIT = 2 ** 64 - 1


def check_nbins(nbins):
    """1 .. 4096 bins over [0, cutoff)"""
    n = int(nbins)
    if n != nbins or not 1 <= n <= _lib.CT_MAX_BINS:
        raise ValueError("nbins must be an integer in 1 .. %d, not %r" % (_lib.CT_MAX_BINS, nbins))
    return n


def check_max_pairs(max_pairs):
    """None: no limit; else a count that fits 64 bits"""
    if max_pairs is None:
        return NO_LIMIT
    m = int(max_pairs)
    if m != max_pairs or not 0 <= m <= NO_LIMIT:
        raise ValueError("max_pairs must be None or an integer in 0 .. 2^64 - 1, not %r" % (max_pairs,))
    return m


class Contacts:
    """all pairs (i in group1, j in group2, i != j) with distance <= cutoff, frame by frame, ordered by i then j"""

    def __init__(self, system, group1, group2, cutoff):
        self.cutoff = float(np.float32(cutoff))
        self._lib = _lib.load()
        self.system, self._ct = system, None
        st = C.c_int(0)
        self._ct = self._lib.gr_contacts_create(system._ctx, group1.encode(), group2.encode(), C.c_float(cutoff), C.byref(st))
        if not self._ct:
            system._raise_group(st.value)
        n1, n2 = C.c_uint64(0), C.c_uint64(0)
        self._lib.gr_contacts_sizes(self._ct, C.byref(n1), C.byref(n2))
        self.n1, self.n2 = int(n1.value), int(n2.value)
        system._plans.append(self)

    # -- lifetime: close() (or `with`) frees the device buffers now; System.close() closes what is still open, before its context goes
    def close(self):
        if getattr(self, "_ct", None):
            self._lib.gr_contacts_destroy(self._ct)
            self._ct = None

    def __enter__(self): return self
    def __exit__(self, *a): self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- pair lists
    def pairs(self, first, n, max_pairs=None, raise_on_error=True):
        """searches slots first .. first + n - 1 and keeps the lists on the device -> (n_pairs uint64 [n], status int32 [n]); a failed
        frame has 0 pairs.  When the total exceeds max_pairs the call only counts (`lists` then raises; `total` is still right)"""
        cap = check_max_pairs(max_pairs)
        n_pairs = np.zeros(n, np.uint64); st_arr = np.zeros(n, np.int32)
        total = C.c_uint64(0)
        st = self._lib.gr_contacts_pairs_batch(self._ct, first, n, cap, _ptr(n_pairs), C.byref(total), _ptr(st_arr))
        if st != OK and raise_on_error:
            self.system._raise_group(st)
        return n_pairs, st_arr

    @property
    def total(self):
        """pairs of the last `pairs` call"""
        return self.stat(_lib.CT_STAT_LAST_TOTAL)

    def offsets(self):
        """-> offsets uint64 [n_frames + 1] of the last `pairs` call (also after a count-only call)"""
        nf = C.c_uint64(0)
        self._lib.gr_contacts_read_device(self._ct, None, None, None, None, C.byref(nf), None)
        offsets = np.zeros(nf.value + 1, np.uint64)
        st = self._lib.gr_contacts_read(self._ct, _ptr(offsets), None, None, None, 0, None)
        if st != OK:
            self.system._raise_group(st)
        return offsets

    def lists(self):
        """-> (offsets uint64 [n_frames + 1], i uint32 [total], j uint32 [total], d float32 [total]) of the last `pairs` call: frame f
        is [offsets[f]:offsets[f + 1]]"""
        nf, total = C.c_uint64(0), C.c_uint64(0)
        self._lib.gr_contacts_read_device(self._ct, None, None, None, None, C.byref(nf), C.byref(total))
        m = int(total.value)
        offsets = np.zeros(nf.value + 1, np.uint64)
        i = np.zeros(max(m, 1), np.uint32); j = np.zeros(max(m, 1), np.uint32); d = np.zeros(max(m, 1), np.float32)
        st = self._lib.gr_contacts_read(self._ct, _ptr(offsets), _ptr(i), _ptr(j), _ptr(d), m, None)
        if st != OK:
            self.system._raise_group(st)
        return offsets, i[:m], j[:m], d[:m]

    def frame(self, f):
        """(i, j, d) of frame f of the last `pairs` call"""
        offsets, i, j, d = self.lists()
        if not 0 <= int(f) < offsets.size - 1:
            raise IndexError("frame %r is not part of the last call" % (f,))
        a, b = int(offsets[f]), int(offsets[f + 1])
        return i[a:b], j[a:b], d[a:b]

    def lists_device(self):
        """-> (device pointers to i, j, d and the uint64 offsets, n_frames, total), valid until the next `pairs`"""
        i, j, d, offsets, nf, total = C.c_void_p(0), C.c_void_p(0), C.c_void_p(0), C.c_void_p(0), C.c_uint64(0), C.c_uint64(0)
        self._lib.gr_contacts_read_device(self._ct, C.byref(i), C.byref(j), C.byref(d), C.byref(offsets), C.byref(nf), C.byref(total))
        return i, j, d, offsets, int(nf.value), int(total.value)

    # -- the same walk without the lists
    def counts(self, first, n, raise_on_error=True):
        """-> (per_atom uint32 [n, n1], n_pairs uint64 [n], status int32 [n]): per_atom[f, k] = pairs of the k-th atom of group1 in frame f"""
        per_atom = np.zeros((n, self.n1), np.uint32); n_pairs = np.zeros(n, np.uint64); st_arr = np.zeros(n, np.int32)
        st = self._lib.gr_contacts_count_batch(self._ct, first, n, _ptr(per_atom) if self.n1 else None, _ptr(n_pairs), _ptr(st_arr))
        if st != OK and raise_on_error:
            self.system._raise_group(st)
        return per_atom, n_pairs, st_arr

    def hist(self, first, n, nbins, raise_on_error=True):
        """-> (hist uint64 [n, nbins], status int32 [n]) over [0, cutoff): bin = uint32(d * (float32(nbins) / cutoff)), counted iff that
        product is < nbins"""
        nbins = check_nbins(nbins)
        hist = np.zeros((n, nbins), np.uint64); st_arr = np.zeros(n, np.int32)
        st = self._lib.gr_contacts_hist_batch(self._ct, first, n, nbins, _ptr(hist), _ptr(st_arr))
        if st != OK and raise_on_error:
            self.system._raise_group(st)
        return hist, st_arr

    def set_piece_frames(self, n):
        """frames per piece of the sort workspace (0: the default); the result does not depend on it"""
        self._lib.gr_contacts_set_piece_frames(self._ct, int(n))

    def set_walk_groups(self, n):
        """workgroups of a walk launch, at most (0: the default); the result does not depend on it"""
        self._lib.gr_contacts_set_walk_groups(self._ct, int(n))

    def stat(self, key):
        v = C.c_uint64(0)
        if self._lib.gr_contacts_stat(self._ct, int(key), C.byref(v)) != OK:
            raise ValueError("unknown contacts stat %r" % (key,))
        return int(v.value)
