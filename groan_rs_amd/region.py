"""Region: which atoms of a group lie inside a set of shapes, for every frame of a block of resident frames, in one C call.

The reference's loop is `for atom in system.group_iter("Water")?.filter_geometry(cylinder)` (src/lib.rs:170-188) or
`group_create_from_geometries` (src/system/groups.rs:94-188), once per frame.  Here the shapes are one object (gr_region_*): made once,
then `select` evaluates them for n slots and leaves the per-frame index lists on the device; `lists` / `frame` copy them to the host and
`to_group` turns one frame's list into a named group.  No arithmetic on atoms happens in Python.
"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import OK, E_GROUP_EXISTS
from .shapes import pack
from .system import _ptr


def pack_anchors(anchors, n_frames):
    """-> C-contiguous float32 [n_frames, 3] (None stays None).  Only float32 is taken: the anchors are added to the shapes in f32, and
    a silent conversion would hide from the caller which bits were used"""
    if anchors is None:
        return None
    a = np.asarray(anchors)
    if a.dtype != np.float32:
        raise TypeError("anchors must be float32, not %s" % a.dtype)
    if a.shape != (int(n_frames), 3):
        raise ValueError("anchors must have shape (n_frames, 3) = (%d, 3), not %r" % (int(n_frames), a.shape))
    return np.ascontiguousarray(a)


class Region:
    """up to 8 shapes and the naive flag; an atom is selected when it has a position and lies inside every shape"""

    def __init__(self, system, shapes, naive=False):
        shapes = list(shapes)
        if len(shapes) > _lib.MAX_SHAPES:
            raise ValueError("at most %d shapes" % _lib.MAX_SHAPES)
        if naive and any(not s.has_naive for s in shapes):
            raise TypeError("TriangularPrism does not implement NaiveShape")
        self._shapes, self._n_shapes = pack(shapes)
        self.naive = bool(naive)
        self._lib = _lib.load()
        self.system, self._rg = system, None
        st = C.c_int(0)
        self._rg = self._lib.gr_region_create(system._ctx, self._shapes, self._n_shapes, int(self.naive), C.byref(st))
        if not self._rg:
            system._raise_group(st.value)
        system._plans.append(self)

    # -- lifetime: close() (or `with`) frees the device buffers now; System.close() closes what is still open, before its context goes
    def close(self):
        if getattr(self, "_rg", None):
            self._lib.gr_region_destroy(self._rg)
            self._rg = None

    def __enter__(self): return self
    def __exit__(self, *a): self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- selection
    def select(self, group, first, n, anchors=None, raise_on_error=True):
        """the atoms of `group` (None: all atoms) inside the shapes in slots first .. first + n - 1; with `anchors` (float32 [n, 3]) the
        shapes of frame f are the stored ones moved by anchors[f].  -> (counts uint64 [n], status int32 [n]); a failed frame counts 0"""
        a = pack_anchors(anchors, n)
        counts = np.zeros(n, np.uint64); st_arr = np.zeros(n, np.int32)
        st = self._lib.gr_region_select_batch(self._rg, first, n, group.encode() if group is not None else None, _ptr(a), _ptr(counts), _ptr(st_arr))
        if st != OK and raise_on_error:
            self.system._raise_group(st)
        return counts, st_arr

    def lists(self):
        """-> (offsets uint64 [n_frames + 1], atoms uint64 [total]) of the last select: frame f is atoms[offsets[f]:offsets[f + 1]]"""
        nf, total = C.c_uint64(0), C.c_uint64(0)
        self._lib.gr_region_read_device(self._rg, None, None, C.byref(nf), C.byref(total))
        offsets = np.zeros(nf.value + 1, np.uint64); atoms = np.zeros(total.value, np.uint64)
        st = self._lib.gr_region_read(self._rg, _ptr(offsets), _ptr(atoms) if total.value else None, total.value, None)
        if st != OK:
            self.system._raise_group(st)
        return offsets, atoms

    def lists_device(self):
        """-> (device pointer to the uint32 atom list, device pointer to the uint64 offsets, n_frames, total), valid until the next select"""
        atoms, offsets, nf, total = C.c_void_p(0), C.c_void_p(0), C.c_uint64(0), C.c_uint64(0)
        self._lib.gr_region_read_device(self._rg, C.byref(atoms), C.byref(offsets), C.byref(nf), C.byref(total))
        return atoms, offsets, int(nf.value), int(total.value)

    def frame(self, f):
        """the index array of frame f of the last select"""
        offsets, atoms = self.lists()
        if not 0 <= int(f) < offsets.size - 1:
            raise IndexError("frame %r is not part of the last selection" % (f,))
        return atoms[int(offsets[f]):int(offsets[f + 1])]

    def to_group(self, f, name):
        """frame f's list becomes the group `name` -> True when a group of that name was replaced (AlreadyExistsWarning)"""
        st = self._lib.gr_region_group(self._rg, int(f), name.encode())
        if st not in (OK, E_GROUP_EXISTS):
            self.system._raise_group(st)
        return st == E_GROUP_EXISTS

    def set_piece_frames(self, n):
        """frames per piece of the mask workspace (0: the default); the result does not depend on it"""
        self._lib.gr_region_set_piece_frames(self._rg, int(n))

    def stat(self, key):
        v = C.c_uint64(0)
        if self._lib.gr_region_stat(self._rg, int(key), C.byref(v)) != OK:
            raise ValueError("unknown region stat %r" % (key,))
        return int(v.value)
