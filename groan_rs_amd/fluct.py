"""Fluctuations on resident frames: the average structure and the per-atom RMSF of a group.

The reference has no function for this; its users download every fitted frame and add it up around `calc_rmsd_and_fit`.  Here
`accumulate` runs that loop over a block of resident slots in one C call (gr_fluct_accumulate_batch): per atom and component an
origin (f32, the first counted frame), the sum of d = x - origin and the sum of d * d (f64), added frame after frame in ascending
order, so the sums are the same bit for bit however the frames were cut into calls.  The closing step (mean = o + s / n,
var = max(q - s^2 / n, 0) / n, rmsf = sqrt(var_x + var_y + var_z)) is the library's; no arithmetic on atoms happens in Python.
"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import OK, E_EMPTY_GROUP, E_GROUP_NOT_FOUND, E_INCONSISTENT_GROUP, E_NO_POSITION
from .system import DeviceError, GroupError, _ptr


class Fluctuations:
    """the sums of `group` (snapshot of its atoms, group order) over the frames handed to accumulate()"""

    def __init__(self, system, group):
        self._lib = _lib.load()
        self.system, self.group, self._f = system, group, None
        st = C.c_int(0)
        self._f = self._lib.gr_fluct_create(system._ctx, group.encode(), C.byref(st))
        if not self._f:
            self._raise(st.value)
        self.n_atoms = int(self._lib.gr_fluct_n_atoms(self._f))
        system._plans.append(self)

    # -- lifetime: close() (or `with`) frees the device buffers now; System.close() closes what is still open, before its context goes
    def close(self):
        if getattr(self, "_f", None):
            self._lib.gr_fluct_destroy(self._f)
            self._f = None

    def __enter__(self): return self
    def __exit__(self, *a): self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _raise(self, status):
        lib, ctx = self._lib, self.system._ctx
        msg = lib.gr_last_error(ctx).decode(errors="replace")
        idx = int(lib.gr_last_error_index(ctx))
        if status == E_GROUP_NOT_FOUND: raise GroupError("NotFound", msg, status)
        if status == E_EMPTY_GROUP: raise GroupError("EmptyGroup", msg, status)
        if status == E_NO_POSITION: raise GroupError("InvalidPosition", idx, status)
        if status == E_INCONSISTENT_GROUP:
            cnt = (C.c_uint64 * 2)()
            lib.gr_last_error_counts(ctx, cnt)
            raise GroupError("InconsistentGroup", (msg, int(cnt[0]), int(cnt[1])), status)
        raise DeviceError(lib.gr_status_string(status).decode(), msg, status)

    def _check(self, status):
        if status != OK:
            self._raise(status)

    # -- filling
    def accumulate(self, first_slot, n_frames, raise_on_error=True):
        """counts slots first_slot .. first_slot + n_frames - 1 -> status int32 [n_frames]; a frame in which an atom of the group has
        no position fails with InvalidPosition and is counted for no atom"""
        st_arr = np.zeros(n_frames, np.int32)
        st = self._lib.gr_fluct_accumulate_batch(self._f, first_slot, n_frames, _ptr(st_arr))
        if st != OK and raise_on_error:
            self._raise(st)
        return st_arr

    def clear(self):
        self._check(self._lib.gr_fluct_clear(self._f))

    def merge(self, other):
        """adds the frames of `other` (same number of atoms; any context, any device) to this object"""
        self._check(self._lib.gr_fluct_merge(self._f, other._f))

    def store_mean(self, system, slot):
        """the mean, rounded to f32, into the group's atoms of `slot` of `system` (same device, same n_atoms); nothing else of the slot changes"""
        self._check(self._lib.gr_fluct_store_mean(self._f, system._ctx, int(slot)))

    def set_launch(self, range_groups=0, check_groups=0):
        """the ranges the group is cut into and a cap on the position check's grid (0: the default).  The result never depends on it;
        FL_STAT_LAST_*_GROUPS report what was launched"""
        if self._lib.gr_fluct_set_launch(self._f, int(range_groups), int(check_groups)) != OK:
            raise ValueError("set_launch on a closed Fluctuations object")

    def stat(self, key):
        v = C.c_uint64(0)
        if self._lib.gr_fluct_stat(self._f, int(key), C.byref(v)) != OK:
            raise ValueError("unknown fluctuations stat %r" % (key,))
        return int(v.value)

    # -- reading
    @property
    def n_frames(self):
        """counted frames"""
        return int(self._lib.gr_fluct_frames(self._f))

    def _read(self):
        s = max(self.n_atoms, 1)
        mean, var, rmsf = np.zeros((s, 3), np.float64), np.zeros((s, 3), np.float64), np.zeros(s, np.float64)
        self._check(self._lib.gr_fluct_read(self._f, _ptr(mean), _ptr(var), _ptr(rmsf)))
        return mean[:self.n_atoms], var[:self.n_atoms], rmsf[:self.n_atoms]

    def mean(self):
        """float64 [S, 3], NaN before the first counted frame"""
        return self._read()[0]

    def variance(self):
        """float64 [S, 3]: per axis, over the counted frames (divided by n)"""
        return self._read()[1]

    def rmsf(self):
        """float64 [S]"""
        return self._read()[2]

    def raw(self):
        """(origin float32 [S, 3], sum float64 [S, 3], sum of squares float64 [S, 3], n): the state as it stands"""
        s = max(self.n_atoms, 1)
        o, sm, sq = np.zeros((s, 3), np.float32), np.zeros((s, 3), np.float64), np.zeros((s, 3), np.float64)
        n = C.c_uint64(0)
        self._check(self._lib.gr_fluct_read_raw(self._f, _ptr(o), _ptr(sm), _ptr(sq), C.byref(n)))
        return o[:self.n_atoms], sm[:self.n_atoms], sq[:self.n_atoms], int(n.value)
