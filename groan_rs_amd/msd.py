"""MSD on resident frames: "nojump" unwrapping and the windowed mean-squared displacement of a group.

The most common dynamical analysis (diffusion of lipids, water, ions; `gmx msd`).  The reference has no function for it; its users
download every frame, undo the periodic jumps in numpy and run a double loop over time origins.  Here `append` takes a block of
resident slots as the next time indices in one C call (gr_msd_append_batch): per atom the displacement from the first counted frame,
unwrapped by summing minimum-image steps in f64, goes into a device panel, and the slots may be overwritten at once.  `msd` closes
the band of lags on the f64 matrix cores (gr_msd_compute): D2(t, t') = q_t + q_t' - 2 G(t, t') with G the Gram matrix of the panel's
rows.  No arithmetic on atoms happens in Python.
"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import OK, E_EMPTY_GROUP, E_GROUP_NOT_FOUND, E_NO_BOX, E_NO_POSITION, E_NOT_ORTHOGONAL, E_UNSUPPORTED_BOX, E_ZERO_BOX
from .system import DeviceError, GroupError, _ptr, _simbox

_DIMS = {"x": _lib.MSD_X, "y": _lib.MSD_Y, "z": _lib.MSD_Z}


class MSD:
    """the displacements of `group` (snapshot of its atoms, group order) over the frames handed to append(), and their MSD curve.
    dims: which components enter ("xy": the lateral MSD of a membrane); nojump: undo periodic jumps while appending"""

    def __init__(self, system, group, capacity, dims="xyz", nojump=True):
        self._lib = _lib.load()
        self.system, self.group, self._f = system, group, None
        flags = _lib.MSD_NOJUMP if nojump else 0
        for d in str(dims).lower():
            if d not in _DIMS:
                raise ValueError("dims is made of 'x', 'y' and 'z', not %r" % (dims,))
            flags |= _DIMS[d]
        self.flags = flags
        st = C.c_int(0)
        self._f = self._lib.gr_msd_create(system._ctx, group.encode(), int(capacity), flags, C.byref(st))
        if not self._f:
            self._raise(st.value)
        self.n_atoms = int(self._lib.gr_msd_n_atoms(self._f))
        self.capacity = int(self._lib.gr_msd_capacity(self._f))
        system._plans.append(self)

    # -- lifetime: close() (or `with`) frees the device buffers now; System.close() closes what is still open, before its context goes
    def close(self):
        if getattr(self, "_f", None):
            self._lib.gr_msd_destroy(self._f)
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
        if status in (E_NO_BOX, E_NOT_ORTHOGONAL, E_ZERO_BOX, E_UNSUPPORTED_BOX): raise _simbox(status)
        raise DeviceError(lib.gr_status_string(status).decode(), msg, status)

    def _check(self, status):
        if status != OK:
            self._raise(status)

    def _handle(self):
        if not self._f:
            raise ValueError("the MSD object is closed")
        return self._f

    # -- filling
    def append(self, first_slot, n_frames, raise_on_error=True):
        """slots first_slot .. first_slot + n_frames - 1 become the next time indices -> status int32 [n_frames].  A failed frame (an
        atom of the group without position; with nojump a frame without a box) still takes a time index and enters no pair.  Beyond
        the capacity the call is refused and nothing changes"""
        st_arr = np.zeros(n_frames, np.int32)
        st = self._lib.gr_msd_append_batch(self._handle(), first_slot, n_frames, _ptr(st_arr))
        if st != OK and raise_on_error:
            self._raise(st)
        return st_arr

    def clear(self):
        self._check(self._lib.gr_msd_clear(self._handle()))

    def set_launch(self, walk_groups=0, gram_groups=0):
        """the number of ranges of the walk and a cap on the grid of the product (0: the default).  The result never depends on it"""
        if self._lib.gr_msd_set_launch(self._f, int(walk_groups), int(gram_groups)) != OK:
            raise ValueError("set_launch on a closed MSD object")

    def stat(self, key):
        v = C.c_uint64(0)
        if self._lib.gr_msd_stat(self._f, int(key), C.byref(v)) != OK:
            raise ValueError("unknown msd stat %r" % (key,))
        return int(v.value)

    # -- reading
    @property
    def n_frames(self):
        """time indices taken so far (failed frames included)"""
        return int(self._lib.gr_msd_frames(self._handle()))

    def msd(self, max_lag=None):
        """(msd float64 [L], pairs uint64 [L]) for lags 0 .. L - 1, L = min(max_lag, n_frames - 1) + 1 (None: every lag): msd[tau] is
        the mean over the pairs (t, t + tau) of good frames and over the atoms of |d(t + tau) - d(t)|^2, NaN where there is no pair;
        msd[0] is exactly 0"""
        n = self.n_frames
        lag = 0xFFFFFFFF if max_lag is None else int(max_lag)
        if lag < 0:
            raise ValueError("max_lag is not negative")
        self._check(self._lib.gr_msd_compute(self._handle(), min(lag, 0xFFFFFFFF)))
        lags = self.stat(_lib.MSD_STAT_LAGS)
        assert lags == min(lag, n - 1) + 1
        msd, pairs = np.zeros(lags, np.float64), np.zeros(lags, np.uint64)
        self._check(self._lib.gr_msd_read(self._handle(), _ptr(msd), _ptr(pairs)))
        return msd, pairs

    def from_origin(self):
        """float64 [n_frames]: the MSD of every frame from the first counted one, NaN for a failed frame"""
        out = np.zeros(self.n_frames, np.float64)
        if len(out):
            self._check(self._lib.gr_msd_read_from_origin(self._handle(), _ptr(out)))
        return out

    def displacements(self, t0, nt):
        """float32 [nt, S, 3]: the unwrapped displacements of frames t0 .. t0 + nt - 1 from the origin, group order; zeros for a failed
        frame and in the components that dims leaves out"""
        out = np.zeros((nt, self.n_atoms, 3), np.float32)
        self._check(self._lib.gr_msd_read_displacements(self._handle(), int(t0), int(nt), _ptr(out)))
        return out
