"""RMSDPanel / rmsd_matrix: the RMSD of every frame against every other frame.

The reference's way is a double loop of `System::calc_rmsd(&other, group)` (src/system/rmsd.rs:75-166).  Each side of calc_rmsd is
prepared without its partner, so a panel (gr_rmsd_panel_*) keeps the group's centred coordinates of the frames appended to it -- the
slots they came from may be overwritten at once, a long trajectory is packed block by block -- and `rmsd_matrix` is one dense product
in f64 on the matrix cores, closed per pair on the device.  No arithmetic on atoms happens in Python.
"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import OK
from .system import _ptr

MAX_FRAMES = 1 << 20             # capacity of a panel (GR_RP_MAX_FRAMES)
MAX_DEVICE_ENTRIES = 1 << 28     # n_rows x n_cols of a matrix left on the device


def check_capacity(capacity):
    """1 .. 2^20 frames"""
    n = int(capacity)
    if n != capacity or not 1 <= n <= MAX_FRAMES:
        raise ValueError("capacity must be an integer in 1 .. %d, not %r" % (MAX_FRAMES, capacity))
    return n


def check_device_size(n_rows, n_cols):
    """a matrix that stays on the device holds at most 2^28 entries"""
    if int(n_rows) * int(n_cols) > MAX_DEVICE_ENTRIES:
        raise ValueError("a %d x %d matrix does not stay on the device (at most %d entries): take the host form" % (n_rows, n_cols, MAX_DEVICE_ENTRIES))


class RMSDPanel:
    """the centred coordinates of `group` for up to `capacity` frames, kept after their slots have moved on"""

    def __init__(self, system, group, capacity):
        capacity = check_capacity(capacity)
        self._lib = _lib.load()
        self.system, self.group, self.capacity, self._p = system, group, capacity, None
        st = C.c_int(0)
        self._p = self._lib.gr_rmsd_panel_create(system._ctx, group.encode(), capacity, C.byref(st))
        if not self._p:
            system._raise_rmsd(st.value)
        self.n_atoms = int(self._lib.gr_rmsd_panel_n_atoms(self._p))
        system._plans.append(self)

    # -- lifetime: close() (or `with`) frees the device buffers now; System.close() closes what is still open, before its context goes
    def close(self):
        if getattr(self, "_p", None):
            self._lib.gr_rmsd_panel_destroy(self._p)
            self._p = None

    def __enter__(self): return self
    def __exit__(self, *a): self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __len__(self):
        """frames appended so far, failed ones included"""
        return int(self._lib.gr_rmsd_panel_frames(self._p))

    def append(self, first_slot, n_frames, raise_on_error=True):
        """packs slots first_slot .. first_slot + n_frames - 1 as the next rows -> status int32 [n_frames]; a failed frame still takes
        a row (its entries of the matrix are NaN).  The slots may be overwritten as soon as this returns."""
        st_arr = np.zeros(n_frames, np.int32)
        st = self._lib.gr_rmsd_panel_append_batch(self._p, first_slot, n_frames, _ptr(st_arr))
        if st != OK and raise_on_error:
            self.system._raise_rmsd(st)
        return st_arr

    def clear(self):
        self._lib.gr_rmsd_panel_clear(self._p)

    @property
    def status(self):
        """status int32 [len(self)] of the rows"""
        out = np.zeros(max(len(self), 1), np.int32)
        self._lib.gr_rmsd_panel_status(self._p, _ptr(out))
        return out[:len(self)]

    def set_block_entries(self, n):
        """entries per column block of the host form of rmsd_matrix with this panel as rows (0: the default); the result does not depend on it"""
        self._lib.gr_rmsd_panel_set_block_entries(self._p, int(n))


def rmsd_matrix(rows, cols=None, device=False):
    """M[i, j] = calc_rmsd of row frame i (self) against column frame j (reference); NaN where either frame is invalid.  cols=None (or
    cols is rows): the panel against itself, one triangle computed and mirrored.  device=True -> (device pointer, n_rows, n_cols), valid
    until the next matrix call with these rows; read it with rows.system.device_read"""
    lib, cp = rows._lib, (cols._p if cols is not None else None)
    n_rows, n_cols = len(rows), len(cols if cols is not None else rows)
    if device:
        check_device_size(n_rows, n_cols)
        dev, nr, nc = C.c_void_p(0), C.c_uint32(0), C.c_uint32(0)
        st = lib.gr_rmsd_matrix_device(rows._p, cp, C.byref(dev), C.byref(nr), C.byref(nc))
        if st != OK:
            rows.system._raise_rmsd(st)
        return dev, int(nr.value), int(nc.value)
    out = np.zeros((max(n_rows, 1), max(n_cols, 1)), np.float32)
    st = lib.gr_rmsd_matrix(rows._p, cp, _ptr(out))
    if st != OK:
        rows.system._raise_rmsd(st)
    return out[:n_rows, :n_cols]
