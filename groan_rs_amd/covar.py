"""Covariance on resident frames: the positional covariance matrix (3S x 3S) and the dynamical cross-correlation map (S x S) of a group.

The step after Fluctuations: essential dynamics / PCA as in `gmx covar`.  The reference has no function for it; its users download every
fitted frame and accumulate X.T @ X in numpy.  Here `accumulate` runs that over a block of resident slots in one C call
(gr_covar_accumulate_batch): an origin (f32, the first counted frame), the sum of d = x - origin and the sum of d_i * d_j (f64), the
latter a symmetric rank-K update on the f64 matrix cores.  The closing steps (mean = o + s / n, cov_ij = (Q_ij - s_i s_j / n) / n, the
mass weighting, the DCCM) are the library's; no arithmetic on atoms happens in Python.  The eigen-solve is numpy's:
`w, v = numpy.linalg.eigh(cov.matrix())`.
"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import OK, E_EMPTY_GROUP, E_GROUP_NOT_FOUND, E_INCONSISTENT_GROUP, E_NO_POSITION
from .system import DeviceError, GroupError, _ptr


class Covariance:
    """the sums of `group` (snapshot of its atoms and masses, group order; dimension 3 k + c) over the frames handed to accumulate()"""

    def __init__(self, system, group):
        self._lib = _lib.load()
        self.system, self.group, self._f = system, group, None
        st = C.c_int(0)
        self._f = self._lib.gr_covar_create(system._ctx, group.encode(), C.byref(st))
        if not self._f:
            self._raise(st.value)
        self.n_atoms = int(self._lib.gr_covar_n_atoms(self._f))
        system._plans.append(self)

    # -- lifetime: close() (or `with`) frees the device buffers now; System.close() closes what is still open, before its context goes
    def close(self):
        if getattr(self, "_f", None):
            self._lib.gr_covar_destroy(self._f)
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

    def _handle(self):
        if not self._f:
            raise ValueError("the Covariance object is closed")
        return self._f

    # -- filling
    def accumulate(self, first_slot, n_frames, raise_on_error=True):
        """counts slots first_slot .. first_slot + n_frames - 1 -> status int32 [n_frames]; a frame in which an atom of the group has
        no position fails with InvalidPosition and is counted for no dimension"""
        st_arr = np.zeros(n_frames, np.int32)
        st = self._lib.gr_covar_accumulate_batch(self._handle(), first_slot, n_frames, _ptr(st_arr))
        if st != OK and raise_on_error:
            self._raise(st)
        return st_arr

    def clear(self):
        self._check(self._lib.gr_covar_clear(self._handle()))

    def merge(self, other):
        """adds the frames of `other` (same number of atoms; any context, any device) to this object"""
        self._check(self._lib.gr_covar_merge(self._handle(), other._handle()))

    def set_launch(self, product_groups=0, check_groups=0):
        """caps on the grids of the product (it then strides over the blocks of Q) and of the position check (0: the default).  The
        result never depends on it; CV_STAT_LAST_*_GROUPS report what was launched"""
        if self._lib.gr_covar_set_launch(self._f, int(product_groups), int(check_groups)) != OK:
            raise ValueError("set_launch on a closed Covariance object")

    def stat(self, key):
        v = C.c_uint64(0)
        if self._lib.gr_covar_stat(self._f, int(key), C.byref(v)) != OK:
            raise ValueError("unknown covariance stat %r" % (key,))
        return int(v.value)

    # -- reading
    @property
    def n_frames(self):
        """counted frames"""
        return int(self._lib.gr_covar_frames(self._handle()))

    def mean(self):
        """float64 [S, 3], NaN before the first counted frame"""
        mean = np.zeros((self.n_atoms, 3), np.float64)
        self._check(self._lib.gr_covar_read(self._handle(), _ptr(mean), None, 0))
        return mean

    def matrix(self, mass_weighted=False):
        """float64 [3S, 3S]: the covariance over the counted frames (divided by n); mass_weighted: times sqrt(m_i m_j).  NaN before the
        first counted frame"""
        d = 3 * self.n_atoms
        cov = np.zeros((d, d), np.float64)
        self._check(self._lib.gr_covar_read(self._handle(), None, _ptr(cov), _lib.CV_MASS_WEIGHTED if mass_weighted else 0))
        return cov

    def dccm(self):
        """float64 [S, S]: the dynamical cross-correlation map"""
        corr = np.zeros((self.n_atoms, self.n_atoms), np.float64)
        self._check(self._lib.gr_covar_read_dccm(self._handle(), _ptr(corr)))
        return corr

    def raw(self):
        """(origin float32 [S, 3], sum float64 [S, 3], Q float64 [3S, 3S], n): the state as it stands"""
        d = 3 * self.n_atoms
        o, sm, q = np.zeros((self.n_atoms, 3), np.float32), np.zeros((self.n_atoms, 3), np.float64), np.zeros((d, d), np.float64)
        n = C.c_uint64(0)
        self._check(self._lib.gr_covar_read_raw(self._handle(), _ptr(o), _ptr(sm), _ptr(q), C.byref(n)))
        return o, sm, q, int(n.value)
