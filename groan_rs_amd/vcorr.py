"""VectorCorrelation on resident frames: the P1 / P2 reorientation autocorrelation functions of a fixed list of bond vectors.

C1(tau) = <u(t) . u(t + tau)> and C2(tau) = <P2(u(t) . u(t + tau))>, P2(x) = (3 x^2 - 1) / 2 (`gmx rotacf`): water reorientation
times, lipid tail and head-group dynamics, NMR relaxation and the Lipari-Szabo S^2 of every N-H bond.  The reference has no function
for it; its users download every frame, gather the vectors and run a double loop over time origins.  Here `append` takes a block of
resident slots as the next time indices in one C call (gr_vcorr_append_batch): per vector u and the six components of u u^T go into
device panels, and the slots may be overwritten at once.  `correlate` closes the band of lags over all vectors on the f64 matrix
cores (gr_vcorr_compute: both curves are Gram products of a panel's rows), `correlate_each` gives the curve of every vector
(gr_vcorr_compute_each).  No arithmetic on atoms happens in Python.
"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import OK, E_NO_BOX, E_NO_POSITION, E_NOT_ORTHOGONAL, E_OUT_OF_RANGE, E_UNSUPPORTED_BOX, E_ZERO_BOX
from .system import AtomError, DeviceError, _ptr, _simbox

_RANKS = {1: _lib.VCORR_P1, 2: _lib.VCORR_P2}


class VectorCorrelation:
    """the vectors i -> j of `pairs` ([V, 2] atom indices) over the frames handed to append(), and their reorientation curves.
    rank: which curves are kept (1: C1, 2: C2; C2 needs unit vectors); pbc: the vector is the minimum image of the frame's own box
    (and a frame needs one); unit: the vectors are normalised"""

    def __init__(self, system, pairs, capacity, rank=(1, 2), pbc=False, unit=True):
        self._lib = _lib.load()
        self.system, self._f = system, None
        p = np.ascontiguousarray(np.asarray(pairs, np.uint64).reshape(-1, 2))
        flags = (_lib.VCORR_PBC if pbc else 0) | (_lib.VCORR_UNIT if unit else 0)
        for r in ((rank,) if isinstance(rank, int) else tuple(rank)):
            if r not in _RANKS:
                raise ValueError("rank is made of 1 and 2, not %r" % (rank,))
            flags |= _RANKS[r]
        self.flags = flags
        st = C.c_int(0)
        self._f = self._lib.gr_vcorr_create(system._ctx, _ptr(p), len(p), int(capacity), flags, C.byref(st))
        if not self._f:
            self._raise(st.value)
        self.pairs = p
        self.n_vectors = int(self._lib.gr_vcorr_count(self._f))
        self.capacity = int(self._lib.gr_vcorr_capacity(self._f))
        system._plans.append(self)

    # -- lifetime: close() (or `with`) frees the device buffers now; System.close() closes what is still open, before its context goes
    def close(self):
        if getattr(self, "_f", None):
            self._lib.gr_vcorr_destroy(self._f)
            self._f = None

    def __enter__(self): return self
    def __exit__(self, *a): self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __len__(self):
        return self.n_vectors

    def _raise(self, status):
        lib, ctx = self._lib, self.system._ctx
        msg = lib.gr_last_error(ctx).decode(errors="replace")
        idx = int(lib.gr_last_error_index(ctx))
        if status == E_OUT_OF_RANGE: raise AtomError("OutOfRange", idx, status)
        if status == E_NO_POSITION: raise AtomError("InvalidPosition", idx, status)
        if status in (E_NO_BOX, E_NOT_ORTHOGONAL, E_ZERO_BOX, E_UNSUPPORTED_BOX): raise _simbox(status)
        raise DeviceError(lib.gr_status_string(status).decode(), msg, status)

    def _check(self, status):
        if status != OK:
            self._raise(status)

    def _handle(self):
        if not self._f:
            raise ValueError("the VectorCorrelation object is closed")
        return self._f

    def _kept(self, rank):
        return bool(self.flags & _RANKS[rank])

    # -- filling
    def append(self, first_slot, n_frames, raise_on_error=True):
        """slots first_slot .. first_slot + n_frames - 1 become the next time indices -> status int32 [n_frames].  A failed frame (a
        named atom without position; with pbc a frame without a box) still takes a time index and enters no pair.  Beyond the
        capacity the call is refused and nothing changes"""
        st_arr = np.zeros(n_frames, np.int32)
        st = self._lib.gr_vcorr_append_batch(self._handle(), first_slot, n_frames, _ptr(st_arr))
        if st != OK and raise_on_error:
            self._raise(st)
        return st_arr

    def clear(self):
        self._check(self._lib.gr_vcorr_clear(self._handle()))

    def set_launch(self, walk_groups=0, gram_groups=0, each_groups=0):
        """test hook: the ranges of the walk, a cap on the grid of the product and of correlate_each (0: the default).  No result depends on it"""
        if not self._f or self._lib.gr_vcorr_set_launch(self._f, int(walk_groups), int(gram_groups), int(each_groups)) != OK:
            raise ValueError("set_launch on a closed VectorCorrelation object")

    def stat(self, key):
        v = C.c_uint64(0)
        if self._lib.gr_vcorr_stat(self._handle(), int(key), C.byref(v)) != OK:
            raise ValueError("unknown vcorr stat %r" % (key,))
        return int(v.value)

    # -- reading
    @property
    def n_frames(self):
        """time indices taken so far (failed frames included)"""
        return int(self._lib.gr_vcorr_frames(self._handle()))

    @staticmethod
    def _lag(max_lag):
        lag = 0xFFFFFFFF if max_lag is None else int(max_lag)
        if lag < 0:
            raise ValueError("max_lag is not negative")
        return min(lag, 0xFFFFFFFF)

    def correlate(self, max_lag=None):
        """(c1 float64 [L], c2 float64 [L], pairs uint64 [L]) for lags 0 .. L - 1, L = min(max_lag, n_frames - 1) + 1 (None: every lag):
        the mean over the pairs (t, t + tau) of good frames and over the vectors; NaN where there is no pair; None for a rank that is
        not kept.  A vector of length zero adds nothing but counts in the mean"""
        self._check(self._lib.gr_vcorr_compute(self._handle(), self._lag(max_lag)))
        lags = self.stat(_lib.VCORR_STAT_LAGS)
        c1 = np.zeros(lags, np.float64) if self._kept(1) else None
        c2 = np.zeros(lags, np.float64) if self._kept(2) else None
        pairs = np.zeros(lags, np.uint64)
        self._check(self._lib.gr_vcorr_read(self._handle(), _ptr(c1), _ptr(c2), _ptr(pairs)))
        return c1, c2, pairs

    def correlate_each(self, max_lag=None):
        """(c1 float64 [V, L], c2 float64 [V, L]): the curves of every vector, the mean over the pairs of good frames; None for a rank
        that is not kept"""
        n = self.n_frames
        lag = self._lag(max_lag)
        lags = min(lag, max(n, 1) - 1) + 1
        c1 = np.zeros((self.n_vectors, lags), np.float64) if self._kept(1) else None
        c2 = np.zeros((self.n_vectors, lags), np.float64) if self._kept(2) else None
        self._check(self._lib.gr_vcorr_compute_each(self._handle(), lag, _ptr(c1), _ptr(c2)))
        return c1, c2

    def vectors(self, t0, nt):
        """float32 [nt, V, 3]: the vectors of frames t0 .. t0 + nt - 1 as the rank-1 panel holds them, the caller's order; zeros for a
        failed frame (needs rank 1)"""
        out = np.zeros((nt, self.n_vectors, 3), np.float32)
        self._check(self._lib.gr_vcorr_read_vectors(self._handle(), int(t0), int(nt), _ptr(out)))
        return out
