"""Internals on resident frames: the distance, angle, dihedral or axis cosine of a fixed list of atom tuples in every frame.

"What is this bond length, this angle or this torsion in every frame?" -- Ramachandran maps, side-chain chi angles, distance and
angle series, lipid order parameters.  The reference has Vector3D::angle and distance only; its users download every frame and gather
in numpy.  Here `values` gives the series of a block of resident slots in one C call (gr_internals_values_batch: one lane per tuple
walks the frames), and `accumulate` keeps per tuple an origin (f32, the first counted frame), the sum of d = v - origin and of d * d
(f64), added frame after frame in ascending order, without storing the series.  Angles are in radians; the dihedral's sign is IUPAC's
(include/groan_hip.h has the definitions and the pins).  No arithmetic on atoms happens in Python.
"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import (OK, E_INCONSISTENT_GROUP, E_NO_BOX, E_NO_POSITION, E_NOT_ORTHOGONAL, E_OUT_OF_RANGE, E_UNSUPPORTED_BOX, E_ZERO_BOX)
from .system import AtomError, DeviceError, GroupError, _ptr, _simbox

KINDS = {"distance": (_lib.IC_DISTANCE, 2), "angle": (_lib.IC_ANGLE, 3), "dihedral": (_lib.IC_DIHEDRAL, 4), "axis": (_lib.IC_AXIS, 2)}


def _neighbours(bonds):
    b = np.asarray(bonds, np.int64).reshape(-1, 2)
    nb = {}
    for i, j in b.tolist():
        if i != j:
            nb.setdefault(i, set()).add(j)
            nb.setdefault(j, set()).add(i)
    return nb


def angles_from_bonds(bonds):
    """every bond angle i-j-k of the bond list `bonds` ([n, 2], what gr_add_bonds takes) with i < k -> uint64 [n, 3], sorted"""
    nb = _neighbours(bonds)
    out = [(i, j, k) for j, around in nb.items() for i in around for k in around if i < k]
    return np.array(sorted(out), np.uint64).reshape(-1, 3)


def dihedrals_from_bonds(bonds):
    """every proper dihedral i-j-k-l of the bond list with j < k and i != l (i, l off the central bond) -> uint64 [n, 4], sorted"""
    nb = _neighbours(bonds)
    out = [(i, j, k, l) for j, around in nb.items() for k in around if j < k
           for i in around if i != k for l in nb[k] if l != j and l != i]
    return np.array(sorted(out), np.uint64).reshape(-1, 4)


class Internals:
    """the series and the running statistics of `tuples` ([T, arity] atom indices) of one `kind`: "distance" (i, j), "angle" (i, j, k:
    vertex j), "dihedral" (i, j, k, l) or "axis" (i, j: the cosine of i->j against `axis`).  pbc: displacements take the minimum image
    of the frame's own box (and a frame needs one)"""

    def __init__(self, system, kind, tuples, pbc=True, axis=None):
        self._lib = _lib.load()
        self.system, self.kind, self._f = system, kind, None
        if kind not in KINDS:
            raise ValueError("kind is one of %s, not %r" % (", ".join(sorted(KINDS)), kind))
        code, arity = KINDS[kind]
        t = np.ascontiguousarray(np.asarray(tuples, np.uint64).reshape(-1, arity))
        ax = None if axis is None else np.ascontiguousarray(np.asarray(axis, np.float32).reshape(3))
        if kind != "axis" and axis is not None:
            raise ValueError("only kind 'axis' takes an axis")
        self.flags = _lib.IC_PBC if pbc else 0
        st = C.c_int(0)
        self._f = self._lib.gr_internals_create(system._ctx, code, _ptr(t), len(t), self.flags, _ptr(ax), C.byref(st))
        if not self._f:
            self._raise(st.value)
        self.tuples, self.arity = t, arity
        self.n_tuples = int(self._lib.gr_internals_count(self._f))
        system._plans.append(self)

    # -- lifetime: close() (or `with`) frees the device buffers now; System.close() closes what is still open, before its context goes
    def close(self):
        if getattr(self, "_f", None):
            self._lib.gr_internals_destroy(self._f)
            self._f = None

    def __enter__(self): return self
    def __exit__(self, *a): self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __len__(self):
        return self.n_tuples

    def _raise(self, status):
        lib, ctx = self._lib, self.system._ctx
        msg = lib.gr_last_error(ctx).decode(errors="replace")
        idx = int(lib.gr_last_error_index(ctx))
        if status == E_OUT_OF_RANGE: raise AtomError("OutOfRange", idx, status)
        if status == E_NO_POSITION: raise AtomError("InvalidPosition", idx, status)
        if status in (E_NO_BOX, E_NOT_ORTHOGONAL, E_ZERO_BOX, E_UNSUPPORTED_BOX): raise _simbox(status)
        if status == E_INCONSISTENT_GROUP: raise GroupError("InconsistentGroup", msg, status)
        raise DeviceError(lib.gr_status_string(status).decode(), msg, status)

    def _check(self, status):
        if status != OK:
            self._raise(status)

    def _handle(self):
        if not self._f:
            raise ValueError("the Internals object is closed")
        return self._f

    # -- the series
    def values(self, first_slot, n_frames, raise_on_error=True):
        """-> (float32 [n_frames, T], status int32 [n_frames]); a failed frame (no box with pbc, a named atom without position) is a row of NaN"""
        out = np.zeros((n_frames, self.n_tuples), np.float32); st_arr = np.zeros(n_frames, np.int32)
        st = self._lib.gr_internals_values_batch(self._handle(), first_slot, n_frames, _ptr(out), _ptr(st_arr))
        if st != OK and raise_on_error:
            self._raise(st)
        return out, st_arr

    def values_device(self, out, first_slot, n_frames, ld=None, raise_on_error=True):
        """the same, left on the device: `out` is a float32 torch tensor [>= n_frames, >= T] on the system's device whose rows are
        contiguous (stride(1) == 1; stride(0) is the row pitch) -- or a device pointer (int or ctypes.c_void_p, e.g. one the library
        handed out) with `ld`, the floats per row.  Columns beyond T are not written.  -> status int32 [n_frames]"""
        if hasattr(out, "data_ptr"):
            if str(out.dtype) != "torch.float32" or out.dim() != 2 or out.shape[0] < n_frames or out.shape[1] < self.n_tuples or (out.shape[1] > 1 and out.stride(1) != 1) or not out.is_cuda:
                raise ValueError("values_device wants a float32 device tensor [>= n_frames, >= T] with contiguous rows")
            ptr, ld = out.data_ptr(), out.stride(0) if out.shape[0] > 1 else max(out.stride(0), out.shape[1])
        else:
            ptr = out.value if isinstance(out, C.c_void_p) else int(out)
            if ld is None or not ptr:
                raise ValueError("values_device with a device pointer wants ld, the floats per row")
        st_arr = np.zeros(n_frames, np.int32)
        st = self._lib.gr_internals_values_batch_device(self._handle(), first_slot, n_frames, C.c_void_p(ptr), int(ld), _ptr(st_arr))
        if st != OK and raise_on_error:
            self._raise(st)
        return st_arr

    # -- the statistics
    def accumulate(self, first_slot, n_frames, raise_on_error=True):
        """counts slots first_slot .. first_slot + n_frames - 1 -> status int32 [n_frames]; a failed frame is counted for no tuple"""
        st_arr = np.zeros(n_frames, np.int32)
        st = self._lib.gr_internals_accumulate_batch(self._handle(), first_slot, n_frames, _ptr(st_arr))
        if st != OK and raise_on_error:
            self._raise(st)
        return st_arr

    def clear(self):
        self._check(self._lib.gr_internals_clear(self._handle()))

    @property
    def n_frames(self):
        """frames counted by accumulate"""
        return int(self._lib.gr_internals_frames(self._handle()))

    def read(self):
        """-> (mean, var) float64 [T] each over the counted frames (var divided by n); a dihedral's mean lies in (-pi, pi]"""
        mean, var = np.zeros(self.n_tuples, np.float64), np.zeros(self.n_tuples, np.float64)
        self._check(self._lib.gr_internals_read(self._handle(), _ptr(mean), _ptr(var)))
        return mean, var

    def read_raw(self):
        """(origin float32 [T], sum float64 [T], sum of squares float64 [T], n): the state as it stands"""
        o, s, q = np.zeros(self.n_tuples, np.float32), np.zeros(self.n_tuples, np.float64), np.zeros(self.n_tuples, np.float64)
        n = C.c_uint64(0)
        self._check(self._lib.gr_internals_read_raw(self._handle(), _ptr(o), _ptr(s), _ptr(q), C.byref(n)))
        return o, s, q, int(n.value)

    def order_parameter(self):
        """S = 1/2 <3 cos^2 theta - 1> per tuple, kind "axis" only: 1.5 (var + mean^2) - 0.5"""
        if self.kind != "axis":
            raise ValueError("order_parameter belongs to kind 'axis'")
        mean, var = self.read()
        return 1.5 * (var + mean * mean) - 0.5

    def merge(self, other):
        """adds the frames of `other` (same kind, flags, axis and tuples; any context, any device) to this object"""
        self._check(self._lib.gr_internals_merge(self._handle(), other._handle()))

    def set_launch(self, tuple_ranges=0, frame_chunk=0):
        """test hook: the ranges the tuples are cut into and the frames of one workgroup of values (0: the default).  No result depends on it"""
        if not self._f or self._lib.gr_internals_set_launch(self._f, int(tuple_ranges), int(frame_chunk)) != OK:
            raise ValueError("set_launch on a closed Internals object")

    def stat(self, key):
        v = C.c_uint64(0)
        if self._lib.gr_internals_stat(self._handle(), int(key), C.byref(v)) != OK:
            raise ValueError("unknown internals stat %r" % (key,))
        return int(v.value)
