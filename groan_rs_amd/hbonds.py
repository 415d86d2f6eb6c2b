"""Hydrogen-bond analysis on resident frames: HBondChain / HBondAnalysis / HBondError (src/system/hbonds.rs, errors.rs:655-690).

The plan (chains resolved to acceptors, donors with their bonded hydrogens, the pairs' segments) is built once by
gr_hbond_plan_create; `batch` analyses a block of resident slots in one C call (gr_hbond_batch), `analyze` is the
FrameAnalyze form for one slot and returns the reference's HBondMap: {(chain1, chain2): bonds}.
"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import (OK, E_DUPLICATE_PAIR, E_EMPTY_CHAIN, E_GROUP_NOT_FOUND, E_INVALID_ARG, E_NO_BOX, E_NO_POSITION, E_NONEXISTENT_CHAIN,
                   E_NOT_ORTHOGONAL, E_OUT_OF_RANGE, E_UNUSED_CHAIN, E_ZERO_BOX)
from .system import AtomError, DeviceError, GroanError, _ptr, _simbox
from .traj import FrameAnalyze

HBOND_DTYPE = np.dtype([("donor", np.uint32), ("hydrogen", np.uint32), ("acceptor", np.uint32), ("distance", np.float32), ("angle", np.float32)])


class HBondError(GroanError):       # errors.rs:655-690
    pass


class HBondChain:
    """HBondChain::new: group names (of the System) for the acceptors, donors and hydrogens of one chain"""

    def __init__(self, acceptors, donors, hydrogens):
        self.acceptors, self.donors, self.hydrogens = acceptors, donors, hydrogens


class HBondAnalysis(FrameAnalyze):
    """HBondAnalysis on the device.  `bonds`: [n, 2] atom indices of the system's bonds (either order)."""

    def __init__(self, system, chains, pairs, max_distance, min_angle, bonds, slot=0):
        self._lib = _lib.load()
        self.system, self.slot = system, slot
        self.pairs = [(int(a), int(b)) for a, b in pairs]
        names = (C.c_char_p * (3 * len(chains) or 1))()
        self._names = [n.encode() for ch in chains for n in (ch.acceptors, ch.donors, ch.hydrogens)]
        for k, n in enumerate(self._names):
            names[k] = n
        pr = np.ascontiguousarray(np.asarray(self.pairs, np.uint32).reshape(-1, 2))
        bd = np.ascontiguousarray(np.asarray(bonds, np.uint64).reshape(-1, 2))
        st = C.c_int(0)
        self._plan = self._lib.gr_hbond_plan_create(system._ctx, names, len(chains), _ptr(pr), len(self.pairs), _ptr(bd), bd.shape[0],
                                                    C.c_float(max_distance), C.c_float(min_angle), C.byref(st))
        if not self._plan:
            self._raise(st.value, plan=True)
        self._cap = 0          # capacity hint: bonds of the largest batch so far (steady state: one C call per batch)
        system._plans.append(self)

    def close(self):
        if getattr(self, "_plan", None):
            self._lib.gr_hbond_plan_destroy(self._plan)
            self._plan = None

    def _raise(self, status, plan=False):
        lib, ctx = self._lib, self.system._ctx
        msg = lib.gr_last_error(ctx).decode(errors="replace")
        idx = int(lib.gr_last_error_index(ctx))
        if status == E_EMPTY_CHAIN: raise HBondError("EmptyChain", idx, status)
        if status == E_NONEXISTENT_CHAIN: raise HBondError("NonexistentChain", idx, status)
        if status == E_DUPLICATE_PAIR: raise HBondError("PairSpecifiedMultipleTimes", self.pairs[idx], status)
        if status == E_UNUSED_CHAIN: raise HBondError("UnusedChain", None, status)
        if status == E_GROUP_NOT_FOUND: raise HBondError("SelectError", msg, status)
        if status == E_INVALID_ARG and plan: raise HBondError("CellGridError", "InvalidCellSize", status)
        if status in (E_NO_BOX, E_NOT_ORTHOGONAL, E_ZERO_BOX): raise HBondError("InvalidSimBox", _simbox(status), status)
        if status == E_NO_POSITION: raise HBondError("AtomError", AtomError("InvalidPosition", idx, status), status)
        if status == E_OUT_OF_RANGE: raise HBondError("AtomError", AtomError("OutOfRange", idx, status), status)
        raise DeviceError(lib.gr_status_string(status).decode(), msg, status)

    def _call(self, first_slot, n, cap, offsets, total, status):
        if cap:
            out = [np.empty(cap, np.uint32) for _ in range(3)] + [np.empty(cap, np.float32) for _ in range(2)]
        else:
            out = [None] * 5
        st = self._lib.gr_hbond_batch(self._plan, first_slot, n, cap, *[_ptr(a) for a in out], _ptr(offsets), C.byref(total), _ptr(status))
        return st, out

    def batch(self, first_slot, n_frames, raise_on_error=True):
        """-> (donor, hydrogen, acceptor, distance, angle, offsets uint64 [n_frames * n_pairs + 1], status int32 [n_frames]);
        the bonds of frame f and pair p are offsets[f * n_pairs + p] .. offsets[f * n_pairs + p + 1]"""
        offsets = np.zeros(n_frames * len(self.pairs) + 1, np.uint64)
        status = np.zeros(n_frames, np.int32)
        total = C.c_uint64(0)
        st, out = self._call(first_slot, n_frames, self._cap, offsets, total, status)
        if int(total.value) > self._cap or not self._cap:
            self._cap = max(int(total.value) + int(total.value) // 4, 1)
            st, out = self._call(first_slot, n_frames, self._cap, offsets, total, status)
        if st != OK and raise_on_error:
            self._raise(st)
        m = int(total.value)
        return tuple(a[:m] for a in out) + (offsets, status)

    def count(self, first_slot, n_frames):
        """count-only form (NULL buffers): -> (offsets, status, n_total)"""
        offsets = np.zeros(n_frames * len(self.pairs) + 1, np.uint64)
        status = np.zeros(n_frames, np.int32)
        total = C.c_uint64(0)
        self._lib.gr_hbond_batch(self._plan, first_slot, n_frames, 0, None, None, None, None, None, _ptr(offsets), C.byref(total), _ptr(status))
        return offsets, status, int(total.value)

    @staticmethod
    def to_map(pairs, arrays, offsets, frame=0):
        """one frame of a batch as the reference's HBondMap: {(c1, c2): structured array (donor, hydrogen, acceptor, distance, angle)}"""
        don, hyd, acc, dist, ang = arrays
        out = {}
        np_ = len(pairs)
        for p, key in enumerate(pairs):
            a, b = int(offsets[frame * np_ + p]), int(offsets[frame * np_ + p + 1])
            rec = np.empty(b - a, HBOND_DTYPE)
            rec["donor"], rec["hydrogen"], rec["acceptor"], rec["distance"], rec["angle"] = don[a:b], hyd[a:b], acc[a:b], dist[a:b], ang[a:b]
            out[key] = rec
        return out

    def analyze(self, system):
        """FrameAnalyze::analyze -> HBondMap of the System's current slot"""
        r = self.batch(self.slot, 1)
        return self.to_map(self.pairs, r[:5], r[5], 0)
