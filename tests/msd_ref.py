"""numpy restatement of the library's MSD (gr_msd_*; groan_rs_amd.MSD), shared by the host and the GPU tests.

THE APPEND RULE.  The panel is DEFINED by the walk of `Walk.append`, so the device's displacements are compared with it bit for bit:
  d = x - w                      one f32 subtraction per component
  k = rint(d * iL), +1 where fmaf(-k, L, d) > L/2, -1 where it is < -L/2       (gr_minimg_k; iL = float32(1) / L as gr_box_setup stores it)
  d = fmaf(-k, L, d)             along c, then b, then a, the off-diagonal components of the box vector likewise
  u += float64(d)                a sequential f64 chain (np.add.accumulate over the frames gives the same)
  entry = float32(u - float64(o))
fmaf(-k, L, d) is restated as float32(float64(d) - float64(k) * float64(L)).  For coordinates on the nm scale that rounds ONCE, like
the fused operation: k is a small integer and L an f32, so the f64 product is exact, and the f64 sum of two such terms is exact as long
as their bits span fewer than 53 binary places.  The one case in which they do not -- an off-diagonal term k * cx of order 1 nm added to
a |d| below 2^-29 nm -- could round twice; `fma32` closes it by rounding the f64 sum TO ODD from its exact error term (TwoSum) before the
f32 rounding, which makes the restatement the fused operation for every input, not only for the likely ones.

THE DIRECT MSD.  sum over the selected components and atoms of (d_t - d_t')^2 in f64 (or long double), pair by pair -- no Gram matrix.

THE INPUTS.  Seeded random walks of sigma = 0.05 nm per step and component in periodic cells of at least 3 nm, wrapped into the cell: no
|d| comes near half a box edge and rint never sees a tie (tests/test_msd_host.py checks both on the CPU).  One orthorhombic cell, one
general triclinic cell, one cell rescaled by a few parts in 10^3 from frame to frame (the positions scale with it, as under a barostat)."""
import os
import re

import numpy as np

F, D = np.float32, np.float64
OK, E_NO_BOX, E_NO_POSITION, E_INVALID_ARG = 0, 1, 6, 10
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIGMA = 0.05
CELLS = {"ortho": [3.0, 3.5, 4.0, 0, 0, 0, 0, 0, 0], "tric": [3.2, 3.4, 3.1, 0, 0, 0.7, 0, -0.9, 1.1], "rescaled": [3.3, 3.0, 3.6, 0, 0, 0, 0, 0, 0]}


def source_ahead():
    """GR_FL_AHEAD of the kernel source: the frames whose rows a lane has in flight"""
    src = open(os.path.join(ROOT, "groan_rs_amd", "csrc", "gr_fluct.h")).read()
    return int(re.search(r"#define\s+GR_FL_AHEAD\s+(\d+)\b", src).group(1))


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


# ------------------------------------------------------------------------------------------------ the inputs
def _vectors(box9):
    b = np.asarray(box9, D)
    return np.array([b[0], 0.0, 0.0]), np.array([b[5], b[1], 0.0]), np.array([b[7], b[8], b[2]])       # a, b, c (gro order: v1x v2y v3z v1y v1z v2x v2z v3x v3y)


def _wrap(r, box9):
    """r [N, 3] f64 into the cell spanned by a, b, c -> (wrapped, image counts [N, 3])"""
    a, b, c = _vectors(box9)
    sc = np.floor(r[:, 2] / c[2]); r = r - sc[:, None] * c
    sb = np.floor(r[:, 1] / b[1]); r = r - sb[:, None] * b
    sa = np.floor(r[:, 0] / a[0]); r = r - sa[:, None] * a
    return r, np.stack([sa, sb, sc], 1)


def walk(n_atoms, n_frames, seed, cell="ortho", sigma=SIGMA):
    """-> (frames [n_frames][n_atoms, 3] f32 wrapped into the cell, boxes [n_frames][9] f32, U [n_frames, n_atoms, 3] f64: the unwrapped
    walk the frames were cut from, crossings [n_atoms]: how often an atom changed its image).  "rescaled": the cell and the wrapped
    positions are scaled by 1 + up to 3e-3 per frame before the step, as a barostat scales them; U follows the wrapped atom."""
    rng = np.random.default_rng(seed)
    box = np.asarray(CELLS[cell], D).copy()
    p = rng.random((n_atoms, 3)) @ np.stack(_vectors(box))
    p, _ = _wrap(p, box)
    u = p.copy()
    frames, boxes, U, crossings = [], [], [], np.zeros(n_atoms, np.int64)
    for t in range(n_frames):
        if t:
            mu = 1.0 + (3e-3 * (2 * rng.random() - 1) if cell == "rescaled" else 0.0)
            box = np.asarray((box * mu).astype(F), D)
            step = np.clip(rng.standard_normal((n_atoms, 3)), -4, 4) * sigma
            q = mu * p + step
            u = u + (q - p)
            p, img = _wrap(q, box)
            crossings += (img != 0).any(1)
        frames.append(p.astype(F)); boxes.append(box.astype(F)); U.append(u.copy())
    return frames, boxes, np.stack(U), crossings


# ------------------------------------------------------------------------------------------------ the append rule
def fma32(a, b, c):
    """float32(a * b + c) rounded once, for f32 a, b, c whose product is exact in f64 (|a| a small integer here)"""
    a, b, c = np.asarray(a, F).astype(D), np.asarray(b, F).astype(D), np.asarray(c, F).astype(D)
    p = a * b                                                     # exact: at most 48 bits
    s = p + c
    bb = s - p
    e = (p - (s - bb)) + (c - bb)                                 # TwoSum: p + c = s + e exactly
    even = (s.view(np.int64) & 1) == 0
    odd = np.where((e != 0.0) & even, np.nextafter(s, np.where(e > 0.0, np.inf, -np.inf)), s)      # round to odd: no second rounding can tie
    return odd.astype(F)


def minimg_k(d, L, seen=None):
    """gr_minimg_k(d, L, 1 / L, L / 2); seen: a list that collects what rint was given"""
    L = F(L)
    iL, h = F(1.0) / L, L / F(2.0)
    if seen is not None:
        seen.append(d * iL)
    k = np.rint(d * iL).astype(F)
    r = fma32(-k, L, d)
    return (k + (r > h).astype(F) - (r < -h).astype(F)).astype(F)


def reduce_step(d, box9, seen=None):
    """d [N, 3] f32 reduced along c, then b, then a: the brick reduction of gr_min_image_vec's non-orthogonal branch, no table refinement"""
    b = np.asarray(box9, F)
    ax, by, cz, bx, cx, cy = b[0], b[1], b[2], b[5], b[7], b[8]
    dx, dy, dz = d[:, 0].copy(), d[:, 1].copy(), d[:, 2].copy()
    k = minimg_k(dz, cz, seen)
    dx, dy, dz = fma32(-k, cx, dx), fma32(-k, cy, dy), fma32(-k, cz, dz)
    k = minimg_k(dy, by, seen)
    dx, dy = fma32(-k, bx, dx), fma32(-k, by, dy)
    k = minimg_k(dx, ax, seen)
    dx = fma32(-k, ax, dx)
    return np.stack([dx, dy, dz], 1)


def dims_mask(dims):
    return np.array([c in dims for c in "xyz"])


class Walk:
    """the object's state and panel: o, w (f32 [S, 3]), u (f64 [S, 3]), rows [T][S, 3] f32, ok [T]"""

    def __init__(self, n_atoms, dims="xyz", nojump=True):
        self.S, self.mask, self.nojump = n_atoms, dims_mask(dims), nojump
        self.o = self.w = self.u = None
        self.rows, self.ok, self.us = [], [], []

    def append(self, frames, boxes, idx):
        """-> (status [len(frames)], the first atom without position per frame or -1); boxes[f] None: the frame has no box"""
        st, bad = np.zeros(len(frames), np.int32), np.full(len(frames), -1, np.int64)
        for f, x in enumerate(frames):
            p = np.asarray(x, F)[idx]
            nan = np.isnan(p[:, 0])
            if self.nojump and boxes[f] is None:                  # the host check comes first (the library's first-error order per frame)
                st[f] = E_NO_BOX
            elif nan.any():
                st[f], bad[f] = E_NO_POSITION, int(np.asarray(idx)[nan].min())
            if st[f]:
                self.rows.append(np.zeros((self.S, 3), F)); self.ok.append(False)
                continue
            if self.o is None:
                self.o, self.w, self.u = p.copy(), p.copy(), p.astype(D)
            else:
                if self.nojump:
                    d = reduce_step(p - self.w, boxes[f])
                    self.u = self.u + d.astype(D)
                else:
                    self.u = p.astype(D)
                self.w = p.copy()
            row = (self.u - self.o.astype(D)).astype(F)
            row[:, ~self.mask] = 0.0
            self.rows.append(row); self.ok.append(True); self.us.append(self.u.copy())
        return st, bad

    def panel(self):
        return np.stack(self.rows) if self.rows else np.zeros((0, self.S, 3), F)


# ------------------------------------------------------------------------------------------------ the direct MSD
def direct_msd(panel, ok, max_lag=None, dtype=D):
    """-> (msd [L], pairs [L], qsum [L]: the sum over a lag's pairs of q_t + q_t', the scale of the device's rounding bound).  panel
    [T, S, 3] f32, every pair of good frames evaluated as sum (d_t - d_t')^2 in `dtype`"""
    T, S = panel.shape[0], panel.shape[1]
    L = T if max_lag is None else min(max_lag, T - 1) + 1
    X = panel.reshape(T, -1).astype(dtype)
    q = (X * X).sum(1)
    ok = np.asarray(ok, bool)
    msd, pairs, qsum = np.full(L, np.nan), np.zeros(L, np.uint64), np.zeros(L)
    for tau in range(L):
        both = ok[:T - tau] & ok[tau:]
        n = int(both.sum())
        pairs[tau] = n
        if n:
            diff = X[tau:][both] - X[:T - tau][both]
            msd[tau] = float((diff * diff).sum(1).sum() / dtype(n) / dtype(S)) if tau else 0.0
            qsum[tau] = float((q[tau:][both] + q[:T - tau][both]).sum())
    return msd, pairs, qsum


def msd_bound(qsum, pairs, n_pad, S):
    """the bound on |msd - direct| per lag: (2 K + 4) 2^-53 (q_t + q_t') per pair (tests/test_gpu_msd.py derives it), K = 3 n_pad, plus
    the additions of a lag's pairs -- at most `pairs` of them, each within 2^-53 of a partial sum that is at most the sum of the |D2|,
    and |D2| <= 2 (q_t + q_t') -- divided like the mean"""
    K = 3 * n_pad
    p = np.maximum(pairs.astype(D), 1.0)
    return ((2 * K + 4) + 2.0 * p) * 2.0 ** -53 * qsum / (p * S)
