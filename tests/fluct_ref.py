"""numpy restatement of the library's Fluctuations (gr_fluct_*; groan_rs_amd.Fluctuations), shared by the host and the GPU tests.

The raw state is DEFINED by the walk below -- origin = the first counted frame (f32), d = x - origin as ONE f32 subtraction, then
s += d and q += d * d in f64, frame after frame in ascending order -- so the device's state is compared with it bit for bit.  (d * d of
a widened f32 is exact in f64: whether the device fuses the multiply into the add changes nothing.)  two_pass() is the independent
reference of the CLOSED results: mean and RMSF straight from the f64 frames, no origin, no running sums."""
import os
import re

import numpy as np

F, D = np.float32, np.float64
OK, E_INCONSISTENT_GROUP, E_NO_POSITION, E_INVALID_ARG = 0, 5, 6, 10
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def source_ahead():
    """GR_FL_AHEAD of the kernel source: the frames whose rows a lane has in flight"""
    src = open(os.path.join(ROOT, "groan_rs_amd", "csrc", "gr_fluct.h")).read()
    return int(re.search(r"#define\s+GR_FL_AHEAD\s+(\d+)\b", src).group(1))


class State:
    def __init__(self, n_atoms):
        self.o, self.s, self.q, self.n = np.zeros((n_atoms, 3), F), np.zeros((n_atoms, 3), D), np.zeros((n_atoms, 3), D), 0

    def accumulate(self, frames, idx):
        """-> (status [len(frames)], index of the first atom without position per frame or -1); a failed frame is counted for no atom"""
        st, bad = np.zeros(len(frames), np.int32), np.full(len(frames), -1, np.int64)
        for f, x in enumerate(frames):
            p = np.asarray(x, F)[idx]
            nan = np.isnan(p[:, 0])
            if nan.any():
                st[f], bad[f] = E_NO_POSITION, int(np.asarray(idx)[nan].min())
                continue
            if self.n == 0:
                self.o = p.copy()
            d = (p - self.o).astype(D)          # the f32 subtraction, then widened
            self.s += d
            self.q += d * d
            self.n += 1
        return st, bad

    def close(self):
        """-> mean [S, 3], var [S, 3], rmsf [S], f64 (NaN before the first counted frame)"""
        if self.n == 0:
            nan = np.full(self.s.shape, np.nan)
            return nan, nan.copy(), np.full(len(self.s), np.nan)
        n = D(self.n)
        mean = self.o.astype(D) + self.s / n
        var = np.maximum(self.q - self.s * self.s / n, 0.0) / n
        return mean, var, np.sqrt(var.sum(1))

    def merge(self, src):
        """src's frames added to this state: its sums moved to this origin in f64"""
        if src.n == 0:
            return
        if self.n == 0:
            self.o, self.s, self.q, self.n = src.o.copy(), src.s.copy(), src.q.copy(), src.n
            return
        delta = src.o.astype(D) - self.o.astype(D)
        ns = D(src.n)
        self.s += src.s + ns * delta
        self.q += src.q + 2.0 * delta * src.s + ns * delta * delta
        self.n += src.n


def two_pass(frames, idx):
    """mean [S, 3], var [S, 3], rmsf [S] of the frames that have every atom of idx, in two passes over the f64 positions"""
    X = np.stack([np.asarray(x, F)[idx].astype(D) for x in frames if not np.isnan(np.asarray(x)[idx, 0]).any()])
    mean = X.sum(0) / len(X)
    var = ((X - mean) ** 2).sum(0) / len(X)
    return mean, var, np.sqrt(var.sum(1))


def fitted_frames(n_atoms, n_frames, seed, extent=14.0):
    """frames as a fit leaves them: one structure within |x| <= extent plus per-atom thermal motion (0.01 .. 0.4 nm), [n_frames][n_atoms, 3] f32"""
    rng = np.random.default_rng(seed)
    base = (rng.random((n_atoms, 3)) * 2 - 1) * extent
    sigma = 0.01 + 0.39 * rng.random((n_atoms, 1))
    return [(base + sigma * np.clip(rng.standard_normal((n_atoms, 3)), -4, 4)).astype(F) for _ in range(n_frames)]


def jumping_frames(n_atoms, n_frames, seed, extent=16.0):
    """every atom anywhere in the box in every frame: the worst case for the running sums"""
    rng = np.random.default_rng(seed)
    return [((rng.random((n_atoms, 3)) * 2 - 1) * extent).astype(F) for _ in range(n_frames)]


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))
