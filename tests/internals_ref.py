"""The f64 restatement of Internals (gr_internals_*): values of atom tuples from f32 positions in f64 arithmetic, the error bounds the
tests hold the device to, an f32 emulation of the device's arithmetic, the sums `accumulate` keeps restated from the rows `values`
returns, and the generators of the tests' inputs.

Boxes are box9 in gro order (v1x v2y v3z v1y v1z v2x v2z v3x v3y); the minimum image is an exhaustive 5 x 5 x 5 image search."""
import itertools
import os
import re

import numpy as np

F = np.float32
ARITY = {"distance": 2, "angle": 3, "dihedral": 4, "axis": 2}
E_NO_BOX, E_NO_POSITION, E_OUT_OF_RANGE, E_INVALID_ARG, E_INCONSISTENT_GROUP = 1, 6, 9, 10, 5
PI_F = F(np.pi)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def source_ahead():
    """GR_IC_AHEAD as the kernel's source has it: the edge tests are written around it"""
    src = open(os.path.join(ROOT, "groan_rs_amd", "csrc", "gr_internals.h")).read()
    return int(re.search(r"#define\s+GR_IC_AHEAD\s+(\d+)", src).group(1))


def ulp32(x):
    """the spacing of f32 at |x|"""
    return np.spacing(np.abs(np.asarray(x, F))).astype(np.float64)


def lattice(box9):
    b = np.asarray(box9, np.float64)
    return np.array([[b[0], b[3], b[4]], [b[5], b[1], b[6]], [b[7], b[8], b[2]]])


_SHIFTS = np.array(list(itertools.product(range(-2, 3), repeat=3)), np.float64)


def min_image(d, box9):
    """the shortest image of each row of d (f64 [n, 3]) among the 125 nearest after reduction along c, b, a"""
    L = lattice(box9)
    d = np.array(d, np.float64)
    for k in (2, 1, 0):
        d -= np.rint(d[:, k] / L[k, k])[:, None] * L[k]
    cand = d[:, None, :] + (_SHIFTS @ L)[None, :, :]
    best = np.argmin((cand * cand).sum(-1), axis=1)
    return cand[np.arange(len(d)), best]


def disp(pos, a, b, box9):
    d = pos[b].astype(np.float64) - pos[a].astype(np.float64)
    return d if box9 is None else min_image(d, box9)


def values64(kind, pos, tuples, box9=None, axis=None, parts=False):
    """f64 values of the tuples ([T, arity]) from the f32 positions pos [N, 3]; box9 None: no minimum image.
    parts: also the lengths the bounds are made of (see bounds())"""
    t = np.asarray(tuples, np.int64)
    if kind in ("distance", "axis"):
        d = disp(pos, t[:, 0], t[:, 1], box9)
        r = np.sqrt((d * d).sum(1))
        if kind == "distance":
            v, p = r, (r,)
        else:
            a = np.asarray(axis, np.float64)
            a = (a / np.sqrt((a * a).sum())).astype(F).astype(np.float64)
            v, p = np.where(r > 0, (d @ a) / np.where(r > 0, r, 1.0), 0.0), (r,)
    elif kind == "angle":
        u, w = disp(pos, t[:, 1], t[:, 0], box9), disp(pos, t[:, 1], t[:, 2], box9)
        c = np.cross(u, w)
        v = np.arctan2(np.sqrt((c * c).sum(1)), (u * w).sum(1))
        p = (np.sqrt((u * u).sum(1)), np.sqrt((w * w).sum(1)))
    else:
        b1, b2, b3 = disp(pos, t[:, 0], t[:, 1], box9), disp(pos, t[:, 1], t[:, 2], box9), disp(pos, t[:, 2], t[:, 3], box9)
        n1, n2 = np.cross(b1, b2), np.cross(b2, b3)
        l2 = np.sqrt((b2 * b2).sum(1))
        v = np.arctan2(l2 * (b1 * n2).sum(1), (n1 * n2).sum(1))
        p = (np.sqrt((n1 * n1).sum(1)) / l2, np.sqrt((n2 * n2).sum(1)) / l2)
    return (v, p) if parts else v


def bounds(kind, pos, tuples, box9=None, axis=None, E=None):
    """the largest |device value - values64| allowed, per tuple.  E = ulp_f32(largest |coordinate| among the frame's named atoms):
    the f32 displacement of a PBC-broken tuple is formed at the magnitude of the coordinates, not of the bond.
        distance 2E + 4 ulp(v);  axis 2E / |d| + 4 ulp(1);  angle 2E (1/|u| + 1/|v|) + 4 ulp(pi);
        dihedral 2E (1/rho1 + 1/rho4) + 4 ulp(pi), rho the end atoms' distances from the central axis"""
    t = np.asarray(tuples, np.int64)
    if E is None:                                                      # (given: per tuple, where pos stacks several frames)
        E = float(ulp32(np.abs(pos[np.unique(t)]).max()))
    v, p = values64(kind, pos, tuples, box9, axis, parts=True)
    if kind == "distance":
        return 2 * E + 4 * ulp32(v)
    if kind == "axis":
        return 2 * E / p[0] + 4 * float(ulp32(1.0))
    return 2 * E * (1 / p[0] + 1 / p[1]) + 4 * float(ulp32(np.pi))


def error(kind, got, want):
    """|got - want|, a dihedral's modulo 2 pi"""
    e = np.abs(np.asarray(got, np.float64) - want)
    return np.minimum(e, np.abs(2 * np.pi - e)) if kind == "dihedral" else e


# ---------------------------------------------------------------- the device's arithmetic in f32 numpy
def _fma(a, b, c):
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(F)


def _minimg_k(d, L, h):
    k = np.rint(d * (F(1) / L)).astype(F)
    r = _fma(-k, np.full_like(d, L), d)
    return (k + (r > h).astype(F) - (r < -h).astype(F)).astype(F)


def min_image32(d, box9):
    """gr_min_image_vec in f32: the brick reduction along c, b, a with fused steps, then the better of the 26 neighbours"""
    L = lattice(box9).astype(F)
    d = np.array(d, F)
    for k in (2, 1, 0):
        kk = _minimg_k(d[:, k], L[k, k], L[k, k] / F(2))
        for c in range(3):
            if L[k, c] != 0:
                d[:, c] = _fma(-kk, np.full_like(kk, L[k, c]), d[:, c])
    if not (L[1, 0] or L[2, 0] or L[2, 1]):
        return d
    sh = (np.array(list(itertools.product(range(-1, 2), repeat=3)), F) @ L).astype(F)
    cand = (d[:, None, :] + sh[None, :, :]).astype(F)
    best = np.argmin((cand * cand).sum(-1), axis=1)
    return cand[np.arange(len(d)), best]


def _disp32(pos, a, b, box9):
    d = (pos[b] - pos[a]).astype(F)
    return d if box9 is None else min_image32(d, box9)


def _dot32(a, b):
    return ((a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]).astype(F) + a[:, 2] * b[:, 2]).astype(F)


def _cross32(a, b):
    return np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2], a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], 1).astype(F)


def values32(kind, pos, tuples, box9=None, axis=None):
    """the formulas of include/groan_hip.h with every product and sum rounded to f32 on its own"""
    pos = np.asarray(pos, F)
    t = np.asarray(tuples, np.int64)
    if kind in ("distance", "axis"):
        d = _disp32(pos, t[:, 0], t[:, 1], box9)
        r = np.sqrt(_dot32(d, d)).astype(F)
        if kind == "distance":
            return r
        a = np.asarray(axis, np.float64)
        a = (a / np.sqrt((a * a).sum())).astype(F)
        return np.where(r > 0, (_dot32(d, np.broadcast_to(a, d.shape)) / np.where(r > 0, r, F(1))).astype(F), F(0))
    if kind == "angle":
        u, w = _disp32(pos, t[:, 1], t[:, 0], box9), _disp32(pos, t[:, 1], t[:, 2], box9)
        c = _cross32(u, w)
        return np.arctan2(np.sqrt(_dot32(c, c)).astype(F), _dot32(u, w)).astype(F)
    b1, b2, b3 = _disp32(pos, t[:, 0], t[:, 1], box9), _disp32(pos, t[:, 1], t[:, 2], box9), _disp32(pos, t[:, 2], t[:, 3], box9)
    n1, n2 = _cross32(b1, b2), _cross32(b2, b3)
    return np.arctan2((np.sqrt(_dot32(b2, b2)).astype(F) * _dot32(b1, n2)).astype(F), _dot32(n1, n2)).astype(F)


# ---------------------------------------------------------------- the sums accumulate keeps, from the rows values returns
class State:
    """o (f32), s, q (f64), n: per tuple, over the rows handed to add() in order; a row of NaN (a failed frame) is counted for no tuple"""

    def __init__(self, kind, T):
        self.kind, self.n = kind, 0
        self.o, self.s, self.q = np.zeros(T, F), np.zeros(T, np.float64), np.zeros(T, np.float64)

    def delta(self, row):
        d = (np.asarray(row, F) - self.o).astype(F)                    # ONE f32 subtraction
        if self.kind == "dihedral":                                    # reduced once, in f32
            two = F(2) * PI_F
            d = np.where(d > PI_F, (d - two).astype(F), np.where(d < -PI_F, (d + two).astype(F), d)).astype(F)
        return d.astype(np.float64)

    def add(self, rows):
        for row in np.asarray(rows, F):
            if np.isnan(row).all():
                continue
            if self.n == 0:
                self.o = row.copy()
            d = self.delta(row)
            self.s = self.s + d                                        # one f64 chain per tuple, in frame order
            self.q = self.q + d * d                                    # (d * d is exact in f64: fma(d, d, q) rounds once, like this)
            self.n += 1
        return self

    def close(self):
        mean = self.o.astype(np.float64) + self.s / self.n
        if self.kind == "dihedral":
            mean = np.where(mean > np.pi, mean - 2 * np.pi, np.where(mean <= -np.pi, mean + 2 * np.pi, mean))
        return mean, np.maximum(self.q - self.s * self.s / self.n, 0.0) / self.n

    def two_pass(self, rows):
        """mean and variance of the same d terms, two passes in f64 (needs the origin: call after add)"""
        d = np.stack([self.delta(r) for r in np.asarray(rows, F) if not np.isnan(r).all()])
        m = d.mean(0)
        mean = self.o.astype(np.float64) + m
        if self.kind == "dihedral":
            mean = np.where(mean > np.pi, mean - 2 * np.pi, np.where(mean <= -np.pi, mean + 2 * np.pi, mean))
        return mean, ((d - m) ** 2).mean(0)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


# ---------------------------------------------------------------- inputs
def wrap(x, box9):
    """positions (f64) into the cell, along c, b, a"""
    L = lattice(box9)
    x = np.array(x, np.float64)
    for k in (2, 1, 0):
        x -= np.floor(x[:, k] / L[k, k])[:, None] * L[k]
    return x


def chains(n, box9, seed):
    """n four-atom chains (atoms 4c .. 4c + 3): bonds of 0.09 .. 0.2 nm, bond angles of 60 .. 150 degrees, any torsion, anywhere in the
    cell -> (f32 [4n, 3] wrapped into the cell so that most chains are broken, f32 [4n, 3] the same chains whole).  Chains that miss the
    conditions of the bounds after rounding to f32 are drawn again."""
    rng = np.random.default_rng(seed)
    L = lattice(box9)
    out_w, out_u = np.zeros((4 * n, 3), F), np.zeros((4 * n, 3), F)
    todo = np.arange(n)
    while len(todo):
        m = len(todo)

        def unit(k):
            v = rng.standard_normal((k, 3))
            return v / np.sqrt((v * v).sum(1))[:, None]

        def bend(prev, theta):
            """a unit vector at angle pi - theta from -prev ... i.e. the bond angle at the joint is theta"""
            r = unit(len(prev))
            perp = r - (r * prev).sum(1)[:, None] * prev
            perp /= np.sqrt((perp * perp).sum(1))[:, None]
            return -np.cos(theta)[:, None] * prev + np.sin(theta)[:, None] * perp

        e1 = unit(m)
        e2 = bend(e1, np.radians(rng.uniform(62, 148, m)))
        e3 = bend(e2, np.radians(rng.uniform(62, 148, m)))
        l = rng.uniform(0.092, 0.198, (m, 3))
        q = np.stack([0 * e1, l[:, :1] * e1, l[:, :1] * e1 + l[:, 1:2] * e2, l[:, :1] * e1 + l[:, 1:2] * e2 + l[:, 2:] * e3], 1)
        # the chain's centre: anywhere, but for 9 chains in 10 moved along x, y or z to within 0.03 nm of that face of the cell the wrap
        # fills (a brick: z is reduced first, then y, then x), so that the wrap breaks most chains
        p = q + (rng.random((m, 3)) @ L)[:, None, :]
        near, k = np.nonzero(rng.random(m) < 0.9)[0], rng.integers(0, 3, m)
        centre = wrap(p.mean(1), box9)
        p[near, :, k[near]] += (rng.uniform(-0.03, 0.03, len(near)) - centre[near, k[near]])[:, None]
        p = p.reshape(-1, 3)
        pw = wrap(p, box9).astype(F)
        pu = p.astype(F)
        ok = chain_ok(pw, box9) & chain_ok(pu, None)
        idx = (4 * todo[:, None] + np.arange(4)[None, :])
        out_w[idx[ok].ravel()] = pw.reshape(m, 4, 3)[ok].reshape(-1, 3)
        out_u[idx[ok].ravel()] = pu.reshape(m, 4, 3)[ok].reshape(-1, 3)
        todo = todo[~ok]
    return out_w, out_u


def chain_ok(pos, box9):
    """per chain: bonds >= 0.09 nm, bond angles within 60 .. 150 degrees, and (with a box) no raw displacement component within
    1e-3 nm of half a box edge -- all checked in f64 on the f32 positions"""
    n = len(pos) // 4
    t = 4 * np.arange(n)[:, None] + np.arange(4)[None, :]
    ok = np.ones(n, bool)
    for a, b in ((0, 1), (1, 2), (2, 3)):
        ok &= values64("distance", pos, t[:, [a, b]], box9) >= 0.09
        if box9 is not None:
            raw = pos[t[:, b]].astype(np.float64) - pos[t[:, a]].astype(np.float64)
            L = lattice(box9)
            for k in (2, 1, 0):                                        # the components as the brick reduction meets them
                ok &= np.abs(np.abs(raw[:, k] - np.rint(raw[:, k] / L[k, k]) * L[k, k]) - L[k, k] / 2) > 1e-3
                raw = raw - np.rint(raw[:, k] / L[k, k])[:, None] * L[k]
    for tr in ((0, 1, 2), (1, 2, 3)):
        ang = np.degrees(values64("angle", pos, t[:, list(tr)], box9))
        ok &= (ang >= 60) & (ang <= 150)
    return ok


def chain_tuples(kind, n):
    """the tuples of `kind` of n chains: 3 distances / axis bonds, 2 angles, 1 dihedral per chain"""
    base = 4 * np.arange(n, dtype=np.uint64)[:, None]
    rel = {"distance": [(0, 1), (1, 2), (2, 3)], "axis": [(0, 1), (1, 2), (2, 3)], "angle": [(0, 1, 2), (1, 2, 3)], "dihedral": [(0, 1, 2, 3)]}[kind]
    return np.concatenate([base + np.array(r, np.uint64)[None, :] for r in rel]).astype(np.uint64)


DODECAHEDRON = np.array([6.26832, 6.26832, 4.43237, 0, 0, 0, 0, 3.13416, 3.13416], F)


def frame_boxes(box9, nf):
    """nf boxes that differ: the cell grows by 0.7 % a frame"""
    return [(np.asarray(box9, np.float64) * (1 + 0.007 * f)).astype(F) for f in range(nf)]
