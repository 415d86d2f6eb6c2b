"""numpy restatement of the library's VectorCorrelation (gr_vcorr_*; groan_rs_amd.VectorCorrelation), shared by the host and the GPU tests.

THE PANEL RULE (`vectors32`, `rank2`), f32, operation by operation -- the device's panels are compared with it bit for bit:
  d = x_j - x_i                                      one f32 subtraction per component
  len = sqrt((d_x d_x + d_y d_y) + d_z d_z)          every product and sum rounded on its own, the square root correctly rounded
  inv = float32(1) / len;  u_c = d_c * inv           u = 0 where len = 0 (such a vector adds nothing to a sum, but counts in the mean)
  rank 2: u_x u_x, u_y u_y, u_z u_z, S (u_x u_y), S (u_x u_z), S (u_y u_z)   with S = float32(sqrt 2), the product first, then times S
With a minimum image the f32 rule is the library's gr_min_image_vec; here only its f64 value is restated (`vectors64`, an exhaustive
image search, tests/internals_ref.py): a vector that does not straddle the cell is left untouched by the minimum image, bit for bit,
and one that does is held to a derived bound (tests/test_gpu_vcorr.py).

THE PER-VECTOR CHAINS (`chains`): for every vector and lag ONE sequential f64 sum s = s + a * b, frames ascending, within a frame the
components in panel order; the product of two f32 values is exact in f64, so this is the device's fma((double)a, (double)b, s).

THE DIRECT SUM (`direct`): S[tau] = sum over the valid pairs (t, t + tau) and the vectors of X_t . X_(t + tau) in long double, with the
sum of the |products|, the scale of the device's rounding bound.

THE RIGID ROTOR (`rotor`): V vectors of length b tilted by theta from z that turn by omega per frame about z, each with its own phase
and its own anchor:  C1 = cos^2 theta + sin^2 theta cos(omega tau),
C2 = P2(cos theta)^2 + 3/4 sin^2(2 theta) cos(omega tau) + 3/4 sin^4 theta cos(2 omega tau)."""
import numpy as np

import internals_ref as IR
import msd_ref as MR

F, D, LD = np.float32, np.float64, np.longdouble
OK, E_NO_BOX, E_NO_POSITION, E_OUT_OF_RANGE, E_INVALID_ARG = 0, 1, 6, 9, 10
SQRT2_F = F(np.sqrt(2.0))
EPS32 = 2.0 ** -24
same_bits = MR.same_bits


# ------------------------------------------------------------------------------------------------ the panel rule
def vectors32(pos, pairs, unit=True):
    """u [V, 3] f32 of the pairs [V, 2] from the positions pos [N, 3]: the device's rule without a minimum image"""
    p = np.asarray(pos, F)
    t = np.asarray(pairs, np.int64)
    d = p[t[:, 1]] - p[t[:, 0]]
    assert d.dtype == F
    if not unit:
        return d
    xx, yy, zz = d[:, 0] * d[:, 0], d[:, 1] * d[:, 1], d[:, 2] * d[:, 2]
    ln = np.sqrt((xx + yy) + zz)
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = F(1.0) / ln
        u = d * inv[:, None]
    assert ln.dtype == F and u.dtype == F
    return np.where(ln[:, None] > 0, u, F(0.0)).astype(F)


def rank2(u):
    """[..., 6] f32: the rank-2 entries of u [..., 3] in panel order"""
    u = np.asarray(u, F)
    x, y, z = u[..., 0], u[..., 1], u[..., 2]
    out = np.stack([x * x, y * y, z * z, SQRT2_F * (x * y), SQRT2_F * (x * z), SQRT2_F * (y * z)], -1)
    assert out.dtype == F
    return out


def vectors64(pos, pairs, box9=None, unit=True):
    """the f64 value of the vectors of f32 positions; box9: the minimum image by exhaustive search"""
    p = np.asarray(pos, F).astype(D)
    t = np.asarray(pairs, np.int64)
    d = p[t[:, 1]] - p[t[:, 0]]
    if box9 is not None:
        d = IR.min_image(d, box9)
    if not unit:
        return d
    ln = np.sqrt((d * d).sum(1))
    return np.where(ln[:, None] > 0, d / np.where(ln > 0, ln, 1.0)[:, None], 0.0)


class Panels:
    """the object's panels: rows [T][V, 3] f32 (and their rank-2 entries), ok [T]"""

    def __init__(self, pairs, unit=True, pbc=False):
        self.pairs, self.unit, self.pbc = np.asarray(pairs, np.int64).reshape(-1, 2), unit, pbc
        self.V = len(self.pairs)
        self.named = np.unique(self.pairs)
        self.rows, self.ok = [], []

    def append(self, frames, boxes=None):
        """-> (status [len(frames)], the lowest named atom without position per frame or -1); boxes[f] None: the frame has no box.
        With pbc the rows are NOT the device's bits (see the module's text): only status and ok are used then"""
        st, bad = np.zeros(len(frames), np.int32), np.full(len(frames), -1, np.int64)
        for f, x in enumerate(frames):
            p = np.asarray(x, F)
            nan = np.isnan(p[self.named, 0])
            if self.pbc and (boxes is None or boxes[f] is None):     # the host check comes first (the library's first-error order per frame)
                st[f] = E_NO_BOX
            elif nan.any():
                st[f], bad[f] = E_NO_POSITION, int(self.named[nan].min())
            if st[f]:
                self.rows.append(np.zeros((self.V, 3), F)); self.ok.append(False)
                continue
            self.rows.append(vectors32(p, self.pairs, self.unit)); self.ok.append(True)
        return st, bad

    def x1(self):
        return np.stack(self.rows) if self.rows else np.zeros((0, self.V, 3), F)

    def x2(self):
        return rank2(self.x1())


# ------------------------------------------------------------------------------------------------ pair counts and closings
def pair_counts(ok, max_lag=None):
    ok = np.asarray(ok, bool)
    T = len(ok)
    L = T if max_lag is None else min(max_lag, T - 1) + 1
    return np.array([int((ok[:T - tau] & ok[tau:]).sum()) for tau in range(L)], np.uint64)


def close(s, den, rank):
    """the host's closing in f64: s / den, or (1.5 s) / den - 0.5; NaN where den is 0.  s [..., L], den [L]"""
    s, den = np.asarray(s, D), np.asarray(den, D)
    with np.errstate(divide="ignore", invalid="ignore"):
        c = s / den if rank == 1 else (1.5 * s) / den - 0.5
    return np.where(den > 0, c, np.nan)


# ------------------------------------------------------------------------------------------------ the per-vector chains
def chains(panel, ok, max_lag=None):
    """s [V, L] f64 from panel [T, V, C] f32: per (vector, lag) one sequential sum s = s + a * b, frames ascending, components inside"""
    X = np.asarray(panel, F).astype(D)
    T, V, C = X.shape
    ok = np.asarray(ok, bool)
    L = T if max_lag is None else min(max_lag, T - 1) + 1
    s = np.zeros((V, L), D)
    for t in range(T):
        if not ok[t]:
            continue
        n = min(L, T - t)                                            # lags 0 .. n - 1 have a partner t + tau
        cols = np.nonzero(ok[t:t + n])[0]
        for c in range(C):
            s[:, cols] = s[:, cols] + X[t, :, c][:, None] * X[t + cols, :, c].T
    return s


def each(panel, ok, rank, max_lag=None):
    """the curves of every vector [V, L] as gr_vcorr_compute_each closes them"""
    s = chains(panel, ok, max_lag)
    return close(s, pair_counts(ok, max_lag), rank)


# ------------------------------------------------------------------------------------------------ the direct sum over all vectors
def direct(panel, ok, max_lag=None, dtype=LD):
    """-> (S [L], A [L]) in `dtype`: the sum over a lag's valid pairs and the vectors of X_t . X_(t + tau), and of the |products|"""
    X = np.asarray(panel, F)
    T = X.shape[0]
    X = X.reshape(T, -1).astype(dtype)
    ok = np.asarray(ok, bool)
    L = T if max_lag is None else min(max_lag, T - 1) + 1
    S, A = np.zeros(L, dtype), np.zeros(L, dtype)
    for tau in range(L):
        both = ok[:T - tau] & ok[tau:]
        if both.any():
            pr = X[:T - tau][both] * X[tau:][both]
            S[tau], A[tau] = pr.sum(), np.abs(pr).sum()
    return S, A


def sum_bound(A, pairs, K):
    """the bound on |S_device - S| per lag (tests/test_gpu_vcorr.py derives it): (K + 1 + pairs) 2^-53 A"""
    return (K + 1.0 + np.asarray(pairs, D)) * 2.0 ** -53 * np.asarray(A, D)


# ------------------------------------------------------------------------------------------------ inputs
def rotor(V, T, theta, omega, seed, bond=0.1, span=3.0):
    """-> (frames [T][2 V, 3] f32, pairs [V, 2]): atom 2 k is the anchor of vector k (fixed, inside [0, span)^3), atom 2 k + 1 lies
    `bond` away along (sin theta cos(omega t + phi_k), sin theta sin(omega t + phi_k), cos theta)"""
    rng = np.random.default_rng(seed)
    anchor = rng.random((V, 3)) * span
    phi = rng.random(V) * 2 * np.pi
    frames = []
    for t in range(T):
        a = omega * t + phi
        u = np.stack([np.sin(theta) * np.cos(a), np.sin(theta) * np.sin(a), np.full(V, np.cos(theta))], 1)
        x = np.empty((2 * V, 3), D)
        x[0::2], x[1::2] = anchor, anchor + bond * u
        frames.append(x.astype(F))
    return frames, np.stack([np.arange(0, 2 * V, 2), np.arange(1, 2 * V, 2)], 1)


def rotor_curves(theta, omega, L):
    tau = np.arange(L)
    c1 = np.cos(theta) ** 2 + np.sin(theta) ** 2 * np.cos(omega * tau)
    p2 = 0.5 * (3 * np.cos(theta) ** 2 - 1)
    c2 = p2 ** 2 + 0.75 * np.sin(2 * theta) ** 2 * np.cos(omega * tau) + 0.75 * np.sin(theta) ** 4 * np.cos(2 * omega * tau)
    return c1, c2


def unit_error(coord_max, bond, steps=1.0, size=None, stored=True):
    """eps: the bound on |u_device - u_exact| (norm, and so per component) of a unit vector formed by the panel rule.
    stored: the exact vector is that of the f64 coordinates the f32 ones were rounded from -- each stored coordinate is within
    ulp32(coord_max) / 2 of its exact one, so a component of the difference is within ulp32(coord_max); otherwise the exact vector
    is that of the stored coordinates themselves and this term is absent.  The f32 subtraction -- and with a minimum image each of up
    to four more single-rounded steps (three fused reductions, one candidate shift), `steps` counts them all -- adds
    steps * ulp32(size) / 2, size the magnitude at which they round: the bond for a pair inside the cell, the raw difference (at most
    twice the largest coordinate) for a pair that straddles it.  |delta d| <= sqrt(3) of the sum; normalising a vector that is
    delta d off moves the unit vector by at most 2 |delta d| / |d|; the rule's own roundings (three products and two sums under a
    square root: 1.25 ulp in len; the reciprocal and the product half an ulp each) are below 4 * 2^-24."""
    size = bond if size is None else size
    dd = np.sqrt(3.0) * ((float(IR.ulp32(coord_max)) if stored else 0.0) + steps * float(IR.ulp32(size)) / 2.0)
    return 2.0 * dd / bond + 4.0 * EPS32


def curve_bounds(eps):
    """-> (bound on |C1 - exact|, on |C2 - exact|) for unit vectors within eps of the exact ones: |delta (u . u')| <= 2 eps + eps^2 =: e;
    C2 = 1.5 x^2 - 0.5 with |x| <= 1 + e: 1.5 (2 + e) e; the rank-2 entries are f32 (a product, times S: 2^-24 each on both sides, and
    S^2 is within 2^-24 of 2): 5 * 2^-24 of sum |e_ab e'_ab| <= 1 + e, times 1.5 -- stated as 8 * 2^-24.  The f64 sums are far below."""
    e = 2.0 * eps + eps * eps
    return e + 1e-13, 1.5 * (2.0 + e) * e + 8.0 * EPS32 + 1e-13


def bonded_world(n_pairs, n_frames, seed, cell, bond=0.1, turn=0.15):
    """-> (frames [T][2 n_pairs, 3] f32 wrapped into the cell, boxes [T][9] f32, pairs [n_pairs, 2], straddle [T, n_pairs] bool).  The
    even atoms are msd_ref.walk's random walk; atom 2 k + 1 sits `bond` from atom 2 k in a direction that diffuses on the sphere (a
    Gaussian kick of `turn` per frame, renormalised), wrapped into the cell on its own: straddle says where the raw difference of the
    stored pair is not the bond (a whole box vector lies between the two)."""
    heavy, boxes, U, crossings = MR.walk(n_pairs, n_frames, seed, cell)
    rng = np.random.default_rng(seed + 7)
    u = rng.standard_normal((n_pairs, 3))
    u /= np.sqrt((u * u).sum(1))[:, None]
    frames, straddle = [], []
    for t in range(n_frames):
        if t:
            u = u + turn * rng.standard_normal((n_pairs, 3))
            u /= np.sqrt((u * u).sum(1))[:, None]
        partner, _ = MR._wrap(heavy[t].astype(D) + bond * u, boxes[t].astype(D))
        x = np.empty((2 * n_pairs, 3), F)
        x[0::2], x[1::2] = heavy[t], partner.astype(F)
        frames.append(x)
        raw = x[1::2].astype(D) - x[0::2].astype(D)
        straddle.append(np.sqrt((raw * raw).sum(1)) > 2 * bond)
    return frames, boxes, np.stack([np.arange(0, 2 * n_pairs, 2), np.arange(1, 2 * n_pairs, 2)], 1), np.stack(straddle)
