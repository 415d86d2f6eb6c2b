"""numpy restatement of the library's Covariance (gr_covar_*; groan_rs_amd.Covariance), shared by the host and the GPU tests.

The raw state is the walk below -- origin = the first counted frame (f32), d = x - origin as ONE f32 subtraction, then widened, s += d
and Q += d d^T in f64.  Every product d_i d_j is exact in f64, so the device's Q differs from this one by the ORDER of its f64 additions
only (the matrix instruction adds four frames at a time): q_bound() / s_bound() are the bound of any summation order of n terms,
(n - 1) u sum |terms| to first order with u = 2^-53, taken twice over (the restatement's own sum carries the same error).
two_pass() is the independent reference of the CLOSED results: the covariance straight from the f64 positions, no origin, no running sums."""
import numpy as np

from fluct_ref import E_INCONSISTENT_GROUP, E_INVALID_ARG, E_NO_POSITION, OK, fitted_frames, jumping_frames, same_bits  # noqa: F401 (re-exported)

F, D = np.float32, np.float64
U = 2.0 ** -53


class State:
    """dimension 3 k + c of the group's k-th atom"""

    def __init__(self, n_atoms):
        d = 3 * n_atoms
        self.o, self.s, self.Q, self.n = np.zeros(d, F), np.zeros(d, D), np.zeros((d, d), D), 0
        self.abs_s, self.abs_Q = np.zeros(d, D), np.zeros((d, d), D)           # sum |d|, sum |d_i d_j|: what the rounding bounds are made of

    def accumulate(self, frames, idx):
        """-> (status [len(frames)], index of the first atom without position per frame or -1); a failed frame is counted for no dimension"""
        st, bad = np.zeros(len(frames), np.int32), np.full(len(frames), -1, np.int64)
        rows = []
        for f, x in enumerate(frames):
            p = np.asarray(x, F)[idx]
            nan = np.isnan(p[:, 0])
            if nan.any():
                st[f], bad[f] = E_NO_POSITION, int(np.asarray(idx)[nan].min())
                continue
            p = p.reshape(-1)
            if self.n == 0:
                self.o = p.copy()
            rows.append((p - self.o).astype(D))     # the f32 subtraction, then widened
            self.n += 1
        if rows:
            X = np.stack(rows)
            self.s += X.sum(0)
            self.Q += X.T @ X
            self.abs_s += np.abs(X).sum(0)
            self.abs_Q += np.abs(X).T @ np.abs(X)
        return st, bad

    def q_bound(self):
        return 2.0 * self.n * U * self.abs_Q

    def s_bound(self):
        return 2.0 * self.n * U * self.abs_s

    def merge(self, src):
        """src's frames added to this state: its sums moved to this origin in f64"""
        if src.n == 0:
            return
        if self.n == 0:
            self.o, self.s, self.Q, self.n = src.o.copy(), src.s.copy(), src.Q.copy(), src.n
            self.abs_s, self.abs_Q = src.abs_s.copy(), src.abs_Q.copy()
            return
        delta = src.o.astype(D) - self.o.astype(D)
        ns = D(src.n)
        self.s += src.s + ns * delta
        self.Q += src.Q + np.outer(delta, src.s) + np.outer(src.s, delta) + ns * np.outer(delta, delta)
        ad = np.abs(delta)                          # |d + delta| <= |d| + |delta|
        self.abs_Q += src.abs_Q + np.outer(ad, src.abs_s) + np.outer(src.abs_s, ad) + ns * np.outer(ad, ad)
        self.abs_s += src.abs_s + ns * ad
        self.n += src.n


def close(o, s, Q, n, masses=None):
    """-> mean [S, 3], cov [3S, 3S], f64, in the library's operation order (NaN before the first counted frame)"""
    if n == 0:
        return np.full((len(s) // 3, 3), np.nan), np.full(Q.shape, np.nan)
    dn = D(n)
    mean = np.asarray(o, F).reshape(-1).astype(D) + np.asarray(s, D).reshape(-1) / dn
    s = np.asarray(s, D).reshape(-1)
    cov = (Q - np.outer(s, s) / dn) / dn
    if masses is not None:
        rm = np.sqrt(np.repeat(np.asarray(masses, F).astype(D), 3))
        cov = cov * np.outer(rm, rm)
    return mean.reshape(-1, 3), cov


def dccm(cov):
    """corr[a][b] = sum_c cov[3a+c][3b+c] / sqrt(tr_a tr_b); an atom with tr = 0: 1 on the diagonal, NaN elsewhere in its row and column"""
    S = len(cov) // 3
    if np.isnan(cov).all():
        return np.full((S, S), np.nan)
    c4 = cov.reshape(S, 3, S, 3)
    x = c4[:, 0, :, 0] + c4[:, 1, :, 1] + c4[:, 2, :, 2]
    tr = np.diagonal(x).copy()
    still = ~(tr > 0.0)
    with np.errstate(invalid="ignore", divide="ignore"):
        corr = x / np.sqrt(np.outer(tr, tr))
    corr[still, :] = np.nan; corr[:, still] = np.nan
    corr[still, still] = 1.0
    return corr


def two_pass(frames, idx):
    """mean [S, 3], cov [3S, 3S], sd [3S] of the frames that have every atom of idx, in two passes over the f64 positions"""
    X = np.stack([np.asarray(x, F)[idx].astype(D).reshape(-1) for x in frames if not np.isnan(np.asarray(x)[idx, 0]).any()])
    mean = X.sum(0) / len(X)
    Y = X - mean
    cov = Y.T @ Y / len(X)
    return mean.reshape(-1, 3), cov, np.sqrt(np.diagonal(cov))
