"""The ORDER of the band product's sums (groan_rs_amd/csrc/gr_band.h), restated in numpy for panels of ONE column -- one atom of MSD, one
vector of VectorCorrelation.  A row then holds one value per component, n_pad = 64 values apart, so the components fall into different
trips of the product and every matrix instruction adds at most ONE product that is not zero to its accumulator: the order in which the
hardware adds the four products of an instruction does not matter, G(t, t') is the sequential f64 chain over the components
(`gram`, the products of two f32 are exact in f64), and the device's sums can be restated bit for bit:
  per 64 x 64 block of frame pairs (block column bi .. bi + W) and diagonal, the valid entries, rows ascending (entries that are not valid add +0.0)
  per lag tau = 64 d0 + r, block rows ascending, per block row diagonal r of block (bi, bi + d0), then diagonal r - 64 of block (bi, bi + d0 + 1)
With more than one column an instruction adds several products and only a bound holds (tests/test_gpu_msd.py, tests/test_gpu_vcorr.py)."""
import numpy as np

D = np.float64
BLOCK = 64


def gram(panel):
    """panel [T, C] f32, one column's components -> G [T, T] f64, every entry the chain ((0 + a_0 b_0) + a_1 b_1) + ..."""
    X = np.asarray(panel, np.float32).astype(D)
    G = np.zeros((len(X), len(X)), D)
    for c in range(X.shape[1]):
        G = G + X[:, c][:, None] * X[:, c][None, :]
    return G


def band_sums(value, ok, max_lag, strict):
    """value [T, T] f64: a block's value per frame pair; valid pairs: ok on both sides, t < t' (strict) or t <= t', t' - t <= max_lag
    -> sum [lags] f64 in the order of k_band_gram's diagonals and k_band_lags"""
    ok = np.asarray(ok, bool)
    T = len(ok)
    max_lag = min(max_lag, T - 1)
    nblk = -(-T // BLOCK)
    W = min(nblk - 1, -(-max_lag // BLOCK))
    part = {}
    for bi in range(nblk):
        for bj in range(bi, min(bi + W, nblk - 1) + 1):
            diags = np.zeros(2 * BLOCK - 1, D)
            for dl in range(2 * BLOCK - 1):
                s = D(0.0)
                for i in range(max(0, BLOCK - 1 - dl), min(BLOCK, 2 * BLOCK - 1 - dl)):
                    gi, gj = BLOCK * bi + i, BLOCK * bj + i + dl - (BLOCK - 1)
                    valid = gi < T and gj < T and ok[gi] and ok[gj] and (gi < gj if strict else gi <= gj) and gj - gi <= max_lag
                    s = s + (value[gi, gj] if valid else D(0.0))
                diags[dl] = s
            part[bi, bj] = diags
    sums = np.zeros(max_lag + 1, D)
    for tau in range(max_lag + 1):
        d0, r = divmod(tau, BLOCK)
        s = D(0.0)
        for bi in range(nblk):
            if d0 <= W and bi + d0 < nblk:
                s = s + part[bi, bi + d0][BLOCK - 1 + r]
            if r >= 1 and d0 + 1 <= W and bi + d0 + 1 < nblk:
                s = s + part[bi, bi + d0 + 1][r - 1]
        sums[tau] = s
    return sums
