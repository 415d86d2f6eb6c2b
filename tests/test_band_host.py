"""The band's HIP-free half (groan_rs_amd/csrc/gr_band.h: grband::block_index, block_decode, geometry, pair_counts) on the CPU: a small
C++ driver includes the header with the host compiler and prints its tables.  The kernels of MSD and VectorCorrelation decode a block
number with block_decode, k_band_lags looks the blocks of a lag up with block_index, and the host sizes the launch with geometry: here
the three are checked against each other, against the closed form, and against a brute-force enumeration of the frame pairs."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "groan_rs_amd", "csrc")
TS = (1, 63, 64, 65, 130)


def max_lags(T):
    return sorted({0, 1, 63, 64, T - 1, T + 5})

DRIVER = r"""
#include "gr_band.h"
#include <cinttypes>
#include <cstdio>
#include <iostream>
#include <sstream>
int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string op; in >> op;
        if (op == "blocks") {
            // blocks nblk W: every (bi, db) of the band in row order -> index, and the decode of that index
            uint32_t nblk, W; in >> nblk >> W;
            for (uint32_t bi = 0; bi < nblk; ++bi)
                for (uint32_t db = 0; db <= W && bi + db < nblk; ++db) {
                    const uint32_t t = grband::block_index(bi, db, nblk, W);
                    uint32_t bi2 = ~0u, db2 = ~0u;
                    grband::block_decode(t, nblk, W, bi2, db2);
                    printf("%u %u %u %u %u\n", bi, db, t, bi2, db2);
                }
        } else if (op == "geometry") {
            uint32_t T, max_lag; in >> T >> max_lag;
            const grband::Geometry g = grband::geometry(T, max_lag);
            printf("%u %u %u %u %" PRIu64 "\n", g.max_lag, g.lags, g.nblk, g.W, g.nblocks);
        } else if (op == "pairs") {
            // pairs lags ok...
            uint32_t lags; in >> lags;
            std::vector<uint8_t> ok; int v; while (in >> v) ok.push_back((uint8_t)v);
            std::vector<uint64_t> pairs(3, 77u);                      // (assigned, not appended to)
            grband::pair_counts(ok.data(), (uint32_t)ok.size(), lags, pairs);
            for (uint64_t p : pairs) printf("%" PRIu64 " ", p);
            printf("\n");
        }
        printf("end\n");
    }
    return 0;
}
"""


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    d = tmp_path_factory.mktemp("band")
    src, exe = d / "band_driver.cpp", d / "band_driver"
    src.write_text(DRIVER)
    r = subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-I" + CSRC, "-o", str(exe), str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert "warning" not in r.stderr, r.stderr

    def run(cmds):
        """one process for a list of commands -> the output lines of each"""
        out = subprocess.run([str(exe)], input="\n".join(cmds) + "\n", capture_output=True, text=True, check=True).stdout.splitlines()
        res, cur = [], []
        for l in out:
            if l == "end":
                res.append(cur); cur = []
            else:
                cur.append(l)
        assert len(res) == len(cmds) and not cur
        return res
    return run


def test_block_index_and_decode_are_inverses_dense_and_counted_by_the_closed_form(driver):
    cases = [(nblk, W) for nblk in range(1, 13) for W in range(nblk)]
    for (nblk, W), lines in zip(cases, driver(["blocks %d %d" % c for c in cases])):
        rows = np.array([[int(x) for x in l.split()] for l in lines])
        bi, db, t, bi2, db2 = rows.T
        assert (bi2 == bi).all() and (db2 == db).all(), (nblk, W)                  # decode(index(bi, db)) is the identity
        nblocks = (nblk - W) * (W + 1) + W * (W + 1) // 2
        assert len(t) == nblocks and t.tolist() == list(range(nblocks)), (nblk, W)  # dense in [0, nblocks), numbered row by row
        # row bi holds the columns bi .. min(bi + W, nblk - 1), each once
        assert sorted(zip(bi.tolist(), db.tolist())) == [(i, d) for i in range(nblk) for d in range(min(W, nblk - 1 - i) + 1)]


def test_geometry_covers_the_band_and_the_pair_counts_are_numpy_s(driver):
    cases = [(T, L) for T in TS for L in max_lags(T)]
    rng = np.random.default_rng(20261021)
    oks = {T: (rng.random(T) < 0.8).astype(np.uint8) for T in TS}
    oks[130][[0, 64, 129]] = 0
    geo = driver(["geometry %d %d" % c for c in cases])
    cnt = driver(["pairs %d %s" % (min(L, T - 1) + 1, " ".join(str(v) for v in oks[T])) for T, L in cases])
    assert any((ok == 0).any() for ok in oks.values())
    for (T, L), g, p in zip(cases, geo, cnt):
        max_lag, lags, nblk, W, nblocks = (int(x) for x in g[0].split())
        assert max_lag == min(L, T - 1) and lags == max_lag + 1, (T, L)            # CLAMPED
        assert nblk == -(-T // 64) and 0 <= W < nblk, (T, L)
        assert nblocks == (nblk - W) * (W + 1) + W * (W + 1) // 2, (T, L)
        # every pair t <= t' with t' - t <= max_lag lies in an enumerated block: its block column is at most W beyond its block row
        t = np.arange(T)
        far = np.minimum(t + L, T - 1)
        assert ((far // 64 - t // 64) <= W).all(), (T, L)
        # ... and W is no wider than the band needs (or than the matrix is)
        assert W == min(nblk - 1, -(-max_lag // 64)), (T, L)
        ok = oks[T]
        want = [int((ok[:T - tau] & ok[tau:]).sum()) for tau in range(lags)]
        assert [int(x) for x in p[0].split()] == want, (T, L)


def test_the_restated_order_of_the_band_s_sums_adds_every_valid_pair_once():
    """tests/band_ref.py (the GPU tests of one-column panels compare bits with it) against the plain sum per lag: the two differ by the
    order of at most T additions of values in [0, 1): T * 2^-53 * T"""
    import band_ref as B
    rng = np.random.default_rng(7)
    for T in (1, 64, 65, 130):
        value = rng.random((T, T))
        ok = rng.random(T) < 0.8
        for max_lag in (0, 3, 64, T + 5):
            for strict in (False, True):
                got = B.band_sums(value, ok, max_lag, strict)
                L = min(max_lag, T - 1) + 1
                want = np.array([value[np.arange(T - tau), np.arange(tau, T)][ok[:T - tau] & ok[tau:]].sum() if (tau or not strict) else 0.0 for tau in range(L)])
                assert got.shape == (L,) and np.abs(got - want).max() <= T * T * 2.0 ** -53, (T, max_lag, strict)
    x = rng.standard_normal((5, 3)).astype(np.float32)
    assert np.array_equal(B.gram(x)[1, 3], (np.float64(x[1, 0]) * x[3, 0] + np.float64(x[1, 1]) * x[3, 1]) + np.float64(x[1, 2]) * x[3, 2])
