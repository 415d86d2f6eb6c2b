"""The closing arithmetic of the gyration calls (groan_rs_amd/csrc/gr_gyration.h, host part) on the CPU, and the host mirrors.

A small C++ driver includes the header directly (its first part compiles without HIP) and answers line commands:
  close n s0 .. s9      gr_gyr_close of the ten sums (W, w d, w d d: xx yy zz xy xz yz) -> rg, S[6]
  order w[3] V[9]       gr_gyr_order of eigenvalues and eigenvector COLUMNS (V row-major) -> lam[3], rows[9]
  axes S[6]             gr_gyr_axes -> lam[3], rows[9]
The driver is built twice, plainly and with -fsanitize=address,undefined, and every test runs against both.

Closed forms: one atom (all zeros, the identity); two atoms of masses 1 and 3 at distance r along (1, 1, 0) / sqrt 2 (lambda_1 = 3 r^2 / 16,
the others 0, v_1 along the bond with positive components); a planar ring of 12 atoms (lambda_3 = 0, v_3 = +- the normal); the clamp of
a diagonal entry that rounding left below zero; equal eigenvalues keep the solver's order; equal largest components: the first decides.
All of it is f64 arithmetic on a handful of terms: the tolerances are 1e-12 relative, thousands of roundings wide."""
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "groan_rs_amd", "csrc")

DRIVER = r"""
#include "gr_gyration.h"
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
static void show(const double *lam, const double R[3][3]) {
    printf("%.17g %.17g %.17g", lam[0], lam[1], lam[2]);
    for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) printf(" %.17g", R[i][j]);
    printf("\n");
}
int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string op; in >> op;
        if (op == "close") {
            unsigned n; double s[GR_GYR_SUMS], rg, S[6];
            in >> n; for (double &v : s) in >> v;
            gr_gyr_close(s, n, &rg, S);
            printf("%.17g %.17g %.17g %.17g %.17g %.17g %.17g\n", rg, S[0], S[1], S[2], S[3], S[4], S[5]);
        } else if (op == "order") {
            double w[3], V[3][3], lam[3], R[3][3];
            for (double &v : w) in >> v;
            for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) in >> V[i][j];
            gr_gyr_order(w, V, lam, R);
            show(lam, R);
        } else if (op == "axes") {
            double S[6], lam[3], R[3][3];
            for (double &v : S) in >> v;
            gr_gyr_axes(S, lam, R);
            show(lam, R);
        } else printf("?\n");
    }
    return 0;
}
"""


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def driver(request, tmp_path_factory):
    d = tmp_path_factory.mktemp("gyration_" + request.param)
    src, exe = d / "gyr_driver.cpp", d / "gyr_driver"
    src.write_text(DRIVER)
    flags = ["-O2"] if request.param == "plain" else ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I" + CSRC, "-o", str(exe), str(src)] + flags, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr

    def run(cmd):
        p = subprocess.run([str(exe)], input=cmd + "\n", capture_output=True, text=True)
        assert p.returncode == 0 and not p.stderr, p.stderr
        return np.array([float(v) for v in p.stdout.split()])
    return run


def _sums(pos, w, origin):
    d = np.asarray(pos, np.float64) - np.asarray(origin, np.float64)
    w = np.asarray(w, np.float64)
    q = [(w * d[:, a] * d[:, b]).sum() for a, b in ((0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2))]
    return [w.sum()] + [(w * d[:, a]).sum() for a in range(3)] + q


def _close(driver, pos, w, origin):
    out = driver("close %d %s" % (len(pos), " ".join(repr(float(v)) for v in _sums(pos, w, origin))))
    return out[0], out[1:7]


def _axes(driver, S):
    out = driver("axes " + " ".join(repr(float(v)) for v in S))
    return out[0:3], out[3:12].reshape(3, 3)


def test_one_atom(driver):
    rg, S = _close(driver, [[1.25, -3.5, 0.75]], [12.011], [1.2500001, -3.4999998, 0.75])
    assert rg == 0.0 and (S == 0.0).all()
    lam, R = _axes(driver, S)
    assert (lam == 0.0).all() and np.array_equal(R, np.eye(3))


def test_two_atoms(driver):
    r = 0.37
    u = np.array([1.0, 1.0, 0.0]) / np.sqrt(2.0)
    a = np.array([2.0, -1.0, 0.5])
    pos, w = [a, a + r * u], [1.0, 3.0]
    want = 3.0 * r * r / 16.0
    for origin in ([0.0, 0.0, 0.0], a, [2.1, -0.8, 0.4]):            # the origin of the sums drops out
        rg, S = _close(driver, pos, w, origin)
        assert abs(rg * rg - want) <= 1e-12 * max(1.0, float(np.dot(a, a)))
        lam, R = _axes(driver, S)
        assert abs(lam[0] - want) <= 1e-12 and abs(lam[1]) <= 1e-12 and abs(lam[2]) <= 1e-12 and lam[0] >= lam[1] >= lam[2]
        assert np.abs(R[0] - u).max() <= 1e-6 and R[0][0] > 0 and R[0][1] > 0
        assert np.abs(R @ R.T - np.eye(3)).max() <= 1e-12 and np.linalg.det(R) > 0.999999


def test_planar_ring(driver):
    normal = np.array([1.0, -2.0, 2.0]) / 3.0
    e1 = np.cross(normal, [0.0, 0.0, 1.0]); e1 /= np.linalg.norm(e1)
    e2 = np.cross(normal, e1)
    t = 2.0 * np.pi * np.arange(12) / 12.0
    pos = np.array([4.0, 4.0, 4.0]) + 0.5 * (np.cos(t)[:, None] * e1 + 0.6 * np.sin(t)[:, None] * e2)
    rg, S = _close(driver, pos, np.ones(12), [3.9, 4.2, 4.0])
    lam, R = _axes(driver, S)
    assert abs(lam[0] - 0.125) <= 1e-12 and abs(lam[1] - 0.125 * 0.36) <= 1e-12 and abs(lam[2]) <= 1e-12
    assert abs(abs(float(R[2] @ normal)) - 1.0) <= 1e-9 and abs(abs(float(R[0] @ e1)) - 1.0) <= 1e-9
    assert abs(rg * rg - lam.sum()) <= 1e-12
    for k in (0, 1):                                                  # the sign convention
        assert R[k][np.argmax(np.abs(R[k]))] > 0
    assert np.abs(np.cross(R[0], R[1]) - R[2]).max() <= 1e-15


def test_negative_diagonal_is_stored_as_zero(driver):
    # sum w d_x^2 / W an ulp below m_x^2: S_xx = -1.1e-16 before the clamp; the off-diagonals are left alone
    s = [1.0, 1.0, 0.5, 0.0, float(np.nextafter(1.0, 0.0)), 0.5, 0.25, 0.25, 0.0, 0.0]
    out = driver("close 3 " + " ".join(repr(v) for v in s))
    assert out[1] == 0.0 and out[2] == 0.25 and out[3] == 0.25 and out[4] == -0.25 and out[0] == np.sqrt(0.5)
    # a NaN stays a NaN (no weight at all)
    assert np.isnan(driver("close 3 " + " ".join(["0.0"] * 10))).all()
    assert np.isnan(driver("close 1 " + " ".join(["0.0"] * 10))).all()


def test_order_and_ties(driver):
    s = float(np.sqrt(0.5))
    V = [[-s, -s, 0.0], [s, -s, 0.0], [0.0, 0.0, 1.0]]             # columns (-s, s, 0), (-s, -s, 0), (0, 0, 1)

    def order(w):
        out = driver("order %s %s" % (" ".join(repr(float(v)) for v in w), " ".join(repr(v) for row in V for v in row)))
        return out[0:3].tolist(), out[3:12].reshape(3, 3)
    # equal largest components: the FIRST decides -- (-s, s, 0) is flipped, (s, -s, 0) would not be
    lam, R = order([3.0, 2.0, 1.0])
    assert lam == [3.0, 2.0, 1.0] and R[0].tolist() == [s, -s, 0.0] and R[1].tolist() == [s, s, 0.0]
    assert np.abs(R[2] - [0.0, 0.0, 1.0]).max() <= 1e-15
    # ascending input is reversed; v3 is the cross product, not the solver's column
    lam, R = order([1.0, 2.0, 3.0])
    assert lam == [3.0, 2.0, 1.0] and R[0].tolist() == [0.0, 0.0, 1.0] and R[1].tolist() == [s, s, 0.0] and np.abs(R[2] - [-s, s, 0.0]).max() <= 1e-15
    # equal eigenvalues keep the solver's order
    lam, R = order([1.0, 2.0, 2.0])
    assert lam == [2.0, 2.0, 1.0] and R[0].tolist() == [s, s, 0.0] and R[1].tolist() == [0.0, 0.0, 1.0]
    lam, R = order([2.0, 2.0, 2.0])
    assert R[0].tolist() == [s, -s, 0.0] and R[1].tolist() == [s, s, 0.0]
    lam, R = order([2.0, 1.0, 2.0])
    assert lam == [2.0, 2.0, 1.0] and R[0].tolist() == [s, -s, 0.0] and R[1].tolist() == [0.0, 0.0, 1.0]


def test_axes_of_a_general_tensor(driver):
    rng = np.random.default_rng(20260701)
    for _ in range(8):
        Q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
        T = Q @ np.diag(np.array([1.0, 0.5, 0.2]) * rng.uniform(0.5, 2.0)) @ Q.T
        lam, R = _axes(driver, [T[0, 0], T[1, 1], T[2, 2], T[0, 1], T[0, 2], T[1, 2]])
        assert np.abs(lam - np.linalg.eigvalsh(T)[::-1]).max() <= 1e-12
        assert np.abs(R.T @ np.diag(lam) @ R - T).max() <= 1e-12 and np.linalg.det(R) > 0.999999


# ------------------------------------------------------------------ the mirrors
def test_cpp_mirror_compiles_without_a_warning():
    """tests/cpp/gyration_mirror.cpp calls every new method of groan::Segments"""
    src = os.path.join(ROOT, "tests", "cpp", "gyration_mirror.cpp")
    hpp = open(os.path.join(ROOT, "include", "groan_hip.hpp")).read()
    cls = hpp.split("class Segments {")[1].split("  private:")[0]
    text = open(src).read()
    for name in ("gyration", "gyration_device", "set_piece_frames"):
        assert re.search(r"\b%s\(" % name, cls) and re.search(r"\.%s\(" % name, text), name
    p = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"), src], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    assert cls.count("detail::batch_status") >= 3                     # a refused call throws, like centers


def test_shape_descriptors_by_hand():
    import groan_rs_amd as G
    b, c, k2 = G.shape_descriptors([[2.0, 2.0, 2.0], [3.0, 0.0, 0.0], [0.0, 0.0, 0.0], [4.0, 2.0, 1.0]])
    assert b.tolist() == [0.0, 3.0, 0.0, 2.5] and c.tolist() == [0.0, 0.0, 0.0, 1.0]
    assert k2[0] == 0.0 and k2[1] == 1.0 and k2[2] == 0.0 and abs(k2[3] - (1.5 * 21.0 / 49.0 - 0.5)) <= 1e-15
    assert b.dtype == np.float64 and G.shape_descriptors(np.zeros((2, 5, 3), np.float32))[2].shape == (2, 5)


def test_moments_of_inertia_by_hand():
    import groan_rs_amd as G

    class Two:                                                        # the partition alone: two segments over five atoms
        def __len__(self): return 2
        def atoms(self, s): return np.array([[0, 1], [2, 3, 4]][s], np.uint64)
    masses = [1.0, 3.0, 2.0, 2.0, 2.0]
    lam = np.array([[[0.5, 0.0, 0.0], [0.25, 0.25, 0.0]]])          # a rod of total mass 4, a disc of total mass 6
    I = G.Segments.moments_of_inertia(Two(), lam, masses)
    assert I.shape == (1, 2, 3) and I[0].tolist() == [[0.0, 2.0, 2.0], [1.5, 1.5, 3.0]]
    with pytest.raises(ValueError):
        G.Segments.moments_of_inertia(Two(), lam[:, :1], masses)


def test_python_declares_the_header_s_functions():
    import groan_rs_amd as G
    header = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "groan_hip.h")).read(), flags=re.S)
    for name in ("gr_segments_gyration_batch", "gr_segments_gyration_batch_device", "gr_segments_set_piece_frames"):
        m = re.search(r"\bint\s+%s\s*\(([^;]*?)\)\s*;" % name, header, flags=re.S)
        assert m, name
        res, args = G._lib.SIGNATURES[name]
        assert len(args) == len(m.group(1).split(",")), name
    assert G._lib.SEG_STAT_LAST_PIECES == int(re.search(r"GR_SEG_STAT_LAST_PIECES\s*=\s*(\d+)", header).group(1)) == 7
    for name in ("gyration", "gyration_device", "set_piece_frames", "from_group", "moments_of_inertia"):
        assert hasattr(G.Segments, name), name
    lib = G._lib.load()
    assert lib.gr_segments_gyration_batch(None, 0, 1, 2, 1, None, None, None) == G._lib.E_INVALID_ARG
    assert lib.gr_segments_gyration_batch_device(None, 0, 1, 2, 1, 0, None, None, None, None) == G._lib.E_INVALID_ARG
    assert lib.gr_segments_set_piece_frames(None, 1) == G._lib.E_INVALID_ARG
