"""The GridMap geometry (groan_rs_amd/csrc/gr_gridmap.h) on the CPU, against the reference's known answers.

A small C++ driver includes the header directly (its first part compiles without HIP) and answers line commands; the same
functions are reached through the library's context-free C ABI (gr_gridmap_len / _coord2index / _index2coord) and through the
Python helpers built on them (groan_rs_amd.gridmap).  Pinned here, as literals:
  new                 spans (-2, 7), (3, 6), tiles (0.15, 0.20) -> 61 x 16                 src/structures/gridmap.rs:778-788
  from_box            spans (0, 10), (0, 20), tiles (0.15, 0.20) -> 68 x 101               :849-860
  new_failures        InvalidSpan / InvalidGridTile                                          :791-846
  coord2index         the sixteen x2index / y2index values around both edges               :1173-1204
  is_inside, get_tile                                                                        :1399-1418
  write, write_column_major   the two output strings                                        :1373, :1393
and the numpy restatement tests/gridmap_ref.py == the driver on random coordinates, on every half-way point between two tiles with
its two f32 neighbours, on NaN / +-inf, and on the quantiser's edge values; the C++ mirror of the new calls compiles.
The launch geometry (grg::gm_launch) is held against its second statement gridmap_ref.launch, with and without gr_gridmap_set_launch's
overrides; a range of at most 2^18 units -- the bound that keeps the u32 LDS counts of 1024 frames below 2^32 -- is pinned only here."""
import io
import os
import subprocess

import numpy as np
import pytest

import gridmap_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "groan_rs_amd", "csrc")
F = np.float32
I64_MAX, I64_MIN = 2 ** 63 - 1, -2 ** 63

DRIVER = r"""
#include "gr_gridmap.h"
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>
static float bits(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }
static uint32_t ubits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }
int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string op; in >> op;
        if (op == "len") { uint32_t a, b, t; in >> a >> b >> t; uint64_t n = 0; int st = grg::gm_len(bits(a), bits(b), bits(t), &n); printf("%d %" PRIu64 "\n", st, st ? 0 : n); }
        else if (op == "idx") {   // span0 tile coord... -> index, inside(n)?, tile index
            uint32_t s, t, n, c; in >> s >> t >> n;
            while (in >> c) {
                uint32_t k = 0; const bool inside = grg::gm_tile(bits(c), bits(s), bits(t), n, k);
                printf("%" PRId64 " %d %u ", grg::gm_coord2index(bits(c), bits(s), bits(t)), inside ? 1 : 0, k);
            }
            printf("\n");
        }
        else if (op == "coord") { uint32_t s, t; uint64_t i; in >> s >> t; while (in >> i) printf("%u ", ubits(grg::gm_index2coord(i, bits(s), bits(t)))); printf("\n"); }
        else if (op == "quant") { uint32_t v; while (in >> v) { int64_t q = 0; const bool ok = grg::gm_quant(bits(v), q); printf("%d %" PRId64 " ", ok ? 1 : 0, q); } printf("\n"); }
        else if (op == "launch") {   // units n_cus lds_bytes nb range_groups frame_groups check_groups -> wx fy check_wgs per
            uint64_t units, lds; uint32_t cus, nb, rg, fg, cg; in >> units >> cus >> lds >> nb >> rg >> fg >> cg;
            const grg::GmLaunch L = grg::gm_launch(units, cus, lds, nb, rg, fg, cg);
            printf("%u %u %u %u\n", L.wx, L.fy, L.check_wgs, L.per);
        }
        else if (op == "mean") { int64_t s; uint64_t c; in >> s >> c; printf("%u\n", ubits(grg::gm_mean(s, c))); }
        else printf("?\n");
    }
    return 0;
}
"""


def _u(v):
    return int(np.asarray(v, F).reshape(1).view(np.uint32)[0])


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    d = tmp_path_factory.mktemp("gridmap")
    src, exe = d / "gm_driver.cpp", d / "gm_driver"
    src.write_text(DRIVER)
    r = subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Wno-unknown-pragmas", "-I" + CSRC, "-o", str(exe), str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr

    def run(*cmds):
        out = subprocess.run([str(exe)], input="\n".join(cmds) + "\n", capture_output=True, text=True, check=True).stdout
        return out.splitlines()
    return run


@pytest.fixture(scope="module")
def M():
    import groan_rs_amd as g
    g._lib.load()
    from groan_rs_amd import gridmap
    return gridmap


def _len_all(driver, M, span, tile):
    """(status, n) from the driver, the C ABI helper and the restatement: they must agree"""
    st, n = [int(v) for v in driver("len %d %d %d" % (_u(span[0]), _u(span[1]), _u(tile)))[0].split()]
    want = R.get_len(span, tile)
    assert (st == 0) == (want[0] == R.OK) and (st != 0 or n == want[1]), (span, tile, st, n, want)
    try:
        got = (R.OK, M.get_len(span, tile))
    except M.GridMapError as e:
        got = (e.status, 0)
    assert got == (want[0], want[1] if want[0] == R.OK else 0), (span, tile, got, want)
    return want


# ------------------------------------------------------------------ known answers of the reference
def test_new_and_from_box(driver, M):
    assert _len_all(driver, M, (-2.0, 7.0), 0.15) == (R.OK, 61) and _len_all(driver, M, (3.0, 6.0), 0.20) == (R.OK, 16)      # gridmap.rs:778-788
    assert _len_all(driver, M, (0.0, 10.0), 0.15) == (R.OK, 68) and _len_all(driver, M, (0.0, 20.0), 0.20) == (R.OK, 101)    # :849-860
    g = M.TileGeometry((-2.0, 7.0), (3.0, 6.0), (0.15, 0.20))
    assert (g.n_tiles_x, g.n_tiles_y, g.n_tiles) == (61, 16, 61 * 16)
    assert g.span_x == (F(-2.0), F(7.0)) and g.span_y == (F(3.0), F(6.0)) and g.tile_dim == (F(0.15), F(0.20))


def test_new_failures(driver, M):
    """gridmap.rs:791-846"""
    assert _len_all(driver, M, (2.0, -2.0), 0.15)[0] == R.E_INVALID_SPAN
    assert _len_all(driver, M, (3.0, -6.0), 0.20)[0] == R.E_INVALID_SPAN
    assert _len_all(driver, M, (-2.0, 7.0), 0.0)[0] == R.E_INVALID_TILE
    assert _len_all(driver, M, (3.0, 6.0), 0.0)[0] == R.E_INVALID_TILE
    assert _len_all(driver, M, (-2.0, 7.0), 10.5)[0] == R.E_INVALID_TILE
    assert _len_all(driver, M, (3.0, 6.0), 3.10)[0] == R.E_INVALID_TILE
    for args, variant in [(((2.0, -2.0), (3.0, 6.0), (0.15, 0.20)), "InvalidSpan"), (((-2.0, 7.0), (3.0, -6.0), (0.15, 0.20)), "InvalidSpan"),
                          (((-2.0, 7.0), (3.0, 6.0), (0.0, 0.20)), "InvalidGridTile"), (((-2.0, 7.0), (3.0, 6.0), (0.15, 0.0)), "InvalidGridTile"),
                          (((-2.0, 7.0), (3.0, 6.0), (10.5, 0.20)), "InvalidGridTile"), (((-2.0, 7.0), (3.0, 6.0), (0.15, 3.10)), "InvalidGridTile")]:
        with pytest.raises(M.GridMapError) as e:
            M.TileGeometry(*args)
        assert e.value.variant == variant
    # the library's own refusals
    nan = float("nan")
    for span, tile in [((nan, 1.0), 0.1), ((0.0, nan), 0.1), ((0.0, 1.0), nan), ((0.0, 1.0), -0.1)]:
        assert _len_all(driver, M, span, tile)[0] == R.E_INVALID_ARG
    assert _len_all(driver, M, (0.0, 1.0), 1.0) == (R.OK, 2) and _len_all(driver, M, (1.0, 1.0), 0.5)[0] == R.E_INVALID_TILE


COORD2INDEX = [("x", -2.0, 0), ("x", -2.07, 0), ("x", -2.08, -1), ("x", -2.32, -2), ("x", 7.0, 60), ("x", 7.07, 60), ("x", 7.08, 61), ("x", 7.32, 62),
               ("y", 3.0, 0), ("y", 2.91, 0), ("y", 2.89, -1), ("y", 2.58, -2), ("y", 6.0, 15), ("y", 6.09, 15), ("y", 6.11, 16), ("y", 6.42, 17)]


def test_coord2index(driver, M):
    """gridmap.rs:1173-1204 (the reference's usize values after the wrapping cast)"""
    for axis, c, want in COORD2INDEX:
        s0, t, n = (-2.0, 0.15, 61) if axis == "x" else (3.0, 0.20, 16)
        out = driver("idx %d %d %d %d" % (_u(s0), _u(t), n, _u(c)))[0].split()
        assert int(out[0]) == want, (axis, c, out)
        assert int(out[1]) == (1 if 0 <= want < n else 0) and (int(out[2]) == want if 0 <= want < n else True)
        assert M.coord2index(s0, t, c) == want
        assert int(R.coord2index([c], s0, t)[0]) == want


def test_is_inside_and_get_tile(M):
    """gridmap.rs:1399-1418"""
    g = M.TileGeometry((-2.0, 7.0), (3.0, 6.0), (0.15, 0.20))
    assert g.is_inside(-1.8, 4.5) and g.is_inside(-2.05, 3.09) and g.is_inside(7.05, 6.09)
    assert not g.is_inside(7.11, 4.5) and not g.is_inside(0.11, 2.8)
    assert g.get_tile(-1.8, 4.5) == (F(-1.85), F(4.6))
    assert g.get_tile(5.8, 4.2) == (F(5.8), F(4.2)) and g.get_tile(5.7843, 4.12374) == (F(5.8), F(4.2))
    assert g.get_tile(7.11, 4.5) is None and g.get_tile(0.11, 2.8) is None
    for t in g.get_tile(-1.8, 4.5):
        assert isinstance(t, np.float32)


def test_write_strings(M):
    """gridmap.rs:1359-1396: the converted values 10, 24, 9, 7, 87, 0 on a 3 x 2 map of span (0, 2), (0, 1), tile 1"""
    g = M.TileGeometry((0.0, 2.0), (0.0, 1.0), (1.0, 1.0))
    assert (g.n_tiles_x, g.n_tiles_y) == (3, 2)
    values = np.array([[10, 24], [9, 7], [87, 0]], np.uint64)
    out = io.StringIO(); g.write_map(out, values)
    assert out.getvalue() == "  0.000000   0.000000 10\n  0.000000   1.000000 24\n  1.000000   0.000000 9\n  1.000000   1.000000 7\n  2.000000   0.000000 87\n  2.000000   1.000000 0\n"
    out = io.StringIO(); g.write_map(out, values, column_major=True)
    assert out.getvalue() == "  0.000000   0.000000 10\n  1.000000   0.000000 9\n  2.000000   0.000000 87\n  0.000000   1.000000 24\n  1.000000   1.000000 7\n  2.000000   1.000000 0\n"
    assert [(float(x), float(y), int(v)) for x, y, v in g.extract(values, column_major=True)][:3] == [(0.0, 0.0, 10), (1.0, 0.0, 9), (2.0, 0.0, 87)]
    # floats print like Rust's Display for f32: shortest round-trip digits, positional, no trailing ".0"
    out = io.StringIO(); g.write_map(out, np.array([[1.0, np.nan], [0.1, 1e-7], [np.inf, 123456789.0]], np.float32))
    assert [ln.split()[2] for ln in out.getvalue().splitlines()] == ["1", "NaN", "0.1", "0.0000001", "inf", "123456790"]
    assert M.format_f32(F(-0.0)) == "-0" and M.format_f32(-np.inf) == "-inf" and M.format_f32(F(2.5)) == "2.5" and M.format_f32(F(16777216.0)) == "16777216"
    # column-major x coordinates come from index2x (the reference calls index2y there, which only agrees for equal spans and tiles)
    h = M.TileGeometry((1.0, 2.0), (1.0, 2.5), (1.0, 0.5))
    v = np.arange(8).reshape(2, 4)
    assert [(float(x), float(y), int(k)) for x, y, k in h.extract(v, column_major=True)][:3] == [(1.0, 1.0, 0), (2.0, 1.0, 4), (1.0, 1.5, 1)]


# ------------------------------------------------------------------ restatement == header == ABI
def _idx_driver(driver, s0, t, n, coords):
    out = []
    coords = np.asarray(coords, F)
    for a in range(0, len(coords), 500):
        vals = driver("idx %d %d %d " % (_u(s0), _u(t), n) + " ".join(str(_u(c)) for c in coords[a:a + 500]))[0].split()
        out += [(int(vals[3 * k]), int(vals[3 * k + 1]), int(vals[3 * k + 2])) for k in range(len(vals) // 3)]
    return out


@pytest.mark.parametrize("s0, t, n", [(-2.0, 0.15, 61), (3.0, 0.20, 16), (0.0, 0.02, 301), (0.0, 0.025, 257), (0.0, 1.0, 4)])
def test_restatement_equals_driver(driver, M, s0, t, n):
    rng = np.random.default_rng(20260501)
    s0f, tf = F(s0), F(t)
    k = np.arange(-3, n + 3, dtype=np.float64)
    half = np.array([F(s0f + F(F(kk + sg) * tf)) for kk in k for sg in (-0.5, 0.5)], F)      # span0 + (k +- 0.5) * tile
    edge = np.concatenate([half, np.nextafter(half, F(np.inf)), np.nextafter(half, F(-np.inf))])
    rand = (rng.random(3000) * (n + 6) * t + s0 - 3 * t).astype(F)
    special = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, 1e30, -1e30, 3.0e38, -3.0e38, 9.3e18 * t, -9.3e18 * t, 1e-45], F)
    coords = np.concatenate([edge, rand, special])
    got = _idx_driver(driver, s0, t, n, coords)
    want = R.coord2index(coords, s0, t)
    assert [g[0] for g in got] == want.tolist()
    inside = (want >= 0) & (want < n)
    assert [g[1] for g in got] == inside.astype(int).tolist()                      # the kernels' 32-bit form decides the same
    assert all(g[2] == w for g, w, i in zip(got, want.tolist(), inside) if i)
    for c in list(special) + list(edge[:40]):                                       # and the C ABI
        assert M.coord2index(s0, t, c) == int(R.coord2index([c], s0, t)[0])
    # NaN -> 0, saturation
    assert int(R.coord2index([np.nan], s0, t)[0]) == 0 and int(R.coord2index([np.inf], s0, t)[0]) == I64_MAX and int(R.coord2index([-np.inf], s0, t)[0]) == I64_MIN
    # index -> coordinate, bit for bit
    idx = list(range(0, n)) + [n, 10 ** 6, 2 ** 26, 2 ** 40 + 12345]
    out = [int(v) for v in driver("coord %d %d " % (_u(s0), _u(t)) + " ".join(str(i) for i in idx))[0].split()]
    assert out == [_u(v) for v in R.index2coord(np.array(idx, np.uint64), s0, t)]
    assert [_u(M.index2coord(s0, t, i)) for i in idx[:8] + idx[-4:]] == out[:8] + out[-4:]


def test_quantiser(driver):
    big = np.nextafter(F(2.0 ** 31), F(0))                                           # the largest accepted value
    vals = np.array([0.0, -0.0, 2.0 ** -21, -2.0 ** -21, 1.5 * 2.0 ** -20, -1.5 * 2.0 ** -20, 2.5 * 2.0 ** -20, 1.0, -3.75, big, -big, 2.0 ** 31, -2.0 ** 31,
                     np.nan, np.inf, -np.inf, 1e-45, 0.3], F)
    out = driver("quant " + " ".join(str(_u(v)) for v in vals))[0].split()
    got_ok, got_q = [int(v) for v in out[0::2]], [int(v) for v in out[1::2]]
    ok, q = R.quantise(vals)
    assert got_ok == ok.astype(int).tolist() and got_q == q.tolist()
    # by hand: ties go to even, the limits
    assert got_q[:9] == [0, 0, 0, 0, 2, -2, 2, 2 ** 20, -3932160]
    assert got_ok[9:17] == [1, 1, 0, 0, 0, 0, 0, 1] and got_q[9] == 2147483520 * 2 ** 20 and got_q[10] == -2147483520 * 2 ** 20
    assert got_q[17] == int(np.rint(np.float64(F(0.3)) * 2 ** 20))
    # the mean
    for s, c in [(0, 0), (5, 0), (3 * 2 ** 20, 2), (-7, 3), (2 ** 62, 2 ** 32), (1, 3)]:
        assert int(driver("mean %d %d" % (s, c))[0]) == _u(R.mean(np.array([c], np.uint64), np.array([s], np.int64))[0])
    assert np.isnan(R.mean(np.array([0], np.uint64), np.array([5], np.int64))[0])


# ------------------------------------------------------------------ the launch geometry
CUS, LDS_BYTES, NBS = (0, 1, 256, 304), (0, 12, 11712, 65532, 65536), (1, 12, 1024)


def _launch(driver, cases):
    out = driver(*["launch %d %d %d %d %d %d %d" % c for c in cases])
    assert len(out) == len(cases)
    return [tuple(int(v) for v in ln.split()) for ln in out]


def _target(n_cus, lds):
    return max(n_cus, 1) * (min(8, 163840 // lds) if lds else 8)


def test_launch_defaults(driver):
    """no override: the grids the library has always launched, stated a second time in gridmap_ref.launch"""
    cases = []
    for cus in CUS:
        for lds in LDS_BYTES:
            t = _target(cus, lds)
            for nb in NBS:
                for units in (1, 255, 256, 257, 2073, 250000, 2 ** 18 * t - 1, 2 ** 18 * t, 2 ** 18 * t + 1, 2 ** 30):
                    cases.append((units, cus, lds, nb, 0, 0, 0))
    got = _launch(driver, cases)
    for c, (wx, fy, check, per) in zip(cases, got):
        units, cus, lds, nb = c[:4]
        assert (wx, fy, check, per) == R.launch(units, cus, lds, nb), c
        assert wx >= 1 and 1 <= fy <= nb and wx * per >= units, (c, wx, fy, per)           # (trailing ranges may be empty: the kernel clamps u0, u1)
        assert per <= 2 ** 18, (c, per)                                            # the u32-count bound: 1024 frames x 4 atoms x 2^18 units = 2^30 per tile at most ...
        assert 1 <= check <= 4096 and check * 256 >= min(units, 4096 * 256)
    # ... and it binds: beyond 2^18 x target units the floor, not the target, decides the grid
    t = _target(256, 11712)
    assert _launch(driver, [(2 ** 18 * t, 256, 11712, 12, 0, 0, 0), (2 ** 18 * t + 1, 256, 11712, 12, 0, 0, 0)]) == [(t, 1, 4096, 2 ** 18), (t + 1, 1, 4096, -(-(2 ** 18 * t + 1) // (t + 1)))]
    # by hand: the shapes of tests/test_gpu_gridmap_edges.py on 256 CUs (2 workgroups of 65532 B per CU; 8 of 11712 B)
    assert _launch(driver, [(2073, 256, 65532, 64, 0, 0, 0), (2073, 256, 11712, 12, 0, 0, 0), (1186, 256, 0, 12, 0, 0, 0)]) == [(9, 56, 9, 231), (9, 12, 9, 231), (5, 12, 5, 238)]


def test_launch_overrides(driver):
    cases = []
    for cus in CUS:
        for lds in LDS_BYTES:
            for nb in NBS:
                for units in (1, 255, 2073, 2 ** 18 + 1, 2 ** 30):
                    for rg, fg, cg in [(1, 1, 1), (2, 3, 2), (3, 5, 0), (1, 12, 0), (2073, 1, 0), (0, 5, 0), (7, 0, 0), (0, 0, 3), (2 ** 32 - 1, 2 ** 32 - 1, 2 ** 32 - 1)]:
                        cases.append((units, cus, lds, nb, rg, fg, cg))
    got = _launch(driver, cases)
    for c, (wx, fy, check, per) in zip(cases, got):
        units, cus, lds, nb, rg, fg, cg = c
        d_wx, d_fy, d_check, _ = R.launch(units, cus, lds, nb)
        assert (wx, fy, check, per) == R.launch(*c), c
        floor = -(-units // 2 ** 18)
        assert wx == (max(min(rg, units), floor) if rg else d_wx), c              # clamped to the units; never below the floor; 0: the default
        assert fy == (min(fg, nb) if fg else min(nb, max(1, _target(cus, lds) // wx))), c
        assert check == (min(cg, d_check) if cg else d_check), c
        assert per == -(-units // wx) and per <= 2 ** 18 and wx * per >= units, c
    assert _launch(driver, [(100, 256, 12, 12, 1000, 0, 0)])[0][:2] == (100, 12)             # a requested wx larger than the units
    assert _launch(driver, [(2 ** 18 + 1, 256, 12, 12, 1, 0, 0)])[0][0] == 2                 # the floor stays above the hook
    assert _launch(driver, [(2073, 256, 12, 12, 1, 99, 0)])[0][:2] == (1, 12)                # frame_groups larger than nb
    assert _launch(driver, [(2073, 256, 12, 12, 0, 0, 0)])[0] == _launch(driver, [(2073, 256, 12, 12, 9, 12, 9)])[0] == (9, 12, 9, 231)


def test_launch_of_the_documented_benchmark(driver):
    """tools/gridmap_bench.py: 1e6 atoms ("all": 250 000 units), 256 frames per call, a 68 x 51 from_box map with sums, 256 CUs: a workgroup
    strides through its range (per > 256) and walks several frames (fy < nb) -- both loops run in the documented workload"""
    (wx, fy, check, per), = _launch(driver, [(250000, 256, 68 * 51 * 12, 256, 0, 0, 0)])
    assert (wx, fy, check, per) == (768, 1, 977, 326)
    assert per > 256 and fy < 256


def test_status_strings_and_abi(M):
    import groan_rs_amd as g
    lib = g._lib.load()
    assert g._lib.E_INVALID_SPAN == 23 and g._lib.E_INVALID_TILE == 24
    assert lib.gr_status_string(23) == b"invalid span of the grid map" and lib.gr_status_string(24) == b"invalid grid tile"
    assert lib.gr_gridmap_len(None, 1.0, None) == g._lib.E_INVALID_ARG
    assert lib.gr_gridmap_set_launch(None, 1, 1, 1) == g._lib.E_INVALID_ARG
    assert (g._lib.GM_STAT_LAST_RANGE_GROUPS, g._lib.GM_STAT_LAST_FRAME_GROUPS, g._lib.GM_STAT_LAST_CHECK_GROUPS) == (4, 5, 6)
    assert callable(M.GridMap.set_launch)
    assert g.GridMap is M.GridMap and issubclass(M.GridMap, M.TileGeometry)


MIRROR = r"""
#include "groan_hip.hpp"
int main() {
    groan::System system(1000, 0, 4);
    groan::GridMap map(system, {-2.0f, 7.0f}, {3.0f, 6.0f}, {0.15f, 0.20f});
    try { groan::GridMap bad(system, {2.0f, -2.0f}, {3.0f, 6.0f}, {0.15f, 0.20f}); } catch (const groan::Error &e) { if (e.variant != "InvalidSpan") return 1; }
    groan::GridMap box = groan::GridMap::from_box(system, {0.15f, 0.20f}, 0);
    std::vector<int> status;
    std::vector<float> offset(4, 1.5f);
    std::vector<uint64_t> outside = map.accumulate("all", 0, 4);
    outside = map.accumulate("all", 0, 4, groan::GridValue::Z, &offset, true, &status);
    std::vector<uint64_t> c = map.counts();
    std::vector<int64_t> s = map.sums_q();
    std::vector<float> m = map.mean();
    float tx = 0, ty = 0;
    bool in = map.is_inside(1.0f, 4.0f) && map.get_tile(1.0f, 4.0f, tx, ty);
    map.set_launch(2, 3, 1);
    map.set_launch();
    const uint64_t grid = map.stat(GR_GM_STAT_LAST_RANGE_GROUPS) + map.stat(GR_GM_STAT_LAST_FRAME_GROUPS) + map.stat(GR_GM_STAT_LAST_CHECK_GROUPS);
    map.clear();
    groan::GridMap moved(std::move(box));
    return (int)(c.size() + s.size() + m.size() + outside.size() + map.n_tiles() + map.n_tiles_x() + map.n_tiles_y() + grid) + (in ? 0 : 1);
}
"""


def test_cpp_mirror_compiles(tmp_path):
    src = tmp_path / "gridmap_snippet.cpp"
    src.write_text(MIRROR)
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
