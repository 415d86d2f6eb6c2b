"""The cell grid's geometry in orthorhombic boxes, restated in float32 numpy (groan_rs_amd/csrc/gr_cellgrid.h: gr_cellgrid_make and
gr_cg_cell_of; groan_rs_amd/csrc/gr_math.h: gr_wrap_k, gr_wrap_value).  Every operation is one IEEE float32 operation applied
elementwise, so the cells are the same bits on every host; tests/test_cellgrid_host.py compares them with the C++ functions' own.

The one fused multiply-add of the original, fmaf(-k, L, t), is taken in float64: k is a whole number below 2^24 and L has 24 bits, so
k L is exact there, and t lies within a box length of it, so the sum is exact too -- rounding it to float32 is the fma's single rounding.

The GPU tests use this module to put atoms ON cell borders: border(L, cutoff, m) is the lowest float binned to cell m."""
import numpy as np

F = np.float32
SLACK = F(2.0 ** -15)          # GR_CG_SLACK
LOOP_TURNS = 16                # GR_LOOP_TURNS
MAX_CELLS = 1024


def _fma(a, b, c):
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(F)


def wrap_k(t, L):
    t = np.asarray(t, F); L = np.broadcast_to(np.asarray(L, F), t.shape); iL = F(1.0) / L
    k = np.floor(t * iL).astype(F)
    r = _fma(-k, L, t)
    k = k + np.where(r < 0, F(-1.0), F(0.0)) + np.where(r > L, F(1.0), F(0.0))
    k = k + np.where((r == L) & (t < 0) & (_fma(-(k + F(1.0)), L, t) == 0), F(1.0), F(0.0))
    r = _fma(-k, L, t)
    return k - np.where((r == 0) & (t > 0), F(1.0), F(0.0))


def wrap(t, L):
    """gr_wrap_value: one rounded t - k L within one turn and beyond LOOP_TURNS, the reference's loop in between"""
    t = np.asarray(t, F); L = np.broadcast_to(np.asarray(L, F), t.shape)
    k = wrap_k(t, L)
    closed = _fma(-k, L, t)
    w = t.copy()
    for _ in range(LOOP_TURNS + 2):
        w = np.where(w > L, w - L, w)
    for _ in range(LOOP_TURNS + 2):
        w = np.where(w < 0, w + L, w)
    with np.errstate(invalid="ignore"):
        loop = (np.abs(k) > 1) & (np.abs(k) <= LOOP_TURNS)
    return np.where(loop, w, closed).astype(F)


def thickness(L, cutoff):
    """the least cell thickness along an axis of length L"""
    return F(F(F(cutoff) + F(SLACK * F(L))) * F(1.00001))


def cells(L, cutoff):
    """gr_cellgrid_make along one axis -> (cells, inv_cell)"""
    L = F(L)
    n = np.floor(F(L / thickness(L, cutoff)))
    n = F(min(max(n, 1.0), float(MAX_CELLS))) if n == n else F(1.0)
    return int(n), F(n / L)


def cell(x, L, cutoff):
    """gr_cg_cell_of along one axis, elementwise over x"""
    n, inv = cells(L, cutoff)
    k = np.floor(wrap(x, L) * inv).astype(np.int64)
    return np.maximum(k, 0) % n


def grid(box3, cutoff):
    """cells per axis of an orthorhombic box"""
    return tuple(cells(L, cutoff)[0] for L in box3)


def border(L, cutoff, m):
    """the lowest float of [0, L) binned to cell m (0 < m < cells): the float below it is the highest binned to cell m - 1"""
    n, _ = cells(L, cutoff)
    assert 0 < m < n
    w = F(float(m) * float(F(L)) / n)
    while w > 0 and cell(np.nextafter(w, F(0.0)), L, cutoff) >= m:
        w = np.nextafter(w, F(0.0))
    while cell(w, L, cutoff) < m:
        w = np.nextafter(w, F(np.inf))
    return F(w)


def step_length(cutoff, k):
    """the lowest box length that gives k cells along its axis"""
    lo = F(cutoff) * F(k); hi = lo
    while cells(hi, cutoff)[0] < k:
        hi = F(hi * F(1.001))
    lo_b, hi_b = int(lo.view(np.uint32)), int(hi.view(np.uint32))
    while hi_b - lo_b > 1:
        mid = (lo_b + hi_b) // 2
        if cells(np.uint32(mid).view(F), cutoff)[0] < k: lo_b = mid
        else: hi_b = mid
    return np.uint32(hi_b).view(F)
