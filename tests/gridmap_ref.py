"""numpy restatement of the GridMap geometry and of gr_gridmap_accumulate_batch (the yardstick of the grid-map tests).

Written from the library's specification (include/groan_hip.h, "GridMap"), which restates the reference
(src/structures/gridmap.rs:146-157 get_len, :715-724 x2index / y2index, :729-738 index2x / index2y):
  index      the f32 quotient (coord - span0) / tile, promoted to f64, then trunc(q + copysign(0.5, q)) -- round half away from
             zero (np.round is half-even and is not used); NaN -> 0, saturation at the ends of int64 like Rust's `as isize`
  coordinate (f32) index * tile + span0, every operation rounded to f32 on its own
  quantum    q = rint((float64) v * 2^20), v = coordinate - offset in f32; not finite or |v| >= 2^31: the atom counts as outside
  mean       (float32)((float64) sum_q * 2^-20 / (float64) count), NaN where count == 0
The wrap is the oracle's (oracle_lib.wrap_atoms).  A frame that fails contributes nothing and reports no atom outside."""
import numpy as np

F = np.float32
I64_MAX, I64_MIN = np.iinfo(np.int64).max, np.iinfo(np.int64).min
OK, E_NO_BOX, E_NOT_ORTHOGONAL, E_EMPTY_GROUP, E_NO_POSITION, E_GROUP_NOT_FOUND, E_INVALID_ARG, E_INVALID_SPAN, E_INVALID_TILE = 0, 1, 2, 4, 6, 8, 10, 23, 24
COUNT, X, Y, Z = 0, 1, 2, 3


def get_len(span, tile):
    """-> (status, n)"""
    s0, s1, t = F(span[0]), F(span[1]), F(tile)
    if np.isnan(s0) or np.isnan(s1) or np.isnan(t):
        return E_INVALID_ARG, 0
    with np.errstate(all="ignore"):
        diff = F(s1 - s0)
        if diff < 0:
            return E_INVALID_SPAN, 0
        if t < 0:
            return E_INVALID_ARG, 0
        if t > diff or t == 0:
            return E_INVALID_TILE, 0
        q = np.float64(F(diff / t))
    r = np.trunc(q + np.copysign(0.5, q))
    if np.isnan(r):
        return OK, 1
    return OK, (2 ** 64 - 1 if r >= 2.0 ** 64 else int(r) + 1)


def coord2index(coord, span0, tile):
    """int64 array of tile indices (any shape)"""
    c = np.asarray(coord, F)
    with np.errstate(all="ignore"):
        q = ((c - F(span0)).astype(F) / F(tile)).astype(F).astype(np.float64)
        r = np.trunc(q + np.copysign(0.5, q))
    out = np.zeros(c.shape, np.int64)
    hi, lo, nan = r >= 2.0 ** 63, r <= -(2.0 ** 63), np.isnan(r)
    mid = ~(hi | lo | nan)
    out[mid] = r[mid].astype(np.int64)
    out[hi], out[lo] = I64_MAX, I64_MIN
    return out


def index2coord(index, span0, tile):
    with np.errstate(all="ignore"):
        return ((np.asarray(index).astype(F) * F(tile)).astype(F) + F(span0)).astype(F)


def quantise(v):
    """-> (accepted, q int64) for f32 values v"""
    v = np.asarray(v, F)
    with np.errstate(all="ignore"):
        ok = np.isfinite(v) & (np.abs(v) < F(2.0 ** 31))
        q = np.zeros(v.shape, np.int64)
        q[ok] = np.rint(v[ok].astype(np.float64) * 2.0 ** 20).astype(np.int64)
    return ok, q


def mean(count, sum_q):
    with np.errstate(all="ignore"):
        m = (sum_q.astype(np.float64) * 2.0 ** -20 / count.astype(np.float64)).astype(F)
    m[count == 0] = np.nan
    return m


def launch(units, n_cus, lds_bytes, nb, range_groups=0, frame_groups=0, check_groups=0):
    """the grids of one segment, from the header's words (gr_gridmap_set_launch) and DESIGN.md 3.8 -> (wx, fy, check_wgs, per).
    per_cu workgroups fit a CU beside each other: 8, or fewer when the privatised map of lds_bytes fills the CU's 160 KiB sooner
    (lds_bytes 0: the global path); target = CUs x per_cu workgroups fill the chip; a range is 256 units or more, 2^18 at most."""
    per_cu = min(8, (160 * 1024) // lds_bytes) if lds_bytes else 8
    target = max(n_cus, 1) * per_cu
    wx = min(range_groups, units) if range_groups else min(-(-units // 256), target)
    wx = max(wx, -(-units // 2 ** 18))
    fy = min(frame_groups, nb) if frame_groups else min(nb, max(1, target // wx))
    check = min(-(-units // 256), 4096)
    if check_groups:
        check = min(check, check_groups)
    return wx, fy, check, -(-units // wx)


def units(idx, contiguous_or_masked):
    """what k_gm_accumulate cuts its ranges from: the 4-atom groups of the span of a block or a masked selection, else list entries"""
    idx = np.asarray(idx)
    return int((idx[-1] >> 2) - (idx[0] >> 2) + 1) if contiguous_or_masked else len(idx)


class Map:
    def __init__(self, span_x, span_y, tile_dim):
        self.span_x, self.span_y, self.tile = (F(span_x[0]), F(span_x[1])), (F(span_y[0]), F(span_y[1])), (F(tile_dim[0]), F(tile_dim[1]))
        sx, self.nx = get_len(span_x, tile_dim[0])
        sy, self.ny = get_len(span_y, tile_dim[1])
        assert sx == OK and sy == OK
        self.count = np.zeros((self.nx, self.ny), np.uint64)
        self.sum_q = np.zeros((self.nx, self.ny), np.int64)

    def clear(self):
        self.count[:] = 0; self.sum_q[:] = 0

    def mean(self):
        return mean(self.count, self.sum_q)

    def accumulate(self, frames, boxes, idx, value=COUNT, offset=None, wrap=False, wrap_fn=None):
        """frames: [nf] arrays [n, 3] f32; boxes: [nf] box9 or None; idx: the group's atoms in group order.
        -> (n_outside uint64 [nf], status int32 [nf], first bad atom per frame or -1)"""
        nf = len(frames)
        idx = np.asarray(idx, np.int64)
        n_out, status, bad = np.zeros(nf, np.uint64), np.zeros(nf, np.int32), np.full(nf, -1, np.int64)
        for f in range(nf):
            pos = np.asarray(frames[f], F)
            if wrap and boxes[f] is None:
                status[f] = E_NO_BOX
                continue
            p = pos[idx]
            nanx = np.isnan(p[:, 0])
            if nanx.any():
                status[f] = E_NO_POSITION; bad[f] = idx[np.argmax(nanx)]
                continue
            if wrap:
                p = wrap_fn(p, boxes[f])
            ix = coord2index(p[:, 0], self.span_x[0], self.tile[0])
            iy = coord2index(p[:, 1], self.span_y[0], self.tile[1])
            inside = (ix >= 0) & (ix < self.nx) & (iy >= 0) & (iy < self.ny)
            q = np.zeros(len(idx), np.int64)
            if value != COUNT:
                with np.errstate(all="ignore"):
                    v = (p[:, value - 1] - (F(offset[f]) if offset is not None else F(0))).astype(F)
                ok, q = quantise(v)
                inside &= ok
            n_out[f] = np.count_nonzero(~inside)
            np.add.at(self.count, (ix[inside], iy[inside]), np.uint64(1))
            if value != COUNT:
                np.add.at(self.sum_q, (ix[inside], iy[inside]), q[inside])
        return n_out, status, bad
