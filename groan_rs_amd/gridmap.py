"""GridMap on resident frames: the xy tile map of src/structures/gridmap.rs, filled on the device.

The reference's GridMap is a container its user's trajectory loop fills atom by atom.  Here `accumulate` runs that loop over a
block of resident slots in one C call (gr_gridmap_accumulate_batch): per tile a count and the sum of one coordinate of the atoms
that fell into it -- density, height and thickness maps are ratios and differences of those.  The sums are 64-bit integers in
units of 2^-20 nm, so a map is bit for bit reproducible.  No arithmetic on atoms happens in Python; the tile geometry
(get_tile, is_inside, the coordinates written by write_map) goes through the library's own functions.
"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import (OK, E_EMPTY_GROUP, E_GROUP_NOT_FOUND, E_INVALID_ARG, E_INVALID_SPAN, E_INVALID_TILE, E_NO_BOX, E_NO_POSITION, E_NOT_ORTHOGONAL,
                   E_UNSUPPORTED_BOX, E_ZERO_BOX)
from .system import DeviceError, Dimension, GroanError, GroupError, _ptr, _simbox

Q_SCALE = 1048576.0     # quanta of the sums per nm


class GridMapError(GroanError):     # errors.rs: GridMapError
    pass


def _status_error(lib, status, msg=""):
    if status == E_INVALID_SPAN: return GridMapError("InvalidSpan", None, status)
    if status == E_INVALID_TILE: return GridMapError("InvalidGridTile", None, status)
    if status == E_INVALID_ARG: return GridMapError("InvalidArgument", msg, status)
    if status in (E_NO_BOX, E_NOT_ORTHOGONAL, E_ZERO_BOX, E_UNSUPPORTED_BOX): return GridMapError("InvalidSimBox", _simbox(status), status)
    return DeviceError(lib.gr_status_string(status).decode(), msg, status)


def get_len(span, tile):
    """GridMap::get_len: tiles along one axis, or GridMapError InvalidSpan / InvalidGridTile"""
    lib = _lib.load()
    s = (C.c_float * 2)(float(span[0]), float(span[1]))
    n = C.c_uint64(0)
    st = lib.gr_gridmap_len(s, C.c_float(tile), C.byref(n))
    if st != OK:
        raise _status_error(lib, st)
    return int(n.value)


def coord2index(span0, tile, coord):
    """x2index / y2index as a signed index (the reference's usize is this value after the wrapping cast)"""
    return int(_lib.load().gr_gridmap_coord2index(C.c_float(span0), C.c_float(tile), C.c_float(coord)))


def index2coord(span0, tile, index):
    """index2x / index2y, f32"""
    return np.float32(_lib.load().gr_gridmap_index2coord(C.c_float(span0), C.c_float(tile), int(index)))


def format_f32(v):
    """Rust's Display for f32: shortest digits that round-trip, positional, no trailing '.0'"""
    v = np.float32(v)
    if np.isnan(v):
        return "NaN"
    if np.isinf(v):
        return "inf" if v > 0 else "-inf"
    s = np.format_float_positional(v, unique=True, trim="-")
    return "-0" if s == "0" and np.signbit(v) else s


def _format_value(v):
    if isinstance(v, (float, np.floating)):
        return format_f32(v)
    return str(int(v))


class TileGeometry:
    """the map's geometry alone (no device, no values): GridMap::new's checks, is_inside, get_tile, extract, write_map"""

    def __init__(self, span_x, span_y, tile_dim):
        f = np.float32
        self.span_x, self.span_y = (f(span_x[0]), f(span_x[1])), (f(span_y[0]), f(span_y[1]))
        self.tile_dim = (f(tile_dim[0]), f(tile_dim[1]))
        self.n_tiles_x, self.n_tiles_y = get_len(self.span_x, self.tile_dim[0]), get_len(self.span_y, self.tile_dim[1])

    @property
    def n_tiles(self):
        return self.n_tiles_x * self.n_tiles_y

    def _index(self, x, y):
        return coord2index(self.span_x[0], self.tile_dim[0], x), coord2index(self.span_y[0], self.tile_dim[1], y)

    def is_inside(self, x, y):
        ix, iy = self._index(x, y)
        return 0 <= ix < self.n_tiles_x and 0 <= iy < self.n_tiles_y

    def get_tile(self, x, y):
        """coordinates (f32) of the tile the point lies in, or None outside the map"""
        if not self.is_inside(x, y):
            return None
        ix, iy = self._index(x, y)
        return index2coord(self.span_x[0], self.tile_dim[0], ix), index2coord(self.span_y[0], self.tile_dim[1], iy)

    def extract(self, values, column_major=False):
        """[(x, y, value)] over the tiles, row-major (x outer) or column-major (y outer); `values` is an [nx, ny] array.
        (Column-major x coordinates come from index2x; the reference calls index2y there, gridmap.rs:678.)"""
        v = np.asarray(values)
        if v.shape != (self.n_tiles_x, self.n_tiles_y):
            raise ValueError("values must have the map's shape (n_tiles_x, n_tiles_y)")
        xs = [index2coord(self.span_x[0], self.tile_dim[0], i) for i in range(self.n_tiles_x)]
        ys = [index2coord(self.span_y[0], self.tile_dim[1], j) for j in range(self.n_tiles_y)]
        if column_major:
            return [(xs[i], ys[j], v[i, j]) for j in range(self.n_tiles_y) for i in range(self.n_tiles_x)]
        return [(xs[i], ys[j], v[i, j]) for i in range(self.n_tiles_x) for j in range(self.n_tiles_y)]

    def write_map(self, fh, values, column_major=False):
        """GridMap::write_map / write_map_column_major: one line "%10.6f %10.6f value" per tile"""
        for x, y, v in self.extract(values, column_major):
            fh.write("%10.6f %10.6f %s\n" % (x, y, _format_value(v)))


class GridMap(TileGeometry):
    """GridMap::new((x0, x1), (y0, y1), (tile_x, tile_y)) over the frames of `system`"""

    def __init__(self, system, span_x, span_y, tile_dim, _from_box_slot=None):
        self._lib = _lib.load()
        self.system = system
        st = C.c_int(0)
        td = np.ascontiguousarray(tile_dim, np.float32)
        if _from_box_slot is None:
            sx, sy = np.ascontiguousarray(span_x, np.float32), np.ascontiguousarray(span_y, np.float32)
            self._map = self._lib.gr_gridmap_create(system._ctx, _ptr(sx), _ptr(sy), _ptr(td), C.byref(st))
        else:
            self._map = self._lib.gr_gridmap_from_box(system._ctx, int(_from_box_slot), _ptr(td), C.byref(st))
        if not self._map:
            raise _status_error(self._lib, st.value, self._lib.gr_last_error(system._ctx).decode(errors="replace"))
        nx, ny = C.c_uint64(0), C.c_uint64(0)
        sx, sy, td = np.zeros(2, np.float32), np.zeros(2, np.float32), np.zeros(2, np.float32)
        self._lib.gr_gridmap_dims(self._map, C.byref(nx), C.byref(ny), _ptr(sx), _ptr(sy), _ptr(td))
        self.n_tiles_x, self.n_tiles_y = int(nx.value), int(ny.value)
        self.span_x, self.span_y, self.tile_dim = (sx[0], sx[1]), (sy[0], sy[1]), (td[0], td[1])
        system._plans.append(self)

    @classmethod
    def from_box(cls, system, tile_dim, slot=0):
        """GridMap::from_box: spans (0, box.x), (0, box.y) of the slot's box (orthogonal boxes only)"""
        return cls(system, None, None, tile_dim, _from_box_slot=slot)

    def close(self):
        if getattr(self, "_map", None):
            self._lib.gr_gridmap_destroy(self._map)
            self._map = None

    def stat(self, key):
        v = C.c_uint64(0)
        if self._lib.gr_gridmap_stat(self._map, int(key), C.byref(v)) != OK:
            raise ValueError("unknown grid map stat %r" % (key,))
        return int(v.value)

    def set_launch(self, range_groups=0, frame_groups=0, check_groups=0):
        """cap the grids of a call's launches: ranges of the group, workgroups sharing the frames of a range, workgroups of the
        position check (0: the default).  The result never depends on it; GM_STAT_LAST_*_GROUPS report what was launched"""
        if self._lib.gr_gridmap_set_launch(self._map, int(range_groups), int(frame_groups), int(check_groups)) != OK:
            raise ValueError("set_launch on a closed grid map")

    # -- filling
    def _raise(self, status):
        lib, ctx = self._lib, self.system._ctx
        msg = lib.gr_last_error(ctx).decode(errors="replace")
        idx = int(lib.gr_last_error_index(ctx))
        if status == E_GROUP_NOT_FOUND: raise GroupError("NotFound", msg, status)
        if status == E_EMPTY_GROUP: raise GroupError("EmptyGroup", msg, status)
        if status == E_NO_POSITION: raise GroupError("InvalidPosition", idx, status)
        raise _status_error(lib, status, msg)

    def accumulate(self, group, first_slot, n_frames, value="count", offset=None, wrap=False, raise_on_error=True, force_global=False):
        """bin the atoms of `group` of n_frames slots: count per tile and, for value = Dimension.X / Y / Z, the sum of that
        coordinate minus offset[frame].  -> (n_outside uint64 [n_frames], status int32 [n_frames])"""
        val = _lib.GM_COUNT if (isinstance(value, str) and value == "count") else {Dimension.X: _lib.GM_X, Dimension.Y: _lib.GM_Y, Dimension.Z: _lib.GM_Z}.get(value)
        if val is None:
            raise ValueError("value must be 'count', Dimension.X, Dimension.Y or Dimension.Z")
        off = None
        if offset is not None:
            off = np.ascontiguousarray(offset, np.float32)
            if off.shape != (n_frames,):
                raise ValueError("offset must have one entry per frame")
        n_out, st_arr = np.zeros(n_frames, np.uint64), np.zeros(n_frames, np.int32)
        flags = (_lib.GM_WRAP if wrap else 0) | (_lib.GM_FORCE_GLOBAL if force_global else 0)
        st = self._lib.gr_gridmap_accumulate_batch(self._map, first_slot, n_frames, group.encode(), val, _ptr(off), flags, _ptr(n_out), _ptr(st_arr))
        if st != OK and raise_on_error:
            self._raise(st)
        return n_out, st_arr

    def clear(self):
        st = self._lib.gr_gridmap_clear(self._map)
        if st != OK:
            self._raise(st)

    # -- reading
    def _read(self, want_mean=False):
        shape = (self.n_tiles_x, self.n_tiles_y)
        cnt, sq = np.zeros(shape, np.uint64), np.zeros(shape, np.int64)
        mean = np.zeros(shape, np.float32) if want_mean else None
        st = self._lib.gr_gridmap_read(self._map, _ptr(cnt), _ptr(sq), _ptr(mean))
        if st != OK:
            self._raise(st)
        return cnt, sq, mean

    @property
    def counts(self):
        return self._read()[0]

    @property
    def sums_q(self):
        return self._read()[1]

    @property
    def sums(self):
        """float64 nm (exact: the integer sums times 2^-20)"""
        return self._read()[1].astype(np.float64) / Q_SCALE

    def mean(self):
        """float32 [nx, ny]: sum / count per tile, NaN where nothing was counted"""
        return self._read(True)[2]
