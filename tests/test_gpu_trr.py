"""trr frames straight into device slots (gr_trr_read_frames_device: raw big-endian positions over PCIe, byte order and
precision converted on the GPU) must equal the host reader (gr_trr_read_frame), which equals the reference's reader
(tests/test_trr_reader.py); all-zero positions arrive as the missing-position marker (trr_io.rs:108-112)."""
import os
import struct

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def G():
    import groan_rs_amd as g
    g._lib.load()
    return g


@pytest.mark.parametrize("name", ["triclinic_trajectory.trr", "triclinic_trajectory_double_precision.trr", "dodecahedron_trajectory_full.trr",
                                  "octahedron_trajectory.trr", "short_trajectory_protein.trr"])
def test_device_conversion_equals_the_host_reader(G, name):
    t = G.TrrFile(os.path.join(GOLD, name))
    nb = 4
    s = G.System(t.n_atoms, n_slots=nb)
    for f0 in range(0, t.n_frames, nb):
        n = min(nb, t.n_frames - f0)
        steps, times = t.read_frames_device(s, f0, n)
        for k in range(n):
            x, _, _, box9, step, time, _ = t.read_frame(f0 + k)
            got = s.get_positions(k)
            zero = ~x.any(axis=1)
            assert np.array_equal(np.isnan(got[:, 0]), zero)
            assert np.array_equal(got[~zero], x[~zero])
            assert steps[k] == step and times[k] == np.float32(time)
            if box9 is not None:
                assert np.array_equal(s.get_box(k), box9)
    # strided frames, then an analysis on what arrived
    steps, _ = t.read_frames_device(s, 0, 3, frame_step=2)
    assert [int(v) for v in steps] == [t.frame_info(k)["step"] for k in (0, 2, 4)]
    if t.frame_info(0)["positions"]:
        np.testing.assert_allclose(s.group_get_center_naive("all", slot=0), t.read_frame(0)[0].mean(0), atol=1e-5)
    s.close(); t.close()


def x_sections(raw):
    """-> per frame (offset of the positions section or None, bytes per real, atoms): XDR header = magic, version string, 13 ints
    (ir e box vir pres top sym x v f sizes, natoms, step, nre), time, lambda; then ir, e, box, vir, pres, top, sym, x, v, f"""
    out, p = [], 0
    while p < len(raw):
        magic, _, sl = struct.unpack_from(">iii", raw, p)
        assert magic == 1993 and sl == 12
        ir, e, box, vir, pres, top, sym, xs, vs, fs, natoms, _, _ = struct.unpack_from(">13i", raw, p + 24)
        rs = box // 9 if box else xs // (3 * natoms)
        q = p + 24 + 52 + 2 * rs + ir + e + box + vir + pres + top + sym
        out.append((q if xs else None, rs, natoms))
        p = q + xs + vs + fs
    return out


@pytest.mark.parametrize("precision", ["single", "double"])
def test_a_nan_x_in_the_file_is_no_position_in_all_three(G, tmp_path, precision):
    """a position whose x is a literal NaN (y and z finite) is an atom without position: the device reader must store it as the host reader +
    set_frame do (NaN in x, y and z), and the one-float4-per-lane translate / wrap must then give the same bits as the walk"""
    L = np.array([6.0, 5.5, 7.0], np.float32)
    box9 = np.array([L[0], L[1], L[2], 0, 0, 0, 0, 0, 0], np.float32)
    if precision == "single":
        n, nf = 301, 3
        rng = np.random.default_rng(43)
        path = str(tmp_path / "nan_x.trr")
        with G.TrrWriter(path) as w:
            for f in range(nf):
                x = (rng.uniform(-0.3, 1.3, (n, 3)) * L).astype(np.float32)
                if f == 1:
                    x[17] = 0.0                                                   # (the all-zero rule, beside it)
                w.write_frame(x, box9, step=f)
        raw = bytearray(open(path, "rb").read())
    else:
        raw = bytearray(open(os.path.join(GOLD, "triclinic_trajectory_double_precision.trr"), "rb").read())
    secs = x_sections(raw)
    assert all(rs == (4 if precision == "single" else 8) for _, rs, _ in secs)
    n, nf = secs[0][2], min(len(secs), 4)
    with_x = [f for f in range(nf) if secs[f][0] is not None]
    patched = {with_x[0]: 5, with_x[-1]: n - 2}                                   # frame -> atom whose x becomes NaN
    for f, a in patched.items():
        off, rs, _ = secs[f]
        raw[off + 3 * a * rs: off + 3 * a * rs + rs] = struct.pack(">f" if rs == 4 else ">d", float("nan"))
    path = str(tmp_path / ("patched_%s.trr" % precision))
    open(path, "wb").write(bytes(raw))
    t = G.TrrFile(path)
    s = G.System(n, n_slots=nf)
    ref = G.System(n, n_slots=nf)
    host = []
    for f in range(nf):
        x = t.read_frame(f)[0]
        if f in patched:
            a = patched[f]
            assert np.isnan(x[a, 0]) and np.isfinite(x[a, 1:]).all() and (x[a, 1:] != 0).any()
        x[~x.any(axis=1), 0] = np.nan                                             # the reference's all-zero rule (TrrFile.frames)
        host.append(x)
        ref.set_frame(x, box9, slot=f)
    t.read_frames_device(s, 0, nf)
    for f in range(nf):
        assert np.array_equal(s.get_positions(f), ref.get_positions(f), equal_nan=True), f
        if f in patched:
            assert np.isnan(s.get_positions(f)[patched[f]]).all()
    # the rows kernel against the walk on what the device reader stored (orthorhombic boxes: the rows kernel's case)
    s.group_create_from_ranges("part", [(3, n - 5)])
    res = {}
    for rows in (1, 0):
        s.set_tuning(translate_rows=rows, center_resident=0)
        out = []
        for op in ("wrap", "translate"):
            t.read_frames_device(s, 0, nf)
            for f in range(nf):
                s.set_box(box9, slot=f)
            st = s.group_wrap_batch(None, 0, nf, raise_on_error=False) if op == "wrap" else s.group_translate_batch("part", [0.4, -7.9, 13.1], 0, nf, raise_on_error=False)
            out.append((list(st), [s.get_positions(f) for f in range(nf)]))
        res[rows] = out
    for k in range(2):
        assert res[1][k][0] == res[0][k][0], (k, res[1][k][0], res[0][k][0])
        for f in range(nf):
            assert np.array_equal(res[1][k][1][f], res[0][k][1][f], equal_nan=True), (k, f)
    s.close(); ref.close(); t.close()
