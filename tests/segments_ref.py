"""What the Segments tests share (test_gpu_segments.py, test_gpu_segments_edges.py): the oracle called once per segment as a group, in
its f64-accumulation mode (within 1e-6 nm of exact arithmetic on the segments used), and the comparison against it.

Margin: TOL = 1e-5 nm per component, the project's parity margin.  A periodic centre that lies within SEAM = 1e-4 nm of a cell face may
legitimately come out on either side of it: a component whose oracle ESTIMATE (for the PBC kind: the segment's unweighted estimate, about
which it unwraps) lies that close to 0 or to the box length is compared modulo the box vector, and _check_against asserts that at most
16 segments per frame and kind need that rule."""
import itertools

import numpy as np

import oracle_lib as O

F = np.float32
TOL = 1e-5
SEAM = 1e-4
NAIVE, ESTIMATE, PBC = 0, 1, 2
KINDS = [(NAIVE, 0), (NAIVE, 1), (ESTIMATE, 0), (ESTIMATE, 1), (PBC, 0), (PBC, 1)]
E_NO_BOX, E_NO_POSITION, E_NO_MASS, E_INVALID_ARG = 1, 6, 7, 10


def _bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def _cell(box):
    """rows = the box vectors (gromacs order xx yy zz xy xz yx yz zx zy)"""
    b = np.zeros(9); b[:len(box)] = box
    return np.array([[b[0], b[3], b[4]], [b[5], b[1], b[6]], [b[7], b[8], b[2]]], np.float64)


# ------------------------------------------------------------------ the oracle, per segment
def _oracle(pos, box, masses, lists, kind, weighted):
    """-> (centres float32 [M, 3] with NaN rows for failed segments, [(status, index) or None] per segment)"""
    out, err = np.full((len(lists), 3), np.nan, F), [None] * len(lists)
    m = masses if weighted else None
    for s, idx in enumerate(lists):
        try:
            if kind == NAIVE: out[s] = O.center_naive(pos, idx, m)
            elif kind == ESTIMATE: out[s] = O.estimate_center(pos, idx, box, m)
            else: out[s] = O.get_center(pos, idx, box, m)
        except O.OracleError as e:
            err[s] = (e.status, int(e.index))
    return out, err


def _seam_flags(est, box):
    """[M, 3] bool: the estimate's component (along the box vectors) lies within SEAM nm of 0 or of the box length"""
    H = _cell(box)
    u = np.asarray(est, np.float64) @ np.linalg.inv(H)
    L = np.diag(H)
    with np.errstate(invalid="ignore"):
        return (np.abs(u) * L < SEAM) | (np.abs(1.0 - u) * L < SEAM)


def _max_error(got, want, flags, box):
    """largest component error; flagged components are compared modulo their box vector"""
    d = np.asarray(got, np.float64) - np.asarray(want, np.float64)
    err = np.abs(d).max(axis=1)
    if flags is not None and flags.any():
        H = _cell(box)
        for s in np.nonzero(flags.any(axis=1))[0]:
            shifts = [(-1, 0, 1) if flags[s, k] else (0,) for k in range(3)]
            err[s] = min(np.abs(d[s] - np.array(sh, np.float64) @ H).max() for sh in itertools.product(*shifts))
    return err


def _reference(frames, boxes, masses, lists):
    """{(kind, weighted): (centres [F, M, 3], errors [F][M], seam flags [F, M, 3] or None)}, the oracle summing in double"""
    ref = {}
    O.set_accumulate_f64(True)
    try:
        for kind, w in KINDS:
            cen, errs = [], []
            for f, pos in enumerate(frames):
                if boxes[f] is None and kind != NAIVE:
                    cen.append(np.full((len(lists), 3), np.nan, F)); errs.append(None)
                    continue
                c, e = _oracle(pos, boxes[f], masses, lists, kind, w)
                cen.append(c); errs.append(e)
            ref[(kind, w)] = [np.stack(cen), errs, None]
    finally:
        O.set_accumulate_f64(False)
    for kind, w in KINDS:
        if kind == NAIVE:
            continue
        est = ref[(ESTIMATE, 0 if kind == PBC else w)][0]
        ref[(kind, w)][2] = np.stack([_seam_flags(est[f], boxes[f]) if boxes[f] is not None else np.zeros(est[f].shape, bool) for f in range(len(frames))])
    return ref


def _check_against(got, status, ref, key, boxes, n_failed_expected=None):
    """every frame of one call against the reference: values, NaN rows exactly where the oracle fails, the frame's status"""
    cen, errs, flags = ref[key]
    kind = key[0]
    for f in range(cen.shape[0]):
        if boxes[f] is None and kind != NAIVE:
            assert status[f] == E_NO_BOX and np.isnan(got[f]).all()
            continue
        failed = [s for s, e in enumerate(errs[f]) if e is not None]
        assert np.isnan(got[f]).any(axis=1).nonzero()[0].tolist() == failed, (key, f)
        assert status[f] == (errs[f][failed[0]][0] if failed else 0), (key, f, status[f])
        ok = np.array([e is None for e in errs[f]])
        fl = flags[f] if flags is not None else None
        if fl is not None:
            assert int(fl[ok].any(axis=1).sum()) <= 16, (key, f)
        err = _max_error(got[f][ok], cen[f][ok], fl[ok] if fl is not None else None, boxes[f])
        print("segments kind %d weighted %d frame %d: max |error| %.3g nm over %d segments, %d at a cell face" %
              (key[0], key[1], f, err.max(), int(ok.sum()), 0 if fl is None else int(fl[ok].any(axis=1).sum())))
        assert err.max() <= TOL, (key, f, float(err.max()), int(err.argmax()))
