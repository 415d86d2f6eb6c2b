"""What the gyration tests share (test_gpu_gyration.py, test_gpu_gyration_edges.py): the reference in numpy f64 and the comparison.

Reference.  For one frame and one segment the unwrapping origin is the centre the GPU returned (it is pinned to `centers` bit for bit
separately, and the tensor does not depend on it).  For the periodic kinds every atom is brought to its nearest image of that origin:
the difference is reduced along the box vectors and then the 27 neighbouring cells are searched.  The weighted mean and
S_ab = sum w (d_a - m_a)(d_b - m_b) / sum w are then computed in two passes.

Margin, derived and not measured.  A component of d carries at most 2 E of f32 rounding -- one subtraction, plus the shifts of the minimum
image -- with E the f32 spacing at the largest coordinate or box length involved.  To first order the products and the parallel-axis
term are therefore off by at most 8 E r_max, r_max the largest |d| in the segment; the f32 store adds 2^-24 of the value.  Allowed:
    |dS_ab| <= 16 E r_max + 2^-22 tr S          (twice the first-order bound)
    |dRg^2| <= 3 times that                     (Rg^2 and not Rg: a segment of one atom has Rg = 0)
check_moments prints the largest observed error over margin."""
import itertools

import numpy as np

from segments_ref import NAIVE, _cell

F = np.float32
SHIFTS = np.array(list(itertools.product((-1.0, 0.0, 1.0), repeat=3)))


def tensor_of(moments):
    """[..., 10] -> [..., 3, 3] from the entries xx yy zz xy xz yz"""
    m = np.asarray(moments)
    return m[..., [4, 7, 8, 7, 5, 9, 8, 9, 6]].reshape(m.shape[:-1] + (3, 3))


def flatten(lists):
    """the segments' atom lists -> (flat atom list, segment of each entry, M): what `reference` takes in place of the lists"""
    return (np.concatenate([np.asarray(l, np.int64) for l in lists]), np.repeat(np.arange(len(lists)), [len(l) for l in lists]), len(lists))


def reference(pos, box, masses, lists, centres, kind, weighted):
    """one frame -> (S [M, 3, 3], margin [M]) in f64; NaN rows where the centre is NaN"""
    idx, sid, M = lists if isinstance(lists, tuple) else flatten(lists)
    x = np.asarray(pos, np.float64)[idx]
    c = np.asarray(centres, np.float64)
    w = np.asarray(masses, np.float64)[idx] if weighted else np.ones(len(idx))
    big = np.zeros(M)
    with np.errstate(invalid="ignore"):
        np.maximum.at(big, sid, np.abs(x).max(axis=1))
        d = x - c[sid]
        if kind != NAIVE:
            H = _cell(box)
            u = d @ np.linalg.inv(H)
            d = (u - np.rint(u)) @ H
            cand = d[:, None, :] + (SHIFTS @ H)[None, :, :]
            d = cand[np.arange(len(d)), np.argmin((cand * cand).sum(axis=2), axis=1)]
            big = np.maximum(big, np.abs(H).sum(axis=1).max())       # (the longest box vector, generously)
        W = np.bincount(sid, w, M)
        mean = np.stack([np.bincount(sid, w * d[:, a], M) for a in range(3)], axis=1) / W[:, None]
        dd = d - mean[sid]
        S = np.zeros((M, 3, 3))
        for a in range(3):
            for b in range(3):
                S[:, a, b] = np.bincount(sid, w * dd[:, a] * dd[:, b], M) / W
        r_max = np.zeros(M)
        np.maximum.at(r_max, sid, np.nan_to_num(np.sqrt((d * d).sum(axis=1)), nan=0.0))
        E = np.spacing(np.nan_to_num(big, nan=1.0).astype(F)).astype(np.float64)
        margin = 16.0 * E * r_max + 2.0 ** -22 * np.trace(S, axis1=1, axis2=2)
    bad = np.isnan(c).any(axis=1)
    S[bad] = np.nan
    margin[bad] = np.nan
    return S, margin


def check_moments(what, moments, S_ref, margin):
    """moments [M, 10] of one frame against the reference; rows whose reference is NaN must be NaN everywhere"""
    bad = np.isnan(margin)
    assert np.isnan(moments[bad]).all() and not np.isnan(moments[~bad]).any(), what
    if bad.all():
        return 0.0
    S = tensor_of(moments).astype(np.float64)[~bad]
    m = margin[~bad]
    err_s = np.abs(S - S_ref[~bad]).max(axis=(1, 2))
    err_r = np.abs(moments[~bad, 3].astype(np.float64) ** 2 - np.trace(S_ref[~bad], axis1=1, axis2=2))
    tiny = np.finfo(np.float64).tiny
    ratio_s, ratio_r = err_s / np.maximum(m, tiny), err_r / np.maximum(3.0 * m, tiny)
    ratio_s[err_s == 0.0] = 0.0
    ratio_r[err_r == 0.0] = 0.0
    print("gyration %s: max |dS| / margin %.3g, max |dRg^2| / margin %.3g over %d segments" % (what, ratio_s.max(), ratio_r.max(), int((~bad).sum())))
    assert (err_s <= m).all(), (what, int(np.argmax(ratio_s)), float(ratio_s.max()))
    assert (err_r <= 3.0 * m).all(), (what, int(np.argmax(ratio_r)), float(ratio_r.max()))
    return float(max(ratio_s.max(), ratio_r.max()))


def check_axes(what, moments, axes, S_ref=None, need_all=None):
    """the axes block [M, 12] of one frame against the RETURNED tensor, and (S_ref given) its directions against the reference's:
    v_k is compared wherever the reference's lambda_k is at least 0.2 lambda_1 away from both other eigenvalues; need_all [M] bool marks
    the segments for which that must hold for all three"""
    bad = np.isnan(moments).any(axis=1)
    assert np.isnan(axes[bad]).all() and not np.isnan(axes[~bad]).any(), what
    S = tensor_of(moments).astype(np.float64)
    worst = 0.0
    for s in np.nonzero(~bad)[0]:
        lam, V = axes[s, 0:3].astype(np.float64), axes[s, 3:12].astype(np.float64).reshape(3, 3)
        tr = float(np.trace(S[s]))
        assert lam[0] >= lam[1] >= lam[2], (what, s, lam)
        assert np.abs(lam - np.linalg.eigvalsh(S[s])[::-1]).max() <= 2.0 ** -22 * tr, (what, s)
        assert np.abs(V @ V.T - np.eye(3)).max() <= 1e-6 and np.linalg.det(V) > 0.0, (what, s)
        for k in (0, 1):      # the component of largest magnitude is positive (an exact tie of two f32 magnitudes may hide which was first)
            assert V[k].max() > 0.0 and V[k].max() >= -V[k].min(), (what, s, k, V[k])
        assert np.abs(np.cross(V[0], V[1]) - V[2]).max() <= 1e-6, (what, s)
        assert np.abs(V.T @ np.diag(lam) @ V - S[s]).max() <= 2.0 ** -20 * tr, (what, s)
        if S_ref is None:
            continue
        wr, Vr = np.linalg.eigh(S_ref[s])
        wr, Vr = wr[::-1], Vr[:, ::-1].T
        gap = np.array([min(abs(wr[k] - wr[j]) for j in range(3) if j != k) for k in range(3)])
        sep = (gap >= 0.2 * wr[0]) & (wr[0] > 0.0)
        if need_all is not None and need_all[s]:
            assert sep.all(), (what, s, wr)
        for k in np.nonzero(sep)[0]:
            dot = abs(float(V[k] @ Vr[k]))
            worst = max(worst, 1.0 - dot)
            assert dot >= 1.0 - 1e-4, (what, s, k, dot)
    if S_ref is not None:
        print("gyration axes %s: max 1 - |v . v_ref| %.3g" % (what, worst))
