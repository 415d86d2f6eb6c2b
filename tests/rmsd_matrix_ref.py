"""Helpers shared by tests/test_gpu_rmsd_matrix.py and tests/test_gpu_rmsd_matrix_edges.py: the oracle's matrix (a double loop of
oracle_lib.calc_rmsd), bit comparison of f32 matrices (NaN included), systems with a trajectory in their slots, and the synthetic
trajectories of the edge tests."""
import numpy as np

import oracle_lib as O

F32 = np.float32
TOL = 1e-5                      # nm: the project's bar for an RMSD
BOX10 = np.array([10, 10, 10, 0, 0, 0, 0, 0, 0], F32)


def bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def oracle_matrix(rows, row_boxes, cols, col_boxes, masses, idx=None):
    """M[i, j] = oracle calc_rmsd(reference = column frame j, current = row frame i) over the atoms `idx` (default: all)"""
    idx = np.arange(rows[0].shape[0]) if idx is None else idx
    M = np.zeros((len(rows), len(cols)), np.float64)
    for i in range(len(rows)):
        for j in range(len(cols)):
            M[i, j] = O.calc_rmsd(cols[j], masses, idx, col_boxes[j], rows[i], masses, idx, row_boxes[i])[0]
    return M


def system_with(G, frames, boxes, masses, n_slots=None):
    """a System whose slot f holds frames[f] / boxes[f]"""
    s = G.System(frames[0].shape[0], masses=masses, n_slots=n_slots or len(frames))
    for f in range(len(frames)):
        s.set_frame(frames[f], boxes[f], slot=f)
    return s


def matrix_of(G, s, group, slots, pieces=None, **kw):
    """the matrix of the frames in `slots` (any order), appended in runs of consecutive slots (or `pieces` slots per call at most)"""
    p = G.RMSDPanel(s, group, len(slots))
    k = 0
    while k < len(slots):
        n = 1
        while k + n < len(slots) and slots[k + n] == slots[k] + n and (pieces is None or n < pieces):
            n += 1
        p.append(slots[k], n)
        k += n
    M = G.rmsd_matrix(p, **kw)
    p.close()
    return M


def synthetic(n_atoms, n_frames, seed, sigma=0.6, noise=0.05):
    """-> (frames [F, N, 3] f32 wrapped into the 10 nm cube, masses f32 [N]).  A seeded base structure within 3 nm of its centre,
    per-frame Gaussian noise of 0.05 nm and a random translation anywhere in the box -- so most frames are broken by the wrap.  After the
    shift of its centre of mass to the box centre every atom must stay more than 1e-3 nm clear of every cell face (asserted here, in
    f64, on the unwrapped coordinates): a 1-ulp difference in the centre cannot then flip an image."""
    rng = np.random.default_rng(seed)
    base = rng.normal(0.0, sigma, (n_atoms, 3))
    r = np.linalg.norm(base, axis=1, keepdims=True)
    base *= np.minimum(1.0, 3.0 / np.maximum(r, 1e-12))
    masses = rng.uniform(1.0, 32.0, n_atoms).astype(F32)
    frames = np.zeros((n_frames, n_atoms, 3), F32)
    for f in range(n_frames):
        x = base + rng.normal(0.0, noise, (n_atoms, 3))
        com = (x * masses[:, None].astype(np.float64)).sum(0) / masses.astype(np.float64).sum()
        c = x - com + 5.0
        assert c.min() > 1e-3 + 0.01 and c.max() < 10.0 - 1e-3 - 0.01, (n_atoms, f, c.min(), c.max())      # (0.01: the f32 rounding of the frame itself)
        frames[f] = np.mod(x + rng.uniform(0.0, 10.0, 3), 10.0).astype(F32)
    frames[frames >= F32(10.0)] = F32(0.0)
    return frames, masses
