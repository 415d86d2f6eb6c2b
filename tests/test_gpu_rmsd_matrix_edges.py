"""RMSDPanel / rmsd_matrix at the smallest shapes at which the product kernel can still go wrong.

The kernel's tile is 8 row frames x 16 column frames (a 48 x 48 block of the product, 3 x 3 MFMA tiles); a wave walks the atoms in
trips of 16 (rows are zero-padded to that) and the four waves of a workgroup share the trips of a block in turn, so 64 atoms are one
round of the workgroup.  No length of the atom loop is special beyond that -- a workgroup walks any N -- so the "largest K" case of the
frame sweep is simply N = 4 099 (65 rounds and a ragged trip).

Inputs (rmsd_matrix_ref.synthetic): a seeded base structure in a 10 nm cube, 0.05 nm of noise per frame, a random translation anywhere in
the box (most frames are broken by the wrap), seeded masses; every atom stays clear of the cell faces after centring, asserted there.
Every entry is compared with the oracle at 1e-5 nm (its f64 accumulation above 1 000 atoms), and with the entry the same two frames
have in any other panel, bit for bit."""
import numpy as np
import pytest

import oracle_lib as O
from rmsd_matrix_ref import BOX10, TOL, matrix_of, oracle_matrix, same_bits, synthetic, system_with

pytestmark = pytest.mark.gpu
F = np.float32
FRAME_COUNTS = [1, 7, 8, 9, 15, 16, 17, 33]                 # below, at and above the 8- and the 16-frame edge; three column blocks
ATOM_COUNTS = [3, 4, 5, 15, 16, 17, 63, 64, 65, 363, 4099]   # the 16-atom trip, the 64-atom round, a ragged end, many rounds


@pytest.fixture(scope="module")
def G():
    import groan_rs_amd as g
    g._lib.load()
    return g


def make(G, n_atoms, n_frames, seed):
    frames, masses = synthetic(n_atoms, n_frames, seed)
    s = system_with(G, list(frames), [BOX10] * n_frames, masses)
    return s, frames, masses


def oracle(frames, masses, rows, cols):
    a, b = [frames[f] for f in rows], [frames[f] for f in cols]
    if frames.shape[1] > 1000:
        with O.acc64():
            return oracle_matrix(a, [BOX10] * len(a), b, [BOX10] * len(b), masses)
    return oracle_matrix(a, [BOX10] * len(a), b, [BOX10] * len(b), masses)


@pytest.fixture(scope="module")
def w65(G):
    """33 frames of 65 atoms, the oracle's 33 x 33 matrix and the library's"""
    s, frames, masses = make(G, 65, 33, 65)
    want = oracle(frames, masses, range(33), range(33))
    full = matrix_of(G, s, "all", list(range(33)))
    yield dict(s=s, want=want, full=full)
    s.close()


@pytest.mark.parametrize("nf", FRAME_COUNTS)
def test_frame_counts_one_panel(G, w65, nf):
    M = matrix_of(G, w65["s"], "all", list(range(nf)))
    assert M.shape == (nf, nf) and np.array_equal(M, M.T)
    err = np.abs(M - w65["want"][:nf, :nf]).max()
    print("F = %d, N = 65: max |M - oracle| = %.3g nm" % (nf, err))
    assert err <= TOL
    assert same_bits(M, w65["full"][:nf, :nf])                # the neighbours in the tile do not matter


@pytest.mark.parametrize("nf", FRAME_COUNTS)
def test_frame_counts_two_panels(G, w65, nf):
    """rows: the last nf frames, columns: the first nf -- and the unequal 9 x 17 / 17 x 9 pairs below"""
    s = w65["s"]
    rows, cols = G.RMSDPanel(s, "all", nf), G.RMSDPanel(s, "all", nf)
    rows.append(33 - nf, nf); cols.append(0, nf)
    M = G.rmsd_matrix(rows, cols)
    assert np.abs(M - w65["want"][33 - nf:, :nf]).max() <= TOL
    assert same_bits(M, w65["full"][33 - nf:, :nf])
    rows.close(); cols.close()


@pytest.mark.parametrize("nr,nc", [(9, 17), (17, 9), (1, 33), (33, 1)])
def test_unequal_panels(G, w65, nr, nc):
    s = w65["s"]
    rows, cols = G.RMSDPanel(s, "all", nr), G.RMSDPanel(s, "all", nc)
    rows.append(0, nr); cols.append(33 - nc, nc)
    M = G.rmsd_matrix(rows, cols)
    assert M.shape == (nr, nc) and np.abs(M - w65["want"][:nr, 33 - nc:]).max() <= TOL
    assert same_bits(M, w65["full"][:nr, 33 - nc:])
    rows.set_block_entries(nr * 16)                           # the host form in column blocks
    assert same_bits(G.rmsd_matrix(rows, cols), M)
    rows.close(); cols.close()


@pytest.mark.parametrize("n_atoms", ATOM_COUNTS)
def test_atom_counts(G, n_atoms):
    s, frames, masses = make(G, n_atoms, 17, 1000 + n_atoms)
    want = oracle(frames, masses, range(17), range(17))
    M = matrix_of(G, s, "all", list(range(17)))
    err = np.abs(M - want).max()
    print("F = 17, N = %d: max |M - oracle| = %.3g nm (rmsd %.3g .. %.3g)" % (n_atoms, err, want[want > 0].min(), want.max()))
    assert np.array_equal(M, M.T) and err <= TOL
    rows, cols = G.RMSDPanel(s, "all", 9), G.RMSDPanel(s, "all", 8)
    rows.append(8, 9); cols.append(0, 8)
    assert same_bits(G.rmsd_matrix(rows, cols), M[8:, :8])
    s.close()


@pytest.mark.parametrize("n_atoms", [1, 2])
def test_rank_deficient_groups(G, n_atoms):
    """H has rank 0 / 1: finite values, within 1e-5 nm of gr_calc_rmsd of the same pair (the oracle is not consulted)"""
    s, frames, masses = make(G, n_atoms, 9, 2000 + n_atoms)
    M = matrix_of(G, s, "all", list(range(9)))
    assert np.isfinite(M).all() and np.array_equal(M, M.T)
    for i in range(9):
        for j in range(9):
            assert abs(M[i, j] - s.calc_rmsd(s, "all", slot=i, ref_slot=j)) <= TOL, (i, j)
    s.close()


def test_near_zero_rmsd(G):
    """the same frame three times and a copy moved by a whole box vector: the cancellation that f32 sums fail (1e-4 nm)"""
    frames, masses = synthetic(363, 1, 77)
    x = frames[0]
    moved = x.copy(); moved[:, 1] += F(10.0)
    s = system_with(G, [x, x, moved, x], [BOX10] * 4, masses)
    M = matrix_of(G, s, "all", [0, 1, 2, 3])
    print("near-zero: max entry = %.3g nm" % M.max())
    assert M.shape == (4, 4) and np.isfinite(M).all() and M.max() <= TOL
    s.close()


@pytest.mark.parametrize("shape", ["every_third", "two_blocks"])
def test_scattered_group_gives_the_bits_of_the_contiguous_one(G, shape):
    n = 65
    frames, masses = synthetic(3 * n + 40, 9, 3000)
    idx = np.arange(0, 3 * n, 3) if shape == "every_third" else np.concatenate([np.arange(5, 30), np.arange(3 * n, 3 * n + 40)])
    assert idx.size == n
    big = system_with(G, list(frames), [BOX10] * 9, masses)
    big.group_create_from_indices("Sel", idx)
    small = system_with(G, [x[idx] for x in frames], [BOX10] * 9, masses[idx])
    A, B = matrix_of(G, big, "Sel", list(range(9))), matrix_of(G, small, "all", list(range(9)))
    assert same_bits(A, B)
    want = oracle_matrix(list(frames), [BOX10] * 9, list(frames), [BOX10] * 9, masses, idx)
    assert np.abs(A - want).max() <= TOL
    big.close(); small.close()
