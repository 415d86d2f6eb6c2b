"""The hydrogen-bond yardstick (tests/hbond_ref.py) against every pin of the reference's hbond tests, on the CPU.

These pin the restatement the GPU tests compare against: counts, first and last bonds of the water frames (including the
frame-20 bond that exists only through handle_nan), the 181 bonds of the peptide trajectory and the protein-water pins of the
gro frame, in order; plus the topology fixture's integrity and the plan-time error variants."""
import os

import numpy as np
import pytest

import hbond_pins as P
import hbond_ref as R

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def full():
    return np.load(os.path.join(GOLD, "aa_full.npz"))


@pytest.fixture(scope="module")
def pep():
    return np.load(os.path.join(GOLD, "aa_peptide.npz"))


@pytest.fixture(scope="module")
def topo():
    return np.load(os.path.join(GOLD, "aa_hbond_topology.npz"))


def test_topology_fixture_integrity(topo, full):
    b, el = topo["peptide_bonds"], topo["peptide_element"]
    assert b.dtype == np.uint32 and b.shape == (362, 2) and el.dtype == np.dtype("S1") and el.shape == (363,)
    assert b.max() < 363 and (b[:, 0] != b[:, 1]).all()
    assert len({tuple(sorted(x)) for x in b.tolist()}) == 362                 # no bond twice
    assert set(el.tolist()) == {b"C", b"H", b"N", b"O"}
    assert (el == np.array([n[:1] for n in full["atomname"][:363]], "S1")).all()
    deg = np.bincount(b.ravel(), minlength=363)
    assert (deg[el == b"H"] == 1).all()                                       # every hydrogen has exactly one partner
    assert (deg >= 1).all()                                                   # one connected peptide: no isolated atom
    ow, hw, wb = R.water_topology(full["atomname"])
    assert len(hw) == 2 * len(ow) and wb.shape == (2 * len(ow), 2)


def _water(full, frame):
    ow, hw, bonds = R.water_topology(full["atomname"])
    nb = R.bonded(bonds, full["frames"].shape[1])
    chain = R.resolve_chain(ow, ow, hw, nb)
    return R.analyze(full["frames"][frame], full["boxes9"][frame], [chain], [(0, 0)], 0.3, 150.0)[(0, 0)]


@pytest.mark.parametrize("k", [0, 1])
def test_water_counts_first_and_last(full, k):
    bonds = _water(full, k)
    frame = int(full["frame_index"][k])
    assert len(bonds) == P.WATER_COUNTS[frame]
    assert R.close(bonds[0], P.WATER_FIRST_LAST[2 * frame]), bonds[0]
    assert R.close(bonds[-1], P.WATER_FIRST_LAST[2 * frame + 1]), bonds[-1]
    if frame == 20:   # the bond that exists only through handle_nan: the f32 cosine rounds below -1
        hit = [b for b in bonds if (b[0], b[1], b[2]) == (24613, 24614, 30592)]
        assert len(hit) == 1 and float(hit[0][4]) == 180.0


def test_protein_trajectory_181_pins(pep, topo):
    don, hyd = R.protein_groups(topo["peptide_element"])
    chain = R.resolve_chain(don, don, hyd, R.bonded(topo["peptide_bonds"], 363))
    got = []
    for f in range(pep["traj_peptide"].shape[0]):
        got += R.analyze(pep["traj_peptide"][f], pep["traj_boxes9"][f], [chain], [(0, 0)], 0.3, 150.0)[(0, 0)]
    assert len(got) == len(P.PROTEIN_TRAJ) == 181
    for g, w in zip(got, P.PROTEIN_TRAJ):
        assert R.close(g, w), (g, w)


def test_protein_water_gro_pins(pep, topo, full):
    ow, hw, wb = R.water_topology(full["atomname"])
    don, hyd = R.protein_groups(topo["peptide_element"])
    nb = R.bonded(np.concatenate([topo["peptide_bonds"].astype(np.int64), wb]), pep["pos"].shape[0])
    hs = np.concatenate([hyd, hw])          # "element name hydrogen" (the lipids' hydrogens bond to no donor of either chain)
    chains = [R.resolve_chain(don, don, hs, nb), R.resolve_chain(ow, ow, hs, nb)]
    out = R.analyze(pep["pos"], pep["box9"], chains, [(0, 0), (0, 1)], 0.3, 150.0)
    for key, want in (((0, 0), P.PROTEIN_PROTEIN_GRO), ((0, 1), P.PROTEIN_WATER_GRO)):
        assert len(out[key]) == len(want), (key, len(out[key]))
        for g, w in zip(out[key], want):
            assert R.close(g, w), (key, g, w)


@pytest.mark.parametrize("pairs, variant, payload", [
    ([(0, 1), (0, 2)], "NonexistentChain", 2),
    ([(0, 1), (0, 0), (0, 1)], "PairSpecifiedMultipleTimes", (0, 1)),
    ([(1, 0), (0, 0), (0, 1)], "PairSpecifiedMultipleTimes", (0, 1)),
    ([(0, 0), (1, 0), (0, 0)], "PairSpecifiedMultipleTimes", (0, 0)),
    ([(0, 0)], "UnusedChain", None),
])
def test_pair_checks(pairs, variant, payload):
    with pytest.raises(R.HBondRefError) as e:
        R.check_pairs(pairs, 2)
    assert e.value.variant == variant and e.value.payload == payload


def test_empty_chain():
    with pytest.raises(R.HBondRefError) as e:
        R.resolve_chain([], [0, 1], [5], R.bonded([(2, 3)], 6))
    assert e.value.variant == "EmptyChain"
