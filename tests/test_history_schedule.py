"""tests/history_world.py on the CPU: the schedules contain every kind, the mandatory adjacencies in order and a failing kind of the
own and of another family directly in front of every non-failing kind; the host-side world has the hydrogen bonds and the broken
molecules that the GPU history tests (test_gpu_history.py) rely on."""
import numpy as np
import pytest

import hbond_ref
import history_world as HW
import whole_ref

REQUIRED = [
    "center_small_00", "center_big_21", "center_masked_11", "center_batch_small_20", "center_batch_big_01", "center_batch_masked_21", "group_distance",
    "atoms_center_small", "atoms_center_mass_big", "atoms_center_batch_res", "atoms_center_batch_two", "atoms_center_mass_batch_res",
    "translate_batch_ortho_rows1", "translate_batch_ortho_rows0", "translate_batch_tric", "wrap_batch_ortho_rows1", "wrap_batch_ortho_rows0", "wrap_batch_tric",
    "calc_rmsd_small", "calc_rmsd_fit_small", "plan_rmsd_all", "plan_rmsd_big", "plan_rmsd_masked", "plan_rmsd_listbig", "plan_fit_all_fuse0", "plan_fit_all_fuse1",
    "plan_fit_big_fuse1", "plan_fit_masked_fuse0", "plan_fit_listbig_fuse1", "res_fit_3", "res_fit_9", "res_fit_2", "plan_begin_end",
    "atoms_distance", "alldist_40x50", "alldist_300x400", "alldist_masked_self", "alldist_batch_device_40x50", "reduce_max", "reduce_min_rows", "reduce_count_rows",
    "reduce_hist", "iter_all_distances", "pairs_within", "geometries_small_all_small",
    "contacts_pairs_8", "contacts_hist_tric_8", "contacts_counts_1", "region_select_16", "region_anchored_8",
    "whole_mols", "whole_group_big", "rebond_whole", "seg_mol_2", "seg_mol_9", "seg_mol_1", "seg_resid_2", "seg_resid_9", "seg_resid_1", "hbond_2", "hbond_8", "hbond_1", "gridmap",
    "xtc_write_4", "xtc_write_12", "xtc_read_small", "xtc_read_full", "xtc_read_masked", "trr_read", "xtc_read_full_again", "xtc_read_small_redefined",
    "fail_translate_nan_small", "fail_com_nan_big", "fail_translate_nan_tail", "fail_center_nobox", "fail_center_batch_mixed", "fail_fit_mixed_fused", "fail_center_nogroup",
    "fail_alldist_skewed", "fail_contacts_nan", "fail_xtc_range", "fail_seg_nobox",
    "fail_redefined_small_plan", "restored_small_plan", "masses_changed", "tune_small_calls0", "tune_pairsym0", "tune_masked0",
]


def test_the_kinds_the_history_tests_need_exist():
    assert not [k for k in REQUIRED if k not in HW.KINDS]
    assert len(HW.KINDS) >= 100 and set(HW.META) == set(HW.KINDS)
    assert sorted(HW.ADJACENCIES) == list(range(1, 11)) and all(k in HW.KINDS for a in HW.ADJACENCIES.values() for k in a)
    families = set(m["family"] for m in HW.META.values())
    assert families == {"centres", "rmsd", "pairs", "topology", "io", "redef"}
    for fam in families:                                                   # every family can fail, and fail in more than one way
        assert sum(1 for m in HW.META.values() if m["family"] == fam and m["failing"]) >= 2, fam


@pytest.mark.parametrize("seed", [0, 1])
def test_schedule(seed):
    sched = HW.schedule(seed)
    assert sched == HW.schedule(seed) and all(k in HW.KINDS for k in sched)
    assert set(sched) == set(HW.KINDS)
    head = HW.mandatory()
    assert sched[:len(head)] == head
    at = 0
    for a in sorted(HW.ADJACENCIES):                                       # each adjacency stands as a block, in order
        assert sched[at:at + len(HW.ADJACENCIES[a])] == HW.ADJACENCIES[a]
        at += len(HW.ADJACENCIES[a])
    tail = sched[len(head):]
    for name in HW.KINDS:
        assert tail.count(name) >= 2, name
    own, other = set(), set()
    for before, name in zip(sched[:-1], sched[1:]):
        if HW.META[before]["failing"] and not HW.META[name]["failing"]:
            (own if HW.META[before]["family"] == HW.META[name]["family"] else other).add(name)
    good = set(k for k in HW.KINDS if not HW.META[k]["failing"])
    assert own == good and other == good, (sorted(good - own), sorted(good - other))
    assert HW.schedule(0) != HW.schedule(1)


def test_the_groups_take_the_paths_they_are_named_for():
    g = HW.host_world()["groups"]
    assert HW.N == 12003 and HW.N % 4 == 3 and HW.N % 256 != 0 and HW.N_MOL * 3 == HW.N
    assert len(g["small"]) == 363 and g["small"][0] % 4 != 0 and len(g["small"]) <= 4096
    assert len(g["big"]) == 5000 and np.all(np.diff(g["big"]) == 1)
    span = g["masked"][-1] - g["masked"][0] + 1
    assert len(g["masked"]) >= 4096 and len(g["masked"]) * 8 >= span and np.array_equal(g["masked"], g["listbig"])
    assert np.all(np.diff(g["list"]) == 7)
    assert HW.NAN_SMALL in g["small"] and HW.NAN_BIG in g["big"] and HW.NAN_TAIL // 4 == (HW.N - 1) // 4 and HW.NAN_A40 in g["a40"]
    assert HW.N * 20 >= 200_000 and HW.N * 24 >= 200_000 and HW.N * 16 < 200_000      # the writer's spool passes the device encoder's threshold, 16 slots would not


def test_every_frame_has_hydrogen_bonds_and_broken_molecules():
    h = HW.host_world()
    nb = hbond_ref.bonded(h["bonds"], HW.N)
    # the bonds among the 800 molecules placed in pairs: a lower bound of the frame's bonds (the oracle's triclinic all-pairs search
    # over all 4 001 oxygens takes 16 s a frame)
    placed = 3 * np.sort(np.concatenate([h["donors"], h["donors"] + 1]))
    chain = hbond_ref.resolve_chain(placed, placed, h["groups"]["hyd"], nb)
    assert len(chain[1]) == 2 * HW.N_HB_PAIRS
    nbrs = whole_ref.neighbours(HW.N, h["bonds"])
    refs, orders = whole_ref.molecules(nbrs)
    assert len(refs) == HW.N_MOL
    ref_of = whole_ref.ref_of(HW.N, refs, orders)
    for f in range(HW.N_FRAMES + 1):
        pos, box = h["frames"][f], h["boxes"][f]
        assert pos.shape == (HW.N, 3) and pos.dtype == np.float32 and np.isfinite(pos).all()
        bonds = hbond_ref.analyze(pos, box, [chain], [(0, 0)], HW.HB_DISTANCE, HW.HB_ANGLE)[(0, 0)]
        assert len(bonds) >= 100, (f, len(bonds))
        if len(box) == 3:
            whole, bad = whole_ref.make_molecules_whole(pos, box, ref_of, orders)
            assert bad is None
            moved = np.abs(whole - pos).max(axis=1) > 1.0
        else:                                                              # (whole_ref is orthorhombic: a bond longer than 1 nm is a broken one)
            o = np.repeat(pos[0::3], 3, axis=0)
            moved = np.linalg.norm(pos - o, axis=1) > 1.0
        broken = int(moved.reshape(HW.N_MOL, 3).any(axis=1).sum())
        assert 0.07 * HW.N_MOL <= broken <= 0.15 * HW.N_MOL, (f, broken)
