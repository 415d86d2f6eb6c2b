"""tests/history_world.py on the CPU: the schedules contain every kind, the mandatory adjacencies in order and a failing kind of the
own and of another family directly in front of every non-failing kind; the host-side world has the hydrogen bonds and the broken
molecules that the GPU history tests (test_gpu_history.py) rely on, and what the kinds of the family "series" and the gyration kinds
need: the three snapshot forms, dihedrals away from flat bends, eigenvalue gaps of the `sizes` segments, unambiguous MSD steps."""
import numpy as np
import pytest

import gyration_ref
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
    "fluct_small_8", "fluct_masked_16", "fluct_list_tric_8", "fluct_two_calls", "covar_small_16", "covar_a300_tric_8",
    "msd_small_ortho_8", "msd_masked_tric_8", "msd_appended_in_three", "vcorr_ortho_8", "vcorr_tric_8",
    "internals_distance_16", "internals_angle_16", "internals_dihedral_8", "internals_accumulate_16", "panel_big_16", "panel_big_small_cols", "panel_device",
    "gyr_mol_9_axes", "gyr_resid_2", "gyr_sizes_16_axes", "gyr_mol_9_pieces", "gyr_sizes_device_4",
    "fail_fluct_nan", "fail_msd_nobox", "fail_covar_all_bad", "fail_vcorr_nan", "fail_internals_nan", "fail_panel_nan", "fail_msd_capacity", "fail_panel_masses",
    "fail_gyr_mixed",
]
N_KINDS_BEFORE_SERIES, N_SERIES_KINDS = 100, 32          # the floor of the table before the series objects and gyration joined it, and the kinds they added


def test_the_kinds_the_history_tests_need_exist():
    assert not [k for k in REQUIRED if k not in HW.KINDS]
    assert len(REQUIRED) == len(set(REQUIRED)) and len(HW.KINDS) >= N_KINDS_BEFORE_SERIES + N_SERIES_KINDS and set(HW.META) == set(HW.KINDS)
    assert sorted(HW.ADJACENCIES) == list(range(1, 20)) and all(k in HW.KINDS for a in HW.ADJACENCIES.values() for k in a)
    families = set(m["family"] for m in HW.META.values())
    assert families == {"centres", "rmsd", "pairs", "topology", "io", "redef", "series"}
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


def _snapshot_form(atoms):
    """GrSnapshot::build of csrc/gr_series.h: 0 a contiguous run, 2 a masked span (at least every second atom of it), 1 an index list"""
    n, span = len(atoms), int(atoms[-1] - atoms[0] + 1)
    return 0 if span == n else 2 if 2 * n >= span else 1


def _periodic_centre(x, H):
    """the centre of atoms that cover less than half of every cell vector: the circular mean of the fractional coordinates"""
    a = 2 * np.pi * (x @ np.linalg.inv(H))
    return (np.arctan2(np.sin(a).mean(0), np.cos(a).mean(0)) / (2 * np.pi) % 1.0) @ H


def test_the_world_of_the_series_kinds():
    """what the kinds of the family "series" and the gyration kinds rely on, from the host frames alone"""
    h, t = HW.host_world(), HW.series_tuples()
    g = h["groups"]
    # Fluctuations runs all three forms of GrSnapshot / k_fl_check
    assert [_snapshot_form(g[name]) for name in ("small", "masked", "list")] == [0, 2, 1] and g["small"][0] % 4 != 0
    assert 3 * len(g["small"]) <= 1100 and 3 * len(g["a300"]) <= 1100                  # Covariance: D = 3 S stays near 1 000
    assert HW.NAN_SMALL in g["small"] and HW.NAN_BIG in g["big"] and 310 in g["a300"] and 599 in g["a300"]
    assert HW.NAN_SERIES in t["pairs"][:, 1] and HW.NAN_SERIES in t["angles"][:, 0]
    assert len(t["pairs"]) == len(t["angles"]) == len(HW.SERIES_MOLS) == 401 and max(HW.SERIES_CAPACITY, HW.PANEL_SMALL_CAPACITY) <= 16
    # the dihedrals H2-O...O'-H2': those whose bend angles come near 0 or 180 degrees in some frame are left out, and enough remain
    d = 3 * h["donors"].astype(np.int64)
    every = np.stack([d + 2, d, d + 3, d + 5], 1)
    keep = (HW.bend_sines(every) >= HW.DIHEDRAL_MIN_SINE).all(axis=(0, 2))
    assert np.array_equal(t["dihedrals"], every[keep].astype(np.uint64)) and 200 <= len(t["dihedrals"]) < len(every)
    assert HW.bend_sines(t["dihedrals"]).min() >= HW.DIHEDRAL_MIN_SINE
    on_line = HW.bend_sines(np.stack([d + 1, d, d + 3, d + 5], 1))[:, :, 0]             # with H1 in place of H2 the first bend is flat: that dihedral is degenerate
    assert on_line.max() < 0.2
    # the segments of seg["sizes"]: consecutive atoms, one size per team class
    assert [len(l) for l in t["sizes"]] == list(HW.SIZES) and np.array_equal(np.concatenate(t["sizes"]), np.arange(sum(HW.SIZES)))
    assert HW.NAN_BIG // 3 < HW.N_MOL and sum(HW.SIZES) < HW.N
    # ... and their principal axes.  The water lattice does not separate all three eigenvalues by 0.2 lambda_1 (the condition under which
    # gyration_ref.check_axes compares a direction): the 65 and the 257 atoms are a few rows of the lattice (a rod: only the long axis
    # stands apart), the 4 097 are a slab of layers (only the short axis does).  So the GPU test compares the directions where the
    # condition holds, as test_gpu_gyration.py does, and this test says where that is: the same axis in every frame
    for f in range(HW.N_FRAMES):
        H = HW.cell(h["boxes"][f])
        x = h["frames"][f].astype(np.float64)
        centres = np.stack([_periodic_centre(x[l.astype(np.int64)], H) for l in t["sizes"]])
        S, margin = gyration_ref.reference(h["frames"][f], h["boxes"][f], h["masses"], t["sizes"], centres, HW.PBC, True)
        assert not np.isnan(S).any() and np.abs(S[0]).max() == 0.0
        for s, want in ((3, [True, False, False]), (4, [True, False, False]), (5, [False, False, True])):
            w = np.linalg.eigvalsh(S[s])[::-1]
            gap = np.array([min(abs(w[k] - w[j]) for j in range(3) if j != k) for k in range(3)])
            assert (gap >= 0.2 * w[0]).tolist() == want, (f, s, w)
    # MSD: between consecutive frames of a cell no atom of its groups moves further than a quarter of the shortest box height once the
    # periodic jump is taken off, so the reference's unwrapping (msd_ref.Walk) is unambiguous -- and some atoms do jump
    for slots, group in ((HW.ORTHO8, "small"), (HW.TRIC8, "masked"), (HW.ORTHO8, "masked")):
        H = HW.cell(h["boxes"][slots[0]])
        height = min(abs(np.linalg.det(H)) / np.linalg.norm(np.cross(H[(k + 1) % 3], H[(k + 2) % 3])) for k in range(3))
        jumped = 0
        for a, b in zip(slots[:-1], slots[1:]):
            raw = h["frames"][b][g[group]].astype(np.float64) - h["frames"][a][g[group]].astype(np.float64)
            step = raw - np.round(raw @ np.linalg.inv(H)) @ H
            assert np.linalg.norm(step, axis=1).max() <= height / 4, (group, a, b)
            jumped += int((np.abs(raw - step).max(axis=1) > 1.0).sum())
        assert jumped > 0, group
    # the failing kinds of the family fail in more than one way: positions, boxes, capacity, masses
    fails = [k for k, m in HW.META.items() if m["family"] == "series" and m["failing"]]
    assert len(fails) >= 4 and {"fail_fluct_nan", "fail_msd_nobox", "fail_msd_capacity", "fail_panel_masses"} <= set(fails)
    series = [k for k, m in HW.META.items() if m["family"] == "series" or k.startswith("gyr_") or k == "fail_gyr_mixed"]
    assert len(series) == N_SERIES_KINDS and all(HW.META[k]["family"] == "topology" for k in series if "gyr_" in k)


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
