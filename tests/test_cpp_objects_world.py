"""What tests/test_gpu_cpp_objects.py relies on and what can be checked without a GPU: the world of cpp_objects_world.py keeps every
atom clear of every decision point of the call script (so no case has to be left out of a comparison), and tests/cpp/test_objects.cpp
compiles against the header without a warning."""
import os
import subprocess

import numpy as np
import pytest

import cpp_objects_world as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def world():
    return W.build()


def test_no_atom_sits_on_a_decision_point(world):
    """seen by the references alone: no result of a reference changes when a shape surface, a Contacts cut-off, the hydrogen-bond
    distance or a GridMap tile edge moves by 1e-4 nm either way, or the hydrogen-bond angle by 0.1 degree; no periodic centre lies
    within SEAM of a cell face"""
    fr, bx = world["frames"], world["boxes"]
    assert (W.MARGIN_NM, W.MARGIN_DEG) == (1e-4, 0.1)
    assert W.violations(fr, bx, W.MARGIN_NM, W.MARGIN_DEG) == set()
    assert W.seam_flags(fr, bx, world["masses"]) == 0
    # ... and the check can see: with margins of the size of the world itself it finds atoms on every kind of decision point
    assert len(W.violations(fr, bx, 0.05, 20.0, slots=[0])) > 50


def test_the_world_is_the_one_the_script_needs(world):
    fr, bx = world["frames"], world["boxes"]
    assert len(fr) == len(bx) == W.NS and all(x.shape == (W.N, 3) and x.dtype == np.float32 for x in fr)
    nan = [f for f in range(W.NS) if np.isnan(fr[f]).any()]
    assert nan == [W.NAN_SLOT] and np.isnan(fr[W.NAN_SLOT]).any(axis=1).nonzero()[0].tolist() == [W.NAN_ATOM]
    assert [f for f in range(W.NS) if bx[f] is None] == [W.NOBOX_SLOT] and 0 < W.NAN_SLOT < W.NS - 1 and 0 < W.NOBOX_SLOT < W.NS - 1
    assert all(W.NAN_ATOM in W.GROUPS[g] for g in ("rng", "lst", "hyd", "hydA")) and W.NAN_ATOM in W.SEG_LISTS[2]
    assert W.GROUPS["rng"][0] % 4 != 0 and 3 * W.GROUPS["lst"].size + 1 > 64
    # the same seed, the same world: the GPU test and the program it starts see identical bytes
    again = W.build()
    assert all(a.tobytes() == b.tobytes() for a, b in zip(fr, again["frames"])) and world["masses"].tobytes() == again["masses"].tobytes()
    # every hydrogen-bond pair finds bonds somewhere, the plan with the short distance none
    found = {p: 0 for p in W.HB_PAIRS}
    for f in range(W.NS):
        for p, bonds in W.hbonds_of(fr[f], bx[f], W.HB_DIST, W.HB_ANGLE)[0].items():
            found[p] += len(bonds)
        assert not any(W.hbonds_of(fr[f], bx[f], W.HB_DIST_NONE, W.HB_ANGLE)[0].values())
    assert all(n > 0 for n in found.values())


def test_fixture_files_round_trip(world, tmp_path):
    W.write(world, str(tmp_path))
    frames = np.fromfile(tmp_path / "frames.f32", "<f4").reshape(W.NS, W.N, 3)
    boxes = np.fromfile(tmp_path / "boxes.f32", "<f4").reshape(W.NS, 9)
    assert frames.tobytes() == np.stack(world["frames"]).tobytes()
    assert [bool(np.isnan(b[0])) for b in boxes] == [b is None for b in world["boxes"]]
    assert np.fromfile(tmp_path / "meta.u64", "<u8").tolist() == [W.N, W.NS, W.NAN_SLOT, W.NOBOX_SLOT, W.NAN_ATOM]
    assert np.array_equal(np.fromfile(tmp_path / "group_hyd.u64", "<u8"), W.GROUPS["hyd"]) and not os.path.exists(tmp_path / "group_rng.u64")
    assert np.fromfile(tmp_path / "bonds.u64", "<u8").size == 2 * len(W.BONDS)


def test_objects_program_compiles_without_a_warning():
    src = os.path.join(ROOT, "tests", "cpp", "test_objects.cpp")
    p = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"), src],
                       capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
