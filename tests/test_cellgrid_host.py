"""Host-side checks of the cell grid's geometry (groan_rs_amd/csrc/gr_cellgrid.h), without a GPU: the scan of every cell border for
pairs within the cut-off that the grid would put two cells apart (tests/cpp/test_cellgrid.cpp), and the numpy restatement that the GPU
tests place their atoms with (tests/cellgrid_ref.py) against the C++ functions, bit for bit."""
import os
import subprocess

import numpy as np

import cellgrid_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")
F = np.float32


def program():
    subprocess.check_call(["make", "-C", CPP, "test_cellgrid"])
    return os.path.join(CPP, "test_cellgrid")


def test_no_pair_within_the_cutoff_is_two_cells_apart():
    """every cell border of ~9 000 cubic boxes on the steps of floor(L / cs), beyond the 1024-cell clamp, of ordinary and of the three
    named boxes, and of five triclinic cells: 0 violating pairs with gr_cellgrid_make, and more than 0 with the control (a cell
    1.00001 x cutoff thick), which shows that the scan can fail"""
    p = subprocess.run([program()], capture_output=True, text=True, timeout=600)
    print(p.stdout, p.stderr)
    assert p.returncode == 0 and "PASS" in p.stdout
    assert "gr_cellgrid_make: 0 violating pairs" in p.stdout
    control = [l for l in p.stdout.splitlines() if l.startswith("control (")]
    assert len(control) == 1 and int(control[0].split(":")[1].split()[0]) > 0
    # the smallest d - cutoff among the pairs two cells apart, per cut-off and family of boxes: positive with gr_cellgrid_make (above the
    # 2e-6 nm that a borderline pair is granted in triclinic cells), negative somewhere with the control
    lines = p.stdout.splitlines()
    split = lines.index("== gr_cellgrid_make")
    margin = lambda l: float(l.split("margin")[1].split(",")[0])
    mine = [l for l in lines[split:] if "margin" in l]
    assert len(mine) >= 9 + 3 + 15
    assert all(margin(l) > (-2e-6 if "triclinic" in l else 0.0) for l in mine), [l for l in mine if margin(l) <= 0.0]
    assert min(margin(l) for l in lines[:split] if "margin" in l) < 0.0
    named = [l for l in p.stdout.splitlines() if "x_i" in l]
    assert len(named) == 6 and all("two cells apart" in l for l in named[:3]) and not any("two cells apart" in l for l in named[3:])


def test_numpy_restatement_gives_the_same_cells():
    p = subprocess.run([program(), "--dump"], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0
    rows = np.array([[int(w, 16) for w in l.split()[:3]] + [int(w) for w in l.split()[3:]] for l in p.stdout.splitlines()], np.uint64)
    assert rows.shape[0] > 3000
    L, cutoff, x = (rows[:, q].astype(np.uint32).view(F) for q in range(3))
    bad = 0
    for key in {(a, b) for a, b in zip(rows[:, 0], rows[:, 1])}:
        m = (rows[:, 0] == key[0]) & (rows[:, 1] == key[1])
        n, _ = R.cells(L[m][0], cutoff[m][0])
        assert n == int(rows[m][0, 3]), (L[m][0], cutoff[m][0], n, int(rows[m][0, 3]))
        got = R.cell(x[m], L[m][0], cutoff[m][0])
        bad += int((got != rows[m][:, 4].astype(np.int64)).sum())
    assert bad == 0


def test_borders_and_steps_of_the_restatement():
    """border(): the float below it is binned one cell lower; step_length(): one float below it the axis has one cell fewer"""
    for L, cutoff in ((41.25042, 0.25), (7.25, 0.5), (400.0, 0.3)):
        n, _ = R.cells(L, cutoff)
        for m in (1, 2, n // 2, n - 1):
            w = R.border(L, cutoff, m)
            assert R.cell(w, L, cutoff) == m and R.cell(np.nextafter(w, F(0)), L, cutoff) == m - 1
    assert R.cells(400.0, 0.3)[0] == 1024
    for cutoff in (0.25, 0.5, 1.2):
        for k in (2, 3, 4, 165, 1024):
            s = R.step_length(cutoff, k)
            assert R.cells(s, cutoff)[0] == k and R.cells(np.nextafter(s, F(0)), cutoff)[0] == k - 1
    # the expectations that tests of the consumers rest on: 0.9 nm is one cell and 1.6 nm three at a cut-off of 0.5 nm
    assert R.grid([0.9, 0.9, 0.9], 0.5) == (1, 1, 1) and R.grid([1.6, 1.6, 1.6], 0.5) == (3, 3, 3)
