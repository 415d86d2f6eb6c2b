#!/usr/bin/env python3
"""Generate tests/golden/whole_fixture.npz: the inputs and known answers of the make-whole tests.

Run in the build container only (reads the reference's DATA files test_files/conect.pdb, multiple_molecules_conect.pdb,
whole_molecules_expected.gro and whole_group_expected.gro):

    python tests/golden/make_whole_fixture.py

Outputs (numpy .npz, data only), for P in (conect, multi) = conect.pdb, multiple_molecules_conect.pdb:
  P_pos        float32 [50, 3]  positions as the pdb reader makes them: the f32 value of the field / 10
  P_box        float32 [3]      CRYST1 lengths / 10 (both cells are rectangular)
  P_serial     uint32 [50]      atom numbers (serials) in file order: both files list serial 10 between 28 and 29
  P_bonds      uint32 [k, 2]    0-based (atom, partner) index pairs of the CONECT records, as written; serials are mapped to
                                indices as the reader does (atom_number_to_index, pdb_io.rs:150-154)
  whole_molecules_lines / whole_group_lines   str [53]   the lines of the two expected gro files
Known answers that are lists of numbers (BFS orders, molecule references) live in tests/test_topology_host.py next to the
reference line that pins them.
"""
import os

import numpy as np

REF = os.environ.get("GROAN_REFERENCE", "/root/reference")
TF = os.path.join(REF, "test_files")
HERE = os.path.dirname(os.path.abspath(__file__))


def read_pdb(name):
    pos, bonds, box, index = [], [], None, {}
    with open(os.path.join(TF, name)) as fh:
        for line in fh:
            if line.startswith(("ATOM", "HETATM")):
                serial = int(line[6:11])
                index[serial] = len(pos)
                pos.append([np.float32(line[c:c + 8].strip()) / np.float32(10.0) for c in (30, 38, 46)])
            elif line.startswith("CRYST1"):
                box = [np.float32(line[c:c + 9].strip()) / np.float32(10.0) for c in (6, 15, 24)]
                assert [float(line[c:c + 7]) for c in (33, 40, 47)] == [90.0, 90.0, 90.0]
            elif line.startswith("CONECT"):
                a = index[int(line[6:11])]
                k = 11
                while k + 4 < len(line.rstrip("\n")):
                    t = line[k:k + 5].strip()
                    if t:
                        bonds.append((a, index[int(t)]))
                    k += 5
    serials = sorted(index, key=index.get)
    return np.asarray(pos, np.float32), np.asarray(box, np.float32), np.asarray(bonds, np.uint32), np.asarray(serials, np.uint32)


def main():
    out = {}
    for key, name in (("conect", "conect.pdb"), ("multi", "multiple_molecules_conect.pdb")):
        pos, box, bonds, serials = read_pdb(name)
        assert pos.shape == (50, 3) and bonds.max() < 50 and len(set(serials.tolist())) == 50
        out[key + "_pos"], out[key + "_box"], out[key + "_bonds"], out[key + "_serial"] = pos, box, bonds, serials
    for key, name in (("whole_molecules_lines", "whole_molecules_expected.gro"), ("whole_group_lines", "whole_group_expected.gro")):
        with open(os.path.join(TF, name)) as fh:
            out[key] = np.asarray(fh.read().splitlines())
    np.savez_compressed(os.path.join(HERE, "whole_fixture.npz"), **out)


if __name__ == "__main__":
    main()
