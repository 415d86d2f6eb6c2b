#!/usr/bin/env python3
"""Generate tests/golden/aa_hbond_topology.npz: the peptide's topology for the hydrogen-bond tests.

Run in the build container only (reads the reference's DATA file test_files/aa_peptide.pdb):

    python tests/golden/make_hbond_fixture.py

Outputs (numpy .npz, data only):
  peptide_bonds    uint32 [362, 2]  0-based atom pairs of the CONECT records of aa_peptide.pdb (the peptide's bonds)
  peptide_element  S1 [363]         element symbol of each peptide atom by the first-letter rule make_golden.py uses
                                    (hydrogen r'^[1-9]?[Hh].*', otherwise the first letter of the atom name)
The water's topology needs no file: in aa_full.npz every OW is followed by its HW1 and HW2 (the tests assert it).
"""
import os
import re

import numpy as np

REF = os.environ.get("GROAN_REFERENCE", "/root/reference")
HERE = os.path.dirname(os.path.abspath(__file__))


def main():
    bonds, names = [], []
    with open(os.path.join(REF, "test_files", "aa_peptide.pdb")) as fh:
        for line in fh:
            if line.startswith(("ATOM", "HETATM")):
                names.append(line[12:16].strip())
            elif line.startswith("CONECT"):
                f = line.split()
                a = int(f[1]) - 1
                bonds.extend((a, int(b) - 1) for b in f[2:])
    assert len(names) == 363 and len(bonds) == 362, (len(names), len(bonds))
    elem = [b"H" if re.match(r"^[1-9]?[Hh]", n) else n[0].upper().encode() for n in names]
    np.savez_compressed(os.path.join(HERE, "aa_hbond_topology.npz"), peptide_bonds=np.asarray(bonds, np.uint32),
                        peptide_element=np.asarray(elem, "S1"))


if __name__ == "__main__":
    main()
