#!/usr/bin/env python3
"""Counterpart of the first half of SwiftOrtho's scripts/rbh2phy.py: the core-gene families from reciprocal best hits against a reference
taxon, one FASTA file per family (-G T: on the GPU).  Aligning them with an external program is left out: see swiftortho_amd/rbh.py.
-A T joins the families along the alignments the search itself made (the 17th column of find_hit.py -C T) instead: the core-gene
supermatrix as FASTA on stdout, -g <share> trims gappy columns, -t <file.nwk> writes the neighbour-joining tree: swiftortho_amd/phy.py."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from swiftortho_amd.rbh import main_rbh2phy  # noqa: E402

if __name__ == "__main__":
    sys.exit(main_rbh2phy())
