#!/usr/bin/env python3
"""Counterpart of the first half of SwiftOrtho's scripts/rbh2phy.py: the core-gene families from reciprocal best hits against a reference
taxon, one FASTA file per family (-G T: on the GPU).  Aligning and joining them is left out: see swiftortho_amd/rbh.py."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from swiftortho_amd.rbh import main_rbh2phy  # noqa: E402

if __name__ == "__main__":
    sys.exit(main_rbh2phy())
