#!/usr/bin/env python3
"""Drop-in for SwiftOrtho's scripts/pan_genome.py (core / shared / specific families, the family-by-taxon table and the rarefaction
curves of a set of ortholog groups; -G T: on the GPU): see swiftortho_amd/pan.py."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from swiftortho_amd.pan import main  # noqa: E402

if __name__ == "__main__":
    sys.exit(main())
