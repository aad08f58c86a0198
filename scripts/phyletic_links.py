#!/usr/bin/env python3
"""Phyletic profiles: the pairs of gene families that co-occur across the genomes of a pan-genome table, with their Jaccard index and
hypergeometric enrichment (-G T: the family pairs on the GPU): see swiftortho_amd/phyletic.py."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from swiftortho_amd.phyletic import main  # noqa: E402

if __name__ == "__main__":
    sys.exit(main())
