#!/usr/bin/env python3
"""Drop-in for SwiftOrtho's scripts/pan_genome.py (core / shared / specific families, the family-by-taxon table and the rarefaction
curves of a set of ortholog groups; -G T: on the GPU): see swiftortho_amd/pan.py.  -t tree.nwk / -d pairs.tsv add what the reference
does not have: the gene-content tree of the genomes (-m jaccard|overlap, -B bootstrap replicates, -S seed) and the families every pair
of genomes shares."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from swiftortho_amd.pan import main  # noqa: E402

if __name__ == "__main__":
    sys.exit(main())
