#!/usr/bin/env python3
"""Drop-in for SwiftOrtho's scripts/operon_cluster.py (scored pairs of operons that share more than two gene families; -G T: the
shared-family counts on the GPU): see swiftortho_amd/operon.py."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from swiftortho_amd.operon import main  # noqa: E402

if __name__ == "__main__":
    sys.exit(main())
