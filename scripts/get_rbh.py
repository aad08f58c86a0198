#!/usr/bin/env python3
"""Drop-in for SwiftOrtho's scripts/get_rbh.py (reciprocal best hits of an all-vs-all search; -G T: on the GPU): see swiftortho_amd/rbh.py."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from swiftortho_amd.rbh import main_get_rbh  # noqa: E402

if __name__ == "__main__":
    sys.exit(main_get_rbh())
