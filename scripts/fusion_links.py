#!/usr/bin/env python3
"""Gene-fusion links: the pairs of proteins that align side by side on one composite protein of the hit table and are not homologous to
each other, with the number of composites that link them (-G T: the links on the GPU): see swiftortho_amd/fusion.py."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from swiftortho_amd.fusion import main  # noqa: E402

if __name__ == "__main__":
    sys.exit(main())
