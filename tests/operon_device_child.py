"""Child process of tests/test_gpu_operon.py: so_operon_pairs in both modes on every designed table and every golden input, under the
SOHIT_* switches of its environment; the arrays go into the .npz file named on the command line.

    python tests/operon_device_child.py out.npz
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)


def tables():
    """-> [(key, table)]: the designed tables, then the goldens' inputs"""
    import operon_inputs as oi
    from swiftortho_amd import operon
    out = [("d_" + k, t) for k, (t, _) in sorted(oi.designed().items())]
    return out + [("g_" + n, operon.operon_table(*oi.case_texts(n))) for n in oi.golden_names()]


def main(path):
    from swiftortho_amd import operon
    res = {}
    for key, t in tables():
        for flags in (0, 1):
            c = operon.device_operon_pairs(t.start, t.fam, t.length, t.has0, t.n_fam, flags)
            p = "%s/%d/" % (key, flags)
            res[p + "i"], res[p + "j"], res[p + "nshr"] = c.i, c.j, c.nshr
            if flags:
                res[p + "cand_start"] = c.cand_start
            res[p + "stats"] = np.asarray([c.stats[k] for k in ("n_pairs", "n_candidates", "n_expansions", "batches", "waits")], dtype=np.int64)
    np.savez(path, **res)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1]))
