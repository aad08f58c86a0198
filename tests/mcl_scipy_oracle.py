"""TEST INFRASTRUCTURE -- the Markov-cluster loop of the reference through scipy on the CPU, the oracle for the device loop
(swiftortho_amd/csrc/mcl.hip, so_mcl).  Follows /root/reference/bin/find_cluster.py `normalize` (636-646) and `mcl` (652-689)
statement by statement on purpose; never imported by the product (tests/test_abi.py checks).  Pinned by the `clu_*` goldens
(stdout of the REAL find_cluster.py): tests/test_find_cluster.py runs the product's host bookkeeping with this loop plugged in."""
import numpy as np
from scipy import sparse

MIDPOINT_ZONE = 2.0 ** -44   # relative half-width of the zone around a float32 rounding boundary that `midpoint_hits` counts


def _normalize(x):
    y = np.asarray(x.sum(0))[0]
    if y.min() == 0 and y.max() > 0:
        y += y.nonzero()[0].min() / 1e3
    else:
        y += 1e-8
    x.data /= y.take(x.indices, mode='clip')


def _midpoint_hits(v64, v32):
    """how many of the float64 powers `v64` lie within a relative MIDPOINT_ZONE of the midpoint between the float32 they round to
    (`v32`) and its neighbour on the other side of them: there a last-bit difference between two double-precision pow routines (a
    16-ulp error is 2^-49 relative) could change the rounded float32.  Zeros, infinities and NaNs round the same way everywhere."""
    ok = np.isfinite(v64) & (v64 != 0) & np.isfinite(v32)
    v64, v32 = v64[ok], v32[ok]
    up = v32.astype(np.float64) < v64
    other = np.where(up, np.nextafter(v32, np.float32(np.inf)), np.nextafter(v32, np.float32(-np.inf)))
    mid = (v32.astype(np.float64) + other.astype(np.float64)) / 2
    return int(np.count_nonzero(np.abs(v64 - mid) <= MIDPOINT_ZONE * np.abs(mid)))


def scipy_mcl(indptr, indices, data, inflation, expansion=2, prune=1e-5, rtol=1e-5, atol=1e-8, rounds=100, check=5, power="numpy", info=None):
    """same signature and result as swiftortho_amd.find_cluster.device_mcl: CSR in, final CSR (storage order, stored zeros) out.

    power: "numpy" -- the reference's own statement `x.data **= inflation` (numpy's float32 power: not correctly rounded, and
    CPU-dispatched); "exact" -- the double-precision power of the float32 value to the float32 exponent, rounded once, which is
    what the device computes: the two can then be compared bit for bit.
    info: a dict that receives `rounds` (rounds begun), `converged` (0 / 1), `checks` (one dict per convergence check: `round` = the
    loop index i of the check, `longest_old_row` = stored entries of the longest row of x_old, `max` = the float32 maximum that was
    compared with atol, `row` = the row that holds it, -1 when it is an implicit zero) and, in "exact" mode, `midpoint_hits`
    (see _midpoint_hits; 0 = no inflated value of the run was near a rounding boundary).
    An empty block (n = 0; the reference never builds one, and scipy refuses the reductions of a 0 x 0 matrix) has no entry that
    could differ: every round is a no-op and the first convergence check succeeds on the maximum of nothing, 0."""
    if power not in ("numpy", "exact"):
        raise ValueError("power: 'numpy' or 'exact'")
    n = len(indptr) - 1
    x = sparse.csr_matrix((np.asarray(data, dtype=np.float32), np.asarray(indices, dtype=np.int32), np.asarray(indptr)), shape=(n, n), dtype='float32')
    done, converged, checks, hits = 0, 0, [], 0
    for i in range(rounds):
        done = i + 1
        if n == 0:
            if i % check == 0 and i > 0:
                checks.append({"round": i, "longest_old_row": 0, "max": np.float32(0), "row": -1})
                if np.float32(0) <= atol:
                    converged = 1
                    break
            continue
        _normalize(x)
        if i % check == 0:
            x_old = x.copy()
        x = x ** expansion
        if power == "exact":
            v64 = x.data.astype(np.float64) ** np.float64(np.float32(inflation))
            x.data = v64.astype(np.float32)
            hits += _midpoint_hits(v64, x.data)
        else:
            x.data **= inflation
        if i % check == 0 and i > 0:
            d = abs(x - x_old) - rtol * abs(x_old)
            m = d.max()
            row = -1
            if d.nnz and (m != m or m == d.data.max()):
                coo = d.tocoo()
                row = int(coo.row[np.flatnonzero(np.isnan(coo.data))[0] if m != m else np.argmax(coo.data)])
            checks.append({"round": i, "longest_old_row": int(np.diff(x_old.indptr).max()), "max": np.float32(m), "row": row})
            if m <= atol:
                converged = 1
                break
        x.data[x.data < prune] = 0.
    if isinstance(info, dict):
        info.update(rounds=done, converged=converged, checks=checks)
        if power == "exact":
            info["midpoint_hits"] = hits
    return np.asarray(x.indptr, dtype=np.int64), np.asarray(x.indices, dtype=np.int32), np.asarray(x.data, dtype=np.float32)
