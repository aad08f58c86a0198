"""Test oracle (NOT product code): the affinity-propagation loop of SwiftOrtho's bin/find_cluster.py `apclust_blk` (404-513) with
its passes `max_row`, `update_R`, `sum_col`, `update_A`, `get_change` (309-401), restated literally: one Python loop per pass over the
entries in entry order, float64 arithmetic on values re-read from float32 stores, one rounding to float32 per pass.  It shares
nothing with the device kernels (no grouping by row or column, no prefix maxima) -- which is the point."""
import numpy as np


def apc_rounds(row, col, score, n_genes, damp, rounds=100):
    """yields (labels int64, r float32, a float32) after every round"""
    I = np.asarray(row).astype(np.float32).astype(np.int64).tolist()      # ids pass through the float32 store too
    K = np.asarray(col).astype(np.float32).astype(np.int64).tolist()
    S = np.asarray(score, dtype=np.float32).astype(np.float64).tolist()
    N, D = len(I), int(n_genes)
    damp = float(damp)
    beta = 1 - damp
    R32, A32 = np.zeros(N, dtype=np.float32), np.zeros(N, dtype=np.float32)
    # diag: 0 row max, 1 its column, 2 second row max, 3 its column, 4 column sum, 5 R of the diagonal -- zeros, created once
    d0, d1, d2, d3, d5 = [0.0] * D, [0.0] * D, [0.0] * D, [0.0] * D, [0.0] * D
    lab = list(range(D))
    for _ in range(rounds):
        R, A = R32.astype(np.float64).tolist(), A32.astype(np.float64).tolist()
        for n in range(N):                                  # max_row
            i, k = I[n], K[n]
            ra = R[n] + A[n]
            if d0[i] < ra:
                d0[i] = ra
                d1[i] = k
            elif d2[i] < ra:
                d2[i] = ra
                d3[i] = k
        for n in range(N):                                  # update_R
            i, k = I[n], K[n]
            if k != d1[i]:
                r = S[n] - d0[i]
            else:
                r = S[n] - d2[i]
            x = R[n]
            x *= damp
            x += beta * r
            R[n] = x
            if i == k:
                d5[i] = x
        with np.errstate(over='ignore'):
            R32 = np.array(R, dtype=np.float64).astype(np.float32)
        R = R32.astype(np.float64).tolist()
        d4 = [0.0] * D
        for n in range(N):                                  # sum_col
            if I[n] != K[n]:
                d4[K[n]] += max(0, R[n])
        for n in range(N):                                  # update_A
            i, k = I[n], K[n]
            x = A[n]
            x *= damp
            if i != k:
                x += beta * min(0, d5[k] + d4[k] - max(0, R[n]))
            else:
                x += beta * d4[k]
            A[n] = x
        with np.errstate(over='ignore'):
            A32 = np.array(A, dtype=np.float64).astype(np.float32)
        A = A32.astype(np.float64).tolist()
        ras = [-np.inf] * D
        for n in range(N):                                  # get_change
            i, k = I[n], K[n]
            ra = R[n] + A[n]
            if ras[i] < ra:
                ras[i] = ra
                if lab[i] != k:
                    lab[i] = k
        yield np.array(lab, dtype=np.int64), R32.copy(), A32.copy()


def numpy_apc(row, col, score, n_genes, damp, rounds=100):
    """(labels, r, a) after `rounds` rounds; pluggable into find_cluster.apc(loop=)"""
    out = (np.arange(int(n_genes), dtype=np.int64), np.zeros(len(row), dtype=np.float32), np.zeros(len(row), dtype=np.float32))
    for out in apc_rounds(row, col, score, n_genes, damp, rounds):
        pass
    return out
