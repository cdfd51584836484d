"""numpy references for the DTW kernels (csrc/dtw.hip): the sequential recurrence with the kernels' tie rule in fp32 and in fp64, and
a brute-force enumeration of every warping path (tests/test_dtw_host.py checks the first against the second).  No torch, no GPU."""
import numpy as np


def cell_costs(x, y, metric, dtype):
    """c[i][j] over x (n, C), y (m, C): the channels are added in the order k = 0 .. C-1, in `dtype`"""
    x, y = np.asarray(x, dtype=dtype), np.asarray(y, dtype=dtype)
    acc = np.zeros((x.shape[0], y.shape[0]), dtype=dtype)
    for k in range(x.shape[1]):
        d = x[:, None, k] - y[None, :, k]
        acc = acc + (np.abs(d) if metric == "l1" else d * d)
    return acc if metric == "l1" else np.sqrt(acc)


def dtw_from_costs(c):
    """D[0][0] = c[0][0], D[i][j] = c[i][j] + min(D[i-1][j-1], D[i-1][j], D[i][j-1]) in c's dtype, cell by cell; the first minimum wins
    in the order diagonal, (i-1, j), (i, j-1).  -> (cost, path as a list of (i, j) from (0, 0))"""
    n, m = c.shape
    dt = c.dtype.type
    inf = dt(np.inf)
    D = np.full((n, m), inf, dtype=c.dtype)
    step = np.zeros((n, m), dtype=np.int8)
    for i in range(n):
        for j in range(m):
            if i == 0 and j == 0:
                D[0, 0] = c[0, 0]
                continue
            best, d = (D[i - 1, j - 1] if i > 0 and j > 0 else inf), 0
            up = D[i - 1, j] if i > 0 else inf
            if up < best:
                best, d = up, 1
            left = D[i, j - 1] if j > 0 else inf
            if left < best:
                best, d = left, 2
            D[i, j] = dt(c[i, j] + best)
            step[i, j] = d
    i, j, path = n - 1, m - 1, [(n - 1, m - 1)]
    while (i, j) != (0, 0):
        d = step[i, j]
        i, j = i - (d != 2), j - (d != 1)
        path.append((i, j))
    return D[n - 1, m - 1], path[::-1]


def dtw_ref(x, y, metric="l1", dtype=np.float32):
    return dtw_from_costs(cell_costs(x, y, metric, dtype))


def all_paths(n, m):
    """every warping path from (0, 0) to (n-1, m-1) with steps (1, 0), (0, 1), (1, 1)"""
    if n == 1 and m == 1:
        return [[(0, 0)]]
    out = []
    for di, dj in ((1, 1), (1, 0), (0, 1)):
        if n - di >= 1 and m - dj >= 1:
            out += [p + [(n - 1, m - 1)] for p in all_paths(n - di, m - dj)]
    return out


def brute_force(c):
    """the least path cost over all warping paths through c (exact for integer-valued c)"""
    n, m = c.shape
    return min(sum(c[i, j] for i, j in p) for p in all_paths(n, m))


def path_cost(c, path):
    return sum(c[i, j] for i, j in path)
