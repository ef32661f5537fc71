"""Plain numpy / Python restatement of what d3net_amd/csrc/assign.hip computes: scipy's rectangular assignment solver
(shortest augmenting paths, float64, scipy's scan and tie order) and the float32 GIoU cost in the kernel's operation order.
A test helper: tests/test_lsap.py pins it against scipy and caption_eval.generalized_box3d_iou, the GPU tests compare the
kernel's cost bits against it."""
import numpy as np

F = np.float32


def lsap(cost):
    """-> (rows, cols) like scipy.optimize.linear_sum_assignment(cost), or raises ValueError like scipy"""
    cost = np.asarray(cost, dtype=np.float64)
    if cost.ndim != 2:
        raise ValueError("expected a matrix")
    if not np.all(np.isfinite(cost)):
        raise ValueError("matrix contains invalid numeric entries")
    transposed = cost.shape[1] < cost.shape[0]
    if transposed:
        cost = cost.T
    nr, nc = cost.shape
    if nr == 0:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    inf = float("inf")
    u, v = [0.0] * nr, [0.0] * nc
    col4row, row4col = [-1] * nr, [-1] * nc
    path = [-1] * nc
    for cur in range(nr):
        remaining = [nc - 1 - it for it in range(nc)]
        num_remaining = nc
        SR, SC, sp = [False] * nr, [False] * nc, [inf] * nc
        min_val, i, sink = 0.0, cur, -1
        while sink == -1:
            SR[i] = True
            lowest, index = inf, -1
            for it in range(num_remaining):
                j = remaining[it]
                r = min_val + float(cost[i, j]) - u[i] - v[j]
                if r < sp[j]:
                    path[j] = i
                    sp[j] = r
                if sp[j] < lowest or (sp[j] == lowest and row4col[j] == -1):
                    lowest = sp[j]
                    index = it
            min_val = lowest
            if min_val == inf:
                raise ValueError("cost matrix is infeasible")
            j = remaining[index]
            if row4col[j] == -1:
                sink = j
            else:
                i = row4col[j]
            SC[j] = True
            num_remaining -= 1
            remaining[index] = remaining[num_remaining]
        u[cur] += min_val
        for i in range(nr):
            if SR[i] and i != cur:
                u[i] += min_val - sp[col4row[i]]
        for j in range(nc):
            if SC[j]:
                v[j] -= min_val - sp[j]
        j = sink
        while True:
            i = path[j]
            row4col[j] = i
            col4row[i], j = j, col4row[i]
            if i == cur:
                break
    if transposed:
        order = np.argsort(np.asarray(col4row))
        return np.asarray(col4row, np.int64)[order], np.arange(nr, dtype=np.int64)[order]
    return np.arange(nr, dtype=np.int64), np.asarray(col4row, np.int64)


def _edge_volume(c):
    def edge(i, j):
        d = c[:, i, :] - c[:, j, :]
        return np.sqrt(np.maximum((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2], F(1e-6)))
    return (edge(0, 1) * edge(1, 2)) * edge(0, 4)


def giou_cost(pred, gt):
    """(K,8,3), (G,8,3) float32 corners -> (K,G) float32 cost = -GIoU, every operation float32 in the kernel's order"""
    a, b = np.asarray(pred, F)[:, None], np.asarray(gt, F)[None]
    with np.errstate(all="ignore"):
        top = np.minimum(a[..., 0, 2], b[..., 0, 2])
        height = np.maximum(top - np.maximum(a[..., 4, 2], b[..., 4, 2]), F(0))
        w0 = np.maximum(np.minimum(a[..., 0, 0], b[..., 0, 0]) - np.maximum(a[..., 2, 0], b[..., 2, 0]), F(0))
        w1 = np.maximum(top - np.maximum(a[..., 2, 2], b[..., 2, 2]), F(0))
        inter = (w0 * w1) * height
        lo = np.minimum(a.min(2), b.min(2))
        hi = np.maximum(a.max(2), b.max(2))
        ext = np.abs(hi - lo)
        enclosing = (ext[..., 0] * ext[..., 1]) * ext[..., 2]
        v1 = np.maximum(_edge_volume(np.asarray(pred, F)), F(1e-8))[:, None]
        v2 = np.maximum(_edge_volume(np.asarray(gt, F)), F(1e-8))[None]
        s = v1 + v2
        good = ((enclosing > F(2e-8)) & (s > F(4e-8))).astype(F)
        union = np.maximum(s - inter, F(1e-8))
        cost = -((inter / union - (F(1) - union / enclosing)) * good)
    assert cost.dtype == F
    return cost


def per_col_from_scipy(cost, ncols):
    """what the host loop of assign_dense_caption leaves in per_gt: (B,R,C) cost, (B) valid columns -> (B,C) int64"""
    from scipy.optimize import linear_sum_assignment
    cost = np.asarray(cost)
    out = np.zeros((cost.shape[0], cost.shape[2]), np.int64)
    for b in range(cost.shape[0]):
        n = int(ncols[b])
        if n > 0:
            rows, cols = linear_sum_assignment(cost[b, :, :n])
            out[b, cols] = rows
    return out


def matrix_family(rng, family, R, C):
    """the cost families of the issue: exact ties are the point of all but 'continuous'"""
    if family == "integer":
        return rng.integers(0, 3, (R, C)).astype(F)
    m = rng.random((R, C)).astype(F)
    if family == "continuous":
        return m
    if family == "half_zero_rows":
        m[rng.permutation(R)[:R // 2]] = 0
        return m
    if family == "duplicated_rows":
        src = rng.integers(0, R, R)
        dup = rng.random(R) < 0.5
        m[dup] = m[src[dup]]
        return m
    raise ValueError(family)


def machol_wien(R, C):
    return np.outer(np.arange(1, R + 1), np.arange(1, C + 1)).astype(F)


FAMILIES = ("integer", "continuous", "half_zero_rows", "duplicated_rows")
