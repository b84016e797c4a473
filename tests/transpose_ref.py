"""Restatements for the transposed-table tests, independent of the code under test: the transposition itself as two nested
loops in (q, j) order (numpy), and the three gradients in SCATTER form in float64 (the form the library's gather form must
reproduce): KPConv d x, max_pool, closest_pool."""
import numpy as np
import torch


def transpose_table(idx, h, ns, cols=None, with_columns=True):
    """idx [nq, >= h] integer array, entries outside [0, ns) are shadows.  -> deg [ns] i32, (n_edges, d_max), tq [ns, cols] i64
    (pad nq), th [ns, cols] i32 (pad -1), status.  cols = None: max(d_max, 1).  A row with more edges than columns keeps its
    first `cols`."""
    idx = np.asarray(idx)
    nq = idx.shape[0]
    rows = [[] for _ in range(ns)]
    for q in range(nq):
        for j in range(h):
            v = int(idx[q, j])
            if 0 <= v < ns:
                rows[v].append((q, j))
    deg = np.array([len(r) for r in rows], dtype=np.int32).reshape(ns)
    n_edges = int(deg.sum())
    d_max = int(deg.max()) if ns else 0
    if cols is None:
        cols = max(d_max, 1)
    tq = np.full((ns, cols), nq, dtype=np.int64)
    th = np.full((ns, cols), -1, dtype=np.int32)
    for s, r in enumerate(rows):
        for e, (q, j) in enumerate(r[:cols]):
            tq[s, e], th[s, e] = q, j
    status = int(any(len(r) > cols for r in rows))
    return deg, (n_edges, d_max), tq, (th if with_columns else None), status


def edge_table(g, nq=300, ns=200, h=70, ld=76):
    """The random table of the tests (torch int64 [nq, ld]): 20 % shadows anywhere in a row, two all-shadow rows,
    idx[:, 0] = 0 (fan-in nq: a row of the transpose longer than a wavefront and than 256), support ns - 1 listed by nobody,
    query 11 listing support 7 twice, -1 and ns + 5 as shadows; the columns behind h are never read."""
    idx = torch.randint(0, ns - 1, (nq, ld), generator=g)             # ns - 1: nobody lists it
    idx[torch.rand(nq, ld, generator=g) < 0.2] = ns
    idx[:, 0] = 0
    idx[5, :h] = ns
    idx[9, :h] = -1
    idx[11, 3] = 7
    idx[11, 40] = 7
    idx[20, 2] = -1
    idx[21, 5] = ns + 5
    idx[:, h:] = 3                                                    # a real index the entry must not read
    return idx


def kpconv_dx(q_pts, s_pts, idx, h, dy, inv_n, kp, extent, weights):
    """float64 d x [ns, cin] of the rigid KPConv in scatter form: dx[idx[q, j]] += sum_k w[q, j, k] ((dy / n)[q] @ W[k]^T)."""
    ns = s_pts.shape[0]
    nq = q_pts.shape[0]
    kdim, cin, cout = weights.shape
    ix = idx[:, :h].clone()
    valid = (ix >= 0) & (ix < ns)
    ix[~valid] = ns
    nb = s_pts.double()[ix.clamp(max=ns - 1)] - q_pts.double()[:, None, :]
    w = (1.0 - (nb[:, :, None, :] - kp.double()[None, None]).norm(dim=-1) / extent).clamp(min=0.0) * valid[:, :, None]
    g = dy.double() * inv_n.double()[:, None]
    d_wf = torch.einsum("qo,kco->qkc", g, weights.double())           # [nq, 15, cin]
    contrib = torch.einsum("qhk,qkc->qhc", w, d_wf)
    want = torch.zeros(ns + 1, cin, dtype=torch.float64)
    want.index_add_(0, ix.reshape(-1), contrib.reshape(nq * h, cin))
    return want[:ns]


def max_pool(x, idx, h, dy):
    """float64 (y, d x) of y[q, c] = max_j x[idx[q, j], c] with shadows as 0: the gradient goes to the FIRST column attaining
    the maximum, nowhere when that is a shadow."""
    ns, c = x.shape
    xe = torch.cat([x, torch.zeros(1, c)])
    ix = idx[:, :h].clone()
    ix[(ix < 0) | (ix >= ns)] = ns
    vals = xe[ix]
    y = vals.max(1).values
    first = (vals == y[:, None, :]).to(torch.int8).argmax(1)
    tgt = ix.gather(1, first)
    flat = (tgt * c + torch.arange(c)[None, :]).reshape(-1)
    dx = torch.zeros((ns + 1) * c, dtype=torch.float64)
    dx.index_add_(0, flat, dy.double().reshape(-1))
    return y, dx.view(ns + 1, c)[:ns]


def closest_pool(idx, ns, dy):
    """float64 d x of y = x[idx[:, 0]] (a shadow first index reads the zero row)."""
    c = dy.shape[1]
    i0 = idx[:, 0].clone()
    i0[(i0 < 0) | (i0 >= ns)] = ns
    dx = torch.zeros(ns + 1, c, dtype=torch.float64)
    dx.index_add_(0, i0, dy.double())
    return dx[:ns]
