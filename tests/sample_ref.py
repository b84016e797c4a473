"""float64 numpy restatement of the interest-point sampler's specification (include/pcrcg.h
"Interest-point sampler"), written from the text, not from csrc/sample.hip.

Segment of N float32 scores w_i, keep count n, seed s in [0, 2^24):
  h_i   = splitmix64(splitmix64((s << 40) + i) ^ D),  D = 0x53414D504C455231
  u_i   = ((h_i >> 11) + 0.5) * 2^-53                 (IEEE double)
  key_i = -log(u_i) / w_i for a finite w_i > 0, else +inf
  N <= n: every row; otherwise the n smallest keys, ties by ascending row; emitted in ascending row."""
import itertools

import numpy as np

DOMAIN = np.uint64(0x53414D504C455231)
_MASK = (1 << 64) - 1


def splitmix64(x):
    """Vectorised over uint64 arrays (arithmetic mod 2^64)."""
    with np.errstate(over="ignore"):
        z = x + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def keys(scores, seed):
    """float64 [N] keys of one segment."""
    w = np.asarray(scores, dtype=np.float32).reshape(-1)
    if not 0 <= int(seed) < (1 << 24):
        raise ValueError("seed outside [0, 2^24)")
    ctr = np.uint64((int(seed) << 40) & _MASK) + np.arange(len(w), dtype=np.uint64)
    h = splitmix64(splitmix64(ctr) ^ DOMAIN)
    u = ((h >> np.uint64(11)).astype(np.float64) + 0.5) * 2.0 ** -53
    good = np.isfinite(w) & (w > 0)
    key = np.full(len(w), np.inf)
    key[good] = np.abs(-np.log(u[good]) / w[good].astype(np.float64))     # abs: -0.0 (u = 1) is 0
    return key


def sample(scores, n, seed):
    """int64 indices of the kept rows, ascending."""
    key = keys(scores, seed)
    if len(key) <= n:
        return np.arange(len(key), dtype=np.int64)
    order = np.argsort(key, kind="stable")               # stable: equal keys stay in ascending row order
    return np.sort(order[:n]).astype(np.int64)


def relative_gap(scores, n, seed):
    """(k_{n+1} - k_n) / k_n between the n-th and (n+1)-th smallest FINITE keys (inf when there is no such pair: the
    boundary then lies among the +inf keys, which are ordered by row alone, or N <= n)."""
    key = np.sort(keys(scores, seed))
    key = key[np.isfinite(key)]
    if len(key) <= n:
        return np.inf
    return (key[n] - key[n - 1]) / key[n - 1]


def inclusion_probabilities(weights, n):
    """Exact probability of every row being among n successive draws without replacement, each proportional to the
    weights that are left (what np.random.choice(replace=False, p=w / sum) does), by enumerating the ordered draws."""
    w = np.asarray(weights, dtype=np.float64)
    p = np.zeros(len(w))
    for seq in itertools.permutations(range(len(w)), n):
        left, pr = w.sum(), 1.0
        for i in seq:
            pr *= w[i] / left
            left -= w[i]
        p[list(seq)] += pr
    return p
