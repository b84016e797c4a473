"""numpy restatement of the reference's grid subsampling WITH features and classes (test infrastructure only), and the
fixed cases of tests/golden/subsample_features.npz.

Restated from zip:cpp_subsampling/grid_subsampling/grid_subsampling.cpp:5-211 and grid_subsampling.h:10-80:

* points:   fp32 sums in input order, times float(1.0 / count)                                   (.cpp:87)
* features: start at +0.0f, fp32 sums in input order, one true fp32 division by float(count)    (.cpp:90-94, .h:46,59)
* classes:  per label column a std::unordered_map<int,int> histogram filled in input order; the winner is the FIRST
            element of maximal count in the map's iteration order                               (.cpp:99-101, .h:48-52)
* rows:     the cells in the iteration order of std::unordered_map<size_t,SampledData>; max_p keeps the first rows

The libstdc++ iteration order is emulated explicitly here (`umap_order`): one singly linked list, a bucket remembers the
node before its first node, identity hash (an int is converted to size_t, so a negative label hashes to a huge value),
buckets grow 1 -> 13 -> 29 -> 59 -> ... right before the insert that would make size() exceed the bucket count.
tests/test_subsample_features_cpu.py pins this file to the unmodified reference through the fixture.

Two places where the reference is undefined are decided as the product decides them: an empty cloud yields no rows, and
every cloud's classes are its own rows (the reference slices them wrongly for ldim > 1 after the first cloud)."""
import zlib

import numpy as np

GROW = [1, 13, 29, 59, 127, 257, 541, 1109, 2357, 5087, 10273, 20753, 42043, 85229, 172933, 351061, 712697, 1447153]
_MASK = (1 << 64) - 1


def umap_order(keys):
    """Iteration order of a libstdc++ unordered_map after inserting the DISTINCT `keys` (python ints, already reduced to
    size_t) in that order: a list of insertion ranks."""
    m = len(keys)
    HEAD = m
    nxt = [-1] * (m + 1)
    gi, B = 0, GROW[0]
    before = [-1]
    for i in range(m):
        if i + 1 > B:                                  # _M_need_rehash, then _M_rehash_aux (unique keys)
            gi += 1
            B = GROW[gi]
            before = [-1] * B
            p, nxt[HEAD], bbegin = nxt[HEAD], -1, 0
            while p != -1:
                nx, b = nxt[p], keys[p] % B
                if before[b] == -1:
                    nxt[p], nxt[HEAD], before[b] = nxt[HEAD], p, HEAD
                    if nxt[p] != -1:
                        before[bbegin] = p
                    bbegin = b
                else:
                    nxt[p] = nxt[before[b]]
                    nxt[before[b]] = p
                p = nx
        b = keys[i] % B                                # _M_insert_bucket_begin
        if before[b] != -1:
            nxt[i] = nxt[before[b]]
            nxt[before[b]] = i
        else:
            nxt[i], nxt[HEAD] = nxt[HEAD], i
            if nxt[i] != -1:
                before[keys[nxt[i]] % B] = i
            before[b] = HEAD
    out, p = [], nxt[HEAD]
    while p != -1:
        out.append(p)
        p = nxt[p]
    assert len(out) == m
    return out


def vote(labels):
    """max_element over an unordered_map<int,int> histogram of `labels` (filled in this order) with the comparator
    a.second < b.second: the first maximal count in iteration order."""
    distinct, count = [], {}
    for v in labels:
        v = int(v)
        if v not in count:
            distinct.append(v)
            count[v] = 0
        count[v] += 1
    best = None
    for r in umap_order([v & _MASK for v in distinct]):
        v = distinct[r]
        if best is None or count[best] < count[v]:
            best = v
    return best


def _one_cloud(p, dl, f, c):
    f32 = np.float32
    dl = f32(dl)
    mn, mx = p.min(axis=0), p.max(axis=0)
    origin = np.floor(mn * (f32(1) / dl)) * dl                                      # .cpp:27
    nx = int(np.floor((mx[0] - origin[0]) / dl)) + 1                                 # .cpp:30-31
    ny = int(np.floor((mx[1] - origin[1]) / dl)) + 1
    ijk = np.floor((p - origin) / dl).astype(np.int64)                               # .cpp:53-55
    keys = [(int(i) + nx * int(j) + nx * ny * int(k)) & _MASK for i, j, k in ijk]    # .cpp:56
    cell_of, members = {}, []
    for i, k in enumerate(keys):
        if k not in cell_of:
            cell_of[k] = len(members)
            members.append([])
        members[cell_of[k]].append(i)
    first_keys = [keys[ids[0]] for ids in members]
    pts, feats, cls = [], [], []
    with np.errstate(all="ignore"):
        for r in umap_order(first_keys):
            ids = members[r]
            acc = np.zeros(3, f32)
            for i in ids:
                acc = acc + p[i]
            pts.append(acc * f32(1.0 / len(ids)))                                    # .cpp:87
            if f is not None:
                acc = np.zeros(f.shape[1], f32)                                      # vector<float>(fdim): +0.0f
                for i in ids:
                    acc = acc + f[i]
                feats.append(acc / f32(len(ids)))                                    # .cpp:90-94
            if c is not None:
                cls.append([vote(c[ids, j]) for j in range(c.shape[1])])             # .cpp:99-101
    return pts, feats, cls


def subsample_ref(points, lengths, dl, max_p=0, features=None, classes=None):
    """-> (points f32 [M,3], lengths i32 [B], features f32 [M,fdim] or None, classes i32 [M,ldim] or None)"""
    p = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
    lens = np.asarray(lengths, np.int32).reshape(-1)
    f = None if features is None else np.ascontiguousarray(features, np.float32).reshape(p.shape[0], -1)
    c = None if classes is None else np.ascontiguousarray(classes, np.int32).reshape(p.shape[0], -1)
    if max_p < 1:
        max_p = p.shape[0]                                                           # .cpp:134-135
    out_p, out_f, out_c, out_len, lo = [], [], [], [], 0
    for n in lens:
        hi = lo + int(n)
        if n > 0:
            a, b, d = _one_cloud(p[lo:hi], dl, None if f is None else f[lo:hi], None if c is None else c[lo:hi])
            out_p += a[:max_p]
            out_f += b[:max_p]
            out_c += d[:max_p]
            out_len.append(min(len(a), max_p))                                      # .cpp:181-204
        else:
            out_len.append(0)
        lo = hi
    m = len(out_p)
    return (np.asarray(out_p, np.float32).reshape(m, 3), np.asarray(out_len, np.int32),
            None if f is None else np.asarray(out_f, np.float32).reshape(m, f.shape[1]),
            None if c is None else np.asarray(out_c, np.int32).reshape(m, c.shape[1]))


# ------------------------------------------------------------------------------------------------
# the fixed cases of tests/golden/subsample_features.npz (scripts/make_golden_subsample_features.py runs the unmodified
# reference on them; the fixture stores the reference's outputs and a checksum of the inputs, which are rebuilt here)
# ------------------------------------------------------------------------------------------------
FDIMS = (1, 3, 4, 5, 32, 64, 129)


def _case(name, points, lengths, dl, max_p=0, features=None, classes=None, entry="batch"):
    return dict(name=name, points=np.ascontiguousarray(points, np.float32), lengths=np.asarray(lengths, np.int32), dl=float(dl),
                max_p=int(max_p), features=None if features is None else np.ascontiguousarray(features, np.float32),
                classes=None if classes is None else np.ascontiguousarray(classes, np.int32), entry=entry)


def _one_cell(n, rs):
    """n points inside one cell of edge 1 (and far from its faces)"""
    return (0.25 + 0.5 * rs.rand(n, 3)).astype(np.float32)


def fixture_cases():
    cases = []
    rs = np.random.RandomState(20240607)
    cases.append(_case("one_point", [[0.3, 0.2, 0.1]], [1], 0.1, features=[[-0.0, 2.5, 1e8]], classes=[7]))

    # more than 256 cells; sums whose order shows; a lone point carrying -0.0f; one +Inf
    n = 2000
    p = rs.rand(n, 3).astype(np.float32)
    p[-1] = (5.0, 5.0, 5.0)
    f = np.empty((n, 5), np.float32)
    f[:, 0] = np.float32(1e8) + rs.randint(0, 50, n).astype(np.float32)
    f[:, 1] = rs.randn(n)
    f[:, 2] = rs.randn(n) * 1e-3 + 1e4
    f[:, 3] = rs.rand(n)
    f[:, 4] = rs.randint(-4, 5, n)
    f[-1] = -0.0
    f[777, 3] = np.inf
    cases.append(_case("cloud2000", p, [n], 0.12, features=f, classes=rs.randint(-3, 4, n)))

    for d in FDIMS:
        n = 300
        p = rs.rand(n, 3).astype(np.float32)
        f = (rs.randn(n, d) + 1e4).astype(np.float32)
        cases.append(_case("fdim_%d" % d, p, [n], 0.2, features=f))

    lens = [150, 37, 400]
    p = rs.rand(sum(lens), 3).astype(np.float32)
    f = (rs.randn(sum(lens), 3) * 100).astype(np.float32)
    c = rs.randint(0, 6, sum(lens))
    cases.append(_case("three_clouds", p, lens, 0.25, features=f, classes=c))
    cases.append(_case("three_clouds_cap10", p, lens, 0.25, max_p=10, features=f, classes=c))

    n = 5000
    p = (rs.rand(n, 3) * 2).astype(np.float32)
    f = np.stack([np.float32(1e8) + np.arange(n), rs.randn(n), rs.rand(n) * 1e-3, -rs.rand(n)], 1).astype(np.float32)
    cases.append(_case("single_cell_5000", p, [n], 10.0, features=f, classes=rs.randint(0, 40, n)))

    cases.append(_case("tie_5335", _one_cell(4, rs), [4], 1.0, classes=[5, 3, 3, 5]))
    cases.append(_case("tie_3553", _one_cell(4, rs), [4], 1.0, classes=[3, 5, 5, 3]))

    # two cells: 14 distinct labels (past the 13-bucket stage) and 31 (past 29); negative labels, labels that collide
    # modulo 13 and 29, every maximal count tied several times
    a = [0, 13, 26, -1, -13, 29, 58, 2 ** 31 - 1, -2 ** 31, 7, 8, 9, 10, 11]
    b = list(range(-15, 16))
    la = a + a[3:9] + a[3:9]                       # six labels three times, the rest once
    lb = b + b[::3] + b[::3]
    p = np.concatenate([_one_cell(len(la), rs), _one_cell(len(lb), rs) + np.float32([3, 0, 0])])
    cases.append(_case("labels_14_31", p, [len(p)], 1.0, classes=la + lb))

    n = 260
    lab = np.concatenate([rs.permutation(150) * 7919 - 500000, rs.randint(0, 150, n - 150) * 7919 - 500000])
    cases.append(_case("labels_150", _one_cell(n, rs), [n], 1.0, classes=lab, features=rs.randn(n, 2)))

    n = 500
    p = rs.rand(n, 3).astype(np.float32)
    c2 = np.stack([rs.randint(-5, 6, n), rs.randint(100, 103, n)], 1)
    f = rs.randn(n, 3).astype(np.float32)
    cases.append(_case("ldim2_one_cloud", p, [n], 0.2, features=f, classes=c2))
    cases.append(_case("ldim2_single", p, [n], 0.2, features=f, classes=c2, entry="single"))
    cases.append(_case("ldim2_classes_only", p, [n], 0.2, classes=c2, entry="single"))
    return cases


def input_checksum(case):
    h = 0
    for k in ("points", "lengths", "features", "classes"):
        if case[k] is not None:
            h = zlib.crc32(case[k].tobytes(), h)
    return h


def bits(a):
    """float32 array -> its int32 bit patterns (so that -0.0 != +0.0 and Inf == Inf)"""
    return np.ascontiguousarray(a, np.float32).view(np.int32)
