"""GPU: the image-input kernels at their edges, bit for bit against references that share no code with them.

  pcrcg_project_depth          against tests/golden/projection_edges.npz (the reference's own output) and PR.project
  pcrcg_inject_frames          against PR.inject_frames_ref (PR.project + include/pcrcg.h's rule in numpy)
  pcrcg_fill2d + pcrcg_inject_image_features   against MR.inject_image_features on PR.project's indices
  pcrcg_superglue_valid_maps   against PR.paint_valid_maps (numpy's own slice assignment)

Every entry is called through ctypes on output buffers pre-filled with a sentinel (a NaN with a payload / a negative
int64) that carry a guard region behind the last row: what the entry promises must be overwritten, everything else --
the padding columns where the entry does not own them, and the guard -- must still hold the sentinel.  Expected sides
never come from the library; the one exception is the closing fused == unfused assertion of _check_injection."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import model_ref as MR
from pcrcg_amd import _lib, ops
from pcrcg_amd.projection import Projection
from pcrcg_amd.synthetic import _pose

from . import projection_ref as PR

pytestmark = pytest.mark.gpu

F32 = np.float32
GUARD = 8                          # guard rows behind every output (one whole 8-point group of pcrcg_inject_frames)
NAN_BITS = 0x7FC0BEEF              # the float sentinel: a quiet NaN no arithmetic produces
I64_SENTINEL = -0x5A5A5A5A5A5A5A5B


def _sentinel_f32(rows, ld, dev):
    return torch.full((rows + GUARD, ld), NAN_BITS, dtype=torch.int32, device=dev).view(torch.float32)


def _untouched(t):
    """bool mask: the element still holds the sentinel."""
    if t.dtype == torch.float32:
        return t.view(torch.int32) == NAN_BITS
    return t == I64_SENTINEL


def _dev(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


# ------------------------------------------------------------------------------------------------
# pcrcg_project_depth
# ------------------------------------------------------------------------------------------------
def _project(dev, points, depth, w2c, K, thresh=0.1):
    """pcrcg_project_depth through ctypes on guarded sentinel buffers -> (inds2d, inds3d) numpy, having asserted that the
    count, exactly the first k rows and nothing else were written."""
    L = _lib.lib()
    points = np.asarray(points, F32).reshape(-1, 3)
    n = len(points)
    depth = np.asarray(depth, F32)
    h, w = depth.shape[-2:]
    pts, d = _dev(points, dev), _dev(depth, dev)
    i2 = torch.full((n + GUARD, 2), I64_SENTINEL, dtype=torch.int64, device=dev)
    i3 = torch.full((n + GUARD,), I64_SENTINEL, dtype=torch.int64, device=dev)
    k = torch.full((2,), -77, dtype=torch.int32, device=dev)
    nbytes = L.pcrcg_project_depth_ws_bytes(n)
    ws = torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=dev)
    _lib.check(L.pcrcg_project_depth(pts.data_ptr() if n else None, n, d.data_ptr(), h, w, ops.matrix16(w2c), ops.matrix16(K),
                                     float(thresh), i2.data_ptr(), i3.data_ptr(), k.data_ptr(), ws.data_ptr(), nbytes,
                                     ops._stream()), "pcrcg_project_depth")
    kk, after = (int(v) for v in k.cpu())
    assert after == -77 and 0 <= kk <= n
    assert bool(_untouched(i2[kk:]).all()) and bool(_untouched(i3[kk:]).all())
    assert not bool(_untouched(i2[:kk]).any()) and not bool(_untouched(i3[:kk]).any())
    return i2[:kk].cpu().numpy(), i3[:kk].cpu().numpy()


@pytest.fixture(scope="module")
def edges(golden_dir):
    return PR.load_edges(golden_dir)


def test_project_edge_fixture(cuda, edges):
    """The reference's recorded decisions at every boundary (scripts/make_golden_projection_edges.py)."""
    for c in edges:
        i2, i3 = _project(cuda, c["points"], c["depth"], c["world2camera"], c["intrinsics"], c["thresh"])
        assert np.array_equal(i3, c["inds3d"]), c["name"]
        assert np.array_equal(i2, c["inds2d"]), c["name"]


def test_project_matrix_and_depth_forms(cuda, edges):
    """3x3 and 4x4 intrinsics, a host and a device world2camera, [H, W] and [1, H, W] depth: one result."""
    by_name = {c["name"]: c for c in edges}
    for name in ("borders_f64_perm", "frame_37x53", "borders_f1_z2.0"):
        c = by_name[name]
        K3 = torch.from_numpy(c["intrinsics"][:3, :3].copy())
        K4 = torch.eye(4)
        K4[:3, :3] = K3
        depth2 = torch.from_numpy(c["depth"].reshape(c["depth"].shape[-2:])).to(cuda)
        pts, w2c = torch.from_numpy(c["points"]).to(cuda), torch.from_numpy(c["world2camera"])
        for K in (K3, K4):
            for depth in (depth2, depth2[None]):
                for pose in (w2c, w2c.to(cuda)):
                    i2, i3 = Projection(K, thresh=c["thresh"]).projection(pts, depth, pose)
                    assert i2.dtype == torch.int64 and i3.dtype == torch.int64 and i2.shape == (len(c["inds3d"]), 2)
                    assert np.array_equal(i2.cpu().numpy(), c["inds2d"]), name
                    assert np.array_equal(i3.cpu().numpy(), c["inds3d"]), name


def _plane_cloud(rng, n, w, h, K, w2c, margin):
    """n world points that land on the camera plane z = 1.5 at quotients within `margin` pixels outside the frame
    (negative: inside), under a composed, non-exact pose."""
    q = np.stack([rng.uniform(-margin, w + margin, n), rng.uniform(-margin, h + margin, n)], 1)
    cam = np.stack([(q[:, 0] - K[0, 2]) * 1.5 / K[0, 0], (q[:, 1] - K[1, 2]) * 1.5 / K[1, 1], np.full(n, 1.5)], 1)
    R, t = w2c[:3, :3].astype(np.float64), w2c[:3, 3].astype(np.float64)
    return ((cam - t) @ R).astype(F32)


def _scan_case(n, mode):
    rng = np.random.RandomState(n % 1000 + len(mode))
    w, h = 160, 120
    K = np.array([[128.0, 0, 80.0], [0, 128.0, 60.0], [0, 0, 1]], F32)
    w2c = (_pose(rng) @ _pose(rng)).astype(F32)
    pts = _plane_cloud(rng, n, w, h, K, w2c, -0.5 if mode == "all" else 6.0)
    depth = np.full((h, w), 1.5, F32)
    if mode == "none":
        depth[:] = 100.0
    elif mode == "half":
        depth[(np.arange(h)[:, None] + np.arange(w)[None, :]) % 2 == 1] = 100.0
    return pts, depth, w2c, K


SCAN_CASES = [(n, "half") for n in (0, 1, 2047, 2048, 2049, 65536, 65537, 150001)]
SCAN_CASES += [(n, m) for n in (2049, 65537, 150001) for m in ("none", "all")]


@pytest.mark.parametrize("n,mode", SCAN_CASES)
def test_project_scan_paths(cuda, n, mode):
    """n on either side of the one-tile (2048) and one-block (65536) bounds of the compaction's scan, with no / every /
    every second point surviving."""
    pts, depth, w2c, K = _scan_case(n, mode)
    want2, want3 = PR.project(pts, depth, w2c, K)
    k = len(want3)
    if mode == "none":
        assert k == 0
    elif mode == "all":
        assert k == n
    elif n >= 2047:
        assert 0.3 * n < k < 0.7 * n
    i2, i3 = _project(cuda, pts, depth, w2c, K)
    assert len(i3) == k
    assert np.array_equal(i3, want3) and np.array_equal(i2, want2)
    assert (np.diff(i3) > 0).all()


# ------------------------------------------------------------------------------------------------
# pcrcg_inject_frames, and pcrcg_fill2d + pcrcg_inject_image_features
# ------------------------------------------------------------------------------------------------
SIZES = {"s": (37, 53), "m": (24, 40), "l": (160, 120)}       # (w, h)


def _frame(rng, size, target, c, valid, thresh, fmap_value=None, accept=0.6):
    """One raw frame that looks at the plane cloud of _cloud(): a composed pose, intrinsics scaled to its size, a depth
    map that accepts about `accept` of its pixels (and holds NaN, 0 and inf pixels), a random or constant fmap, and
    `valid`: None, or a non-symmetric [w, h] map holding zeros and values above 1."""
    w, h = SIZES[size]
    K = np.array([[0.7 * w, 0, 0.5 * w], [0, 0.7 * w, 0.5 * h], [0, 0, 1]], F32)
    w2c = _pose(rng, angle=0.05, shift=0.04).astype(F32)
    depth = np.where(rng.rand(h, w) < accept, 1.5, 100.0).astype(F32)
    depth.flat[rng.permutation(h * w)[:6]] = [np.nan, 0.0, np.inf, -np.inf, np.nan, 0.0]
    fmap = rng.uniform(-2, 2, (c, h, w)).astype(F32) if fmap_value is None else np.full((c, h, w), fmap_value, F32)
    fr = dict(fmap=fmap, depth=depth, world2camera=w2c, intrinsics=K, target=bool(target), thresh=thresh)
    if valid:
        v = rng.uniform(0.25, 3.0, (w, h)).astype(F32)
        v[rng.rand(w, h) < 0.3] = 0.0
        fr["valid"] = v
    return fr


def _cloud(rng, n):
    """n points near the plane z = 1.5 in front of the identity camera, about a tenth outside any frame's view."""
    return np.stack([rng.uniform(-1.25, 1.25, n), rng.uniform(-1.25, 1.25, n), 1.5 + rng.uniform(-0.15, 0.15, n)], 1).astype(F32)


def _scene(seed, n, c, slots, fmap_values=None):
    """slots: a string of frames in write order, e.g. "sS mM lL": lower case = source side, upper = target side, the
    letter = the size (SIZES).  Per-frame thresh values differ; every second frame carries a valid map."""
    rng = np.random.RandomState(seed)
    frames = []
    for j, s in enumerate(slots.replace(" ", "")):
        frames.append(_frame(rng, s.lower(), s.isupper(), c, valid=j % 2 == 0, thresh=(0.1, 0.04, 0.2)[j % 3],
                             fmap_value=None if fmap_values is None else fmap_values[j]))
    return _cloud(rng, n), frames


def _frames_on(frames, dev):
    return [{k: (_dev(v, dev) if k in ("fmap", "depth", "valid") else v) for k, v in fr.items()} for fr in frames]


def _inject_frames(dev, points, len_src, frames_dev, c, ldx):
    """pcrcg_inject_frames through ctypes -> x [n, ldx] (device), having asserted every row written and the guard kept."""
    L = _lib.lib()
    n = len(points)
    pts = _dev(np.asarray(points, F32).reshape(-1, 3), dev)
    arr = (ops.ImageFrame * max(len(frames_dev), 1))()
    keep = []
    for j, fr in enumerate(frames_dev):
        arr[j], ts = ops.frame_struct(fr, c)
        keep.append(ts)
    x = _sentinel_f32(n, ldx, dev)
    _lib.check(L.pcrcg_inject_frames(pts.data_ptr(), n, int(len_src), ctypes.cast(arr, ctypes.c_void_p), len(frames_dev), c,
                                     x.data_ptr(), ldx, ops._stream()), "pcrcg_inject_frames")
    assert bool(_untouched(x[n:]).all()), "guard rows written"
    assert not bool(_untouched(x[:n]).any()), "a promised element was not written"
    return x[:n]


def _inject_unfused(dev, n, len_src, frames_dev, projections, c, ldx):
    """pcrcg_fill2d + one pcrcg_inject_image_features per frame, fed the REFERENCE's indices -> x [n, ldx] (device), having
    asserted that the padding columns (which these entries do not own) and the guard were left alone."""
    L = _lib.lib()
    x = _sentinel_f32(n, ldx, dev)
    _lib.check(L.pcrcg_fill2d(x.data_ptr(), ldx, n, c + 1, 1.0, ops._stream()), "pcrcg_fill2d")
    for fr, (i2, i3) in zip(frames_dev, projections):
        h, w = fr["fmap"].shape[1:]
        d2, d3 = _dev(i2, dev), _dev(i3, dev)
        _lib.check(L.pcrcg_inject_image_features(fr["fmap"].data_ptr(), c, h, w, ops._ptr(fr.get("valid")),
                                                 d2.data_ptr() if len(i3) else None, d3.data_ptr() if len(i3) else None,
                                                 len(i3), int(len_src) if fr["target"] else 0, n, x.data_ptr(), ldx,
                                                 ops._stream()), "pcrcg_inject_image_features")
    assert bool(_untouched(x[n:]).all()), "guard rows written"
    assert bool(_untouched(x[:n, c + 1:]).all()), "padding columns written"
    assert not bool(_untouched(x[:n, :c + 1]).any()), "a promised element was not written"
    return x[:n]


def _check_injection(dev, points, len_src, frames, c, ldx):
    """Both paths against their references, then fused == unfused.  -> winner [n] (PR.inject_frames_ref)."""
    n = len(points)
    want, winner = PR.inject_frames_ref(points, len_src, frames, c, ldx)
    projections, images = [], []
    for fr in frames:
        lo, hi = (len_src, n) if fr["target"] else (0, len_src)
        i2, i3 = PR.project(points[lo:hi], fr["depth"], fr["world2camera"], fr["intrinsics"], fr["thresh"])
        projections.append((i2, i3))
        images.append(dict(fmap=torch.from_numpy(fr["fmap"]), inds2d=torch.from_numpy(i2), inds3d=torch.from_numpy(i3),
                           target=fr["target"], valid=None if fr.get("valid") is None else torch.from_numpy(fr["valid"])))
    want_mr = MR.inject_image_features(n, len_src, images, channels=c)
    assert torch.equal(want_mr, torch.from_numpy(want[:, :c + 1]))          # the two statements of the rule agree
    frames_dev = _frames_on(frames, dev)
    fused = _inject_frames(dev, points, len_src, frames_dev, c, ldx)
    assert torch.equal(fused.cpu(), torch.from_numpy(want))
    unfused = _inject_unfused(dev, n, len_src, frames_dev, projections, c, ldx)
    assert torch.equal(unfused[:, :c + 1].cpu(), want_mr)
    assert torch.equal(fused[:, :c + 1], unfused[:, :c + 1])
    return winner


def _len_srcs(n):
    mid = max(1, (3 * n) // 7)
    if mid % 8 == 0:
        mid += 3
    return sorted({0, n, min(mid, n)})


GROUP_CASES = [(n, ls) for n in (1, 7, 8, 9, 251, 2051) for ls in _len_srcs(n)]


@pytest.mark.parametrize("n,len_src", GROUP_CASES)
def test_inject_frames_groups(cuda, n, len_src):
    """Whole and tail groups of 8 points, one block and several, the clouds' boundary at either end and inside a group."""
    assert len_src in (0, n) or len_src % 8
    points, frames = _scene(n, n, 5, "sS mM sM")
    winner = _check_injection(cuda, points, len_src, frames, 5, 9)
    if n >= 251:
        assert (winner >= 0).any() and (winner < 0).any()
        if 0 < len_src < n:
            assert len(set(winner[:len_src]) - {-1}) == 3 and len(set(winner[len_src:]) - {-1}) == 3


@pytest.mark.parametrize("pad", [1, 4, 68])
@pytest.mark.parametrize("c", [1, 3, 63, 64, 65, 128, 130])
def test_inject_frames_channels(cuda, c, pad):
    """c below, at and above one and two wavefronts of lanes; ldx = c + 1 (no padding), c + 4, c + 68 (padding that spans
    more than one pass over the lanes).  Three sizes of frame in one call."""
    points, frames = _scene(100 + c, 251, c, "sM lS m")
    winner = _check_injection(cuda, points, 123, frames, c, c + pad)
    assert {0, 1, 2, 3, 4} <= set(winner)


@pytest.mark.parametrize("slots", ["", "s", "L", "sml", "LMS", "lms SML", "sml SML", "lSmMsL", "sml L", "S lms", "mM", "lll"])
def test_inject_frames_slots(cuda, slots):
    """0 frames, one side only, 3 + 3, 3 + 1 and 1 + 3, frames of three sizes in one call with the largest first and last,
    the sides interleaved."""
    n, len_src = 251, 123
    points, frames = _scene(len(slots) * 7 + 1, n, 3, slots)
    winner = _check_injection(cuda, points, len_src, frames, 3, 7)
    for side, rows in ((False, winner[:len_src]), (True, winner[len_src:])):
        own = {j for j, fr in enumerate(frames) if fr["target"] == side}
        assert set(rows) - {-1} == own, (slots, side)               # every frame wins somewhere; none on the other side
    if not slots:
        assert (winner == -1).all()


def test_inject_frames_write_order(cuda):
    """Overlapping frames of one side with a distinct constant per frame: each point carries the value of the LAST frame in
    the list that accepts it."""
    values = [2.0, 3.0, 5.0, 7.0, 11.0, 13.0]
    n, len_src, c = 2051, 1003, 3
    points, frames = _scene(9, n, c, "sml LSM", fmap_values=values)
    for fr in frames:
        fr.pop("valid", None)
    winner = _check_injection(cuda, points, len_src, frames, c, c + 4)
    x = _inject_frames(cuda, points, len_src, _frames_on(frames, cuda), c, c + 4).cpu().numpy()
    accepts = np.zeros((len(frames), n), bool)
    for j, fr in enumerate(frames):
        lo, hi = (len_src, n) if fr["target"] else (0, len_src)
        accepts[j, lo + PR.project(points[lo:hi], fr["depth"], fr["world2camera"], fr["intrinsics"], fr["thresh"])[1]] = True
    last = np.where(accepts.any(0), len(frames) - 1 - np.argmax(accepts[::-1], 0), -1)
    assert np.array_equal(winner, last)
    assert np.array_equal(x[:, 0], np.where(last >= 0, np.asarray(values, F32)[last], F32(1)))
    for rows in (slice(0, len_src), slice(len_src, n)):
        assert len(set(last[rows]) - {-1}) == 3 and (last[rows] == -1).any()
        assert (accepts[:, rows].sum(0) >= 2).sum() > 50            # points that several frames accept: the order matters


def test_inject_frames_valid_layout(cuda):
    """A [w, h] valid map that a [h, w] read would get wrong (non-square, non-symmetric, zeros and values above 1), present
    on some frames of the call and absent on others; per-frame thresh values that differ."""
    n, len_src, c = 251, 123, 65
    points, frames = _scene(21, n, c, "sS mL")
    assert [("valid" in fr) for fr in frames] == [True, False, True, False]
    assert len({fr["thresh"] for fr in frames}) == 3
    for fr in frames:
        if "valid" in fr:
            v = fr["valid"]
            assert v.shape[0] != v.shape[1] and (v == 0).any() and (v > 1).any()
            assert not np.array_equal(v.reshape(-1), v.T.reshape(-1))
    winner = _check_injection(cuda, points, len_src, frames, c, c + 4)
    for j, fr in enumerate(frames):
        # a tighter or wider thresh changes what the frame keeps: the differing values are all in use
        lo, hi = (len_src, n) if fr["target"] else (0, len_src)
        kept = [len(PR.project(points[lo:hi], fr["depth"], fr["world2camera"], fr["intrinsics"], t)[1]) for t in (0.04, 0.2)]
        assert kept[0] < kept[1], j
    assert (winner == 0).any() and (winner == 2).any()


def test_inject_frames_edge_points(cuda, edges):
    """The edge fixture's clouds (quotients at the borders, z = 0, behind the camera, non-finite coordinates) as the two
    clouds of a pair, its frames as the frames, among ordinary points."""
    by_name = {c["name"]: c for c in edges}
    rng = np.random.RandomState(5)
    c = 3

    def frame(name, target):
        e = by_name[name]
        h, w = e["depth"].shape[-2:]
        return dict(fmap=rng.uniform(-2, 2, (c, h, w)).astype(F32), depth=e["depth"].reshape(h, w),
                    world2camera=e["world2camera"], intrinsics=e["intrinsics"], thresh=e["thresh"], target=target,
                    valid=rng.uniform(0.5, 2, (w, h)).astype(F32))
    src_names = ("borders_f1_z1.0", "z_zero_f1", "behind_z-0.0625", "nonfinite", "thresh0.125_d0", "depth_special_z1.0")
    tgt_names = ("borders_f64_perm", "behind_perm", "nonfinite_perm", "z_zero_f64", "behind_z-1.0")
    ordinary = _cloud(rng, 40) * np.array([60, 50, 1], F32) + np.array([80, 60, -0.5], F32)     # in view of the f = 1 frames
    src = np.concatenate([by_name[k]["points"] for k in src_names] + [ordinary])
    tgt = np.concatenate([by_name[k]["points"] for k in tgt_names] + [ordinary])
    points = np.concatenate([src, tgt])
    frames = [frame("behind_z-0.0625", False), frame("borders_f64_perm", True), frame("borders_f1_z1.0", False),
              frame("behind_perm", True), frame("depth_special_z1.0", False), frame("behind_z-1.0", True)]
    winner = _check_injection(cuda, points, len(src), frames, c, c + 4)
    assert set(winner) == {-1, 0, 1, 2, 3, 4, 5}
    bad = ~np.isfinite(points).all(1)
    assert bad.sum() >= 30 and (winner[bad] == -1).all()


def test_unfused_entries_alone(cuda):
    """pcrcg_inject_image_features: an index pair repeated across two images resolves in call order, an empty index list
    writes nothing, rows outside [0, n_rows) are dropped; pcrcg_fill2d with ld > cols and with rows = 0."""
    L = _lib.lib()
    rng = np.random.RandomState(3)
    c, w, h, n, ldx = 65, 37, 53, 40, 70
    fm = [rng.uniform(-2, 2, (c, h, w)).astype(F32) for _ in range(2)]
    valid = rng.uniform(0, 2, (w, h)).astype(F32)
    i2 = np.stack([rng.randint(0, w, 25), rng.randint(0, h, 25)], 1).astype(np.int64)
    i3 = np.sort(rng.permutation(n)[:25]).astype(np.int64)
    images = [dict(fmap=torch.from_numpy(fm[0]), inds2d=torch.from_numpy(i2), inds3d=torch.from_numpy(i3), valid=None),
              dict(fmap=torch.from_numpy(fm[1]), inds2d=torch.from_numpy(i2[5:]), inds3d=torch.from_numpy(i3[5:]),
                   valid=torch.from_numpy(valid)),
              dict(fmap=torch.from_numpy(fm[0]), inds2d=torch.zeros((0, 2), dtype=torch.int64),
                   inds3d=torch.zeros(0, dtype=torch.int64), valid=None)]
    want = MR.inject_image_features(n, 0, images, channels=c)
    x = _sentinel_f32(n, ldx, cuda)
    _lib.check(L.pcrcg_fill2d(x.data_ptr(), ldx, n, c + 1, 1.0, ops._stream()), "pcrcg_fill2d")
    assert bool(_untouched(x[:, c + 1:]).all()) and bool(_untouched(x[n:]).all()) and bool((x[:n, :c + 1] == 1).all())
    for im in images:
        k = len(im["inds3d"])
        f, v = im["fmap"].to(cuda), None if im["valid"] is None else im["valid"].to(cuda)
        d2, d3 = im["inds2d"].to(cuda), im["inds3d"].to(cuda)
        _lib.check(L.pcrcg_inject_image_features(f.data_ptr(), c, h, w, ops._ptr(v), d2.data_ptr() if k else None,
                                                 d3.data_ptr() if k else None, k, 0, n, x.data_ptr(), ldx, ops._stream()),
                   "pcrcg_inject_image_features")
    assert torch.equal(x[:n, :c + 1].cpu(), want)
    assert bool(_untouched(x[:n, c + 1:]).all()) and bool(_untouched(x[n:]).all())
    assert not torch.equal(want[i3[5:]], MR.inject_image_features(n, 0, images[:1], channels=c)[i3[5:]])   # the order showed
    # fill2d: rows = 0 and cols = 0 write nothing; ld > cols leaves the columns behind cols alone, for any value
    y = _sentinel_f32(5, 9, cuda)
    _lib.check(L.pcrcg_fill2d(y.data_ptr(), 9, 0, 4, 1.0, ops._stream()), "pcrcg_fill2d")
    _lib.check(L.pcrcg_fill2d(y.data_ptr(), 9, 5, 0, 1.0, ops._stream()), "pcrcg_fill2d")
    assert bool(_untouched(y).all())
    _lib.check(L.pcrcg_fill2d(y.data_ptr(), 9, 5, 4, -2.5, ops._stream()), "pcrcg_fill2d")
    assert bool((y[:5, :4] == -2.5).all()) and bool(_untouched(y[:5, 4:]).all()) and bool(_untouched(y[5:]).all())
    big = _sentinel_f32(1031, 131, cuda)                                 # more than one block, an odd leading dimension
    _lib.check(L.pcrcg_fill2d(big.data_ptr(), 131, 1031, 129, 1.0, ops._stream()), "pcrcg_fill2d")
    assert bool((big[:1031, :129] == 1).all()) and bool(_untouched(big[:1031, 129:]).all()) and bool(_untouched(big[1031:]).all())


# ------------------------------------------------------------------------------------------------
# pcrcg_superglue_valid_maps
# ------------------------------------------------------------------------------------------------
def _valid_maps(dev, kp0, kp1, matches, conf, window, size):
    """pcrcg_superglue_valid_maps through ctypes -> (src, tgt) numpy [size], every pixel written, the guard kept."""
    L = _lib.lib()
    n0, n1 = len(kp0), len(kp1)
    k0, k1 = _dev(np.asarray(kp0, F32).reshape(-1, 2), dev), _dev(np.asarray(kp1, F32).reshape(-1, 2), dev)
    m, cf = _dev(np.asarray(matches, np.int64), dev), _dev(np.asarray(conf, F32), dev)
    px = size[0] * size[1]
    out = [torch.full((px + 64,), NAN_BITS, dtype=torch.int32, device=dev).view(torch.float32) for _ in range(2)]
    _lib.check(L.pcrcg_superglue_valid_maps(k0.data_ptr() if n0 else None, n0, k1.data_ptr() if n1 else None, n1,
                                            m.data_ptr() if n0 else None, cf.data_ptr() if n0 else None, int(window), size[0],
                                            size[1], out[0].data_ptr(), out[1].data_ptr(), ops._stream()),
               "pcrcg_superglue_valid_maps")
    for o in out:
        assert bool(_untouched(o[px:]).all()) and not bool(_untouched(o[:px]).any())
    return tuple(o[:px].reshape(size).cpu().numpy() for o in out)


def _axis_classes(length, window):
    """Keypoint coordinates by class along an axis of `length` pixels."""
    w = float(window)
    v = []
    for b in (0.0, float(length)):
        v += [b, b + 0.5, b - 0.5, b + w, b - w, b + w - 0.5, b - w + 0.5, b + w + 0.5, b - w - 0.5, b + w / 2, b - w / 2,
              b + w + 2, b - w - 2, b + w - 0.25, b + w - 1.0]
    v += [w - 0.5, w - 0.25, w - 0.999, 4.5, 3.0, -3.0, -0.5, -1e-3, length / 2.0, length - 1.0, length + 2 * w + 7,
          -2 * w - 7, 1.5 * 2.0 ** 30, -1.5 * 2.0 ** 30, 2.0 ** 31, -2.0 ** 31, 3e9, -3e9, 1e20, -1e20, 3e38, -3e38]
    return np.unique(np.asarray(v, F32))


def _class_keypoints(size, window):
    """Every class on one axis against coordinates on the other that paint a strict, non-empty part of it (w + 1 leaves
    pixel 0 out): (class, part), (part, class) and (part, part)."""
    px, py = ([window + 1.0, window + 1.5] if length > 1 else [0.5] for length in size)      # (one pixel has no strict part)
    xs, ys = _axis_classes(size[0], window), _axis_classes(size[1], window)
    kp = [(x, p) for x in xs for p in py] + [(p, y) for y in ys for p in px] + [(p, q) for p in px for q in py]
    return np.asarray(kp, F32)


@pytest.mark.parametrize("window", [0, 1, 5, 300])
@pytest.mark.parametrize("size", [(160, 120), (7, 5), (1, 1), (3, 200)])
def test_valid_maps_border_classes(cuda, size, window):
    rng = np.random.RandomState(size[0] * 1000 + window)
    kp1 = _class_keypoints(size, window)
    kp0 = kp1[rng.permutation(len(kp1))]
    n0, n1 = len(kp0), len(kp1)
    matches = rng.permutation(n1)[:n0].astype(np.int64)
    matches[rng.rand(n0) < 0.2] = -1
    matches[rng.rand(n0) < 0.2] = matches[3]                    # repeated targets
    matches[:4] = [0, -1, 1, n1 - 1]
    conf = rng.uniform(0.05, 1.0, n0).astype(F32)
    want = PR.paint_valid_maps(kp0, kp1, matches, conf, window, size)
    got = _valid_maps(cuda, kp0, kp1, matches, conf, window, size)
    for g, w_ in zip(got, want):
        assert np.array_equal(g, w_)
        if window == 0:
            assert not w_.any()                                  # start == stop everywhere: the case is empty
        else:
            assert w_.any() and (size == (1, 1) or not w_.all())


def test_valid_maps_dense_overwrites(cuda):
    """About 2000 matches on the 160 x 120 map: later matches overwrite earlier ones almost everywhere."""
    rng = np.random.RandomState(11)
    n0, n1 = 2600, 2100
    kp0 = (rng.rand(n0, 2) * [140, 100] + [10, 10]).astype(F32)          # (a border of 5 pixels stays unpainted)
    kp1 = (rng.rand(n1, 2) * [140, 100] + [10, 10]).astype(F32)
    matches = rng.randint(0, n1, n0).astype(np.int64)
    matches[rng.rand(n0) < 0.23] = -1
    assert 1900 < (matches > -1).sum() < 2100
    conf = rng.uniform(0.05, 1.0, n0).astype(F32)
    want = PR.paint_valid_maps(kp0, kp1, matches, conf)
    got = _valid_maps(cuda, kp0, kp1, matches, conf, 5, (160, 120))
    first = PR.paint_valid_maps(kp0[::-1], kp1, matches[::-1], conf[::-1])        # the same boxes, the other order
    for g, w_, f in zip(got, want, first):
        assert np.array_equal(g, w_)
        assert w_.any() and not w_.all() and (w_ != f).mean() > 0.5


def test_valid_maps_empty_and_dropped_matches(cuda):
    size, window = (160, 120), 5
    rng = np.random.RandomState(2)
    kp = (rng.rand(30, 2) * size).astype(F32)
    # n0 = 0; n1 = 0 with every match -1: zero maps
    for k0, k1, m in ((kp[:0], kp, np.zeros(0, np.int64)), (kp, kp[:0], np.full(30, -1, np.int64))):
        conf = rng.uniform(0.05, 1.0, len(k0)).astype(F32)
        for g in _valid_maps(cuda, k0, k1, m, conf, window, size):
            assert g.shape == size and not g.any()
    # matches[i] >= n1 and non-finite keypoints (on either side of the match) paint nothing, on either map: what the
    # painter gives once those matches are removed
    kp0, kp1 = kp.copy(), (rng.rand(25, 2) * size).astype(F32)
    matches = rng.permutation(25).astype(np.int64).repeat(2)[:30]
    matches[[2, 9]] = [25, 1 << 40]
    kp0[4, 0], kp0[11, 1], kp0[12] = np.nan, np.inf, -np.inf
    kp1[matches[6], 1], kp1[matches[17], 0] = np.nan, np.inf
    conf = rng.uniform(0.05, 1.0, 30).astype(F32)
    drop = (matches >= 25) | ~np.isfinite(kp0).all(1) | ~np.isfinite(kp1[np.clip(matches, 0, 24)]).all(1)
    assert 7 <= drop.sum() <= 12
    cleaned = np.where(drop, -1, matches)
    want = PR.paint_valid_maps(np.nan_to_num(kp0, posinf=0, neginf=0), np.nan_to_num(kp1, posinf=0, neginf=0), cleaned, conf,
                               window, size)
    got = _valid_maps(cuda, kp0, kp1, matches, conf, window, size)
    for g, w_ in zip(got, want):
        assert np.array_equal(g, w_) and w_.any() and not w_.all()
    # dropping only the non-finite SIDE of such a match (painting its finite keypoint) would have shown
    z0, z1 = np.nan_to_num(kp0, posinf=0, neginf=0), np.nan_to_num(kp1, posinf=0, neginf=0)
    src_only = np.where((matches >= 25) | ~np.isfinite(kp0).all(1), -1, matches)
    tgt_only = np.where((matches >= 25) | ~np.isfinite(kp1[np.clip(matches, 0, 24)]).all(1), -1, matches)
    assert (PR.paint_valid_maps(z0, z1, src_only, conf, window, size)[0] != want[0]).any()
    assert (PR.paint_valid_maps(z0, z1, tgt_only, conf, window, size)[1] != want[1]).any()
