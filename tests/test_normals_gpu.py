"""GPU: the normal estimation (csrc/normals.hip, registration.estimate_normals_batch) against the numpy restatement
tests/normals_ref.py: neighbour counts exactly, covariances to float64 rounding, directions where the spectrum defines
them, and the edges of the neighbour search."""
import numpy as np
import pytest
import torch

from pcrcg_amd import registration as REG

from . import normals_ref as NR

pytestmark = pytest.mark.gpu


def _run(pcds, radius, max_nn, viewpoints=None, **kw):
    nrm, cnt, cov = REG.estimate_normals_batch(pcds, radius, max_nn, viewpoints=viewpoints, trace=True, **kw)
    return [(a.cpu().numpy(), b.cpu().numpy(), c.cpu().numpy()) for a, b, c in zip(nrm, cnt, cov)]


def _check(pts, radius, max_nn, got, viewpoint=None, qualify=None, ref=None):
    """One cloud against the restatement -> the restatement.  count: exact.  cov: every entry within 1e-13 * (sum |d|^2 / k)
    (at most 64 float64 roundings per sum, with margin).  Rows: finite, unit to 1e-12, signed by the rule, (0, 0, 1) where the
    definition falls back.  Direction: 1 - |n . n_ref| <= 1e-9 where (l1 - l0) / l2 >= 1e-3 (the eigenvector's perturbation
    bound is ~1e-13 / gap); qualify: the least share of such rows."""
    ref = ref or NR.estimate(pts, radius, max_nn, viewpoint)
    n, cnt, cov = got
    v = np.zeros(3) if viewpoint is None else np.asarray(viewpoint, np.float64)
    assert n.shape == (len(pts), 3) and n.dtype == np.float64
    assert np.array_equal(cnt, ref["count"])
    assert (np.abs(cov - ref["cov"]) <= 1e-13 * ref["scale"][:, None]).all(), np.abs(cov - ref["cov"]).max()
    if len(pts) == 0:
        return ref
    assert np.isfinite(n).all() and np.abs(np.linalg.norm(n, axis=1) - 1.0).max() <= 1e-12
    fb = ref["fallback"]
    assert np.array_equal(n[fb], np.tile([0.0, 0.0, 1.0], (int(fb.sum()), 1)))
    p64 = np.asarray(pts, np.float32).astype(np.float64)
    for i in np.flatnonzero(~fb):
        assert NR.sign_ok(n[i], p64[i], v), i
    ok = NR.well_separated(ref["eig"]) & ~fb
    dev = 1.0 - np.abs((n[ok] * ref["normals"][ok]).sum(1))
    assert (dev <= 1e-9).all(), dev.max()
    # with the direction settled the sign is the restatement's too, unless the viewpoint lies in the tangent plane to rounding
    dots = ((v - p64[ok]) * ref["normals"][ok]).sum(1)
    clear = np.abs(dots) > 1e-6 * np.abs(v - p64[ok]).sum(1)
    assert ((n[ok] * ref["normals"][ok]).sum(1)[clear] > 0).all()
    if qualify is not None:
        assert (ok | fb).mean() >= qualify, ok.mean()
    return ref


CLOUDS = {"sphere": (lambda: NR.noisy_sphere(0), 0.25), "cube": (lambda: NR.cube(0), 0.15),
          "lattice_sphere": (lambda: NR.lattice_sphere(0), 0.25)}


@pytest.mark.parametrize("name", sorted(CLOUDS))
def test_counts_covariances_and_directions(cuda, name):
    make, r = CLOUDS[name]
    pts = make()
    ref = _check(pts, r, 30, _run([pts], r, 30)[0], qualify=0.99)
    if name == "sphere":
        assert ref["count"].min() >= 8 and ref["count"].max() == 30
        radial = pts.astype(np.float64) / np.linalg.norm(pts.astype(np.float64), axis=1, keepdims=True)
        got = REG.estimate_normals(pts, r, 30).cpu().numpy()
        assert np.median(np.abs((got * radial).sum(1))) > 0.999


def test_small_empty_and_block_edge_clouds_in_one_call(cuda):
    sizes = [1, 2, 3, 0, 63, 64, 65, 513]
    clouds = [NR.cube(10 + i, n) * np.float32(0.5) for i, n in enumerate(sizes)]
    got = _run(clouds, 0.2, 30)
    for pts, g in zip(clouds, got):
        ref = _check(pts, 0.2, 30, g)
        if len(pts) < 3:
            assert ref["fallback"].all()
    assert ref["count"].max() == 30                    # (of the 513-point cloud)


@pytest.mark.parametrize("max_nn", [1, 3, 30, 64])
def test_max_nn(cuda, max_nn):
    """400 points, radius 0.4: about 100 points within the radius, so every cut is taken -- and the list of candidates is cut
    once on the way (more than 64 hits)."""
    pts = NR.cube(20, 400)
    ref = _check(pts, 0.4, max_nn, _run([pts], 0.4, max_nn)[0])
    assert ref["count"].max() == max_nn and (ref["count"] == max_nn).mean() > 0.3
    if max_nn < 3:
        assert ref["fallback"].all()


def test_more_hits_than_the_list_holds(cuda):
    """1500 points, radius 0.3: up to ~170 points within the radius, more than the 128 entries a wavefront's list holds."""
    pts = NR.cube(21, 1500)
    full = NR.neighbours(pts, 0.3, 10 ** 6)
    assert max(len(x) for x in full) > 128
    _check(pts, 0.3, 64, _run([pts], 0.3, 64)[0], qualify=0.99)


@pytest.mark.parametrize("max_nn", [4, 10])
def test_a_cut_inside_equal_distances_follows_the_index(cuda, max_nn):
    pts = NR.tie_lattice(0)
    ref = NR.estimate(pts, 1.5 * 0.125, max_nn)
    other = NR.estimate(pts[::-1].copy(), 1.5 * 0.125, max_nn)          # the same points in another index order
    assert not np.allclose(ref["cov"], other["cov"][::-1])              # ... enter other neighbours: the order matters here
    _check(pts, 1.5 * 0.125, max_nn, _run([pts], 1.5 * 0.125, max_nn)[0], ref=ref)


def test_coincident_and_collinear_points(cuda):
    same = np.tile(np.float32([0.5, -1.0, 2.0]), (5, 1))
    t = (np.arange(40, dtype=np.float32) - 20) * np.float32(0.03125)
    line = np.stack([t * np.float32(0.6), t * np.float32(0.8), np.zeros_like(t)], 1)
    got = _run([same, line], 0.2, 30)
    n, cnt, cov = got[0]
    assert (cnt == 5).all() and not cov.any() and np.array_equal(n, np.tile([0.0, 0.0, 1.0], (5, 1)))
    n, cnt, cov = got[1]
    ref = NR.estimate(line, 0.2, 30)
    assert np.array_equal(cnt, ref["count"]) and (np.abs(cov - ref["cov"]) <= 1e-13 * ref["scale"][:, None]).all()
    assert np.isfinite(n).all() and np.abs(np.linalg.norm(n, axis=1) - 1.0).max() <= 1e-12
    assert np.abs(n @ np.array([0.6, 0.8, 0.0])).max() <= 1e-9


def test_a_cloud_far_from_the_origin(cuda):
    """+1000 on every axis: the moments are taken about the query point, so the covariance keeps its bound."""
    pts = (NR.noisy_sphere(3, 800).astype(np.float64) + 1000.0).astype(np.float32)
    _check(pts, 0.25, 30, _run([pts], 0.25, 30)[0])


def test_viewpoints(cuda):
    pts = NR.noisy_sphere(4, 600)
    view = np.array([[0.0, 0.0, 0.0], [10.0, 0.0, 0.0], [0.3, -0.2, 5.0]])
    got = _run([pts, pts, pts], 0.25, 30, viewpoints=view)
    none = _run([pts], 0.25, 30)[0]
    assert got[0][0].tobytes() == none[0].tobytes()
    for b in range(3):
        _check(pts, 0.25, 30, got[b], viewpoint=view[b])
    assert (got[1][0] != got[0][0]).any()
    assert np.array_equal(np.abs(got[1][0]), np.abs(got[0][0]))          # the viewpoint moves signs alone
    one = REG.estimate_normals(pts, 0.25, 30, viewpoint=view[2]).cpu().numpy()
    assert one.tobytes() == got[2][0].tobytes()


def test_a_cloud_alone_and_inside_a_shuffled_batch_bit_for_bit(cuda):
    sizes = [513, 65, 700, 3, 300]
    clouds = [NR.noisy_sphere(30 + i, n) for i, n in enumerate(sizes)]
    order = [3, 0, 4, 2, 1]
    batch = _run([clouds[i] for i in order], 0.3, 30)
    chunked = _run([clouds[i] for i in order], 0.3, 30, pairs_per_call=2)
    for pos, i in enumerate(order):
        alone = _run([clouds[i]], 0.3, 30)[0]
        for a, b, c in zip(alone, batch[pos], chunked[pos]):
            assert a.tobytes() == b.tobytes() == c.tobytes(), i


def test_optional_outputs_do_not_change_the_normals(cuda):
    pts = NR.cube(40, 500)
    plain = REG.estimate_normals_batch([pts], 0.2, 30)
    assert isinstance(plain, list) and plain[0].dtype == torch.float64 and plain[0].is_cuda
    traced = REG.estimate_normals_batch([torch.from_numpy(pts).cuda()], 0.2, 30, trace=True)
    assert torch.equal(plain[0], traced[0][0])
    assert traced[1][0].dtype == torch.int32 and tuple(traced[2][0].shape) == (500, 6)


def test_reads_nothing_back(cuda):
    pts = NR.cube(41, 300)
    reads = REG.D2H_READS
    REG.estimate_normals_batch([pts, pts], 0.2, 30, trace=True)
    assert REG.D2H_READS == reads
