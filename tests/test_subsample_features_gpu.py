"""GPU: grid subsampling with features and classes (ops.grid_subsample_ex, the cpp_subsampling shim, the C ABI) against
the unmodified reference's outputs (tests/golden/subsample_features.npz) and, on fresh inputs, against the numpy
restatement that test_subsample_features_cpu.py pins to it.  Every comparison is exact; floats are compared through
their bit patterns."""
import os

import numpy as np
import pytest
import torch

from pcrcg_amd import _lib, ops
from pcrcg_amd.cpp_wrappers.cpp_subsampling import grid_subsampling as G
from tests import subsample_ref as R

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "subsample_features.npz")
CASES = {c["name"]: c for c in R.fixture_cases()}


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(GOLDEN))


def _dev(a, cuda):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(cuda)


def _run(case, cuda):
    """-> (points, lengths, features or None, classes or None) as numpy, through ops.grid_subsample_ex"""
    out = ops.grid_subsample_ex(_dev(case["points"], cuda), _dev(case["lengths"], cuda), case["dl"], case["max_p"],
                                _dev(case["features"], cuda), _dev(case["classes"], cuda))
    return [None if t is None else t.cpu().numpy() for t in out]


def _same(got, want):
    for g, w in zip(got, want):
        assert (g is None) == (w is None)
        if g is not None:
            assert g.dtype == w.dtype and g.shape == w.shape
            assert np.array_equal(g.view(np.int32), w.view(np.int32))


# cases 1, 2, 3, 5 (without the empty cloud), 6 and 7 of the issue, each against what the reference returned
@pytest.mark.parametrize("name", sorted(CASES))
def test_equals_the_reference(cuda, golden, name):
    case = CASES[name]
    want = [golden.get(name + "/" + k) for k in ("points", "lengths", "features", "classes")]
    _same(_run(case, cuda), want)
    if name == "single_cell_5000":
        assert want[0].shape[0] == 1                      # one segment of 5 000 points, far longer than a wavefront


@pytest.mark.parametrize("fdim", R.FDIMS)
def test_feature_widths_on_fresh_input(cuda, fdim):
    """tail lanes, several rows per wavefront (fdim < 64), column blocks (fdim > 64), 16-byte reads on (4, 32, 64) and off"""
    rs = np.random.RandomState(100 + fdim)
    n = 700
    p = rs.rand(n, 3).astype(np.float32)
    f = (np.float32(1e8) + rs.randint(0, 64, (n, fdim))).astype(np.float32)
    case = dict(points=p, lengths=np.array([400, 300], np.int32), dl=0.15, max_p=0, features=f, classes=None)
    want = R.subsample_ref(p, case["lengths"], 0.15, 0, f, None)
    assert want[0].shape[0] > 256
    _same(_run(case, cuda), want)


@pytest.mark.parametrize("fdim", [4, 5, 64])
def test_row_stride_and_advanced_pointers_through_the_c_abi(cuda, fdim):
    """ld_feat = fdim + 3 and base pointers that are not 16-byte aligned: the wide reads must switch themselves off"""
    rs = np.random.RandomState(7 + fdim)
    n, ld = 300, fdim + 3
    p = rs.rand(n, 3).astype(np.float32)
    wide = rs.randn(n, ld).astype(np.float32)
    c = rs.randint(-2, 3, n).astype(np.int32)
    lens = np.array([n], np.int32)
    want = R.subsample_ref(p, lens, 0.2, 0, wide[:, :fdim], c)
    L = _lib.lib()
    pad = 1                                               # every array starts one element into its allocation
    d_p, d_f, d_c = (torch.zeros(a.size + pad, dtype=t, device=cuda) for a, t in
                     ((p, torch.float32), (wide, torch.float32), (c, torch.int32)))
    d_p[pad:] = _dev(p.ravel(), cuda)
    d_f[pad:] = _dev(wide.ravel(), cuda)
    d_c[pad:] = _dev(c, cuda)
    d_len = _dev(lens, cuda)
    o_p = torch.full((n * 3 + pad,), -7.0, device=cuda)
    o_f = torch.full((n * fdim + pad,), -7.0, device=cuda)
    o_c = torch.full((n + pad,), -7, dtype=torch.int32, device=cuda)
    o_len, o_m = torch.zeros(1, dtype=torch.int32, device=cuda), torch.zeros(1, dtype=torch.int32, device=cuda)
    nbytes = L.pcrcg_grid_subsample_ex_ws_bytes(n, 1, fdim, 1)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=cuda)
    rc = L.pcrcg_grid_subsample_batch_ex(d_p.data_ptr() + 4, n, d_len.data_ptr(), 1, 0.2, 0, d_f.data_ptr() + 4, fdim, ld,
                                         d_c.data_ptr() + 4, 1, o_p.data_ptr() + 4, o_len.data_ptr(), o_m.data_ptr(),
                                         o_f.data_ptr() + 4, o_c.data_ptr() + 4, ws.data_ptr(), nbytes,
                                         torch.cuda.current_stream().cuda_stream)
    assert rc == 0, L.pcrcg_last_error()
    m = int(o_m.item())
    assert m == want[0].shape[0] and o_len.tolist() == [m]
    _same([o_p[pad:pad + 3 * m].cpu().numpy().reshape(m, 3), o_f[pad:pad + m * fdim].cpu().numpy().reshape(m, fdim),
           o_c[pad:pad + m].cpu().numpy().reshape(m, 1)], [want[0], want[2], want[3]])
    # nothing before the arrays, nothing behind the rows written
    assert float(o_p[0]) == -7.0 and float(o_f[0]) == -7.0 and int(o_c[0]) == -7
    assert (o_f[pad + m * fdim:] == -7.0).all() and (o_c[pad + m:] == -7).all()
    # a too small workspace is refused, not overrun
    assert L.pcrcg_grid_subsample_batch_ex(d_p.data_ptr() + 4, n, d_len.data_ptr(), 1, 0.2, 0, d_f.data_ptr() + 4, fdim, ld,
                                           d_c.data_ptr() + 4, 1, o_p.data_ptr() + 4, o_len.data_ptr(), o_m.data_ptr(),
                                           o_f.data_ptr() + 4, o_c.data_ptr() + 4, ws.data_ptr(),
                                           L.pcrcg_grid_subsample_ws_bytes(n, 1), None) == -2


@pytest.mark.parametrize("max_p", [0, 10])
def test_three_clouds_one_of_them_empty(cuda, max_p):
    """lengths and row offsets around an empty cloud (which the reference cannot run: here it yields no rows); the cap
    falls on the same rows for points, features and classes"""
    rs = np.random.RandomState(5)
    lens = np.array([150, 0, 400], np.int32)
    n = int(lens.sum())
    p, f, c = rs.rand(n, 3).astype(np.float32), (rs.randn(n, 3) * 100).astype(np.float32), rs.randint(0, 6, n).astype(np.int32)
    case = dict(points=p, lengths=lens, dl=0.25, max_p=max_p, features=f, classes=c)
    want = R.subsample_ref(p, lens, 0.25, max_p, f, c)
    got = _run(case, cuda)
    _same(got, want)
    assert got[1][1] == 0 and (got[1].tolist() == [10, 0, 10] if max_p else got[1].min() == 0 and got[1].max() > 10)
    if max_p:
        full = _run(dict(case, max_p=0), cuda)
        lo = 0
        for b, m in enumerate(full[1]):
            keep, at = min(int(m), 10), int(got[1][:b].sum())
            for k in (0, 2, 3):
                assert np.array_equal(got[k][at:at + keep].view(np.int32), full[k][lo:lo + keep].view(np.int32))
            lo += int(m)


def test_fresh_labels_small_and_large_cells(cuda):
    """cells of 1 ... 13 points (voted by one lane) beside cells of 14 and more, up to 76 (voted by a wavefront, with
    dozens of distinct labels: bucket stages 13 and 29; the fixture's labels_150 goes on to 257), negative labels, two
    label columns on one cloud"""
    rs = np.random.RandomState(11)
    n = 3000
    p = rs.rand(n, 3).astype(np.float32)
    p[:1500] *= np.float32(0.3)                           # a dense corner: large cells
    for k, size in enumerate((13, 14)):                   # and, apart from the rest, one cell on either side of the threshold
        at = 2000 + 20 * k
        p[at:at + size] = np.float32([2.05 + 0.2 * k, 0.05, 0.05]) + (rs.rand(size, 3).astype(np.float32) - 0.5) * np.float32(0.06)
    c = np.stack([rs.randint(-60, 60, n), rs.randint(-2, 2, n) * 1000003], 1).astype(np.int32)
    lens = np.array([n], np.int32)
    want = R.subsample_ref(p, lens, 0.1, 0, None, c)
    got = _run(dict(points=p, lengths=lens, dl=0.1, max_p=0, features=None, classes=c), cuda)
    _same(got, want)
    sizes = np.bincount(np.unique(np.floor(p / np.float32(0.1)).astype(np.int64) @ [1, 100, 10000], return_inverse=True)[1])
    assert sizes.min() <= 2 and (sizes == 13).any() and (sizes == 14).any() and sizes.max() > 64


@pytest.mark.parametrize("with_f, with_c", [(True, False), (False, True), (True, True)], ids=["features", "classes", "both"])
def test_points_are_those_of_the_points_only_call(cuda, with_f, with_c):
    case = CASES["three_clouds"]
    p, l = _dev(case["points"], cuda), _dev(case["lengths"], cuda)
    base_p, base_l = ops.grid_subsample(p, l, case["dl"], 0)
    sp, sl, sf, sc = ops.grid_subsample_ex(p, l, case["dl"], 0, _dev(case["features"], cuda) if with_f else None,
                                           _dev(case["classes"], cuda) if with_c else None)
    assert torch.equal(sp, base_p) and torch.equal(sl, base_l)
    assert (sf is not None) == with_f and (sc is not None) == with_c
    again_p, again_l = ops.grid_subsample(p, l, case["dl"], 0)        # and the shared workspace leaves nothing behind
    assert torch.equal(again_p, base_p) and torch.equal(again_l, base_l)


def test_shim_numpy_in_numpy_out(cuda, golden):
    """tuples in the reference's order; 1-D classes come back [M, 1]"""
    c = CASES["three_clouds"]
    want = [golden["three_clouds/" + k] for k in ("points", "lengths", "features", "classes")]
    got = G.subsample_batch(c["points"], c["lengths"], features=c["features"], classes=c["classes"], sampleDl=c["dl"])
    assert isinstance(got, tuple) and len(got) == 4 and all(isinstance(a, np.ndarray) for a in got)
    _same(got, want)
    assert c["classes"].ndim == 1 and got[3].shape == (want[0].shape[0], 1)
    got = G.subsample_batch(c["points"], c["lengths"], features=c["features"], sampleDl=c["dl"], max_p=10)
    assert len(got) == 3
    _same(got, [golden["three_clouds_cap10/" + k] for k in ("points", "lengths", "features")])
    got = G.subsample_batch(c["points"].tolist(), c["lengths"].tolist(), classes=c["classes"].tolist(), sampleDl=c["dl"])
    assert len(got) == 3
    _same(got, [want[0], want[1], want[3]])
    assert len(G.subsample_batch(c["points"], c["lengths"], sampleDl=c["dl"])) == 2

    s = CASES["ldim2_single"]
    want = [golden["ldim2_single/" + k] for k in ("points", "features", "classes")]
    got = G.subsample(s["points"], features=s["features"], classes=s["classes"], sampleDl=s["dl"])
    assert isinstance(got, tuple) and len(got) == 3
    _same(got, want)
    got = G.subsample(s["points"], classes=s["classes"], sampleDl=s["dl"])
    _same(got, [want[0], want[2]])
    got = G.subsample(s["points"], features=s["features"], sampleDl=s["dl"])
    _same(got, [want[0], want[1]])
    assert isinstance(G.subsample(s["points"], sampleDl=s["dl"]), np.ndarray)
    # wide classes on ONE cloud pass through the batch entry too
    got = G.subsample_batch(s["points"], s["lengths"], classes=s["classes"], sampleDl=s["dl"])
    _same(got, [want[0], golden["ldim2_single/lengths"], want[2]])


def test_shim_device_in_device_out(cuda, golden):
    c = CASES["three_clouds"]
    d = {k: _dev(c[k], cuda) for k in ("points", "lengths", "features", "classes")}
    got = G.subsample_batch(d["points"], d["lengths"], features=d["features"][:, :2].t().contiguous().t(), classes=d["classes"],
                            sampleDl=c["dl"])
    assert len(got) == 4 and all(isinstance(t, torch.Tensor) and t.is_cuda for t in got)
    want = R.subsample_ref(c["points"], c["lengths"], c["dl"], 0, c["features"][:, :2], c["classes"])
    _same([t.cpu().numpy() for t in got], want)
    one = G.subsample(d["points"][:150], features=d["features"][:150], sampleDl=c["dl"])
    assert isinstance(one, tuple) and len(one) == 2 and all(t.is_cuda for t in one)
    m = int(golden["three_clouds/lengths"][0])
    _same([t.cpu().numpy() for t in one], [golden["three_clouds/points"][:m], golden["three_clouds/features"][:m]])
