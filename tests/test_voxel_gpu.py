"""GPU: pcrcg_voxel_down_sample_batch against its numpy restatement (tests/voxel_ref.py), BIT for bit -- rows, first
indices, counts and lengths.  Both sides are IEEE float64 with the same operations in the same order, so there is no
tolerance."""
import functools

import numpy as np
import pytest
import torch

from pcrcg_amd import _lib, kitti

from . import voxel_ref as VR

pytestmark = pytest.mark.gpu

CASES = VR.single_cases()


@functools.lru_cache(maxsize=None)
def _ref(name):
    return VR.voxel_down_sample(*CASES[name])


def _bits(t):
    return t.cpu().numpy().tobytes()


def _assert_same(got, ref, what):
    rows, first, count = got
    assert rows.dtype == torch.float64 and tuple(rows.shape) == ref[0].shape, what
    assert _bits(rows) == ref[0].tobytes(), what
    assert first.dtype == torch.int32 and _bits(first) == ref[1].tobytes(), what
    assert count.dtype == torch.int32 and _bits(count) == ref[2].tobytes(), what


def _one(pts, voxel):
    p, f, c = kitti.voxel_down_sample_batch([pts], voxel, with_index=True)
    return p[0], f[0], c[0]


@pytest.mark.parametrize("name", sorted(CASES))
def test_single_cloud_matches_the_restatement_bit_for_bit(cuda, name):
    pts, voxel = CASES[name]
    got = _one(torch.from_numpy(pts).to(cuda), voxel)
    _assert_same(got, _ref(name), name)
    plain = kitti.voxel_down_sample(pts, voxel)               # host input, no index outputs: the same rows
    assert _bits(plain) == _ref(name)[0].tobytes()


def test_ragged_batch_is_cloud_by_cloud_the_single_result(cuda):
    """B = 5 with an empty cloud in the middle and clouds of 1 and 700 points: every cloud's rows are those of the same
    cloud run alone, and of the same cloud at another position of another batch."""
    clouds = [VR.cube(31, 300), VR.cube(32, 1), np.zeros((0, 3), np.float32), VR.cube(33, 700), VR.slab(34, 257)]
    refs = [VR.voxel_down_sample(c, 0.3) for c in clouds]
    batch = kitti.voxel_down_sample_batch(clouds, 0.3, with_index=True)
    assert [len(p) for p in batch[0]] == [len(r[0]) for r in refs] and len(batch[0][2]) == 0
    order = [4, 2, 0, 3, 1]
    moved = kitti.voxel_down_sample_batch([clouds[b] for b in order], 0.3, with_index=True)
    for b in range(5):
        _assert_same([x[b] for x in batch], refs[b], f"cloud {b} in the batch")
        _assert_same(_one(clouds[b], 0.3), refs[b], f"cloud {b} alone")
        _assert_same([x[order.index(b)] for x in moved], refs[b], f"cloud {b} moved")


def _raw(cuda, pts, off, B, voxel, n_total=None, fill=-7):
    """The C entry as it is -> (rc, out_pts [n,3] f64, out_len [B], first [n], count [n]) with outputs pre-filled (NaN / fill)."""
    L = _lib.lib()
    n = len(pts) if n_total is None else n_total
    p = torch.from_numpy(np.ascontiguousarray(pts, np.float32)).to(cuda) if len(pts) else torch.zeros((1, 3), device=cuda)
    o = torch.tensor(off, dtype=torch.int32, device=cuda)
    out = torch.full((max(n, 1), 3), float("nan"), dtype=torch.float64, device=cuda)
    ln = torch.full((B,), fill, dtype=torch.int32, device=cuda)
    first = torch.full((max(n, 1),), fill, dtype=torch.int32, device=cuda)
    count = torch.full((max(n, 1),), fill, dtype=torch.int32, device=cuda)
    wsb = L.pcrcg_voxel_down_sample_ws_bytes(B, n)
    ws = torch.empty(max(wsb, 1), dtype=torch.uint8, device=cuda)
    rc = L.pcrcg_voxel_down_sample_batch(p.data_ptr(), o.data_ptr(), n, B, voxel, out.data_ptr(), ln.data_ptr(), first.data_ptr(),
                                         count.data_ptr(), ws.data_ptr(), wsb, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc, out.cpu().numpy(), ln.cpu().numpy(), first.cpu().numpy(), count.cpu().numpy()


def test_rejected_clouds_leave_the_others_alone(cuda):
    """A batch of three: a cloud with a NaN, a cloud whose extent / voxel reaches 2^21, and an ordinary one.  The first two
    get out_len = -1 and no rows; the third is what it is alone.  The Python wrapper raises and names the cloud."""
    bad = VR.cube(41, 100)
    bad[57, 2] = np.nan
    fine, good = VR.too_fine(0.3), VR.cube(42, 400)
    ref = VR.voxel_down_sample(good, 0.3)
    assert VR.voxel_down_sample(bad, 0.3) is None and VR.voxel_down_sample(fine, 0.3) is None
    for order in ([0, 1, 2], [2, 0, 1], [1, 2, 0]):
        clouds = [[bad, fine, good][k] for k in order]
        ns = [len(c) for c in clouds]
        rc, out, ln, first, count = _raw(cuda, np.concatenate(clouds), np.cumsum([0] + ns), 3, 0.3)
        K = len(ref[0])
        assert rc == 0 and ln.tolist() == [K if k == 2 else -1 for k in order]
        assert out[:K].tobytes() == ref[0].tobytes() and first[:K].tobytes() == ref[1].tobytes()
        assert count[:K].tobytes() == ref[2].tobytes()
        assert np.isnan(out[K:]).all() and (first[K:] == -7).all() and (count[K:] == -7).all()     # no rows of the rejected
        with pytest.raises(ValueError, match=f"cloud {min(order.index(0), order.index(1))} was rejected"):
            kitti.voxel_down_sample_batch(clouds, 0.3)
    inf = VR.cube(43, 10)
    inf[0, 0] = -np.inf
    with pytest.raises(ValueError, match="cloud 0 was rejected"):
        kitti.voxel_down_sample(inf, 0.3)


def test_offsets_outside_the_rows_read_as_empty_clouds(cuda):
    pts = VR.cube(51, 100)
    # cloud 0 = rows 10..60 (rows outside every range belong to no cloud); cloud 1 runs backwards; cloud 2 steps back over
    # cloud 0; cloud 3 ends past n_total
    rc, out, ln, first, count = _raw(cuda, pts, [10, 60, 40, 100, 200], 4, 0.3)
    ref = VR.voxel_down_sample(pts[10:60], 0.3)
    K = len(ref[0])
    assert rc == 0 and ln.tolist() == [K, 0, 0, 0]
    assert out[:K].tobytes() == ref[0].tobytes() and first[:K].tobytes() == ref[1].tobytes() and np.isnan(out[K:]).all()
    rc, out, ln, _, _ = _raw(cuda, pts, [-5, 20, 100], 2, 0.3)
    ref = VR.voxel_down_sample(pts[20:], 0.3)
    assert rc == 0 and ln.tolist() == [0, len(ref[0])] and out[:len(ref[0])].tobytes() == ref[0].tobytes()
    rc, out, ln, _, _ = _raw(cuda, np.zeros((0, 3), np.float32), [0, 0, 0], 2, 0.3)       # n_total = 0
    assert rc == 0 and ln.tolist() == [0, 0] and np.isnan(out).all()


def test_entry_point_errors(cuda):
    """PCRCG_EBADARG / PCRCG_EWORKSPACE through the raw entry, with real device buffers: nothing is launched, the outputs
    keep their fill."""
    L = _lib.lib()
    pts = torch.from_numpy(VR.cube(61, 64)).to(cuda)
    off = torch.tensor([0, 64], dtype=torch.int32, device=cuda)
    out = torch.full((64, 3), float("nan"), dtype=torch.float64, device=cuda)
    ln = torch.full((1,), -7, dtype=torch.int32, device=cuda)
    wsb = L.pcrcg_voxel_down_sample_ws_bytes(1, 64)
    ws = torch.empty(wsb, dtype=torch.uint8, device=cuda)
    st = torch.cuda.current_stream().cuda_stream
    ok = dict(pts=pts.data_ptr(), off=off.data_ptr(), n=64, B=1, vs=0.3, out=out.data_ptr(), ln=ln.data_ptr(), ws=ws.data_ptr(),
              wsb=wsb)

    def call(**kw):
        a = dict(ok, **kw)
        return L.pcrcg_voxel_down_sample_batch(a["pts"], a["off"], a["n"], a["B"], a["vs"], a["out"], a["ln"], None, None, a["ws"],
                                               a["wsb"], st)

    for kw in (dict(pts=None), dict(off=None), dict(out=None), dict(ln=None), dict(ws=None), dict(B=0), dict(B=65536), dict(n=-1),
               dict(vs=0.0), dict(vs=-1.0), dict(vs=float("nan")), dict(vs=float("inf"))):
        assert call(**kw) == -1, kw                                                    # PCRCG_EBADARG
    assert call(wsb=wsb - 1) == -2 and call(wsb=0) == -2                               # PCRCG_EWORKSPACE
    torch.cuda.synchronize()
    assert torch.isnan(out).all() and int(ln[0]) == -7
    assert call() == 0
    torch.cuda.synchronize()
    ref = VR.voxel_down_sample(pts.cpu().numpy(), 0.3)
    assert int(ln[0]) == len(ref[0]) and out[:len(ref[0])].cpu().numpy().tobytes() == ref[0].tobytes()
