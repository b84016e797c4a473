"""CPU: the numpy restatement of PCR-CG's projection (tests/projection_ref.py) against the UNMODIFIED reference's output
(tests/golden/projection.npz, scripts/make_golden_projection.py), the valid-map painter against the fixture's maps, and the
argument checks of the projection entries of the C ABI (nothing is launched)."""
import ctypes
import os

import numpy as np
import pytest
import torch

from pcrcg_amd import _lib
from pcrcg_amd.ops import ImageFrame, matrix16

from . import projection_ref as PR

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def gold():
    return PR.load_fixture(GOLDEN)


def test_restatement_reproduces_the_reference(gold):
    assert len(gold["projection"]) == 5
    for c in gold["projection"]:
        i2, i3 = PR.project(c["points"].numpy(), c["depth"].numpy(), c["world2camera"].numpy(), c["intrinsics"].numpy())
        assert np.array_equal(i2, c["inds2d"].numpy()), c["name"]
        assert np.array_equal(i3, c["inds3d"].numpy()), c["name"]
        assert 0 < len(i3) < c["points"].shape[0], c["name"]          # the depth test rejects a share of every case


def test_restatement_reproduces_the_reference_at_the_edges():
    """tests/golden/projection_edges.npz: the reference's own decisions on inputs with exact arithmetic -- quotients at -1,
    in (-1, 0), at w / h and one ulp below, z = 0, z < 0, non-finite coordinates, |z - d| at thresh, thresh = 0, NaN / inf
    / 0 depths, a 37 x 53 and a 1 x 1 frame."""
    cases = PR.load_edges(GOLDEN)
    assert len(cases) == 23 and sum(len(c["points"]) for c in cases) == 3270
    for c in cases:
        i2, i3 = PR.project(c["points"], c["depth"], c["world2camera"], c["intrinsics"], c["thresh"])
        assert np.array_equal(i2, c["inds2d"]), c["name"]
        assert np.array_equal(i3, c["inds3d"]), c["name"]
    kept = {c["name"]: len(c["inds3d"]) for c in cases}
    assert 0 < kept["borders_f1_z1.0"] < 138 and 0 < kept["frame_37x53"] < 2079 and kept["frame_1x1"] == 25
    assert kept["thresh0.0_d1"] == kept["thresh0.0_d0"] == kept["behind_z-0.125"] == 0 and kept["behind_perm"] == 12


def test_fixture_tells_the_rounding_apart(gold):
    """Unfused products (round after every multiply and add) change the result on the composed poses: the fixture pins the
    fused chain, not just "some float32 arithmetic"."""
    def unfused(m, p):
        m = np.asarray(m, np.float32)
        return np.stack([((m[r, 0] * p[:, 0] + m[r, 1] * p[:, 1]) + m[r, 2] * p[:, 2]) + m[r, 3] for r in range(3)], 1)
    differs = 0
    for c in gold["projection"]:
        if "composed" not in c["name"]:
            continue
        p = c["points"].numpy()
        differs += int((unfused(c["world2camera"].numpy(), p) != PR.mm_rows(c["world2camera"].numpy(), p)).sum())
    assert differs > 0


def test_fma_is_exact():
    rng = np.random.RandomState(0)
    a, b, c = (rng.randn(4096).astype(np.float32) for _ in range(3))
    got = PR.fmaf(a, b, c)
    from fractions import Fraction
    for j in range(0, 4096, 97):
        exact = Fraction(float(a[j])) * Fraction(float(b[j])) + Fraction(float(c[j]))
        lo = np.float32(float(exact))                        # float(Fraction) is correctly rounded to f64 ...
        cands = [np.nextafter(lo, np.float32(-np.inf)), lo, np.nextafter(lo, np.float32(np.inf))]
        best = min(cands, key=lambda v: (abs(Fraction(float(v)) - exact), int(np.float32(v).view(np.uint32)) & 1))
        assert got[j] == best, j                             # ... and this picks the nearest f32, ties to even


def test_painter_reproduces_the_fixture_maps(gold):
    for v in gold["valid_maps"]:
        s, t = PR.paint_valid_maps(v["keypoints0"].numpy(), v["keypoints1"].numpy(), v["matches"].numpy(),
                                   v["confidence"].numpy(), gold["window"])
        assert np.array_equal(s, v["src_valid"].numpy()) and np.array_equal(t, v["tgt_valid"].numpy())
    # numpy's slice rules: a keypoint at x < 5 paints nothing on that axis (the start counts from the end)
    s, _ = PR.paint_valid_maps(np.array([[3.0, 60.0]], np.float32), np.array([[80.0, 60.0]], np.float32),
                               np.array([0]), np.array([0.5], np.float32))
    assert not s.any()


P = ctypes.c_void_p(256)      # a non-null dummy: every call below is rejected before anything touches it


def _frame(h=120, w=160, dh=120, dw=160, target=0, fmap=P, depth=P):
    return ImageFrame(fmap.value if fmap else None, depth.value if depth else None, None, matrix16(torch.eye(4)),
                      matrix16(torch.eye(3)), 0.1, h, w, dh, dw, target)


def _inject(frames, n=10, len_src=5, c=128, ldx=132, points=P, x=P):
    lib = _lib.lib()
    arr = (ImageFrame * max(len(frames), 1))(*frames)
    return lib.pcrcg_inject_frames(points, n, len_src, ctypes.cast(arr, ctypes.c_void_p), len(frames), c, x, ldx, None)


def test_projection_entries_reject_bad_arguments():
    lib = _lib.lib()
    m16 = matrix16(torch.eye(4))
    ws_n = lib.pcrcg_project_depth_ws_bytes(1000)
    assert ws_n >= 2 * 4 * 1000
    args = dict(points=P, n=1000, depth=P, h=120, w=160, w2c=m16, K=m16, i2=P, i3=P, k=P, ws=P)

    def proj(**over):
        a = {**args, **over}
        return lib.pcrcg_project_depth(a["points"], a["n"], a["depth"], a["h"], a["w"], a["w2c"], a["K"], 0.1, a["i2"],
                                       a["i3"], a["k"], a["ws"], ws_n, None)
    for over in (dict(points=None), dict(depth=None), dict(w2c=None), dict(K=None), dict(i2=None), dict(i3=None),
                 dict(k=None), dict(ws=None), dict(h=0), dict(w=-1), dict(n=-1), dict(h=1 << 16, w=1 << 16)):
        assert proj(**over) == -1, over
        assert b"bad argument" in lib.pcrcg_last_error()
    assert lib.pcrcg_project_depth(P, 1000, P, 120, 160, m16, m16, 0.1, P, P, P, P, ws_n - 256, None) == -2

    assert _inject([_frame(h=0)]) == -1
    assert _inject([_frame(w=-3, dw=-3)]) == -1
    assert _inject([_frame(dh=119)]) == -1                  # depth and fmap of different sizes
    assert _inject([_frame(dw=80)]) == -1
    assert _inject([_frame(fmap=None)]) == -1
    assert _inject([_frame(depth=None)]) == -1
    assert _inject([_frame(target=2)]) == -1
    assert _inject([_frame(target=1)] * 4) == -1            # more than 3 frames of one side
    assert _inject([_frame(target=0)] * 3 + [_frame(target=1)] * 4) == -1
    assert _inject([_frame()], points=None) == -1
    assert _inject([_frame()], x=None) == -1
    assert _inject([_frame()], ldx=128) == -1               # ldx < c + 1
    assert _inject([_frame()], len_src=11) == -1
    assert b"bad argument" in lib.pcrcg_last_error()

    def sg(**over):
        a = dict(k0=P, n0=10, k1=P, n1=10, m=P, c=P, window=5, mw=160, mh=120, s=P, t=P)
        a.update(over)
        return lib.pcrcg_superglue_valid_maps(a["k0"], a["n0"], a["k1"], a["n1"], a["m"], a["c"], a["window"], a["mw"],
                                              a["mh"], a["s"], a["t"], None)
    for over in (dict(k0=None), dict(k1=None), dict(m=None), dict(c=None), dict(s=None), dict(t=None), dict(mw=0),
                 dict(mh=-1), dict(window=-1), dict(n0=-1)):
        assert sg(**over) == -1, over
