"""CPU: the host side of the 3DMatch pair preparation (pcrcg_amd/indoor.py) -- the restated nearest resize against PIL's
output (tests/golden/indoor_frames.npz, and PIL itself where it imports), adjust_intrinsic against hand-computed values,
the order in which augment_draws consumes the generator, the relabelling of rot / trans, and the argument errors that are
raised before anything touches a device."""
import numpy as np
import pytest

from pcrcg_amd import indoor, indoor_config

from . import indoor_ref as IR


@pytest.fixture(scope="module")
def gold(golden_dir):
    return IR.load_golden(golden_dir)


def test_golden_holds_the_edge_values(gold):
    inputs = IR.golden_inputs()
    for name, frames in inputs.items():
        assert gold[name].dtype == frames.dtype and np.array_equal(gold[name], frames), name
        assert gold[name + "_resized"].shape[1:3] == IR.GOLDEN_SIZES[name]
    depth = np.concatenate([gold["depth_odd_resized"].ravel(), gold["depth_big_resized"].ravel()])
    for v in (0, 1, 32767, 32768, 65535):
        assert (depth == v).any(), v
    assert (gold["color_resized"] == 0).any() and (gold["color_resized"] == 255).any()


def test_restated_resize_equals_the_golden(gold):
    for name, size in IR.GOLDEN_SIZES.items():
        for k, frame in enumerate(gold[name]):
            assert np.array_equal(IR.resize_nearest(frame, size), gold[name + "_resized"][k]), (name, k)
    # ToTensor's values at the edges: int16 reading of the depth, / 255 of the colour
    d = IR.depth_to_tensor(np.array([[0, 1, 32767, 32768, 65535]], np.uint16), (1, 5))
    want = np.array([[0, 1, 32767, -32768, -1]], np.float32) / np.float32(1000)
    assert d.dtype == np.float32 and d.tobytes() == want.tobytes() and d[0, 4] == np.float32(-0.001)
    c = IR.color_to_tensor(np.array([[[0, 128, 255]]], np.uint8), (1, 1))
    assert c.shape == (3, 1, 1) and c[0, 0, 0] == 0.0 and c[2, 0, 0] == 1.0 and c[1, 0, 0] == np.float32(128) / np.float32(255)


def test_restated_resize_equals_pil():
    Image = pytest.importorskip("PIL.Image")
    rng = np.random.RandomState(4)
    cases = [((7, 11), (3, 4), np.uint16), ((48, 64), (12, 16), np.uint16), ((48, 64, 3), (24, 32), np.uint8),
             ((480, 640), (120, 160), np.uint16), ((480, 640, 3), (240, 320), np.uint8), ((9, 5), (4, 3), np.uint8)]
    for shape, size, dtype in cases:
        frame = rng.randint(0, np.iinfo(dtype).max + 1, shape).astype(dtype)
        pil = np.asarray(Image.fromarray(frame).resize((size[1], size[0]), Image.NEAREST))
        assert np.array_equal(IR.resize_nearest(frame, size), pil), (shape, size)


def test_adjust_intrinsic():
    K = np.array([[585.0, 0.0, 320.0], [0.0, 585.0, 240.0], [0.0, 0.0, 1.0]])
    for fn in (indoor.adjust_intrinsic, IR.adjust_intrinsic):
        got = fn(K, [640, 480], [160, 120])
        want = np.array([[585.0 * (160.0 / 640.0), 0.0, 320.0 * (159.0 / 639.0)],
                         [0.0, 585.0 * (120.0 / 480.0), 240.0 * (119.0 / 479.0)], [0.0, 0.0, 1.0]])
        assert got.dtype == np.float64 and np.array_equal(got, want) and got[0, 0] == 146.25
        assert K[0, 0] == 585.0                                          # (a copy: the input is left alone)
        # unequal ratios: 0.5 in width, 0.75 in height -> the smaller one scales both axes (640x480 -> 320x240)
        K2 = np.array([[500.0, 0.0, 310.0], [0.0, 520.0, 250.0], [0.0, 0.0, 1.0]])
        got = fn(K2, [640, 480], [320, 360])
        want = np.array([[500.0 * (320.0 / 640.0), 0.0, 310.0 * (319.0 / 639.0)],
                         [0.0, 520.0 * (240.0 / 480.0), 250.0 * (239.0 / 479.0)], [0.0, 0.0, 1.0]])
        assert np.array_equal(got, want)
        # ... and 0.5 in width, 0.25 in height (640x480 -> 160x120)
        got = fn(K2, [640, 480], [320, 120])
        assert got[0, 0] == 125.0 and got[1, 1] == 130.0 and got[0, 2] == 310.0 * (159.0 / 639.0) and got[1, 2] == 250.0 * (119.0 / 479.0)
        assert fn(K, [640, 480], [640, 480]) is K


def test_world2camera_chain_is_the_restated_one():
    rng = np.random.RandomState(2)
    poses = []
    for _ in range(3):
        q, _r = np.linalg.qr(rng.randn(3, 3))
        p = np.eye(4)
        p[:3, :3], p[:3, 3] = q, rng.randn(3)
        poses.append(p)
    w1 = np.eye(4, dtype=np.float32)
    w1[:3, :3] = np.linalg.qr(rng.randn(3, 3))[0].astype(np.float32)
    for n in (1, 2, 3):
        got, want = indoor.world2camera_chain(poses[:n], w1), IR.pose_chain(poses[:n], w1)
        assert len(got) == n
        for g, w in zip(got, want):
            assert g.dtype.is_floating_point and g.numpy().dtype == np.float32 and np.abs(g.numpy() - w).max() <= 4e-6
    # the association order: pose_2^-1 . (pose_1 . w1), a product with pose_1 first
    full = np.linalg.inv(poses[1]) @ poses[0] @ w1.astype(np.float64)
    assert np.abs(indoor.world2camera_chain(poses[:2], w1)[1].numpy() - full).max() <= 1e-5
    with pytest.raises(ValueError):
        indoor.world2camera_chain(poses + poses[:1], w1)


@pytest.mark.parametrize("n_src,n_tgt", [(500, 700), (30001, 700), (30001, 30500)])
def test_augment_draws_consumes_the_generator_in_the_reference_order(n_src, n_tgt):
    cfg = indoor_config(augment_noise=0.005)
    a, b = np.random.RandomState(9), np.random.RandomState(9)
    d = indoor.augment_draws(n_src, n_tgt, cfg, a)
    # by hand, ref:datasets/indoor.py:142-168
    perm_s = b.permutation(n_src)[:30000] if n_src > 30000 else None
    perm_t = b.permutation(n_tgt)[:30000] if n_tgt > 30000 else None
    euler = b.rand(3) * np.pi * 2
    side = b.rand(1)[0]
    noise_s = (b.rand(min(n_src, 30000), 3) - 0.5) * 0.005
    noise_t = (b.rand(min(n_tgt, 30000), 3) - 0.5) * 0.005
    for got, want in ((d["perm_src"], perm_s), (d["perm_tgt"], perm_t)):
        assert (got is None and want is None) or np.array_equal(got, want)
    assert np.array_equal(d["euler"], euler) and d["rotate_src"] == bool(side > 0.5)
    assert np.array_equal(d["noise_src"], noise_s) and np.array_equal(d["noise_tgt"], noise_t)
    assert np.array_equal(d["rot"], IR.euler_zyx(euler))
    assert a.rand() == b.rand()                                           # the generator stands where the reference's would


@pytest.mark.parametrize("seed", [0, 1, 2, 3, 5, 6])
def test_relabelled_transform_maps_the_augmented_clouds(seed):
    """rot', trans' map the augmented source onto the augmented target wherever rot, trans mapped the originals (noise off:
    it moves both sides independently).  Seeds cover both sides: three rotate the source, three the target."""
    rng = np.random.RandomState(100 + seed)
    src = rng.rand(400, 3) * 2.0
    rot = np.linalg.qr(rng.randn(3, 3))[0]
    trans = rng.randn(3, 1)
    tgt = src @ rot.T + trans.T                                           # rot, trans map src onto tgt exactly (to rounding)
    a = IR.augment(src, tgt, rot, trans, 0.0, np.random.RandomState(seed))
    assert a["rotate_src"] == (seed in (0, 3, 5)), "the seeds no longer cover both sides evenly"
    resid = np.abs(a["src"] @ a["rot"].T + a["trans"].T - a["tgt"]).max()
    assert resid <= 1e-12, resid
    # frame 1's world2camera undoes the rotation of the rotated side
    back = a["src" if a["rotate_src"] else "tgt"] @ a["src_world2camera1" if a["rotate_src"] else "tgt_world2camera1"][:3, :3].astype(np.float64).T
    assert np.abs(back - (src if a["rotate_src"] else tgt)).max() <= 1e-6
    other = a["tgt_world2camera1" if a["rotate_src"] else "src_world2camera1"]
    assert np.array_equal(other, np.eye(4, dtype=np.float32))
    # the product's host side (indoor.relabel) from the product's draws: the same property, and the restatement's values
    d = indoor.augment_draws(400, 400, indoor_config(augment_noise=0.0), np.random.RandomState(seed))
    assert np.array_equal(d["rot"], a["rot_ab"]) and d["rotate_src"] == a["rotate_src"]
    rot2, trans2, w_src, w_tgt = indoor.relabel(rot, trans, d)
    moved_s = src @ d["rot"].T if d["rotate_src"] else src
    moved_t = tgt if d["rotate_src"] else tgt @ d["rot"].T
    resid = np.abs(moved_s @ rot2.T + trans2.T - moved_t).max()
    assert rot2.dtype == np.float64 and trans2.shape == (3, 1) and resid <= 1e-12, resid
    assert np.array_equal(rot2, a["rot"]) and np.array_equal(trans2, a["trans"])
    assert np.array_equal(w_src.numpy(), a["src_world2camera1"]) and np.array_equal(w_tgt.numpy(), a["tgt_world2camera1"])


def test_argument_errors_come_before_any_device_work():
    cfg = indoor_config()
    pts = np.zeros((10, 3), np.float32)
    eye, t0 = np.eye(3), np.zeros(3)
    with pytest.raises(ValueError, match="list lengths differ"):
        indoor.prepare_pairs([pts, pts], [pts], [eye, eye], [t0, t0], cfg)
    with pytest.raises(ValueError, match="list lengths differ"):
        indoor.prepare_pairs([pts], [pts], [eye], [t0, t0], cfg)
    with pytest.raises(ValueError, match="no pairs"):
        indoor.prepare_pairs([], [], [], [], cfg)
    with pytest.raises(ValueError, match=r"\[N, 3\]"):
        indoor.prepare_pairs([np.zeros((10, 2), np.float32)], [pts], [eye], [t0], cfg)
    colour, depth, pose = np.zeros((48, 64, 3), np.uint8), np.zeros((48, 64), np.uint16), np.eye(4)
    K = np.eye(3)
    for n in (0, 4):
        fr = {"src": [(colour, depth, pose)] * n, "tgt": [(colour, depth, pose)] * n, "intrinsics": K}
        with pytest.raises(ValueError, match="img_num must be 1, 2 or 3"):
            indoor.prepare_pairs([pts], [pts], [eye], [t0], cfg, frames=[fr], matches=[[]])
    fr = {"src": [(colour, depth, pose)] * 2, "tgt": [(colour, depth, pose)], "intrinsics": K}
    with pytest.raises(ValueError, match="others have"):
        indoor.prepare_pairs([pts], [pts], [eye], [t0], cfg, frames=[fr], matches=[[]])
    fr = {"src": [(colour, depth, pose)], "tgt": [(colour, depth, pose)], "intrinsics": K}
    with pytest.raises(ValueError, match="frames has 1 entries for 2 pairs"):
        indoor.prepare_pairs([pts, pts], [pts, pts], [eye, eye], [t0, t0], cfg, frames=[fr], matches=[[], []])
    with pytest.raises(ValueError, match="needs SuperGlue"):
        indoor.prepare_pairs([pts], [pts], [eye], [t0], cfg, frames=[fr])
    # prepare_frames: a frame of the wrong rank, mixed sizes, a wrong dtype, nothing at all
    with pytest.raises(ValueError, match=r"must be \[H, W, 3\]"):
        indoor.prepare_frames([np.zeros((48, 64), np.uint8)], [])
    with pytest.raises(ValueError, match=r"must be \[H, W\]"):
        indoor.prepare_frames([], [np.zeros((48, 64, 1), np.uint16)])
    with pytest.raises(ValueError, match="share one size"):
        indoor.prepare_frames([colour, np.zeros((24, 64, 3), np.uint8)], [])
    with pytest.raises(ValueError, match="dtype"):
        indoor.prepare_frames([colour.astype(np.float32)], [])
    with pytest.raises(ValueError, match="no frames"):
        indoor.prepare_frames([], [])
