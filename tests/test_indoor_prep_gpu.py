"""GPU: the 3DMatch pair preparation (pcrcg_amd/indoor.py) -- prepare_frames (pcrcg_prepare_frames) against PIL's output
(tests/golden/indoor_frames.npz) and the numpy restatement, augment against the float64 restatement, and prepare_pairs on
two mini pairs with synthetic frames: every key, the correspondences, the projections, and one dict through
collate_fn_descriptor and a KPFCNN forward against a batch assembled by hand from the existing pieces."""
import functools

import numpy as np
import pytest
import torch

from pcrcg_amd import _lib, indoor, indoor_config, synthetic
from pcrcg_amd.correspondences import get_correspondences
from pcrcg_amd.projection import Projection, superglue_valid_maps

from . import indoor_ref as IR

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gold(golden_dir):
    return IR.load_golden(golden_dir)


def _bits(t):
    return t.cpu().numpy().tobytes()


def test_prepare_frames_equals_pil(cuda, gold):
    """Bit-equal to ToTensor applied to PIL's resize: colour and the 48x64 depth frames in ONE call, the odd 7x11 -> 3x4
    depth frames in another; 0, 1, 32767, 32768 and 65535 are among the depth values, 0 and 255 among the colours."""
    colour, depth = indoor.prepare_frames(list(gold["color"]), list(gold["depth_big"]), image_size=(24, 32), depth_size=(12, 16))
    assert colour.is_cuda and colour.dtype == torch.float32 and tuple(colour.shape) == (2, 3, 24, 32)
    assert depth.dtype == torch.float32 and tuple(depth.shape) == (2, 12, 16)
    want_c = gold["color_resized"].transpose(0, 3, 1, 2).astype(np.float32) / np.float32(255)
    want_d = gold["depth_big_resized"].view(np.int16).astype(np.float32) / np.float32(1000)
    assert _bits(colour) == np.ascontiguousarray(want_c).tobytes()
    assert _bits(depth) == want_d.tobytes()
    _, odd = indoor.prepare_frames([], list(gold["depth_odd"]), depth_size=(3, 4))
    want = gold["depth_odd_resized"].view(np.int16).astype(np.float32) / np.float32(1000)
    assert _bits(odd) == want.tobytes()
    assert float(odd.min()) < 0 and bool((odd == np.float32(-0.001)).any())      # 65535 -> -0.001: the reference's int16 reading


def test_prepare_frames_one_kind_only_and_input_forms(cuda, gold):
    c, d = indoor.prepare_frames([gold["color"][1]], [], image_size=(24, 32))                       # F = 1, G = 0
    assert tuple(c.shape) == (1, 3, 24, 32) and tuple(d.shape)[0] == 0
    assert _bits(c[0]) == IR.color_to_tensor(gold["color"][1], (24, 32)).tobytes()
    five = [gold["depth_big"][k % 2][::-1] if k > 1 else gold["depth_big"][k] for k in range(5)]    # F = 0, G = 5
    c, d = indoor.prepare_frames([], five, depth_size=(12, 16))
    assert tuple(c.shape)[0] == 0 and tuple(d.shape) == (5, 12, 16)
    for k in range(5):
        assert _bits(d[k]) == IR.depth_to_tensor(np.ascontiguousarray(five[k]), (12, 16)).tobytes(), k
    # tensors on the host and on the device, int16 bits, an odd number of colour bytes in front of the depth block
    odd_c = gold["color"][0][:7, :11]
    c2, d2 = indoor.prepare_frames([torch.from_numpy(np.ascontiguousarray(odd_c)).to(cuda)],
                                   [torch.from_numpy(gold["depth_odd"][0].view(np.int16)), gold["depth_odd"][1]],
                                   image_size=(3, 4), depth_size=(3, 4))
    assert _bits(c2[0]) == IR.color_to_tensor(odd_c, (3, 4)).tobytes()
    assert _bits(d2) == (gold["depth_odd_resized"].view(np.int16).astype(np.float32) / np.float32(1000)).tobytes()


def test_prepare_frames_at_the_reference_sizes(cuda):
    """One 480x640 colour and depth frame through 240x320 / 120x160, and an up-scaling, against the restatement."""
    rng = np.random.RandomState(8)
    col = rng.randint(0, 256, (480, 640, 3)).astype(np.uint8)
    dep = rng.randint(0, 65536, (480, 640)).astype(np.uint16)
    c, d = indoor.prepare_frames([col], [dep])
    assert tuple(c.shape) == (1, 3, 240, 320) and tuple(d.shape) == (1, 120, 160)
    assert _bits(c[0]) == IR.color_to_tensor(col, (240, 320)).tobytes()
    assert _bits(d[0]) == IR.depth_to_tensor(dep, (120, 160)).tobytes()
    c, d = indoor.prepare_frames([col[:30, :50]], [dep[:31, :17]], image_size=(77, 123), depth_size=(40, 19))
    assert _bits(c[0]) == IR.color_to_tensor(col[:30, :50], (77, 123)).tobytes()
    assert _bits(d[0]) == IR.depth_to_tensor(np.ascontiguousarray(dep[:31, :17]), (40, 19)).tobytes()


@functools.lru_cache(maxsize=None)
def _mini(seed):
    """A mini LoMatch pair (about 600 points a side) with each fragment moved in front of its own first camera, which sits
    at the fragment's origin looking along +z as a 3DMatch fragment's does; rot / trans follow the move."""
    src, tgt, rot, trans = synthetic.lomatch_pair("mini", seed, overlap=0.3)
    rot, trans = rot.astype(np.float64), trans.astype(np.float64).reshape(3, 1)

    def off(p):
        lo, hi = p.min(0), p.max(0)
        return np.array([-(lo[0] + hi[0]) / 2, -(lo[1] + hi[1]) / 2, 0.8 - lo[2] + 0.5 * (hi[0] - lo[0])], np.float32)
    o_s, o_t = off(src), off(tgt)
    src, tgt = src + o_s, tgt + o_t
    trans = trans - rot @ o_s.astype(np.float64)[:, None] + o_t.astype(np.float64)[:, None]
    return src, tgt, rot, trans


@pytest.mark.parametrize("seed", [0, 1, 2, 3])          # 0, 3 rotate the source, 1, 2 the target
def test_augment_against_the_float64_restatement(cuda, seed):
    src, tgt, rot, trans = _mini(2)
    cfg = indoor_config(augment_noise=0.005)
    got = indoor.augment(torch.from_numpy(src).to(cuda), tgt, rot, trans, cfg, np.random.RandomState(seed))
    want = IR.augment(src, tgt, rot, trans, 0.005, np.random.RandomState(seed))
    assert got["draws"]["rotate_src"] == want["rotate_src"] == (seed in (0, 3))
    for k in ("src", "tgt"):
        assert got[k].dtype == torch.float64 and got[k].is_cuda
        diff = float(np.abs(got[k].cpu().numpy() - want[k]).max())
        print(f"augment seed {seed} {k}: max |diff| {diff:.3e}")
        assert diff <= 1e-12, (k, diff)
    for k in ("rot", "trans"):
        assert got[k].dtype == np.float64 and float(np.abs(got[k] - want[k]).max()) <= 1e-12, k
    for k in ("src_world2camera1", "tgt_world2camera1"):
        assert got[k].dtype == torch.float32 and not got[k].is_cuda and np.array_equal(got[k].numpy(), want[k]), k


def _raw_frames(src, tgt, seed, img_num):
    """Raw frames in the manner of synthetic.frame_inputs: per side and image a random 48x64 colour frame, a 16-bit depth
    frame z-buffer-rendered from the cloud at 48x64 (millimetres), and the camera pose; SuperGlue-like arrays per image."""
    rng = np.random.RandomState(3000 + seed)
    K_raw = np.array([[58.5, 0.0, 32.0], [0.0, 58.5, 24.0], [0.0, 0.0, 1.0]])
    out = {"intrinsics": K_raw}
    for side, pts in (("src", src), ("tgt", tgt)):
        triples = []
        for i in range(img_num):
            pose = np.eye(4) if i == 0 else synthetic._pose(rng)
            w2c = np.linalg.inv(pose)                         # pose_i^-1 . pose_1 with pose_1 = identity
            depth = synthetic.render_depth(pts, w2c.astype(np.float32), intrinsics=K_raw.astype(np.float32), h=48, w=64, rng=rng)
            triples.append((rng.randint(0, 256, (48, 64, 3)).astype(np.uint8), np.round(depth * 1000).astype(np.uint16), pose))
        out[side] = triples
    sg = [dict(synthetic.superglue_like(rng)) for _ in range(img_num)]
    for m in sg:
        m["match_confidence"] = m.pop("confidence")
    return out, sg


@pytest.fixture(scope="module")
def prepared(cuda):
    """B = 2 mini pairs, two frames per side, augmentation on: the raw-frame dicts and the projected ones, prepared once."""
    cfg = indoor_config(first_feats_dim=32, gnn_feats_dim=64, image_feature=True, img_num=2, in_feats_dim=129,
                        augment_noise=0.005, window_size=5)
    data = [_mini(s) for s in (1, 4)]
    fm = [_raw_frames(src, tgt, s, 2) for s, (src, tgt, _, _) in enumerate(data)]
    args = ([d[0] for d in data], [d[1] for d in data], [d[2] for d in data], [d[3] for d in data], cfg)
    kw = dict(frames=[f for f, _ in fm], matches=[m for _, m in fm])
    raw = indoor.prepare_pairs(*args, augment=np.random.RandomState(7), **kw)
    proj = indoor.prepare_pairs(*args, augment=np.random.RandomState(7), projections=True, **kw)
    return cfg, data, fm, raw, proj


def test_prepare_pairs_keys_and_values(cuda, prepared):
    cfg, data, fm, raw, proj = prepared
    base = {"src_pcd", "tgt_pcd", "src_feats", "tgt_feats", "rot", "trans", "correspondences", "sample"}
    per_image = lambda names: {f"{side}{i}_{n}" for side in ("src", "tgt") for i in (1, 2) for n in names}
    common = base | {f"{side}_color{i}" for side in ("src", "tgt") for i in (1, 2)} | \
        {f"{side}_valid_map{i}" for side in ("src", "tgt") for i in (1, 2)}
    rng = np.random.RandomState(7)
    assert len(raw) == len(proj) == 2
    for b in range(2):
        assert set(raw[b]) == common | per_image(("depth", "world2camera", "intrinsics"))
        assert set(proj[b]) == common | per_image(("inds2d", "inds3d"))
        src, tgt, rot, trans = data[b]
        want = IR.augment(src, tgt, rot, trans, 0.005, rng)               # the pairs consume ONE generator in order
        item = raw[b]
        for k in ("src", "tgt"):
            assert item[f"{k}_pcd"].dtype == torch.float32 and item[f"{k}_pcd"].is_cuda
            assert float(np.abs(item[f"{k}_pcd"].cpu().numpy() - want[k]).max()) <= 1e-6
            n = item[f"{k}_pcd"].shape[0]
            assert tuple(item[f"{k}_feats"].shape) == (n, 1) and bool((item[f"{k}_feats"] == 1).all())
        assert item["rot"].dtype == np.float32 and item["rot"].shape == (3, 3) and item["trans"].shape == (3, 1)
        assert np.array_equal(item["rot"], want["rot"].astype(np.float32)) and np.array_equal(item["trans"], want["trans"].astype(np.float32))
        assert torch.equal(item["sample"], torch.ones(1))
        # correspondences: the per-pair call on the clouds the dict holds, under the relabelled float64 transform
        T = np.eye(4)
        T[:3, :3], T[:3, 3] = want["rot"], want["trans"][:, 0]
        by_hand = get_correspondences(item["src_pcd"], item["tgt_pcd"], T, cfg.overlap_radius)
        assert by_hand.shape[0] > 500 and torch.equal(item["correspondences"], by_hand)
        assert torch.equal(proj[b]["correspondences"], by_hand) and torch.equal(proj[b]["src_pcd"], item["src_pcd"])
        # frames: colour / depth from the restatement, matrices from the restated chain, intrinsics at 160 x 120
        K = np.eye(4)
        K[:3, :3] = IR.adjust_intrinsic(fm[b][0]["intrinsics"], [64, 48], [160, 120])
        for side in ("src", "tgt"):
            chain = IR.pose_chain([t[2] for t in fm[b][0][side]], want[f"{side}_world2camera1"])
            for i in (1, 2):
                colour, depth, _ = fm[b][0][side][i - 1]
                assert _bits(item[f"{side}_color{i}"]) == IR.color_to_tensor(colour, (240, 320)).tobytes()
                assert _bits(item[f"{side}{i}_depth"]) == IR.depth_to_tensor(depth, (120, 160)).tobytes()
                w = item[f"{side}{i}_world2camera"]
                assert w.dtype == torch.float32 and not w.is_cuda and float(np.abs(w.numpy() - chain[i - 1]).max()) <= 4e-6
                assert np.array_equal(item[f"{side}{i}_intrinsics"].numpy(), K.astype(np.float32))
                # projections=True: Projection.projection on the same prepared depth and matrices
                i2, i3 = Projection(item[f"{side}{i}_intrinsics"]).projection(item[f"{side}_pcd"], item[f"{side}{i}_depth"], w)
                assert torch.equal(proj[b][f"{side}{i}_inds2d"], i2) and torch.equal(proj[b][f"{side}{i}_inds3d"], i3)
                assert torch.equal(proj[b][f"{side}_color{i}"], item[f"{side}_color{i}"])
        assert sum(int(proj[b][f"{side}{i}_inds3d"].shape[0]) for side in ("src", "tgt") for i in (1, 2)) > 200
        for i in (1, 2):
            m = fm[b][1][i - 1]
            s, t = superglue_valid_maps(*(torch.from_numpy(m[k]).to(cuda) for k in ("keypoints0", "keypoints1", "matches",
                                                                                     "match_confidence")), window=5)
            assert torch.equal(item[f"src_valid_map{i}"], s) and torch.equal(item[f"tgt_valid_map{i}"], t)


def test_prepare_pair_without_frames_or_augmentation(cuda):
    src, tgt, rot, trans = _mini(1)
    cfg = indoor_config()
    item = indoor.prepare_pair(src, torch.from_numpy(tgt).to(cuda), rot, trans, cfg)
    assert set(item) == {"src_pcd", "tgt_pcd", "src_feats", "tgt_feats", "rot", "trans", "correspondences", "sample"}
    assert _bits(item["src_pcd"]) == src.tobytes() and _bits(item["tgt_pcd"]) == tgt.tobytes()
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = rot, trans.reshape(3)
    assert torch.equal(item["correspondences"], get_correspondences(item["src_pcd"], item["tgt_pcd"], T, cfg.overlap_radius))
    assert np.array_equal(item["rot"], rot.astype(np.float32)) and item["trans"].shape == (3, 1)


def test_prepared_dict_through_the_network(cuda, prepared):
    """One prepared dict -> collate_fn_descriptor -> KPFCNN(image_feature=True, img_num=2), against the same forward of a
    batch assembled by hand from the existing pieces (get_correspondences, Projection's inputs as raw-frame keys,
    superglue_valid_maps): bit-equal outputs.  Both forwards run under deterministic=1 (include/pcrcg.h): by default the
    path adds with floating-point atomics and two forwards of ONE batch differ in the last bits
    (tests/test_deterministic_gpu.py), so only under the switch is the output a function of the batch alone.  The 129-column
    input build, which has no such sums, is compared bit for bit in the default mode."""
    from pcrcg_amd.architectures import KPFCNN
    from pcrcg_amd.pyramid import collate_fn_descriptor
    cfg, data, fm, raw, _ = prepared
    limits = [24, 37, 45, 48]
    item = dict(raw[1])
    g = torch.Generator().manual_seed(12)
    fmaps = {f"{side}{i}_feature2d": torch.rand(128, 120, 160, generator=g).to(cuda) for side in ("src", "tgt") for i in (1, 2)}
    item.update(fmaps)
    # by hand, from the restatement and the existing entry points
    src, tgt, rot, trans = data[1]
    rng = np.random.RandomState(7)
    IR.augment(*data[0], 0.005, rng)                                      # (pair 0's draws come first)
    a = IR.augment(src, tgt, rot, trans, 0.005, rng)
    hand = {"src_pcd": torch.from_numpy(a["src"]).to(cuda).float(), "tgt_pcd": torch.from_numpy(a["tgt"]).to(cuda).float(),
            "rot": a["rot"].astype(np.float32), "trans": a["trans"].astype(np.float32), "sample": torch.ones(1)}
    assert torch.equal(hand["src_pcd"], item["src_pcd"]) and torch.equal(hand["tgt_pcd"], item["tgt_pcd"])
    for k in ("src", "tgt"):
        hand[f"{k}_feats"] = torch.ones((hand[f"{k}_pcd"].shape[0], 1), device=cuda)
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = a["rot"], a["trans"][:, 0]
    hand["correspondences"] = get_correspondences(hand["src_pcd"], hand["tgt_pcd"], T, cfg.overlap_radius)
    K = np.eye(4)
    K[:3, :3] = IR.adjust_intrinsic(fm[1][0]["intrinsics"], [64, 48], [160, 120])
    for side in ("src", "tgt"):
        chain = indoor.world2camera_chain([t[2] for t in fm[1][0][side]], torch.from_numpy(a[f"{side}_world2camera1"]))
        for i in (1, 2):
            hand[f"{side}{i}_depth"] = torch.from_numpy(IR.depth_to_tensor(fm[1][0][side][i - 1][1], (120, 160))).to(cuda)
            hand[f"{side}{i}_world2camera"] = chain[i - 1]
            hand[f"{side}{i}_intrinsics"] = torch.from_numpy(K).float()
    for i in (1, 2):
        m = fm[1][1][i - 1]
        hand[f"src_valid_map{i}"], hand[f"tgt_valid_map{i}"] = superglue_valid_maps(
            *(torch.from_numpy(m[k]).to(cuda) for k in ("keypoints0", "keypoints1", "matches", "match_confidence")), window=5)
    hand.update(fmaps)
    torch.manual_seed(3)
    np.random.seed(3)
    net = KPFCNN(cfg).to(cuda).eval()
    outs = []
    L = _lib.lib()
    try:
        _lib.check(L.pcrcg_debug_set(b"deterministic=1"), "pcrcg_debug_set")
        for d in (item, hand):
            batch = collate_fn_descriptor([d], cfg, limits, device=cuda)
            with torch.no_grad():
                outs.append({k: v.clone() for k, v in net(batch).items()})
        torch.cuda.synchronize()
    finally:
        _lib.check(L.pcrcg_debug_set(None), "pcrcg_debug_set")
    n = item["src_pcd"].shape[0] + item["tgt_pcd"].shape[0]
    for k in ("feats_f", "scores_overlap", "scores_saliency"):
        assert outs[0][k].shape[0] == n and bool(torch.isfinite(outs[0][k]).all())
        assert torch.equal(outs[0][k], outs[1][k]), k
    x = net.image_features(collate_fn_descriptor([item], cfg, limits, device=cuda))
    assert torch.equal(x, net.image_features(collate_fn_descriptor([hand], cfg, limits, device=cuda)))
    assert int((x[:, :128] != 1).any(1).sum()) > n // 20                 # the frames do reach the points
