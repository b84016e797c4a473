"""Preparing 3DMatch pairs on the device: the body of ref:datasets/indoor.py IndoorDataset.__getitem__ (:123-831) after the
files are read -- two fragments, their rot / trans, and for the image branch 1-3 decoded colour / depth frames per side with
their poses, the scene's intrinsics and SuperGlue's arrays -- batched over pairs.

  * `adjust_intrinsic`    -- ref:datasets/visualize.py:244-275, float64 numpy on the host.
  * `world2camera_chain`  -- :587-594, 777-790: pose_i^-1 . pose_1 . world2camera_1 for frames 2 and 3, float32 torch.mm on
                             the host in the reference's association order.
  * `prepare_frames`      -- :63-78, 465-486: Resize(NEAREST) + ToTensor of every colour and depth frame, and the depth's
                             `/ 1000.0`, in ONE upload and ONE library call (pcrcg_prepare_frames; include/pcrcg.h "Decoded
                             RGB-D frames").
  * `augment_draws`, `augment` -- :142-168: the draws on the host in the reference's order and shapes, applied on the device.
  * `prepare_pairs`       -- :123-190 and the image branch for B pairs: augmentation, ONE get_correspondences_batch call, ONE
                             prepare_frames call for every frame of every pair, and one dict per pair with the reference's
                             keys; `prepare_pair` is one pair.

Depth values: ToTensor reads a 16-bit PNG (PIL mode I;16) through np.int16, so a raw 65535 ("no reading") becomes -0.001 m
and every raw value of 32768 or more comes out negative.  That is the reference's behaviour and it is kept.
"""
import numpy as np
import torch

from . import _lib
from .config import as_config
from .correspondences import get_correspondences_batch
from .kitti import _device, _rotate, _rows, euler_zyx_matrix

MAX_POINTS = 30000          # ref:datasets/indoor.py:62
ROT_FACTOR = 1.0            # :60
AUGMENT_NOISE = 0.005       # ref:configs/train/indoor.yaml, where the config does not carry augment_noise
_MAX_FRAMES = 65535         # pcrcg_prepare_frames: F + G
_MAX_SIDE = 1 << 15         # ... and every image side


def adjust_intrinsic(intrinsic, intrinsic_image_dim, image_dim):
    """ref:datasets/visualize.py:244-275: the intrinsics of a (width, height) = intrinsic_image_dim image for the same
    image resized to image_dim.  float64 numpy; equal sizes return the input itself, as the reference does."""
    if list(intrinsic_image_dim) == list(image_dim):
        return intrinsic
    out = np.array(intrinsic, dtype=np.float64, copy=True)
    height_after, height_before = image_dim[1], intrinsic_image_dim[1]
    width_after, width_before = image_dim[0], intrinsic_image_dim[0]
    height_ratio = height_after / height_before
    width_ratio = width_after / width_before
    if width_ratio >= height_ratio:
        resize_height = height_after
        resize_width = height_ratio * width_before
    else:
        resize_width = width_after
        resize_height = width_ratio * height_before
    out[0, 0] *= float(resize_width) / float(width_before)
    out[1, 1] *= float(resize_height) / float(height_before)
    out[0, 2] *= float(resize_width - 1) / float(width_before - 1)       # (the reference's account of cropping/padding)
    out[1, 2] *= float(resize_height - 1) / float(height_before - 1)
    return out


def _pose44(p, what):
    p = np.asarray(p.cpu() if isinstance(p, torch.Tensor) else p, dtype=np.float64)
    if p.shape != (4, 4):
        raise ValueError(f"{what} must be a [4, 4] matrix, got shape {p.shape}")
    return p


def world2camera_chain(poses, world2camera1):
    """ref:datasets/indoor.py:587-594 (img_num 2) and :777-790 (img_num 3): the world2camera of every frame of one side.
    poses: the side's 1-3 camera poses ([4,4], the .pose.txt matrices); world2camera1: frame 1's [4,4] (the identity, or the
    inverse of the augmentation's rotation).  -> list of float32 host tensors: [world2camera1, pose_2^-1 . (pose_1 .
    world2camera1), pose_3^-1 . (pose_1 . world2camera1)].  The inverse is float64 numpy, the products float32 torch.mm."""
    if not 1 <= len(poses) <= 3:
        raise ValueError(f"world2camera_chain: a side has 1 to 3 frames, got {len(poses)}")
    w1 = torch.as_tensor(world2camera1).detach().to("cpu", torch.float32)
    if tuple(w1.shape) != (4, 4):
        raise ValueError(f"world2camera_chain: world2camera1 must be [4, 4], got {tuple(w1.shape)}")
    ps = [_pose44(p, "world2camera_chain: a pose") for p in poses]
    out = [w1]
    for p in ps[1:]:
        rev = np.linalg.inv(p)
        out.append(torch.mm(torch.from_numpy(rev).float(), torch.mm(torch.from_numpy(ps[0]).float(), w1)))
    return out


def _stack_frames(frames, rank, who):
    """Checks that a list of decoded frames (numpy, CPU or HIP tensors) has one shape of the given rank -> (frames, shape)."""
    first = None
    arrs = []
    for k, f in enumerate(frames):
        shape = tuple(f.shape) if hasattr(f, "shape") else np.shape(f)
        if len(shape) != rank or (rank == 3 and shape[2] != 3):
            raise ValueError(f"prepare_frames: {who} frame {k} must be {'[H, W, 3]' if rank == 3 else '[H, W]'}, got shape {shape}")
        if first is None:
            first = shape
        elif shape != first:
            raise ValueError(f"prepare_frames: the {who} frames of one call share one size ({first} and {shape})")
        if min(shape[:2]) < 1 or max(shape[:2]) > _MAX_SIDE:
            raise ValueError(f"prepare_frames: {who} frame {k} has a side outside 1..{_MAX_SIDE}")
        arrs.append(f)
    return arrs, first


def _as_bytes(f, dtypes, who):
    """One frame -> a tensor of its bytes: a uint8 view of a HIP tensor, or of a host array."""
    if isinstance(f, torch.Tensor):
        if str(f.dtype).split(".")[1] not in dtypes:
            raise ValueError(f"prepare_frames: a {who} frame must have dtype {' or '.join(dtypes)}, got {f.dtype}")
        if f.is_cuda:
            return f.contiguous().view(torch.uint8).reshape(-1)
        f = f.contiguous().view(torch.uint8).numpy()
    else:
        f = np.asarray(f)
        if f.dtype.name not in dtypes:
            raise ValueError(f"prepare_frames: a {who} frame must have dtype {' or '.join(dtypes)}, got {f.dtype}")
    return torch.from_numpy(np.ascontiguousarray(f).view(np.uint8).reshape(-1))


def prepare_frames(colors, depths, image_size=(240, 320), depth_size=(120, 160)):
    """The reference's frame transforms (ref:datasets/indoor.py:63-78) for F colour and G depth frames ->
    (colour [F, 3, image_size] float32, depth [G, depth_size] float32) on the device; either list may be empty.

    colors: decoded colour frames, uint8 [H, W, 3] (numpy, CPU or HIP tensors), all of one size; depths: decoded 16-bit depth
    frames, uint16 or int16 [Hd, Wd] (the same bits), all of one size.  Sizes are (height, width).  Resize is PIL's
    Image.NEAREST rule -- output index i reads input index floor((i + 0.5) * n_in / n_out) -- and the values are ToTensor's:
    colour / 255, depth float(int16(v)) / 1000 (so 65535 becomes -0.001: the module docstring).  Host frames travel in ONE
    upload; everything is converted by ONE pcrcg_prepare_frames call."""
    colors, depths = list(colors), list(depths)
    F, G = len(colors), len(depths)
    if F + G == 0:
        raise ValueError("prepare_frames: no frames")
    if F + G > _MAX_FRAMES:
        raise ValueError(f"prepare_frames: {F + G} frames in one call, at most {_MAX_FRAMES}")
    oh, ow = (int(v) for v in image_size)
    ohd, owd = (int(v) for v in depth_size)
    if min(oh, ow, ohd, owd) < 1 or max(oh, ow, ohd, owd) > _MAX_SIDE:
        raise ValueError(f"prepare_frames: output sides must lie in 1..{_MAX_SIDE}")
    colors, cshape = _stack_frames(colors, 3, "colour")
    depths, dshape = _stack_frames(depths, 2, "depth")
    parts = [_as_bytes(f, ("uint8",), "colour") for f in colors] + [_as_bytes(f, ("uint16", "int16"), "depth") for f in depths]
    dev = _device(colors + depths)
    if all(not p.is_cuda for p in parts):
        buf = torch.cat(parts).to(dev)                                   # the ONE upload
    else:
        buf = torch.cat([p.to(dev) for p in parts])
    # (a colour frame holds 3 H W bytes: the depth block starts at an even byte only if F H W is even -- pad by copy if not)
    cbytes = F * cshape[0] * cshape[1] * 3 if F else 0
    cbuf = buf[:cbytes]
    dbuf = buf[cbytes:]
    if G and dbuf.data_ptr() % 2:
        dbuf = dbuf.clone()
    L = _lib.lib()
    color_out = torch.empty((F, 3, oh, ow), dtype=torch.float32, device=dev)
    depth_out = torch.empty((G, ohd, owd), dtype=torch.float32, device=dev)
    H, W = cshape[:2] if F else (0, 0)
    Hd, Wd = dshape if G else (0, 0)
    _lib.check(L.pcrcg_prepare_frames(cbuf.data_ptr() if F else None, F, H, W, oh, ow, color_out.data_ptr() if F else None,
                                      dbuf.data_ptr() if G else None, G, Hd, Wd, ohd, owd,
                                      depth_out.data_ptr() if G else None, torch.cuda.current_stream(dev).cuda_stream),
               "pcrcg_prepare_frames")
    return color_out, depth_out


def augment_draws(n_src, n_tgt, config, np_rng):
    """The random numbers of ref:datasets/indoor.py:142-168, drawn on the host from `np_rng` (a numpy.random.RandomState;
    the reference draws from numpy's global state) in the reference's call order and shapes: the permutation of a cloud of
    more than MAX_POINTS = 30000 points (source first), rand(3) Euler angles, rand(1) for the side, rand(n_src, 3) and
    rand(n_tgt, 3) for the noise (n = the size after the cut).  -> dict of float64 numpy values; perm_src / perm_tgt are
    None where no cut happens."""
    d = {}
    d["perm_src"] = np_rng.permutation(n_src)[:MAX_POINTS] if n_src > MAX_POINTS else None        # :142-144
    d["perm_tgt"] = np_rng.permutation(n_tgt)[:MAX_POINTS] if n_tgt > MAX_POINTS else None        # :145-147
    n_src, n_tgt = min(n_src, MAX_POINTS), min(n_tgt, MAX_POINTS)
    d["euler"] = np_rng.rand(3) * np.pi * 2 / ROT_FACTOR                                            # :154
    d["rot"] = euler_zyx_matrix(d["euler"])                                                         # :155
    d["rotate_src"] = bool(np_rng.rand(1)[0] > 0.5)                                                 # :156-157
    noise = as_config(config).get("augment_noise", AUGMENT_NOISE)
    d["noise_src"] = (np_rng.rand(n_src, 3) - 0.5) * noise                                          # :167
    d["noise_tgt"] = (np_rng.rand(n_tgt, 3) - 0.5) * noise                                          # :168
    return d


def relabel(rot, trans, draws):
    """The host side of the augmentation: the pair's rot [3,3] / trans [3,1] after `draws`' rotation (:157-165) and frame 1's
    world2camera of both sides (:569-586) -> (rot, trans: float64 numpy; src_world2camera1, tgt_world2camera1: float32 host
    [4,4]).  Source rotated: rot @ rot_ab.T, trans unchanged; target rotated: rot_ab @ rot, rot_ab @ trans.  The rotated
    side's world2camera is rot_ab^-1 (numpy's inverse, as the reference takes it) in the identity, the other the identity."""
    rot = np.asarray(rot, dtype=np.float64).reshape(3, 3)
    trans = np.asarray(trans, dtype=np.float64).reshape(3, 1)
    w2c = np.eye(4)
    w2c[:3, :3] = np.linalg.inv(draws["rot"])                             # :573-574, 580-581
    w2c = torch.from_numpy(w2c).float()
    if draws["rotate_src"]:
        return np.matmul(rot, draws["rot"].T), trans, w2c, torch.eye(4)   # :159
    return np.matmul(draws["rot"], rot), np.matmul(draws["rot"], trans), torch.eye(4), w2c       # :164-165


def augment(src, tgt, rot, trans, config, np_rng):
    """ref:datasets/indoor.py:142-168 and :569-586 -> dict: `src`, `tgt` (float64 device tensors: the cut, ONE rotation
    applied to the source or to the target, THEN the noise -- the other order than KITTI's), `rot` [3,3] and `trans` [3,1]
    relabelled (float64 numpy: rot @ rot_ab.T when the source was rotated; rot_ab @ rot and rot_ab @ trans when the target
    was), `src_world2camera1`, `tgt_world2camera1` (float32 host [4,4]: rot_ab^-1 of the rotated side, the identity of the
    other) and `draws` (augment_draws' dict).  The draws happen on the host; the points are moved in float64 torch on the
    device, each rotated row's three products added left to right.  config: augment_noise (0.005, the shipped value, when
    absent)."""
    config = as_config(config)
    dev = _device([src, tgt])
    s = (src if isinstance(src, torch.Tensor) else torch.as_tensor(np.asarray(src))).to(device=dev, dtype=torch.float64)
    t = (tgt if isinstance(tgt, torch.Tensor) else torch.as_tensor(np.asarray(tgt))).to(device=dev, dtype=torch.float64)
    _rows(s, "augment", 0), _rows(t, "augment", 1)
    d = augment_draws(s.shape[0], t.shape[0], config, np_rng)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    if d["perm_src"] is not None:
        s = s[up(d["perm_src"])]
    if d["perm_tgt"] is not None:
        t = t[up(d["perm_tgt"])]
    if d["rotate_src"]:
        s = _rotate(s, up(d["rot"]))
    else:
        t = _rotate(t, up(d["rot"]))
    rot, trans, w2c_src, w2c_tgt = relabel(rot, trans, d)
    s = s + up(d["noise_src"])
    t = t + up(d["noise_tgt"])
    return {"src": s, "tgt": t, "rot": rot, "trans": trans, "src_world2camera1": w2c_src, "tgt_world2camera1": w2c_tgt,
            "draws": d}


_augment = augment      # (prepare_pairs has a keyword of that name)


def _check_frames(frames, matches, B):
    """-> img_num after checking the layout of prepare_pairs' `frames` and `matches`."""
    if len(frames) != B:
        raise ValueError(f"prepare_pairs: frames has {len(frames)} entries for {B} pairs")
    img_num = None
    for b, fr in enumerate(frames):
        for side in ("src", "tgt"):
            n = len(fr[side])
            if not 1 <= n <= 3:
                raise ValueError(f"prepare_pairs: pair {b}: img_num must be 1, 2 or 3, the {side} side has {n} frames")
            if img_num is None:
                img_num = n
            elif n != img_num:
                raise ValueError(f"prepare_pairs: pair {b}: the {side} side has {n} frames, others have {img_num}")
            for triple in fr[side]:
                if len(triple) != 3:
                    raise ValueError(f"prepare_pairs: pair {b}: a frame is a (colour, depth, pose) triple")
        if "intrinsics" not in fr:
            raise ValueError(f"prepare_pairs: pair {b}: frames carry the scene's intrinsics under 'intrinsics'")
    if img_num < 3:
        if matches is None:
            raise ValueError("prepare_pairs: img_num < 3 needs SuperGlue's arrays (matches=) for the valid maps")
        if len(matches) != B:
            raise ValueError(f"prepare_pairs: matches has {len(matches)} entries for {B} pairs")
        for b, m in enumerate(matches):
            if len(m) != img_num:
                raise ValueError(f"prepare_pairs: pair {b}: {len(m)} match records for {img_num} images")
    return img_num


def prepare_pairs(fragments_src, fragments_tgt, rots, transs, config, *, frames=None, matches=None, augment=None,
                  projections=False):
    """ref:datasets/indoor.py:123-831 for B pairs -> a list of B dicts with the reference's keys, what
    pyramid.collate_fn_descriptor takes.

    fragments_src[b], fragments_tgt[b]: the two fragments' [N,3] points (numpy, CPU or HIP tensors; the reference's .pth
    clouds); rots[b] [3,3], transs[b] [3] or [3,1]: the pair's ground truth.  augment: None, or a numpy.random.RandomState:
    every pair then goes through `augment` in order (the cut to 30000 points included; without it a larger cloud is taken
    whole -- the reference cuts it with a draw from numpy's global state even then, which is the caller's to do).

    Every dict holds src_pcd, tgt_pcd (fp32 device tensors), src_feats, tgt_feats (ones, [N,1] fp32), rot [3,3] and trans
    [3,1] (fp32 numpy, relabelled by the augmentation), correspondences ([K,2] int64 device: ONE get_correspondences_batch
    call for all pairs at config.overlap_radius under the relabelled transforms) and sample = torch.ones(1).

    frames: None, or per pair a dict {"src": [(colour, depth, pose), ...], "tgt": [...], "intrinsics": K}: 1-3 triples per
    side (the same number everywhere: img_num) of a decoded colour frame (uint8 [H,W,3]), a decoded depth frame (uint16
    [Hd,Wd]) and the frame's [4,4] camera pose, and the scene's [3,3] or [4,4] intrinsics at the depth frames' raw size.
    All frames of all pairs go through ONE prepare_frames call (240 x 320 colour, 120 x 160 depth).  The dicts then also
    carry {side}_color{i} [3,240,320], the raw-frame keys KPFCNN's fused input build reads -- {side}{i}_depth [120,160]
    (device), {side}{i}_world2camera and {side}{i}_intrinsics ([4,4] fp32 host tensors: world2camera_chain from the
    augmentation's frame-1 matrix, adjust_intrinsic to the depth size embedded in the identity) -- and for img_num < 3
    src_valid_map{i}, tgt_valid_map{i} painted by projection.superglue_valid_maps from matches[b][i-1], a dict with
    SuperGlue's keypoints0, keypoints1, matches and match_confidence (window = config.window_size, 5 when absent).
    projections=True: {side}{i}_inds2d / _inds3d from projection.Projection replace the three raw-frame keys, as the
    reference's loader emits them.

    The reference searches the correspondences among its float64 clouds; this searches what the network is fed, the same
    clouds rounded to fp32 (as kitti.prepare_pairs does), so a pair within fp32 rounding of the radius may differ."""
    config = as_config(config)
    B = len(fragments_src)
    if B == 0:
        raise ValueError("prepare_pairs: no pairs")
    if len(fragments_tgt) != B or len(rots) != B or len(transs) != B:
        raise ValueError(f"prepare_pairs: list lengths differ ({B}, {len(fragments_tgt)}, {len(rots)}, {len(transs)})")
    for b in range(B):
        _rows(fragments_src[b], "prepare_pairs: fragments_src", b)
        _rows(fragments_tgt[b], "prepare_pairs: fragments_tgt", b)
    img_num = _check_frames(frames, matches, B) if frames is not None else 0
    dev = _device(list(fragments_src) + list(fragments_tgt))
    f64 = lambda x: (x if isinstance(x, torch.Tensor) else torch.as_tensor(np.asarray(x))).to(device=dev, dtype=torch.float64)

    pairs = []
    for b in range(B):
        rot = np.asarray(rots[b].cpu() if isinstance(rots[b], torch.Tensor) else rots[b], dtype=np.float64)
        trans = np.asarray(transs[b].cpu() if isinstance(transs[b], torch.Tensor) else transs[b], dtype=np.float64)
        if rot.shape != (3, 3) or trans.size != 3:
            raise ValueError(f"prepare_pairs: pair {b}: rot must be [3, 3] and trans [3] or [3, 1], got {rot.shape}, {trans.shape}")
        if augment is not None:
            a = _augment(fragments_src[b], fragments_tgt[b], rot, trans, config, augment)
        else:
            a = {"src": f64(fragments_src[b]), "tgt": f64(fragments_tgt[b]), "rot": rot, "trans": trans.reshape(3, 1),
                 "src_world2camera1": torch.eye(4), "tgt_world2camera1": torch.eye(4)}
        a["src"], a["tgt"] = a["src"].float(), a["tgt"].float()
        a["tsfm"] = np.eye(4)
        a["tsfm"][:3, :3], a["tsfm"][:3, 3] = a["rot"], a["trans"][:, 0]                          # to_tsfm, :176
        pairs.append(a)
    corrs = get_correspondences_batch([a["src"] for a in pairs], [a["tgt"] for a in pairs], [a["tsfm"] for a in pairs],
                                      config.overlap_radius)

    if frames is not None:
        sides = [(b, side) for b in range(B) for side in ("src", "tgt")]
        colour, depth = prepare_frames([t[0] for b, side in sides for t in frames[b][side]],
                                       [t[1] for b, side in sides for t in frames[b][side]])
    items = []
    for b, a in enumerate(pairs):
        item = {"src_pcd": a["src"], "tgt_pcd": a["tgt"],
                "src_feats": torch.ones((a["src"].shape[0], 1), dtype=torch.float32, device=dev),
                "tgt_feats": torch.ones((a["tgt"].shape[0], 1), dtype=torch.float32, device=dev),
                "rot": a["rot"].astype(np.float32), "trans": a["trans"].astype(np.float32),
                "correspondences": corrs[b], "sample": torch.ones(1)}
        if frames is not None:
            from .projection import Projection, superglue_valid_maps
            raw = frames[b]["src"][0][1]
            raw_h, raw_w = (tuple(raw.shape) if hasattr(raw, "shape") else np.shape(raw))[:2]
            K = np.asarray(frames[b]["intrinsics"].cpu() if isinstance(frames[b]["intrinsics"], torch.Tensor)
                           else frames[b]["intrinsics"], dtype=np.float64)
            K = adjust_intrinsic(K, [raw_w, raw_h], [depth.shape[2], depth.shape[1]])             # :548-551
            if K.shape[0] == 3:                                                                   # :553-556
                K4 = np.eye(4)
                K4[:3, :3] = K
                K = K4
            K = torch.from_numpy(np.ascontiguousarray(K)).float()                                 # :604
            for s_i, side in enumerate(("src", "tgt")):
                chain = world2camera_chain([t[2] for t in frames[b][side]], a[f"{side}_world2camera1"])
                for i in range(1, img_num + 1):
                    k = (2 * b + s_i) * img_num + i - 1
                    item[f"{side}_color{i}"] = colour[k]
                    if projections:
                        item[f"{side}{i}_inds2d"], item[f"{side}{i}_inds3d"] = Projection(K).projection(
                            a[side], depth[k], chain[i - 1])
                    else:
                        item[f"{side}{i}_depth"] = depth[k]
                        item[f"{side}{i}_world2camera"] = chain[i - 1]
                        item[f"{side}{i}_intrinsics"] = K
            if img_num < 3:
                for i in range(1, img_num + 1):
                    m = matches[b][i - 1]
                    on = lambda x: (x if isinstance(x, torch.Tensor) else torch.from_numpy(np.asarray(x))).to(dev)
                    item[f"src_valid_map{i}"], item[f"tgt_valid_map{i}"] = superglue_valid_maps(
                        on(m["keypoints0"]), on(m["keypoints1"]), on(m["matches"]), on(m["match_confidence"]),
                        window=int(config.get("window_size", 5)))
        items.append(item)
    return items


def prepare_pair(fragment_src, fragment_tgt, rot, trans, config, *, frames=None, matches=None, augment=None,
                 projections=False):
    """One pair -> its dict: prepare_pairs with a batch of one."""
    return prepare_pairs([fragment_src], [fragment_tgt], [rot], [trans], config, frames=None if frames is None else [frames],
                         matches=None if matches is None else [matches], augment=augment, projections=projections)[0]
