"""Numpy restatements of the 3DMatch pair preparation (pcrcg_amd/indoor.py) and the inputs its tests
share.  The reference's own modules (ref:datasets/indoor.py, ref:datasets/visualize.py) import open3d, cv2 and torchvision,
so what they do is restated here, line for line where the arithmetic matters:

    resize + ToTensor : PIL's Image.NEAREST -- out[i] = in[min(floor((i + 0.5) * n_in / n_out), n_in - 1)], float64 --
                        then float32(v) / float32(255) for uint8 colour (HWC -> CHW) and float32(int16(v)) / float32(1000)
                        for 16-bit depth (ToTensor reads mode I;16 through np.int16: 65535 -> -0.001);
    adjust_intrinsic  : ref:datasets/visualize.py:244-275;
    pose chain        : ref:datasets/indoor.py:587-594, 777-790 (float64 inverse, float32 products, pose_i^-1 (pose_1 w2c_1));
    augmentation      : ref:datasets/indoor.py:142-168, 569-586 (cut, rotation of one side, relabelling, THEN noise)."""
import os

import numpy as np

GOLDEN = "indoor_frames.npz"
MAX_POINTS = 30000


def nearest_index(n_in, n_out):
    i = np.arange(n_out, dtype=np.float64)
    return np.minimum(np.floor((i + 0.5) * np.float64(n_in) / np.float64(n_out)).astype(np.int64), n_in - 1)


def resize_nearest(img, size):
    """img [H, W] or [H, W, C], size = (height, width) -> PIL's Image.NEAREST resize, restated."""
    return img[nearest_index(img.shape[0], size[0])][:, nearest_index(img.shape[1], size[1])]


def color_to_tensor(img, size):
    """uint8 [H, W, 3] -> float32 [3, size]: Resize(size, NEAREST) + ToTensor."""
    r = resize_nearest(np.asarray(img, np.uint8), size)
    return np.ascontiguousarray(r.transpose(2, 0, 1)).astype(np.float32) / np.float32(255)


def depth_to_tensor(img, size):
    """uint16 [H, W] -> float32 [size]: Resize(size, NEAREST) + ToTensor (through np.int16) + / 1000.0."""
    r = resize_nearest(np.asarray(img).view(np.uint16) if np.asarray(img).dtype == np.int16 else np.asarray(img, np.uint16), size)
    return r.view(np.int16).astype(np.float32) / np.float32(1000)


def adjust_intrinsic(intrinsic, intrinsic_image_dim, image_dim):
    if intrinsic_image_dim == image_dim:
        return intrinsic
    out = np.copy(intrinsic)
    height_ratio = image_dim[1] / intrinsic_image_dim[1]
    width_ratio = image_dim[0] / intrinsic_image_dim[0]
    if width_ratio >= height_ratio:
        resize_height, resize_width = image_dim[1], height_ratio * intrinsic_image_dim[0]
    else:
        resize_width, resize_height = image_dim[0], width_ratio * intrinsic_image_dim[1]
    out[0, 0] *= float(resize_width) / float(intrinsic_image_dim[0])
    out[1, 1] *= float(resize_height) / float(intrinsic_image_dim[1])
    out[0, 2] *= float(resize_width - 1) / float(intrinsic_image_dim[0] - 1)
    out[1, 2] *= float(resize_height - 1) / float(intrinsic_image_dim[1] - 1)
    return out


def pose_chain(poses, world2camera1):
    """-> list of float32 [4,4]: world2camera1, then pose_i^-1 (pose_1 world2camera1) with float32 products."""
    w1 = np.asarray(world2camera1, np.float32)
    p1 = np.asarray(poses[0], np.float64).astype(np.float32)
    out = [w1]
    for p in poses[1:]:
        rev = np.linalg.inv(np.asarray(p, np.float64)).astype(np.float32)
        out.append(np.matmul(rev, np.matmul(p1, w1)))
    return out


def euler_zyx(angles):
    """scipy's Rotation.from_euler('zyx', angles).as_matrix(): Rx(angles[2]) Ry(angles[1]) Rz(angles[0])."""
    az, ay, ax = (float(a) for a in angles)
    Rz = np.array([[np.cos(az), -np.sin(az), 0.0], [np.sin(az), np.cos(az), 0.0], [0.0, 0.0, 1.0]])
    Ry = np.array([[np.cos(ay), 0.0, np.sin(ay)], [0.0, 1.0, 0.0], [-np.sin(ay), 0.0, np.cos(ay)]])
    Rx = np.array([[1.0, 0.0, 0.0], [0.0, np.cos(ax), -np.sin(ax)], [0.0, np.sin(ax), np.cos(ax)]])
    return Rx @ Ry @ Rz


def augment(src, tgt, rot, trans, noise, rng):
    """ref:datasets/indoor.py:142-168, 569-586 with the reference's draws from `rng` in its order -> dict (float64)."""
    src, tgt = np.asarray(src, np.float64), np.asarray(tgt, np.float64)
    rot, trans = np.asarray(rot, np.float64), np.asarray(trans, np.float64).reshape(3, 1)
    if src.shape[0] > MAX_POINTS:
        src = src[rng.permutation(src.shape[0])[:MAX_POINTS]]
    if tgt.shape[0] > MAX_POINTS:
        tgt = tgt[rng.permutation(tgt.shape[0])[:MAX_POINTS]]
    rot_ab = euler_zyx(rng.rand(3) * np.pi * 2 / 1.0)
    aug_src = rng.rand(1)[0]
    rows = lambda p: (p[:, 0:1] * rot_ab[:, 0] + p[:, 1:2] * rot_ab[:, 1]) + p[:, 2:3] * rot_ab[:, 2]   # matmul(rot_ab, p.T).T
    w2c = np.eye(4)
    w2c[:3, :3] = np.linalg.inv(rot_ab)
    if aug_src > 0.5:
        src = rows(src)
        rot = np.matmul(rot, rot_ab.T)
        w_src, w_tgt = w2c.astype(np.float32), np.eye(4, dtype=np.float32)
    else:
        tgt = rows(tgt)
        rot = np.matmul(rot_ab, rot)
        trans = np.matmul(rot_ab, trans)
        w_src, w_tgt = np.eye(4, dtype=np.float32), w2c.astype(np.float32)
    src = src + (rng.rand(src.shape[0], 3) - 0.5) * noise
    tgt = tgt + (rng.rand(tgt.shape[0], 3) - 0.5) * noise
    return dict(src=src, tgt=tgt, rot=rot, trans=trans, src_world2camera1=w_src, tgt_world2camera1=w_tgt,
                rotate_src=bool(aug_src > 0.5), rot_ab=rot_ab)


def golden_inputs():
    """The seeded frames of tests/golden/indoor_frames.npz (scripts/make_golden_indoor.py resizes them with PIL itself):
    depth 7x11 and 48x64 (uint16, with 0, 1, 32767, 32768 and 65535 among the values), colour 48x64x3 (uint8, with 0 and 255)."""
    rng = np.random.RandomState(15)
    edge = np.array([0, 1, 32767, 32768, 65535], np.uint16)
    d_odd = rng.randint(0, 65536, (2, 7, 11)).astype(np.uint16)
    d_odd[0].reshape(-1)[::3][:20] = np.resize(edge, 20)
    d_odd[1, :, 5] = np.resize(edge, 7)
    d_big = rng.randint(0, 9000, (2, 48, 64)).astype(np.uint16)
    for k in range(2):
        d_big[k].reshape(-1)[k::7] = np.resize(edge, len(d_big[k].reshape(-1)[k::7]))
    color = rng.randint(0, 256, (2, 48, 64, 3)).astype(np.uint8)
    color[0, ::2, 1::2] = 0
    color[1, 1::2, ::3] = 255
    return dict(depth_odd=d_odd, depth_big=d_big, color=color)


GOLDEN_SIZES = dict(depth_odd=(3, 4), depth_big=(12, 16), color=(24, 32))


def load_golden(golden_dir):
    return dict(np.load(os.path.join(golden_dir, GOLDEN)))
