"""Preparing ModelNet pairs on the device: the body of ref:datasets/modelnet.py ModelNetHdf.__getitem__ (:174-197) after the
h5 arrays are in memory -- the transform chains of get_transforms (:59-130, ref:datasets/transforms.py) for the three noise
types in train and test form, the ground-truth correspondences and the item dicts -- batched over pairs.  (modelnet.py is
the other end: the evaluation of the estimated poses.)

  * `get_transforms`   -- ref:datasets/modelnet.py:59-130 as data: (train, test), each a tuple of (step, params).
  * `resample_sizes`   -- Resampler's sizes (ref:datasets/transforms.py:75-86), the hard-coded 717 / 717 included.
  * `percentile_index` -- numpy's rule for np.percentile(x, (1.0 - np.float32(p)) * 100): the lower order statistic and weight.
  * `draws`            -- every random number one pair's chain consumes, drawn on the host from a numpy.random.RandomState
                          in the reference's order and shapes, reseeded with `idx` where SetDeterministic makes a step reseed.
  * `crop_batch`       -- RandomCrop.crop (:164-176) for many clouds in ONE library call (pcrcg_modelnet_crop;
                          include/pcrcg.h "ModelNet pair preparation").
  * `transform_pairs`  -- a chain for B pairs -> B `sample` dicts with the reference's keys: one crop call, one read-back
                          of the 2 B kept counts, the remaining draws on the host, one pcrcg_modelnet_assemble call.
  * `prepare_pairs`    -- :174-197 for B pairs -> the dicts pyramid.collate_fn_descriptor takes, ONE
                          get_correspondences_batch call; `prepare_pair` is a batch of one.

Every random step of the chains reduces to index arrays, a noise array, two directions and one [3, 4] matrix
(np.random.permutation(array) is array[np.random.permutation(n)]; choice(n, k, replace=False) is permutation(n)[:k]), so the
host draws and composes indices and the device does the rest: the crop (centroid, projection, two order statistics, stable
compaction) and one pass that gathers, moves and jitters every output row.

Quirks of the reference that are kept: with a two-element `partial` the Resampler's sizes are 717 / 717 whatever num_points
and the proportions are (ref:datasets/transforms.py:83-84); rows whose distance ties with the percentile are dropped by the
literal `dist > percentile`; `clean` resamples before the split, so its points_raw is the resampled cloud.

The h5 reader is not here: the input is the [S, n, 6] float32 array and the labels that _read_h5_files returns.
"""
import math

import numpy as np
import torch

from . import _lib, ragged
from .config import as_config
from .correspondences import get_correspondences_batch

# library calls and device-to-host reads made by this module (tests count them: per transform_pairs call one of each
# whenever the cropped sizes come out as the percentile rule predicts -- see transform_pairs)
CALLS = {"crop": 0, "assemble": 0, "read_back": 0}

CROP_MAX_ROWS = 8192        # PCRCG_MODELNET_CROP_MAX_ROWS: what one workgroup of pcrcg_modelnet_crop holds
_MAX_CLOUDS = 1 << 20       # pcrcg_modelnet_crop: C; pcrcg_modelnet_assemble: K
_MAX_ROWS = 1 << 30         # ... and n_total, m_total
_KEEP_ALL, _HALF, _PERCENTILE = 0, 1, 2

_DRAWING = ("Resampler", "RandomCrop", "RandomTransformSE3_euler", "RandomJitter", "ShufflePoints")


def get_transforms(noise_type, rot_mag=45.0, trans_mag=0.5, num_points=1024, partial_p_keep=None):
    """ref:datasets/modelnet.py:59-130 -> (train, test): each a tuple of (step, params), the reference's transforms by
    class name in its order.  noise_type: 'clean', 'jitter' or 'crop'; anything else raises NotImplementedError."""
    p_keep = [float(p) for p in (partial_p_keep if partial_p_keep is not None else [0.7, 0.7])]       # :81
    se3 = ("RandomTransformSE3_euler", {"rot_mag": float(rot_mag), "trans_mag": float(trans_mag)})
    resample = ("Resampler", {"num": int(num_points)})
    split, shuffle, det = ("SplitSourceRef", {}), ("ShufflePoints", {}), ("SetDeterministic", {})
    jitter = ("RandomJitter", {"scale": 0.01, "clip": 0.05})
    if noise_type == "clean":                                                                          # :83-94
        return (resample, split, se3, shuffle), (det, ("FixedResampler", {"num": int(num_points)}), split, se3, shuffle)
    if noise_type == "jitter":                                                                         # :96-109
        train = (split, se3, resample, jitter, shuffle)
    elif noise_type == "crop":                                                                         # :111-126
        train = (split, ("RandomCrop", {"p_keep": p_keep}), se3, resample, jitter, shuffle)
    else:
        raise NotImplementedError(f"get_transforms: noise_type {noise_type!r} (the reference has clean, jitter and crop)")
    return train, (det,) + train


def resample_sizes(num, crop_proportion=None):
    """Resampler's (src, ref) sizes (ref:datasets/transforms.py:75-86).  No crop_proportion: (num, num); one element:
    (ceil(p * num), num); two elements: (717, 717) -- the reference overwrites what it has just computed (:83-84), whatever
    num and the proportions are, and so does this."""
    if crop_proportion is None:
        return int(num), int(num)
    p = np.asarray(crop_proportion, dtype=np.float32).reshape(-1)
    if len(p) == 1:
        return int(math.ceil(p[0] * num)), int(num)
    if len(p) == 2:
        return 717, 717
    raise ValueError("Crop proportion must have 1 or 2 elements")


def percentile_index(n, p_keep):
    """-> (lo, gamma) such that np.percentile(x, (1.0 - np.float32(p_keep)) * 100) of n values is the lerp of the lo-th and
    (lo+1)-th smallest with weight gamma (numpy's 'linear' method: a + (b - a) * gamma, or b - (b - a) * (1 - gamma) for
    gamma >= 0.5); lo = n - 1 with gamma 0 where the virtual index reaches the last value."""
    n = int(n)
    if n < 1:
        raise ValueError(f"percentile_index: n must be at least 1, got {n}")
    q = np.true_divide((1.0 - np.float32(p_keep)) * 100, np.float64(100))
    if not 0.0 <= q <= 1.0:
        raise ValueError(f"percentile_index: p_keep must lie in [0, 1], got {p_keep!r}")
    virtual = (n - 1) * q                                   # numpy's virtual index of the 'linear' method
    if virtual >= n - 1:
        return n - 1, 0.0
    if virtual < 0:
        return 0, 0.0
    lo = int(np.floor(virtual))
    return lo, float(virtual - lo)


def _uniform_2_sphere(rng):
    """ref:datasets/transforms.py:13-38 with num=None."""
    phi = rng.uniform(0.0, 2 * np.pi)
    cos_theta = rng.uniform(-1.0, 1.0)
    theta = np.arccos(cos_theta)
    return np.stack((np.sin(theta) * np.cos(phi), np.sin(theta) * np.sin(phi), np.cos(theta)), axis=-1)


def _euler_transform(rng, rot_mag, trans_mag):
    """RandomTransformSE3_euler.generate_transform (ref:datasets/transforms.py:269-301) -> float32 [3, 4]."""
    anglex = rng.uniform() * np.pi * rot_mag / 180.0
    angley = rng.uniform() * np.pi * rot_mag / 180.0
    anglez = rng.uniform() * np.pi * rot_mag / 180.0
    cosx, cosy, cosz = np.cos(anglex), np.cos(angley), np.cos(anglez)
    sinx, siny, sinz = np.sin(anglex), np.sin(angley), np.sin(anglez)
    Rx = np.array([[1, 0, 0], [0, cosx, -sinx], [0, sinx, cosx]])
    Ry = np.array([[cosy, 0, siny], [0, 1, 0], [-siny, 0, cosy]])
    Rz = np.array([[cosz, -sinz, 0], [sinz, cosz, 0], [0, 0, 1]])
    R_ab = Rx @ Ry @ Rz
    t_ab = rng.uniform(-trans_mag, trans_mag, 3)
    return np.concatenate((R_ab, t_ab[:, None]), axis=1).astype(np.float32)


def _se3_inverse(g):
    """ref:common/math/se3.py:26-44 for a [3, 4]."""
    rot, trans = g[:3, :3], g[:3, 3]
    inv_rot = np.swapaxes(rot, -1, -2)
    return np.concatenate([inv_rot, inv_rot @ -trans[..., None]], axis=-1)


def _resample_draw(rng, n, k):
    """Resampler._resample's index array (ref:datasets/transforms.py:103-111)."""
    if k <= n:
        return rng.choice(n, k, replace=False)
    return np.concatenate([rng.choice(n, n, replace=False), rng.choice(n, k - n, replace=True)])


def _crop_mode(p):
    return _HALF if p == 0.5 else _PERCENTILE


def _predicted_kept(n, p):
    """How many rows RandomCrop.crop keeps of n when no distance ties with the threshold: every row above the lower order
    statistic.  (The half-space mode keeps what the data says; n // 2 is a guess.)"""
    return n // 2 if p == 0.5 else n - percentile_index(n, p)[0] - 1


def draws(n_raw, idx, steps, rng, kept_counts=None):
    """The random numbers one pair's chain consumes from `rng` (a numpy.random.RandomState; the reference draws from
    numpy's global one), in the reference's call order and shapes -> dict.  After SetDeterministic, RandomCrop,
    RandomTransformSE3_euler and Resampler each reseed `rng` with `idx` before they draw; RandomJitter and ShufflePoints
    never do.  Keys, as the chain has the steps: resample_points / resample_src / resample_ref (index arrays: choice without
    replacement, then with replacement for the rows beyond the cloud's size; FixedResampler's arange(num) % n draws
    nothing), dir_src / dir_ref (float64 [3], uniform_2_sphere), crop_proportion (float32), transform (float32 [3, 4]:
    Rx @ Ry @ Rz and the translation, rounded) and transform_gt (its inverse as se3.inverse forms it), noise_src /
    noise_ref (float64 [n, 3], clipped), perm_points / perm_ref / perm_src (ShufflePoints draws the reference side first),
    kept_counts (the (src, ref) sizes after RandomCrop; n_raw for a side that is not cropped) and predicted.

    kept_counts: the sizes the crop left, which the draws after it depend on.  None: the sizes the percentile rule predicts
    (n - lo - 1; n // 2 for p_keep 0.5) and predicted=True -- what transform_pairs draws before it has read the counts."""
    n, split, det, crop_prop = int(n_raw), False, False, None
    ns = nr = None
    d = {"predicted": False, "kept_counts": (n, n)}

    def reseed():
        if det:
            rng.seed(int(idx))

    for step, prm in steps:
        if step == "SetDeterministic":
            det = True
        elif step == "FixedResampler":
            if split:
                raise NotImplementedError("draws: FixedResampler after SplitSourceRef is in none of the reference's chains")
            d["resample_points"] = np.arange(int(prm["num"])) % n
            n = int(prm["num"])
        elif step == "Resampler":
            reseed()
            if not split:
                d["resample_points"] = _resample_draw(rng, n, int(prm["num"]))
                n = int(prm["num"])
            else:
                ks, kr = resample_sizes(prm["num"], crop_prop)
                d["resample_src"] = _resample_draw(rng, ns, ks)
                d["resample_ref"] = _resample_draw(rng, nr, kr)
                ns, nr = ks, kr
        elif step == "SplitSourceRef":
            split, ns, nr = True, n, n
        elif step == "RandomCrop":
            if not split:
                raise NotImplementedError("draws: RandomCrop before SplitSourceRef is in none of the reference's chains")
            p = np.array(prm["p_keep"], dtype=np.float32)
            if len(p) not in (1, 2):
                raise ValueError("Crop proportion must have 1 or 2 elements")
            d["crop_proportion"] = crop_prop = p
            if np.all(p == 1.0):
                continue
            reseed()
            d["dir_src"] = _uniform_2_sphere(rng)
            if len(p) == 2:
                d["dir_ref"] = _uniform_2_sphere(rng)
            if kept_counts is None:
                d["predicted"] = True
                ns = _predicted_kept(ns, p[0])
                nr = _predicted_kept(nr, p[1]) if len(p) == 2 else nr
            else:
                ns, nr = int(kept_counts[0]), int(kept_counts[1])
            if ns < 1 or nr < 1:
                raise ValueError(f"pair idx {int(idx)}: the crop keeps no row of the {'source' if ns < 1 else 'reference'} cloud")
            d["kept_counts"] = (ns, nr)
        elif step == "RandomTransformSE3_euler":
            if not split:
                raise NotImplementedError("draws: RandomTransformSE3_euler before SplitSourceRef is in none of the reference's chains")
            reseed()
            d["transform"] = _euler_transform(rng, prm["rot_mag"], prm["trans_mag"])
            d["transform_gt"] = _se3_inverse(d["transform"])
        elif step == "RandomJitter":
            if not split:
                raise NotImplementedError("draws: RandomJitter before SplitSourceRef is in none of the reference's chains")
            d["noise_src"] = np.clip(rng.normal(0.0, scale=prm["scale"], size=(ns, 3)), a_min=-prm["clip"], a_max=prm["clip"])
            d["noise_ref"] = np.clip(rng.normal(0.0, scale=prm["scale"], size=(nr, 3)), a_min=-prm["clip"], a_max=prm["clip"])
        elif step == "ShufflePoints":
            if not split:
                d["perm_points"] = rng.permutation(n)
            else:
                d["perm_ref"] = rng.permutation(nr)
                d["perm_src"] = rng.permutation(ns)
        else:
            raise NotImplementedError(f"draws: unknown step {step!r}")
    d["deterministic"] = det
    return d


def _take(cur, index):
    return index if cur is None else cur[index]


def compose(steps, d):
    """One pair's chain under the draws `d` as what pcrcg_modelnet_assemble takes -> dict: `base` (None, or the index of
    every points_raw row in the input cloud: the steps before the split), and per side `pick_src` / `pick_ref` (the index
    of every output row in the side's kept list; the resample index taken through the shuffle), `noise_src` / `noise_ref`
    (None, or the jitter in output order) and `moved` (whether the source goes through `transform`).  A chain whose steps
    cannot be written that way (a transform after the jitter, a crop after a resample) raises NotImplementedError."""
    base, split = None, False
    pick = {"src": None, "ref": None}
    noise = {"src": None, "ref": None}
    moved = False
    for step, prm in steps:
        if step in ("Resampler", "FixedResampler"):
            if not split:
                base = _take(base, d["resample_points"])
            else:
                for s in ("src", "ref"):
                    r = d["resample_" + s]
                    pick[s] = _take(pick[s], r)
                    noise[s] = None if noise[s] is None else noise[s][r]
        elif step == "SplitSourceRef":
            split = True
            pick["src"] = pick["ref"] = base
        elif step == "RandomCrop":
            if "dir_src" in d and (base is not None or pick["src"] is not None or pick["ref"] is not None or moved
                                   or noise["src"] is not None or noise["ref"] is not None):
                raise NotImplementedError("compose: RandomCrop comes first after the split in every chain of the reference")
        elif step == "RandomTransformSE3_euler":
            if moved or noise["src"] is not None:
                raise NotImplementedError("compose: one RandomTransformSE3_euler, before the jitter")
            moved = True
        elif step == "RandomJitter":
            for s in ("src", "ref"):
                if noise[s] is not None:
                    raise NotImplementedError("compose: one RandomJitter per chain")
                noise[s] = d["noise_" + s]
        elif step == "ShufflePoints":
            if not split:
                base = _take(base, d["perm_points"])
            else:
                for s in ("src", "ref"):
                    pick[s] = _take(pick[s], d["perm_" + s])
                    noise[s] = None if noise[s] is None else noise[s][d["perm_" + s]]
    if not split:
        raise NotImplementedError("compose: a chain without SplitSourceRef makes no pair")
    return {"base": base, "pick_src": pick["src"], "pick_ref": pick["ref"], "noise_src": noise["src"],
            "noise_ref": noise["ref"], "moved": moved}


def _device(clouds):
    return ragged.device(clouds, "modelnet_prep")


def _cloud_list(points, who):
    """A [B, n, ld] array / tensor or a list of [n_b, ld] clouds -> (list, ld) after the checks that need no device."""
    clouds = list(points)
    if len(clouds) == 0:
        raise ValueError(f"{who}: no clouds")
    ld = None
    for b, x in enumerate(clouds):
        shape = ragged.shape_of(x)
        if len(shape) != 2 or shape[1] not in (3, 6):
            raise ValueError(f"{who}: cloud {b} must be an [n, 3] or [n, 6] array, got shape {shape}")
        if ld is None:
            ld = shape[1]
        elif shape[1] != ld:
            raise ValueError(f"{who}: cloud {b} has {shape[1]} columns, the others {ld}")
        if shape[0] < 1:
            raise ValueError(f"{who}: cloud {b} is empty")
        if shape[0] > CROP_MAX_ROWS:
            raise ValueError(f"{who}: cloud {b} has {shape[0]} rows, one workgroup holds {CROP_MAX_ROWS}")
    return clouds, ld


def _upload(clouds, dev):
    """-> the clouds as one float32 device stack (host clouds travel in one upload)."""
    return ragged.upload(clouds, dev, torch.float32, name="clouds")


def _crop(stack, ld, off, first, params, kept, count):
    """ONE pcrcg_modelnet_crop call for the clouds first .. of the stack (off: the host's [C+1] offsets; params: per cloud
    (mode, dir, lo, gamma)) into the rows of `kept` / `count` that belong to them -> their counts from ONE read-back."""
    dev = stack.device
    C = len(params)
    ints = np.concatenate([np.asarray(off[first:first + C + 1], dtype=np.int32), np.array([p[0] for p in params], dtype=np.int32),
                           np.array([p[2] for p in params], dtype=np.int32)])
    reals = np.concatenate([np.array([p[1] for p in params], dtype=np.float64).reshape(-1),
                            np.array([p[3] for p in params], dtype=np.float64)])
    ints, reals = torch.from_numpy(ints).to(dev), torch.from_numpy(reals).to(dev)
    max_rows = int(max(off[c + 1] - off[c] for c in range(first, first + C)))
    _lib.check(_lib.lib().pcrcg_modelnet_crop(stack.data_ptr(), ld, stack.shape[0], ints.data_ptr(), C, max(max_rows, 1),
                                              ints[C + 1:].data_ptr(), reals.data_ptr(), ints[2 * C + 1:].data_ptr(),
                                              reals[3 * C:].data_ptr(), kept.data_ptr(), count[first:].data_ptr(),
                                              torch.cuda.current_stream(dev).cuda_stream), "pcrcg_modelnet_crop")
    CALLS["crop"] += 1
    got = count[first:first + C].cpu().numpy()
    CALLS["read_back"] += 1
    return got


def crop_batch(clouds, directions, p_keep):
    """RandomCrop.crop (ref:datasets/transforms.py:164-176) for C clouds in ONE pcrcg_modelnet_crop call and one
    read-back -> a list of C int32 device tensors: the kept rows' indices, ascending.

    clouds: [n_c, 3] or [n_c, 6] arrays (numpy, CPU or HIP tensors; rounded to float32), 1 to 8192 rows each; directions:
    [C, 3] float64, the planes' normals (uniform_2_sphere's draws); p_keep: one value or one per cloud -- 0.5 keeps the
    rows with dist > 0, any other value those with dist > np.percentile(dist, (1.0 - np.float32(p)) * 100), and None keeps
    the cloud whole.  The mask is the reference's literal comparison: rows that tie with the threshold are dropped, so a
    cloud of one row keeps nothing.  A cloud with a non-finite coordinate raises ValueError naming it."""
    clouds, ld = _cloud_list(clouds, "crop_batch")
    C = len(clouds)
    if C > _MAX_CLOUDS:
        raise ValueError(f"crop_batch: {C} clouds in one call, at most {_MAX_CLOUDS}")
    dirs = np.asarray(directions.cpu() if isinstance(directions, torch.Tensor) else directions, dtype=np.float64)
    if dirs.shape != (C, 3):
        raise ValueError(f"crop_batch: directions must be [{C}, 3], got {dirs.shape}")
    ps = list(p_keep) if isinstance(p_keep, (list, tuple, np.ndarray)) else [p_keep] * C
    if len(ps) != C:
        raise ValueError(f"crop_batch: {len(ps)} p_keep values for {C} clouds")
    ns = [int(x.shape[0]) for x in clouds]
    off = np.cumsum([0] + ns)
    if off[-1] > _MAX_ROWS:
        raise ValueError(f"crop_batch: {off[-1]} rows in one call, at most {_MAX_ROWS}")
    params = []
    for c in range(C):
        if ps[c] is None:
            params.append((_KEEP_ALL, np.zeros(3), 0, 0.0))
        else:
            lo, gamma = percentile_index(ns[c], ps[c])
            params.append((_crop_mode(np.float32(ps[c])), dirs[c], lo, gamma))
    dev = _device(clouds)
    stack = _upload(clouds, dev)
    kept = torch.empty(int(off[-1]), dtype=torch.int32, device=dev)
    count = torch.empty(C, dtype=torch.int32, device=dev)
    got = _crop(stack, ld, off, 0, params, kept, count)
    for c in range(C):
        if got[c] < 0:
            raise ValueError(f"crop_batch: cloud {c} was rejected: it has a non-finite coordinate")
    return [kept[off[c]:off[c] + int(got[c])] for c in range(C)]


def _pair_crop_params(steps, d, n):
    """The (mode, dir, lo, gamma) of a pair's source and reference clouds of n rows under its draws."""
    keep = (_KEEP_ALL, np.zeros(3), 0, 0.0)
    out = [keep, keep]
    if "dir_src" in d:
        p = d["crop_proportion"]
        for s, key in enumerate(("dir_src", "dir_ref")[:len(p)]):
            lo, gamma = percentile_index(n, p[s])
            out[s] = (_crop_mode(p[s]), d[key], lo, gamma)
    return out


def _reseeds_first(steps):
    """Whether every pair's first draw follows a reseed, so that no pair's numbers depend on the pair before it."""
    det = False
    for step, prm in steps:
        if step == "SetDeterministic":
            det = True
        elif step == "RandomCrop" and np.all(np.asarray(prm["p_keep"], dtype=np.float32) == 1.0):
            continue
        elif step in _DRAWING:
            return det and step in ("Resampler", "RandomCrop", "RandomTransformSE3_euler")
    return True


def transform_pairs(points, idxs, steps, rng, labels=None):
    """A transform chain of get_transforms for B pairs -> a list of B `sample` dicts with the reference's keys: points_raw,
    points_src, points_ref (float32 device tensors that keep every input column: 3, or 6 with the normals, which are
    rotated with the source and never jittered), transform_gt (float32 [3, 4] numpy: source -> reference), idx (int32
    0-d array), and crop_proportion (float32 numpy), deterministic and label where the chain or the caller gives them.

    points: [B, n, 3|6] array or tensor, or a list of [n_b, 3|6] clouds (numpy, CPU or HIP tensors; 1 to 8192 rows);
    idxs: the B dataset indices (what SetDeterministic's steps reseed with); steps: one of get_transforms' tuples; rng: a
    numpy.random.RandomState, consumed pair after pair exactly as the reference's loop consumes numpy's global one.

    Two phases, because the Resampler's draws need the cropped sizes: ONE pcrcg_modelnet_crop call for the 2 B sides (a
    side that is not cropped passes whole -- the call is also what rejects non-finite coordinates), ONE read-back of the
    2 B kept counts, the remaining draws on the host, ONE pcrcg_modelnet_assemble call that gathers, moves and jitters
    every output row of the batch.  In a chain without SetDeterministic the crop directions of pair b + 1 come after every
    draw of pair b, whose number depends on pair b's kept counts; those are drawn ahead with the counts the percentile rule
    predicts (n - lo - 1).  Where a read count differs -- a distance tied with the threshold, or p_keep = 0.5, whose count
    only the data knows -- the generator is put back, that pair is redrawn with its true counts and the pairs after it go
    through another crop call: always the reference's numbers, at the price of further calls (CALLS counts them).  The
    worst case is a train chain with p_keep = 0.5: nothing predicts its counts, so it is cropped pair by pair -- B crop
    calls and B read-backs of one pair each (every cloud still cropped once).  The reference's own configurations
    (partial [0.7, 0.7]; every test chain) take the one call.

    ValueError naming the cloud: an empty cloud or one of more than 8192 rows, a non-finite coordinate, a crop that keeps
    no row (the reference's choice() raises there too)."""
    clouds, ld = _cloud_list(points, "transform_pairs")
    B = len(clouds)
    idxs = [int(i) for i in idxs]
    if len(idxs) != B or (labels is not None and len(labels) != B):
        raise ValueError(f"transform_pairs: {B} clouds, {len(idxs)} idxs" + ("" if labels is None else f", {len(labels)} labels"))
    if 3 * B > _MAX_CLOUDS:
        raise ValueError(f"transform_pairs: {B} pairs in one call, at most {_MAX_CLOUDS // 3}")
    steps = tuple(steps)
    ns = [int(x.shape[0]) for x in clouds]
    if 2 * sum(ns) > _MAX_ROWS:
        raise ValueError(f"transform_pairs: {2 * sum(ns)} rows in one call, at most {_MAX_ROWS}")
    dev = _device(clouds)
    raw = list(_upload(clouds, dev).split(ns))
    stack = torch.cat([raw[b] for b in range(B) for _ in range(2)]).contiguous()          # cloud 2 b: source, 2 b + 1: reference
    off = np.cumsum([0] + [ns[b] for b in range(B) for _ in range(2)])
    kept = torch.empty(int(off[-1]), dtype=torch.int32, device=dev)
    count = torch.empty(2 * B, dtype=torch.int32, device=dev)

    independent = _reseeds_first(steps)
    # a chain whose pairs depend on one another and whose kept counts nothing predicts (p_keep = 0.5) goes pair by pair:
    # drawing ahead would be wrong every time, and every miss would crop all the later pairs again
    ahead = independent or not any(step == "RandomCrop" and np.any(np.asarray(prm["p_keep"], dtype=np.float32) == 0.5)
                                   for step, prm in steps)
    final = [None] * B
    start = 0
    while start < B:
        stop = B if ahead else start + 1
        states, trial = [], []
        for b in range(start, stop):
            states.append(rng.get_state())
            trial.append(draws(ns[b], idxs[b], steps, rng))
        params = [p for b in range(start, stop) for p in _pair_crop_params(steps, trial[b - start], ns[b])]
        got = _crop(stack, ld, off, 2 * start, params, kept, count).reshape(-1, 2)
        b = start
        while b < stop:
            g = got[b - start]
            for s in range(2):
                if g[s] < 0:
                    raise ValueError(f"transform_pairs: cloud {b} (idx {idxs[b]}) was rejected: it has a non-finite coordinate")
                if g[s] == 0:
                    raise ValueError(f"transform_pairs: cloud {b} (idx {idxs[b]}): the crop keeps no row of the "
                                     f"{'source' if s == 0 else 'reference'} cloud")
            if (int(g[0]), int(g[1])) == tuple(trial[b - start]["kept_counts"]):
                final[b] = trial[b - start]
                b += 1
                continue
            end_state = rng.get_state()
            rng.set_state(states[b - start])
            final[b] = draws(ns[b], idxs[b], steps, rng, kept_counts=(int(g[0]), int(g[1])))
            b += 1
            if not independent:
                break                                     # the pairs after it were drawn from the wrong place
            if b < stop:
                rng.set_state(end_state)                  # (the last pair leaves the generator where its true draws end)
        start = b

    # the output clouds: per pair the source, the reference, and points_raw where the chain resamples before the split
    jobs = []                                             # (pair, key, input cloud, pick, noise, transform)
    for b in range(B):
        d = final[b]
        plan = compose(steps, d)
        tf = d.get("transform") if plan["moved"] else None
        jobs.append((b, "points_src", 2 * b, plan["pick_src"], plan["noise_src"], tf))
        jobs.append((b, "points_ref", 2 * b + 1, plan["pick_ref"], plan["noise_ref"], None))
        if plan["base"] is not None:
            jobs.append((b, "points_raw", 2 * b, plan["base"], None, None))
    K = len(jobs)
    counts_h = [c for b in range(B) for c in final[b]["kept_counts"]]
    picks = [np.arange(counts_h[j[2]]) if j[3] is None else np.asarray(j[3]) for j in jobs]
    ms = [len(p) for p in picks]
    out_off = np.cumsum([0] + ms)
    m_total = int(out_off[-1])
    if m_total > _MAX_ROWS:
        raise ValueError(f"transform_pairs: {m_total} output rows in one call, at most {_MAX_ROWS}")
    flags = [(1 if j[5] is not None else 0) | (2 if j[4] is not None else 0) for j in jobs]
    ints = torch.from_numpy(np.concatenate([out_off, [j[2] for j in jobs], flags, np.concatenate(picks)]).astype(np.int32)).to(dev)
    tfs = np.zeros((K, 12), dtype=np.float32)
    for k, j in enumerate(jobs):
        if j[5] is not None:
            tfs[k] = np.asarray(j[5], dtype=np.float32).reshape(12)
    tfs = torch.from_numpy(tfs).to(dev)
    noise = None
    if any(j[4] is not None for j in jobs):
        noise = np.zeros((m_total, 3), dtype=np.float64)
        for k, j in enumerate(jobs):
            if j[4] is not None:
                noise[out_off[k]:out_off[k + 1]] = j[4]
        noise = torch.from_numpy(noise).to(dev)
    in_off = torch.from_numpy(off.astype(np.int32)).to(dev)
    out = torch.empty((m_total, ld), dtype=torch.float32, device=dev)
    _lib.check(_lib.lib().pcrcg_modelnet_assemble(stack.data_ptr(), ld, stack.shape[0], in_off.data_ptr(), 2 * B, kept.data_ptr(),
                                                  count.data_ptr(), ints.data_ptr(), ints[K + 1:].data_ptr(),
                                                  ints[2 * K + 1:].data_ptr(), tfs.data_ptr(), K, ints[3 * K + 1:].data_ptr(),
                                                  noise.data_ptr() if noise is not None else None, m_total, out.data_ptr(),
                                                  torch.cuda.current_stream(dev).cuda_stream), "pcrcg_modelnet_assemble")
    CALLS["assemble"] += 1
    parts = out.split(ms)
    samples = []
    for b in range(B):
        d = final[b]
        s = {}
        if labels is not None:
            s["label"] = labels[b]
        s["idx"] = np.array(idxs[b], dtype=np.int32)
        if d["deterministic"]:
            s["deterministic"] = True
        s["points_raw"] = raw[b]
        samples.append(s)
    for k, j in enumerate(jobs):
        samples[j[0]][j[1]] = parts[k]
    for b in range(B):
        d = final[b]
        if "crop_proportion" in d:
            samples[b]["crop_proportion"] = d["crop_proportion"]
        if "transform_gt" in d:
            samples[b]["transform_gt"] = d["transform_gt"]
    return samples


def prepare_pairs(points, labels, idxs, config, *, subset="test", rng=None):
    """ref:datasets/modelnet.py:174-197 for B pairs -> a list of B dicts, what pyramid.collate_fn_descriptor takes.

    points: [B, n, 3|6] (the rows of _read_h5_files' data the pairs are made from), labels: their B labels or None, idxs:
    their dataset indices.  config: noise_type, rot_mag, trans_mag, num_points, partial (get_transforms' arguments;
    modelnet_config() carries ref:configs/test/modelnet.yaml's), overlap_radius and in_feats_dim.  subset: 'train' takes
    get_transforms' train chain, anything else ('val', 'test') its test chain, as the reference's datasets do.  rng: a
    numpy.random.RandomState; None: numpy's global one, which is what the reference draws from.

    Every dict holds src_pcd, tgt_pcd ([n, 3] fp32 device tensors: the xyz of points_src / points_ref), src_feats,
    tgt_feats (ones [n, 1] for in_feats_dim = 1, the xyz for 3), rot [3, 3] and trans [3, 1] (fp32 numpy, from
    transform_gt), correspondences ([K, 2] int64 device: ONE get_correspondences_batch call for all pairs at
    config.overlap_radius under transform_gt), n_correspondences, and sample: transform_pairs' dict with the leading batch
    dimension of one the reference's loader leaves on every array (tester.evaluate_modelnet_records accepts it).

    The reference searches the correspondences among float64 copies of the fp32 clouds; this searches the fp32 clouds the
    network is fed, under the same fp32 transform_gt, as kitti.prepare_pairs and indoor.prepare_pairs do."""
    config = as_config(config)
    train, test = get_transforms(config.noise_type, config.rot_mag, config.trans_mag, config.num_points, config.partial)
    if rng is None:
        # numpy's global legacy generator, the one np.random.seed() seeds and the reference draws from.  numpy exposes it
        # only under this private name; should it go away, the caller has to hand a generator over.
        rng = getattr(np.random.mtrand, "_rand", None)
        if rng is None:
            raise RuntimeError("prepare_pairs: this numpy does not expose its global RandomState; pass rng=")
    samples = transform_pairs(points, idxs, train if subset == "train" else test, rng, labels=labels)
    n_feats = int(config.get("in_feats_dim", 1))
    if n_feats not in (1, 3):
        raise ValueError(f"prepare_pairs: in_feats_dim must be 1 or 3, got {n_feats}")
    srcs = [s["points_src"][:, :3].contiguous() for s in samples]
    tgts = [s["points_ref"][:, :3].contiguous() for s in samples]
    tsfms = []
    for s in samples:
        t = np.eye(4)
        t[:3, :] = s["transform_gt"]                                                              # to_tsfm, :184
        tsfms.append(t)
    corrs = get_correspondences_batch(srcs, tgts, tsfms, config.overlap_radius)
    items = []
    for b, s in enumerate(samples):
        dev = srcs[b].device
        feats = [torch.ones((x.shape[0], 1), dtype=torch.float32, device=dev) if n_feats == 1 else x for x in (srcs[b], tgts[b])]
        sample = {}
        for k, v in s.items():
            if k in ("deterministic", "label", "idx"):                                            # :193-195
                sample[k] = v
            else:
                sample[k] = (v if isinstance(v, torch.Tensor) else torch.from_numpy(v)).unsqueeze(0)
        items.append({"src_pcd": srcs[b], "tgt_pcd": tgts[b], "src_feats": feats[0], "tgt_feats": feats[1],
                      "rot": s["transform_gt"][:, :3].copy(), "trans": s["transform_gt"][:, 3][:, None].copy(),
                      "correspondences": corrs[b], "sample": sample, "n_correspondences": int(corrs[b].shape[0])})
    return items


def prepare_pair(points, label, idx, config, *, subset="test", rng=None):
    """One pair -> its dict: prepare_pairs with a batch of one."""
    return prepare_pairs([points], None if label is None else [label], [idx], config, subset=subset, rng=rng)[0]
