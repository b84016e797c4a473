"""Generate tests/golden/modelnet_prep.npz from the UNMODIFIED reference transforms (ref:datasets/transforms.py, and
get_transforms of ref:datasets/modelnet.py).  Needs the reference checkout beside the repository; no test reads it.

ref:datasets/transforms.py imports as it is.  ref:datasets/modelnet.py is loaded for get_transforms under a private module
name, with inert stubs for the packages it imports at the top and get_transforms never uses (h5py, open3d, torchvision);
scripts/ref_import.py, whose stub of `datasets.modelnet` other generators rely on, is not touched.

Inputs: four synthetic [2048, 6] float32 clouds -- pcrcg_amd.synthetic.modelnet_clouds: the wavy torus of
synthetic.modelnet_pairs with its analytic unit normals.  Cloud 3 has its last eight rows duplicated from other rows, the last of them chosen so that under the `crop`
test chain (idx 3) the two order statistics that bracket the source side's percentile are the two copies: the threshold
then lies ON the tie and both rows are dropped.

Recorded: every sample key of the six chains (three noise types, train and test) and of the `crop` test chain under
partial = [0.7], [0.5, 0.5] and [1.0, 1.0].  Test chains use idx 0..3; train chains run under np.random.seed(1234),
consumed pair after pair.  For every cropped side also the direction, the kept rows (from RandomCrop.crop itself, run on a
copy of the cloud with an index column appended under the same generator state) and the gap between the two order
statistics that bracket the percentile: asserted to exceed 1e-9 or to be exactly zero (the duplicated cloud), which is what
makes an exact mask comparison legitimate.  The reference's own float32 outputs are asserted to lie within the bound the
GPU test applies (tests/modelnet_prep_ref.py transform_bound), so the bound is not fitted to the code under test.
"""
import importlib.util
import os
import sys
import types

import numpy as np

REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.dont_write_bytecode = True
for p in (REPO, REF):
    if p not in sys.path:
        sys.path.insert(0, p)

from pcrcg_amd import modelnet_prep as MP  # noqa: E402
from pcrcg_amd import synthetic  # noqa: E402
from tests import modelnet_prep_ref as PR  # noqa: E402

OUT = os.path.join(REPO, "tests", "golden", "modelnet_prep.npz")
N, B = 2048, 4
CHAINS = [("clean", 256), ("jitter", 256), ("crop", 1024)]      # (noise type, num_points: 717 / 717 holds for `crop` whatever it is)
EXTRA = {"crop_p07": [0.7], "crop_p0505": [0.5, 0.5], "crop_p11": [1.0, 1.0]}
LABELS = np.array([3, 17, 0, 39], dtype=np.int64)


def reference_modules():
    import datasets.transforms as T
    for name in ("h5py", "open3d", "torchvision"):
        if name not in sys.modules:
            try:
                __import__(name)
            except Exception:
                sys.modules[name] = types.ModuleType(name)
    try:
        import lib.benchmark_utils  # noqa: F401
    except Exception:
        stub = types.ModuleType("lib.benchmark_utils")
        stub.get_correspondences = stub.to_o3d_pcd = stub.to_tsfm = None
        sys.modules["lib.benchmark_utils"] = stub
    spec = importlib.util.spec_from_file_location("_pcrcg_ref_datasets_modelnet", os.path.join(REF, "datasets", "modelnet.py"))
    M = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(M)
    return T, M


def torus(seed):
    """One cloud of synthetic.modelnet_clouds -> [2048, 6] float32."""
    return synthetic.modelnet_clouds(seed + 1, 77, n_raw=N)[seed]


def bracket(T, cloud, direction, p_keep):
    """-> (gap between the two order statistics that bracket the percentile, their rows) as the reference computes dist."""
    centroid = np.mean(cloud[:, :3], axis=0)
    dist = np.dot(cloud[:, :3] - centroid, direction)
    lo, _ = MP.percentile_index(len(cloud), p_keep)
    order = np.argsort(dist, kind="stable")
    hi = min(lo + 1, len(cloud) - 1)
    return dist[order[hi]] - dist[order[lo]], (order[lo], order[hi])


def duplicated_cloud(T, seed, idx, p_keep):
    """A torus cloud whose last eight rows are copies of other rows; the last copy makes the source side's percentile
    bracket under np.random.seed(idx) a tie."""
    c = torus(seed)
    c[N - 8:N - 1] = c[100:107]
    np.random.seed(idx)
    direction = T.uniform_2_sphere()
    centroid = np.mean(c[:, :3], axis=0)
    order = np.argsort(np.dot(c[:, :3] - centroid, direction), kind="stable")
    lo, _ = MP.percentile_index(N, p_keep)
    for cand in order[lo - 4:lo + 5]:
        if cand >= N - 8:
            continue
        trial = c.copy()
        trial[N - 1] = trial[cand]
        gap, rows = bracket(T, trial, direction, p_keep)
        if gap == 0.0 and set(rows) == {cand, N - 1}:
            return trial
    raise AssertionError("no row puts the tie on the bracket")


def run_reference(T, transforms, clouds, seed):
    """The reference's loop over the four items -> per pair (sample, crop records)."""
    if seed is not None:
        np.random.seed(seed)
    out = []
    for b in range(B):
        sample = {"points": clouds[b].copy(), "label": LABELS[b], "idx": np.array(b, dtype=np.int32)}
        crops = {}
        for t in transforms:                                                   # torchvision's Compose is this loop
            if isinstance(t, T.RandomCrop) and not np.all(t.p_keep == 1.0):
                state0 = np.random.get_state()
                if sample.get("deterministic"):
                    np.random.seed(sample["idx"])
                for side, p in zip(("src", "ref"), t.p_keep):
                    pts = sample["points_" + side]
                    state = np.random.get_state()
                    direction = T.uniform_2_sphere()
                    np.random.set_state(state)
                    with_index = np.concatenate([pts, np.arange(len(pts), dtype=np.float32)[:, None]], 1)
                    kept = T.RandomCrop.crop(with_index, p)
                    gap, _ = bracket(T, pts, direction, p) if p != 0.5 else (np.inf, None)
                    crops[side] = {"dir": direction, "kept": kept[:, 6].astype(np.int32), "points": kept[:, :6], "gap": gap}
                np.random.set_state(state0)
                sample = t(sample)
                for side in crops:
                    assert np.array_equal(sample["points_" + side], crops[side]["points"]), "the index column changed the crop"
            else:
                sample = t(sample)
        out.append((sample, crops))
    return out


def main():
    T, M = reference_modules()
    clouds = np.stack([torus(0), torus(1), torus(2), duplicated_cloud(T, 3, 3, np.float32(0.7))])
    data = {"clouds": clouds, "labels": LABELS}
    runs = []
    for noise, num in CHAINS:
        train, test = M.get_transforms(noise, num_points=num)
        mine = MP.get_transforms(noise, num_points=num)
        runs += [(f"{noise}_train", train, mine[0], 1234), (f"{noise}_test", test, mine[1], None)]
        data[f"{noise}_train/num_points"] = data[f"{noise}_test/num_points"] = np.int32(num)
    for name, partial in EXTRA.items():
        num = 256 if len(partial) == 1 else 1024
        runs.append((name, M.get_transforms("crop", num_points=num, partial_p_keep=partial)[1],
                     MP.get_transforms("crop", num_points=num, partial_p_keep=partial)[1], None))
        data[f"{name}/num_points"], data[f"{name}/partial"] = np.int32(num), np.array(partial)
    ties = 0
    for name, transforms, steps, seed in runs:
        data[f"{name}/steps"] = np.array([type(t).__name__ for t in transforms])
        rng = np.random.RandomState(1234)
        for b, (sample, crops) in enumerate(run_reference(T, transforms, clouds, seed)):
            stored = {}
            assert sample["transform_gt"].dtype == np.float32 and sample["points_src"].dtype == np.float32
            counts = [len(clouds[b]), len(clouds[b])]
            for s, side in enumerate(("src", "ref")):
                if side in crops:
                    c = crops[side]
                    counts[s] = len(c["kept"])
                    mask = np.zeros(N, dtype=bool)
                    mask[c["kept"]] = True
                    assert np.array_equal(np.nonzero(mask)[0], c["kept"])
                    data[f"{name}/{b}/dir_{side}"], data[f"{name}/{b}/keptbits_{side}"] = c["dir"], np.packbits(mask)
                    data[f"{name}/{b}/gap_{side}"] = np.float64(c["gap"])
                    assert c["gap"] > 1e-9 or (c["gap"] == 0.0 and b == 3), (name, b, side, c["gap"])
                    ties += c["gap"] == 0.0
            data[f"{name}/{b}/kept_counts"] = np.array(counts, dtype=np.int32)
            # the reference's own arrays against the bound of the GPU test, through this project's reading of the draws
            d = MP.draws(N, b, steps, rng, kept_counts=counts)
            _, trace = PR.run_chain(clouds[b], b, steps, d)
            for side, tf in (("src", d["transform"]), ("ref", None)):
                rows, got = clouds[b][trace["rows_" + side]], sample["points_" + side]
                want, bound = PR.transform_bound(rows, tf, trace["noise_" + side])
                assert np.all(np.abs(got[:, :3] - want) <= bound), (name, b, side)
                if tf is not None:
                    want, bound = PR.normal_bound(rows, tf)
                    assert np.all(np.abs(got[:, 3:] - want) <= bound), (name, b, side)
                else:
                    assert np.array_equal(got[:, 3:], rows[:, 3:])
            # what is a copy of input rows is stored as the rows' indices (tests/modelnet_prep_ref.py load_fixture puts the
            # arrays back); everything else as the reference returned it
            for k, v in sample.items():
                v = np.asarray(v)
                if k in ("points_raw", "points_src", "points_ref"):
                    rows = trace["rows_" + k[7:]]
                    if np.array_equal(v, clouds[b][rows]):
                        stored[k + "__rows"] = rows.astype(np.int16)
                    elif np.array_equal(v[:, 3:], clouds[b][rows][:, 3:]):
                        stored[k + "__rows"], stored[k + "__xyz"] = rows.astype(np.int16), v[:, :3]
                    else:
                        stored[k] = v
                else:
                    stored[k] = v
            for k, v in stored.items():
                data[f"{name}/{b}/{k}"] = v
    assert ties >= 1, "the duplicated cloud never put a tie on a bracket"
    np.savez_compressed(OUT, **data)
    back = PR.load_fixture(OUT)
    for name, transforms, steps, seed in runs:
        for b, (sample, crops) in enumerate(run_reference(T, transforms, clouds, seed)):
            for k, v in sample.items():
                assert np.array_equal(back[name]["samples"][b][k], v) and back[name]["samples"][b][k].dtype == np.asarray(v).dtype, (name, b, k)
    print("modelnet_prep.npz", os.path.getsize(OUT), "bytes,", len(data), "arrays,", ties, "tied brackets")


if __name__ == "__main__":
    main()
