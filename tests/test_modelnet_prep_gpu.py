"""GPU: ModelNet pair preparation (pcrcg_modelnet_crop, pcrcg_modelnet_assemble: csrc/modelnet.hip; pcrcg_amd/modelnet_prep.py)
against the unmodified reference's recorded run tests/golden/modelnet_prep.npz and the numpy restatement
tests/modelnet_prep_ref.py.

Masks and everything derived from indices are compared exactly (the fixture's generator asserts that no distance lies within
1e-9 of a percentile threshold except the one tie it builds on purpose).  Transformed coordinates are compared with the
float64 evaluation of the same expression from the same float32 inputs, within 4 * 2^-23 * (|x r0| + |y r1| + |z r2| + |t|)
plus one float32 rounding of the jittered sum (modelnet_prep_ref.transform_bound): the standard bound of a four-term float32
sum with a factor of two to spare, which the reference's own arrays satisfy (asserted by the generator)."""
import os

import numpy as np
import pytest
import torch

from pcrcg_amd import _lib, modelnet_config
from pcrcg_amd import modelnet_prep as MP

from . import modelnet_prep_ref as PR
from .test_modelnet_prep_cpu import EXTRA, MAIN, _bits, steps_of

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "modelnet_prep.npz")
CAP = 8192


@pytest.fixture(scope="module")
def fx(cuda):
    return PR.load_fixture(GOLDEN)


def _np(t):
    return t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)


def test_crop_batch_on_the_fixture_clouds(fx):
    """Every cropped side of every chain of the fixture in ONE call: kept rows and counts equal the reference's exactly,
    no cloud left out.  Cloud 3 of the `crop` test chain has its threshold on a tie: both copies go."""
    clouds, dirs, ps, want, who = [], [], [], [], []
    for name in MAIN + EXTRA:
        for b, crop in enumerate(fx[name]["crops"]):
            p_keep = fx[name]["samples"][b].get("crop_proportion")
            for s, side in enumerate(("src", "ref")):
                if "dir_" + side in crop:
                    clouds.append(fx["clouds"][b])
                    dirs.append(crop["dir_" + side])
                    ps.append(p_keep[s])
                    want.append(crop["kept_" + side])
                    who.append((name, b, side))
    assert len(clouds) == 4 * (2 + 2 + 1 + 2)
    before = dict(MP.CALLS)
    got = MP.crop_batch(clouds, np.stack(dirs), ps)
    assert MP.CALLS["crop"] == before["crop"] + 1 and MP.CALLS["read_back"] == before["read_back"] + 1
    for g, w, name in zip(got, want, who):
        assert g.dtype == torch.int32 and g.is_cuda
        assert np.array_equal(_np(g), w), name
    tie = who.index(("crop_test", 3, "src"))
    lo, _ = MP.percentile_index(2048, 0.7)
    assert len(got[tie]) == 2048 - lo - 2 and len(got[who.index(("crop_test", 0, "src"))]) == 2048 - lo - 1
    # p_keep None keeps the cloud whole
    whole = MP.crop_batch([fx["clouds"][0][:100, :3]], np.zeros((1, 3)), None)
    assert np.array_equal(_np(whole[0]), np.arange(100))


def _raw_crop(cuda, clouds, modes, dirs, los, gammas, max_rows=None, off=None, n_total=None):
    """pcrcg_modelnet_crop as it is exported -> (rc, kept stack, counts); the outputs start as -7 everywhere."""
    ld = clouds[0].shape[1]
    stack = torch.from_numpy(np.concatenate(clouds).astype(np.float32)).to(cuda)
    ns = [len(c) for c in clouds]
    if off is None:
        off = np.cumsum([0] + ns)
    C = len(off) - 1
    d_off = torch.tensor(np.asarray(off), dtype=torch.int32, device=cuda)
    d_mode = torch.tensor(modes, dtype=torch.int32, device=cuda)
    d_lo = torch.tensor(los, dtype=torch.int32, device=cuda)
    d_dir = torch.tensor(np.asarray(dirs, dtype=np.float64).reshape(C, 3), dtype=torch.float64, device=cuda)
    d_gamma = torch.tensor(gammas, dtype=torch.float64, device=cuda)
    kept = torch.full((stack.shape[0],), -7, dtype=torch.int32, device=cuda)
    count = torch.full((C,), -7, dtype=torch.int32, device=cuda)
    rc = _lib.lib().pcrcg_modelnet_crop(stack.data_ptr(), ld, stack.shape[0] if n_total is None else n_total, d_off.data_ptr(), C,
                                        max(ns) if max_rows is None else max_rows, d_mode.data_ptr(), d_dir.data_ptr(),
                                        d_lo.data_ptr(), d_gamma.data_ptr(), kept.data_ptr(), count.data_ptr(),
                                        torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc, kept.cpu().numpy(), count.cpu().numpy()


def _cloud(rng, n, ld):
    return (rng.rand(n, ld) * 2 - 1).astype(np.float32)


def _direction(rng):
    d = rng.randn(3)
    return d / np.linalg.norm(d)


def _check_call(cuda, clouds, modes, dirs, los, gammas, singles=True):
    """One call over `clouds` against the contract's restatement, and each cloud's own call bit for bit."""
    rc, kept, count = _raw_crop(cuda, clouds, modes, dirs, los, gammas)
    assert rc == 0, _lib.lib().pcrcg_last_error()
    off = np.cumsum([0] + [len(c) for c in clouds])
    for c, cloud in enumerate(clouds):
        want = PR.crop_contract(cloud, dirs[c], modes[c], los[c], gammas[c])
        assert count[c] == len(want), (c, len(cloud), modes[c], count[c], len(want))
        assert np.array_equal(kept[off[c]:off[c] + count[c]], want), (c, len(cloud), modes[c])
        assert np.all(kept[off[c] + count[c]:off[c + 1]] == -7)           # rows past the count are not written
        if singles:
            rc1, k1, c1 = _raw_crop(cuda, [cloud], [modes[c]], [dirs[c]], [los[c]], [gammas[c]])
            assert rc1 == 0 and c1[0] == count[c] and np.array_equal(k1[:c1[0]], kept[off[c]:off[c] + count[c]]), c
    return kept, count


@pytest.mark.parametrize("ld", [3, 6])
def test_crop_entry_sizes_and_modes(cuda, ld):
    """n = 1 (keeps nothing), 2, 3, 63, 64, 65, 2047 and a cloud at capacity, the three modes mixed in one call, gamma 0,
    gamma on both sides of 0.5, lo = n - 1 (the threshold is the largest distance: nothing is kept)."""
    rng = np.random.RandomState(11 + ld)
    sizes = [1, 2, 3, 63, 64, 65, 2047, CAP, 64, 65, 500, 2, 1]
    modes = [2, 2, 2, 2, 2, 2, 2, 2, 1, 0, 2, 1, 1]
    clouds = [_cloud(rng, n, ld) for n in sizes]
    dirs = [_direction(rng) for _ in sizes]
    los, gammas = [], []
    for n in sizes:
        lo, g = MP.percentile_index(n, 0.7)
        los.append(lo)
        gammas.append(g)
    gammas[3], gammas[4] = 0.0, 0.75                # gamma 0; the second lerp form
    los[5], los[10] = 64, 499                       # lo = n - 1
    kept, count = _check_call(cuda, clouds, modes, dirs, los, gammas)
    assert count[0] == 0 and count[5] == 0 and count[10] == 0 and count[9] == 65 and count[12] in (0, 1)
    assert count[7] == CAP - los[7] - 1


def test_crop_entry_capacity(cuda):
    """A cloud of capacity + 1 rows: an error code, nothing launched, nothing written."""
    rng = np.random.RandomState(3)
    cloud = _cloud(rng, CAP + 1, 3)
    rc, kept, count = _raw_crop(cuda, [cloud], [2], [_direction(rng)], [10], [0.5])
    assert rc == -1 and str(CAP + 1).encode() in _lib.lib().pcrcg_last_error()
    assert np.all(kept == -7) and np.all(count == -7)
    # the statement of the longest cloud is what sizes the launch: a longer cloud than stated is rejected by the kernel
    rc, kept, count = _raw_crop(cuda, [cloud[:100], cloud[:50]], [2, 2], [_direction(rng)] * 2, [10, 10], [0.5, 0.5], max_rows=64)
    assert rc == 0 and count[0] == -1 and count[1] == 50 - 10 - 1 and np.all(kept[:100] == -7)
    with pytest.raises(ValueError, match="cloud 1 has 8193 rows"):
        MP.crop_batch([cloud[:10], cloud], np.zeros((2, 3)), 0.7)


def test_crop_entry_ragged_batch(cuda):
    """C = 1 and C = 300 ragged clouds in one call, each equal bit for bit to its own single-cloud call."""
    rng = np.random.RandomState(4)
    sizes = rng.randint(1, 400, 300).tolist()
    clouds = [_cloud(rng, n, 6) for n in sizes]
    modes = rng.randint(0, 3, 300).tolist()
    dirs = [_direction(rng) for _ in sizes]
    ps = rng.choice([0.7, 0.3, 0.9], 300)
    los, gammas = zip(*[MP.percentile_index(n, p) for n, p in zip(sizes, ps)])
    _check_call(cuda, clouds, modes, dirs, list(los), list(gammas))
    _check_call(cuda, clouds[:1], modes[:1], dirs[:1], list(los[:1]), list(gammas[:1]))


def test_crop_entry_bad_clouds(cuda):
    """A NaN cloud and an infinite one among good ones get -1 and leave their neighbours untouched; an offsets pair that
    does not describe a range inside the stack reads as an empty cloud."""
    rng = np.random.RandomState(5)
    clouds = [_cloud(rng, n, 3) for n in (100, 1500, 70, 64)]
    clouds[1][1499, 2] = np.nan
    clouds[2][0, 0] = np.inf
    dirs = [_direction(rng) for _ in clouds]
    los, gammas = zip(*[MP.percentile_index(len(c), 0.7) for c in clouds])
    for modes in ([2, 2, 2, 2], [1, 0, 1, 0]):
        rc, kept, count = _raw_crop(cuda, clouds, modes, dirs, list(los), list(gammas))
        assert rc == 0 and count[1] == -1 and count[2] == -1
        assert np.all(kept[100:1670] == -7)
        for c, o in ((0, 0), (3, 1670)):
            want = PR.crop_contract(clouds[c], dirs[c], modes[c], los[c], gammas[c])
            assert count[c] == len(want) and np.array_equal(kept[o:o + count[c]], want)
    with pytest.raises(ValueError, match="cloud 1 was rejected"):
        MP.crop_batch(clouds, np.stack(dirs), 0.7)
    # offsets: (0, 10) good | (10, 50) past the 40 rows | (50, 25) descending | (25, 40) good
    stack = _cloud(rng, 40, 3)
    rc, kept, count = _raw_crop(cuda, [stack], [1, 1, 1, 1], [dirs[0]] * 4, [0] * 4, [0.0] * 4, max_rows=40, off=[0, 10, 50, 25, 40])
    assert rc == 0 and count[1] == 0 and count[2] == 0
    for c, (a, b) in ((0, (0, 10)), (3, (25, 40))):
        want = PR.crop_contract(stack[a:b], dirs[0], 1)
        assert count[c] == len(want) and np.array_equal(kept[a:a + count[c]], want)
    assert np.all(kept[10:25] == -7)
    rc, kept, count = _raw_crop(cuda, [stack], [1], [dirs[0]], [0], [0.0], max_rows=40, off=[-1, 40])
    assert rc == 0 and count[0] == 0 and np.all(kept == -7)


def _check_samples(fx, name, got, pairs, steps, rng):
    """transform_pairs' dicts for the fixture's pairs `pairs` of chain `name` against the recorded run and the bound."""
    for s, b in zip(got, pairs):
        want, crop = fx[name]["samples"][b], fx[name]["crops"][b]
        d = MP.draws(2048, b, steps, rng, kept_counts=crop["kept_counts"])
        _, trace = PR.run_chain(fx["clouds"][b], b, steps, d)
        assert set(s) == set(want) - {"label"} | ({"label"} if "label" in s else set()), (name, b)
        for k in ("points_raw", "points_src", "points_ref"):
            assert s[k].is_cuda and s[k].dtype == torch.float32 and tuple(s[k].shape) == want[k].shape, (name, b, k)
        assert s["transform_gt"].dtype == np.float32 and np.array_equal(_bits(s["transform_gt"]), _bits(want["transform_gt"]))
        assert s["idx"].dtype == np.int32 and int(s["idx"]) == b
        assert s.get("deterministic") == want.get("deterministic")
        if "crop_proportion" in want:
            assert s["crop_proportion"].dtype == np.float32 and np.array_equal(s["crop_proportion"], want["crop_proportion"])
        raw, src, ref = (_np(s[k]) for k in ("points_raw", "points_src", "points_ref"))
        assert np.array_equal(_bits(raw), _bits(want["points_raw"])), (name, b)
        rows = fx["clouds"][b][trace["rows_src"]]
        exact, bound = PR.transform_bound(rows, d["transform"], trace["noise_src"])
        err = np.abs(src[:, :3] - exact)
        print(name, b, "points_src: worst error / bound", float(np.max(err / bound)))
        assert np.all(err <= bound), (name, b)
        exact, bound = PR.normal_bound(rows, d["transform"])
        assert np.all(np.abs(src[:, 3:] - exact) <= bound), (name, b)
        rows = fx["clouds"][b][trace["rows_ref"]]
        assert np.array_equal(_bits(ref[:, 3:]), _bits(rows[:, 3:])), (name, b)            # the reference side's rows: exact
        if trace["noise_ref"] is None:
            assert np.array_equal(_bits(ref), _bits(want["points_ref"])), (name, b)
        else:
            exact, bound = PR.transform_bound(rows, None, trace["noise_ref"])
            assert np.all(np.abs(ref[:, :3] - exact) <= bound), (name, b)
            # f32(f64(x) + noise) has one correctly rounded value: the reference's
            assert np.array_equal(_bits(ref), _bits(want["points_ref"])), (name, b)


@pytest.mark.parametrize("name", MAIN + EXTRA)
def test_transform_pairs_against_the_reference(fx, name):
    """The four pairs of every recorded chain in one call: row counts, transform_gt, crop_proportion and every index-derived
    array exact, moved coordinates within the derived bound, one crop call, one read-back, one assemble call."""
    steps = steps_of(fx, name)
    seed = 1234 if name.endswith("train") else 99
    before = dict(MP.CALLS)
    got = MP.transform_pairs(fx["clouds"], range(4), steps, np.random.RandomState(seed), labels=fx["labels"])
    assert {k: MP.CALLS[k] - before[k] for k in before} == {"crop": 1, "assemble": 1, "read_back": 1}
    assert [int(s["label"]) for s in got] == fx["labels"].tolist()
    _check_samples(fx, name, got, range(4), steps, np.random.RandomState(seed))
    if name == "crop_test":
        # three columns in, three columns out, the same xyz
        xyz = MP.transform_pairs(fx["clouds"][:, :, :3], range(4), steps, np.random.RandomState(seed))
        for a, b in zip(xyz, got):
            for k in ("points_raw", "points_src", "points_ref"):
                assert a[k].shape[1] == 3 and torch.equal(a[k].view(torch.int32), b[k][:, :3].contiguous().view(torch.int32)), k


def test_counts_the_percentile_rule_does_not_predict(fx):
    """A train chain (one generator consumed pair after pair) with p_keep = 0.5, whose kept counts only the data knows:
    the batch redraws what it had drawn ahead and crops the later pairs again, so that it equals the pairs run one after
    another -- bit for bit, generator state included."""
    steps = MP.get_transforms("crop", partial_p_keep=[0.5, 0.5])[0]
    a, b = np.random.RandomState(7), np.random.RandomState(7)
    before = dict(MP.CALLS)
    batch = MP.transform_pairs(fx["clouds"][:3], [0, 1, 2], steps, a)
    assert MP.CALLS["crop"] - before["crop"] >= 2 and MP.CALLS["assemble"] - before["assemble"] == 1
    ones = [MP.transform_pairs(fx["clouds"][i:i + 1], [i], steps, b)[0] for i in range(3)]
    assert np.array_equal(a.get_state()[1], b.get_state()[1])
    for x, y in zip(batch, ones):
        assert np.array_equal(_bits(x["transform_gt"]), _bits(y["transform_gt"]))
        for k in ("points_src", "points_ref"):
            assert x[k].shape == y[k].shape == (717, 6) and torch.equal(x[k].view(torch.int32), y[k].view(torch.int32)), k
    # and each pair is the restatement's under the same draws
    rng = np.random.RandomState(7)
    for i, s in enumerate(batch):
        probe = np.random.RandomState()
        probe.set_state(rng.get_state())
        ahead = MP.draws(2048, i, steps, probe)
        counts = [len(PR.crop_contract(fx["clouds"][i], ahead["dir_" + side], 1)) for side in ("src", "ref")]
        d = MP.draws(2048, i, steps, rng, kept_counts=counts)
        want, trace = PR.run_chain(fx["clouds"][i], i, steps, d)
        assert np.array_equal(_bits(_np(s["points_ref"])), _bits(want["points_ref"])), i
        exact, bound = PR.transform_bound(fx["clouds"][i][trace["rows_src"]], d["transform"], trace["noise_src"])
        assert np.all(np.abs(_np(s["points_src"])[:, :3] - exact) <= bound), i


def test_transform_pairs_rejects_bad_clouds(fx):
    steps = steps_of(fx, "crop_test")
    bad = fx["clouds"][:2].copy()
    bad[1, 2047, 1] = np.nan
    with pytest.raises(ValueError, match="cloud 1 .idx 5. was rejected"):
        MP.transform_pairs(bad, [4, 5], steps, np.random.RandomState(0))
    with pytest.raises(ValueError, match="cloud 1 .idx 5. was rejected"):
        MP.transform_pairs(bad, [4, 5], steps_of(fx, "clean_test"), np.random.RandomState(0))     # no crop step: still checked
    flat = np.zeros((1, 16, 3), np.float32)                 # every distance 0: dist > 0 keeps nothing
    with pytest.raises(ValueError, match="keeps no row of the source"):
        MP.transform_pairs(flat, [0], MP.get_transforms("crop", partial_p_keep=[0.5, 0.5])[1], np.random.RandomState(0))


def _unbatch(sample):
    """prepare_pairs' sample (a leading dimension of one on every array) -> transform_pairs' form."""
    out = {}
    for k, v in sample.items():
        if k in ("deterministic", "label", "idx"):
            out[k] = v
        else:
            out[k] = v[0] if k.startswith("points_") else v[0].numpy()
    return out


def _same_item(a, b):
    assert set(a) == set(b)
    for k in a:
        if k == "sample":
            assert set(a[k]) == set(b[k])
            for kk in a[k]:
                x, y = _np(a[k][kk]), _np(b[k][kk])
                assert x.shape == y.shape and np.array_equal(_bits(x) if x.dtype.kind == "f" else x, _bits(y) if y.dtype.kind == "f" else y), kk
        elif isinstance(a[k], int):
            assert a[k] == b[k], k
        else:
            x, y = _np(a[k]), _np(b[k])
            assert x.dtype == y.dtype and x.shape == y.shape and np.array_equal(_bits(x) if x.dtype.kind == "f" else x,
                                                                                _bits(y) if y.dtype.kind == "f" else y), k


def test_prepare_pairs(fx, cuda):
    """B = 3 on the `crop` test chain: keys, dtypes, devices; correspondences pair by pair; a pair does not depend on the
    others of its call; the train chain under RandomState(1234) is the fixture's train run."""
    from pcrcg_amd.correspondences import get_correspondences
    cfg = modelnet_config()
    items = MP.prepare_pairs(fx["clouds"][:3], fx["labels"][:3], [0, 1, 2], cfg)
    assert len(items) == 3
    steps = steps_of(fx, "crop_test")
    _check_samples(fx, "crop_test", [_unbatch(it["sample"]) for it in items], range(3), steps, np.random.RandomState(0))
    for b, it in enumerate(items):
        assert set(it) == {"src_pcd", "tgt_pcd", "src_feats", "tgt_feats", "rot", "trans", "correspondences", "sample",
                           "n_correspondences"}
        want = fx["crop_test"]["samples"][b]
        for k, n in (("src_pcd", 717), ("tgt_pcd", 717)):
            assert it[k].is_cuda and it[k].dtype == torch.float32 and tuple(it[k].shape) == (n, 3) and it[k].is_contiguous()
        for k in ("src_feats", "tgt_feats"):
            assert it[k].is_cuda and it[k].dtype == torch.float32 and tuple(it[k].shape) == (717, 1) and bool((it[k] == 1).all())
        assert it["rot"].dtype == np.float32 and np.array_equal(it["rot"], want["transform_gt"][:, :3])
        assert it["trans"].dtype == np.float32 and it["trans"].shape == (3, 1) and np.array_equal(it["trans"][:, 0], want["transform_gt"][:, 3])
        assert torch.equal(it["src_pcd"], it["sample"]["points_src"][0, :, :3]) and torch.equal(it["tgt_pcd"], it["sample"]["points_ref"][0, :, :3])
        for k in ("points_raw", "points_src", "points_ref"):
            assert it["sample"][k].is_cuda and it["sample"][k].dim() == 3 and it["sample"][k].shape[0] == 1
        assert tuple(it["sample"]["transform_gt"].shape) == (1, 3, 4) and tuple(it["sample"]["crop_proportion"].shape) == (1, 2)
        assert it["sample"]["deterministic"] is True and int(it["sample"]["idx"]) == b and int(it["sample"]["label"]) == int(fx["labels"][b])
        tsfm = np.eye(4)
        tsfm[:3] = want["transform_gt"]
        corr = get_correspondences(it["src_pcd"], it["tgt_pcd"], tsfm, cfg.overlap_radius)
        assert it["correspondences"].dtype == torch.int64 and it["correspondences"].is_cuda
        assert torch.equal(it["correspondences"], corr) and it["n_correspondences"] == corr.shape[0] > 100
    # in_feats_dim = 3: the features are the coordinates
    three = MP.prepare_pair(fx["clouds"][1], None, 1, modelnet_config(in_feats_dim=3))
    assert torch.equal(three["src_feats"], three["src_pcd"]) and torch.equal(three["src_pcd"], items[1]["src_pcd"])
    assert "label" not in three["sample"]
    # a pair alone is the pair inside the batch, bit for bit
    alone = MP.prepare_pairs(fx["clouds"][2:3], fx["labels"][2:3], [2], cfg)[0]
    _same_item(alone, items[2])
    # train: numbers of the fixture's run under np.random.seed(1234)
    train = MP.prepare_pairs(fx["clouds"][:3], fx["labels"][:3], [0, 1, 2], cfg, subset="train", rng=np.random.RandomState(1234))
    _check_samples(fx, "crop_train", [_unbatch(it["sample"]) for it in train], range(3), steps_of(fx, "crop_train"),
                   np.random.RandomState(1234))
    assert "deterministic" not in train[0]["sample"]


def test_prepared_pairs_feed_the_network_and_the_evaluation(fx, cuda):
    """One dict through collate_fn_descriptor and a KPFCNN(modelnet_config()) forward; the dicts as records through
    tester.evaluate_modelnet_records with descriptors that agree across the ground-truth transform."""
    from pcrcg_amd import tester
    from pcrcg_amd.architectures import KPFCNN
    from pcrcg_amd.pyramid import collate_fn_descriptor
    cfg = modelnet_config()
    items = MP.prepare_pairs(fx["clouds"][:3], fx["labels"][:3], [0, 1, 2], cfg)
    torch.manual_seed(0)
    net = KPFCNN(cfg).to(cuda).eval()
    batch = collate_fn_descriptor([items[0]], cfg, [24, 30, 32])
    with torch.no_grad():
        out = net(batch)
    n = items[0]["src_pcd"].shape[0] + items[0]["tgt_pcd"].shape[0]
    assert tuple(out["feats_f"].shape) == (n, cfg.final_feats_dim)
    for k in ("feats_f", "scores_overlap", "scores_saliency"):
        assert bool(torch.isfinite(out[k]).all()), k
    assert batch["sample"] is items[0]["sample"]

    freq = np.random.RandomState(8).randn(3, 16) * 6.0

    def descriptors(p):          # a smooth function of the position in the reference frame: close points, close descriptors
        ph = p.astype(np.float64) @ freq
        f = np.concatenate([np.sin(ph), np.cos(ph)], 1)
        return (f / np.linalg.norm(f, axis=1, keepdims=True)).astype(np.float32)

    records = []
    for it in items:
        src, tgt = _np(it["src_pcd"]), _np(it["tgt_pcd"])
        moved = src @ it["rot"].T + it["trans"][:, 0]
        pcd = np.concatenate([src, tgt])
        records.append({"pcd": torch.from_numpy(pcd), "feats": torch.from_numpy(np.concatenate([descriptors(moved), descriptors(tgt)])),
                        "overlaps": torch.ones(len(pcd), 1), "saliency": torch.ones(len(pcd), 1), "len_src": len(src),
                        "rot": torch.from_numpy(it["rot"]), "trans": torch.from_numpy(it["trans"]), "sample": it["sample"]})
    np.random.seed(3)
    poses, metrics, summary = tester.evaluate_modelnet_records(records, seeds=1)
    assert len(poses) == 3
    assert set(summary) == {"r_rmse", "r_mae", "t_rmse", "t_mae", "err_r_deg_mean", "err_r_deg_rmse", "err_t_mean", "err_t_rmse",
                            "chamfer_dist", "rotation_mean", "rotation_max"}
    assert all(np.isfinite(v) for v in summary.values())
    assert 0 < summary["rotation_max"] <= 45.0 * 3
