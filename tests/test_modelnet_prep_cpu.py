"""CPU: the host side of ModelNet pair preparation (pcrcg_amd/modelnet_prep.py) -- the step lists, numpy's percentile rule,
the resample sizes, and above all the draws: the numpy restatement tests/modelnet_prep_ref.py fed with `draws` reproduces
every array the unmodified reference returned for the six chains (tests/golden/modelnet_prep.npz) bit for bit, which pins
the order of the draws and the reseeding."""
import os

import numpy as np
import pytest

from pcrcg_amd import _lib, modelnet_config
from pcrcg_amd import modelnet_prep as MP

from . import modelnet_prep_ref as PR

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "modelnet_prep.npz")
MAIN = [f"{noise}_{form}" for noise in ("clean", "jitter", "crop") for form in ("train", "test")]
EXTRA = ["crop_p07", "crop_p0505", "crop_p11"]


@pytest.fixture(scope="module")
def fx():
    return PR.load_fixture(GOLDEN)


def steps_of(fx, name):
    noise, form = name.split("_")[:2]
    chain = fx[name]
    train, test = MP.get_transforms(noise, num_points=chain["num_points"], partial_p_keep=chain["partial"])
    return train if form == "train" else test


def _bits(x):
    x = np.ascontiguousarray(x)
    return x.view({4: np.uint32, 8: np.uint64}[x.dtype.itemsize]) if x.dtype.kind == "f" else x


@pytest.mark.parametrize("name", MAIN + EXTRA)
def test_step_lists_are_the_references(fx, name):
    assert [s for s, _ in steps_of(fx, name)] == fx[name]["steps"]


def test_get_transforms_defaults_and_unknown_noise():
    train, test = MP.get_transforms("crop")
    assert dict(train)["RandomCrop"] == {"p_keep": [0.7, 0.7]} and dict(train)["Resampler"] == {"num": 1024}
    assert dict(train)["RandomTransformSE3_euler"] == {"rot_mag": 45.0, "trans_mag": 0.5}
    assert test[0] == ("SetDeterministic", {}) and test[1:] == train
    assert dict(MP.get_transforms("clean")[1])["FixedResampler"] == {"num": 1024}
    with pytest.raises(NotImplementedError):
        MP.get_transforms("outlier")


def test_percentile_index_is_numpys_rule():
    """For every n in 1..100 and four proportions: the lerp of the two order statistics percentile_index names is
    np.percentile's value, bit for bit, and so is the mask."""
    rng = np.random.RandomState(5)
    for n in range(1, 101):
        x = rng.randn(n)
        s = np.sort(x)
        for p in (0.7, 0.5001, 0.3, 1 / 3):
            p32 = np.float32(p)
            want = np.percentile(x, (1.0 - p32) * 100)
            lo, g = MP.percentile_index(n, p)
            assert 0 <= lo <= n - 1 and 0.0 <= g < 1.0
            if lo + 1 == n:
                thr = s[lo]
            else:
                a, b = s[lo], s[lo + 1]
                thr = b - (b - a) * (1.0 - g) if g >= 0.5 else a + (b - a) * g
            assert _bits(np.float64(thr)) == _bits(np.float64(want)), (n, p)
            assert np.array_equal(x > thr, x > want)
    assert MP.percentile_index(10, 1.0) == (0, 0.0)          # a side kept "whole" next to a cropped one: dist > min
    assert MP.percentile_index(1, 0.7)[0] == 0
    with pytest.raises(ValueError):
        MP.percentile_index(0, 0.7)
    with pytest.raises(ValueError):
        MP.percentile_index(10, 1.5)


def test_the_two_draw_identities():
    pts = np.random.RandomState(0).rand(50, 6)
    a, b = np.random.RandomState(9), np.random.RandomState(9)
    assert np.array_equal(a.permutation(pts), pts[b.permutation(50)])
    assert np.array_equal(a.get_state()[1], b.get_state()[1])
    for n, k in ((50, 50), (50, 17), (1434, 717), (3, 1)):
        assert np.array_equal(a.choice(n, k, replace=False), b.permutation(n)[:k])
        assert np.array_equal(a.get_state()[1], b.get_state()[1])


def test_resample_sizes():
    assert MP.resample_sizes(1024) == (1024, 1024)
    for num in (1024, 256, 2048, 10):
        assert MP.resample_sizes(num, [0.7, 0.7]) == (717, 717)
        assert MP.resample_sizes(num, np.array([0.5, 1.0], dtype=np.float32)) == (717, 717)
    assert MP.resample_sizes(1024, [0.7]) == (717, 1024)
    assert MP.resample_sizes(256, np.array([0.7], dtype=np.float32)) == (180, 256)
    assert MP.resample_sizes(1000, [0.5]) == (500, 1000)
    with pytest.raises(ValueError):
        MP.resample_sizes(1024, [0.7, 0.7, 0.7])


@pytest.mark.parametrize("name", MAIN + EXTRA)
def test_restatement_under_draws_is_the_reference_bit_for_bit(fx, name):
    """draws + the restatement = the reference's run: every sample key of every pair, transform_gt included.  Train chains
    consume one RandomState(1234) pair after pair, as the fixture's run consumed numpy's global generator."""
    steps = steps_of(fx, name)
    rng = np.random.RandomState(1234 if name.endswith("train") else 99)
    for b in range(4):
        want, crop = fx[name]["samples"][b], fx[name]["crops"][b]
        d = MP.draws(2048, b, steps, rng, kept_counts=crop["kept_counts"])
        got, trace = PR.run_chain(fx["clouds"][b], b, steps, d, label=fx["labels"][b])
        assert set(got) == set(want), (b, set(got) ^ set(want))
        for k, v in want.items():
            g = np.asarray(got[k])
            assert g.dtype == v.dtype and g.shape == v.shape, (b, k, g.dtype, v.dtype, g.shape, v.shape)
            assert np.array_equal(_bits(g), _bits(v)), (b, k)
        for side in ("src", "ref"):
            if "dir_" + side in crop:
                assert np.array_equal(_bits(d["dir_" + side]), _bits(crop["dir_" + side]))
                assert np.array_equal(trace["kept_" + side], crop["kept_" + side])
                # the contract's arithmetic (sequential float32 centroid, unfused float64 distances) gives the same mask
                p = d["crop_proportion"][0 if side == "src" else 1]
                lo, g = MP.percentile_index(2048, p)
                mode = 1 if p == 0.5 else 2
                assert np.array_equal(PR.crop_contract(fx["clouds"][b], d["dir_" + side], mode, lo, g), crop["kept_" + side])
        assert tuple(d["kept_counts"]) == tuple(crop["kept_counts"])
        # what transform_pairs composes from the draws points at the same input rows
        plan = MP.compose(steps, d)
        for side in ("src", "ref"):
            kept = trace["kept_" + side] if trace["kept_" + side] is not None else np.arange(2048)
            pick = plan["pick_" + side] if plan["pick_" + side] is not None else np.arange(len(kept))
            assert np.array_equal(kept[pick], trace["rows_" + side])
            if trace["noise_" + side] is None:
                assert plan["noise_" + side] is None
            else:
                assert np.array_equal(plan["noise_" + side], trace["noise_" + side])
        base = plan["base"] if plan["base"] is not None else np.arange(2048)
        assert np.array_equal(base, trace["rows_raw"])


def test_the_fixture_holds_a_tie_on_a_bracket_and_clear_gaps_elsewhere(fx):
    gaps = [(name, b, side, float(c["gap_" + side])) for name in MAIN + EXTRA for b, c in enumerate(fx[name]["crops"])
            for side in ("src", "ref") if "gap_" + side in c]
    assert len(gaps) >= 4 * 2 * 2
    assert all(g > 1e-9 or (g == 0.0 and b == 3) for _, b, _, g in gaps)
    assert ("crop_test", 3, "src", 0.0) in gaps
    # the duplicated cloud: the prediction n - lo - 1 counts one row too many, the tie takes both copies
    lo, _ = MP.percentile_index(2048, 0.7)
    assert fx["crop_test"]["crops"][3]["kept_counts"][0] == 2048 - lo - 2
    assert fx["crop_test"]["crops"][0]["kept_counts"][0] == 2048 - lo - 1


def test_predicted_draws_equal_the_true_ones_where_no_tie(fx):
    steps = steps_of(fx, "crop_train")
    a, b = np.random.RandomState(1234), np.random.RandomState(1234)
    for i in range(3):
        ahead = MP.draws(2048, i, steps, a)
        true = MP.draws(2048, i, steps, b, kept_counts=fx["crop_train"]["crops"][i]["kept_counts"])
        assert ahead["predicted"] and not true["predicted"] and ahead["kept_counts"] == true["kept_counts"]
        for k in ("resample_src", "resample_ref", "noise_src", "perm_ref", "perm_src", "transform"):
            assert np.array_equal(ahead[k], true[k]), k


def test_error_paths_that_need_no_device():
    steps = MP.get_transforms("crop")[1]
    rng = np.random.RandomState(0)
    with pytest.raises(ValueError, match="keeps no row"):
        MP.draws(1, 0, steps, rng)                                  # one row: dist > dist keeps nothing
    with pytest.raises(ValueError, match="keeps no row of the reference"):
        MP.draws(2048, 7, steps, rng, kept_counts=(5, 0))
    with pytest.raises(ValueError, match="cloud 1 is empty"):
        MP.transform_pairs([np.zeros((4, 3), np.float32), np.zeros((0, 3), np.float32)], [0, 1], steps, rng)
    with pytest.raises(ValueError, match="cloud 0 has 8193 rows"):
        MP.transform_pairs([np.zeros((8193, 6), np.float32)], [0], steps, rng)
    with pytest.raises(ValueError, match="cloud 0 must be"):
        MP.crop_batch([np.zeros((8, 4), np.float32)], np.zeros((1, 3)), 0.7)
    with pytest.raises(ValueError, match="cloud 1 has 6 columns"):
        MP.crop_batch([np.zeros((8, 3), np.float32), np.zeros((8, 6), np.float32)], np.zeros((2, 3)), 0.7)
    with pytest.raises(ValueError, match="2 clouds, 1 idxs"):
        MP.transform_pairs(np.zeros((2, 8, 3), np.float32), [0], steps, rng)
    with pytest.raises(ValueError):
        MP.draws(8, 0, MP.get_transforms("crop", partial_p_keep=[0.7, 0.7, 0.7])[1], rng)
    with pytest.raises(NotImplementedError):
        MP.compose((("SplitSourceRef", {}), ("RandomJitter", {"scale": 0.01, "clip": 0.05}),
                    ("RandomTransformSE3_euler", {"rot_mag": 45.0, "trans_mag": 0.5})), {"noise_src": 0, "noise_ref": 0})


def test_config_and_abi():
    cfg = modelnet_config()
    assert (cfg.overlap_radius, cfg.partial, cfg.num_points, cfg.noise_type, cfg.rot_mag, cfg.trans_mag) == \
        (0.04, [0.7, 0.7], 1024, "crop", 45.0, 0.5)
    for name in ("pcrcg_modelnet_crop", "pcrcg_modelnet_assemble"):
        assert name in _lib.SIGNATURES and hasattr(_lib.lib(), name)
    assert MP.CROP_MAX_ROWS == 8192
    lib = _lib.lib()
    # nothing launches on a bad argument: over-capacity max_rows, a bad row width, null pointers
    import ctypes
    p = ctypes.c_void_p(4096)
    assert lib.pcrcg_modelnet_crop(p, 3, 10, p, 1, 8193, p, p, p, p, p, p, None) == -1
    assert b"8193" in lib.pcrcg_last_error()
    assert lib.pcrcg_modelnet_crop(p, 4, 10, p, 1, 10, p, p, p, p, p, p, None) == -1
    assert lib.pcrcg_modelnet_crop(None, 3, 10, p, 1, 10, p, p, p, p, p, p, None) == -1
    assert lib.pcrcg_modelnet_assemble(p, 5, 10, p, 1, None, None, p, p, p, None, 1, p, None, 4, p, None) == -1
    assert lib.pcrcg_modelnet_assemble(p, 3, 10, p, 1, p, None, p, p, p, None, 1, p, None, 4, p, None) == -1
