"""CPU: grid subsampling with features and classes -- the numpy restatement (tests/subsample_ref.py) equals the unmodified
reference on every case of tests/golden/subsample_features.npz (scripts/make_golden_subsample_features.py), and the shim
and the C ABI refuse what they must before any device is touched."""
import ctypes
import os

import numpy as np
import pytest

from pcrcg_amd import _lib
from pcrcg_amd.cpp_wrappers.cpp_subsampling import grid_subsampling as G
from tests import subsample_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "subsample_features.npz")
CASES = {c["name"]: c for c in R.fixture_cases()}
P = ctypes.c_void_p(4096)        # "some pointer": a rejected call never dereferences it


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(GOLDEN))


def test_fixture_holds_every_case(golden):
    assert {k.split("/")[0] for k in golden} == set(CASES)
    assert os.path.getsize(GOLDEN) <= os.path.getsize(os.path.join(os.path.dirname(GOLDEN), "frontend_mini.npz"))
    for name, case in CASES.items():
        assert int(golden[name + "/checksum"][0]) == R.input_checksum(case), name   # the inputs are rebuilt, not stored


@pytest.mark.parametrize("name", sorted(CASES))
def test_restatement_equals_the_reference(golden, name):
    c = CASES[name]
    p, l, f, k = R.subsample_ref(c["points"], c["lengths"], c["dl"], c["max_p"], c["features"], c["classes"])
    assert np.array_equal(R.bits(p), R.bits(golden[name + "/points"]))
    assert np.array_equal(l, golden[name + "/lengths"])
    assert (f is None) == (name + "/features" not in golden) and (k is None) == (name + "/classes" not in golden)
    if f is not None:
        assert np.array_equal(R.bits(f), R.bits(golden[name + "/features"]))
    if k is not None:
        assert k.ndim == 2 and np.array_equal(k, golden[name + "/classes"])


def test_reference_facts_the_fixture_records(golden):
    """what is easy to get wrong: a tie goes by list order, not by label value; -0.0f alone becomes +0.0f; Inf stays"""
    assert golden["tie_5335/classes"].tolist() == [[3]] and golden["tie_3553/classes"].tolist() == [[5]]
    assert R.bits(golden["one_point/features"])[0, 0] == 0
    lone = np.flatnonzero((golden["cloud2000/points"] == 5.0).all(axis=1))
    assert len(lone) == 1 and (R.bits(golden["cloud2000/features"])[lone[0]] == 0).all()
    assert np.isposinf(golden["cloud2000/features"]).sum() == 1 and not np.isnan(golden["cloud2000/features"]).any()
    assert golden["cloud2000/points"].shape[0] > 256
    assert golden["three_clouds_cap10/lengths"].tolist() == [10, 10, 10]
    for k in ("points", "features", "classes"):       # the cap cuts all three at the same rows
        full, cut, lo = golden["three_clouds/" + k], golden["three_clouds_cap10/" + k], 0
        for b, m in enumerate(golden["three_clouds/lengths"]):
            assert np.array_equal(cut[10 * b:10 * b + 10].view(np.int32), full[lo:lo + 10].view(np.int32))
            lo += int(m)


def test_vote_crosses_the_bucket_stages():
    """the emulated unordered_map<int,int>: bucket counts 13 and 29 are left with the 14th and the 30th distinct label"""
    assert R.umap_order(list(range(13))) == list(range(12, -1, -1))
    assert R.umap_order(list(range(14)))[0] == 13 and sorted(R.umap_order(list(range(31)))) == list(range(31))
    assert R.vote([5, 3, 3, 5]) == 3 and R.vote([3, 5, 5, 3]) == 5
    # (size_t)-1 % 13 == 2: label -1 shares the bucket of label 2, which then sits in front of it and behind 7 (with a
    # signed hash the list would begin with 2)
    assert R.vote([-1, 7, 2]) == 7


PTS = np.zeros((4, 3), np.float32)


@pytest.mark.parametrize("kw, message", [
    (dict(features=np.zeros(4, np.float32)), "Wrong dimensions : features.shape is not (N, d)"),
    (dict(features=np.zeros((4, 2, 2), np.float32)), "Wrong dimensions : features.shape is not (N, d)"),
    (dict(features=np.zeros((3, 2), np.float32)), "Wrong dimensions : features.shape is not (N, d)"),
    (dict(classes=np.zeros((4, 1, 1), np.int32)), "Wrong dimensions : classes.shape is not (N,) or (N, d)"),
    (dict(classes=np.zeros(5, np.int32)), "Wrong dimensions : classes.shape is not (N,) or (N, d)"),
    (dict(classes=np.zeros((3, 2), np.int32)), "Wrong dimensions : classes.shape is not (N,) or (N, d)"),
    (dict(features=[["a", "b"]] * 4), "Error converting input features to numpy arrays of type float32"),
    (dict(classes=["x"] * 4), "Error converting input classes to numpy arrays of type int32"),
], ids=lambda v: None if isinstance(v, dict) else v.split(":")[-1].strip()[:24])
def test_shim_raises_the_reference_errors_without_a_device(kw, message):
    for call in (lambda: G.subsample_batch(PTS, np.array([4], np.int32), sampleDl=0.1, **kw),
                 lambda: G.subsample(PTS, sampleDl=0.1, **kw)):
        with pytest.raises(RuntimeError) as e:
            call()
        assert str(e.value) == message


def test_shim_refuses_wide_classes_on_several_clouds():
    with pytest.raises(RuntimeError, match="more than one column and more than one cloud"):
        G.subsample_batch(PTS, np.array([2, 2], np.int32), classes=np.zeros((4, 2), np.int32), sampleDl=0.1)


def _ex(**bad):
    a = dict(pts=P, n=10, len=P, nb=1, dl=0.1, feats=P, fdim=3, ld=3, classes=P, ldim=1, out_pts=P, out_len=P, out_m=P,
             out_feats=P, out_classes=P, ws=P)
    a.update(bad)
    return _lib.lib().pcrcg_grid_subsample_batch_ex(a["pts"], a["n"], a["len"], a["nb"], a["dl"], 0, a["feats"], a["fdim"], a["ld"],
                                                    a["classes"], a["ldim"], a["out_pts"], a["out_len"], a["out_m"],
                                                    a["out_feats"], a["out_classes"], a["ws"], 1 << 30, None)


@pytest.mark.parametrize("bad", [dict(pts=None), dict(len=None), dict(out_pts=None), dict(out_len=None), dict(out_m=None),
                                 dict(ws=None), dict(feats=None), dict(out_feats=None), dict(classes=None),
                                 dict(out_classes=None), dict(n=-1), dict(nb=0), dict(fdim=-1), dict(ldim=-1), dict(ld=2),
                                 dict(dl=0.0)], ids=lambda d: next(iter(d)))
def test_ex_entry_rejects_it_before_any_launch(bad):
    assert _ex(**bad) == -1 and b"bad argument" in _lib.lib().pcrcg_last_error()


def test_ex_workspace_query():
    lib = _lib.lib()
    ws = lib.pcrcg_grid_subsample_ex_ws_bytes
    base = lib.pcrcg_grid_subsample_ws_bytes(60000, 2)
    assert ws(60000, 2, 0, 0) == base                       # nothing asked for, nothing added
    # the features are summed straight into the output rows: they cost the row -> cell map and nothing per column
    assert base + 60000 * 4 <= ws(60000, 2, 3, 0) <= ws(60000, 2, 128, 0) < base + 60000 * 8
    assert ws(60000, 2, 0, 1) >= ws(60000, 2, 3, 0) + 6 * 60000 * 4
    assert ws(60000, 2, 0, 2) >= ws(60000, 2, 0, 1) + 6 * 60000 * 4
    assert ws(60000, 2, 32, 2) == ws(60000, 2, 0, 2)
    assert ws(-5, 2, -1, -1) == lib.pcrcg_grid_subsample_ws_bytes(0, 2)
