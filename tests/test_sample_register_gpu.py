"""GPU: the device sampler inside the evaluation path -- tester.register_records / evaluate_records with
sampler="device" against registration.register_batch on the rows tests/sample_ref.py picks, the untouched host
generator, the unchanged host path, and tester.register_outputs on network outputs that never leave the device."""
import numpy as np
import pytest
import torch

from pcrcg_amd import registration as REG
from pcrcg_amd import tester

from . import ransac_ref as RR
from . import sample_ref as SR

pytestmark = pytest.mark.gpu

N_POINTS = 400
KW = dict(distance_threshold=0.05, ransac_n=3)
SAMPLE_SEEDS = [5, 70001, (1 << 23) - 1]
SEEDS = [1, 2, 3]


def _record(seed, n_src=1500, n_tgt=1200):
    rng = np.random.RandomState(seed)
    src, tgt, f, g, _ = RR.registration_pair(200 + seed, n=max(n_src, n_tgt), outliers=0.3)
    n = n_src + n_tgt
    return {"pcd": torch.from_numpy(np.concatenate([src[:n_src], tgt[:n_tgt]])),
            "feats": torch.from_numpy(np.concatenate([f[:n_src], g[:n_tgt]])),
            "overlaps": torch.from_numpy(rng.rand(n, 1).astype(np.float32)),
            "saliency": torch.from_numpy(rng.rand(n, 1).astype(np.float32)),
            "len_src": n_src, "rot": torch.eye(3), "trans": torch.zeros(3, 1)}


@pytest.fixture(scope="module")
def records():
    return [_record(b) for b in range(3)]


def _reference_subsets(records, sample_seeds, n_points=N_POINTS):
    """The four lists register_batch takes, from the rows the specification keeps (numpy, on the host)."""
    lists = [[], [], [], []]
    for r, seed in zip(records, sample_seeds):
        ls = r["len_src"]
        sc = (r["overlaps"] * r["saliency"]).numpy().reshape(-1)
        pcd, feats = r["pcd"].numpy(), r["feats"].numpy()
        for side, (lo, hi) in enumerate(((0, ls), (ls, len(pcd)))):
            assert SR.relative_gap(sc[lo:hi], n_points, 2 * seed + side) > 1e-9
            idx = SR.sample(sc[lo:hi], n_points, 2 * seed + side)
            lists[side].append(pcd[lo:hi][idx])
            lists[2 + side].append(feats[lo:hi][idx])
    return lists


def test_device_sampler_registers_the_specified_rows(cuda, records):
    want = REG.register_batch(*_reference_subsets(records, SAMPLE_SEEDS), seeds=SEEDS, **KW)
    state = np.random.get_state()
    got = tester.register_records(records, n_points=N_POINTS, seeds=SEEDS, sampler="device", sample_seeds=SAMPLE_SEEDS, **KW)
    poses, inliers = tester.evaluate_records(records, n_points=N_POINTS, seeds=SEEDS, sampler="device",
                                             sample_seeds=SAMPLE_SEEDS, **KW)
    after = np.random.get_state()
    assert state[0] == after[0] and np.array_equal(state[1], after[1]) and state[2:] == after[2:]      # np.random untouched
    assert len(got) == 3
    for b in range(3):
        assert got[b].shape == (4, 4) and np.array_equal(got[b], want.matrices[b]), b
        assert np.array_equal(poses[b], want.matrices[b]), b
    assert list(inliers.n_points) == [N_POINTS] * 3


def test_one_seed_for_every_record_and_seed_checks(cuda, records):
    want = REG.register_batch(*_reference_subsets(records[:2], [9, 9]), seeds=0, **KW)
    got = tester.register_records(records[:2], n_points=N_POINTS, sampler="device", sample_seeds=9, **KW)
    assert all(np.array_equal(got[b], want.matrices[b]) for b in range(2))
    for bad in (dict(sample_seeds=1 << 23), dict(sample_seeds=[1, 2, 3]), dict(sampler="gpu")):
        with pytest.raises(ValueError):
            tester.register_records(records[:2], n_points=N_POINTS, **{"sampler": "device", **bad})


def test_host_sampler_is_unchanged(cuda, records):
    """sampler="host" (the default): the same draws from np.random and the same poses as the direct path."""
    np.random.seed(21)
    direct = REG.register_batch(*tester._sample_records(records, N_POINTS), seeds=SEEDS, **KW)
    end = np.random.get_state()
    for kw in ({}, {"sampler": "host", "sample_seeds": 12345}):
        np.random.seed(21)
        got = tester.register_records(records, n_points=N_POINTS, seeds=SEEDS, **KW, **kw)
        after = np.random.get_state()
        assert np.array_equal(end[1], after[1]) and end[2] == after[2]              # consumed exactly as before
        assert all(np.array_equal(got[b], direct.matrices[b]) for b in range(3))


def test_sampled_rows_come_back_on_the_device(cuda, records):
    r = records[0]
    ls = r["len_src"]
    sc = r["overlaps"] * r["saliency"]
    pts, fts = tester.probabilistic_sample_batch([r["pcd"][:ls].to(cuda), r["pcd"][ls:]], [r["feats"][:ls].to(cuda), r["feats"][ls:]],
                                                 [sc[:ls], sc[ls:].to(cuda)], 2000, [4, 5])
    idx = SR.sample(sc[:ls].numpy(), 2000, 4)
    assert pts[0].is_cuda and pts[0].shape == (1500, 3) and np.array_equal(pts[0].cpu().numpy(), r["pcd"][:ls].numpy())
    assert len(idx) == 1500 and pts[1].shape == (1200, 3) and fts[1].shape == (1200, r["feats"].shape[1])
    pts, fts = tester.probabilistic_sample_batch([r["pcd"][ls:]], [r["feats"][ls:]], [sc[ls:]], 64, 77)
    idx = SR.sample(sc[ls:].numpy(), 64, 77)
    assert np.array_equal(pts[0].cpu().numpy(), r["pcd"][ls:].numpy()[idx])
    assert np.array_equal(fts[0].cpu().numpy(), r["feats"][ls:].numpy()[idx])


def test_register_outputs_equals_the_record_path(cuda):
    """Two KPFCNN.forward results, kept on the device, against the same outputs taken to the host as records."""
    from pcrcg_amd import indoor_config, synthetic
    from pcrcg_amd.architectures import KPFCNN
    from pcrcg_amd.pyramid import build_pyramid
    cfg = indoor_config(first_feats_dim=32, gnn_feats_dim=64)
    torch.manual_seed(0)
    np.random.seed(0)
    net = KPFCNN(cfg).eval().to(cuda)
    outputs, points, lengths, recs = [], [], [], []
    for b in range(2):
        src, tgt = synthetic.pair("mini", b)
        pts = torch.from_numpy(np.concatenate([src, tgt])).to(cuda)
        lens = torch.tensor([len(src), len(tgt)], dtype=torch.int32, device=cuda)
        with torch.no_grad():
            out = net(build_pyramid(pts, lens, cfg, [20, 26, 30, 32]))
        out = {k: v for k, v in out.items() if k in ("feats_f", "scores_overlap", "scores_saliency")}
        if b == 1:                                     # as PairStreams.result(wait=False) hands it over
            out["done_event"] = torch.cuda.Event()
            out["done_event"].record()
        outputs.append(out)
        points.append(pts)
        lengths.append(len(src) if b == 0 else (len(src), len(tgt)))
        recs.append({"pcd": pts.cpu(), "feats": out["feats_f"].cpu(), "overlaps": out["scores_overlap"].cpu(),
                     "saliency": out["scores_saliency"].cpu(), "len_src": len(src)})
    kw = dict(n_points=N_POINTS, seeds=[3, 4], sample_seeds=[10, 11], **KW)
    want = tester.register_records(recs, sampler="device", **kw)
    state = np.random.get_state()
    before = REG.D2H_READS
    res = tester.register_outputs(outputs, points, lengths, **kw)
    assert REG.D2H_READS == before + 1                                       # the poses, nothing else
    assert np.array_equal(state[1], np.random.get_state()[1])
    assert len(res) == 2
    for b in range(2):
        assert np.array_equal(res.matrices[b], want[b]), b
    with pytest.raises(TypeError):
        tester.register_outputs(outputs, points, [torch.tensor([1500, 1500], device=cuda)] * 2, **kw)
    with pytest.raises(ValueError):
        tester.register_outputs(outputs, points[:1], lengths, **kw)
