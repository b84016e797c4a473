"""GPU: the decoder's `nearest_upsample -> cat(skip) -> unary` with the unary's upsampled half applied to the COARSE rows and
the product's rows copied up (csrc/runner.hip), against the op-by-op mirror KPFCNN.forward_ops, which restates the reference's
order (upsample first); and the multi-cloud row copy it uses (gather_first_multi) against indexing on the host.

(a) the copy: 1-4 clouds, one of them with zero rows; nq in {1, 5, 257}, c in {1, 34, 257} with ld_out = pad4(c); first indices
    equal to ns, negative and beyond ns give zero rows; the result equals host indexing exactly and the padding columns of the
    output stay untouched.
(b) the runner against forward_ops at the 1e-5 bar tests/test_scale_gpu.py holds between the two, with 1 pair and 4 pairs per
    call: tests/golden/model_mini.pt; modelnet_mini.pt (two consecutive decoder unaries: the lazy hand-over is materialised);
    hand-made pyramids whose coarse levels have 65, 1 and 63 rows and whose up-sample tables' first columns hold shadow indices."""
import os

import pytest
import torch

from pcrcg_amd import indoor_config, modelnet_config, ops
from pcrcg_amd.architectures import KPFCNN
from tests.test_descriptor_forms_gpu import KEYS, _edited, _to, forward, rel

pytestmark = pytest.mark.gpu
SAME = 1e-5


def pad4(c):
    return (c + 3) & ~3


# ---- (a) the multi-cloud row copy -------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", [1, 34, 257])
@pytest.mark.parametrize("nq", [1, 5, 257])
@pytest.mark.parametrize("clouds", [1, 2, 3, 4])
def test_gather_first_multi_equals_host_indexing(cuda, clouds, nq, c):
    g = torch.Generator().manual_seed(1000 * clouds + 10 * nq + c)
    ld_x, ld_out = pad4(c), pad4(c)
    empty = clouds - 2                                  # the cloud without rows (none when there is only one cloud)
    xs, idxs, outs, wants = [], [], [], []
    for k in range(clouds):
        n = 0 if k == empty else nq + k
        ns = (1, 7, 64, 300)[k]
        xb = torch.randn(ns, ld_x, generator=g)         # rows of ld_x floats, as the runner's product leaves them
        x = xb[:, :c]
        idx = torch.randint(0, ns, (n, 3), generator=g)
        if n >= 1:
            idx[0, 0] = ns                              # the shadow index
        if n >= 3:
            idx[1, 0], idx[2, 0] = -1, ns + 5
        if n >= 5:
            idx[4, 0] = -(1 << 40)
        idx[:, 1:] = -3                                 # only the first column is read
        want = torch.zeros(n, c)
        real = (idx[:, 0] >= 0) & (idx[:, 0] < ns)
        want[real] = x[idx[real, 0]]
        xs.append(xb.to(cuda)[:, :c])
        idxs.append(idx.to(cuda))
        outs.append(torch.full((n, ld_out), float("nan"), device=cuda))
        wants.append(want)
    ops.gather_first_multi(xs, idxs, [o[:, :c] for o in outs])
    torch.cuda.synchronize()
    for k in range(clouds):
        got = outs[k].cpu()
        assert torch.equal(got[:, :c], wants[k]), (k, float((got[:, :c] - wants[k]).abs().max()))
        assert torch.isnan(got[:, c:]).all(), "padding columns written"


# ---- (b) the runner against the mirror ----------------------------------------------------------------------------------
def _check(net, batches, cuda):
    """One call per group size: the first pair alone, then every pair of `batches` in one call; each against its own mirror."""
    runner = net.runner()
    with torch.no_grad():
        once = {id(b): net.forward_ops(b) for b in {id(b): b for b in batches}.values()}
        refs = [once[id(b)] for b in batches]
    structs = [runner.batch_struct(b)[:2] for b in batches]
    desc = _edited(runner, [])
    for group in ([0], list(range(len(batches)))):
        got = forward(runner, desc, [structs[i][0] for i in group], cuda)
        for out, i in zip(got, group):
            for k in KEYS:
                assert torch.isfinite(out[k]).all(), (len(group), i, k)
                assert rel(out[k], refs[i][k]) <= SAME, (len(group), i, k, rel(out[k], refs[i][k]))
    del structs


def test_mini_runner_equals_mirror(cuda, golden_dir):
    gold = torch.load(os.path.join(golden_dir, "model_mini.pt"))
    col = torch.load(os.path.join(golden_dir, "collate_mini.pt"))
    net = KPFCNN(indoor_config(first_feats_dim=32, gnn_feats_dim=64))
    net.load_state_dict(gold["state_dict"], strict=True)
    net = net.to(cuda).eval()
    batch = {k: _to(v, cuda) for k, v in col["batch"].items()}
    _check(net, [batch] * 4, cuda)


def test_modelnet_mini_runner_equals_mirror(cuda, golden_dir):
    mm = torch.load(os.path.join(golden_dir, "modelnet_mini.pt"))
    net = KPFCNN(modelnet_config(first_feats_dim=32, gnn_feats_dim=64, final_feats_dim=32))
    net.load_state_dict(mm["state_dict"], strict=True)
    net = net.to(cuda).eval()
    batch = {k: _to(v, cuda) for k, v in mm["batch"].items()}
    _check(net, [batch] * 4, cuda)


def _hand_made(n0, seed, dev):
    """A four-level batch dict with levels of n0, 65, 1 and 63 rows (the decoder's products run on 63, 1 and 65 coarse rows):
    random points, random tables with shadow entries; every up-sample table's first column holds shadow indices."""
    g = torch.Generator().manual_seed(seed)
    n = [n0, 65, 1, 63]
    h_nb, h_pool, h_up = 9, 7, 5
    pts = [torch.rand(m, 3, generator=g) * 0.08 * 2 ** l for l, m in enumerate(n)]

    def table(rows, width, ns):
        t = torch.randint(0, ns, (rows, width), generator=g)
        t[torch.rand(rows, width, generator=g) < 0.2] = ns
        return t
    nb = [table(n[l], h_nb, n[l]) for l in range(4)]
    pools = [table(n[l + 1], h_pool, n[l]) for l in range(3)] + [torch.zeros(0, 1, dtype=torch.int64)]
    ups = [table(n[l], h_up, n[l + 1]) for l in range(3)] + [torch.zeros(0, 1, dtype=torch.int64)]
    for l in range(3):
        ups[l][0, 0] = n[l + 1]                                             # at least one shadow first index per table
        ups[l][::4, 0] = n[l + 1]
        if n[l] > 1:
            ups[l][1, 0] = n[l + 1] - 1                                     # ... and the last coarse row
    lens = [torch.tensor([m // 2, m - m // 2], dtype=torch.int32) for m in n]
    lens[2] = torch.tensor([1, 0], dtype=torch.int32)
    batch = {"points": pts, "neighbors": nb, "pools": pools, "upsamples": ups, "stack_lengths": lens,
             "features": torch.ones(n0, 1)}
    return {k: _to(v, dev) for k, v in batch.items()}


def test_hand_made_pyramids_runner_equals_mirror(cuda):
    torch.manual_seed(5)
    net = KPFCNN(indoor_config(first_feats_dim=32, gnn_feats_dim=64)).to(cuda).eval()
    batches = [_hand_made(n0, 40 + i, cuda) for i, n0 in enumerate((130, 257, 64, 191))]
    for b in batches:
        for l in range(3):
            first = b["upsamples"][l][:, 0]
            assert bool((first == b["points"][l + 1].shape[0]).any())
    _check(net, batches, cuda)
