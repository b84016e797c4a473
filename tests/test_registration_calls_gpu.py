"""Which library calls the ragged-batch entries make: every case of tests/registration_cases.py, run once per form of input
(numpy, device tensors, mixed), against tests/golden/registration_calls.json -- the sequence of library entries with every
non-pointer argument, whether each pointer was null, and how often the device was read.  The file was recorded on the GPU
by scripts/registration_digests.py --record-calls at the commit before the marshalling moved to pcrcg_amd/ragged.py, and again,
with the cases of generalized and colored ICP, the colour gradients and covariances_from_normals added, at the commit before
the ICP entries were folded onto one driver (registration._icp_batch); only the colored ICP cases were then recorded from the
folded code, which builds the ICP cell grid before the normals and gradients and not after.  The three forms gave one record
each time, so it is kept once.  No numerical result is checked here: the suites of the entries do that."""
import json
import os

import pytest

from . import registration_cases as RC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden(golden_dir):
    with open(os.path.join(golden_dir, "registration_calls.json")) as f:
        return json.load(f)


@pytest.mark.parametrize("form", RC.FORMS)
def test_calls_arguments_and_reads_are_the_recorded_ones(cuda, golden, form):
    got = json.loads(json.dumps(RC.record_calls(form, cuda)))       # tuples -> lists, as the file holds them
    assert list(got) == list(golden)
    for name in golden:
        assert got[name]["counters"] == golden[name]["counters"], name
        assert [c[0] for c in got[name]["calls"]] == [c[0] for c in golden[name]["calls"]], name
        for mine, want in zip(got[name]["calls"], golden[name]["calls"]):
            assert mine == want, name


def test_the_cases_reach_every_branch_of_the_marshalling(golden):
    """What the inputs are chosen for: chunks of 2, 2 and 1; a null cloud pointer in the empty chunk; both ICP entries."""
    def calls(case, entry):
        return [c for c in golden[case]["calls"] if c[0] == entry]
    assert [c[9] for c in calls("register_batch/c32", "pcrcg_ransac_batch")] == [2, 2, 1]
    empty = ["null" if sum(n for n, _ in RC.EMPTY[b0:b0 + RC.PER_CALL]) == 0 else "ptr" for b0 in range(0, RC.B, RC.PER_CALL)]
    assert empty == ["null", "ptr", "null"]
    assert [c[1] for c in calls("estimate_normals_batch/empty_chunk", "pcrcg_cellgrid_build")] == empty
    assert [c[1] for c in calls("refine_batch/point/empty_chunk", "pcrcg_icp_batch")] == empty
    assert len(calls("refine_batch/plane_normals", "pcrcg_icp_batch_ex")) == 3 and not calls("refine_batch/plane_normals", "pcrcg_icp_batch")
    assert len(calls("refine_batch/point", "pcrcg_icp_batch")) == 3 and not calls("refine_batch/point", "pcrcg_icp_batch_ex")
    assert all(golden[k]["counters"]["d2h_reads"] == 1 for k in golden if k.startswith(("register_batch", "refine_batch", "inlier")))
    # the estimators that joined the ICP loop later: their own entry three times per batched case and no other ICP entry, the
    # empty chunk's null clouds, one read per call; the gradients and covariances alone read nothing
    icp_entries = ("pcrcg_icp_batch", "pcrcg_icp_batch_ex", "pcrcg_gicp_batch", "pcrcg_colored_icp_batch")
    for prefix, entry in (("generalized_icp_batch/", "pcrcg_gicp_batch"), ("colored_icp_batch/", "pcrcg_colored_icp_batch")):
        batched = [k for k in golden if k.startswith(prefix)]
        assert len(batched) >= 8 and sum(k.endswith("/empty_chunk") for k in batched) * 2 == len(batched)
        for k in batched:
            assert len(calls(k, entry)) == 3 and not any(calls(k, other) for other in icp_entries if other != entry), k
            assert [c[9] for c in calls(k, entry)] == [2, 2, 1], k
            assert golden[k]["counters"]["d2h_reads"] == 1, k
            if k.endswith("/empty_chunk"):
                assert [c[1] for c in calls(k, entry)] == empty, k
    empty_tgt = ["null" if sum(m for _, m in RC.EMPTY[b0:b0 + RC.PER_CALL]) == 0 else "ptr" for b0 in range(0, RC.B, RC.PER_CALL)]
    assert empty_tgt == ["null", "ptr", "ptr"]
    assert [c[15] for c in calls("generalized_icp_batch/covariances/empty_chunk", "pcrcg_gicp_batch")] == empty_tgt   # tgt_cov
    assert [c[14] for c in calls("generalized_icp_batch/covariances/empty_chunk", "pcrcg_gicp_batch")] == empty       # src_cov
    assert [c[15] for c in calls("colored_icp_batch/normals_rgb/empty_chunk", "pcrcg_colored_icp_batch")] == empty_tgt  # tgt_rec
    assert [c[16] for c in calls("colored_icp_batch/normals_rgb/empty_chunk", "pcrcg_colored_icp_batch")] == empty      # src_intensity
    assert [c[1] for c in calls("color_gradients_batch/empty_chunk", "pcrcg_color_gradients_batch")] == empty
    assert len(calls("color_gradients_batch", "pcrcg_color_gradients_batch")) == 3
    assert all(golden[k]["counters"]["d2h_reads"] == 0 for k in golden if k.startswith(("color_gradients", "covariances_from")))
    assert all(golden[k]["counters"]["d2h_reads"] == 1 for k in ("generalized_icp", "colored_icp"))
    assert [c[0] for c in golden["covariances_from_normals"]["calls"]] == ["pcrcg_covariances_from_normals"]
