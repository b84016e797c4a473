"""The argument contract of the ragged-batch entries (registration, tester, modelnet, kitti, modelnet_prep): for every row of
tests/golden/registration_errors.json -- a call with small literal arguments -- the exception type and the exact message.
The file was recorded by scripts/record_registration_contract.py at the commit before the marshalling moved to
pcrcg_amd/ragged.py -- the rows of generalized and colored ICP, the colour gradients and covariances_from_normals at the commit
before the ICP entries were folded onto one driver --, so it pins the messages and the ORDER of the host checks (the rows with two things wrong), and, with one
valid call per entry, that nothing past the device lookup runs without a device."""
import importlib.util
import json
import os

import pytest

from .conftest import GOLDEN, REPO

_spec = importlib.util.spec_from_file_location("record_registration_contract",
                                               os.path.join(REPO, "scripts", "record_registration_contract.py"))
RC = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(RC)

with open(os.path.join(GOLDEN, "registration_errors.json")) as f:
    ROWS = json.load(f)

ENTRIES = ("registration.feature_match_batch", "registration.register_batch", "registration.estimate_normals_batch",
           "registration.estimate_normals", "registration.compute_fpfh_feature_batch", "registration.compute_fpfh_feature",
           "registration.refine_batch", "registration.refine", "registration.generalized_icp_batch", "registration.generalized_icp",
           "registration.colored_icp_batch", "registration.colored_icp", "registration.color_gradients_batch",
           "registration.color_gradients", "registration.covariances_from_normals", "registration.inlier_ratio_batch",
           "registration.sample_batch",
           "tester.probabilistic_sample_batch", "modelnet.chamfer_batch", "kitti.voxel_down_sample_batch",
           "modelnet_prep.crop_batch")


def test_the_table_covers_every_entry():
    for entry in ENTRIES:
        mine = [r for r in ROWS if r["entry"] == entry]
        assert any(r["raises"] == "ValueError" for r in mine), entry
        # the valid call: it ends at the device lookup (registration's is replaced; the siblings find no device)
        assert any(r["raises"] == "DeviceReached" or (r["raises"] == "RuntimeError" and "no HIP device" in r["message"])
                   for r in mine), entry
    assert {r["entry"] for r in ROWS} == set(ENTRIES)
    assert all(r["raises"] is not None for r in ROWS)


@pytest.mark.parametrize("entry", ENTRIES)
def test_the_rows_of_one_entry(entry):
    rows = [r for r in ROWS if r["entry"] == entry]
    for want, now in zip(rows, RC.observe(rows)):
        assert (now["raises"], now["message"]) == (want["raises"], want["message"]), (want["args"], want["kwargs"])
