"""CPU: the argument rules of the robust kernels -- registration.RobustKernel and its constructors, robust_refine_batch,
robust_colored_icp_batch, kernel= of refine / colored_icp, and the C entries pcrcg_icp_plane_robust_batch / pcrcg_colored_icp_robust_batch -- none
of which needs a device (registration._device is replaced, as tests/test_registration_contract_cpu.py replaces it), and the
outlier scene's claim on the numpy restatement alone."""
import ctypes

import numpy as np
import pytest

from pcrcg_amd import _lib
from pcrcg_amd import registration as REG

from . import icp_plane_ref as PR
from . import robust_ref as RK


class DeviceReached(Exception):
    pass


@pytest.fixture
def no_device(monkeypatch):
    def stop(*a, **k):
        raise DeviceReached("the device lookup")
    monkeypatch.setattr(REG, "_device", stop)


P, Q = np.zeros((5, 3), np.float32), np.zeros((7, 3), np.float32)
NRM = np.zeros((7, 3))


def _plane(kernel=None, **kw):
    return REG.robust_refine_batch([P], [Q], None, 0.1, kernel, tgt_normals=[NRM], **kw)


def _colored(kernel=None, **kw):
    return REG.robust_colored_icp_batch([P], [Q], [np.zeros(5)], [np.zeros((7, 3))], None, 0.1, kernel, tgt_normals=[NRM], **kw)


def test_the_constructors_carry_open3ds_names_and_check_k():
    made = [REG.L2Loss(), REG.L1Loss(), REG.HuberLoss(0.005), REG.CauchyLoss(0.5), REG.GMLoss(1e-4), REG.TukeyLoss(3)]
    assert [m.kind for m in made] == [0, 1, 2, 3, 4, 5]
    assert [m.k for m in made[2:]] == [0.005, 0.5, 1e-4, 3.0] and isinstance(made[5].k, float)
    assert all(isinstance(m, REG.RobustKernel) for m in made)
    assert repr(made[2]) == "HuberLoss(0.005)" and repr(made[0]) == "L2Loss()"
    assert REG.HuberLoss(0.005) == REG.HuberLoss(0.005) and REG.HuberLoss(0.005) != REG.CauchyLoss(0.005)
    with pytest.raises(AttributeError):
        made[2].k = 1.0                                     # immutable
    for make in (REG.HuberLoss, REG.CauchyLoss, REG.GMLoss, REG.TukeyLoss):
        for bad in (0, 0.0, -1, float("nan"), float("inf"), -float("inf"), None, "x"):
            with pytest.raises(ValueError, match="k must be a positive finite number"):
                make(bad)
    for bad in (-1, 6, 2.0, True, "Huber"):
        with pytest.raises(ValueError, match="kind must be 0..5"):
            REG.RobustKernel(bad, 1.0)


def test_kernel_none_reaches_the_device_lookup_as_before(no_device):
    for call in (_plane, _colored):
        with pytest.raises(DeviceReached):
            call()
        with pytest.raises(DeviceReached):
            call(kernel=None)
        with pytest.raises(DeviceReached):
            call(kernel=REG.HuberLoss(0.005))               # a kernel passes the host checks too
    with pytest.raises(DeviceReached):
        REG.refine_batch([P], [Q], None, 0.1)
    with pytest.raises(DeviceReached):
        REG.refine_batch([P], [Q], None, 0.1, estimation="point_to_plane", tgt_normals=[NRM])
    with pytest.raises(DeviceReached):
        REG.colored_icp_batch([P], [Q], [np.zeros(5)], [np.zeros((7, 3))], None, 0.1, tgt_normals=[NRM])
    with pytest.raises(DeviceReached):
        REG.refine(P, Q, None, 0.1, estimation="point_to_plane", tgt_normals=NRM, kernel=None)
    with pytest.raises(DeviceReached):
        REG.refine(P, Q, None, 0.1, estimation="point_to_plane", tgt_normals=NRM, kernel=REG.TukeyLoss(0.1))
    with pytest.raises(DeviceReached):
        REG.colored_icp(P, Q, np.zeros(5), np.zeros(7), None, 0.1, tgt_normals=NRM, kernel=REG.L1Loss())


def test_what_is_not_a_kernel_raises(no_device):
    for bad in (2, 0.005, "huber", (2, 0.005), REG.HuberLoss, object()):
        for call in (_plane, _colored):
            with pytest.raises(TypeError, match="kernel must be a RobustKernel"):
                call(kernel=bad)
    with pytest.raises(TypeError, match="refine_batch: kernel must be a RobustKernel"):
        REG.refine(P, Q, None, 0.1, estimation="point_to_plane", tgt_normals=NRM, kernel="huber")
    with pytest.raises(TypeError, match="robust_colored_icp_batch: kernel must be a RobustKernel"):
        REG.colored_icp(P, Q, np.zeros(5), np.zeros(7), None, 0.1, tgt_normals=NRM, kernel=3)


def test_point_to_point_takes_no_kernel(no_device):
    for kernel in (REG.L2Loss(), REG.HuberLoss(0.005)):
        with pytest.raises(ValueError, match="a kernel belongs to estimation='point_to_plane'"):
            REG.refine(P, Q, None, 0.1, kernel=kernel)
        with pytest.raises(ValueError, match="a kernel belongs to estimation='point_to_plane'"):
            REG.refine(P, Q, None, 0.1, estimation="point_to_point", kernel=kernel)
    with pytest.raises(TypeError):
        REG.robust_refine_batch([P], [Q], None, 0.1, REG.L2Loss(), estimation="point_to_point")      # point-to-plane alone
    assert "kernel" not in REG.generalized_icp_batch.__kwdefaults__            # out of scope, and said so in its place


def test_the_new_checks_come_after_the_existing_ones(no_device):
    """Two things wrong: the older message is the one that is raised."""
    with pytest.raises(ValueError, match="robust_refine_batch: max_correspondence_distance must be positive"):
        REG.robust_refine_batch([P], [Q], None, -1.0, "huber", tgt_normals=[NRM])
    with pytest.raises(ValueError, match="the target normals must have one row per target point"):
        REG.robust_refine_batch([P], [Q], None, 0.1, "huber", tgt_normals=[np.zeros((6, 3))])
    with pytest.raises(ValueError, match="refine_batch: tgt_normals / normal_radius belong to estimation='point_to_plane'"):
        REG.refine(P, Q, None, 0.1, tgt_normals=NRM, kernel=REG.HuberLoss(1.0))
    with pytest.raises(ValueError, match="lambda_geometric must lie in"):
        _colored(lambda_geometric=2.0, kernel=7)
    with pytest.raises(ValueError, match="colours must have one row per point"):
        REG.robust_colored_icp_batch([P], [Q], [np.zeros(4)], [np.zeros(7)], None, 0.1, 7, tgt_normals=[NRM])


# --- the C entries ---------------------------------------------------------------------------------------------------------------
FAKE = ctypes.c_void_p(4096)
HEAD = dict(src=FAKE, src_off=FAKE, n_total=10, n_max=10, tgt_off=FAKE, m_total=12, grid=FAKE, init=None, B=1, d=0.1, mi=5,
            rf=1e-6, rr=1e-6)
TAIL = dict(out_t=FAKE, out_s=FAKE, trace=None, ws=FAKE, wsb=1 << 20, stream=None)
ENTRIES = {"pcrcg_icp_plane_robust_batch": dict(HEAD, nrm=FAKE, kernel=2, k=0.005, **TAIL),
           "pcrcg_colored_icp_robust_batch": dict(HEAD, lam=0.968, tgt_rec=FAKE, src_int=FAKE, kernel=2, k=0.005, **TAIL)}
PLAIN = {"pcrcg_icp_plane_robust_batch": "pcrcg_icp_batch_ex", "pcrcg_colored_icp_robust_batch": "pcrcg_colored_icp_batch"}
BAD_K = (0.0, -1.0, float("nan"), float("inf"), -float("inf"))


@pytest.mark.parametrize("entry", sorted(ENTRIES))
def test_the_c_entries_reject_bad_arguments_before_any_launch(entry):
    """Every call below ends in the argument rules or at the workspace carve: with fake pointers nothing may launch.  The one
    way past both is a call that is right, so the accepted kernels are shown by what they fail on LATER: another argument."""
    lib = _lib.lib()
    good = ENTRIES[entry]

    def call(**kw):
        return getattr(lib, entry)(*{**good, **kw}.values())

    def refused(what, **kw):
        assert call(**kw) == -1, kw
        msg = lib.pcrcg_last_error()
        assert (entry + ": bad argument").encode() in msg and what.encode() in msg, (kw, msg)

    for kind in (-1, 6, 7, 1 << 30, -(1 << 31)):
        refused("c.kernel >= 0", kernel=kind)
    for kind in (2, 3, 4, 5):
        for k in BAD_K:
            refused("c.kernel_k > 0.0", kernel=kind, k=k)
    # kinds 0 and 1 read no scale: whatever it is, the call goes on to the next thing that is wrong
    for kind in (0, 1):
        for k in BAD_K + (0.005,):
            assert call(kernel=kind, k=k, wsb=64) == -2 and b"workspace too small" in lib.pcrcg_last_error(), (kind, k)
    for kind in (2, 3, 4, 5):
        assert call(kernel=kind, k=1e-300, wsb=64) == -2 and call(kernel=kind, k=1e300, wsb=64) == -2
    # the kernel rules come after the plain entry's: its messages stand
    other = dict(nrm=None) if "plane" in entry else dict(tgt_rec=None)
    refused("tgt_normals" if "plane" in entry else "tgt_rec", kernel=9, **other)
    for kw in (dict(src=None), dict(src_off=None), dict(grid=None), dict(out_t=None), dict(ws=None), dict(B=0), dict(B=65536),
               dict(n_max=11), dict(d=0.0), dict(d=float("nan")), dict(mi=0), dict(rf=-1.0), dict(rr=float("nan"))):
        refused("", **kw)
    if "colored" in entry:
        refused("lambda_geometric", lam=1.5)
        refused("src_intensity", src_int=None)
    assert call(wsb=64) == -2 and (entry + ": workspace too small").encode() in lib.pcrcg_last_error()     # PCRCG_EWORKSPACE
    # the workspace is the plain entry's
    ws_bytes, plain = getattr(lib, entry + "_ws_bytes"), getattr(lib, PLAIN[entry] + "_ws_bytes")
    for args in ((1, 10, 12, 5), (2, 1000, 900, 30), (7, 0, 0, 1), (65535, 100000, 5, 1 << 16)):
        assert ws_bytes(*args) == plain(*args) > 0, args
    for args in ((0, 10, 10, 5), (65536, 10, 10, 5), (1, -1, 10, 5), (1, 10, -1, 5), (1, 10, 10, 0), (1, 10, 10, (1 << 16) + 1)):
        assert ws_bytes(*args) == 0, args


def test_the_abi_version_and_the_bindings():
    lib = _lib.lib()
    assert lib.pcrcg_abi_version() == 4 == _lib.ABI_VERSION
    extra = {"pcrcg_icp_plane_robust_batch": [ctypes.c_void_p, ctypes.c_int, ctypes.c_double],
             "pcrcg_colored_icp_robust_batch": [ctypes.c_double, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_double]}
    for name, mid in extra.items():
        assert _lib.SIGNATURES[name] == (ctypes.c_int, _lib._ICP_HEAD + mid + _lib._ICP_TAIL)
        assert _lib.SIGNATURES[name + "_ws_bytes"] == (ctypes.c_size_t, [ctypes.c_int] * 4)
    # the plain entries' bindings did not move
    assert _lib.SIGNATURES["pcrcg_icp_batch_ex"] == (ctypes.c_int, _lib._ICP_HEAD + [ctypes.c_int, ctypes.c_void_p] + _lib._ICP_TAIL)


# --- the claim, on the restatement ---------------------------------------------------------------------------------------------
def test_the_outlier_scene_is_what_it_claims_on_the_restatement():
    """One scene of tests/test_robust_icp_gpu.py's seven (the others run there, beside the device): a quarter of the targets on a
    second sheet 0.03 off, inside d = 0.06.  Plain point-to-plane ends a centimetre off; Huber, Cauchy and GM at a third of
    that or far below."""
    src, tgt, nrm, start, T_gt = RK.outlier_scene(1, 600)
    assert 0.2 < (np.abs(((tgt - (src.astype(np.float64) @ T_gt[:3, :3].T + T_gt[:3, 3])) * nrm).sum(1)) > 0.02).mean() < 0.3
    e = {}
    for name, kind, k in (("plain", RK.L2, 1.0), ("Huber", RK.HUBER, 0.005), ("Cauchy", RK.CAUCHY, 0.005), ("GM", RK.GM, 1e-4),
                          ("Tukey", RK.TUKEY, 0.015)):
        T = RK.plane_icp(src, tgt, nrm, start, RK.OUTLIER_D, kind, k, max_iteration=RK.OUTLIER_MI)[0]
        e[name] = PR.worst_displacement(src, T, T_gt)
    print({k: f"{1e3 * v:.3f} mm" for k, v in e.items()})
    # kind 0 of the restatement is the plain restatement
    plain = PR.icp(src, tgt, nrm, start, RK.OUTLIER_D, max_iteration=RK.OUTLIER_MI)
    assert PR.worst_displacement(src, plain[0], T_gt) == e["plain"]
    assert e["plain"] > 5e-3
    for name in ("Huber", "Cauchy", "GM", "Tukey"):
        assert e[name] < e["plain"] / 3, (name, e)
