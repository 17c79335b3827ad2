"""CPU: the host side of the ensemble anomaly map -- the new symbol and its define in header, ctypes table and library, the entry point's
refusals (made before anything touches a stream: there is no device here), every ``ValueError`` of ``anomaly_map_ensemble``, the ``--anomaly_ensemble``
flag and its refusals, per-member file discovery, and the bound of tests/anomaly_ensemble_ref.py with its two witnesses on an fp32 numpy model of the
rule.  No launch is made here."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import anomaly_ensemble_ref as ER
import run_vqvae as RV
from synthanatomy_amd.engines import anomaly as AS
from conftest import ROOT
from synthanatomy_amd.metrics import anomaly as A


def test_header_ctypes_table_and_library_agree_on_the_symbol_and_the_define():
    from synthanatomy_amd import _ffi
    from synthanatomy_amd.build import build
    txt = open(os.path.join(ROOT, "include", "synthanatomy_hip.h")).read()
    assert re.search(r"^#define SA_ANOMALY_MAX_MEMBERS 16$", txt, flags=re.M)
    assert _ffi.ANOMALY_MAX_MEMBERS == 16 == A.MAX_MEMBERS == ER.MAX_MEMBERS
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    decl = re.search(r"int sa_anomaly_map_ensemble\((.*?)\);", code, flags=re.S).group(1)
    names = [p.split()[-1].lstrip("*") for p in decl.split(",")]
    assert names == ["x", "r", "r_member_stride", "m", "m_member_stride", "label", "a_out", "params", "members", "results", "ws", "stream"]
    assert "sa_anomaly_map_ensemble" in _ffi.declared_symbols()
    restype, argtypes = _ffi._SIGS["sa_anomaly_map_ensemble"]
    assert restype is ctypes.c_int and len(argtypes) == 12 and argtypes[2] is ctypes.c_int64 and argtypes[4] is ctypes.c_int64 and argtypes[8] is ctypes.c_int
    lib = ctypes.CDLL(build(verbose=False))
    assert hasattr(lib, "sa_anomaly_map_ensemble") and lib.sa_abi_version() == 5 == _ffi.ABI_VERSION


def test_the_entry_point_refuses_without_a_device():
    from synthanatomy_amd import _ffi
    from synthanatomy_amd.build import build
    lib = ctypes.CDLL(build(verbose=False))
    fn = lib.sa_anomaly_map_ensemble
    fn.restype, fn.argtypes = _ffi._SIGS["sa_anomaly_map_ensemble"]
    P = _ffi.AnomalyParams(B=2, D=8, H=12, W=20, d=2, h=3, w=5, residual=0, R=3, has_threshold=0, inv_bin=256.0, threshold=0.0)
    vol, lat = 2 * 8 * 12 * 20, 2 * 2 * 3 * 5
    host = (ctypes.c_double * 4)()      # an aligned address that is never read: every call below is refused before the stream is touched
    p = ctypes.cast(host, ctypes.c_void_p)

    def call(r=p, rs=vol, m=p, ms=lat, members=3, params=P):
        return fn(p, r, rs, m, ms, None, p, ctypes.byref(params), members, p, p, None)

    for members in (0, 17, -1, 1 << 20):
        assert call(members=members) == _ffi.SA_EINVAL, members
    assert call(rs=vol - 1) == _ffi.SA_EINVAL and call(rs=0) == _ffi.SA_EINVAL and call(rs=-vol) == _ffi.SA_EINVAL
    assert call(ms=lat - 1) == _ffi.SA_EINVAL and call(ms=0) == _ffi.SA_EINVAL
    assert call(rs=vol - 1, members=1) == _ffi.SA_EINVAL      # a single member's stride is checked like any other
    assert call(r=None) == _ffi.SA_EINVAL
    for field, bad in (("d", 3), ("R", 25), ("residual", 3), ("inv_bin", 0.0), ("B", 0)):      # what an_plan refuses, through this entry point
        Q = _ffi.AnomalyParams.from_buffer_copy(P)
        setattr(Q, field, bad)
        assert call(params=Q) == _ffi.SA_EINVAL, field
    Q = _ffi.AnomalyParams.from_buffer_copy(P)
    Q.B = 65536
    assert call(params=Q, rs=65536 * vol, ms=65536 * lat) == _ffi.SA_EUNSUPPORTED


def test_anomaly_map_ensemble_refuses_by_name_before_the_device(monkeypatch):
    from synthanatomy_amd import _ffi

    def touched():
        raise AssertionError("the device was reached")
    monkeypatch.setattr(_ffi, "require_gpu", touched)
    monkeypatch.setattr(_ffi, "lib", touched)
    x = torch.zeros(2, 1, 8, 12, 16)
    w = torch.zeros(2, 2, 3, 4)
    with pytest.raises(ValueError, match=r"recons holds 17 members"):
        A.anomaly_map_ensemble(x, torch.zeros(17, 2, 1, 8, 12, 16), sigma=1.0)
    with pytest.raises(ValueError, match=r"recons holds 0 members"):
        A.anomaly_map_ensemble(x, [], sigma=1.0)
    with pytest.raises(ValueError, match=r"recons of shape \(2, 1, 8, 12, 16\)"):      # no member axis
        A.anomaly_map_ensemble(x, x, sigma=1.0)
    with pytest.raises(ValueError, match=r"recons\[1\] of shape \(2, 1, 8, 12, 15\)"):
        A.anomaly_map_ensemble(x, [x, torch.zeros(2, 1, 8, 12, 15)], sigma=1.0)
    with pytest.raises(ValueError, match=r"recons\[0\] of shape \(2, 8, 12, 16\)"):
        A.anomaly_map_ensemble(x, [torch.zeros(2, 8, 12, 16), x], sigma=1.0)
    with pytest.raises(ValueError, match=r"weights for 2 of 3 members"):
        A.anomaly_map_ensemble(x, [x, x, x], [w, None, w], sigma=1.0)
    with pytest.raises(ValueError, match=r"weights for 2 of 3 members"):
        A.anomaly_map_ensemble(x, [x, x, x], torch.zeros(2, 2, 2, 3, 4), sigma=1.0)
    with pytest.raises(ValueError, match=r"weights\[1\] of shape \(2, 4, 3, 4\)"):
        A.anomaly_map_ensemble(x, [x, x], [w, torch.zeros(2, 4, 3, 4)], sigma=1.0)
    with pytest.raises(ValueError, match=r"weights of shape \(2, 2, 3, 4\)"):      # no member axis
        A.anomaly_map_ensemble(x, [x, x], w, sigma=1.0)
    with pytest.raises(ValueError, match=r"\(2, 3, 3, 4\)"):      # check_arguments: a grid that does not divide
        A.anomaly_map_ensemble(x, [x, x], torch.zeros(2, 2, 3, 3, 4), sigma=1.0)
    with pytest.raises(ValueError, match="sigma"):
        A.anomaly_map_ensemble(x, [x, x], [w, w], sigma=9)
    with pytest.raises(ValueError, match="hist_max"):
        A.anomaly_map_ensemble(x, [x, x], sigma=1, hist_max=0)
    with pytest.raises(ValueError, match="residual"):
        A.anomaly_map_ensemble(x, [x, x], sigma=1, residual="both")
    with pytest.raises(ValueError, match="threshold"):
        A.anomaly_map_ensemble(x, [x, x], sigma=1, threshold=float("nan"))
    with pytest.raises(ValueError, match="labels"):
        A.anomaly_map_ensemble(x, [x, x], sigma=1, labels=torch.zeros(2, 1, 8, 12, 15))
    with pytest.raises(ValueError, match="volumes"):
        A.anomaly_map_ensemble(torch.zeros(2, 2, 8, 12, 16), [x, x], sigma=1)
    with pytest.raises(AssertionError, match="the device was reached"):      # a valid call goes on to the device
        A.anomaly_map_ensemble(x, [x, x], [w, w], sigma=1)


class _DeviceTouched(Exception):
    pass


@pytest.fixture
def no_device(monkeypatch):
    from synthanatomy_amd.runtime import ddp

    def touched():
        raise _DeviceTouched()
    monkeypatch.setattr(ddp, "init_distributed", touched)
    monkeypatch.setattr(torch.cuda, "is_available", touched)


def _argv(tmp_path, *extra, mode="anomaly"):
    return ["run", "--training_subjects=synthetic:2", "--validation_subjects=synthetic:2", f"--project_directory={tmp_path}/", "--experiment_name=e",
            f"--mode={mode}", *extra]


def test_the_flag_its_default_and_its_two_spellings(tmp_path):
    from synthanatomy_amd.utils.general import parse_flags
    assert RV.DEFAULTS["anomaly_ensemble"] is None and AS._ensemble_specs(parse_flags(_argv(tmp_path), RV.DEFAULTS)) is None
    assert (RV.DEFAULTS["anomaly_codes"], RV.DEFAULTS["anomaly_weight"], RV.DEFAULTS["mode"]) == (None, "mask", "training")      # nothing else moved
    cfg = parse_flags(_argv(tmp_path, "--anomaly_ensemble=/h/a,/h/b/*,/h/c"), RV.DEFAULTS)
    assert cfg["anomaly_ensemble"] == "/h/a,/h/b/*,/h/c" and AS._ensemble_specs(cfg) == ["/h/a", "/h/b/*", "/h/c"]
    AS._check_anomaly_flags(cfg)
    cfg = parse_flags(_argv(tmp_path, "--anomaly_ensemble=('/h/a','/h/b')"), RV.DEFAULTS)
    assert AS._ensemble_specs(cfg) == ["/h/a", "/h/b"]
    AS._check_anomaly_flags(cfg)
    AS._check_anomaly_flags(dict(cfg, anomaly_ensemble=[f"/h/{k}" for k in range(16)]))


@pytest.mark.parametrize("value, what", [("/h/a", "1 members"), (",".join(f"/h/{k}" for k in range(17)), "17 members"), ("/h/a,,/h/b", "empty spec"),
                                         ("/h/a,", "empty spec"), ("('/h/a',7)", "7 is not"), ("7", "7 is not"), ("/h/a,/h/b,/h/a", "/h/a is given twice")])
def test_a_bad_ensemble_flag_is_refused_by_name_before_the_device(tmp_path, no_device, value, what):
    with pytest.raises(ValueError, match=r"--anomaly_ensemble.*" + re.escape(what)):
        RV.run(_argv(tmp_path, f"--anomaly_ensemble={value}"))
    assert not os.path.exists(tmp_path / "e")


def test_the_flag_with_anomaly_codes_or_another_mode_is_refused_and_a_valid_one_goes_on(tmp_path, no_device):
    with pytest.raises(ValueError, match=r"--anomaly_ensemble=/h/a,/h/b with --anomaly_codes=/h/c"):
        RV.run(_argv(tmp_path, "--anomaly_ensemble=/h/a,/h/b", "--anomaly_codes=/h/c"))
    for mode in ("training", "extracting", "decoding"):
        with pytest.raises(ValueError, match=r"--anomaly_ensemble=/h/a,/h/b.*--mode=anomaly, not --mode=" + mode):
            RV.run(_argv(tmp_path, "--anomaly_ensemble=/h/a,/h/b", mode=mode))
    assert not os.path.exists(tmp_path / "e")
    with pytest.raises(_DeviceTouched):
        RV.run(_argv(tmp_path, "--anomaly_ensemble=/h/a,/h/b"))
    with pytest.raises(_DeviceTouched):      # without the flag the other modes run as before
        RV.run(_argv(tmp_path, mode="extracting"))


def test_healing_outputs_are_found_per_member(tmp_path):
    import run_transformer as RT
    grid = np.zeros((2, 2, 2))
    dirs = [str(tmp_path / name) + "/" for name in ("a", "b", "c")]
    for d in dirs:
        for stem in ("s0", "s1"):
            RT.save_healing(grid, grid, grid, d, f"/codes/{stem}_quantization_0.npy")
    subjects = ["/data/s0.nii.gz", "/data/s1.npy"]
    members = AS.find_ensemble_outputs(subjects, dirs)
    assert len(members) == 3 and all(len(recs) == 2 for recs in members)
    for d, recs in zip(dirs, members):
        assert recs == AS.find_healing_outputs(subjects, d)
        assert [os.path.relpath(r["healed"], d) for r in recs] == [f"{s}_quantization_0/{s}_quantization_0_healed_sample.npy" for s in ("s0", "s1")]
    # every member needs exactly one match per subject, as a single healing does
    with pytest.raises(ValueError, match=r"s2\.npy: no healing output"):
        AS.find_ensemble_outputs(subjects + ["/data/s2.npy"], dirs)
    os.remove(members[1][0]["nll"])
    with pytest.raises(ValueError, match=r"s0\.nii\.gz.*s0_quantization_0_nll\.npy"):
        AS.find_ensemble_outputs(subjects, dirs, weight="nll")
    # two specs that differ as strings and reach the same healed file for s1
    with pytest.raises(ValueError, match=r"/data/s0\.nii\.gz: members 0 \(.*a/\) and 2 \(.*a/s\*\) .* same healed file"):
        AS.find_ensemble_outputs(subjects, [dirs[0], dirs[1], dirs[0] + "s*"])
    os.symlink(dirs[0], str(tmp_path / "link"))
    with pytest.raises(ValueError, match=r"same healed file"):
        AS.find_ensemble_outputs(subjects, [dirs[0], str(tmp_path / "link") + "/"])
    # a member whose code grid has another shape
    RT.save_healing(np.zeros((2, 2, 3)), np.zeros((2, 2, 3)), np.zeros((2, 2, 3)), dirs[2], "/codes/s1_quantization_0.npy")
    with pytest.raises(ValueError, match=r"/data/s1\.npy: member 2 \(.*c/\) .* shape \(2, 2, 3\), member 0 \(.*a/\) has \(2, 2, 2\)"):
        AS.find_ensemble_outputs(subjects, dirs)


def test_compose_fp32_of_one_member_is_the_identity_and_the_scale_is_the_hosts():
    rng = np.random.default_rng(0)
    a = rng.random((3, 5, 7), dtype=np.float32)
    a[0, 0, :3] = (0.0, -0.0, np.float32(1e-45))      # zeros of either sign and the smallest subnormal survive
    assert ER.compose_fp32([a]).tobytes() == a.tobytes()
    b, c = rng.random((3, 5, 7), dtype=np.float32), rng.random((3, 5, 7), dtype=np.float32)
    assert ER.compose_fp32([a, b]).tobytes() == ER.compose_fp32([b, a]).tobytes()
    want = ((a + b) + c) * np.float32(1.0 / 3)
    assert ER.compose_fp32([a, b, c]).tobytes() == want.tobytes() and want.dtype == np.float32
    for K in range(1, 17):      # (float)(1.0 / (double)K): the double rounded once to fp32
        assert np.float32(1.0 / K) == ctypes.c_float(1.0 / K).value


@pytest.mark.parametrize("case", sorted(ER.CASES))
def test_an_fp32_model_of_the_rule_stays_inside_the_bound_and_the_witnesses_do_not(case):
    for K, mode in ((3, "abs"), (2, "positive"), (5, "negative")):
        good, unscaled, rotated = ER.worst_ratios(ER.model_fp32(case, K, mode), case, K, mode)
        print(f"{case} K = {K} {mode}: worst |err| / bound {good:.4f}; without inv_K {unscaled:.4g}; weights rotated {rotated:.4g}")
        assert good <= 1.0
        assert unscaled > 1.0
        if ER.CASES[case][1] is not None:      # (without grids every weight is 1 and there is nothing to rotate)
            assert rotated > 1.0
