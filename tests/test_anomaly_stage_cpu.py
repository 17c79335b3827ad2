"""CPU: the pieces of ``run_vqvae.py --mode=anomaly`` that need no device (synthanatomy_amd/engines/anomaly.py): the score table, whose one definition
gives the CSV header (from the flags alone) and every row, and the table of the flags that only this mode takes."""
import itertools

import numpy as np
import pytest

import run_vqvae as RV
from synthanatomy_amd.engines import anomaly as AS

# the columns as tests/test_anomaly_cli_gpu.py, test_anomaly_ensemble_cli_gpu.py, test_components_cli_gpu.py and test_median_cli_gpu.py pin them
BASE = ["subject", "sum", "max"]
LABEL = ["dice", "best_dice", "best_dice_threshold", "average_precision"]
FILTERED = ["filtered_sum", "filtered_max"]
FILTERED_LABEL = ["filtered_dice", "filtered_best_dice", "filtered_best_dice_threshold", "filtered_average_precision"]
PLAIN = ["components", "components_kept", "voxels_kept", "largest_component"]
LESION = ["dice_cleaned", "lesions", "lesions_detected", "lesion_recall", "lesion_precision", "lesion_f1"]
MEMBERS = ["members"]


def _summary(rng, threshold=True, members=None):
    hist = rng.integers(0, 50, size=(2, 2, 256)).astype(np.int64)
    counts = {k: rng.integers(1, 99, size=2).astype(np.int64) if threshold else None for k in ("tp", "fp", "fn")}
    s = dict(sum=rng.random(2), max=rng.random(2).astype(np.float32), hist=hist, inv_bin=np.float32(256.0), threshold=None, taps=None, **counts)
    return dict(s, members=members) if members else s


def _components(rng):
    names = ("components", "components_kept", "voxels_foreground", "voxels_kept", "largest_component", "tp", "fp", "fn", "lesions", "lesions_detected", "kept_true")
    return {k: rng.integers(1, 9, size=2).astype(np.int64) for k in names}


@pytest.mark.parametrize("labels, filtered, components, ensemble", list(itertools.product((False, True), repeat=4)))
def test_header_and_rows_come_from_one_table(labels, filtered, components, ensemble):
    cfg = dict(RV.DEFAULTS, mode="anomaly", anomaly_labels="/labels" if labels else None, anomaly_mask="scan" if filtered else None,
               anomaly_min_component=4 if components else None, anomaly_threshold=0.1, anomaly_ensemble="/h/a,/h/b,/h/c" if ensemble else None)
    want = BASE + (LABEL if labels else [])
    if filtered:
        want = want + FILTERED + (FILTERED_LABEL if labels else [])
    if components:
        want = want + PLAIN + (LESION if labels else [])
    if ensemble:
        want = want + MEMBERS
    table = AS.score_table(cfg)
    header = AS.score_header(table)
    assert header == want
    rng = np.random.default_rng(0)
    summaries = {"raw": _summary(rng, members=3 if ensemble else None), "filtered": _summary(rng), "components": _components(rng)}
    for j in range(2):
        row = AS.score_row(table, f"/data/s{j}.nii.gz", summaries, j)
        assert list(row) == header and row["subject"] == f"s{j}" and all(isinstance(v, str) and v for v in row.values())
        assert row["sum"] == repr(float(summaries["raw"]["sum"][j])) and row["max"] == repr(float(summaries["raw"]["max"][j]))
        if filtered:
            assert row["filtered_sum"] == repr(float(summaries["filtered"]["sum"][j])) != row["sum"]
        if components:
            assert row["voxels_kept"] == str(int(summaries["components"]["voxels_kept"][j]))
        if ensemble:
            assert row["members"] == "3"
    # without --anomaly_threshold nothing was counted: the Dice cells are empty, the columns stay
    summaries = {"raw": _summary(rng, threshold=False, members=3 if ensemble else None), "filtered": _summary(rng, threshold=False),
                 "components": _components(rng)}
    row = AS.score_row(table, "s0", summaries, 0)
    assert list(row) == header
    if labels:
        assert row["dice"] == "" and row["best_dice"] != ""
        assert not filtered or row["filtered_dice"] == ""


def test_the_anomaly_only_table_decides_whether_the_checks_run_and_names_the_refusals():
    assert ("anomaly_median", "anomaly_mask", "anomaly_mask_threshold", "anomaly_mask_erosion", "anomaly_min_component", "anomaly_connectivity",
            "anomaly_ensemble") == tuple(name for name, _ in AS.ANOMALY_ONLY)
    assert {k: RV.DEFAULTS[k] for k in AS.ANOMALY_FLAGS} == AS.ANOMALY_FLAGS
    cfg = dict(RV.DEFAULTS, mode="extracting")
    assert AS.anomaly_only_flags_given(cfg) == []
    assert AS.anomaly_only_flags_given(dict(cfg, anomaly_weight="both", anomaly_codes="/h", anomaly_threshold=0.5)) == []      # inert in another mode
    for name, value in (("anomaly_median", 3), ("anomaly_mask", "scan"), ("anomaly_mask_threshold", 0.5), ("anomaly_mask_threshold", False),
                        ("anomaly_mask_erosion", 1), ("anomaly_min_component", 4), ("anomaly_connectivity", 6), ("anomaly_connectivity", None),
                        ("anomaly_ensemble", "/h/a,/h/b")):
        given = dict(cfg, **{name: value})
        assert AS.anomaly_only_flags_given(given) == [name]
        with pytest.raises(ValueError, match=f"--{name}={value}: the flag belongs to --mode=anomaly, not --mode=extracting"):
            AS._check_anomaly_flags(given)
    for name, value in (("anomaly_mask_threshold", None), ("anomaly_mask_threshold", 0), ("anomaly_mask_erosion", None), ("anomaly_connectivity", 26.0)):
        assert AS.anomaly_only_flags_given(dict(cfg, **{name: value})) == []
