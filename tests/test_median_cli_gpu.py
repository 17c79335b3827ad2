"""GPU: ``run_vqvae.py --mode=anomaly --anomaly_median=3 --anomaly_mask=... --anomaly_mask_erosion=1`` end to end, set up like
tests/test_components_cli_gpu.py: a randomly initialised two-level VQ-VAE (factor 4) with its own encoder outputs as the codebook, two 16 x 16 x 16
subjects and a planted healing.  ``<name>_anomaly_map_filtered`` must equal the numpy reference applied to the WRITTEN ``<name>_anomaly_map`` and the
same mask bit for bit, the segmentation must come from the filtered map, and the ``filtered_*`` columns must match the host helpers; without the four
flags the run writes the files and the header it wrote before."""
import contextlib
import csv
import io
import os

import numpy as np
import pytest

import components_ref
import median_ref as ref
from nifti_ref import signed_perm_affine, write_nifti

pytestmark = pytest.mark.gpu

SIDE, LATENT = (16, 16, 16), (4, 4, 4)
BLOCK = (slice(1, 3),) * 3
PERM, SIGN = (2, 0, 1), (-1, 1, -1)   # how the NIfTI copies are stored
NAMES = ("s0", "s1")
T = 0.002
MASK_T = 0.4375      # exact in fp32
HIST_MAX = 0.25
SCORES = ["--anomaly_sigma=0.5", f"--anomaly_threshold={T}", f"--anomaly_hist_max={HIST_MAX}"]
FILTERED = ["filtered_sum", "filtered_max"]
FILTERED_LABEL = ["filtered_dice", "filtered_best_dice", "filtered_best_dice_threshold", "filtered_average_precision"]
PLAIN = ["components", "components_kept", "voxels_kept", "largest_component"]
LESION = ["dice_cleaned", "lesions", "lesions_detected", "lesion_recall", "lesion_precision", "lesion_f1"]


def _flags(proj, extra=()):
    return ["--project_directory=" + proj, "--experiment_name=fixed", "--no_levels=2", "--downsample_parameters=((4,2,1,1),(4,2,1,1))",
            "--upsample_parameters=((4,2,1,0,1),(4,2,1,0,1))", "--no_channels=32", "--num_embeddings=(64,)", "--embedding_dim=(16,)", "--decay=(0.5,)",
            "--roi=((0,16),(0,16),(0,16))", "--batch_size=2", "--eval_batch_size=2", "--amp=False", "--num_workers=0", *extra]


def _stored(canonical, perm, sign):
    v = canonical
    for a in range(3):
        if sign[a] < 0:
            v = np.flip(v, axis=a)
    return np.ascontiguousarray(np.transpose(v, np.argsort(perm)))


def _run(argv):
    import run_vqvae
    with contextlib.redirect_stdout(io.StringIO()):
        run_vqvae.run(argv)


def _rows(out):
    with open(out + "anomaly_scores_rank0.csv", newline="") as f:
        return list(csv.DictReader(f))


def _listing(out):
    return sorted(os.path.join(d, f) for d in NAMES for f in os.listdir(out + d)) + sorted(f for f in os.listdir(out) if f.endswith(".csv"))


@pytest.fixture(scope="module")
def work(tmp_path_factory):
    """(project, outputs, the files and the CSV header of a run WITHOUT the flags, the scans as the encoder saw them) after extraction and a healing"""
    import torch
    import run_transformer
    import run_vqvae
    from synthanatomy_amd.utils.general import parse_flags
    proj = str(tmp_path_factory.mktemp("median_cli")) + "/"
    for d in ("npy", "nii", "labels", "masks", "masks_nii", "heal"):
        os.mkdir(proj + d)
    rng = np.random.default_rng(0)
    label = np.zeros(SIDE, dtype=np.float32)
    label[4:12, 4:12, 4:12] = 1.0
    g = np.meshgrid(*[np.arange(n) - (n - 1) / 2 for n in SIDE], indexing="ij")
    brain = ((g[0] / 8.5) ** 2 + (g[1] / 7.0) ** 2 + (g[2] / 7.5) ** 2 <= 1.0).astype(np.float32)      # touches the border along the first axis
    for name in NAMES:
        x, y, z = np.meshgrid(*(np.arange(n) / n for n in SIDE), indexing="ij")
        v = (0.5 + 0.3 * np.sin(5 * x + 1) * np.cos(3 * y) + 0.2 * z * x + 0.05 * rng.standard_normal(SIDE)).astype(np.float32)
        np.save(f"{proj}npy/{name}.npy", v)
        np.save(f"{proj}labels/{name}.npy", label * 3.0)      # labels and masks are not normalised: class 1 where > 0.5
        np.save(f"{proj}masks/{name}.npy", brain * 7.0)
        write_nifti(f"{proj}nii/{name}.nii", _stored(v, PERM, SIGN), sform=signed_perm_affine(PERM, SIGN))
        write_nifti(f"{proj}masks_nii/{name}.nii", _stored(brain * 7.0, PERM, SIGN), sform=signed_perm_affine(PERM, SIGN))
    sub = [f"--training_subjects={proj}npy", f"--validation_subjects={proj}npy"]
    cfg = parse_flags(_flags(proj, sub + ["--mode=extracting"]), run_vqvae.DEFAULTS)
    torch.manual_seed(0)
    dev = torch.device("cuda", 0)
    net = run_vqvae.build_network(cfg, dev).eval()
    # an untrained network maps every position to one code: 64 of its own encoder outputs as the codebook make the codes depend on the position
    x = torch.stack([run_vqvae._load_volume(f"{proj}npy/{name}.npy", cfg, None, dev) for name in NAMES])
    scans = {name: x[j].reshape(SIDE).cpu().numpy() for j, name in enumerate(NAMES)}
    with torch.no_grad():
        z = net.encode(x)[0].float()
    book = z.movedim(1, -1).reshape(-1, z.shape[1])[::2][:64].contiguous()
    sd = {k: v.clone() for k, v in net.state_dict().items()}
    keys = [k for k in sd if k.endswith(("impl.weight", "impl.embedding.weight", "impl.embed_avg"))]
    assert len(keys) == 3
    for k in keys:
        sd[k] = book.clone()
    os.makedirs(proj + "fixed/baseline_vqvae/checkpoints")
    torch.save({"network": sd}, proj + "fixed/baseline_vqvae/checkpoints/checkpoint_epoch=1.pt")
    out = proj + "fixed/baseline_vqvae/outputs/"
    _run(_flags(proj, sub + ["--mode=extracting"]))
    for name in NAMES:
        codes = np.load(f"{out}{name}/{name}_quantization_0.npy")
        new = codes.copy()
        new[BLOCK] = (codes[BLOCK] + 1 + rng.integers(0, 62, size=(2, 2, 2))) % 64      # every entry of the block changes
        mask = np.zeros(LATENT, dtype=bool)
        mask[BLOCK] = True
        run_transformer.save_healing(new, rng.exponential(1.0, LATENT).astype(np.float32), mask, f"{proj}heal/", f"{out}{name}/{name}_quantization_0.npy")
    _run(_flags(proj, sub + ["--mode=anomaly", f"--anomaly_codes={proj}heal", f"--anomaly_labels={proj}labels", *SCORES]))
    before = _listing(out)
    header = list(_rows(out)[0])
    assert header == ["subject", "sum", "max", "dice", "best_dice", "best_dice_threshold", "average_precision"]
    assert not any("filtered" in f or "segmentation" in f for f in before)
    return proj, out, before, header, scans


def _check_filtered_columns(row, want, label):
    from synthanatomy_amd.metrics.anomaly import average_precision, best_dice, dice_from_counts
    s = ref.summaries(want, np.float32(256 / HIST_MAX), label, T)
    total = float(row["filtered_sum"])
    assert abs(total - s["sum"]) <= want.size * 2.0 ** -53 * float(np.abs(want.astype(np.float64)).sum())
    assert float(row["filtered_max"]) == float(s["max"])
    if label is not None:
        bd, bt = best_dice(s["hist"][0], s["hist"][1], np.float32(256 / HIST_MAX))
        assert float(row["filtered_dice"]) == dice_from_counts(s["tp"], s["fp"], s["fn"])
        assert (float(row["filtered_best_dice"]), float(row["filtered_best_dice_threshold"])) == (bd, bt)
        assert float(row["filtered_average_precision"]) == average_precision(s["hist"][0], s["hist"][1])


def test_scan_mask_with_labels_the_filtered_map_is_the_reference_of_the_written_map_and_feeds_the_components(work):
    proj, out, before, header, scans = work
    sub = [f"--training_subjects={proj}npy", f"--validation_subjects={proj}npy", "--mode=anomaly", f"--anomaly_codes={proj}heal",
           f"--anomaly_labels={proj}labels", *SCORES]
    _run(_flags(proj, sub + ["--anomaly_median=3", "--anomaly_mask=scan", f"--anomaly_mask_threshold={MASK_T}", "--anomaly_mask_erosion=1",
                             "--anomaly_min_component=4"]))
    assert set(_listing(out)) == set(before) | {f"{n}/{n}_anomaly_{post}.npy" for n in NAMES for post in ("map_filtered", "segmentation")}
    rows = _rows(out)
    assert list(rows[0]) == header + FILTERED + FILTERED_LABEL + PLAIN + LESION and [r["subject"] for r in rows] == list(NAMES)
    label = np.load(f"{proj}labels/s0.npy") > 0.5
    for name, row in zip(NAMES, rows):
        raw = np.load(f"{out}{name}/{name}_anomaly_map.npy")
        mask = scans[name] > np.float32(MASK_T)
        assert 0 < ref.erode(mask, 1).sum() < mask.sum() < mask.size
        want = ref.median(raw, 3, mask, 1)
        got = np.load(f"{out}{name}/{name}_anomaly_map_filtered.npy")
        assert got.dtype == np.float32 and got.view(np.int32).tobytes() == want.view(np.int32).tobytes()
        assert want.any() and want.view(np.int32).tobytes() != raw.view(np.int32).tobytes()
        assert (repr(float(raw.astype(np.float64).sum())) != row["filtered_sum"]) and float(row["max"]) == float(raw.max())      # the old columns: the raw map
        _check_filtered_columns(row, want, label)
        ids, s = components_ref.components(want, np.float32(T), 26, 4, label)
        ids_raw, _ = components_ref.components(raw, np.float32(T), 26, 4, label)
        seg = np.load(f"{out}{name}/{name}_anomaly_segmentation.npy")
        assert np.array_equal(seg, (ids > 0).astype(np.float32)) and seg.any() and not np.array_equal(seg, (ids_raw > 0).astype(np.float32))
        assert [int(row[k]) for k in PLAIN] == [s["components"], s["components_kept"], s["voxels_kept"], s["largest_component"]]
    # without the four flags again: the header is the old one
    _run(_flags(proj, sub))
    assert list(_rows(out)[0]) == header


def test_a_mask_directory_nifti_subjects_and_nifti_outputs_carry_the_source_geometry(work):
    from synthanatomy_amd.utils.nifti import read_nifti
    from synthanatomy_amd.utils.vqvae import hip_ingest
    proj, out, before, header, scans = work
    _run(_flags(proj, [f"--training_subjects={proj}nii", f"--validation_subjects={proj}nii", "--mode=anomaly", f"--anomaly_codes={proj}heal",
                       "--anomaly_sigma=0.5", f"--anomaly_threshold={T}", f"--anomaly_hist_max={HIST_MAX}", "--anomaly_median=3",
                       f"--anomaly_mask={proj}masks_nii", "--anomaly_mask_erosion=1", "--anomaly_min_component=3", "--output_ext=.nii"]))
    rows = _rows(out)
    assert list(rows[0]) == ["subject", "sum", "max"] + FILTERED + PLAIN

    def back(name, post):
        hdr, raw = read_nifti(f"{out}{name}/{name}_{post}.nii")
        return hip_ingest(hdr, raw, None, normalize=False, canonical=True, device="cuda:0")[0].cpu().numpy()
    brain = np.load(f"{proj}masks/s0.npy") > 0.5      # the canonical orientation of the stored NIfTI mask
    for name, row in zip(NAMES, rows):
        raw = back(name, "anomaly_map")
        want = ref.median(raw, 3, brain, 1)
        got = back(name, "anomaly_map_filtered")
        assert got.shape == SIDE and got.view(np.int32).tobytes() == want.view(np.int32).tobytes() and want.any()
        _check_filtered_columns(row, want, None)
        ids, s = components_ref.components(want, np.float32(T), 26, 3, None)
        assert np.array_equal(back(name, "anomaly_segmentation"), (ids > 0).astype(np.float32))
        assert read_nifti(f"{out}{name}/{name}_anomaly_map_filtered.nii")[0].affine.tolist() == read_nifti(f"{out}{name}/{name}_anomaly_map.nii")[0].affine.tolist()
        src = read_nifti(f"{proj}nii/{name}.nii")[0]      # the whole volume is the ROI: the source's own affine
        assert np.allclose(read_nifti(f"{out}{name}/{name}_anomaly_map_filtered.nii")[0].affine, src.affine, rtol=0, atol=1e-5)


def test_a_mask_alone_is_size_one_and_npy_mask_volumes_are_matched_by_stem(work):
    proj, out, before, header, scans = work
    _run(_flags(proj, [f"--training_subjects={proj}npy", f"--validation_subjects={proj}npy", "--mode=anomaly", f"--anomaly_codes={proj}heal", *SCORES,
                       f"--anomaly_mask={proj}masks"]))
    rows = _rows(out)
    assert list(rows[0]) == ["subject", "sum", "max"] + FILTERED
    brain = np.load(f"{proj}masks/s0.npy") > 0.5
    for name, row in zip(NAMES, rows):
        raw = np.load(f"{out}{name}/{name}_anomaly_map.npy")
        want = np.where(brain, raw, np.float32(0))
        assert np.load(f"{out}{name}/{name}_anomaly_map_filtered.npy").view(np.int32).tobytes() == want.view(np.int32).tobytes()
        _check_filtered_columns(row, want, None)


@pytest.mark.parametrize("extra, match", [
    (["--anomaly_median=4"], "--anomaly_median=4"),
    (["--anomaly_median=3", "--anomaly_mask_erosion=1"], r"--anomaly_mask_erosion=1.*--anomaly_mask"),
    (["--anomaly_mask=masks", "--anomaly_mask_threshold=0.5"], r"--anomaly_mask_threshold=0.5.*--anomaly_mask=scan"),
    (["--anomaly_median=3", "--mode=decoding"], r"--anomaly_median=3.*--mode=anomaly"),
])
def test_each_refusal_names_its_flag_before_the_network_is_built(work, extra, match, monkeypatch):
    import run_vqvae
    from synthanatomy_amd import _ffi
    proj, out, before, header, scans = work

    def built(*a, **k):
        raise AssertionError("the network was built")
    monkeypatch.setattr(run_vqvae, "build_network", built)
    listing = _listing(out)
    with _ffi.kernel_log() as launched:
        with pytest.raises(ValueError, match=match):
            _run(_flags(proj, [f"--training_subjects={proj}npy", f"--validation_subjects={proj}npy", "--mode=anomaly", f"--anomaly_codes={proj}heal", *extra]))
    assert launched == [] and _listing(out) == listing


def test_a_subject_without_its_mask_volume_is_refused_by_name_before_the_network_is_built(work, monkeypatch):
    import run_vqvae
    proj, out, before, header, scans = work
    os.makedirs(proj + "masks_one", exist_ok=True)
    np.save(f"{proj}masks_one/s0.npy", np.ones(SIDE, dtype=np.float32))
    monkeypatch.setattr(run_vqvae, "build_network", lambda *a, **k: (_ for _ in ()).throw(AssertionError("the network was built")))
    with pytest.raises(ValueError, match=r"s1.*0 mask volumes.*--anomaly_mask="):
        _run(_flags(proj, [f"--training_subjects={proj}npy", f"--validation_subjects={proj}npy", "--mode=anomaly", f"--anomaly_codes={proj}heal",
                           f"--anomaly_mask={proj}masks_one"]))
