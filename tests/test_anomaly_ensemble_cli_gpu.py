"""GPU: ``run_vqvae.py --mode=anomaly --anomaly_ensemble=<dirA>,<dirB>,<dirC>`` end to end, in the manner of tests/test_anomaly_cli_gpu.py: a
randomly initialised two-level VQ-VAE (factor 4) with its own encoder outputs as the codebook, two 16 x 16 x 16 subjects, and three healing directories
written by ``run_transformer.save_healing``, each with another planted block and mask.  Single mode runs once per directory and its files are kept; the
ensemble run must write the fp32 composition of the three single-run maps bit for bit, every member's healed reconstruction as the single run wrote it,
and scores that follow from the written map.  One run reads NIfTI subjects in a non-canonical orientation and writes ``.nii``."""
import contextlib
import csv
import io
import os

import numpy as np
import pytest

import anomaly_ensemble_ref as ER
import anomaly_ref
from nifti_ref import signed_perm_affine, write_nifti

pytestmark = pytest.mark.gpu

SIDE, LATENT = (16, 16, 16), (4, 4, 4)
BLOCKS = ((slice(1, 3),) * 3, (slice(0, 2), slice(1, 3), slice(2, 4)), (slice(2, 4), slice(0, 2), slice(1, 3)))      # one planted latent block per member
PERM, SIGN = (2, 0, 1), (-1, 1, -1)   # how the NIfTI copies are stored
NAMES = ("s0", "s1")
MEMBERS = ("healA", "healB", "healC")
SCORES = ["--anomaly_sigma=0.5", "--anomaly_threshold=0.002", "--anomaly_hist_max=0.25"]


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


@pytest.fixture(scope="module")
def work(tmp_path_factory):
    """(project, outputs, per member and subject the single run's map and healed reconstruction) after extraction, the three planted healings and one
    single-mode run per healing directory"""
    import torch
    import run_transformer
    import run_vqvae
    from synthanatomy_amd.utils.general import parse_flags
    proj = str(tmp_path_factory.mktemp("anomaly_ensemble_cli")) + "/"
    for d in ("npy", "nii", "labels", *MEMBERS):
        os.mkdir(proj + d)
    rng = np.random.default_rng(0)
    label = np.zeros(SIDE, dtype=np.float32)
    label[4:12, 4:12, 4:12] = 1.0
    for name in NAMES:
        x, y, z = np.meshgrid(*(np.arange(n) / n for n in SIDE), indexing="ij")
        v = (0.5 + 0.3 * np.sin(5 * x + 1) * np.cos(3 * y) + 0.2 * z * x + 0.05 * rng.standard_normal(SIDE)).astype(np.float32)
        np.save(f"{proj}npy/{name}.npy", v)
        np.save(f"{proj}labels/{name}.npy", label * 3.0)      # labels are not normalised: class 1 where > 0.5
        write_nifti(f"{proj}nii/{name}.nii", _stored(v, PERM, SIGN), sform=signed_perm_affine(PERM, SIGN))
    sub = [f"--training_subjects={proj}npy", f"--validation_subjects={proj}npy"]
    cfg = parse_flags(_flags(proj, sub + ["--mode=extracting"]), run_vqvae.DEFAULTS)
    torch.manual_seed(0)
    dev = torch.device("cuda", 0)
    net = run_vqvae.build_network(cfg, dev).eval()
    # an untrained network maps every position to one code: 64 of its own encoder outputs as the codebook make the codes depend on the position
    x = torch.stack([run_vqvae._load_volume(f"{proj}npy/{name}.npy", cfg, None, dev) for name in NAMES])
    with torch.no_grad():
        z = net.encode(x)[0].float()
    book = z.movedim(1, -1).reshape(-1, z.shape[1])[::2][:64].contiguous()
    assert book.shape == (64, 16)
    sd = {k: v.clone() for k, v in net.state_dict().items()}
    keys = [k for k in sd if k.endswith(("impl.weight", "impl.embedding.weight", "impl.embed_avg"))]
    assert len(keys) == 3
    for k in keys:
        sd[k] = book.clone()
    os.makedirs(proj + "fixed/baseline_vqvae/checkpoints")
    torch.save({"network": sd}, proj + "fixed/baseline_vqvae/checkpoints/checkpoint_epoch=1.pt")
    out = proj + "fixed/baseline_vqvae/outputs/"
    _run(_flags(proj, sub + ["--mode=extracting"]))
    for member, block in zip(MEMBERS, BLOCKS):
        for name in NAMES:
            codes = np.load(f"{out}{name}/{name}_quantization_0.npy")
            assert codes.shape == LATENT and codes.dtype == np.uint16
            new = codes.copy()
            new[block] = (codes[block] + 1 + rng.integers(0, 62, size=(2, 2, 2))) % 64      # every entry of the block changes
            mask = np.zeros(LATENT, dtype=bool)
            mask[block] = True
            run_transformer.save_healing(new, rng.exponential(1.0, LATENT).astype(np.float32), mask, f"{proj}{member}/", f"{out}{name}/{name}_quantization_0.npy")
    single = {}
    for member in MEMBERS:
        _run(_flags(proj, sub + ["--mode=anomaly", f"--anomaly_codes={proj}{member}", f"--anomaly_labels={proj}labels", *SCORES]))
        assert "members" not in _rows(out)[0]      # without the flag the CSV keeps its columns
        for name in NAMES:
            single[member, name] = (np.load(f"{out}{name}/{name}_anomaly_map.npy"), np.load(f"{out}{name}/{name}_healed_reconstruction.npy"))
    assert not np.array_equal(single["healA", "s0"][0], single["healB", "s0"][0])
    return proj, out, single


def _spec(proj):
    return "--anomaly_ensemble=" + ",".join(proj + member for member in MEMBERS)


def test_npy_subjects_the_map_the_members_reconstructions_and_the_scores(work):
    from synthanatomy_amd.metrics.anomaly import average_precision, best_dice, dice_from_counts
    proj, out, single = work
    _run(_flags(proj, [f"--training_subjects={proj}npy", f"--validation_subjects={proj}npy", "--mode=anomaly", _spec(proj), f"--anomaly_labels={proj}labels",
                       *SCORES]))
    rows = _rows(out)
    assert [r["subject"] for r in rows] == list(NAMES)
    assert list(rows[0]) == ["subject", "sum", "max", "dice", "best_dice", "best_dice_threshold", "average_precision", "members"]
    label = np.load(f"{proj}labels/s0.npy") > 0.5
    inv_bin = np.float32(256.0 / 0.25)
    for name, row in zip(NAMES, rows):
        got = np.load(f"{out}{name}/{name}_anomaly_map.npy")
        assert got.shape == SIDE and got.dtype == np.float32
        assert got.tobytes() == ER.compose_fp32([single[member, name][0] for member in MEMBERS]).tobytes()
        for k, member in enumerate(MEMBERS):
            hr = np.load(f"{out}{name}/{name}_healed_reconstruction_m{k}.npy")
            assert hr.dtype == np.float32 and hr.tobytes() == single[member, name][1].tobytes(), (name, k)
        assert not os.path.exists(f"{out}{name}/{name}_healed_reconstruction_m3.npy")
        # the scores follow from the written map and the label
        assert row["members"] == "3"
        hist = anomaly_ref.histograms(got, label, inv_bin)
        tp, fp, fn = anomaly_ref.counts(got, label, np.float32(0.002))
        assert float(row["max"]) == float(got.max()) > 0
        exact = float(np.sum(got.astype(np.float64)))
        assert abs(float(row["sum"]) - exact) <= 1e-12 * exact
        assert float(row["dice"]) == dice_from_counts(tp, fp, fn) > 0
        assert (float(row["best_dice"]), float(row["best_dice_threshold"])) == best_dice(hist[0], hist[1], inv_bin)
        assert float(row["average_precision"]) == average_precision(hist[0], hist[1]) > 0


def test_the_flag_with_anomaly_codes_is_refused_before_the_network_is_built(work, monkeypatch):
    import run_vqvae
    from synthanatomy_amd import _ffi
    proj, out, _ = work

    def built(*a, **k):
        raise AssertionError("the network was built")
    monkeypatch.setattr(run_vqvae, "build_network", built)
    before = sorted(os.listdir(out + "s0"))
    with _ffi.kernel_log() as launched:
        with pytest.raises(ValueError, match=r"--anomaly_ensemble=.*healA.* with --anomaly_codes="):
            _run(_flags(proj, [f"--training_subjects={proj}npy", f"--validation_subjects={proj}npy", "--mode=anomaly", _spec(proj),
                               f"--anomaly_codes={proj}healA"]))
    assert launched == [] and sorted(os.listdir(out + "s0")) == before


def test_nifti_subjects_and_nifti_outputs_in_the_sources_axes(work):
    from synthanatomy_amd.utils.nifti import header_orientation, read_nifti
    from synthanatomy_amd.utils.vqvae import hip_ingest
    proj, out, single = work
    argv = _flags(proj, [f"--training_subjects={proj}nii", f"--validation_subjects={proj}nii", "--mode=anomaly", _spec(proj), "--anomaly_sigma=0.5"])
    _run(argv)      # the same subjects and members with .npy outputs: the map in canonical axes (the scan went through the NIfTI ingest)
    maps = {name: np.load(f"{out}{name}/{name}_anomaly_map.npy") for name in NAMES}
    _run(argv + ["--output_ext=.nii"])
    src = read_nifti(f"{proj}nii/s0.nii")[0]
    for name in NAMES:
        want = {"anomaly_map": maps[name]}
        assert maps[name].any()
        want.update({f"healed_reconstruction_m{k}": single[member, name][1] for k, member in enumerate(MEMBERS)})
        for post, canonical in want.items():
            header, raw = read_nifti(f"{out}{name}/{name}_{post}.nii")
            assert header.datatype == 16 and header_orientation(header, True) == (list(PERM), list(SIGN))
            assert np.allclose(header.affine, src.affine, rtol=0, atol=1e-5)      # the whole volume is the ROI: the source's own affine
            back = hip_ingest(header, raw, None, normalize=False, canonical=True, device="cuda:0")[0].cpu().numpy()
            assert back.shape == SIDE and back.tobytes() == canonical.tobytes(), (name, post)
    rows = _rows(out)
    assert list(rows[0]) == ["subject", "sum", "max", "members"] and [r["members"] for r in rows] == ["3", "3"]
