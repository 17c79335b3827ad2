"""GPU: ``run_vqvae.py --mode=anomaly`` end to end with a randomly initialised two-level VQ-VAE (factor 4) on two 16 x 16 x 16 subjects:
extraction writes the codes, ``run_transformer.save_healing`` writes healed codes with a planted block of changed entries, its mask and an NLL grid, label
volumes cover the block, and the anomaly stage must write the map ``anomaly_map`` gives for the same tensors, the healed reconstruction and the scores.
One run reads the same subjects from NIfTI files in a non-canonical orientation and writes ``.nii``: the outputs come back in the source's axes."""
import contextlib
import csv
import io
import os

import numpy as np
import pytest

import anomaly_ref
from nifti_ref import signed_perm_affine, write_nifti

pytestmark = pytest.mark.gpu

SIDE, LATENT = (16, 16, 16), (4, 4, 4)
BLOCK = (slice(1, 3),) * 3            # the planted latent block: voxels 4..11 on every axis
PERM, SIGN = (2, 0, 1), (-1, 1, -1)   # how the NIfTI copies are stored
NAMES = ("s0", "s1")


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


@pytest.fixture(scope="module")
def work(tmp_path_factory):
    import torch
    import run_transformer
    import run_vqvae
    from synthanatomy_amd.utils.general import parse_flags
    proj = str(tmp_path_factory.mktemp("anomaly_cli")) + "/"
    for d in ("npy", "nii", "labels", "labels_nii", "healed"):
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
        write_nifti(f"{proj}labels_nii/{name}.nii.gz", _stored(label, PERM, SIGN), sform=signed_perm_affine(PERM, SIGN))
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
    net.load_state_dict(sd)
    out = proj + "fixed/baseline_vqvae/outputs/"
    _run(_flags(proj, sub + ["--mode=extracting"]))
    healed = {}
    for name in NAMES:
        codes = np.load(f"{out}{name}/{name}_quantization_0.npy")
        assert codes.shape == LATENT and codes.dtype == np.uint16
        new = codes.copy()
        new[BLOCK] = (codes[BLOCK] + 1 + rng.integers(0, 62, size=(2, 2, 2))) % 64      # every entry of the block changes
        mask = np.zeros(LATENT, dtype=bool)
        mask[BLOCK] = True
        assert np.array_equal(new != codes, mask)
        nll = rng.exponential(1.0, LATENT).astype(np.float32)
        run_transformer.save_healing(new, nll, mask, proj + "healed/", f"{out}{name}/{name}_quantization_0.npy")
        healed[name] = (new, nll, mask)
    return proj, out, net, cfg, healed


def _direct(net, cfg, paths, healed, weight, sigma, labels, **kw):
    """anomaly_map called on the tensors the CLI builds"""
    import torch
    import run_vqvae
    from synthanatomy_amd.metrics.anomaly import anomaly_map
    dev = torch.device("cuda", 0)
    x = torch.stack([run_vqvae._load_volume(p, cfg, None, dev) for p in paths])
    with torch.no_grad():
        rec = net.decode_samples([torch.stack([torch.from_numpy(healed[n][0].astype(np.int64)) for n in NAMES]).to(dev)]).float()
    w = None if weight is None else torch.stack([torch.from_numpy(healed[n][weight].astype(np.float32)) for n in NAMES]).to(dev)
    amap, s = anomaly_map(x, rec, w, sigma=sigma, labels=labels, **kw)
    return amap.cpu().numpy()[:, 0], rec.cpu().numpy()[:, 0], s


def test_npy_subjects_mask_weight_labels_and_scores(work):
    import torch
    from synthanatomy_amd.metrics.anomaly import average_precision, best_dice, dice_from_counts, gaussian_taps
    proj, out, net, cfg, healed = work
    _run(_flags(proj, [f"--training_subjects={proj}npy", f"--validation_subjects={proj}npy", "--mode=anomaly", f"--anomaly_codes={proj}healed",
                       f"--anomaly_labels={proj}labels", "--anomaly_sigma=0.5", "--anomaly_threshold=0.002", "--anomaly_hist_max=0.25"]))
    label = torch.from_numpy((np.load(f"{proj}labels/s0.npy") > 0.5)).to("cuda:0")[None, None].expand(2, 1, *SIDE)
    amap, rec, s = _direct(net, cfg, [f"{proj}npy/{n}.npy" for n in NAMES], healed, 2, 0.5, label, threshold=0.002, hist_max=0.25)
    w = anomaly_ref.weight_ref(healed["s0"][2].astype(np.float32), SIDE, gaussian_taps(0.5))
    assert (w == 0).sum() > 1000 and (w > 0).sum() > 1000      # sigma 0.5: R = 2, the block's voxels 4..11 reach 2..13
    for j, name in enumerate(NAMES):
        got = np.load(f"{out}{name}/{name}_anomaly_map.npy")
        assert got.shape == SIDE and got.dtype == np.float32 and got.tobytes() == amap[j].tobytes()
        hr = np.load(f"{out}{name}/{name}_healed_reconstruction.npy")
        assert hr.shape == SIDE and hr.dtype == np.float32 and hr.tobytes() == rec[j].tobytes()
        assert not got[w == 0].any() and got[w > 0].max() > 0
        assert not np.array_equal(hr, np.load(f"{out}{name}/{name}_reconstruction.npy"))      # the planted block changed the decoding
    with open(out + "anomaly_scores_rank0.csv", newline="") as f:
        rows = list(csv.DictReader(f))
    assert [r["subject"] for r in rows] == list(NAMES)
    assert list(rows[0]) == ["subject", "sum", "max", "dice", "best_dice", "best_dice_threshold", "average_precision"]
    hist, counts = s["hist"].cpu().numpy(), [s[k].cpu().numpy() for k in ("tp", "fp", "fn")]
    for j, r in enumerate(rows):
        assert float(r["sum"]) == float(s["sum"][j]) > 0 and float(r["max"]) == float(s["max"][j]) > 0
        assert float(r["dice"]) == dice_from_counts(counts[0][j], counts[1][j], counts[2][j]) > 0
        assert (float(r["best_dice"]), float(r["best_dice_threshold"])) == best_dice(hist[j, 0], hist[j, 1], s["inv_bin"])
        assert float(r["average_precision"]) == average_precision(hist[j, 0], hist[j, 1])
        assert 0 < float(r["best_dice"]) <= 1 and 0 < float(r["average_precision"]) <= 1


def test_nifti_subjects_default_sigma_and_nifti_outputs_in_the_sources_axes(work, tmp_path):
    from synthanatomy_amd.utils.nifti import header_orientation, read_nifti
    from synthanatomy_amd.utils.vqvae import hip_ingest
    proj, out, net, cfg, healed = work
    _run(_flags(proj, [f"--training_subjects={proj}nii", f"--validation_subjects={proj}nii", "--mode=anomaly", f"--anomaly_codes={proj}healed/*",
                       "--anomaly_weight=nll", "--anomaly_residual=positive", "--output_ext=.nii"]))
    amap, rec, s = _direct(net, cfg, [f"{proj}nii/{n}.nii" for n in NAMES], healed, 1, 2.0, None, residual="positive")      # None: factor 4 / 2
    src = read_nifti(f"{proj}nii/s0.nii")[0]
    for j, name in enumerate(NAMES):
        for post, want in (("anomaly_map", amap[j]), ("healed_reconstruction", rec[j])):
            header, raw = read_nifti(f"{out}{name}/{name}_{post}.nii")
            assert header.datatype == 16 and header_orientation(header, True) == (list(PERM), list(SIGN))
            assert np.allclose(header.affine, src.affine, rtol=0, atol=1e-5)      # the whole volume is the ROI: the source's own affine
            back = hip_ingest(header, raw, None, normalize=False, canonical=True, device="cuda:0")[0].cpu().numpy()
            assert back.shape == SIDE and back.tobytes() == want.tobytes(), (name, post)
    with open(out + "anomaly_scores_rank0.csv", newline="") as f:
        rows = list(csv.DictReader(f))
    assert [r["subject"] for r in rows] == list(NAMES) and list(rows[0]) == ["subject", "sum", "max"]
    assert [float(r["sum"]) for r in rows] == [float(v) for v in s["sum"]]


def test_nifti_labels_take_the_scans_reorientation(work):
    import torch
    proj, out, net, cfg, healed = work
    _run(_flags(proj, [f"--training_subjects={proj}nii", f"--validation_subjects={proj}nii", "--mode=anomaly", f"--anomaly_codes={proj}healed",
                       f"--anomaly_labels={proj}labels_nii", "--anomaly_weight=none", "--anomaly_threshold=0.01"]))
    label = torch.from_numpy((np.load(f"{proj}labels/s0.npy") > 0.5)).to("cuda:0")[None, None].expand(2, 1, *SIDE)
    amap, _, s = _direct(net, cfg, [f"{proj}nii/{n}.nii" for n in NAMES], healed, None, 0.0, label, threshold=0.01)
    with open(out + "anomaly_scores_rank0.csv", newline="") as f:
        rows = list(csv.DictReader(f))
    hist = s["hist"].cpu().numpy()
    from synthanatomy_amd.metrics.anomaly import average_precision
    for j, r in enumerate(rows):
        assert np.load(f"{out}{NAMES[j]}/{NAMES[j]}_anomaly_map.npy").tobytes() == amap[j].tobytes()
        assert hist[j, 1].sum() == 8 ** 3 and float(r["average_precision"]) == average_precision(hist[j, 0], hist[j, 1])


def test_a_subject_without_healing_files_is_refused_by_name_before_any_launch(work):
    from synthanatomy_amd import _ffi
    proj, out, net, cfg, healed = work
    os.makedirs(proj + "more", exist_ok=True)
    for name in ("s0", "s7"):
        np.save(f"{proj}more/{name}.npy", np.zeros(SIDE, dtype=np.float32))
    before = sorted(os.listdir(out))
    with _ffi.kernel_log() as launched:
        with pytest.raises(ValueError, match=r"s7\.npy: no healing output s7_quantization_0_healed_sample\.npy"):
            _run(_flags(proj, [f"--training_subjects={proj}more", f"--validation_subjects={proj}more", "--mode=anomaly", f"--anomaly_codes={proj}healed"]))
    assert launched == [] and sorted(os.listdir(out)) == before
