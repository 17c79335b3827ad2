"""GPU: ``run_vqvae.py`` on NIfTI inputs with the small network and ROI of tests/test_augment_cli_gpu.py.  The same canonical data stored
as ``.npy`` and as deliberately non-canonical ``.nii.gz`` gives the same codes and reconstructions; the ROI crop runs as the kernel's window; a training
run works on a NIfTI directory; ``--load_nii_canonical=False`` changes what the network sees."""
import contextlib
import glob
import io
import os
import re

import numpy as np
import pytest

from nifti_ref import signed_perm_affine, write_nifti

pytestmark = pytest.mark.gpu

PERM, SIGN = (2, 0, 1), (-1, -1, 1)      # stored LPS with the file axes rotated: canonical axis a reads file axis PERM[a]


def _flags(proj, exp, extra=()):
    return ["--project_directory=" + proj, "--experiment_name=" + exp, "--no_levels=2", "--downsample_parameters=((4,2,1,1),(4,2,1,1))",
            "--upsample_parameters=((4,2,1,0,1),(4,2,1,0,1))", "--no_channels=32", "--num_embeddings=(64,)", "--embedding_dim=(16,)", "--decay=(0.5,)",
            "--roi=((0,32),(0,32),(0,32))", "--batch_size=2", "--eval_batch_size=2", "--learning_rate=1e-3", "--gamma=0.9", "--amp=False", "--eval_every=1",
            *extra]


def _stored(canonical, perm=PERM, sign=SIGN):
    """The array a file with orientation (perm, sign) stores for the canonical array."""
    v = canonical
    for a in range(3):
        if sign[a] < 0:
            v = np.flip(v, axis=a)
    return np.ascontiguousarray(np.transpose(v, np.argsort(perm)))


def _subject(rng, dims, top):
    """A smooth volume without any symmetry plus a little noise, in [0, top]: position matters, so a reorientation changes the codes."""
    x, y, z = np.meshgrid(*(np.arange(n, dtype=np.float64) for n in dims), indexing="ij")
    k, phase = rng.integers(1, 4, 3), rng.uniform(0, 2 * np.pi, 3)
    v = 0.5 + 0.2 * np.sin(2 * np.pi * k[0] * x / dims[0] + phase[0]) + 0.15 * np.cos(2 * np.pi * k[1] * y / dims[1] + phase[1]) * (z / dims[2])
    v += 0.1 * (x / dims[0]) * np.sin(2 * np.pi * k[2] * z / dims[2] + phase[2]) + 0.02 * rng.standard_normal(dims)
    return np.clip(v, 0, 1) * top


def _run(argv):
    import run_vqvae
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        run_vqvae.run(argv)
    return out.getvalue()


def _outputs(proj, exp, names):
    out = f"{proj}{exp}/baseline_vqvae/outputs/"
    return ([np.load(f"{out}{n}/{n}_quantization_0.npy") for n in names], [np.load(f"{out}{n}/{n}_reconstruction.npy") for n in names])


@pytest.fixture(scope="module")
def work(tmp_path_factory):
    """Four subjects, written as .npy and as .nii.gz (int16 with a slope, LPS, axes permuted), and one epoch of training on the NIfTI directory."""
    root = tmp_path_factory.mktemp("nifti_cli")
    proj = str(root) + "/"
    rng = np.random.default_rng(0)
    for d in ("npy", "nii", "big_npy", "big_nii"):
        os.mkdir(proj + d)
    for s in range(4):
        q = np.round(_subject(rng, (32, 32, 32), 4000)).astype(np.int16)
        np.save(f"{proj}npy/s{s}.npy", q.astype(np.float32) * np.float32(0.25) - np.float32(8))      # exact in fp32, as the scaled file's voxels are
        write_nifti(f"{proj}nii/s{s}.nii.gz", _stored(q), slope=0.25, inter=-8.0, sform=signed_perm_affine(PERM, SIGN))
        big = _subject(rng, (40, 36, 34), 1).astype(np.float32)
        np.save(f"{proj}big_npy/b{s}.npy", big[4:36, 2:34, 1:33])
        write_nifti(f"{proj}big_nii/b{s}.nii", _stored(big), big_endian=bool(s % 2), sform=signed_perm_affine(PERM, SIGN))
    log = _run(_flags(proj, "exp", [f"--training_subjects={proj}nii", f"--validation_subjects={proj}nii", "--mode=training", "--epochs=1"]))
    _fixed_checkpoint(proj)
    return proj, log


def _fixed_checkpoint(proj):
    """The one fixed checkpoint of the extraction cases, experiment ``fixed``: the network of the training run above with a codebook of 64 of its own
    encoder outputs on the four subjects (every 32nd latent position).  A network two iterations old maps every position to one code; with this codebook
    the code grids depend on the position, so equal grids mean equal inputs and a reorientation shows."""
    import torch
    import run_vqvae
    from synthanatomy_amd.utils.general import load_network_state, parse_flags
    cfg = parse_flags(_flags(proj, "exp", [f"--training_subjects={proj}npy", f"--validation_subjects={proj}npy", "--mode=extracting"]), run_vqvae.DEFAULTS)
    dev = torch.device("cuda", 0)
    net = run_vqvae.build_network(cfg, dev).eval()
    load_network_state(net, glob.glob(proj + "exp/baseline_vqvae/checkpoints/checkpoint_epoch=1.pt")[0])
    x = torch.stack([run_vqvae._load_volume(f"{proj}npy/s{s}.npy", cfg, None, dev) for s in range(4)])
    with torch.no_grad():
        z = net.encode(x)[0].float()
    book = z.movedim(1, -1).reshape(-1, z.shape[1])[::32][:64].contiguous()
    assert book.shape == (64, 16) and len({r.tobytes() for r in book.cpu().numpy()}) == 64
    sd = {k: v.clone() for k, v in net.state_dict().items()}
    keys = [k for k in sd if k.endswith(("impl.weight", "impl.embedding.weight", "impl.embed_avg"))]
    assert len(keys) == 3
    for k in keys:
        sd[k] = book.clone()
    os.makedirs(proj + "fixed/baseline_vqvae/checkpoints")
    torch.save({"network": sd}, proj + "fixed/baseline_vqvae/checkpoints/checkpoint_epoch=1.pt")


def test_training_on_a_nifti_directory_logs_a_finite_loss_and_writes_a_checkpoint(work):
    proj, log = work
    losses = [float(m.group(1)) for m in re.finditer(r"^epoch 0 it \d+ loss (\S+)", log, flags=re.M)]
    assert len(losses) == 2 and all(np.isfinite(v) for v in losses)
    assert re.search(r"^epoch 0 validation mse \S+", log, flags=re.M)
    assert glob.glob(proj + "exp/baseline_vqvae/checkpoints/checkpoint_epoch=1.pt")


def test_same_canonical_data_in_different_storage_gives_the_same_codes(work):
    proj, _ = work
    names = [f"s{s}" for s in range(4)]
    _run(_flags(proj, "fixed", [f"--training_subjects={proj}npy", f"--validation_subjects={proj}npy", "--mode=extracting"]))
    codes_npy, recs_npy = _outputs(proj, "fixed", names)
    _run(_flags(proj, "fixed", [f"--training_subjects={proj}nii", f"--validation_subjects={proj}nii", "--mode=extracting", "--num_workers=0"]))
    codes_nii, recs_nii = _outputs(proj, "fixed", names)
    assert all(c.shape == (8, 8, 8) and c.dtype == np.uint16 for c in codes_nii)
    assert len({c.tobytes() for c in codes_nii}) == 4
    for a, b in zip(codes_npy, codes_nii):
        assert np.array_equal(a, b)
    # the normalisation differs by 0 ulp between the host expression and the kernel (tests/test_ingest_gpu.py), so the networks saw the same bits
    print("reconstruction: max difference", max(float(np.abs(a - b).max()) for a, b in zip(recs_npy, recs_nii)))
    for a, b in zip(recs_npy, recs_nii):
        assert np.array_equal(a, b)


def test_roi_crop_of_larger_files_is_the_kernels_window(work):
    proj, _ = work
    names = [f"b{s}" for s in range(4)]
    roi = ["--roi=((4,36),(2,34),(1,33))", "--normalize=False", "--mode=extracting"]
    _run(_flags(proj, "fixed", [f"--training_subjects={proj}big_nii", f"--validation_subjects={proj}big_nii", *roi]))
    codes_nii, recs_nii = _outputs(proj, "fixed", names)
    # the .npy files hold the crop already; their path does not crop, so the ROI flag only has to name a window of that size
    _run(_flags(proj, "fixed", [f"--training_subjects={proj}big_npy", f"--validation_subjects={proj}big_npy", *roi]))
    codes_npy, recs_npy = _outputs(proj, "fixed", names)
    assert all(len(np.unique(c)) > 1 for c in codes_nii) and len({c.tobytes() for c in codes_nii}) == 4
    for a, b in zip(codes_npy, codes_nii):
        assert np.array_equal(a, b)
    for a, b in zip(recs_npy, recs_nii):
        assert np.array_equal(a, b)


def test_load_nii_canonical_false_trains_and_extracts_on_the_stored_order(work):
    proj, log = work
    stored = [f"--training_subjects={proj}nii", f"--validation_subjects={proj}nii", "--load_nii_canonical=False"]
    log_stored = _run(_flags(proj, "stored", [*stored, "--mode=training", "--epochs=1"]))
    first = [re.search(r"^epoch 0 it 1 loss (\S+)", l, flags=re.M).group(1) for l in (log, log_stored)]
    assert all(np.isfinite(float(v)) for v in first) and first[0] != first[1]
    names = [f"s{s}" for s in range(4)]
    _run(_flags(proj, "fixed", [f"--training_subjects={proj}nii", f"--validation_subjects={proj}nii", "--mode=extracting"]))
    canonical, _ = _outputs(proj, "fixed", names)
    _run(_flags(proj, "fixed", [*stored, "--mode=extracting"]))      # the same checkpoint on the stored order
    stored_order_codes, _ = _outputs(proj, "fixed", names)
    assert all(not np.array_equal(a, b) for a, b in zip(canonical, stored_order_codes))
