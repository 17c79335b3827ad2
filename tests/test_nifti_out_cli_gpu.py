"""GPU: ``run_vqvae.py --output_ext / --output_dtype`` with the small network of tests/test_nifti_cli_gpu.py and a 32 x 24 x 16 ROI that really
crops.  Extraction over three NIfTI subjects stored in three non-canonical orientations writes each reconstruction back in its SOURCE's axes with an
affine that puts it where the source has those voxels; decoding from ``.npy`` code grids writes identity-oriented samples.  One untrained network with a
codebook of its own encoder outputs, saved once as the experiment's checkpoint, serves every run: the comparisons are between output formats of the same
network."""
import contextlib
import io
import os
import shutil

import numpy as np
import pytest

from nifti_out_ref import ulp32
from nifti_ref import signed_perm_affine, write_nifti

pytestmark = pytest.mark.gpu

ROI = ((4, 36), (2, 26), (1, 17))
SIZE = (32, 24, 16)
START = (4, 2, 1)
SUBJECTS = [("s0", (40, 30, 20), (2, 0, 1), (-1, -1, 1), ".nii.gz"), ("s1", (38, 28, 22), (1, 0, 2), (1, -1, -1), ".nii"),
            ("s2", (36, 32, 18), (0, 2, 1), (-1, 1, 1), ".nii")]      # name, canonical dims, perm, sign, container


def _flags(proj, extra=()):
    return ["--project_directory=" + proj, "--experiment_name=fixed", "--no_levels=2", "--downsample_parameters=((4,2,1,1),(4,2,1,1))",
            "--upsample_parameters=((4,2,1,0,1),(4,2,1,0,1))", "--no_channels=32", "--num_embeddings=(64,)", "--embedding_dim=(16,)", "--decay=(0.5,)",
            f"--roi={ROI}".replace(" ", ""), "--batch_size=2", "--eval_batch_size=2", "--amp=False", *extra]


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


def _files(directory):
    return {os.path.relpath(os.path.join(d, f), directory): open(os.path.join(d, f), "rb").read() for d, _, fs in os.walk(directory) for f in fs}


@pytest.fixture(scope="module")
def work(tmp_path_factory):
    import torch
    import run_vqvae
    from synthanatomy_amd.utils.general import parse_flags
    proj = str(tmp_path_factory.mktemp("nifti_out_cli")) + "/"
    os.mkdir(proj + "nii")
    rng = np.random.default_rng(0)
    for name, dims, perm, sign, ext in SUBJECTS:
        x, y, z = np.meshgrid(*(np.arange(n) / n for n in dims), indexing="ij")
        v = (0.5 + 0.3 * np.sin(5 * x + 1) * np.cos(3 * y) + 0.2 * z * x + 0.05 * rng.standard_normal(dims)).astype(np.float32)
        write_nifti(f"{proj}nii/{name}{ext}", _stored(v, perm, sign), sform=signed_perm_affine(perm, sign))
    sub = [f"--training_subjects={proj}nii", f"--validation_subjects={proj}nii", "--mode=extracting"]
    cfg = parse_flags(_flags(proj, sub), run_vqvae.DEFAULTS)
    torch.manual_seed(0)
    dev = torch.device("cuda", 0)
    net = run_vqvae.build_network(cfg, dev).eval()
    # an untrained network maps every position to one code; with 64 of its own encoder outputs as the codebook (tests/test_nifti_cli_gpu.py) the code grids
    # and the reconstructions depend on the subject and on the position
    x = torch.stack([run_vqvae._load_volume(f"{proj}nii/{name}{ext}", cfg, None, dev) for name, _, _, _, ext in SUBJECTS])
    with torch.no_grad():
        z = net.encode(x)[0].float()
    book = z.movedim(1, -1).reshape(-1, z.shape[1])[::9][:64].contiguous()
    assert book.shape == (64, 16)
    sd = {k: v.clone() for k, v in net.state_dict().items()}
    keys = [k for k in sd if k.endswith(("impl.weight", "impl.embedding.weight", "impl.embed_avg"))]
    assert len(keys) == 3
    for k in keys:
        sd[k] = book.clone()
    os.makedirs(proj + "fixed/baseline_vqvae/checkpoints")
    torch.save({"network": sd}, proj + "fixed/baseline_vqvae/checkpoints/checkpoint_epoch=1.pt")
    out = proj + "fixed/baseline_vqvae/outputs/"
    runs = {}
    for key, extra in (("npy", []), ("gz4", ["--output_ext=.nii.gz", "--num_workers=4"]), ("gz0", ["--output_ext=.nii.gz", "--num_workers=0"])):
        shutil.rmtree(out, ignore_errors=True)
        _run(_flags(proj, sub + extra))
        runs[key] = _files(out)
    os.mkdir(proj + "codes")
    for name, *_ in SUBJECTS:
        with open(f"{proj}codes/{name}_quantization_0.npy", "wb") as f:
            f.write(runs["npy"][f"{name}/{name}_quantization_0.npy"])
    dec = [f"--training_subjects={proj}codes", f"--validation_subjects={proj}codes", "--mode=decoding"]
    for key, extra in (("dec_npy", []), ("dec_nii", ["--output_ext=.nii"]), ("dec_i16", ["--output_ext=.nii", "--output_dtype=int16", "--num_workers=0"])):
        shutil.rmtree(out, ignore_errors=True)
        _run(_flags(proj, dec + extra))
        runs[key] = _files(out)
    return proj, runs


def _npy(blob):
    return np.load(io.BytesIO(blob))


def _parse(blob, tmp_path, name):
    from synthanatomy_amd.utils.nifti import read_nifti
    path = str(tmp_path / name)
    with open(path, "wb") as f:
        f.write(blob)
    return read_nifti(path)


def test_extraction_writes_the_codes_as_before_and_one_nifti_per_subject(work):
    _, runs = work
    names = [s[0] for s in SUBJECTS]
    assert sorted(runs["npy"]) == sorted(f"{n}/{n}_{p}.npy" for n in names for p in ("quantization_0", "reconstruction"))
    assert sorted(runs["gz4"]) == sorted([f"{n}/{n}_quantization_0.npy" for n in names] + [f"{n}/{n}_reconstruction.nii.gz" for n in names])
    for n in names:
        assert runs["gz4"][f"{n}/{n}_quantization_0.npy"] == runs["npy"][f"{n}/{n}_quantization_0.npy"]
        assert _npy(runs["npy"][f"{n}/{n}_quantization_0.npy"]).dtype == np.uint16
    assert len({runs["npy"][f"{n}/{n}_quantization_0.npy"] for n in names}) == 3      # the subjects differ
    assert runs["gz0"] == runs["gz4"]      # byte-identical files whatever the worker count


def test_reconstructions_come_back_bit_for_bit_in_the_sources_axes(work, tmp_path):
    from synthanatomy_amd.utils.nifti import header_orientation, read_nifti
    from synthanatomy_amd.utils.vqvae import hip_ingest
    proj, runs = work
    recs = []
    for name, dims, perm, sign, container in SUBJECTS:
        blob = runs["gz4"][f"{name}/{name}_reconstruction.nii.gz"]
        assert blob[:2] == b"\x1f\x8b"
        header, raw = _parse(blob, tmp_path, name + ".nii.gz")
        want_dims = [0, 0, 0]
        for a in range(3):
            want_dims[perm[a]] = SIZE[a]
        assert header.dims == tuple(want_dims) and header.datatype == 16 and (header.slope, header.inter) == (1.0, 0.0)
        assert header_orientation(header, True) == (list(perm), list(sign))
        back = hip_ingest(header, raw, None, normalize=False, canonical=True, device="cuda:0")[0].cpu().numpy()
        rec = _npy(runs["npy"][f"{name}/{name}_reconstruction.npy"])
        assert rec.shape == SIZE and rec.dtype == np.float32 and back.tobytes() == rec.tobytes()
        recs.append(rec)
        # the affine: the output's voxel (0, 0, 0) and its far corner lie where the source has the voxels they came from
        src = read_nifti(f"{proj}nii/{name}{container}")[0].affine      # computed from the source file's own header
        assert np.array_equal(header.affine[:3, :3], src[:3, :3])
        atol = float(np.spacing(np.float32(np.abs(header.affine[:3, 3]).max())))      # the header stores the new translation as float32: half an ulp of it
        for g in ([0, 0, 0], [n - 1 for n in header.dims]):
            o = [g[perm[a]] if sign[a] > 0 else SIZE[a] - 1 - g[perm[a]] for a in range(3)]      # the window's voxel, canonical axes
            c = [START[a] + o[a] for a in range(3)]                                              # the canonical volume's voxel
            i = [0, 0, 0]
            for a in range(3):
                i[perm[a]] = c[a] if sign[a] > 0 else dims[a] - 1 - c[a]                         # the source file's voxel
            assert np.allclose(header.affine @ [*g, 1.0], src @ [*i, 1.0], rtol=0, atol=atol), (name, g)
    assert len({r.tobytes() for r in recs}) == 3 and all(np.ptp(r) > 0 for r in recs)


def test_decoding_writes_identity_oriented_samples(work, tmp_path):
    _, runs = work
    for name, *_ in SUBJECTS:
        stem = f"{name}_quantization_0/{name}_quantization_0_sample"
        sample = _npy(runs["dec_npy"][stem + ".npy"])
        assert sample.shape == SIZE and sample.dtype == np.float32
        blob = runs["dec_nii"][stem + ".nii"]
        assert blob[:2] != b"\x1f\x8b" and blob[252:256] == b"\0\0\2\0"      # qform_code 0, sform_code 2
        header, raw = _parse(blob, tmp_path, name + ".nii")
        assert header.dims == SIZE and header.datatype == 16 and np.array_equal(header.affine, np.eye(4))
        assert np.frombuffer(raw, dtype="<f4").reshape(SIZE, order="F").tobytes(order="C") == sample.tobytes()
        # int16 with auto-scaling: 0.5 * slope + ulp32(|inter|) + ulp32(max |x|), the bound derived in tests/test_egress_gpu.py
        header, raw = _parse(runs["dec_i16"][stem + ".nii"], tmp_path, name + "_i16.nii")
        assert header.dims == SIZE and header.datatype == 4 and np.array_equal(header.affine, np.eye(4))
        codes = np.frombuffer(raw, dtype="<i2").reshape(SIZE, order="F")
        value = (codes.astype(np.float64) * header.slope + header.inter).astype(np.float32)
        err = float(np.abs(value.astype(np.float64) - sample.astype(np.float64)).max())
        bound = 0.5 * header.slope + ulp32(header.inter) + ulp32(np.abs(sample).max())
        print(f"{name} int16 sample: max error {err:.6g}, bound {bound:.6g}")
        assert err <= bound
        assert codes.min() == -32768 and codes.max() >= 32766
