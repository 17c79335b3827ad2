"""CPU: the NIfTI writer of utils/nifti.py (``output_header``, ``output_affine``, ``write_nifti``), the refusals of ``run_vqvae.py --output_ext /
--output_dtype`` before anything touches the device, and the next stage's directory listing next to the new outputs."""
import builtins
import itertools
import os

import numpy as np
import pytest

from nifti_ref import SIGNED_PERMS, rotation_about, signed_perm_affine


def test_output_header_reads_back_through_parse_header():
    from synthanatomy_amd.utils.nifti import output_header, parse_header
    aff = signed_perm_affine((2, 0, 1), (-1, 1, -1), rotation=rotation_about((1, 2, 3), 9.0))
    for code, slope, inter in ((4, 0.0123, -7.5), (2, 3.0, 0.25), (16, 0.0123, -7.5)):
        blob = output_header((33, 65, 31), code, aff, slope, inter)
        assert len(blob) == 352 and blob[348:] == b"\0\0\0\0" and blob[344:348] == b"n+1\0"
        h = parse_header(blob)
        assert h.dims == (33, 65, 31) and h.datatype == code and not h.byteswap and h.vox_offset == 352
        want = (1.0, 0.0) if code == 16 else (float(np.float32(slope)), float(np.float32(inter)))      # float32: "no scaling"
        assert (h.slope, h.inter) == want
        assert np.array_equal(h.affine[:3], aff[:3].astype(np.float32).astype(np.float64)) and np.array_equal(h.affine[3], [0, 0, 0, 1])
    import struct
    assert struct.unpack("<i", blob[:4]) == (348,) and struct.unpack("<8h", blob[40:56]) == (3, 33, 65, 31, 1, 1, 1, 1)
    assert struct.unpack("<2h", blob[70:74]) == (16, 32) and struct.unpack("<3f", blob[108:120]) == (352.0, 0.0, 0.0)
    assert np.allclose(struct.unpack("<3f", blob[80:92]), (0.7, 1.0, 2.5), rtol=1e-6)      # pixdim[1..3]: the column norms (signed_perm_affine's zooms)
    assert blob[123] == 2 and struct.unpack("<2h", blob[252:256]) == (0, 2)                 # mm; qform_code 0, sform_code 2
    for bad in (dict(dims=(5, 0, 3)), dict(dims=(5, 40000, 3)), dict(datatype=64), dict(affine=np.eye(3))):
        with pytest.raises(ValueError):
            output_header(**{"dims": (5, 7, 11), "datatype": 16, "affine": np.eye(4), **bad})


def _canonical_to_file(c, perm, sign, n_can):
    """The source-file voxel of canonical voxel c (sa_ingest_params' convention)."""
    i = [0, 0, 0]
    for a in range(3):
        i[perm[a]] = c[a] if sign[a] > 0 else n_can[a] - 1 - c[a]
    return i


def test_output_affine_puts_every_corner_of_the_window_where_the_source_has_it():
    from synthanatomy_amd.utils.nifti import orientation, output_affine
    file_dims, rot = (12, 9, 14), rotation_about((3, -1, 2), 11.0)
    for (perm, sign), rotation in itertools.product(SIGNED_PERMS, (None, rot)):
        src = signed_perm_affine(perm, sign, rotation=rotation)
        assert orientation(src) == (list(perm), list(sign))
        n_can = [file_dims[perm[a]] for a in range(3)]
        start, size = [2, 1, 3], [n_can[0] - 5, n_can[1] - 2, n_can[2] - 7]
        out = output_affine(src, perm, sign, n_can, start, size)
        assert np.array_equal(out[:3, :3], src[:3, :3]) and np.array_equal(out[3], [0, 0, 0, 1])
        for corner in itertools.product((0, 1), repeat=3):
            o = [k * (s - 1) for k, s in zip(corner, size)]                                  # a corner of the window, canonical axes
            g = _canonical_to_file(o, perm, sign, size)                                      # its voxel in the output file
            i = _canonical_to_file([a + b for a, b in zip(start, o)], perm, sign, n_can)     # its voxel in the source file
            assert np.allclose(out @ [*g, 1.0], src @ [*i, 1.0], rtol=0, atol=1e-9), (perm, sign, corner)
    ident = np.eye(4)
    assert np.array_equal(output_affine(ident, (0, 1, 2), (1, 1, 1), (8, 8, 8), (0, 0, 0), (8, 8, 8)), ident)
    assert np.array_equal(output_affine(None, (2, 0, 1), (-1, 1, 1), (8, 9, 10), (1, 2, 3), (4, 4, 4)), ident)
    shifted = output_affine(ident, (0, 1, 2), (1, 1, 1), (8, 8, 8), (1, -2, 3), (4, 12, 4))      # a negative start: the mirror-padded small file
    assert np.array_equal(shifted[:3, 3], [1, -2, 3])


def test_output_geometry_of_a_file_smaller_than_the_roi_starts_before_the_file():
    """A file smaller than the ROI is mirror-padded by the loader (``pad_to_roi``: (w - n) // 2 voxels in front), so the window starts before the file."""
    from nifti_ref import header_bytes
    from synthanatomy_amd.utils.nifti import parse_header
    from synthanatomy_amd.utils.vqvae import nifti_output_geometry, pad_to_roi
    perm, sign, n_can, roi = (2, 0, 1), (-1, 1, -1), (8, 10, 6), (12, 10, 9)
    file_dims = [0, 0, 0]
    for a in range(3):
        file_dims[perm[a]] = n_can[a]
    src = signed_perm_affine(perm, sign, rotation=rotation_about((1, 1, 0), 7.0))
    header = parse_header(header_bytes(file_dims, 16, sform=src))
    got_perm, got_sign, aff = nifti_output_geometry(header, roi, True, roi)
    assert (got_perm, got_sign) == (list(perm), list(sign))
    front = (2, 0, 1)                                                     # (12 - 8) // 2, 0, (9 - 6) // 2: the odd voxel goes behind
    vol = np.arange(8 * 10 * 6, dtype=np.float32).reshape(n_can)
    padded = pad_to_roi(vol, roi)
    assert padded.shape == roi and padded[front] == vol[0, 0, 0] and padded[front[0] + 7, 9, front[2] + 5] == vol[7, 9, 5]
    for c in ((0, 0, 0), (7, 9, 5), (3, 4, 2)):                           # canonical voxels of the file; o = c + front in the padded window
        g = _canonical_to_file([a + b for a, b in zip(c, front)], perm, sign, roi)
        i = _canonical_to_file(c, perm, sign, n_can)
        assert np.allclose(aff @ [*g, 1.0], header.affine @ [*i, 1.0], rtol=0, atol=1e-9), c
    # an ROI of pairs inside a larger file: the window's own start; no header: the identity
    big = parse_header(header_bytes((20, 30, 40), 16, sform=signed_perm_affine((0, 1, 2), (1, 1, 1))))
    _, _, aff = nifti_output_geometry(big, ((2, 10), (3, 19), (5, 37)), True, (8, 16, 32))
    assert np.allclose(aff[:3, 3], big.affine[:3, :3] @ [2, 3, 5] + big.affine[:3, 3], rtol=0, atol=1e-12)
    assert nifti_output_geometry(None, roi, True, roi)[:2] == ([0, 1, 2], [1, 1, 1]) and np.array_equal(nifti_output_geometry(None, roi, True, roi)[2], np.eye(4))


def test_write_nifti_is_reproducible_atomic_and_readable(tmp_path, monkeypatch):
    from synthanatomy_amd.utils import nifti
    block = np.arange(5 * 7 * 11, dtype="<f4")
    header = nifti.output_header((5, 7, 11), 16, np.eye(4))
    for ext, gz in ((".nii", False), (".nii.gz", True)):
        a, b = str(tmp_path / ("a" + ext)), str(tmp_path / ("b" + ext))
        nifti.write_nifti(a, header, block)
        nifti.write_nifti(b, header, memoryview(block.tobytes()))
        blob = open(a, "rb").read()
        assert blob == open(b, "rb").read() and (blob[:2] == b"\x1f\x8b") == gz
        if not gz:
            assert blob == header + block.tobytes()
        h, raw = nifti.read_nifti(a)
        assert h.dims == (5, 7, 11) and raw == block.tobytes()
    assert sorted(os.listdir(tmp_path)) == ["a.nii", "a.nii.gz", "b.nii", "b.nii.gz"]      # no .part file is left behind
    with pytest.raises(ValueError, match="write_nifti"):
        nifti.write_nifti(str(tmp_path / "c.npy"), header, block)

    real_open = builtins.open

    class Failing:
        def __init__(self, f):
            self.f, self.calls = f, 0

        def write(self, data):
            self.calls += 1
            if self.calls > 1:
                raise OSError("disk full")
            return self.f.write(data)

        def __getattr__(self, name):
            return getattr(self.f, name)

        def __enter__(self):
            return self

        def __exit__(self, *exc):
            self.f.close()

    monkeypatch.setattr(builtins, "open", lambda p, mode="r", *a, **k: Failing(real_open(p, mode, *a, **k)) if "w" in mode else real_open(p, mode, *a, **k))
    for ext in (".nii", ".nii.gz"):
        with pytest.raises(OSError, match="disk full"):
            nifti.write_nifti(str(tmp_path / ("d" + ext)), header, block)
    monkeypatch.undo()
    assert sorted(os.listdir(tmp_path)) == ["a.nii", "a.nii.gz", "b.nii", "b.nii.gz"]      # neither the final name nor the .part


def _argv(tmp_path, *extra):
    return ["--training_subjects=synthetic:2", "--validation_subjects=synthetic:2", f"--project_directory={tmp_path}/", "--experiment_name=e", *extra]


def test_output_flags_refuse_before_any_gpu_call(tmp_path, monkeypatch):
    import run_vqvae
    from synthanatomy_amd import _ffi
    from synthanatomy_amd.runtime import ddp
    monkeypatch.setattr(_ffi, "lib", lambda: (_ for _ in ()).throw(AssertionError("a kernel library call before the refusal")))
    monkeypatch.setattr(ddp, "init_distributed", lambda *a, **k: (_ for _ in ()).throw(AssertionError("the process group before the refusal")))
    cases = [(["--mode=decoding", "--output_ext=.mha"], "--output_ext"),
             (["--mode=decoding", "--output_ext=.nii", "--output_dtype=float16"], "--output_dtype"),
             (["--mode=decoding", "--output_dtype=int16"], "--output_dtype"),
             (["--mode=extracting", "--output_dtype=uint8", "--output_ext=.npy"], "--output_dtype"),
             (["--mode=extracting", "--output_ext=.nii.gz", "--no_augmented_extractions=2"], "--output_ext"),
             (["--mode=extracting", "--output_ext=.nii", "--no_augmented_extractions=1", "--output_dtype=int16"], "--no_augmented_extractions"),
             (["--mode=training", "--output_ext=.nii.gz"], "--output_ext")]
    for extra, flag in cases:
        with pytest.raises(ValueError, match=flag):
            run_vqvae.run(_argv(tmp_path, *extra))
    assert not os.listdir(tmp_path)      # nothing was created either


def test_output_flag_defaults_are_unchanged():
    import run_vqvae
    from synthanatomy_amd.utils.general import parse_flags
    assert run_vqvae.DEFAULTS["output_ext"] == ".npy" and run_vqvae.DEFAULTS["output_dtype"] == "float32"
    cfg = parse_flags(_argv("/tmp/x", "--mode=extracting"), run_vqvae.DEFAULTS)
    run_vqvae._check_output_flags(cfg)
    cfg = parse_flags(_argv("/tmp/x", "--mode=decoding", "--output_ext=.nii.gz", "--output_dtype=int16"), run_vqvae.DEFAULTS)
    assert (cfg["output_ext"], cfg["output_dtype"]) == (".nii.gz", "int16")
    run_vqvae._check_output_flags(cfg)
    cfg["outputs_directory"] = "/o/"
    assert run_vqvae._output_path(cfg, "/data/sub-01_T1w.nii.gz", "reconstruction") == "/o/sub-01_T1w/sub-01_T1w_reconstruction.nii.gz"


def test_the_next_stage_lists_only_the_code_files(tmp_path):
    from synthanatomy_amd.utils.general import list_inputs
    from synthanatomy_amd.utils.nifti import output_header, write_nifti
    d = tmp_path / "outputs" / "x"
    os.makedirs(d)
    np.save(d / "x_quantization_0.npy", np.zeros((2, 2, 2), dtype=np.uint16))
    write_nifti(str(d / "x_reconstruction.nii.gz"), output_header((2, 2, 2), 16, np.eye(4)), np.zeros(8, dtype="<f4"))
    open(d / "x_reconstruction.nii.gz.part", "wb").close()      # a writer caught in the middle
    assert list_inputs(str(tmp_path / "outputs"), postfix="quantization_0") == [str(d / "x_quantization_0.npy")]
    assert list_inputs(str(tmp_path / "outputs")) == [str(d / "x_quantization_0.npy"), str(d / "x_reconstruction.nii.gz")]      # (.part matches nothing)
