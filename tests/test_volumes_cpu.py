"""CPU: the output side of synthanatomy_amd/utils/volumes.py: one ``stem`` behind every output name, and ``VolumeWriter`` in ``.npy`` mode."""
import os

import numpy as np
import pytest
import torch

import run_vqvae as RV
from synthanatomy_amd.utils import volumes as V
from synthanatomy_amd.utils.general import save_npy, stem

NAMES = ["/data/in/s0.nii.gz", "/data/in/s1.nii", "/data/in/s2.npy", "synthetic_0003"]


def test_stem_strips_the_three_extensions_and_nothing_else():
    assert [stem(n) for n in NAMES] == ["s0", "s1", "s2", "synthetic_0003"]
    assert V.stem is stem and stem("s4.npz") == "s4.npz" and stem("/a.nii/b") == "b"
    # stacked extensions: one rule for every name derived from a file, the one save_npy has always used for its directories
    assert stem("/d/x.npy.nii.gz") == "x" and stem("x.nii.npy") == "x.nii" and V._augmented_name("/d/x.npy.nii.gz", 2) == "/d/x_2.npy.nii.gz"
    assert V._output_path({"outputs_directory": "/o/", "output_ext": ".npy"}, "/d/x.npy.nii.gz", "sample") == "/o/x/x_sample.npy"


def test_the_output_names_are_the_ones_written_before(tmp_path):
    out = str(tmp_path) + "/"
    got = [save_npy(np.zeros(2), out, n, "quantization_0") for n in NAMES]
    assert got == [out + "s0/s0_quantization_0.npy", out + "s1/s1_quantization_0.npy", out + "s2/s2_quantization_0.npy",
                   out + "synthetic_0003/synthetic_0003_quantization_0.npy"]
    assert all(os.path.exists(p) for p in got) and np.load(got[0]).dtype == np.uint16
    cfg = {"outputs_directory": "/proj/outputs/", "output_ext": ".nii.gz"}
    assert [RV._output_path(cfg, n, "reconstruction") for n in NAMES] == [
        "/proj/outputs/s0/s0_reconstruction.nii.gz", "/proj/outputs/s1/s1_reconstruction.nii.gz", "/proj/outputs/s2/s2_reconstruction.nii.gz",
        "/proj/outputs/synthetic_0003/synthetic_0003_reconstruction.nii.gz"]
    assert RV._output_path(dict(cfg, output_ext=".npy"), NAMES[0], "sample") == "/proj/outputs/s0/s0_sample.npy"
    assert [RV._augmented_name(n, 2) for n in NAMES] == ["/data/in/s0_2.nii.gz", "/data/in/s1_2.nii", "/data/in/s2_2.npy", "synthetic_0003_2"]
    assert RV._output_path is V._output_path and RV._augmented_name is V._augmented_name and RV._load_volume is V._load_volume


def test_volume_writer_in_npy_mode_writes_what_save_npy_writes(tmp_path):
    cfg = dict(RV.DEFAULTS, outputs_directory=str(tmp_path / "w") + "/", num_workers=0)
    x = torch.randn(3, 1, 4, 5, 6, generator=torch.Generator().manual_seed(0)).to(torch.bfloat16)      # the decoder's dtype under --amp
    names = NAMES[:3]
    writer = V.VolumeWriter(cfg)
    try:
        writer.batch()
        writer.save(names, {"reconstruction": x}, [None, None, None])
        writer.save(names[:1], {"sample": x.float()})
    finally:
        writer.close()
    for j, n in enumerate(names):
        want = save_npy(x[j, 0].float().numpy(), str(tmp_path / "ref") + "/", n, "reconstruction", np.float32)
        got = V._output_path(cfg, n, "reconstruction")
        assert os.path.relpath(got, cfg["outputs_directory"]) == os.path.relpath(want, str(tmp_path / "ref"))
        assert np.load(got).dtype == np.float32 and np.load(got).shape == (4, 5, 6)
        with open(got, "rb") as a, open(want, "rb") as b:
            assert a.read() == b.read()
    assert sorted(os.listdir(tmp_path / "w" / "s0")) == ["s0_reconstruction.npy", "s0_sample.npy"]


def test_close_re_raises_a_writers_exception(tmp_path):
    writer = V.VolumeWriter(dict(RV.DEFAULTS, outputs_directory=str(tmp_path) + "/", output_ext=".nii", num_workers=1))

    def fail():
        raise OSError("the disk is full")
    writer.saver.current.append(writer.saver.pool.submit(fail))      # a writer thread's job, as NiftiSaver.save queues them
    with pytest.raises(OSError, match="the disk is full"):
        writer.close()
