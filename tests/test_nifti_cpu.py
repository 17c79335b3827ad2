"""CPU: the NIfTI-1 reader (synthanatomy_amd/utils/nifti.py), ``list_inputs`` over NIfTI directories and the read-ahead of ``run_vqvae.py``.  nibabel is
not available offline, so every expectation here is hand-built (tests/nifti_ref.py writes the files)."""
import os

import numpy as np
import pytest

from nifti_ref import CODES, SIGNED_PERMS, header_bytes, rotation_about, signed_perm_affine, write_nifti


def _volume(dtype, dims=(3, 4, 5), seed=0):
    rng = np.random.default_rng(seed)
    dt = np.dtype(dtype)
    if dt.kind == "f":
        return rng.standard_normal(dims).astype(dt)
    info = np.iinfo(dt)
    v = rng.integers(info.min, info.max, size=dims, endpoint=True, dtype=dt)
    v.flat[0], v.flat[-1] = info.min, info.max
    return v


@pytest.mark.parametrize("big_endian", [False, True])
@pytest.mark.parametrize("ext", [".nii", ".nii.gz"])
@pytest.mark.parametrize("dtype", sorted(CODES))
def test_round_trip(tmp_path, dtype, ext, big_endian):
    from synthanatomy_amd.utils.nifti import read_nifti
    data = _volume(dtype)
    path = str(tmp_path / ("v" + ext))
    written = write_nifti(path, data, big_endian=big_endian, slope=2.0, inter=-1.0, sform=signed_perm_affine((0, 1, 2), (1, 1, 1)))
    header, raw = read_nifti(path)
    assert bytes(raw) == written and len(raw) == header.nbytes == data.size * data.dtype.itemsize
    assert header.dims == (3, 4, 5) and header.datatype == CODES[dtype] and header.byteswap == big_endian and header.vox_offset == 352
    assert (header.slope, header.inter) == (2.0, -1.0)
    back = np.frombuffer(raw, dtype=header.numpy_dtype).reshape(header.dims, order="F")
    assert np.array_equal(back, data, equal_nan=data.dtype.kind == "f")


def test_vox_offset_behind_an_extension(tmp_path):
    from synthanatomy_amd.utils.nifti import read_nifti
    data = _volume("int16")
    plain = write_nifti(str(tmp_path / "a.nii"), data)
    with_ext = write_nifti(str(tmp_path / "b.nii.gz"), data, extension=struct_extension())
    ha, ra = read_nifti(str(tmp_path / "a.nii"))
    hb, rb = read_nifti(str(tmp_path / "b.nii.gz"))
    assert (ha.vox_offset, hb.vox_offset) == (352, 384) and bytes(ra) == bytes(rb) == plain == with_ext


def struct_extension():
    import struct
    return struct.pack("<2i", 32, 4) + b"comment".ljust(24, b"\0")      # esize 32, ecode 4 (comment)


@pytest.mark.parametrize("slope,inter,want", [(0.0, 5.0, (1.0, 0.0)), (float("nan"), 0.0, (1.0, 0.0)), (float("inf"), 1.0, (1.0, 0.0)), (1.0, 0.0, (1.0, 0.0)),
                                              (1.0, 2.0, (1.0, 2.0)), (0.5, 0.0, (0.5, 0.0)), (-2.0, -3.25, (-2.0, -3.25))])
def test_scaling_rule(slope, inter, want):
    from synthanatomy_amd.utils.nifti import parse_header
    h = parse_header(header_bytes((2, 2, 2), 4, slope=slope, inter=inter))
    assert (h.slope, h.inter) == want


def test_trailing_singleton_dims_are_accepted():
    from synthanatomy_amd.utils.nifti import parse_header
    assert parse_header(header_bytes((2, 3, 4), 4, dim0=5, extra_dims=(1, 1))).dims == (2, 3, 4)
    assert parse_header(header_bytes((2, 3, 1), 4, dim0=2)).dims == (2, 3, 1)
    with pytest.raises(ValueError, match="dim"):
        parse_header(header_bytes((2, 3, 4), 4, dim0=4, extra_dims=(2,)))


def test_affine_precedence(tmp_path):
    from synthanatomy_amd.utils.nifti import header_orientation, parse_header
    # quaternion (b, c, d) = (0, 0, 1): a rotation by 180 degrees about z, R = diag(-1, -1, 1)
    q_lps = (0.0, 0.0, 1.0, 1.0, (1.0, 2.0, 3.0), (4.0, 5.0, 6.0))
    h = parse_header(header_bytes((2, 3, 4), 4, sform=signed_perm_affine((1, 0, 2), (1, 1, -1)), qform=q_lps))
    assert np.allclose(h.affine, signed_perm_affine((1, 0, 2), (1, 1, -1)))                       # sform over qform
    assert header_orientation(h, True) == ([1, 0, 2], [1, 1, -1])
    h = parse_header(header_bytes((2, 3, 4), 4, qform=q_lps))                                        # qform alone
    assert np.allclose(h.affine, [[-1, 0, 0, 4], [0, -2, 0, 5], [0, 0, 3, 6], [0, 0, 0, 1]], atol=1e-6)
    assert header_orientation(h, True) == ([0, 1, 2], [-1, -1, 1])
    h = parse_header(header_bytes((2, 3, 4), 4, qform=(0.0, 0.0, 1.0, -1.0, (1.0, 2.0, 3.0), (4.0, 5.0, 6.0))))      # qfac = -1 negates the third column
    assert np.allclose(h.affine[:3, :3], np.diag([-1, -2, -3]), atol=1e-6) and header_orientation(h, True) == ([0, 1, 2], [-1, -1, -1])
    # (b, c, d) = (1/2, 1/2, 1/2), a = 1/2: the cyclic rotation x -> y -> z -> x, so file axis 0 points along world y
    h = parse_header(header_bytes((2, 3, 4), 4, qform=(0.5, 0.5, 0.5, 1.0, (1.0, 1.0, 1.0), (0.0, 0.0, 0.0))))
    assert np.allclose(h.affine[:3, :3], [[0, 0, 1], [1, 0, 0], [0, 1, 0]], atol=1e-6) and header_orientation(h, True) == ([2, 0, 1], [1, 1, 1])
    h = parse_header(header_bytes((2, 3, 4), 4), "nowhere.nii")                                      # neither: refuse canonical, load as stored
    assert h.affine is None and header_orientation(h, False) == ([0, 1, 2], [1, 1, 1])
    with pytest.raises(ValueError, match=r"nowhere\.nii.*sform_code.*qform_code"):
        header_orientation(h, True)


@pytest.mark.parametrize("rotated", [False, True])
def test_orientation_gives_back_every_signed_permutation(rotated):
    """All 48 signed permutations times positive zooms (0.7, 1.0, 2.5), and the same composed with a rotation of 15 degrees about (1, 2, 3) / sqrt(14).
    LIMIT: in every case the dominant entry of each column stays dominant (cos 15 = 0.97 against at most sin 15 = 0.26 elsewhere), so no tie-break of
    the greedy assignment is exercised; nibabel's behaviour on ties is not pinned here."""
    from synthanatomy_amd.utils.nifti import orientation
    rot = rotation_about((1, 2, 3), 15.0) if rotated else None
    assert len(SIGNED_PERMS) == 48
    for perm, sign in SIGNED_PERMS:
        assert orientation(signed_perm_affine(perm, sign, rotation=rot)) == (list(perm), list(sign)), (perm, sign)
    with pytest.raises(ValueError, match="affine"):
        orientation(np.diag([1.0, 0.0, 1.0, 1.0]))


def test_refusals_name_the_file_and_the_field(tmp_path):
    from synthanatomy_amd.utils.nifti import read_nifti
    data = _volume("int16")

    def refuse(name, match, **kw):
        path = str(tmp_path / name)
        write_nifti(path, data, **kw)
        with pytest.raises(ValueError, match=match) as e:
            read_nifti(path)
        assert name in str(e.value)

    refuse("nifti2.nii", "sizeof_hdr = 540", sizeof_hdr=540)
    refuse("nifti2be.nii", "sizeof_hdr = 540", sizeof_hdr=540, big_endian=True)
    refuse("pair.nii", "magic.*ni1", magic=b"ni1\0")
    refuse("magic.nii", "magic", magic=b"abc\0")
    refuse("size.nii", "sizeof_hdr", sizeof_hdr=100)
    refuse("short.nii", "truncated.*vox_offset", truncate=3)
    refuse("short.nii.gz", "truncated.*vox_offset", truncate=3)
    refuse("fourd.nii", "dim", dim0=4, extra_dims=(2,))
    refuse("offset.nii", "vox_offset", vox_offset=100.0)
    for code in (32, 128, 1024, 1280, 1536, 1792, 2304, 7):      # complex64, RGB24, int64, uint64, float128, complex128, RGBA32, no code at all
        path = str(tmp_path / f"dt{code}.nii")
        with open(path, "wb") as f:
            f.write(header_bytes((3, 4, 5), code) + b"\0" * 4 + b"\0" * 2000)
        with pytest.raises(ValueError, match=rf"dt{code}\.nii: datatype = {code}"):
            read_nifti(path)
    path = str(tmp_path / "stub.nii")
    with open(path, "wb") as f:
        f.write(b"\x5c\x01\0\0" + b"\0" * 10)
    with pytest.raises(ValueError, match=r"stub\.nii: sizeof_hdr"):
        read_nifti(path)


def test_list_inputs_finds_nifti_and_leaves_npy_listings_alone(tmp_path):
    from synthanatomy_amd.utils import general as G
    mixed, only = tmp_path / "mixed", tmp_path / "only"
    (mixed / "sub").mkdir(parents=True)
    only.mkdir()
    for name in ("b.nii.gz", "a.npy", "c.nii", "sub/d.nii.gz", "notes.txt", "e.nii.txt"):
        (mixed / name).write_bytes(b"")
    for name in ("y.npy", "x.npy", "x_quantization_0.npy", "readme.md"):
        (only / name).write_bytes(b"")
    assert G.list_inputs(str(mixed)) == [str(mixed / n) for n in ("a.npy", "b.nii.gz", "c.nii", "sub/d.nii.gz")]
    assert G.list_inputs(str(only)) == [str(only / n) for n in ("x.npy", "x_quantization_0.npy", "y.npy")]
    assert G.list_inputs(str(only), postfix="quantization_0") == [str(only / "x_quantization_0.npy")]
    assert G.list_inputs(str(mixed / "*.nii*")) == [str(mixed / n) for n in ("b.nii.gz", "c.nii", "e.nii.txt")]      # a glob passes any name through


def test_read_ahead_does_not_change_order_or_content(tmp_path):
    """--num_workers=0 (inline) and 4 (threads fetching the next batch) deliver the same names and the same bytes in the same order."""
    import run_vqvae
    files = []
    for i in range(7):
        path = str(tmp_path / f"s{i}.nii{'.gz' if i % 2 else ''}")
        write_nifti(path, _volume("int16", seed=i), sform=signed_perm_affine((0, 1, 2), (1, 1, 1)))
        files.append(path)
    np.save(str(tmp_path / "plain.npy"), np.zeros((2, 2, 2), np.float32))
    files.insert(3, str(tmp_path / "plain.npy"))
    order = [5, 0, 7, 3, 2, 6, 1, 4]
    chunks = [[files[k] for k in order[i:i + 3]] for i in range(0, len(order), 3)]

    def collect(workers):
        got = []
        for chunk, blocks in run_vqvae._with_nifti_blocks(chunks, lambda f: f, {"num_workers": workers}):
            assert len(chunk) == len(blocks)
            got.append([(f, None if b is None else (b[0].dims, b[0].datatype, bytes(b[1]))) for f, b in zip(chunk, blocks)])
        return got

    inline, threaded = collect(0), collect(4)
    assert inline == threaded and [[f for f, _ in c] for c in inline] == chunks
    assert all((b is None) == f.endswith(".npy") for c in inline for f, b in c)
    assert len({b[2] for c in inline for _, b in c if b is not None}) == 7      # seven different voxel blocks
    assert os.path.basename(inline[1][0][0]) == "plain.npy"
