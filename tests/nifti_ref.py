"""Test-only helpers for the NIfTI input path: a minimal NIfTI-1 writer (every header field the reader looks at, either byte order, optional gzip, and
deliberately broken files) and ``ingest_ref``, a numpy restatement of ``sa_volume_ingest`` (include/synthanatomy_hip.h) written from the header's text, not
from the kernel: decode the whole block with numpy, scale in float64, transpose / flip the whole array, then crop."""
import gzip
import itertools
import struct

import numpy as np

CODES = {"uint8": 2, "int16": 4, "int32": 8, "float32": 16, "float64": 64, "int8": 256, "uint16": 512, "uint32": 768}
SIGNED_PERMS = [(p, s) for p in itertools.permutations(range(3)) for s in itertools.product((1, -1), repeat=3)]      # all 48


def signed_perm_affine(perm, sign, zooms=(0.7, 1.0, 2.5), rotation=None):
    """A 4 x 4 affine whose closest canonical orientation is (perm, sign): canonical (world) axis a is fed by file axis perm[a], pointing backwards
    where sign[a] < 0 -- column perm[a] of the 3 x 3 part is sign[a] * e_a, times the zoom of that FILE axis; ``rotation`` (3 x 3) is applied on the left."""
    m = np.zeros((3, 3))
    for a in range(3):
        m[a, perm[a]] = sign[a]
    m = m @ np.diag(zooms)
    if rotation is not None:
        m = rotation @ m
    aff = np.eye(4)
    aff[:3, :3] = m
    aff[:3, 3] = (-11.0, 7.5, 3.0)
    return aff


def rotation_about(axis, degrees):
    """Rodrigues' formula."""
    k = np.asarray(axis, dtype=np.float64)
    k = k / np.linalg.norm(k)
    t = np.deg2rad(degrees)
    kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(t) * kx + (1 - np.cos(t)) * (kx @ kx)


def header_bytes(dims, datatype, *, big_endian=False, slope=0.0, inter=0.0, sform=None, qform=None, vox_offset=352.0, magic=b"n+1\0", sizeof_hdr=348,
                 dim0=3, bitpix=None, extra_dims=()):
    """The 348 header bytes.  ``sform``: a 4 x 4 affine (sform_code 1); ``qform``: (b, c, d, qfac, (dx, dy, dz), (ox, oy, oz)) (qform_code 1)."""
    en = ">" if big_endian else "<"
    size = {2: 1, 4: 2, 8: 4, 16: 4, 64: 8, 256: 1, 512: 2, 768: 4}.get(datatype, 2)
    h = bytearray(348)
    struct.pack_into(en + "i", h, 0, sizeof_hdr)
    dim = [dim0, *dims, *extra_dims] + [1] * (7 - 3 - len(extra_dims))
    struct.pack_into(en + "8h", h, 40, *dim)
    struct.pack_into(en + "2h", h, 70, datatype, 8 * size if bitpix is None else bitpix)
    pixdim = [1.0] * 8
    if qform is not None:
        b, c, d, qfac, zooms, offset = qform
        pixdim[0], pixdim[1:4] = qfac, zooms
        struct.pack_into(en + "h", h, 252, 1)
        struct.pack_into(en + "6f", h, 256, b, c, d, *offset)
    struct.pack_into(en + "8f", h, 76, *pixdim)
    struct.pack_into(en + "3f", h, 108, vox_offset, slope, inter)
    if sform is not None:
        struct.pack_into(en + "h", h, 254, 1)
        struct.pack_into(en + "12f", h, 280, *np.asarray(sform, dtype=np.float64)[:3].reshape(-1))
    h[344:348] = magic
    return bytes(h)


def write_nifti(path, data, *, big_endian=False, extension=b"", truncate=0, **header):
    """``data`` [n0, n1, n2] (as nibabel would hand it out: data[i0, i1, i2]) in one of the dtypes of ``CODES`` -> a single-file NIfTI-1 at ``path``
    (gzip-compressed when the name ends in .gz), voxels in Fortran order.  ``extension``: bytes between the header and the voxel block (vox_offset moves);
    ``truncate``: bytes cut off the end of the voxel block.  Returns the voxel block as written."""
    data = np.asarray(data)
    code = CODES[data.dtype.name]
    raw = np.asfortranarray(data).astype(data.dtype.newbyteorder(">" if big_endian else "<")).tobytes(order="F")
    header.setdefault("vox_offset", 352.0 + len(extension))
    blob = header_bytes(data.shape, code, big_endian=big_endian, **header) + (b"\1\0\0\0" if extension else b"\0\0\0\0") + extension
    blob += raw[:len(raw) - truncate]
    with (gzip.open(path, "wb", compresslevel=1) if str(path).endswith(".gz") else open(path, "wb")) as f:
        f.write(blob)
    return raw


def canonical_array(header, raw, canonical=True):
    """(the whole volume in canonical axes as fp32 with non-finite voxels replaced by 0, their count, min and max of the finite voxels)."""
    from synthanatomy_amd.utils.nifti import header_orientation
    n = int(np.prod(header.dims))
    stored = np.frombuffer(raw, dtype=header.numpy_dtype, count=n).reshape(header.dims, order="F")
    if (header.slope, header.inter) == (1.0, 0.0):
        v = stored.astype(np.float32)
    else:
        with np.errstate(over="ignore", invalid="ignore"):
            v = ((stored.astype(np.float64) * np.float64(header.slope)) + np.float64(header.inter)).astype(np.float32)
    bad = ~np.isfinite(v)
    finite = v[~bad]
    mn, mx = (np.float32(finite.min()), np.float32(finite.max())) if finite.size else (np.float32(0), np.float32(0))
    v = np.where(bad, np.float32(0), v)
    perm, sign = header_orientation(header, canonical)
    v = np.transpose(v, perm)
    for a in range(3):
        if sign[a] < 0:
            v = np.flip(v, axis=a)
    return np.array(v, order="C", copy=True), int(bad.sum()), mn, mx


def scale_intensity_fp32(v, mn, mx):
    """The expression of run_vqvae._read_volume, every operation in fp32: (v - min) / (max - min + 1e-8)."""
    den = np.float32(np.float32(mx - mn) + np.float32(1e-8))
    return ((v - np.float32(mn)) / den).astype(np.float32)


def ingest_ref(header, raw, window=None, normalize=True, canonical=True):
    """What ``hip_ingest`` must return (without the channel axis), and the non-finite count."""
    v, bad, mn, mx = canonical_array(header, raw, canonical)
    if normalize:
        v = scale_intensity_fp32(v, mn, mx)
    if window is not None:
        (a, b, c), (da, db, dc) = window
        v = v[a:a + da, b:b + db, c:c + dc]
    return np.array(v, order="C", copy=True), bad
