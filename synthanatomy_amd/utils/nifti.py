"""Single-file NIfTI-1 reader on the standard library and numpy: the header, the affine and the orientation of the reference's
``LoadImaged(reader="NibabelReader", as_closest_canonical=load_nii_canonical)`` (reference ``src/utils/vqvae.py:205-215``).  The voxel block is NOT decoded
here: ``read_nifti`` hands it out as stored and ``sa_volume_ingest`` (csrc/ingest.hip) converts, reorients, crops and normalises it on the
device.

UNPINNED: nibabel and MONAI are not available offline.  The scaling rule, the affine precedence (sform, then qform), the quaternion formula and
``orientation`` (nibabel's ``io_orientation`` followed by the transform to RAS+ of ``as_closest_canonical``) are this package's restatement; the tests check
them on hand-built vectors whose answer does not depend on tie-breaking.

Deliberate refusals: NIfTI-2, ``.hdr`` / ``.img`` pairs, complex / RGB / 64-bit integer / float128 voxels, more than three non-singleton dims, and
canonical loading of a file without orientation (both codes 0: nothing is guessed).

The writer at the end of the file (``output_header``, ``output_affine``, ``write_nifti``) is the other direction on the same terms: standard
library and numpy only, nibabel's ``Nifti1Image(data, affine)`` and MONAI's ``SegmentationSaver`` conventions restated and UNPINNED, the voxel block
produced on the device by ``sa_volume_egress`` (csrc/egress.hip)."""
from __future__ import annotations

import gzip
import os
import struct
from dataclasses import dataclass
from typing import Optional

import numpy as np

# NIfTI datatype code -> (numpy kind + size, bytes per voxel); include/synthanatomy_hip.h: SA_NII_*
DATATYPES = {2: ("u1", 1), 4: ("i2", 2), 8: ("i4", 4), 16: ("f4", 4), 64: ("f8", 8), 256: ("i1", 1), 512: ("u2", 2), 768: ("u4", 4)}
_UNSUPPORTED = {0: "unknown", 1: "binary", 32: "complex64", 128: "RGB24", 1024: "int64", 1280: "uint64", 1536: "float128", 1792: "complex128",
                2048: "complex256", 2304: "RGBA32"}


@dataclass
class NiftiHeader:
    path: str
    dims: tuple                     # (n0, n1, n2), axis 0 fastest in the file
    datatype: int                   # NIfTI code, a key of DATATYPES
    byteswap: bool                  # the file is big-endian
    slope: float                    # (1.0, 0.0) when the file's pair is unusable or the identity
    inter: float
    affine: Optional[np.ndarray]    # 4 x 4 fp64 voxel -> world, None when sform_code == qform_code == 0
    vox_offset: int

    @property
    def numpy_dtype(self) -> np.dtype:
        return np.dtype((">" if self.byteswap else "<") + DATATYPES[self.datatype][0])

    @property
    def nbytes(self) -> int:
        return int(np.prod(self.dims, dtype=np.int64)) * DATATYPES[self.datatype][1]


def _open(path):
    with open(path, "rb") as f:
        gz = f.read(2) == b"\x1f\x8b"
    return gzip.open(path, "rb") if gz else open(path, "rb")


def _quaternion_affine(b, c, d, qfac, pixdim, offset) -> np.ndarray:
    """The qform of the NIfTI-1 standard: a = sqrt(1 - b^2 - c^2 - d^2), columns scaled by pixdim[1..3], the third negated for qfac = -1."""
    b, c, d = float(b), float(c), float(d)
    a = np.sqrt(max(1.0 - (b * b + c * c + d * d), 0.0))
    rot = np.array([[a * a + b * b - c * c - d * d, 2 * b * c - 2 * a * d, 2 * b * d + 2 * a * c],
                    [2 * b * c + 2 * a * d, a * a + c * c - b * b - d * d, 2 * c * d - 2 * a * b],
                    [2 * b * d - 2 * a * c, 2 * c * d + 2 * a * b, a * a + d * d - c * c - b * b]], dtype=np.float64)
    zooms = np.array([float(pixdim[1]), float(pixdim[2]), float(pixdim[3]) * (-1.0 if qfac < 0 else 1.0)], dtype=np.float64)
    aff = np.eye(4)
    aff[:3, :3] = rot * zooms[None, :]
    aff[:3, 3] = offset
    return aff


def parse_header(hdr: bytes, path: str = "<bytes>") -> NiftiHeader:
    if len(hdr) < 348:
        raise ValueError(f"{path}: sizeof_hdr: the file ends after {len(hdr)} bytes, a NIfTI-1 header has 348")
    size_le, size_be = struct.unpack("<i", hdr[:4])[0], struct.unpack(">i", hdr[:4])[0]
    if size_le == 540 or size_be == 540:
        raise ValueError(f"{path}: sizeof_hdr = 540: NIfTI-2 is not supported (convert to NIfTI-1)")
    if size_le == 348:
        en = "<"
    elif size_be == 348:
        en = ">"
    else:
        raise ValueError(f"{path}: sizeof_hdr = {size_le}: not a NIfTI-1 file")
    magic = hdr[344:348]
    if magic == b"ni1\0":
        raise ValueError(f"{path}: magic = 'ni1': .hdr / .img pairs are not supported (convert to a single .nii file)")
    if magic != b"n+1\0":
        raise ValueError(f"{path}: magic = {magic!r}: not a single-file NIfTI-1 ('n+1')")
    dim = struct.unpack(en + "8h", hdr[40:56])
    if not 1 <= dim[0] <= 7:
        raise ValueError(f"{path}: dim[0] = {dim[0]}: outside 1..7")
    if any(n < 1 for n in dim[1:dim[0] + 1]):
        raise ValueError(f"{path}: dim = {dim}: an extent below 1")
    if any(n != 1 for n in dim[4:dim[0] + 1]):
        raise ValueError(f"{path}: dim = {dim}: more than three dims with an extent above 1")
    dims = tuple(int(dim[k]) if k <= dim[0] else 1 for k in (1, 2, 3))
    datatype, bitpix = struct.unpack(en + "2h", hdr[70:74])
    if datatype not in DATATYPES:
        raise ValueError(f"{path}: datatype = {datatype} ({_UNSUPPORTED.get(datatype, 'not a NIfTI-1 code')}): supported are uint8, int16, int32, float32, "
                         "float64, int8, uint16 and uint32")
    if bitpix != 8 * DATATYPES[datatype][1]:
        raise ValueError(f"{path}: bitpix = {bitpix} contradicts datatype = {datatype}")
    pixdim = struct.unpack(en + "8f", hdr[76:108])
    vox_offset, slope, inter = struct.unpack(en + "3f", hdr[108:120])
    if not np.isfinite(vox_offset) or vox_offset < 352 or vox_offset != int(vox_offset):
        raise ValueError(f"{path}: vox_offset = {vox_offset}: a single-file NIfTI-1 keeps its voxels at a whole offset of at least 352")
    # nibabel's rule: the pair applies when the slope is finite and non-zero (and the intercept finite) and the pair is not the identity
    if not (np.isfinite(slope) and slope != 0 and np.isfinite(inter)) or (slope == 1 and inter == 0):
        slope, inter = 1.0, 0.0
    qform_code, sform_code = struct.unpack(en + "2h", hdr[252:256])
    affine = None
    if sform_code != 0:
        affine = np.eye(4)
        affine[:3, :] = np.array(struct.unpack(en + "12f", hdr[280:328]), dtype=np.float64).reshape(3, 4)
    elif qform_code != 0:
        b, c, d, ox, oy, oz = struct.unpack(en + "6f", hdr[256:280])
        affine = _quaternion_affine(b, c, d, pixdim[0], pixdim, (ox, oy, oz))
    return NiftiHeader(path=str(path), dims=dims, datatype=int(datatype), byteswap=en == ">", slope=float(slope), inter=float(inter), affine=affine,
                       vox_offset=int(vox_offset))


def read_nifti(path):
    """(header, raw): the parsed header and the voxel block as stored (``bytes``, ``header.nbytes`` long) -- plain or gzip-compressed single-file NIfTI-1."""
    with _open(path) as f:
        header = parse_header(f.read(348), path)
        try:
            f.read(header.vox_offset - 348)          # the extension flag and the extensions
            raw = f.read(header.nbytes)
        except EOFError:                             # (a gzip stream that ends early)
            raw = b""
    if len(raw) < header.nbytes:
        raise ValueError(f"{path}: voxel block truncated: dim = {header.dims} and datatype = {header.datatype} need {header.nbytes} bytes behind "
                         f"vox_offset = {header.vox_offset}, the file holds {len(raw)}")
    return header, raw


def orientation(affine) -> tuple:
    """(perm, sign) of the closest canonical (RAS+) orientation: canonical axis a reads file axis perm[a], reversed where sign[a] < 0
    (``SA_AUG_SIGNED_PERM``'s convention).  nibabel's ``io_orientation``: the columns of the 3 x 3 part over their norms, replaced by the nearest orthogonal
    matrix P @ Qs of the SVD; then for file axes 0, 1, 2 in order the world axis with the largest |entry| of that column, its sign, and that world row
    zeroed."""
    rzs = np.asarray(affine, dtype=np.float64)[:3, :3]
    if not np.all(np.isfinite(rzs)):
        raise ValueError("affine: a non-finite entry")
    zooms = np.sqrt((rzs * rzs).sum(axis=0))
    zooms[zooms == 0] = 1.0
    rs = rzs / zooms
    p, s, qs = np.linalg.svd(rs)
    keep = s > s.max() * 3 * np.finfo(s.dtype).eps
    r = p[:, keep] @ qs[keep]
    perm, sign = [-1, -1, -1], [1, 1, 1]
    for in_ax in range(3):
        col = r[:, in_ax]
        if np.allclose(col, 0):
            raise ValueError(f"affine: file axis {in_ax} has no direction in world space (a singular affine)")
        out_ax = int(np.argmax(np.abs(col)))
        perm[out_ax] = in_ax
        sign[out_ax] = -1 if col[out_ax] < 0 else 1
        r[out_ax, :] = 0
    return perm, sign


def header_orientation(header: NiftiHeader, canonical: bool) -> tuple:
    """(perm, sign) for ``sa_volume_ingest``: the stored order without ``canonical``; with it the file must carry an orientation."""
    if not canonical:
        return [0, 1, 2], [1, 1, 1]
    if header.affine is None:
        raise ValueError(f"{header.path}: sform_code = qform_code = 0: the file carries no orientation, so --load_nii_canonical=True cannot reorient it "
                         "(nothing is guessed; pass --load_nii_canonical=False to load it as stored)")
    return orientation(header.affine)


def is_nifti(path: str) -> bool:
    return isinstance(path, str) and path.endswith((".nii", ".nii.gz"))


# ---- the writer: what SegmentationSaver(output_ext=".nii.gz", resample=False) -> nibabel.Nifti1Image(data, affine) leaves on disk, as far as
# this package restates it.  UNPINNED like the reader: the header fields below are the restatement, ``parse_header`` reads back what is written, and the
# voxel block comes from ``sa_volume_egress`` (csrc/egress.hip), not from numpy.

def output_header(dims, datatype: int, affine, slope: float = 1.0, inter: float = 0.0) -> bytes:
    """352 bytes: the little-endian NIfTI-1 header of a [n0, n1, n2] volume plus the four zero extension bytes, the voxel block follows at once
    (vox_offset 352).  sform_code 2 with ``affine`` in srow_*, qform_code 0, pixdim[1..3] = the affine's column norms, xyzt_units 2 (mm).  float32 carries
    scl_slope = scl_inter = 0 ("no scaling"); an integer datatype carries (slope, inter) as float32."""
    if datatype not in (2, 4, 16):
        raise ValueError(f"output_header: datatype = {datatype}: the writer stores uint8 (2), int16 (4) and float32 (16)")
    dims = [int(n) for n in dims]
    if len(dims) != 3 or any(not 1 <= n <= 32767 for n in dims):
        raise ValueError(f"output_header: dims = {dims}: three extents in 1..32767")
    aff = np.asarray(affine, dtype=np.float64)
    if aff.shape != (4, 4) or not np.all(np.isfinite(aff)):
        raise ValueError("output_header: the affine must be a finite 4 x 4 matrix")
    h = bytearray(352)
    struct.pack_into("<i", h, 0, 348)
    struct.pack_into("<8h", h, 40, 3, *dims, 1, 1, 1, 1)
    struct.pack_into("<2h", h, 70, datatype, 8 * DATATYPES[datatype][1])
    zooms = np.sqrt((aff[:3, :3] ** 2).sum(axis=0))
    struct.pack_into("<8f", h, 76, 1.0, *zooms, 1.0, 1.0, 1.0, 1.0)
    struct.pack_into("<3f", h, 108, 352.0, *((0.0, 0.0) if datatype == 16 else (float(slope), float(inter))))
    h[123] = 2
    struct.pack_into("<2h", h, 252, 0, 2)
    struct.pack_into("<12f", h, 280, *aff[:3].reshape(-1))
    h[344:348] = b"n+1\0"
    return bytes(h)


def output_affine(src_affine, perm, sign, n_can, start, size) -> np.ndarray:
    """The affine of the block [start, start + size) of a canonical volume, stored back in the SOURCE file's own axes: output voxel g is source-file
    voxel g + s, with s = start[a] along file axis perm[a] where sign[a] > 0 and n_can[a] - start[a] - size[a] where the axis is reversed, so only the
    translation changes: t' = R s + t.  (MONAI 0.5's crop leaves the affine untouched, so upstream's saved crop lands shifted: deliberately not
    reproduced)  ``start`` may be negative (a file smaller than the ROI, mirror-padded).  ``src_affine`` None: the identity."""
    if src_affine is None:
        return np.eye(4)
    aff = np.array(src_affine, dtype=np.float64)
    s = np.zeros(3)
    for a in range(3):
        s[perm[a]] = start[a] if sign[a] > 0 else n_can[a] - start[a] - size[a]
    aff[:3, 3] = aff[:3, :3] @ s + aff[:3, 3]
    return aff


def write_nifti(path, header_bytes: bytes, block) -> str:
    """``header_bytes`` (``output_header``) and the voxel block (anything with the buffer protocol) -> ``path``: plain for ``.nii``, one gzip member for
    ``.nii.gz`` (level 1: compression is the bound of this path; mtime 0 and no name: the bytes depend on the content only).  Written to ``<path>.part``
    and renamed, so no reader ever sees a partial file under the final name."""
    path = str(path)
    if not is_nifti(path):
        raise ValueError(f"write_nifti: {path}: the name must end in .nii or .nii.gz")
    part = path + ".part"
    try:
        with open(part, "wb") as f:
            if path.endswith(".gz"):
                with gzip.GzipFile(filename="", mode="wb", compresslevel=1, fileobj=f, mtime=0) as z:
                    z.write(header_bytes)
                    z.write(block)
            else:
                f.write(header_bytes)
                f.write(block)
        os.replace(part, path)
    except BaseException:
        if os.path.exists(part):
            os.remove(part)
        raise
    return path
