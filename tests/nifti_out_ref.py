"""Test-only numpy restatement of ``sa_volume_egress`` (include/synthanatomy_hip.h), written from the header's text, not from the kernel:
screen the non-finite values, flip / transpose the whole array into the file's axes, then float64 arithmetic with ``np.rint``, a clip and ``astype``."""
import numpy as np

from nifti_ref import CODES, SIGNED_PERMS  # noqa: F401  (shared with the ingest tests)

RANGES = {"int16": (-32768.0, 32767.0), "uint8": (0.0, 255.0)}


def stored_array(x, perm, sign):
    """F[i0, i1, i2] of the file: file voxel i takes x[c] with c_a = i[perm[a]], reversed where sign[a] < 0."""
    v = np.asarray(x)
    for a in range(3):
        if sign[a] < 0:
            v = np.flip(v, axis=a)
    return np.transpose(v, np.argsort(perm))      # file axis perm[a] is canonical axis a


def egress_ref(x, perm, sign, dtype="float32", slope=1.0, inter=0.0):
    """(the voxel block ``sa_volume_egress`` must write for x [ext0, ext1, ext2] (float32 values), the non-finite count)."""
    v = np.asarray(x, dtype=np.float32)
    bad = ~np.isfinite(v)
    v = stored_array(np.where(bad, np.float32(0), v), perm, sign)
    if dtype == "float32":
        out = v.astype("<f4")
    else:
        tmin, tmax = RANGES[dtype]
        q = (v.astype(np.float64) - np.float64(inter)) / np.float64(slope)      # two rounded double operations
        out = np.clip(np.rint(q), tmin, tmax).astype(np.dtype(dtype).newbyteorder("<"))
    return out.tobytes(order="F"), int(bad.sum())


def autoscale_ref(mn, mx, dtype):
    """(slope, inter) of SA_EGRESS_AUTOSCALE for the finite range [mn, mx] (float32 values): both float32-representable."""
    tmin, tmax = RANGES[dtype]
    mn, mx = np.float32(mn), np.float32(mx)
    if not mx > mn:
        return 1.0, float(mn)
    rng, span = tmax - tmin, np.float64(mx) - np.float64(mn)
    s = np.float32(span / rng)
    if np.float64(s) * rng < span:
        s = np.nextafter(s, np.float32(np.inf))
    return float(s), float(np.float32(np.float64(mn) - tmin * np.float64(s)))


def finite_min_max(x):
    v = np.asarray(x, dtype=np.float32)
    f = v[np.isfinite(v)]
    return (np.float32(f.min()), np.float32(f.max())) if f.size else (np.float32(0), np.float32(0))


def ulp32(v):
    return float(np.spacing(np.float32(abs(v))))
