"""numpy reference of the connected-component rule of DESIGN §7.17 (sa_components): ids by min-propagation to a fixed point, then sizes, the filter
and the summaries.  Everything is an integer: the kernel is held to this bit for bit."""
import numpy as np

NORM = {6: 1, 18: 2, 26: 3}
NAMES = ("components", "components_kept", "voxels_foreground", "voxels_kept", "largest_component")
LABEL_NAMES = ("tp", "fp", "fn", "lesions", "lesions_detected", "kept_true")


def offsets(connectivity):
    """the neighbours of the rule: offsets in {-1, 0, 1}^3 with 1 <= |o|_1 <= 1, 2, 3"""
    k = NORM[connectivity]
    return [(a, b, c) for a in (-1, 0, 1) for b in (-1, 0, 1) for c in (-1, 0, 1) if 1 <= abs(a) + abs(b) + abs(c) <= k]


def label_mask(mask, connectivity):
    """int64 [D, H, W]: 1 + the smallest linear index of the voxel's component on the foreground of the bool volume ``mask``, 0 elsewhere"""
    D, H, W = mask.shape
    big = np.int64(D * H * W + 1)
    ids = np.where(mask, np.arange(1, D * H * W + 1, dtype=np.int64).reshape(D, H, W), big)
    pad = np.full((D + 2, H + 2, W + 2), big, dtype=np.int64)
    offs = offsets(connectivity)
    while True:
        pad[1:-1, 1:-1, 1:-1] = ids
        best = ids
        for a, b, c in offs:
            best = np.minimum(best, pad[1 + a:1 + a + D, 1 + b:1 + b + H, 1 + c:1 + c + W])
        best = np.where(mask, best, big)
        # an id names a voxel of the same component, whose own id is no larger: taking it as well (pointer jumping) changes no fixed point and lets a
        # snake of thousands of voxels settle in tens of sweeps
        best = np.where(mask, np.minimum(best, best.ravel()[np.where(mask, best - 1, 0)]), big)
        if np.array_equal(best, ids):
            break
        ids = best
    return np.where(mask, ids, 0)


def foreground(a, threshold):
    """[a >= t] compared in fp32; a NaN is background"""
    with np.errstate(invalid="ignore"):
        return np.asarray(a, dtype=np.float32) >= np.float32(threshold)


def components(a, threshold, connectivity, min_size, labels=None):
    """(ids int32 [D, H, W], summaries dict of ints) for one volume ``a`` [D, H, W]; ``labels``: class 1 where non-zero"""
    full = label_mask(foreground(a, threshold), connectivity)
    return filter_ids(full, connectivity, min_size, labels)


def filter_ids(full, connectivity, min_size, labels=None):
    """the size filter and the summaries from the unfiltered canonical ids ``full``"""
    sizes = np.bincount(full.ravel())
    sizes[0] = 0
    found = np.flatnonzero(sizes)
    kept_ids = found[sizes[found] >= min_size]
    keep = np.zeros(sizes.shape, dtype=bool)
    keep[kept_ids] = True
    ids = np.where(keep[full], full, 0).astype(np.int32)
    kept = ids > 0
    s = {"components": int(found.size), "components_kept": int(kept_ids.size), "voxels_foreground": int(sizes.sum()),
         "voxels_kept": int(kept.sum()), "largest_component": int(sizes.max()) if sizes.size else 0}
    if labels is None:
        s.update({k: None for k in LABEL_NAMES})
        return ids, s
    y = np.asarray(labels) != 0
    lesion = label_mask(y, connectivity)
    s.update(tp=int((kept & y).sum()), fp=int((kept & ~y).sum()), fn=int((~kept & y).sum()),
             lesions=int(np.unique(lesion[y]).size), lesions_detected=int(np.unique(lesion[y & kept]).size),
             kept_true=int(np.unique(ids[kept & y]).size))
    return ids, s


def extents(ids, value):
    """(lo, hi) per axis of the voxels of ``ids`` equal to ``value``"""
    idx = np.nonzero(ids == value)
    return [(int(i.min()), int(i.max())) for i in idx]
