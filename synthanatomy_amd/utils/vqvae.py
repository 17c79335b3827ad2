"""VQ-VAE helpers of the reference's ``src/utils/vqvae.py`` that the training loop needs."""
from __future__ import annotations

from math import floor


def get_ms_ssim_window(config: dict, logger=None) -> int:
    """Window size of the MS-SSIM key metric (reference ``src/utils/vqvae.py:499-543``).  The smallest spatial side comes from ``eval_patch_size``,
    else from ``roi`` (ints or (start, stop) pairs), else from ``input_shape``.  A side > 160 gives 11; otherwise w = floor((side / 16 + 1) / 2),
    ``ValueError`` for w <= 1, and an even w becomes the next odd number (default roi 160 -> 5, 112 -> 5, 48 -> 3, 47 -> ValueError)."""
    if config.get("eval_patch_size"):
        min_ps = min(config["eval_patch_size"])
    elif config.get("roi"):
        roi = config["roi"]
        if isinstance(roi[0], int):
            min_ps = min(roi)
        else:
            min_ps = min(a[1] - a[0] for a in roi)
    else:
        min_ps = min(config["input_shape"])

    if min_ps > 160:
        win_size = 11
    else:
        win_size = floor(((min_ps / 2 ** 4) + 1) / 2)
        if win_size <= 1:
            raise ValueError("Window size for MS-SSIM can't be calculated. Please increase patch_size's smallest dimension.")
        if win_size % 2 == 0:
            win_size += 1

    if logger:
        logger.info("MS-SSIM window calculation:")
        if config.get("eval_patch_size"):
            logger.info(f"\tMinimum spatial dimension: {min_ps}")
        logger.info(f"\tWindow size {win_size}")
    return win_size
