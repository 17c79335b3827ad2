"""Restatement of the dead-code restart rule of csrc/vq.hip in numpy, on tests/dropout_ref.py's Philox:

* donor rows: R_eff = min(R, Mtot), stride = Mtot // R_eff, g_j = j stride + (w_j mod stride), w_j = word 0 of
  philox4x32_10((j, lo32 step, hi32 step, 0x56515253), (lo32 seed, hi32 seed));
* idle[k] <- counts[k] > 0 ? 0 : min(idle[k] + 1, INT32_MAX); dead: idle[k] >= patience; the first R_eff dead codes in ascending k are restarted (idle 0);
* the identity: the restarting update is sa_vq_ema_update on inputs in which every restarted code has N = 0, embed_avg = 0, counts = 1, dw = its donor row.
"""
import numpy as np

import dropout_ref

INT32_MAX = 2 ** 31 - 1
TAG = 0x56515253
_M32 = 0xFFFFFFFF


def donor_indices(Mtot, R, seed, step):
    """the global row of every slot j < min(R, Mtot)"""
    r_eff = min(R, Mtot)
    stride = Mtot // r_eff
    key = (seed & _M32, (seed >> 32) & _M32)
    return [j * stride + dropout_ref.philox4x32_10((j, step & _M32, (step >> 32) & _M32, TAG), key)[0] % stride for j in range(r_eff)]


def donors(rows, R, seed, step, row_base=0, Mtot=None):
    """the [R, D] buffer one rank's gather writes: ``rows`` are the global rows row_base .. row_base + len(rows) - 1 of Mtot"""
    rows = np.asarray(rows, dtype=np.float32)
    M, D = rows.shape
    Mtot = M if Mtot is None else Mtot
    out = np.zeros((R, D), dtype=np.float32)
    for j, g in enumerate(donor_indices(Mtot, R, seed, step)):
        if row_base <= g < row_base + M:
            out[j] = rows[g - row_base]
    return out


def idle_rule(idle, counts, patience, r_eff):
    """(new idle, info [2 + r_eff]) -- info = dead codes found, codes restarted, their ids ascending, padded with -1"""
    idle = np.asarray(idle, dtype=np.int64)
    new = np.where(np.asarray(counts) > 0, 0, np.minimum(idle + 1, INT32_MAX))
    dead = np.flatnonzero(new >= patience)
    ids = dead[:r_eff]
    new[ids] = 0
    info = np.full(2 + r_eff, -1, dtype=np.int32)
    info[0], info[1] = len(dead), len(ids)
    info[2:2 + len(ids)] = ids
    return new.astype(np.int32), info


def substitute(N, avg, counts, dw, ids, donor_rows):
    """the inputs on which plain sa_vq_ema_update gives the restarting update, bit for bit"""
    N, avg, counts, dw = (np.array(a, dtype=np.float32, copy=True) for a in (N, avg, counts, dw))
    for i, k in enumerate(ids):
        N[k], counts[k] = 0.0, 1.0
        avg[k] = 0.0
        dw[k] = donor_rows[i]
    return N, avg, counts, dw
