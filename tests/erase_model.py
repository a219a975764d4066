"""The compaction rule of swps_erase / swps_prune in numpy.

N rows, dead[r] marks the rows to remove, M = N - #dead survive.  The holes are the dead rows
r < M, the movers the live rows r >= M, both ascending and equally many; the k-th mover is copied
into the k-th hole and every other row stays where it is."""
import numpy as np


def plan(dead):
    """dead: [N] flags -> (M, src, dst): row src[k] moves into row dst[k]."""
    dead = np.asarray(dead).reshape(-1) != 0
    n = len(dead)
    m = n - int(dead.sum())
    rows = np.arange(n, dtype=np.uint32)
    dst = rows[:m][dead[:m]]
    src = rows[m:][~dead[m:]]
    assert len(src) == len(dst)
    return m, src, dst


def apply(keys_in_row_order, dead):
    """The row order after the erase: row r of the result holds this key."""
    keys = np.array(keys_in_row_order, copy=True)
    m, src, dst = plan(dead)
    keys[dst] = keys[src]
    return keys[:m]
