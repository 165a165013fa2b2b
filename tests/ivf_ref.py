"""numpy reference of the cluster-pruned (IVF) search's definition (csrc/ivf.hip header), independent
of the kernels: from an exact score matrix, the assignment of columns to lists, each user's probed
lists and the masked entries, the first K of (score descending, column ascending) over the eligible
columns, and the filler (-1, -inf) behind them."""
import numpy as np


def ivf_ref(S, assign, probe, K, masked=None):
    """S [B, N] scores; assign [N] the list of column c; probe [B, nprobe] the lists user b probes;
    masked [B, N] bool or None: True where history or a filter excludes the column (a score of
    -inf in S excludes it too). -> (cols int32 [B, K], vals fp32 [B, K])."""
    S = np.asarray(S, dtype=np.float32)
    assign = np.asarray(assign)
    probe = np.asarray(probe)
    B, N = S.shape
    cols = np.full((B, K), -1, np.int32)
    vals = np.full((B, K), -np.inf, np.float32)
    for b in range(B):
        ok = np.isin(assign, probe[b]) & (S[b] > -np.inf)
        if masked is not None:
            ok &= ~np.asarray(masked[b], dtype=bool)
        c = np.flatnonzero(ok)
        order = c[np.lexsort((c, -S[b, c].astype(np.float64)))][:K]   # last key first: -score, then column
        cols[b, :len(order)] = order
        vals[b, :len(order)] = S[b, order]
    return cols, vals


def work_item_count(probe, nlist):
    """The number of work items the grouping makes: per list, its (user, slot) pairs in tiles of 32."""
    counts = np.bincount(np.asarray(probe).reshape(-1), minlength=nlist)
    return int(((counts + 31) // 32).sum())
