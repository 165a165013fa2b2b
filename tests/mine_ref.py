"""numpy mirror of rs_sample_negatives' definition (include/rsys_hip.h, csrc/sample.hip), shared by
test_mine_negatives_host.py and test_gpu_mine_negatives.py: the hash in Python integers, the pool
rule, the draw, and np_mine = np_topk's order on an exact masked score matrix followed by them."""
import numpy as np

M64 = (1 << 64) - 1
M32 = (1 << 32) - 1


def mix64(z):
    z &= M64
    z = ((z ^ (z >> 30)) * 0xbf58476d1ce4e5b9) & M64
    z = ((z ^ (z >> 27)) * 0x94d049bb133111eb) & M64
    return z ^ (z >> 31)


def fmix32(h):
    h &= M32
    h ^= h >> 16
    h = (h * 0x85ebca6b) & M32
    h ^= h >> 13
    h = (h * 0xc2b2ae35) & M32
    return h ^ (h >> 16)


def stream_keys(seed, draw, b):
    base = mix64((seed & M64) ^ mix64(((draw & M64) * 0x9e3779b97f4a7c15 + b * 0xd1b54a32d192ed03) & M64))
    return base & M32, base >> 32


def key(seed, draw, b, col):
    """(h << 32) | col of pool member `col` of user row b."""
    k0, k1 = stream_keys(seed, draw, b)
    return ((fmix32((col & M32) ^ k0) ^ k1) << 32) | (col & M32)


def fmix32_array(h):
    """fmix32 of a uint64 array holding 32-bit values, vectorised -> uint64 array."""
    h = h ^ (h >> np.uint64(16))
    h = (h * np.uint64(0x85ebca6b)) & np.uint64(M32)
    h = h ^ (h >> np.uint64(13))
    h = (h * np.uint64(0xc2b2ae35)) & np.uint64(M32)
    return h ^ (h >> np.uint64(16))


def keys_of(seed, draw, b, cols):
    """key() of an int array of columns (0 <= col < 2^31), vectorised -> uint64 array."""
    k0, k1 = stream_keys(seed, draw, b)
    h = fmix32_array(np.asarray(cols, dtype=np.uint64) ^ np.uint64(k0)) ^ np.uint64(k1)
    return (h << np.uint64(32)) | np.asarray(cols, dtype=np.uint64)


def pool_bounds(E, skip, window, n):
    """(lo, hi) of the pool among E eligible positions."""
    hi = min(skip + window, E)
    lo = min(skip, max(hi - n, 0))
    return lo, hi


def np_sample(cand, cand_val, item_ids, pos_ids, skip, window, n, seed=0, draw=0):
    """The definition on candidate lists cand / cand_val [B, C] -> (ids int64 [B, n], cols int32
    [B, n], count int32 [B]); pos_ids None or [B]."""
    cand, cand_val = np.asarray(cand), np.asarray(cand_val)
    item_ids = np.asarray(item_ids, dtype=np.int64)
    B, N = cand.shape[0], len(item_ids)
    ids = np.full((B, n), -1, np.int64)
    cols = np.full((B, n), -1, np.int32)
    count = np.zeros(B, np.int32)
    for b in range(B):
        c, v = cand[b].astype(np.int64), cand_val[b]
        ok = (v > -np.inf) & (c >= 0) & (c < N)
        if pos_ids is not None:
            ok &= item_ids[np.where(ok, c, 0)] != int(pos_ids[b])
        elig = c[ok]                                    # candidate order
        lo, hi = pool_bounds(len(elig), skip, window, n)
        pool = elig[lo:hi]
        P = len(pool)
        count[b] = min(P, n)
        if P == 0:
            continue
        order = pool[np.argsort(keys_of(seed, draw, b, pool), kind='stable')]
        take = order[np.arange(n) % P]
        cols[b] = take
        ids[b] = item_ids[take]
    return ids, cols, count


def np_candidates(S_masked, C):
    """The first C entries of search's order on masked scores: value descending, ties by the lower
    column (np_topk of the retrieval suites)."""
    order = np.argsort(-S_masked, axis=1, kind='stable')[:, :C]
    return order.astype(np.int32), np.take_along_axis(S_masked, order, axis=1).astype(np.float32)


def np_mine(S_masked, item_ids, pos_ids, skip, window, n, seed, draw, C):
    cand, val = np_candidates(S_masked, C)
    return np_sample(cand, val, item_ids, pos_ids, skip, window, n, seed, draw)
