"""Host side of hard-negative mining (csrc/sample.hip rs_sample_negatives, ops.sample_negatives,
retrieval.ItemIndex.mine_negatives), no GPU: the entry point exists in header, binding and library,
its argument checks run before any device call, ItemIndex.mine_negatives fails with ValueError (or,
on host tensors, with the no-CPU-fallback error), and the numpy mirror of the definition
(tests/mine_ref.py), which the GPU suite compares the kernel against, has the properties the
definition states, the uniformity of its draw included."""
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import mine_ref  # noqa: E402
from recommendsystemproject_amd import _hip  # noqa: E402
from recommendsystemproject_amd.retrieval import ItemIndex  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = np.float32(np.inf)


def test_entry_point_in_header_binding_and_library():
    header = open(os.path.join(ROOT, 'include', 'rsys_hip.h')).read()
    assert re.search(r'\bint rs_sample_negatives\(', header)
    assert 'rs_sample_negatives' in _hip.SIGNATURES
    assert hasattr(_hip.lib(), 'rs_sample_negatives')


def _sample(cand=4096, val=8192, ldc=None, B=4, C=32, ids=12288, N=1000, pos=16384, ps=1, skip=0, window=31, n=10,
            seed=0, draw=0, oid=20480, ocol=24576, ldo=None, cnt=28672):
    # fake, aligned, never dereferenced: every check below fails before a device call
    return _hip.call('rs_sample_negatives', cand, val, C if ldc is None else ldc, B, C, ids, N, pos, ps, skip, window,
                     n, seed, draw, oid, ocol, n if ldo is None else ldo, cnt, None)


def test_argument_checks_raise_without_a_device():
    for name in ('cand', 'val', 'ids', 'oid', 'ocol', 'cnt'):
        with pytest.raises(_hip.HipError, match='null'):
            _sample(**{name: None})
    with pytest.raises(_hip.HipError, match='C = 0'):
        _sample(C=0)
    with pytest.raises(_hip.HipError, match='C = 257'):
        _sample(C=257)
    with pytest.raises(_hip.HipError, match='skip = -1'):
        _sample(skip=-1)
    with pytest.raises(_hip.HipError, match='n = 0'):
        _sample(n=0)
    with pytest.raises(_hip.HipError, match=r'n = 32 outside \[1, window = 31\]'):
        _sample(n=32)
    with pytest.raises(_hip.HipError, match=r'skip \+ window = 256'):
        _sample(skip=100, window=156)
    with pytest.raises(_hip.HipError, match=r'skip \+ window = 256'):
        _sample(skip=0, window=256, n=256)
    with pytest.raises(_hip.HipError, match='ld_cand = 31'):
        _sample(ldc=31)
    with pytest.raises(_hip.HipError, match='ld_out = 9'):
        _sample(ldo=9)
    with pytest.raises(_hip.HipError, match='bad sizes'):
        _sample(N=0)
    with pytest.raises(_hip.HipError, match='bad sizes'):
        _sample(N=2 ** 31)
    with pytest.raises(_hip.HipError, match='bad sizes'):
        _sample(B=-1)
    # the full 64-bit range of seed and draw passes the binding (B = 0: nothing is launched)
    assert _sample(B=0, seed=2 ** 64 - 1, draw=2 ** 63 + 5, pos=None, ps=0) == 0


def _index(N=50, D=32, dtype='bf16', ids=None):
    return ItemIndex.from_embeddings(torch.randn(N, D), ids, dtype=dtype)


def test_mine_negatives_argument_errors_need_no_device():
    idx = _index()
    U = torch.randn(4, 32)
    with pytest.raises(ValueError, match='n = 11 outside'):
        idx.mine_negatives(U, 11, window=10)
    with pytest.raises(ValueError, match='n = 0 outside'):
        idx.mine_negatives(U, 0)
    with pytest.raises(ValueError, match=r'skip \+ window = 256'):
        idx.mine_negatives(U, 5, skip=200, window=56)
    with pytest.raises(ValueError, match='skip = -1'):
        idx.mine_negatives(U, 5, skip=-1)
    with pytest.raises(ValueError, match='3 positive items for 4 users'):
        idx.mine_negatives(U, 5, positive_item_ids=torch.arange(3))
    with pytest.raises(ValueError, match='set_filters'):
        idx.mine_negatives(U, 5, filters=0)
    with pytest.raises(ValueError, match='n = 51 outside'):     # window=None: min(255 - skip, N) = 50
        idx.mine_negatives(U, 51)
    wide = _index(D=20, dtype='fp32')
    with pytest.raises(ValueError, match='multiple of 16'):
        wide.mine_negatives(torch.randn(4, 20), 5)
    # valid arguments on host tensors: the no-CPU-fallback error
    with pytest.raises(_hip.HipError, match='MI355X only'):
        idx.mine_negatives(U, 5, positive_item_ids=torch.arange(4), skip=2, window=20)
    with pytest.raises(_hip.HipError, match='MI355X only'):
        idx.mine_negatives(U, 50)


def test_ops_sample_negatives_has_no_cpu_fallback():
    from recommendsystemproject_amd import ops
    cand = torch.zeros(2, 8, dtype=torch.int32)
    with pytest.raises(_hip.HipError, match='MI355X only'):
        ops.sample_negatives(cand, torch.zeros(2, 8), torch.arange(20), None, 0, 7, 3)


# ---------------------------------------------------------------- the mirror

def test_hash_is_the_librarys_construction():
    # mix64 / fmix32 of rng.h (splitmix64's and murmur3's finalisers): published test values
    assert mine_ref.mix64(0) == 0
    assert mine_ref.fmix32(0) == 0
    assert mine_ref.mix64(0x9e3779b97f4a7c15) == 0xe220a8397b1dcdaf    # splitmix64's first output from state 0
    assert mine_ref.fmix32(1) == 0x514e28b7
    cols = np.array([0, 1, 77, 2 ** 31 - 1])
    for b in (0, 3, 4095):
        want = [mine_ref.key(11, 5, b, int(c)) for c in cols]
        assert [int(k) for k in mine_ref.keys_of(11, 5, b, cols)] == want
        assert all(k & 0xffffffff == int(c) for k, c in zip(want, cols))


@pytest.mark.parametrize('E,skip,window,n,want', [
    (300, 0, 255, 10, (0, 255)),      # more eligible than the window: the window as asked
    (256, 100, 155, 10, (100, 255)),
    (120, 100, 155, 10, (100, 120)),  # the window's tail is missing, it still holds n: no slide
    (105, 100, 155, 10, (95, 105)),   # 5 left past skip: slides up just far enough for n
    (100, 100, 155, 10, (90, 100)),   # E == skip
    (50, 100, 155, 10, (40, 50)),     # E < skip
    (7, 100, 155, 10, (0, 7)),        # E < n: everything, P = 7
    (7, 0, 31, 10, (0, 7)),
    (0, 0, 31, 10, (0, 0)),           # P = 0
    (0, 5, 31, 10, (0, 0)),
    (40, 0, 1, 1, (0, 1)),
    (40, 39, 1, 1, (39, 40)),
    (40, 40, 1, 1, (39, 40)),
])
def test_pool_bounds(E, skip, window, n, want):
    assert mine_ref.pool_bounds(E, skip, window, n) == want


def _lists(rows):
    """Hand-written candidate lists [(col, val), ...] per user, padded to one width with (-1, -inf)."""
    C = max(len(r) for r in rows)
    cand = np.full((len(rows), C), -1, np.int32)
    val = np.full((len(rows), C), -INF, np.float32)
    for b, r in enumerate(rows):
        for j, (c, v) in enumerate(r):
            cand[b, j], val[b, j] = c, v
    return cand, val


def test_mirror_short_pools_and_cyclic_fill():
    item_ids = np.arange(100, 120)
    rows = [[(c, 10.0 - c) for c in range(12)],                             # 12 eligible
            [(3, 5.0), (7, 4.0), (9, 3.0)],                                 # E = 3 < n
            [(3, 5.0), (7, -INF), (9, -INF)],                               # one eligible
            [(3, -INF), (7, -INF)],                                         # none: P = 0
            [(25, 5.0), (-4, 4.0), (2, 3.0)]]                               # columns outside [0, N)
    cand, val = _lists(rows)
    ids, cols, count = mine_ref.np_sample(cand, val, item_ids, None, skip=2, window=6, n=4, seed=1, draw=0)
    assert count.tolist() == [4, 3, 1, 0, 1]
    assert set(cols[0]) <= set(range(2, 8)) and len(set(cols[0])) == 4      # positions 2 .. 7
    assert sorted(cols[1][:3]) == [3, 7, 9] and cols[1][3] == cols[1][0]    # all three, then the first again
    assert cols[2].tolist() == [3, 3, 3, 3]
    assert cols[3].tolist() == [-1] * 4 and ids[3].tolist() == [-1] * 4
    assert cols[4].tolist() == [2, 2, 2, 2]
    assert np.array_equal(ids[:3], cols[:3] + 100)
    # ascending key order
    for b in (0, 1):
        k = [mine_ref.key(1, 0, b, int(c)) for c in cols[b][:count[b]]]
        assert k == sorted(k)
    # a pure function: the same call again, and another draw
    again = mine_ref.np_sample(cand, val, item_ids, None, skip=2, window=6, n=4, seed=1, draw=0)
    assert all(np.array_equal(x, y) for x, y in zip((ids, cols, count), again))
    other = mine_ref.np_sample(cand, val, item_ids, None, skip=2, window=6, n=4, seed=1, draw=1)
    assert not np.array_equal(other[1][0], cols[0]) or not np.array_equal(other[1][1], cols[1])


def test_mirror_excludes_every_column_of_the_positive_id():
    item_ids = np.array([5, 9, 5, 7, 5, 8, 6, 9])           # id 5 in columns 0, 2, 4; id 9 in 1, 7
    rows = [[(c, 20.0 - c) for c in range(8)]] * 3
    cand, val = _lists(rows)
    pos = np.array([5, 9, 1000])                             # the third user's positive is not in the catalog
    ids, cols, count = mine_ref.np_sample(cand, val, item_ids, pos, skip=0, window=8, n=8, seed=3, draw=2)
    assert count.tolist() == [5, 6, 8]
    assert set(cols[0]) == {1, 3, 5, 6, 7} and 5 not in ids[0]
    assert set(cols[1]) == {0, 2, 3, 4, 5, 6} and 9 not in ids[1]
    assert sorted(cols[2]) == list(range(8))
    # with the positive sitting above the window, the window moves down by one eligible position
    ids, cols, count = mine_ref.np_sample(cand, val, item_ids, np.array([5, 5, 5]), skip=1, window=2, n=2)
    assert set(cols[0]) == {3, 5}                            # eligible: 1, 3, 5, 6, 7 -> positions 1, 2


def test_np_mine_takes_candidates_in_search_order():
    S = np.array([[1.0, 3.0, 3.0, -INF, 2.0, 0.0],
                  [0.0, 0.0, 0.0, 0.0, 0.0, 0.0]], np.float32)
    cand, val = mine_ref.np_candidates(S, 5)
    assert cand.tolist() == [[1, 2, 4, 0, 5], [0, 1, 2, 3, 4]]
    ids, cols, count = mine_ref.np_mine(S, np.arange(6) + 10, np.array([12, 10]), 1, 2, 2, 0, 0, 5)
    assert sorted(cols[0]) == [0, 4] and sorted(cols[1]) == [2, 3]     # eligible 1,4,0,5 / 1,2,3,4
    assert count.tolist() == [2, 2]


@pytest.mark.parametrize('P,n', [(20, 5), (255, 8), (3, 1)])
def test_draw_is_uniform(P, n):
    """Every pool member is selected T n / P times within 6 binomial standard deviations, for each
    of 8 users over T = 2000 draws. The key is deterministic, so this cannot flake."""
    T, users = 2000, 8
    pool = np.arange(1000, 1000 + 7 * P, 7)                 # P distinct columns
    for b in range(users):
        hits = np.zeros(P, np.int64)
        for draw in range(T):
            k = mine_ref.keys_of(12345, draw, b, pool)
            hits[np.argpartition(k, n - 1)[:n]] += 1
        p = n / P
        sigma = np.sqrt(T * p * (1 - p))
        worst = np.abs(hits - T * p).max() / sigma
        assert worst <= 6.0, (b, worst)
