"""Host side of the full-catalog ranking metrics (csrc/retrieve.hip rs_target_rank, retrieval.py,
training_utils.ranking_metrics), no GPU: the metrics against values written out by hand, the split
choice and workspace size, rs_target_rank's argument checks (which run before any device call),
the id -> column map, and the no-CPU-fallback rule."""
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from recommendsystemproject_amd import _hip  # noqa: E402
from recommendsystemproject_amd.project.utils.training_utils import ranking_metrics  # noqa: E402
from recommendsystemproject_amd.retrieval import ItemIndex  # noqa: E402


def test_ranking_metrics_hand_written():
    m = ranking_metrics(torch.tensor([0, 1, 9, 10, -1, 299], dtype=torch.int32), [1, 10, 300])
    n = 6
    assert m['num_samples'] == 6 and m['num_ranked'] == 5
    assert m['recall@1'] == 1 / n and m['recall@10'] == 3 / n and m['recall@300'] == 5 / n
    # gains 1 / log2(r + 2): r = 0 -> 1, 1 -> 1 / log2 3, 9 -> 1 / log2 11, 10 -> 1 / log2 12, 299 -> 1 / log2 301
    g = [1.0, 1 / math.log2(3), 1 / math.log2(11), 1 / math.log2(12), 1 / math.log2(301)]
    assert m['ndcg@1'] == pytest.approx(g[0] / n, abs=1e-15)
    assert m['ndcg@10'] == pytest.approx(sum(g[:3]) / n, abs=1e-15)
    assert m['ndcg@300'] == pytest.approx(sum(g) / n, abs=1e-15)
    assert m['mrr'] == pytest.approx((1 + 1 / 2 + 1 / 10 + 1 / 11 + 1 / 300) / n, abs=1e-15)
    assert m['mean_rank'] == (1 + 2 + 10 + 11 + 300) / 5
    for k in (1, 10, 300):
        assert m[f'ndcg@{k}'] <= m[f'recall@{k}']
    # the order of the samples does not matter, nor does their shape or integer dtype
    m2 = ranking_metrics(torch.tensor([[299, -1, 10], [9, 1, 0]]), (1, 10, 300))
    assert m2 == pytest.approx(m, abs=1e-15)
    assert all(m2[k] == m[k] for k in ('recall@1', 'recall@10', 'recall@300', 'mean_rank', 'num_ranked'))


def test_ranking_metrics_without_a_ranked_sample():
    m = ranking_metrics(torch.full((4,), -1, dtype=torch.int32), [1, 10])
    assert m['num_samples'] == 4 and m['num_ranked'] == 0
    assert m['recall@1'] == 0 and m['recall@10'] == 0 and m['ndcg@1'] == 0 and m['ndcg@10'] == 0 and m['mrr'] == 0
    assert math.isnan(m['mean_rank'])
    e = ranking_metrics(torch.zeros(0, dtype=torch.int32), [5])
    assert e['num_samples'] == 0 and e['recall@5'] == 0 and e['mrr'] == 0


SHAPES = [(1, 1, 16), (37, 7, 16), (64, 1000, 64), (4096, 3706, 64), (4096, 10 ** 6, 128), (64, 10 ** 6, 128),
          (4096, 10 ** 7, 128), (19, 4096, 256), (1, 4095, 16), (1, 4096, 16), (4096, 2 ** 31 - 1, 256)]


@pytest.mark.parametrize('B,N,D', SHAPES)
def test_splits_keep_2048_columns(B, N, D):
    L = _hip.lib()
    s = L.rs_target_rank_splits(B, N, D)
    assert s >= 1
    if s > 1:
        assert N // s >= 2048
    assert L.rs_target_rank_ws_bytes(B, N, D, 0) == L.rs_target_rank_ws_bytes(B, N, D, s)
    prev = 0
    for f in (1, 2, 3, 8, 64):
        w = L.rs_target_rank_ws_bytes(B, N, D, f)
        assert w >= 16 and w >= prev
        if f > 1:
            assert w >= B * f * 4  # an int32 partial count per split and user
        prev = w


def test_splits_of_small_and_large_catalogs():
    L = _hip.lib()
    assert L.rs_target_rank_splits(1, 1, 16) == 1
    assert L.rs_target_rank_splits(4096, 4095, 64) == 1
    assert L.rs_target_rank_splits(4096, 10 ** 6, 128) > 1
    assert L.rs_target_rank_splits(64, 10 ** 6, 128) > L.rs_target_rank_splits(4096, 10 ** 6, 128)


def _call(U=4096, items=8192, B=4, N=1000, D=64, ldi=None, tc=16384, splits=1, ws=None, ws_bytes=0, out=12288):
    # fake, aligned, never dereferenced: every check below fails before a device call
    return _hip.call('rs_target_rank', U, D, B, items, 0, D if ldi is None else ldi, N, D, tc, 1, None, 0, None,
                     None, 0, splits, ws, ws_bytes, out, None)


def test_bad_arguments_raise_without_a_device():
    with pytest.raises(_hip.HipError, match='multiple of 16'):
        _call(D=24)
    with pytest.raises(_hip.HipError, match='multiple of 16'):
        _call(D=272)
    with pytest.raises(_hip.HipError, match='ld >= D'):
        _call(ldi=60)
    with pytest.raises(_hip.HipError, match='workspace'):
        _call(splits=2, ws=20480, ws_bytes=4 * 2 * 4 - 1)
    with pytest.raises(_hip.HipError, match='workspace'):
        _call(splits=2, ws=None, ws_bytes=1 << 20)
    with pytest.raises(_hip.HipError, match='null'):
        _call(tc=None)
    with pytest.raises(_hip.HipError, match='null'):
        _call(out=None)
    with pytest.raises(_hip.HipError, match='bad sizes'):
        _call(N=2 ** 31)
    with pytest.raises(_hip.HipError, match='no column'):
        _call(N=5, splits=8, ws=20480, ws_bytes=1 << 20)


def test_columns_of_maps_ids_to_columns():
    ids = torch.tensor([5, 9, 7, 9, 2, 100])  # 9 twice: its last column wins
    index = ItemIndex.from_embeddings(torch.randn(6, 16), ids)
    got = index.columns_of(torch.tensor([[9, 5], [3, 100], [2, 101]]))
    assert got.dtype == torch.int32 and got.tolist() == [[3, 0], [-1, 5], [4, -1]]
    assert index.columns_of(torch.tensor([0, -7])).tolist() == [-1, -1]
    assert index.columns_of(torch.zeros(0, dtype=torch.int64)).shape == (0,)
    perm = torch.randperm(500) + 100
    index = ItemIndex.from_embeddings(torch.randn(500, 16), perm)
    assert torch.equal(index.columns_of(perm).long(), torch.arange(500))
    assert torch.equal(perm[index.columns_of(perm[::7]).long()], perm[::7])


def test_rank_on_cpu_tensors_fails_loudly():
    from recommendsystemproject_amd import ops
    index = ItemIndex.from_embeddings(torch.randn(50, 32), dtype='bf16')
    with pytest.raises(_hip.HipError, match='MI355X only'):
        index.rank(torch.randn(4, 32), torch.arange(4))
    with pytest.raises(_hip.HipError, match='MI355X only'):
        ops.target_rank(torch.randn(4, 32), torch.randn(50, 32), torch.arange(4, dtype=torch.int32))
