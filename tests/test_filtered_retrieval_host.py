"""Host side of the catalog filters (csrc/retrieve.hip rs_pack_mask / rs_fused_topk_filtered /
rs_target_rank_filtered, retrieval.ItemIndex.set_filters), no GPU: the three entry points exist in
header, binding and library, their argument checks run before any device call, and ItemIndex's
filter arguments fail with ValueError (or, on host tensors, with the no-CPU-fallback error)."""
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from recommendsystemproject_amd import _hip  # noqa: E402
from recommendsystemproject_amd.retrieval import ItemIndex  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('rs_pack_mask', 'rs_fused_topk_filtered', 'rs_target_rank_filtered')


def test_new_entry_points_in_header_binding_and_library():
    header = open(os.path.join(ROOT, 'include', 'rsys_hip.h')).read()
    L = _hip.lib()
    for name in NEW:
        assert re.search(r'\bint %s\(' % name, header), name
        assert name in _hip.SIGNATURES, name
        assert hasattr(L, name), name


def _topk(U=4096, items=8192, B=4, N=1000, D=64, ldi=None, K=10, kind=0, exp=0, fids=20480, bits=24576,
          fld=None, F=3, splits=1, ws=None, ws_bytes=0, out=12288):
    # fake, aligned, never dereferenced: every check below fails before a device call
    return _hip.call('rs_fused_topk_filtered', U, D, B, items, kind, exp, D if ldi is None else ldi, N, D, K,
                     None, 0, None, None, 0, fids, 1, bits, (N + 31) // 32 if fld is None else fld, F, splits, ws,
                     ws_bytes, out, None, K, None)


def _rank(U=4096, items=8192, B=4, N=1000, D=64, ldi=None, kind=0, exp=0, tc=16384, fids=20480, bits=24576,
          fld=None, F=3, splits=1, ws=None, ws_bytes=0, out=12288):
    return _hip.call('rs_target_rank_filtered', U, D, B, items, kind, exp, D if ldi is None else ldi, N, D, tc, 1,
                     None, 0, None, None, 0, fids, 1, bits, (N + 31) // 32 if fld is None else fld, F, splits, ws,
                     ws_bytes, out, None)


@pytest.mark.parametrize('call', [_topk, _rank])
def test_filter_argument_checks_raise_without_a_device(call):
    with pytest.raises(_hip.HipError, match='filter_ld'):
        call(N=1000, fld=31)         # 1000 columns are 32 words
    with pytest.raises(_hip.HipError, match='filter_ld'):
        call(N=1025, fld=32)
    with pytest.raises(_hip.HipError, match='filter_bits'):
        call(bits=None)
    with pytest.raises(_hip.HipError, match='num_filters'):
        call(F=-1)
    with pytest.raises(_hip.HipError, match='item_kind'):
        call(kind=3)
    with pytest.raises(_hip.HipError, match='item_kind'):
        call(kind=-1)
    with pytest.raises(_hip.HipError, match='item_exp'):
        call(kind=2, exp=41)
    with pytest.raises(_hip.HipError, match='item_exp'):
        call(kind=2, exp=-41)


def test_fused_topk_filtered_keeps_the_old_checks_and_messages():
    with pytest.raises(_hip.HipError, match='multiple of 16'):
        _topk(D=20)
    with pytest.raises(_hip.HipError, match='multiple of 16'):
        _topk(D=272)
    with pytest.raises(_hip.HipError, match='K <= min'):
        _topk(K=257)
    with pytest.raises(_hip.HipError, match='K <= min'):
        _topk(N=5, K=10)
    with pytest.raises(_hip.HipError, match='workspace'):
        _topk(splits=2, ws=16384, ws_bytes=4 * 2 * 10 * 8 - 1)
    with pytest.raises(_hip.HipError, match='workspace'):
        _topk(splits=2, ws=None, ws_bytes=1 << 20)
    with pytest.raises(_hip.HipError, match='null'):
        _topk(U=None)
    with pytest.raises(_hip.HipError, match='fewer than K'):
        _topk(N=25, K=10, splits=3, ws=16384, ws_bytes=1 << 20)
    with pytest.raises(_hip.HipError, match='16-byte aligned'):
        _topk(kind=2, D=64, ldi=72)   # e4m3: a byte stride that is no multiple of 16
    with pytest.raises(_hip.HipError, match='16-byte aligned'):
        _topk(kind=1, D=64, ldi=68)   # bf16: no multiple of 8 elements


def test_target_rank_filtered_keeps_the_old_checks_and_messages():
    with pytest.raises(_hip.HipError, match='multiple of 16'):
        _rank(D=24)
    with pytest.raises(_hip.HipError, match='ld >= D'):
        _rank(ldi=60)
    with pytest.raises(_hip.HipError, match='workspace'):
        _rank(splits=2, ws=20480, ws_bytes=4 * 2 * 4 - 1)
    with pytest.raises(_hip.HipError, match='null'):
        _rank(tc=None)
    with pytest.raises(_hip.HipError, match='bad sizes'):
        _rank(N=2 ** 31)
    with pytest.raises(_hip.HipError, match='no column'):
        _rank(N=5, splits=8, ws=20480, ws_bytes=1 << 20)


def test_pack_mask_argument_checks_raise_without_a_device():
    def pack(mask=4096, ld=1000, F=2, N=1000, bits=8192, ldb=32):
        return _hip.call('rs_pack_mask', mask, ld, F, N, bits, ldb, None)
    with pytest.raises(_hip.HipError, match='null'):
        pack(mask=None)
    with pytest.raises(_hip.HipError, match='null'):
        pack(bits=None)
    with pytest.raises(_hip.HipError, match='F = 0'):
        pack(F=0)
    with pytest.raises(_hip.HipError, match='bad sizes'):
        pack(N=0, ld=0)
    with pytest.raises(_hip.HipError, match='bad sizes'):
        pack(N=2 ** 31, ld=2 ** 31, ldb=2 ** 26)
    with pytest.raises(_hip.HipError, match='ld = 999'):
        pack(ld=999)
    with pytest.raises(_hip.HipError, match='ld_bits = 31'):
        pack(ldb=31)


def test_the_filtered_calls_keep_the_split_count_of_the_queries():
    # a filtered call moves split boundaries onto filter words but never changes how many splits
    # there are, so rs_fused_topk_splits / _ws_bytes describe it as they describe the unfiltered
    # call; with too small a workspace for that count the call itself says so
    from test_retrieval_host import SHAPES
    L = _hip.lib()
    for B, N, D, K in SHAPES:
        s = L.rs_fused_topk_splits(B, N, D, K)
        assert N // s >= K
        if s > 1:
            need = L.rs_fused_topk_ws_bytes(B, N, D, K, 0)
            with pytest.raises(_hip.HipError, match=f'needs {need} '):
                _topk(B=B, N=N, D=D, K=K, splits=0, ws=16384, ws_bytes=need - 1)


def _index(N=50, D=32, dtype='bf16', ids=None):
    return ItemIndex.from_embeddings(torch.randn(N, D), ids, dtype=dtype)


def test_set_filters_shape_and_dtype_errors():
    idx = _index()
    with pytest.raises(ValueError, match='N = 50'):
        idx.set_filters(torch.ones(49, dtype=torch.bool))
    with pytest.raises(ValueError, match='N = 50'):
        idx.set_filters(np.ones((2, 51), dtype=np.uint8))
    with pytest.raises(ValueError, match='N = 50'):
        idx.set_filters(torch.ones(2, 5, 10, dtype=torch.bool))
    with pytest.raises(ValueError, match='N = 50'):
        idx.set_filters(torch.ones(0, 50, dtype=torch.bool))
    with pytest.raises(ValueError, match='bool or uint8'):
        idx.set_filters(torch.ones(50))
    with pytest.raises(ValueError, match="'b' has 49"):
        idx.set_filters({'a': np.ones(50, dtype=bool), 'b': np.ones(49, dtype=bool)})
    with pytest.raises(ValueError, match='empty'):
        idx.set_filters({})
    assert idx.num_filters == 0


def test_filters_argument_errors_need_no_device():
    idx = _index()
    U = torch.randn(4, 32)
    with pytest.raises(ValueError, match='set_filters'):
        idx.search(U, 5, filters=0)
    with pytest.raises(ValueError, match='set_filters'):
        idx.rank(U, torch.arange(4), filters=0)
    rng = np.random.default_rng(0)
    masks = rng.random((3, 50)) < 0.5
    idx.set_filters(masks)
    assert idx.num_filters == 3
    # the words an index keeps: little-endian bit order, as rs_pack_mask's
    want = np.packbits(masks, axis=1, bitorder='little')
    want = np.pad(want, ((0, 0), (0, 8 - want.shape[1]))).view('<u4')
    assert np.array_equal(idx._filters.numpy(), want)
    for bad in (3, -1, 'in_stock'):
        with pytest.raises(ValueError, match='filter'):
            idx.search(U, 5, filters=bad)
        with pytest.raises(ValueError, match='filter'):
            idx.rank(U, torch.arange(4), filters=bad)
    with pytest.raises(ValueError, match='integer tensor'):
        idx.search(U, 5, filters=torch.zeros(3, dtype=torch.int32))     # 3 ids for 4 users
    with pytest.raises(ValueError, match='integer tensor'):
        idx.search(U, 5, filters=torch.zeros(4))                        # floating point
    idx.set_filters({'in_stock': masks[0], 'kids': torch.from_numpy(masks[1])})
    assert idx.num_filters == 2
    with pytest.raises(ValueError, match='unknown filter'):
        idx.search(U, 5, filters='adults')
    with pytest.raises(ValueError, match='out of range'):
        idx.search(U, 5, filters=2)
    # a valid filter on host tensors: the no-CPU-fallback error, not a silent unfiltered answer
    for f in (0, 'kids', torch.tensor([0, 1, -1, 0])):
        with pytest.raises(_hip.HipError, match='MI355X only'):
            idx.search(U, 5, filters=f)
        with pytest.raises(_hip.HipError, match='MI355X only'):
            idx.rank(U, torch.arange(4), filters=f)
    idx.set_filters(None)
    assert idx.num_filters == 0
    with pytest.raises(ValueError, match='set_filters'):
        idx.search(U, 5, filters='kids')


def test_filters_need_a_width_the_fused_kernels_take():
    idx = _index(D=20, dtype='fp32')    # searchable through the staged path, which has no filters
    idx.set_filters(torch.ones(50, dtype=torch.bool))
    with pytest.raises(ValueError, match='multiple of 16'):
        idx.search(torch.randn(4, 20), 5, filters=0)
    with pytest.raises(ValueError, match='multiple of 16'):
        idx.rank(torch.randn(4, 20), torch.arange(4), filters=0)


def test_mask_of_matches_isin():
    ids = np.array([7, 3, 9, 3, 11, 20, 5, 9, 9, 1])     # 3 twice, 9 three times
    idx = _index(N=10, ids=torch.from_numpy(ids))
    for q in ([3], [9, 1], [4], [3, 4, 20, 100], [], list(ids)):
        got = idx.mask_of(torch.tensor(q, dtype=torch.int64))
        assert got.dtype == torch.bool and got.shape == (10,)
        assert np.array_equal(got.numpy(), np.isin(ids, np.array(q, dtype=np.int64))), q
    assert idx.mask_of(np.array([[3], [5]])).sum().item() == 3   # any shape of ids
    idx.set_filters(idx.mask_of([9, 7]))
    assert idx.num_filters == 1
    assert int(idx._filters.view(torch.int32)[0, 0]) == 0b0110000101
