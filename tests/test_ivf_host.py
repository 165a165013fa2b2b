"""Host side of the cluster-pruned (IVF) retrieval (csrc/ivf.hip, ops.ivf_topk, retrieval.IvfIndex),
no GPU: the new symbols, their argument checks (before any device call), the workspace query and
its work-item bound, IvfIndex.from_assignment on host tensors, and the numpy reference
(tests/ivf_ref.py) against a plain loop on a case written out by hand."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from ivf_ref import ivf_ref, work_item_count  # noqa: E402
from recommendsystemproject_amd import _hip, ops  # noqa: E402
from recommendsystemproject_amd.retrieval import ItemIndex, IvfIndex  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('rs_ivf_ws_bytes', 'rs_ivf_group', 'rs_ivf_scan', 'rs_ivf_merge')


def test_symbols_exist_and_header_and_binding_agree():
    L = _hip.lib()
    src = open(os.path.join(ROOT, 'include', 'rsys_hip.h')).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    for name in NEW:
        assert hasattr(L, name) and name in _hip.SIGNATURES
        decl = re.search(r'\b%s\s*\(([^;]*)\)\s*;' % name, src)
        assert decl, name
        assert len(decl.group(1).split(',')) == len(_hip.SIGNATURES[name][1]), name
    assert hasattr(ops, 'ivf_topk') and hasattr(ops, 'ivf_workspace')


# fake, aligned, never dereferenced: every check below fails before a device call
BIG = 1 << 40


def _group(probe=4096, ld=None, B=4, nprobe=3, nlist=7, K=10, ws=16384, ws_bytes=BIG):
    return _hip.call('rs_ivf_group', probe, nprobe if ld is None else ld, B, nprobe, nlist, K, ws, ws_bytes, None)


def _scan(U=4096, rows=8192, kind=1, exp=0, B=4, N=1000, D=64, ldi=None, K=10, perm=12288, off=20480, nlist=7,
          nprobe=3, fid=None, bits=None, fld=0, F=0, ws=16384, ws_bytes=BIG):
    return _hip.call('rs_ivf_scan', U, D, B, rows, kind, exp, D if ldi is None else ldi, N, D, K, perm, off, nlist,
                     nprobe, None, 0, None, None, 0, fid, 1, bits, fld, F, ws, ws_bytes, None)


def _merge(B=4, nprobe=3, nlist=7, K=10, ws=16384, ws_bytes=BIG, cols=4096, val=8192, ld=None):
    return _hip.call('rs_ivf_merge', B, nprobe, nlist, K, ws, ws_bytes, cols, val, K if ld is None else ld, None)


@pytest.mark.parametrize('fn', [_group, _scan, _merge])
def test_shared_size_checks_raise_without_a_device(fn):
    with pytest.raises(_hip.HipError, match=r'K = 0, must be in \[1, 256\]'):
        fn(K=0)
    with pytest.raises(_hip.HipError, match=r'K = 257, must be in \[1, 256\]'):
        fn(K=257)
    with pytest.raises(_hip.HipError, match='nlist = 0'):
        fn(nlist=0)
    with pytest.raises(_hip.HipError, match='nlist = 65537'):
        fn(nlist=65537, nprobe=1)
    with pytest.raises(_hip.HipError, match='nprobe = 0'):
        fn(nprobe=0)
    with pytest.raises(_hip.HipError, match='nprobe = 8'):
        fn(nprobe=8, nlist=7)
    with pytest.raises(_hip.HipError, match='nprobe = 257'):
        fn(nprobe=257, nlist=1000)
    with pytest.raises(_hip.HipError, match='B = -1'):
        fn(B=-1)
    with pytest.raises(_hip.HipError, match='pairs'):
        fn(B=1 << 24, nprobe=200, nlist=1000)
    with pytest.raises(_hip.HipError, match='workspace'):
        fn(ws=None)
    with pytest.raises(_hip.HipError, match='workspace'):
        fn(ws_bytes=ops.ivf_workspace(4, 3, 7, 10)[0] - 1)
    with pytest.raises(_hip.HipError, match='workspace'):
        fn(ws=16388)


def test_stage_checks_raise_without_a_device():
    with pytest.raises(_hip.HipError, match='null probe'):
        _group(probe=None)
    with pytest.raises(_hip.HipError, match='ld_probe'):
        _group(ld=2)
    for D in (20, 272, 8):
        with pytest.raises(_hip.HipError, match='multiple of 16'):
            _scan(D=D)
    with pytest.raises(_hip.HipError, match='bad sizes'):
        _scan(N=2 ** 31)
    with pytest.raises(_hip.HipError, match='bad sizes'):
        _scan(N=0)
    for bad in (dict(U=None), dict(rows=None), dict(perm=None), dict(off=None)):
        with pytest.raises(_hip.HipError, match='null'):
            _scan(**bad)
    with pytest.raises(_hip.HipError, match='16-byte aligned'):
        _scan(rows=8200)
    with pytest.raises(_hip.HipError, match='16-byte aligned'):
        _scan(ldi=68)              # bf16 rows: a stride that is no multiple of 8 elements
    with pytest.raises(_hip.HipError, match='16-byte aligned'):
        _scan(kind=2, ldi=72)
    with pytest.raises(_hip.HipError, match='ld >= D'):
        _scan(ldi=48)
    with pytest.raises(_hip.HipError, match='item_kind'):
        _scan(kind=3)
    with pytest.raises(_hip.HipError, match='item_exp'):
        _scan(kind=2, exp=41)
    with pytest.raises(_hip.HipError, match='null filter_bits'):
        _scan(fid=4096, F=2)
    with pytest.raises(_hip.HipError, match='filter_ld'):
        _scan(fid=4096, bits=8192, fld=31, F=2)       # 1000 columns: 32 words
    with pytest.raises(_hip.HipError, match='num_filters'):
        _scan(F=-1)
    with pytest.raises(_hip.HipError, match='null out_cols'):
        _merge(cols=None)
    with pytest.raises(_hip.HipError, match='null out_cols'):
        _merge(val=None)
    with pytest.raises(_hip.HipError, match='ld_out'):
        _merge(ld=9)


def test_ops_and_index_argument_errors_need_no_device():
    idx = ItemIndex.from_embeddings(torch.randn(50, 32))
    ivf = IvfIndex.from_assignment(idx, torch.randn(4, 32), torch.arange(50) % 4)
    with pytest.raises(_hip.HipError, match='MI355X only'):
        ivf.search(torch.randn(3, 32), 5, 2)
    with pytest.raises(ValueError, match='nprobe'):
        ivf.search(torch.randn(3, 32), 5, 5)
    with pytest.raises(ValueError, match='nprobe'):
        ivf.search(torch.randn(3, 32), 5, 0)
    with pytest.raises(ValueError, match='k = 257'):
        ivf.search(torch.randn(3, 32), 257, 2)
    with pytest.raises(TypeError):
        ivf.search(torch.randn(3, 32), 5, 2, oversample=2)      # not offered
    with pytest.raises(ValueError, match='filters given'):
        ivf.search(torch.randn(3, 32), 5, 2, filters=0)
    with pytest.raises(ValueError, match='keep_fp32'):
        IvfIndex.build(ItemIndex.from_embeddings(torch.randn(50, 32), dtype='bf16', keep_fp32=False), 4)
    with pytest.raises(ValueError, match='nlist'):
        IvfIndex.build(idx, 51)
    with pytest.raises(_hip.HipError, match='MI355X only'):
        IvfIndex.build(idx, 4)
    with pytest.raises(ValueError, match='assign'):
        IvfIndex.from_assignment(idx, torch.randn(4, 32), torch.arange(49) % 4)
    with pytest.raises(ValueError, match='outside'):
        IvfIndex.from_assignment(idx, torch.randn(4, 32), torch.arange(50) % 5)
    with pytest.raises(ValueError, match='centroids'):
        IvfIndex.from_assignment(idx, torch.randn(4, 16), torch.arange(50) % 4)
    with pytest.raises(ValueError, match='multiple of 16'):
        IvfIndex.from_assignment(ItemIndex.from_embeddings(torch.randn(50, 20)), torch.randn(4, 20), torch.arange(50) % 4)


def _bound(B, nprobe, nlist, K=10):
    nbytes, lay = ops.ivf_workspace(B, nprobe, nlist, K)
    assert lay[7] == nbytes and all(v % 16 == 0 for v in lay[1:])
    return nbytes, lay[0]


def test_workspace_and_bound_are_monotone():
    base = (64, 8, 100, 20)
    b0, w0 = _bound(*base)
    for i in range(4):
        prev = (b0, w0)
        for step in (1, 7, 50):
            a = list(base)
            a[i] += step
            if a[1] > a[2]:
                continue
            cur = _bound(*a)
            assert cur[0] >= prev[0] and cur[1] >= prev[1], (i, step)
            prev = cur
    # the parts do not overlap and hold what the header says
    B, nprobe, nlist, K = base
    _, lay = ops.ivf_workspace(*base)
    P = B * nprobe
    sizes = {1: P * K * 8, 2: lay[0] * 16, 3: P * 4, 4: nlist * 4, 5: (nlist + 1) * 4, 6: (nlist + 1) * 4}
    spans = sorted((lay[i], lay[i] + n) for i, n in sizes.items())
    assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:])) and spans[-1][1] <= lay[7]
    # nothing to do: the minimum, and a zeroed layout
    assert ops.ivf_workspace(0, 3, 7, 10) == (16, [0] * 8)
    assert _hip.lib().rs_ivf_ws_bytes(4, 3, 7, 10, None) == ops.ivf_workspace(4, 3, 7, 10)[0]


def test_bound_holds_against_a_brute_force_count():
    rng = np.random.default_rng(0)
    for B, nprobe, nlist in [(1, 1, 1), (70, 3, 7), (33, 7, 7), (100, 5, 40), (64, 1, 1000), (31, 2, 2), (32, 1, 5),
                             (257, 16, 50), (5, 4, 65536)]:
        _, bound = _bound(B, nprobe, nlist)
        assert bound == -(-B * nprobe // 32) + min(nlist, B * nprobe)
        for trial in range(7):
            if trial == 0:      # every pair in ONE list (a probe tensor with repeats; the grouping takes it)
                probe = np.full((B, nprobe), nlist - 1)
            elif trial == 1:    # every user probes the same lists
                probe = np.tile(np.arange(nprobe), (B, 1))
            elif trial == 2:    # spread as evenly as distinct lists allow
                probe = (np.arange(B)[:, None] * nprobe + np.arange(nprobe)[None, :]) % nlist
            else:
                probe = np.stack([rng.choice(nlist, nprobe, replace=False) for _ in range(B)])
            assert work_item_count(probe, nlist) <= bound, (B, nprobe, nlist, trial)


@pytest.mark.parametrize('dtype', ['fp32', 'bf16'])
def test_from_assignment_on_host_tensors(dtype):
    rng = np.random.default_rng(3)
    N, D, nlist = 500, 32, 9
    X = torch.from_numpy(rng.standard_normal((N, D)).astype(np.float32))
    base = ItemIndex.from_embeddings(X, torch.arange(1000, 1000 + N), dtype=dtype)
    assign = rng.integers(0, nlist, N)
    assign[assign == 4] = 5            # list 4 is empty
    assign[assign == 8] = 0            # and the last one
    ivf = IvfIndex.from_assignment(base, torch.randn(nlist, D), torch.from_numpy(assign))
    perm, off = ivf.perm.numpy(), ivf.list_off.numpy()
    assert ivf.perm.dtype == torch.int32 and ivf.list_off.dtype == torch.int32 and ivf.nlist == nlist
    assert np.array_equal(np.sort(perm), np.arange(N))                                  # a permutation
    assert np.array_equal(off, np.concatenate([[0], np.cumsum(np.bincount(assign, minlength=nlist))]))
    assert off[4] == off[5] and off[8] == off[9] == N
    for l in range(nlist):
        seg = perm[off[l]:off[l + 1]]
        assert np.all(assign[seg] == l) and np.all(np.diff(seg) > 0)                     # ascending columns
    assert ivf.rows_sorted.dtype == base._rows().dtype
    assert torch.equal(ivf.rows_sorted, base._rows()[ivf.perm.long()])
    assert np.array_equal(ivf.assign.numpy(), assign) and ivf.base is base and len(ivf) == N


def test_reference_on_a_case_written_out_by_hand():
    """6 users, 8 columns in 3 lists, K = 3. Lists: 0 = {0, 3, 6}, 1 = {1, 4}, 2 = {2, 5, 7}."""
    assign = np.array([0, 1, 2, 0, 1, 2, 0, 2])
    ninf = -np.inf
    S = np.array([
        [5, 9, 1, 5, 9, 1, 7, 0],      # user 0 probes 0, 1: 9 (col 1), 9 (col 4), 7 (col 6)
        [5, 9, 1, 5, 9, 1, 7, 0],      # user 1 probes 0 only: 7 (col 6), 5 (col 0), 5 (col 3)
        [4, 4, 4, 4, 4, 4, 4, 4],      # user 2 probes 1, 2: a tie across lists, by column: 1, 2, 4
        [1, 2, 3, 4, 5, 6, 7, 8],      # user 3 probes 1: two eligible columns only: 4, 1, filler
        [1, 2, 3, 4, 5, 6, 7, 8],      # user 4 probes 2, 0 with 7, 6 masked and 5 at -inf: 3 (col 3), 2, 0
        [1, 2, 3, 4, 5, 6, 7, 8],      # user 5 probes 1 with both masked: nothing
    ], dtype=np.float32)
    S[4, 5] = ninf
    probe = np.array([[0, 1], [0, 0], [1, 2], [1, 1], [2, 0], [1, 1]])
    masked = np.zeros(S.shape, bool)
    masked[4, [7, 6]] = True
    masked[5, [1, 4]] = True
    want_cols = np.array([[1, 4, 6], [6, 0, 3], [1, 2, 4], [4, 1, -1], [3, 2, 0], [-1, -1, -1]], np.int32)
    want_vals = np.array([[9, 9, 7], [7, 5, 5], [4, 4, 4], [5, 2, ninf], [4, 3, 1], [ninf, ninf, ninf]], np.float32)
    cols, vals = ivf_ref(S, assign, probe, 3, masked)
    assert cols.dtype == np.int32 and vals.dtype == np.float32
    assert np.array_equal(cols, want_cols) and np.array_equal(vals, want_vals)
    # and a plain python loop over (user, column)
    for b in range(6):
        cand = [(-float(S[b, c]), c) for c in range(8)
                if assign[c] in set(probe[b].tolist()) and not masked[b, c] and S[b, c] > ninf]
        cand.sort()
        loop = [c for _, c in cand[:3]] + [-1] * (3 - min(3, len(cand)))
        assert cols[b].tolist() == loop
    # without masks, and K past what any user has
    c8, v8 = ivf_ref(S, assign, probe, 8)
    assert c8[0].tolist() == [1, 4, 6, 0, 3, -1, -1, -1] and np.all(np.isneginf(v8[0, 5:]))
