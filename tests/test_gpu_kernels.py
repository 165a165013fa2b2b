"""Per-kernel numerics on the GPU against plain PyTorch fp32 references of the same op
(index work bit-exact)."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from recommendsystemproject_amd import _hip, ops
from recommendsystemproject_amd.functions import _seg

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')


def rnd(*shape, seed=0):
    g = torch.Generator(device='cpu').manual_seed(seed)
    return torch.randn(*shape, generator=g).to(DEV)


@pytest.mark.parametrize('M,N,K', [(1, 1, 1), (5, 7, 3), (64, 64, 64), (130, 70, 40), (4096, 128, 128),
                                   (3000, 192, 64), (192, 64, 20000)])
@pytest.mark.parametrize('ta,tb', [(0, 0), (0, 1), (1, 0), (1, 1)])
def test_gemm_transposes(M, N, K, ta, tb):
    A = rnd(K, M, seed=1) if ta else rnd(M, K, seed=1)
    B = rnd(N, K, seed=2) if tb else rnd(K, N, seed=2)
    C = torch.empty(M, N, device=DEV)
    ops.gemm(A, B, C, M, N, K, transA=ta, transB=tb, lda=A.stride(0), ldb=B.stride(0), ldc=N)
    ref = (A.t() if ta else A).double() @ (B.t() if tb else B).double()
    err = (C.double() - ref).abs().max().item()
    assert err <= 1e-5 * math.sqrt(K) * max(1.0, ref.abs().max().item()), err


@pytest.mark.parametrize('M,N,K', [(777, 96, 64), (5000, 256, 64), (5003, 64, 256), (4096, 192, 64),
                                   (6000, 40, 64), (6000, 64, 40), (4100, 64, 192), (6000, 72, 64),
                                   (6000, 64, 72), (40000, 72, 64), (40000, 64, 72)])
def test_gemm_epilogues_and_split(M, N, K):
    x, W, b = rnd(M, K, seed=3), rnd(N, K, seed=4), rnd(N, seed=5)
    pos = rnd(13, N, seed=6)
    tol = 1e-4 * max(1.0, K / 64)
    y = ops.linear_fwd(x, W, b, aux=pos, aux_mod=13)
    ref = x @ W.t() + b + pos[torch.arange(M, device=DEV) % 13]
    assert torch.allclose(y, ref, atol=tol, rtol=1e-5)
    y = ops.linear_fwd(x, W, b, relu=True)
    assert torch.allclose(y, torch.relu(x @ W.t() + b), atol=tol, rtol=1e-5)
    y2 = rnd(M, N, seed=13)
    ref2 = 0.5 * y2 + x @ W.t()
    ops.linear_fwd(x, W, None, out=y2, beta=0.5)
    assert torch.allclose(y2, ref2, atol=tol, rtol=1e-5)
    dy = rnd(M, N, seed=7)
    mask_src = rnd(M, K, seed=11)
    dx = ops.linear_bwd_input(dy, W, relu_mask_of=mask_src, alpha=2.0)
    assert torch.allclose(dx, 2.0 * (dy @ W) * (mask_src > 0), atol=2 * tol, rtol=1e-5)
    dW = rnd(N, K, seed=8)
    db = rnd(N, seed=12)
    ref, refb = dW + dy.t() @ x, db + dy.sum(0)
    ops.linear_bwd_weight(dy, x, dW, beta=1.0, db=db)
    assert torch.allclose(dW, ref, atol=1e-3 * max(1, M / 1000), rtol=1e-5)
    assert torch.allclose(db, refb, atol=1e-3 * max(1, M / 1000), rtol=1e-5)
    for split in (1, 3, 16):
        C = torch.zeros(N, K, device=DEV)
        rs = torch.zeros(N, device=DEV)
        ops.gemm(dy, x, C, N, K, M, transA=1, transB=0, lda=N, ldb=K, ldc=K, split=split, rowsum=rs)
        assert torch.allclose(C, dy.t() @ x, atol=1e-3 * max(1, M / 1000), rtol=1e-5), split
        assert torch.allclose(rs, dy.sum(0), atol=1e-3 * max(1, M / 1000), rtol=1e-5), split


@pytest.mark.parametrize('Mo,No', [(64, 64), (64, 256), (256, 64), (192, 64), (64, 40), (128, 128), (64, 72), (80, 64), (64, 100),
                                   (256, 192), (256, 172)])
def test_wgrad_streaming_kernel(Mo, No):
    """dW = dY^T X over a long M (wgrad path) incl. fused bias sums, beta accumulate, ragged tail."""
    M = 20000 + 37
    dy, x = rnd(M, Mo, seed=21), rnd(M, No, seed=22)
    dW, db = rnd(Mo, No, seed=23), rnd(Mo, seed=24)
    ref, refb = dW.double() + dy.double().t() @ x.double(), db.double() + dy.double().sum(0)
    ops.linear_bwd_weight(dy, x, dW, beta=1.0, db=db)
    assert (dW.double() - ref).abs().max().item() < 2e-3
    assert (db.double() - refb).abs().max().item() < 2e-3
    dW2 = torch.empty_like(dW)
    ops.linear_bwd_weight(dy, x, dW2, beta=0.0)
    dW3 = torch.empty_like(dW)
    ops.linear_bwd_weight(dy, x, dW3, beta=0.0)
    assert torch.equal(dW2, dW3)  # deterministic reduction


def test_colsum_deterministic():
    X = rnd(20000, 70, seed=9)
    out = torch.full((70,), 2.0, device=DEV)
    ops.colsum(X, out, scale=0.5, beta=1.0)
    assert torch.allclose(out, 2.0 + 0.5 * X.sum(0), atol=1e-3)
    o1 = torch.zeros(70, device=DEV)
    o2 = torch.zeros(70, device=DEV)
    ops.colsum(X, o1)
    ops.colsum(X, o2)
    assert torch.equal(o1, o2)


def test_gather_small_tables_staged_in_lds(monkeypatch):
    """Tables of at most 16 KB are staged whole into LDS by the forward gather (gather.hip
    kStageBytes); the result is the same bits as reading them from HBM (RSYS_NO_LDS_STAGE=1),
    for sparse, pooled mean / sum / max and split bags; out-of-range ids still raise the flag."""
    B = 4096
    cases = [(30, 8, 6, 'mean'), (25, 8, 1, None), (3, 4, 1, None), (152, 8, 1, None), (30, 8, 6, 'max'),
             (500, 8, 40, 'sum'), (1000, 4, 12, 'mean')]
    for V, D, Lb, mode in cases:
        t = rnd(V, D, seed=V + D)
        ids = torch.randint(0, V, (B, Lb), device=DEV)
        ids[::7, 0] = 0
        kind = _hip.RS_SEG_SPARSE if mode is None else _hip.RS_SEG_POOL
        seg = dict(kind=kind, dim=D, out_col=4, vocab=V, idx_stride=Lb, idx=ids.data_ptr(), table=t.data_ptr())
        if mode is not None:
            seg.update(pool_mode=_hip.RS_POOL[mode], bag=Lb)
        outs = []
        for off in ('', '1'):
            monkeypatch.setenv('RSYS_NO_LDS_STAGE', off)
            out = torch.zeros(B, D + 8, device=DEV)
            err = torch.zeros(1, dtype=torch.int32, device=DEV)
            ops.gather_fwd([_seg(**seg)], B, out, err)
            assert err.item() == 0
            outs.append(out)
        assert torch.equal(outs[0], outs[1]), (V, D, Lb, mode)
        ref = t[ids]
        ref = ref[:, 0] if mode is None else {'mean': ref.mean(1), 'sum': ref.sum(1), 'max': ref.max(1)[0]}[mode]
        assert torch.allclose(outs[0][:, 4:4 + D], ref, atol=1e-5), (V, D, Lb, mode)
    monkeypatch.setenv('RSYS_NO_LDS_STAGE', '')
    bad = torch.randint(0, 30, (B, 6), device=DEV)
    bad[5, 2] = 31
    out = torch.empty(B, 8, device=DEV)
    err = torch.zeros(1, dtype=torch.int32, device=DEV)
    tb = rnd(30, 8)
    ops.gather_fwd([_seg(kind=_hip.RS_SEG_POOL, dim=8, out_col=0, pool_mode=0, bag=6, vocab=30, idx_stride=6,
                         idx=bad.data_ptr(), table=tb.data_ptr())], B, out, err)
    assert err.item() == 1


@pytest.mark.parametrize('zipf,B,V,D,Lb', [(None, 4096, 1_000_000, 128, 50), (1.05, 4096, 1_000_000, 128, 50),
                                            (1.05, 300, 200_000, 64, 30), (None, 64, 50_000, 32, 8)])
def test_gather_hot_rows_bitwise(monkeypatch, zipf, B, V, D, Lb):
    """Pooled (mean / sum) lookups with their sorted call (seg.hot_keys), RSYS_HOT_ROWS=1 (opt-in:
    measured slower in the step, gather.hip): the rows looked up >= 512 times -- the padding row,
    Zipf-hot rows -- are staged into LDS per workgroup and served from there; the result is
    bitwise the plain gather's and matches torch."""
    from recommendsystemproject_amd import synth
    g = np.random.default_rng(B + D)
    ids_np = synth._ids(g, V, (B, Lb), zipf)
    k = g.integers(0, Lb + 1, size=B)
    ids_np = np.where(np.arange(Lb)[None, :] < k[:, None], ids_np, 0)  # right-padded with row 0
    ids = torch.from_numpy(ids_np).to(DEV)
    t = rnd(V, D, seed=3)
    n = B * Lb
    keys = torch.empty(n, dtype=torch.int32, device=DEV)
    vals = torch.empty(n, dtype=torch.int32, device=DEV)
    ws = torch.empty(int(_hip.lib().rs_lookup_sort_ws_bytes(n, V)) // 4 + 1, dtype=torch.int32, device=DEV)
    _hip.call('rs_lookup_sort', ids.data_ptr(), 8, B, Lb, Lb, V, keys.data_ptr(), vals.data_ptr(), ws.data_ptr(),
              ops.stream())
    for mode in ('mean', 'sum'):
        outs = []
        for on in ('1', ''):
            monkeypatch.setenv('RSYS_HOT_ROWS', on)
            seg = _seg(kind=_hip.RS_SEG_POOL, dim=D, out_col=4, pool_mode=_hip.RS_POOL[mode], bag=Lb, vocab=V,
                       idx_stride=Lb, idx=ids.data_ptr(), table=t.data_ptr())
            seg.hot_keys, seg.hot_n = keys.data_ptr(), n
            out = torch.zeros(B, D + 8, device=DEV)
            err = torch.zeros(1, dtype=torch.int32, device=DEV)
            ops.gather_fwd([seg], B, out, err)
            assert err.item() == 0
            outs.append(out)
        assert torch.equal(outs[0], outs[1]), (zipf, mode, (outs[0] - outs[1]).abs().max().item())
        ref = t[ids].sum(1) / (Lb if mode == 'mean' else 1)
        assert torch.allclose(outs[0][:, 4:4 + D], ref, atol=1e-5)
    monkeypatch.setenv('RSYS_HOT_ROWS', '')


def test_gather_bit_exact_all_kinds():
    B = 257
    V1, D1 = 1000, 64
    V2, D2, Lb = 30, 8, 3
    t1, t2 = rnd(V1, D1, seed=1), rnd(V2, D2, seed=2)
    t3 = rnd(11, 6, seed=3)  # odd width -> scalar path
    ids = torch.randint(0, V1, (B, 2), device=DEV)
    bag = torch.randint(0, V2, (B, Lb), device=DEV)
    ids3 = torch.randint(0, 11, (B,), device=DEV)
    w, bb, x = rnd(4, seed=4), rnd(4, seed=5), rnd(B, 1, seed=6)
    src = rnd(B * 5, 8, seed=7)
    last = torch.randint(0, 5, (B,), device=DEV)
    outs = {}
    for mode, red in (('mean', lambda e: e.mean(1)), ('sum', lambda e: e.sum(1)), ('max', lambda e: e.max(1)[0])):
        segs = [
            _seg(kind=_hip.RS_SEG_SPARSE, dim=D1, out_col=0, vocab=V1, idx_stride=2, idx=ids.data_ptr() + 8,
                 table=t1.data_ptr()),
            _seg(kind=_hip.RS_SEG_POOL, dim=D2, out_col=64, pool_mode=_hip.RS_POOL[mode], bag=Lb, vocab=V2,
                 idx_stride=Lb, idx=bag.data_ptr(), table=t2.data_ptr()),
            _seg(kind=_hip.RS_SEG_SPARSE, dim=6, out_col=72, vocab=11, idx_stride=1, idx=ids3.data_ptr(),
                 table=t3.data_ptr()),
            _seg(kind=_hip.RS_SEG_DENSE, dim=4, out_col=78, idx_stride=1, x=x.data_ptr(), table=w.data_ptr(),
                 bias=bb.data_ptr()),
            _seg(kind=_hip.RS_SEG_LASTVALID, dim=8, out_col=82, bag=5, idx=last.data_ptr(), table=src.data_ptr()),
        ]
        out = torch.empty(B, 90, device=DEV)
        err = torch.zeros(1, dtype=torch.int32, device=DEV)
        ops.gather_fwd(segs, B, out, err)
        assert torch.equal(out[:, :64], t1[ids[:, 1]])
        assert torch.allclose(out[:, 64:72], red(t2[bag]), atol=1e-6)
        if mode == 'max':
            assert torch.equal(out[:, 64:72], red(t2[bag]))
        assert torch.equal(out[:, 72:78], t3[ids3])
        assert torch.allclose(out[:, 78:82], x * w + bb, atol=1e-6)
        assert torch.equal(out[:, 82:90], src.view(B, 5, 8)[torch.arange(B), last])
        assert err.item() == 0
        outs[mode] = out
    bad = ids.clone()
    bad[3, 1] = V1 + 5
    segs = [_seg(kind=_hip.RS_SEG_SPARSE, dim=D1, out_col=0, vocab=V1, idx_stride=2, idx=bad.data_ptr() + 8,
                 table=t1.data_ptr())]
    out = torch.empty(B, 64, device=DEV)
    err = torch.zeros(1, dtype=torch.int32, device=DEV)
    ops.gather_fwd(segs, B, out, err)
    assert err.item() == 1


@pytest.mark.parametrize('V', [50, 5000])  # LDS-privatised small table / global atomics
def test_gather_backward_matches_embedding_backward(V):
    B, D, Lb = 3000, 16, 4
    t = rnd(V, D, seed=1).requires_grad_(True)
    bag = torch.randint(0, V, (B, Lb), device=DEV)
    bag[:, 3] = 0  # padding slot
    ids = torch.randint(0, V, (B,), device=DEV)
    dout = rnd(B, 2 * D, seed=2)
    ref_out = torch.cat([F.embedding(ids, t, padding_idx=0), F.embedding(bag, t, padding_idx=0).mean(1)], 1)
    ref_out.backward(dout)
    g = torch.zeros(V, D, device=DEV)
    segs = [_seg(kind=_hip.RS_SEG_SPARSE, dim=D, out_col=0, vocab=V, idx_stride=1, idx=ids.data_ptr(),
                 table=t.data_ptr(), grad=g.data_ptr(), pad_idx=0),
            _seg(kind=_hip.RS_SEG_POOL, dim=D, out_col=D, pool_mode=0, bag=Lb, vocab=V, idx_stride=Lb,
                 idx=bag.data_ptr(), table=t.data_ptr(), grad=g.data_ptr(), pad_idx=0)]
    ops.gather_bwd(segs, B, dout)
    assert torch.allclose(g, t.grad, atol=1e-5)
    assert (g[0] == 0).all()


def _bwd_routes(segs, rows, ldo):
    return [_hip.GATHER_BWD_ROUTES[p.route] for p in ops.gather_plan(segs, rows, ldo, 1)[0]]


@pytest.mark.parametrize('V,D,rows,Lb,mode', [(3500, 32, 204800, 1, None), (5001, 64, 50000, 1, None),
                                               (3000, 16, 20000, 20, 'mean'), (2000, 8, 9000, 7, 'sum'),
                                               (70000, 4, 600000, 1, None), (30, 8, 204800, 3, 'mean'),
                                               (25, 8, 4096, 1, None), (700, 16, 4096, 1, None),
                                               (3, 4, 5000, 1, None), (40, 64, 3000, 5, 'sum')])
def test_gather_backward_ranged_hot_tables(monkeypatch, V, D, rows, Lb, mode):
    """Mid-size tables (48 KB - 4 MB, D in 16..256: C2's 3,500 x 32
    history table at 204,800 token lookups) take the ranged LDS path (gather.hip
    gather_bwd_range_kernel: row-owner waves, chunk partials reduced in order; bitwise
    reproducible) when hit >= 8 times per row; smaller ones the float-atomic small-table kernel.
    Deterministic mode (rs_set_deterministic, torch.use_deterministic_algorithms): the slot-image
    kernel (slot-private LDS images, no atomics) or the ranged kernel for every table of <= 4 MB,
    bitwise reproducible. RSYS_NO_RANGE_GRAD=1: the atomic scatter. All against the embedding
    backward, padding row skipped, out-of-range ids ignored, grad accumulated (+=)."""
    t = rnd(V, D, seed=31).requires_grad_(True)
    shape = (rows,) if mode is None else (rows, Lb)
    ids = torch.randint(0, V, shape, device=DEV)
    ids.view(-1)[::97] = 0  # padding row
    ids.view(-1)[:64] = min(17, V - 1)  # one hot row many times in one wave
    kind = _hip.RS_SEG_SPARSE if mode is None else _hip.RS_SEG_POOL
    ldo = D + 8
    dout = rnd(rows, ldo, seed=32)
    emb = F.embedding(ids, t, padding_idx=0)
    ref = emb if mode is None else (emb.mean(1) if mode == 'mean' else emb.sum(1))
    ref.backward(dout[:, 4:4 + D])
    seg = dict(kind=kind, dim=D, out_col=4, vocab=V, idx_stride=1 if mode is None else Lb, idx=ids.data_ptr(),
               table=t.data_ptr(), pad_idx=0)
    if mode is not None:
        seg.update(pool_mode=_hip.RS_POOL[mode], bag=Lb)
    arr = ops.segments_array([_seg(**seg)])
    n = rows * Lb
    L = _hip.lib()
    ranged = 48 * 1024 < V * D * 4 <= 4 << 20 and D >= 16 and n >= 8 * V
    onehot = V <= 64 and D <= 16 and n >= 65536  # gather_bwd_onehot_kernel, both modes
    assert (L.rs_gather_ws_bytes(arr, 1, rows) > 0) == (ranged or onehot)  # partials in ws
    det_ok = V * D * 4 <= 4 << 20 and (D >= 16 or V * D * 4 <= 48 * 1024)  # slot, ranged or one-hot
    # the route rs_gather_plan names: (default, deterministic mode)
    routes = {(3500, 32): ('range', 'range'), (5001, 64): ('range', 'range'), (3000, 16): ('range', 'range'),
              (2000, 8): ('scatter', 'scatter'), (70000, 4): ('scatter', 'scatter'), (30, 8): ('onehot', 'onehot'),
              (25, 8): ('small_lds', 'slot'), (700, 16): ('small_lds', 'range'), (3, 4): ('small_lds', 'slot'),
              (40, 64): ('small_lds', 'slot')}[V, D]
    grads = []
    # the planned path, deterministic mode twice, the atomic scatter
    for off, det in (('', 0), ('', 1), ('', 1), ('1', 0)):
        monkeypatch.setenv('RSYS_NO_RANGE_GRAD', off)
        torch.use_deterministic_algorithms(bool(det), warn_only=True)
        try:
            ops.sync_deterministic()
            if det:
                assert (L.rs_gather_ws_bytes(arr, 1, rows) > 0) == det_ok
            route = _bwd_routes([_seg(**seg)], rows, ldo)[0]
            assert route == ('scatter' if off and routes[det] == 'range' else routes[det])
            g = torch.full((V, D), 0.25, device=DEV)
            ops.gather_bwd([_seg(**seg, grad=g.data_ptr())], rows, dout)
            torch.cuda.synchronize()
        finally:
            torch.use_deterministic_algorithms(False)
            ops.sync_deterministic()
        grads.append(g)
    monkeypatch.setenv('RSYS_NO_RANGE_GRAD', '')
    scale = max(1.0, t.grad.abs().max().item())
    for gr in grads:
        assert (gr - 0.25 - t.grad).abs().max().item() <= 2e-5 * scale
        assert (gr[0] == 0.25).all()
    if det_ok:  # slot-image and ranged gradients are bitwise reproducible
        assert torch.equal(grads[1], grads[2])
    # out-of-range / negative ids contribute nothing and do not fault
    bad = ids.clone()
    bad.view(-1)[5] = V + 100
    bad.view(-1)[6] = -3
    g = torch.zeros(V, D, device=DEV)
    ops.gather_bwd([_seg(**dict(seg, idx=bad.data_ptr()), grad=g.data_ptr())], rows, dout)
    assert torch.isfinite(g).all()


@pytest.mark.parametrize('V,D,rows,Lb,mode', [(30, 8, 204800, 3, 'mean'), (30, 8, 22000, 3, 'sum'),
                                               (3, 4, 70000, 1, None), (25, 8, 65537, 1, None),
                                               (64, 8, 70001, 1, None), (64, 16, 8000, 9, 'mean'),
                                               (17, 3, 1333, 50, 'sum'), (1, 1, 65536, 1, None),
                                               (50, 10, 70000, 5, 'mean')])
def test_gather_backward_onehot_tiny_tables(monkeypatch, V, D, rows, Lb, mode):
    """Tiny, heavily hit tables (V <= 64, D <= 16, >= 65,536 lookups a call: C2's per-token genre
    bags of the history) take the one-hot MFMA kernel in both modes
    (gather.hip gather_bwd_onehot_kernel): against the embedding backward (padding row skipped,
    out-of-range ids ignored, grad accumulated), bitwise reproducible, and within fp32 summation
    order of the atomic kernel (RSYS_NO_ONEHOT_GRAD=1). Odd row counts, bags longer than one pass
    of four ids, D not a multiple of 4."""
    t = rnd(V, D, seed=41).requires_grad_(True)
    shape = (rows,) if mode is None else (rows, Lb)
    ids = torch.randint(0, V, shape, device=DEV)
    ids.view(-1)[::13] = 0  # padding row
    ids.view(-1)[:100] = V - 1  # one row many times in one batch
    kind = _hip.RS_SEG_SPARSE if mode is None else _hip.RS_SEG_POOL
    ldo = D + 5
    dout = rnd(rows, ldo, seed=42)
    emb = F.embedding(ids, t, padding_idx=0)
    ref = emb if mode is None else (emb.mean(1) if mode == 'mean' else emb.sum(1))
    ref.backward(dout[:, 3:3 + D])
    seg = dict(kind=kind, dim=D, out_col=3, vocab=V, idx_stride=1 if mode is None else Lb, idx=ids.data_ptr(),
               table=t.data_ptr(), pad_idx=0)
    if mode is not None:
        seg.update(pool_mode=_hip.RS_POOL[mode], bag=Lb)
    assert _hip.lib().rs_gather_ws_bytes(ops.segments_array([_seg(**seg)]), 1, rows) > 0
    grads = []
    for off in ('', '', '1'):
        monkeypatch.setenv('RSYS_NO_ONEHOT_GRAD', off)
        assert _bwd_routes([_seg(**seg)], rows, ldo)[0] == ('small_lds' if off else 'onehot')
        g = torch.full((V, D), 0.5, device=DEV)
        ops.gather_bwd([_seg(**seg, grad=g.data_ptr())], rows, dout)
        torch.cuda.synchronize()
        grads.append(g)
    monkeypatch.delenv('RSYS_NO_ONEHOT_GRAD')
    assert torch.equal(grads[0], grads[1])
    scale = max(1.0, t.grad.abs().max().item())
    for gr in grads:
        assert (gr - 0.5 - t.grad).abs().max().item() <= 2e-5 * scale * max(1, Lb // 8)
        assert (gr[0] == 0.5).all() or V == 1
    bad = ids.clone()
    bad.view(-1)[5] = V + 100
    bad.view(-1)[6] = -3
    g = torch.zeros(V, D, device=DEV)
    ops.gather_bwd([_seg(**dict(seg, idx=bad.data_ptr()), grad=g.data_ptr())], rows, dout)
    assert torch.isfinite(g).all()


def test_gather_backward_all_routes_one_launch():
    """One rs_gather_bwd call whose segments take every backward route between default and
    deterministic mode (rs_gather_plan names them): the smallest launch in which the per-route
    workgroup offsets and workspace offsets of different routes sit side by side. Table gradients
    against the embedding backward, the dense segment against a float64 column reduction (bound:
    fp32 summation of rows / 32 + 32 terms deep, the kernel's row-lane chains and its tree);
    deterministic mode bitwise reproducible on every route but the atomic scatter."""
    rows, ldo, dcol = 22016, 60, 52
    tables = [(70000, 4, 1), (700, 16, 1), (800, 16, 1), (30, 8, 3), (25, 8, 1)]  # V, D, bag (sum-pooled when > 1)
    want = {False: ['scatter', 'small_lds', 'range', 'onehot', 'small_lds', 'dense'],
            True: ['scatter', 'range', 'range', 'onehot', 'slot', 'dense']}
    dout = rnd(rows, ldo, seed=52)
    x, w, b = rnd(rows, 1, seed=53), rnd(8, seed=54), rnd(8, seed=55)
    ts, idss, base, outs, col = [], [], [], [], 0
    for k, (V, D, bag) in enumerate(tables):
        t = rnd(V, D, seed=60 + k).requires_grad_(True)
        ids = torch.randint(0, V, (rows, bag), device=DEV)
        ids.view(-1)[::97] = 0  # padding row
        emb = F.embedding(ids, t, padding_idx=0)
        outs.append(emb.sum(1))
        base.append(dict(kind=_hip.RS_SEG_SPARSE if bag == 1 else _hip.RS_SEG_POOL, dim=D, out_col=col, vocab=V,
                         idx_stride=bag, idx=ids.data_ptr(), table=t.data_ptr(), pad_idx=0,
                         pool_mode=_hip.RS_POOL['sum'], bag=bag))
        ts.append(t)
        idss.append(ids)
        col += D
    assert col == dcol
    torch.cat(outs, 1).backward(dout[:, :dcol])
    gd = dout[:, dcol:dcol + 8].double()
    ref_w, ref_b = (gd * x.double()).sum(0), gd.sum(0)
    depth = rows // 32 + 32
    tol_w = (depth + 1) * 2.0 ** -24 * (gd * x.double()).abs().sum(0)
    tol_b = depth * 2.0 ** -24 * gd.abs().sum(0)

    def run(det):
        torch.use_deterministic_algorithms(det, warn_only=True)
        try:
            ops.sync_deterministic()
            grads = [torch.full_like(t, 0.25) for t in ts]
            gw, gb = torch.zeros(8, device=DEV), torch.zeros(8, device=DEV)
            segs = [_seg(**s, grad=g.data_ptr()) for s, g in zip(base, grads)]
            segs.append(_seg(kind=_hip.RS_SEG_DENSE, dim=8, out_col=dcol, idx_stride=1, x=x.data_ptr(),
                             table=w.data_ptr(), bias=b.data_ptr(), grad=gw.data_ptr(), grad_bias=gb.data_ptr()))
            assert _bwd_routes(segs, rows, ldo) == want[det]
            ops.gather_bwd(segs, rows, dout)
            torch.cuda.synchronize()
        finally:
            torch.use_deterministic_algorithms(False)
            ops.sync_deterministic()
        for t, g in zip(ts, grads):
            err = (g - 0.25 - t.grad).abs().max().item()
            assert err <= 2e-5 * max(1.0, t.grad.abs().max().item()), (det, tuple(t.shape), err)
            assert (g[0] == 0.25).all()
        assert ((gw.double() - ref_w).abs() <= tol_w).all() and ((gb.double() - ref_b).abs() <= tol_b).all()
        return grads + [gw, gb]

    run(False)
    first, second = run(True), run(True)
    for k, (g1, g2) in enumerate(zip(first, second)):
        assert k == 0 or torch.equal(g1, g2), k  # segment 0 is the float-atomic scatter


@pytest.mark.parametrize('B,D,Lb,mode', [(300, 128, 50, 'mean'), (300, 128, 50, 'sum'), (257, 64, 17, 'mean'),
                                          (4096, 128, 50, 'mean'), (5, 128, 33, 'mean')])
def test_pooled_split_bags(B, D, Lb, mode):
    """Long sum/mean bags at small batch are split over several row groups (gather.hip
    gather_pool_split); forward against torch, backward (with touch counts: a row looked up
    once is a plain store) against the embedding backward, bad ids flagged."""
    V = 20000
    t = rnd(V, D, seed=11).requires_grad_(True)
    bag = torch.randint(0, V, (B, Lb), device=DEV)
    bag[:, -1] = 0  # padding slot
    bag[1, :] = 7  # one row many times in one bag
    red = (lambda e: e.mean(1)) if mode == 'mean' else (lambda e: e.sum(1))
    ref = red(F.embedding(bag, t, padding_idx=0))
    segs = [_seg(kind=_hip.RS_SEG_POOL, dim=D, out_col=0, pool_mode=_hip.RS_POOL[mode], bag=Lb, vocab=V,
                 idx_stride=Lb, idx=bag.data_ptr(), table=t.data_ptr(), pad_idx=0)]
    out = torch.empty(B, D, device=DEV)
    err = torch.zeros(1, dtype=torch.int32, device=DEV)
    ops.gather_fwd(segs, B, out, err)
    assert err.item() == 0
    # fp32 summation-order tolerance: the split bag adds S partial sums of Lb/S rows
    assert torch.allclose(out, ref, atol=2e-6 * (Lb if mode == 'sum' else 1), rtol=1e-5)
    dout = rnd(B, D, seed=12)
    ref.backward(dout)
    counts = torch.bincount(bag.flatten(), minlength=V).to(torch.int32)
    g = torch.zeros(V, D, device=DEV)
    segs[0].grad = g.data_ptr()
    segs[0].touch_count = counts.data_ptr()
    ops.gather_bwd(segs, B, dout)
    assert torch.allclose(g, t.grad, atol=1e-5, rtol=1e-5)
    bad = bag.clone()
    bad[B - 1, Lb // 2] = V + 3
    segs[0].idx = bad.data_ptr()
    ops.gather_fwd(segs, B, out, err)
    assert err.item() == 1


def test_seq_mask_quirks():
    seq = torch.tensor([[5, 3, 0, 0], [0, 0, 0, 0], [1, 2, 3, 4], [0, 7, 0, 0]], device=DEV)
    key_pad, last = ops.seq_mask(seq, 0)
    assert key_pad.tolist() == [[0, 0, 1, 1], [1, 1, 1, 0], [0, 0, 0, 0], [1, 0, 1, 1]]  # T6
    assert last.tolist() == [1, 0, 3, 0]  # T7: count-based, all-pad row -> 0


@pytest.mark.parametrize('B,L', [(1000, 50), (37, 1), (300, 64), (300, 65), (257, 200), (64, 129)])
def test_seq_mask_random(B, L):
    """One wave per row (ballot count): bit-exact against the reference's mask / last-valid rules
    (SequenceEncoder.py:32-74, T6/T7) on random padding patterns incl. all-padding rows, and on a
    strided id matrix (a column slice of a wider [B, ld] tensor)."""
    g = torch.Generator().manual_seed(B * 1000 + L)
    wide = torch.randint(0, 4, (B, L + 3), generator=g)  # 0 = padding, ~25 %
    wide[::7] = 0  # all-padding rows
    seq = wide.to(DEV)[:, 2:2 + L]
    key_pad, last = ops.seq_mask(seq, 0)
    s = wide[:, 2:2 + L]
    ref_pad = (s == 0)
    allpad = ref_pad.all(1)
    ref_pad[allpad, L - 1] = False
    valid = (~(s == 0)).sum(1)
    ref_last = torch.clamp(valid - 1, min=0)
    assert torch.equal(key_pad.cpu().bool(), ref_pad)
    assert torch.equal(last.cpu(), ref_last)


def ref_attention(qkv, key_pad, B, L, d, H):
    hd = d // H
    q, k, v = qkv.view(B, L, 3, H, hd).permute(2, 0, 3, 1, 4)
    s = q @ k.transpose(-1, -2) / math.sqrt(hd)
    s = s.masked_fill(key_pad.bool()[:, None, None, :], float('-inf'))
    return (torch.softmax(s, -1) @ v).transpose(1, 2).reshape(B * L, d)


# head_dim 16 with L <= 64 takes the MFMA kernels (NT = ceil(L/16) tiles); the rest the VALU ones
@pytest.mark.parametrize('B,L,d,H', [(3, 50, 64, 4), (2, 7, 64, 2), (5, 200, 64, 4), (4, 20, 32, 4),
                                     (6, 33, 64, 4), (5, 16, 64, 4), (3, 64, 64, 4), (5, 16, 48, 3),
                                     (3, 50, 32, 2), (2, 1, 64, 4)])
def test_attention_fwd_bwd(B, L, d, H):
    qkv = rnd(B * L, 3 * d, seed=1).requires_grad_(True)
    lens = torch.randint(0, L + 1, (B,))
    seq = (torch.arange(L)[None, :] < lens[:, None]).long().to(DEV)
    key_pad, _ = ops.seq_mask(seq, 0)
    ref = ref_attention(qkv, key_pad, B, L, d, H)
    out, lse = ops.attn_fwd(qkv.detach(), key_pad, B, L, d, H)
    assert torch.allclose(out, ref, atol=2e-5, rtol=1e-4)
    dout = rnd(B * L, d, seed=2)
    ref.backward(dout)
    dqkv = ops.attn_bwd(qkv.detach(), key_pad, out, dout, lse, B, L, d, H)
    assert torch.allclose(dqkv, qkv.grad, atol=5e-5, rtol=1e-4)


def test_attention_dropout_consistent():
    """Dropout on attention probabilities: fwd/bwd use the same mask (finite-difference check
    of <dout, out> along a random direction) and the keep rate is ~1-p."""
    B, L, d, H, p = 4, 30, 64, 4, 0.25
    qkv = rnd(B * L, 3 * d, seed=3).double().float()
    key_pad = torch.zeros(B, L, dtype=torch.uint8, device=DEV)
    key = torch.tensor([1234, 7], dtype=torch.int64, device=DEV)
    out, lse = ops.attn_fwd(qkv, key_pad, B, L, d, H, p, key, 3)
    out0, _ = ops.attn_fwd(qkv, key_pad, B, L, d, H, 0.0)
    assert not torch.allclose(out, out0)
    dout = rnd(B * L, d, seed=4)
    dq = ops.attn_bwd(qkv, key_pad, out, dout, lse, B, L, d, H, p, key, 3)
    direc = rnd(B * L, 3 * d, seed=5)
    eps = 1e-3
    fp, _ = ops.attn_fwd(qkv + eps * direc, key_pad, B, L, d, H, p, key, 3)
    fm, _ = ops.attn_fwd(qkv - eps * direc, key_pad, B, L, d, H, p, key, 3)
    fd = ((fp - fm) * dout).sum().item() / (2 * eps)
    an = (dq * direc).sum().item()
    assert abs(fd - an) < 2e-2 * max(1.0, abs(an)), (fd, an)


@pytest.mark.parametrize('L', [30, 50])
def test_attention_mfma_matches_valu_kernel(L, monkeypatch):
    """The MFMA and VALU attention kernels draw the same dropout masks and agree numerically."""
    B, d, H, p = 5, 64, 4, 0.2
    qkv = rnd(B * L, 3 * d, seed=8)
    lens = torch.tensor([L, 1, L // 2, 3, L - 1])
    seq = (torch.arange(L)[None, :] < lens[:, None]).long().to(DEV)
    key_pad, _ = ops.seq_mask(seq, 0)
    key = torch.tensor([99, 5], dtype=torch.int64, device=DEV)
    dout = rnd(B * L, d, seed=9)
    res = []
    for valu in ('0', '1'):
        monkeypatch.setenv('RSYS_ATTN_VALU', valu)
        out, lse = ops.attn_fwd(qkv, key_pad, B, L, d, H, p, key, 4)
        dq = ops.attn_bwd(qkv, key_pad, out, dout, lse, B, L, d, H, p, key, 4)
        res.append((out, lse, dq))
    for a, b in zip(*res):
        assert torch.allclose(a, b, atol=2e-5, rtol=1e-4)


@pytest.mark.parametrize('M,N', [(1000, 64), (40003, 64), (777, 48)])  # N = 64: the 16-row kernel
def test_layernorm_fwd_bwd(M, N):
    a, b = rnd(M, N, seed=1), rnd(M, N, seed=2)
    g, be = rnd(N, seed=3), rnd(N, seed=4)
    h_ref = (a + b).requires_grad_(True)
    gr, br = g.clone().requires_grad_(True), be.clone().requires_grad_(True)
    y_ref = F.layer_norm(h_ref, (N,), gr, br, 1e-5)
    a2 = a.clone()
    y, mean, rstd = ops.add_layernorm_fwd(a2, b, g, be)
    assert torch.allclose(y, y_ref, atol=1e-5)
    assert torch.allclose(a2, a + b)
    dy = rnd(M, N, seed=5)
    y_ref.backward(dy)
    dg, db = torch.zeros(N, device=DEV), torch.zeros(N, device=DEV)
    dh = ops.layernorm_bwd(a2, dy.clone(), g, mean, rstd, dg, db)
    assert torch.allclose(dh, h_ref.grad, atol=1e-4)
    assert torch.allclose(dg, gr.grad, atol=1e-3 * max(1.0, M / 1000)) and \
        torch.allclose(db, br.grad, atol=1e-3 * max(1.0, M / 1000))
    # the sublayer's dropout in the same pass: da == dropout_bwd(dh) (same draw)
    key = torch.tensor([3, 4], dtype=torch.int64, device=DEV)
    da = torch.empty_like(dh)
    dh2 = ops.layernorm_bwd(a2, dy.clone(), g, mean, rstd, torch.zeros_like(dg), torch.zeros_like(db), da=da,
                            p=0.2, key=key, site=7)
    assert torch.equal(dh2, dh)
    ref_da = dh.clone()
    ops.dropout_bwd(ref_da, 0.2, key, 7)
    assert torch.equal(da, ref_da)


@pytest.mark.parametrize('Bg', [300, 6000])  # single-kernel path / partials path (G*Bg > 16384)
@pytest.mark.parametrize('G', [1, 3])
@pytest.mark.parametrize('relu', [False, True])
def test_batchnorm_train_fwd_bwd(G, relu, Bg):
    C = 172
    bn = torch.nn.BatchNorm1d(C).to(DEV)
    with torch.no_grad():
        bn.weight.copy_(1 + 0.1 * rnd(C, seed=1))
        bn.bias.copy_(0.1 * rnd(C, seed=2))
    ref_bn = torch.nn.BatchNorm1d(C).to(DEV)
    ref_bn.load_state_dict(bn.state_dict())
    x = (rnd(G * Bg, C, seed=3) * 3 + 1)
    y, mean, rstd = ops.batchnorm_fwd(x, bn, G, relu, training=True)
    xr = x.clone().requires_grad_(True)
    outs = [ref_bn(xr[g * Bg:(g + 1) * Bg]) for g in range(G)]
    yr = torch.cat(outs)
    if relu:
        yr = torch.relu(yr)
    assert torch.allclose(y, yr, atol=1e-5)
    assert torch.allclose(bn.running_mean, ref_bn.running_mean, atol=1e-6)
    assert torch.allclose(bn.running_var, ref_bn.running_var, atol=1e-5)
    assert bn.num_batches_tracked.item() == ref_bn.num_batches_tracked.item() == G
    dy = rnd(G * Bg, C, seed=4)
    yr.backward(dy)
    dw, db = torch.zeros(C, device=DEV), torch.zeros(C, device=DEV)
    dx = ops.batchnorm_bwd(x, y, dy, bn.weight, mean, rstd, dw, db, G, relu)
    assert torch.allclose(dx, xr.grad, atol=2e-5)
    assert torch.allclose(dw, ref_bn.weight.grad, atol=1e-3) and torch.allclose(db, ref_bn.bias.grad, atol=1e-3)
    bn.eval()
    ref_bn.eval()
    ye, _, _ = ops.batchnorm_fwd(x, bn, 1, False, training=False)
    assert torch.allclose(ye, ref_bn(x), atol=1e-5)


@pytest.mark.parametrize('G', [1, 2])
def test_batchnorm_fused_dropout_equals_separate(G):
    """BN -> ReLU -> Dropout in one kernel (MLP block) == BN+ReLU then the standalone dropout
    kernel (same draw, bitwise), and its backward == dropout_bwd then the BN backward."""
    C, Bg, p = 256, 4096, 0.3
    bn = torch.nn.BatchNorm1d(C).to(DEV)
    bn2 = torch.nn.BatchNorm1d(C).to(DEV)
    x = rnd(G * Bg, C, seed=7) * 2 + 0.5
    key = torch.tensor([42, 9], dtype=torch.int64, device=DEV)
    y, mean, rstd = ops.batchnorm_fwd(x, bn, G, True, training=True, drop_p=p, drop_key=key, drop_site=257)
    y2, mean2, rstd2 = ops.batchnorm_fwd(x, bn2, G, True, training=True)
    ops.dropout_fwd(y2, p, key, 257)
    assert torch.equal(y, y2) and torch.equal(mean, mean2)
    assert 0.6 < (y2 != 0).float().mean().item() / max((torch.relu(x - x.mean(0)) > 0).float().mean().item(), 1e-6) < 0.8
    dy = rnd(G * Bg, C, seed=8)
    dw, db = torch.zeros(C, device=DEV), torch.zeros(C, device=DEV)
    dx = ops.batchnorm_bwd(x, y, dy, bn.weight, mean, rstd, dw, db, G, True, drop_p=p)
    dy2 = dy.clone()
    ops.dropout_bwd(dy2, p, key, 257)
    dw2, db2 = torch.zeros(C, device=DEV), torch.zeros(C, device=DEV)
    dx2 = ops.batchnorm_bwd(x, y2, dy2, bn2.weight, mean2, rstd2, dw2, db2, G, True)
    assert torch.allclose(dx, dx2, atol=1e-6) and torch.allclose(dw, dw2, atol=1e-5) and torch.allclose(db, db2, atol=1e-5)


def test_l2norm():
    x = rnd(500, 128, seed=1).requires_grad_(True)
    x.data[3] = 0.0
    yr = F.normalize(x, p=2, dim=1)
    y, norm = ops.l2norm_fwd(x.detach())
    assert torch.allclose(y, yr, atol=1e-6)
    dy = rnd(500, 128, seed=2)
    yr.backward(dy)
    dx = ops.l2norm_bwd(y, norm, dy)
    assert torch.allclose(dx, x.grad, atol=1e-4)


@pytest.mark.parametrize('K', [40, 36, 64, 72])
@pytest.mark.parametrize('p', [0.0, 0.1])
def test_projection_specialised_k_remainder(K, p, monkeypatch):
    """The sequence projection (M >= 32768, N = 64, K = 40: bias + dropout + positional add +
    dropout) on the compile-time-epilogue rowgemm, whose last k tile re-reads the row's last
    float4 when K % 16 != 0: bit-equal to the generic kernel, and torch at p = 0."""
    M, N, L = 50 * 700, 64, 50
    x, W, b = rnd(M, K, seed=1), rnd(N, K, seed=2) * 0.2, rnd(N, seed=3)
    pos = rnd(L, N, seed=4)
    key = torch.tensor([23, 2], dtype=torch.int64, device=DEV)
    outs = []
    for generic in ('0', '1'):
        monkeypatch.setenv('RSYS_ROWGEMM_GENERIC', generic)
        outs.append(ops.linear_fwd(x, W, b, aux=pos, aux_mod=L, drop_p=p, drop_key=key, site_a=0, site_b=1))
    assert torch.equal(outs[0], outs[1])
    if p == 0.0:
        ref = x @ W.t() + b + pos[torch.arange(M, device=DEV) % L]
        assert torch.allclose(outs[0], ref, atol=1e-4, rtol=1e-5)


@pytest.mark.parametrize('K', [64, 256, 40])
@pytest.mark.parametrize('p', [0.0, 0.1])
def test_linear_add_layernorm_fused(K, p, monkeypatch):
    """rs_gemm_add_layernorm: the fused streaming kernel (M >= 32768, N = 64, K in {64, 256})
    equals the GEMM + rs_add_layernorm_fwd pair it replaces, and torch at p = 0."""
    M, N = 40000, 64
    x, W, b = rnd(M, K, seed=1), rnd(N, K, seed=2) * 0.2, rnd(N, seed=3)
    res, g, be = rnd(M, N, seed=4), 1 + 0.1 * rnd(N, seed=5), 0.1 * rnd(N, seed=6)
    key = torch.tensor([17, 4], dtype=torch.int64, device=DEV)
    outs = []
    for unfused in ('0', '1'):
        monkeypatch.setenv('RSYS_UNFUSED_LN', unfused)
        outs.append(ops.linear_add_layernorm(x, W, b, res, g, be, 1e-5, p, key, 9))
    (h, y, mu, rs), (h2, y2, mu2, rs2) = outs
    # same products and masks; fma contraction of drop(.) + resid may differ by an ulp
    assert torch.allclose(h, h2, rtol=1e-6, atol=1e-6)
    assert torch.allclose(y, y2, atol=1e-5) and torch.allclose(mu, mu2, atol=1e-6)
    assert torch.allclose(rs, rs2, rtol=1e-5)
    if p == 0.0:
        href = x @ W.t() + b + res
        assert torch.allclose(h, href, atol=1e-4)
        assert torch.allclose(y, F.layer_norm(href, (N,), g, be, 1e-5), atol=1e-4)


@pytest.mark.parametrize('M', [300, 5000])
def test_gemm_dropout_epilogue_matches_dropout_kernel(M):
    """GEMM epilogue dropout == rs_dropout_fwd with the same (key, site) (masks are shared by
    the fused forward and the unfused backward)."""
    K, N, L, p = 40, 64, 25, 0.2
    x, W, b, pos = rnd(M, K, seed=1), rnd(N, K, seed=2), rnd(N, seed=3), rnd(L, N, seed=4)
    key = torch.tensor([77, 3], dtype=torch.int64, device=DEV)
    fused = ops.linear_fwd(x, W, b, aux=pos, aux_mod=L, drop_p=p, drop_key=key, site_a=0, site_b=1)
    ref = ops.linear_fwd(x, W, b)
    ops.dropout_fwd(ref, p, key, 0)
    ops.dropout_fwd(ref, p, key, 1, aux=pos, aux_mod=L)
    assert torch.allclose(fused, ref, atol=1e-5)
    f1 = ops.linear_fwd(x, W, b, relu=True, drop_p=p, drop_key=key, site_a=9)
    r1 = ops.linear_fwd(x, W, b, relu=True)
    ops.dropout_fwd(r1, p, key, 9)
    assert torch.allclose(f1, r1, atol=1e-5)


def test_dropout_statistics_and_mask_reuse():
    n, p = 1 << 20, 0.3
    x = torch.ones(n // 64, 64, device=DEV)
    key = torch.tensor([99, 5], dtype=torch.int64, device=DEV)
    ops.dropout_fwd(x, p, key, 2)
    kept = (x != 0).float().mean().item()
    assert abs(kept - (1 - p)) < 3e-3
    assert torch.allclose(x[x != 0], torch.full_like(x[x != 0], 1 / (1 - p)))
    g = torch.ones_like(x)
    ops.dropout_bwd(g, p, key, 2)
    assert torch.equal(g, x)
    state = torch.tensor([5, 0], dtype=torch.int64, device=DEV)
    k1, k2 = ops.rng_next(state), ops.rng_next(state)
    assert k1.tolist() == [5, 0] and k2.tolist() == [5, 1] and state.tolist() == [5, 2]


def test_adam_matches_torch():
    n = 10007
    p0 = rnd(n, seed=1)
    ours = p0.clone()
    m, v = torch.zeros_like(p0), torch.zeros_like(p0)
    tp = p0.clone().cpu().requires_grad_(True)
    opt = torch.optim.Adam([tp], lr=1e-3, weight_decay=0.01)
    for step in range(1, 4):
        g = rnd(n, seed=10 + step)
        tp.grad = g.cpu().clone()
        opt.step()
        _hip.call('rs_adam_step', ours.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), n, 1e-3, 0.9,
                  0.999, 1e-8, 0.01, step, None, 1.0, None, 0, ops.stream())
    assert torch.allclose(ours.cpu(), tp.detach(), atol=1e-6)


def test_clip_coefficient():
    g = rnd(100000, seed=1) * 0.01
    ws = torch.empty(int(_hip.lib().rs_sqnorm_ws_bytes(g.numel())), dtype=torch.uint8, device=DEV)
    norm = torch.zeros((), device=DEV)
    coef = torch.zeros((), device=DEV)
    _hip.call('rs_grad_sqnorm', g.data_ptr(), g.numel(), 0.5, ws.data_ptr(), ops.stream())
    nparts = int(_hip.lib().rs_sqnorm_parts(g.numel()))
    _hip.call('rs_clip_coef', ws.data_ptr(), nparts, 1.0, norm.data_ptr(), coef.data_ptr(), ops.stream())
    tn = (0.5 * g).norm().item()
    assert abs(norm.item() - tn) < 1e-5 * tn
    assert abs(coef.item() - min(1.0, 1.0 / (tn + 1e-6))) < 1e-6


@pytest.mark.parametrize('n', [1, 4097, 100003, 1900000, 5000000])
def test_sqnorm_clip_one_launch_bitwise(n):
    """rs_grad_sqnorm_clip_step (the partials' last workgroup makes the coefficient, advances the
    step counter, re-arms its ticket) against rs_grad_sqnorm + rs_clip_coef_step: the same bits,
    twice in a row (the ticket is left at zero)."""
    L = _hip.lib()
    g = rnd(n, seed=7) * 0.01
    nparts = int(L.rs_sqnorm_parts(n))
    ws = torch.empty(nparts + 2, dtype=torch.float64, device=DEV)
    out = []
    for fused in (0, 1, 1):
        norm = torch.zeros((), device=DEV)
        coef = torch.zeros((), device=DEV)
        cnt = torch.full((), 5, dtype=torch.int64, device=DEV)
        if fused:
            ticket = out[-1][3] if len(out) > 1 else torch.zeros((), dtype=torch.int32, device=DEV)
            _hip.call('rs_grad_sqnorm_clip_step', g.data_ptr(), n, 0.5, ws.data_ptr(), ticket.data_ptr(), 0.3,
                      norm.data_ptr(), coef.data_ptr(), cnt.data_ptr(), ops.stream())
        else:
            ticket = None
            _hip.call('rs_grad_sqnorm', g.data_ptr(), n, 0.5, ws.data_ptr(), ops.stream())
            _hip.call('rs_clip_coef_step', ws.data_ptr(), nparts, 0.3, norm.data_ptr(), coef.data_ptr(),
                      cnt.data_ptr(), ops.stream())
        torch.cuda.synchronize()
        out.append((norm.clone(), coef.clone(), cnt.item(), ticket))
    for o in out[1:]:
        assert torch.equal(o[0], out[0][0]) and torch.equal(o[1], out[0][1]) and o[2] == 6
        assert o[3].item() == 0
    tn = (0.5 * g).double().norm().item()
    assert abs(out[0][0].item() - tn) < 1e-5 * tn


@pytest.mark.parametrize('B,L,d,p', [(4096, 50, 64, 0.15), (37, 7, 64, 0.3), (300, 20, 16, 0.5)])
def test_seq_input_dropout_bwd_fused(B, L, d, p):
    """rs_seq_input_dropout_bwd (one pass: drop_b backward, positional-embedding colsum, drop_a
    backward) against rs_dropout_bwd + rs_colsum + rs_dropout_bwd: dx bit-exact (same draws,
    same products), the colsum to fp32 summation order; accumulates into pos_grad."""
    key = torch.tensor([77, 12], dtype=torch.int64, device=DEV)
    dx = rnd(B * L, d, seed=3)
    pos0 = rnd(L + 5, d, seed=4)
    ref, pr = dx.clone(), pos0.clone()
    ops.dropout_bwd(ref, p, key, 1)
    ops.colsum(ref, pr, M=B, N=L * d, ldx=L * d)
    ops.dropout_bwd(ref, p, key, 0)
    got, pg = dx.clone(), pos0.clone()
    ops.seq_input_dropout_bwd(got, pg, B, L * d, p, key, 0, 1)
    assert torch.equal(got, ref)
    assert torch.equal(pg[L:], pos0[L:])
    assert torch.allclose(pg, pr, atol=1e-4 * max(1.0, B / 1000), rtol=1e-5)
    g2, p2 = dx.clone(), pos0.clone()
    ops.seq_input_dropout_bwd(g2, p2, B, L * d, p, key, 0, 1)
    assert torch.equal(p2, pg)
