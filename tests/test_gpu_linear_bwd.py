"""The one-pass backwards of the bf16 compute mode (csrc/linear_bwd.hip). rs_seq_input_bwd_bf16
(behind functions.seq_input_grads; RSYS_SEQ_BWD_FUSED=0 reverts to the three-pass form): both
dropout backwards, the projection's weight / bias gradients and its input gradient from one read
of dx, the positional-embedding gradient from rs_seq_input_pos_grad's read-only pass.
rs_linear_bwd_bf16 (RSYS_LINBWD_FUSED=0 reverts): the in-projection's weight / bias gradients and
dx from one read of the bf16 dqkv. Where the kernels they replace are the bf16 streaming ones
(>= 32,768 rows, a multiple of 16), the new ones give their bits.

References are built here from torch: the two masks come from rs_dropout_bwd on ones (pinned by
test_gpu_kernels), the products from float64 matmuls of the bf16-rounded operands.
"""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F
import yaml

from recommendsystemproject_amd import functions, ops, precision

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def rnd(*shape, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g).to(DEV)


def r16(t):
    return t.to(torch.bfloat16).float()


@pytest.fixture
def bf16_mode():
    precision.set_compute_dtype('bf16')
    yield
    precision.set_compute_dtype('fp32')


# (B, L, d, dcat, p)
CASES = [
    (33, 50, 64, 40, 0.15),   # ragged last chunk, several workgroups, C2 widths
    (5, 200, 64, 72, 0.15),   # L * d = 12,800: C5's regime and widths
    (37, 7, 64, 40, 0.3),     # L shorter than a row chunk
    (64, 20, 64, 24, 0.0),    # no masks, narrow padded dcat
    (700, 50, 64, 40, 0.15),  # 35,000 rows (>= the 32,768 streaming threshold), many chunks per workgroup
]


def _inputs(B, L, d, dcat, p, masks=None):
    """masks: (mask_a, mask_b) [M, d] of key [4321, 7], sites 0 and 1, from somewhere else than the
    library (tests/dropout_ref.py); default: rs_dropout_bwd on ones."""
    M = B * L
    t = dict(dx=rnd(M, d, seed=1), cat=rnd(M, dcat, seed=2), W=rnd(d, dcat, seed=3) * 0.2,
             dW0=rnd(d, dcat, seed=4), db0=rnd(d, seed=5), pos0=rnd(L + 3, d, seed=6),
             key=torch.tensor([4321, 7], dtype=torch.int64, device=DEV))
    if masks is not None:
        t['mask_a'], t['mask_b'] = masks
    elif p > 0:
        ones = torch.ones(M, d, device=DEV)
        t['mask_a'] = ops.dropout_bwd(ones.clone(), p, t['key'], 0)
        t['mask_b'] = ops.dropout_bwd(ones.clone(), p, t['key'], 1)
    else:
        t['mask_a'] = t['mask_b'] = torch.ones(M, d, device=DEV)
    t['v'] = t['dx'] * t['mask_b']
    t['y'] = t['v'] * t['mask_a']
    return t


def _run(t, B, L, p):
    """-> (dcat, dW, db, pos_g) of one call on fresh copies of the accumulators."""
    dW, db, pos = t['dW0'].clone(), t['db0'].clone(), t['pos0'].clone()
    dcat = functions.seq_input_grads(t['dx'], t['cat'], t['W'], B, L, p, t['key'] if p > 0 else None, dW, db,
                                     pos, consume=False)
    torch.cuda.synchronize()
    return dcat, dW, db, pos


@pytest.mark.parametrize('B,L,d,dcat,p', CASES)
def test_seq_input_bwd_fused(B, L, d, dcat, p, bf16_mode, monkeypatch):
    monkeypatch.setenv('RSYS_SEQ_BWD_FUSED', '1')
    M = B * L
    t = _inputs(B, L, d, dcat, p)
    dx_before = t['dx'].clone()
    got = _run(t, B, L, p)
    out, dW, db, pos = got
    # dx is only read
    assert torch.equal(t['dx'], dx_before)
    y, v = t['y'], t['v']
    # dcat = y W: exact products of the bf16-rounded operands, only the summation order differs
    ref = (r16(y).double() @ r16(t['W']).double())
    err = (out.double() - ref).abs().max().item()
    scale = ref.abs().max().item()
    print('dcat err', err, 'scale', scale)
    assert err < 2e-5 * scale, (err, scale)
    # dW += y^T cat: no worse than twice today's kernel on the same operands (+ a rounding floor)
    refW = t['dW0'].double() + r16(y).double().t() @ r16(t['cat']).double()
    oldW = t['dW0'].clone()
    ops.wgrad_bf16(y.contiguous(), t['cat'], oldW)
    err_new = (dW.double() - refW).abs().max().item()
    err_old = (oldW.double() - refW).abs().max().item()
    print('dW err_new', err_new, 'err_old', err_old, 'scale', refW.abs().max().item())
    assert err_new <= 2 * err_old + 1e-6 * refW.abs().max().item(), (err_new, err_old)
    # db += colsum(y) from the fp32 values
    refb = t['db0'].double() + y.double().sum(0)
    errb = (db.double() - refb).abs().max().item()
    print('db err', errb)
    assert errb < 2e-3 * max(1.0, M / 40960), errb
    # d pos_emb[l] += sum over samples of v; rows >= L untouched
    refp = t['pos0'][:L].double() + v.view(B, L * d).double().sum(0).view(L, d)
    print('dpos err', (pos[:L].double() - refp).abs().max().item())
    assert torch.allclose(pos[:L].double(), refp, atol=1e-4 * max(1.0, B / 1000), rtol=1e-5)
    assert torch.equal(pos[L:], t['pos0'][L:])
    # deterministic
    again = _run(t, B, L, p)
    for a, b in zip(got, again):
        assert torch.equal(a, b)
    # the same bits when the reduction rides in a deferred flush
    with ops.deferred_reduce():
        deferred = _run(t, B, L, p)
    torch.cuda.synchronize()
    for a, b in zip(got, deferred):
        assert torch.equal(a, b)


def test_seq_input_bwd_switch_off_is_three_pass(bf16_mode, monkeypatch):
    """RSYS_SEQ_BWD_FUSED=0: the dropout backward, weight gradient and input gradient as before
    (the bits of the separate calls)."""
    B, L, d, dcat, p = 33, 50, 64, 40, 0.15
    t = _inputs(B, L, d, dcat, p)
    monkeypatch.setenv('RSYS_SEQ_BWD_FUSED', '0')
    assert not ops.seq_input_bwd_fused_ok(t['dx'], t['cat'], t['W'], t['dW0'], L)
    out, dW, db, pos = _run(t, B, L, p)
    dx2, dW2, db2, pos2 = t['dx'].clone(), t['dW0'].clone(), t['db0'].clone(), t['pos0'].clone()
    ops.seq_input_dropout_bwd(dx2, pos2, B, L * d, p, t['key'], 0, 1)
    ops.linear_bwd_weight(dx2, t['cat'], dW2, db=db2)
    out2 = ops.linear_bwd_input(dx2, t['W'])
    for a, b in zip((out, dW, db, pos), (out2, dW2, db2, pos2)):
        assert torch.equal(a, b)
    monkeypatch.setenv('RSYS_SEQ_BWD_FUSED', '1')
    assert ops.seq_input_bwd_fused_ok(t['dx'], t['cat'], t['W'], t['dW0'], L)


def test_seq_input_bwd_fused_has_the_unfused_bits(bf16_mode, monkeypatch):
    """35,200 rows (a multiple of 16 above the streaming threshold, 2.2 chunks per workgroup, the
    last one ragged): the unfused path runs the one-pass dropout backward, wgrad_bf16 and the bf16
    input-gradient GEMM, and the fused kernels reproduce all four outputs bit for bit -- the
    switch changes the time, not the training run."""
    B, L, d, dcat, p = 704, 50, 64, 40, 0.15
    t = _inputs(B, L, d, dcat, p)
    monkeypatch.setenv('RSYS_SEQ_BWD_FUSED', '0')
    unfused = _run(t, B, L, p)
    monkeypatch.setenv('RSYS_SEQ_BWD_FUSED', '1')
    assert ops.seq_input_bwd_fused_ok(t['dx'], t['cat'], t['W'], t['dW0'], L)
    fused = _run(t, B, L, p)
    for name, a, b in zip(('dcat', 'dW', 'db', 'dpos'), fused, unfused):
        assert torch.equal(a, b), (name, (a - b).abs().max().item())


@pytest.mark.parametrize('res', [False, True])
@pytest.mark.parametrize('M', [1650, 35008])
def test_linear_bwd_fused(M, res, bf16_mode, monkeypatch):
    """rs_linear_bwd_bf16 at the in-projection's shape (dY = dqkv [M, 192] bf16, X [M, 64],
    W [192, 64]): dx = dY W (+ dx_in, in place), dW += dY^T X, db += colsum(dY)."""
    monkeypatch.setenv('RSYS_LINBWD_FUSED', '1')
    N, K = 192, 64
    dy = rnd(M, N, seed=11).to(torch.bfloat16)
    x, W = rnd(M, K, seed=12), rnd(N, K, seed=13) * 0.1
    dW0, db0, dx0 = rnd(N, K, seed=14), rnd(N, seed=15), rnd(M, K, seed=16)
    assert ops.linear_bwd_fused_ok(dy, x, W, dW0)

    def run():
        dW, db = dW0.clone(), db0.clone()
        dx = ops.linear_bwd_fused(dy, x, W, dW, db, dx_in=dx0.clone() if res else None)
        torch.cuda.synchronize()
        return dx, dW, db

    got = run()
    dx, dW, db = got
    ref = dy.double() @ r16(W).double() + (dx0.double() if res else 0)
    err = (dx.double() - ref).abs().max().item()
    scale = ref.abs().max().item()
    print('dx err', err, 'scale', scale)
    assert err < 2e-5 * scale, (err, scale)
    refW = dW0.double() + dy.double().t() @ r16(x).double()
    oldW, oldb = dW0.clone(), db0.clone()
    ops.wgrad_bf16(dy, x, oldW, db=oldb)
    err_new = (dW.double() - refW).abs().max().item()
    err_old = (oldW.double() - refW).abs().max().item()
    print('dW err_new', err_new, 'err_old', err_old, 'scale', refW.abs().max().item())
    assert err_new <= 2 * err_old + 1e-6 * refW.abs().max().item(), (err_new, err_old)
    refb = db0.double() + dy.double().sum(0)
    errb = (db.double() - refb).abs().max().item()
    print('db err', errb)
    assert errb < 2e-3 * max(1.0, M / 40960), errb
    for a, b in zip(got, run()):
        assert torch.equal(a, b)
    # the row split, MFMA order and reduce of wgrad_bf16: its bits
    assert torch.equal(dW, oldW) and torch.equal(db, oldb)
    monkeypatch.setenv('RSYS_LINBWD_FUSED', '0')
    assert not ops.linear_bwd_fused_ok(dy, x, W, dW0)
    if M >= ops.STREAM_BF16_MIN_ROWS:  # the pair it replaces streams the bf16 dy: the same dx bits too
        old_dx = ops.linear_bwd_input(dy, W, out=dx0.clone(), beta=1.0) if res else ops.linear_bwd_input(dy, W)
        assert torch.equal(dx, old_dx)


@pytest.mark.parametrize('B', [700, 704])
def test_c2_step_fused_vs_unfused(B, monkeypatch):
    """One C2-structure step (dropout as configured, bf16, deterministic table gradients) with the
    one-pass backwards on (RSYS_SEQ_BWD_FUSED, RSYS_LINBWD_FUSED = 1) and off: the same loss
    bitwise, the same gradients bitwise except those downstream of the changed kernels (the
    sequence input's parameters and tables, in_proj, and layer 0 behind the last layer's dx),
    which stay within the bf16 mode's distance from the fp32 mode. B = 700: 35,000 tokens, not a
    multiple of 16, so qkv stays fp32 and only the sequence-input kernel runs, beside an unfused
    input gradient that is not the bf16 streaming GEMM; B = 704 stores dqkv as bf16, takes the
    in-projection kernel too, and every kernel replaced is a bf16 streaming one: there all
    gradients are bitwise the same."""
    from oracle.twotower_oracle import model_state_shapes
    from recommendsystemproject_amd import synth
    from recommendsystemproject_amd.flat import ensure_flat, grad_of
    from recommendsystemproject_amd.project.models.TwoTower.GenericTower import GenericTower
    from recommendsystemproject_amd.project.models.TwoTower.TwoTowerModel import TwoTowerModel
    from recommendsystemproject_amd.project.utils.training_utils import extract_item_id
    monkeypatch.setenv('RSYS_DETERMINISTIC', '1')
    cfg = yaml.safe_load(open(os.path.join(ROOT, 'configs', 'c2.yaml')))
    maps = {'user': synth.tower_layout(cfg['two_tower']['user_tower']),
            'item': synth.tower_layout(cfg['two_tower']['item_tower'])}
    shapes = {k: s for k, s, _ in model_state_shapes(cfg)}
    state = synth.make_state(shapes, seed=3)
    b = synth.batch_to_torch(synth.make_batch(cfg, B, seed=7), DEV)
    m = TwoTowerModel(GenericTower(cfg, 'user_tower'), GenericTower(cfg, 'item_tower'), maps['user'], maps['item'])
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in state.items()})
    m = m.to(DEV).train()
    f = ensure_flat(m)
    rng = [(mod, mod.rng_state.clone()) for mod in m.modules() if isinstance(getattr(mod, 'rng_state', None), torch.Tensor)]
    assert rng, 'no dropout state found'

    def step(mode, fused):
        monkeypatch.setenv('RSYS_SEQ_BWD_FUSED', fused)
        monkeypatch.setenv('RSYS_LINBWD_FUSED', fused)
        precision.set_compute_dtype(mode)
        try:
            for mod, s in rng:  # the same masks in every run
                mod.rng_state.copy_(s)
            f.zero_grad()
            U, I, H = m(b)
            loss = m.compute_loss(U, I, item_ids=extract_item_id(b['item_tower']), temperature=0.15)
            loss.backward()
            torch.cuda.synchronize()
            return loss.item(), {n: grad_of(p).clone() for n, p in m.named_parameters()}
        finally:
            precision.set_compute_dtype('fp32')

    l1, g1 = step('bf16', '1')
    l0, g0 = step('bf16', '0')
    l32, g32 = step('fp32', '0')
    assert l1 == l0  # the forward is unchanged
    touched = ('feature_embedder.feature_projection', 'feature_embedder.pos_emb', 'feature_embedder.embeddings',
               'in_proj', 'transformer_backbone.layers.0.')
    differ = []
    for n in g1:
        if torch.equal(g1[n], g0[n]):
            continue
        differ.append(n)
        assert any(k in n for k in touched), n
        cos = F.cosine_similarity(g1[n].flatten(), g0[n].flatten(), dim=0).item()
        d10 = (g1[n] - g0[n]).abs().max().item()
        d032 = (g0[n] - g32[n]).abs().max().item()
        print(n, 'cos', cos, 'max|fused - unfused|', d10, 'max|bf16 - fp32|', d032)
        assert cos >= 0.99, (n, cos)
        assert d10 < d032, (n, d10, d032)
    print('gradients that differ:', differ)
    if B == 704:
        assert not differ, differ


def test_misaligned_views_take_the_unfused_path(bf16_mode, monkeypatch):
    """The one-pass kernels load 16 bytes at a time: a view whose data does not start on a 16-byte
    boundary is not offered to them (the wrappers fall back; the entry points would refuse it)."""
    monkeypatch.setenv('RSYS_SEQ_BWD_FUSED', '1')
    monkeypatch.setenv('RSYS_LINBWD_FUSED', '1')

    def shifted(t):  # the same values, 4 (fp32) or 2 (bf16) bytes further on
        buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
        v = buf[1:].view(t.shape)
        v.copy_(t)
        return v

    B, L, d, dcat, p = 33, 50, 64, 40, 0.15
    t = _inputs(B, L, d, dcat, p)
    assert ops.seq_input_bwd_fused_ok(t['dx'], t['cat'], t['W'], t['dW0'], L)
    assert not ops.seq_input_bwd_fused_ok(shifted(t['dx']), t['cat'], t['W'], t['dW0'], L)
    got = _run(dict(t, dx=shifted(t['dx'])), B, L, p)  # falls back, does not raise
    monkeypatch.setenv('RSYS_SEQ_BWD_FUSED', '0')
    for a, b in zip(got, _run(t, B, L, p)):  # the unfused kernels on the same values: their bits
        assert torch.equal(a, b)
    M, N, K = 1650, 192, 64
    dy, x, W, dW = rnd(M, N, seed=21).to(torch.bfloat16), rnd(M, K, seed=22), rnd(N, K, seed=23), rnd(N, K, seed=24)
    assert ops.linear_bwd_fused_ok(dy, x, W, dW, rnd(M, K, seed=25))
    assert not ops.linear_bwd_fused_ok(shifted(dy), x, W, dW)
    assert not ops.linear_bwd_fused_ok(dy, shifted(x), W, dW)
    assert not ops.linear_bwd_fused_ok(dy, x, W, dW, shifted(rnd(M, K, seed=25)))


# ------------------------------------------------------------------------------------------
# Exact check of the shared weight-gradient tile and row split, independent of both sides of the
# fused-vs-unfused comparisons above (which now run the same tile code). Every operand is a small
# integer: dy / dx, x / cat, W and the starting dW, db, dx_in lie in [-4, 4], the masks of p = 0.5
# in {0, 2}. All of them are exact in bf16, and with at most 70,000 rows the largest sum is
# 4 * 4 * 4 * 70,000 = 4.48M < 2^24, so every partial and final sum is exact in fp32 whatever the
# order: the float64 torch reference, cast to fp32, must be met bit for bit.
EXACT_ROWS = [
    20,     # one ragged chunk
    48,     # one workgroup: a whole chunk and a ragged one
    64,     # two whole chunks: the paired loop with no tail
    150,    # two workgroups
    2050,   # 22 workgroups of three chunks: pair plus odd tail, ragged last workgroup
    70000,  # 438 workgroups of five chunks
]
EXACT_KEY = (4321, 7)


def ints(*shape, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-4, 5, shape, generator=g).float().to(DEV)


def mask(M, d, p, site):
    """The keep mask (scaled by 1 / (1 - p)) of rs_dropout_* at `site`; ones for p == 0."""
    ones = torch.ones(M, d, device=DEV)
    if p == 0:
        return ones
    key = torch.tensor(EXACT_KEY, dtype=torch.int64, device=DEV)
    m = ops.dropout_bwd(ones, p, key, site)
    assert p == 0.5 and bool(((m == 0) | (m == 2)).all())
    return m


def exact(got, ref64):
    torch.cuda.synchronize()
    ref = ref64.float()
    assert ref.abs().max().item() < 2 ** 24
    assert torch.equal(got, ref), (got - ref).abs().max().item()


@pytest.mark.parametrize('M', EXACT_ROWS)
@pytest.mark.parametrize('Mo,No,dy_bf16', [(64, 64, False), (64, 40, False), (192, 64, True)])
def test_wgrad_bf16_exact_on_integers(Mo, No, dy_bf16, M):
    dy, x = ints(M, Mo, seed=31), ints(M, No, seed=32)
    dW0, db0 = ints(Mo, No, seed=33), ints(Mo, seed=34)
    dW, db = dW0.clone(), db0.clone()
    ops.wgrad_bf16(dy.to(torch.bfloat16) if dy_bf16 else dy, x, dW, db=db)
    exact(dW, dW0.double() + dy.double().t() @ x.double())
    exact(db, db0.double() + dy.double().sum(0))


@pytest.mark.parametrize('M', EXACT_ROWS)
@pytest.mark.parametrize('dcat', [24, 40, 72])
def test_seq_input_bwd_fused_exact_on_integers(dcat, M):
    d, L, p = 64, 2, 0.5
    dx, cat, W = ints(M, d, seed=41), ints(M, dcat, seed=42), ints(d, dcat, seed=43)
    dW0, db0 = ints(d, dcat, seed=44), ints(d, seed=45)
    y = (dx * mask(M, d, p, 1) * mask(M, d, p, 0)).double()
    dW, db, pos = dW0.clone(), db0.clone(), torch.zeros(L, d, device=DEV)
    key = torch.tensor(EXACT_KEY, dtype=torch.int64, device=DEV)
    out = ops.seq_input_bwd_fused(dx, cat, W, L, p, key, 0, 1, dW, db, pos)
    exact(out, y @ W.double())
    exact(dW, dW0.double() + y.t() @ cat.double())
    exact(db, db0.double() + y.sum(0))


@pytest.mark.parametrize('M', EXACT_ROWS)
@pytest.mark.parametrize('p', [0.0, 0.5])
def test_outproj_bwd_fused_exact_on_integers(p, M):
    d, site = 64, 3
    dh, att, W = ints(M, d, seed=51), ints(M, d, seed=52), ints(d, d, seed=53)
    dW0, db0 = ints(d, d, seed=54), ints(d, seed=55)
    y = (dh * mask(M, d, p, site)).double()
    dW, db = dW0.clone(), db0.clone()
    key = torch.tensor(EXACT_KEY, dtype=torch.int64, device=DEV)
    datt = ops.outproj_bwd_fused(dh, att, W, p, key, site, dW, db)
    exact(datt, y @ W.double())
    exact(dW, dW0.double() + y.t() @ att.double())
    exact(db, db0.double() + y.sum(0))


@pytest.mark.parametrize('M', EXACT_ROWS)
@pytest.mark.parametrize('res', [False, True])
def test_linear_bwd_fused_exact_on_integers(res, M):
    N, K = 192, 64
    dy, x, W = ints(M, N, seed=61), ints(M, K, seed=62), ints(N, K, seed=63)
    dW0, db0, dx0 = ints(N, K, seed=64), ints(N, seed=65), ints(M, K, seed=66)
    dW, db = dW0.clone(), db0.clone()
    dx = ops.linear_bwd_fused(dy.to(torch.bfloat16), x, W, dW, db, dx_in=dx0.clone() if res else None)
    exact(dx, dy.double() @ W.double() + (dx0.double() if res else 0))
    exact(dW, dW0.double() + dy.double().t() @ x.double())
    exact(db, db0.double() + dy.double().sum(0))
