"""The one-pass backward of the attention out-projection in the bf16 compute mode
(csrc/linear_bwd.hip rs_outproj_bwd_bf16, behind functions._post_attn_bwd; RSYS_OUTPROJ_BWD_FUSED=0
reverts to the stored dsa and the two passes over it) and the FFN backward variant that no longer
stores dsa (csrc/ffn.hip). (A bf16 datt into the attention backward was built with this and taken
out again with its tests: bit-equal, but it made the step no faster)

Every comparison is bit for bit (torch.equal) against the kernels replaced:
wgrad_bf16_kernel<64, 64> with its reduce, and the bf16 streaming row GEMM
rowgemm_bf16_kernel<4, 1, false, 0, 0>. Nothing changes a summation order, so no tolerance applies.

How the references reach those kernels. ops.linear_bwd_weight takes wgrad_bf16_kernel from 2,048
rows on and a split-K tile GEMM below; ops.linear_bwd_input takes the bf16 streaming row GEMM from
32,768 rows (a multiple of 16) on and an fp32-MFMA row GEMM below. So at the small shapes
 * dW / db are compared with ops.wgrad_bf16 (the replaced kernel called directly), and with
   ops.linear_bwd_weight too wherever that is the same kernel (M >= 2048);
 * dx is compared with ops.linear_bwd_input on the same rows embedded at the top of a 32,768-row
   tensor (the streaming kernel computes each row from that row alone, and the mask of element
   m * 64 + c does not depend on the row count);
and one case at 35,008 rows compares with ops.linear_bwd_weight + ops.linear_bwd_input as they are.
For the same reason functions._post_attn_bwd offers the kernel only from 32,768 tokens on: the
pruned last layer's B rows keep their fp32-MFMA input gradient, so a training step computes what it
computed before. The fused FFN kernels need M % 16 == 0, so the no-dsa case beside M = 48 is 2,064
rows (129 row groups: a last workgroup with one live wave), not 2,050.
"""
import os

import numpy as np
import pytest
import torch
import yaml

from recommendsystemproject_amd import ops, precision

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIG = ops.STREAM_BF16_MIN_ROWS  # from here on the unfused input gradient is the bf16 streaming GEMM
SITE = 17


def rnd(*shape, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g).to(DEV)


@pytest.fixture
def bf16_mode():
    precision.set_compute_dtype('bf16')
    yield
    precision.set_compute_dtype('fp32')


def shifted(t):  # the same values, one element (4 or 2 bytes) further on: not 16-byte aligned
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    v = buf[1:].view(t.shape)
    v.copy_(t)
    return v


_REF = {}


def _case(M, p):
    """Inputs and the replaced kernels' outputs for (M, p), computed once and left unchanged."""
    if (M, p) in _REF:
        return _REF[(M, p)]
    assert precision.compute_dtype() == 'bf16'
    t = dict(dh=rnd(M, 64, seed=1), att=rnd(M, 64, seed=2), Wo=rnd(64, 64, seed=3) * 0.2,
             dW0=rnd(64, 64, seed=4), db0=rnd(64, seed=5),
             key=torch.tensor([4321, 7], dtype=torch.int64, device=DEV))
    dsa = t['dh'].clone()
    if p > 0:
        ops.dropout_bwd(dsa, p, t['key'], SITE)
    dW, db = t['dW0'].clone(), t['db0'].clone()
    ops.wgrad_bf16(dsa, t['att'], dW, db=db)
    if M >= 2048:  # ops.linear_bwd_weight is that kernel here
        dW2, db2 = t['dW0'].clone(), t['db0'].clone()
        ops.linear_bwd_weight(dsa, t['att'], dW2, db=db2)
        assert torch.equal(dW, dW2) and torch.equal(db, db2)
    if M >= BIG and M % 16 == 0:
        dx = ops.linear_bwd_input(dsa, t['Wo'])
    else:
        big = torch.zeros(BIG, 64, device=DEV)
        big[:M] = dsa
        dx = ops.linear_bwd_input(big, t['Wo'])[:M].clone()
    torch.cuda.synchronize()
    t.update(dW=dW, db=db, dx=dx)
    _REF[(M, p)] = t
    return t


def _fused(t, p):
    dW, db = t['dW0'].clone(), t['db0'].clone()
    dx = ops.outproj_bwd_fused(t['dh'], t['att'], t['Wo'], p, t['key'] if p > 0 else None, SITE, dW, db)
    return dx, dW, db


# 48: one workgroup, a 16-row tail chunk; 150: workgroups of 96 and 54 rows, a partial last chunk;
# 2050: 22 workgroups of 96 rows (three chunks each: the odd last chunk); 4096: even chunk pairs;
# 35008: the size class of the training path, where the unfused calls are the replaced kernels
@pytest.mark.parametrize('defer', [False, True])
@pytest.mark.parametrize('p', [0.0, 0.15])
@pytest.mark.parametrize('M', [48, 150, 2050, 4096, 35008])
def test_outproj_bwd_has_the_pair_bits(M, p, defer, bf16_mode):
    t = _case(M, p)
    dh_before = t['dh'].clone()
    with ops.deferred_reduce(defer):
        dx, dW, db = _fused(t, p)
    torch.cuda.synchronize()
    assert torch.equal(t['dh'], dh_before)  # dh is only read
    for name, a, b in (('dW', dW, t['dW']), ('db', db, t['db']), ('dx', dx, t['dx'])):
        assert a.shape == b.shape and torch.equal(a, b), (name, M, p, (a - b).abs().max().item())


def test_outproj_bwd_fallback(bf16_mode, monkeypatch):
    """Misaligned views, the fp32 mode, the switch and token counts below the streaming threshold
    are not offered to the kernel; _post_attn_bwd then runs the stored-dsa pair (the encoder test
    below compares the two paths on a whole step)."""
    monkeypatch.setenv('RSYS_OUTPROJ_BWD_FUSED', '1')
    M = 35008
    t = _case(M, 0.15)
    args = (t['att'], t['Wo'], t['dW0'])
    assert ops.outproj_bwd_fused_ok(t['dh'], *args)
    assert not ops.outproj_bwd_fused_ok(shifted(t['dh']), *args)
    assert not ops.outproj_bwd_fused_ok(t['dh'], shifted(t['att']), t['Wo'], t['dW0'])
    assert not ops.outproj_bwd_fused_ok(t['dh'][:4096], t['att'][:4096], t['Wo'], t['dW0'])
    assert not ops.outproj_bwd_fused_ok(t['dh'][:M - 8], t['att'][:M - 8], t['Wo'], t['dW0'])
    monkeypatch.setenv('RSYS_OUTPROJ_BWD_FUSED', '0')
    assert not ops.outproj_bwd_fused_ok(t['dh'], *args)
    monkeypatch.setenv('RSYS_OUTPROJ_BWD_FUSED', '1')
    precision.set_compute_dtype('fp32')
    assert not ops.outproj_bwd_fused_ok(t['dh'], *args)
    precision.set_compute_dtype('bf16')
    # the entry point refuses what the wrapper filters
    with pytest.raises(RuntimeError):
        _fused(dict(t, dh=shifted(t['dh'])), 0.15)


@pytest.mark.parametrize('p', [0.0, 0.15])
@pytest.mark.parametrize('M', [48, 2064])
def test_ffn_bwd_without_dsa(M, p, bf16_mode):
    """rs_ffn_bwd_ln2_bf16 with dsa not stored: dh1, dff and the four LayerNorm gradients carry the
    bits of the dsa-storing call, whose dsa is dh1 under dropout1's mask."""
    x = rnd(M, 64, seed=7)
    W1, b1 = rnd(256, 64, seed=1) * 0.15, rnd(256, seed=2) * 0.1
    W2, b2 = rnd(64, 256, seed=3) * 0.08, rnd(64, seed=4) * 0.1
    g, be = 1 + 0.1 * rnd(64, seed=5), 0.1 * rnd(64, seed=6)
    key = torch.tensor([4321, 6], dtype=torch.int64, device=DEV)
    h2, _, mu2, rs2, mask = ops.ffn_fwd_bf16(x, W1, b1, W2, b2, g, be, 1e-5, p, key, 18, 19)
    g2 = 1 + 0.1 * rnd(64, seed=14)
    dy2 = rnd(M, 64, seed=8)
    h1 = rnd(M, 64, seed=10) * 2 + 0.3
    g1 = 1 + 0.1 * rnd(64, seed=11)
    mu1 = h1.mean(1)
    rs1 = 1.0 / torch.sqrt(h1.var(1, unbiased=False) + 1e-5)
    init = [rnd(64, seed=20 + i) for i in range(4)]  # dgamma2, dbeta2, dgamma1, dbeta1

    def run(**kw):
        f = [t.clone() for t in init]
        dh1, dsa, dff = ops.ffn_bwd_ln2_bf16(x, W1, b1, W2, mask, dy2, h2, g2, mu2, rs2, f[0], f[1], h1, g1,
                                             mu1, rs1, f[2], f[3], p, key, 17, 19, **kw)
        torch.cuda.synchronize()
        return dh1, dsa, dff, f

    dh1, dsa, dff, f = run()
    dh1n, dsan, dffn, fn = run(dsa=False)
    assert dsan is None and (dsa is None) == (p == 0)
    assert torch.equal(dh1, dh1n) and torch.equal(dff, dffn)
    assert all(torch.equal(a, b) for a, b in zip(f, fn))
    if p > 0:  # what the one-pass out-projection backward rebuilds from dh1
        assert torch.equal(dsa, ops.dropout_bwd(dh1.clone(), p, key, 17))


def _c2_model(L):
    from oracle.twotower_oracle import model_state_shapes
    from recommendsystemproject_amd import synth
    from recommendsystemproject_amd.project.models.TwoTower.GenericTower import GenericTower
    from recommendsystemproject_amd.project.models.TwoTower.TwoTowerModel import TwoTowerModel
    cfg = yaml.safe_load(open(os.path.join(ROOT, 'configs', 'c2.yaml')))
    assert cfg['two_tower']['user_tower']['transformer_parameters']['n_layers'] == 2
    maps = {'user': synth.tower_layout(cfg['two_tower']['user_tower']),
            'item': synth.tower_layout(cfg['two_tower']['item_tower'])}
    shapes = {k: s for k, s, _ in model_state_shapes(cfg)}
    state = synth.make_state(shapes, seed=3)
    m = TwoTowerModel(GenericTower(cfg, 'user_tower'), GenericTower(cfg, 'item_tower'), maps['user'], maps['item'])
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in state.items()})
    return cfg, m.to(DEV).train()


# B = 41: the issue's size, below the streaming threshold (both layers keep the stored-dsa pair);
# 704 x 50 = 35,200 and 4,688 x 7 = 32,816 tokens (multiples of 16 above it): layer 0 takes the
# one-pass kernel, the pruned last layer (B rows) does not
@pytest.mark.parametrize('B,L', [(41, 50), (41, 7), (704, 50), (4688, 7)])
def test_encoder_step_fused_vs_unfused(B, L, monkeypatch):
    """One C2-structure step (two encoder layers, the last one pruned to the selected rows; padded
    histories with an all-padding sample; dropout as configured; bf16; deterministic table
    gradients) with RSYS_OUTPROJ_BWD_FUSED on and off: the same loss and bit-equal gradients of
    every parameter -- those of the sequence input's projection, positional rows and tables are
    functions of the dx that reaches it."""
    from recommendsystemproject_amd import functions, synth
    from recommendsystemproject_amd.flat import ensure_flat, grad_of
    from recommendsystemproject_amd.project.utils.training_utils import extract_item_id
    monkeypatch.setenv('RSYS_DETERMINISTIC', '1')
    cfg, m = _c2_model(L)
    b = synth.batch_to_torch(synth.make_batch(cfg, B, seed=7, seq_len=L, edge_cases=True), DEV)
    f = ensure_flat(m)
    rng = [(mod, mod.rng_state.clone()) for mod in m.modules() if isinstance(getattr(mod, 'rng_state', None), torch.Tensor)]
    assert rng, 'no dropout state found'
    assert functions.prune_last_layer()
    calls = []
    real = ops.outproj_bwd_fused
    monkeypatch.setattr(ops, 'outproj_bwd_fused', lambda *a, **k: (calls.append(a[0].shape[0]), real(*a, **k))[1])

    def step(fused):
        monkeypatch.setenv('RSYS_OUTPROJ_BWD_FUSED', fused)
        del calls[:]
        precision.set_compute_dtype('bf16')
        try:
            for mod, s in rng:  # the same masks in every run
                mod.rng_state.copy_(s)
            f.zero_grad()
            U, I, H = m(b)
            loss = m.compute_loss(U, I, item_ids=extract_item_id(b['item_tower']), temperature=0.15)
            loss.backward()
            torch.cuda.synchronize()
            return loss.item(), {n: grad_of(p).clone() for n, p in m.named_parameters()}, list(calls)
        finally:
            precision.set_compute_dtype('fp32')

    l1, g1, c1 = step('1')
    l0, g0, c0 = step('0')
    # the user tower's first layer (the item tower of this config has no sequence encoder to run)
    assert c0 == [] and c1 == ([B * L] if B * L >= BIG else [])
    assert l1 == l0 and np.isfinite(l1)
    for n in g1:
        assert torch.equal(g1[n], g0[n]), (n, (g1[n] - g0[n]).abs().max().item())
