"""The encoder forward's chained kernel (csrc/chain.h, RSYS_FWD_CHAIN): a Linear computed from the
rows the previous stage still holds on chip. rs_layer_tail_fwd_bf16 (out-proj + LN1 + FFN + LN2 +
the next layer's qkv) against the chain of separate kernels it replaces: bitwise, since every part
keeps its kernel's operation order; small row counts (below the separate bf16 streaming instances)
against torch, stage by stage. rs_ffn_wgrad_ln_bf16, which rebuilds the x1 that kernel does not
store, against rs_ffn_wgrad_bf16 on the stored x1.
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
NAMES = ('h1', 'x1', 'mean1', 'rstd1', 'h2', 'x2', 'mean2', 'rstd2', 'mask', 'qkv')


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


def _weights():
    w = dict(Wo=rnd(64, 64, seed=20) * 0.15, bo=0.1 * rnd(64, seed=21),
             g1=1 + 0.1 * rnd(64, seed=22), be1=0.1 * rnd(64, seed=23),
             W1=rnd(256, 64, seed=11) * 0.15, b1=0.1 * rnd(256, seed=12),
             W2=rnd(64, 256, seed=13) * 0.1, b2=0.1 * rnd(64, seed=14),
             g2=1 + 0.1 * rnd(64, seed=15), be2=0.1 * rnd(64, seed=16),
             Win=rnd(192, 64, seed=24) * 0.15, bin=0.1 * rnd(192, seed=25))
    return w


def _tail(att, resid, w, p, key, site, qkv=True, rows=None, bag=0, store_x1=True):
    return ops.layer_tail_fwd(att, w['Wo'], w['bo'], resid, w['g1'], w['be1'], 1e-5, w['W1'], w['b1'], w['W2'],
                              w['b2'], w['g2'], w['be2'], 1e-5, p, key, site,
                              Win=w['Win'] if qkv else None, bin_=w['bin'] if qkv else None, rows=rows, bag=bag,
                              store_x1=store_x1)


_CHAIN = {}


def _separate(M, p):
    """The chain the tail kernel replaces, once per (M, p): inputs and its outputs in NAMES order."""
    if (M, p) not in _CHAIN:
        att, resid, w = rnd(M, 64, seed=1), rnd(M, 64, seed=2), _weights()
        key = torch.tensor([4321, 7], dtype=torch.int64, device=DEV)
        h1, x1, m1, r1 = ops.linear_add_layernorm(att, w['Wo'], w['bo'], resid, w['g1'], w['be1'], 1e-5, p, key, 17)
        h2, x2, m2, r2, mask = ops.ffn_fwd_bf16(x1, w['W1'], w['b1'], w['W2'], w['b2'], w['g2'], w['be2'], 1e-5,
                                                p, key, 18, 19)
        qkv = ops.linear_fwd(x2, w['Win'], w['bin'], out_dtype=torch.bfloat16)
        assert qkv.dtype == torch.bfloat16
        _CHAIN[(M, p)] = (att, resid, w, key, (h1, x1, m1, r1, h2, x2, m2, r2, mask, qkv))
    return _CHAIN[(M, p)]


@pytest.mark.parametrize('with_qkv', [True, False])
@pytest.mark.parametrize('p', [0.0, 0.15])
@pytest.mark.parametrize('r', [0, 3])
def test_tail_bitwise_against_separate_kernels(r, p, with_qkv, bf16_mode):
    """M = 32768 + 16 r: the smallest row counts at which the separate bf16 streaming instances run
    (r = 3: the row groups do not divide evenly over the waves)."""
    M = 32768 + 16 * r
    att, resid, w, key, want = _separate(M, p)
    got = _tail(att, resid, w, p, key, 16, qkv=with_qkv)
    for name, a, b in zip(NAMES, got, want):
        if name == 'qkv' and not with_qkv:
            assert a is None
            continue
        assert torch.equal(a, b), (name, (a.float() - b.float()).abs().max().item())
    # x1 not stored: nothing else changes
    lean = _tail(att, resid, w, p, key, 16, qkv=with_qkv, store_x1=False)
    assert lean[1] is None
    for name, a, b in zip(NAMES, lean, got):
        assert name == 'x1' or (a is None and b is None) or torch.equal(a, b), name


@pytest.mark.parametrize('M', [64, 4096 + 16])
def test_ffn_wgrad_ln_bitwise_against_stored_x1(M, bf16_mode):
    """rs_ffn_wgrad_ln_bf16 rebuilds x1 = LN1(h1) while staging; rs_ffn_wgrad_bf16 reads the x1 the
    forward stored. M = 64: one chunk; 4096 + 16: several workgroups and a ragged last chunk."""
    att, resid, w, p = rnd(M, 64, seed=31), rnd(M, 64, seed=32), _weights(), 0.15
    key = torch.tensor([77, 1], dtype=torch.int64, device=DEV)
    h1, x1, m1, r1, _, _, _, _, mask, _ = _tail(att, resid, w, p, key, 16, qkv=False)
    dff = rnd(M, 64, seed=33)
    grads = []
    for rebuilt in (False, True):
        g = [torch.zeros_like(w[n]) for n in ('W1', 'b1', 'W2', 'b2')]
        if rebuilt:
            ops.ffn_wgrad_ln_bf16(h1, m1, r1, w['g1'], w['be1'], w['W1'], w['b1'], w['W2'], mask, dff, p, *g)
        else:
            ops.ffn_wgrad_bf16(x1, w['W1'], w['b1'], w['W2'], mask, dff, p, *g)
        grads.append(g)
    assert grads[0][0].abs().max().item() > 0
    for name, a, b in zip(('dW1', 'db1', 'dW2', 'db2'), *grads):
        assert torch.equal(a, b), (name, (a - b).abs().max().item())


def _ln(h, g, b):
    mu = h.mean(1, keepdim=True)
    var = ((h - mu) ** 2).mean(1, keepdim=True)
    rs = 1.0 / torch.sqrt(var + 1e-5)
    return (h - mu) * rs * g + b, mu[:, 0], rs[:, 0]


def _allclose(name, a, b, atol, rtol):
    return torch.allclose(a, b, atol=atol, rtol=rtol)


def _check_ffn_against_torch(x1, w, ffn_out, p=0.0, masks=None, close=_allclose):
    """The feed-forward half of _check_tail_against_torch: ffn_out = (h2, x2, mean2, rstd2, mask) of
    rs_ffn_fwd_bf16 or of the tail kernel on the rows x1. masks: the multipliers (0 or 1/(1-p)) of
    the FFN's inner dropout [M, 256] and of dropout2 [M, 64], from somewhere else than the library;
    the absolute bounds grow by the 1/(1-p) the kept values are scaled by."""
    h2, x2, m2, r2, mask = ffn_out
    s = 1.0 / (1.0 - p)
    za, zb = masks if masks is not None else (1.0, 1.0)
    # f1 never leaves the forward kernel. torch's own f1 would be rounded to bf16 from a sum with
    # another fp32 summation order, and one element that lands on the other side of a rounding
    # boundary moves h2 by far more than the bound below. So f1 is the library's: rs_ffn_bwd_bf16
    # recomputes it in the forward's operation order (bit-exact with the forward's f1,
    # test_fused_ffn_matches_unfused) and writes it out; torch checks it to one bf16 step and then
    # does the W2 product, the residual and LN2.
    zero = torch.zeros_like(x1)
    f1 = ops.ffn_bwd_bf16(x1, w['W1'], w['b1'], w['W2'], mask, zero, zero, p)[1].float()
    f1r = torch.relu(r16(x1) @ r16(w['W1']).t() + w['b1']) * za
    assert close('f1', f1, f1r, 1e-5 * s, 2.0 ** -7)
    h2r = x1 + (f1 @ r16(w['W2']).t() + w['b2']) * zb
    assert close('h2', h2, h2r, 2e-5 * s, 1e-5)
    x2r, m2r, r2r = _ln(h2, w['g2'], w['be2'])
    assert close('x2', x2, x2r, 1e-4, 1e-4)
    assert torch.allclose(m2, m2r, atol=1e-5) and torch.allclose(r2, r2r, rtol=1e-4)


def _check_tail_against_torch(att, res_rows, w, got, p=0.0, masks=None, close=_allclose):
    """Stage by stage on the kernel's own intermediate rows, so that a bf16 rounding flip of an
    operand (x1, f1, x2 differ from torch's in the last fp32 bits) cannot enter the comparison:
    torch fp32 products of bf16-rounded operands differ from the MFMA's in summation order only.
    masks: the multipliers of dropout1 [M, 64] and of the FFN's two sites (_check_ffn_against_torch).
    close(name, a, b, atol, rtol): the comparison of each masked stage (default torch.allclose)."""
    h1, x1, m1, r1, h2, x2, m2, r2, mask, qkv = got
    s = 1.0 / (1.0 - p)
    z1 = masks[0] if masks is not None else 1.0
    h1r = res_rows + (r16(att) @ r16(w['Wo']).t() + w['bo']) * z1
    assert close('h1', h1, h1r, 2e-5 * s, 1e-5)
    x1r, m1r, r1r = _ln(h1, w['g1'], w['be1'])
    assert torch.allclose(x1, x1r, atol=1e-4, rtol=1e-4)
    assert torch.allclose(m1, m1r, atol=1e-5) and torch.allclose(r1, r1r, rtol=1e-4)
    _check_ffn_against_torch(x1, w, (h2, x2, m2, r2, mask), p, masks[1:] if masks is not None else None, close)
    if qkv is not None:
        # bf16 storage: within one bf16 ulp (2^-7 relative) of the fp32 product
        qr = r16(x2) @ r16(w['Win']).t() + w['bin']
        assert torch.allclose(qkv.float(), qr, atol=1e-4, rtol=2.0 ** -7)


@pytest.mark.parametrize('M', [16, 48])
def test_tail_fewer_groups_than_waves(M, bf16_mode):
    att, resid, w = rnd(M, 64, seed=3), rnd(M, 64, seed=4), _weights()
    got = _tail(att, resid, w, 0.0, None, 16)
    _check_tail_against_torch(att, resid, w, got)
    # and the chain of separate kernels has small-M bf16 instances too: the same bits
    h1, x1, m1, r1 = ops.linear_add_layernorm(att, w['Wo'], w['bo'], resid, w['g1'], w['be1'], 1e-5)
    h2, x2, m2, r2, mask = ops.ffn_fwd_bf16(x1, w['W1'], w['b1'], w['W2'], w['b2'], w['g2'], w['be2'], 1e-5, 0.0,
                                            None, 18, 19)
    for name, a, b in zip(NAMES, got, (h1, x1, m1, r1, h2, x2, m2, r2, mask)):
        assert torch.equal(a, b), name


def test_tail_residual_row_index(bf16_mode):
    M, bag = 64, 5
    att, table, w = rnd(M, 64, seed=5), rnd(M * bag, 64, seed=6), _weights()
    rows = torch.randint(0, bag, (M,), generator=torch.Generator().manual_seed(7)).to(DEV)
    got = _tail(att, table, w, 0.0, None, 16, rows=rows, bag=bag)
    picked = table.view(M, bag, 64)[torch.arange(M, device=DEV), rows]
    _check_tail_against_torch(att, picked, w, got)
    same = _tail(att, picked.contiguous(), w, 0.0, None, 16)
    for name, a, b in zip(NAMES, got, same):
        assert torch.equal(a, b), name


def test_fwd_chain_bad_args(bf16_mode):
    w = _weights()
    with pytest.raises(RuntimeError):  # M % 16 != 0
        _tail(rnd(40, 64), rnd(40, 64), w, 0.0, None, 16)
    with pytest.raises(RuntimeError):  # F != 256
        ops.layer_tail_fwd(rnd(64, 64), w['Wo'], w['bo'], rnd(64, 64), w['g1'], w['be1'], 1e-5, w['W1'][:128],
                           w['b1'][:128], w['W2'][:, :128].contiguous(), w['b2'], w['g2'], w['be2'], 1e-5, 0.0,
                           None, 16)
    with pytest.raises(RuntimeError):  # null operand
        ops.layer_tail_fwd(rnd(64, 64), w['Wo'], None, rnd(64, 64), w['g1'], w['be1'], 1e-5, w['W1'], w['b1'],
                           w['W2'], w['b2'], w['g2'], w['be2'], 1e-5, 0.0, None, 16)
    with pytest.raises(RuntimeError):  # rs_ffn_wgrad_ln_bf16: M % 16 != 0, null statistics
        ops.ffn_wgrad_ln_bf16(rnd(40, 64), rnd(40), rnd(40), w['g1'], w['be1'], w['W1'], w['b1'], w['W2'],
                              torch.zeros(160, dtype=torch.int64, device=DEV), rnd(40, 64), 0.0,
                              *[torch.zeros_like(w[n]) for n in ('W1', 'b1', 'W2', 'b2')])
    with pytest.raises(RuntimeError):
        ops.ffn_wgrad_ln_bf16(rnd(64, 64), None, rnd(64), w['g1'], w['be1'], w['W1'], w['b1'], w['W2'],
                              torch.zeros(256, dtype=torch.int64, device=DEV), rnd(64, 64), 0.0,
                              *[torch.zeros_like(w[n]) for n in ('W1', 'b1', 'W2', 'b2')])
    with pytest.raises(RuntimeError):  # Win without its bias
        ops.layer_tail_fwd(rnd(64, 64), w['Wo'], w['bo'], rnd(64, 64), w['g1'], w['be1'], 1e-5, w['W1'], w['b1'],
                           w['W2'], w['b2'], w['g2'], w['be2'], 1e-5, 0.0, None, 16, Win=w['Win'])


def test_fwd_chain_switch_same_step(monkeypatch):
    """RSYS_FWD_CHAIN=0 (the separate kernels) against the default on one demo-config training step
    with dropout on, at a token count where the tail kernel also emits the next layer's qkv: the same loss and gradients,
    bitwise in deterministic mode."""
    from oracle.twotower_oracle import model_state_shapes
    from recommendsystemproject_amd import synth
    from recommendsystemproject_amd.flat import ensure_flat
    from recommendsystemproject_amd.project.models.TwoTower.GenericTower import GenericTower
    from recommendsystemproject_amd.project.models.TwoTower.TwoTowerModel import TwoTowerModel
    from recommendsystemproject_amd.project.utils.training_utils import extract_item_id
    monkeypatch.setenv('RSYS_DETERMINISTIC', '1')
    cfg = yaml.safe_load(open(os.path.join(ROOT, 'configs', 'demo.yaml')))
    maps = {'user': synth.tower_layout(cfg['two_tower']['user_tower']),
            'item': synth.tower_layout(cfg['two_tower']['item_tower'])}
    shapes = {k: s for k, s, _ in model_state_shapes(cfg)}
    m = TwoTowerModel(GenericTower(cfg, 'user_tower'), GenericTower(cfg, 'item_tower'), maps['user'], maps['item'])
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in synth.make_state(shapes, seed=2).items()})
    m = m.to(DEV).train()
    b = synth.batch_to_torch(synth.make_batch(cfg, 2048, seed=9), DEV)  # 2048 x 20 = 40,960 tokens
    f = ensure_flat(m)
    # the dropout streams ({seed, counter} per module) restart for the second pass
    rng = [(mod, mod.rng_state.clone()) for mod in m.modules() if isinstance(getattr(mod, 'rng_state', None),
                                                                             torch.Tensor)]
    assert rng
    calls = {'tail': 0, 'lean': 0, 'wgrad_ln': 0}
    tail, wgln = ops.layer_tail_fwd, ops.ffn_wgrad_ln_bf16

    def tail_spy(*a, **k):
        calls['tail'] += 1
        calls['lean'] += k.get('store_x1') is False and k.get('Win') is not None
        return tail(*a, **k)

    def wgln_spy(*a, **k):
        calls['wgrad_ln'] += 1
        return wgln(*a, **k)

    monkeypatch.setattr(ops, 'layer_tail_fwd', tail_spy)
    monkeypatch.setattr(ops, 'ffn_wgrad_ln_bf16', wgln_spy)
    out = {}
    precision.set_compute_dtype('bf16')
    try:
        for mode in ('1', '0'):
            monkeypatch.setenv('RSYS_FWD_CHAIN', mode)
            for mod, st in rng:
                mod.rng_state.copy_(st)
            f.zero_grad()
            U, I, H = m(b)
            loss = m.compute_loss(U, I, item_ids=extract_item_id(b['item_tower']), temperature=0.15)
            loss.backward()
            torch.cuda.synchronize()
            out[mode] = (loss.item(), f.grad.clone(), dict(calls))
    finally:
        precision.set_compute_dtype('fp32')
    # the tail kernel ran, with the next layer's qkv and without x1, which the backward rebuilt ...
    assert out['1'][2]['tail'] >= 1 and out['1'][2]['lean'] >= 1 and out['1'][2]['wgrad_ln'] >= 1
    assert out['0'][2] == out['1'][2]  # ... and not with the switch off
    assert out['0'][0] == out['1'][0]
    assert torch.equal(out['0'][1], out['1'][1])
