"""Every dropout site against an independent mask reference. The masks come from tests/dropout_ref.py
(the numpy mirror of csrc/rng.h, pinned and checked against the header by test_dropout_ref_host.py),
the operation from float64 torch with the mask multiplied in where the reference model applies
F.dropout, autograd for the backward. No mask and no expected value comes from another kernel. Two
references do take intermediate values from the library, for the reason written at each: the
stage-by-stage forward references of the fused bf16 kernels read f1 back through rs_ffn_bwd_bf16 (as
test_gpu_fwd_chain's dropout-free reference does), and _post_attn_ref takes the rows x1 the kernels
are given, the forward's h2, and its ReLU decisions within 1e-5 of zero.

Bounds. fp32 kernels: the atol / rtol of the same kernel's dropout-free test, atol times 1/(1-p)
(kept values are scaled by exactly that factor, so their rounding error is too). bf16 kernels: the
dropout-free bounds relative to the reference's own maximum (the reference carries the 1/(1-p)).
Where a kernel's dropout-free test has no bound against an independent reference (the weight
gradients of rs_outproj_bwd_bf16 and rs_seq_input_bwd_bf16 are bounded there by the replaced
kernel's error), the bound is the one another test sets for the same error, named at the place.
Every comparison also has to tell the right mask from a wrong one: the same reference built with the
masks of site + 1 must miss the kernel by at least 10 times the bound."""
import math
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F
import yaml

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import dropout_ref as dr  # noqa: E402
from recommendsystemproject_amd import _hip, functions, ops, precision  # noqa: E402
from test_gpu_bf16 import _bf16_attention_ref  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the host test's p values and keys
PS = [0.0, 1e-6, 0.1, 0.5, 0.99999, 1.0]
KEYS = [(1234, 7), (77, 3), (-5, 2 ** 40), (-2 ** 63, 0), (2 ** 63 - 1, 2 ** 40 + 3)]


def rnd(*shape, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g).to(DEV)


def r16(t):
    return t.to(torch.bfloat16).float()


def key_t(seed, counter):
    return torch.tensor([seed, counter], dtype=torch.int64, device=DEV)


def mult_t(key, site, p, idx):
    """The mirror's multipliers of element indices idx (numpy) as a float32 device tensor."""
    return torch.from_numpy(dr.mult(key[0], key[1], site, p, idx)).to(DEV)


@pytest.fixture
def bf16_mode():
    precision.set_compute_dtype('bf16')
    yield
    precision.set_compute_dtype('fp32')


def inv(p):
    return 1.0 / (1.0 - p)


def excess(got, ref, rtol):
    """max(|got - ref| - rtol |ref|): `got` is allclose(ref, atol, rtol) iff this is <= atol."""
    got, ref = got.double(), ref.double()
    return ((got - ref).abs() - rtol * ref.abs()).max().item()


def check_close(name, got, ref, wrong, atol, rtol=0.0):
    """got within atol + rtol |ref| of ref, and at least 10 atol (past rtol |wrong|) from `wrong`,
    the same reference under another site's masks."""
    e, w = excess(got, ref, rtol), excess(got, wrong, rtol)
    print(f'{name}: err {e:.3e} (bound {atol:.3e}); wrong mask {w:.3e}')
    assert e <= atol, (name, e, atol)
    assert w >= 10 * atol, (name, 'does not tell a wrong mask', w, atol)


def check_rel(name, got, ref, wrong, max_tol, mean_tol=None):
    """max (and mean) |got - ref| relative to max |ref|; the wrong-mask reference at >= 10x."""
    got, ref, wrong = got.double(), ref.double(), wrong.double()
    sc = ref.abs().max().item()
    err, werr = (got - ref).abs(), (got - wrong).abs()
    print(f'{name}: max {err.max().item() / sc:.3e} (bound {max_tol:.1e}) mean {err.mean().item() / sc:.3e}'
          f' (bound {mean_tol}); wrong mask max {werr.max().item() / sc:.3e} mean {werr.mean().item() / sc:.3e}')
    assert err.max().item() < max_tol * sc, (name, err.max().item() / sc)
    assert werr.max().item() >= 10 * max_tol * sc, (name, 'does not tell a wrong mask', werr.max().item() / sc)
    if mean_tol is not None:
        assert err.mean().item() < mean_tol * sc, (name, err.mean().item() / sc)
        assert werr.mean().item() >= 10 * mean_tol * sc, (name, 'wrong mask, mean', werr.mean().item() / sc)


# =========================================================================== a. the mask kernels
@pytest.mark.parametrize('with_aux', [False, True])
@pytest.mark.parametrize('M,N', [(1, 1), (3, 5), (37, 64), (1000, 48)])
def test_dropout_kernels_bit_exact(M, N, with_aux):
    x0 = rnd(M, N, seed=1)
    Lm = 7
    aux = rnd(Lm, N, seed=2) if with_aux else None
    idx = dr.rows(M, N)
    combos = [(KEYS[i % len(KEYS)], PS[i % len(PS)], site) for i, site in
              enumerate([0, 1, 16, 17, 18, 19, 24, 27, 256, 257, 3, 5])]
    combos += [(KEYS[0], 0.25, 3), (KEYS[1], 0.1, 5)]  # the pinned keys
    for key, p, site in combos:
        m = mult_t(key, site, p, idx)
        kd = key_t(*key)
        x = x0.clone()
        ops.dropout_fwd(x, p, kd, site, aux=aux, aux_mod=Lm if with_aux else 0)
        base = x0 + aux[torch.arange(M, device=DEV) % Lm] if with_aux else x0
        assert torch.equal(x, base * m), (key, p, site)
        g = x0.clone()
        ops.dropout_bwd(g, p, kd, site)
        assert torch.equal(g, x0 * m), (key, p, site)


def test_rng_next_counts_the_mirrors_counter():
    state = key_t(-5, 2 ** 40)
    k1, k2 = ops.rng_next(state), ops.rng_next(state)
    assert k1.tolist() == [-5, 2 ** 40] and k2.tolist() == [-5, 2 ** 40 + 1] and state.tolist() == [-5, 2 ** 40 + 2]
    x0 = rnd(37, 64, seed=3)
    idx = dr.rows(37, 64)
    outs = []
    for k, counter in ((k1, 2 ** 40), (k2, 2 ** 40 + 1)):
        x = x0.clone()
        ops.dropout_fwd(x, 0.3, k, 257)
        assert torch.equal(x, x0 * mult_t((-5, counter), 257, 0.3, idx))
        outs.append(x)
    assert not torch.equal(outs[0], outs[1])


@pytest.mark.parametrize('B,L,d,p', [(37, 7, 64, 0.3), (300, 20, 16, 0.5)])
def test_seq_input_dropout_bwd(B, L, d, p):
    key = KEYS[1]
    dx0 = rnd(B * L, d, seed=3)
    pos0 = rnd(L + 5, d, seed=4)
    idx = dr.rows(B * L, d)
    ma, mb = mult_t(key, 0, p, idx), mult_t(key, 1, p, idx)
    got, pg = dx0.clone(), pos0.clone()
    ops.seq_input_dropout_bwd(got, pg, B, L * d, p, key_t(*key), 0, 1)
    assert torch.equal(got, dx0 * mb * ma)
    assert torch.equal(pg[L:], pos0[L:])

    def pos_ref(m):
        return pos0[:L].double() + (dx0.double() * m.double()).view(B, L, d).sum(0)
    # test_seq_input_dropout_bwd_fused's colsum bound, times 1/(1-p)
    check_close('pos_grad', pg[:L], pos_ref(mb), pos_ref(mult_t(key, 2, p, idx)),
                atol=1e-4 * max(1.0, B / 1000) * inv(p), rtol=1e-5)


# ============================================================================== b. attention
def _lens(B, L):
    return torch.tensor(([L, 1, max(1, L // 2), min(3, L), max(1, L - 1)])[:B])


_ATTN = {}


def _attn_case(B, L, d, H, p, site, selected=False):
    """Inputs of one attention case, built once: padding with lengths that include 1 and L, and a
    key under which (by the mirror) some (b, h, query) row has every unmasked key dropped
    (selected: a row i = last[b] among them)."""
    k = (B, L, d, H, p, site, selected)
    if k in _ATTN:
        return _ATTN[k]
    seq = (torch.arange(L)[None, :] < _lens(B, L)[:, None]).long().to(DEV)
    key_pad, last = ops.seq_mask(seq, 0)
    valid = ~key_pad.bool().cpu().numpy()
    assert valid.any(1).all()  # no sample is all padding: seq_mask had nothing to rewrite
    assert (valid.sum(1) == 1).any() and valid.all(1).any()
    idx = dr.attn(B, H, L)
    last_np = last.cpu().numpy()
    for counter in range(200):
        keep = dr.keep(4321, counter, site, p, idx)
        dead = ~(keep & valid[:, None, None, :]).any(-1)  # [B, H, L]
        if dead[np.arange(B), :, last_np].any() if selected else dead.any():
            break
    assert dead.any() and (not selected or dead[np.arange(B), :, last_np].any()), \
        'no (b, h, query) row with all of its keys dropped'
    key = (4321, counter)
    t = dict(qkv=rnd(B * L, 3 * d, seed=1 + L), dout=rnd(B * L, d, seed=2 + L), key_pad=key_pad, last=last, key=key,
             kd=key_t(*key), dead=torch.from_numpy(dead).to(DEV),
             Z=mult_t(key, site, p, idx).double(), Zw=mult_t(key, site + 1, p, idx).double())
    _ATTN[k] = t
    return t


def _attention_ref64(qkv, key_pad, dout, Z, B, L, d, H):
    """softmax(masked scores) * Z @ V in float64, backward by autograd -> (out, dqkv)."""
    hd = d // H
    x = qkv.double().clone().requires_grad_(True)
    q, k, v = x.view(B, L, 3, H, hd).permute(2, 0, 3, 1, 4)
    s = (q @ k.transpose(-1, -2) / math.sqrt(hd)).masked_fill(key_pad.bool()[:, None, None, :], float('-inf'))
    out = ((torch.softmax(s, -1) * Z) @ v).transpose(1, 2).reshape(B * L, d)
    out.backward(dout.double())
    return out.detach(), x.grad


def _assert_dead_rows_zero(t, out, dqkv, B, L, d, H):
    """A query row whose unmasked keys were all dropped: its output and dQ are exactly 0."""
    hd = d // H
    dead = t['dead'].permute(0, 2, 1)  # [B, L, H]
    o = out.float().view(B, L, H, hd)
    dq = dqkv.float().view(B, L, 3, H, hd)[:, :, 0]
    assert dead.any()
    assert torch.count_nonzero(o[dead]) == 0 and torch.count_nonzero(dq[dead]) == 0


ATTN_CASES = (
    [('valu', 'fp32', (3, 50, 32, 4), False), ('valu', 'fp32', (2, 100, 64, 4), False)] +
    [('wave_f32', 'fp32', (3 + L % 3, L, 64, 4), False) for L in (7, 16, 33, 50, 64)] +
    [('wave_bf16', 'bf16', (3 + L % 3, L, 64, 4), st) for L in (7, 16, 33, 50, 64) for st in (False, True)] +
    [('long_bf16', 'bf16', (3, L, 64, 4), st) for L in (65, 100) for st in (False, True)])


def _route(mode, shape, stored_bf16, p, bwd):
    flags = (_hip.RS_GEMM_BF16 if mode == 'bf16' else 0) | (_hip.RS_ATTN_QKV_BF16 if stored_bf16 else 0)
    return ops.attn_plan(*shape, p, flags, bwd).route_name


def test_attention_cases_reach_every_route():
    names = {_route(mode, shape, st, 0.1, bwd) for _, mode, shape, st in ATTN_CASES for bwd in (False, True)}
    assert names == set(_hip.ATTN_ROUTES)


@pytest.mark.parametrize('p', [0.1, 0.5])
@pytest.mark.parametrize('route,mode,shape,stored_bf16', ATTN_CASES,
                         ids=[f'{r}-L{s[1]}-d{s[2]}-{"q16" if st else "q32"}' for r, _, s, st in ATTN_CASES])
def test_attention_against_float64(route, mode, shape, stored_bf16, p):
    B, L, d, H = shape
    site = 16
    t = _attn_case(B, L, d, H, p, site)
    qkv = t['qkv'].to(torch.bfloat16) if stored_bf16 else t['qkv']
    precision.set_compute_dtype(mode)
    try:
        for bwd in (False, True):
            assert ops.attn_plan(B, L, d, H, p, ops._attn_flags(qkv), bwd).route_name == route
        out, lse = ops.attn_fwd(qkv, t['key_pad'], B, L, d, H, p, t['kd'], site)
        grads = [ops.attn_bwd(qkv, t['key_pad'], out, t['dout'], lse, B, L, d, H, p, t['kd'], site)]
        if route.startswith('wave'):  # above: the forward's saved keep bits (wave_bf16); here: drawn again
            saved = ops.attn_plan(B, L, d, H, p, ops._attn_flags(qkv), True).zbits_words > 0
            assert saved == (route == 'wave_bf16')
            assert (lse.untyped_storage().nbytes() > 4 * lse.numel()) == saved
            grads.append(ops.attn_bwd(qkv, t['key_pad'], out, t['dout'], lse.clone(), B, L, d, H, p, t['kd'], site))
    finally:
        precision.set_compute_dtype('fp32')
    torch.cuda.synchronize()
    if mode == 'fp32':
        ro, rg = _attention_ref64(qkv, t['key_pad'], t['dout'], t['Z'], B, L, d, H)
        wo, wg = _attention_ref64(qkv, t['key_pad'], t['dout'], t['Zw'], B, L, d, H)
        # test_attention_fwd_bwd's bounds
        check_close('out', out, ro, wo, atol=2e-5 * inv(p), rtol=1e-4)
        for g in grads:
            check_close('dqkv', g, rg, wg, atol=5e-5 * inv(p), rtol=1e-4)
    else:
        ro, rg = _bf16_attention_ref(qkv.float(), t['key_pad'], t['dout'], B, L, d, H, drop=t['Z'])
        wo, wg = _bf16_attention_ref(qkv.float(), t['key_pad'], t['dout'], B, L, d, H, drop=t['Zw'])
        if stored_bf16:  # dqkv is stored as bf16: so is the reference's
            rg, wg = r16(rg), r16(wg)
        # test_bf16_attention's bounds
        check_rel('out', out, ro, wo, 5e-3, 1.5e-4)
        for g in grads:
            assert g.dtype == qkv.dtype
            check_rel('dqkv', g, rg, wg, 5e-3, 1.5e-4)
    for g in grads:
        _assert_dead_rows_zero(t, out, g, B, L, d, H)


@pytest.mark.parametrize('p', [0.1, 0.5])
@pytest.mark.parametrize('mode', ['fp32', 'bf16'])
@pytest.mark.parametrize('L', [7, 50])
def test_attention_rows_against_float64(L, mode, p):
    """The pruned last layer's attention: the query rows i = last[b] only."""
    B, d, H, site = 4, 64, 4, 24
    hd = d // H
    t = _attn_case(B, L, d, H, p, site, selected=True)
    qkv, last = t['qkv'], t['last']
    dsel = rnd(B, d, seed=5)
    precision.set_compute_dtype(mode)
    try:
        assert ops.attn_plan(B, L, d, H, p, ops._attn_flags(qkv)).rows_ok
        out, lse = ops.attn_rows_fwd(qkv, t['key_pad'], last, B, L, d, H, p, t['kd'], site)
        dqkv = ops.attn_rows_bwd(qkv, t['key_pad'], last, dsel, lse, B, L, d, H, p, t['kd'], site)
    finally:
        precision.set_compute_dtype('fp32')
    torch.cuda.synchronize()
    sel = torch.arange(B, device=DEV) * L + last
    dfull = torch.zeros(B * L, d, device=DEV)
    dfull[sel] = dsel
    # the selected rows of the mirror's index helper are the selected rows of the full masks
    rows_idx = dr.attn_rows(B, H, L, last.cpu().numpy())
    zr = mult_t(t['key'], site, p, rows_idx).double()
    assert torch.equal(zr, t['Z'][torch.arange(B, device=DEV), :, last, :])
    live = torch.zeros(B, L, dtype=torch.bool, device=DEV)
    live[torch.arange(B, device=DEV), last] = True

    def computed(g):
        """What the kernel computes of dqkv: dK and dV of every key and dQ of the selected rows (dQ of
        the other rows is a stored zero, asserted below: it would only dilute a mean)."""
        g = g.view(B, L, 3, d)
        return torch.cat([g[:, :, 0][live].reshape(-1), g[:, :, 1:].reshape(-1)])
    if mode == 'fp32':
        ro, rg = _attention_ref64(qkv, t['key_pad'], dfull, t['Z'], B, L, d, H)
        wo, wg = _attention_ref64(qkv, t['key_pad'], dfull, t['Zw'], B, L, d, H)
        check_close('out', out, ro[sel], wo[sel], atol=2e-5 * inv(p), rtol=1e-4)
        check_close('dqkv', computed(dqkv), computed(rg), computed(wg), atol=5e-5 * inv(p), rtol=1e-4)
    else:
        ro, rg = _bf16_attention_ref(qkv, t['key_pad'], dfull, B, L, d, H, drop=t['Z'], rows=True)
        wo, wg = _bf16_attention_ref(qkv, t['key_pad'], dfull, B, L, d, H, drop=t['Zw'], rows=True)
        check_rel('out', out, ro[sel], wo[sel], 5e-3, 1.5e-4)
        check_rel('dqkv', computed(dqkv), computed(rg), computed(wg), 5e-3, 1.5e-4)
    # dQ is zero off the selected rows, and on a selected row whose keys were all dropped
    dq = dqkv.view(B, L, 3, H, hd)[:, :, 0]
    assert torch.count_nonzero(dq[~live]) == 0
    dead_sel = t['dead'][torch.arange(B, device=DEV), :, last]  # [B, H]
    assert dead_sel.any()
    assert torch.count_nonzero(out.view(B, H, hd)[dead_sel]) == 0
    assert torch.count_nonzero(dq[torch.arange(B, device=DEV), last][dead_sel]) == 0


# ======================================================== c. LayerNorm and the GEMM epilogues
@pytest.mark.parametrize('M,N', [(777, 48), (1000, 64)])
@pytest.mark.parametrize('p', [0.1, 0.5])
def test_add_layernorm_against_float64(M, N, p):
    key, site = KEYS[0], 17
    a, b = rnd(M, N, seed=1), rnd(M, N, seed=2)
    g, be = rnd(N, seed=3), rnd(N, seed=4)
    dy = rnd(M, N, seed=5)
    idx = dr.rows(M, N)
    m, mw = mult_t(key, site, p, idx), mult_t(key, site + 1, p, idx)

    def ref(mask):
        a64, b64 = a.double().requires_grad_(True), b.double().requires_grad_(True)
        g64, be64 = g.double().requires_grad_(True), be.double().requires_grad_(True)
        h = a64 * mask.double() + b64
        y = F.layer_norm(h, (N,), g64, be64, 1e-5)
        y.backward(dy.double())
        return h.detach(), y.detach(), b64.grad, a64.grad, g64.grad, be64.grad

    (h_r, y_r, dh_r, da_r, dg_r, db_r), (h_w, y_w, dh_w, da_w, dg_w, db_w) = ref(m), ref(mw)
    a2 = a.clone()
    y, mean, rstd = ops.add_layernorm_fwd(a2, b, g, be, 1e-5, p, key_t(*key), site)
    # test_layernorm_fwd_bwd's bounds
    check_close('h', a2, h_r, h_w, atol=1e-8 * inv(p), rtol=1e-5)  # allclose's default atol there
    check_close('y', y, y_r, y_w, atol=1e-5 * inv(p), rtol=1e-5)
    dg, db = torch.zeros(N, device=DEV), torch.zeros(N, device=DEV)
    da = torch.empty_like(dy)
    dh = ops.layernorm_bwd(a2, dy.clone(), g, mean, rstd, dg, db, da=da, p=p, key=key_t(*key), site=site)
    assert torch.equal(da, dh * m)  # the sublayer's dropout backward: the mirror's mask, bit for bit
    check_close('da', da, da_r, da_w, atol=1e-4 * inv(p), rtol=1e-5)
    check_close('dh', dh, dh_r, dh_w, atol=1e-4 * inv(p), rtol=1e-5)
    check_close('dgamma', dg, dg_r, dg_w, atol=1e-3 * inv(p), rtol=1e-5)
    # dbeta = colsum(dy): no mask enters it (db_w is db_r), so there is no wrong mask to tell
    assert excess(db, db_r, 1e-5) <= 1e-3 * inv(p)


def _linear_ref(x, W, b, relu, ma, aux, aux_mod, mb):
    y = x.double() @ W.double().t() + b.double()
    if relu:
        y = torch.relu(y)
    if ma is not None:
        y = y * ma.double()
    if aux is not None:
        y = y + aux.double()[torch.arange(x.shape[0], device=DEV) % aux_mod]
    return y * mb.double() if mb is not None else y


# M = 300: the generic GEMM; 32768: the streaming row GEMM at its smallest size
@pytest.mark.parametrize('M', [300, 32768])
@pytest.mark.parametrize('N,K,kind', [(64, 40, 'proj'), (64, 64, 'proj'), (256, 64, 'relu')])
def test_linear_epilogue_against_float64(M, N, K, kind):
    p, key, Lm = 0.15, KEYS[1], 50
    x, W, b = rnd(M, K, seed=1), rnd(N, K, seed=2) * 0.2, rnd(N, seed=3)
    pos = rnd(Lm, N, seed=4)
    idx = dr.rows(M, N)
    kd = key_t(*key)
    if kind == 'proj':  # the sequence projection: drop_b(drop_a(x W^T + b) + pos[m % L])
        got = ops.linear_fwd(x, W, b, aux=pos, aux_mod=Lm, drop_p=p, drop_key=kd, site_a=0, site_b=1)
        ref = _linear_ref(x, W, b, False, mult_t(key, 0, p, idx), pos, Lm, mult_t(key, 1, p, idx))
        # a wrong mask at either site
        wrongs = [_linear_ref(x, W, b, False, mult_t(key, 1, p, idx), pos, Lm, mult_t(key, 1, p, idx)),
                  _linear_ref(x, W, b, False, mult_t(key, 0, p, idx), pos, Lm, mult_t(key, 2, p, idx))]
    else:  # linear1: drop_a(relu(x W^T + b))
        got = ops.linear_fwd(x, W, b, relu=True, drop_p=p, drop_key=kd, site_a=18)
        ref = _linear_ref(x, W, b, True, mult_t(key, 18, p, idx), None, 0, None)
        wrongs = [_linear_ref(x, W, b, True, mult_t(key, 19, p, idx), None, 0, None)]
    for w in wrongs:  # test_projection_specialised_k_remainder's bounds
        check_close(kind, got, ref, w, atol=1e-4 * inv(p), rtol=1e-5)


@pytest.mark.parametrize('unfused', ['0', '1'])
@pytest.mark.parametrize('K', [64, 256])
def test_linear_add_layernorm_against_float64(K, unfused, monkeypatch):
    monkeypatch.setenv('RSYS_UNFUSED_LN', unfused)
    M, N, p, key, site = 32768, 64, 0.15, KEYS[2], 19
    x, W, b = rnd(M, K, seed=1), rnd(N, K, seed=2) * 0.2, rnd(N, seed=3)
    res, g, be = rnd(M, N, seed=4), 1 + 0.1 * rnd(N, seed=5), 0.1 * rnd(N, seed=6)
    idx = dr.rows(M, N)
    h, y, mu, rs = ops.linear_add_layernorm(x, W, b, res, g, be, 1e-5, p, key_t(*key), site)

    def ref(mask):
        hr = (x.double() @ W.double().t() + b.double()) * mask.double() + res.double()
        return hr, F.layer_norm(hr, (N,), g.double(), be.double(), 1e-5)

    (h_r, y_r), (h_w, y_w) = ref(mult_t(key, site, p, idx)), ref(mult_t(key, site + 1, p, idx))
    # test_linear_add_layernorm_fused's bounds
    check_close('h', h, h_r, h_w, atol=1e-4 * inv(p), rtol=1e-5)
    check_close('y', y, y_r, y_w, atol=1e-4 * inv(p), rtol=1e-5)
    # a row's mean is no further off than its elements: h's atol (its dropout-free test bounds the mean against the
    # unfused kernel only)
    check_close('mean', mu, h_r.mean(1), h_w.mean(1), atol=1e-4 * inv(p))


# ==================================================== d. the fused encoder kernels, bf16 mode
# 16: one row group; 272: 17 row groups, a ragged split over the waves; 32768: the token-sized routes
FUSED_M = [16, 272, 32768]


class _RoundGrad(torch.autograd.Function):
    """Identity whose gradient is rounded to bf16: a gradient that a backward kernel feeds to an MFMA
    (or stores as bf16) enters the reference's products rounded the same way."""

    @staticmethod
    def forward(ctx, x):
        return x.view_as(x)

    @staticmethod
    def backward(ctx, g):
        return r16(g.float()).double()


def _rr(t):
    """t rounded to bf16 in the forward and the identity in the backward: an MFMA operand."""
    return t + (r16(t.detach().float()).double() - t.detach())


def check_abs(name, got, ref, wrong, bound):
    err, werr = (got.double() - ref.double()).abs().max().item(), (got.double() - wrong.double()).abs().max().item()
    print(f'{name}: err {err:.3e} (bound {bound:.3e}); wrong mask {werr:.3e}')
    assert err < bound, (name, err, bound)
    assert werr >= 10 * bound, (name, 'does not tell a wrong mask', werr, bound)


class _Stages:
    """close() of test_gpu_fwd_chain's stage-by-stage helpers: keeps each masked stage's excess over
    rtol |ref| and its atol. enforce false (a reference under wrong masks): every stage passes on, and
    the caller asserts how far off each one was."""

    def __init__(self, enforce):
        self.enforce, self.seen = enforce, {}

    def __call__(self, name, a, b, atol, rtol):
        e = excess(a, b, rtol)
        self.seen[name] = (e, atol)
        print(f'{name}: err {e:.3e} (bound {atol:.3e})' + ('' if self.enforce else ' under wrong masks'))
        return e <= atol or not self.enforce

    def assert_missed(self, *names):
        for n in names:
            e, atol = self.seen[n]
            assert e >= 10 * atol, (n, 'does not tell a wrong mask', e, atol)


def _layer_masks(key, site, p, M, shift=0):
    """dropout1 [M, 64], the FFN's inner dropout [M, 256], dropout2 [M, 64] of the layer at `site`."""
    return (mult_t(key, site + 1 + shift, p, dr.rows(M, 64)), mult_t(key, site + 2 + shift, p, dr.rows(M, 256)),
            mult_t(key, site + 3 + shift, p, dr.rows(M, 64)))


@pytest.mark.parametrize('with_qkv', [True, False])
@pytest.mark.parametrize('M', FUSED_M)
def test_layer_tail_forward_stage_by_stage(M, with_qkv, bf16_mode):
    """rs_layer_tail_fwd_bf16 (sites + 1, + 2, + 3) with test_gpu_fwd_chain's stage-by-stage torch
    reference under the mirror's masks, its bounds times 1/(1-p)."""
    import test_gpu_fwd_chain as fc
    p, key, site = 0.15, KEYS[1], 16
    att, resid, w = rnd(M, 64, seed=1), rnd(M, 64, seed=2), fc._weights()
    got = fc._tail(att, resid, w, p, key_t(*key), site, qkv=with_qkv)
    assert (got[9] is not None) == with_qkv
    fc._check_tail_against_torch(att, resid, w, got, p, _layer_masks(key, site, p, M), _Stages(True))
    wrong = _Stages(False)
    fc._check_tail_against_torch(att, resid, w, got, p, _layer_masks(key, site, p, M, 1), wrong)
    wrong.assert_missed('h1', 'f1', 'h2')


@pytest.mark.parametrize('M', FUSED_M)
def test_ffn_forward_stage_by_stage(M, bf16_mode):
    """rs_ffn_fwd_bf16 (sites 18, 19) the same way."""
    import test_gpu_fwd_chain as fc
    p, key = 0.15, KEYS[2]
    x, w = rnd(M, 64, seed=7), fc._weights()
    out = ops.ffn_fwd_bf16(x, w['W1'], w['b1'], w['W2'], w['b2'], w['g2'], w['be2'], 1e-5, p, key_t(*key), 18, 19)
    fc._check_ffn_against_torch(x, w, out, p, _layer_masks(key, 16, p, M)[1:], _Stages(True))
    wrong = _Stages(False)
    fc._check_ffn_against_torch(x, w, out, p, _layer_masks(key, 16, p, M, 1)[1:], wrong)
    wrong.assert_missed('f1', 'h2')


def _post_attn_ref(h1, x1_in, h2_fwd, f1_fwd, w, masks, dy2):
    """x2 = LN2(x1 + drop2(linear2(drop(relu(linear1(x1)))))), x1 = LN1(h1), in float64 with the bf16
    roundings of csrc/ffn.hip (x1, W1, f1, W2 as operands; the gradients dff and dPre1 where they enter
    a product), backward by autograd from dy2. x1 takes the values of the fp32 rows the kernels are
    given (x1_in; a float64 LayerNorm would round to another bf16 here and there, and such a row's
    pre-activations move by 1e-3). Two things are the forward kernel's own, as in the forward's
    stage-by-stage reference (which checks them): norm2's backward runs on its h2 (h2_fwd),
    so that a bf16 flip of one f1 element in the forward is no business of the backward's, and the
    ReLU decision of a pre-activation within fp32 summation error of 0 (|pre1| < 1e-5; a handful of
    8.4 M elements at M = 32768, each worth a whole gradient entry) is read from its f1 (f1_fwd). The
    masks are the mirror's everywhere. -> the gradients the backward kernels produce."""
    z1, z2, z3 = (m.double() for m in masks)
    P = {k: v.double().clone().requires_grad_(True) for k, v in w.items()}
    h = h1.double().clone().requires_grad_(True)
    x1 = F.layer_norm(h, (64,), P['g1'], P['be1'], 1e-5)
    x1 = x1 + (x1_in.double() - x1.detach())
    pre1 = _RoundGrad.apply(_rr(x1) @ _rr(P['W1']).t() + P['b1'])
    pos = torch.where(pre1.detach().abs() < 1e-5, f1_fwd > 0, pre1.detach() > 0)
    f1 = _rr(pre1 * pos * z2)
    ff = _RoundGrad.apply(f1 @ _rr(P['W2']).t()) + P['b2']
    ff.retain_grad()
    h2 = x1 + ff * z3
    h2 = h2 + (h2_fwd.double() - h2.detach())
    F.layer_norm(h2, (64,), P['g2'], P['be2'], 1e-5).backward(dy2.double())
    out = {k: P[k].grad for k in ('W1', 'b1', 'W2', 'b2', 'g1', 'be1', 'g2', 'be2')}
    out.update(dh1=h.grad, dsa=h.grad * z1, dff=ff.grad)
    return out


@pytest.mark.parametrize('M', FUSED_M)
def test_ffn_backward_against_float64(M, bf16_mode):
    """The layer's backward after the attention: rs_ffn_bwd_ln2_bf16 (norm2, the FFN, norm1; dropout
    sites + 1 and + 3, the inner site through the forward's bits) and the weight gradients by
    rs_ffn_wgrad_bf16 (from the stored x1) and rs_ffn_wgrad_ln_bf16 (x1 rebuilt from h1). Bounds:
    test_fused_ffn_ln2_backward's (dff 1e-5, dh1 2e-3 max / 1e-5 mean, dsa 3e-3, the LayerNorm
    gradients 2e-3, all of the reference's maximum) and test_fused_ffn_matches_unfused's for the
    weight gradients (2e-3; db1, a sum of bf16 values, 1e-2)."""
    import test_gpu_fwd_chain as fc
    p, key, site = 0.15, KEYS[0], 24
    kd = key_t(*key)
    w = fc._weights()
    h1 = rnd(M, 64, seed=10) * 2 + 0.3
    dy2 = rnd(M, 64, seed=8)
    x1 = F.layer_norm(h1, (64,), w['g1'], w['be1'], 1e-5)
    mu1 = h1.mean(1)
    rs1 = 1.0 / torch.sqrt(h1.var(1, unbiased=False) + 1e-5)
    h2, _, mu2, rs2, fmask = ops.ffn_fwd_bf16(x1, w['W1'], w['b1'], w['W2'], w['b2'], w['g2'], w['be2'], 1e-5, p, kd,
                                              site + 2, site + 3)
    ln0 = [rnd(64, seed=20 + i) for i in range(4)]  # dgamma2, dbeta2, dgamma1, dbeta1: accumulated into
    ln = [t.clone() for t in ln0]
    dh1, dsa, dff = ops.ffn_bwd_ln2_bf16(x1, w['W1'], w['b1'], w['W2'], fmask, dy2, h2, w['g2'], mu2, rs2, ln[0], ln[1],
                                         h1, w['g1'], mu1, rs1, ln[2], ln[3], p, kd, site + 1, site + 3)
    wg0 = [rnd(*w[n].shape, seed=30 + i) for i, n in enumerate(('W1', 'b1', 'W2', 'b2'))]
    wg, wg_ln = [t.clone() for t in wg0], [t.clone() for t in wg0]
    ops.ffn_wgrad_bf16(x1, w['W1'], w['b1'], w['W2'], fmask, dff, p, *wg)
    ops.ffn_wgrad_ln_bf16(h1, mu1, rs1, w['g1'], w['be1'], w['W1'], w['b1'], w['W2'], fmask, dff, p, *wg_ln)
    torch.cuda.synchronize()
    zero = torch.zeros_like(x1)
    f1 = ops.ffn_bwd_bf16(x1, w['W1'], w['b1'], w['W2'], fmask, zero, zero, p)[1]
    r = _post_attn_ref(h1, x1, h2, f1, w, _layer_masks(key, site, p, M), dy2)
    x = _post_attn_ref(h1, x1, h2, f1, w, _layer_masks(key, site, p, M, 1), dy2)
    check_rel('dff', dff, r['dff'], x['dff'], 1e-5)
    check_rel('dh1', dh1, r['dh1'], x['dh1'], 2e-3, 1e-5)
    check_abs('dsa', dsa, r['dsa'], x['dsa'], 3e-3 * r['dh1'].abs().max().item())
    assert torch.equal(dsa, dh1 * _layer_masks(key, site, p, M)[0])  # dropout1's backward: the mirror's mask, bit for bit
    for got, g0, n in zip(ln, ln0, ('g2', 'be2', 'g1', 'be1')):
        bound = 2e-3 * max(1.0, r[n].abs().max().item())
        if n in ('g2', 'be2'):
            # dgamma2 = colsum(dy2 * xhat(h2)) and dbeta2 = colsum(dy2) with h2 the forward kernel's in both
            # references (_post_attn_ref): no mask enters them, x[n] is r[n], there is no wrong mask to tell
            err = (got - g0 - r[n]).abs().max().item()
            print(f'd{n}: err {err:.3e} (bound {bound:.3e})')
            assert err < bound, (n, err, bound)
        else:
            check_abs('d' + n, got - g0, r[n], x[n], bound)
    for name, grads in (('stored x1', wg), ('rebuilt x1', wg_ln)):
        for got, g0, n in zip(grads, wg0, ('W1', 'b1', 'W2', 'b2')):
            check_abs(f'd{n} ({name})', got - g0, r[n], x[n], (1e-2 if n == 'b1' else 2e-3) * r[n].abs().max().item())


@pytest.mark.parametrize('M', FUSED_M)
def test_outproj_bwd_against_float64(M, bf16_mode):
    """rs_outproj_bwd_bf16: y = dh * mask(site), datt = y Wo, dWo += y^T att, dbo += colsum(y), against
    float64 products of the bf16-rounded operands. Exact products, so only the fp32 summation order
    differs: test_seq_input_bwd_fused's 2e-5 of the maximum for the 64-term datt and its 2e-3 for the
    bias; 2e-6 of the largest sum of |terms| for dWo (test_tower_wgrad_grouped_vs_float64's fp32 figure
    for the same error)."""
    p, key, site = 0.15, KEYS[1], 17
    dh, att, Wo = rnd(M, 64, seed=1), rnd(M, 64, seed=2), rnd(64, 64, seed=3) * 0.2
    dW0, db0 = rnd(64, 64, seed=4), rnd(64, seed=5)
    dW, db = dW0.clone(), db0.clone()
    datt = ops.outproj_bwd_fused(dh, att, Wo, p, key_t(*key), site, dW, db)
    torch.cuda.synchronize()

    def ref(s):
        y = dh * mult_t(key, s, p, dr.rows(M, 64))
        yb, ab = r16(y).double(), r16(att).double()
        return yb @ r16(Wo).double(), yb.t() @ ab, y.double().sum(0), (yb.abs().t() @ ab.abs()).max().item()

    (dx_r, dW_r, db_r, terms), (dx_w, dW_w, db_w, _) = ref(site), ref(site + 1)
    check_abs('datt', datt, dx_r, dx_w, 2e-5 * dx_r.abs().max().item())
    check_abs('dWo', dW - dW0, dW_r, dW_w, 2e-6 * terms + 2.0 ** -22 * dW0.abs().max().item())
    check_abs('dbo', db - db0, db_r, db_w, 2e-3 * max(1.0, M / 40960))


@pytest.mark.parametrize('B,L', [(1, 16), (17, 16), (2048, 16)])
def test_seq_input_bwd_against_float64(B, L, bf16_mode):
    """rs_seq_input_bwd_bf16 + rs_seq_input_pos_grad (sites 0, 1) on test_gpu_linear_bwd's inputs under
    the mirror's masks, test_seq_input_bwd_fused's references and bounds (dW: as dWo above)."""
    import test_gpu_linear_bwd as lb
    d, dcat, p, key, M = 64, 40, 0.15, (4321, 7), B * L
    idx = dr.rows(M, d)

    def ref(sa, sb):
        t = lb._inputs(B, L, d, dcat, p, masks=(mult_t(key, sa, p, idx), mult_t(key, sb, p, idx)))
        yb, cb = r16(t['y']).double(), r16(t['cat']).double()
        return t, (yb @ r16(t['W']).double(), yb.t() @ cb, t['y'].double().sum(0),
                   t['v'].view(B, L * d).double().sum(0).view(L, d), (yb.abs().t() @ cb.abs()).max().item())

    (t, (dc_r, dW_r, db_r, pos_r, terms)), (_, (dc_w, dW_w, db_w, pos_w, _)) = ref(0, 1), ref(1, 2)
    assert tuple(t['key'].tolist()) == key
    dW, db, pos = t['dW0'].clone(), t['db0'].clone(), t['pos0'].clone()
    out = ops.seq_input_bwd_fused(t['dx'], t['cat'], t['W'], L, p, t['key'], 0, 1, dW, db, pos)
    torch.cuda.synchronize()
    check_abs('dcat', out, dc_r, dc_w, 2e-5 * dc_r.abs().max().item())
    check_abs('dW', dW - t['dW0'], dW_r, dW_w, 2e-6 * terms + 2.0 ** -22 * t['dW0'].abs().max().item())
    check_abs('db', db - t['db0'], db_r, db_w, 2e-3 * max(1.0, M / 40960))
    check_close('dpos', pos[:L] - t['pos0'][:L], pos_r, pos_w, atol=1e-4 * max(1.0, B / 1000) * inv(p), rtol=1e-5)
    assert torch.equal(pos[L:], t['pos0'][L:])


def test_seq_head_against_float64(bf16_mode):
    """rs_seq_head_fwd_bf16 (sites 0, 1) at 656 x 50 = 32,800 tokens, the smallest count it takes
    (32,768 and a multiple of L): x0 against test_gpu_seq_head's float64 reference under the mirror's
    masks, its 2e-5 of the reference's maximum; qkv0 from the kernel's own x0, as the tail's qkv."""
    import test_gpu_seq_head as sh
    feats, w, ids, segs, cat = sh._case('c2', 656)
    B, p = 656, 0.15
    M = B * sh.L
    key = tuple(w['key'].tolist())
    x0, cat_h, qkv = sh._head(segs, M, w, p)
    torch.cuda.synchronize()
    assert torch.equal(cat_h, cat)
    idx = dr.rows(M, 64)
    m = {s: mult_t(key, s, p, idx) for s in (0, 1, 2)}
    ref = sh._x0_ref(cat, w, B, (m[0], m[1]))
    for wrong in (sh._x0_ref(cat, w, B, (m[1], m[1])), sh._x0_ref(cat, w, B, (m[0], m[2]))):
        check_abs('x0', x0, ref, wrong, 2e-5 * ref.abs().max().item())
    qr = r16(x0) @ r16(w['Win']).t() + w['bin']
    assert torch.allclose(qkv.float(), qr, atol=1e-4, rtol=2.0 ** -7)


# ================================================================================ e. the towers
@pytest.mark.parametrize('G', [1, 3])
def test_batchnorm_dropout_against_float64(G):
    C, Bg, p, key, site = 172, 300, 0.3, KEYS[0], 257
    bn = torch.nn.BatchNorm1d(C).to(DEV)
    with torch.no_grad():
        bn.weight.copy_(1 + 0.1 * rnd(C, seed=1))
        bn.bias.copy_(0.1 * rnd(C, seed=2))
    x = rnd(G * Bg, C, seed=3) * 3 + 1
    dy = rnd(G * Bg, C, seed=4)
    idx = dr.rows(G * Bg, C)  # (g * Bg + row) * C + col

    def ref(mask):
        x64 = x.double().requires_grad_(True)
        w64, b64 = bn.weight.detach().double().requires_grad_(True), bn.bias.detach().double().requires_grad_(True)
        ys = [F.batch_norm(x64[g * Bg:(g + 1) * Bg], None, None, w64, b64, training=True, eps=bn.eps) for g in range(G)]
        y = torch.relu(torch.cat(ys)) * mask.double()
        y.backward(dy.double())
        return y.detach(), x64.grad, w64.grad, b64.grad

    (y_r, dx_r, dw_r, db_r), (y_w, dx_w, dw_w, db_w) = ref(mult_t(key, site, p, idx)), ref(mult_t(key, site + 1, p, idx))
    y, mean, rstd = ops.batchnorm_fwd(x, bn, G, True, training=True, drop_p=p, drop_key=key_t(*key), drop_site=site)
    dw, db = torch.zeros(C, device=DEV), torch.zeros(C, device=DEV)
    dx = ops.batchnorm_bwd(x, y, dy, bn.weight, mean, rstd, dw, db, G, True, drop_p=p)
    # test_batchnorm_train_fwd_bwd's bounds
    check_close('y', y, y_r, y_w, atol=1e-5 * inv(p), rtol=1e-5)
    check_close('dx', dx, dx_r, dx_w, atol=2e-5 * inv(p), rtol=1e-5)
    check_close('dw', dw, dw_r, dw_w, atol=1e-3 * inv(p), rtol=1e-5)
    check_close('db', db, db_r, db_w, atol=1e-3 * inv(p), rtol=1e-5)


def _rel(a, b):
    return ((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-30)).item()


def _tower_ref64(m, x, G, dout, key, p, site_shift=0):
    """feature_bn -> [Linear -> BatchNorm1d per group -> ReLU -> mask(256 + j)]* -> Linear -> L2
    normalize in float64 (bf16 mode: the GEMM operands rounded to bf16), backward by autograd."""
    bf = precision.compute_dtype() == 'bf16'
    rr = (lambda t: t + (r16(t.detach().float()).double() - t.detach())) if bf else (lambda t: t)  # straight through
    P = {n: q.detach().double().requires_grad_(True) for n, q in m.named_parameters()}
    Bg = x.shape[0] // G
    x64 = x.double().requires_grad_(True)

    def bn(h, name, mod):
        return torch.cat([F.batch_norm(h[g * Bg:(g + 1) * Bg], None, None, P[name + '.weight'], P[name + '.bias'],
                                       training=True, eps=mod.eps) for g in range(G)])
    h = bn(x64, 'feature_bn', m.feature_bn)
    seq = m.mlp.mlp
    n_hidden = (len(seq) - 1) // 4
    for j in range(n_hidden):
        h = rr(h) @ rr(P[f'mlp.mlp.{4 * j}.weight']).t() + P[f'mlp.mlp.{4 * j}.bias']
        h = torch.relu(bn(h, f'mlp.mlp.{4 * j + 1}', seq[4 * j + 1]))
        h = h * mult_t(key, 256 + j + site_shift, p, dr.rows(x.shape[0], h.shape[1])).double()
    out = rr(h) @ rr(P[f'mlp.mlp.{4 * n_hidden}.weight']).t() + P[f'mlp.mlp.{4 * n_hidden}.bias']
    out = F.normalize(out, p=2, dim=1)  # Tower.py:41
    out.backward(dout.double())
    return out.detach(), x64.grad, {n: q.grad for n, q in P.items()}


@pytest.mark.parametrize('mode', ['fp32', 'bf16'])
@pytest.mark.parametrize('G', [1, 3])
def test_tower_chain_against_float64(G, mode):
    """The fused tower (csrc/tower.hip, functions.TowerChainFn) with dropout on. fp32: the bounds of
    test_tower_chain_fp32_matches_per_op (2e-5 forward; 5e-3 on the gradients, where a ReLU decision
    at |BN output| ~ 1e-7 may differ from float64's). bf16: those of
    test_tower_chain_bf16_close_to_fp32 with the hidden BatchNorm outputs kept away from 0 (its
    no_flips setting: weight 0.5, bias 5), so that no ReLU decision can differ (1e-2 forward, 2e-2
    gradients, 5e-2 for the second Linear's weight). ReLU never clips in that bf16 case: it checks the
    bf16 tower's masks, scale and group layout; ReLU followed by the mask is covered by the fp32 case,
    and in bf16 mode by the item and user towers of test_c2_step_with_dropout_matches_oracle_bf16."""
    import test_gpu_tower as tt
    Bg, C0, hidden, out, p = 300, 172, [256, 128], 128, 0.3
    gen = torch.Generator(device=DEV).manual_seed(1)
    x = torch.randn(G * Bg, C0, device=DEV, generator=gen) * 2 + 0.5
    dout = torch.randn(G * Bg, out, device=DEV, generator=gen)
    m = tt._make(C0, hidden, out, p)
    if mode == 'bf16':
        with torch.no_grad():
            for j in range(len(hidden)):
                m.mlp.mlp[4 * j + 1].weight.fill_(0.5)
                m.mlp.mlp[4 * j + 1].bias.fill_(5.0)
    precision.set_compute_dtype(mode)
    m.mlp.rng_state.copy_(torch.tensor([4242, 0]))  # the module's own seed depends on the process's history
    try:
        key = tuple(m.mlp.rng_state.tolist())
        y, dx, grads, _ = tt._run(m, x, G, dout, fused=True)
        assert tuple(m.mlp.rng_state.tolist()) == (key[0], key[1] + 1)
        y_r, dx_r, g_r = _tower_ref64(m, x, G, dout, key, p)
        y_w, dx_w, g_w = _tower_ref64(m, x, G, dout, key, p, site_shift=1)
    finally:
        precision.set_compute_dtype('fp32')
    fwd, bwd = (2e-5, 5e-3) if mode == 'fp32' else (1e-2, 2e-2)
    checks = [('y', y, y_r, y_w, fwd), ('dx', dx, dx_r, dx_w, bwd)]
    for n in ('mlp.mlp.0.weight', 'mlp.mlp.4.weight', 'mlp.mlp.8.weight', 'feature_bn.weight', 'mlp.mlp.1.weight'):
        tol = 5e-2 if (mode == 'bf16' and n == 'mlp.mlp.4.weight') else bwd
        checks.append((n, grads[n], g_r[n], g_w[n], tol))
    for name, got, ref, wrong, tol in checks:
        e, w = _rel(got, ref), _rel(got, wrong)
        print(f'{name}: rel {e:.3e} (bound {tol:.1e}); wrong mask {w:.3e}')
        assert e < tol, (name, e)
        assert w >= 10 * tol, (name, 'does not tell a wrong mask', w)


# ============================================================================ f. the whole step
def _c2_step_setup(B, L, seed=5, lr=1e-3):
    from oracle.twotower_oracle import OracleTrainer, model_state_shapes
    from recommendsystemproject_amd import synth
    from recommendsystemproject_amd.project.models.TwoTower.GenericTower import GenericTower
    from recommendsystemproject_amd.project.models.TwoTower.TwoTowerModel import TwoTowerModel
    cfg = yaml.safe_load(open(os.path.join(ROOT, 'configs', 'c2.yaml')))  # dropout as configured
    ut = cfg['two_tower']['user_tower']
    assert ut['dropout'] == 0.3 and ut['transformer_parameters']['dropout'] == 0.15
    assert cfg['two_tower']['item_tower']['dropout'] == 0.1
    ut['transformer_parameters']['max_seq_len'] = L
    maps = {'user': synth.tower_layout(ut), 'item': synth.tower_layout(cfg['two_tower']['item_tower'])}
    shapes = {k: s for k, s, _ in model_state_shapes(cfg)}
    state = synth.make_state(shapes, seed=seed)
    model = TwoTowerModel(GenericTower(cfg, 'user_tower'), GenericTower(cfg, 'item_tower'), maps['user'], maps['item'])
    model.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in state.items()})
    model = model.to(DEV).train()
    for name, s in dr.STEP_SEEDS.items():  # a module's own seed depends on what the process built before it
        model.get_submodule(name).rng_state.copy_(torch.tensor([s, 0]))
    tp = ut['transformer_parameters']
    pruned = functions.prune_last_layer() and bool(
        ops.attn_plan(B, L, ut['embedding_dim'], tp['n_head'], 0.0, precision.gemm_flags(), strict=False).rows_ok)
    masks = dr.StepMasks(tp['n_layers'], pruned)
    ref = OracleTrainer(cfg, state, lr=lr, dropout=None, masks=masks)
    return cfg, maps, model, ref, masks


STEP_SITES = {('user_tower.seq_encoder', s) for s in (0, 1, 16, 17, 18, 19, 24, 25, 26, 27)} | \
    {('user_tower.mlp', 256), ('user_tower.mlp', 257), ('item_tower.mlp', 256), ('item_tower.mlp', 257)}


@pytest.mark.parametrize('B,L', [(37, 7), (128, 50)])
def test_c2_step_with_dropout_matches_oracle_fp32(B, L):
    """test_c2_shape_step_matches_oracle with dropout as configs/c2.yaml has it (0.15 in the encoder,
    0.3 and 0.1 in the MLPs): two steps, the same 1e-4 bounds on the loss and the four parameters."""
    from recommendsystemproject_amd import synth
    from recommendsystemproject_amd.optim import Adam
    from recommendsystemproject_amd.project.utils.training_utils import train_step
    cfg, maps, model, ref, masks = _c2_step_setup(B, L)
    opt = Adam(model.parameters(), lr=1e-3)
    for step in range(2):
        b = synth.make_batch(cfg, B, seed=50 + step, edge_cases=True)
        masks.read(model)
        before = dict(masks.keys)
        got = train_step(model, synth.batch_to_torch(b, DEV), opt, 1.0, 0.15).item()
        want = float(ref.step(synth.batch_to_torch(b), maps, temperature=0.15))
        print(f'step {step}: loss {got:.6f} oracle {want:.6f}')
        assert abs(got - want) < 1e-4, (step, got, want)
        masks.read(model)
        for mod, _ in STEP_SITES:  # one forward, one key
            assert masks.keys[mod] == (before[mod][0], before[mod][1] + 1)
    assert set(masks.calls) == STEP_SITES
    sd = model.state_dict()
    for k in dr.STEP_PARAMS:
        err = (sd[k].cpu() - ref.S[k].detach()).abs().max().item()
        print(f'{k}: {err:.3e}')
        assert err < 1e-4, (k, err)
    assert masks.pruned  # the last layer ran on the selected rows: StepMasks' row-b indexing was used


def test_c2_step_with_dropout_matches_oracle_bf16():
    """One bf16-mode step at 672 x 50 = 33,600 tokens (the fused sequence head, layer tail and
    streaming routes) against the fp32 oracle under the same masks: the loss within
    test_bf16_training_step_close_to_fp32's 1e-2 relative, the flat gradient's cosine above 0.99."""
    from recommendsystemproject_amd import synth
    from recommendsystemproject_amd.flat import ensure_flat, grad_of
    from recommendsystemproject_amd.project.utils.training_utils import extract_item_id
    B, L = 672, 50
    precision.set_compute_dtype('bf16')
    try:
        cfg, maps, model, ref, masks = _c2_step_setup(B, L, seed=3)
        b = synth.make_batch(cfg, B, seed=7, edge_cases=True)
        tb = synth.batch_to_torch(b, DEV)
        f = ensure_flat(model)
        f.zero_grad()
        masks.read(model)
        enc = model.user_tower.seq_encoder
        feats = functions.seq_feature_segments(enc.feature_embedder, tb['user_tower']['sequence'], B, L)
        plan = functions.plan_encoder(enc, feats[0], feats[1], B, L)
        print('encoder plan', plan)
        assert plan.qkv_bf16 and plan.head == 'fused' and plan.layers[0].post == 'tail_qkv' and plan.layers[1].rows
        U, I, H = model(tb)
        loss = model.compute_loss(U, I, item_ids=extract_item_id(tb['item_tower']), temperature=0.15)
        loss.backward()
        torch.cuda.synchronize()
        got = loss.item()
        grads = {n: grad_of(q).detach().cpu().clone() for n, q in model.named_parameters()}
    finally:
        precision.set_compute_dtype('fp32')
    for q in ref.params():
        q.grad = None
    _, _, _, want = ref.forward_loss(synth.batch_to_torch(b), maps, temperature=0.15)
    want.backward()
    want = want.item()
    assert set(masks.calls) == STEP_SITES
    g = torch.cat([grads[k].reshape(-1) for k in ref.keys])
    gr = torch.cat([ref.S[k].grad.reshape(-1) for k in ref.keys])
    cos = F.cosine_similarity(g.double(), gr.double(), dim=0).item()
    print(f'loss {got:.6f} oracle {want:.6f}; gradient cosine {cos:.6f}')
    assert abs(got - want) < 1e-2 * abs(want), (got, want)
    assert cos > 0.99, cos
