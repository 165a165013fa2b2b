"""The attention planner (csrc/attention.hip, rs_attn_plan) on the CPU: the route, tile count,
bf16-storage answer and saved keep-bit words of rs_attn_fwd / rs_attn_bwd by shape, flags and the
RSYS_ATTN_VALU switch. The planner launches nothing and follows no pointer. The expectations are the
entry points' dispatch as it stood before it had a planner, evaluated by hand at these shapes: the
wave-per-head MFMA kernels at head_dim 16, L <= 64 and B*H*L*L < 2^32, the long bf16 kernels up to
L = 256 in bf16 mode, else the VALU kernels within their 64 KB of LDS ((2 L hd + L) 4 bytes forward,
(4 L hd + 3 L) 4 backward) -- and bf16 qkv storage on the two bf16 MFMA routes only."""
import pytest

from recommendsystemproject_amd import _hip, ops, precision

BF, QB = _hip.RS_GEMM_BF16, _hip.RS_ATTN_QKV_BF16


def _plan(monkeypatch, env, *args, **kw):
    monkeypatch.delenv('RSYS_ATTN_VALU', raising=False)
    if env is not None:
        monkeypatch.setenv('RSYS_ATTN_VALU', env)  # C getenv sees it
    return ops.attn_plan(*args, **kw)


# flags, RSYS_ATTN_VALU, B, L, d, H, p, bwd values -> route, then the fields named
PLANS = [
    (0, None, 6, 50, 64, 4, 0.0, (0, 1), 'wave_f32', dict(nt=4, zbits_words=0, qkv_bf16=0)),
    (BF, None, 6, 50, 64, 4, 0.0, (0, 1), 'wave_bf16', dict(nt=4, zbits_words=0, qkv_bf16=1)),
    (BF, None, 5, 50, 64, 4, 0.2, (0, 1), 'wave_bf16', dict(zbits_words=5 * 4 * 4 * 64)),
    (BF, None, 5, 7, 64, 4, 0.3, (0,), 'wave_bf16', dict(nt=1, zbits_words=1280)),
    (BF, None, 3, 64, 64, 4, 0.2, (0,), 'wave_bf16', dict(nt=4, zbits_words=3072)),
    (BF, None, 3, 65, 64, 4, 0.2, (0, 1), 'long_bf16', dict(nt=5, zbits_words=0, qkv_bf16=1)),
    (BF, None, 3, 256, 64, 4, 0.0, (0, 1), 'long_bf16', dict(nt=16, rows_ok=1)),
    (BF, None, 3, 257, 64, 4, 0.0, (0,), 'valu', dict(nt=0, qkv_bf16=0, rows_ok=0)),
    (0, None, 3, 65, 64, 4, 0.0, (0, 1), 'valu', dict(nt=0)),
    (0, None, 3, 244, 64, 4, 0.0, (1,), 'valu', {}),
    (0, None, 3, 245, 64, 4, 0.0, (0,), 'valu', {}),
    (0, None, 3, 496, 64, 4, 0.0, (0,), 'valu', {}),
    (BF, None, 3, 50, 64, 8, 0.2, (0,), 'valu', dict(zbits_words=0, qkv_bf16=0, rows_ok=1)),  # head_dim 8
    (BF, None, 3, 50, 128, 4, 0.0, (0,), 'valu', dict(rows_ok=1)),  # head_dim 32
    (BF, '1', 5, 50, 64, 4, 0.2, (0,), 'valu', dict(zbits_words=0, qkv_bf16=0)),
    (BF, '0', 5, 50, 64, 4, 0.2, (0,), 'wave_bf16', dict(zbits_words=5120)),  # "0" is off, as in C
    (BF, None, 262143, 64, 64, 4, 0.0, (0,), 'wave_bf16', dict(qkv_bf16=1)),
    (BF, None, 262144, 64, 64, 4, 0.0, (0,), 'valu', dict(qkv_bf16=0)),  # B*H*L*L = 2^32
    (BF | QB, None, 6, 50, 64, 4, 0.0, (0, 1), 'wave_bf16', dict(qkv_bf16=1)),
    (BF | QB, None, 3, 201, 64, 4, 0.2, (0, 1), 'long_bf16', dict(nt=13, qkv_bf16=1)),
]


@pytest.mark.parametrize('flags,env,B,L,d,H,p,bwds,route,fields', PLANS)
def test_plan(monkeypatch, flags, env, B, L, d, H, p, bwds, route, fields):
    for bwd in bwds:
        plan = _plan(monkeypatch, env, B, L, d, H, p, flags, bwd=bool(bwd))
        assert plan.route_name == route and _hip.ATTN_ROUTES[plan.route] == route
        assert {k: getattr(plan, k) for k in fields} == fields


# flags, RSYS_ATTN_VALU, B, L, d, H, bwd -> the message
ERRORS = [
    (BF, None, 3, 257, 64, 4, 1, 'exceeds LDS'),
    (0, None, 3, 245, 64, 4, 1, 'exceeds LDS'),
    (0, None, 3, 497, 64, 4, 0, 'exceeds LDS'),
    (BF | QB, None, 262144, 64, 64, 4, 0, 'bf16 qkv storage'),  # once read by a kernel as fp32
    (BF | QB, '1', 5, 50, 64, 4, 0, 'bf16 qkv storage'),
    (QB, None, 5, 50, 64, 4, 0, 'bf16 qkv storage'),
    (BF, None, 3, 50, 64, 5, 0, 'bad shape'),
    (BF, None, 3, 50, 60, 4, 0, 'head_dim'),
]


@pytest.mark.parametrize('flags,env,B,L,d,H,bwd,message', ERRORS)
def test_plan_errors(monkeypatch, flags, env, B, L, d, H, bwd, message):
    with pytest.raises(_hip.HipError, match=message):
        _plan(monkeypatch, env, B, L, d, H, 0.0, flags, bwd=bool(bwd))


def test_bad_dropout_is_an_error(monkeypatch):
    with pytest.raises(_hip.HipError, match='bad dropout'):
        _plan(monkeypatch, None, 3, 50, 64, 4, 1.0, BF)


def test_qkv_bf16_ok_asks_the_planner(monkeypatch):
    """ops.qkv_bf16_ok: its own terms (compute mode, RSYS_QKV_FP32, the streaming GEMMs' token
    counts) and the planner's answer; nothing is allocated, so the 2^32 shape is only planned."""
    for name in ('RSYS_ATTN_VALU', 'RSYS_QKV_FP32'):
        monkeypatch.delenv(name, raising=False)
    assert not ops.qkv_bf16_ok(64, 64, 4, 32768)  # fp32 mode
    precision.set_compute_dtype('bf16')
    try:
        assert ops.qkv_bf16_ok(64, 64, 4, 32768)
        assert not ops.qkv_bf16_ok(64, 64, 4, 64 * 262144)
        assert ops.qkv_bf16_ok(64, 64, 4, 64 * 262143)
        assert not ops.qkv_bf16_ok(64, 64, 4, 32760) and not ops.qkv_bf16_ok(64, 64, 4, 16384)
        monkeypatch.setenv('RSYS_ATTN_VALU', '1')
        assert not ops.qkv_bf16_ok(64, 64, 4, 32768)
        monkeypatch.setenv('RSYS_ATTN_VALU', '0')
        assert ops.qkv_bf16_ok(64, 64, 4, 32768)
        monkeypatch.delenv('RSYS_ATTN_VALU')
        monkeypatch.setenv('RSYS_QKV_FP32', '1')
        assert not ops.qkv_bf16_ok(64, 64, 4, 32768)
    finally:
        precision.set_compute_dtype('fp32')


# shapes the selected-row kernels take and the full attention kernels do not
ROWS_ONLY = [(0, 3, 200, 256, 4), (BF, 3, 200, 256, 4), (0, 3, 256, 128, 4), (BF, 3, 257, 64, 4)]


@pytest.mark.parametrize('flags,B,L,d,H', ROWS_ONLY)
def test_plan_not_strict_answers_where_the_call_would_fail(monkeypatch, flags, B, L, d, H):
    """strict=False: rows_ok and qkv_bf16 of a shape beyond the VALU kernels' LDS, without the error."""
    with pytest.raises(_hip.HipError, match='exceeds LDS'):
        _plan(monkeypatch, None, B, L, d, H, 0.0, flags, bwd=True)
    plan = _plan(monkeypatch, None, B, L, d, H, 0.0, flags, bwd=True, strict=False)
    assert (plan.route_name, plan.qkv_bf16, plan.rows_ok) == ('valu', 0, int(L <= 256))
    plan = _plan(monkeypatch, None, 5, 50, 64, 4, 0.0, QB, strict=False)  # the flag off its routes
    assert (plan.route_name, plan.qkv_bf16, plan.rows_ok) == ('wave_f32', 0, 1)
    plan = _plan(monkeypatch, None, 3, 50, 60, 4, 0.0, flags, strict=False)  # head_dim 15: refused outright
    assert (plan.route, plan.nt, plan.qkv_bf16, plan.zbits_words, plan.rows_ok) == (0, 0, 0, 0, 0)


@pytest.mark.parametrize('mode', ['fp32', 'bf16'])
@pytest.mark.parametrize('model_dim,L', [(256, 200), (128, 256)])
def test_one_layer_encoder_beyond_full_attention_is_planned(monkeypatch, mode, model_dim, L):
    """A one-layer encoder runs attn_rows_* only (its layer is the pruned last one), so head_dim 64 at
    L = 200 and head_dim 32 at L = 256 -- beyond the full attention kernels' LDS -- plan as they ran
    before the attention planner: the layer pruned, fp32 qkv, no error. 176 x L: the bf16 streaming
    kernels' token counts."""
    import torch

    from recommendsystemproject_amd import functions
    from recommendsystemproject_amd.project.models.TwoTower.SequenceEncoder import SequenceEncoder
    for name in ('RSYS_ATTN_VALU', 'RSYS_QKV_FP32', 'RSYS_FULL_LAST_LAYER'):
        monkeypatch.delenv(name, raising=False)
    B, vocab = 176, 97
    torch.manual_seed(5)
    enc = SequenceEncoder([dict(name='hist_movie_ids', vocab_size=vocab, embedding_dim=32, padding_index=0)],
                          model_dim=model_dim, dim_feedforward=256, max_seq_len=L, n_head=4, n_layers=1,
                          dropout=0.1)
    w = enc.feature_embedder.embeddings['hist_movie_ids'].weight
    x = torch.randint(0, vocab, (B, L), generator=torch.Generator().manual_seed(3))
    segs = [functions._seg(kind=_hip.RS_SEG_SPARSE, dim=32, out_col=0, vocab=vocab, idx_stride=1,
                           idx=x.data_ptr(), table=w.data_ptr(), pad_idx=0)]
    precision.set_compute_dtype(mode)
    try:
        plan = functions.plan_encoder(enc, segs, [w], B, L)
        assert not ops.qkv_bf16_ok(L, model_dim, 4, B * L)
    finally:
        precision.set_compute_dtype('fp32')
    assert [lp.rows for lp in plan.layers] == [True] and not plan.qkv_bf16 and plan.head == 'separate'
