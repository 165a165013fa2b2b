"""Thin tensor-level wrappers over the C ABI (pointers, strides, current HIP stream).

Only torch is used here for device memory (torch.empty on the caching allocator) and for the
current stream handle; all arithmetic runs in librsys_hip.so.
"""
from __future__ import annotations

import contextlib
import os
import threading

import numpy as np
import torch

from . import _hip, precision
from ._hip import call

_ZERO = {}


def P(t):
    return None if t is None else t.data_ptr()


def stream():
    return torch.cuda.current_stream().cuda_stream


class _DeferState(threading.local):
    """deferred_reduce's scope state, per host thread like the library's queue (csrc/reduce.hip
    g_defer / g_jobs are thread_local): a scope opened on one thread (the autograd device thread
    running the encoder backward) neither sees nor keeps another thread's workspaces."""

    def __init__(self):
        self.keep = []  # the workspaces of each open scope, alive until its flush is queued


_DEFER = _DeferState()


def ws(nbytes: int, device) -> torch.Tensor:
    """Workspace from the caching allocator (capture-safe)."""
    t = torch.empty(max(int(nbytes), 16), dtype=torch.uint8, device=device)
    if _DEFER.keep:
        _DEFER.keep[-1].append(t)  # a queued reduction reads it at the flush
    return t


@contextlib.contextmanager
def deferred_reduce(on=True):
    """The parameter-gradient reductions queued inside run as ONE launch at the end of the scope
    (rs_reduce_defer / rs_reduce_flush, round 5): nothing inside may read those gradients. Off
    (plain pass-through) when `on` is false, in a nested scope, or with RSYS_DEFER_REDUCE=0. The
    scope belongs to the calling host thread (library-side queue and this side's workspaces are
    thread-local): reductions issued by other threads meanwhile are not deferred."""
    if not on or _DEFER.keep or os.environ.get('RSYS_DEFER_REDUCE', '1') == '0':
        yield
        return
    _DEFER.keep.append([])
    call('rs_reduce_defer', 1)
    try:
        yield
    finally:
        call('rs_reduce_defer', 0)
        try:
            call('rs_reduce_flush', stream())
        finally:
            _DEFER.keep.pop()


def gemm(A, B, C, M, N, K, *, transA, transB, lda, ldb, ldc, alpha=1.0, beta=0.0, epi=0,
         bias=None, aux=None, ld_aux=0, aux_mod=0, split=None, rowsum=None, drop_p=0.0,
         drop_key=None, site_a=0, site_b=0):
    L = _hip.lib()
    if split is None:
        split = L.rs_gemm_auto_split(M, N, K)
    w = None
    if split > 1:
        w = ws(L.rs_gemm_ws_bytes(M, N, K, split), C.device)
    call('rs_gemm_f32', int(transA), int(transB), M, N, K, float(alpha), P(A), lda, P(B), ldb,
         float(beta), P(C), ldc, epi | precision.gemm_flags(), P(bias), P(aux), ld_aux, aux_mod,
         float(drop_p), P(drop_key),
         site_a, site_b, P(rowsum), split, P(w), stream())
    return C


def _io_flags(a, c):
    """bf16 storage of the A operand / the output C (bf16 compute mode, streaming instances)."""
    return (_hip.RS_GEMM_A_BF16 if a.dtype == torch.bfloat16 else 0) | \
        (_hip.RS_GEMM_C_BF16 if c.dtype == torch.bfloat16 else 0)


def linear_fwd(x, W, b=None, out=None, *, relu=False, aux=None, aux_mod=0, beta=0.0,
               drop_p=0.0, drop_key=None, site_a=None, site_b=None, out_dtype=torch.float32):
    """out[M,N] = drop_b(drop_a(relu(x[M,K] @ W[N,K]^T + b)) + aux[m % aux_mod]) (+ beta*out);
    dropout stages are active when drop_p > 0 and their site is given. out_dtype bf16: the
    result is stored as bf16 (only for outputs consumed as bf16 MFMA operands)."""
    M, K = x.shape
    N = W.shape[0]
    if out is None:
        out = torch.empty(M, N, device=x.device, dtype=out_dtype)
    epi = (_hip.RS_EPI_BIAS if b is not None else 0) | (_hip.RS_EPI_RELU if relu else 0) | \
        (_hip.RS_EPI_AUX_ADD if aux is not None else 0) | _io_flags(x, out)
    if drop_p > 0:
        epi |= (_hip.RS_EPI_DROP_A if site_a is not None else 0) | (_hip.RS_EPI_DROP_B if site_b is not None else 0)
    return gemm(x, W, out, M, N, K, transA=0, transB=1, lda=x.stride(0), ldb=W.stride(0),
                ldc=out.stride(0), beta=beta, epi=epi, bias=b, aux=aux,
                ld_aux=(aux.stride(0) if aux is not None else 0), aux_mod=aux_mod, drop_p=drop_p,
                drop_key=drop_key, site_a=site_a or 0, site_b=site_b or 0)


def linear_bwd_input(dy, W, out=None, *, beta=0.0, relu_mask_of=None, alpha=1.0):
    """out[M,K] = (dy[M,N] @ W[N,K]) (* (relu_mask_of > 0)) (+ beta*out)."""
    M, N = dy.shape
    K = W.shape[1]
    if out is None:
        out = torch.empty(M, K, device=dy.device, dtype=torch.float32)
    epi = (_hip.RS_EPI_AUX_MASK if relu_mask_of is not None else 0) | _io_flags(dy, out)
    return gemm(dy, W, out, M, K, N, transA=0, transB=0, lda=dy.stride(0), ldb=W.stride(0),
                ldc=out.stride(0), alpha=alpha, beta=beta, epi=epi, aux=relu_mask_of,
                ld_aux=(relu_mask_of.stride(0) if relu_mask_of is not None else 0))


def linear_bwd_weight(dy, x, dW, *, beta=1.0, db=None):
    """dW[N,K] (+)= dy[M,N]^T @ x[M,K] (reduction over M, split-K); db[N] += colsum(dy) fused."""
    M, N = dy.shape
    K = x.shape[1]
    return gemm(dy, x, dW, N, K, M, transA=1, transB=0, lda=dy.stride(0), ldb=x.stride(0),
                ldc=dW.stride(0), beta=beta, rowsum=db)


def ffn_supported(rows, W1):
    """The fused feed-forward block on `rows` rows: bf16 compute mode, d_model 64, dim_feedforward
    256 (W1 [256, 64]), rows a multiple of 16."""
    return (precision.compute_dtype() == 'bf16' and not os.environ.get('RSYS_UNFUSED_FFN') and
            tuple(W1.shape) == (256, 64) and rows % 16 == 0)


def ffn_fwd_bf16(x, W1, b1, W2, b2, gamma, beta, eps, p, key, site1, site2):
    """x2 = LN(x + drop2(linear2(drop(relu(linear1(x)))))) -> (h, x2, mean, rstd, mask)."""
    M, F = x.shape[0], W1.shape[0]
    dev = x.device
    h = torch.empty(M, 64, device=dev)
    y = torch.empty(M, 64, device=dev)
    mean = torch.empty(M, device=dev)
    rstd = torch.empty(M, device=dev)
    mask = torch.empty(int(_hip.lib().rs_ffn_mask_words(M, F)), dtype=torch.int64, device=dev)
    call('rs_ffn_fwd_bf16', M, F, P(x), P(W1), P(b1), P(W2), P(b2), P(gamma), P(beta), float(eps), P(h),
         P(y), P(mean), P(rstd), P(mask), float(p), P(key), site1, site2, stream())
    return h, y, mean, rstd, mask


def ffn_bwd_bf16(x, W1, b1, W2, mask, dff, dres, p, dx=None, acts=True):
    """-> (dx = dres + dPre1 W1, f1 bf16 [M,F], dPre1 bf16 [M,F]); acts=False: f1 / dPre1 are
    not written (None; the weight gradients by ffn_wgrad_bf16)."""
    M, F = x.shape[0], W1.shape[0]
    dev = x.device
    if dx is None:
        dx = torch.empty_like(dres)
    f1 = torch.empty(M, F, device=dev, dtype=torch.bfloat16) if acts else None
    dpre = torch.empty(M, F, device=dev, dtype=torch.bfloat16) if acts else None
    call('rs_ffn_bwd_bf16', M, F, P(x), P(W1), P(b1), P(W2), P(mask), P(dff), P(dres), P(dx), P(f1), P(dpre),
         float(p), stream())
    return dx, f1, dpre


def ffn_bwd_ln_bf16(x, W1, b1, W2, mask, dff, dres, h1, gamma1, mean1, rstd1, dgamma1, dbeta1, p,
                    key, site, acts=True):
    """ffn_bwd_bf16 with norm1's backward fused: -> (dh1, dsa or None, f1 bf16, dPre1 bf16)
    (acts=False: f1 / dPre1 None, as in ffn_bwd_bf16)."""
    M, F = x.shape[0], W1.shape[0]
    dev = x.device
    dh1 = torch.empty_like(dres)
    dsa = torch.empty_like(dres) if p > 0 else None
    f1 = torch.empty(M, F, device=dev, dtype=torch.bfloat16) if acts else None
    dpre = torch.empty(M, F, device=dev, dtype=torch.bfloat16) if acts else None
    w = ws(_hip.lib().rs_ffn_bwd_ln_ws_bytes(M, F), dev)
    call('rs_ffn_bwd_ln_bf16', M, F, P(x), P(W1), P(b1), P(W2), P(mask), P(dff), P(dres), P(h1), P(gamma1),
         P(mean1), P(rstd1), P(dh1), P(dsa), P(dgamma1), P(dbeta1), P(f1), P(dpre), float(p), P(key), site,
         P(w), stream())
    return dh1, dsa, f1, dpre


def ffn_bwd_ln2_bf16(x, W1, b1, W2, mask, dy2, h2, gamma2, mean2, rstd2, dgamma2, dbeta2, h1, gamma1,
                     mean1, rstd1, dgamma1, dbeta1, p, key, site1, site2, dsa=True):
    """norm2's backward + the FFN backward + norm1's backward in one pass (weight gradients by
    ffn_wgrad_bf16 from the returned dff): -> (dh1, dsa or None, dff = drop2(dh2)). dsa=False:
    dsa = drop1(dh1) is not stored (None; outproj_bwd_fused masks dh1 itself). x (= x1) is not read
    by this kernel and may be None (a forward that did not store it)."""
    M, F = dy2.shape[0], W1.shape[0]
    dff = torch.empty_like(dy2)
    dh1 = torch.empty_like(dy2)
    dsa = torch.empty_like(dy2) if p > 0 and dsa else None
    w = ws(_hip.lib().rs_ffn_bwd_ln2_ws_bytes(M, F), dy2.device)
    call('rs_ffn_bwd_ln2_bf16', M, F, P(x), P(W1), P(b1), P(W2), P(mask), P(dy2), P(h2), P(gamma2), P(mean2),
         P(rstd2), P(dff), P(dgamma2), P(dbeta2), P(h1), P(gamma1), P(mean1), P(rstd1), P(dh1), P(dsa),
         P(dgamma1), P(dbeta1), float(p), P(key), site1, site2, P(w), stream())
    return dh1, dsa, dff


def ffn_wgrad_bf16(x, W1, b1, W2, mask, dff, p, dW1, db1, dW2, db2):
    """dW1 += dPre1^T x, db1 += colsum(dPre1), dW2 += dff^T f1, db2 += colsum(dff), f1 / dPre1
    recomputed on chip (csrc/ffn.hip rs_ffn_wgrad_bf16)."""
    M, F = x.shape[0], W1.shape[0]
    w = ws(_hip.lib().rs_ffn_wgrad_ws_bytes(M, F), x.device)
    call('rs_ffn_wgrad_bf16', M, F, P(x), P(W1), P(b1), P(W2), P(mask), P(dff), float(p), P(dW1), P(db1),
         P(dW2), P(db2), P(w), stream())


def ffn_wgrad_ln_bf16(h1, mean1, rstd1, gamma1, beta1, W1, b1, W2, mask, dff, p, dW1, db1, dW2, db2):
    """ffn_wgrad_bf16 with x1 = LN1(h1) rebuilt while the rows are staged instead of read (the
    forward's bits: csrc/ffn.hip ln_apply), for a forward that did not store x1
    (rs_ffn_wgrad_ln_bf16)."""
    M, F = h1.shape[0], W1.shape[0]
    w = ws(_hip.lib().rs_ffn_wgrad_ws_bytes(M, F), h1.device)
    call('rs_ffn_wgrad_ln_bf16', M, F, P(h1), P(mean1), P(rstd1), P(gamma1), P(beta1), P(W1), P(b1), P(W2),
         P(mask), P(dff), float(p), P(dW1), P(db1), P(dW2), P(db2), P(w), stream())


def wgrad_bf16(dy, x, dW, *, db=None, beta=1.0):
    """dW[Mo,No] = beta*dW + dy[rows,Mo]^T x[rows,No] on bf16 MFMA; db += colsum(dy). dy / x may be
    fp32 or bf16 tensors."""
    rows, Mo = dy.shape
    No = x.shape[1]
    w = ws(_hip.lib().rs_wgrad_ws_bytes(Mo, No, rows), dy.device)
    call('rs_wgrad_bf16', rows, Mo, No, P(dy), dy.stride(0), int(dy.dtype == torch.bfloat16), P(x), x.stride(0),
         int(x.dtype == torch.bfloat16), float(beta), P(dW), dW.stride(0), P(db), P(w), stream())
    return dW


def _aligned16(*tensors):
    """The 16-byte alignment the one-pass kernels' vector loads need (their entry points check it):
    a view that lacks it takes the unfused path."""
    return all(t.data_ptr() % 16 == 0 for t in tensors)


def linear_bwd_fused_ok(dy, x, W, dW, dx_in=None):
    """The one-pass Linear backward for a bf16-stored dy (csrc/linear_bwd.hip: the in-projection's
    [M, 192] x [192, 64]): bf16 compute mode, a covered shape, and RSYS_LINBWD_FUSED not 0."""
    if precision.compute_dtype() != 'bf16' or os.environ.get('RSYS_LINBWD_FUSED', '1') == '0':
        return False
    M, N = dy.shape
    K = x.shape[1]
    return (dy.dtype == torch.bfloat16 and x.dtype == torch.float32 and dy.is_contiguous() and
            x.is_contiguous() and tuple(W.shape) == (N, K) and W.stride(1) == 1 and W.stride(0) % 4 == 0 and
            dW.is_contiguous() and _aligned16(dy, x, W) and
            (dx_in is None or (dx_in.is_contiguous() and tuple(dx_in.shape) == (M, K) and _aligned16(dx_in))) and
            _hip.lib().rs_linear_bwd_bf16_ws_bytes(M, N, K) > 0)


def linear_bwd_fused(dy, x, W, dW, db, dx_in=None):
    """dW += dy^T x, db += colsum(dy), returns dx = dy W (+ dx_in, written over dx_in) from one read
    of dy (rs_linear_bwd_bf16)."""
    M, N = dy.shape
    K = x.shape[1]
    if dx_in is not None and not (dx_in.is_contiguous() and tuple(dx_in.shape) == (M, K)):
        raise RuntimeError('linear_bwd_fused: dx_in must be a contiguous [M, K] tensor')
    dx = dx_in if dx_in is not None else torch.empty(M, K, device=dy.device, dtype=torch.float32)
    w = ws(_hip.lib().rs_linear_bwd_bf16_ws_bytes(M, N, K), dy.device)
    call('rs_linear_bwd_bf16', P(dy), P(x), P(W), W.stride(0), M, N, K, P(dx_in), P(dx), P(dW), P(db), P(w),
         stream())
    return dx


def outproj_bwd_fused_ok(dh, att, W, dW):
    """The one-pass backward of the attention out-projection (csrc/linear_bwd.hip
    rs_outproj_bwd_bf16): bf16 compute mode, d_model 64, RSYS_OUTPROJ_BWD_FUSED not 0, and a token
    count at which the pair it replaces is the bf16 streaming pair (wgrad_bf16 and the bf16 row GEMM:
    >= 32,768 rows, a multiple of 16), whose bits it reproduces. Below that the input gradient is an
    fp32-MFMA GEMM (the pruned last layer's B rows), which stays as it is."""
    if precision.compute_dtype() != 'bf16' or os.environ.get('RSYS_OUTPROJ_BWD_FUSED', '1') == '0':
        return False
    M, d = dh.shape
    return (d == 64 and M >= STREAM_BF16_MIN_ROWS and M % 16 == 0 and
            dh.dtype == torch.float32 and att.dtype == torch.float32 and dh.is_contiguous() and
            att.is_contiguous() and tuple(att.shape) == (M, d) and tuple(W.shape) == (d, d) and
            W.stride(1) == 1 and dW.is_contiguous() and _aligned16(dh, att) and
            _hip.lib().rs_outproj_bwd_bf16_ws_bytes(M, d) > 0)


def outproj_bwd_fused(dh, att, W, p, key, site, dW, db):
    """dW += y^T att, db += colsum(y), returns datt = y W with y = dh * mask(key, site) (p == 0:
    y = dh), from one read of dh, which is not written (rs_outproj_bwd_bf16)."""
    M, d = dh.shape
    datt = torch.empty(M, d, device=dh.device, dtype=torch.float32)
    w = ws(_hip.lib().rs_outproj_bwd_bf16_ws_bytes(M, d), dh.device)
    call('rs_outproj_bwd_bf16', P(dh), P(att), P(W), W.stride(0), M, d, float(p), P(key) if p > 0 else None, site,
         P(datt), P(dW), P(db), P(w), stream())
    return datt


def colsum(X, out, *, scale=1.0, beta=1.0, M=None, N=None, ldx=None):
    """out[n] = beta*out[n] + scale*sum_m X[m, n]."""
    if M is None:
        M, N = X.shape
        ldx = X.stride(0)
    w = ws(_hip.lib().rs_colsum_ws_bytes(M, N), X.device)
    call('rs_colsum', P(X), M, N, ldx, float(scale), float(beta), P(out), P(w), stream())
    return out


def seq_mask(seq, pad_value=0):
    B, L = seq.shape[0], seq.shape[1]
    key_pad = torch.empty(B, L, dtype=torch.uint8, device=seq.device)
    last = torch.empty(B, dtype=torch.int64, device=seq.device)
    call('rs_seq_mask', P(seq), seq.stride(0), B, L, int(pad_value), P(key_pad), P(last), stream())
    return key_pad, last


def segments_array(segs):
    arr = (_hip.FeatureSeg * len(segs))(*segs)
    return arr


def gather_plan(segs, rows, ldo, bwd):
    """rs_gather_plan (host only): the per-segment _hip.GatherSegPlan array and the
    _hip.GatherLaunchPlan of a gather_fwd / gather_bwd call."""
    per, launch = (_hip.GatherSegPlan * len(segs))(), _hip.GatherLaunchPlan()
    call('rs_gather_plan', segments_array(segs), len(segs), rows, ldo, int(bwd), per, _hip.C.byref(launch))
    return per, launch


def gather_fwd(segs, rows, out, err_flag=None, lazy=None):
    """rs_gather_fwd; with `lazy` = (m_off, v_off, step, consts, b1, b2, eps, wd) the segments
    whose lazy_last is set read their rows through the lazy-Adam catch-up (rs_gather_fwd_lazy)."""
    arr = segments_array(segs)
    if lazy is not None and any(s.lazy_last for s in segs):
        call('rs_gather_fwd_lazy', arr, len(segs), rows, P(out), out.stride(0), P(err_flag), *lazy, stream())
    else:
        call('rs_gather_fwd', arr, len(segs), rows, P(out), out.stride(0), P(err_flag), stream())
    return out


_DETERMINISTIC = [None]


def sync_deterministic():
    """Mirror torch.are_deterministic_algorithms_enabled() into the library (rs_set_deterministic):
    deterministic table gradients (slot-image / ranged kernels) instead of the float-atomic
    scatter. RSYS_DETERMINISTIC=1 turns it on regardless."""
    on = bool(torch.are_deterministic_algorithms_enabled())
    if on != _DETERMINISTIC[0]:
        _hip.lib().rs_set_deterministic(int(on))
        _DETERMINISTIC[0] = on


def deterministic_enabled() -> bool:
    """Deterministic table gradients requested (torch.use_deterministic_algorithms or
    RSYS_DETERMINISTIC=1)."""
    return bool(torch.are_deterministic_algorithms_enabled()) or os.environ.get('RSYS_DETERMINISTIC', '0') == '1'


def gather_bwd(segs, rows, dout):
    sync_deterministic()
    arr = segments_array(segs)
    # hot mid-size tables (C2's 3,500-row history table) reduce per-chunk partials from ws
    w = ws(_hip.lib().rs_gather_ws_bytes(arr, len(segs), rows), dout.device)
    call('rs_gather_bwd', arr, len(segs), rows, P(dout), dout.stride(0), P(w), stream())


STREAM_BF16_MIN_ROWS = 32768  # gemm_stream.hip kSmallM: the bf16-storage GEMM instances are big-M only


def attn_plan(B, L, d, H, p, flags, bwd=False, strict=True):
    """rs_attn_plan (host only): the _hip.AttnPlan of an attn_fwd / attn_bwd call with these flags --
    its kernel route (.route_name, one of _hip.ATTN_ROUTES), whether that route takes bf16-stored qkv,
    the keep-bit words the forward saves, and whether attn_rows_* take the shape. strict: raise where
    attn_fwd / attn_bwd would. Not strict, for a caller that only asks what the shape could take
    (plan_encoder: a pruned layer never calls attn_fwd): no error, the plan as far as the library
    filled it -- whole but for a VALU shape beyond its LDS, all zero for a shape it refuses outright.
    Not through call(): a plan is no launch, and call() is where launches are timed and recorded."""
    plan, lib = _hip.AttnPlan(), _hip.lib()
    if lib.rs_attn_plan(B, L, d, H, float(p), flags, int(bwd), _hip.C.byref(plan)) != 0 and strict:
        raise _hip.HipError(f"rs_attn_plan failed: {lib.rs_last_error().decode(errors='replace')}")
    return plan


def qkv_bf16_ok(L, d, H, M, plan=None):
    """Store the packed qkv (and dqkv) as bf16: bf16 compute mode on an attention route that takes
    it (attn_plan: Q, K, V are only MFMA operands there, RS_ATTN_QKV_BF16), for token counts M the
    bf16-storage streaming GEMMs cover (M >= 32768, a multiple of 16). plan: the caller's
    attn_plan(M // L, L, d, H, 0, gemm_flags, strict=False) where it already has it."""
    if not (precision.compute_dtype() == 'bf16' and M >= STREAM_BF16_MIN_ROWS and M % 16 == 0 and
            not os.environ.get('RSYS_QKV_FP32')):
        return False
    if plan is None:
        plan = attn_plan(M // L, L, d, H, 0.0, precision.gemm_flags(), strict=False)
    return bool(plan.qkv_bf16)


def _attn_flags(qkv):
    return precision.gemm_flags() | (_hip.RS_ATTN_QKV_BF16 if qkv.dtype == torch.bfloat16 else 0)


def attn_fwd(qkv, key_pad, B, L, d, H, p=0.0, key=None, site=0):
    """-> out [B*L, d], lse [B*H*L]. Where the kernel saves its dropout keep bits for the backward
    (attn_plan's zbits_words), they live in lse's storage past its B*H*L floats, so whoever keeps lse for
    attn_bwd keeps them too; an lse without that tail makes attn_bwd draw them again."""
    out = torch.empty(B * L, d, device=qkv.device, dtype=torch.float32)
    flags = _attn_flags(qkv)
    n, zw = B * H * L, attn_plan(B, L, d, H, p, flags).zbits_words
    if zw:
        buf = torch.empty(n + (zw + 1) // 2 + 4, device=qkv.device, dtype=torch.float32)
        lse, zb = buf[:n], _zbits_ptr(buf, n)
    else:
        lse, zb = torch.empty(n, device=qkv.device, dtype=torch.float32), None
    call('rs_attn_fwd', P(qkv), P(key_pad), P(out), P(lse), B, L, d, H,
         float((d // H) ** -0.5), float(p), P(key), site, flags, stream(), zb)
    return out, lse


def _zbits_ptr(lse, n):
    return (lse.data_ptr() + 4 * n + 15) // 16 * 16  # 16-byte aligned start past the lse floats


def attn_bwd(qkv, key_pad, out, dout, lse, B, L, d, H, p=0.0, key=None, site=0):
    """dqkv has qkv's storage dtype (bf16 with RS_ATTN_QKV_BF16)."""
    dqkv = torch.empty(B * L, 3 * d, device=qkv.device, dtype=qkv.dtype)
    flags = _attn_flags(qkv)
    n, zw = B * H * L, attn_plan(B, L, d, H, p, flags, bwd=True).zbits_words
    zb = None
    if zw and lse.storage_offset() == 0 and lse.numel() == n and \
            lse.untyped_storage().nbytes() == 4 * (n + (zw + 1) // 2 + 4):
        zb = _zbits_ptr(lse, n)  # attn_fwd's tail (its docstring; exactly its allocation's size)
    call('rs_attn_bwd', P(qkv), P(key_pad), P(out), P(dout), P(lse), P(dqkv), B, L, d, H,
         float((d // H) ** -0.5), float(p), P(key), site, flags, stream(), zb)
    return dqkv


def attn_rows_fwd(qkv, key_pad, last, B, L, d, H, p=0.0, key=None, site=0):
    """Attention of the selected query row last[b] of each sample -> out [B, d], lse [B*H]."""
    out = torch.empty(B, d, device=qkv.device, dtype=torch.float32)
    lse = torch.empty(B * H, device=qkv.device, dtype=torch.float32)
    call('rs_attn_rows_fwd', P(qkv), P(key_pad), P(last), P(out), P(lse), B, L, d, H,
         float((d // H) ** -0.5), float(p), P(key), site, _attn_flags(qkv), stream())
    return out, lse


def attn_rows_bwd(qkv, key_pad, last, dout, lse, B, L, d, H, p=0.0, key=None, site=0):
    """-> dqkv [B*L, 3d] (qkv's dtype), dQ zero off the selected rows."""
    dqkv = torch.empty(B * L, 3 * d, device=qkv.device, dtype=qkv.dtype)
    call('rs_attn_rows_bwd', P(qkv), P(key_pad), P(last), P(dout), P(lse), P(dqkv), B, L, d, H,
         float((d // H) ** -0.5), float(p), P(key), site, _attn_flags(qkv), stream())
    return dqkv


def linear_add_layernorm(x, W, bias, resid, gamma, beta, eps=1e-5, p=0.0, key=None, site=0):
    """h = dropout(x W^T + bias) + resid, y = LayerNorm(h): one fused kernel at the encoder
    width. Returns h (kept for the backward), y, mean, rstd."""
    M, K = x.shape
    N = W.shape[0]
    if tuple(resid.shape) != (M, N) or not resid.is_contiguous():
        raise RuntimeError('linear_add_layernorm: resid must be a contiguous [M, N] tensor')
    dev = x.device
    h = torch.empty(M, N, device=dev, dtype=torch.float32)
    y = torch.empty(M, N, device=dev, dtype=torch.float32)
    mean = torch.empty(M, device=dev, dtype=torch.float32)
    rstd = torch.empty(M, device=dev, dtype=torch.float32)
    call('rs_gemm_add_layernorm', M, N, K, P(x), x.stride(0), P(W), W.stride(0), P(bias), P(resid),
         P(h), P(y), P(gamma), P(beta), P(mean), P(rstd), float(eps), float(p), P(key), site,
         precision.gemm_flags(), stream())
    return h, y, mean, rstd


def linear_add_layernorm_rows_ok(M, W):
    """rs_gemm_add_layernorm_rows takes M rows through W [64, K]: bf16 MFMA mode, M a multiple of
    16, K 64 or 256."""
    return bool(precision.gemm_flags() & _hip.RS_GEMM_BF16) and M % 16 == 0 and W.dim() == 2 and \
        W.shape[0] == 64 and W.shape[1] in (64, 256) and W.stride(0) % 4 == 0


def linear_add_layernorm_rows(x, W, bias, table, rows, bag, gamma, beta, eps=1e-5, p=0.0, key=None, site=0):
    """linear_add_layernorm with the residual rows read in place: row m's residual is
    table[m * bag + rows[m]] (rs_gemm_add_layernorm_rows). Only where linear_add_layernorm_rows_ok
    holds (elsewhere the caller gathers the rows and runs linear_add_layernorm)."""
    M, K = x.shape
    N = W.shape[0]
    if not linear_add_layernorm_rows_ok(M, W) or K != W.shape[1] or x.stride(0) % 4 or \
            rows.dtype != torch.int64 or not table.is_contiguous():
        raise RuntimeError('linear_add_layernorm_rows: a shape or layout the fused bf16 kernel does not take')
    dev = x.device
    h = torch.empty(M, N, device=dev, dtype=torch.float32)
    y = torch.empty(M, N, device=dev, dtype=torch.float32)
    mean = torch.empty(M, device=dev, dtype=torch.float32)
    rstd = torch.empty(M, device=dev, dtype=torch.float32)
    call('rs_gemm_add_layernorm_rows', M, N, K, P(x), x.stride(0), P(W), W.stride(0), P(bias), P(table), P(rows),
         int(bag), P(h), P(y), P(gamma), P(beta), P(mean), P(rstd), float(eps), float(p), P(key), site,
         precision.gemm_flags(), stream())
    return h, y, mean, rstd


def fwd_chain_on() -> bool:
    """The encoder forward's chained kernels (csrc/chain.h: a Linear computed from the rows the
    previous stage still holds on chip): bf16 compute mode, RSYS_FWD_CHAIN not 0."""
    return precision.compute_dtype() == 'bf16' and os.environ.get('RSYS_FWD_CHAIN', '1') != '0'


def _rowmajor(W, cols):
    return W.dim() == 2 and W.shape[1] == cols and W.stride(1) == 1 and W.stride(0) % 4 == 0


def layer_tail_ok(rows, W1, Wo):
    """The encoder layer's fused forward tail (rs_layer_tail_fwd_bf16) on `rows` rows: where the
    fused FFN runs (d = 64, F = 256, rows a multiple of 16) and the out-projection's fused LayerNorm
    is not switched off (RSYS_UNFUSED_LN), RSYS_FWD_CHAIN not 0. The attention output and the
    residual are the encoder's own fresh fp32 allocations; layer_tail_fwd and the entry point guard
    them."""
    return (fwd_chain_on() and ffn_supported(rows, W1) and
            os.environ.get('RSYS_UNFUSED_LN', '0') in ('', '0') and
            tuple(Wo.shape) == (64, 64) and _rowmajor(Wo, 64) and _aligned16(Wo))


def layer_tail_qkv_ok(Win):
    """The fused tail can also emit the next layer's qkv through that layer's in-projection Win."""
    return Win.shape[0] == 192 and _rowmajor(Win, 64) and _aligned16(Win)


def layer_tail_fwd(att, Wo, bo, resid, g1, be1, eps1, W1, b1, W2, b2, g2, be2, eps2, p, key, site,
                   Win=None, bin_=None, rows=None, bag=0, store_x1=True):
    """out-proj + dropout1 + residual + LN1 + FFN + LN2 (+ the next layer's qkv when Win is given)
    in one pass over the rows -> (h1, x1, mean1, rstd1, h2, x2, mean2, rstd2, mask, qkv or None).
    Dropout sites: site + 1 (dropout1), site + 2, site + 3 (the FFN's). rows / bag: the residual of
    row m is resid[m * bag + rows[m]]. store_x1 false: x1 is not written (returned as None); the
    backward rebuilds it from h1, mean1, rstd1 (ffn_wgrad_ln_bf16)."""
    M = att.shape[0]
    F = W1.shape[0]
    dev = att.device
    h1, h2, x2 = (torch.empty(M, 64, device=dev) for _ in range(3))
    x1 = torch.empty(M, 64, device=dev) if store_x1 else None
    m1, r1, m2, r2 = (torch.empty(M, device=dev) for _ in range(4))
    mask = torch.empty(int(_hip.lib().rs_ffn_mask_words(M, F)), dtype=torch.int64, device=dev)
    qkv = torch.empty(M, 192, device=dev, dtype=torch.bfloat16) if Win is not None else None
    if not resid.is_contiguous() or (rows is None and tuple(resid.shape) != (M, 64)):
        raise RuntimeError('layer_tail_fwd: resid must be a contiguous [M, 64] tensor (or a table with rows)')
    call('rs_layer_tail_fwd_bf16', M, F, P(att), P(Wo), Wo.stride(0), P(bo), P(resid), P(rows), int(bag),
         P(g1), P(be1), float(eps1), P(h1), P(x1), P(m1), P(r1), P(W1), P(b1), P(W2), P(b2), P(g2), P(be2),
         float(eps2), P(h2), P(x2), P(m2), P(r2), P(mask), P(Win), Win.stride(0) if Win is not None else 0,
         P(bin_), P(qkv), float(p), P(key) if p > 0 else None, site + 1, site + 2, site + 3, stream())
    return h1, x1, m1, r1, h2, x2, m2, r2, mask, qkv


def add_layernorm_fwd(a, b, gamma, beta, eps=1e-5, p=0.0, key=None, site=0):
    """h = dropout(a) + b (into a); returns y, mean, rstd."""
    M, N = a.shape
    y = torch.empty_like(a)
    mean = torch.empty(M, device=a.device, dtype=torch.float32)
    rstd = torch.empty(M, device=a.device, dtype=torch.float32)
    call('rs_add_layernorm_fwd', P(a), P(b), P(gamma), P(beta), P(y), P(mean), P(rstd), M, N,
         float(eps), float(p), P(key), site, stream())
    return y, mean, rstd


def layernorm_bwd(h, dy, gamma, mean, rstd, dgamma, dbeta, dh=None, da=None, p=0.0, key=None,
                  site=0):
    """dh = LN backward (in place over dy by default); da = dropout-backward(dh) if given."""
    M, N = h.shape
    if dh is None:
        dh = dy
    w = ws(_hip.lib().rs_layernorm_ws_bytes(M, N), h.device)
    call('rs_layernorm_bwd', P(h), P(dy), P(gamma), P(mean), P(rstd), P(dh), P(dgamma), P(dbeta),
         M, N, P(da), float(p), P(key), site, P(w), stream())
    return dh


def rng_next(state):
    key = torch.empty(2, dtype=torch.int64, device=state.device)
    call('rs_rng_next', P(state), P(key), stream())
    return key


def dropout_fwd(x, p, key, site, aux=None, aux_mod=0):
    """x = dropout(x (+ aux[row % aux_mod])) in place; x is [M, N] contiguous."""
    N = x.shape[-1]
    call('rs_dropout_fwd', P(x), x.numel(), N, P(aux), aux.stride(0) if aux is not None else 0,
         aux_mod, float(p), P(key), site, stream())
    return x


def seq_input_dropout_bwd(dx, pos_grad, rows, N, p, key, site_a, site_b):
    """dx [rows, N] <- dx * mask_b * mask_a; pos_grad[:N] += colsum(dx * mask_b) (one pass)."""
    w = ws(_hip.lib().rs_seq_input_dropout_bwd_ws_bytes(rows, N), dx.device)
    call('rs_seq_input_dropout_bwd', P(dx), rows, N, float(p), P(key), site_a, site_b, P(pos_grad), P(w),
         stream())
    return dx


def seq_input_bwd_fused_ok(dx, cat, W, dW, L):
    """The one-pass sequence-input backward (csrc/linear_bwd.hip): bf16 compute mode, a supported
    shape, and RSYS_SEQ_BWD_FUSED not 0."""
    if precision.compute_dtype() != 'bf16' or os.environ.get('RSYS_SEQ_BWD_FUSED', '1') == '0':
        return False
    M, d = dx.shape
    dcat = cat.shape[1]
    return (dx.is_contiguous() and dx.dtype == torch.float32 and cat.dtype == torch.float32 and
            cat.stride(1) == 1 and cat.stride(0) % 4 == 0 and tuple(W.shape) == (d, dcat) and W.stride(1) == 1 and
            dW.is_contiguous() and _aligned16(dx, cat) and L >= 1 and M % L == 0 and (L * d) % 4 == 0 and
            bool(_hip.lib().rs_seq_input_bwd_bf16_supported(M, d, dcat)))


def seq_input_bwd_fused(dx, cat, W, L, p, key, site_a, site_b, dW, db, pos_grad):
    """dcat = (dx * mask_b * mask_a) W; dW += y^T cat, db += colsum(y) in one pass
    (rs_seq_input_bwd_bf16), and pos_grad[:L] += the sum over samples of dx * mask_b
    (rs_seq_input_pos_grad); dx is only read. Returns dcat."""
    M, d = dx.shape
    dcat = cat.shape[1]
    k = P(key) if p > 0 else None
    w = ws(_hip.lib().rs_seq_input_dropout_bwd_ws_bytes(M // L, L * d), dx.device)
    call('rs_seq_input_pos_grad', P(dx), M // L, L * d, float(p), k, site_b, P(pos_grad), P(w), stream())
    out = torch.empty(M, dcat, device=dx.device, dtype=torch.float32)
    w = ws(_hip.lib().rs_seq_input_bwd_bf16_ws_bytes(M, d, dcat), dx.device)
    call('rs_seq_input_bwd_bf16', P(dx), P(cat), cat.stride(0), P(W), W.stride(0), M, d, dcat, float(p), k,
         site_a, site_b, P(out), P(dW), P(db), P(w), stream())
    return out


def seq_head_ok(segs, M, L, dcat, lin, pos, attn, qkv_bf16=None):
    """The fused sequence head (rs_seq_head_fwd_bf16: gather + projection + layer 0's in-projection
    in one kernel): bf16 compute mode with the chained forward on (fwd_chain_on), bf16 qkv
    (qkv_bf16_ok), d = 64, a schema and shape the kernel takes (rs_seq_head_fwd_bf16_supported:
    single-id or mean / sum pooled segments on ordinary tables, widths multiples of 4, dcat <= 64,
    bag <= 8, the positional table within its LDS budget), both biases present, and
    RSYS_SEQ_HEAD_FUSED not 0. The caller checks that no segment is a lazy-Adam call. qkv_bf16:
    qkv_bf16_ok's answer where the caller already has it."""
    if os.environ.get('RSYS_SEQ_HEAD_FUSED', '1') == '0' or not fwd_chain_on():
        return False
    W, Win = lin.weight, attn.in_proj_weight
    d = W.shape[0]
    if lin.bias is None or attn.in_proj_bias is None or Win is None or d != 64 or attn.embed_dim != d:
        return False
    if not (qkv_bf16_ok(L, d, attn.num_heads, M) if qkv_bf16 is None else qkv_bf16):
        return False
    lib = _hip.lib()
    return (tuple(W.shape) == (64, dcat) and _rowmajor(W, dcat) and tuple(Win.shape) == (192, 64) and
            _rowmajor(Win, 64) and _aligned16(W, Win) and pos.dim() == 2 and pos.shape[1] == 64 and
            pos.stride(1) == 1 and pos.shape[0] >= L and
            all(t.dtype == torch.float32 for t in (W, Win, pos, lin.bias, attn.in_proj_bias)) and
            bool(lib.rs_seq_head_fwd_bf16_supported(segments_array(segs), len(segs), M, L, d, dcat)))


def seq_head_fwd(segs, M, L, dcat, W, b, pos, Win, bin_, err_flag, p, key, site_a, site_b):
    """cat [M, dcat] (the gathered features, fp32), x0 = drop_b(drop_a(cat W^T + b) + pos[m % L])
    (fp32) and qkv0 = x0 Win^T + bin (bf16) from the segments' ids in one kernel -> (x0, cat, qkv0)."""
    dev = W.device
    x0 = torch.empty(M, 64, device=dev, dtype=torch.float32)
    cat = torch.empty(M, dcat, device=dev, dtype=torch.float32)
    qkv = torch.empty(M, 192, device=dev, dtype=torch.bfloat16)
    call('rs_seq_head_fwd_bf16', segments_array(segs), len(segs), M, L, dcat, P(W), W.stride(0), P(b), P(pos),
         pos.stride(0), P(Win), Win.stride(0), P(bin_), P(x0), P(cat), P(qkv), P(err_flag), float(p),
         P(key) if p > 0 else None, site_a, site_b, stream())
    return x0, cat, qkv


def dropout_bwd(dx, p, key, site):
    call('rs_dropout_bwd', P(dx), dx.numel(), float(p), P(key), site, stream())
    return dx


def batchnorm_fwd(x, bn, G, relu, training, momentum=None, eps=None, drop_p=0.0, drop_key=None,
                  drop_site=0):
    """x [G*Bg, C]; bn: nn.BatchNorm1d-like (weight, bias, running_*, num_batches_tracked).
    drop_p > 0: the following nn.Dropout fused into the output (relu and training only)."""
    M, Cc = x.shape
    Bg = M // G
    y = torch.empty_like(x)
    mean = torch.empty(G * Cc, device=x.device, dtype=torch.float32)
    rstd = torch.empty(G * Cc, device=x.device, dtype=torch.float32)
    mom = bn.momentum if momentum is None else momentum
    if mom is None:
        raise NotImplementedError('BatchNorm1d(momentum=None) (cumulative average) is not supported')
    track = bn.track_running_stats and bn.running_mean is not None
    batch_stats = training or not track          # nn.BatchNorm1d: eval uses running stats
    update = training and track
    run = update or not batch_stats
    w = ws(_hip.lib().rs_batchnorm_ws_bytes(G, Bg, Cc), x.device)
    call('rs_batchnorm_fwd', P(x), P(y), P(bn.weight), P(bn.bias),
         P(bn.running_mean) if run else None, P(bn.running_var) if run else None,
         P(bn.num_batches_tracked) if update else None,
         P(mean), P(rstd), G, Bg, Cc, float(mom), float(bn.eps if eps is None else eps), int(relu),
         int(batch_stats), float(drop_p), P(drop_key), drop_site, P(w), stream())
    return y, mean, rstd


def batchnorm_bwd(x, y, dy, weight, mean, rstd, dw, db, G, relu, dx=None, drop_p=0.0):
    M, Cc = x.shape
    Bg = M // G
    if dx is None:
        dx = torch.empty_like(x)
    w = ws(_hip.lib().rs_batchnorm_ws_bytes(G, Bg, Cc), x.device)
    # the fused dropout's scale, in the forward's fp32 arithmetic (rng.h make_key)
    scale = float(np.float32(1.0) / (np.float32(1.0) - np.float32(drop_p))) if drop_p > 0 else 1.0
    call('rs_batchnorm_bwd', P(x), P(y), P(dy), P(weight), P(mean), P(rstd), P(dx), P(dw), P(db),
         G, Bg, Cc, int(relu), scale, P(w), stream())
    return dx


def l2norm_fwd(x, eps=1e-12):
    M, N = x.shape
    y = torch.empty_like(x)
    norm = torch.empty(M, device=x.device, dtype=torch.float32)
    call('rs_l2norm_fwd', P(x), P(y), P(norm), M, N, float(eps), stream())
    return y, norm


def l2norm_bwd(y, norm, dy, eps=1e-12):
    M, N = y.shape
    dx = torch.empty_like(y)
    call('rs_l2norm_bwd', P(y), P(norm), P(dy), P(dx), M, N, float(eps), stream())
    return dx


def _item_kind(name, items, item_exp):
    """The entry-point suffix and the dtype argument of fused_topk / target_rank's items."""
    if items.dtype == torch.float8_e4m3fn:
        if item_exp is None:
            raise ValueError(f'{name}: float8_e4m3fn items need item_exp, the index scale exponent (quantize_e4m3)')
        return '_e4m3', int(item_exp)
    if items.dtype not in (torch.float32, torch.bfloat16):
        raise TypeError(f'{name}: items must be float32, bfloat16 or float8_e4m3fn, got {items.dtype}')
    if item_exp is not None:
        raise ValueError(f'{name}: item_exp goes with float8_e4m3fn items, got {items.dtype}')
    return '', int(items.dtype == torch.bfloat16)


def e4m3_exponent(absmax):
    """The scale exponent of the e4m3 index format for a largest magnitude (rs_e4m3_exponent): the
    largest e with absmax * 2^e <= 448, clamped to [-40, 40]; 0 for absmax = 0."""
    return int(_hip.lib().rs_e4m3_exponent(float(absmax)))


def quantize_e4m3(rows, exp=None):
    """fp32 rows [N, D] (D a multiple of 16) -> (q float8_e4m3fn [N, D], exp): q = RNE(rows * 2^exp)
    on the device (rs_quantize_e4m3), exp = e4m3_exponent(rows.abs().max()) unless given (one host
    sync). The rows must be finite."""
    _hip.require_device(rows)
    x = rows.detach().float()
    if x.dim() != 2 or x.shape[1] % 16 or x.shape[1] < 16:
        raise ValueError(f'quantize_e4m3: rows [N, D] with D a multiple of 16, got {tuple(x.shape)}')
    if x.stride(1) != 1 or x.stride(0) % 4 or x.data_ptr() % 16:
        x = x.contiguous()
    N, D = int(x.shape[0]), int(x.shape[1])
    if exp is None:
        exp = e4m3_exponent(x.abs().max().item()) if N else 0
    q = torch.empty(N, D, device=x.device, dtype=torch.float8_e4m3fn)
    call('rs_quantize_e4m3', P(x), int(x.stride(0)), N, D, int(exp), P(q), D, stream())
    return q, int(exp)


def pack_mask(mask):
    """Allow-lists as the packed words the filtered retrieval kernels read (rs_pack_mask): mask
    [F, N] or [N], bool or uint8 on the device, nonzero = the column is allowed ->
    uint32 [F, ceil(N / 32)], column c at bit c & 31 of word c >> 5, the last word's unused high
    bits zero."""
    _hip.require_device(mask)
    m = mask.detach()
    if m.dim() == 1:
        m = m.view(1, -1)
    if m.dim() != 2 or m.dtype not in (torch.bool, torch.uint8):
        raise ValueError(f'pack_mask: a bool or uint8 mask [F, N] or [N], got {m.dtype} {tuple(mask.shape)}')
    if m.dtype == torch.bool:
        m = m.view(torch.uint8) if m.is_contiguous() else m.to(torch.uint8)
    F, N = int(m.shape[0]), int(m.shape[1])
    if F < 1 or N < 1:
        raise ValueError(f'pack_mask: needs at least one filter and one column, got {tuple(mask.shape)}')
    if m.stride(1) != 1 or (F > 1 and m.stride(0) < N):
        m = m.contiguous()
    W = (N + 31) // 32
    bits = torch.empty(F, W, device=m.device, dtype=torch.uint32)
    call('rs_pack_mask', P(m), int(m.stride(0)) if F > 1 else N, F, N, P(bits), W, stream())
    return bits


def _filter_args(name, filter_ids, filters, B, N):
    """(ids int32 [B], stride, bits, ld, F) of a filtered call: filters = pack_mask's words."""
    if filters is None:
        raise ValueError(f'{name}: filter_ids given without filters (pack_mask)')
    for t in (filter_ids, filters):
        _hip.require_device(t)
    if filters.dim() != 2 or filters.dtype != torch.uint32 or filters.shape[1] < (N + 31) // 32:
        raise ValueError(f'{name}: filters must be uint32 [F, >= {(N + 31) // 32}] (pack_mask), got '
                         f'{filters.dtype} {tuple(filters.shape)}')
    if filters.stride(1) != 1:
        filters = filters.contiguous()
    fid = filter_ids.reshape(-1)
    if fid.numel() != B:
        raise ValueError(f'{name}: {fid.numel()} filter ids for {B} users')
    if fid.dtype != torch.int32:
        fid = fid.long().clamp(-1, int(filters.shape[0])).int()  # out of range either way: unfiltered
    return fid, int(fid.stride(0)), filters, int(filters.stride(0)), int(filters.shape[0])


def fused_topk(U, items, K, user_ids=None, history=None, splits=0, item_exp=None, filter_ids=None, filters=None):
    """The K best catalog columns of every user by dot product, and their scores, without the
    [B, N] score matrix (rs_fused_topk). U [B, D] fp32; items [N, D] fp32, bf16 or float8_e4m3fn
    with item_exp, the index scale exponent (the dtype picks the kernel; rs_fused_topk_e4m3);
    history = (off, idx, num_users) with each user's columns SORTED ascending
    (retrieval.sorted_history_csr), applied when user_ids is given. -> (idx int32 [B, K],
    val fp32 [B, K]), values descending, ties by the lower column. filter_ids integer [B] with
    filters = pack_mask(allow-lists [F, N]) (rs_fused_topk_filtered): user b sees only the columns
    of filter filter_ids[b], the others score -inf as history columns do; an id outside [0, F)
    leaves that user unfiltered. No CPU fallback."""
    use_hist = history is not None and user_ids is not None
    for t in (U, items) + ((user_ids,) + tuple(history[:2]) if use_hist else ()):
        _hip.require_device(t)
    suffix, kind = _item_kind('fused_topk', items, item_exp)
    U = U.float()
    if U.stride(1) != 1 or U.stride(0) % 4 or U.data_ptr() % 16:
        U = U.contiguous()
    if items.stride(1) != 1 or (items.stride(0) * items.element_size()) % 16 or items.data_ptr() % 16:
        items = items.contiguous()
    B, D = int(U.shape[0]), int(U.shape[1])
    N = int(items.shape[0])
    L = _hip.lib()
    if splits <= 0:
        splits = L.rs_fused_topk_splits(B, N, D, K)
    idx = torch.empty(B, K, device=U.device, dtype=torch.int32)
    val = torch.empty(B, K, device=U.device, dtype=torch.float32)
    nbytes = L.rs_fused_topk_ws_bytes(B, N, D, K, splits) if splits > 1 else 0
    w = ws(nbytes, U.device) if splits > 1 else None
    uid, us, off, hidx, nu = None, 0, None, None, 0
    if use_hist:
        uid = user_ids if user_ids.dtype == torch.int64 else user_ids.long()
        us = int(uid.stride(0))
        off, hidx, nu = history
    if filter_ids is None:
        call('rs_fused_topk' + suffix, P(U), int(U.stride(0)), B, P(items), kind,
             int(items.stride(0)), N, D, int(K), P(uid), us, P(off), P(hidx), int(nu), int(splits), P(w), int(nbytes),
             P(idx), P(val), K, stream())
        return idx, val
    fid, fs, bits, fld, F = _filter_args('fused_topk', filter_ids, filters, B, N)
    call('rs_fused_topk_filtered', P(U), int(U.stride(0)), B, P(items), 2 if suffix else kind, kind if suffix else 0,
         int(items.stride(0)), N, D, int(K), P(uid), us, P(off), P(hidx), int(nu), P(fid), fs, P(bits), fld, F,
         int(splits), P(w), int(nbytes), P(idx), P(val), K, stream())
    return idx, val


def ivf_workspace(B, nprobe, nlist, K):
    """(bytes, layout) of the cluster-pruned search's workspace (rs_ivf_ws_bytes, host only):
    layout = [work-item bound, then the byte offsets of the candidate words, the work items, the
    grouped pairs, the cursors, the pair offsets, the work-item offsets, and the bytes]."""
    import ctypes
    lay = (ctypes.c_int64 * 8)()
    nbytes = _hip.lib().rs_ivf_ws_bytes(int(B), int(nprobe), int(nlist), int(K), ctypes.addressof(lay))
    return int(nbytes), [int(v) for v in lay]


def ivf_topk(U, rows_sorted, perm, list_off, centroids, K, nprobe, user_ids=None, history=None, item_exp=None,
             filter_ids=None, filters=None):
    """Cluster-pruned top-K (csrc/ivf.hip): fused_topk's result restricted, per user, to the
    catalog columns of the nprobe lists whose centroids score highest against the user. U [B, D]
    fp32; rows_sorted [N, D] (fp32, bf16 or float8_e4m3fn with item_exp) the item rows sorted by
    list, row r = catalog column perm[r] (int32 [N], ascending inside a list), list l = rows
    [list_off[l], list_off[l + 1]) (int32 [nlist + 1]); centroids fp32 [nlist, D]. The coarse step
    is fused_topk(U, centroids, nprobe). user_ids / history / filter_ids / filters as fused_topk's,
    on catalog columns. -> (cols int32 [B, K], val fp32 [B, K]): masked score descending, ties by
    the lower catalog column, only entries above -inf; the rest (-1, -inf). The coarse
    step and the three stages (rs_ivf_group / rs_ivf_scan / rs_ivf_merge) run on the current stream
    with no host synchronisation. No CPU fallback."""
    use_hist = history is not None and user_ids is not None
    for t in (U, rows_sorted, perm, list_off, centroids) + ((user_ids,) + tuple(history[:2]) if use_hist else ()):
        _hip.require_device(t)
    suffix, kind = _item_kind('ivf_topk', rows_sorted, item_exp)
    U = U.float()
    if U.stride(1) != 1 or U.stride(0) % 4 or U.data_ptr() % 16:
        U = U.contiguous()
    items = rows_sorted
    if items.stride(1) != 1 or (items.stride(0) * items.element_size()) % 16 or items.data_ptr() % 16:
        items = items.contiguous()
    B, D = int(U.shape[0]), int(U.shape[1])
    N, nlist = int(items.shape[0]), int(centroids.shape[0])
    K, nprobe = int(K), int(nprobe)
    if perm.dtype != torch.int32 or list_off.dtype != torch.int32 or perm.numel() != N or list_off.numel() != nlist + 1:
        raise ValueError(f'ivf_topk: perm int32 [N = {N}] and list_off int32 [nlist + 1 = {nlist + 1}], got '
                         f'{perm.dtype} {tuple(perm.shape)} and {list_off.dtype} {tuple(list_off.shape)}')
    if centroids.dim() != 2 or int(centroids.shape[1]) != D or centroids.dtype != torch.float32:
        raise ValueError(f'ivf_topk: centroids fp32 [nlist, D = {D}], got {centroids.dtype} {tuple(centroids.shape)}')
    if not 1 <= nprobe <= min(nlist, 256):
        raise ValueError(f'ivf_topk: nprobe = {nprobe}, must be in [1, min(nlist = {nlist}, 256)]')
    cols = torch.empty(B, K, device=U.device, dtype=torch.int32)
    val = torch.empty(B, K, device=U.device, dtype=torch.float32)
    if B == 0:
        return cols, val
    probe, _ = fused_topk(U, centroids, nprobe)
    nbytes, _ = ivf_workspace(B, nprobe, nlist, K)
    w = ws(nbytes, U.device)
    uid, us, off, hidx, nu = None, 0, None, None, 0
    if use_hist:
        uid = user_ids if user_ids.dtype == torch.int64 else user_ids.long()
        us = int(uid.stride(0))
        off, hidx, nu = history
    fid, fs, bits, fld, F = None, 0, None, 0, 0
    if filter_ids is not None:
        fid, fs, bits, fld, F = _filter_args('ivf_topk', filter_ids, filters, B, N)
    st = stream()
    call('rs_ivf_group', P(probe), nprobe, B, nprobe, nlist, K, P(w), nbytes, st)
    call('rs_ivf_scan', P(U), int(U.stride(0)), B, P(items), 2 if suffix else kind, kind if suffix else 0,
         int(items.stride(0)), N, D, K, P(perm), P(list_off), nlist, nprobe, P(uid), us, P(off), P(hidx), int(nu),
         P(fid), fs, P(bits), fld, F, P(w), nbytes, st)
    call('rs_ivf_merge', B, nprobe, nlist, K, P(w), nbytes, P(cols), P(val), K, st)
    return cols, val


def sample_negatives(cand, cand_val, item_ids, pos_ids, skip, window, n, seed=0, draw=0):
    """n catalog columns per user drawn uniformly without replacement from a window of ranks of
    fused_topk's order (rs_sample_negatives; include/rsys_hip.h has the definition). cand int32 and
    cand_val fp32 [B, C <= 256]: fused_topk's result; item_ids int64 [N]; pos_ids integer [B] or
    None: the item id a user never gets. The pool is the eligible candidates (value above -inf, id
    not the positive's) at eligible positions [skip, skip + window), slid towards the top only as
    far as needed to hold n. -> (ids int64 [B, n], cols int32 [B, n], count int32 [B]): count < n
    where the pool had fewer than n members (its members repeat cyclically; ids and cols -1 at
    count 0). A pure function of (seed, draw) and the candidates. No CPU fallback."""
    for t in (cand, cand_val, item_ids) + ((pos_ids,) if pos_ids is not None else ()):
        _hip.require_device(t)
    if cand.dim() != 2 or cand.dtype != torch.int32 or cand_val.dtype != torch.float32 or cand_val.shape != cand.shape:
        raise ValueError(f'sample_negatives: cand int32 and cand_val float32 of one shape [B, C], got {cand.dtype} '
                         f'{tuple(cand.shape)} and {cand_val.dtype} {tuple(cand_val.shape)}')
    if cand.stride(1) != 1:
        cand = cand.contiguous()
    if cand_val.stride(1) != 1 or cand_val.stride(0) != cand.stride(0):
        cand_val = cand_val.contiguous()
        cand = cand.contiguous()
    B, C = int(cand.shape[0]), int(cand.shape[1])
    ids = item_ids.reshape(-1)
    if ids.dtype != torch.int64 or ids.stride(0) != 1:
        ids = ids.long().contiguous()
    pos, ps = None, 0
    if pos_ids is not None:
        pos = pos_ids.reshape(-1)
        if pos.numel() != B:
            raise ValueError(f'sample_negatives: {pos.numel()} positive ids for {B} users')
        if pos.dtype != torch.int64:
            pos = pos.long()
        ps = int(pos.stride(0))
    n = int(n)
    out_ids = torch.empty(B, max(n, 0), device=cand.device, dtype=torch.int64)
    out_cols = torch.empty(B, max(n, 0), device=cand.device, dtype=torch.int32)
    count = torch.empty(B, device=cand.device, dtype=torch.int32)
    if B == 0:
        return out_ids, out_cols, count
    call('rs_sample_negatives', P(cand), P(cand_val), int(cand.stride(0)) if B > 1 else C, B, C, P(ids),
         int(ids.numel()), P(pos), ps, int(skip), int(window), n, int(seed) & (2 ** 64 - 1), int(draw) & (2 ** 64 - 1),
         P(out_ids), P(out_cols), n, P(count), stream())
    return out_ids, out_cols, count


def target_rank(U, items, target_cols, user_ids=None, history=None, splits=0, item_exp=None, filter_ids=None,
                filters=None):
    """For every user the 0-based position of catalog column target_cols[b] in fused_topk's order
    over the whole catalog (rs_target_rank): the number of columns with a higher masked score, or
    an equal one and a lower column. rank < K exactly when the target is among the user's top K,
    for any K. U, items, item_exp, user_ids and history as fused_topk's (history applies to the target too);
    target_cols integer [B], a column outside [0, N) ranks -1. filter_ids / filters as fused_topk's
    (rs_target_rank_filtered): a target outside the user's filter ranks behind every allowed
    column. -> int32 [B]. No CPU fallback."""
    use_hist = history is not None and user_ids is not None
    for t in (U, items, target_cols) + ((user_ids,) + tuple(history[:2]) if use_hist else ()):
        _hip.require_device(t)
    suffix, kind = _item_kind('target_rank', items, item_exp)
    U = U.float()
    if U.stride(1) != 1 or U.stride(0) % 4 or U.data_ptr() % 16:
        U = U.contiguous()
    if items.stride(1) != 1 or (items.stride(0) * items.element_size()) % 16 or items.data_ptr() % 16:
        items = items.contiguous()
    B, D = int(U.shape[0]), int(U.shape[1])
    N = int(items.shape[0])
    tc = target_cols.reshape(-1)
    if tc.numel() != B:
        raise ValueError(f'target_rank: {tc.numel()} target columns for {B} users')
    if tc.dtype != torch.int32:
        # an id beyond int32 is no column of a catalog with N < 2^31: keep it out of range
        tc = tc.long().clamp(-1, N).int()
    L = _hip.lib()
    if splits <= 0:
        splits = L.rs_target_rank_splits(B, N, D)
    nbytes = L.rs_target_rank_ws_bytes(B, N, D, splits) if splits > 1 else 0
    w = ws(nbytes, U.device) if splits > 1 else None
    out = torch.empty(B, device=U.device, dtype=torch.int32)
    if B == 0:
        return out
    uid, us, off, hidx, nu = None, 0, None, None, 0
    if use_hist:
        uid = user_ids if user_ids.dtype == torch.int64 else user_ids.long()
        us = int(uid.stride(0))
        off, hidx, nu = history
    if filter_ids is None:
        call('rs_target_rank' + suffix, P(U), int(U.stride(0)), B, P(items), kind,
             int(items.stride(0)), N, D, P(tc), int(tc.stride(0)), P(uid), us, P(off), P(hidx), int(nu),
             int(splits), P(w), int(nbytes), P(out), stream())
        return out
    fid, fs, bits, fld, F = _filter_args('target_rank', filter_ids, filters, B, N)
    call('rs_target_rank_filtered', P(U), int(U.stride(0)), B, P(items), 2 if suffix else kind, kind if suffix else 0,
         int(items.stride(0)), N, D, P(tc), int(tc.stride(0)), P(uid), us, P(off), P(hidx), int(nu), P(fid), fs,
         P(bits), fld, F, int(splits), P(w), int(nbytes), P(out), stream())
    return out


def rescore_rows(U, items, cand, cand_val=None):
    """out[b, j] = fp32 dot of U[b] with items[cand[b, j]] (rs_rescore_rows); -inf where cand_val is
    -inf. U, items fp32 [., D]; cand int32 [B, C]."""
    for t in (U, items, cand) + ((cand_val,) if cand_val is not None else ()):
        _hip.require_device(t)
    U, items, cand = U.contiguous(), items.contiguous(), cand.contiguous()
    B, D = int(U.shape[0]), int(U.shape[1])
    Cn = int(cand.shape[1])
    cv = cand_val.contiguous() if cand_val is not None else None
    out = torch.empty(B, Cn, device=U.device, dtype=torch.float32)
    call('rs_rescore_rows', P(U), D, B, P(items), int(items.stride(0)), int(items.shape[0]), D, P(cand), P(cv),
         Cn, Cn, P(out), Cn, stream())
    return out
