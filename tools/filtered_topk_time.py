"""Time the catalog filters of the fused retrieval kernels (ops.fused_topk / ops.target_rank with
filter_ids) on seeded inputs in one process, with device events, retrieval_time.py's protocol: a
warm-up of every path, then alternating rounds (every second one in reverse order, so that no
path always runs behind the same neighbour), per path the times, the best and the spread.

Paths per batch size and item dtype (bf16, e4m3):
  unfiltered        the fused kernel of this tree without a filter
  unfiltered parent the same call into another build of the library (--parent-lib: librsys_hip.so
                    of the parent commit, e.g. built in a `git archive` of it), loaded beside this
                    tree's in the same process so that the rounds alternate
  filtered d, one   one filter of density d for every user
  filtered d, 8 mix 8 filters of density d, mixed across the batch
  staged d, ...     what a caller had before: fp32 ops.gemm per 65,536-column chunk, a torch
                    masked_fill from the bool mask, rs_topk_rows per chunk and a merge (top-K), or
                    the comparison against the gathered target score (rank)
Every filtered result is compared with the staged one on the way (the share of equal rows; bf16 /
e4m3 scores differ from fp32 ones, so this is a sanity figure, not a test).

    python tools/filtered_topk_time.py [--what topk|rank] [--n 1000000] [--d 128] [--k 20]
        [--batches 4096,64] [--densities 1,0.5,0.01,0.0001] [--parent-lib PATH] [--out FILE]
"""
import argparse
import ctypes
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from recommendsystemproject_amd import _hip, ops  # noqa: E402
from retrieval_time import timed  # noqa: E402

CHUNK = 65536
NEG = float('-inf')


def load_parent(path):
    L = ctypes.CDLL(os.path.abspath(path))
    for name in ('rs_fused_topk', 'rs_fused_topk_e4m3', 'rs_target_rank', 'rs_target_rank_e4m3'):
        fn = getattr(L, name)
        fn.restype, fn.argtypes = _hip.SIGNATURES[name]
    return L


def parent_call(L, what, U, items, exp, K, tcols):
    """The unfiltered call as ops.fused_topk / ops.target_rank make it, into library L."""
    B, D = int(U.shape[0]), int(U.shape[1])
    N = int(items.shape[0])
    sfx, kind = ('_e4m3', int(exp)) if exp is not None else ('', int(items.dtype == torch.bfloat16))
    st = ops.stream()
    if what == 'topk':
        s = L.rs_fused_topk_splits(B, N, D, K)
        nb = L.rs_fused_topk_ws_bytes(B, N, D, K, s)
        w = ops.ws(nb, U.device)
        idx = torch.empty(B, K, device=U.device, dtype=torch.int32)
        val = torch.empty(B, K, device=U.device, dtype=torch.float32)
        rc = getattr(L, 'rs_fused_topk' + sfx)(U.data_ptr(), D, B, items.data_ptr(), kind, int(items.stride(0)), N, D,
                                               K, None, 0, None, None, 0, s, w.data_ptr(), nb, idx.data_ptr(),
                                               val.data_ptr(), K, st)
        out = idx
    else:
        s = L.rs_target_rank_splits(B, N, D)
        nb = L.rs_target_rank_ws_bytes(B, N, D, s)
        w = ops.ws(nb, U.device)
        out = torch.empty(B, device=U.device, dtype=torch.int32)
        rc = getattr(L, 'rs_target_rank' + sfx)(U.data_ptr(), D, B, items.data_ptr(), kind, int(items.stride(0)), N,
                                                D, tcols.data_ptr(), 1, None, 0, None, None, 0, s, w.data_ptr(), nb,
                                                out.data_ptr(), st)
    if rc != 0:
        raise RuntimeError(f'parent library call failed (rc={rc})')
    return out


def staged_topk(U, I, K, masks, fid):
    """fp32 GEMM per chunk, masked_fill from the bool masks [F, N], top-K per chunk, merge."""
    B, D = int(U.shape[0]), int(U.shape[1])
    N = int(I.shape[0])
    chunks = [(c0, min(CHUNK, N - c0)) for c0 in range(0, N, CHUNK)]
    C = K * len(chunks)
    cand_i = torch.empty(B, C, device=U.device, dtype=torch.int32)
    cand_v = torch.empty(B, C, device=U.device, dtype=torch.float32)
    S = torch.empty(B * min(CHUNK, N), device=U.device, dtype=torch.float32)
    st = ops.stream()
    for j, (c0, n) in enumerate(chunks):
        Sc = S[:B * n].view(B, n)
        ops.gemm(U, I[c0:c0 + n], Sc, B, n, D, transA=0, transB=1, lda=D, ldb=D, ldc=n)
        m = masks[0, c0:c0 + n].view(1, n) if masks.shape[0] == 1 else masks[:, c0:c0 + n][fid]
        Sc.masked_fill_(~m, NEG)
        _hip.call('rs_topk_rows', Sc.data_ptr(), n, B, n, K, None, 0, c0, cand_i.data_ptr() + 4 * K * j,
                  cand_v.data_ptr() + 4 * K * j, C, st)
    out = torch.empty(B, K, device=U.device, dtype=torch.int32)
    _hip.call('rs_topk_rows', cand_v.data_ptr(), C, B, C, K, cand_i.data_ptr(), C, 0, out.data_ptr(), None, K, st)
    return out


def staged_rank(U, I, tcols, masks, fid):
    """The same chunks compared against the gathered (and equally masked) target score."""
    B, D = int(U.shape[0]), int(U.shape[1])
    N = int(I.shape[0])
    t = tcols.long().view(-1, 1)
    ts = ops.rescore_rows(U, I, tcols.view(-1, 1).contiguous())
    t_ok = masks[0][t] if masks.shape[0] == 1 else masks[fid.view(-1, 1), t]
    ts = ts.masked_fill(~t_ok, NEG)
    count = torch.zeros(B, device=U.device, dtype=torch.int64)
    S = torch.empty(B * min(CHUNK, N), device=U.device, dtype=torch.float32)
    for c0 in range(0, N, CHUNK):
        n = min(CHUNK, N - c0)
        Sc = S[:B * n].view(B, n)
        ops.gemm(U, I[c0:c0 + n], Sc, B, n, D, transA=0, transB=1, lda=D, ldb=D, ldc=n)
        m = masks[0, c0:c0 + n].view(1, n) if masks.shape[0] == 1 else masks[:, c0:c0 + n][fid]
        Sc.masked_fill_(~m, NEG)
        col = torch.arange(c0, c0 + n, device=U.device).view(1, -1)
        ahead = (Sc > ts) | ((Sc == ts) & (col < t))
        count += (ahead & (col != t)).sum(dim=1)
    return count.int()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--what', choices=['topk', 'rank'], default='topk')
    ap.add_argument('--n', type=int, default=1000000)
    ap.add_argument('--d', type=int, default=128)
    ap.add_argument('--k', type=int, default=20)
    ap.add_argument('--batches', default='4096,64')
    ap.add_argument('--densities', default='1,0.5,0.01,0.0001')
    ap.add_argument('--dtypes', default='bf16,fp8')
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--parent-lib', default=None)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out_path = a.out or os.path.join(root, 'profiles', f'r18_filtered_{a.what}_time.txt')
    dev = torch.device('cuda:0')
    _hip.require_device(torch.empty(1, device=dev))
    parent = load_parent(a.parent_lib) if a.parent_lib else None
    N, D, K = a.n, a.d, a.k
    g = torch.Generator(device=dev).manual_seed(0)
    I = torch.nn.functional.normalize(torch.randn(N, D, device=dev, generator=g), dim=1)
    rows = {'bf16': (I.bfloat16(), None), 'fp8': ops.quantize_e4m3(I)}
    dens = [float(x) for x in a.densities.split(',')]
    masks = {}
    for d in dens:      # 8 independent filters per density; "one" uses the first
        m = torch.rand(8, N, device=dev, generator=g) < d
        masks[d] = (m, ops.pack_mask(m))
    what = 'top-K' if a.what == 'topk' else 'target rank'
    lines = [f'catalog filters, fused {what}, N = {N}, D = {D}' + (f', K = {K}' if a.what == 'topk' else '') +
             f'; ms per call (device events), {a.rounds} alternating rounds after warm-up (the second in reverse '
             f'order); the staged paths read fp32 items']
    for B in [int(x) for x in a.batches.split(',')]:
        U = torch.nn.functional.normalize(torch.randn(B, D, device=dev, generator=g), dim=1)
        tcols = torch.randint(0, N, (B,), device=dev, generator=g).int()
        fid1 = torch.zeros(B, device=dev, dtype=torch.int32)
        fid8 = torch.randint(0, 8, (B,), device=dev, generator=g).int()
        many = B > 256

        def fused(items, exp, **flt):
            if a.what == 'topk':
                return ops.fused_topk(U, items, K, item_exp=exp, **flt)[0]
            return ops.target_rank(U, items, tcols, item_exp=exp, **flt)

        def staged(m, fid):
            return staged_topk(U, I, K, m, fid) if a.what == 'topk' else staged_rank(U, I, tcols, m, fid)

        paths = []      # (name, fn, iterations per timing)
        for d in dens:
            m, _ = masks[d]
            paths.append((f'staged   {d:<6g} one', lambda m=m: staged(m[:1], fid1.long()), 1 if many else 4))
            paths.append((f'staged   {d:<6g} 8 mix', lambda m=m: staged(m, fid8.long()), 1 if many else 4))
        for dtype in a.dtypes.split(','):
            items, exp = rows[dtype]
            paths.append((f'{dtype:4s} unfiltered', lambda items=items, exp=exp: fused(items, exp), 10 if many else 20))
            if parent is not None:
                paths.append((f'{dtype:4s} unfiltered parent',
                              lambda items=items, exp=exp: parent_call(parent, a.what, U, items, exp, K, tcols),
                              10 if many else 20))
            for d in dens:
                _, bits = masks[d]
                for label, fid in (('one', fid1), ('8 mix', fid8)):
                    paths.append((f'{dtype:4s} filtered {d:<6g} {label}',
                                  lambda items=items, exp=exp, bits=bits, fid=fid:
                                  fused(items, exp, filter_ids=fid, filters=bits), 10 if many else 20))
        results = {name: fn() for name, fn, _ in paths}      # warm-up of every path, and the results
        torch.cuda.synchronize()
        times = {name: [] for name, _, _ in paths}
        for r in range(a.rounds):      # odd rounds in reverse: no path always follows the same neighbour
            for name, fn, iters in (paths if r % 2 == 0 else paths[::-1]):
                times[name].append(timed(fn, iters))
        L = _hip.lib()
        splits = L.rs_fused_topk_splits(B, N, D, K) if a.what == 'topk' else L.rs_target_rank_splits(B, N, D)
        lines.append(f'B = {B} ({splits} column splits)')
        for name, _, _ in paths:
            t = times[name]
            extra = ''
            parts = name.split()
            if parts[1] == 'filtered':
                ref = 'staged   ' + name.split('filtered ')[1]
                r, s = results[name], results[ref]
                same = float((r == s).all(dim=1).float().mean()) if r.dim() == 2 else float((r == s).float().mean())
                extra = f'  vs staged x{min(times[ref]) / min(t):7.2f}  rows equal to staged {same:.4f}'
                base = min(times[f'{parts[0]:4s} unfiltered'])
                extra += f'  vs unfiltered x{min(t) / base:5.2f}'
            elif parts[-1] == 'parent':
                r, s = results[name], results[f'{parts[0]:4s} unfiltered']
                extra = f'  this tree / parent x{min(times[f"{parts[0]:4s} unfiltered"]) / min(t):5.3f}  ' \
                        f'same result {bool(torch.equal(r, s))}'
            lines.append(f'  {name:28s} {" ".join(f"{x:9.3f}" for x in t)}  best {min(t):9.3f}  spread '
                         f'{max(t) - min(t):7.3f}{extra}')
        print('\n'.join(lines[-len(paths) - 1:]), flush=True)
    text = '\n'.join(lines) + '\n'
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, 'w') as f:
        f.write(text)


if __name__ == '__main__':
    main()
