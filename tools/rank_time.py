"""Time the fused target-rank kernel (ops.target_rank, rs_target_rank) against the fused top-K
(ops.fused_topk, rs_fused_topk at K = 20) on identical seeded inputs in one process, with device
events: per shape a warm-up of both, then alternating rounds, the median per path and the spread.
The rank kernel does the top-K kernel's loads and MFMAs and none of its list work, so the
expectation to check is rank <= top-K per shape. Shapes: B = 4096; N in {3,706, 1,000,000,
10,000,000}; D in {64, 128}; fp32, bf16 and e4m3 items (--dtypes); without and with a history of about 100 items
per user. Each line also says whether rank < K agreed with membership in the top-K list.

    python tools/rank_time.py [--b 4096] [--ns 3706,1000000,10000000] [--ds 64,128] [--k 20]
                              [--dtypes fp32,bf16,fp8] [--out FILE]
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from recommendsystemproject_amd import _hip, ops  # noqa: E402
from retrieval_time import timed  # noqa: E402


def random_history(B, N, per_user, dev, g):
    """user b -> about per_user distinct random columns, as the sorted CSR of sorted_history_csr."""
    cols, _ = torch.sort(torch.randint(0, N, (B, per_user), device=dev, generator=g), dim=1)
    keep = torch.ones_like(cols, dtype=torch.bool)
    keep[:, 1:] = cols[:, 1:] != cols[:, :-1]
    off = torch.zeros(B + 1, dtype=torch.int64, device=dev)
    off[1:] = keep.sum(dim=1).cumsum(0)
    return off, cols[keep].int().contiguous(), B


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--b', type=int, default=4096)
    ap.add_argument('--ns', default='3706,1000000,10000000')
    ap.add_argument('--ds', default='64,128')
    ap.add_argument('--k', type=int, default=20)
    ap.add_argument('--dtypes', default='fp32,bf16,fp8')
    ap.add_argument('--history', type=int, default=100)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--out', default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                  'profiles', 'r12_rank_time.txt'))
    a = ap.parse_args()
    dev = torch.device('cuda:0')
    _hip.require_device(torch.empty(1, device=dev))
    L = _hip.lib()
    B, K = a.b, a.k
    lines = [f'target rank vs fused top-K (K = {K}), B = {B}; median ms per call (device events) of {a.rounds} '
             f'alternating rounds after warm-up, (spread); history = about {a.history} columns per user']
    lines.append(f'{"N":>9s} {"D":>4s} {"items":>5s} {"hist":>4s}  {"splits r/t":>10s}  {"rank ms":>16s}  '
                 f'{"top-K ms":>16s}  rank/top-K  agree')
    for N in [int(x) for x in a.ns.split(',')]:
        for D in [int(x) for x in a.ds.split(',')]:
            g = torch.Generator(device=dev).manual_seed(N + D)
            I = torch.nn.functional.normalize(torch.randn(N, D, device=dev, generator=g), dim=1)
            U = torch.nn.functional.normalize(torch.randn(B, D, device=dev, generator=g), dim=1)
            tcols = torch.randint(0, N, (B,), device=dev, generator=g).int()
            hist = random_history(B, N, a.history, dev, g)
            uids = torch.arange(B, device=dev)
            for dtype in a.dtypes.split(','):
                exp = None
                if dtype == 'fp8':
                    items, exp = ops.quantize_e4m3(I)
                else:
                    items = I if dtype == 'fp32' else I.bfloat16()
                for with_hist in (False, True):
                    u, h = (uids, hist) if with_hist else (None, None)
                    paths = {'rank': lambda: ops.target_rank(U, items, tcols, u, h, item_exp=exp),
                             'topk': lambda: ops.fused_topk(U, items, K, u, h, item_exp=exp)}
                    rank = paths['rank']()
                    top = paths['topk']()[0]
                    torch.cuda.synchronize()
                    agree = bool(torch.equal((rank >= 0) & (rank < K), (top == tcols.view(-1, 1)).any(dim=1)))
                    iters = {}
                    for name, fn in paths.items():  # about 0.3 s per timing
                        iters[name] = max(2, min(200, int(300.0 / max(timed(fn, 2), 1e-3))))
                    times = {name: [] for name in paths}
                    for _ in range(a.rounds):
                        for name, fn in paths.items():
                            times[name].append(timed(fn, iters[name]))
                    med = {n: statistics.median(t) for n, t in times.items()}
                    spr = {n: max(t) - min(t) for n, t in times.items()}
                    splits = f'{L.rs_target_rank_splits(B, N, D)}/{L.rs_fused_topk_splits(B, N, D, K)}'
                    lines.append(f'{N:9d} {D:4d} {dtype:>5s} {"yes" if with_hist else "no":>4s}  {splits:>10s}  '
                                 f'{med["rank"]:8.3f} ({spr["rank"]:5.3f})  {med["topk"]:8.3f} ({spr["topk"]:5.3f})  '
                                 f'{med["rank"] / med["topk"]:10.2f}  {"yes" if agree else "NO"}')
                    print(lines[-1], flush=True)
            del I, U, items
            torch.cuda.empty_cache()
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write(text)


if __name__ == '__main__':
    main()
