"""Time hard-negative mining (ItemIndex.mine_negatives: the fused sweep for C candidates, then
rs_sample_negatives) against the sweep it is built on, on seeded inputs in one process, with device
events, retrieval_time.py's protocol: a warm-up of every path, then alternating rounds (every
second one in reverse order, so that no path always runs behind the same neighbour), per path the
times, the best and the spread.

Paths per item dtype (bf16, e4m3), batch size, with / without a history and window:
  search   index.search(user_emb, k=C), C = skip + window + 1: the yardstick (code this feature
           does not touch)
  mine     index.mine_negatives(user_emb, n, positives, skip, window): the same sweep + the sampler
  sampler  ops.sample_negatives alone on the stored candidates of that sweep (reads B * C * 12 bytes)

    python tools/mine_time.py [--n 1000000] [--d 128] [--batches 4096,64] [--windows 0:31:10,100:155:10]
        [--hist 200] [--out FILE]
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from recommendsystemproject_amd import _hip, ops  # noqa: E402
from recommendsystemproject_amd.retrieval import ItemIndex  # noqa: E402
from retrieval_time import timed  # noqa: E402


def random_history(users, N, per_user, rng, device):
    """A sorted CSR (off, idx, U) of `per_user` random columns for each of `users` users."""
    cols = np.sort(rng.integers(0, N, (users, per_user)), axis=1)
    keep = np.ones_like(cols, dtype=bool)
    keep[:, 1:] = cols[:, 1:] != cols[:, :-1]
    counts = np.concatenate([[0], keep.sum(axis=1)])
    off = torch.from_numpy(np.cumsum(counts).astype(np.int64)).to(device)
    idx = torch.from_numpy(cols[keep].astype(np.int32)).to(device)
    return off, idx, users


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=1000000)
    ap.add_argument('--d', type=int, default=128)
    ap.add_argument('--batches', default='4096,64')
    ap.add_argument('--windows', default='0:31:10,100:155:10', help='skip:window:n, comma separated')
    ap.add_argument('--dtypes', default='bf16,fp8')
    ap.add_argument('--hist', type=int, default=200, help='history columns a user in the "history" runs')
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out_path = a.out or os.path.join(root, 'profiles', 'r19_mine_time.txt')
    dev = torch.device('cuda:0')
    _hip.require_device(torch.empty(1, device=dev))
    N, D = a.n, a.d
    g = torch.Generator(device=dev).manual_seed(0)
    rng = np.random.default_rng(0)
    I = torch.nn.functional.normalize(torch.randn(N, D, device=dev, generator=g), dim=1)
    windows = [tuple(int(x) for x in w.split(':')) for w in a.windows.split(',')]
    batches = [int(x) for x in a.batches.split(',')]
    lines = [f'hard-negative mining, N = {N}, D = {D}; ms per call (device events), {a.rounds} alternating rounds '
             f'after warm-up (the second in reverse order); search = index.search(k = C), mine = '
             f'index.mine_negatives, sampler = rs_sample_negatives alone on stored candidates']
    for dtype in a.dtypes.split(','):
        index = ItemIndex.from_embeddings(I, dtype=dtype, keep_fp32=False)
        for B in batches:
            U = torch.nn.functional.normalize(torch.randn(B, D, device=dev, generator=g), dim=1)
            pos = torch.randint(0, N, (B,), device=dev, generator=g)
            uid = torch.arange(B, device=dev)
            hist = random_history(B, N, a.hist, rng, dev)
            iters = 5 if B > 256 else 20
            paths = []
            for with_hist in (False, True):
                for skip, window, n in windows:
                    C = min(skip + window + 1, N)
                    users = uid if with_hist else None
                    tag = f'{dtype:4s} B={B:<5d} {"hist" if with_hist else "none"} C={C:<3d} n={n:<3d}'
                    index._history = hist if with_hist else None
                    cand, cval = ops.fused_topk(U, index._rows(), C, users, index._history, item_exp=index.scale_exp)

                    def search(C=C, users=users, h=index._history):
                        index._history = h
                        return index.search(U, C, user_ids=users)

                    def mine(skip=skip, window=window, n=n, users=users, h=index._history):
                        index._history = h
                        return index.mine_negatives(U, n, pos, skip=skip, window=window, user_ids=users, draw=1)

                    def sampler(cand=cand, cval=cval, skip=skip, window=window, n=n):
                        return ops.sample_negatives(cand, cval, index.item_ids, pos, skip, window, n, draw=1)

                    paths += [(tag + ' search', search, iters), (tag + ' mine', mine, iters),
                              (tag + ' sampler', sampler, 50)]
            for _, fn, _ in paths:      # warm-up of every path
                fn()
            torch.cuda.synchronize()
            times = {name: [] for name, _, _ in paths}
            for r in range(a.rounds):   # odd rounds in reverse: no path always follows the same neighbour
                for name, fn, it in (paths if r % 2 == 0 else paths[::-1]):
                    times[name].append(timed(fn, it))
            for name, _, _ in paths:
                t = times[name]
                extra = ''
                base = name.rsplit(' ', 1)[0]
                if not name.endswith('search'):
                    s = times[base + ' search']
                    own = min(t) if name.endswith('sampler') else min(t) - min(s)   # what mining adds to the sweep
                    extra = (f'  / search x{min(t) / min(s):6.4f}  adds {own:8.4f} ms = {own / min(s):7.4f} of search '
                             f'(search spread {max(s) - min(s):.4f} ms)')
                lines.append(f'  {name:44s} {" ".join(f"{x:9.4f}" for x in t)}  best {min(t):9.4f}  spread '
                             f'{max(t) - min(t):7.4f}{extra}')
            print('\n'.join(lines[-len(paths):]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, 'w') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
