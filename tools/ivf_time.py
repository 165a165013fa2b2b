"""Time the cluster-pruned (IVF) search (retrieval.IvfIndex, csrc/ivf.hip) stage by stage against
the exhaustive sweep it restricts, on seeded inputs, with device events (retrieval_time.py's
`timed`): a warm-up of every path, then alternating rounds (every second one in reverse order),
per path the best time and the spread.

Per data set, item dtype and batch size:
  search   base.search(U, K): the existing exhaustive kernel, the yardstick
  coarse   ops.fused_topk(U, centroids, nprobe)
  group    rs_ivf_group, scan rs_ivf_scan, merge rs_ivf_merge, each alone on the stored output of
           the stage before it
  ivf      IvfIndex.search(U, K, nprobe), everything together
  Recall@K of the IVF lists against the exhaustive lists, the workspace bytes, the list-length
  spread (the longest list bounds one work item's sweep) and the item bytes the scan requests per
  second of its own time (every work item reads its whole list; many hit L2).

Data sets: 'mixture' = a normalised mixture of `nlist` Gaussians, each row its centre plus noise
of norm about --noise (the clustering helps the index), users likewise around catalog rows;
'iid' = normalised iid Gaussian rows and users (the worst case).

Without --step the tool runs every (data set, dtype) as a child process of its own under
`timeout`, stops at the first that fails, and writes the table to --out.

    python tools/ivf_time.py [--n 1048576] [--d 64] [--nlist 1024] [--batches 4096,256]
        [--nprobes 1,4,16,64] [--ks 10,100] [--dtypes bf16,fp8] [--data mixture,iid] [--out FILE]
"""
import argparse
import os
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from recommendsystemproject_amd import _hip, ops  # noqa: E402
from recommendsystemproject_amd.retrieval import ItemIndex, IvfIndex  # noqa: E402
from retrieval_time import timed  # noqa: E402

ITEM_BYTES = {'bf16': 2, 'fp8': 1, 'fp32': 4}


def make_rows(kind, N, D, nlist, dev, g, noise):
    if kind == 'iid':
        return torch.nn.functional.normalize(torch.randn(N, D, device=dev, generator=g), dim=1)
    centres = torch.nn.functional.normalize(torch.randn(nlist, D, device=dev, generator=g), dim=1)
    which = torch.randint(0, nlist, (N,), device=dev, generator=g)
    return torch.nn.functional.normalize(centres[which] + noise / D ** 0.5 * torch.randn(N, D, device=dev, generator=g),
                                      dim=1)


def make_users(kind, rows, B, dev, g, noise):
    """Users near catalog rows for the mixture (a trained tower's users sit where items are), iid otherwise."""
    D = rows.shape[1]
    if kind == 'iid':
        return torch.nn.functional.normalize(torch.randn(B, D, device=dev, generator=g), dim=1)
    pick = torch.randint(0, rows.shape[0], (B,), device=dev, generator=g)
    return torch.nn.functional.normalize(rows[pick] + noise / D ** 0.5 * torch.randn(B, D, device=dev, generator=g), dim=1)


def recall(got, want):
    hit = (got.unsqueeze(2) == want.unsqueeze(1)).any(dim=2) & (got >= 0)
    return float(hit.sum().item()) / want.numel()


def run_step(a, kind, dtype):
    dev = torch.device('cuda:0')
    _hip.require_device(torch.empty(1, device=dev))
    N, D, nlist = a.n, a.d, a.nlist
    g = torch.Generator(device=dev).manual_seed(0)
    X = make_rows(kind, N, D, nlist, dev, g, a.noise)
    base = ItemIndex.from_embeddings(X, dtype=dtype)
    ivf = IvfIndex.build(base, nlist, iters=a.iters, seed=0)
    lens = (ivf.list_off[1:] - ivf.list_off[:-1]).float()
    lines = [f'{kind}{f" (noise {a.noise})" if kind == "mixture" else ""} {dtype}: N = {N}, D = {D}, nlist = {nlist}, k-means iters = {a.iters}; list length mean '
             f'{lens.mean().item():.0f}, max {int(lens.max().item())}, min {int(lens.min().item())}, empty '
             f'{int((lens == 0).sum().item())}']
    print(lines[0], flush=True)
    st = ops.stream
    for B in [int(x) for x in a.batches.split(',')]:
        U = make_users(kind, X, B, dev, g, a.noise)
        iters = 5 if B > 256 else 20
        for K in [int(x) for x in a.ks.split(',')]:
            want = base.search(U, K)[2]
            paths = [(f'search K={K}', lambda K=K: base.search(U, K), iters)]
            info = {}
            for nprobe in [int(x) for x in a.nprobes.split(',')]:
                nbytes, lay = ops.ivf_workspace(B, nprobe, nlist, K)
                w = ops.ws(nbytes, dev)
                probe = ops.fused_topk(U, ivf.centroids, nprobe)[0]
                cols = torch.empty(B, K, device=dev, dtype=torch.int32)
                val = torch.empty(B, K, device=dev, dtype=torch.float32)
                rows = ivf.rows_sorted
                kind_arg, exp = (2, base.scale_exp) if dtype == 'fp8' else (int(dtype == 'bf16'), 0)

                def group(probe=probe, nprobe=nprobe, w=w, nbytes=nbytes):
                    _hip.call('rs_ivf_group', probe.data_ptr(), nprobe, B, nprobe, nlist, K, w.data_ptr(), nbytes, st())

                def scan(nprobe=nprobe, w=w, nbytes=nbytes):
                    _hip.call('rs_ivf_scan', U.data_ptr(), D, B, rows.data_ptr(), kind_arg, exp, D, N, D, K,
                              ivf.perm.data_ptr(), ivf.list_off.data_ptr(), nlist, nprobe, None, 0, None, None, 0,
                              None, 0, None, 0, 0, w.data_ptr(), nbytes, st())

                def merge(nprobe=nprobe, w=w, nbytes=nbytes, cols=cols, val=val):
                    _hip.call('rs_ivf_merge', B, nprobe, nlist, K, w.data_ptr(), nbytes, cols.data_ptr(), val.data_ptr(),
                              K, st())

                tag = f'K={K} nprobe={nprobe}'
                paths += [(f'coarse {tag}', lambda nprobe=nprobe: ops.fused_topk(U, ivf.centroids, nprobe), iters),
                          (f'group {tag}', group, iters), (f'scan {tag}', scan, iters), (f'merge {tag}', merge, iters),
                          (f'ivf {tag}', lambda nprobe=nprobe: ivf.search(U, K, nprobe), iters)]
                got = ivf.search(U, K, nprobe)[2]
                swept = float(lens[probe.long().reshape(-1)].sum().item())    # rows requested by all pairs
                info[tag] = (recall(got, want), nbytes, swept)
            for _, fn, _ in paths:      # warm-up of every path (group before scan before merge)
                fn()
            torch.cuda.synchronize()
            times = {name: [] for name, _, _ in paths}
            for r in range(a.rounds):
                for name, fn, it in (paths if r % 2 == 0 else paths[::-1]):
                    times[name].append(timed(fn, it))
            s = min(times[f'search K={K}'])
            sp = max(times[f'search K={K}']) - s
            lines.append(f'  B={B:<5d} K={K:<4d} search (exhaustive) best {s:9.4f} ms  spread {sp:7.4f}')
            for tag, (rec, nbytes, swept) in info.items():
                t = {k: min(times[f'{k} {tag}']) for k in ('coarse', 'group', 'scan', 'merge', 'ivf')}
                spread = max(times[f'ivf {tag}']) - t['ivf']
                gbs = swept * D * ITEM_BYTES[dtype] / (t['scan'] * 1e-3) / 1e9
                lines.append(f'    {tag:18s} coarse {t["coarse"]:8.4f} group {t["group"]:8.4f} scan {t["scan"]:9.4f} '
                             f'merge {t["merge"]:8.4f} | ivf {t["ivf"]:9.4f} (spread {spread:7.4f}) = x{t["ivf"] / s:6.3f} of '
                             f'search | recall@{K} {rec:6.4f} | ws {nbytes / 2 ** 20:8.1f} MiB | scan requests '
                             f'{gbs:8.1f} GB/s of item rows')
            print('\n'.join(lines[-(len(info) + 1):]), flush=True)
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=1 << 20)
    ap.add_argument('--d', type=int, default=64)
    ap.add_argument('--nlist', type=int, default=1024)
    ap.add_argument('--iters', type=int, default=8)
    ap.add_argument('--batches', default='4096,256')
    ap.add_argument('--nprobes', default='1,4,16,64')
    ap.add_argument('--ks', default='10,100')
    ap.add_argument('--dtypes', default='bf16,fp8')
    ap.add_argument('--data', default='mixture,iid')
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--noise', type=float, default=0.5, help='mixture: the norm of a row\'s offset from its centre')
    ap.add_argument('--step-timeout', type=int, default=240)
    ap.add_argument('--step', default=None, help='internal: one "data:dtype" in this process, table to stdout')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'r21_ivf_time.txt'))
    a = ap.parse_args()
    if a.step:
        kind, dtype = a.step.split(':')
        run_step(a, kind, dtype)
        return 0
    head = ('cluster-pruned (IVF) search against the exhaustive sweep; ms per call (device events), best of '
            f'{a.rounds} alternating rounds after a warm-up (the second in reverse order); every (data set, dtype) in '
            'a process of its own')
    out = [head]
    passthrough = [x for x in sys.argv[1:]]
    for kind in a.data.split(','):
        for dtype in a.dtypes.split(','):
            cmd = ['timeout', '-k', '10', str(a.step_timeout), sys.executable, os.path.abspath(__file__)] + passthrough + \
                  ['--step', f'{kind}:{dtype}']
            p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
            print(p.stdout + (p.stderr if p.returncode else ''), flush=True)
            out.append(p.stdout.rstrip())
            if p.returncode != 0:       # nothing more on the device after a failure
                out.append(f'{kind} {dtype}: FAILED, exit status {p.returncode}; stopped here')
                break
        else:
            continue
        break
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write('\n'.join(out) + '\n')
    return 1 if 'FAILED' in out[-1] else 0


if __name__ == '__main__':
    sys.exit(main())
