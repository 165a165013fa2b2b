"""Time top-K retrieval three ways on the same seeded inputs, with device events: the staged
retrieval_topk (fp32 GEMM per 65,536-column chunk -> top-K per chunk -> merge), the fused kernel on
fp32 items, on bf16 items and on e4m3 items (ops.fused_topk; the e4m3 rows from
ops.quantize_e4m3, their scores on the bf16 MFMA). Three alternating rounds after a
warm-up of every path; per path the three times, their spread, and the share of the binding floor
(the dot products at the MFMA peak of the item dtype, or the item matrix read once from HBM,
whichever is larger; the line says which binds). No history.

    python tools/retrieval_time.py [--n 1000000] [--d 128] [--k 20] [--batches 4096,64] [--out FILE]
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from recommendsystemproject_amd import _hip, ops  # noqa: E402
from recommendsystemproject_amd.project.utils.training_utils import retrieval_topk  # noqa: E402

PEAK_TF = {'fp32': 157.3, 'bf16': 2500.0, 'fp8': 2500.0}  # dense MFMA peaks (datasheet), TFLOP/s; e4m3 rows run on the bf16 MFMA
ITEM_BYTES = {'fp32': 4, 'bf16': 2, 'fp8': 1}
PEAK_HBM = 8.0e12                            # bytes/s (datasheet)


def floor_ms(B, N, D, dtype):
    mfma = 2.0 * B * N * D / (PEAK_TF[dtype] * 1e12) * 1e3
    mem = N * D * ITEM_BYTES[dtype] / PEAK_HBM * 1e3
    return (mfma, 'MFMA rate') if mfma >= mem else (mem, 'item-matrix bytes')


def timed(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=1000000)
    ap.add_argument('--d', type=int, default=128)
    ap.add_argument('--k', type=int, default=20)
    ap.add_argument('--batches', default='4096,64')
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--out', default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                  'profiles', 'r8_retrieval_time.txt'))
    a = ap.parse_args()
    dev = torch.device('cuda:0')
    _hip.require_device(torch.empty(1, device=dev))
    g = torch.Generator(device=dev).manual_seed(0)
    I = torch.nn.functional.normalize(torch.randn(a.n, a.d, device=dev, generator=g), dim=1)
    Ib = I.bfloat16()
    Iq, exp = ops.quantize_e4m3(I)
    lines = [f'top-K retrieval, N = {a.n}, D = {a.d}, K = {a.k}, no history; ms per call (device events), '
             f'{a.rounds} alternating rounds after warm-up']
    for B in [int(x) for x in a.batches.split(',')]:
        U = torch.nn.functional.normalize(torch.randn(B, a.d, device=dev, generator=g), dim=1)
        paths = [('staged fp32', 'fp32', lambda: retrieval_topk(U, I, a.k), 2 if B > 256 else 10),
                 ('fused fp32', 'fp32', lambda: ops.fused_topk(U, I, a.k), 5 if B > 256 else 20),
                 ('fused bf16', 'bf16', lambda: ops.fused_topk(U, Ib, a.k), 10 if B > 256 else 20),
                 ('fused fp8', 'fp8', lambda: ops.fused_topk(U, Iq, a.k, item_exp=exp), 10 if B > 256 else 20)]
        staged = retrieval_topk(U, I, a.k)
        f32 = ops.fused_topk(U, I, a.k)[0]
        ops.fused_topk(U, Ib, a.k)
        ops.fused_topk(U, Iq, a.k, item_exp=exp)
        torch.cuda.synchronize()
        same = float((staged == f32).all(dim=1).float().mean())
        times = {name: [] for name, _, _, _ in paths}
        for _ in range(a.rounds):
            for name, _, fn, iters in paths:
                times[name].append(timed(fn, iters))
        splits = _hip.lib().rs_fused_topk_splits(B, a.n, a.d, a.k)
        lines.append(f'B = {B} (fused: {splits} column splits; rows whose fused fp32 list equals the staged one: '
                     f'{same:.4f})')
        base = min(times['staged fp32'])
        for name, dtype, _, _ in paths:
            t = times[name]
            fl, what = floor_ms(B, a.n, a.d, dtype)
            lines.append(f'  {name:12s} {" ".join(f"{x:9.3f}" for x in t)}  best {min(t):9.3f}  spread '
                         f'{max(t) - min(t):7.3f}  floor {fl:7.3f} ({what}) share {fl / min(t):6.1%}  '
                         f'vs staged x{base / min(t):.2f}')
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write(text)


if __name__ == '__main__':
    main()
