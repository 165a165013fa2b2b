"""The CPU emulation of the e4m3 index format that the fp8 tests compare against (never the code
under test): the scale exponent by the format's rule in plain Python, and the quantisation by
torch's float8_e4m3fn cast."""
import math

import numpy as np
import torch


def py_exponent(absmax):
    """The largest e with absmax * 2^e <= 448, clamped to [-40, 40]; 0 for absmax = 0. absmax is
    taken as a float32; frexp gives absmax = m 2^p with m in [0.5, 1), all exact."""
    a = float(np.float32(absmax))
    if a == 0.0:
        return 0
    m, p = math.frexp(a)
    e = 9 - p - (1 if 2.0 * m > 1.75 else 0)
    assert math.ldexp(a, e) <= 448.0 < math.ldexp(a, e + 1)
    return max(-40, min(40, e))


def quantize(x, e=None):
    """x [., D] float32 (numpy or torch) -> (q float8_e4m3fn on the CPU, e): one scale for the
    array unless e is given."""
    t = torch.as_tensor(np.asarray(x, dtype=np.float32)) if not isinstance(x, torch.Tensor) else x.detach().float().cpu()
    if e is None:
        e = py_exponent(float(t.abs().max())) if t.numel() else 0
    return (t * (2.0 ** e)).to(torch.float8_e4m3fn), e


def quantize_rows(x):
    """Each row under its own scale (what the kernel does to the users) -> (q, e [rows])."""
    t = torch.as_tensor(np.asarray(x, dtype=np.float32)) if not isinstance(x, torch.Tensor) else x.detach().float().cpu()
    e = np.array([py_exponent(float(r.abs().max())) for r in t], dtype=np.int64)
    scale = torch.from_numpy(np.exp2(e.astype(np.float64))).float().view(-1, 1)
    return (t * scale).to(torch.float8_e4m3fn), e


def scores64(U, I):
    """The fp64 scores of the format: users and items quantised, dequantised exactly, multiplied
    in float64. -> numpy [B, N]."""
    qu, eu = quantize_rows(U)
    qi, ei = quantize(I)
    du = qu.double() * torch.from_numpy(np.exp2(-eu.astype(np.float64))).view(-1, 1)
    di = qi.double() * (2.0 ** -ei)
    return (du @ di.t()).numpy()
