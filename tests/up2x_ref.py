"""Float64 model of mf_conv_up2x (include/mfhip.h): the 3x3 / padding 1 conv over a nearest-2x upsampled image as four 2x2 convs.

Plain torch float64; never calls a project kernel.  `model` follows the entry's own formula — output pixel (2y + py, 2x + px) reads
the low-resolution window that starts at (y - 1 + py, x - 1 + px), zeros outside the image, times the phase's [n][(ty * 2 + tx) * c0 + c]
weights — and the epilogue in the kernel's order (csrc/gemm_conv_kernel.h epilogue_store8): alpha * (acc + bias) + res0 + res1, SiLU.
S is the sum of |a_k w_k| carried through the epilogue by first-order propagation, as tests/gemm_ref.py defines it."""
from typing import Optional, Tuple

import torch


def model(x: torch.Tensor, w4: torch.Tensor, bias: Optional[torch.Tensor] = None, res0: Optional[torch.Tensor] = None,
          res1: Optional[torch.Tensor] = None, res1_rows: int = 0, alpha: float = 1.0, silu: bool = False) -> Tuple[torch.Tensor, torch.Tensor]:
    """x [B, H, W, C], w4 [4, N, 4 C] (k = (ty * 2 + tx) * C + c), bias [N], res0 / res1 [rows, N] over the output's 4 B H W rows
    (res1 with res1_rows rows is shared: output row m adds row m % res1_rows) -> (out, S) float64 [4 B H W, N] in output row order."""
    x, w4 = x.double(), w4.double()
    b, h, w, c = x.shape
    n = w4.shape[1]
    xp = torch.zeros(b, h + 2, w + 2, c, dtype=torch.float64, device=x.device)
    xp[:, 1:h + 1, 1:w + 1] = x
    out = torch.zeros(b, 2 * h, 2 * w, n, dtype=torch.float64, device=x.device)
    s = torch.zeros_like(out)
    for py in range(2):
        for px in range(2):
            wp = w4[2 * py + px].view(n, 2, 2, c)
            for ty in range(2):
                for tx in range(2):
                    win = xp[:, py + ty: py + ty + h, px + tx: px + tx + w]              # low-resolution pixel (y - 1 + py + ty, x - 1 + px + tx)
                    out[:, py::2, px::2] += win @ wp[:, ty, tx].T
                    s[:, py::2, px::2] += win.abs() @ wp[:, ty, tx].abs().T
    v, s = out.view(-1, n), s.view(-1, n)
    if bias is not None:
        v, s = v + bias.double()[None, :], s + bias.double().abs()[None, :]
    v, s = v * alpha, s * abs(alpha)
    if res0 is not None:
        v, s = v + res0.double().view(-1, n), s + res0.double().abs().view(-1, n)
    if res1 is not None:
        r1 = res1.double().view(-1, n)
        if 0 < res1_rows < v.shape[0]:
            r1 = r1[torch.arange(v.shape[0], device=v.device) % res1_rows]
        v, s = v + r1, s + r1.abs()
    if silu:
        sg = torch.sigmoid(v)
        y = v * sg
        s = (sg * (1.0 + v * (1.0 - sg))).abs() * s + y.abs()
        v = y
    return v, s


def gn_block_rows(batch: int, h: int, w: int, r: int) -> torch.Tensor:
    """[blocks, R] output rows of every partial row the epilogue leaves, in its (image, phase, block of R low-resolution rows) order:
    low-resolution row m = (b h + y) w + x of phase (py, px) is output row 4 m - 2 (m mod w) + 2 w py + px."""
    out = []
    for b in range(batch):
        for p in range(4):
            for blk in range(h * w // r):
                m = b * h * w + blk * r + torch.arange(r)
                out.append(4 * m - 2 * (m % w) + 2 * w * (p >> 1) + (p & 1))
    return torch.stack(out)
