"""bf16-class CPU reference of the encoder's opt-in matrix modes (TEST INFRASTRUCTURE ONLY).

rca_codec_set_mfma_mode(1 / 3) runs the encoder's strided layers and conv_out on the bf16 matrix instruction.  This module
restates that arithmetic plainly, in float64, layer by layer, so the tests can check every stored activation of the HIP
pipeline against it (tests/test_codec_bf16_gpu.py).  Read off the kernels in csrc/rca_codec.hip (conv_pack_bf16x2,
conv_split8, pack_weights_bf16, conv_in_blk_kernel, conv_bf16_blk_kernel, conv1d_mfma_kernel's BF path):

  * operands: both the activation and the weight of a product are bf16.  Mode 1 rounds an f32 value to nearest even
    (v_cvt_pk_bf16_f32 on the device, `rne` in pack_weights_bf16 on the host); mode 3 splits it into hi = rne(v) and
    lo = rne(v - hi) (v - hi is exact in f32) and keeps three products hi*hi + hi*lo + lo*hi, dropping lo*lo.
    Mode 0 here means "no rounding": f32 operands, the f32 path's value class.
  * accumulation: f32, starting at the f32 bias.  A bf16 x bf16 product is exact in f32; only the order of the sums is
    the matrix pipe's own.  `conv_layer` returns the exact (f64) sum and, for tolerances, sum |x * w| + |b|.
  * store: the f32 accumulator, LeakyReLU in f32 as max(v, slope * v) when the next layer is pre-activated, then
    rounded (mode 1) or split (mode 3).  The last layer (conv_out) is stored as f32.
  * conv_in (Cin = 1) is never on the matrix pipe: an f32 fma chain in every mode, the value the mode-0 tap 0 holds.

Geometry as oracle/codec_ref.py: zero padding padL = (k - s + 1) // 2, padR = (k - s) // 2, pre-activation on `pre` layers.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Tuple

import numpy as np
import torch
import torch.nn.functional as F

Operand = Tuple[np.ndarray, Optional[np.ndarray]]   # (hi, lo): uint16 bf16 bits (modes 1 / 3) or f32 values (mode 0, lo None)


def rne_bf16(x) -> np.ndarray:
    """f32 -> bf16 bits, round to nearest, ties to even (the bit trick of pack_weights_bf16; finite inputs)."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    return ((u + np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1))) >> np.uint32(16)).astype(np.uint16)


def trunc_bf16(x) -> np.ndarray:
    """f32 -> bf16 bits by truncation (not what any kernel does: the tests' mutation of rne_bf16)."""
    return (np.ascontiguousarray(x, dtype=np.float32).view(np.uint32) >> np.uint32(16)).astype(np.uint16)


def bf16_to_f32(h) -> np.ndarray:
    return (np.ascontiguousarray(h, dtype=np.uint16).astype(np.uint32) << np.uint32(16)).view(np.float32)


def split_bf16(x) -> Tuple[np.ndarray, np.ndarray]:
    """f32 -> (hi, lo) bf16 bits, hi = rne(x), lo = rne(x - hi): conv_pack_bf16x2 / conv_split8 / pack_weights_bf16."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    hi = rne_bf16(x)
    return hi, rne_bf16(x - bf16_to_f32(hi))


def operand(x_f32, mode: int, rnd=rne_bf16) -> Operand:
    """The bf16 operand(s) of an f32 value in `mode` (0: the f32 value itself)."""
    x = np.ascontiguousarray(x_f32, dtype=np.float32)
    if mode == 0:
        return x, None
    hi = rnd(x)
    if mode == 1:
        return hi, None
    return hi, rnd(x - bf16_to_f32(hi))


def leaky_f32(v, slope: float) -> np.ndarray:
    """LeakyReLU as the kernels compute it: max(v, slope * v) in f32."""
    v = np.asarray(v, dtype=np.float32)
    return np.maximum(v, (v * np.float32(slope)).astype(np.float32))


def store(v, act: bool, mode: int, slope: float) -> Operand:
    """What a layer stores for the next one: its f32 value, LeakyReLU in f32 when `act`, then rounded / split."""
    a = np.asarray(v, dtype=np.float64).astype(np.float32)
    if act:
        a = leaky_f32(a, slope)
    return operand(a, mode)


def _value(plane) -> Optional[np.ndarray]:
    """f64 value of one plane: bf16 bits (uint16) or f32 values; None stays None."""
    if plane is None:
        return None
    return (bf16_to_f32(plane) if plane.dtype == np.uint16 else plane).astype(np.float64)


def operand_value(op: Operand) -> np.ndarray:
    """f64 value an operand stands for (hi + lo)."""
    hi, lo = (_value(p) for p in op)
    return hi if lo is None else hi + lo


def encoder_specs(cfg, weights: Dict[str, np.ndarray]) -> List[dict]:
    """cfg.encoder_layers() with their f32 weight [cout, cin, k] and bias [cout]."""
    out = []
    for spec in cfg.encoder_layers():
        d = dict(spec)
        d["w"] = np.ascontiguousarray(weights[spec["name"] + ".weight"], dtype=np.float32)
        d["b"] = np.ascontiguousarray(weights[spec["name"] + ".bias"], dtype=np.float32)
        out.append(d)
    return out


def _conv(x: np.ndarray, w: np.ndarray, k: int, s: int) -> torch.Tensor:
    xt = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64))
    xt = F.pad(xt, ((k - s + 1) // 2, (k - s) // 2))
    return F.conv1d(xt, torch.from_numpy(np.ascontiguousarray(w, dtype=np.float64)), stride=s)


def conv_layer(x_op: Operand, layer: dict, mode: int, w_op: Optional[Operand] = None) -> Tuple[np.ndarray, np.ndarray]:
    """One conv layer on bf16 operands: (r, absum), f64 [B, cout, Lout].

    r is the exact value of the layer's f32 output before any rounding: the products of the bf16 operands (mode 3: hi*hi +
    hi*lo + lo*hi, no lo*lo) plus the bias.  absum = sum |x * w| + |b| over the same products.  x_op: the stored input
    (pre-activation already applied, as the kernels stage it); w_op: the weight operand, default operand(layer w, mode);
    an operand whose lo is None has no lo products."""
    k, s = layer["k"], layer["s"]
    if w_op is None:
        w_op = operand(layer["w"], mode)
    xh, xl = (_value(p) for p in x_op)
    wh, wl = (_value(p) for p in w_op)
    # hi * (hi + lo) + lo * hi: every product exact in f64 (8 x <= 24 significant bits)
    r = _conv(xh, wh + wl if wl is not None else wh, k, s)
    if xl is not None:
        r = r + _conv(xl, wh, k, s)
    xa = np.abs(xh + xl) if xl is not None else np.abs(xh)
    wa = np.abs(wh + wl) if wl is not None else np.abs(wh)
    b = torch.from_numpy(layer["b"].astype(np.float64))[None, :, None]
    return (r + b).numpy(), (_conv(xa, wa, k, s) + b.abs()).numpy()


def products_per_output(layer: dict) -> int:
    return layer["cin"] * layer["k"]


def encode(pcm: np.ndarray, cfg, weights: Dict[str, np.ndarray], mode: int) -> List[np.ndarray]:
    """The whole encoder chained through this reference: pcm [B, T] -> the f64 output r of every layer (before its store).
    conv_in runs on f32 operands in every mode (no kernel puts it on the matrix pipe).  mode 0 is the f32 encoder of
    oracle/codec_ref.py (up to summation order)."""
    hop = cfg.hop
    x = np.asarray(pcm, dtype=np.float32)
    x = np.pad(x, ((0, 0), (0, (-x.shape[1]) % hop)))[:, None, :]
    specs = encoder_specs(cfg, weights)
    outs = []
    op: Operand = (x, None)
    for li, layer in enumerate(specs):
        m = 0 if li == 0 else mode
        r, _ = conv_layer(op, layer, m)
        outs.append(r)
        if li + 1 < len(specs):
            op = store(r, specs[li + 1]["pre"], mode, cfg.leaky_slope)
    return outs
