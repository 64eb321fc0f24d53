"""Host restatement of the context shift on a q8_0 KV cache (TEST INFRASTRUCTURE ONLY: rca_lm_set_kv_shift_requant + rca_lm_kv_remove,
include/rca.h), shared by tests/test_kv_q8_shift_cpu.py, tests/test_kv_q8_shift_gpu.py and tests/kv_q8_shift_spread.py.

CONTRACT.  V blocks move bit for bit.  A moved K head row (q, d16) becomes

    x = dequant(q, d16)                     fp16, the row attention stages                      (kv_q8_ref.dequant)
    e = R_-delta(x)                         the rotation of tests/kv_shift_ref.py, float64: pair (j, j + 32), angle = f32(delta) * f32
                                            inv_freq[j] as the table forms it, cos / sin and the products in float64
    y = fp16_rne(e)                         the row an fp16 cache holding x would hold after its own shift
    (q', d16') = quant_rows(y)              the cache's quantiser                                (kv_q8_ref.quant_rows)

BOUND (shift_bound) on |dequant(device blocks) - e| per element, e from the device's own pre-shift blocks.  Term by term:
  1. rotation.  The device forms y in f32 and rounds once to fp16: |y_dev - e| <= rot = ulp16(e) / 2 + (|x1| + |x2|) * 2^-21 -- the
     bound of tests/test_kv_shift_gpu.py::_check_rotated (three f32 roundings of at most 2^-24 relative on terms of at most |x1| + |x2|,
     cosf / sinf of the table good to about 2^-22 absolute: 3 * 2^-24 + 2^-22 < 2^-21).
  2. quantiser step.  q' = roundf(y / d) with d = amax(y) / 127 moves a value by at most d / 2 = amax(y) / 254, and amax(y) <= A =
     max over the block of (|e| + rot): half = A / 254.
  3. the scale's fp16 rounding.  The stored scale is d16' = fp16_rne(d): relative error 2^-11 while d16' is a normal fp16 number, which
     moves q' d16' by |q' d| * 2^-11, |e| * 2^-11 to first order.  A block whose d is below 2^-14 has a SUBNORMAL (or zero) d16', spaced
     2^-24 whatever d is: there the scale moves by up to 2^-25 and the value by up to |q'| * 2^-25 <= 127 * 2^-25.  (edge_rows classes 3
     and 5 are such blocks: class 3's scale rounds to zero and the whole row de-quantises to 0, an error of |e| itself, which is
     127 d <= 127 * 2^-25.)  Term: |e| * 2^-11, and 127 * 2^-25 in its place where A / 127 < 2^-14.
  4. the de-quantiser's fp16 rounding, fp16_rne(d16' * q'): ulp16(e) / 2, with ulp16 taken at |e| + the three terms above.
The bound is a statement about the number formats and the rule; nothing in it is fitted to a device result."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kv_q8_ref as kr  # noqa: E402
from agent_fakes import OracleLLM  # noqa: E402


def ulp16(e: np.ndarray) -> np.ndarray:
    """spacing of fp16 at |e| (subnormal spacing 2^-24 below 2^-14)"""
    k = np.floor(np.log2(np.maximum(np.abs(e), 2.0 ** -14)))
    return 2.0 ** (k - 10)


def table_inv_freq(cfg) -> np.ndarray:
    """inv_freq as the library derives it for a handle created without a rope.inv_freq tensor (random-init): double arithmetic, rounded
    to f32 once (the derivation tests/test_kv_shift_gpu.py checks the fp16 shift with)"""
    import math
    out = []
    for i in range(32):
        f = 1.0 / math.pow(cfg.rope_theta, (2 * i) / 64.0)
        if cfg.rope_scaling == "llama3":
            low_wl, high_wl = cfg.rope_orig_ctx / cfg.rope_low_freq_factor, cfg.rope_orig_ctx / cfg.rope_high_freq_factor
            wl = 2.0 * math.pi / f
            if wl > low_wl:
                f = f / cfg.rope_factor
            elif wl >= high_wl:
                smooth = (cfg.rope_orig_ctx / wl - cfg.rope_low_freq_factor) / (cfg.rope_high_freq_factor - cfg.rope_low_freq_factor)
                f = (1.0 - smooth) * f / cfg.rope_factor + smooth * f
        out.append(f)
    return np.asarray(out, np.float64).astype(np.float32)


def rotate_f64(x: np.ndarray, delta: int, inv_freq: np.ndarray, sign: float = 1.0):
    """x: fp16 [..., 64] -> (e float64 [..., 64], mag = |x1| + |x2| repeated to 64); sign = -1 rotates the other way (a mutant)"""
    ang = (np.float32(delta) * np.asarray(inv_freq, np.float32)).astype(np.float32).astype(np.float64)
    c, s = np.cos(ang), sign * np.sin(ang)
    x1, x2 = x[..., :32].astype(np.float64), x[..., 32:].astype(np.float64)
    e = np.concatenate((x1 * c + x2 * s, x2 * c - x1 * s), axis=-1)
    mag = np.abs(x1) + np.abs(x2)
    return e, np.concatenate((mag, mag), axis=-1)


def rotated_rows(k_q, k_d16, delta, inv_freq) -> np.ndarray:
    """y of the contract: the fp16 rows whose quantisation the new blocks are"""
    e, _ = rotate_f64(kr.dequant(k_q, k_d16), delta, inv_freq)
    return e.astype(np.float16)


def shift_rows_ref(k_q, k_d16, delta, inv_freq):
    """K blocks (int8 [..., 64], fp16 [..., 2]) of rows that move by -delta positions -> their new blocks, by the contract"""
    return kr.quant_rows(rotated_rows(k_q, k_d16, delta, inv_freq))


def shift_bound(k_q, k_d16, delta, inv_freq):
    """(e, bound): the float64 rotation of the de-quantised old rows and the per-element bound on |dequant(new blocks) - e|"""
    e, mag = rotate_f64(kr.dequant(k_q, k_d16), delta, inv_freq)
    rot = ulp16(e) / 2 + mag * 2.0 ** -21
    wide = np.abs(e) + rot
    A = wide.reshape(*wide.shape[:-1], 2, 32).max(-1, keepdims=True)
    A = np.broadcast_to(A, (*wide.shape[:-1], 2, 32)).reshape(wide.shape)
    half = A / 254.0
    scale = np.where(A / 127.0 < 2.0 ** -14, 127.0 * 2.0 ** -25, np.abs(e) * 2.0 ** -11)
    deq = ulp16(np.abs(e) + rot + half + scale) / 2
    return e, rot + half + scale + deq


def worst_ratio(new_q, new_d16, old_q, old_d16, delta, inv_freq) -> float:
    e, bound = shift_bound(old_q, old_d16, delta, inv_freq)
    got = kr.dequant(new_q, new_d16).astype(np.float64)
    return float((np.abs(got - e) / bound).max())


# ------------------------------------------------------------------ mutants (what the bound has to catch; test_kv_q8_shift_cpu.py)
def mutant_swapped_scales(k_q, k_d16, delta, inv_freq):
    return shift_rows_ref(k_q, np.ascontiguousarray(k_d16[..., ::-1]), delta, inv_freq)


def mutant_wrong_sign(k_q, k_d16, delta, inv_freq):
    e, _ = rotate_f64(kr.dequant(k_q, k_d16), delta, inv_freq, sign=-1.0)
    return kr.quant_rows(e.astype(np.float16))


def mutant_one_amax(k_q, k_d16, delta, inv_freq):
    """one amax over the 64 values of the head row: both blocks get the scale of the larger"""
    y = rotated_rows(k_q, k_d16, delta, inv_freq).astype(np.float32)
    d = np.abs(y).max(-1, keepdims=True) / np.float32(127.0)
    with np.errstate(divide="ignore"):
        inv = np.where(d != 0, np.float32(1.0) / d, np.float32(0.0)).astype(np.float32)
    t = y * inv
    q = (np.sign(t) * np.floor(np.abs(t) + np.float32(0.5))).astype(np.int8)
    return q, np.broadcast_to(d.astype(np.float16), (*y.shape[:-1], 2)).copy()


# ------------------------------------------------------------------ inputs of the planted-row tests (CPU conditions and GPU test)
def planted_rows(rng, n_pos: int, nkv: int) -> np.ndarray:
    """fp16 K rows [n_pos, nkv, 64]: N(0, 1) rows, then from position 8 on in turns N(0, 30) rows, kv_q8_ref.edge_rows without class 2
    (65504 de-quantises to infinity: no non-finite value goes into a shifted K row), and "lopsided" rows -- the last eight RoPE pairs
    (the slowest frequencies) carry N(0, 1) in block 0 and N(0, 1) / 64 in block 1, every other element is zero -- whose two blocks keep
    scales a factor of ten and more apart after a rotation by a few positions: what one amax over the head row gets wrong."""
    x = rng.standard_normal((n_pos, nkv, 64)).astype(np.float16)
    edge = kr.edge_rows(rng, 6, nkv)[[0, 1, 3, 4, 5]]
    for p in range(8, n_pos):
        kind = (p - 8) % 16
        if kind < 5:
            x[p] = edge[kind]
        elif kind < 9:
            x[p] = (rng.standard_normal((nkv, 64)) * 30).astype(np.float16)
        elif kind < 12:
            row = np.zeros((nkv, 64), np.float32)
            row[:, 24:32] = rng.standard_normal((nkv, 8))
            row[:, 56:64] = rng.standard_normal((nkv, 8)) / 64
            x[p] = row.astype(np.float16)
    return x


# ------------------------------------------------------------------ the oracle with the same shift
def kv_remove_q8_ref(ref, p0: int, p1: int, jitter=None) -> None:
    """kv_shift_ref.kv_remove_ref on a Q8KVRef (whose cache holds de-quantised fp16 values): cut [p0, p1), rotate the kept tail's keys
    in float64, round once to fp16, fake-quantise; V moved as it is.  jitter: a numpy Generator moves the rotated fp16 rows by
    -1 / 0 / +1 ulp ahead of the quantiser (tests/kv_q8_shift_spread.py)."""
    n = ref.n_tokens
    assert 0 <= p0 <= p1 <= n, (p0, p1, n)
    delta = p1 - p0
    inv_freq = ref.inv_freq.numpy()
    for l in range(ref.cfg.n_layers):
        if ref.k[l] is None:
            continue
        k, v = ref.k[l][:, :n], ref.v[l][:, :n]
        if delta and p1 < n:
            e, _ = rotate_f64(k[:, p1:].numpy().astype(np.float16), delta, inv_freq)
            y = e.astype(np.float16)
            if jitter is not None:
                y = kr.ulp_jitter(y, jitter)
            k = torch.cat((k[:, :p0], torch.from_numpy(kr.fake_quant(y).astype(np.float32))), dim=1)
        else:
            k = torch.cat((k[:, :p0], k[:, p1:]), dim=1)
        ref.k[l], ref.v[l] = k, torch.cat((v[:, :p0], v[:, p1:]), dim=1)
    ref.n_tokens = n - delta


class Q8ShiftOracleLLM(OracleLLM):
    """OracleLLM over Q8KVRef (the q8_0 cache's oracle) with the kv_remove of a q8_0 HIP LM object that may shift"""

    kv_format = "q8_0"
    kv_shift_requant = True

    def __init__(self, cfg, weights, n_ctx=4096):
        super().__init__(cfg, weights, n_ctx)
        self.ref = kr.Q8KVRef(cfg, weights)

    def kv_remove(self, p0, p1):
        kv_remove_q8_ref(self.ref, int(p0), int(p1))
