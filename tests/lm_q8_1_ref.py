"""Host restatement of the LM's q8_1 activation mode (TEST INFRASTRUCTURE ONLY), shared by test_lm_q8_1_cpu.py / test_lm_q8_1_gpu.py.

activation_format="q8_1" (rca_lm_set_act_format, include/rca.h) cuts an activation row into blocks of 32 consecutive values and
quantises each like this project quantises q8_0 weights (oracle/q8_ref.py): d = amax / 127, inv = d != 0 ? 1 / d : 0,
q = roundf(x * inv), scale used = (float)(fp16 of d) -- ggml's quantize_row_q8_1 restated from the published algorithm (ggml is not
part of this tree: parity with llama.cpp's own bits is NOT pinned).  The decode GEMVs then take integer dot products against the
quantised weights.  Here: the quantiser, the three integer product forms in float64 with the magnitude sum a rounding bound needs,
the five GEMV stages of a decode step built from them, an LMRef whose projections see fake-quantised activations, and inputs on
which the device's quantiser provably takes the same decisions as this one.
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import lm_ref, q4k_ref, q8_ref  # noqa: E402

U = 2.0 ** -24          # unit roundoff of f32

# ---- guards of a PRE-NORM input (the stages whose prologue is the RMSNorm: QKV, gate/up, head; K = hidden <= 2048, NIT = 1).
# The reference normalises in float64, the kernel in f32:
#   sum of squares: a lane's fma chain over its 8 * NIT values, 6 adds of the wave reduction, 3 adds across the waves
#       -> depth 8 * NIT + 9 = 17, relative error of a sum of non-negative terms <= 17 u
#   tot / K, + eps: 2 more roundings; rsqrtf: documented 1 ulp = 2 u (and it HALVES the error of its argument, which is not used here:
#       the full 19 u are kept); (v * rstd) * w: 2 roundings                       -> eps_n = (17 + 2 + 2 + 2) u = 23 u per value
#   t = x * inv with inv = 1 / (amax / 127): amax carries eps_n too, the two divisions and the product round once each
#       -> |t_dev - t_ref| <= |t| (2 eps_n + 3 u) <= 127 * 49 u = 3.7e-4
# GUARD_T is 5 times that: no t of a guarded input is closer to a rounding boundary (n + 1/2).  The scale the kernel uses is the
# fp16 rounding of d = amax / 127, whose relative error is eps_n + u = 24 u: GUARD_D is 5 times that, relative to d, from the
# midpoint of two fp16 neighbours.  Inside the guards the device's (q, d) equal the reference's bit for bit.
NORM_EPS_N = 23 * U
GUARD_T = 5 * 127 * (2 * NORM_EPS_N + 3 * U)        # 1.85e-3
GUARD_D = 5 * (NORM_EPS_N + U)                      # 7.2e-6
GUARD_PASSES = 40


# ------------------------------------------------------------------------------------------------------------------ quantiser
def _t_values(x: np.ndarray):
    """float32 [..., K] -> (t = x * inv float32 [..., K / 32, 32], d float32 [..., K / 32]) by the f32 operations of the rule"""
    x = np.ascontiguousarray(x, dtype=np.float32)
    blk = x.reshape(*x.shape[:-1], x.shape[-1] // 32, 32)
    amax = np.abs(blk).max(axis=-1)
    d = (amax / np.float32(127.0)).astype(np.float32)
    with np.errstate(divide="ignore"):
        inv = np.where(d != 0, np.float32(1.0) / np.where(d != 0, d, np.float32(1.0)), np.float32(0.0)).astype(np.float32)
    return (blk * inv[..., None]).astype(np.float32), d


def quantize_q8_1(x: np.ndarray):
    """float32 [..., K] (K % 32 == 0) -> (q int8 [..., K], d float16 [..., K / 32]); roundf = ties away from zero, evaluated exactly"""
    t, d = _t_values(x)
    t64 = t.astype(np.float64)
    q = (np.sign(t64) * np.floor(np.abs(t64) + 0.5)).astype(np.int8)
    with np.errstate(over="ignore"):
        return q.reshape(np.shape(x)), d.astype(np.float16)


def fake_quant_q8_1(x: np.ndarray) -> np.ndarray:
    """the values the integer products stand for: q * (float)(fp16 d), float32 (exact: 8 + 11 bits)"""
    q, d = quantize_q8_1(x)
    return (q.reshape(*d.shape, 32).astype(np.float32) * d.astype(np.float32)[..., None]).reshape(np.shape(x))


# ------------------------------------------------------------------------------------------------------------------ weights
class QMat:
    """A quantised matrix [N, K] as the integer forms read it.
    q8_0: q int8, s float32 [N, K / 32] = fp16 d.   q6_k: q int8 (-32 .. 31), s float32 [N, K / 16] = d * scale (exact in f32).
    q4_k: q uint8 (0 .. 15), s float32 [N, K / 32] = d * sc, m float32 [N, K / 32] = dmin * m (both exact in f32)."""

    def __init__(self, fmt, q, s, m=None):
        self.fmt, self.q, self.s, self.m = fmt, q, s, m
        self.N, self.K = q.shape

    @staticmethod
    def from_f32(w: np.ndarray, fmt: str) -> "QMat":
        """quantised with this build's rules, as weight_format=fmt does on the device"""
        if w.dtype == np.uint16:
            w = (w.astype(np.uint32) << 16).view(np.float32)
        if fmt == "q8_0":
            q, d = q8_ref.quantize_q8_0(w)
            return QMat(fmt, q, d.astype(np.float32))
        if fmt == "q4_k":
            p = q4k_ref.quantize_q4_k(w)
            d, dmin = p["d"].astype(np.float32).repeat(8, axis=-1), p["dmin"].astype(np.float32).repeat(8, axis=-1)
            return QMat(fmt, p["q"], (d * p["sc"].astype(np.float32)).astype(np.float32), (dmin * p["m"].astype(np.float32)).astype(np.float32))
        if fmt == "q6_k":
            p = q4k_ref.quantize_q6_k(w)
            return QMat(fmt, p["q"], (p["d"].astype(np.float32).repeat(16, axis=-1) * p["sc"].astype(np.float32)).astype(np.float32))
        raise ValueError(fmt)

    @staticmethod
    def from_blocks(b) -> "QMat":
        """a GGUF tensor kept as raw blocks (realtime_codec_agent_amd._native.Q8Blocks / Q4KBlocks / Q6KBlocks)"""
        N, K = b.shape
        kind = type(b).__name__
        if kind == "Q8Blocks":
            blk = b.raw.reshape(-1, 34)
            return QMat("q8_0", blk[:, 2:].copy().view(np.int8).reshape(N, K), blk[:, :2].copy().view(np.float16).astype(np.float32).reshape(N, K // 32))
        if kind == "Q4KBlocks":
            blk = b.raw.reshape(-1, 144)
            d = blk[:, 0:2].copy().view(np.float16).astype(np.float32)
            dmin = blk[:, 2:4].copy().view(np.float16).astype(np.float32)
            sc, m = q4k_ref.unpack_scales(blk[:, 4:16])
            qs = blk[:, 16:144].reshape(-1, 4, 32)
            q = np.stack([qs & 0xF, qs >> 4], axis=2).reshape(N, K)
            return QMat("q4_k", q, (d * sc.astype(np.float32)).astype(np.float32).reshape(N, K // 32), (dmin * m.astype(np.float32)).astype(np.float32).reshape(N, K // 32))
        if kind == "Q6KBlocks":
            blk = b.raw.reshape(-1, 210)
            nb = blk.shape[0]
            ql, qh = blk[:, 0:128].reshape(nb, 2, 64), blk[:, 128:192].reshape(nb, 2, 32)
            sc = blk[:, 192:208].copy().view(np.int8).astype(np.float32)
            d = blk[:, 208:210].copy().view(np.float16).astype(np.float32)
            q = np.empty((nb, 2, 4, 32), np.int16)
            q[:, :, 0] = (ql[:, :, 0:32] & 0xF) | (((qh >> 0) & 3) << 4)
            q[:, :, 1] = (ql[:, :, 32:64] & 0xF) | (((qh >> 2) & 3) << 4)
            q[:, :, 2] = (ql[:, :, 0:32] >> 4) | (((qh >> 4) & 3) << 4)
            q[:, :, 3] = (ql[:, :, 32:64] >> 4) | (((qh >> 6) & 3) << 4)
            return QMat("q6_k", (q.reshape(N, K) - 32).astype(np.int8), (d * sc).astype(np.float32).reshape(N, K // 16))
        raise TypeError(kind)

    def dequantize(self) -> np.ndarray:
        """float32 values by the formats' de-quantisation rules (what LMRef multiplies)"""
        g = self.K // self.s.shape[1]
        v = (self.s.repeat(g, axis=1) * self.q.astype(np.float32)).astype(np.float32)
        if self.fmt == "q4_k":
            v = (v - self.m.repeat(32, axis=1)).astype(np.float32)
        return v


def gemv_q8_1(W: QMat, x: np.ndarray):
    """The integer forms of the three formats in float64.  x float32 [M, K] -> (y [M, N], mag [M, N]): per block b of 32
        q8_0  (d_w d_x) sum q_w q_x        q6_k  d_x (s_w0 sum_first16 q_w q_x + s_w1 sum_second16 q_w q_x)
        q4_k  d_x ((d sc_b) sum q_w q_x - (dmin m_b) sum q_x)
    evaluated per 8-value chunk (a lane's share; all of a chunk's values share their scales, so the chunk sums add up to exactly the
    block terms above).  mag = sum over chunks of |term| (q4_k: of both of its terms): what the f32 rounding bound scales with."""
    q, d = quantize_q8_1(x)
    M, K = q.shape
    nc = K // 8
    xq = q.reshape(M, nc, 8).astype(np.float64).transpose(1, 2, 0)                 # [nc, 8, M]
    wq = W.q.reshape(W.N, nc, 8).astype(np.float64).transpose(1, 0, 2)             # [nc, N, 8]
    P = np.matmul(wq, xq)                                                          # [nc, N, M] exact integers
    dx = d.astype(np.float64).repeat(4, axis=1).T[:, None, :]                      # [nc, 1, M]
    sw = W.s.astype(np.float64).repeat((W.K // W.s.shape[1]) // 8, axis=1).T[:, :, None]     # [nc, N, 1]: the scale of the chunk's group
    term = sw * dx * P
    y, mag = term.sum(axis=0), np.abs(term).sum(axis=0)
    if W.fmt == "q4_k":
        S = xq.sum(axis=1)[:, None, :]                                             # [nc, 1, M]
        tm = W.m.astype(np.float64).repeat(4, axis=1).T[:, :, None] * dx * S
        y, mag = y - tm.sum(axis=0), mag + np.abs(tm).sum(axis=0)
    return y.T, mag.T


# ------------------------------------------------------------------------------------------------------------------ the five stages
def gemv_ops(K: int) -> int:
    """f32 roundings on the path of one chunk term to the stage's sum (lm_gemv_kernel, ACT = 1): the product of the two scales (or
    d_x * sum q_x) 1; the lane's fma chain, one fma per chunk and term kind: <= 2 * NIT; wave_reduce_transposed 2 + 4 adds; the three
    adds across the waves."""
    nit = -(-(-(-(K // 8) // 4)) // 64)
    nit = 4 if nit == 3 else nit
    return 1 + 2 * nit + 6 + 3


def gemv_bound(K: int, mag: np.ndarray) -> np.ndarray:
    n = gemv_ops(K)
    return n * U / (1 - n * U) * mag


def rms_norm64(x: np.ndarray, w: np.ndarray, eps: float) -> np.ndarray:
    x = x.astype(np.float64)
    return (x / np.sqrt((x * x).mean(axis=-1, keepdims=True) + eps) * w.astype(np.float64)).astype(np.float32)


class StageRef:
    """The GEMV stages of a decode pass over QMat matrices: kind 0 QKV (+ RoPE, K / V rows), 1 O, 2 gate/up (+ SwiGLU), 3 down, 4 head.
    mats: HF name -> QMat; norms: HF name -> float32 vector."""

    def __init__(self, cfg, mats, norms):
        self.cfg, self.mats, self.norms = cfg, mats, norms
        self.inv_freq = lm_ref.inv_freq(cfg).numpy()

    def run(self, kind: int, layer: int, x: np.ndarray, pos0: int = 0):
        """x float32 [M, K] (the stage's input: the residual for 0 / 2 / 4) -> dict(y, bound [, k, v, k_bound, v_bound]) in float64"""
        c, p = self.cfg, f"model.layers.{layer}."
        if kind == 1:
            y, mag = gemv_q8_1(self.mats[p + "self_attn.o_proj.weight"], x)
            return dict(y=y, bound=gemv_bound(x.shape[1], mag))
        if kind == 3:
            y, mag = gemv_q8_1(self.mats[p + "mlp.down_proj.weight"], x)
            return dict(y=y, bound=gemv_bound(x.shape[1], mag))
        K = x.shape[1]
        if kind == 4:
            y, mag = gemv_q8_1(self.mats["lm_head.weight"], rms_norm64(x, self.norms["model.norm.weight"], c.rms_eps))
            return dict(y=y, bound=gemv_bound(K, mag))
        if kind == 2:
            h = rms_norm64(x, self.norms[p + "post_attention_layernorm.weight"], c.rms_eps)
            g, gm = gemv_q8_1(self.mats[p + "mlp.gate_proj.weight"], h)
            u, um = gemv_q8_1(self.mats[p + "mlp.up_proj.weight"], h)
            dg, du = gemv_bound(K, gm), gemv_bound(K, um)
            sg = 1.0 / (1.0 + np.exp(-g))
            y = g * sg * u
            # epilogue (g / (1 + __expf(-g))) * u: the argument -g * log2(e) rounds once and the constant once more (1.5 u, times |g| ln 2
            # * log2 e = |g| in the exponential), v_exp_f32 1 ulp = 2 u, the add 1 u, the division <= 4 u, the product 1 u; the error of
            # 1 + e is at most that of e.  d silu / dg lies in [-0.1, 1.1].
            eps_epi = (1.5 * np.abs(g) + 8) * U
            return dict(y=y, bound=1.1 * np.abs(u) * dg + np.abs(g * sg) * du + eps_epi * np.abs(y) + dg * du)
        h = rms_norm64(x, self.norms[p + "input_layernorm.weight"], c.rms_eps)
        out = {}
        M = x.shape[0]
        pos = pos0 + np.arange(M)
        ang = (pos[:, None].astype(np.float32) * self.inv_freq[None, :].astype(np.float32)).astype(np.float32).astype(np.float64)   # the table's f32 angle
        cs, sn = np.cos(ang)[:, None, :], np.sin(ang)[:, None, :]                  # [M, 1, 32]
        for name, key, nh in (("q", "self_attn.q_proj.weight", c.n_heads), ("k", "self_attn.k_proj.weight", c.n_kv_heads), ("v", "self_attn.v_proj.weight", c.n_kv_heads)):
            y, mag = gemv_q8_1(self.mats[p + key], h)
            b = gemv_bound(K, mag)
            if name != "v":
                y, b = y.reshape(M, nh, 2, 32), b.reshape(M, nh, 2, 32)
                x1, x2, b1, b2 = y[:, :, 0], y[:, :, 1], b[:, :, 0], b[:, :, 1]
                o1, o2 = x1 * cs - x2 * sn, x2 * cs + x1 * sn
                # o = x1 * c + (+-x2) * s in f32 without contraction: two products and an add, each within u of its result; the table
                # entries cosf / sinf of the f32 angle are within 2 u (1 ulp) of the exact values taken here; a library-derived
                # inv_freq (double pow, rounded once) may sit a few f32 ulp from lm_ref's float32 pow chain: 4 ulp moves the angle by
                # <= 8 u * angle, cos and sin by no more
                tab = 8 * U * ang[:, None, :] * (np.abs(x1) + np.abs(x2))
                r = 4 * U * (np.abs(x1 * cs) + np.abs(x2 * sn)) + np.abs(cs) * b1 + np.abs(sn) * b2 + tab
                r2 = 4 * U * (np.abs(x2 * cs) + np.abs(x1 * sn)) + np.abs(cs) * b2 + np.abs(sn) * b1 + tab
                y, b = np.stack([o1, o2], axis=2).reshape(M, nh * 64), np.stack([r, r2], axis=2).reshape(M, nh * 64)
            out[name], out[name + "_bound"] = y, b
        return dict(y=out["q"], bound=out["q_bound"], k=out["k"], k_bound=out["k_bound"], v=out["v"], v_bound=out["v_bound"])


def fp16_within_one_ulp(got16: np.ndarray, want64: np.ndarray, bound64: np.ndarray) -> np.ndarray:
    """K / V rows: the device rounds its f32 value (within `bound64` of want64) to fp16.  True where got16 is the fp16 rounding of
    some value in [want - bound, want + bound], or one fp16 ulp from it."""
    lo = (want64 - bound64).astype(np.float16)
    hi = (want64 + bound64).astype(np.float16)
    lo = np.nextafter(lo, np.float16(-np.inf))
    hi = np.nextafter(hi, np.float16(np.inf))
    return (got16 >= lo) & (got16 <= hi)


class LazyMats:
    """HF name -> QMat over a state dict, built on first use (a test touches one layer; quantising a whole model costs seconds).
    Values that are raw GGUF blocks are taken as they are; float / bf16-bit matrices are quantised with this build's rule for `fmt`
    (what weight_format=fmt does at load)."""

    def __init__(self, weights: dict, fmt: str = None):
        self.weights, self.fmt, self.done = weights, fmt, {}

    def __getitem__(self, k) -> QMat:
        if k not in self.done:
            v = self.weights[k]
            self.done[k] = QMat.from_blocks(v) if hasattr(v, "raw") else QMat.from_f32(v, self.fmt)
        return self.done[k]


def model_norms(weights: dict) -> dict:
    return {k: np.asarray(v, np.float32) for k, v in weights.items() if k.endswith("norm.weight") or k.endswith("layernorm.weight")}


# ------------------------------------------------------------------------------------------------------------------ inputs
def _violations(x, pre_norm):
    h = rms_norm64(x, *pre_norm) if pre_norm is not None else np.ascontiguousarray(x, np.float32)
    t, d = _t_values(h)
    frac = np.abs(t.astype(np.float64)) % 1.0
    bad_t = (np.abs(frac - 0.5) < GUARD_T).reshape(x.shape)
    d64 = d.astype(np.float64)
    with np.errstate(over="ignore"):
        f = d.astype(np.float16)
        lo, hi = np.nextafter(f, np.float16(-np.inf)).astype(np.float64), np.nextafter(f, np.float16(np.inf)).astype(np.float64)
    f = f.astype(np.float64)
    near = np.minimum(np.abs(d64 - (f + lo) / 2), np.abs(d64 - (f + hi) / 2))
    bad_d = (near < GUARD_D * d64) & (d64 > 0)
    return bad_t, bad_d, h


def guarded_input(rng, shape, pre_norm=None, scale=1.0):
    """Rows [M, K] of normal values on which the device's quantiser takes the reference's decisions: after the float64 RMSNorm
    (pre_norm = (norm weights, eps)) or directly (None) no t = x * inv is within GUARD_T of a rounding boundary and no d = amax / 127
    within GUARD_D (relative) of an fp16 midpoint.  Offending elements (for d: the block's largest) are nudged by up to 2 %;
    a nudge moves the row's norm and with it every other t a little, hence the passes.  Returns (x float32, passes used)."""
    x = (rng.standard_normal(shape) * scale).astype(np.float32)
    for n in range(1, GUARD_PASSES + 1):
        bad_t, bad_d, h = _violations(x, pre_norm)
        if not bad_t.any() and not bad_d.any():
            return x, n
        blk = np.abs(h).reshape(*h.shape[:-1], -1, 32)
        top = (blk == blk.max(axis=-1, keepdims=True)) & bad_d[..., None]
        bad = bad_t | top.reshape(x.shape)
        x = np.where(bad, x * (1 + rng.uniform(0.002, 0.02, x.shape) * rng.choice([-1.0, 1.0], x.shape)), x).astype(np.float32)
    raise AssertionError(f"guarded_input: guards not reached in {GUARD_PASSES} passes for shape {shape}")


def planted_input(rng, shape, scale=1.0):
    """Rows for the stages WITHOUT a norm (O, down): the device quantises the very f32 values the reference does, so no guard is
    needed; instead the first blocks of every row are edge cases of the rule -- exact ties (amax = 127 * 2^e, values (n + 1/2) * 2^e
    of both signs: t is exactly n + 1/2), an all-zero block, a block whose largest magnitude is negative, a block so small that the
    fp16 scale is subnormal."""
    x = (rng.standard_normal(shape) * scale).astype(np.float32)
    assert shape[-1] >= 160
    for r in range(shape[0]):
        e = np.float32(2.0 ** (-3 - r))
        n = rng.integers(0, 126, 31).astype(np.float32) + np.float32(0.5)
        x[r, 0] = np.float32(127.0) * e
        x[r, 1:32] = n * e * rng.choice([-1.0, 1.0], 31).astype(np.float32)
        x[r, 32:64] = 0.0
        x[r, 64:96] = (rng.uniform(-0.5, 0.5, 32) * scale).astype(np.float32)
        x[r, 64 + 5] = np.float32(-0.75 * scale)
        x[r, 96:128] = (rng.standard_normal(32) * 1e-4).astype(np.float32)       # amax ~ 3e-4 -> d ~ 2.4e-6 < 6.1e-5: subnormal fp16
        e2 = np.float32(2.0 ** -6)
        x[r, 128] = np.float32(-127.0) * e2                                       # ties again, amax carried by a negative value
        x[r, 129:160] = (rng.integers(0, 126, 31).astype(np.float32) + np.float32(0.5)) * e2 * rng.choice([-1.0, 1.0], 31).astype(np.float32)
    return x


# ------------------------------------------------------------------------------------------------------------------ whole model
class LMRefQ81(lm_ref.LMRef):
    """LMRef whose projections and head multiply FAKE-QUANTISED activations (q * fp16 d: the values the integer products stand for).
    `q81 = False` turns that off for evals the device runs on its MFMA prefill tiles, which keep f32 activations: the eval is then
    LMRef's, bit for bit.  f64=True evaluates every product, norm and softmax in float64; the quantiser still decides on the float32
    rounding of its input, as the rule is stated in f32 -- the difference to the f32 evaluation is the reference's own noise, and where
    one activation lands on the other side of a rounding boundary, a flip that cascades through the later quantisers."""

    q81 = True

    def __init__(self, cfg, weights, kv_dtype=torch.float16, f64=False):
        super().__init__(cfg, weights, kv_dtype)
        if f64:
            self.w = {k: v.double() for k, v in self.w.items()}

    def _fq(self, h: torch.Tensor) -> torch.Tensor:
        return torch.from_numpy(fake_quant_q8_1(h.float().numpy())).to(h.dtype) if self.q81 else h

    def _eval(self, ids, last_only, drop_keys) -> torch.Tensor:
        if drop_keys is not None:
            raise NotImplementedError("LMRefQ81 does not mask keys (drop_keys)")
        c = self.cfg
        ids = torch.as_tensor(list(ids), dtype=torch.long)
        S = ids.shape[0]
        pos = torch.arange(self.n_tokens, self.n_tokens + S)
        freqs = pos[:, None].float() * self.inv_freq[None, :]
        emb = torch.cat((freqs, freqs), dim=-1)
        x = self.w["model.embed_tokens.weight"][ids]
        cos, sin = emb.cos()[None].to(x.dtype), emb.sin()[None].to(x.dtype)
        G = c.n_heads // c.n_kv_heads
        for l in range(c.n_layers):
            p = f"model.layers.{l}."
            h = self._fq(self._norm(x, self.w[p + "input_layernorm.weight"]))
            q = (h @ self.w[p + "self_attn.q_proj.weight"].T).view(S, c.n_heads, c.head_dim).transpose(0, 1)
            k = (h @ self.w[p + "self_attn.k_proj.weight"].T).view(S, c.n_kv_heads, c.head_dim).transpose(0, 1)
            v = (h @ self.w[p + "self_attn.v_proj.weight"].T).view(S, c.n_kv_heads, c.head_dim).transpose(0, 1)
            q = q * cos + lm_ref._rotate_half(q) * sin
            k = k * cos + lm_ref._rotate_half(k) * sin
            if self.kv_dtype is not None:
                k, v = k.to(self.kv_dtype).to(x.dtype), v.to(self.kv_dtype).to(x.dtype)
            if self.k[l] is not None and self.n_tokens > 0:
                k = torch.cat((self.k[l][:, : self.n_tokens], k), dim=1)
                v = torch.cat((self.v[l][:, : self.n_tokens], v), dim=1)
            self.k[l], self.v[l] = k, v
            T = k.shape[1]
            qg = q.reshape(c.n_kv_heads, G * S, c.head_dim)
            att = (qg @ k.transpose(1, 2)) * (c.head_dim ** -0.5)
            mask = torch.arange(T)[None, :] > (self.n_tokens + torch.arange(S))[:, None]
            att = att.view(c.n_kv_heads, G, S, T).masked_fill(mask[None, None], float("-inf")).softmax(-1).view(c.n_kv_heads, G * S, T)
            o = (att @ v).view(c.n_heads, S, c.head_dim).transpose(0, 1).reshape(S, c.n_heads * c.head_dim)
            x = x + self._fq(o.contiguous()) @ self.w[p + "self_attn.o_proj.weight"].T
            h = self._fq(self._norm(x, self.w[p + "post_attention_layernorm.weight"]))
            g = h @ self.w[p + "mlp.gate_proj.weight"].T
            u = h @ self.w[p + "mlp.up_proj.weight"].T
            x = x + self._fq(torch.nn.functional.silu(g) * u) @ self.w[p + "mlp.down_proj.weight"].T
        if last_only:
            x = x[-1:]
        x = self._fq(self._norm(x, self.w["model.norm.weight"]))
        self.n_tokens += S
        return x @ self.w["lm_head.weight"].T


# ------------------------------------------------------------------------------------------------------------------ the cases
INIT_STD = 0.05
# name -> (vocab, hidden, heads, kv heads, ffn, weight format, seed): 2-layer random-init models, RoPE without frequency scaling
#   h192:  K = 192 / 320 = 24 / 40 chunks: 6 / 10 chunks per wave on the f32 path, so a 32-block would straddle two waves
#   h768:  K = 3 x 256 (Q4_K super-blocks, not a power of two), G = 4 row pairing in the QKV epilogue
#   h1024: ffn 6144 = the NIT = 4 instance of the down projection with a short last chunk
TAP_MODELS = {
    "h192_q8_0": (1000, 192, 3, 3, 320, "q8_0", 32),
    "h768_q8_0": (1536, 768, 12, 3, 768, "q8_0", 39),
    "h768_q4_k": (1536, 768, 12, 3, 768, "q4_k", 39),
    "h1024_q8_0": (2048, 1024, 16, 16, 6144, "q8_0", 37),
    "h1024_q4_k": (2048, 1024, 16, 16, 6144, "q4_k", 37),
}
GGUF_MODEL = dict(vocab_size=1024, hidden=256, n_layers=2, n_heads=4, n_kv_heads=2, ffn=512, seed=5)   # Q4_K_M: layer 1 has Q6_K attn_v / ffn_down
STAGE_WIDTHS = lambda c: {0: c.hidden, 1: c.n_heads * 64, 2: c.hidden, 3: c.ffn, 4: c.hidden}            # noqa: E731
WHOLE_CASES = ("h192_q8_0", "h768_q4_k")
WHOLE_PROMPT, WHOLE_STEPS = 40, 8
# max |LMRefQ81 - LMRef| over the logits of the 40-token prompt's last position and of the 8 decode steps after it, in units of
# max(1, |logit|max): the size of the mode's effect, measured with this file on the CPU (test_lm_q8_1_cpu.py re-measures it)
EFFECT = {"h192_q8_0": 1.54e-2, "h768_q4_k": 2.74e-2}


def tap_config(name: str):
    from realtime_codec_agent_amd.llm import LMConfig
    v, h, nh, nkv, f, _, _ = TAP_MODELS[name]
    return LMConfig(vocab_size=v, hidden=h, n_layers=2, n_heads=nh, n_kv_heads=nkv, head_dim=64, ffn=f, rope_scaling=None, rope_theta=10000.0)


def tap_weights(name: str) -> dict:
    """the bf16-bit state dict rca_lm_create_random generates for the case"""
    return lm_ref.random_weights(tap_config(name), TAP_MODELS[name][6], INIT_STD)


def whole_ids(name: str) -> np.ndarray:
    return np.random.default_rng(700 + TAP_MODELS[name][6]).integers(0, TAP_MODELS[name][0], WHOLE_PROMPT + WHOLE_STEPS).astype(np.int64)


def whole_model_logits(ref, ids) -> np.ndarray:
    """[1 + WHOLE_STEPS, V]: the prompt's last logits, then one row per single-token decode step"""
    ref.reset()
    rows = [ref.eval(ids[:WHOLE_PROMPT], last_only=True)[-1].numpy()]
    for t in ids[WHOLE_PROMPT:]:
        rows.append(ref.eval([int(t)])[-1].numpy())
    return np.stack(rows)


def dequantized_weights(name: str) -> dict:
    w, fmt = tap_weights(name), TAP_MODELS[name][5]
    return (q8_ref if fmt == "q8_0" else q4k_ref).quantized_model(w)
