"""GGUF Q5_K on the host (TEST INFRASTRUCTURE ONLY), beside oracle/q4k_ref.py.

A `llama-quantize ... Q5_K_S / Q5_K_M` file is made of Q5_K and Q6_K tensors.  ggml is not part of this tree, so the published
format and de-quantisation rule are restated here (ggml-common.h `block_q5_K`, ggml-quants.c `dequantize_row_q5_K`):

    block_q5_K (176 bytes, 256 weights, GGUF tensor type 13) = { fp16 d; fp16 dmin; uint8 scales[12]; uint8 qh[32]; uint8 qs[128] }
    scales: packed exactly as in Q4_K (get_scale_min_k4, q4k_ref.unpack_scales): a 6-bit scale sc_j and minimum m_j per 32 weights
    for t = 0..3, l = 0..31:  weight 64 t + l      = low nibble of qs[32 t + l]  | bit 2 t     of qh[l] << 4     (sub-block 2 t)
                              weight 64 t + 32 + l = high nibble of qs[32 t + l] | bit 2 t + 1 of qh[l] << 4     (sub-block 2 t + 1)
    value = (d * sc_j) * q - (dmin * m_j)         (f32: two products, one subtraction, in this order; q in 0..31)

What is pinned is that rule, not a file llama-quantize wrote.  The QUANTISER is this build's min / max rule of q4k_ref.quantize_q4_k
with 31 steps instead of 15 and q clipped to 0..31; the HIP library applies the same rule on the device for weight_format="q5_k".
"""
import os
import sys
from unittest import mock

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import q4k_ref  # noqa: E402

Q5_K = 13          # GGUF tensor type
BLOCK_BYTES = 176


def quantize_q5_k(w: np.ndarray):
    """float32 [..., K] (K % 256 == 0) -> dict(q uint8 [..., K] in 0..31, sc, m uint8 [..., K/32], d, dmin float16 [..., K/256]):
    q4k_ref.quantize_q4_k operation for operation, with 31 for 15."""
    w = np.ascontiguousarray(w, dtype=np.float32)
    lead, K = w.shape[:-1], w.shape[-1]
    assert K % 256 == 0
    sub = w.reshape(-1, K // 256, 8, 32)
    mn = np.minimum(sub.min(axis=-1), np.float32(0.0))
    mx = sub.max(axis=-1)
    s = ((mx - mn) / np.float32(31.0)).astype(np.float32)
    o = (-mn).astype(np.float32)
    d = (s.max(axis=-1) / np.float32(63.0)).astype(np.float16)
    dmin = (o.max(axis=-1) / np.float32(63.0)).astype(np.float16)
    df, dminf = d.astype(np.float32)[..., None], dmin.astype(np.float32)[..., None]
    rnd = lambda x: np.floor(x + np.float32(0.5))   # noqa: E731
    with np.errstate(divide="ignore", invalid="ignore"):
        sc = np.where(df > 0, rnd(s / np.where(df > 0, df, 1)), 0)
        m = np.where(dminf > 0, rnd(o / np.where(dminf > 0, dminf, 1)), 0)
    sc = np.clip(sc, 0, 63).astype(np.float32)
    m = np.clip(m, 0, 63).astype(np.float32)
    d1 = (df * sc).astype(np.float32)[..., None]
    m1 = (dminf * m).astype(np.float32)[..., None]
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(d1 > 0, rnd((sub + m1) / np.where(d1 > 0, d1, 1)), 0)
    q = np.clip(q, 0, 31).astype(np.uint8)
    return dict(q=q.reshape(*lead, K), sc=sc.astype(np.uint8).reshape(*lead, K // 32), m=m.astype(np.uint8).reshape(*lead, K // 32),
                d=d.reshape(*lead, K // 256), dmin=dmin.reshape(*lead, K // 256))


def pack_blocks(p: dict) -> np.ndarray:
    """the dict of quantize_q5_k (or of q4k_ref.quantize_q4_k: all high bits zero) -> raw GGUF blocks uint8 [n_blocks, 176]"""
    q = p["q"].reshape(-1, 4, 2, 32)                     # [blk][t][low / high nibble][l]
    nb = q.shape[0]
    four = q4k_ref.pack_blocks(dict(p, q=p["q"] & 0xF))  # d, dmin, scales and the nibbles as Q4_K lays them out
    out = np.empty((nb, BLOCK_BYTES), np.uint8)
    out[:, 0:16] = four[:, 0:16]
    qh = np.zeros((nb, 32), np.uint8)
    for t in range(4):
        for hi in range(2):
            qh |= ((q[:, t, hi, :] >> 4) & 1) << (2 * t + hi)
    out[:, 16:48] = qh
    out[:, 48:176] = four[:, 16:144]
    return out


def unpack(raw: np.ndarray):
    """raw blocks uint8 [nb, 176] -> (q uint8 [nb, 256], sc uint8 [nb, 8], m uint8 [nb, 8], d float32 [nb, 1], dmin float32 [nb, 1])"""
    raw = raw.reshape(-1, BLOCK_BYTES)
    d = raw[:, 0:2].copy().view(np.float16).astype(np.float32)
    dmin = raw[:, 2:4].copy().view(np.float16).astype(np.float32)
    sc, m = q4k_ref.unpack_scales(raw[:, 4:16])
    qh = raw[:, 16:48]
    qs = raw[:, 48:176].reshape(-1, 4, 32)
    q = np.empty((raw.shape[0], 4, 2, 32), np.uint8)
    for t in range(4):
        q[:, t, 0] = (qs[:, t] & 0xF) | (((qh >> (2 * t)) & 1) << 4)
        q[:, t, 1] = (qs[:, t] >> 4) | (((qh >> (2 * t + 1)) & 1) << 4)
    return q.reshape(-1, 256), sc, m, d, dmin


def dequantize_blocks(raw: np.ndarray) -> np.ndarray:
    """raw blocks uint8 [nb, 176] -> float32 [nb * 256] by dequantize_row_q5_K's rule"""
    q, sc, m, d, dmin = unpack(raw)
    d1 = (d * sc.astype(np.float32)).astype(np.float32).reshape(-1, 8, 1)
    m1 = (dmin * m.astype(np.float32)).astype(np.float32).reshape(-1, 8, 1)
    return ((d1 * q.reshape(-1, 8, 32).astype(np.float32)).astype(np.float32) - m1).astype(np.float32).reshape(-1)


def _f32(w: np.ndarray) -> np.ndarray:
    return (w.astype(np.uint32) << 16).view(np.float32) if w.dtype == np.uint16 else np.asarray(w, np.float32)


def fake_quant(w: np.ndarray) -> np.ndarray:
    """bf16 bits or float32 matrix [N, K] -> float32 values of its Q5_K blocks (this build's quantiser, GGUF's de-quantiser)"""
    w = _f32(w)
    return dequantize_blocks(pack_blocks(quantize_q5_k(w))).reshape(w.shape)


def is_projection(name: str) -> bool:
    return name.endswith("_proj.weight") or name == "lm_head.weight"


def quantized_model(weights: dict) -> dict:
    """The model the device runs with weight_format='q5_k': every projection matrix and lm_head replaced by its Q5_K values (f32)"""
    return {k: (fake_quant(v) if is_projection(k) else v) for k, v in weights.items()}


def blocks_model(weights: dict) -> dict:
    """The same model as raw blocks: projections and lm_head as _native.Q5KBlocks (host-quantised), the rest as it is"""
    from realtime_codec_agent_amd._native import Q5KBlocks
    out = {}
    for k, v in weights.items():
        if is_projection(k):
            w = _f32(v)
            out[k] = Q5KBlocks(pack_blocks(quantize_q5_k(w)), w.shape)
        else:
            out[k] = v
    return out


# ---------------------------------------------------------------------------------------------------- the integer product form
def qmat(blocks):
    """_native.Q5KBlocks -> lm_q8_1_ref.QMat.  Q5_K is Q4_K's form with q in 0..31 -- value = s q - m with s = d sc and m = dmin m_j
    exact in f32 -- so QMat's "q4_k" arithmetic (dequantize, gemv_q8_1: the integer product form in float64) applies as it is."""
    import lm_q8_1_ref as R
    N, K = blocks.shape
    q, sc, m, d, dmin = unpack(blocks.raw)
    return R.QMat("q4_k", q.reshape(N, K), (d * sc.astype(np.float32)).astype(np.float32).reshape(N, K // 32),
                  (dmin * m.astype(np.float32)).astype(np.float32).reshape(N, K // 32))


class Mats:
    """HF name -> QMat over a dict of Q5KBlocks / Q6KBlocks (built on first use), for lm_q8_1_ref.StageRef"""

    def __init__(self, weights: dict):
        self.weights, self.done = weights, {}

    def __getitem__(self, k):
        import lm_q8_1_ref as R
        if k not in self.done:
            v = self.weights[k]
            self.done[k] = qmat(v) if type(v).__name__ == "Q5KBlocks" else R.QMat.from_blocks(v)
        return self.done[k]


def gemv_f32(W, x: np.ndarray):
    """The f32-activation form of lm_gemv_kernel over a QMat of the "q4_k" kind in float64, per 8-value chunk of a lane:
    (d sc) sum q_j x_j - (dmin m) sum x_j.  -> (y [M, N], mag [M, N]): mag = sum over chunks of sum_j |s q_j x_j| + |m| sum_j |x_j|,
    what the rounding bound of gemv_f32_bound scales with."""
    x64 = np.asarray(x, np.float32).astype(np.float64)
    M, K = x64.shape
    nc = K // 8
    xc = x64.reshape(M, nc, 8).transpose(1, 2, 0)                                  # [nc, 8, M]
    wq = W.q.reshape(W.N, nc, 8).astype(np.float64).transpose(1, 0, 2)             # [nc, N, 8]
    s = W.s.astype(np.float64).repeat(4, axis=1).T[:, :, None]                     # [nc, N, 1]
    mm = W.m.astype(np.float64).repeat(4, axis=1).T[:, :, None]
    P, Pa = np.matmul(wq, xc), np.matmul(wq, np.abs(xc))
    S, Sa = xc.sum(axis=1)[:, None, :], np.abs(xc).sum(axis=1)[:, None, :]
    y = (s * P - mm * S).sum(axis=0)
    mag = (s * Pa + mm * Sa).sum(axis=0)
    return y.T, mag.T


def gemv_f32_ops(K: int) -> int:
    """f32 roundings on the path of one product q_j x_j to the stage's sum on the f32-activation path: the lane's chain of 8 fmas
    (or the 7 adds of sum x and one more fma), the factor d sc / dmin m is exact, one fma per chunk and term kind: <= 2 * NIT, then
    lm_q8_1_ref.gemv_ops' reduction: 2 + 4 adds inside the wave, 3 across the waves."""
    import lm_q8_1_ref as R
    return R.gemv_ops(K) - 1 + 8


def gemv_f32_bound(K: int, mag: np.ndarray, normed: bool = False) -> np.ndarray:
    """normed: the stage's input is the kernel's own f32 RMSNorm of the residual, each value within lm_q8_1_ref.NORM_EPS_N (relative)
    of the exact one, and the reference's float32 rounding of its float64 norm within another u / 2: (NORM_EPS_N + u) * mag on top."""
    import lm_q8_1_ref as R
    n = gemv_f32_ops(K)
    return (n * R.U / (1 - n * R.U) + ((R.NORM_EPS_N + R.U) if normed else 0.0)) * mag


def stage_ref_f32(cfg, mats, norms):
    """lm_q8_1_ref.StageRef (RoPE, SwiGLU and K / V epilogues with their bounds) over the f32-activation product form above"""
    import lm_q8_1_ref as R

    class StageF32(R.StageRef):
        def run(self, kind, layer, x, pos0=0):
            normed = kind in (0, 2, 4)
            with mock.patch.object(R, "gemv_q8_1", gemv_f32), mock.patch.object(R, "gemv_bound", lambda K, mag: gemv_f32_bound(K, mag, normed)):
                return super().run(kind, layer, x, pos0)

    return StageF32(cfg, mats, norms)


# ---------------------------------------------------------------------------------------------------- GGUF files
def q5_k_m_type(gguf_name: str, n_layers: int) -> int:
    """The mix llama-quantize writes for LLAMA_FTYPE_MOSTLY_Q5_K_M (llama_tensor_get_type): output.weight Q6_K; attn_v and ffn_down
    Q6_K in the layers use_more_bits() picks (first and last eighth, every third in between), Q5_K otherwise -- the rule of
    gguf_writer.q4_k_m_type with Q5_K in the place of Q4_K."""
    import gguf_writer as gw
    if gguf_name == "output.weight":
        return gw.Q6_K
    if ".attn_v." in gguf_name or ".ffn_down." in gguf_name:
        i = int(gguf_name.split(".")[1])
        more = i < n_layers // 8 or i >= 7 * n_layers // 8 or (i - n_layers // 8) % 3 == 2
        return gw.Q6_K if more else Q5_K
    return Q5_K


def write_llama_gguf(path, cfg, weights, matrix_type=Q5_K):
    """A llama-architecture GGUF v3 file laid out as gguf_writer.write_llama_gguf lays one out (same metadata keys, reversed dims, Q / K
    row permutation, 32-byte aligned data), with Q5_K tensors: matrix_type = Q5_K (every matrix) or "Q5_K_M" (the mix above).  Norms
    stay F32.  Only gguf_writer's leaf helpers are called; nothing of it is changed."""
    import struct
    import gguf_writer as gw
    mix = matrix_type == "Q5_K_M"
    base = Q5_K if mix else matrix_type

    def data_of(a, tt):
        if tt == Q5_K:
            return pack_blocks(quantize_q5_k(np.ascontiguousarray(a, np.float32).reshape(-1, 256))).tobytes()
        return gw.quantize(a, tt)

    u32 = lambda key, v: gw._kv(key, 4, struct.pack("<I", v))   # noqa: E731
    kv = [gw._kv("general.architecture", 8, gw._s(b"llama")), u32("general.alignment", 32), u32("llama.embedding_length", cfg.hidden),
          u32("llama.block_count", cfg.n_layers), u32("llama.attention.head_count", cfg.n_heads), u32("llama.attention.head_count_kv", cfg.n_kv_heads),
          u32("llama.feed_forward_length", cfg.ffn), u32("llama.rope.dimension_count", cfg.head_dim), u32("llama.context_length", 2048),
          gw._kv("llama.attention.layer_norm_rms_epsilon", 6, struct.pack("<f", cfg.rms_eps)),
          gw._kv("llama.rope.freq_base", 6, struct.pack("<f", cfg.rope_theta))]
    ts = [("token_embd.weight", weights["model.embed_tokens.weight"]), ("output_norm.weight", weights["model.norm.weight"]),
          ("output.weight", weights["lm_head.weight"])]
    names = {"self_attn.q_proj": "attn_q", "self_attn.k_proj": "attn_k", "self_attn.v_proj": "attn_v", "self_attn.o_proj": "attn_output",
             "mlp.gate_proj": "ffn_gate", "mlp.up_proj": "ffn_up", "mlp.down_proj": "ffn_down", "input_layernorm": "attn_norm",
             "post_attention_layernorm": "ffn_norm"}
    for l in range(cfg.n_layers):
        for hf, gg in names.items():
            a = np.asarray(weights[f"model.layers.{l}.{hf}.weight"], np.float32)
            if gg == "attn_q":
                a = gw.permute(a, cfg.n_heads)
            elif gg == "attn_k":
                a = gw.permute(a, cfg.n_kv_heads)
            ts.append((f"blk.{l}.{gg}.weight", a))
    infos, blobs, off = [], [], 0
    for name, a in ts:
        a = np.asarray(a, np.float32)
        tt = gw.F32 if a.ndim == 1 else (q5_k_m_type(name, cfg.n_layers) if mix else base)
        data = data_of(a, tt)
        ne = list(reversed(a.shape))
        infos.append(gw._s(name.encode()) + struct.pack("<I", len(ne)) + b"".join(struct.pack("<Q", d) for d in ne) + struct.pack("<IQ", tt, off))
        pad = (-len(data)) % 32
        blobs.append(data + b"\0" * pad)
        off += len(data) + pad
    head = struct.pack("<IIQQ", 0x46554747, 3, len(ts), len(kv)) + b"".join(kv) + b"".join(infos)
    with open(path, "wb") as f:
        f.write(head + b"\0" * ((-len(head)) % 32))
        for b in blobs:
            f.write(b)
