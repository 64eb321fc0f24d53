"""GGUF Q4_0 / Q4_1 on the host (TEST INFRASTRUCTURE ONLY), beside tests/q5k_ref.py.

ggml is not part of this tree, so the published formats, de-quantisation rules and reference quantisers are restated here
(ggml-common.h `block_q4_0` / `block_q4_1`, ggml-quants.c `dequantize_row_q4_0` / `_q4_1`, `quantize_row_q4_0_ref` / `_q4_1_ref`):

    block_q4_0 (18 bytes, 32 weights, GGUF tensor type 2) = { fp16 d; uint8 qs[16] }          value = (q - 8) * d
    block_q4_1 (20 bytes, 32 weights, GGUF tensor type 3) = { fp16 d; fp16 m; uint8 qs[16] }  value = q * d + m
    weight j of a block (j < 16) = low nibble of qs[j], weight j + 16 = high nibble of qs[j]

    quantize_row_q4_0_ref: max = the value of largest magnitude (the first on ties), d = max / -8, id = d != 0 ? 1 / d : 0,
                           q = min(15, (int)(x * id + 8.5f)); fp16(d) is stored
    quantize_row_q4_1_ref: d = (max - min) / 15, id likewise, q = min(15, (int)((x - min) * id + 0.5f)); fp16(d), fp16(min) stored
    (float32 operations, each rounded on its own)

What is pinned is these rules, not a file llama-quantize wrote.  The HIP library applies the same rules on the device for
weight_format="q4_0" / "q4_1".  On the device both types are the Q4_K form s q - t with (s, t) = (d, 8 d) resp. (d, -m): `qmat` gives
lm_q8_1_ref.QMat("q4_k", q, s, t) and the float64 product forms of lm_q8_1_ref / q5k_ref apply.
"""
import os
import sys
from unittest import mock

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from oracle import q4k_ref  # noqa: E402

Q4_0, Q4_1 = 2, 3          # GGUF tensor types
BLOCK_BYTES = {Q4_0: 18, Q4_1: 20}
KINDS = {"q4_0": Q4_0, "q4_1": Q4_1}
F32 = np.float32


def _f32(w: np.ndarray) -> np.ndarray:
    return (w.astype(np.uint32) << 16).view(np.float32) if w.dtype == np.uint16 else np.ascontiguousarray(w, np.float32)


def quantize_q4_0(w: np.ndarray) -> dict:
    """float32 [..., K] (K % 32 == 0) -> dict(q uint8 [..., K] in 0..15, d float16 [..., K / 32])"""
    w = _f32(w)
    lead, K = w.shape[:-1], w.shape[-1]
    assert K % 32 == 0
    blk = w.reshape(-1, 32)
    mx = np.take_along_axis(blk, np.abs(blk).argmax(axis=1)[:, None], axis=1)          # argmax: the first of equal magnitudes
    d = (mx / F32(-8.0)).astype(F32)
    with np.errstate(divide="ignore"):
        inv = np.where(d != 0, (F32(1.0) / np.where(d != 0, d, F32(1.0))).astype(F32), F32(0.0)).astype(F32)
    y = ((blk * inv).astype(F32) + F32(8.5)).astype(F32)
    q = np.minimum(15, y.astype(np.int32)).astype(np.uint8)                            # (int): truncation; y >= 0.5 here
    return dict(q=q.reshape(*lead, K), d=d.astype(np.float16).reshape(*lead, K // 32))


def quantize_q4_1(w: np.ndarray) -> dict:
    """float32 [..., K] (K % 32 == 0) -> dict(q uint8 [..., K] in 0..15, d, m float16 [..., K / 32])"""
    w = _f32(w)
    lead, K = w.shape[:-1], w.shape[-1]
    assert K % 32 == 0
    blk = w.reshape(-1, 32)
    mn, mx = blk.min(axis=1, keepdims=True), blk.max(axis=1, keepdims=True)
    d = ((mx - mn).astype(F32) / F32(15.0)).astype(F32)
    inv = np.where(d != 0, (F32(1.0) / np.where(d != 0, d, F32(1.0))).astype(F32), F32(0.0)).astype(F32)
    y = (((blk - mn).astype(F32) * inv).astype(F32) + F32(0.5)).astype(F32)
    q = np.minimum(15, y.astype(np.int32)).astype(np.uint8)
    return dict(q=q.reshape(*lead, K), d=d.astype(np.float16).reshape(*lead, K // 32), m=mn.astype(np.float16).reshape(*lead, K // 32))


def quantize(w: np.ndarray, ttype: int) -> dict:
    return quantize_q4_1(w) if ttype == Q4_1 else quantize_q4_0(w)


def pack_blocks(p: dict) -> np.ndarray:
    """the dict of quantize_q4_0 (no "m") or quantize_q4_1 -> raw GGUF blocks uint8 [n_blocks, 18 or 20]"""
    q = p["q"].reshape(-1, 2, 16)
    nb = q.shape[0]
    head = 4 if "m" in p else 2
    out = np.empty((nb, head + 16), np.uint8)
    out[:, 0:2] = np.ascontiguousarray(p["d"], np.float16).reshape(-1, 1).view(np.uint8)
    if "m" in p:
        out[:, 2:4] = np.ascontiguousarray(p["m"], np.float16).reshape(-1, 1).view(np.uint8)
    out[:, head:] = q[:, 0] | (q[:, 1] << 4)
    return out


def unpack(raw: np.ndarray, ttype: int):
    """raw blocks -> (q uint8 [nb, 32], d float32 [nb, 1], m float32 [nb, 1] or None)"""
    raw = raw.reshape(-1, BLOCK_BYTES[ttype])
    head = 4 if ttype == Q4_1 else 2
    d = raw[:, 0:2].copy().view(np.float16).astype(F32)
    m = raw[:, 2:4].copy().view(np.float16).astype(F32) if ttype == Q4_1 else None
    qs = raw[:, head:]
    return np.concatenate([qs & 0xF, qs >> 4], axis=1), d, m


def dequantize_blocks(raw: np.ndarray, ttype: int) -> np.ndarray:
    """raw blocks -> float32 [nb * 32]: the elementwise float32 formula (q - 8) * d resp. q * d + m"""
    q, d, m = unpack(raw, ttype)
    qf = q.astype(F32)
    if ttype == Q4_0:
        return ((qf - F32(8.0)) * d).astype(F32).reshape(-1)
    return ((qf * d).astype(F32) + m).astype(F32).reshape(-1)


def block_class(ttype: int):
    from realtime_codec_agent_amd._native import Q40Blocks, Q41Blocks
    return Q41Blocks if ttype == Q4_1 else Q40Blocks


def type_of(blocks) -> int:
    return Q4_1 if type(blocks).__name__ == "Q41Blocks" else Q4_0


def to_blocks(w: np.ndarray, ttype: int):
    """float32 / bf16-bit matrix [N, K] -> _native.Q40Blocks / Q41Blocks by the numpy rule"""
    w = _f32(w)
    return block_class(ttype)(pack_blocks(quantize(w, ttype)), w.shape)


def fake_quant(w: np.ndarray, ttype: int) -> np.ndarray:
    w = _f32(w)
    return dequantize_blocks(pack_blocks(quantize(w, ttype)), ttype).reshape(w.shape)


def is_projection(name: str) -> bool:
    return name.endswith("_proj.weight") or name == "lm_head.weight"


def blocks_model(weights: dict, ttype: int) -> dict:
    """projections and lm_head as host-quantised blocks, the rest as it is"""
    return {k: (to_blocks(v, ttype) if is_projection(k) else v) for k, v in weights.items()}


# ---------------------------------------------------------------------------------------------------- the product forms
def factors(blocks):
    """(q uint8 [N, K], s float32 [N, K / 32], t float32 [N, K / 32]): value = s q - t with s = d and t = 8 d (Q4_0) or -m (Q4_1), as the
    device forms them at load.  8 d is exact in f32 (and in fp16 unless it overflows, which the load refuses)."""
    N, K = blocks.shape
    q, d, m = unpack(blocks.raw, type_of(blocks))
    t = (F32(8.0) * d).astype(F32) if m is None else (-m).astype(F32)
    return q.reshape(N, K), d.reshape(N, K // 32), t.reshape(N, K // 32)


def qmat(blocks):
    """_native.Q40Blocks / Q41Blocks -> lm_q8_1_ref.QMat of the "q4_k" kind"""
    import lm_q8_1_ref as R
    return R.QMat("q4_k", *factors(blocks))


class Mats:
    """HF name -> QMat over a dict of Q40Blocks / Q41Blocks / other block classes (built on first use), for lm_q8_1_ref.StageRef"""

    def __init__(self, weights: dict):
        self.weights, self.done = weights, {}

    def __getitem__(self, k):
        import lm_q8_1_ref as R
        if k not in self.done:
            v = self.weights[k]
            self.done[k] = qmat(v) if type(v).__name__ in ("Q40Blocks", "Q41Blocks") else R.QMat.from_blocks(v)
        return self.done[k]


def gemv_f32(W, x: np.ndarray):
    """q5k_ref.gemv_f32 for factors of either sign.  The value y is that function's, term for term: s sum q_j x_j - t sum x_j per
    8-value chunk in float64.  Its magnitude sum  s * sum q_j |x_j| + t * sum |x_j|  equals  sum_j |s q_j x_j| + |t| sum_j |x_j|  (what
    its docstring defines and the rounding bound scales with) only for s, t >= 0, which Q4_K / Q5_K guarantee and the legacy types do
    not: a Q4_0 block whose largest magnitude is positive has d < 0, and Q4_1 has t = -m of either sign.  Here |s| and |t| are used,
    i.e. the definition itself.  No operation is added or dropped against the Q4_K body -- (s, t) are exact in f32 exactly as
    d sc / dmin m are -- so q5k_ref.gemv_f32_ops and gemv_f32_bound hold as they are."""
    x64 = np.asarray(x, np.float32).astype(np.float64)
    M, K = x64.shape
    nc = K // 8
    xc = x64.reshape(M, nc, 8).transpose(1, 2, 0)                                  # [nc, 8, M]
    wq = W.q.reshape(W.N, nc, 8).astype(np.float64).transpose(1, 0, 2)             # [nc, N, 8]
    s = W.s.astype(np.float64).repeat(4, axis=1).T[:, :, None]                     # [nc, N, 1]
    t = W.m.astype(np.float64).repeat(4, axis=1).T[:, :, None]
    P, Pa = np.matmul(wq, xc), np.matmul(wq, np.abs(xc))
    S, Sa = xc.sum(axis=1)[:, None, :], np.abs(xc).sum(axis=1)[:, None, :]
    y = (s * P - t * S).sum(axis=0)
    mag = (np.abs(s) * Pa + np.abs(t) * Sa).sum(axis=0)
    return y.T, mag.T


def stage_ref_f32(cfg, mats, norms):
    """q5k_ref.stage_ref_f32 over gemv_f32 above (the bound is q5k_ref.gemv_f32_bound, unchanged)"""
    import lm_q8_1_ref as R
    import q5k_ref

    class StageF32(R.StageRef):
        def run(self, kind, layer, x, pos0=0):
            normed = kind in (0, 2, 4)
            with mock.patch.object(R, "gemv_q8_1", gemv_f32), mock.patch.object(R, "gemv_bound", lambda K, mag: q5k_ref.gemv_f32_bound(K, mag, normed)):
                return super().run(kind, layer, x, pos0)

    return StageF32(cfg, mats, norms)


# ---------------------------------------------------------------------------------------------------- the Q4_K twin
def twin_matrix(rng, N: int, K: int, ttype: int):
    """(Q40Blocks / Q41Blocks, Q4KBlocks) holding the same values: d (and m) constant over each run of 256 values, so the Q4_0 tensor is
    the Q4_K tensor with sc = 1, m = 8, d = dmin = d0, and the Q4_1 tensor the one with sc = 1, m = 1, d = d0, dmin = -m0.  d0 takes
    both signs (a Q4_0 d is negative whenever the block's largest magnitude is positive)."""
    from realtime_codec_agent_amd._native import Q4KBlocks
    assert K % 256 == 0
    q = rng.integers(0, 16, (N, K), dtype=np.uint8)
    d0 = (rng.uniform(2e-3, 1.5e-2, (N, K // 256)) * rng.choice([-1.0, 1.0], (N, K // 256))).astype(np.float16)
    p = dict(q=q, d=d0.repeat(8, axis=1))
    p4 = dict(q=q, sc=np.ones((N, K // 32), np.uint8), d=d0)
    if ttype == Q4_1:
        m0 = (rng.uniform(-6e-2, 6e-2, (N, K // 256))).astype(np.float16)
        p["m"] = m0.repeat(8, axis=1)
        p4.update(m=np.ones((N, K // 32), np.uint8), dmin=(-m0).astype(np.float16))
    else:
        p4.update(m=np.full((N, K // 32), 8, np.uint8), dmin=d0)
    return block_class(ttype)(pack_blocks(p), (N, K)), Q4KBlocks(q4k_ref.pack_blocks(p4), (N, K))


def twin_models(cfg, seed: int, ttype: int):
    """(weights with every projection and the head as Q4_0 / Q4_1 blocks, the same with their Q4_K twins)"""
    from oracle import lm_ref
    rng = np.random.default_rng(seed)
    a, b = {}, {}
    for k, v in lm_ref.random_weights(cfg, seed, 0.05).items():
        if is_projection(k):
            a[k], b[k] = twin_matrix(rng, v.shape[0], v.shape[1], ttype)
        else:
            a[k] = b[k] = v
    return a, b


# ---------------------------------------------------------------------------------------------------- GGUF files
def q4_0_mix_type(gguf_name: str) -> int:
    """"Q4_0 as llama-quantize writes it" for the test files: Q4_0 everywhere, output.weight Q6_K (llama_tensor_get_type gives the output
    tensor Q6_K for this file type), and ffn_down of layer 0 Q4_1 (what the tool falls to for some ffn_down tensors when an
    importance matrix is given)."""
    import gguf_writer as gw
    if gguf_name == "output.weight":
        return gw.Q6_K
    if gguf_name == "blk.0.ffn_down.weight":
        return Q4_1
    return Q4_0


def write_llama_gguf(path, cfg, weights, matrix_type=Q4_0):
    """A llama-architecture GGUF v3 file laid out as gguf_writer.write_llama_gguf lays one out (same metadata keys, reversed dims, Q / K
    row permutation, 32-byte aligned data): matrix_type = Q4_0 / Q4_1 (every matrix) or "Q4_0_MIX" (the mix above).  Norms stay F32.
    Only gguf_writer's leaf helpers are called; nothing of it is changed."""
    import struct
    import gguf_writer as gw
    mix = matrix_type == "Q4_0_MIX"

    def data_of(a, tt):
        if tt in (Q4_0, Q4_1):
            return pack_blocks(quantize(np.ascontiguousarray(a, np.float32).reshape(-1, 32), tt)).tobytes()
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
        tt = gw.F32 if a.ndim == 1 else (q4_0_mix_type(name) if mix else matrix_type)
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
