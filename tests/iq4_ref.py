"""GGUF IQ4_NL / IQ4_XS on the host (TEST INFRASTRUCTURE ONLY), beside tests/q40_ref.py and tests/q5k_ref.py.

ggml is not part of this tree, so the published formats and de-quantisation rules are restated here (ggml-common.h `block_iq4_nl` /
`block_iq4_xs` and `kvalues_iq4nl`, ggml-quants.c `dequantize_row_iq4_nl` / `_iq4_xs`):

    kvalues_iq4nl[16] = { -127, -104, -83, -65, -49, -35, -22, -10, 1, 13, 25, 38, 53, 69, 89, 113 }   (int8)
    block_iq4_nl (18 bytes, 32 weights, GGUF tensor type 20) = { fp16 d; uint8 qs[16] }
        weight j = d * kv[qs[j] & 15], weight j + 16 = d * kv[qs[j] >> 4]                      (Q4_0's nibble order)
    block_iq4_xs (136 bytes, 256 weights, GGUF tensor type 23) = { fp16 d; uint16 scales_h; uint8 scales_l[4]; uint8 qs[128] }
        sub-block ib = 0..7: ls = ((scales_l[ib / 2] >> 4 (ib % 2)) & 15) | (((scales_h >> 2 ib) & 3) << 4), dl = d * (ls - 32)
        weight j = dl * kv[qs[16 ib + j] & 15], weight j + 16 = dl * kv[qs[16 ib + j] >> 4]
    d * (ls - 32) is 11 x 6 bits and dl * kv 17 x 7 bits: both exact in f32, so every weight has ONE f32 value.

What is pinned is these rules, not a file llama-quantize wrote.  The load-time quantiser (weight_format="iq4_nl") is this build's plain
rule, NOT llama-quantize's (an iterative weighted search that cannot be pinned offline):

    max = the value of largest magnitude per 32 (the first on ties), d = fp16(max / -127)
    index = argmin_i |x - d * kv[i]| in float32 (ties to the lower index); a block whose d is 0 (all-zero blocks among them): index 8

On the device both types are one form, value = s * kv[q] with one f32 factor s per row and 32 values (s = d resp. d (ls - 32)): `qmat`
gives lm_q8_1_ref.QMat("q8_0", kv[q], s), whose de-quantisation s * q and integer product form (s d_x) sum q_w q_x are exactly this
form's.  The rounding bounds are derived below.
"""
import os
import sys
from unittest import mock

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

IQ4_NL, IQ4_XS = 20, 23          # GGUF tensor types
BLOCK_BYTES = {IQ4_NL: 18, IQ4_XS: 136}
BLOCK_VALUES = {IQ4_NL: 32, IQ4_XS: 256}
KV = np.array([-127, -104, -83, -65, -49, -35, -22, -10, 1, 13, 25, 38, 53, 69, 89, 113], np.int8)
F32 = np.float32


def _f32(w: np.ndarray) -> np.ndarray:
    return (w.astype(np.uint32) << 16).view(np.float32) if w.dtype == np.uint16 else np.ascontiguousarray(w, np.float32)


# ---------------------------------------------------------------------------------------------------- the load-time rule
def quantize_iq4_nl(w: np.ndarray) -> dict:
    """float32 [..., K] (K % 32 == 0) -> dict(q uint8 [..., K] table indices, d float16 [..., K / 32])"""
    w = _f32(w)
    lead, K = w.shape[:-1], w.shape[-1]
    assert K % 32 == 0
    blk = w.reshape(-1, 32)
    mx = np.take_along_axis(blk, np.abs(blk).argmax(axis=1)[:, None], axis=1)          # argmax: the first of equal magnitudes
    with np.errstate(over="ignore"):
        d16 = (mx / F32(-127.0)).astype(F32).astype(np.float16)
    d = d16.astype(F32)                                                                # [nb, 1]
    cand = (d * KV.astype(F32)[None, :]).astype(F32)                                   # [nb, 16] exact
    q = np.empty(blk.shape, np.uint8)
    for i in range(0, blk.shape[0], 1 << 15):                                          # in slices: the distances are 16 floats per value
        dist = np.abs((blk[i:i + (1 << 15), :, None] - cand[i:i + (1 << 15), None, :]).astype(F32))   # [n, 32, 16], f32 subtraction
        q[i:i + (1 << 15)] = dist.argmin(axis=2)                                       # argmin: the lowest index of equal distances
    q[(d == 0).reshape(-1)] = 8
    return dict(q=q.reshape(*lead, K), d=d16.reshape(*lead, K // 32))


# ---------------------------------------------------------------------------------------------------- blocks
def pack_iq4_nl(p: dict) -> np.ndarray:
    """dict(q [.., K] indices, d float16 [.., K / 32]) -> raw blocks uint8 [n_blocks, 18]"""
    q = p["q"].reshape(-1, 2, 16)
    out = np.empty((q.shape[0], 18), np.uint8)
    out[:, 0:2] = np.ascontiguousarray(p["d"], np.float16).reshape(-1, 1).view(np.uint8)
    out[:, 2:] = q[:, 0] | (q[:, 1] << 4)
    return out


def pack_iq4_xs(p: dict) -> np.ndarray:
    """dict(q [.., K] indices, d float16 [.., K / 256], ls [.., K / 32] in 0..63) -> raw super-blocks uint8 [n_blocks, 136]"""
    q = p["q"].reshape(-1, 8, 2, 16)
    nb = q.shape[0]
    ls = np.asarray(p["ls"]).reshape(nb, 8).astype(np.uint32)
    assert ls.max() <= 63
    out = np.empty((nb, 136), np.uint8)
    out[:, 0:2] = np.ascontiguousarray(p["d"], np.float16).reshape(-1, 1).view(np.uint8)
    sh = np.zeros(nb, np.uint32)
    for ib in range(8):
        sh |= (ls[:, ib] >> 4) << (2 * ib)
    out[:, 2:4] = sh.astype(np.uint16).reshape(-1, 1).view(np.uint8)
    lo = ls & 15
    out[:, 4:8] = (lo[:, 0::2] | (lo[:, 1::2] << 4)).astype(np.uint8)
    out[:, 8:] = (q[:, :, 0] | (q[:, :, 1] << 4)).reshape(nb, 128)
    return out


def unpack(raw: np.ndarray, ttype: int):
    """raw blocks -> (q uint8 [n32, 32] indices, d float32 [n32, 1] the block's fp16 d, ls int32 [n32, 1]; IQ4_NL: ls = 33, i.e. ls - 32 = 1)
    with n32 = the number of 32-value (sub-)blocks.  Written from the bit rules, independently of _native's classes."""
    raw = raw.reshape(-1, BLOCK_BYTES[ttype])
    if ttype == IQ4_NL:
        d = raw[:, 0:2].copy().view(np.float16).astype(F32)
        qs = raw[:, 2:]
        return np.concatenate([qs & 0xF, qs >> 4], axis=1), d, np.full((raw.shape[0], 1), 33, np.int32)
    nb = raw.shape[0]
    d = raw[:, 0:2].copy().view(np.float16).astype(F32).repeat(8, axis=0)
    sh = raw[:, 2:4].copy().view(np.uint16).astype(np.int32).reshape(nb)
    ls = np.empty((nb, 8), np.int32)
    for ib in range(8):
        ls[:, ib] = ((raw[:, 4 + ib // 2].astype(np.int32) >> (4 * (ib % 2))) & 15) | (((sh >> (2 * ib)) & 3) << 4)
    qs = raw[:, 8:].reshape(nb * 8, 16)
    return np.concatenate([qs & 0xF, qs >> 4], axis=1), d, ls.reshape(-1, 1)


def dequantize_blocks(raw: np.ndarray, ttype: int) -> np.ndarray:
    """raw blocks -> float32 [values]: d * (ls - 32) * kv[q] written out directly, float32 products (both exact)"""
    q, d, ls = unpack(raw, ttype)
    dl = (d * (ls - 32).astype(F32)).astype(F32)
    return (dl * KV[q].astype(F32)).astype(F32).reshape(-1)


def block_class(ttype: int):
    from realtime_codec_agent_amd._native import IQ4NLBlocks, IQ4XSBlocks
    return IQ4XSBlocks if ttype == IQ4_XS else IQ4NLBlocks


def type_of(blocks) -> int:
    return IQ4_XS if type(blocks).__name__ == "IQ4XSBlocks" else IQ4_NL


def is_iq4(v) -> bool:
    return type(v).__name__ in ("IQ4NLBlocks", "IQ4XSBlocks")


def to_blocks(w: np.ndarray):
    """float32 / bf16-bit matrix [N, K] -> _native.IQ4NLBlocks by the numpy rule"""
    w = _f32(w)
    return block_class(IQ4_NL)(pack_iq4_nl(quantize_iq4_nl(w)), w.shape)


def xs_blocks_of(w: np.ndarray, rng):
    """float32 matrix [N, K] (K % 256 == 0) -> _native.IQ4XSBlocks for the test FILES: one fp16 d per 256 values, a scale code ls per 32
    chosen so that d (ls - 32) is near the sub-block's max / -127 (ls != 32 unless the sub-block is zero), indices to the nearest value.
    Not llama-quantize's search either: the files only need plausible IQ4_XS content with many different ls."""
    w = _f32(w)
    N, K = w.shape
    assert K % 256 == 0
    sub = w.reshape(-1, 8, 32)
    mx = np.take_along_axis(sub, np.abs(sub).argmax(axis=2)[:, :, None], axis=2)[:, :, 0]           # [nb, 8] signed extreme values
    want = mx / -127.0                                                                           # the step each sub-block would like
    big = np.abs(want).max(axis=1, keepdims=True)
    d = (big / 31.0 * np.where(rng.random((sub.shape[0], 1)) < 0.5, -1.0, 1.0)).astype(np.float16)  # both signs of d
    df = d.astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        l = np.where(df != 0, np.rint(want / np.where(df != 0, df, 1.0)), 0.0)
    l = np.clip(l, -32, 31)
    l = np.where((l == 0) & (mx != 0), 1.0, l)
    ls = (l + 32).astype(np.int32)
    dl = (d.astype(F32) * (ls - 32).astype(F32)).astype(F32)                                     # [nb, 8]
    cand = (dl[:, :, None] * KV.astype(F32)[None, None, :]).astype(F32)                            # [nb, 8, 16]
    q = np.abs(sub[:, :, :, None] - cand[:, :, None, :]).argmin(axis=3).astype(np.uint8)
    return block_class(IQ4_XS)(pack_iq4_xs(dict(q=q, d=d, ls=ls)), (N, K))


def fake_quant(w: np.ndarray) -> np.ndarray:
    w = _f32(w)
    return dequantize_blocks(pack_iq4_nl(quantize_iq4_nl(w)), IQ4_NL).reshape(w.shape)


def is_projection(name: str) -> bool:
    return name.endswith("_proj.weight") or name == "lm_head.weight"


def blocks_model(weights: dict) -> dict:
    """projections and lm_head as host-quantised IQ4_NL blocks, the rest as it is"""
    return {k: (to_blocks(v) if is_projection(k) else v) for k, v in weights.items()}


# ---------------------------------------------------------------------------------------------------- the product forms
def factors(blocks):
    """(kv[q] int8 [N, K], s float32 [N, K / 32]): value = s kv[q] with s = d (IQ4_NL) or d (ls - 32) (IQ4_XS), as formed at load"""
    N, K = blocks.shape
    q, d, ls = unpack(blocks.raw, type_of(blocks))
    return KV[q].reshape(N, K), (d * (ls - 32).astype(F32)).astype(F32).reshape(N, K // 32)


def qmat(blocks):
    """_native.IQ4NLBlocks / IQ4XSBlocks -> lm_q8_1_ref.QMat of the "q8_0" kind: int8 values kv[q] and one f32 factor per 32"""
    import lm_q8_1_ref as R
    return R.QMat("q8_0", *factors(blocks))


class Mats:
    """HF name -> QMat over a dict of IQ4 / other block classes (built on first use), for lm_q8_1_ref.StageRef"""

    def __init__(self, weights: dict):
        self.weights, self.done = weights, {}

    def __getitem__(self, k):
        import lm_q8_1_ref as R
        import q5k_ref
        if k not in self.done:
            v = self.weights[k]
            self.done[k] = qmat(v) if is_iq4(v) else (q5k_ref.qmat(v) if type(v).__name__ == "Q5KBlocks" else R.QMat.from_blocks(v))
        return self.done[k]


def gemv_f32(W, x: np.ndarray):
    """The f32-activation form of lm_gemv_kernel over an IQ4 QMat in float64, per 8-value chunk of a lane: s sum_j kv_j x_j (no minimum
    term: the table is signed).  -> (y [M, N], mag [M, N]) with mag = sum over chunks of |s| sum_j |kv_j| |x_j|."""
    x64 = np.asarray(x, np.float32).astype(np.float64)
    M, K = x64.shape
    nc = K // 8
    xc = x64.reshape(M, nc, 8).transpose(1, 2, 0)                                  # [nc, 8, M]
    wq = W.q.reshape(W.N, nc, 8).astype(np.float64).transpose(1, 0, 2)             # [nc, N, 8]
    s = W.s.astype(np.float64).repeat(4, axis=1).T[:, :, None]                     # [nc, N, 1]
    y = (s * np.matmul(wq, xc)).sum(axis=0)
    mag = (np.abs(s) * np.matmul(np.abs(wq), np.abs(xc))).sum(axis=0)
    return y.T, mag.T


def _nit(K: int) -> int:
    nit = -(-(-(-(K // 8) // 4)) // 64)             # chunks per lane: ceil(ceil(K / 8 / 4 waves) / 64 lanes), 3 runs as 4
    return 4 if nit == 3 else nit


def gemv_f32_ops(K: int) -> int:
    """f32 roundings on the path of one product kv_j x_j to the stage's sum, f32 activations (lm_gemv_body, IQ4 branch): kv_j converts
    exactly; the lane's chain of 8 fmas over the chunk; the factor s is exact and val = fma(s, p, val) rounds once per chunk of the
    lane: NIT; then the reduction lm_q8_1_ref.gemv_ops counts: 2 + 4 adds inside the wave, 3 across the waves.  There is no second term
    kind (no minimum), so the chunk fmas count NIT where Q4_K's count 2 NIT."""
    return 8 + _nit(K) + 6 + 3


def gemv_f32_bound(K: int, mag: np.ndarray, normed: bool = False) -> np.ndarray:
    """gamma_n * mag, n = gemv_f32_ops.  normed: the stage's input is the kernel's own f32 RMSNorm of the residual, as in
    q5k_ref.gemv_f32_bound: (NORM_EPS_N + u) * mag on top."""
    import lm_q8_1_ref as R
    n = gemv_f32_ops(K)
    return (n * R.U / (1 - n * R.U) + ((R.NORM_EPS_N + R.U) if normed else 0.0)) * mag


def gemv_q8_1_ops(K: int) -> int:
    """q8_1 activations: the integer sum of a chunk is exact (|sum| <= 8 * 127 * 127 < 2^20, so its conversion to f32 is too); the
    product s * d_x rounds once; one fma per chunk of the lane: NIT; the reduction: 6 + 3."""
    return 1 + _nit(K) + 6 + 3


def gemv_q8_1_bound(K: int, mag: np.ndarray) -> np.ndarray:
    import lm_q8_1_ref as R
    n = gemv_q8_1_ops(K)
    return n * R.U / (1 - n * R.U) * mag


def stage_refs(cfg, mats, norms):
    """{"f32", "q8_1"}: lm_q8_1_ref.StageRef (RoPE, SwiGLU and K / V epilogues with their bounds) over the two product forms of the IQ4
    body with the bounds above.  lm_q8_1_ref.gemv_q8_1 computes the "q8_0" kind's (s d_x) sum q_w q_x with mag = sum |term|, which is
    this form's."""
    import lm_q8_1_ref as R

    class StageF32(R.StageRef):
        def run(self, kind, layer, x, pos0=0):
            normed = kind in (0, 2, 4)
            with mock.patch.object(R, "gemv_q8_1", gemv_f32), mock.patch.object(R, "gemv_bound", lambda K, mag: gemv_f32_bound(K, mag, normed)):
                return super().run(kind, layer, x, pos0)

    class StageQ81(R.StageRef):
        def run(self, kind, layer, x, pos0=0):
            with mock.patch.object(R, "gemv_bound", gemv_q8_1_bound):
                return super().run(kind, layer, x, pos0)

    return {"f32": StageF32(cfg, mats, norms), "q8_1": StageQ81(cfg, mats, norms)}


# ---------------------------------------------------------------------------------------------------- the two types as one form
def twin_matrix(rng, N: int, K: int):
    """(IQ4NLBlocks, IQ4XSBlocks) holding the same values: d constant over each run of 256 values, every ls = 33 (ls - 32 = 1).  d takes
    both signs."""
    assert K % 256 == 0
    q = rng.integers(0, 16, (N, K), dtype=np.uint8)
    d0 = (rng.uniform(2e-4, 1.5e-3, (N, K // 256)) * rng.choice([-1.0, 1.0], (N, K // 256))).astype(np.float16)
    nl = block_class(IQ4_NL)(pack_iq4_nl(dict(q=q, d=d0.repeat(8, axis=1))), (N, K))
    xs = block_class(IQ4_XS)(pack_iq4_xs(dict(q=q, d=d0, ls=np.full((N, K // 32), 33))), (N, K))
    return nl, xs


def twin_models(cfg, seed: int):
    """(weights with every projection and the head as IQ4_NL blocks, the same values as IQ4_XS blocks)"""
    from oracle import lm_ref
    rng = np.random.default_rng(seed)
    a, b = {}, {}
    for k, v in lm_ref.random_weights(cfg, seed, 0.05).items():
        if is_projection(k):
            a[k], b[k] = twin_matrix(rng, v.shape[0], v.shape[1])
        else:
            a[k] = b[k] = v
    return a, b


# ---------------------------------------------------------------------------------------------------- GGUF files
def iq4_xs_mix_type(gguf_name: str, n_layers: int) -> int:
    """"IQ4_XS as llama-quantize writes it" for the test files, after llama_tensor_get_type as the issue recalls it: output.weight Q6_K,
    attn_v Q5_K (the rule for a query group size of 4 or more, applied to the test models whatever theirs is) and the first eighth of
    the ffn_down tensors (at least layer 0) Q5_K; IQ4_XS everywhere else."""
    import gguf_writer as gw
    import q5k_ref
    if gguf_name == "output.weight":
        return gw.Q6_K
    parts = gguf_name.split(".")
    if parts[0] == "blk" and (parts[2] == "attn_v" or (parts[2] == "ffn_down" and int(parts[1]) < max(1, n_layers // 8))):
        return q5k_ref.Q5_K
    return IQ4_XS


def write_llama_gguf(path, cfg, weights, matrix_type=IQ4_NL, seed=0):
    """A llama-architecture GGUF v3 file laid out as gguf_writer.write_llama_gguf lays one out (same metadata keys, reversed dims, Q / K
    row permutation, 32-byte aligned data): matrix_type = IQ4_NL / IQ4_XS (every matrix) or "IQ4_XS_MIX" (the mix above).  Norms stay
    F32.  Only gguf_writer's / q5k_ref's leaf helpers are called; nothing of them is changed."""
    import struct
    import gguf_writer as gw
    import q5k_ref
    mix = matrix_type == "IQ4_XS_MIX"
    rng = np.random.default_rng(seed)

    def data_of(a, tt):
        if tt == IQ4_NL:
            return pack_iq4_nl(quantize_iq4_nl(np.ascontiguousarray(a, np.float32).reshape(-1, 32))).tobytes()
        if tt == IQ4_XS:
            return np.ascontiguousarray(xs_blocks_of(np.ascontiguousarray(a, np.float32).reshape(-1, 256), rng).raw).tobytes()
        if tt == q5k_ref.Q5_K:
            return q5k_ref.pack_blocks(q5k_ref.quantize_q5_k(np.ascontiguousarray(a, np.float32).reshape(-1, 256))).tobytes()
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
        tt = gw.F32 if a.ndim == 1 else (iq4_xs_mix_type(name, cfg.n_layers) if mix else matrix_type)
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
