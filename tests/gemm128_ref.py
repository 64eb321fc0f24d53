"""Cases, float64 reference and error bound of the 128-token-tile GEMMs run alone (rca_lm_gemm128_tap), shared by
tests/test_gemm128_cpu.py (do the cases meet their conditions, does the bound have teeth?) and tests/test_gemm128_gpu.py (do
lm_gemm128_kernel<EPI, WF> and lm_gemm128_epilogue_kernel<EPI> compute it, in every k-slice form?).

THE OPERATION.  y[t][n] = sum_k W[n][k] (xh + xl)[t][k], then the projection's epilogue.  The test hands over the two bf16 planes xh, xl
themselves, so the operand is known exactly.  W[n][k] is the ONE f32 value the format's de-quantisation rule gives (oracle/q8_ref.py,
oracle/q4k_ref.py, tests/q5k_ref.py, tests/q40_ref.py, tests/iq4_ref.py; bf16 / fp16 widened).  The device forms that same f32 value
while staging, operation for operation: fp16 -> f32 is exact; d q (q8_0, 11 x 8 bits), (d sc) q (Q4_K / Q5_K, 11 x 6 x 5 bits),
(d sc) q (Q6_K, 11 x 7 x 6), d (q - 8) (Q4_0), s kv (IQ4, 17 x 7) are exact products, so q4k_value's d1 * q - m1 and q40_value's
s * q - t round ONCE, at the subtraction, whether or not the compiler contracts them into an fma -- as the restatements do.  The
"f32 de-quantisation" therefore adds no term: reference and device start from the same f32 weight.

THE BOUND, per output element, in the units of tests/attn_ref.py: u = 2^-24 (one IEEE f32 operation), U = 2^-23 (one addition
inside an MFMA accumulation: a whole ulp covers truncation and the alignment of the 16 products of one instruction).

  GEMM.  With S = sum_k |w| (|xh| + |xl|):
    * bf16 weights go to the MFMA as they are: the products are exact in f32 (8 x 8 bits); a slice of K / ns values accumulates
      2 K / ns products (w xh, w xl), each addition within U of a partial sum that is at most S: 2 (K / ns) U S.
    * every other format is split while staging (split_w8): hi = RNE_bf16(w), lo = RNE_bf16(w - hi), and three MFMAs per k step add
      hi xh + hi xl + lo xh: 3 (K / ns) U S.  What they leave out is computed from the planes, not estimated:
          sum_k |w - hi - lo| |x|       (the split residual: bf16 keeps 8 significant bits, so <= 2^-17 |w| per weight)
        + sum_k |lo| |xl|               (the dropped product, <= 2^-16 |w| |x|).
    * ns > 1: the slices are added in two levels (g128_group): groups of grp slices from 0, then the ng group sums from 0, each an
      IEEE addition of partial sums bounded by S: (grp + ng) u S.  The walking forms do the same additions in registers.
  Epilogues.
    * residual (kinds 1, 3) and logits (kind 4): 0 + y and a plain store: nothing.
    * RoPE (kind 0): o1 = x1 c + (-x2) s, o2 = x2 c + x1 s: two products and a sum, or a product and an fma: 2 u (|x1 c| + |x2 s|);
      the GEMM bounds of x1, x2 pass through |c|, |s|.  The table entries are cosf / sinf of the f32 angle pos * inv_freq (the same f32
      product here): the HIP math API's accuracy table lists both at 1 ulp; 2 ulp of values <= 1 are granted, 4 u absolutely: 4 u (|x1| + |x2|).
      K rows are o rounded to fp16 (RNE), V rows the sums themselves rounded: the interval [want - b, want + b] is rounded at both
      ends (RNE is monotone), no further ulp is granted.
    * SwiGLU (kind 2): h = (g / (1 + __expf(-g))) * up.  __expf(x) = exp2(x * log2 e) on v_exp_f32: the constant and the product
      round (2 u |x| log2 e in the argument, 2 u |g| in the result), the HIP math API's table of fast intrinsics lists __expf at 1 ulp = 2 u; 1 + e rounds (u,
      and the error of e weighs e / (1 + e) <= 1); the division is correctly rounded (u; hipcc's default), the product u:
      (2 |g| + 6) u |h| with one u of slack for second-order terms, plus 2^-120 (1 + |up|) for v_exp_f32 flushing denormals.  silu has slope
      in [-0.1, 1.1]: the GEMM bounds pass through as 1.1 |up| b_g + |silu(g)| b_u + 1.1 b_g b_u.  The planes are bf16 hi = RNE(h),
      lo = RNE(h - hi), returned as f32 hi + lo: 2^-17 |h| + u |h|.

Nothing here is fitted to a device's output: a correct kernel outside this bound means a missing term, which is to be found and named.
"""
import functools

import numpy as np

import iq4_ref
import q40_ref
import q5k_ref
from oracle import q4k_ref, q8_ref

u = 2.0 ** -24
U = 2.0 ** -23
F32 = np.float32
LM_MAXM = 1024
KINDS = {0: "qkv", 1: "o", 2: "gate_up", 3: "down", 4: "head"}


# ------------------------------------------------------------------------------------------------ k-slice forms (rca_lm.hip restated)
def g128_splits(N, K):
    ns = 1
    while ns * (N // 128) < 512 and K % (ns * 2 * 32) == 0 and K // (ns * 2) >= 256:
        ns *= 2
    return ns


def g128_group(ns):
    return ns // min(ns, 4)


def g128_form(N, ns, tbz, seq_min):
    """-> (grid_y, nseq, ep_nsplit, ep_grp), what rca_lm_gemm128_tap reports"""
    grp = g128_group(ns)
    ng = ns // grp
    if ns == 1:
        return (1, 1, 0, 1)
    if grp == 1 and seq_min > 0 and (N // 128) * tbz >= seq_min:
        return (1, ns, 0, 1)
    if grp > 1 and seq_min > 0 and (N // 128) * tbz * ng >= seq_min:
        return (ng, grp, ng, 1)
    return (ns, 1, ns, grp)


def form_name(f):
    gy, nseq, ep, grp = f
    if (gy, nseq, ep) == (1, 1, 0):
        return "fused"
    if ep == 0:
        return "walking"
    if nseq > 1:
        return "group sums stored"
    return "every slice stored" + (", grouped epilogue" if grp > 1 else "")


# ------------------------------------------------------------------------------------------------ models
MODELS = {"B": dict(hidden=256, n_heads=4, n_kv_heads=1, ffn=1024),
          "A": dict(hidden=512, n_heads=8, n_kv_heads=4, ffn=2048),
          "C": dict(hidden=1024, n_heads=16, n_kv_heads=4, ffn=4096)}
N_CTX = 2048
VOCABS = (388, 644)
VOCAB_BF16_EXTRA = 130
PROJ = ("q", "k", "v", "o", "gate", "up", "down", "head")
HF = {"q": "model.layers.0.self_attn.q_proj.weight", "k": "model.layers.0.self_attn.k_proj.weight", "v": "model.layers.0.self_attn.v_proj.weight",
      "o": "model.layers.0.self_attn.o_proj.weight", "gate": "model.layers.0.mlp.gate_proj.weight", "up": "model.layers.0.mlp.up_proj.weight",
      "down": "model.layers.0.mlp.down_proj.weight", "head": "lm_head.weight"}


def dims(model, vocab):
    m = MODELS[model]
    H, AO, KV, F = m["hidden"], m["n_heads"] * 64, m["n_kv_heads"] * 64, m["ffn"]
    return {"q": (AO, H), "k": (KV, H), "v": (KV, H), "o": (H, AO), "gate": (F, H), "up": (F, H), "down": (H, F), "head": (vocab, H)}


def kind_nk(model, kind, vocab=VOCABS[0]):
    """(N, K) of the GEMM a kind launches (the fused matrix)"""
    m = MODELS[model]
    H, AO, KV, F = m["hidden"], m["n_heads"] * 64, m["n_kv_heads"] * 64, m["ffn"]
    return {0: (AO + 2 * KV, H), 1: (H, AO), 2: (2 * F, H), 3: (H, F), 4: (vocab, H)}[kind]


def config(model, vocab):
    from realtime_codec_agent_amd.llm import LMConfig
    return LMConfig(vocab_size=vocab, n_layers=1, head_dim=64, rope_scaling=None, rope_theta=10000.0, **MODELS[model])


# the eight device forms: name -> type of each matrix; the head's type also depends on the vocabulary (the second type of a pair gets a
# ragged head of its own)
FORMATS = ("bf16", "f16", "q8_0", "q4_k", "q5_k", "q6_k", "q4_0", "iq4")


def matrix_types(fmt, vocab):
    one = lambda t: {p: t for p in PROJ}   # noqa: E731
    if fmt == "q6_k":     # a q4_k_m-style layer: V and down (and the head) Q6_K, the rest Q4_K: the V projection is a segment of its own
        return dict(one("q4_k"), v="q6_k", down="q6_k", head="q6_k")
    if fmt == "q4_0":
        return dict(one("q4_0"), o="q4_1", down="q4_1", head="q4_0" if vocab == VOCABS[0] else "q4_1")
    if fmt == "iq4":
        return dict(one("iq4_nl"), o="iq4_xs", down="iq4_xs", head="iq4_nl" if vocab == VOCABS[0] else "iq4_xs")
    return one(fmt)


# ------------------------------------------------------------------------------------------------ bf16 planes
def bf16_rne(a):
    """float32 -> float32 holding the bf16 value nearest to it (ties to even): v_cvt_pk_bf16_f32, f32_to_bf16_rne"""
    b = np.ascontiguousarray(a, F32).view(np.uint32)
    return (((b + 0x7FFF + ((b >> 16) & 1)) >> 16) << 16).astype(np.uint32).view(F32)


def split(a):
    """split_w8 / the passes' activation split: hi = RNE(a), lo = RNE(a - hi), as float32 arrays"""
    a = np.ascontiguousarray(a, F32)
    hi = bf16_rne(a)
    return hi, bf16_rne((a - hi).astype(F32))


def bits(a):
    """float32 that holds bf16 values -> their uint16 bit patterns"""
    b = np.ascontiguousarray(a, F32).view(np.uint32)
    assert not (b & 0xFFFF).any()
    return (b >> 16).astype(np.uint16)


def widen(b):
    return (np.asarray(b, np.uint16).astype(np.uint32) << 16).view(F32)


# ------------------------------------------------------------------------------------------------ blocks of every type
def blocks_of(ttype, p, shape):
    """the parameters of one matrix -> (the tensor rca_lm_create takes, its float32 values by the type's restated rule)"""
    from realtime_codec_agent_amd import _native as N
    n, k = shape
    if ttype == "bf16":
        return bits(p["w"]), np.array(p["w"], F32)
    if ttype == "f16":
        h = np.asarray(p["w"]).astype(np.float16)
        return h, h.astype(F32)
    if ttype == "q8_0":
        q, d = p["q"].astype(np.int8), p["d"].astype(np.float16)
        raw = np.concatenate([d.reshape(-1, 1).view(np.uint8), q.reshape(-1, 32).view(np.uint8)], axis=1)
        return N.Q8Blocks(raw, shape), q8_ref.dequantize_q8_0(q, d).astype(F32)
    if ttype == "q4_k":
        raw = q4k_ref.pack_blocks(p)
        return N.Q4KBlocks(raw, shape), q4k_ref.dequantize_blocks(raw).reshape(shape)
    if ttype == "q5_k":
        raw = q5k_ref.pack_blocks(p)
        return N.Q5KBlocks(raw, shape), q5k_ref.dequantize_blocks(raw).reshape(shape)
    if ttype == "q6_k":
        raw = q4k_ref.pack_blocks_q6_k(p)
        return N.Q6KBlocks(raw, shape), q4k_ref.dequantize_blocks_q6_k(raw).reshape(shape)
    if ttype in ("q4_0", "q4_1"):
        t = q40_ref.KINDS[ttype]
        raw = q40_ref.pack_blocks(p)
        return q40_ref.block_class(t)(raw, shape), q40_ref.dequantize_blocks(raw, t).reshape(shape)
    t = {"iq4_nl": iq4_ref.IQ4_NL, "iq4_xs": iq4_ref.IQ4_XS}[ttype]
    raw = iq4_ref.pack_iq4_nl(p) if ttype == "iq4_nl" else iq4_ref.pack_iq4_xs(p)
    return iq4_ref.block_class(t)(raw, shape), iq4_ref.dequantize_blocks(raw, t).reshape(shape)


def _f16(a):
    return np.asarray(a, np.float64).astype(np.float16)


def _pow2(rng, shape, lo, hi):
    return 2.0 ** rng.integers(lo, hi + 1, shape)


def normal_params(ttype, n, k, rng):
    """class b / c weights: normal data, sigma 0.05, quantised by the tree's own numpy rules"""
    w = (rng.standard_normal((n, k)) * 0.05).astype(F32)
    if ttype == "bf16":
        return dict(w=bf16_rne(w))
    if ttype == "f16":
        return dict(w=w)
    if ttype == "q8_0":
        q, d = q8_ref.quantize_q8_0(w)
        return dict(q=q, d=d)
    if ttype == "q4_k":
        return q4k_ref.quantize_q4_k(w)
    if ttype == "q5_k":
        return q5k_ref.quantize_q5_k(w)
    if ttype == "q6_k":
        return q4k_ref.quantize_q6_k(w)
    if ttype in ("q4_0", "q4_1"):
        return q40_ref.quantize(w, q40_ref.KINDS[ttype])
    if ttype == "iq4_nl":
        return iq4_ref.quantize_iq4_nl(w)
    # IQ4_XS has no load-time rule: the plausible blocks the file tests use (both signs of d, many ls), taken apart again
    xs = iq4_ref.xs_blocks_of(w, rng)
    q, d, ls = iq4_ref.unpack(xs.raw, iq4_ref.IQ4_XS)
    return dict(q=q.reshape(n, k), d=d.reshape(n, k // 32)[:, ::8].astype(np.float16), ls=ls.reshape(n, k // 32))


def int_params(ttype, n, k, rng):
    """class a weights: every value an integer (power-of-two d / dmin, integer scales).  32-value blocks alternate between BIG -- as
    many significant bits as the type reaches, so w_lo != 0 where it can be -- and SMALL (at most 8 significant bits: w_lo = 0), the
    columns on which the activations carry an x_lo."""
    kb = k // 32
    big = (np.arange(kb) % 2 == 0)[None, :].repeat(n, axis=0)                      # [n, kb]
    bigk = big.repeat(32, axis=1)
    ri = lambda lo, hi, shape: rng.integers(lo, hi + 1, shape)   # noqa: E731
    if ttype in ("bf16", "f16"):
        top = 255 if ttype == "bf16" else 2047
        return dict(w=np.where(bigk, ri(-top, top, (n, k)), ri(-15, 15, (n, k))).astype(F32))
    if ttype == "q8_0":
        return dict(q=np.where(bigk, ri(-127, 127, (n, k)), ri(-15, 15, (n, k))), d=_f16(np.where(big, _pow2(rng, (n, kb), 0, 2), 1.0)))
    if ttype in ("q4_k", "q5_k"):
        d = _f16(_pow2(rng, (n, k // 256), 0, 1))
        return dict(q=ri(0, 15 if ttype == "q4_k" else 31, (n, k)).astype(np.uint8), sc=np.where(big, ri(1, 63, (n, kb)), 1).astype(np.uint8),
                    m=np.where(big, ri(0, 63, (n, kb)), ri(0, 7, (n, kb))).astype(np.uint8), d=d, dmin=_f16(_pow2(rng, (n, k // 256), 0, 1)))
    if ttype == "q6_k":
        big16 = big.repeat(2, axis=1)
        sc = np.where(big16, ri(1, 127, (n, 2 * kb)) * rng.choice([-1, 1], (n, 2 * kb)), rng.choice([-1, 1], (n, 2 * kb)))
        sc = np.where(big16 & (rng.random((n, 2 * kb)) < 0.05), -128, sc)
        return dict(q=ri(-32, 31, (n, k)).astype(np.int8), sc=sc.astype(np.int8), d=_f16(_pow2(rng, (n, k // 256), 0, 1)))
    if ttype == "q4_0":
        return dict(q=ri(0, 15, (n, k)).astype(np.uint8), d=_f16(np.where(big, _pow2(rng, (n, kb), 0, 4) * rng.choice([-1, 1], (n, kb)), 1.0)))
    if ttype == "q4_1":
        return dict(q=ri(0, 15, (n, k)).astype(np.uint8), d=_f16(np.where(big, _pow2(rng, (n, kb), 0, 2), 1.0)),
                    m=_f16(np.where(big, ri(-1024, 1024, (n, kb)), ri(-4, 4, (n, kb)))))
    if ttype == "iq4_nl":
        return dict(q=ri(0, 15, (n, k)).astype(np.uint8), d=_f16(np.where(big, _pow2(rng, (n, kb), 0, 3) * rng.choice([-1, 1], (n, kb)), 1.0)))
    ls = np.where(big, ri(0, 63, (n, kb)), rng.choice([31, 33], (n, kb)))
    return dict(q=ri(0, 15, (n, k)).astype(np.uint8), d=_f16(rng.choice([-1.0, 1.0], (n, k // 256))), ls=ls)


def _coh(rng, shape, exp):
    """(1 + 2 m 2^-7 + 2^-8) 2^exp, m in 0 .. 7: a tie between two bf16 values, which RNE resolves to the even one below it: hi =
    (1 + 2 m 2^-7) 2^exp, lo = +2^(exp - 8), the largest lo a weight can have (2^-8 |w| / 1.12 and more); an fp16 value"""
    return (1.0 + 2 * rng.integers(0, 8, shape) * 2.0 ** -7 + 2.0 ** -8) * 2.0 ** exp


def coherent_params(ttype, n, k, rng):
    """class d weights: all positive, every w_lo = +2^-8 of its binade: an fp16 factor (1 + 2 m 2^-7 + 2^-8) times powers of two only"""
    kb = k // 32
    if ttype == "bf16":      # no lo plane in this form: 8-bit values
        return dict(w=((1.0 + rng.integers(0, 32, (n, k)) * 2.0 ** -7) * 2.0 ** -4).astype(F32))
    if ttype == "f16":
        return dict(w=_coh(rng, (n, k), -4).astype(F32))
    if ttype == "q8_0":
        return dict(q=_pow2(rng, (n, k), 0, 6).astype(np.int8), d=_f16(_coh(rng, (n, kb), -10)))
    if ttype in ("q4_k", "q5_k"):
        return dict(q=_pow2(rng, (n, k), 0, 3 if ttype == "q4_k" else 4).astype(np.uint8), sc=_pow2(rng, (n, kb), 0, 2).astype(np.uint8),
                    m=np.zeros((n, kb), np.uint8), d=_f16(_coh(rng, (n, k // 256), -9)), dmin=_f16(np.zeros((n, k // 256))))
    if ttype == "q6_k":
        return dict(q=_pow2(rng, (n, k), 0, 4).astype(np.int8), sc=_pow2(rng, (n, 2 * kb), 0, 2).astype(np.int8), d=_f16(_coh(rng, (n, k // 256), -10)))
    if ttype == "q4_0":
        return dict(q=(8 + _pow2(rng, (n, k), 0, 2)).astype(np.uint8), d=_f16(_coh(rng, (n, kb), -6)))
    if ttype == "q4_1":
        return dict(q=_pow2(rng, (n, k), 0, 3).astype(np.uint8), d=_f16(_coh(rng, (n, kb), -7)), m=_f16(np.zeros((n, kb))))
    if ttype == "iq4_nl":    # kv[8] = 1 is the table's only power of two
        return dict(q=np.full((n, k), 8, np.uint8), d=_f16(_coh(rng, (n, kb), -4)))
    return dict(q=np.full((n, k), 8, np.uint8), d=_f16(_coh(rng, (n, k // 256), -8)), ls=32 + _pow2(rng, (n, kb), 0, 4).astype(np.int64))


WCLASSES = {"int": int_params, "normal": normal_params, "coherent": coherent_params}
WCLASS_OF = {"a": "int", "b": "normal", "c": "normal", "d": "coherent"}


@functools.lru_cache(maxsize=None)
def layer(model, fmt, wclass, vocab=VOCABS[0]):
    """-> (weights for rca_lm_create, {projection: float32 values [N, K]}): one layer whose every value is known"""
    from realtime_codec_agent_amd.llm import rope_inv_freq
    cfg = config(model, vocab)
    rng = np.random.default_rng([sorted(MODELS).index(model), FORMATS.index(fmt), sorted(WCLASSES).index(wclass), vocab])
    types = matrix_types(fmt, vocab)
    weights, values = {}, {}
    for p, shape in dims(model, vocab).items():
        weights[HF[p]], values[p] = blocks_of(types[p], WCLASSES[wclass](types[p], *shape, rng), shape)
        values[p].setflags(write=False)
    H = cfg.hidden
    weights["model.embed_tokens.weight"] = np.zeros((vocab, H), F32)
    for nm in ("model.norm.weight", "model.layers.0.input_layernorm.weight", "model.layers.0.post_attention_layernorm.weight"):
        weights[nm] = np.ones(H, F32)
    weights["rope.inv_freq"] = rope_inv_freq(cfg)
    return weights, values


def fused(values, kind):
    """the matrix a kind multiplies by, rows in the order of the reference's outputs: [q; k; v], o, [gate; up], down, head"""
    if kind == 0:
        return np.concatenate([values["q"], values["k"], values["v"]])
    if kind == 2:
        return np.concatenate([values["gate"], values["up"]])
    return values[{1: "o", 3: "down", 4: "head"}[kind]]


def is_bf16(fmt):
    return fmt == "bf16"


# ------------------------------------------------------------------------------------------------ activations
def act_int(W, M, seed):
    """class a planes for the matrix W [N, K] (integers): on the SMALL blocks (odd k / 32) x = +-(257 .. 271): x_lo = +-1 on the odd
    ones; on the BIG blocks |x| <= 3.  Each row keeps a random share of its columns, sized so that sum |w| |x| stays near 2^21."""
    rng = np.random.default_rng(seed)
    N, K = W.shape
    bigk = ((np.arange(K) // 32) % 2 == 0)
    x = np.where(bigk[None, :], rng.integers(-3, 4, (M, K)), rng.choice([-1, 1], (M, K)) * rng.integers(257, 272, (M, K))).astype(np.float64)
    worst = float((np.abs(W.astype(np.float64)) @ np.where(bigk, 3.0, 271.0)).max())
    x *= rng.random((M, K)) < min(1.0, 2.0 ** 21 / worst)
    hi, lo = split(x.astype(F32))
    return bits(hi), bits(lo)


def act_onehot(K, k0, M):
    """class b planes: token t reads column k0 + t"""
    xh = np.zeros((M, K), np.uint16)
    xh[np.arange(M), k0 + np.arange(M)] = 0x3F80
    return xh, np.zeros((M, K), np.uint16)


def act_normal(K, M, seed):
    """class c planes: sigma 1, split as the passes split their rows"""
    hi, lo = split(np.random.default_rng(seed).standard_normal((M, K)).astype(F32))
    return bits(hi), bits(lo)


def act_coherent(K, M, seed):
    """class d planes: xh = 1 + 2 m 2^-7, xl = +2^-8 (the split of the tie 1 + 2 m 2^-7 + 2^-8, as for the weights)"""
    rng = np.random.default_rng(seed)
    return bits((1.0 + 2 * rng.integers(0, 8, (M, K)) * 2.0 ** -7).astype(F32)), bits(np.full((M, K), 2.0 ** -8, F32))


# ------------------------------------------------------------------------------------------------ reference and bound
def gemm(W, xh, xl, bf16_weights, ns):
    """-> (y float64 [M, N], bound) of the GEMM alone (module docstring); ns: the slice count of the launch"""
    W64 = np.asarray(W, np.float64)
    h, l = widen(xh).astype(np.float64), widen(xl).astype(np.float64)
    x = h + l
    y = x @ W64.T
    S = (np.abs(h) + np.abs(l)) @ np.abs(W64).T
    K = W.shape[1]
    grp = g128_group(ns)
    acc = ((2 if bf16_weights else 3) * (K // ns) * U + ((grp + ns // grp) * u if ns > 1 else 0.0)) * S
    if bf16_weights:
        return y, acc
    hi, lo = split(W)
    res = np.abs(W64 - hi.astype(np.float64) - lo.astype(np.float64))
    return y, acc + np.abs(x) @ res.T + np.abs(l) @ np.abs(lo.astype(np.float64)).T


def rope_tables(inv_freq, pos):
    ang = (np.asarray(pos, F32)[:, None] * np.asarray(inv_freq, F32)[None, :]).astype(F32).astype(np.float64)   # the table's f32 angle
    return np.cos(ang), np.sin(ang)


def epilogue(kind, y, b, model, pos0=0, inv_freq=None):
    """the float64 epilogue of kind over the GEMM result y [M, N] known within b -> dict(y, bound [, k, k_bound, v, v_bound])"""
    if kind in (1, 3, 4):
        return dict(y=y, bound=b)
    M = y.shape[0]
    if kind == 2:
        F = y.shape[1] // 2
        g, up, bg, bu = y[:, :F], y[:, F:], b[:, :F], b[:, F:]
        with np.errstate(over="ignore"):
            s = g / (1.0 + np.exp(-g))
        h = s * up
        prop = 1.1 * np.abs(up) * bg + np.abs(s) * bu + 1.1 * bg * bu
        eps = (2.0 * np.abs(g) + 6.0) * u + 2.0 ** -17 + u
        return dict(y=h, bound=prop + eps * (np.abs(h) + prop) + 2.0 ** -120 * (1.0 + np.abs(up)))
    m = MODELS[model]
    nh, nkv = m["n_heads"], m["n_kv_heads"]
    cs, sn = (t[:, None, :] for t in rope_tables(inv_freq, pos0 + np.arange(M)))
    out = {}
    lo = 0
    for name, heads in (("y", nh), ("k", nkv), ("v", nkv)):
        yy, bb = y[:, lo:lo + heads * 64], b[:, lo:lo + heads * 64]
        lo += heads * 64
        if name != "v":
            yy, bb = yy.reshape(M, heads, 2, 32), bb.reshape(M, heads, 2, 32)
            x1, x2, b1, b2 = yy[:, :, 0], yy[:, :, 1], bb[:, :, 0], bb[:, :, 1]
            o1, o2 = x1 * cs - x2 * sn, x2 * cs + x1 * sn
            tab = 4 * u * (np.abs(x1) + b1 + np.abs(x2) + b2)
            r1 = 2 * u * (1 + 2.0 ** -20) * (np.abs(x1 * cs) + np.abs(x2 * sn)) + (np.abs(cs) + 4 * u) * b1 + (np.abs(sn) + 4 * u) * b2 + tab
            r2 = 2 * u * (1 + 2.0 ** -20) * (np.abs(x2 * cs) + np.abs(x1 * sn)) + (np.abs(cs) + 4 * u) * b2 + (np.abs(sn) + 4 * u) * b1 + tab
            yy, bb = np.stack([o1, o2], axis=2).reshape(M, heads * 64), np.stack([r1, r2], axis=2).reshape(M, heads * 64)
        out[name], out[name + "_bound" if name != "y" else "bound"] = yy, bb
    return out


def reference(model, fmt, kind, values, xh, xl, pos0=0, inv_freq=None, vocab=VOCABS[0]):
    """everything a GPU case compares with: the float64 result of kind and its bound"""
    W = fused(values, kind)
    N, K = kind_nk(model, kind, vocab)
    assert W.shape == (N, K)
    bf = matrix_types(fmt, vocab)[{0: "q", 1: "o", 2: "gate", 3: "down", 4: "head"}[kind]] == "bf16"
    if kind == 0 and matrix_types(fmt, vocab)["v"] != matrix_types(fmt, vocab)["q"]:      # two segments, two slice counts
        nqk = values["q"].shape[0] + values["k"].shape[0]
        parts = [gemm(W[:nqk], xh, xl, bf, g128_splits(nqk, K)), gemm(W[nqk:], xh, xl, bf, g128_splits(N - nqk, K))]
        y, b = np.concatenate([p[0] for p in parts], axis=1), np.concatenate([p[1] for p in parts], axis=1)
    else:
        y, b = gemm(W, xh, xl, bf, 1 if kind == 4 else g128_splits(N, K))
    # (kind 2: [gate; up] here, interleaved rows on the device: the order of the ROWS changes no sum)
    return epilogue(kind, y, b, model, pos0, inv_freq)


def f16_interval_ok(got16, want, bound):
    """K / V rows: the device rounds an f32 value within `bound` of `want` to fp16 (RNE, monotone)"""
    with np.errstate(over="ignore"):
        lo, hi = (want - bound).astype(np.float16), (want + bound).astype(np.float16)
    g = np.asarray(got16, np.float16)
    return (g >= lo) & (g <= hi)


def kernel_f32(W, xh, xl, bf16_weights, ns):
    """The kernel's own arithmetic restated in f32, for the bound's self-check: per slice an f32 accumulator takes, per 16 k, the
    exactly summed products of hi xh, hi xl [, lo xh] one MFMA after the other; the slices are added in the two levels of g128_group."""
    hi, lo = (np.asarray(W, F32), None) if bf16_weights else split(W)
    h, l = widen(xh).astype(np.float64), widen(xl).astype(np.float64)
    K = W.shape[1]
    ks = K // ns
    parts = []
    for s in range(ns):
        acc = np.zeros((xh.shape[0], W.shape[0]), F32)
        for k0 in range(s * ks, (s + 1) * ks, 16):
            a = hi[:, k0:k0 + 16].astype(np.float64)
            acc = (acc + h[:, k0:k0 + 16] @ a.T).astype(F32)
            acc = (acc + l[:, k0:k0 + 16] @ a.T).astype(F32)
            if lo is not None:
                acc = (acc + h[:, k0:k0 + 16] @ lo[:, k0:k0 + 16].astype(np.float64).T).astype(F32)
        parts.append(acc)
    grp = g128_group(ns)
    tot = np.zeros_like(parts[0])
    for g0 in range(0, ns, grp):
        gs = np.zeros_like(tot)
        for s in range(g0, g0 + grp):
            gs = (gs + parts[s]).astype(F32)
        tot = (tot + gs).astype(F32)
    return tot


def ratio(err, bound):
    """worst err / bound; an error where the bound is 0 counts as infinite"""
    err, bound = np.asarray(err, np.float64), np.asarray(bound, np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0))
    return float(r.max()) if r.size else 0.0
