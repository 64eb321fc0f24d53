"""Cases, float64 reference and error bound of the decode GEMVs run alone (rca_lm_gemv_tap, f32 activations: ACT = 0), shared by
tests/test_gemv_cpu.py (do the cases reach their seams, does the bound have teeth and room?) and tests/test_gemv_gpu.py (does
lm_gemv_kernel compute it, in every weight form, stage and launch geometry?).  No GPU is used here.

THE OPERATION.  y[m][n] = sum_k W[n][k] h[m][k], then the stage's epilogue.  h is the f32 input row itself (kinds 1 O, 3 down) or
the RMSNorm of the f32 residual row, (x * rsqrt(mean(x^2) + eps)) * norm_w (kinds 0 QKV, 2 gate/up, 4 head): the reference
normalises in float64.  W[n][k] is the ONE f32 value the format's de-quantisation rule gives (gemm128_ref.blocks_of).

THE KERNEL'S TERM STRUCTURE (lm_gemv_body).  The four waves split the K / 8 chunks of 8 values, cpw = ceil(K / 8 / 4) each; lane l of
a wave takes chunks l, l + 64, .. (NIT of them) of the wave's range.  Per lane and output:
  * bf16 / f16: ONE fma chain over its 8 NIT products.
  * q8_0 / Q6_K / IQ4_NL / IQ4_XS: per chunk p = an 8-fma chain of (float)q x from 0 (kv[q] for IQ4), then acc = fma(s, p, acc) with the
    chunk's scale s (fp16 d; the exact f32 products d * sc of Q6_K and d (ls - 32) of IQ4_XS).
  * Q4_K / Q5_K / Q4_0 / Q4_1: the same with s = d1, then acc = fma(-m1, sx, acc): sx is the sequential f32 sum of the chunk's 8 x values,
    d1 = d * sc and m1 = dmin * m are exact products (Q4_0: (d, 8 d); Q4_1: (d, -m)).
Then wave_reduce_transposed adds the 64 lanes in 2 + 4 levels and the first threads add the four waves in order: 3 more additions.

THE BOUND, per output element, with u = 2^-24 and gamma(n) = n u / (1 - n u) (n roundings on the path of a term to the sum; an
addition's error is within u of a partial sum, which the magnitude sum below bounds):
  * bf16 / f16: gamma(8 NIT + 9) S, S = sum_k |w| |h|.
  * q8_0 / Q6_K / IQ4: gamma(8 + NIT + 9) sum_chunks |s| sum |q| |h| (= S, every product s q being exact).
  * Q4_K / Q5_K / Q4_0 / Q4_1: gamma(8 + 2 NIT + 9) sum_chunks (|d1| sum |q| |h| + |m1| sum |h|): the chain of sx has 7 roundings, one fewer
    than the products', and its magnitude |m1| sum |h| belongs here because d1 p and m1 sx cancel.  The reference multiplies the
    format's f32 value round(d1 q - m1) while the kernel never forms it: + u S for that rounding.
  * prologue (kinds 0, 2, 4; NIT = 1): the sum of squares is an 8-fma chain, 6 + 3 additions of non-negative terms: 17 u relative; / K and
    + eps: 2 u; rsqrtf halves the relative error of its argument (9.5 u) and adds its own: the HIP math API's accuracy table lists
    rsqrtf at 1 ulp = 2 u, the figure taken here; (x * rstd) * w: 2 u.  C_PRO = 13.5: every h is within 13.5 u of the float64 one,
    which passes through the GEMV as C_PRO u (magnitude sum above).
  * one factor (1 + 2^-20) over all of it for second-order terms and for the magnitude sums being formed from the float64 h.
  * epilogues: RoPE and SwiGLU as in gemm128_ref (two products and a sum; table entries cosf / sinf of the f32 angle at 1 ulp; __expf at
    1 ulp, a correctly rounded division), without that module's bf16 output planes; K / V rows are fp16 roundings of a value in the
    bound's interval (gemm128_ref.f16_interval_ok); residual (the tap zeroes it) and logits add nothing.
Nothing is fitted to a device's output: a correct kernel outside this bound means a missing term, which is to be found and named.
"""
import functools

import numpy as np

import gemm128_ref as G
import iq4_ref

u = 2.0 ** -24
F32 = np.float32
C_PRO = 13.5
SLACK = 1.0 + 2.0 ** -20
KINDS = G.KINDS
FORMATS = G.FORMATS
PROJ_OF_KIND = {0: ("q", "k", "v"), 1: ("o",), 2: ("gate", "up"), 3: ("down",), 4: ("head",)}
FORMAT_ID = {"bf16": 0, "q8_0": 1, "f16": 2, "q4_k": 3, "q6_k": 4, "q5_k": 5, "q4_0": 6, "q4_1": 7, "iq4_nl": 8, "iq4_xs": 9}
FOUR_BIT = ("q4_k", "q5_k", "q4_0", "q4_1", "iq4_nl", "iq4_xs")
PAIR = ("q8_0", "q6_k")
MIN_FORMS = ("q4_k", "q5_k", "q4_0", "q4_1")
N_CTX = 256
POS0 = 5


def cdiv(a, b):
    return -(-a // b)


def gamma(n):
    return n * u / (1.0 - n * u)


# ------------------------------------------------------------------------------------------------ launch rules (rca_lm.hip restated)
GEOM_DEFAULT = {0: (4, 1), 1: (4, 1), 2: (16, 2), 3: (4, 1), 4: (16, 8)}


def gemv_instance(kind, ttype, N, K, M, geom=None):
    """-> (NIT, R, batches_per_wg, grid) of the launch of one matrix [N, K] of type ttype: gemv_geom (defaults or an RCA_GEMV_* pair, then
    the 64-workgroup rule), launch_gemv_q (loads per row, the load limit, the minimum R of 8 of the 4-bit forms and Q6_K), nit == 3 -> 4,
    launch_gemv_r's grid.  M (1 or 2) changes nothing here; it is the instance's first template argument."""
    assert M in (1, 2)
    R, bpw = geom or GEOM_DEFAULT[kind]
    while bpw > 1 and cdiv(N, R * bpw) < 64:
        bpw >>= 1
    nit = cdiv(cdiv(K >> 3, 4), 64)
    nit_t = 4 if nit == 3 else nit
    four = ttype in FOUR_BIT
    lpr = 2 if ttype in PAIR else (4 if four else 1)
    max_loads = 8 if four else 16
    while R > 4 and (R // lpr) * nit_t > max_loads:
        R >>= 1
    if (four or ttype == "q6_k") and R < 8:
        R = 8
    NIT = nit_t if (kind in (1, 3) and nit > 1) else 1
    assert nit == 1 or kind == 3, "only the down projection is wider than 2048"
    return NIT, R, bpw, cdiv(cdiv(N, R), bpw)


def wave_chunks(K):
    """-> (cpw, [chunks of wave 0..3]): cpw = ceil(K / 8 / 4), cn = max(0, min(cpw, nchunk - wave * cpw))"""
    nchunk = K >> 3
    cpw = (nchunk + 3) >> 2
    return cpw, [max(0, min(cpw, nchunk - w * cpw)) for w in range(4)]


def row_of(b, r, R, qkv):
    """slot r of batch b -> weight row (EPI 2 pairs rows (d, d + 32) of one head)"""
    if qkv:
        pair = b * (R // 2) + (r >> 1)
        return (pair >> 5) * 64 + (pair & 31) + 32 * (r & 1)
    return b * R + r


def lane_index(K, NIT):
    """idx[wave][it][lane] = the chunk a lane multiplies, K / 8 (a chunk of zeros) where the lane is idle"""
    nchunk = K >> 3
    cpw, cns = wave_chunks(K)
    assert cpw <= 64 * NIT
    idx = np.full((4, NIT, 64), nchunk, np.int64)
    for w in range(4):
        for it in range(NIT):
            c = np.arange(64) + 64 * it
            idx[w, it] = np.where(c < cns[w], w * cpw + c, nchunk)
    return idx


# ------------------------------------------------------------------------------------------------ models
ALL5 = (0, 1, 2, 3, 4)
MODELS = {"P": dict(hidden=136, n_heads=4, n_kv_heads=2, ffn=264),      # K = 136: 17 chunks, 5 / 5 / 5 / 2; down K = 264: 9 / 9 / 9 / 6; AO = 256 != hidden
          "Q": dict(hidden=264, n_heads=4, n_kv_heads=2, ffn=136),      # the two widths exchanged: K = 264 under the prologue
          "S": dict(hidden=256, n_heads=4, n_kv_heads=1, ffn=768),      # K = 256: 8 chunks per wave, 56 idle lanes; G = 4
          "T": dict(hidden=768, n_heads=12, n_kv_heads=12, ffn=256),    # K = 768: 24 per wave; G = 1
          "W": dict(hidden=2048, n_heads=4, n_kv_heads=4, ffn=256),     # K = 2048: every lane busy
          "D4": dict(hidden=256, n_heads=4, n_kv_heads=2, ffn=4096),    # down: NIT = 2; G = 2
          "D6": dict(hidden=256, n_heads=4, n_kv_heads=2, ffn=6144),    # down: nit == 3, the NIT = 4 instance with an empty fourth chunk
          "D8": dict(hidden=256, n_heads=4, n_kv_heads=2, ffn=8192)}    # down: NIT = 4; gate/up keeps 2 batches per workgroup; head 8204
FORMATS_OF = {"P": ("bf16", "f16"), "Q": ("bf16", "f16"), "S": FORMATS, "T": FORMATS, "W": ("bf16", "q8_0", "q4_k"), "D4": FORMATS, "D6": FORMATS, "D8": FORMATS}
KINDS_OF = {"P": ALL5, "Q": ALL5, "S": ALL5, "T": ALL5, "W": ALL5, "D4": (3,), "D6": (3,), "D8": (2, 3, 4)}
SECOND_TYPE = ("T", "D6")      # models whose head takes the second type of a pair (q4_1, iq4_xs): gemm128_ref.matrix_types
VOCAB_BIG = 8204               # head: 513 batches of 16, 8 per workgroup, the 65th workgroup holds one batch of 12 rows
MODEL_FORMATS = [(m, f) for m in MODELS for f in FORMATS_OF[m]]
STAGES = [(m, f, k) for m, f in MODEL_FORMATS for k in KINDS_OF[m]]


def types_of(model, fmt):
    return G.matrix_types(fmt, G.VOCABS[1] if model in SECOND_TYPE else G.VOCABS[0])


def vocab_of(model, fmt):
    """ragged N: 1001 (16-bit rows: the last batch of 16 holds 9), 1002 (pair forms), 1004 (quad forms: the last batch is one quad)"""
    if model == "D8":
        return VOCAB_BIG
    t = types_of(model, fmt)["head"]
    return 1001 if t in ("bf16", "f16") else (1002 if t in PAIR else 1004)


def dims(model, vocab):
    m = MODELS[model]
    H, AO, KV, F = m["hidden"], m["n_heads"] * 64, m["n_kv_heads"] * 64, m["ffn"]
    return {"q": (AO, H), "k": (KV, H), "v": (KV, H), "o": (H, AO), "gate": (F, H), "up": (F, H), "down": (H, F), "head": (vocab, H)}


def config(model, fmt):
    from realtime_codec_agent_amd.llm import LMConfig
    return LMConfig(vocab_size=vocab_of(model, fmt), n_layers=1, head_dim=64, rope_scaling=None, rope_theta=10000.0, **MODELS[model])


def launches(model, fmt, kind):
    """[(type, N, K)] of the launches a stage makes: one, or two where the layer keeps V apart"""
    t, d = types_of(model, fmt), dims(model, vocab_of(model, fmt))
    if kind == 0:
        K = d["q"][1]
        if t["v"] != t["q"]:
            return [(t["q"], d["q"][0] + d["k"][0], K), (t["v"], d["v"][0], K)]
        return [(t["q"], d["q"][0] + 2 * d["k"][0], K)]
    if kind == 2:
        return [(t["gate"], 2 * d["gate"][0], d["gate"][1])]
    p = PROJ_OF_KIND[kind][0]
    return [(t[p],) + d[p]]


# ------------------------------------------------------------------------------------------------ weights
def _h(a):
    return np.asarray(a, np.float64).astype(np.float16)


def rand_params(ttype, n, k, rng):
    """classes b / c: random blocks whose values have a sigma near 0.05: every field of every format takes many values"""
    kb, ksb = k // 32, k // 256
    ri = lambda lo, hi, shape: rng.integers(lo, hi + 1, shape)   # noqa: E731
    uni = lambda shape: rng.uniform(0.5, 1.5, shape)             # noqa: E731
    sgn = lambda shape: rng.choice([-1.0, 1.0], shape)           # noqa: E731
    if ttype == "bf16":
        return dict(w=G.bf16_rne((rng.standard_normal((n, k)) * 0.05).astype(F32)))
    if ttype == "f16":
        return dict(w=(rng.standard_normal((n, k)) * 0.05).astype(np.float16).astype(F32))
    if ttype == "q8_0":
        return dict(q=ri(-127, 127, (n, k)).astype(np.int8), d=_h(7e-4 * uni((n, kb))))
    if ttype in ("q4_k", "q5_k"):
        top = 15 if ttype == "q4_k" else 31
        sc = ri(1, 63, (n, kb))
        return dict(q=ri(0, top, (n, k)).astype(np.uint8), sc=sc.astype(np.uint8), m=np.clip(sc + ri(-6, 6, (n, kb)), 0, 63).astype(np.uint8),
                    d=_h(6e-3 / top * uni((n, ksb))), dmin=_h(3e-3 * uni((n, ksb))))
    if ttype == "q6_k":
        return dict(q=ri(-32, 31, (n, k)).astype(np.int8), sc=(ri(1, 127, (n, 2 * kb)) * sgn((n, 2 * kb))).astype(np.int8), d=_h(4e-5 * uni((n, ksb))))
    if ttype == "q4_0":
        return dict(q=ri(0, 15, (n, k)).astype(np.uint8), d=_h(1e-2 * uni((n, kb)) * sgn((n, kb))))
    if ttype == "q4_1":
        return dict(q=ri(0, 15, (n, k)).astype(np.uint8), d=_h(1e-2 * uni((n, kb))), m=_h(-7.5e-2 * uni((n, kb))))
    if ttype == "iq4_nl":
        return dict(q=ri(0, 15, (n, k)).astype(np.uint8), d=_h(7e-4 * uni((n, kb)) * sgn((n, kb))))
    return dict(q=ri(0, 15, (n, k)).astype(np.uint8), d=_h(4e-5 * uni((n, ksb)) * sgn((n, ksb))), ls=ri(0, 63, (n, kb)))


def int_params(ttype, n, k, rng):
    """class a: gemm128_ref's integer blocks; 16-bit rows of any width (K = 136 has no 32-value blocks)"""
    if ttype in ("bf16", "f16"):
        top = 255 if ttype == "bf16" else 2047
        return dict(w=rng.integers(-top, top + 1, (n, k)).astype(F32))
    return G.int_params(ttype, n, k, rng)


WCLASSES = {"int": int_params, "rand": rand_params, "coherent": G.coherent_params}
WCLASS_OF = {"a": "int", "b": "rand", "c": "rand", "d": "coherent"}
NORMS = {0: "model.layers.0.input_layernorm.weight", 2: "model.layers.0.post_attention_layernorm.weight", 4: "model.norm.weight"}


def chunk_form(ttype, p):
    """the factors of the kernel's per-chunk arithmetic -> (qf [n, k], s [n, k / 8], m1 [n, k / 8] or None), float64 holding f32 values;
    None for the 16-bit forms"""
    f = lambda a: np.asarray(a, np.float16).astype(F32)   # noqa: E731
    rep = lambda a, r: np.repeat(np.asarray(a, F32), r, axis=1).astype(np.float64)   # noqa: E731
    if ttype in ("bf16", "f16"):
        return None
    if ttype == "q8_0":
        return p["q"].astype(np.float64), rep(f(p["d"]), 4), None
    if ttype in ("q4_k", "q5_k"):
        d1 = np.repeat(f(p["d"]), 8, axis=1) * p["sc"].astype(F32)
        m1 = np.repeat(f(p["dmin"]), 8, axis=1) * p["m"].astype(F32)
        return p["q"].astype(np.float64), rep(d1, 4), rep(m1, 4)
    if ttype == "q6_k":
        return p["q"].astype(np.float64), rep(np.repeat(f(p["d"]), 16, axis=1) * p["sc"].astype(F32), 2), None
    if ttype == "q4_0":
        return p["q"].astype(np.float64), rep(f(p["d"]), 4), rep((f(p["d"]) * F32(8.0)).astype(np.float16), 4)
    if ttype == "q4_1":
        return p["q"].astype(np.float64), rep(f(p["d"]), 4), rep(-f(p["m"]), 4)
    kv = iq4_ref.KV.astype(np.float64)[p["q"]]
    if ttype == "iq4_nl":
        return kv, rep(f(p["d"]), 4), None
    return kv, rep(np.repeat(f(p["d"]), 8, axis=1) * (np.asarray(p["ls"]).astype(F32) - F32(32.0)), 4), None


def magnitude_matrix(ttype, W, form):
    """[n, k] float64: what |h| is multiplied by in the bound's magnitude sum: |w|, or |d1| |q| + |m1| for the forms with a minimum"""
    if form is None or form[2] is None:
        return np.abs(np.asarray(W, np.float64))
    qf, s, m1 = form
    return np.abs(np.repeat(s, 8, axis=1) * qf) + np.abs(np.repeat(m1, 8, axis=1))


@functools.lru_cache(maxsize=4)
def layer(model, fmt, wclass):
    """-> dict(weights for rca_lm_create, values {projection: f32 [N, K]}, params, types, norms {kind: f32 [hidden]}, inv_freq, config)"""
    from realtime_codec_agent_amd.llm import rope_inv_freq
    cfg = config(model, fmt)
    vocab = cfg.vocab_size
    rng = np.random.default_rng([77, sorted(MODELS).index(model), FORMATS.index(fmt), sorted(WCLASSES).index(wclass)])
    types = types_of(model, fmt)
    weights, values, params = {}, {}, {}
    for p, shape in dims(model, vocab).items():
        params[p] = WCLASSES[wclass](types[p], *shape, rng)
        weights[G.HF[p]], values[p] = G.blocks_of(types[p], params[p], shape)
        values[p].setflags(write=False)
    H = cfg.hidden
    weights["model.embed_tokens.weight"] = np.zeros((vocab, H), F32)
    norms = {}
    for kind, nm in NORMS.items():      # a weight per column, all different: one read from another chunk shows
        norms[kind] = (0.75 + 0.5 * rng.random(H)).astype(F32)
        weights[nm] = norms[kind]
    weights["rope.inv_freq"] = rope_inv_freq(cfg)
    return dict(weights=weights, values=values, params=params, types=types, norms=norms, inv_freq=weights["rope.inv_freq"], config=cfg)


# ------------------------------------------------------------------------------------------------ activations
def kind_k(model, kind):
    m = MODELS[model]
    return {0: m["hidden"], 1: m["n_heads"] * 64, 2: m["hidden"], 3: m["ffn"], 4: m["hidden"]}[kind]


def act_int(mags, K, seed):
    """class a rows [2, K] (kinds 1, 3): integers in -3 .. 3 on a random share of the columns, sized so that every magnitude sum -- and so
    every partial sum in any order -- stays below 2^22"""
    rng = np.random.default_rng(seed)
    worst = max(float(m.sum(axis=1).max()) for m in mags) * 3.0
    x = rng.integers(-3, 4, (2, K)) * (rng.random((2, K)) < min(1.0, 2.0 ** 22 / worst))
    return x.astype(F32)


def act_normal(K, kind, seed):
    """class c rows [2, K]: sigma 1; under a prologue the second row has sigma 2^-6, where eps is 4 % of the mean square"""
    x = np.random.default_rng(seed).standard_normal((2, K))
    if kind in NORMS:
        x[1] *= 2.0 ** -6
    return x.astype(F32)


def act_coherent(K, kind, seed):
    """class d rows [2, K]: all positive, 1 + m 2^-7 (second row under a prologue: times 2^-6)"""
    x = 1.0 + np.random.default_rng(seed).integers(0, 128, (2, K)) * 2.0 ** -7
    if kind in NORMS:
        x[1] *= 2.0 ** -6
    return x.astype(F32)


def onehot_columns(K, NIT):
    """class b: every k up to 512; beyond, at most 256 columns that hold the first and the last column of each wave's range and of each
    `it` step of it, the rest spread evenly"""
    if K <= 512:
        return np.arange(K)
    seam = seam_columns(K, NIT)
    rest = [int(k) for k in np.linspace(0, K - 1, 256 - len(seam)).astype(int) if k not in seam]
    if (len(seam) + len(set(rest))) % 2:
        rest = rest[1:]
    return np.array(sorted(seam | set(rest)))


def seam_columns(K, NIT):
    cpw, cns = wave_chunks(K)
    out = set()
    for w in range(4):
        for it in range(NIT):
            lo, hi = 64 * it, min(cns[w], 64 * (it + 1)) - 1
            if lo <= hi:
                out |= {8 * (w * cpw + lo), 8 * (w * cpw + hi) + 7}
    return out


def act_onehot(K, cols):
    x = np.zeros((len(cols), K), F32)
    x[np.arange(len(cols)), cols] = 1.0
    return x


# ------------------------------------------------------------------------------------------------ reference and bound
def rms_norm64(x, w, eps):
    x = np.asarray(x, np.float64)
    return x / np.sqrt((x * x).mean(axis=-1, keepdims=True) + float(F32(eps))) * np.asarray(w, np.float64)


def depth(ttype, NIT):
    if ttype in ("bf16", "f16"):
        return 8 * NIT + 9
    return 8 + (2 if ttype in MIN_FORMS else 1) * NIT + 9


def gemv(W, ttype, form, h, NIT, pro):
    """-> (y float64 [M, N], bound) of one matrix over the float64 rows h"""
    W64 = np.asarray(W, np.float64)
    y = h @ W64.T
    mag = np.abs(h) @ magnitude_matrix(ttype, W, form).T
    b = (gamma(depth(ttype, NIT)) + (C_PRO * u if pro else 0.0)) * mag
    if ttype in MIN_FORMS:
        b = b + u * (np.abs(h) @ np.abs(W64).T)
    return y, b * SLACK


def epilogue(kind, y, b, nh, nkv, pos, inv_freq=None):
    """the float64 epilogue of kind over the sums y [M, N] known within b -> dict(y, bound [, k, k_bound, v, v_bound]); pos: the rows' positions"""
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
        eps = (2.0 * np.abs(g) + 6.0) * u
        return dict(y=h, bound=prop + eps * (np.abs(h) + prop) + 2.0 ** -120 * (1.0 + np.abs(up)))
    cs, sn = (t[:, None, :] for t in G.rope_tables(inv_freq, np.asarray(pos)))
    out, lo = {}, 0
    for name, heads in (("y", nh), ("k", nkv), ("v", nkv)):
        yy, bb = y[:, lo:lo + heads * 64], b[:, lo:lo + heads * 64]
        lo += heads * 64
        if name != "v":
            yy, bb = yy.reshape(M, heads, 2, 32), bb.reshape(M, heads, 2, 32)
            x1, x2, b1, b2 = yy[:, :, 0], yy[:, :, 1], bb[:, :, 0], bb[:, :, 1]
            o1, o2 = x1 * cs - x2 * sn, x2 * cs + x1 * sn
            tab = 4 * u * (np.abs(x1) + b1 + np.abs(x2) + b2)
            r1 = 2 * u * SLACK * (np.abs(x1 * cs) + np.abs(x2 * sn)) + (np.abs(cs) + 4 * u) * b1 + (np.abs(sn) + 4 * u) * b2 + tab
            r2 = 2 * u * SLACK * (np.abs(x2 * cs) + np.abs(x1 * sn)) + (np.abs(cs) + 4 * u) * b2 + (np.abs(sn) + 4 * u) * b1 + tab
            yy, bb = np.stack([o1, o2], axis=2).reshape(M, heads * 64), np.stack([r1, r2], axis=2).reshape(M, heads * 64)
        out[name], out[name + "_bound" if name != "y" else "bound"] = yy, bb
    return out


class Stage:
    """one stage of one layer: the float64 matrices of its reference and bound, formed once"""

    def __init__(self, model, fmt, kind, L):
        self.kind, self.L, self.K, self.pro = kind, L, kind_k(model, kind), kind in NORMS
        self.parts = []
        for p in PROJ_OF_KIND[kind]:
            t, W = L["types"][p], L["values"][p]
            NIT = gemv_instance(kind, t, W.shape[0], self.K, 1)[0]
            c = gamma(depth(t, NIT)) + (C_PRO * u if self.pro else 0.0)
            W64 = W.astype(np.float64)
            self.parts.append((W64.T.copy(), c * magnitude_matrix(t, W, chunk_form(t, L["params"][p])).T + (u * np.abs(W64).T if t in MIN_FORMS else 0.0)))

    def __call__(self, x, pos0=POS0):
        """x: f32 rows [M, K] at positions pos0 .. -> dict(y, bound [, k, k_bound, v, v_bound])"""
        cfg = self.L["config"]
        assert x.shape[1] == self.K and x.dtype == F32
        h = rms_norm64(x, self.L["norms"][self.kind], cfg.rms_eps) if self.pro else x.astype(np.float64)
        y = np.concatenate([h @ Wt for Wt, _ in self.parts], axis=1)
        b = np.concatenate([np.abs(h) @ Bt for _, Bt in self.parts], axis=1) * SLACK
        return epilogue(self.kind, y, b, cfg.n_heads, cfg.n_kv_heads, pos0 + np.arange(x.shape[0]), self.L["inv_freq"])


@functools.lru_cache(maxsize=2)
def stage(model, fmt, kind, wclass):
    return Stage(model, fmt, kind, layer(model, fmt, wclass))


def reference(model, fmt, kind, L, x, pos0=POS0):
    """everything a case compares with: the float64 result of the stage over the f32 rows x [M, K] at positions pos0 .., and its bound.
    L = layer(model, fmt, class)."""
    return Stage(model, fmt, kind, L)(x, pos0)


f16_interval_ok = G.f16_interval_ok
ratio = G.ratio


# ------------------------------------------------------------------------------------------------ the kernel's order in f32
def _r(a):
    return np.asarray(a, np.float64).astype(F32).astype(np.float64)


def _fma(a, b, c):
    """f32 fma through float64: the product of two f32 values is exact there, the sum rounds to 53 bits and then to 24"""
    return _r(a * b + c)


def _tree(v):
    """[..., 4, 64] lane values -> [...] : xor 32, xor 16, then the four DPP steps of a row of 16; then the waves in order"""
    v = _r(v[..., :32] + v[..., 32:])
    v = _r(v[..., :16] + v[..., 16:])
    v = _r(v[..., :8] + v[..., 8:])
    v = _r(v[..., :4] + v[..., 4:])
    v = _r(v[..., :2] + v[..., 2:])
    v = _r(v[..., 0] + v[..., 1])
    return _r(_r(_r(v[..., 0] + v[..., 1]) + v[..., 2]) + v[..., 3])


def _lanes(a, idx):
    """[r, K] -> [r, 4, NIT, 64, 8] by the lane index, zeros where a lane is idle"""
    r, K = a.shape
    pad = np.concatenate([np.asarray(a, np.float64).reshape(r, K // 8, 8), np.zeros((r, 1, 8))], axis=1)
    return pad[:, idx]


FAULTS = ("x_bf16", "scale_f16_twice", "drop_last_min", "drop_chunk", "no_eps", "rope_neighbour")


def prologue_f32(x, w, eps, fault=None):
    x = np.asarray(x, F32)
    K = x.shape[1]
    idx = lane_index(K, 1)
    xc = _lanes(x, idx)[:, :, 0]                       # [M, 4, 64, 8]
    ss = np.zeros(xc.shape[:-1])
    for j in range(8):
        ss = _fma(xc[..., j], xc[..., j], ss)
    tot = _tree(ss)                                    # [M]
    arg = _r(_r(tot / F32(K)) + (0.0 if fault == "no_eps" else float(F32(eps))))
    rstd = _r(1.0 / np.sqrt(arg))
    return _r(_r(x.astype(np.float64) * rstd[:, None]) * np.asarray(w, np.float64)[None, :]).astype(F32)


def gemv_f32(W, ttype, form, h, NIT, fault=None):
    """one matrix in the kernel's order -> f32 sums [M, n] (as float64).  h: the f32 rows after the prologue."""
    h = np.asarray(h, F32)
    K = h.shape[1]
    if fault == "x_bf16":
        h = G.bf16_rne(h)
    idx = lane_index(K, NIT)
    if fault == "drop_chunk":
        cpw = wave_chunks(K)[0]
        idx = np.where(idx == cpw + 1, K >> 3, idx)   # the second chunk of wave 1
    xc = _lanes(h, idx)[:, None]                       # [M, 1, 4, NIT, 64, 8]
    val = np.zeros((h.shape[0], W.shape[0], 4, 64))
    if form is None:
        wc = _lanes(np.asarray(W, np.float64), idx)[None]
        for it in range(NIT):
            for j in range(8):
                val = _fma(wc[:, :, :, it, :, j], xc[:, :, :, it, :, j], val)
        return _tree(val)
    qf, s, m1 = form
    if fault == "scale_f16_twice":
        with np.errstate(over="ignore"):
            s = s.astype(np.float16).astype(np.float64)
    if fault == "drop_last_min" and m1 is not None:
        m1 = m1.copy()
        m1[:, -1] = 0.0
    wc = _lanes(qf, idx)[None]
    pick = lambda a: np.concatenate([a, np.zeros((a.shape[0], 1))], axis=1)[:, idx][None]   # noqa: E731  [1, n, 4, NIT, 64]
    sc, mc = pick(s), (pick(m1) if m1 is not None else None)
    for it in range(NIT):
        p = np.zeros(val.shape)
        for j in range(8):
            p = _fma(wc[:, :, :, it, :, j], xc[:, :, :, it, :, j], p)
        val = _fma(sc[:, :, :, it], p, val)
        if mc is not None:
            sx = np.zeros(xc.shape[:3] + (64,))
            for j in range(8):
                sx = _r(sx + xc[:, :, :, it, :, j])
            val = _fma(-mc[:, :, :, it], sx, val)
    return _tree(val)


def epilogue_f32(kind, y, nh, nkv, pos, inv_freq, fault=None):
    """the epilogues operation by operation in f32 (no contraction): -> the stage's f32 outputs, K / V rows before their fp16 rounding"""
    if kind in (1, 3, 4):
        return dict(y=y)
    M = y.shape[0]
    if kind == 2:
        F = y.shape[1] // 2
        g, up = y[:, :F], y[:, F:]
        with np.errstate(over="ignore"):
            e = _r(np.exp(-g))
        return dict(y=_r(_r(g / _r(1.0 + e)) * up))
    pos = np.asarray(pos) + (np.arange(M) == 0) * (1 if fault == "rope_neighbour" else 0)
    cs, sn = (_r(t)[:, None, :] for t in G.rope_tables(inv_freq, pos))
    out, lo = {}, 0
    for name, heads in (("y", nh), ("k", nkv), ("v", nkv)):
        yy = y[:, lo:lo + heads * 64]
        lo += heads * 64
        if name != "v":
            yy = yy.reshape(M, heads, 2, 32)
            x1, x2 = yy[:, :, 0], yy[:, :, 1]
            yy = np.stack([_r(_r(x1 * cs) + _r(-x2 * sn)), _r(_r(x2 * cs) + _r(x1 * sn))], axis=2).reshape(M, heads * 64)
        out[name] = yy
    return out


def stage_f32(model, fmt, kind, L, x, pos0=POS0, fault=None, rows=64):
    """the whole stage in the kernel's order on the first `rows` rows of every matrix of the stage (kind 0: the first head of q, k and v) ->
    (restated outputs, the reference cut to the same rows)"""
    cfg = L["config"]
    K = kind_k(model, kind)
    pro = kind in NORMS
    h = prologue_f32(x, L["norms"][kind], cfg.rms_eps, fault) if pro else np.asarray(x, F32)
    ref_h = rms_norm64(x, L["norms"][kind], cfg.rms_eps) if pro else x.astype(np.float64)
    ys, ry, rb = [], [], []
    for p in PROJ_OF_KIND[kind]:
        t = L["types"][p]
        n = 64 if kind == 0 else min(rows, L["values"][p].shape[0])
        NIT = gemv_instance(kind, t, L["values"][p].shape[0], K, 1)[0]
        form = chunk_form(t, L["params"][p])
        form = None if form is None else tuple(None if a is None else a[:n] for a in form)
        W = L["values"][p][:n]
        ys.append(gemv_f32(W, t, form, h, NIT, fault))
        y, b = gemv(W, t, form, ref_h, NIT, pro)
        ry.append(y)
        rb.append(b)
    nh, nkv = (1, 1) if kind == 0 else (0, 0)
    pos = pos0 + np.arange(x.shape[0])
    return (epilogue_f32(kind, np.concatenate(ys, axis=1), nh, nkv, pos, L["inv_freq"], fault),
            epilogue(kind, np.concatenate(ry, axis=1), np.concatenate(rb, axis=1), nh, nkv, pos, L["inv_freq"]))


def worst_ratio(got, ref):
    """over y and, for kind 0, the K / V values before their fp16 rounding"""
    r = ratio(np.abs(got["y"] - ref["y"]), ref["bound"])
    for nm in ("k", "v"):
        if nm in got:
            r = max(r, ratio(np.abs(got[nm] - ref[nm]), ref[nm + "_bound"]))
    return r


# ------------------------------------------------------------------------------------------------ geometry invariance (parent and children)
GEOMETRIES = {"4,1": (4, 1), "8,4": (8, 4)}
GEOMETRY_ENV = [a + b for a in ("RCA_GEMV_", "RCA_GEMVQ_") for b in ("QKV", "O", "GU", "DOWN", "HEAD")]
GEOMETRY_STAGES = [("P", "bf16", k) for k in ALL5] + [("S", f, k) for f in ("f16", "q8_0", "q4_k", "q6_k", "iq4") for k in ALL5] + \
                  [("D6", f, 3) for f in ("bf16", "q8_0", "q5_k", "q4_0")] + [("D8", f, k) for f in ("bf16", "q8_0", "q4_k") for k in (2, 3, 4)] + \
                  [("D8", "q6_k", 4)]


def make_handle(model, fmt, wclass, n_ctx=N_CTX):
    from realtime_codec_agent_amd.llm import LlamaForAlternatingCodeChannels
    L = layer(model, fmt, wclass)
    return LlamaForAlternatingCodeChannels(config=L["config"], weights=L["weights"], n_ctx=n_ctx, device=0), L


def geometry_outputs():
    """{name: bits} of GEOMETRY_STAGES on class c rows, M = 2, in whatever geometry this process's library read from its environment"""
    out, forms = {}, {}
    llm, key = None, None
    for model, fmt, kind in GEOMETRY_STAGES:
        if key != (model, fmt):
            if llm is not None:
                llm.close()
            llm, _ = make_handle(model, fmt, "rand")
            key = (model, fmt)
        llm.n_tokens = POS0
        got = llm.gemv_tap(0, kind, act_normal(kind_k(model, kind), kind, 400 + kind), want_kv=(kind == 0))
        name = f"{model}.{fmt}.{kind}"
        forms[name] = llm.gemv_tap_form()
        for i, a in enumerate(got if isinstance(got, tuple) else (got,)):
            out[f"{name}.{i}"] = np.ascontiguousarray(a).view(np.uint16 if a.dtype == np.float16 else np.uint32)
    if llm is not None:
        llm.close()
    return out, forms


if __name__ == "__main__":      # the child of test_gemv_gpu.py's geometry test: python gemv_ref.py <out.npz>; the RCA_GEMV* variables are set
    import json
    import sys
    outs, forms = geometry_outputs()
    np.savez(sys.argv[1], forms=np.array(json.dumps(forms)), **outs)
