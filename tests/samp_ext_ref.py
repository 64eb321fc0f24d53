"""typical_p and mirostat v2: THE DEFINITION of what the device draws (a float32 restatement, operation for operation), plain float64
references of what a draw may return, and the hand-made rows both are tested on.

ggml and llama-cpp-python are absent offline, so both samplers are restated from their published definitions
(llama_sampler_typical_apply, llama_sampler_mirostat_v2_apply, llama-cpp-python's _init_sampler ordering); bit parity with llama.cpp
is not pinned.  The restatement below is the definition: tests/test_sampler_ext_cpu.py holds it to the float64 references,
tests/test_sampler_ext_gpu.py holds the device to it token for token (and mu bit for bit).

numpy, plus ctypes on the oracle library for the three primitives the device shares with it bit for bit: oracle_expf, oracle_logf,
oracle_splitmix.  splitmix over a whole vocabulary is integer arithmetic and is done in numpy uint64 (the CPU test compares it with
oracle_splitmix); the one fused multiply-add of the Gumbel key is made exact by rounding the float64 sum to odd first (the CPU test
compares it with libm's fmaf).
"""
import ctypes as C
import functools

import numpy as np

import oracle
import samp_cases as S

f32, f64 = np.float32, np.float64
LOG2E = f32(1.44269504)
FX, FX_INV = f32(2.0 ** 40), f32(2.0 ** -40)
SAMP_RING = 128

# ------------------------------------------------------------------ margins (derived, never measured)
# Typical.  The float32 chain sums at most 256 terms serially; an exponential is within 2^-22 of exp and a logarithm within 2^-22
# (absolute, for arguments in [1, 256]).  s_i = |(L - d_i) - H| with |d_i| <= 87 (beyond that e_i is 0 and s_i is +inf on both
# sides): L - d_i carries 2^-22 from L and half an ulp of a value below 128 (2^-18 ... at most 3.8e-6 absolute); H <= ln 256 < 5.6 is a
# sum of 256 terms, each within 3 * 2^-23 relative, each partial sum rounded once: < 5.6 * (256 * 2^-24 + 3 * 2^-23) < 9e-5.  Two s
# values further apart than TYP_S_MARGIN order the same way in float64; identical logits tie identically on both sides.
TYP_S_MARGIN = 2e-4          # nats
# the cumulative mass against typical_p * total: the serial sum of <= 256 exponentials, as samp_cases.MARGIN_MIN derives it
TYP_MASS_MARGIN = S.MARGIN_MIN
# Mirostat.  The fixed-point sums: each of V <= 8192 masses is truncated by less than 2^-40, S >= 1 (the top token's mass is exactly
# 1): relative error below 8192 * 2^-40 < 7.5e-9; (float)S rounds once more (2^-24), the logarithm adds 2^-22 absolute.
# surprise_i = (lnS - x_i) * log2(e), x_i = (v_i - max) * (1 / temp): for |x_i| <= 64 three roundings of a value below 128 are within
# 3 * 2^-18 * ... = 3 half-ulps of 2^-17 = 1.1e-5; times 1.4427, plus the logarithm: < 2.5e-5 bits per surprise, the observed one
# included.  mu moves by eta * (observed - tau) per draw, eta <= 1: after n draws the float32 mu is within n * MIRO_DRAW_ERR of the
# float64 trajectory along the same tokens, as long as both keep the same set at every draw (guaranteed where the margin is clear).
MIRO_DRAW_ERR = 5e-5         # bits per draw (twice the bound above)
MIRO_DRAWS = 32


def miro_mu_bound(n_draws, eta):
    return n_draws * max(eta, 1.0) * MIRO_DRAW_ERR


MIRO_MARGIN_MIN = miro_mu_bound(MIRO_DRAWS, 1.0) + MIRO_DRAW_ERR      # bits: a surprise further than this from mu is on the same side in float64

# ------------------------------------------------------------------ primitives
_lib = None


def _olib():
    global _lib
    if _lib is None:
        oracle.build()
        _lib = C.CDLL(oracle.LIB_PATH)
        _lib.oracle_expf.restype = C.c_float
        _lib.oracle_expf.argtypes = [C.c_float]
        _lib.oracle_logf.restype = C.c_float
        _lib.oracle_logf.argtypes = [C.c_float]
        _lib.oracle_splitmix.restype = C.c_uint64
        _lib.oracle_splitmix.argtypes = [C.c_uint64, C.c_uint64]
    return _lib


def _each(fn, x):
    x = np.asarray(x, f32)
    return np.fromiter((fn(float(v)) for v in x.ravel()), f32, x.size).reshape(x.shape)


def expf(x):
    return _each(_olib().oracle_expf, x)


def logf(x):
    return _each(_olib().oracle_logf, x)


def splitmix(seed, ctr):
    """oracle_splitmix over arrays: wrapping uint64 arithmetic"""
    seed, ctr = np.atleast_1d(np.asarray(seed, np.uint64)), np.atleast_1d(np.asarray(ctr, np.uint64))
    z = seed * np.uint64(0x9E3779B97F4A7C15) + ctr * np.uint64(0xBF58476D1CE4E5B9) + np.uint64(0x94D049BB133111EB)
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def fmaf(a, b, c):
    """float32 fma(a, b, c), correctly rounded: the product is exact in float64, the sum is rounded to odd (the sticky bit survives),
    and 53 bits leave more than the two guard bits the final rounding to 24 needs.  Finite arguments."""
    p = np.asarray(a, f32).astype(f64) * np.asarray(b, f32).astype(f64)
    c = np.asarray(c, f32).astype(f64)
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)                       # TwoSum: p + c = s + err exactly
    bits = np.atleast_1d(s).view(np.int64).copy()
    even = (np.atleast_1d(err) != 0) & ((bits & 1) == 0)
    away = (np.atleast_1d(err) > 0) == (np.atleast_1d(s) > 0)
    bits = np.where(even, np.where(away, bits + 1, bits - 1), bits)
    return bits.view(f64).astype(f32).reshape(np.shape(s))


def _serial_sum(x):
    """x[0] + x[1] + ... in float32, each partial sum rounded once (add.accumulate is strictly sequential)"""
    return np.add.accumulate(np.asarray(x, f32), dtype=f32)


def gumbel_keys(d, inv_t, seed, counter, idx):
    """(v_i - max) / temp + g_i of the whole-vocabulary sampler for the tokens idx"""
    z = splitmix(splitmix(np.uint64(seed & 0xFFFFFFFF), np.uint64(counter)), np.asarray(idx, np.uint64))
    u = (((z >> np.uint64(41)) << np.uint64(1)) | np.uint64(1)).astype(f32) * f32(2.0 ** -24)
    g = -logf(-logf(u))
    return fmaf(d, np.full(len(idx), inv_t, f32), g)


# ------------------------------------------------------------------ the serial chain with the typical cut (float32 restatement)
@functools.lru_cache(maxsize=256)
def _top(row_bytes, k):
    row = np.frombuffer(row_bytes, f32)
    order = np.lexsort((np.arange(row.shape[0]), -(row + f32(0.0))))[:k]      # value descending, then index ascending
    return order, (row[order] + f32(0.0)).astype(f32)


def typical_cut(cval, typical_p):
    """indices (into the k sorted candidates, ascending = logit order) that survive the typical cut"""
    cnt = len(cval)
    with np.errstate(invalid="ignore", over="ignore"):
        d = cval - cval[0]
        e = expf(d)
        tot = _serial_sum(e)[-1]
        L, inv = logf(tot), f32(1.0) / tot
        nl = L - d
        p = e * inv
        term = np.where(e > 0, p * nl, f32(0.0)).astype(f32)
        H = _serial_sum(term)[-1]
        s = np.where(e > 0, np.abs(nl - H), f32(np.inf)).astype(f32)
    order = np.lexsort((np.arange(cnt), s))             # s ascending, then rank ascending
    cum = _serial_sum(e[order])
    over = np.nonzero(cum > f32(typical_p) * tot)[0]
    keep = int(over[0]) + 1 if over.size else cnt
    return np.sort(order[:keep])


def serial_sample(row, top_k, top_p, min_p, temp, seed, counter, typical_p=1.0):
    """the serial chain (top_k 1..256 or temp <= 0) as samp_final_kernel / samp_final_typ_kernel run it; typical_p off (>= 1 or 0)
    is oracle/sampler_oracle.c's serial branch"""
    row = np.ascontiguousarray(row, f32)
    greedy = temp <= 0.0
    k = S.serial_k(top_k, temp, row.shape[0])
    order, cval = _top(row.tobytes(), k)
    if greedy or k <= 1:
        return int(order[0])
    if 0.0 < typical_p < 1.0:
        kept = typical_cut(cval, typical_p)
        order, cval = order[kept], cval[kept]
    cnt = len(cval)
    if cnt <= 1:
        return int(order[0])
    inv_t = f32(1.0) / f32(temp)
    with np.errstate(invalid="ignore", over="ignore"):
        d = cval - cval[0]
        e_plain, e_temp = expf(d), expf(d * inv_t)
    if top_p < 1.0:
        cum = _serial_sum(e_plain)
        hit = np.nonzero(cum >= f32(top_p) * cum[-1])[0]
        cnt = int(hit[0]) + 1 if hit.size else cnt
    if min_p > 0.0:
        keep = 1
        for i in range(1, cnt):
            if e_plain[i] >= f32(min_p):
                keep = i + 1
            else:
                break
        cnt = keep
    cum = _serial_sum(e_temp[:cnt])
    z = int(splitmix(np.uint64(seed & 0xFFFFFFFF), np.uint64(counter))[0])
    target = f32(z >> 40) * f32(2.0 ** -24) * cum[-1]
    hit = np.nonzero(cum > target)[0]
    return int(order[int(hit[0]) if hit.size else cnt - 1])


# ------------------------------------------------------------------ mirostat v2 (float32 restatement)
@functools.lru_cache(maxsize=64)
def _miro_row(row_bytes, temp):
    row = np.frombuffer(row_bytes, f32)
    mx = row.max()
    inv_t = f32(1.0) / f32(temp)
    with np.errstate(invalid="ignore", over="ignore"):
        d = row - mx
        x = (d * inv_t).astype(f32)
    e = expf(x)
    w = (e * FX).astype(np.uint64)                      # trunc(e * 2^40): exact scaling, then truncation
    return mx, inv_t, d, x, w


def _fx_ln(total):
    return logf(f32(int(total)) * FX_INV)[()]


def mirostat_draw(row, temp, seed, counter, mu, tau, eta):
    """one draw: (token, mu after it, kept tokens).  row: what the sampler sees (logit bias and penalties applied)"""
    row = np.ascontiguousarray(row, f32)
    mx, inv_t, d, x, w = _miro_row(row.tobytes(), float(temp))
    mu, tau, eta = f32(mu), f32(tau), f32(eta)
    lnS = _fx_ln(w.sum(dtype=np.uint64))
    if not (lnS * LOG2E <= mu):                         # not even the top token passes: the lowest index among the maxima, alone
        kept = np.nonzero(row == mx)[0][:1]
        tok, kept_mass = int(kept[0]), 1 << 40
    else:
        with np.errstate(invalid="ignore", over="ignore"):
            kept = np.nonzero(((lnS - x) * LOG2E).astype(f32) <= mu)[0]
        kept_mass = w[kept].sum(dtype=np.uint64)
        keys = gumbel_keys(d[kept], inv_t, seed, counter, kept) + f32(0.0)
        tok = int(kept[int(np.argmax(keys))])           # the first maximum: ties go to the lowest index
    observed = (_fx_ln(kept_mass) - x[tok]) * LOG2E
    err = f32(observed) - tau
    step = eta * err
    return tok, f32(mu - step), kept


def mirostat_run(rows_seen, temp, seed, tau, eta, n, first=0, mu=None):
    """n consecutive draws; rows_seen(c, tokens so far) -> the row draw c sees.  Returns (tokens, mu before each draw and after the last)"""
    mus = [f32(2.0) * f32(tau) if mu is None else f32(mu)]
    toks = []
    for c in range(first, first + n):
        t, m, _ = mirostat_draw(rows_seen(c, toks), temp, seed, c, mus[-1], tau, eta)
        toks.append(t)
        mus.append(m)
    return toks, mus


# ------------------------------------------------------------------ plain float64 references
def typical_allowed(row, top_k, typical_p, top_p, min_p):
    """(tokens a draw may return, margin > 0 when every cut is clear).  Margin: the smaller of (nearest gap between two s values up
    to the one behind the cut, tokens of identical logit excepted) / TYP_S_MARGIN and (distance of the cumulative mass from typical_p,
    relative to the total) / TYP_MASS_MARGIN, in units of the derived minimum -- clear means > 1 -- and samp_cases.allowed_set's margin
    of the top_p / min_p cuts behind it, likewise scaled by MARGIN_MIN."""
    v = np.asarray(row, f32).astype(f64)
    V = v.shape[0]
    order = np.lexsort((np.arange(V), -v))[:S.serial_k(top_k, 1.0, V)]
    margin = np.inf
    if 0.0 < typical_p < 1.0 and len(order) > 1:
        vv = v[order]
        with np.errstate(divide="ignore", invalid="ignore"):
            e = np.exp(vv - vv[0])
            p = e / e.sum()
            nl = -np.log(p)
            H = float(np.where(p > 0, p * nl, 0.0).sum())
            s = np.where(p > 0, np.abs(nl - H), np.inf)
        o2 = np.lexsort((np.arange(len(order)), s))
        cum = np.cumsum(p[o2])
        over = np.nonzero(cum > typical_p)[0]
        keep = int(over[0]) + 1 if over.size else len(order)
        for r in range(min(keep, len(order) - 1)):      # gaps between neighbours up to (last kept, first dropped)
            a, b = o2[r], o2[r + 1]
            if vv[a] != vv[b] and np.isfinite(s[b]):
                margin = min(margin, (s[b] - s[a]) / TYP_S_MARGIN)
        margin = min(margin, (cum[keep - 1] - typical_p) / TYP_MASS_MARGIN)
        if keep >= 2:
            margin = min(margin, (typical_p - cum[keep - 2]) / TYP_MASS_MARGIN)
        order = order[np.sort(o2[:keep])]
    masked = np.full(V, -np.inf, f32)
    masked[order] = np.asarray(row, f32)[order]
    allowed, m2 = S.allowed_set(masked, len(order), top_p, min_p)
    return allowed, float(min(margin, m2 / S.MARGIN_MIN))


def mirostat_reference(rows_seen, temp, tau, eta, tokens, first=0):
    """float64 along a GIVEN token sequence: per draw (mu before it, allowed set, margin = min |surprise_i - mu| in bits), and the mu
    after the last draw"""
    mu = 2.0 * tau
    out = []
    for j, tok in enumerate(tokens):
        v = np.asarray(rows_seen(first + j, list(tokens[:j])), f32).astype(f64) / temp
        with np.errstate(divide="ignore"):
            lp = (v - v.max()) - np.log(np.exp(v - v.max()).sum())
            sur = -lp / np.log(2.0)
        kept = sur <= mu
        top = int(np.lexsort((np.arange(len(v)), -v))[0])
        margin = float(np.abs(sur[np.isfinite(sur)] - mu).min())
        if not kept.any():
            kept[top] = True
        out.append((mu, np.nonzero(kept)[0], margin))
        observed = -(lp[tok] - np.log(np.exp(lp[kept]).sum())) / np.log(2.0)
        mu = mu - eta * (observed - tau)
    return out, mu


def draw_probs(row, allowed, temp):
    return S.draw_probs(row, allowed, temp)


# ------------------------------------------------------------------ rows
def flat(V, seed):                      # every s ties: the index order decides
    return S.all_equal(V, seed)


def two_level(V, seed):
    """one token at 2.0, thirty at 0.0, the rest far below: p_top = 0.198 with -ln p = 1.62, the crowd's 3.62 each, H = 3.22 -- the
    crowd is the typical set and at typical_p = 0.2 / 0.5 the argmax is cut, which top_p can never do"""
    rng = np.random.default_rng(seed)
    row = (-50.0 - rng.random(V)).astype(f32)
    pos = rng.permutation(V)[:31]
    row[pos[0]] = 2.0
    row[pos[1:]] = 0.0
    return row


def neg_inf_tail(V, seed):              # 100 finite values, everything else -inf: at top_k = 256 most candidates have p = 0
    rng = np.random.default_rng(seed)
    row = np.full(V, -np.inf, f32)
    row[rng.permutation(V)[:100]] = rng.standard_normal(100).astype(f32)
    return row


def zipf(a):
    def build(V, seed):
        rng = np.random.default_rng(seed)
        return (-a * np.log(np.arange(V) + 1.0)).astype(f32)[rng.permutation(V)]
    return build


def levels(V, seed):
    """2^j tokens at logit -1.5 j, j = 0 .. 9, the rest at -40: the surprises sit on ten levels 2.16 bits apart, so that mu lies
    clear of every token's surprise on almost every draw -- the row the float64 set and trajectory checks are meant for"""
    rng = np.random.default_rng(seed)
    row = np.full(V, -40.0, f32)
    pos = rng.permutation(V)
    at = 0
    for j in range(10):
        row[pos[at:at + (1 << j)]] = -1.5 * j
        at += 1 << j
    return row


def spike_over_noise(V, seed):
    """one token holds 0.9 of the mass at temp 1, the rest share 0.1 almost evenly (surprise ~ log2(10 (V - 1)) bits, 16.3 at 8192):
    nearly every draw returns the top token, the observed surprise stays below tau, and mu climbs until the kept set has crossed
    every slice seam and holds the whole vocabulary"""
    rng = np.random.default_rng(seed)
    row = (0.5 * rng.standard_normal(V)).astype(f32)
    row[int(rng.integers(0, V))] = f32(np.log(9.0 * (V - 1)) + 0.125)
    return row


TYP_ROWS = {            # name -> builder, seed
    "flat": (flat, 0), "two_level": (two_level, 31), "peaked": (S.peaked, 22), "neg_inf_but_3": (S.neg_inf_but_3, 21),
    "neg_inf_tail": (neg_inf_tail, 32), "gaussian": (S.gaussian, 11), "shifted_up": (S.shifted_up, 12), "cap_1025": (S.cap_row(1025), 15),
}
TYP_TOP_K, TYP_P = (2, 40, 256), (0.2, 0.5, 0.9)
TYP_BEHIND = ((1.0, 0.0), (0.9, 0.05))       # (top_p, min_p) behind the typical cut
TYP_TEMP = 0.8
# the body of the last kernel a row reaches (samp_cases.candidates) per top_k, at V = 8192 / 4096
_C, _SS, _XS = ("count", "count"), ("sort", "sort"), ("scan", "sort")
TYP_BODIES = {
    "flat": {2: _XS, 40: _XS, 256: _XS}, "shifted_up": {2: _XS, 40: _XS, 256: _XS}, "two_level": {2: _C, 40: _XS, 256: _XS},
    "neg_inf_but_3": {2: _C, 40: _XS, 256: _XS}, "neg_inf_tail": {2: _C, 40: _C, 256: _XS}, "cap_1025": {2: _C, 40: _SS, 256: _SS},
    "gaussian": {2: _C, 40: _C, 256: _C}, "peaked": {2: _C, 40: _C, 256: _C},
}
# rows the float64 allowed-set check is meant for: every configuration of theirs has a clear margin (asserted by the CPU test).
# (flat is not among them by construction: at typical_p = 0.5 its cumulative mass lands exactly on the cut.)
TYP_CLEAR_ROWS = ("two_level", "peaked", "neg_inf_but_3")


def typ_body(name, V, k):
    return "count" if V <= S.SAMP_FAST_CAP else TYP_BODIES[name][k][S.VOCABS.index(V)]


MIRO_ROWS = {
    "zipf": (zipf(1.0), 41),
    "climb": (spike_over_noise, 42),
    "fall": (zipf(0.05), 42),           # nearly flat: every draw surprises by ~ log2(V) bits, mu falls until only the top token is kept
    "spike": (S.peaked, 22),            # every other mass is 0: one token kept at any mu, the observed surprise is exactly 0
    "levels": (levels, 43),
    "neg_inf_tail": (neg_inf_tail, 32),
}
MIRO_CONFIGS = ((5.0, 0.1, 0.8), (5.0, 0.1, 1.0), (3.0, 1.0, 0.8), (3.0, 1.0, 1.0))      # (tau, eta, temp)
MIRO_VOCABS = S.VOCABS + (1001,)        # 1001: samp_cases.ODD_SHAPE's vocabulary, the 64 slices are ragged
MIRO_CLEAR_ROWS = ("levels", "spike")
MIRO_SEED = 7
MIRO_BIAS_PEN = dict(bias={3: 4.0, 17: -np.inf}, repeat_penalty=1.3, frequency_penalty=0.25, presence_penalty=0.15)


def make(table, name, V):
    build, seed = table[name]
    return build(V, seed)


def seen_fn(row, bias=None, repeat_penalty=1.0, frequency_penalty=0.0, presence_penalty=0.0):
    """rows_seen for a fixed uploaded row: logit bias and penalties over the tokens this sampler accepted"""
    if not bias and repeat_penalty == 1.0 and frequency_penalty == 0.0 and presence_penalty == 0.0:
        return lambda c, toks: row
    return lambda c, toks: S.penalised(row, bias or {}, toks, repeat_penalty, frequency_penalty, presence_penalty)


# chi-square: the form of samp_cases' test (its 8-token row at V = 4096, its temperature, seed and 4096 draws); the allowed set is
# what the float64 reference leaves of the 8 tokens, and the bound is the 1 - 1e-4 quantile of chi-square at (tokens left - 1)
# degrees of freedom (rounded up; 7 degrees give samp_cases.CHI_BOUND)
CHI_QUANTILE = {1: 15.14, 2: 18.43, 3: 21.11, 4: 23.52, 5: 25.75, 6: 27.86, 7: 29.88}
CHI_TYP = dict(top_k=40, typical_p=0.5, top_p=1.0, min_p=0.0)
CHI_MIRO = dict(tau=1.5, eta=0.0)        # eta = 0: mu stays 2 tau = 3 bits, the distribution is stationary


def chi_square(tokens, row, allowed, temp):
    toks = np.asarray(tokens)
    assert np.isin(toks, allowed).all(), "a draw left the allowed set"
    want = draw_probs(row, allowed, temp) * len(toks)
    got = np.array([(toks == t).sum() for t in allowed], f64)
    return float(((got - want) ** 2 / want).sum())
