"""Float64 reference, input builders and the error bound of the LM attention kernels run alone (rca_lm_attn_tap), shared by
tests/test_attn_cpu.py (is the reference the oracle's attention, do the inputs meet their conditions, does the bound have teeth?)
and tests/test_attn_gpu.py (do lm_attn_mfma_kernel + its two merges and lm_attn_flash_kernel compute it?); the batch pass's table
instances (rca_lm_batch_attn_tap) are route 3 of the bound, with their ragged batch cases at the end of this file
(tests/test_attn_batch_gpu.py).

Conventions (rca_lm.hip): q [M][n_heads][64] f32 after RoPE, K / V [T][n_kv_heads][64] fp16 cache rows; the token at index t sits at
position pos0 + t and sees keys 0 .. pos0 + t; q head h reads kv head h // G; score = q . k / 8; out [M][n_heads * 64].

THE BOUND.  With w_j = p_j / L the normalised weights of a row, a kernel that uses weights p_j (1 + e_j) in numerator and denominator
alike computes out + sum_j w_j e_j (v_j - out) / (1 + sum_j w_j e_j); an error f_j that only the numerator sees adds sum_j w_j f_j v_j,
a relative error g of the denominator adds g * out.  So per output element d

    bound_d = sqrt(S_a * sum_j a_j (v_jd - out_d)^2) / (1 - S_a)        a_j = w_j Ec_j, S_a = sum_j a_j  (Cauchy-Schwarz over
                                                                        sum_j a_j |v_jd - out_d|: everything stays a matrix product)
            + sum_j w_j En |v_jd| + sum_j min(w_j, FLOOR / L) |v_jd| + ACC sum_j w_j |v_jd|
            + DEN |out_d| + FIN |out_d|

with u = 2^-24 (an IEEE fp32 operation, round to nearest), U = 2^-23 (one addition inside an MFMA accumulation: the hardware does
not promise round-to-nearest there, a whole ulp covers truncation), X = 2^-22 (v_exp_f32, within two ulp), and the terms

  Ec_j, what the weight of key j is off by, relatively, before the split into fp16:
    * the score.  q is used as fp16 hi + lo: what is left of q_d is at most 2^-22 |q_d| + 2^-25 (lo may be a denormal, spacing
      2^-24).  The flash kernel first multiplies q by fl(scale * log2 e): two more roundings, 2 u |q_d|.  The 64 x 2 products are
      exact in fp32 and summed by 8 MFMAs: 128 U sum_d |q_d k_jd|.  scale = 1/8 is a power of two.  In nats:
          A_j = scale (2^-22 + 128 U [+ 2 u]) sum_d |q_d k_jd|  +  FLOOR_Q sum_d |k_jd|,
      FLOOR_Q = scale 2^-25 (decode) or ln 2 * 2^-25 (flash: the floor applies to q * scale * log2 e, in log2 units).
    * the exp argument.  Every subtraction s - m rounds, u |s - m|; __expf multiplies by fl(log2 e), two more.  The maxima a key
      is referred to -- its wave's, its split's, the row's; in the flash kernel the running maximum of its wave block after
      block, then the row's -- only grow, so the arguments telescope: CARG u (m - s_j), CARG = 3 (decode) or 1 (flash).
    * the exponentials: one for the key, one per merge level (decode: the 8 waves, then the splits; flash: the three waves), and in
      the flash kernel one alpha (plus the rounding of the product with it) per later key block of the same wave: NEXP_j X + NRESC_j u.
  En, FLOOR: p enters the P V product as fp16 hi + lo.  Decode rounds both to nearest: the rest is at most 2^-22 p, and never more
    than 2^-25 absolutely nor than p itself (a p below half the smallest denormal is lost outright).  The flash kernel truncates both
    (v_cvt_pkrtz): 2^-20 p, floor 2^-24.  p is relative to a maximum that is at most the row's, and L >= 1 relative to the row's, so
    the floor costs at most min(w_j, FLOOR / L) |v_jd| per key.  The denominator sums the unsplit fp32 p: numerator only.
  ACC: the products p v are exact in fp32; a key block is 64 of them added by MFMAs (64 U), then decode merges 8 waves and NSPLIT
    splits with one fma each ((8 + NSPLIT) u); the flash kernel keeps adding into the same accumulators over the NBW key blocks its
    wave owns (64 NBW U) and merges three waves with a product and a sum each (6 u).
  DEN: L is 16 in-lane additions and one across the half-waves per block, then the same merges: decode (17 + 8 + NSPLIT) u, flash
    (19 NBW + 6) u (l * alpha + block sum: two roundings).
  FIN: decode O / L, one division: u.  Flash 1 / L and a product: 3 u (a reciprocal within one ulp).  Route 2 stores bf16 hi + lo,
    each rounded to nearest (8-bit significands): 2^-16, and their f32 sum rounds once more: u.

ROUTE 3, "batch decode" (rca_lm_batch_attn_tap: lm_attn_mfma_kernel<G, TAB = true, KVQ> + lm_attn_mfma_batch_combine_kernel<G>).  The
table instance of the split kernel is the decode kernel with its pointers read from a table, and the batch merge is attn_merge_row,
the decode route's merge as a launch of its own: score, exp argument, En / FLOOR, ACC and DEN are the decode terms, unchanged, with
NSPLIT the number of splits the ROW's positions need (splits that are launched beyond them, for a bucket or for a companion with a
longer context, enter the merge with weight exactly 0).  What differs is the store: O / L (u), then bf16 hi + lo, each rounded to
nearest (2^-16, as on route 2), and the f32 sum of the two read back (u): FIN = u + 2^-16 + u.  Derived, like the rest.

Nothing here is fitted to a device's output: a correct kernel outside this bound means a missing term, which is to be found and named.
"""
import functools
from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np

SCALE = 0.125
ATT_KEYS = 256
u = 2.0 ** -24
U = 2.0 ** -23
X = 2.0 ** -22
ROUTES = {0: "decode", 1: "flash f32", 2: "flash bf16", 3: "batch decode"}
BATCH_ROUTE = 3


# ------------------------------------------------------------------ the reference
@dataclass(frozen=True)
class Wrong:
    """a deliberately wrong attention, for the teeth of the bound (test_attn_cpu.py) only"""
    swap_v: Optional[Tuple[int, int]] = None          # the V rows of these two keys exchanged
    drop_key: Optional[int] = None                    # this key masked out
    mask_shift: int = 0                               # token t sees keys 0 .. pos0 + t + mask_shift
    swap_kv_heads: Optional[Tuple[int, int]] = None   # q heads of kv head a read kv head b and the other way round
    drop_split: Optional[int] = None                  # the 256 keys of this split masked out
    no_max: bool = False                              # fp32 exp of the unshifted score


def attention(q, K, V, pos0, wrong: Optional[Wrong] = None, with_bound_for: Optional[int] = None):
    """q [M, nh, 64] f32, K / V [T >= pos0 + M, nkv, 64] fp16 -> out [M, nh * 64] float64; with_bound_for = route (a key of ROUTES) also
    returns the bound, same shape."""
    assert with_bound_for is None or with_bound_for in ROUTES
    q = np.asarray(q)
    M, nh, hd = q.shape
    nkv = K.shape[1]
    G = nh // nkv
    assert hd == 64 and nh == nkv * G and K.shape == V.shape and K.dtype == np.float16 and V.dtype == np.float16
    T = pos0 + M
    assert K.shape[0] >= T
    w = wrong or Wrong()
    K64, V64 = K[:T].astype(np.float64), V[:T].astype(np.float64)
    if w.swap_v:
        a, b = w.swap_v
        V64[[a, b]] = V64[[b, a]]
    q64 = q.astype(np.float64)
    keys = np.arange(T)
    qpos = np.repeat(pos0 + np.arange(M), G)                     # row = token * G + head of the group
    mask = keys[None, :] > (qpos + w.mask_shift)[:, None]
    if w.drop_key is not None:
        mask = mask | (keys == w.drop_key)[None, :]
    if w.drop_split is not None:
        mask = mask | (keys // ATT_KEYS == w.drop_split)[None, :]
    out = np.empty((M, nh, 64))
    bnd = np.empty((M, nh, 64)) if with_bound_for is not None else None
    for g in range(nkv):
        gk = g
        if w.swap_kv_heads and g in w.swap_kv_heads:
            gk = w.swap_kv_heads[1 - w.swap_kv_heads.index(g)]
        Qg = q64[:, g * G:(g + 1) * G].reshape(M * G, 64)
        Kg, Vg = K64[:, gk], V64[:, gk]
        S = (Qg @ Kg.T) * SCALE
        S[mask] = -np.inf
        if w.no_max:
            with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
                P = np.exp(S.astype(np.float32))
                o = (P @ Vg.astype(np.float32)) / P.sum(1, keepdims=True, dtype=np.float32)
            out[:, g * G:(g + 1) * G] = o.reshape(M, G, 64)
            continue
        m = S.max(1, keepdims=True)
        P = np.exp(S - m)
        L = P.sum(1, keepdims=True)
        W = P / L
        o = W @ Vg
        out[:, g * G:(g + 1) * G] = o.reshape(M, G, 64)
        if bnd is not None:
            bnd[:, g * G:(g + 1) * G] = _bound(with_bound_for, Qg, Kg, Vg, S, m, W, L, o, qpos, mask).reshape(M, G, 64)
    out = out.reshape(M, nh * 64)
    return (out, bnd.reshape(M, nh * 64)) if bnd is not None else out


def _bound(route, Qg, Kg, Vg, S, m, W, L, o, qpos, mask):
    """the module docstring, for the rows of one kv head"""
    flash = route in (1, 2)
    T = Kg.shape[0]
    absqk = np.abs(Qg) @ np.abs(Kg).T
    sumk = np.abs(Kg).sum(1)[None, :]
    A = SCALE * (2.0 ** -22 + 128 * U + (2 * u if flash else 0.0)) * absqk + (np.log(2.0) * 2.0 ** -25 if flash else SCALE * 2.0 ** -25) * sumk
    gap = np.where(mask, 0.0, m - np.where(mask, 0.0, S))
    if flash:
        nb_row = (qpos >> 5) + 1                                     # key blocks the row sees
        nbw = -(-nb_row // 3).astype(np.float64)[:, None]            # ... of which one wave owns at most this many
        later = np.maximum((nb_row[:, None] - 1 - (np.arange(T) >> 5)[None, :]) // 3, 0)
        Ec = A + u * gap + (2 + later) * X + later * u
        En, floor = 2.0 ** -20, 2.0 ** -24
        acc = 64 * nbw * U + 6 * u
        den = (19 * nbw + 6) * u
        fin = 3 * u + ((2.0 ** -16 + u) if route == 2 else 0.0)
    else:
        nsp = -(-(qpos + 1) // ATT_KEYS).astype(np.float64)[:, None]
        Ec = A + 3 * u * gap + 3 * X
        En, floor = 2.0 ** -22, 2.0 ** -25
        acc = 64 * U + (8 + nsp) * u
        den = (17 + 8 + nsp) * u
        fin = u + ((2.0 ** -16 + u) if route == BATCH_ROUTE else 0.0)
    a = W * Ec
    Sa = a.sum(1, keepdims=True)
    assert float(Sa.max()) < 0.5, "the weights' relative error bound is not small: the first-order form does not apply"
    var = np.maximum(a @ (Vg * Vg) - 2.0 * o * (a @ Vg) + o * o * Sa, 0.0)
    centred = np.sqrt(Sa * var) / (1.0 - Sa)
    absV = np.abs(Vg)
    WV = W @ absV
    numer = En * WV + np.minimum(W, floor / L) @ absV + acc * WV
    return centred + numer + (den + fin) * np.abs(o)


def splits_needed(pos0, M):
    return -(-(pos0 + M) // ATT_KEYS)


# ------------------------------------------------------------------ inputs
def f16(a):
    return np.asarray(a, dtype=np.float32).astype(np.float16)


def onehot_kv(seed, T, nkv):
    """keys: random +-1 vectors (exact in fp16); values: random fp16 up to 300 in magnitude.  Conditions (test_attn_cpu.py): no two
    keys of a head share a V row; for every target used, the lead of 16 * k_target over every other visible key is >= 40 nats."""
    rng = np.random.default_rng(seed)
    K = f16(rng.integers(0, 2, (T, nkv, 64)) * 2 - 1)
    V = f16(rng.uniform(-300.0, 300.0, (T, nkv, 64)))
    return K, V


def onehot_q(K, targets, n_heads):
    """targets [M, n_heads] key indices -> q [M, n_heads, 64] = 16 * K[target, kv head of the q head]"""
    nkv = K.shape[1]
    G = n_heads // nkv
    heads = np.arange(n_heads) // G
    return (16.0 * K[np.asarray(targets), heads[None, :]].astype(np.float32)).astype(np.float32)


def onehot_lead(K, targets, n_heads, pos0):
    """float64: the smallest lead (nats) of a row's target over its best other visible key"""
    q = onehot_q(K, targets, n_heads).astype(np.float64)
    M = q.shape[0]
    G = n_heads // K.shape[1]
    lead = np.inf
    for h in range(n_heads):
        s = (q[:, h] @ K[:pos0 + M, h // G].astype(np.float64).T) * SCALE
        s[np.arange(pos0 + M)[None, :] > (pos0 + np.arange(M))[:, None]] = -np.inf
        t = np.asarray(targets)[:, h]
        assert np.all(t <= pos0 + np.arange(M)), "a target must be visible to its row"
        top = s[np.arange(M), t].copy()
        s[np.arange(M), t] = -np.inf
        lead = min(lead, float((top - s.max(1)).min()))
    return lead


SCORE_CLASSES = {"flat": 0.1, "moderate": 3.0, "peaked": 15.0}
OFFSETS = (0.0, 80.0, -80.0)


def class_kv(seed, T, nkv, offset=0.0):
    """keys N(0, 1), the last component 16 for every key when a common score offset is wanted; values of mixed sign and magnitude
    (N(0, 1) * 10^U(-2, 2))"""
    rng = np.random.default_rng(seed)
    K = rng.standard_normal((T, nkv, 64))
    if offset:
        K[:, :, 63] = 16.0
    V = rng.standard_normal((T, nkv, 64)) * 10.0 ** rng.uniform(-2.0, 2.0, (T, nkv, 64))
    return f16(K), f16(V)


def class_q(seed, M, n_heads, sigma, offset=0.0):
    """q = sigma * N(0, 1): scores q . k / 8 over N(0, 1) keys have standard deviation sigma; the last component carries the offset:
    q_63 * 16 / 8 = offset nats on every key alike"""
    rng = np.random.default_rng(seed)
    q = sigma * rng.standard_normal((M, n_heads, 64))
    if offset:
        q[:, :, 63] = offset / 2.0
    return q.astype(np.float32)


def dominant_kv(seed, T, nkv, at):
    """class_kv with one planted key: component 63 is 16 at key `at` and 0 elsewhere; with dominant_q the planted key scores 96 nats
    plus its random part, every other key only its random part (sigma 3: +-12)"""
    K, V = class_kv(seed, T, nkv)
    K[:, :, 63] = 0
    K[at, :, 63] = 16
    return K, V


def dominant_q(seed, M, n_heads):
    q = class_q(seed, M, n_heads, 3.0)
    q[:, :, 63] = 48.0
    return q


def far(a, b, bound):
    """distance of two outputs in bounds; a non-finite value on either side is infinitely far"""
    if not (np.isfinite(a).all() and np.isfinite(b).all()):
        return np.inf
    return float((np.abs(a - b) / bound).max())


# ------------------------------------------------------------------ the cases both test files walk
GEOMS = {"g1": (2, 2), "g2": (4, 2), "g4": (4, 1), "kv3": (3, 3), "w32": (32, 32), "w16": (32, 16)}    # name -> (q heads, kv heads)
SMALL = ("g1", "g2", "g4", "kv3")
ONEHOT_T = 2200          # planted one-hot keys: the M = 1024 flash pass at pos0 = 1100 ends at key 2123
ONEHOT_SEED = 11
FLASH_POS0 = 1100


def decode_onehot_calls(n_heads):
    """(pos0, targets [M, n_heads]) of the decode one-hot calls: every key offset of split 1 (keys 256 .. 511: 8 waves x 32 register
    slots) once; the first and last key of splits 0, 1, 2 and keys 31 / 32; the newest key; and 2-token calls whose token 0 targets its own position
    (the key token 1's row sits one past).  The rows of a call target different keys."""
    calls = []
    pos0 = 699
    for base in range(0, 256, n_heads):
        calls.append((pos0, np.array([[256 + (base + h) % 256 for h in range(n_heads)]])))
    edge = [0, 31, 32, 255, 256, 511, 512, 767]
    for i in range(0, len(edge), n_heads):
        row = [edge[(i + h) % len(edge)] for h in range(n_heads)]
        if len(set(row)) == n_heads:
            calls.append((800, np.array([row])))
    for p in (699, 767, 768):
        for own in range(n_heads):                                  # the newest key, on each head in turn
            calls.append((p, np.array([[p if h == own else 300 + h for h in range(n_heads)]])))
            calls.append((p, np.array([[p if h == own else 300 + h for h in range(n_heads)],
                                       [p + 1 if h == (own + 1) % n_heads else 400 + h for h in range(n_heads)]])))
    return calls


def flash_onehot_targets(M, n_heads, pos0):
    """row r = token * n_heads + head.  One row per token (head token % n_heads) targets one of the token's newest keys, token - k with
    k = (token // 32) % 33, its own position included (the masked blocks); the others walk the keys 0 .. pos0 - 1 with a stride coprime
    to pos0, so that any pos0 consecutive ones differ and every slot of a 32-key block on each of the three waves is a target"""
    stride = 389
    assert np.gcd(stride, pos0) == 1
    r = np.arange(M * n_heads).reshape(M, n_heads)
    t = np.arange(M)[:, None]
    recent = pos0 + t - (t // 32) % 33
    return np.where(r % n_heads == t % n_heads, recent, (r * stride) % pos0)


FLASH_ONEHOT_M = (1024, 33, 7)

CLASS_T = 700            # class-b / seam inputs: 700 planted keys (n_ctx = 700 on the small handles)
CLASS_POS0 = 640


def class_case(geom, cls, offset, route):
    """(K, V, q, pos0) of one accuracy case; M = 2 on the decode route, 40 (two G = 1 tiles, one short) on the flash routes"""
    nh, nkv = GEOMS[geom]
    seed = 1000 + 97 * list(GEOMS).index(geom) + 7 * list(SCORE_CLASSES).index(cls) + OFFSETS.index(offset)
    K, V = class_kv(seed, CLASS_T, nkv, offset)
    M = 2 if route == 0 else 40
    return K, V, class_q(seed + 1, M, nh, SCORE_CLASSES[cls], offset), CLASS_POS0


LONG_CTX = 32768
LONG_SPLITS = (32, 33, 64, 65, 128)
LONG_PATTERNS = ("moderate", "dominant first", "dominant last")


def long_case(geom, nsplits, pattern, M=2):
    """(K, V, q, pos0) with pos0 + M keys needing exactly `nsplits` splits (the last one holds 5 keys)"""
    nh, nkv = GEOMS[geom]
    T = (nsplits - 1) * ATT_KEYS + 5
    seed = 5000 + nsplits
    if pattern == "moderate":
        K, V = class_kv(seed, T, nkv)
        q = class_q(seed + 1, M, nh, SCORE_CLASSES["moderate"])
    else:
        at = 100 if pattern == "dominant first" else T - M - 2
        K, V = dominant_kv(seed, T, nkv, at)
        q = dominant_q(seed + 1, M, nh)
    assert splits_needed(T - M, M) == nsplits
    return K, V, q, T - M


# ------------------------------------------------------------------ the batch pass's attention (route 3; test_attn_batch_gpu.py)
BATCH_GEOMS = {"g1": (12, 12), "g2": (6, 3), "g4": (12, 3)}     # the k768 models of test_lm_batch_gpu.py: name -> (q heads, kv heads)
# the n_ctx of the 64 twins of a family, in slot order: the first six are all different, 1 / 3 / 33 / 65 / 4 / 3 splits
BATCH_FAMILY_CTX = (700, 256, 8448, 16640, 1024, 520) + tuple((256, 700, 1024)[i % 3] for i in range(57)) + (520,)
BATCH_ONEHOT_SHAPES = ((2, 1), (2, 2), (5, 1), (5, 2), (33, 1), (33, 2), (64, 1), (64, 2))      # (members, tokens per member)
BATCH_BUCKETS = 8                                                                # LM_GRAPH_BUCKETS


@dataclass(frozen=True)
class BatchMember:
    """one member of a ragged batch case: its own cache size, where its n tokens start, and what its cache and query rows hold --
    kind "onehot", a name of SCORE_CLASSES (with `offset`), "dominant first" or "dominant last" -- from `seed`"""
    n_ctx: int
    pos0: int
    kind: str
    seed: int
    offset: float = 0.0


@functools.lru_cache(maxsize=48)
def _batch_kv(nkv, T, n, kind, seed, offset):
    if kind == "onehot":
        return onehot_kv(seed, T, nkv)
    if kind in SCORE_CLASSES:
        return class_kv(seed, T, nkv, offset)
    assert kind in ("dominant first", "dominant last") and T >= 110
    return dominant_kv(seed, T, nkv, 100 if kind == "dominant first" else T - n - 2)


def batch_onehot_targets(seed, n, n_heads, pos0):
    """[n, n_heads] keys, all different: every token targets its own position on one head; the seams of the 32-key blocks and of the
    256-key splits, the first key of the token's last split and the key before its own where it sees them; random visible keys
    for the rest"""
    assert pos0 + 1 >= 2 * n_heads
    rng = np.random.default_rng(seed + 7)
    tg = np.empty((n, n_heads), np.int64)
    used = set()
    for j in range(n):
        last = pos0 + j
        must = list(dict.fromkeys(k for k in (0, 31, 32, 255, 256, 511, 512, (last // ATT_KEYS) * ATT_KEYS, last - 1) if 0 <= k < last and k not in used))
        rng.shuffle(must)
        row = [last] + must[:n_heads - 1]
        free = np.array([k for k in range(last) if k not in used and k not in row])
        row += rng.choice(free, n_heads - len(row), replace=False).tolist()
        tg[j] = rng.permutation(row)
        used |= set(row)
    return tg


def batch_member_inputs(geom, n, mb):
    """(K, V, q, targets): K / V [pos0 + n, nkv, 64] fp16, the rows the member's cache holds from position 0 on; q [n, nh, 64] f32;
    targets [n, nh] for a one-hot member, else None"""
    nh, nkv = BATCH_GEOMS[geom]
    assert 0 <= mb.pos0 and mb.pos0 + n <= mb.n_ctx
    K, V = _batch_kv(nkv, mb.pos0 + n, n, mb.kind, mb.seed, mb.offset)
    if mb.kind == "onehot":
        tg = batch_onehot_targets(mb.seed, n, nh, mb.pos0)
        return K, V, onehot_q(K, tg, nh), tg
    if mb.kind in SCORE_CLASSES:
        return K, V, class_q(mb.seed + 1, n, nh, SCORE_CLASSES[mb.kind], mb.offset), None
    return K, V, dominant_q(mb.seed + 1, n, nh), None


def batch_reference(geom, n, members, kv=None, wrong=None):
    """(want, bound) [len(members) * n, nh * 64] of a batch case on route 3, member k's token j in row k * n + j; kv: the rows the
    caches really hold, [(K, V)] per member (a q8_0 cache: the de-quantised rows), instead of the planted ones"""
    outs = []
    for k, mb in enumerate(members):
        K, V, q, _ = batch_member_inputs(geom, n, mb)
        if kv is not None:
            K, V = kv[k]
        outs.append(attention(q, K, V, mb.pos0, wrong, with_bound_for=BATCH_ROUTE))
    return np.concatenate([o for o, _ in outs]), np.concatenate([b for _, b in outs])


def batch_onehot_members(nm, n):
    """the first nm twins of a family, every one with a seed of its own, started at the seams of the blocks and splits or at its
    last slot"""
    out = []
    for s, c in enumerate(BATCH_FAMILY_CTX[:nm]):
        pool = (24, 25, 254, 255, 256, 257, 300, 511, 512, c - n)
        p = pool[s % len(pool)]
        out.append(BatchMember(c, p if p + n <= c else c - n, "onehot", 9000 + s))
    return out


def batch_class_members(cls, offset):
    """n = 2; five members with inputs of their own: 642 / 702 keys, the last slots of a 700 and a 1024 cache (the context limit inside
    / at the end of the last split), and the split seam of a long cache"""
    seed = 12000 + 97 * list(SCORE_CLASSES).index(cls) + 11 * OFFSETS.index(offset)
    return [BatchMember(c, p, cls, seed + 2 * k, offset) for k, (c, p) in enumerate(((700, 640), (1024, 700), (700, 698), (8448, 255), (1024, 1022)))]


def batch_seam_members(n):
    """every start of {0, 1, 254, 255, 256, 257, 511, 512, n_ctx - n}: n = 2 straddles a split at 255 (token 0 in one split, token 1
    in two) and at 511, and ends on the context limit of every cache size"""
    spec = ((256, 0), (700, 1), (700, 254), (700, 255), (1024, 256), (520, 257), (700, 511), (1024, 512),
            (700, 700 - n), (256, 256 - n), (1024, 1024 - n), (520, 520 - n))
    return [BatchMember(c, p, "moderate", 13000 + 2 * k) for k, (c, p) in enumerate(spec)]


BATCH_RAGGED = ("last", "short", "mixed")


def batch_ragged_members(n, variant):
    """caches of 1, 3, 33 and 65 splits in one batch.  last: every member at its last slot.  short: the long caches at short contexts
    (launched splits beyond their context: the empty-split path).  mixed: the 65-split cache at exactly 32 splits of context next to
    the 33-split cache at its end."""
    spec = {"last": ((256, 256 - n, "moderate"), (700, 700 - n, "moderate"), (8448, 8448 - n, "dominant first"), (16640, 16640 - n, "dominant last")),
            "short": ((256, 256 - n, "moderate"), (700, 511, "moderate"), (8448, 300, "dominant last"), (16640, 255, "dominant first")),
            "mixed": ((256, 100, "moderate"), (700, 256, "moderate"), (8448, 8448 - n, "dominant last"), (16640, 8192 - n, "dominant first"))}[variant]
    return [BatchMember(c, p, kind, 14000 + 10 * BATCH_RAGGED.index(variant) + 2 * k) for k, (c, p, kind) in enumerate(spec)]


def batch_launches(members, n):
    """the split counts a batch pass over these members can be launched with: what they need now (0) and every graph bucket's
    min(all members' splits, 4 << bucket) from there up; the last bucket launches all"""
    need = max(splits_needed(mb.pos0, n) for mb in members)
    nsp_all = max(-(-mb.n_ctx // ATT_KEYS) for mb in members)
    buckets = {nsp_all if b + 1 == BATCH_BUCKETS else min(nsp_all, 4 << b) for b in range(BATCH_BUCKETS)}
    return [0] + sorted(x for x in buckets if x >= need)
