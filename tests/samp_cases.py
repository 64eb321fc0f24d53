"""Hand-made logit rows for the sampler, and plain float64 references of what a draw may return.

Shared by tests/test_sampler_cpu.py (are the rows what they say they are, does the C restatement oracle/sampler_oracle.c respect the
plain references?) and tests/test_sampler_gpu.py (does the device draw, token for token, what the restatement draws from the same
row?).  numpy only; the restatement is loaded by chi_reference() alone.

The device's serial chain (top_k 1..256) first builds a candidate list: a 2048-bin histogram of the top 11 bits of the monotone
key (sign, exponent, two mantissa bits: a bin spans a quarter octave), the highest bin b with count(bins >= b) >= k, and every
token at or above that bin.  The size of that list selects one of three bodies of the last kernel -- `count` (<= 1024), `sort`
(<= 4096) or `scan` (the list overflowed: the whole vocabulary is scanned again) -- and a model's near-Gaussian logits only ever
reach the first.  candidates() restates that rule, so that every test can assert which body the row it uploads reaches.

No row here holds a NaN, and no row is entirely -inf: the restatement does not define a draw from either.
"""
import functools
from dataclasses import dataclass
from typing import Callable, Dict, Tuple

import numpy as np

SAMP_MAXK, SAMP_FAST_CAP, SAMP_CAND_CAP = 256, 1024, 4096      # rca_lm.hip
VOCABS = (8192, 4096)
ODD_SHAPE = "g1_tile32"      # lm_shape_cases.py: bf16, vocabulary 1001 (no multiple of 64: the 64 slices of the whole-vocabulary kernels are ragged)
# allowed_set()'s margin is relative to the candidates' total mass (top_p) or to min_p.  The device sums at most 256 float
# exponentials serially (each within 2^-22 of exp, each partial sum rounded once: < 256 * 2^-23 + 2^-22 ~ 3.1e-5 relative) or
# truncates at most 8192 masses to 2^-40 (< 1e-8): a cut further than MARGIN_MIN from every token's mass is the same cut in float64.
MARGIN_MIN = 1e-4


def sample_key32(logits: np.ndarray) -> np.ndarray:
    """upper half of the device's monotone key: larger float <=> larger unsigned; -0.0 and +0.0 are one value"""
    u = (np.asarray(logits, np.float32) + np.float32(0.0)).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def serial_k(top_k: int, temp: float, V: int) -> int:
    k = 1 if temp <= 0.0 else top_k
    if k <= 0 or k > SAMP_MAXK:
        k = SAMP_MAXK
    return min(k, V)


def candidates(logits: np.ndarray, k: int) -> Tuple[int, str]:
    """(size of the candidate list the device builds for the k best, body of the last kernel that list selects)"""
    hist = np.bincount(sample_key32(logits) >> np.uint32(21), minlength=2048)
    suffix = np.cumsum(hist[::-1])[::-1]
    reach = np.nonzero(suffix >= k)[0]
    n = int(suffix[reach.max() if reach.size else 0])
    return n, "count" if n <= SAMP_FAST_CAP else "sort" if n <= SAMP_CAND_CAP else "scan"


def path(top_k: int, top_p: float, temp: float, V: int) -> str:
    """which sampler a configuration runs (rca_lm_sampler_init)"""
    if temp <= 0.0 or 1 <= top_k <= SAMP_MAXK:
        return "serial"
    return "big" if top_p < 1.0 or SAMP_MAXK < top_k < V else "whole"


def allowed_set(logits: np.ndarray, top_k: int, top_p: float, min_p: float, greedy: bool = False) -> Tuple[np.ndarray, float]:
    """(tokens a draw may return, margin) in float64.  The chain is llama.cpp's: the top_k best (value descending, ties to the
    lowest index; <= 0 or beyond the vocabulary = all), of those the shortest prefix whose mass reaches top_p of their total, of
    those the tokens with p >= min_p * p_max.  margin: how far the nearest token's mass is from flipping a cut, relative to the total
    (top_p) or to min_p; inf when neither cut is active.  The rank cut needs no margin: float32 values compare exactly."""
    v = np.asarray(logits, np.float32).astype(np.float64)
    V = v.shape[0]
    order = np.lexsort((np.arange(V), -v))          # value descending, then index ascending
    if greedy:
        return order[:1], np.inf
    k = top_k if 1 <= top_k <= V else V
    order = order[:k]
    e = np.exp(v[order] - v[order[0]])
    margin = np.inf
    if top_p < 1.0 and len(order) > 1:
        cum = np.cumsum(e)
        need = top_p * cum[-1]
        keep = int(np.argmax(cum >= need)) + 1
        below = cum[keep - 2] if keep >= 2 else -np.inf
        margin = min(margin, (cum[keep - 1] - need) / cum[-1], (need - below) / cum[-1])
        order, e = order[:keep], e[:keep]
    if min_p > 0.0 and len(order) > 1:
        margin = min(margin, float(np.abs(e / min_p - 1.0).min()))
        keep = e >= min_p
        keep[0] = True
        order = order[keep]
    return order, float(margin)


def draw_probs(logits: np.ndarray, allowed: np.ndarray, temp: float) -> np.ndarray:
    """float64 softmax(logits / temp) over the allowed tokens, in their order"""
    v = np.asarray(logits, np.float32).astype(np.float64)[allowed] / temp
    e = np.exp(v - v.max())
    return e / e.sum()


def penalised(logits: np.ndarray, bias: Dict[int, float], prev, repeat: float, freq: float, present: float) -> np.ndarray:
    """the row the sampler sees: logit bias, then llama.cpp's penalties over the window of accepted tokens (float32, as both sides do)"""
    v = np.array(logits, np.float32)
    for t, b in bias.items():
        v[t] = v[t] + np.float32(b)
    prev = list(prev)[-64:]
    if repeat != 1.0 or freq != 0.0 or present != 0.0:
        for t in sorted(set(prev)):
            c = prev.count(t)
            x = v[t] * np.float32(repeat) if v[t] <= 0 else v[t] / np.float32(repeat)
            v[t] = x - (np.float32(c) * np.float32(freq) + np.float32(present))
    return v


# ------------------------------------------------------------------ row builders (seeded)
def gaussian(V, seed):
    return np.random.default_rng(seed).standard_normal(V).astype(np.float32)


def shifted_up(V, seed):
    return (100.0 + 2.0 * np.random.default_rng(seed).standard_normal(V)).astype(np.float32)


def shifted_down(V, seed):       # every key on the negative, bit-inverted side
    return (-100.0 + np.random.default_rng(seed).standard_normal(V)).astype(np.float32)


def _floor(rng, V, at=-50.0):
    return (at - rng.random(V)).astype(np.float32)


def cap_row(n):
    """exactly n candidates for any top_k in 6..256: five distinct large values, n - 5 distinct values inside the bin [1.0, 1.25),
    everything else far below"""
    def build(V, seed):
        rng = np.random.default_rng(seed)
        row = _floor(rng, V)
        pos = rng.permutation(V)[:n]
        row[pos[:5]] = np.array([3.0, 2.75, 2.5, 2.25, 2.0], np.float32)
        m = n - 5
        row[pos[5:]] = rng.permutation((1.0 + 0.25 * (np.arange(m) + 0.5) / m).astype(np.float32))
        return row
    return build


def all_equal(V, seed):
    return np.full(V, 0.5, np.float32)


def tie_at_cut(k, low):
    """the k-th and (k + 1)-th largest values are equal: k - 3 distinct values on top, then SIX tokens at 4.0 (three inside the
    rank cut, three outside), at the lowest or at the highest indices"""
    def build(V, seed):
        rng = np.random.default_rng(seed)
        row = (0.5 * rng.standard_normal(V) - 10.0).astype(np.float32)
        ties = np.arange(1, 7) if low else np.arange(V - 7, V - 1)
        rest = np.setdiff1d(rng.permutation(V)[:k + 8], ties)[:k - 3]
        row[rest] = (4.5 + 0.01 * np.arange(k - 3)).astype(np.float32)
        row[ties] = 4.0
        return row
    return build


def neg_inf_but_3(V, seed):
    rng = np.random.default_rng(seed)
    row = np.full(V, -np.inf, np.float32)
    row[rng.permutation(V)[:3]] = np.array([1.0, 0.5, -0.25], np.float32)
    return row


def peaked(V, seed):             # every other mass is 0 in 2^-40 fixed point (and in the float chain: exp(x < -87) = 0)
    rng = np.random.default_rng(seed)
    row = rng.standard_normal(V).astype(np.float32)
    row[int(rng.integers(0, V))] = row.max() + np.float32(100.0)
    return row


def eight_equal(V, seed):        # with top_k = 0, top_p = 0.5: every mass is exactly 2^40 and the mass cut lands on cum == need
    rng = np.random.default_rng(seed)
    row = np.full(V, -200.0, np.float32)
    row[rng.permutation(V)[:8]] = 3.0
    return row


def huge(V, seed):
    rng = np.random.default_rng(seed)
    row = rng.standard_normal(V).astype(np.float32)
    pos = rng.permutation(V)[:8]
    row[pos] = np.array([3e38, 3e38, 2.9e38, 1e38, -3e38, -3e38, -2.9e38, -1e38], np.float32)
    return row


def denormal(V, seed):           # every logit a float32 denormal (either sign) or zero
    rng = np.random.default_rng(seed)
    bits = rng.integers(1, 0x800000, V).astype(np.uint32) | (rng.integers(0, 2, V).astype(np.uint32) << np.uint32(31))
    row = bits.view(np.float32).copy()
    row[rng.permutation(V)[:4]] = np.array([0.0, -0.0, 0.0, -0.0], np.float32)
    return row


def signed_zero_top(V, seed):    # the maximum is a zero: -0.0 at a low index, +0.0 at a high one; equal values, the lowest index wins
    rng = np.random.default_rng(seed)
    row = (rng.standard_normal(V) - 5.0).astype(np.float32)
    row[row >= 0] = -1.0
    row[3] = -0.0
    row[V - 5] = 0.0
    return row


def signed_zero_cut(V, seed, n_top=16):
    """n_top values just above zero, then zeros across the rank cut of top_k = n_top + 4 (or + 3): -0.0 at indices 10..12, +0.0 at
    the three highest indices but one: the cut keeps 10, 11, 12, then V - 4 (lowest indices first, whatever the sign of the zero)"""
    rng = np.random.default_rng(seed)
    row = (rng.standard_normal(V) - 8.0).astype(np.float32)
    row[row >= 0] = -1.0
    top = np.setdiff1d(rng.permutation(V - 8)[:n_top + 24], np.arange(10, 13))[:n_top]
    row[top] = (0.1 + (0.01 if n_top == 16 else 0.0001) * np.arange(n_top)).astype(np.float32)
    row[10:13] = -0.0
    row[V - 4:V - 1] = 0.0
    return row


def chi_row(V, seed=0):
    """the chi-square support: eight tokens spread over the vocabulary, logits 2.0 ... -1.5 in steps of 0.5, the rest at -60"""
    row = np.full(V, -60.0, np.float32)
    row[chi_support(V)] = (2.0 - 0.5 * np.arange(8)).astype(np.float32)
    return row


def chi_support(V):
    return np.linspace(5, V - 7, 8).astype(np.int64)


CHI_TEMP, CHI_SEED, CHI_DRAWS, CHI_BOUND = 0.8, 1234, 4096, 29.88   # 29.88: the 1 - 1e-4 quantile of chi-square, 7 degrees of freedom
CHI_CONFIGS = {"serial": (20, 1.0), "whole": (0, 1.0), "big": (300, 0.999)}     # path -> (top_k, top_p); min_p 0


CHI_V = 4096


@functools.lru_cache(maxsize=None)
def chi_reference(path: str) -> tuple:
    """the restatement's CHI_DRAWS draws from chi_row(CHI_V) on one path, computed once per process (the only function here that
    loads the restatement)"""
    from oracle import lm_ref
    top_k, top_p = CHI_CONFIGS[path]
    row = chi_row(CHI_V)
    return tuple(lm_ref.sample(row, top_k, top_p, 0.0, CHI_TEMP, CHI_SEED, c) for c in range(CHI_DRAWS))


def chi_square(tokens, V) -> float:
    sup = chi_support(V)
    toks = np.asarray(tokens)
    assert np.isin(toks, sup).all(), "a draw left the 8-token support"
    want = draw_probs(chi_row(V), sup, CHI_TEMP) * len(toks)
    got = np.array([(toks == t).sum() for t in sup], np.float64)
    return float(((got - want) ** 2 / want).sum())


@dataclass(frozen=True)
class Row:
    name: str
    build: Callable
    seed: int
    bodies: Dict[int, Tuple[str, str]]      # top_k -> (body at V = 8192, body at V = 4096); a vocabulary of <= 1024 is always `count`
    sizes: Tuple[int, int] = (0, 0)         # list size at top_k = 20 where the row promises one (the cap rows), per vocabulary; 0 = none

    def make(self, V):
        return self.build(V, self.seed)

    def body(self, V, k):
        if V <= SAMP_FAST_CAP:
            return "count"
        return self.bodies[k][VOCABS.index(V)]


_C, _S, _X = "count", "sort", "scan"
_ALL = lambda a, b: {1: (a, b), 20: (a, b), 256: (a, b)}
ROWS = (
    Row("gaussian", gaussian, 11, _ALL(_C, _C)),
    Row("shifted_up", shifted_up, 12, _ALL(_X, _S)),
    Row("shifted_down", shifted_down, 13, {1: (_C, _C), 20: (_X, _S), 256: (_X, _S)}),
    Row("cap_1024", cap_row(1024), 14, _ALL(_C, _C), (1024, 1024)),
    Row("cap_1025", cap_row(1025), 15, {1: (_C, _C), 20: (_S, _S), 256: (_S, _S)}, (1025, 1025)),
    Row("cap_4096", cap_row(4096), 16, {1: (_C, _C), 20: (_S, _S), 256: (_S, _S)}, (4096, 4096)),
    Row("cap_4097", cap_row(4097), 17, {1: (_C, _C), 20: (_X, _S), 256: (_X, _S)}, (4097, 0)),
    Row("all_equal", all_equal, 0, _ALL(_X, _S)),
    Row("tie_cut20_low", tie_at_cut(20, True), 18, {1: (_C, _C), 20: (_C, _C), 256: (_S, _S)}),
    Row("tie_cut20_high", tie_at_cut(20, False), 19, {1: (_C, _C), 20: (_C, _C), 256: (_S, _S)}),
    Row("tie_cut256_high", tie_at_cut(256, False), 20, _ALL(_C, _C)),
    Row("neg_inf_but_3", neg_inf_but_3, 21, {1: (_C, _C), 20: (_X, _S), 256: (_X, _S)}),
    Row("peaked", peaked, 22, _ALL(_C, _C)),
    Row("eight_equal", eight_equal, 23, {1: (_C, _C), 20: (_X, _S), 256: (_X, _S)}),
    Row("huge", huge, 24, _ALL(_C, _C)),
    Row("denormal", denormal, 25, _ALL(_C, _C)),
    Row("signed_zero_top", signed_zero_top, 26, _ALL(_C, _C)),
    Row("signed_zero_cut", signed_zero_cut, 27, {1: (_C, _C), 20: (_C, _C), 256: (_S, _C)}),
)
BY_NAME = {r.name: r for r in ROWS}
# cap_4097 cannot exist in a vocabulary of 4096: there the builder is not used
ROW_VOCABS = tuple((r.name, V) for r in ROWS for V in VOCABS if not (r.name == "cap_4097" and V == 4096))

# (top_k, top_p, min_p, temp): the fixed list every row is crossed with.  top_k -1 stands for V - 1.
SERIAL_CONFIGS = ((1, 1.0, 0.0, 0.7), (20, 1.0, 0.0, 0.7), (256, 1.0, 0.0, 1.5), (20, 0.9, 0.0, 0.7), (256, 0.9, 0.05, 1.5),
                  (20, 1.0, 0.05, 1.5), (256, 1.0, 0.0, 0.0), (20, 0.9, 0.05, 0.0), (1, 0.9, 0.05, 1.5), (256, 0.9, 0.0, 0.7))
WHOLE_CONFIGS = ((0, 1.0, 0.0, 0.7), (0, 1.0, 0.05, 1.5))
BIG_CONFIGS = ((257, 0.9, 0.0, 0.7), (257, 0.02, 0.0, 1.5), (5000, 0.9, 0.05, 1.5), (5000, 0.02, 0.0, 0.7), (-1, 0.9, 0.0, 1.5),
               (-1, 0.02, 0.05, 0.7), (0, 0.9, 0.0, 0.7), (0, 0.5, 0.0, 1.5), (257, 1.0, 0.0, 0.7))
DRAWS = 8


def configs(V):
    return tuple((V - 1 if k == -1 else k, p, m, t) for k, p, m, t in SERIAL_CONFIGS + WHOLE_CONFIGS + BIG_CONFIGS)
