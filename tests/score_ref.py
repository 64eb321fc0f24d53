"""Float64 reference of the rows rca_lm_score reduces logits to, input builders and the error bounds, shared by
tests/test_lm_score_cpu.py (is the reference right on closed forms, do the oracle rows leave the end-to-end checks something to check?)
and tests/test_lm_score_gpu.py (does lm_score_rows_kernel compute it, alone and behind the head on the 128-token tiles?).

Conventions (include/rca.h, rca_score_row_t): a [M][V] f32 logits of the scored handle, b the base's; P = softmax(a), P_base =
softmax(b); lse = log sum_j exp(a_j); argmax = lowest index of the maximum; logprob = a[target] - lse (NaN for target -1);
kl = KL(P_base || P) = sum_j p_base,j (b_j - a_j) - lse_b + lse_a.  A -inf logit has probability 0, a 0 * inf term of the KL sum
counts as 0, a -inf in P where the base has mass gives kl = +inf, a NaN in a row makes the row's floats NaN.

THE BOUND of the row kernel alone (the reduction's shape is restated from rca_lm.hip: SCORE_THREADS = 256 threads, 16-byte chunks
tid, tid + 256, ..., up to 3 ragged values in front / behind for thread 0 / 255, a 6-step butterfly per wave, 3 merges of waves).
With u = 2^-24 (one IEEE f32 operation, round to nearest) and X = 2^-22 (expf / logf: documented within 1 ulp, taken as 2):

  C     = ceil((V // 4) / 256)            chunks of the busiest thread
  NADD  = 4 C + 3 + 6 + 3                 f32 additions on the longest path into s = sum exp(a_j - m)
  NRESC = C + 6 + 3                       rescalings s * exp(m_old - m_new) on that path (at worst one per chunk, one per merge)

Every term of s is positive, so relative errors do not amplify:
  * a term exp(a_j - m') and each rescaling is one expf (X) and, for the rescaling, one product (u): (1 + NRESC) X + NRESC u;
  * the exp ARGUMENTS round (u |a_j - m'|, u |m_old - m_new|); the maxima only grow, so for term j they telescope to u (m - a_j),
    and weighted by the term's share that is ARG = u sum_j p_j (m - a_j), computed on the row;
  * the additions: NADD u.
  eps_s = (ARG + (1 + NRESC) X + NRESC u + NADD u) / (1 - the same)       (second order)
  lse = m + logf(s):      eps_s + X |log s| + u |lse|
  logprob = a_t - lse:    the above + u (|a_t| + |lse|)                      (one rounding of the difference)
  max_logit, argmax:      exact
  kl = (t / s_b - lse_b) + lse_a with t = sum_j exp(b_j - m_b) fl(b_j - a_j): the terms have signs, so the error is relative to
    TA = sum_j p_b,j |b_j - a_j|: per term the difference (u), the product (u), the term's exp and rescalings and additions as for
    s_b, the argument error weighted by |b_j - a_j| (ARGK = u sum_j p_b,j (m_b - b_j) |b_j - a_j|); the quotient takes s_b's relative
    error and one rounding; the two sums round once each; both lse errors add:
    TA ((1 + NRESC) X + (NRESC + NADD + 2) u) / (1 - ..) + ARGK + |q| (eps_sb + u) + u |q - lse_b| + u |kl| + err(lse_a) + err(lse_b)
Nothing here is fitted to a device's output.

THE END-TO-END BOUNDS.  A logit error of at most e per entry moves lse and max_logit by at most e and logit - lse by at most 2 e:
2 * lm_shape_cases.bound(want, tol) for all three.  For the KL of two models whose logits are off by at most e_a and e_b:
d kl = sum_j dp_b,j (log p_b,j - log p_a,j) + sum_j p_b,j (dlog p_b,j - dlog p_a,j) to first order, |dlog p| <= 2 e, |dp_b,j| <=
p_b,j 2 e_b: |d kl| <= 2 e_b (max_j |log p_b,j - log p_a,j| + KL) + 2 e_a (the sum of p_b,j dlog p_b,j vanishes to first order and
is covered by the KL term); doubled for the neglected second-order terms.
"""
import numpy as np

u = 2.0 ** -24
X = 2.0 ** -22
SCORE_THREADS = 256
FLOATS = ("logprob", "lse", "max_logit", "kl", "base_logprob")


def reduction_shape(V: int):
    """(C, NADD, NRESC) of lm_score_rows_kernel for rows of V logits"""
    C = max(1, -(-(V // 4) // SCORE_THREADS))
    return C, 4 * C + 3 + 6 + 3, C + 6 + 3


def owner(V: int, row: int, idx: int):
    """(thread, chunk or -1 for the ragged head / tail) that takes logit idx of row `row` of a dense [M][V] f32 array"""
    pre = min(V, (4 - (row * V) % 4) % 4)
    nb4 = (V - pre) // 4
    if idx < pre:
        return 0, -1
    c = (idx - pre) // 4
    if c >= nb4:
        return SCORE_THREADS - 1, -1
    return c % SCORE_THREADS, c


def seam_indices(V: int, row: int):
    """pairs / triples of indices on both sides of every seam of the reduction for that row: the ragged head and the first chunk,
    two lanes, two waves (threads 63 | 64, 127 | 128, 191 | 192), two iterations of a thread (chunks 255 | 256), last chunk and the
    ragged tail, and the row's two ends"""
    pre = min(V, (4 - (row * V) % 4) % 4)
    nb4 = (V - pre) // 4
    at = lambda c, e=0: pre + 4 * c + e
    groups = [(0, V - 1), (0, 1, V - 1)]
    if pre:
        groups.append((pre - 1, pre))                       # head | first chunk
    groups.append((at(0, 3), at(1, 0)))                     # lanes 0 | 1
    groups.append((at(0, 1), at(0, 2)))                     # inside one chunk
    for t in (63, 127, 191):
        if t + 1 < nb4:
            groups.append((at(t, 3), at(t + 1, 0)))         # waves
            groups.append((at(t + 1, 0), at(t, 3), at(min(t + 40, nb4 - 1), 2)))
    if nb4 > SCORE_THREADS:
        groups.append((at(SCORE_THREADS - 1, 3), at(SCORE_THREADS, 0)))     # thread 255's chunk | thread 0's second chunk
        groups.append((at(0, 0), at(SCORE_THREADS, 0), at(2 * SCORE_THREADS if nb4 > 2 * SCORE_THREADS else nb4 - 1, 0)))   # one thread, several iterations
    if pre + 4 * nb4 < V:
        groups.append((at(nb4 - 1, 3), at(nb4, 0)))         # last chunk | tail
        groups.append((at(0, 0), V - 1))
    return [tuple(sorted(set(g))) for g in groups if max(g) < V and len(set(g)) > 1]


def _lse(x):
    """float64 log-sum-exp over the last axis with -inf = probability 0; an all -inf row gives -inf"""
    m = np.max(np.where(np.isnan(x), -np.inf, x), axis=-1, keepdims=True)
    ms = np.where(np.isfinite(m), m, 0.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        s = np.sum(np.exp(x - ms), axis=-1, keepdims=True)
        return (ms + np.log(s))[..., 0], m[..., 0], s[..., 0]


def score_rows(a, targets, b=None, with_bounds: bool = False):
    """a [M, V] (and b) logits, targets [M] in [-1, V) -> dict of float64 / int arrays [M] named like rca_score_row_t; with_bounds
    also "bound_<float field>" (the row kernel's bound above; rows holding NaN / inf results get bound 0: those are compared as
    classes)."""
    a = np.asarray(a, np.float64)
    M, V = a.shape
    targets = np.asarray(targets, np.int64)
    rows = np.arange(M)
    nan_a = np.isnan(a).any(axis=1)
    out = {}
    lse_a, m_a, s_a = _lse(a)
    out["argmax"] = np.argmax(np.where(np.isnan(a), -np.inf, a), axis=1).astype(np.int64)
    out["max_logit"] = np.where(nan_a, np.nan, m_a)
    out["lse"] = np.where(nan_a, np.nan, lse_a)
    at = a[rows, np.maximum(targets, 0)]
    with np.errstate(invalid="ignore"):
        out["logprob"] = np.where((targets < 0) | nan_a, np.nan, at - lse_a)
    out["flags"] = nan_a.astype(np.int64)
    out["kl"] = np.full(M, np.nan)
    out["base_logprob"] = np.full(M, np.nan)
    out["base_argmax"] = np.full(M, -1, np.int64)
    if b is not None:
        b = np.asarray(b, np.float64)
        nan_b = np.isnan(b).any(axis=1)
        lse_b, m_b, s_b = _lse(b)
        out["base_argmax"] = np.argmax(np.where(np.isnan(b), -np.inf, b), axis=1).astype(np.int64)
        bt = b[rows, np.maximum(targets, 0)]
        with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
            out["base_logprob"] = np.where((targets < 0) | nan_b, np.nan, bt - lse_b)
            pb = np.exp(b - lse_b[:, None])
            mass = np.greater(b, -np.inf)                                         # the base gives the entry mass (false for NaN)
            d = np.where(mass, b - a, 0.0)                                        # 0 * inf counts as 0
            inf_kl = (mass & (a == -np.inf)).any(axis=1)
            d = np.where(np.isinf(d), 0.0, d)
            q = np.sum(np.where(mass, pb, 0.0) * d, axis=1)
            kl = q - lse_b + lse_a
        kl = np.where(inf_kl, np.inf, kl)
        out["kl"] = np.where(nan_a | nan_b, np.nan, kl)
        out["flags"] = out["flags"] + 2 * nan_b.astype(np.int64) + 4 * inf_kl.astype(np.int64)
    if not with_bounds:
        return out
    C, NADD, NRESC = reduction_shape(V)

    def lse_err(x, lse, m, s):
        with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
            p = np.exp(x - lse[:, None])
            arg = u * np.nansum(np.where(p > 0, p * (m[:, None] - x), 0.0), axis=1)
            e = arg + (1 + NRESC) * X + NRESC * u + NADD * u
            eps = e / (1 - e)
            return eps, eps + X * np.abs(np.log(s)) + u * np.abs(lse)

    ok = lambda v: np.isfinite(v)
    eps_a, err_lse_a = lse_err(a, lse_a, m_a, s_a)
    zero = lambda e, v: np.where(ok(v), np.nan_to_num(e, nan=0.0, posinf=0.0), 0.0)
    out["bound_lse"] = zero(err_lse_a, out["lse"])
    out["bound_max_logit"] = np.zeros(M)
    out["bound_logprob"] = zero(err_lse_a + u * (np.abs(at) + np.abs(lse_a)), out["logprob"])
    out["bound_kl"] = np.zeros(M)
    out["bound_base_logprob"] = np.zeros(M)
    if b is not None:
        eps_b, err_lse_b = lse_err(b, lse_b, m_b, s_b)
        out["bound_base_logprob"] = zero(err_lse_b + u * (np.abs(bt) + np.abs(lse_b)), out["base_logprob"])
        with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
            ad = np.abs(d)
            TA = np.sum(np.where(mass, pb, 0.0) * ad, axis=1)
            argk = u * np.nansum(np.where(mass & (pb > 0), pb * (m_b[:, None] - b) * ad, 0.0), axis=1)
            rel = (1 + NRESC) * X + (NRESC + NADD + 2) * u
            e = TA * rel / (1 - rel) + argk + np.abs(q) * (eps_b + u) + u * np.abs(q - lse_b) + u * np.abs(kl) + err_lse_a + err_lse_b
        out["bound_kl"] = zero(e, out["kl"])
    return out


def compare_rows(tag, got, want, floats=FLOATS, verbose=True):
    """got: the structured rows of the device (realtime_codec_agent_amd._native.SCORE_ROW_DTYPE), want: score_rows(...,
    with_bounds=True).  argmax / base_argmax / flags equal; every float within its row's bound, NaN and +-inf as classes.  Prints the
    worst error / bound ratio per field; returns it."""
    worst = {}
    for k in ("argmax", "base_argmax", "flags"):
        assert np.array_equal(np.asarray(got[k], np.int64), want[k]), (tag, k, np.flatnonzero(np.asarray(got[k], np.int64) != want[k])[:8],
                                                                        got[k][:8], want[k][:8])
    for k in floats:
        g, w, bd = np.asarray(got[k], np.float64), want[k], want["bound_" + k]
        fin = np.isfinite(w)
        assert np.array_equal(np.isnan(g), np.isnan(w)), (tag, k, "NaN rows differ", np.flatnonzero(np.isnan(g) != np.isnan(w))[:8])
        assert np.array_equal(g[~fin & ~np.isnan(w)], w[~fin & ~np.isnan(w)]), (tag, k, "infinite rows differ")
        if fin.any():
            err = np.abs(g[fin] - w[fin])
            b = bd[fin]
            i = int(np.argmax(err - b))
            worst[k] = float(np.max(np.where(b > 0, err / np.where(b > 0, b, 1.0), np.where(err > 0, np.inf, 0.0))))
            assert np.all(err <= b), (tag, k, f"row {np.flatnonzero(fin)[i]}: |err| {err[i]:.3e} > bound {b[i]:.3e}")
    if verbose:
        print(f"SCORE {tag}: worst err / bound " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    return worst


def kl_oracle_bound(want_a, want_b, e_a: float, e_b: float):
    """first-order bound of |kl_device - kl_oracle| per row from the two logit tolerances (module docstring), doubled"""
    want_a, want_b = np.asarray(want_a, np.float64), np.asarray(want_b, np.float64)
    la = want_a - _lse(want_a)[0][:, None]
    lb = want_b - _lse(want_b)[0][:, None]
    kl = np.sum(np.exp(lb) * (lb - la), axis=1)
    return 2.0 * (2.0 * e_a + 2.0 * e_b * (np.max(np.abs(lb - la), axis=1) + kl)), kl


def top2_gap(logits):
    """the gap between the largest and the second largest logit of every row"""
    s = np.sort(np.asarray(logits, np.float64), axis=1)
    return s[:, -1] - s[:, -2]


# ------------------------------------------------------------------ the end-to-end cases (shared so that the CPU test can vet the seeds)
E2E_SHAPE = "g4_k768"
E2E_CASES = (("q4_k", 1000), ("q8_0", 1000), ("bf16", 1000), ("bf16", 1001), ("f16", 1001))
E2E_PROMPT = 300            # blocks of 128 + 128 + 44, across the 256-key split
E2E_EVAL_THEN = (37, 150)   # eval 37 tokens, then score 150
FALLBACK_CASES = (("g1_tile32", "bf16"), ("g1_fallback", "q8_0"))
MIN_ARGMAX_ROWS = 0.9


def e2e_case(vocab: int):
    import dataclasses

    import lm_shape_cases as sc
    return dataclasses.replace(sc.BY_NAME[E2E_SHAPE], vocab=vocab, name=f"{E2E_SHAPE}_v{vocab}")
