"""Scoring without a GPU: the float64 reference of the row outputs (tests/score_ref.py) against closed forms, the seams the GPU
test plants its maxima on against the reduction's ownership rule, whether the oracle rows leave the end-to-end argmax check
something to check for the seeds it uses, the window / burn-in table and the aggregation of realtime_codec_agent_amd.lm_quality on
fake rows, and the C ABI: include/rca.h declares rca_lm_score and rca_lm_score_rows_tap and the built library exports them."""
import ctypes
import functools
import math
import os
import re

import numpy as np
import pytest

import lm_shape_cases as sc
import score_ref as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NINF = -np.inf


# ------------------------------------------------------------------ the reference against closed forms
@pytest.mark.parametrize("V", [4, 1000, 1001])
@pytest.mark.parametrize("a0", [0.0, -3.5, 80.0])
def test_uniform_row(V, a0):
    a = np.full((1, V), a0)
    r = sr.score_rows(a, [V - 1], b=a, with_bounds=True)
    assert r["argmax"][0] == 0 and r["base_argmax"][0] == 0 and r["max_logit"][0] == a0
    assert abs(r["lse"][0] - (a0 + math.log(V))) < 1e-12
    assert abs(r["logprob"][0] + math.log(V)) < 1e-12 and r["base_logprob"][0] == r["logprob"][0]
    assert abs(r["kl"][0]) < 1e-12 and r["flags"][0] == 0


def test_one_hot_row():
    V, k, c = 1001, 517, 2.25
    a = np.full((3, V), NINF)
    a[:, k] = c
    r = sr.score_rows(a, [k, 0, -1])
    assert np.all(r["argmax"] == k) and np.all(r["lse"] == c) and np.all(r["max_logit"] == c)
    assert r["logprob"][0] == 0.0 and r["logprob"][1] == NINF and np.isnan(r["logprob"][2])
    assert np.all(np.isnan(r["kl"])) and np.all(r["base_argmax"] == -1)


def test_two_point_rows_and_the_kl_corner_cases():
    V, i, j = 1000, 3, 998
    x, y, p, q = 1.5, -0.5, 0.25, 2.0
    a = np.full((4, V), NINF)
    b = np.full((4, V), NINF)
    a[:, i], a[:, j] = x, y
    b[:, i], b[:, j] = p, q
    b[1, j] = NINF          # the base has no mass at j: the term 0 * (-inf - y) counts as 0 -> kl = -log P(i)
    a[2, j] = NINF          # P has no mass where the base has: kl = +inf
    a[3, 7] = np.nan        # a NaN anywhere in P's row
    r = sr.score_rows(a, [i, i, i, i], b=b)
    la = math.log(math.exp(x) + math.exp(y))
    lb = math.log(math.exp(p) + math.exp(q))
    pb = (math.exp(p - lb), math.exp(q - lb))
    kl = pb[0] * ((p - lb) - (x - la)) + pb[1] * ((q - lb) - (y - la))
    assert abs(r["lse"][0] - la) < 1e-12 and abs(r["logprob"][0] - (x - la)) < 1e-12 and abs(r["base_logprob"][0] - (p - lb)) < 1e-12
    assert abs(r["kl"][0] - kl) < 1e-12 and kl > 0
    assert r["argmax"][0] == i and r["base_argmax"][0] == j
    assert abs(r["kl"][1] - (-(x - la))) < 1e-12 and r["flags"][1] == 0
    assert r["kl"][2] == np.inf and r["flags"][2] == 4 and r["lse"][2] == x
    assert np.isnan(r["kl"][3]) and np.isnan(r["lse"][3]) and np.isnan(r["logprob"][3]) and r["flags"][3] == 1
    assert r["base_logprob"][3] == r["base_logprob"][0]          # the base's row is clean


def test_ties_go_to_the_lowest_index():
    a = np.zeros((1, 1000))
    a[0, [700, 12, 401]] = 5.0
    assert sr.score_rows(a, [-1])["argmax"][0] == 12


def test_the_bound_has_teeth_and_follows_the_reduction():
    """a few 1e-6 for a thousand logits, a few 1e-4 at the deployed vocabulary (1028 additions on the longest path): nowhere near the
    1e-3 a wrong kernel (a dropped chunk: 4 of 1000 equal terms move lse by 4e-3) is off by"""
    assert sr.reduction_shape(1000) == (1, 16, 10) and sr.reduction_shape(259344) == (254, 1028, 263)
    rng = np.random.default_rng(0)
    for V, cap in ((1000, 2e-5), (259344, 4e-4)):
        a = rng.standard_normal((2, V)).astype(np.float32)
        b = (a + 0.1 * rng.standard_normal((2, V))).astype(np.float32)
        r = sr.score_rows(a, [0, V - 1], b=b, with_bounds=True)
        for k in ("lse", "logprob", "kl", "base_logprob"):
            assert np.all(r["bound_" + k] > 0) and np.all(r["bound_" + k] < cap), (V, k, r["bound_" + k])
    flat = np.zeros((1, 1000))
    want = sr.score_rows(flat, [0], with_bounds=True)
    dropped = sr.score_rows(flat[:, :996], [0])
    assert abs(dropped["lse"][0] - want["lse"][0]) > 100 * want["bound_lse"][0]


@pytest.mark.parametrize("V", [1000, 1001, 4099, 259344])
def test_seams_are_seams(V):
    """every group the GPU test plants equal maxima on spans two owners (threads, or iterations of one thread) or the ragged ends"""
    for row in (0, 1, 2, 3):
        groups = sr.seam_indices(V, row)
        assert len(groups) >= 6
        kinds = set()
        for g in groups:
            own = [sr.owner(V, row, i) for i in g]
            assert all(0 <= i < V for i in g) and list(g) == sorted(g)
            t = [o[0] for o in own]
            if len(set(own)) == 1:
                kinds.add("chunk")                       # inside one chunk: the in-thread strict >
            elif len(set(t)) == 1:
                kinds.add("iterations")
            elif {a // 64 for a in t} != {t[0] // 64}:
                kinds.add("waves")
            else:
                kinds.add("lanes")
            if any(o[1] == -1 for o in own):
                kinds.add("ragged")
        need = {"chunk", "lanes", "waves"} | ({"iterations"} if V // 4 > 2 * sr.SCORE_THREADS else set()) | ({"ragged"} if (V % 4 or (row * V) % 4) else set())
        assert need <= kinds, (V, row, need - kinds)


# ------------------------------------------------------------------ the end-to-end cases: do the oracle rows leave something to check?
@functools.lru_cache(maxsize=None)
def _oracle_logits(fmt, vocab):
    import torch
    from oracle import lm_ref
    c = sr.e2e_case(vocab)
    ref = lm_ref.LMRef(c.config(), sc.oracle_weights(c, fmt), kv_dtype=torch.float16)
    return ref.eval(c.ids().tolist()[:sr.E2E_PROMPT]).numpy()


@pytest.mark.parametrize("fmt,vocab", [sr.E2E_CASES[0], sr.E2E_CASES[3]])
def test_oracle_top_two_gap_leaves_the_argmax_check_its_rows(fmt, vocab):
    """the GPU test compares argmax where the oracle's top-two gap exceeds the logprob bound and asserts that 90 % of the rows
    qualify: the oracle alone must meet that for the seeds in use (prompt rows, and the 150 rows behind a 37-token eval)"""
    want = _oracle_logits(fmt, vocab)
    b = 2 * sc.bound(want, sc.TOL_TILE)
    ok = sr.top2_gap(want) > b
    n0, n1 = sr.E2E_EVAL_THEN
    print(f"SCORE oracle {fmt} V={vocab}: {ok.mean():.3f} of the rows have a top-two gap above {b:.3e}")
    assert ok.mean() >= sr.MIN_ARGMAX_ROWS and ok[n0:n0 + n1].mean() >= sr.MIN_ARGMAX_ROWS


def test_kl_oracle_bound_is_small_against_the_kl_it_guards():
    a, b = _oracle_logits("q4_k", 1000), _oracle_logits("bf16", 1000)
    bd, kl = sr.kl_oracle_bound(a, b, sc.bound(a, sc.TOL_TILE), sc.bound(b, sc.TOL_TILE))
    want = sr.score_rows(a, np.full(len(a), -1), b=b)["kl"]
    assert np.allclose(kl, want, rtol=0, atol=1e-12) and np.all(kl > 0) and np.all(bd > 0)
    print(f"SCORE oracle KL(bf16 || q4_k): mean {kl.mean():.4e}, bound mean {bd.mean():.4e}")


# ------------------------------------------------------------------ the CLI's bookkeeping
def test_window_table_and_burn_in():
    from realtime_codec_agent_amd import lm_quality as q
    t = q.plan_windows([10, 3, 25], window=8, burn_in=4)
    assert [tuple(int(x) for x in r) for r in t] == [(0, 0, 8, 4), (2, 0, 8, 4), (2, 8, 8, 4), (2, 16, 8, 4)]
    # stream 0's tail of 2 tokens, stream 1 (3 tokens) and stream 2's tail (1 token) score nothing behind a burn-in of 4
    t = q.plan_windows([10], window=8, burn_in=0)
    assert [tuple(int(x) for x in r) for r in t] == [(0, 0, 8, 0), (0, 8, 2, 0)]
    m = q.scored_mask(8, 4)
    assert m.tolist() == [False] * 4 + [True] * 3 + [False]          # the last position predicts nothing
    assert q.scored_mask(2, 0).tolist() == [True, False]
    for bad in (dict(window=1, burn_in=0), dict(window=8, burn_in=7), dict(window=8, burn_in=-1)):
        with pytest.raises(ValueError):
            q.plan_windows([100], **bad)


def test_aggregation_on_fake_rows():
    from realtime_codec_agent_amd import lm_quality as q
    lp = np.log(np.array([0.5, 0.25, 0.125, 0.5]))
    kl = np.array([0.0, 0.1, 0.2, 0.1])
    rep = q.aggregate(lp, kl, np.array([1, 2, 3, 4]), np.array([1, 2, 0, 4]), base_logprob=lp)
    nll = -lp.mean()
    assert rep["n_scored"] == 4 and abs(rep["nll"] - nll) < 1e-12 and abs(rep["ppl"] - math.exp(nll)) < 1e-12
    assert abs(rep["ppl"] - (2 * 4 * 8 * 2) ** 0.25) < 1e-12 and rep["base_ppl"] == rep["ppl"]
    se = np.std(-lp, ddof=1) / 2.0
    assert abs(rep["nll_se"] - se) < 1e-12 and abs(rep["ppl_se"] - math.exp(nll) * se) < 1e-12
    assert abs(rep["kl_mean"] - 0.1) < 1e-12 and abs(rep["kl_se"] - np.std(kl, ddof=1) / 2.0) < 1e-12
    assert abs(rep["kl_p99"] - np.percentile(kl, 99)) < 1e-12 and rep["kl_max"] == 0.2 and rep["top1_agreement"] == 0.75
    assert "kl_mean" not in q.aggregate(lp)
    with pytest.raises(ValueError):
        q.aggregate(np.array([-1.0, np.nan]))
    with pytest.raises(ValueError):
        q.aggregate(np.zeros(0))


def test_score_streams_masks_and_resets(tmp_path):
    """score_streams against a fake model: every window on a reset context, burn-in and last position dropped, columns concatenated"""
    from realtime_codec_agent_amd import lm_quality as q
    from realtime_codec_agent_amd._native import SCORE_ROW_DTYPE
    from realtime_codec_agent_amd.llm import ScoreResult

    class Fake:
        def __init__(self):
            self.calls, self.n = [], 0

        def reset(self):
            self.n = 0

        def score(self, ids, base=None):
            assert self.n == 0 and (base is None or base.n == 0)
            self.n = len(ids)
            self.calls.append(list(ids))
            rows = np.zeros(len(ids), SCORE_ROW_DTYPE)
            rows["logprob"] = -np.asarray(ids, np.float32) / 10.0          # position i "scores" its own id
            rows["kl"], rows["argmax"], rows["base_argmax"], rows["base_logprob"] = 0.5, np.asarray(ids), 0, -1.0
            return ScoreResult(rows, base is not None)

    np.save(tmp_path / "a.npy", np.arange(10, dtype=np.int32))
    np.save(tmp_path / "b.npy", np.arange(100, 105, dtype=np.int32))
    streams = q.load_streams(str(tmp_path))
    assert [len(s) for s in streams] == [10, 5] and streams[0].dtype == np.int32
    llm, base = Fake(), Fake()
    rep = q.score_streams(llm, streams, window=6, burn_in=2, base=base)
    assert llm.calls == [[0, 1, 2, 3, 4, 5], [6, 7, 8, 9], [100, 101, 102, 103, 104]]
    kept = [2, 3, 4, 8, 102, 103]
    assert rep["n_scored"] == len(kept) and rep["n_windows"] == 3 and abs(rep["nll"] - np.mean(kept) / 10.0) < 1e-6
    assert rep["kl_mean"] == 0.5 and rep["top1_agreement"] == 0.0
    assert "perplexity" in q.format_report(rep) and "top-1" in q.format_report(rep)
    (tmp_path / "empty").mkdir()
    with pytest.raises(ValueError):
        q.load_streams(str(tmp_path / "empty"))


# ------------------------------------------------------------------ the C ABI
def test_header_declares_and_library_exports_the_scoring_calls():
    """without the feature this fails (and with it every GPU test of test_lm_score_gpu.py)"""
    from realtime_codec_agent_amd import _native
    header = open(os.path.join(ROOT, "include", "rca.h")).read()
    assert re.search(r"\bint\s+rca_lm_score\s*\(\s*rca_lm_t\s*\*\s*h\s*,\s*rca_lm_t\s*\*\s*base\s*,", header)
    assert re.search(r"\bint\s+rca_lm_score_rows_tap\s*\(", header)
    m = re.search(r"typedef struct rca_score_row \{(.*?)\} rca_score_row_t;", header, re.S)
    assert m, "rca_score_row_t"
    fields = re.findall(r"\b(\w+)\s*[,;]", m.group(1))
    assert fields == [f for f, _ in _native.ScoreRowC._fields_] == list(_native.SCORE_ROW_DTYPE.names)
    assert ctypes.sizeof(_native.ScoreRowC) == 32 == _native.SCORE_ROW_DTYPE.itemsize
    assert {"rca_lm_score", "rca_lm_score_rows_tap"} <= set(_native.ABI_SYMBOLS)
    if _native.needs_build():
        _native.build()
    lib = _native.lib()
    assert hasattr(lib, "rca_lm_score") and hasattr(lib, "rca_lm_score_rows_tap")
    # bad arguments are rejected before any HIP call
    assert lib.rca_lm_score(None, None, None, 3, None, None) == -1
    assert lib.rca_lm_score_rows_tap(None, None, None, None, 1, None) == -1 and b"null" in lib.rca_last_error()
