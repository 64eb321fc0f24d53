"""rca_lm_score on the device: the row reduction alone (rca_lm_score_rows_tap) against the float64 reference and the bound derived
from the reduction's shape (tests/score_ref.py), then the whole call -- head on the 128-token tiles + row reduction -- against the
fp32 oracle, the state it leaves against rca_lm_eval_async, a base handle (a weight-sharing twin, another format), the fallback
on the exact decode passes, get_logprobs(route="prefill"), the refusals and the captured step graphs.  Every comparison prints its
worst error / bound ratio (-s)."""
import dataclasses
import functools

import numpy as np
import pytest
import torch

import lm_shape_cases as sc
import score_ref as sr
from oracle import lm_ref

pytestmark = pytest.mark.gpu

SAMPLER = dict(top_k=50, top_p=1.0, min_p=0.0, temp=1.0, seed=3)
NINF = np.float32(-np.inf)


def _new(c, fmt, **kw):
    from realtime_codec_agent_amd.llm import LlamaForAlternatingCodeChannels
    llm = LlamaForAlternatingCodeChannels(model_path=f"random:{c.name}", config=c.config(), n_ctx=c.n_ctx, random_seed=c.seed,
                                          init_std=sc.INIT_STD, device=0, weight_format=fmt, **kw)
    assert llm.weight_format == fmt
    return llm


# ------------------------------------------------------------------ the row kernel alone
@functools.lru_cache(maxsize=None)
def _tap_handle(V):
    """a tiny handle whose only job is to carry the vocabulary"""
    c = dataclasses.replace(sc.BY_NAME["g1_tile32"], hidden=64, n_heads=1, n_kv_heads=1, ffn=64, vocab=V, n_ctx=64, name=f"tap_v{V}")
    return _new(c, "bf16")


def _tap_rows(V, M, seed):
    """M rows of logits (+ the base's) and targets.  Row kinds, cycling: random; the maximum planted two or three times across a seam
    of the reduction (sr.seam_indices: a new seam every time); all equal; offset by +80 / -80; -inf entries incl. the two KL corner
    cases; a NaN row between clean rows; an all -inf row.  Targets rotate through argmax, V - 1 and -1."""
    rng = np.random.default_rng(seed)
    a = (2.0 * rng.standard_normal((M, V))).astype(np.float32)
    b = (a + 0.3 * rng.standard_normal((M, V))).astype(np.float32)
    kinds, lowest = [], {}
    planted = 0
    order = ("random", "plant", "equal", "plant", "up80", "ninf", "clean", "nan", "clean", "plant", "down80", "plant", "corner", "allninf")
    for r in range(M):
        kind = order[r % len(order)]
        kinds.append(kind)
        if kind == "plant":
            groups = sr.seam_indices(V, r)
            ga, gb = groups[planted % len(groups)], groups[(planted + 1) % len(groups)]
            planted += 1
            lowest[r] = (min(ga), min(gb))
            a[r, list(ga)] = np.float32(a[r].max() + 1.0)
            b[r, list(gb)] = np.float32(b[r].max() + 0.5)
        elif kind == "equal":
            a[r], b[r] = np.float32(1.25), np.float32(-0.75)
        elif kind == "up80":
            a[r] += np.float32(80.0); b[r] += np.float32(80.0)
        elif kind == "down80":
            a[r] -= np.float32(80.0); b[r] -= np.float32(80.0)
        elif kind == "ninf":        # both rows thinned out, at the same places and at different ones where the BASE has no mass
            hole = rng.random(V) < 0.3
            a[r, hole] = NINF
            b[r, hole | (rng.random(V) < 0.1)] = NINF
            a[r, 0] = b[r, 0] = 1.0
        elif kind == "corner":      # P has no mass at an entry where the base has: kl = +inf
            a[r, rng.integers(0, V, 5)] = NINF
            b[r] = np.where(np.isinf(b[r]), 0.0, b[r])
        elif kind == "nan":
            a[r, int(rng.integers(0, V))] = np.nan
        elif kind == "allninf":
            a[r] = NINF
    am = np.argmax(np.where(np.isnan(a), -np.inf, a), axis=1)
    targets = np.array([(am[r], V - 1, -1)[r % 3] for r in range(M)], np.int32)
    return a, b, targets, kinds, lowest


@pytest.mark.parametrize("with_base", [False, True], ids=["alone", "base"])
@pytest.mark.parametrize("V,Ms", [(1000, (1, 2, 129)), (1001, (1, 2, 129)), (4099, (1, 2, 129)), (259344, (3,))], ids=lambda v: str(v))
def test_row_kernel_against_float64(V, Ms, with_base):
    llm = _tap_handle(V)
    for M in Ms:
        a, b, targets, kinds, lowest = _tap_rows(V, M, seed=V + M)
        want = sr.score_rows(a, targets, b=b if with_base else None, with_bounds=True)
        got = llm.score_rows_tap(a, targets, base_logits=b if with_base else None).rows
        sr.compare_rows(f"tap V={V} M={M} {'base' if with_base else 'alone'}", got, want)
        for r, kind in enumerate(kinds):
            if kind == "equal":
                assert got["argmax"][r] == 0 and abs(float(got["lse"][r]) - (1.25 + np.log(V))) <= want["bound_lse"][r]
            if kind == "plant":
                assert got["argmax"][r] == lowest[r][0] and (not with_base or got["base_argmax"][r] == lowest[r][1])
            if kind == "nan":
                assert np.isnan(got["lse"][r]) and np.isnan(got["logprob"][r]) and np.isnan(got["max_logit"][r]) and got["flags"][r] & 1
                for n in (r - 1, r + 1):
                    if 0 <= n < M:
                        assert kinds[n] == "clean" and np.isfinite(got["lse"][n]) and got["flags"][n] == 0
            if kind == "corner" and with_base:
                assert got["kl"][r] == np.inf and got["flags"][r] == 4
            if kind == "ninf" and with_base:
                assert np.isfinite(got["kl"][r]) and got["flags"][r] == 0
            if targets[r] == -1:
                assert np.isnan(got["logprob"][r])
        if not with_base:
            assert np.all(np.isnan(got["kl"])) and np.all(np.isnan(got["base_logprob"])) and np.all(got["base_argmax"] == -1)


def test_tap_refuses_bad_arguments():
    from realtime_codec_agent_amd._native import RcaError
    llm = _tap_handle(1000)
    a = np.zeros((2, 1000), np.float32)
    for bad in ([0, 1000], [-2, 0]):
        with pytest.raises(RcaError, match=r"rc=-1"):
            llm.score_rows_tap(a, bad)


# ------------------------------------------------------------------ end to end on the gemm128 route
@functools.lru_cache(maxsize=None)
def _llm(fmt, vocab):
    return _new(sr.e2e_case(vocab), fmt)


@functools.lru_cache(maxsize=None)
def _want(fmt, vocab):
    """the oracle's logits of the first 300 ids (float64), computed once per case and shared"""
    c = sr.e2e_case(vocab)
    ref = lm_ref.LMRef(c.config(), sc.oracle_weights(c, fmt), kv_dtype=torch.float16)
    w = ref.eval(c.ids().tolist()[:sr.E2E_PROMPT]).numpy().astype(np.float64)
    w.setflags(write=False)
    return w


@functools.lru_cache(maxsize=None)
def _fallback(name, fmt):
    c = sc.BY_NAME[name]
    ref = lm_ref.LMRef(c.config(), sc.oracle_weights(c, fmt), kv_dtype=torch.float16)
    w = ref.eval(c.ids().tolist()[:sr.E2E_PROMPT]).numpy().astype(np.float64)
    w.setflags(write=False)
    return _new(c, fmt), w


def _ids(vocab):
    return sr.e2e_case(vocab).ids().tolist()


def _fresh(llm, mfma=True):
    llm.set_mfma_prefill(mfma)
    llm.set_graphs(True)
    llm.reset()
    return llm


def _against_oracle(tag, r, want, targets, tol, lo=0):
    """logprob / lse / max_logit of the rows r (positions lo ..) within 2 * bound(want, tol) of the oracle rows, argmax equal wherever
    the oracle's top-two gap exceeds that bound -- which must be at least 90 % of the rows"""
    n = len(r)
    w = want[lo:lo + n]
    ref = sr.score_rows(w, targets)
    B = 2 * sc.bound(want, tol)
    worst = {}
    for k in ("logprob", "lse", "max_logit"):
        g = np.asarray(getattr(r, k), np.float64)
        assert np.array_equal(np.isnan(g), np.isnan(ref[k])), (tag, k)
        worst[k] = float(np.nanmax(np.abs(g - ref[k])))
    sure = sr.top2_gap(w) > B
    print(f"SCORE {tag}: bound {B:.3e}, worst err / bound " + ", ".join(f"{k} {v / B:.3f}" for k, v in worst.items())
          + f"; argmax compared on {sure.mean():.3f} of {n} rows")
    assert all(v <= B for v in worst.values()), (tag, worst, B)
    assert sure.mean() >= sr.MIN_ARGMAX_ROWS, (tag, sure.mean())
    assert np.array_equal(r.argmax[sure], ref["argmax"][sure]), tag
    assert np.all(r.flags == 0)
    return B


def _next_targets(ids, lo, n, last):
    return np.array(ids[lo + 1:lo + n] + [last], np.int32)


@pytest.mark.parametrize("fmt,vocab", sr.E2E_CASES, ids=[f"{f}-v{v}" for f, v in sr.E2E_CASES])
def test_score_matches_oracle_on_the_tiles(fmt, vocab):
    """a 300-token prompt (blocks of 128 + 128 + 44, across the 256-key split; the vocabulary is ragged against the 128-row tiles),
    then eval 37 + score 150 with explicit targets"""
    llm, want, ids = _fresh(_llm(fmt, vocab)), _want(fmt, vocab), _ids(vocab)
    assert llm.prefill_route() == "gemm128"
    P = sr.E2E_PROMPT
    r = llm.score(ids[:P])
    assert llm.n_tokens == P and len(r) == P and r.kl is None and np.isnan(r.logprob[-1])
    _against_oracle(f"{fmt} V={vocab} prompt of {P}", r, want, _next_targets(ids, 0, P, -1), sc.TOL_TILE)
    n0, n1 = sr.E2E_EVAL_THEN
    llm.reset()
    llm.eval(ids[:n0])
    tg = _next_targets(ids, n0, n1, ids[n0 + n1])
    r = llm.score(ids[n0:n0 + n1], targets=tg)
    assert llm.n_tokens == n0 + n1 and np.all(np.isfinite(r.logprob))
    _against_oracle(f"{fmt} V={vocab} eval {n0} + score {n1}", r, want, tg, sc.TOL_TILE, lo=n0)


@pytest.mark.parametrize("fmt,vocab", [("q4_k", 1000), ("bf16", 1001)], ids=["q4_k-v1000", "bf16-v1001"])
def test_state_after_score_is_the_state_after_eval(fmt, vocab):
    """K and V of both layers, n_tokens, the last logits and the next sampled token against a twin that ran rca_lm_eval_async"""
    llm, ids = _fresh(_llm(fmt, vocab)), _ids(vocab)
    P = sr.E2E_PROMPT
    twin = llm.make_kv_shadow(low_priority=False)
    try:
        twin.eval_async(ids[:P])
        twin.sync()
        llm.score(ids[:P])
        assert llm.n_tokens == twin.n_tokens == P
        for layer in (0, 1):
            (k0, v0), (k1, v1) = llm.kv_read(layer, 0, P), twin.kv_read(layer, 0, P)
            assert np.array_equal(k0.view(np.uint16), k1.view(np.uint16)) and np.array_equal(v0.view(np.uint16), v1.view(np.uint16)), layer
        assert np.array_equal(llm._scores[-1].view(np.uint32), twin._scores[-1].view(np.uint32))
        toks = []
        for h in (llm, twin):
            h.init_sampler_for_generate(**SAMPLER)
            toks.append(h.sample())
        assert toks[0] == toks[1] == lm_ref.sample(llm._scores[-1], 50, 1.0, 0.0, 1.0, 3, 0)
    finally:
        twin.close()


def test_twin_as_base_gives_zero_kl():
    fmt, vocab = "q8_0", 1000
    llm, want, ids = _fresh(_llm(fmt, vocab)), _want(fmt, vocab), _ids(vocab)
    P = sr.E2E_PROMPT
    twin = llm.make_kv_shadow(low_priority=False)
    try:
        r = llm.score(ids[:P], base=twin)
        twin.sync()
        assert twin.n_tokens == llm.n_tokens == P
        tg = _next_targets(ids, 0, P, -1)
        bd = sr.score_rows(want, tg, b=want, with_bounds=True)["bound_kl"]
        print(f"SCORE twin base: max |kl| {np.abs(r.kl).max():.3e}, tap bound {bd.min():.3e} .. {bd.max():.3e}")
        assert np.all(np.abs(r.kl) <= bd)
        assert np.array_equal(r.base_logprob.view(np.uint32), r.logprob.view(np.uint32))
        assert np.array_equal(r.argmax, r.base_argmax)
        assert np.array_equal(llm._scores[-1].view(np.uint32), twin._scores[-1].view(np.uint32))
        _against_oracle("q8_0 V=1000 with its twin as base", r, want, tg, sc.TOL_TILE)
    finally:
        twin.close()


def test_bf16_base_of_q4_k():
    vocab = 1000
    llm, base, ids = _fresh(_llm("q4_k", vocab)), _fresh(_llm("bf16", vocab)), _ids(vocab)
    wa, wb = _want("q4_k", vocab), _want("bf16", vocab)
    P = sr.E2E_PROMPT
    r = llm.score(ids[:P], base=base)
    base.sync()
    assert base.n_tokens == llm.n_tokens == P
    tg = _next_targets(ids, 0, P, -1)
    _against_oracle("q4_k V=1000 (base bf16)", r, wa, tg, sc.TOL_TILE)
    ea, eb = sc.bound(wa, sc.TOL_TILE), sc.bound(wb, sc.TOL_TILE)
    ref_b = sr.score_rows(wb, tg)
    err_b = float(np.nanmax(np.abs(r.base_logprob.astype(np.float64) - ref_b["logprob"])))
    agree = sr.top2_gap(wb) > 2 * eb
    assert err_b <= 2 * eb and np.array_equal(r.base_argmax[agree], ref_b["argmax"][agree])
    bd, kl = sr.kl_oracle_bound(wa, wb, ea, eb)
    d = np.abs(r.kl.astype(np.float64) - kl)
    print(f"SCORE KL(bf16 || q4_k): mean {r.kl.mean():.4e} (oracle {kl.mean():.4e}), worst |dkl| / bound {np.max(d / bd):.3f}, "
          f"base logprob err / bound {err_b / (2 * eb):.3f}, top-1 agreement {np.mean(r.argmax == r.base_argmax):.3f}")
    assert np.all(r.kl >= -bd) and np.all(d <= bd)


# ------------------------------------------------------------------ the fallback on the exact decode passes
@pytest.mark.parametrize("name,fmt", sr.FALLBACK_CASES, ids=[f"{n}-{f}" for n, f in sr.FALLBACK_CASES])
def test_fallback_shapes_score_on_the_decode_passes(name, fmt):
    llm, want = _fallback(name, fmt)
    _fresh(llm)
    assert llm.prefill_route() != "gemm128"
    ids = sc.BY_NAME[name].ids().tolist()
    P = sr.E2E_PROMPT
    r = llm.score(ids[:P])
    assert llm.n_tokens == P
    _against_oracle(f"{name}/{fmt} fallback", r, want, _next_targets(ids, 0, P, -1), sc.TOL_EXACT)
    last = llm._scores[-1].copy()
    llm.reset()
    llm.set_mfma_prefill(False)
    llm.eval(ids[:P])
    assert np.array_equal(llm._scores[-1].view(np.uint32), last.view(np.uint32))      # the exact passes, as rca_lm_eval runs them
    llm.set_mfma_prefill(True)


def test_gemm128_shape_with_mfma_prefill_off_scores_on_the_decode_passes():
    fmt, vocab = "q8_0", 1000
    llm, want, ids = _fresh(_llm(fmt, vocab), mfma=False), _want(fmt, vocab), _ids(vocab)
    try:
        P = sr.E2E_PROMPT
        r = llm.score(ids[:P])
        _against_oracle("q8_0 V=1000 with MFMA prefill off", r, want, _next_targets(ids, 0, P, -1), sc.TOL_EXACT)
    finally:
        llm.set_mfma_prefill(True)


# ------------------------------------------------------------------ get_logprobs
def test_get_logprobs_prefill_route_and_default_route_unchanged():
    from realtime_codec_agent_amd.llm import LlamaForAlternatingCodeChannels
    fmt, vocab = "q8_0", 1000
    llm, want, ids = _fresh(_llm(fmt, vocab)), _want(fmt, vocab), _ids(vocab)
    ctx, inp = ids[:40], ids[40:100]
    la = LlamaForAlternatingCodeChannels(model_path="random:twin", n_ctx=1024, share_weights_with=llm, device=0, logits_all=True)
    try:
        dec = la.get_logprobs(ctx, inp)
        assert np.array_equal(dec, la.get_logprobs(ctx, inp, route="decode"))
        # the default route restated (llamacpp_utils.py:30-37 as this handle has always run it): context without logits_all, scored
        # tokens with it, log-softmax on the host
        la.reset()
        la._lib.rca_lm_set_logits_all(la._h, 0)
        la.eval(ctx)
        last_ctx = la._scores[-1].copy()
        la._lib.rca_lm_set_logits_all(la._h, 1)
        la.eval(inp)
        logits = np.concatenate([last_ctx[None, :], la._scores], axis=0)[-len(inp) - 1:-1]
        manual = la.logits_to_logprobs(logits)[range(len(inp)), inp]
        assert np.array_equal(np.asarray(dec).view(np.uint32), manual.view(np.uint32))
        pre = llm.get_logprobs(ctx, inp, route="prefill")
        assert llm.n_tokens == 99 and pre.shape == (60,)
        ref = sr.score_rows(want[39:99], np.array(inp))["logprob"]
        B = 2 * sc.bound(want, sc.TOL_TILE)
        e_pre, e_dec, e_between = (float(np.abs(x).max()) for x in (pre - ref, dec - ref, pre - dec))
        print(f"SCORE get_logprobs: prefill vs oracle {e_pre / B:.3f}, decode vs oracle {e_dec / B:.3f}, prefill vs decode {e_between / B:.3f} of the bound {B:.3e}")
        assert e_pre <= B and e_between <= B
        with pytest.raises(ValueError):
            llm.get_logprobs(ctx, inp, route="tiles")
    finally:
        la.close()


# ------------------------------------------------------------------ refusals and graphs
def test_refused_calls_change_nothing():
    from realtime_codec_agent_amd._native import RcaError
    llm, ids = _fresh(_llm("q8_0", 1000)), _ids(1000)
    other_vocab = _fresh(_llm("bf16", 1001))
    same_vocab = _fresh(_llm("bf16", 1000))
    llm.eval(ids[:50])
    same_vocab.eval(ids[:49])
    before = [x.copy() for x in llm.kv_read(0, 0, 64)], llm._scores[-1].copy()

    def unchanged():
        k, v = llm.kv_read(0, 0, 64)
        assert llm.n_tokens == 50 and np.array_equal(k, before[0][0]) and np.array_equal(v, before[0][1])
        assert np.array_equal(llm._scores[-1], before[1])

    cases = [
        (dict(tokens=ids[:1000]), r"rc=-3"),                                            # 50 + 1000 > n_ctx 1024
        (dict(tokens=ids[:10] + [1000]), r"rc=-1"),                                     # an id outside the vocabulary
        (dict(tokens=ids[:3], targets=[1, 1000, 2]), r"rc=-1"),                         # a target outside it
        (dict(tokens=ids[:3], targets=[1, -2, 2]), r"rc=-1"),
        (dict(tokens=ids[:20], base=other_vocab), r"rc=-1"),                            # base on another vocabulary
        (dict(tokens=ids[:20], base=same_vocab), r"rc=-1"),                             # base at another n_tokens
        (dict(tokens=ids[:20], base=llm), r"rc=-1"),                                    # the handle as its own base
    ]
    for kw, rc in cases:
        with pytest.raises(RcaError, match=rc):
            llm.score(**kw)
        unchanged()
        assert same_vocab.n_tokens == 49 and other_vocab.n_tokens == 0
    with pytest.raises(ValueError):
        llm.score(ids[:3], targets=[1, 2])
    assert len(llm.score([])) == 0
    unchanged()


def test_captured_step_graphs_survive_a_score():
    """steps are captured, a score runs (first use: it allocates its scratch), and the next step still replays and equals an eager one"""
    llm, ids = _fresh(_llm("q8_0", 1000)), _ids(1000)
    llm.init_sampler_for_generate(**SAMPLER)
    llm.eval(ids[:20])
    for i in range(3):                                   # the replayed steady-state step
        llm.step(ids[20 + 2 * i:22 + 2 * i])
    n = llm.n_tokens
    llm.score(ids[n:n + 150])
    n = llm.n_tokens
    out = []
    for graphs in (True, False):
        llm.set_graphs(graphs)
        llm.n_tokens = n
        llm.init_sampler_for_generate(**SAMPLER)
        tok = llm.step(ids[n:n + 2])
        out.append((tok, llm._scores[-1].copy()))
    llm.set_graphs(True)
    assert out[0][0] == out[1][0] and np.array_equal(out[0][1].view(np.uint32), out[1][1].view(np.uint32))
