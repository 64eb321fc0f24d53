"""The context shift of several handles in one call on the GPU (rca_lm_kv_remove_many, llm.kv_remove_many, LlamaBatch.kv_remove,
RealtimeAgentBatch(batch_shift_trims=True)).

The contract is bit equality with the single call, so every check has the same form: for each member two weight-sharing twins, A_k
(goes through the one batched call) and B_k (takes its own kv_remove), evaluate the same tokens; their caches are compared before
the shift (equal inputs) and after it -- n_tokens, the _input_ids mirror and the raw K / V rows [0, n_tokens) of every layer with
np.array_equal.  No tolerance anywhere.  Models are the 2-layer cases of tests/test_kv_shift_gpu.py.

Fails on a tree without the call: the symbol, kv_remove_many and the driver's flag do not exist."""
import functools
import os
import re

import numpy as np
import pytest

import lm_shape_cases as sc
from conftest import rich_signal

pytestmark = pytest.mark.gpu

SAMPLER = dict(top_k=50, top_p=1.0, min_p=0.0, temp=1.0, seed=3)
# (n, p0, p1): the seven geometries of tests/test_kv_shift_gpu.py::GEOMETRIES
GEOS = [(900, 20, 21),       # delta 1: maximal overlap, a tail over four slabs
        (900, 7, 44),
        (600, 10, 400),      # delta above the tail and above 256: the direct route
        (300, 0, 100),
        (520, 256, 512),     # on the slab seams (delta 256: the smallest direct slab)
        (300, 100, 300),     # pure truncation
        (300, 50, 50)]       # no-op


def _group():
    """members per launch group, as include/rca.h states it"""
    header = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "rca.h")
    return int(re.search(r"#define RCA_LM_KV_REMOVE_GROUP (\d+)", open(header).read()).group(1))


@functools.lru_cache(maxsize=None)
def _parent(name):
    from realtime_codec_agent_amd.llm import LlamaForAlternatingCodeChannels
    c = sc.BY_NAME[name]
    return LlamaForAlternatingCodeChannels(model_path=f"random:{name}", config=c.config(), n_ctx=c.n_ctx, random_seed=c.seed,
                                           init_std=sc.INIT_STD, device=0)


_POOL = {}


def _twins(name, count):
    """the first `count` twins of the model's pool (made once, reset before every use)"""
    from realtime_codec_agent_amd.llm import LlamaForAlternatingCodeChannels
    parent = _parent(name)
    pool = _POOL.setdefault(name, [])
    while len(pool) < count:
        pool.append(LlamaForAlternatingCodeChannels(model_path=parent.model_path, n_ctx=parent._n_ctx, share_weights_with=parent, device=0))
    for m in pool[:count]:
        m.set_mfma_prefill(True)
        m.set_graphs(True)
        m.reset()
    return pool[:count]


def _read_all(llm, n):
    return [tuple(x.view(np.uint16).copy() for x in llm.kv_read(l, 0, n)) for l in range(llm.config.n_layers)] if n else []


def _same_rows(a, b):
    return len(a) == len(b) and all(np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1]) for x, y in zip(a, b))


def _assert_same(tag, a, b):
    assert a.n_tokens == b.n_tokens, (tag, a.n_tokens, b.n_tokens)
    n = a.n_tokens
    assert np.array_equal(np.asarray(a._input_ids[:n]), np.asarray(b._input_ids[:n])), (tag, "_input_ids")
    assert _same_rows(_read_all(a, n), _read_all(b, n)), (tag, "cache rows")


def _pairs(name, geos):
    """A_k, B_k for every geometry, both holding the first n tokens of the model's id stream; caches equal before the shift"""
    ids = sc.BY_NAME[name].ids().tolist()
    tw = _twins(name, 2 * len(geos))
    A, B = tw[:len(geos)], tw[len(geos):]
    for k, (n, _, _) in enumerate(geos):
        A[k].eval(ids[:n])
        B[k].eval(ids[:n])
        _assert_same((name, k, "before"), A[k], B[k])
    return A, B


def _shift_and_compare(name, geos, staged_only=False):
    from realtime_codec_agent_amd.llm import kv_remove_many
    A, B = _pairs(name, geos)
    for k, (n, p0, p1) in enumerate(geos):
        B[k].kv_remove(p0, p1)
    kv_remove_many(A, [(p0, p1) for _, p0, p1 in geos], staged_only=staged_only)
    for k, (n, p0, p1) in enumerate(geos):
        assert A[k].n_tokens == n - (p1 - p0)
        _assert_same((name, k, geos[k]), A[k], B[k])


@pytest.mark.parametrize("route", ["auto", "staged"])
@pytest.mark.parametrize("name", ["g4_tile32", "g2_tile32"])
def test_all_seven_geometries_in_one_call(name, route):
    """seven deltas in one launch group: staged and direct members side by side ("auto"), and every member staged"""
    _shift_and_compare(name, GEOS, staged_only=route == "staged")


def test_full_ragged_cache_nctx700():
    _shift_and_compare("nctx700", [(700, 5, 130), (300, 0, 100)])


@pytest.mark.parametrize("extra", [1, 2], ids=["group+1", "2group+1"])
def test_more_members_than_one_launch_group(extra):
    g = _group()
    n_h = extra * g + 1
    _shift_and_compare("g4_tile32", [GEOS[k % len(GEOS)] for k in range(n_h)])


def test_the_class_attribute_and_the_package_export():
    from realtime_codec_agent_amd import llm as L
    import realtime_codec_agent_amd as pkg
    assert pkg.kv_remove_many is L.kv_remove_many
    A, B = _pairs("g2_tile32", GEOS[:3])
    for k, (n, p0, p1) in enumerate(GEOS[:3]):
        B[k].kv_remove(p0, p1)
    L.LlamaForAlternatingCodeChannels.kv_remove_many(A, [(p0, p1) for _, p0, p1 in GEOS[:3]])
    for k in range(3):
        _assert_same(("class attribute", k), A[k], B[k])


def test_a_bystander_twin_is_not_touched():
    from realtime_codec_agent_amd.llm import kv_remove_many
    name = "g2_tile32"
    ids = sc.BY_NAME[name].ids().tolist()
    tw = _twins(name, 4)
    for m in tw:
        m.eval(ids[:600])
    by = tw[3]
    n_ctx = by._n_ctx
    before, logits = _read_all(by, n_ctx), by._scores[-1].copy()
    kv_remove_many(tw[:3], [(20, 21), (10, 400), (0, 300)])
    assert by.n_tokens == 600
    assert _same_rows(_read_all(by, n_ctx), before)
    assert np.array_equal(by._scores[-1], logits)


def test_captured_graphs_stay_valid_across_the_call():
    """every A_k and B_k steps twice before the shift (the second step replays a captured graph) and twice after it"""
    from realtime_codec_agent_amd.llm import kv_remove_many
    name = "g4_tile32"
    ids = sc.BY_NAME[name].ids().tolist()
    geos = [GEOS[0], GEOS[2], GEOS[3]]
    A, B = _pairs(name, geos)
    out = {}
    for side, hs in (("A", A), ("B", B)):
        for k, m in enumerate(hs):
            m.init_sampler_for_generate(**SAMPLER)
            n = geos[k][0]
            out[side, k] = [(m.step(ids[n:n + 2]), m._scores[-1].copy()), (m.step(ids[n + 2:n + 4]), m._scores[-1].copy())]
    for k, (n, p0, p1) in enumerate(geos):
        B[k].kv_remove(p0, p1)
    kv_remove_many(A, [(p0, p1) for _, p0, p1 in geos])
    for side, hs in (("A", A), ("B", B)):
        for k, m in enumerate(hs):
            n = geos[k][0]
            out[side, k] += [(m.step(ids[n + 4:n + 6]), m._scores[-1].copy()), (m.step(ids[n + 6:n + 8]), m._scores[-1].copy())]
    for k in range(len(geos)):
        for (ta, la), (tb, lb) in zip(out["A", k], out["B", k]):
            assert ta == tb and np.array_equal(la, lb), k
        _assert_same(("graphs", k), A[k], B[k])


def test_pending_eval_async_is_settled_first():
    from realtime_codec_agent_amd.llm import kv_remove_many
    name = "g2_tile32"
    ids = sc.BY_NAME[name].ids().tolist()
    a0, a1, b0, b1 = _twins(name, 4)
    for m in (a0, a1, b0, b1):
        m.eval(ids[:400])
    b0.eval(ids[400:600])              # a long eval: the arithmetic of eval_async
    a1.eval(ids[400:600])
    b1.eval(ids[400:600])
    b0.kv_remove(30, 200)
    b1.kv_remove(0, 300)
    a0.eval_async(ids[400:600])        # still running when the call arrives
    kv_remove_many([a1, a0], [(0, 300), (30, 200)])
    _assert_same("pending member", a0, b0)
    _assert_same("its companion", a1, b1)


def test_refusals_change_nothing_and_name_the_member():
    from realtime_codec_agent_amd._native import RcaError
    from realtime_codec_agent_amd.llm import LlamaForAlternatingCodeChannels, kv_remove_many
    name = "g2_tile32"
    c = sc.BY_NAME[name]
    ids = c.ids().tolist()
    a, b, d = _twins(name, 3)
    for m in (a, b, d):
        m.eval(ids[:300])
    q8 = LlamaForAlternatingCodeChannels(model_path=a.model_path, n_ctx=a._n_ctx, share_weights_with=_parent(name), device=0, kv_format="q8_0")
    other = LlamaForAlternatingCodeChannels(model_path=f"random:{name}", config=c.config(), n_ctx=c.n_ctx, random_seed=c.seed,
                                            init_std=sc.INIT_STD, device=0)        # the same dimensions, its own weights
    try:
        q8.eval(ids[:300])
        other.eval(ids[:300])
        before = [_read_all(m, 300) for m in (a, b, d)]
        mirrors = [np.asarray(m._input_ids[:300]).copy() for m in (a, b, d)]
        ok = (10, 60)
        for llms, spans, rc, pat in (([], [], -1, r"0 handles"),
                                     ([a] * 65, [ok] * 65, -1, r"65 handles"),
                                     ([a, b, a], [ok] * 3, -1, r"handle 2 is handle 0 again"),
                                     ([a, b, other], [ok] * 3, -1, r"handle 2 does not share"),
                                     ([a, q8, b], [ok] * 3, -3, r"handle 1 keeps a q8_0"),
                                     ([a, b, d], [ok, (60, 50), ok], -1, r"of handle 1 is not a span"),
                                     ([a, b, d], [ok, ok, (10, 301)], -1, r"of handle 2 is not a span"),
                                     ([a, b, d], [(-1, 5), ok, ok], -1, r"of handle 0 is not a span")):
            with pytest.raises(RcaError, match=pat) as e:
                kv_remove_many(llms, spans)
            assert f"rc={rc}" in str(e.value), str(e.value)
            for m, rows, ids_before in zip((a, b, d), before, mirrors):
                assert m.n_tokens == 300
                assert np.array_equal(np.asarray(m._input_ids[:300]), ids_before)
                assert _same_rows(_read_all(m, 300), rows)
        with pytest.raises(RcaError, match="q8_0"):
            kv_remove_many([q8, a], [ok, ok])
        assert q8.n_tokens == 300 and other.n_tokens == 300
    finally:
        other.close()
        q8.close()


# ------------------------------------------------------------------ the driver
CHUNK, TICKS = 1280, 42
_SIG = [rich_signal(CHUNK * TICKS, 60 + s) for s in range(8)]


def test_llama_batch_kv_remove_over_member_indices():
    """a model on the 128-token tiles (what LlamaBatch needs): members 2 and 0 through the batch, members 3 and 1 through their own calls"""
    from realtime_codec_agent_amd.llm import LlamaBatch
    llms = [a.resources.llm for a in _make_agents(4)]
    ids = np.random.default_rng(5).integers(0, 259344, 700).tolist()
    batch = LlamaBatch(llms)
    try:
        for m in llms:
            m.reset()
        for m, n in zip(llms, (700, 700, 400, 400)):
            m.eval(ids[:n])
        _assert_same("before", llms[0], llms[1])
        _assert_same("before", llms[2], llms[3])
        llms[1].kv_remove(3, 330)
        llms[3].kv_remove(10, 12)
        with pytest.raises(ValueError):
            batch.kv_remove([4], [(0, 1)])
        batch.kv_remove([2, 0], [(10, 12), (3, 330)])
        _assert_same("member 0", llms[0], llms[1])
        _assert_same("member 2", llms[2], llms[3])
    finally:
        batch.close()
        for m in llms:
            m.close()


def _make_agents(n):
    """the sessions of tests/test_agent_batch_gpu.py in shift mode; the context limit sits just below a chunk boundary, so every trim
    falls due before the first step of a frame (where the driver can see it), never between two steps, and at 27 chunks, after the
    codec windows have filled (tick 24), from where on every tick is planned as a one-replay frame: trims at ticks 27, 31, 35, 39"""
    from realtime_codec_agent_amd.llm import LMConfig
    from realtime_codec_agent_amd.realtime_agent_config import RealtimeAgentConfig
    from realtime_codec_agent_amd.realtime_agent_resources import RealtimeAgentResources
    from realtime_codec_agent_amd.realtime_agent_v2 import RealtimeAgent
    lm = LMConfig(vocab_size=259344, hidden=256, n_layers=2, n_heads=4, n_kv_heads=2, head_dim=64, ffn=512)
    res = [RealtimeAgentResources(llm_model_path="random:small", llm_n_ctx=4096, llm_config=lm, with_aux_llm=False, llm_random_seed=3)]
    res += [res[0].clone_for_self_play() for _ in range(n - 1)]
    at = res[0].audio_tokenizer
    per_chunk = 2 * int(0.08 * at.framerate)            # frames of both channels a chunk adds
    per_sec = at.framerate * 2
    cfg = RealtimeAgentConfig(chunk_size_secs=0.08, use_whisper=False, force_trans_after_inactivity_secs=0.0,
                              force_response_after_inactivity_secs=0.0, max_context_secs=(27 * per_chunk - 1) / per_sec,
                              trim_by_secs=4 * per_chunk / per_sec)
    return [RealtimeAgent(resources=r, config=cfg, kv_trim_mode="shift") for r in res]


def _drive(n, flag):
    from realtime_codec_agent_amd import RealtimeAgentBatch
    agents = _make_agents(n)
    drv = RealtimeAgentBatch(agents, min_batch=1, batch_shift_trims=flag)
    outs, trim_ticks = [], 0
    for t in range(TICKS):
        was = [a.trim_to_secs for a in agents]
        outs.append(drv.process_audio([_SIG[s][t * CHUNK:(t + 1) * CHUNK] for s in range(n)]))
        moved = [a.trim_to_secs != w for a, w in zip(agents, was)]
        assert all(moved) or not any(moved), (t, moved)       # sessions that start together trim together
        trim_ticks += 1 if moved[0] else 0
    state = [(list(a.input_ids), a.resources.llm.n_tokens, _read_all(a.resources.llm, a.resources.llm.n_tokens), a.trim_to_secs) for a in agents]
    counters = (drv.fused_shift_calls, drv.fused_shift_trims, drv.fused_ticks)
    drv.close()
    return outs, state, counters, trim_ticks


@pytest.mark.parametrize("n", [4, 8])
def test_the_driver_with_batched_shift_trims_equals_the_driver_without(n):
    on, s_on, c_on, trims_on = _drive(n, True)
    off, s_off, c_off, trims_off = _drive(n, False)
    print(f"KVSHIFTMANY driver n={n}: trim ticks {trims_on}, fused shift calls / trims {c_on[:2]}, fused ticks {c_on[2]}")
    assert trims_on == trims_off >= 2
    assert c_off[:2] == (0, 0)
    assert c_on[0] == trims_on and c_on[1] == n * trims_on, (c_on, trims_on)
    assert c_on[2] == c_off[2] >= 10
    for t in range(TICKS):
        for s in range(n):
            assert np.array_equal(on[t][s], off[t][s]), ("PCM of agent", s, "tick", t)
    for s, (a, b) in enumerate(zip(s_on, s_off)):
        assert a[0] == b[0], ("input_ids of agent", s)
        assert a[1] == b[1] and a[3] == b[3], ("n_tokens / trim_to_secs of agent", s)
        assert _same_rows(a[2], b[2]), ("final cache of agent", s)
