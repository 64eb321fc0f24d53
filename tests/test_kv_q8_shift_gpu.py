"""The context shift on a q8_0 KV cache on the GPU (rca_lm_set_kv_shift_requant + rca_lm_kv_remove / rca_lm_kv_remove_many), against
tests/kv_q8_shift_ref.py:
  1. planted rows, the kernel alone: untouched rows, V blocks bit for bit, K inside the bound of kv_q8_shift_ref.shift_bound, full scale;
  2. GPU against GPU, bit for bit: Q8(the fp16 kernel's shift of the de-quantised rows) == the q8_0 kernel's blocks;
  3. kv_remove_many (one launch group and two, staged and direct members side by side) == each handle's own kv_remove;
  4. logits on a shifted q8_0 cache against the oracle carrying the same shifts;
  5. captured graphs across a shift, twins;
  6. refusals and inheritance of the switch;
  7. the agent in shift mode over q8_0 objects, alone and under RealtimeAgentBatch(batch_shift_trims=True).
Models: the 2-layer cases g1_fallback, g4_tile32, g4_k768 of tests/lm_shape_cases.py (kv_q8_spread.E2E_CASES: one per prefill route).
Every test fails on a library without rca_lm_set_kv_shift_requant (the constructor argument does not exist)."""
import functools

import numpy as np
import pytest

import kv_q8_ref as kr
import kv_q8_shift_ref as qs
import kv_q8_shift_spread as qsp
import lm_shape_cases as sc
from conftest import rich_signal

pytestmark = pytest.mark.gpu

SAMPLER = dict(top_k=50, top_p=1.0, min_p=0.0, temp=1.0, seed=3)
MODELS = ("g1_fallback", "g4_tile32", "g4_k768")
FMT = {name: fmt for name, fmt in qsp.CASES.values()}
ROUTE = {name: route for route, (name, _) in qsp.CASES.items()}
# (n, p0, p1): the geometries of tests/test_kv_shift_gpu.py::GEOMETRIES
GEOS = [(900, 20, 21),       # delta 1: maximal overlap, the tail spans four 256-position slabs
        (900, 7, 44),        # odd delta, unaligned
        (600, 10, 400),      # delta greater than the tail
        (300, 0, 100),       # no header
        (520, 256, 512),     # on the slab seams
        (300, 100, 300),     # pure truncation: launches nothing
        (300, 50, 50)]       # no-op


def _L():
    from realtime_codec_agent_amd.llm import LlamaForAlternatingCodeChannels
    return LlamaForAlternatingCodeChannels


def _err():
    from realtime_codec_agent_amd import _native
    return _native.RcaError


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint16) if a.dtype == np.float16 else a


@functools.lru_cache(maxsize=None)
def _parent(name):
    c = sc.BY_NAME[name]
    llm = _L()(model_path=f"random:{name}", config=c.config(), n_ctx=c.n_ctx, random_seed=c.seed, init_std=sc.INIT_STD, device=0,
               weight_format=FMT[name], kv_format="q8_0", kv_shift_requant=True)
    assert llm.kv_format == "q8_0" and llm.kv_shift_requant is True and llm.prefill_route() == ROUTE[name]
    return llm


_POOL = {}


def _twins(name, count, kv_format=None):
    """the first `count` twins of the model's pool in that format (made once, reset before every use); q8_0 twins inherit the switch"""
    parent = _parent(name)
    pool = _POOL.setdefault((name, kv_format), [])
    while len(pool) < count:
        pool.append(_L()(model_path=parent.model_path, n_ctx=parent._n_ctx, share_weights_with=parent, device=0, kv_format=kv_format))
    for m in pool[:count]:
        m.set_mfma_prefill(True)
        m.set_graphs(True)
        m.reset()
    return pool[:count]


@functools.lru_cache(maxsize=None)
def _planted(name):
    """K and V rows for positions [0, 900) of each layer (fixed seeds: tests/test_kv_q8_shift_cpu.py checks the mutants on them)"""
    c = sc.BY_NAME[name]
    out = []
    for l in range(2):
        K = qs.planted_rows(np.random.default_rng(2026 + l), 900, c.n_kv_heads)
        V = (np.random.default_rng(3026 + l).standard_normal((900, c.n_kv_heads, 64)) * 3).astype(np.float16)
        out.append((K, V))
    return out


def _plant(llm, name, n, deq=False):
    """write the planted rows [0, n) of every layer (deq: their fake-quantised values, for an fp16 handle) and set n_tokens = n"""
    ids = sc.BY_NAME[name].ids().tolist()
    llm.eval(ids[:4])                                     # logits to keep readable
    for l, (K, V) in enumerate(_planted(name)):
        llm.kv_write(l, 0, kr.fake_quant(K[:n]) if deq else K[:n], kr.fake_quant(V[:n]) if deq else V[:n])
    llm.n_tokens = n


def _read_q8(llm, n):
    return [llm.kv_read_q8(l, 0, n) for l in range(llm.config.n_layers)] if n else []


def _same_blocks(a, b):
    return len(a) == len(b) and all(np.array_equal(_bits(x), _bits(y)) for la, lb in zip(a, b) for x, y in zip(la, lb))


# ------------------------------------------------------------------ 1. planted rows, the kernel alone
@pytest.mark.parametrize("n,p0,p1", GEOS, ids=[f"{g[0]}-{g[1]}-{g[2]}" for g in GEOS])
@pytest.mark.parametrize("name", MODELS)
def test_planted_rows_after_remove(name, n, p0, p1):
    c = sc.BY_NAME[name]
    llm = _twins(name, 1)[0]
    _plant(llm, name, n)
    logits = llm._scores[-1].copy()
    before = _read_q8(llm, n)
    for l, (K, V) in enumerate(_planted(name)):           # kv_write quantises with the passes' kernel: the blocks are known bit for bit
        wq, wd = kr.quant_rows(K[:n])
        assert np.array_equal(before[l][0], wq) and np.array_equal(_bits(before[l][1]), _bits(wd))
    llm.kv_remove(p0, p1)
    delta, moved = p1 - p0, n - p1
    assert llm.n_tokens == n - delta
    assert np.array_equal(llm._scores[-1], logits)
    after = _read_q8(llm, n - delta)
    inv_freq = qs.table_inv_freq(c.config())
    for l, ((kq, kd, vq, vd), (aq, ad, avq, avd)) in enumerate(zip(before, after)):
        for x, y in ((kq, aq), (kd, ad), (vq, avq), (vd, avd)):
            assert np.array_equal(_bits(x[:p0]), _bits(y[:p0])), (l, "rows below the cut")
        assert np.array_equal(avq[p0:], vq[p1:]) and np.array_equal(_bits(avd[p0:]), _bits(vd[p1:])), (l, "moved V blocks")
        if delta == 0 or moved == 0:
            assert np.array_equal(aq, kq[:n - delta]) and np.array_equal(_bits(ad), _bits(kd[:n - delta])), (l, "nothing moves")
            continue
        ratio = qs.worst_ratio(aq[p0:], ad[p0:], kq[p1:], kd[p1:], delta, inv_freq)
        print(f"KVQ8SHIFT {name} n={n} [{p0}, {p1}) layer {l}: K max |d| / bound = {ratio:.3f} over {aq[p0:].size} values")
        assert ratio <= 1.0, (name, l, ratio)
        live = _bits(ad[p0:]).reshape(-1) != 0
        peak = np.abs(aq[p0:].reshape(-1, 32).astype(np.int32)).max(-1)
        assert live.any() and (peak[live] == 127).all(), (l, "a live block is not at full scale")
    if delta == 0 or moved == 0:                          # the rows past the new n_tokens are stale, not rewritten
        assert _same_blocks(_read_q8(llm, n), before)


# ------------------------------------------------------------------ 2. GPU against GPU, bit for bit
@pytest.mark.parametrize("n,p0,p1", GEOS[:5], ids=[f"{g[0]}-{g[1]}-{g[2]}" for g in GEOS[:5]])
@pytest.mark.parametrize("name", MODELS)
def test_q8_shift_is_q8_of_the_fp16_shift(name, n, p0, p1):
    """the same planted blocks, de-quantised on the host, in an fp16 twin whose kv_remove is the fp16 kernel: Q8 of its rows afterwards
    == the q8_0 handle's blocks after its own kv_remove, q and d16, every layer (what the shared rotation helper exists for).  Bit for
    bit on every row that moved.  The rows below the cut were planted, not produced by a shift, and are compared through their
    de-quantised values: a planted block whose scale underflows to fp16 zero (edge_rows class 3) keeps non-zero int8 values that
    Q8(its de-quantised zeros) cannot give back."""
    q8 = _twins(name, 1)[0]
    f16 = _twins(name, 1, "f16")[0]
    assert f16.kv_format == "f16" and not f16.kv_shift_requant
    _plant(q8, name, n)
    _plant(f16, name, n, deq=True)
    q8.kv_remove(p0, p1)
    f16.kv_remove(p0, p1)
    m = n - (p1 - p0)
    for l in range(2):
        kq, kd, _, _ = q8.kv_read_q8(l, 0, m)
        kf, vf = f16.kv_read(l, 0, m)
        wq, wd = kr.quant_rows(kf[p0:])
        assert np.array_equal(kq[p0:], wq), f"{name} layer {l} K: int8 values differ at {np.argwhere(kq[p0:] != wq)[:4].tolist()}"
        assert np.array_equal(_bits(kd[p0:]), _bits(wd)), f"{name} layer {l} K: scales differ at {np.argwhere(_bits(kd[p0:]) != _bits(wd))[:4].tolist()}"
        assert np.array_equal(_bits(kr.dequant(kq[:p0], kd[:p0])), _bits(kf[:p0])), f"{name} layer {l}: K rows below the cut"
        assert np.array_equal(_bits(q8.kv_read(l, 0, m)[1]), _bits(vf)), f"{name} layer {l}: the de-quantised V rows are not the fp16 twin's"


# ------------------------------------------------------------------ 3. many
@pytest.mark.parametrize("staged_only", [False, True], ids=["auto", "staged"])
@pytest.mark.parametrize("n_h", [3, 9])
def test_remove_many_equals_each_handles_own_remove(n_h, staged_only):
    """3 handles (one launch group) and 9 (two): deltas 1, 390 and 256 in turn, so that staged and direct members share a launch;
    every A_k through the one call, every B_k through its own kv_remove; a bystander twin is unchanged"""
    from realtime_codec_agent_amd.llm import kv_remove_many
    name = "g4_tile32"
    geos = [(GEOS[0], GEOS[2], GEOS[4])[k % 3] for k in range(n_h)]
    tw = _twins(name, 2 * n_h + 1)
    A, B, by = tw[:n_h], tw[n_h:2 * n_h], tw[2 * n_h]
    for k, (n, _, _) in enumerate(geos):
        _plant(A[k], name, n)
        _plant(B[k], name, n)
    _plant(by, name, 600)
    by_before = _read_q8(by, by._n_ctx)
    for k, (n, p0, p1) in enumerate(geos):
        B[k].kv_remove(p0, p1)
    kv_remove_many(A, [(p0, p1) for _, p0, p1 in geos], staged_only=staged_only)
    for k, (n, p0, p1) in enumerate(geos):
        assert A[k].n_tokens == B[k].n_tokens == n - (p1 - p0)
        assert _same_blocks(_read_q8(A[k], A[k].n_tokens), _read_q8(B[k], B[k].n_tokens)), (k, geos[k])
    assert by.n_tokens == 600 and _same_blocks(_read_q8(by, by._n_ctx), by_before)


# ------------------------------------------------------------------ 4. logits
def _compare(tag, got, want, tol):
    d, b = float(np.abs(got - want).max()), sc.bound(want, tol)
    print(f"KVQ8SHIFT {tag}: max|dlogit| = {d:.3e}, bound {b:.3e} (tol {tol:g}), ratio {d / b:.3f}")
    assert d <= b, (tag, d, b)


@pytest.mark.parametrize("route", list(qsp.CASES))
def test_logits_on_a_shifted_q8_cache(route):
    """A q8_0 handle evaluated to 300 tokens; its blocks, de-quantised, become the oracle's cache, so both sides start the shift from
    identical rows.  Then kv_remove [20, 120), a 2-token decode, a 40-token prefill, kv_remove [5, 60), another decode
    (kv_q8_shift_spread.sequence), each against Q8KVRef carrying the same shifts (kv_remove_q8_ref).  Tolerance, in units of
    max(1, |logit|max), of the form of test_kv_q8_gpu.py::_tol: the route's lm_shape_cases tolerance (TOL_EXACT 1e-3 on the GEMV route,
    TOL_TILE 2e-3 on the tile routes) plus 4 x the spread an fp16-ulp disagreement ahead of the quantisers causes, measured on the CPU
    by tests/kv_q8_shift_spread.py over 5 seeds: gemv 2.11e-3, tile32 2.63e-3, gemm128 1.13e-2 -> 9.44e-3 / 1.25e-2 / 4.72e-2."""
    import torch
    name, fmt = qsp.CASES[route]
    c = sc.BY_NAME[name]
    ids = c.ids().tolist()[:qsp.PROMPT + 44]
    tol = (sc.TOL_EXACT if route == "gemv" else sc.TOL_TILE) + 4.0 * qsp.SPREAD[route]
    llm = _twins(name, 1)[0]
    llm.eval(ids[:qsp.PROMPT])
    ref = kr.Q8KVRef(c.config(), sc.oracle_weights(c, fmt))
    ref.n_tokens = qsp.PROMPT
    for l in range(2):
        k, v = llm.kv_read(l, 0, qsp.PROMPT)                                    # the de-quantised blocks
        ref.k[l] = torch.from_numpy(np.ascontiguousarray(k.transpose(1, 0, 2)).astype(np.float32))
        ref.v[l] = torch.from_numpy(np.ascontiguousarray(v.transpose(1, 0, 2)).astype(np.float32))
    want = qsp.oracle_sequence(ref, ids)

    def evaluate(tokens):
        llm.eval(tokens)
        return llm._fetch_logits().copy()

    got = qsp.sequence(ids, evaluate, llm.kv_remove)
    assert llm.n_tokens == ref.n_tokens == 189
    for i, step in enumerate(("decode after one remove", "40-token prefill after one remove", "decode after a second remove")):
        _compare(f"{route} {step}", got[i], want[i], tol)


# ------------------------------------------------------------------ 5. graphs and twins
@pytest.mark.parametrize("use_frame", [False, True], ids=["step", "frame"])
def test_captured_graphs_stay_valid_across_a_q8_remove(use_frame):
    """the pattern of test_kv_shift_gpu.py::test_captured_graphs_stay_valid_across_a_remove on a q8_0 handle (n_ctx 1536): graphs of two
    context buckets captured, a remove takes the context back into the first; tokens and logits equal to the run without graph replay"""
    name = "g4_tile32"
    c = sc.BY_NAME[name]
    ids = np.random.default_rng(77).integers(0, c.vocab, 1400).tolist()
    llm = _L()(model_path=f"random:{name}", config=c.config(), n_ctx=1536, random_seed=c.seed, init_std=sc.INIT_STD, device=0,
               kv_format="q8_0", kv_shift_requant=True)

    def advance(at):
        if use_frame:
            toks = llm.frame(ids[at:at + 2], ids[at + 2:at + 6], -1)
            assert len(toks) == 4
        else:
            toks = [llm.step(ids[at:at + 2])]
        return toks, llm._scores[-1].copy(), llm.n_tokens

    try:
        runs = []
        for graphs in (True, False):
            llm.reset()
            llm.set_graphs(graphs)
            llm.init_sampler_for_generate(**SAMPLER)
            out = []
            llm.eval(ids[:800])
            out.append(advance(800))
            llm.n_tokens = 800
            llm.eval(ids[800:1100])
            out.append(advance(1100))
            n = llm.n_tokens
            llm.kv_remove(30, 330)
            assert llm.n_tokens == n - 300 < 1024 - 8
            out.append(advance(1200))
            out.append(advance(1210))
            runs.append(out)
        for (ta, la, na), (tb, lb, nb) in zip(*runs):
            assert ta == tb and na == nb and np.array_equal(la, lb)
    finally:
        llm.close()


def test_remove_on_a_q8_twin_leaves_the_parent_alone():
    name, n = "g1_fallback", 300
    parent = _parent(name)
    parent.reset()
    _plant(parent, name, n)
    before = _read_q8(parent, n)
    twin = parent.make_kv_shadow(low_priority=False)
    try:
        assert twin.kv_format == "q8_0" and twin.kv_shift_requant, "make_kv_shadow inherits the switch"
        twin.copy_kv_from(parent, n)
        twin.n_tokens = n
        twin.kv_remove(10, 60)
        assert twin.n_tokens == n - 50 and parent.n_tokens == n
        own = _twins(name, 1)[0]
        _plant(own, name, n)
        own.kv_remove(10, 60)
        assert _same_blocks(_read_q8(twin, n - 50), _read_q8(own, n - 50)), "the twin's shift is not the shift of a handle of its own (the owner's RoPE tables)"
        assert _same_blocks(_read_q8(parent, n), before)
    finally:
        twin.close()
        parent.reset()


# ------------------------------------------------------------------ 6. refusals and inheritance
def test_refusals_and_inheritance_of_the_switch():
    from realtime_codec_agent_amd import _native as native
    from realtime_codec_agent_amd.llm import kv_remove_many
    E = _err()
    name, n = "g4_tile32", 300
    a, b = _twins(name, 2)
    f, = _twins(name, 1, "f16")
    for m in (a, b):
        _plant(m, name, n)
    _plant(f, name, n, deq=True)
    # the flag off: both calls refuse as before, nothing changed
    a.set_kv_shift_requant(False)
    try:
        assert a.kv_shift_requant is False and b.kv_shift_requant is True
        before = [_read_q8(m, n) for m in (a, b)]
        f_before = [tuple(_bits(x).copy() for x in f.kv_read(l, 0, n)) for l in range(2)]
        with pytest.raises(E, match=r"rc=-3.*q8_0.*does not do"):
            a.kv_remove(3, 9)
        with pytest.raises(E, match=r"rc=-3.*handle 1 keeps a q8_0"):
            kv_remove_many([b, a], [(3, 9), (3, 9)])
        # an fp16 handle has no such switch, and cannot share a call with a q8_0 one
        with pytest.raises(E, match=r"rc=-3"):
            f.set_kv_shift_requant(True)
        with pytest.raises(E, match=r"rc=-1"):
            native.check(a._lib.rca_lm_set_kv_shift_requant(a._h, 2), "rca_lm_set_kv_shift_requant")
        for llms in ([f, b], [b, f]):
            with pytest.raises(E, match=r"rc=-1.*handle 1 has KV format"):
                kv_remove_many(llms, [(3, 9), (3, 9)])
        assert all(m.n_tokens == n for m in (a, b, f))
        assert all(_same_blocks(_read_q8(m, n), rows) for m, rows in zip((a, b), before))
        assert all(np.array_equal(_bits(x), y) for l in range(2) for x, y in zip(f.kv_read(l, 0, n), f_before[l]))
    finally:
        a.set_kv_shift_requant(True)
    # a shared twin of a handle with the flag carries it; one of a handle without does not
    a.set_kv_shift_requant(False)
    try:
        t = _L()(model_path=a.model_path, n_ctx=a._n_ctx, share_weights_with=a, device=0)
        assert t.kv_format == "q8_0" and t.kv_shift_requant is False
        t.close()
    finally:
        a.set_kv_shift_requant(True)
    t = _L()(model_path=a.model_path, n_ctx=a._n_ctx, share_weights_with=a, device=0)
    try:
        assert t.kv_shift_requant is True
        # set_kv_format("f16") on the emptied handle clears it; back on q8_0 the handle refuses the shift again
        t.reset()
        t.set_kv_format("f16")
        assert t.kv_format == "f16" and t.kv_shift_requant is False
        t.set_kv_format("q8_0")
        assert t.kv_shift_requant is False
        t.eval(sc.BY_NAME[name].ids().tolist()[:40])
        with pytest.raises(E, match="q8_0"):
            t.kv_remove(3, 9)
        assert t.n_tokens == 40
    finally:
        t.close()
    with pytest.raises(ValueError, match="kv_shift_requant"):
        _L()(model_path="random:x", config=sc.BY_NAME[name].config(), device=0, kv_shift_requant=True)


# ------------------------------------------------------------------ 7. the agent
def _paired_resources(seed=3):
    """the set-up of tests/test_kv_shift_gpu.py::_paired_resources with a q8_0 cache that may shift on both sides"""
    from types import SimpleNamespace
    from agent_fakes import OracleCodecModel
    from oracle import lm_ref
    from oracle.codec import OracleCodec
    from realtime_codec_agent_amd.audio_tokenizer import AudioTokenizer
    from realtime_codec_agent_amd.codec import MagiCodecHIP
    from realtime_codec_agent_amd.codec_model import init_codec_weights, tiny_codec_config
    from realtime_codec_agent_amd.llm import LMConfig
    from realtime_codec_agent_amd.tokenizer import CodecTokenizer
    ccfg = tiny_codec_config()
    cw = init_codec_weights(ccfg, seed=0)
    tok = CodecTokenizer(base_vocab_size=512, codebook_size=ccfg.codebook_size)
    lcfg = LMConfig(vocab_size=tok.vocab_size, hidden=256, n_layers=2, n_heads=4, n_kv_heads=2, head_dim=64, ffn=512)
    w = lm_ref.random_weights(lcfg, seed, 0.05)
    head = w["lm_head.weight"].copy()
    head[: tok.codec_vocab_start] = 0
    head[len(tok):] = 0
    w["lm_head.weight"] = head
    hip = SimpleNamespace(llm=_L()(config=lcfg, weights=w, n_ctx=2048, device=0, kv_format="q8_0", kv_shift_requant=True), aux_llm=None, tokenizer=tok,
                          audio_tokenizer=AudioTokenizer(codec_model=MagiCodecHIP(ccfg, cw)), whisper_model=None, llm_model_dir="")
    ora = SimpleNamespace(llm=qs.Q8ShiftOracleLLM(lcfg, w, n_ctx=2048), aux_llm=None, tokenizer=tok,
                          audio_tokenizer=AudioTokenizer(codec_model=OracleCodecModel(OracleCodec(ccfg, cw)), device="cpu"),
                          whisper_model=None, llm_model_dir="")
    return hip, ora


@pytest.mark.parametrize("exact_prefill", [True, False])
def test_shift_mode_session_over_q8_hip_objects_equals_the_session_over_oracle_objects(exact_prefill):
    """the session of test_kv_shift_gpu.py::test_shift_mode_session_over_hip_objects_equals_shift_mode_session_over_oracle_objects over a
    q8_0 cache: ids equal, PCM bit for bit, same KV position, no twin; last-step logits inside that test's bounds (2e-4 exact, 6e-4
    tiles) widened by 4 x the spread of tests/kv_q8_shift_spread.py for the route, in units of max(1, |logit|max)"""
    from realtime_codec_agent_amd.realtime_agent_config import RealtimeAgentConfig
    from realtime_codec_agent_amd.realtime_agent_v2 import RealtimeAgent
    hip, ora = _paired_resources()
    try:
        hip.llm.set_mfma_prefill(not exact_prefill)
        cfg = dict(chunk_size_secs=0.08, use_whisper=False, force_trans_after_inactivity_secs=0.0, force_response_after_inactivity_secs=0.0,
                   temperature=0.0, max_context_secs=1.0, trim_by_secs=0.4)
        removes = []
        hip_remove = hip.llm.kv_remove
        hip.llm.kv_remove = lambda p0, p1: (removes.append((p0, p1)), hip_remove(p0, p1))[1]
        a_hip = RealtimeAgent(resources=hip, config=RealtimeAgentConfig(**cfg), kv_trim_mode="shift")
        a_ora = RealtimeAgent(resources=ora, config=RealtimeAgentConfig(**cfg), kv_trim_mode="shift")
        n = 1280
        sig = rich_signal(n * 36, 21)
        for s in range(0, len(sig), n):
            o_hip = a_hip.process_audio(sig[s:s + n])
            o_ora = a_ora.process_audio(sig[s:s + n])
            assert a_hip.input_ids == a_ora.input_ids, f"token streams diverge in chunk {s // n}"
            assert np.array_equal(o_hip, o_ora), f"emitted PCM differs in chunk {s // n}"
            assert hip.llm.n_tokens == ora.llm.n_tokens
        assert a_hip.trim_to_secs == a_ora.trim_to_secs and a_hip.trim_to_secs >= 0.8
        assert len(removes) == round(a_hip.trim_to_secs / 0.4) and all(p1 > p0 for p0, p1 in removes)
        assert a_hip._kv_shadow is None and not a_hip.kv_shadow_active
        want = ora.llm._logits
        d = float(np.abs(hip.llm._scores[-1] - want).max())
        route = "gemv" if exact_prefill else "tile32"
        bound = (2e-4 if exact_prefill else 6e-4) + 4.0 * qsp.SPREAD[route] * max(1.0, float(np.abs(want).max()))
        print(f"KVQ8SHIFT session: {len(removes)} removes {removes}, last-step logits HIP vs oracle max|d| = {d:.2e}, bound {bound:.2e}")
        assert d < bound
    finally:
        hip.llm.close()


def _drive(flag, n=4, ticks=30, chunk=1280):
    """the driver sessions of tests/test_kv_shift_many_gpu.py over q8_0 handles: one trim, at tick 27, of all sessions together"""
    from realtime_codec_agent_amd import RealtimeAgentBatch
    from realtime_codec_agent_amd.llm import LMConfig
    from realtime_codec_agent_amd.realtime_agent_config import RealtimeAgentConfig
    from realtime_codec_agent_amd.realtime_agent_resources import RealtimeAgentResources
    from realtime_codec_agent_amd.realtime_agent_v2 import RealtimeAgent
    lm = LMConfig(vocab_size=259344, hidden=256, n_layers=2, n_heads=4, n_kv_heads=2, head_dim=64, ffn=512)
    res = [RealtimeAgentResources(llm_model_path="random:small", llm_n_ctx=4096, llm_config=lm, with_aux_llm=False, llm_random_seed=3,
                                  llm_kv_format="q8_0", llm_kv_shift_requant=True)]
    res += [res[0].clone_for_self_play() for _ in range(n - 1)]
    assert all(r.llm.kv_format == "q8_0" and r.llm.kv_shift_requant for r in res), "clone_for_self_play carries format and switch"
    at = res[0].audio_tokenizer
    per_chunk, per_sec = 2 * int(0.08 * at.framerate), at.framerate * 2
    cfg = RealtimeAgentConfig(chunk_size_secs=0.08, use_whisper=False, force_trans_after_inactivity_secs=0.0,
                              force_response_after_inactivity_secs=0.0, max_context_secs=(27 * per_chunk - 1) / per_sec,
                              trim_by_secs=4 * per_chunk / per_sec)
    agents = [RealtimeAgent(resources=r, config=cfg, kv_trim_mode="shift") for r in res]
    drv = RealtimeAgentBatch(agents, min_batch=1, batch_shift_trims=flag)
    sig = [rich_signal(chunk * ticks, 60 + s) for s in range(n)]
    outs = [drv.process_audio([sig[s][t * chunk:(t + 1) * chunk] for s in range(n)]) for t in range(ticks)]
    state = [(list(a.input_ids), a.resources.llm.n_tokens, _read_q8(a.resources.llm, a.resources.llm.n_tokens), a.trim_to_secs) for a in agents]
    counters = (drv.fused_shift_calls, drv.fused_shift_trims)
    drv.close()
    for r in res[1:] + res[:1]:
        r.llm.close()
    return outs, state, counters


def test_the_driver_fuses_the_q8_shift_trims_of_four_sessions():
    on, s_on, c_on = _drive(True)
    off, s_off, c_off = _drive(False)
    assert c_on == (1, 4) and c_off == (0, 0), (c_on, c_off)
    for t, (x, y) in enumerate(zip(on, off)):
        for s in range(4):
            assert np.array_equal(x[s], y[s]), ("PCM of agent", s, "tick", t)
    for s, (a, b) in enumerate(zip(s_on, s_off)):
        assert a[0] == b[0], ("input_ids of agent", s)
        assert a[1] == b[1] and a[3] == b[3] and a[3] > 0, ("n_tokens / trim_to_secs of agent", s)
        assert _same_blocks(a[2], b[2]), ("final cache of agent", s)
