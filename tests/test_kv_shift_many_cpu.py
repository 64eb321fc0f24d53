"""rca_lm_kv_remove_many without a GPU: the header declares the call, the library exports it and the ctypes prototype follows the
declaration; and the driver logic of RealtimeAgentBatch(batch_shift_trims=...) over ShiftOracleLLM fakes (tests/kv_shift_ref.py) with a
recording kv_remove_many that applies kv_remove_ref per handle, in the pattern of tests/test_agent_batch_speaker_cpu.py: a fake batch
whose frame() runs the members' own LMs, and an agent is ready whenever its frame could run as one replay.

With the flag on a trim tick makes exactly one kv_remove_many, holding exactly the due agents' spans, before any LM call of the tick; one
due trim takes the single call; with the flag off the call is never made; a trim that falls between two steps is not deferred; the
sessions are the same in every case.  Fails on a tree without the call: the symbol, the Python call and the flag do not exist."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from agent_fakes import OracleCodecModel, user_audio
from kv_shift_ref import ShiftOracleLLM, kv_remove_ref

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "rca.h")
CTYPES = {"rca_lm_t*const*": C.POINTER(C.c_void_p), "int32_t": C.c_int32, "int32_t*": C.POINTER(C.c_int32)}
SYMBOLS = ("rca_lm_kv_remove_many", "rca_lm_kv_remove_many_staged")


def _declared_args(sym):
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    args = re.search(r"\bint %s\((.*?)\);" % sym, text, re.S).group(1)
    out = []
    for a in args.split(","):
        m = re.match(r"\s*(?:const\s+)?(\w+)\s*((?:\*\s*(?:const\s*)?)*)(\w+)\s*$", a)
        out.append((m.group(3), CTYPES[m.group(1) + re.sub(r"\s+", "", m.group(2))]))
    return out


@pytest.mark.parametrize("sym", SYMBOLS)
def test_the_header_declares_the_call_and_the_prototype_follows_it(sym):
    from realtime_codec_agent_amd import _native as N
    want = _declared_args(sym)
    assert [n for n, _ in want] == ["hs", "n_h", "p0", "p1"]
    assert len(N.KV_REMOVE_MANY_ARGTYPES) == len(want)
    for (name, t), got in zip(want, N.KV_REMOVE_MANY_ARGTYPES):
        assert got is t, (name, got, t)
    assert sym in N.ABI_SYMBOLS
    group = int(re.search(r"#define RCA_LM_KV_REMOVE_GROUP (\d+)", open(HEADER).read()).group(1))
    assert 1 <= group <= 64                      # the staging bound is stated where the call is declared


@pytest.mark.parametrize("sym", SYMBOLS)
def test_the_entry_point_is_bound_and_exported_and_refuses_bad_counts_before_any_hip_call(sym):
    from realtime_codec_agent_amd import _native as N
    if N.needs_build():
        N.build()
    lib = N.lib()
    assert hasattr(lib, sym)
    fn = getattr(lib, sym)
    assert list(fn.argtypes) == N.KV_REMOVE_MANY_ARGTYPES and fn.restype is C.c_int
    assert fn(None, 1, None, None) == -1 and b"kv_remove_many: null argument" in lib.rca_last_error()
    hs, p = (C.c_void_p * 65)(), (C.c_int32 * 65)()
    for n in (0, 65, -3):
        assert fn(hs, n, p, p) == -1 and b"(1 to 64)" in lib.rca_last_error()
    assert fn(hs, 2, p, p) == -1 and b"handle 0 is null" in lib.rca_last_error()


def test_the_python_surface():
    import inspect
    import realtime_codec_agent_amd as pkg
    from realtime_codec_agent_amd import llm as L
    from realtime_codec_agent_amd.realtime_agent_batch import RealtimeAgentBatch
    assert pkg.kv_remove_many is L.kv_remove_many and "kv_remove_many" in pkg.__all__
    assert list(inspect.signature(L.kv_remove_many).parameters)[:2] == ["llms", "spans"]
    assert callable(L.LlamaForAlternatingCodeChannels.kv_remove_many)
    assert list(inspect.signature(L.LlamaBatch.kv_remove).parameters)[1:] == ["members", "spans"]
    assert inspect.signature(RealtimeAgentBatch.__init__).parameters["batch_shift_trims"].default is False
    with pytest.raises(ValueError, match="2 spans for 1 handles"):
        L.kv_remove_many([object()], [(0, 1), (0, 1)])


# ---------------------------------------------------------------------------------------------- the driver
class ManyLLM(ShiftOracleLLM):
    """ShiftOracleLLM that records every call that touches the cache, and offers kv_remove_many: kv_remove_ref per handle"""
    events = None            # one list per driver, shared by its sessions

    def eval(self, tokens):
        self.events.append(("eval", self.idx))
        super().eval(tokens)

    def kv_remove(self, p0, p1):
        self.events.append(("single", self.idx, int(p0), int(p1)))
        super().kv_remove(p0, p1)

    @staticmethod
    def kv_remove_many(llms, spans):
        llms[0].events.append(("many", [m.idx for m in llms], [(int(a), int(b)) for a, b in spans]))
        for m, (a, b) in zip(llms, spans):
            kv_remove_ref(m.ref, int(a), int(b))


class SingleOnlyLLM(ShiftOracleLLM):
    """an LM object without kv_remove_many (a llama.cpp object): the driver keeps the per-session call"""
    events = None

    def eval(self, tokens):
        self.events.append(("eval", self.idx))
        super().eval(tokens)

    def kv_remove(self, p0, p1):
        self.events.append(("single", self.idx, int(p0), int(p1)))
        super().kv_remove(p0, p1)


def _softmax(x):
    e = np.exp(x.astype(np.float64) - x.max())
    return e / e.sum()


class FakeBatch:
    """LlamaBatch.frame(members=) over the members' own LMs, one member after the other"""

    def __init__(self, llms, events):
        self.members, self.events = llms, events

    def frame(self, first_pairs, user_ids, audio_id_floor, probe_ids=None, members=None):
        self.events.append(("frame", list(members)))
        toks, probs = [], []
        for k, s in enumerate(members):
            llm, pair, out = self.members[s], list(first_pairs[k]), []
            for u in user_ids[k]:
                llm.eval(pair)
                out.append(llm.sample())
                pair = [out[-1], u]
            toks.append(out)
            probs.append(_softmax(llm._logits)[probe_ids[k]])
        return toks, np.array(probs, np.float32)

    def close(self):
        pass


@pytest.fixture(scope="module")
def parts():
    """codec, tokenizer and LM weights shared by every session of this module (each session gets its own LM object and codec windows)"""
    from oracle import lm_ref
    from oracle.codec import OracleCodec
    from realtime_codec_agent_amd.codec_model import init_codec_weights, tiny_codec_config
    from realtime_codec_agent_amd.llm import LMConfig
    from realtime_codec_agent_amd.tokenizer import CodecTokenizer
    ccfg = tiny_codec_config()
    cw = init_codec_weights(ccfg, seed=0)
    tok = CodecTokenizer(base_vocab_size=512, codebook_size=ccfg.codebook_size)
    lcfg = LMConfig(vocab_size=tok.vocab_size, hidden=128, n_layers=2, n_heads=2, n_kv_heads=1, head_dim=64, ffn=256)
    w = lm_ref.random_weights(lcfg, 3, 0.05)
    head = w["lm_head.weight"].copy()
    head[: tok.codec_vocab_start] = 0          # audio mode throughout: the text rows never win
    head[len(tok):] = 0
    w["lm_head.weight"] = head
    return ccfg, cw, tok, lcfg, w, OracleCodec


def _driver(parts, n, flag, llm_cls=ManyLLM, mid_chunk=False):
    """n sessions in shift mode under a driver whose batch is a FakeBatch.  The context limit sits one frame below a chunk boundary, so
    a trim falls due before the first step of a frame; mid_chunk puts it one step further, between the first two steps."""
    from types import SimpleNamespace
    from realtime_codec_agent_amd import RealtimeAgentBatch
    from realtime_codec_agent_amd.audio_tokenizer import AudioTokenizer
    from realtime_codec_agent_amd.realtime_agent_config import RealtimeAgentConfig
    from realtime_codec_agent_amd.realtime_agent_v2 import RealtimeAgent
    from test_agent_batch_cpu import _plan
    ccfg, cw, tok, lcfg, w, OracleCodec = parts
    events = []
    agents = []
    for i in range(n):
        llm = llm_cls(lcfg, w, n_ctx=2048)
        llm.idx, llm.events = i, events
        at = AudioTokenizer(codec_model=OracleCodecModel(OracleCodec(ccfg, cw)), device="cpu")
        res = SimpleNamespace(llm=llm, aux_llm=None, tokenizer=tok, audio_tokenizer=at, whisper_model=None, llm_model_dir="")
        per_chunk = 2 * int(0.08 * at.framerate)
        per_sec = at.framerate * 2
        cfg = RealtimeAgentConfig(chunk_size_secs=0.08, use_whisper=False, force_trans_after_inactivity_secs=0.0,
                                  force_response_after_inactivity_secs=0.0, temperature=0.0,
                                  max_context_secs=(6 * per_chunk + (2 if mid_chunk else 0) - 1) / per_sec, trim_by_secs=2 * per_chunk / per_sec)
        agents.append(RealtimeAgent(resources=res, config=cfg, kv_trim_mode="shift"))
    kw = {} if flag is None else dict(batch_shift_trims=flag)
    drv = RealtimeAgentBatch(agents, min_batch=1, use_duplex_batch_graph=False, **kw)
    assert drv._batch is None
    drv._batch = FakeBatch([a.resources.llm for a in agents], events)
    for a in agents:
        nf = a.chunk_size_frames_per_channel
        a._replay_plan = lambda chunk, a=a, nf=nf: _plan(n=nf) if a._frame_ready(nf, False) else None
    return drv, agents, events


def _run(parts, n, flag, ticks=14, late=0, **kw):
    """`late`: session s joins s * late ticks after session 0"""
    drv, agents, events = _driver(parts, n, flag, **kw)
    size = agents[0].chunk_size_samples
    sigs = [user_audio(size * ticks, seed=3 + s) for s in range(n)]
    per_tick = []
    for t in range(ticks):
        del events[:]
        was = [a.trim_to_secs for a in agents]
        row = [None if t < late * s else sigs[s][(t - late * s) * size:(t - late * s + 1) * size] for s in range(n)]
        outs = drv.process_audio(row)
        per_tick.append(dict(events=list(events), outs=outs, trimmed=[i for i, a in enumerate(agents) if a.trim_to_secs != was[i]]))
    return drv, agents, per_tick


def _same_sessions(x, y):
    for a, b in zip(x[1], y[1]):
        assert a.input_ids == b.input_ids and a.resources.llm.n_tokens == b.resources.llm.n_tokens and a.trim_to_secs == b.trim_to_secs
        for l in range(2):
            assert np.array_equal(a.resources.llm.ref.k[l].numpy(), b.resources.llm.ref.k[l].numpy())
            assert np.array_equal(a.resources.llm.ref.v[l].numpy(), b.resources.llm.ref.v[l].numpy())
    for ta, tb in zip(x[2], y[2]):
        assert ta["trimmed"] == tb["trimmed"]
        for p, q in zip(ta["outs"], tb["outs"]):
            assert (p is None and q is None) or np.array_equal(p, q)


def test_flag_on_one_call_per_trim_tick_before_any_lm_call_and_the_sessions_are_those_of_the_flag_off(parts):
    n = 3
    on, off, default = _run(parts, n, True), _run(parts, n, False), _run(parts, n, None)
    trim_ticks = 0
    for tk, tk_off in zip(on[2], off[2]):
        kinds = [e[0] for e in tk["events"]]
        if not tk["trimmed"]:
            assert "many" not in kinds and "single" not in kinds
            continue
        trim_ticks += 1
        assert tk["trimmed"] == list(range(n))                         # sessions that start together trim together
        assert kinds.count("many") == 1 and "single" not in kinds and kinds[0] == "many", kinds
        _, members, spans = tk["events"][0]
        assert members == list(range(n))
        # exactly the spans the sessions issue on their own with the flag off, in agent order
        singles = [e for e in tk_off["events"] if e[0] == "single"]
        assert [e[1] for e in singles] == members and [(e[2], e[3]) for e in singles] == spans and all(b > a for a, b in spans)
    assert trim_ticks >= 3
    assert (on[0].fused_shift_calls, on[0].fused_shift_trims) == (trim_ticks, n * trim_ticks)
    for drv, _, ticks in (off, default):
        assert drv.batch_shift_trims is False and (drv.fused_shift_calls, drv.fused_shift_trims) == (0, 0)
        assert all(e[0] != "many" for tk in ticks for e in tk["events"])
    assert all(a._shift_sink is None for a in on[1])
    _same_sessions(on, off)
    _same_sessions(on, default)


def test_one_due_trim_takes_the_single_call(parts):
    """session 1 joins a tick late: the two sessions' trims never fall due on the same tick"""
    on, off = _run(parts, 2, True, late=1), _run(parts, 2, False, late=1)
    trims = 0
    for tk in on[2]:
        kinds = [e[0] for e in tk["events"]]
        assert "many" not in kinds and len(tk["trimmed"]) <= 1
        if tk["trimmed"]:
            trims += 1
            assert kinds.count("single") == 1 and kinds[0] == "single" and tk["events"][0][1] == tk["trimmed"][0]
    assert trims >= 4 and (on[0].fused_shift_calls, on[0].fused_shift_trims) == (0, 0)
    _same_sessions(on, off)


def test_lm_objects_without_the_call_keep_the_per_session_call(parts):
    on, off = _run(parts, 3, True, llm_cls=SingleOnlyLLM), _run(parts, 3, False, llm_cls=SingleOnlyLLM)
    trims = 0
    for tk in on[2]:
        if tk["trimmed"]:
            trims += 1
            assert [e[0] for e in tk["events"]][:3] == ["single"] * 3 and [e[1] for e in tk["events"][:3]] == [0, 1, 2]
    assert trims >= 3 and (on[0].fused_shift_calls, on[0].fused_shift_trims) == (0, 0)
    _same_sessions(on, off)


def test_a_trim_between_two_steps_is_not_deferred(parts):
    on, off = _run(parts, 3, True, mid_chunk=True), _run(parts, 3, False, mid_chunk=True)
    trims = 0
    for tk in on[2]:
        kinds = [e[0] for e in tk["events"]]
        assert "many" not in kinds
        if tk["trimmed"]:
            trims += 1
            assert tk["trimmed"] == [0, 1, 2] and kinds.count("single") == 3 and "frame" not in kinds
            for i in range(3):       # each session's own call, after the step in front of it
                mine = [e for e in tk["events"] if e[1] == i]
                assert [e[0] for e in mine].index("single") >= 1
    assert trims >= 3 and (on[0].fused_shift_calls, on[0].fused_shift_trims) == (0, 0)
    _same_sessions(on, off)
