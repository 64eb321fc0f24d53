"""rca_lm_batch_eval without a GPU: the header declares the call and the ctypes prototype follows it argument for argument; the two
halves KVShadow.advance was split into (next_tile: which tile is due, commit_tile: it was fed) are, step for step, what advance did;
RealtimeAgentBatch(batch_shadow_tiles=True) over LM objects without the call keeps every session's own advance.

Every test here fails on a tree without the call: the symbol, LlamaBatchEval, the flag and the two KVShadow methods do not exist."""
import ctypes as C
import os
import re

import numpy as np

from agent_fakes import FakeLLM, build_fakes, user_audio

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "rca.h")
CTYPES = {"rca_lm_t*": C.c_void_p, "rca_lm_t*const*": C.POINTER(C.c_void_p), "int32_t": C.c_int32, "int32_t*": C.POINTER(C.c_int32)}


def _declared_args(sym):
    """[(name, ctype)] of `int <sym>(...)` in rca.h"""
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    args = re.search(r"\bint %s\((.*?)\);" % sym, text, re.S).group(1)
    out = []
    for a in args.split(","):
        m = re.match(r"\s*(?:const\s+)?(\w+)\s*((?:\*\s*(?:const\s*)?)*)(\w+)\s*$", a)
        out.append((m.group(3), CTYPES[m.group(1) + re.sub(r"\s+", "", m.group(2))]))
    return out


def test_the_header_declares_the_call_and_the_prototype_follows_it():
    from realtime_codec_agent_amd import _native as N
    want = _declared_args("rca_lm_batch_eval")
    assert [n for n, _ in want] == ["ws", "hs", "n_h", "ids", "counts", "want_logits"]
    assert len(N.BATCH_EVAL_ARGTYPES) == len(want)
    for (name, t), got in zip(want, N.BATCH_EVAL_ARGTYPES):
        assert got is t, (name, got, t)
    assert "rca_lm_batch_eval" in N.ABI_SYMBOLS


def test_the_entry_point_is_bound_and_exported_and_refuses_null_arguments_before_any_hip_call():
    from realtime_codec_agent_amd import _native as N
    if N.needs_build():
        N.build()
    lib = N.lib()
    assert hasattr(lib, "rca_lm_batch_eval")
    assert list(lib.rca_lm_batch_eval.argtypes) == N.BATCH_EVAL_ARGTYPES and lib.rca_lm_batch_eval.restype is C.c_int
    assert lib.rca_lm_batch_eval(None, None, 1, None, None, 0) == -1 and b"batch_eval: null argument" in lib.rca_last_error()


def test_the_python_surface():
    import inspect
    import realtime_codec_agent_amd as pkg
    from realtime_codec_agent_amd.llm import LlamaBatchEval
    assert pkg.LlamaBatchEval is LlamaBatchEval and "LlamaBatchEval" in pkg.__all__
    p = inspect.signature(LlamaBatchEval.__init__).parameters
    assert list(p)[1:] == ["llm", "low_priority"] and p["low_priority"].default is True
    p = inspect.signature(LlamaBatchEval.eval_async).parameters
    assert list(p)[1:] == ["handles", "token_lists", "want_logits"] and p["want_logits"].default is False
    for name in ("eval", "sync", "close", "supported"):
        assert callable(getattr(LlamaBatchEval, name))
    assert LlamaBatchEval.supported(FakeLLM(600, 512, 64)) is False     # an LM object without a native handle


# ---------------------------------------------------------------------------------------------- KVShadow
class _ShadowLLM(FakeLLM):
    """FakeLLM with the shadow-cache surface: the twin records what it is fed"""

    def make_kv_shadow(self):
        twin = _ShadowLLM(self._n_vocab, self.codec_start, self.n_codec)
        twin.fed_calls = []
        return twin

    def set_mfma_prefill(self, enable):
        pass

    def copy_kv_from(self, other, n):
        self.kv = list(other.kv[:n])

    def eval_async(self, tokens):
        self.fed_calls.append(list(tokens))
        self.eval(tokens)

    def swap_kv(self, other):
        self.kv, other.kv = other.kv, self.kv


def _old_advance(sh, input_ids, max_tiles=1):
    """KVShadow.advance as it was before the split, restated"""
    if not sh.planned:
        return
    for _ in range(max_tiles):
        a = sh.src_pos + len(sh.fed)
        avail = len(input_ids) - sh.keep_back - a
        if avail < sh.tile:
            return
        chunk = input_ids[a:a + sh.tile]
        sh.twin.eval_async(chunk)
        sh.fed.extend(chunk)
        sh.stats["tiles"] += 1


def _shadow(tile, keep_back):
    from realtime_codec_agent_amd.kv_shadow import KVShadow
    llm = _ShadowLLM(600, 512, 64)
    return KVShadow(llm, tile=tile, keep_back=keep_back)


def test_next_tile_and_commit_tile_are_step_for_step_what_advance_did():
    rng = np.random.default_rng(5)
    seq = rng.integers(0, 600, 400).tolist()
    for tile, keep_back, src in ((8, 3, 5), (16, 16, 0), (128, 16, 40), (7, 0, 11)):
        old, new, split = _shadow(tile, keep_back), _shadow(tile, keep_back), _shadow(tile, keep_back)
        for sh in (old, new, split):
            assert sh.next_tile(seq) is None            # not planned: nothing is due
            sh.llm.eval(seq[:4])
        _old_advance(old, seq)
        new.advance(seq)
        assert old.twin.fed_calls == new.twin.fed_calls == []
        for sh in (old, new, split):
            sh.plan(4, src)
        for n in range(src, len(seq) + 1, 5):          # the sequence grows by five tokens per frame
            ids = seq[:n]
            _old_advance(old, ids)
            new.advance(ids)
            chunk = split.next_tile(ids)
            assert split.next_tile(ids) == chunk        # asking changes nothing
            if chunk is not None:
                split.twin.eval_async(chunk)
                split.commit_tile(chunk)
            for sh in (new, split):
                assert sh.fed == old.fed and sh.stats == old.stats and sh.twin.fed_calls == old.twin.fed_calls, (tile, keep_back, src, n)
                assert sh.twin.n_tokens == old.twin.n_tokens
        assert old.stats["tiles"] >= 2
        _old_advance(old, seq, max_tiles=3)
        new.advance(seq, max_tiles=3)
        assert new.fed == old.fed and new.stats == old.stats and new.twin.fed_calls == old.twin.fed_calls
        for sh in (old, new, split):                    # finish() is unchanged: the swap stands on what was fed
            assert sh.finish(seq, src, 4, len(seq) - 2) is True
        assert new.llm.kv == old.llm.kv and new.stats == old.stats


# ---------------------------------------------------------------------------------------------- the driver's fallback
def _agents(n, shadow_llm):
    from realtime_codec_agent_amd.realtime_agent_config import RealtimeAgentConfig
    from realtime_codec_agent_amd.realtime_agent_v2 import RealtimeAgent
    out = []
    for _ in range(n):
        res, tok = build_fakes()
        if shadow_llm:
            res.llm = _ShadowLLM(res.llm._n_vocab, res.llm.codec_start, res.llm.n_codec)
        a = RealtimeAgent(resources=res, config=RealtimeAgentConfig(chunk_size_secs=0.1, use_whisper=False, force_trans_after_inactivity_secs=0.0,
                                                                    force_response_after_inactivity_secs=0.0, max_context_secs=1.0, trim_by_secs=0.4))
        a.kv_shadow_tile = 8
        out.append(a)
    return out


def test_over_lms_without_the_call_the_flag_keeps_every_sessions_own_advance():
    from realtime_codec_agent_amd import RealtimeAgentBatch
    n, ticks = 3, 24
    plain, flagged = _agents(n, True), _agents(n, True)
    off = RealtimeAgentBatch(plain, min_batch=1)
    on = RealtimeAgentBatch(flagged, min_batch=1, batch_shadow_tiles=True)
    assert off.batch_shadow_tiles is False and on.batch_shadow_tiles is True
    assert on._shadow_pool is None and on._batch is None
    assert (on.fused_shadow_calls, on.fused_shadow_tiles) == (0, 0) == (off.fused_shadow_calls, off.fused_shadow_tiles)
    size = plain[0].chunk_size_samples
    sigs = [user_audio(size * ticks, seed=3 + s) for s in range(n)]
    for t in range(ticks):
        row = [sigs[s][t * size:(t + 1) * size] for s in range(n)]
        a, b = off.process_audio(row), on.process_audio(row)
        for s in range(n):
            assert np.array_equal(a[s], b[s]), (t, s)
        # the end of a tick as the driver runs it for its fused members: without a pool, the sessions' own advance
        off._advance_shadows(list(range(n)))
        on._advance_shadows(list(range(n)))
    for a, b in zip(plain, flagged):
        assert a.input_ids == b.input_ids and a.resources.llm.n_tokens == b.resources.llm.n_tokens
        assert a._kv_shadow is not None and b._kv_shadow is not None
        assert a._kv_shadow.stats == b._kv_shadow.stats and b._kv_shadow.stats["tiles"] > 0 and b._kv_shadow.stats["swaps"] > 0
    assert (on.fused_shadow_calls, on.fused_shadow_tiles) == (0, 0)
    on.close()
    off.close()
