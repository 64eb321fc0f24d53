"""RealtimeAgentBatch on the CPU: over tests/agent_fakes.py objects (no duplex_frame, so every agent falls through to its own
process_audio) it is N independent sessions; the partition of ready and not-ready agents and the min_batch rule on stubbed plans."""
import numpy as np
import pytest

from agent_fakes import build_fakes, user_audio


def _agents(n, **cfg_kw):
    from realtime_codec_agent_amd.realtime_agent_config import RealtimeAgentConfig
    from realtime_codec_agent_amd.realtime_agent_v2 import RealtimeAgent
    kw = dict(chunk_size_secs=0.1, use_whisper=False, force_trans_after_inactivity_secs=0.0, force_response_after_inactivity_secs=0.0)
    kw.update(cfg_kw)
    return [RealtimeAgent(resources=build_fakes()[0], config=RealtimeAgentConfig(**kw)) for _ in range(n)]


def _chunks(n_agents, ticks, size):
    sigs = [user_audio(size * ticks, seed=3 + s) for s in range(n_agents)]
    return [[sigs[s][t * size:(t + 1) * size] for s in range(n_agents)] for t in range(ticks)]


def test_over_fakes_the_batch_is_n_independent_sessions_and_none_chunks_are_honoured():
    from realtime_codec_agent_amd import RealtimeAgentBatch
    n, ticks = 3, 24
    solo, batched = _agents(n, max_context_secs=1.0, trim_by_secs=0.4), _agents(n, max_context_secs=1.0, trim_by_secs=0.4)
    drv = RealtimeAgentBatch(batched, min_batch=1)
    assert drv._batch is None
    rows = _chunks(n, ticks, solo[0].chunk_size_samples)
    for t, row in enumerate(rows):
        row = [None if (s == 1 and 5 <= t < 8) or t < 2 * s else c for s, c in enumerate(row)]      # late joiners, one agent pausing
        before = [(len(a.input_ids), a.resources.llm.n_tokens) for a in batched]
        outs = drv.process_audio(row)
        for s, c in enumerate(row):
            if c is None:
                assert outs[s] is None and (len(batched[s].input_ids), batched[s].resources.llm.n_tokens) == before[s]
            else:
                assert np.array_equal(outs[s], solo[s].process_audio(c)), (t, s)
    for a, b in zip(solo, batched):
        assert a.input_ids == b.input_ids and a.resources.llm.n_tokens == b.resources.llm.n_tokens
        assert np.array_equal(a.stats.event_prob.values, b.stats.event_prob.values)
    assert drv.fused_ticks == 0 and solo[0].trim_to_secs > 0
    with pytest.raises(ValueError, match="3 chunks|2 chunks"):
        drv.process_audio(rows[0][:2])


def _plan(T=32000, F=96, n=4, n_samples=1440):
    return {"window": np.zeros(T, np.float32), "code_ctx": np.zeros(F, np.int64), "n_codes": n, "n_samples": n_samples, "preroll": 160}


def test_the_partition_of_ready_agents_and_the_min_batch_rule():
    from realtime_codec_agent_amd import RealtimeAgentBatch
    drv = RealtimeAgentBatch(_agents(2), min_batch=3)
    a, b = _plan(), _plan(F=48)
    #            0     1  2  3     4  5  6     7
    plans = [None, a, b, a, None, a, b, None]
    groups, rest = drv._partition(plans)
    assert groups == [[1, 3, 5]] and rest == [2, 6]          # three of one shape are a group, two of another run on their own
    drv.min_batch = 2
    groups, rest = drv._partition(plans)
    assert sorted(groups) == [[1, 3, 5], [2, 6]] and rest == []
    drv.min_batch = 4
    assert drv._partition(plans) == ([], [1, 2, 3, 5, 6])
    assert drv._partition([None] * 5) == ([], [])
    drv.min_batch = 1
    assert drv._partition([None, _plan(n_samples=1280)]) == ([[1]], [])
    assert RealtimeAgentBatch(_agents(2), min_batch=0).min_batch == 1


def test_mismatched_agents_are_refused():
    from realtime_codec_agent_amd import RealtimeAgentBatch
    ag = _agents(2)
    with pytest.raises(ValueError, match="at least two"):
        RealtimeAgentBatch(ag[:1])
    with pytest.raises(ValueError, match="LM handle of its own"):
        RealtimeAgentBatch([ag[0], ag[0]])
    ag[1].end_audio_token_id += 1
    with pytest.raises(ValueError, match="agent 1 has another end_audio_token_id"):
        RealtimeAgentBatch(ag)
