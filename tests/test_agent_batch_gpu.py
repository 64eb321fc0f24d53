"""RealtimeAgentBatch on the GPU: five RealtimeAgents over weight-sharing LM handles and one codec handle, driven tick by tick.
The run with use_duplex_batch_graph=True (ONE rca_duplex_batch_frame per tick for the ready agents) equals the run with False (the
separate codec calls around one selection frame) on a second set of agents: tokens, PCM, sequences, positions, event probabilities.
Agent s joins 7 s ticks late, agent 2 pauses for three ticks, and the sessions trim through their shadow caches on the way."""
import numpy as np
import pytest

from conftest import rich_signal

pytestmark = pytest.mark.gpu

N_AGENTS, TICKS, CHUNK = 5, 48, 1280


def _make(n=N_AGENTS):
    from realtime_codec_agent_amd.llm import LMConfig
    from realtime_codec_agent_amd.realtime_agent_config import RealtimeAgentConfig
    from realtime_codec_agent_amd.realtime_agent_resources import RealtimeAgentResources
    from realtime_codec_agent_amd.realtime_agent_v2 import RealtimeAgent
    lm = LMConfig(vocab_size=259344, hidden=256, n_layers=2, n_heads=4, n_kv_heads=2, head_dim=64, ffn=512)
    res = [RealtimeAgentResources(llm_model_path="random:small", llm_n_ctx=4096, llm_config=lm, with_aux_llm=False, llm_random_seed=3)]
    assert res[0].llm.prefill_route() == "gemm128"
    res += [res[0].clone_for_self_play() for _ in range(n - 1)]
    cfg = RealtimeAgentConfig(chunk_size_secs=0.08, use_whisper=False, force_trans_after_inactivity_secs=0.0,
                              force_response_after_inactivity_secs=0.0, max_context_secs=2.0, trim_by_secs=0.8)
    return [RealtimeAgent(resources=r, config=cfg) for r in res], res


def _chunk(s, t):
    return _SIG[s][t * CHUNK:(t + 1) * CHUNK]


_SIG = [rich_signal(CHUNK * TICKS, 30 + s) for s in range(N_AGENTS)]


def _row(t):
    return [None if t < 7 * s or (s == 2 and 34 <= t < 37) else _chunk(s, t - 7 * s) for s in range(N_AGENTS)]


def _drive(fused):
    from realtime_codec_agent_amd import RealtimeAgentBatch
    agents, res = _make()
    drv = RealtimeAgentBatch(agents, min_batch=1, use_duplex_batch_graph=fused)
    outs = []
    for t in range(TICKS):
        row = _row(t)
        before = [(len(a.input_ids), a.resources.llm.n_tokens, len(a.audio_history_ch2)) for a in agents]
        out = drv.process_audio(row)
        for s, c in enumerate(row):
            if c is None:       # an agent without a chunk is not touched
                assert out[s] is None and (len(agents[s].input_ids), agents[s].resources.llm.n_tokens, len(agents[s].audio_history_ch2)) == before[s], (t, s)
            else:
                assert out[s].shape == (CHUNK,) and np.isfinite(out[s]).all()
        outs.append(out)
    state = [(list(a.input_ids), a.resources.llm.n_tokens, np.array(a.stats.event_prob.values, dtype=np.float64).copy(), a.trim_to_secs,
              a._kv_shadow.stats["swaps"] if a._kv_shadow is not None else 0, a.duplex_graph_frames) for a in agents]
    counters = (drv.fused_ticks, drv.fused_frames)
    drv.close()
    return outs, state, counters


def test_the_fused_run_equals_the_unfused_run():
    fused, sf, cf = _drive(True)
    plain, sp, cp = _drive(False)
    assert cf == cp and cf[0] >= 20, (cf, cp)
    assert sf[0][5] >= 20, ("fused frames of the oldest agent", sf[0][5])
    assert any(s[3] > 0 and s[4] > 0 for s in sf), "no session trimmed through its shadow cache"
    for t in range(TICKS):
        for s in range(N_AGENTS):
            if fused[t][s] is None:
                assert plain[t][s] is None
            else:
                assert np.array_equal(fused[t][s], plain[t][s]), ("PCM of agent", s, "tick", t)
    for s, (a, b) in enumerate(zip(sf, sp)):
        assert a[0] == b[0], ("input_ids of agent", s)
        assert a[1] == b[1], ("n_tokens of agent", s)
        assert np.array_equal(a[2], b[2]), ("event probabilities of agent", s)
        assert a[3] == b[3] and a[4] == b[4], ("trims of agent", s)


def test_mismatched_agents_raise_value_error():
    from realtime_codec_agent_amd import RealtimeAgentBatch
    from realtime_codec_agent_amd.realtime_agent_resources import RealtimeAgentResources
    from realtime_codec_agent_amd.realtime_agent_v2 import RealtimeAgent
    agents, res = _make(2)
    lm = res[0].llm.config
    other_codec = RealtimeAgentResources(llm_model_path="random:small", llm_n_ctx=4096, llm_config=lm, with_aux_llm=False, llm_random_seed=3)
    with pytest.raises(ValueError, match="another codec handle"):
        RealtimeAgentBatch([agents[0], RealtimeAgent(resources=other_codec, config=agents[0].config)])
    other_weights = RealtimeAgentResources(llm_model_path="random:small", llm_n_ctx=4096, llm_config=lm, with_aux_llm=False, llm_random_seed=3,
                                           codec_model=res[0].audio_tokenizer.codec_model, tokenizer=res[0].tokenizer)
    with pytest.raises(ValueError, match="cannot form one batch"):
        RealtimeAgentBatch([agents[0], RealtimeAgent(resources=other_weights, config=agents[0].config)])
    RealtimeAgentBatch(agents).close()
