"""RealtimeAgentBatch(batch_shadow_tiles=True) on the GPU: the shadow-cache tiles that fall due in one tick go to the sessions' twins
in ONE LlamaBatchEval call (rca_lm_batch_eval) instead of one eval_async per session.  A twin ends with the bits of its own
eval_async, so the run with the flag on equals the run with it off on a second set of agents: output chunks, sequences, positions.

Four sessions of tests/test_agent_batch_gpu.py's kind start together and run in lock step, with a shadow tile of 16 tokens (a session
grows by about 8 tokens per tick), so the same ticks owe a tile in every session; each session trims through its shadow cache on the way.

Fails on a tree without the flag (the parent commit: RealtimeAgentBatch takes no batch_shadow_tiles)."""
import numpy as np
import pytest

import test_agent_batch_gpu as base

pytestmark = pytest.mark.gpu

N_AGENTS, TICKS, TILE = 4, 48, 16


def _drive(flag):
    from realtime_codec_agent_amd import RealtimeAgentBatch
    agents, res = base._make(N_AGENTS)
    for a in agents:
        a.kv_shadow_tile = TILE
    drv = RealtimeAgentBatch(agents, min_batch=1, batch_shadow_tiles=flag)
    assert (drv._shadow_pool is not None) == flag
    outs = []
    for t in range(TICKS):
        row = [base._chunk(s, t) for s in range(N_AGENTS)]
        out = drv.process_audio(row)
        for o in out:
            assert o.shape == (base.CHUNK,) and np.isfinite(o).all()
        outs.append(out)
    for a in agents:
        a._settle_shadow()
    state = [(list(a.input_ids), a.resources.llm.n_tokens, dict(a._kv_shadow.stats), a.trim_to_secs) for a in agents]
    counters = (drv.fused_shadow_calls, drv.fused_shadow_tiles, drv.fused_ticks, drv.fused_frames)
    drv.close()
    return outs, state, counters


def test_the_run_with_batched_shadow_tiles_equals_the_run_without():
    on, s_on, c_on = _drive(True)
    off, s_off, c_off = _drive(False)
    print("fused shadow calls / tiles:", c_on[:2], "shadow stats of agent 0:", s_on[0][2])
    assert c_off[:2] == (0, 0)
    assert c_on[0] > 0 and c_on[1] >= 2 * c_on[0], c_on            # every pool call carried at least two tiles
    assert c_on[2:] == c_off[2:] and c_on[2] >= 10, (c_on, c_off)
    for t in range(TICKS):
        for s in range(N_AGENTS):
            assert np.array_equal(on[t][s], off[t][s]), ("PCM of agent", s, "tick", t)
    for s, (a, b) in enumerate(zip(s_on, s_off)):
        assert a[0] == b[0], ("input_ids of agent", s)
        assert a[1] == b[1], ("n_tokens of agent", s)
        assert a[2] == b[2], ("shadow stats of agent", s, a[2], b[2])
        assert a[2]["fallbacks"] == b[2]["fallbacks"]
        assert a[2]["swaps"] >= 1 and a[3] > 0, ("agent", s, "did not trim through its shadow cache", a[2], a[3])
