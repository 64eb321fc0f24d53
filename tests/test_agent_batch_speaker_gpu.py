"""RealtimeAgentBatch(batch_speaker_step=True) on the GPU: the agents' speculative <|end_audio|> steps of a tick as ONE
LlamaBatch.step_probe (rca_lm_batch_step_sel).  Setup as tests/test_agent_batch_gpu.py: five agents over weight-sharing LM handles
and one codec handle, 48 ticks, late joiners, a pause, trims through the shadow caches.
  - flag on: the run with use_duplex_batch_graph=True equals the run with False, per tick: PCM, prob_event_speaker_token_id; at the end:
    sequences, positions, event probabilities, trims;
  - a third run replaces LlamaBatch.step_probe by a reference made of the calls that existed before: a throw-away LlamaBatch over
    exactly the owing handles, its step(), then token_probs() per handle -- the same session byte for byte;
  - the batch call was taken, and some tick had fewer than min_batch owing members and took the single steps;
  - flag off: the run equals the driver as it was before the flag existed (its logic restated here), and never calls step_probe.
Fails on the parent commit: the constructor argument, the deferral and LlamaBatch.step_probe do not exist."""
import functools

import numpy as np
import pytest

import test_agent_batch_gpu as ag

pytestmark = pytest.mark.gpu

N_AGENTS, TICKS = ag.N_AGENTS, ag.TICKS
MIN_BATCH = 2


def _reference_step_probe(self, members, tokens_per_member, probe_ids_per_member=None):
    """LlamaBatch.step_probe from LlamaBatch.step and token_probs alone (a handle may be a member of two batches)"""
    from realtime_codec_agent_amd.llm import LlamaBatch
    handles = [self.members[s] for s in members]
    tmp = LlamaBatch(handles)
    try:
        toks = tmp.step(tokens_per_member)
    finally:
        tmp.close()
    return toks, np.stack([h.token_probs(p) for h, p in zip(handles, probe_ids_per_member)])


def _parent_driver():
    """RealtimeAgentBatch.process_audio / _run_group as they were before batch_speaker_step existed"""
    from realtime_codec_agent_amd import RealtimeAgentBatch

    class ParentDriver(RealtimeAgentBatch):
        def process_audio(self, chunks):
            outs = [None] * len(self.agents)
            live = [i for i, c in enumerate(chunks) if c is not None]
            for i in live:
                self.agents[i]._settle_shadow()
            plans = [None] * len(self.agents)
            for i in live:
                plans[i] = self.agents[i]._replay_plan(chunks[i])
            groups, _ = self._partition(plans)
            fused = {i for g in groups for i in g}
            for g in groups:
                self._run_group(g, chunks, plans, outs)
            for i in live:
                if i not in fused:
                    outs[i] = self.agents[i].process_audio(chunks[i])
            for i in sorted(fused):
                self.agents[i]._advance_shadow()
            if groups:
                self.fused_ticks += 1
                self.fused_frames += len(fused)
            return outs

        def _run_group(self, sel, chunks, plans, outs):
            A = self.agents
            first, p0 = A[sel[0]], plans[sel[0]]
            res = self._batch.duplex_frame(self._codec(first), sel, np.stack([np.reshape(plans[i]["window"], -1) for i in sel]),
                                           np.stack([plans[i]["code_ctx"] for i in sel]), p0["n_codes"], p0["n_samples"], first._code_token_base,
                                           first.end_header_token_id, [first.end_audio_token_id] * len(sel), [A[i].input_ids[-2:] for i in sel])
            for k, i in enumerate(sel):
                a = A[i]
                with a.profilers.total_profiler:
                    out = a._replay_commit(chunks[i], plans[i], lambda r=res[k]: r)
                outs[i] = out if a.self_play_mode else out[0]

    return ParentDriver


@functools.lru_cache(maxsize=None)
def _drive(kind):
    """kind: 'fused' / 'unfused' / 'reference' with the flag on; 'off' with it off; 'parent' the driver before the flag"""
    from realtime_codec_agent_amd import RealtimeAgentBatch
    from realtime_codec_agent_amd.llm import LlamaBatch
    agents, _ = ag._make()
    if kind == "parent":
        drv = _parent_driver()(agents, min_batch=MIN_BATCH)
    else:
        drv = RealtimeAgentBatch(agents, min_batch=MIN_BATCH, use_duplex_batch_graph=kind != "unfused", batch_speaker_step=kind != "off")
    owed, calls = [], []
    real_steps = drv._run_speaker_steps
    real_probe = LlamaBatch.step_probe

    def counting_steps(fused):
        owed.append(sum(1 for i in fused if agents[i].speaker_step_owed))
        real_steps(fused)

    def counting_probe(self, members, *a, **kw):
        calls.append(list(members))
        return (_reference_step_probe if kind == "reference" else real_probe)(self, members, *a, **kw)

    drv._run_speaker_steps = counting_steps
    LlamaBatch.step_probe = counting_probe
    outs, speakers = [], []
    try:
        for t in range(TICKS):
            outs.append(drv.process_audio(ag._row(t)))
            speakers.append([a.prob_event_speaker_token_id for a in agents])
            assert not any(a.speaker_step_owed for a in agents), ("an owed step left behind at tick", t)
        state = [(list(a.input_ids), a.resources.llm.n_tokens, np.array(a.stats.event_prob.values, dtype=np.float64).copy(), a.trim_to_secs,
                  a._kv_shadow.stats["swaps"] if a._kv_shadow is not None else 0) for a in agents]
        counters = (drv.fused_ticks, drv.fused_frames, drv.fused_speaker_calls, drv.fused_speaker_steps)
    finally:
        LlamaBatch.step_probe = real_probe
        drv.close()
    return outs, speakers, state, counters, owed, calls


def _assert_same_session(x, y, tag):
    (ox, spx, stx, cx, owx, _), (oy, spy, sty, cy, owy, _) = x, y
    assert cx == cy and owx == owy, (tag, cx, cy)
    for t in range(TICKS):
        assert spx[t] == spy[t], (tag, "prob_event_speaker_token_id at tick", t)
        for s in range(N_AGENTS):
            if ox[t][s] is None:
                assert oy[t][s] is None
            else:
                assert np.array_equal(ox[t][s], oy[t][s]), (tag, "PCM of agent", s, "tick", t)
    for s, (a, b) in enumerate(zip(stx, sty)):
        assert a[0] == b[0], (tag, "input_ids of agent", s)
        assert a[1] == b[1], (tag, "n_tokens of agent", s)
        assert np.array_equal(a[2], b[2]), (tag, "event probabilities of agent", s)
        assert a[3] == b[3] and a[4] == b[4], (tag, "trims of agent", s)


def test_with_the_flag_on_the_fused_run_equals_the_unfused_run():
    fused = _drive("fused")
    _assert_same_session(fused, _drive("unfused"), "fused / unfused")
    assert any(s[3] > 0 and s[4] > 0 for s in fused[2]), "no session trimmed through its shadow cache"
    assert any(sp is not None for row in fused[1] for sp in row)


def test_the_batch_call_equals_a_reference_made_of_batch_step_and_token_probs():
    _assert_same_session(_drive("fused"), _drive("reference"), "rca_lm_batch_step_sel / step + token_probs")


def test_the_batch_call_is_taken_and_small_ticks_take_the_single_steps():
    _, _, _, counters, owed, calls = _drive("fused")
    assert counters[2] > 0 and counters[2] == len(calls) == sum(1 for n in owed if n >= MIN_BATCH)
    assert counters[3] == sum(len(c) for c in calls) == sum(n for n in owed if n >= MIN_BATCH)
    assert any(0 < n < MIN_BATCH for n in owed), ("no tick with fewer than min_batch owing members", owed)


def test_with_the_flag_off_the_run_is_the_driver_as_it_was():
    off, parent = _drive("off"), _drive("parent")
    assert off[5] == [] and parent[5] == [] and off[3][2:] == (0, 0), "step_probe on the batch with the flag off"
    assert off[4] == [], "the deferred steps ran with the flag off"
    _assert_same_session(off, parent, "flag off / the driver before the flag")
    assert off[3][0] >= 10      # two agents with full windows from about tick 32 of 48 on: groups of min_batch and more
