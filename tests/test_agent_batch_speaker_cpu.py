"""RealtimeAgentBatch(batch_speaker_step=...) on the CPU, over the fakes of tests/test_agent_batch_cpu.py and a fake batch whose
frame() and step_probe() run the members' FakeLLMs: with the flag on a tick makes exactly one batch step_probe with exactly the members
whose z-score was >= 0, after every commit and before any _advance_shadow, and rolls every member back by one position; fewer than
min_batch owing members take their own steps; with the flag off the batch call is never made; measure_event_prob() with its default
arguments behaves as before.  The fake LM's next token is a function of the evaluated context alone, so the sessions with the flag on
are the sessions with it off.  Fails on the parent commit: the constructor argument and the deferral do not exist."""
import numpy as np

from test_agent_batch_cpu import _agents, _chunks, _plan


def _softmax(x):
    e = np.exp(x.astype(np.float64) - x.max())
    return e / e.sum()


class FakeBatch:
    """LlamaBatch's frame(members=) and step_probe over FakeLLMs: what the members' own steps would do, one member after the other"""

    def __init__(self, llms, events):
        self.members, self.events = llms, events
        self.probe_calls = []        # (members, n_tokens of each before the step)

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
            probs.append(_softmax(llm.logits_for_state())[probe_ids[k]])
        return toks, np.array(probs, np.float32)

    def step_probe(self, members, tokens_per_member, probe_ids_per_member=None):
        self.events.append(("probe", list(members)))
        self.probe_calls.append((list(members), [self.members[s].n_tokens for s in members]))
        toks, probs = [], []
        for k, s in enumerate(members):
            llm = self.members[s]
            llm.eval(tokens_per_member[k])
            toks.append(llm.sample())
            probs.append(_softmax(llm.logits_for_state())[probe_ids_per_member[k]])
        return toks, np.array(probs, np.float32)

    def close(self):
        pass


def _driver(n, min_batch, flag, **drv_kw):
    """n fake agents under a driver whose batch is a FakeBatch; an agent is ready whenever its frame could run as one replay"""
    from realtime_codec_agent_amd import RealtimeAgentBatch
    agents = _agents(n)
    kw = dict(batch_speaker_step=flag) if flag is not None else {}
    drv = RealtimeAgentBatch(agents, min_batch=min_batch, use_duplex_batch_graph=False, **kw, **drv_kw)
    events, singles = [], []
    drv._batch = FakeBatch([a.resources.llm for a in agents], events)
    for i, a in enumerate(agents):
        nf = a.chunk_size_frames_per_channel
        a._replay_plan = lambda chunk, a=a, nf=nf: _plan(n=nf) if a._frame_ready(nf, False) else None

        def measure(*args, _real=a.measure_event_prob, i=i, **kwargs):
            _real(*args, **kwargs)
            events.append(("commit", i))

        def advance(_real=a._advance_shadow, i=i):
            events.append(("advance", i))
            _real()

        def single(_real=a.get_probable_event_speaker, i=i):
            singles.append(i)
            return _real()

        a.measure_event_prob, a._advance_shadow, a.get_probable_event_speaker = measure, advance, single
    return drv, agents, events, singles


def _run(n, min_batch, flag, ticks=30):
    drv, agents, events, singles = _driver(n, min_batch, flag)
    rows = _chunks(n, ticks, agents[0].chunk_size_samples)
    per_tick = []
    for row in rows:
        del events[:], singles[:]
        n_calls = len(drv._batch.probe_calls)
        outs = drv.process_audio(row)
        per_tick.append(dict(events=list(events), singles=list(singles), calls=drv._batch.probe_calls[n_calls:], outs=outs,
                             z=[a.stats.event_prob.last_zscore for a in agents], pos=[a.resources.llm.n_tokens for a in agents],
                             speaker=[a.prob_event_speaker_token_id for a in agents]))
    return drv, agents, per_tick


def test_flag_on_one_batch_step_probe_per_tick_with_exactly_the_owing_members():
    n, min_batch = 5, 2
    drv, agents, ticks = _run(n, min_batch, True)
    batched = small = 0
    for t, tk in enumerate(ticks):
        fused = sorted(i for kind, m in tk["events"] if kind == "frame" for i in m)      # the members of this tick's batch frame
        if not fused:       # (the first tick: no agent is in audio mode yet, each runs on its own and keeps its own step)
            assert tk["calls"] == [] and tk["singles"] == [i for i in range(n) if tk["z"][i] >= 0.0]
            continue
        assert fused == list(range(n))
        owing = [i for i in fused if tk["z"][i] >= 0.0]
        assert not any(a.speaker_step_owed for a in agents), t
        if len(owing) >= min_batch:
            batched += 1
            assert len(tk["calls"]) == 1 and tk["calls"][0][0] == owing and tk["singles"] == [], (t, tk["calls"], owing)
            kinds = [k for k, _ in tk["events"]]
            assert kinds.count("probe") == 1
            at = kinds.index("probe")
            assert kinds[:at] == ["frame"] + ["commit"] * n and kinds[at + 1:] == ["advance"] * n, (t, kinds)
            for s, before in zip(*tk["calls"][0]):
                assert tk["pos"][s] == before, ("member", s, "is not rolled back by one position at tick", t)
        else:
            small += 1 if owing else 0
            assert tk["calls"] == [] and tk["singles"] == owing, (t, tk["singles"], owing)
        for i in range(n):
            want_none = tk["z"][i] < 0.0
            assert (tk["speaker"][i] is None) == want_none, (t, i)
    assert batched >= 5 and small >= 1, (batched, small)
    assert drv.fused_speaker_calls == batched and drv.fused_speaker_steps == sum(len(tk["calls"][0][0]) for tk in ticks if tk["calls"])


def test_below_min_batch_the_members_take_their_own_steps():
    """min_batch above the number of agents that can owe the step: frames are fused (the group rule is the same number), the steps single"""
    n = 3
    drv, agents, ticks = _run(n, 3, True)
    assert drv.fused_ticks >= 10
    singles = 0
    for tk in ticks:
        owing = [i for i in range(n) if tk["z"][i] >= 0.0]
        if len(owing) < 3:
            assert tk["calls"] == [] and tk["singles"] == owing
            singles += len(owing) if any(kind == "frame" for kind, _ in tk["events"]) else 0
    assert singles >= 5


def test_flag_off_never_calls_it_and_the_sessions_are_the_same():
    on = _run(4, 2, True)
    off = _run(4, 2, False)
    default = _run(4, 2, None)
    assert on[0].fused_speaker_calls > 0
    for drv, agents, ticks in (off, default):
        assert drv.batch_speaker_step is False and drv.fused_speaker_calls == 0 and drv.fused_speaker_steps == 0
        assert drv._batch.probe_calls == [] and not any(a.speaker_step_owed for a in agents)
        assert all(k != "probe" for tk in ticks for k, _ in tk["events"])
    for a, b, c in zip(on[1], off[1], default[1]):
        assert a.input_ids == b.input_ids == c.input_ids and a.resources.llm.n_tokens == b.resources.llm.n_tokens == c.resources.llm.n_tokens
        assert np.array_equal(a.stats.event_prob.values, b.stats.event_prob.values)
    for ta, tb in zip(on[2], off[2]):
        assert ta["speaker"] == tb["speaker"] and ta["pos"] == tb["pos"]
        for x, y in zip(ta["outs"], tb["outs"]):
            assert np.array_equal(x, y)


def test_measure_event_prob_defaults_keep_the_step_and_defer_speaker_marks_it_owed():
    a = _agents(1)[0]
    a.process_audio(_chunks(1, 1, a.chunk_size_samples)[0][0])
    llm = a.resources.llm
    evals = len(llm.log)
    a.measure_event_prob(1.0)                               # at or above the rolling mean: the speculative step runs here
    assert a.stats.event_prob.last_zscore >= 0.0
    assert a.prob_event_speaker_token_id in (a.agent_speaker_token_id, a.user_speaker_token_id) and a.speaker_step_owed is False
    assert len(llm.log) == evals + 1 and llm.log[-1][2] == [a.end_audio_token_id]
    pos = llm.n_tokens
    a.measure_event_prob(1.0, defer_speaker=True)            # deferred: no step, the driver reads and clears the mark
    assert a.prob_event_speaker_token_id is None and a.speaker_step_owed is True and len(llm.log) == evals + 1 and llm.n_tokens == pos
    a.speaker_step_owed = False
    a.measure_event_prob(0.0, defer_speaker=True)            # below the mean: nothing owed either way
    assert a.stats.event_prob.last_zscore < 0.0 and a.prob_event_speaker_token_id is None and a.speaker_step_owed is False
    assert a._set_probable_event_speaker(0.2, 0.1) == a.agent_speaker_token_id == a.prob_event_speaker_token_id
    assert a._set_probable_event_speaker(0.1, 0.1) == a.user_speaker_token_id == a.prob_event_speaker_token_id
