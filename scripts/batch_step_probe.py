"""The batched speculative <|end_audio|> step: (1) ms per call of ONE LlamaBatch.step_probe (rca_lm_batch_step_sel) over a selection of
4, 8, 16, 32 and 64 of 64 members (n = 1, 2 probe ids) against the same members' step_probe calls one after another; (2) a
RealtimeAgentBatch tick of 64 sessions end to end with batch_speaker_step off and on, and how many members owed the step per tick.
1B dims, random-init weights (head rows outside the codec range zeroed), the default codec, weight-sharing handles, graphs on.
usage: batch_step_probe.py CONTEXT STEPS     (RCA_LM_FORMAT=q8_0|q4_k|... as scripts/lm_profile.py; RCA_LM_KV=q8_0: q8_0 KV caches;
                                              RCA_PROBE_PARTS=lm|driver: one part only)
(1) The two legs alternate inside one process (batch, single, batch, ... REPEATS times each); every timed leg is STEPS calls behind
WARMUP untimed calls of the same leg; every call starts from CONTEXT (n_tokens is put back, as the agent does after the step).
(2) 64 agents with their own signals and sampler seeds are driven with the flag off until their contexts reach CONTEXT tokens (the
first 25 ticks fill the codec windows, each session on its own); then blocks of TICKS ticks alternate between flag off and on, REPEATS
blocks each, on the same sessions (a tick adds 8 tokens per session, so the legs see the same contexts within 1 %).  A tick is timed
around RealtimeAgentBatch.process_audio.  KV shadows are off and no trim falls into the run: the tick is the duplex batch frame, the
commits and the speaker steps."""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from realtime_codec_agent_amd import RealtimeAgentBatch
from realtime_codec_agent_amd.duplex_bench import synth_signal
from realtime_codec_agent_amd.llm import LlamaBatch, LlamaForAlternatingCodeChannels, LMConfig
from realtime_codec_agent_amd.realtime_agent_config import RealtimeAgentConfig
from realtime_codec_agent_amd.realtime_agent_resources import RealtimeAgentResources
from realtime_codec_agent_amd.realtime_agent_v2 import RealtimeAgent

ctx = int(sys.argv[1]) if len(sys.argv) > 1 else 2200
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 20
REPEATS, WARMUP, NB, TICKS = 3, 3, 64, 20
SHAPES = (4, 8, 16, 32, 64)
parts = (os.environ.get("RCA_PROBE_PARTS") or "lm,driver").split(",")
cfg = LMConfig.llama_3_2_1b()
fmt = os.environ.get("RCA_LM_FORMAT")
kvf = os.environ.get("RCA_LM_KV") or None    # "q8_0": quantised KV cache; the twins inherit it
n_ctx = (ctx + 64 + TICKS * 2 * REPEATS * 8 + 255) // 256 * 256


def mmm(v):
    return f"{float(np.median(v)):.3f} [{min(v):.3f} .. {max(v):.3f}]"


def lm_legs():
    parent = LlamaForAlternatingCodeChannels(model_path="random:1b", config=cfg, n_ctx=n_ctx, device=0, weight_format=fmt, **({"kv_format": kvf} if kvf else {}))
    if kvf:
        print(f"kv_format {parent.kv_format}: {parent.kv_bytes_per_position()} bytes per cached position")
    members = [parent] + [LlamaForAlternatingCodeChannels(n_ctx=n_ctx, share_weights_with=parent, device=0) for _ in range(NB - 1)]
    rng = np.random.default_rng(0)
    ids = rng.integers(128266, 259338, ctx + 80).tolist()
    parent.eval(ids[:ctx]); parent.sync()
    for s, m in enumerate(members):
        m.init_sampler_for_generate(top_k=100, top_p=1.0, min_p=0.0, temp=1.0, seed=42 + s)
        if s:
            m.copy_kv_from(parent, ctx); m.sync()
    bat = LlamaBatch(members)
    end_audio, spk = ids[ctx], [ids[ctx + 1], ids[ctx + 2]]       # any three ids: the step's cost does not depend on them

    def leg_batch(sel, rounds):
        for _ in range(rounds):
            bat.step_probe(sel, [[end_audio]] * len(sel), [spk] * len(sel))
            for s in sel:
                members[s].n_tokens = ctx

    def leg_single(sel, rounds):
        for _ in range(rounds):
            for s in sel:
                members[s].step_probe([end_audio], spk)
                members[s].n_tokens = ctx

    def timed(f, sel):
        f(sel, WARMUP)
        t0 = time.perf_counter()
        f(sel, steps)
        return (time.perf_counter() - t0) / steps * 1e3

    print(f"(1) fmt={parent.weight_format} ctx={ctx} steps={steps} repeats={REPEATS} warmup={WARMUP} n=1, 2 probe ids (ms per call over N of {NB} members; median [min .. max])",
          flush=True)
    med = {}
    for nm in SHAPES:
        sel = list(range(0, NB, NB // nm))[:nm]       # spread over the batch: a selection, not its first members
        tb, ts = [], []
        for _ in range(REPEATS):
            tb.append(timed(leg_batch, sel)); ts.append(timed(leg_single, sel))
        b, s = float(np.median(tb)), float(np.median(ts))
        med[nm] = (b, s)
        print(f"N={nm:2d}: one batch step_probe {mmm(tb)}   {nm} single step_probe calls {mmm(ts)} ({s / nm:.3f} each)   batch / single = {b / s:.3f}", flush=True)
    wins = [nm for nm in SHAPES if med[nm][0] < med[nm][1]]
    print(f"the batch call is faster than the single calls from N = {min(wins) if wins else 'never (up to 64)'} on (of {SHAPES}); captures {bat.captures()}", flush=True)
    bat.close()
    for m in reversed(members):
        m.close()


def driver_legs():
    res = [RealtimeAgentResources(llm_model_path="random:Llama-3.2-1B-codec", llm_n_ctx=n_ctx, llm_config=cfg, with_aux_llm=False, llm_random_seed=0,
                                  llm_weight_format=fmt, llm_kv_format=kvf)]
    res += [res[0].clone_for_self_play() for _ in range(NB - 1)]
    agents = []
    for s, r in enumerate(res):
        c = RealtimeAgentConfig(chunk_size_secs=0.08, use_whisper=False, top_k=100, temperature=1.0, seed=42 + s, max_context_secs=1e6, trim_by_secs=20.0,
                                force_trans_after_inactivity_secs=0.0, force_response_after_inactivity_secs=0.0)
        a = RealtimeAgent(resources=r, config=c)
        a.use_kv_shadow = False
        agents.append(a)
    drv = RealtimeAgentBatch(agents, min_batch=4)
    cs = agents[0].chunk_size_samples
    fill = (ctx - agents[0].resources.llm.n_tokens) // 8 + 1
    total = fill + 2 * REPEATS * TICKS
    sigs = [synth_signal(total * cs, 100 + s) * (0.5 + 0.5 * np.sin(np.arange(total * cs) / 16000.0 * (0.3 + 0.05 * s)) ** 2).astype(np.float32) for s in range(NB)]
    t = [0]

    def tick():
        row = [sigs[s][t[0] * cs:(t[0] + 1) * cs] for s in range(NB)]
        t[0] += 1
        t0 = time.perf_counter()
        drv.process_audio(row)
        ms = (time.perf_counter() - t0) * 1e3
        return ms, sum(1 for a in agents if a.stats.event_prob.last_zscore >= 0.0)

    t0 = time.perf_counter()
    for _ in range(fill):
        tick()
    print(f"(2) 64 sessions driven to {min(a.resources.llm.n_tokens for a in agents)} .. {max(a.resources.llm.n_tokens for a in agents)} tokens in {fill} ticks "
          f"({time.perf_counter() - t0:.1f} s); fused frames so far {drv.fused_frames}; min_batch {drv.min_batch}", flush=True)
    legs = {False: [], True: []}
    owed = {False: [], True: []}
    for rep in range(REPEATS):
        for flag in (False, True):
            drv.batch_speaker_step = flag
            for _ in range(WARMUP):
                tick()
            c0, s0, f0 = drv.fused_speaker_calls, drv.fused_speaker_steps, drv.fused_frames
            got = [tick() for _ in range(TICKS - WARMUP)]
            legs[flag].append(float(np.median([g[0] for g in got])))
            owed[flag] += [g[1] for g in got]
            print(f"    block {rep} batch_speaker_step={flag}: tick median {np.median([g[0] for g in got]):.3f} ms, max {max(g[0] for g in got):.3f}; owing members per tick "
                  f"{np.mean([g[1] for g in got]):.1f} [{min(g[1] for g in got)} .. {max(g[1] for g in got)}]; fused frames {drv.fused_frames - f0}, "
                  f"batch speaker calls {drv.fused_speaker_calls - c0} over {drv.fused_speaker_steps - s0} steps; context {agents[0].resources.llm.n_tokens}", flush=True)
    off, on = float(np.median(legs[False])), float(np.median(legs[True]))
    print(f"tick of 64 sessions at ctx ~{ctx}: batch_speaker_step off {mmm(legs[False])} ms   on {mmm(legs[True])} ms   on / off = {on / off:.3f}; "
          f"owing members per tick: off {np.mean(owed[False]):.1f}, on {np.mean(owed[True]):.1f} of 64 ({REPEATS} blocks of {TICKS - WARMUP} timed ticks per leg)", flush=True)
    drv.close()


if "lm" in parts:
    lm_legs()
if "driver" in parts:
    driver_legs()
