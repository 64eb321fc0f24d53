"""rca_lm_batch_eval: (1) ms for k shadow tiles of 128 tokens on k twins as ONE LlamaBatchEval.eval_async + sync against the same k
eval_async calls one after another + a sync of each, k = 1, 2, 4, 8; (2) a RealtimeAgentBatch tick of 64 sessions end to end with
batch_shadow_tiles off and on, and the counters.
1B dims, random-init weights, bf16, the default codec, weight-sharing handles, graphs on.
usage: lm_batch_eval.py CONTEXT STEPS     (RCA_LM_FORMAT / RCA_LM_KV as scripts/batch_step_probe.py; RCA_PROBE_PARTS=lm|driver: one part only)
(1) The two legs alternate inside one process (batch, single, batch, ... REPEATS times each); every timed leg is STEPS calls behind
WARMUP untimed calls of the same leg (the second call of a geometry captures its graph); every call starts from CONTEXT (n_tokens is
put back).  The twins run on low-priority streams, as the shadow twins do.
(2) 64 agents with their own signals and sampler seeds and the default shadow tile of 128 are driven with the flag off until their
contexts reach CONTEXT tokens; the sessions start together, so every session's shadow cache is planned in the same tick (20 s of
audio in) and all 64 owe a tile in the same tick, once per 16 ticks: the burst case.  Then blocks of TICKS ticks (two bursts each)
alternate between flag off and on, REPEATS blocks each, on the same sessions.  A tick is timed around
RealtimeAgentBatch.process_audio, which begins by waiting for the tiles of the tick before.  No trim falls into the run."""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from realtime_codec_agent_amd import RealtimeAgentBatch
from realtime_codec_agent_amd.duplex_bench import synth_signal
from realtime_codec_agent_amd.llm import LlamaBatchEval, LlamaForAlternatingCodeChannels, LMConfig
from realtime_codec_agent_amd.realtime_agent_config import RealtimeAgentConfig
from realtime_codec_agent_amd.realtime_agent_resources import RealtimeAgentResources
from realtime_codec_agent_amd.realtime_agent_v2 import RealtimeAgent

ctx = int(sys.argv[1]) if len(sys.argv) > 1 else 2200
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 10
REPEATS, WARMUP, NB, TICKS, TILE = 3, 3, 64, 32, 128
SHAPES = (1, 2, 4, 8)
parts = (os.environ.get("RCA_PROBE_PARTS") or "lm,driver").split(",")
cfg = LMConfig.llama_3_2_1b()
fmt = os.environ.get("RCA_LM_FORMAT")
kvf = os.environ.get("RCA_LM_KV") or None
n_ctx = (ctx + 256 + TICKS * 2 * REPEATS * 8 + 255) // 256 * 256


def mmm(v):
    return f"{float(np.median(v)):.3f} [{min(v):.3f} .. {max(v):.3f}]"


def lm_legs():
    parent = LlamaForAlternatingCodeChannels(model_path="random:1b", config=cfg, n_ctx=n_ctx, device=0, weight_format=fmt, **({"kv_format": kvf} if kvf else {}))
    twins = [parent.make_kv_shadow() for _ in range(max(SHAPES))]
    rng = np.random.default_rng(0)
    ids = rng.integers(128266, 259338, ctx + TILE * max(SHAPES)).tolist()
    parent.eval(ids[:ctx]); parent.sync()
    for m in twins:
        m.copy_kv_from(parent, ctx); m.n_tokens = ctx; m.sync()
    pool = LlamaBatchEval(parent)
    tiles = [ids[ctx + TILE * k:ctx + TILE * (k + 1)] for k in range(max(SHAPES))]

    def leg_batch(k, rounds):
        for _ in range(rounds):
            pool.eval_async(twins[:k], tiles[:k])
            pool.sync()
            for m in twins[:k]:
                m.n_tokens = ctx

    def leg_single(k, rounds):
        for _ in range(rounds):
            for m, t in zip(twins[:k], tiles[:k]):
                m.eval_async(t)
            for m in twins[:k]:
                m.sync()
                m.n_tokens = ctx

    def timed(f, k):
        f(k, WARMUP)
        t0 = time.perf_counter()
        f(k, steps)
        return (time.perf_counter() - t0) / steps * 1e3

    print(f"(1) fmt={parent.weight_format} kv={parent.kv_format} ctx={ctx} steps={steps} repeats={REPEATS} warmup={WARMUP} "
          f"(ms for k tiles of {TILE} tokens on k twins; median [min .. max])", flush=True)
    med = {}
    for k in SHAPES:
        tb, ts = [], []
        for _ in range(REPEATS):
            tb.append(timed(leg_batch, k)); ts.append(timed(leg_single, k))
        b, s = float(np.median(tb)), float(np.median(ts))
        med[k] = (b, s)
        print(f"k={k}: one batch eval {mmm(tb)}   {k} eval_async calls {mmm(ts)} ({s / k:.3f} each)   batch / single = {b / s:.3f}", flush=True)
    wins = [k for k in SHAPES if med[k][0] < med[k][1]]
    print(f"the batch call is faster than the single calls at k in {wins or 'no k'} (of {SHAPES})", flush=True)
    pool.close()
    for m in reversed(twins):
        m.close()
    parent.close()


def driver_legs():
    res = [RealtimeAgentResources(llm_model_path="random:Llama-3.2-1B-codec", llm_n_ctx=n_ctx, llm_config=cfg, with_aux_llm=False, llm_random_seed=0,
                                  llm_weight_format=fmt, llm_kv_format=kvf)]
    res += [res[0].clone_for_self_play() for _ in range(NB - 1)]
    agents = []
    for s, r in enumerate(res):
        c = RealtimeAgentConfig(chunk_size_secs=0.08, use_whisper=False, top_k=100, temperature=1.0, seed=42 + s, max_context_secs=1e6, trim_by_secs=20.0,
                                force_trans_after_inactivity_secs=0.0, force_response_after_inactivity_secs=0.0)
        agents.append(RealtimeAgent(resources=r, config=c))
    drv = RealtimeAgentBatch(agents, min_batch=4, batch_shadow_tiles=True)
    if drv._shadow_pool is None:
        print("(2) not measured: no LlamaBatchEval for these LMs", flush=True)
        return
    drv.batch_shadow_tiles = False
    cs = agents[0].chunk_size_samples
    fill = (ctx - agents[0].resources.llm.n_tokens) // 8 + 1
    total = fill + 2 * REPEATS * TICKS
    sigs = [synth_signal(total * cs, 100 + s) * (0.5 + 0.5 * np.sin(np.arange(total * cs) / 16000.0 * (0.3 + 0.05 * s)) ** 2).astype(np.float32) for s in range(NB)]
    t = [0]

    def tiles_fed():
        return sum(a._kv_shadow.stats["tiles"] for a in agents if a._kv_shadow is not None)

    def tick():
        row = [sigs[s][t[0] * cs:(t[0] + 1) * cs] for s in range(NB)]
        t[0] += 1
        t0 = time.perf_counter()
        drv.process_audio(row)
        return (time.perf_counter() - t0) * 1e3

    t0 = time.perf_counter()
    for _ in range(fill):
        tick()
    print(f"(2) 64 sessions driven to {min(a.resources.llm.n_tokens for a in agents)} .. {max(a.resources.llm.n_tokens for a in agents)} tokens in {fill} ticks "
          f"({time.perf_counter() - t0:.1f} s); fused frames so far {drv.fused_frames}; shadow tiles fed so far {tiles_fed()}; min_batch {drv.min_batch}", flush=True)
    legs, worst = {False: [], True: []}, {False: [], True: []}
    for rep in range(REPEATS):
        for flag in (False, True):
            drv.batch_shadow_tiles = flag
            c0, s0, f0, n0 = drv.fused_shadow_calls, drv.fused_shadow_tiles, drv.fused_frames, tiles_fed()
            got = [tick() for _ in range(TICKS)]
            legs[flag].append(float(np.median(got)))
            worst[flag].append(max(got))
            slow = sorted(got)[-4:]
            print(f"    block {rep} batch_shadow_tiles={flag}: tick median {np.median(got):.3f} ms, mean {np.mean(got):.3f}, four slowest {' '.join(f'{x:.1f}' for x in slow)}; "
                  f"tiles fed {tiles_fed() - n0}, fused_shadow_calls {drv.fused_shadow_calls - c0} over fused_shadow_tiles {drv.fused_shadow_tiles - s0}; "
                  f"fused frames {drv.fused_frames - f0}; context {agents[0].resources.llm.n_tokens}", flush=True)
    off, on = float(np.median(legs[False])), float(np.median(legs[True]))
    print(f"tick of 64 sessions at ctx ~{ctx}: batch_shadow_tiles off median {mmm(legs[False])} ms, slowest tick {mmm(worst[False])} ms   "
          f"on median {mmm(legs[True])} ms, slowest tick {mmm(worst[True])} ms   median on / off = {on / off:.3f}, slowest on / off = "
          f"{float(np.median(worst[True])) / float(np.median(worst[False])):.3f} ({REPEATS} blocks of {TICKS} ticks per leg)", flush=True)
    drv.close()


if "lm" in parts:
    lm_legs()
if "driver" in parts:
    driver_legs()
