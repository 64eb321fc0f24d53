"""rca_lm_kv_remove_many: (a) HOST time of ONE kv_remove_many over N weight-sharing twins against the same N kv_remove calls one after
another, N = 2 .. 64, at the trims of scripts/kv_shift_timing.py (150-token header; 2.2 k context with 550 positions removed, 6.6 k
with 1 650 removed), with the batched call on its own routing (delta >= 256: the direct route) and held on the staged route; (b) a
RealtimeAgentBatch tick of 64 sessions that start together in kv_trim_mode="shift" with batch_shift_trims off and on, and the same
sessions in the default recompute / shadow mode.
1B dims, random-init weights, bf16, the default codec, weight-sharing handles, graphs on.  The KV cache is fp16, or with RCA_LM_KV=q8_0
q8_0 blocks with the shift allowed (kv_shift_requant=True: the moved keys are re-quantised).
usage: kv_shift_many.py [CONTEXT ...]     (RCA_PROBE_PARTS=call|driver: one part only; RCA_PROBE_SHAPES=2,8,64: the N of (a);
                                           RCA_PROBE_MODES=shift: the modes of (b); contexts default to 2200 6600 for (a), 2200 for (b))
(a) The three legs alternate inside one process (single, many, many-staged, single, ... REPEATS times each); a timed leg is CALLS calls
behind one untimed call of the same leg, each around a host clock with every stream idle before it; n_tokens is put back between
calls (the rows above are stale but still there: the same work again).  Bytes are the cache bytes read + written once (the staged
routes move them twice).
(b) A quarter of the context is trimmed each time and the limit sits one frame below a chunk boundary, so every trim falls due before
the first step of a frame, in all 64 sessions in the same tick.  The first trim is a warm-up (staging allocations, code objects);
then the flag alternates from trim period to trim period on the same sessions, TRIMS periods each.  A tick is timed around
RealtimeAgentBatch.process_audio; "inside the shift calls" is a host clock around the sessions' kv_remove / kv_remove_many alone."""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from realtime_codec_agent_amd import RealtimeAgentBatch
from realtime_codec_agent_amd.duplex_bench import synth_signal
from realtime_codec_agent_amd.llm import LlamaForAlternatingCodeChannels, LMConfig, kv_remove_many
from realtime_codec_agent_amd.realtime_agent_config import RealtimeAgentConfig
from realtime_codec_agent_amd.realtime_agent_resources import RealtimeAgentResources
from realtime_codec_agent_amd.realtime_agent_v2 import RealtimeAgent

contexts = [int(a) for a in sys.argv[1:]]
parts = (os.environ.get("RCA_PROBE_PARTS") or "call,driver").split(",")
REPEATS, CALLS, NB, TRIMS, HEADER = 3, 5, 64, 3, 150
SHAPES = tuple(int(x) for x in (os.environ.get("RCA_PROBE_SHAPES") or "2,4,8,16,32,64").split(","))
MODES = (os.environ.get("RCA_PROBE_MODES") or "shift,recompute").split(",")
KV = os.environ.get("RCA_LM_KV") or None                          # None / "f16" / "q8_0"
KV_ARGS = dict(kv_format=KV, kv_shift_requant=True) if KV == "q8_0" else dict(kv_format=KV)
cfg = LMConfig.llama_3_2_1b()
row_bytes = cfg.n_layers * cfg.n_kv_heads * (68 if KV == "q8_0" else 64 * 2) * 2      # one position: K and V of every layer, fp16 rows or q8_0 blocks


def mmm(v):
    return f"{float(np.median(v)):.3f} [{min(v):.3f} .. {max(v):.3f}]"


def call_legs(ctxs):
    n_ctx = (max(ctxs) + 511) // 256 * 256
    parent = LlamaForAlternatingCodeChannels(model_path="random:1b", config=cfg, n_ctx=n_ctx, random_seed=0, device=0, **KV_ARGS)
    assert parent.kv_bytes_per_position() == row_bytes
    print(f"KV cache {parent.kv_format}: {row_bytes} bytes per position", flush=True)
    twins = [parent.make_kv_shadow(low_priority=False) for _ in range(max(SHAPES))]
    ids = np.random.default_rng(5).integers(128266, 259338, max(ctxs)).tolist()
    for n in ctxs:
        cut = n // 4
        span = (HEADER, HEADER + cut)
        moved = n - HEADER - cut
        parent.reset()
        parent.eval(ids[:n]); parent.sync()
        for m in twins:
            m.copy_kv_from(parent, n); m.n_tokens = n; m.sync()

        def restore(k):
            for m in twins[:k]:
                m.n_tokens = n
                m.sync()

        def leg_single(k):
            for m in twins[:k]:
                m.kv_remove(*span)

        def leg_many(k):
            kv_remove_many(twins[:k], [span] * k)

        def leg_staged(k):
            kv_remove_many(twins[:k], [span] * k, staged_only=True)

        def timed(f, k):
            out = []
            for i in range(CALLS + 1):
                restore(k)
                t0 = time.perf_counter()
                f(k)
                out.append((time.perf_counter() - t0) * 1e3)
            return float(np.median(out[1:]))

        print(f"(a) ctx={n} span=[{span[0]}, {span[1]}) rows moved per handle {moved} ({2 * moved * row_bytes / 1e6:.1f} MB read + written); single: "
              f"{-(-moved // 256) + 1} launches + 1 synchronisation per handle; many: {-(-moved // cut)} launches per group of 8 handles, 1 synchronisation; "
              f"many staged: {-(-moved // 256) + 1} launches per group; ms, median of {CALLS} calls per run, {REPEATS} runs: median [min .. max]", flush=True)
        med = {}
        for k in SHAPES:
            ts, tm, tg = [], [], []
            for _ in range(REPEATS):
                ts.append(timed(leg_single, k)); tm.append(timed(leg_many, k)); tg.append(timed(leg_staged, k))
            s, m_, g = float(np.median(ts)), float(np.median(tm)), float(np.median(tg))
            med[k] = (s, m_, g)
            gb = k * 2 * moved * row_bytes / 1e6
            print(f"N={k}: {k} kv_remove calls {mmm(ts)} ({gb / s:.0f} GB/s)   one kv_remove_many {mmm(tm)} ({gb / m_:.0f} GB/s)   "
                  f"held on the staged route {mmm(tg)} ({gb / g:.0f} GB/s)   many / single = {m_ / s:.3f}   staged many / single = {g / s:.3f}", flush=True)
        wins = [k for k in SHAPES if med[k][1] < med[k][0]]
        wins_g = [k for k in SHAPES if med[k][2] < med[k][0]]
        print(f"ctx={n}: kv_remove_many is faster than the single calls at N in {wins or 'no N'}; held on the staged route at N in {wins_g or 'no N'} (of {SHAPES})", flush=True)
    for m in reversed(twins):
        m.close()
    parent.close()


def driver_legs(ctx, mode):
    """mode 'shift': flag off / on alternating; 'recompute': the default trim through the shadow cache, the flag does not apply"""
    per_chunk, per_sec = 8, 100.0                       # 80 ms chunks of 4 frames per channel
    limit_chunks = (ctx - HEADER) // per_chunk
    period = limit_chunks // 4                          # a quarter of the context per trim
    n_ctx = (ctx + 767) // 256 * 256
    res = [RealtimeAgentResources(llm_model_path="random:Llama-3.2-1B-codec", llm_n_ctx=n_ctx, llm_config=cfg, with_aux_llm=False, llm_random_seed=0,
                                  **{"llm_" + k: v for k, v in KV_ARGS.items()})]
    res += [res[0].clone_for_self_play() for _ in range(NB - 1)]
    bpp = res[0].llm.kv_bytes_per_position()
    print(f"(b) KV cache {res[0].llm.kv_format}: {bpp} bytes per position, {bpp * ctx / 1e6:.1f} MB per session and cache at {ctx} positions "
          f"({mode}: {'one cache' if mode == 'shift' else 'two caches, live and shadow'} per session)", flush=True)
    agents = []
    for s, r in enumerate(res):
        c = RealtimeAgentConfig(chunk_size_secs=0.08, use_whisper=False, top_k=100, temperature=1.0, seed=42 + s,
                                max_context_secs=(limit_chunks * per_chunk - 1) / per_sec, trim_by_secs=period * per_chunk / per_sec,
                                force_trans_after_inactivity_secs=0.0, force_response_after_inactivity_secs=0.0)
        agents.append(RealtimeAgent(resources=r, config=c, **({"kv_trim_mode": "shift"} if mode == "shift" else {})))
    assert 2 * agents[0].chunk_size_frames_per_channel == per_chunk and agents[0].resources.audio_tokenizer.framerate * 2 == per_sec
    drv = RealtimeAgentBatch(agents, min_batch=4)
    cs = agents[0].chunk_size_samples
    spent = [0.0]                                       # host ms inside kv_remove / kv_remove_many: a trim tick's share that is the shift itself

    def clocked(f):
        def g(*a, **k):
            t0 = time.perf_counter()
            r = f(*a, **k)
            spent[0] += (time.perf_counter() - t0) * 1e3
            return r
        return g

    if mode == "shift":
        for a in agents:
            m = a.resources.llm
            m.kv_remove, m.kv_remove_many = clocked(m.kv_remove), clocked(m.kv_remove_many)
    n_periods = 1 + (2 * TRIMS if mode == "shift" else TRIMS)
    total = limit_chunks + n_periods * period - period // 2
    sigs = [synth_signal(total * cs, 100 + s) * (0.5 + 0.5 * np.sin(np.arange(total * cs) / 16000.0 * (0.3 + 0.05 * s)) ** 2).astype(np.float32) for s in range(NB)]
    t = [0]

    def tick():
        row = [sigs[s][t[0] * cs:(t[0] + 1) * cs] for s in range(NB)]
        t[0] += 1
        was = agents[0].trim_to_secs
        t0 = time.perf_counter()
        drv.process_audio(row)
        return (time.perf_counter() - t0) * 1e3, agents[0].trim_to_secs != was

    t0 = time.perf_counter()
    fill = limit_chunks - period // 2
    for _ in range(fill):
        tick()
    print(f"(b) {mode}: 64 sessions driven to {min(a.resources.llm.n_tokens for a in agents)} .. {max(a.resources.llm.n_tokens for a in agents)} tokens in {fill} ticks "
          f"({time.perf_counter() - t0:.1f} s); limit {limit_chunks} chunks, {period} chunks ({period * per_chunk} positions) per trim; fused frames so far {drv.fused_frames}", flush=True)
    legs = {}
    for p in range(n_periods):
        flag = mode == "shift" and p >= 1 and p % 2 == 1
        drv.batch_shift_trims = flag
        c0, f0, spent[0] = drv.fused_shift_calls, drv.fused_frames, 0.0
        got = [tick() for _ in range(period)]
        ms = [g[0] for g in got]
        trim = [g[0] for g in got if g[1]]
        label = "warm-up" if p == 0 else (f"batch_shift_trims={flag}" if mode == "shift" else "recompute / shadow")
        if p:
            legs.setdefault(label, []).append((float(np.median(ms)), trim, max(ms), spent[0]))
        print(f"    period {p} {label}: tick median {np.median(ms):.3f} ms, mean {np.mean(ms):.3f}, trim ticks {' '.join(f'{x:.2f}' for x in trim) or 'none'}, four slowest "
              f"{' '.join(f'{x:.1f}' for x in sorted(ms)[-4:])}; inside the shift calls {spent[0]:.3f} ms; fused_shift_calls {drv.fused_shift_calls - c0}; fused frames {drv.fused_frames - f0}; "
              f"context {agents[0].resources.llm.n_tokens}", flush=True)
    for label, v in legs.items():
        print(f"{mode} ctx ~{ctx}, {label}: median tick {mmm([x[0] for x in v])} ms; trim tick {mmm([y for x in v for y in x[1]])} ms; slowest tick of a period "
              f"{mmm([x[2] for x in v])} ms; inside the shift calls of a trim tick {mmm([x[3] for x in v])} ms ({len(v)} periods of {period} ticks)", flush=True)
    drv.close()


if "call" in parts:
    call_legs(contexts or [2200, 6600])
if "driver" in parts:
    for ctx in (contexts or [2200]):
        for mode in MODES:
            driver_legs(ctx, mode)
