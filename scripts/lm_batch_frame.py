"""Batch frame against the same steps taken one call at a time: ms per frame in which B sessions advance by N_STEPS S=2 steps each, as
(a) ONE rca_lm_batch_frame and (b) N_STEPS rca_lm_batch_step calls of B x 2 with the sampled tokens fed back on the host, for B in 16,
64.  1B dims, random-init weights, one parent handle and its weight-sharing twins, every member at CONTEXT tokens (the parent's
prefill, copied into the twins' caches), graph replay, audio_id_floor = -1 (no member is cut).
usage: lm_batch_frame.py CONTEXT FRAMES [steps-only]      (RCA_LM_FORMAT=q8_0|q4_k|... as scripts/lm_profile.py)
The two legs alternate inside one process (frame, steps, frame, ... REPEATS times each), every timed leg is FRAMES frames behind
WARMUP untimed frames of the same leg, and every frame starts from the same context (n_tokens is put back).  Printed per shape: the
median over the repeats with the spread (min .. max) per leg, and the ratio of the medians.  With `steps-only` the frame leg is left
out, so the script also runs on a library from before rca_lm_batch_frame (RCA_LIB_PATH=..., the parent's leg of the A/B).  Every run
ends with the single 2-token rca_lm_step of member 0, the third figure the A/B compares."""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from realtime_codec_agent_amd.llm import LlamaBatch, LlamaForAlternatingCodeChannels, LMConfig

ctx = int(sys.argv[1]) if len(sys.argv) > 1 else 2200
frames = int(sys.argv[2]) if len(sys.argv) > 2 else 20
steps_only = len(sys.argv) > 3 and sys.argv[3] == "steps-only"
REPEATS, WARMUP, N_STEPS = 3, 3, 4
SHAPES = (16, 64)
cfg = LMConfig.llama_3_2_1b()
fmt = os.environ.get("RCA_LM_FORMAT")
n_ctx = (ctx + 64 + 255) // 256 * 256
parent = LlamaForAlternatingCodeChannels(model_path="random:1b", config=cfg, n_ctx=n_ctx, device=0, weight_format=fmt)
members = [parent] + [LlamaForAlternatingCodeChannels(n_ctx=n_ctx, share_weights_with=parent, device=0) for _ in range(max(SHAPES) - 1)]
rng = np.random.default_rng(0)
ids = rng.integers(128266, 259338, ctx + 80).tolist()
parent.eval(ids[:ctx]); parent.sync()
for s, m in enumerate(members):
    m.init_sampler_for_generate(top_k=100, top_p=1.0, min_p=0.0, temp=1.0, seed=42 + s)
    if s:
        m.copy_kv_from(parent, ctx); m.sync()


def leg_frame(bat, ms, pairs, users, rounds):
    for _ in range(rounds):
        for m in ms:
            m.n_tokens = ctx
        bat.frame(pairs, users, -1)


def leg_steps(bat, ms, pairs, users, rounds):
    for _ in range(rounds):
        for m in ms:
            m.n_tokens = ctx
        rows = pairs
        for i in range(N_STEPS):
            toks = bat.step(rows)
            rows = [[t, u[i]] for t, u in zip(toks, users)]


def leg_single(m, pair, rounds):
    for _ in range(rounds):
        m.n_tokens = ctx
        m.step(pair)


def timed(f, *a):
    f(*a, WARMUP)
    t0 = time.perf_counter()
    f(*a, frames)
    return (time.perf_counter() - t0) / frames * 1e3


def mmm(v):
    return f"{float(np.median(v)):.3f} [{min(v):.3f} .. {max(v):.3f}]"


print(f"fmt={parent.weight_format} ctx={ctx} frames={frames} repeats={REPEATS} warmup={WARMUP} n_steps={N_STEPS}"
      f" (ms per frame of B sessions x {N_STEPS} steps; median [min .. max])", flush=True)
for nm in SHAPES:
    ms = members[:nm]
    pairs = [ids[ctx + s:ctx + s + 2] for s in range(nm)]
    users = [ids[ctx + 8 + s:ctx + 8 + s + N_STEPS] for s in range(nm)]
    bat = LlamaBatch(ms)
    tf, ts = [], []
    for _ in range(REPEATS):
        if not steps_only:
            tf.append(timed(leg_frame, bat, ms, pairs, users))
        ts.append(timed(leg_steps, bat, ms, pairs, users))
    bat.close()
    s = float(np.median(ts))
    if steps_only:
        print(f"shape {nm}x{N_STEPS}: {N_STEPS} batch steps {mmm(ts)}", flush=True)
    else:
        f = float(np.median(tf))
        print(f"shape {nm}x{N_STEPS}: batch frame {mmm(tf)}   {N_STEPS} batch steps {mmm(ts)}   frame / steps = {f / s:.3f}"
              f"   per session and step {f / nm / N_STEPS * 1e3:.1f} us", flush=True)
t1 = [timed(leg_single, parent, ids[ctx:ctx + 2]) for _ in range(REPEATS)]
print(f"single 2-token step: {mmm(t1)}", flush=True)
