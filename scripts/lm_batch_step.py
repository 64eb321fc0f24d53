"""Batch step against group steps and single steps: ms per round in which B sessions advance by n tokens each, as (a) ONE rca_lm_batch_step,
(b) ceil(B / 4) rca_lm_group_step calls of 4 x 1 (n = 2: ceil(B / 2) calls of 2 x 2) and (c) B rca_lm_step calls, for B x n in
8x1, 16x1, 32x1, 64x1, 8x2, 32x2, 64x2.  1B dims, random-init weights, one parent handle and its weight-sharing twins, every member
at CONTEXT tokens (the parent's prefill, copied into the twins' caches), graph replay.
usage: lm_batch_step.py CONTEXT STEPS        (RCA_LM_FORMAT=q8_0|q4_k|... as scripts/lm_profile.py; RCA_LM_KV=q8_0: q8_0 KV caches)
The three legs alternate inside one process (batch, group, single, batch, ... REPEATS times each), every timed leg is STEPS rounds
behind WARMUP untimed rounds of the same leg, and every round starts from the same context (n_tokens is put back).  Printed per shape:
the median over the repeats with the spread (min .. max) per leg, and the ratios of the medians."""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from realtime_codec_agent_amd.llm import LlamaBatch, LlamaForAlternatingCodeChannels, LlamaGroup, LMConfig

ctx = int(sys.argv[1]) if len(sys.argv) > 1 else 2200
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 50
REPEATS, WARMUP = 5, 5
SHAPES = ((8, 1), (16, 1), (32, 1), (64, 1), (8, 2), (32, 2), (64, 2))
if os.environ.get("RCA_BATCH_SHAPES"):   # e.g. "16x1,64x1,64x2": a subset, for a short run
    SHAPES = tuple(tuple(int(v) for v in t.split("x")) for t in os.environ["RCA_BATCH_SHAPES"].split(","))
BATCH_ONLY = os.environ.get("RCA_BATCH_ONLY") == "1"   # time the batch leg alone (the group / single legs do not depend on what is compared)
cfg = LMConfig.llama_3_2_1b()
fmt = os.environ.get("RCA_LM_FORMAT")
n_ctx = (ctx + 64 + 255) // 256 * 256
kvf = os.environ.get("RCA_LM_KV") or None    # "q8_0": quantised KV cache; the twins inherit it
parent = LlamaForAlternatingCodeChannels(model_path="random:1b", config=cfg, n_ctx=n_ctx, device=0, weight_format=fmt, **({"kv_format": kvf} if kvf else {}))
if kvf:
    print(f"kv_format {parent.kv_format}: {parent.kv_bytes_per_position()} bytes per cached position")
members = [parent] + [LlamaForAlternatingCodeChannels(n_ctx=n_ctx, share_weights_with=parent, device=0) for _ in range(63)]
rng = np.random.default_rng(0)
ids = rng.integers(128266, 259338, ctx + 80).tolist()
parent.eval(ids[:ctx]); parent.sync()
for s, m in enumerate(members):
    m.init_sampler_for_generate(top_k=100, top_p=1.0, min_p=0.0, temp=1.0, seed=42 + s)
    if s:
        m.copy_kv_from(parent, ctx); m.sync()


def leg_batch(bat, ms, rows, rounds):
    for _ in range(rounds):
        for m in ms:
            m.n_tokens = ctx
        bat.step(rows)


def leg_group(grps, ms, rows, rounds):
    for _ in range(rounds):
        for m in ms:
            m.n_tokens = ctx
        for g, r in grps:
            g.step(r)


def leg_single(ms, rows, rounds):
    for _ in range(rounds):
        for m, r in zip(ms, rows):
            m.n_tokens = ctx
            m.step(r)


def timed(f, *a):
    f(*a, WARMUP)
    t0 = time.perf_counter()
    f(*a, steps)
    return (time.perf_counter() - t0) / steps * 1e3


def mmm(v):
    return f"{float(np.median(v)):.3f} [{min(v):.3f} .. {max(v):.3f}]"


print(f"fmt={parent.weight_format} ctx={ctx} steps={steps} repeats={REPEATS} warmup={WARMUP} (ms per round of B sessions x n tokens; median [min .. max])", flush=True)
for nm, n in SHAPES:
    ms = members[:nm]
    rows = [ids[ctx + s:ctx + s + n] for s in range(nm)]
    per = 4 if n == 1 else 2                       # members per group step: 4 x 1 or 2 x 2 rows
    bat = LlamaBatch(ms)
    grps = [(LlamaGroup(ms[i:i + per]), rows[i:i + per]) for i in range(0, nm, per)]
    tb, tg, ts = [], [], []
    for _ in range(REPEATS):
        tb.append(timed(leg_batch, bat, ms, rows))
        tg.append(timed(leg_group, grps, ms, rows) if not BATCH_ONLY else float("nan"))
        ts.append(timed(leg_single, ms, rows) if not BATCH_ONLY else float("nan"))
    bat.close()
    for g, _ in grps:
        g.close()
    b, g, s = (float(np.median(v)) for v in (tb, tg, ts))
    print(f"shape {nm}x{n}: batch step {mmm(tb)}   {len(grps)} group steps {mmm(tg)}   {nm} single steps {mmm(ts)}"
          f"   batch / group = {b / g:.3f}   batch / single = {b / s:.3f}   per session {b / nm * 1e3:.1f} us", flush=True)
