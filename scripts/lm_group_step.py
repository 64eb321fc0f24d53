"""Group step against single steps: ms per round of (a) n_members rca_lm_step calls, one per session, and (b) ONE rca_lm_group_step over the
same sessions, for the three group shapes (2 x 1, 2 x 2, 4 x 1 = members x tokens per member).  1B dims, random-init weights, one
parent handle and its weight-sharing twins, every member prefilled to CONTEXT tokens.
usage: lm_group_step.py CONTEXT STEPS        (RCA_LM_FORMAT=q8_0|q4_k|..., RCA_LM_ACT=q8_1 as scripts/lm_profile.py)
The two legs alternate inside one process (single, group, single, group, ... REPEATS times each), every timed leg is STEPS rounds
behind WARMUP untimed rounds of the same leg, and every round starts from the same context (n_tokens is put back).  Printed per shape:
the median over the repeats, the spread (min .. max) and the ratio of the medians."""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from realtime_codec_agent_amd.llm import LlamaForAlternatingCodeChannels, LlamaGroup, LMConfig

ctx = int(sys.argv[1]) if len(sys.argv) > 1 else 2200
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 200
REPEATS, WARMUP = 5, 10
cfg = LMConfig.llama_3_2_1b()
fmt = os.environ.get("RCA_LM_FORMAT")
act = os.environ.get("RCA_LM_ACT") or None
n_ctx = (ctx + 64 + 255) // 256 * 256
parent = LlamaForAlternatingCodeChannels(model_path="random:1b", config=cfg, n_ctx=n_ctx, device=0, weight_format=fmt, activation_format=act)
members = [parent] + [LlamaForAlternatingCodeChannels(n_ctx=n_ctx, share_weights_with=parent, device=0) for _ in range(3)]
rng = np.random.default_rng(0)
ids = rng.integers(128266, 259338, ctx + 8).tolist()
for s, m in enumerate(members):
    m.init_sampler_for_generate(top_k=100, top_p=1.0, min_p=0.0, temp=1.0, seed=42 + s)
    m.eval(ids[:ctx]); m.sync()


def leg_single(ms, rows, rounds):
    for _ in range(rounds):
        for m, r in zip(ms, rows):
            m.n_tokens = ctx
            m.step(r)


def leg_group(grp, ms, rows, rounds):
    for _ in range(rounds):
        for m in ms:
            m.n_tokens = ctx
        grp.step(rows)


def timed(f, *a):
    f(*a, WARMUP)
    t0 = time.perf_counter()
    f(*a, steps)
    return (time.perf_counter() - t0) / steps * 1e3


print(f"fmt={parent.weight_format} act={parent.activation_format} ctx={ctx} steps={steps} repeats={REPEATS} warmup={WARMUP} (ms per round; median [min .. max])")
for nm, n in ((2, 1), (2, 2), (4, 1)):
    ms = members[:nm]
    rows = [ids[ctx + s:ctx + s + n] for s in range(nm)]
    grp = LlamaGroup(ms)
    single, group = [], []
    for _ in range(REPEATS):
        single.append(timed(leg_single, ms, rows))
        group.append(timed(leg_group, grp, ms, rows))
    grp.close()
    sm, gm = float(np.median(single)), float(np.median(group))
    print(f"shape {nm}x{n}: {nm} single steps {sm:.3f} [{min(single):.3f} .. {max(single):.3f}]   group step {gm:.3f} [{min(group):.3f} .. {max(group):.3f}]"
          f"   group / single = {gm / sm:.3f}")
