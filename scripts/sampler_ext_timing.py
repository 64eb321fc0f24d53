"""The single 2-token LM step (graph replay, 1B dims, random-init weights) under the sampler's routes: the default serial chain
(top_k = 100), the whole-vocabulary sampler (top_k = 0), the serial chain with typical_p = 0.5, and mirostat v2.
Usage: sampler_ext_timing.py [steps] [ctx ...]    (default 200 steps at 2200 and 6600 tokens of context)
One line per (context, mode); run under rocprofv3 --kernel-trace --stats for the per-kernel durations of the sampler's launches."""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from realtime_codec_agent_amd.llm import LlamaForAlternatingCodeChannels, LMConfig

steps = int(sys.argv[1]) if len(sys.argv) > 1 else 200
ctxs = [int(a) for a in sys.argv[2:]] or [2200, 6600]
MODES = {
    "default top_k=100": dict(top_k=100),
    "whole vocabulary top_k=0": dict(top_k=0),
    "typical_p=0.5 top_k=100": dict(top_k=100, typical_p=0.5),
    "mirostat v2 tau=5 eta=0.1": dict(top_k=100, mirostat_mode=2, mirostat_tau=5.0, mirostat_eta=0.1),
}
cfg = LMConfig.llama_3_2_1b()
llm = LlamaForAlternatingCodeChannels(model_path="random:1b", config=cfg, n_ctx=16384, device=0, weight_format=os.environ.get("RCA_LM_FORMAT"))
rng = np.random.default_rng(0)
ids = rng.integers(128266, 259338, max(ctxs) + 2).tolist()
llm.set_graphs(True)
llm.set_sampler_extensions(True)
done = 0
for ctx in sorted(ctxs):
    llm.eval(ids[done:ctx]); llm.sync(); done = ctx
    for name, kw in MODES.items():
        llm.init_sampler_for_generate(top_p=1.0, min_p=0.0, temp=1.0, seed=42, **kw)
        for _ in range(5):
            llm.n_tokens = ctx; llm.step(ids[ctx:ctx + 2])
        llm.sync(); t0 = time.perf_counter()
        for _ in range(steps):
            llm.n_tokens = ctx; llm.step(ids[ctx:ctx + 2])
        llm.sync(); dt = (time.perf_counter() - t0) / steps
        print(f"ctx={ctx} sampler={name}: step_ms={dt * 1e3:.3f}", flush=True)
    llm.n_tokens = ctx
