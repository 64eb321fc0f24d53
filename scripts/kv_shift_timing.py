"""rca_lm_kv_remove alone at Llama-3.2-1B dimensions (random-init weights): HOST time of the call (a host clock around it; it returns
after its own stream synchronisation, so the figure holds the launches and the synchronisation, not the kernels alone) for the trims of a session with a 150-token header -- 2.2 k context with 550 positions removed, 6.6 k context with
1 650 removed -- the cache bytes it moves over that time, and, for information, max |dlogit| of a decode step on the shifted cache
against the same step on a cache recomputed from header + suffix.
RCA_LM_KV=q8_0: the same on a q8_0 cache with the shift allowed (kv_shift_requant=True: the moved keys are re-quantised).
usage: kv_shift_timing.py [repeats]"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from realtime_codec_agent_amd.llm import LlamaForAlternatingCodeChannels, LMConfig

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
cfg = LMConfig.llama_3_2_1b()
KV = os.environ.get("RCA_LM_KV") or None
llm = LlamaForAlternatingCodeChannels(model_path="random:1b", config=cfg, n_ctx=16384, random_seed=0, device=0,
                                      **(dict(kv_format=KV, kv_shift_requant=True) if KV == "q8_0" else dict(kv_format=KV)))
ids = np.random.default_rng(5).integers(128266, 259338, 7000).tolist()
row_bytes = llm.kv_bytes_per_position()                           # one position: K and V of every layer, fp16 rows or q8_0 blocks
print(f"KV cache {llm.kv_format}: {row_bytes} bytes per position")
header = 150
for n, cut in ((2200, 550), (6600, 1650)):
    llm.reset()
    llm.eval(ids[:n])
    llm.kv_remove(header, header + cut)                             # first call: staging allocation, code object load
    ms = []
    for _ in range(reps):
        llm.n_tokens = n                                            # the rows above n - cut are stale but still there: same work again
        llm.sync()
        t0 = time.perf_counter()
        llm.kv_remove(header, header + cut)
        ms.append((time.perf_counter() - t0) * 1e3)
    moved = n - header - cut
    med = float(np.median(ms))
    print(f"kv_remove at {n} tokens, [{header}, {header + cut}): {moved} rows moved in {-(-moved // 256) + 1} launches; host time median {med:.3f} ms "
          f"(min {min(ms):.3f}, max {max(ms):.3f}, {reps} calls); cache bytes read + written {2 * moved * row_bytes / 1e6:.1f} MB -> "
          f"{2 * moved * row_bytes / (med * 1e-3) / 1e9:.0f} GB/s over the HOST time of the call, launches and synchronisation included "
          f"({4 * moved * row_bytes / (med * 1e-3) / 1e9:.0f} GB/s counting the staging copy); kernel time alone: rocprofv3 --kernel-trace --stats on this script")
n, cut = 2200, 550
llm.reset()
llm.eval(ids[:n])
llm.kv_remove(header, header + cut)
llm.eval(ids[n:n + 2])
shifted = llm._scores[-1].copy()
llm.reset()
llm.eval(ids[:header] + ids[header + cut:n])
llm.eval(ids[n:n + 2])
fresh = llm._scores[-1].copy()
print(f"decode step after one trim ({n} tokens, {cut} removed): max |dlogit| shifted vs recomputed cache = {np.abs(shifted - fresh).max():.3e} "
      f"(max |logit| {np.abs(fresh).max():.2f}); argmax equal: {bool(shifted.argmax() == fresh.argmax())}")
