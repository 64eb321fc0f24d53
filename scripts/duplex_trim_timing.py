"""What a trim frame spends where.  --trim-mode recompute (default): wraps KVShadow.finish / plan and the twin's eval_async / the swap
with host timers (each followed by a stream sync, so the numbers are the pieces' own durations, not their overlap).  --trim-mode
shift: the session trims by context shift (RealtimeAgent(kv_trim_mode="shift")) and the timer sits around llm.kv_remove, which returns
after its own synchronisation.  Either way the last line summarises the frames after the first ten.
usage: duplex_trim_timing.py [secs] [--trim-mode {recompute,shift}]"""
import argparse, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from realtime_codec_agent_amd.duplex_bench import synth_signal, session_resources_kwargs
from realtime_codec_agent_amd.realtime_agent_config import RealtimeAgentConfig
from realtime_codec_agent_amd.realtime_agent_resources import RealtimeAgentResources
from realtime_codec_agent_amd.realtime_agent_v2 import RealtimeAgent
from realtime_codec_agent_amd import kv_shadow

ap = argparse.ArgumentParser()
ap.add_argument("secs", nargs="?", type=float, default=125.0)
ap.add_argument("--trim-mode", choices=("recompute", "shift"), default="recompute")
args = ap.parse_args()
secs = args.secs
res = RealtimeAgentResources(**session_resources_kwargs(0, 16384, None))
config = RealtimeAgentConfig(chunk_size_secs=0.08, use_whisper=False, top_k=100, temperature=1.0, seed=42, max_context_secs=80.0,
                             trim_by_secs=20.0, force_trans_after_inactivity_secs=0.0, force_response_after_inactivity_secs=0.0)
log = []
orig_finish, orig_plan = kv_shadow.KVShadow.finish, kv_shadow.KVShadow.plan
def timed_finish(self, input_ids, src_pos, prefix_len, end):
    twin, llm = self.twin, self.llm
    ev, sw = twin.eval_async, llm.swap_kv
    t = {}
    def ev2(toks):
        t0 = time.perf_counter(); ev(toks); t["enqueue_ms"] = (time.perf_counter() - t0) * 1e3; t["rest"] = len(toks)
        t0 = time.perf_counter(); twin.sync(); t["rest_gpu_ms"] = (time.perf_counter() - t0) * 1e3
    def sw2(other):
        t0 = time.perf_counter(); sw(other); t["swap_ms"] = (time.perf_counter() - t0) * 1e3
    twin.eval_async, llm.swap_kv = ev2, sw2
    t0 = time.perf_counter()
    try:
        r = orig_finish(self, input_ids, src_pos, prefix_len, end)
    finally:
        twin.eval_async, llm.swap_kv = ev, sw
    t["finish_ms"] = (time.perf_counter() - t0) * 1e3
    log.append(("finish", t))
    return r
def timed_plan(self, prefix_len, src_pos):
    t0 = time.perf_counter(); orig_plan(self, prefix_len, src_pos); self.twin.sync()
    log.append(("plan", {"plan_ms": (time.perf_counter() - t0) * 1e3, "prefix": prefix_len}))
kv_shadow.KVShadow.finish, kv_shadow.KVShadow.plan = timed_finish, timed_plan
if args.trim_mode == "shift":
    llm = res.llm
    orig_remove = llm.kv_remove
    def timed_remove(p0, p1):
        n = llm.n_tokens
        llm.sync()
        t0 = time.perf_counter(); orig_remove(p0, p1)
        log.append(("kv_remove", {"kv_remove_ms": (time.perf_counter() - t0) * 1e3, "p0": p0, "p1": p1, "n_tokens_before": n, "rows_moved": n - p1}))
    llm.kv_remove = timed_remove
agent = RealtimeAgent(resources=res, config=config, kv_trim_mode=args.trim_mode)
sig = synth_signal(int(secs * 16000), 0)
cs = agent.chunk_size_samples
frame_ms, trim_frames = [], []
for i, s in enumerate(range(0, len(sig) - cs + 1, cs)):
    n0 = len(log)
    last_trim = agent.trim_to_secs
    t0 = time.perf_counter()
    agent.process_audio(sig[s:s + cs])
    dt = (time.perf_counter() - t0) * 1e3
    frame_ms.append(dt)
    if agent.trim_to_secs != last_trim:
        trim_frames.append((i, dt))
    if len(log) > n0:
        print(f"frame {i} ({i * 0.08:.2f} s) {dt:.2f} ms: " + "; ".join(f"{k} {({a: round(b, 2) for a, b in v.items()})}" for k, v in log[n0:]))
f = np.asarray(frame_ms[10:])
print(f"summary trim_mode={args.trim_mode} kv_shadow={agent.kv_shadow_active} frames={f.size} p50={np.percentile(f, 50):.2f} p99={np.percentile(f, 99):.2f} "
      f"max={f.max():.2f} ms; trim frames: " + ", ".join(f"{i} ({i * 0.08:.2f} s) {dt:.2f} ms" for i, dt in trim_frames))
