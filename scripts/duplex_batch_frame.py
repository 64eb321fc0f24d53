"""A tick of N duplex sessions: ms per tick as (a) ONE rca_duplex_batch_frame, (b) the unfused path -- N encode tails, one selection
frame (rca_lm_batch_frame_sel), N decode tails, N probes -- and (c) N rca_duplex_frame calls, for N in 4, 8, 16, 32, 64.  1B dims,
random-init weights (head rows outside the codec range zeroed), the default codec, one parent handle and its weight-sharing twins in ONE
batch of 64, every member at CONTEXT tokens, 4 steps per tick, the steady-state call shape (T 32000, F_ctx 96, 1440 samples), graphs on.
usage: duplex_batch_frame.py CONTEXT TICKS      (RCA_LM_FORMAT=q8_0|q4_k|... as scripts/lm_profile.py; RCA_LM_KV=q8_0: q8_0 KV caches)
The three legs alternate inside one process (a, b, c, a, ... REPEATS times each); every timed leg is TICKS ticks behind WARMUP untimed
ticks of the same leg, and every tick starts from the same context (n_tokens is put back).  Printed per N: the median over the repeats
with the spread per leg, a / c and a / b.  Then: the session count from which (a) is faster than (c); the host time of stacking N PCM
windows into one array (the copy into pinned memory is inside (a)); and, at N = 12, a steady tick next to the tick straight after a
member's rca_lm_swap_kv and the tick after the selection shrinks to 9 inside the class, with the captures each made."""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from realtime_codec_agent_amd.audio_tokenizer import AudioTokenizer
from realtime_codec_agent_amd.llm import LlamaBatch, LlamaForAlternatingCodeChannels, LMConfig
from realtime_codec_agent_amd.tokenizer import CodecTokenizer

ctx = int(sys.argv[1]) if len(sys.argv) > 1 else 2200
ticks = int(sys.argv[2]) if len(sys.argv) > 2 else 10
REPEATS, WARMUP, N_STEPS, NB = 3, 2, 4, 64
T, F_CTX, N_SAMPLES = 32000, 96, 1440
SHAPES = (4, 8, 16, 32, 64)
if os.environ.get("RCA_DUPLEX_SHAPES"):   # e.g. "64": a subset, for a short run
    SHAPES = tuple(int(v) for v in os.environ["RCA_DUPLEX_SHAPES"].split(","))
cfg = LMConfig.llama_3_2_1b()
fmt = os.environ.get("RCA_LM_FORMAT")
at = AudioTokenizer(codec_model="MagiCodec-50Hz-Base", device=None)
hip = at.codec_model.hip
tok = CodecTokenizer(codebook_size=at.codebook_size, unicode_offset=at.unicode_offset)
base, ncb = tok.codec_vocab_start, at.codebook_size
n_ctx = (ctx + 64 + 255) // 256 * 256
kvf = os.environ.get("RCA_LM_KV") or None    # "q8_0": quantised KV cache; the twins inherit it
parent = LlamaForAlternatingCodeChannels(model_path="random:1b", config=cfg, n_ctx=n_ctx, device=0, weight_format=fmt, **({"kv_format": kvf} if kvf else {}))
if kvf:
    print(f"kv_format {parent.kv_format}: {parent.kv_bytes_per_position()} bytes per cached position")
parent.mask_head_rows(0, base)
parent.mask_head_rows(len(tok), parent.n_vocab())
members = [parent] + [LlamaForAlternatingCodeChannels(n_ctx=n_ctx, share_weights_with=parent, device=0) for _ in range(NB - 1)]
shadow = LlamaForAlternatingCodeChannels(n_ctx=n_ctx, share_weights_with=parent, device=0)
rng = np.random.default_rng(0)
ids = rng.integers(base, base + ncb, ctx + 80).tolist()
parent.eval(ids[:ctx]); parent.sync()
for s, m in enumerate(members):
    m.init_sampler_for_generate(top_k=100, top_p=1.0, min_p=0.0, temp=1.0, seed=42 + s)
    if s:
        m.copy_kv_from(parent, ctx); m.sync()
windows = [(rng.standard_normal(T) * 0.1).astype(np.float32) for _ in range(NB)]
ctxs = [rng.integers(0, ncb, F_CTX).astype(np.int64) for _ in range(NB)]
pairs = [ids[ctx + s:ctx + s + 2] for s in range(NB)]
end_audio = tok.convert_tokens_to_ids("<|end_audio|>")
bat = LlamaBatch(members)


def put_back(sel):
    for s in sel:
        members[s].n_tokens = ctx


def tick_a(sel):
    put_back(sel)
    return bat.duplex_frame(hip, sel, np.stack([windows[s] for s in sel]), np.stack([ctxs[s] for s in sel]), N_STEPS, N_SAMPLES, base, -1,
                            [end_audio] * len(sel), [pairs[s] for s in sel])


def tick_b(sel):
    put_back(sel)
    users = [[base + int(c) for c in hip.encode_tail(windows[s][None], N_STEPS)[0]] for s in sel]
    toks, probs = bat.frame([pairs[s] for s in sel], users, -1, probe_ids=[end_audio] * len(sel), members=sel)
    for k, s in enumerate(sel):
        hip.decode_tail(np.concatenate([ctxs[s], np.array([t - base for t in toks[k]], dtype=np.int64)])[None], N_SAMPLES)
    return toks


def tick_c(sel):
    put_back(sel)
    for s in sel:
        members[s].duplex_frame(hip, windows[s], ctxs[s], N_STEPS, N_SAMPLES, base, -1, end_audio, pairs[s])


def timed(f, sel, n=None):
    for _ in range(WARMUP):
        f(sel)
    t0 = time.perf_counter()
    for _ in range(n or ticks):
        f(sel)
    return (time.perf_counter() - t0) / (n or ticks) * 1e3


def mmm(v):
    return f"{float(np.median(v)):.3f} [{min(v):.3f} .. {max(v):.3f}]"


print(f"fmt={parent.weight_format} ctx={ctx} ticks={ticks} repeats={REPEATS} warmup={WARMUP} n_steps={N_STEPS} T={T} F_ctx={F_CTX} n_samples={N_SAMPLES}"
      f" (ms per tick of N sessions; median [min .. max])", flush=True)
med = {}
for nm in SHAPES:
    sel = list(range(nm))
    ta, tb, tc = [], [], []
    for _ in range(REPEATS):
        ta.append(timed(tick_a, sel)); tb.append(timed(tick_b, sel)); tc.append(timed(tick_c, sel))
    a, b, c = (float(np.median(v)) for v in (ta, tb, tc))
    med[nm] = (a, b, c)
    print(f"N={nm:2d}: (a) one duplex batch frame {mmm(ta)}   (b) unfused {mmm(tb)}   (c) {nm} duplex frames {mmm(tc)}   a / c = {a / c:.3f}   a / b = {a / b:.3f}"
          f"   per session {a / nm * 1e3:.0f} us", flush=True)
wins = [nm for nm in SHAPES if med[nm][0] < med[nm][2]]
print(f"(a) faster than (c) from N = {min(wins) if wins else 'never (up to 64)'} on (of {SHAPES}); 64 sessions: {med[64][0]:.2f} ms of an 80 ms tick", flush=True)
t0 = time.perf_counter()
for _ in range(20):
    np.stack([windows[s] for s in range(NB)])
print(f"host: stacking 64 x {T} floats ({64 * T * 4 / 1e6:.1f} MB): {(time.perf_counter() - t0) / 20 * 1e3:.3f} ms per tick", flush=True)
# a steady tick, the tick after a member's swap_kv, the tick after the selection size changes inside the class
sel12, sel9 = list(range(12)), list(range(9))
steady = timed(tick_a, sel12)
c0 = bat.captures()
shadow.reset(); shadow.copy_kv_from(members[2], ctx); members[2].swap_kv(shadow)
t0 = time.perf_counter(); tick_a(sel12); after_swap = (time.perf_counter() - t0) * 1e3
c1 = bat.captures()
t0 = time.perf_counter(); tick_a(sel9); after_resize = (time.perf_counter() - t0) * 1e3
c2 = bat.captures()
print(f"N=12 steady tick {steady:.3f} ms; straight after rca_lm_swap_kv of member 2: {after_swap:.3f} ms ({c1 - c0} captures); "
      f"then 9 of the class: {after_resize:.3f} ms ({c2 - c1} captures)", flush=True)
bat.close()
