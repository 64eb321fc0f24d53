"""Tokens per second of scoring at Llama-3.2-1B dims (random-init weights), per weight format:
  * leg "score":      LlamaForAlternatingCodeChannels.score on 2048-token windows (rca_lm_score: head on the 128-token tiles, row
                      reduction on the device, one download of n small rows);
  * leg "logits_all": get_logprobs on a logits_all handle, the only per-position route before rca_lm_score (2-token decode passes,
                      every [n, vocab] row to the host, log-softmax in numpy).  Meant to be run against the PARENT commit's library,
                      built apart and selected with RCA_LIB_PATH as scripts/ab_logits.py does.
Three timed runs per leg and format after one warm-up, each leg in a child process of its own (one library per process).

    python scripts/lm_score_timing.py --parent_lib /path/to/parent/librca_hip.so --out profiles/r12/lm_score.txt [--quality]
    python scripts/lm_score_timing.py --leg score --formats bf16 q8_0            (one leg, this process, stdout)

--quality adds a SMOKE RUN of the quality tool (realtime_codec_agent_amd.lm_quality.score_streams) per format against the f16 model
on a synthetic id stream: random-init weights and random ids, so the numbers only show that the tool runs."""
import argparse
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FORMATS = ("bf16", "f16", "q8_0", "q4_k", "q5_k", "q4_0")
WINDOW = 2048
LOGITS_ALL_TOKENS = 512     # scored tokens of the logits_all leg: every row is 1 MB on the host (the rate is per token)


def _ids(n, seed=5):
    import numpy as np
    return np.random.default_rng(seed).integers(128266, 259338, n).astype(np.int32)


def leg_score(formats, quality):
    from realtime_codec_agent_amd import lm_quality
    from realtime_codec_agent_amd.llm import LlamaForAlternatingCodeChannels, LMConfig
    cfg = LMConfig.llama_3_2_1b()
    ids = _ids(4 * WINDOW)
    base = None
    for fmt in formats:
        llm = LlamaForAlternatingCodeChannels(model_path="random:1b", config=cfg, n_ctx=WINDOW, random_seed=0, device=0, weight_format=fmt)
        win = ids[:WINDOW].tolist()
        llm.score(win)                                  # warm-up: scratch allocation, one-time attribute calls
        rates = []
        for _ in range(3):
            llm.reset()
            t0 = time.perf_counter()
            llm.score(win)
            rates.append(WINDOW / (time.perf_counter() - t0))
        llm.reset()
        t0 = time.perf_counter()
        llm.eval(win)
        t_eval = time.perf_counter() - t0
        print(f"score       {fmt:5s} route {llm.prefill_route():8s} window {WINDOW}: " + " ".join(f"{r:9.0f}" for r in rates)
              + f" tok/s   (plain eval of the window: {WINDOW / t_eval:9.0f} tok/s)", flush=True)
        if quality:
            if base is None:
                base = LlamaForAlternatingCodeChannels(model_path="random:1b", config=cfg, n_ctx=WINDOW, random_seed=0, device=0, weight_format="f16")
            rep = lm_quality.score_streams(llm, [ids], WINDOW, WINDOW // 2, base=base)
            print(f"quality     {fmt:5s} vs f16 (SMOKE RUN: random-init weights, random ids): ppl {rep['ppl']:.1f} +- {rep['ppl_se']:.1f}, "
                  f"base ppl {rep['base_ppl']:.1f}, mean KL {rep['kl_mean']:.3e} +- {rep['kl_se']:.1e}, p99 KL {rep['kl_p99']:.3e}, "
                  f"top-1 agreement {100 * rep['top1_agreement']:.2f} %, {rep['n_scored']} positions", flush=True)
        llm.close()
    if base is not None:
        base.close()


def leg_logits_all(formats):
    from realtime_codec_agent_amd import _native
    from realtime_codec_agent_amd.llm import LlamaForAlternatingCodeChannels, LMConfig
    cfg = LMConfig.llama_3_2_1b()
    ids = _ids(WINDOW)
    n = LOGITS_ALL_TOKENS
    ctx, inp = ids[:WINDOW - n].tolist(), ids[WINDOW - n:].tolist()
    print(f"library {_native.LIB_PATH}", flush=True)
    for fmt in formats:
        llm = LlamaForAlternatingCodeChannels(model_path="random:1b", config=cfg, n_ctx=WINDOW, random_seed=0, device=0, weight_format=fmt,
                                              logits_all=True)
        llm.get_logprobs(ctx, inp[:64])                 # warm-up
        rates = []
        for _ in range(3):
            t0 = time.perf_counter()
            llm.get_logprobs(ctx, inp)
            rates.append(n / (time.perf_counter() - t0))
        # the context of WINDOW - n tokens is a plain prefill inside get_logprobs: its share of the time is charged to the n scored tokens
        print(f"logits_all  {fmt:5s} get_logprobs of {n} tokens behind a {WINDOW - n}-token context: " + " ".join(f"{r:9.0f}" for r in rates) + " tok/s", flush=True)
        llm.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--leg", choices=("score", "logits_all"), default=None)
    ap.add_argument("--formats", nargs="+", default=list(FORMATS))
    ap.add_argument("--quality", action="store_true")
    ap.add_argument("--parent_lib", default=None, help="the parent commit's library for the logits_all leg (RCA_LIB_PATH of that child)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.leg == "score":
        return leg_score(a.formats, a.quality)
    if a.leg == "logits_all":
        return leg_logits_all(a.formats)
    if not a.parent_lib or not os.path.exists(a.parent_lib):
        sys.exit("--parent_lib: build the parent commit's library apart and name it here (or run one --leg)")
    out = []
    me = [sys.executable, os.path.abspath(__file__), "--formats"] + a.formats
    for leg, env in (("score", {}), ("logits_all", {"RCA_LIB_PATH": os.path.abspath(a.parent_lib)})):
        cmd = me + ["--leg", leg] + (["--quality"] if a.quality and leg == "score" else [])
        p = subprocess.run(cmd, env={**os.environ, **env}, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=900)
        out.append(p.stdout)
        print(p.stdout, flush=True)
        if p.returncode != 0:
            sys.exit(f"leg {leg} failed with status {p.returncode}")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("".join(out))


if __name__ == "__main__":
    main()
