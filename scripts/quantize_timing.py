"""Seconds to quantise a Llama-3.2-1B-sized model on the card, and a SMOKE RUN of the quality tool over what comes out.

Weights: LMConfig.llama_3_2_1b() with seeded normal values (std 0.02) rounded to bf16 on the host -- no trained checkpoint.  Timed:
  * realtime_codec_agent_amd.quantize.quantize_weights(..., "q4_k_m") with rule="search" and with rule="minmax" (host bf16 -> blocks
    on the host: upload in slabs, the quantiser kernels, download), and the seconds spent inside rca_quantize_rows alone;
  * LlamaForAlternatingCodeChannels(weights=..., weight_format="q4_k"): the load-time path, which quantises and packs every matrix on
    every process start (its code is the parent commit's; the figure includes upload and packing, as a start does);
  * loading the ready-made q4_k_m blocks through weights=, and writing / reading the GGUF.
Quality (lm_quality.score_streams, 8192 random ids, 2048-token windows, mean KL against the f16 model of the same weights) for
weight_format="q4_k" (min / max at load; that path leaves the embedding table as supplied), the "q4_k" recipe (the table Q4_K too) with
min / max and with the search, and "q4_k_m" with the search.  A random model's logits are nearly flat: the KL figures show that the
pipeline runs and how the variants rank on noise, not what a trained model would lose.

    python scripts/quantize_timing.py [--out profiles/r23/quantize.txt] [--layers N]
"""
import argparse
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WINDOW = 2048


def _weights(cfg, seed=0, std=0.02):
    from realtime_codec_agent_amd.llm import f32_to_bf16_bits, lm_tensor_names
    rng = np.random.default_rng(seed)
    shapes = {"model.embed_tokens.weight": (cfg.vocab_size, cfg.hidden), "lm_head.weight": (cfg.vocab_size, cfg.hidden)}
    qkv = {"q_proj": cfg.n_heads * cfg.head_dim, "k_proj": cfg.n_kv_heads * cfg.head_dim, "v_proj": cfg.n_kv_heads * cfg.head_dim}
    out = {}
    for name in lm_tensor_names(cfg):
        leaf = name.split(".")[-2]
        if "norm" in name:
            out[name] = np.ones(cfg.hidden, np.float32)
            continue
        if name in shapes:
            shape = shapes[name]
        elif leaf in qkv:
            shape = (qkv[leaf], cfg.hidden)
        elif leaf == "o_proj":
            shape = (cfg.hidden, cfg.n_heads * cfg.head_dim)
        elif leaf in ("gate_proj", "up_proj"):
            shape = (cfg.ffn, cfg.hidden)
        else:
            shape = (cfg.hidden, cfg.ffn)
        out[name] = f32_to_bf16_bits(rng.standard_normal(shape, dtype=np.float32) * np.float32(std))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--layers", type=int, default=None, help="fewer layers than the 1B model's 16 (a quick look)")
    a = ap.parse_args()
    from realtime_codec_agent_amd import gguf, lm_quality
    from realtime_codec_agent_amd import quantize as Q
    from realtime_codec_agent_amd.llm import LlamaForAlternatingCodeChannels, LMConfig
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    cfg = LMConfig.llama_3_2_1b()
    if a.layers:
        cfg.n_layers = a.layers
    t0 = time.perf_counter()
    src = _weights(cfg)
    n_val = sum(v.size for v in src.values() if v.ndim == 2)
    say(f"model: {cfg.n_layers} layers, hidden {cfg.hidden}, ffn {cfg.ffn}, vocab {cfg.vocab_size}: {n_val / 1e9:.3f} G weights in matrices "
        f"(bf16, seeded normal std 0.02; generated on the host in {time.perf_counter() - t0:.1f} s)")
    Q.quantize_matrix(src["model.layers.0.self_attn.k_proj.weight"], "q4_k")          # first HIP call of the process: not timed
    made = {}
    say("quantise (host bf16 -> host blocks):            total s   inside rca_quantize_rows   bytes   bits per weight")
    for recipe, rule in (("q4_k_m", "search"), ("q4_k_m", "minmax"), ("q4_k", "search"), ("q4_k", "minmax"), ("q5_k_m", "search"), ("q8_0", "search")):
        t0 = time.perf_counter()
        q = Q.quantize_weights(cfg, src, recipe, rule=rule)
        dt = time.perf_counter() - t0
        nb = sum(v.raw.nbytes for v in q.values() if hasattr(v, "raw"))
        say(f"  {recipe:7s} rule={rule:7s}                        {dt:8.2f}   {sum(q.seconds.values()):8.2f}   {nb:12d}   {8.0 * nb / n_val:.3f}")
        if recipe in ("q4_k_m", "q4_k") and (recipe, rule) != ("q4_k_m", "minmax"):
            made[recipe, rule] = q
        del q
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "q4_k_m.gguf")
        t0 = time.perf_counter()
        n = Q.write_llama_gguf(path, cfg, made["q4_k_m", "search"])
        t1 = time.perf_counter()
        gguf.load_llama_gguf(path)
        say(f"write_llama_gguf q4_k_m: {n} bytes in {t1 - t0:.2f} s; gguf.load_llama_gguf of it: {time.perf_counter() - t1:.2f} s")

    def load(**kw):
        t0 = time.perf_counter()
        llm = LlamaForAlternatingCodeChannels(config=cfg, n_ctx=WINDOW, device=0, **kw)
        llm.sync()
        return llm, time.perf_counter() - t0

    base, dt = load(weights=src, weight_format="f16")
    say(f"process start, weights= bf16 with weight_format='f16' (the KL base): {dt:.2f} s")
    ids = np.random.default_rng(5).integers(128266, 259338, 4 * WINDOW).astype(np.int32)
    say(f"quality smoke run (RANDOM model, {len(ids)} random ids, windows of {WINDOW}, burn-in {WINDOW // 2}; mean KL(f16 || model)):")
    for label, kw in (("weight_format='q4_k' at load (min / max; table kept bf16)", dict(weights=src, weight_format="q4_k")),
                      ("quantize_weights 'q4_k' rule=minmax (table Q4_K too)", dict(weights=made["q4_k", "minmax"])),
                      ("quantize_weights 'q4_k' rule=search", dict(weights=made["q4_k", "search"])),
                      ("quantize_weights 'q4_k_m' rule=search", dict(weights=made["q4_k_m", "search"]))):
        llm, dt = load(**kw)
        rep = lm_quality.score_streams(llm, [ids], WINDOW, WINDOW // 2, base)
        say(f"  {label:58s} start {dt:6.2f} s  {llm.weight_bytes_per_step() / 1e9:.3f} GB / step  KL {rep['kl_mean']:.6f} +- {rep['kl_se']:.6f}  "
            f"p99 {rep['kl_p99']:.6f}  top-1 agreement {100 * rep['top1_agreement']:.2f} %  ppl {rep['ppl']:.1f} (base {rep['base_ppl']:.1f})")
        llm.close()
    base.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
