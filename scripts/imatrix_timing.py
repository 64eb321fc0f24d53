"""Seconds of a q4_k_m quantise with and without an importance matrix at Llama-3.2-1B dims, and a SMOKE RUN of the quality tool over both.

Weights: scripts/quantize_timing.py's (LMConfig.llama_3_2_1b(), seeded normal values rounded to bf16 on the host -- no trained
checkpoint).  The importance matrix is either a GGUF imatrix file (--imatrix) or SEEDED: one vector exp(N(0, 1)) per projection input
(shared by attn_q / attn_k / attn_v and by ffn_gate / ffn_up, as a collected one is), written to a file and read back, so the run
goes through realtime_codec_agent_amd.imatrix as a user's would.  Timed: quantize_weights(..., "q4_k_m") without and with it
(rca_quantize_rows / rca_quantize_rows_w).  Then lm_quality.score_streams on 8192 random ids, mean KL against the f16 model, for both
results: a random model, random ids and -- unless --imatrix names a real one -- made-up weights, so the KL figures show that the chain
runs and say nothing about what a matrix collected on a corpus would gain on a trained checkpoint.  Not measured: a trained checkpoint.

    python scripts/imatrix_timing.py [--out profiles/r24/imatrix.txt] [--imatrix F.gguf] [--layers N]
"""
import argparse
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

WINDOW = 2048
SHARED = ((("attn_q", "attn_k", "attn_v"), "hidden"), (("attn_output",), "ao"), (("ffn_gate", "ffn_up"), "hidden"), (("ffn_down",), "ffn"))


def seeded_imatrix(cfg, seed=1, count=8192):
    from realtime_codec_agent_amd.imatrix import Imatrix
    rs = np.random.RandomState(seed)
    width = {"hidden": cfg.hidden, "ao": cfg.n_heads * cfg.head_dim, "ffn": cfg.ffn}
    out = Imatrix(datasets=[f"seeded exp(N(0, 1)), RandomState({seed})"], chunk_count=count // WINDOW, chunk_size=WINDOW)
    for l in range(cfg.n_layers):
        for names, k in SHARED:
            v = np.exp(rs.randn(width[k])) * count
            for n in names:
                out[f"blk.{l}.{n}.weight"] = (v, count)
    out["output.weight"] = (np.exp(rs.randn(cfg.hidden)) * count, count)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--imatrix", default=None, help="a GGUF imatrix file for this model's dims (default: a seeded one)")
    ap.add_argument("--layers", type=int, default=None, help="fewer layers than the 1B model's 16 (a quick look)")
    a = ap.parse_args()
    from quantize_timing import _weights
    from realtime_codec_agent_amd import imatrix as I
    from realtime_codec_agent_amd import lm_quality
    from realtime_codec_agent_amd import quantize as Q
    from realtime_codec_agent_amd.llm import LlamaForAlternatingCodeChannels, LMConfig
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    cfg = LMConfig.llama_3_2_1b()
    if a.layers:
        cfg.n_layers = a.layers
    src = _weights(cfg)
    n_val = sum(v.size for v in src.values() if v.ndim == 2)
    say(f"model: {cfg.n_layers} layers, hidden {cfg.hidden}, ffn {cfg.ffn}, vocab {cfg.vocab_size}: {n_val / 1e9:.3f} G weights in matrices "
        "(bf16, seeded normal std 0.02)")
    if a.imatrix:
        imx = I.read_imatrix_gguf(a.imatrix)
    else:
        with tempfile.TemporaryDirectory() as tmp:
            path = os.path.join(tmp, "seeded.gguf")
            nb = I.write_imatrix_gguf(path, seeded_imatrix(cfg))
            imx = I.read_imatrix_gguf(path)
            imx.file = "seeded"
        say(f"importance matrix: SEEDED, not collected ({imx.datasets[0]}; one vector per projection input): {len(imx)} entries, {nb} bytes as a file")
    Q.quantize_matrix(src["model.layers.0.self_attn.k_proj.weight"], "q4_k")          # first HIP call of the process: not timed
    made = {}
    say("quantize_weights 'q4_k_m' rule=search (host bf16 -> host blocks), two runs each:   total s   inside the quantiser   bytes")
    for _ in range(2):
        for label, kw in (("no importance matrix", {}), ("importance matrix", dict(imatrix=imx))):
            t0 = time.perf_counter()
            q = Q.quantize_weights(cfg, src, "q4_k_m", **kw)
            dt = time.perf_counter() - t0
            nb = sum(v.raw.nbytes for v in q.values() if hasattr(v, "raw"))
            say(f"  {label:24s}                                                          {dt:8.2f}   {sum(q.seconds.values()):8.2f}   {nb:12d}")
            made[label] = q
    ids = np.random.default_rng(5).integers(128266, 259338, 4 * WINDOW).astype(np.int32)
    base = LlamaForAlternatingCodeChannels(config=cfg, weights=src, n_ctx=WINDOW, device=0, weight_format="f16")
    say(f"SMOKE RUN of lm_quality (RANDOM model, {len(ids)} random ids, {'the file ' + a.imatrix if a.imatrix else 'SEEDED weights'}; windows of {WINDOW}, "
        f"burn-in {WINDOW // 2}; mean KL(f16 || model)): shows that the chain runs, no quality claim; a trained checkpoint: not measured")
    for label, q in made.items():
        m = LlamaForAlternatingCodeChannels(config=cfg, weights=q, n_ctx=WINDOW, device=0)
        rep = lm_quality.score_streams(m, [ids], WINDOW, WINDOW // 2, base)
        say(f"  q4_k_m, {label:24s} KL {rep['kl_mean']:.6f} +- {rep['kl_se']:.6f}  p99 {rep['kl_p99']:.6f}  top-1 agreement "
            f"{100 * rep['top1_agreement']:.2f} %  ppl {rep['ppl']:.1f} (base {rep['base_ppl']:.1f})")
        m.close()
    base.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
