"""Perplexity and KL divergence of a model (file, weight format, activation format) on token streams: what llama.cpp's
llama-perplexity and its --kl-divergence mode report, computed with LlamaForAlternatingCodeChannels.score (the logits stay on the
device; rca_lm_score).

    python -m realtime_codec_agent_amd.lm_quality --model M [--base B] --ids PATH [--window 2048] [--burn_in N] [--weight_format F]
                                                  [--activation_format A] [--base_weight_format F] [--kv_format K] [--base_kv_format K] [--json]

PATH is a .npy of int32 token ids or a directory of them (one stream per file).  Every stream is cut into consecutive windows of
`window` tokens; each window is scored on a reset context and its first `burn_in` positions (default: half the window, as
llama-perplexity discards the first half of a chunk) are discarded, as is the last position of a window (nothing to predict).  A last
window too short to score anything is dropped.  Reported: perplexity = exp(mean -logprob) with its standard error (delta method:
ppl * se(mean)), and against the base the mean KL(P_base || P) with its standard error, the 99th percentile of the KL and the top-1
agreement.  The base defaults to the same file as --model (so --weight_format q4_0 --base_weight_format f16 compares two formats
of one checkpoint); with neither --base nor --base_weight_format only the perplexity is computed.

The window bookkeeping (plan_windows, scored_mask, aggregate) is pure numpy and is tested without a GPU.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
from typing import Dict, List, Optional, Sequence

import numpy as np

WINDOW_DTYPE = np.dtype([("stream", np.int64), ("start", np.int64), ("length", np.int64), ("first_scored", np.int64)])


def plan_windows(stream_lengths: Sequence[int], window: int, burn_in: int) -> np.ndarray:
    """The table of windows: stream index, first token, tokens, first scored position (relative to the window).  Position i of a
    window is scored against token i + 1, so a window of `length` tokens scores positions first_scored .. length - 2."""
    if window < 2:
        raise ValueError(f"window {window}: a window needs at least two tokens")
    if not 0 <= burn_in < window - 1:
        raise ValueError(f"burn_in {burn_in} leaves nothing to score in a window of {window}")
    rows = []
    for s, n in enumerate(stream_lengths):
        for start in range(0, int(n), window):
            length = min(window, int(n) - start)
            if length - 1 > burn_in:
                rows.append((s, start, length, burn_in))
    return np.array(rows, dtype=WINDOW_DTYPE)


def scored_mask(length: int, first_scored: int) -> np.ndarray:
    """which of a window's `length` positions count"""
    m = np.zeros(int(length), bool)
    m[int(first_scored):int(length) - 1] = True
    return m


def _mean_se(x: np.ndarray):
    n = x.size
    mean = float(np.mean(x)) if n else float("nan")
    se = float(np.std(x, ddof=1) / np.sqrt(n)) if n > 1 else float("nan")
    return mean, se


def aggregate(logprob: np.ndarray, kl: Optional[np.ndarray] = None, argmax: Optional[np.ndarray] = None,
              base_argmax: Optional[np.ndarray] = None, base_logprob: Optional[np.ndarray] = None) -> Dict[str, float]:
    """The report over the scored positions (already masked and concatenated)."""
    logprob = np.asarray(logprob, np.float64)
    if logprob.size == 0:
        raise ValueError("no scored position")
    if not np.all(np.isfinite(logprob)):
        raise ValueError("a scored position has no finite logprob (NaN logits, or a target the model gives no mass)")
    nll, nll_se = _mean_se(-logprob)
    out = {"n_scored": int(logprob.size), "nll": nll, "nll_se": nll_se, "ppl": float(np.exp(nll)), "ppl_se": float(np.exp(nll) * nll_se)}
    if base_logprob is not None:
        bn, bse = _mean_se(-np.asarray(base_logprob, np.float64))
        out.update(base_ppl=float(np.exp(bn)), base_ppl_se=float(np.exp(bn) * bse))
    if kl is not None:
        kl = np.asarray(kl, np.float64)
        m, se = _mean_se(kl)
        out.update(kl_mean=m, kl_se=se, kl_p99=float(np.percentile(kl, 99)), kl_max=float(np.max(kl)))
    if argmax is not None and base_argmax is not None:
        out["top1_agreement"] = float(np.mean(np.asarray(argmax) == np.asarray(base_argmax)))
    return out


def load_streams(path: str) -> List[np.ndarray]:
    files = [path] if os.path.isfile(path) else sorted(os.path.join(path, f) for f in os.listdir(path) if f.endswith(".npy"))
    if not files:
        raise ValueError(f"{path}: no .npy file")
    out = []
    for f in files:
        a = np.load(f)
        if a.ndim != 1 or not np.issubdtype(a.dtype, np.integer):
            raise ValueError(f"{f}: expected a 1-D integer array of token ids, got {a.dtype} {a.shape}")
        out.append(a.astype(np.int32))
    return out


def score_streams(llm, streams: Sequence[np.ndarray], window: int, burn_in: int, base=None) -> Dict[str, float]:
    """Score every window of every stream on a reset context and aggregate."""
    table = plan_windows([len(s) for s in streams], window, burn_in)
    cols: Dict[str, List[np.ndarray]] = {k: [] for k in ("logprob", "kl", "argmax", "base_argmax", "base_logprob")}
    for w in table:
        ids = streams[int(w["stream"])][int(w["start"]):int(w["start"]) + int(w["length"])].tolist()
        llm.reset()
        if base is not None:
            base.reset()
        r = llm.score(ids, base=base)
        keep = scored_mask(int(w["length"]), int(w["first_scored"]))
        cols["logprob"].append(r.logprob[keep])
        cols["argmax"].append(r.argmax[keep])
        if base is not None:
            for k in ("kl", "base_argmax", "base_logprob"):
                cols[k].append(getattr(r, k)[keep])
    cat = lambda k: np.concatenate(cols[k]) if cols[k] else None
    if not cols["logprob"]:
        raise ValueError(f"no window of more than burn_in + 1 = {burn_in + 1} tokens")
    out = aggregate(cat("logprob"), cat("kl"), cat("argmax"), cat("base_argmax"), cat("base_logprob"))
    out.update(n_windows=int(len(table)), window=int(window), burn_in=int(burn_in))
    return out


def format_report(rep: Dict[str, float]) -> str:
    lines = [f"windows {rep['n_windows']} x {rep['window']} tokens, burn-in {rep['burn_in']}, scored positions {rep['n_scored']}",
             f"perplexity      {rep['ppl']:.4f} +- {rep['ppl_se']:.4f}"]
    if "kl_mean" in rep:
        lines += [f"base perplexity {rep['base_ppl']:.4f} +- {rep['base_ppl_se']:.4f}",
                  f"mean KL(base || model)  {rep['kl_mean']:.6f} +- {rep['kl_se']:.6f}",
                  f"99th percentile KL      {rep['kl_p99']:.6f}   (max {rep['kl_max']:.6f})",
                  f"top-1 agreement         {100.0 * rep['top1_agreement']:.3f} %"]
    return "\n".join(lines)


def main(argv: Optional[Sequence[str]] = None) -> int:
    ap = argparse.ArgumentParser(prog="python -m realtime_codec_agent_amd.lm_quality", description=__doc__.split("\n\n")[0])
    ap.add_argument("--model", required=True)
    ap.add_argument("--base", default=None, help="the reference model (default: --model, when --base_weight_format is given)")
    ap.add_argument("--ids", required=True, help=".npy of int32 token ids, or a directory of them")
    ap.add_argument("--window", type=int, default=2048)
    ap.add_argument("--burn_in", type=int, default=None, help="positions discarded at the head of every window (default: window // 2)")
    ap.add_argument("--weight_format", default=None, help="load-time format of the scored model: bf16, q8_0, f16, q4_k, q5_k, q4_0, q4_1 or iq4_nl (default: as the file supplies it)")
    ap.add_argument("--activation_format", default=None)
    ap.add_argument("--base_weight_format", default=None)
    ap.add_argument("--kv_format", default=None, help="KV cache of the scored model: f16 (default) or q8_0")
    ap.add_argument("--base_kv_format", default=None, help="KV cache of the reference model; given alone it makes --model its own reference")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--json", action="store_true", help="print the report as one JSON object")
    a = ap.parse_args(argv)
    from .llm import LlamaForAlternatingCodeChannels
    streams = load_streams(a.ids)
    burn_in = a.window // 2 if a.burn_in is None else a.burn_in
    llm = LlamaForAlternatingCodeChannels(model_path=a.model, n_ctx=a.window, device=a.device, weight_format=a.weight_format,
                                          activation_format=a.activation_format, kv_format=a.kv_format)
    base = None
    if a.base is not None or a.base_weight_format is not None or a.base_kv_format is not None:
        base = LlamaForAlternatingCodeChannels(model_path=a.base or a.model, n_ctx=a.window, device=a.device,
                                               weight_format=a.base_weight_format if (a.base is not None or a.base_weight_format is not None) else a.weight_format,
                                               kv_format=a.base_kv_format)
    try:
        rep = score_streams(llm, streams, a.window, burn_in, base)
    finally:
        llm.close()
        if base is not None:
            base.close()
    rep.update(model=a.model, base=(a.base or a.model) if base is not None else None, weight_format=llm.weight_format,
               activation_format=llm.activation_format, base_weight_format=base.weight_format if base is not None else None,
               kv_format=llm.kv_format, base_kv_format=base.kv_format if base is not None else None)
    print(json.dumps(rep) if a.json else format_report(rep))
    return 0


if __name__ == "__main__":
    sys.exit(main())
