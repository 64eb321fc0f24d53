"""What collecting an importance matrix costs at Llama-3.2-1B dims (random-init weights, random ids), and that nothing else moved.

  * leg "rate":  tokens per second of imatrix.collect at chunk 512 and 1024 (16 / 8 chunks, three timed runs after a warm-up), against the
                 same chunks walked with reset() + eval_async() on the same build -- that call's code is the parent commit's: the
                 difference is the collection launches, the final norm over every row and one synchronisation per chunk.
  * leg "trace": from rocprofv3 kernel traces, the duration of ONE collection launch (lm_imatrix_kernel, 1024 live rows) at K = 2048
                 and K = 8192 through rca_lm_imatrix_rows_tap, for this build and -- with --parent_lib -- for the parent commit's
                 kernel on the same planes; and inside two collecting passes of 1024 tokens, the launches' count, average and share
                 of the pass's kernel time -- with --old_kernel_lib also for a build of this tree that has the parent commit's
                 kernel body in place of the rewrite (the parent itself has no collecting pass), and the rates under that build.
  * leg "ab":    with --parent_lib, scripts/ab_logits.py per weight format under both libraries (identical lines of 80) and
                 scripts/lm_profile.py's 2-token step time under both.
  * --smoke:     a SMOKE RUN of the chain on seeded normal weights: collect on them, q4_k_m with and without the collected matrix,
                 lm_quality against f16 (scripts/imatrix_timing.py --imatrix).  A random model and random ids: it shows that the
                 chain runs and makes no quality claim.  A trained checkpoint: not measured.
Every leg is a child process (one library per process); a leg that fails ends the run.

    python scripts/imatrix_collect_timing.py --parent_lib /path/to/parent/librca_hip.so [--old_kernel_lib /path/to/lib.so] --out profiles/r25/imatrix_collect.txt [--smoke]
"""
import argparse
import collections
import csv
import glob
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

FORMATS = ("bf16", "f16", "q8_0", "q4_k", "q5_k", "q4_0")
TOKENS = 8192


def _llm(n_ctx):
    from realtime_codec_agent_amd.llm import LlamaForAlternatingCodeChannels, LMConfig
    return LlamaForAlternatingCodeChannels(model_path="random:1b", config=LMConfig.llama_3_2_1b(), n_ctx=n_ctx, random_seed=0, device=0)


def _ids(n, seed=5):
    import numpy as np
    return np.random.default_rng(seed).integers(128266, 259338, n).astype(np.int32)


# ------------------------------------------------------------------------------------------------------------------ the legs (children)
def leg_rate():
    from realtime_codec_agent_amd import imatrix as I
    ids = _ids(TOKENS)
    llm = _llm(1024)
    for chunk in (512, 1024):
        pieces = [ids[o:o + chunk].tolist() for o in range(0, TOKENS, chunk)]

        def walk():
            for p in pieces:
                llm.reset()
                llm.eval_async(p)
            llm.sync()

        I.collect(llm, [ids[:2 * chunk]], chunk=chunk)
        walk()
        for leg, run in (("collect", lambda: I.collect(llm, [ids], chunk=chunk)), ("reset + eval_async", walk)):
            rates = []
            for _ in range(3):
                t0 = time.perf_counter()
                run()
                rates.append(TOKENS / (time.perf_counter() - t0))
            print(f"  chunk {chunk:4d}, {len(pieces):2d} chunks, {leg:20s} " + "  ".join(f"{r:9.0f}" for r in rates) + f"   tokens / s (best {max(rates):.0f})", flush=True)
    llm.close()


def leg_trace_tap():
    """the kernel alone: 6 launches per K over 1024 live rows (runs under either library)"""
    import numpy as np
    from realtime_codec_agent_amd.llm import LlamaForAlternatingCodeChannels, LMConfig
    llm = LlamaForAlternatingCodeChannels(model_path="random:tap", config=LMConfig(vocab_size=1000, hidden=256, n_layers=1, n_heads=4, n_kv_heads=2, head_dim=64, ffn=512),
                                          n_ctx=256, random_seed=1, device=0, weight_format="bf16")
    rng = np.random.default_rng(3)
    for K in (2048, 8192):
        xh = rng.integers(0x3C00, 0x4000, (1024, K)).astype(np.uint16)
        xl = rng.integers(0x3000, 0x3400, (1024, K)).astype(np.uint16)
        acc = np.zeros(K)
        for _ in range(6):
            acc = llm.imatrix_rows_tap(xh, xl, 1024, acc)
    llm.close()


def leg_trace_pass():
    """two collecting passes of 1024 tokens"""
    llm = _llm(1024)
    ids = _ids(2048)
    llm.imatrix_begin()
    for o in (0, 1024):
        llm.reset()
        llm.imatrix_chunk(ids[o:o + 1024])
    llm.imatrix_end()
    llm.close()


# ------------------------------------------------------------------------------------------------------------------ the parent process
def _child(args, env=None, timeout=600, profile_dir=None):
    cmd = [sys.executable] + args
    if profile_dir:
        cmd = ["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", profile_dir, "--"] + cmd
    e = dict(os.environ)
    e.update(env or {})
    r = subprocess.run(cmd, env=e, capture_output=True, text=True, timeout=timeout, cwd=ROOT)
    if r.returncode != 0:
        sys.stdout.write(r.stdout[-2000:] + r.stderr[-4000:])
        raise SystemExit(f"{' '.join(args)}: exit status {r.returncode}: the run ends here")
    return r.stdout


def _trace(leg, env=None):
    """[(kernel name, K of a collection launch or None, start ns, duration us)] of a leg run under rocprofv3"""
    with tempfile.TemporaryDirectory() as d:
        _child([os.path.abspath(__file__), "--leg", leg], env=env, profile_dir=d)
        files = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
        if not files:
            raise SystemExit(f"{leg}: rocprofv3 wrote no kernel trace")
        out = []
        for r in csv.DictReader(open(files[0])):
            name = r["Kernel_Name"]
            K = None
            if "lm_imatrix_kernel" in name:      # (a workgroup covers 64 columns in both kernels; the grid is counted in lanes)
                K = 64 * int(r["Grid_Size_X"]) // int(r["Workgroup_Size_X"])
            out.append((name, K, int(r["Start_Timestamp"]), (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3))
        return sorted(out, key=lambda t: t[2])


def _per_k(rows):
    by = collections.defaultdict(list)
    for _, K, _, us in rows:
        if K is not None:
            by[K].append(us)
    return by


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", default=None, choices=("rate", "trace_tap", "trace_pass"))
    ap.add_argument("--parent_lib", default=None, help="the parent commit's library, built apart")
    ap.add_argument("--old_kernel_lib", default=None, help="this tree built with the parent commit's lm_imatrix_kernel in place of the rewrite")
    ap.add_argument("--out", default=None)
    ap.add_argument("--smoke", action="store_true")
    ap.add_argument("--formats", nargs="*", default=list(FORMATS))
    a = ap.parse_args()
    if a.leg:
        {"rate": leg_rate, "trace_tap": leg_trace_tap, "trace_pass": leg_trace_pass}[a.leg]()
        return
    me = os.path.abspath(__file__)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").close()

    def say(s):
        print(s, flush=True)
        if a.out:                      # line by line: a leg that fails leaves what was measured before it
            with open(a.out, "a") as f:
                f.write(s + "\n")

    parent = {"RCA_LIB_PATH": os.path.abspath(a.parent_lib)} if a.parent_lib else None
    oldk = {"RCA_LIB_PATH": os.path.abspath(a.old_kernel_lib)} if a.old_kernel_lib else None
    say(f"Llama-3.2-1B dims, random-init bf16 weights, {TOKENS} random ids, n_ctx 1024; three timed runs after a warm-up")
    for ln in _child([me, "--leg", "rate"]).splitlines():
        say(ln)
    say("one collection launch alone (rca_lm_imatrix_rows_tap, 1024 live rows; rocprofv3 --kernel-trace; us: median, min of 6, the first dropped):")
    for label, env in (("this build", None),) + ((("parent's kernel", parent),) if parent else ()):
        by = _per_k(_trace("trace_tap", env))
        for K in sorted(by):
            v = sorted(by[K][1:])
            say(f"  {label:16s} K = {K:5d}: {v[len(v) // 2]:8.1f} {v[0]:8.1f}")
    for label, env in (("this build", None),) + ((("this tree with the parent's kernel", oldk),) if oldk else ()):
        rows = _trace("trace_pass", env)
        first = next(i for i, r in enumerate(rows) if "lm_embed_kernel" in r[0])
        rows = rows[first:]
        total = sum(r[3] for r in rows)
        by = _per_k(rows)
        n_imx = sum(len(v) for v in by.values())
        say(f"two collecting passes of 1024 tokens, {label}: {len(rows)} launches, {total / 2e3:.2f} ms of kernel time per pass; collection launches: "
            f"{n_imx // 2} per pass, {100 * sum(sum(v) for v in by.values()) / total:.2f} % of the kernel time")
        for K in sorted(by):
            say(f"  K = {K:5d}: {len(by[K]) // 2:3d} per pass, average {sum(by[K]) / len(by[K]):7.1f} us")
    if oldk:
        say("the rates again, this tree with the parent's kernel:")
        for ln in _child([me, "--leg", "rate"], env=oldk).splitlines():
            say(ln)
    if parent:
        say("scripts/ab_logits.py, this build against the parent's library (identical lines / lines):")
        for fmt in a.formats:
            arg = [] if fmt == "bf16" else [fmt]
            new = _child([os.path.join(ROOT, "scripts", "ab_logits.py")] + arg).splitlines()
            old = _child([os.path.join(ROOT, "scripts", "ab_logits.py")] + arg, env=parent).splitlines()
            same = sum(x == y for x, y in zip(new, old))
            say(f"  {fmt:5s} {same} of {max(len(new), len(old))}" + ("" if same == len(new) == len(old) else "   DIFFERENT"))
        say("scripts/lm_profile.py 2165 300 (2-token step, graph replay), this build and the parent's library:")
        for label, env in (("this build", None), ("parent", parent), ("this build", None), ("parent", parent)):
            say(f"  {label:10s} " + _child([os.path.join(ROOT, "scripts", "lm_profile.py"), "2165", "300"], env=env).strip().splitlines()[-1])
    if a.smoke:
        import numpy as np
        from quantize_timing import _weights
        from realtime_codec_agent_amd import imatrix as I
        from realtime_codec_agent_amd.llm import LlamaForAlternatingCodeChannels, LMConfig
        cfg = LMConfig.llama_3_2_1b()
        llm = LlamaForAlternatingCodeChannels(config=cfg, weights=_weights(cfg), n_ctx=512, device=0)
        imx = I.collect(llm, [_ids(TOKENS, seed=6)], chunk=512)
        llm.close()
        imx.datasets = [f"{TOKENS} random ids, default_rng(6)"]
        with tempfile.TemporaryDirectory() as d:
            path = os.path.join(d, "collected.gguf")
            I.write_imatrix_gguf(path, imx)
            say(f"SMOKE RUN: collected on the seeded normal weights of scripts/quantize_timing.py: {len(imx)} entries, {imx.chunk_count} chunks of "
                f"{imx.chunk_size}; then scripts/imatrix_timing.py --imatrix (the path below is a temporary file):")
            for ln in _child([os.path.join(ROOT, "scripts", "imatrix_timing.py"), "--imatrix", path], timeout=900).splitlines():
                say("  " + ln)


if __name__ == "__main__":
    main()
