"""CLI-level throughput of the batch encoder on a synthetic corpus of short utterances (10-60 s stereo .wav, like the reference's
corpora): `audio_to_codes` one file at a time vs. windows batched across files with read / encode / write overlapped, and the same
with --device_ingest (PCM uploaded as the files hold it; conversion, downmix and resampling on the GPU).
usage: cli_corpus_bench.py [hours=1.5] [seed=0] [rate=16000]   (writes the corpus under $TMPDIR or /tmp)
environment: RCA_CLI_RATE (the third argument's default; CallFriend / CallHome are 8000), RCA_CLI_WIDTH = 2 (PCM16, default) or 4
(float32 .wav), RCA_CLI_SWEEP = super-batch sizes (log2) to try, RCA_CLI_READERS = reader thread counts to try on the default and the
device-ingest pipelines (e.g. 4,16), RCA_CLI_REPEAT = runs per leg (default 1; every run is reported)."""
import json, os, shutil, sys, tempfile, time, wave
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from realtime_codec_agent_amd import audio_to_codes

hours = float(sys.argv[1]) if len(sys.argv) > 1 else 1.5
rng = np.random.default_rng(int(sys.argv[2]) if len(sys.argv) > 2 else 0)
rate = int(sys.argv[3]) if len(sys.argv) > 3 else int(os.environ.get("RCA_CLI_RATE", "16000"))
width = int(os.environ.get("RCA_CLI_WIDTH", "2"))
repeat = int(os.environ.get("RCA_CLI_REPEAT", "1"))
root = tempfile.mkdtemp(prefix="rca_corpus_")
raw = os.path.join(root, "raw")
os.makedirs(raw)
total, i = 0.0, 0
t0 = time.perf_counter()
while total < hours * 3600:
    secs = float(rng.uniform(10, 60))
    n = int(secs * rate)
    t = np.arange(n) / float(rate)
    sig = np.stack([0.1 * np.sin(2 * np.pi * f * t) + rng.normal(0, 0.02, n) for f in (220.0 + i, 330.0 + i)])
    d = os.path.join(raw, f"spk{i % 17:02d}")
    os.makedirs(d, exist_ok=True)
    with wave.open(os.path.join(d, f"utt{i:05d}.wav"), "wb") as w:
        w.setnchannels(2); w.setsampwidth(width); w.setframerate(rate)
        w.writeframes((np.clip(sig.T, -1, 1) * 32767).astype("<i2").tobytes() if width == 2 else np.ascontiguousarray(sig.T, "<f4").tobytes())
    total += secs
    i += 1
print(f"corpus: {i} files, {total / 3600:.2f} h stereo at {rate} Hz, {'PCM16' if width == 2 else 'float32'}, written in {time.perf_counter() - t0:.1f} s", flush=True)
res = {}
sweep = [int(x) for x in os.environ.get("RCA_CLI_SWEEP", "").split(",") if x]      # super-batch sizes (log2) to try, e.g. 22,23,24,25,26
readers = [x for x in os.environ.get("RCA_CLI_READERS", "").split(",") if x]       # reader thread counts to try, e.g. 4,16
runs = [("one_file_at_a_time", ["--one_file_at_a_time"]), ("cross_file_pipelined", []), ("cross_file_pipelined+rf_trim", ["--receptive_field_trim"]),
        ("cross_file_pipelined+device_ingest", ["--device_ingest"]), ("one_file_at_a_time+device_ingest", ["--device_ingest", "--one_file_at_a_time"]),
        ("cross_file_pipelined+rf_trim+device_ingest", ["--receptive_field_trim", "--device_ingest"])]
runs += [(f"super_batch_2^{k}", ["--super_batch_samples", str(1 << k)]) for k in sweep]
for k in readers:
    runs += [(f"cross_file_pipelined readers={k}", ["--reader_threads", k]), (f"cross_file_pipelined+device_ingest readers={k}", ["--device_ingest", "--reader_threads", k])]
for name, extra in runs:
    out = os.path.join(root, name.replace("+", "_").replace("^", "").replace(" ", "_").replace("=", ""))
    for rep in range(repeat):
        shutil.rmtree(out, ignore_errors=True)
        s = audio_to_codes.main(["--audio_path", raw, "--codes_path", out, "--stereo"] + extra)
        one = dict(audio_hours_per_hour=s["audio_hours_per_hour"], elapsed_s=s["elapsed_s"])
        st = s.get("stages")
        if st:
            one["stages"] = {k: (round(v, 3) if isinstance(v, float) else v) for k, v in st.items()}
        res.setdefault(name, []).append(one)
        print(name, json.dumps(one), flush=True)
res = {k: (v[0] if repeat == 1 else v) for k, v in res.items()}


def compare(a, b):
    """(every file of tree a equals its twin in b, share of code ids that are equal)"""
    same, equal, count = True, 0, 0
    for r, _, fs in os.walk(a):
        for f in fs:
            pa, pb = os.path.join(r, f), os.path.join(b, os.path.relpath(os.path.join(r, f), a))
            same &= open(pa, "rb").read() == open(pb, "rb").read()
            if f.endswith(".npy"):
                ca, cb = np.load(pa), np.load(pb)
                same &= ca.shape == cb.shape
                if ca.shape == cb.shape:
                    equal += int((ca == cb).sum())
                count += ca.size
    return bool(same), equal / max(count, 1)


same, _ = compare(os.path.join(root, "one_file_at_a_time"), os.path.join(root, "cross_file_pipelined"))
same_ingest, _ = compare(os.path.join(root, "one_file_at_a_time_device_ingest"), os.path.join(root, "cross_file_pipelined_device_ingest"))
_, share = compare(os.path.join(root, "cross_file_pipelined"), os.path.join(root, "cross_file_pipelined_device_ingest"))
print(json.dumps(dict(files=i, audio_hours=total / 3600, rate=rate, sample_width=width, trees_identical=same, device_ingest_trees_identical=same_ingest,
                      device_ingest_ids_equal_to_default=share, **res)))
shutil.rmtree(root, ignore_errors=True)
