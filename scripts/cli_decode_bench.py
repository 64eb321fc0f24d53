"""CLI-level throughput of the batch decoder on a synthetic tree of code files (10-60 s files, mono and stereo stems, as audio_to_codes
writes them): three legs of the same build, each rendering the same tree to exact float32 --
  per_chunk_loop        AudioTokenizer.detokenize_audio(chunk, preroll_samples=L) + smooth_join per 0.1 s chunk, one file at a time
                        (run_stream_codes.py:60-68: the only way to render codes before codes_to_audio existed)
  one_file_at_a_time    codes_to_audio --one_file_at_a_time: the plan on the device, a pass never spans files
  pipelined             codes_to_audio's default: super-batches of files, reader / GPU / writer overlapped
and the share of the pipelined run's wall time the GPU spent in the decode passes and the join (events around them).
usage: cli_decode_bench.py [hours=0.5] [seed=0]     environment: RCA_CLI_REPEAT = runs per leg (default 3; every run is reported)"""
import json, os, shutil, sys, tempfile, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from realtime_codec_agent_amd import codes_to_audio
from realtime_codec_agent_amd.audio_tokenizer import AudioTokenizer
from realtime_codec_agent_amd.codec_chars import codes_to_chars
from realtime_codec_agent_amd.utils.audio_utils import create_crossfade_ramps, smooth_join

hours = float(sys.argv[1]) if len(sys.argv) > 1 else 0.5
rng = np.random.default_rng(int(sys.argv[2]) if len(sys.argv) > 2 else 0)
repeat = int(os.environ.get("RCA_CLI_REPEAT", "3"))
root = tempfile.mkdtemp(prefix="rca_codes_")
dec = codes_to_audio.HipStreamDecoder("MagiCodec-50Hz-Base", int(os.environ.get("RCA_DEVICE", "0")))
cfg = dec.cfg
leaf = os.path.join(root, "codes", cfg.name, "0.1s_2.0s", "stereo")
os.makedirs(leaf)
with open(os.path.join(leaf, "codec_info.json"), "w") as f:
    json.dump({"num_codebooks": 1, "codebook_size": cfg.codebook_size, "framerate": cfg.framerate}, f)
total, i = 0.0, 0
while total < hours * 3600:
    secs = float(rng.uniform(10, 60))
    n = int(secs * cfg.framerate)
    d = os.path.join(leaf, f"spk{i % 17:02d}")
    os.makedirs(d, exist_ok=True)
    for c in range(1 if i % 3 == 0 else 2):                                   # every third stem is mono
        np.save(os.path.join(d, f"utt{i:05d}_c{c}.npy"), rng.integers(0, cfg.codebook_size, size=(1, n)).astype(np.int64))
        total += n / cfg.framerate
    i += 1
print(f"tree: {i} stems, {total / 3600:.2f} channel-hours of codes at {cfg.framerate} Hz", flush=True)


def per_chunk_loop(out_root):
    """The loop the CLI replaces, on the same model object, writing the same files."""
    n_fade, fade_in, fade_out = create_crossfade_ramps(cfg.sample_rate, 0.02)
    toks = {}
    args = codes_to_audio.build_parser().parse_args(["--codes_path", os.path.join(root, "codes"), "--audio_path", out_root, "--stereo", "--format", "npy"])
    t0 = time.perf_counter()
    secs = 0.0
    for item in codes_to_audio.list_items(leaf, True):
        codes = codes_to_audio.read_item(item)
        C = codes.shape[0]
        tok = toks.get(C)
        if tok is None:
            tok = toks[C] = AudioTokenizer(codec_model=dec.model, num_channels=C, device=dec.device)
        tok.reset_context()
        chars = "".join(ch for frame in zip(*[codes_to_chars(r, cfg.codebook_size) for r in codes]) for ch in frame)
        step = int(0.1 * tok.framerate * C)
        audio = np.zeros((C, 0), np.float32)
        for s in range(0, len(chars), step):
            (_, out), _, _ = tok.detokenize_audio(chars[s:s + step], preroll_samples=n_fade)
            audio = smooth_join(audio, out.reshape(C, -1), n_fade, fade_in, fade_out)
        codes_to_audio.write_audio(codes_to_audio._out_base(args, item), audio, cfg.sample_rate, "npy")
        secs += audio.shape[-1] / cfg.sample_rate
    el = time.perf_counter() - t0
    return dict(audio_hours_per_hour=secs / el, elapsed_s=el)


def cli(out_root, extra):
    s = codes_to_audio.main(["--codes_path", os.path.join(root, "codes"), "--audio_path", out_root, "--stereo", "--format", "npy"] + extra, decoder=dec)
    one = dict(audio_hours_per_hour=s["audio_hours_per_hour"], elapsed_s=s["elapsed_s"])
    if s.get("stages") and not extra:
        one["stages"] = {k: (round(v, 3) if isinstance(v, float) else v) for k, v in s["stages"].items()}
    return one


res = {}
for name, fn in (("per_chunk_loop", per_chunk_loop), ("one_file_at_a_time", lambda o: cli(o, ["--one_file_at_a_time"])), ("pipelined", lambda o: cli(o, []))):
    out = os.path.join(root, name)
    for rep in range(repeat):
        shutil.rmtree(out, ignore_errors=True)
        before = dict(dec.stage_times)
        one = fn(out)
        if name == "pipelined":
            gpu_ms = dec.stage_times["gpu_ms"] - before["gpu_ms"]
            one["decode_gpu_share_of_wall"] = round(gpu_ms / 1e3 / one["elapsed_s"], 3)
            one["decode_gpu_ms"] = round(gpu_ms, 1)
        res.setdefault(name, []).append(one)
        print(name, json.dumps(one), flush=True)


def same_tree(a, b):
    ok, n = True, 0
    for r, _, fs in os.walk(a):
        for f in fs:
            pa, pb = os.path.join(r, f), os.path.join(b, os.path.relpath(os.path.join(r, f), a))
            ok &= os.path.exists(pb) and open(pa, "rb").read() == open(pb, "rb").read()
            n += 1
    return bool(ok and n > 0)


best = {k: max(r["audio_hours_per_hour"] for r in v) for k, v in res.items()}
print(json.dumps(dict(stems=i, channel_hours=total / 3600, loop_tree_equals_one_file=same_tree(os.path.join(root, "per_chunk_loop"), os.path.join(root, "one_file_at_a_time")),
                      one_file_tree_equals_pipelined=same_tree(os.path.join(root, "one_file_at_a_time"), os.path.join(root, "pipelined")),
                      best_audio_hours_per_hour=best, pipelined_over_loop=best["pipelined"] / best["per_chunk_loop"], **res)))
shutil.rmtree(root, ignore_errors=True)
