"""Batch decoder CLI -- the way back from a tree of code files to audio, rendered as the streaming detokenizer renders it:

    python -m realtime_codec_agent_amd.codes_to_audio --codes_path data/audio/codes --audio_path data/audio/rendered \
        --chunk_size_secs 0.1 --context_secs 2.0 --fade_secs 0.02 --codec_model MagiCodec-50Hz-Base [--stereo] [--format {wav16,npy}]

--codes_path is a leaf directory written by audio_to_codes (codec_info.json next to <relative path>_c<channel>.npy files, each an
int64 array (1, T)) or any directory above such leaves; the output tree repeats the input tree below --audio_path.  Without
--stereo every code file becomes one mono file of the same name; with it the _c0 / _c1 / ... files of one stem become one
multi-channel file <stem>.wav (a stem whose channels differ in length is refused by name, the others are rendered).

What is rendered is the per-chunk loop of run_stream_codes.py:60-68 -- detokenize_audio(chunk, preroll_samples=L) followed by
smooth_join, one chunk of --chunk_size_secs at a time with --context_secs of rolling code context -- because that, not a whole-file
decode, is what a listener of the live agent hears: a streaming window has no right context and the 20 ms equal-power crossfade
hides the seam.  The loop is executed as a plan (stream_decode.py): every window of every chunk of every channel is one row of
rca_codec_decode_rows_dev, rows grouped by shape, and one rca_codec_crossfade_join_dev per super-batch joins all streams.  Default
path: super-batches of code files are uploaded once, reader threads / GPU / writer thread overlap; --one_file_at_a_time is the
simple loop over files.  Both give the same bytes (tests compare the trees).  Multi-GPU as audio_to_codes: one process per GPU, files
dealt to ranks by duration.
"""
from __future__ import annotations

import argparse
import json
import os
import queue
import re
import sys
import threading
import time
import wave
from concurrent.futures import ThreadPoolExecutor
from typing import Callable, Iterator, List, Optional, Sequence, Tuple

import numpy as np

from .dist_utils import ControlPlane, env_rank_world, shard_by_duration
from .stream_decode import plan_batch, run_plan_host
from .utils.audio_utils import create_crossfade_ramps

DEFAULT_SUPER_BATCH_CODES = 1 << 17       # codes (all channels) per super-batch: 44 min of audio, ~200 MB of f32 pieces and output
_CHANNEL_FILE = re.compile(r"^(.*)_c(\d+)\.npy$")


class HostStreamDecoder:
    """The plan executed on the host for any decode_tail(codes [B, F] int64, n) -> f32 [B, n] (the CPU oracle in the tests):
    the same table, the same grouping, numpy's own smooth_join arithmetic."""

    def __init__(self, cfg, decode_tail: Callable[[np.ndarray, int], np.ndarray], clip: bool = True):
        self.cfg = cfg
        self._decode_tail = decode_tail
        self.dec_left = cfg.receptive_field()[1] if clip else None

    def decode_many(self, streams: Sequence[np.ndarray], chunk_frames: int, context_frames: int, n_fade: int, fade_in: np.ndarray, batch: int):
        """streams: int64 [C_f, N_f] per file.  -> (flat f32 host buffer, [(a, b)] slice of every (file, channel) row, wait())."""
        rows = [r for s in streams for r in s]
        plan = plan_batch([len(r) for r in rows], [0] * len(rows), chunk_frames, context_frames, n_fade, self.cfg.hop, self.cfg.framerate,
                          self.cfg.sample_rate, dec_left=self.dec_left)
        codes = np.concatenate(rows).astype(np.int64) if rows else np.zeros(0, np.int64)
        if codes.size and (codes.min() < 0 or codes.max() >= self.cfg.codebook_size):
            raise ValueError(f"code out of range [0, {self.cfg.codebook_size})")
        return run_plan_host(self._decode_tail, codes, plan, fade_in, batch), plan.out_slices, (lambda: None)

    def decode(self, codes: np.ndarray, chunk_frames: int, context_frames: int, n_fade: int, fade_in: np.ndarray, batch: int) -> np.ndarray:
        out, slices, _ = self.decode_many([codes], chunk_frames, context_frames, n_fade, fade_in, batch)
        return np.stack([out[a:b] for a, b in slices]) if slices else np.zeros((0, 0), np.float32)


class HipStreamDecoder:
    """codes [C, N] int64 -> f32 [C, N_out] through MagiCodecHIP.run_stream_plan."""

    RING = 3      # super-batches in flight: one being packed, one on the GPU, one being written

    def __init__(self, codec_model: str, device_index: int):
        import torch
        from .codec import load_magicodec_model
        self.torch = torch
        self.device = torch.device("cuda", device_index)
        self.model, _, _ = load_magicodec_model(codec_model, self.device)
        self.cfg = self.model.cfg
        self.dec_left = self.model.hip.receptive_field()[1]
        self.stage_times = dict(slot_wait_s=0.0, pack_s=0.0, enqueue_s=0.0, gpu_ms=0.0, super_batches=0, passes=0)

    def decode(self, codes: np.ndarray, chunk_frames: int, context_frames: int, n_fade: int, fade_in: np.ndarray, batch: int) -> np.ndarray:
        return self.model.stream_decode_np(codes, chunk_frames, context_frames, n_fade, fade_in, batch=batch)

    def _slot(self, k: int, n_codes: int, n_out: int):
        """Ring slot k: pinned staging for the codes and for the rendered samples, grown on demand and reused."""
        torch = self.torch
        if not hasattr(self, "_ring"):
            self._ring = [dict() for _ in range(self.RING)]
        sl = self._ring[k]
        if sl.get("ev") is not None:
            sl["ev"].synchronize()                              # the slot's previous super-batch has left the GPU
        if sl.get("free") is not None:
            sl["free"].wait()                                   # ... and the writer is done with its samples
        sl["free"] = threading.Event()
        for name, n, dtype in (("codes", n_codes, torch.int64), ("pcm", n_out, torch.float32)):
            if sl.get(name) is None or sl[name].numel() < n:
                sl[name] = torch.empty(max(int(n * 1.25), 1), dtype=dtype).pin_memory()
        return sl

    def decode_many(self, streams: Sequence[np.ndarray], chunk_frames: int, context_frames: int, n_fade: int, fade_in: np.ndarray, batch: int):
        """As HostStreamDecoder.decode_many; everything up to the D2H copy is enqueued asynchronously, wait() blocks until the samples
        have landed and raises if a code was out of range; the host buffer stays valid until wait.release() / RING - 1 further calls."""
        torch = self.torch
        t_in = time.perf_counter()
        rows = [r for s in streams for r in s]
        plan = plan_batch([len(r) for r in rows], [0] * len(rows), chunk_frames, context_frames, n_fade, self.cfg.hop, self.cfg.framerate,
                          self.cfg.sample_rate, dec_left=self.dec_left)
        self._calls = getattr(self, "_calls", 0) + 1
        sl = self._slot(self._calls % self.RING, plan.code_span, plan.out_span)
        t_slot = time.perf_counter()
        st_ = self.stage_times
        if plan.out_span == 0:
            sl["free"].set()
            return sl["pcm"].numpy()[:0], plan.out_slices, (lambda: None)
        cv, o = sl["codes"].numpy(), 0
        for r in rows:
            cv[o:o + len(r)] = r
            o += len(r)
        t_pack = time.perf_counter()
        with torch.cuda.device(self.device):
            st = torch.cuda.current_stream(self.device)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            codes_dev = sl["codes"][:plan.code_span].to(self.device, non_blocking=True)
            e0.record(st)
            out = self.model.run_stream_plan(codes_dev, plan, fade_in, batch, st_)
            e1.record(st)
            sl["pcm"][:plan.out_span].copy_(out, non_blocking=True)
            ev = torch.cuda.Event()
            ev.record(st)
            sl["ev"] = ev
        host = sl["pcm"].numpy()[:plan.out_span]
        t_out = time.perf_counter()
        st_["slot_wait_s"] += t_slot - t_in; st_["pack_s"] += t_pack - t_slot; st_["enqueue_s"] += t_out - t_pack; st_["super_batches"] += 1
        hip, stream = self.model.hip, st.cuda_stream

        def wait():
            ev.synchronize()
            st_["gpu_ms"] += e0.elapsed_time(e1)
            hip.check_decode_error(stream)
        wait.release = sl["free"].set
        return host, plan.out_slices, wait


# ------------------------------------------------------------------------------------------------ the tree
class Item:
    """One output file: the code files of its channels, in channel order."""
    __slots__ = ("leaf", "rel", "paths")

    def __init__(self, leaf: str, rel: str, paths: List[str]):
        self.leaf, self.rel, self.paths = leaf, rel, paths


def find_leaves(codes_path: str) -> List[str]:
    """Directories at or below codes_path that hold a codec_info.json, sorted."""
    return sorted(root for root, _, files in os.walk(codes_path) if "codec_info.json" in files)


def check_codec_info(leaf: str, cfg) -> None:
    with open(os.path.join(leaf, "codec_info.json")) as f:
        info = json.load(f)
    if int(info.get("num_codebooks", 1)) != 1:
        raise ValueError(f"{leaf}: codec_info.json names {info['num_codebooks']} codebooks, this codec has 1")
    if int(info.get("codebook_size", -1)) != cfg.codebook_size:
        raise ValueError(f"{leaf}: codec_info.json names a codebook of {info.get('codebook_size')}, the model has {cfg.codebook_size}")
    if float(info.get("framerate", -1)) != float(cfg.framerate):
        raise ValueError(f"{leaf}: codec_info.json names {info.get('framerate')} frames per second, the model makes {cfg.framerate}")


def list_items(leaf: str, stereo: bool) -> List[Item]:
    """The outputs of one leaf.  Mono: one per code file.  Stereo: one per stem, its _c<k> files in channel order."""
    found = []
    for root, _, files in os.walk(leaf):
        for f in sorted(files):
            m = _CHANNEL_FILE.match(f)
            if m:
                found.append((os.path.relpath(os.path.join(root, m.group(1)), leaf), int(m.group(2)), os.path.join(root, f)))
    found.sort()
    if not stereo:
        return [Item(leaf, f"{stem}_c{c}", [p]) for stem, c, p in found]
    items: List[Item] = []
    for stem, c, p in found:
        if items and items[-1].rel == stem:
            items[-1].paths.append(p)
        else:
            items.append(Item(leaf, stem, [p]))
    return items


def probe_codes(item: Item) -> int:
    return int(np.load(item.paths[0], mmap_mode="r").shape[-1])


def read_item(item: Item) -> np.ndarray:
    """-> int64 [C, N]; ValueError naming the stem when its channels differ in length."""
    rows = [np.load(p).reshape(-1).astype(np.int64, copy=False) for p in item.paths]
    if len({len(r) for r in rows}) > 1:
        raise ValueError(f"{os.path.join(item.leaf, item.rel)}: channels differ in length ({', '.join(str(len(r)) for r in rows)} codes)")
    return np.stack(rows)


def write_audio(path_no_ext: str, pcm: np.ndarray, sr: int, fmt: str) -> str:
    """pcm f32 [C, N].  npy: the array as it is.  wav16: rint(clip(x, -1, 1) * 32767) as little-endian int16, channels interleaved."""
    if fmt == "npy":
        dst = path_no_ext + ".npy"
        np.save(dst, np.ascontiguousarray(pcm, dtype=np.float32))
        return dst
    dst = path_no_ext + ".wav"
    q = np.rint(np.clip(pcm, -1.0, 1.0) * 32767.0).astype("<i2")
    with wave.open(dst, "wb") as w:
        w.setnchannels(pcm.shape[0])
        w.setsampwidth(2)
        w.setframerate(sr)
        w.writeframes(np.ascontiguousarray(q.T).tobytes())
    return dst


def _out_base(args, item: Item) -> str:
    rel_leaf = os.path.relpath(item.leaf, args.codes_path)
    dst = os.path.normpath(os.path.join(args.audio_path, rel_leaf, item.rel))
    os.makedirs(os.path.dirname(dst), exist_ok=True)
    return dst


class _Refused:
    def __init__(self):
        self.names: List[str] = []
        self.lock = threading.Lock()

    def add(self, err: ValueError) -> None:
        with self.lock:
            self.names.append(str(err))
        print(f"codes_to_audio: refused: {err}", file=sys.stderr)


def _read_or_refuse(item: Item, refused: _Refused) -> Optional[np.ndarray]:
    try:
        return read_item(item)
    except ValueError as e:
        refused.add(e)
        return None


def _plan_args(args, cfg) -> Tuple[int, int, int, np.ndarray]:
    chunk_frames = int(args.chunk_size_secs * cfg.framerate)
    if chunk_frames < 1:
        raise ValueError(f"--chunk_size_secs {args.chunk_size_secs} holds no code at {cfg.framerate} Hz")
    n_fade, fade_in, _ = create_crossfade_ramps(cfg.sample_rate, args.fade_secs)
    return chunk_frames, int(args.context_secs * cfg.framerate), n_fade, fade_in


def decode_files(items: Sequence[Item], decoder, args, refused: _Refused) -> Tuple[float, int]:
    """Render `items` with `decoder` (anything with .cfg and .decode(codes, chunk_frames, context_frames, n_fade, fade_in, batch));
    returns (audio seconds, codes read)."""
    if hasattr(decoder, "decode_many") and not args.one_file_at_a_time:
        return decode_files_pipelined(items, decoder, args, refused)
    cfg = decoder.cfg
    chunk_frames, ctx_frames, n_fade, fade_in = _plan_args(args, cfg)
    secs, n_codes = 0.0, 0
    for item in items:
        codes = _read_or_refuse(item, refused)
        if codes is None:
            continue
        pcm = decoder.decode(codes, chunk_frames, ctx_frames, n_fade, fade_in, args.batch_size)
        write_audio(_out_base(args, item), pcm, cfg.sample_rate, args.format)
        secs += pcm.shape[-1] / cfg.sample_rate
        n_codes += int(codes.size)
    return secs, n_codes


def _super_batches(items: Sequence[Item], budget_codes: int, readers: int, refused: _Refused) -> Iterator[List[Tuple[Item, np.ndarray]]]:
    """Reader stage: code files are loaded by a small thread pool a bounded distance ahead of the consumer and handed over in groups
    of about budget_codes codes (all channels counted); the first groups are small so that the GPU has work early."""
    with ThreadPoolExecutor(max_workers=readers) as pool:
        pending: "queue.Queue" = queue.Queue()
        it = iter(items)
        inflight = 0

        def submit_more():
            nonlocal inflight
            while inflight < 4 * readers:
                item = next(it, None)
                if item is None:
                    return
                pending.put((item, pool.submit(_read_or_refuse, item, refused)))
                inflight += 1
        submit_more()
        group, size, n_groups = [], 0, 0
        while inflight:
            item, fut = pending.get()
            codes = fut.result()
            inflight -= 1
            submit_more()
            if codes is None:
                continue
            budget = budget_codes >> 3 if n_groups == 0 else budget_codes >> 1 if n_groups == 1 else budget_codes
            if group and size + codes.size > budget:
                yield group
                group, size, n_groups = [], 0, n_groups + 1
            group.append((item, codes))
            size += codes.size
        if group:
            yield group


def decode_files_pipelined(items: Sequence[Item], decoder, args, refused: _Refused) -> Tuple[float, int]:
    """The same output tree as the one-file-at-a-time loop, with rows batched across files and the three stages (read, decode,
    write) overlapped.  Per-stage wall times are left in `decoder.pipeline_times`."""
    cfg = decoder.cfg
    chunk_frames, ctx_frames, n_fade, fade_in = _plan_args(args, cfg)
    done: "queue.Queue" = queue.Queue(maxsize=1)     # the ring of the decoder bounds what is in flight
    totals = [0.0, 0]
    errors: List[BaseException] = []
    times = dict(read_wait_s=0.0, decode_many_s=0.0, queue_wait_s=0.0, writer_wait_s=0.0, writer_save_s=0.0)

    def writer():
        while True:
            job = done.get()
            if job is None:
                return
            group, wait, host, slices = job
            try:
                if errors:
                    continue                                  # a failed run writes nothing more; the queue is still drained
                t0 = time.perf_counter()
                wait()                                        # the D2H copy of this super-batch has landed
                t1 = time.perf_counter()
                r = 0
                for item, codes in group:
                    rows = slices[r:r + codes.shape[0]]
                    r += codes.shape[0]
                    write_audio(_out_base(args, item), np.stack([host[a:b] for a, b in rows]), cfg.sample_rate, args.format)
                times["writer_wait_s"] += t1 - t0
                times["writer_save_s"] += time.perf_counter() - t1
            except BaseException as e:                        # surfaced by the main thread after the join
                errors.append(e)
            finally:
                rel_fn = getattr(wait, "release", None)
                if rel_fn is not None:
                    rel_fn()
    wt = threading.Thread(target=writer, daemon=True)
    wt.start()
    t_start = time.perf_counter()
    try:
        gen = _super_batches(items, args.super_batch_codes, args.reader_threads, refused)
        while not errors:
            t0 = time.perf_counter()
            group = next(gen, None)
            t1 = time.perf_counter()
            times["read_wait_s"] += t1 - t0
            if group is None:
                break
            streams = [c for _, c in group]
            host, slices, wait = decoder.decode_many(streams, chunk_frames, ctx_frames, n_fade, fade_in, args.batch_size)
            t2 = time.perf_counter()
            times["decode_many_s"] += t2 - t1
            if len(slices) != sum(c.shape[0] for c in streams):
                raise RuntimeError(f"decode_many returned {len(slices)} rows for {sum(c.shape[0] for c in streams)} (file, channel) rows")
            done.put((group, wait, host, slices))
            times["queue_wait_s"] += time.perf_counter() - t2
            totals[0] += sum((b - a) for (a, b), _ in zip(_first_rows(slices, streams), streams)) / cfg.sample_rate
            totals[1] += int(sum(c.size for c in streams))
    finally:
        done.put(None)
        wt.join()
    if errors:
        raise errors[0]
    times["total_s"] = time.perf_counter() - t_start
    if hasattr(decoder, "stage_times"):
        times.update({f"decode_many_{k}": v for k, v in decoder.stage_times.items()})
    decoder.pipeline_times = times
    return totals[0], totals[1]


def _first_rows(slices, streams):
    r = 0
    for c in streams:
        yield slices[r]
        r += c.shape[0]


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(description="Render code files as the streaming detokenizer would (sharded batch decode).")
    ap.add_argument("--codes_path", required=True, help="a leaf written by audio_to_codes (holds codec_info.json) or a tree of such leaves")
    ap.add_argument("--audio_path", required=True)
    ap.add_argument("--chunk_size_secs", type=float, default=0.1)
    ap.add_argument("--context_secs", type=float, default=2.0)
    ap.add_argument("--fade_secs", type=float, default=0.02)
    ap.add_argument("--batch_size", type=int, default=256)
    ap.add_argument("--codec_model", default="MagiCodec-50Hz-Base")
    ap.add_argument("--stereo", action="store_true", help="merge the _c0 / _c1 / ... files of one stem into one multi-channel file")
    ap.add_argument("--format", choices=("wav16", "npy"), default="wav16",
                    help="wav16: rint(clip(x, -1, 1) * 32767) as 16-bit PCM; npy: the exact float32 [C, N]")
    ap.add_argument("--one_file_at_a_time", action="store_true", help="the simple loop (a pass never spans files, no overlap of read / decode / write)")
    ap.add_argument("--super_batch_codes", type=int, default=DEFAULT_SUPER_BATCH_CODES, help="codes (all channels) uploaded and decoded per super-batch")
    ap.add_argument("--reader_threads", type=int, default=4)
    return ap


def main(argv=None, decoder=None, backend: Optional[str] = None) -> dict:
    args = build_parser().parse_args(argv)
    rank, world, local = env_rank_world()
    if decoder is None:
        if os.environ.get("RCA_DEVICE") is not None:
            local = int(os.environ["RCA_DEVICE"])
        decoder = HipStreamDecoder(args.codec_model, local)
        backend = backend or os.environ.get("RCA_DIST_BACKEND", "nccl")
    leaves = find_leaves(args.codes_path)
    if not leaves:
        raise ValueError(f"{args.codes_path}: no codec_info.json at or below it (not a tree written by audio_to_codes)")
    for leaf in leaves:
        check_codec_info(leaf, decoder.cfg)
    cp = ControlPlane(prefer=backend or "gloo", device_index=local)
    items = [it for leaf in leaves for it in list_items(leaf, args.stereo)]
    shards = shard_by_duration([probe_codes(it) / decoder.cfg.framerate for it in items], world)
    mine = [items[i] for i in shards[rank]]
    refused = _Refused()
    dev = getattr(decoder, "device", None)
    cp.barrier()
    t0 = time.perf_counter()
    secs, ncodes = decode_files(mine, decoder, args, refused)
    if dev is not None and hasattr(decoder, "torch"):
        decoder.torch.cuda.synchronize(dev)
    cp.barrier()
    elapsed = cp.max(time.perf_counter() - t0)
    total_secs = cp.sum(secs)
    total_codes = cp.sum(float(ncodes))
    summary = dict(files=len(items), world_size=world, audio_hours=total_secs / 3600.0, codes=int(total_codes), elapsed_s=elapsed,
                   audio_hours_per_hour=(total_secs / elapsed) if elapsed > 0 else None, control_plane=cp.backend,
                   refused=sorted(refused.names), stages=getattr(decoder, "pipeline_times", None))
    if rank == 0:
        print(json.dumps(summary))
    return summary


if __name__ == "__main__":
    main()
