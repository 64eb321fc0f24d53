"""The plan of a streamed decode: which windows the per-chunk loop decodes, what it keeps of each and where the pieces land.

The loop this restates is the one that renders a code string as the live agent would have said it (run_stream_codes.py:60-68):

    for every chunk of the string:
        (_, out), _, _ = tokenizer.detokenize_audio(chunk, preroll_samples=L)      # audio_tokenizer.py:106-149
        audio = smooth_join(audio, out, L, fade_in, fade_out)                      # utils/audio_utils.py:22-30

Per channel, chunk i of a stream ends at code e_i.  detokenize_audio decodes the last max(chunk_i, context_frames) codes up to e_i
(fewer while the stream is younger than that) and keeps the last n_i = int(len_chunk / (framerate * C) * sr) + L samples, at most the
whole window.  smooth_join lays every kept piece L samples before the end of the audio so far and blends the overlap.  None of
this depends on the samples: it is a table, made here in pure Python so that it can be checked without a GPU, and executed either on
the device (rca_codec_decode_rows_dev per row shape, then one rca_codec_crossfade_join_dev) or on the host (run_plan_host, for any
decoder that maps [B, F] codes to the last n samples of their decode).
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Callable, List, Sequence, Tuple

import numpy as np

from ._native import JOIN_SEG, RCA_JOIN_HEAD, RCA_JOIN_TAIL


def chunk_samples(len_chunk: int, framerate: float, channels: int, sr: int, preroll: int) -> int:
    """Samples detokenize_audio owes for a chunk of len_chunk characters (all channels counted): the reference's own expression
    (audio_tokenizer.py:113,141), NOT frames * hop -- at 50 Hz / 16 kHz the two differ for 201, 203, 402, ... frames."""
    return int(len_chunk / (framerate * channels) * sr) + preroll


@dataclass
class StreamPlan:
    """One stream (one channel) of n_codes new codes behind `have` codes of earlier context; offsets are relative to the stream:
    src counts codes from the first context code, seg_off samples in the buffer of decoded pieces, out_off samples of the output."""
    F: np.ndarray         # [S] codes in the window of chunk i (clipped to what the kept samples can see when dec_left is given)
    n: np.ndarray         # [S] samples kept of its decode: preroll + chunk
    src: np.ndarray       # [S] first code of the window
    seg_off: np.ndarray   # [S] pieces back to back
    out_off: np.ndarray   # [S] out_off[i + 1] = out_off[i] + n[i] - n_fade
    n_fade: int
    n_seg: int            # samples of all pieces
    n_out: int            # samples of the joined stream
    joinable: bool        # every piece is long enough for its blends (what rca_codec_crossfade_join_dev asks for)


def plan_stream(n_codes: int, chunk_frames: int, context_frames: int, preroll: int, hop: int, framerate: float, sr: int,
                channels: int = 1, have: int = 0, dec_left=None, n_fade=None) -> StreamPlan:
    """chunk_frames / context_frames / have count frames of ONE channel (the tokenizer's character counts divided by `channels`).
    dec_left: whole frames a kept sample can see to its left (rca_codec_receptive_field); when given, a window is cut down to the
    frames of its kept samples plus that many -- the cut rca_codec_decode_tail_dev makes anyway, so the bits are the same and a
    corpus has two or three row shapes instead of one per warm-up length.  n_fade: overlap of the join (default: the preroll)."""
    if chunk_frames < 1 or context_frames < 0 or preroll < 0 or n_codes < 0 or have < 0:
        raise ValueError(f"plan_stream: n_codes={n_codes} chunk_frames={chunk_frames} context_frames={context_frames} preroll={preroll} have={have}")
    n_fade = preroll if n_fade is None else int(n_fade)
    starts = np.arange(0, n_codes, chunk_frames, dtype=np.int64)
    ends = np.minimum(starts + chunk_frames, n_codes)
    lens = ends - starts
    W = np.minimum(have + ends, np.maximum(lens, context_frames))                     # CodeWindow.push, in closed form
    uniq, inv = np.unique(lens, return_inverse=True)                                  # the chunk size and a shorter last chunk
    n = np.array([chunk_samples(int(l) * channels, framerate, channels, sr, preroll) for l in uniq], dtype=np.int64)[inv].reshape(lens.shape)
    n = np.minimum(n, W * hop)
    F = W.copy()
    if dec_left is not None:
        f0 = (W * hop - n) // hop                                                       # first frame a kept sample belongs to
        F = W - np.maximum(0, f0 - int(dec_left))
    S = len(starts)
    seg_off = np.concatenate([[0], np.cumsum(n)[:-1]]).astype(np.int64) if S else np.zeros(0, np.int64)
    out_off = np.concatenate([[0], np.cumsum(n - n_fade)[:-1]]).astype(np.int64) if S else np.zeros(0, np.int64)
    need = np.full(S, 2 * n_fade, dtype=np.int64)
    if S:
        need[0] -= n_fade
        need[-1] -= n_fade
    ok = bool(S == 0 or (np.all(n >= need) and np.all(n >= 1)))
    return StreamPlan(F=F, n=n, src=have + ends - F, seg_off=seg_off, out_off=out_off, n_fade=n_fade, n_seg=int(n.sum()),
                      n_out=int(n.sum() - n_fade * max(S - 1, 0)), joinable=ok)


def group_rows(F: np.ndarray, n: np.ndarray) -> Tuple[np.ndarray, List[Tuple[int, int, int, int]]]:
    """Rows sorted by shape, stable, largest first -> (order, [(F, n_samples, begin, end)] over the sorted rows)."""
    if len(F) == 0:
        return np.zeros(0, np.int64), []
    order = np.lexsort((-n, -F))                                                        # lexsort is stable; last key is the primary
    Fs, ns = F[order], n[order]
    cut = np.flatnonzero((np.diff(Fs) != 0) | (np.diff(ns) != 0)) + 1
    bounds = np.concatenate([[0], cut, [len(order)]])
    return order, [(int(Fs[a]), int(ns[a]), int(a), int(b)) for a, b in zip(bounds[:-1], bounds[1:])]


@dataclass
class BatchPlan:
    """The plans of many streams laid into one code buffer, one buffer of pieces and one output buffer.  Rows are sorted by shape."""
    F: np.ndarray
    n: np.ndarray
    src: np.ndarray       # code offset of each row's window
    dst: np.ndarray       # offset of each row's piece among the pieces
    groups: List[Tuple[int, int, int, int]]
    segs: np.ndarray      # [S] records (seg_off, n, out_off, flags, reserved): stream-major, the order rca_codec_crossfade_join_dev wants
    n_fade: int
    code_span: int
    seg_span: int
    out_span: int
    out_slices: List[Tuple[int, int]]   # where each stream's samples lie in the output


def plan_batch(lengths: Sequence[int], haves: Sequence[int], chunk_frames: int, context_frames: int, preroll: int, hop: int, framerate: float,
               sr: int, channels: int = 1, dec_left=None, n_fade=None) -> BatchPlan:
    """Stream r holds haves[r] context codes followed by lengths[r] new ones; the streams lie back to back in the code buffer."""
    Fs, ns, srcs, dsts, segs, slices = [], [], [], [], [], []
    code0 = seg0 = out0 = 0
    fade = preroll if n_fade is None else int(n_fade)
    for N, have in zip(lengths, haves):
        p = plan_stream(int(N), chunk_frames, context_frames, preroll, hop, framerate, sr, channels, int(have), dec_left, fade)
        if not p.joinable:
            raise ValueError(f"stream of {N} codes in chunks of {chunk_frames} with {context_frames} context frames: a kept piece is shorter "
                             f"than the {fade}-sample overlaps on its sides (the chunk, or the window, is shorter than the fade)")
        S = len(p.n)
        Fs.append(p.F); ns.append(p.n); srcs.append(code0 + p.src); dsts.append(seg0 + p.seg_off)
        rec = np.zeros(S, JOIN_SEG)
        rec["seg_off"], rec["n"], rec["out_off"] = seg0 + p.seg_off, p.n, out0 + p.out_off
        if S:
            rec["flags"][0] |= RCA_JOIN_HEAD
            rec["flags"][-1] |= RCA_JOIN_TAIL
        segs.append(rec)
        slices.append((out0, out0 + p.n_out))
        code0 += int(have) + int(N); seg0 += p.n_seg; out0 += p.n_out
    cat = lambda xs, dt=np.int64: np.concatenate(xs).astype(dt) if xs else np.zeros(0, dt)
    F, n, src, dst = cat(Fs), cat(ns), cat(srcs), cat(dsts)
    order, groups = group_rows(F, n)
    return BatchPlan(F=F[order], n=n[order], src=src[order], dst=dst[order], groups=groups,
                     segs=np.concatenate(segs) if segs else np.zeros(0, JOIN_SEG), n_fade=fade, code_span=code0, seg_span=seg0, out_span=out0,
                     out_slices=slices)


def join_host(pieces: np.ndarray, segs: np.ndarray, n_fade: int, fade_in: np.ndarray, out: np.ndarray) -> np.ndarray:
    """What rca_codec_crossfade_join_dev computes, in numpy: chained smooth_join written piece by piece."""
    fade_in = np.asarray(fade_in, dtype=np.float32)
    fade_out = fade_in[::-1]
    for s, d in enumerate(segs):
        a, n, o = int(d["seg_off"]), int(d["n"]), int(d["out_off"])
        head, tail = bool(d["flags"] & RCA_JOIN_HEAD), bool(d["flags"] & RCA_JOIN_TAIL)
        lo = 0
        if not head and n_fade:
            p = segs[s - 1]
            pe = int(p["seg_off"]) + int(p["n"])
            out[o:o + n_fade] = pieces[pe - n_fade:pe] * fade_out + pieces[a:a + n_fade] * fade_in
            lo = n_fade
        hi = n if tail else n - n_fade
        out[o + lo:o + hi] = pieces[a + lo:a + hi]
    return out


def run_plan_host(decode_tail: Callable[[np.ndarray, int], np.ndarray], codes: np.ndarray, plan: BatchPlan, fade_in: np.ndarray,
                  batch: int = 256) -> np.ndarray:
    """Execute a BatchPlan with decode_tail(codes [B, F] int64, n) -> f32 [B, n] (the last n samples of each row's decode).
    codes: the flat code buffer the plan was laid over.  -> the flat output buffer (plan.out_slices cuts it into streams)."""
    pieces = np.empty(plan.seg_span, np.float32)
    for F, n, a, b in plan.groups:
        for k in range(a, b, batch):
            rows = range(k, min(b, k + batch))
            win = np.stack([codes[plan.src[r]:plan.src[r] + F] for r in rows])
            pcm = np.asarray(decode_tail(win, n), dtype=np.float32).reshape(len(rows), n)
            for i, r in enumerate(rows):
                pieces[plan.dst[r]:plan.dst[r] + n] = pcm[i]
    return join_host(pieces, plan.segs, plan.n_fade, fade_in, np.empty(plan.out_span, np.float32))
