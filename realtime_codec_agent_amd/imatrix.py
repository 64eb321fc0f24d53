"""Importance matrix files: how strongly a corpus drives every input column of every projection, for the weighted quantisers.

What llama-imatrix computes -- per matrix, per input column, the sum over the corpus's tokens of the squared activation (in_sum2) and
the number of tokens (counts) -- in llama.cpp's published GGUF imatrix layout, restated: general.type = "imatrix", imatrix.datasets /
imatrix.chunk_count / imatrix.chunk_size, and per weight `<name>.in_sum2` (F32 [K]) and `<name>.counts` (F32 [1]).  No llama.cpp was
at hand: parity with llama-imatrix's own files is not pinned; read_imatrix_gguf reads what write_imatrix_gguf writes.

Collecting one (DESIGN.md "The collector"): a handle whose long evals take the 128-token prefill tiles sums every projection's input on
the card while it evaluates a corpus (LlamaForAlternatingCodeChannels.imatrix_begin / imatrix_chunk / imatrix_read / imatrix_end);
collect() walks token streams as llama-imatrix does, in chunks evaluated from an empty context, and the tool writes the file:

    python -m realtime_codec_agent_amd.imatrix --model M --ids PATH --out F.gguf [--chunk 512] [--chunks N] [--in_file PRIOR.gguf ...]
                                               [--dataset NAME] [--weight_format F] [--kv_format F] [--device N]
    python -m realtime_codec_agent_amd.quantize --model M --out Q.gguf --type q4_k_m --imatrix F.gguf

--ids is a .npy of int32 token ids or a directory of them (as lm_quality reads it); --in_file merges earlier files into the result
(sums, counts and chunks add).  Importing this module loads neither torch nor the library: the tool loads the model inside main().
"""
from __future__ import annotations

import struct
import sys
import time
from typing import Callable, Dict, Iterable, List, Optional, Sequence, Tuple

import numpy as np

from . import gguf as G


class Imatrix(dict):
    """{GGUF tensor name: (in_sum2 float64 [K], count)} with where it came from"""

    def __init__(self, entries=(), datasets: Iterable[str] = (), chunk_count: int = 0, chunk_size: int = 0, file: Optional[str] = None):
        super().__init__(entries)
        self.datasets: List[str] = [str(d) for d in datasets]
        self.chunk_count, self.chunk_size, self.file = int(chunk_count), int(chunk_size), file


# the matrices of a layer that share an input vector, by the collector's kind (kind 4, the final norm's rows, is output.weight's)
KIND_NAMES = {0: ("attn_q", "attn_k", "attn_v"), 1: ("attn_output",), 2: ("ffn_gate", "ffn_up"), 3: ("ffn_down",)}


def merge(a: Imatrix, b: Imatrix) -> Imatrix:
    """Both corpora as one: in_sum2 and counts add per tensor (a tensor only one of them holds is kept), the chunks add."""
    out = Imatrix(datasets=list(getattr(a, "datasets", [])) + [d for d in getattr(b, "datasets", []) if d not in getattr(a, "datasets", [])],
                  chunk_count=getattr(a, "chunk_count", 0) + getattr(b, "chunk_count", 0),
                  chunk_size=getattr(a, "chunk_size", 0) or getattr(b, "chunk_size", 0))
    for name in list(a) + [k for k in b if k not in a]:
        if name in a and name in b:
            (sa, ca), (sb, cb) = a[name], b[name]
            sa, sb = np.asarray(sa, np.float64), np.asarray(sb, np.float64)
            if sa.shape != sb.shape:
                raise ValueError(f"{name}: {sa.shape[0]} columns in one importance matrix, {sb.shape[0]} in the other")
            out[name] = (sa + sb, int(ca) + int(cb))
        else:
            s, c = (a if name in a else b)[name]
            out[name] = (np.array(s, np.float64), int(c))
    return out


def write_imatrix_gguf(path: str, imx: Dict[str, Tuple[np.ndarray, int]], datasets: Optional[Iterable[str]] = None,
                       chunk_count: Optional[int] = None, chunk_size: Optional[int] = None) -> int:
    """A GGUF v3 file of the importance matrix; returns the bytes written.  in_sum2 and counts are stored as F32, as the layout has them."""
    from .quantize import _s, _value
    datasets = list(getattr(imx, "datasets", [])) if datasets is None else [str(d) for d in datasets]
    kv = {"general.type": "imatrix", "general.alignment": 32, "imatrix.datasets": datasets,
          "imatrix.chunk_count": int(getattr(imx, "chunk_count", 0) if chunk_count is None else chunk_count),
          "imatrix.chunk_size": int(getattr(imx, "chunk_size", 0) if chunk_size is None else chunk_size)}
    ts = []
    for name, (sums, count) in imx.items():
        sums = np.asarray(sums, np.float64).reshape(-1)
        if not np.all(np.isfinite(sums)) or np.any(sums < 0) or int(count) < 0:
            raise ValueError(f"{name}: in_sum2 holds a value that is negative or not finite")
        ts.append((f"{name}.in_sum2", sums.astype(np.float32)))
        ts.append((f"{name}.counts", np.array([count], np.float32)))
    infos, off = [], 0
    for name, a in ts:
        infos.append(_s(name.encode()) + struct.pack("<I", 1) + struct.pack("<Q", a.size) + struct.pack("<IQ", G.GGML_F32, off))
        off += a.nbytes + (-a.nbytes) % 32
    head = struct.pack("<IIQQ", G.GGUF_MAGIC, 3, len(ts), len(kv)) + b"".join(_s(k.encode()) + _value(v) for k, v in kv.items()) + b"".join(infos)
    total = 0
    with open(path, "wb") as fh:
        total += fh.write(head + b"\0" * ((-len(head)) % 32))
        for _, a in ts:
            total += fh.write(a.tobytes() + b"\0" * ((-a.nbytes) % 32))
    return total


def read_imatrix_gguf(path: str) -> Imatrix:
    meta, tensors = G.read_gguf(path)
    if meta.get("general.type") != "imatrix":
        raise G.GGUFError(f"{path}: general.type is {meta.get('general.type')!r}, not 'imatrix'")
    ds = meta.get("imatrix.datasets", [])
    out = Imatrix(datasets=[ds] if isinstance(ds, str) else list(ds), chunk_count=int(meta.get("imatrix.chunk_count", 0)),
                  chunk_size=int(meta.get("imatrix.chunk_size", 0)), file=path)
    for name, a in tensors.items():
        if not name.endswith(".in_sum2"):
            continue
        base = name[:-len(".in_sum2")]
        if base + ".counts" not in tensors:
            raise G.GGUFError(f"{path}: {name} has no {base}.counts beside it")
        counts = np.asarray(tensors[base + ".counts"], np.float64).reshape(-1)
        out[base] = (np.asarray(a, np.float32).reshape(-1).astype(np.float64), int(counts[0]))
    return out


def collect(llm, streams: Sequence[Sequence[int]], chunk: int = 512, max_chunks: Optional[int] = None,
            report: Optional[Callable[[str], None]] = None) -> Imatrix:
    """Collect an importance matrix over token streams as llama-imatrix does: every stream is cut into chunks of `chunk` tokens (a
    trailing part-chunk is dropped), each chunk is evaluated from an empty context (reset() before it) and at most `max_chunks` are
    taken.  `llm` is left at the end of the last chunk and no longer collecting."""
    chunk = int(chunk)
    if chunk < 1:
        raise ValueError(f"collect: chunk = {chunk}")
    if chunk > llm.n_ctx():
        raise ValueError(f"collect: a chunk of {chunk} tokens does not fit n_ctx = {llm.n_ctx()}")
    pieces = [(s, off) for s, stream in enumerate(streams) for off in range(0, len(stream) - chunk + 1, chunk)]
    if max_chunks is not None:
        pieces = pieces[:max(int(max_chunks), 0)]
    if not pieces:
        raise ValueError(f"collect: no stream holds a whole chunk of {chunk} tokens")
    llm.imatrix_begin()
    try:
        for i, (s, off) in enumerate(pieces):
            llm.reset()
            llm.imatrix_chunk(np.asarray(streams[s][off:off + chunk], np.int32))
            if report is not None and ((i + 1) % 16 == 0 or i + 1 == len(pieces)):
                report(f"chunk {i + 1} / {len(pieces)}")
        out = llm.imatrix_read()
    finally:
        llm.imatrix_end()
    out.chunk_count, out.chunk_size = len(pieces), chunk
    return out


def main(argv: Optional[Sequence[str]] = None, make_llm: Optional[Callable] = None) -> int:
    """make_llm(args) -> the handle to collect on (tests hand in a stand-in; default: load --model)"""
    import argparse
    ap = argparse.ArgumentParser(prog="python -m realtime_codec_agent_amd.imatrix", description="Collect an importance matrix on the card and write it as a GGUF imatrix file.")
    ap.add_argument("--model", required=True)
    ap.add_argument("--ids", required=True, help=".npy of int32 token ids, or a directory of them")
    ap.add_argument("--out", required=True, help="the GGUF imatrix file to write")
    ap.add_argument("--chunk", type=int, default=512, help="tokens per chunk, each evaluated from an empty context")
    ap.add_argument("--chunks", type=int, default=None, help="at most this many chunks (default: all)")
    ap.add_argument("--in_file", action="append", default=[], help="an earlier imatrix file to merge into the result (repeatable)")
    ap.add_argument("--dataset", default=None, help="the name stored in imatrix.datasets (default: --ids)")
    ap.add_argument("--weight_format", default=None)
    ap.add_argument("--kv_format", default=None)
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args(argv)
    from .lm_quality import load_streams
    streams = load_streams(a.ids)
    prior = [read_imatrix_gguf(f) for f in a.in_file]
    if make_llm is None:
        from .llm import LlamaForAlternatingCodeChannels
        make_llm = lambda a: LlamaForAlternatingCodeChannels(model_path=a.model, n_ctx=a.chunk, device=a.device, weight_format=a.weight_format,
                                                             kv_format=a.kv_format)
    llm = make_llm(a)
    try:
        t0 = time.perf_counter()
        imx = collect(llm, streams, chunk=a.chunk, max_chunks=a.chunks, report=lambda s: print(s, file=sys.stderr))
        dt = time.perf_counter() - t0
    finally:
        llm.close()
    imx.datasets = [a.dataset if a.dataset is not None else a.ids]
    tokens = imx.chunk_count * imx.chunk_size
    for p in prior:
        imx = merge(p, imx)
    write_imatrix_gguf(a.out, imx)
    print(f"{a.out}: {len(imx)} entries, {imx.chunk_count} chunks of {imx.chunk_size} tokens"
          + (f" ({len(prior)} merged in)" if prior else ""))
    print(f"collected {tokens} tokens in {dt:.2f} s: {tokens / max(dt, 1e-9):.0f} tokens / s")
    return 0


if __name__ == "__main__":
    sys.exit(main())
