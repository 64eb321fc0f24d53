"""Importance matrix files: how strongly a corpus drives every input column of every projection, for the weighted quantisers.

What llama-imatrix computes -- per matrix, per input column, the sum over the corpus's tokens of the squared activation (in_sum2) and
the number of tokens (counts) -- in llama.cpp's published GGUF imatrix layout, restated: general.type = "imatrix", imatrix.datasets /
imatrix.chunk_count / imatrix.chunk_size, and per weight `<name>.in_sum2` (F32 [K]) and `<name>.counts` (F32 [1]).  No llama.cpp was
at hand: parity with llama-imatrix's own files is not pinned; read_imatrix_gguf reads what write_imatrix_gguf writes.  This build
does not collect a matrix itself yet (DESIGN.md "Importance matrix"): it reads, merges and writes them, and quantises under one:

    python -m realtime_codec_agent_amd.quantize --model M --out Q.gguf --type q4_k_m --imatrix F.gguf
"""
from __future__ import annotations

import struct
from typing import Dict, Iterable, List, Optional, Tuple

import numpy as np

from . import gguf as G


class Imatrix(dict):
    """{GGUF tensor name: (in_sum2 float64 [K], count)} with where it came from"""

    def __init__(self, entries=(), datasets: Iterable[str] = (), chunk_count: int = 0, chunk_size: int = 0, file: Optional[str] = None):
        super().__init__(entries)
        self.datasets: List[str] = [str(d) for d in datasets]
        self.chunk_count, self.chunk_size, self.file = int(chunk_count), int(chunk_size), file


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
