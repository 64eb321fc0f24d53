"""Make a quantised LM here: quantise a checkpoint's matrices on the card and write a llama-architecture GGUF.

The reference gets its Q8_0 / Q4_K_M models from llama.cpp's tools (prep_test_model.sh:28-31: convert_hf_to_gguf.py + llama-quantize).
This module goes from an HF directory, an .npz (llm.save_npz) or an F32 / F16 / BF16 GGUF to a Q8_0 / Q4_K / Q5_K / Q6_K / Q4_K_M / Q5_K_M
model, in memory (`quantize_weights`, handed to LlamaForAlternatingCodeChannels(weights=..., config=...)) or as a file (`write_llama_gguf`,
read back by gguf.load_llama_gguf; laid out as convert_hf_to_gguf.py lays one out, though no llama.cpp was at hand to open one):

    python -m realtime_codec_agent_amd.quantize --model IN --out OUT.gguf --type q4_k_m [--rule search|minmax] [--imatrix F.gguf] [--device N]

The quantisers run on the device (rca_quantize_rows, csrc/rca_quant_rows.h).  rule="search" restates the scale searches of ggml's published
reference quantisers (make_qkx2_quants for Q4_K / Q5_K, make_qx_quants for Q6_K; DESIGN.md "Quantising on the card"); ggml is not part of this
tree, so parity with llama-quantize's own bits is not pinned -- every block written de-quantises by GGUF's rule, which is what a reader
depends on.  rule="minmax" is this build's plain rule, the one weight_format="q4_k" / "q5_k" applies at load.

--imatrix / imatrix=: an importance matrix (a GGUF imatrix file, realtime_codec_agent_amd.imatrix: per input column of every projection,
the mean squared activation over a corpus) turns the search into the weighted one (rca_quantize_rows_w; DESIGN.md "Weighted K-quant search"): the error
of a column counts by how strongly the corpus drives it.  What llama-quantize --imatrix does, restated; parity with its bits is not pinned.

The "q4_k_m" / "q5_k_m" recipes are llama-quantize's type mix (llama_tensor_get_type for LLAMA_FTYPE_MOSTLY_Q4_K_M / Q5_K_M on a model
without MoE / GQA special cases): Q6_K for output.weight and for attn_v / ffn_down in the layers use_more_bits() picks, Q4_K resp. Q5_K for
every other matrix, the embedding table included; norms and rope_freqs stay F32.  A matrix whose K is not a multiple of 256 or whose N is
not a multiple of 4 stays F16 with a warning (llama-quantize would fall back to legacy types this build refuses).
"""
from __future__ import annotations

import argparse
import ctypes as C
import struct
import sys
import time
import warnings
from typing import Any, Callable, Dict, Optional

import numpy as np

from . import _native as N
from . import gguf as G

# type name -> (RCA dtype, blocks class, values per block, bytes per block, GGUF tensor type)
TYPES = {"q8_0": (N.RCA_Q8_0, N.Q8Blocks, 32, 34, G.GGML_Q8_0), "q4_k": (N.RCA_Q4_K, N.Q4KBlocks, 256, 144, G.GGML_Q4_K),
         "q5_k": (N.RCA_Q5_K, N.Q5KBlocks, 256, 176, G.GGML_Q5_K), "q6_k": (N.RCA_Q6_K, N.Q6KBlocks, 256, 210, G.GGML_Q6_K)}
RULES = {"minmax": 0, "search": 1}
RECIPES = ("q8_0", "q4_k", "q5_k", "q6_k", "q4_k_m", "q5_k_m")
# general.file_type (llama.cpp's llama_ftype): MOSTLY_Q8_0 7, Q4_K_S 14 (the nearest name for "every matrix Q4_K"), Q4_K_M 15, Q5_K_S 16,
# Q5_K_M 17, Q6_K 18; F32 0, F16 1, BF16 32
FILE_TYPE = {"q8_0": 7, "q4_k": 14, "q4_k_m": 15, "q5_k": 16, "q5_k_m": 17, "q6_k": 18}
GGUF_NAMES = {"self_attn.q_proj": "attn_q", "self_attn.k_proj": "attn_k", "self_attn.v_proj": "attn_v", "self_attn.o_proj": "attn_output",
              "mlp.gate_proj": "ffn_gate", "mlp.up_proj": "ffn_up", "mlp.down_proj": "ffn_down", "input_layernorm": "attn_norm",
              "post_attention_layernorm": "ffn_norm"}


def use_more_bits(i_layer: int, n_layers: int) -> bool:
    """llama.cpp's use_more_bits: the first and the last eighth of the layers and every third in between"""
    return i_layer < n_layers // 8 or i_layer >= 7 * n_layers // 8 or (i_layer - n_layers // 8) % 3 == 2


def recipe_type(gguf_name: str, n_layers: int, recipe: str) -> str:
    """The type a matrix gets under a recipe, by its GGUF tensor name."""
    if recipe not in RECIPES:
        raise ValueError(f"recipe {recipe!r}: one of {', '.join(RECIPES)}")
    if recipe in TYPES:
        return recipe
    base = "q4_k" if recipe == "q4_k_m" else "q5_k"
    if gguf_name == "output.weight":
        return "q6_k"
    if ".attn_v." in gguf_name or ".ffn_down." in gguf_name:
        return "q6_k" if use_more_bits(int(gguf_name.split(".")[1]), n_layers) else base
    return base


def gguf_name(hf_name: str) -> str:
    """HF tensor name -> GGUF tensor name (llama architecture)"""
    fixed = {"model.embed_tokens.weight": "token_embd.weight", "model.norm.weight": "output_norm.weight", "lm_head.weight": "output.weight"}
    if hf_name in fixed:
        return fixed[hf_name]
    p = hf_name.split(".")          # model.layers.<l>.<block>.<proj>.weight
    if len(p) == 6 and p[0] == "model" and p[1] == "layers" and f"{p[3]}.{p[4]}" in GGUF_NAMES:
        return f"blk.{p[2]}.{GGUF_NAMES[p[3] + '.' + p[4]]}.weight"
    if len(p) == 5 and p[0] == "model" and p[1] == "layers" and p[3] in GGUF_NAMES:
        return f"blk.{p[2]}.{GGUF_NAMES[p[3]]}.weight"
    raise ValueError(f"tensor {hf_name!r} has no place in a llama-architecture GGUF")


def quantize_matrix(w: np.ndarray, type: str, rule: str = "search", device: int = 0, name: str = "tensor",
                    col_weights: Optional[np.ndarray] = None):
    """w [N, K] (float32, float16, or uint16 holding bf16 bits; K % 256 == 0) -> the _native blocks object of `type` ("q8_0", "q4_k", "q5_k",
    "q6_k": Q8Blocks / Q4KBlocks / Q5KBlocks / Q6KBlocks, what the GGUF loader produces for such a tensor), quantised on `device`.
    A value that is not finite, or a block whose d / dmin is not finite in fp16, is refused (RcaError naming `name` and the row).
    col_weights: one non-negative float32 per input column [K] -> the weighted rules (rule "search" only; "q8_0" ignores them)."""
    if type not in TYPES:
        raise ValueError(f"type {type!r}: one of {', '.join(TYPES)}")
    if rule not in RULES:
        raise ValueError(f"rule {rule!r}: 'search' or 'minmax'")
    w = np.asarray(w)
    if w.ndim != 2:
        raise ValueError(f"{name}: a matrix is needed, got shape {w.shape}")
    if w.dtype == np.uint16:
        dt = N.RCA_BF16
    elif w.dtype == np.float16:
        dt = N.RCA_F16
    else:
        w, dt = w.astype(np.float32, copy=False), N.RCA_F32
    w = np.ascontiguousarray(w)
    rows, K = w.shape
    rca_type, cls, nv, nbytes, _ = TYPES[type]
    if K % 256:
        raise N.RcaError(f"{name}: K = {K} is not a multiple of 256")
    out = np.empty((rows, K // nv * nbytes), np.uint8)
    entry = "rca_quantize_rows" if col_weights is None else "rca_quantize_rows_w"
    if col_weights is None:
        rc = N.lib().rca_quantize_rows(int(device), w.ctypes.data, dt, rows, K, rca_type, RULES[rule], out.ctypes.data, out.nbytes)
    else:
        qw = np.ascontiguousarray(col_weights, np.float32)
        if qw.shape != (K,):
            raise ValueError(f"{name}: {qw.shape} column weights for K = {K}")
        rc = N.lib().rca_quantize_rows_w(int(device), w.ctypes.data, dt, rows, K, rca_type, RULES[rule], qw.ctypes.data, out.ctypes.data, out.nbytes)
    if rc != 0:
        msg = N.lib().rca_last_error()
        raise N.RcaError(f"{name}: {entry} failed (rc={rc}): {msg.decode(errors='replace') if msg else ''}")
    return cls(out, (rows, K))


class QuantizedWeights(dict):
    """The weights dict of quantize_weights: HF names -> blocks objects (matrices), float16 (matrices no type could take) and float32 arrays.
    `recipe` and `types` (HF name -> type name) ride along for write_llama_gguf and for reports."""
    recipe: Optional[str] = None
    types: Dict[str, str]
    seconds: Dict[str, float]
    imatrix_meta: Optional[Dict[str, Any]] = None       # the quantize.imatrix.* keys write_llama_gguf adds (quantised under an imatrix)


def _to_f32(a: np.ndarray) -> np.ndarray:
    a = np.asarray(a)
    if a.dtype == np.uint16:
        return (a.astype(np.uint32) << 16).view(np.float32)
    return a.astype(np.float32)


def imatrix_vector(imatrix, name: str) -> Optional[np.ndarray]:
    """The column weights of GGUF tensor `name` under an importance matrix {name: (in_sum2 [K], count)}: float32(in_sum2 / count), or None
    where it has no entry (or no token was collected)."""
    e = imatrix.get(name)
    if e is None or int(e[1]) <= 0:
        return None
    return (np.asarray(e[0], np.float64).reshape(-1) / float(int(e[1]))).astype(np.float32)


def quantize_weights(cfg, weights: Dict[str, Any], recipe: str, rule: str = "search", device: int = 0,
                     quantize_matrix: Callable = quantize_matrix, report: Optional[Callable[[str], None]] = None,
                     imatrix: Optional[Dict[str, Any]] = None) -> QuantizedWeights:
    """cfg: LMConfig; weights: HF-named arrays (float32 / float16 / bf16 bits; a missing lm_head.weight is tied to the embedding table) ->
    a weights dict LlamaForAlternatingCodeChannels(weights=..., config=cfg) takes as it is.  A source that is already quantised (blocks
    objects) is refused.  quantize_matrix: the matrix quantiser (tests substitute a host one).
    imatrix: {GGUF tensor name: (in_sum2 [K], count)} (imatrix.read_imatrix_gguf): every matrix with an entry is quantised
    under the column weights float32(in_sum2 / count) (rule "search" only).  The embedding table has no vector by construction; any other
    matrix without an entry is quantised unweighted with one warning naming it; a vector whose length is not the matrix's K is refused
    before any work."""
    if recipe not in RECIPES:
        raise ValueError(f"recipe {recipe!r}: one of {', '.join(RECIPES)}")
    out = QuantizedWeights()
    out.recipe, out.types, out.seconds = recipe, {}, {}
    src = dict(weights)
    if "lm_head.weight" not in src:
        src["lm_head.weight"] = src["model.embed_tokens.weight"]
    for k, v in src.items():          # before any work
        if k.startswith("model.embed_codec_tokens."):
            raise ValueError(f"{k}: the checkpoint was saved before persist_codec_embeddings; persist the codec embeddings into the table "
                             "first (a quantised table cannot take them afterwards)")
        if hasattr(v, "dequantize"):
            raise ValueError(f"{k} is already quantised ({type(v).__name__}): re-quantising a quantised source is not supported")
    vectors: Dict[str, np.ndarray] = {}
    if imatrix is not None:
        if rule != "search":
            raise ValueError(f"an importance matrix needs rule 'search', not {rule!r}")
        for k, v in src.items():
            if k == "rope.inv_freq" or k.startswith("codec.") or np.asarray(v).ndim != 2:
                continue
            qw = imatrix_vector(imatrix, gguf_name(k))
            if qw is not None:
                if qw.shape != (np.asarray(v).shape[1],):
                    raise ValueError(f"{k}: the importance matrix holds {qw.shape[0]} columns for {gguf_name(k)}, the matrix has K = {np.asarray(v).shape[1]}")
                if not np.all(np.isfinite(qw)) or np.any(qw < 0):
                    raise ValueError(f"{k}: the importance matrix's vector for {gguf_name(k)} holds a value that is negative or not finite")
                vectors[k] = qw
        out.imatrix_meta = {"quantize.imatrix.file": str(getattr(imatrix, "file", "") or ""),
                            "quantize.imatrix.dataset": str((list(getattr(imatrix, "datasets", [])) or [""])[0]),
                            "quantize.imatrix.entries_count": int(len(imatrix)),
                            "quantize.imatrix.chunks_count": int(getattr(imatrix, "chunk_count", 0) or 0)}
    for k, v in src.items():
        if k == "rope.inv_freq" or k.startswith("codec."):
            out[k] = v
            continue
        a = np.asarray(v)
        if a.ndim != 2:
            out[k] = _to_f32(a)
            continue
        t = recipe_type(gguf_name(k), cfg.n_layers, recipe)
        rows, K = a.shape
        if K % 256 or rows % 4:
            warnings.warn(f"{k} is {rows} x {K} (K must be a multiple of 256, N of 4 for {t}): it stays F16")
            out[k], out.types[k] = (a if a.dtype == np.float16 else _to_f32(a).astype(np.float16)), "f16"
            continue
        t0 = time.perf_counter()
        if k in vectors:
            out[k] = quantize_matrix(a, t, rule=rule, device=device, name=k, col_weights=vectors[k])
        else:
            if imatrix is not None and k != "model.embed_tokens.weight":
                warnings.warn(f"{k} ({gguf_name(k)}) has no entry in the importance matrix: it is quantised unweighted")
            out[k] = quantize_matrix(a, t, rule=rule, device=device, name=k)
        out.seconds[k] = time.perf_counter() - t0
        out.types[k] = t
        if report:
            nb = out[k].raw.nbytes
            report(f"{gguf_name(k):28s} {rows:7d} x {K:5d}  {t:5s} {nb:12d} bytes  {8.0 * nb / a.size:6.3f} bpw  {out.seconds[k]:7.3f} s")
    return out


# ------------------------------------------------------------------------------------------------------------------ the writer
def _s(b: bytes) -> bytes:
    return struct.pack("<Q", len(b)) + b


_INT_RANGES = ((G._U32, 0, 1 << 32), (G._I32, -(1 << 31), 1 << 31), (G._U64, 0, 1 << 64), (G._I64, -(1 << 63), 1 << 63))
_NP_TO_GGUF = {np.dtype(v): k for k, v in G._NP.items()}


def _value(v) -> bytes:
    """one metadata value with its type tag.  Scalars read back by gguf.read_gguf have lost their width: an int is written as the
    narrowest of u32 / i32 / u64 / i64 that holds it, a float as f32; arrays keep their element type."""
    if isinstance(v, (bool, np.bool_)):
        return struct.pack("<I?", G._BOOL, bool(v))
    if isinstance(v, (int, np.integer)):
        for t, lo, hi in _INT_RANGES:
            if lo <= int(v) < hi:
                return struct.pack("<I", t) + struct.pack(G._SCALAR[t], int(v))
        raise ValueError(f"integer {v} does not fit a GGUF value")
    if isinstance(v, (float, np.floating)):
        return struct.pack("<If", G._F32, float(v))
    if isinstance(v, (str, bytes)):
        return struct.pack("<I", G._STR) + _s(v.encode() if isinstance(v, str) else v)
    if isinstance(v, np.ndarray):
        if v.dtype not in _NP_TO_GGUF:
            raise ValueError(f"array of {v.dtype} does not fit a GGUF value")
        return struct.pack("<IIQ", G._ARR, _NP_TO_GGUF[v.dtype], v.size) + np.ascontiguousarray(v).tobytes()
    if isinstance(v, (list, tuple)):
        if all(isinstance(x, str) for x in v):
            return struct.pack("<IIQ", G._ARR, G._STR, len(v)) + b"".join(_s(x.encode()) for x in v)
        items = [_value(x) for x in v]
        tags = {it[:4] for it in items}
        if len(tags) > 1:
            raise ValueError("a GGUF array holds one element type")
        tag = tags.pop() if tags else struct.pack("<I", G._U32)
        return struct.pack("<I", G._ARR) + tag + struct.pack("<Q", len(v)) + b"".join(it[4:] for it in items)
    raise ValueError(f"metadata value of type {type(v).__name__} does not fit a GGUF value")


def permute_rows(n_rows: int, n_head: int) -> np.ndarray:
    """row index of convert_hf_to_gguf.py's LlamaModel.permute (rotate-half rows -> interleaved pairs): out = w[index]"""
    return np.arange(n_rows).reshape(n_head, 2, n_rows // n_head // 2).swapaxes(1, 2).reshape(-1)


def rope_freq_factors(cfg, inv_freq: np.ndarray) -> np.ndarray:
    """The rope_freqs.weight a reader divides the plain frequencies by: factors f with float32(base / f) == inv_freq bit for bit where one
    exists within a few ulps of base / inv_freq (gguf.load_llama_gguf computes exactly that quotient), f32(base / inv_freq) otherwise:
    one f32 step of f can move the quotient by more than an ulp, so a few frequencies come back one ulp off."""
    import dataclasses
    from .llm import rope_inv_freq
    base = rope_inv_freq(dataclasses.replace(cfg, rope_scaling=None))
    inv = np.asarray(inv_freq, np.float32).reshape(-1)
    f = (base / inv).astype(np.float32)
    best = f.copy()
    done = (base / best).astype(np.float32) == inv
    for k in range(1, 9):
        for cand in (f.view(np.int32) + k, f.view(np.int32) - k):
            c = cand.astype(np.int32).view(np.float32)
            hit = ~done & ((base / c).astype(np.float32) == inv)
            best = np.where(hit, c, best)
            done |= hit
    return best.astype(np.float32)


def _tensor_type(a):
    """-> (GGUF tensor type, bytes it takes) of one tensor as it is stored"""
    if hasattr(a, "raw"):
        for _rca, cls, _nv, _nb, gg in TYPES.values():
            if type(a) is cls:
                return gg, int(a.raw.nbytes)
        raise ValueError(f"{type(a).__name__} tensors cannot be written")
    a = np.asarray(a)
    if a.dtype == np.float16:
        return G.GGML_F16, 2 * a.size
    if a.dtype == np.uint16:
        return G.GGML_BF16, 2 * a.size
    return G.GGML_F32, 4 * a.size


def _tensor_bytes(a) -> bytes:
    if hasattr(a, "raw"):
        return np.ascontiguousarray(a.raw).tobytes()
    a = np.asarray(a)
    return np.ascontiguousarray(a if a.dtype in (np.float16, np.uint16) else a.astype(np.float32, copy=False)).tobytes()


def write_llama_gguf(path: str, cfg, weights: Dict[str, Any], meta: Optional[Dict[str, Any]] = None, file_type: Optional[int] = None) -> int:
    """A llama-architecture GGUF v3 file of `weights` (HF names: quantize_weights' result, or plain float32 / float16 / bf16-bit arrays), laid
    out as convert_hf_to_gguf.py lays one out: reversed dims, q_proj / k_proj rows permuted to interleaved pairs, llama3 rope scaling as
    a rope_freqs.weight tensor, data aligned to 32 bytes -- gguf.load_llama_gguf undoes all of it.  meta: metadata to copy through (the
    third result of gguf.load_llama_gguf: that is how a tokenizer survives); the keys this writer owns (architecture, alignment, the
    llama.* dimensions, general.file_type) are replaced.  general.file_type: FILE_TYPE of the weights' recipe (7 / 15 / 17 for q8_0 /
    q4_k_m / q5_k_m), 1 / 32 / 0 for F16 / BF16 / F32 matrices, or `file_type`.  Returns the bytes written."""
    from .llm import CODEC_PREFIX, rope_inv_freq
    if any(k.startswith(CODEC_PREFIX) for k in weights):
        raise ValueError(f"the checkpoint still carries {CODEC_PREFIX}* (saved before persist_codec_embeddings): a llama-architecture GGUF "
                         "has no place for the codec projector; persist the embeddings into the table first")
    lm_head = weights.get("lm_head.weight", weights["model.embed_tokens.weight"])
    if file_type is None:
        recipe = getattr(weights, "recipe", None)
        if recipe is not None:
            file_type = FILE_TYPE[recipe]
        else:
            gg = _tensor_type(lm_head)[0] if not hasattr(lm_head, "raw") else None
            file_type = {G.GGML_F16: 1, G.GGML_BF16: 32, G.GGML_F32: 0}.get(gg)
            if file_type is None:
                raise ValueError("general.file_type cannot be told from these weights: pass file_type=")
    own = {"general.architecture": "llama", "general.alignment": 32, "general.file_type": int(file_type),
           "llama.embedding_length": cfg.hidden, "llama.block_count": cfg.n_layers, "llama.attention.head_count": cfg.n_heads,
           "llama.attention.head_count_kv": cfg.n_kv_heads, "llama.feed_forward_length": cfg.ffn, "llama.rope.dimension_count": cfg.head_dim,
           "llama.vocab_size": cfg.vocab_size, "llama.attention.layer_norm_rms_epsilon": float(cfg.rms_eps), "llama.rope.freq_base": float(cfg.rope_theta)}
    kv = dict(own)
    kv.setdefault("llama.context_length", int((meta or {}).get("llama.context_length", 131072 if cfg.rope_scaling else 2048)))
    for k, v in (meta or {}).items():
        if k not in kv and k != "gguf.version" and not k.startswith("quantize.imatrix."):
            kv[k] = v
    kv.update(getattr(weights, "imatrix_meta", None) or {})
    ts = [("token_embd.weight", weights["model.embed_tokens.weight"]), ("output_norm.weight", _to_f32(weights["model.norm.weight"])),
          ("output.weight", lm_head)]
    inv = weights.get("rope.inv_freq")
    if inv is None and cfg.rope_scaling:
        inv = rope_inv_freq(cfg)
    if inv is not None:
        f = rope_freq_factors(cfg, inv)
        if np.any(f != 1.0):
            ts.append(("rope_freqs.weight", f))
    for l in range(cfg.n_layers):
        for hf, gg in GGUF_NAMES.items():
            a = weights[f"model.layers.{l}.{hf}.weight"]
            if gg in ("attn_q", "attn_k"):
                idx = permute_rows(a.shape[0], cfg.n_heads if gg == "attn_q" else cfg.n_kv_heads)
                a = a.take_rows(idx) if hasattr(a, "take_rows") else np.asarray(a)[idx]
            elif not hasattr(a, "raw") and np.asarray(a).ndim == 1:
                a = _to_f32(a)
            ts.append((f"blk.{l}.{gg}.weight", a))
    infos, off, sizes = [], 0, []
    for name, a in ts:
        gg, nbytes = _tensor_type(a)
        ne = list(reversed(a.shape))
        infos.append(_s(name.encode()) + struct.pack("<I", len(ne)) + b"".join(struct.pack("<Q", d) for d in ne) + struct.pack("<IQ", gg, off))
        sizes.append(nbytes)
        off += nbytes + (-nbytes) % 32
    head = struct.pack("<IIQQ", G.GGUF_MAGIC, 3, len(ts), len(kv)) + b"".join(_s(k.encode()) + _value(v) for k, v in kv.items()) + b"".join(infos)
    total = 0
    with open(path, "wb") as fh:
        total += fh.write(head + b"\0" * ((-len(head)) % 32))
        for (name, a), nbytes in zip(ts, sizes):       # one tensor in memory at a time
            data = _tensor_bytes(a)
            assert len(data) == nbytes, name
            total += fh.write(data + b"\0" * ((-nbytes) % 32))
    return total


# ------------------------------------------------------------------------------------------------------------------ sources and the CLI
def load_source(path: str):
    """-> (LMConfig, HF-named weights, metadata or None) of an HF directory, an .npz or a GGUF whose matrices are F32 / F16 / BF16.  A GGUF
    that holds a quantised tensor is refused: re-quantising is not supported."""
    from .llm import load_weights
    if path.endswith(".gguf"):
        _, raw = G.read_gguf(path, keep_q8_0=True)
        packed = sorted(k for k, v in raw.items() if hasattr(v, "dequantize"))
        if packed:
            raise G.GGUFError(f"{path}: {packed[0]} (and {len(packed) - 1} more) is already quantised ({type(raw[packed[0]]).__name__}): "
                              "the source must hold F32 / F16 / BF16 matrices")
        del raw
        cfg, w, meta = G.load_llama_gguf(path)
        return cfg, w, meta
    cfg, w = load_weights(path)
    return cfg, w, None


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(prog="python -m realtime_codec_agent_amd.quantize", description=__doc__.split("\n\n")[0])
    ap.add_argument("--model", required=True, help="HF directory, .npz, or a GGUF whose matrices are F32 / F16 / BF16")
    ap.add_argument("--out", required=True, help="the GGUF file to write")
    ap.add_argument("--type", required=True, choices=RECIPES)
    ap.add_argument("--rule", default="search", choices=sorted(RULES))
    ap.add_argument("--imatrix", default=None, help="an importance matrix (a GGUF imatrix file): weighted search")
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args(argv)
    if a.imatrix is not None and a.rule != "search":
        ap.error("--imatrix needs --rule search")
    imx = None
    if a.imatrix is not None:
        from .imatrix import read_imatrix_gguf
        imx = read_imatrix_gguf(a.imatrix)
        print(f"{a.imatrix}: {len(imx)} entries, {imx.chunk_count} chunks of {imx.chunk_size} tokens")
    t0 = time.perf_counter()
    cfg, w, meta = load_source(a.model)
    t1 = time.perf_counter()
    print(f"{a.model}: {cfg.n_layers} layers, hidden {cfg.hidden}, vocab {cfg.vocab_size}; loaded in {t1 - t0:.2f} s")
    q = quantize_weights(cfg, w, a.type, rule=a.rule, device=a.device, report=print, imatrix=imx)
    t2 = time.perf_counter()
    n_val = sum(int(np.prod(v.shape)) for k, v in q.items() if k in q.types)
    n_bytes = sum((v.raw.nbytes if hasattr(v, "raw") else v.nbytes) for k, v in q.items() if k in q.types)
    total = write_llama_gguf(a.out, cfg, q, meta=meta)
    t3 = time.perf_counter()
    print(f"{a.type} ({a.rule}): {n_bytes} bytes for {n_val} weights, {8.0 * n_bytes / max(n_val, 1):.3f} bits per weight; "
          f"quantised in {t2 - t1:.2f} s ({sum(q.seconds.values()):.2f} s in the quantiser), {a.out}: {total} bytes written in {t3 - t2:.2f} s")
    return 0


if __name__ == "__main__":
    sys.exit(main())
