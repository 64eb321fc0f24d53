"""LlamaForAlternatingCodeChannels -- the LM step object of the duplex loop.

Same control surface as the reference subclass of llama_cpp.Llama
(realtime_codec_agent/utils/llamacpp_utils.py:26-181) for every member the agent uses
(SURVEY.md 8b-3): reset, eval, generate(tokens, reset=False), sample, read/WRITE n_tokens,
init_sampler_for_generate, set_seed, get_logprobs, logits_to_logprobs, _ctx.get_logits(),
_n_vocab, _scores, model_path, n_ctx().  The forward pass, KV cache and sampler live behind the
C ABI (include/rca.h, rca_lm_*) as HIP kernels; there is no CPU fallback.

The model is a vanilla Llama (codec_llama.py after persist_codec_embeddings, codec_llama.py:178-206).
`model_path` may name a directory holding config.json + *.safetensors, an .npz written by
`save_npz`, or the literal "random:<name>" for seeded random-init weights generated on the device
(bench configs 3/4: no checkpoint exists offline).
"""
from __future__ import annotations

import ctypes as C
import json
import math
import os
from dataclasses import asdict, dataclass
from typing import Dict, Generator, List, Optional, Sequence

import numpy as np

from . import _native as N


@dataclass
class LMConfig:
    vocab_size: int = 259344
    hidden: int = 2048
    n_layers: int = 16
    n_heads: int = 32
    n_kv_heads: int = 8
    head_dim: int = 64
    ffn: int = 8192
    rms_eps: float = 1e-5
    rope_theta: float = 500000.0
    rope_scaling: Optional[str] = "llama3"  # None | "llama3"
    rope_factor: float = 32.0
    rope_low_freq_factor: float = 1.0
    rope_high_freq_factor: float = 4.0
    rope_orig_ctx: int = 8192

    @staticmethod
    def llama_3_2_1b(vocab_size: int = 259344) -> "LMConfig":
        """Llama-3.2-1B dims with the codec vocabulary."""
        return LMConfig(vocab_size=vocab_size)

    @staticmethod
    def from_hf(d: dict) -> "LMConfig":
        rp = d.get("rope_parameters") or d.get("rope_scaling") or {}
        theta = rp.get("rope_theta", d.get("rope_theta", 10000.0))
        rtype = rp.get("rope_type", rp.get("type", "default"))
        nh = d["num_attention_heads"]
        return LMConfig(
            vocab_size=d["vocab_size"], hidden=d["hidden_size"], n_layers=d["num_hidden_layers"], n_heads=nh,
            n_kv_heads=d.get("num_key_value_heads", nh), head_dim=d.get("head_dim") or d["hidden_size"] // nh,
            ffn=d["intermediate_size"], rms_eps=d.get("rms_norm_eps", 1e-5), rope_theta=float(theta),
            rope_scaling="llama3" if rtype == "llama3" else None, rope_factor=float(rp.get("factor", 32.0)),
            rope_low_freq_factor=float(rp.get("low_freq_factor", 1.0)), rope_high_freq_factor=float(rp.get("high_freq_factor", 4.0)),
            rope_orig_ctx=int(rp.get("original_max_position_embeddings", 8192)),
        )

    def n_params(self) -> int:
        per_layer = self.hidden * (self.n_heads + 2 * self.n_kv_heads) * self.head_dim + self.n_heads * self.head_dim * self.hidden \
            + 3 * self.hidden * self.ffn
        return self.n_layers * per_layer + 2 * self.vocab_size * self.hidden

    def weight_bytes_per_step(self) -> int:
        """bf16 bytes streamed by one decode step: all layer weights + lm_head (embedding rows are gathered)."""
        return 2 * (self.n_params() - self.vocab_size * self.hidden)


def rope_inv_freq(cfg: LMConfig) -> np.ndarray:
    """inv_freq exactly as transformers computes it in float32 (default and llama3 scaling)."""
    import torch
    dim = cfg.head_dim
    inv = 1.0 / (cfg.rope_theta ** (torch.arange(0, dim, 2, dtype=torch.int64).to(dtype=torch.float) / dim))
    if cfg.rope_scaling == "llama3":
        factor, low, high, old = cfg.rope_factor, cfg.rope_low_freq_factor, cfg.rope_high_freq_factor, cfg.rope_orig_ctx
        low_wl, high_wl = old / low, old / high
        wl = 2 * math.pi / inv
        inv_l = torch.where(wl > low_wl, inv / factor, inv)
        smooth = (old / wl - low) / (high - low)
        smoothed = (1 - smooth) * inv_l / factor + smooth * inv_l
        medium = ~(wl < high_wl) * ~(wl > low_wl)
        inv = torch.where(medium, smoothed, inv_l)
    return inv.numpy().astype(np.float32)


def f32_to_bf16_bits(a: np.ndarray) -> np.ndarray:
    """float32 -> bf16 bit pattern (round to nearest even) as uint16."""
    u = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def bf16_bits_to_f32(b: np.ndarray) -> np.ndarray:
    return (b.astype(np.uint32) << 16).view(np.float32)


ACTIVATION_FORMATS = ("f32", "q8_1")          # rca_lm_set_act_format's 0 / 1
KV_FORMATS = ("f16", "q8_0")                  # rca_lm_set_kv_format's 0 / 1
# the library's format ids, as rca_lm_weight_format reports them (4: a file whose gate / up tensors are Q6_K, llama-quantize Q6_K) ...
WEIGHT_FORMAT_NAMES = ("bf16", "q8_0", "f16", "q4_k", "q6_k", "q5_k", "q4_0", "q4_1", "iq4_nl", "iq4_xs")
# ... and rca_lm_config_t::decode_weights, the load-time conversions of a 16-bit checkpoint (0: as supplied)
DECODE_WEIGHTS = {"q8_0": 1, "f16": 2, "q4_k": 3, "q5_k": 4, "q4_0": 5, "q4_1": 6, "iq4_nl": 7}
CODEC_PREFIX = "model.embed_codec_tokens."   # CodecLlamaCodecEmbedding's tensors (codec_llama.py:46-69)


def lm_tensor_names(cfg: LMConfig) -> List[str]:
    names = ["model.embed_tokens.weight", "model.norm.weight", "lm_head.weight"]
    for l in range(cfg.n_layers):
        p = f"model.layers.{l}."
        names += [p + s for s in ("self_attn.q_proj.weight", "self_attn.k_proj.weight", "self_attn.v_proj.weight",
                                  "self_attn.o_proj.weight", "mlp.gate_proj.weight", "mlp.up_proj.weight", "mlp.down_proj.weight",
                                  "input_layernorm.weight", "post_attention_layernorm.weight")]
    return names


def save_npz(path: str, cfg: LMConfig, weights: Dict[str, np.ndarray]) -> None:
    np.savez(path, __config__=np.array(json.dumps(asdict(cfg))), **{k: v for k, v in weights.items()})


def load_weights(model_path: str):
    """-> (LMConfig, {name: ndarray}) from an .npz (save_npz), a llama-architecture .gguf (the reference's format,
    realtime_agent_resources.py:12,19-25) or an HF directory with safetensors."""
    if model_path.endswith(".gguf"):
        from .gguf import load_llama_gguf
        cfg, weights, _meta = load_llama_gguf(model_path)
        return cfg, weights
    if model_path.endswith(".npz"):
        z = np.load(model_path)
        cfg = LMConfig(**json.loads(str(z["__config__"])))
        return cfg, {k: z[k] for k in z.files if k != "__config__"}
    d = model_path if os.path.isdir(model_path) else os.path.dirname(model_path)
    with open(os.path.join(d, "config.json")) as f:
        cfg = LMConfig.from_hf(json.load(f))
    from safetensors import safe_open
    import torch
    weights = {}
    for fn in sorted(os.listdir(d)):
        if fn.endswith(".safetensors"):
            with safe_open(os.path.join(d, fn), framework="pt") as sf:
                for k in sf.keys():
                    t = sf.get_tensor(k)
                    if t.dtype == torch.bfloat16:
                        weights[k] = t.view(torch.int16).numpy().view(np.uint16)
                    elif t.dtype == torch.float16 and t.dim() == 2:   # fp16 matrices stay fp16 on the device (RCA_F16)
                        weights[k] = t.numpy()
                    else:
                        weights[k] = t.float().numpy()
    if "lm_head.weight" not in weights:  # tied checkpoints
        weights["lm_head.weight"] = weights["model.embed_tokens.weight"]
    if CODEC_PREFIX + "codec_embed.weight" in weights:
        # a CodecLlamaForCausalLM checkpoint saved BEFORE persist_codec_embeddings (codec_llama.py:178-206): the constructor
        # bakes the projected codec embeddings into the table on the device
        with open(os.path.join(d, "config.json")) as f:
            hf = json.load(f)
        if hf.get("projector_hidden_act", "gelu") != "gelu":
            raise NotImplementedError(f"projector_hidden_act={hf['projector_hidden_act']!r}: only the reference default 'gelu' is built")
        weights["codec.vocab_start"] = np.array(int(hf.get("codec_vocab_start", 0)))
        weights["codec.codebook_size"] = np.array(int(hf.get("codebook_size", 131072)))
    return cfg, weights


class _Ctx:
    """llm._ctx.get_logits(): a C float* over the last logits (realtime_agent_v2.py:449,461)."""

    def __init__(self, llm: "LlamaForAlternatingCodeChannels"):
        self._llm = llm

    def get_logits(self):
        buf = self._llm._fetch_logits()
        return buf.ctypes.data_as(C.POINTER(C.c_float))

    def kv_cache_seq_rm(self, seq_id: int, p0: int, p1: int) -> None:
        # stale slots are simply overwritten by the next eval
        return None


class LlamaForAlternatingCodeChannels:
    def __init__(
        self,
        model_path: Optional[str] = None,
        n_ctx: int = 16384,
        n_gpu_layers: int = -1,
        verbose: bool = False,
        flash_attn: bool = True,
        logits_all: bool = False,
        seed: int = 0xFFFFFFFF,
        *,
        config: Optional[LMConfig] = None,
        weights: Optional[Dict[str, np.ndarray]] = None,
        device: Optional[int] = None,
        random_seed: int = 0,
        init_std: float = 0.02,
        share_weights_with: Optional["LlamaForAlternatingCodeChannels"] = None,
        weight_format: Optional[str] = None,
        activation_format: Optional[str] = None,
        kv_format: Optional[str] = None,
        kv_shift_requant: Optional[bool] = None,
        **_ignored,
    ):
        """weight_format: the format every projection matrix and lm_head is KEPT in (one copy: the decode step streams it, the prefill
        tiles de-quantise it while staging).  None = as the checkpoint supplies it (bf16 / fp16 / Q8_0 tensors keep their format, f32 is
        rounded to bf16); "q8_0" = quantised at load like the Q8_0 file the reference deploys (prep_test_model.sh:29); "f16" = bf16
        values converted to fp16 (the F16 file of prep_test_model.sh:28, the reference's default model); "q4_k" = GGUF Q4_K blocks
        (the bulk of the Q4_K_M file of prep_test_model.sh:31), quantised at load with this build's own min / max rule; "q5_k" = the same
        rule into GGUF Q5_K blocks (the bulk of a Q5_K_S / Q5_K_M file), 31 steps per sub-block instead of 15; "q4_0" / "q4_1" = the legacy
        4-bit GGUF blocks of 32 values, quantised at load by ggml's reference rule (the bulk of a llama-quantize Q4_0 file; the
        importance-matrix search of llama-quantize is not part of it); "iq4_nl" = GGUF IQ4_NL blocks (32 values: an fp16 step and 4-bit
        indices into the 16-entry non-linear table kvalues_iq4nl), quantised at load by this build's plain rule -- d = fp16(max / -127)
        with max the value of largest magnitude, every value to the nearest d * kv[i] -- which is NOT llama-quantize's result (an
        iterative weighted search); it exists so that random: models and bf16 checkpoints run in the format.  IQ4_XS comes from files only.
        activation_format: what the decode GEMVs over quantised (q8_0 / Q4_K / Q5_K / Q6_K / Q4_0 / Q4_1 / IQ4_NL / IQ4_XS) matrices multiply the weights with.  None / "f32"
        (default) = f32 activations; "q8_1" = activations quantised to 32-value int8 blocks inside the GEMV and integer dot products,
        the arithmetic class of llama.cpp's GPU mat-vec (set_activation_format).  A twin inherits its parent's.
        kv_format: what the KV cache holds.  None / "f16" (default) = fp16 rows; "q8_0" = ggml q8_0 blocks, 68 bytes per head row instead
        of 128 (llama-cpp-python's type_k = type_v = GGML_TYPE_Q8_0 next to flash_attn=True; set_kv_format).  A twin inherits its parent's.
        kv_shift_requant: True lets kv_remove / kv_remove_many shift a "q8_0" cache by de-quantising, rotating and RE-QUANTISING the moved
        keys (llama.cpp's K-shift on --cache-type-k q8_0; set_kv_shift_requant).  None / False (default): a "q8_0" handle refuses the
        shift.  Needs kv_format="q8_0"; a twin inherits its parent's."""
        if kv_format not in (None,) + KV_FORMATS:
            raise ValueError(f"kv_format {kv_format!r}: None / 'f16' or 'q8_0'")
        if kv_shift_requant and share_weights_with is None and kv_format != "q8_0":
            raise ValueError(f"kv_shift_requant=True needs kv_format='q8_0' (got {kv_format!r}): the shift of an fp16 cache quantises nothing")
        if activation_format not in (None,) + ACTIVATION_FORMATS:
            raise ValueError(f"activation_format {activation_format!r}: None / 'f32' or 'q8_1'")
        if weight_format not in (None, "bf16") + tuple(DECODE_WEIGHTS):
            raise ValueError(f"weight_format {weight_format!r}: None / 'bf16' (as supplied), 'q8_0', 'f16', 'q4_k', 'q5_k', 'q4_0', 'q4_1' or 'iq4_nl'")
        self._lib = N.lib()
        self.model_path = model_path
        self.verbose = verbose
        self.draft_model = None
        self._logits_all = bool(logits_all)
        if device is None:
            import torch
            if not torch.cuda.is_available():
                raise N.RcaError("LlamaForAlternatingCodeChannels needs a GPU; there is no CPU fallback")
            device = torch.cuda.current_device()
        self._device = device
        if share_weights_with is not None:
            # a second instance over the same device weights (the reference loads its GGUF twice: llm and the logits_all twin
            # aux_llm, realtime_agent_resources.py:19-33): own KV cache / sampler / stream, n_ctx <= the parent's
            parent = share_weights_with
            self.config = parent.config
            self._n_vocab = parent._n_vocab
            self._n_ctx = int(n_ctx)
            self._h = C.c_void_p()
            N.check(self._lib.rca_lm_create_shared(parent._h, self._n_ctx, 1 if logits_all else 0, C.byref(self._h)), "rca_lm_create_shared")
            self._weights_parent = parent   # (the library also copes with the parent being closed first)
            self._finish_init(seed)
            self.weight_format = parent.weight_format
            self.activation_format = self._query_activation_format()   # rca_lm_create_shared copied the parent's
            self._init_activation_format(activation_format)
            self.kv_format = self._query_kv_format()                   # and the parent's KV format
            self._init_kv_format(kv_format, kv_shift_requant)
            return
        random_init = weights is None and (model_path is None or str(model_path).startswith("random:"))
        if weights is None and not random_init:
            config, weights = load_weights(model_path)
        if config is None:
            config = LMConfig.llama_3_2_1b()
        self.config = config
        self._n_vocab = config.vocab_size
        self._n_ctx = int(n_ctx)
        c = N.LMConfigC(
            vocab_size=config.vocab_size, hidden=config.hidden, n_layers=config.n_layers, n_heads=config.n_heads,
            n_kv_heads=config.n_kv_heads, head_dim=config.head_dim, ffn=config.ffn, n_ctx=self._n_ctx, rms_eps=config.rms_eps,
            rope_theta=config.rope_theta, rope_scaling=1 if config.rope_scaling == "llama3" else 0, rope_factor=config.rope_factor,
            rope_low_freq_factor=config.rope_low_freq_factor, rope_high_freq_factor=config.rope_high_freq_factor,
            rope_orig_ctx=config.rope_orig_ctx, logits_all=1 if logits_all else 0, decode_weights=DECODE_WEIGHTS.get(weight_format, 0),
        )
        self._h = C.c_void_p()
        if random_init:
            N.check(self._lib.rca_lm_create_random(C.byref(c), C.c_uint64(random_seed), C.c_float(init_std), device, C.byref(self._h)),
                    "rca_lm_create_random")
        else:
            w = {k: v for k, v in weights.items() if not k.startswith((CODEC_PREFIX, "codec."))}
            w.setdefault("rope.inv_freq", rope_inv_freq(config))   # a GGUF brings the file's own frequencies
            tensors, keep = N.make_tensors(w)
            N.check(self._lib.rca_lm_create(C.byref(c), tensors, len(w), device, C.byref(self._h)), "rca_lm_create")
            del keep
            if CODEC_PREFIX + "codec_embed.weight" in weights:   # un-persisted checkpoint: bake the projector output now
                self.persist_codec_embeddings({k[len(CODEC_PREFIX):]: v for k, v in weights.items() if k.startswith(CODEC_PREFIX)},
                                              int(weights["codec.vocab_start"]), int(weights.get("codec.codebook_size", 0)) or None)
        self._finish_init(seed)
        self.weight_format = self._query_format()[0]
        self.activation_format = "f32"
        self._init_activation_format(activation_format)
        self.kv_format = "f16"
        self._init_kv_format(kv_format, kv_shift_requant)

    def _init_kv_format(self, kv_format: Optional[str], kv_shift_requant: Optional[bool] = None) -> None:
        try:
            if kv_format is not None:
                self.set_kv_format(kv_format)
            if kv_shift_requant is not None and (kv_shift_requant or self.kv_format == "q8_0"):
                self.set_kv_shift_requant(kv_shift_requant)
        except Exception:
            self.close()
            raise

    def _query_kv_format(self) -> str:
        fmt = C.c_int32()
        N.check(self._lib.rca_lm_get_kv_format(self._h, C.byref(fmt)), "rca_lm_get_kv_format")
        return KV_FORMATS[fmt.value]

    def set_kv_format(self, kv_format: str) -> None:
        """"f16" or "q8_0" (see the constructor).  Only an empty handle (n_tokens == 0) can change: the cache is re-allocated and captured
        graphs are dropped.  kv_remove (the context-shift trim) is refused on a "q8_0" handle unless set_kv_shift_requant(True) allows
        it; switching to "f16" clears that permission."""
        if kv_format not in KV_FORMATS:
            raise ValueError(f"kv_format {kv_format!r}: 'f16' or 'q8_0'")
        N.check(self._lib.rca_lm_set_kv_format(self._h, KV_FORMATS.index(kv_format)), "rca_lm_set_kv_format")
        self.kv_format = kv_format

    def set_kv_shift_requant(self, on: bool) -> None:
        """Allow (True) or refuse again (False) the context shift of this handle's "q8_0" cache (rca_lm_set_kv_shift_requant): kv_remove
        then de-quantises the moved keys, rotates them as on an fp16 cache and quantises them again -- every shift costs the surviving
        keys one q8_0 quantisation on top of the fp16 rounding.  A permission only, allowed at any n_tokens; an "f16" handle refuses it."""
        N.check(self._lib.rca_lm_set_kv_shift_requant(self._h, 1 if on else 0), "rca_lm_set_kv_shift_requant")

    @property
    def kv_shift_requant(self) -> bool:
        """whether kv_remove may shift this handle's "q8_0" cache, read from the library (a twin carries its parent's value)"""
        if not getattr(self, "_h", None):
            return False
        on = C.c_int32()
        N.check(self._lib.rca_lm_get_kv_shift_requant(self._h, C.byref(on)), "rca_lm_get_kv_shift_requant")
        return bool(on.value)

    def kv_bytes_per_position(self) -> int:
        """Bytes one cached position takes (all layers, K and V) in the handle's KV format."""
        b = C.c_int64()
        N.check(self._lib.rca_lm_kv_bytes_per_position(self._h, C.byref(b), None), "rca_lm_kv_bytes_per_position")
        return int(b.value)

    def kv_ring_positions(self) -> int:
        """Positions of the fp16 staging ring of a "q8_0" cache (0 for "f16"): tests pick passes that wrap it."""
        b, r = C.c_int64(), C.c_int32()
        N.check(self._lib.rca_lm_kv_bytes_per_position(self._h, C.byref(b), C.byref(r)), "rca_lm_kv_bytes_per_position")
        return int(r.value)

    def kv_read_q8(self, layer: int, pos0: int, n_pos: int):
        """Tests only (rca_lm_kv_read_q8): the raw blocks of a "q8_0" cache: (k_q, k_d, v_q, v_d), int8 [n_pos, n_kv_heads, 64] and
        float16 scales [n_pos, n_kv_heads, 2]."""
        nkv = self.config.n_kv_heads
        kq, vq = (np.empty((n_pos, nkv, 64), np.int8) for _ in range(2))
        kd, vd = (np.empty((n_pos, nkv, 2), np.float16) for _ in range(2))
        N.check(self._lib.rca_lm_kv_read_q8(self._h, int(layer), int(pos0), int(n_pos), kq.ctypes.data_as(C.POINTER(C.c_int8)),
                                            kd.ctypes.data_as(C.POINTER(C.c_uint16)), vq.ctypes.data_as(C.POINTER(C.c_int8)),
                                            vd.ctypes.data_as(C.POINTER(C.c_uint16))), "rca_lm_kv_read_q8")
        return kq, kd, vq, vd

    def _init_activation_format(self, activation_format: Optional[str]) -> None:
        if activation_format is None:
            return
        try:
            self.set_activation_format(activation_format)
        except Exception:
            self.close()          # a refused mode must not leave the handle (and its weights) behind
            raise

    def _query_activation_format(self) -> str:
        fmt = C.c_int32()
        N.check(self._lib.rca_lm_get_act_format(self._h, C.byref(fmt)), "rca_lm_get_act_format")
        return ACTIVATION_FORMATS[fmt.value]

    def set_activation_format(self, activation_format: str) -> None:
        """"f32" or "q8_1" (see the constructor).  Captured graphs are dropped on a change; the library refuses "q8_1" on a handle
        whose matrices are all bf16 / f16 (RcaError).  The MFMA prefill tiles keep f32 activations in either mode."""
        if activation_format not in ACTIVATION_FORMATS:
            raise ValueError(f"activation_format {activation_format!r}: 'f32' or 'q8_1'")
        N.check(self._lib.rca_lm_set_act_format(self._h, ACTIVATION_FORMATS.index(activation_format)), "rca_lm_set_act_format")
        self.activation_format = activation_format

    def gemv_tap(self, layer: int, kind: int, x: np.ndarray, want_kv: bool = False):
        """Tests only (rca_lm_gemv_tap): one decode GEMV stage on the rows x [M, K]; kind 0 QKV, 1 O, 2 gate/up, 3 down, 4 head.
        Returns y [M, N] float32, and with want_kv (kind 0) also the new K and V cache rows [M, n_kv_heads * 64] as float16."""
        c = self.config
        x = np.ascontiguousarray(x, dtype=np.float32)
        M = x.shape[0]
        widths = {0: (c.hidden, c.n_heads * 64), 1: (c.n_heads * 64, c.hidden), 2: (c.hidden, c.ffn), 3: (c.ffn, c.hidden), 4: (c.hidden, c.vocab_size)}
        if kind not in widths or x.ndim != 2 or x.shape[1] != widths[kind][0]:
            raise ValueError(f"gemv_tap: kind {kind} takes rows of {widths.get(kind, ('?',))[0]} values, got {x.shape}")
        y = np.empty((M, widths[kind][1]), np.float32)
        kv = np.empty((2, M, c.n_kv_heads * 64), np.float16) if (want_kv and kind == 0) else None
        N.check(self._lib.rca_lm_gemv_tap(self._h, int(layer), int(kind), x.ctypes.data_as(C.POINTER(C.c_float)), M,
                                          y.ctypes.data_as(C.POINTER(C.c_float)), C.c_int64(y.size),
                                          kv.ctypes.data_as(C.POINTER(C.c_uint16)) if kv is not None else None), "rca_lm_gemv_tap")
        return (y, kv[0], kv[1]) if kv is not None else y

    def gemv_tap_form(self) -> dict:
        """Tests only (rca_lm_gemv_tap_form): the instance and grid of the handle's last decode GEMV launch."""
        form = (C.c_int32 * 8)()
        N.check(self._lib.rca_lm_gemv_tap_form(self._h, form), "rca_lm_gemv_tap_form")
        return dict(zip(("M", "NIT", "R", "batches", "grid", "format", "ACT", "N"), (int(v) for v in form)))

    def _query_format(self):
        fmt, nbytes = C.c_int32(), C.c_int64()
        N.check(self._lib.rca_lm_weight_format(self._h, C.byref(fmt), C.byref(nbytes)), "rca_lm_weight_format")
        if not 0 <= fmt.value < len(WEIGHT_FORMAT_NAMES):
            raise N.RcaError(f"rca_lm_weight_format reported an unknown format id {fmt.value}")
        return WEIGHT_FORMAT_NAMES[fmt.value], int(nbytes.value)

    def _finish_init(self, seed: int) -> None:
        self._ctx = _Ctx(self)
        self._input_ids = np.zeros(self._n_ctx, dtype=np.intc)
        self.input_ids = self._input_ids
        self._logits_host = np.zeros(self._n_vocab, dtype=np.float32)
        self._logits_valid = False
        self._sampler = None
        self._seed = seed
        self._sampler_params = None
        self._sampler_ext = False      # set_sampler_extensions: typical_p and mirostat v2 are refused, as they always were, until asked for
        self._mfma_prefill = True
        self.last_n_tokens_size = 64      # llama_cpp.Llama's default penalty window (the reference never overrides it)

    # ------------------------------------------------------------------ lifetime
    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            self._lib.rca_lm_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ------------------------------------------------------------------ llama_cpp.Llama surface
    def n_ctx(self) -> int:
        return self._n_ctx

    def n_vocab(self) -> int:
        return self._n_vocab

    @property
    def n_tokens(self) -> int:
        n = C.c_int32()
        N.check(self._lib.rca_lm_get_n_tokens(self._h, C.byref(n)), "rca_lm_get_n_tokens")
        return n.value

    @n_tokens.setter
    def n_tokens(self, value: int) -> None:
        # the agent rolls the KV cache back by assigning n_tokens (realtime_agent_v2.py:208,219,261,465,730)
        N.check(self._lib.rca_lm_set_n_tokens(self._h, int(value)), "rca_lm_set_n_tokens")

    def reset(self) -> None:
        N.check(self._lib.rca_lm_reset(self._h), "rca_lm_reset")
        self._logits_valid = False

    def set_seed(self, seed: int) -> None:
        self._seed = seed & 0xFFFFFFFF

    def eval(self, tokens: Sequence[int]) -> None:
        tokens = list(tokens)
        if not tokens:
            return
        n0 = self.n_tokens
        arr = (C.c_int32 * len(tokens))(*tokens)
        N.check(self._lib.rca_lm_eval(self._h, arr, len(tokens)), "rca_lm_eval")
        self._input_ids[n0:n0 + len(tokens)] = tokens
        self._logits_valid = False

    def _fetch_logits(self) -> np.ndarray:
        if not self._logits_valid:
            N.check(self._lib.rca_lm_get_logits(self._h, C.c_void_p(self._logits_host.ctypes.data)), "rca_lm_get_logits")
            self._logits_valid = True
        return self._logits_host

    def _put_logits(self, row: np.ndarray) -> None:
        """Tests only (rca_lm_put_logits): `row` [n_vocab] replaces the last logits row; sample(), token_probs() and _fetch_logits()
        then behave as after an eval that had produced it."""
        row = np.ascontiguousarray(row, dtype=np.float32)
        if row.shape != (self._n_vocab,):
            raise ValueError(f"_put_logits: the row has {self._n_vocab} logits, got {row.shape}")
        N.check(self._lib.rca_lm_put_logits(self._h, row.ctypes.data_as(C.POINTER(C.c_float))), "rca_lm_put_logits")
        self._logits_valid = False

    @property
    def _scores(self) -> np.ndarray:
        """Rows of logits of the last eval call (all of them for logits_all handles, else the last)."""
        rows = []
        r = 0
        while True:
            buf = np.empty(self._n_vocab, np.float32)
            rc = self._lib.rca_lm_get_logits_row(self._h, r, C.c_void_p(buf.ctypes.data))
            if rc != 0:
                break
            rows.append(buf)
            r += 1
        return np.stack(rows) if rows else np.zeros((0, self._n_vocab), np.float32)

    @property
    def scores(self) -> np.ndarray:
        return self._scores

    @staticmethod
    def logits_to_logprobs(logits: np.ndarray, axis: int = -1) -> np.ndarray:
        logits = np.asarray(logits, dtype=np.float32)
        mx = np.max(logits, axis=axis, keepdims=True)
        shifted = logits - mx
        return shifted - np.log(np.sum(np.exp(shifted), axis=axis, keepdims=True))

    def score(self, tokens: Sequence[int], targets: Optional[Sequence[int]] = None,
              base: Optional["LlamaForAlternatingCodeChannels"] = None) -> "ScoreResult":
        """Append `tokens` at n_tokens like a long eval and reduce every position's logits ON THE DEVICE (rca_lm_score): what
        llama-perplexity and its --kl-divergence mode compute.  targets[i] is the token scored at position i (-1 = not scored: its
        logprob is NaN); None = the next token of `tokens`, the last position unscored.  base: a second handle (any weight format, or
        a twin of this one) at the same n_tokens, advanced over the same tokens; the result then carries KL(P_base || P), the base's
        logprob and its top-1 token per position.  The last position's logits are left as after eval()."""
        tokens = list(tokens)
        n = len(tokens)
        rows = np.zeros(n, N.SCORE_ROW_DTYPE)
        if n == 0:
            return ScoreResult(rows, base is not None)
        if targets is not None and len(targets) != n:
            raise ValueError(f"score: {len(targets)} targets for {n} tokens")
        n0 = self.n_tokens
        arr = (C.c_int32 * n)(*tokens)
        tg = (C.c_int32 * n)(*[int(t) for t in targets]) if targets is not None else None
        N.check(self._lib.rca_lm_score(self._h, base._h if base is not None else None, arr, n, tg,
                                       rows.ctypes.data_as(C.POINTER(N.ScoreRowC))), "rca_lm_score")
        for llm in (self, base):
            if llm is not None:
                llm._input_ids[n0:n0 + n] = tokens
                llm._logits_valid = False
        return ScoreResult(rows, base is not None)

    def imatrix_rows_tap(self, xh: np.ndarray, xl: np.ndarray, m_live: int, acc: np.ndarray) -> np.ndarray:
        """Tests only (rca_lm_imatrix_rows_tap): the importance matrix's column-sum kernel alone on planes xh / xl [M, K] (uint16 bf16 bits) whose first m_live rows are
        live; returns acc (float64 [K]) with their sums added."""
        xh, xl = np.ascontiguousarray(xh, np.uint16), np.ascontiguousarray(xl, np.uint16)
        if xh.ndim != 2 or xh.shape != xl.shape:
            raise ValueError(f"imatrix_rows_tap: planes {xh.shape} / {xl.shape}")
        out = np.array(acc, np.float64)
        if out.shape != (xh.shape[1],):
            raise ValueError(f"imatrix_rows_tap: {out.shape} accumulators for {xh.shape[1]} columns")
        N.check(self._lib.rca_lm_imatrix_rows_tap(self._h, xh.ctypes.data, xl.ctypes.data, xh.shape[0], xh.shape[1], int(m_live), out.ctypes.data),
                "rca_lm_imatrix_rows_tap")
        return out

    # ------------------------------------------------------------------ importance matrix (rca_lm_imatrix_*; imatrix.collect walks a corpus)
    def imatrix_begin(self) -> None:
        """Start collecting an importance matrix on this handle (its own accumulators, zeroed).  Only imatrix_chunk() adds to them."""
        N.check(self._lib.rca_lm_imatrix_begin(self._h), "rca_lm_imatrix_begin")

    def imatrix_end(self) -> None:
        """Free the accumulators (close() does too)."""
        N.check(self._lib.rca_lm_imatrix_end(self._h), "rca_lm_imatrix_end")

    def imatrix_chunk(self, tokens: Sequence[int]) -> None:
        """Append `tokens` at n_tokens as score() does, on the 128-token tiles, summing every projection's input planes; context, K / V
        rows and the last position's logits are left as score() leaves them."""
        arr = np.ascontiguousarray(tokens, dtype=np.int32).reshape(-1)
        if arr.size == 0:
            return
        n0 = self.n_tokens
        N.check(self._lib.rca_lm_imatrix_chunk(self._h, arr.ctypes.data, int(arr.size)), "rca_lm_imatrix_chunk")
        self._input_ids[n0:n0 + arr.size] = arr
        self._logits_valid = False

    def _imatrix_width(self, kind: int) -> int:
        c = self.config
        return {1: c.n_heads * c.head_dim, 3: c.ffn}.get(int(kind), c.hidden)

    def imatrix_chunk_tap(self, tokens: Sequence[int], layer: int, kind: int):
        """Tests only (rca_lm_imatrix_chunk_tap): imatrix_chunk() for one pass; returns the planes (xh, xl) [n, K] (uint16 bf16 bits) of
        (layer, kind) as they stood right behind their collection launch."""
        arr = np.ascontiguousarray(tokens, dtype=np.int32).reshape(-1)
        K = self._imatrix_width(kind)
        xh, xl = np.zeros((max(arr.size, 1), K), np.uint16), np.zeros((max(arr.size, 1), K), np.uint16)
        n0 = self.n_tokens
        N.check(self._lib.rca_lm_imatrix_chunk_tap(self._h, arr.ctypes.data, int(arr.size), int(layer), int(kind), xh.ctypes.data, xl.ctypes.data),
                "rca_lm_imatrix_chunk_tap")
        self._input_ids[n0:n0 + arr.size] = arr
        self._logits_valid = False
        return xh[:arr.size], xl[:arr.size]

    def imatrix_get(self, layer: int, kind: int, width: Optional[int] = None):
        """(sums float64 [K], token count) of one accumulator: kind 0 the attn_q / attn_k / attn_v input, 1 attn_output's, 2 ffn_gate /
        ffn_up's, 3 ffn_down's, 4 output.weight's (layer ignored)."""
        K = self._imatrix_width(kind) if width is None else int(width)
        out, count = np.zeros(max(K, 1), np.float64), C.c_int64(0)
        N.check(self._lib.rca_lm_imatrix_get(self._h, int(layer), int(kind), out.ctypes.data, K, C.byref(count)), "rca_lm_imatrix_get")
        return out[:K], int(count.value)

    def imatrix_read(self):
        """The collection so far as an imatrix.Imatrix: 7 * n_layers + 1 entries under GGUF names, a shared vector under each of its
        names, the head's under output.weight (the name quantize looks up, tied embeddings or not)."""
        from .imatrix import KIND_NAMES, Imatrix
        out = Imatrix()
        for l in range(self.config.n_layers):
            for kind, names in KIND_NAMES.items():
                sums, count = self.imatrix_get(l, kind)
                if not np.isfinite(sums).all():
                    raise ValueError(f"imatrix_read: layer {l}, kind {kind} ({names[0]}): a sum is not finite")
                for name in names:
                    out[f"blk.{l}.{name}.weight"] = (sums.copy(), count)
        sums, count = self.imatrix_get(0, 4)
        if not np.isfinite(sums).all():
            raise ValueError("imatrix_read: output.weight: a sum is not finite")
        out["output.weight"] = (sums, count)
        return out

    def score_rows_tap(self, logits: np.ndarray, targets: Sequence[int], base_logits: Optional[np.ndarray] = None) -> "ScoreResult":
        """Tests only (rca_lm_score_rows_tap): the row reduction of score() alone on host-supplied logits [M, n_vocab]."""
        logits = np.ascontiguousarray(logits, dtype=np.float32)
        if logits.ndim != 2 or logits.shape[1] != self._n_vocab:
            raise ValueError(f"score_rows_tap: rows have {self._n_vocab} logits, got {logits.shape}")
        M = logits.shape[0]
        fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
        if base_logits is not None:
            base_logits = np.ascontiguousarray(base_logits, dtype=np.float32)
            if base_logits.shape != logits.shape:
                raise ValueError(f"score_rows_tap: base rows {base_logits.shape} against {logits.shape}")
        tg = np.ascontiguousarray(targets, dtype=np.int32)
        if tg.shape != (M,):
            raise ValueError(f"score_rows_tap: {tg.shape} targets for {M} rows")
        rows = np.zeros(M, N.SCORE_ROW_DTYPE)
        N.check(self._lib.rca_lm_score_rows_tap(self._h, fp(logits), fp(base_logits) if base_logits is not None else None,
                                                tg.ctypes.data_as(C.POINTER(C.c_int32)), M, rows.ctypes.data_as(C.POINTER(N.ScoreRowC))),
                "rca_lm_score_rows_tap")
        return ScoreResult(rows, base_logits is not None)

    def get_logprobs(self, ctx_input_ids, input_ids, route: str = "decode"):
        """llamacpp_utils.py:30-37: log p(input_ids[i] | ctx, input_ids[:i]) on a logits_all handle.
        route="prefill" (opt-in: the prefill tiles round differently from the decode passes) evaluates the context with eval() and
        the scored tokens with score(): no logits_all handle needed, no logits on the host."""
        if route not in ("decode", "prefill"):
            raise ValueError(f"get_logprobs: route {route!r} is neither 'decode' nor 'prefill'")
        if route == "prefill":
            ctx_input_ids, input_ids = list(ctx_input_ids), list(input_ids)
            if not ctx_input_ids:
                raise ValueError("get_logprobs: the context holds no token to predict input_ids[0] from")
            if not input_ids:
                return np.zeros(0, np.float32)
            self.reset()
            self.eval(ctx_input_ids[:-1])
            return self.score(ctx_input_ids[-1:] + input_ids[:-1], targets=input_ids).logprob
        if not self._logits_all:
            raise N.RcaError("get_logprobs needs a handle created with logits_all=True")
        self.reset()
        # only the LAST context position is scored: evaluate the context as a plain prefill (no per-position head
        # GEMV, no [n_ctx_tokens, vocab] logits buffer), then the scored tokens with every position kept
        N.check(self._lib.rca_lm_set_logits_all(self._h, 0), "rca_lm_set_logits_all")
        self._logits_all = False
        try:
            self.eval(ctx_input_ids)
            last_ctx = self._scores[-1].copy()
        finally:
            N.check(self._lib.rca_lm_set_logits_all(self._h, 1), "rca_lm_set_logits_all")
            self._logits_all = True
        self.eval(input_ids)
        logits = np.concatenate([last_ctx[None, :], self._scores], axis=0)[-len(input_ids) - 1:-1]
        logprobs = self.logits_to_logprobs(logits)
        return logprobs[range(len(input_ids)), list(input_ids)]

    def init_sampler_for_generate(
        self,
        top_k: int = 40,
        top_p: float = 0.95,
        min_p: float = 0.05,
        typical_p: float = 1.0,
        temp: float = 0.80,
        repeat_penalty: float = 1.0,
        frequency_penalty: float = 0.0,
        presence_penalty: float = 0.0,
        tfs_z: float = 1.0,
        mirostat_mode: int = 0,
        mirostat_tau: float = 5.0,
        mirostat_eta: float = 0.1,
        penalize_nl: bool = True,
        logits_processor=None,
        grammar=None,
        seed: Optional[int] = None,
        logit_bias: Optional[Dict[int, float]] = None,
    ) -> None:
        """llamacpp_utils.py:39-77.  The chain llama-cpp-python builds for these arguments, on the device: logit bias (the logits
        processor) -> penalties over the last 64 accepted tokens (repeat / frequency / presence) -> top_k -> typical -> top_p -> min_p ->
        temp -> dist -- every member the agent's config forwards (realtime_agent_v2.py:172-185, realtime_agent_config.py:11-20), top_k
        anywhere from 1 to the vocabulary or <= 0.  typical_p < 1 needs top_k in 1..256 (the whole vocabulary is not sorted by
        typicality; refused otherwise).  mirostat_mode 2: logit bias -> penalties -> temp -> mirostat v2, with top_k, top_p, min_p and
        typical_p ignored as llama-cpp-python leaves them out of that chain; mu starts at 2 * mirostat_tau (mirostat_mu() reads it).
        temp <= 0 is greedy and ignores both.  Both are restated from their published definitions (tests/samp_ext_ref.py); parity with
        llama.cpp is not pinned.  mirostat_mode 1 (its k is computed per draw and can land on any of the three sampler routes) and
        grammars are refused.  Both options are opt-in per handle: until set_sampler_extensions(True) any typical_p other than 1.0
        and any mirostat_mode other than 0 raise NotImplementedError, as they always did."""
        if grammar is not None:
            raise NotImplementedError("grammar samplers are not implemented (the duplex agent never sets one)")
        if (typical_p != 1.0 or mirostat_mode != 0) and not getattr(self, "_sampler_ext", False):
            raise NotImplementedError("typical_p / mirostat samplers are off on this handle (the duplex agent never sets them): "
                                      "call set_sampler_extensions(True) first; mirostat_mode 1 and grammars are not implemented")
        mirostat_mode = int(mirostat_mode)
        if mirostat_mode == 1:
            raise NotImplementedError("mirostat_mode 1 (mirostat v1) is not implemented: its k is computed on the device per draw and can "
                                      "land on any of the three sampler routes; mirostat_mode 2 is")
        if mirostat_mode not in (0, 2):
            raise ValueError(f"mirostat_mode {mirostat_mode} is none of 0 (off), 2 (v2)")
        typical_p = float(typical_p)
        if not typical_p >= 0.0:
            raise ValueError(f"typical_p {typical_p} must be 0 (unset) or positive")
        typical_on = 0.0 < typical_p < 1.0 and temp > 0.0 and mirostat_mode != 2
        if typical_on and not 1 <= int(top_k) <= 256:
            raise ValueError(f"typical_p {typical_p} needs top_k in 1..256 (top_k is {top_k}): the whole vocabulary is not sorted by typicality")
        if mirostat_mode == 2 and not (0.0 <= float(mirostat_tau) < float("inf") and 0.0 <= float(mirostat_eta) < float("inf")):
            raise ValueError(f"mirostat_tau {mirostat_tau} and mirostat_eta {mirostat_eta} must be finite and not negative")
        self.set_seed(seed if seed is not None else -1)
        bias = dict(logit_bias or {})
        if logits_processor is not None:
            lb = getattr(logits_processor, "logit_bias_map", None)
            if lb is None:
                raise NotImplementedError("logits_processor must come from get_logits_bias_processor")
            bias.update(lb)
        ids = (C.c_int32 * max(1, len(bias)))(*bias.keys())
        vals = (C.c_float * max(1, len(bias)))(*bias.values())
        p = N.SamplerParamsC(top_k=int(top_k), top_p=float(top_p), min_p=float(min_p), temp=float(temp), seed=self._seed,
                             n_bias=len(bias), bias_ids=ids, bias_vals=vals, repeat_penalty=float(repeat_penalty),
                             freq_penalty=float(frequency_penalty), presence_penalty=float(presence_penalty),
                             penalty_last_n=int(getattr(self, "last_n_tokens_size", 64)))
        N.check(self._lib.rca_lm_sampler_init(self._h, C.byref(p)), "rca_lm_sampler_init")
        # (rca_lm_sampler_init has reset both options to off)
        if typical_on:
            N.check(self._lib.rca_lm_sampler_set_typical(self._h, typical_p), "rca_lm_sampler_set_typical")
        if mirostat_mode == 2:
            N.check(self._lib.rca_lm_sampler_set_mirostat(self._h, 2, float(mirostat_tau), float(mirostat_eta)), "rca_lm_sampler_set_mirostat")
        self._sampler = True
        self._sampler_params = dict(top_k=top_k, top_p=top_p, min_p=min_p, temp=temp, seed=self._seed, logit_bias=bias,
                                    repeat_penalty=repeat_penalty, frequency_penalty=frequency_penalty, presence_penalty=presence_penalty,
                                    typical_p=typical_p, mirostat_mode=mirostat_mode, mirostat_tau=mirostat_tau, mirostat_eta=mirostat_eta)

    def set_sampler_extensions(self, enable: bool) -> None:
        """Opt in to (or out of) typical_p and mirostat v2 in init_sampler_for_generate.  Off, the default, the call refuses both
        keywords exactly as it did before they existed; the sampler in force is not touched either way."""
        self._sampler_ext = bool(enable)

    def mirostat_mu(self) -> float:
        """mirostat v2's mu as the next draw will read it (settles the stream); an error when mirostat is off"""
        mu = C.c_float()
        N.check(self._lib.rca_lm_sampler_get_mirostat_mu(self._h, C.byref(mu)), "rca_lm_sampler_get_mirostat_mu")
        return float(mu.value)

    def sample(self, idx: Optional[int] = None) -> int:
        assert self.n_tokens > 0
        assert self._sampler is not None
        tok = C.c_int32()
        N.check(self._lib.rca_lm_sample(self._h, C.byref(tok)), "rca_lm_sample")
        return tok.value

    def step(self, tokens: Sequence[int]) -> int:
        """eval(tokens) + sample() in one C-ABI call (hipGraph replay for 1-2 tokens)."""
        tokens = list(tokens)
        n0 = self.n_tokens
        arr = (C.c_int32 * len(tokens))(*tokens)
        tok = C.c_int32()
        N.check(self._lib.rca_lm_step(self._h, arr, len(tokens), C.byref(tok)), "rca_lm_step")
        self._input_ids[n0:n0 + len(tokens)] = tokens
        self._logits_valid = False
        return tok.value

    def step_probe(self, tokens: Sequence[int], probe_ids: Sequence[int]):
        """step(tokens) and token_probs(probe_ids) of the position it evaluated in ONE C-ABI call (one replay, one synchronisation):
        the agent's speculative <|end_audio|> step (realtime_agent_v2.py:455-466).  Returns (token, probabilities)."""
        tokens, probe_ids = list(tokens), list(probe_ids)
        n0 = self.n_tokens
        arr = (C.c_int32 * len(tokens))(*tokens)
        pid = (C.c_int32 * len(probe_ids))(*probe_ids)
        out = (C.c_float * len(probe_ids))()
        tok = C.c_int32()
        N.check(self._lib.rca_lm_step_probe(self._h, arr, len(tokens), pid, len(probe_ids), C.byref(tok), out), "rca_lm_step_probe")
        self._input_ids[n0:n0 + len(tokens)] = tokens
        self._logits_valid = False
        return tok.value, np.array(out[:], dtype=np.float32)

    def frame(self, first_pair: Sequence[int], user_ids: Sequence[int], audio_id_floor: int) -> List[int]:
        """One chunk of process_audio_input_ids (realtime_agent_v2.py:332-372) as ONE graph replay: len(user_ids) S=2 steps with
        the sampled agent token fed back on the device.  Returns the sampled tokens; the list is shorter than user_ids when a
        step sampled a token <= audio_id_floor (it is the last element): n_tokens and the sampler state are then what the same
        number of single steps would have left, and the caller continues step by step."""
        first_pair, user_ids = [int(t) for t in first_pair], [int(t) for t in user_ids]
        if len(first_pair) != 2:
            raise ValueError("frame() starts from the last [agent, user] pair")
        n, n0 = len(user_ids), self.n_tokens
        fp = (C.c_int32 * 2)(*first_pair)
        us = (C.c_int32 * n)(*user_ids)
        out = (C.c_int32 * n)()
        done = C.c_int32()
        N.check(self._lib.rca_lm_frame(self._h, fp, us, n, int(audio_id_floor), out, C.byref(done)), "rca_lm_frame")
        toks = list(out[:done.value])
        evaluated = first_pair + [t for pair in zip(toks[:-1], user_ids) for t in pair]
        self._input_ids[n0:n0 + len(evaluated)] = evaluated
        self._logits_valid = False
        return toks

    def duplex_prepare(self, T: int, F_ctx: int, n_steps: int, n_samples: int) -> None:
        """duplex_frame's one-time allocations for a call shape, ahead of the first frame (rca_duplex_prepare)."""
        N.check(self._lib.rca_duplex_prepare(self._h, int(T), int(F_ctx), int(n_steps), int(n_samples)), "rca_duplex_prepare")

    def duplex_precapture(self, codec_handle, T: int, F_ctx: int, n_steps: int, n_samples: int, code_token_base: int, with_probe: bool,
                          twin: Optional["LlamaForAlternatingCodeChannels"] = None, n_step_probe: int = 0) -> None:
        """Every graph the session's frames can replay, captured now (rca_duplex_precapture): the one-replay frame of this call
        shape for every context bucket on this handle's KV cache and on `twin`'s (the shadow cache the two trade at a trim), and the
        speculative step with n_step_probe probabilities.  Needs the sampler to be initialised."""
        a = N.DuplexFrameArgsC(pcm_window=None, code_ctx=None, T=int(T), F_ctx=int(F_ctx), n_steps=int(n_steps), n_samples=int(n_samples),
                               code_token_base=int(code_token_base), audio_id_floor=-1, probe_id=0 if with_probe else -1)
        N.check(self._lib.rca_duplex_precapture(self._h, twin._h if twin is not None else None, codec_handle._h, C.byref(a), int(n_step_probe)),
                "rca_duplex_precapture")

    def duplex_frame(self, codec_handle, pcm_window: np.ndarray, code_ctx: np.ndarray, n_steps: int, n_samples: int,
                     code_token_base: int, audio_id_floor: int, probe_id: int, first_pair: Sequence[int]) -> dict:
        """One whole duplex frame (encode tail -> the chunk's LM steps -> decode tail -> P(probe)) as ONE graph replay
        (rca_duplex_frame; RealtimeAgent.process_audio, realtime_agent_v2.py:504-554).  `codec_handle` is the HipCodec whose tail
        calls are captured.  Returns user_codes [n_steps], tokens (as frame(): shorter when a step left audio mode), pcm
        [n_samples] or None when the decode of this replay must not be used, probe_prob or None."""
        first_pair = [int(t) for t in first_pair]
        if len(first_pair) != 2:
            raise ValueError("duplex_frame() starts from the last [agent, user] pair")
        pcm_window = np.ascontiguousarray(pcm_window, dtype=np.float32).reshape(-1)
        code_ctx = np.ascontiguousarray(code_ctx, dtype=np.int64).reshape(-1)
        n0 = self.n_tokens
        a = N.DuplexFrameArgsC(pcm_window=pcm_window.ctypes.data, code_ctx=code_ctx.ctypes.data if code_ctx.size else None,
                               T=pcm_window.size, F_ctx=code_ctx.size, n_steps=int(n_steps), n_samples=int(n_samples),
                               code_token_base=int(code_token_base), audio_id_floor=int(audio_id_floor), probe_id=int(probe_id))
        a.first_pair[0], a.first_pair[1] = first_pair
        out = N.DuplexFrameOutC()
        pcm = np.empty(int(n_samples), dtype=np.float32)
        N.check(self._lib.rca_duplex_frame(self._h, codec_handle._h, C.byref(a), C.byref(out), C.c_void_p(pcm.ctypes.data)), "rca_duplex_frame")
        codes = [int(c) for c in out.user_codes[:n_steps]]
        toks = [int(t) for t in out.tokens[:out.n_done]]
        user_ids = [int(code_token_base) + c for c in codes]
        evaluated = first_pair + [t for pair in zip(toks[:-1], user_ids) for t in pair]
        self._input_ids[n0:n0 + len(evaluated)] = evaluated
        self._logits_valid = False
        return {"user_codes": codes, "tokens": toks, "pcm": pcm if out.flags == 0 else None,
                "probe_prob": float(out.probe_prob) if out.probe_prob >= 0.0 else None}

    def generate(self, tokens: Sequence[int], reset: bool = True, stopping_criteria=None) -> Generator[int, Optional[Sequence[int]], None]:
        """llamacpp_utils.py:97-181.  The agent always calls next(generate(ids, reset=False)) and drops the
        generator, so the first yield is the fused step; continuing the generator keeps sampling."""
        tokens = list(tokens)
        if reset and self.n_tokens > 0:
            longest_prefix = 0
            for a, b in zip(self._input_ids[: self.n_tokens], tokens[:-1]):
                if a == b:
                    longest_prefix += 1
                else:
                    break
            if longest_prefix > 0:
                reset = False
                tokens = tokens[longest_prefix:]
                self.n_tokens = longest_prefix
        if reset:
            self.reset()
        while True:
            token = self.step(tokens)
            if stopping_criteria is not None and stopping_criteria(self._input_ids[: self.n_tokens], self._fetch_logits()):
                return
            tokens_or_none = yield token
            tokens = [token]
            if tokens_or_none is not None:
                tokens.extend(tokens_or_none)

    def token_probs(self, token_ids: Sequence[int]) -> np.ndarray:
        """softmax(last logits)[ids], reduced on the device (measure_event_prob, realtime_agent_v2.py:448-452)."""
        ids = (C.c_int32 * len(token_ids))(*token_ids)
        out = (C.c_float * len(token_ids))()
        N.check(self._lib.rca_lm_token_probs(self._h, ids, len(token_ids), out), "rca_lm_token_probs")
        return np.array(out[:], dtype=np.float32)

    def sync(self) -> None:
        N.check(self._lib.rca_lm_sync(self._h), "rca_lm_sync")

    # ------------------------------------------------------------------ shadow KV cache (sliding-window trim without a prefill spike)
    def make_kv_shadow(self, low_priority: bool = True) -> "LlamaForAlternatingCodeChannels":
        """A twin over the same device weights with its own KV cache, workspace and (low-priority) stream: the place where the
        post-trim cache is built while this handle keeps stepping (kv_shadow.py; reference behaviour it replaces:
        recompute_kv_cache inside the trimming frame, realtime_agent_v2.py:187-190,725-733)."""
        twin = LlamaForAlternatingCodeChannels(model_path=self.model_path, n_ctx=self._n_ctx, share_weights_with=self, device=self._device)
        if low_priority:
            N.check(self._lib.rca_lm_set_low_priority(twin._h, 1), "rca_lm_set_low_priority")
        return twin

    def eval_async(self, tokens: Sequence[int]) -> None:
        """eval() that returns once its last tile / pass is enqueued; the next call on this handle waits for it."""
        tokens = list(tokens)
        if not tokens:
            return
        n0 = self.n_tokens
        arr = (C.c_int32 * len(tokens))(*tokens)
        N.check(self._lib.rca_lm_eval_async(self._h, arr, len(tokens)), "rca_lm_eval_async")
        self._input_ids[n0:n0 + len(tokens)] = tokens
        self._logits_valid = False

    def copy_kv_from(self, other: "LlamaForAlternatingCodeChannels", n_positions: int) -> None:
        """KV entries [0, n_positions) of every layer, device to device, from `other`'s cache into this one's."""
        N.check(self._lib.rca_lm_copy_kv(self._h, other._h, int(n_positions)), "rca_lm_copy_kv")
        self._input_ids[:n_positions] = other._input_ids[:n_positions]

    def swap_kv(self, other: "LlamaForAlternatingCodeChannels") -> None:
        """Exchange the KV caches of the two handles (O(1); n_tokens stays with each handle and is set by the caller)."""
        N.check(self._lib.rca_lm_swap_kv(self._h, other._h), "rca_lm_swap_kv")
        n = max(self._n_ctx, other._n_ctx)
        tmp = self._input_ids[:n].copy()
        self._input_ids[:n] = other._input_ids[:n]
        other._input_ids[:n] = tmp
        self._logits_valid = other._logits_valid = False

    # ------------------------------------------------------------------ context shift (sliding-window trim without re-evaluation)
    def kv_remove(self, p0: int, p1: int) -> None:
        """llama.cpp's context shift (rca_lm_kv_remove): drop cache positions [p0, p1) and slide positions [p1, n_tokens) down by
        p1 - p0, re-rotating their keys; n_tokens shrinks by p1 - p0 and the last logits stay readable.  Logits after a kv_remove
        are those of a shifted cache, not those of a recompute: the surviving keys and values of every layer above the first were
        computed while attending to the removed tokens, and each shift adds one fp16 rounding to the surviving keys.  On a "q8_0"
        cache the call needs set_kv_shift_requant(True) and adds one q8_0 quantisation of the surviving keys as well."""
        p0, p1, n = int(p0), int(p1), self.n_tokens
        N.check(self._lib.rca_lm_kv_remove(self._h, p0, p1), "rca_lm_kv_remove")
        self._input_ids[p0:n - (p1 - p0)] = self._input_ids[p1:n].copy()

    @staticmethod
    def kv_remove_many(llms: Sequence["LlamaForAlternatingCodeChannels"], spans: Sequence[Sequence[int]], staged_only: bool = False) -> None:
        """kv_remove(p0, p1) of several handles over one set of weights in ONE library call (the module function kv_remove_many)."""
        kv_remove_many(llms, spans, staged_only)

    def kv_read(self, layer: int, pos0: int, n_pos: int):
        """Tests only (rca_lm_kv_read): the raw K and V cache rows [n_pos, n_kv_heads, 64] of one layer as float16."""
        k = np.empty((int(n_pos), self.config.n_kv_heads, 64), np.float16)
        v = np.empty_like(k)
        N.check(self._lib.rca_lm_kv_read(self._h, int(layer), int(pos0), int(n_pos), k.ctypes.data_as(C.POINTER(C.c_uint16)),
                                         v.ctypes.data_as(C.POINTER(C.c_uint16))), "rca_lm_kv_read")
        return k, v

    def kv_write(self, layer: int, pos0: int, k: Optional[np.ndarray] = None, v: Optional[np.ndarray] = None) -> None:
        """Tests only (rca_lm_kv_write): replace the raw K and / or V cache rows [n_pos, n_kv_heads, 64] (float16) of one layer from
        position pos0 on.  n_tokens is left as it was."""
        for a in (k, v):
            if a is not None and (a.dtype != np.float16 or a.ndim != 3 or a.shape[1:] != (self.config.n_kv_heads, 64)):
                raise ValueError(f"kv_write: rows are float16 [n_pos, {self.config.n_kv_heads}, 64], got {a.dtype} {a.shape}")
        if k is not None and v is not None and k.shape != v.shape:
            raise ValueError(f"kv_write: K rows {k.shape} and V rows {v.shape} differ")
        rows = [np.ascontiguousarray(a).view(np.uint16) if a is not None else None for a in (k, v)]
        n_pos = next((a.shape[0] for a in (k, v) if a is not None), 0)
        ptr = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint16)) if a is not None else None
        N.check(self._lib.rca_lm_kv_write(self._h, int(layer), int(pos0), int(n_pos), ptr(rows[0]), ptr(rows[1])), "rca_lm_kv_write")

    def attn_tap(self, layer: int, route: int, q: np.ndarray, nsp_launch: int = 0, out_rows: Optional[int] = None) -> np.ndarray:
        """Tests only (rca_lm_attn_tap): the attention of one layer alone for the post-RoPE query rows q [M, n_heads * 64] at positions
        n_tokens .. n_tokens + M - 1, over whatever the cache holds.  route 0: the decode launch, 1: the prefill launch with f32 output,
        2: the prefill launch with bf16 hi / lo output (returned as hi + lo).  nsp_launch 0: the splits the positions need.  Returns
        [out_rows, n_heads * 64] float32; rows >= M hold the NaN the device rows were filled with before the launch."""
        q = np.ascontiguousarray(q, dtype=np.float32)
        if q.ndim != 2 or q.shape[1] != self.config.n_heads * 64:
            raise ValueError(f"attn_tap: q rows have {self.config.n_heads * 64} values, got {q.shape}")
        M = q.shape[0]
        out_rows = M if out_rows is None else int(out_rows)
        out = np.empty((max(out_rows, 0), q.shape[1]), np.float32)
        N.check(self._lib.rca_lm_attn_tap(self._h, int(layer), int(route), int(nsp_launch), q.ctypes.data_as(C.POINTER(C.c_float)), M,
                                          out.ctypes.data_as(C.POINTER(C.c_float)), out_rows), "rca_lm_attn_tap")
        return out

    def gemm128_tap(self, layer: int, kind: int, xh: np.ndarray, xl: np.ndarray, rows: Optional[int] = None, row_base: int = 0,
                    seq_min: int = -1, out_rows: Optional[int] = None, want_kv: bool = False, M: Optional[int] = None):
        """Tests only (rca_lm_gemm128_tap): one projection of a 128-token-tile pass on the bf16 hi / lo planes xh, xl (uint16 [M, K]);
        kind 0 QKV, 1 O, 2 gate/up, 3 down, 4 head (M <= 128 rows that are rows row_base .. of a pass of row_base + M tokens).  rows: the
        pass's launch geometry (ceil(rows / 128) token blocks, default M); seq_min: the workgroup threshold that picks the k-slice form, -1 =
        the process value.  Returns (y, form): y float32 [out_rows, N] whose rows >= M hold the NaN the device rows were filled with
        before the launch, form = (grid_y, nseq, ep_nsplit, ep_grp).  kind 4 returns (y, form, tail): the 128 values behind the last row
        of the device block [128, V], NaN unless a kernel wrote past column V.  With want_kv (kind 0) also the new K and V cache rows
        [M, n_kv_heads * 64] as float16: (y, form, k, v).  M (refusal tests): the row count handed to the library, default xh's."""
        c = self.config
        xh, xl = (np.ascontiguousarray(a, dtype=np.uint16) for a in (xh, xl))
        widths = {0: (c.hidden, c.n_heads * 64), 1: (c.n_heads * 64, c.hidden), 2: (c.hidden, c.ffn), 3: (c.ffn, c.hidden), 4: (c.hidden, c.vocab_size)}
        K, W = widths.get(kind, widths[1])
        if xh.ndim != 2 or xh.shape != xl.shape or (kind in widths and xh.shape[1] != K):
            raise ValueError(f"gemm128_tap: kind {kind} takes two planes of rows of {K} values, got {xh.shape} and {xl.shape}")
        M = xh.shape[0] if M is None else int(M)
        rows = M if rows is None else int(rows)
        out_rows = M if out_rows is None else int(out_rows)
        pad = 128 if kind == 4 else 0
        y = np.full(max(out_rows, 1) * W + pad, np.nan, np.float32)
        kv = np.empty((2, max(M, 1), c.n_kv_heads * 64), np.float16) if (want_kv and kind == 0) else None
        form = (C.c_int32 * 4)()
        N.check(self._lib.rca_lm_gemm128_tap(self._h, int(layer), int(kind), xh.ctypes.data, xl.ctypes.data, M, rows, int(row_base), int(seq_min),
                                             y.ctypes.data, out_rows, kv.ctypes.data if kv is not None else None, form), "rca_lm_gemm128_tap")
        if kind == 4:
            return y[:out_rows * W].reshape(out_rows, W), tuple(form), y[out_rows * W:]
        y = y.reshape(out_rows, W)
        return (y, tuple(form), kv[0], kv[1]) if kv is not None else (y, tuple(form))

    def mask_head_rows(self, row_begin: int, row_end: int) -> None:
        """Zero lm_head rows (random-init models: keep sampling on codec tokens like a trained model in audio mode)."""
        N.check(self._lib.rca_lm_mask_head_rows(self._h, int(row_begin), int(row_end)), "rca_lm_mask_head_rows")

    def persist_codec_embeddings(self, codec_state: Dict[str, np.ndarray], codec_vocab_start: int, codebook_size: Optional[int] = None,
                                 return_f32: bool = False) -> Optional[np.ndarray]:
        """CodecLlamaForCausalLM.persist_codec_embeddings (codec_llama.py:178-206) on the device: table row
        codec_vocab_start + i <- linear_2(gelu(linear_1(codec_embed[i]))), one projector per codebook (codec_llama.py:62-67).
        `codec_state` holds CodecLlamaCodecEmbedding's tensors under their state-dict names ("codec_embed.weight",
        "codebook_projectors.<i>.linear_{1,2}.{weight,bias}").  With return_f32 the rows are also returned before the
        16-bit rounding (the reference's own check compares the table with the projector output, :206)."""
        f32 = lambda a: np.ascontiguousarray(bf16_bits_to_f32(a) if a.dtype == np.uint16 else a, dtype=np.float32)
        embed = f32(codec_state["codec_embed.weight"])
        n_books = 1 + max(int(k.split(".")[1]) for k in codec_state if k.startswith("codebook_projectors."))
        size = codebook_size or embed.shape[0] // n_books
        if size * n_books != embed.shape[0]:
            raise ValueError(f"codec_embed has {embed.shape[0]} rows, expected {n_books} codebooks of {size}")
        out = np.empty((embed.shape[0], self.config.hidden), dtype=np.float32) if return_f32 else None
        fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
        for i in range(n_books):
            p = f"codebook_projectors.{i}."
            w1, b1, w2, b2 = (f32(codec_state[p + s]) for s in ("linear_1.weight", "linear_1.bias", "linear_2.weight", "linear_2.bias"))
            if w1.shape != (self.config.hidden, embed.shape[1]) or w2.shape != (self.config.hidden, self.config.hidden):
                raise ValueError(f"projector {i}: linear_1 {w1.shape} / linear_2 {w2.shape} do not match hidden={self.config.hidden}, dim={embed.shape[1]}")
            rows = np.ascontiguousarray(embed[i * size:(i + 1) * size])
            dst = out[i * size:(i + 1) * size] if return_f32 else None
            N.check(self._lib.rca_lm_persist_codec_embeddings(self._h, fp(rows), size, embed.shape[1], fp(w1), fp(b1), fp(w2), fp(b2),
                                                              codec_vocab_start + i * size, fp(dst) if return_f32 else None),
                    "rca_lm_persist_codec_embeddings")
        self._logits_valid = False
        return out

    def set_mfma_prefill(self, enable: bool) -> None:
        """Long evals on bf16 MFMA tiles (default) or on the exact path (the decode GEMV kernels, two tokens per pass)."""
        N.check(self._lib.rca_lm_set_mfma_prefill(self._h, 1 if enable else 0), "rca_lm_set_mfma_prefill")
        self._mfma_prefill = bool(enable)

    def prefill_route(self) -> str:
        """Tests only: the route an eval of more than 8 tokens takes with the current settings: "gemv" (the exact GEMV chunks),
        "tile32" (32-token bf16 MFMA tiles) or "gemm128" (128-token tiles)."""
        r = C.c_int32()
        N.check(self._lib.rca_lm_prefill_route(self._h, C.byref(r)), "rca_lm_prefill_route")
        return ("gemv", "tile32", "gemm128")[r.value]

    def set_attn_fuse(self, enable: bool) -> None:
        """Merge the attention splits inside the attention launch (default) or in a launch of its own."""
        N.check(self._lib.rca_lm_set_attn_fuse(self._h, 1 if enable else 0), "rca_lm_set_attn_fuse")

    def weight_bytes_per_step(self) -> int:
        """bytes of weights one decode step streams, in the format this handle keeps them"""
        return self._query_format()[1]

    def set_graphs(self, enable: bool) -> None:
        N.check(self._lib.rca_lm_set_graphs(self._h, 1 if enable else 0), "rca_lm_set_graphs")


def kv_remove_many(llms: Sequence["LlamaForAlternatingCodeChannels"], spans: Sequence[Sequence[int]], staged_only: bool = False) -> None:
    """The context shift of 1 to 64 handles over ONE set of weights (a handle and its share_weights_with= twins) in one library call
    (rca_lm_kv_remove_many): llms[k] ends exactly as llms[k].kv_remove(*spans[k]) would leave it, bit for bit, but the handles' slabs
    share their launches and the call ends in one synchronisation.  A refusal (a repeated handle, a handle of other weights, a q8_0
    cache without set_kv_shift_requant(True), handles of different KV formats, a span outside a handle's positions) raises and leaves
    every handle and every mirror as it was.  staged_only (tests and measurements) keeps every handle on the staged route whatever its
    span."""
    llms = list(llms)
    rows = [(int(a), int(b)) for a, b in spans]
    if len(rows) != len(llms):
        raise ValueError(f"{len(rows)} spans for {len(llms)} handles")
    lib = llms[0]._lib if llms else N.lib()
    ns = [m.n_tokens for m in llms]
    hs = (C.c_void_p * max(len(llms), 1))(*[m._h for m in llms])
    p0 = (C.c_int32 * max(len(rows), 1))(*[r[0] for r in rows])
    p1 = (C.c_int32 * max(len(rows), 1))(*[r[1] for r in rows])
    call = lib.rca_lm_kv_remove_many_staged if staged_only else lib.rca_lm_kv_remove_many
    N.check(call(hs, len(llms), p0, p1), "rca_lm_kv_remove_many")
    for m, n, (a, b) in zip(llms, ns, rows):
        m._input_ids[a:n - (b - a)] = m._input_ids[b:n].copy()


class LlamaGroup:
    """2 to 4 sessions over ONE set of weights (a handle and its share_weights_with= twins) stepped together: every weight matrix is
    streamed once per step for all of them (rca_lm_group_step; llama.cpp's parallel sequences).  The reference's self-play loads the
    model once per agent and steps each on its own (inference_client_self_play.py:148-159).  Every member ends a group step in the
    state its own step() would have left, bit for bit, so step() / eval() / sample() on a member and group steps mix freely.
    Close the group before its members."""

    def __init__(self, members: Sequence["LlamaForAlternatingCodeChannels"], lib=None):
        self.members = list(members)
        self._lib = lib if lib is not None else N.lib()
        self._g = C.c_void_p()
        handles = (C.c_void_p * len(self.members))(*[m._h for m in self.members])
        N.check(self._lib.rca_lm_group_create(handles, len(self.members), C.byref(self._g)), "rca_lm_group_create")

    def step(self, tokens_per_member: Sequence[Sequence[int]]) -> List[int]:
        """Member s evaluates tokens_per_member[s] (all of one length n, len(members) * n = 2 or 4) at its own n_tokens and samples with
        its own sampler; returns the sampled token of every member.  A refusal (context overflow of any member, an id outside the
        vocabulary, a member without a sampler) raises and leaves every member as it was."""
        rows = [list(t) for t in tokens_per_member]
        if len(rows) != len(self.members):
            raise ValueError(f"{len(rows)} token lists for {len(self.members)} members")
        n = len(rows[0])
        if any(len(r) != n for r in rows):
            raise ValueError("every member evaluates the same number of tokens in a group step")
        starts = [m.n_tokens for m in self.members]
        flat = [t for r in rows for t in r]
        arr = (C.c_int32 * max(len(flat), 1))(*flat)
        out = (C.c_int32 * len(self.members))()
        N.check(self._lib.rca_lm_group_step(self._g, arr, n, out), "rca_lm_group_step")
        for m, n0, r in zip(self.members, starts, rows):
            m._input_ids[n0:n0 + n] = r
            m._logits_valid = False
        return [int(t) for t in out]

    def close(self) -> None:
        if getattr(self, "_g", None) is not None and self._g:
            self._lib.rca_lm_group_destroy(self._g)
            self._g = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class LlamaBatch:
    """2 to 64 sessions over ONE set of weights (a handle and its share_weights_with= twins) stepped together as one token block of the
    128-token MFMA tiles (rca_lm_batch_step; llama.cpp's -np N above 4): every projection is one tile GEMM over all members' rows,
    attention one launch per layer, the head one tile GEMM, the top-k sampler one chain.  Needs a model whose long evals take the
    128-token tiles; smaller models stay with LlamaGroup.  Unlike a group step a batch step is NOT bit-identical to step(): it is in
    the arithmetic class of a decode on a tile-built cache, and a member's result does not depend on its slot or companions.
    step() / eval() / sample() on a member, group steps and batch steps mix freely.  Close the batch before its members.
    Sessions that sit a tick out stay members and are left out of the call: frame(members=[...]) and duplex_frame(codec, members, ...)
    run over a selection and touch no other member, and so does step_probe(members, ...), a 1- or 2-token step with token probabilities
    (the agents' speculative <|end_audio|> step, or the sessions in a text branch); selections of one size class (up to 8, 16, 32, 64) share their graphs, which hold
    no member's pointers and outlive a member's swap_kv (captures() counts them)."""

    def __init__(self, members: Sequence["LlamaForAlternatingCodeChannels"], lib=None):
        self.members = list(members)
        self._lib = lib if lib is not None else N.lib()
        self._b = C.c_void_p()
        handles = (C.c_void_p * len(self.members))(*[m._h for m in self.members])
        N.check(self._lib.rca_lm_batch_create(handles, len(self.members), C.byref(self._b)), "rca_lm_batch_create")

    def step(self, tokens_per_member: Sequence[Sequence[int]]) -> List[int]:
        """Member s evaluates tokens_per_member[s] (all of one length n = 1 or 2, len(members) * n <= 128) at its own n_tokens and
        samples with its own sampler; returns the sampled token of every member.  A refusal (context overflow of any member, an id
        outside the vocabulary, a member without a sampler) raises and leaves every member as it was."""
        rows = [list(t) for t in tokens_per_member]
        if len(rows) != len(self.members):
            raise ValueError(f"{len(rows)} token lists for {len(self.members)} members")
        n = len(rows[0])
        if any(len(r) != n for r in rows):
            raise ValueError("every member evaluates the same number of tokens in a batch step")
        starts = [m.n_tokens for m in self.members]
        flat = [t for r in rows for t in r]
        arr = (C.c_int32 * max(len(flat), 1))(*flat)
        out = (C.c_int32 * len(self.members))()
        N.check(self._lib.rca_lm_batch_step(self._b, arr, n, out), "rca_lm_batch_step")
        for m, n0, r in zip(self.members, starts, rows):
            m._input_ids[n0:n0 + n] = r
            m._logits_valid = False
        return [int(t) for t in out]

    def frame(self, first_pairs: Sequence[Sequence[int]], user_ids: Sequence[Sequence[int]], audio_id_floor: int,
              probe_ids: Optional[Sequence[int]] = None, members: Optional[Sequence[int]] = None):
        """frame() of every member in ONE call (rca_lm_batch_frame; one graph replay when every member has graphs on): member s runs
        len(user_ids[s]) S=2 steps from first_pairs[s] with its sampled token fed back on the device.  Returns (tokens, probe_probs):
        tokens[s] is the list of member s's sampled tokens, shorter than user_ids[s] when a step sampled a token <= audio_id_floor
        (the cutting token is its last element; the member's n_tokens and draw counter are then what that many batch steps leave and
        it has no logits until its next eval or step).  probe_probs is None without probe_ids, else a float32 array with
        softmax(member s's last logits)[probe_ids[s]], NaN where the member was cut or its probe id is -1.  A refusal raises and
        leaves every member as it was.
        members: a list of distinct member indices (any order) that take part (rca_lm_batch_frame_sel); every argument and result
        is then indexed by the position in that list.  A selected member ends as frame() of a batch over only the selected members
        would leave it, bit for bit; the others are not touched.  None: every member, the call as it always was."""
        pairs = [[int(t) for t in p] for p in first_pairs]
        users = [[int(t) for t in u] for u in user_ids]
        sel = None if members is None else [int(s) for s in members]
        if sel is not None and any(s < 0 or s >= len(self.members) for s in sel):
            raise N.RcaError(f"members {sel}: an index outside the batch's {len(self.members)} members")
        taking = self.members if sel is None else [self.members[s] for s in sel]
        nm = len(taking)
        if nm == 0:
            raise N.RcaError("an empty selection (1 to len(members) members take part)")
        if len(pairs) != nm or len(users) != nm:
            raise ValueError(f"{len(pairs)} first pairs and {len(users)} user id lists for {nm} members")
        if any(len(p) != 2 for p in pairs):
            raise ValueError("frame() starts from the last [agent, user] pair of every member")
        n = len(users[0])
        if any(len(u) != n for u in users):
            raise ValueError("every member runs the same number of steps in a batch frame")
        probes = None
        if probe_ids is not None:
            probes = [int(p) for p in probe_ids]
            if len(probes) != nm:
                raise ValueError(f"{len(probes)} probe ids for {nm} members")
        starts = [m.n_tokens for m in taking]
        fp = (C.c_int32 * (2 * nm))(*[t for p in pairs for t in p])
        us = (C.c_int32 * max(nm * n, 1))(*[t for u in users for t in u])
        out = (C.c_int32 * max(nm * n, 1))()
        done = (C.c_int32 * nm)()
        pid = (C.c_int32 * nm)(*probes) if probes is not None else None
        pp = (C.c_float * nm)() if probes is not None else None
        if sel is None:
            N.check(self._lib.rca_lm_batch_frame(self._b, fp, us, n, int(audio_id_floor), pid, out, done, pp), "rca_lm_batch_frame")
        else:
            sl = (C.c_int32 * nm)(*sel)
            N.check(self._lib.rca_lm_batch_frame_sel(self._b, sl, nm, fp, us, n, int(audio_id_floor), pid, out, done, pp), "rca_lm_batch_frame_sel")
        tokens = []
        for s, (m, n0) in enumerate(zip(taking, starts)):
            toks = [int(t) for t in out[s * n:s * n + done[s]]]
            evaluated = pairs[s] + [t for pair in zip(toks[:-1], users[s]) for t in pair]
            m._input_ids[n0:n0 + len(evaluated)] = evaluated
            m._logits_valid = False
            tokens.append(toks)
        if probes is None:
            return tokens, None
        probs = np.array(pp[:], dtype=np.float32)
        probs[probs < 0.0] = np.nan
        return tokens, probs

    def step_probe(self, members: Sequence[int], tokens_per_member: Sequence[Sequence[int]],
                   probe_ids_per_member: Optional[Sequence[Sequence[int]]] = None):
        """step_probe() of the members in `members` (distinct indices, any order) in ONE pass (rca_lm_batch_step_sel): member
        members[k] evaluates tokens_per_member[k] (all of one length n = 1 or 2) at its own n_tokens, samples with its own sampler and
        has softmax(its new logits)[probe_ids_per_member[k]] taken (all of one length, up to 8).  Returns (tokens, probs): the sampled
        token of every selected member and a float32 array [len(members), n_probe], None without probe ids.  A selected member ends
        as step() of a batch over only the selected members, then token_probs(), would leave it, bit for bit; the others are not
        touched.  The agents' speculative <|end_audio|> step: roll back with member.n_tokens -= n afterwards.  A refusal raises and
        leaves every member as it was."""
        sel = [int(s) for s in members]
        if not sel or any(s < 0 or s >= len(self.members) for s in sel):
            raise N.RcaError(f"members {sel}: 1 to {len(self.members)} indices inside the batch's members")
        nm = len(sel)
        rows = [[int(t) for t in r] for r in tokens_per_member]
        if len(rows) != nm:
            raise ValueError(f"{len(rows)} token lists for {nm} members")
        n = len(rows[0])
        if any(len(r) != n for r in rows):
            raise ValueError("every member evaluates the same number of tokens in a batch step")
        probes = None if probe_ids_per_member is None else [[int(p) for p in r] for r in probe_ids_per_member]
        n_probe = 0
        if probes is not None:
            if len(probes) != nm:
                raise ValueError(f"{len(probes)} probe id lists for {nm} members")
            n_probe = len(probes[0])
            if any(len(r) != n_probe for r in probes):
                raise ValueError("every member probes the same number of ids in a batch step")
        taking = [self.members[s] for s in sel]
        starts = [m.n_tokens for m in taking]
        sl = (C.c_int32 * nm)(*sel)
        arr = (C.c_int32 * max(nm * n, 1))(*[t for r in rows for t in r])
        pid = (C.c_int32 * (nm * n_probe))(*[p for r in probes for p in r]) if n_probe else None
        out = (C.c_int32 * nm)()
        pp = (C.c_float * (nm * n_probe))() if n_probe else None
        N.check(self._lib.rca_lm_batch_step_sel(self._b, sl, nm, arr, n, pid, n_probe, out, pp), "rca_lm_batch_step_sel")
        for m, n0, r in zip(taking, starts, rows):
            m._input_ids[n0:n0 + n] = r
            m._logits_valid = False
        toks = [int(t) for t in out]
        if not n_probe:
            return toks, None
        return toks, np.array(pp[:], dtype=np.float32).reshape(nm, n_probe)

    def duplex_frame(self, codec_handle, members: Sequence[int], pcm_windows, code_ctxs, n_steps: int, n_samples: int, code_token_base: int,
                     audio_id_floor: int, probe_ids: Optional[Sequence[int]], first_pairs: Sequence[Sequence[int]]) -> List[dict]:
        """duplex_frame() of every member of `members` in ONE call (rca_duplex_batch_frame): encode tails -> ids -> the selection frame
        -> codes -> decode tails -> P(probe), one replay from the second call of a shape on.  pcm_windows [len(members)][T] and
        code_ctxs [len(members)][F_ctx] are the members' rolling windows in one call shape; probe_ids one id per member (-1: none) or
        None.  Returns, per member, the dict LlamaForAlternatingCodeChannels.duplex_frame returns: user_codes, tokens (shorter when a
        step left audio mode), pcm or None when the decode of this call must not be used, probe_prob or None, plus "flags" (the C
        call's bits: 1 a sampled token is no codec token, 2 cut).  Only the selected
        members' _input_ids are touched.  A refusal raises and leaves every member as it was."""
        sel = [int(s) for s in members]
        if not sel or any(s < 0 or s >= len(self.members) for s in sel):
            raise N.RcaError(f"members {sel}: 1 to {len(self.members)} indices inside the batch's members")
        nm, n = len(sel), int(n_steps)
        taking = [self.members[s] for s in sel]
        pairs = [[int(t) for t in p] for p in first_pairs]
        if len(pairs) != nm or any(len(p) != 2 for p in pairs):
            raise ValueError("duplex_frame() starts from the last [agent, user] pair of every selected member")
        pcm_in = np.ascontiguousarray(pcm_windows, dtype=np.float32).reshape(nm, -1)
        ctx = np.ascontiguousarray(code_ctxs, dtype=np.int64)
        ctx = ctx.reshape(nm, ctx.size // nm)          # (an empty context, F_ctx = 0, is a call shape too)
        probes = None if probe_ids is None else [int(p) for p in probe_ids]
        if probes is not None and len(probes) != nm:
            raise ValueError(f"{len(probes)} probe ids for {nm} members")
        starts = [m.n_tokens for m in taking]
        sl = (C.c_int32 * nm)(*sel)
        fp = (C.c_int32 * (2 * nm))(*[t for p in pairs for t in p])
        pid = (C.c_int32 * nm)(*probes) if probes is not None else None
        a = N.DuplexBatchArgsC(sel=C.addressof(sl), n_sel=nm, pcm_windows=pcm_in.ctypes.data, code_ctx=ctx.ctypes.data if ctx.size else None,
                               first_pairs=C.addressof(fp), probe_ids=C.addressof(pid) if pid is not None else None, T=pcm_in.shape[1],
                               F_ctx=ctx.shape[1], n_steps=n, n_samples=int(n_samples), code_token_base=int(code_token_base),
                               audio_id_floor=int(audio_id_floor))
        codes = np.zeros((nm, 8), np.int64)
        toks = np.zeros((nm, 8), np.int32)
        done, flags, prob = np.zeros(nm, np.int32), np.zeros(nm, np.int32), np.zeros(nm, np.float32)
        out = N.DuplexBatchOutC(user_codes=codes.ctypes.data, tokens=toks.ctypes.data, n_done=done.ctypes.data, flags=flags.ctypes.data,
                                probe_prob=prob.ctypes.data)
        pcm = np.empty((nm, int(n_samples)), dtype=np.float32)
        N.check(self._lib.rca_duplex_batch_frame(self._b, codec_handle._h, C.byref(a), C.byref(out), C.c_void_p(pcm.ctypes.data)), "rca_duplex_batch_frame")
        res = []
        for k, (m, n0) in enumerate(zip(taking, starts)):
            uc = [int(c) for c in codes[k, :n]]
            tk = [int(t) for t in toks[k, :done[k]]]
            user_ids = [int(code_token_base) + c for c in uc]
            evaluated = pairs[k] + [t for pair in zip(tk[:-1], user_ids) for t in pair]
            m._input_ids[n0:n0 + len(evaluated)] = evaluated
            m._logits_valid = False
            res.append({"user_codes": uc, "tokens": tk, "pcm": pcm[k] if flags[k] == 0 else None,
                        "probe_prob": float(prob[k]) if prob[k] >= 0.0 else None, "flags": int(flags[k])})
        return res

    def kv_remove(self, members: Sequence[int], spans: Sequence[Sequence[int]]) -> None:
        """kv_remove_many over the members with these indices: member members[k] drops its cache positions spans[k] = (p0, p1)."""
        idx = [int(s) for s in members]
        for s in idx:
            if not 0 <= s < len(self.members):
                raise ValueError(f"member {s} outside the batch of {len(self.members)}")
        kv_remove_many([self.members[s] for s in idx], spans)

    def attn_tap(self, layer: int, q: np.ndarray, n: int, nsp_launch: int = 0, sel: Optional[Sequence[int]] = None,
                 out_rows: Optional[int] = None) -> np.ndarray:
        """Tests only (rca_lm_batch_attn_tap): the batch pass's decode attention of one layer alone, for n = 1 or 2 post-RoPE query
        tokens per member, q [members of the pass * n, n_heads * 64] with member k's token j in row k * n + j, at each member's own
        n_tokens over whatever its cache holds.  sel None: the batch's own table; else the selection table of frame(members=sel).
        nsp_launch 0: the splits the members need.  Returns [out_rows, n_heads * 64] float32 (the bf16 hi + lo the O projection
        reads); rows the launch did not write hold NaN.  Every member's n_tokens is left as it was."""
        q = np.ascontiguousarray(q, dtype=np.float32)
        width = self.members[0].config.n_heads * 64
        nm = len(self.members) if sel is None else len(sel)
        if q.ndim != 2 or q.shape != (nm * int(n), width):
            raise ValueError(f"attn_tap: q is [{nm} members x {n} tokens, {width}], got {q.shape}")
        out_rows = q.shape[0] if out_rows is None else int(out_rows)
        out = np.empty((max(out_rows, 0), width), np.float32)
        sl = None if sel is None else (C.c_int32 * max(nm, 1))(*[int(s) for s in sel])
        N.check(self._lib.rca_lm_batch_attn_tap(self._b, int(layer), int(n), int(nsp_launch), sl, nm if sel is not None else 0, q.ctypes.data,
                                                out.ctypes.data, out_rows), "rca_lm_batch_attn_tap")
        return out

    def captures(self) -> int:
        """graph captures this batch has made so far (rca_lm_batch_captures): selections of one geometry class (up to 8, 16, 32, 64
        members) share one capture per (steps, context bucket, probes), also after a member's swap_kv"""
        n = C.c_int64()
        N.check(self._lib.rca_lm_batch_captures(self._b, C.byref(n)), "rca_lm_batch_captures")
        return int(n.value)

    def close(self) -> None:
        if getattr(self, "_b", None) is not None and self._b:
            self._lib.rca_lm_batch_destroy(self._b)
            self._b = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class LlamaBatchEval:
    """eval_async() of several sessions over ONE set of weights in shared passes of the 128-token prefill tiles (rca_lm_batch_eval;
    llama.cpp: one llama_decode over a llama_batch with prompt tokens of several sequences): every matrix is streamed once per pass of
    up to 1024 rows instead of once per handle.  The shadow-cache tiles of many sessions, or the prompts of sessions admitted together.
    Every handle ends exactly as its own eval_async(tokens) would leave it -- n_tokens, KV bits, and with want_logits the logits --
    so the call mixes freely with everything else on the handles; a later call on a handle waits for the pass first.
    Owns the workspace, one more weight-sharing twin with a small context whose buffers and (low-priority) stream the passes use.
    Close it before the handles."""

    WORKSPACE_N_CTX = 256

    @staticmethod
    def supported(llm) -> bool:
        """the model takes the 128-token tiles (smaller models keep eval_async) and the library has the call"""
        return hasattr(llm, "_h") and hasattr(llm, "prefill_route") and hasattr(N.lib(), "rca_lm_batch_eval") and llm.prefill_route() == "gemm128"

    def __init__(self, llm: "LlamaForAlternatingCodeChannels", low_priority: bool = True):
        self._lib = llm._lib
        self.ws = LlamaForAlternatingCodeChannels(model_path=llm.model_path, n_ctx=min(self.WORKSPACE_N_CTX, llm._n_ctx), share_weights_with=llm,
                                                  device=llm._device)
        if low_priority:
            N.check(self._lib.rca_lm_set_low_priority(self.ws._h, 1), "rca_lm_set_low_priority")

    def eval_async(self, handles: Sequence["LlamaForAlternatingCodeChannels"], token_lists: Sequence[Sequence[int]], want_logits: bool = False) -> None:
        """handles[k] appends token_lists[k] (at least one token) at its own n_tokens; returns once the last pass is enqueued.  A refusal
        raises and leaves every handle as it was.  want_logits=False runs no head: the handles have no logits afterwards."""
        handles = list(handles)
        rows = [list(t) for t in token_lists]
        if len(rows) != len(handles):
            raise ValueError(f"{len(rows)} token lists for {len(handles)} handles")
        starts = [h.n_tokens for h in handles]
        flat = [t for r in rows for t in r]
        hs = (C.c_void_p * max(len(handles), 1))(*[h._h for h in handles])
        ids = (C.c_int32 * max(len(flat), 1))(*flat)
        counts = (C.c_int32 * max(len(rows), 1))(*[len(r) for r in rows])
        N.check(self._lib.rca_lm_batch_eval(self.ws._h, hs, len(handles), ids, counts, 1 if want_logits else 0), "rca_lm_batch_eval")
        for h, n0, r in zip(handles, starts, rows):
            h._input_ids[n0:n0 + len(r)] = r
            h._logits_valid = False

    def eval(self, handles, token_lists, want_logits: bool = False) -> None:
        self.eval_async(handles, token_lists, want_logits)
        self.sync()

    def sync(self) -> None:
        self.ws.sync()

    def close(self) -> None:
        if getattr(self, "ws", None) is not None:
            self.ws.close()
            self.ws = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class ScoreResult:
    """What score() returns: one numpy array per field of rca_score_row_t, one entry per position.  logprob / lse / max_logit /
    argmax of the scored handle; with a base also kl = KL(P_base || P), base_logprob and base_argmax (None without one).
    flags: bit 0 a NaN in the row, bit 1 a NaN in the base's row, bit 2 kl = +inf."""

    def __init__(self, rows: np.ndarray, has_base: bool):
        self.rows = rows
        self.logprob, self.lse, self.max_logit = rows["logprob"].copy(), rows["lse"].copy(), rows["max_logit"].copy()
        self.argmax, self.flags = rows["argmax"].copy(), rows["flags"].copy()
        self.kl = rows["kl"].copy() if has_base else None
        self.base_logprob = rows["base_logprob"].copy() if has_base else None
        self.base_argmax = rows["base_argmax"].copy() if has_base else None

    def __len__(self) -> int:
        return len(self.rows)


class _LogitBiasProcessorList(list):
    """Return type of get_logits_bias_processor: a one-element processor list that also exposes the
    bias map so the device sampler can apply it (the llama.cpp path copies the whole logits array on the
    host per step, llamacpp_utils.py:13-22)."""
    logit_bias_map: Dict[int, float] = {}


def get_logits_bias_processor(logit_bias: Dict[int, float]):
    """llamacpp_utils.py:8-24."""
    logit_bias_map = {int(k): float(v) for k, v in logit_bias.items()}

    def logit_bias_processor(input_ids, scores):
        new_scores = np.copy(scores)
        for input_id, score in logit_bias_map.items():
            new_scores[input_id] = score + scores[input_id]
        return new_scores

    out = _LogitBiasProcessorList([logit_bias_processor])
    out.logit_bias_map = logit_bias_map
    return out
