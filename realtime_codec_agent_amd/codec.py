"""HIP-backed codec model object.

`HipCodec` is the thin handle over the C ABI (include/rca.h, rca_codec_*).
`MagiCodecHIP` wraps it with exactly the attribute surface the reference
AudioTokenizer expects of its `codec_model` (audio_tokenizer.py:26-36,158,189-200;
SURVEY.md 8b-1): codebook_size, sample_rate, pad_audio, encoder,
quantizer.inference, quantizer.codebook.weight, quantizer.codebook_proj, decoder,
eval(), to().  torch is plumbing only: it owns the I/O tensors in HBM and the
stream; every kernel is ours.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, Optional, Tuple

import numpy as np

from . import _native as N
from .codec_model import CodecConfig, init_codec_weights


class HipCodec:
    def __init__(self, cfg: CodecConfig, weights: Dict[str, np.ndarray], device: int = 0):
        self.cfg = cfg
        self.device = device
        self._lib = N.lib()
        self._h = C.c_void_p()
        tensors, keep = N.make_tensors(weights)
        ccfg = N.codec_config_c(cfg)
        N.check(self._lib.rca_codec_create(C.byref(ccfg), tensors, len(weights), device, C.byref(self._h)), "rca_codec_create")
        del keep
        self.hop = cfg.hop
        self.mfma_mode = 0

    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            self._lib.rca_codec_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def num_frames(self, T: int) -> int:
        return (T + self.hop - 1) // self.hop

    def set_variant(self, v: int) -> None:
        N.check(self._lib.rca_codec_set_variant(self._h, v), "rca_codec_set_variant")

    def sync(self) -> None:
        N.check(self._lib.rca_codec_sync(self._h), "rca_codec_sync")

    # ---- host-pointer API (numpy in / numpy out)
    def encode(self, pcm: np.ndarray) -> np.ndarray:
        pcm = np.ascontiguousarray(pcm, dtype=np.float32)
        if pcm.ndim != 2:
            raise ValueError("pcm must be [B,T]")
        B, T = pcm.shape
        codes = np.empty((B, self.num_frames(T)), np.int64)
        N.check(self._lib.rca_codec_encode(self._h, C.c_void_p(pcm.ctypes.data), B, T, C.c_void_p(codes.ctypes.data)), "rca_codec_encode")
        return codes

    def decode(self, codes: np.ndarray) -> np.ndarray:
        codes = np.ascontiguousarray(codes, dtype=np.int64)
        if codes.ndim != 2:
            raise ValueError("codes must be [B,F]")
        B, F = codes.shape
        pcm = np.empty((B, F * self.hop), np.float32)
        N.check(self._lib.rca_codec_decode(self._h, C.c_void_p(codes.ctypes.data), B, F, C.c_void_p(pcm.ctypes.data)), "rca_codec_decode")
        return pcm

    def encode_tail(self, pcm: np.ndarray, n_keep: int) -> np.ndarray:
        """Last n_keep codes of encode(pcm), host buffers, graph-replayed per shape (rca_codec_encode_tail)."""
        pcm = np.ascontiguousarray(pcm, dtype=np.float32)
        if pcm.ndim != 2:
            raise ValueError("pcm must be [B,T]")
        B, T = pcm.shape
        n_keep = min(int(n_keep), self.num_frames(T))
        codes = np.empty((B, n_keep), np.int64)
        N.check(self._lib.rca_codec_encode_tail(self._h, C.c_void_p(pcm.ctypes.data), B, T, n_keep, C.c_void_p(codes.ctypes.data)),
                "rca_codec_encode_tail")
        return codes

    def decode_tail(self, codes: np.ndarray, n_samples: int) -> np.ndarray:
        """Last n_samples of decode(codes), host buffers, graph-replayed per shape (rca_codec_decode_tail)."""
        codes = np.ascontiguousarray(codes, dtype=np.int64)
        if codes.ndim != 2:
            raise ValueError("codes must be [B,F]")
        B, F = codes.shape
        n = min(int(n_samples), F * self.hop)
        pcm = np.empty((B, n), np.float32)
        N.check(self._lib.rca_codec_decode_tail(self._h, C.c_void_p(codes.ctypes.data), B, F, n, C.c_void_p(pcm.ctypes.data)),
                "rca_codec_decode_tail")
        return pcm

    def set_mfma_mode(self, mode: int) -> None:
        """Encoder conv arithmetic: 0 = f32 matrix instruction (bit-exact, default), 3 = bf16 hi + lo split, 1 = bf16 (opt-in, not bit-exact)."""
        N.check(self._lib.rca_codec_set_mfma_mode(self._h, int(mode)), "rca_codec_set_mfma_mode")
        self.mfma_mode = int(mode)

    def set_stream_graphs(self, enable: bool) -> None:
        N.check(self._lib.rca_codec_set_stream_graphs(self._h, int(bool(enable))), "rca_codec_set_stream_graphs")

    def codebook(self) -> np.ndarray:
        out = np.empty((self.cfg.codebook_size, self.cfg.codebook_dim), np.float32)
        N.check(self._lib.rca_codec_codebook(self._h, C.c_void_p(out.ctypes.data)), "rca_codec_codebook")
        return out

    def encode_tap(self, pcm: np.ndarray, layer: int) -> np.ndarray:
        pcm = np.ascontiguousarray(pcm, dtype=np.float32)
        B, T = pcm.shape
        F = self.num_frames(T)
        n = self.cfg.n_stages
        L = F * self.hop
        if layer == 0:
            shape = (B, self.cfg.channels[0], L)
        elif layer <= n:
            for i in range(layer):
                L //= self.cfg.strides[i]
            shape = (B, self.cfg.channels[layer], L)
        elif layer == n + 1:
            shape = (B, self.cfg.latent_dim, F)
        else:
            shape = (B * F, self.cfg.codebook_dim)
        out = np.empty(shape, np.float32)
        N.check(self._lib.rca_codec_encode_tap(self._h, C.c_void_p(pcm.ctypes.data), B, T, layer, C.c_void_p(out.ctypes.data),
                                               C.c_int64(out.size)), "rca_codec_encode_tap")
        return out

    def encode_tap_bf16(self, pcm: np.ndarray, layer: int) -> Tuple[np.ndarray, Optional[np.ndarray]]:
        """Tests only (rca_codec_encode_tap_bf16): the bf16 planes encode()'s blocked pipeline stores after encoder layer `layer`
        in mfma mode 1 / 3, as raw bf16 bits [B, C, L] uint16: (hi, lo), lo None in mode 1."""
        pcm = np.ascontiguousarray(pcm, dtype=np.float32)
        B, T = pcm.shape
        L = self.num_frames(T) * self.hop
        for i in range(layer):
            L //= self.cfg.strides[i]
        Cn = self.cfg.channels[layer] if 0 <= layer <= self.cfg.n_stages else 0
        hi = np.empty((B, Cn // 16, L, 16), np.uint16)
        lo = np.empty_like(hi) if self.mfma_mode == 3 else None
        N.check(self._lib.rca_codec_encode_tap_bf16(self._h, C.c_void_p(pcm.ctypes.data), B, T, layer, C.c_void_p(hi.ctypes.data),
                                                    C.c_void_p(lo.ctypes.data if lo is not None else None), C.c_int64(B * Cn * L)),
                "rca_codec_encode_tap_bf16")
        unblock = lambda a: np.ascontiguousarray(a.transpose(0, 1, 3, 2).reshape(B, Cn, L))   # [B][C/16][L][C%16] -> [B][C][L]
        return unblock(hi), (unblock(lo) if lo is not None else None)

    def decoder_layer_tap(self, layer: int, route: int, x: np.ndarray) -> Tuple[np.ndarray, int, bool]:
        """Tests only (rca_codec_decoder_layer_tap): ONE decoder layer (0 = conv_in, 1..n = up.{0..n-1}, n + 1 = conv_out with its
        clamp) as a decode pass (route 0) or a streaming tail call (route 1) launches it, on x [B, Cin, Lin].  Returns
        (y [B, Cout, Lout], kernel class, guards intact); an element the kernel did not write is NaN."""
        x = np.ascontiguousarray(x, dtype=np.float32)
        layers = self.cfg.decoder_layers()
        if x.ndim != 3 or not 0 <= layer < len(layers) or x.shape[1] != layers[layer]["cin"]:
            raise ValueError("x must be [B, Cin, Lin] of a decoder layer")
        ly = layers[layer]
        B, _, Lin = x.shape
        y = np.empty((B, ly["cout"], Lin * ly["s"] if ly["tr"] else Lin), np.float32)
        kclass, guards = C.c_int32(-1), C.c_int32(-1)
        fp = C.POINTER(C.c_float)
        N.check(self._lib.rca_codec_decoder_layer_tap(self._h, layer, route, x.ctypes.data_as(fp), B, Lin, y.ctypes.data_as(fp),
                                                      C.c_int64(y.size), C.byref(kclass), C.byref(guards)), "rca_codec_decoder_layer_tap")
        return y, kclass.value, bool(guards.value)

    def encoder_layer_tap(self, layer: int, route: int, x: np.ndarray, flags: int = 0, view: int = 0) -> Tuple[np.ndarray, int, bool, bool]:
        """Tests only (rca_codec_encoder_layer_tap): ONE encoder layer (0 = conv_in, 1..n = down.{0..n-1}, n + 1 = conv_out) as an
        encode pass (route 0) or a streaming tail call (route 1) launches it.  x is PCM [B, T] for layer 0 and for flags & 4 (the
        fused first layer), else [B, Cin, Lin].  flags: 1 = x holds LeakyReLU(x), 2 = store LeakyReLU(y), 4 = fused first layer;
        view: trailing columns per row of the last layer (0 = all).  Returns (y [B, Cout, Lout or view], kernel class, the launch
        stored LeakyReLU(y), guards intact); an element the kernel did not write is NaN."""
        x = np.ascontiguousarray(x, dtype=np.float32)
        layers = self.cfg.encoder_layers()
        if not 0 <= layer < len(layers):
            raise ValueError("layer out of range")
        ly = layers[layer]
        if layer == 0 or flags & 4:
            if x.ndim != 2:
                raise ValueError("x must be PCM [B, T] for conv_in and the fused first layer")
            B, Lin = x.shape
            L = -(-Lin // self.hop) * self.hop
        else:
            if x.ndim != 3 or x.shape[1] != ly["cin"]:
                raise ValueError("x must be [B, Cin, Lin] of an encoder layer")
            B, _, Lin = x.shape
            L = Lin
        y = np.empty((B, ly["cout"], view if view else L // ly["s"]), np.float32)
        kclass, post, guards = C.c_int32(-1), C.c_int32(-1), C.c_int32(-1)
        fp = C.POINTER(C.c_float)
        N.check(self._lib.rca_codec_encoder_layer_tap(self._h, layer, route, flags, view, x.ctypes.data_as(fp), B, Lin, y.ctypes.data_as(fp),
                                                      C.c_int64(y.size), C.byref(kclass), C.byref(post), C.byref(guards)),
                "rca_codec_encoder_layer_tap")
        return y, kclass.value, bool(post.value), bool(guards.value)

    # ---- device-pointer API (raw addresses; stream = hipStream_t as int, 0 = handle's own stream)
    def encode_dev(self, pcm_ptr: int, B: int, T: int, codes_ptr: int, stream: int = 0) -> None:
        N.check(self._lib.rca_codec_encode_dev(self._h, C.c_void_p(pcm_ptr), B, T, C.c_void_p(codes_ptr), C.c_void_p(stream)), "rca_codec_encode_dev")

    def decode_dev(self, codes_ptr: int, B: int, F: int, pcm_ptr: int, stream: int = 0) -> None:
        N.check(self._lib.rca_codec_decode_dev(self._h, C.c_void_p(codes_ptr), B, F, C.c_void_p(pcm_ptr), C.c_void_p(stream)), "rca_codec_decode_dev")

    def encode_tail_dev(self, pcm_ptr: int, B: int, T: int, n_keep: int, codes_ptr: int, stream: int = 0) -> None:
        """Last n_keep codes of encode_dev(pcm), computed over their receptive field only (bit-identical)."""
        N.check(self._lib.rca_codec_encode_tail_dev(self._h, C.c_void_p(pcm_ptr), B, T, n_keep, C.c_void_p(codes_ptr), C.c_void_p(stream)),
                "rca_codec_encode_tail_dev")

    def decode_tail_dev(self, codes_ptr: int, B: int, F: int, n_samples: int, pcm_ptr: int, stream: int = 0) -> None:
        """Last n_samples of decode_dev(codes), computed from the codes they depend on only (bit-identical)."""
        N.check(self._lib.rca_codec_decode_tail_dev(self._h, C.c_void_p(codes_ptr), B, F, n_samples, C.c_void_p(pcm_ptr), C.c_void_p(stream)),
                "rca_codec_decode_tail_dev")

    def receptive_field(self) -> Tuple[int, int]:
        """(encoder, decoder) whole frames a kept code / sample can see to its left."""
        a, b = C.c_int32(), C.c_int32()
        N.check(self._lib.rca_codec_receptive_field(self._h, C.byref(a), C.byref(b)), "rca_codec_receptive_field")
        return a.value, b.value

    def set_window_trim(self, enable: bool) -> None:
        """Batch windows encode only what their kept codes can see (same codes, ~10x less work at 2 s context)."""
        N.check(self._lib.rca_codec_set_window_trim(self._h, int(bool(enable))), "rca_codec_set_window_trim")

    def encode_windows_dev(self, audio_ptr: int, Cn: int, Nsamp: int, chunk: int, ctx: int, batch_windows: int, codes_ptr: int,
                           codes_per_channel: int, stream: int = 0) -> None:
        N.check(self._lib.rca_codec_encode_windows_dev(self._h, C.c_void_p(audio_ptr), Cn, C.c_int64(Nsamp), chunk, ctx, batch_windows,
                                                       C.c_void_p(codes_ptr), C.c_int64(codes_per_channel), C.c_void_p(stream)),
                "rca_codec_encode_windows_dev")

    def encode_chunk_range_dev(self, audio_ptr: int, Cn: int, Nsamp: int, chunk: int, ctx: int, batch_windows: int, chunk_begin: int,
                               chunk_end: int, codes_ptr: int, codes_per_channel: int, stream: int = 0) -> None:
        N.check(self._lib.rca_codec_encode_chunk_range_dev(self._h, C.c_void_p(audio_ptr), Cn, C.c_int64(Nsamp), chunk, ctx, batch_windows,
                                                           C.c_int64(chunk_begin), C.c_int64(chunk_end), C.c_void_p(codes_ptr),
                                                           C.c_int64(codes_per_channel), C.c_void_p(stream)),
                "rca_codec_encode_chunk_range_dev")

    def encode_rows_dev(self, audio_ptr: int, src_off_ptr: int, B: int, T: int, n_keep: int, codes_ptr: int, dst_off_ptr: int, span: int,
                        stream: int = 0) -> None:
        """B windows of T samples at audio + src_off[b]; the last n_keep codes of window b land at codes + dst_off[b]."""
        N.check(self._lib.rca_codec_encode_rows_dev(self._h, C.c_void_p(audio_ptr), C.c_void_p(src_off_ptr), B, T, n_keep, C.c_void_p(codes_ptr),
                                                    C.c_void_p(dst_off_ptr), C.c_int64(span), C.c_void_p(stream)), "rca_codec_encode_rows_dev")

    def ingest_supported(self, up: int, down: int, n_taps: int) -> bool:
        """Whether rca_codec_ingest_rows_dev takes this ratio (its phase table and input tile fit the kernel's LDS budget)."""
        return self._lib.rca_codec_ingest_supported(self._h, int(up), int(down), int(n_taps)) == 0

    def ingest_rows_dev(self, src_ptr: int, src_span: int, src_fmt: int, rows_dev_ptr: int, rows_host: np.ndarray, up: int, down: int,
                        taps: Optional[np.ndarray], dst_ptr: int, dst_span: int, stream: int = 0) -> None:
        """PCM as the file holds it -> f32 rows at the codec rate (rca_codec_ingest_rows_dev).  rows_host: a contiguous array of
        _native.INGEST_ROW records, the host copy of the table at rows_dev_ptr; taps: float32, odd length (None for 1 : 1)."""
        if rows_host.dtype != N.INGEST_ROW or not rows_host.flags.c_contiguous:
            raise ValueError("rows_host must be a contiguous array of _native.INGEST_ROW records")
        if taps is None:
            taps_ptr, n_taps = None, 1
        else:
            taps = np.ascontiguousarray(taps, dtype=np.float32)
            taps_ptr, n_taps = taps.ctypes.data, taps.size
        N.check(self._lib.rca_codec_ingest_rows_dev(self._h, C.c_void_p(src_ptr), C.c_int64(src_span), int(src_fmt), C.c_void_p(rows_dev_ptr),
                                                    C.c_void_p(rows_host.ctypes.data), int(rows_host.size), int(up), int(down),
                                                    C.c_void_p(taps_ptr), int(n_taps), C.c_void_p(dst_ptr), C.c_int64(dst_span),
                                                    C.c_void_p(stream)), "rca_codec_ingest_rows_dev")

    def decode_rows_dev(self, codes_ptr: int, src_off_ptr: int, B: int, F: int, n_samples: int, pcm_ptr: int, dst_off_ptr: int, code_span: int,
                        pcm_span: int, stream: int = 0) -> None:
        """B rows of F codes at codes + src_off[b]; the last n_samples of row b's decode land at pcm + dst_off[b] (each row bit-identical
        to decode_tail_dev of that row).  Destination rows must not overlap."""
        N.check(self._lib.rca_codec_decode_rows_dev(self._h, C.c_void_p(codes_ptr), C.c_void_p(src_off_ptr), B, F, n_samples, C.c_void_p(pcm_ptr),
                                                    C.c_void_p(dst_off_ptr), C.c_int64(code_span), C.c_int64(pcm_span), C.c_void_p(stream)),
                "rca_codec_decode_rows_dev")

    def check_decode_error(self, stream: int = 0) -> None:
        """Synchronise `stream` and raise if a decode kernel flagged a code outside the codebook or a row outside its span."""
        flag = C.c_int32()
        N.check(self._lib.rca_codec_decode_error(self._h, C.c_void_p(stream), C.byref(flag)), "rca_codec_decode_error")
        if flag.value:
            raise N.RcaError(f"decode: code out of range [0, {self.cfg.codebook_size}) or row outside its span")

    def crossfade_join_dev(self, seg_ptr: int, seg_span: int, segs_dev_ptr: int, segs_host: np.ndarray, fade_in_ptr: int, n_fade: int, out_ptr: int,
                           out_span: int, stream: int = 0) -> None:
        """smooth_join of many streams in one launch (rca_codec_crossfade_join_dev).  segs_host: a contiguous array of _native.JOIN_SEG
        records, the host copy of the table at segs_dev_ptr; fade_in_ptr: n_fade float32 on the device (0 when n_fade == 0)."""
        if segs_host.dtype != N.JOIN_SEG or not segs_host.flags.c_contiguous:
            raise ValueError("segs_host must be a contiguous array of _native.JOIN_SEG records")
        N.check(self._lib.rca_codec_crossfade_join_dev(self._h, C.c_void_p(seg_ptr), C.c_int64(seg_span), C.c_void_p(segs_dev_ptr),
                                                       C.c_void_p(segs_host.ctypes.data), int(segs_host.size), C.c_void_p(fade_in_ptr or None),
                                                       int(n_fade), C.c_void_p(out_ptr), C.c_int64(out_span), C.c_void_p(stream)),
                "rca_codec_crossfade_join_dev")

    def encoder_dev(self, pcm_ptr: int, B: int, T: int, ze_ptr: int, stream: int = 0) -> None:
        N.check(self._lib.rca_codec_encoder_dev(self._h, C.c_void_p(pcm_ptr), B, T, C.c_void_p(ze_ptr), C.c_void_p(stream)), "rca_codec_encoder_dev")

    def quantize_dev(self, ze_ptr: int, rows: int, codes_ptr: int, stream: int = 0) -> None:
        N.check(self._lib.rca_codec_quantize_dev(self._h, C.c_void_p(ze_ptr), C.c_int64(rows), C.c_void_p(codes_ptr), C.c_void_p(stream)), "rca_codec_quantize_dev")

    def decoder_dev(self, zq_ptr: int, B: int, F: int, pcm_ptr: int, stream: int = 0) -> None:
        N.check(self._lib.rca_codec_decoder_dev(self._h, C.c_void_p(zq_ptr), B, F, C.c_void_p(pcm_ptr), C.c_void_p(stream)), "rca_codec_decoder_dev")

    def codebook_dev_ptr(self) -> int:
        p = C.c_void_p()
        N.check(self._lib.rca_codec_codebook_dev(self._h, C.byref(p)), "rca_codec_codebook_dev")
        return p.value

    def profile(self, enable: bool) -> None:
        N.check(self._lib.rca_codec_profile(self._h, 1 if enable else 0), "rca_codec_profile")

    def profile_read(self, kclass: int) -> dict:
        ms, n, fl, by = C.c_double(), C.c_int64(), C.c_double(), C.c_double()
        N.check(self._lib.rca_codec_profile_read(self._h, kclass, C.byref(ms), C.byref(n), C.byref(fl), C.byref(by)), "rca_codec_profile_read")
        return dict(ms=ms.value, launches=n.value, flops=fl.value, bytes=by.value)

    def frames_per_chunk(self, chunk_samples: int) -> int:
        # int(audio_secs * framerate) as audio_tokenizer.py:99-100
        return int((chunk_samples / self.cfg.sample_rate) * self.cfg.framerate)


# ----------------------------------------------------------------------------------------------
def _torch():
    import torch
    return torch


def _stream_of(t) -> int:
    torch = _torch()
    return int(torch.cuda.current_stream(t.device).cuda_stream)


class _Codebook:
    def __init__(self, weight):
        self.weight = weight


class _Quantizer:
    """quantizer.inference / .codebook.weight / .codebook_proj (audio_tokenizer.py:158,192,198)."""

    def __init__(self, model: "MagiCodecHIP"):
        self._m = model
        torch = _torch()
        self.codebook = _Codebook(torch.from_numpy(model._weights["quantizer.codebook.weight"]).to(model.device))
        self._cb_proj = None

    def projected_codebook(self):
        if self._cb_proj is None:
            torch = _torch()
            # the handle computed codebook_proj(codebook.weight) once at load; fetch that constant
            self._cb_proj = torch.from_numpy(self._m.hip.codebook()).to(self._m.device)
        return self._cb_proj

    def codebook_proj(self, w):
        # The projection of the model's own codebook is a constant computed once at load
        # (rca_codec_create); any other input goes through the same linear map on the device.
        if w is self.codebook.weight:
            return self.projected_codebook()
        torch = _torch()
        pw = torch.from_numpy(self._m._weights["quantizer.codebook_proj.weight"]).to(w.device)
        pb = torch.from_numpy(self._m._weights["quantizer.codebook_proj.bias"]).to(w.device)
        return torch.nn.functional.linear(w.float(), pw, pb)

    def inference(self, z_e):
        torch = _torch()
        B, F, D = z_e.shape
        z_e = z_e.contiguous().float()
        idx = torch.empty((B, F), dtype=torch.int64, device=z_e.device)
        self._m.hip.quantize_dev(z_e.data_ptr(), B * F, idx.data_ptr(), _stream_of(z_e))
        z_q = torch.nn.functional.embedding(idx, self.projected_codebook())
        return z_q, idx


class MagiCodecHIP:
    """Model object with the MagiCodec attribute surface, every op a HIP kernel of this repo."""

    def __init__(self, cfg: Optional[CodecConfig] = None, weights: Optional[Dict[str, np.ndarray]] = None, device=None, seed: int = 0):
        torch = _torch()
        if not torch.cuda.is_available():
            raise N.RcaError("MagiCodecHIP needs a GPU (torch.cuda.is_available() is False); there is no CPU fallback")
        self.cfg = cfg or CodecConfig()
        self._weights = weights if weights is not None else init_codec_weights(self.cfg, seed)
        if device is None:
            device = torch.device("cuda", torch.cuda.current_device())
        elif not isinstance(device, torch.device):
            device = torch.device(device)
        if device.type != "cuda":
            raise N.RcaError(f"MagiCodecHIP cannot live on device '{device}'")
        if device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        self.device = device
        self.hip = HipCodec(self.cfg, self._weights, device.index)
        self.codebook_size = self.cfg.codebook_size
        self.sample_rate = self.cfg.sample_rate
        self.hop = self.cfg.hop
        self.quantizer = _Quantizer(self)

    # nn.Module-like no-ops used by the reference (audio_tokenizer.py:28)
    def eval(self):
        return self

    def to(self, device):
        torch = _torch()
        d = torch.device(device) if not isinstance(device, torch.device) else device
        if d.type != "cuda" or (d.index is not None and d.index != self.device.index):
            raise N.RcaError(f"MagiCodecHIP is bound to {self.device}; cannot move to {d}")
        return self

    def pad_audio(self, x):
        torch = _torch()
        pad = (-x.shape[-1]) % self.hop
        return torch.nn.functional.pad(x, (0, pad)) if pad else x

    def encoder(self, x):
        torch = _torch()
        x = x.contiguous().float()
        B, T = x.shape
        F = self.hip.num_frames(T)
        ze = torch.empty((B, F, self.cfg.latent_dim), dtype=torch.float32, device=x.device)
        self.hip.encoder_dev(x.data_ptr(), B, T, ze.data_ptr(), _stream_of(x))
        return ze

    def decoder(self, z_q):
        torch = _torch()
        z_q = z_q.contiguous().float()
        B, F, J = z_q.shape
        pcm = torch.empty((B, 1, F * self.hop), dtype=torch.float32, device=z_q.device)
        self.hip.decoder_dev(z_q.data_ptr(), B, F, pcm.data_ptr(), _stream_of(z_q))
        return pcm

    # fused fast paths used by this repo's AudioTokenizer
    def encode_codes(self, x):
        """pad_audio -> encoder -> quantizer.inference in one C-ABI call: [B,T] f32 -> [B,F] int64."""
        torch = _torch()
        x = x.contiguous().float()
        B, T = x.shape
        codes = torch.empty((B, self.hip.num_frames(T)), dtype=torch.int64, device=x.device)
        self.hip.encode_dev(x.data_ptr(), B, T, codes.data_ptr(), _stream_of(x))
        return codes

    def encode_tail(self, x, n_keep: int):
        """The last n_keep columns of encode_codes(x), bit-identical, at the cost of n_keep + margin frames:
        what tokenize_audio keeps of each rolling window (audio_tokenizer.py:98-101).  [B,T] f32 -> [B,n_keep] int64."""
        torch = _torch()
        x = x.contiguous().float()
        B, T = x.shape
        n_keep = min(int(n_keep), self.hip.num_frames(T))
        codes = torch.empty((B, n_keep), dtype=torch.int64, device=x.device)
        self.hip.encode_tail_dev(x.data_ptr(), B, T, n_keep, codes.data_ptr(), _stream_of(x))
        return codes

    def encode_tail_np(self, x: np.ndarray, n_keep: int) -> np.ndarray:
        """encode_tail on host arrays, no torch in the loop: what AudioTokenizer calls once per frame."""
        return self.hip.encode_tail(x, n_keep)

    def decode_tail_np(self, codes: np.ndarray, n_samples: int) -> np.ndarray:
        """decode_tail on host arrays: [B,F] int64 -> [B,min(n_samples, F*hop)] f32."""
        return self.hip.decode_tail(codes, n_samples)

    def decode_tail(self, codes, n_samples: int):
        """The last n_samples of decode_codes(codes), bit-identical (audio_tokenizer.py:141-145).
        [B,F] int64 -> [B,1,min(n_samples, F*hop)] f32."""
        torch = _torch()
        codes = codes.contiguous().to(torch.int64)
        B, F = codes.shape
        n = min(int(n_samples), F * self.hop)
        pcm = torch.empty((B, 1, n), dtype=torch.float32, device=codes.device)
        self.hip.decode_tail_dev(codes.data_ptr(), B, F, n, pcm.data_ptr(), _stream_of(codes))
        return pcm

    def run_stream_plan(self, codes_dev, plan, fade_in: np.ndarray, batch: int = 256, times: Optional[dict] = None):
        """Execute a stream_decode.BatchPlan on the device: codes_dev is the flat int64 code buffer the plan was laid over (a torch
        tensor on this device).  Every row group goes through rca_codec_decode_rows_dev in passes of `batch` rows, then ONE
        rca_codec_crossfade_join_dev writes the joined streams.  -> flat f32 device tensor [plan.out_span]; everything is enqueued
        on the current stream, nothing is synchronised (HipCodec.check_decode_error does both)."""
        torch = _torch()
        dev = codes_dev.device
        n_rows, S = len(plan.F), len(plan.segs)
        out = torch.empty(max(plan.out_span, 1), dtype=torch.float32, device=dev)
        if n_rows == 0:
            return out[:0]
        st = _stream_of(codes_dev)
        tab = torch.from_numpy(np.concatenate([plan.src, plan.dst]).astype(np.int64)).pin_memory().to(dev, non_blocking=True)
        segs_host = np.ascontiguousarray(plan.segs)
        segs_dev = torch.from_numpy(segs_host.view(np.uint8).copy()).pin_memory().to(dev, non_blocking=True)
        fade_dev = torch.from_numpy(np.ascontiguousarray(fade_in, dtype=np.float32)).to(dev) if plan.n_fade else None
        pieces = torch.empty(plan.seg_span, dtype=torch.float32, device=dev)
        src_ptr, dst_ptr = tab.data_ptr(), tab.data_ptr() + 8 * n_rows
        for F, n, a, b in plan.groups:
            for k in range(a, b, batch):
                self.hip.decode_rows_dev(codes_dev.data_ptr(), src_ptr + 8 * k, min(batch, b - k), F, n, pieces.data_ptr(), dst_ptr + 8 * k,
                                         plan.code_span, plan.seg_span, st)
                if times is not None:
                    times["passes"] = times.get("passes", 0) + 1
        self.hip.crossfade_join_dev(pieces.data_ptr(), plan.seg_span, segs_dev.data_ptr(), segs_host, fade_dev.data_ptr() if plan.n_fade else 0,
                                    plan.n_fade, out.data_ptr(), plan.out_span, st)
        # the tables and the pieces are read by work still in flight: the caching allocator hands their memory out again only to
        # later work on the same stream, which runs after it
        return out[:plan.out_span]

    def stream_decode_np(self, codes: np.ndarray, chunk_frames: int, context_frames: int, preroll: int, fade_in: Optional[np.ndarray] = None,
                         have: int = 0, clip: bool = True, batch: int = 256) -> np.ndarray:
        """R independent streams rendered as the per-chunk loop renders them (detokenize_audio(chunk, preroll_samples=preroll) +
        smooth_join per chunk of chunk_frames codes, context_frames of rolling code context), the whole plan on the device.
        codes [R, have + N] int64: `have` codes of earlier context, then the N codes to render.  fade_in: the `preroll` ramp values
        (default: create_crossfade_ramps' equal-power ramp).  -> f32 [R, N_out], bit-identical to the loop."""
        from .stream_decode import plan_batch
        torch = _torch()
        codes = np.ascontiguousarray(codes, dtype=np.int64)
        if codes.ndim != 2 or codes.shape[1] < have:
            raise ValueError("codes must be [R, have + N]")
        R, N_ = codes.shape[0], codes.shape[1] - have
        if fade_in is None:
            fade_in = np.sin(0.5 * np.pi * np.linspace(0, 1, preroll, endpoint=False, dtype=np.float32))
        if len(fade_in) != preroll:
            raise ValueError(f"fade_in holds {len(fade_in)} values for a preroll of {preroll}")
        dec_left = self.hip.receptive_field()[1] if clip else None
        plan = plan_batch([N_] * R, [have] * R, chunk_frames, context_frames, preroll, self.hop, self.cfg.framerate, self.cfg.sample_rate,
                          dec_left=dec_left)
        if plan.out_span == 0:
            return np.zeros((R, 0), np.float32)
        with torch.cuda.device(self.device):
            codes_dev = torch.from_numpy(codes.reshape(-1)).to(self.device)
            out = self.run_stream_plan(codes_dev, plan, fade_in, batch)
            self.hip.check_decode_error(_stream_of(codes_dev))
            return out.cpu().numpy().reshape(R, -1)

    def decode_codes(self, codes):
        """embedding(codes, projected codebook) -> decoder in one C-ABI call: [B,F] int64 -> [B,1,T] f32."""
        torch = _torch()
        codes = codes.contiguous().to(torch.int64)
        B, F = codes.shape
        pcm = torch.empty((B, 1, F * self.hop), dtype=torch.float32, device=codes.device)
        self.hip.decode_dev(codes.data_ptr(), B, F, pcm.data_ptr(), _stream_of(codes))
        return pcm


_MODEL_REGISTRY = {"MagiCodec-50Hz-Base": CodecConfig}


def load_magicodec_model(name: str, device, seed: int = 0) -> Tuple[MagiCodecHIP, None, None]:
    """Stand-in for codec_bpe.tools.codec_utils.load_magicodec_model (audio_tokenizer.py:8,27):
    same (model, _, _) return shape.  No checkpoint exists offline, so the named architecture
    is built with seeded random weights."""
    if name not in _MODEL_REGISTRY:
        raise ValueError(f"unknown codec model '{name}' (known: {sorted(_MODEL_REGISTRY)})")
    return MagiCodecHIP(_MODEL_REGISTRY[name](), device=device, seed=seed), None, None
