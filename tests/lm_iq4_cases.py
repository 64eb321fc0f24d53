"""Models and files shared by tests/test_lm_iq4_cpu.py and tests/test_lm_iq4_gpu.py (TEST INFRASTRUCTURE ONLY)."""
import functools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import iq4_ref  # noqa: E402
from lm_shape_cases import TOL_EXACT, TOL_TILE  # noqa: E402,F401
from oracle import lm_ref  # noqa: E402

INIT_STD = 0.05
FILE_PROMPT = 40
# name -> (matrix type for iq4_ref.write_llama_gguf, layers, weight seed, prompt seed).  "iq4_xs_mix" is IQ4_XS as llama-quantize writes
# it: output.weight Q6_K, attn_v and layer 0's ffn_down Q5_K beside IQ4_XS neighbours.
# The argmax of a compared position is checked only where the oracle's two largest logits are more than 2 * TOL_TILE * max(1, |logit|max)
# apart (it cannot flip inside the tolerance then); the seeds are chosen so that every file's compared position qualifies (3 of 3, above
# the 90 % the comparison needs): test_lm_iq4_cpu.py checks that without a GPU.
FILES = {"iq4_nl": (iq4_ref.IQ4_NL, 2, 6, 5), "iq4_xs": (iq4_ref.IQ4_XS, 2, 6, 4), "iq4_xs_mix": ("IQ4_XS_MIX", 2, 6, 4)}


def file_config(name: str):
    from realtime_codec_agent_amd.llm import LMConfig
    return LMConfig(vocab_size=1024, hidden=256, n_layers=FILES[name][1], n_heads=4, n_kv_heads=2, head_dim=64, ffn=512, rope_scaling=None,
                    rope_theta=10000.0)


def f32_weights(cfg, seed: int) -> dict:
    """the state dict rca_lm_create_random generates for (cfg, seed), as float32"""
    from realtime_codec_agent_amd.llm import bf16_bits_to_f32
    return {k: (bf16_bits_to_f32(v) if v.dtype == np.uint16 else v.astype(np.float32)) for k, v in lm_ref.random_weights(cfg, seed, INIT_STD).items()}


def write_file(name: str, path: str):
    cfg = file_config(name)
    iq4_ref.write_llama_gguf(path, cfg, f32_weights(cfg, FILES[name][2]), matrix_type=FILES[name][0], seed=FILES[name][2])
    return cfg


def file_ids(name: str) -> np.ndarray:
    return np.random.default_rng(FILES[name][3]).integers(0, 1024, FILE_PROMPT)


@functools.lru_cache(maxsize=None)
def file_oracle(name: str, path: str):
    """(tensors as the importer returns them, LMRef logits of the prompt's last position over the file's own blocks de-quantised on
    the host with an fp16 KV cache, top-two gap of those logits)"""
    import torch
    from realtime_codec_agent_amd.gguf import load_llama_gguf
    cfg = file_config(name)
    _, file_w, _ = load_llama_gguf(path)
    deq = {k: (v.dequantize() if hasattr(v, "dequantize") else np.array(v)) for k, v in file_w.items() if k != "rope.inv_freq"}
    want = lm_ref.LMRef(cfg, deq, kv_dtype=torch.float16).eval(file_ids(name))[-1].numpy()
    want.setflags(write=False)
    top = np.sort(want)[-2:]
    return file_w, want, float(top[1] - top[0])


def gap_needed(want: np.ndarray) -> float:
    return 2 * TOL_TILE * max(1.0, float(np.abs(want).max()))


def xs_scale_blocks(nb: int = 8):
    """IQ4_XS super-blocks that use all 64 scale codes and both nibble positions of scales_l, with every bit pair of scales_h taking all of
    its four values: block b, sub-block ib has ls = (8 b + 9 ib + (b >> 3)) mod 64.  -> (raw [nb, 136], q [nb, 256], d f16 [nb], ls [nb, 8])"""
    assert nb >= 8
    b, ib = np.meshgrid(np.arange(nb), np.arange(8), indexing="ij")
    ls = ((8 * b + 9 * ib + (b >> 3)) % 64).astype(np.int32)
    k = np.arange(256)
    q = ((5 * k[None, :] + 3 * np.arange(nb)[:, None] + (k[None, :] >> 4)) & 15).astype(np.uint8)
    d = (np.where(np.arange(nb) % 3 == 0, -1.0, 1.0) * 2.0 ** -(8 + np.arange(nb) % 4) * (1 + np.arange(nb) % 5 / 8)).astype(np.float16)
    return iq4_ref.pack_iq4_xs(dict(q=q, d=d, ls=ls)), q, d, ls
