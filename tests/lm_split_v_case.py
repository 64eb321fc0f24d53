"""The two-layer Q4_K_M file of tests/test_lm_q8_1_gpu.py as handles over one set of weights, for the routes of the 128-token tiles.

llama-quantize's Q4_K_M mix gives layer 1 a Q6_K attn_v beside Q4_K attn_q / attn_k, so that layer's V projection is a GEMM of its own
with a row base in the RoPE / KV-write epilogue (the second segment of the QKV loop of lm_enqueue_layers128); layer 0 keeps [q; k; v]
as one matrix.  hidden 256, 4 heads over 2 kv heads: small enough for contexts under 300 tokens to run in well under a second."""
import functools
import tempfile

import numpy as np

import lm_q8_1_ref as R
from oracle import lm_ref

NAME = "q4_k_m_gguf"
N_CTX = 288


def ids():
    return np.random.default_rng(17).integers(0, R.GGUF_MODEL["vocab_size"], N_CTX).tolist()


def write_file(path):
    import gguf_writer as gw
    from realtime_codec_agent_amd.gguf import load_llama_gguf
    from realtime_codec_agent_amd.llm import LMConfig, bf16_bits_to_f32
    g = R.GGUF_MODEL
    cfg = LMConfig(vocab_size=g["vocab_size"], hidden=g["hidden"], n_layers=g["n_layers"], n_heads=g["n_heads"], n_kv_heads=g["n_kv_heads"],
                   head_dim=64, ffn=g["ffn"], rope_scaling=None, rope_theta=10000.0)
    w = lm_ref.random_weights(cfg, g["seed"], 0.05)
    wf = {k: (bf16_bits_to_f32(v) if v.dtype == np.uint16 else v.astype(np.float32)) for k, v in w.items()}
    gw.write_llama_gguf(path, cfg, wf, matrix_type="Q4_K_M")
    kinds = {k: type(v).__name__ for k, v in load_llama_gguf(path)[1].items()}
    assert kinds["model.layers.1.self_attn.v_proj.weight"] == "Q6KBlocks" and kinds["model.layers.1.self_attn.q_proj.weight"] == "Q4KBlocks"
    assert kinds["model.layers.0.self_attn.v_proj.weight"] == "Q4KBlocks"


@functools.lru_cache(maxsize=None)
def family(size, kv_format="f16"):
    """a parent loaded from the file and size - 1 twins that share its weights"""
    from realtime_codec_agent_amd.llm import LlamaForAlternatingCodeChannels as L
    with tempfile.TemporaryDirectory() as d:
        write_file(f"{d}/two-layer-q4_k_m.gguf")
        parent = L(model_path=f"{d}/two-layer-q4_k_m.gguf", n_ctx=N_CTX, device=0, kv_format=kv_format)
    assert parent.prefill_route() == "gemm128" and parent.kv_format == kv_format
    return [parent] + [L(n_ctx=N_CTX, share_weights_with=parent, device=0) for _ in range(size - 1)]
