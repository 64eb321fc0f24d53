"""Quantising checkpoints on the card: rca_quantize_rows against the numpy restatement (tests/quant_search_ref.py) byte for byte, its
refusals, and the models realtime_codec_agent_amd.quantize makes -- in memory against LMRef over their own blocks, as a written file
against the in-memory handle, and through the command line."""
import ctypes
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lm_shape_cases as sc  # noqa: E402
import q5k_ref  # noqa: E402
import quant_search_ref as R  # noqa: E402
from oracle import lm_ref, q4k_ref  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QTYPES = ("q4_k", "q5_k", "q6_k", "q8_0")


def _bf16(w):
    from realtime_codec_agent_amd.llm import bf16_bits_to_f32, f32_to_bf16_bits
    b = f32_to_bf16_bits(w)
    return b, bf16_bits_to_f32(b)


def _sources():
    """name -> (what is handed to the device, the float32 values it holds)"""
    rs = np.random.RandomState(11)
    gauss = (rs.randn(8, 512) * 0.02).astype(np.float32)
    t4 = (rs.standard_t(4, (8, 512)) * 0.02).astype(np.float32)
    out = {}
    for name, w in (("gaussian", gauss), ("student_t4", t4)):
        out[f"8x512 {name} f32"] = (w, w)
        out[f"8x512 {name} bf16"] = _bf16(w)
        out[f"8x512 {name} f16"] = (w.astype(np.float16), w.astype(np.float16).astype(np.float32))
    w = (rs.randn(3, 256) * 0.05).astype(np.float32)
    out["3x256 f32"] = (w, w)
    out["1x2048 bf16"] = _bf16((rs.standard_t(4, (1, 2048)) * 0.02).astype(np.float32))
    edges = np.stack([R.edge_block(k) for k in R.EDGE_BLOCKS])
    out["edge blocks f32"] = (edges, edges)
    exact = np.array([np.array_equal(e.astype(np.float16).astype(np.float32), e) for e in edges])
    assert exact.sum() >= 6
    out["edge blocks f16"] = (edges[exact].astype(np.float16), edges[exact])
    return out


@pytest.mark.parametrize("qtype", QTYPES)
def test_device_search_is_the_restatement_byte_for_byte(qtype):
    """rule = 1 over bf16 / fp16 / f32 sources, one super-block per row with an odd row count, one long row, and every edge block of the
    CPU test (all-zero, constant, one outlier, all-positive, fp16 denormals, amax 65504)."""
    from realtime_codec_agent_amd import quantize as Q
    for name, (src, values) in _sources().items():
        got = Q.quantize_matrix(src, qtype, rule="search", name=name)
        want = R.quantize_blocks(values, qtype)
        assert type(got) is Q.TYPES[qtype][1] and got.shape == values.shape
        bad = np.argwhere(got.raw != want)
        assert bad.size == 0, f"{qtype} {name}: {len(bad)} bytes differ, first at (row, byte) {bad[0].tolist()}"


@pytest.mark.parametrize("qtype", ["q4_k", "q5_k", "q6_k"])
def test_device_min_max_rule_is_what_weight_format_keeps(qtype):
    """rule = 0: the bytes of oracle/q4k_ref.py / tests/q5k_ref.py, the rule weight_format="q4_k" / "q5_k" applies at load (tests/
    test_lm_q5k_gpu.py compares that path with the same numpy rule); for Q6_K q4k_ref.quantize_q6_k."""
    from realtime_codec_agent_amd import quantize as Q
    for name, (src, values) in _sources().items():
        if name.startswith("8x512") or name.startswith("1x2048"):
            got = Q.quantize_matrix(src, qtype, rule="minmax", name=name)
            want = R.minmax_blocks(values, qtype)
            assert np.array_equal(got.raw, want), f"{qtype} {name}"
    w = _sources()["8x512 gaussian bf16"]
    assert not np.array_equal(Q.quantize_matrix(w[0], qtype, rule="minmax").raw, Q.quantize_matrix(w[0], qtype, rule="search").raw)


def test_refusals_name_their_reason_and_write_nothing_past_the_buffer():
    from realtime_codec_agent_amd import _native as N
    lib = N.lib()
    GUARD = 64

    def call(w, K, qtype, rule, nbytes, dtype=N.RCA_F32, rows=None):
        buf = np.full(max(nbytes, 0) + GUARD, 0xA5, np.uint8)
        rc = lib.rca_quantize_rows(0, w.ctypes.data, dtype, w.shape[0] if rows is None else rows, K, qtype, rule, buf.ctypes.data, nbytes)
        assert (buf[max(nbytes, 0):] == 0xA5).all(), "guard bytes were overwritten"
        return rc, lib.rca_last_error().decode(), buf[:max(nbytes, 0)]

    w = np.random.RandomState(2).randn(4, 264).astype(np.float32)
    rc, msg, body = call(w, 264, N.RCA_Q4_K, 1, 4 * 144)
    assert rc == -1 and "K = 264 is not a multiple of 256" in msg and (body == 0xA5).all()
    w = np.random.RandomState(2).randn(4, 256).astype(np.float32)
    rc, msg, body = call(w, 256, N.RCA_Q4_K, 1, 4 * 144 - 1)
    assert rc == -1 and "blocks_bytes = 575" in msg and "take 576" in msg and (body == 0xA5).all()
    rc, msg, body = call(w, 256, N.RCA_F16, 1, 4 * 144)
    assert rc == -1 and "unknown type 3" in msg and (body == 0xA5).all()
    rc, msg, body = call(w, 256, N.RCA_Q4_K, 2, 4 * 144)
    assert rc == -1 and "unknown rule 2" in msg and (body == 0xA5).all()
    rc = lib.rca_quantize_rows(0, None, N.RCA_F32, 4, 256, N.RCA_Q4_K, 1, None, 4 * 144)
    assert rc == -1 and "null pointer" in lib.rca_last_error().decode()
    w[2, 17] = np.inf
    for qtype, bs in ((N.RCA_Q4_K, 144), (N.RCA_Q5_K, 176), (N.RCA_Q6_K, 210), (N.RCA_Q8_0, 8 * 34)):
        rc, msg, _ = call(w, 256, qtype, 1, 4 * bs)
        assert rc == -1 and "row 2 holds a value that is not finite" in msg, (qtype, msg)
    w[2, 17] = 1e9                                                   # finite, but no fp16 d can hold its scale
    rc, msg, _ = call(w, 256, N.RCA_Q4_K, 1, 4 * 144)
    assert rc == -1 and "row 2: a block's d or dmin is not finite in fp16" in msg
    from realtime_codec_agent_amd import quantize as Q
    with pytest.raises(N.RcaError, match=r"blk\.3\.ffn_up\.weight: .*row 2"):
        Q.quantize_matrix(w, "q6_k", name="blk.3.ffn_up.weight")
    w[2, 17] = 1.0                                                   # and the call works after all of that
    rc, msg, body = call(w, 256, N.RCA_Q4_K, 1, 4 * 144)
    assert rc == 0 and np.array_equal(body.reshape(4, 144), R.quantize_blocks(w, "q4_k"))


# ------------------------------------------------------------------------------------------------------------------ models
PROMPT = 40


def _config():
    from realtime_codec_agent_amd.llm import LMConfig
    return LMConfig(vocab_size=1024, hidden=256, n_layers=8, n_heads=4, n_kv_heads=2, head_dim=64, ffn=512, rope_scaling=None, rope_theta=10000.0,
                    rms_eps=float(np.float32(1e-5)))


@functools.lru_cache(maxsize=None)
def _source():
    return lm_ref.random_weights(_config(), 5, 0.05)                 # seeded bf16 weights


@functools.lru_cache(maxsize=None)
def _quantised(recipe):
    from realtime_codec_agent_amd import quantize as Q
    return Q.quantize_weights(_config(), _source(), recipe)


def _ids():
    return np.random.default_rng(4).integers(0, 1024, PROMPT + 4).tolist()


def _run(llm):
    """a 40-token eval and two 2-token steps -> the three last-position logit rows"""
    ids = _ids()
    rows = []
    for part in (ids[:PROMPT], ids[PROMPT:PROMPT + 2], ids[PROMPT + 2:PROMPT + 4]):
        llm.eval(part)
        rows.append(llm._scores[-1].copy())
    return rows


@functools.lru_cache(maxsize=None)
def _memory_rows(recipe):
    from realtime_codec_agent_amd.llm import LlamaForAlternatingCodeChannels
    g = LlamaForAlternatingCodeChannels(config=_config(), weights=_quantised(recipe), n_ctx=256, device=0)
    out = (g.weight_format, g.weight_bytes_per_step(), g.prefill_route(), _run(g))
    g.close()
    return out


def test_in_memory_q4_k_m_model_is_the_mix_and_matches_the_oracle_over_its_blocks():
    """quantize_weights(..., "q4_k_m") through weights=: the handle reports q4_k, its matrices are the recipe's mix (Q6_K lm_head and, in
    layers 0, 3, 6, 7, attn_v / ffn_down: such a layer's V projection is a matrix of its own on the device, which shows as more bytes
    streamed per step than an all-Q4_K model), and its logits after a 40-token eval and two 2-token steps are within the Q4_K tolerance
    of tests/test_lm_q5k_gpu.py (lm_shape_cases.TOL_TILE on a tile-built cache, TOL_EXACT otherwise) of LMRef over the de-quantised blocks."""
    from realtime_codec_agent_amd import quantize as Q
    cfg, q = _config(), _quantised("q4_k_m")
    for k, v in q.items():
        if k in q.types:
            assert q.types[k] == R.recipe_type(Q.gguf_name(k), cfg.n_layers, "q4_k_m") and type(v) is Q.TYPES[q.types[k]][1], k
    assert {type(v).__name__ for v in q.values() if hasattr(v, "raw")} == {"Q4KBlocks", "Q6KBlocks"}
    assert [l for l in range(8) if q.types[f"model.layers.{l}.self_attn.v_proj.weight"] == "q6_k"] == [0, 3, 6, 7]
    fmt, nbytes, route, got = _memory_rows("q4_k_m")
    assert fmt == "q4_k" and nbytes > _memory_rows("q4_k")[1]
    deq = {k: (v.dequantize() if hasattr(v, "raw") else np.asarray(v)) for k, v in q.items()}
    ref = lm_ref.LMRef(cfg, deq, kv_dtype=torch.float16)
    ids = _ids()
    want = [ref.eval(ids[:PROMPT], last_only=True)[-1].numpy(), ref.eval(ids[PROMPT:PROMPT + 2])[-1].numpy(),
            ref.eval(ids[PROMPT + 2:PROMPT + 4])[-1].numpy()]
    tol = sc.TOL_EXACT if route == "gemv" else sc.TOL_TILE
    for i, (g, w) in enumerate(zip(got, want)):
        d, b = float(np.abs(g - w).max()), sc.bound(w, tol)
        print(f"q4_k_m in memory ({route}) pass {i}: max|dlogit| = {d:.3e}, bound {b:.3e} (|logit| max {np.abs(w).max():.2f})")
        assert d <= b


@pytest.mark.parametrize("recipe", ["q4_k_m", "q5_k_m", "q8_0"])
def test_written_file_computes_what_the_in_memory_model_computes(recipe, tmp_path):
    from realtime_codec_agent_amd import quantize as Q
    from realtime_codec_agent_amd.llm import LlamaForAlternatingCodeChannels
    path = str(tmp_path / f"{recipe}.gguf")
    Q.write_llama_gguf(path, _config(), _quantised(recipe))
    fmt, nbytes, _, want = _memory_rows(recipe)
    g = LlamaForAlternatingCodeChannels(model_path=path, n_ctx=256, device=0)
    assert g.config == _config() and g.weight_format == fmt == recipe[:4] and g.weight_bytes_per_step() == nbytes
    got = _run(g)
    g.close()
    for a, b in zip(got, want):
        assert np.array_equal(a, b)


def test_command_line_writes_the_blocks_quantize_weights_makes(tmp_path):
    """python -m realtime_codec_agent_amd.quantize on the model's F16 twin: every tensor of the file it writes holds the bytes
    quantize_weights gives for the same fp16 values; a quantised source is refused."""
    from realtime_codec_agent_amd import gguf as G
    from realtime_codec_agent_amd import quantize as Q
    from realtime_codec_agent_amd.llm import bf16_bits_to_f32
    cfg = _config()
    f16 = {k: (bf16_bits_to_f32(v).astype(np.float16) if v.ndim == 2 else bf16_bits_to_f32(v)) for k, v in _source().items()}
    src, out = str(tmp_path / "f16.gguf"), str(tmp_path / "out.gguf")
    Q.write_llama_gguf(src, cfg, f16, meta={"tokenizer.ggml.tokens": [f"<{i}>" for i in range(cfg.vocab_size)]})
    cmd = [sys.executable, "-m", "realtime_codec_agent_amd.quantize", "--model", src, "--out", out, "--type", "q4_k_m"]
    p = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "bits per weight" in p.stdout and "blk.0.attn_v.weight" in p.stdout and " bpw " in p.stdout
    want = Q.quantize_weights(cfg, f16, "q4_k_m")
    cfg2, got, meta = G.load_llama_gguf(out)
    assert cfg2 == cfg and meta["general.file_type"] == 15 and meta["tokenizer.ggml.tokens"][5] == "<5>"
    for k, v in want.items():
        if k == "model.embed_tokens.weight":
            assert np.array_equal(got[k], v.dequantize())
        elif hasattr(v, "raw"):
            assert type(got[k]) is type(v) and np.array_equal(got[k].raw, v.raw), k
        else:
            assert np.array_equal(got[k], v), k
    p = subprocess.run(cmd[:4] + [out, "--out", str(tmp_path / "again.gguf"), "--type", "q8_0"], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert p.returncode != 0 and "already quantised" in p.stderr and not os.path.exists(str(tmp_path / "again.gguf"))
