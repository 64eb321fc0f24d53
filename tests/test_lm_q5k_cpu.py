"""GGUF Q5_K on the host: the block layout restated in tests/q5k_ref.py and _native.Q5KBlocks against an independent per-weight loop,
this build's load-time quantiser, and the importer (Q5_K-only files and the Q5_K_M mix of Q5_K and Q6_K tensors)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lm_q5k_cases as C  # noqa: E402
import q5k_ref  # noqa: E402


def _loop_dequantize(raw: np.ndarray) -> np.ndarray:
    """The bit rules of block_q5_K, one weight at a time, the arithmetic in float64 (each product of an fp16 value and a 6-bit integer,
    and of that with a 5-bit integer, is exact in float64 AND in f32, so only the final subtraction rounds: once, to f32)."""
    out = np.empty((raw.shape[0], 256), np.float32)
    for b, blk in enumerate(raw):
        d = float(blk[0:2].copy().view(np.float16)[0])
        dmin = float(blk[2:4].copy().view(np.float16)[0])
        scales, qh, qs = blk[4:16], blk[16:48], blk[48:176]
        for j in range(8):                                   # get_scale_min_k4
            if j < 4:
                sc, m = int(scales[j]) & 63, int(scales[j + 4]) & 63
            else:
                sc = (int(scales[j + 4]) & 0xF) | ((int(scales[j - 4]) >> 6) << 4)
                m = (int(scales[j + 4]) >> 4) | ((int(scales[j]) >> 6) << 4)
            t, high = j >> 1, j & 1
            for l in range(32):
                nib = (int(qs[32 * t + l]) >> 4) if high else (int(qs[32 * t + l]) & 0xF)
                q = nib | (((int(qh[l]) >> (2 * t + high)) & 1) << 4)
                out[b, 64 * t + 32 * high + l] = np.float32(np.float32((d * sc) * q) - np.float32(dmin * m))
    return out


def test_pack_and_dequantise_equal_the_per_weight_bit_rules():
    from realtime_codec_agent_amd._native import Q5KBlocks
    rng = np.random.default_rng(3)
    nb = 24
    raw = rng.integers(0, 256, (nb, q5k_ref.BLOCK_BYTES), dtype=np.uint8)
    raw[:, 0:2] = (rng.uniform(1e-3, 2e-2, (nb, 1))).astype(np.float16).view(np.uint8)
    raw[:, 2:4] = (rng.uniform(1e-3, 2e-2, (nb, 1))).astype(np.float16).view(np.uint8)
    qh = raw[:, 16:48]
    for bit in range(8):                                     # both values of every one of the 8 bit positions occur
        assert ((qh >> bit) & 1).any() and not ((qh >> bit) & 1).all()
    want = _loop_dequantize(raw)
    assert np.array_equal(q5k_ref.dequantize_blocks(raw).reshape(nb, 256), want)
    assert np.array_equal(Q5KBlocks(raw, (nb, 256)).dequantize(), want)
    # pack is unpack's inverse: every field of a random block survives the round trip
    q, sc, m, d, dmin = q5k_ref.unpack(raw)
    assert q.max() == 31 and q.min() == 0
    again = q5k_ref.pack_blocks(dict(q=q, sc=sc, m=m, d=d.astype(np.float16), dmin=dmin.astype(np.float16)))
    assert np.array_equal(again, raw)


def test_the_quantiser_uses_the_fifth_bit_and_stays_within_one_step():
    """The numpy restatement of the load-time rule (q5k_ref.quantize_q5_k) is not vacuous.  This covers no product code by itself:
    test_lm_q5k_gpu.py::test_the_device_quantiser_is_the_numpy_rule_block_for_block ties the device rule to it bit for bit."""
    rng = np.random.default_rng(4)
    w = (rng.standard_normal((16, 768)) * 0.05).astype(np.float32)
    p = q5k_ref.quantize_q5_k(w)
    assert p["q"].max() == 31 and p["q"].min() == 0
    frac = float((p["q"] >= 16).mean())
    assert 0.30 <= frac <= 0.70, frac
    got = q5k_ref.fake_quant(w)
    step = (p["d"].astype(np.float32).repeat(8, -1) * p["sc"].astype(np.float32)).astype(np.float32)       # d * sc per sub-block
    err = np.abs(got - w).reshape(16, 24, 32).max(-1)
    assert np.all(err <= step), float((err / np.where(step > 0, step, 1)).max())
    # twice the resolution of the Q4_K rule on the same rows
    from oracle import q4k_ref
    assert np.abs(got - w).mean() < 0.6 * np.abs(q4k_ref.fake_quant(w) - w).mean()


def test_q5_k_gguf_round_trip_and_the_q5_k_m_mix(tmp_path):
    from realtime_codec_agent_amd._native import Q5KBlocks, Q6KBlocks
    from realtime_codec_agent_amd.gguf import GGUFError, load_llama_gguf, read_gguf
    path = str(tmp_path / "q5k.gguf")
    cfg = C.write_file("q5_k", path)
    wf = C.f32_weights(cfg, C.FILES["q5_k"][2])
    cfg2, file_w, _ = load_llama_gguf(path)
    assert cfg2.hidden == cfg.hidden and cfg2.n_layers == 2
    for k in ("self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj", "mlp.down_proj"):
        t = file_w[f"model.layers.1.{k}.weight"]
        assert isinstance(t, Q5KBlocks) and t.raw.shape[1] == t.shape[1] // 256 * 176
        # rows come back in Hugging Face order: equal to quantising the un-permuted source (a block never crosses a row)
        assert np.array_equal(t.dequantize(), q5k_ref.fake_quant(wf[f"model.layers.1.{k}.weight"])), k
    assert isinstance(file_w["lm_head.weight"], Q5KBlocks)
    emb = file_w["model.embed_tokens.weight"]
    assert emb.dtype == np.float32 and np.array_equal(emb, q5k_ref.fake_quant(wf["model.embed_tokens.weight"]))
    # a Q5_K tensor whose size is no multiple of 256
    bad = str(tmp_path / "bad.gguf")
    import gguf_writer as gw
    import struct
    head = struct.pack("<IIQQ", 0x46554747, 3, 1, 0) + gw._s(b"t") + struct.pack("<I", 1) + struct.pack("<Q", 300) + struct.pack("<IQ", 13, 0)
    with open(bad, "wb") as f:
        f.write(head + b"\0" * ((-len(head)) % 32) + b"\0" * 352)
    with pytest.raises(GGUFError, match="Q5_K tensor whose size is not a multiple of 256"):
        read_gguf(bad)
    # the Q5_K_M mix: both block classes, Q6_K where llama-quantize puts it
    mix = str(tmp_path / "q5_k_m.gguf")
    C.write_file("q5_k_m", mix)
    _, fw, _ = load_llama_gguf(mix)
    assert isinstance(fw["lm_head.weight"], Q6KBlocks) and isinstance(fw["model.layers.0.mlp.gate_proj.weight"], Q5KBlocks)
    six = [l for l in range(8) if isinstance(fw[f"model.layers.{l}.self_attn.v_proj.weight"], Q6KBlocks)]
    assert six == [l for l in range(8) if isinstance(fw[f"model.layers.{l}.mlp.down_proj.weight"], Q6KBlocks)] == [0, 3, 6, 7]
    assert all(isinstance(fw[f"model.layers.{l}.self_attn.v_proj.weight"], Q5KBlocks) for l in (1, 2, 4, 5))
    assert all(isinstance(fw[f"model.layers.{l}.self_attn.q_proj.weight"], Q5KBlocks) for l in range(8))


@pytest.mark.parametrize("name", sorted(C.FILES))
def test_the_file_cases_have_a_clear_argmax(name, tmp_path):
    """what test_lm_q5k_gpu.py's argmax comparison relies on: the oracle's two largest logits are further apart than twice the tolerance"""
    path = str(tmp_path / f"{name}.gguf")
    C.write_file(name, path)
    _, want, gap = C.file_oracle(name, path)
    print(f"{name}: top-two gap {gap:.4f}, needed {C.gap_needed(want):.4f} (|logit| max {np.abs(want).max():.2f})")
    assert gap > C.gap_needed(want)


def test_refused_types_name_q5_k_among_the_supported_ones():
    from realtime_codec_agent_amd import gguf
    with pytest.raises(gguf.GGUFError, match="Q3_K is not supported .*Q5_K"):
        gguf._nbytes(11, 256)
    with pytest.raises(gguf.GGUFError, match="Q5_0 is not supported .*Q5_K"):
        gguf._dequant(np.zeros(22, np.uint8), 6, 32)
