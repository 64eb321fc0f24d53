"""GGUF Q4_0 / Q4_1 on the host: ggml's reference quantisers and block layouts restated in tests/q40_ref.py and
_native.Q40Blocks / Q41Blocks on hand-made blocks, the Q4_K twin the GPU test relies on, and the importer (Q4_0-only and Q4_1-only files
and the mix of Q4_0, Q4_1 and Q6_K tensors a llama-quantize Q4_0 file holds)."""
import os
import struct
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lm_q40_cases as C  # noqa: E402
import q40_ref  # noqa: E402

F32 = np.float32


def _blocks(p, ttype, shape):
    return q40_ref.block_class(ttype)(q40_ref.pack_blocks(p), shape)


def test_q4_0_hand_cases():
    """largest magnitude negative (d > 0) and positive (d < 0), a +v / -v tie (the first wins), an all-zero block"""
    x = np.zeros((5, 32), F32)
    x[0] = np.linspace(-1.0, 0.8, 32)               # largest magnitude -1.0: d = 0.125 > 0
    x[1] = np.linspace(-0.8, 1.0, 32)               # largest magnitude +1.0: d = -0.125 < 0
    x[2, 3], x[2, 9] = 0.5, -0.5                    # tie: +0.5 comes first, d = -0.0625
    x[3, 3], x[3, 9] = -0.5, 0.5                    # tie: -0.5 comes first, d = +0.0625
    p = q40_ref.quantize_q4_0(x)
    d = p["d"].astype(F32).reshape(-1)
    assert d.tolist() == [0.125, -0.125, -0.0625, 0.0625, 0.0]
    assert p["q"][0, 0] == 0 and p["q"][1, 31] == 0            # the extreme value itself maps to q = 0: x / d = -8
    assert p["q"][2, 3] == 0 and p["q"][2, 9] == 15            # -8 and +8 -> min(15, 16)
    assert p["q"][3, 3] == 0 and p["q"][3, 9] == 15
    assert np.all(p["q"][4] == 8)
    got = q40_ref.fake_quant(x, q40_ref.Q4_0)
    assert np.all(got[4] == 0) and np.all(got[2, [3, 9]] == [0.5, -0.4375]) and np.all(got[3, [3, 9]] == [-0.5, 0.4375])
    assert np.abs(got - x).max() <= 0.125 / 2 + 0.125 / 16 + 1e-7   # half a step, and the clipped q = 16 -> 15 at the far end


def test_q4_1_hand_cases():
    """a constant block has d = 0 and reads its minimum back; a ramp uses all 16 steps"""
    x = np.zeros((3, 32), F32)
    x[0] = 0.375
    x[1] = np.arange(32) / 31.0 * 1.5 - 0.5
    p = q40_ref.quantize_q4_1(x)
    assert p["d"].astype(F32).reshape(-1).tolist() == [0.0, F32(np.float16(F32(2.0 - 0.5) / F32(15.0))), 0.0]
    assert p["m"].astype(F32).reshape(-1).tolist() == [0.375, -0.5, 0.0]
    assert np.all(p["q"][0] == 0) and set(np.unique(p["q"][1])) == set(range(16))
    got = q40_ref.fake_quant(x, q40_ref.Q4_1)
    assert np.all(got[0] == F32(0.375)) and np.all(got[2] == 0)
    assert np.abs(got[1] - x[1]).max() <= 0.1 / 2 + 2e-3


@pytest.mark.parametrize("ttype", [q40_ref.Q4_0, q40_ref.Q4_1])
def test_blocks_dequantise_by_the_elementwise_formula_bit_for_bit(ttype):
    """random raw blocks: _native's block class, q40_ref.dequantize_blocks, QMat("q4_k", q, s, t).dequantize() (the form s q - t the device
    evaluates) and a per-weight loop over the bit rules agree bit for bit; pack is unpack's inverse"""
    rng = np.random.default_rng(3)
    nb, bs = 48, q40_ref.BLOCK_BYTES[ttype]
    raw = rng.integers(0, 256, (nb, bs), dtype=np.uint8)
    raw[:, 0:2] = (rng.uniform(1e-3, 2e-2, (nb, 1)) * rng.choice([-1, 1], (nb, 1))).astype(np.float16).view(np.uint8)
    if ttype == q40_ref.Q4_1:
        raw[:, 2:4] = rng.uniform(-0.1, 0.1, (nb, 1)).astype(np.float16).view(np.uint8)
    want = np.empty((nb, 32), F32)
    for b, blk in enumerate(raw):
        d = F32(blk[0:2].copy().view(np.float16)[0])
        m = F32(blk[2:4].copy().view(np.float16)[0]) if ttype == q40_ref.Q4_1 else None
        qs = blk[bs - 16:]
        for j in range(32):
            q = (int(qs[j]) & 0xF) if j < 16 else (int(qs[j - 16]) >> 4)
            want[b, j] = F32(F32(q - 8) * d) if m is None else F32(F32(F32(q) * d) + m)
    blocks = q40_ref.block_class(ttype)(raw, (nb // 8, 256))
    assert np.array_equal(blocks.dequantize().reshape(nb, 32), want)
    assert np.array_equal(q40_ref.dequantize_blocks(raw, ttype).reshape(nb, 32), want)
    assert np.array_equal(q40_ref.qmat(blocks).dequantize().reshape(nb, 32), want)
    q, d, m = q40_ref.unpack(raw, ttype)
    assert q.max() == 15 and q.min() == 0
    p = dict(q=q, d=d.astype(np.float16)) if m is None else dict(q=q, d=d.astype(np.float16), m=m.astype(np.float16))
    assert np.array_equal(q40_ref.pack_blocks(p), raw)
    assert np.array_equal(blocks.take_rows([2, 0]).dequantize(), blocks.dequantize()[[2, 0]]) and type(blocks.take_rows([1])) is type(blocks)


def test_the_quantisers_stay_within_half_a_step():
    """the numpy restatements are not vacuous; test_lm_q40_gpu.py ties the device rule to them bit for bit"""
    rng = np.random.default_rng(4)
    w = (rng.standard_normal((16, 768)) * 0.05).astype(F32)
    for ttype in (q40_ref.Q4_0, q40_ref.Q4_1):
        p = q40_ref.quantize(w, ttype)
        assert p["q"].max() == 15 and p["q"].min() == 0
        step = np.abs(p["d"].astype(F32))
        err = np.abs(q40_ref.fake_quant(w, ttype) - w).reshape(16, 24, 32).max(-1)
        # half a step + the fp16 rounding of d (and m) over at most 15 steps; Q4_0 clips x / d = +8 to q = 15: one whole step there
        lim = (1.0 if ttype == q40_ref.Q4_0 else 0.5) * step + 16 * step * 2.0 ** -11 + (np.abs(p["m"].astype(F32)) * 2.0 ** -11 if "m" in p else 0)
        assert np.all(err <= lim * (1 + 1e-6)), float((err / lim).max())
    assert np.abs(q40_ref.fake_quant(w, q40_ref.Q4_1) - w).mean() < np.abs(q40_ref.fake_quant(w, q40_ref.Q4_0) - w).mean()


@pytest.mark.parametrize("ttype", [q40_ref.Q4_0, q40_ref.Q4_1])
def test_a_block_run_with_constant_factors_is_a_q4_k_tensor(ttype):
    """the fixture of test_lm_q40_gpu.py's twin test: the host de-quantisations are equal bit for bit, with d0 of both signs"""
    a, b = q40_ref.twin_matrix(np.random.default_rng(8), 12, 512, ttype)
    assert type(a).__name__ == ("Q41Blocks" if ttype == q40_ref.Q4_1 else "Q40Blocks") and type(b).__name__ == "Q4KBlocks"
    d0 = b.raw.reshape(-1, 144)[:, 0:2].copy().view(np.float16)
    assert (d0 > 0).any() and (d0 < 0).any()
    assert np.array_equal(a.dequantize(), b.dequantize()) and np.abs(a.dequantize()).max() > 0
    import lm_q8_1_ref as R
    qa, qb = q40_ref.qmat(a), R.QMat.from_blocks(b)                    # and the same (q, s, t) for the integer form
    assert np.array_equal(qa.q, qb.q) and np.array_equal(qa.s, qb.s) and np.array_equal(qa.m, qb.m)


def test_gguf_round_trip_of_the_three_files(tmp_path):
    from realtime_codec_agent_amd._native import Q40Blocks, Q41Blocks, Q6KBlocks
    from realtime_codec_agent_amd.gguf import GGUFError, load_llama_gguf, read_gguf
    for name, cls, ttype in (("q4_0", Q40Blocks, q40_ref.Q4_0), ("q4_1", Q41Blocks, q40_ref.Q4_1)):
        path = str(tmp_path / f"{name}.gguf")
        cfg = C.write_file(name, path)
        wf = C.f32_weights(cfg, C.FILES[name][2])
        cfg2, file_w, _ = load_llama_gguf(path)
        assert cfg2.hidden == cfg.hidden and cfg2.n_layers == 2
        for k in ("self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj", "mlp.down_proj"):
            t = file_w[f"model.layers.1.{k}.weight"]
            assert type(t) is cls and t.raw.shape[1] == t.shape[1] // 32 * q40_ref.BLOCK_BYTES[ttype]
            # rows come back in Hugging Face order: equal to quantising the un-permuted source (a block never crosses a row)
            assert np.array_equal(t.dequantize(), q40_ref.fake_quant(wf[f"model.layers.1.{k}.weight"], ttype)), k
        assert type(file_w["lm_head.weight"]) is cls
        emb = file_w["model.embed_tokens.weight"]
        assert emb.dtype == np.float32 and np.array_equal(emb, q40_ref.fake_quant(wf["model.embed_tokens.weight"], ttype))
    mix = str(tmp_path / "mix.gguf")
    C.write_file("q4_0_mix", mix)
    _, fw, _ = load_llama_gguf(mix)
    assert type(fw["lm_head.weight"]) is Q6KBlocks
    assert type(fw["model.layers.0.mlp.down_proj.weight"]) is Q41Blocks and type(fw["model.layers.1.mlp.down_proj.weight"]) is Q40Blocks
    assert all(type(fw[f"model.layers.{l}.{k}.weight"]) is Q40Blocks for l in range(2)
               for k in ("self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj", "self_attn.o_proj", "mlp.gate_proj", "mlp.up_proj"))
    # a Q4_0 tensor whose size is no multiple of 32, and one whose data the file does not hold
    import gguf_writer as gw
    for numel, nbytes, msg in ((300, 352, "Q4_0 tensor whose size is not a multiple of 32"), (512, 16 * 18 - 4, "tensor 't' runs past the end of the file")):
        bad = str(tmp_path / f"bad{numel}.gguf")
        head = struct.pack("<IIQQ", 0x46554747, 3, 1, 0) + gw._s(b"t") + struct.pack("<I", 1) + struct.pack("<Q", numel) + struct.pack("<IQ", 2, 0)
        with open(bad, "wb") as f:
            f.write(head + b"\0" * ((-len(head)) % 32) + b"\0" * nbytes)
        with pytest.raises(GGUFError, match=msg):
            read_gguf(bad)


def test_the_other_legacy_and_small_k_quant_types_stay_refused():
    from realtime_codec_agent_amd import gguf
    for ttype, tname in ((6, "Q5_0"), (7, "Q5_1"), (10, "Q2_K"), (11, "Q3_K")):
        with pytest.raises(gguf.GGUFError, match=f"{tname} is not supported .*Q4_0, Q4_1"):
            gguf._nbytes(ttype, 256)
        with pytest.raises(gguf.GGUFError, match=f"{tname} is not supported .*Q4_0, Q4_1"):
            gguf._dequant(np.zeros(256, np.uint8), ttype, 256)
    assert gguf._nbytes(2, 64) == 36 and gguf._nbytes(3, 64) == 40


@pytest.mark.parametrize("name", sorted(C.FILES))
def test_the_file_cases_have_a_clear_argmax(name, tmp_path):
    """what test_lm_q40_gpu.py's argmax comparison relies on: the oracle's two largest logits are further apart than twice the tolerance"""
    path = str(tmp_path / f"{name}.gguf")
    C.write_file(name, path)
    _, want, gap = C.file_oracle(name, path)
    print(f"{name}: top-two gap {gap:.4f}, needed {C.gap_needed(want):.4f} (|logit| max {np.abs(want).max():.2f})")
    assert gap > C.gap_needed(want)
