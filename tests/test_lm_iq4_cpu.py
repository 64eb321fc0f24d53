"""GGUF IQ4_NL / IQ4_XS on the host: the block layouts restated in tests/iq4_ref.py and _native.IQ4NLBlocks / IQ4XSBlocks on hand-made
blocks, the importer (IQ4_NL-only and IQ4_XS-only files and the mix of IQ4_XS, Q5_K and Q6_K tensors a llama-quantize IQ4_XS file holds),
and the numpy statement of the load-time IQ4_NL rule that test_lm_iq4_gpu.py ties the device to."""
import os
import struct
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import iq4_ref  # noqa: E402
import lm_iq4_cases as C  # noqa: E402

F32 = np.float32
KV = [-127, -104, -83, -65, -49, -35, -22, -10, 1, 13, 25, 38, 53, 69, 89, 113]


def test_the_table_is_the_published_one():
    from realtime_codec_agent_amd import _native
    assert iq4_ref.KV.tolist() == KV and _native.KVALUES_IQ4NL.tolist() == KV and _native.KVALUES_IQ4NL.dtype == np.int8
    assert (_native.RCA_IQ4_NL, _native.RCA_IQ4_XS) == (9, 10)
    assert _native.IQ4NLBlocks.BLOCK_BYTES == 18 and _native.IQ4XSBlocks.BLOCK_BYTES == 136


def test_iq4_nl_blocks_round_trip_and_dequantise_by_the_formula_bit_for_bit():
    """random raw blocks: _native's class, iq4_ref.dequantize_blocks, the QMat the GPU tests use and a per-weight loop over the bit rules
    agree bit for bit; pack is unpack's inverse"""
    rng = np.random.default_rng(3)
    nb = 48
    raw = rng.integers(0, 256, (nb, 18), dtype=np.uint8)
    raw[:, 0:2] = (rng.uniform(1e-4, 2e-3, (nb, 1)) * rng.choice([-1, 1], (nb, 1))).astype(np.float16).view(np.uint8)
    want = np.empty((nb, 32), F32)
    for b, blk in enumerate(raw):
        d = F32(blk[0:2].copy().view(np.float16)[0])
        for j in range(32):
            q = (int(blk[2 + j]) & 0xF) if j < 16 else (int(blk[2 + j - 16]) >> 4)
            want[b, j] = F32(d * F32(KV[q]))
    blocks = iq4_ref.block_class(iq4_ref.IQ4_NL)(raw, (nb // 8, 256))
    assert blocks.raw.shape == (nb // 8, 8 * 18)
    assert np.array_equal(blocks.dequantize().reshape(nb, 32), want)
    assert np.array_equal(iq4_ref.dequantize_blocks(raw, iq4_ref.IQ4_NL).reshape(nb, 32), want)
    assert np.array_equal(iq4_ref.qmat(blocks).dequantize().reshape(nb, 32), want)
    q, d, ls = iq4_ref.unpack(raw, iq4_ref.IQ4_NL)
    assert q.max() == 15 and q.min() == 0 and np.all(ls == 33)
    assert np.array_equal(iq4_ref.pack_iq4_nl(dict(q=q, d=d.astype(np.float16))), raw)
    assert np.array_equal(blocks.take_rows([2, 0]).dequantize(), blocks.dequantize()[[2, 0]]) and type(blocks.take_rows([1])) is type(blocks)


def test_iq4_xs_blocks_with_every_scale_code_round_trip_exactly():
    """C.xs_scale_blocks: all 64 scale codes, both nibble positions of scales_l, every bit pair of scales_h with all four values.  Packing
    then unpacking returns (q, d, ls); the de-quantisation equals d * (ls - 32) * kv written out directly, in float64 too (the float32
    products are exact)."""
    raw, q, d, ls = C.xs_scale_blocks(16)
    nb = raw.shape[0]
    assert set(ls.reshape(-1).tolist()) == set(range(64))
    for ib in range(8):
        assert set((ls[:, ib] >> 4).tolist()) == {0, 1, 2, 3} and len(set((ls[:, ib] & 15).tolist())) >= 2
    assert {0, 31, 32, 63} <= set(ls.reshape(-1).tolist())
    q2, d2, ls2 = iq4_ref.unpack(raw, iq4_ref.IQ4_XS)
    assert np.array_equal(q2.reshape(nb, 256), q) and np.array_equal(ls2.reshape(nb, 8), ls) and np.array_equal(d2.reshape(nb, 8)[:, 0], d.astype(F32))
    assert np.array_equal(iq4_ref.pack_iq4_xs(dict(q=q2, d=d, ls=ls2)), raw)
    want = np.empty((nb, 256), F32)
    want64 = np.empty((nb, 256))
    for b in range(nb):
        blk = raw[b]
        dd = F32(blk[0:2].copy().view(np.float16)[0])
        sh = int(blk[2]) | (int(blk[3]) << 8)
        for ib in range(8):
            l = ((int(blk[4 + ib // 2]) >> (4 * (ib % 2))) & 15) | (((sh >> (2 * ib)) & 3) << 4)
            assert l == ls[b, ib]
            dl = F32(dd * F32(l - 32))
            for j in range(32):
                byte = int(blk[8 + 16 * ib + (j & 15)])
                n = (byte & 15) if j < 16 else (byte >> 4)
                want[b, 32 * ib + j] = F32(dl * F32(KV[n]))
                want64[b, 32 * ib + j] = float(dd) * (l - 32) * KV[n]
    assert np.array_equal(want.astype(np.float64), want64)                                # one exact f32 value per weight
    blocks = iq4_ref.block_class(iq4_ref.IQ4_XS)(raw, (nb // 2, 512))
    assert blocks.raw.shape == (nb // 2, 2 * 136) and np.array_equal(blocks.scales(), ls)
    assert np.array_equal(blocks.dequantize().reshape(nb, 256), want)
    assert np.array_equal(iq4_ref.dequantize_blocks(raw, iq4_ref.IQ4_XS).reshape(nb, 256), want)
    assert np.array_equal(iq4_ref.qmat(blocks).dequantize().reshape(nb, 256), want)
    assert np.array_equal(blocks.take_rows([3, 1]).dequantize(), blocks.dequantize()[[3, 1]]) and type(blocks.take_rows([1])) is type(blocks)


def test_the_two_types_hold_the_same_values_when_every_scale_is_one():
    """the fixture of test_lm_iq4_gpu.py's one-form test"""
    a, b = iq4_ref.twin_matrix(np.random.default_rng(8), 12, 512)
    assert type(a).__name__ == "IQ4NLBlocks" and type(b).__name__ == "IQ4XSBlocks" and np.all(b.scales() == 33)
    assert np.array_equal(a.dequantize(), b.dequantize()) and np.abs(a.dequantize()).max() > 0
    qa, qb = iq4_ref.qmat(a), iq4_ref.qmat(b)
    assert np.array_equal(qa.q, qb.q) and np.array_equal(qa.s, qb.s) and (qa.s > 0).any() and (qa.s < 0).any()


def test_the_numpy_quantiser_hand_cases():
    """largest magnitude negative (d > 0) and positive (d < 0), a +v / -v tie (the first wins), an all-zero block, a block too small for fp16"""
    x = np.zeros((6, 32), F32)
    x[0] = np.linspace(-1.27, 1.0, 32)              # largest magnitude -1.27: d = 0.01 > 0
    x[1] = np.linspace(-1.0, 1.27, 32)              # largest magnitude +1.27: d = -0.01 < 0
    x[2, 3], x[2, 9] = 0.5, -0.5                    # tie: +0.5 comes first, d < 0
    x[3, 3], x[3, 9] = -0.5, 0.5                    # tie: -0.5 comes first, d > 0
    x[5] = 1e-10                                    # max / -127 rounds to -0 in fp16
    p = iq4_ref.quantize_iq4_nl(x)
    d = p["d"].astype(F32).reshape(-1)
    assert d[0] == F32(np.float16(F32(-1.27) / F32(-127.0))) > 0 and d[1] == -d[0]
    assert d[2] < 0 < d[3] and d[4] == 0 and d[5] == 0
    assert p["q"][0, 0] == 0 and p["q"][1, 31] == 0            # the extreme value itself maps to index 0: kv = -127
    assert p["q"][2, 3] == 0 and p["q"][2, 9] == 15            # d < 0: +0.5 = d * -127, -0.5 is nearest d * 113
    assert p["q"][3, 3] == 0 and p["q"][3, 9] == 15
    assert np.all(p["q"][4] == 8) and np.all(p["q"][5] == 8)
    got = iq4_ref.fake_quant(x)
    assert np.all(got[4] == 0) and np.all(got[5] == 0)


def test_the_numpy_quantiser_is_idempotent_and_picks_the_nearest_table_entry():
    rng = np.random.default_rng(4)
    w = (rng.standard_normal((16, 768)) * 0.05).astype(F32)
    w[3, 64:96] = 0
    p = iq4_ref.quantize_iq4_nl(w)
    assert p["q"].max() == 15 and p["q"].min() == 0 and np.all(p["q"][3, 64:96] == 8)
    d = p["d"].astype(np.float64).repeat(32, axis=1)
    cand = d[:, :, None] * np.array(KV, np.float64)[None, None, :]                       # exact
    dist = np.abs(w.astype(np.float64)[:, :, None] - cand)
    chosen = np.take_along_axis(dist, p["q"].astype(np.int64)[:, :, None], axis=2)[:, :, 0]
    # the nearest entry, up to the float32 rounding of the subtraction the rule is stated in (half an ulp of the larger operand)
    slack = 2.0 ** -24 * (np.abs(w) + np.abs(cand).max(axis=2))
    assert np.all(chosen <= dist.min(axis=2) + slack)
    # how far that can be: |x| <= |max| <= 127 |d| (1 + 2^-11) (fp16 rounding of d), and the entries span -127 d .. 113 d: inside the span
    # half the widest gap (-127 .. -104: 11.5 steps), past the 113 end (a value of the sign opposite to max) 14 steps + the rounding of d
    assert np.all(chosen <= (14 + 127 * 2.0 ** -11) * np.abs(d) + slack)
    # idempotent: the de-quantised values quantise to themselves (same d, same values)
    v = iq4_ref.fake_quant(w)
    p2 = iq4_ref.quantize_iq4_nl(v)
    assert np.array_equal(p2["d"], p["d"]) and np.array_equal(iq4_ref.fake_quant(v), v)
    nz = (p["d"].astype(F32) != 0).repeat(32, axis=1)
    assert np.array_equal(p2["q"][nz], p["q"][nz])
    # bf16 bit patterns are taken as the device takes them
    bits = (w.view(np.uint32) >> 16).astype(np.uint16)
    assert np.array_equal(iq4_ref.quantize_iq4_nl(bits)["q"], iq4_ref.quantize_iq4_nl((bits.astype(np.uint32) << 16).view(F32))["q"])


def test_gguf_round_trip_of_the_three_files(tmp_path):
    from realtime_codec_agent_amd._native import IQ4NLBlocks, IQ4XSBlocks, Q5KBlocks, Q6KBlocks
    from realtime_codec_agent_amd.gguf import GGUFError, load_llama_gguf, read_gguf
    for name, cls, ttype in (("iq4_nl", IQ4NLBlocks, iq4_ref.IQ4_NL), ("iq4_xs", IQ4XSBlocks, iq4_ref.IQ4_XS)):
        path = str(tmp_path / f"{name}.gguf")
        cfg = C.write_file(name, path)
        wf = C.f32_weights(cfg, C.FILES[name][2])
        cfg2, file_w, _ = load_llama_gguf(path)
        assert cfg2.hidden == cfg.hidden and cfg2.n_layers == 2
        for k in ("self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj", "mlp.down_proj"):
            t = file_w[f"model.layers.1.{k}.weight"]
            assert type(t) is cls and t.raw.shape[1] == t.shape[1] // iq4_ref.BLOCK_VALUES[ttype] * iq4_ref.BLOCK_BYTES[ttype]
            src = wf[f"model.layers.1.{k}.weight"]
            if ttype == iq4_ref.IQ4_NL:
                # rows come back in Hugging Face order: equal to quantising the un-permuted source (a block never crosses a row)
                assert np.array_equal(t.dequantize(), iq4_ref.fake_quant(src)), k
            else:
                assert len(np.unique(t.scales())) > 8 and np.abs(t.dequantize() - src).max() < 0.25 * np.abs(src).max(), k
        assert type(file_w["lm_head.weight"]) is cls
        emb = file_w["model.embed_tokens.weight"]
        assert emb.dtype == np.float32 and emb.shape == (1024, 256)
        if ttype == iq4_ref.IQ4_NL:
            assert np.array_equal(emb, iq4_ref.fake_quant(wf["model.embed_tokens.weight"]))
    mix = str(tmp_path / "mix.gguf")
    C.write_file("iq4_xs_mix", mix)
    _, fw, _ = load_llama_gguf(mix)
    assert type(fw["lm_head.weight"]) is Q6KBlocks
    assert type(fw["model.layers.0.mlp.down_proj.weight"]) is Q5KBlocks and type(fw["model.layers.1.mlp.down_proj.weight"]) is IQ4XSBlocks
    assert all(type(fw[f"model.layers.{l}.self_attn.v_proj.weight"]) is Q5KBlocks for l in range(2))
    assert all(type(fw[f"model.layers.{l}.{k}.weight"]) is IQ4XSBlocks for l in range(2)
               for k in ("self_attn.q_proj", "self_attn.k_proj", "self_attn.o_proj", "mlp.gate_proj", "mlp.up_proj"))
    # tensors whose size is no multiple of the block, and one whose data the file does not hold
    import gguf_writer as gw
    for ttype, numel, nbytes, msg in ((20, 300, 352, "IQ4_NL tensor whose size is not a multiple of 32"),
                                      (23, 384, 352, "IQ4_XS tensor whose size is not a multiple of 256"),
                                      (23, 512, 2 * 136 - 4, "tensor 't' runs past the end of the file")):
        bad = str(tmp_path / f"bad{ttype}_{numel}.gguf")
        head = struct.pack("<IIQQ", 0x46554747, 3, 1, 0) + gw._s(b"t") + struct.pack("<I", 1) + struct.pack("<Q", numel) + struct.pack("<IQ", ttype, 0)
        with open(bad, "wb") as f:
            f.write(head + b"\0" * ((-len(head)) % 32) + b"\0" * nbytes)
        with pytest.raises(GGUFError, match=msg):
            read_gguf(bad)


def test_sizes_and_the_names_of_the_grid_types_that_stay_refused():
    from realtime_codec_agent_amd import gguf
    assert gguf._nbytes(20, 64) == 36 and gguf._nbytes(23, 256) == 136 and gguf._nbytes(23, 512) == 272
    with pytest.raises(gguf.GGUFError, match="IQ4_NL tensor whose size is not a multiple of 32"):
        gguf._nbytes(20, 48)
    with pytest.raises(gguf.GGUFError, match="IQ4_XS tensor whose size is not a multiple of 256"):
        gguf._nbytes(23, 128)
    for ttype, tname in ((16, "IQ2_XXS"), (17, "IQ2_XS"), (18, "IQ3_XXS"), (19, "IQ1_S"), (21, "IQ3_S"), (22, "IQ2_S")):
        with pytest.raises(gguf.GGUFError, match=f"tensor type {tname} is not supported .*Q4_0, Q4_1.*IQ4_NL, IQ4_XS are"):
            gguf._nbytes(ttype, 256)
        with pytest.raises(gguf.GGUFError, match=f"tensor type {tname} is not supported .*Q4_0, Q4_1.*IQ4_NL, IQ4_XS are"):
            gguf._dequant(np.zeros(256, np.uint8), ttype, 256)
    raw, _, _, _ = C.xs_scale_blocks(8)
    assert np.array_equal(gguf._dequant(raw.reshape(-1), 23, 8 * 256), iq4_ref.dequantize_blocks(raw, iq4_ref.IQ4_XS))


def test_weight_format_iq4_nl_is_a_known_name():
    """the constructor refuses unknown names before it touches the library, and names iq4_nl among the known ones"""
    from realtime_codec_agent_amd.llm import LlamaForAlternatingCodeChannels
    with pytest.raises(ValueError, match="'iq4_nl'"):
        LlamaForAlternatingCodeChannels(model_path="random:x", weight_format="iq4_xs")


@pytest.mark.parametrize("name", sorted(C.FILES))
def test_the_file_cases_have_a_clear_argmax(name, tmp_path):
    """what test_lm_iq4_gpu.py's argmax comparison relies on: the oracle's two largest logits are further apart than twice the tolerance
    at the compared position of every file (3 of 3 rows qualify)"""
    path = str(tmp_path / f"{name}.gguf")
    C.write_file(name, path)
    _, want, gap = C.file_oracle(name, path)
    print(f"{name}: top-two gap {gap:.4f}, needed {C.gap_needed(want):.4f} (|logit| max {np.abs(want).max():.2f})")
    assert gap > C.gap_needed(want)
