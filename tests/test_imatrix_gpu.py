"""The importance matrix on the device: the column-sum kernel alone against its bit-exact definition (tests/imatrix_ref.py),
rca_quantize_rows_w against tests/quant_weighted_ref.py byte for byte, and the chain importance-matrix file -> quantise -> file -> load."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import imatrix_ref as IR  # noqa: E402
import quant_search_ref as R  # noqa: E402
import quant_weighted_ref as W  # noqa: E402
from oracle import lm_ref  # noqa: E402

pytestmark = pytest.mark.gpu

INIT_STD, SEED, N_CTX = 0.05, 5, 1280


def _config(ffn=512):
    from realtime_codec_agent_amd.llm import LMConfig
    return LMConfig(vocab_size=1000, hidden=256, n_layers=2, n_heads=4, n_kv_heads=2, head_dim=64, ffn=ffn)


def _new(ffn=512, **kw):
    from realtime_codec_agent_amd.llm import LlamaForAlternatingCodeChannels
    return LlamaForAlternatingCodeChannels(model_path="random:imatrix", config=_config(ffn), n_ctx=N_CTX, random_seed=SEED, init_std=INIT_STD,
                                           device=0, weight_format="bf16", **kw)


@functools.lru_cache(maxsize=None)
def _llm():
    return _new()


@functools.lru_cache(maxsize=None)
def _ids():
    ids = np.random.default_rng(77).integers(0, 1000, 165 + 1029).astype(np.int32)
    ids.setflags(write=False)
    return ids


# ------------------------------------------------------------------------------------------------------------------ the kernel alone
TAP_CASES = [(1, 1), (127, 127), (127, 5), (128, 128), (128, 127), (129, 129), (129, 128), (1024, 1024), (1024, 1019), (1024, 5)]


@pytest.mark.parametrize("K", [256, 512])
@pytest.mark.parametrize("M,m_live", TAP_CASES)
def test_tap_is_the_definition_bit_for_bit(M, m_live, K):
    """Values over a wide range (the order of the f32 sums shows), NaN planted in every dead row of both planes (a dead row read into a
    sum shows), and a second call into the same accumulator (the f64 fold order shows)."""
    rng = np.random.default_rng(1000 * M + m_live + K)
    acc = np.zeros(K, np.float64)
    want = acc.copy()
    for call in range(2):
        v = (rng.standard_normal((M, K)) * np.exp(2.0 * rng.standard_normal((M, K)))).astype(np.float32)
        xh, xl = IR.split_planes(v)
        xh[m_live:], xl[m_live:] = 0x7FC0, 0x7FC0
        acc = _llm().imatrix_rows_tap(xh, xl, m_live, acc)
        want = IR.collect(xh, xl, m_live, want)
        assert np.isfinite(acc).all() and np.array_equal(acc, want), (call, int(np.argmax(acc != want)))
    assert (acc > 0).all()


def test_tap_refuses_bad_shapes():
    from realtime_codec_agent_amd._native import RcaError
    z = np.zeros((4, 256), np.uint16)
    for m in (0, 5):
        with pytest.raises(RcaError, match="m_live"):
            _llm().imatrix_rows_tap(z, z, m, np.zeros(256))
    with pytest.raises(RcaError, match="planes of 1025 x 256"):
        _llm().imatrix_rows_tap(np.zeros((1025, 256), np.uint16), np.zeros((1025, 256), np.uint16), 3, np.zeros(256))


# ------------------------------------------------------------------------------------------------------------------ rca_quantize_rows_w
def _as_source(w, dtype):
    """(the array handed to the device, the float32 values it holds)"""
    if dtype == "f32":
        return w, w
    if dtype == "f16":
        h = w.astype(np.float16)
        return h, h.astype(np.float32)
    b = IR.f32_to_bf16(w)
    return b, IR.bf16_to_f32(b)


@pytest.mark.parametrize("dtype", ["f32", "f16", "bf16"])
@pytest.mark.parametrize("qtype", ["q4_k", "q5_k", "q6_k", "q8_0"])
def test_quantize_rows_w_is_the_numpy_definition(qtype, dtype):
    """Byte for byte on a Student-t matrix under qw = exp(randn), on the edge blocks, and on 3 x 512 with the halves of qw 1e6 apart
    (a lane indexing the weights by its block would read other columns' weights, or past them); col_weights=None is rca_quantize_rows."""
    from realtime_codec_agent_amd import quantize as Q
    rs = np.random.RandomState(31)
    mats = {"student_t4": ((rs.standard_t(4, (24, 1024)) * 0.02).astype(np.float32), np.exp(rs.randn(1024)).astype(np.float32)),
            "edges": (np.stack([R.edge_block(k) for k in R.EDGE_BLOCKS]), np.exp(rs.randn(256)).astype(np.float32)),
            "halves": ((rs.standard_t(4, (3, 512)) * 0.02).astype(np.float32), np.exp(rs.randn(512)).astype(np.float32))}
    mats["halves"][1][256:] *= np.float32(1e6)
    for name, (w, qw) in mats.items():
        src, vals = _as_source(w, dtype)
        got = Q.quantize_matrix(src, qtype, col_weights=qw, name=name)
        assert got.shape == w.shape and np.array_equal(got.raw, W.quantize_blocks_w(vals, qtype, qw)), name
        plain = Q.quantize_matrix(src, qtype, name=name)
        assert np.array_equal(plain.raw, R.quantize_blocks(vals, qtype)), name
        if name != "edges":
            assert (qtype == "q8_0") == np.array_equal(plain.raw, got.raw), name


def test_quantize_rows_w_refusals_on_the_card():
    from realtime_codec_agent_amd import quantize as Q
    from realtime_codec_agent_amd._native import RcaError
    w = np.zeros((4, 512), np.float32)
    w[2, 300] = 1e9
    with pytest.raises(RcaError, match=r"big: .*row 2: a block's d or dmin is not finite in fp16"):
        Q.quantize_matrix(w, "q4_k", col_weights=np.ones(512, np.float32), name="big")
    w[2, 300] = np.nan
    with pytest.raises(RcaError, match=r"row 2 holds a value that is not finite"):
        Q.quantize_matrix(w, "q6_k", col_weights=np.ones(512, np.float32))
    with pytest.raises(RcaError, match=r"column weights need rule 1"):
        Q.quantize_matrix(np.zeros((4, 512), np.float32), "q4_k", rule="minmax", col_weights=np.ones(512, np.float32))
    with pytest.raises(ValueError, match=r"column weights for K = 512"):
        Q.quantize_matrix(np.zeros((4, 512), np.float32), "q4_k", col_weights=np.ones(256, np.float32))


# ------------------------------------------------------------------------------------------------------------------ the chain
def _made_up_imatrix(cfg, count=1194):
    """an importance matrix as a collector would fill it (shared vectors under each of their names), from seeded values"""
    from realtime_codec_agent_amd.imatrix import Imatrix
    rs = np.random.RandomState(9)
    out = Imatrix(datasets=["made up"], chunk_count=2, chunk_size=1029)
    for l in range(cfg.n_layers):
        for kind, names in IR.NAMES.items():
            v = np.exp(rs.randn({1: cfg.n_heads * cfg.head_dim, 3: cfg.ffn}.get(kind, cfg.hidden))) * count
            for n in names:
                out[f"blk.{l}.{n}.weight"] = (v, count)
    out["output.weight"] = (np.exp(rs.randn(cfg.hidden)) * count, count)
    return out


def test_chain_file_quantise_write_load_score(tmp_path):
    """imatrix file -> quantize_weights(q4_k_m, imatrix=) on the card -> write_llama_gguf -> load -> one score with finite results; the
    file names the importance matrix.  (A random model under made-up weights: no quality claim.)"""
    from realtime_codec_agent_amd import gguf as G
    from realtime_codec_agent_amd import imatrix as I
    from realtime_codec_agent_amd import quantize as Q
    from realtime_codec_agent_amd.llm import LlamaForAlternatingCodeChannels
    cfg = _config()
    ipath = str(tmp_path / "imatrix.gguf")
    I.write_imatrix_gguf(ipath, _made_up_imatrix(cfg))
    imx = I.read_imatrix_gguf(ipath)
    src = lm_ref.random_weights(cfg, SEED, INIT_STD)
    q = Q.quantize_weights(cfg, src, "q4_k_m", imatrix=imx)
    plain = Q.quantize_weights(cfg, src, "q4_k_m")
    name = "model.layers.0.mlp.down_proj.weight"
    assert q.types[name] == plain.types[name] and not np.array_equal(q[name].raw, plain[name].raw)
    assert np.array_equal(q["model.embed_tokens.weight"].raw, plain["model.embed_tokens.weight"].raw)      # no vector: unweighted
    vec = (imx["blk.0.ffn_down.weight"][0] / imx["blk.0.ffn_down.weight"][1]).astype(np.float32)
    assert np.array_equal(q[name].raw, W.quantize_blocks_w(IR.bf16_to_f32(src[name]), q.types[name], vec))
    path = str(tmp_path / "q4_k_m.gguf")
    Q.write_llama_gguf(path, cfg, q)
    meta, _ = G.read_gguf(path)
    assert meta["quantize.imatrix.file"] == ipath and meta["quantize.imatrix.dataset"] == "made up"
    assert meta["quantize.imatrix.entries_count"] == len(imx) == 15 and meta["quantize.imatrix.chunks_count"] == 2
    llm = LlamaForAlternatingCodeChannels(model_path=path, n_ctx=512, device=0)
    try:
        r = llm.score(_ids()[:300].tolist())
        assert np.isfinite(r.logprob[:-1]).all() and np.isfinite(llm._fetch_logits()).all()
    finally:
        llm.close()
