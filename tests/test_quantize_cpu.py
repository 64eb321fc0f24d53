"""Quantising checkpoints, the parts that need no card: the numpy restatement of the search quantisers (tests/quant_search_ref.py) --
format, optimality against its own starting candidate, RMSE against this build's min / max rule, the edge blocks --, the recipe table
of realtime_codec_agent_amd.quantize, its GGUF writer against the importer (with a host quantiser in the device one's place), and the
C++ the device kernels call (csrc/rca_quant_rows.h) built for the host under AddressSanitizer / UBSan against the restatement."""
import dataclasses
import functools
import os
import sys
import warnings

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gguf_writer  # noqa: E402
import q5k_ref  # noqa: E402
import quant_search_ref as R  # noqa: E402
from oracle import lm_ref  # noqa: E402

NMAX = {"q4_k": 15, "q5_k": 31}
MATRICES = ("gaussian", "student_t4", "laplace")


@functools.lru_cache(maxsize=None)
def _matrix(name):
    """the three seeded 512 x 2048 matrices, scale 0.02, drawn in this order from one RandomState(0)"""
    rs = np.random.RandomState(0)
    mats = {"gaussian": rs.randn(512, 2048), "student_t4": rs.standard_t(4, (512, 2048)), "laplace": rs.laplace(size=(512, 2048))}
    w = (mats[name] * 0.02).astype(np.float32)
    w.setflags(write=False)
    return w


@functools.lru_cache(maxsize=None)
def _searched(name, qtype):
    return R.quantize_qk(_matrix(name), NMAX[qtype])


def _rmse(a, b):
    return float(np.sqrt(np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2)))


# ------------------------------------------------------------------------------------------------------------------ format, optimality
@pytest.mark.parametrize("qtype", ["q4_k", "q5_k"])
@pytest.mark.parametrize("name", MATRICES)
def test_search_blocks_decode_and_never_lose_to_their_starting_candidate(name, qtype):
    """Every block de-quantises to finite values under the existing de-quantisers, and for every sub-block the weighted error of the chosen
    (scale, min) -- evaluated here in float64 with the levels nearest to it -- is <= that of the starting candidate iscale = nmax / (max -
    min) (the 1e-5 allows for the f32 sums the search itself compared)."""
    w, nmax = _matrix(name), NMAX[qtype]
    p = _searched(name, qtype)
    raw = (R.q4k_ref if qtype == "q4_k" else q5k_ref).pack_blocks(p)
    assert raw.shape == (w.size // 256, R.BLOCK[qtype][1])
    deq = R.dequantize(raw, qtype)
    assert np.isfinite(deq).all()
    assert p["q"].max() <= nmax and p["sc"].max() <= 63 and p["m"].max() <= 63
    s = p["search"]
    x = w.reshape(-1, 32).astype(np.float64)
    wt = s["w"].astype(np.float64)
    mn = np.minimum(x.min(axis=1), 0.0)
    rng = x.max(axis=1) - mn
    ok = rng > 0

    def werr(scale, minimum):
        with np.errstate(all="ignore"):
            L = np.clip(np.rint((x - minimum[:, None]) / np.where(scale > 0, scale, 1.0)[:, None]), 0, nmax)
        return (wt * (scale[:, None] * L + minimum[:, None] - x) ** 2).sum(axis=1)

    start = werr(np.where(ok, rng / nmax, 0.0), mn)
    chosen = werr(s["scale"].astype(np.float64), -s["the_min"].astype(np.float64))
    assert (chosen[ok] <= start[ok] * (1 + 1e-5)).all()
    assert (s["best_err"] <= s["start_err"]).all()
    better = float((s["best_err"] < s["start_err"]).mean())
    print(f"{name} {qtype}: {100 * better:.1f}% of {len(x)} sub-blocks found a candidate strictly better than the start")
    assert better > 0.5


@pytest.mark.parametrize("qtype", ["q6_k", "q8_0"])
def test_q6_k_and_q8_0_blocks_decode_under_the_existing_dequantisers(qtype):
    from realtime_codec_agent_amd import _native as N
    w = _matrix("student_t4")[:64]
    raw = R.quantize_blocks(w, qtype)
    assert raw.shape == (64, 2048 // R.BLOCK[qtype][0] * R.BLOCK[qtype][1])
    deq = R.dequantize(raw, qtype).reshape(w.shape)
    assert np.isfinite(deq).all()
    cls = N.Q6KBlocks if qtype == "q6_k" else N.Q8Blocks
    assert np.array_equal(cls(raw, w.shape).dequantize(), deq)
    if qtype == "q6_k":
        a, b = _rmse(deq, w), _rmse(R.dequantize(R.minmax_blocks(w, qtype), qtype).reshape(w.shape), w)
        print(f"Q6_K student_t4 64 x 2048: min/max RMSE {b:.4e}, search RMSE {a:.4e}, ratio {a / b:.3f}")
        assert a < b


# ------------------------------------------------------------------------------------------------------------------ RMSE
@pytest.mark.parametrize("qtype", ["q4_k", "q5_k"])
@pytest.mark.parametrize("name", MATRICES)
def test_search_rmse_is_below_the_min_max_rule(name, qtype):
    """search RMSE / min-max RMSE < 1.0 on the three seeded matrices (DESIGN.md quotes the printed figures)."""
    w = _matrix(name)
    pack = (R.q4k_ref if qtype == "q4_k" else q5k_ref).pack_blocks
    got = R.dequantize(pack(_searched(name, qtype)), qtype).reshape(w.shape)
    base = R.dequantize(R.minmax_blocks(w, qtype), qtype).reshape(w.shape)
    a, b = _rmse(got, w), _rmse(base, w)
    rows = np.sqrt(((got - w) ** 2).mean(axis=1)) / np.sqrt(((base - w) ** 2).mean(axis=1))
    print(f"{qtype} {name}: min/max RMSE {b:.4e}, search RMSE {a:.4e}, search / min/max {a / b:.4f}, worst row ratio {rows.max():.4f}")
    assert a / b < 1.0


# ------------------------------------------------------------------------------------------------------------------ edge blocks
@pytest.mark.parametrize("qtype", ["q4_k", "q5_k", "q6_k", "q8_0"])
@pytest.mark.parametrize("kind", R.EDGE_BLOCKS)
def test_edge_blocks_are_handled_as_defined(kind, qtype):
    """Finite values out, none further from its source than the block's own range (amax for the symmetric types); and what the rules
    define exactly: an all-zero block is all-zero bytes; a constant negative Q4_K / Q5_K block has scale 0, every level 0 and the value in
    the minimum (m = 63, dmin = fp16(c / 63)); a constant positive one is its top level within fp16's rounding of d."""
    x = R.edge_block(kind)
    raw = R.quantize_blocks(x[None], qtype)
    deq = R.dequantize(raw, qtype)
    assert np.isfinite(deq).all()
    span = float(max(x.max(), 0.0) - min(x.min(), 0.0)) if qtype in NMAX else float(np.abs(x).max())   # the levels' range includes 0
    assert np.abs(deq - x).max() <= span
    if kind == "zero":
        assert not raw.any()
    if kind in ("const_pos", "const_neg"):
        assert np.abs(deq - x).max() <= 0.375 * (2.0 ** -9 if qtype in NMAX else 1 / 31)
    if kind == "const_neg" and qtype in NMAX:
        p = R.quantize_qk(x[None], NMAX[qtype])
        assert not p["q"].any() and not p["sc"].any() and (p["m"] == 63).all() and p["d"][0, 0] == 0
        assert p["dmin"][0, 0] == np.float16(np.float32(0.375) / np.float32(63))
    if kind == "outlier":
        assert abs(deq[77] - 1e4) <= 1e4 / 15
    if kind == "amax_65504":
        assert abs(deq[5] - 65504.0) <= 65504.0 * 2 / 15 and deq[200] < -50000.0


@pytest.mark.parametrize("qtype", ["q4_k", "q5_k", "q6_k", "q8_0"])
def test_values_no_fp16_scale_can_hold_and_nan_are_refused_by_name(qtype):
    w = np.zeros((3, 256), np.float32)
    w[2, 9] = 1e9
    with pytest.raises(R.QuantError, match=r"blk\.0\.ffn_up\.weight: row 2.*not finite in fp16"):
        R.quantize_blocks(w, qtype, name="blk.0.ffn_up.weight")
    w[2, 9] = 1.0
    w[1, 255] = np.nan
    with pytest.raises(R.QuantError, match=r"blk\.0\.ffn_up\.weight: row 1 holds a value that is not finite"):
        R.quantize_blocks(w, qtype, name="blk.0.ffn_up.weight")


# ------------------------------------------------------------------------------------------------------------------ recipe
MORE_BITS = {2: [1], 8: [0, 3, 6, 7], 16: [0, 1, 4, 7, 10, 13, 14, 15], 28: [0, 1, 2, 5, 8, 11, 14, 17, 20, 23, 24, 25, 26, 27]}


@pytest.mark.parametrize("n", sorted(MORE_BITS))
def test_use_more_bits_is_the_hand_written_list(n):
    from realtime_codec_agent_amd import quantize as Q
    assert [i for i in range(n) if Q.use_more_bits(i, n)] == MORE_BITS[n]
    assert [i for i in range(n) if R.use_more_bits(i, n)] == MORE_BITS[n]


def test_recipe_tables_equal_the_test_writers():
    """q4_k_m of an 8-layer model, tensor for tensor, is gguf_writer.q4_k_m_type (what its "Q4_K_M" files hold); q5_k_m is q5k_ref's."""
    from realtime_codec_agent_amd import quantize as Q
    from realtime_codec_agent_amd.llm import LMConfig, lm_tensor_names
    cfg = LMConfig(vocab_size=1024, hidden=256, n_layers=8, n_heads=4, n_kv_heads=2, head_dim=64, ffn=512)
    ggml = {gguf_writer.Q4_K: "q4_k", gguf_writer.Q6_K: "q6_k", q5k_ref.Q5_K: "q5_k"}
    seen = set()
    for hf in lm_tensor_names(cfg):
        if "norm" in hf:
            continue
        g = Q.gguf_name(hf)
        assert Q.recipe_type(g, 8, "q4_k_m") == R.recipe_type(g, 8, "q4_k_m") == ggml[gguf_writer.q4_k_m_type(g, 8)]
        assert Q.recipe_type(g, 8, "q5_k_m") == R.recipe_type(g, 8, "q5_k_m") == ggml[q5k_ref.q5_k_m_type(g, 8)]
        for one in ("q8_0", "q4_k", "q5_k", "q6_k"):
            assert Q.recipe_type(g, 8, one) == one
        seen.add((g.split(".")[-2], Q.recipe_type(g, 8, "q4_k_m")))
    assert ("attn_v", "q6_k") in seen and ("attn_v", "q4_k") in seen and ("ffn_down", "q6_k") in seen and ("output", "q6_k") in seen
    assert ("token_embd", "q4_k") in seen and ("attn_q", "q6_k") not in seen


# ------------------------------------------------------------------------------------------------------------------ writer and loader
def _host_quantize_matrix(w, type, rule="search", device=0, name="tensor"):
    """quantize.quantize_matrix with the restatement in the device's place"""
    from realtime_codec_agent_amd import quantize as Q
    w = np.asarray(w)
    f = (w.astype(np.uint32) << 16).view(np.float32) if w.dtype == np.uint16 else w.astype(np.float32)
    raw = R.quantize_blocks(f, type, name) if rule == "search" else R.minmax_blocks(f, type)
    return Q.TYPES[type][1](raw, f.shape)


def _config(n_layers=2, **kw):
    from realtime_codec_agent_amd.llm import LMConfig
    return LMConfig(vocab_size=512, hidden=256, n_layers=n_layers, n_heads=4, n_kv_heads=2, head_dim=64, ffn=512, rope_theta=10000.0,
                    rms_eps=float(np.float32(1e-5)), **{"rope_scaling": None, **kw})      # a GGUF keeps rms_eps as an f32


@functools.lru_cache(maxsize=None)
def _quantised_model(recipe):
    from realtime_codec_agent_amd import quantize as Q
    cfg = _config()
    src = lm_ref.random_weights(cfg, 3, 0.05)                       # bf16 bits, as a checkpoint supplies them
    return cfg, src, Q.quantize_weights(cfg, src, recipe, quantize_matrix=_host_quantize_matrix)


@pytest.mark.parametrize("recipe", ["q4_k_m", "q5_k_m", "q8_0"])
def test_written_files_load_back_to_the_same_model(recipe, tmp_path):
    """write_llama_gguf then gguf.load_llama_gguf: the same config, HF names, the same block bytes per tensor (q_proj / k_proj rows back in
    HF order: the file holds them permuted), the embedding table as its blocks' values, rope.inv_freq and the metadata passed through."""
    from realtime_codec_agent_amd import gguf as G
    from realtime_codec_agent_amd import quantize as Q
    from realtime_codec_agent_amd.llm import rope_inv_freq
    cfg, src, q = _quantised_model(recipe)
    assert q.recipe == recipe and set(q) == set(src)
    meta = {"general.name": "tiny", "tokenizer.ggml.model": "gpt2", "tokenizer.ggml.tokens": [f"<{i}>" for i in range(cfg.vocab_size)],
            "tokenizer.ggml.token_type": np.arange(cfg.vocab_size, dtype=np.int32) % 3, "tokenizer.ggml.bos_token_id": 7,
            "tokenizer.ggml.scores": np.linspace(-1, 0, cfg.vocab_size).astype(np.float32), "custom.ratio": 0.25, "custom.flag": True,
            "llama.block_count": 99, "gguf.version": 2}
    path = str(tmp_path / f"{recipe}.gguf")
    n = Q.write_llama_gguf(path, cfg, q, meta=meta)
    assert n == os.path.getsize(path)
    cfg2, w2, meta2 = G.load_llama_gguf(path)
    assert cfg2 == cfg
    assert set(w2) == set(q) | {"rope.inv_freq"}
    for k, v in q.items():
        if k == "model.embed_tokens.weight":
            assert w2[k].dtype == np.float32 and np.array_equal(w2[k], v.dequantize())
        elif hasattr(v, "raw"):
            assert type(w2[k]) is type(v) and w2[k].shape == v.shape and np.array_equal(w2[k].raw, v.raw), k
            assert q.types[k] == R.recipe_type(Q.gguf_name(k), cfg.n_layers, recipe)
        else:
            assert w2[k].dtype == np.float32 and np.array_equal(w2[k], Q._to_f32(v)), k
    assert np.array_equal(w2["rope.inv_freq"], rope_inv_freq(cfg))
    assert meta2["general.file_type"] == {"q8_0": 7, "q4_k_m": 15, "q5_k_m": 17}[recipe] and meta2["gguf.version"] == 3
    assert meta2["llama.block_count"] == cfg.n_layers and meta2["general.architecture"] == "llama"
    for k in ("general.name", "tokenizer.ggml.model", "tokenizer.ggml.tokens", "tokenizer.ggml.bos_token_id", "custom.flag"):
        assert meta2[k] == meta[k], k
    assert meta2["custom.ratio"] == 0.25
    for k in ("tokenizer.ggml.token_type", "tokenizer.ggml.scores"):
        assert meta2[k].dtype == meta[k].dtype and np.array_equal(meta2[k], meta[k])
    # the file itself holds q_proj / k_proj as convert_hf_to_gguf.py permutes them
    _, raw = G.read_gguf(path, keep_q8_0=True)
    for gg, hf, nh in (("attn_q", "q_proj", cfg.n_heads), ("attn_k", "k_proj", cfg.n_kv_heads)):
        hfm = q[f"model.layers.1.self_attn.{hf}.weight"]
        assert np.array_equal(raw[f"blk.1.{gg}.weight"].dequantize(), gguf_writer.permute(hfm.dequantize(), nh))
    assert "rope_freqs.weight" not in raw


def test_llama3_rope_scaling_survives_the_file_within_an_ulp(tmp_path):
    """The format keeps llama3 scaling as f32 divisors of the plain frequencies (rope_freqs.weight) and a reader forms f32(base / f): where
    one f32 step of f moves that quotient by more than an ulp, some frequencies have no exact divisor, so the bound is one ulp (2^-23
    relative), and the writer's choice hits most of them exactly."""
    from realtime_codec_agent_amd import gguf as G
    from realtime_codec_agent_amd import quantize as Q
    from realtime_codec_agent_amd.llm import rope_inv_freq
    cfg, _, q = _quantised_model("q8_0")
    cfg3 = dataclasses.replace(cfg, rope_scaling="llama3", rope_theta=500000.0)
    path = str(tmp_path / "l3.gguf")
    Q.write_llama_gguf(path, cfg3, q)
    cfg2, w2, _ = G.load_llama_gguf(path)
    assert cfg2 == dataclasses.replace(cfg3, rope_scaling=None)       # the importer returns the scaling as frequencies, not as settings
    got, want = w2["rope.inv_freq"], rope_inv_freq(cfg3)
    assert (np.abs(got.astype(np.float64) - want) <= 2.0 ** -23 * want).all() and (got == want).mean() >= 0.9
    assert not np.allclose(got, rope_inv_freq(cfg2), rtol=1e-3)


def test_matrices_no_k_quant_can_hold_stay_f16_and_quantised_sources_are_refused():
    from realtime_codec_agent_amd import quantize as Q
    from realtime_codec_agent_amd._native import Q8Blocks
    cfg = _config(n_layers=0)
    rs = np.random.RandomState(1)
    src = {"model.embed_tokens.weight": rs.randn(8, 264).astype(np.float32), "model.norm.weight": np.ones(264, np.float32),
           "lm_head.weight": rs.randn(6, 256).astype(np.float32)}
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        q = Q.quantize_weights(cfg, src, "q4_k_m", quantize_matrix=_host_quantize_matrix)
    said = sorted(str(r.message).split(" ")[0] for r in rec)
    assert said == ["lm_head.weight", "model.embed_tokens.weight"]                # K = 264, and N = 6
    assert q["model.embed_tokens.weight"].dtype == np.float16 and q["lm_head.weight"].dtype == np.float16 and q.types["lm_head.weight"] == "f16"
    src["lm_head.weight"] = Q8Blocks(np.zeros((8, 8 * 34), np.uint8), (8, 256))
    with pytest.raises(ValueError, match="lm_head.weight is already quantised"), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        Q.quantize_weights(cfg, src, "q4_k", quantize_matrix=_host_quantize_matrix)
    with pytest.raises(ValueError, match="recipe 'q3_k'"):
        Q.quantize_weights(cfg, src, "q3_k")
    src["lm_head.weight"] = rs.randn(8, 256).astype(np.float32)
    src["model.embed_codec_tokens.codec_embed.weight"] = np.zeros((4, 16), np.float32)      # saved before persist_codec_embeddings
    with pytest.raises(ValueError, match="persist the codec embeddings"):
        Q.quantize_weights(cfg, src, "q8_0", quantize_matrix=_host_quantize_matrix)


# ------------------------------------------------------------------------------------------------------------------ the kernels' C++ on the host
RCA_TYPE = {"q8_0": 2, "q4_k": 4, "q5_k": 6, "q6_k": 5}


@functools.lru_cache(maxsize=None)
def _host_program():
    """tests/quant_rows_host.cpp over csrc/rca_quant_rows.h, built by ROCm's clang with AddressSanitizer and UBSan (host code only)"""
    import shutil
    import subprocess
    import tempfile
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    cands = [os.path.join(os.path.dirname(os.path.realpath(hipcc)), "..", "llvm", "bin", "clang++"), "/opt/rocm/llvm/bin/clang++",
             shutil.which("clang++") or ""]
    clang = next((c for c in cands if c and os.path.exists(c)), None)
    assert clang, "no clang++ next to hipcc: the host build of csrc/rca_quant_rows.h needs the compiler that has _Float16"
    out = os.path.join(tempfile.mkdtemp(prefix="quant_rows_host_"), "quant_rows_host")
    cmd = [clang, "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-I", os.path.join(root, "realtime_codec_agent_amd", "csrc"), os.path.join(root, "tests", "quant_rows_host.cpp"), "-o", out]
    p = subprocess.run(cmd, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    return out


def _host_run(w, qtype, rule, tmp_path):
    import subprocess
    src, dst = str(tmp_path / "in.f32"), str(tmp_path / "out.bin")
    np.ascontiguousarray(w, np.float32).tofile(src)
    p = subprocess.run([_host_program(), str(RCA_TYPE[qtype]), str(rule), str(w.shape[0]), str(w.shape[1]), src, dst], capture_output=True, text=True)
    assert p.returncode == 0, p.stdout + p.stderr            # a sanitizer report ends the program with another status
    words = p.stdout.split()
    return np.fromfile(dst, np.uint8).reshape(w.shape[0], -1), int(words[1]), int(words[3]), int(words[5])


@pytest.mark.parametrize("qtype", ["q4_k", "q5_k", "q6_k", "q8_0"])
def test_the_kernels_cxx_on_the_host_is_the_restatement_and_clean_under_sanitizers(qtype, tmp_path):
    """The functions the device kernels call (csrc/rca_quant_rows.h) compiled for the host: the same bytes as the numpy restatement on
    seeded matrices and on every edge block (rule 1), the bytes of the min / max oracles (rule 0), the status bits and rows for inf, NaN
    and a value no fp16 d can hold -- under AddressSanitizer and UBSan, with an output buffer of exactly the blocks' size."""
    rs = np.random.RandomState(11)
    mats = {"gaussian": (rs.randn(8, 512) * 0.02).astype(np.float32), "student_t4": (rs.standard_t(4, (8, 512)) * 0.02).astype(np.float32),
            "edges": np.stack([R.edge_block(k) for k in R.EDGE_BLOCKS])}
    for name, w in mats.items():
        got, status, _, _ = _host_run(w, qtype, 1, tmp_path)
        assert status == 0 and np.array_equal(got, R.quantize_blocks(w, qtype)), name
        if name != "edges":
            got, status, _, _ = _host_run(w, qtype, 0, tmp_path)
            assert status == 0 and np.array_equal(got, R.minmax_blocks(w, qtype)), name
    w = mats["gaussian"].copy()
    w[5, 300], w[6, 1] = np.inf, np.nan
    for rule in (0, 1):
        _, status, bad_in, _ = _host_run(w, qtype, rule, tmp_path)
        assert status & 1 and bad_in == 5
    w = mats["gaussian"].copy()
    w[3, 17] = 1e9
    _, status, bad_in, bad_d = _host_run(w, qtype, 1, tmp_path)
    assert status == 2 and bad_in == -1 and bad_d == 3
