"""The importance matrix off the card: the GGUF imatrix file (write -> read, merge), the vector each matrix gets in
quantize_weights(imatrix=...) with a host quantiser in the device one's place, and the command line's argument errors."""
import os
import sys
import warnings

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import quant_search_ref as R  # noqa: E402
import quant_weighted_ref as W  # noqa: E402
from oracle import lm_ref  # noqa: E402


def _config(n_layers=2):
    from realtime_codec_agent_amd.llm import LMConfig
    return LMConfig(vocab_size=512, hidden=256, n_layers=n_layers, n_heads=4, n_kv_heads=2, head_dim=64, ffn=512, rope_theta=10000.0,
                    rms_eps=float(np.float32(1e-5)), rope_scaling=None)


def _imatrix(cfg, seed=0, count=1194):
    """an importance matrix with the shared vectors under each of their names"""
    from realtime_codec_agent_amd.imatrix import Imatrix
    rs = np.random.RandomState(seed)
    out = Imatrix(datasets=["corpus-a"], chunk_count=3, chunk_size=512)
    for l in range(cfg.n_layers):
        for names, K in ((("attn_q", "attn_k", "attn_v"), cfg.hidden), (("attn_output",), cfg.n_heads * cfg.head_dim),
                         (("ffn_gate", "ffn_up"), cfg.hidden), (("ffn_down",), cfg.ffn)):
            v = np.exp(rs.randn(K)) * count
            for nm in names:
                out[f"blk.{l}.{nm}.weight"] = (v, count)
    out["output.weight"] = (np.exp(rs.randn(cfg.hidden)) * count, count)
    return out


def test_file_round_trip_is_exact_in_f32(tmp_path):
    from realtime_codec_agent_amd import gguf as G
    from realtime_codec_agent_amd import imatrix as I
    imx = _imatrix(_config())
    path = str(tmp_path / "a.gguf")
    n = I.write_imatrix_gguf(path, imx)
    assert n == os.path.getsize(path)
    meta, tensors = G.read_gguf(path)
    assert meta["general.type"] == "imatrix" and list(meta["imatrix.datasets"]) == ["corpus-a"]
    assert meta["imatrix.chunk_count"] == 3 and meta["imatrix.chunk_size"] == 512
    assert set(tensors) == {f"{k}.{s}" for k in imx for s in ("in_sum2", "counts")}
    assert tensors["output.weight.in_sum2"].dtype == np.float32 and tensors["output.weight.counts"].shape == (1,)
    back = I.read_imatrix_gguf(path)
    assert list(back) == list(imx) and back.datasets == ["corpus-a"] and (back.chunk_count, back.chunk_size, back.file) == (3, 512, path)
    for k, (s, c) in imx.items():
        assert back[k][1] == c and back[k][0].dtype == np.float64
        assert np.array_equal(back[k][0].astype(np.float32), s.astype(np.float32)) and np.array_equal(back[k][0], s.astype(np.float32))
    other = str(tmp_path / "m.gguf")
    from realtime_codec_agent_amd import quantize as Q
    Q.write_llama_gguf(other, _config(0), {"model.embed_tokens.weight": np.zeros((8, 256), np.float32), "model.norm.weight": np.ones(256, np.float32)})
    with pytest.raises(G.GGUFError, match="not 'imatrix'"):
        I.read_imatrix_gguf(other)
    bad = dict(imx)
    bad["output.weight"] = (np.full(256, np.nan), 5)
    with pytest.raises(ValueError, match="output.weight"):
        I.write_imatrix_gguf(str(tmp_path / "bad.gguf"), bad)


def test_merge_sums_both_fields():
    from realtime_codec_agent_amd import imatrix as I
    cfg = _config()
    a, b = _imatrix(cfg, 0, 1000), _imatrix(cfg, 1, 194)
    b.datasets = ["corpus-b"]
    del b["blk.1.ffn_down.weight"]
    b["extra.weight"] = (np.ones(256), 7)
    m = I.merge(a, b)
    assert set(m) == set(a) | {"extra.weight"} and m.datasets == ["corpus-a", "corpus-b"] and m.chunk_count == 6 and m.chunk_size == 512
    for k in a:
        if k in b:
            assert m[k][1] == 1194 and np.array_equal(m[k][0], a[k][0] + b[k][0])
        else:
            assert m[k][1] == 1000 and np.array_equal(m[k][0], a[k][0])
    assert m["extra.weight"][1] == 7
    b["output.weight"] = (np.ones(128), 3)
    with pytest.raises(ValueError, match="output.weight: 256 columns in one importance matrix, 128 in the other"):
        I.merge(a, b)


def test_every_matrix_gets_its_own_vector_and_the_file_names_the_imatrix(tmp_path):
    """q / k / v share a vector and gate / up share one; the embedding table gets none and no warning; a matrix without an entry is
    quantised unweighted with one warning naming it; every weighted matrix carries the bytes of the weighted definition under exactly
    float32(in_sum2 / count); the written file holds the quantize.imatrix.* keys."""
    from realtime_codec_agent_amd import gguf as G
    from realtime_codec_agent_amd import quantize as Q
    cfg = _config()
    src = lm_ref.random_weights(cfg, 3, 0.05)
    imx = _imatrix(cfg)
    imx.file = "calib.gguf"
    del imx["blk.1.ffn_up.weight"]
    seen = {}

    def host(w, type, rule="search", device=0, name="tensor", col_weights=None):
        f = (np.asarray(w).astype(np.uint32) << 16).view(np.float32) if np.asarray(w).dtype == np.uint16 else np.asarray(w, np.float32)
        seen[name] = None if col_weights is None else np.array(col_weights)
        raw = R.quantize_blocks(f, type, name) if col_weights is None else W.quantize_blocks_w(f, type, col_weights, name)
        return Q.TYPES[type][1](raw, f.shape)

    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        q = Q.quantize_weights(cfg, src, "q4_k_m", quantize_matrix=host, imatrix=imx)
    said = [str(r.message) for r in rec if issubclass(r.category, UserWarning) and "importance matrix" in str(r.message)]
    assert [m.split(" ")[0] for m in said] == ["model.layers.1.mlp.up_proj.weight"]
    assert seen["model.embed_tokens.weight"] is None and seen["model.layers.1.mlp.up_proj.weight"] is None
    vec = lambda name: (imx[name][0] / imx[name][1]).astype(np.float32)
    for l in range(cfg.n_layers):
        p = f"model.layers.{l}."
        for hf, gg in Q.GGUF_NAMES.items():
            if "norm" in gg or (l == 1 and gg == "ffn_up"):
                continue
            got = seen[p + hf + ".weight"]
            assert got.dtype == np.float32 and np.array_equal(got, vec(f"blk.{l}.{gg}.weight")), (l, gg)
        assert np.array_equal(seen[p + "self_attn.q_proj.weight"], seen[p + "self_attn.k_proj.weight"])
        assert np.array_equal(seen[p + "self_attn.q_proj.weight"], seen[p + "self_attn.v_proj.weight"])
        assert not np.array_equal(seen[p + "self_attn.q_proj.weight"], seen[p + "self_attn.o_proj.weight"])
    assert np.array_equal(seen["model.layers.0.mlp.gate_proj.weight"], seen["model.layers.0.mlp.up_proj.weight"])
    assert np.array_equal(seen["lm_head.weight"], vec("output.weight"))
    path = str(tmp_path / "q.gguf")
    Q.write_llama_gguf(path, cfg, q, meta={"quantize.imatrix.file": "stale", "general.name": "tiny"})
    meta, _ = G.read_gguf(path)
    assert meta["quantize.imatrix.file"] == "calib.gguf" and meta["quantize.imatrix.dataset"] == "corpus-a"
    assert meta["quantize.imatrix.entries_count"] == len(imx) and meta["quantize.imatrix.chunks_count"] == 3 and meta["general.name"] == "tiny"
    plain = Q.quantize_weights(cfg, src, "q8_0", quantize_matrix=host)
    Q.write_llama_gguf(path, cfg, plain)
    assert not any(k.startswith("quantize.imatrix.") for k in G.read_gguf(path)[0])


def test_a_vector_of_the_wrong_length_and_the_minmax_rule_are_refused_before_any_work():
    from realtime_codec_agent_amd import quantize as Q
    cfg = _config()
    src = lm_ref.random_weights(cfg, 3, 0.05)
    imx = _imatrix(cfg)
    imx["blk.1.ffn_down.weight"] = (np.ones(256), 10)
    calls = []

    def host(*a, **k):
        calls.append(a)
        raise AssertionError("no matrix may be quantised")

    with pytest.raises(ValueError, match=r"model\.layers\.1\.mlp\.down_proj\.weight: the importance matrix holds 256 columns.*K = 512"):
        Q.quantize_weights(cfg, src, "q4_k_m", quantize_matrix=host, imatrix=imx)
    with pytest.raises(ValueError, match="needs rule 'search'"):
        Q.quantize_weights(cfg, src, "q4_k_m", rule="minmax", quantize_matrix=host, imatrix=_imatrix(cfg))
    assert not calls
    assert Q.imatrix_vector({"a": (np.ones(4), 0)}, "a") is None and Q.imatrix_vector({}, "a") is None


def test_command_line_argument_errors(tmp_path, capsys):
    from realtime_codec_agent_amd import quantize as Q
    with pytest.raises(SystemExit) as e:
        Q.main(["--model", "m", "--out", "o.gguf", "--type", "q4_k_m", "--rule", "minmax", "--imatrix", "f.gguf"])
    assert e.value.code == 2 and "--imatrix needs --rule search" in capsys.readouterr().err
    with pytest.raises(SystemExit) as e:
        Q.main(["--model", "m", "--out", "o.gguf", "--type", "q4_k_m", "--imatrix"])
    assert e.value.code == 2
    with pytest.raises(OSError):
        Q.main(["--model", "m", "--out", "o.gguf", "--type", "q4_k_m", "--imatrix", str(tmp_path / "none.gguf")])       # before the model loads
