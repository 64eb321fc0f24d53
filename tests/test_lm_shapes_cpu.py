"""The LM shape table (tests/lm_shape_cases.py) checked on the host: every case is a shape rca_lm_create accepts and takes the
route / instances it claims, the table as a whole covers the dispatch space, and the tolerances of tests/test_lm_shapes_gpu.py
are tight enough to see the bugs that file exists for (probed on the fp32 oracle alone, no GPU)."""
import functools
import os
import re

import numpy as np
import pytest
import torch

import lm_shape_cases as sc
from conftest import ROOT
from oracle import lm_ref

CASE_IDS = [c.name for c in sc.CASES]


def test_every_case_is_accepted_and_routed_as_claimed():
    names = [c.name for c in sc.CASES]
    assert len(set(names)) == len(names)
    for c in sc.CASES:
        assert c.formats and set(c.formats) <= set(sc.FORMATS), c.name
        for fmt in c.formats:
            assert sc.rejected(c, fmt) is None, (c.name, fmt, sc.rejected(c, fmt))
            assert sc.route(c, fmt) == c.route, (c.name, fmt, sc.route(c, fmt))
            assert sc.route(c, fmt, mfma_prefill=False) == "gemv"
        assert c.prompt > sc.ATT_KEYS + 8 and c.prompt + 2 <= c.n_ctx         # the oracle comparison crosses the 256-key split
        assert c.n_ctx >= 520                                                   # room for the decode steps around 512 keys
        if c.flash is not None:
            # the long prompt's first pass is a full LM_MAXM-token pass of the 128-token route and selects the claimed
            # lm_attn_flash_kernel<G, TEAMS> on a 256-CU device; a piece of more than 512 tokens for the cut-invariance test
            assert c.route == "gemm128" and c.long_prompt > sc.LM_MAXM and c.long_prompt + 2 <= c.n_ctx
            for fmt in c.formats:
                assert sc.first_pass(c, fmt, c.long_prompt) == sc.LM_MAXM
            assert (c.G, sc.flash_teams(c, sc.LM_MAXM, 256)) == c.flash, c.name
            assert sc.flash_teams(c, c.long_prompt - sc.LM_MAXM, 256) == 1       # the remainder pass: the <G, 1> instance


def test_stated_properties_of_the_named_cases():
    """the properties the case names and `reaches` lines promise"""
    b = sc.BY_NAME
    assert b["g1_tile32"].G == 1 and b["g1_tile32"].vocab % 2 == 1
    assert b["g1_fallback"].hidden == b["g1_tile32"].hidden and b["g1_fallback"].ffn == b["g1_tile32"].ffn
    h = b["h136_fallback"]
    assert h.hidden % 64 and (h.hidden >> 3, h.ffn >> 3) == (17, 33) and h.AO != h.hidden and h.vocab % 2 == 1
    assert b["g2_tile32"].G == 2 and b["g2_tile32"].AO != b["g2_tile32"].hidden
    assert b["g4_tile32"].G == 4 and (b["g4_tile32"].AO, b["g4_tile32"].QKV) == (256, 384)
    w = b["g1_gemm128_ffn6144"]
    assert w.G == 1 and sc.gemv_nit(w.ffn) == 3 and set(w.formats) == set(sc.FORMATS)
    assert b["g2_gemm128_ffn4096"].G == 2 and sc.gemv_nit(b["g2_gemm128_ffn4096"].ffn) == 2
    assert sc.gemv_nit(b["g1_h2048_ffn8192"].ffn) == 4
    for n in ("g4_k768", "g1_k768"):
        assert b[n].hidden == 768 and b[n].ffn == 768 and "q4_k" in b[n].formats
    r = b["nctx700"]
    assert r.n_ctx % sc.ATT_KEYS and sc.cdiv(r.n_ctx, sc.ATT_KEYS) * sc.ATT_KEYS == 768


def test_table_covers_the_dispatch_space():
    pairs = {(c.G, sc.route(c, f)) for c in sc.CASES for f in c.formats}
    # every (group size, route) pair: all nine are reachable under the shape rules
    assert pairs == {(g, r) for g in (1, 2, 4) for r in sc.ROUTES}
    assert {sc.gemv_nit(c.ffn) for c in sc.CASES} == {1, 2, 3, 4}
    pow2 = lambda n: n & (n - 1) == 0
    for fmt in sc.FORMATS:
        assert any(fmt in c.formats and not pow2(c.hidden) and not pow2(c.ffn) for c in sc.CASES), fmt
    assert any(c.vocab % 2 for c in sc.CASES)
    assert any(c.n_ctx % sc.ATT_KEYS for c in sc.CASES)
    assert {c.flash for c in sc.CASES if c.flash} >= {(1, 2), (2, 2)}
    assert any(c.AO != c.hidden for c in sc.CASES if c.route == "tile32")


def test_restated_rules_refuse_what_the_library_refuses():
    """the restatement is not vacuous: shapes outside the ABI are refused, near misses of a route fall to the next one"""
    mk = lambda **kw: sc.ShapeCase(**{**dict(name="x", hidden=256, n_heads=4, n_kv_heads=1, ffn=512, vocab=100, formats=("bf16",),
                                             route="", reaches="", seed=0), **kw})
    assert sc.rejected(mk(), "bf16") is None and sc.route(mk(), "bf16") == "gemm128"
    assert sc.rejected(mk(n_heads=8, n_kv_heads=1), "bf16") and sc.rejected(mk(n_heads=3, n_kv_heads=2), "bf16")
    assert sc.rejected(mk(hidden=132), "bf16") and sc.rejected(mk(ffn=3072), "bf16") and sc.rejected(mk(ffn=10240), "bf16")
    assert sc.rejected(mk(hidden=2176), "bf16") and sc.rejected(mk(hidden=136), "q8_0") and sc.rejected(mk(hidden=192), "q4_k")
    assert sc.rejected(mk(vocab=1001), "q8_0") and sc.rejected(mk(vocab=1002), "q4_k") and sc.rejected(mk(vocab=1001), "f16") is None
    assert sc.rejected(mk(hidden=192), "q8_0") is None and sc.rejected(mk(ffn=6144), "q4_k") is None
    assert sc.route(mk(hidden=192), "bf16") == "tile32" and sc.route(mk(hidden=192), "f16") == "gemv"
    assert sc.route(mk(ffn=328), "bf16") == "gemv" and sc.route(mk(hidden=136), "bf16") == "gemv"
    assert [sc.gemv_nit(k) for k in (136, 2048, 2056, 4096, 6144, 8192)] == [1, 1, 2, 2, 3, 4]
    assert [sc.flash_teams(mk(n_heads=16, n_kv_heads=16), m, 256) for m in (76, 512, 960, 961, 1024)] == [1, 1, 1, 2, 2]
    assert sc.flash_teams(mk(n_heads=16, n_kv_heads=16), 1024, 304) == 1


def test_restated_constants_and_predicates_match_the_source():
    """the limits and the predicates restated in lm_shape_cases.py, read back from rca_lm.hip: a changed dispatch condition fails
    here (and in the GPU file's route assertion) instead of silently moving a case to another route"""
    src = open(os.path.join(ROOT, "realtime_codec_agent_amd", "csrc", "rca_lm.hip")).read()
    for name, val in (("LM_KSLICE", sc.LM_KSLICE), ("LM_MAXSPLIT", sc.LM_MAXSPLIT), ("LM_MAXM", sc.LM_MAXM), ("LM_TILE32", sc.LM_TILE32),
                      ("LM_PREFILL_MIN", sc.LM_PREFILL_MIN), ("ATT_KEYS", sc.ATT_KEYS)):
        m = re.search(rf"#define {name}\s+(\d+)", src)
        assert m and int(m.group(1)) == val, name
    squash = lambda s: re.sub(r"\s+", "", s)
    flat = squash(src)
    for line in (
        "H % 128 == 0 && QKV % 128 == 0 && (2 * F) % 128 == 0 && AO % 32 == 0 && F % 32 == 0",
        "lm_all_bf16(h) && c.hidden % 64 == 0 && AO % 64 == 0 && c.ffn % 64 == 0 && (2 * c.ffn) % 32 == 0",
        "const int nit = cdiv(cdiv(K >> 3, 4), 64);",
        "if (c.n_kv_heads * cdiv(ntiles, 4) >= h->n_cus)",
        "else if (c.n_kv_heads * cdiv(ntiles, 2) >= h->n_cus)",
        "const int ntiles = cdiv(M * G, 32);",
    ):
        assert squash(line) in flat, line


# ------------------------------------------------------------------ would the tolerance catch the bugs this sweep exists for?
PROBE_FACTOR = 3.0     # a condition of the table, not a measurement: a case that misses it gets other inputs, not a smaller factor


@functools.lru_cache(maxsize=None)
def _probe_ratios(name):
    c = sc.BY_NAME[name]
    cfg = c.config()
    ids = c.ids()[:c.prompt]
    w = lm_ref.random_weights(cfg, c.seed, sc.INIT_STD)
    last = f"model.layers.{cfg.n_layers - 1}."

    def logits(weights, **kw):
        return lm_ref.LMRef(cfg, weights, kv_dtype=torch.float16).eval(ids, last_only=True, **kw)[-1].numpy()

    def edited(key, fn):
        w2 = dict(w)
        a = w[key].copy()
        fn(a)
        w2[key] = a
        return w2

    want = logits(w)
    bound = sc.bound(want, sc.TOL_TILE)

    def zero_cols(a): a[:, -8:] = 0
    def zero_rows4(a): a[-4:, :] = 0
    def zero_rows2(a): a[-2:, :] = 0
    out = {
        "down_proj K tail (8 columns, layer 0)": logits(edited("model.layers.0.mlp.down_proj.weight", zero_cols)),
        "o_proj N tail (4 rows, last layer)": logits(edited(last + "self_attn.o_proj.weight", zero_rows4)),
        "gate_proj N tail (2 rows, layer 0)": logits(edited("model.layers.0.mlp.gate_proj.weight", zero_rows2)),
        "key 256 dropped": logits(w, drop_keys=(256, 257)),
    }
    if c.n_kv_heads >= 2:
        w2 = dict(w)
        for l in range(cfg.n_layers):
            k = f"model.layers.{l}.self_attn.k_proj.weight"
            a = w[k].copy()
            a[:64], a[64:128] = w[k][64:128], w[k][:64]
            w2[k] = a
        out["K heads 0 and 1 exchanged"] = logits(w2)
    # for scale: what a legitimate rounding difference (fp32 instead of fp16 KV) moves
    kv32 = lm_ref.LMRef(cfg, w, kv_dtype=None).eval(ids, last_only=True)[-1].numpy()
    return {k: float(np.abs(v - want).max()) / bound for k, v in out.items()}, float(np.abs(kv32 - want).max()) / bound


@pytest.mark.parametrize("name", CASE_IDS)
def test_tolerance_would_catch_a_lost_tail_a_lost_key_and_a_wrong_group_mapping(name):
    """On the oracle alone: logits of a deliberately wrong model (a lost K tail, lost N tails, one key of the second attention split
    masked out, two K heads exchanged) are at least PROBE_FACTOR tile-route bounds away from the right ones, while the legitimate
    fp16-vs-fp32 KV rounding stays well inside one bound."""
    ratios, kv32 = _probe_ratios(name)
    print(f"{name}: " + "; ".join(f"{k} {v:.1f}x" for k, v in ratios.items()) + f"; fp32 KV {kv32:.2f}x")
    for k, v in ratios.items():
        assert v >= PROBE_FACTOR, (name, k, v)
    assert kv32 < 1.0, (name, kv32)
