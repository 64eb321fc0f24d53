"""GGUF IQ4_NL / IQ4_XS matrices on the device (WF_IQ4 / WF_IQ4XS in rca_lm.hip): the Q4_K quad layout of the nibbles, which index the
16-entry int8 table kvalues_iq4nl, plus one f32 factor per slot and 32 values, value = s kv[q], streamed packed by the decode GEMVs (f32
and q8_1 activations; the table look-up is three byte permutes per four weights) and de-quantised while staging by the prefill tiles.

A hand-made matrix is read out EXACTLY first (one-hot inputs); then the same values as IQ4_NL and as IQ4_XS blocks must give the same
bits on every path (one device form); every GEMV stage is held to the derived rounding bound of the float64 product forms
(tests/iq4_ref.py, tests/lm_q8_1_ref.py); files and the load-time quantiser go against LMRef at the project's tolerances
(lm_shape_cases.TOL_EXACT / TOL_TILE)."""
import functools

import numpy as np
import pytest
import torch

import iq4_ref
import lm_iq4_cases as C
import lm_q8_1_ref as R
import lm_shape_cases as sc
from oracle import lm_ref

pytestmark = pytest.mark.gpu

KINDS = {0: "qkv", 1: "o", 2: "gate_up", 3: "down", 4: "head"}
ACTS = ("f32", "q8_1")
TYPES = ("iq4_nl", "iq4_xs")
TTYPE = {"iq4_nl": iq4_ref.IQ4_NL, "iq4_xs": iq4_ref.IQ4_XS}


def _config(vocab, hidden, n_heads, n_kv, ffn, n_layers=2):
    from realtime_codec_agent_amd.llm import LMConfig
    return LMConfig(vocab_size=vocab, hidden=hidden, n_layers=n_layers, n_heads=n_heads, n_kv_heads=n_kv, head_dim=64, ffn=ffn, rope_scaling=None,
                    rope_theta=10000.0)


def _from_weights(cfg, weights, **kw):
    from realtime_codec_agent_amd.llm import LlamaForAlternatingCodeChannels
    return LlamaForAlternatingCodeChannels(config=cfg, weights=weights, n_ctx=kw.pop("n_ctx", 256), device=0, **kw)


def _random(name, cfg, seed, fmt, **kw):
    from realtime_codec_agent_amd.llm import LlamaForAlternatingCodeChannels
    return LlamaForAlternatingCodeChannels(model_path=f"random:{name}", config=cfg, n_ctx=kw.pop("n_ctx", 256), random_seed=seed, init_std=C.INIT_STD,
                                           device=0, weight_format=fmt, **kw)


# ------------------------------------------------------------------------------------------------------------------ 1. one-hot readout
HAND_CFG = dict(vocab=512, hidden=256, n_heads=4, n_kv=2, ffn=512)


@functools.lru_cache(maxsize=None)
def _hand_model(fmt):
    """Every matrix IQ4_NL; layer 0's down_proj [256, 512] hand-made in the type under test: d a power of two that differs per block and
    per row parity, of both signs; indices a function of (row, k) that takes all 16 values at every (row mod 4, k mod 8), i.e. at every
    nibble of the quad's 16-byte unit; IQ4_XS: ls from a list that holds 0, 31, 32 and 63."""
    cfg = _config(**HAND_CFG)
    w = iq4_ref.blocks_model(lm_ref.random_weights(cfg, 21, C.INIT_STD))
    N, K = cfg.hidden, cfg.ffn
    row, k = np.meshgrid(np.arange(N), np.arange(K), indexing="ij")
    q = ((5 * k + 11 * row + 3 * (k >> 3) + (row >> 2)) & 15).astype(np.uint8)
    seen = np.zeros((4, 8, 16), bool)
    seen[row % 4, k % 8, q] = True
    assert seen.all()
    if fmt == "iq4_nl":
        rb, kb = row[:, ::32], k[:, ::32] // 32                                              # [N, K / 32]
        d = (np.where((kb + rb // 2) % 3 == 0, -1.0, 1.0) * 2.0 ** -(9 + kb % 3 + rb % 2)).astype(np.float16)
        assert (d > 0).any() and (d < 0).any() and len(np.unique(d)) == 8
        down = iq4_ref.block_class(iq4_ref.IQ4_NL)(iq4_ref.pack_iq4_nl(dict(q=q, d=d)), (N, K))
    else:
        rb, kb = row[:, ::256], k[:, ::256] // 256                                           # [N, K / 256]
        d = (np.where((kb + rb // 2) % 3 == 0, -1.0, 1.0) * 2.0 ** -(12 + kb % 2 + rb % 2)).astype(np.float16)
        assert (d > 0).any() and (d < 0).any() and len(np.unique(d)) >= 4
        codes = np.array([0, 31, 32, 63, 1, 33, 47, 16, 62, 30, 34, 5])
        r32, k32 = row[:, ::32], k[:, ::32] // 32
        ls = codes[(3 * k32 + r32) % len(codes)]
        assert {0, 31, 32, 63} <= set(ls.reshape(-1).tolist())
        down = iq4_ref.block_class(iq4_ref.IQ4_XS)(iq4_ref.pack_iq4_xs(dict(q=q, d=d, ls=ls)), (N, K))
    w["model.layers.0.mlp.down_proj.weight"] = down
    values = down.dequantize()
    values.setflags(write=False)
    return _from_weights(cfg, w), down, values


@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("fmt", TYPES)
def test_one_hot_inputs_read_every_weight_of_a_hand_made_matrix(fmt, act):
    """rca_lm_gemv_tap(kind 3) with one-hot rows, two columns per call, all 512 k.
    f32 activations: the lane's chain is kv * 1 plus zeros, s kv is exact and every later sum adds zeros: y must equal the de-quantised
    column, so every nibble position of the permute look-up returns the table's entry.
    q8_1 activations: the one-hot row quantises to q_x = 127 and d_x = fp16(1 / 127), and fp16(1 / 127) * 127 is not 1: that path is NOT
    exact.  It is compared with the integer form in float64 within the derived bound (iq4_ref.gemv_q8_1_bound)."""
    llm, down, values = _hand_model(fmt)
    llm.set_activation_format(act)
    K = values.shape[1]
    W = iq4_ref.qmat(down)
    worst = 0.0
    for k0 in range(0, K, 2):
        x = np.zeros((2, K), np.float32)
        x[0, k0] = x[1, k0 + 1] = 1.0
        llm.reset()
        y = llm.gemv_tap(0, 3, x)
        if act == "f32":
            assert np.array_equal(y, values[:, k0:k0 + 2].T), k0
        else:
            want, mag = R.gemv_q8_1(W, x)
            bound = iq4_ref.gemv_q8_1_bound(K, mag)
            err = np.abs(y.astype(np.float64) - want)
            assert np.all(err <= bound), k0
            worst = max(worst, float((err / np.where(bound > 0, bound, 1)).max()))
    if act == "q8_1":
        print(f"{fmt} q8_1 one-hot readout: max err / bound = {worst:.3f}")
    llm.set_activation_format("f32")


# ------------------------------------------------------------------------------------------------------------------ 2. one device form
def test_the_same_values_as_iq4_nl_and_as_iq4_xs_give_the_same_bits():
    """The same values twice (iq4_ref.twin_models): as IQ4_NL blocks whose d is constant over each 256 values, and as IQ4_XS blocks with
    that d and every ls = 33.  40-token evals on both prefill routes and two graph steps give the same logits bit for bit, with f32 and
    with q8_1 activations in the decode GEMVs: the two types are one form on the device."""
    cfg = _config(1024, 256, 4, 2, 512)
    wa, wb = iq4_ref.twin_models(cfg, 23)
    a, b = _from_weights(cfg, wa), _from_weights(cfg, wb)
    assert (a.weight_format, b.weight_format) == ("iq4_nl", "iq4_xs")
    assert a.weight_bytes_per_step() == b.weight_bytes_per_step()
    ids = np.random.default_rng(2).integers(0, 1024, 44).tolist()
    for act in ACTS:
        for mfma in (False, True):
            rows = []
            for llm in (a, b):
                llm.set_activation_format(act)
                llm.set_mfma_prefill(mfma)
                llm.set_graphs(True)
                llm.reset()
                llm.eval(ids[:40])
                out = [llm._scores[-1].copy()]
                llm.init_sampler_for_generate(top_k=50, top_p=1.0, min_p=0.0, temp=1.0, seed=3)
                for s in range(2):
                    llm.step(ids[40 + 2 * s:42 + 2 * s])
                    out.append(llm._scores[-1].copy())
                rows.append(out)
            assert a.prefill_route() == b.prefill_route() == ("gemm128" if mfma else "gemv")
            for x, y in zip(*rows):
                assert np.array_equal(x, y) and np.abs(x).max() > 0, (act, mfma)
    a.close()
    b.close()


# ------------------------------------------------------------------------------------------------------------------ 3. stages
# the three shapes of test_lm_q40_gpu.py: name -> (vocab, hidden, heads, kv heads, ffn, seed)
#   k256:  K = 256: 32 chunks, 8 per wave; a head of 1004 rows: a multiple of 4 but not of 16, the last group of 16 factor slots is ragged
#   k768:  K = 3 x 256 (not a power of two), G = 4
#   k1024: ffn 6144 = the NIT = 4 instance of the down projection with a short last chunk
STAGE_MODELS = {"k256": (1004, 256, 4, 2, 512, 51), "k768": (1536, 768, 12, 3, 768, 39), "k1024": (2048, 1024, 16, 16, 6144, 37)}


class _LazyIQ4:
    """HF name -> QMat of the matrix's IQ4_NL blocks by the numpy rule, built on first use"""

    def __init__(self, weights):
        self.weights, self.done = weights, {}

    def __getitem__(self, k):
        if k not in self.done:
            self.done[k] = iq4_ref.qmat(iq4_ref.to_blocks(self.weights[k]))
        return self.done[k]


@functools.lru_cache(maxsize=None)
def _stage_model(name):
    v, h, nh, nkv, f, seed = STAGE_MODELS[name]
    cfg = _config(v, h, nh, nkv, f)
    w = lm_ref.random_weights(cfg, seed, C.INIT_STD)
    return _random(name, cfg, seed, "iq4_nl"), iq4_ref.stage_refs(cfg, _LazyIQ4(w), R.model_norms(w))


@functools.lru_cache(maxsize=None)
def _stage_input(name, kind, M):
    llm, refs = _stage_model(name)
    c = refs["f32"].cfg
    rng = np.random.default_rng(1000 * kind + 10 * M + len(name))
    K = R.STAGE_WIDTHS(c)[kind]
    if kind in (0, 2, 4):    # behind an RMSNorm: rows on which the device's q8_1 quantiser provably takes the reference's decisions
        nw = refs["f32"].norms[{0: "model.layers.0.input_layernorm.weight", 2: "model.layers.0.post_attention_layernorm.weight", 4: "model.norm.weight"}[kind]]
        x, _ = R.guarded_input(rng, (M, K), (nw, c.rms_eps))
    else:
        x = R.planted_input(rng, (M, K), scale=0.3 if kind == 1 else 0.1)
    x.setflags(write=False)
    return x


@pytest.mark.parametrize("M", [1, 2])
@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("kind", sorted(KINDS))
@pytest.mark.parametrize("name", sorted(STAGE_MODELS))
def test_stage_is_within_the_rounding_bound_of_its_float64_form(name, kind, act, M):
    """Every GEMV stage of the decode step, as the step launches it, on IQ4_NL matrices quantised on the device: within the derived f32
    rounding bound of the float64 form over the numpy-quantised blocks -- magnitudes |s| |kv| |x|, operation counts
    iq4_ref.gemv_f32_ops / gemv_q8_1_ops (the signed table is converted directly: there is no bias term) -- and the new K / V rows after
    the same fp16 rounding, one fp16 ulp allowed."""
    llm, refs = _stage_model(name)
    x = _stage_input(name, kind, M)
    want = refs[act].run(kind, 0, x, pos0=0)
    llm.set_activation_format(act)
    llm.reset()
    got = llm.gemv_tap(0, kind, x, want_kv=(kind == 0))
    llm.set_activation_format("f32")
    y = got[0] if kind == 0 else got
    err = np.abs(y.astype(np.float64) - want["y"])
    r = float(np.max(np.where(want["bound"] > 0, err / np.where(want["bound"] > 0, want["bound"], 1.0), np.where(err > 0, np.inf, 0.0))))
    print(f"iq4_nl {name} {KINDS[kind]} {act} M={M}: max err / bound = {r:.3f} (max|y| {np.abs(want['y']).max():.3f}, max bound {want['bound'].max():.3e})")
    assert r <= 1.0
    if kind == 0:
        for nm, rows in (("k", got[1]), ("v", got[2])):
            ok = R.fp16_within_one_ulp(rows, want[nm], want[nm + "_bound"])
            assert ok.all(), f"{nm} rows: {np.count_nonzero(~ok)} values off by more than one fp16 ulp"


# ------------------------------------------------------------------------------------------------------------------ 4. files
@pytest.mark.parametrize("name", sorted(C.FILES))
def test_gguf_files_stay_packed_and_match_their_dequantisation(name, tmp_path):
    """An IQ4_NL-only file, an IQ4_XS-only file and the mix a llama-quantize IQ4_XS file holds (output.weight Q6_K, attn_v and layer 0's
    ffn_down Q5_K beside IQ4_XS neighbours) through model_path=.  Logits equal LMRef over the file's own blocks de-quantised on the host,
    exact route and 128-token tiles (and a decode pass on the tiles' cache); prefill equals incremental evaluation; a graph step equals
    the eager one; a twin over the same weights computes the same bits; masked head rows read exactly 0 and the others do not move.
    The argmax is compared where the oracle's top-two margin exceeds twice the bound (every file's compared position: lm_iq4_cases)."""
    from realtime_codec_agent_amd.llm import LlamaForAlternatingCodeChannels
    path = str(tmp_path / f"{name}.gguf")
    C.write_file(name, path)
    file_w, want, gap = C.file_oracle(name, path)
    kinds = {type(v).__name__ for k, v in file_w.items() if hasattr(v, "raw")}
    assert kinds == {"iq4_nl": {"IQ4NLBlocks"}, "iq4_xs": {"IQ4XSBlocks"}, "iq4_xs_mix": {"IQ4XSBlocks", "Q5KBlocks", "Q6KBlocks"}}[name]
    clear = gap > C.gap_needed(want)
    assert clear, "the compared position has no clear argmax: pick another seed (tests/lm_iq4_cases.py)"
    g = LlamaForAlternatingCodeChannels(model_path=path, n_ctx=512, device=0)
    fmt = "iq4_nl" if name == "iq4_nl" else "iq4_xs"
    assert g.weight_format == fmt
    nbytes = 0
    for k, v in file_w.items():
        if iq4_ref.is_projection(k):
            n = int(np.prod(v.shape))
            kind = type(v).__name__
            nbytes += n + n // 4 if kind == "Q6KBlocks" else (n // 2 + n // 8 + n // 16 + n // 64 if kind == "Q5KBlocks" else n // 2 + n // 8)
    assert g.weight_bytes_per_step() == nbytes
    ids = C.file_ids(name).tolist()
    got = {}
    for mfma in (False, True):
        g.set_mfma_prefill(mfma)
        g.reset()
        g.eval(ids)
        got[mfma] = g._scores[-1].copy()
        d, b = float(np.abs(got[mfma] - want).max()), sc.bound(want, sc.TOL_TILE if mfma else sc.TOL_EXACT)
        print(f"{name} GGUF ({g.prefill_route()}) vs LMRef over the file's blocks: max|dlogit| = {d:.3e}, bound {b:.3e} (|logit| max {np.abs(want).max():.2f})")
        assert g.prefill_route() == ("gemm128" if mfma else "gemv")
        assert d <= b and got[mfma].argmax() == want.argmax()
    # a decode pass on the tiles' cache: the last two tokens again as a step over the cache the tiles built
    g.n_tokens = len(ids) - 2
    g.eval(ids[-2:])
    d, b = float(np.abs(g._scores[-1] - want).max()), sc.bound(want, sc.TOL_TILE)
    print(f"{name} GGUF decode pass on the tile cache: max|dlogit| = {d:.3e}, bound {b:.3e}")
    assert d <= b and g._scores[-1].argmax() == want.argmax()
    # tiles: prefill == incremental evaluation at the tiles' tolerance
    g.reset()
    g.eval(ids[:-9])
    g.eval(ids[-9:])
    d = float(np.abs(g._scores[-1] - want).max())
    assert d <= b, ("incremental evaluation on the tile route", d, b)
    # exact route: a 2-token pass on the exact-route cache, eager eval == graph step; twin
    g.set_mfma_prefill(False)
    g.reset()
    g.eval(ids[:-2])
    g.eval(ids[-2:])
    assert np.array_equal(g._scores[-1], got[False])            # prefill == incremental on the exact route
    g.init_sampler_for_generate(top_k=50, top_p=1.0, min_p=0.0, temp=0.0, seed=1)
    g.set_graphs(True)
    for _ in range(2):                                           # the second round replays the captured step
        g.n_tokens = len(ids) - 2
        assert g.step(ids[-2:]) == int(want.argmax()) and np.array_equal(g._scores[-1], got[False])
    twin = LlamaForAlternatingCodeChannels(model_path="random:twin", n_ctx=256, share_weights_with=g, device=0)
    assert twin.weight_format == fmt
    twin.set_mfma_prefill(False)
    twin.eval(ids)
    assert np.array_equal(twin._scores[-1], got[False])
    twin.close()
    g.mask_head_rows(0, 64)
    g.n_tokens = len(ids) - 2
    g.eval(ids[-2:])
    assert np.all(g._scores[-1][:64] == 0) and np.array_equal(g._scores[-1][64:], got[False][64:])
    g.close()


# ------------------------------------------------------------------------------------------------------------------ 5. quantiser
QUANT_CASES = ("g4_k768", "g1_gemm128_ffn6144")


@functools.lru_cache(maxsize=None)
def _quantised(name):
    """(bf16-bit weights of the shape case, the same as host-quantised blocks, their float32 values): one pass of the numpy rule"""
    c = sc.BY_NAME[name]
    src = lm_ref.random_weights(c.config(), c.seed, sc.INIT_STD)
    blocks = iq4_ref.blocks_model(src)
    return src, blocks, {k: (v.dequantize() if hasattr(v, "raw") else v) for k, v in blocks.items()}


@pytest.mark.parametrize("name", QUANT_CASES)
def test_the_device_quantiser_is_the_numpy_rule_block_for_block(name):
    """weight_format="iq4_nl" over bf16 weights (quantised on the device at load) against the same weights quantised by
    iq4_ref.quantize_iq4_nl and supplied as blocks: the same logits bit for bit, prefill tiles, exact route and decode passes.
    g1_gemm128_ffn6144 runs the NIT = 4 down projection."""
    c = sc.BY_NAME[name]
    src, blocks, _ = _quantised(name)
    dev = _from_weights(c.config(), src, weight_format="iq4_nl", n_ctx=c.n_ctx)
    host = _from_weights(c.config(), blocks, n_ctx=c.n_ctx)
    assert dev.weight_format == host.weight_format == "iq4_nl"
    n = sum(int(np.prod(v.shape)) for k, v in src.items() if iq4_ref.is_projection(k))
    assert dev.weight_bytes_per_step() == host.weight_bytes_per_step() == n // 2 + n // 8          # nibbles, f32 s per 32: 5.0 bits
    ids = c.ids().tolist()
    for mfma in (True, False):
        out = []
        for llm in (dev, host):
            llm.set_mfma_prefill(mfma)
            llm.reset()
            llm.eval(ids[:40])
            a = llm._scores[-1].copy()
            llm.eval(ids[40:42])
            out.append((a, llm._scores[-1].copy()))
        assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1]), mfma
        assert np.abs(out[0][0]).max() > 0
    dev.close()
    host.close()


@pytest.mark.parametrize("name", QUANT_CASES)
def test_load_time_quantisation_matches_oracle_over_the_quantised_model(name):
    """model_path="random:" with weight_format="iq4_nl" at two shapes of lm_shape_cases -- K = 3 x 256 at G = 4, and hidden 1024 /
    ffn 6144 (the NIT = 4 down projection) -- against LMRef over the numpy-quantised model: exact route at TOL_EXACT, the 128-token tiles
    and a decode pass on their cache at TOL_TILE; argmax compared where the oracle's top-two margin exceeds twice the bound (the shape
    cases fix their own seeds: on g1_gemm128_ffn6144 the oracle's two largest logits after the prefill are closer than that, and that
    row is held to the logit bound alone)."""
    c = sc.BY_NAME[name]
    ids = c.ids().tolist()
    P = c.prompt
    llm = _random(name, c.config(), c.seed, "iq4_nl", n_ctx=c.n_ctx)
    for mfma in (False, True):
        ref = lm_ref.LMRef(c.config(), _quantised(name)[2], kv_dtype=torch.float16)
        llm.set_mfma_prefill(mfma)
        llm.reset()
        assert llm.prefill_route() == ("gemm128" if mfma else "gemv")
        tol = sc.TOL_TILE if mfma else sc.TOL_EXACT
        llm.eval(ids[:P - 2])
        rows = [(llm._scores[-1].copy(), ref.eval(ids[:P - 2], last_only=True)[-1].numpy(), f"prefill of {P - 2}")]
        llm.eval(ids[P - 2:P])
        rows.append((llm._scores[-1].copy(), ref.eval(ids[P - 2:P])[-1].numpy(), f"decode at {P} keys"))
        for got, want, what in rows:
            d, b = float(np.abs(got - want).max()), sc.bound(want, tol)
            top = np.sort(want)[-2:]
            clear = float(top[1] - top[0]) > 2 * b
            print(f"iq4_nl {name} {llm.prefill_route()} {what}: max|dlogit| = {d:.3e}, bound {b:.3e} (max|logit| {np.abs(want).max():.2f}), ratio {d / b:.3f}, "
                  f"top-two margin {'clear' if clear else 'inside twice the bound'}")
            assert d <= b, (name, mfma, what)
            if clear:
                assert got.argmax() == want.argmax(), (name, mfma, what)
    llm.close()


# ------------------------------------------------------------------------------------------------------------------ 6. embedding table
@pytest.mark.parametrize("fmt", TYPES)
def test_an_embedding_table_of_iq4_rows_is_dequantised_on_the_device_exactly(fmt):
    """RCA_IQ4_NL / RCA_IQ4_XS are accepted for the embedding table too (the GGUF importer de-quantises it on the host, a C caller need
    not): the device's f32 rows equal the host's de-quantisation, so the logits are the same bits."""
    cfg = _config(1024, 256, 4, 2, 512)
    src = lm_ref.random_weights(cfg, 29, C.INIT_STD)
    w = iq4_ref.blocks_model(src)
    emb = iq4_ref._f32(src["model.embed_tokens.weight"])
    rows = iq4_ref.to_blocks(emb) if fmt == "iq4_nl" else iq4_ref.xs_blocks_of(emb, np.random.default_rng(3))
    assert type(rows).__name__ == ("IQ4NLBlocks" if fmt == "iq4_nl" else "IQ4XSBlocks")
    ids = np.random.default_rng(6).integers(0, 1024, 12).tolist()
    out = []
    for table in (rows, rows.dequantize()):
        llm = _from_weights(cfg, dict(w, **{"model.embed_tokens.weight": table}))
        llm.eval(ids)
        out.append(llm._scores[-1].copy())
        llm.close()
    assert np.array_equal(out[0], out[1]) and np.abs(out[0]).max() > 0


# ------------------------------------------------------------------------------------------------------------------ 7. group and batch
@functools.lru_cache(maxsize=None)
def _family(n):
    """a parent over host-quantised IQ4_NL blocks and n - 1 twins, and the float32 values for LMRef"""
    from realtime_codec_agent_amd.llm import LlamaForAlternatingCodeChannels as L
    cfg = C.file_config("iq4_nl")
    blocks = iq4_ref.blocks_model(lm_ref.random_weights(cfg, 5, C.INIT_STD))
    parent = _from_weights(cfg, blocks, n_ctx=512)
    deq = {k: (v.dequantize() if hasattr(v, "raw") else v) for k, v in blocks.items()}
    return cfg, [parent] + [L(n_ctx=512, share_weights_with=parent, device=0) for _ in range(n - 1)], deq


@pytest.mark.parametrize("act", ACTS)
def test_a_group_step_over_iq4_members_equals_their_single_steps(act):
    """the four-row group step (4 members x 1 token) and the 2 x 2 one: every member's logits are the bits its own step() gives"""
    from realtime_codec_agent_amd.llm import LlamaGroup
    cfg, fam, _ = _family(8)
    ids = np.random.default_rng(77).integers(0, cfg.vocab_size, 600).tolist()
    for nm, n in ((4, 1), (2, 2)):
        A, B = fam[4:4 + nm], fam[:nm]                      # the group holds the parent and its twins
        for llm in fam:
            llm.set_activation_format(act)
            llm.set_graphs(True)
        for s in range(nm):
            for llm in (A[s], B[s]):
                llm.reset()
                llm.eval(ids[7 * s:7 * s + 30 + 5 * s])
                llm.init_sampler_for_generate(top_k=50, top_p=1.0, min_p=0.0, temp=1.0, seed=3 + s)
        grp = LlamaGroup(B)
        try:
            for t in range(2):
                rows = [[ids[(300 + 31 * s + n * t + j)] for j in range(n)] for s in range(nm)]
                want = [a.step(r) for a, r in zip(A, rows)]
                assert grp.step(rows) == want, (nm, n, t)
                for a, b in zip(A, B):
                    assert np.array_equal(a._scores[-1], b._scores[-1]) and np.abs(a._scores[-1]).max() > 0, (nm, n, t)
        finally:
            grp.close()
    for llm in fam:
        llm.set_activation_format("f32")


def test_a_batch_step_over_iq4_members_is_inside_the_tile_tolerance_of_lmref():
    """five members on the 128-token tiles: caches built by eval, one batch step of 2 tokens each; every member's logits against LMRef
    over the member's own sequence (the host de-quantisation of the same blocks), inside bound(want, TOL_TILE)"""
    from realtime_codec_agent_amd.llm import LlamaBatch
    cfg, fam, deq = _family(8)
    members = fam[:5]
    ids = np.random.default_rng(78).integers(0, cfg.vocab_size, 600).tolist()
    seqs = []
    for s, llm in enumerate(members):
        llm.set_activation_format("f32")
        llm.set_mfma_prefill(True)
        llm.set_graphs(True)
        llm.reset()
        seq = ids[11 * s:11 * s + 36 + 3 * s]
        llm.eval(seq)
        llm.init_sampler_for_generate(top_k=50, top_p=1.0, min_p=0.0, temp=1.0, seed=9 + s)
        seqs.append(seq + ids[400 + 2 * s:402 + 2 * s])
    bat = LlamaBatch(members)
    try:
        bat.step([q[-2:] for q in seqs])
        worst = 0.0
        for s, llm in enumerate(members):
            want = lm_ref.LMRef(cfg, deq, kv_dtype=torch.float16).eval(np.array(seqs[s]))[-1].numpy()
            got = llm._scores[-1]
            worst = max(worst, float(np.abs(got - want).max()) / sc.bound(want, sc.TOL_TILE))
        print(f"batch step over IQ4_NL members: worst max|dlogit| / bound(TOL_TILE) = {worst:.3f}")
        assert worst <= 1.0
    finally:
        bat.close()
    for llm in members:
        llm.set_mfma_prefill(False)


# ------------------------------------------------------------------------------------------------------------------ 8. refusals
def test_shapes_the_layout_cannot_hold_are_refused_by_name():
    from realtime_codec_agent_amd._native import RcaError
    with pytest.raises(RcaError, match="IQ4_NL needs rows of a multiple of 256"):
        _random("h192", _config(1000, 192, 3, 3, 320), 1, "iq4_nl")
    with pytest.raises(RcaError, match=r"IQ4_NL weights: lm_head is 1002 x 256 \(K must be a multiple of 256, N of 4\)"):
        _random("v1002", _config(1002, 256, 4, 2, 512), 1, "iq4_nl")
    cfg = _config(1002, 256, 4, 2, 512)
    src = lm_ref.random_weights(cfg, 29, C.INIT_STD)
    w = {k: (iq4_ref.xs_blocks_of(iq4_ref._f32(v), np.random.default_rng(1)) if iq4_ref.is_projection(k) else v) for k, v in src.items()}
    with pytest.raises(RcaError, match=r"IQ4_XS weights: lm_head is 1002 x 256 \(K must be a multiple of 256, N of 4\)"):
        _from_weights(cfg, w)
    llm = _random("q81", _config(1024, 256, 4, 2, 512), 1, "iq4_nl", activation_format="q8_1")      # an IQ4-only handle counts as packed
    assert llm.weight_format == "iq4_nl" and llm.activation_format == "q8_1"
    llm.eval([1, 2, 3])
    assert np.isfinite(llm._scores[-1]).all()
    llm.close()


@pytest.mark.parametrize("fmt", TYPES)
def test_a_block_whose_d_is_not_finite_is_refused_with_the_tensors_name(fmt):
    from realtime_codec_agent_amd._native import RcaError
    cfg = _config(1024, 256, 4, 2, 512)
    src = lm_ref.random_weights(cfg, 29, C.INIT_STD)
    w = iq4_ref.blocks_model(src)
    key = "model.layers.1.mlp.down_proj.weight"                                     # [256, 512]: two IQ4_XS super-blocks per row
    bad = w[key] if fmt == "iq4_nl" else iq4_ref.xs_blocks_of(iq4_ref._f32(src[key]), np.random.default_rng(1))
    raw = bad.raw.copy()
    off = iq4_ref.BLOCK_BYTES[TTYPE[fmt]]                                           # the second block of row 3
    raw[3, off:off + 2] = np.array([np.inf if fmt == "iq4_nl" else np.nan], np.float16).view(np.uint8)
    w[key] = type(bad)(raw, bad.shape)
    with pytest.raises(RcaError, match=r"model\.layers\.1\.mlp\.down_proj\.weight.*" + fmt.upper() + r" block's d is not finite"):
        _from_weights(cfg, w)
