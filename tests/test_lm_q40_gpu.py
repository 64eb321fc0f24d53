"""GGUF Q4_0 / Q4_1 matrices on the device (WF_Q40 / WF_Q41 in rca_lm.hip): the Q4_K quad layout of the nibbles plus one
(fp16 s | fp16 t << 16) dword per slot and 32 values, value = s q - t, streamed packed by the decode GEMVs (f32 and q8_1 activations) and
de-quantised while staging by the 128-token prefill tiles.

A hand-made matrix is read out EXACTLY first (one-hot inputs); then a Q4_0 / Q4_1 matrix whose factors are constant over 256 values
must be its Q4_K twin, bit for bit, on every path; every GEMV stage is held to the derived rounding bound of the float64 product forms
(tests/q40_ref.py, tests/q5k_ref.py, tests/lm_q8_1_ref.py); files and the load-time quantisers go against LMRef at the project's
tolerances (lm_shape_cases.TOL_EXACT / TOL_TILE)."""
import functools

import numpy as np
import pytest
import torch

import lm_q40_cases as C
import lm_q8_1_ref as R
import lm_shape_cases as sc
import q40_ref
from oracle import lm_ref

pytestmark = pytest.mark.gpu

KINDS = {0: "qkv", 1: "o", 2: "gate_up", 3: "down", 4: "head"}
ACTS = ("f32", "q8_1")
TYPES = ("q4_0", "q4_1")


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
    """Every matrix Q4_0 / Q4_1; layer 0's down_proj [256, 512] hand-made: d a power of two that differs per block and per row parity, of
    both signs; q a function of (row, k) that takes all 16 values at every (row mod 4, k mod 8), i.e. at every nibble of the quad's
    16-byte unit; Q4_1: m a multiple of d, so that d q + m is exact."""
    ttype = q40_ref.KINDS[fmt]
    cfg = _config(**HAND_CFG)
    w = q40_ref.blocks_model(lm_ref.random_weights(cfg, 21, C.INIT_STD), ttype)
    N, K = cfg.hidden, cfg.ffn
    row, k = np.meshgrid(np.arange(N), np.arange(K), indexing="ij")
    q = ((5 * k + 11 * row + 3 * (k >> 3) + (row >> 2)) & 15).astype(np.uint8)
    seen = np.zeros((4, 8, 16), bool)
    seen[row % 4, k % 8, q] = True
    assert seen.all()
    rb, kb = row[:, ::32], k[:, ::32] // 32                                                  # [N, K / 32]
    d = (np.where((kb + rb // 2) % 3 == 0, -1.0, 1.0) * 2.0 ** -(5 + kb % 3 + rb % 2)).astype(np.float16)
    assert (d > 0).any() and (d < 0).any() and len(np.unique(d)) == 8
    p = dict(q=q, d=d)
    if ttype == q40_ref.Q4_1:
        p["m"] = (d.astype(np.float32) * ((7 * kb + rb) % 9 - 4)).astype(np.float16)
    down = q40_ref.block_class(ttype)(q40_ref.pack_blocks(p), (N, K))
    w["model.layers.0.mlp.down_proj.weight"] = down
    values = down.dequantize()
    values.setflags(write=False)
    return _from_weights(cfg, w), down, values


@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("fmt", TYPES)
def test_one_hot_inputs_read_every_weight_of_a_hand_made_matrix(fmt, act):
    """rca_lm_gemv_tap(kind 3) with one-hot rows, two columns per call, all 512 k.
    f32 activations: p = q * 1 (the other products are 0), s q is a 4-bit integer times a power of two and t a small multiple of the same
    power: their difference and every later sum (all other terms are 0) are exact, so y must equal the de-quantised column.
    q8_1 activations: the one-hot row quantises to q_x = 127 and d_x = fp16(1 / 127), and fp16(1 / 127) * 127 is not 1: that path is NOT
    exact for these weights.  It is compared with the integer form in float64 within lm_q8_1_ref.gemv_bound."""
    llm, down, values = _hand_model(fmt)
    llm.set_activation_format(act)
    K = values.shape[1]
    W = q40_ref.qmat(down)
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
            bound = R.gemv_bound(K, mag)
            err = np.abs(y.astype(np.float64) - want)
            assert np.all(err <= bound), k0
            worst = max(worst, float((err / np.where(bound > 0, bound, 1)).max()))
    if act == "q8_1":
        print(f"{fmt} q8_1 one-hot readout: max err / bound = {worst:.3f}")
    llm.set_activation_format("f32")


# ------------------------------------------------------------------------------------------------------------------ 2. the Q4_K twin
@pytest.mark.parametrize("fmt", TYPES)
def test_a_matrix_with_constant_factors_is_its_q4_k_twin_bit_for_bit(fmt):
    """The same values twice (q40_ref.twin_models): as Q4_0 / Q4_1 blocks whose d (and m) is constant over each 256 values, and as Q4_K
    blocks with sc = 1, m = 8, d = dmin = d0 (resp. m = 1, dmin = -m0).  40-token evals on both prefill routes and two graph steps give
    the same logits bit for bit, with f32 and with q8_1 activations in the decode GEMVs: the new body's arithmetic is the Q4_K body's."""
    cfg = _config(1024, 256, 4, 2, 512)
    wa, wb = q40_ref.twin_models(cfg, 23, q40_ref.KINDS[fmt])
    a, b = _from_weights(cfg, wa), _from_weights(cfg, wb)
    assert (a.weight_format, b.weight_format) == (fmt, "q4_k")
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
# the three shapes of test_lm_q5k_gpu.py: name -> (vocab, hidden, heads, kv heads, ffn, seed)
#   k256:  K = 256: 32 chunks, 8 per wave; a head of 1004 rows: a multiple of 4 but not of 16, the last group of 16 factor slots is ragged
#   k768:  K = 3 x 256 (not a power of two), G = 4
#   k1024: ffn 6144 = the NIT = 4 instance of the down projection with a short last chunk
STAGE_MODELS = {"k256": (1004, 256, 4, 2, 512, 51), "k768": (1536, 768, 12, 3, 768, 39), "k1024": (2048, 1024, 16, 16, 6144, 37)}


class _LazyQ40:
    """HF name -> QMat of the matrix's Q4_0 / Q4_1 blocks by the numpy rule, built on first use"""

    def __init__(self, weights, ttype):
        self.weights, self.ttype, self.done = weights, ttype, {}

    def __getitem__(self, k):
        if k not in self.done:
            self.done[k] = q40_ref.qmat(q40_ref.to_blocks(self.weights[k], self.ttype))
        return self.done[k]


@functools.lru_cache(maxsize=None)
def _stage_model(name, fmt):
    v, h, nh, nkv, f, seed = STAGE_MODELS[name]
    cfg = _config(v, h, nh, nkv, f)
    w = lm_ref.random_weights(cfg, seed, C.INIT_STD)
    mats, norms = _LazyQ40(w, q40_ref.KINDS[fmt]), R.model_norms(w)
    return _random(name, cfg, seed, fmt), {"q8_1": R.StageRef(cfg, mats, norms), "f32": q40_ref.stage_ref_f32(cfg, mats, norms)}


@functools.lru_cache(maxsize=None)
def _stage_input(name, kind, M):
    llm, refs = _stage_model(name, "q4_0")     # the input depends on the norm weights (all ones) and the shape only
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
@pytest.mark.parametrize("fmt", TYPES)
def test_stage_is_within_the_rounding_bound_of_its_float64_form(fmt, name, kind, act, M):
    """Every GEMV stage of the decode step, as the step launches it, on Q4_0 / Q4_1 matrices quantised on the device: within the derived
    f32 rounding bound of the float64 form over the numpy-quantised blocks -- f32 activations: q40_ref.gemv_f32 with
    q5k_ref.gemv_f32_bound; q8_1: the integer form and bound of lm_q8_1_ref -- and the new K / V rows after the same fp16 rounding, one
    fp16 ulp allowed."""
    llm, refs = _stage_model(name, fmt)
    x = _stage_input(name, kind, M)
    want = refs[act].run(kind, 0, x, pos0=0)
    llm.set_activation_format(act)
    llm.reset()
    got = llm.gemv_tap(0, kind, x, want_kv=(kind == 0))
    llm.set_activation_format("f32")
    y = got[0] if kind == 0 else got
    err = np.abs(y.astype(np.float64) - want["y"])
    r = float(np.max(np.where(want["bound"] > 0, err / np.where(want["bound"] > 0, want["bound"], 1.0), np.where(err > 0, np.inf, 0.0))))
    print(f"{fmt} {name} {KINDS[kind]} {act} M={M}: max err / bound = {r:.3f} (max|y| {np.abs(want['y']).max():.3f}, max bound {want['bound'].max():.3e})")
    assert r <= 1.0
    if kind == 0:
        for nm, rows in (("k", got[1]), ("v", got[2])):
            ok = R.fp16_within_one_ulp(rows, want[nm], want[nm + "_bound"])
            assert ok.all(), f"{nm} rows: {np.count_nonzero(~ok)} values off by more than one fp16 ulp"


# ------------------------------------------------------------------------------------------------------------------ 4. files
@pytest.mark.parametrize("name", sorted(C.FILES))
def test_gguf_files_stay_packed_and_match_their_dequantisation(name, tmp_path):
    """A Q4_0-only file, a Q4_1-only file and the mix a llama-quantize Q4_0 file holds (output.weight Q6_K, layer 0's ffn_down Q4_1 beside
    Q4_0 neighbours) through model_path=.  Logits equal LMRef over the file's own blocks de-quantised on the host, exact route and
    128-token tiles; prefill equals incremental evaluation; a graph step equals the eager one; a twin over the same weights computes the
    same bits; masked head rows read exactly 0 and the others do not move."""
    from realtime_codec_agent_amd.llm import LlamaForAlternatingCodeChannels
    path = str(tmp_path / f"{name}.gguf")
    C.write_file(name, path)
    file_w, want, gap = C.file_oracle(name, path)
    kinds = {type(v).__name__ for k, v in file_w.items() if hasattr(v, "raw")}
    assert kinds == {"q4_0": {"Q40Blocks"}, "q4_1": {"Q41Blocks"}, "q4_0_mix": {"Q40Blocks", "Q41Blocks", "Q6KBlocks"}}[name]
    assert gap > C.gap_needed(want), "the compared position has no clear argmax: pick another seed (tests/lm_q40_cases.py)"
    g = LlamaForAlternatingCodeChannels(model_path=path, n_ctx=512, device=0)
    fmt = "q4_1" if name == "q4_1" else "q4_0"
    assert g.weight_format == fmt
    nbytes = 0
    for k, v in file_w.items():
        if q40_ref.is_projection(k):
            n = int(np.prod(v.shape))
            nbytes += n + n // 4 if type(v).__name__ == "Q6KBlocks" else n // 2 + n // 8      # Q6_K: int8 values + an f32 scale per 16
    assert g.weight_bytes_per_step() == nbytes
    if name == "q4_0_mix":
        assert type(file_w["model.layers.0.mlp.down_proj.weight"]).__name__ == "Q41Blocks"
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
    # decode: a 2-token pass on the exact-route cache, eager eval == graph step; twin
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


# ------------------------------------------------------------------------------------------------------------------ 5. quantisers
QUANT_CASES = ("g4_k768", "g1_gemm128_ffn6144")


@functools.lru_cache(maxsize=None)
def _quantised(name, fmt):
    """(bf16-bit weights of the shape case, the same as host-quantised blocks, their float32 values): one pass of the numpy rule"""
    c = sc.BY_NAME[name]
    src = lm_ref.random_weights(c.config(), c.seed, sc.INIT_STD)
    blocks = q40_ref.blocks_model(src, q40_ref.KINDS[fmt])
    return src, blocks, {k: (v.dequantize() if hasattr(v, "raw") else v) for k, v in blocks.items()}


@pytest.mark.parametrize("fmt", TYPES)
def test_the_device_quantiser_is_the_numpy_rule_block_for_block(fmt):
    """weight_format="q4_0" / "q4_1" over bf16 weights (quantised on the device at load) against the same weights quantised by
    q40_ref.quantize_q4_0 / _q4_1 and supplied as blocks: the same logits bit for bit, prefill tiles, exact route and decode passes."""
    name = "g4_k768"
    c = sc.BY_NAME[name]
    src, blocks, _ = _quantised(name, fmt)
    dev = _from_weights(c.config(), src, weight_format=fmt)
    host = _from_weights(c.config(), blocks)
    assert dev.weight_format == host.weight_format == fmt
    n = sum(int(np.prod(v.shape)) for k, v in src.items() if q40_ref.is_projection(k))
    assert dev.weight_bytes_per_step() == host.weight_bytes_per_step() == n // 2 + n // 8          # nibbles, (s, t): 5.0 bits
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
    dev.close()
    host.close()


@pytest.mark.parametrize("name", QUANT_CASES)
@pytest.mark.parametrize("fmt", TYPES)
def test_load_time_quantisation_matches_oracle_over_the_quantised_model(fmt, name):
    """model_path="random:" with weight_format="q4_0" / "q4_1" at two shapes of lm_shape_cases -- K = 3 x 256 at G = 4, and hidden 1024 /
    ffn 6144 (the NIT = 4 down projection) -- against LMRef over the numpy-quantised model: exact route at TOL_EXACT, the 128-token tiles
    and a decode pass on their cache at TOL_TILE; argmax equal."""
    c = sc.BY_NAME[name]
    ids = c.ids().tolist()
    P = c.prompt
    llm = _random(name, c.config(), c.seed, fmt, n_ctx=c.n_ctx)
    for mfma in (False, True):
        ref = lm_ref.LMRef(c.config(), _quantised(name, fmt)[2], kv_dtype=torch.float16)
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
            print(f"{fmt} {name} {llm.prefill_route()} {what}: max|dlogit| = {d:.3e}, bound {b:.3e} (max|logit| {np.abs(want).max():.2f}), ratio {d / b:.3f}")
            assert d <= b and got.argmax() == want.argmax(), (name, mfma, what)
    llm.close()


# ------------------------------------------------------------------------------------------------------------------ 6. embedding table
def test_an_embedding_table_of_q4_0_rows_is_dequantised_on_the_device_exactly():
    """RCA_Q4_0 is accepted for the embedding table too (the GGUF importer de-quantises it on the host, a C caller need not): the device's
    f32 rows equal the host's de-quantisation, so the logits are the same bits."""
    cfg = _config(1024, 256, 4, 2, 512)
    w = q40_ref.blocks_model(lm_ref.random_weights(cfg, 29, C.INIT_STD), q40_ref.Q4_0)
    rows = q40_ref.to_blocks(w["model.embed_tokens.weight"], q40_ref.Q4_0)
    ids = np.random.default_rng(6).integers(0, 1024, 12).tolist()
    out = []
    for table in (rows, rows.dequantize()):
        llm = _from_weights(cfg, dict(w, **{"model.embed_tokens.weight": table}))
        llm.eval(ids)
        out.append(llm._scores[-1].copy())
        llm.close()
    assert np.array_equal(out[0], out[1]) and np.abs(out[0]).max() > 0


# ------------------------------------------------------------------------------------------------------------------ 7. refusals
def test_shapes_the_layout_cannot_hold_are_refused_by_name():
    from realtime_codec_agent_amd._native import RcaError
    with pytest.raises(RcaError, match="Q4_0 needs rows of a multiple of 256"):
        _random("h192", _config(1000, 192, 3, 3, 320), 1, "q4_0")
    with pytest.raises(RcaError, match=r"Q4_0 weights: lm_head is 1002 x 256 \(K must be a multiple of 256, N of 4\)"):
        _random("v1002", _config(1002, 256, 4, 2, 512), 1, "q4_0")
    with pytest.raises(RcaError, match=r"Q4_1 weights: lm_head is 1002 x 256 \(K must be a multiple of 256, N of 4\)"):
        _random("v1002", _config(1002, 256, 4, 2, 512), 1, "q4_1")
    with pytest.raises(ValueError, match="q4_0"):
        _random("x", _config(1000, 256, 4, 2, 512), 1, "q5_0")
    llm = _random("q81", _config(1024, 256, 4, 2, 512), 1, "q4_0", activation_format="q8_1")      # a Q4_0-only handle counts as packed
    assert llm.weight_format == "q4_0" and llm.activation_format == "q8_1"
    llm.eval([1, 2, 3])
    assert np.isfinite(llm._scores[-1]).all()
    llm.close()


def test_a_q4_0_block_whose_8_d_overflows_fp16_is_refused_with_the_tensors_name():
    from realtime_codec_agent_amd._native import RcaError
    cfg = _config(1024, 256, 4, 2, 512)
    w = q40_ref.blocks_model(lm_ref.random_weights(cfg, 29, C.INIT_STD), q40_ref.Q4_0)
    bad = w["model.layers.1.self_attn.o_proj.weight"]
    raw = bad.raw.copy()
    raw[3, 18:20] = np.array([16384.0], np.float16).view(np.uint8)           # 8 d = 131072 > 65504
    w["model.layers.1.self_attn.o_proj.weight"] = type(bad)(raw, bad.shape)
    with pytest.raises(RcaError, match=r"model\.layers\.1\.self_attn\.o_proj\.weight.*8 d is not finite in fp16"):
        _from_weights(cfg, w)
