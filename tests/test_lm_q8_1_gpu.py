"""activation_format="q8_1": the decode GEMVs over quantised matrices quantise their activations to q8_1 blocks and take integer dot
products (rca_lm_set_act_format, lm_gemv_kernel<..., ACT = 1>).

A whole-model comparison at a tight tolerance means nothing for this mode: one activation on the other side of a rounding boundary
cascades through every later quantiser (test_lm_q8_1_cpu.py measures the mode's effect, the reference's own noise and the
size of such a flip).  So exactness is shown STAGE BY STAGE through
rca_lm_gemv_tap, on inputs where the device's quantiser provably takes the reference's decisions (lm_q8_1_ref.guarded_input for the
stages behind an RMSNorm; planted ties / zero / negative-amax / subnormal-scale blocks for the others), against the integer forms in
float64 and a DERIVED rounding bound: (f32 roundings on a term's path) * 2^-24 * sum |term| (lm_q8_1_ref.gemv_ops).  The mode's
plumbing is checked bit for bit without a reference, the whole model loosely."""
import functools

import numpy as np
import pytest
import torch

import lm_q8_1_ref as R
from oracle import lm_ref

pytestmark = pytest.mark.gpu

KINDS = {0: "qkv", 1: "o", 2: "gate_up", 3: "down", 4: "head"}


def _llm(name, **kw):
    from realtime_codec_agent_amd.llm import LlamaForAlternatingCodeChannels
    fmt, seed = R.TAP_MODELS[name][5], R.TAP_MODELS[name][6]
    args = dict(model_path=f"random:{name}", config=R.tap_config(name), n_ctx=256, random_seed=seed, init_std=R.INIT_STD, device=0,
                weight_format=fmt, activation_format="q8_1")
    args.update(kw)
    return LlamaForAlternatingCodeChannels(**args)


@functools.lru_cache(maxsize=None)
def tap_model(name):
    """(handle in q8_1 mode, StageRef over the same quantised matrices, layer to tap)"""
    if name == "q4_k_m_gguf":
        return _gguf_model()
    w = R.tap_weights(name)
    return _llm(name), R.StageRef(R.tap_config(name), R.LazyMats(w, R.TAP_MODELS[name][5]), R.model_norms(w)), 0


def _gguf_model():
    """A Q4_K_M file of two layers: llama-quantize's mix makes layer 1's attn_v and ffn_down Q6_K beside Q4_K attn_q / attn_k (the V
    projection is a launch of its own with a row base), and the head Q6_K."""
    import tempfile
    import gguf_writer as gw
    from realtime_codec_agent_amd.gguf import load_llama_gguf
    from realtime_codec_agent_amd.llm import LlamaForAlternatingCodeChannels, LMConfig, bf16_bits_to_f32
    g = R.GGUF_MODEL
    cfg = LMConfig(vocab_size=g["vocab_size"], hidden=g["hidden"], n_layers=g["n_layers"], n_heads=g["n_heads"], n_kv_heads=g["n_kv_heads"],
                   head_dim=64, ffn=g["ffn"], rope_scaling=None, rope_theta=10000.0)
    w = lm_ref.random_weights(cfg, g["seed"], 0.05)
    wf = {k: (bf16_bits_to_f32(v) if v.dtype == np.uint16 else v.astype(np.float32)) for k, v in w.items()}
    with tempfile.TemporaryDirectory() as d:
        path = f"{d}/two-layer-q4_k_m.gguf"
        gw.write_llama_gguf(path, cfg, wf, matrix_type="Q4_K_M")
        _, file_w, _ = load_llama_gguf(path)
        kinds = {k: type(v).__name__ for k, v in file_w.items()}
        assert kinds["lm_head.weight"] == "Q6KBlocks" and kinds["model.layers.1.self_attn.v_proj.weight"] == "Q6KBlocks"
        assert kinds["model.layers.1.mlp.down_proj.weight"] == "Q6KBlocks" and kinds["model.layers.1.self_attn.q_proj.weight"] == "Q4KBlocks"
        llm = LlamaForAlternatingCodeChannels(model_path=path, n_ctx=256, device=0, activation_format="q8_1")
    return llm, R.StageRef(cfg, R.LazyMats(file_w), R.model_norms(file_w)), 1


@functools.lru_cache(maxsize=None)
def stage_input(name, kind, M):
    """the stage's input rows and the reference's result for them (computed once, shared by the tests below)"""
    llm, ref, layer = tap_model(name)
    c = ref.cfg
    rng = np.random.default_rng(1000 * kind + 10 * M + len(name))
    K = R.STAGE_WIDTHS(c)[kind]
    if kind in (0, 2, 4):
        p = f"model.layers.{layer}."
        nw = ref.norms[{0: p + "input_layernorm.weight", 2: p + "post_attention_layernorm.weight", 4: "model.norm.weight"}[kind]]
        x, _ = R.guarded_input(rng, (M, K), (nw, c.rms_eps))
    else:
        x = R.planted_input(rng, (M, K), scale=0.3 if kind == 1 else 0.1)
    x.setflags(write=False)
    return x, ref.run(kind, layer, x, pos0=0)


def _ratio(got, want, bound):
    err = np.abs(got.astype(np.float64) - want)
    return float(np.max(np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0))))


ALL_MODELS = tuple(R.TAP_MODELS) + ("q4_k_m_gguf",)


@pytest.mark.parametrize("M", [1, 2])
@pytest.mark.parametrize("kind", sorted(KINDS))
@pytest.mark.parametrize("name", ALL_MODELS)
def test_stage_equals_the_integer_form(name, kind, M):
    """every GEMV stage of the decode step, as the step launches it, within the derived f32 rounding bound of the float64 integer form;
    new K / V rows after the same fp16 rounding, one fp16 ulp allowed"""
    llm, ref, layer = tap_model(name)
    assert llm.activation_format == "q8_1"
    x, want = stage_input(name, kind, M)
    llm.reset()
    got = llm.gemv_tap(layer, kind, x, want_kv=(kind == 0))
    y = got[0] if kind == 0 else got
    r = _ratio(y, want["y"], want["bound"])
    print(f"{name} {KINDS[kind]} M={M}: max err / bound = {r:.3f}  (ops {R.gemv_ops(x.shape[1])}, max|y| {np.abs(want['y']).max():.3f}, "
          f"max bound {want['bound'].max():.3e})")
    assert r <= 1.0
    if kind == 0:
        for nm, rows in (("k", got[1]), ("v", got[2])):
            ok = R.fp16_within_one_ulp(rows, want[nm], want[nm + "_bound"])
            assert ok.all(), f"{nm} rows: {np.count_nonzero(~ok)} values off by more than one fp16 ulp"


@pytest.mark.parametrize("name", ALL_MODELS)
def test_f32_activations_are_not_the_integer_form(name):
    """the same tap with activation_format="f32" is far outside the bound: the stage test cannot pass on f32 activations"""
    llm, ref, layer = tap_model(name)
    worst = 0.0
    try:
        llm.set_activation_format("f32")
        for kind in sorted(KINDS):
            x, want = stage_input(name, kind, 2)
            llm.reset()
            y = llm.gemv_tap(layer, kind, x)
            worst = max(worst, _ratio(y, want["y"], want["bound"]))
    finally:
        llm.set_activation_format("q8_1")
    print(f"{name}: f32-activation tap is {worst:.1f} x the rounding bound from the q8_1 form")
    assert worst > 100.0


# ------------------------------------------------------------------------------------------------------------------ plumbing
def _ids(name, n=24):
    return np.random.default_rng(55).integers(0, R.TAP_MODELS[name][0], n).tolist()


@pytest.mark.parametrize("name", ["h192_q8_0", "h768_q4_k"])
def test_single_steps_pairs_and_the_exact_prefill_route_agree_bit_for_bit(name):
    llm, ids = _llm(name), _ids(name)
    llm.set_mfma_prefill(False)
    outs = []
    for piece in (1, 2, 8):
        llm.reset()
        for i in range(0, 8, piece):
            llm.eval(ids[i:i + piece])
        a = llm._scores[-1].copy()
        llm.eval(ids[8:9])                       # reads every cache row the pieces wrote
        outs.append((a, llm._scores[-1].copy()))
    for a, b in outs[1:]:
        assert np.array_equal(a, outs[0][0]) and np.array_equal(b, outs[0][1])
    llm.reset()
    llm.eval(ids[:20])                           # a longer exact-route eval (GEMV passes of up to 8 tokens) against single steps
    long = llm._scores[-1].copy()
    llm.reset()
    for t in ids[:20]:
        llm.eval([t])
    assert np.array_equal(long, llm._scores[-1])
    llm.close()


def _steps(llm, ids, n_tok):
    llm.reset()
    llm.init_sampler_for_generate(top_k=20, top_p=1.0, min_p=0.0, temp=1.0, seed=3)
    llm.eval(ids[:6])
    toks, cur = [], ids[6:6 + n_tok]
    for s in range(4):
        t = llm.step(cur)
        toks.append(t)
        cur = [t, ids[10 + s]][:n_tok]
    return toks, llm._scores[-1].copy()


def test_graph_replay_frame_and_twin_match_eager_single_steps():
    llm, ids = _llm("h192_q8_0"), _ids("h192_q8_0")
    from realtime_codec_agent_amd.llm import LlamaForAlternatingCodeChannels
    for n_tok in (2, 1):
        llm.set_graphs(False)
        eager = _steps(llm, ids, n_tok)
        llm.set_graphs(True)
        for _ in range(2):                       # the second round replays what the first captured
            graph = _steps(llm, ids, n_tok)
            assert graph[0] == eager[0] and np.array_equal(graph[1], eager[1])
    # rca_lm_frame == the same steps one at a time
    llm.set_graphs(False)
    eager = _steps(llm, ids, 2)
    llm.set_graphs(True)
    llm.reset()
    llm.init_sampler_for_generate(top_k=20, top_p=1.0, min_p=0.0, temp=1.0, seed=3)
    llm.eval(ids[:6])
    assert llm.frame(ids[6:8], ids[10:14], -1) == eager[0] and np.array_equal(llm._scores[-1], eager[1])
    # a twin over the same weights inherits the mode
    twin = LlamaForAlternatingCodeChannels(model_path="random:twin", n_ctx=256, share_weights_with=llm, device=0)
    assert twin.activation_format == "q8_1"
    t = _steps(twin, ids, 2)
    assert t[0] == eager[0] and np.array_equal(t[1], eager[1])
    twin.close()
    llm.close()


def test_switching_modes_on_one_handle_reproduces_each_mode_bit_for_bit():
    name = "h768_q4_k"
    ids = _ids(name)
    plain = _llm(name, activation_format=None)
    assert plain.activation_format == "f32"
    want_f32 = _steps(plain, ids, 2)
    plain.close()
    llm = _llm(name)
    q81 = _steps(llm, ids, 2)                    # captures graphs in q8_1 mode
    assert not np.array_equal(q81[1], want_f32[1])
    llm.set_activation_format("f32")
    got = _steps(llm, ids, 2)
    assert got[0] == want_f32[0] and np.array_equal(got[1], want_f32[1])
    llm.set_activation_format("q8_1")
    again = _steps(llm, ids, 2)
    assert again[0] == q81[0] and np.array_equal(again[1], q81[1])
    with pytest.raises(ValueError):
        llm.set_activation_format("q8_0")
    llm.close()


def test_a_bf16_handle_refuses_the_mode_and_says_why():
    from realtime_codec_agent_amd._native import RcaError
    from realtime_codec_agent_amd.llm import LlamaForAlternatingCodeChannels
    with pytest.raises(ValueError):
        _llm("h192_q8_0", activation_format="int8")
    llm = _llm("h192_q8_0", weight_format=None, activation_format=None)
    assert llm.weight_format == "bf16"
    with pytest.raises(RcaError, match="q8_0 / Q4_K / Q6_K"):
        llm.set_activation_format("q8_1")
    assert llm.activation_format == "f32"
    llm.close()
    with pytest.raises(RcaError, match="q8_0 / Q4_K / Q6_K"):
        LlamaForAlternatingCodeChannels(model_path="random:refused", config=R.tap_config("h192_q8_0"), n_ctx=256, random_seed=1, device=0,
                                        activation_format="q8_1")


# ------------------------------------------------------------------------------------------------------------------ whole model
@pytest.mark.parametrize("name", R.WHOLE_CASES)
def test_whole_model_stays_near_the_f32_reference_and_is_not_a_no_op(name):
    """40-token exact-route prefill + 8 decode steps.  Loose on purpose (see the module docstring): within 2 x EFFECT of the
    f32-activation LMRef -- the q8_1 reference is EFFECT away from it and a cascade can put the device as far from that reference --
    and more than 1e-4 from the device's own f32-activation logits.  Greedy tokens are not compared."""
    cfg, ids = R.tap_config(name), R.whole_ids(name)
    want = R.whole_model_logits(lm_ref.LMRef(cfg, R.dequantized_weights(name), kv_dtype=torch.float16), ids)
    norm = max(1.0, float(np.abs(want).max()))
    got = {}
    llm = _llm(name)
    llm.set_mfma_prefill(False)
    for mode in ("q8_1", "f32"):
        llm.set_activation_format(mode)
        llm.reset()
        llm.eval(ids[:R.WHOLE_PROMPT].tolist())
        rows = [llm._scores[-1].copy()]
        for t in ids[R.WHOLE_PROMPT:]:
            llm.eval([int(t)])
            rows.append(llm._scores[-1].copy())
        got[mode] = np.stack(rows)
    llm.close()
    d_ref = np.abs(got["q8_1"] - want).max() / norm
    d_own = np.abs(got["q8_1"] - got["f32"]).max() / norm
    print(f"{name}: q8_1 device vs f32 LMRef {d_ref:.3e} (bound {2 * R.EFFECT[name]:.3e}); vs the device's f32 mode {d_own:.3e}; "
          f"f32 device vs LMRef {np.abs(got['f32'] - want).max() / norm:.3e}")
    assert d_ref <= 2 * R.EFFECT[name]
    assert d_own > 1e-4
