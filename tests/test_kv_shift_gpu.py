"""Context shift on the GPU (rca_lm_kv_remove, LlamaForAlternatingCodeChannels.kv_remove, RealtimeAgent(kv_trim_mode="shift")):
the cache rows the call leaves, the logits evaluated on top of a shifted cache against the oracle carrying the same shift
(tests/kv_shift_ref.py), captured graphs across a shift, weight-sharing twins, and the paired HIP / oracle session in shift mode.

Models are 2-layer cases of tests/lm_shape_cases.py with device-generated weights: g4_tile32 (one KV head, G = 4), g2_tile32 (two
KV heads), nctx700 (n_ctx_pad 768 > n_ctx)."""
import functools
import math

import numpy as np
import pytest
import torch

import lm_shape_cases as sc
from conftest import rich_signal
from kv_shift_ref import ShiftOracleLLM, kv_remove_ref
from oracle import lm_ref

pytestmark = pytest.mark.gpu

SAMPLER = dict(top_k=50, top_p=1.0, min_p=0.0, temp=1.0, seed=3)


@functools.lru_cache(maxsize=None)
def _llm(name, n_ctx=None):
    from realtime_codec_agent_amd.llm import LlamaForAlternatingCodeChannels
    c = sc.BY_NAME[name]
    return LlamaForAlternatingCodeChannels(model_path=f"random:{name}", config=c.config(), n_ctx=n_ctx or c.n_ctx, random_seed=c.seed,
                                           init_std=sc.INIT_STD, device=0)


@functools.lru_cache(maxsize=None)
def _weights(name):
    return sc.oracle_weights(sc.BY_NAME[name], "bf16")


def _fresh(name, mfma=True, n_ctx=None):
    llm = _llm(name, n_ctx)
    llm.set_mfma_prefill(mfma)
    llm.set_graphs(True)
    llm.reset()
    return llm


def _table_inv_freq(cfg) -> np.ndarray:
    """inv_freq as lm_common_init derives it for a handle created without a rope.inv_freq tensor (random-init): double arithmetic,
    rounded to f32 once"""
    out = []
    for i in range(32):
        f = 1.0 / math.pow(cfg.rope_theta, (2 * i) / 64.0)
        if cfg.rope_scaling == "llama3":
            low_wl, high_wl = cfg.rope_orig_ctx / cfg.rope_low_freq_factor, cfg.rope_orig_ctx / cfg.rope_high_freq_factor
            wl = 2.0 * math.pi / f
            if wl > low_wl:
                f = f / cfg.rope_factor
            elif wl >= high_wl:
                smooth = (cfg.rope_orig_ctx / wl - cfg.rope_low_freq_factor) / (cfg.rope_high_freq_factor - cfg.rope_low_freq_factor)
                f = (1.0 - smooth) * f / cfg.rope_factor + smooth * f
        out.append(f)
    return np.asarray(out, np.float64).astype(np.float32)


def _ulp16(e: np.ndarray) -> np.ndarray:
    """spacing of fp16 at |e| (subnormal spacing 2^-24 below 2^-14)"""
    k = np.floor(np.log2(np.maximum(np.abs(e), 2.0 ** -14)))
    return 2.0 ** (k - 10)


def _check_rotated(tag, k_before_tail, k_after_tail, cfg, delta):
    """k_before_tail / k_after_tail: fp16 [rows, nkv, 64], the rows that moved, before and after.  The expectation e is the float64
    rotation of the STORED fp16 inputs by the table angle of position `delta` as lm_rope_table_kernel forms it (f32 position times
    f32 inv_freq; cos / sin of that f32 angle).  Bound per element: ulp16(e) / 2 for the one fp16 store, plus (|x1| + |x2|) * 2^-21
    for what the device computes in f32 in front of it: three roundings (two products, one sum) of at most 2^-24 relative on
    terms of at most |x1| + |x2|, and cosf / sinf, good to about 2^-22 absolute: 2^-24 * 3 + 2^-22 < 2^-21."""
    ang = (np.float32(delta) * _table_inv_freq(cfg)).astype(np.float32).astype(np.float64)
    c, s = np.cos(ang), np.sin(ang)
    x1, x2 = k_before_tail[..., :32].astype(np.float64), k_before_tail[..., 32:].astype(np.float64)
    e = np.concatenate((x1 * c + x2 * s, x2 * c - x1 * s), axis=-1)
    mag = np.abs(x1) + np.abs(x2)
    bound = _ulp16(e) / 2 + np.concatenate((mag, mag), axis=-1) * 2.0 ** -21
    d = np.abs(k_after_tail.astype(np.float64) - e)
    ratio = float((d / bound).max())
    print(f"KVSHIFT {tag}: rotated K max |d| / bound = {ratio:.3f} over {d.size} values, max|k| {np.abs(e).max():.3f}")
    assert ratio <= 1.0, (tag, ratio)
    assert float(np.abs(e).max()) > 0.05, tag         # real keys, not an empty cache


def _read_all(llm, n):
    return [llm.kv_read(l, 0, n) for l in range(llm.config.n_layers)]


GEOMETRIES = [
    ("g4_tile32", 900, 20, 21),      # delta = 1: maximal overlap, the tail spans four 256-position slabs
    ("g4_tile32", 900, 7, 44),       # odd delta, unaligned
    ("g4_tile32", 600, 10, 400),     # delta greater than the tail: no overlap
    ("g4_tile32", 300, 0, 100),      # no header
    ("g4_tile32", 520, 256, 512),    # on the split boundaries
    ("g4_tile32", 300, 100, 300),    # pure truncation
    ("g4_tile32", 300, 50, 50),      # no-op
    ("g2_tile32", 900, 20, 21),
    ("g2_tile32", 900, 7, 44),
    ("g2_tile32", 600, 10, 400),
    ("g2_tile32", 300, 0, 100),
    ("g2_tile32", 520, 256, 512),
    ("g2_tile32", 300, 100, 300),
    ("g2_tile32", 300, 50, 50),
    ("nctx700", 700, 5, 130),        # ragged n_ctx_pad, a full cache
]


@pytest.mark.parametrize("name,n,p0,p1", GEOMETRIES, ids=[f"{g[0]}-{g[1]}-{g[2]}-{g[3]}" for g in GEOMETRIES])
def test_cache_contents_after_remove(name, n, p0, p1):
    """prefill n tokens, read every layer's cache, remove [p0, p1), read again: the p0 rows below the cut untouched bit for bit, V
    rows moved bit for bit, K rows the rotation of the moved rows (bound: _check_rotated), n_tokens = n - delta, logits readable"""
    c = sc.BY_NAME[name]
    llm = _fresh(name)
    llm.eval(c.ids().tolist()[:n])
    logits = llm._scores[-1].copy()
    before = _read_all(llm, n)
    llm.kv_remove(p0, p1)
    delta = p1 - p0
    assert llm.n_tokens == n - delta
    assert np.array_equal(llm._scores[-1], logits)     # read from the device again
    after = _read_all(llm, n - delta)
    moved = n - p1
    for l, ((kb, vb), (ka, va)) in enumerate(zip(before, after)):
        assert np.array_equal(ka[:p0].view(np.uint16), kb[:p0].view(np.uint16)), (l, "K rows below the cut")
        assert np.array_equal(va[:p0].view(np.uint16), vb[:p0].view(np.uint16)), (l, "V rows below the cut")
        assert np.array_equal(va[p0:].view(np.uint16), vb[p1:].view(np.uint16)), (l, "moved V rows")
        if delta == 0 or moved == 0:
            assert np.array_equal(ka.view(np.uint16), kb[:n - delta].view(np.uint16)), (l, "nothing moves")
        else:
            _check_rotated(f"{name} n={n} [{p0}, {p1}) layer {l}", kb[p1:], ka[p0:], c.config(), delta)
    if delta == 0 or moved == 0:                        # the rows past the new n_tokens are stale, not rewritten
        tail_now = _read_all(llm, n)
        assert all(np.array_equal(a[0].view(np.uint16), b[0].view(np.uint16)) and np.array_equal(a[1].view(np.uint16), b[1].view(np.uint16))
                   for a, b in zip(tail_now, before))


def test_refused_arguments_touch_nothing():
    from realtime_codec_agent_amd._native import RcaError
    name, n = "g2_tile32", 300
    llm = _fresh(name)
    llm.eval(sc.BY_NAME[name].ids().tolist()[:n])
    before = _read_all(llm, n)
    for p0, p1 in ((60, 50), (10, n + 1), (-1, 20), (-5, -2), (n + 1, n + 1)):
        with pytest.raises(RcaError, match=r"rc=-1"):                    # RCA_ERR_ARG
            llm.kv_remove(p0, p1)
        assert llm.n_tokens == n
    after = _read_all(llm, n)
    assert all(np.array_equal(a[0].view(np.uint16), b[0].view(np.uint16)) and np.array_equal(a[1].view(np.uint16), b[1].view(np.uint16))
               for a, b in zip(after, before))


def _compare(tag, got, want, tol):
    d, b = float(np.abs(got - want).max()), sc.bound(want, tol)
    print(f"KVSHIFT {tag}: max|dlogit| = {d:.3e}, bound {b:.3e} (tol {tol:g}), ratio {d / b:.3f}")
    assert d <= b, (tag, d, b)
    assert got.argmax() == want.argmax(), tag


@pytest.mark.parametrize("mfma", [True, False], ids=["tiles", "exact"])
@pytest.mark.parametrize("name", ["g4_tile32", "g2_tile32", "nctx700"])
def test_logits_on_a_shifted_cache_match_the_oracle_with_the_same_shift(name, mfma):
    """prefill 600, remove [20, 150) (a tail of 450 rows: two slabs, overlapping), then on the shifted cache a 2-token decode pass, a
    40-token prefill and, after a second remove [5, 60) of the already shifted cache (one more fp16 rounding of the surviving keys),
    another decode pass -- each against LMRef carrying the helper-shifted cache, at lm_shape_cases' tolerance of the route that built
    the cache (TOL_TILE with the MFMA prefill tiles, TOL_EXACT on the exact GEMV route)."""
    c = sc.BY_NAME[name]
    ids = c.ids().tolist()
    tol = sc.TOL_TILE if mfma else sc.TOL_EXACT
    llm = _fresh(name, mfma)
    assert llm.prefill_route() == ("tile32" if mfma else "gemv")
    ref = lm_ref.LMRef(c.config(), _weights(name), kv_dtype=torch.float16)
    n = 600
    llm.eval(ids[:n])
    ref.eval(ids[:n], last_only=True)
    llm.kv_remove(20, 150)
    kv_remove_ref(ref, 20, 150)
    assert llm.n_tokens == ref.n_tokens == 470
    tag = f"{name} {'tiles' if mfma else 'exact'}"
    llm.eval(ids[n:n + 2])
    _compare(f"{tag} decode after one remove", llm._scores[-1].copy(), ref.eval(ids[n:n + 2])[-1].numpy(), tol)
    llm.eval(ids[n + 2:n + 42])
    _compare(f"{tag} 40-token prefill after one remove", llm._scores[-1].copy(), ref.eval(ids[n + 2:n + 42], last_only=True)[-1].numpy(), tol)
    llm.kv_remove(5, 60)
    kv_remove_ref(ref, 5, 60)
    assert llm.n_tokens == ref.n_tokens == 457
    llm.eval(ids[n + 42:n + 44])
    _compare(f"{tag} decode after a second remove", llm._scores[-1].copy(), ref.eval(ids[n + 42:n + 44])[-1].numpy(), tol)


@pytest.mark.parametrize("use_frame", [False, True], ids=["step", "frame"])
def test_captured_graphs_stay_valid_across_a_remove(use_frame):
    """n_ctx 1536 (six attention splits): a step / frame at ~800 keys captures the graph of the first context bucket, one at ~1100
    keys the graph of the second; a remove takes the context back below 1024 keys and the next steps replay the first bucket's graph,
    captured before the remove.  Tokens and logits bit-identical to the same sequence with graph replay switched off."""
    name = "g4_tile32"
    c = sc.BY_NAME[name]
    ids = np.random.default_rng(77).integers(0, c.vocab, 1400).tolist()

    def advance(llm, at):
        if use_frame:
            toks = llm.frame(ids[at:at + 2], ids[at + 2:at + 6], -1)
            assert len(toks) == 4
        else:
            toks = [llm.step(ids[at:at + 2])]
        return toks, llm._scores[-1].copy(), llm.n_tokens

    runs = []
    for graphs in (True, False):
        llm = _fresh(name, True, 1536)
        llm.set_graphs(graphs)
        llm.init_sampler_for_generate(**SAMPLER)
        out = []
        llm.eval(ids[:800])
        out.append(advance(llm, 800))
        llm.n_tokens = 800
        llm.eval(ids[800:1100])
        out.append(advance(llm, 1100))
        n = llm.n_tokens
        llm.kv_remove(30, 330)
        assert llm.n_tokens == n - 300 < 1024 - 8
        out.append(advance(llm, 1200))
        out.append(advance(llm, 1210))
        runs.append(out)
    llm.set_graphs(True)
    for (ta, la, na), (tb, lb, nb) in zip(*runs):
        assert ta == tb and na == nb and np.array_equal(la, lb)


def test_remove_on_a_weight_sharing_twin_leaves_the_parent_alone():
    name, n = "g2_tile32", 300
    c = sc.BY_NAME[name]
    parent = _fresh(name)
    parent.eval(c.ids().tolist()[:n])
    before = _read_all(parent, n)
    twin = parent.make_kv_shadow(low_priority=False)
    try:
        twin.copy_kv_from(parent, n)
        twin.n_tokens = n
        twin.kv_remove(10, 60)
        assert twin.n_tokens == n - 50 and parent.n_tokens == n
        for l, (kb, vb) in enumerate(before):
            ka, va = twin.kv_read(l, 0, n - 50)
            assert np.array_equal(ka[:10].view(np.uint16), kb[:10].view(np.uint16)) and np.array_equal(va[:10].view(np.uint16), vb[:10].view(np.uint16))
            assert np.array_equal(va[10:].view(np.uint16), vb[60:].view(np.uint16))
            _check_rotated(f"twin of {name} layer {l} (the owner's RoPE tables)", kb[60:], ka[10:], c.config(), 50)
        after = _read_all(parent, n)
        assert all(np.array_equal(a[0].view(np.uint16), b[0].view(np.uint16)) and np.array_equal(a[1].view(np.uint16), b[1].view(np.uint16))
                   for a, b in zip(after, before))
    finally:
        twin.close()


# ------------------------------------------------------------------ the session (set-up of tests/test_agent_gpu.py::_paired_resources)
def _paired_resources(seed=3):
    """HIP objects and oracle objects over the SAME weights; the oracle LM carries kv_remove (kv_shift_ref.ShiftOracleLLM)"""
    from types import SimpleNamespace
    from agent_fakes import OracleCodecModel
    from oracle.codec import OracleCodec
    from realtime_codec_agent_amd.audio_tokenizer import AudioTokenizer
    from realtime_codec_agent_amd.codec import MagiCodecHIP
    from realtime_codec_agent_amd.codec_model import init_codec_weights, tiny_codec_config
    from realtime_codec_agent_amd.llm import LlamaForAlternatingCodeChannels, LMConfig
    from realtime_codec_agent_amd.tokenizer import CodecTokenizer
    ccfg = tiny_codec_config()
    cw = init_codec_weights(ccfg, seed=0)
    tok = CodecTokenizer(base_vocab_size=512, codebook_size=ccfg.codebook_size)
    lcfg = LMConfig(vocab_size=tok.vocab_size, hidden=256, n_layers=2, n_heads=4, n_kv_heads=2, head_dim=64, ffn=512)
    w = lm_ref.random_weights(lcfg, seed, 0.05)
    head = w["lm_head.weight"].copy()
    head[: tok.codec_vocab_start] = 0          # like a trained codec LM in audio mode: the text rows never win
    head[len(tok):] = 0
    w["lm_head.weight"] = head
    hip = SimpleNamespace(llm=LlamaForAlternatingCodeChannels(config=lcfg, weights=w, n_ctx=2048, device=0), aux_llm=None, tokenizer=tok,
                          audio_tokenizer=AudioTokenizer(codec_model=MagiCodecHIP(ccfg, cw)), whisper_model=None, llm_model_dir="")
    ora = SimpleNamespace(llm=ShiftOracleLLM(lcfg, w, n_ctx=2048), aux_llm=None, tokenizer=tok,
                          audio_tokenizer=AudioTokenizer(codec_model=OracleCodecModel(OracleCodec(ccfg, cw)), device="cpu"),
                          whisper_model=None, llm_model_dir="")
    return hip, ora


@pytest.mark.parametrize("exact_prefill", [True, False])
def test_shift_mode_session_over_hip_objects_equals_shift_mode_session_over_oracle_objects(exact_prefill):
    """The small trimming session of test_agent_gpu.py (greedy sampling, 80 ms frames, 1 s of context trimmed by 0.4 s: several
    trims, the later ones between one-replay frames) with both agents in shift mode: ids exactly equal, PCM bit for bit, same KV
    position, and the HIP agent never built a twin."""
    from realtime_codec_agent_amd.realtime_agent_config import RealtimeAgentConfig
    from realtime_codec_agent_amd.realtime_agent_v2 import RealtimeAgent
    hip, ora = _paired_resources()
    hip.llm.set_mfma_prefill(not exact_prefill)
    cfg = dict(chunk_size_secs=0.08, use_whisper=False, force_trans_after_inactivity_secs=0.0, force_response_after_inactivity_secs=0.0,
               temperature=0.0, max_context_secs=1.0, trim_by_secs=0.4)
    removes = []
    hip_remove = hip.llm.kv_remove
    hip.llm.kv_remove = lambda p0, p1: (removes.append((p0, p1)), hip_remove(p0, p1))[1]
    a_hip = RealtimeAgent(resources=hip, config=RealtimeAgentConfig(**cfg), kv_trim_mode="shift")
    a_ora = RealtimeAgent(resources=ora, config=RealtimeAgentConfig(**cfg), kv_trim_mode="shift")
    assert a_hip.input_ids == a_ora.input_ids
    n = 1280
    sig = rich_signal(n * 36, 21)
    for s in range(0, len(sig), n):
        o_hip = a_hip.process_audio(sig[s:s + n])
        o_ora = a_ora.process_audio(sig[s:s + n])
        assert a_hip.input_ids == a_ora.input_ids, f"token streams diverge in chunk {s // n}"
        assert np.array_equal(o_hip, o_ora), f"emitted PCM differs in chunk {s // n}"
        assert hip.llm.n_tokens == ora.llm.n_tokens
    assert a_hip.trim_to_secs == a_ora.trim_to_secs and a_hip.trim_to_secs >= 0.8      # several trims happened
    assert len(removes) == round(a_hip.trim_to_secs / 0.4) and all(p0 == a_hip.context_start_pos and p1 > p0 for p0, p1 in removes)
    assert a_hip._kv_shadow is None and not a_hip.kv_shadow_active
    assert np.array_equal(a_hip.get_audio_history(), a_ora.get_audio_history())
    assert a_hip.audio_tokens_idx == a_ora.audio_tokens_idx
    trim_pos = a_hip.audio_tokens_idx[a_hip.frames_from_secs(a_hip.trim_to_secs)]
    assert hip.llm.n_tokens == a_hip.context_start_pos + len(a_hip.input_ids[trim_pos:-2])
    d = np.abs(hip.llm._scores[-1] - ora.llm._logits).max()
    print(f"KVSHIFT session: {len(removes)} removes {removes}, one-replay frames {a_hip.duplex_graph_frames}, last-step logits HIP vs oracle max|d| = {d:.2e}")
    assert d < (2e-4 if exact_prefill else 6e-4)                                     # that session's bounds, on the shifted caches
    assert len(set(a_hip.input_ids[a_hip.context_start_pos + 8::2])) > 10           # the agent channel is not stuck on one code
