"""Sliding-window trim by KV context shift, the parts that need no GPU: the CPU reference of the shift (tests/kv_shift_ref.py)
against keys the oracle computes directly at the new positions, and the agent's shift mode (RealtimeAgent(kv_trim_mode="shift"))
on the fake LM objects of tests/agent_fakes.py."""
import numpy as np
import pytest
import torch

import mp_fakes
from agent_fakes import FakeLLM, build_fakes, scenarios, user_audio
from kv_shift_ref import kv_remove_ref
from oracle import lm_ref
from realtime_codec_agent_amd.llm import LMConfig
from realtime_codec_agent_amd.realtime_agent_config import RealtimeAgentConfig
from realtime_codec_agent_amd.realtime_agent_v2 import RealtimeAgent


# ------------------------------------------------------------------ the reference itself: direction and pairing
def _small_weights(cfg, seed):
    rng = np.random.default_rng(seed)
    g = lambda *shape: (rng.standard_normal(shape) * 0.05).astype(np.float32)
    H, F, KVD, Q = cfg.hidden, cfg.ffn, cfg.n_kv_heads * 64, cfg.n_heads * 64
    w = {"model.embed_tokens.weight": g(cfg.vocab_size, H), "lm_head.weight": g(cfg.vocab_size, H), "model.norm.weight": np.ones(H, np.float32)}
    for l in range(cfg.n_layers):
        p = f"model.layers.{l}."
        w.update({p + "self_attn.q_proj.weight": g(Q, H), p + "self_attn.k_proj.weight": g(KVD, H), p + "self_attn.v_proj.weight": g(KVD, H),
                  p + "self_attn.o_proj.weight": g(H, Q), p + "mlp.gate_proj.weight": g(F, H), p + "mlp.up_proj.weight": g(F, H),
                  p + "mlp.down_proj.weight": g(H, F), p + "input_layernorm.weight": np.ones(H, np.float32),
                  p + "post_attention_layernorm.weight": np.ones(H, np.float32)})
    return w


@pytest.mark.parametrize("rope_scaling", ["llama3", None])
def test_shifted_layer0_keys_are_the_keys_of_the_new_positions(rope_scaling):
    """Layer-0 keys depend on token and position only, so the shifted layer-0 keys of the kept tail must be the layer-0 keys of a
    fresh oracle that evaluated header + tail directly -- a statement about the direction of the rotation and the d / d + 32 pairing
    that does not rest on the helper's own convention.  The fresh oracle keeps its cache in f32, so per pair (x1, x2) of radius
    r = hypot(x1, x2) the two sides differ by
      * three f32 angle roundings (position * inv_freq at the old position, at delta, at the new position), each at most half an ulp
        of an angle below n_ctx, i.e. n_ctx * 2^-24 rad (inv_freq <= 1), each displacing the pair by at most r times that;
      * two fp16 roundings (the shifted oracle's cache store, the helper's store), each at most 2^-11 relative per component, i.e.
        at most 2^-11 r.
    A wrong sign or pairing is off by the order of r itself wherever the angle is not small; the last assertion shows the bound
    tells: the tail merely moved, not rotated, misses it by orders of magnitude."""
    n_ctx, n, p0, p1 = 128, 120, 10, 47
    cfg = LMConfig(vocab_size=300, hidden=64, n_layers=2, n_heads=2, n_kv_heads=2, head_dim=64, ffn=128, rope_scaling=rope_scaling)
    w = _small_weights(cfg, 7)
    ids = np.random.default_rng(8).integers(0, cfg.vocab_size, n).tolist()
    shifted = lm_ref.LMRef(cfg, w, kv_dtype=torch.float16)
    direct = lm_ref.LMRef(cfg, w, kv_dtype=None)
    # one token per pass on both sides: the projection of a token is then the same f32 arithmetic whatever sequence it sits in
    shifted.eval(ids, last_only=True, chunk=1)
    moved_only = shifted.k[0][:, p1:].double()
    kv_remove_ref(shifted, p0, p1)
    direct.eval(ids[:p0] + ids[p1:], last_only=True, chunk=1)
    assert shifted.n_tokens == direct.n_tokens == n - (p1 - p0)
    got, want = shifted.k[0][:, p0:].double(), direct.k[0][:, p0:].double()
    assert got.shape == want.shape == (cfg.n_kv_heads, n - p1, 64)
    r = torch.hypot(want[..., :32], want[..., 32:])
    bound = torch.cat((r, r), dim=-1) * (3 * n_ctx * 2.0 ** -24 + 2 * 2.0 ** -11)
    ratio = ((got - want).abs() / bound).max().item()
    print(f"KVSHIFT layer-0 keys, rope_scaling={rope_scaling}: max |d| / bound = {ratio:.3f}")
    assert ratio <= 1.0
    assert torch.equal(shifted.k[0][:, :p0], direct.k[0][:, :p0].to(torch.float16).float())     # the header did not move
    assert ((moved_only - want).abs() / bound).max().item() > 100.0
    # V rows move bit for bit; every layer was cut alike
    for l in range(cfg.n_layers):
        assert shifted.k[l].shape == shifted.v[l].shape == (cfg.n_kv_heads, n - (p1 - p0), 64)
    assert torch.equal(shifted.v[0][:, p0:], direct.v[0][:, p0:].to(torch.float16).float())


def test_reference_edge_cases():
    cfg = LMConfig(vocab_size=300, hidden=64, n_layers=1, n_heads=2, n_kv_heads=1, head_dim=64, ffn=128)
    ref = lm_ref.LMRef(cfg, _small_weights(cfg, 9), kv_dtype=torch.float16)
    ref.eval(list(range(40)), last_only=True)
    k0, v0 = ref.k[0].clone(), ref.v[0].clone()
    kv_remove_ref(ref, 13, 13)                        # no-op
    assert ref.n_tokens == 40 and torch.equal(ref.k[0], k0) and torch.equal(ref.v[0], v0)
    kv_remove_ref(ref, 25, 40)                        # pure truncation
    assert ref.n_tokens == 25 and torch.equal(ref.k[0], k0[:, :25]) and torch.equal(ref.v[0], v0[:, :25])
    with pytest.raises(AssertionError):
        kv_remove_ref(ref, 5, 26)


# ------------------------------------------------------------------ the agent's shift mode on fakes
class ShiftLLM(FakeLLM):
    """FakeLLM with kv_remove (and a make_kv_shadow that only counts: shift mode must never ask for a twin)."""
    twins = 0

    def kv_remove(self, p0, p1):
        assert 0 <= p0 <= p1 <= self.n_tokens
        self.kv = self.kv[:p0] + self.kv[p1:self.n_tokens]
        self.n_tokens = len(self.kv)
        self.log.append(("kv_remove", p0, p1))
        self.on_remove(p0, p1)

    def on_remove(self, p0, p1):
        pass

    def make_kv_shadow(self):
        type(self).twins += 1
        raise AssertionError("a twin was asked for")


def _session(llm_cls, mode, on_remove=None):
    cfg_kw, script, secs = scenarios(build_fakes()[1])["trim"]
    resources, tok = build_fakes(script)
    resources.llm = llm_cls(tok.vocab_size, tok.codec_vocab_start, resources.audio_tokenizer.codebook_size, script)
    agent = RealtimeAgent(resources=resources, config=RealtimeAgentConfig(**cfg_kw), **({} if mode is None else {"kv_trim_mode": mode}))
    if on_remove is not None:
        resources.llm.on_remove = lambda p0, p1: on_remove(agent, p0, p1)
    audio = user_audio(int(secs * 16000))
    cs = agent.chunk_size_samples
    outs = [agent.process_audio(audio[s:s + cs]) for s in range(0, len(audio) - cs + 1, cs)]
    return agent, resources.llm, np.concatenate(outs)


def test_agent_shift_mode_on_fakes():
    ref_agent, ref_llm, ref_out = _session(FakeLLM, None)
    n_trims = round(ref_agent.trim_to_secs / ref_agent.config.trim_by_secs)
    assert n_trims >= 3
    frame_tokens = 2 * ref_agent.chunk_size_frames_per_channel
    assert sum(len(t) > frame_tokens for op, _, t in ref_llm.log[1:] if op == "eval") == n_trims     # the recomputes shift mode avoids

    seen = []
    prev_trim_pos = [None]

    def on_remove(agent, p0, p1):
        csp = agent.context_start_pos
        new_pos = agent.audio_tokens_idx[agent.frames_from_secs(agent.trim_to_secs)]
        old_pos = csp if prev_trim_pos[0] is None else prev_trim_pos[0]
        prev_trim_pos[0] = new_pos
        assert (p0, p1) == (csp, csp + new_pos - old_pos) and p1 > p0
        last_n = 2 if agent._in_audio_mode() else 1
        assert agent.resources.llm.n_tokens == csp + len(agent.input_ids[new_pos:-last_n])
        seen.append((p0, p1))

    ShiftLLM.twins = 0
    agent, llm, out = _session(ShiftLLM, "shift", on_remove)
    assert len(seen) == n_trims and agent.trim_to_secs == ref_agent.trim_to_secs
    assert ShiftLLM.twins == 0 and agent._kv_shadow is None and not agent.kv_shadow_active and agent._shadow() is None
    evals = [t for op, _, t in llm.log if op == "eval"]
    assert max(len(t) for t in evals[1:]) <= frame_tokens                  # nothing but the session prefill is longer than a frame
    # the fake's next token is a function of the cached tokens: the shifted cache holds what the recompute leaves, same session
    assert agent.input_ids == ref_agent.input_ids and agent.audio_tokens_idx == ref_agent.audio_tokens_idx
    assert llm.n_tokens == ref_llm.n_tokens and llm.kv[:llm.n_tokens] == ref_llm.kv[:ref_llm.n_tokens]
    assert np.array_equal(out, ref_out)


class _RemoveOnly(FakeLLM):
    """kv_remove without make_kv_shadow: in the default mode the agent must neither call it nor behave differently"""

    def kv_remove(self, p0, p1):
        raise AssertionError("kv_remove called in the default mode")


@pytest.mark.parametrize("llm_cls,mode", [(_RemoveOnly, None), (_RemoveOnly, "recompute"), (FakeLLM, "shift")])
def test_default_mode_and_lm_objects_without_kv_remove_keep_the_reference_path(llm_cls, mode):
    ref_agent, ref_llm, ref_out = _session(FakeLLM, None)
    agent, llm, out = _session(llm_cls, mode)
    assert agent.kv_trim_mode == (mode or "recompute")
    assert llm.log == ref_llm.log and agent.input_ids == ref_agent.input_ids and np.array_equal(out, ref_out)


def test_unknown_mode_is_refused_and_the_worker_process_gets_the_knob():
    with pytest.raises(ValueError, match="kv_trim_mode"):
        RealtimeAgent(resources=build_fakes()[0], config=RealtimeAgentConfig(use_whisper=False), kv_trim_mode="evict")
    from realtime_codec_agent_amd.realtime_agent_mp import RealtimeAgentMultiprocessing, RealtimeAgentWorkerError
    with pytest.raises(RealtimeAgentWorkerError, match="kv_trim_mode 'evict'"):      # the worker's RealtimeAgent saw the value
        RealtimeAgentMultiprocessing(config=RealtimeAgentConfig(use_whisper=False), resources_factory=mp_fakes.fake_resources, kv_trim_mode="evict")


def test_switching_to_shift_mode_at_a_reset_gives_the_twin_back():
    closed = []

    class Twin:
        def close(self):
            closed.append(self)

    class Both(ShiftLLM):
        def make_kv_shadow(self):
            return Twin()

    resources, tok = build_fakes()
    resources.llm = Both(tok.vocab_size, tok.codec_vocab_start, resources.audio_tokenizer.codebook_size)
    agent = RealtimeAgent(resources=resources, config=RealtimeAgentConfig(use_whisper=False))
    agent._shadow()
    assert agent.kv_shadow_active and not closed
    agent.kv_trim_mode = "shift"
    agent.reset()
    assert not agent.kv_shadow_active and agent._shadow() is None and len(closed) == 1
