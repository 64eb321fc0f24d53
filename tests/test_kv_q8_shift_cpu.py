"""The context shift on a q8_0 KV cache without a GPU (tests/kv_q8_shift_ref.py): the reference against its own bound, the bound
against three mutants on the rows the GPU test plants, the properties of the contract, and the public surface.
The surface tests fail on a tree without rca_lm_set_kv_shift_requant."""
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest

import kv_q8_ref as kr
import kv_q8_shift_ref as qs
import lm_shape_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DELTAS = (1, 7, 255, 256, 1000)
# (name, n, p0, p1) with rows to move, of tests/test_kv_shift_gpu.py::GEOMETRIES, as tests/test_kv_q8_shift_gpu.py uses them
GPU_GEOMETRIES = [(900, 20, 21), (900, 7, 44), (600, 10, 400), (300, 0, 100), (520, 256, 512)]


def _inv_freq(name="g4_tile32"):
    return qs.table_inv_freq(sc.BY_NAME[name].config())


def _blocks(rows):
    return kr.quant_rows(rows)


def _rows(seed, scale):
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((40, 2, 64)) * scale).astype(np.float16)
    x[:5] = kr.edge_rows(rng, 6, 2)[[0, 1, 3, 4, 5]]
    return x


@pytest.mark.parametrize("scale", [1.0, 30.0])
@pytest.mark.parametrize("delta", DELTAS)
def test_reference_is_inside_its_own_bound(delta, scale):
    """edge_rows classes 0, 1, 3, 4, 5 and normal rows: |dequant(shift_rows_ref) - float64 rotation| / bound <= 1, and the bound is
    not slack by more than the quantiser step allows (the worst ratio is above 0.25: half a step alone reaches about 1 / 2)"""
    q, d = _blocks(_rows(11 + delta, scale))
    nq, nd = qs.shift_rows_ref(q, d, delta, _inv_freq())
    ratio = qs.worst_ratio(nq, nd, q, d, delta, _inv_freq())
    assert 0.25 < ratio <= 1.0, ratio


@pytest.mark.parametrize("n,p0,p1", GPU_GEOMETRIES)
def test_bound_catches_the_three_mutants_on_the_planted_rows(n, p0, p1):
    """the rows tests/test_kv_q8_shift_gpu.py plants (kv_q8_shift_ref.planted_rows, same seed), at its geometries: the reference is
    inside the bound; with the two scales of a head swapped, rotated by +delta, or with one amax over the head row it is outside.
    The last mutant differs from the rule only where a row's two blocks end with different scales, which the lopsided rows keep
    through a rotation by a few positions only (their pairs turn by delta * inv_freq[24..31]): it must be outside at delta <= 37 and
    is caught at every delta by the full-scale check below."""
    inv_freq = _inv_freq()
    delta = p1 - p0
    rows = qs.planted_rows(np.random.default_rng(2026), n, 1)[p1:]
    q, d = _blocks(rows)
    assert qs.worst_ratio(*qs.shift_rows_ref(q, d, delta, inv_freq), q, d, delta, inv_freq) <= 1.0
    assert qs.worst_ratio(*qs.mutant_swapped_scales(q, d, delta, inv_freq), q, d, delta, inv_freq) > 1.0
    assert qs.worst_ratio(*qs.mutant_wrong_sign(q, d, delta, inv_freq), q, d, delta, inv_freq) > 1.0
    mq, md = qs.mutant_one_amax(q, d, delta, inv_freq)
    if delta <= 37:
        assert qs.worst_ratio(mq, md, q, d, delta, inv_freq) > 1.0
    live = md.view(np.uint16).reshape(-1) != 0
    peak = np.abs(mq.reshape(-1, 32).astype(np.int32)).max(-1)
    assert (peak[live] < 127).any(), "one amax over the head row leaves a block short of full scale"


@pytest.mark.parametrize("delta", DELTAS)
def test_every_live_block_is_at_full_scale(delta):
    q, d = _blocks(_rows(5, 1.0))
    nq, nd = qs.shift_rows_ref(q, d, delta, _inv_freq())
    live = nd.view(np.uint16).reshape(-1) != 0
    peak = np.abs(nq.reshape(-1, 32).astype(np.int32)).max(-1)
    assert live.any() and (peak[live] == 127).all()


def test_v_blocks_are_untouched_and_the_cut_is_the_fp16_cut():
    """kv_remove_q8_ref on a Q8KVRef-shaped cache: V columns moved as they are, K columns below p0 kept, the tail's K = fake-quantised
    rotation"""
    import torch
    kq, kd = kr.quant_rows(np.ascontiguousarray(_rows(9, 1.0).transpose(1, 0, 2)))      # [nkv, T, ...]
    rows = kr.dequant(kq, kd)
    vrows = kr.fake_quant(_rows(10, 30.0)).transpose(1, 0, 2)
    ref = SimpleNamespace(n_tokens=40, cfg=SimpleNamespace(n_layers=1), inv_freq=torch.from_numpy(_inv_freq()),
                          k=[torch.from_numpy(rows.astype(np.float32))], v=[torch.from_numpy(vrows.astype(np.float32))])
    qs.kv_remove_q8_ref(ref, 6, 13)
    assert ref.n_tokens == 33
    assert np.array_equal(ref.v[0].numpy(), np.concatenate((vrows[:, :6], vrows[:, 13:]), 1).astype(np.float32))
    assert np.array_equal(ref.k[0][:, :6].numpy(), rows[:, :6].astype(np.float32))
    want = kr.dequant(*qs.shift_rows_ref(np.ascontiguousarray(kq[:, 13:]), np.ascontiguousarray(kd[:, 13:]), 7, _inv_freq()))
    assert np.array_equal(ref.k[0][:, 6:].numpy(), want.astype(np.float32))


def test_invariant_after_two_shifts():
    """cache row == Q8(an fp16 row) after any number of shifts: the reference keeps that row (rotated_rows)"""
    inv_freq = _inv_freq()
    q, d = _blocks(_rows(21, 1.0))
    for delta in (37, 256):
        y = qs.rotated_rows(q, d, delta, inv_freq)
        nq, nd = qs.shift_rows_ref(q, d, delta, inv_freq)
        wq, wd = kr.quant_rows(y)
        assert y.dtype == np.float16 and np.array_equal(nq, wq) and np.array_equal(nd.view(np.uint16), wd.view(np.uint16))
        q, d = nq, nd


# ------------------------------------------------------------------ surface
def test_header_and_binding_declare_the_switch():
    from realtime_codec_agent_amd import _native
    header = open(os.path.join(ROOT, "include", "rca.h")).read()
    assert re.search(r"int rca_lm_set_kv_shift_requant\(rca_lm_t\* h, int32_t on\);", header)
    assert re.search(r"int rca_lm_get_kv_shift_requant\(const rca_lm_t\* h, int32_t\* on\);", header)
    assert {"rca_lm_set_kv_shift_requant", "rca_lm_get_kv_shift_requant"} <= set(_native.ABI_SYMBOLS)


def test_python_surface():
    import inspect
    from realtime_codec_agent_amd.llm import LlamaForAlternatingCodeChannels as L
    from realtime_codec_agent_amd.realtime_agent_resources import RealtimeAgentResources
    assert callable(L.set_kv_shift_requant) and isinstance(L.kv_shift_requant, property)
    assert "kv_shift_requant" in inspect.signature(L.__init__).parameters
    assert "llm_kv_shift_requant" in inspect.signature(RealtimeAgentResources.__init__).parameters
    for kv_format in (None, "f16"):
        with pytest.raises(ValueError, match="kv_shift_requant"):
            L(model_path="random:x", kv_format=kv_format, kv_shift_requant=True)       # refused before any device is asked for


def _fake_q8_resources(requant):
    """the fake objects of tests/agent_fakes.py, their LM marked as a q8_0 one"""
    from agent_fakes import build_fakes
    resources = build_fakes()[0]
    resources.llm.kv_format = "q8_0"
    if requant is not None:
        resources.llm.kv_shift_requant = requant
    return resources


@pytest.mark.parametrize("requant", [None, False])
def test_agent_refuses_shift_mode_over_a_q8_cache_without_the_switch(requant):
    from realtime_codec_agent_amd.realtime_agent_config import RealtimeAgentConfig
    from realtime_codec_agent_amd.realtime_agent_v2 import RealtimeAgent
    with pytest.raises(ValueError, match="q8_0") as e:
        RealtimeAgent(resources=_fake_q8_resources(requant), config=RealtimeAgentConfig(use_whisper=False), kv_trim_mode="shift")
    assert "kv_shift_requant" in str(e.value)


def test_agent_accepts_shift_mode_over_a_q8_cache_with_the_switch():
    from realtime_codec_agent_amd.realtime_agent_config import RealtimeAgentConfig
    from realtime_codec_agent_amd.realtime_agent_v2 import RealtimeAgent
    agent = RealtimeAgent(resources=_fake_q8_resources(True), config=RealtimeAgentConfig(use_whisper=False), kv_trim_mode="shift")
    assert agent.kv_trim_mode == "shift" and agent._kv_shadow is None
