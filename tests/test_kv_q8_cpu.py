"""The q8_0 KV cache's host restatement (tests/kv_q8_ref.py) checked on the CPU: the rule's edge cases, the error bound of one
quantise / de-quantise round trip, Q8KVRef against the oracle it extends, and the presence of the new ABI."""
import os
import re

import numpy as np
import pytest
import torch

import kv_q8_ref as kr
import lm_shape_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("rca_lm_set_kv_format", "rca_lm_get_kv_format", "rca_lm_kv_read_q8", "rca_lm_kv_bytes_per_position")


def _ulp16(a):
    a = np.abs(np.asarray(a, np.float16))
    return (np.nextafter(a, np.float16(np.inf)).astype(np.float64) - a.astype(np.float64))


def test_round_trip_error_bound():
    """For every block, |x - deq| <= d / 2 + 127 d 2^-11 + half an fp16 ulp of the result, d = amax / 127:
      * quantisation: q = round(x / d), so |x - q d| <= d / 2 (the f32 roundings of d, 1 / d and x * inv move t = x * inv by at most
        127 * 3 * 2^-24 = 2.3e-5 of a step, four orders below the half step);
      * scale rounding: the stored scale is fp16_rne(d), |d16 - d| <= 2^-11 d while d16 is a normal fp16 number, times |q| <= 127;
      * output rounding: attention multiplies fp16_rne(d16 * q): half an ulp of that result.
    Rows over six decades of magnitude whose scales stay normal in fp16 (d >= 2^-14; the subnormal and underflowing scales have tests
    of their own below)."""
    rng = np.random.default_rng(0)
    rows = (rng.standard_normal((4000, 64)) * 10.0 ** rng.uniform(-1.5, 3.5, (4000, 1))).astype(np.float16)
    q, d16 = kr.quant_rows(rows)
    deq = kr.dequant(q, d16)
    x = rows.astype(np.float64).reshape(-1, 2, 32)
    d = np.abs(x).max(-1, keepdims=True) / 127.0
    assert d.min() >= 2.0 ** -14
    bound = d / 2 + 127 * d * 2.0 ** -11 + _ulp16(deq).reshape(x.shape) / 2
    err = np.abs(x - deq.astype(np.float64).reshape(x.shape))
    print(f"KVQ8 round trip: worst error / bound = {(err / bound).max():.3f}")
    assert (err <= bound).all()
    assert (np.abs(q.astype(np.int32)) <= 127).all() and (np.abs(q.reshape(-1, 32)).max(1) == 127).all()


def test_rule_edge_cases():
    rng = np.random.default_rng(1)
    rows = kr.edge_rows(rng, 8, 3)
    q, d16 = kr.quant_rows(rows)
    deq = kr.dequant(q, d16)
    # all-zero block: q = 0, d16 = 0
    assert not q[0].any() and not d16[0].view(np.uint16).any() and not deq[0].any()
    # amax carried by a negative value: that value is -127, the scale is positive
    assert (q[1, :, 5] == -127).all() and (q[1, :, 37] == -127).all() and (d16[1] > 0).all()
    assert np.array_equal(deq[1, :, 5], (np.float32(-127) * d16[1, :, 0].astype(np.float32)).astype(np.float16))
    # amax = 65504: d = 515.78 is finite in fp16 but rounds UP to 516, and 516 * 127 = 65532 lies above the largest fp16 value's rounding
    # range (65520): by the rule as it stands the two extreme elements de-quantise to +-inf, every other element (|q| <= 126) is finite.
    # Pinned here so that device and reference agree on it; cache rows of a model are nowhere near 65504.
    assert (q[2, :, 3] == 127).all() and (q[2, :, 40] == -127).all() and (d16[2] == np.float16(516.0)).all()
    inf = np.isinf(deq[2].astype(np.float32))
    assert inf[:, 3].all() and inf[:, 40].all() and inf.sum() == 2 * 3
    assert (deq[2, :, 3] > 0).all() and (deq[2, :, 40] < 0).all()
    # ... while amax = 65024 (d16 = 512 exactly) comes back exactly
    r = np.zeros((1, 64), np.float16); r[0, 7] = np.float16(65024.0); r[0, 39] = np.float16(-65024.0)
    assert np.array_equal(kr.fake_quant(r), r)
    # a block whose d underflows in fp16: q is what the rule says, the stored scale is zero, the block de-quantises to zeros
    assert (np.abs(q[3]).reshape(3, 2, 32).max(-1) == 127).all() and not d16[3].view(np.uint16).any() and not deq[3].any()
    # ties go away from zero: t = +-(n + 1/2) exactly -> q = +-(n + 1)
    t = rows[4].astype(np.float64) * 16.0
    assert np.array_equal(np.abs(t) % 1.0 == 0.5, np.abs(t) != 127.0)
    want = np.where(np.abs(t) == 127.0, t, np.sign(t) * (np.abs(t) + 0.5)).astype(np.int8)
    assert np.array_equal(q[4], want)
    assert np.array_equal(d16[4], np.full((3, 2), 0.0625, np.float16))
    # subnormal (but non-zero) scale: values come back as multiples of that scale
    sub = d16[5].astype(np.float32)
    assert (sub > 0).all() and (sub < 2.0 ** -14).all()
    assert np.array_equal(deq[5].reshape(3, 2, 32), (q[5].reshape(3, 2, 32).astype(np.float32) * sub[..., None]).astype(np.float16))


def test_ulp_jitter_moves_by_at_most_one_ulp():
    rng = np.random.default_rng(2)
    rows = (rng.standard_normal((64, 64))).astype(np.float16)
    j = kr.ulp_jitter(rows, rng)
    diff = np.abs(j.astype(np.float64) - rows.astype(np.float64))
    assert (diff <= _ulp16(rows) + 1e-12).all() and (diff > 0).any()


@pytest.mark.parametrize("case", ["g1_fallback", "g4_tile32"])
def test_q8kvref_switched_off_is_lmref(case):
    from oracle import lm_ref
    c = sc.BY_NAME[case]
    w = sc.oracle_weights(c, c.formats[0])
    ids = c.ids()[:40]
    a, b = lm_ref.LMRef(c.config(), w), kr.Q8KVRef(c.config(), w)
    b.kvq8 = False
    la = torch.cat([a.eval(ids[:33]), a.eval(ids[33:35]), a.eval(ids[35:36])])
    lb = torch.cat([b.eval(ids[:33]), b.eval(ids[33:35]), b.eval(ids[35:36])])
    assert torch.equal(la, lb)
    for l in range(c.config().n_layers):
        assert torch.equal(a.k[l], b.k[l]) and torch.equal(a.v[l], b.v[l])
    # switched on it is another model (the guard of the GPU end-to-end test, here for the oracle); layer 0's K rows are the fake-quantised rows of LMRef
    b2 = kr.Q8KVRef(c.config(), w)
    l2 = torch.cat([b2.eval(ids[:33]), b2.eval(ids[33:35]), b2.eval(ids[35:36])])
    assert float((l2 - la).abs().max()) > 0
    assert np.array_equal(b2.k[0].numpy().astype(np.float16), kr.fake_quant(a.k[0].numpy().astype(np.float16)))   # layer 0 sees the same input


def test_new_symbols_are_declared():
    hdr = open(os.path.join(ROOT, "include", "rca.h")).read()
    from realtime_codec_agent_amd import _native
    for s in NEW_SYMBOLS:
        assert re.search(r"\bint\s+" + s + r"\s*\(", hdr), f"{s} is not declared in include/rca.h"
        assert s in _native.ABI_SYMBOLS, f"{s} is not in _native.ABI_SYMBOLS"
    from realtime_codec_agent_amd.llm import KV_FORMATS, LlamaForAlternatingCodeChannels
    assert KV_FORMATS == ("f16", "q8_0")
    for name in ("set_kv_format", "kv_read_q8", "kv_bytes_per_position", "kv_ring_positions"):
        assert callable(getattr(LlamaForAlternatingCodeChannels, name))
    with pytest.raises(ValueError):
        LlamaForAlternatingCodeChannels(model_path="random:x", kv_format="q4_0", device=0)
