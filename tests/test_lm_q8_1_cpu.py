"""The q8_1 activation mode's host restatement (tests/lm_q8_1_ref.py) checked against itself and the oracle's quantisers -- no GPU.
The GPU test (test_lm_q8_1_gpu.py) rests on four claims made there: the quantiser follows the stated rule on its edge cases, the
integer product forms equal the plain product of de-quantised weights and fake-quantised activations, guarded inputs exist for
every shape used, and the mode's effect on whole-model logits is as large as EFFECT says."""
import numpy as np
import pytest

import lm_q8_1_ref as R
from oracle import lm_ref, q4k_ref, q8_ref


def test_quantiser_on_planted_blocks():
    """ties go away from zero on both signs, an all-zero block is (0, 0), a negative amax gives -127, a tiny block gets a subnormal
    fp16 scale"""
    x = R.planted_input(np.random.default_rng(1), (2, 192))
    q, d = R.quantize_q8_1(x)
    for r in range(2):
        e = 2.0 ** (-3 - r)
        assert q[r, 0] == 127 and float(d[r, 0]) == e                       # 127 e / 127: the scale is the power of two itself
        t = x[r, 1:32].astype(np.float64) / e                               # exactly +-(n + 1/2)
        assert np.all(np.abs(t) % 1.0 == 0.5)
        assert np.array_equal(q[r, 1:32], (np.sign(t) * (np.abs(t) + 0.5)).astype(np.int8))
        assert not q[r, 32:64].any() and float(d[r, 1]) == 0.0
        assert q[r, 64 + 5] == -127 and np.abs(q[r, 64:96]).max() == 127
        assert 0 < float(d[r, 3]) < 2.0 ** -14                              # below the smallest normal fp16
        assert q[r, 128] == -127 and np.all(np.abs(x[r, 129:160].astype(np.float64) * 64) % 1.0 == 0.5)
        assert np.array_equal(np.abs(q[r, 129:160]), (np.abs(x[r, 129:160].astype(np.float64) * 64) + 0.5).astype(np.int8))
    assert np.array_equal(R.fake_quant_q8_1(np.zeros((1, 64), np.float32)), np.zeros((1, 64), np.float32))
    # the rule is the q8_0 weight rule of the oracle
    y = np.random.default_rng(2).standard_normal((3, 96)).astype(np.float32)
    q0, d0 = q8_ref.quantize_q8_0(y)
    q1, d1 = R.quantize_q8_1(y)
    assert np.array_equal(q0, q1) and np.array_equal(d0, d1)


@pytest.mark.parametrize("fmt", ["q8_0", "q4_k", "q6_k"])
def test_integer_forms_equal_the_dequantised_product(fmt):
    rng = np.random.default_rng(3)
    w = (rng.standard_normal((24, 512)) * 0.05).astype(np.float32)
    W = R.QMat.from_f32(w, fmt)
    deq = {"q8_0": q8_ref.fake_quant, "q4_k": q4k_ref.fake_quant, "q6_k": q4k_ref.fake_quant_q6_k}[fmt](w)
    assert np.array_equal(W.dequantize(), deq)
    x = R.planted_input(rng, (2, 512))
    y, mag = R.gemv_q8_1(W, x)
    want = R.fake_quant_q8_1(x).astype(np.float64) @ deq.astype(np.float64).T
    assert np.all(mag >= np.abs(y) * (1 - 1e-12))
    assert np.abs(y - want).max() <= 1e-12 * mag.max()


def test_block_forms_from_gguf_blocks_match_the_packed_tensors():
    from realtime_codec_agent_amd._native import Q4KBlocks, Q6KBlocks, Q8Blocks
    rng = np.random.default_rng(4)
    w = (rng.standard_normal((8, 256)) * 0.05).astype(np.float32)
    b4 = Q4KBlocks(q4k_ref.pack_blocks(q4k_ref.quantize_q4_k(w)), w.shape)
    b6 = Q6KBlocks(q4k_ref.pack_blocks_q6_k(q4k_ref.quantize_q6_k(w)), w.shape)
    q, d = q8_ref.quantize_q8_0(w)
    raw = np.concatenate([d.reshape(-1, 1).view(np.uint8), q.reshape(-1, 32).view(np.uint8)], axis=1)
    b8 = Q8Blocks(raw, w.shape)
    for b in (b4, b6, b8):
        assert np.array_equal(R.QMat.from_blocks(b).dequantize(), b.dequantize())


SHAPES = sorted({(M, R.STAGE_WIDTHS(R.tap_config(n))[k]) for n in R.TAP_MODELS for k in (0, 2, 4) for M in (1, 2)} | {(1, 256), (2, 256)})


@pytest.mark.parametrize("shape", SHAPES)
def test_guarded_input_reaches_its_guards(shape):
    rng = np.random.default_rng(shape[1] + shape[0])
    pre = (np.ones(shape[1], np.float32), 1e-5)
    x, passes = R.guarded_input(rng, shape, pre)
    print(f"shape {shape}: {passes} passes")
    assert passes <= R.GUARD_PASSES
    bad_t, bad_d, _ = R._violations(x, pre)
    assert not bad_t.any() and not bad_d.any()
    assert 1.5e-3 < R.GUARD_T < 2.5e-3 and 5e-6 < R.GUARD_D < 1e-5


@pytest.mark.parametrize("name", R.WHOLE_CASES)
def test_effect_noise_and_flips_of_the_whole_model_reference(name):
    """Three sizes, in units of max(1, |logit|max), on the GPU test's whole-model cases:
      effect  q8_1 reference against the f32-activation LMRef: ~1e-2, what EFFECT stores;
      noise   the q8_1 reference evaluated with f32 against float64 products while no quantiser decision differs (a 1-token
              eval): ~1e-7, five orders below the effect -- the mode is far above anything arithmetic order can explain;
      flip    the same comparison once ONE activation lands on the other side of a rounding boundary (2 * 127 * 1e-7 per value, tens
              of thousands of values per eval: it happens within a few tokens): the later quantisers see other inputs and the two
              evaluations end up as far apart as two independent quantisations of the model, i.e. about EFFECT, not about the noise.
    Hence no tight whole-model tolerance exists for this mode, and the GPU test bounds the device -- one more evaluation order -- by
    2 x EFFECT from the f32-activation LMRef.  Asserted here: noise <= 1e-3 EFFECT; every evaluation of the q8_1 reference, flipped
    or not, is itself within that GPU bound; a flip never exceeds 2 x EFFECT (two evaluations, each about EFFECT from LMRef)."""
    cfg, ids = R.tap_config(name), R.whole_ids(name)
    w = R.dequantized_weights(name)
    f32 = R.whole_model_logits(lm_ref.LMRef(cfg, w), ids)
    ref32, ref64 = R.LMRefQ81(cfg, w), R.LMRefQ81(cfg, w, f64=True)
    q81, q81_64 = R.whole_model_logits(ref32, ids), R.whole_model_logits(ref64, ids)
    norm = max(1.0, np.abs(f32).max())
    eff, eff64 = np.abs(q81 - f32).max() / norm, np.abs(q81_64 - f32).max() / norm
    flip = np.abs(q81 - q81_64).max() / norm
    ref32.reset(); ref64.reset()
    noise = np.abs(ref32.eval(ids[:1])[-1].numpy() - ref64.eval(ids[:1])[-1].numpy()).max() / norm
    print(f"{name}: effect {eff:.3e} (float64 products {eff64:.3e}; |logit|max {np.abs(f32).max():.2f}), stored {R.EFFECT[name]:.3e}; "
          f"noise {noise:.1e}; f32 against float64 evaluation over the 48 tokens {flip:.3e}")
    assert R.EFFECT[name] > 5e-3
    assert 0.5 * R.EFFECT[name] <= eff <= 2.0 * R.EFFECT[name]
    assert noise <= 1e-3 * R.EFFECT[name]
    assert eff64 <= 2 * R.EFFECT[name]
    assert flip <= 2 * R.EFFECT[name]


def test_lmrefq81_switched_off_is_lmref_bit_for_bit():
    """the per-eval switch for evals the device runs on MFMA tiles (f32 activations): a prompt with q81 = False, then q8_1 decode
    steps on that cache; and masking keys is refused, not ignored"""
    name = R.WHOLE_CASES[0]
    cfg, ids, w = R.tap_config(name), R.whole_ids(name), R.dequantized_weights(name)
    a, b = R.LMRefQ81(cfg, w), lm_ref.LMRef(cfg, w)
    a.q81 = False
    assert np.array_equal(a.eval(ids[:12]).numpy(), b.eval(ids[:12]).numpy())
    a.q81 = True
    assert not np.array_equal(a.eval(ids[12:13]).numpy(), b.eval(ids[12:13]).numpy())
    with pytest.raises(NotImplementedError):
        a.eval(ids[13:14], drop_keys=(0, 2))
