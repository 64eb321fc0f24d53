"""CPU: the bf16-class reference (oracle/codec_bf16_ref.py) the GPU tests of the opt-in bf16 encoder modes are checked against."""
import numpy as np
import torch

from oracle import codec_bf16_ref as R


def _f(bits):
    return np.array(bits, dtype=np.uint32).view(np.float32)


def test_rne_bf16_hand_written_bit_patterns():
    cases = [
        (0x3F800000, 0x3F80),   # 1.0
        (0x3F808000, 0x3F80),   # exact tie, even neighbour below: down
        (0x3F818000, 0x3F82),   # exact tie, even neighbour above: up
        (0x3F808001, 0x3F81),   # just above the tie
        (0x3F807FFF, 0x3F80),   # just below the tie
        (0xBF808000, 0xBF80),   # negative ties: the same magnitude rule
        (0xBF818000, 0xBF82),
        (0xC0490FDB, 0xC049),   # -pi
        (0x3FFF8000, 0x4000),   # tie on an all-ones significand: carries into the next binade (2.0)
        (0x3FFFC000, 0x4000),
        (0x7F7FFFFF, 0x7F80),   # largest f32 rounds to +inf
        (0x00008000, 0x0000),   # subnormal tie to even (zero)
        (0x00018000, 0x0002),   # subnormal tie to even (up)
        (0x0000C000, 0x0001),
        (0x00007FFF, 0x0000),
        (0x007FFFFF, 0x0080),   # largest subnormal carries into the smallest normal
        (0x80008000, 0x8000),   # negative subnormal tie: -0
        (0x00000000, 0x0000),   # +0
        (0x80000000, 0x8000),   # -0
    ]
    got = R.rne_bf16(_f([c[0] for c in cases]))
    assert got.dtype == np.uint16
    for (x, want), g in zip(cases, got):
        assert int(g) == want, f"{x:#010x}: {int(g):#06x} != {want:#06x}"
    assert [int(v) for v in R.trunc_bf16(_f([0x3F81FFFF, 0xBF81FFFF]))] == [0x3F81, 0xBF81]


def test_rne_bf16_equals_torch_round_to_nearest_even():
    rng = np.random.default_rng(0)
    x = (rng.standard_normal(200000) * np.exp2(rng.integers(-140, 120, 200000))).astype(np.float32)
    x = x[np.isfinite(x)]
    want = torch.from_numpy(x).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    assert np.array_equal(R.rne_bf16(x), want)
    assert np.array_equal(R.bf16_to_f32(want), torch.from_numpy(want.view(np.int16)).view(torch.bfloat16).float().numpy())


def test_split_bf16_reconstructs_to_2_pow_minus_17():
    rng = np.random.default_rng(1)
    x = (rng.standard_normal(200000) * np.exp2(rng.integers(-60, 60, 200000))).astype(np.float32)
    hi, lo = R.split_bf16(x)
    assert hi.dtype == np.uint16 and lo.dtype == np.uint16
    assert np.array_equal(hi, R.rne_bf16(x))
    rec = R.bf16_to_f32(hi).astype(np.float64) + R.bf16_to_f32(lo).astype(np.float64)
    rel = np.abs(rec - x) / np.abs(x.astype(np.float64))
    assert rel.max() <= 2.0 ** -17
    # lo is the rounded remainder, so the pair is not the same as rounding twice, and mode 1 keeps hi alone
    assert (lo != 0).mean() > 0.9
    ops = R.operand(x, 3)
    assert np.array_equal(ops[0], hi) and np.array_equal(ops[1], lo) and R.operand(x, 1)[1] is None


def test_store_applies_leaky_relu_in_f32_before_rounding():
    v = np.array([-1.0 - 2.0 ** -9, -3.0, 0.5, -0.0], np.float64)
    slope = 0.1
    hi, lo = R.store(v, True, 3, slope)
    a = R.leaky_f32(v.astype(np.float32), slope)
    assert np.array_equal(a, np.maximum(v.astype(np.float32), v.astype(np.float32) * np.float32(slope)))
    assert np.array_equal(hi, R.split_bf16(a)[0]) and np.array_equal(lo, R.split_bf16(a)[1])
    assert np.array_equal(R.store(v, False, 1, slope)[0], R.rne_bf16(v.astype(np.float32)))


def test_conv_layer_products_and_bound():
    """mode 1 / 3 products on a small layer against a direct loop over (co, ci, tap); the lo*lo term is not included."""
    rng = np.random.default_rng(2)
    layer = dict(cin=3, cout=2, k=4, s=2, pre=True, w=rng.standard_normal((2, 3, 4)).astype(np.float32),
                 b=rng.standard_normal(2).astype(np.float32))
    x = rng.standard_normal((1, 3, 10)).astype(np.float32)
    padL = (4 - 2 + 1) // 2
    for mode in (1, 3):
        xo, wo = R.operand(x, mode), R.operand(layer["w"], mode)
        xh, wh = R.bf16_to_f32(xo[0]).astype(np.float64), R.bf16_to_f32(wo[0]).astype(np.float64)
        xl = R.bf16_to_f32(xo[1]).astype(np.float64) if mode == 3 else 0 * xh
        wl = R.bf16_to_f32(wo[1]).astype(np.float64) if mode == 3 else 0 * wh
        r, absum = R.conv_layer(xo, layer, mode)
        assert r.shape == (1, 2, 5)
        for co in range(2):
            for t in range(5):
                acc, bound = float(layer["b"][co]), abs(float(layer["b"][co]))
                for ci in range(3):
                    for kk in range(4):
                        i = t * 2 + kk - padL
                        if 0 <= i < 10:
                            acc += xh[0, ci, i] * wh[co, ci, kk] + xh[0, ci, i] * wl[co, ci, kk] + xl[0, ci, i] * wh[co, ci, kk]
                            bound += abs((xh[0, ci, i] + xl[0, ci, i]) * (wh[co, ci, kk] + wl[co, ci, kk]))
                assert abs(r[0, co, t] - acc) <= 1e-12 * bound and abs(absum[0, co, t] - bound) <= 1e-12 * bound


def test_reference_without_rounding_equals_the_f32_encoder(tiny_codec):
    """mode 0 (no rounding): every layer equals oracle/codec_ref.py's fp32 encoder to 1e-6 of its scale."""
    from oracle.codec_ref import MagiCodecStyleRef
    cfg, w = tiny_codec
    rng = np.random.default_rng(3)
    pcm = np.stack([rng.standard_normal(3200 - 77) * 0.2, np.full(3200 - 77, 0.7)]).astype(np.float32)
    outs = R.encode(pcm, cfg, w, 0)
    ref = MagiCodecStyleRef(cfg, w)
    h = ref.pad_audio(torch.from_numpy(pcm)).unsqueeze(1)
    with torch.no_grad():
        for li, layer in enumerate(ref.encoder.layers):
            h = layer(h)
            want = h.numpy()
            assert outs[li].shape == want.shape
            assert np.abs(outs[li] - want).max() <= 1e-6 * np.abs(want).max(), li
    # rounding on: the same network to bf16 accuracy, and a different value
    o1, o3 = R.encode(pcm, cfg, w, 1)[-1], R.encode(pcm, cfg, w, 3)[-1]
    scale = np.abs(outs[-1]).max()
    assert 1e-5 * scale < np.abs(o1 - outs[-1]).max() < 5e-2 * scale
    assert np.abs(o3 - outs[-1]).max() < 1e-4 * scale
