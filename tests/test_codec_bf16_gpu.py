"""GPU: the opt-in bf16 encoder modes (rca_codec_set_mfma_mode 1 / 3) layer by layer against a bf16-class CPU reference
(oracle/codec_bf16_ref.py), on the full CodecConfig (the tiny one never takes the blocked pipeline).

Every layer is checked in isolation: it is fed the kernel's OWN stored input and its stored output is compared with the
reference's exact value r of the same products.  Accumulation tolerance, per output element:

    eps = c * 2^-24 * sqrt(K) * (sum |x * w| + |b|)        K = products per output (Cin * k)

    mode 1 stored planes:   hi == rne(leaky(r)); the adjacent bf16 value only where r lies within eps of the rounding midpoint
    mode 3 stored planes:   |hi + lo - leaky(r)| <= 2^-17 |leaky(r)| + eps
    f32 outputs:            |y - r| <= eps

`ratio` below is the observed maximum of |err| / (2^-24 sqrt(K) (sum |x * w| + |b|)) -- for a mode-1 plane the distance from r
to the midpoint the kernel crossed, a lower bound of its error -- measured on an MI355X over the shapes of this file:

    path / mode                         layer 1   layer 2   layer 3   layer 4   conv_out
    blocked, mode 1 (planes / f32)      0.054     0.0283    0.0173    0.00973   0.0631
    blocked, mode 3 (planes / f32)      7.09      1.96      0.826     0.279     0.093
    conv1d_mfma_kernel<1> (f32 taps)    0.227     0.133     0.0805    0.0361    -
    conv1d_mfma_kernel<3> (f32 taps)    0.377     0.203     0.138     0.0705    0.169   (conv_out: RCA_BF16_BLK_SPLIT=0)

(A mode-3 plane's error includes the split's own rounding, up to 2^-17 |v|: on the k4 layer, K = 128, that alone is several
units.)  Mode 1 stored planes differ from rne(r) in at most 3.3e-4 of the elements (layer 3).  C_CAL holds c per (path, mode,
layer): 4x the observed ratio of that layer, rounded down.  The mutation checks show that a reference with a subtly wrong
arithmetic is rejected by the kernels' actual output at these tolerances.
"""
import math
import os

import numpy as np
import pytest
import torch

from conftest import rich_signal
from oracle import codec_bf16_ref as R

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
SPLIT_REL = 2.0 ** -17
MAX_TIE_FRACTION = 1e-3          # mode-1 elements allowed to differ from rne(r) (each within eps of a midpoint)

# c per (path, mode) and encoder layer 1..5 (calibrated, see the module docstring)
C_CAL = {
    ("blk", 1): [0.21, 0.11, 0.069, 0.038, 0.25],
    ("blk", 3): [28.0, 7.8, 3.3, 1.1, 0.37],
    ("fb", 1): [0.9, 0.53, 0.32, 0.14, None],      # (mode 1 never runs conv_out on this kernel at these shapes)
    ("fb", 3): [1.5, 0.81, 0.55, 0.28, 0.67],
}

# B in {1, 3, 9}: n_ct * B not a multiple of 8 (padding workgroups); T = 320 leaves one output column in the k16 layer,
# 641 and 32000 - 77 are not multiples of the hop (zero tail)
SHAPES = [(9, 32000), (3, 32000 - 77), (1, 641), (9, 320)]


def _batch(B, T, seed):
    x = np.stack([rich_signal(T, seed + b) for b in range(B)]).astype(np.float32)
    if B == 9:
        x[7] = 0.0                                   # a silent row, next to ...
        x[8] = 0.85 + 0.1 * x[8]                     # ... a row with a large DC offset (the last row, past the multiple of 8)
    elif B == 3:
        x[2] = -0.9 + 0.05 * x[2]
    return x


def _rows(B):
    """rows the CPU reference is computed for: the first, the last, either side of a multiple of 8"""
    return sorted({0, B - 1} | {r for r in (7, 8) if r < B})


@pytest.fixture(scope="module")
def codec(full_codec):
    from realtime_codec_agent_amd.codec import HipCodec
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    cfg, w = full_codec
    hip = HipCodec(cfg, w, device=0)
    yield hip, cfg, R.encoder_specs(cfg, w)
    hip.set_mfma_mode(0)


class _Env:
    """set environment variables for a block, restore them after"""

    def __init__(self, **kv):
        self.kv, self.old = kv, {}

    def __enter__(self):
        for k, v in self.kv.items():
            self.old[k] = os.environ.get(k)
            os.environ[k] = v

    def __exit__(self, *exc):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


# ---------------------------------------------------------------------------------------------------- comparisons
def _unit(layer, absum):
    return U * math.sqrt(R.products_per_output(layer)) * absum


def _leaky64(v, slope):
    return np.where(v > 0, v, slope * v)


def _act_scale(r, eps, act, slope):
    """d leaky / dv over [r - eps, r + eps]: errors before the activation shrink by `slope` where all of it is negative"""
    return np.where(r + eps < 0, slope, 1.0) if act else np.ones_like(r)


def check_mode1(hi, r, absum, layer, c, act, slope, store_hi=None):
    """Stored mode-1 plane `hi` (bf16 bits) against r.  store_hi(v) -> bf16 bits of the store of an f64 value (monotone in v);
    default the kernels' store.  Returns (violations, differ fraction, band fraction, observed ratio)."""
    if store_hi is None:
        store_hi = lambda v: R.store(v, act, 1, slope)[0]
    unit = _unit(layer, absum)
    eps = c * unit
    kv = R.bf16_to_f32(hi).astype(np.float64)
    ex = R.bf16_to_f32(store_hi(r)).astype(np.float64)
    lo_v = R.bf16_to_f32(store_hi(r - eps)).astype(np.float64)
    hi_v = R.bf16_to_f32(store_hi(r + eps)).astype(np.float64)
    ok = (kv >= lo_v) & (kv <= hi_v)
    differ = kv != ex
    ratio = 0.0
    if differ.any():
        # the kernel's accumulator lay beyond the midpoint between rne(r) and its value: at least this far from r
        a = _leaky64(r, slope) if act else r
        mid = 0.5 * (kv + ex)
        dist = np.abs(a - mid) / _act_scale(r, 0 * r, act, slope)
        ratio = float((dist[differ] / unit[differ]).max())
    return int((~ok).sum()), float(differ.mean()), float((lo_v != hi_v).mean()), ratio


def check_mode3(hi, lo, r, absum, layer, c, act, slope):
    """Stored mode-3 planes against r: |hi + lo - leaky(r)| <= 2^-17 |leaky(r)| + eps.  Returns (violations, observed ratio)."""
    unit = _unit(layer, absum)
    eps = c * unit
    a = _leaky64(r, slope) if act else r
    sc = _act_scale(r, eps, act, slope)
    kv = R.bf16_to_f32(hi).astype(np.float64) + R.bf16_to_f32(lo).astype(np.float64)
    err = np.abs(kv - a)
    return int((err > SPLIT_REL * np.abs(a) + eps * sc).sum()), float((err / (unit * sc)).max())


def check_f32(y, r, absum, layer, c):
    unit = _unit(layer, absum)
    err = np.abs(y.astype(np.float64) - r)
    return int((err > c * unit).sum()), float((err / unit).max())


def _check_planes(mode, planes, r, absum, layer, c, act, slope):
    """(violations, ratio, differ fraction) of stored planes in `mode`"""
    if mode == 1:
        v, differ, _, ratio = check_mode1(planes[0], r, absum, layer, c, act, slope)
        return v, ratio, differ
    v, ratio = check_mode3(planes[0], planes[1], r, absum, layer, c, act, slope)
    return v, ratio, 0.0


def _sel(op, rows):
    return tuple(p[rows] if p is not None else None for p in op)


# ---------------------------------------------------------------------------------------------------- (a) blocked pipeline
@pytest.mark.parametrize("mode", [1, 3])
def test_blocked_pipeline_layer_by_layer(codec, mode):
    """encode()'s blocked bf16 pipeline (conv_bf16_blk_kernel: the fused first layer, WMT = 2 on k10 in mode 1, the split
    variant in mode 3, the f32 conv_out), every stored plane against the reference fed the kernel's own input planes."""
    hip, cfg, specs = codec
    n = len(specs)                     # conv_in, 4 strided layers, conv_out
    slope = cfg.leaky_slope
    cal = C_CAL[("blk", mode)]
    worst = [0.0] * n
    differ_max = [0.0] * n
    try:
        for si, (B, T) in enumerate(SHAPES):
            x = _batch(B, T, 1000 + 17 * si)
            rows = _rows(B)
            hip.set_mfma_mode(0)
            tap0 = hip.encode_tap(x, 0)[rows]            # the oracle-pinned f32 conv_in chain == the fused layer's staged values
            hip.set_mfma_mode(mode)
            x_op = R.store(tap0, specs[1]["pre"], mode, slope)
            for li in range(1, n):
                layer = specs[li]
                r, absum = R.conv_layer(x_op, layer, mode)
                c = cal[li - 1]
                if li + 1 < n:
                    got = _sel(hip.encode_tap_bf16(x, li), rows)
                    v, ratio, differ = _check_planes(mode, got, r, absum, layer, c, specs[li + 1]["pre"], slope)
                    if si == 0 and li == 2:
                        _mutations_blocked(mode, x_op, got, layer, c, specs[li + 1]["pre"], slope)
                    x_op = got
                else:
                    got = hip.encode_tap(x, li)[rows]
                    v, ratio = check_f32(got, r, absum, layer, c)
                    differ = 0.0
                    if si == 0:
                        _mutation_bias_f32(x_op, got, layer, mode, c)
                worst[li] = max(worst[li], ratio)
                differ_max[li] = max(differ_max[li], differ)
                assert v == 0, f"mode {mode} B={B} T={T} layer {li}: {v} elements outside the tolerance (ratio {ratio:.3g}, c {c})"
                if mode == 1:
                    assert differ <= MAX_TIE_FRACTION, (B, T, li, differ)
    finally:
        hip.set_mfma_mode(0)
    for li in range(1, n):
        print(f"blocked mode {mode} layer {li}: observed ratio {worst[li]:.3g}, calibrated c {cal[li - 1]}"
              + (f", exempted tie fraction {differ_max[li]:.2e}" if mode == 1 and li + 1 < n else ""))


def _rejected(what, mode, v):
    print(f"  mutation ({what}, mode {mode}): {v} elements outside the tolerance -> {'rejected' if v else 'NOT rejected'}")
    assert v > 0, f"the {what} mutation passes the mode-{mode} check: the tolerance cannot see it"


def _mutated_layers(layer):
    drop = dict(layer, w=layer["w"].copy())
    drop["w"][:, 5, layer["k"] // 2] = 0.0         # one tap of one input channel
    nob = dict(layer, b=np.zeros_like(layer["b"]))
    return drop, nob


def _mutations_blocked(mode, x_op, got, layer, c, act, slope):
    drop, nob = _mutated_layers(layer)
    for what, lay in (("one tap of one input channel dropped", drop), ("bias omitted", nob)):
        r, absum = R.conv_layer(x_op, lay, mode)
        _rejected(what, mode, _check_planes(mode, got, r, absum, layer, c, act, slope)[0])
    if mode == 1:
        r, absum = R.conv_layer(x_op, layer, 1, w_op=R.operand(layer["w"], 1, rnd=R.trunc_bf16))
        _rejected("truncated weight rounding", mode, check_mode1(got[0], r, absum, layer, c, act, slope)[0])
        r, absum = R.conv_layer(x_op, layer, 1)
        after = lambda v: R.store(R.bf16_to_f32(R.store(v, False, 1, slope)[0]), act, 1, slope)[0]   # round, then LeakyReLU
        _rejected("LeakyReLU after rounding", mode, check_mode1(got[0], r, absum, layer, c, act, slope, store_hi=after)[0])
    else:
        r, absum = R.conv_layer((x_op[0], None), layer, 3)
        _rejected("lo plane dropped", mode, _check_planes(mode, got, r, absum, layer, c, act, slope)[0])


def _mutation_bias_f32(x_op, got, layer, mode, c):
    _, nob = _mutated_layers(layer)
    r, absum = R.conv_layer(x_op, nob, mode)
    _rejected("bias omitted, f32 conv_out", mode, check_f32(got, r, absum, layer, c)[0])


# ---------------------------------------------------------------------------------------------------- (b) fallback kernel
@pytest.mark.parametrize("mode,split0", [(1, False), (3, False), (3, True)])
def test_fallback_kernel_layer_by_layer(codec, mode, split0):
    """encode_tap in modes 1 / 3 runs conv1d_mfma_kernel<BF> on f32 activations (a mid-layer tap never takes the blocked
    pipeline; RCA_BF16_BLK_SPLIT=0 sends all of mode 3 there, conv_out included): tap li against the reference applied to
    tap li - 1 (LeakyReLU in f32, then rounded / split, as the kernel stages it)."""
    hip, cfg, specs = codec
    n = len(specs)
    slope = cfg.leaky_slope
    cal = C_CAL[("fb", mode)]
    worst = [0.0] * n
    last = n if split0 else n - 1        # the conv_out tap takes the blocked pipeline unless it is switched off
    try:
        with _Env(**({"RCA_BF16_BLK_SPLIT": "0"} if split0 else {})):
            hip.set_mfma_mode(0)
            hip.set_mfma_mode(mode)      # RCA_BF16_BLK_SPLIT is read here
        for si, (B, T) in enumerate(SHAPES):
            x = _batch(B, T, 2000 + 17 * si)
            rows = _rows(B)
            prev = hip.encode_tap(x, 0)[rows]
            for li in range(1, last):
                layer = specs[li]
                got = hip.encode_tap(x, li)[rows]
                x_op = R.store(prev, layer["pre"], mode, slope)
                r, absum = R.conv_layer(x_op, layer, mode)
                c = cal[li - 1]
                v, ratio = check_f32(got, r, absum, layer, c)
                worst[li] = max(worst[li], ratio)
                assert v == 0, f"mode {mode} B={B} T={T} layer {li}: {v} elements outside the tolerance (ratio {ratio:.3g}, c {c})"
                if si == 0 and li == 2 and not split0:
                    _mutations_fallback(mode, prev, got, layer, c, slope)
                prev = got
    finally:
        hip.set_mfma_mode(0)
    for li in range(1, last):
        print(f"conv1d_mfma_kernel<{mode}>{' (RCA_BF16_BLK_SPLIT=0)' if split0 else ''} layer {li}: observed ratio {worst[li]:.3g}, "
              f"calibrated c {cal[li - 1]}")


def _mutations_fallback(mode, prev, got, layer, c, slope):
    x_op = R.store(prev, layer["pre"], mode, slope)
    drop, nob = _mutated_layers(layer)
    muts = [("one tap of one input channel dropped", R.conv_layer(x_op, drop, mode)), ("bias omitted", R.conv_layer(x_op, nob, mode))]
    if mode == 1:
        muts.append(("truncated weight rounding", R.conv_layer(x_op, layer, 1, w_op=R.operand(layer["w"], 1, rnd=R.trunc_bf16))))
        after = R.store(R.bf16_to_f32(R.store(prev, False, 1, slope)[0]), layer["pre"], 1, slope)   # round, then LeakyReLU
        muts.append(("LeakyReLU after rounding", R.conv_layer(after, layer, 1)))
    else:
        muts.append(("lo plane dropped", R.conv_layer((x_op[0], None), layer, 3)))
    for what, (r, absum) in muts:
        _rejected(what, mode, check_f32(got, r, absum, layer, c)[0])


# ---------------------------------------------------------------------------------------------------- (c) unfused conv_in
@pytest.mark.parametrize("mode", [1, 3])
def test_unfused_conv_in_planes_bit_exact(codec, mode):
    """RCA_BF16_NO_FUSE_IN=1 (read per call): conv_in_blk_kernel's layer-0 planes == store(mode-0 tap 0) bit for bit, lo
    included (the same f32 chain, LeakyReLU, rne / split); the unfused k4 instantiation of layer 1 is then checked like (a)."""
    hip, cfg, specs = codec
    slope = cfg.leaky_slope
    try:
        for si, (B, T) in enumerate(SHAPES):
            x = _batch(B, T, 3000 + 17 * si)
            hip.set_mfma_mode(0)
            tap0 = hip.encode_tap(x, 0)
            hip.set_mfma_mode(mode)
            with _Env(RCA_BF16_NO_FUSE_IN="1"):
                got0 = hip.encode_tap_bf16(x, 0)
                got1 = hip.encode_tap_bf16(x, 1)
            want = R.store(tap0, specs[1]["pre"], mode, slope)
            assert np.array_equal(got0[0], want[0]), (B, T, int((got0[0] != want[0]).sum()))
            if mode == 3:
                assert np.array_equal(got0[1], want[1]), (B, T, int((got0[1] != want[1]).sum()))
            rows = _rows(B)
            r, absum = R.conv_layer(_sel(got0, rows), specs[1], mode)
            v, ratio, differ = _check_planes(mode, _sel(got1, rows), r, absum, specs[1], C_CAL[("blk", mode)][0], specs[2]["pre"], slope)
            print(f"unfused layer 1, mode {mode}, B={B} T={T}: observed ratio {ratio:.3g}, differ {differ:.2e}")
            assert v == 0 and differ <= MAX_TIE_FRACTION, (B, T, v, ratio, differ)
            # the fused first layer is not materialised: no layer-0 planes to copy
            with pytest.raises(Exception, match="not materialised"):
                hip.encode_tap_bf16(x, 0)
    finally:
        hip.set_mfma_mode(0)


def test_encode_tap_bf16_refuses_what_encode_does_not_run(codec):
    """RCA_ERR_ARG, never a different pipeline: mode 0, the scalar-chain variant, the split pipeline switched off, the f32 last layer"""
    hip, cfg, specs = codec
    x = _batch(1, 3200, 7)
    try:
        hip.set_mfma_mode(0)
        with pytest.raises(Exception, match="blocked bf16 pipeline"):
            hip.encode_tap_bf16(x, 2)
        hip.set_mfma_mode(1)
        assert hip.encode_tap_bf16(x, 2)[0].shape == (1, cfg.channels[2], 3200 // 8)
        with pytest.raises(Exception, match="out of range"):
            hip.encode_tap_bf16(x, cfg.n_stages + 1)
        hip.set_variant(0)
        try:
            with pytest.raises(Exception, match="blocked bf16 pipeline"):
                hip.encode_tap_bf16(x, 2)
        finally:
            hip.set_variant(1)
        with _Env(RCA_BF16_BLK_SPLIT="0"):
            hip.set_mfma_mode(0)
            hip.set_mfma_mode(3)
        with pytest.raises(Exception, match="blocked bf16 pipeline"):
            hip.encode_tap_bf16(x, 2)
    finally:
        hip.set_mfma_mode(0)


# ---------------------------------------------------------------------------------------------------- (d) code ids
def _stream():
    return torch.cuda.current_stream().cuda_stream


@pytest.mark.parametrize("mode", [1, 3])
def test_code_ids_follow_the_kernels_latent(codec, mode):
    """encode() == quantize_dev(the kernel's own conv_out tap as [B*F, D] rows) == encoder_dev -> quantize_dev (the reference's
    three-step call path): pins the OUT = 1 hand-off to in_proj and the search (the f32 quantiser the mode-0 tests pin)."""
    hip, cfg, specs = codec
    D = cfg.latent_dim
    try:
        hip.set_mfma_mode(mode)
        for si, (B, T) in enumerate(SHAPES):
            x = _batch(B, T, 4000 + 17 * si)
            F = hip.num_frames(T)
            codes = hip.encode(x)
            ze = hip.encode_tap(x, cfg.n_stages + 1)                       # [B, D, F]
            rows = torch.from_numpy(np.ascontiguousarray(ze.transpose(0, 2, 1).reshape(B * F, D))).cuda()
            q1 = torch.full((B * F,), -1, dtype=torch.int64, device="cuda")
            hip.quantize_dev(rows.data_ptr(), B * F, q1.data_ptr(), _stream())
            xd = torch.from_numpy(x).cuda()
            ze_d = torch.empty((B, F, D), dtype=torch.float32, device="cuda")
            hip.encoder_dev(xd.data_ptr(), B, T, ze_d.data_ptr(), _stream())
            q2 = torch.full((B * F,), -1, dtype=torch.int64, device="cuda")
            hip.quantize_dev(ze_d.data_ptr(), B * F, q2.data_ptr(), _stream())
            torch.cuda.synchronize()
            assert np.array_equal(ze_d.cpu().numpy(), ze.transpose(0, 2, 1)), (B, T)
            assert np.array_equal(q1.cpu().numpy().reshape(B, F), codes), (B, T)
            assert np.array_equal(q2.cpu().numpy().reshape(B, F), codes), (B, T)
    finally:
        hip.set_mfma_mode(0)


# ---------------------------------------------------------------------------------------------------- (e) entry points
@pytest.mark.parametrize("mode", [1, 3])
def test_entry_points_agree_at_bench_shape(codec, mode):
    """Stereo audio cut into windows of 2 s context at a 0.1 s hop, 256 rows per pass (the bench's step): encode_windows_dev,
    encode_chunk_range_dev and encode_rows_dev give the ids of encode() on the materialised windows, bit for bit."""
    hip, cfg, specs = codec
    chunk, ctx, per_pass = 1600, 32000, 256
    C = 2
    first = (ctx + chunk - 1) // chunk - 1                  # first chunk whose window is full: 19 warm-up windows before it
    n_chunks = first + per_pass // C                        # then one full pass of 128 chunks x 2 channels
    N = n_chunks * chunk
    audio = np.stack([rich_signal(N, 5100 + c) for c in range(C)]).astype(np.float32)
    fpc = hip.frames_per_chunk(chunk)
    try:
        hip.set_mfma_mode(mode)
        want = np.empty((C, n_chunks * fpc), np.int64)
        for i in range(first):                               # warm-up windows: [0, end)
            want[:, i * fpc:(i + 1) * fpc] = hip.encode(audio[:, :(i + 1) * chunk])[:, -fpc:]
        wins = np.stack([audio[c, (i + 1) * chunk - ctx:(i + 1) * chunk] for i in range(first, n_chunks) for c in range(C)])
        full = hip.encode(wins)[:, -fpc:].reshape(n_chunks - first, C, fpc)
        for k, i in enumerate(range(first, n_chunks)):
            want[:, i * fpc:(i + 1) * fpc] = full[k]
        dev = torch.from_numpy(audio).cuda()
        out = torch.full((C, n_chunks * fpc), -1, dtype=torch.int64, device="cuda")
        hip.encode_windows_dev(dev.data_ptr(), C, N, chunk, ctx, per_pass, out.data_ptr(), n_chunks * fpc, _stream())
        rng_out = torch.full((C, (n_chunks - first) * fpc), -1, dtype=torch.int64, device="cuda")
        hip.encode_chunk_range_dev(dev.data_ptr(), C, N, chunk, ctx, per_pass, first, n_chunks, rng_out.data_ptr(),
                                   rng_out.shape[1], _stream())
        src = torch.tensor([c * N + (i + 1) * chunk - ctx for i in range(first, n_chunks) for c in range(C)], dtype=torch.int64, device="cuda")
        dst = torch.tensor([c * n_chunks * fpc + i * fpc for i in range(first, n_chunks) for c in range(C)], dtype=torch.int64, device="cuda")
        rows_out = torch.full((C, n_chunks * fpc), -1, dtype=torch.int64, device="cuda")
        hip.encode_rows_dev(dev.data_ptr(), src.data_ptr(), len(src), ctx, fpc, rows_out.data_ptr(), dst.data_ptr(), C * N, _stream())
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        assert np.array_equal(got, want), int((got != want).sum())
        assert np.array_equal(rng_out.cpu().numpy(), want[:, first * fpc:])
        assert np.array_equal(rows_out.cpu().numpy()[:, first * fpc:], want[:, first * fpc:])
    finally:
        hip.set_mfma_mode(0)
