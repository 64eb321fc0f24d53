"""GPU: the fused first layer with conv_in on the matrix pipe (conv_first_mfma_kernel) against the VALU conv_in of
conv1d_mfma_kernel (RCA_FUSE_MFMA_IN=0, read per call) and the unfused scalar chain (variant 0).  Layer-1 outputs bit for bit,
codes equal, at shapes that take the new kernel: large batches, ragged and short windows, row edges inside a wave's columns,
rows from several files through an offset table, and a weight set with zero biases and negative conv_in weights."""
import os

import numpy as np
import pytest

from conftest import bench_signal, rich_signal

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip_full(full_codec):
    from realtime_codec_agent_amd.codec import HipCodec
    return HipCodec(*full_codec, device=0)


def _paths(fn):
    """fn() under the new kernel, the old fused kernel and the unfused chain (variant 0)."""
    old = os.environ.get("RCA_FUSE_MFMA_IN")
    try:
        os.environ.pop("RCA_FUSE_MFMA_IN", None)
        new = fn(1)
        os.environ["RCA_FUSE_MFMA_IN"] = "0"
        valu = fn(1)
    finally:
        if old is None:
            os.environ.pop("RCA_FUSE_MFMA_IN", None)
        else:
            os.environ["RCA_FUSE_MFMA_IN"] = old
    return new, valu, fn(0)


def _tap1(hip, x):
    def run(variant):
        hip.set_variant(variant)
        out = hip.encode_tap(x, 1)
        hip.set_variant(1)
        return out
    new, valu, chain = _paths(run)
    assert np.array_equal(new, valu) and np.array_equal(new, chain)
    return new


def test_layer1_bit_exact_wide_batch(hip_full):
    """40 windows of 2 s (10 k wave tiles of 64 x 128): row edges at multiples of 16000 columns."""
    x = np.stack([rich_signal(32000, 300 + b) if b % 2 else bench_signal(32000, 300 + b) for b in range(40)])
    y = _tap1(hip_full, x)
    assert np.abs(y).max() > 0


@pytest.mark.parametrize("T", [320, 320 - 77, 640 + 5])
def test_layer1_bit_exact_short_ragged_rows(hip_full, T):
    """Rows of 160-320 columns (row edges inside every wave's 128 columns; 160 is the shortest row the kernel takes) and lengths
    that are not a multiple of the hop (zero-padded tail inside the last frame)."""
    B = 3400 if T <= 320 else 1700
    x = np.stack([rich_signal(T, 500 + b % 97) for b in range(B)]).astype(np.float32)
    _tap1(hip_full, x)


def test_layer1_zero_biases_negative_conv_in_weights():
    """Zero biases everywhere and conv_in weights all <= 0: signed zeros of conv_in outputs on silent stretches."""
    from realtime_codec_agent_amd.codec import HipCodec
    from realtime_codec_agent_amd.codec_model import CodecConfig, init_codec_weights
    cfg = CodecConfig()
    w = init_codec_weights(cfg, seed=7)
    w = {k: v.copy() for k, v in w.items()}
    for k in w:
        if k.startswith("enc.") and k.endswith(".bias"):
            w[k][:] = 0.0
    w["enc.conv_in.weight"] = -np.abs(w["enc.conv_in.weight"])
    hip = HipCodec(cfg, w, device=0)
    x = np.stack([rich_signal(32000, 700 + b) for b in range(36)])
    x[::3, 5000:21000] = 0.0   # silence: conv_in outputs +0 / -0 from the zero bias
    x[1::3, :] *= -1.0
    _tap1(hip, x)


def test_codes_stereo_windows_bench_shape(hip_full):
    """The bench shape: 256 windows of 32 000 samples of stereo audio through the windowed batch entry point."""
    import torch
    C, chunk, ctx, B = 2, 1600, 32000, 256
    per = B // C
    first = 20
    N = (first + per) * chunk
    audio = torch.from_numpy(np.stack([bench_signal(N, 11), rich_signal(N, 12)])).cuda()
    fpc = hip_full.frames_per_chunk(chunk)
    st = torch.cuda.current_stream().cuda_stream

    def run(variant):
        hip_full.set_variant(variant)
        codes = torch.full((C, per * fpc), -1, dtype=torch.int64, device="cuda")
        hip_full.encode_chunk_range_dev(audio.data_ptr(), C, N, chunk, ctx, B, first, first + per, codes.data_ptr(), codes.shape[1], st)
        torch.cuda.synchronize()
        hip_full.set_variant(1)
        return codes.cpu().numpy()
    new, valu, chain = _paths(run)
    assert new.min() >= 0
    assert np.array_equal(new, valu) and np.array_equal(new, chain)


def test_codes_multi_file_rows(hip_full):
    """Rows of several files through the per-row offset table (as the batch CLI builds them): windows of 2 s that start at
    arbitrary sample offsets of three concatenated files."""
    import torch
    lens = [70000, 45000, 90000]
    audio = np.concatenate([rich_signal(n, 80 + i) for i, n in enumerate(lens)]).astype(np.float32)
    starts = np.cumsum([0] + lens[:-1])
    T, B = 32000, 48
    rng = np.random.default_rng(4)
    f = rng.integers(0, 3, B)
    src_off = np.array([starts[i] + rng.integers(0, lens[i] - T) for i in f], dtype=np.int64)
    n_keep = 100
    dst_off = np.arange(B, dtype=np.int64) * n_keep
    dev = torch.from_numpy(audio).cuda()
    so, do = torch.from_numpy(src_off).cuda(), torch.from_numpy(dst_off).cuda()
    st = torch.cuda.current_stream().cuda_stream

    def run(variant):
        hip_full.set_variant(variant)
        codes = torch.full((B * n_keep,), -1, dtype=torch.int64, device="cuda")
        hip_full.encode_rows_dev(dev.data_ptr(), so.data_ptr(), B, T, n_keep, codes.data_ptr(), do.data_ptr(), audio.size, st)
        torch.cuda.synchronize()
        hip_full.set_variant(1)
        return codes.cpu().numpy()
    new, valu, chain = _paths(run)
    assert new.min() >= 0
    assert np.array_equal(new, valu) and np.array_equal(new, chain)
    rows = np.stack([audio[o:o + T] for o in src_off])
    assert np.array_equal(new.reshape(B, n_keep), hip_full.encode(rows)[:, -n_keep:])
