"""GPU tests (MI355X) of the kept-frames view of the encoder's last layer: a call that hands the encoder's output straight to the
quantiser with a keep count evaluates the last layer only at the frames it reads (plus the halo column it skips).  Codes are
compared as integer arrays, without tolerance.  The reference is rca_codec_encode_dev on the materialised windows, which always
computes all frames; where the existing tests use it, the CPU oracle is the second reference."""
import numpy as np
import pytest

from conftest import bench_signal, rich_signal

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip_tiny(tiny_codec):
    from realtime_codec_agent_amd.codec import HipCodec
    return HipCodec(*tiny_codec, device=0)


@pytest.fixture(scope="module")
def hip_full(full_codec):
    from realtime_codec_agent_amd.codec import HipCodec
    return HipCodec(*full_codec, device=0)


@pytest.fixture(scope="module")
def odd_pair():
    """the odd-channel config of test_odd_channel_counts_and_big_batches_bit_exact: Cin of the last layer (36) is not a multiple of
    its channel chunk, Cout (24) is narrower than a 32-row tile"""
    from realtime_codec_agent_amd.codec import HipCodec
    from realtime_codec_agent_amd.codec_model import init_codec_weights, tiny_codec_config
    from oracle.codec import OracleCodec
    cfg = tiny_codec_config(channels=(6, 10, 12, 20, 36), latent_dim=24, name="odd")
    w = init_codec_weights(cfg, seed=3)
    return HipCodec(cfg, w, device=0), OracleCodec(cfg, w)


def _audio(C, N, seed):
    return np.stack([bench_signal(N, seed) if c == 0 else rich_signal(N, seed + c) for c in range(C)])


def _reference_windows(hip, audio, chunk, ctx, chunk_begin, chunk_end):
    """Every window [end - max(chunk, ctx), end) materialised and encoded at ALL frames by rca_codec_encode_dev (hip.encode), the
    chunk's own frames kept on the host: windows of one length go through in one batch."""
    Cn, _ = audio.shape
    fpc = hip.frames_per_chunk(chunk)
    W = max(chunk, ctx)
    out = np.empty((Cn, (chunk_end - chunk_begin) * fpc), np.int64)
    by_len = {}
    for i in range(chunk_begin, chunk_end):
        end = (i + 1) * chunk
        by_len.setdefault(end - max(0, end - W), []).append(i)
    for T, idx in by_len.items():
        x = np.concatenate([audio[:, (i + 1) * chunk - T:(i + 1) * chunk] for i in idx])   # rows (window, channel)
        codes = hip.encode(x)
        for n, i in enumerate(idx):
            out[:, (i - chunk_begin) * fpc:(i - chunk_begin + 1) * fpc] = codes[n * Cn:(n + 1) * Cn, -fpc:]
    return out


def _chunk_range(hip, audio, chunk, ctx, batch_windows, chunk_begin, chunk_end):
    import torch
    Cn, N = audio.shape
    fpc = hip.frames_per_chunk(chunk)
    dev = torch.from_numpy(audio).cuda()
    out = torch.full((Cn, (chunk_end - chunk_begin) * fpc), -1, dtype=torch.int64, device="cuda")
    hip.encode_chunk_range_dev(dev.data_ptr(), Cn, N, chunk, ctx, batch_windows, chunk_begin, chunk_end, out.data_ptr(), out.shape[1],
                               torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _conv_flops(hip, fn):
    """FLOPs the conv launches (profile class 0) of fn() report: each launch reports what it executes"""
    hip.profile(True)
    try:
        hip.profile_read(0)
        fn()
        hip.sync()
        return hip.profile_read(0)
    finally:
        hip.profile(False)


@pytest.mark.parametrize("trim", [False, True])
@pytest.mark.parametrize("C", [1, 2])
@pytest.mark.parametrize("chunk,ctx", [(1600, 32000), (1280, 32000), (1600, 960), (1280, 640)])
def test_chunk_range_small_batches_equal_all_frames(chunk, ctx, C, trim, hip_full, full_oracle, monkeypatch):
    """Chunk 1600 (5 kept frames) and 1280 (4), a 2 s context and one shorter than the chunk, mono and stereo, window trim off and
    on, from chunk 0 (so the short warm-up windows, F <= keep + 1 among them, are included), with pass sizes that leave a ragged
    last pass and a ragged last column tile (6 and 37 windows per pass).  Equal to the all-frames reference, to the oracle where
    the window is short enough for it to be quick, and to the same call with RCA_HEAD_KEEP=0."""
    hip_full.set_variant(1)
    n_chunks = 46
    audio = _audio(C, n_chunks * chunk + 123, 3)
    want = _reference_windows(hip_full, audio, chunk, ctx, 0, n_chunks)
    if ctx < 32000:
        assert np.array_equal(want, full_oracle.encode_windows(audio[:, :n_chunks * chunk], chunk, ctx))
    hip_full.set_window_trim(trim)
    try:
        for bw in (6, 37):
            got = _chunk_range(hip_full, audio, chunk, ctx, bw, 0, n_chunks)
            assert np.array_equal(got, want), (bw, int((got != want).sum()))
            monkeypatch.setenv("RCA_HEAD_KEEP", "0")
            full = _chunk_range(hip_full, audio, chunk, ctx, bw, 0, n_chunks)
            monkeypatch.delenv("RCA_HEAD_KEEP")
            assert np.array_equal(full, want), (bw, "RCA_HEAD_KEEP=0")
        # a range that starts inside the warm-up and one that starts in the steady state
        for b, e in ((3, 29), (25, 46)):
            got = _chunk_range(hip_full, audio, chunk, ctx, 6, b, e)
            fpc = hip_full.frames_per_chunk(chunk)
            assert np.array_equal(got, want[:, b * fpc:e * fpc]), (b, e)
    finally:
        hip_full.set_window_trim(False)


def test_streaming_semantics_against_the_oracle(hip_full, full_oracle):
    """The shapes of test_batch_windows_match_streaming_semantics (4 s of stereo, 2 s context, 16 windows per pass) against
    oracle.encode_windows, for both chunk sizes."""
    hip_full.set_variant(1)
    audio = np.stack([bench_signal(64000, 1), rich_signal(64000, 2)])
    for chunk in (1600, 1280):
        got = _chunk_range(hip_full, audio, chunk, 32000, 16, 0, 64000 // chunk)
        assert np.array_equal(got, full_oracle.encode_windows(audio, chunk, 32000)), chunk


@pytest.mark.parametrize("chunk", [1600, 1280])
def test_bench_shape_256_windows_per_pass(chunk, hip_full, monkeypatch):
    """batch_windows 256 at the headline shape (2 s windows): two full passes and a ragged third, from chunk 0.  The restricted
    launch really runs: the conv launches of a pass report the FLOPs of the full last layer less its unread columns."""
    hip_full.set_variant(1)
    ctx = 32000
    warm = ctx // chunk
    n_chunks = warm + 256 + 256 + 37
    audio = _audio(1, n_chunks * chunk, 17)
    want = _reference_windows(hip_full, audio, chunk, ctx, 0, n_chunks)
    got = _chunk_range(hip_full, audio, chunk, ctx, 256, 0, n_chunks)
    assert np.array_equal(got, want), int((got != want).sum())
    monkeypatch.setenv("RCA_HEAD_KEEP", "0")
    full = _chunk_range(hip_full, audio, chunk, ctx, 256, 0, n_chunks)
    monkeypatch.delenv("RCA_HEAD_KEEP")
    assert np.array_equal(full, want)
    # one steady-state pass of 256 windows, with and without the view
    fpc = hip_full.frames_per_chunk(chunk)
    b, e = warm + 3, warm + 3 + 256
    head = _conv_flops(hip_full, lambda: _chunk_range(hip_full, audio, chunk, ctx, 256, b, e))
    monkeypatch.setenv("RCA_HEAD_KEEP", "0")
    base = _conv_flops(hip_full, lambda: _chunk_range(hip_full, audio, chunk, ctx, 256, b, e))
    monkeypatch.delenv("RCA_HEAD_KEEP")
    cfg = hip_full.cfg
    F = ctx // hip_full.hop
    per_column = 2.0 * cfg.channels[-1] * cfg.k_latent * cfg.latent_dim
    assert head["launches"] == base["launches"]
    assert base["flops"] - head["flops"] == pytest.approx(per_column * 256 * (F - (fpc + 1)), rel=1e-9)


@pytest.mark.parametrize("which", ["tiny", "odd"])
def test_small_configs(which, hip_tiny, tiny_oracle, odd_pair, monkeypatch):
    """The tiny config and the odd-channel config (last layer: Cin not a multiple of the chunk, Cout narrower than a tile):
    chunk-range calls against the all-frames reference and the oracle, and the big batch of the odd-channel test through
    encode_rows_dev."""
    import torch
    hip, oc = (hip_tiny, tiny_oracle) if which == "tiny" else odd_pair
    hip.set_variant(1)
    for chunk, ctx, C, bw in ((1600, 32000, 2, 6), (1280, 32000, 1, 37), (1600, 960, 2, 37), (1600, 32000, 1, 256)):
        n_chunks = 70 if bw < 256 else 20 + 256 + 37
        audio = _audio(C, n_chunks * chunk, 31)
        want = _reference_windows(hip, audio, chunk, ctx, 0, n_chunks)
        if bw < 256:
            assert np.array_equal(want, oc.encode_windows(audio, chunk, ctx)), (chunk, ctx, C)
        for trim in (False, True):
            hip.set_window_trim(trim)
            try:
                got = _chunk_range(hip, audio, chunk, ctx, bw, 0, n_chunks)
            finally:
                hip.set_window_trim(False)
            assert np.array_equal(got, want), (chunk, ctx, C, bw, trim)
        monkeypatch.setenv("RCA_HEAD_KEEP", "0")
        full = _chunk_range(hip, audio, chunk, ctx, bw, 0, n_chunks)
        monkeypatch.delenv("RCA_HEAD_KEEP")
        assert np.array_equal(full, want), (chunk, ctx, C, bw)
    # 160 windows of 2.1 s (64 x 64 wave tiles and the fused first layer of a small model), 5 frames kept of 105
    T, B, keep = 33600, 160, 5
    big = np.stack([rich_signal(T, 40 + b) for b in range(B)])
    all_frames = hip.encode(big)
    assert np.array_equal(all_frames[:6], oc.encode(big[:6]))
    dev = torch.from_numpy(big).cuda()
    src = torch.arange(B, dtype=torch.int64, device="cuda") * T
    dst = torch.arange(B, dtype=torch.int64, device="cuda") * keep
    out = torch.full((B, keep), -1, dtype=torch.int64, device="cuda")
    hip.encode_rows_dev(dev.data_ptr(), src.data_ptr(), B, T, keep, out.data_ptr(), dst.data_ptr(), B * T, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), all_frames[:, -keep:])


@pytest.mark.parametrize("trim", [False, True])
@pytest.mark.parametrize("which", ["tiny", "full"])
def test_encode_rows_with_an_offset_table(which, trim, hip_tiny, hip_full, monkeypatch):
    """rca_codec_encode_rows_dev: windows picked by a row-offset table (overlapping, out of order, from two "files" in one buffer),
    codes scattered by a second table, n_keep of 1, 5 and F, for a 2 s window, a ragged one and a short one."""
    import torch
    hip = hip_tiny if which == "tiny" else hip_full
    hip.set_variant(1)
    rng = np.random.default_rng(5)
    span = 200000
    buf = np.concatenate([rich_signal(span // 2, 71), bench_signal(span // 2, 72)])
    dev = torch.from_numpy(buf).cuda()
    st = torch.cuda.current_stream().cuda_stream
    hip.set_window_trim(trim)
    try:
        for T, B in ((32000, 37), (31900, 6), (1600, 9), (320, 3)):
            F = hip.num_frames(T)
            off = rng.integers(0, span - T, B).astype(np.int64)
            off[0], off[-1] = span - T, 0
            want = hip.encode(np.stack([buf[o:o + T] for o in off]))
            for keep in sorted({1, min(5, F), F}):
                slots = rng.permutation(B).astype(np.int64) * keep
                out = torch.full((B * keep,), -1, dtype=torch.int64, device="cuda")
                src, dst = torch.from_numpy(off).cuda(), torch.from_numpy(slots).cuda()
                for head in ("1", "0"):
                    monkeypatch.setenv("RCA_HEAD_KEEP", head)
                    out.fill_(-1)
                    hip.encode_rows_dev(dev.data_ptr(), src.data_ptr(), B, T, keep, out.data_ptr(), dst.data_ptr(), span, st)
                    torch.cuda.synchronize()
                    got = out.cpu().numpy().reshape(B, keep)
                    assert np.array_equal(got[slots // keep], want[:, F - keep:]), (T, B, keep, head)
                monkeypatch.delenv("RCA_HEAD_KEEP")
    finally:
        hip.set_window_trim(False)


def test_encode_tail_of_a_large_batch(hip_full, full_oracle):
    """rca_codec_encode_tail_dev with a batch too large for the streaming-tail kernels (they stay as they are): the last n_keep
    codes of the all-frames call."""
    import torch
    hip_full.set_variant(1)
    st = torch.cuda.current_stream().cuda_stream
    for T, B in ((32000, 37), (6400, 64)):
        x = np.stack([rich_signal(T, 120 + b) for b in range(B)])
        want = hip_full.encode(x)
        if T == 6400:
            assert np.array_equal(want[:3], full_oracle.encode(x[:3]))
        dev = torch.from_numpy(x).cuda()
        F = want.shape[1]
        for keep in (1, 4, 5, F - 1, F):
            out = torch.full((B, keep), -1, dtype=torch.int64, device="cuda")
            hip_full.encode_tail_dev(dev.data_ptr(), B, T, keep, out.data_ptr(), st)
            torch.cuda.synchronize()
            assert np.array_equal(out.cpu().numpy(), want[:, -keep:]), (T, B, keep)


@pytest.mark.parametrize("which", ["tiny", "full"])
def test_all_frame_entry_points_after_a_kept_frames_call(which, hip_tiny, hip_full, tiny_oracle, full_oracle):
    """After a kept-frames call has left a compact last-layer output in the workspace, encode_tap of the last layer and
    rca_codec_encoder_dev still return all F frames, bit-equal to the oracle, and encode() all F codes."""
    import torch
    hip, oc = (hip_tiny, tiny_oracle) if which == "tiny" else (hip_full, full_oracle)
    hip.set_variant(1)
    chunk, ctx = 1600, 6400
    audio = _audio(2, 24 * chunk, 9)
    want = _reference_windows(hip, audio, chunk, ctx, 0, 24)
    x = np.stack([rich_signal(6400, 5), rich_signal(6400, 9), bench_signal(6400, 0)])
    n = oc.cfg.n_stages
    codes_want, ze_want = oc.encode(x, tap_layer=n + 1)
    for _ in range(2):
        assert np.array_equal(_chunk_range(hip, audio, chunk, ctx, 6, 0, 24), want)
        got = hip.encode_tap(x, n + 1)
        assert got.shape == ze_want.shape == (3, oc.cfg.latent_dim, 20) and np.array_equal(got, ze_want)
        assert np.array_equal(_chunk_range(hip, audio, chunk, ctx, 6, 4, 24), want[:, 20:])
        dev = torch.from_numpy(x).cuda()
        ze = torch.full((3, 20, oc.cfg.latent_dim), np.nan, dtype=torch.float32, device="cuda")
        hip.encoder_dev(dev.data_ptr(), 3, 6400, ze.data_ptr(), torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert np.array_equal(ze.cpu().numpy(), ze_want.transpose(0, 2, 1))
        assert np.array_equal(_chunk_range(hip, audio, chunk, ctx, 37, 4, 24), want[:, 20:])
        assert np.array_equal(hip.encode(x), codes_want)
