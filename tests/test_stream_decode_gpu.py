"""Streamed batch decode on the GPU (MI355X): rca_codec_decode_rows_dev against rca_codec_decode_tail_dev row by row,
rca_codec_crossfade_join_dev against chained numpy smooth_join, whole streams against the per-chunk loop (tiny codec: the oracle;
full codec: detokenize_audio + smooth_join on the same handle; tests/test_decoder_layers_gpu.py pins the full decoder to the oracle,
layer by layer and on the 64 x 64 tiles of the B = 257 launches here), and the CLI's two paths.
Everything is compared bit for bit."""
import os

import numpy as np
import pytest

from conftest import bench_signal, rich_signal
from tests.stream_decode_ref import stream_decode_loop

pytestmark = pytest.mark.gpu

HOP, SR, FR, L = 320, 16000, 50.0, 320
SHAPES = [(1, 1), (1, 320), (2, 321), (3, 640), (4, 1279), (12, 1920), (100, 1920), (100, 32000)]


@pytest.fixture(scope="module")
def hips(tiny_codec, full_codec):
    from realtime_codec_agent_amd.codec import HipCodec
    return {"tiny": HipCodec(*tiny_codec, device=0), "full": HipCodec(*full_codec, device=0)}


@pytest.fixture(scope="module")
def full_model(full_codec):
    from realtime_codec_agent_amd.codec import MagiCodecHIP
    return MagiCodecHIP(*full_codec, device="cuda:0")


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


# ------------------------------------------------------------------------------------------------ the rows call
def _rows_case(hip, B, F, n, seed):
    """Overlapping source rows anywhere in one code buffer, destinations in shuffled order with gaps, NaN fill."""
    rng = np.random.default_rng(seed)
    span = F + min(B, 40) * 3 + 5
    codes = rng.integers(0, hip.cfg.codebook_size, span).astype(np.int64)
    src = rng.integers(0, span - F + 1, B).astype(np.int64)                 # B rows in < B * F codes: they overlap
    src[0], src[-1] = span - F, 0
    gap = 7
    dst = (rng.permutation(B).astype(np.int64) * (n + gap)) + 3
    pcm_span = int(B * (n + gap) + 3)
    return codes, src, dst, pcm_span


@pytest.mark.parametrize("F, n", SHAPES)
@pytest.mark.parametrize("B", [1, 3, 257])
@pytest.mark.parametrize("tag", ["tiny", "full"])
def test_rows_equal_the_tail_call_row_by_row(hips, tag, B, F, n):
    import torch
    hip = hips[tag]
    codes, src, dst, pcm_span = _rows_case(hip, B, F, n, 1000 * B + F + n)
    st = _stream()
    cdev, sdev, ddev = (torch.from_numpy(a).cuda() for a in (codes, src, dst))
    out = torch.full((pcm_span,), float("nan"), dtype=torch.float32, device="cuda")
    hip.decode_rows_dev(cdev.data_ptr(), sdev.data_ptr(), B, F, n, out.data_ptr(), ddev.data_ptr(), len(codes), pcm_span, st)
    hip.check_decode_error(st)
    block = torch.from_numpy(np.stack([codes[s:s + F] for s in src])).cuda()
    want = torch.zeros((B, n), dtype=torch.float32, device="cuda")
    hip.decode_tail_dev(block.data_ptr(), B, F, n, want.data_ptr(), st)
    torch.cuda.synchronize()
    got, want = out.cpu().numpy(), want.cpu().numpy()
    written = np.zeros(pcm_span, bool)
    for b in range(B):
        assert np.array_equal(got[dst[b]:dst[b] + n], want[b]), (tag, B, F, n, b)
        written[dst[b]:dst[b] + n] = True
    assert not np.isnan(want).any() and np.isnan(got[~written]).all() and (~written).sum() == pcm_span - B * n


def test_rows_equal_the_oracle(hips, tiny_oracle):
    """The reference of the test above is itself checked elsewhere; here a few rows go straight against the CPU oracle."""
    import torch
    hip = hips["tiny"]
    codes, src, dst, pcm_span = _rows_case(hip, 5, 12, 1920, 9)
    st = _stream()
    cdev, sdev, ddev = (torch.from_numpy(a).cuda() for a in (codes, src, dst))
    out = torch.full((pcm_span,), float("nan"), dtype=torch.float32, device="cuda")
    hip.decode_rows_dev(cdev.data_ptr(), sdev.data_ptr(), 5, 12, 1920, out.data_ptr(), ddev.data_ptr(), len(codes), pcm_span, st)
    hip.check_decode_error(st)
    got = out.cpu().numpy()
    want = tiny_oracle.decode(np.stack([codes[s:s + 12] for s in src]))[:, -1920:]
    assert all(np.array_equal(got[dst[b]:dst[b] + 1920], want[b]) for b in range(5))


def test_rows_flag_bad_codes_and_rows_outside_their_span(hips):
    import torch
    from realtime_codec_agent_amd._native import RcaError
    hip = hips["tiny"]
    st = _stream()
    B, F, n = 3, 4, 640
    codes = np.arange(20, dtype=np.int64)
    src, dst = np.array([0, 5, 16], np.int64), np.array([0, 700, 1400], np.int64)

    def run(codes, src, dst, code_span, pcm_span=2100):
        out = torch.full((2100,), float("nan"), dtype=torch.float32, device="cuda")
        c, s, d = (torch.from_numpy(a).cuda() for a in (codes, src, dst))
        hip.decode_rows_dev(c.data_ptr(), s.data_ptr(), B, F, n, out.data_ptr(), d.data_ptr(), code_span, pcm_span, st)
        hip.check_decode_error(st)
        return out.cpu().numpy()
    assert not np.isnan(run(codes, src, dst, 20)[:640]).any()
    for bad in (hip.cfg.codebook_size, -1):
        c = codes.copy()
        c[6] = bad
        with pytest.raises(RcaError, match="out of range"):
            run(c, src, dst, 20)
    assert not np.isnan(run(codes, src, dst, 20)[700:1340]).any()             # the flag was cleared
    with pytest.raises(RcaError):                                             # row 2 would read codes [16, 20) of a 19-code span
        run(codes, src, dst, 19)
    with pytest.raises(RcaError):                                             # a negative source offset
        run(codes, np.array([0, -1, 16], np.int64), dst, 20)
    with pytest.raises(RcaError):                                             # row 2 would write [1500, 2140) of 2100
        run(codes, src, np.array([0, 700, 1500], np.int64), 20)
    assert not np.isnan(run(codes, src, dst, 20)[1400:2040]).any()


def test_rows_refusals_enqueue_nothing(hips):
    import torch
    from realtime_codec_agent_amd._native import RcaError
    hip = hips["tiny"]
    st = _stream()
    codes = torch.arange(64, dtype=torch.int64, device="cuda")
    off = torch.zeros(4, dtype=torch.int64, device="cuda")
    out = torch.full((4096,), float("nan"), dtype=torch.float32, device="cuda")
    c, o, p = codes.data_ptr(), off.data_ptr(), out.data_ptr()
    bad = [dict(B=0), dict(F=0), dict(n=0), dict(B=-1), dict(n=4 * HOP + 1), dict(codes=0), dict(src=0), dict(pcm=0), dict(dst=0),
           dict(code_span=3), dict(pcm_span=639)]
    for kw in bad:
        a = dict(codes=c, src=o, B=1, F=4, n=640, pcm=p, dst=o, code_span=64, pcm_span=4096)
        a.update(kw)
        with pytest.raises(RcaError, match="rc=-1"):
            hip.decode_rows_dev(a["codes"], a["src"], a["B"], a["F"], a["n"], a["pcm"], a["dst"], a["code_span"], a["pcm_span"], st)
    hip.check_decode_error(st)
    assert np.isnan(out.cpu().numpy()).all()


# ------------------------------------------------------------------------------------------------ the join call
def _ramps(n_fade):
    from realtime_codec_agent_amd.utils.audio_utils import create_crossfade_ramps
    sr, secs = {0: (16000, 0.0), 1: (50, 0.02), 320: (16000, 0.02)}[n_fade]
    got = create_crossfade_ramps(sr, secs)
    assert got[0] == n_fade
    return got


def _join_case(n_fade, rng):
    """Streams of 1, 2 and 9 segments (and one more of 2), a middle segment of exactly 2 * n_fade, tails of exactly n_fade;
    segments lie in the piece buffer in another order than the streams, with gaps; outputs with gaps."""
    from realtime_codec_agent_amd._native import JOIN_SEG
    streams = [[700], [1300, n_fade], [400, 2 * n_fade, 1500, 2 * n_fade + 1, 333 + 2 * n_fade, 2048, 2 * n_fade, 900, n_fade], [max(n_fade, 1), 1025]]
    lens = [n for s in streams for n in s]
    order = rng.permutation(len(lens))
    seg_off = np.zeros(len(lens), np.int64)
    pos = 2
    for i in order:
        seg_off[i] = pos
        pos += lens[i] + 3
    seg_span = pos
    segs = np.zeros(len(lens), JOIN_SEG)
    segs["seg_off"], segs["n"] = seg_off, lens
    i, out0, slices = 0, 5, []
    for s in streams:
        o = out0
        for k, n in enumerate(s):
            segs["out_off"][i] = o
            segs["flags"][i] = (1 if k == 0 else 0) | (2 if k == len(s) - 1 else 0)
            o += n - n_fade
            i += 1
        slices.append((out0, o + n_fade))
        out0 = o + n_fade + 11
    return streams, segs, seg_span, out0, slices


def _run_join(hip, pieces, segs, seg_span, fade_in, n_fade, out_span, segs_dev=None):
    import torch
    st = _stream()
    pdev = torch.from_numpy(pieces).cuda()
    sdev = torch.from_numpy(np.ascontiguousarray(segs_dev if segs_dev is not None else segs).view(np.uint8).copy()).cuda()
    fdev = torch.from_numpy(np.ascontiguousarray(fade_in, dtype=np.float32)).cuda() if n_fade else None
    out = torch.full((out_span,), float("nan"), dtype=torch.float32, device="cuda")
    try:
        hip.crossfade_join_dev(pdev.data_ptr(), seg_span, sdev.data_ptr(), np.ascontiguousarray(segs), fdev.data_ptr() if n_fade else 0, n_fade,
                               out.data_ptr(), out_span, st)
    finally:
        torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize("n_fade", [0, 1, 320])
def test_join_equals_chained_smooth_join(hips, n_fade):
    from realtime_codec_agent_amd.utils.audio_utils import smooth_join
    rng = np.random.default_rng(20 + n_fade)
    _, fade_in, fade_out = _ramps(n_fade)
    streams, segs, seg_span, out_span, slices = _join_case(n_fade, rng)
    pieces = rng.standard_normal(seg_span).astype(np.float32)
    got = _run_join(hips["tiny"], pieces, segs, seg_span, fade_in, n_fade, out_span)
    written = np.zeros(out_span, bool)
    i = 0
    for s, (a, b) in zip(streams, slices):
        want = np.zeros(0, np.float32)
        for n in s:
            o = int(segs["seg_off"][i])
            want = smooth_join(want, pieces[o:o + n], n_fade, fade_in, fade_out)
            i += 1
        assert len(want) == b - a and np.array_equal(got[a:b], want), (n_fade, s)
        written[a:b] = True
    assert np.isnan(got[~written]).all()


def test_join_refuses_malformed_descriptors(hips):
    from realtime_codec_agent_amd._native import RcaError
    n_fade = 320
    rng = np.random.default_rng(4)
    _, fade_in, _ = _ramps(n_fade)
    streams, good, seg_span, out_span, _ = _join_case(n_fade, rng)
    pieces = rng.standard_normal(seg_span).astype(np.float32)

    def edit(i, field, value):
        s = good.copy()
        s[field][i] = value
        return s
    bad = {
        "broken chain": edit(4, "out_off", good["out_off"][4] + 1),
        "non-head shorter than the fade": edit(2, "n", n_fade - 1),
        "segment with a successor shorter than the fade": edit(1, "n", n_fade - 1),
        "middle shorter than two fades": edit(4, "n", 2 * n_fade - 1),
        "reads past the pieces": edit(5, "seg_off", seg_span - 10),
        "reads before the pieces": edit(5, "seg_off", -1),
        "writes past the output": edit(len(good) - 1, "n", 1025 + 4096),
        "first is no head": edit(0, "flags", 2),
        "last is no tail": edit(len(good) - 1, "flags", 0),
        "head inside a stream": edit(4, "flags", 1),
        "no predecessor": edit(1, "flags", 2),
        "unknown flag": edit(0, "flags", 7),
        "negative length": edit(0, "n", -1),
    }
    for why, segs in bad.items():
        with pytest.raises(RcaError, match="rc=-1"):
            _run_join(hips["tiny"], pieces, segs, seg_span, fade_in, n_fade, out_span)
    # nothing was written by any refused call: every check comes from the host copy, before the launch
    import torch
    st = _stream()
    out = torch.full((out_span,), float("nan"), dtype=torch.float32, device="cuda")
    pdev, fdev = torch.from_numpy(pieces).cuda(), torch.from_numpy(fade_in.copy()).cuda()
    sdev = torch.from_numpy(good.view(np.uint8).copy()).cuda()
    for segs in bad.values():
        with pytest.raises(RcaError):
            hips["tiny"].crossfade_join_dev(pdev.data_ptr(), seg_span, sdev.data_ptr(), segs, fdev.data_ptr(), n_fade, out.data_ptr(), out_span, st)
    with pytest.raises(RcaError):
        hips["tiny"].crossfade_join_dev(pdev.data_ptr(), seg_span, sdev.data_ptr(), good, 0, n_fade, out.data_ptr(), out_span, st)
    torch.cuda.synchronize()
    assert np.isnan(out.cpu().numpy()).all()


# ------------------------------------------------------------------------------------------------ whole streams
@pytest.fixture(scope="module")
def tiny_model(tiny_codec):
    from realtime_codec_agent_amd.codec import MagiCodecHIP
    return MagiCodecHIP(*tiny_codec, device="cuda:0")


@pytest.fixture(scope="module")
def tiny_codes():
    return np.random.default_rng(11).integers(0, 1024, size=(2, 37)).astype(np.int64)


@pytest.mark.parametrize("k", [1, 3, 5])
def test_tiny_streams_equal_the_loop_on_the_oracle(tiny_model, tiny_oracle, tiny_codes, k):
    want = stream_decode_loop(tiny_oracle.decode, tiny_codes, k, 10, SR, FR)[0]
    for clip in (True, False):
        got = tiny_model.stream_decode_np(tiny_codes, k, 10, L, clip=clip, batch=8)
        assert got.dtype == np.float32 and got.shape == (2, 37 * HOP) and np.array_equal(got, want), (k, clip)


def _hip_loop(tok, chars, step):
    """The per-chunk loop as it exists without this feature: detokenize_audio(chunk, preroll_samples=L) + smooth_join."""
    from realtime_codec_agent_amd.utils.audio_utils import create_crossfade_ramps, smooth_join
    n_fade, fade_in, fade_out = create_crossfade_ramps(tok.sampling_rate, 0.02)
    audio = np.zeros((tok.num_channels, 0), np.float32)
    for start in range(0, len(chars), step):
        (_, out), _, _ = tok.detokenize_audio(chars[start:start + step], preroll_samples=n_fade)
        audio = smooth_join(audio, out.reshape(tok.num_channels, -1), n_fade, fade_in, fade_out)
    return audio


@pytest.mark.parametrize("N, k, ctx_secs", [(230, 5, 2.0), (450, 201, 2.0)])
def test_full_streams_equal_the_per_chunk_hip_loop(full_model, N, k, ctx_secs):
    from realtime_codec_agent_amd.audio_tokenizer import AudioTokenizer
    from realtime_codec_agent_amd.codec_chars import codes_to_chars
    codes = np.random.default_rng(N).integers(0, 131072, size=(1, N)).astype(np.int64)
    tok = AudioTokenizer(codec_model=full_model, num_channels=1, context_secs=ctx_secs, device="cuda:0")
    assert tok.framerate == FR and tok.context_frames == 100
    want = _hip_loop(tok, codes_to_chars(codes, 131072), k)
    got = full_model.stream_decode_np(codes, k, 100, L)
    assert got.shape == want.shape and np.array_equal(got, want)
    assert got.shape[1] == {230: 230 * HOP, 450: 449 * HOP}[N]               # 450 / 201: the second window has no room for a preroll


@pytest.mark.parametrize("channels", [1, 2])
def test_chunked_detokenize_audio_is_the_loop_from_any_context(full_model, channels):
    from realtime_codec_agent_amd.audio_tokenizer import AudioTokenizer
    from realtime_codec_agent_amd.codec_chars import codes_to_chars
    rng = np.random.default_rng(70 + channels)
    toks = [AudioTokenizer(codec_model=full_model, num_channels=channels, device="cuda:0") for _ in range(2)]
    mk = lambda n: codes_to_chars(rng.integers(0, 131072, size=(1, n * channels)), 131072)
    warm, text = mk(23), mk(57)
    for t in toks:
        t.detokenize_audio(warm)                                             # both start from the same non-empty context
    step = int(0.1 * FR * channels)
    want = _hip_loop(toks[0], text, step)
    sr, got = toks[1].chunked_detokenize_audio(text, 0.1)
    assert sr == SR and np.array_equal(got.reshape(channels, -1), want)
    assert toks[1].detokenize_context == toks[0].detokenize_context and len(toks[1].detokenize_context) == 80 * channels
    # a string the device plan does not take (a hanging channel code, or chunks shorter than the fade) goes through the loop itself
    toks[0].reset_context(); toks[1].reset_context()
    odd = mk(9)[:-1] if channels == 2 else mk(9)
    want = _hip_loop(toks[0], odd, step)
    assert np.array_equal(toks[1].chunked_detokenize_audio(odd, 0.1)[1].reshape(channels, -1), want)
    assert toks[1].detokenize_context == toks[0].detokenize_context


# ------------------------------------------------------------------------------------------------ the CLI
def test_cli_pipelined_tree_equals_one_file_at_a_time(tmp_path, full_model):
    """A tree written by audio_to_codes (three short stereo files and a mono one, full codec) rendered by both paths of
    codes_to_audio: byte for byte the same files, as exact float32 and as 16-bit PCM; one stem is also checked against the loop."""
    import wave
    from realtime_codec_agent_amd import audio_to_codes, codes_to_audio
    raw = str(tmp_path / "raw")
    os.makedirs(os.path.join(raw, "sub"))
    for i, n in enumerate([16000 + 700, 9000, 16000 * 2 + 1600]):
        sig = np.stack([rich_signal(n, 40 + i), bench_signal(n, 50 + i)])
        with wave.open(os.path.join(raw, "sub" if i % 2 else "", f"f{i}.wav"), "wb") as w:
            w.setnchannels(2); w.setsampwidth(2); w.setframerate(16000)
            w.writeframes((np.clip(sig.T, -1, 1) * 32767).astype("<i2").tobytes())
    with wave.open(os.path.join(raw, "m.wav"), "wb") as w:
        w.setnchannels(1); w.setsampwidth(2); w.setframerate(16000)
        w.writeframes((np.clip(rich_signal(16000 + 300, 77), -1, 1) * 32767).astype("<i2").tobytes())
    codes_root = str(tmp_path / "codes")
    audio_to_codes.main(["--audio_path", raw, "--codes_path", codes_root, "--stereo"])

    class Dec(codes_to_audio.HipStreamDecoder):
        def __init__(self, model):                                            # the module's model instead of a second set of weights
            import torch
            self.torch, self.model, self.cfg, self.device = torch, model, model.cfg, model.device
            self.dec_left = model.hip.receptive_field()[1]
            self.stage_times = dict(slot_wait_s=0.0, pack_s=0.0, enqueue_s=0.0, gpu_ms=0.0, super_batches=0, passes=0)
    dec = Dec(full_model)

    def tree(root):
        out = {}
        for r, _, fs in os.walk(root):
            for f in fs:
                with open(os.path.join(r, f), "rb") as fh:
                    out[os.path.relpath(os.path.join(r, f), root)] = fh.read()
        return out
    for fmt in ("npy", "wav16"):
        a, b = str(tmp_path / f"a_{fmt}"), str(tmp_path / f"b_{fmt}")
        common = ["--codes_path", codes_root, "--stereo", "--format", fmt]
        s1 = codes_to_audio.main(common + ["--audio_path", a, "--one_file_at_a_time"], decoder=dec)
        s2 = codes_to_audio.main(common + ["--audio_path", b, "--super_batch_codes", "150", "--batch_size", "16"], decoder=dec)
        ta, tb = tree(a), tree(b)
        assert ta.keys() == tb.keys() and len(ta) == 4
        assert not [k for k in ta if ta[k] != tb[k]]
        assert s1["codes"] == s2["codes"] > 0 and s1["refused"] == s2["refused"] == []
        assert dec.pipeline_times["decode_many_super_batches"] >= 2
    leaf = os.path.join("MagiCodec-50Hz-Base", "0.1s_2.0s", "stereo")
    from realtime_codec_agent_amd.audio_tokenizer import AudioTokenizer
    from realtime_codec_agent_amd.codec_chars import codes_to_chars
    tok = AudioTokenizer(codec_model=full_model, num_channels=1, device="cuda:0")
    got = np.load(os.path.join(str(tmp_path / "b_npy"), leaf, "f0.npy"))
    assert got.dtype == np.float32 and got.shape[0] == 2
    for c in range(2):
        tok.reset_context()
        codes = np.load(os.path.join(codes_root, leaf, f"f0_c{c}.npy"))
        assert np.array_equal(got[c], _hip_loop(tok, codes_to_chars(codes, 131072), 5)[0])
