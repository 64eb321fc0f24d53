"""Device ingest of the batch CLI, everything that needs no GPU: the filter and the lengths against scipy's resample_poly, the float64
restatement (tests/ingest_ref.py) against scipy's f32 output, the raw reader, and audio_to_codes.main --device_ingest end to end on
a CPU stand-in whose ingest is that restatement rounded to f32."""
import os
import wave

import numpy as np
import pytest

import ingest_ref
from conftest import bench_signal, rich_signal

RATES = (8000, 11025, 22050, 24000, 32000, 44100, 48000)
CR = 16000


def _n_ins(down):
    return (0, 1, 2, 7, 100, 333, 1500, 3 * down - 1, 3 * down, 3 * down + 1)


@pytest.mark.parametrize("sr", RATES)
def test_taps_and_lengths_are_resample_polys(sr):
    """ingest_taps is the filter resample_poly designs for itself, ingest_out_len the length it returns; the float64 restatement of
    the definition reproduces its f32 output within the bound of an f32 sum (scipy's own rounding) -- so the kernel, held to the same
    restatement, computes what _resample computes."""
    from realtime_codec_agent_amd.audio_tokenizer import _resample, ingest_out_len, ingest_taps
    up, down, taps = ingest_taps(sr, CR)
    g = np.gcd(sr, CR)
    assert (up, down) == (CR // g, sr // g) and taps.dtype == np.float32 and taps.size == 20 * max(up, down) + 1
    rng = np.random.default_rng(sr)
    for n_in in _n_ins(down):
        m = rng.standard_normal(n_in).astype(np.float32)
        want = _resample(m, sr, CR) if n_in else np.zeros(0, np.float32)
        assert ingest_out_len(n_in, up, down) == ingest_ref.out_len(n_in, up, down) == len(want), (sr, n_in)
        if n_in:
            y, bound = ingest_ref.resample64(m, up, down, taps)
            assert (np.abs(want - y) <= bound).all(), (sr, n_in, float(np.abs(want - y).max()))


def test_equal_rates_are_a_pure_conversion():
    from realtime_codec_agent_amd.audio_tokenizer import ingest_out_len, ingest_taps
    up, down, taps = ingest_taps(CR, CR)
    assert (up, down) == (1, 1) and taps.tolist() == [1.0] and ingest_out_len(12345, 1, 1) == 12345
    pcm = np.array([[-32768, 32767], [1, -1], [12345, -54], [0, 7]], "<i2")
    f = pcm.astype(np.float32) / 32768.0
    for c in range(2):
        assert np.array_equal(ingest_ref.frames(pcm.reshape(-1), c, 4, 2, 1), f[:, c])
    assert np.array_equal(ingest_ref.frames(pcm.reshape(-1), 0, 4, 2, 2), f.T.mean(axis=0))
    x = np.random.default_rng(0).standard_normal((3, 50)).astype(np.float32)
    assert np.array_equal(ingest_ref.frames(np.ascontiguousarray(x.T).reshape(-1), 0, 50, 3, 3), x.mean(axis=0))


def _wav(path, sig, sr, width=2):
    """sig [C, N] float -> PCM16 (width 2) or float32 (width 4) .wav"""
    with wave.open(path, "wb") as w:
        w.setnchannels(sig.shape[0]); w.setsampwidth(width); w.setframerate(sr)
        w.writeframes((np.clip(sig.T, -1, 1) * 32767).astype("<i2").tobytes() if width == 2 else np.ascontiguousarray(sig.T, "<f4").tobytes())


def test_raw_reader_returns_the_files_own_samples(tmp_path):
    from realtime_codec_agent_amd.audio_to_codes import RawAudio, read_audio, read_audio_raw
    sig = np.stack([rich_signal(1000, 1), bench_signal(1000, 2)])
    cases = {"m16.wav": (sig[:1], 8000, 2), "s16.wav": (sig, 44100, 2), "f32.wav": (sig, 16000, 4)}
    for name, (s, sr, width) in cases.items():
        p = str(tmp_path / name)
        _wav(p, s, sr, width)
        fsr, a, layout = read_audio_raw(p)
        assert fsr == sr and layout == "interleaved" and a.shape == (1000, s.shape[0])
        assert a.dtype == np.dtype("<i2" if width == 2 else "<f4") and not a.flags.owndata and a.flags.c_contiguous      # a view of the file's bytes
        want = read_audio(p)[1]
        got = a.astype(np.float32) / 32768.0 if width == 2 else a
        assert np.array_equal(got.T, want)
        raw = RawAudio(fsr, a, layout, True, CR)
        assert raw.n_rows == 1 and raw.channels == s.shape[0] and raw.frames == 1000 and raw.out_len == -(-1000 * CR // sr)
    for name, arr, shape in (("mono.npy", sig[0], (1, 1000)), ("st.npy", sig, (2, 1000))):
        p = str(tmp_path / name)
        np.save(p, arr)
        fsr, a, layout = read_audio_raw(p)
        assert (fsr, layout, a.shape, a.dtype) == (16000, "planar", shape, np.float32) and np.array_equal(a, np.atleast_2d(arr))
    with pytest.raises(ValueError):
        RawAudio(16000, sig, "planar", True, CR)          # planar channels cannot be averaged by the kernel


class _IngestCpuEncoder:
    """CPU stand-in for HipWindowEncoder with device ingest: RawAudio items become the float64 restatement rounded to f32, then the
    windows go one by one through the C oracle (tiny codec), as rca_codec_encode_rows_dev treats them."""
    supports_device_ingest = True

    def __init__(self, refuse=()):
        from oracle.codec import OracleCodec
        from realtime_codec_agent_amd.codec_model import init_codec_weights, tiny_codec_config
        self.cfg = tiny_codec_config()
        self.oc = OracleCodec(self.cfg, init_codec_weights(self.cfg, seed=0))
        self.refuse = set(refuse)                          # (up, down) pairs this "kernel" does not take
        self.raw_seen, self.host_seen = 0, 0

    def ingest_supported(self, up, down, n_taps):
        return (up, down) not in self.refuse

    def _rows(self, a):
        from realtime_codec_agent_amd.audio_to_codes import RawAudio
        from realtime_codec_agent_amd.audio_tokenizer import ingest_taps
        if not isinstance(a, RawAudio):
            self.host_seen += 1
            return a
        self.raw_seen += 1
        up, down, taps = ingest_taps(a.sr, self.cfg.sample_rate)
        out = ingest_ref.ingest_rows_f32(a.data, a.layout, a.mix, up, down, taps)
        assert out.shape == (a.n_rows, a.out_len)
        return out

    def encode(self, audio, chunk, ctx, batch):
        return self.oc.encode_windows(self._rows(audio), chunk, ctx)

    def encode_many(self, audios, chunk, ctx, batch_windows):
        from realtime_codec_agent_amd.audio_to_codes import window_table
        audios = [self._rows(a) for a in audios]
        W, fpc = max(chunk, ctx), int((chunk / self.cfg.sample_rate) * self.cfg.framerate)
        lengths = [a.shape[-1] for a in audios for _ in range(a.shape[0])]
        src_base = np.cumsum([0] + lengths)[:-1]
        n_codes = [(n // chunk) * fpc for n in lengths]
        dst_base = np.cumsum([0] + n_codes)[:-1]
        flat = np.concatenate([a[c] for a in audios for c in range(a.shape[0])])
        T, src, dst = window_table(lengths, chunk, W, fpc, src_base, dst_base)
        out = np.full(int(sum(n_codes)), -1, np.int64)
        for t in sorted(set(T.tolist())):
            sel = np.flatnonzero(T == t)
            codes = self.oc.encode(np.stack([flat[s:s + t] for s in src[sel]]))[:, -fpc:]
            for d, c in zip(dst[sel], codes):
                out[d:d + fpc] = c
        assert (out >= 0).all()
        return out, [(int(b), int(b + n)) for b, n in zip(dst_base, n_codes)], (lambda: None)


class _PlainEncoder:
    """An encoder without device ingest (the shape of the existing CPU fakes)."""

    def __init__(self, inner):
        self.cfg, self.encode = inner.cfg, inner.encode


def _tree(root):
    out = {}
    for r, _, fs in os.walk(root):
        for f in fs:
            with open(os.path.join(r, f), "rb") as fh:
                out[os.path.relpath(os.path.join(r, f), root)] = fh.read()
    return out


def _code_counts(root):
    return {os.path.relpath(os.path.join(r, f), root): np.load(os.path.join(r, f)).shape
            for r, _, fs in os.walk(root) for f in fs if f.endswith(".npy")}


def _mixed_corpus(tmp):
    raw = os.path.join(tmp, "raw")
    os.makedirs(os.path.join(raw, "sub"))
    st = lambda n, s: np.stack([rich_signal(n, s), bench_signal(n, s + 1)])
    _wav(os.path.join(raw, "a_8k_stereo.wav"), st(5300, 10), 8000)                 # 10 600 samples after resampling
    _wav(os.path.join(raw, "sub", "b_44k_mono.wav"), st(30000, 20)[:1], 44100)     # 10 885: a mono file (also in the --stereo run)
    _wav(os.path.join(raw, "c_16k_stereo.wav"), st(9000, 30), 16000)
    np.save(os.path.join(raw, "sub", "d.npy"), rich_signal(7000, 40))
    _wav(os.path.join(raw, "e_short_8k.wav"), st(700, 50), 8000)                   # 1 400 samples: shorter than a chunk, no codes
    _wav(os.path.join(raw, "f_float_24k.wav"), st(9100, 60), 24000, width=4)       # float .wav, 2 / 3
    return raw


def test_cli_device_ingest_per_file_tree_equals_pipelined_tree(tmp_path, capsys):
    from realtime_codec_agent_amd import audio_to_codes
    tmp = str(tmp_path)
    raw = _mixed_corpus(tmp)
    enc = _IngestCpuEncoder()
    base = ["--audio_path", raw, "--batch_size", "16", "--context_secs", "0.5"]
    for stereo in ([], ["--stereo"]):
        tag = "s" if stereo else "m"
        enc.raw_seen = enc.host_seen = 0
        out = {k: os.path.join(tmp, k + tag) for k in ("file", "pipe", "host")}
        a = audio_to_codes.main(base + stereo + ["--codes_path", out["file"], "--device_ingest", "--one_file_at_a_time"], encoder=enc, backend="gloo")
        b = audio_to_codes.main(base + stereo + ["--codes_path", out["pipe"], "--device_ingest", "--super_batch_samples", "30000",
                                                 "--reader_threads", "2"], encoder=enc, backend="gloo")
        assert enc.raw_seen == 12 and enc.host_seen == 0      # every file reached the encoder unconverted
        c = audio_to_codes.main(base + stereo + ["--codes_path", out["host"]], encoder=enc, backend="gloo")
        ta, tb = _tree(out["file"]), _tree(out["pipe"])
        assert ta.keys() == tb.keys() and len(ta) == 1 + (10 if stereo else 6)
        assert [k for k in ta if ta[k] != tb[k]] == []
        assert a["codes"] == b["codes"] == c["codes"] > 0 and abs(a["audio_hours"] - b["audio_hours"]) < 1e-12
        # as many codes per file as the default run (host resampling) writes; files at the codec rate: the same bytes
        na, nc = _code_counts(out["file"]), _code_counts(out["host"])
        assert na == nc and any(v[-1] == 0 for v in na.values())
        th = _tree(out["host"])
        same_rate = [k for k in ta if "c_16k" in k or os.sep + "d_c" in k]
        assert len(same_rate) == (3 if stereo else 2) and all(ta[k] == th[k] for k in same_rate)
    capsys.readouterr()
    # a ratio the kernel refuses: those files are prepared on the host and enter as f32 rows, one line on stderr per rate
    enc2 = _IngestCpuEncoder(refuse={(160, 441)})
    d = audio_to_codes.main(base + ["--codes_path", os.path.join(tmp, "r1"), "--device_ingest", "--one_file_at_a_time"], encoder=enc2, backend="gloo")
    e = audio_to_codes.main(base + ["--codes_path", os.path.join(tmp, "r2"), "--device_ingest"], encoder=enc2, backend="gloo")
    err = capsys.readouterr().err
    assert err.count("44100 Hz") == 1 and enc2.host_seen == 2 and enc2.raw_seen == 10
    td, te = _tree(os.path.join(tmp, "r1")), _tree(os.path.join(tmp, "r2"))
    assert td.keys() == te.keys() and all(td[k] == te[k] for k in td) and d["codes"] == e["codes"]
    refused = [k for k in td if "b_44k" in k]
    assert len(refused) == 1 and td[refused[0]] == _tree(os.path.join(tmp, "hostm"))[refused[0]]
    # the flag with an encoder that has no ingest: an error, not a silent host path
    with pytest.raises(ValueError, match="device_ingest"):
        audio_to_codes.main(base + ["--codes_path", os.path.join(tmp, "x"), "--device_ingest"], encoder=_PlainEncoder(enc), backend="gloo")
