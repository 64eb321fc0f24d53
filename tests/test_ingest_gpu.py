"""Device ingest on the MI355X: rca_codec_ingest_rows_dev against the float64 restatement (tests/ingest_ref.py) on every output
sample, what it may touch and read, row independence, the exact 1 : 1 case, the refusals, and the batch CLI with --device_ingest."""
import os
import wave

import numpy as np
import pytest

import ingest_ref
from conftest import bench_signal, rich_signal

pytestmark = pytest.mark.gpu

TILE, SPAN = 256, 2048          # outputs per tile / per block of ingest_rows_kernel
SENTINEL = np.uint32(0x7FC0DEAD)
RATIOS = [(1, 1), (2, 1), (1, 2), (1, 3), (2, 3), (160, 441), (320, 441), (640, 441)]
GAP = 4


@pytest.fixture(scope="module")
def hip(tiny_codec):
    from realtime_codec_agent_amd.codec import HipCodec
    return HipCodec(*tiny_codec, device=0)


def _taps(up, down):
    from realtime_codec_agent_amd.audio_tokenizer import ingest_taps
    g = np.gcd(up, down)
    assert g == 1
    u, d, taps = ingest_taps(16000 * down, 16000 * up)      # any pair of rates in the ratio down : up designs the same filter
    assert (u, d) == (up, down)
    return taps


def _launch(hip, src: np.ndarray, rows, up, down, taps, dst_len, dst_span=None, refused=False):
    """One rca_codec_ingest_rows_dev over the flat int16 / float32 array src; rows = (src_off, n_in, dst_off, src_stride, n_mix).
    -> the whole destination as uint32 bits (pre-filled with SENTINEL).  refused: the call must fail with RCA_ERR_ARG."""
    import contextlib
    import torch
    from realtime_codec_agent_amd import _native as N
    rows_np = np.array(rows, dtype=N.INGEST_ROW)
    src_dev = torch.from_numpy(src.view(np.uint8).copy()).cuda()
    rows_dev = torch.from_numpy(rows_np.view(np.uint8).copy()).cuda()
    dst = torch.full((dst_len,), int(SENTINEL), dtype=torch.int32, device="cuda")
    with pytest.raises(N.RcaError, match="rc=-1") if refused else contextlib.nullcontext():
        hip.ingest_rows_dev(src_dev.data_ptr(), src.size, N.RCA_PCM_S16 if src.dtype == np.int16 else N.RCA_PCM_F32, rows_dev.data_ptr(), rows_np,
                            up, down, taps, dst.data_ptr(), dst_len if dst_span is None else dst_span, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return dst.cpu().numpy().view(np.uint32)


def _edge(up, n_taps):
    return max(3, (n_taps // up) // 2)


def _n_ins(up, down, n_taps):
    """0, 1, 2; one length so short that the zero extensions of both ends meet inside one output's taps; lengths whose outputs end one
    short of, at and one past a tile and a block of the kernel (as near as the ratio allows); about 3 000 outputs."""
    out = {0, 1, 2, _edge(up, n_taps)}
    for edge in (TILE, SPAN):
        for n_out in (edge - 1, edge, edge + 1):
            out.add(max(1, n_out * down // up))
            out.add(-(-n_out * down // up))
    out.add(3000 * down // up)
    return sorted(out)


def _forms(n_ins, rng, scale_of, poison_odd):
    """The three source forms.  -> [(flat source, [(src_off, n_in, src_stride, n_mix, start of the row's region)])]: regions back to
    back with GAP poisoned elements between them (1e30 / 32767); region i is noise of scale scale_of(i), or poison all over when
    poison_odd and i is odd.  The int16 regions begin with -32768, 32767."""
    forms = []
    for dtype, stride, mixes in ((np.int16, 2, ((0, 1), (1, 1), (0, 2))), (np.float32, 1, ((0, 1),)), (np.float32, 3, ((0, 3),))):
        poison = 32767 if dtype == np.int16 else np.float32(1e30)
        parts, rows, pos = [np.full(GAP, poison, dtype)], [], GAP
        for i, n in enumerate(n_ins):
            x = rng.standard_normal(n * stride) * scale_of(i)
            if dtype == np.int16:
                reg = np.clip(np.round(x * 10000.0), -32768, 32767).astype(np.int16)
                if reg.size >= 2:
                    reg[:2] = (-32768, 32767)
            else:
                reg = x.astype(np.float32)
            if poison_odd and i % 2:
                reg[:] = poison
            parts += [reg, np.full(GAP, poison, dtype)]
            rows += [(pos + off, n, stride, n_mix, pos) for off, n_mix in mixes]
            pos += n * stride + GAP
        forms.append((np.concatenate(parts), rows))
    return forms


def _check(hip, src, rows, up, down, taps, label):
    """Launch all rows (destinations back to back with GAP-sample gaps); every output sample within the bound of the float64
    restatement, every other element of the destination still the sentinel.  -> {row index: the row's output bits}."""
    n_outs = [ingest_ref.out_len(r[1], up, down) for r in rows]
    dst_offs = np.concatenate([[GAP], GAP + np.cumsum([n + GAP for n in n_outs])]).astype(np.int64)
    dst_len = int(dst_offs[-1])
    bits = _launch(hip, src, [(o, n, int(d), s, mx) for (o, n, s, mx, _), d in zip(rows, dst_offs)], up, down, taps, dst_len)
    touched = np.zeros(dst_len, bool)
    got_rows = {}
    for i, ((off, n, stride, n_mix, _), d, n_out) in enumerate(zip(rows, dst_offs, n_outs)):
        touched[d:d + n_out] = True
        got = bits[d:d + n_out].view(np.float32)
        y, bound = ingest_ref.resample64(ingest_ref.frames(src, off, n, stride, n_mix), up, down, taps)
        err = np.abs(got.astype(np.float64) - y)
        bad = np.flatnonzero(~(err <= bound))
        assert bad.size == 0, f"{label} row {i} (n_in={n} stride={stride} n_mix={n_mix}): {bad.size} samples outside the bound, first {bad[:4]}, " \
                              f"err {err[bad[:4]]} bound {bound[bad[:4]]}"
        got_rows[i] = bits[d:d + n_out].copy()
    assert (bits[~touched] == SENTINEL).all(), f"{label}: elements outside the rows were written"
    return got_rows


@pytest.mark.parametrize("up,down", RATIOS)
def test_kernel_against_float64_and_row_independence(hip, up, down):
    taps = _taps(up, down)
    n_ins = _n_ins(up, down, taps.size)
    rng = np.random.default_rng(1000 * up + down)
    sets = (("unit", lambda i: 1.0, False), ("1e4 range", lambda i: 1.0 if i % 2 == 0 else 1e-4, False), ("poisoned neighbours", lambda i: 1.0, True))
    for name, scale_of, poison_odd in sets:
        for src, rows in _forms(n_ins, rng, scale_of, poison_odd):
            label = f"{up}/{down} {name} {src.dtype} stride {rows[0][2]}"
            got = _check(hip, src, rows, up, down, taps, label)
            if name != "unit":
                continue
            # row independence: a row ingested alone, from a copy of its samples at two other placements, gives the bits it got above
            pick = {1, _edge(up, taps.size), max(n_ins)} | {n for n in n_ins if ingest_ref.out_len(n, up, down) in (*range(TILE, TILE + 3), *range(SPAN, SPAN + 3))}
            for i, (off, n, stride, n_mix, start) in enumerate(rows):
                if n not in pick:
                    continue
                for s_pad, d_pad in ((0, 0), (7, 13)):
                    own = np.concatenate([np.zeros(s_pad, src.dtype), src[start:start + n * stride]])
                    n_out = ingest_ref.out_len(n, up, down)
                    alone = _launch(hip, own, [(s_pad + off - start, n, d_pad, stride, n_mix)], up, down, taps, d_pad + n_out + 3)
                    assert np.array_equal(alone[d_pad:d_pad + n_out], got[i]), f"{label} row {i}: alone at ({s_pad}, {d_pad}) != in the batch"
                    assert (alone[:d_pad] == SENTINEL).all() and (alone[d_pad + n_out:] == SENTINEL).all()


def test_one_to_one_is_exact(hip):
    rng = np.random.default_rng(7)
    pcm = rng.integers(-32768, 32768, size=(1000, 2)).astype(np.int16)
    pcm[:2] = [[-32768, 32767], [32767, -32768]]
    f = pcm.astype(np.float32) / 32768.0
    taps = _taps(1, 1)
    n = len(pcm)
    bits = _launch(hip, pcm.reshape(-1), [(0, n, 0, 2, 1), (1, n, n, 2, 1), (0, n, 2 * n, 2, 2)], 1, 1, taps, 3 * n)
    got = bits.view(np.float32).reshape(3, n)
    assert np.array_equal(got[0], f[:, 0]) and np.array_equal(got[1], f[:, 1]) and np.array_equal(got[2], f.T.mean(axis=0))
    x = rng.standard_normal(999).astype(np.float32)
    x[:6] = [-0.0, 0.0, np.float32(1e-45), np.inf, -np.inf, np.float32(3.4e38)]
    bits = _launch(hip, x, [(0, 999, 0, 1, 1), (1, 333, 999, 3, 1)], 1, 1, None, 999 + 333)
    assert np.array_equal(bits[:999], x.view(np.uint32)) and np.array_equal(bits[999:], x[1::3].view(np.uint32))


def test_refusals_leave_the_destination_alone(hip):
    x = np.ones(100, np.float32)
    taps21 = _taps(2, 1)
    assert hip.ingest_supported(640, 441, 12801) and not hip.ingest_supported(1000, 999, 20001)
    for what, (rows, up, down, taps, span) in {
        "even n_taps": ([(0, 100, 0, 1, 1)], 2, 1, taps21[:-1], None),
        "up = 0": ([(0, 100, 0, 1, 1)], 0, 1, taps21, None),
        "row past dst_span": ([(0, 50, 0, 1, 1), (50, 50, 100, 1, 1)], 2, 1, taps21, 199),
        "row past the source": ([(51, 50, 0, 1, 1)], 2, 1, taps21, None),
        "n_mix over the stride": ([(0, 50, 0, 1, 2)], 2, 1, taps21, None),
        "tap table over the budget": ([(0, 100, 0, 1, 1)], 1000, 999, np.zeros(20001, np.float32), None),
    }.items():
        bits = _launch(hip, x, rows, up, down, taps, 220, span, refused=True)
        assert (bits == SENTINEL).all(), what
    good = _launch(hip, x, [(0, 50, 0, 1, 1), (50, 50, 100, 1, 1)], 2, 1, taps21, 220, 200)      # the same rows fit a span of 200
    assert (good[:200] != SENTINEL).all() and (good[200:] == SENTINEL).all()


# ------------------------------------------------------------------------------------------------ the CLI
@pytest.fixture(scope="module")
def encoder():
    from realtime_codec_agent_amd.audio_to_codes import HipWindowEncoder
    return HipWindowEncoder("MagiCodec-50Hz-Base", 0)


def _wav(path, sig, sr):
    with wave.open(path, "wb") as w:
        w.setnchannels(sig.shape[0]); w.setsampwidth(2); w.setframerate(sr)
        w.writeframes((np.clip(sig.T, -1, 1) * 32767).astype("<i2").tobytes())


def _corpus(root, sr, lengths, mono):
    """The corpus shape of test_batch_cli_cross_file_pipeline_equals_per_file_loop: stereo PCM16 files in two directories plus one
    mono file; `lengths` and `mono` = (rate, frames) in frames of the files' own rates."""
    os.makedirs(os.path.join(root, "sub"))
    for i, n in enumerate(lengths):
        _wav(os.path.join(root, "sub" if i % 2 else "", f"f{i}.wav"), np.stack([rich_signal(n, 40 + i), bench_signal(n, 50 + i, sr)]), sr)
    _wav(os.path.join(root, "f2b_mono.wav"), rich_signal(mono[1], 77)[None, :], mono[0])


def _tree(root):
    out = {}
    for r, _, fs in os.walk(root):
        for f in fs:
            with open(os.path.join(r, f), "rb") as fh:
                out[os.path.relpath(os.path.join(r, f), root)] = fh.read()
    return out


def _main(encoder, raw, out, *extra):
    from realtime_codec_agent_amd import audio_to_codes
    return audio_to_codes.main(["--audio_path", raw, "--codes_path", out, "--super_batch_samples", "200000"] + list(extra), encoder=encoder, backend="gloo")


def test_cli_at_the_codec_rate_writes_the_default_tree(encoder, tmp_path):
    raw = str(tmp_path / "raw")
    _corpus(raw, 16000, [16000 * 3, 16000 * 5 + 700, 9000, 16000 * 2 + 1600, 40000, 1000], (16000, 16000 * 2 + 300))
    for stereo in ([], ["--stereo"]):
        ref = str(tmp_path / f"ref{len(stereo)}")
        s0 = _main(encoder, raw, ref, *stereo)
        want = _tree(ref)
        assert len(want) == 1 + (2 if stereo else 1) * 6 + 1 and s0["codes"] > 0
        for k, mode in enumerate(([], ["--one_file_at_a_time"])):
            out = str(tmp_path / f"ing{len(stereo)}{k}")
            s = _main(encoder, raw, out, "--device_ingest", *stereo, *mode)
            got = _tree(out)
            assert got.keys() == want.keys() and [f for f in want if want[f] != got[f]] == [] and s["codes"] == s0["codes"]
    assert encoder.stage_times["ingest_gpu_ms"] > 0.0


def test_cli_at_other_rates(encoder, tmp_path):
    """8 kHz stereo PCM16 files of 1-5 s and one 44.1 kHz mono file.  With --device_ingest the per-file tree is the pipelined tree;
    every file's codes are what the existing default path (HipWindowEncoder.encode on an f32 array) gives on that file's
    device-ingested rows; the code counts are the default (host-resample) run's.  The share of ids equal to the default run's is
    printed, not asserted: downmix-before-filter and another summation order move ids near ties, by an amount nobody has a floor for."""
    from realtime_codec_agent_amd.audio_to_codes import RawAudio, read_audio_raw
    raw = str(tmp_path / "raw")
    _corpus(raw, 8000, [8000 * 3, 8000 * 5 - 350, 8000, 8000 * 2 + 800, 20000, 500], (44100, 44100 * 2 + 300))
    chunk, ctx = 1600, 32000
    for stereo in ([], ["--stereo"]):
        outs = {k: str(tmp_path / f"{k}{len(stereo)}") for k in ("host", "file", "pipe")}
        s0 = _main(encoder, raw, outs["host"], *stereo)
        s1 = _main(encoder, raw, outs["file"], "--device_ingest", "--one_file_at_a_time", *stereo)
        s2 = _main(encoder, raw, outs["pipe"], "--device_ingest", *stereo)
        host, per_file, piped = _tree(outs["host"]), _tree(outs["file"]), _tree(outs["pipe"])
        assert per_file.keys() == piped.keys() == host.keys() and len(piped) == 1 + (2 if stereo else 1) * 6 + 1
        assert [f for f in piped if piped[f] != per_file[f]] == []
        assert s0["codes"] == s1["codes"] == s2["codes"] > 0
        leaf = os.path.join("MagiCodec-50Hz-Base", "0.1s_2.0s", "stereo" if stereo else "mono")
        equal = total = 0
        for r, _, fs in os.walk(raw):
            for f in fs:
                fsr, data, layout = read_audio_raw(os.path.join(r, f))
                rows = encoder.ingest(RawAudio(fsr, data, layout, not stereo, 16000)).cpu().numpy()
                want = encoder.encode(rows, chunk, ctx, 256)
                rel = os.path.splitext(os.path.relpath(os.path.join(r, f), raw))[0]
                for c in range(rows.shape[0]):
                    got = np.load(os.path.join(outs["pipe"], leaf, f"{rel}_c{c}.npy"))
                    ref = np.load(os.path.join(outs["host"], leaf, f"{rel}_c{c}.npy"))
                    assert got.dtype == np.int64 and np.array_equal(got, want[c][None, :]), (rel, c)
                    assert got.shape == ref.shape, (rel, c)
                    equal += int((got == ref).sum()); total += got.size
        print(f"device ingest vs host resample ({'stereo' if stereo else 'mono'}): {equal} of {total} ids equal = {equal / max(total, 1):.4f}")
