"""Streamed batch decode, the parts that need no GPU: the planner against CodeWindow.push and detokenize_audio's arithmetic step by
step, the plan executed on the host against the per-chunk loop (tiny oracle codec), and the CLI with an injected CPU decoder."""
import json
import os

import numpy as np
import pytest

from realtime_codec_agent_amd import codes_to_audio as c2a
from realtime_codec_agent_amd._native import JOIN_SEG
from realtime_codec_agent_amd.audio_tokenizer import CodeWindow
from realtime_codec_agent_amd.stream_decode import chunk_samples, join_host, plan_batch, plan_stream, run_plan_host
from realtime_codec_agent_amd.utils.audio_utils import create_crossfade_ramps, smooth_join
from tests.stream_decode_ref import stream_decode_loop

SR, FR, HOP, L = 16000, 50.0, 320, 320


def _steps(N, k, ctx, C=1, have=0):
    """(window frames, samples kept, first code of the window) per chunk, by pushing characters through CodeWindow."""
    win = CodeWindow(C, ctx * C)
    win.push("c" * (have * C))
    out = []
    for start in range(0, N, k):
        chunk = "x" * ((min(N, start + k) - start) * C)
        text = win.push(chunk)
        W = len(text) // C
        n = min(int(len(chunk) / (FR * C) * SR) + L, W * HOP)          # detokenize_audio: n_samples, then pcm[..., -n_samples:]
        out.append((W, n, have + min(N, start + k) - W))
    return out


@pytest.mark.parametrize("ctx", [10, 100, 300])
@pytest.mark.parametrize("k", [1, 3, 5, 7, 201])
@pytest.mark.parametrize("N", [1, 4, 37, 230, 450])
def test_planner_equals_the_loop_step_by_step(N, k, ctx):
    for C, have in ((1, 0), (2, 0), (1, 7), (1, 250)):
        ref = _steps(N, k, ctx, C, have)
        p = plan_stream(N, k, ctx, L, HOP, FR, SR, channels=C, have=have)
        assert list(zip(p.F.tolist(), p.n.tolist(), p.src.tolist())) == ref
        # the pieces lie back to back; each lands L before the end of the audio so far
        assert p.seg_off.tolist() == np.concatenate([[0], np.cumsum(p.n)[:-1]]).tolist()
        assert all(p.out_off[i + 1] == p.out_off[i] + p.n[i] - L for i in range(len(p.n) - 1))
        assert p.n_out == p.out_off[-1] + p.n[-1]
        # clipped windows name the same kept samples: same count, same last code, and still every frame those samples can see
        q = plan_stream(N, k, ctx, L, HOP, FR, SR, channels=C, have=have, dec_left=2)
        assert q.n.tolist() == p.n.tolist() and (q.src + q.F).tolist() == (p.src + p.F).tolist()
        assert np.all(q.F <= p.F) and np.all(q.F * HOP >= q.n)
        f0 = (p.F * HOP - p.n) // HOP
        assert q.F.tolist() == (p.F - np.maximum(0, f0 - 2)).tolist()
        if have == 0 and k < ctx and k != 201:                       # every later window has room for the preroll: N * hop samples
            assert p.n_out == N * HOP


def test_planner_uses_the_reference_sample_count_not_frames_times_hop():
    assert chunk_samples(201, FR, 1, SR, 0) == int(201 / FR * SR) == 64319 != 201 * HOP
    assert all(chunk_samples(k, FR, 1, SR, 0) == k * HOP for k in range(1, 201))
    p = plan_stream(450, 201, 300, L, HOP, FR, SR)
    assert p.F.tolist() == [201, 300, 300] and p.n.tolist() == [201 * HOP, 64319 + L, 48 * HOP + L]
    assert p.n_out == 450 * HOP - 1


def test_planner_flags_pieces_too_short_for_their_blends():
    assert plan_stream(37, 5, 10, L, HOP, FR, SR).joinable
    assert plan_stream(1, 5, 10, L, HOP, FR, SR).joinable
    assert not plan_stream(3, 1, 1, L, HOP, FR, SR).joinable           # window == chunk == 320 samples, the middle piece needs 640
    with pytest.raises(ValueError, match="shorter"):
        plan_batch([3], [0], 1, 1, L, HOP, FR, SR)


def test_join_host_is_chained_smooth_join():
    rng = np.random.default_rng(3)
    n_fade, fade_in, fade_out = create_crossfade_ramps(SR, 0.02)
    lens = [400, 640, 1000, 320]
    pieces = rng.standard_normal(sum(lens)).astype(np.float32)
    segs = np.zeros(len(lens), JOIN_SEG)
    segs["seg_off"], segs["n"] = np.concatenate([[0], np.cumsum(lens)[:-1]]), lens
    segs["out_off"] = np.concatenate([[0], np.cumsum(np.array(lens) - n_fade)[:-1]])
    segs["flags"][0], segs["flags"][-1] = 1, 2
    want = np.zeros(0, np.float32)
    for a, n in zip(segs["seg_off"], lens):
        want = smooth_join(want, pieces[a:a + n], n_fade, fade_in, fade_out)
    got = join_host(pieces, segs, n_fade, fade_in, np.full(len(want), np.nan, np.float32))
    assert np.array_equal(got, want)


@pytest.fixture(scope="module")
def tiny_codes():
    return np.random.default_rng(11).integers(0, 1024, size=(2, 37)).astype(np.int64)


@pytest.fixture(scope="module")
def tiny_loop(tiny_oracle, tiny_codes):
    """The per-chunk loop on the oracle, once per chunk size."""
    return {k: stream_decode_loop(tiny_oracle.decode, tiny_codes, k, 10, SR, FR)[0] for k in (1, 3, 5)}


@pytest.mark.parametrize("k", [1, 3, 5])
def test_clipped_windows_render_what_full_windows_render(tiny_oracle, tiny_codes, tiny_loop, k):
    fade_in = create_crossfade_ramps(SR, 0.02)[1]
    tail = lambda w, n: tiny_oracle.decode(w)[:, -n:]
    want = tiny_loop[k]
    assert want.shape == (2, 37 * HOP)
    for dec_left in (None, 2):
        plan = plan_batch([37, 37], [0, 0], k, 10, L, HOP, FR, SR, dec_left=dec_left)
        flat = run_plan_host(tail, tiny_codes.reshape(-1), plan, fade_in, batch=7)
        got = np.stack([flat[a:b] for a, b in plan.out_slices])
        assert np.array_equal(got, want), (k, dec_left)
    assert len(plan_batch([37], [0], k, 10, L, HOP, FR, SR, dec_left=2).groups) <= len(plan_batch([37], [0], k, 10, L, HOP, FR, SR).groups)


# ------------------------------------------------------------------------------------------------ the CLI on a CPU decoder
def _write_tree(root, cfg, rng):
    """A leaf as audio_to_codes writes it: stems of 37 codes (stereo), 1 code (stereo), 3 codes (mono), and one whose channels differ."""
    leaf = os.path.join(root, "tiny", "0.1s_0.2s", "stereo")
    files = {"a_c0": 37, "a_c1": 37, "sub/b_c0": 1, "sub/b_c1": 1, "sub/deep/c_c0": 3, "bad_c0": 5, "bad_c1": 4}
    codes = {}
    for rel, n in files.items():
        p = os.path.join(leaf, rel + ".npy")
        os.makedirs(os.path.dirname(p), exist_ok=True)
        codes[rel] = rng.integers(0, cfg.codebook_size, size=(1, n)).astype(np.int64)
        np.save(p, codes[rel])
    with open(os.path.join(leaf, "codec_info.json"), "w") as f:
        json.dump({"num_codebooks": 1, "codebook_size": cfg.codebook_size, "framerate": cfg.framerate}, f)
    return leaf, codes


def _tree_bytes(root):
    out = {}
    for d, _, files in os.walk(root):
        for f in files:
            with open(os.path.join(d, f), "rb") as fh:
                out[os.path.relpath(os.path.join(d, f), root)] = fh.read()
    return out


@pytest.fixture(scope="module")
def cpu_decoder(tiny_codec, tiny_oracle):
    return c2a.HostStreamDecoder(tiny_codec[0], lambda w, n: tiny_oracle.decode(w)[:, -n:])


@pytest.fixture(scope="module")
def code_tree(tmp_path_factory, tiny_codec):
    root = str(tmp_path_factory.mktemp("codes"))
    leaf, codes = _write_tree(root, tiny_codec[0], np.random.default_rng(5))
    return root, leaf, codes


@pytest.mark.parametrize("fmt", ["npy", "wav16"])
@pytest.mark.parametrize("stereo", [False, True])
def test_cli_pipelined_tree_equals_one_file_at_a_time_and_the_loop(tmp_path, code_tree, cpu_decoder, tiny_oracle, stereo, fmt):
    root, leaf, codes = code_tree
    common = ["--codes_path", root, "--chunk_size_secs", "0.1", "--context_secs", "0.2", "--format", fmt] + (["--stereo"] if stereo else [])
    a = c2a.main(common + ["--audio_path", str(tmp_path / "p"), "--super_batch_codes", "40", "--batch_size", "8"], decoder=cpu_decoder)
    b = c2a.main(common + ["--audio_path", str(tmp_path / "o"), "--one_file_at_a_time"], decoder=cpu_decoder)
    ta, tb = _tree_bytes(str(tmp_path / "p")), _tree_bytes(str(tmp_path / "o"))
    assert ta == tb
    ext = ".npy" if fmt == "npy" else ".wav"
    rel_leaf = os.path.relpath(leaf, root)
    if stereo:
        stems = {"a": ["a_c0", "a_c1"], "sub/b": ["sub/b_c0", "sub/b_c1"], "sub/deep/c": ["sub/deep/c_c0"]}
        assert len(a["refused"]) == len(b["refused"]) == 1 and os.path.join(leaf, "bad") in a["refused"][0] and "5, 4" in a["refused"][0]
    else:
        stems = {k: [k] for k in codes}                    # every channel file on its own, the unequal pair included
        assert a["refused"] == b["refused"] == []
    assert sorted(ta) == sorted(os.path.join(rel_leaf, s + ext) for s in stems)
    for stem, chans in stems.items():
        want = stream_decode_loop(tiny_oracle.decode, np.concatenate([codes[c] for c in chans]), 5, 10, SR, FR)[0]
        blob = ta[os.path.join(rel_leaf, stem + ext)]
        if fmt == "npy":
            got = np.load(os.path.join(str(tmp_path / "p"), rel_leaf, stem + ext))
            assert got.dtype == np.float32 and np.array_equal(got, want)
        else:
            q = np.rint(np.clip(want, -1.0, 1.0) * 32767.0).astype("<i2")
            assert blob[-q.size * 2:] == np.ascontiguousarray(q.T).tobytes() and len(blob) == 44 + q.size * 2
    assert a["codes"] == b["codes"] == sum(codes[c].size for cs in stems.values() for c in cs)


@pytest.mark.parametrize("field, value", [("codebook_size", 2048), ("framerate", 25.0), ("num_codebooks", 2)])
def test_cli_refuses_a_tree_of_another_codec(tmp_path, tiny_codec, cpu_decoder, field, value):
    leaf, _ = _write_tree(str(tmp_path / "codes"), tiny_codec[0], np.random.default_rng(1))
    info = json.load(open(os.path.join(leaf, "codec_info.json")))
    info[field] = value
    json.dump(info, open(os.path.join(leaf, "codec_info.json"), "w"))
    with pytest.raises(ValueError, match="codec_info.json"):
        c2a.main(["--codes_path", leaf, "--audio_path", str(tmp_path / "out")], decoder=cpu_decoder)
    assert not os.path.exists(str(tmp_path / "out"))
    with pytest.raises(ValueError, match="no codec_info.json"):
        c2a.main(["--codes_path", str(tmp_path / "nowhere"), "--audio_path", str(tmp_path / "out")], decoder=cpu_decoder)


def test_cli_takes_a_leaf_as_codes_path(tmp_path, code_tree, cpu_decoder):
    _, leaf, _ = code_tree
    c2a.main(["--codes_path", leaf, "--audio_path", str(tmp_path / "out"), "--chunk_size_secs", "0.1", "--context_secs", "0.2", "--format", "npy"],
             decoder=cpu_decoder)
    assert sorted(_tree_bytes(str(tmp_path / "out"))) == ["a_c0.npy", "a_c1.npy", "bad_c0.npy", "bad_c1.npy", "sub/b_c0.npy", "sub/b_c1.npy",
                                                          "sub/deep/c_c0.npy"]
