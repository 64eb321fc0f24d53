"""LlamaBatch.frame without a GPU: the wrapper's bookkeeping over a fake library object, and rca_lm_batch_frame in include/rca.h, the
binding and the built library.  (What a batch frame computes is checked on the GPU, tests/test_lm_batch_frame_gpu.py.)"""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class FakeMember:
    """what LlamaBatch touches of a LlamaForAlternatingCodeChannels"""

    def __init__(self, handle, n_tokens, n_ctx=64):
        self._h = C.c_void_p(handle)
        self.n_tokens = n_tokens
        self._input_ids = np.zeros(n_ctx, dtype=np.intc)
        self._logits_valid = True


class FakeLib:
    """records the calls; rca_lm_batch_frame samples 1000 + 10 * member - step, cuts a member at the first token <= audio_id_floor,
    advances the members as the library does and answers a probe with (member + 1) / 100"""

    def __init__(self, members, refuse=False):
        self.members, self.refuse, self.frames = members, refuse, []

    def rca_lm_batch_create(self, handles, n, out):
        out._obj.value = 0xBA7C
        return 0

    def rca_lm_batch_destroy(self, b):
        return 0

    def rca_lm_batch_frame(self, b, first_pairs, user_ids, n_steps, floor, probe_ids, out_tokens, n_done, probe_probs):
        assert b.value == 0xBA7C
        nm = len(self.members)
        self.frames.append(dict(pairs=list(first_pairs), users=list(user_ids), n_steps=n_steps, floor=floor,
                                probes=None if probe_ids is None else list(probe_ids), has_probs=probe_probs is not None,
                                sizes=(len(first_pairs), len(user_ids), len(out_tokens), len(n_done))))
        if self.refuse:
            return -3
        for s, m in enumerate(self.members):
            done = n_steps
            for i in range(n_steps):
                out_tokens[s * n_steps + i] = -1
            for i in range(n_steps):
                out_tokens[s * n_steps + i] = 1000 + 10 * s - i
                if out_tokens[s * n_steps + i] <= floor:
                    done = i + 1
                    break
            n_done[s] = done
            m.n_tokens += 2 * done
            if probe_ids is not None:
                probe_probs[s] = -1.0 if done < n_steps or probe_ids[s] < 0 else (s + 1) / 100
        return 0

    def rca_last_error(self):
        return b"batch_frame: context overflow of member 1: 60 + 8 > n_ctx 64"


def _batch(members, **kw):
    from realtime_codec_agent_amd.llm import LlamaBatch
    lib = FakeLib(members, **kw)
    return LlamaBatch(members, lib=lib), lib


def test_frame_lays_out_its_arguments_member_major_and_records_what_was_evaluated():
    ms = [FakeMember(0x10 * (s + 1), 5 + 7 * s) for s in range(3)]
    bat, lib = _batch(ms)
    pairs = [[100 + s, 200 + s] for s in range(3)]
    users = [[300 + 10 * s + i for i in range(4)] for s in range(3)]
    toks, probs = bat.frame(pairs, users, -1)
    assert probs is None
    assert toks == [[1000 + 10 * s - i for i in range(4)] for s in range(3)]
    (call,) = lib.frames
    assert call["pairs"] == [100, 200, 101, 201, 102, 202]                       # [n_members][2]
    assert call["users"] == [t for u in users for t in u]                        # [n_members][n_steps]
    assert call["n_steps"] == 4 and call["floor"] == -1 and call["probes"] is None and not call["has_probs"]
    assert call["sizes"] == (6, 12, 12, 3)
    for s, m in enumerate(ms):
        n0 = 5 + 7 * s
        want = pairs[s] + [t for i in range(3) for t in (toks[s][i], users[s][i])]      # first_pair + interleave(tokens[:-1], user_ids)
        assert m.n_tokens == n0 + 8
        assert m._input_ids[n0:n0 + 8].tolist() == want
        assert m._input_ids[:n0].sum() == 0 and m._input_ids[n0 + 8:].sum() == 0
        assert not m._logits_valid


def test_cut_members_return_shorter_lists_and_nan_probes():
    ms = [FakeMember(0x10 * (s + 1), 4) for s in range(3)]
    bat, lib = _batch(ms)
    pairs = [[1, 2], [3, 4], [5, 6]]
    users = [[10, 11, 12], [20, 21, 22], [30, 31, 32]]
    # floor 1009: member 0 is cut by its first token (1000), member 1 by its second (1010, 1009), member 2 (1020, 1019, 1018) is complete
    toks, probs = bat.frame(pairs, users, 1009, probe_ids=[7, 7, -1])
    assert toks == [[1000], [1010, 1009], [1020, 1019, 1018]]
    assert lib.frames[0]["probes"] == [7, 7, -1] and lib.frames[0]["has_probs"]
    assert probs.dtype == np.float32 and probs.shape == (3,) and np.isnan(probs).all()     # cut, cut, no probe id
    assert [m.n_tokens for m in ms] == [6, 8, 10]
    assert ms[0]._input_ids[4:8].tolist() == [1, 2, 0, 0]
    assert ms[1]._input_ids[4:10].tolist() == [3, 4, 1010, 20, 0, 0]
    assert ms[2]._input_ids[4:11].tolist() == [5, 6, 1020, 30, 1019, 31, 0]
    assert not any(m._logits_valid for m in ms)
    # uncut, with probes: the library's numbers come back as float32
    toks, probs = bat.frame(pairs, users, -1, probe_ids=[7, -1, 9])
    assert [len(t) for t in toks] == [3, 3, 3]
    assert probs[0] == np.float32(0.01) and np.isnan(probs[1]) and probs[2] == np.float32(0.03)


def test_shape_errors_never_reach_the_library():
    ms = [FakeMember(0x10, 5), FakeMember(0x20, 6)]
    bat, lib = _batch(ms)
    for pairs, users, probes in (
        ([[1, 2], [3]], [[4], [5]], None),                  # a first pair of one id
        ([[1, 2], [3, 4, 5]], [[4], [5]], None),            # ... of three
        ([[1, 2]], [[4], [5]], None),                       # one pair for two members
        ([[1, 2], [3, 4]], [[4, 6], [5]], None),            # n_steps differs between members
        ([[1, 2], [3, 4]], [[4]], None),                    # one user list for two members
        ([[1, 2], [3, 4]], [[4], [5]], [7]),                # one probe id for two members
    ):
        with pytest.raises(ValueError):
            bat.frame(pairs, users, -1, probe_ids=probes)
    assert lib.frames == []
    assert all(m._input_ids.sum() == 0 and m._logits_valid for m in ms) and [m.n_tokens for m in ms] == [5, 6]


def test_a_refusal_is_raised_and_nothing_is_recorded():
    from realtime_codec_agent_amd import _native as N
    ms = [FakeMember(0x10, 5), FakeMember(0x20, 60), FakeMember(0x30, 9)]
    bat, lib = _batch(ms, refuse=True)
    # the error text comes from the real library's rca_last_error when it is built; the fake's return code is what matters here
    with pytest.raises(N.RcaError, match="rca_lm_batch_frame failed"):
        bat.frame([[7, 8], [9, 10], [11, 12]], [[1, 2, 3, 4]] * 3, -1)
    assert len(lib.frames) == 1
    assert all(m._input_ids.sum() == 0 and m._logits_valid for m in ms)
    assert [m.n_tokens for m in ms] == [5, 60, 9]


def test_batch_frame_is_declared_bound_and_exported():
    from realtime_codec_agent_amd import _native
    header = open(os.path.join(ROOT, "include", "rca.h")).read()
    sym = "rca_lm_batch_frame"
    assert re.search(r"\bint\s+%s\s*\(" % sym, header)
    assert sym in _native.ABI_SYMBOLS
    import realtime_codec_agent_amd
    assert callable(realtime_codec_agent_amd.LlamaBatch.frame)
    if _native.needs_build():
        _native.build()
    lib = _native.lib()
    assert hasattr(lib, sym)
    # bad arguments are rejected before any HIP call
    assert lib.rca_lm_batch_frame(None, None, None, 4, -1, None, None, None, None) == -1 and b"null" in lib.rca_last_error()
