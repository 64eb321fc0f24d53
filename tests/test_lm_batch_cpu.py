"""LlamaBatch without a GPU: the wrapper's bookkeeping over a fake library object, and the three batch symbols in include/rca.h and
the binding.  (What a batch step computes is checked on the GPU, tests/test_lm_batch_gpu.py.)"""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("rca_lm_batch_create", "rca_lm_batch_destroy", "rca_lm_batch_step")


class FakeMember:
    """what LlamaBatch touches of a LlamaForAlternatingCodeChannels"""

    def __init__(self, handle, n_tokens, n_ctx=64):
        self._h = C.c_void_p(handle)
        self.n_tokens = n_tokens
        self._input_ids = np.zeros(n_ctx, dtype=np.intc)
        self._logits_valid = True


class FakeLib:
    """records the calls; rca_lm_batch_step advances the members as the library does and returns the sum of each member's ids"""

    def __init__(self, members, refuse_step=False):
        self.members, self.refuse_step = members, refuse_step
        self.created, self.destroyed, self.steps = [], 0, []

    def rca_lm_batch_create(self, handles, n, out):
        self.created.append([handles[i] for i in range(n)])
        out._obj.value = 0xBA7C
        return 0

    def rca_lm_batch_destroy(self, b):
        assert b.value == 0xBA7C
        self.destroyed += 1
        return 0

    def rca_lm_batch_step(self, b, ids, n, tokens):
        assert b.value == 0xBA7C
        self.steps.append((list(ids), n))
        if self.refuse_step:
            return -3
        for s, m in enumerate(self.members):
            tokens[s] = sum(ids[s * n:s * n + n])
            m.n_tokens += n
        return 0

    def rca_last_error(self):
        return b"batch_step: context overflow of member 1: 63 + 2 > n_ctx 64"


def _batch(members, **kw):
    from realtime_codec_agent_amd.llm import LlamaBatch
    lib = FakeLib(members, **kw)
    return LlamaBatch(members, lib=lib), lib


def test_step_records_ids_per_member_and_invalidates_logits():
    ms = [FakeMember(0x10 * (s + 1), 5 + 7 * s) for s in range(5)]
    bat, lib = _batch(ms)
    assert lib.created == [[0x10, 0x20, 0x30, 0x40, 0x50]]
    rows = [[10 * s + 1, 10 * s + 2] for s in range(5)]
    assert bat.step(rows) == [20 * s + 3 for s in range(5)]
    assert lib.steps == [([t for r in rows for t in r], 2)]      # ids [n_members][n], member-major
    for s, m in enumerate(ms):
        n0 = 5 + 7 * s
        assert m._input_ids[n0:n0 + 2].tolist() == rows[s]
        assert m._input_ids[:n0].sum() == 0 and m._input_ids[n0 + 2:].sum() == 0
        assert not m._logits_valid and m.n_tokens == n0 + 2
    assert bat.step([[s + 1] for s in range(5)]) == [1, 2, 3, 4, 5]   # a 5 x 1 step on the same batch, recorded behind the pairs
    assert [int(m._input_ids[5 + 7 * s + 2]) for s, m in enumerate(ms)] == [1, 2, 3, 4, 5]
    bat.close()
    bat.close()                                              # idempotent
    assert lib.destroyed == 1


def test_sixty_four_members_one_token_each():
    ms = [FakeMember(0x100 + s, s % 7, n_ctx=16) for s in range(64)]
    bat, lib = _batch(ms)
    assert bat.step([[100 + s] for s in range(64)]) == [100 + s for s in range(64)]
    assert lib.steps == [([100 + s for s in range(64)], 1)]
    for s, m in enumerate(ms):
        assert m._input_ids[s % 7] == 100 + s and m.n_tokens == s % 7 + 1


def test_a_refusal_is_raised_and_nothing_is_recorded():
    from realtime_codec_agent_amd import _native as N
    ms = [FakeMember(0x10, 5), FakeMember(0x20, 63), FakeMember(0x30, 9)]
    bat, lib = _batch(ms, refuse_step=True)
    # the error text comes from the real library's rca_last_error when it is built; the fake's return code is what matters here
    with pytest.raises(N.RcaError, match="rca_lm_batch_step failed"):
        bat.step([[7, 8], [9, 10], [11, 12]])
    assert all(m._input_ids.sum() == 0 and m._logits_valid for m in ms)
    assert [m.n_tokens for m in ms] == [5, 63, 9]


def test_ragged_or_miscounted_token_lists_never_reach_the_library():
    ms = [FakeMember(0x10, 5), FakeMember(0x20, 6)]
    bat, lib = _batch(ms)
    with pytest.raises(ValueError):
        bat.step([[1, 2], [3]])
    with pytest.raises(ValueError):
        bat.step([[1], [2], [3]])
    assert lib.steps == []


def test_batch_symbols_are_declared_bound_and_exported():
    from realtime_codec_agent_amd import _native
    header = open(os.path.join(ROOT, "include", "rca.h")).read()
    for sym in SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(" % sym, header), sym
        assert sym in _native.ABI_SYMBOLS, sym
    assert re.search(r"typedef\s+struct\s+rca_lm_batch\s+rca_lm_batch_t\s*;", header)
    assert "rca_lm_set_act_format does not apply" in header      # the header says what the activation format means for a batch
    import realtime_codec_agent_amd
    assert realtime_codec_agent_amd.LlamaBatch.__name__ == "LlamaBatch"
    if _native.needs_build():
        _native.build()
    lib = _native.lib()
    for sym in SYMBOLS:
        assert hasattr(lib, sym), sym
    # bad arguments are rejected before any HIP call
    assert lib.rca_lm_batch_create(None, 2, None) == -1 and b"null" in lib.rca_last_error()
    assert lib.rca_lm_batch_step(None, None, 1, None) == -1
    assert lib.rca_lm_batch_destroy(None) == 0
