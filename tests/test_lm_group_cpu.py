"""LlamaGroup without a GPU: the wrapper's bookkeeping over a fake library object, and the three group symbols in include/rca.h and
the binding.  (What a group step computes is checked on the GPU, tests/test_lm_group_gpu.py.)"""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("rca_lm_group_create", "rca_lm_group_destroy", "rca_lm_group_step")


class FakeMember:
    """what LlamaGroup touches of a LlamaForAlternatingCodeChannels"""

    def __init__(self, handle, n_tokens, n_ctx=64):
        self._h = C.c_void_p(handle)
        self.n_tokens = n_tokens
        self._input_ids = np.zeros(n_ctx, dtype=np.intc)
        self._logits_valid = True


class FakeLib:
    """records the calls; rca_lm_group_step advances the members as the library does and returns the sum of each member's ids"""

    def __init__(self, members, refuse_step=False):
        self.members, self.refuse_step = members, refuse_step
        self.created, self.destroyed, self.steps = [], 0, []

    def rca_lm_group_create(self, handles, n, out):
        self.created.append([handles[i] for i in range(n)])
        out._obj.value = 0xBEEF
        return 0

    def rca_lm_group_destroy(self, g):
        assert g.value == 0xBEEF
        self.destroyed += 1
        return 0

    def rca_lm_group_step(self, g, ids, n, tokens):
        assert g.value == 0xBEEF
        self.steps.append((list(ids), n))
        if self.refuse_step:
            return -3
        for s, m in enumerate(self.members):
            tokens[s] = sum(ids[s * n:s * n + n])
            m.n_tokens += n
        return 0

    def rca_last_error(self):
        return b"group_step: context overflow of member 1: 63 + 2 > n_ctx 64"


def _group(members, **kw):
    from realtime_codec_agent_amd.llm import LlamaGroup
    lib = FakeLib(members, **kw)
    return LlamaGroup(members, lib=lib), lib


def test_step_records_ids_per_member_and_invalidates_logits():
    ms = [FakeMember(0x10, 5), FakeMember(0x20, 40)]
    grp, lib = _group(ms)
    assert lib.created == [[0x10, 0x20]]
    assert grp.step([[7, 8], [9, 10]]) == [15, 19]
    assert lib.steps == [([7, 8, 9, 10], 2)]                 # ids [n_members][n], member-major
    assert ms[0]._input_ids[5:7].tolist() == [7, 8] and ms[1]._input_ids[40:42].tolist() == [9, 10]
    assert ms[0]._input_ids[:5].tolist() == [0] * 5 and ms[1]._input_ids[42:].sum() == 0
    assert not ms[0]._logits_valid and not ms[1]._logits_valid
    assert (ms[0].n_tokens, ms[1].n_tokens) == (7, 42)
    assert grp.step([[1], [2]]) == [1, 2]                    # a 2 x 1 step on the same group, recorded behind the pair
    assert ms[0]._input_ids[7] == 1 and ms[1]._input_ids[42] == 2
    grp.close()
    grp.close()                                              # idempotent
    assert lib.destroyed == 1


def test_four_members_one_token_each():
    ms = [FakeMember(0x10 * (s + 1), 3 * s) for s in range(4)]
    grp, lib = _group(ms)
    assert grp.step([[11], [12], [13], [14]]) == [11, 12, 13, 14]
    assert lib.steps == [([11, 12, 13, 14], 1)]
    for s, m in enumerate(ms):
        assert m._input_ids[3 * s] == 11 + s and m.n_tokens == 3 * s + 1


def test_a_refusal_is_raised_and_nothing_is_recorded():
    from realtime_codec_agent_amd import _native as N
    ms = [FakeMember(0x10, 5), FakeMember(0x20, 63)]
    grp, lib = _group(ms, refuse_step=True)
    # the error text comes from the real library's rca_last_error when it is built; the fake's return code is what matters here
    with pytest.raises(N.RcaError, match="rca_lm_group_step failed"):
        grp.step([[7, 8], [9, 10]])
    assert ms[0]._input_ids.sum() == 0 and ms[1]._input_ids.sum() == 0
    assert ms[0]._logits_valid and ms[1]._logits_valid
    assert (ms[0].n_tokens, ms[1].n_tokens) == (5, 63)


def test_ragged_or_miscounted_token_lists_never_reach_the_library():
    ms = [FakeMember(0x10, 5), FakeMember(0x20, 6)]
    grp, lib = _group(ms)
    with pytest.raises(ValueError):
        grp.step([[1, 2], [3]])
    with pytest.raises(ValueError):
        grp.step([[1], [2], [3]])
    assert lib.steps == []


def test_group_symbols_are_declared_bound_and_exported():
    from realtime_codec_agent_amd import _native
    header = open(os.path.join(ROOT, "include", "rca.h")).read()
    for sym in SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(" % sym, header), sym
        assert sym in _native.ABI_SYMBOLS, sym
    assert re.search(r"typedef\s+struct\s+rca_lm_group\s+rca_lm_group_t\s*;", header)
    import realtime_codec_agent_amd
    assert realtime_codec_agent_amd.LlamaGroup.__name__ == "LlamaGroup"
    if _native.needs_build():
        _native.build()
    lib = _native.lib()
    for sym in SYMBOLS:
        assert hasattr(lib, sym), sym
    # bad arguments are rejected before any HIP call
    assert lib.rca_lm_group_create(None, 2, None) == -1 and b"null" in lib.rca_last_error()
    assert lib.rca_lm_group_step(None, None, 1, None) == -1
    assert lib.rca_lm_group_destroy(None) == 0
