"""The ctypes prototype of rca_lm_batch_step_sel follows its declaration in include/rca.h argument for argument, the entry point is
listed among the ABI symbols and the built library exports it; LlamaBatch.step_probe has the signature the driver calls."""
import ctypes as C
import os
import re

from realtime_codec_agent_amd import _native as N

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "rca.h")
CTYPES = {"rca_lm_batch_t*": C.c_void_p, "int32_t": C.c_int32, "int32_t*": C.POINTER(C.c_int32), "float*": C.POINTER(C.c_float)}


def _declared_args(sym):
    """[(name, ctype)] of `int <sym>(...)` in rca.h"""
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    args = re.search(r"\bint %s\((.*?)\);" % sym, text, re.S).group(1)
    out = []
    for a in args.split(","):
        m = re.match(r"\s*(?:const\s+)?(\w+)\s*(\*?)\s*(\w+)\s*$", a)
        out.append((m.group(3), CTYPES[m.group(1) + m.group(2)]))
    return out


def test_the_prototype_matches_the_header():
    want = _declared_args("rca_lm_batch_step_sel")
    assert [n for n, _ in want] == ["b", "sel", "n_sel", "ids", "n", "probe_ids", "n_probe", "tokens", "probs"]
    assert len(N.BATCH_STEP_SEL_ARGTYPES) == len(want)
    for (name, t), got in zip(want, N.BATCH_STEP_SEL_ARGTYPES):
        assert got is t, (name, got, t)


def test_the_entry_point_is_an_abi_symbol_bound_and_exported():
    assert "rca_lm_batch_step_sel" in N.ABI_SYMBOLS
    if N.needs_build():
        N.build()
    lib = N.lib()
    assert hasattr(lib, "rca_lm_batch_step_sel")
    assert list(lib.rca_lm_batch_step_sel.argtypes) == N.BATCH_STEP_SEL_ARGTYPES and lib.rca_lm_batch_step_sel.restype is C.c_int
    # bad arguments are rejected before any HIP call
    assert lib.rca_lm_batch_step_sel(None, None, 1, None, 1, None, 0, None, None) == -1 and b"batch_step_sel: null argument" in lib.rca_last_error()


def test_step_probe_takes_members_tokens_and_optional_probe_ids():
    import inspect
    from realtime_codec_agent_amd.llm import LlamaBatch
    p = inspect.signature(LlamaBatch.step_probe).parameters
    assert list(p)[1:] == ["members", "tokens_per_member", "probe_ids_per_member"] and p["probe_ids_per_member"].default is None
