"""The ctypes mirrors of rca_duplex_batch_args_t / rca_duplex_batch_out_t follow include/rca.h field for field, and every new entry
point is listed among the ABI symbols (the build checks the library exports each of them)."""
import ctypes as C
import os
import re

from realtime_codec_agent_amd import _native as N

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "rca.h")
CTYPES = {"int32_t": C.c_int32, "float": C.c_float}


def _struct_fields(name):
    """[(field, ctype)] of `typedef struct <name> { ... }` in rca.h; every pointer is a c_void_p"""
    text = open(HEADER).read()
    body = re.search(r"typedef struct %s \{(.*?)\} %s_t;" % (name, name), text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        m = re.match(r"(?:const\s+)?(\w+)\s*(\*?)\s*(.+)$", decl)
        ctype = C.c_void_p if m.group(2) or "*" in m.group(3) else CTYPES[m.group(1)]
        fields += [(f.strip().lstrip("*").strip(), ctype) for f in m.group(3).split(",")]
    return fields


def test_the_batch_structs_match_the_header():
    for name, mirror in (("rca_duplex_batch_args", N.DuplexBatchArgsC), ("rca_duplex_batch_out", N.DuplexBatchOutC)):
        want = _struct_fields(name)
        assert [(f, t) for f, t in mirror._fields_] == want, name
    assert C.sizeof(N.DuplexBatchArgsC) == 72 and C.sizeof(N.DuplexBatchOutC) == 40      # LP64: 5 pointers, 7 ints (+ padding) / 5 pointers
    assert N.DuplexBatchArgsC.T.offset == 48 and N.DuplexBatchArgsC.pcm_windows.offset == 16


def test_the_new_entry_points_are_abi_symbols_declared_in_the_header():
    text = open(HEADER).read()
    for sym in ("rca_lm_batch_frame_sel", "rca_lm_batch_captures", "rca_duplex_batch_frame"):
        assert sym in N.ABI_SYMBOLS, sym
        assert re.search(r"\bint %s\(" % sym, text), sym


def test_frame_takes_members_and_the_batch_offers_captures_and_duplex_frame():
    import inspect
    from realtime_codec_agent_amd.llm import LlamaBatch
    assert inspect.signature(LlamaBatch.frame).parameters["members"].default is None
    assert list(inspect.signature(LlamaBatch.duplex_frame).parameters)[1:] == [
        "codec_handle", "members", "pcm_windows", "code_ctxs", "n_steps", "n_samples", "code_token_base", "audio_id_floor", "probe_ids", "first_pairs"]
    assert callable(LlamaBatch.captures)
