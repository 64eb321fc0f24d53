"""The importance-matrix collector without a card: its C ABI (declared, exported, bound; null handles refused before any HIP call), the
tolerance condition of the GPU test against the restatement, and imatrix.collect / the tool over a stand-in LM."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import imatrix_collect_ref as CR  # noqa: E402
import imatrix_ref as IR  # noqa: E402

CALLS = ("rca_lm_imatrix_begin", "rca_lm_imatrix_chunk", "rca_lm_imatrix_get", "rca_lm_imatrix_end", "rca_lm_imatrix_chunk_tap")


# ------------------------------------------------------------------------------------------------------------------ 1. the ABI
def test_header_declares_library_exports_and_native_binds_the_collector():
    from realtime_codec_agent_amd import _native as N
    if N.needs_build():
        N.build()
    lib = N.lib()
    header = open(os.path.join(ROOT, "include", "rca.h")).read()
    for sym in CALLS:
        assert re.search(r"\bint\s+" + sym + r"\s*\(\s*rca_lm_t\s*\*\s*h\b", header), sym
        assert sym in N.ABI_SYMBOLS, sym
        assert hasattr(lib, sym), sym
        assert getattr(lib, sym).argtypes is not None and getattr(lib, sym).restype is ctypes.c_int, sym
    assert "No pass launches it yet" not in header
    # null handles are refused before any HIP call (this machine may have no GPU at all)
    ids = np.zeros(4, np.int32)
    buf = np.zeros(256, np.float64)
    planes = np.zeros((4, 256), np.uint16)
    count = ctypes.c_int64(-7)
    for rc in (lib.rca_lm_imatrix_begin(None), lib.rca_lm_imatrix_end(None), lib.rca_lm_imatrix_chunk(None, ids.ctypes.data, 4),
               lib.rca_lm_imatrix_get(None, 0, 0, buf.ctypes.data, 256, ctypes.byref(count)),
               lib.rca_lm_imatrix_chunk_tap(None, ids.ctypes.data, 4, 0, 0, planes.ctypes.data, planes.ctypes.data)):
        assert rc == -1 and b"null" in lib.rca_last_error()
    assert count.value == -7 and not buf.any() and not planes.any()


# ------------------------------------------------------------------------------------------------------------------ 2. the tolerance condition
def test_the_restatement_tells_slots_apart_and_the_definition_sits_on_it():
    """d_min, the smallest relative L2 distance between two of the restatement's vectors of equal width, is what a mis-wired slot would
    show at the least: it has to stay far above the d_min / 10 the GPU test allows (measured: 0.112, kind 0 of layer 0 against kind 0 of
    layer 1).  And the device's definition (bf16 hi + lo planes, f32 sums per 128 rows: imatrix_ref.collect) over the restatement's own
    final-norm rows lies within d_min / 1000 per column of the float64 sums (measured: 9.1e-7), so the definition's own rounding takes
    none of that allowance."""
    ref = CR.restatement()
    assert ref.count == sum(CR.PARTS) == 1194 and sorted(ref.sums) == sorted(CR.PAIRS)
    for (l, k), v in ref.sums.items():
        assert v.shape == (CR.width(ref.cfg, k),) and np.isfinite(v).all() and (v > 0).all(), (l, k)
    d, where = CR.d_min(ref.sums)
    print(f"d_min = {d:.4f} between (layer, kind) {where[0]} and {where[1]}")
    assert d > 0.05, (d, where)
    acc = np.zeros(ref.cfg.hidden, np.float64)
    for rows in ref.final_rows:
        for r0 in range(0, len(rows), 1024):                # the passes of a chunk
            xh, xl = IR.split_planes(rows[r0:r0 + 1024])
            acc = IR.collect(xh, xl, len(xh), acc)
    err = float(np.max(np.abs(acc - ref.sums[(0, 4)]) / ref.sums[(0, 4)]))
    print(f"definition against float64 sums, final-norm rows: max relative error per column {err:.3g}")
    assert err <= d / 1000, (err, d)


# ------------------------------------------------------------------------------------------------------------------ 3. collect over a stand-in
class FakeLM:
    """What imatrix.collect and the tool touch of a handle, with sums a test can predict: a chunk adds, to column j of (layer, kind),
    (1 + layer + 10 * kind + j) * sum(token + 1) -- and position-dependent nothing, but it records n_tokens at every call."""

    def __init__(self, n_ctx=64, n_layers=2):
        from realtime_codec_agent_amd.llm import LlamaForAlternatingCodeChannels, LMConfig
        self.config = LMConfig(vocab_size=1000, hidden=8, n_layers=n_layers, n_heads=2, n_kv_heads=1, head_dim=6, ffn=16)
        self._n_ctx, self.n_tokens, self.acc, self.count = n_ctx, 0, None, 0
        self.log, self.chunks, self.closed = [], [], False
        self._real = LlamaForAlternatingCodeChannels

    def n_ctx(self):
        return self._n_ctx

    def reset(self):
        self.log.append("reset")
        self.n_tokens = 0

    def close(self):
        self.closed = True

    def _imatrix_width(self, kind):
        return self._real._imatrix_width(self, kind)

    def imatrix_begin(self):
        assert self.acc is None
        self.log.append("begin")
        self.acc = {(l, k): np.zeros(self._imatrix_width(k)) for l in range(self.config.n_layers) for k in range(4)}
        self.acc[(0, 4)] = np.zeros(self.config.hidden)
        self.count = 0

    def imatrix_chunk(self, tokens):
        tokens = np.asarray(tokens)
        assert self.acc is not None and tokens.dtype == np.int32 and self.n_tokens + len(tokens) <= self._n_ctx
        self.log.append(("chunk", self.n_tokens, len(tokens)))
        self.chunks.append(tokens.copy())
        for (l, k), v in self.acc.items():
            v += (1 + l + 10 * k + np.arange(len(v))) * float(np.sum(tokens + 1))
        self.n_tokens += len(tokens)
        self.count += len(tokens)

    def imatrix_get(self, layer, kind, width=None):
        return self.acc[(0 if kind == 4 else layer, kind)].copy(), self.count

    def imatrix_read(self):
        self.log.append("read")
        return self._real.imatrix_read(self)

    def imatrix_end(self):
        self.log.append("end")
        self.acc = None


def _expected(chunks, l, k, K):
    return (1 + l + 10 * k + np.arange(K)) * float(sum(np.sum(c + 1) for c in chunks))


def test_collect_cuts_chunks_drops_tails_and_names_the_entries():
    from realtime_codec_agent_amd import imatrix as I
    streams = [np.arange(0, 50, dtype=np.int32), np.arange(100, 107, dtype=np.int32), np.arange(200, 233, dtype=np.int32)]
    llm = FakeLM(n_ctx=64)
    said = []
    imx = I.collect(llm, streams, chunk=16, report=said.append)
    want = [streams[0][0:16], streams[0][16:32], streams[0][32:48], streams[2][0:16], streams[2][16:32]]   # tails of 2, 7 and 1 dropped
    assert len(llm.chunks) == 5 and all(np.array_equal(a, b) for a, b in zip(llm.chunks, want))
    assert llm.log == ["begin"] + ["reset", ("chunk", 0, 16)] * 5 + ["read", "end"]           # one reset per chunk, each from n_tokens 0
    assert said and said[-1] == "chunk 5 / 5"
    assert isinstance(imx, I.Imatrix) and imx.chunk_count == 5 and imx.chunk_size == 16
    c = llm.config
    assert len(imx) == 7 * c.n_layers + 1
    widths = {0: c.hidden, 1: c.n_heads * c.head_dim, 2: c.hidden, 3: c.ffn}
    assert widths[1] == 12 and widths[3] == 16
    for l in range(c.n_layers):
        for kind, names in IR.NAMES.items():
            for n in names:
                sums, count = imx[f"blk.{l}.{n}.weight"]
                assert count == 80 and sums.dtype == np.float64 and np.array_equal(sums, _expected(want, l, kind, widths[kind])), (l, n)
        assert imx[f"blk.{l}.attn_q.weight"][0] is not imx[f"blk.{l}.attn_k.weight"][0]       # shared values, not one shared array
    sums, count = imx["output.weight"]
    assert count == 80 and np.array_equal(sums, _expected(want, 0, 4, c.hidden))
    assert I.KIND_NAMES == IR.NAMES


def test_collect_max_chunks_and_refusals():
    from realtime_codec_agent_amd import imatrix as I
    streams = [np.arange(0, 50, dtype=np.int32), np.arange(200, 233, dtype=np.int32)]
    llm = FakeLM(n_ctx=64)
    imx = I.collect(llm, streams, chunk=16, max_chunks=4)
    assert imx.chunk_count == 4 and imx.chunk_size == 16 and imx["output.weight"][1] == 64 and llm.log.count("reset") == 4
    assert np.array_equal(llm.chunks[3], streams[1][0:16])
    llm = FakeLM(n_ctx=64)
    with pytest.raises(ValueError, match=r"chunk of 65 tokens does not fit n_ctx = 64"):
        I.collect(llm, [np.arange(300, dtype=np.int32)], chunk=65)
    assert llm.log == []                                                                      # before any device call
    with pytest.raises(ValueError, match=r"no stream holds a whole chunk"):
        I.collect(llm, [np.arange(10, dtype=np.int32)], chunk=16)
    assert llm.log == []
    imx = I.collect(llm, [np.arange(64, dtype=np.int32)], chunk=64)                           # chunk == n_ctx is fine
    assert imx.chunk_count == 1 and imx["output.weight"][1] == 64

    class Nan(FakeLM):
        def imatrix_get(self, layer, kind, width=None):
            s, c = super().imatrix_get(layer, kind)
            if (layer, kind) == (1, 3):
                s[5] = np.inf
            return s, c

    bad = Nan()
    with pytest.raises(ValueError, match=r"layer 1, kind 3 \(ffn_down\): a sum is not finite"):
        I.collect(bad, [np.arange(64, dtype=np.int32)], chunk=16)
    assert bad.log[-1] == "end"                                                               # the collection is ended all the same


# ------------------------------------------------------------------------------------------------------------------ 4. the tool
def test_cli_writes_a_file_and_merges_prior_files(tmp_path, capsys):
    from realtime_codec_agent_amd import imatrix as I
    d = tmp_path / "ids"
    d.mkdir()
    np.save(d / "a.npy", np.arange(0, 50, dtype=np.int32))
    np.save(d / "b.npy", np.arange(200, 233, dtype=np.int64))
    made = []

    def make(a):
        made.append(FakeLM(n_ctx=a.chunk))
        return made[-1]

    first = str(tmp_path / "first.gguf")
    assert I.main(["--model", "none", "--ids", str(d), "--out", first, "--chunk", "16", "--dataset", "corpus A"], make_llm=make) == 0
    out = capsys.readouterr().out
    assert "15 entries, 5 chunks of 16 tokens" in out and re.search(r"collected 80 tokens in .* tokens / s", out)
    assert made[0].closed and made[0].n_ctx() == 16
    a = I.read_imatrix_gguf(first)
    assert len(a) == 15 and a.chunk_count == 5 and a.chunk_size == 16 and a.datasets == ["corpus A"]
    want = made[0].chunks
    for name, (l, k, K) in {"blk.1.ffn_down.weight": (1, 3, 16), "blk.0.attn_v.weight": (0, 0, 8), "output.weight": (0, 4, 8)}.items():
        sums, count = a[name]
        assert count == 80 and np.array_equal(sums, _expected(want, l, k, K).astype(np.float32).astype(np.float64)), name
    # a second run over one file of the corpus, two chunks at the most, with the first file merged in
    second = str(tmp_path / "second.gguf")
    assert I.main(["--model", "none", "--ids", str(d / "b.npy"), "--out", second, "--chunk", "16", "--chunks", "2", "--in_file", first],
                  make_llm=make) == 0
    assert "15 entries, 7 chunks of 16 tokens (1 merged in)" in capsys.readouterr().out
    b = I.read_imatrix_gguf(second)
    assert len(b) == 15 and b.chunk_count == 7 and b.chunk_size == 16 and b.datasets == ["corpus A", str(d / "b.npy")]
    assert len(made[1].chunks) == 2
    for name, (l, k, K) in {"blk.1.ffn_down.weight": (1, 3, 16), "blk.0.attn_q.weight": (0, 0, 8), "output.weight": (0, 4, 8)}.items():
        sums, count = b[name]
        both = a[name][0] + _expected(made[1].chunks, l, k, K)
        assert count == 80 + 32 and np.array_equal(sums, both.astype(np.float32).astype(np.float64)), name
