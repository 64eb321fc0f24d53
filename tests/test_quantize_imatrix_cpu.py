"""The weighted quantisers (rca_quantize_rows_w), the parts that need no card: the C++ the device kernel calls (csrc/rca_quant_rows.h)
built for the host under AddressSanitizer / UBSan against the numpy definition tests/quant_weighted_ref.py, byte for byte; and the
condition the weights exist for -- under the weights, the weighted rule loses less than today's search."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import quant_search_ref as R  # noqa: E402
import quant_weighted_ref as W  # noqa: E402

RCA_TYPE = {"q4_k": 4, "q5_k": 6, "q6_k": 5}
TYPES = ("q4_k", "q5_k", "q6_k")
MATRICES = ("gaussian", "student_t4", "laplace")


def _draw(rs, shape):
    return {"gaussian": rs.randn(*shape), "student_t4": rs.standard_t(4, shape), "laplace": rs.laplace(size=shape)}


@functools.lru_cache(maxsize=None)
def _host_program():
    """tests/quant_rows_w_host.cpp over csrc/rca_quant_rows.h, built by ROCm's clang with AddressSanitizer and UBSan (host code only)"""
    import shutil
    import tempfile
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    cands = [os.path.join(os.path.dirname(os.path.realpath(hipcc)), "..", "llvm", "bin", "clang++"), "/opt/rocm/llvm/bin/clang++",
             shutil.which("clang++") or ""]
    clang = next((c for c in cands if c and os.path.exists(c)), None)
    assert clang, "no clang++ next to hipcc: the host build of csrc/rca_quant_rows.h needs the compiler that has _Float16"
    out = os.path.join(tempfile.mkdtemp(prefix="quant_rows_w_host_"), "quant_rows_w_host")
    cmd = [clang, "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-I", os.path.join(root, "realtime_codec_agent_amd", "csrc"), os.path.join(root, "tests", "quant_rows_w_host.cpp"), "-o", out]
    p = subprocess.run(cmd, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    return out


def _host_run(w, qtype, qw, tmp_path):
    src, wts, dst = str(tmp_path / "in.f32"), str(tmp_path / "qw.f32"), str(tmp_path / "out.bin")
    np.ascontiguousarray(w, np.float32).tofile(src)
    np.ascontiguousarray(qw, np.float32).tofile(wts)
    p = subprocess.run([_host_program(), str(RCA_TYPE[qtype]), str(w.shape[0]), str(w.shape[1]), src, wts, dst], capture_output=True, text=True)
    assert p.returncode == 0, p.stdout + p.stderr            # a sanitizer report ends the program with another status
    words = p.stdout.split()
    return np.fromfile(dst, np.uint8).reshape(w.shape[0], -1), int(words[1]), int(words[3]), int(words[5])


@pytest.mark.parametrize("qtype", TYPES)
def test_the_weighted_cxx_on_the_host_is_the_numpy_definition_and_clean_under_sanitizers(qtype, tmp_path):
    """Seeded Gaussian / Student-t(4) / Laplace matrices of 64 x 1024 under qw = exp(randn), and every edge block under random weights:
    the same bytes, status 0, no sanitizer report (the program owns exactly K weights and exactly the blocks' bytes)."""
    rs = np.random.RandomState(21)
    mats = {k: (v * 0.02).astype(np.float32) for k, v in _draw(rs, (64, 1024)).items()}
    qw = np.exp(rs.randn(1024)).astype(np.float32)
    for name, w in mats.items():
        got, status, _, _ = _host_run(w, qtype, qw, tmp_path)
        want = W.quantize_blocks_w(w, qtype, qw)
        assert status == 0 and got.shape == want.shape and np.array_equal(got, want), name
        assert np.isfinite(R.dequantize(got, qtype)).all()
    edges = np.stack([R.edge_block(k) for k in R.EDGE_BLOCKS])
    qe = np.exp(rs.randn(256)).astype(np.float32)
    got, status, _, _ = _host_run(edges, qtype, qe, tmp_path)
    assert status == 0 and np.array_equal(got, W.quantize_blocks_w(edges, qtype, qe))
    deq = R.dequantize(got, qtype).reshape(edges.shape)
    assert np.isfinite(deq).all() and not got[0].any()                 # the all-zero block is all-zero bytes under weights too


@pytest.mark.parametrize("qtype", TYPES)
def test_groups_whose_weights_are_all_zero_use_one(qtype, tmp_path):
    """A sub-block of 32 and a group of 16 with all-zero weights: the bytes of the definition, which are those of weights 1.0 there."""
    rs = np.random.RandomState(22)
    w = (rs.randn(4, 512) * 0.02).astype(np.float32)
    qw = np.exp(rs.randn(512)).astype(np.float32)
    qw[64:96] = 0.0          # a whole Q4_K / Q5_K sub-block (two Q6_K groups)
    qw[304:320] = 0.0        # one Q6_K group: half a sub-block, whose other half keeps its weights
    qw[7] = 0.0              # a single zero stays a zero
    got, status, _, _ = _host_run(w, qtype, qw, tmp_path)
    assert status == 0 and np.array_equal(got, W.quantize_blocks_w(w, qtype, qw))
    ones = qw.copy()
    ones[64:96] = 1.0
    if qtype == "q6_k":
        ones[304:320] = 1.0
    assert np.array_equal(got, W.quantize_blocks_w(w, qtype, ones))
    other = ones.copy()
    other[64:96] = 2.0 ** np.arange(32)
    assert not np.array_equal(got, W.quantize_blocks_w(w, qtype, other))          # (the weights there do matter)


@pytest.mark.parametrize("qtype", TYPES)
def test_weights_are_indexed_by_column_not_by_block(qtype, tmp_path):
    """3 x 512 with the two halves of qw 1e6 apart: block b of the matrix reads the weights of column block b % 2.  A lane that indexes the
    weights by its block number reads past the K weights from the third block on (an AddressSanitizer report) and gives other bytes."""
    rs = np.random.RandomState(23)
    w = (rs.standard_t(4, (3, 512)) * 0.02).astype(np.float32)
    qw = np.exp(rs.randn(512)).astype(np.float32)
    qw[256:] *= np.float32(1e6)
    got, status, _, _ = _host_run(w, qtype, qw, tmp_path)
    want = W.quantize_blocks_w(w, qtype, qw)
    assert status == 0 and np.array_equal(got, want)
    swapped = W.quantize_blocks_w(w, qtype, np.concatenate([qw[256:], qw[:256]]))
    assert not np.array_equal(want, swapped)


@pytest.mark.parametrize("qtype", TYPES)
def test_values_no_fp16_scale_can_hold_and_nan_set_the_status_bits(qtype, tmp_path):
    rs = np.random.RandomState(24)
    w = (rs.randn(8, 512) * 0.02).astype(np.float32)
    qw = np.exp(rs.randn(512)).astype(np.float32)
    bad = w.copy()
    bad[5, 300], bad[6, 1] = np.inf, np.nan
    _, status, bad_in, _ = _host_run(bad, qtype, qw, tmp_path)
    assert status & 1 and bad_in == 5
    bad = w.copy()
    bad[3, 17] = 1e9
    _, status, bad_in, bad_d = _host_run(bad, qtype, qw, tmp_path)
    assert status == 2 and bad_in == -1 and bad_d == 3
    with pytest.raises(R.QuantError, match=r"t: row 3.*not finite in fp16"):
        W.quantize_blocks_w(bad, qtype, qw, name="t")
    for v in (-1.0, np.nan, np.inf):
        q2 = qw.copy()
        q2[130] = v
        with pytest.raises(R.QuantError, match="column 130"):
            W.quantize_blocks_w(w, qtype, q2)


# ------------------------------------------------------------------------------------------------------------------ the weighted error
@functools.lru_cache(maxsize=None)
def _matrix(name):
    """the three seeded 256 x 2048 matrices, scale 0.02, drawn in this order from one RandomState(0)"""
    w = (_draw(np.random.RandomState(0), (256, 2048))[name] * 0.02).astype(np.float32)
    w.setflags(write=False)
    return w


@pytest.mark.parametrize("qtype", TYPES)
@pytest.mark.parametrize("name", MATRICES)
def test_weighted_rule_has_less_weighted_error_than_todays_search(name, qtype):
    """A property of the DEFINITION (tests/quant_weighted_ref.py), not of the build: the C++ is tied to it by the byte-for-byte tests
    above.  sum_j qw_j (x_hat - x)^2 over the whole matrix, qw = exp(RandomState(1).randn(K)): the weighted rule is below the unweighted
    search for every distribution and type (single rows may not be: nothing is asserted per row).  DESIGN.md quotes the printed ratios."""
    w = _matrix(name)
    qw = np.exp(np.random.RandomState(1).randn(w.shape[1])).astype(np.float32)
    a = W.weighted_error(W.quantize_blocks_w(w, qtype, qw), qtype, w, qw)
    b = W.weighted_error(R.quantize_blocks(w, qtype), qtype, w, qw)
    print(f"{qtype} {name}: weighted error of the search {b:.6e}, of the weighted rule {a:.6e}, ratio {a / b:.3f}")
    assert a < b
