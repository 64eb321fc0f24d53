"""lm_gemv_kernel run ALONE (rca_lm_gemv_tap: one stage of a decode pass, launched by the call the step makes) with f32 activations
against the float64 reference and the derived bound of tests/gemv_ref.py: five stages x eight device weight forms x four input
classes x M = 1, 2, the instance that ran, other launch geometries bit for bit, the cache rows and buffers next to what a stage
writes, masked head rows, the refusals."""
import ctypes as C
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import gemv_ref as R

pytestmark = pytest.mark.gpu

WORST = {}          # (kind name, format, class) -> worst error / bound
STAGES_M = [s + (M,) for s in R.STAGES for M in (1, 2)]
KIND_ENV = ("QKV", "O", "GU", "DOWN", "HEAD")


@functools.lru_cache(maxsize=2)
def handle(model, fmt, wclass):
    return R.make_handle(model, fmt, wclass)


def process_geometry(kind, ttype):
    """the (R, batches) pair this process's library read from its environment for a stage, None for the default"""
    e = os.environ.get(("RCA_GEMV_" if ttype in ("bf16", "f16") else "RCA_GEMVQ_") + KIND_ENV[kind], "")
    try:
        r, b = (int(v) for v in e.split(","))
    except ValueError:
        return None
    return (r, b) if r in (4, 8, 16) and b >= 1 else None


def expected_form(model, fmt, kind, M, geom=None):
    t, n, k = R.launches(model, fmt, kind)[-1]      # (a layer that keeps V apart: the record is the V launch's)
    NIT, Rr, bpw, grid = R.gemv_instance(kind, t, n, k, M, geom or process_geometry(kind, t))
    return dict(M=M, NIT=NIT, R=Rr, batches=bpw, grid=grid, format=R.FORMAT_ID[t], ACT=0, N=n)


def tap(llm, model, fmt, kind, x, pos0=R.POS0):
    """one call.  The library fills what it reads back with NaN before the launch (kinds 0, 2, 4), so an element the stage skipped fails
    the finiteness check; the head's guard is checked by the library (RCA_ERR_STATE).  The launch must be the restated rules'."""
    llm.n_tokens = pos0
    out = llm.gemv_tap(0, kind, x, want_kv=(kind == 0))
    assert llm.n_tokens == pos0
    assert llm.gemv_tap_form() == expected_form(model, fmt, kind, x.shape[0]), (llm.gemv_tap_form(), expected_form(model, fmt, kind, x.shape[0]))
    out = out if isinstance(out, tuple) else (out,)
    assert np.isfinite(out[0]).all(), "an output element was not written"
    return out


def note(kind, fmt, cls, r):
    key = (R.KINDS[kind], fmt, cls)
    WORST[key] = max(WORST.get(key, 0.0), r)


def check(kind, fmt, cls, got, ref, what):
    """prints the figure before it asserts"""
    r = R.ratio(np.abs(got[0].astype(np.float64) - ref["y"]), ref["bound"])
    note(kind, fmt, cls, r)
    print(f"gemv {what} {fmt} {R.KINDS[kind]} class {cls}: err / bound {r:.3f}")
    assert r <= 1.0, (what, r)
    if kind == 0:
        assert R.f16_interval_ok(got[1], ref["k"], ref["k_bound"]).all(), (what, "K rows")
        assert R.f16_interval_ok(got[2], ref["v"], ref["v_bound"]).all(), (what, "V rows")


# ------------------------------------------------------------------------------------------------------------------ class a
@pytest.mark.parametrize("model,fmt,kind,M", [s for s in STAGES_M if s[2] in (1, 3)])
def test_class_a_exact_integers(model, fmt, kind, M):
    """kinds 1 and 3 (no prologue): integer factors and rows with every magnitude sum below 2^22 (test_gemv_cpu.py): every partial sum in
    any order is an exact integer, so the result must EQUAL the int64 product"""
    llm, L = handle(model, fmt, "int")
    p = R.PROJ_OF_KIND[kind][0]
    W = L["values"][p]
    x = R.act_int([R.magnitude_matrix(L["types"][p], W, R.chunk_form(L["types"][p], L["params"][p]))], W.shape[1], 100 + kind)[:M]
    got = tap(llm, model, fmt, kind, x)
    want = x.astype(np.int64) @ W.astype(np.int64).T
    assert want.any(axis=1).all()
    assert np.array_equal(got[0], want.astype(np.float32)), int((got[0] != want).sum())
    note(kind, fmt, "a", 0.0)


# ------------------------------------------------------------------------------------------------------------------ class b
@pytest.mark.parametrize("model,fmt,kind,M", STAGES_M)
def test_class_b_one_hot_rows_read_every_weight(model, fmt, kind, M):
    """Row m reads column k(m): kinds 1 and 3 must return the f32 weight itself; kinds 0, 2 and 4 the epilogue of w times the one value
    the RMSNorm leaves, within the bound of a single product.  M = 2: every k up to 512, a stratified set with every wave's and every
    `it` step's first and last column beyond; M = 1: those seam columns alone."""
    llm, L = handle(model, fmt, "rand")
    K = R.kind_k(model, kind)
    NIT = max(R.gemv_instance(kind, t, n, k, M)[0] for t, n, k in R.launches(model, fmt, kind))
    cols = R.onehot_columns(K, NIT) if M == 2 else np.array(sorted(R.seam_columns(K, NIT)))
    W = np.concatenate([L["values"][p] for p in R.PROJ_OF_KIND[kind]]) if kind in (1, 3) else None
    st = R.stage(model, fmt, kind, "rand") if W is None else None
    worst = 0.0
    for i in range(0, len(cols), M):
        x = R.act_onehot(K, cols[i:i + M])
        got = tap(llm, model, fmt, kind, x)
        if W is not None:
            assert np.array_equal(got[0], W[:, cols[i:i + M]].T), cols[i:i + M]
            continue
        ref = st(x)
        r = R.ratio(np.abs(got[0].astype(np.float64) - ref["y"]), ref["bound"])
        worst = max(worst, r)
        assert r <= 1.0, (cols[i:i + M], r)
        if kind == 0:
            assert R.f16_interval_ok(got[1], ref["k"], ref["k_bound"]).all() and R.f16_interval_ok(got[2], ref["v"], ref["v_bound"]).all(), cols[i:i + M]
    note(kind, fmt, "b", worst)
    print(f"gemv {model} M {M} {fmt} {R.KINDS[kind]} class b, {len(cols)} columns: err / bound {worst:.3f}")


# ------------------------------------------------------------------------------------------------------------------ classes c, d
@pytest.mark.parametrize("model,fmt,kind,M", STAGES_M)
def test_class_c_normal_data_within_the_bound(model, fmt, kind, M):
    """random blocks (sigma near 0.05), rows of sigma 1; under a prologue the second row has sigma 2^-6, where eps weighs 4 %"""
    llm, L = handle(model, fmt, "rand")
    x = R.act_normal(R.kind_k(model, kind), kind, 200 + kind)[:M]
    check(kind, fmt, "c", tap(llm, model, fmt, kind, x), R.stage(model, fmt, kind, "rand")(x), f"{model} M {M}")


@pytest.mark.parametrize("model,fmt,kind,M", STAGES_M)
def test_class_d_coherent_data_within_the_bound(model, fmt, kind, M):
    """all weights and activations positive: the accumulation is worst-case, and every output of kinds 1 and 3 (whose residual the
    tap zeroes instead of filling it with NaN) is non-zero, so an element the kernel skipped shows"""
    llm, L = handle(model, fmt, "coherent")
    x = R.act_coherent(R.kind_k(model, kind), kind, 300 + kind)[:M]
    got = tap(llm, model, fmt, kind, x)
    if kind in (1, 3):
        assert (got[0] > 0).all(), "an output element was not written"
    check(kind, fmt, "d", got, R.stage(model, fmt, kind, "coherent")(x), f"{model} M {M}")


# ------------------------------------------------------------------------------------------------------------------ geometry
def test_other_launch_geometries_give_the_same_bits(tmp_path):
    """Two fresh child processes load the library under RCA_GEMV_* / RCA_GEMVQ_* = "4,1" and "8,4" for all five stages and tap a fixed list of
    stages on class c rows: their instances are the restated rules' for that pair, their bits are this process's.
    (First MI355X run: "8,4" differed in 384 of 1536 gate/up outputs of the q8_0 model S -- q8_0 at R = 8 with a second batch in the
    workgroup read the next batch's scales for its second half; fixed in issue_scales, DESIGN.md "Decode GEMVs alone".)"""
    mine, my_forms = R.geometry_outputs()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for name, geom in R.GEOMETRIES.items():
        out = str(tmp_path / f"geom_{geom[0]}_{geom[1]}.npz")
        env = dict(os.environ, PYTHONPATH=os.pathsep.join([root, os.path.join(root, "tests")] + [p for p in [os.environ.get("PYTHONPATH")] if p]))
        env.update({v: name for v in R.GEOMETRY_ENV})
        cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [os.path.join(root, "tests", "gemv_ref.py"), out]
        r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, (name, r.returncode, r.stdout[-1500:], r.stderr[-1500:])
        with np.load(out) as z:
            forms = json.loads(str(z["forms"]))
            differ = 0
            for model, fmt, kind in R.GEOMETRY_STAGES:
                stage = f"{model}.{fmt}.{kind}"
                assert forms[stage] == expected_form(model, fmt, kind, 2, geom), (name, stage, forms[stage])
                differ += forms[stage] != my_forms[stage]
                for key in [k for k in mine if k.startswith(stage + ".")]:
                    assert np.array_equal(z[key], mine[key]), (name, key, int((z[key] != mine[key]).sum()))
            assert differ == sum(expected_form(m, f, k, 2, geom) != expected_form(m, f, k, 2) for m, f, k in R.GEOMETRY_STAGES) and differ >= 10, (name, differ)
        print(f"geometry {name}: {len(mine)} arrays of {len(R.GEOMETRY_STAGES)} stages identical, {differ} stages on another instance or grid")


# ------------------------------------------------------------------------------------------------------------------ writes stay inside
@pytest.mark.parametrize("model,fmt", [("S", "q4_k"), ("S", "q6_k"), ("P", "bf16")])
def test_kind_0_positions_and_the_cache_rows_next_to_them(model, fmt):
    """n_ctx = 700, positions 0, 350 and n_ctx - M: the RoPE rows of the table's ends, K / V rows where the tap says, and the planted rows
    on either side of the written positions come back unchanged"""
    llm, L = R.make_handle(model, fmt, "rand", n_ctx=700)
    try:
        nkv = L["config"].n_kv_heads
        st = R.Stage(model, fmt, 0, L)
        left, right = np.full((1, nkv, 64), 123.25, np.float16), np.full((1, nkv, 64), -77.5, np.float16)
        for M in (1, 2):
            x = R.act_normal(R.kind_k(model, 0), 0, 700)[:M]
            for pos0 in (0, 350, 700 - M):
                if pos0 > 0:
                    llm.kv_write(0, pos0 - 1, left, left)
                if pos0 + M < 700:
                    llm.kv_write(0, pos0 + M, right, right)
                got = tap(llm, model, fmt, 0, x, pos0)
                check(0, fmt, "c", got, st(x, pos0), f"{model} M {M} pos0 {pos0}")
                k, v = llm.kv_read(0, pos0, M)
                assert np.array_equal(k.reshape(M, -1).view(np.uint16), got[1].view(np.uint16)) and np.array_equal(v.reshape(M, -1).view(np.uint16), got[2].view(np.uint16))
                for p, want in ((pos0 - 1, left), (pos0 + M, right)):
                    if 0 <= p < 700:
                        k, v = llm.kv_read(0, p, 1)
                        assert np.array_equal(k, want) and np.array_equal(v, want), (M, pos0, p)
    finally:
        llm.close()


@pytest.mark.parametrize("fmt", R.FORMATS)
def test_the_heads_guard_is_intact_at_every_ragged_vocabulary(fmt):
    """vocabularies 1001 / 1002 / 1004 (the last batch of 16 holds 9, 10 or 12 rows) and 8204 (the last workgroup holds one batch): the
    library checks the 64 floats behind row M - 1 of the head's output after the launch and refuses when they changed"""
    for model in ("S", "T", "D8"):
        llm, L = handle(model, fmt, "rand")
        for M in (1, 2):
            got = tap(llm, model, fmt, 4, R.act_normal(R.kind_k(model, 4), 4, 500)[:M])
            assert got[0].shape == (M, R.vocab_of(model, fmt))


@pytest.mark.parametrize("fmt", R.FORMATS)
def test_masked_head_rows(fmt):
    """rca_lm_mask_head_rows: the masked rows give logit 0 exactly, every other row keeps its bits, in every form; the ranges start and
    end inside a pair, a quad and a batch, and one reaches the ragged end"""
    llm, L = R.make_handle("S", fmt, "rand")
    try:
        V = L["config"].vocab_size
        x = R.act_normal(256, 4, 600)
        before = tap(llm, "S", fmt, 4, x)[0]
        assert (before != 0).all()
        masked = np.zeros(V, bool)
        for a, b in ((5, 23), (V - 3, V)):
            llm.mask_head_rows(a, b)
            masked[a:b] = True
            after = tap(llm, "S", fmt, 4, x)[0]
            assert (after[:, masked] == 0).all(), (a, b)
            assert np.array_equal(after[:, ~masked].view(np.uint32), before[:, ~masked].view(np.uint32)), (a, b)
    finally:
        llm.close()


# ------------------------------------------------------------------------------------------------------------------ refusals
def test_refusals_leave_the_handle_alone():
    from realtime_codec_agent_amd import _native as N
    llm, L = R.make_handle("S", "bf16", "rand")
    try:
        V = L["config"].vocab_size
        row = np.random.default_rng(1).standard_normal(V).astype(np.float32)
        llm.eval([3])                   # a logits row exists from here on; the test replaces it with a known one
        llm._put_logits(row)
        llm.n_tokens = 12
        x = R.act_normal(256, 0, 800)
        y = np.zeros((3, V), np.float32)

        def call(layer=0, kind=0, M=2, numel=None):
            width = {0: 256, 1: 256, 2: 768, 3: 256, 4: V}.get(kind, 256)
            rc = llm._lib.rca_lm_gemv_tap(llm._h, layer, kind, x.ctypes.data_as(C.POINTER(C.c_float)), M, y.ctypes.data_as(C.POINTER(C.c_float)),
                                          C.c_int64(M * width if numel is None else numel), None)
            N.check(rc, "rca_lm_gemv_tap")

        def untouched(n):
            assert llm.n_tokens == n
            llm._logits_valid = False
            assert np.array_equal(llm._fetch_logits().view(np.uint32), row.view(np.uint32))

        for what, kw in ((r"gemv_tap: M = 3, a decode pass has 1 or 2 tokens", dict(M=3)), (r"gemv_tap: M = 0,", dict(M=0)),
                         (r"gemv_tap: kind 5 outside \[0, 4\]", dict(kind=5)), (r"gemv_tap: kind -1 outside", dict(kind=-1)),
                         (r"gemv_tap: layer 1 outside \[0, 1\)", dict(layer=1)), (r"gemv_tap: layer -1 outside", dict(layer=-1)),
                         (r"gemv_tap: y_numel 7, kind 0 writes 2 x 256 values", dict(numel=7))):
            with pytest.raises(N.RcaError, match=what):
                call(**kw)
            untouched(12)
        llm.n_tokens = R.N_CTX - 1
        with pytest.raises(N.RcaError, match=rf"rc=-3\): gemv_tap: positions {R.N_CTX - 1} \.\. {R.N_CTX} are outside the context of {R.N_CTX}"):
            call()
        untouched(R.N_CTX - 1)
        call(M=1)                       # the last position itself is taken
        untouched(R.N_CTX - 1)
    finally:
        llm.close()


# ------------------------------------------------------------------------------------------------------------------ report
def test_report_of_worst_ratios():
    """what the tests above measured (run with them): the worst error / bound ratio per kind, format and class"""
    for kind in R.KINDS.values():
        for cls in "abcd":
            row = ", ".join(f"{fmt} {WORST[kind, fmt, cls]:.3f}" for fmt in R.FORMATS if (kind, fmt, cls) in WORST)
            if row:
                print(f"GEMV worst error / bound, {kind} class {cls}: {row}")
    assert all(v <= 1.0 for v in WORST.values())
