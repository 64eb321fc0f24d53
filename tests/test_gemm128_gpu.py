"""lm_gemm128_kernel<EPI, WF> and lm_gemm128_epilogue_kernel<EPI> run ALONE (rca_lm_gemm128_tap: one projection of a 128-token-tile
pass, through the launchers the passes use) against the float64 reference and the derived bound of tests/gemm128_ref.py: five kinds x
eight device weight forms x four input classes, every k-slice form, the token-block, row-mask and vocabulary seams, the refusals."""
import functools
import os

import numpy as np
import pytest

import gemm128_ref as G

pytestmark = pytest.mark.gpu

WORST = {}          # (kind name, format, class) -> worst error / bound
POS0 = 5            # class cases of kind 0 sit at positions 5 ..
PROCESS_SEQ_MIN = int(os.environ.get("RCA_LM_SEQ_MIN_WGS", "512"))


@functools.lru_cache(maxsize=None)
def handle(model, fmt, wclass, vocab=G.VOCABS[0]):
    from realtime_codec_agent_amd.llm import LlamaForAlternatingCodeChannels
    weights, values = G.layer(model, fmt, wclass, vocab)
    llm = LlamaForAlternatingCodeChannels(config=G.config(model, vocab), weights=weights, n_ctx=G.N_CTX, device=0)
    assert llm.prefill_route() == "gemm128"
    return llm, values, weights["rope.inv_freq"]


def tap(llm, kind, xh, xl, pos0=0, **kw):
    """one call; rows >= M of what comes back must still be the NaN they were filled with"""
    llm.n_tokens = pos0
    M = xh.shape[0]
    cap = 128 if kind == 4 else G.LM_MAXM
    kw.setdefault("out_rows", min(cap, M + 3))
    out = llm.gemm128_tap(0, kind, xh, xl, **kw)
    assert llm.n_tokens == pos0
    assert np.isnan(out[0][M:]).all(), "rows behind M were written"
    if kind == 4:
        assert np.isnan(out[2]).all(), "the head wrote behind its block"
    return (out[0][:M],) + tuple(out[1:])


def note(kind, fmt, cls, r):
    key = (G.KINDS[kind], fmt, cls)
    WORST[key] = max(WORST.get(key, 0.0), r)


def check(kind, fmt, cls, got, ref, model, what):
    """got = the tap's return (rows < M); ref = gemm128_ref.reference / epilogue.  Prints each figure before it asserts."""
    y = got[0]
    assert np.isfinite(y).all(), what
    r = G.ratio(np.abs(y.astype(np.float64) - ref["y"]), ref["bound"])
    note(kind, fmt, cls, r)
    print(f"gemm128 {model} {fmt} {G.KINDS[kind]} class {cls} {what}: err / bound {r:.3f}")
    assert r <= 1.0, (what, r)
    if kind == 0:
        k, v = got[2], got[3]
        assert G.f16_interval_ok(k, ref["k"], ref["k_bound"]).all(), (what, "K rows")
        assert G.f16_interval_ok(v, ref["v"], ref["v_bound"]).all(), (what, "V rows")


def geometry(kind, M):
    return {} if kind == 4 else dict(rows=M, want_kv=(kind == 0))


MODEL_FORMATS = [("A", f) for f in G.FORMATS] + [(m, f) for m in ("B", "C") for f in ("bf16", "q4_k")]
HEAD_VOCABS = {fmt: G.VOCABS + ((G.VOCAB_BF16_EXTRA,) if fmt == "bf16" else ()) for fmt in G.FORMATS}


def cases(kind, model, fmt):
    """the handles a kind runs on: the head once per vocabulary"""
    return [G.VOCABS[0]] if kind != 4 else list(HEAD_VOCABS[fmt]) if model == "A" else [G.VOCABS[0]]


# ------------------------------------------------------------------------------------------------------------------ class a
@pytest.mark.parametrize("kind", sorted(G.KINDS))
@pytest.mark.parametrize("model,fmt", MODEL_FORMATS)
def test_class_a_exact_integers(model, fmt, kind):
    """Integer weights and activations with w_lo x_lo = 0 and sum |w| |x| <= 2^22 (test_gemm128_cpu.py): every partial sum in any order is
    an exact integer, so kinds 1, 3, 4 must EQUAL the int64 dot product and kinds 0, 2 are held to the float64 epilogue of that sum."""
    for vocab in cases(kind, model, fmt):
        llm, values, inv = handle(model, fmt, "int", vocab)
        W = G.fused(values, kind)
        M = 128 if kind == 4 else 129
        xh, xl = G.act_int(W, M, 100 + kind)
        got = tap(llm, kind, xh, xl, POS0, **geometry(kind, M))
        x = (G.widen(xh).astype(np.int64) + G.widen(xl).astype(np.int64))
        want = x @ W.astype(np.int64).T
        if kind in (1, 3, 4):
            assert np.array_equal(got[0], want.astype(np.float32)), (vocab, int((got[0] != want).sum()))
            note(kind, fmt, "a", 0.0)
        else:
            ref = G.epilogue(kind, want.astype(np.float64), np.zeros(want.shape), model, POS0, inv)
            check(kind, fmt, "a", got, ref, model, f"V {vocab}")


# ------------------------------------------------------------------------------------------------------------------ class b
@pytest.mark.parametrize("kind", sorted(G.KINDS))
@pytest.mark.parametrize("model,fmt", MODEL_FORMATS)
def test_class_b_one_hot_columns_read_every_weight(model, fmt, kind):
    """Token t reads column k(t): y[t][n] must equal w_hi + w_lo of W[n][k(t)] (W itself for bf16) -- every element of every format on
    this path, realistic blocks quantised from normal data.  Kinds 0 and 2: the float64 epilogue of exactly that value."""
    for vocab in cases(kind, model, fmt):
        llm, values, inv = handle(model, fmt, "normal", vocab)
        W = G.fused(values, kind)
        K = W.shape[1]
        types = G.matrix_types(fmt, vocab)
        if types[{0: "q", 1: "o", 2: "gate", 3: "down", 4: "head"}[kind]] == "bf16":
            exact = W.astype(np.float64)
        else:
            hi, lo = G.split(W)
            exact = hi.astype(np.float64) + lo.astype(np.float64)
            assert (np.abs(exact - W) <= 2.0 ** -17 * np.abs(W)).all()
        step = 128 if kind == 4 else min(K, G.LM_MAXM)
        for k0 in range(0, K, step):
            xh, xl = G.act_onehot(K, k0, step)
            got = tap(llm, kind, xh, xl, 0, **geometry(kind, step))
            want = exact[:, k0:k0 + step].T
            if kind in (1, 3, 4):
                assert np.array_equal(got[0], want.astype(np.float32)), (vocab, k0)
                note(kind, fmt, "b", 0.0)
            else:
                check(kind, fmt, "b", got, G.epilogue(kind, want, np.zeros(want.shape), model, 0, inv), model, f"V {vocab} k0 {k0}")


# ------------------------------------------------------------------------------------------------------------------ classes c, d
ROWS_C = (1, 31, 128, 129, 257)


@pytest.mark.parametrize("kind", sorted(G.KINDS))
@pytest.mark.parametrize("model,fmt", MODEL_FORMATS)
def test_class_c_normal_data_within_the_bound(model, fmt, kind):
    """weights sigma 0.05, activations sigma 1 split as a pass splits them, M = 1, 31, 128, 129, 257 rows (the head: one block, M <= 128):
    one reference over the longest input, every call takes its first M rows"""
    for vocab in cases(kind, model, fmt):
        llm, values, inv = handle(model, fmt, "normal", vocab)
        Ms = [m for m in ROWS_C if kind != 4 or m <= 128]
        xh, xl = G.act_normal(G.kind_nk(model, kind, vocab)[1], max(Ms), 200 + kind)
        ref = G.reference(model, fmt, kind, values, xh, xl, POS0, inv, vocab)
        for M in Ms:
            check(kind, fmt, "c", tap(llm, kind, xh[:M], xl[:M], POS0, **geometry(kind, M)), {k: v[:M] for k, v in ref.items()}, model, f"V {vocab} M {M}")


@pytest.mark.parametrize("kind", sorted(G.KINDS))
@pytest.mark.parametrize("model,fmt", MODEL_FORMATS)
def test_class_d_coherent_data_within_the_bound(model, fmt, kind):
    """all weights and activations positive, every w_lo and every x_lo of one sign: a dropped hi x lo product adds up over K (it exceeds
    the bound 8 times and more: test_gemm128_cpu.py)"""
    for vocab in cases(kind, model, fmt):
        llm, values, inv = handle(model, fmt, "coherent", vocab)
        M = 31
        xh, xl = G.act_coherent(G.kind_nk(model, kind, vocab)[1], M, 300 + kind)
        ref = G.reference(model, fmt, kind, values, xh, xl, POS0, inv, vocab)
        check(kind, fmt, "d", tap(llm, kind, xh, xl, POS0, **geometry(kind, M)), ref, model, f"V {vocab}")


# ------------------------------------------------------------------------------------------------------------------ forms
def _split_projections():
    out = []
    for model in ("A", "C"):
        for kind in (0, 1, 2, 3):
            ns = G.g128_splits(*G.kind_nk(model, kind))
            if ns > 1:
                out.append((model, kind, ns))
    return out


@pytest.mark.parametrize("fmt", ["bf16", "q4_k"])
@pytest.mark.parametrize("model,kind,ns", _split_projections())
def test_every_form_gives_the_same_bits(model, kind, ns, fmt):
    """rows = 128 and 1024 with seq_min 0, 1 and the process value: the reported form is the one named, and every form -- and the same
    rows inside a 1024-row and inside a 128-row launch -- gives the same bits, K and V rows included"""
    llm, values, inv = handle(model, fmt, "normal")
    N, K = G.kind_nk(model, kind)
    xh, xl = G.act_normal(K, 1024, 400 + kind)
    named = {0: "every slice stored" + (", grouped epilogue" if ns >= 8 else ""), 1: "walking" if ns <= 4 else "group sums stored"}
    outs = {}
    for rows in (128, 1024):
        for seq_min in (0, 1, -1):
            got = tap(llm, kind, xh[:rows], xl[:rows], POS0, rows=rows, seq_min=seq_min, want_kv=(kind == 0), out_rows=rows)
            want_form = G.g128_form(N, ns, rows // 128, PROCESS_SEQ_MIN if seq_min < 0 else seq_min)
            assert got[1] == want_form, (rows, seq_min, got[1], want_form)
            if seq_min >= 0:
                assert G.form_name(got[1]) == named[seq_min], (rows, seq_min, got[1])
            assert np.isfinite(got[0]).all()
            outs[rows, seq_min] = [got[0]] + [a.view(np.uint16) for a in got[2:]]
    assert len({G.form_name(G.g128_form(N, ns, r // 128, s)) for r in (128, 1024) for s in (0, 1)}) == 2
    first = outs[1024, 0]
    for (rows, seq_min), o in outs.items():
        for a, b in zip(o, first):
            assert np.array_equal(a, b[:rows]), (rows, seq_min)


# ------------------------------------------------------------------------------------------------------------------ seams
@pytest.mark.parametrize("fmt", ["bf16", "q4_k"])
@pytest.mark.parametrize("kind", [0, 1, 2, 3])
def test_rows_behind_m_are_masked_in_every_token_block(kind, fmt):
    """M = 1, 127, 128, 129 of rows = 1024 with NaN planes behind M: rows < M equal the M = 1024 call's bit for bit, rows >= M stay NaN"""
    llm, values, inv = handle("A", fmt, "normal")
    xh, xl = G.act_normal(G.kind_nk("A", kind)[1], 1024, 500 + kind)
    full = tap(llm, kind, xh, xl, POS0, rows=1024, want_kv=(kind == 0), out_rows=1024)
    assert np.isfinite(full[0]).all()
    for M in (1, 127, 128, 129):
        got = tap(llm, kind, xh[:M], xl[:M], POS0, rows=1024, want_kv=(kind == 0), out_rows=1024)
        assert np.array_equal(got[0], full[0][:M]), M
        for a, b in zip(got[2:], full[2:]):
            assert np.array_equal(a.view(np.uint16), b[:M].view(np.uint16)), M


@pytest.mark.parametrize("fmt", G.FORMATS)
def test_head_row_mask_and_vocabulary_tail(fmt):
    """kind 4 at row_base 0 and 128 with M = 1, 5, 128 (the state's m is row_base + M): class a, so the tail columns of the ragged last
    row tile are exact; rows >= M and the row tile behind the block stay NaN"""
    for vocab in HEAD_VOCABS[fmt]:
        llm, values, inv = handle("A", fmt, "int", vocab)
        W = values["head"]
        assert vocab % 128 == (2 if vocab == 130 else 4)
        xh, xl = G.act_int(W, 128, 600)
        want = ((G.widen(xh).astype(np.int64) + G.widen(xl).astype(np.int64)) @ W.astype(np.int64).T).astype(np.float32)
        for row_base in (0, 128):
            for M in (1, 5, 128):
                got = tap(llm, 4, xh[:M], xl[:M], 0, row_base=row_base, out_rows=128)
                assert np.array_equal(got[0], want[:M]), (vocab, row_base, M)


def test_kind_0_at_the_first_and_the_last_positions():
    """n_tokens 0 and n_ctx - M: the RoPE rows of the table's two ends, the last cache rows"""
    llm, values, inv = handle("A", "q4_k", "normal")
    M = 129
    xh, xl = G.act_normal(G.kind_nk("A", 0)[1], M, 700)
    for pos0 in (0, G.N_CTX - M):
        ref = G.reference("A", "q4_k", 0, values, xh, xl, pos0, inv)
        check(0, "q4_k", "c", tap(llm, 0, xh, xl, pos0, rows=M, want_kv=True), ref, "A", f"pos0 {pos0}")
        k, v = llm.kv_read(0, pos0, M)
        assert G.f16_interval_ok(k.reshape(M, -1), ref["k"], ref["k_bound"]).all()


def test_split_v_layer_gives_the_rows_of_the_matrices_kept_as_one():
    """the same integer values twice: V as Q6_K next to Q4_K q / k (two segments, two launches) and all three as Q4_K (one matrix)"""
    from realtime_codec_agent_amd import _native as N
    from realtime_codec_agent_amd.llm import LlamaForAlternatingCodeChannels
    from oracle import q4k_ref
    weights, values = G.layer("A", "q4_k", "int")
    n, k = values["v"].shape
    rng = np.random.default_rng(9)
    q = rng.integers(0, 16, (n, k)).astype(np.uint8)      # 0 .. 15: a Q4_K value with sc = 1, m = 0 and a Q6_K value with scale 1
    one = np.ones((n, k // 256))
    as4 = q4k_ref.pack_blocks(dict(q=q, sc=np.ones((n, k // 32), np.uint8), m=np.zeros((n, k // 32), np.uint8), d=one.astype(np.float16), dmin=one.astype(np.float16)))
    as6 = q4k_ref.pack_blocks_q6_k(dict(q=q.astype(np.int8), sc=np.ones((n, k // 16), np.int8), d=one.astype(np.float16)))
    name = G.HF["v"]
    llms = [LlamaForAlternatingCodeChannels(config=G.config("A", G.VOCABS[0]), weights=dict(weights, **{name: t}), n_ctx=G.N_CTX, device=0)
            for t in (N.Q4KBlocks(as4, (n, k)), N.Q6KBlocks(as6, (n, k)))]
    W = np.concatenate([values["q"], values["k"], q.astype(np.float32)])
    xh, xl = G.act_int(W, 129, 800)
    outs = [tap(llm, 0, xh, xl, POS0, rows=129, want_kv=True) for llm in llms]
    for a, b in zip(outs[0][:1] + outs[0][2:], outs[1][:1] + outs[1][2:]):
        assert np.array_equal(a.view(np.uint16 if a.dtype == np.float16 else np.uint32), b.view(np.uint16 if b.dtype == np.float16 else np.uint32))
    want = (G.widen(xh).astype(np.int64) + G.widen(xl).astype(np.int64)) @ q.astype(np.int64).T
    with np.errstate(over="ignore"):      # (sums past 65504 are Inf in the cache and here)
        want16 = want.astype(np.float16)
    assert np.array_equal(outs[1][3].astype(np.float64), want16.astype(np.float64)), "V rows: fp16 of the exact sums"
    for llm in llms:
        llm.close()


# ------------------------------------------------------------------------------------------------------------------ refusals
def test_refusals_leave_the_handle_alone():
    from realtime_codec_agent_amd._native import RcaError
    llm, values, inv = handle("A", "bf16", "normal")
    H = 512
    xh, xl = G.act_normal(H, 4, 900)
    llm.n_tokens = 12
    k0, v0 = llm.kv_read(0, 0, 64)
    big = np.zeros((1025, H), np.uint16)
    call = lambda **kw: llm.gemm128_tap(**{**dict(layer=0, kind=0, xh=xh, xl=xl), **kw})   # noqa: E731
    for what, c in (
        (r"gemm128_tap: kind 5 outside", lambda: call(kind=5, xh=np.zeros((4, 512), np.uint16), xl=np.zeros((4, 512), np.uint16))),
        (r"gemm128_tap: kind -1 outside", lambda: call(kind=-1, xh=np.zeros((4, 512), np.uint16), xl=np.zeros((4, 512), np.uint16))),
        (r"gemm128_tap: layer 1 outside", lambda: call(layer=1)),
        (r"gemm128_tap: layer -1 outside", lambda: call(layer=-1)),
        (r"gemm128_tap: M = 0, kind 0 takes 1 \.\. 1024", lambda: call(M=0)),
        (r"gemm128_tap: M = 1025, kind 0 takes 1 \.\. 1024", lambda: call(xh=big, xl=big)),
        (r"gemm128_tap: M = 129, kind 4 takes 1 \.\. 128", lambda: call(kind=4, xh=big[:129], xl=big[:129])),
        (r"gemm128_tap: rows 3 outside \[M = 4, 1024\]", lambda: call(rows=3)),
        (r"gemm128_tap: rows 1025 outside", lambda: call(rows=1025)),
        (r"gemm128_tap: out_rows 3 outside", lambda: call(out_rows=3)),
        (r"gemm128_tap: out_rows 1025 outside", lambda: call(out_rows=1025)),
        (r"gemm128_tap: row_base 64 ", lambda: call(kind=4, row_base=64)),
        (r"gemm128_tap: row_base 1024 ", lambda: call(kind=4, row_base=1024)),
        (r"gemm128_tap: row_base 128 ", lambda: call(kind=1, row_base=128)),
    ):
        with pytest.raises(RcaError, match=what):
            c()
        assert llm.n_tokens == 12, what
    llm.n_tokens = G.N_CTX - 3
    with pytest.raises(RcaError, match=rf"gemm128_tap: positions {G.N_CTX - 3} \.\. {G.N_CTX} are outside the context of {G.N_CTX}"):
        call()
    assert llm.n_tokens == G.N_CTX - 3
    llm.n_tokens = 12
    llm.set_mfma_prefill(False)       # a handle off the tile route
    try:
        assert llm.prefill_route() == "gemv"
        with pytest.raises(RcaError, match=r"rc=-1\): gemm128_tap: the handle does not take the 128-token tiles \(rca_lm_prefill_route 0"):
            call()
    finally:
        llm.set_mfma_prefill(True)
    assert llm.n_tokens == 12
    k1, v1 = llm.kv_read(0, 0, 64)
    assert np.array_equal(k0.view(np.uint16), k1.view(np.uint16)) and np.array_equal(v0.view(np.uint16), v1.view(np.uint16))


# ------------------------------------------------------------------------------------------------------------------ report
def test_report_of_worst_ratios():
    """what the tests above measured (run with them): the worst error / bound ratio per kind, format and class"""
    for kind in G.KINDS.values():
        for cls in "abcd":
            row = ", ".join(f"{fmt} {WORST[kind, fmt, cls]:.3f}" for fmt in G.FORMATS if (kind, fmt, cls) in WORST)
            if row:
                print(f"GEMM128 worst error / bound, {kind} class {cls}: {row}")
    assert all(v <= 1.0 for v in WORST.values())
