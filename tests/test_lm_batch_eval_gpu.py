"""rca_lm_batch_eval: rca_lm_eval_async for several sessions over one set of weights in shared passes of the 128-token tiles.

The contract, checked here against a SECOND handle taken from the same start through its own eval_async with the same tokens:
  1. n_tokens, every layer's K / V rows (raw blocks too under a q8_0 cache) and, with want_logits, the logits are equal bit for bit;
  2. one case against the fp32 oracle (LMRef) inside TOL_TILE, the tolerance lm_shape_cases defines for the tile route;
  3. a handle's rows and logits do not depend on its index, its companions, graphs on / off on the workspace, or whether the call is
     the first or the second of its geometry;
  4. rows above a handle's final n_tokens, a bystander twin and the workspace's own cache and n_tokens are untouched;
  5. want_logits = 0 leaves the handles without logits, as rca_lm_reset does;
  6. a step() or an eval() on a participant right behind the call, with no sync, waits for the pass;
  7. every refusal leaves every handle as it was.

Starts come from {0, 1, 31, 32, 255, 256, 257, 300} and n_ctx - count, counts from {1, 7, 8, 9, 31, 32, 33, 127, 128, 129, 200}:
both sides of a flash tile (8 / 16 / 32 tokens), of the 32-row alignment of a segment, of a 128-token block and of the 256-key split.
One more case runs the Q4_K_M file of lm_split_v_case (a layer whose V projection is a GEMM of its own) at contexts under 300 tokens.

Every test here fails on a library without rca_lm_batch_eval (the parent commit: LlamaBatchEval does not exist)."""
import ctypes as C
import dataclasses
import functools

import numpy as np
import pytest
import torch

import lm_shape_cases as sc
import lm_split_v_case as sv

pytestmark = pytest.mark.gpu

G4 = sc.BY_NAME["g4_k768"]
MODELS = {
    "g4_k768": G4,
    "g1_k768": sc.BY_NAME["g1_k768"],
    "g2_k768": dataclasses.replace(G4, name="g2_k768", n_heads=6, n_kv_heads=3, seed=44),     # G = 2, as tests/test_lm_batch_gpu.py builds it
}
for _n in ("g1_gemm128_ffn6144", "g2_gemm128_ffn4096", "g1_h2048_ffn8192", "g2_h2048"):        # the 1280-context cases
    MODELS[_n] = sc.BY_NAME[_n]
CASES = tuple((n, f, kv) for n, f in (("g4_k768", "bf16"), ("g4_k768", "q8_0"), ("g4_k768", "q4_k"), ("g1_k768", "bf16"), ("g2_k768", "bf16"))
              for kv in ("f16", "q8_0"))
CASE_IDS = [f"{n}-{f}-kv_{kv}" for n, f, kv in CASES]
LONG_CASES = tuple((n, "bf16", kv) for n, kv in (("g1_gemm128_ffn6144", "f16"), ("g2_gemm128_ffn4096", "q8_0"), ("g1_h2048_ffn8192", "f16"), ("g2_h2048", "f16")))
GREEDY = dict(top_k=1, top_p=1.0, min_p=0.0, temp=0.0, seed=1)
FAMILY = 30      # 13 handles and their 13 references, a bystander, spares for the refusals


def _ids(name):
    return sv.ids() if name == sv.NAME else MODELS[name].ids().tolist()


@functools.lru_cache(maxsize=None)
def _family(name, fmt, kv, size=FAMILY):
    from realtime_codec_agent_amd.llm import LlamaForAlternatingCodeChannels as L
    if name == sv.NAME:
        return sv.family(6, kv)
    c = MODELS[name]
    parent = L(model_path=f"random:{name}", config=c.config(), n_ctx=c.n_ctx, random_seed=c.seed, init_std=sc.INIT_STD, device=0, weight_format=fmt, kv_format=kv)
    assert parent.weight_format == fmt and parent.prefill_route() == "gemm128" and parent.kv_format == kv
    fam = [parent] + [L(n_ctx=c.n_ctx, share_weights_with=parent, device=0) for _ in range(size - 1)]
    assert all(m.kv_format == kv for m in fam)
    return fam


@functools.lru_cache(maxsize=None)
def _pool(name, fmt, kv):
    from realtime_codec_agent_amd.llm import LlamaBatchEval
    assert LlamaBatchEval.supported(_family(name, fmt, kv)[0])
    return LlamaBatchEval(_family(name, fmt, kv)[0])


def _at(llm, ids, start):
    """the handle at `start` tokens of the id stream, its cache built by eval; every switch at a known value"""
    llm.set_mfma_prefill(True)
    llm.set_graphs(True)
    llm.reset()
    if start:
        llm.eval(ids[:start])
    assert llm.n_tokens == start


def _tokens(ids, k, count):
    """the `count` tokens handle k appends (a different stretch of the stream per handle)"""
    return [ids[(400 + 53 * k + j) % len(ids)] for j in range(count)]


def _state(llm, n_pos=None):
    """everything the contract names: n_tokens and the bits of every layer's K / V rows [0, n_pos) (default: n_tokens)"""
    n = llm.n_tokens if n_pos is None else n_pos
    rows = []
    for layer in range(llm.config.n_layers):
        k, v = llm.kv_read(layer, 0, n)
        rows += [k.view(np.uint16).copy(), v.view(np.uint16).copy()]
        if llm.kv_format == "q8_0":
            rows += [a.copy() if a.dtype == np.int8 else a.view(np.uint16).copy() for a in llm.kv_read_q8(layer, 0, n)]
    return llm.n_tokens, rows


def _same_state(a, b, what):
    assert a[0] == b[0], (what, "n_tokens", a[0], b[0])
    assert len(a[1]) == len(b[1])
    for i, (x, y) in enumerate(zip(a[1], b[1])):
        assert x.shape == y.shape and np.array_equal(x, y), (what, "K / V array", i, int((x != y).sum()), "elements differ")


def _logits(llm):
    s = llm._scores
    assert s.shape[0] == 1
    return s[-1].view(np.uint32).copy()


def _run_and_compare(name, fmt, kv, starts, counts, want_logits=True):
    """handles 0 .. n - 1 through ONE batch eval, references n .. 2 n - 1 through their own eval_async; compares"""
    fam, pool, ids = _family(name, fmt, kv), _pool(name, fmt, kv), _ids(name)
    n = len(starts)
    hs, refs = fam[:n], fam[n:2 * n]
    toks = [_tokens(ids, k, c) for k, c in enumerate(counts)]
    for h, r, s in zip(hs, refs, starts):
        _at(h, ids, s)
        _at(r, ids, s)
    pool.eval_async(hs, toks, want_logits=want_logits)
    for r, t in zip(refs, toks):
        r.eval_async(t)
    for k, (h, r) in enumerate(zip(hs, refs)):
        _same_state(_state(h), _state(r), (name, fmt, kv, "handle", k, "start", starts[k], "count", counts[k]))
        assert h.n_tokens == starts[k] + counts[k]
        assert h._input_ids[:h.n_tokens].tolist() == r._input_ids[:r.n_tokens].tolist()
        if want_logits:
            assert np.array_equal(_logits(h), _logits(r)), (name, fmt, kv, "logits of handle", k)
    return hs, refs


# ---------------------------------------------------------------------------------------------- 1. bit identity
def _shapes(n_ctx):
    return {
        # eight 128-token tiles: exactly one pass
        "8x128": ([0, 1, 31, 32, 255, 256, 257, 300], [128] * 8),
        # padded rows 224 160 128 128 64 32 32 32 32 32 32 | 224 160 = 1280: two passes, handle 11 continued across them (128 + 72)
        "ragged": ([0, 1, 31, 32, 255, 256, 257, 300, n_ctx - 8, n_ctx - 7, n_ctx - 1, 300, n_ctx - 129],
                   [200, 129, 128, 127, 33, 32, 31, 9, 8, 7, 1, 200, 129]),
        "one_handle": ([257], [129]),
        "one_token_in_the_last_slot": ([n_ctx - 1], [1]),
    }


@pytest.mark.parametrize("shape", ["8x128", "ragged", "one_handle", "one_token_in_the_last_slot"])
@pytest.mark.parametrize("name,fmt,kv", CASES, ids=CASE_IDS)
def test_every_handle_ends_with_the_bits_of_its_own_eval_async(name, fmt, kv, shape):
    starts, counts = _shapes(MODELS[name].n_ctx)[shape]
    _run_and_compare(name, fmt, kv, starts, counts)


@pytest.mark.parametrize("kv", ("f16", "q8_0"))
def test_a_file_with_a_v_projection_of_its_own_ends_with_the_bits_of_its_own_eval_async(kv):
    """the Q4_K_M file of lm_split_v_case (layer 1: V as a GEMM of its own, row base in the row-table epilogue); padded rows
    160 + 64 + 32, so two token blocks with pad rows inside and behind the segments, then a second call of the same geometry (replay)"""
    _run_and_compare(sv.NAME, "q4_k", kv, [0, 31, 100], [129, 33, 7])
    _run_and_compare(sv.NAME, "q4_k", kv, [3, 140, 32], [130, 40, 1])


@pytest.mark.parametrize("name,fmt,kv", LONG_CASES, ids=[f"{n}-{f}-kv_{kv}" for n, f, kv in LONG_CASES])
def test_one_handle_with_1100_tokens_takes_two_passes(name, fmt, kv):
    """1024 + 76 rows; the wide models reach the flash instances with 2 and 4 teams per workgroup"""
    _run_and_compare(name, fmt, kv, [31], [1100])


# ---------------------------------------------------------------------------------------------- 2. against the fp32 oracle
def test_logits_after_a_batch_eval_match_the_oracle():
    from oracle import lm_ref
    name, fmt, kv = "g4_k768", "bf16", "f16"
    c, ids = MODELS[name], _ids(name)
    fam, pool = _family(name, fmt, kv), _pool(name, fmt, kv)
    for h in fam[:3]:
        _at(h, ids, 0)
    pool.eval(fam[:3], [ids[:300], ids[100:229], ids[:33]], want_logits=True)      # crosses the 256-key split
    ref = lm_ref.LMRef(c.config(), sc.oracle_weights(c, fmt), kv_dtype=torch.float16)
    for h, seq in ((fam[0], ids[:300]), (fam[2], ids[:33])):
        ref.set_n_tokens(0)
        want = ref.eval(seq, last_only=True, chunk=256)[-1].numpy()
        got = h._scores[-1]
        err = float(np.abs(got - want).max())
        print(f"batch eval against LMRef, {len(seq)} tokens: max |diff| {err:.3e}, bound {sc.bound(want, sc.TOL_TILE):.3e}")
        assert err <= sc.bound(want, sc.TOL_TILE)


# ---------------------------------------------------------------------------------------------- 3. independence
@pytest.mark.parametrize("name,fmt,kv", [CASES[0], CASES[3], CASES[9]], ids=[CASE_IDS[0], CASE_IDS[3], CASE_IDS[9]])
def test_a_handles_result_does_not_depend_on_index_companions_graphs_or_replay(name, fmt, kv):
    fam, pool, ids = _family(name, fmt, kv), _pool(name, fmt, kv), _ids(name)
    h, start, toks = fam[0], 255, _tokens(ids, 0, 129)
    runs = []
    # (index of h, companions' (start, count), graphs on the workspace)
    plans = ((0, [(0, 128), (300, 33)], True), (0, [(0, 128), (300, 33)], True),      # first (eager) and second call of one geometry
             (2, [(31, 7), (1, 200), (256, 1), (32, 128)], True), (0, [], True), (1, [(0, 128), (300, 33)], False))
    for at, comp, graphs in plans:
        others = fam[1:1 + len(comp)]
        for o, (s, _) in zip(others, comp):
            _at(o, ids, s)
        _at(h, ids, start)
        pool.ws.set_graphs(graphs)
        hs = others[:at] + [h] + others[at:]
        lists = [_tokens(ids, 7 + i, cnt) for i, (_, cnt) in enumerate(comp)]
        lists = lists[:at] + [toks] + lists[at:]
        pool.eval_async(hs, lists, want_logits=True)
        runs.append((_state(h), _logits(h)))
    pool.ws.set_graphs(True)
    for i, (st, lg) in enumerate(runs[1:], 1):
        _same_state(st, runs[0][0], ("run", i))
        assert np.array_equal(lg, runs[0][1]), ("logits of run", i)


# ---------------------------------------------------------------------------------------------- 4. nothing else moves
@pytest.mark.parametrize("name,fmt,kv", [CASES[0], CASES[1]], ids=[CASE_IDS[0], CASE_IDS[1]])
def test_rows_above_n_tokens_a_bystander_and_the_workspace_are_untouched(name, fmt, kv):
    fam, pool, ids = _family(name, fmt, kv), _pool(name, fmt, kv), _ids(name)
    c = MODELS[name]
    starts, counts = [0, 31, 300], [33, 128, 9]
    hs, bystander, ws = fam[:3], fam[3], pool.ws
    rng = np.random.default_rng(9)
    for h, s in zip(hs, starts):
        _at(h, ids, s)
    _at(bystander, ids, 40)
    _at(ws, ids, 16)
    sentinels = {}
    for k, h in enumerate(hs + [bystander]):
        top = starts[k] + counts[k] if k < 3 else 40
        n = min(64, c.n_ctx - top)
        for layer in range(c.config().n_layers):
            k_rows = (rng.standard_normal((n, c.n_kv_heads, 64)) * 0.5).astype(np.float16)
            v_rows = (rng.standard_normal((n, c.n_kv_heads, 64)) * 0.5).astype(np.float16)
            h.kv_write(layer, top, k_rows, v_rows)
        sentinels[k] = (top, n, _state(h, top + n)[1])
    by_before, ws_before = _state(bystander), _state(ws, ws._n_ctx)
    pool.eval(hs, [_tokens(ids, k, cnt) for k, cnt in enumerate(counts)], want_logits=True)
    for k, h in enumerate(hs + [bystander]):
        top, n, before = sentinels[k]
        after = _state(h, top + n)[1]
        for a, b in zip(before, after):
            assert np.array_equal(a[top:], b[top:]), ("sentinel rows of handle", k)
    _same_state(_state(bystander), by_before, "bystander")
    _same_state(_state(ws, ws._n_ctx), ws_before, "workspace")
    assert ws.n_tokens == 16 and bystander.n_tokens == 40


# ---------------------------------------------------------------------------------------------- 5. want_logits = 0
def test_without_logits_the_participants_read_as_a_reset_handle_does():
    from realtime_codec_agent_amd import _native as N
    name, fmt, kv = CASES[0]
    fam, pool, ids = _family(name, fmt, kv), _pool(name, fmt, kv), _ids(name)
    hs, refs = _run_and_compare(name, fmt, kv, [0, 300], [128, 9], want_logits=False)
    fresh = fam[5]
    _at(fresh, ids, 12)
    fresh.reset()
    for h in hs:
        h._logits_valid = False
        assert h._scores.shape == fresh._scores.shape == (0, MODELS[name].vocab)
        with pytest.raises(N.RcaError) as e_h:
            h._fetch_logits()
        with pytest.raises(N.RcaError) as e_f:
            fresh._fetch_logits()
        assert str(e_h.value) == str(e_f.value)
    # and a later eval on a participant has logits again
    hs[0].eval(_tokens(ids, 3, 9))
    refs[0].eval(_tokens(ids, 3, 9))
    assert np.array_equal(_logits(hs[0]), _logits(refs[0]))


# ---------------------------------------------------------------------------------------------- 6. ordering
@pytest.mark.parametrize("name,fmt,kv", [CASES[0], CASES[1]], ids=[CASE_IDS[0], CASE_IDS[1]])
def test_a_step_and_an_eval_right_behind_the_call_wait_for_the_pass(name, fmt, kv):
    fam, pool, ids = _family(name, fmt, kv), _pool(name, fmt, kv), _ids(name)
    hs, refs = fam[:3], fam[3:6]
    starts, toks = [255, 31, 0], [_tokens(ids, 0, 128), _tokens(ids, 1, 33), _tokens(ids, 2, 200)]
    for h, r, s in zip(hs, refs, starts):
        _at(h, ids, s)
        _at(r, ids, s)
        h.init_sampler_for_generate(**GREEDY)
        r.init_sampler_for_generate(**GREEDY)
    pool.eval_async(hs, toks, want_logits=True)
    t_h = hs[0].step([ids[7], ids[8]])          # no sync in between
    hs[1].eval(ids[500:520])
    for r, t in zip(refs, toks):
        r.eval_async(t)
        r.sync()
    t_r = refs[0].step([ids[7], ids[8]])
    refs[1].eval(ids[500:520])
    assert t_h == t_r
    for k in range(3):
        _same_state(_state(hs[k]), _state(refs[k]), ("handle", k))
        assert np.array_equal(_logits(hs[k]), _logits(refs[k])), ("logits of handle", k)


# ---------------------------------------------------------------------------------------------- 7. refusals
def test_every_refusal_leaves_every_handle_as_it_was():
    from realtime_codec_agent_amd import _native as N
    from realtime_codec_agent_amd.llm import LlamaForAlternatingCodeChannels as L
    name, fmt, kv = CASES[0]
    c = MODELS[name]
    fam, pool, ids = _family(name, fmt, kv), _pool(name, fmt, kv), _ids(name)
    lib, ws = N.lib(), pool.ws
    a, b = fam[0], fam[1]
    _at(a, ids, 300)
    _at(b, ids, 31)
    before = [_state(a, c.n_ctx), _state(b, c.n_ctx)]

    def call(handles, lists, n_h=None):
        hs = (C.c_void_p * max(len(handles), 1))(*[h if (h is None or isinstance(h, C.c_void_p)) else h._h for h in handles])
        flat = [t for r in lists for t in r]
        arr = (C.c_int32 * max(len(flat), 1))(*flat)
        cnt = (C.c_int32 * max(len(lists), 1))(*[len(r) for r in lists])
        rc = lib.rca_lm_batch_eval(ws._h, hs, len(handles) if n_h is None else n_h, arr, cnt, 1)
        return rc, (lib.rca_last_error() or b"").decode()

    def refused(handles, lists, text, n_h=None):
        rc, msg = call(handles, lists, n_h)
        assert rc != 0 and text in msg, (rc, msg, text)
        for k, h in enumerate((a, b)):
            _same_state(_state(h, c.n_ctx), before[k], ("after the refusal:", text, "handle", k))

    ok = [ids[:9], ids[:9]]
    refused([a, b], ok, "0 handles", n_h=0)
    refused([a] * 65, [ids[:1]] * 65, "65 handles")
    refused([a, None], ok, "handle 1 is null")
    refused([a, b, a], ok + [ids[:9]], "handle 2 is the same handle as handle 0")
    refused([a, ws], ok, "handle 1 is the workspace")
    other = L(model_path=f"random:{name}", config=c.config(), n_ctx=c.n_ctx, random_seed=c.seed, init_std=sc.INIT_STD, device=0, weight_format=fmt)
    refused([a, other], ok, "handle 1 does not share the workspace's weights")
    if torch.cuda.device_count() > 1:      # another device needs a second one: the branch runs where there is one
        far = L(model_path=f"random:{name}", config=c.config(), n_ctx=c.n_ctx, random_seed=c.seed, init_std=sc.INIT_STD, device=1, weight_format=fmt)
        refused([a, far], ok, "handle 1 is on device 1")
        far.close()
    all_rows = L(n_ctx=c.n_ctx, share_weights_with=fam[0], device=0, logits_all=True)
    refused([a, all_rows], ok, "handle 1 is a logits_all handle")
    b.set_mfma_prefill(False)
    refused([a, b], ok, "handle 1 does not take the 128-token tiles")
    b.set_mfma_prefill(True)
    q8 = L(n_ctx=c.n_ctx, share_weights_with=fam[0], device=0, kv_format="q8_0")
    refused([a, q8], ok, "handle 1 has KV format 1, handle 0 has 0")
    refused([a, b], [ids[:9], []], "handle 1 has 0 tokens")
    refused([a, b], [ids[:9], ids[:c.n_ctx - 30]], "context overflow of handle 1")
    refused([a, b], [ids[:9], [3, c.vocab, 5]], f"token id {c.vocab} of handle 1 at index 1")
    refused([a, b], [[-1], ids[:9]], "token id -1 of handle 0 at index 0")
    for h in (other, all_rows, q8):
        h.close()
    # and the same handles are taken once nothing is wrong
    rc, msg = call([a, b], ok)
    assert rc == 0, msg
    assert a.n_tokens == 309 and b.n_tokens == 40
