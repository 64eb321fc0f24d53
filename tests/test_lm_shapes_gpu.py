"""The LM at every shape class and kernel route the ABI accepts (tests/lm_shape_cases.py): per case and weight format, decode and
prefill against the fp32 oracle over the same (de-quantised) values, the prefill route the library reports against the one the
table claims, and the two bit-exactness contracts the agent relies on (prefill == incremental on the exact route; any cut of a
prompt into pieces of more than 8 tokens gives the same bits on the tile routes).

Tolerances are test_lm_gpu.py's, normalised the same way (tol * max(1, max|want|)): 1e-3 for a decode pass on a cache the exact GEMV
passes built, 2e-3 whenever a tile route built the cache.  Every comparison prints max|dlogit| and its ratio to the bound."""
import functools

import numpy as np
import pytest
import torch

import lm_shape_cases as sc
from oracle import lm_ref

pytestmark = pytest.mark.gpu

SAMPLER = dict(top_k=50, top_p=1.0, min_p=0.0, temp=1.0, seed=3)
CF = pytest.mark.parametrize("name,fmt", sc.CASE_FORMATS, ids=[f"{n}-{f}" for n, f in sc.CASE_FORMATS])


@functools.lru_cache(maxsize=None)
def _llm(name, fmt):
    from realtime_codec_agent_amd.llm import LlamaForAlternatingCodeChannels
    c = sc.BY_NAME[name]
    llm = LlamaForAlternatingCodeChannels(model_path=f"random:{name}", config=c.config(), n_ctx=c.n_ctx, random_seed=c.seed,
                                          init_std=sc.INIT_STD, device=0, weight_format=fmt)
    assert llm.weight_format == fmt
    return llm


@functools.lru_cache(maxsize=None)
def _weights(name, fmt):
    return sc.oracle_weights(sc.BY_NAME[name], fmt)


def _ref(name, fmt):
    return lm_ref.LMRef(sc.BY_NAME[name].config(), _weights(name, fmt), kv_dtype=torch.float16)


def _fresh(name, fmt, mfma):
    """the case's handle with every switch at a known value"""
    llm = _llm(name, fmt)
    llm.set_mfma_prefill(mfma)
    llm.set_graphs(True)
    llm.set_attn_fuse(True)
    llm.reset()
    return llm


def _compare(tag, got, want, tol):
    d, b = float(np.abs(got - want).max()), sc.bound(want, tol)
    print(f"SHAPES {tag}: max|dlogit| = {d:.3e}, bound {b:.3e} (tol {tol:g}, max|logit| {np.abs(want).max():.2f}), ratio {d / b:.3f}")
    assert d <= b, (tag, d, b)
    assert got.argmax() == want.argmax(), tag


def _n_cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


@CF
def test_decode_matches_oracle_and_step_graphs_equal_eval(name, fmt):
    """Exact route.  A 298-token eval (2-token GEMV passes across the 256-key split) and a 2-token eval against the oracle; then, with
    the cache filled to 516 keys, 1- and 2-token steps that end just below, at and just above 256 and 512 keys: rca_lm_step with
    graphs on / off times the in-launch merge on / off gives the same token and the logits of the plain eval, bit for bit."""
    c = sc.BY_NAME[name]
    ids = c.ids().tolist()
    llm, ref = _fresh(name, fmt, False), _ref(name, fmt)
    P = c.prompt
    llm.eval(ids[:P - 2])
    ref.eval(ids[:P - 2], last_only=True)
    llm.eval(ids[P - 2:P])
    got = llm._scores[-1].copy()
    _compare(f"{name}/{fmt} decode at {P} keys (exact route)", got, ref.eval(ids[P - 2:P])[-1].numpy(), sc.TOL_EXACT)
    llm.eval(ids[P:516])
    for start in (253, 254, 255, 256, 509, 510, 511, 512):
        for n in (2, 1):
            cur = ids[start:start + n]
            llm.n_tokens = start
            llm.eval(cur)
            want = llm._scores[-1].copy()
            toks = []
            for graphs in (True, False):
                for fuse in (True, False):
                    llm.set_graphs(graphs)
                    llm.set_attn_fuse(fuse)
                    llm.n_tokens = start
                    llm.init_sampler_for_generate(**SAMPLER)
                    toks.append(llm.step(cur))
                    assert llm.n_tokens == start + n
                    assert np.array_equal(llm._scores[-1], want), (name, fmt, start, n, graphs, fuse)
            assert len(set(toks)) == 1 and toks[0] == lm_ref.sample(want, 50, 1.0, 0.0, 1.0, 3, 0), (name, fmt, start, n, toks)
    llm.set_graphs(True)
    llm.set_attn_fuse(True)


@CF
def test_prefill_matches_oracle(name, fmt):
    """MFMA prefill switched on (the default): the prompt through whatever route the shape gets, then a 2-token decode pass on top of
    the cache it left, against the oracle.  The wide cases repeat it with a prompt whose first pass is a full 1024-token pass (the
    lm_attn_flash_kernel<G, TEAMS> instance is computed from the device's CU count with the library's rule and printed)."""
    c = sc.BY_NAME[name]
    ids = c.ids().tolist()
    tol = sc.TOL_EXACT if c.route == "gemv" else sc.TOL_TILE
    for P in (c.prompt, c.long_prompt):
        if P is None:
            continue
        llm, ref = _fresh(name, fmt, True), _ref(name, fmt)
        teams = sc.flash_teams(c, sc.first_pass(c, fmt, P - 2), _n_cus())
        print(f"SHAPES {name}/{fmt} prefill of {P - 2}: route {llm.prefill_route()}, first pass {sc.first_pass(c, fmt, P - 2)} tokens"
              + (f", lm_attn_flash_kernel<{c.G}, {teams}> on {_n_cus()} CUs" if c.route != "gemv" else ""))
        llm.eval(ids[:P - 2])
        assert llm.n_tokens == P - 2
        _compare(f"{name}/{fmt} prefill of {P - 2} ({c.route})", llm._scores[-1].copy(), ref.eval(ids[:P - 2], last_only=True)[-1].numpy(), tol)
        llm.eval(ids[P - 2:P])
        _compare(f"{name}/{fmt} decode on the {c.route} cache at {P} keys", llm._scores[-1].copy(), ref.eval(ids[P - 2:P])[-1].numpy(), tol)


@CF
def test_route_is_the_one_the_table_claims(name, fmt):
    """rca_lm_prefill_route (the predicate rca_lm_eval branches on) against the table.  A case without a tile route must quietly use
    the exact GEMV passes with MFMA prefill switched on: same bits as with it switched off, through eval and through eval_async pieces."""
    c = sc.BY_NAME[name]
    ids = c.ids().tolist()
    llm = _fresh(name, fmt, True)
    assert llm.prefill_route() == c.route == sc.route(c, fmt), (name, fmt, llm.prefill_route())
    llm.set_mfma_prefill(False)
    assert llm.prefill_route() == "gemv"
    if c.route != "gemv":
        return
    P = c.prompt
    llm.eval(ids[:P])
    off = llm._scores[-1].copy()
    llm = _fresh(name, fmt, True)
    llm.eval(ids[:P])
    assert np.array_equal(llm._scores[-1], off), (name, fmt, "eval")
    llm.reset()
    for a, b in ((0, 13), (13, 163), (163, 170), (170, P)):       # a 7-token piece too: eval_async pieces are prefill whatever their size
        llm.eval_async(ids[a:b])
    llm.sync()
    assert llm.n_tokens == P and np.array_equal(llm._scores[-1], off), (name, fmt, "eval_async")


@CF
def test_bit_exactness_contracts(name, fmt):
    """Exact route: one long eval == a 9-token eval + 2-token evals == rollback via n_tokens + re-eval == 1-token evals (the body of
    test_prefill_equals_incremental_bit_exact, across the 256-key split).  Tile routes: two cuts of the prompt into pieces of more
    than 8 tokens, one with a piece of more than 128 (wide cases: more than 512) tokens so that the 128-row GEMMs take another
    form, leave the same logits and support the same decode pass."""
    c = sc.BY_NAME[name]
    ids = c.ids().tolist()
    P = c.prompt
    llm = _fresh(name, fmt, False)
    llm.eval(ids[:P])
    a = llm._scores[-1].copy()
    llm.reset()
    llm.eval(ids[:9])
    for i in range(9, P, 2):
        llm.eval(ids[i:min(i + 2, P)])
    assert llm.n_tokens == P and np.array_equal(llm._scores[-1], a), (name, fmt, "incremental")
    llm.n_tokens = P - 2
    llm.eval(ids[P - 2:P])
    assert np.array_equal(llm._scores[-1], a), (name, fmt, "rollback")
    llm.n_tokens = P - 9
    for i in range(P - 9, P):
        llm.eval([ids[i]])
    assert np.array_equal(llm._scores[-1], a), (name, fmt, "one-token evals")
    if c.route == "gemv":
        return
    cuts = [(P, ((0, P),), ((0, 13), (13, 163), (163, 172), (172, P)))]
    if c.long_prompt:
        L = c.long_prompt
        cuts.append((L, ((0, L),), ((0, 700), (700, 740), (740, L))))
    for n, cut_a, cut_b in cuts:
        outs = []
        for cut in (cut_a, cut_b):
            llm = _fresh(name, fmt, True)
            for lo, hi in cut:
                assert hi - lo > sc.LM_PREFILL_MIN
                llm.eval(ids[lo:hi])
            first = llm._scores[-1].copy()
            llm.eval(ids[n:n + 2])
            outs.append((first, llm._scores[-1].copy()))
        assert np.array_equal(outs[0][0], outs[1][0]), (name, fmt, n, "prefill logits depend on the cut")
        assert np.array_equal(outs[0][1], outs[1][1]), (name, fmt, n, "the caches the two cuts left differ")


@pytest.mark.parametrize("kv", ("f16", "q8_0"))
def test_split_v_file_pieces_and_one_pass_leave_the_same_cache(kv):
    """A Q4_K_M file whose layer 1 runs its V projection as a GEMM of its own (lm_split_v_case): one pass of 270 tokens (three token
    blocks, the last ragged) and pieces of 13, 150, 9 and 98 tokens leave the same logits and the same K / V bits in every layer."""
    import lm_split_v_case as sv
    ids, n = sv.ids(), 270
    outs = []
    for cut in (((0, n),), ((0, 13), (13, 163), (163, 172), (172, n))):
        llm = sv.family(1, kv)[0]
        llm.set_mfma_prefill(True)
        llm.set_graphs(True)
        llm.reset()
        for lo, hi in cut:
            assert hi - lo > sc.LM_PREFILL_MIN
            llm.eval(ids[lo:hi])
        state = [llm._scores[-1].copy()]
        for layer in range(llm.config.n_layers):
            state += [a.view(np.uint16).copy() for a in llm.kv_read(layer, 0, n)]
            if kv == "q8_0":
                state += [a.copy() if a.dtype == np.int8 else a.view(np.uint16).copy() for a in llm.kv_read_q8(layer, 0, n)]
        outs.append(state)
    assert len(outs[0]) == len(outs[1]) and all(a.any() for a in outs[0])
    for i, (a, b) in enumerate(zip(*outs)):
        assert a.shape == b.shape and np.array_equal(a, b), (kv, "logits" if i == 0 else f"K / V array {i - 1}", "depends on the cut")


def test_context_limit_inside_the_last_attention_split():
    """n_ctx = 700 (cache padded to 768 positions): decode and prefill up to within 2 tokens of n_ctx and up to n_ctx itself against
    the oracle; the eval that would pass n_ctx is refused with RCA_ERR_STATE and leaves n_tokens and the logits as they were."""
    from realtime_codec_agent_amd._native import RcaError
    name, fmt = "nctx700", "bf16"
    c = sc.BY_NAME[name]
    ids = c.ids().tolist()
    assert c.n_ctx == 700 and len(ids) == 700
    for mfma, tol in ((False, sc.TOL_EXACT), (True, sc.TOL_TILE)):
        llm, ref = _fresh(name, fmt, mfma), _ref(name, fmt)
        tag = f"{name} mfma_prefill={mfma}"
        llm.eval(ids[:696])
        _compare(f"{tag} eval of 696", llm._scores[-1].copy(), ref.eval(ids[:696], last_only=True)[-1].numpy(), tol)
        llm.eval(ids[696:698])
        got = llm._scores[-1].copy()
        _compare(f"{tag} decode at 698 keys", got, ref.eval(ids[696:698])[-1].numpy(), tol)
        for bad in (ids[:3], ids[:12]):                      # a decode-sized and a prefill-sized eval past the limit
            with pytest.raises(RcaError, match=r"rc=-3"):    # RCA_ERR_STATE
                llm.eval(bad)
            assert llm.n_tokens == 698 and np.array_equal(llm._scores[-1], got)
        llm.init_sampler_for_generate(**SAMPLER)
        with pytest.raises(RcaError, match=r"rc=-3"):
            llm.step(ids[:3])
        assert llm.n_tokens == 698
        tok = llm.step(ids[698:700])                         # the last two slots, through the graph
        want = ref.eval(ids[698:700])[-1].numpy()
        _compare(f"{tag} step to 700 keys (= n_ctx)", llm._scores[-1].copy(), want, tol)
        assert llm.n_tokens == 700 and tok == lm_ref.sample(llm._scores[-1], 50, 1.0, 0.0, 1.0, 3, 0)
        with pytest.raises(RcaError, match=r"rc=-3"):
            llm.eval(ids[:1])
        # a prompt of exactly n_ctx tokens in one eval
        llm.reset()
        llm.eval(ids)
        ref.reset()
        _compare(f"{tag} eval of 700 (= n_ctx)", llm._scores[-1].copy(), ref.eval(ids, last_only=True)[-1].numpy(), tol)


@pytest.mark.parametrize("fmt,kw", [("q8_0", dict(vocab=1001)), ("q4_k", dict(vocab=1002)), ("q8_0", dict(hidden=136)), ("q4_k", dict(hidden=192)),
                                    ("bf16", dict(n_heads=3, n_kv_heads=2)), ("bf16", dict(n_heads=8, n_kv_heads=1)), ("bf16", dict(ffn=3072)),
                                    ("bf16", dict(hidden=132))])
def test_shapes_outside_the_abi_are_refused_not_computed(fmt, kw):
    """what lm_shape_cases.rejected() says the library refuses, rca_lm_create refuses (with a message), for each rule once"""
    import dataclasses

    from realtime_codec_agent_amd._native import RcaError
    from realtime_codec_agent_amd.llm import LlamaForAlternatingCodeChannels
    c = dataclasses.replace(sc.BY_NAME["g4_tile32"], **kw)
    assert sc.rejected(c, fmt) is not None and sc.rejected(sc.BY_NAME["g4_tile32"], "q8_0") is None
    with pytest.raises(RcaError, match=r"rc=-1"):
        LlamaForAlternatingCodeChannels(model_path="random:refused", config=c.config(), n_ctx=512, random_seed=1, init_std=sc.INIT_STD,
                                        device=0, weight_format=fmt)
