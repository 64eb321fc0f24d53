"""rca_lm_group_step: sessions that share one set of weights stepped together must end, bit for bit, where their own rca_lm_step calls
would have left them.

The oracle is the library's own single step: rca_lm_step is pinned to the fp32 oracle by the existing suite (test_lm_gpu.py,
test_lm_shapes_gpu.py, ...) and the group step does not touch it.  Two families of handles are made from the same seed (a parent and
its share_weights_with= twins each): family A is stepped one handle at a time, family B through a LlamaGroup.  Everything compared is
compared with array_equal -- all V logits of every member, the sampled tokens, the K / V rows of every layer over the written
positions.  There is no tolerance anywhere in this file.

Every test here fails on a library without rca_lm_group_create / rca_lm_group_step."""
import functools

import numpy as np
import pytest

import lm_shape_cases as sc

pytestmark = pytest.mark.gpu

SHAPES = ((2, 1), (2, 2), (4, 1))          # (members, tokens per member): every row count the ABI accepts
STEPS = 6
GREEDY = dict(top_k=1, top_p=1.0, min_p=0.0, temp=0.0, seed=1)
SAMPLERS = (                                   # members have different samplers and seeds
    GREEDY,
    dict(top_k=40, top_p=0.9, min_p=0.0, temp=0.9, seed=11, repeat_penalty=1.3, logit_bias={5: 4.0, 17: -3.0}),
    dict(top_k=0, top_p=1.0, min_p=0.0, temp=1.0, seed=12),     # whole vocabulary
    dict(top_k=50, top_p=1.0, min_p=0.0, temp=1.0, seed=13),
)


# ---------------------------------------------------------------------------------------------- models
def _q5k_config():
    import lm_q5k_cases
    return lm_q5k_cases.file_config("q5_k")


def _q40_config():
    import lm_q40_cases
    return lm_q40_cases.file_config("q4_0")


def _model(name):
    """(config, n_ctx, weight seed, ids)"""
    if name in sc.BY_NAME:
        c = sc.BY_NAME[name]
        return c.config(), c.n_ctx, c.seed, c.ids()
    cfg = {"q5k_file": _q5k_config, "q40_file": _q40_config}[name]()       # the models of tests/lm_q5k_cases.py / lm_q40_cases.py
    return cfg, 1024, 5, np.random.default_rng(77).integers(0, cfg.vocab_size, 1024).astype(np.int64)


# case, weight format, activation format: both activation formats on every packed case
CASES = (
    ("g4_tile32", "bf16", "f32"),
    ("h136_fallback", "bf16", "f32"),            # a partly idle wave, K = 17 / 33 chunks
    ("g1_gemm128_ffn6144", "bf16", "f32"),       # the NIT = 4 down projection
    ("g1_gemm128_ffn6144", "f16", "f32"),
    ("g1_gemm128_ffn6144", "q8_0", "f32"), ("g1_gemm128_ffn6144", "q8_0", "q8_1"),
    ("g1_gemm128_ffn6144", "q4_k", "f32"), ("g1_gemm128_ffn6144", "q4_k", "q8_1"),
    ("g4_k768", "q4_k", "f32"), ("g4_k768", "q4_k", "q8_1"),
    ("g4_k768", "q8_0", "f32"), ("g4_k768", "q8_0", "q8_1"),
    ("q5k_file", "q5_k", "f32"), ("q5k_file", "q5_k", "q8_1"),
    ("q40_file", "q4_0", "f32"), ("q40_file", "q4_0", "q8_1"),
)


@functools.lru_cache(maxsize=None)
def _families(name, fmt):
    """two families over the same values: [parent, twin, twin, twin] each, and one spare twin per family (swap_kv partner)"""
    from realtime_codec_agent_amd.llm import LlamaForAlternatingCodeChannels as L
    cfg, n_ctx, seed, _ = _model(name)
    fams = []
    for _ in range(2):
        parent = L(model_path=f"random:{name}", config=cfg, n_ctx=n_ctx, random_seed=seed, init_std=sc.INIT_STD, device=0, weight_format=fmt)
        assert parent.weight_format == fmt
        fams.append([parent] + [L(n_ctx=n_ctx, share_weights_with=parent, device=0) for _ in range(4)])
    return fams


def _prepare(name, fmt, act, starts, graphs, samplers):
    """members of both families at the start contexts (same prefill on both), every switch at a known value"""
    A, B = _families(name, fmt)
    ids = _model(name)[3].tolist()
    for fam in (A, B):
        for llm in fam:       # the whole family first: a group refuses members of mixed activation formats
            llm.set_activation_format(act)
            llm.set_graphs(graphs)
            llm.set_attn_fuse(True)
        for s, start in enumerate(starts):
            llm = fam[s]
            llm.reset()
            if start:
                llm.eval(ids[7 * s:7 * s + start])
            llm.init_sampler_for_generate(**samplers[s % len(samplers)])
    return A[:len(starts)], B[:len(starts)], ids


def _rows(ids, starts, n, t):
    """the n input tokens of member s at step t (a different stream per member)"""
    return [[ids[(500 + 31 * s + n * t + j) % len(ids)] for j in range(n)] for s in range(len(starts))]


def _assert_same_state(tag, A, B, starts, ends):
    for s, (a, b) in enumerate(zip(A, B)):
        assert a.n_tokens == b.n_tokens == ends[s], (tag, s, a.n_tokens, b.n_tokens, ends[s])
        la, lb = a._scores[-1], b._scores[-1]
        assert np.array_equal(la, lb), (tag, "logits of member", s, float(np.abs(la - lb).max()))
        assert np.array_equal(a._input_ids[:ends[s]], b._input_ids[:ends[s]]), (tag, "recorded ids of member", s)
        if ends[s] > starts[s]:
            for layer in range(a.config.n_layers):
                ka, va = a.kv_read(layer, starts[s], ends[s] - starts[s])
                kb, vb = b.kv_read(layer, starts[s], ends[s] - starts[s])
                assert np.array_equal(ka.view(np.uint16), kb.view(np.uint16)), (tag, "K rows of member", s, "layer", layer)
                assert np.array_equal(va.view(np.uint16), vb.view(np.uint16)), (tag, "V rows of member", s, "layer", layer)


def _run(tag, name, fmt, act, shape, starts, graphs, samplers=SAMPLERS, steps=STEPS, check_every_step=True):
    from realtime_codec_agent_amd.llm import LlamaGroup
    nm, n = shape
    A, B, ids = _prepare(name, fmt, act, starts[:nm], graphs, samplers)
    grp = LlamaGroup(B)
    try:
        pos = list(starts[:nm])
        for t in range(steps):
            rows = _rows(ids, pos, n, t)
            want = [a.step(r) for a, r in zip(A, rows)]
            got = grp.step(rows)
            assert got == want, (tag, "tokens at step", t, got, want)
            before, pos = pos, [p + n for p in pos]
            if check_every_step:
                _assert_same_state(f"{tag} step {t}", A, B, before, pos)
        _assert_same_state(tag, A, B, starts[:nm], pos)
    finally:
        grp.close()


# ---------------------------------------------------------------------------------------------- 1. shapes x cases x formats
@pytest.mark.parametrize("shape", SHAPES, ids=[f"{a}x{b}" for a, b in SHAPES])
@pytest.mark.parametrize("name,fmt,act", CASES, ids=[f"{n}-{f}-{a}" for n, f, a in CASES])
def test_group_step_equals_single_steps(name, fmt, act, shape):
    """Members at 0, 254, 300 and 255 tokens (the pair step writes across the 256-key split), six steps, graph replay."""
    _run(f"{name}/{fmt}/{act} {shape}", name, fmt, act, shape, (0, 254, 300, 255), True)


# ---------------------------------------------------------------------------------------------- 2. positions, 3. eager and graphs
@pytest.mark.parametrize("graphs", (True, False), ids=("graph", "eager"))
@pytest.mark.parametrize("shape", SHAPES, ids=[f"{a}x{b}" for a, b in SHAPES])
def test_members_in_different_context_buckets(shape, graphs):
    """n_ctx 1280: a member at 1030 tokens (5 splits, graph bucket 1) beside members at 10, 254 and 511 tokens (bucket 0): every
    attention launch takes the larger bucket's split count, the later splits of the short members exit at once."""
    _run(f"buckets {shape} graphs={graphs}", "g1_gemm128_ffn6144", "bf16", "f32", shape, (1030, 10, 254, 511), graphs)


@pytest.mark.parametrize("shape", SHAPES, ids=[f"{a}x{b}" for a, b in SHAPES])
@pytest.mark.parametrize("name,fmt,act", (("g4_tile32", "bf16", "f32"), ("g4_k768", "q4_k", "q8_1"), ("h136_fallback", "bf16", "f32")),
                         ids=("g4_tile32-bf16", "g4_k768-q4_k-q8_1", "h136-bf16"))
def test_eager_group_step(name, fmt, act, shape):
    """graphs switched off on the members: the same launches, enqueued one by one"""
    _run(f"eager {name}/{fmt}/{act} {shape}", name, fmt, act, shape, (0, 254, 300, 255), False)


def test_set_graphs_off_on_one_member_makes_the_group_eager_and_back():
    from realtime_codec_agent_amd.llm import LlamaGroup
    A, B, ids = _prepare("g4_tile32", "bf16", "f32", (3, 254), True, SAMPLERS)
    grp = LlamaGroup(B)
    try:
        pos = [3, 254]
        for t, off in enumerate((None, 1, None, 0, None)):
            if off is not None:
                B[off].set_graphs(False)
            elif t:
                for b in B:
                    b.set_graphs(True)
            rows = _rows(ids, pos, 2, t)
            assert grp.step(rows) == [a.step(r) for a, r in zip(A, rows)], t
            before, pos = pos, [p + 2 for p in pos]
            _assert_same_state(f"graphs toggled, step {t}", A, B, before, pos)
    finally:
        grp.close()
        for b in B:
            b.set_graphs(True)


@pytest.mark.parametrize("shape", ((2, 2), (2, 1)), ids=("2x2", "2x1"))
def test_graph_replay_after_swap_kv_recaptures(shape):
    """A captured group graph holds the members' cache addresses.  After rca_lm_swap_kv of a member with a twin that holds a copy of its
    cache, the member's epoch differs and the group captures again: the new rows land in the cache the member has NOW (a stale graph
    would write the old one, and the K / V comparison below would find the rows missing)."""
    from realtime_codec_agent_amd.llm import LlamaGroup
    nm, n = shape
    name, fmt = "g4_tile32", "bf16"
    A, B, ids = _prepare(name, fmt, "f32", (20, 254), True, SAMPLERS)
    spare_a, spare_b = _families(name, fmt)[0][4], _families(name, fmt)[1][4]
    grp = LlamaGroup(B)
    try:
        pos = [20, 254]
        t = 0
        for phase in range(3):
            for _ in range(2):
                rows = _rows(ids, pos, n, t)
                assert grp.step(rows) == [a.step(r) for a, r in zip(A, rows)], (phase, t)
                before, pos = pos, [p + n for p in pos]
                _assert_same_state(f"swap_kv phase {phase} step {t}", A, B, before, pos)
                t += 1
            if phase < 2:      # member 1 (phase 0), then member 0 (phase 1), trades caches with the spare twin of its family
                s = 1 - phase
                for fam, spare in ((A, spare_a), (B, spare_b)):
                    spare.copy_kv_from(fam[s], pos[s])
                    spare.sync()
                    keep = fam[s].n_tokens
                    fam[s].swap_kv(spare)
                    fam[s].n_tokens = keep
    finally:
        grp.close()


# ---------------------------------------------------------------------------------------------- 4. interleaving
@pytest.mark.parametrize("graphs", (True, False), ids=("graph", "eager"))
def test_group_and_single_steps_interleave(graphs):
    """member 0: group step, its own step(), group step == three single steps.  Member 1 sits out the middle one."""
    from realtime_codec_agent_amd.llm import LlamaGroup
    A, B, ids = _prepare("g4_k768", "q8_0", "f32", (254, 40), graphs, SAMPLERS)
    grp = LlamaGroup(B)
    try:
        r0, r1, r2 = (_rows(ids, (254, 40), 2, t) for t in range(3))
        assert grp.step(r0) == [A[0].step(r0[0]), A[1].step(r0[1])]
        assert B[0].step(r1[0]) == A[0].step(r1[0])
        _assert_same_state("after the single step", A, B, (254, 40), (258, 42))
        assert B[0].sample() == A[0].sample()          # the member's logits are where rca_lm_sample finds them
        assert grp.step(r2) == [A[0].step(r2[0]), A[1].step(r2[1])]
        _assert_same_state("group, single, group", A, B, (254, 40), (260, 44))
        assert np.array_equal(A[0].token_probs([1, 2, 3]), B[0].token_probs([1, 2, 3]))
    finally:
        grp.close()


# ---------------------------------------------------------------------------------------------- 5. samplers
@pytest.mark.parametrize("shape", SHAPES, ids=[f"{a}x{b}" for a, b in SHAPES])
def test_members_with_different_samplers(shape):
    """greedy / top_k 40 + top_p 0.9 + repeat penalty + logit bias / top_k 0 (whole vocabulary) / top_k 50, every member its own seed:
    20 steps, so that the penalty window and the draw counters matter.  A sampler of another kind set on a member between steps
    changes the launch sequence: the group captures again."""
    from realtime_codec_agent_amd.llm import LlamaGroup
    nm, n = shape
    _run(f"samplers {shape}", "g4_tile32", "bf16", "f32", shape, (5, 254, 300, 17), True, steps=20, check_every_step=False)
    rot = SAMPLERS[1:] + SAMPLERS[:1]
    A, B, ids = _prepare("g4_tile32", "bf16", "f32", (5, 254, 300, 17)[:nm], True, SAMPLERS)
    grp = LlamaGroup(B)
    try:
        pos = [5, 254, 300, 17][:nm]
        for t in range(6):
            if t == 3:
                for fam in (A, B):
                    for s, llm in enumerate(fam):
                        llm.init_sampler_for_generate(**rot[s])
            rows = _rows(ids, pos, n, t)
            assert grp.step(rows) == [a.step(r) for a, r in zip(A, rows)], t
            pos = [p + n for p in pos]
        _assert_same_state(f"samplers changed {shape}", A, B, [5, 254, 300, 17][:nm], pos)
    finally:
        grp.close()


# ---------------------------------------------------------------------------------------------- 6. refusals
def _snapshot(members):
    return [(m.n_tokens, m._scores[-1].copy()) for m in members]


def _assert_unchanged(members, snap, tag):
    for s, (m, (n, lg)) in enumerate(zip(members, snap)):
        assert m.n_tokens == n, (tag, s)
        assert np.array_equal(m._scores[-1], lg), (tag, s)


def test_refusals_leave_every_member_unchanged():
    from realtime_codec_agent_amd import _native as N
    from realtime_codec_agent_amd.llm import LlamaForAlternatingCodeChannels as L, LlamaGroup
    name, fmt = "g4_tile32", "bf16"
    A, B, ids = _prepare(name, fmt, "f32", (30, 40, 50), True, SAMPLERS)
    cfg, n_ctx, seed, _ = _model(name)
    V = cfg.vocab_size
    grp = LlamaGroup(B[:2])
    try:
        snap = _snapshot(B)
        # a member one token short of n_ctx (the other member has room)
        B[1].n_tokens = n_ctx - 1
        with pytest.raises(N.RcaError, match="context overflow of member 1"):
            grp.step([[1, 2], [3, 4]])
        assert B[0].n_tokens == 30 and B[1].n_tokens == n_ctx - 1
        B[1].n_tokens = 40
        _assert_unchanged(B, snap, "context overflow")
        # an id equal to V
        with pytest.raises(N.RcaError, match="outside the vocabulary"):
            grp.step([[1, 2], [3, V]])
        _assert_unchanged(B, snap, "id == V")
        # 2 x 3 = 6 rows
        with pytest.raises(N.RcaError, match="6 rows"):
            grp.step([[1, 2, 3], [4, 5, 6]])
        _assert_unchanged(B, snap, "6 rows")
        # 3 x 1 = 3 rows
        grp3 = LlamaGroup(B[:3])
        try:
            with pytest.raises(N.RcaError, match="3 rows"):
                grp3.step([[1], [2], [3]])
        finally:
            grp3.close()
        _assert_unchanged(B, snap, "3 rows")
        # duplicate members
        with pytest.raises(N.RcaError, match="member 1 is the same handle as member 0"):
            LlamaGroup([B[0], B[0]])
        # an unrelated handle: the same values, but its own weights
        with pytest.raises(N.RcaError, match="member 1 does not share member 0's weights"):
            LlamaGroup([B[0], A[0]])
        # a logits_all member
        twin_all = L(n_ctx=n_ctx, share_weights_with=B[0], device=0, logits_all=True)
        try:
            with pytest.raises(N.RcaError, match="member 1 is a logits_all handle"):
                LlamaGroup([B[0], twin_all])
        finally:
            twin_all.close()
        # a member without a sampler
        bare = L(n_ctx=n_ctx, share_weights_with=B[0], device=0)
        try:
            g2 = LlamaGroup([B[0], bare])
            try:
                with pytest.raises(N.RcaError, match="member 1 has no sampler"):
                    g2.step([[1], [2]])
            finally:
                g2.close()
        finally:
            bare.close()
        _assert_unchanged(B, snap, "create refusals")
        # and the group still steps, from the unchanged state, as the single handles do
        rows = [[ids[1], ids[2]], [ids[3], ids[4]]]
        assert grp.step(rows) == [A[0].step(rows[0]), A[1].step(rows[1])]
        _assert_same_state("after the refusals", A[:2], B[:2], (30, 40), (32, 42))
    finally:
        grp.close()


def test_mixed_activation_formats_are_refused():
    from realtime_codec_agent_amd import _native as N
    from realtime_codec_agent_amd.llm import LlamaGroup
    A, B, ids = _prepare("g4_k768", "q8_0", "f32", (10, 20), True, SAMPLERS)
    B[1].set_activation_format("q8_1")
    try:
        with pytest.raises(N.RcaError, match="member 1 has activation format 1"):
            LlamaGroup(B)
    finally:
        B[1].set_activation_format("f32")
    grp = LlamaGroup(B)
    try:
        snap = _snapshot(B)
        B[1].set_activation_format("q8_1")      # after the group was made: refused at the step, nothing changed
        with pytest.raises(N.RcaError, match="member 1 has activation format 1"):
            grp.step([[1], [2]])
        B[1].set_activation_format("f32")
        _assert_unchanged(B, snap, "activation format changed under the group")
        rows = [[ids[1]], [ids[2]]]
        assert grp.step(rows) == [A[0].step(rows[0]), A[1].step(rows[1])]
        _assert_same_state("after set_act_format there and back", A, B, (10, 20), (11, 21))
    finally:
        grp.close()
