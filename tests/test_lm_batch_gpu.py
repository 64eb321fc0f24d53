"""rca_lm_batch_step: 2 to 64 sessions over one set of weights stepped together as one token block of the 128-token MFMA tiles.

The batch step does not promise rca_lm_step's bits (the tiles round differently from the GEMVs); its contract, checked here:
  1. every member's logits against the fp32 oracle (LMRef on the member's own sequence) inside TOL_TILE, the project's tolerance for a
     decode on a tile-built cache -- the batch step is in that arithmetic class and gets no tolerance of its own;
  2. layer 0's K / V rows are, bit for bit, the rows rca_lm_eval_async writes for the same tokens at the same position (embedding,
     norm, QKV tile GEMM, RoPE: this pins the row-table epilogue);
  3. a member's logits and K / V rows do not depend on its slot, its companions, or graphs on / off;
  4. the sampled tokens are what oracle/sampler_oracle.c draws from the member's downloaded logits at its draw counter;
  5. single steps, group steps and batch steps mix;
  6. a refusal leaves every member as it was.

Start contexts come from {0, 1, 254, 255, 256, 257, 300, 511, 512, LAST}: an empty cache, both sides of the 256-key attention split
(n = 2 straddles it), and LAST = n_ctx - steps * n, so that the final step of a test starts at n_ctx - n and writes the last slot.  Every
batch then launches attention splits that some members do not have.  All members of a family evaluate prefixes of ONE id stream, so
the oracle walks the stream once per (model, format) and every member's steps are a short continuation of a truncated copy.
One more case (contract 2 and 3) runs the Q4_K_M file of lm_split_v_case, a layer of which has a V projection of its own.

Every test here fails on a library without rca_lm_batch_create / rca_lm_batch_step (the parent commit: LlamaBatch does not exist and
the symbols are missing)."""
import dataclasses
import functools

import numpy as np
import pytest
import torch

import lm_shape_cases as sc
from oracle import lm_ref

pytestmark = pytest.mark.gpu

SHAPES = ((5, 1), (33, 1), (17, 2), (64, 2), (2, 1))     # (members, tokens per member)
SHAPE_IDS = [f"{a}x{b}" for a, b in SHAPES]
STEPS = 3
FAMILY = 66                                               # parent + 65 twins: a full batch, the 65th member of the refusals, one spare
GREEDY = dict(top_k=1, top_p=1.0, min_p=0.0, temp=0.0, seed=1)
SAMPLERS = (                                              # members have different samplers and seeds
    GREEDY,
    dict(top_k=40, top_p=0.9, min_p=0.0, temp=0.9, seed=11, repeat_penalty=1.3, logit_bias={5: 4.0, 17: -3.0}),
    dict(top_k=50, top_p=1.0, min_p=0.0, temp=1.0, seed=13),
    dict(top_k=0, top_p=1.0, min_p=0.0, temp=1.0, seed=12),     # whole vocabulary: its own launches behind the table chain
)

G4 = sc.BY_NAME["g4_k768"]
MODELS = {
    "g4_k768": G4,
    "g1_k768": sc.BY_NAME["g1_k768"],
    "g2_k768": dataclasses.replace(G4, name="g2_k768", n_heads=6, n_kv_heads=3, seed=44),     # G = 2: 6 heads over 3 kv heads
}
# formats on one case, the three query group sizes in bf16
CASES = (("g4_k768", "bf16"), ("g4_k768", "f16"), ("g4_k768", "q8_0"), ("g4_k768", "q4_k"), ("g1_k768", "bf16"), ("g2_k768", "bf16"))
CASE_IDS = [f"{n}-{f}" for n, f in CASES]


def _ids(name):
    return MODELS[name].ids().tolist()


def _starts(name, nm, n, steps=STEPS):
    last = MODELS[name].n_ctx - steps * n
    pool = (0, 1, 254, 255, 256, 257, 300, 511, 512, last)
    if nm == 2:
        return [254, last]
    if nm == 5:
        return [0, 255, 300, 512, last]
    return [pool[s % len(pool)] for s in range(nm)]


def _rows(ids, nm, n, t, salt=0):
    """the n input tokens of member s at step t (a different stream per member)"""
    return [[ids[(500 + 31 * (s + salt) + n * t + j) % len(ids)] for j in range(n)] for s in range(nm)]


# ---------------------------------------------------------------------------------------------- handles and oracle, built once
@functools.lru_cache(maxsize=None)
def _family(name, fmt, which=0, size=FAMILY):
    from realtime_codec_agent_amd.llm import LlamaForAlternatingCodeChannels as L
    c = MODELS[name]
    parent = L(model_path=f"random:{name}", config=c.config(), n_ctx=c.n_ctx, random_seed=c.seed, init_std=sc.INIT_STD, device=0, weight_format=fmt)
    assert parent.weight_format == fmt and parent.prefill_route() == "gemm128"
    return [parent] + [L(n_ctx=c.n_ctx, share_weights_with=parent, device=0) for _ in range(size - 1)]


@functools.lru_cache(maxsize=None)
def _oracle(name, fmt):
    """LMRef after one walk over the whole id stream, and its full K / V (a member's oracle is a truncated copy + its own steps)"""
    c = MODELS[name]
    ref = lm_ref.LMRef(c.config(), sc.oracle_weights(c, fmt), kv_dtype=torch.float16)
    ref.eval(_ids(name)[:c.n_ctx], last_only=True, chunk=256)
    return ref, list(ref.k), list(ref.v)


def _oracle_at(name, fmt, ctx):
    ref, k, v = _oracle(name, fmt)
    ref.k, ref.v, ref.n_tokens = list(k), list(v), MODELS[name].n_ctx
    ref.set_n_tokens(ctx)
    return ref


def _prepare(members, ids, starts, graphs=True, samplers=(GREEDY,)):
    """every member at its start context (its cache built by eval: the tile route for more than 8 tokens), every switch at a known value"""
    for s, (llm, start) in enumerate(zip(members, starts)):
        llm.set_mfma_prefill(True)
        llm.set_graphs(graphs)
        llm.set_attn_fuse(True)
        llm.reset()
        if start:
            llm.eval(ids[:start])
        llm.init_sampler_for_generate(**samplers[s % len(samplers)])


def _kv_bits(llm, layer, pos, n):
    k, v = llm.kv_read(layer, pos, n)
    return k.view(np.uint16).copy(), v.view(np.uint16).copy()


# ---------------------------------------------------------------------------------------------- 1. against the fp32 oracle
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
@pytest.mark.parametrize("name,fmt", CASES, ids=CASE_IDS)
def test_batch_steps_match_the_oracle(name, fmt, shape):
    """Caches built by eval, then three batch steps (graph replay); after every step the logits of EVERY member against LMRef over
    the member's own sequence, inside bound(want, TOL_TILE)."""
    from realtime_codec_agent_amd.llm import LlamaBatch
    nm, n = shape
    ids = _ids(name)
    starts = _starts(name, nm, n)
    members = _family(name, fmt)[:nm]
    _prepare(members, ids, starts)
    bat = LlamaBatch(members)
    got = []
    try:
        for t in range(STEPS):
            bat.step(_rows(ids, nm, n, t))
            got.append([m._scores[-1].copy() for m in members])
    finally:
        bat.close()
    worst, where = 0.0, None
    for s in range(nm):
        ref = _oracle_at(name, fmt, starts[s])
        for t in range(STEPS):
            want = ref.eval(_rows(ids, nm, n, t)[s])[-1].numpy()
            ratio = float(np.abs(got[t][s] - want).max()) / sc.bound(want, sc.TOL_TILE)
            if ratio > worst:
                worst, where = ratio, (s, starts[s], t)
        assert members[s].n_tokens == starts[s] + STEPS * n
    print(f"BATCH {name}/{fmt} {nm}x{n}: worst max|dlogit| / bound(TOL_TILE) = {worst:.3f} at (member, start, step) {where}")
    assert worst <= 1.0, (name, fmt, shape, worst, where)


# ---------------------------------------------------------------------------------------------- 2. exact, layer 0
@pytest.mark.parametrize("shape", ((17, 2), (33, 1)), ids=("17x2", "33x1"))
@pytest.mark.parametrize("name,fmt", CASES, ids=CASE_IDS)
def test_layer0_kv_rows_are_eval_asyncs_bits(name, fmt, shape):
    """Layer 0's K / V rows depend on embedding, norm, the QKV tile GEMM and RoPE only: the rows a batch step writes for a member equal
    those a twin writes through rca_lm_eval_async for the same tokens at the same position."""
    from realtime_codec_agent_amd.llm import LlamaBatch
    nm, n = shape
    ids = _ids(name)
    starts = _starts(name, nm, n, steps=1)
    fam = _family(name, fmt)
    members, twin = fam[:nm], fam[FAMILY - 1]
    _prepare(members, ids, starts)
    rows = _rows(ids, nm, n, 0)
    bat = LlamaBatch(members)
    try:
        bat.step(rows)
    finally:
        bat.close()
    for s in range(nm):
        twin.n_tokens = starts[s]
        twin.eval_async(rows[s])
        twin.sync()
        kw, vw = _kv_bits(twin, 0, starts[s], n)
        kg, vg = _kv_bits(members[s], 0, starts[s], n)
        assert kw.any() and vw.any()
        assert np.array_equal(kg, kw), (name, fmt, "K rows of member", s, "at", starts[s])
        assert np.array_equal(vg, vw), (name, fmt, "V rows of member", s, "at", starts[s])


# ---------------------------------------------------------------------------------------------- 3. exact, independence
def _one_run(name, fmt, target, t_start, n, nm, slot, graphs, salt):
    """`target` at t_start in `slot` of an nm-member batch among companions drawn by `salt`; its logits and K / V rows of every layer"""
    from realtime_codec_agent_amd.llm import LlamaBatch
    ids = _ids(name)
    fam = [m for m in _family(name, fmt) if m is not target]
    members = fam[:nm - 1]
    members.insert(slot, target)
    starts = _starts(name, nm, n, steps=1)
    starts = starts[salt % nm:] + starts[:salt % nm]
    starts[slot] = t_start
    _prepare(members, ids, starts, graphs=graphs)
    rows = _rows(ids, nm, n, 0, salt=salt)
    rows[slot] = [ids[(900 + j) % len(ids)] for j in range(n)]
    bat = LlamaBatch(members)
    try:
        bat.step(rows)
    finally:
        bat.close()
        for m in members:
            m.set_graphs(True)
    out = [target._scores[-1].copy()]
    for layer in range(target.config.n_layers):
        out.extend(_kv_bits(target, layer, t_start, n))
    return out


@pytest.mark.parametrize("t_start,n", ((255, 2), (512, 1)), ids=("255+2", "512+1"))
@pytest.mark.parametrize("name,fmt", (("g4_k768", "bf16"), ("g4_k768", "q4_k"), ("g1_k768", "bf16")), ids=("g4-bf16", "g4-q4_k", "g1-bf16"))
def test_a_member_does_not_depend_on_slot_companions_or_graphs(name, fmt, t_start, n):
    target = _family(name, fmt)[FAMILY - 2]
    a = _one_run(name, fmt, target, t_start, n, 5, 0, True, 0)
    b = _one_run(name, fmt, target, t_start, n, 64, 40, True, 3)
    c = _one_run(name, fmt, target, t_start, n, 5, 0, False, 0)
    for tag, other in (("slot 40 of 64", b), ("eager", c)):
        for i, (x, y) in enumerate(zip(a, other)):
            assert np.array_equal(x, y), (name, fmt, tag, "logits" if i == 0 else f"K/V array {i - 1}")


def test_a_file_with_a_v_projection_of_its_own_steps_the_same_in_every_batch():
    """The Q4_K_M file of lm_split_v_case (layer 1: V as a GEMM of its own, row base in the row-table epilogue), 5 x 2 rows of one token
    block.  The target's token, logits and K / V rows of every layer in slot 0 of 5 (graph replay) equal those in slot 1 of the smallest
    batch (two members, eager, another companion); its layer-0 rows equal those its own rca_lm_eval_async writes."""
    import lm_split_v_case as sv
    from realtime_codec_agent_amd.llm import LlamaBatch
    fam, ids = sv.family(6), sv.ids()
    target, twin, t_start, n = fam[4], fam[5], 257, 2
    cur = [ids[280], ids[281]]
    outs = []
    for members, starts, graphs in (([target] + fam[:4], [t_start, 0, 1, 255, 31], True), ([fam[3], target], [130, t_start], False)):
        _prepare(members, ids, starts, graphs=graphs)
        rows = [cur if m is target else [ids[(200 + 7 * s + j) % len(ids)] for j in range(n)] for s, m in enumerate(members)]
        bat = LlamaBatch(members)
        try:
            for _ in range(2 if graphs else 1):                      # (with graphs: once more from the same positions, a replay)
                for m, s in zip(members, starts):
                    m.n_tokens = s
                toks = bat.step(rows)
        finally:
            bat.close()
            for m in members:
                m.set_graphs(True)
        out = [np.asarray(toks[members.index(target)]), target._scores[-1].copy()]
        for layer in range(target.config.n_layers):
            out.extend(_kv_bits(target, layer, t_start, n))
        outs.append(out)
    assert all(a.any() for a in outs[0][1:])
    for i, (x, y) in enumerate(zip(*outs)):
        assert np.array_equal(x, y), ("token", "logits")[i] if i < 2 else f"K/V array {i - 2}"
    _prepare([twin], ids, [t_start])
    twin.eval_async(cur)
    twin.sync()
    for got, want in zip(outs[0][2:4], _kv_bits(twin, 0, t_start, n)):
        assert np.array_equal(got, want), "layer 0 rows differ from eval_async's"


@pytest.mark.parametrize("nm,n", ((33, 1), (17, 2)), ids=("33x1", "17x2"))
def test_identical_members_get_identical_logits_in_every_slot(nm, n):
    from realtime_codec_agent_amd.llm import LlamaBatch
    name, fmt = "g4_k768", "q8_0"
    ids = _ids(name)
    members = _family(name, fmt)[:nm]
    _prepare(members, ids, [300] * nm)
    bat = LlamaBatch(members)
    try:
        toks = bat.step([ids[700:700 + n]] * nm)
    finally:
        bat.close()
    first = members[0]._scores[-1].copy()
    for s in range(1, nm):
        assert np.array_equal(members[s]._scores[-1], first), s
    assert len(set(toks)) == 1


# ---------------------------------------------------------------------------------------------- 4. sampler
def _sampler_run(name, fmt, nm, n, graphs, steps=4):
    from realtime_codec_agent_amd.llm import LlamaBatch
    ids = _ids(name)
    starts = _starts(name, nm, n, steps=steps)
    members = _family(name, fmt)[:nm]
    _prepare(members, ids, starts, graphs=graphs, samplers=SAMPLERS)
    bat = LlamaBatch(members)
    toks, logits = [], []
    try:
        for t in range(steps):
            toks.append(bat.step(_rows(ids, nm, n, t)))
            logits.append([m._scores[-1].copy() for m in members])
    finally:
        bat.close()
        for m in members:
            m.set_graphs(True)
    return toks, logits


@pytest.mark.parametrize("nm,n", ((9, 1), (6, 2)), ids=("9x1", "6x2"))
def test_tokens_are_the_sampler_oracles_draws(nm, n):
    """greedy / top_k 40 + top_p + repeat penalty + bias / top_k 50 / whole vocabulary, every member its own seed, four consecutive
    steps (penalty windows and draw counters must have advanced): token for token the C restatement's draw from the member's
    downloaded logits; the eager run gives the graph run's tokens and logits."""
    name, fmt = "g4_k768", "bf16"
    toks, logits = _sampler_run(name, fmt, nm, n, True)
    for s in range(nm):
        p = SAMPLERS[s % len(SAMPLERS)]
        hist = []
        for t in range(len(toks)):
            want = lm_ref.sample(logits[t][s], p["top_k"], p["top_p"], p["min_p"], p["temp"], p["seed"], t, p.get("logit_bias"),
                                 repeat_penalty=p.get("repeat_penalty", 1.0), prev_tokens=hist)
            assert toks[t][s] == want, ("member", s, "step", t, toks[t][s], want)
            hist.append(want)
    toks_e, logits_e = _sampler_run(name, fmt, nm, n, False)
    assert toks_e == toks
    for t in range(len(toks)):
        for s in range(nm):
            assert np.array_equal(logits_e[t][s], logits[t][s]), (t, s)


# ---------------------------------------------------------------------------------------------- 5. mixing
@pytest.mark.parametrize("graphs", (True, False), ids=("graph", "eager"))
def test_single_group_and_batch_steps_mix(graphs):
    """Two families over the same values take the same batch steps; then rca_lm_step on member 0 and a LlamaGroup step on members 1 and
    2 of one family give what the same calls give on the other, and a further batch step on both agrees too."""
    from realtime_codec_agent_amd.llm import LlamaBatch, LlamaGroup
    name, fmt, nm, n = "g4_k768", "q8_0", 6, 2
    ids = _ids(name)
    starts = [254, 40, 300, 0, 511, 257]
    fams = [_family(name, fmt, which, 8)[:nm] for which in (1, 2)]
    res = []
    for fam in fams:
        _prepare(fam, ids, starts, graphs=graphs, samplers=SAMPLERS)
        bat = LlamaBatch(fam)
        grp = LlamaGroup(fam[1:3])
        try:
            out = [bat.step(_rows(ids, nm, n, t)) for t in range(2)]
            out.append(fam[0].step(ids[600:602]))
            out.append(grp.step([ids[610:612], ids[620:622]]))
            out.append(fam[0].sample())                  # the member's logits are where rca_lm_sample finds them
            out.append(bat.step(_rows(ids, nm, n, 2)))
        finally:
            grp.close()
            bat.close()
            for m in fam:
                m.set_graphs(True)
        res.append((out, [m._scores[-1].copy() for m in fam], [m.n_tokens for m in fam],
                    [_kv_bits(m, 1, starts[s], m.n_tokens - starts[s]) for s, m in enumerate(fam)]))
    (oa, la, na, ka), (ob, lb, nb, kb) = res
    assert oa == ob and na == nb == [starts[0] + 8] + [s + 8 for s in starts[1:3]] + [s + 6 for s in starts[3:]]
    for s in range(nm):
        assert np.array_equal(la[s], lb[s]), s
        assert np.array_equal(ka[s][0], kb[s][0]) and np.array_equal(ka[s][1], kb[s][1]), s


# ---------------------------------------------------------------------------------------------- 6. refusals
def _snapshot(members, n=2):
    return [(m.n_tokens, m._scores[-1].copy(), [_kv_bits(m, l, m.n_tokens, n) for l in range(m.config.n_layers)]) for m in members]


def _assert_unchanged(members, snap, tag):
    for s, (m, (nt, lg, kv)) in enumerate(zip(members, snap)):
        assert m.n_tokens == nt, (tag, s)
        assert np.array_equal(m._scores[-1], lg), (tag, s)
        for l, (k, v) in enumerate(kv):
            k2, v2 = _kv_bits(m, l, nt, k.shape[0])
            assert np.array_equal(k, k2) and np.array_equal(v, v2), (tag, s, l)


def test_refusals_leave_every_member_unchanged():
    from realtime_codec_agent_amd import _native as N
    from realtime_codec_agent_amd.llm import LlamaForAlternatingCodeChannels as L, LlamaBatch
    name, fmt = "g4_k768", "bf16"
    c = MODELS[name]
    ids = _ids(name)
    fam = _family(name, fmt)
    B = fam[:5]
    _prepare(B, ids, [30, 40, 254, 300, 511])
    V = c.vocab
    bat = LlamaBatch(B)
    try:
        bat.step(_rows(ids, 5, 2, 0))                  # logits to snapshot
        snap = _snapshot(B)
        # one member a token short of n_ctx (the others have room)
        keep = B[3].n_tokens
        B[3].n_tokens = c.n_ctx - 1
        with pytest.raises(N.RcaError, match="context overflow of member 3"):
            bat.step(_rows(ids, 5, 2, 1))
        assert B[3].n_tokens == c.n_ctx - 1
        B[3].n_tokens = keep
        _assert_unchanged(B, snap, "context overflow")
        rows = _rows(ids, 5, 2, 1)
        rows[4][1] = V                                 # an id equal to V
        with pytest.raises(N.RcaError, match="of member 4 at index 1 is outside the vocabulary"):
            bat.step(rows)
        _assert_unchanged(B, snap, "id == V")
        with pytest.raises(N.RcaError, match="3 tokens per member"):
            bat.step([[1, 2, 3]] * 5)
        _assert_unchanged(B, snap, "n = 3")
        # 65 members (so also 65 x 2 rows) never become a batch
        with pytest.raises(N.RcaError, match="65 members"):
            LlamaBatch(fam[:65])
        with pytest.raises(N.RcaError, match="member 1 is the same handle as member 0"):
            LlamaBatch([B[0], B[0]])
        other = _family(name, fmt, 1, 8)[0]            # the same values, but its own weights
        with pytest.raises(N.RcaError, match="member 1 does not share member 0's weights"):
            LlamaBatch([B[0], other])
        twin_all = L(n_ctx=c.n_ctx, share_weights_with=B[0], device=0, logits_all=True)
        try:
            with pytest.raises(N.RcaError, match="member 1 is a logits_all handle"):
                LlamaBatch([B[0], twin_all])
        finally:
            twin_all.close()
        bare = L(n_ctx=c.n_ctx, share_weights_with=B[0], device=0)
        try:
            b2 = LlamaBatch([B[0], B[1], bare])
            try:
                with pytest.raises(N.RcaError, match="member 2 has no sampler"):
                    b2.step([[1], [2], [3]])
            finally:
                b2.close()
        finally:
            bare.close()
        # a model without the 128-token tile route stays with the group step
        t32 = sc.BY_NAME["g4_tile32"]
        p32 = L(model_path="random:g4_tile32", config=t32.config(), n_ctx=t32.n_ctx, random_seed=t32.seed, init_std=sc.INIT_STD, device=0, weight_format="bf16")
        w32 = L(n_ctx=t32.n_ctx, share_weights_with=p32, device=0)
        try:
            assert p32.prefill_route() == "tile32"
            with pytest.raises(N.RcaError, match="member 0 does not take the 128-token tiles"):
                LlamaBatch([p32, w32])
        finally:
            w32.close()
            p32.close()
        _assert_unchanged(B, snap, "create refusals")
        # and the batch still steps from the unchanged state
        bat.step(_rows(ids, 5, 2, 1))
        assert [m.n_tokens for m in B] == [nt + 2 for nt, _, _ in snap]
    finally:
        bat.close()
