"""rca_lm_batch_step_sel / LlamaBatch.step_probe: a batch step of 1 or 2 tokens over a SUBSET of the members that also returns token
probabilities (rca_lm_step_probe for a selection).

The contract is bit for bit.  Family B is ONE batch over 64 members and runs step_probe(members=sel, ...); family A (its own weights,
the same values) runs LlamaBatch(only those members).step(rows), then token_probs(probe ids) on each member.  Checked here:
  1. selected members: tokens, probability bytes, logits, n_tokens, the K / V bits of every layer at the new positions and the next
     batch step's tokens, for selections of 2, 9, 33 and 64 members, an unsorted one and one with slot 63; n 1 and 2; 0, 1, 2 and 8
     probe ids; starts from {0, 254, 255, 256, 511, n_ctx - n}; one case over the q8_0 KV cache; a selection of 1 against the same
     member in one of 2;
  2. the roll-back the agent makes: n_tokens -= n, then a selection frame gives the plain batch frame's bits;
  3. unselected members: EVERY row of the K / V cache of every layer, n_tokens, the logits and the next draw, one of them with a full
     cache and one without a sampler;
  4. graphs on == off; a selection with a whole-vocabulary sampler; three consecutive calls with other selections;
  5. every probability against a float64 softmax of the member's downloaded logits (1e-6 relative: float32 exp and division round at
     2^-24 = 6e-8 each, the sum of the vocabulary's terms is taken in slices and adds about as much; this guards the id stride, the
     byte equality of 1 is the real check);
  6. captures: selections of 9, 12 and 16 members share one capture, also after a member's swap_kv; 17 take one more; the selection
     frame and the duplex batch frame keep their own graphs;
  7. refusals leave every member unchanged.
All comparisons but 5 are np.array_equal / tobytes.  Models, samplers and helpers are those of tests/test_lm_batch_gpu.py,
tests/test_lm_batch_frame_gpu.py and tests/test_lm_batch_sel_gpu.py (imported, so the files share one family cache).

Every test here fails on a library without rca_lm_batch_step_sel (the parent commit: LlamaBatch.step_probe does not exist and the
symbol is missing)."""
import functools

import numpy as np
import pytest

import lm_shape_cases as sc
import test_lm_batch_frame_gpu as bf
import test_lm_batch_gpu as bg
import test_lm_batch_sel_gpu as bs

pytestmark = pytest.mark.gpu

FAMILY = bg.FAMILY
WHICH_B = bf.WHICH_B
SERIAL = bs.SERIAL
NB = bs.NB
SELECTIONS = {k: bs.SELECTIONS[k] for k in ("2", "9", "33", "64", "unsorted", "slot63")}


def _starts(n_ctx, nm, n):
    pool = (0, 254, 255, 256, 511, n_ctx - n)
    return [pool[k % len(pool)] for k in range(nm)]


def _probes(vocab, nm, n_probe):
    return [[(5 + 100 * k + 37 * i) % vocab for i in range(n_probe)] for k in range(nm)]


def _check_probs(m, ids, probs, tag):
    """item 5: float64 softmax of the member's downloaded logits"""
    lg = m._scores[-1].astype(np.float64)
    want = np.exp(lg - lg.max())
    want = want[ids] / want.sum()
    assert np.all(np.abs(probs.astype(np.float64) - want) <= 1e-6 * want), (tag, probs, want)


def _step_sel_against_own_batch(A, B, bb, sel, ids, vocab, n, n_probe, tag, graphs_b=True, samplers=SERIAL, salt=0, prepare=True, starts=None):
    """step_probe(members=sel) of the batch bb (B = its selected members) against step() of a batch over A, then token_probs per member;
    both families are left one step past their starts"""
    from realtime_codec_agent_amd.llm import LlamaBatch
    nm = len(sel)
    if starts is None:
        starts = _starts(A[0].n_ctx(), nm, n)
    if prepare:
        bg._prepare(A, ids, starts, samplers=samplers)
        bg._prepare(B, ids, starts, graphs=graphs_b, samplers=samplers)
    rows = bg._rows(ids, nm, n, 0, salt=salt)
    probes = _probes(vocab, nm, n_probe)
    ba = LlamaBatch(A)
    try:
        want = ba.step(rows)
        wprobs = [A[k].token_probs(probes[k]) for k in range(nm)] if n_probe else None
    finally:
        ba.close()
    got, probs = bb.step_probe(sel, rows, probes if n_probe else None)
    assert got == want, (tag, "tokens")
    if n_probe:
        assert probs.shape == (nm, n_probe) and probs.dtype == np.float32
        for k in range(nm):
            assert probs[k].tobytes() == wprobs[k].tobytes(), (tag, "probabilities of k", k, probs[k], wprobs[k])
            _check_probs(B[k], probes[k], probs[k], (tag, "softmax of k", k))
    else:
        assert probs is None
    bf._assert_same_state(A, B, starts, [n] * nm, tag)
    for k in range(nm):
        assert B[k]._input_ids[starts[k]:starts[k] + n].tolist() == rows[k], (tag, "_input_ids of k", k)
    return starts, rows


def _next_step_agrees(A, B, ids, starts, tag):
    """the next batch step of both families: equal tokens, so the draw counters and penalty windows agree"""
    from realtime_codec_agent_amd.llm import LlamaBatch
    for k in range(len(A)):
        if A[k].n_tokens + 1 > A[k].n_ctx():
            A[k].n_tokens = B[k].n_tokens = starts[k]
    nxt = [[ids[(40 + k) % len(ids)]] for k in range(len(A))]
    ba, bn = LlamaBatch(A), LlamaBatch(B)
    try:
        assert ba.step(nxt) == bn.step(nxt), (tag, "next step")
    finally:
        ba.close()
        bn.close()


def _run(name, fmt, sel, n, n_probe, tag, **kw):
    ids = bg._ids(name)
    Bfull = bg._family(name, fmt, WHICH_B, FAMILY)
    A, B = bg._family(name, fmt)[:len(sel)], [Bfull[s] for s in sel]
    try:
        starts, _ = _step_sel_against_own_batch(A, B, bs._batch64(name, fmt), sel, ids, bg.MODELS[name].vocab, n, n_probe, tag, **kw)
        _next_step_agrees(A, B, ids, starts, tag)
    finally:
        bf._graphs_back_on(B)
    return A, B, starts


# ---------------------------------------------------------------------------------------------- 1. selected members
@pytest.mark.parametrize("n_probe", (0, 1, 2, 8))
@pytest.mark.parametrize("n", (1, 2))
@pytest.mark.parametrize("which", list(SELECTIONS))
@pytest.mark.parametrize("name,fmt", bf.CASES, ids=bf.CASE_IDS)
def test_a_selected_member_ends_as_in_a_batch_step_of_the_selected_members(name, fmt, which, n, n_probe):
    _run(name, fmt, SELECTIONS[which], n, n_probe, (name, fmt, which, n, n_probe))


@functools.lru_cache(maxsize=None)
def _q8kv_family(which):
    from realtime_codec_agent_amd.llm import LlamaForAlternatingCodeChannels as L
    c = bg.G4
    parent = L(model_path=f"random:{c.name}", config=c.config(), n_ctx=c.n_ctx, random_seed=c.seed, init_std=sc.INIT_STD, device=0, weight_format="bf16",
               kv_format="q8_0")
    assert parent.kv_format == "q8_0" and parent.prefill_route() == "gemm128"
    return [parent] + [L(n_ctx=c.n_ctx, share_weights_with=parent, device=0) for _ in range(11)]


@pytest.mark.parametrize("n", (1, 2))
def test_over_the_q8_0_kv_cache(n):
    """a batch of 12 over q8_0 caches, 9 selected unsorted: the raw int8 blocks and scales of the new rows too"""
    from realtime_codec_agent_amd.llm import LlamaBatch
    c = bg.G4
    ids = c.ids().tolist()
    sel = [7, 2, 11, 0, 4, 9, 1, 10, 5]
    famA, famB = _q8kv_family(0), _q8kv_family(1)
    A, B = famA[:len(sel)], [famB[s] for s in sel]
    bb = LlamaBatch(famB)
    try:
        starts, _ = _step_sel_against_own_batch(A, B, bb, sel, ids, c.vocab, n, 2, ("q8_0 KV", n))
        for k, (a, b) in enumerate(zip(A, B)):
            for layer in range(c.config().n_layers):
                for x, y in zip(a.kv_read_q8(layer, starts[k], n), b.kv_read_q8(layer, starts[k], n)):
                    assert np.array_equal(x, y), ("q8_0 blocks of k", k, "layer", layer)
        _next_step_agrees(A, B, ids, starts, "q8_0 KV")
    finally:
        bb.close()


@pytest.mark.parametrize("name,fmt", (("g4_k768", "bf16"), ("g4_k768", "q4_k")), ids=("g4-bf16", "g4-q4_k"))
def test_a_selection_of_one_equals_the_member_inside_a_selection_of_two(name, fmt):
    """family B runs members=[37] alone, family A's batch of 64 runs members=[37, 5]"""
    from realtime_codec_agent_amd.llm import LlamaBatch
    ids = bg._ids(name)
    n, start = 2, 255
    a, a2 = bg._family(name, fmt)[37], bg._family(name, fmt)[5]
    b = bg._family(name, fmt, WHICH_B, FAMILY)[37]
    bg._prepare([a, a2, b], ids, [start, 300, start], samplers=(SERIAL[1],))
    rows = bg._rows(ids, 2, n, 0)
    ba = LlamaBatch(bg._family(name, fmt)[:NB])
    try:
        want, wp = ba.step_probe([37, 5], rows, [[7, 9, 11], [1, 2, 3]])
        got, gp = bs._batch64(name, fmt).step_probe([37], rows[:1], [[7, 9, 11]])
    finally:
        ba.close()
    assert got[0] == want[0] and gp[0].tobytes() == wp[0].tobytes()
    bf._assert_same_state([a], [b], [start], [n], "selection of one")
    assert a.sample() == b.sample()


# ---------------------------------------------------------------------------------------------- 2. roll-back
@pytest.mark.parametrize("n", (1, 2))
def test_after_the_roll_back_a_selection_frame_gives_the_plain_batch_frames_bits(n):
    """the agent's use: the speculative step, n_tokens -= n, and the next frame overwrites the speculative rows"""
    from realtime_codec_agent_amd.llm import LlamaBatch
    name, fmt, n_steps = "g4_k768", "bf16", 3
    ids = bg._ids(name)
    sel = SELECTIONS["9"]
    Bfull = bg._family(name, fmt, WHICH_B, FAMILY)
    A, B = bg._family(name, fmt)[:len(sel)], [Bfull[s] for s in sel]
    starts = [0, 250, 254, 255, 256, 511, 300, 1, bg.MODELS[name].n_ctx - 2 * n_steps]
    starts, _ = _step_sel_against_own_batch(A, B, bs._batch64(name, fmt), sel, ids, bg.MODELS[name].vocab, n, 2, ("roll-back", n), starts=starts)
    for m in A + B:
        m.n_tokens -= n
    pairs, users = bf._inputs(ids, len(sel), n_steps)
    ba = LlamaBatch(A)
    try:
        want, wp = ba.frame(pairs, users, -1, probe_ids=[5] * len(sel))
    finally:
        ba.close()
    got, gp = bs._batch64(name, fmt).frame(pairs, users, -1, probe_ids=[5] * len(sel), members=sel)
    assert got == want and gp.tobytes() == wp.tobytes()
    bf._assert_same_state(A, B, starts, [2 * n_steps] * len(sel), ("roll-back", n))


# ---------------------------------------------------------------------------------------------- 3. unselected members
@pytest.mark.parametrize("which,n", (("9", 1), ("unsorted", 2)))
def test_an_unselected_member_is_not_touched(which, n):
    """All 64 members of both families prepared alike; B runs a selection step, A nothing.  Every unselected member of B keeps every
    byte of its caches, its n_tokens and logits, and draws next what its untouched counterpart of A draws.  Member 50 sits at
    n_tokens == n_ctx, and slot 51 holds a bare twin that never got a sampler: neither is a reason to refuse."""
    from realtime_codec_agent_amd.llm import LlamaForAlternatingCodeChannels as L, LlamaBatch
    name, fmt = "g4_k768", "bf16"
    c = bg.MODELS[name]
    ids = bg._ids(name)
    sel = SELECTIONS[which]
    A, Bfam = bg._family(name, fmt)[:NB], bg._family(name, fmt, WHICH_B, FAMILY)
    pool = (1, 250, 511, 254, 255, 256, 300, 512, 700)
    starts = [pool[s % len(pool)] for s in range(NB)]
    bare = L(n_ctx=c.n_ctx, share_weights_with=Bfam[0], device=0)
    B = Bfam[:51] + [bare] + Bfam[52:NB]
    bb = None
    try:
        bg._prepare(A, ids, starts, samplers=SERIAL)
        bg._prepare(Bfam[:NB], ids, starts, samplers=SERIAL)
        bare.eval(ids[:starts[51]])
        A[50].n_tokens = B[50].n_tokens = c.n_ctx              # a full cache: any step of this member would be refused
        assert 50 not in sel and 51 not in sel
        bb = LlamaBatch(B)
        rest = [s for s in range(NB) if s not in sel]
        snaps = {s: bs._snapshot(B[s]) for s in rest}
        got, probs = bb.step_probe(sel, bg._rows(ids, len(sel), n, 0), _probes(c.vocab, len(sel), 2))
        assert len(got) == len(sel) and np.all((probs > 0.0) & (probs < 1.0))
        for k, s in enumerate(sel):
            assert B[s].n_tokens == starts[s] + n, ("selected", k, s)
        for s in rest:
            bs._assert_snapshot(B[s], snaps[s], ("unselected member", s))
        A[50].n_tokens = B[50].n_tokens = starts[50]
        for s in rest:
            if s != 51:
                assert A[s].sample() == B[s].sample(), ("next draw of unselected member", s)
    finally:
        if bb is not None:
            bb.close()
        bare.close()


# ---------------------------------------------------------------------------------------------- 4. eager, whole vocabulary, consecutive calls
@pytest.mark.parametrize("name,fmt", (("g4_k768", "bf16"), ("g4_k768", "q4_k")), ids=("g4-bf16", "g4-q4_k"))
def test_an_eager_selection_step_gives_the_replayed_steps_bits(name, fmt):
    """graphs off on family B's selected members against the replayed step of family A's batch (test 1 holds the replayed selection
    step to the same reference)"""
    _run(name, fmt, SELECTIONS["9"], 2, 2, (name, fmt, "eager"), graphs_b=False)


def test_a_selection_with_a_whole_vocabulary_sampler():
    """every fourth member of the selection samples over the whole vocabulary (its own launches behind the table chain): eager, same bits"""
    _run("g4_k768", "bf16", SELECTIONS["9"], 1, 2, "whole vocabulary", samplers=bg.SAMPLERS)


def test_three_consecutive_calls_with_other_selections():
    """calls over {0..4}, {1, 3} and all members of a batch of 9 with other n and probe counts: the block of a call leaves nothing for the next"""
    from realtime_codec_agent_amd.llm import LlamaBatch
    name, fmt, nm = "g4_k768", "q8_0", 9
    ids = bg._ids(name)
    A, B = bg._family(name, fmt)[:nm], bg._family(name, fmt, WHICH_B, FAMILY)[:nm]
    starts = [0, 250, 511, 300, 254, 1, 255, 256, 512]
    bg._prepare(A, ids, starts, samplers=SERIAL)
    bg._prepare(B, ids, starts, samplers=SERIAL)
    bb = LlamaBatch(B)
    try:
        for call, (sel, n, n_probe) in enumerate((([0, 1, 2, 3, 4], 2, 8), ([1, 3], 1, 1), (list(range(nm)), 2, 2))):
            now = [A[s].n_tokens for s in sel]
            _step_sel_against_own_batch([A[s] for s in sel], [B[s] for s in sel], bb, sel, ids, bg.MODELS[name].vocab, n, n_probe, ("call", call),
                                        salt=call, prepare=False, starts=now)
        _next_step_agrees(A, B, ids, starts, "three calls")
    finally:
        bb.close()


# ---------------------------------------------------------------------------------------------- 6. captures
def test_selections_of_one_class_share_one_capture_and_the_frames_keep_their_graphs():
    from realtime_codec_agent_amd.llm import LlamaBatch
    name, fmt, nm = "g4_k768", "bf16", 17
    ids = bg._ids(name)
    vocab = bg.MODELS[name].vocab
    famA, famB = bg._family(name, fmt), bg._family(name, fmt, WHICH_B, FAMILY)
    A, B = famA[:nm], famB[:nm]
    shadows = (famA[FAMILY - 1], famB[FAMILY - 1])
    starts = [(3 + 29 * s) % 500 for s in range(nm)]
    bg._prepare(A, ids, starts, samplers=SERIAL)
    bg._prepare(B, ids, starts, samplers=SERIAL)
    bb = LlamaBatch(famB[:NB])

    def call(n, salt, n_probe=2):
        now = [A[s].n_tokens for s in range(n)]
        _step_sel_against_own_batch(A[:n], B[:n], bb, list(range(n)), ids, vocab, 1, n_probe, ("selection of", n), salt=salt, prepare=False, starts=now)

    def frame(n, salt):
        pairs, users = bf._inputs(ids, n, 2, salt=salt)
        ba = LlamaBatch(A[:n])
        try:
            want, _ = ba.frame(pairs, users, -1, probe_ids=[5] * n)
        finally:
            ba.close()
        got, _ = bb.frame(pairs, users, -1, probe_ids=[5] * n, members=list(range(n)))
        assert got == want

    try:
        frame(9, 0)
        c0 = bb.captures()
        call(9, 0)
        assert bb.captures() == c0 + 1
        call(12, 1, n_probe=8)
        call(16, 2, n_probe=1)
        assert bb.captures() == c0 + 1, "selections of 9, 12 and 16 members with 2, 8 and 1 probe ids are one capture: the ids travel in the block"
        frame(12, 1)
        assert bb.captures() == c0 + 1, "the selection frame replays its own graph"
        for fam, shadow in zip((A, B), shadows):       # the shadow-cache trim of member 2: its cache now lives in other memory, the same bits in it
            shadow.reset()
            shadow.copy_kv_from(fam[2], fam[2].n_tokens)
            fam[2].swap_kv(shadow)
        call(12, 3)
        assert bb.captures() == c0 + 1, "a graph holds no member's cache pointer: rca_lm_swap_kv of a member re-captures nothing"
        call(17, 4)
        assert bb.captures() == c0 + 2, "17 members are the next class"
        call(9, 5, n_probe=0)
        assert bb.captures() == c0 + 3, "without probes: another launch sequence"
        call(9, 6)
        frame(9, 2)
        assert bb.captures() == c0 + 3
    finally:
        bb.close()


def test_a_duplex_batch_frame_before_and_after_replays_its_own_graph():
    """the agents' driver: ticks of a duplex batch frame with a batched speculative step between them make no capture after the first
    of each kind (tests/test_agent_batch_speaker_gpu.py compares the sessions)"""
    import test_agent_batch_gpu as ag
    from realtime_codec_agent_amd import RealtimeAgentBatch
    agents, _ = ag._make()
    drv = RealtimeAgentBatch(agents, min_batch=1, batch_speaker_step=True)
    try:
        seen = []
        for t in range(ag.TICKS):
            drv.process_audio([ag._chunk(s, t) for s in range(ag.N_AGENTS)])
            seen.append((drv._batch.captures(), drv.fused_frames, drv.fused_speaker_calls))
        both = [i for i in range(1, len(seen)) if seen[i][1] > seen[i - 1][1] and seen[i][2] > seen[i - 1][2]]     # ticks with both calls
        assert len(both) >= 12, seen
        # the selection step captures on its first call; the duplex batch frame runs its first call of a shape eagerly and captures on
        # its second, which the second tick with both calls has seen at the latest.  Five agents are one class, their contexts one bucket.
        settled = both[1]
        assert seen[-1][0] == seen[settled][0], ("a capture after both graphs existed", seen)
        assert len([i for i in both if i > settled]) >= 10
    finally:
        drv.close()


# ---------------------------------------------------------------------------------------------- 7. refusals
def test_refusals_leave_every_member_unchanged():
    from realtime_codec_agent_amd import _native as N
    from realtime_codec_agent_amd.llm import LlamaForAlternatingCodeChannels as L, LlamaBatch
    import ctypes as C
    name, fmt, nm = "g4_k768", "bf16", 5
    c = bg.MODELS[name]
    ids = bg._ids(name)
    A, B = bg._family(name, fmt)[:nm], bg._family(name, fmt, WHICH_B, FAMILY)[:nm]
    starts = [30, 40, 254, 300, 511]
    bg._prepare(A, ids, starts, samplers=SERIAL)
    bg._prepare(B, ids, starts, samplers=SERIAL)
    ba, bb = LlamaBatch(A), LlamaBatch(B)
    rows = bg._rows(ids, nm, 1, 0)
    I32 = C.c_int32

    def unchanged(snap, tag):
        for s, (m, (nt, lg)) in enumerate(zip(B, snap)):
            assert m.n_tokens == nt, (tag, s)
            assert np.array_equal(m._scores[-1], lg), (tag, s)

    def raw(sel, n_sel, n=1, n_probe=2, toks=None, pids=True, probs=True, tokens=True, b=True, sel_null=False, ids_null=False):
        sl = (I32 * max(len(sel), 1))(*sel)
        flat = toks if toks is not None else [1] * (nm * 2)
        arr = (I32 * len(flat))(*flat)
        pid = (I32 * (nm * 8))(*([3] * (nm * 8))) if pids is True else ((I32 * len(pids))(*pids) if pids else None)
        out, pp = (I32 * nm)(), (C.c_float * (nm * 8))()
        N.check(bb._lib.rca_lm_batch_step_sel(bb._b if b else None, None if sel_null else sl, n_sel, None if ids_null else arr, n, pid, n_probe,
                                              out if tokens else None, pp if probs else None), "rca_lm_batch_step_sel")

    try:
        assert ba.step(rows) == bb.step_probe(list(range(nm)), rows)[0]
        snap = [(m.n_tokens, m._scores[-1].copy()) for m in B]
        for kw in (dict(b=False), dict(sel_null=True), dict(ids_null=True), dict(tokens=False)):
            with pytest.raises(N.RcaError, match=r"batch_step_sel: null argument"):
                raw([0, 1], 2, **kw)
        for n in (0, 3):
            with pytest.raises(N.RcaError, match=r"batch_step_sel: %d tokens per member \(1\.\.2\)" % n):
                raw([0, 1], 2, n=n)
        for n_probe in (-1, 9):
            with pytest.raises(N.RcaError, match=r"batch_step_sel: %d probe ids per member \(0\.\.8\)" % n_probe):
                raw([0, 1], 2, n_probe=n_probe)
        with pytest.raises(N.RcaError, match=r"probe_ids is null exactly when n_probe is 0"):
            raw([0, 1], 2, pids=None)
        with pytest.raises(N.RcaError, match=r"probe_ids is null exactly when n_probe is 0"):
            raw([0, 1], 2, n_probe=0)
        with pytest.raises(N.RcaError, match=r"probe_ids without probs"):
            raw([0, 1], 2, probs=False)
        unchanged(snap, "arguments")
        with pytest.raises(N.RcaError, match=r"sel\[1\] = member 5 is outside the batch's members \[0, 5\)"):
            raw([0, 5, 1], 3)
        with pytest.raises(N.RcaError, match=r"sel\[0\] = member -1 is outside"):
            raw([-1, 2], 2)
        with pytest.raises(N.RcaError, match=r"sel\[2\] = member 3 is selected twice \(also sel\[0\]\)"):
            raw([3, 1, 3], 3)
        with pytest.raises(N.RcaError, match=r"batch_step_sel: 0 selected members"):
            raw([], 0)
        with pytest.raises(N.RcaError, match=r"batch_step_sel: 6 selected members, the batch has 5"):
            raw([0, 1, 2, 3, 4, 0], 6)
        with pytest.raises(N.RcaError):
            bb.step_probe([], [])
        with pytest.raises(N.RcaError):
            bb.step_probe([0, 5], rows[:2])
        with pytest.raises(ValueError):
            bb.step_probe([0, 1], [[1], [1, 2]])
        with pytest.raises(ValueError):
            bb.step_probe([0, 1], rows[:2], [[1], [1, 2]])
        with pytest.raises(ValueError):
            bb.step_probe([0, 1], rows[:2], [[1]])
        unchanged(snap, "selection")
        with pytest.raises(N.RcaError, match=r"token id %d of sel\[1\] = member 0 at index 1 is outside the vocabulary" % c.vocab):
            bb.step_probe([2, 0], [[1, 2], [3, c.vocab]])
        with pytest.raises(N.RcaError, match=r"token id -1 of sel\[0\] = member 2 at index 0"):
            bb.step_probe([2, 0], [[-1], [3]])
        with pytest.raises(N.RcaError, match=r"probe id %d of sel\[1\] = member 4 at index 2 is outside the vocabulary" % c.vocab):
            bb.step_probe([1, 4], rows[:2], [[1, 2, 3], [4, 5, c.vocab]])
        with pytest.raises(N.RcaError, match=r"probe id -1 of sel\[0\] = member 1 at index 0"):
            bb.step_probe([1, 4], rows[:2], [[-1], [4]])
        unchanged(snap, "ids")
        # a selected member a token short of the step's n; unselected, the same member is no reason to refuse
        keep = B[3].n_tokens
        A[3].n_tokens = B[3].n_tokens = c.n_ctx - 1
        with pytest.raises(N.RcaError, match=r"context overflow of sel\[1\] = member 3: %d \+ 2 > n_ctx %d" % (c.n_ctx - 1, c.n_ctx)):
            bb.step_probe([4, 3], [[1, 2], [3, 4]])
        assert B[3].n_tokens == c.n_ctx - 1
        A[3].n_tokens = B[3].n_tokens = keep
        unchanged(snap, "context overflow")
        # a member without a sampler, and one in another KV format than member 0
        twins = [L(n_ctx=c.n_ctx, share_weights_with=B[0], device=0) for _ in range(4)]
        bt = LlamaBatch(B[:2] + twins)
        try:
            twins[0].eval(ids[:20])
            with pytest.raises(N.RcaError, match=r"sel\[1\] = member 2 has no sampler"):
                bt.step_probe([0, 2], rows[:2])
            twins[1].set_kv_format("q8_0")
            twins[1].init_sampler_for_generate(**bg.GREEDY)
            with pytest.raises(N.RcaError, match=r"sel\[0\] = member 3 has KV format"):
                bt.step_probe([3, 1], rows[:2])
            # a member switched to logits_all, and one taken off the 128-token tile route, since the batch was made
            twins[2].init_sampler_for_generate(**bg.GREEDY)
            N.check(twins[2]._lib.rca_lm_set_logits_all(twins[2]._h, 1), "rca_lm_set_logits_all")
            with pytest.raises(N.RcaError, match=r"sel\[1\] = member 4 was switched to logits_all"):
                bt.step_probe([0, 4], rows[:2])
            twins[3].init_sampler_for_generate(**bg.GREEDY)
            twins[3].set_mfma_prefill(False)
            with pytest.raises(N.RcaError, match=r"sel\[0\] = member 5 no longer takes the 128-token tiles"):
                bt.step_probe([5, 1], rows[:2])
        finally:
            bt.close()
            for t in twins:
                t.close()
        unchanged(snap, "sampler / KV format")
        # the next step of every member is what the family that saw no refusal gets
        nxt = bg._rows(ids, nm, 2, 1)
        assert ba.step(nxt) == bb.step_probe(list(range(nm)), nxt)[0]
        bf._assert_same_state(A, B, [nt for nt, _ in snap], [2] * nm, "after the refusals")
    finally:
        ba.close()
        bb.close()
