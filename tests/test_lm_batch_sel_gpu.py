"""rca_lm_batch_frame_sel / LlamaBatch.frame(members=...): a batch frame over a SUBSET of the members, and rca_lm_batch_captures.

The contract is bit for bit.  Family B is ONE batch over 64 members and runs frame(members=sel); family A (its own weights, the same
values) runs LlamaBatch(only those members).frame(...).  Checked here:
  1. selected members: tokens, logits, n_tokens, the K / V bits of every layer at the new positions and the next step's tokens, for
     selections of 2, 5, 8, 9, 33 and 64 members, an unsorted one and one with the member of slot 63; 1, 3 and 8 steps; starts 0, 250
     (crosses the 256-key split inside the frame), 511 and n_ctx - 2 * n_steps; a selection of 1 against the same member in one of 2;
  2. unselected members: EVERY row of the K / V cache of every layer (all n_ctx rows), n_tokens, the logits and the next draw, one of
     them with a full cache and one without a sampler;
  3. cut members and probes inside a selection; graphs on == off; a selection with a whole-vocabulary sampler; three consecutive ticks
     with other selections;
  4. captures: selections of 9, 12 and 16 members share one capture, also after a member's swap_kv; 17 members take one more;
  5. refusals leave every member unchanged.
All comparisons are np.array_equal.  The models, samplers and helpers are those of tests/test_lm_batch_gpu.py and
tests/test_lm_batch_frame_gpu.py (imported, so the files share one family cache).

Every test here fails on a library without rca_lm_batch_frame_sel (the parent commit: LlamaBatch.frame has no members= and the symbol
is missing)."""
import functools

import numpy as np
import pytest

import test_lm_batch_frame_gpu as bf
import test_lm_batch_gpu as bg

pytestmark = pytest.mark.gpu

FAMILY = bg.FAMILY
WHICH_B = bf.WHICH_B
SERIAL = bg.SAMPLERS[:3]          # the table sampler chain only: such a selection replays a graph
NB = 64
SELECTIONS = {
    "2": [3, 40],
    "5": [1, 9, 17, 30, 44],
    "8": list(range(8, 16)),
    "9": list(range(0, 45, 5)),
    "33": list(range(30, 63)),
    "64": list(range(64)),
    "unsorted": [20, 3, 41, 7, 12, 2],
    "slot63": [63, 0, 31],
}


@functools.lru_cache(maxsize=None)
def _batch64(name, fmt):
    """family B's one batch over 64 members, kept for the session: its graphs serve every test of the (model, format)"""
    from realtime_codec_agent_amd.llm import LlamaBatch
    return LlamaBatch(bg._family(name, fmt, WHICH_B, FAMILY)[:NB])


def _starts(n_ctx, n, n_steps):
    last = n_ctx - 2 * n_steps
    pool = (0, 250, 511, last, 1, 254, 255, 256, 300, 512)
    return [pool[k % len(pool)] for k in range(n)]


def _sel_against_own_batch(name, fmt, sel, n_steps, tag, graphs_b=True, samplers=SERIAL, floor=-1, probe_ids=None):
    """frame(members=sel) of the 64-member batch against frame() of a batch over family A's first len(sel) members; returns
    (tokens, probs of B, A, B's selected members, starts)"""
    from realtime_codec_agent_amd.llm import LlamaBatch
    ids = bg._ids(name)
    Bfull = bg._family(name, fmt, WHICH_B, FAMILY)
    A, B = bg._family(name, fmt)[:len(sel)], [Bfull[s] for s in sel]
    starts = _starts(bg.MODELS[name].n_ctx, len(sel), n_steps)
    bg._prepare(A, ids, starts, samplers=samplers)
    bg._prepare(B, ids, starts, graphs=graphs_b, samplers=samplers)
    pairs, users = bf._inputs(ids, len(sel), n_steps)
    ba, bb, bn = LlamaBatch(A), _batch64(name, fmt), LlamaBatch(B)
    try:
        want, wprobs = ba.frame(pairs, users, floor, probe_ids=probe_ids)
        got, probs = bb.frame(pairs, users, floor, probe_ids=probe_ids, members=sel)
        assert got == want, (tag, "tokens")
        if probe_ids is not None:
            assert probs.tobytes() == wprobs.tobytes(), (tag, "probes", probs, wprobs)
        done = [len(t) for t in want]
        complete = [k for k in range(len(sel)) if done[k] == n_steps]
        for k in range(len(sel)):
            assert A[k].n_tokens == B[k].n_tokens == starts[k] + 2 * done[k], (tag, "n_tokens of k", k)
            assert len(B[k]._scores) == len(A[k]._scores) == (1 if k in complete else 0), (tag, "logits rows of k", k)
            if k in complete:
                assert np.array_equal(A[k]._scores[-1], B[k]._scores[-1]), (tag, "logits of k", k)
            for layer, ((ka, va), (kb, vb)) in enumerate(zip(bf._kv_all(A[k], starts[k], 2 * done[k]), bf._kv_all(B[k], starts[k], 2 * done[k]))):
                assert ka.any() and va.any()
                assert np.array_equal(ka, kb) and np.array_equal(va, vb), (tag, "K / V of k", k, "layer", layer)
        # the next step of every member: equal tokens, so the draw counters (and penalty windows) agree
        for k in range(len(sel)):
            if A[k].n_tokens + 1 > A[k].n_ctx():
                A[k].n_tokens = B[k].n_tokens = starts[k]
        nxt = [[ids[(40 + k) % len(ids)]] for k in range(len(sel))]
        assert ba.step(nxt) == bn.step(nxt), (tag, "next step")
    finally:
        ba.close()
        bn.close()
        bf._graphs_back_on(B)
    return want, probs, A, B, starts


# ---------------------------------------------------------------------------------------------- 1. selected members
@pytest.mark.parametrize("n_steps", (1, 3, 8))
@pytest.mark.parametrize("which", list(SELECTIONS))
@pytest.mark.parametrize("name,fmt", bf.CASES, ids=bf.CASE_IDS)
def test_a_selected_member_ends_as_in_a_batch_of_the_selected_members(name, fmt, which, n_steps):
    _sel_against_own_batch(name, fmt, SELECTIONS[which], n_steps, (name, fmt, which, n_steps))


@pytest.mark.parametrize("name,fmt", (("g4_k768", "bf16"), ("g4_k768", "q4_k")), ids=("g4-bf16", "g4-q4_k"))
def test_a_selection_of_one_equals_the_member_inside_a_selection_of_two(name, fmt):
    """family B runs members=[37] alone, family A's batch of 64 runs members=[37, 5]"""
    from realtime_codec_agent_amd.llm import LlamaBatch
    ids = bg._ids(name)
    n_steps, start = 4, 250
    a, a2 = bg._family(name, fmt)[37], bg._family(name, fmt)[5]
    b = bg._family(name, fmt, WHICH_B, FAMILY)[37]
    bg._prepare([a, a2, b], ids, [start, 300, start], samplers=(SERIAL[1],))
    pairs, users = bf._inputs(ids, 2, n_steps)
    ba = LlamaBatch(bg._family(name, fmt)[:NB])
    try:
        want, wp = ba.frame(pairs, users, -1, probe_ids=[7, 9], members=[37, 5])
        got, gp = _batch64(name, fmt).frame(pairs[:1], users[:1], -1, probe_ids=[7], members=[37])
    finally:
        ba.close()
    assert got[0] == want[0] and gp[0].tobytes() == wp[0].tobytes()
    bf._assert_same_state([a], [b], [start], [2 * n_steps], "selection of one")
    assert a.sample() == b.sample()


# ---------------------------------------------------------------------------------------------- 2. unselected members
def _snapshot(m, logits=True):
    n_layers = m.config.n_layers
    kv = [bg._kv_bits(m, layer, 0, m.n_ctx()) for layer in range(n_layers)]
    return m.n_tokens, (m._scores.copy() if logits else None), kv


def _assert_snapshot(m, snap, tag):
    nt, lg, kv = snap
    assert m.n_tokens == nt, (tag, "n_tokens")
    if lg is not None:
        assert np.array_equal(m._scores, lg), (tag, "logits")
    for layer, (k0, v0) in enumerate(kv):
        k1, v1 = bg._kv_bits(m, layer, 0, m.n_ctx())
        assert np.array_equal(k0, k1) and np.array_equal(v0, v1), (tag, "K / V cache, layer", layer)


@pytest.mark.parametrize("which", ("9", "unsorted"))
def test_an_unselected_member_is_not_touched(which):
    """All 64 members of both families prepared alike; B runs a selection frame, A nothing.  Every unselected member of B keeps every
    byte of its caches, its n_tokens and logits, and draws next what its untouched counterpart of A draws.  Member 50 sits at
    n_tokens == n_ctx, and slot 51 holds a bare twin that never got a sampler: neither is a reason to refuse."""
    from realtime_codec_agent_amd.llm import LlamaForAlternatingCodeChannels as L, LlamaBatch
    name, fmt, n_steps = "g4_k768", "bf16", 4
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
        A[50].n_tokens = B[50].n_tokens = c.n_ctx              # a full cache: any frame of this member would be refused
        assert 50 not in sel and 51 not in sel
        bb = LlamaBatch(B)
        rest = [s for s in range(NB) if s not in sel]
        snaps = {s: _snapshot(B[s]) for s in rest}
        pairs, users = bf._inputs(ids, len(sel), n_steps)
        got, _ = bb.frame(pairs, users, -1, members=sel)
        assert all(len(t) == n_steps for t in got)
        for k, s in enumerate(sel):
            assert B[s].n_tokens == starts[s] + 2 * n_steps, ("selected", k, s)
        for s in rest:
            _assert_snapshot(B[s], snaps[s], ("unselected member", s))
        A[50].n_tokens = B[50].n_tokens = starts[50]
        for s in rest:
            if s != 51:
                assert A[s].sample() == B[s].sample(), ("next draw of unselected member", s)
    finally:
        if bb is not None:
            bb.close()
        bare.close()


# ---------------------------------------------------------------------------------------------- 3. cuts, probes, eager, whole vocabulary, ticks
def test_cut_members_and_probes_inside_a_selection():
    """The floor comes from the reference's own uncut tokens (as in the batch-frame tests): members cut early, cut at the last step
    and not cut; probes NaN on the cut members and where the probe id is -1, otherwise token_probs' bits (the reference's)."""
    name, fmt, n_steps = "g4_k768", "q8_0", 4
    sel = SELECTIONS["9"]
    full, _, _, _, _ = _sel_against_own_batch(name, fmt, sel, n_steps, "uncut")
    floor = bf._floor_from(full)
    assert floor is not None, full
    early, at_last, uncut = bf._kinds(full, floor)
    complete = at_last + uncut
    probe = [-1 if k == complete[0] else (5 + 100 * k) % bg.MODELS[name].vocab for k in range(len(sel))]
    got, probs, A, B, starts = _sel_against_own_batch(name, fmt, sel, n_steps, "cut", floor=floor, probe_ids=probe)
    assert got == [t[:bf._n_done(t, floor)] for t in full]
    for k in range(len(sel)):
        if k in early or probe[k] < 0:
            assert np.isnan(probs[k]), k
        else:
            assert 0.0 < probs[k] < 1.0, (k, probs[k])
    assert early and np.isnan(probs[early[0]]) and np.isnan(probs[complete[0]])


@pytest.mark.parametrize("name,fmt", (("g4_k768", "bf16"), ("g4_k768", "q4_k")), ids=("g4-bf16", "g4-q4_k"))
def test_an_eager_selection_frame_gives_the_replayed_frames_bits(name, fmt):
    """graphs off on family B's selected members against the replayed frame of family A's batch (test 1 holds the replayed selection
    frame to the same reference)"""
    _sel_against_own_batch(name, fmt, SELECTIONS["9"], 4, (name, fmt, "eager"), graphs_b=False)


def test_a_selection_with_a_whole_vocabulary_sampler():
    """every fourth member of the selection samples over the whole vocabulary (its own launches behind the table chain): eager, same bits"""
    _sel_against_own_batch("g4_k768", "bf16", SELECTIONS["9"], 3, "whole vocabulary", samplers=bg.SAMPLERS)


def test_three_consecutive_ticks_with_other_selections():
    """ticks over {0..4}, {1, 3} and all members of a batch of 9: the reference is driven tick by tick with a batch per selection"""
    from realtime_codec_agent_amd.llm import LlamaBatch
    name, fmt, nm, n_steps = "g4_k768", "q8_0", 9, 3
    ids = bg._ids(name)
    A, B = bg._family(name, fmt)[:nm], bg._family(name, fmt, WHICH_B, FAMILY)[:nm]
    starts = [0, 250, 511, 300, 254, 1, 255, 256, 512]
    bg._prepare(A, ids, starts, samplers=SERIAL)
    bg._prepare(B, ids, starts, samplers=SERIAL)
    bb = LlamaBatch(B)
    grown = [0] * nm
    try:
        for tick, sel in enumerate(([0, 1, 2, 3, 4], [1, 3], list(range(nm)))):
            pairs, users = bf._inputs(ids, len(sel), n_steps, salt=tick)
            ba = LlamaBatch([A[s] for s in sel])
            try:
                want, _ = ba.frame(pairs, users, -1)
            finally:
                ba.close()
            got, _ = bb.frame(pairs, users, -1, members=sel)
            assert got == want, ("tick", tick)
            for s in sel:
                grown[s] += 2 * n_steps
        bf._assert_same_state(A, B, starts, grown, "three ticks")
        nxt = bg._rows(ids, nm, 1, 3)
        ba = LlamaBatch(A)
        try:
            assert ba.step(nxt) == bb.step(nxt)
        finally:
            ba.close()
    finally:
        bb.close()


# ---------------------------------------------------------------------------------------------- 4. captures
def test_selections_of_one_class_share_one_capture_also_after_a_swap_kv():
    from realtime_codec_agent_amd.llm import LlamaBatch
    name, fmt, n_steps, nm = "g4_k768", "bf16", 2, 17
    ids = bg._ids(name)
    famA, famB = bg._family(name, fmt), bg._family(name, fmt, WHICH_B, FAMILY)
    A, B = famA[:nm], famB[:nm]
    shadows = (famA[FAMILY - 1], famB[FAMILY - 1])
    starts = [(3 + 29 * s) % 500 for s in range(nm)]
    bg._prepare(A, ids, starts, samplers=SERIAL)
    bg._prepare(B, ids, starts, samplers=SERIAL)
    bb = LlamaBatch(famB[:NB])
    grown = [0] * nm

    def tick(n, salt):
        pairs, users = bf._inputs(ids, n, n_steps, salt=salt)
        ba = LlamaBatch(A[:n])
        try:
            want, wp = ba.frame(pairs, users, -1, probe_ids=[5] * n)
        finally:
            ba.close()
        got, gp = bb.frame(pairs, users, -1, probe_ids=[5] * n, members=list(range(n)))
        assert got == want and gp.tobytes() == wp.tobytes(), ("selection of", n)
        for s in range(n):
            grown[s] += 2 * n_steps

    try:
        c0 = bb.captures()
        tick(9, 0)
        assert bb.captures() == c0 + 1
        tick(12, 1)
        tick(16, 2)
        assert bb.captures() == c0 + 1, "selections of 9, 12 and 16 members are one geometry class: one capture"
        # the shadow-cache trim of member 2: its cache now lives in other memory, the same bits in it
        for fam, shadow in zip((A, B), shadows):
            shadow.reset()
            shadow.copy_kv_from(fam[2], fam[2].n_tokens)
            fam[2].swap_kv(shadow)
        tick(12, 3)
        assert bb.captures() == c0 + 1, "a graph holds no member's cache pointer: rca_lm_swap_kv of a member re-captures nothing"
        tick(17, 4)
        assert bb.captures() == c0 + 2, "17 members are the next class"
        tick(9, 5)
        assert bb.captures() == c0 + 2
        bf._assert_same_state(A, B, starts, grown, "captures")
    finally:
        bb.close()


# ---------------------------------------------------------------------------------------------- 5. refusals
def test_refusals_leave_every_member_unchanged():
    from realtime_codec_agent_amd import _native as N
    from realtime_codec_agent_amd.llm import LlamaBatch
    import ctypes as C
    name, fmt, nm, n_steps = "g4_k768", "bf16", 5, 4
    c = bg.MODELS[name]
    ids = bg._ids(name)
    A, B = bg._family(name, fmt)[:nm], bg._family(name, fmt, WHICH_B, FAMILY)[:nm]
    starts = [30, 40, 254, 300, 511]
    bg._prepare(A, ids, starts, samplers=SERIAL)
    bg._prepare(B, ids, starts, samplers=SERIAL)
    ba, bb = LlamaBatch(A), LlamaBatch(B)
    pairs, users = bf._inputs(ids, nm, n_steps)

    def unchanged(snap, tag):
        for s, (m, (nt, lg)) in enumerate(zip(B, snap)):
            assert m.n_tokens == nt, (tag, s)
            assert np.array_equal(m._scores[-1], lg), (tag, s)

    def raw(sel, n_sel):
        fp = (C.c_int32 * (2 * nm))(*[t for p in pairs for t in p])
        us = (C.c_int32 * (nm * n_steps))(*[t for u in users for t in u])
        out, done = (C.c_int32 * (nm * n_steps))(), (C.c_int32 * nm)()
        sl = (C.c_int32 * max(len(sel), 1))(*sel)
        N.check(bb._lib.rca_lm_batch_frame_sel(bb._b, sl, n_sel, fp, us, n_steps, -1, None, out, done, None), "rca_lm_batch_frame_sel")

    try:
        assert ba.frame(pairs, users, -1)[0] == bb.frame(pairs, users, -1, members=list(range(nm)))[0]
        snap = [(m.n_tokens, m._scores[-1].copy()) for m in B]
        with pytest.raises(N.RcaError, match=r"sel\[1\] = member 5 is outside the batch's members \[0, 5\)"):
            raw([0, 5, 1], 3)
        unchanged(snap, "index 5")
        with pytest.raises(N.RcaError, match=r"sel\[0\] = member -1 is outside"):
            raw([-1, 2], 2)
        unchanged(snap, "index -1")
        with pytest.raises(N.RcaError, match=r"sel\[2\] = member 3 is selected twice \(also sel\[0\]\)"):
            raw([3, 1, 3], 3)
        unchanged(snap, "duplicate")
        with pytest.raises(N.RcaError, match=r"batch_frame_sel: 0 selected members"):
            raw([], 0)
        unchanged(snap, "n_sel 0")
        with pytest.raises(N.RcaError, match=r"batch_frame_sel: 6 selected members, the batch has 5"):
            raw([0, 1, 2, 3, 4, 0], 6)
        unchanged(snap, "n_sel 6")
        with pytest.raises(N.RcaError):
            bb.frame([], [], -1, members=[])
        # a selected member a token short of the frame's 2 * n_steps; unselected, the same member is no reason to refuse
        keep = B[3].n_tokens
        A[3].n_tokens = B[3].n_tokens = c.n_ctx - 8 + 1
        with pytest.raises(N.RcaError, match=r"context overflow of sel\[1\] = member 3: %d \+ 8 > n_ctx %d" % (c.n_ctx - 7, c.n_ctx)):
            bb.frame(pairs[:2], users[:2], -1, members=[4, 3])
        assert B[3].n_tokens == c.n_ctx - 7
        A[3].n_tokens = B[3].n_tokens = keep
        unchanged(snap, "context overflow")
        with pytest.raises(N.RcaError, match=r"batch_frame_sel: 9 steps"):
            bb.frame(pairs[:2], [[1] * 9] * 2, -1, members=[0, 1])
        bad = [list(u) for u in users[:2]]
        bad[1][2] = c.vocab
        with pytest.raises(N.RcaError, match=r"of sel\[1\] = member 0 at step 2 is outside the vocabulary"):
            bb.frame(pairs[:2], bad, -1, members=[2, 0])
        unchanged(snap, "n_steps 9 / user id == V")
        # the next frame of every member is what the family that saw no refusal gets
        assert ba.frame(pairs, users, -1)[0] == bb.frame(pairs, users, -1, members=list(range(nm)))[0]
        bf._assert_same_state(A, B, [nt for nt, _ in snap], [2 * n_steps] * nm, "after the refusals")
    finally:
        ba.close()
        bb.close()
