"""rca_lm_batch_frame / LlamaBatch.frame: a whole frame of n_steps S=2 steps for 2 to 64 sessions in one launch sequence.

A batch step promises that a member's result does not depend on slot, companions or graphs, so a batch frame is held BIT FOR BIT to
the same steps taken one call at a time.  Two families over the same weight values are prepared identically; family A is stepped with
LlamaBatch.step n_steps times, the sampled tokens fed back on the host, family B gets ONE LlamaBatch.frame.  Checked here:
  1. frame == steps: every token, the final logits, n_tokens, the K / V bits of every layer at the new positions, and the next
     batch step's tokens (so the draw counters agree), with mixed samplers, from start contexts that include an empty cache, a
     frame that crosses the 256-key attention split inside itself (250, 8 steps), 511 and n_ctx - 2 * n_steps (the last slot);
  2. a frame that ends in the second graph bucket (n_ctx 1280, start 1020) beside a member at 0;
  3. graphs on == graphs off;
  4. cut frames: n_done, the -1 padding, n_tokens, K / V of the steps that stand, "no logits" on cut members, and then one batch step
     whose draws are oracle/sampler_oracle.c's at counter c0 + n_done, whose logits are inside bound(want, TOL_TILE) of LMRef on
     the member's true sequence and whose layer-0 K / V rows are rca_lm_eval_async's bits;
  5. probes equal token_probs called after the frame, bit for bit; NaN for cut members and probe id -1; probes do not change tokens;
  6. single frame(), batch frame, group step, batch step and batch frame mix;
  7. refusals leave every member unchanged.
All comparisons are np.array_equal unless said otherwise.  The models, samplers and helpers are those of tests/test_lm_batch_gpu.py
(imported, so both files share one family cache).

Every test here fails on a library without rca_lm_batch_frame (the parent commit: LlamaBatch has no frame() and the symbol is
missing)."""
import dataclasses
import functools

import numpy as np
import pytest
import torch

import lm_shape_cases as sc
import test_lm_batch_gpu as bg
from oracle import lm_ref

pytestmark = pytest.mark.gpu

SAMPLERS = bg.SAMPLERS
FAMILY = bg.FAMILY
WHICH_B = 3                                              # family B: its own weights, the same values
CASES = (("g4_k768", "bf16"), ("g4_k768", "q8_0"), ("g4_k768", "q4_k"), ("g1_k768", "bf16"), ("g2_k768", "bf16"))
CASE_IDS = [f"{n}-{f}" for n, f in CASES]
LONG = dataclasses.replace(bg.G4, name="g4_k768_ctx1280", n_ctx=1280)     # five 256-key splits: the second graph bucket exists


def _starts(n_ctx, nm, n_steps):
    last = n_ctx - 2 * n_steps
    pool = (0, 250, 511, last, 1, 254, 255, 256, 300, 512)
    if nm == 5:
        return [0, 250, 511, last, 300]
    return [pool[s % len(pool)] for s in range(nm)]


def _inputs(ids, nm, n_steps, salt=0):
    """(first pairs, user ids) of a frame: a different stream per member"""
    L = len(ids)
    pairs = [[ids[(500 + 31 * (s + salt) + j) % L] for j in range(2)] for s in range(nm)]
    users = [[ids[(700 + 17 * (s + salt) + i) % L] for i in range(n_steps)] for s in range(nm)]
    return pairs, users


def _steps(bat, pairs, users):
    """the reference: len(users[s]) batch steps with the sampled tokens fed back on the host; tokens per member"""
    rows = [list(p) for p in pairs]
    toks = [[] for _ in pairs]
    for i in range(len(users[0])):
        out = bat.step(rows)
        for s, t in enumerate(out):
            toks[s].append(t)
        rows = [[t, users[s][i]] for s, t in enumerate(out)]
    return toks


def _kv_all(m, pos, n):
    return [bg._kv_bits(m, layer, pos, n) for layer in range(m.config.n_layers)]


def _assert_same_state(A, B, starts, n_new, tag):
    """logits, n_tokens and the K / V bits of every layer at the n_new[s] positions from starts[s]"""
    for s, (a, b) in enumerate(zip(A, B)):
        assert a.n_tokens == b.n_tokens == starts[s] + n_new[s], (tag, "n_tokens of member", s, a.n_tokens, b.n_tokens)
        assert np.array_equal(a._scores[-1], b._scores[-1]), (tag, "logits of member", s)
        for layer, ((ka, va), (kb, vb)) in enumerate(zip(_kv_all(a, starts[s], n_new[s]), _kv_all(b, starts[s], n_new[s]))):
            assert ka.any() and va.any()
            assert np.array_equal(ka, kb), (tag, "K of member", s, "layer", layer)
            assert np.array_equal(va, vb), (tag, "V of member", s, "layer", layer)


def _graphs_back_on(*fams):
    for fam in fams:
        for m in fam:
            m.set_graphs(True)


def _frame_against_steps(A, B, ids, starts, n_steps, tag, graphs_b=True):
    from realtime_codec_agent_amd.llm import LlamaBatch
    nm = len(A)
    bg._prepare(A, ids, starts, samplers=SAMPLERS)
    bg._prepare(B, ids, starts, graphs=graphs_b, samplers=SAMPLERS)
    pairs, users = _inputs(ids, nm, n_steps)
    ba, bb = LlamaBatch(A), LlamaBatch(B)
    try:
        want = _steps(ba, pairs, users)
        got, probs = bb.frame(pairs, users, -1)
        assert probs is None
        assert got == want, (tag, "tokens")
        _assert_same_state(A, B, starts, [2 * n_steps] * nm, tag)
        # the next draw of every member: equal tokens, so the draw counters (and penalty windows) agree.  A member whose frame filled
        # its cache is rolled back to its start first, in both families (a draw does not depend on the position).
        for s in range(nm):
            if A[s].n_tokens + 1 > A[s].n_ctx():
                A[s].n_tokens = B[s].n_tokens = starts[s]
        nxt = [[ids[(40 + s) % len(ids)]] for s in range(nm)]
        assert ba.step(nxt) == bb.step(nxt), (tag, "next step")
    finally:
        ba.close()
        bb.close()
        _graphs_back_on(B)
    return want


# ---------------------------------------------------------------------------------------------- 1. frame == steps
@pytest.mark.parametrize("n_steps", (1, 3, 8))
@pytest.mark.parametrize("nm", (5, 33, 64))
@pytest.mark.parametrize("name,fmt", CASES, ids=CASE_IDS)
def test_a_frame_is_the_same_steps_taken_one_call_at_a_time(name, fmt, nm, n_steps):
    """Uncut (floor -1), mixed samplers (greedy / top-k 40 with bias and penalties / top-k 50 / whole vocabulary).  The members that
    start at n_ctx - 2 * n_steps write the last slot of their caches."""
    ids = bg._ids(name)
    n_ctx = bg.MODELS[name].n_ctx
    A, B = bg._family(name, fmt)[:nm], bg._family(name, fmt, WHICH_B, FAMILY)[:nm]
    starts = _starts(n_ctx, nm, n_steps)
    _frame_against_steps(A, B, ids, starts, n_steps, (name, fmt, nm, n_steps))


# ---------------------------------------------------------------------------------------------- 2. bucket crossing
@functools.lru_cache(maxsize=None)
def _long_family(which):
    from realtime_codec_agent_amd.llm import LlamaForAlternatingCodeChannels as L
    c = LONG
    parent = L(model_path=f"random:{c.name}", config=c.config(), n_ctx=c.n_ctx, random_seed=c.seed, init_std=sc.INIT_STD, device=0, weight_format="bf16")
    assert parent.prefill_route() == "gemm128"
    return [parent] + [L(n_ctx=c.n_ctx, share_weights_with=parent, device=0) for _ in range(2)]


def test_a_frame_that_ends_in_the_second_graph_bucket():
    """n_ctx 1280 has five 256-key splits; a graph of the first bucket launches four.  The frame starts at 1020 and ends at 1028, so its
    graph is the second bucket's although its first steps need four splits only; the other member starts at 0."""
    ids = LONG.ids().tolist()
    A, B = _long_family(0)[:2], _long_family(1)[:2]
    _frame_against_steps(A, B, ids, [1020, 0], 4, "bucket crossing")


# ---------------------------------------------------------------------------------------------- 3. graphs on == graphs off
@pytest.mark.parametrize("name,fmt", (("g4_k768", "bf16"), ("g4_k768", "q4_k")), ids=("g4-bf16", "g4-q4_k"))
def test_an_eager_frame_gives_the_replayed_frames_bits(name, fmt):
    """the eager frame of family B against the steps of family A (graph replays; test 1 holds the replayed frame to the same steps)"""
    ids = bg._ids(name)
    nm, n_steps = 9, 4
    A, B = bg._family(name, fmt)[:nm], bg._family(name, fmt, WHICH_B, FAMILY)[:nm]
    starts = [0, 250, 511, 300, 254, 1, 255, 256, 512]
    _frame_against_steps(A, B, ids, starts, n_steps, (name, fmt, "eager"), graphs_b=False)


# ---------------------------------------------------------------------------------------------- 4. cut frames
def _n_done(toks, floor):
    for j, t in enumerate(toks):
        if t <= floor:
            return j + 1
    return len(toks)


def _kinds(all_toks, floor):
    """(members cut before the last step, members cut exactly at the last step, members not cut) by family A's tokens"""
    early, at_last, uncut = [], [], []
    for s, toks in enumerate(all_toks):
        d = _n_done(toks, floor)
        if d < len(toks):
            early.append(s)
        elif toks[-1] <= floor:
            at_last.append(s)
        else:
            uncut.append(s)
    return early, at_last, uncut


def _floor_from(all_toks):
    """The floor comes from family A's own tokens at run time: the order statistics of its step-1 tokens from the middle outwards,
    then its other tokens in ascending order; the first that gives all three kinds of member.  None when no token does."""
    first = sorted(t[0] for t in all_toks)
    mid = len(first) // 2
    cand = sorted(first, key=lambda t: abs(first.index(t) - mid)) + sorted({t for toks in all_toks for t in toks[1:]})
    for f in cand:
        if all(_kinds(all_toks, f)):
            return f
    return None


def test_cut_frames_leave_what_the_step_by_step_loop_leaves():
    from realtime_codec_agent_amd import _native as N
    from realtime_codec_agent_amd.llm import LlamaBatch
    name, fmt, nm, n_steps = "g4_k768", "bf16", 9, 4
    ids = bg._ids(name)
    famB = bg._family(name, fmt, WHICH_B, FAMILY)
    A, B, twin = bg._family(name, fmt)[:nm], famB[:nm], famB[FAMILY - 1]
    starts = [0, 250, 511, 300, 254, 1, 255, 256, 512]
    bg._prepare(A, ids, starts, samplers=SAMPLERS)
    bg._prepare(B, ids, starts, samplers=SAMPLERS)
    pairs, users = _inputs(ids, nm, n_steps)
    ba, bb = LlamaBatch(A), LlamaBatch(B)
    try:
        toks_a = _steps(ba, pairs, users)
        floor = _floor_from(toks_a)
        print("CUT tokens of family A", toks_a, "floor", floor)
        assert floor is not None, ("no token of family A gives a member cut early, one cut at the last step and one not cut", toks_a)
        early, at_last, uncut = _kinds(toks_a, floor)
        assert early and at_last and uncut, (floor, toks_a)
        want_done = [_n_done(t, floor) for t in toks_a]
        got, probs = bb.frame(pairs, users, floor)
        assert got == [t[:d] for t, d in zip(toks_a, want_done)]
        # the C ABI's own outputs: the -1 padding behind a cut (a second, identical frame on a re-prepared family)
        bg._prepare(B, ids, starts, samplers=SAMPLERS)
        import ctypes as C
        fp = (C.c_int32 * (2 * nm))(*[t for p in pairs for t in p])
        us = (C.c_int32 * (nm * n_steps))(*[t for u in users for t in u])
        out, done = (C.c_int32 * (nm * n_steps))(), (C.c_int32 * nm)()
        N.check(bb._lib.rca_lm_batch_frame(bb._b, fp, us, n_steps, floor, None, out, done, None), "rca_lm_batch_frame")
        assert list(done) == want_done
        for s in range(nm):
            assert list(out[s * n_steps:(s + 1) * n_steps]) == toks_a[s][:want_done[s]] + [-1] * (n_steps - want_done[s]), s
        for s in range(nm):
            d = want_done[s]
            assert B[s].n_tokens == starts[s] + 2 * d, s
            for layer, ((ka, va), (kb, vb)) in enumerate(zip(_kv_all(A[s], starts[s], 2 * d), _kv_all(B[s], starts[s], 2 * d))):
                assert np.array_equal(ka, kb) and np.array_equal(va, vb), ("K / V of member", s, "layer", layer)
            B[s]._logits_valid = False
            if s in early:
                for what, call in (("get_logits", B[s]._fetch_logits), ("sample", B[s].sample), ("token_probs", lambda: B[s].token_probs([3]))):
                    with pytest.raises(N.RcaError, match="no logits"):
                        call()
            else:        # complete, cut at the last step or not: the last step's logits, as family A has them
                assert np.array_equal(B[s]._scores[-1], A[s]._scores[-1]), s
        # one batch step on B from where the frame left every member
        fresh = [[ids[(900 + 7 * s + j) % len(ids)] for j in range(2)] for s in range(nm)]
        at = [m.n_tokens for m in B]
        drawn = bb.step(fresh)
        worst = 0.0
        for s in range(nm):
            d, p = want_done[s], SAMPLERS[s % len(SAMPLERS)]
            lg = B[s]._scores[-1].copy()
            want_tok = lm_ref.sample(lg, p["top_k"], p["top_p"], p["min_p"], p["temp"], p["seed"], d, p.get("logit_bias"),
                                     repeat_penalty=p.get("repeat_penalty", 1.0), prev_tokens=toks_a[s][:d])
            assert drawn[s] == want_tok, ("draw of member", s, "at counter", d, drawn[s], want_tok)
            seq = pairs[s] + [t for pair in zip(toks_a[s][:d - 1], users[s]) for t in pair] + fresh[s]
            assert B[s]._input_ids[starts[s]:starts[s] + len(seq)].tolist() == seq, s
            want = bg._oracle_at(name, fmt, starts[s]).eval(seq)[-1].numpy()
            ratio = float(np.abs(lg - want).max()) / sc.bound(want, sc.TOL_TILE)
            worst = max(worst, ratio)
            assert ratio <= 1.0, ("logits of member", s, ratio)
            twin.n_tokens = at[s]
            twin.eval_async(fresh[s])
            twin.sync()
            kw, vw = bg._kv_bits(twin, 0, at[s], 2)
            kg, vg = bg._kv_bits(B[s], 0, at[s], 2)
            assert kw.any() and np.array_equal(kg, kw) and np.array_equal(vg, vw), ("layer 0 K / V rows of member", s)
        print(f"CUT n_done {want_done}; step after the frame: worst max|dlogit| / bound(TOL_TILE) = {worst:.3f}")
    finally:
        ba.close()
        bb.close()


# ---------------------------------------------------------------------------------------------- 5. probes
def test_probes_are_token_probs_of_the_last_logits():
    from realtime_codec_agent_amd.llm import LlamaBatch
    name, fmt, nm, n_steps = "g4_k768", "q8_0", 9, 4
    ids = bg._ids(name)
    A, B = bg._family(name, fmt)[:nm], bg._family(name, fmt, WHICH_B, FAMILY)[:nm]
    starts = [0, 250, 511, 300, 254, 1, 255, 256, 512]
    pairs, users = _inputs(ids, nm, n_steps)
    ba, bb = LlamaBatch(A), LlamaBatch(B)
    try:
        bg._prepare(A, ids, starts, samplers=SAMPLERS)
        full, _ = ba.frame(pairs, users, -1)
        floor = _floor_from(full)
        assert floor is not None, full
        early, at_last, uncut = _kinds(full, floor)
        complete = at_last + uncut
        probe = [-1 if s == complete[0] else (5 + 100 * s) % bg.MODELS[name].vocab for s in range(nm)]
        bg._prepare(A, ids, starts, samplers=SAMPLERS)
        bg._prepare(B, ids, starts, samplers=SAMPLERS)
        plain, none = ba.frame(pairs, users, floor)
        got, probs = bb.frame(pairs, users, floor, probe_ids=probe)
        assert none is None and got == plain == [t[:_n_done(t, floor)] for t in full]
        assert probs.dtype == np.float32 and probs.shape == (nm,)
        checked = 0
        for s in range(nm):
            if s in early or probe[s] < 0:
                assert np.isnan(probs[s]), s
            else:
                want = B[s].token_probs([probe[s]])
                assert 0.0 < probs[s] < 1.0 and probs[s].tobytes() == want[0].tobytes(), (s, probs[s], want)
                assert np.array_equal(B[s]._scores[-1], A[s]._scores[-1]), s
                checked += 1
        assert checked >= 1 and np.isnan(probs[complete[0]]) and np.isnan(probs[early[0]])
    finally:
        ba.close()
        bb.close()


# ---------------------------------------------------------------------------------------------- 6. mixing
@pytest.mark.parametrize("graphs", (True, False), ids=("graph", "eager"))
def test_single_frames_batch_frames_group_steps_and_batch_steps_mix(graphs):
    """single frame() on member 0, batch frame, group step on members 1 and 2, batch step, batch frame: family B takes the batch frames
    as frames, family A as steps; everything else is the same call on both."""
    from realtime_codec_agent_amd.llm import LlamaBatch, LlamaGroup
    name, fmt, nm, n_steps = "g4_k768", "q8_0", 6, 3
    ids = bg._ids(name)
    starts = [254, 40, 300, 0, 511, 250]
    A, B = bg._family(name, fmt)[:nm], bg._family(name, fmt, WHICH_B, FAMILY)[:nm]
    res = []
    for fam, framed in ((A, False), (B, True)):
        bg._prepare(fam, ids, starts, graphs=graphs, samplers=SAMPLERS)
        bat, grp = LlamaBatch(fam), LlamaGroup(fam[1:3])
        run = (lambda p, u: bat.frame(p, u, -1)[0]) if framed else (lambda p, u: _steps(bat, p, u))
        try:
            out = [fam[0].frame(ids[600:602], ids[610:612], -1)]
            out.append(run(*_inputs(ids, nm, n_steps)))
            out.append(grp.step([ids[620:622], ids[630:632]]))
            out.append(bat.step(bg._rows(ids, nm, 2, 5)))
            out.append(run(*_inputs(ids, nm, n_steps, salt=3)))
            out.append(fam[0].sample())
        finally:
            grp.close()
            bat.close()
            _graphs_back_on(fam)
        res.append(out)
    assert res[0] == res[1]
    grown = [4 + 2 * n_steps + 2 + 2 * n_steps] + [2 * n_steps + 2 + 2 + 2 * n_steps] * 2 + [2 * n_steps + 2 + 2 * n_steps] * 3
    _assert_same_state(A, B, starts, grown, "mixing")


# ---------------------------------------------------------------------------------------------- 7. refusals
def test_refusals_leave_every_member_unchanged():
    from realtime_codec_agent_amd import _native as N
    from realtime_codec_agent_amd.llm import LlamaForAlternatingCodeChannels as L, LlamaBatch
    name, fmt, nm = "g4_k768", "bf16", 5
    c = bg.MODELS[name]
    ids = bg._ids(name)
    fam = bg._family(name, fmt, WHICH_B, FAMILY)
    A, B = bg._family(name, fmt)[:nm], fam[:nm]
    starts = [30, 40, 254, 300, 511]
    V = c.vocab
    bg._prepare(A, ids, starts, samplers=SAMPLERS)
    bg._prepare(B, ids, starts, samplers=SAMPLERS)
    ba, bb = LlamaBatch(A), LlamaBatch(B)
    pairs, users = _inputs(ids, nm, 4)

    def unchanged(snap, tag):
        for s, (m, (nt, lg)) in enumerate(zip(B, snap)):
            assert m.n_tokens == nt, (tag, s)
            assert np.array_equal(m._scores[-1], lg), (tag, s)

    try:
        assert ba.frame(pairs, users, -1)[0] == bb.frame(pairs, users, -1)[0]        # logits to snapshot, both families alike
        snap = [(m.n_tokens, m._scores[-1].copy()) for m in B]
        with pytest.raises(N.RcaError, match=r"batch_frame: 0 steps"):
            bb.frame(pairs, [[] for _ in range(nm)], -1)
        unchanged(snap, "n_steps 0")
        with pytest.raises(N.RcaError, match=r"batch_frame: 9 steps"):
            bb.frame(pairs, [[1] * 9 for _ in range(nm)], -1)
        unchanged(snap, "n_steps 9")
        with pytest.raises(N.RcaError, match="65 members"):
            LlamaBatch(fam[:65])
        # one member a token short of the frame's 2 * n_steps (the others have room)
        keep = B[3].n_tokens
        B[3].n_tokens = c.n_ctx - 8 + 1
        with pytest.raises(N.RcaError, match=r"context overflow of member 3: %d \+ 8 > n_ctx %d" % (c.n_ctx - 7, c.n_ctx)):
            bb.frame(pairs, users, -1)
        assert B[3].n_tokens == c.n_ctx - 7
        B[3].n_tokens = keep
        unchanged(snap, "context overflow")
        bad = [list(p) for p in pairs]
        bad[4][1] = V
        with pytest.raises(N.RcaError, match="of member 4 at index 1 of its first pair is outside the vocabulary"):
            bb.frame(bad, users, -1)
        unchanged(snap, "first pair id == V")
        bad = [list(u) for u in users]
        bad[2][3] = -1
        with pytest.raises(N.RcaError, match="of member 2 at step 3 is outside the vocabulary"):
            bb.frame(pairs, bad, -1)
        unchanged(snap, "user id -1")
        for pid in (V, -2):
            with pytest.raises(N.RcaError, match="probe id %d of member 1 is outside the vocabulary" % pid):
                bb.frame(pairs, users, -1, probe_ids=[3, pid, 3, 3, 3])
            unchanged(snap, f"probe id {pid}")
        bare = L(n_ctx=c.n_ctx, share_weights_with=B[0], device=0)
        try:
            b3 = LlamaBatch([B[0], B[1], bare])
            try:
                with pytest.raises(N.RcaError, match="batch_frame: member 2 has no sampler"):
                    b3.frame(pairs[:3], users[:3], -1)
                bare.init_sampler_for_generate(**bg.GREEDY)
                N.check(bare._lib.rca_lm_set_logits_all(bare._h, 1), "rca_lm_set_logits_all")
                with pytest.raises(N.RcaError, match="batch_frame: member 2 was switched to logits_all"):
                    b3.frame(pairs[:3], users[:3], -1)
            finally:
                b3.close()
        finally:
            bare.close()
        unchanged(snap, "no sampler / logits_all")
        # the next draw of every member is what the family that saw no refusal draws, and the frame still runs
        nxt = bg._rows(ids, nm, 2, 7)
        assert ba.step(nxt) == bb.step(nxt)
        assert ba.frame(pairs, users, -1)[0] == bb.frame(pairs, users, -1)[0]
        _assert_same_state(A, B, [nt + 2 for nt, _ in snap], [8] * nm, "after the refusals")
    finally:
        ba.close()
        bb.close()
