"""rca_duplex_batch_frame / LlamaBatch.duplex_frame: rca_duplex_frame for every selected member of a batch in one call.

Model and codec as in tests/test_agent_gpu.py::make_agent (LM 256 wide, 2 layers, 4 heads over 2 kv heads, the codec tokens behind the
text rows of the vocabulary), n_ctx 1024, a parent and 16 twins per family.  Family B takes ONE LlamaBatch.duplex_frame per tick; family
A (its own weights, the same values) takes the separate calls: encode_tail of each row alone, frame(members=...), decode_tail of each
row alone, token_probs.  Compared per member with np.array_equal: user_codes, tokens, flags (pcm None or not), PCM, probe, n_tokens.
The first tick of a (class, shape) runs eagerly, later ticks replay; contexts roll on the host between ticks.

Every test here fails on a library without rca_duplex_batch_frame (the parent commit: the symbol is missing)."""
import functools

import numpy as np
import pytest

from conftest import rich_signal

pytestmark = pytest.mark.gpu

NM = 17
N_CTX = 1024
SHAPE_A = dict(T=32000, F_ctx=96, n=4, n_samples=1440)
SHAPE_B = dict(T=16000, F_ctx=48, n=2, n_samples=800)       # a second shape: its graphs live beside the first's
SAMPLER = dict(top_k=100, top_p=1.0, min_p=0.0, temp=1.0)


@functools.lru_cache(maxsize=None)
def _world():
    """(audio tokenizer, base, codebook size, end_audio id): one codec handle for every family"""
    from realtime_codec_agent_amd.audio_tokenizer import AudioTokenizer
    from realtime_codec_agent_amd.tokenizer import CodecTokenizer
    at = AudioTokenizer(codec_model="MagiCodec-50Hz-Base", device=None)
    tok = CodecTokenizer(codebook_size=at.codebook_size, unicode_offset=at.unicode_offset)
    return at, tok


@functools.lru_cache(maxsize=None)
def _family(which, masked=True):
    from realtime_codec_agent_amd.llm import LlamaForAlternatingCodeChannels as L, LMConfig
    at, tok = _world()
    lm = LMConfig(vocab_size=259344, hidden=256, n_layers=2, n_heads=4, n_kv_heads=2, head_dim=64, ffn=512)
    parent = L(model_path="random:small", n_ctx=N_CTX, config=lm, random_seed=3)
    assert parent.prefill_route() == "gemm128"
    if masked:      # head rows outside the codec range are zeroed: the sampler stays on codec tokens
        parent.mask_head_rows(0, tok.codec_vocab_start)
        parent.mask_head_rows(len(tok), parent.n_vocab())
    return [parent] + [L(model_path="random:small", n_ctx=N_CTX, share_weights_with=parent) for _ in range(NM - 1)]


def _base():
    at, tok = _world()
    return tok.codec_vocab_start, at.codebook_size


def _prepare(fam, seed0=0, graphs=True):
    base, ncb = _base()
    for s, m in enumerate(fam):
        rng = np.random.default_rng(100 + s)
        prompt = [int(t) for t in rng.integers(base, base + ncb, size=20 + 3 * s)]
        m.set_graphs(graphs)
        m.reset()
        m.eval(prompt)
        m.init_sampler_for_generate(seed=seed0 + 11 + s, **SAMPLER)
    return [[int(m._input_ids[m.n_tokens - 2]), int(m._input_ids[m.n_tokens - 1])] for m in fam]


class _Host:
    """the host side of NM sessions: each member's signal, rolling code context and last pair"""

    def __init__(self, pairs, shape, seed=17):
        _, ncb = _base()
        self.shape = shape
        self.sig = [rich_signal(shape["T"] + 1280 * 12, seed + s) for s in range(NM)]
        self.ctx = [np.random.default_rng(50 + s).integers(0, ncb, size=shape["F_ctx"]).astype(np.int64) for s in range(NM)]
        self.pairs = [list(p) for p in pairs]
        self.tick = [0] * NM

    def window(self, s):
        o = 1280 * (self.tick[s] + 1) + 37 * s
        return self.sig[s][o:o + self.shape["T"]]

    def commit(self, s, toks, codes, complete):
        base, _ = _base()
        if complete:
            new = np.array([t - base for t in toks], dtype=np.int64)
            both = np.concatenate([self.ctx[s], new])
            self.ctx[s] = both[len(both) - self.shape["F_ctx"]:]
        self.pairs[s] = [toks[-1], base + int(codes[len(toks) - 1])]
        self.tick[s] += 1


def _reference_tick(ba, A, host, sel, floor, probes):
    """the separate calls on family A; per member a dict like duplex_frame's"""
    at, _ = _world()
    hip = at.codec_model.hip
    base, ncb = _base()
    sh = host.shape
    codes = [hip.encode_tail(host.window(s)[None], sh["n"])[0] for s in sel]
    toks, _ = ba.frame([host.pairs[s] for s in sel], [[base + int(c) for c in cs] for cs in codes], floor, members=sel)
    res = []
    for k, s in enumerate(sel):
        complete = len(toks[k]) == sh["n"]
        in_book = all(base <= t < base + ncb for t in toks[k])
        pcm = None
        if complete and in_book:
            new = np.array([t - base for t in toks[k]], dtype=np.int64)
            pcm = hip.decode_tail(np.concatenate([host.ctx[s], new])[None], sh["n_samples"])[0]
        prob = None
        if complete and probes is not None and probes[k] >= 0:
            prob = float(A[s].token_probs([probes[k]])[0])
        res.append({"user_codes": [int(c) for c in codes[k]], "tokens": toks[k], "pcm": pcm, "probe_prob": prob,
                    "flags": (0 if in_book else 1) | (0 if complete else 2)})
    return res


def _batch_tick(bb, host, sel, floor, probes):
    at, _ = _world()
    sh = host.shape
    base, _ = _base()
    return bb.duplex_frame(at.codec_model.hip, sel, np.stack([host.window(s) for s in sel]), np.stack([host.ctx[s] for s in sel]), sh["n"], sh["n_samples"],
                           base, floor, probes, [host.pairs[s] for s in sel])


def _assert_tick(got, want, A, B, sel, tag):
    for k, s in enumerate(sel):
        g, w = got[k], want[k]
        assert g["user_codes"] == w["user_codes"], (tag, "user codes of member", s)
        assert g["tokens"] == w["tokens"], (tag, "tokens of member", s)
        assert (g["pcm"] is None) == (w["pcm"] is None), (tag, "flags of member", s)
        if w["pcm"] is not None:
            assert np.array_equal(g["pcm"], w["pcm"]), (tag, "PCM of member", s)
        assert g["probe_prob"] == w["probe_prob"], (tag, "probe of member", s, g["probe_prob"], w["probe_prob"])
        assert A[s].n_tokens == B[s].n_tokens, (tag, "n_tokens of member", s)
        assert g["flags"] == w["flags"], (tag, "flag bits of member", s, g["flags"], w["flags"])
        # a cut member has NO logits (its buffer holds a rolled-back step's), a complete one its last step's
        cut = bool(w["flags"] & 2)
        assert len(B[s]._scores) == len(A[s]._scores) == (0 if cut else 1), (tag, "logits rows of member", s)
        if not cut:
            assert np.array_equal(A[s]._scores[-1], B[s]._scores[-1]), (tag, "logits of member", s)


def _run(sels, shape=SHAPE_A, floor=None, probe_of=lambda s: 7 + s, graphs=True, masked=True, fams=(0, 1)):
    from realtime_codec_agent_amd.llm import LlamaBatch
    A, B = _family(fams[0], masked), _family(fams[1], masked)
    pa, pb = _prepare(A), _prepare(B, graphs=graphs)
    assert pa == pb
    ha, hb = _Host(pa, shape), _Host(pb, shape)
    ba, bb = LlamaBatch(A), LlamaBatch(B)
    floor = -1 if floor is None else floor
    seen = []
    try:
        for t, sel in enumerate(sels):
            probes = None if probe_of is None else [probe_of(s) for s in sel]
            want = _reference_tick(ba, A, ha, sel, floor, probes)
            got = _batch_tick(bb, hb, sel, floor, probes)
            _assert_tick(got, want, A, B, sel, ("tick", t))
            for k, s in enumerate(sel):
                for host, r in ((ha, want[k]), (hb, got[k])):
                    host.commit(s, r["tokens"], r["user_codes"], r["pcm"] is not None)
            seen.append((got, want))
        # the next step of every member: the draw counters agree
        nxt = [[ha.pairs[s][0]] for s in range(NM)]
        assert ba.step(nxt) == bb.step(nxt)
    finally:
        ba.close()
        bb.close()
        for m in B:
            m.set_graphs(True)
    return seen


ALL = list(range(NM))


def test_six_ticks_equal_the_separate_calls():
    """all 17 members (the class of 32 rows), six ticks: the first eager, the others replayed; no member is flagged"""
    seen = _run([ALL] * 6)
    assert all(r["pcm"] is not None and r["probe_prob"] is not None and len(r["tokens"]) == 4 for got, _ in seen for r in got)


def test_selections_that_change_between_ticks_and_two_shapes():
    """|sel| = 2, 5 and 9 of the 17 members, unsorted, changing between ticks; then the same on a shorter shape whose graphs coexist"""
    sels = [[3, 11], [0, 4, 8, 12, 16], [16, 1, 2, 5, 7, 9, 10, 13, 15], [3, 11], [12, 0, 4, 16, 8], [1, 2, 5, 7, 9, 10, 13, 15, 16]]
    _run(sels)
    _run(sels[:4], shape=SHAPE_B)
    _run(sels[2:5])


def test_a_floor_above_every_id_cuts_every_member():
    seen = _run([ALL[:9], ALL[:9]], floor=259344)
    for got, _ in seen:
        assert all(len(r["tokens"]) == 1 and r["pcm"] is None and r["probe_prob"] is None for r in got)


def test_one_member_cut_while_the_others_are_complete():
    """the floor is the smallest first-step token of the reference's own uncut run: exactly the members that sampled it are cut"""
    sel = ALL[:9]
    uncut = _run([sel])[0][1]
    floor = min(r["tokens"][0] for r in uncut)
    got = _run([sel, sel], floor=floor)[0][0]
    cut = [k for k, r in enumerate(got) if len(r["tokens"]) < 4]
    assert cut and len(cut) < len(sel)
    assert all((got[k]["pcm"] is None) == (k in cut) for k in range(len(sel)))


def test_sampled_tokens_outside_the_codebook_raise_flag_bit_0():
    """head rows unmasked: some members sample text or padding ids.  Their PCM is withheld, the others' equals the reference"""
    base, ncb = _base()
    seen = _run([ALL, ALL], masked=False, fams=(2, 3))
    flagged = [r["pcm"] is None for got, _ in seen for r in got]
    outside = [not all(base <= t < base + ncb for t in r["tokens"]) for _, want in seen for r in want]
    assert flagged == outside and any(flagged)


def test_graphs_off_gives_the_replayed_ticks_bits():
    _run([ALL[:9]] * 3, graphs=False)


def test_probe_minus_one_for_some_members():
    seen = _run([ALL[:9]] * 2, probe_of=lambda s: -1 if s % 3 == 0 else 7 + s)
    for got, _ in seen:
        assert [r["probe_prob"] is None for r in got] == [s % 3 == 0 for s in range(9)]
    _run([ALL[:5]] * 2, probe_of=None)


def test_a_pcm_row_of_a_flagged_member_is_untouched():
    """the C ABI's own outputs: sentinel-filled PCM rows stay as they are for cut members, tokens are -1 from n_done on"""
    import ctypes as C
    from realtime_codec_agent_amd import _native as N
    from realtime_codec_agent_amd.llm import LlamaBatch
    at, _ = _world()
    base, _ = _base()
    B = _family(1, True)
    host = _Host(_prepare(B), SHAPE_A)
    sel, sh = [2, 0, 5], SHAPE_A
    bb = LlamaBatch(B)
    try:
        nm = len(sel)
        win = np.ascontiguousarray(np.stack([host.window(s) for s in sel]))
        ctx = np.ascontiguousarray(np.stack([host.ctx[s] for s in sel]))
        sl = (C.c_int32 * nm)(*sel)
        fp = (C.c_int32 * (2 * nm))(*[t for s in sel for t in host.pairs[s]])
        a = N.DuplexBatchArgsC(sel=C.addressof(sl), n_sel=nm, pcm_windows=win.ctypes.data, code_ctx=ctx.ctypes.data, first_pairs=C.addressof(fp), probe_ids=None,
                               T=sh["T"], F_ctx=sh["F_ctx"], n_steps=sh["n"], n_samples=sh["n_samples"], code_token_base=base, audio_id_floor=259344)
        codes, toks = np.zeros((nm, 8), np.int64), np.zeros((nm, 8), np.int32)
        done, flags, prob = np.zeros(nm, np.int32), np.zeros(nm, np.int32), np.zeros(nm, np.float32)
        out = N.DuplexBatchOutC(user_codes=codes.ctypes.data, tokens=toks.ctypes.data, n_done=done.ctypes.data, flags=flags.ctypes.data, probe_prob=prob.ctypes.data)
        pcm = np.full((nm, sh["n_samples"]), 7.5, np.float32)
        N.check(bb._lib.rca_duplex_batch_frame(bb._b, at.codec_model.hip._h, C.byref(a), C.byref(out), C.c_void_p(pcm.ctypes.data)), "rca_duplex_batch_frame")
        assert done.tolist() == [1] * nm and flags.tolist() == [2] * nm and prob.tolist() == [-1.0] * nm
        assert (toks[:, 1:] == -1).all() and (toks[:, 0] >= base).all()
        assert (pcm == 7.5).all()
    finally:
        bb.close()


def test_an_empty_code_context_is_a_call_shape_too():
    """F_ctx = 0: the decode runs over the frame's own codes only"""
    _run([ALL[:5], ALL[:5], [2, 0]], shape=dict(T=32000, F_ctx=0, n=4, n_samples=1280))


def test_refusals_change_nothing():
    from realtime_codec_agent_amd import _native as N
    from realtime_codec_agent_amd.llm import LlamaBatch
    at, _ = _world()
    hip = at.codec_model.hip
    base, ncb = _base()
    A, B = _family(0, True), _family(1, True)
    pa, pb = _prepare(A), _prepare(B)
    host = _Host(pb, SHAPE_A)
    sel = [4, 1, 9]
    bb = LlamaBatch(B)
    sh = SHAPE_A
    win = np.stack([host.window(s) for s in sel])
    ctx = np.stack([host.ctx[s] for s in sel])
    pairs = [host.pairs[s] for s in sel]
    snap = [(m.n_tokens, m._scores.copy()) for m in B]

    def unchanged(tag):
        for s, (m, (nt, lg)) in enumerate(zip(B, snap)):
            assert m.n_tokens == nt and np.array_equal(m._scores, lg), (tag, s)

    try:
        bad = ctx.copy()
        bad[1, 40] = ncb
        with pytest.raises(N.RcaError, match=r"code %d of sel\[1\] = member 1 at index 40 of its context is out of range" % ncb):
            bb.duplex_frame(hip, sel, win, bad, sh["n"], sh["n_samples"], base, -1, None, pairs)
        unchanged("context code")
        with pytest.raises(N.RcaError, match="fall outside the vocabulary"):
            bb.duplex_frame(hip, sel, win, ctx, sh["n"], sh["n_samples"], 259344 - ncb + 1, -1, None, pairs)
        unchanged("base")
        with pytest.raises(N.RcaError, match=r"samples wanted, 100 codes give"):
            bb.duplex_frame(hip, sel, win, ctx, sh["n"], 100 * 4000, base, -1, None, pairs)
        unchanged("n_samples")
        with pytest.raises(N.RcaError, match=r"duplex_batch_frame: 0 steps"):
            bb.duplex_frame(hip, sel, win, ctx, 0, sh["n_samples"], base, -1, None, pairs)
        with pytest.raises(N.RcaError, match=r"duplex_batch_frame: 9 steps"):
            bb.duplex_frame(hip, sel, win, ctx, 9, sh["n_samples"], base, -1, None, pairs)
        with pytest.raises(N.RcaError, match=r"sel\[1\] = member 4 is selected twice"):
            bb.duplex_frame(hip, [4, 4, 9], win, ctx, sh["n"], sh["n_samples"], base, -1, None, pairs)
        unchanged("n_steps / duplicate")
        # and the call still runs, as on a family that saw no refusal
        ha = _Host(pa, SHAPE_A)
        ba = LlamaBatch(A)
        try:
            want = _reference_tick(ba, A, ha, sel, -1, None)
        finally:
            ba.close()
        _assert_tick(_batch_tick(bb, host, sel, -1, None), want, A, B, sel, "after the refusals")
    finally:
        bb.close()
