"""typical_p and mirostat v2 on the device, through the tests-only rca_lm_put_logits: every draw token for token against the float32
restatement of tests/samp_ext_ref.py (the definition), mirostat's mu bit for bit after every draw, and the float64 allowed sets where
their margins are clear (tests/test_sampler_ext_cpu.py holds the restatement itself to the float64 references and asserts that the
rows meant for that check are clear).  Then what rides on the draw counter: a cut frame and a cut batch frame rewind mu, a second
init restores it, a change of mode re-captures the graphs, and a replayed step draws what an eager one draws."""
import numpy as np
import pytest

import samp_cases as S
import samp_ext_ref as R
import test_sampler_gpu as T        # the families of small models (one per vocabulary, cached per process) and their helpers

pytestmark = pytest.mark.gpu

ODD_V = T.ODD.vocab


def _llm(V):
    llm = T._llm(V)
    llm.set_sampler_extensions(True)
    return llm


def _family(V):
    fam = T._family(V)
    for m in fam:
        m.set_sampler_extensions(True)
    return fam


def _bits(x):
    return np.float32(x).view(np.uint32)


def _untouched(llm, row):
    assert np.array_equal(llm._fetch_logits().view(np.uint32), row.view(np.uint32))       # no draw wrote to the row


def test_both_options_are_opt_in_per_handle():
    """a handle that never asked refuses both keywords as it always did, and its sampler stays the one in force"""
    from oracle import lm_ref
    V = 4096
    llm, row = _llm(V), S.BY_NAME["gaussian"].make(V)
    llm.set_sampler_extensions(False)
    try:
        llm.init_sampler_for_generate(top_k=20, top_p=1.0, min_p=0.0, temp=0.7, seed=2)
        for kw in (dict(typical_p=0.5), dict(mirostat_mode=2), dict(mirostat_mode=1)):
            with pytest.raises(NotImplementedError, match="typical_p / mirostat"):
                llm.init_sampler_for_generate(top_k=20, top_p=1.0, min_p=0.0, temp=0.7, seed=2, **kw)
        llm._put_logits(row)
        assert [llm.sample() for _ in range(4)] == [lm_ref.sample(row, 20, 1.0, 0.0, 0.7, 2, c) for c in range(4)]
    finally:
        llm.set_sampler_extensions(True)


# ---------------------------------------------------------------------------------------------- typical
@pytest.mark.parametrize("V", S.VOCABS)
@pytest.mark.parametrize("name", sorted(R.TYP_ROWS))
def test_typical_draws_match_restatement(name, V):
    """every row x top_k 2 / 40 / 256 x typical_p 0.2 / 0.5 / 0.9, with and without top_p / min_p behind the cut: 8 draws each, on the
    body of the last kernel the row is built to reach"""
    row = R.make(R.TYP_ROWS, name, V)
    llm = _llm(V)
    seed = 70
    for k in R.TYP_TOP_K:
        assert S.candidates(row, k)[1] == R.typ_body(name, V, k), (name, V, k)
        for tp in R.TYP_P:
            for top_p, min_p in R.TYP_BEHIND:
                seed += 1
                llm.init_sampler_for_generate(top_k=k, top_p=top_p, min_p=min_p, temp=R.TYP_TEMP, seed=seed, typical_p=tp)
                llm._put_logits(row)
                allowed, margin = R.typical_allowed(row, k, tp, top_p, min_p)
                allowed = set(allowed.tolist())
                for c in range(S.DRAWS):
                    t = llm.sample()
                    want = R.serial_sample(row, k, top_p, min_p, R.TYP_TEMP, seed, c, tp)
                    assert t == want, (k, tp, top_p, min_p, "draw", c, "device", t, "restatement", want)
                    if margin > 1.0:
                        assert t in allowed, (k, tp, top_p, min_p, c, t)
    _untouched(llm, row)


def test_typical_off_and_greedy_draw_what_they_drew():
    """typical_p 1.0, 0 (unset) and any value under temp <= 0 leave the serial chain alone: the oracle's tokens"""
    from oracle import lm_ref
    V = 4096
    llm, row = _llm(V), S.BY_NAME["gaussian"].make(V)
    for tp, cfg in ((1.0, (20, 0.9, 0.05, 0.7)), (0.0, (20, 0.9, 0.05, 0.7)), (0.5, (20, 0.9, 0.05, 0.0))):
        llm.init_sampler_for_generate(top_k=cfg[0], top_p=cfg[1], min_p=cfg[2], temp=cfg[3], seed=4, typical_p=tp)
        llm._put_logits(row)
        assert [llm.sample() for _ in range(6)] == [lm_ref.sample(row, *cfg, 4, c) for c in range(6)], tp


# ---------------------------------------------------------------------------------------------- mirostat
@pytest.mark.parametrize("V", R.MIRO_VOCABS)
@pytest.mark.parametrize("name", sorted(R.MIRO_ROWS))
@pytest.mark.parametrize("pen", (False, True))
def test_mirostat_draws_and_mu_match_restatement(name, V, pen):
    """32 consecutive draws at (tau, eta) = (5, 0.1) and (3, 1.0), temp 0.8 and 1.0: every token is the restatement's and mirostat_mu()
    is its float32 mu, bit for bit, after every draw; again with logit bias and penalties; vocabulary 1001 has ragged slices.  top_k,
    top_p, min_p and typical_p are set to values that would cut -- and are ignored."""
    row = R.make(R.MIRO_ROWS, name, V)
    llm = _llm(V)
    extra = R.MIRO_BIAS_PEN if pen else {}
    fn = R.seen_fn(row, **extra)
    for tau, eta, temp in R.MIRO_CONFIGS:
        llm.init_sampler_for_generate(top_k=3, top_p=0.5, min_p=0.3, typical_p=0.5, temp=temp, seed=R.MIRO_SEED, mirostat_mode=2, mirostat_tau=tau,
                                      mirostat_eta=eta, logit_bias=extra.get("bias"), **{k: v for k, v in extra.items() if k != "bias"})
        llm._put_logits(row)
        assert _bits(llm.mirostat_mu()) == _bits(2.0 * tau)
        toks, mus = R.mirostat_run(fn, temp, R.MIRO_SEED, tau, eta, R.MIRO_DRAWS)
        ref, _ = R.mirostat_reference(fn, temp, tau, eta, toks)
        same = True
        for c in range(R.MIRO_DRAWS):
            t = llm.sample()
            assert t == toks[c], (tau, eta, temp, "draw", c, "device", t, "restatement", toks[c])
            mu = llm.mirostat_mu()
            assert _bits(mu) == _bits(mus[c + 1]), (tau, eta, temp, "draw", c, "mu", mu, "restatement", float(mus[c + 1]))
            same = same and ref[c][2] > R.MIRO_MARGIN_MIN
            if same:
                assert t in set(ref[c][1].tolist()), (tau, eta, temp, c, t)
    _untouched(llm, row)


def test_second_init_restores_mu_and_the_draws():
    V = 4096
    llm, row = _llm(V), R.make(R.MIRO_ROWS, "zipf", V)
    kw = dict(top_k=0, top_p=1.0, min_p=0.0, temp=0.8, seed=12, mirostat_mode=2, mirostat_tau=5.0, mirostat_eta=0.1)
    runs = []
    for _ in range(2):
        llm.init_sampler_for_generate(**kw)
        assert llm.mirostat_mu() == 10.0
        llm._put_logits(row)
        runs.append([(llm.sample(), llm.mirostat_mu()) for _ in range(8)])
    assert runs[0] == runs[1] and len({m for _, m in runs[0]}) > 1
    llm.init_sampler_for_generate(top_k=20, top_p=1.0, min_p=0.0, temp=0.8, seed=12)       # init alone: both options off again
    from realtime_codec_agent_amd._native import RcaError
    with pytest.raises(RcaError, match="mirostat is off"):
        llm.mirostat_mu()


def test_library_refusals_name_the_value():
    llm = _llm(4096)
    lib = llm._lib
    llm.init_sampler_for_generate(top_k=0, top_p=1.0, min_p=0.0, temp=0.8, seed=1)
    for call, text in ((lambda: lib.rca_lm_sampler_set_typical(llm._h, 0.5), "typical_p 0.5 needs top_k in 1..256"),
                       (lambda: lib.rca_lm_sampler_set_typical(llm._h, -0.25), "typical_p -0.25"),
                       (lambda: lib.rca_lm_sampler_set_typical(llm._h, float("nan")), "typical_p nan"),
                       (lambda: lib.rca_lm_sampler_set_mirostat(llm._h, 1, 5.0, 0.1), "mirostat_mode 1"),
                       (lambda: lib.rca_lm_sampler_set_mirostat(llm._h, 3, 5.0, 0.1), "mirostat_mode 3"),
                       (lambda: lib.rca_lm_sampler_set_mirostat(llm._h, 2, -1.0, 0.1), "mirostat_tau -1"),
                       (lambda: lib.rca_lm_sampler_set_mirostat(llm._h, 2, 5.0, float("inf")), "mirostat_eta inf")):
        assert call() == -1       # RCA_ERR_ARG
        assert text in lib.rca_last_error().decode(), (text, lib.rca_last_error())
    assert lib.rca_lm_sampler_set_typical(llm._h, 0.5) != 0       # and a refusal leaves the sampler as it was: the oracle's tokens
    from oracle import lm_ref
    row = S.BY_NAME["gaussian"].make(4096)
    llm._put_logits(row)
    assert [llm.sample() for _ in range(4)] == [lm_ref.sample(row, 0, 1.0, 0.0, 0.8, 1, c) for c in range(4)]


# ---------------------------------------------------------------------------------------------- what rides on the draw counter
MIRO_KW = dict(top_k=40, top_p=0.95, min_p=0.05, temp=0.9, mirostat_mode=2, mirostat_tau=4.0, mirostat_eta=0.5)
TYP_KW = dict(top_k=256, top_p=0.95, min_p=0.0, temp=1.3, typical_p=0.5)


def _prepare(members, V, kws, graphs=True):
    for m, kw in zip(members, kws):
        m.set_graphs(graphs)
        m.reset()
        m.init_sampler_for_generate(**kw)
        m.eval(T._ids(V)[:12])


def _restore(fam, V):
    for m in fam:
        m.set_graphs(True)
        m.reset()
        m.eval(T._ids(V)[:12])


def _steps(llm, first_pair, users, n):
    toks, pair, mus = [], list(first_pair), []
    for i in range(n):
        t = llm.step(pair)
        toks.append(t)
        mus.append(llm.mirostat_mu())
        pair = [t, users[i]]
    return toks, mus


def _cut_at(toks):
    """(j, floor): a frame over these tokens with this audio_id_floor is cut by its step j, the latest step that can cut it"""
    for j in range(len(toks) - 2, -1, -1):
        if all(t > toks[j] for t in toks[:j]):
            return j, toks[j]
    raise AssertionError(toks)


def test_cut_frame_rewinds_mu():
    """a frame() that step j cuts leaves mirostat_mu(), the draw counter and the next token as j + 1 single step() calls on a twin do:
    the speculative steps behind the cut wrote their mu into ring slots the rewound counter no longer points at"""
    V = 4096
    fam, ids = _family(V), T._ids(V)
    try:
        a, b = fam[0], fam[1]
        kws = [dict(MIRO_KW, seed=33)] * 2
        _prepare([a, b], V, kws)
        users = ids[14:18]
        single, mus = _steps(b, ids[12:14], users, 4)
        j, floor = _cut_at(single)
        _prepare([b], V, kws)
        single, mus = _steps(b, ids[12:14], users, j + 1)
        got = a.frame(ids[12:14], users, floor)
        assert got == single and len(got) == j + 1 < 4
        assert _bits(a.mirostat_mu()) == _bits(mus[-1]) and a.n_tokens == b.n_tokens
        nxt = [single[-1], users[j]]
        assert a.step(nxt) == b.step(nxt) and _bits(a.mirostat_mu()) == _bits(b.mirostat_mu())
        assert len({_bits(m).item() for m in mus + [a.mirostat_mu()]}) > 1       # mu did move
    finally:
        _restore(fam, V)


def test_cut_batch_frame_rewinds_a_members_mu():
    """the same for a member of a LlamaBatch.frame, against batch steps of a batch of twins: the mirostat member has its own launches
    behind every pass, the other member the table kernels"""
    from realtime_codec_agent_amd.llm import LlamaBatch
    V = 4096
    fam, ids = _family(V), T._ids(V)
    kws = [dict(MIRO_KW, seed=34), dict(top_k=20, top_p=0.95, min_p=0.0, temp=1.3, seed=35)] * 2
    pairs, users = [ids[12:14], ids[20:22]], [ids[14:18], ids[22:26]]
    try:
        _prepare(fam[:4], V, kws)
        x, y = LlamaBatch(fam[0:2]), LlamaBatch(fam[2:4])
        try:
            cur, toks = [list(p) for p in pairs], [[], []]
            for i in range(4):
                out = y.step(cur)
                for s in range(2):
                    toks[s].append(out[s])
                cur = [[out[s], users[s][i]] for s in range(2)]
            j, floor = _cut_at(toks[0])       # (member 1 may be cut too, anywhere: a member's result does not depend on its companions)
            _prepare(fam[2:4], V, kws[2:])
            cur, mus = [list(p) for p in pairs], []
            for i in range(j + 1):
                out = y.step(cur)
                mus.append(fam[2].mirostat_mu())
                cur = [[out[s], users[s][i]] for s in range(2)]
            got, _ = x.frame(pairs, users, floor)
            assert got[0] == toks[0][:j + 1] and j + 1 < 4
            assert _bits(fam[0].mirostat_mu()) == _bits(mus[-1]) and fam[0].n_tokens == fam[2].n_tokens
            nxt = [toks[0][j], users[0][j]]
            assert fam[0].step(nxt) == fam[2].step(nxt) and _bits(fam[0].mirostat_mu()) == _bits(fam[2].mirostat_mu())
        finally:
            x.close()
            y.close()
    finally:
        _restore(fam, V)


@pytest.mark.parametrize("mode", ("mirostat", "typical"))
def test_graph_replay_draws_what_the_eager_path_draws(mode):
    """steps and a frame with set_graphs on and off: identical tokens (and mu); then a change of mode and back -- the captured graphs
    are dropped and captured again -- draws what a handle that never left the mode draws"""
    V = 4096
    fam, ids = _family(V), T._ids(V)
    kw = dict(MIRO_KW if mode == "mirostat" else TYP_KW, seed=36)
    other = dict(top_k=20, top_p=0.95, min_p=0.0, temp=1.3, seed=37)

    def run(llm, graphs, excursion):
        _prepare([llm], V, [kw], graphs)
        out, pair = [], ids[12:14]
        for i in range(3):
            t = llm.step(pair)
            out.append((t, llm.mirostat_mu() if mode == "mirostat" else None))
            pair = [t, ids[14 + i]]
        if excursion:       # another sampler on the same handle (its own graphs), then back
            llm.init_sampler_for_generate(**other)
            llm.step(pair)
            _prepare([llm], V, [kw], graphs)
            pair = ids[12:14]
            again = []
            for i in range(3):
                t = llm.step(pair)
                again.append((t, llm.mirostat_mu() if mode == "mirostat" else None))
                pair = [t, ids[14 + i]]
            assert again == out
        out.append(tuple(llm.frame(pair, ids[20:24], -1)))
        return out

    try:
        base = run(fam[0], False, False)
        assert run(fam[0], True, False) == base
        assert run(fam[1], True, True) == base
        assert len({t for t, _ in base[:3]} | set(base[3])) > 1
    finally:
        _restore(fam, V)


# ---------------------------------------------------------------------------------------------- chi-square on the device
@pytest.mark.parametrize("mode", ("typical", "mirostat"))
def test_device_draws_pass_chi_square(mode):
    """4096 device draws from samp_cases' 8-token row are the restatement's and pass the 1 - 1e-4 quantile of chi-square against the
    float64 distribution over the float64 allowed set (typical: a fixed row; mirostat: eta = 0, so that mu and the set stand still)"""
    V = S.CHI_V
    llm, row = _llm(V), S.chi_row(S.CHI_V)
    if mode == "typical":
        k, tp = R.CHI_TYP["top_k"], R.CHI_TYP["typical_p"]
        llm.init_sampler_for_generate(top_k=k, top_p=1.0, min_p=0.0, temp=S.CHI_TEMP, seed=S.CHI_SEED, typical_p=tp)
        want = [R.serial_sample(row, k, 1.0, 0.0, S.CHI_TEMP, S.CHI_SEED, c, tp) for c in range(S.CHI_DRAWS)]
        allowed, margin = R.typical_allowed(row, k, tp, 1.0, 0.0)
        assert margin > 1.0
    else:
        tau = R.CHI_MIRO["tau"]
        llm.init_sampler_for_generate(top_k=0, top_p=1.0, min_p=0.0, temp=S.CHI_TEMP, seed=S.CHI_SEED, mirostat_mode=2, mirostat_tau=tau, mirostat_eta=0.0)
        want, _ = R.mirostat_run(R.seen_fn(row), S.CHI_TEMP, S.CHI_SEED, tau, 0.0, S.CHI_DRAWS)
        ref, _ = R.mirostat_reference(R.seen_fn(row), S.CHI_TEMP, tau, 0.0, want[:1])
        allowed, margin = ref[0][1], ref[0][2]
        assert margin > R.MIRO_MARGIN_MIN
    llm._put_logits(row)
    got = [llm.sample() for _ in range(S.CHI_DRAWS)]
    assert got == want
    chi = R.chi_square(got, row, allowed, S.CHI_TEMP)
    bound = R.CHI_QUANTILE[len(allowed) - 1]
    print(f"chi-square on the device, {mode}: {chi:.2f} over {len(allowed)} tokens (bound {bound})")
    assert chi < bound and sorted(set(got)) == sorted(allowed.tolist())
