"""The device sampler and rca_lm_token_probs on hand-made logit rows (tests/samp_cases.py), uploaded through the tests-only
rca_lm_put_logits: every body of the serial chain's last kernel (count / sort / scan), both caps between them, the whole-vocabulary
and the big path, ties, infinities, denormals and signed zeros -- token for token against oracle/sampler_oracle.c, and against the
float64 allowed set where its cuts are clear of every token's mass (tests/test_sampler_cpu.py holds the restatement itself to the
float64 references).  A random-init model's near-Gaussian logits only ever reach the count body; the rows here are what reaches the
others.  Every serial-path case first asserts, from the row it is about to upload, the body it is meant to reach."""
import functools

import numpy as np
import pytest

import lm_shape_cases as sc
import samp_cases as S
from oracle import lm_ref

pytestmark = pytest.mark.gpu

ODD = sc.BY_NAME[S.ODD_SHAPE]
ODD_ROWS = tuple(r.name for r in S.ROWS if not r.name.startswith("cap_"))     # a cap row needs more than 1001 tokens
# (vocabulary, lm_head rows [0, n) zeroed): the masked models' own logits reach the sort and the scan body inside graphs
MASKED = {4096: 3700, 8192: 8186}
FAMILY = 6


@functools.lru_cache(maxsize=None)
def _family(V):
    """one small bf16 model per vocabulary (2 layers, hidden 512) and five twins over its weights, every handle after an eval"""
    from realtime_codec_agent_amd.llm import LlamaForAlternatingCodeChannels as L, LMConfig
    if V == ODD.vocab:
        fam = [L(model_path=f"random:{ODD.name}", config=ODD.config(), n_ctx=256, random_seed=ODD.seed, init_std=sc.INIT_STD, device=0)]
    else:
        cfg = LMConfig(vocab_size=V, hidden=512, n_layers=2, n_heads=8, n_kv_heads=2, head_dim=64, ffn=1024)
        parent = L(model_path="random:mid", config=cfg, n_ctx=512, random_seed=3, init_std=0.05, device=0)
        parent.mask_head_rows(0, MASKED[V])
        fam = [parent] + [L(n_ctx=512, share_weights_with=parent, device=0) for _ in range(FAMILY - 1)]
    for m in fam:
        m.eval(_ids(V)[:12])
    return fam


def _ids(V):
    return np.random.default_rng(4).integers(0, V, 80).tolist()


def _llm(V):
    llm = _family(V)[0]
    if llm.n_tokens != 12:
        llm.reset()
        llm.eval(_ids(V)[:12])
    return llm


def _sampler(llm, cfg, seed, bias=None, **pen):
    top_k, top_p, min_p, temp = cfg
    llm.init_sampler_for_generate(top_k=top_k, top_p=top_p, min_p=min_p, temp=temp, seed=seed, logit_bias=bias, **pen)


def _assert_body(row, cfg, V, body):
    """the serial chain's list for this row and configuration selects the body the case is about"""
    if S.path(cfg[0], cfg[1], cfg[3], V) == "serial":
        n, got = S.candidates(row, S.serial_k(cfg[0], cfg[3], V))
        assert got == body, (cfg, n, got, body)


def _check_draws(llm, row, cfg, seed, V, first=0, n=S.DRAWS):
    """n draws from the uploaded row equal the restatement's, and lie in the float64 allowed set where its margin is positive"""
    top_k, top_p, min_p, temp = cfg
    allowed, margin = S.allowed_set(row, top_k, top_p, min_p, greedy=temp <= 0.0)
    allowed = set(allowed.tolist())
    for c in range(first, first + n):
        t = llm.sample()
        want = lm_ref.sample(row, top_k, top_p, min_p, temp, seed, c)
        assert t == want, (cfg, "draw", c, "device", t, "restatement", want)
        if margin > S.MARGIN_MIN:
            assert t in allowed, (cfg, "draw", c, t)


# ---------------------------------------------------------------------------------------------- token for token, every row
def _row_cases():
    return S.ROW_VOCABS + tuple((n, ODD.vocab) for n in ODD_ROWS)


@pytest.mark.parametrize("name,V", _row_cases())
def test_draws_match_restatement_on_every_row(name, V):
    """every row x the fixed list of configurations (serial chain at top_k 1 / 20 / 256, whole vocabulary, big path): 8 draws each"""
    r = S.BY_NAME[name]
    row = r.make(V)
    llm = _llm(V)
    for i, cfg in enumerate(S.configs(V)):
        if S.path(cfg[0], cfg[1], cfg[3], V) == "serial":
            _assert_body(row, cfg, V, r.body(V, S.serial_k(cfg[0], cfg[3], V)))
        _sampler(llm, cfg, 40 + i)
        llm._put_logits(row)
        _check_draws(llm, row, cfg, 40 + i, V)
    assert np.array_equal(llm._fetch_logits().view(np.uint32), row.view(np.uint32))       # no draw wrote to the row


def test_signed_zeros_tie_by_lowest_index():
    """-0.0 and +0.0 are one value: ties between them rank by the lowest index like any other tie.  The greedy draw from a row whose
    maximum is -0.0 at index 3 and +0.0 at index V - 5 is 3; the rank cut of top_k 20 through six zeros keeps the four lowest indices
    whatever their signs; the raw logits keep their signs."""
    V = 8192
    llm = _llm(V)
    row = S.BY_NAME["signed_zero_top"].make(V)
    assert np.signbit(row[3]) and not np.signbit(row[V - 5]) and row[3] == row[V - 5] == row.max()
    for cfg in ((1, 1.0, 0.0, 0.7), (20, 1.0, 0.0, 0.0), (0, 1.0, 0.0, 0.0)):
        _sampler(llm, cfg, 1)
        llm._put_logits(row)
        assert llm.sample() == 3 == lm_ref.sample(row, *cfg, 1, 0)
    two = np.full(V, -1.0, np.float32)
    two[0], two[1] = -0.0, 0.0
    _sampler(llm, (5, 1.0, 0.0, 0.0), 1)
    llm._put_logits(two)
    assert llm.sample() == 0
    assert np.array_equal(llm._fetch_logits().view(np.uint32), two.view(np.uint32))
    row = S.BY_NAME["signed_zero_cut"].make(V)
    zeros = set(np.nonzero(row == 0)[0].tolist())
    assert zeros == {10, 11, 12, V - 4, V - 3, V - 2}
    # serial chain: 16 values above the zeros, top_k 20; big path: 254 values above them, top_k 257 -- the rank cut goes through the zeros
    for cfg, seed, row, kept, n in (((20, 1.0, 0.0, 1.5), 2, row, {10, 11, 12, V - 4}, 48),
                                    ((257, 1.0, 0.0, 1.5), 3, S.signed_zero_cut(V, 28, n_top=254), {10, 11, 12}, 256)):
        assert S.allowed_set(row, *cfg[:3])[0].size == cfg[0] and kept <= set(S.allowed_set(row, *cfg[:3])[0].tolist())
        _sampler(llm, cfg, seed)
        llm._put_logits(row)
        seen = set()
        for c in range(n):
            t = llm.sample()
            assert t == lm_ref.sample(row, *cfg, seed, c), (cfg, c)
            assert t not in zeros - kept, (cfg, c, t)
            seen.add(t)
        assert seen & kept, cfg          # the zeros really are drawn


# ---------------------------------------------------------------------------------------------- the tail leaves no state
def test_tail_leaves_no_state_between_bodies_and_paths():
    """One sampler, one handle: a draw from a scan-body row (overflow flag set, list counter past the cap), then from a sort-body row,
    each followed by draws from a count-body row that must still match -- the last kernel re-zeroes the histogram, the list counter and
    the overflow flag.  Then the same across a switch from the big path (whose radix histograms must be zero again) to the serial one."""
    V = 8192
    llm = _llm(V)
    cfg, seed = (20, 0.9, 0.0, 0.7), 7
    plain = S.BY_NAME["gaussian"].make(V)
    _sampler(llm, cfg, seed)
    c = 0
    for name, body in (("shifted_up", "scan"), ("cap_4096", "sort"), ("cap_4097", "scan"), ("cap_1025", "sort"), ("all_equal", "scan")):
        row = S.BY_NAME[name].make(V)
        _assert_body(row, cfg, V, body)
        llm._put_logits(row)
        _check_draws(llm, row, cfg, seed, V, first=c, n=2)
        _assert_body(plain, cfg, V, "count")
        llm._put_logits(plain)
        _check_draws(llm, plain, cfg, seed, V, first=c + 2, n=3)
        c += 5
    for big in ((5000, 0.9, 0.0, 0.7), (0, 0.02, 0.0, 1.5), (300, 1.0, 0.0, 0.7)):
        for name in ("shifted_up", "gaussian"):
            row = S.BY_NAME[name].make(V)
            _sampler(llm, big, 8)
            llm._put_logits(row)
            _check_draws(llm, row, big, 8, V, n=3)
            _sampler(llm, cfg, 9)
            llm._put_logits(plain)
            _check_draws(llm, plain, cfg, 9, V, n=3)
            _sampler(llm, (0, 1.0, 0.0, 0.7), 10)           # and the plain whole-vocabulary sampler, which borrows the histogram area
            llm._put_logits(row)
            _check_draws(llm, row, (0, 1.0, 0.0, 0.7), 10, V, n=2)
            _sampler(llm, cfg, 11)
            llm._put_logits(plain)
            _check_draws(llm, plain, cfg, 11, V, n=2)


PEN = dict(repeat_penalty=1.3, frequency_penalty=0.25, presence_penalty=0.15)


def _patch_row(base, V):
    """a row for the patch tests: every logit negative but token A, exactly 0.0 and the maximum; B the best of the negative ones;
    C the next; LOW the lowest"""
    row = S.BY_NAME[base].make(V)
    row = -np.abs(row) - np.float32(0.01)
    a = 1234
    row[a] = 0.0
    order = np.argsort(-row, kind="stable")
    return row, a, int(order[1]), int(order[2]), int(order[-1])


def _rank(v, t):
    return int((v > v[t]).sum())


def _accept(llm, V, tokens):
    """make the sampler accept `tokens`: each is drawn from a row on which it is the only candidate with any mass"""
    for t in tokens:
        peak = np.full(V, -1000.0, np.float32)
        peak[t] = 1000.0
        llm._put_logits(peak)
        assert llm.sample() == t


@pytest.mark.parametrize("base,body", (("shifted_down", "scan"), ("gaussian", "count")))
@pytest.mark.parametrize("what", ("lift", "remove_max", "penalty", "all"))
def test_patches_that_cross_the_threshold(base, body, what):
    """A +50 bias lifts the lowest token of the row into the top k, a -inf bias removes the maximum, a repeat penalty (with frequency
    and presence terms) hits an accepted token at exactly 0.0 -- the maximum -- and an accepted negative one; "all" = the lift, the
    penalties and a -inf bias on the best token the penalties leave.  The sampler sees the patched row, the histogram, the list and
    the scan included, and the caller's row is back bit for bit afterwards."""
    V = 8192
    llm = _llm(V)
    row, a, b, c3, low = _patch_row(base, V)
    bias = {"lift": {low: 50.0}, "remove_max": {a: -np.inf}, "penalty": {}, "all": {low: 50.0, c3: -np.inf}}[what]
    pen = PEN if what in ("penalty", "all") else {}
    hist = [a, b, a] if pen else []
    cfg, seed = (20, 1.0, 0.0, 0.7), 21
    seen = S.penalised(row, bias, hist, pen.get("repeat_penalty", 1.0), pen.get("frequency_penalty", 0.0), pen.get("presence_penalty", 0.0))
    _assert_body(seen, cfg, V, body)
    assert _rank(row, a) == 0 and _rank(row, b) == 1 and _rank(row, low) == V - 1 and row[b] < 0
    if what in ("lift", "all"):
        assert _rank(seen, low) < 2
    if what == "remove_max":
        assert _rank(seen, b) == 0 and seen[a] == -np.inf
    if what in ("penalty", "all"):
        assert seen[a] == np.float32(-0.65) and seen[b] == row[b] * np.float32(1.3) - np.float32(0.4) and _rank(seen, b) > 1
    if what == "all":
        assert seen[c3] == -np.inf
    _sampler(llm, cfg, seed, bias=bias or None, **pen)
    _accept(llm, V, hist)
    for c in range(len(hist), len(hist) + 6):
        llm._put_logits(row)
        t = llm.sample()
        want = lm_ref.sample(row, *cfg, seed, c, bias or None, prev_tokens=hist, **pen)
        assert t == want, (what, c, t, want)
        assert np.array_equal(llm._fetch_logits().view(np.uint32), row.view(np.uint32)), (what, c)
        hist.append(t)
    # greedy: the patched maximum
    _sampler(llm, (20, 1.0, 0.0, 0.0), seed, bias=bias or None)
    llm._put_logits(row)
    nb = S.penalised(row, bias, [], 1.0, 0.0, 0.0)
    assert llm.sample() == int(np.argsort(-nb, kind="stable")[0])


def test_penalised_draw_on_a_scan_row_restores_the_logits():
    V = 8192
    llm = _llm(V)
    row = S.BY_NAME["shifted_up"].make(V)
    cfg, seed, bias = (20, 0.9, 0.0, 1.5), 5, {int(row.argmax()): -np.inf, int(row.argmin()): 50.0, 17: -3.0}
    _sampler(llm, cfg, seed, bias=bias, **PEN)
    hist = []
    llm._put_logits(row)
    for c in range(6):                                   # no re-upload: every draw must find the raw row its predecessor left
        _assert_body(S.penalised(row, bias, hist, 1.3, 0.25, 0.15), cfg, V, "scan")
        t = llm.sample()
        assert t == lm_ref.sample(row, *cfg, seed, c, bias, prev_tokens=hist, **PEN), c
        hist.append(t)
    assert np.array_equal(llm._fetch_logits().view(np.uint32), row.view(np.uint32))


# ---------------------------------------------------------------------------------------------- chi-square on the device
@pytest.mark.parametrize("path", sorted(S.CHI_CONFIGS))
def test_device_draws_pass_chi_square(path):
    """the device's 4096 draws from the 8-token support are the restatement's, and pass the bound the restatement passes"""
    V = S.CHI_V
    llm = _llm(V)
    top_k, top_p = S.CHI_CONFIGS[path]
    _sampler(llm, (top_k, top_p, 0.0, S.CHI_TEMP), S.CHI_SEED)
    llm._put_logits(S.chi_row(V))
    got = [llm.sample() for _ in range(S.CHI_DRAWS)]
    want = S.chi_reference(path)
    assert got == list(want)
    chi = S.chi_square(got, V)
    print(f"chi-square on the device, {path} path: {chi:.2f} (bound {S.CHI_BOUND})")
    assert chi < S.CHI_BOUND and sorted(set(got)) == S.chi_support(V).tolist()


# ---------------------------------------------------------------------------------------------- the same bodies inside graphs and the table kernels
def _prepare(members, V, samplers):
    for m, p in zip(members, samplers):
        m.set_graphs(True)
        m.reset()
        m.init_sampler_for_generate(**p)
        m.eval(_ids(V)[:12])


def _check_member(llm, p, counter, tok, V, body, hist):
    lg = llm._scores[-1]
    n, got = S.candidates(lg, S.serial_k(p["top_k"], p["temp"], V))
    assert got == body, (n, got, body)
    want = lm_ref.sample(lg, p["top_k"], p["top_p"], p["min_p"], p["temp"], p["seed"], counter,
                         repeat_penalty=p.get("repeat_penalty", 1.0), prev_tokens=hist)
    assert tok == want, (p, counter, tok, want)


@pytest.mark.parametrize("V,top_k,body", ((4096, 256, "sort"), (8192, 20, "scan")))
def test_sort_and_scan_bodies_inside_graphs_and_table_kernels(V, top_k, body):
    """A model whose head rows are almost all zeroed produces the rows itself: thousands of logits exactly 0.0 below a few positive
    ones put the k-th best into the zero bin, the list holds the whole tie group, and the rank cut falls inside it.  A graph-replayed
    step, a frame graph, a group step and a batch step over 6 twins (the table forms of the sampler's kernels): every token is the
    restatement's draw from the logits read back, and the read-back logits select the body this case names."""
    from realtime_codec_agent_amd.llm import LlamaBatch, LlamaGroup
    fam = _family(V)
    ids = _ids(V)
    base = dict(top_k=top_k, top_p=0.95, min_p=0.0, temp=1.3)
    samplers = [dict(base, seed=60 + s, **({"repeat_penalty": 1.3} if s == 1 else {})) for s in range(FAMILY)]
    try:
        # graph-replayed steps on one handle
        llm, p = fam[0], samplers[0]
        _prepare(fam[:1], V, samplers)
        toks, single = ids[12:14], []
        for step in range(4):
            t = llm.step(toks)
            _check_member(llm, p, step, t, V, body, [])
            single.append(t)
            toks = [t, ids[14 + step]]
        assert int((llm._scores[-1] == 0).sum()) >= MASKED[V] and len(set(single)) > 1
        # the frame graph: the same four steps with the token fed back on the device
        _prepare(fam[:1], V, samplers)
        assert llm.frame(ids[12:14], ids[14:18], -1) == single
        # a group step of two members, then batch steps of all six
        _prepare(fam, V, samplers)
        hist = [[] for _ in fam]
        grp = LlamaGroup(fam[1:3])
        try:
            for step in range(2):
                out = grp.step([ids[20 + 2 * step:22 + 2 * step], ids[30 + 2 * step:32 + 2 * step]])
                for s in (1, 2):
                    _check_member(fam[s], samplers[s], step, out[s - 1], V, body, hist[s])
                    hist[s].append(out[s - 1])
        finally:
            grp.close()
        bat = LlamaBatch(fam)
        try:
            for step in range(3):
                out = bat.step([[ids[40 + s + step], ids[50 + s + step]] for s in range(FAMILY)])
                for s in range(FAMILY):
                    _check_member(fam[s], samplers[s], len(hist[s]), out[s], V, body, hist[s])
                    hist[s].append(out[s])
        finally:
            bat.close()
    finally:
        for m in fam:
            m.reset()
            m.eval(ids[:12])


# ---------------------------------------------------------------------------------------------- token_probs on uploaded rows
def _probs_rows(V):
    per = -(-V // 64)
    g = S.BY_NAME["gaussian"].make(V)
    holes = g.copy()
    for s in (0, 3, 4, 31, 63):
        holes[s * per:(s + 1) * per] = -np.inf
    peaked = S.BY_NAME["peaked"].make(V)
    edges = [0, V - 1, per - 1, per, 3 * per - 1, 3 * per, 5 * per - 1, 5 * per, 31 * per, 32 * per, min(63 * per, V - 2), int(peaked.argmax())]
    return {"holes": holes, "shifted": g + np.float32(1e4), "peaked": peaked, "gaussian": g}, sorted(set(i for i in edges if 0 <= i < V))


@pytest.mark.parametrize("V", (8192, ODD.vocab))
def test_token_probs_on_uploaded_rows(V):
    """softmax(row)[ids] against float64 at the absolute 1e-6 of the model-logits test: whole slices of the vocabulary at -inf (a
    slice's maximum is then -inf and its sum undefined: it must count as nothing), a vocabulary that 64 slices do not divide (the last
    slice is short or empty), logits near 1e4, a peaked row; first and last token, slice edges, and -inf tokens, whose probability is
    exactly 0."""
    llm = _llm(V)
    rows, ids = _probs_rows(V)
    for name, row in rows.items():
        llm._put_logits(row)
        got = llm.token_probs(ids)
        v = row.astype(np.float64)
        p = np.exp(v - v.max())
        p /= p.sum()
        assert np.isfinite(got).all() and np.abs(got - p[ids]).max() < 1e-6, (name, np.abs(got - p[ids]).max())
        dead = [i for i, t in enumerate(ids) if row[t] == -np.inf]
        assert (got[dead] == 0).all()
        if name == "holes":
            assert len(dead) >= 3
        if name == "peaked":
            assert got[ids.index(int(row.argmax()))] > 1 - 1e-6


# ---------------------------------------------------------------------------------------------- refusals
def test_put_logits_refusals():
    from realtime_codec_agent_amd import _native as N
    from realtime_codec_agent_amd.llm import LlamaForAlternatingCodeChannels as L
    llm = L(model_path=f"random:{ODD.name}", config=ODD.config(), n_ctx=64, random_seed=ODD.seed, init_std=sc.INIT_STD, device=0)
    row = np.zeros(ODD.vocab, np.float32)
    with pytest.raises(N.RcaError, match="no logits: call eval first"):
        llm._put_logits(row)
    llm.eval([1, 2, 3])
    for bad in (np.zeros(ODD.vocab - 1, np.float32), np.zeros(ODD.vocab + 1, np.float32), np.zeros((1, ODD.vocab), np.float32)):
        with pytest.raises(ValueError, match="_put_logits"):
            llm._put_logits(bad)
    before = llm._fetch_logits().copy()
    row[5] = 3.0
    llm._put_logits(row)
    assert np.array_equal(llm._fetch_logits(), row) and not np.array_equal(before, row)
    assert np.array_equal(llm._scores[-1], row) and llm.n_tokens == 3
    llm.init_sampler_for_generate(top_k=1, top_p=1.0, min_p=0.0, temp=0.0, seed=1)
    assert llm.sample() == 5
    llm.reset()
    with pytest.raises(N.RcaError, match="no logits: call eval first"):
        llm._put_logits(row)
    llm.close()
