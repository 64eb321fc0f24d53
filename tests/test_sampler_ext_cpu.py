"""typical_p and mirostat v2 without a GPU: the float32 restatement of tests/samp_ext_ref.py (the definition of what the device
draws) against the plain float64 references beside it, its primitives against the oracle library and libm, options off against
oracle/sampler_oracle.c, and the refusals of init_sampler_for_generate over a fake library."""
import ctypes as C
import ctypes.util

import numpy as np
import pytest

import samp_cases as S
import samp_ext_ref as R
from oracle import lm_ref


# ---------------------------------------------------------------------------------------------- primitives
def test_vector_primitives_are_the_oracles():
    lib = R._olib()
    rng = np.random.default_rng(1)
    seeds, ctrs = rng.integers(0, 1 << 63, 256, dtype=np.uint64), rng.integers(0, 1 << 63, 256, dtype=np.uint64)
    assert R.splitmix(seeds, ctrs).tolist() == [lib.oracle_splitmix(int(s), int(c)) for s, c in zip(seeds, ctrs)]
    libm = C.CDLL(ctypes.util.find_library("m"))
    libm.fmaf.restype = C.c_float
    libm.fmaf.argtypes = [C.c_float] * 3
    a = (30.0 * rng.standard_normal(20000)).astype(np.float32)
    b = np.where(rng.random(20000) < 0.5, np.float32(1.0) / np.float32(0.8), rng.standard_normal(20000)).astype(np.float32)
    c = (3.0 * rng.standard_normal(20000)).astype(np.float32)
    want = np.array([libm.fmaf(float(x), float(y), float(z)) for x, y, z in zip(a, b, c)], np.float32)
    assert np.array_equal(R.fmaf(a, b, c).view(np.uint32), want.view(np.uint32))
    assert R.expf(np.float32(-np.inf)) == 0 and R.expf(np.float32(0.0)) == 1 and R.logf(np.float32(1.0)) == 0


def test_margins_are_the_derived_ones():
    """the constants the GPU test relies on, restated from the derivations in samp_ext_ref.py"""
    assert R.TYP_S_MARGIN >= 2 * (5.6 * (256 * 2.0 ** -24 + 3 * 2.0 ** -23) + 4e-6)
    assert R.TYP_MASS_MARGIN == S.MARGIN_MIN >= 256 * 2.0 ** -23 + 2.0 ** -22
    assert R.MIRO_DRAW_ERR >= 2 * 1.4427 * (3 * 2.0 ** -18 + 2.0 ** -22 + 8192 * 2.0 ** -40 + 2.0 ** -24)
    assert R.MIRO_MARGIN_MIN >= R.MIRO_DRAWS * R.MIRO_DRAW_ERR


# ---------------------------------------------------------------------------------------------- options off
@pytest.mark.parametrize("name,V", S.ROW_VOCABS)
def test_options_off_reproduce_the_oracle(name, V):
    """typical_p 1.0 and 0 (unset): the serial chain is oracle/sampler_oracle.c's, token for token, on every row of samp_cases"""
    row = S.BY_NAME[name].make(V)
    for i, cfg in enumerate(S.SERIAL_CONFIGS):
        for c in range(S.DRAWS):
            want = lm_ref.sample(row, *cfg, 40 + i, c)
            assert R.serial_sample(row, *cfg, 40 + i, c) == want == R.serial_sample(row, *cfg, 40 + i, c, typical_p=0.0), (cfg, c)


def test_mirostat_with_nothing_to_cut_is_the_whole_vocabulary_sampler():
    """eta = 0 and a mu above every surprise: the kept set is every token with any mass and the draw is the oracle's top_k = 0 draw"""
    for name in ("gaussian", "shifted_down", "neg_inf_but_3"):
        row = S.BY_NAME[name].make(4096)
        for c in range(16):
            tok, mu, _ = R.mirostat_draw(row, 0.7, 9, c, 250.0, 125.0, 0.0)
            assert tok == lm_ref.sample(row, 0, 1.0, 0.0, 0.7, 9, c) and mu == 250.0


# ---------------------------------------------------------------------------------------------- typical against float64
def test_typical_rows_are_what_they_say():
    for V in S.VOCABS:
        for name in R.TYP_ROWS:
            row = R.make(R.TYP_ROWS, name, V)
            for k in R.TYP_TOP_K:
                assert S.candidates(row, k)[1] == R.typ_body(name, V, k), (name, V, k)
        assert {R.typ_body(n, V, k) for n in R.TYP_ROWS for k in R.TYP_TOP_K} >= ({"count", "sort"} | ({"scan"} if V == 8192 else set()))
        two = R.make(R.TYP_ROWS, "two_level", V)
        top = int(two.argmax())
        for tp in (0.2, 0.5):       # the typical set leaves the argmax out -- what no top_p does
            assert top not in R.typical_allowed(two, 40, tp, 1.0, 0.0)[0]
        assert top in R.typical_allowed(two, 40, 0.9, 1.0, 0.0)[0]
        assert R.typical_allowed(R.make(R.TYP_ROWS, "peaked", V), 256, 0.9, 1.0, 0.0)[0].size == 1
        inf_row = R.make(R.TYP_ROWS, "neg_inf_tail", V)
        assert np.isinf(np.sort(inf_row)[::-1][:256]).sum() == 156


@pytest.mark.parametrize("V", S.VOCABS)
@pytest.mark.parametrize("name", sorted(R.TYP_ROWS))
def test_typical_draws_lie_in_the_float64_allowed_set(name, V):
    row = R.make(R.TYP_ROWS, name, V)
    for k in R.TYP_TOP_K:
        for tp in R.TYP_P:
            for top_p, min_p in R.TYP_BEHIND:
                allowed, margin = R.typical_allowed(row, k, tp, top_p, min_p)
                if name in R.TYP_CLEAR_ROWS:        # the rows meant for this check: none may be skipped
                    assert margin > 1.0, (k, tp, top_p, min_p, margin)
                if margin > 1.0:
                    allowed = set(allowed.tolist())
                    for c in range(S.DRAWS):
                        t = R.serial_sample(row, k, top_p, min_p, R.TYP_TEMP, 5, c, tp)
                        assert t in allowed, (k, tp, top_p, min_p, c, t)


def test_flat_row_ties_go_by_index():
    """every s ties: the typical set is the lowest-ranked candidates, i.e. the lowest indices; exactly half the mass is not enough"""
    row = R.make(R.TYP_ROWS, "flat", 4096)
    kept = R.typical_cut(np.full(40, 0.5, np.float32), 0.5)
    assert kept.tolist() == list(range(21))
    assert {R.serial_sample(row, 40, 1.0, 0.0, 0.8, 3, c, 0.5) for c in range(200)} == set(range(21))


# ---------------------------------------------------------------------------------------------- mirostat against float64
@pytest.mark.parametrize("V", R.MIRO_VOCABS)
@pytest.mark.parametrize("name", sorted(R.MIRO_ROWS))
@pytest.mark.parametrize("pen", (False, True))
def test_mirostat_against_the_float64_trajectory(name, V, pen):
    """32 draws per configuration: where the margin is clear the draw lies in the float64 set, and up to the first unclear draw the
    float32 mu stays within the derived bound of the float64 trajectory along the same tokens.  On the rows meant for the check every
    draw is clear."""
    row = R.make(R.MIRO_ROWS, name, V)
    fn = R.seen_fn(row, **(R.MIRO_BIAS_PEN if pen else {}))
    for tau, eta, temp in R.MIRO_CONFIGS:
        toks, mus = R.mirostat_run(fn, temp, R.MIRO_SEED, tau, eta, R.MIRO_DRAWS)
        ref, _ = R.mirostat_reference(fn, temp, tau, eta, toks)
        same = True
        for j, (tok, (mu64, allowed, margin)) in enumerate(zip(toks, ref)):
            if same:
                assert abs(float(mus[j]) - mu64) <= R.miro_mu_bound(j, eta), (tau, eta, temp, j, mus[j], mu64)
            if margin > R.MIRO_MARGIN_MIN:
                if same:
                    assert tok in set(allowed.tolist()), (tau, eta, temp, j, tok)
            else:
                assert name not in R.MIRO_CLEAR_ROWS or pen, (name, V, tau, eta, temp, j, margin)
                same = False


def test_mirostat_rows_are_what_they_say():
    for V in R.MIRO_VOCABS:
        for tau, eta, temp in R.MIRO_CONFIGS:
            row = R.make(R.MIRO_ROWS, "climb", V)
            toks, mus = R.mirostat_run(R.seen_fn(row), temp, R.MIRO_SEED, tau, eta, R.MIRO_DRAWS)
            sizes = [len(R.mirostat_draw(row, temp, R.MIRO_SEED, c, mus[c], tau, eta)[2]) for c in range(R.MIRO_DRAWS)]
            assert max(float(m) for m in mus) > 17.0 and sizes[0] == 1 and max(sizes) > V // 2, (V, tau, eta, temp, max(mus), max(sizes))
            assert any(1 < s < V // 2 for s in sizes) or eta == 1.0       # the kept set grows through the slices at the slow rate
            row = R.make(R.MIRO_ROWS, "fall", V)
            toks, mus = R.mirostat_run(R.seen_fn(row), temp, R.MIRO_SEED, tau, eta, R.MIRO_DRAWS)
            if eta == 1.0:
                sizes = [len(R.mirostat_draw(row, temp, R.MIRO_SEED, c, mus[c], tau, eta)[2]) for c in range(R.MIRO_DRAWS)]
                assert min(sizes) == 1 and min(float(m) for m in mus) < mus[0]
            row = R.make(R.MIRO_ROWS, "spike", V)
            toks, mus = R.mirostat_run(R.seen_fn(row), temp, R.MIRO_SEED, tau, eta, 4)
            assert set(toks) == {int(row.argmax())} and float(mus[1]) == float(np.float32(2 * tau) + np.float32(eta) * np.float32(tau))


# ---------------------------------------------------------------------------------------------- chi-square of the restatement
def test_restatement_passes_chi_square():
    row = S.chi_row(S.CHI_V)
    allowed, margin = R.typical_allowed(row, R.CHI_TYP["top_k"], R.CHI_TYP["typical_p"], 1.0, 0.0)
    assert margin > 1.0 and 2 <= len(allowed) <= 8 and set(allowed.tolist()) <= set(S.chi_support(S.CHI_V).tolist())
    toks = [R.serial_sample(row, R.CHI_TYP["top_k"], 1.0, 0.0, S.CHI_TEMP, S.CHI_SEED, c, R.CHI_TYP["typical_p"]) for c in range(S.CHI_DRAWS)]
    assert R.chi_square(toks, row, allowed, S.CHI_TEMP) < R.CHI_QUANTILE[len(allowed) - 1]
    fn = R.seen_fn(row)
    toks, mus = R.mirostat_run(fn, S.CHI_TEMP, S.CHI_SEED, R.CHI_MIRO["tau"], 0.0, S.CHI_DRAWS)
    ref, _ = R.mirostat_reference(fn, S.CHI_TEMP, R.CHI_MIRO["tau"], 0.0, toks[:1])
    _, allowed, margin = ref[0]
    assert margin > R.MIRO_MARGIN_MIN and 2 <= len(allowed) <= 8 and all(float(m) == 2 * R.CHI_MIRO["tau"] for m in mus)
    assert R.chi_square(toks, row, allowed, S.CHI_TEMP) < R.CHI_QUANTILE[len(allowed) - 1]


# ---------------------------------------------------------------------------------------------- the Python surface over a fake library
class _FakeLib:
    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def call(*a):
            self.calls.append((name,) + tuple(a[1:]))
            if name == "rca_lm_sampler_get_mirostat_mu":
                a[1]._obj.value = 7.5
            return 0
        return call


def _fake_llm():
    from realtime_codec_agent_amd.llm import LlamaForAlternatingCodeChannels as L
    llm = L.__new__(L)
    llm._lib, llm._h, llm._seed, llm._sampler, llm._sampler_params = _FakeLib(), C.c_void_p(), 0, None, None
    llm._sampler_ext = True        # what set_sampler_extensions(True) leaves
    return llm


def test_options_are_refused_until_the_handle_opts_in():
    llm = _fake_llm()
    llm.set_sampler_extensions(False)
    base = dict(top_k=20, top_p=1.0, min_p=0.0, temp=1.0, seed=1)
    for kw in (dict(typical_p=0.5), dict(typical_p=0.0), dict(mirostat_mode=2), dict(mirostat_mode=1)):
        with pytest.raises(NotImplementedError, match="set_sampler_extensions"):
            llm.init_sampler_for_generate(**dict(base, **kw))
    assert llm._lib.calls == []
    llm.init_sampler_for_generate(**base)
    assert [c[0] for c in llm._lib.calls] == ["rca_lm_sampler_init"] and llm._sampler_params["typical_p"] == 1.0
    llm.set_sampler_extensions(True)
    llm.init_sampler_for_generate(typical_p=0.5, **base)
    assert llm._lib.calls[-1][0] == "rca_lm_sampler_set_typical"


def test_init_sampler_forwards_and_refuses():
    base = dict(top_k=40, top_p=0.95, min_p=0.05, temp=0.8, seed=3)
    llm = _fake_llm()
    llm.init_sampler_for_generate(**base)
    assert [c[0] for c in llm._lib.calls] == ["rca_lm_sampler_init"]             # neither option: the calls of before, nothing else
    llm = _fake_llm()
    llm.init_sampler_for_generate(typical_p=0.5, **base)
    assert [c[0] for c in llm._lib.calls] == ["rca_lm_sampler_init", "rca_lm_sampler_set_typical"] and llm._lib.calls[1][1] == 0.5
    assert llm._sampler_params["typical_p"] == 0.5 and llm._sampler_params["mirostat_mode"] == 0
    llm = _fake_llm()
    llm.init_sampler_for_generate(typical_p=0.5, mirostat_mode=2, mirostat_tau=3.0, mirostat_eta=0.25, **dict(base, top_k=0))
    assert llm._lib.calls[1:] == [("rca_lm_sampler_set_mirostat", 2, 3.0, 0.25)]      # typical is ignored under mirostat, top_k too
    assert llm.mirostat_mu() == 7.5
    again = _fake_llm()
    again.init_sampler_for_generate(**llm._sampler_params)                        # what a re-created sampler forwards
    assert again._lib.calls[1:] == llm._lib.calls[1:2] and again._sampler_params == llm._sampler_params
    for kw in (dict(typical_p=1.0), dict(typical_p=0.0), dict(typical_p=0.5, temp=0.0, top_k=0), dict(mirostat_mode=2, temp=0.0)):
        llm = _fake_llm()
        llm.init_sampler_for_generate(**dict(base, **kw))
        assert "rca_lm_sampler_set_typical" not in [c[0] for c in llm._lib.calls], kw
    llm = _fake_llm()
    for kw, exc, text in ((dict(typical_p=0.5, top_k=0), ValueError, "typical_p 0.5 needs top_k in 1..256"),
                          (dict(typical_p=0.5, top_k=257), ValueError, "top_k is 257"),
                          (dict(typical_p=-0.1), ValueError, "typical_p -0.1"),
                          (dict(typical_p=float("nan")), ValueError, "typical_p nan"),
                          (dict(mirostat_mode=1), NotImplementedError, "mirostat_mode 1"),
                          (dict(mirostat_mode=3), ValueError, "mirostat_mode 3"),
                          (dict(mirostat_mode=2, mirostat_tau=-1.0), ValueError, "mirostat_tau -1.0"),
                          (dict(mirostat_mode=2, mirostat_eta=float("nan")), ValueError, "mirostat_eta nan"),
                          (dict(grammar=object()), NotImplementedError, "grammar")):
        with pytest.raises(exc, match=text):
            llm.init_sampler_for_generate(**dict(base, **kw))
    assert llm._lib.calls == []                                                   # refused before anything reached the library
