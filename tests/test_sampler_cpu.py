"""The sampler's hand-made rows (tests/samp_cases.py) and the C restatement (oracle/sampler_oracle.c) against plain float64
references -- no GPU.  tests/test_sampler_gpu.py holds the device to the restatement token for token on the same rows; this file is
what keeps the restatement itself honest: it shares the counter RNG, the polynomial exp and its whole structure with the device, so
it is checked here against references that share none of them (a float64 allowed set, a float64 softmax, a chi-square test)."""
import numpy as np
import pytest

import samp_cases as S
from oracle import lm_ref


@pytest.mark.parametrize("name,V", S.ROW_VOCABS)
def test_rows_reach_the_bodies_they_name(name, V):
    r = S.BY_NAME[name]
    row = r.make(V)
    assert row.dtype == np.float32 and row.shape == (V,)
    assert not np.isnan(row).any() and np.isfinite(row).any() and row.max() > -np.inf
    assert np.array_equal(row.view(np.uint32), r.make(V).view(np.uint32))          # seeded: the same bits every time
    for k in (1, 20, 256):
        n, body = S.candidates(row, k)
        assert body == r.body(V, k), (name, V, k, n, body)
    want = r.sizes[S.VOCABS.index(V)]
    if want:
        assert S.candidates(row, 20)[0] == want and S.candidates(row, 256)[0] == want


def test_the_cap_rows_straddle_both_caps_and_every_body_is_reached():
    sizes = [S.candidates(S.BY_NAME[f"cap_{n}"].make(8192), 20) for n in (1024, 1025, 4096, 4097)]
    assert sizes == [(1024, "count"), (1025, "sort"), (4096, "sort"), (4097, "scan")]
    assert (S.SAMP_FAST_CAP, S.SAMP_CAND_CAP) == (1024, 4096)
    reached = {r.body(V, k) for r in S.ROWS for V in S.VOCABS for k in (1, 20, 256)}
    assert reached == {"count", "sort", "scan"}
    # a vocabulary inside the first cap never leaves the count body; the odd shape is one
    from lm_shape_cases import BY_NAME
    c = BY_NAME[S.ODD_SHAPE]
    assert c.vocab % 64 and c.vocab <= S.SAMP_FAST_CAP and "bf16" in c.formats
    assert {S.path(*cfg[:2], cfg[3], 8192) for cfg in S.configs(8192)} == {"serial", "whole", "big"}


def test_candidates_restates_the_bin_rule_on_known_rows():
    """the bin of a key is sign, exponent and two mantissa bits: [1.0, 1.25) is one bin, 1.25 the next; both zeros share one"""
    row = np.full(64, -3.0, np.float32)
    row[:10] = np.linspace(1.0, 1.2499, 10)
    row[10] = 1.25
    assert S.candidates(row, 1) == (1, "count") and S.candidates(row, 2) == (11, "count") and S.candidates(row, 12) == (64, "count")
    z = np.array([-0.0, 0.0, -1.0], np.float32)
    assert S.sample_key32(z)[0] == S.sample_key32(z)[1] > S.sample_key32(z)[2]
    k = S.sample_key32(np.array([-np.inf, -3e38, -1.0, -1e-45, 0.0, 1e-45, 1.0, 3e38, np.inf], np.float32)).astype(np.int64)
    assert (np.diff(k) > 0).all()


def test_allowed_set_and_draw_probs_on_rows_worked_by_hand():
    row = np.array([0.0, np.log(4.0), np.log(2.0), np.log(2.0), -np.inf], np.float32)      # masses 1, 4, 2, 2, 0 of 9
    a, m = S.allowed_set(row, 3, 1.0, 0.0)
    assert a.tolist() == [1, 2, 3] and m == np.inf                                          # the tie at the cut: lowest index first
    a, m = S.allowed_set(row, 0, 0.7, 0.0)                                                  # need 6.3 of 9: 4 + 2 = 6 < 6.3 <= 8
    assert a.tolist() == [1, 2, 3] and abs(m - 0.3 / 9) < 1e-6
    a, m = S.allowed_set(row, 4, 1.0, 0.3)                                                  # p / p_max = 1, .5, .5, .25
    assert a.tolist() == [1, 2, 3] and abs(m - (1 - 0.25 / 0.3)) < 1e-6
    assert S.allowed_set(row, 4, 0.5, 0.3, greedy=True)[0].tolist() == [1]
    p = S.draw_probs(row, np.array([1, 2, 3]), 0.5)                                         # temp 0.5 squares the masses: 16, 4, 4
    assert np.allclose(p, [16 / 24, 4 / 24, 4 / 24], atol=1e-6)
    eq = S.BY_NAME["eight_equal"].make(8192)
    a, m = S.allowed_set(eq, 0, 0.5, 0.0)                                                   # cum == need exactly after four
    assert a.tolist() == np.sort(np.nonzero(eq == 3.0)[0])[:4].tolist() and m == 0.0


@pytest.mark.parametrize("name,V", S.ROW_VOCABS)
def test_restatement_draws_only_allowed_tokens(name, V):
    """every path of the restatement (serial, whole vocabulary, big) on every row: where the float64 cut is clear of every token's
    mass (margin > MARGIN_MIN) a draw is a token of allowed_set; greedy draws are the first of the best"""
    row = S.BY_NAME[name].make(V)
    checked = 0
    for top_k, top_p, min_p, temp in S.configs(V):
        allowed, margin = S.allowed_set(row, top_k, top_p, min_p, greedy=temp <= 0.0)
        if not margin > S.MARGIN_MIN:
            continue
        checked += 1
        allowed = set(allowed.tolist())
        for c in range(S.DRAWS):
            t = lm_ref.sample(row, top_k, top_p, min_p, temp, 99, c)
            assert t in allowed, (name, V, top_k, top_p, min_p, temp, c, t)
    assert checked >= len(S.configs(V)) // 2, checked


def test_restatement_penalties_and_bias_follow_the_plain_row():
    """logit bias, then penalties: a draw from (row, bias, history) is the draw from the row patched in numpy"""
    for name in ("gaussian", "shifted_up"):
        row = S.BY_NAME[name].make(4096)
        row[7] = 0.0
        prev = [7, int(row.argmin()), 7, 100]
        bias = {int(row.argmax()): -np.inf, 200: 50.0}
        pen = dict(repeat_penalty=1.3, frequency_penalty=0.25, presence_penalty=0.15)
        patched = S.penalised(row, bias, prev, 1.3, 0.25, 0.15)
        assert patched[7] == np.float32(-(np.float32(prev.count(7)) * np.float32(0.25) + np.float32(0.15))) and patched[int(row.argmax())] == -np.inf
        for top_k, top_p, min_p, temp in S.configs(4096)[::3]:
            for c in range(4):
                assert (lm_ref.sample(row, top_k, top_p, min_p, temp, 5, c, bias, prev_tokens=prev, **pen)
                        == lm_ref.sample(patched, top_k, top_p, min_p, temp, 5, c))


@pytest.mark.parametrize("path", sorted(S.CHI_CONFIGS))
def test_restatement_passes_chi_square(path):
    """4096 draws with consecutive counters from an 8-token support at temp 0.8 against the float64 softmax: chi-square below the
    1 - 1e-4 quantile of 7 degrees of freedom.  Measured with seed 1234: serial 5.95, whole vocabulary and big path 4.72 (their
    Gumbel noise is keyed by (draw, token), the same for both)."""
    chi = S.chi_square(S.chi_reference(path), S.CHI_V)
    print(f"chi-square, {path} path: {chi:.2f} (bound {S.CHI_BOUND})")
    assert chi < S.CHI_BOUND
