"""tests/gemm128_ref.py held to its own definitions without a GPU: the k-slice forms restated from rca_lm.hip give the slice counts the
test models were chosen for, class a meets the two conditions that make every partial sum an exact integer, the one-hot and split
restatements are what they say, and the bound has teeth (a dropped hi x lo product exceeds it 8 times on class d) while the kernel's
own arithmetic restated in f32 stays under half of it."""
import numpy as np
import pytest

import gemm128_ref as G


def test_slice_counts_and_forms_of_the_test_models():
    """the table of the three models: slices per projection (g128_splits), groups (g128_group), and the four forms (g128_form)"""
    want = {"B": (1, 1, 1, 4), "A": (2, 2, 2, 8), "C": (4, 4, 4, 16)}
    for model, ns in want.items():
        assert tuple(G.g128_splits(*G.kind_nk(model, kind)) for kind in range(4)) == ns, model
    assert [G.g128_group(n) for n in (1, 2, 4, 8, 16)] == [1, 1, 1, 2, 4]
    # B: QKV has 384 rows (the K head and the V head share one 128-row tile), every epilogue but down's fused
    assert G.kind_nk("B", 0)[0] == 384
    assert G.form_name(G.g128_form(384, 1, 1, 512)) == "fused"
    seen = set()
    for model in ("A", "C"):
        for kind in range(4):
            N, K = G.kind_nk(model, kind)
            ns = G.g128_splits(N, K)
            for rows in (128, 1024):
                for seq_min in (0, 1, 512):
                    f = G.g128_form(N, ns, rows // 128, seq_min)
                    seen.add(G.form_name(f))
                    gy, nseq, ep, grp = f
                    assert gy * nseq == ns and (ep == 0 or ep * grp * nseq == ns * (grp if nseq == 1 else 1))
            assert G.form_name(G.g128_form(N, ns, 1, 0)) == "every slice stored" + (", grouped epilogue" if ns >= 8 else "")
            assert G.form_name(G.g128_form(N, ns, 1, 1)) == ("walking" if ns <= 4 else "group sums stored")
    assert seen == {"walking", "group sums stored", "every slice stored", "every slice stored, grouped epilogue"}
    # at the process threshold (512 workgroups) model A never leaves "every slice stored": the other forms need the tap's seq_min
    for kind in range(4):
        N, K = G.kind_nk("A", kind)
        assert G.form_name(G.g128_form(N, G.g128_splits(N, K), 8, 512)).startswith("every slice stored")
    for v in G.VOCABS:
        assert v % 4 == 0 and v % 128 == 4
    assert G.VOCAB_BF16_EXTRA % 128 == 2


def test_split_restates_the_staging_split():
    rng = np.random.default_rng(0)
    w = (rng.standard_normal(4096) * 0.05).astype(np.float32)
    hi, lo = G.split(w)
    assert not (hi.view(np.uint32) & 0xFFFF).any() and not (lo.view(np.uint32) & 0xFFFF).any()
    assert (np.abs(w - hi) <= 2.0 ** -8 * np.abs(w)).all()
    assert (np.abs(w.astype(np.float64) - hi - lo) <= 2.0 ** -17 * np.abs(w)).all()
    assert G.bf16_rne(np.array([257.0, 259.0, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8], np.float32)).tolist() == [256.0, 260.0, 1.0, 1.0 + 2.0 ** -6]   # ties to even
    assert np.array_equal(G.widen(G.bits(hi)), hi)


@pytest.mark.parametrize("fmt", G.FORMATS)
def test_class_a_meets_its_two_conditions(fmt):
    """integers throughout; w_lo[n, k] x_lo[t, k] = 0 for every (n, k, t); sum_k |w| |x| <= 2^22; and the class is not vacuous: w_lo != 0
    wherever the type reaches more than 8 significant bits, x_lo != 0 on part of the columns, every column read by some row"""
    reaches = {"bf16": (), "f16": "all", "q8_0": (), "q4_k": "all", "q5_k": "all", "q6_k": "all", "q4_0": ("o", "down"), "iq4": ("o", "down")}[fmt]
    for model, vocab in [("A", v) for v in G.VOCABS] + ([("B", G.VOCABS[0]), ("C", G.VOCABS[0])] if fmt in ("bf16", "q4_k") else []):
        _, values = G.layer(model, fmt, "int", vocab)
        for kind in range(5):
            if vocab != G.VOCABS[0] and kind != 4:
                continue
            W = G.fused(values, kind)
            assert np.array_equal(W, np.rint(W))
            M = 128 if kind == 4 else 129
            xh, xl = G.act_int(W, M, 100 + kind)
            h, l = G.widen(xh), G.widen(xl)
            assert np.array_equal(h, np.rint(h)) and np.array_equal(l, np.rint(l))
            _, wlo = G.split(W)
            assert not ((wlo != 0).any(axis=0) & (l != 0).any(axis=0)).any(), (model, kind)
            S = (np.abs(h.astype(np.float64)) + np.abs(l)) @ np.abs(W.astype(np.float64)).T
            assert S.max() <= 2.0 ** 22, (model, kind, S.max())
            assert (l != 0).any() and ((h != 0).any(axis=0)).all(), (model, kind)
            name = {0: "q", 1: "o", 2: "gate", 3: "down", 4: "head"}[kind]
            types = G.matrix_types(fmt, vocab)
            if types[name] not in ("bf16", "q8_0", "q4_0", "iq4_nl"):
                assert reaches == "all" or name in reaches or kind == 4
                assert (wlo != 0).mean() > 0.05, (model, kind)
            else:
                assert not wlo.any()


def test_head_class_a_reaches_the_high_bits_of_the_second_types():
    for fmt, t in (("q4_0", "q4_1"), ("iq4", "iq4_xs"), ("q6_k", "q6_k")):
        assert G.matrix_types(fmt, G.VOCABS[1])["head"] == t
        _, values = G.layer("A", fmt, "int", G.VOCABS[1])
        assert (G.split(values["head"])[1] != 0).mean() > 0.05


@pytest.mark.parametrize("fmt", G.FORMATS)
def test_class_d_bound_has_teeth_and_room(fmt):
    """coherent data: the reference with w_lo x_hi left out, and with w_hi x_lo left out, each miss the bound 8 times and more at every
    K in use (bf16 weights have no lo plane: only the second), and the kernel's f32 arithmetic restated stays under half of it"""
    for model in ("A", "B", "C") if fmt in ("bf16", "q4_k") else ("A",):
        _, values = G.layer(model, fmt, "coherent")
        for kind in range(5):
            W = G.fused(values, kind)
            N, K = W.shape
            name = {0: "q", 1: "o", 2: "gate", 3: "down", 4: "head"}[kind]
            bf = G.matrix_types(fmt, G.VOCABS[0])[name] == "bf16"
            ns = 1 if kind == 4 else G.g128_splits(N, K)
            xh, xl = G.act_coherent(K, 31, 300 + kind)
            rows = slice(0, 256) if N > 256 else slice(None)      # (the restatement walks K / 16 steps: a slab of rows is enough)
            y, b = G.gemm(W[rows], xh, xl, bf, ns)
            assert (W > 0).all() and (G.widen(xl) > 0).all()
            hi, lo = G.split(W[rows])
            h, l = G.widen(xh).astype(np.float64), G.widen(xl).astype(np.float64)
            if not bf:
                assert (lo > 0).all()
                assert ((h @ lo.astype(np.float64).T) >= 8 * b).all(), (model, kind, "w_lo x_hi")
            assert ((l @ hi.astype(np.float64).T) >= 8 * b).all(), (model, kind, "w_hi x_lo")
            own = G.kernel_f32(W[rows], xh, xl, bf, ns)
            assert G.ratio(np.abs(own.astype(np.float64) - y), b) < 0.5, (model, kind)


def test_normal_class_restatement_stays_under_the_bound():
    """class c at the shapes of model A: the f32 restatement of the kernel against the float64 reference"""
    for fmt in ("bf16", "q4_k", "q6_k"):
        _, values = G.layer("A", fmt, "normal")
        for kind in (0, 3):
            W = G.fused(values, kind)[:256]
            xh, xl = G.act_normal(W.shape[1], 31, 200 + kind)
            bf = fmt == "bf16"
            ns = G.g128_splits(*G.kind_nk("A", kind))
            y, b = G.gemm(W, xh, xl, bf, ns)
            assert G.ratio(np.abs(G.kernel_f32(W, xh, xl, bf, ns).astype(np.float64) - y), b) < 0.5


def test_epilogues_restate_rope_and_swiglu():
    """the float64 epilogues against plain formulas on a few values; fp16 interval check is exact at zero bound"""
    from realtime_codec_agent_amd.llm import rope_inv_freq
    inv = rope_inv_freq(G.config("B", G.VOCABS[0]))
    rng = np.random.default_rng(1)
    y = rng.standard_normal((3, 384))
    out = G.epilogue(0, y, np.zeros_like(y), "B", 7, inv)
    ang = (7 + np.arange(3))[:, None] * inv[None, :].astype(np.float64)
    q0 = y[:, :64]
    assert np.allclose(out["y"][:, :32], q0[:, :32] * np.cos(ang) - q0[:, 32:] * np.sin(ang), atol=1e-5)
    assert np.allclose(out["y"][:, 32:64], q0[:, 32:] * np.cos(ang) + q0[:, :32] * np.sin(ang), atol=1e-5)
    assert np.array_equal(out["v"], y[:, 320:]) and out["k"].shape == (3, 64)
    assert (out["bound"] > 0).all() and (out["v_bound"] == 0).all()
    g = G.epilogue(2, y, np.zeros_like(y), "B")
    assert np.allclose(g["y"], y[:, :192] / (1 + np.exp(-y[:, :192])) * y[:, 192:])
    assert (g["bound"] >= 2.0 ** -17 * np.abs(g["y"])).all()
    v = np.array([1.0, 1.0 + 2.0 ** -11, 60000.0])
    assert G.f16_interval_ok(v.astype(np.float16), v, np.zeros(3)).all()
    assert not G.f16_interval_ok(np.array([1.0 + 2.0 ** -10], np.float16), v[:1], np.zeros(1)).any()
