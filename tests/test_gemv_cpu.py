"""tests/gemv_ref.py checked without a GPU: the cases meet their stated conditions and reach every seam of lm_gemv_body according to the
restated launch rules, and the derived bound has room (the kernel's own order, restated in f32, stays inside it) and teeth (six
deliberate faults in that restatement leave it)."""
import numpy as np
import pytest

import gemv_ref as R

SMALL = [(m, f) for m, f in R.MODEL_FORMATS if m in ("P", "Q", "S", "T")]


def instances(model, fmt, kind, M=1):
    return [R.gemv_instance(kind, t, n, k, M) for t, n, k in R.launches(model, fmt, kind)]


# ------------------------------------------------------------------------------------------------------------------ the cases
@pytest.mark.parametrize("model,fmt", SMALL)
def test_the_chunk_factors_give_the_formats_f32_values(model, fmt):
    """s q - m1 rounded once is the value gemm128_ref.blocks_of reports, in every class: the restated kernel and the reference start from
    the same weights"""
    for wclass in R.WCLASSES:
        L = R.layer(model, fmt, wclass)
        for p, W in L["values"].items():
            form = R.chunk_form(L["types"][p], L["params"][p])
            if form is None:
                continue
            qf, s, m1 = form
            v = np.repeat(s, 8, axis=1) * qf - (np.repeat(m1, 8, axis=1) if m1 is not None else 0.0)
            assert np.array_equal(v.astype(np.float32), W), (wclass, p)
            if m1 is None:
                assert np.array_equal(v, W.astype(np.float64)), (wclass, p, "an exact product")


@pytest.mark.parametrize("model,fmt", SMALL + [("D6", f) for f in R.FORMATS])
def test_class_a_is_exact_in_any_order(model, fmt):
    """kinds 1 and 3: integer factors and rows whose magnitude sums stay below 2^22, and the f32 restatement equals the integer product"""
    L = R.layer(model, fmt, "int")
    for kind in (1, 3):
        p = R.PROJ_OF_KIND[kind][0]
        t, W = L["types"][p], L["values"][p]
        form = R.chunk_form(t, L["params"][p])
        mag = R.magnitude_matrix(t, W, form)
        assert np.array_equal(W, np.round(W)) and np.array_equal(mag, np.round(mag))
        x = R.act_int([mag], W.shape[1], 100 + kind)
        assert np.array_equal(x, np.round(x)) and x.any()
        assert (np.abs(x.astype(np.float64)) @ mag.T).max() < 2.0 ** 22
        want = x.astype(np.int64) @ W.astype(np.int64).T
        assert np.array_equal(x.astype(np.float64) @ W.astype(np.float64).T, want)
        n = min(64, W.shape[0])
        NIT = R.gemv_instance(kind, t, W.shape[0], W.shape[1], 2)[0]
        got = R.gemv_f32(W[:n], t, None if form is None else tuple(None if a is None else a[:n] for a in form), x, NIT)
        assert np.array_equal(got, want[:, :n])


def test_one_hot_sets_hold_the_seam_columns():
    for K in (136, 256, 264, 768, 2048, 4096, 6144, 8192):
        nit = R.cdiv(R.cdiv(K // 8, 4), 64)
        NIT = 4 if nit == 3 else nit
        cols = R.onehot_columns(K, NIT)
        assert len(cols) % 2 == 0 and len(cols) <= max(256, min(K, 512)) and len(set(cols)) == len(cols)
        if K <= 512:
            assert len(cols) == K
        assert R.seam_columns(K, NIT) <= set(cols.tolist()), K
        cpw, cns = R.wave_chunks(K)
        assert {0, K - 1} <= set(cols.tolist()) and sum(cns) == K // 8


def test_every_seam_is_reached():
    """each seam the kernel has, by the restated launch rules, on the cases the GPU test runs"""
    S = set(R.STAGES)
    # partly idle waves, 16-bit rows only, AO != hidden, G = 2, vocabulary 1001
    assert R.wave_chunks(136) == (5, [5, 5, 5, 2]) and R.wave_chunks(264) == (9, [9, 9, 9, 6])
    for m in ("P", "Q"):
        assert R.FORMATS_OF[m] == ("bf16", "f16") and R.MODELS[m]["n_heads"] * 64 != R.MODELS[m]["hidden"]
        assert R.MODELS[m]["n_heads"] // R.MODELS[m]["n_kv_heads"] == 2 and R.vocab_of(m, "bf16") == 1001
    assert {R.kind_k("P", k) for k in (0, 2, 4)} == {136} and R.kind_k("P", 3) == 264 and {R.kind_k("Q", k) for k in (0, 2, 4)} == {264}
    # K = 256 (56 idle lanes) and K = 768 (24 chunks per wave) in all eight forms, under the prologue and without it
    for f in R.FORMATS:
        for k in R.ALL5:
            assert ("S", f, k) in S and ("T", f, k) in S
    assert R.wave_chunks(256) == (8, [8] * 4) and R.wave_chunks(768) == (24, [24] * 4)
    assert {R.kind_k("S", k) for k in (0, 1, 2, 4)} == {256} and R.kind_k("S", 3) == 768 and R.kind_k("T", 1) == 768 and R.kind_k("T", 3) == 256
    # K = 2048: every lane busy, one chunk each
    assert R.wave_chunks(2048) == (64, [64] * 4) and set(R.FORMATS_OF["W"]) == {"bf16", "q8_0", "q4_k"}
    # down projections: NIT = 2, nit == 3 on the NIT = 4 instance, NIT = 4, in all eight forms; R per format
    for f in R.FORMATS:
        t = R.types_of("D4", f)["down"]
        want_r = 8 if (t in R.FOUR_BIT or t == "q6_k") else 4
        for m, nit in (("D4", 2), ("D6", 4), ("D8", 4)):
            assert (m, f, 3) in S
            assert instances(m, f, 3) == [(nit, want_r, 1, R.cdiv(256, want_r))], (m, f)
        assert R.cdiv(R.cdiv(6144 // 8, 4), 64) == 3 and R.wave_chunks(6144) == (192, [192] * 4)     # lanes: chunks l, l + 64, l + 128; the fourth is empty
    # ragged N
    heads = {f: R.types_of("S", f)["head"] for f in R.FORMATS}
    assert {R.vocab_of("S", f) for f in R.FORMATS} == {1001, 1002, 1004}
    for f, t in heads.items():
        v = R.vocab_of("S", f)
        assert v % 16 == (9 if t in ("bf16", "f16") else 10 if t in R.PAIR else 12) and instances("S", f, 4)[0][1] == 16
    assert {R.types_of("T", "q4_0")["head"], R.types_of("S", "q4_0")["head"]} == {"q4_0", "q4_1"}
    assert {R.types_of("T", "iq4")["head"], R.types_of("S", "iq4")["head"]} == {"iq4_nl", "iq4_xs"}
    # several batches per workgroup: the head keeps 8 with a last workgroup of one batch of 12 rows; gate/up keeps 2
    for f in R.FORMATS:
        assert instances("D8", f, 4) == [(1, 16, 8, 65)] and R.cdiv(R.VOCAB_BIG, 16) == 513 and R.VOCAB_BIG % 16 == 12
        assert instances("D8", f, 2) == [(1, 16, 2, 512)]
        assert instances("S", f, 4)[0][2] == 1 and instances("S", f, 2)[0][2] == 1       # the 64-workgroup rule on the small ones
    # grouped-query shapes
    assert {R.MODELS[m]["n_heads"] // R.MODELS[m]["n_kv_heads"] for m in R.MODELS} == {1, 2, 4}
    # the split-V layer: two launches, the second Q6_K with a row base
    assert R.launches("S", "q6_k", 0) == [("q4_k", 320, 256), ("q6_k", 64, 256)]
    assert all(len(R.launches(m, f, 0)) == (2 if f == "q6_k" else 1) for m, f in R.MODEL_FORMATS)
    # the QKV pairing: a batch of 4 slots is two (d, d + 32) pairs
    assert [R.row_of(0, r, 4, True) for r in range(4)] == [0, 32, 1, 33] and R.row_of(16, 0, 4, True) == 64
    assert sorted(R.row_of(b, r, 8, True) for b in range(16) for r in range(8)) == list(range(128))


def test_overridden_geometries_are_legal():
    """the two pairs the GPU test hands to its children: every stage still launches an instance that exists, with another (R, batches)"""
    changed = 0
    for name, geom in R.GEOMETRIES.items():
        for model, fmt, kind in R.GEOMETRY_STAGES:
            for t, n, k in R.launches(model, fmt, kind):
                NIT, Rr, bpw, grid = R.gemv_instance(kind, t, n, k, 2, geom)
                assert Rr in (4, 8, 16) and bpw >= 1 and grid * bpw * Rr >= n and (grid - 1) * bpw * Rr < n
                assert not (t in ("q5_k", "q4_0", "q4_1", "iq4_nl", "iq4_xs") and NIT == 4 and Rr == 16)
                changed += (Rr, bpw) != R.gemv_instance(kind, t, n, k, 2)[1:3]
    assert changed > len(R.GEOMETRY_STAGES)


# ------------------------------------------------------------------------------------------------------------------ room
ROOM = [(m, f, k) for m, f, k in R.STAGES if m in ("P", "Q", "S", "T", "D6") or (m in ("W", "D4", "D8") and f in ("bf16", "q4_k"))]
WORST = {}


def rows_of(cls, model, kind, seed):
    K = R.kind_k(model, kind)
    return R.act_normal(K, kind, seed) if cls == "c" else R.act_coherent(K, kind, seed)


@pytest.mark.parametrize("model,fmt,kind", ROOM)
def test_the_restated_kernel_stays_inside_the_bound(model, fmt, kind):
    for cls in "cd":
        L = R.layer(model, fmt, R.WCLASS_OF[cls])
        got, ref = R.stage_f32(model, fmt, kind, L, rows_of(cls, model, kind, 200 + kind), rows=32)
        r = R.worst_ratio(got, ref)
        WORST[fmt, cls] = max(WORST.get((fmt, cls), 0.0), r)
        assert r <= 1.0, (cls, r)


def test_report_of_the_restatements_worst_ratios():
    for cls in "cd":
        print(f"GEMV restated in f32, worst error / bound, class {cls}: " + ", ".join(f"{f} {WORST[f, cls]:.3f}" for f in R.FORMATS if (f, cls) in WORST))
    assert WORST and all(v <= 1.0 for v in WORST.values())


# ------------------------------------------------------------------------------------------------------------------ teeth
FAULT_CASES = {
    "x_bf16": [("S", f, 1, "c") for f in R.FORMATS] + [("P", "bf16", 3, "c")],
    "scale_f16_twice": [("S", "q4_k", 1, "c"), ("S", "q5_k", 1, "c"), ("S", "q6_k", 3, "c"), ("S", "iq4", 1, "c"), ("T", "q4_k", 0, "c")],
    "drop_last_min": [("S", "q4_k", 1, "c"), ("S", "q5_k", 1, "c"), ("S", "q4_0", 1, "c"), ("S", "q4_0", 2, "c"), ("D6", "q4_k", 3, "c")],
    "drop_chunk": [("P", f, k, c) for f in ("bf16", "f16") for k in (0, 2, 4) for c in "cd"],
    "no_eps": [("S", "bf16", 4, "c"), ("P", "bf16", 0, "c"), ("S", "q4_k", 2, "c"), ("T", "q8_0", 0, "d")],
    "rope_neighbour": [("S", "bf16", 0, "c"), ("S", "q4_k", 0, "c"), ("T", "q6_k", 0, "d")],
}


@pytest.mark.parametrize("fault", R.FAULTS)
def test_a_deliberate_fault_leaves_the_bound(fault):
    for model, fmt, kind, cls in FAULT_CASES[fault]:
        L = R.layer(model, fmt, R.WCLASS_OF[cls])
        x = rows_of(cls, model, kind, 200 + kind)
        clean, ref = R.stage_f32(model, fmt, kind, L, x, rows=32)
        got, _ = R.stage_f32(model, fmt, kind, L, x, rows=32, fault=fault)
        r0, r = R.worst_ratio(clean, ref), R.worst_ratio(got, ref)
        print(f"{fault} on {model} {fmt} kind {kind} class {cls}: error / bound {r0:.3f} -> {r:.1f}")
        assert r0 <= 1.0 < r, (model, fmt, kind, cls, r0, r)
