"""The tables and references of the layer-by-layer tests of the f32 encoder, checked without a GPU (tests/enc_cases.py):
  * every threshold, forced-seam, view, fused and route-1 case against the launch rule it claims, in plain integers;
  * every class and every instantiation the encoder can launch is reached by at least one case;
  * the C oracle's layer function chains to the oracle's own taps bit for bit on every config, and stays within the fma-chain bound
    (K + 1) 2^-24 m of float64 (derived in dec_cases, not measured);
  * the two hand-off identities hold bit for bit on the `signed` inputs;
  * teeth: an activation applied twice, a dropped activated store, a view shifted by one column and a zero pad replaced by the
    neighbouring row's sample each change at least one compared element of the test's own inputs;
  * large cases leave no seam row and no affordable row to the NaN check alone;
  * the prototype of rca_codec_encoder_layer_tap against its declaration in include/rca.h."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import enc_cases as ec
from realtime_codec_agent_amd import _native as N

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "rca.h")


def _by(group):
    return [c for c in ec.cases() if c.group == group]


# ------------------------------------------------------------------------------------------------ the tables against the rules
def test_threshold_cases_satisfy_the_inequality_they_claim():
    for name, layer, w in ec.THRESHOLDS + ec.UNBALANCED:
        ly = ec.layer_of(name, layer)
        B, Lin = ec.shape_for(name, layer, w)
        cols = Lin // ly["s"]
        assert B >= 3 and cols % 64 != 0 and Lin % ec.frame_mult(name, layer) == 0
        got = ec.cdiv(B * cols, 64) * ec.cdiv(ly["cout"], 64)
        # at the threshold or within 8 column tiles above it; one tile below it or within 8 (rows are whole frames: layer 1 of the
        # default strides has 160 columns per frame)
        assert (w <= got < w + 8 * ec.cdiv(ly["cout"], 64)) if w % 1024 == 0 else (w - 8 * ec.cdiv(ly["cout"], 64) < got <= w), (name, layer, w, got)
    for c in _by("threshold") + _by("unbalanced"):
        ly = ec.layer_of(c.config, c.layer)
        w = ec.cdiv(c.B * (c.Lin // ly["s"]), 64) * ec.cdiv(ly["cout"], 64)
        bal = dict(c.env).get("RCA_CONV_BALANCE") != "0" and ly["k"] >= 8 and ly["cin"] % ec.CIC[ly["k"]] == 0
        want = (ec.M64x64 if w >= (3072 if bal else 8192) else ec.M32x64 if w >= 2048 else
                ec.M64x32 if ly["k"] == 3 and ly["cout"] >= 64 and w >= 1024 else ec.M32x32)
        assert c.kclass == want, c
        assert c.mixed is (None if bal and want in (ec.M32x64, ec.M64x64) else False), c
    seen = {(ec.layer_of(n, l)["k"], w) for n, l, w in ec.THRESHOLDS}
    for k in (8, 10, 16):      # the balanced layers: 32 x 64 from 2048, 64 x 64 from 3072, and one column tile below each
        assert {(k, 2047), (k, 2048), (k, 3071), (k, 3072)} <= seen
    assert {(4, 2047), (4, 2048), (4, 8191), (4, 8192), (3, 1023), (3, 1024), (3, 2047), (3, 2048), (3, 8191), (3, 8192)} <= seen
    # whole-chunk and partial-chunk channel counts, on the strided layers and on conv_out
    chunks = {(ec.layer_of(c.config, c.layer)["k"], ec.whole_chunks(ec.layer_of(c.config, c.layer))) for c in ec.cases() if c.layer > 0}
    assert chunks >= {(k, w) for k in (4, 8, 3) for w in (True, False)} | {(10, True), (16, True)}
    assert ec.layer_of("odd", 5)["cin"] % 16 != 0 and ec.layer_of("tiny", 5)["cin"] % 16 == 0


def test_flag_cases_cover_every_combination_the_predicates_allow():
    for name in ec.SMALL_CONFIGS:
        n = ec.n_layers(name)
        for layer in range(1, n):
            got = {c.flags for c in _by("small") if (c.config, c.layer, c.variant) == (name, layer, 1)}
            want = {0} | ({1} if layer >= 2 and ec.packed(ec.layer_of(name, layer)) else set())
            if layer + 1 < n and ec.packed(ec.layer_of(name, layer + 1)):
                want |= {2} | ({3} if 1 in want else set())
            assert got == want, (name, layer, got, want)
            assert {c.flags for c in _by("small") if (c.config, c.layer, c.variant) == (name, layer, 0)} == {0}
    for c in ec.cases():
        assert (c.kind == "signed") == bool(c.flags), c               # every case with a flag runs the signed input
        assert not c.flags or (c.route == 0 and c.variant >= 1), c
        assert ec.flags_ok(c.config, c.layer, c.flags, c.variant, bool(c.flags & 4) and ec.fuse_ok(c.config, c.B, c.Lin, c.variant)), c
    for layer in (2, 3, 4):
        assert {c.flags for c in _by("threshold") if c.layer == layer} == {0, 1, 2, 3}
        assert {c.flags for c in _by("forced") if c.layer == layer} == {0, 3}


def test_forced_seams_fall_inside_a_row_and_have_a_single_shape_twin():
    fine = set()
    for c in _by("forced"):
        ly = ec.layer_of(c.config, c.layer)
        cols = c.Lin // ly["s"]
        plan = dict(c.env)["RCA_CONV_BALANCE_PLAN"]
        p = ec.plan_of(plan, ly, c.B, cols, c.kclass)
        assert c.mixed is (p is not None) and ly["k"] >= 8
        if p is None:
            continue
        bulk, fcols = p
        total = ec.cdiv(c.B * cols, 64)
        assert bulk % 8 == 0 and 0 <= bulk < total
        if bulk:
            assert (bulk * 64) % cols != 0, c                          # the seam is inside a row
            assert ec.seam_rows(c) and (bulk * 64) // cols in ec.seam_rows(c)
        fine.add((ly["k"], c.kclass, fcols))
        # the single-shape twin: the same input under RCA_CONV_BALANCE=0 or an unforced case, compared with the same oracle rows
        assert any((t.config, t.layer, t.B, t.Lin) == (c.config, c.layer, c.B, c.Lin) and not t.mixed
                   for t in _by("unbalanced") + _by("threshold")), c
    for k in (8, 10, 16):      # 64 x 64 bulk with both fine shapes (32 x 64: the <.., 1, 2, 1> instance), 32 x 64 bulk with 32 x 32
        assert {(k, ec.M64x64, 64), (k, ec.M64x64, 32), (k, ec.M32x64, 32)} <= fine


def test_view_cases_sit_on_both_sides_of_the_chunk_rule():
    sides = set()
    for c in _by("view"):
        ly = ec.layer_of(c.config, c.layer)
        assert ec.view_ok(c.config, c.layer, c.B, c.Lin, c.view) and (ly["k"], ly["s"]) == (3, 1) and ec.view_halo(ly) == 1
        tiles = ec.cdiv(c.B * c.view, 32) * ec.cdiv(ly["cout"], 32)
        assert ec.view_chunk16(ly, c.B, c.view) == (tiles <= 1024 and ly["cin"] % 16 == 0)
        sides.add((ly["cin"] % 16 == 0, tiles))
        assert c.kclass == ec.view_class(ly, c.B, c.Lin, c.view)
    assert {(True, 1024), (True, 1025)} <= sides and any(not whole for whole, _ in sides)
    views = {(c.view, c.Lin) for c in _by("view")}
    assert any(v == 2 for v, _ in views) and any(v == L - 1 for v, L in views)      # keep + halo = 2; Lout - 1


def test_fused_cases_reach_every_fused_launch():
    got = {}
    for c in _by("fused"):
        e1 = ec.layer_of(c.config, 1)
        cfg = ec.config(c.config)[0]
        Lout = ec.cdiv(c.Lin, cfg.hop) * cfg.hop // e1["s"]
        assert cfg.k_in == 7 and (e1["k"], e1["s"]) in ec.FUSABLE and Lout >= 67 and c.flags & 4
        w = ec.cdiv(c.B * Lout, 64) * ec.cdiv(e1["cout"], 64)
        got.setdefault((e1["k"], c.kclass), set()).add((c.flags, w >= 8192))
        if c.kclass == ec.FIRST:
            assert e1["cin"] == 32 and e1["cout"] % 64 == 0 and w >= 8192 and Lout >= 131 and not dict(c.env)
        if c.kclass == ec.WIDE:
            assert e1["k"] == 4 and w >= 8192 and Lout >= 131
        if c.kclass == ec.M64x64:
            assert e1["k"] in (8, 16) and w >= 8192
        if c.kclass == ec.M32x32:
            assert w < 8192
    for key in ((4, ec.FIRST), (4, ec.WIDE), (4, ec.M32x32), (8, ec.M64x64), (8, ec.M32x32), (16, ec.M64x64), (16, ec.M32x32)):
        assert {f for f, _ in got[key]} == {4, 6}, key                 # each with the activated store off and on
    assert (4, ec.WS) in got
    assert any(c.kclass == ec.WIDE and dict(c.env).get("RCA_FUSE_MFMA_IN") == "0" and c.config == "full" for c in _by("fused"))
    # the k16s8 first layer's one-frame window stays unfused (40 columns), the GPU file's refusal case
    assert not ec.fuse_ok("f168", 3, 320, 1) and ec.fuse_ok("f168", 3, 536, 1)
    assert not ec.fuse_ok("k105", 3, 3200, 1) and not ec.fuse_ok("kin3", 3, 3200, 1)


def test_route1_cases_are_what_a_tail_call_can_launch():
    for c in _by("route1"):
        cfg = ec.config(c.config)[0]
        frames = ec.cdiv(c.Lin, cfg.hop) if c.layer == 0 else c.Lin // ec.frame_mult(c.config, c.layer)
        assert c.variant >= 1 and c.flags == 0 and c.view == 0 and c.B * frames <= ec.LAT_MAX_FRAMES
        assert c.layer == 0 or c.Lin % ec.frame_mult(c.config, c.layer) == 0
    assert {B * F for B, F in ec.ROUTE1_FRAMES} >= {1, 2, 3, 8, 9, 64}
    ks = {(ec.layer_of(c.config, c.layer)["k"], ec.layer_of(c.config, c.layer)["s"], c.kclass) for c in _by("route1")}
    for k, s in ((4, 2), (8, 4), (10, 5), (16, 8), (3, 1), (7, 1)):      # every instance of try_conv_lds, with 4 waves and with 1
        assert (k, s, ec.LDS4) in ks and (k, s, ec.LDS1) in ks or (k, s) == (7, 1) and (k, s, ec.LDS4) in ks, (k, s)
    assert (6, 3, ec.CHAIN) in ks and (5, 1, ec.CHAIN) in ks              # no instance: the launch of route 0
    assert any(c.layer == 0 and c.Lin % ec.config(c.config)[0].hop for c in _by("route1"))     # a ragged T: Lvalid < Lin
    ly = ec.layer_of("full", 3)
    assert ec.lds_columns(ly, 8 * 40) == 32 and ec.lds_columns(ec.layer_of("tiny", 3), 8 * 40) == 64   # columns halved by the LDS budget
    assert any(c.config == "full" and c.layer == 3 and c.Lin // 5 >= 64 for c in _by("route1"))


def test_the_tables_reach_every_documented_class():
    reach = {c.kclass for c in ec.cases()} | {c.kclass | ec.MIXED for c in ec.cases() if c.mixed}
    assert reach == ec.ENCODER_CLASSES, sorted(reach ^ ec.ENCODER_CLASSES)
    assert {ec.config(c.config)[0].k_in for c in _by("conv_in")} == {7, 5, 3}
    text = open(HEADER).read()
    for macro, value in (("CHAIN", ec.CHAIN), ("MFMA_32x32", ec.M32x32), ("MFMA_64x32", ec.M64x32), ("MFMA_32x64", ec.M32x64),
                         ("MFMA_64x64", ec.M64x64), ("WS", ec.WS), ("BF16", ec.BF16), ("MFMA_OTHER", ec.WIDE), ("FIRST_MFMA", 9),
                         ("LDS", N.KCLASS_LDS), ("MIXED", 32)):
        assert re.search(r"#define RCA_KCLASS_%s %d\b" % (macro, value), text), macro
    assert ec.FIRST == 9 and ec.MIXED == 32


def test_no_large_case_leaves_a_seam_row_or_an_affordable_row_unchecked():
    for c in ec.cases():
        pcm = ec.pcm_input(c)
        rows = ec.oracle_rows(c.config, c.layer, pcm, c.B, c.Lin, ec.extra_rows(c.config, c.layer, pcm, c.B, c.Lin))
        assert set(ec.seam_rows(c)) <= set(rows), c
        if len(rows) != c.B:
            assert ec.macs(c.config, c.layer, pcm, c.B, c.Lin) > ec.GMAC_ALL_ROWS and {0, 1, c.B // 2, c.B - 2, c.B - 1} <= set(rows), c


# ------------------------------------------------------------------------------------------------ the references
@pytest.mark.parametrize("name", sorted(ec._CONFIGS))
def test_oracle_layers_chain_to_the_oracle_taps_and_stay_within_the_fma_bound(name):
    cfg = ec.config(name)[0]
    B, T = (2, 2 * cfg.hop - 37) if name != "full" else (1, cfg.hop + 11)
    pcm = ec.make_input(name, 0, True, B, T, "signed")
    oc = ec.oracle_codec(name)
    prev = oc.encode(pcm, tap_layer=0)[1]
    for layer in range(1, ec.n_layers(name)):
        ly = ec.layer_of(name, layer)
        tap = oc.encode(pcm, tap_layer=layer)[1]
        got = ec.oracle_layer(name, layer, prev)
        assert np.array_equal(got, tap), (name, layer)
        y64, m = ec.ref64(name, layer, prev)
        ratio = np.abs(got.astype(np.float64) - y64) / ec.fma_bound(ly, m)
        assert ratio.max() <= 1.0, (name, layer, float(ratio.max()))
        prev = tap


@pytest.mark.parametrize("name,layer", [("tiny", 2), ("odd", 3), ("tiny", 5), ("f168", 1)])
def test_the_hand_off_identities_hold_bit_for_bit(name, layer):
    ly = ec.layer_of(name, layer)
    x = ec.make_input(name, layer, False, 3, 3 * ec.frame_mult(name, layer), "signed")
    assert (x == 0).any() and np.signbit(x[x == 0]).any() and not np.signbit(x[x == 0]).all() and (x < 0).any() and (x > 0).any()
    y = ec.oracle_layer(name, layer, x, pre=True)
    assert np.array_equal(y, ec.oracle_layer(name, layer, ec.leaky(name, x), pre=False))
    slope = np.float32(ec.config(name)[0].leaky_slope)
    assert np.array_equal(ec.leaky(name, y), np.where(y >= 0, y, slope * y))


def test_teeth_each_fault_changes_a_compared_element():
    """on the test's own inputs: the references would not pass a kernel with one of these faults"""
    for c in ec.cases():
        if c.group not in ("small", "view") or c.kind != "signed" or c.config not in ("tiny", "odd"):
            continue
        x, rows, want = ec.reference(c.config, c.layer, False, c.B, c.Lin, c.kind)
        assert len(rows) == c.B
        ly = ec.layer_of(c.config, c.layer)
        if c.flags & 1:      # the activation applied twice: the kernel re-activates an input that already is
            twice = ec.oracle_layer(c.config, c.layer, ec.leaky(c.config, x), pre=True)
            assert not np.array_equal(twice, want), c
        if c.flags & 2:      # the activated store dropped
            assert not np.array_equal(ec.expected(c, want), want[:, :, -c.view:] if c.view else want), c
        if c.view:           # the view one column to the left
            assert not np.array_equal(want[:, :, -c.view - 1:-1], ec.expected(c._replace(flags=0), want)), c
            whole = ec.view_reference(c._replace(flags=0), x)
            assert np.array_equal(whole[:, :, 1:], want[:, :, -c.view + 1:]) and not np.array_equal(whole[:, :, 0], want[:, :, -c.view])
        if c.flags == 0 or c.view:
            continue
        # a zero pad replaced by the neighbouring row's sample: the rows laid end to end as one row
        cat = np.ascontiguousarray(x.transpose(1, 0, 2).reshape(1, ly["cin"], c.B * c.Lin))
        run = ec.oracle_layer(c.config, c.layer, cat).reshape(ly["cout"], c.B, -1).transpose(1, 0, 2)
        assert not np.array_equal(run, want), c
        assert not np.array_equal(run[:, :, 0], want[:, :, 0]) or not np.array_equal(run[:, :, -1], want[:, :, -1]), c


def test_impulse_cases_are_bias_plus_single_taps():
    for c in ec.cases():
        if c.kind.startswith("imp") and c.layer > 0 and c.route == 0 and c.variant == 1 and c.config == "tiny":
            _, _, want = ec.reference(c.config, c.layer, False, c.B, c.Lin, c.kind)
            b = ec.layer_weights(c.config, c.layer)[1]
            assert (want[:-1] == b[None, :, None]).all() and (want[-1] != b[:, None]).any(), c


# ------------------------------------------------------------------------------------------------ the entry point
CTYPES = {"rca_codec_t*": C.c_void_p, "int32_t": C.c_int32, "int64_t": C.c_int64, "int32_t*": C.POINTER(C.c_int32),
          "float*": C.POINTER(C.c_float)}


def _declared_args(sym):
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    args = re.search(r"\bint %s\((.*?)\);" % sym, text, re.S).group(1)
    out = []
    for a in args.split(","):
        m = re.match(r"\s*(?:const\s+)?(\w+)\s*(\*?)\s*(\w+)\s*$", a)
        out.append((m.group(3), CTYPES[m.group(1) + m.group(2)]))
    return out


def test_the_tap_prototype_matches_the_header():
    want = _declared_args("rca_codec_encoder_layer_tap")
    assert [n for n, _ in want] == ["h", "layer", "route", "flags", "view", "x_host", "B", "Lin", "y_host", "y_numel", "kernel_class",
                                    "post_done", "guards_ok"]
    assert len(N.ENCODER_LAYER_TAP_ARGTYPES) == len(want)
    for (name, t), got in zip(want, N.ENCODER_LAYER_TAP_ARGTYPES):
        assert got is t, (name, got, t)


def test_the_tap_is_an_abi_symbol_bound_and_exported():
    assert "rca_codec_encoder_layer_tap" in N.ABI_SYMBOLS
    if N.needs_build():
        N.build()
    f = N.lib().rca_codec_encoder_layer_tap
    assert list(f.argtypes) == N.ENCODER_LAYER_TAP_ARGTYPES and f.restype is C.c_int
    # a null argument is refused before any HIP call (this machine may have no GPU at all)
    x = (C.c_float * 4)()
    k = C.c_int32()
    assert f(None, 0, 0, 0, 0, x, 1, 1, x, 4, C.byref(k), C.byref(k), C.byref(k)) == -1
    assert b"encoder_layer_tap: null argument" in N.lib().rca_last_error()


def test_encoder_layer_tap_wrapper_signature():
    import inspect
    from realtime_codec_agent_amd.codec import HipCodec
    assert list(inspect.signature(HipCodec.encoder_layer_tap).parameters)[1:] == ["layer", "route", "x", "flags", "view"]
