"""The references and tables of the layer-by-layer decoder tests, checked without a GPU (tests/dec_cases.py):
  * the C oracle's per-layer functions against float64 on every input the GPU file uses, within the fma-chain bound
    (K + 1) 2^-24 m (derived in dec_cases, not measured; on the four `up` layers of the full model the error reaches about 5 % of it);
  * every threshold case against the class inequality it claims, in plain integers;
  * the clamp cases really clamp, on both sides, and leave a share unclamped;
  * the prototype of rca_codec_decoder_layer_tap against its declaration in include/rca.h."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import dec_cases as dc
from realtime_codec_agent_amd import _native as N

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "rca.h")


def _layer_keys():
    return sorted({(k[0], k[1]) for k in dc.input_keys()})


@pytest.mark.parametrize("name,layer", _layer_keys(), ids=lambda v: str(v))
def test_oracle_layers_stay_within_the_fma_bound_of_float64(name, layer):
    ly = dc.layer_of(name, layer)
    worst = 0.0
    for key in dc.input_keys():
        if key[:2] != (name, layer):
            continue
        _, _, B, Lin, kind = key
        x = dc.make_input(*key)
        rows = dc.oracle_rows(ly, B, Lin)
        xr = x if len(rows) == B else x[rows]
        y32 = dc.oracle_layer(name, layer, xr, clamp=False)
        y64, m = dc.ref64(name, layer, xr)
        assert y32.shape == y64.shape and np.isfinite(y32).all()
        ratio = np.abs(y32.astype(np.float64) - y64) / dc.fma_bound(ly, m)
        assert ratio.max() <= 1.0, (key, float(ratio.max()), np.unravel_index(ratio.argmax(), ratio.shape))
        worst = max(worst, float(ratio.max()))
        if kind.startswith("imp"):      # bias plus single taps: one rounding per fma, and most of the output is the bias alone
            assert (y32[:-1] == dc.layer_weights(name, layer)[1][None, :, None]).all()
    print(f"{name} layer {layer}: worst error / bound = {worst:.3f}")


def test_the_float64_reference_agrees_with_a_direct_loop():
    """ref64 itself, on shapes small enough for the definition written out index by index"""
    for name, layer, B, Lin in (("tiny", 0, 2, 5), ("tiny", 2, 2, 3), ("odd", 4, 1, 4), ("tiny", 5, 1, 9)):
        ly, (w, b) = dc.layer_of(name, layer), dc.layer_weights(name, layer)
        x = dc.make_input(name, layer, B, Lin, "normal")
        slope = np.float32(dc.config(name)[0].leaky_slope)
        xa = np.where(x >= 0, x, x * slope).astype(np.float64) if ly["pre"] else x.astype(np.float64)
        k, s = ly["k"], ly["s"]
        pad = (k - s + 1) // 2
        Lout = Lin * s if ly["tr"] else Lin // s
        want = np.zeros((B, ly["cout"], Lout))
        for bi in range(B):
            for co in range(ly["cout"]):
                for u in range(Lout):
                    acc = float(b[co])
                    for ci in range(ly["cin"]):
                        for kk in range(k):
                            if ly["tr"]:
                                if (u + pad - kk) % s == 0 and 0 <= (u + pad - kk) // s < Lin:
                                    acc += float(w[ci, co, kk]) * xa[bi, ci, (u + pad - kk) // s]
                            elif 0 <= u * s + kk - pad < Lin:
                                acc += float(w[co, ci, kk]) * xa[bi, ci, u * s + kk - pad]
                    want[bi, co, u] = acc
        got, m = dc.ref64(name, layer, x)
        assert np.abs(got - want).max() <= 1e-12 * m.max(), (name, layer)


def test_threshold_cases_satisfy_the_inequality_they_claim():
    for name, layer, B, Lin, product, kclass in dc.TR_THRESHOLD:
        ly = dc.layer_of(name, layer)
        assert ly["tr"] and ly["cout"] > 32
        assert dc.cdiv(B * (Lin + 1), 64) * dc.cdiv(ly["cout"], 64) * ly["s"] == product
        assert (kclass == dc.M64x64) == (product >= 2048) and kclass in (dc.M64x64, dc.M32x32)
        assert dc.route0_class(ly, B, Lin, 1) == kclass
    assert {p for *_, p, _ in dc.TR_THRESHOLD} >= {2048, 2032}      # the threshold itself and one tile below it
    ly = dc.layer_of("full", 0)
    assert (ly["cin"], ly["cout"], ly["k"], ly["s"]) == (16, 512, 3, 1)
    for B, Lin, variant, waves, kclass in dc.CONV_IN_R0:
        assert dc.cdiv(B * Lin, 64) * 8 == waves
        want = (dc.CHAIN if variant == 0 else dc.WS if variant == 2 and waves >= 1024 else dc.M64x64 if waves >= 8192 else
                dc.M32x64 if waves >= 2048 else dc.M64x32 if waves >= 1024 else dc.M32x32)
        assert kclass == want == dc.route0_class(ly, B, Lin, variant), (B, Lin, variant)
    waves = {w for *_, w, _ in dc.CONV_IN_R0}
    assert waves >= {1024, 2048, 8192} and any(1024 - 8 <= w < 1024 for w in waves)      # each class exactly at its threshold ...
    assert any(2048 - 8 <= w < 2048 for w in waves) and any(8192 - 32 <= w < 8192 for w in waves)   # ... and just under it
    # the sweep: a tile of 32 columns exactly full and one over, per row and for three rows
    assert {Lin + 1 for _, Lin in dc.TR_SWEEP_SHAPES} >= {2, 3, 32, 33, 64, 65}
    # route 1: only what decode_tail can launch, and both staging branches of conv_in (Lin % 4 == 0 and != 0)
    assert all(B * F <= dc.LAT_MAX_FRAMES for B, F in dc.ROUTE1_FRAMES + dc.ROUTE1_FIT_FRAMES)
    assert {F % 4 == 0 for _, F in dc.ROUTE1_FRAMES} == {True, False}
    for c in dc.cases():
        if c.route == 1:
            assert c.Lin % dc.frame_mult(c.config, c.layer) == 0 and c.variant >= 1
    assert {c.kclass for c in dc.cases() if c.config == "odd" and c.route == 1 and c.layer == 4} == {dc.M32x32}   # Cin = 10: declined
    assert {c.kclass for c in dc.cases() if c.group == "route1_fit"} == {dc.LDS1, dc.LDS2, dc.LDS4}


def test_the_tables_reach_every_documented_class_and_never_bf16():
    assert {c.kclass for c in dc.cases()} == dc.DECODER_CLASSES and dc.BF16 not in dc.DECODER_CLASSES
    text = open(HEADER).read()
    for macro, value in (("CHAIN", dc.CHAIN), ("MFMA_32x32", dc.M32x32), ("MFMA_64x32", dc.M64x32), ("MFMA_32x64", dc.M32x64),
                         ("MFMA_64x64", dc.M64x64), ("WS", dc.WS), ("BF16", dc.BF16), ("LDS", N.KCLASS_LDS)):
        assert re.search(r"#define RCA_KCLASS_%s %d\b" % (macro, value), text), macro


@pytest.mark.parametrize("name", ["full", "tiny"])
def test_clamp_inputs_clamp_on_both_sides_and_not_everywhere(name):
    """on the oracle's UNCLAMPED conv_out output: at least 5 % above +1, 5 % below -1 and 25 % inside, over the config's clamp cases;
    every single case has all three kinds"""
    n = len(dc.config(name)[0].decoder_layers())
    keys = [k for k in dc.input_keys() if k[0] == name and k[4] == "clamp"]
    assert keys and all(k[1] == n - 1 for k in keys)
    above = below = total = 0
    for key in keys:
        y = dc.oracle_layer(name, n - 1, dc.make_input(*key), clamp=False)
        assert (y > 1).any() and (y < -1).any() and (np.abs(y) < 1).any(), key
        above, below, total = above + int((y > 1).sum()), below + int((y < -1).sum()), total + y.size
    print(f"{name}: {above / total:.1%} above +1, {below / total:.1%} below -1, {1 - (above + below) / total:.1%} inside")
    assert above >= 0.05 * total and below >= 0.05 * total and total - above - below >= 0.25 * total


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
    want = _declared_args("rca_codec_decoder_layer_tap")
    assert [n for n, _ in want] == ["h", "layer", "route", "x_host", "B", "Lin", "y_host", "y_numel", "kernel_class", "guards_ok"]
    assert len(N.DECODER_LAYER_TAP_ARGTYPES) == len(want)
    for (name, t), got in zip(want, N.DECODER_LAYER_TAP_ARGTYPES):
        assert got is t, (name, got, t)


def test_the_tap_is_an_abi_symbol_bound_and_exported():
    assert "rca_codec_decoder_layer_tap" in N.ABI_SYMBOLS
    if N.needs_build():
        N.build()
    lib = N.lib()
    assert hasattr(lib, "rca_codec_decoder_layer_tap")
    f = lib.rca_codec_decoder_layer_tap
    assert list(f.argtypes) == N.DECODER_LAYER_TAP_ARGTYPES and f.restype is C.c_int
    # a null argument is refused before any HIP call (this machine may have no GPU at all)
    x = (C.c_float * 4)()
    k = C.c_int32()
    assert f(None, 0, 0, x, 1, 1, x, 4, C.byref(k), C.byref(k)) == -1 and b"decoder_layer_tap: null argument" in lib.rca_last_error()


def test_decoder_layer_tap_wrapper_signature():
    import inspect
    from realtime_codec_agent_amd.codec import HipCodec
    assert list(inspect.signature(HipCodec.decoder_layer_tap).parameters)[1:] == ["layer", "route", "x"]
