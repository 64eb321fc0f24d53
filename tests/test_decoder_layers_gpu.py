"""The decoder layer by layer against the C oracle on every launch route (MI355X).

rca_codec_decoder_layer_tap runs ONE decoder layer through the launch logic of a decode pass (route 0) or of a streaming tail call
(route 1) on the inputs of tests/dec_cases.py.  Every case is compared with the oracle's layer function bit for bit (np.array_equal;
dec.conv_out after np.clip), must leave the guard floats around the output alone, must write every element (the output starts as
NaN) and must report the kernel class the table expects, so a case cannot pass on another kernel than the one it is aimed at.
Where a case is too large for the CPU oracle the GPU runs all batch rows and the oracle the rows dec_cases.oracle_rows names; the
other rows are still checked for NaN and the guards.  Then the whole decoder against the oracle at a batch that takes the 64 x 64
tiles and on both sides of the latency threshold, and the promise of rca.h that the mfma mode leaves the decoder alone.
test_decoder_layers_cpu.py pins the oracle's layer functions to float64."""
import numpy as np
import pytest

import dec_cases as dc

pytestmark = pytest.mark.gpu

SEEN = set()      # every kernel class a tap reported in this run
RAN = set()       # the groups of dec_cases.groups() that ran to their end


@pytest.fixture(scope="module")
def hips(tiny_codec, full_codec):
    from realtime_codec_agent_amd.codec import HipCodec
    made = {}

    def get(name):
        if name not in made:
            cfg, w = {"tiny": tiny_codec, "full": full_codec}.get(name) or dc.config(name)
            ref_w = dc.config(name)[1]      # what the references of dec_cases are computed with
            assert all(np.array_equal(w[k], ref_w[k]) for k in ref_w if k.startswith("dec."))
            made[name] = HipCodec(cfg, w, device=0)
        return made[name]

    yield get
    for h in made.values():
        h.close()


def _run_case(hip, c):
    x, rows, want = dc.reference(c.config, c.layer, c.B, c.Lin, c.kind)
    got, kclass, guards = hip.decoder_layer_tap(c.layer, c.route, x)
    SEEN.add(kclass)
    assert guards, f"{c}: a guard float next to the output changed"
    assert not np.isnan(got).any(), f"{c}: {int(np.isnan(got).sum())} of {got.size} elements not written (or NaN)"
    assert kclass == c.kclass, f"{c}: ran kernel class {kclass}"
    msg = dc.first_mismatch(got if len(rows) == c.B else got[rows], want)
    assert not msg, f"{c} (rows {rows if len(rows) != c.B else 'all'}): {msg}"
    if c.layer == len(dc.config(c.config)[0].decoder_layers()) - 1:
        assert np.abs(got).max() <= 1.0


@pytest.mark.parametrize("key", dc.groups(), ids=lambda k: "-".join(str(v) for v in k))
def test_layer_against_the_oracle(key, hips):
    """(table, config, layer, route, variant): every shape and input kind of that group"""
    hip = hips(key[1])
    hip.set_variant(key[4])
    try:
        for c in dc.cases_of(key):
            _run_case(hip, c)
        RAN.add(tuple(key))
    finally:
        hip.set_variant(1)


def test_the_tap_refuses_what_a_decode_pass_cannot_launch(hips):
    from realtime_codec_agent_amd._native import RcaError
    hip = hips("tiny")
    n = hip.cfg.n_stages
    x = dc.make_input("tiny", 2, 1, 8, "normal")                 # dec.up.1: 8 samples per frame
    got, kclass, guards = hip.decoder_layer_tap(2, 1, x)
    assert guards and kclass == dc.LDS4 and got.shape == (1, 8, 40)
    import ctypes as C
    k, g = C.c_int32(), C.c_int32()
    fp = C.POINTER(C.c_float)
    y = np.empty(got.size + 1, np.float32)
    call = lambda layer, route, B, Lin, numel: hip._lib.rca_codec_decoder_layer_tap(
        hip._h, layer, route, x.ctypes.data_as(fp), B, Lin, y.ctypes.data_as(fp), C.c_int64(numel), C.byref(k), C.byref(g))
    assert call(2, 1, 1, 8, got.size) == 0
    for bad in ((-1, 0, 1, 8, got.size), (n + 2, 0, 1, 8, got.size), (2, 2, 1, 8, got.size), (2, -1, 1, 8, got.size),
                (2, 0, 0, 8, got.size), (2, 0, 1, 0, got.size), (2, 0, 1, 8, got.size + 1), (2, 0, 1, 8, got.size - 1),
                (2, 1, 1, 7, 7 * 5 * 8)):                         # route 1: 7 samples are no whole number of frames
        assert call(*bad) == -1, bad
    with pytest.raises(RcaError):                                 # route 1: 65 frames run on the throughput kernels in production
        hip.decoder_layer_tap(0, 1, dc.make_input("tiny", 0, 5, 13, "normal"))
    hip.set_variant(0)
    try:
        with pytest.raises(RcaError):                             # route 1 exists from variant 1 on
            hip.decoder_layer_tap(2, 1, x)
    finally:
        hip.set_variant(1)
    assert np.array_equal(hip.decoder_layer_tap(2, 1, x)[0], got)


# ------------------------------------------------------------------------------------------------ the whole decoder
def _oracle_of(name, tiny_oracle, full_oracle):
    return {"tiny": tiny_oracle, "full": full_oracle}[name]


def test_batch_decode_on_the_64x64_tiles_against_the_oracle(hips, full_oracle):
    """full model, 257 rows of 16 frames: dec.up.0 (2208 waves) and dec.up.1 (5190) both run on 64 x 64 wave tiles"""
    B, F = 257, 16
    assert dc.route0_class(dc.layer_of("full", 1), B, F, 1) == dc.M64x64 and dc.route0_class(dc.layer_of("full", 2), B, F * 8, 1) == dc.M64x64
    codes = np.random.default_rng(11).integers(0, full_oracle.cfg.codebook_size, (B, F))
    got = hips("full").decode(codes)
    rows = [0, 1, 128, 255, 256]
    want = full_oracle.decode(codes[rows])
    assert got.shape == (B, F * 320) and not np.isnan(got).any()
    assert not dc.first_mismatch(got[rows][:, None, :], want[:, None, :])


@pytest.mark.parametrize("name", ["tiny", "full"])
@pytest.mark.parametrize("B,F", [(8, 8), (5, 13)])
def test_whole_tail_decode_on_both_sides_of_the_latency_threshold(name, B, F, hips, tiny_oracle, full_oracle):
    """n = F * hop keeps every frame: 8 x 8 = 64 frames run on the latency kernels, 5 x 13 = 65 on the throughput kernels"""
    import torch
    hip, oc = hips(name), _oracle_of(name, tiny_oracle, full_oracle)
    codes = np.random.default_rng(B * 100 + F).integers(0, oc.cfg.codebook_size, (B, F))
    want = oc.decode(codes)
    assert np.array_equal(hip.decode_tail(codes, F * hip.hop), want)
    ct = torch.from_numpy(codes).cuda()
    out = torch.full((B, F * hip.hop), float("nan"), device="cuda")
    hip.decode_tail_dev(ct.data_ptr(), B, F, F * hip.hop, out.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert not dc.first_mismatch(out.cpu().numpy()[:, None, :], want[:, None, :])


# ------------------------------------------------------------------------------------------------ the mfma mode
@pytest.mark.parametrize("mode", [1, 3])
def test_the_mfma_mode_leaves_the_decoder_alone(mode, hips):
    """include/rca.h on rca_codec_set_mfma_mode: "Decoder and streaming-tail kernels are not affected".  Before run_conv gave decoder
    layers mode 0, the route-0 conv_in taps reported the bf16 class here and decode() differed from mode 0 by up to 2.6e-3 (mode 1) and
    4.9e-6 (mode 3) on the MI355X; the latency route of decode_tail was the same in every mode."""
    hip = hips("full")
    rng = np.random.default_rng(mode)
    codes_a, codes_b = rng.integers(0, hip.cfg.codebook_size, (3, 100)), rng.integers(0, hip.cfg.codebook_size, (1, 12))
    base_a, base_b = hip.decode(codes_a), hip.decode_tail(codes_b, 1920)
    taps = [(0, 2, 5), (0, 33, 247), (1, 1, 12)]          # dec.conv_in: (route, B, Lin)
    base_taps = [hip.decoder_layer_tap(0, r, dc.reference("full", 0, B, Lin, "normal")[0]) for r, B, Lin in taps]
    try:
        hip.set_mfma_mode(mode)
        got_taps = [hip.decoder_layer_tap(0, r, dc.reference("full", 0, B, Lin, "normal")[0]) for r, B, Lin in taps]
        got_a, got_b = hip.decode(codes_a), hip.decode_tail(codes_b, 1920)
    finally:
        hip.set_mfma_mode(0)
        hip.set_variant(1)
    print(f"mode {mode}: conv_in classes {[k for _, k, _ in got_taps]} (mode 0: {[k for _, k, _ in base_taps]}), max |difference| decode "
          f"{float(np.abs(got_a - base_a).max()):.3e}, decode_tail {float(np.abs(got_b - base_b).max()):.3e}")
    for (y0, k0, g0), (y1, k1, g1), shape in zip(base_taps, got_taps, taps):
        assert k1 != dc.BF16 and k1 == k0 and g0 and g1, (shape, k0, k1)
        assert np.array_equal(y0, y1), shape
    assert np.array_equal(got_a, base_a), float(np.abs(got_a - base_a).max())
    assert np.array_equal(got_b, base_b), float(np.abs(got_b - base_b).max())


def test_every_documented_class_ran_and_no_other():
    """the tables name every decoder class of rca.h, bf16 excluded (each case above asserts the class it reports); nothing this run
    saw lies outside them, and a run of the whole file saw them all"""
    assert {c.kclass for c in dc.cases()} == dc.DECODER_CLASSES and dc.BF16 not in dc.DECODER_CLASSES
    assert SEEN <= dc.DECODER_CLASSES, sorted(SEEN - dc.DECODER_CLASSES)
    if RAN == {tuple(k) for k in dc.groups()}:
        assert SEEN == dc.DECODER_CLASSES, sorted(dc.DECODER_CLASSES - SEEN)
