"""The f32 encoder layer by layer against the C oracle, as an encode pass launches it (MI355X).

rca_codec_encode_tap switches the production path off: a tapped pass runs without the LeakyReLU hand-off between layers, without the
kept-frames view of conv_out and, for layer 0, without the fused first layer.  rca_codec_encoder_layer_tap runs ONE layer through the
code a pass uses -- the hand-off flags, the view, the fusion, the streaming tail's latency launch -- on the inputs of
tests/enc_cases.py.  Every case is compared with the oracle bit for bit (np.array_equal, no tolerance anywhere in this file), must
leave the guard floats around the output alone, must write every element (the output starts as NaN), must report whether it stored the
activated output and must report the kernel class the table expects, so a case cannot pass on another kernel than the one it is aimed
at.  Where a case is too large for the CPU oracle the GPU runs all batch rows and the oracle the rows enc_cases.oracle_rows names
(first, middle, last and both sides of every forced seam); the other rows are still checked for NaN and the guards.
Then the production sequence itself (rca_codec_encoder_dev) at the benchmark's batch and at B = 40 against the oracle's z_e, under the
automatic plan, the single-shape grids and one forced seam per mixed layer.  test_encoder_layers_cpu.py checks the tables and
references."""
import contextlib
import os

import numpy as np
import pytest

import enc_cases as ec
from conftest import bench_signal, rich_signal

pytestmark = pytest.mark.gpu

SEEN = set()      # every kernel class a tap reported in this run
RAN = set()       # the groups of enc_cases.groups() that ran to their end
ENV_KEYS = ("RCA_CONV_BALANCE", "RCA_CONV_BALANCE_PLAN", "RCA_FUSE_MFMA_IN", "RCA_HEAD_KEEP")


@contextlib.contextmanager
def env(pairs=()):
    """the switches a pass reads per call, set around single calls and restored; a switch not named is unset"""
    want = dict(pairs)
    old = {k: os.environ.get(k) for k in ENV_KEYS}
    try:
        for k in ENV_KEYS:
            if k in want:
                os.environ[k] = want[k]
            else:
                os.environ.pop(k, None)
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


@pytest.fixture(scope="module")
def hips(tiny_codec, full_codec):
    from realtime_codec_agent_amd.codec import HipCodec
    made = {}

    def get(name):
        if name not in made:
            cfg, w = {"tiny": tiny_codec, "full": full_codec}.get(name) or ec.config(name)
            ref_w = ec.config(name)[1]      # what the references of enc_cases are computed with
            assert all(np.array_equal(w[k], ref_w[k]) for k in ref_w if k.startswith("enc."))
            made[name] = HipCodec(cfg, w, device=0)
        return made[name]

    yield get
    for h in made.values():
        h.close()


def _run_case(hip, c):
    x, rows, want = ec.reference(c.config, c.layer, ec.pcm_input(c), c.B, c.Lin, c.kind)
    with env(c.env):
        got, kclass, post, guards = hip.encoder_layer_tap(c.layer, c.route, ec.tap_input(c, x), c.flags, c.view)
    SEEN.add(kclass)
    assert guards, f"{c}: a guard float next to the output changed"
    assert not np.isnan(got).any(), f"{c}: {int(np.isnan(got).sum())} of {got.size} elements not written (or NaN)"
    assert kclass & ~ec.MIXED == c.kclass, f"{c}: ran kernel class {kclass}"
    if c.mixed is not None:      # None: the automatic plan decides whether the launch is the mixed grid
        assert bool(kclass & ec.MIXED) == c.mixed, f"{c}: ran kernel class {kclass}"
    assert post == ec.post_expected(c), f"{c}: post_done {post}"
    sub = got if len(rows) == c.B else got[rows]
    if c.view:
        # the kept columns against the full row of the oracle; the whole view, halo included, against the row cut at its left edge
        halo = ec.view_halo(ec.layer_of(c.config, c.layer))
        msg = ec.first_mismatch(sub[:, :, halo:], ec.expected(c, want)[:, :, halo:])
        assert not msg, f"{c} (rows {rows if len(rows) != c.B else 'all'}), kept columns: {msg}"
        msg = ec.first_mismatch(sub, ec.view_reference(c, x if len(rows) == c.B else x[rows]))
        assert not msg, f"{c}, whole view: {msg}"
    else:
        msg = ec.first_mismatch(sub, ec.expected(c, want))
        assert not msg, f"{c} (rows {rows if len(rows) != c.B else 'all'}): {msg}"
    return got


@pytest.mark.parametrize("key", ec.groups(), ids=lambda k: "-".join(str(v) for v in k))
def test_layer_against_the_oracle(key, hips):
    """(table, config, layer, route, variant): every shape, flag set, plan and input kind of that group"""
    hip = hips(key[1])
    hip.set_variant(key[4])
    try:
        outs = {}
        for c in ec.cases_of(key):
            got = _run_case(hip, c)
            if c.group in ("forced", "unbalanced", "threshold") and c.B * c.Lin > 100000:
                # a forced seam, the automatic plan and the single-shape grid of one input and flag set: equal over ALL rows
                prev = outs.setdefault((c.B, c.Lin, c.flags), got)
                assert prev is got or np.array_equal(prev, got), c
        RAN.add(tuple(key))
    finally:
        hip.set_variant(1)


def test_mixed_grid_equals_its_single_shape_twin_on_every_row(hips):
    """every forced seam of the balanced layers against the RCA_CONV_BALANCE=0 launch of the same input, all rows, both flags set"""
    hip = hips("tiny")
    for name, layer, w in sorted({f[:3] for f in ec.FORCED}):
        B, Lin = ec.shape_for(name, layer, w)
        xin = ec.leaky(name, ec.make_input(name, layer, False, B, Lin, "signed"))
        with env({"RCA_CONV_BALANCE": "0"}):
            ref, k0, _, g0 = hip.encoder_layer_tap(layer, 0, xin, 3)
        assert g0 and not k0 & ec.MIXED and not np.isnan(ref).any(), (name, layer, w, k0)
        for plan in [f[3] for f in ec.FORCED if f[:3] == (name, layer, w)]:
            with env({"RCA_CONV_BALANCE_PLAN": plan}):
                got, k1, _, g1 = hip.encoder_layer_tap(layer, 0, xin, 3)
            assert g1 and np.array_equal(ref, got), (name, layer, w, plan, k1)


# ------------------------------------------------------------------------------------------------ refusals
def test_the_tap_refuses_what_an_encode_pass_cannot_launch(hips):
    from realtime_codec_agent_amd._native import RcaError
    hip = hips("tiny")
    n = hip.cfg.n_stages
    tap = hip.encoder_layer_tap
    x2 = ec.make_input("tiny", 2, False, 3, 3 * 160, "signed")                 # enc.down.1: 160 samples per frame
    got, kclass, post, guards = tap(2, 0, ec.leaky("tiny", x2), 3)
    assert guards and post and kclass == ec.M32x32 and got.shape == (3, 8, 120)

    def refused(*a, **kw):
        with pytest.raises(RcaError):
            tap(*a, **kw)

    pcm = ec.make_input("tiny", 0, True, 3, 700, "normal")
    x1 = ec.make_input("tiny", 1, False, 3, 640, "normal")
    x5 = ec.make_input("tiny", 5, False, 3, 9, "normal")
    refused(0, 0, pcm, 1)                        # flag 1: conv_in has no pre-activation
    refused(0, 0, pcm, 2)                        # flag 2: conv_in_kernel never stores an activated output
    refused(1, 0, x1, 1)                         # flag 1 on layer 1: neither of its producers stores one
    refused(n + 1, 0, x5, 2)                     # flag 2 on the last layer: nothing follows it
    refused(2, 0, pcm, 4)                        # flag 4 on another layer than 1
    refused(1, 0, pcm, 5)                        # flag 4 with flag 1
    assert tap(1, 0, ec.make_input("tiny", 1, True, 3, 100, "signed"), 6)[1] == ec.M32x32     # one frame of k4s2 is 160 columns: fused ...
    f168 = hips("f168")
    refused_f = lambda *a: pytest.raises(RcaError, f168.encoder_layer_tap, *a)
    refused_f(1, 0, ec.make_input("f168", 1, True, 3, 320, "normal"), 4)     # ... one frame of k16s8 is 40 columns < 67: not fused
    refused_k = lambda name: pytest.raises(RcaError, hips(name).encoder_layer_tap, 1, 0, ec.make_input(name, 1, True, 3, 3200, "normal"), 4)
    refused_k("k105")                            # a k10s5 first layer is never fused
    refused_k("kin3")                            # nor one behind a 3-tap conv_in
    refused(n + 1, 0, x5, 0, 1)                  # a view of the halo alone: no pass keeps 0 frames
    refused(n + 1, 0, x5, 0, 9)                  # a view of the whole row
    refused(n, 0, ec.make_input("tiny", n, False, 3, 72, "normal"), 0, 2)    # a view on another layer
    refused(n + 1, 1, x5, 0, 2)                  # a view on route 1
    with env({"RCA_HEAD_KEEP": "0"}):
        refused(n + 1, 0, x5, 0, 2)              # RCA_HEAD_KEEP=0: the pass computes the whole row
    for flags in (1, 2, 3):
        refused(2, 1, ec.leaky("tiny", x2), flags)                             # any flag on route 1
    refused(2, 1, ec.make_input("tiny", 2, False, 5, 13 * 160, "normal"))     # route 1: 65 frames run on the throughput kernels
    refused(0, 1, ec.make_input("tiny", 0, True, 5, 13 * 320 - 5, "normal"))
    refused(2, 0, ec.make_input("tiny", 2, False, 3, 3 * 160 - 40, "normal"))  # no whole number of frames
    import ctypes as C
    k, p, g = C.c_int32(), C.c_int32(), C.c_int32()
    fp = C.POINTER(C.c_float)
    y = np.empty(got.size + 1, np.float32)
    call = lambda layer, route, flags, view, B, Lin, numel: hip._lib.rca_codec_encoder_layer_tap(
        hip._h, layer, route, flags, view, x2.ctypes.data_as(fp), B, Lin, y.ctypes.data_as(fp), C.c_int64(numel), C.byref(k), C.byref(p),
        C.byref(g))
    assert call(2, 0, 0, 0, 3, 480, got.size) == 0
    for bad in ((-1, 0, 0, 0, 3, 480, got.size), (n + 2, 0, 0, 0, 3, 480, got.size), (2, 2, 0, 0, 3, 480, got.size),
                (2, -1, 0, 0, 3, 480, got.size), (2, 0, 8, 0, 3, 480, got.size), (2, 0, -1, 0, 3, 480, got.size),
                (2, 0, 0, -1, 3, 480, got.size), (2, 0, 0, 0, 0, 480, got.size), (2, 0, 0, 0, 3, 0, got.size),
                (2, 0, 0, 0, 3, 480, got.size + 1), (2, 0, 0, 0, 3, 480, got.size - 1),
                (2, 0, 0, 0, 1 << 20, 160 * 1024, (1 << 20) * 8 * 40 * 1024)):          # more than 2^30 elements
        assert call(*bad) == -1, bad
    hip.set_variant(0)
    try:
        refused(2, 1, x2)                        # route 1 exists from variant 1 on
        refused(2, 0, ec.leaky("tiny", x2), 1)   # the hand-off is the default variant's
        refused(2, 0, x2, 2)
        refused(n + 1, 0, x5, 0, 2)              # and so is the view
    finally:
        hip.set_variant(1)
    hip.set_variant(2)
    try:
        refused(2, 0, x2, 2)
    finally:
        hip.set_variant(1)
    assert np.array_equal(tap(2, 0, ec.leaky("tiny", x2), 3)[0], got)


# ------------------------------------------------------------------------------------------------ the production sequence
def _headline_rows(B, T):
    """B rows of T samples: amplitude-modulated noise and the benchmark's sines, every row different"""
    x = np.ascontiguousarray(rich_signal(B * T, 23).reshape(B, T))
    for b in range(0, B, 7):
        x[b] = bench_signal(T, seed=b)
    return x


def _encoder_dev(hip, xd, B, T, pairs=()):
    import torch
    F = hip.num_frames(T)
    ze = torch.full((B, F, hip.cfg.latent_dim), float("nan"), dtype=torch.float32, device="cuda")
    with env(pairs):
        hip.encoder_dev(xd.data_ptr(), B, T, ze.data_ptr(), torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
    return ze


@pytest.mark.parametrize("B", [256, 40])
def test_the_production_sequence_against_the_oracle(B, hips, full_oracle):
    """rca_codec_encoder_dev, full model, default variant, B rows of 32 000 samples: the launches encode() makes, hand-off and fusion
    on.  B = 256 is the benchmark's batch: conv_first_mfma_kernel, then 64 x 64 tiles with the mixed grid on the three layers with
    k >= 8 and 64 x 32 on conv_out; at B = 40 only the first two layers leave the 32 x 32 class.  Six fixed rows and 18 seeded ones equal the oracle's z_e bit
    for bit, no row holds a NaN, and the automatic plan, the single-shape grids (RCA_CONV_BALANCE=0) and one forced seam inside a row
    per mixed layer give the same bits on every row."""
    import torch
    T = 32000
    hip = hips("full")
    hip.set_variant(1)
    ly = [ec.layer_of("full", i) for i in range(6)]
    L = [T, 16000, 4000, 800, 100, 100]
    classes = [ec.fuse_class("full", B, T, 1)] + [ec.enc_route0_class(ly[i], B, L[i - 1], 1) for i in range(2, 6)]
    assert classes == ([ec.FIRST, ec.M64x64, ec.M64x64, ec.M64x64, ec.M64x32] if B == 256 else
                       [ec.FIRST, ec.M64x64, ec.M32x32, ec.M32x32, ec.M32x32])
    x = _headline_rows(B, T)
    rng = np.random.default_rng(B)
    fixed = [0, 1, B // 2 - 1, B // 2, B - 2, B - 1]
    rows = sorted(set(fixed) | set(int(v) for v in rng.choice(np.setdiff1d(np.arange(B), fixed), 18, replace=False)))
    assert len(rows) == 24
    want = full_oracle.encode(x[rows], tap_layer=5)[1].transpose(0, 2, 1)           # [24][F][D]
    xd = torch.from_numpy(x).cuda()
    base = _encoder_dev(hip, xd, B, T)
    assert not torch.isnan(base).any()
    msg = ec.first_mismatch(base[rows].cpu().numpy(), want)
    assert not msg, msg
    # column tiles of 64 per mixed layer at B = 256: 16 000, 3 200 and 400; each plan puts one layer's seam inside a row
    plans = ["8008:32x64", "1608:32x32", "208:32x32"] if B == 256 else ["1256:32x32"]
    for pairs in [{"RCA_CONV_BALANCE": "0"}] + [{"RCA_CONV_BALANCE_PLAN": p} for p in plans]:
        got = _encoder_dev(hip, xd, B, T, pairs)
        assert torch.equal(got, base), pairs


def test_every_documented_class_ran_and_no_other():
    """the tables name every encoder class of rca.h (each case above asserts the class it reports); nothing this run saw lies outside
    them, and a run of the whole file saw them all"""
    assert SEEN <= ec.ENCODER_CLASSES, sorted(SEEN - ec.ENCODER_CLASSES)
    if RAN == {tuple(k) for k in ec.groups()}:
        assert SEEN == ec.ENCODER_CLASSES, sorted(ec.ENCODER_CLASSES - SEEN)
