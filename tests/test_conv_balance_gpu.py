"""Mixed-tile conv grids (conv1d_mfma_mixed_kernel): whole rounds of resident waves on the bulk wave tile, the remaining columns
on finer tiles at the end of the same grid.  A wave tile changes which wave computes an output, never its fma chain, so every plan
must give the bits of the single-shape grid (RCA_CONV_BALANCE=0), which the existing tests pin to the C oracle.

RCA_CONV_BALANCE and RCA_CONV_BALANCE_PLAN are read per call, so the tests switch them around single calls of one codec."""
import contextlib
import os

import numpy as np
import pytest
import torch

from conftest import rich_signal

pytestmark = pytest.mark.gpu


@contextlib.contextmanager
def conv_env(balance=None, plan=None):
    keys = {"RCA_CONV_BALANCE": balance, "RCA_CONV_BALANCE_PLAN": plan}
    old = {k: os.environ.get(k) for k in keys}
    try:
        for k, v in keys.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


@pytest.fixture(scope="module")
def hip(full_codec):
    from realtime_codec_agent_amd.codec import HipCodec
    return HipCodec(*full_codec, device=0)


def _rows(B, T, seed):
    # one long modulated-noise signal cut into rows: every row differs, generated once
    return np.ascontiguousarray(rich_signal(B * T, seed).reshape(B, T))


# ---------------------------------------------------------------- seams against the C oracle, on the cheapest layer
# 3 rows of 176 000 samples: the k8s4 layer has 3 x 22 000 = 66 000 columns = 1 032 column tiles of 64 (32 x 64 class: 2 064 waves of
# 64 x 64); 22 000 is no multiple of 64, so tiles straddle rows.
@pytest.fixture(scope="module")
def seam_case(full_oracle):
    x = _rows(3, 176000, 31)
    _, want = full_oracle.encode(x, tap_layer=2)
    want.setflags(write=False)
    return x, want


@pytest.mark.parametrize("plan", ["512:32x32", "0:32x32", "1032:32x32", "1024:32x32"])
def test_seam_against_the_oracle(hip, seam_case, plan):
    """512: seam in the middle of row 1; 0: all fine tiles; 1032: no remainder (the plain launch); 1024: the remainder is the last 8
    column tiles with the ragged final one."""
    x, want = seam_case
    assert want.shape == (3, 128, 22000)
    with conv_env(plan=plan):
        got = hip.encode_tap(x, 2)
    bad = np.flatnonzero(got.ravel() != want.ravel())
    assert bad.size == 0, f"plan {plan}: {bad.size} mismatches, first at {bad[:5]}"


def test_unbalanced_and_automatic_plan_against_the_oracle(hip, seam_case):
    x, want = seam_case
    with conv_env(balance="0"):
        assert np.array_equal(hip.encode_tap(x, 2), want)
    with conv_env():
        assert np.array_equal(hip.encode_tap(x, 2), want)


# ---------------------------------------------------------------- every tile class at once, against the single-shape launch
# 16 rows of 330 240 samples (1 032 frames): k16s8 258 column tiles / 2 064 waves of 64 x 64 (32 x 64 class), k10s5 2 064 / 8 256
# (64 x 64 class), k8s4 10 320 / 20 640 (64 x 64 class).  The reference is the RCA_CONV_BALANCE=0 path (the oracle would take minutes).
@pytest.fixture(scope="module")
def class_case(hip):
    x = _rows(16, 330240, 47)
    with conv_env(balance="0"):
        ref = {layer: hip.encode_tap(x, layer) for layer in (2, 3, 4)}
        ref["ids"] = hip.encode(x)
    for v in ref.values():
        v.setflags(write=False)
    assert ref[2].shape == (16, 128, 41280) and ref[3].shape == (16, 256, 8256) and ref[4].shape == (16, 512, 1032)
    return x, ref


def test_automatic_plan_equals_single_shape_launch(hip, class_case):
    x, ref = class_case
    with conv_env():
        for layer in (2, 3, 4):
            assert np.array_equal(hip.encode_tap(x, layer), ref[layer]), layer
        assert np.array_equal(hip.encode(x), ref["ids"])


# one seam per layer, inside a row (bulk column tiles x 64 columns is no multiple of the row length), for both fine shapes.  The k16s8
# layer runs 32 x 64 bulk tiles here, for which 32 x 64 is no finer tile: its only remainder shape is 32 x 32.
@pytest.mark.parametrize("layer,plan", [(2, "5000:32x64"), (2, "5000:32x32"), (3, "1000:32x64"), (3, "1000:32x32"), (4, "128:32x32")])
def test_forced_seam_equals_single_shape_launch(hip, class_case, layer, plan):
    x, ref = class_case
    bulk = int(plan.split(":")[0])
    assert (bulk * 64) % ref[layer].shape[2] != 0
    with conv_env(plan=plan):
        got = hip.encode_tap(x, layer)
        ids = hip.encode(x) if layer == 4 else None
    assert np.array_equal(got, ref[layer]), (layer, plan)
    if ids is not None:
        assert np.array_equal(ids, ref["ids"])


# ---------------------------------------------------------------- the headline shape
def test_headline_pass_ids_equal_and_repeatable(hip):
    """One 256-window pass of encode_chunk_range_dev, as the benchmark makes it: ids with the automatic plan equal the single-shape
    launch's, and two runs of the automatic plan give the same ids (the grid depends on shapes and device properties only)."""
    C, chunk, ctx, B = 2, 1600, 32000, 256
    per = B // C
    first = ctx // chunk
    N = (first + per) * chunk
    g = torch.Generator(device="cpu").manual_seed(3)
    audio = (0.1 * torch.randn(C, N, generator=g)).to("cuda:0").contiguous()
    fpc = hip.frames_per_chunk(chunk)
    st = torch.cuda.current_stream().cuda_stream

    def run():
        codes = torch.full((C, per * fpc), -1, dtype=torch.int64, device="cuda:0")
        hip.encode_chunk_range_dev(audio.data_ptr(), C, N, chunk, ctx, B, first, first + per, codes.data_ptr(), codes.shape[1], st)
        torch.cuda.synchronize()
        return codes

    with conv_env(balance="0"):
        ref = run()
    with conv_env():
        a, b = run(), run()
    assert int(ref.min()) >= 0
    assert torch.equal(a, ref)
    assert torch.equal(a, b)
