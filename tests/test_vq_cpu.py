"""The search cases of tests/vq_cases.py checked on the host: the planted ties win by a margin no f32 rounding can close and the
oracle answers their lowest index, the identity quantizer hands rows and codebook through bit for bit, the stale-key sequence
has the score signs it claims, and under the dispatcher's split formula (restated in vq_cases.py, compared with the source
here) the planted pairs reach every merge seam of the matrix kernel."""
import os
import re

import numpy as np
import pytest

import vq_cases as vq
from conftest import ROOT

SIZES = [vq.SMALL_N, vq.LARGE_N]


def _planted_margins(case):
    """for every planted row: (lowest margin of the group over every other code, E of that row)"""
    rows = [r for r, _ in case.planted]
    s = vq.scores64(case.codebook, case.distinct[rows])
    E = vq.rounding_bound(case.codebook, case.distinct[rows])
    margins = np.empty(len(rows))
    for k, (_, group) in enumerate(case.planted):
        g = list(group)
        inside = s[k, g]
        assert np.all(inside == inside[0]), (case.name, group)            # exact duplicates score alike, to the bit
        rest = s[k].copy()
        rest[g] = -np.inf
        margins[k] = inside[0] - rest.max()
    return margins, E


@pytest.mark.parametrize("N", SIZES)
def test_planted_ties_are_sound(N):
    """families a and e: in exact float64 arithmetic the planted group beats every other code by more than 1000 E, so no
    rounding of the f32 chain can make another code win, and the oracle returns the group's lowest index"""
    worst = np.inf
    for case in vq.family_a(N) + [vq.mixed_case(N)]:
        margins, E = _planted_margins(case)
        worst = min(worst, margins.min())
        assert np.all(margins > 1000.0 * E), (case.name, margins.min(), E.max())
        want = np.array([min(g) for _, g in case.planted])
        rows = [r for r, _ in case.planted]
        assert np.array_equal(vq.oracle_ids(case)[rows], want), case.name
        if case.expected is not None:
            assert np.array_equal(case.expected[rows], want), case.name
    print(f"N={N}: worst planted margin {worst:.3f}")
    members = {c for case in vq.family_a(N) for _, g in case.planted if len(g) > 1 for c in g}
    unique = {g[0] for _, g in vq.group_case(N).planted if len(g) == 1}
    assert {0, N - 1} <= members and {0, N - 1} == unique                    # both ends: a tie member and a unique winner
    if N == vq.LARGE_N:                                                     # family e draws from the same rows: every one is used
        for R in vq.MANY_ROWS:
            case = vq.many_rows_case(R)
            assert case.index.shape == (R,) and set(case.index.tolist()) == set(range(case.distinct.shape[0]))


@pytest.mark.parametrize("N", SIZES)
def test_identity_quantizer_is_bit_exact(N):
    """in_proj = I / [I16 | 0] and codebook_proj = I with zero bias: the oracle's projected codebook is the planted one and
    z is the row, bit for bit (a -0.0 component would become +0.0: the cases hold none)"""
    import ctypes as C
    from oracle.codec import OracleCodec, _fp, lib
    case = vq.mixed_case(N)
    for D in (vq.J, 256) if N == vq.SMALL_N else (vq.J,):
        oc = OracleCodec(*vq.build_model(case.codebook, D))
        assert np.array_equal(oc.codebook().view(np.uint32), case.codebook.view(np.uint32))
        rows = vq.widen_rows(case.distinct, D) if D != vq.J else case.distinct
        z = np.empty((rows.shape[0], vq.J), np.float32)
        lib().oracle_linear(_fp(np.ascontiguousarray(rows)), C.c_long(rows.shape[0]), C.c_int(D), oc._wstruct.q_in_w, oc._wstruct.q_in_b,
                            C.c_int(vq.J), _fp(z))
        assert np.array_equal(z.view(np.uint32), case.distinct.view(np.uint32))
        assert np.array_equal(oc.quantize_rows(rows), vq.oracle_ids(case))
    for name, make in vq.BY_NAME.items():
        if f"_N{N}" in name and not name.startswith("c_"):
            d = make().distinct
            assert np.isfinite(d).all() and not np.any((d == 0) & np.signbit(d)), name


def test_quantize_rows_is_encode_without_the_encoder(tiny_codec, tiny_oracle):
    """quantize_rows(conv_out tap as rows) == the codes encode() gives: the new entry point is the old search"""
    from conftest import rich_signal
    cfg, _ = tiny_codec
    x = np.stack([rich_signal(3200, 3), rich_signal(3200, 4)])
    codes, ze = tiny_oracle.encode(x, tap_layer=cfg.n_stages + 1)
    rows = np.ascontiguousarray(ze.transpose(0, 2, 1).reshape(-1, cfg.latent_dim))
    assert np.array_equal(tiny_oracle.quantize_rows(rows).reshape(codes.shape), codes)


@pytest.mark.parametrize("N", [vq.SMALL_N])
def test_signed_zero_and_nan_rows_on_the_oracle(N):
    """family c as the oracle sees it: the two scores are -0.0 and +0.0, the answer is the lower index either way; NaN -> 0"""
    for mirror in (False, True):
        case = vq.signed_zero_case(N, mirror)
        oc = vq.oracle_for(case)
        z, cb = case.distinct[0], case.codebook
        sc = {}
        for c in (vq.SZ_LO, vq.SZ_HI):
            a = oc.hc[c]
            for j in range(vq.J):
                a = np.float32(np.float64(z[j]) * np.float64(cb[c, j]) + np.float64(a))     # one rounding: an fma (the products are exact in f64)
            sc[c] = a
        zero = vq.SZ_HI if mirror else vq.SZ_LO
        assert sc[zero] == 0 and np.signbit(sc[zero]) and sc[vq.SZ_LO + vq.SZ_HI - zero] == 0 and not np.signbit(sc[vq.SZ_LO + vq.SZ_HI - zero])
        with np.errstate(all="ignore"):
            s = vq.scores64(cb, case.distinct[[0, 4]])
        assert np.sort(s[0])[-3] < -1000.0 and s[1].argmax() == N - 2
        ids = vq.oracle_ids(case)
        keep = case.expected != vq.ANY_IN_RANGE
        assert np.array_equal(ids[keep], case.expected[keep]), (mirror, ids)


@pytest.mark.parametrize("N", SIZES)
def test_stale_sequence_has_the_signs_it_claims(N):
    hot, cold, grow, few = vq.stale_sequence(N)
    assert tuple(c.index.shape[0] for c in (hot, cold, grow, few)) == vq.STALE_ROWS
    assert vq.STALE_ROWS[0] == vq.STALE_ROWS[1] and vq.STALE_ROWS[2] * 8 > (vq.STALE_ROWS[0] * 8) * 9 // 8 and vq.STALE_ROWS[3] < vq.STALE_ROWS[0]
    b_hot, E_hot = vq.best64(hot)
    assert np.all(b_hot > 10.0)
    for c in (cold, few):
        b, E = vq.best64(c)
        assert np.all(b < -1000.0 * E) and np.all(b < 0)
    assert np.all(vq.best64(grow)[0] > 1.0)
    # a key left over from the earlier call would change the answer of every cold row
    assert np.all(vq.expected_ids(hot) != vq.expected_ids(cold))
    assert np.all(vq.expected_ids(grow)[:vq.STALE_ROWS[3]] != vq.expected_ids(few))


def test_restated_split_formula_matches_the_source():
    src = open(os.path.join(ROOT, "realtime_codec_agent_amd", "csrc", "rca_codec.hip")).read()
    body = src[src.index("static int run_quantize("):]
    body = re.sub(r"\s+", "", body[:body.index("vq_finalize_kernel<<<")])
    for line in (
        f"constexprintFN={vq.MFMA_FN};",
        "constintftiles=(int)cdiv(rows,FN*32);",
        "constinttotal_tiles=N/32;",
        f"intsplits=(int)std::max(1L,std::min((long)total_tiles/{vq.MFMA_MIN_TILES},({vq.MFMA_WGS}+ftiles-1)/(long)ftiles));",
        "inttps=(total_tiles+splits-1)/splits;",
        f"tps=(tps+{vq.MFMA_WAVES - 1})/{vq.MFMA_WAVES}*{vq.MFMA_WAVES};",
        "splits=(total_tiles+tps-1)/tps;",
        f"constexprintFB={vq.CHAIN_FB};",
        "constintfblocks=(int)cdiv(rows,FB);",
        f"intsplits=(int)std::max(1L,std::min((long)N/{vq.CHAIN_MIN_CODES},({vq.CHAIN_WGS}+fblocks-1)/(long)fblocks));",
        "intcps=(N+splits-1)/splits;",
        f"cps=(cps+{vq.CHAIN_THREADS - 1})/{vq.CHAIN_THREADS}*{vq.CHAIN_THREADS};",
        "splits=(N+cps-1)/cps;",
    ):
        assert line in body, line
    kernel = re.sub(r"\s+", "", src[src.index("void vq_mfma_kernel("):src.index("struct RowDst")])
    for line in (
        f"for(inttile=tile_beg+wave;tile<tile_end;tile+={vq.MFMA_WAVES})",
        "constinttile_beg=blockIdx.y*tiles_per_split;",
        "constinthalf=lane>>5;",
        "constunsignedc=(unsigned)(c0+(r&3)+8*(r>>2)+4*half);",
        "constintc0=tile*32;",
    ):
        assert line in kernel, line
    # the three split geometries of the deployed codebook that the cases are sized for
    assert vq.mfma_split(64, vq.LARGE_N) == (16, 256)
    assert vq.mfma_split(4096, vq.LARGE_N) == (256, 16)
    assert vq.mfma_split(25600, vq.LARGE_N) == (1368, 3)
    for R in vq.RAGGED_ROWS + vq.STALE_ROWS:
        assert vq.mfma_split(R, vq.SMALL_N) == (16, 2) and vq.chain_split(R, vq.SMALL_N)[1] >= 1


SEAMS = {"lane", "half", "tile", "wave", "split"}


@pytest.mark.parametrize("N", SIZES)
def test_planted_pairs_reach_every_merge_seam(N):
    """same lane, across the lane halves, same wave across tiles, across waves, across code splits: each seam holds at least one
    planted exact pair, in the per-offset cases at their row count and in the mixed codebook at every row count it runs with"""
    def seams(case, rows):
        tps, _ = vq.mfma_split(rows, N)
        out = set()
        for _, g in case.planted:
            out |= {vq.mfma_seam(a, b, tps) for a in g for b in g if a < b}
        return out
    per_offset = set()
    for case in vq.family_a(N):
        per_offset |= seams(case, case.index.shape[0])
    assert per_offset == SEAMS, per_offset
    mixed = vq.mixed_case(N)
    for R in vq.RAGGED_ROWS + vq.STALE_ROWS + (vq.MANY_ROWS if N == vq.LARGE_N else ()):
        assert seams(mixed, R) == SEAMS, (R, seams(mixed, R))
    if N == vq.LARGE_N:
        # the offsets named for the two big geometries put their pairs exactly one split apart there
        for R, off in ((4096, 8192), (25600, 43776)):
            tps, splits = vq.mfma_split(R, N)
            assert off == tps * 32 and splits > 1
