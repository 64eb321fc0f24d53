"""The codebook search on the rows of tests/vq_cases.py (MI355X): rca_codec_quantize_dev with the chain kernel (variant 0) and the
matrix kernel (variant 1) against the expected ids, exactly -- planted exact ties (lowest index), near-ties, +-0 / NaN / inf rows,
ragged row counts, stale keys, many rows -- and, on the finite rows, against float64 scores: the chosen code's exact score lies
within 2 E of the best exact score (vq_cases.rounding_bound), which would also catch a kernel and an oracle wrong alike."""
import numpy as np
import pytest
import torch

import vq_cases as vq
from conftest import rich_signal

pytestmark = pytest.mark.gpu

VARIANTS = (0, 1)
SIZES = [vq.SMALL_N, vq.LARGE_N]
GUARD = 64                 # ids after the last row: a lane of a ragged block that writes shows up here
_U32 = np.uint32


def _new_handle(codebook, latent_dim=vq.J):
    from realtime_codec_agent_amd.codec import HipCodec
    hip = HipCodec(*vq.build_model(codebook, latent_dim), device=0)
    assert np.array_equal(hip.codebook().view(_U32), codebook.view(_U32))       # codebook_proj = I hands the planted rows through
    return hip


@pytest.fixture(scope="module")
def mixed_handles():
    """one handle per size over the mixed codebook (families d and e)"""
    made = {}

    def get(N):
        if N not in made:
            made[N] = _new_handle(vq.mixed_case(N).codebook)
        return made[N]
    yield get
    for h in made.values():
        h.close()


def _quantize(hip, rows):
    R = rows.shape[0]
    dev = torch.from_numpy(np.ascontiguousarray(rows)).cuda()
    out = torch.full((R + GUARD,), -7, dtype=torch.int64, device="cuda")
    hip.quantize_dev(dev.data_ptr(), R, out.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    out = out.cpu().numpy()
    assert np.all(out[R:] == -7), "ids written past the last row"
    return out[:R]


def _check_ids(case, got, tag):
    want = vq.expected_ids(case)
    assert got.shape == want.shape
    assert got.min() >= 0 and got.max() < case.N, (case.name, tag, int(got.min()), int(got.max()))
    pinned = want != vq.ANY_IN_RANGE
    bad = np.flatnonzero(pinned & (got != want))
    assert bad.size == 0, (f"{case.name} [{tag}]: {bad.size} of {got.size} ids differ; rows {bad[:8].tolist()} got {got[bad[:8]].tolist()} "
                           f"want {want[bad[:8]].tolist()} ({case.note})")


def _check_scores64(case, got, tag):
    """score64(chosen) >= max_c score64(c) - 2 E on every row (finite rows only: callers pass families a, b, d)"""
    best, E = vq.best64(case)
    z = case.rows.astype(np.float64)
    c = case.codebook[got].astype(np.float64)
    chosen = (z * c).sum(1) - 0.5 * (c * c).sum(1)
    gap = (best[case.index] - chosen) / E[case.index]
    assert np.all(gap <= 2.0), (case.name, tag, float(gap.max()))
    return float(gap.max())


def _run(case, hip, f64=True):
    worst = 0.0
    for v in VARIANTS:
        hip.set_variant(v)
        got = _quantize(hip, case.rows)
        _check_ids(case, got, f"variant {v}")
        if f64:
            worst = max(worst, _check_scores64(case, got, f"variant {v}"))
    return worst


@pytest.mark.parametrize("N", SIZES)
def test_exact_ties_give_the_lowest_index(N):
    """family a: per offset four planted pairs (code 0, code N-1, the middle of the codebook, an odd interior base), then groups of
    3..5 duplicates and codes 0 / N-1 as unique winners"""
    for case in vq.family_a(N):
        hip = _new_handle(case.codebook)
        _run(case, hip)
        hip.close()


@pytest.mark.parametrize("N", SIZES)
def test_near_ties_follow_the_oracle_bit_for_bit(N):
    """family b: codes one ulp apart, queried at three magnitudes; any other accumulation order than the oracle's flips some"""
    worst = 0.0
    for case in vq.family_b(N):
        hip = _new_handle(case.codebook)
        worst = max(worst, _run(case, hip))
        hip.close()
    print(f"N={N}: largest (best64 - score64(chosen)) / E = {worst:.3g}")


@pytest.mark.parametrize("mirror", [False, True], ids=["plain", "mirror"])
@pytest.mark.parametrize("N", SIZES)
def test_signed_zero_nan_and_inf_rows(N, mirror):
    """family c: scores -0.0 and +0.0 are one maximum and the lower index wins it; an all-NaN row gives code 0; rows with an
    infinity give some id inside the codebook.  (Before pack_key canonicalised the zero, the plain case answered 9, and before
    vq_finalize_kernel mapped the empty key, the NaN row answered 4294967295.)"""
    case = vq.signed_zero_case(N, mirror)
    hip = _new_handle(case.codebook)
    for v in VARIANTS:
        hip.set_variant(v)
        got = _quantize(hip, case.rows)
        print(f"{case.name} variant {v}: ids {got.tolist()}")
        _check_ids(case, got, f"variant {v}")
    hip.close()


@pytest.mark.parametrize("N", SIZES)
def test_ragged_row_counts(N, mixed_handles):
    """family d: row counts around the chain kernel's 4-frame and the matrix kernel's 64-frame blocks; nothing is written past
    the last row; the same rows through the latent_dim 256 model ([I16 | 0]: the D loop of the rows layout)"""
    hip = mixed_handles(N)
    for R in vq.RAGGED_ROWS:
        _run(vq.ragged_case(N, R), hip)
    if N == vq.SMALL_N:
        wide = _new_handle(vq.mixed_case(N).codebook, 256)
        for R in (5, 65):
            case = vq.ragged_case(N, R)
            for v in VARIANTS:
                wide.set_variant(v)
                _check_ids(case, _quantize(wide, vq.widen_rows(case.rows, 256)), f"latent 256, variant {v}")
        wide.close()


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("N", SIZES)
def test_keys_are_rearmed_between_calls(N, variant):
    """family d: large positive scores, then negative ones at the same row count, then more rows (the key buffer grows and is
    cleared), then fewer -- on one fresh handle; a key that survived a call would win the next call's atomicMax"""
    seq = vq.stale_sequence(N)
    hip = _new_handle(seq[0].codebook)
    hip.set_variant(variant)
    for case in seq:
        got = _quantize(hip, case.rows)
        _check_ids(case, got, f"variant {variant}")
        _check_scores64(case, got, f"variant {variant}")
    hip.close()


@pytest.mark.parametrize("R", vq.MANY_ROWS)
def test_many_rows_of_the_deployed_codebook(R, mixed_handles):
    """family e: 16 splits of 256 tiles (4096 rows) and 3 splits of 1368 tiles (25600 rows) in the matrix kernel"""
    assert vq.mfma_split(R, vq.LARGE_N) == {4096: (256, 16), 25600: (1368, 3)}[R]
    _run(vq.many_rows_case(R), mixed_handles(vq.LARGE_N), f64=False)


@pytest.mark.parametrize("latent_dim", [vq.J, 256])
def test_encoder_native_layout_reaches_the_same_search(latent_dim):
    """encode() quantises the encoder's [B][D][F] output (in_proj_kernel's strided branch, RowDst's channel stride); it must give
    quantize_rows of that same latent laid out as rows"""
    from oracle.codec import OracleCodec
    cb = vq.mixed_case(vq.SMALL_N).codebook
    cfg, w = vq.build_model(cb, latent_dim)
    hip, oc = _new_handle(cb, latent_dim), OracleCodec(cfg, w)
    assert np.array_equal(oc.codebook().view(_U32), cb.view(_U32))
    for T in (320 * 5, 320 * 65):
        x = np.stack([rich_signal(T, 31 + b) for b in range(2)])
        B, F = 2, T // 320
        for v in VARIANTS:
            hip.set_variant(v)
            ze = hip.encode_tap(x, cfg.n_stages + 1)                                   # [B][D][F]
            assert ze.shape == (B, latent_dim, F)
            z = hip.encode_tap(x, cfg.n_stages + 2)                                    # [B*F][16] after in_proj = [I16 | 0]
            rows = np.ascontiguousarray(ze.transpose(0, 2, 1).reshape(B * F, latent_dim))
            assert np.array_equal(z, rows[:, :vq.J])
            want = oc.quantize_rows(rows).reshape(B, F)
            got = hip.encode(x)
            assert np.array_equal(got, want), (latent_dim, T, v, int((got != want).sum()))
            assert np.array_equal(_quantize(hip, rows).reshape(B, F), want), (latent_dim, T, v)
        assert T == 320 * 5 or len(np.unique(want)) > 8
    hip.close()
