"""The three LM attention kernels run alone (rca_lm_attn_tap over K / V planted with rca_lm_kv_write) against the float64 reference
and the derived per-element bound of tests/attn_ref.py: lm_attn_mfma_kernel<G> with its in-launch merge over tagged granules,
lm_attn_mfma_combine_kernel<G> and lm_attn_flash_kernel<G, TEAMS>.  One-hot rows pin which key's weight meets which key's value;
score classes from flat to peaked, with common offsets of +-80 nats, challenge the max subtraction and the merges' guards; the
seams of the decode launch, the fused merge beyond 32 splits, the flash tiles, stale rows behind the context and the refusals follow.
Models are one layer of random weights (only the head geometry matters): nothing is evaluated to reach a context.

Every comparison prints its worst error / bound ratio; test_report_of_worst_ratios sums them up per route and per score class."""
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import attn_ref as ar
import lm_shape_cases as sc

pytestmark = pytest.mark.gpu

WORST = {}          # (what, key) -> worst error / bound ratio seen
TEAMS_SEEN = set()
SPLITS_SEEN = set()


def _n_cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


@functools.lru_cache(maxsize=None)
def _llm(geom, n_ctx):
    from realtime_codec_agent_amd.llm import LlamaForAlternatingCodeChannels, LMConfig
    nh, nkv = ar.GEOMS[geom]
    cfg = LMConfig(vocab_size=64, hidden=128, n_layers=1, n_heads=nh, n_kv_heads=nkv, head_dim=64, ffn=64)
    llm = LlamaForAlternatingCodeChannels(model_path=f"random:attn_{geom}", config=cfg, n_ctx=n_ctx, random_seed=3, init_std=0.05, device=0,
                                          weight_format="bf16")
    llm._planted = None
    return llm


def _plant(llm, tag, K, V):
    """the cache rows 0 .. len(K) - 1 (once per tag: the cases of a test share their K / V)"""
    if llm._planted != tag:
        llm.kv_write(0, 0, K, V)
        llm._planted = tag


def _tap(llm, route, q, pos0, nsp=0, out_rows=None):
    llm.n_tokens = pos0
    out = llm.attn_tap(0, route, q.reshape(q.shape[0], -1), nsp, out_rows)
    assert llm.n_tokens == pos0
    return out


def _check(tag, got, want, bound, keys=()):
    """finite first (a NaN row is the fused merge's own timeout signal), then every element within its bound"""
    assert np.isfinite(got).all(), f"{tag}: {np.isnan(got).any(1).sum()} rows hold NaN (the in-launch merge timed out?) / Inf"
    ratio = float((np.abs(got - want) / bound).max())
    for k in keys:
        WORST[k] = max(WORST.get(k, 0.0), ratio)
    assert ratio <= 1.0, f"{tag}: error / bound = {ratio:.3f}"
    return ratio


def _route_key(route, fuse=True):
    return ("route", {0: "decode fused" if fuse else "decode separate combine", 1: "flash f32", 2: "flash bf16"}[route])


def _routes(llm):
    return (0, 1, 2) if llm.prefill_route() == "gemm128" else (0, 1)


def _teams(geom, M):
    nh, nkv = ar.GEOMS[geom]
    t = sc.flash_teams(SimpleNamespace(G=nh // nkv, n_kv_heads=nkv), M, _n_cus())
    TEAMS_SEEN.add((nh // nkv, t))
    return t


# ------------------------------------------------------------------ a. one-hot rows
@functools.lru_cache(maxsize=None)
def _onehot(nkv):
    return ar.onehot_kv(ar.ONEHOT_SEED, ar.ONEHOT_T, nkv)


@pytest.mark.parametrize("geom", ar.SMALL)
def test_onehot_rows_pin_key_order_and_row_mapping(geom):
    """q = 16 * k_target over +-1 keys: the target leads by at least 40 nats (asserted in test_attn_cpu.py), so a row's output is
    its target's V row, within the bound.  Decode: every key offset of a split (8 waves x 32 register slots), the first and last key
    of the first three splits, the newest key, and 2-token calls whose token 0 targets its own position.  Flash, f32 and bf16 output:
    a 1024-token pass at pos0 = 1100 whose rows walk the visible keys (every slot of each wave's blocks), and passes of 33 and 7."""
    nh, nkv = ar.GEOMS[geom]
    llm = _llm(geom, 3072)
    K, V = _onehot(nkv)
    _plant(llm, "onehot", K, V)
    heads = np.arange(nh) // (nh // nkv)
    worst = {}
    calls = []
    for pos0, tg in ar.decode_onehot_calls(nh):
        q = ar.onehot_q(K, tg, nh)
        want, bound = ar.attention(q, K, V, pos0, with_bound_for=0)
        assert np.abs(want - V[tg, heads[None, :]].astype(np.float64).reshape(want.shape)).max() < 1e-9
        calls.append((pos0, tg, q, want, bound))
    for fuse in (True, False):
        llm.set_attn_fuse(fuse)
        for pos0, tg, q, want, bound in calls:
            r = _check(f"{geom} decode one-hot at {pos0}, targets {tg.tolist()}, fuse {fuse}", _tap(llm, 0, q, pos0), want, bound,
                       (_route_key(0, fuse), ("class", "one-hot")))
            worst[_route_key(0, fuse)[1]] = max(worst.get(_route_key(0, fuse)[1], 0.0), r)
    llm.set_attn_fuse(True)
    for route in _routes(llm)[1:]:
        for M in ar.FLASH_ONEHOT_M:
            tg = ar.flash_onehot_targets(M, nh, ar.FLASH_POS0)
            q = ar.onehot_q(K, tg, nh)
            want, bound = ar.attention(q, K, V, ar.FLASH_POS0, with_bound_for=route)
            assert np.abs(want - V[tg, heads[None, :]].astype(np.float64).reshape(want.shape)).max() < 1e-9
            r = _check(f"{geom} flash one-hot M = {M}, route {route}, TEAMS {_teams(geom, M)}", _tap(llm, route, q, ar.FLASH_POS0), want, bound,
                       (_route_key(route), ("class", "one-hot")))
            worst[_route_key(route)[1]] = max(worst.get(_route_key(route)[1], 0.0), r)
    print(f"ATTN {geom} one-hot, worst error / bound: " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))


# ------------------------------------------------------------------ b. accuracy over the score classes
@pytest.mark.parametrize("geom", list(ar.GEOMS))
def test_accuracy_over_score_classes(geom):
    """flat (sigma 0.1), moderate (3) and peaked (15) scores, each plain and with +80 / -80 nats on every key, V of mixed sign and
    magnitude, 642 .. 680 keys: every route of the geometry, decode with the merge inside and outside the launch.  (The moderate
    class found the flash kernel's inconsistent fp16 split of q: w32 token 17 / head 17 was 1.62 bounds off on the f32 route and
    1.57 on the bf16 route, g2 token 19 / head 1 0.42, with every other row below 0.2: DESIGN.md, "Attention alone".)"""
    llm = _llm(geom, 3072)
    lines = []
    for cls in ar.SCORE_CLASSES:
        for off in ar.OFFSETS:
            worst = 0.0
            for route in _routes(llm):
                K, V, q, pos0 = ar.class_case(geom, cls, off, route)
                _plant(llm, ("class", cls, off), K, V)
                want, bound = ar.attention(q, K, V, pos0, with_bound_for=route)
                for fuse in (True, False) if route == 0 else (True,):
                    llm.set_attn_fuse(fuse)
                    worst = max(worst, _check(f"{geom} {cls}{off:+.0f} route {route} fuse {fuse}", _tap(llm, route, q, pos0), want, bound,
                                              (_route_key(route, fuse), ("class", f"{cls}{off:+.0f}"))))
                llm.set_attn_fuse(True)
            lines.append(f"{cls}{off:+.0f} {worst:.3f}")
    print(f"ATTN {geom} score classes, worst error / bound over routes {_routes(llm)}: " + ", ".join(lines))


# ------------------------------------------------------------------ c. seams of the decode launch
SEAM_POS0 = (0, 1, 30, 31, 32, 254, 255, 256, 257, 511, 512)


@pytest.mark.parametrize("geom", ar.SMALL)
def test_decode_seams_and_bucketed_launches(geom):
    """1- and 2-token steps starting at the seams of the 32-key wave blocks and the 256-key splits, launched with the needed splits,
    with the 4- and 8-split buckets and with every split of the handle (splits past the context publish -inf granules and still
    merge rows); on an n_ctx = 700 handle up to pos0 + M = n_ctx, whose limit falls inside the last split.  Merge inside the launch
    and as a launch of its own: both within the bound, and bit-identical to each other."""
    nh, nkv = ar.GEOMS[geom]
    K, V = ar.class_kv(77, ar.CLASS_T, nkv)
    q2 = ar.class_q(78, 2, nh, ar.SCORE_CLASSES["moderate"])
    worst, n = 0.0, 0
    for n_ctx, extra in ((700, (698, 699)), (3072, ())):
        llm = _llm(geom, n_ctx)
        _plant(llm, "seams", K, V)
        all_splits = -(-n_ctx // ar.ATT_KEYS)
        for pos0 in SEAM_POS0 + extra:
            for M in (1, 2):
                if pos0 + M > 700:
                    continue
                q = q2[:M]
                want, bound = ar.attention(q, K, V, pos0, with_bound_for=0)
                need = ar.splits_needed(pos0, M)
                for nsp in sorted({need, 4, 8, all_splits}):
                    if nsp < need or nsp > all_splits:
                        continue
                    outs = []
                    for fuse in (True, False):
                        llm.set_attn_fuse(fuse)
                        outs.append(_tap(llm, 0, q, pos0, nsp, out_rows=M + 1))
                        tag = f"{geom} n_ctx {n_ctx} pos0 {pos0} M {M} nsp_launch {nsp} fuse {fuse}"
                        assert np.isnan(outs[-1][M]).all(), tag + ": the row past the pass was written"
                        worst = max(worst, _check(tag, outs[-1][:M], want, bound, (_route_key(0, fuse), ("class", "moderate+0"))))
                    assert np.array_equal(outs[0], outs[1], equal_nan=True), f"{geom} pos0 {pos0} M {M} nsp {nsp}: fused and separate merge differ"
                    n += 1
        llm.set_attn_fuse(True)
    print(f"ATTN {geom} decode seams: {n} launches x 2 merges, worst error / bound {worst:.3f}")


# ------------------------------------------------------------------ d. the fused merge beyond 32 splits
@pytest.mark.parametrize("geom", ("g2", "g4"))
def test_fused_merge_beyond_32_splits(geom):
    """2 and 1 kv heads at n_ctx = 32768: 2-token steps over contexts that need 32, 33 (the second block of 32 pre-fetched splits), 64,
    65 (the second 64-split chunk) and 128 splits, launched as needed and with the 64- and 128-split buckets; moderate scores, one
    dominant key in split 0, one in the last split.  Merged inside the launch == merged by the combine launch, bit for bit, and
    within the bound.  One fused case 200 times back to back: the tag counter across launches."""
    llm = _llm(geom, ar.LONG_CTX)
    worst, n = 0.0, 0
    for nsplits in ar.LONG_SPLITS:
        for pattern in ar.LONG_PATTERNS:
            K, V, q, pos0 = ar.long_case(geom, nsplits, pattern)
            _plant(llm, ("long", nsplits, pattern), K, V)
            want, bound = ar.attention(q, K, V, pos0, with_bound_for=0)
            for nsp in sorted({nsplits, 64, 128}):
                if nsp < nsplits:
                    continue
                outs = []
                for fuse in (True, False):
                    llm.set_attn_fuse(fuse)
                    outs.append(_tap(llm, 0, q, pos0, nsp))
                    worst = max(worst, _check(f"{geom} {nsplits} splits, launched {nsp}, {pattern}, fuse {fuse}", outs[-1], want, bound,
                                              (_route_key(0, fuse), ("class", pattern if pattern != "moderate" else "moderate+0"))))
                assert np.array_equal(outs[0], outs[1]), f"{geom} {nsplits} splits, launched {nsp}, {pattern}: fused and separate merge differ"
                SPLITS_SEEN.add((ar.GEOMS[geom][1], nsp))
                n += 1
    llm.set_attn_fuse(True)
    first = _tap(llm, 0, q, pos0, 128)
    assert np.isfinite(first).all(), "a NaN row: the in-launch merge timed out"
    for i in range(200):
        again = _tap(llm, 0, q, pos0, 128)
        assert np.isfinite(again).all(), f"repeat {i}: a NaN row, the in-launch merge timed out"
        assert np.array_equal(again, first), f"repeat {i} differs"
    print(f"ATTN {geom} long contexts: {n} launches x 2 merges, worst error / bound {worst:.3f}; 200 repeats of the 128-split launch identical")


def test_fused_merge_selection_rule_gives_right_answers_on_both_sides():
    """3 kv heads: 64 launched splits are merged inside the launch (192 workgroups), 128 are not (384), and neither are the 129 of
    n_ctx = 33024; with the switch off every one of them takes the combine launch.  Same bits either way, within the bound."""
    geom = "kv3"
    for n_ctx, cases in ((ar.LONG_CTX, ((64, 64), (65, 128), (128, 128))), (33024, ((129, 129),))):
        llm = _llm(geom, n_ctx)
        for nsplits, nsp in cases:
            K, V, q, pos0 = ar.long_case(geom, nsplits, "moderate")
            _plant(llm, ("long", nsplits), K, V)
            want, bound = ar.attention(q, K, V, pos0, with_bound_for=0)
            outs = []
            for fuse in (True, False):
                llm.set_attn_fuse(fuse)
                outs.append(_tap(llm, 0, q, pos0, nsp))
                fused = fuse and 3 * nsp <= 256 and nsp <= 128
                r = _check(f"kv3 {nsplits} splits, launched {nsp}, fuse switch {fuse}", outs[-1], want, bound,
                           (_route_key(0, fused), ("class", "moderate+0")))
                print(f"ATTN kv3 n_ctx {n_ctx}: {nsplits} splits needed, {nsp} launched ({3 * nsp} workgroups), merge {'inside' if fused else 'outside'} "
                      f"the launch: error / bound {r:.3f}")
            assert np.array_equal(outs[0], outs[1])
            SPLITS_SEEN.add((3, nsp))
        llm.set_attn_fuse(True)


# ------------------------------------------------------------------ e. flash tiles
FLASH_TILES = (   # (geometry, M, pos0): every M of {1, 7, 8, 9, 31, 32, 33, 96, 1000, 1024} (and 512: TEAMS 2) and every pos0 of {0, 5, 31, 250, 2040}
    ("g1", 1, 0), ("g1", 9, 250), ("g1", 32, 2040),
    ("g2", 7, 5), ("g2", 33, 31), ("g2", 1024, 2040),
    ("g4", 8, 31), ("g4", 96, 5), ("g4", 1000, 250),
    ("kv3", 31, 0), ("kv3", 32, 5),
    ("w32", 1024, 5), ("w32", 512, 250), ("w16", 1000, 31), ("w16", 33, 2040),
)
FLASH_T = 3072


@functools.lru_cache(maxsize=None)
def _flash_kv(nkv):
    return ar.class_kv(900 + nkv, FLASH_T, nkv)


@pytest.mark.parametrize("geom,M,pos0", FLASH_TILES, ids=[f"{g}-M{m}-pos{p}" for g, m, p in FLASH_TILES])
def test_flash_tiles(geom, M, pos0):
    """rows < M within the bound, rows M .. out_rows - 1 still the NaN they were filled with, on the f32 route and (where the
    geometry has the 128-token route) the bf16 hi / lo route; the lm_attn_flash_kernel<G, TEAMS> instance is computed from the device's
    CU count with the library's rule and printed"""
    nh, nkv = ar.GEOMS[geom]
    llm = _llm(geom, 3072)
    K, V = _flash_kv(nkv)
    _plant(llm, "flash", K, V)
    q = ar.class_q(901 + M, M, nh, ar.SCORE_CLASSES["moderate"])
    out_rows = min(M + 3, 1024)
    for route in _routes(llm)[1:]:
        want, bound = ar.attention(q, K, V, pos0, with_bound_for=route)
        got = _tap(llm, route, q, pos0, out_rows=out_rows)
        assert np.isnan(got[M:]).all(), f"{geom} M {M} pos0 {pos0} route {route}: rows past the pass were written"
        r = _check(f"{geom} flash M {M} pos0 {pos0} route {route}", got[:M], want, bound, (_route_key(route), ("class", "moderate+0")))
        print(f"ATTN flash {geom} M = {M} at pos0 = {pos0}, route {route}: lm_attn_flash_kernel<{nh // nkv}, {_teams(geom, M)}> on {_n_cus()} CUs, "
              f"error / bound {r:.3f}")


def test_flash_tiles_reach_every_teams_instance():
    seen = {_teams(g, M) for g, M, _ in FLASH_TILES}
    print(f"ATTN flash TEAMS instances on {_n_cus()} CUs: " + ", ".join(f"{g} M {M}: {_teams(g, M)}" for g, M, _ in FLASH_TILES))
    assert seen == {1, 2, 4}, seen


@pytest.mark.parametrize("geom", ("g2", "w32"))
def test_flash_rows_do_not_depend_on_the_cut(geom):
    """the property the shadow cache rests on: the rows of one 1024-token pass are, bit for bit, the rows of passes of 100 + 924 and
    of 1 + 1023 tokens at the matching positions (other TEAMS instances, other tiles), on both output routes"""
    nh, nkv = ar.GEOMS[geom]
    llm = _llm(geom, 3072)
    K, V = _flash_kv(nkv)
    _plant(llm, "flash", K, V)
    q = ar.class_q(950, 1024, nh, ar.SCORE_CLASSES["moderate"])
    pos0 = 700
    for route in _routes(llm)[1:]:
        whole = _tap(llm, route, q, pos0)
        assert np.isfinite(whole).all()
        for cut in (100, 1):
            parts = np.concatenate((_tap(llm, route, q[:cut], pos0), _tap(llm, route, q[cut:], pos0 + cut)))
            assert np.array_equal(parts, whole), f"{geom} route {route}: {cut} + {1024 - cut} differs from one pass of 1024"
        print(f"ATTN flash {geom} route {route}: 1024 == 100 + 924 == 1 + 1023 (TEAMS {_teams(geom, 1024)} / {_teams(geom, 100)} + {_teams(geom, 924)} / "
              f"{_teams(geom, 1)} + {_teams(geom, 1023)})")


@pytest.mark.parametrize("geom", ("g1", "g4", "kv3"))
def test_flash_last_tile_clamped_by_n_ctx(geom):
    """pos0 + M = n_ctx = 700: the last tile's key range is cut by the context limit"""
    nh, nkv = ar.GEOMS[geom]
    llm = _llm(geom, 700)
    K, V = ar.class_kv(77, ar.CLASS_T, nkv)
    _plant(llm, "seams", K, V)
    for M in (40, 7):
        q = ar.class_q(960 + M, M, nh, ar.SCORE_CLASSES["moderate"])
        for route in _routes(llm)[1:]:
            want, bound = ar.attention(q, K, V, 700 - M, with_bound_for=route)
            r = _check(f"{geom} M {M} ending at n_ctx, route {route}", _tap(llm, route, q, 700 - M), want, bound, (_route_key(route), ("class", "moderate+0")))
            print(f"ATTN flash {geom} M = {M} ending at n_ctx = 700, route {route}: error / bound {r:.3f}")


# ------------------------------------------------------------------ f. stale rows behind the context
def _fills(shape, seed):
    rng = np.random.default_rng(seed)
    junk = ar.f16(np.clip(rng.standard_normal(shape) * 10.0 ** rng.uniform(-3, 4, shape), -65504, 65504))
    junk[rng.random(shape) < 0.2] = 65504
    junk[rng.random(shape) < 0.2] = -65504
    bits = rng.choice(np.array([0x7C00, 0xFC00, 0x7E00, 0xFFFF, 0x7C01], np.uint16), shape)      # +-Inf, quiet / signalling NaN patterns
    return {"zeros": np.zeros(shape, np.float16), "finite junk": junk, "Inf / NaN": bits.view(np.float16)}


@pytest.mark.parametrize("geom", ("g2", "kv3"))
def test_rows_behind_the_context_may_hold_anything(geom):
    """the cache rows [n_tokens + M, n_ctx) filled with zeros, with +-65504 and random finite junk, with Inf / NaN bit patterns: the
    same bits come out, for a decode launch (needed splits, and all splits: a whole split of junk) and a prefill launch per route"""
    nh, nkv = ar.GEOMS[geom]
    llm = _llm(geom, 700)
    K, V = ar.class_kv(77, ar.CLASS_T, nkv)
    llm.kv_write(0, 0, K, V)
    llm._planted = None
    for route, M, pos0, nsp in ((0, 2, 300, 0), (0, 2, 300, 3), (0, 1, 511, 3), (1, 40, 600, 0), (2, 40, 600, 0), (1, 7, 250, 0)):
        if route not in _routes(llm):
            continue
        q = ar.class_q(970 + M, M, nh, ar.SCORE_CLASSES["moderate"])
        want, bound = ar.attention(q, K, V, pos0, with_bound_for=route)
        outs = {}
        for name, fill in _fills((700 - pos0 - M, nkv, 64), 5).items():
            llm.kv_write(0, pos0 + M, fill, fill)
            for fuse in (True, False) if route == 0 else (True,):
                llm.set_attn_fuse(fuse)
                outs[(name, fuse)] = _tap(llm, route, q, pos0, nsp)
        llm.set_attn_fuse(True)
        llm.kv_write(0, 0, K, V)
        _check(f"{geom} route {route} M {M} pos0 {pos0}, zeros behind the context", outs[("zeros", True)], want, bound)
        for k, o in outs.items():
            assert np.array_equal(o, outs[("zeros", True)], equal_nan=True), f"{geom} route {route} M {M} pos0 {pos0} nsp {nsp}: {k} behind the context changes the output"
    print(f"ATTN {geom}: outputs do not depend on the rows behind the context (zeros / finite junk / Inf and NaN)")


@pytest.mark.parametrize("geom", ("g2", "kv3"))
def test_token_0_does_not_see_token_1s_cache_row(geom):
    """a 2-token decode launch: token 0's rows are the same bits whatever finite K / V row token 1's position holds, and whatever K
    row, finite or not.  (A non-finite V row does reach the other rows of its MFMA tile, as 0 * Inf: DESIGN.md says when the cache
    can hold one.)"""
    nh, nkv = ar.GEOMS[geom]
    llm = _llm(geom, 700)
    K, V = ar.class_kv(77, ar.CLASS_T, nkv)
    llm.kv_write(0, 0, K, V)
    llm._planted = None
    q = ar.class_q(980, 2, nh, ar.SCORE_CLASSES["moderate"])
    for pos0 in (255, 300, 511):
        want, bound = ar.attention(q, K, V, pos0, with_bound_for=0)
        base = _tap(llm, 0, q, pos0)
        _check(f"{geom} pos0 {pos0}", base, want, bound)
        fills = _fills((1, nkv, 64), 6)
        for kname, vname in (("finite junk", "finite junk"), ("Inf / NaN", "finite junk"), ("Inf / NaN", "zeros")):
            llm.kv_write(0, pos0 + 1, fills[kname], fills[vname])
            for fuse in (True, False):
                llm.set_attn_fuse(fuse)
                got = _tap(llm, 0, q, pos0)
                assert np.array_equal(got[0], base[0]), f"{geom} pos0 {pos0}: token 0 changes with token 1's row (K {kname}, V {vname}, fuse {fuse})"
        llm.set_attn_fuse(True)
        llm.kv_write(0, pos0 + 1, K[pos0 + 1:pos0 + 2], V[pos0 + 1:pos0 + 2])


# ------------------------------------------------------------------ g. refusals
def test_refusals_touch_nothing():
    from realtime_codec_agent_amd._native import RcaError
    llm, wide = _llm("kv3", 700), _llm("g2", 700)
    assert llm.prefill_route() == "tile32" and wide.prefill_route() == "gemm128"
    ids = np.random.default_rng(1).integers(0, 64, 12).tolist()
    llm.reset()
    llm.eval(ids[:10])
    llm.eval(ids[10:12])
    logits = llm._scores[-1].copy()
    k0, v0 = llm.kv_read(0, 0, 700)
    llm._planted = None
    q = np.zeros((2, 3 * 64), np.float32)
    big = np.zeros((1025, 3 * 64), np.float32)
    tap = lambda **kw: llm.attn_tap(**{**dict(layer=0, route=0, q=q, nsp_launch=0, out_rows=None), **kw})
    for what, call in (
        (r"attn_tap: layer 1 outside", lambda: tap(layer=1)),
        (r"attn_tap: layer -1 outside", lambda: tap(layer=-1)),
        (r"attn_tap: route 3 outside", lambda: tap(route=3)),
        (r"attn_tap: route -1 outside", lambda: tap(route=-1)),
        (r"attn_tap: M = 3, route 0 takes 1 \.\. 2", lambda: tap(q=big[:3])),
        (r"attn_tap: M = 1025, route 1 takes 1 \.\. 1024", lambda: tap(route=1, q=big)),
        (r"attn_tap: route 2 is the attention of the gemm128 prefill route", lambda: tap(route=2)),
        (r"attn_tap: out_rows 1 outside", lambda: tap(out_rows=1)),
        (r"attn_tap: out_rows 1025 outside", lambda: tap(out_rows=1025)),
        (r"attn_tap: nsp_launch 4 outside \[1 needed, 3 splits\]", lambda: tap(nsp_launch=4)),
        (r"attn_tap: nsp_launch -1 outside", lambda: tap(nsp_launch=-1)),
        (r"kv_write: layer 1 outside", lambda: llm.kv_write(1, 0, k0[:2], v0[:2])),
        (r"kv_write: positions \[699, 699 \+ 2\) outside the context of 700", lambda: llm.kv_write(0, 699, k0[:2], v0[:2])),
        (r"kv_write: positions \[-1,", lambda: llm.kv_write(0, -1, k0[:2], v0[:2])),
    ):
        with pytest.raises(RcaError, match=what):
            call()
        assert llm.n_tokens == 12, what
    llm.n_tokens = 300
    with pytest.raises(RcaError, match=r"attn_tap: nsp_launch 1 outside \[2 needed, 3 splits\]"):
        tap(nsp_launch=1)
    llm.n_tokens = 699
    with pytest.raises(RcaError, match=r"rc=-3\): attn_tap: positions 699 \.\. 700 are outside the context of 700"):
        tap()
    assert llm.n_tokens == 699
    k1, v1 = llm.kv_read(0, 0, 700)
    assert np.array_equal(k0.view(np.uint16), k1.view(np.uint16)) and np.array_equal(v0.view(np.uint16), v1.view(np.uint16))
    llm.n_tokens = 10
    llm.eval(ids[10:12])
    assert np.array_equal(llm._scores[-1], logits), "a refused call changed the next step's logits"
    # ... and accepted calls leave the next step alone too (the tap overwrites activation buffers only)
    llm.n_tokens = 10
    llm.attn_tap(0, 1, big[:40], out_rows=43)
    llm.kv_write(0, 12, k0[12:14], None)
    llm.eval(ids[10:12])
    assert llm.n_tokens == 12 and np.array_equal(llm._scores[-1], logits)
    wide.n_tokens = 10
    assert np.isfinite(wide.attn_tap(0, 2, np.zeros((40, 4 * 64), np.float32))).all()


def test_report_of_worst_ratios():
    """what the tests above measured (run with them): one worst error / bound ratio per route and per score class"""
    for kind in ("route", "class"):
        print(f"ATTN worst error / bound per {kind}: " + ", ".join(f"{k[1]} {v:.3f}" for k, v in sorted(WORST.items()) if k[0] == kind))
    print(f"ATTN flash instances <G, TEAMS> reached: {sorted(TEAMS_SEEN)}; decode launches (kv heads, splits) checked fused == separate: {sorted(SPLITS_SEEN)}")
    assert all(v <= 1.0 for v in WORST.values())
