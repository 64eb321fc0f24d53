"""The q8_0 KV cache (rca_lm_set_kv_format) on the GPU, against tests/kv_q8_ref.py:
  1. the quantiser alone, bit for bit (rca_lm_kv_write -> rca_lm_kv_read_q8 / rca_lm_kv_read);
  2. the five writers + lm_kv_quant_kernel: cache row == Q8(fp16 row of the default path), bit for bit, on every route, through group
     and batch steps and across the end of the staging ring;
  3. the attention kernels alone over a planted q8_0 cache, inside tests/attn_ref.py's own bound over the de-quantised rows;
  4. logits end to end against Q8KVRef;
  5. the lifecycle: refusals, twins, the shadow cycle, switching back;
  6. RealtimeAgentBatch over q8_0 handles: the fused tick equals the unfused one.
Every test fails on a library without rca_lm_set_kv_format (the parent commit: the constructor argument does not exist)."""
import functools

import numpy as np
import pytest

import attn_ref as ar
import kv_q8_ref as kr
import kv_q8_spread as ks
import lm_shape_cases as sc

pytestmark = pytest.mark.gpu

GREEDY = dict(top_k=1, top_p=1.0, min_p=0.0, temp=0.0, seed=1)
N_CTX = 1280          # above the ring's 1024 positions: passes can cross its end


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint16)


def _L():
    from realtime_codec_agent_amd.llm import LlamaForAlternatingCodeChannels
    return LlamaForAlternatingCodeChannels


def _err():
    from realtime_codec_agent_amd import _native
    return _native.RcaError


# ------------------------------------------------------------------ handles
@functools.lru_cache(maxsize=None)
def _attn_llm(geom):
    from realtime_codec_agent_amd.llm import LMConfig
    nh, nkv = ar.GEOMS[geom]
    cfg = LMConfig(vocab_size=64, hidden=128, n_layers=2, n_heads=nh, n_kv_heads=nkv, head_dim=64, ffn=64)
    llm = _L()(model_path=f"random:kvq8_{geom}", config=cfg, n_ctx=ar.CLASS_T, random_seed=3, init_std=0.05, device=0, weight_format="bf16",
               kv_format="q8_0")
    assert llm.kv_format == "q8_0"
    return llm


@functools.lru_cache(maxsize=None)
def _family(route):
    """(q8_0 handles, f16 handles): a parent and two twins per format over ONE set of weights, n_ctx above the ring"""
    name, fmt = ks.E2E_CASES[route]
    c = sc.BY_NAME[name]
    parent = _L()(model_path=f"random:{name}", config=c.config(), n_ctx=N_CTX, random_seed=c.seed, init_std=sc.INIT_STD, device=0, weight_format=fmt,
                  kv_format="q8_0")
    assert parent.prefill_route() == route and parent.kv_format == "q8_0"
    q8 = [parent] + [_L()(n_ctx=N_CTX, share_weights_with=parent, device=0) for _ in range(2)]
    assert all(m.kv_format == "q8_0" for m in q8), "a twin inherits its parent's KV format"
    f16 = [_L()(n_ctx=N_CTX, share_weights_with=parent, device=0, kv_format="f16") for _ in range(3)]
    assert all(m.kv_format == "f16" for m in f16)
    for m in q8 + f16:
        m.init_sampler_for_generate(**GREEDY)
    return q8, f16


def _assert_rows_are_q8_of(q8, f16, layer, pos0, n, tag):
    """the contract: the q8_0 handle's blocks == quant_rows(the f16 handle's rows); its de-quantised read == dequant of them"""
    kq, kd, vq, vd = q8.kv_read_q8(layer, pos0, n)
    kf, vf = f16.kv_read(layer, pos0, n)
    for name, q, d, f in (("K", kq, kd, kf), ("V", vq, vd, vf)):
        wq, wd = kr.quant_rows(f)
        assert np.array_equal(q, wq), f"{tag}: {name} int8 values differ at {np.argwhere(q != wq)[:4].tolist()}"
        assert np.array_equal(_bits(d), _bits(wd)), f"{tag}: {name} scales differ"
    kr_, vr_ = q8.kv_read(layer, pos0, n)
    assert np.array_equal(_bits(kr_), _bits(kr.dequant(kq, kd))) and np.array_equal(_bits(vr_), _bits(kr.dequant(vq, vd))), f"{tag}: kv_read is not the de-quantised blocks"


# ------------------------------------------------------------------ 1. the quantiser, exact
@pytest.mark.parametrize("geom", ["g2", "kv3"])
def test_quantiser_is_exact(geom):
    """rows of every class of the rule (kv_q8_ref.edge_rows: zero block, negative amax, 65504, underflowing and subnormal scales, exact
    ties) plus random rows over four decades, written at positions 250 .. 262 (both sides of the 256-key split) and 26 .. 38 (both sides
    of a 32-key wave block), K and V together and each alone; the rows next to the written range keep their contents"""
    llm = _attn_llm(geom)
    nkv = ar.GEOMS[geom][1]
    rng = np.random.default_rng(5)
    assert llm.kv_ring_positions() == 1024 and llm.kv_bytes_per_position() == 2 * nkv * 2 * 68
    back = (rng.standard_normal((60, nkv, 64)) * 3).astype(np.float16)
    for layer, p0 in ((0, 250), (1, 26)):
        llm.kv_write(layer, p0 - 20, back, back[::-1].copy())
        before = llm.kv_read_q8(layer, p0 - 20, 60)
        n = 13
        K = kr.edge_rows(rng, n, nkv)
        V = kr.edge_rows(rng, n, nkv, scale=30.0)[::-1].copy()
        K[8:] = (K[8:].astype(np.float32) * 10.0 ** rng.uniform(-2, 2, (n - 8, nkv, 1))).astype(np.float16)
        llm.kv_write(layer, p0, K, V)
        kq, kd, vq, vd = llm.kv_read_q8(layer, p0, n)
        for name, rows, q, d in (("K", K, kq, kd), ("V", V, vq, vd)):
            wq, wd = kr.quant_rows(rows)
            assert np.array_equal(q, wq), f"{name} int8 values, layer {layer}: {np.argwhere(q != wq)[:4].tolist()}"
            assert np.array_equal(_bits(d), _bits(wd)), f"{name} scales, layer {layer}"
        rk, rv = llm.kv_read(layer, p0, n)
        assert np.array_equal(_bits(rk), _bits(kr.fake_quant(K))) and np.array_equal(_bits(rv), _bits(kr.fake_quant(V)))
        after = llm.kv_read_q8(layer, p0 - 20, 60)
        keep = np.r_[0:20, 20 + n:60]
        for b, a in zip(before, after):
            assert np.array_equal(_bits(b[keep]) if b.dtype == np.float16 else b[keep], _bits(a[keep]) if a.dtype == np.float16 else a[keep]), "a row next to the written range changed"
        # one tensor alone leaves the other as it is
        llm.kv_write(layer, p0, k=V)
        k2, _, v2, _ = llm.kv_read_q8(layer, p0, n)
        assert np.array_equal(k2, vq) and np.array_equal(v2, vq)
        llm.kv_write(layer, p0, v=K)
        k3, _, v3, _ = llm.kv_read_q8(layer, p0, n)
        assert np.array_equal(k3, vq) and np.array_equal(v3, kq)


# ------------------------------------------------------------------ 2. the writers, exact
@pytest.mark.parametrize("route", list(ks.E2E_CASES))
def test_writers_store_q8_of_the_default_rows(route):
    """Layer 0's K / V rows depend on the token and its position only (embedding, norm, QKV, RoPE), so the two handles can be compared
    whatever their caches hold: decode passes (an eval of 7: M = 2, 2, 2, 1), one eval of 33 on the route and, on the 128-token tiles, a
    pass of 128; step with M = 1 and M = 2; an eval of 64 from position 1000 and a 2-token step from 1023, whose ring rows wrap; layer 1
    through rca_lm_gemv_tap (one input, both handles)."""
    q8s, f16s = _family(route)
    a, b = q8s[0], f16s[0]
    c = sc.BY_NAME[ks.E2E_CASES[route][0]]
    ids = c.ids().tolist()
    assert a.kv_ring_positions() == 1024 < N_CTX
    for m in (a, b):
        m.reset()
    pos = 0
    plan = [("eval", 7), ("eval", 33)] + ([("eval", 128)] if route == "gemm128" else []) + [("step", 1), ("step", 2)]
    for kind, n in plan:
        for m in (a, b):
            (m.eval if kind == "eval" else m.step)(ids[pos:pos + n])
        _assert_rows_are_q8_of(a, b, 0, pos, n, f"{route} {kind} of {n} at {pos}")
        pos += n
    for start, kind, n in ((1000, "eval", 64), (1023, "step", 2)):
        for m in (a, b):
            m.n_tokens = start
            (m.eval if kind == "eval" else m.step)(ids[:n])
        _assert_rows_are_q8_of(a, b, 0, start, n, f"{route} {kind} of {n} at {start} (ring wrap)")
    x = (np.random.default_rng(8).standard_normal((2, c.hidden)) * 2).astype(np.float32)
    for m in (a, b):
        m.n_tokens = 300
    ya, ka, va = a.gemv_tap(1, 0, x, want_kv=True)
    yb, kb, vb = b.gemv_tap(1, 0, x, want_kv=True)
    assert np.array_equal(ya, yb)
    assert np.array_equal(_bits(ka), _bits(kr.fake_quant(kb))) and np.array_equal(_bits(va), _bits(kr.fake_quant(vb))), "layer 1 rows through gemv_tap"
    _assert_rows_are_q8_of(a, b, 1, 300, 2, f"{route} gemv_tap layer 1")


def test_group_and_batch_writers_store_q8_of_the_default_rows():
    """one group step of 2 members and one batch step of 3 members at different positions (the last member's rows wrap the ring)"""
    from realtime_codec_agent_amd.llm import LlamaBatch, LlamaGroup
    q8s, f16s = _family("gemm128")
    ids = sc.BY_NAME[ks.E2E_CASES["gemm128"][0]].ids().tolist()
    starts = (5, 300, 1023)
    rows = [[ids[10 + 2 * s], ids[11 + 2 * s]] for s in range(3)]
    for fam in (q8s, f16s):
        for m, st in zip(fam, starts):
            m.reset()
            m.n_tokens = st
        g = LlamaGroup(fam[:2])
        g.step(rows[:2])
        g.close()
    for s in range(2):
        assert q8s[s].n_tokens == starts[s] + 2
        _assert_rows_are_q8_of(q8s[s], f16s[s], 0, starts[s], 2, f"group member {s}")
    for fam in (q8s, f16s):
        for m, st in zip(fam, starts):
            m.n_tokens = st
        bt = LlamaBatch(fam)
        bt.step([r[::-1] for r in rows])
        bt.close()
    for s in range(3):
        assert q8s[s].n_tokens == starts[s] + 2
        _assert_rows_are_q8_of(q8s[s], f16s[s], 0, starts[s], 2, f"batch member {s}")


# ------------------------------------------------------------------ 3. attention alone
def _routes(llm):
    return (0, 1, 2) if llm.prefill_route() == "gemm128" else (0, 1)


def _tap(llm, route, q, pos0):
    llm.n_tokens = pos0
    return llm.attn_tap(0, route, q.reshape(q.shape[0], -1))


@pytest.mark.parametrize("cls", ["moderate", "peaked"])
@pytest.mark.parametrize("geom", ar.SMALL)
def test_attention_over_a_q8_cache(geom, cls):
    """K / V of attn_ref's score classes planted with kv_write and read back de-quantised; every route (decode with the merge inside and
    outside the launch) at pos0 255 / 256 / 257 and at the last positions of the cache, against attn_ref.attention over the
    de-quantised rows inside attn_ref's bound, unchanged: the values the kernels multiply are exactly those fp16 values"""
    nh, nkv = ar.GEOMS[geom]
    llm = _attn_llm(geom)
    seed = 300 + 7 * list(ar.GEOMS).index(geom) + list(ar.SCORE_CLASSES).index(cls)
    K, V = ar.class_kv(seed, ar.CLASS_T, nkv)
    llm.kv_write(0, 0, K, V)
    Kd, Vd = llm.kv_read(0, 0, ar.CLASS_T)
    assert np.array_equal(_bits(Kd), _bits(kr.fake_quant(K))) and np.array_equal(_bits(Vd), _bits(kr.fake_quant(V)))
    worst = 0.0
    for route in _routes(llm):
        M = 2 if route == 0 else 40
        q = ar.class_q(seed + 1, M, nh, ar.SCORE_CLASSES[cls])
        for pos0 in (255, 256, 257, ar.CLASS_T - M):
            want, bound = ar.attention(q, Kd, Vd, pos0, with_bound_for=route)
            for fuse in ((True, False) if route == 0 else (True,)):
                llm.set_attn_fuse(fuse)
                got = _tap(llm, route, q, pos0)
                assert np.isfinite(got).all(), f"{geom} {cls} route {route} pos0 {pos0} fuse {fuse}: non-finite output"
                ratio = float((np.abs(got - want) / bound).max())
                worst = max(worst, ratio)
                assert ratio <= 1.0, f"{geom} {cls} route {route} pos0 {pos0} fuse {fuse}: error / bound = {ratio:.3f}"
    llm.set_attn_fuse(True)
    print(f"KVQ8 attention {geom} {cls}: worst error / bound {worst:.3f}")


@pytest.mark.parametrize("geom", ar.SMALL)
def test_onehot_rows_through_the_q8_staging(geom):
    """+-1 keys quantise to themselves (d16 * 127 rounds to 1), so q = 16 k_target leads by >= 40 nats and a row's output is its
    target's de-quantised V row: key order and row mapping through the new loads and image writes, one case set per route"""
    nh, nkv = ar.GEOMS[geom]
    llm = _attn_llm(geom)
    K, V = ar.onehot_kv(ar.ONEHOT_SEED, ar.CLASS_T, nkv)
    llm.kv_write(0, 0, K, V)
    Kd, Vd = llm.kv_read(0, 0, ar.CLASS_T)
    assert np.array_equal(_bits(Kd), _bits(K)), "+-1 keys must survive the round trip exactly"
    heads = np.arange(nh) // (nh // nkv)
    pos0 = 600
    calls = [np.array([[256 + (base + 17 * h) % 256 for h in range(nh)], [(base * 2 + 31 * h + 3) % 600 for h in range(nh)]]) for base in range(0, 256, 16)]
    calls.append(np.array([[pos0] * nh, [pos0 + 1] * nh]))          # the newest keys
    for route in _routes(llm):
        sets = calls if route == 0 else [ar.flash_onehot_targets(40, nh, pos0)]
        for tg in sets:
            assert ar.onehot_lead(K, tg, nh, pos0) >= 40.0
            q = ar.onehot_q(K, tg, nh)
            want, bound = ar.attention(q, Kd, Vd, pos0, with_bound_for=route)
            assert np.abs(want - Vd[tg, heads[None, :]].astype(np.float64).reshape(want.shape)).max() < 1e-9
            for fuse in ((True, False) if route == 0 else (True,)):
                llm.set_attn_fuse(fuse)
                got = _tap(llm, route, q, pos0)
                assert np.isfinite(got).all()
                ratio = float((np.abs(got - want) / bound).max())
                assert ratio <= 1.0, f"{geom} one-hot route {route} fuse {fuse} targets {tg[:2].tolist()}: error / bound = {ratio:.3f}"
    llm.set_attn_fuse(True)


# ------------------------------------------------------------------ 4. end to end
def _tol(route):
    return (sc.TOL_EXACT if route == "gemv" else sc.TOL_TILE) + 4.0 * ks.SPREAD[route]


@functools.lru_cache(maxsize=None)
def _want(route, s):
    name, fmt = ks.E2E_CASES[route]
    c = sc.BY_NAME[name]
    return ks.ref_logits(kr.Q8KVRef(c.config(), sc.oracle_weights(c, fmt)), ks.member_ids(c, s))


@pytest.mark.parametrize("route", list(ks.E2E_CASES))
def test_end_to_end_logits(route):
    """Logits of the q8_0 handle against Q8KVRef after a 300-token eval and after each of 4 single-token steps.  Tolerance, in units of
    max(1, |logit|max): the route's existing one (lm_shape_cases.TOL_EXACT 1e-3 on the GEMV route, TOL_TILE 2e-3 on the tile routes)
    plus 4 x the spread an fp16-ulp disagreement of the pre-quantisation rows causes, measured on the CPU by tests/kv_q8_spread.py over
    5 seeds: gemv 3.38e-3, tile32 4.49e-3, gemm128 2.05e-2 -> 1.45e-2 / 2.00e-2 / 8.41e-2.  Guard: the q8_0 logits differ from the f16
    handle's (a format switch that did nothing would pass the comparison above on a model this small only by luck, and must not)."""
    q8s, f16s = _family(route)
    a, b = q8s[0], f16s[0]
    c = sc.BY_NAME[ks.E2E_CASES[route][0]]
    ids = ks.member_ids(c, 0).tolist()
    want = _want(route, 0)
    rows = {}
    for m in (a, b):
        m.reset()
        m.eval(ids[:ks.E2E_PROMPT])
        got = [m._fetch_logits().copy()]
        for t in ids[ks.E2E_PROMPT:]:
            m.eval([t])
            got.append(m._fetch_logits().copy())
        rows[m] = np.stack(got)
    err = float(np.abs(rows[a] - want).max())
    bound = sc.bound(want, _tol(route))
    diff = float(np.abs(rows[a] - rows[b]).max())
    print(f"KVQ8 end to end {route}: max |dlogit| {err:.3e} (bound {bound:.3e}), q8_0 vs f16 handle {diff:.3e}")
    assert err <= bound
    assert diff > 0.0, "the q8_0 handle computed the f16 handle's logits: the format switch did nothing"


def test_end_to_end_group_and_batch_steps():
    """the same comparison for a 2-member group step and a 3-member batch step (n = 1, four steps each) on caches built by a 300-token
    eval per member; tolerance of the 128-token tile route (see test_end_to_end_logits)"""
    from realtime_codec_agent_amd.llm import LlamaBatch, LlamaGroup
    q8s, _ = _family("gemm128")
    c = sc.BY_NAME[ks.E2E_CASES["gemm128"][0]]
    for kind, nm in (("group", 2), ("batch", 3)):
        members = q8s[:nm]
        idl = [ks.member_ids(c, s).tolist() for s in range(nm)]
        for m, ids in zip(members, idl):
            m.reset()
            m.eval(ids[:ks.E2E_PROMPT])
        drv = (LlamaGroup if kind == "group" else LlamaBatch)(members)
        worst = 0.0
        for t in range(ks.E2E_STEPS):
            drv.step([[ids[ks.E2E_PROMPT + t]] for ids in idl])
            for s, m in enumerate(members):
                want = _want("gemm128", s)
                err = float(np.abs(m._fetch_logits() - want[1 + t]).max())
                worst = max(worst, err / sc.bound(want, _tol("gemm128")))
        drv.close()
        print(f"KVQ8 end to end {kind} step: worst error / bound {worst:.3f}")
        assert worst <= 1.0


# ------------------------------------------------------------------ 5. lifecycle
def test_lifecycle_refusals_twins_and_switching_back():
    from realtime_codec_agent_amd.llm import LlamaBatch, LlamaGroup
    q8s, f16s = _family("gemm128")
    a, a2, b = q8s[0], q8s[1], f16s[0]
    ids = sc.BY_NAME[ks.E2E_CASES["gemm128"][0]].ids().tolist()
    E = _err()
    for m in (a, a2, b):
        m.reset()
    a.eval(ids[:40])
    snap = a.kv_read_q8(1, 0, 40)
    # set_kv_format at n_tokens > 0: refused, nothing touched
    with pytest.raises(E):
        a.set_kv_format("f16")
    assert a.kv_format == "q8_0" and a.n_tokens == 40
    assert all(np.array_equal(x, y) for x, y in zip(snap, a.kv_read_q8(1, 0, 40)))
    with pytest.raises(ValueError):
        a.set_kv_format("q4_0")
    # kv_remove on a q8_0 handle: refused, n_tokens unchanged
    with pytest.raises(E, match="q8_0"):
        a.kv_remove(3, 9)
    assert a.n_tokens == 40
    # across formats: copy, swap, group, batch
    with pytest.raises(E, match="format"):
        b.copy_kv_from(a, 16)
    with pytest.raises(E, match="format"):
        a.swap_kv(b)
    with pytest.raises(E, match="KV format"):
        LlamaGroup([a, b])
    with pytest.raises(E, match="KV format"):
        LlamaBatch([a, a2, b])
    # kv_read_q8 needs a q8_0 handle
    with pytest.raises(E):
        b.kv_read_q8(0, 0, 1)
    # the agent's context-shift trim is refused at construction over a q8_0 LM
    from types import SimpleNamespace
    from realtime_codec_agent_amd.realtime_agent_v2 import RealtimeAgent
    with pytest.raises(ValueError, match="q8_0"):
        RealtimeAgent(resources=SimpleNamespace(llm=a), kv_trim_mode="shift")
    # switching back to f16 on the empty handle gives the f16 handle's logits bit for bit (and its raw rows)
    a2.reset()
    a2.set_kv_format("f16")
    assert a2.kv_format == "f16" and a2.kv_ring_positions() == 0
    try:
        for m in (a2, b):
            m.reset()
            m.eval(ids[:300])
            m.step(ids[300:302])
        assert np.array_equal(a2._fetch_logits(), b._fetch_logits())
        for layer in (0, 1):
            for x, y in zip(a2.kv_read(layer, 0, 302), b.kv_read(layer, 0, 302)):
                assert np.array_equal(_bits(x), _bits(y))
    finally:
        a2.reset()
        a2.set_kv_format("q8_0")


def test_shadow_cycle_gives_the_bits_of_a_fresh_recompute():
    """copy_kv of a header, eval_async tiles, swap_kv -- the sliding-window trim's cycle (kv_shadow.py) -- leaves the live handle with the
    cache blocks a fresh q8_0 handle gets from evaluating header + suffix"""
    q8s, _ = _family("gemm128")
    a, fresh = q8s[0], q8s[2]
    ids = sc.BY_NAME[ks.E2E_CASES["gemm128"][0]].ids().tolist()
    for m in (a, fresh):
        m.reset()
    a.eval(ids[:400])
    twin = a.make_kv_shadow()
    try:
        assert twin.kv_format == "q8_0"
        head, suffix = 16, ids[150:150 + 300]
        twin.copy_kv_from(a, head)
        twin.n_tokens = head
        for i in range(0, len(suffix), 128):
            twin.eval_async(suffix[i:i + 128])
        a.swap_kv(twin)
        a.n_tokens = head + len(suffix)
        fresh.eval(ids[:head])
        fresh.eval_async(suffix[:128])
        fresh.eval_async(suffix[128:])
        fresh.sync()
        for layer in (0, 1):
            for x, y in zip(a.kv_read_q8(layer, 0, head + len(suffix)), fresh.kv_read_q8(layer, 0, head + len(suffix))):
                assert np.array_equal(x.view(np.uint16) if x.dtype == np.float16 else x, y.view(np.uint16) if y.dtype == np.float16 else y), f"layer {layer}"
        # and the live handle goes on from there like the fresh one
        a.eval(ids[700:702])
        fresh.eval(ids[700:702])
        assert np.array_equal(a._fetch_logits(), fresh._fetch_logits())
        a.swap_kv(twin)      # give the twin its own buffers back before it is closed
    finally:
        twin.close()


# ------------------------------------------------------------------ 6. agents
def test_agent_batch_over_q8_handles_fused_equals_unfused():
    """a RealtimeAgentBatch of 4 sessions over q8_0 handles: the run with one rca_duplex_batch_frame per tick equals the run with
    use_duplex_batch_graph=False on a second set of q8_0 agents -- tokens, positions and PCM.  64 ticks, so that at least 30 go through
    the duplex frame: the codec windows (32000 samples = 25 chunks of 1280) have to fill first, and a tick in which a sliding-window
    trim falls (every 0.8 s = 10 ticks once the 2 s context is full) takes the separate calls; the sessions trim through their q8_0
    shadow caches on the way (copy_kv, eval_async tiles, swap_kv)."""
    from conftest import rich_signal
    from realtime_codec_agent_amd import RealtimeAgentBatch
    from realtime_codec_agent_amd.llm import LMConfig
    from realtime_codec_agent_amd.realtime_agent_config import RealtimeAgentConfig
    from realtime_codec_agent_amd.realtime_agent_resources import RealtimeAgentResources
    from realtime_codec_agent_amd.realtime_agent_v2 import RealtimeAgent
    n_agents, ticks, chunk = 4, 64, 1280
    sig = [rich_signal(chunk * ticks, 50 + s) for s in range(n_agents)]

    def drive(fused):
        lm = LMConfig(vocab_size=259344, hidden=256, n_layers=2, n_heads=4, n_kv_heads=2, head_dim=64, ffn=512)
        res = [RealtimeAgentResources(llm_model_path="random:small", llm_n_ctx=4096, llm_config=lm, with_aux_llm=False, llm_random_seed=3, llm_kv_format="q8_0")]
        res += [res[0].clone_for_self_play() for _ in range(n_agents - 1)]
        assert all(r.llm.kv_format == "q8_0" for r in res), "clone_for_self_play carries the KV format"
        cfg = RealtimeAgentConfig(chunk_size_secs=0.08, use_whisper=False, force_trans_after_inactivity_secs=0.0,
                                  force_response_after_inactivity_secs=0.0, max_context_secs=2.0, trim_by_secs=0.8)
        agents = [RealtimeAgent(resources=r, config=cfg) for r in res]
        drv = RealtimeAgentBatch(agents, min_batch=1, use_duplex_batch_graph=fused)
        outs = [drv.process_audio([sig[s][t * chunk:(t + 1) * chunk] for s in range(n_agents)]) for t in range(ticks)]
        state = [(list(a.input_ids), a.resources.llm.n_tokens, a._kv_shadow.stats["swaps"] if a._kv_shadow is not None else 0) for a in agents]
        fused_ticks = drv.fused_ticks
        drv.close()
        return outs, state, fused_ticks

    of, sf, nf = drive(True)
    op, sp, _ = drive(False)
    assert nf >= 30, ("fused ticks", nf)
    assert any(s[2] > 0 for s in sf), "no session trimmed through its shadow cache"
    for s in range(n_agents):
        assert sf[s][0] == sp[s][0], ("input_ids of agent", s)
        assert sf[s][1] == sp[s][1], ("n_tokens of agent", s)
        for t in range(ticks):
            assert np.array_equal(of[t][s], op[t][s]), ("PCM of agent", s, "tick", t)
