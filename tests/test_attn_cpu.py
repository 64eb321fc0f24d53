"""tests/attn_ref.py checked on the host: the float64 reference is the attention inside oracle.lm_ref.LMRef, every input builder meets
the conditions its docstring states, and the derived bound has teeth: on the very inputs tests/test_attn_gpu.py uses, wrong
attentions (exchanged V rows, a dropped key, a mask off by one, exchanged kv heads, a dropped split, a missing max) lie at least
PROBE_FACTOR bounds away from the right one.  The same for the batch pass's attention (route 3, tests/test_attn_batch_gpu.py): every
ragged batch case meets the bound's precondition and its own conditions, and the wrong attentions, another member's cache, a
neighbour's rows and token 1 in token 0's row are all seen."""
import functools

import numpy as np
import pytest
import torch

import attn_ref as ar
from attn_ref import Wrong
from oracle import lm_ref

PROBE_FACTOR = 3.0     # a condition of the inputs, not a measurement: a case class that misses it gets other inputs, not a smaller factor


def test_reference_is_the_attention_inside_lmref():
    """A 1-layer G = 2 model with the MLP switched off (down_proj = 0): LMRef's logits of a second, 10-token eval on top of 30 cached
    tokens are reproduced by LMRef's own pieces around attn_ref.attention -- its norm, its RoPE helpers, its cached fp16 K / V."""
    from realtime_codec_agent_amd.llm import LMConfig
    cfg = LMConfig(vocab_size=64, hidden=128, n_layers=1, n_heads=4, n_kv_heads=2, head_dim=64, ffn=64)
    w = dict(lm_ref.random_weights(cfg, 5, 0.3))
    w["model.layers.0.mlp.down_proj.weight"] = np.zeros((cfg.hidden, cfg.ffn), np.float32)
    ref = lm_ref.LMRef(cfg, w, kv_dtype=torch.float16)
    ids = np.random.default_rng(0).integers(0, 64, 40).tolist()
    ref.eval(ids[:30])
    want = ref.eval(ids[30:]).numpy()
    p = "model.layers.0."
    x = ref.w["model.embed_tokens.weight"][torch.as_tensor(ids[30:])]
    h = ref._norm(x, ref.w[p + "input_layernorm.weight"])
    q = (h @ ref.w[p + "self_attn.q_proj.weight"].T).view(10, 4, 64).transpose(0, 1)
    freqs = torch.arange(30, 40)[:, None].float() * ref.inv_freq[None, :]
    emb = torch.cat((freqs, freqs), dim=-1)
    q = (q * emb.cos()[None] + lm_ref._rotate_half(q) * emb.sin()[None]).transpose(0, 1).contiguous().numpy()     # [10, 4, 64]
    K = ref.k[0].transpose(0, 1).contiguous().numpy().astype(np.float16)                                            # [40, 2, 64]
    V = ref.v[0].transpose(0, 1).contiguous().numpy().astype(np.float16)
    assert np.array_equal(K.astype(np.float32), ref.k[0].transpose(0, 1).numpy())                                   # the cache is fp16 already
    o = torch.from_numpy(ar.attention(q, K, V, 30).astype(np.float32))
    got = (ref._norm(x + o @ ref.w[p + "self_attn.o_proj.weight"].T, ref.w["model.norm.weight"]) @ ref.w["lm_head.weight"].T).numpy()
    scale = float(np.abs(want).max())
    print(f"attn_ref inside LMRef: max|dlogit| {np.abs(got - want).max():.2e} at max|logit| {scale:.2f}")
    assert np.abs(got - want).max() <= 2e-6 * max(1.0, scale)            # f64 attention against LMRef's f32 one
    wrong = torch.from_numpy(ar.attention(q, K, V, 30, Wrong(mask_shift=-1)).astype(np.float32))
    bad = (ref._norm(x + wrong @ ref.w[p + "self_attn.o_proj.weight"].T, ref.w["model.norm.weight"]) @ ref.w["lm_head.weight"].T).numpy()
    assert np.abs(bad - want).max() > 1e-3 * scale                       # ... and the comparison sees an attention that is not


@functools.lru_cache(maxsize=None)
def _onehot(nkv):
    return ar.onehot_kv(ar.ONEHOT_SEED, ar.ONEHOT_T, nkv)


@pytest.mark.parametrize("geom", list(ar.GEOMS))
def test_onehot_inputs_meet_their_conditions(geom):
    nh, nkv = ar.GEOMS[geom]
    K, V = _onehot(nkv)
    assert set(np.unique(K.astype(np.float32))) == {-1.0, 1.0} and np.isfinite(V.astype(np.float32)).all()
    assert 200 < np.abs(V.astype(np.float32)).max() <= 300
    for g in range(nkv):
        assert len(np.unique(V[:, g].view(np.uint16), axis=0)) == ar.ONEHOT_T, "two keys share a V row"
    lead = np.inf
    if geom in ar.SMALL:
        calls = ar.decode_onehot_calls(nh)
        offsets = set()
        for pos0, tg in calls:
            assert len(set(tg.ravel().tolist())) == tg.size, "the rows of a call target different keys"
            offsets |= {int(k) % 256 for k in tg.ravel()}
            lead = min(lead, ar.onehot_lead(K, tg, nh, pos0))
        assert offsets == set(range(256))                                   # 8 waves x 32 register slots
        hit = {int(k) for _, tg in calls for k in tg.ravel()}
        assert {0, 31, 32, 255, 256, 511, 512, 767} <= hit
        assert any(tg.shape[0] == 2 and pos0 in tg[0] and pos0 + 1 in tg[1] for pos0, tg in calls)
        assert any(tg.shape[0] == 1 and pos0 in tg[0] for pos0, tg in calls)
    for M in ar.FLASH_ONEHOT_M if geom in ar.SMALL else (64,):
        tg = ar.flash_onehot_targets(M, nh, ar.FLASH_POS0)
        lead = min(lead, ar.onehot_lead(K, tg, nh, ar.FLASH_POS0))
        flat = tg.ravel()
        for r0 in range(0, flat.size, 32):
            assert len(set(flat[r0:r0 + 32].tolist())) == min(32, flat.size - r0), "two rows of a 32-row tile share a target"
        if M == 1024:
            assert {(int(k) >> 5) % 3 * 32 + int(k) % 32 for k in flat} == set(range(96))     # every slot of each wave's blocks
            assert (flat > ar.FLASH_POS0).sum() > 100 and (tg[:, 0] == ar.FLASH_POS0 + np.arange(M)).sum() >= 1   # masked blocks, own key
    print(f"{geom}: smallest one-hot lead {lead:.1f} nats")
    assert lead >= 40.0                                                     # if this fails: reseed, do not lower 40


def test_class_inputs_meet_their_conditions():
    for cls, sigma in ar.SCORE_CLASSES.items():
        for off in ar.OFFSETS:
            K, V, q, pos0 = ar.class_case("g2", cls, off, 1)
            assert 600 <= pos0 + q.shape[0] <= 700
            s = np.einsum("mhd,thd->mht", q.astype(np.float64), np.repeat(K.astype(np.float64), 2, axis=1)) * ar.SCALE
            assert abs(np.median(s) - off) < max(0.5, 0.2 * sigma), (cls, off)
            assert 0.7 * sigma < s.std() < 1.4 * sigma, (cls, off, s.std())
            if cls == "peaked":
                assert 45 < np.abs(s - off).max() < 90
            v = V.astype(np.float64)
            assert (v > 0).mean() > 0.4 and (v < 0).mean() > 0.4 and np.abs(v).max() > 100 and np.median(np.abs(v)) < 2
    for pattern in ar.LONG_PATTERNS[1:]:
        for nsp in ar.LONG_SPLITS:
            K, V, q, pos0 = ar.long_case("g2", nsp, pattern)
            s = np.einsum("mhd,thd->mht", q.astype(np.float64), np.repeat(K.astype(np.float64), 2, axis=1)) * ar.SCALE
            top = s.max(-1, keepdims=True)
            at = int(s[0, 0].argmax())
            assert at // 256 == (0 if pattern == "dominant first" else nsp - 1)
            rest = np.delete(s, at, axis=-1)
            assert (top[..., 0] - rest.max(-1)).min() >= 60.0, pattern       # everything else is 60 nats below the planted key


def _probe(tag, q, K, V, pos0, route, wrong, rows=slice(None)):
    o, b = _right(tag, q, K, V, pos0, route)
    r = ar.far(ar.attention(q, K, V, pos0, wrong)[rows], o[rows], b[rows])
    return r


_cache = {}


def _right(tag, q, K, V, pos0, route):
    if (tag, route) not in _cache:
        _cache[(tag, route)] = ar.attention(q, K, V, pos0, with_bound_for=route)
    return _cache[(tag, route)]


@pytest.mark.parametrize("geom", ar.SMALL)
def test_bound_sees_exchanged_v_rows_and_lost_keys_on_the_onehot_inputs(geom):
    """one-hot rows: the target's V row exchanged with its neighbour inside the 32-key block, the target dropped (at the seams 31 / 32,
    255 / 256 and at the newest key), the mask one key short at a row that targets its own position"""
    nh, nkv = ar.GEOMS[geom]
    K, V = _onehot(nkv)
    worst = {"swap": np.inf, "drop": np.inf, "mask": np.inf}
    dec = [(0, p, tg) for p, tg in ar.decode_onehot_calls(nh)]
    calls = [c for c in dec if c[1] == 800] + [c for c in dec if c[1] != 800][::3]      # the seam keys all, a third of the others
    calls += [(route, ar.FLASH_POS0, ar.flash_onehot_targets(M, nh, ar.FLASH_POS0)) for route in (1, 2) for M in (33, 7)]
    seams = set()
    for i, (route, pos0, tg) in enumerate(calls):
        q = ar.onehot_q(K, tg, nh)
        tag = ("onehot", geom, i)
        for t in set(tg.ravel().tolist()) if tg.size <= 8 else {int(tg[0, 0]), int(tg[-1, -1])}:
            other = t ^ 1 if (t ^ 1) < pos0 + tg.shape[0] else t - 1          # a neighbour that exists, in the same 32-key block
            if other >> 5 == t >> 5:
                worst["swap"] = min(worst["swap"], _probe(tag, q, K, V, pos0, route, Wrong(swap_v=(t, other))))
            worst["drop"] = min(worst["drop"], _probe(tag, q, K, V, pos0, route, Wrong(drop_key=t)))
            seams.add(t if t < 768 else -1 if t == pos0 + tg.shape[0] - 1 else -2)
        own = [(m, h) for m in range(tg.shape[0]) for h in range(nh) if tg[m, h] == pos0 + m]
        if own:
            worst["mask"] = min(worst["mask"], _probe(tag, q, K, V, pos0, route, Wrong(mask_shift=-1)))
    print(f"{geom} one-hot probes, in bounds: " + ", ".join(f"{k} {v:.3g}" for k, v in worst.items()))
    assert min(worst.values()) >= PROBE_FACTOR, worst
    assert -1 in seams and seams & {31, 32} and seams & {255, 256}, seams


@pytest.mark.parametrize("route", (0, 1, 2))
@pytest.mark.parametrize("geom", ar.SMALL)
def test_bound_sees_the_wrong_attentions_on_the_class_inputs(geom, route):
    """every score class: exchanged kv heads and a dropped split; the classes with an offset of +80 nats and a spread: a missing max
    (fp32 exp overflows); the classes whose weights are spread over many keys (flat and moderate, no offset: a single key carries
    1 / 600 of a row there, in the peaked classes all but a handful carry nothing, and the offset classes' bound is dominated by
    the 80-nat component's accumulation error): a V exchange inside a 32-key block, a key dropped at 31 / 32, 255 / 256 and at the end,
    the causal mask off by one either way."""
    nh, nkv = ar.GEOMS[geom]
    lines = []
    for cls in ar.SCORE_CLASSES:
        for off in ar.OFFSETS:
            K, V, q, pos0 = ar.class_case(geom, cls, off, route)
            M = q.shape[0]
            tag = ("class", geom, cls, off)
            probes = {"split 1 dropped": Wrong(drop_split=1), "split 2 dropped": Wrong(drop_split=2)}
            if nkv > 1:
                probes["kv heads 0 / 1 exchanged"] = Wrong(swap_kv_heads=(0, 1))
            if off > 0 and cls != "flat":
                probes["no max"] = Wrong(no_max=True)
            if off == 0 and cls == "flat":
                probes.update({f"key {k} dropped": Wrong(drop_key=k) for k in (31, 32, 255, 256, pos0 + M - 1)})
                probes["V rows 300 / 301 exchanged"] = Wrong(swap_v=(300, 301))
                probes["mask one short"] = Wrong(mask_shift=-1)
            got = {k: _probe(tag, q, K, V, pos0, route, w) for k, w in probes.items()}
            if off == 0 and cls == "flat":
                got["mask one long"] = _probe(tag, q, K, V, pos0, route, Wrong(mask_shift=1), rows=slice(0, M - 1))
            lines.append(f"{cls}{off:+.0f}: " + ", ".join(f"{k} {v:.3g}" for k, v in got.items()))
            assert min(got.values()) >= PROBE_FACTOR, (geom, route, cls, off, got)
    print(f"{geom} route {route} class probes, in bounds:\n  " + "\n  ".join(lines))


@pytest.mark.parametrize("geom", ("g2", "g4"))
def test_bound_sees_a_dropped_split_on_the_long_inputs(geom):
    for nsp in ar.LONG_SPLITS:
        for pattern in ar.LONG_PATTERNS:
            K, V, q, pos0 = ar.long_case(geom, nsp, pattern)
            drop = {"moderate": nsp // 2, "dominant first": 0, "dominant last": nsp - 1}[pattern]
            r = _probe(("long", geom, nsp, pattern), q, K, V, pos0, 0, Wrong(drop_split=drop))
            print(f"{geom} {nsp} splits, {pattern}: split {drop} dropped = {r:.3g} bounds")
            assert r >= PROBE_FACTOR, (geom, nsp, pattern, r)


# ------------------------------------------------------------------ the batch pass's attention (route 3)
def _batch_cases():
    """(tag, n, members) of every case tests/test_attn_batch_gpu.py plants"""
    for nm, n in ar.BATCH_ONEHOT_SHAPES:
        yield ("onehot", nm, n), n, ar.batch_onehot_members(nm, n)
    for cls in ar.SCORE_CLASSES:
        for off in ar.OFFSETS:
            yield ("class", cls, off), 2, ar.batch_class_members(cls, off)
    for n in (1, 2):
        yield ("seams", n), n, ar.batch_seam_members(n)
        for variant in ar.BATCH_RAGGED:
            yield ("ragged", variant, n), n, ar.batch_ragged_members(n, variant)


@functools.lru_cache(maxsize=None)
def _batch_right(geom, n, mb):
    K, V, q, _ = ar.batch_member_inputs(geom, n, mb)
    return ar.attention(q, K, V, mb.pos0, with_bound_for=ar.BATCH_ROUTE)


def _batch_probe(geom, n, mb, wrong, rows=slice(None)):
    K, V, q, _ = ar.batch_member_inputs(geom, n, mb)
    o, b = _batch_right(geom, n, mb)
    with np.errstate(invalid="ignore"):       # a token that is left without a visible key comes out NaN: infinitely far
        return ar.far(ar.attention(q, K, V, mb.pos0, wrong)[rows], o[rows], b[rows])


@pytest.mark.parametrize("geom", list(ar.BATCH_GEOMS))
def test_batch_cases_meet_the_bounds_precondition_and_their_own_conditions(geom):
    """every member of every batch case: the bound's first-order form applies (attention() asserts S_a < 0.5 where it forms the
    bound); it fits its cache; one-hot members lead by 40 nats with targets that all differ, each token's own position among them;
    the ragged cases launch both sides of CMB_PRE = 32 and of the merge's 64-split tail; the family has a twin for every member"""
    nh, nkv = ar.BATCH_GEOMS[geom]
    lead, splits = np.inf, set()
    for tag, n, members in _batch_cases():
        assert len(members) * n <= 128 and 2 <= len(members) <= 64
        pool = list(ar.BATCH_FAMILY_CTX)
        for mb in members:
            pool.remove(mb.n_ctx)                                             # ValueError: the family has no twin left with this n_ctx
            K, V, q, tg = ar.batch_member_inputs(geom, n, mb)
            want, bound = _batch_right(geom, n, mb)
            assert np.isfinite(want).all() and np.isfinite(bound).all() and (bound > 0).all(), (tag, mb)
            if tg is not None:
                assert len(set(tg.ravel().tolist())) == tg.size and all(mb.pos0 + j in tg[j] for j in range(n)), (tag, mb)
                lead = min(lead, ar.onehot_lead(K, tg, nh, mb.pos0))
                heads = np.arange(nh) // (nh // nkv)
                assert np.abs(want - V[tg, heads[None, :]].astype(np.float64).reshape(want.shape)).max() < 1e-9
            if tag[0] == "ragged":
                splits.add(ar.splits_needed(mb.pos0, n))
        if tag[0] == "ragged":
            splits |= set(ar.batch_launches(members, n))
    print(f"{geom}: smallest one-hot lead of the batch members {lead:.1f} nats; ragged split counts {sorted(splits)}")
    assert lead >= 40.0                                                       # if this fails: reseed, do not lower 40
    assert {1, 3, 32, 33, 64, 65} <= splits
    for n in (1, 2):                                                          # -1: the member's last slot, n_ctx - n
        starts = [mb.pos0 if mb.pos0 + n < mb.n_ctx else -1 for mb in ar.batch_seam_members(n)]
        assert set(starts) == {0, 1, 254, 255, 256, 257, 511, 512, -1} and starts.count(-1) == 4, starts


@pytest.mark.parametrize("geom", list(ar.BATCH_GEOMS))
def test_batch_bound_sees_the_wrong_attentions(geom):
    """the route-3 bound has teeth on the batch cases, each wrong variant where it can bite: one-hot members (the target's V row
    exchanged inside its 32-key block, the target dropped, the mask one short at the row that targets its own position), class
    members (kv heads exchanged, a split dropped; the flat class without offset: the mask one long), long ragged members (the split
    that holds the dominant key dropped)"""
    nh, nkv = ar.BATCH_GEOMS[geom]
    worst = {}

    def note(k, r):
        worst[k] = min(worst.get(k, np.inf), r)

    for nm, n in ((5, 2), (33, 1)):
        for mb in ar.batch_onehot_members(nm, n)[::4]:
            tg = ar.batch_member_inputs(geom, n, mb)[3]
            for t in {int(tg[0, 0]), int(tg[-1, -1]), mb.pos0, mb.pos0 + n - 1}:
                other = t ^ 1 if (t ^ 1) < mb.pos0 + n else t - 1
                note("swap_v", _batch_probe(geom, n, mb, Wrong(swap_v=(t, other))))
                note("drop_key", _batch_probe(geom, n, mb, Wrong(drop_key=t)))
            note("mask_shift -1", _batch_probe(geom, n, mb, Wrong(mask_shift=-1)))
    for cls in ar.SCORE_CLASSES:
        for off in ar.OFFSETS:
            for mb in ar.batch_class_members(cls, off):
                note("swap_kv_heads", _batch_probe(geom, 2, mb, Wrong(swap_kv_heads=(0, 1))))
                for sp in range(ar.splits_needed(mb.pos0, 1)):           # every split both tokens see keys of
                    note("drop_split", _batch_probe(geom, 2, mb, Wrong(drop_split=sp)))
                if cls == "flat" and off == 0:
                    note("mask_shift +1", _batch_probe(geom, 2, mb, Wrong(mask_shift=1), rows=slice(0, 1)))
                    note("mask_shift -1", _batch_probe(geom, 2, mb, Wrong(mask_shift=-1)))
    for variant in ar.BATCH_RAGGED:
        for mb in ar.batch_ragged_members(2, variant):
            if mb.kind.startswith("dominant"):
                sp = 0 if mb.kind == "dominant first" else (mb.pos0 - 2) // ar.ATT_KEYS
                note("drop_split (dominant)", _batch_probe(geom, 2, mb, Wrong(drop_split=sp)))
    print(f"{geom} batch probes, in bounds: " + ", ".join(f"{k} {v:.3g}" for k, v in worst.items()))
    assert set(worst) == {"swap_v", "drop_key", "mask_shift -1", "mask_shift +1", "swap_kv_heads", "drop_split", "drop_split (dominant)"}
    assert min(worst.values()) >= PROBE_FACTOR, worst


@pytest.mark.parametrize("geom", list(ar.BATCH_GEOMS))
def test_batch_bound_sees_a_wrong_table_entry_and_a_wrong_row0(geom):
    """what only a batch can get wrong: member A's rows computed over member B's cache and position (a wrong table entry), the
    rows of a member written where its neighbour's belong (a wrong row0), token 1 written over token 0 (row0 + m without the m)"""
    worst = {"table": np.inf, "row0": np.inf, "token": np.inf}
    for tag, n, members in _batch_cases():
        if tag[0] == "onehot" and tag[1] > 5:
            continue
        want, bound = ar.batch_reference(geom, n, members)
        for k, mb in enumerate(members):
            other = members[(k + 1) % len(members)]
            rows, orows = slice(k * n, k * n + n), slice(((k + 1) % len(members)) * n, ((k + 1) % len(members)) * n + n)
            worst["row0"] = min(worst["row0"], ar.far(want[orows], want[rows], bound[rows]))
            q = ar.batch_member_inputs(geom, n, mb)[2]
            Ko, Vo = ar.batch_member_inputs(geom, n, other)[:2]
            worst["table"] = min(worst["table"], ar.far(ar.attention(q, Ko, Vo, other.pos0), want[rows], bound[rows]))
            if n == 2 and not mb.kind.startswith("dominant"):     # (both tokens of a dominant member attend to the one planted key)
                worst["token"] = min(worst["token"], ar.far(want[k * n + 1], want[k * n], bound[k * n]))
    print(f"{geom} batch-only probes, in bounds: " + ", ".join(f"{k} {v:.3g}" for k, v in worst.items()))
    assert min(worst.values()) >= PROBE_FACTOR, worst
