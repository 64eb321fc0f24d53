"""The decode attention of a batch pass run alone (rca_lm_batch_attn_tap over K / V planted with rca_lm_kv_write) against the float64
reference and the derived per-element bound of tests/attn_ref.py, route 3: lm_attn_mfma_kernel<G, TAB = true, KVQ>, which takes
everything about a member from its table entry, and lm_attn_mfma_batch_combine_kernel<G>, which merges the splits the member has
into its rows of the bf16 hi / lo planes.  The tap makes the very launches rca_lm_batch_step / _frame / their _sel forms and
rca_duplex_batch_frame make per layer (one helper, lm_batch_launch_attn) over tables staged the way those calls stage theirs.

Members are share_weights_with= twins of a 2-layer random model, each with an n_ctx of its own (attn_ref.BATCH_FAMILY_CTX: 1, 3, 4,
33 and 65 splits); nothing is evaluated to reach a context.  One-hot rows pin member, kv head, split and row0; the score classes,
the member seams and the ragged caches are held to the bound; every member of the seam and ragged cases must also carry, bit for
bit, the bf16 hi + lo split of what the single-handle decode launch (rca_lm_attn_tap, route 0, separate combine) gives for that
member alone; slots, companions and tables must not matter; dead slots of a selection must not write.  The tap fills every live
member's partial buffer with NaN before the launch, so a partial that the merge uses without a workgroup having written it shows.
The tapped layer is 1 (the other layer's cache holds other rows), except for the one-hot rows.

Every comparison prints its worst error / bound ratio; test_report_of_worst_ratios sums them up per G, cache format and class."""
import dataclasses
import functools

import numpy as np
import pytest

import attn_ref as ar
import gemm128_ref as gr
import lm_shape_cases as sc

pytestmark = pytest.mark.gpu

WORST = {}          # (geometry, cache format, class) -> worst error / bound ratio seen
LAYER = 1
GREEDY = dict(top_k=1, top_p=1.0, min_p=0.0, temp=0.0, seed=1)
G4 = sc.BY_NAME["g4_k768"]
MODELS = {"g4": G4, "g1": sc.BY_NAME["g1_k768"], "g2": dataclasses.replace(G4, name="g2_k768", n_heads=6, n_kv_heads=3, seed=44)}
FAMILIES = (("g1", "f16"), ("g2", "f16"), ("g4", "f16"), ("g4", "q8_0"), ("g1", "q8_0"))
FAMILY_IDS = [f"{g}-{f}" for g, f in FAMILIES]
SEAM_FAMILIES = (("g4", "f16"), ("g1", "f16"), ("g4", "q8_0"), ("g1", "q8_0"))
SEAM_IDS = [f"{g}-{f}" for g, f in SEAM_FAMILIES]


@functools.lru_cache(maxsize=None)
def _family(geom, kvf):
    """64 twins over one set of weights, twin s with n_ctx BATCH_FAMILY_CTX[s], every one with a sampler (a batch pass refuses a
    member without)"""
    from realtime_codec_agent_amd.llm import LlamaForAlternatingCodeChannels as L
    c = MODELS[geom]
    assert (c.n_heads, c.n_kv_heads) == ar.BATCH_GEOMS[geom] and c.config().n_layers == 2
    ctx = ar.BATCH_FAMILY_CTX
    big = ctx.index(max(ctx))                              # the parent's RoPE tables serve every twin: it is the longest one
    parent = L(model_path=f"random:{c.name}", config=c.config(), n_ctx=ctx[big], random_seed=c.seed, init_std=sc.INIT_STD, device=0,
               weight_format="bf16", kv_format=kvf)
    assert parent.prefill_route() == "gemm128" and parent.kv_format == kvf
    fam = [parent if s == big else L(n_ctx=x, share_weights_with=parent, device=0) for s, x in enumerate(ctx)]
    for m, x in zip(fam, ctx):
        assert m.kv_format == kvf
        m.init_sampler_for_generate(**GREEDY)
        m._ctx, m._planted = x, None
    return fam


def _pick(fam, members):
    """a twin of its own with the member's n_ctx for every member, the first free one in slot order"""
    free, out = list(range(len(fam))), []
    for mb in members:
        i = next(i for i in free if fam[i]._ctx == mb.n_ctx)
        free.remove(i)
        out.append(fam[i])
    return out


def _plant(llm, geom, n, mb, layer):
    """the member's rows into `layer` of the twin's cache, other rows (K and V exchanged) into the other layer; returns the rows the
    cache then holds at `layer`: the planted ones, or for a q8_0 cache their de-quantised blocks"""
    K, V, _, _ = ar.batch_member_inputs(geom, n, mb)
    tag = (geom, n, mb, layer)
    if llm._planted != tag:
        llm.kv_write(layer, 0, K, V)
        llm.kv_write(1 - layer, 0, V, K)
        llm._planted = tag
        llm._rows = llm.kv_read(layer, 0, K.shape[0]) if llm.kv_format == "q8_0" else (K, V)
    return llm._rows


def _stage(fam, geom, n, members, layer=LAYER):
    """(twins, q rows of the pass, the rows their caches hold): every member planted and at its start position"""
    hs = _pick(fam, members)
    kv = [_plant(h, geom, n, mb, layer) for h, mb in zip(hs, members)]
    for h, mb in zip(hs, members):
        h.n_tokens = mb.pos0
    q = np.concatenate([ar.batch_member_inputs(geom, n, mb)[2].reshape(n, -1) for mb in members])
    return hs, q, kv


@functools.lru_cache(maxsize=None)
def _reference_f16(geom, n, members):
    return ar.batch_reference(geom, n, list(members))


def _reference(geom, kvf, n, members, kv):
    """once per case for an fp16 cache; over the de-quantised rows the cache holds for a q8_0 one"""
    return _reference_f16(geom, n, tuple(members)) if kvf == "f16" else ar.batch_reference(geom, n, members, kv=kv)


def _check(tag, got, want, bound, key):
    """finite first (a NaN is a poisoned partial that the merge used, or a row nobody wrote), then every element within its bound"""
    assert np.isfinite(got).all(), f"{tag}: rows {np.flatnonzero(~np.isfinite(got).all(1)).tolist()} hold NaN / Inf"
    err = np.abs(got - want)
    with np.errstate(divide="ignore"):     # an element with no error at all is inside any bound, a bound of 0 included (a single visible key
        per = np.divide(err, bound, out=np.zeros_like(err), where=err > 0)      # whose de-quantised V element is 0: out = 0 exactly)
    ratio = float(per.max())
    WORST[key] = max(WORST.get(key, 0.0), ratio)
    assert ratio <= 1.0, f"{tag}: error / bound = {ratio:.3f} at row {int(per.max(1).argmax())}"
    return ratio


def _alone(h, layer, q_rows, pos0, nsp):
    """the member's rows by the single-handle decode launch with the separate combine, split into bf16 hi + lo (round to nearest
    even, lo = rne(ov - hi)) and summed in f32: what the batch merge promises to store"""
    h.set_attn_fuse(False)
    try:
        h.n_tokens = pos0
        ov = h.attn_tap(layer, 0, q_rows, nsp)
    finally:
        h.set_attn_fuse(True)
    assert np.isfinite(ov).all()
    hi, lo = gr.split(ov)
    return (hi + lo).astype(np.float32)


def _assert_bits_of_the_single_handle_launch(tag, hs, members, n, q, got, nsp_launch, layer=LAYER):
    launched = nsp_launch or max(ar.splits_needed(mb.pos0, n) for mb in members)
    for k, (h, mb) in enumerate(zip(hs, members)):
        rows = slice(k * n, k * n + n)
        want = _alone(h, layer, q[rows], mb.pos0, min(launched, -(-mb.n_ctx // ar.ATT_KEYS)))
        assert np.array_equal(got[rows], want), (f"{tag}: member {k} (n_ctx {mb.n_ctx}, pos0 {mb.pos0}) differs from its single-handle launch in "
                                                 f"{int((got[rows] != want).sum())} elements, max |d| {np.abs(got[rows] - want).max():.3e}")


def _batch(hs):
    from realtime_codec_agent_amd.llm import LlamaBatch
    return LlamaBatch(hs)


# ------------------------------------------------------------------ a. one-hot rows
@pytest.mark.parametrize("nm,n", ar.BATCH_ONEHOT_SHAPES, ids=[f"{a}x{b}" for a, b in ar.BATCH_ONEHOT_SHAPES])
@pytest.mark.parametrize("geom", list(ar.BATCH_GEOMS))
def test_onehot_rows_pin_member_head_split_and_row0(geom, nm, n):
    """q = 16 * k_target over +-1 keys, a seed per member: a row's output is its target's V row of ITS member's cache and kv head
    (leads of 40 nats and targets that all differ are asserted in test_attn_cpu.py), within the bound; the rows behind the pass
    keep the NaN they were filled with.  2, 5, 33 and 64 members in their own slots, layer 0."""
    fam = _family(geom, "f16")
    members = ar.batch_onehot_members(nm, n)
    hs, q, kv = _stage(fam, geom, n, members, layer=0)
    want, bound = _reference(geom, "f16", n, members, kv)
    bat = _batch(hs)
    try:
        got = bat.attn_tap(0, q, n, out_rows=128)
    finally:
        bat.close()
    assert [h.n_tokens for h in hs] == [mb.pos0 for mb in members]
    assert np.isnan(got[nm * n:]).all(), f"{geom} {nm} x {n}: rows behind the pass were written"
    r = _check(f"{geom} one-hot {nm} x {n}", got[:nm * n], want, bound, (geom, "f16", "one-hot"))
    print(f"BATTN {geom} one-hot, {nm} members x {n}: worst error / bound {r:.3f}")


# ------------------------------------------------------------------ b. score classes
@pytest.mark.parametrize("geom,kvf", FAMILIES, ids=FAMILY_IDS)
def test_accuracy_over_score_classes(geom, kvf):
    """flat, moderate and peaked scores, plain and with +80 / -80 nats on every key, five members with inputs, cache sizes and
    positions of their own (n = 2), layer 1 of both cache formats"""
    fam = _family(geom, kvf)
    bat, lines = None, []
    try:
        for cls in ar.SCORE_CLASSES:
            for off in ar.OFFSETS:
                members = ar.batch_class_members(cls, off)
                hs, q, kv = _stage(fam, geom, 2, members)
                bat = bat or _batch(hs)
                assert bat.members == hs
                want, bound = _reference(geom, kvf, 2, members, kv)
                r = _check(f"{geom} {kvf} {cls}{off:+.0f}", bat.attn_tap(LAYER, q, 2), want, bound, (geom, kvf, f"{cls}{off:+.0f}"))
                lines.append(f"{cls}{off:+.0f} {r:.3f}")
    finally:
        if bat:
            bat.close()
    print(f"BATTN {geom} {kvf} score classes, worst error / bound: " + ", ".join(lines))


# ------------------------------------------------------------------ c. member seams (and f: the single-handle launch's bits)
@pytest.mark.parametrize("n", (1, 2))
@pytest.mark.parametrize("geom,kvf", SEAM_FAMILIES, ids=SEAM_IDS)
def test_member_seams(geom, kvf, n):
    """twelve members in one batch, started at 0, 1, 254, 255, 256, 257, 511, 512 and at the last slot of each cache size (n = 2
    straddles a split: the member at 255 has token 0 in one split and token 1 in two), launched with the splits they need and with the
    4-split bucket (members with 1 to 3 splits leave the others at once): within the bound, and every member's rows are the bits of
    its own single-handle launch"""
    fam = _family(geom, kvf)
    members = ar.batch_seam_members(n)
    hs, q, kv = _stage(fam, geom, n, members)
    want, bound = _reference(geom, kvf, n, members, kv)
    bat = _batch(hs)
    worst = 0.0
    try:
        launches = ar.batch_launches(members, n)
        assert launches == [0, 4]
        for nsp in launches:
            got = bat.attn_tap(LAYER, q, n, nsp)
            worst = max(worst, _check(f"{geom} {kvf} seams n {n} nsp_launch {nsp}", got, want, bound, (geom, kvf, "moderate+0")))
            _assert_bits_of_the_single_handle_launch(f"{geom} {kvf} seams n {n} nsp_launch {nsp}", hs, members, n, q, got, nsp)
            for h, mb in zip(hs, members):
                h.n_tokens = mb.pos0
    finally:
        bat.close()
    print(f"BATTN {geom} {kvf} member seams, n = {n}: {len(members)} members x launches {launches}, worst error / bound {worst:.3f}; "
          f"== the single-handle launches, bit for bit")


# ------------------------------------------------------------------ d. ragged caches (and f)
@pytest.mark.parametrize("n", (1, 2))
@pytest.mark.parametrize("variant", ar.BATCH_RAGGED)
@pytest.mark.parametrize("geom,kvf", SEAM_FAMILIES, ids=SEAM_IDS)
def test_ragged_caches(geom, kvf, variant, n):
    """caches of 256, 700, 8448 and 16640 positions (1, 3, 33 and 65 splits: both sides of CMB_PRE and of the merge's 64-split
    tail) in one batch, launched with what the members need and with every graph bucket from there up: members with fewer splits
    than the launch leave at once, a long cache at a short context takes the empty-split path over its NaN-filled partials.
    Within the bound, finite, and the bits of every member's own single-handle launch."""
    fam = _family(geom, kvf)
    members = ar.batch_ragged_members(n, variant)
    hs, q, kv = _stage(fam, geom, n, members)
    want, bound = _reference(geom, kvf, n, members, kv)
    bat = _batch(hs)
    worst = 0.0
    try:
        launches = ar.batch_launches(members, n)
        for nsp in launches:
            got = bat.attn_tap(LAYER, q, n, nsp)
            for k, mb in enumerate(members):
                worst = max(worst, _check(f"{geom} {kvf} ragged {variant} n {n} nsp_launch {nsp} member {k}", got[k * n:k * n + n], want[k * n:k * n + n],
                                          bound[k * n:k * n + n], (geom, kvf, mb.kind if mb.kind != "moderate" else "moderate+0")))
            _assert_bits_of_the_single_handle_launch(f"{geom} {kvf} ragged {variant} n {n} nsp_launch {nsp}", hs, members, n, q, got, nsp)
            for h, mb in zip(hs, members):
                h.n_tokens = mb.pos0
    finally:
        bat.close()
    print(f"BATTN {geom} {kvf} ragged caches, {variant}, n = {n}: launches {launches}, worst error / bound {worst:.3f}; == the single-handle "
          f"launches, bit for bit")


# ------------------------------------------------------------------ g. independence
@pytest.mark.parametrize("geom,kvf", (("g4", "f16"), ("g2", "q8_0")), ids=("g4-f16", "g2-q8_0"))
def test_a_members_rows_do_not_depend_on_slot_companions_or_table(geom, kvf):
    """the member that starts at 255 with two tokens: the same bits in slot 0, in the last slot, beside other companions, with more
    splits launched, in the batch's own table and in selection tables"""
    fam = _family(geom, kvf)
    members = ar.batch_seam_members(2)
    hs, q, _ = _stage(fam, geom, 2, members)
    x = 3
    assert members[x].pos0 == 255
    rows = lambda order: np.concatenate([q[2 * k:2 * k + 2] for k in order])
    outs = {}
    for name, order in (("slot 0", (x, 0, 1)), ("last slot", (4, 5, 6, 7, x)), ("other companions", (8, x)), ("twelve", tuple(range(12)))):
        bat = _batch([hs[k] for k in order])
        try:
            at = order.index(x)
            outs[name] = bat.attn_tap(LAYER, rows(order), 2)[2 * at:2 * at + 2]
            if name == "twelve":
                outs["twelve, 4 splits launched"] = bat.attn_tap(LAYER, rows(order), 2, 4)[2 * at:2 * at + 2]
                for sel in ((x,), (9, x, 0), (11, 10, 9, 8, 7, 6, 5, 4, x)):
                    got = bat.attn_tap(LAYER, rows(sel), 2, sel=sel)
                    outs[f"selection {sel}"] = got[2 * sel.index(x):2 * sel.index(x) + 2]
        finally:
            bat.close()
    for name, o in outs.items():
        assert np.isfinite(o).all(), name
        assert np.array_equal(o, outs["slot 0"]), f"{geom} {kvf}: the member's rows differ between 'slot 0' and '{name}'"
    print(f"BATTN {geom} {kvf}: one member, the same bits in {len(outs)} settings: " + ", ".join(outs))


# ------------------------------------------------------------------ h. dead slots and neighbours
SELECTIONS = ((5,), (7, 2, 11), (15, 0, 8, 3, 12, 6, 9, 1, 14))


def test_dead_slots_write_nothing_and_bystanders_are_left_alone():
    """selections of 1, 3 and 9 of a 16-member batch (classes of 8, 8 and 16 slots): live rows within the bound, every other row
    of the block still NaN; nobody's n_tokens moves; a bystander's partials, NaN-filled by a tap of its own, change nothing for the
    selection, and its next single-handle launch gives its batch rows; a batch step right behind the taps gives the logits and
    tokens of a batch that was never tapped, bit for bit"""
    geom, kvf, n = "g4", "f16", 2
    fam = _family(geom, kvf)
    members = ar.batch_onehot_members(16, n)
    ids = MODELS[geom].ids().tolist()
    step_rows = [[ids[100 + 2 * s], ids[101 + 2 * s]] for s in range(16)]
    hs, q, kv = _stage(fam, geom, n, members)
    ref = _batch(hs)                                       # never tapped
    try:
        tokens0 = ref.step(step_rows)
        logits0 = [h._scores[-1].copy() for h in hs]
    finally:
        ref.close()
    assert all(np.isfinite(l).all() for l in logits0)
    for h in hs:                                           # the step wrote rows pos0, pos0 + 1 of both layers
        h._planted = None
    hs, q, kv = _stage(fam, geom, n, members)
    want, bound = _reference(geom, kvf, n, members, kv)
    pick = lambda a, sel: np.concatenate([a[n * k:n * k + n] for k in sel])
    bat = _batch(hs)
    try:
        for sel in SELECTIONS:
            got = bat.attn_tap(LAYER, pick(q, sel), n, sel=sel, out_rows=128)
            live = len(sel) * n
            assert np.isnan(got[live:]).all(), f"selection {sel}: rows of dead slots or behind the block were written: {np.flatnonzero(~np.isnan(got[live:]).all(1)) + live}"
            r = _check(f"selection {sel}", got[:live], pick(want, sel), pick(bound, sel), (geom, kvf, "one-hot"))
            assert [h.n_tokens for h in hs] == [mb.pos0 for mb in members]
            bystander = next(k for k in range(16) if k not in sel)
            alone = bat.attn_tap(LAYER, pick(q, (bystander,)), n, sel=(bystander,))     # fills the bystander's partials with NaN, rewrites what it needs
            again = bat.attn_tap(LAYER, pick(q, sel), n, sel=sel, out_rows=128)
            assert np.array_equal(again, got, equal_nan=True), f"selection {sel}: the rows changed with bystander {bystander}'s partials"
            launched = max(ar.splits_needed(members[k].pos0, n) for k in sel)
            big = bat.attn_tap(LAYER, pick(q, (bystander,)), n, max(launched, ar.splits_needed(members[bystander].pos0, n)), sel=(bystander,))
            assert np.array_equal(big, alone), f"bystander {bystander}: its rows change with the splits launched"
            _assert_bits_of_the_single_handle_launch(f"bystander {bystander}", [hs[bystander]], [members[bystander]], n, pick(q, (bystander,)), alone, 0)
            hs[bystander].n_tokens = members[bystander].pos0
            print(f"BATTN selection of {len(sel)} in 16: worst error / bound {r:.3f}, {128 - live} other rows NaN, bystander {bystander} not needed")
        tokens1 = bat.step(step_rows)
        logits1 = [h._scores[-1].copy() for h in hs]
    finally:
        bat.close()
    for h in hs:
        h._planted = None
    assert tokens1 == tokens0
    for k in range(16):
        assert np.array_equal(logits1[k], logits0[k]), f"member {k}: the step behind the taps differs from the step of a batch that was never tapped"


# ------------------------------------------------------------------ i. refusals
def test_refusals_touch_nothing():
    from realtime_codec_agent_amd._native import RcaError
    geom, kvf, n = "g4", "f16", 2
    fam = _family(geom, kvf)
    members = ar.batch_class_members("moderate", 0.0)
    hs, q, kv = _stage(fam, geom, n, members)
    W = q.shape[1]
    pos = [mb.pos0 for mb in members]
    need = max(ar.splits_needed(p, n) for p in pos)
    assert need == 4 and max(-(-mb.n_ctx // 256) for mb in members) == 33
    bat = _batch(hs)
    try:
        base = bat.attn_tap(LAYER, q, n, out_rows=128)
        assert np.isfinite(base[:10]).all() and np.isnan(base[10:]).all()
        tap = lambda **kw: bat.attn_tap(**{**dict(layer=LAYER, q=q, n=n, nsp_launch=0, sel=None, out_rows=None), **kw})
        for what, call in (
            (r"batch_attn_tap: layer 2 outside \[0, 2\)", lambda: tap(layer=2)),
            (r"batch_attn_tap: layer -1 outside", lambda: tap(layer=-1)),
            (r"batch_attn_tap: 3 tokens per member \(1\.\.2\)", lambda: tap(n=3, q=np.zeros((15, W), np.float32))),
            (r"batch_attn_tap: 0 tokens per member", lambda: tap(n=0, q=np.zeros((0, W), np.float32))),
            (r"batch_attn_tap: nsp_launch 3 outside \[4 needed, 33 splits of the batch\]", lambda: tap(nsp_launch=3)),
            (r"batch_attn_tap: nsp_launch 34 outside", lambda: tap(nsp_launch=34)),
            (r"batch_attn_tap: nsp_launch -1 outside", lambda: tap(nsp_launch=-1)),
            (r"batch_attn_tap: out_rows 9 outside \[10 rows of the pass, 128\]", lambda: tap(out_rows=9)),
            (r"batch_attn_tap: out_rows 129 outside", lambda: tap(out_rows=129)),
            (r"batch_attn_tap: 0 selected members", lambda: tap(sel=(), q=np.zeros((0, W), np.float32))),
            (r"batch_attn_tap: 6 selected members, the batch has 5", lambda: tap(sel=(0, 1, 2, 3, 4, 0), q=np.zeros((12, W), np.float32))),
            (r"batch_attn_tap: sel\[1\] = member 5 is outside the batch's members", lambda: tap(sel=(0, 5), q=q[:4])),
            (r"batch_attn_tap: sel\[2\] = member 1 is selected twice", lambda: tap(sel=(1, 0, 1), q=q[:6])),
            (r"batch_attn_tap: out_rows 3 outside \[4 rows of the pass", lambda: tap(sel=(1, 0), q=q[:4], out_rows=3)),
        ):
            with pytest.raises(RcaError, match=what):
                call()
            assert [h.n_tokens for h in hs] == pos, what
        hs[2].n_tokens = 699                                      # n_ctx 700: positions 699 .. 700
        with pytest.raises(RcaError, match=r"rc=-3\): batch_attn_tap: context overflow of member 2: 699 \+ 2 > n_ctx 700"):
            tap()
        with pytest.raises(RcaError, match=r"batch_attn_tap: context overflow of sel\[0\] = member 2"):
            tap(sel=(2,), q=q[:2])
        assert hs[2].n_tokens == 699
        hs[2].n_tokens = pos[2]
        again = bat.attn_tap(LAYER, q, n, out_rows=128)
        assert np.array_equal(again, base, equal_nan=True), "a refused call changed what the next tap gives"
        kr, vr = hs[0].kv_read(LAYER, 0, pos[0] + n)
        assert np.array_equal(kr.view(np.uint16), kv[0][0].view(np.uint16)) and np.array_equal(vr.view(np.uint16), kv[0][1].view(np.uint16))
    finally:
        bat.close()


def test_report_of_worst_ratios():
    """what the tests above measured (run with them): the worst error / bound ratio per G, cache format and class"""
    for (geom, kvf) in sorted({k[:2] for k in WORST}):
        print(f"BATTN worst error / bound, {geom} {kvf}: " + ", ".join(f"{k[2]} {v:.3f}" for k, v in sorted(WORST.items()) if k[:2] == (geom, kvf)))
    assert all(v <= 1.0 for v in WORST.values())
