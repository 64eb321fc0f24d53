"""The importance-matrix collector on the device: the wiring of every collection launch against the kernel's definition bit for bit
(rca_lm_imatrix_chunk_tap + tests/imatrix_ref.py), passes against one another, the sums against the float64 restatement
(tests/imatrix_collect_ref.py), what the collector leaves alone, its refusals, and the chain collect -> file -> quantise -> file -> load."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import imatrix_collect_ref as CR  # noqa: E402
import imatrix_ref as IR  # noqa: E402
import quant_weighted_ref as W  # noqa: E402
from oracle import lm_ref  # noqa: E402

pytestmark = pytest.mark.gpu

N_ALL = sum(CR.PARTS)      # 1194


def _new(**kw):
    from realtime_codec_agent_amd.llm import LlamaForAlternatingCodeChannels
    return LlamaForAlternatingCodeChannels(model_path="random:imatrix", config=CR.config(), n_ctx=CR.N_CTX, random_seed=CR.SEED, init_std=CR.INIT_STD,
                                           device=0, weight_format="bf16", **kw)


@functools.lru_cache(maxsize=None)
def _llm():
    return _new()


@functools.lru_cache(maxsize=None)
def _twin():
    """a second handle over the same device weights: its own cache, stream and accumulators"""
    return _new(share_weights_with=_llm())


def _fresh(h):
    """an empty context and zeroed accumulators"""
    h.imatrix_end()
    h.reset()
    h.imatrix_begin()
    return h


def _vectors(h):
    """({(layer, kind): sums}, the one count every vector reports)"""
    got = {p: h.imatrix_get(*p) for p in CR.PAIRS}
    counts = {c for _, c in got.values()}
    assert len(counts) == 1, counts
    return {p: s for p, (s, _) in got.items()}, counts.pop()


def _same(a, b):
    return all(np.array_equal(a[p], b[p]) for p in CR.PAIRS)


# ------------------------------------------------------------------------------------------------------------------ 1. wiring
WIRING = [(l, k, 129, 0) for l, k in CR.PAIRS] + [(l, k, n, 0) for l, k in ((1, 3), (0, 4)) for n in (1, 128, 1024)] + \
         [(l, k, 129, 165) for l, k in ((1, 3), (0, 4))]


@pytest.mark.parametrize("layer,kind,n,n0", WIRING)
def test_every_collection_launch_is_the_definition_bit_for_bit(layer, kind, n, n0):
    """The planes copied right behind the collection launch of (layer, kind), run through the definition with m = n into the
    accumulator as it stood before the call, give the accumulator after it: wrong planes, a wrong m or stride, a wrong slot or a read
    of a dead row (the buffers hold 300 stale rows of an earlier eval) all break the equality."""
    h = _llm()
    h.imatrix_end()
    h.reset()
    h.eval(CR.ids()[:300].tolist())
    _fresh(h)
    if n0:
        h.imatrix_chunk(CR.ids()[:n0])
    before, c0 = _vectors(h)
    assert c0 == n0 and h.n_tokens == n0
    xh, xl = h.imatrix_chunk_tap(CR.ids()[n0:n0 + n], layer, kind)
    after, c1 = _vectors(h)
    K = CR.width(h.config, kind)
    assert xh.shape == xl.shape == (n, K) and xh.any() and xl.any()
    want = IR.collect(xh, xl, n, before[(layer, kind)])
    assert np.array_equal(after[(layer, kind)], want), int(np.argmax(after[(layer, kind)] != want))
    assert c1 == n0 + n and h.n_tokens == n0 + n
    for p in CR.PAIRS:
        assert np.isfinite(after[p]).all() and (after[p] > before[p]).all(), p


# ------------------------------------------------------------------------------------------------------------------ 2. two passes
def test_a_chunk_of_two_passes_is_its_passes_one_by_one():
    a, b = _fresh(_llm()), _fresh(_twin())
    ids = CR.ids()[:1029]
    a.imatrix_chunk(ids)
    b.imatrix_chunk_tap(ids[:1024], 0, 0)
    b.imatrix_chunk_tap(ids[1024:], 1, 3)
    (va, ca), (vb, cb) = _vectors(a), _vectors(b)
    assert ca == cb == 1029 and a.n_tokens == b.n_tokens == 1029
    assert _same(va, vb)
    for l in range(CR.N_LAYERS):
        for x, y in zip(a.kv_read(l, 0, 1029), b.kv_read(l, 0, 1029)):
            assert np.array_equal(x.view(np.uint16), y.view(np.uint16)), l
    assert np.array_equal(a._fetch_logits(), b._fetch_logits())


# ------------------------------------------------------------------------------------------------------------------ 3 .. 5: one collection of the 165 + 1029 ids
def _collect_parts(h):
    """(vectors, count) after chunk(165) and chunk(1029) appended on an empty context; h is left as those calls left it"""
    _fresh(h)
    off = 0
    for n in CR.PARTS:
        h.imatrix_chunk(CR.ids()[off:off + n])
        off += n
    return _vectors(h)


def test_sums_against_the_float64_restatement():
    """Every vector within d_min / 10 (relative L2) of the restatement's float64 sums, d_min being the smallest distance between two
    of the restatement's vectors of equal width: a tenth of what a swapped slot would show at the least."""
    ref = CR.restatement()
    d_min, where = CR.d_min(ref.sums)
    assert d_min > 0.05, (d_min, where)
    got, count = _collect_parts(_llm())
    assert count == ref.count == N_ALL
    worst = {}
    for p in CR.PAIRS:
        worst[p[1]] = max(worst.get(p[1], 0.0), CR.rel_l2(got[p], ref.sums[p]))
    print(f"d_min = {d_min:.4f}; relative L2 distance to the float64 sums per kind: " + ", ".join(f"{k}: {v:.3g}" for k, v in sorted(worst.items())))
    for p in CR.PAIRS:
        assert CR.rel_l2(got[p], ref.sums[p]) <= d_min / 10, (p, CR.rel_l2(got[p], ref.sums[p]), d_min)


def test_the_collector_leaves_the_context_as_score_does_and_nothing_else_collects():
    got, count = _collect_parts(_llm())
    h, t = _llm(), _twin()
    t.imatrix_end()
    t.reset()
    off = 0
    for n in CR.PARTS:
        r = t.score(CR.ids()[off:off + n].tolist())
        off += n
    assert np.isfinite(r.logprob[:-1]).all()
    assert h.n_tokens == t.n_tokens == N_ALL
    for l in range(CR.N_LAYERS):
        for x, y in zip(h.kv_read(l, 0, N_ALL), t.kv_read(l, 0, N_ALL)):
            assert np.array_equal(x.view(np.uint16), y.view(np.uint16)), l
    assert np.array_equal(h._fetch_logits(), t._fetch_logits()) and np.isfinite(h._fetch_logits()).all()
    # every other call on the collecting handle, long and short, on the tiles and off them
    ids = CR.ids()
    h.reset()
    h.eval(ids[:300].tolist())
    h.eval_async(ids[300:600].tolist())
    h.sync()
    h.eval(ids[600:603].tolist())
    h.init_sampler_for_generate()
    h.step(ids[603:605].tolist())
    h.score(ids[605:905].tolist())
    again, count2 = _vectors(h)
    assert count2 == count == N_ALL and _same(got, again)
    imx = h.imatrix_read()
    assert len(imx) == 7 * CR.N_LAYERS + 1 and all(c == N_ALL for _, c in imx.values())
    assert np.array_equal(imx["blk.1.ffn_up.weight"][0], got[(1, 2)]) and np.array_equal(imx["output.weight"][0], got[(0, 4)])


def test_two_collections_of_one_corpus_are_bit_equal():
    got, count = _collect_parts(_llm())
    again, count2 = _collect_parts(_twin())
    assert count == count2 == N_ALL and _same(got, again)


# ------------------------------------------------------------------------------------------------------------------ 6. merge
def test_one_collection_over_a_then_b_against_the_merge_of_two():
    """A (165 tokens, 2 token blocks) and B (1029 tokens: 9), each from an empty context.  One collection folds the 11 partial sums of
    a column into one double in order; the merge adds two folds.  All terms are positive, every f64 add rounds by at most 2^-53
    relative, so either side is within 10 * 2^-53 of the exact sum: the two differ by less than 11 * 2^-52 relative."""
    from realtime_codec_agent_amd import imatrix as I
    h = _llm()
    a_ids, b_ids = CR.ids()[:CR.PARTS[0]], CR.ids()[CR.PARTS[0]:]
    parts = []
    for pieces in ((a_ids,), (b_ids,), (a_ids, b_ids)):
        _fresh(h)
        for i, ids in enumerate(pieces):
            if i:
                h.reset()
            h.imatrix_chunk(ids)
        parts.append(h.imatrix_read())
    merged, both = I.merge(parts[0], parts[1]), parts[2]
    blocks = sum(-(-n // 128) for n in CR.PARTS)
    assert blocks == 11 and set(merged) == set(both) and len(both) == 15
    for name in both:
        (sm, cm), (sb, cb) = merged[name], both[name]
        assert cm == cb == N_ALL, name
        assert (np.abs(sm - sb) <= blocks * 2.0 ** -52 * sb).all(), (name, float(np.max(np.abs(sm - sb) / sb)))
    assert not np.array_equal(parts[0]["output.weight"][0], parts[1]["output.weight"][0])


# ------------------------------------------------------------------------------------------------------------------ 7. refusals
def test_refusals():
    from realtime_codec_agent_amd._native import RcaError
    h = _llm()
    h.imatrix_end()
    h.imatrix_end()                                  # ending twice is harmless
    h.reset()
    ids = CR.ids()
    with pytest.raises(RcaError, match="not collecting"):
        h.imatrix_chunk(ids[:16])
    with pytest.raises(RcaError, match="not collecting"):
        h.imatrix_get(0, 0)
    assert h.n_tokens == 0
    h.set_mfma_prefill(False)
    try:
        with pytest.raises(RcaError, match="do not take the 128-token tiles"):
            h.imatrix_begin()
    finally:
        h.set_mfma_prefill(True)
    h.imatrix_begin()
    with pytest.raises(RcaError, match="already collecting"):
        h.imatrix_begin()
    h.imatrix_chunk(ids[:200])
    before, c0 = _vectors(h)
    assert c0 == 200
    with pytest.raises(RcaError, match=r"context overflow: 200 \+ 1081 > n_ctx 1280"):
        h.imatrix_chunk(ids[:1081])
    bad = ids[:40].copy()
    bad[17] = 1000
    with pytest.raises(RcaError, match=r"token id 1000 at index 17 is outside the vocabulary"):
        h.imatrix_chunk(bad)
    bad[17] = -1
    with pytest.raises(RcaError, match=r"token id -1 at index 17"):
        h.imatrix_chunk_tap(bad, 0, 0)
    with pytest.raises(RcaError, match=r"more than one pass"):
        h.imatrix_chunk_tap(np.zeros(1025, np.int32), 0, 0)
    after, c1 = _vectors(h)
    assert c1 == 200 and h.n_tokens == 200 and _same(before, after)
    for layer, kind, width, msg in ((2, 0, 256, "no layer 2 / kind 0"), (-1, 3, 512, "no layer -1 / kind 3"), (0, 5, 256, "no layer 0 / kind 5"),
                                    (0, -1, 256, "no layer 0 / kind -1"), (0, 3, 256, "kind 3 has a width of 512"), (1, 0, 512, "kind 0 has a width of 256"),
                                    (0, 4, 1000, "kind 4 has a width of 256")):
        with pytest.raises(RcaError, match=msg):
            h.imatrix_get(layer, kind, width)
    assert h.imatrix_get(7, 4)[1] == 200             # the layer is ignored for the head's vector
    h.imatrix_end()


# ------------------------------------------------------------------------------------------------------------------ 8. the chain
def test_chain_collect_file_quantise_write_load_score(tmp_path):
    """collect -> imatrix file -> quantize_weights(q4_k_m, imatrix=) -> write_llama_gguf -> load -> score.  (A random model: no quality
    claim.)"""
    from realtime_codec_agent_amd import imatrix as I
    from realtime_codec_agent_amd import quantize as Q
    from realtime_codec_agent_amd.llm import LlamaForAlternatingCodeChannels
    cfg = CR.config()
    h = _llm()
    h.imatrix_end()
    got = I.collect(h, [CR.ids()], chunk=256)
    assert len(got) == 15 and got.chunk_count == 4 and got.chunk_size == 256 and all(c == 1024 for _, c in got.values())
    with pytest.raises(Exception, match="not collecting"):
        h.imatrix_get(0, 0)                          # collect() ended its collection
    got.datasets = ["random ids"]
    ipath = str(tmp_path / "collected.gguf")
    I.write_imatrix_gguf(ipath, got)
    imx = I.read_imatrix_gguf(ipath)
    assert len(imx) == 15 and imx.chunk_count == 4 and imx.chunk_size == 256
    assert np.array_equal(imx["blk.0.ffn_down.weight"][0], got["blk.0.ffn_down.weight"][0].astype(np.float32).astype(np.float64))
    src = lm_ref.random_weights(cfg, CR.SEED, CR.INIT_STD)
    q = Q.quantize_weights(cfg, src, "q4_k_m", imatrix=imx)
    name = "model.layers.0.mlp.down_proj.weight"
    vec = (imx["blk.0.ffn_down.weight"][0] / imx["blk.0.ffn_down.weight"][1]).astype(np.float32)
    assert vec.shape == (cfg.ffn,) and (vec > 0).all()
    assert np.array_equal(q[name].raw, W.quantize_blocks_w(IR.bf16_to_f32(src[name]), q.types[name], vec))
    plain = Q.quantize_weights(cfg, src, "q4_k_m")
    assert not np.array_equal(q[name].raw, plain[name].raw)
    path = str(tmp_path / "q4_k_m.gguf")
    Q.write_llama_gguf(path, cfg, q)
    llm = LlamaForAlternatingCodeChannels(model_path=path, n_ctx=512, device=0)
    try:
        r = llm.score(CR.ids()[:300].tolist())
        assert np.isfinite(r.logprob[:-1]).all() and np.isfinite(llm._fetch_logits()).all()
    finally:
        llm.close()
