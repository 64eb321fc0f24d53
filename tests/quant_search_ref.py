"""The search quantisers of realtime_codec_agent_amd.quantize restated in numpy (TEST INFRASTRUCTURE ONLY), beside oracle/q4k_ref.py
and tests/q5k_ref.py, whose block layouts, packers and de-quantisers are used as they are.

What is restated are ggml's published reference quantisers -- make_qkx2_quants (Q4_K / Q5_K sub-blocks of 32 with a minimum),
make_qx_quants (Q6_K groups of 16, symmetric) and quantize_row_q{4,5,6}_K_ref around them -- as DESIGN.md "Quantising on the card"
states them.  ggml is not part of this tree: parity with llama-quantize's own bits is not pinned; THIS file is what the device
kernels (lm_quant_*_kernel, rca_quantize_rows with rule = 1) are compared with byte for byte.

Every operation is one float32 operation, no fused multiply-add; every sum runs over its 32 (or 16) values in index order from 0.0.
nearest() is round-to-nearest-even (np.rint / rintf).  Choices the rules leave open, decided here:
  * every candidate of the Q4_K / Q5_K search uses the sub-block's ORIGINAL min and max (ggml re-uses the min of the last accepted
    candidate: a sequential dependency between candidates that a device mapping over candidates could not keep);
  * min starts at +0.0 and only a value strictly below replaces it, max is the first value that nothing exceeds, the_min = 0.0 - m:
    no -0.0 reaches a stored fp16;
  * a sub-block whose max - min is not finite in f32 is refused like a non-finite d;
  * sc_j / m_j are clamped to 0..63 from both sides;
  * a level whose divisor d * sc is 0 is stored as 0 (Q6_K: as 32, the value 0); an all-zero Q6_K block is 210 zero bytes.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from oracle import q4k_ref  # noqa: E402
import q5k_ref  # noqa: E402

f32 = np.float32
Q8_0, Q4_K, Q5_K, Q6_K = "q8_0", "q4_k", "q5_k", "q6_k"
BLOCK = {Q8_0: (32, 34), Q4_K: (256, 144), Q5_K: (256, 176), Q6_K: (256, 210)}       # values, bytes
GGML_TYPE = {"f32": 0, "f16": 1, Q8_0: 8, Q4_K: 12, Q5_K: 13, Q6_K: 14}
QK_PARAMS = {15: (f32(-1.0), f32(0.1), 20), 31: (f32(-0.5), f32(0.1), 15)}            # nmax -> rmin, rdelta, nstep
GROUP_MAX_EPS = f32(1e-15)


class QuantError(ValueError):
    pass


def _seq_sum(a):
    """sum over the last axis in index order, float32, starting from 0.0"""
    acc = np.zeros(a.shape[:-1], f32)
    for l in range(a.shape[-1]):
        acc = acc + a[..., l]
    return acc


def _levels(x, mn, iscale, nmax):
    return np.clip(np.rint(iscale[:, None] * (x - mn[:, None])), f32(0), f32(nmax)).astype(f32)


def _werr(x, w, L, s, m):
    d = (s[:, None] * L + m[:, None]) - x
    return _seq_sum(w * (d * d))


def search_min(x, nmax):
    """make_qkx2_quants over sub-blocks x float32 [n, 32] -> dict(scale, the_min [n]; start_err, best_err [n]: the weighted error of the
    starting candidate and of the chosen one; w [n, 32])."""
    rmin, rdelta, nstep = QK_PARAMS[nmax]
    x = np.ascontiguousarray(x, f32)
    n = x.shape[0]
    with np.errstate(all="ignore"):
        av = np.sqrt(_seq_sum(x * x) / f32(32.0))
        w = (av[:, None] + np.abs(x)).astype(f32)
        xmin = x.min(axis=1)
        mn = np.where(xmin < 0, xmin, f32(0.0)).astype(f32)
        mx = x.max(axis=1)
        sum_w, sum_x = _seq_sum(w), _seq_sum(w * x)
        flat = mx == mn
        rng = (mx - mn).astype(f32)
        bad = ~np.isfinite(rng)
        rs = np.where(flat | bad, f32(1.0), rng)                       # a harmless divisor where the search does not run
        iscale = f32(nmax) / rs
        scale = f32(1.0) / iscale
        L = _levels(x, mn, iscale, nmax)
        best = _werr(x, w, L, scale, mn)
        start = best.copy()
        bs, bm = scale.copy(), mn.copy()
        for step in range(nstep + 1):
            isc = ((rmin + rdelta * f32(step)) + f32(nmax)) / rs
            La = _levels(x, mn, isc, nmax)
            wl = w * La
            sl, sl2, sxl = _seq_sum(wl), _seq_sum(wl * La), _seq_sum(wl * x)
            D = sum_w * sl2 - sl * sl
            ok = D > 0
            Ds = np.where(ok, D, f32(1.0))
            s = (sum_w * sxl - sum_x * sl) / Ds
            m = (sl2 * sum_x - sl * sxl) / Ds
            pos = m > 0
            s = np.where(pos, sxl / np.where(sl2 != 0, sl2, f32(1.0)), s).astype(f32)
            m = np.where(pos, f32(0.0), m).astype(f32)
            err = _werr(x, w, La, s, m)
            take = ok & (err < best)
            best = np.where(take, err, best)
            bs = np.where(take, s, bs)
            bm = np.where(take, m, bm)
        scale = np.where(flat, f32(0.0), bs).astype(f32)
        the_min = (f32(0.0) - np.where(flat, mn, bm)).astype(f32)
    return dict(scale=scale, the_min=the_min, start_err=np.where(flat, f32(0), start), best_err=np.where(flat, f32(0), best), w=w, bad=bad,
                flat=flat)


def _check_finite(w, name):
    fin = np.isfinite(w)
    if not fin.all():
        row = int(np.argwhere(~fin.reshape(w.shape[0], -1).all(axis=1))[0, 0])
        raise QuantError(f"{name}: row {row} holds a value that is not finite")


def quantize_qk(w, nmax, name="tensor"):
    """float32 [rows, K] -> the dict of q4k_ref.quantize_q4_k / q5k_ref.quantize_q5_k by the search rule (nmax 15 / 31)."""
    w = np.ascontiguousarray(w, f32)
    rows, K = w.shape
    assert K % 256 == 0
    _check_finite(w, name)
    x = w.reshape(-1, 32)
    r = search_min(x, nmax)
    scale, tmin = r["scale"].reshape(-1, 8), r["the_min"].reshape(-1, 8)
    with np.errstate(all="ignore"):
        max_scale = np.maximum(scale.max(axis=1), f32(0.0))
        max_min = np.maximum(tmin.max(axis=1), f32(0.0))
        inv_s = np.where(max_scale > 0, f32(63.0) / np.where(max_scale > 0, max_scale, f32(1)), f32(0)).astype(f32)
        inv_m = np.where(max_min > 0, f32(63.0) / np.where(max_min > 0, max_min, f32(1)), f32(0)).astype(f32)
        sc = np.clip(np.rint(inv_s[:, None] * scale), 0, 63).astype(f32)
        m = np.clip(np.rint(inv_m[:, None] * tmin), 0, 63).astype(f32)
        d = (max_scale / f32(63.0)).astype(np.float16)
        dmin = (max_min / f32(63.0)).astype(np.float16)
        badblk = ~np.isfinite(d.astype(f32)) | ~np.isfinite(dmin.astype(f32)) | r["bad"].reshape(-1, 8).any(axis=1)
        if badblk.any():
            row = int(np.argwhere(badblk)[0, 0]) // (K // 256)
            raise QuantError(f"{name}: row {row}: a block's d or dmin is not finite in fp16")
        d1 = (d.astype(f32)[:, None] * sc).astype(f32).reshape(-1, 1)
        m1 = (dmin.astype(f32)[:, None] * m).astype(f32).reshape(-1, 1)
        q = np.where(d1 != 0, np.rint((x + m1) / np.where(d1 != 0, d1, f32(1))), f32(0))
    q = np.clip(q, 0, nmax).astype(np.uint8)
    return dict(q=q.reshape(rows, K), sc=sc.astype(np.uint8).reshape(rows, K // 32), m=m.astype(np.uint8).reshape(rows, K // 32),
                d=d.reshape(rows, K // 256), dmin=dmin.reshape(rows, K // 256), search=r)


def search_sym(x, nmax=32):
    """make_qx_quants (rmse_type 1, no importance weights) over groups x float32 [n, 16] -> scale float32 [n]"""
    x = np.ascontiguousarray(x, f32)
    n = x.shape[0]
    with np.errstate(all="ignore"):
        ax = np.abs(x)
        idx = ax.argmax(axis=1)                                       # the first on ties
        mx = x[np.arange(n), idx]
        zero = ax[np.arange(n), idx] < GROUP_MAX_EPS
        ms = np.where(zero, f32(1.0), mx)
        w = x * x

        def sums(iscale):
            l = np.clip(np.rint(iscale[:, None] * x), f32(-nmax), f32(nmax - 1)).astype(f32)
            return _seq_sum((w * x) * l), _seq_sum((w * l) * l)

        slx, sl2 = sums(f32(-nmax) / ms)
        scale = np.where(sl2 != 0, slx / np.where(sl2 != 0, sl2, f32(1)), f32(0)).astype(f32)
        best = scale * slx
        for step in range(-9, 10):
            if step == 0:
                continue
            slx, sl2 = sums(-(f32(nmax) + f32(0.1) * f32(step)) / ms)
            take = (sl2 > 0) & (slx * slx > best * sl2)
            ns = (slx / np.where(sl2 > 0, sl2, f32(1))).astype(f32)
            scale = np.where(take, ns, scale)
            best = np.where(take, ns * slx, best)
    return np.where(zero, f32(0.0), scale).astype(f32)


def quantize_q6k(w, name="tensor"):
    """float32 [rows, K] -> the dict of q4k_ref.quantize_q6_k by the search rule, and `zero` bool [blocks]: blocks stored as 210 zero bytes"""
    w = np.ascontiguousarray(w, f32)
    rows, K = w.shape
    assert K % 256 == 0
    _check_finite(w, name)
    x = w.reshape(-1, 16)
    scale = search_sym(x).reshape(-1, 16)
    nb = scale.shape[0]
    with np.errstate(all="ignore"):
        idx = np.abs(scale).argmax(axis=1)
        max_scale = scale[np.arange(nb), idx]
        zero = np.abs(max_scale) < GROUP_MAX_EPS
        iscale = f32(-128.0) / np.where(zero, f32(1.0), max_scale)
        d = (f32(1.0) / iscale).astype(np.float16)
        if (~np.isfinite(d.astype(f32)) | ~np.isfinite(scale).all(axis=1)).any():
            row = int(np.argwhere(~np.isfinite(d.astype(f32)) | ~np.isfinite(scale).all(axis=1))[0, 0]) // (K // 256)
            raise QuantError(f"{name}: row {row}: a block's d is not finite in fp16")
        sc = np.clip(np.rint(iscale[:, None] * scale), -128, 127).astype(f32)
        step = (d.astype(f32)[:, None] * sc).astype(f32).reshape(-1, 1)
        q = np.where(step != 0, np.rint(x / np.where(step != 0, step, f32(1))), f32(0))
    q = np.clip(q, -32, 31).astype(np.int8).reshape(nb, 256)
    sc = sc.astype(np.int8)
    q[zero], sc[zero], d[zero] = -32, 0, 0
    return dict(q=q.reshape(rows, K), sc=sc.reshape(rows, K // 16), d=d.reshape(rows, K // 256), zero=zero)


def _roundf(v):
    """C roundf: to nearest, ties away from zero"""
    t = np.trunc(v)
    return np.where(np.abs(v - t) >= f32(0.5), t + np.sign(v).astype(f32), t).astype(f32)


def quantize_q8_0_blocks(w, name="tensor"):
    """lm_q8_quantize_kernel's rule written out as blocks: d = amax / 127, id = 1 / d, q = roundf(x id), d stored as fp16"""
    w = np.ascontiguousarray(w, f32)
    _check_finite(w, name)
    x = w.reshape(-1, 32)
    with np.errstate(all="ignore"):
        d = (np.abs(x).max(axis=1) / f32(127.0)).astype(f32)
        idd = np.where(d != 0, f32(1.0) / np.where(d != 0, d, f32(1)), f32(0)).astype(f32)
        q = _roundf(x * idd[:, None]).astype(np.int8)
        dh = d.astype(np.float16)
    if not np.isfinite(dh.astype(f32)).all():
        row = int(np.argwhere(~np.isfinite(dh.astype(f32)))[0, 0]) // (w.shape[1] // 32)
        raise QuantError(f"{name}: row {row}: a block's d is not finite in fp16")
    out = np.empty((x.shape[0], 34), np.uint8)
    out[:, :2] = dh.reshape(-1, 1).view(np.uint8)
    out[:, 2:] = q.view(np.uint8)
    return out


def quantize_blocks(w, qtype, name="tensor"):
    """float32 [rows, K] -> raw GGUF blocks uint8 [rows, K / values * bytes] by the search rule (Q8_0: its one rule)"""
    w = np.ascontiguousarray(w, f32)
    rows = w.shape[0]
    if qtype == Q8_0:
        raw = quantize_q8_0_blocks(w, name)
    elif qtype == Q4_K:
        raw = q4k_ref.pack_blocks(quantize_qk(w, 15, name))
    elif qtype == Q5_K:
        raw = q5k_ref.pack_blocks(quantize_qk(w, 31, name))
    elif qtype == Q6_K:
        raw = q4k_ref.pack_blocks_q6_k(quantize_q6k(w, name))
    else:
        raise ValueError(qtype)
    return np.ascontiguousarray(raw.reshape(rows, -1))


def minmax_blocks(w, qtype):
    """the same matrix by this build's min / max rules (oracle/q4k_ref.py, tests/q5k_ref.py): rca_quantize_rows' rule 0"""
    w = np.ascontiguousarray(w, f32)
    if qtype == Q4_K:
        raw = q4k_ref.pack_blocks(q4k_ref.quantize_q4_k(w))
    elif qtype == Q5_K:
        raw = q5k_ref.pack_blocks(q5k_ref.quantize_q5_k(w))
    elif qtype == Q6_K:
        raw = q4k_ref.pack_blocks_q6_k(q4k_ref.quantize_q6_k(w))
    else:
        return quantize_blocks(w, qtype)
    return np.ascontiguousarray(raw.reshape(w.shape[0], -1))


def dequantize(raw, qtype):
    """raw blocks -> float32 values, flat"""
    raw = np.ascontiguousarray(raw)
    if qtype == Q4_K:
        return q4k_ref.dequantize_blocks(raw)
    if qtype == Q5_K:
        return q5k_ref.dequantize_blocks(raw)
    if qtype == Q6_K:
        return q4k_ref.dequantize_blocks_q6_k(raw)
    blk = raw.reshape(-1, 34)
    return (blk[:, 2:].view(np.int8).astype(f32) * blk[:, :2].copy().view(np.float16).astype(f32)).reshape(-1)


# ------------------------------------------------------------------------------------------------------------------ recipes
def use_more_bits(i, n):
    return i < n // 8 or i >= 7 * n // 8 or (i - n // 8) % 3 == 2


def recipe_type(gguf_name, n_layers, recipe):
    """the type a 2-D tensor gets under a recipe: 'q8_0' / 'q4_k' / 'q5_k' / 'q6_k' (one type) or 'q4_k_m' / 'q5_k_m' (the mixes)"""
    if recipe in (Q8_0, Q4_K, Q5_K, Q6_K):
        return recipe
    base = {"q4_k_m": Q4_K, "q5_k_m": Q5_K}[recipe]
    if gguf_name == "output.weight":
        return Q6_K
    if ".attn_v." in gguf_name or ".ffn_down." in gguf_name:
        return Q6_K if use_more_bits(int(gguf_name.split(".")[1]), n_layers) else base
    return base


EDGE_BLOCKS = ("zero", "const_pos", "const_neg", "outlier", "all_pos", "f16_denormal", "amax_65504")


def edge_block(kind):
    """one row of 256 float32 values per case of the issue's list (every value exact in fp16 and, but for the denormals, in bf16-free
    f32: the GPU test feeds them as f32 and fp16)"""
    r = np.random.RandomState(7)
    if kind == "zero":
        return np.zeros(256, f32)
    if kind == "const_pos":
        return np.full(256, 0.375, f32)
    if kind == "const_neg":
        return np.full(256, -0.375, f32)
    if kind == "outlier":
        x = (np.float16(1e-3) * r.choice([-1, 1], 256)).astype(f32)
        x[77] = 1e4
        return x
    if kind == "all_pos":
        return np.abs(r.randn(256)).astype(np.float16).astype(f32) + f32(0.25)
    if kind == "f16_denormal":
        return (r.randint(-1023, 1024, 256).astype(f32) * f32(2.0 ** -24)).astype(f32)
    if kind == "amax_65504":
        x = (r.randn(256) * 100).astype(np.float16).astype(f32)
        x[5] = 65504.0
        x[200] = -65504.0
        return x
    raise ValueError(kind)
