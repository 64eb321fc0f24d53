"""The weighted quantisers of rca_quantize_rows_w restated in numpy (TEST INFRASTRUCTURE ONLY), beside tests/quant_search_ref.py, whose
sequential sums, layouts and packers are used as they are.

What is restated are ggml's published quantize_row_q{4,5,6}_K_impl with quant_weights (make_qkx3_quants, make_qp_quants and
make_qx_quants under given weights) as DESIGN.md "Weighted K-quant search" states them.  ggml is not part of this tree: parity with
llama-quantize's own bits is not pinned; THIS file is what csrc/rca_quant_rows.h (host build and device kernel) is compared with byte
for byte.

Every operation is one float32 operation, no fused multiply-add; every sum runs in index order from 0.0; nearest() is np.rint.
qw is one float32 weight per COLUMN [K] (an importance matrix's in_sum2 / count): every row uses the same weights.
  * Q4_K / Q5_K: sigma2 = 2 sum(x^2) / 256 over the super-block, w_l = qw_l sqrt(sigma2 + x_l^2); the sub-block search is
    quant_search_ref.search_min with these weights, RMIN -0.9, RDELTA 0.05, NSTEP 36 and flat = max <= min; the eight scales and the
    eight minima are each quantised by qp() under the sub-blocks' sum(w) -- d and dmin are its results, not max / 63;
  * Q6_K: quant_search_ref.search_sym with w_l = qw_l in the place of x_l^2;
  * a group (32 columns, Q6_K: 16) whose weights are all 0 uses 1.0 for them;
  * a level set qp() returns is clamped to 0..63 from both sides when it is stored, like every stored level of the unweighted rules.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import quant_search_ref as R  # noqa: E402
from quant_search_ref import QuantError, _seq_sum, f32  # noqa: E402

RMIN, RDELTA, NSTEP = f32(-0.9), f32(0.05), 36


def check_weights(qw, K):
    qw = np.ascontiguousarray(qw, f32)
    if qw.shape != (K,):
        raise QuantError(f"weights of shape {qw.shape} for K = {K}")
    bad = ~np.isfinite(qw) | (qw < 0)
    if bad.any():
        raise QuantError(f"the weight of column {int(np.argwhere(bad)[0, 0])} is negative or not finite")
    return qw


def _group_weights(qw, rows, group):
    """qw [K] -> [rows * K / group, group], the weights of a group whose weights are all 0 replaced by 1.0"""
    g = np.tile(qw.reshape(1, -1), (rows, 1)).reshape(-1, group)
    return np.where((g == 0).all(axis=1)[:, None], f32(1.0), g).astype(f32)


def search_min_w(x, w, nmax):
    """sub-blocks x, weights w float32 [n, 32] -> dict(scale, the_min, sw [n]; bad [n])"""
    x, w = np.ascontiguousarray(x, f32), np.ascontiguousarray(w, f32)
    with np.errstate(all="ignore"):
        xmin = x.min(axis=1)
        mn = np.where(xmin < 0, xmin, f32(0.0)).astype(f32)
        mx = x.max(axis=1)
        sum_w, sum_x = _seq_sum(w), _seq_sum(w * x)
        flat = mx <= mn
        rng = (mx - mn).astype(f32)
        bad = ~flat & ~np.isfinite(rng)
        rs = np.where(flat | bad, f32(1.0), rng)
        iscale = f32(nmax) / rs
        scale = f32(1.0) / iscale
        best = R._werr(x, w, R._levels(x, mn, iscale, nmax), scale, mn)
        bs, bm = scale.copy(), mn.copy()
        for step in range(NSTEP + 1):
            isc = ((RMIN + RDELTA * f32(step)) + f32(nmax)) / rs
            La = R._levels(x, mn, isc, nmax)
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
            err = R._werr(x, w, La, s, m)
            take = ok & (err < best)
            best = np.where(take, err, best)
            bs = np.where(take, s, bs)
            bm = np.where(take, m, bm)
        scale = np.where(flat, f32(0.0), bs).astype(f32)
        the_min = (f32(0.0) - np.where(flat, mn, bm)).astype(f32)
    return dict(scale=scale, the_min=the_min, sw=sum_w, bad=bad)


def qp(v, sw, nmax=63):
    """make_qp_quants: values v, weights sw float32 [n, 8] -> (step d float32 [n], levels float32 [n, 8]) with v ~ d L"""
    v, sw = np.ascontiguousarray(v, f32), np.ascontiguousarray(sw, f32)
    n, k = v.shape
    nm = f32(nmax)
    with np.errstate(all="ignore"):
        mx = v.max(axis=1)
        pos = mx > 0
        ms = np.where(pos, mx, f32(1.0))

        def levels(isc):
            return np.minimum(nm, np.rint(isc[:, None] * v)).astype(f32)

        def err(isc):
            d = v - (f32(1.0) / isc)[:, None] * levels(isc)
            return _seq_sum(sw * (d * d))

        iscale = nm / ms
        best = err(iscale)
        for step in range(-4, 5):
            if step == 0:
                continue
            cand = (f32(0.1) * f32(step) + nm) / ms
            e = err(cand)
            take = e < best
            best = np.where(take, e, best)
            iscale = np.where(take, cand, iscale).astype(f32)
        L = levels(iscale)
        slx, sl2 = _seq_sum((sw * v) * L), _seq_sum((sw * L) * L)
        active = np.ones(n, bool)
        for _ in range(5):
            moved = np.zeros(n, bool)
            for i in range(k):
                wv = sw[:, i] * v[:, i]
                a = slx - wv * L[:, i]
                b = sl2 - (sw[:, i] * L[:, i]) * L[:, i]
                ok = active & (a > 0) & (b > 0)
                nl = np.clip(np.rint((v[:, i] * b) / np.where(ok, a, f32(1.0))), f32(0), nm).astype(f32)
                a2 = a + wv * nl
                b2 = b + (sw[:, i] * nl) * nl
                acc = ok & (nl != L[:, i]) & ((a2 * a2) * sl2 > (slx * slx) * b2)
                L[:, i] = np.where(acc, nl, L[:, i])
                slx = np.where(acc, a2, slx).astype(f32)
                sl2 = np.where(acc, b2, sl2).astype(f32)
                moved |= acc
            active &= moved
        d = np.where(sl2 > 0, slx / np.where(sl2 > 0, sl2, f32(1.0)), f32(0.0)).astype(f32)
    return np.where(pos, d, f32(0.0)).astype(f32), np.where(pos[:, None], L, f32(0.0)).astype(f32)


def quantize_qk_w(w, qw, nmax, name="tensor"):
    """float32 [rows, K], column weights [K] -> the dict of q4k_ref.quantize_q4_k / q5k_ref.quantize_q5_k by the weighted rule"""
    w = np.ascontiguousarray(w, f32)
    rows, K = w.shape
    assert K % 256 == 0
    qw = check_weights(qw, K)
    R._check_finite(w, name)
    with np.errstate(all="ignore"):
        xb = w.reshape(-1, 256)
        sigma2 = ((f32(2.0) * _seq_sum(xb * xb)) / f32(256.0)).astype(f32)
        x = w.reshape(-1, 32)
        wt = (_group_weights(qw, rows, 32) * np.sqrt(np.repeat(sigma2, 8)[:, None] + x * x)).astype(f32)
        r = search_min_w(x, wt, nmax)
        sw = r["sw"].reshape(-1, 8)
        d32, sc = qp(r["scale"].reshape(-1, 8), sw)
        dmin32, m = qp(r["the_min"].reshape(-1, 8), sw)
        d, dmin = d32.astype(np.float16), dmin32.astype(np.float16)
        badblk = ~np.isfinite(d.astype(f32)) | ~np.isfinite(dmin.astype(f32)) | r["bad"].reshape(-1, 8).any(axis=1)
        if badblk.any():
            row = int(np.argwhere(badblk)[0, 0]) // (K // 256)
            raise QuantError(f"{name}: row {row}: a block's d or dmin is not finite in fp16")
        sc, m = np.clip(sc, 0, 63).astype(f32), np.clip(m, 0, 63).astype(f32)
        d1 = (d.astype(f32)[:, None] * sc).astype(f32).reshape(-1, 1)
        m1 = (dmin.astype(f32)[:, None] * m).astype(f32).reshape(-1, 1)
        q = np.where(d1 != 0, np.rint((x + m1) / np.where(d1 != 0, d1, f32(1))), f32(0))
    q = np.clip(q, 0, nmax).astype(np.uint8)
    return dict(q=q.reshape(rows, K), sc=sc.astype(np.uint8).reshape(rows, K // 32), m=m.astype(np.uint8).reshape(rows, K // 32),
                d=d.reshape(rows, K // 256), dmin=dmin.reshape(rows, K // 256))


def search_sym_w(x, qw, nmax=32):
    """make_qx_quants under given weights: groups x, weights qw float32 [n, 16] -> scale float32 [n]"""
    x, w = np.ascontiguousarray(x, f32), np.ascontiguousarray(qw, f32)
    n = x.shape[0]
    with np.errstate(all="ignore"):
        ax = np.abs(x)
        idx = ax.argmax(axis=1)
        mx = x[np.arange(n), idx]
        zero = ax[np.arange(n), idx] < R.GROUP_MAX_EPS
        ms = np.where(zero, f32(1.0), mx)

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


def quantize_q6k_w(w, qw, name="tensor"):
    """float32 [rows, K], column weights [K] -> the dict of quant_search_ref.quantize_q6k by the weighted rule"""
    w = np.ascontiguousarray(w, f32)
    rows, K = w.shape
    assert K % 256 == 0
    qw = check_weights(qw, K)
    R._check_finite(w, name)
    x = w.reshape(-1, 16)
    scale = search_sym_w(x, _group_weights(qw, rows, 16)).reshape(-1, 16)
    nb = scale.shape[0]
    with np.errstate(all="ignore"):
        idx = np.abs(scale).argmax(axis=1)
        max_scale = scale[np.arange(nb), idx]
        zero = np.abs(max_scale) < R.GROUP_MAX_EPS
        iscale = f32(-128.0) / np.where(zero, f32(1.0), max_scale)
        d = (f32(1.0) / iscale).astype(np.float16)
        badblk = ~np.isfinite(d.astype(f32)) | ~np.isfinite(scale).all(axis=1)
        if badblk.any():
            row = int(np.argwhere(badblk)[0, 0]) // (K // 256)
            raise QuantError(f"{name}: row {row}: a block's d is not finite in fp16")
        sc = np.clip(np.rint(iscale[:, None] * scale), -128, 127).astype(f32)
        step = (d.astype(f32)[:, None] * sc).astype(f32).reshape(-1, 1)
        q = np.where(step != 0, np.rint(x / np.where(step != 0, step, f32(1))), f32(0))
    q = np.clip(q, -32, 31).astype(np.int8).reshape(nb, 256)
    sc = sc.astype(np.int8)
    q[zero], sc[zero], d[zero] = -32, 0, 0
    return dict(q=q.reshape(rows, K), sc=sc.reshape(rows, K // 16), d=d.reshape(rows, K // 256), zero=zero)


def quantize_blocks_w(w, qtype, qw, name="tensor"):
    """float32 [rows, K], column weights float32 [K] -> raw GGUF blocks uint8 [rows, ...] by the weighted rule (Q8_0 ignores weights)"""
    w = np.ascontiguousarray(w, f32)
    if qtype == R.Q8_0:
        check_weights(qw, w.shape[1])
        return R.quantize_blocks(w, qtype, name)
    if qtype == R.Q4_K:
        raw = R.q4k_ref.pack_blocks(quantize_qk_w(w, qw, 15, name))
    elif qtype == R.Q5_K:
        raw = R.q5k_ref.pack_blocks(quantize_qk_w(w, qw, 31, name))
    elif qtype == R.Q6_K:
        raw = R.q4k_ref.pack_blocks_q6_k(quantize_q6k_w(w, qw, name))
    else:
        raise ValueError(qtype)
    return np.ascontiguousarray(raw.reshape(w.shape[0], -1))


def weighted_error(raw, qtype, w, qw):
    """sum_j qw_j (x_hat - x)^2 over the whole matrix, float64"""
    d = R.dequantize(raw, qtype).reshape(w.shape).astype(np.float64) - w.astype(np.float64)
    return float((np.asarray(qw, np.float64)[None, :] * d * d).sum())
