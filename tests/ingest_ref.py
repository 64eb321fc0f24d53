"""Float64 restatement of the batch CLI's device ingest (rca_codec_ingest_rows_dev; the definition is in include/rca.h and DESIGN.md)
and the per-sample bound the GPU test holds the kernel to.  Plain helper module: no test lives here.

frames(): the f32 frame values m[k] of a row, exactly as the kernel forms them -- int16 -> v * 2^-15 (exact), f32 as it is, a downmix
as the f32 sum in ascending channel order followed by one IEEE division (numpy's f32 arithmetic is the same arithmetic).
resample64(): y[n] = sum over k of taps[t - k * up] * m[k], t = n * down + half, in float64, the f32 taps and frames taken exactly.

The bound.  The kernel returns an f32 sum of L non-zero products (terms whose tap lies outside the table or whose frame lies outside
the row are exact zeros and add no error).  For any order of the additions, with products rounded on their own or fused into the
addition, the standard result for recursive summation of products is
    |fl(sum) - sum| <= gamma_L * sum |taps * m|,   gamma_L = L u / (1 - L u),  u = 2^-24
(one (1 + delta) per product and at most L - 1 per addition chain; an fma only removes some of them).  gamma_L <= (L + 1) u as long as
L (L + 1) <= 2^24, and L <= 57 here.  On top come u * |y64| (the distance from the f32 result to the float64 one it stands for:
one rounding of the output) and the smallest subnormal, 2^-149, for a result that underflows.  So per output sample
    |y - y64| <= (L + 1) * u * sum |taps * m| + u * |y64| + 2^-149.
"""
import numpy as np

U = 2.0 ** -24
TINY = 2.0 ** -149


def out_len(n_in: int, up: int, down: int) -> int:
    return -(-n_in * up // down)


def frames(src: np.ndarray, src_off: int, n_in: int, src_stride: int, n_mix: int) -> np.ndarray:
    """m[k], k < n_in, of the row (src_off, n_in, src_stride, n_mix) of the flat int16 / float32 array src -> float32 [n_in]."""
    idx = src_off + np.arange(n_in, dtype=np.int64) * src_stride
    cvt = (lambda v: v.astype(np.float32) * np.float32(2.0 ** -15)) if src.dtype == np.int16 else (lambda v: v.astype(np.float32))
    acc = cvt(src[idx])
    if n_mix > 1:
        for c in range(1, n_mix):
            acc = (acc + cvt(src[idx + c])).astype(np.float32)
        acc = (acc / np.float32(n_mix)).astype(np.float32)
    return acc


def resample64(m: np.ndarray, up: int, down: int, taps: np.ndarray):
    """-> (y64 [n_out], bound [n_out]) for the f32 frames m and the f32 taps."""
    n_in, n_taps = len(m), len(taps)
    n_out = out_len(n_in, up, down)
    if up == 1 and down == 1:                               # the pure conversion: exact
        return m.astype(np.float64), np.zeros(n_in)
    half = (n_taps - 1) // 2
    jmax = -(-n_taps // up)
    t = np.arange(n_out, dtype=np.int64) * down + half
    kh, p = t // up, t % up
    j = np.arange(jmax, dtype=np.int64)
    ti = p[:, None] + j[None, :] * up
    k = kh[:, None] - j[None, :]
    valid = (ti < n_taps) & (k >= 0) & (k < n_in)
    m64 = np.concatenate([m.astype(np.float64), [0.0]])     # index n_in: the zero beyond both ends
    prod = np.where(valid, taps.astype(np.float64)[np.minimum(ti, n_taps - 1)] * m64[np.where((k >= 0) & (k < n_in), k, n_in)], 0.0)
    y = prod.sum(axis=1)
    L = valid.sum(axis=1)
    return y, (L + 1) * U * np.abs(prod).sum(axis=1) + U * np.abs(y) + TINY


def ingest_rows_f32(data: np.ndarray, layout: str, mix: bool, up: int, down: int, taps: np.ndarray) -> np.ndarray:
    """A whole file ([N, C] interleaved or [C, N] planar) -> float32 [rows, n_out]: the restatement rounded to f32 (what a CPU
    stand-in for the kernel returns)."""
    flat = np.ascontiguousarray(data).reshape(-1)
    if layout == "interleaved":
        n, ch = data.shape
        rows = [(0, ch, ch)] if mix else [(c, ch, 1) for c in range(ch)]
    else:
        ch, n = data.shape
        assert not (mix and ch > 1)
        rows = [(c * n, 1, 1) for c in range(ch)]
    out = [resample64(frames(flat, off, n, stride, n_mix), up, down, taps)[0].astype(np.float32) for off, stride, n_mix in rows]
    return np.stack(out) if out else np.zeros((0, out_len(n, up, down)), np.float32)
