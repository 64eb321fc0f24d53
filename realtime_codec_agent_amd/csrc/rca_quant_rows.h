// Row quantisers of rca_quantize_rows (include/rca.h): one super-block of 256 values (Q8_0: one block of 32) -> its raw GGUF block,
// byte for byte in the file layout.  Plain C++ that compiles for the device and for the host alike (a host build of these functions is
// how the arithmetic is checked without a card); the kernels that call them are in rca_lm.hip (lm_quant_*_kernel).
//
// rule 0 = this build's min / max rules (lm_q4k_quantize_kernel operation for operation; for Q6_K oracle/q4k_ref.py::quantize_q6_k),
// rule 1 = the scale searches of ggml's published reference quantisers (make_qkx2_quants, make_qx_quants, quantize_row_q{4,5,6}_K_ref)
// restated: DESIGN.md "Quantising on the card" has the rules, the sum orders and the choices; tests/quant_search_ref.py is the numpy
// restatement the results are compared with byte for byte.  ggml is not part of this tree: parity with llama-quantize's own bits is
// not pinned.  Every operation is one f32 operation (the build runs with -ffp-contract=off), every sum runs in index order from 0.0f.
// With column weights (rca_quantize_rows_w: an importance matrix) rule 1 becomes ggml's published quantize_row_q{4,5,6}_K_impl with
// quant_weights, restated: DESIGN.md "Weighted K-quant search", tests/quant_weighted_ref.py.  Without weights nothing changes.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define RCA_QHD __host__ __device__ __forceinline__
#else
#define RCA_QHD inline
#endif

namespace rca_quant {

enum { QS_OK = 0, QS_BAD_INPUT = 1, QS_BAD_D = 2 };   // status bits of one block

RCA_QHD float ldf(const float* p, long i) { return p[i]; }
#if defined(__HIPCC__)
struct bf16_src { unsigned short b; };
struct f16_src { _Float16 h; };
RCA_QHD float ldf(const bf16_src* p, long i) { return __builtin_bit_cast(float, (unsigned)p[i].b << 16); }
RCA_QHD float ldf(const f16_src* p, long i) { return (float)p[i].h; }
RCA_QHD unsigned short f16_bits(float v) { return __builtin_bit_cast(unsigned short, (_Float16)v); }
RCA_QHD float f16_value(unsigned short b) { return (float)__builtin_bit_cast(_Float16, b); }
#else
RCA_QHD unsigned short f16_bits(float v) { _Float16 h = (_Float16)v; unsigned short b; __builtin_memcpy(&b, &h, 2); return b; }
RCA_QHD float f16_value(unsigned short b) { _Float16 h; __builtin_memcpy(&h, &b, 2); return (float)h; }
#endif
RCA_QHD bool f16_finite(unsigned short b) { return (b & 0x7c00u) != 0x7c00u; }
RCA_QHD bool finite32(float v) { return fabsf(v) <= 3.402823466e+38f; }   // false for NaN too
RCA_QHD float clampf(float v, float lo, float hi) { return fminf(fmaxf(v, lo), hi); }

// ---- a sub-block of 32 values with a minimum: (scale, the_min >= 0) with value ~ scale * L - the_min, L in 0..NMAX
template <int NMAX>
RCA_QHD int sub_minmax(const float* x, float* scale, float* the_min) {
    float mn = 0.0f, mx = -INFINITY;
    for (int l = 0; l < 32; ++l) {
        mn = fminf(mn, x[l]);
        mx = fmaxf(mx, x[l]);
    }
    *scale = (mx - mn) / (float)NMAX;
    *the_min = -mn;
    return QS_OK;
}
template <int NMAX>
RCA_QHD int sub_search(const float* x, float* scale, float* the_min) {
    constexpr float RMIN = NMAX == 15 ? -1.0f : -0.5f, RDELTA = 0.1f;
    constexpr int NSTEP = NMAX == 15 ? 20 : 15;
    float sum_x2 = 0.0f;
    for (int l = 0; l < 32; ++l) sum_x2 = sum_x2 + x[l] * x[l];
    const float av = sqrtf(sum_x2 / 32.0f);
    float w[32];
    float mn = 0.0f, mx = x[0], sum_w = 0.0f, sum_x = 0.0f;
    for (int l = 0; l < 32; ++l) {
        if (x[l] < mn) mn = x[l];
        if (x[l] > mx) mx = x[l];
        w[l] = av + fabsf(x[l]);
        sum_w = sum_w + w[l];
        sum_x = sum_x + w[l] * x[l];
    }
    if (mx == mn) {
        *scale = 0.0f;
        *the_min = 0.0f - mn;
        return QS_OK;
    }
    const float range = mx - mn;
    if (!finite32(range)) {
        *scale = 0.0f;
        *the_min = 0.0f;
        return QS_BAD_D;
    }
    float iscale = (float)NMAX / range;
    float bs = 1.0f / iscale, bm = mn, best = 0.0f;
    for (int l = 0; l < 32; ++l) {
        const float L = clampf(rintf(iscale * (x[l] - mn)), 0.0f, (float)NMAX);
        const float diff = (bs * L + mn) - x[l];
        best = best + w[l] * (diff * diff);
    }
    for (int is = 0; is <= NSTEP; ++is) {
        iscale = ((RMIN + RDELTA * (float)is) + (float)NMAX) / range;
        float La[32];
        float sl = 0.0f, sl2 = 0.0f, sxl = 0.0f;
        for (int l = 0; l < 32; ++l) {
            La[l] = clampf(rintf(iscale * (x[l] - mn)), 0.0f, (float)NMAX);
            const float wl = w[l] * La[l];
            sl = sl + wl;
            sl2 = sl2 + wl * La[l];
            sxl = sxl + wl * x[l];
        }
        const float D = sum_w * sl2 - sl * sl;
        if (D > 0.0f) {
            float s = (sum_w * sxl - sum_x * sl) / D;
            float m = (sl2 * sum_x - sl * sxl) / D;
            if (m > 0.0f) {
                m = 0.0f;
                s = sxl / sl2;
            }
            float err = 0.0f;
            for (int l = 0; l < 32; ++l) {
                const float diff = (s * La[l] + m) - x[l];
                err = err + w[l] * (diff * diff);
            }
            if (err < best) {
                best = err;
                bs = s;
                bm = m;
            }
        }
    }
    *scale = bs;
    *the_min = 0.0f - bm;
    return QS_OK;
}

// ---- the same sub-block under importance weights (rca_quantize_rows_w): the weights w[32] are given, the search is finer
// (RMIN -0.9, RDELTA 0.05, NSTEP 36 for both types) and a sub-block is flat when max <= min; every decision else is sub_search's.
// Returns sum(w) in *sum_w_out: the weight of this sub-block's scale and minimum in quant_scales_w.
template <int NMAX>
RCA_QHD int sub_search_w(const float* x, const float* w, float* scale, float* the_min, float* sum_w_out) {
    constexpr float RMIN = -0.9f, RDELTA = 0.05f;
    constexpr int NSTEP = 36;
    float mn = 0.0f, mx = x[0], sum_w = 0.0f, sum_x = 0.0f;
    for (int l = 0; l < 32; ++l) {
        if (x[l] < mn) mn = x[l];
        if (x[l] > mx) mx = x[l];
        sum_w = sum_w + w[l];
        sum_x = sum_x + w[l] * x[l];
    }
    *sum_w_out = sum_w;
    if (mx <= mn) {
        *scale = 0.0f;
        *the_min = 0.0f - mn;
        return QS_OK;
    }
    const float range = mx - mn;
    if (!finite32(range)) {
        *scale = 0.0f;
        *the_min = 0.0f;
        return QS_BAD_D;
    }
    float iscale = (float)NMAX / range;
    float bs = 1.0f / iscale, bm = mn, best = 0.0f;
    for (int l = 0; l < 32; ++l) {
        const float L = clampf(rintf(iscale * (x[l] - mn)), 0.0f, (float)NMAX);
        const float diff = (bs * L + mn) - x[l];
        best = best + w[l] * (diff * diff);
    }
    for (int is = 0; is <= NSTEP; ++is) {
        iscale = ((RMIN + RDELTA * (float)is) + (float)NMAX) / range;
        float La[32];
        float sl = 0.0f, sl2 = 0.0f, sxl = 0.0f;
        for (int l = 0; l < 32; ++l) {
            La[l] = clampf(rintf(iscale * (x[l] - mn)), 0.0f, (float)NMAX);
            const float wl = w[l] * La[l];
            sl = sl + wl;
            sl2 = sl2 + wl * La[l];
            sxl = sxl + wl * x[l];
        }
        const float D = sum_w * sl2 - sl * sl;
        if (D > 0.0f) {
            float s = (sum_w * sxl - sum_x * sl) / D;
            float m = (sl2 * sum_x - sl * sxl) / D;
            if (m > 0.0f) {
                m = 0.0f;
                s = sxl / sl2;
            }
            float err = 0.0f;
            for (int l = 0; l < 32; ++l) {
                const float diff = (s * La[l] + m) - x[l];
                err = err + w[l] * (diff * diff);
            }
            if (err < best) {
                best = err;
                bs = s;
                bm = m;
            }
        }
    }
    *scale = bs;
    *the_min = 0.0f - bm;
    return QS_OK;
}

// make_qp_quants restated: eight non-negative values v (the sub-blocks' scales, or their minima) with weights sw -> levels L in 0..63
// and the returned step d with v ~ d L, by a search over nine starting steps and up to five sweeps that move one level at a time.
RCA_QHD float quant_scales_w(const float* v, const float* sw, float* L) {
    constexpr float NM = 63.0f;
    float mx = v[0];
    for (int i = 1; i < 8; ++i)
        if (v[i] > mx) mx = v[i];
    if (!(mx > 0.0f)) {
        for (int i = 0; i < 8; ++i) L[i] = 0.0f;
        return 0.0f;
    }
    float iscale = NM / mx, best = 0.0f;
    for (int is = -5; is <= 4; ++is) {   // -5 stands for the starting candidate 63 / max; 0 is skipped
        if (is == 0) continue;
        const float cand = is == -5 ? iscale : (0.1f * (float)is + NM) / mx;
        const float inv = 1.0f / cand;
        float err = 0.0f;
        for (int i = 0; i < 8; ++i) {
            const float diff = v[i] - inv * fminf(NM, rintf(cand * v[i]));
            err = err + sw[i] * (diff * diff);
        }
        if (is == -5 || err < best) {
            best = err;
            iscale = cand;
        }
    }
    float slx = 0.0f, sl2 = 0.0f;
    for (int i = 0; i < 8; ++i) {
        L[i] = fminf(NM, rintf(iscale * v[i]));
        slx = slx + (sw[i] * v[i]) * L[i];
        sl2 = sl2 + (sw[i] * L[i]) * L[i];
    }
    for (int sweep = 0; sweep < 5; ++sweep) {
        bool moved = false;
        for (int i = 0; i < 8; ++i) {
            const float wv = sw[i] * v[i];
            const float a = slx - wv * L[i], b = sl2 - (sw[i] * L[i]) * L[i];
            if (a > 0.0f && b > 0.0f) {
                const float nl = clampf(rintf((v[i] * b) / a), 0.0f, NM);
                if (nl != L[i]) {
                    const float a2 = a + wv * nl, b2 = b + (sw[i] * nl) * nl;
                    if ((a2 * a2) * sl2 > (slx * slx) * b2) {
                        L[i] = nl;
                        slx = a2;
                        sl2 = b2;
                        moved = true;
                    }
                }
            }
        }
        if (!moved) break;
    }
    return sl2 > 0.0f ? slx / sl2 : 0.0f;
}

// The scales of one Q4_K / Q5_K super-block under column weights qw[256]: w_l = qw_l sqrt(sigma2 + x_l^2), sigma2 = 2 sum(x^2) / 256;
// a sub-block whose 32 weights are all 0 takes 1.0 for them.  -> d, dmin (fp16 bits) and the levels sc, mm
template <int NMAX, typename T>
RCA_QHD int block_scales_w(const T* src, const float* qw, unsigned short* dh, unsigned short* dminh, unsigned* sc, unsigned* mm) {
    int status = QS_OK;
    float sum_x2 = 0.0f;
    for (int l = 0; l < 256; ++l) {
        const float v = ldf(src, l);
        sum_x2 = sum_x2 + v * v;
    }
    const float sigma2 = (2.0f * sum_x2) / 256.0f;
    float scale[8], tmin[8], sw[8], Ls[8], Lm[8];
    for (int j = 0; j < 8; ++j) {
        float x[32], w[32];
        bool none = true;
        for (int l = 0; l < 32; ++l) {
            x[l] = ldf(src, 32 * j + l);
            if (!finite32(x[l])) status |= QS_BAD_INPUT;
            if (qw[32 * j + l] != 0.0f) none = false;
        }
        for (int l = 0; l < 32; ++l) w[l] = (none ? 1.0f : qw[32 * j + l]) * sqrtf(sigma2 + x[l] * x[l]);
        status |= sub_search_w<NMAX>(x, w, &scale[j], &tmin[j], &sw[j]);
    }
    const float d = quant_scales_w(scale, sw, Ls), dmin = quant_scales_w(tmin, sw, Lm);
    *dh = f16_bits(d);
    *dminh = f16_bits(dmin);
    if (!f16_finite(*dh) || !f16_finite(*dminh)) status |= QS_BAD_D;
    for (int j = 0; j < 8; ++j) {   // (clampf maps NaN to its lower bound, and a negative level -- a negative scale -- to 0)
        sc[j] = (unsigned)clampf(Ls[j], 0.0f, 63.0f);
        mm[j] = (unsigned)clampf(Lm[j], 0.0f, 63.0f);
    }
    return status;
}

// get_scale_min_k4's packing of eight 6-bit scales and minima into 12 bytes, as three little-endian words
RCA_QHD void pack_scales_k4(const unsigned* sc, const unsigned* m, unsigned* words) {
    words[0] = words[1] = words[2] = 0;
    for (int j = 0; j < 4; ++j) {
        words[0] |= ((sc[j] & 63u) | ((sc[j + 4] >> 4) << 6)) << (8 * j);
        words[1] |= ((m[j] & 63u) | ((m[j + 4] >> 4) << 6)) << (8 * j);
        words[2] |= ((sc[j + 4] & 0xFu) | ((m[j + 4] & 0xFu) << 4)) << (8 * j);
    }
}

// d, dmin and the eight (sc, m) of a super-block, then its levels q = nearest((x + dmin m) / (d sc)) in the file's order
template <int NMAX, typename T>
RCA_QHD void store_block_qk(const T* src, int rule, unsigned short dh, unsigned short dminh, const unsigned* sc, const unsigned* mm, unsigned* out) {
    const float df = f16_value(dh), dminf = f16_value(dminh);
    out[0] = (unsigned)dh | ((unsigned)dminh << 16);
    pack_scales_k4(sc, mm, out + 1);
    constexpr int QS0 = NMAX == 31 ? 12 : 4;   // word offset of qs: after d, dmin, scales (and Q5_K's 32 bytes of high bits)
    unsigned qh[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int t = 0; t < 4; ++t) {
        unsigned char q[2][32];
        for (int half = 0; half < 2; ++half) {
            const int j = 2 * t + half;
            const float d1 = df * (float)sc[j], m1 = dminf * (float)mm[j];
            for (int l = 0; l < 32; ++l) {
                const float v = ldf(src, 32 * j + l);
                float qq;
                if (rule) qq = d1 != 0.0f ? rintf((v + m1) / d1) : 0.0f;
                else qq = d1 > 0.0f ? floorf((v + m1) / d1 + 0.5f) : 0.0f;
                q[half][l] = (unsigned char)clampf(qq, 0.0f, (float)NMAX);
            }
        }
        for (int c = 0; c < 8; ++c) {
            unsigned word = 0;
            for (int b = 0; b < 4; ++b) {
                const int l = 4 * c + b;
                word |= (((unsigned)q[0][l] & 0xFu) | (((unsigned)q[1][l] & 0xFu) << 4)) << (8 * b);
                qh[c] |= ((((unsigned)q[0][l] >> 4) & 1u) << (2 * t) | (((unsigned)q[1][l] >> 4) & 1u) << (2 * t + 1)) << (8 * b);
            }
            out[QS0 + 8 * t + c] = word;
        }
    }
    if (NMAX == 31)
        for (int c = 0; c < 8; ++c) out[4 + c] = qh[c];
}
// the super-block under column weights qw[256] (rca_quantize_rows_w): scales by block_scales_w, levels stored as rule 1 stores them
template <int NMAX, typename T>
RCA_QHD int quantize_block_qk_w(const T* src, const float* qw, unsigned* out) {
    unsigned short dh, dminh;
    unsigned sc[8], mm[8];
    const int status = block_scales_w<NMAX>(src, qw, &dh, &dminh, sc, mm);
    if (status & QS_BAD_INPUT)
        for (int j = 0; j < 8; ++j) sc[j] = mm[j] = 0;
    store_block_qk<NMAX>(src, 1, dh, dminh, sc, mm, out);
    return status;
}

// One Q4_K (NMAX 15, 144 bytes) or Q5_K (NMAX 31, 176 bytes) super-block.  out is 4-byte aligned (both block sizes are multiples of 16).
// qw: column weights [256] of rca_quantize_rows_w (rule 1 only), or null.
template <int NMAX, typename T>
RCA_QHD int quantize_block_qk(const T* src, int rule, unsigned* out, const float* qw = nullptr) {
    if (qw) return quantize_block_qk_w<NMAX>(src, qw, out);
    float scale[8], tmin[8];
    int status = QS_OK;
    float max_scale = 0.0f, max_min = 0.0f;
    for (int j = 0; j < 8; ++j) {
        float x[32];
        for (int l = 0; l < 32; ++l) {
            x[l] = ldf(src, 32 * j + l);
            if (!finite32(x[l])) status |= QS_BAD_INPUT;
        }
        status |= rule ? sub_search<NMAX>(x, &scale[j], &tmin[j]) : sub_minmax<NMAX>(x, &scale[j], &tmin[j]);
        if (rule) {
            if (scale[j] > max_scale) max_scale = scale[j];
            if (tmin[j] > max_min) max_min = tmin[j];
        } else {
            max_scale = fmaxf(max_scale, scale[j]);
            max_min = fmaxf(max_min, tmin[j]);
        }
    }
    const unsigned short dh = f16_bits(max_scale / 63.0f), dminh = f16_bits(max_min / 63.0f);
    if (!f16_finite(dh) || !f16_finite(dminh)) status |= QS_BAD_D;
    const float df = f16_value(dh), dminf = f16_value(dminh);
    const float inv_s = max_scale > 0.0f ? 63.0f / max_scale : 0.0f, inv_m = max_min > 0.0f ? 63.0f / max_min : 0.0f;
    unsigned sc[8], mm[8];
    for (int j = 0; j < 8; ++j) {
        float a, b;
        if (rule) {
            a = rintf(inv_s * scale[j]);
            b = rintf(inv_m * tmin[j]);
        } else {
            a = df > 0.0f ? floorf(scale[j] / df + 0.5f) : 0.0f;
            b = dminf > 0.0f ? floorf(tmin[j] / dminf + 0.5f) : 0.0f;
        }
        sc[j] = (unsigned)clampf(a, 0.0f, 63.0f);
        mm[j] = (unsigned)clampf(b, 0.0f, 63.0f);
    }
    if (status & QS_BAD_INPUT) {   // NaN scales must not reach the casts above as anything but 0: clampf maps NaN to its lower bound
        for (int j = 0; j < 8; ++j) sc[j] = mm[j] = 0;
    }
    store_block_qk<NMAX>(src, rule, dh, dminh, sc, mm, out);
    return status;
}

// ---- a group of 16 values, symmetric: scale with value ~ scale * l, l in -32..31
RCA_QHD float group_search(const float* x) {
    constexpr float NM = 32.0f;
    float mx = 0.0f, amax = 0.0f;
    for (int l = 0; l < 16; ++l) {
        const float ax = fabsf(x[l]);
        if (ax > amax) {
            amax = ax;
            mx = x[l];
        }
    }
    if (amax < 1e-15f) return 0.0f;
    float scale = 0.0f, best = 0.0f;
    for (int is = -10; is <= 9; ++is) {   // -10 stands for the starting candidate iscale = -32 / max; 0 is skipped
        if (is == 0) continue;
        const float iscale = is == -10 ? -NM / mx : -(NM + 0.1f * (float)is) / mx;
        float slx = 0.0f, sl2 = 0.0f;
        for (int l = 0; l < 16; ++l) {
            const float lv = clampf(rintf(iscale * x[l]), -NM, NM - 1.0f);
            const float w = x[l] * x[l];
            slx = slx + (w * x[l]) * lv;
            sl2 = sl2 + (w * lv) * lv;
        }
        if (is == -10) {
            scale = sl2 != 0.0f ? slx / sl2 : 0.0f;
            best = scale * slx;
        } else if (sl2 > 0.0f && slx * slx > best * sl2) {
            scale = slx / sl2;
            best = scale * slx;
        }
    }
    return scale;
}

// the same group under column weights qw[16] in the place of x^2 (rca_quantize_rows_w); weights that are all 0 count as 1.0
RCA_QHD float group_search_w(const float* x, const float* qw) {
    constexpr float NM = 32.0f;
    float mx = 0.0f, amax = 0.0f;
    bool none = true;
    for (int l = 0; l < 16; ++l) {
        const float ax = fabsf(x[l]);
        if (ax > amax) {
            amax = ax;
            mx = x[l];
        }
        if (qw[l] != 0.0f) none = false;
    }
    if (amax < 1e-15f) return 0.0f;
    float scale = 0.0f, best = 0.0f;
    for (int is = -10; is <= 9; ++is) {
        if (is == 0) continue;
        const float iscale = is == -10 ? -NM / mx : -(NM + 0.1f * (float)is) / mx;
        float slx = 0.0f, sl2 = 0.0f;
        for (int l = 0; l < 16; ++l) {
            const float lv = clampf(rintf(iscale * x[l]), -NM, NM - 1.0f);
            const float w = none ? 1.0f : qw[l];
            slx = slx + (w * x[l]) * lv;
            sl2 = sl2 + (w * lv) * lv;
        }
        if (is == -10) {
            scale = sl2 != 0.0f ? slx / sl2 : 0.0f;
            best = scale * slx;
        } else if (sl2 > 0.0f && slx * slx > best * sl2) {
            scale = slx / sl2;
            best = scale * slx;
        }
    }
    return scale;
}

// One Q6_K super-block (210 bytes: ql[128], qh[64], int8 scales[16], fp16 d).  out is 2-byte aligned.  qw: column weights [256] of
// rca_quantize_rows_w (rule 1 only), or null.
template <typename T>
RCA_QHD int quantize_block_q6k(const T* src, int rule, unsigned short* out, const float* qw = nullptr) {
    float scale[16];
    int status = QS_OK;
    float max_scale = 0.0f, max_abs = 0.0f;
    for (int g = 0; g < 16; ++g) {
        float x[16];
        float amax = 0.0f;
        for (int l = 0; l < 16; ++l) {
            x[l] = ldf(src, 16 * g + l);
            if (!finite32(x[l])) status |= QS_BAD_INPUT;
            amax = fmaxf(amax, fabsf(x[l]));
        }
        scale[g] = rule ? (qw ? group_search_w(x, qw + 16 * g) : group_search(x)) : amax / 31.0f;
        if (!finite32(scale[g])) status |= QS_BAD_D;
        const float as = fabsf(scale[g]);
        if (as > max_abs) {
            max_abs = as;
            max_scale = scale[g];
        }
    }
    float df;
    unsigned short dh;
    int sc[16];
    bool zero = false;
    if (rule) {
        zero = max_abs < 1e-15f;
        const float iscale = -128.0f / (zero ? 1.0f : max_scale);
        dh = zero ? (unsigned short)0 : f16_bits(1.0f / iscale);
        df = f16_value(dh);
        for (int g = 0; g < 16; ++g) sc[g] = zero ? 0 : (int)clampf(rintf(iscale * scale[g]), -128.0f, 127.0f);
    } else {
        dh = f16_bits(max_abs / 127.0f);
        df = f16_value(dh);
        for (int g = 0; g < 16; ++g) sc[g] = (int)clampf(df > 0.0f ? floorf(scale[g] / df + 0.5f) : 0.0f, 0.0f, 127.0f);
    }
    if (!f16_finite(dh)) status |= QS_BAD_D;
    if (status & QS_BAD_INPUT)
        for (int g = 0; g < 16; ++g) sc[g] = 0;
    for (int n = 0; n < 2; ++n) {
        for (int l2 = 0; l2 < 16; ++l2) {
            unsigned lo[2] = {0, 0}, hi = 0;   // ql[64 n + l], ql[64 n + 32 + l], qh[32 n + l] for l = 2 l2, 2 l2 + 1
            for (int b = 0; b < 2; ++b) {
                const int l = 2 * l2 + b;
                unsigned u[4];
                for (int qr = 0; qr < 4; ++qr) {
                    const int e = 128 * n + 32 * qr + l;
                    const float step = df * (float)sc[e >> 4];
                    const float v = ldf(src, e);
                    float qq;
                    if (rule) qq = step != 0.0f ? rintf(v / step) : 0.0f;
                    else qq = step > 0.0f ? floorf(v / step + 0.5f) : 0.0f;
                    u[qr] = zero ? 0u : (unsigned)((int)clampf(qq, -32.0f, 31.0f) + 32);
                }
                lo[0] |= ((u[0] & 0xFu) | ((u[2] & 0xFu) << 4)) << (8 * b);
                lo[1] |= ((u[1] & 0xFu) | ((u[3] & 0xFu) << 4)) << (8 * b);
                hi |= ((u[0] >> 4) | ((u[1] >> 4) << 2) | ((u[2] >> 4) << 4) | ((u[3] >> 4) << 6)) << (8 * b);
            }
            out[32 * n + l2] = (unsigned short)lo[0];
            out[32 * n + 16 + l2] = (unsigned short)lo[1];
            out[64 + 16 * n + l2] = (unsigned short)hi;
        }
    }
    for (int g2 = 0; g2 < 8; ++g2) out[96 + g2] = (unsigned short)(((unsigned)sc[2 * g2] & 0xFFu) | (((unsigned)sc[2 * g2 + 1] & 0xFFu) << 8));
    out[104] = dh;
    return status;
}

// One Q8_0 block (34 bytes: fp16 d, 32 int8): lm_q8_quantize_kernel's rule.  out is 2-byte aligned.
template <typename T>
RCA_QHD int quantize_block_q8_0(const T* src, unsigned short* out) {
    float v[32];
    float amax = 0.0f;
    int status = QS_OK;
    for (int j = 0; j < 32; ++j) {
        v[j] = ldf(src, j);
        if (!finite32(v[j])) status |= QS_BAD_INPUT;
        amax = fmaxf(amax, fabsf(v[j]));
    }
    const float dd = amax / 127.0f;
    const float id = dd != 0.0f ? 1.0f / dd : 0.0f;
    const unsigned short dh = f16_bits(dd);
    if (!f16_finite(dh)) status |= QS_BAD_D;
    out[0] = dh;
    for (int j = 0; j < 16; ++j) {
        const int a = (status & QS_BAD_INPUT) ? 0 : (int)roundf(v[2 * j] * id), b = (status & QS_BAD_INPUT) ? 0 : (int)roundf(v[2 * j + 1] * id);
        out[1 + j] = (unsigned short)(((unsigned)a & 0xFFu) | (((unsigned)b & 0xFFu) << 8));
    }
    return status;
}

}  // namespace rca_quant
