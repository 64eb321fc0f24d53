"""The importance matrix's column sums restated in numpy (TEST INFRASTRUCTURE ONLY): the bit-exact definition of what the kernel behind
rca_lm_imatrix_rows_tap adds for one pair of planes.

Definition (include/rca.h, rca_lm_imatrix_rows_tap): planes hi, lo [rows][K] (bf16 bits) of a pass with m live rows; per column j
  v_r = f32(hi[r][j]) + f32(lo[r][j])        one f32 add
  s_r = v_r * v_r                            one f32 multiply (no fma)
  p_b = ((0.0f + s_r0) + s_r1) + ...         over the rows of token block b = rows 128 b .. min(128 b + 127, m - 1), ascending
  acc[j] += (double) p_b                     b ascending
Rows >= m are never read."""
import numpy as np

f32 = np.float32
# the matrices that share an input vector: 0 = the QKV input, 1 = the O input, 2 = the gate / up input, 3 = the down input
NAMES = {0: ("attn_q", "attn_k", "attn_v"), 1: ("attn_output",), 2: ("ffn_gate", "ffn_up"), 3: ("ffn_down",)}


def bf16_to_f32(bits):
    return (np.asarray(bits, np.uint16).astype(np.uint32) << 16).view(np.float32)


def f32_to_bf16(v):
    """round to nearest even (finite values)"""
    b = np.ascontiguousarray(v, np.float32).view(np.uint32)
    return ((b + np.uint32(0x7FFF) + ((b >> 16) & np.uint32(1))) >> 16).astype(np.uint16)


def split_planes(v):
    """f32 [rows, K] -> (hi, lo) bf16 bits with hi = bf16(v), lo = bf16(v - hi): how the tile route stages a GEMM input"""
    v = np.ascontiguousarray(v, np.float32)
    hi = f32_to_bf16(v)
    return hi, f32_to_bf16(v - bf16_to_f32(hi))


def collect(xh, xl, m_live, acc):
    """the definition: returns acc (float64 [K]) with the planes' first m_live rows added"""
    xh, xl = np.asarray(xh, np.uint16), np.asarray(xl, np.uint16)
    out = np.array(acc, np.float64)
    for r0 in range(0, int(m_live), 128):
        r1 = min(r0 + 128, int(m_live))
        v = (bf16_to_f32(xh[r0:r1]) + bf16_to_f32(xl[r0:r1])).astype(f32)
        s = (v * v).astype(f32)
        p = np.zeros(xh.shape[1], f32)
        for r in range(r1 - r0):
            p = (p + s[r]).astype(f32)
        out = out + p.astype(np.float64)
    return out
