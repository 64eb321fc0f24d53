// rca_lm.hip -- Llama-architecture autoregressive step on gfx950 (MI355X) with a
// llama_cpp.Llama-like control surface (include/rca.h, rca_lm_*).
//
// The deployed reference LM is codec_llama.py after persist_codec_embeddings
// (codec_llama.py:178-206): a vanilla Llama (RMSNorm, RoPE, GQA attention, SwiGLU, untied
// lm_head) evaluated by llama.cpp with 1-2 tokens per step (llamacpp_utils.py:145-161;
// realtime_agent_v2.py:355).  Here:
//   weights   bf16 in HBM, row-major [N][K]
//   decode    (1-8 tokens per pass) activations f32, every projection a wave-per-row-pair dot product with f32
//             accumulation, weights streamed once per step with non-temporal 16-B loads: HBM-bound, ~3 GB per step
//   prefill   (> 8 tokens) 128-token tiles on bf16 MFMA with hi/lo-split activations (lm_gemm128_kernel)
//   KV cache  fp16 [layer][pos][kv_head][64] (llama.cpp's default cache type)
//   attention decode: 256-key splits x blocks of 32 query rows on MFMA (K / V in whole rows through wave-private LDS images), the
//             splits merged inside the launch by data-tagged 8-byte granules; prefill: a flash-shaped kernel
//   sampler   logit bias + repeat / frequency / presence penalties patched in place -> histogram -> candidate gather ->
//             rank-by-counting top-k -> top-p/min-p/temperature -> inverse CDF (top_k 1..256), or the whole vocabulary by the
//             Gumbel-max rule behind radix-select rank / mass thresholds; counter-based RNG, polynomial exp / log, all on the device
//   the steady-state step (eval 1-2 tokens + sample) is captured once per context bucket into a hipGraph; the KV
//   position, input ids and RNG counter live in device memory so the graph replays unchanged.
#include <algorithm>
#include <type_traits>
#include <utility>
#include <cmath>
#include <climits>

#include "rca_common.h"

using namespace rca;

typedef unsigned short bf16_t;
typedef _Float16 f16_t;
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));

#define LM_MAXM 1024       // tokens per prefill pass (activation buffers): up to 8 token blocks of 128 share one launch per GEMM
#define LM_KV_RING LM_MAXM // q8_0 KV cache: positions of the fp16 staging ring the QKV epilogues store into (the largest pass)
#define LM_STATE_DECODE_BYTES (8 + 4 * 16)   // n_tokens, m and the ids a decode step / frame graph needs (LmDevState prefix)
#define LM_TILE32 32       // token tile of the small-model prefill kernels (lm_gemm_mfma_kernel)
#define LM_GEMV_M 2        // tokens per decode pass (GEMV kernels); evals longer than LM_PREFILL_MIN go through the MFMA prefill path
#define LM_PREFILL_MIN 8    // evals of up to this many tokens are decode passes, longer ones prefill tiles
#define LM_KSLICE 2048     // widest hidden / attention-output dimension (one 16-byte chunk per lane and wave in the GEMV)
#define LM_MAXSPLIT 4      // ffn <= LM_KSLICE * LM_MAXSPLIT (up to four chunks per lane and wave)
#define ATT_KEYS 256       // keys per attention workgroup (8 waves x 32 keys)
#define LM_GRAPH_BUCKETS 8  // 4, 8, ..., 256 splits, the last bucket = all of them
#define ATT_EPOCH_INTS 64          // att_arrive: 64 launch counters (one per kv head), then the granules [kv head][split][8 rows][66]
#define ATT_TAG_MAXSP 128         // splits the in-launch merge can gather: nkv * splits <= 256 with at least 2 kv heads
#define ATT_TAG_SPINS (1 << 22)   // bound of the merger's re-polls (seconds): a NaN row tells
#define SAMP_MAXK 256
#define LM_FRAME_MAX 8        // steps of one frame graph (a chunk is 4-5 frames per channel, realtime_agent_config.py:21,56)
#define LM_FRAME_USER0 8     // LmDevState::ids[LM_FRAME_USER0 + i] = the user's token of frame i (ids[0..1] is the pair being evaluated)

struct LmDevState {
    int n_tokens;      // KV position of the first token of the current pass
    int m;             // tokens in the current pass
    int ids[LM_MAXM];
    unsigned long long rng_counter;
    int out_token;
    int pad;
    int frame_out[LM_FRAME_MAX];   // rca_lm_frame: the token sampled by each step of the frame
};

struct SamplerDev {
    int top_k;
    float top_p, min_p, temp;
    unsigned long long seed;
    int n_bias;
    int bias_ids[8];
    float bias_vals[8];
    // llama.cpp's penalties sampler (llama_sampler_penalties; llama-cpp-python adds it with penalty_last_n = last_n_tokens_size = 64
    // behind the logits processor and in front of top_k): over the last `last_n` tokens THIS sampler accepted
    float repeat_penalty, freq_penalty, presence_penalty;
    int last_n;
    int patch;      // 1: logit bias and / or penalties are applied IN PLACE by samp_prepare_kernel and undone by the sampler's last kernel
    int big_k;      // > 0: the "big" path cuts at this rank (top_k > SAMP_MAXK); 0: no rank cut
    int big_p;      // 1: the "big" path cuts at top_p of the candidates' mass (fixed point)
    // ---- rca_lm_sampler_set_typical / _set_mirostat (appended: the kernels from before them read none of these)
    float typical_p;   // in (0, 1): samp_final_typ_kernel cuts the serial chain's candidates to the locally typical set; anything else = off
    int miro;          // 2: mirostat v2 (the samp_miro_* launches); 0 = off
    float miro_tau, miro_eta;
};

typedef float f32x16 __attribute__((ext_vector_type(16)));
__device__ __forceinline__ bf16_t f32_to_bf16_rne(float f) {
    unsigned u = __float_as_uint(f);
    u += 0x7FFFu + ((u >> 16) & 1u);
    return (bf16_t)(u >> 16);
}
__device__ __forceinline__ float bf16_lo(unsigned u) { return __uint_as_float(u << 16); }
__device__ __forceinline__ float bf16_hi(unsigned u) { return __uint_as_float(u & 0xffff0000u); }
// Cross-lane butterflies without the LDS crossbar: xor 32 / 16 through the gfx950 permlane swaps, xor 8..1 through
// DPP.  Pairing order is 32,16,8,4,2,1 exactly like a __shfl_xor loop, so sums keep the same bits.
template <int CTRL>
__device__ __forceinline__ float dpp_mov(float v) {
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xF, 0xF, true));
}
#define DPP_XOR1 0xB1          // quad_perm [1,0,3,2]
#define DPP_XOR2 0x4E          // quad_perm [2,3,0,1]
#define DPP_ROR4 0x124         // row_ror:4  (== xor 4 once lanes i and i^8 agree)
#define DPP_ROR8 0x128         // row_ror:8  (== xor 8 inside a row of 16)
#define DPP_HALF_MIRROR 0x141  // i -> 7-i inside 8 lanes (== xor 4 once the quads are uniform)
template <typename OP>
__device__ __forceinline__ float wave_butterfly(float v, OP op) {
    // v_permlane{32,16}_swap exchange halves / odd-even rows between TWO registers.  Written as asm: this
    // compiler's builtin mis-assigns the second result.  s_nop covers the VALU-write -> permlane-read hazard
    // the assembler does not see inside an asm block.
    float a = v, b = v;
    asm volatile("s_nop 1\n\tv_permlane32_swap_b32 %0, %1\n\ts_nop 1" : "+v"(a), "+v"(b));   // a = [lo, lo], b = [hi, hi]
    v = op(a, b);
    a = v; b = v;
    asm volatile("s_nop 1\n\tv_permlane16_swap_b32 %0, %1\n\ts_nop 1" : "+v"(a), "+v"(b));   // a = [r0,r0,r2,r2], b = [r1,r1,r3,r3]
    v = op(a, b);
    v = op(v, dpp_mov<DPP_ROR8>(v));
    v = op(v, dpp_mov<DPP_ROR4>(v));
    v = op(v, dpp_mov<DPP_XOR2>(v));
    v = op(v, dpp_mov<DPP_XOR1>(v));
    return v;
}
__device__ __forceinline__ float wave_sum(float v) {
    return wave_butterfly(v, [](float a, float b) { return a + b; });
}
__device__ __forceinline__ float wave_max(float v) {
    return wave_butterfly(v, [](float a, float b) { return fmaxf(a, b); });
}

// ------------------------------------------------------------------------------------- embed
// The table is gathered, never streamed, so it keeps the precision it arrived in: bf16 rows for a bf16 checkpoint, f32 rows for
// an F32 / F16 tensor or a de-quantised Q8_0 / Q4_K one (llama.cpp de-quantises embedding rows exactly, get_rows) -- `f32tab`.
__global__ __launch_bounds__(256) void lm_embed_kernel(const LmDevState* __restrict__ stt, const void* __restrict__ table, int f32tab,
                                                       float* __restrict__ x, int H, int V) {
    const int m = blockIdx.x;
    if (m >= stt->m) return;
    int id = stt->ids[m];
    id = id < 0 ? 0 : (id >= V ? V - 1 : id);
    if (f32tab) {
        const float* row = reinterpret_cast<const float*>(table) + (long)id * H;
        for (int h = threadIdx.x; h < H; h += 256) x[(long)m * H + h] = row[h];
    } else {
        const bf16_t* row = reinterpret_cast<const bf16_t*>(table) + (long)id * H;
        for (int h = threadIdx.x; h < H; h += 256) x[(long)m * H + h] = __uint_as_float((unsigned)row[h] << 16);
    }
}

// --------------------------------------------------- residual add + RMSNorm shared arithmetic
// A wave owns one token row: lane l holds the 8-element chunks c = l + 64*it (it < 4, K <= 2048), adds the
// partial slices in order, accumulates sum(v^2) as an fma chain (it ascending, element ascending), reduces it
// with the xor-shuffle tree and scales (v * rstd) * w.  Used verbatim by the decode GEMV prologue (registers) and
// by the prefill norm kernel, so both paths produce identical bits.
template <typename F>
__device__ __forceinline__ float lm_row_norm(float (&v)[4][8], int nchunk, int K, float eps, F&& after_add) {
    const int lane = threadIdx.x & 63;
    float ss = 0.0f;
#pragma unroll
    for (int it = 0; it < 4; ++it) {
        const int c = lane + 64 * it;
        if (c < nchunk) {
            after_add(it, c);
#pragma unroll
            for (int j = 0; j < 8; ++j) ss = __builtin_fmaf(v[it][j], v[it][j], ss);
        }
    }
    ss = wave_sum(ss);
    return rsqrtf(ss / (float)K + eps);
}
__device__ __forceinline__ void lm_load_row(float (&v)[4][8], const float* __restrict__ row, int nchunk, bool valid) {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int it = 0; it < 4; ++it) {
        const int c = lane + 64 * it;
        if (valid && c < nchunk) {
            const float4 a = *reinterpret_cast<const float4*>(row + c * 8);
            const float4 b = *reinterpret_cast<const float4*>(row + c * 8 + 4);
            v[it][0] = a.x; v[it][1] = a.y; v[it][2] = a.z; v[it][3] = a.w;
            v[it][4] = b.x; v[it][5] = b.y; v[it][6] = b.z; v[it][7] = b.w;
        } else {
#pragma unroll
            for (int j = 0; j < 8; ++j) v[it][j] = 0.0f;
        }
    }
}
__device__ __forceinline__ void lm_add_row(float (&v)[4][8], const float* __restrict__ row, int nchunk) {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int it = 0; it < 4; ++it) {
        const int c = lane + 64 * it;
        if (c < nchunk) {
            const float4 a = *reinterpret_cast<const float4*>(row + c * 8);
            const float4 b = *reinterpret_cast<const float4*>(row + c * 8 + 4);
            v[it][0] += a.x; v[it][1] += a.y; v[it][2] += a.z; v[it][3] += a.w;
            v[it][4] += b.x; v[it][5] += b.y; v[it][6] += b.z; v[it][7] += b.w;
        }
    }
}
__device__ __forceinline__ void lm_store_row(const float (&v)[4][8], float* __restrict__ row, int nchunk) {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int it = 0; it < 4; ++it) {
        const int c = lane + 64 * it;
        if (c < nchunk) {
            *reinterpret_cast<float4*>(row + c * 8) = make_float4(v[it][0], v[it][1], v[it][2], v[it][3]);
            *reinterpret_cast<float4*>(row + c * 8 + 4) = make_float4(v[it][4], v[it][5], v[it][6], v[it][7]);
        }
    }
}
__device__ __forceinline__ void lm_scale_row(float (&v)[4][8], float rstd, const float* __restrict__ w, int nchunk) {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int it = 0; it < 4; ++it) {
        const int c = lane + 64 * it;
        if (c < nchunk) {
            const float4 a = *reinterpret_cast<const float4*>(w + c * 8);
            const float4 b = *reinterpret_cast<const float4*>(w + c * 8 + 4);
            const float wv[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
#pragma unroll
            for (int j = 0; j < 8; ++j) v[it][j] = (v[it][j] * rstd) * wv[j];
        }
    }
}

// prefill chunks: one wave per token
__global__ __launch_bounds__(64) void lm_add_rmsnorm_kernel(const LmDevState* __restrict__ stt, const float* __restrict__ xin,
                                                            float* __restrict__ xout, const float* __restrict__ parts, int nparts,
                                                            long part_stride, const float* __restrict__ w, float* __restrict__ xn,
                                                            int K, float eps, bf16_t* __restrict__ hi = nullptr,
                                                            bf16_t* __restrict__ lo = nullptr) {
    const int m = blockIdx.x;
    if (m >= stt->m) return;
    const int nchunk = K >> 3;
    float v[4][8];
    lm_load_row(v, xin + (long)m * K, nchunk, true);
    for (int s2 = 0; s2 < nparts; ++s2) lm_add_row(v, parts + s2 * part_stride + (long)m * K, nchunk);
    if (xout) lm_store_row(v, xout + (long)m * K, nchunk);
    const float rstd = lm_row_norm(v, nchunk, K, eps, [](int, int) {});
    lm_scale_row(v, rstd, w, nchunk);
    if (hi) {   // prefill tiles: the normalised row goes straight out as the bf16 hi + lo pair the MFMA GEMM reads
        const int lane = threadIdx.x & 63;
#pragma unroll
        for (int it = 0; it < 4; ++it) {
            const int c = lane + 64 * it;
            if (c < nchunk) {
                unsigned ph[4], pl[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const bf16_t h0 = f32_to_bf16_rne(v[it][2 * j]), h1 = f32_to_bf16_rne(v[it][2 * j + 1]);
                    const bf16_t l0 = f32_to_bf16_rne(v[it][2 * j] - __uint_as_float((unsigned)h0 << 16));
                    const bf16_t l1 = f32_to_bf16_rne(v[it][2 * j + 1] - __uint_as_float((unsigned)h1 << 16));
                    ph[j] = (unsigned)h0 | ((unsigned)h1 << 16);
                    pl[j] = (unsigned)l0 | ((unsigned)l1 << 16);
                }
                *reinterpret_cast<uint4*>(hi + (long)m * K + c * 8) = make_uint4(ph[0], ph[1], ph[2], ph[3]);
                *reinterpret_cast<uint4*>(lo + (long)m * K + c * 8) = make_uint4(pl[0], pl[1], pl[2], pl[3]);
            }
        }
    } else {
        lm_store_row(v, xn + (long)m * K, nchunk);
    }
}

// ------------------------------------------------------------------------------------ GEMV (decode passes, M <= 2)
// y[m][n] = sum_k W[n][k] * x[m][k] for the 1-2 tokens of a decode pass, weights streamed ONCE with non-temporal 16-byte
// loads.  Shape of the kernel:
//   * the 4 waves of a workgroup split K: wave w owns the chunk range [w * cpw, (w + 1) * cpw) (a chunk = 8 bf16 = one
//     16-byte lane load), so a lane keeps only ITS x values in registers (8 * NIT * M floats: 16 for the 2048-wide
//     projections) and the registers go to weights in flight instead: R rows x NIT chunks are requested per batch before
//     anything is consumed (R = 16: 16 KB per wave, ~200 KB per CU);
//   * per lane, per (row, token): one fma chain over its chunks (chunk ascending, element ascending);
//   * the R * M partial sums of a batch are reduced across the 64 lanes TOGETHER: two transposing steps on the gfx950
//     permlane swaps (xor 32, xor 16: every exchange halves the number of live registers) and four DPP steps inside the
//     rows of 16 -- R * M / 4 + ... instead of R * M butterflies; lane 0 of row q then holds value i + (V/4)(q&1) + (V/2)(q>>1);
//   * the 4 waves' sums meet in LDS (double-buffered by batch parity: one barrier per batch) and are added in wave order by
//     the first V threads, which run the fused epilogue.
// Any (R, batches per workgroup) gives the same bits: a value's reduction sequence does not depend on its slot
// (tests/test_gemv_gpu.py runs "4,1" and "8,4" against the defaults in child processes).
//   PRO 1: prologue = RMSNorm of the residual row(s): each wave squares its own K range, the 4 partial sums are added in
//          wave order; xs = (v * rstd) * norm_w.  only_last: the single row handled is the pass's last token (head).
//   EPI 0: store (logits)          EPI 1: rows (2i, 2i+1) = (gate_i, up_i): h = silu(g) * u
//   EPI 2: QKV rows paired (d, d+32) inside each head: RoPE (HF rotate_half), q back to qkv[], k / v straight into the
//          fp16 KV cache at position n_tokens + m          EPI 3: add into the residual stream in place
struct GemvPro {
    const float* xin; const float* norm_w; float eps; int only_last;
};
struct GemvRope {
    const float* cos_t; const float* sin_t; f16_t* kc; f16_t* vc; int nh, nkv, n_ctx;
    int row_base;   // first row of this matrix inside the fused [q; k; v] layout (a multiple of 64): a Q4_K_M file keeps some attn_v tensors
                    // in another format than attn_q / attn_k, and such a layer's V projection is a matrix of its own
    int pos_mask = -1;   // a row of position p is stored at row p & pos_mask of kc / vc: all ones over the fp16 cache itself, ring size - 1
                         // over the staging ring of a q8_0 cache (rca_lm_set_kv_format), whose rows lm_kv_quant_kernel quantises
};
__device__ __forceinline__ void lane_swap32(float& a, float& b) {   // a = [a.lo, b.lo], b = [a.hi, b.hi]
    asm volatile("s_nop 1\n\tv_permlane32_swap_b32 %0, %1\n\ts_nop 1" : "+v"(a), "+v"(b));
}
__device__ __forceinline__ void lane_swap16(float& a, float& b) {   // a = [a.r0, b.r0, a.r2, b.r2], b = [a.r1, b.r1, a.r3, b.r3]
    asm volatile("s_nop 1\n\tv_permlane16_swap_b32 %0, %1\n\ts_nop 1" : "+v"(a), "+v"(b));
}
__device__ __forceinline__ float row16_sum(float v) {   // sum over the 16 lanes of a DPP row, every lane gets it
    v = v + dpp_mov<DPP_ROR8>(v);
    v = v + dpp_mov<DPP_ROR4>(v);
    v = v + dpp_mov<DPP_XOR2>(v);
    v = v + dpp_mov<DPP_XOR1>(v);
    return v;
}
// V values per lane -> V / 4 registers; afterwards register i of row q (16 lanes) holds the full sum of value
// i + (V / 4) * (q & 1) + (V / 2) * (q >> 1).  V is a multiple of 4.
template <int V>
__device__ __forceinline__ void wave_reduce_transposed(float (&val)[V]) {
#pragma unroll
    for (int i = 0; i < V / 2; ++i) {
        lane_swap32(val[i], val[i + V / 2]);
        val[i] = val[i] + val[i + V / 2];
    }
#pragma unroll
    for (int i = 0; i < V / 4; ++i) {
        lane_swap16(val[i], val[i + V / 4]);
        val[i] = val[i] + val[i + V / 4];
    }
#pragma unroll
    for (int i = 0; i < V / 4; ++i) val[i] = row16_sum(val[i]);
}

// Q = 1: weights are q8_0 (GGUF block_q8_0: 32 int8 + one fp16 scale, what the reference deploys besides F16 and Q4_K_M,
// prep_test_model.sh:28-31) kept PACKED in HBM -- 8.5 bits per weight streamed instead of 16.  Device layout (built once at load
// from the 34-byte blocks): slot pairs interleaved, qs[pair][chunk] = 8 int8 of the pair's first row + 8 of its second row for
// the same 8 k (one 16-byte lane load feeds two rows with the x values the lane already holds), scales sc[k / 32][pair] =
// (fp16, fp16) so a lane fetches the scales of a whole batch with one or two vector loads.  Arithmetic per lane and row:
// p = fma chain of (float)q_j * x_j over its 8 elements, then d * p accumulated per chunk -- f32 activations throughout
// (llama.cpp quantises the activations to q8_1 for this product; by default only the weights are quantised here, and the opt-in
// ACT = 1 instances of lm_gemv_kernel do what llama.cpp does).
// (float)(int8) of byte `b` of a dword.  The dword must have passed through q8_opaque() first:
//   * if the optimiser can see that a loaded 16-byte value is only ever used byte by byte, it re-types the LOAD as sixteen byte
//     values and unpacks them the moment it lands -- 4x the registers and nothing left in flight;
//   * __builtin_amdgcn_sbfe + cast makes this compiler (ROCm 7.2) emit v_cvt_f32_u32_sdwa sext(...): the UNSIGNED conversion of
//     the sign-extended byte (4.29e9 for -1).
// Behind the opaque copy the plain shift / mask / cast form selects v_cvt_f32_i32_sdwa sext(BYTE_n): one instruction per element.
__device__ __forceinline__ unsigned q8_opaque(unsigned w) {
    asm volatile("" : "+v"(w));
    return w;
}
__device__ __forceinline__ float q8_byte_to_f32(unsigned w, int b) { return (float)(signed char)((w >> (8 * b)) & 0xffu); }
// (float) of UNSIGNED byte B of a dword as ONE instruction.  From the plain shift / mask / cast form this compiler selects
// v_cvt_f32_ubyte0 for byte 0 only and v_bfe_u32 + v_cvt_f32_ubyte0 for bytes 1-3: 96 extra instructions per 128 weights in the
// Q4_K body, whose VALU work (4.8 instructions per weight, not its bytes) is what bounds the Q4_K GEMVs: lm_head 70 -> 59.5 us,
// gate/up 9.6 -> 8.6, the step 0.686 -> 0.638 ms at 6.6 k context (profiles/r04/experiments/lm_step_micro.txt).
template <int B>
__device__ __forceinline__ float ubyte_to_f32(unsigned w) {
    float f;
    if constexpr (B == 0) asm("v_cvt_f32_ubyte0_e32 %0, %1" : "=v"(f) : "v"(w));
    else if constexpr (B == 1) asm("v_cvt_f32_ubyte1_e32 %0, %1" : "=v"(f) : "v"(w));
    else if constexpr (B == 2) asm("v_cvt_f32_ubyte2_e32 %0, %1" : "=v"(f) : "v"(w));
    else asm("v_cvt_f32_ubyte3_e32 %0, %1" : "=v"(f) : "v"(w));
    return f;
}
// kvalues_iq4nl, the table of the IQ4_NL / IQ4_XS types (restated from the published ggml definition): signed bytes, four per dword
#define IQ4_KV0 0xBFAD9881u   // -127 -104  -83  -65
#define IQ4_KV1 0xF6EADDCFu   //  -49  -35  -22  -10
#define IQ4_KV2 0x26190D01u   //    1   13   25   38
#define IQ4_KV3 0x71594535u   //   53   69   89  113
__host__ __device__ __forceinline__ int iq4_kv(unsigned q) {
    const unsigned long long t = (q & 8u) ? (((unsigned long long)IQ4_KV3 << 32) | IQ4_KV2) : (((unsigned long long)IQ4_KV1 << 32) | IQ4_KV0);   // constants: no memory
    return (int)(signed char)((t >> (8 * (q & 7u))) & 0xffu);
}
// Four table look-ups without touching memory: byte b of the result is kv[(w >> (8 b + SH)) & 15].  The table stays in four scalar
// dwords; v_perm_b32 picks a byte of a dword pair by a selector byte 0..7, so one permute reads the table's low half and one its
// high half with the indices' low three bits, and a third picks, byte by byte, which of the two holds: its selector is b + 4 * bit 3
// of index b, a bit-field insert of (w >> (SH + 1)) into the constant 0x03020100 under the mask 0x04040404.  Six vector
// instructions per four weights (and, two permutes, shift, insert, permute; SH = 4: one more shift).
template <int SH>
__device__ __forceinline__ unsigned iq4_map4(unsigned w) {
    const unsigned i3 = (SH ? w >> SH : w) & 0x07070707u;
    const unsigned lo = __builtin_amdgcn_perm(IQ4_KV1, IQ4_KV0, i3);
    const unsigned hi = __builtin_amdgcn_perm(IQ4_KV3, IQ4_KV2, i3);
    const unsigned w1 = w >> (SH + 1);
    const unsigned sel = (w1 & 0x04040404u) | (0x03020100u & ~0x04040404u);   // v_bfi_b32
    return __builtin_amdgcn_perm(hi, lo, sel);
}
// (float) of SIGNED byte B of a dword as one instruction (the SDWA form of v_cvt_f32_i32 with a sign-extended byte operand)
template <int B>
__device__ __forceinline__ float sbyte_to_f32(unsigned w) {
    float f;
    if constexpr (B == 0) asm("v_cvt_f32_i32_sdwa %0, sext(%1) dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:BYTE_0" : "=v"(f) : "v"(w));
    else if constexpr (B == 1) asm("v_cvt_f32_i32_sdwa %0, sext(%1) dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:BYTE_1" : "=v"(f) : "v"(w));
    else if constexpr (B == 2) asm("v_cvt_f32_i32_sdwa %0, sext(%1) dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:BYTE_2" : "=v"(f) : "v"(w));
    else asm("v_cvt_f32_i32_sdwa %0, sext(%1) dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:BYTE_3" : "=v"(f) : "v"(w));
    return f;
}
struct GemvQ8 {          // the packed (quantised) forms: q8_0, and Q4_K (dd != nullptr)
    const u32x4* qs;      // q8_0: [N / 2][K / 8] 16-byte units.  Q4_K: [N / 4][K / 8] units = 8 nibbles x 4 slots (q4k_* below)
    const unsigned* sc;   // q8_0: [ceil(N / 16)][K / 32][8]: (fp16, fp16) per pair and 32-element block, pairs in groups of 8 -- the scales a
                          // wave needs for a batch (<= 8 pairs x its 16 blocks) are ONE contiguous run (was [K / 32][N / 2]: 16
                          // separate lines per wave and load).  Q4_K: ushort (sc | m << 8) per slot and 32-element sub-block,
                          // [ceil(N / 16)][K / 32][16]
    const unsigned* dd;   // Q4_K: (fp16 d | fp16 dmin << 16) per slot and 256-element super-block, [ceil(N / 16)][K / 256][16]
};
// Q4_K (GGUF block_q4_K, what llama-quantize Q4_K_M writes for most tensors, prep_test_model.sh:31): 4-bit values with a 6-bit scale
// and a 6-bit minimum per 32 and two fp16 factors per 256: value = (d * sc) * q - (dmin * m).  Device layout, built once at load:
// slots (rows in the order the GEMV's epilogues pair them) in quads, qs[quad][k / 8] = one dword per slot holding the 8 nibbles of
// 8 consecutive k (nibble j at bits 4 j): a 16-byte lane load feeds four rows with the x values the lane holds; 4.6 bits per weight
// streamed.  Arithmetic per lane, slot and 8-k chunk: p = fma chain of q_j x_j (j ascending), then val += (d * sc) p - (dmin * m) sum(x).
// Q5_K (GGUF block_q5_K: the bulk of a Q5_K_S / Q5_K_M file) is the Q4_K block with a fifth bit per value: q in 0..31, same scales,
// minima and arithmetic.  Streamed as the Q4_K layout over the low nibbles plus ONE plane of high bits, qh[quad][k / 8]: a dword per
// quad and 8-k chunk, the lane's 17th to 20th byte of the chunk.  Bit 8 (j / 2) + 2 slot + (j & 1) is the high bit of element j of
// the quad's slot: shifted by 4 - 2 slot (even elements) or 3 - 2 slot (odd ones), the mask 0x10101010 leaves the four bits exactly
// where the nibble bytes `lo` / `hi` of the Q4_K body want their bit 4 -- a shift and an and-or per four weights.
__host__ __device__ __forceinline__ int q5k_hbit(int slot_in_quad, int j) { return 8 * (j >> 1) + 2 * slot_in_quad + (j & 1); }
// Q4_0 / Q4_1 (GGUF block_q4_0 / block_q4_1, the legacy 4-bit types): 4-bit values with one fp16 step per 32 (Q4_0: value = d (q - 8))
// or a step and a minimum (Q4_1: value = d q + m).  Both are the Q4_K form s q - t with (s, t) = (d, 8 d) resp. (d, -m), formed once at
// load (all exact in fp16).  Streamed as the Q4_K nibble layout plus ONE factor dword (fp16 s | fp16 t << 16) per slot and 32-value
// block, in q8.sc, [ceil(N / 16)][K / 32][16] (q4k_scm_index over dwords): 5.0 bits per weight for both types, no (sc, m) / (d, dmin)
// unpack and no d * sc / dmin * m products in the body.  Arithmetic as for Q4_K: val += s p - t sum(x).
// IQ4_NL / IQ4_XS (GGUF block_iq4_nl / block_iq4_xs): 4-bit INDICES into the 16-entry int8 table kvalues_iq4nl, with one fp16 step per 32
// (IQ4_NL: value = d kv[q]) or an fp16 step per 256 and a 6-bit scale per 32 (IQ4_XS: value = d (ls - 32) kv[q]).  Both are ONE device
// form, s kv[q], with the f32 factor s = d resp. d (ls - 32) formed once at load (11 x 6 bits: exact; s kv[q] is 17 x 7 bits: exact
// too, so every weight has one f32 value).  Streamed as the Q4_K nibble layout plus ONE f32 factor per slot and 32-value block, in
// q8.sc, [ceil(N / 16)][K / 32][16] -- the arrays and sizes of the Q4_0 form: 5.0 bits per weight for both types.  The body maps four
// nibbles at a time to their table bytes with byte permutes (iq4_map4) and has no minimum term: val += s sum kv[q_j] x_j.
__host__ __device__ __forceinline__ long q4k_scm_index(long slot, long kblock, long nkb) { return ((slot >> 4) * nkb + kblock) * 16 + (slot & 15); }
__host__ __device__ __forceinline__ long q8_sc_index(long pair, long kblock, long nkb) { return ((pair >> 3) * nkb + kblock) * 8 + (pair & 7); }
// The format a projection matrix is kept in (ONE copy per matrix; the decode GEMV streams it, the prefill tiles de-quantise it while
// staging): the GEMV's template parameter Q.
#ifndef RCA_GEMV_VARIANT
#define RCA_GEMV_VARIANT 0
#endif
#define WF_BF16 0   // bf16 [N][K]
#define WF_Q8 1     // GGUF q8_0, pair-interleaved (GemvQ8)
#define WF_F16 2    // fp16 [N][K] (the reference's default GGUF is F16, realtime_agent_resources.py:12)
#define WF_Q4K 3    // GGUF Q4_K, quad-interleaved nibbles (GemvQ8 with dd)
#define WF_Q5K 5    // GGUF Q5_K: the Q4_K layout (low nibbles, sc, dd) + one plane of high bits, q5k_hbit() above (5.6 bits per weight streamed)
#define WF_Q40 6    // GGUF Q4_0: the Q4_K nibble layout + one (fp16 s | fp16 t << 16) dword per slot and 32 values, s = d, t = 8 d (5.0 bits per weight streamed)
#define WF_Q41 7    // GGUF Q4_1: the same layout with t = -m.  The kernels know one form (template value WF_Q40); the id only tells the two apart in reports
#define WF_IQ4 8    // GGUF IQ4_NL: the Q4_K nibble layout (table indices) + one f32 factor s = d per slot and 32 values (5.0 bits per weight streamed)
#define WF_IQ4XS 9  // GGUF IQ4_XS: the same layout with s = d (ls - 32).  The kernels know one form (template value WF_IQ4); the id only tells the two apart in reports
#define WF_Q6K 4    // GGUF Q6_K re-encoded losslessly: int8 values (the 6-bit value - 32) in the q8_0 pair layout + one f32 scale d * sc per
                    // row and group of 16 ((s_a, s_b) per pair, pairs in groups of 8: [ceil(N / 16)][K / 16][8][2] floats); 10 bits per
                    // weight streamed (the file holds 6.6); d * sc * q is exact in f32, so the values are llama.cpp's dequantize_row_q6_K's
// What the HOST load path knows of a format, one row per WF_* id (WF_TABLE[id]): upload, conversion, packing and the reports read
// their constants here, the way the launchers get their template argument from wf_dispatch.  A component is an array holding
// `bytes` bytes per `per` values of a row.
enum { WA_NONE = 0, WA_W16, WA_Q, WA_D, WA_DD, WA_QS, WA_SC, WA_QH };   // arrays of RawMat (w16, q, d, dd) and of WMat (w, qs, sc, dd, qh)
struct WfPart { int arr, per, bytes; };
struct WfInfo {
    int id;
    const char* name;       // as the messages print it
    int device;             // the form the kernels are launched as (wf_dispatch's template value)
    int dtype;              // the RCA_* type its file blocks (16-bit formats: its values) arrive as ...
    int blk_vals, blk_bytes;   // ... values and bytes per block ...
    bool bad_flag;          // ... and whether its unblock / quantise kernels report a block whose factor is not finite
    WfPart plain[3];        // RawMat: the components, in the order parts() lists them
    int row_mult;           // RawMat: a row is a multiple of this many values
    int k_mult, n_mult;     // WMat (packed formats; k_mult 0: a 16-bit format, kept as it is) ...
    const char* n_word;     // ... and how the refusal words the multiple of N
    WfPart packed[4];       // WMat: the arrays lm_finish_mat allocates, in that order; sc / dd cover whole groups of 16 rows, zero padded
    int stream64;           // bytes one decode pass reads, in 64ths of a byte per weight (a packed matrix holds a multiple of 64 weights)
    WfPart mask;            // rca_lm_mask_head_rows: the array whose entries of a row are zeroed, `per` values to an entry
};
#define WF_PLAIN_4BIT {{WA_Q, 1, 1}, {WA_DD, 32, 4}}                       // a byte per value + one factor dword per 32
#define WF_PLAIN_K {{WA_Q, 1, 1}, {WA_D, 32, 2}, {WA_DD, 256, 4}}          // a byte per value + (sc | m << 8) per 32 + (d | dmin << 16) per 256
#define WF_PACKED_4BIT {{WA_QS, 2, 1}, {WA_SC, 32, 4}}
constexpr WfInfo WF_TABLE[] = {
    {WF_BF16, "bf16", WF_BF16, RCA_BF16, 1, 2, false, {{WA_W16, 1, 2}}, 1, 0, 0, "", {}, 128, {WA_W16, 1, 2}},
    {WF_Q8, "q8_0", WF_Q8, RCA_Q8_0, 32, 34, false, {{WA_Q, 1, 1}, {WA_D, 32, 2}}, 32, 32, 2, "even", {{WA_QS, 1, 1}, {WA_SC, 32, 2}}, 64 + 4, {WA_SC, 32, 2}},
    {WF_F16, "f16", WF_F16, RCA_F16, 1, 2, false, {{WA_W16, 1, 2}}, 1, 0, 0, "", {}, 128, {WA_W16, 1, 2}},
    {WF_Q4K, "Q4_K", WF_Q4K, RCA_Q4_K, 256, 144, false, WF_PLAIN_K, 256, 256, 4, "of 4", {{WA_QS, 2, 1}, {WA_SC, 32, 2}, {WA_DD, 256, 4}}, 32 + 4 + 1, {WA_DD, 256, 4}},
    // Q6_K: d holds the int8 scales per 16, dd the fp16 d per 256; packed with one f32 scale per row and 16 values
    {WF_Q6K, "Q6_K", WF_Q6K, RCA_Q6_K, 256, 210, false, {{WA_Q, 1, 1}, {WA_D, 16, 1}, {WA_DD, 256, 2}}, 256, 256, 2, "even", {{WA_QS, 1, 1}, {WA_SC, 16, 4}}, 64 + 16, {WA_SC, 16, 4}},
    {WF_Q5K, "Q5_K", WF_Q5K, RCA_Q5_K, 256, 176, false, WF_PLAIN_K, 256, 256, 4, "of 4", {{WA_QS, 2, 1}, {WA_SC, 32, 2}, {WA_DD, 256, 4}, {WA_QH, 8, 1}}, 32 + 8 + 4 + 1, {WA_DD, 256, 4}},
    {WF_Q40, "Q4_0", WF_Q40, RCA_Q4_0, 32, 18, true, WF_PLAIN_4BIT, 256, 256, 4, "of 4", WF_PACKED_4BIT, 32 + 8, {WA_SC, 32, 4}},
    {WF_Q41, "Q4_1", WF_Q40, RCA_Q4_1, 32, 20, true, WF_PLAIN_4BIT, 256, 256, 4, "of 4", WF_PACKED_4BIT, 32 + 8, {WA_SC, 32, 4}},
    {WF_IQ4, "IQ4_NL", WF_IQ4, RCA_IQ4_NL, 32, 18, true, WF_PLAIN_4BIT, 256, 256, 4, "of 4", WF_PACKED_4BIT, 32 + 8, {WA_SC, 32, 4}},
    {WF_IQ4XS, "IQ4_XS", WF_IQ4, RCA_IQ4_XS, 256, 136, true, WF_PLAIN_4BIT, 256, 256, 4, "of 4", WF_PACKED_4BIT, 32 + 8, {WA_SC, 32, 4}},
};
constexpr int WF_COUNT = sizeof(WF_TABLE) / sizeof(WF_TABLE[0]);
constexpr bool wf_table_in_id_order() {
    for (int i = 0; i < WF_COUNT; ++i)
        if (WF_TABLE[i].id != i) return false;
    return true;
}
static_assert(wf_table_in_id_order(), "WF_TABLE[id] is the row of format id");
constexpr bool wf_packed(int fmt) { return fmt >= 0 && fmt < WF_COUNT && WF_TABLE[fmt].k_mult != 0; }
// rca_lm_config_t::decode_weights: the format a 16-bit matrix is brought into at load (a matrix that arrived quantised stays what it is)
enum { DW_AS_SUPPLIED = 0, DW_Q8_0, DW_F16, DW_Q4_K, DW_Q5_K, DW_Q4_0, DW_Q4_1, DW_IQ4_NL, DW_COUNT };
constexpr int DW_FORMAT[DW_COUNT] = {-1, WF_Q8, WF_F16, WF_Q4K, WF_Q5K, WF_Q40, WF_Q41, WF_IQ4};
// minimum waves per SIMD asked of the register allocator.  The q8_0 bodies otherwise spread over 200+ registers (one wave per
// SIMD) although their live set is ~130: a streaming kernel wants the occupancy.
constexpr int gemv_min_waves(int Q, int R, int NIT, int M = 2) {
    if (!wf_packed(Q) || WF_TABLE[Q].device != Q) return 1;   // the packed forms the kernels are instantiated for
    if (M == 4 && NIT == 4) return 1;   // four rows x four chunks: 128 x values per lane beside the batch (group steps, wide FFN)
    return R * NIT >= 16 ? 2 : 4;
}
// the two helpers against the hand-written format lists they replaced, at every argument the kernels are instantiated with
constexpr bool wf_helpers_match_their_lists() {
    for (int Q = 0; Q <= 9; ++Q) {
        if (wf_packed(Q) != (Q == WF_Q8 || Q == WF_Q4K || Q == WF_Q6K || Q == WF_Q5K || Q == WF_Q40 || Q == WF_Q41 || Q == WF_IQ4 || Q == WF_IQ4XS)) return false;
        for (int R = 1; R <= 8; R *= 2)
            for (int NIT = 1; NIT <= 4; ++NIT)
                for (int M = 1; M <= 4; M *= 2) {
                    const int was = (Q != WF_Q8 && Q != WF_Q4K && Q != WF_Q6K && Q != WF_Q5K && Q != WF_Q40 && Q != WF_IQ4) ? 1 : ((M == 4 && NIT == 4) ? 1 : (R * NIT >= 16 ? 2 : 4));
                    if (gemv_min_waves(Q, R, NIT, M) != was) return false;
                }
    }
    return gemv_min_waves(WF_Q8, 4, 1) == 4 && !wf_packed(-1) && !wf_packed(WF_COUNT);
}
static_assert(wf_helpers_match_their_lists(), "wf_packed / gemv_min_waves changed value");
// ACT = 1 (rca_lm_set_act_format, packed formats only): the activations are quantised to q8_1 blocks -- 32 consecutive values, int8 +
// one scale, ggml's quantize_row_q8_1 restated: d = amax / 127, inv = d != 0 ? 1 / d : 0 (IEEE division), q = roundf(x * inv), scale used
// d_x = (float)(fp16 rne of d) -- and the products run on the signed byte dot (v_dot4c_i32_i8), llama.cpp's GPU mat-vec class:
//   q8_0:  val = fma(d_w * d_x, (float)sum q_w q_x, val)            Q6_K: the same with the f32 scale of the group of 16 for d_w
//   Q4_K:  val = fma(d1 * d_x, (float)sum q_w q_x, val); val = fma(-m1, d_x * (float)sum q_x, val)    (d1 = d * sc, m1 = dmin * m, exact)
// per 8-value chunk of the lane; the integer sums are exact, everything after them is the f32 reduction of the f32 path.  The
// quantiser runs INSIDE the GEMV (after the RMSNorm with PRO 1), once per workgroup, on the 8 * NIT * M values the lane holds anyway:
// the four chunks of a block sit in four consecutive lanes of one `it`, so amax is two quad DPP exchanges.  For that a wave's chunk
// range starts on a block boundary: cpw is rounded up to a multiple of 4 (K = 192: 8 / 8 / 8 / 0 chunks instead of 6 / 6 / 6 / 6).
// GRP = 1 (rca_lm_group_step): the M rows of the pass belong to DIFFERENT sessions that share the weights.  Whatever the body reads
// from the step state of "the" handle -- the KV position and cache of a row (EPI 2), which row of x is a session's last token and
// where its logits go (PRO 1 + EPI 0, the head) -- comes per row from a small device table instead; `stt` is not read.  The
// arithmetic of a row is untouched, so a row comes out with the bits its own session's pass would have given it.  The body is shared
// and always inlined: the GRP = 0 kernels below are, instruction for instruction, what they were before the table existed.
struct LmGroupRow {
    LmDevState* stt;         // the row's session: n_tokens = KV position of ITS first token of the pass
    f16_t* kc; f16_t* vc;    // that session's KV cache (layer 0) and its layer stride in elements (q8_0 cache: its fp16 ring, stride 0)
    float* dst;              // head rows: the session's logits buffer
    long kv_stride;
    int j;                   // index of the row inside its session's tokens of the pass
    int xrow;                // row of the activation buffer the slot reads (QKV: the slot itself; head: the session's last token)
    int n_ctx;
    int pos_mask;            // GemvRope::pos_mask of that session
};
struct GemvGroup {
    const LmGroupRow* rows; int layer;
};
template <int M, int NIT, int R, int PRO, int EPI, int Q, int ACT, int GRP>
__device__ __forceinline__ void lm_gemv_body(const LmDevState* __restrict__ stt, const bf16_t* __restrict__ W, const GemvQ8& q8,
                                             const float* __restrict__ x, int N, int K, float* __restrict__ y,
                                             int batches_per_wg, int ldy, const GemvPro& pro, const GemvRope& rope, const GemvGroup& grp) {
    static_assert(!GRP || (PRO == 1 && (EPI == 0 || EPI == 2)), "only the QKV projection and the head read per-session state");
    constexpr int V = R * M;
    static_assert(V % 4 == 0 && R % 2 == 0, "R * M must be a multiple of 4");
    __shared__ float kred[2][4][V];
    __shared__ float nred[M][4];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int tid = threadIdx.x;
    const int nchunk = K >> 3;
    constexpr bool QA = ACT == 1;
    static_assert(!QA || wf_packed(Q), "q8_1 activations go with the packed weight formats");
    const int cpw = QA ? ((((nchunk + 3) >> 2) + 3) & ~3) : (nchunk + 3) >> 2;   // chunks per wave (q8_1: whole 32-blocks)
    const int c0 = wave * cpw;
    const int cn = max(0, min(cpw, nchunk - c0));            // this wave's chunk count (<= 64 * NIT)
    const int n_batches = (N + R - 1) / R;
    const int b_beg = blockIdx.x * batches_per_wg;
    const int b_end = min(n_batches, b_beg + batches_per_wg);
    if (b_beg >= n_batches) return;   // never true for the grids launch_gemv_r builds; the peeled last batch below relies on it
    // slot r of batch b -> weight row
    auto row_of = [&](int b, int r) {
        if (EPI == 2) {   // slots (2s, 2s+1) = rows (d, d+32) of one head
            const int pair = b * (R / 2) + (r >> 1);
            return (pair >> 5) * 64 + (pair & 31) + 32 * (r & 1);
        }
        return b * R + r;
    };
    constexpr bool Q6 = Q == WF_Q6K;                 // the q8_0 body with another scale: f32 per group of 16 instead of fp16 per 32
    constexpr bool Q5 = Q == WF_Q5K;                 // the Q4_K body with a fifth bit per value; its plane of high bits arrives as W
    constexpr bool Q40 = Q == WF_Q40;                // Q4_0 / Q4_1: the Q4_K body with (s, t) read from one dword per slot and 32 values
    constexpr bool IQ4 = Q == WF_IQ4;                // IQ4_NL / IQ4_XS: the Q4_K nibble layout holds table indices, one f32 factor per slot and 32 values, no minimum
    constexpr bool Q8 = Q == WF_Q8 || Q6, Q4 = Q == WF_Q4K || Q5 || Q40 || IQ4;
    constexpr int NL = Q8 ? R / 2 : (Q4 ? R / 4 : R);   // 16-byte weight loads per chunk: one per row, per slot pair (q8_0 / Q6_K) or per slot quad (Q4_K)
    constexpr int H0 = NL / 2;                // the batch's registers refill in two halves: loads [0, H0) and [H0, NL)
    u32x4 wq[NL][NIT];
    constexpr bool Q4F = Q4 && !Q40 && !IQ4;  // the two-level factors of the K-quants
    uint2 wscm[Q4F ? NIT : 1][Q4F ? NL : 1];  // Q4_K: (sc | m << 8) of a quad's four slots for this lane's 32-element sub-block
    u32x4 wdd[Q4 ? NIT : 1][Q4 ? NL : 1];     //       (d | dmin << 16) of the four slots for this lane's 256-element super-block;
                                              //       Q4_0 / Q4_1: (s | t << 16) of the four slots for this lane's 32-element block;
                                              //       IQ4: the f32 factor s of the four slots for that block
    unsigned wqh[Q5 ? NL : 1][Q5 ? NIT : 1];  // Q5_K: the quad's dword of high bits for this lane's chunk
    unsigned wsc[Q8 ? NIT : 1][Q8 ? R / 2 : 1];   // q8_0: (fp16, fp16) scales of the batch's pairs for this lane's 32-element block
    unsigned wsc2[Q6 ? NIT : 1][Q6 ? R / 2 : 1];  // Q6_K: wsc / wsc2 = the f32 scales (bits) of the pair's first / second row for this lane's group of 16
    const int npairs = N >> 1;
    // Every lane loads from a VALID address, whatever its chunk: a lane past the wave's range (narrow test models) re-reads chunk 0
    // and multiplies it by x = 0.  A select or an exec mask on the loaded value would be a vector instruction on the load's
    // result, i.e. a wait for it right behind its issue -- and with it for every load issued before.
    const int cbase = cn > 0 ? c0 : 0;
    // weight loads of ONE row (bf16 / fp16) or row pair (q8_0) of batch b into its registers; the q8_0 scales of a batch separately
    auto issue_row = [&](int b, int r) {
        if (Q4) {   // quad r of the batch: factors first (consumed with the quad), then the nibbles
            const long quad = min((long)b * (R / 4) + r, (long)((N + 3) >> 2) - 1);
#pragma unroll
            for (int it = 0; it < NIT; ++it) {
                const int c = lane + 64 * it;
                const int cc = cbase + (c < cn ? c : 0);
                if constexpr (Q40 || IQ4) {
                    wdd[it][r] = *reinterpret_cast<const u32x4*>(q8.sc + q4k_scm_index(4 * quad, cc >> 2, K >> 5));
                } else {
                    wdd[it][r] = *reinterpret_cast<const u32x4*>(q8.dd + q4k_scm_index(4 * quad, cc >> 5, K >> 8));
                    wscm[it][r] = *reinterpret_cast<const uint2*>(reinterpret_cast<const unsigned short*>(q8.sc) + q4k_scm_index(4 * quad, cc >> 2, K >> 5));
                }
                wq[r][it] = __builtin_nontemporal_load(q8.qs + quad * nchunk + cc);
                if constexpr (Q5) wqh[r][it] = __builtin_nontemporal_load(reinterpret_cast<const unsigned*>(W) + quad * nchunk + cc);
            }
        } else if (Q8) {
            const long pp = min((long)b * (R / 2) + r, (long)npairs - 1);
#pragma unroll
            for (int it = 0; it < NIT; ++it) {
                const int c = lane + 64 * it;
                wq[r][it] = __builtin_nontemporal_load(q8.qs + pp * nchunk + cbase + (c < cn ? c : 0));
            }
        } else {
            const int row = min(row_of(b, r), N - 1);
            const u32x4* wr = reinterpret_cast<const u32x4*>(W + (long)row * K) + cbase;
#pragma unroll
            for (int it = 0; it < NIT; ++it) {
                const int c = lane + 64 * it;
                wq[r][it] = __builtin_nontemporal_load(wr + (c < cn ? c : 0));
            }
        }
    };
    // q8_0 scales of the pairs [s_beg, s_end) of batch b (a (fp16, fp16) dword per pair and 32-element block)
    auto issue_scales = [&](int b, int s_beg, int s_end) {
        if (!Q8) return;
        const long p0 = (long)b * (R / 2);
        if (Q6) {   // (s_a, s_b) floats per pair: two pairs per 16-byte load
#pragma unroll
            for (int it = 0; it < NIT; ++it) {
                const int c = lane + 64 * it;
                const int cc = cbase + (c < cn ? c : 0);
                const unsigned* sp = q8.sc + 2 * q8_sc_index(p0, cc >> 1, K >> 4);
#pragma unroll
                for (int s2 = 0; s2 < R / 2; s2 += 2) {
                    if (s2 < s_beg || s2 >= s_end) continue;
                    const u32x4 t = *reinterpret_cast<const u32x4*>(sp + 2 * s2);
                    wsc[it][s2] = t.x; wsc2[it][s2] = t.y; wsc[it][s2 + 1] = t.z; wsc2[it][s2 + 1] = t.w;
                }
            }
            return;
        }
#pragma unroll
        for (int it = 0; it < NIT; ++it) {
            const int c = lane + 64 * it;
            const int cc = cbase + (c < cn ? c : 0);
            const unsigned* sp = q8.sc + q8_sc_index(p0, cc >> 2, K >> 5);   // a batch never crosses a group of 8 pairs (R <= 16)
            // R = 16 only: four pairs per 16-byte load, one load per register half (groups are padded to 8 pairs: always in bounds and
            // aligned).  At R = 8 such a load would span BOTH halves: the refill of the first half for batch b + 1 then replaced the
            // scales of the second half of batch b before it was consumed ("Decode GEMVs alone"), so R = 8 loads per pair.
            if (R / 2 >= 8) {
#pragma unroll
                for (int s4 = 0; s4 < R / 8; ++s4) {
                    if (4 * s4 < s_beg || 4 * s4 >= s_end) continue;
                    const u32x4 t = *reinterpret_cast<const u32x4*>(sp + 4 * s4);
                    wsc[it][4 * s4 + 0] = t.x; wsc[it][4 * s4 + 1] = t.y; wsc[it][4 * s4 + 2] = t.z; wsc[it][4 * s4 + 3] = t.w;
                }
            } else {
#pragma unroll
                for (int s2 = 0; s2 < R / 2; ++s2)
                    if (s2 >= s_beg && s2 < s_end) wsc[it][s2] = sp[s2];
            }
        }
    };
    // half h (0 / 1) of batch b: its scales first (they are consumed with its first pair), then its rows
    auto load_half = [&](int b, int h) {
        issue_scales(b, h ? H0 : 0, h ? NL : H0);
#pragma unroll
        for (int r = 0; r < NL; ++r)
            if (h ? r >= H0 : r < H0) issue_row(b, r);
    };
    auto load_batch = [&](int b) { load_half(b, 0); load_half(b, 1); };
    // ---- this lane's x values.  Vector-memory results return in issue order, so the (short, L2-served) loads of x and of the
    // norm weights go out FIRST and the first batch of weight loads right behind them: the prologue below then waits for its own
    // operands only while the weights stay in flight under it.  (Issued the other way round, the first use of x would wait for
    // every weight load in front of it and the RMSNorm chain would run after the weights had landed instead of under them.)
    float xr[M][NIT][8];
    float nw[PRO == 1 ? NIT : 1][8];
    {
        int mbase = 0;
        if (!GRP && PRO == 1 && pro.only_last) mbase = stt->m - 1;
        const float* xsrc = PRO == 1 ? pro.xin : x;
#pragma unroll
        for (int m = 0; m < M; ++m)
#pragma unroll
            for (int it = 0; it < NIT; ++it) {
                const int c = lane + 64 * it;
                if (c < cn) {
                    const float* p = xsrc + (long)(GRP ? grp.rows[m].xrow : mbase + m) * K + (long)(c0 + c) * 8;
                    const float4 a = *reinterpret_cast<const float4*>(p);
                    const float4 b = *reinterpret_cast<const float4*>(p + 4);
                    xr[m][it][0] = a.x; xr[m][it][1] = a.y; xr[m][it][2] = a.z; xr[m][it][3] = a.w;
                    xr[m][it][4] = b.x; xr[m][it][5] = b.y; xr[m][it][6] = b.z; xr[m][it][7] = b.w;
                } else {
#pragma unroll
                    for (int j = 0; j < 8; ++j) xr[m][it][j] = 0.0f;
                }
            }
        if (PRO == 1) {
#pragma unroll
            for (int it = 0; it < NIT; ++it) {
                const int c = lane + 64 * it;
                if (c < cn) {
                    const float* p = pro.norm_w + (long)(c0 + c) * 8;
                    const float4 a = *reinterpret_cast<const float4*>(p);
                    const float4 b = *reinterpret_cast<const float4*>(p + 4);
                    nw[it][0] = a.x; nw[it][1] = a.y; nw[it][2] = a.z; nw[it][3] = a.w;
                    nw[it][4] = b.x; nw[it][5] = b.y; nw[it][6] = b.z; nw[it][7] = b.w;
                } else {
#pragma unroll
                    for (int j = 0; j < 8; ++j) nw[it][j] = 0.0f;
                }
            }
        }
        __builtin_amdgcn_sched_barrier(0);   // keep the issue order: x / norm weights, then the weight stream
        // unconditional (the grid never holds a workgroup without a batch): a branch here would join a path with and one without
        // loads in flight, and the compiler would wait for ALL of them at the join
        load_batch(min(b_beg, n_batches - 1));
        __builtin_amdgcn_sched_barrier(0);
        if (PRO == 1) {
#pragma unroll
            for (int m = 0; m < M; ++m) {
                float ss = 0.0f;
#pragma unroll
                for (int it = 0; it < NIT; ++it)
#pragma unroll
                    for (int j = 0; j < 8; ++j) ss = __builtin_fmaf(xr[m][it][j], xr[m][it][j], ss);
                ss = wave_sum(ss);
                if (lane == 0) nred[m][wave] = ss;
            }
            __syncthreads();
#pragma unroll
            for (int m = 0; m < M; ++m) {
                const float tot = ((nred[m][0] + nred[m][1]) + nred[m][2]) + nred[m][3];
                const float rstd = rsqrtf(tot / (float)K + pro.eps);
#pragma unroll
                for (int it = 0; it < NIT; ++it)
#pragma unroll
                    for (int j = 0; j < 8; ++j) xr[m][it][j] = (xr[m][it][j] * rstd) * nw[it][j];
            }
        }
    }
    int pos0 = 0;
    if (!GRP && EPI == 2) pos0 = stt->n_tokens;
    // grouped QKV: the epilogue thread of (row m, pair s) takes position, cache and context bound of row m's session
    int g_pos = 0, g_nctx = 0, g_mask = -1;
    f16_t *g_kc = nullptr, *g_vc = nullptr;
    float* g_dst = nullptr;
    if constexpr (GRP != 0) {
        if (EPI == 2 && tid < V / 2) {
            const LmGroupRow rw = grp.rows[tid / (R / 2)];
            g_pos = rw.stt->n_tokens + rw.j;
            g_nctx = rw.n_ctx;
            g_mask = rw.pos_mask;
            g_kc = rw.kc + (long)grp.layer * rw.kv_stride;
            g_vc = rw.vc + (long)grp.layer * rw.kv_stride;
        }
        if (EPI == 0 && tid < V) g_dst = grp.rows[tid / R].dst;
    }
    // q8_1 activations: this lane's chunks as int8 (two dwords; Q4_K: elements 0 2 4 6 / 1 3 5 7, the order its nibbles unpack in),
    // the block's fp16-rounded scale, and for Q4_K d_x * sum(q_x) of the chunk (the minimum term)
    unsigned xq[QA ? M : 1][QA ? NIT : 1][2];
    float xd[QA ? M : 1][QA ? NIT : 1];
    constexpr bool Q4M = Q4 && !IQ4;      // the forms with a minimum term
    float sx[Q4M ? M : 1][Q4M ? NIT : 1];   // Q4_K: sum of this lane's x values per chunk (the minimum term: - (dmin * m) * sum(x))
    if constexpr (QA) {
#pragma unroll
        for (int m = 0; m < M; ++m)
#pragma unroll
            for (int it = 0; it < NIT; ++it) {
                float amax = 0.0f;
#pragma unroll
                for (int j = 0; j < 8; ++j) amax = fmaxf(amax, fabsf(xr[m][it][j]));
                amax = fmaxf(amax, dpp_mov<DPP_XOR1>(amax));   // c0 and K / 8 are multiples of 4: a quad of lanes is one block,
                amax = fmaxf(amax, dpp_mov<DPP_XOR2>(amax));   // wholly inside the wave's range or wholly outside (x = 0 -> q = 0, d = 0)
                const float d = amax / 127.0f;
                const float inv = d != 0.0f ? 1.0f / d : 0.0f;
                unsigned qb[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) qb[j] = (unsigned)(int)roundf(xr[m][it][j] * inv) & 0xffu;
                if (Q4) {
                    xq[m][it][0] = qb[0] | (qb[2] << 8) | (qb[4] << 16) | (qb[6] << 24);
                    xq[m][it][1] = qb[1] | (qb[3] << 8) | (qb[5] << 16) | (qb[7] << 24);
                } else {
                    xq[m][it][0] = qb[0] | (qb[1] << 8) | (qb[2] << 16) | (qb[3] << 24);
                    xq[m][it][1] = qb[4] | (qb[5] << 8) | (qb[6] << 16) | (qb[7] << 24);
                }
                xd[m][it] = (float)(f16_t)d;
                if (Q4M) {
                    const int s = __builtin_amdgcn_sdot4((int)xq[m][it][1], 0x01010101, __builtin_amdgcn_sdot4((int)xq[m][it][0], 0x01010101, 0, false), false);
                    sx[m][it] = xd[m][it] * (float)s;
                }
            }
    } else if (Q4M) {
#pragma unroll
        for (int m = 0; m < M; ++m)
#pragma unroll
            for (int it = 0; it < NIT; ++it) {
                float t = 0.0f;
#pragma unroll
                for (int j = 0; j < 8; ++j) t = t + xr[m][it][j];
                sx[m][it] = t;
            }
    }

    // The weight registers of a batch are two halves that refill separately: while the second half of batch b is being consumed the
    // first half of batch b + 1 is already in flight, and the other way round -- at least R / 2 loads per lane are outstanding from
    // the first instruction to the last half.  (Batch-synchronous -- wait for all R rows, compute them, then ask for the next R --
    // left the CU's memory pipe idle for the length of a batch's arithmetic between batches.)  Rows are consumed in issue order, so
    // the waits count down row by row.  Finer refills (row by row) make this compiler keep the next batch in a second register set
    // and copy it over behind a vmcnt(0) at the loop end, or spill (two-arm form): measured in profiles/r03/experiments.
    auto consume_row = [&](float (&val)[V], int r) {
        if (Q4) {
#pragma unroll
            for (int it = 0; it < NIT; ++it) {
                const u32x4 a = wq[r][it];
                const u32x4 ddv = wdd[it][r];
                uint2 sm = make_uint2(0u, 0u);
                if constexpr (Q4F) sm = wscm[it][r];
                const unsigned aw[4] = {a.x, a.y, a.z, a.w}, dw[4] = {ddv.x, ddv.y, ddv.z, ddv.w}, sw[2] = {sm.x, sm.y};
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const unsigned w = q8_opaque(aw[i]);
                    if constexpr (IQ4) {   // kv bytes of nibbles 0, 2, 4, 6 / 1, 3, 5, 7; val += s sum kv[q_j] x_j, products in ascending j
                        const unsigned klo = iq4_map4<0>(w), khi = iq4_map4<4>(w);
                        const float s1 = __uint_as_float(dw[i]);
                        if constexpr (QA) {
#pragma unroll
                            for (int m = 0; m < M; ++m) {
                                const int p = __builtin_amdgcn_sdot4((int)khi, (int)xq[m][it][1], __builtin_amdgcn_sdot4((int)klo, (int)xq[m][it][0], 0, false), false);
                                val[m * R + 4 * r + i] = __builtin_fmaf(s1 * xd[m][it], (float)p, val[m * R + 4 * r + i]);
                            }
                        } else {
                            float fk[8];
                            fk[0] = sbyte_to_f32<0>(klo); fk[1] = sbyte_to_f32<0>(khi); fk[2] = sbyte_to_f32<1>(klo); fk[3] = sbyte_to_f32<1>(khi);
                            fk[4] = sbyte_to_f32<2>(klo); fk[5] = sbyte_to_f32<2>(khi); fk[6] = sbyte_to_f32<3>(klo); fk[7] = sbyte_to_f32<3>(khi);
#pragma unroll
                            for (int m = 0; m < M; ++m) {
                                float pk = 0.0f;
#pragma unroll
                                for (int j = 0; j < 8; ++j) pk = __builtin_fmaf(fk[j], xr[m][it][j], pk);
                                val[m * R + 4 * r + i] = __builtin_fmaf(s1, pk, val[m * R + 4 * r + i]);
                            }
                        }
                        continue;
                    }
                    unsigned lo = w & 0x0F0F0F0Fu, hi = (w >> 4) & 0x0F0F0F0Fu;   // bytes of lo = nibbles 0, 2, 4, 6; of hi = 1, 3, 5, 7
                    if constexpr (Q5) {   // bit 4 of every byte from the plane (q5k_hbit): slot i's even elements at bits 8 b + 2 i, odd at 8 b + 2 i + 1
                        const unsigned hb = wqh[r][it];
                        lo |= (i < 2 ? hb << (4 - 2 * i) : hb >> (2 * i - 4)) & 0x10101010u;
                        hi |= (i < 2 ? hb << (3 - 2 * i) : hb >> (2 * i - 3)) & 0x10101010u;
                    }
                    if constexpr (QA) {   // bytes 0..15 (Q5_K: 0..31) are valid signed int8: the signed byte dot against the activation bytes in the same order
                        const f16x2 d2 = __builtin_bit_cast(f16x2, dw[i]);
                        const unsigned scm = (sw[i >> 1] >> (16 * (i & 1))) & 0xffffu;
                        const float d1 = Q40 ? (float)d2[0] : (float)d2[0] * (float)(scm & 0xffu);   // Q4_0 / Q4_1: (s, t) as stored
                        const float m1 = Q40 ? (float)d2[1] : (float)d2[1] * (float)(scm >> 8);
#pragma unroll
                        for (int m = 0; m < M; ++m) {
                            const int p = __builtin_amdgcn_sdot4((int)hi, (int)xq[m][it][1], __builtin_amdgcn_sdot4((int)lo, (int)xq[m][it][0], 0, false), false);
                            float acc = val[m * R + 4 * r + i];
                            acc = __builtin_fmaf(d1 * xd[m][it], (float)p, acc);
                            acc = __builtin_fmaf(-m1, sx[m][it], acc);
                            val[m * R + 4 * r + i] = acc;
                        }
                        continue;
                    }
                    float pq[M];
#pragma unroll
                    for (int m = 0; m < M; ++m) pq[m] = 0.0f;
                    float fq[8];   // nibble j = byte j / 2 of lo (j even) / hi (j odd)
                    fq[0] = ubyte_to_f32<0>(lo); fq[1] = ubyte_to_f32<0>(hi); fq[2] = ubyte_to_f32<1>(lo); fq[3] = ubyte_to_f32<1>(hi);
                    fq[4] = ubyte_to_f32<2>(lo); fq[5] = ubyte_to_f32<2>(hi); fq[6] = ubyte_to_f32<3>(lo); fq[7] = ubyte_to_f32<3>(hi);
#pragma unroll
                    for (int j = 0; j < 8; ++j) {
#pragma unroll
                        for (int m = 0; m < M; ++m) pq[m] = __builtin_fmaf(fq[j], xr[m][it][j], pq[m]);
                    }
                    const f16x2 d2 = __builtin_bit_cast(f16x2, dw[i]);
                    const unsigned scm = (sw[i >> 1] >> (16 * (i & 1))) & 0xffffu;
                    const float d1 = Q40 ? (float)d2[0] : (float)d2[0] * (float)(scm & 0xffu);   // Q4_0 / Q4_1: (s, t) as stored
                    const float m1 = Q40 ? (float)d2[1] : (float)d2[1] * (float)(scm >> 8);
#pragma unroll
                    for (int m = 0; m < M; ++m) {
                        float acc = val[m * R + 4 * r + i];
                        acc = __builtin_fmaf(d1, pq[m], acc);
                        acc = __builtin_fmaf(-m1, sx[m][it], acc);
                        val[m * R + 4 * r + i] = acc;
                    }
                }
                __builtin_amdgcn_sched_barrier(0);   // one quad at a time (see the q8_0 branch)
            }
        } else if (Q8) {
#pragma unroll
            for (int it = 0; it < NIT; ++it) {
                const u32x4 a = wq[r][it];
                const unsigned wa[2] = {q8_opaque(a.x), q8_opaque(a.y)}, wb[2] = {q8_opaque(a.z), q8_opaque(a.w)};
                if constexpr (QA) {
                    const f16x2 d2 = __builtin_bit_cast(f16x2, wsc[it][r]);
                    const float da = Q6 ? __uint_as_float(wsc[it][r]) : (float)d2[0], db = Q6 ? __uint_as_float(wsc2[it][r]) : (float)d2[1];
#pragma unroll
                    for (int m = 0; m < M; ++m) {
                        const int ia = __builtin_amdgcn_sdot4((int)wa[1], (int)xq[m][it][1], __builtin_amdgcn_sdot4((int)wa[0], (int)xq[m][it][0], 0, false), false);
                        const int ib = __builtin_amdgcn_sdot4((int)wb[1], (int)xq[m][it][1], __builtin_amdgcn_sdot4((int)wb[0], (int)xq[m][it][0], 0, false), false);
                        val[m * R + 2 * r] = __builtin_fmaf(da * xd[m][it], (float)ia, val[m * R + 2 * r]);
                        val[m * R + 2 * r + 1] = __builtin_fmaf(db * xd[m][it], (float)ib, val[m * R + 2 * r + 1]);
                    }
                    __builtin_amdgcn_sched_barrier(0);   // one pair at a time, as below
                    continue;
                }
                float pa[M], pb[M];
#pragma unroll
                for (int m = 0; m < M; ++m) pa[m] = pb[m] = 0.0f;
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const float fa = q8_byte_to_f32(wa[j >> 2], j & 3);
                    const float fb = q8_byte_to_f32(wb[j >> 2], j & 3);
#pragma unroll
                    for (int m = 0; m < M; ++m) {
                        pa[m] = __builtin_fmaf(fa, xr[m][it][j], pa[m]);
                        pb[m] = __builtin_fmaf(fb, xr[m][it][j], pb[m]);
                    }
                }
                const f16x2 d2 = __builtin_bit_cast(f16x2, wsc[it][r]);
                const float da = Q6 ? __uint_as_float(wsc[it][r]) : (float)d2[0], db = Q6 ? __uint_as_float(wsc2[it][r]) : (float)d2[1];
#pragma unroll
                for (int m = 0; m < M; ++m) {
                    val[m * R + 2 * r] = __builtin_fmaf(da, pa[m], val[m * R + 2 * r]);
                    val[m * R + 2 * r + 1] = __builtin_fmaf(db, pb[m], val[m * R + 2 * r + 1]);
                }
                // one pair at a time: without the fence the scheduler converts the bytes of EVERY load in flight up front
                // (16 floats each) and the kernel drops to one wave per SIMD
                __builtin_amdgcn_sched_barrier(0);
            }
        } else {
#pragma unroll
            for (int it = 0; it < NIT; ++it) {
                const u32x4 a = wq[r][it];
                float f[8];
                if (Q == WF_F16) {   // fp16 weights: the widening is folded into v_fma_mix_f32 instead of a shift
                    const unsigned au[4] = {a.x, a.y, a.z, a.w};
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const f16x2 h2 = __builtin_bit_cast(f16x2, au[j]);
                        f[2 * j] = (float)h2[0];
                        f[2 * j + 1] = (float)h2[1];
                    }
                } else {
                    f[0] = bf16_lo(a.x); f[1] = bf16_hi(a.x); f[2] = bf16_lo(a.y); f[3] = bf16_hi(a.y);
                    f[4] = bf16_lo(a.z); f[5] = bf16_hi(a.z); f[6] = bf16_lo(a.w); f[7] = bf16_hi(a.w);
                }
#pragma unroll
                for (int m = 0; m < M; ++m)
#pragma unroll
                    for (int j = 0; j < 8; ++j) val[m * R + r] = __builtin_fmaf(f[j], xr[m][it][j], val[m * R + r]);
            }
        }
    };
    // One batch: `more` (compile-time) = another batch of this workgroup follows, and the registers of each half refill as soon as
    // the half has been consumed.  The loop below runs the batches that have a successor; the last one is peeled, so the refill
    // is unconditional inside the loop (no merge of "old" and "new" register contents for the compiler to copy around).
    auto run_batch = [&](int b, auto more_tag) {
        constexpr bool more = decltype(more_tag)::value;
        float val[V];   // value index v = m * R + r
#pragma unroll
        for (int v = 0; v < V; ++v) val[v] = 0.0f;
        // epilogue operands that do not depend on the sums: requested here, ahead of the next batch's weights in the (in-order) return
        // queue, so that waiting for them later does not mean waiting for those
        float yv = 0.0f, cs = 0.0f, sn = 0.0f;
        if (EPI == 3 && tid < V) {
            const int m = tid / R, row = row_of(b, tid % R);
            if (row < N) yv = y[(long)m * ldy + row];
        }
        if (EPI == 2 && tid < V / 2) {
            const int m = tid / (R / 2), s = tid % (R / 2);
            const int d = (b * (R / 2) + s) & 31;
            const long pos = GRP ? min(g_pos, g_nctx - 1) : min(pos0 + m, rope.n_ctx - 1);
            cs = rope.cos_t[pos * 32 + d];
            sn = rope.sin_t[pos * 32 + d];
        }
#if RCA_GEMV_VARIANT == 2
        {   // batch-synchronous (the round-2 structure), for A/B runs
#pragma unroll
            for (int r = 0; r < NL; ++r) consume_row(val, r);
            if (more) load_batch(b + 1);
        }
#else
#pragma unroll
        for (int r = 0; r < H0; ++r) consume_row(val, r);
        if (more) {
            load_half(b + 1, 0);
            // the second half's arithmetic does not depend on the refill above and would be scheduled in front of it (the refill
            // would then be requested only after the WHOLE batch has landed): one register of every row passes through a volatile
            // statement that sits behind the refill
#pragma unroll
            for (int r = H0; r < NL; ++r) asm volatile("" : "+v"(wq[r][0].x));
        }
#pragma unroll
        for (int r = H0; r < NL; ++r) consume_row(val, r);
        if (more) load_half(b + 1, 1);
#endif
        wave_reduce_transposed<V>(val);
        const int buf = (b - b_beg) & 1;
        if ((lane & 15) == 0) {
            const int q = lane >> 4;
#pragma unroll
            for (int i = 0; i < V / 4; ++i) kred[buf][wave][i + (V / 4) * (q & 1) + (V / 2) * (q >> 1)] = val[i];
        }
        __syncthreads();
        auto total = [&](int v) { return ((kred[buf][0][v] + kred[buf][1][v]) + kred[buf][2][v]) + kred[buf][3][v]; };
        if (EPI == 0 || EPI == 3) {
            if (tid < V) {
                const int m = tid / R, row = row_of(b, tid % R);
                if (GRP) { if (row < N) g_dst[row] = total(tid); }
                else if (row < N) y[(long)m * ldy + row] = EPI == 3 ? yv + total(tid) : total(tid);
            }
        } else if (EPI == 1) {
            if (tid < V / 2) {
                const int m = tid / (R / 2), s = tid % (R / 2);
                const int row = b * R + 2 * s;
                if (row + 1 < N) {
                    const float g = total(m * R + 2 * s), u = total(m * R + 2 * s + 1);
                    y[(long)m * ldy + (row >> 1)] = (g / (1.0f + __expf(-g))) * u;
                }
            }
        } else {
            if (tid < V / 2) {
                const int m = tid / (R / 2), s = tid % (R / 2);
                const int rl = row_of(b, 2 * s);             // row inside this matrix
                const int r0 = rl + rope.row_base;           // row inside [q; k; v]
                const int pos = GRP ? g_pos : pos0 + m;
                f16_t* const kcache = GRP ? g_kc : rope.kc;
                f16_t* const vcache = GRP ? g_vc : rope.vc;
                const int prow = pos & (GRP ? g_mask : rope.pos_mask);
                if (rl + 32 < N && pos < (GRP ? g_nctx : rope.n_ctx)) {
                    const float x1 = total(m * R + 2 * s), x2 = total(m * R + 2 * s + 1);
                    const int head = r0 >> 6, d = r0 & 63;   // d < 32
                    if (head < rope.nh + rope.nkv) {
                        const float o1 = x1 * cs + (-x2) * sn;
                        const float o2 = x2 * cs + x1 * sn;
                        if (head < rope.nh) {
                            y[(long)m * ldy + r0] = o1;
                            y[(long)m * ldy + r0 + 32] = o2;
                        } else {
                            f16_t* kp = kcache + ((long)prow * rope.nkv + (head - rope.nh)) * 64;
                            kp[d] = (f16_t)o1;
                            kp[d + 32] = (f16_t)o2;
                        }
                    } else {
                        f16_t* vp = vcache + ((long)prow * rope.nkv + (head - rope.nh - rope.nkv)) * 64;
                        vp[d] = (f16_t)x1;
                        vp[d + 32] = (f16_t)x2;
                    }
                }
            }
        }
    };
    for (int b = b_beg; b + 1 < b_end; ++b) run_batch(b, std::true_type{});
    run_batch(b_end - 1, std::false_type{});
}
template <int M, int NIT, int R, int PRO, int EPI, int Q = 0, int ACT = 0>
__global__ __launch_bounds__(256, gemv_min_waves(Q, R, NIT, M)) void lm_gemv_kernel(const LmDevState* __restrict__ stt, const bf16_t* __restrict__ W, GemvQ8 q8,
                                                      const float* __restrict__ x, int N, int K, float* __restrict__ y,
                                                      int batches_per_wg, int ldy, GemvPro pro, GemvRope rope) {
    // (argument order: the weight pointers of either form, x, N, K -- what the first loads need -- are the 14 dwords the dispatcher
    //  preloads into SGPRs)
    lm_gemv_body<M, NIT, R, PRO, EPI, Q, ACT, 0>(stt, W, q8, x, N, K, y, batches_per_wg, ldy, pro, rope, GemvGroup{nullptr, 0});
}
// the grouped QKV projection and head: the same first 14 dwords, the row table behind everything else
template <int M, int NIT, int R, int PRO, int EPI, int Q = 0, int ACT = 0>
__global__ __launch_bounds__(256, gemv_min_waves(Q, R, NIT, M)) void lm_gemv_group_kernel(const LmDevState* __restrict__ stt, const bf16_t* __restrict__ W, GemvQ8 q8,
                                                      const float* __restrict__ x, int N, int K, float* __restrict__ y,
                                                      int batches_per_wg, int ldy, GemvPro pro, GemvRope rope, GemvGroup grp) {
    lm_gemv_body<M, NIT, R, PRO, EPI, Q, ACT, 1>(stt, W, q8, x, N, K, y, batches_per_wg, ldy, pro, rope, grp);
}


// ------------------------------------------------------------------------- prefill: bf16 MFMA GEMM
// Prefill tiles (up to 32 tokens per pass) run the projections on v_mfma_f32_32x32x16_bf16: weights are bf16
// already; the f32 activations are split into bf16 hi + lo (x ~= hi + lo keeps ~16 mantissa bits), so every
// k step issues two MFMAs into one f32 accumulator.  A workgroup owns one 32-row x 32-token output tile, its 4
// waves split K and are summed in wave order through LDS (deterministic).  Fragments are loaded straight from
// global memory: A = 16 B of a weight row per lane, B = 16 B of a token row per lane.
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

__global__ __launch_bounds__(256) void lm_split_bf16_kernel(const LmDevState* __restrict__ stt, const float* __restrict__ x,
                                                            bf16_t* __restrict__ hi, bf16_t* __restrict__ lo, int K) {
    const int m = blockIdx.y;
    if (m >= stt->m) return;
    for (int k = blockIdx.x * 256 + threadIdx.x; k < K; k += gridDim.x * 256) {
        const float v = x[(long)m * K + k];
        const bf16_t h = f32_to_bf16_rne(v);
        const float r = v - __uint_as_float((unsigned)h << 16);
        hi[(long)m * K + k] = h;
        lo[(long)m * K + k] = f32_to_bf16_rne(r);
    }
}

#define GEMM_EPI_RESID 0
#define GEMM_EPI_ROPE 1
#define GEMM_EPI_SWIGLU 2
#define GEMM_EPI_LOGITS 3   // lm_gemm128_kernel only: the head of rca_lm_score, plain f32 stores into one token block's [128][V] scratch
#define GEMM_EPI_ROPE_ROWS 4   // lm_gemm128_kernel (+ its k-split epilogue) only: GEMM_EPI_ROPE whose token rows belong to DIFFERENT sessions
                               // (rca_lm_batch_step): position, K / V cache and context bound of a row come from an LmGroupRow table
template <int EPI>
__global__ __launch_bounds__(256) void lm_gemm_mfma_kernel(const LmDevState* __restrict__ stt, const bf16_t* __restrict__ W,
                                                           const bf16_t* __restrict__ xh, const bf16_t* __restrict__ xl, int N, int K,
                                                           float* __restrict__ y, int ldy, bf16_t* __restrict__ oh, bf16_t* __restrict__ ol,
                                                           GemvRope rope) {
    __shared__ float red[3][16][64];
    const int lane = threadIdx.x & 63;
    const int half = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int tile = blockIdx.x;
    const int Mv = stt->m;
    auto n_of = [&](int rr) {
        if (EPI == GEMM_EPI_ROPE) return (tile >> 1) * 64 + (rr >> 4) * 32 + (tile & 1) * 16 + (rr & 15);
        return tile * 32 + rr;
    };
    const int Kw = K >> 2;                     // this wave's K slice
    const int k0 = wave * Kw;
    const int nsteps = Kw >> 4;
    const bf16_t* wrow = W + (long)n_of(lane & 31) * K + k0 + 8 * half;
    const bf16_t* hrow = xh + (long)(lane & 31) * K + k0 + 8 * half;
    const bf16_t* lrow = xl + (long)(lane & 31) * K + k0 + 8 * half;
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
    constexpr int U = 4;
    uint4 a[U], bh[U], bl[U];
    auto load = [&](int s0) {
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int st = min(s0 + u, nsteps - 1);
            a[u] = *reinterpret_cast<const uint4*>(wrow + st * 16);
            bh[u] = *reinterpret_cast<const uint4*>(hrow + st * 16);
            bl[u] = *reinterpret_cast<const uint4*>(lrow + st * 16);
        }
    };
    load(0);
    for (int s0 = 0; s0 < nsteps; s0 += U) {
        uint4 ca[U], cbh[U], cbl[U];
#pragma unroll
        for (int u = 0; u < U; ++u) { ca[u] = a[u]; cbh[u] = bh[u]; cbl[u] = bl[u]; }
        if (s0 + U < nsteps) load(s0 + U);
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (s0 + u < nsteps) {
                const bf16x8 av = __builtin_bit_cast(bf16x8, ca[u]);
                acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(av, __builtin_bit_cast(bf16x8, cbh[u]), acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(av, __builtin_bit_cast(bf16x8, cbl[u]), acc, 0, 0, 0);
            }
        }
    }
    if (wave > 0) {
#pragma unroll
        for (int r = 0; r < 16; ++r) red[wave - 1][r][lane] = acc[r];
    }
    __syncthreads();
    if (wave != 0) return;
#pragma unroll
    for (int r = 0; r < 16; ++r) { acc[r] += red[0][r][lane]; acc[r] += red[1][r][lane]; acc[r] += red[2][r][lane]; }
    const int tok = lane & 31;
    if (tok >= Mv) return;
    if (EPI == GEMM_EPI_RESID) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int n = n_of((r & 3) + 8 * (r >> 2) + 4 * half);
            if (n < N) y[(long)tok * ldy + n] = y[(long)tok * ldy + n] + acc[r];
        }
    } else if (EPI == GEMM_EPI_ROPE) {
        const int pos = stt->n_tokens + tok;
        if (pos >= rope.n_ctx) return;
#pragma unroll
        for (int r = 0; r < 8; ++r) {   // registers r and r+8 hold rows d and d+32 of one head
            const int n1 = n_of((r & 3) + 8 * (r >> 2) + 4 * half);
            const int head = n1 >> 6, d = n1 & 63;   // d < 32
            const float x1 = acc[r], x2 = acc[r + 8];
            if (head < rope.nh + rope.nkv) {
                const float c = rope.cos_t[(long)pos * 32 + d], sn = rope.sin_t[(long)pos * 32 + d];
                const float o1 = x1 * c + (-x2) * sn;
                const float o2 = x2 * c + x1 * sn;
                if (head < rope.nh) {
                    y[(long)tok * ldy + n1] = o1;
                    y[(long)tok * ldy + n1 + 32] = o2;
                } else {
                    f16_t* kp = rope.kc + ((long)(pos & rope.pos_mask) * rope.nkv + (head - rope.nh)) * 64;
                    kp[d] = (f16_t)o1;
                    kp[d + 32] = (f16_t)o2;
                }
            } else {
                f16_t* vp = rope.vc + ((long)(pos & rope.pos_mask) * rope.nkv + (head - rope.nh - rope.nkv)) * 64;
                vp[d] = (f16_t)x1;
                vp[d + 32] = (f16_t)x2;
            }
        }
    } else {  // SwiGLU: rows (2i, 2i+1) = (gate_i, up_i) sit in registers (2j, 2j+1)
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int rr = ((2 * j) & 3) + 8 * ((2 * j) >> 2) + 4 * half;
            const int i = (tile * 32 + rr) >> 1;
            const float g = acc[2 * j], u = acc[2 * j + 1];
            const float hv = (g / (1.0f + __expf(-g))) * u;
            const bf16_t hb = f32_to_bf16_rne(hv);
            oh[(long)tok * ldy + i] = hb;
            ol[(long)tok * ldy + i] = f32_to_bf16_rne(hv - __uint_as_float((unsigned)hb << 16));
        }
    }
}

// advance the device-side KV position after a pass
__global__ void lm_advance_kernel(LmDevState* stt) { stt->n_tokens += stt->m; }
// steady-state step: next pass's first id is the token just sampled (realtime_agent_v2.py:355-363)
__global__ void lm_copy_logits_row_kernel(const float* __restrict__ src, float* __restrict__ dst, int V) {
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < V; i += gridDim.x * blockDim.x) dst[i] = src[i];
}

// --------------------------------------------------------------------------------- sampler
// Deterministic exp for x <= 0 (bit-identical to oracle/sampler_oracle.c): Cody-Waite reduction,
// degree-6 Horner in fma, exact ldexp.
__device__ __forceinline__ float rca_expf(float x) {
    if (x < -87.0f) return 0.0f;
    const float n = rintf(x * 1.44269504f);
    float r = __builtin_fmaf(n, -0.693359375f, x);
    r = __builtin_fmaf(n, 2.12194440e-4f, r);
    float p = 1.3888889e-3f;
    p = __builtin_fmaf(p, r, 8.3333333e-3f);
    p = __builtin_fmaf(p, r, 4.1666668e-2f);
    p = __builtin_fmaf(p, r, 1.6666667e-1f);
    p = __builtin_fmaf(p, r, 0.5f);
    p = __builtin_fmaf(p, r, 1.0f);
    p = __builtin_fmaf(p, r, 1.0f);
    return ldexpf(p, (int)n);
}
__device__ __forceinline__ unsigned long long splitmix(unsigned long long seed, unsigned long long ctr) {
    unsigned long long z = seed * 0x9E3779B97F4A7C15ull + ctr * 0xBF58476D1CE4E5B9ull + 0x94D049BB133111EBull;
    z ^= z >> 30; z *= 0xBF58476D1CE4E5B9ull;
    z ^= z >> 27; z *= 0x94D049BB133111EBull;
    z ^= z >> 31;
    return z;
}
// natural log of a positive normal float: cephes' logf polynomial as explicit fmas (the oracle's oracle_logf, bit for bit)
__device__ __forceinline__ float rca_logf(float x) {
    unsigned u = __float_as_uint(x);
    int e = (int)(u >> 23) - 127;
    float m = __uint_as_float((u & 0x007FFFFFu) | 0x3F800000u);
    if (m > 1.41421356f) { m = m * 0.5f; e += 1; }
    const float f = m - 1.0f;
    const float z = f * f;
    float y = 7.0376836292e-2f;
    y = __builtin_fmaf(y, f, -1.1514610310e-1f);
    y = __builtin_fmaf(y, f, 1.1676998740e-1f);
    y = __builtin_fmaf(y, f, -1.2420140846e-1f);
    y = __builtin_fmaf(y, f, 1.4249322787e-1f);
    y = __builtin_fmaf(y, f, -1.6668057665e-1f);
    y = __builtin_fmaf(y, f, 2.0000714765e-1f);
    y = __builtin_fmaf(y, f, -2.4999993993e-1f);
    y = __builtin_fmaf(y, f, 3.3333331174e-1f);
    y = y * f * z;
    const float fe = (float)e;
    y = __builtin_fmaf(fe, -2.12194440e-4f, y);
    y = __builtin_fmaf(z, -0.5f, y);
    float r = f + y;
    r = __builtin_fmaf(fe, 0.693359375f, r);
    return r;
}
// (value, index) as one unsigned key: larger value first, then the LOWER index.  -0.0 and +0.0 are one value (v + 0.0f turns the
// first into the second), so a tie between them ranks by index like any other tie; the logits the caller reads keep their signs.
__device__ __forceinline__ unsigned long long sample_key(float v, unsigned idx) {
    unsigned u = __float_as_uint(v + 0.0f);
    u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
    return ((unsigned long long)u << 32) | (unsigned long long)(0xFFFFFFFFu - idx);
}
// the float whose monotone image is the key's upper half (sample_key's inverse: same bits, NaN payloads included; a zero comes back as +0.0)
__device__ __forceinline__ float sample_key_value(unsigned long long key) {
    const unsigned u = (unsigned)(key >> 32);
    return __uint_as_float((u & 0x80000000u) ? (u & 0x7FFFFFFFu) : ~u);
}

// Sampler = three launches (llama.cpp chain order top_k -> top_p -> min_p -> temp -> softmax -> draw;
// llamacpp_utils.py:39-95; realtime_agent_config.py:11-20,29):
//   1. samp_hist:   2048-bin histogram of the monotone keys' top 11 bits (128 workgroups, LDS then global)
//   2. samp_gather: every workgroup finds the bin holding the k-th largest value from the histogram and
//                   appends its slice's elements at or above that bin to a candidate list (a few hundred)
//   3. samp_final:  one workgroup: exact top-k of the candidates by 8-bit radix select over 64-bit
//                   (value, index) keys, bitonic sort, then the serial chain with the polynomial exp and
//                   the counter RNG.  Falls back to scanning the whole vocabulary if the list overflowed.
#define SAMP_BINS 2048
#define SAMP_CAND_CAP 4096
#define SAMP_FAST_CAP 1024   // candidate lists up to this size are ranked by counting in samp_final_kernel
#define SAMP_RING 128          // accepted tokens kept (window <= 64 + the <= 8 speculative steps of a frame graph: a cut frame only rewinds the counter)
#define SAMP_OV_CAP 80         // logits patched in place per draw: <= 64 penalised + <= 8 biased
#define SAMP_LEVELS 6          // radix levels of the 64-bit (value, ~index) key: 11 + 11 + 11 + 11 + 11 + 9 bits
struct SampWork {
    unsigned hist[SAMP_BINS];
    unsigned ncand;
    unsigned overflow;
    unsigned pad[2];
    unsigned long long cand[SAMP_CAND_CAP];
    // ---- round 4
    int ring[SAMP_RING];                   // token accepted by draw c sits in ring[c % SAMP_RING] (c = LmDevState::rng_counter before the draw)
    int ov_n;                              // logits currently patched in place
    int ov_ids[SAMP_OV_CAP];
    float ov_orig[SAMP_OV_CAP];
    unsigned long long rhist[2][SAMP_LEVELS][SAMP_BINS];   // [0] rank (counts) / [1] mass (2^-40 fixed point) histograms of the radix selects
    unsigned long long rstate[2][SAMP_LEVELS][2];          // after level l: {key prefix fixed so far, what is still needed inside it}
    // ---- mirostat v2
    float mu_ring[SAMP_RING];              // mu BEFORE draw c sits in mu_ring[c % SAMP_RING]: draw c reads its slot and writes the next, so whatever
                                           // rewinds LmDevState::rng_counter rewinds mu with it (like `ring`, a cut frame only rewinds the counter)
    unsigned long long miro_part[2][64];   // per slice: [0] mass of the slice, [1] mass of its kept tokens (2^-40 fixed point)
};

// The value the sampler sees for token i.  Logit bias and penalties are NOT applied here any more: samp_prepare_kernel writes the
// adjusted values of the (at most 72) affected tokens into the logits row before the sampler's passes and the sampler's last kernel
// puts the originals back, so every pass is a plain read (llama.cpp applies both to its candidate copy, never to the context's
// logits: _ctx.get_logits() / _scores keep the raw values here too).
__device__ __forceinline__ float samp_value(const float* __restrict__ logits, const SamplerDev* __restrict__ sp, int i) {
    (void)sp;
    return logits[i];
}

// llama_sampler_penalties_apply on one logit (llama.cpp llama-sampling.cpp): a token seen `count` times in the window
__device__ __forceinline__ float samp_penalise(float v, int count, float repeat, float freq, float present) {
    if (count <= 0) return v;
    v = v <= 0.0f ? v * repeat : v / repeat;
    const float t = (float)count * freq + present;
    return v - t;
}

// One workgroup of 128 threads, in front of the sampler's passes when SamplerDev::patch is set: thread j < window takes the token
// accepted j draws ago, thread 64 + b bias entry b.  The first holder of a token owns it: bias entries in order (as the logits
// processor adds them, llamacpp_utils.py:8-24), then the penalty; the original goes to the override list, the adjusted value into
// the row.
// (The bodies of the four kernels of the serial chain are device functions, always inlined: the kernels of one handle pass their
// arguments through, the table kernels of rca_lm_batch_step -- one member per grid y -- read them from the member's table entry.
// A member's draw is the same instructions on the same operands either way.)
__device__ __forceinline__ void samp_prepare_body(float* __restrict__ logits, int V, const SamplerDev* __restrict__ sp,
                                                  const LmDevState* __restrict__ stt, SampWork* __restrict__ w) {
    __shared__ int tok[72];
    const int tid = threadIdx.x;
    const unsigned long long cnt = stt->rng_counter;
    const bool pen = sp->repeat_penalty != 1.0f || sp->freq_penalty != 0.0f || sp->presence_penalty != 0.0f;
    const int nwin = pen ? (int)min((unsigned long long)max(min(sp->last_n, 64), 0), cnt) : 0;
    const int nb = sp->n_bias;
    if (tid < 72) {
        int t = -1;
        if (tid < nwin) t = w->ring[(cnt - 1ull - (unsigned long long)tid) % SAMP_RING];
        else if (tid >= 64 && tid - 64 < nb) t = sp->bias_ids[tid - 64];
        tok[tid] = (t >= 0 && t < V) ? t : -1;
    }
    __syncthreads();
    if (tid < 72 && tok[tid] >= 0) {
        const int t = tok[tid];
        bool first = true;
        int count = 0;
        for (int q = 0; q < 72; ++q) {
            if (tok[q] != t) continue;
            if (q < tid) first = false;
            if (q < 64) ++count;
        }
        if (first) {
            const float orig = logits[t];
            float v = orig;
            for (int b = 0; b < nb; ++b)
                if (sp->bias_ids[b] == t) v = v + sp->bias_vals[b];
            v = samp_penalise(v, count, sp->repeat_penalty, sp->freq_penalty, sp->presence_penalty);
            const int slot = atomicAdd(&w->ov_n, 1);
            w->ov_ids[slot] = t;
            w->ov_orig[slot] = orig;
            logits[t] = v;
        }
    }
}
// the sampler's last kernel: the token just drawn joins the window, the patched logits get their values back
__device__ __forceinline__ void samp_accept_and_restore(float* __restrict__ logits, const SamplerDev* __restrict__ sp, SampWork* __restrict__ w,
                                                        unsigned long long draw, int tok, int tid) {
    if (tid == 0) w->ring[draw % SAMP_RING] = tok;
    if (sp->patch) {
        const int n = w->ov_n;
        if (tid < n) logits[w->ov_ids[tid]] = w->ov_orig[tid];
        __syncthreads();
        if (tid == 0) w->ov_n = 0;
    }
}
__device__ __forceinline__ int samp_k(const SamplerDev* sp, int V) {
    int k = sp->temp <= 0.0f ? 1 : sp->top_k;
    if (k <= 0 || k > SAMP_MAXK) k = SAMP_MAXK;
    return k > V ? V : k;
}

__global__ __launch_bounds__(128) void samp_prepare_kernel(float* __restrict__ logits, int V, const SamplerDev* __restrict__ sp,
                                                           const LmDevState* __restrict__ stt, SampWork* __restrict__ w) {
    samp_prepare_body(logits, V, sp, stt, w);
}

__device__ __forceinline__ void samp_hist_body(const float* __restrict__ logits, int V, const SamplerDev* __restrict__ sp,
                                               SampWork* __restrict__ w) {
    __shared__ unsigned hl[SAMP_BINS];
    for (int b = threadIdx.x; b < SAMP_BINS; b += 256) hl[b] = 0;
    __syncthreads();
    for (int i = blockIdx.x * 256 + threadIdx.x; i < V; i += gridDim.x * 256) {
        const unsigned long long key = sample_key(samp_value(logits, sp, i), (unsigned)i);
        atomicAdd(&hl[(unsigned)(key >> 53)], 1u);
    }
    __syncthreads();
    for (int b = threadIdx.x; b < SAMP_BINS; b += 256)
        if (hl[b]) atomicAdd(&w->hist[b], hl[b]);
}

__global__ __launch_bounds__(256) void samp_hist_kernel(const float* __restrict__ logits, int V, const SamplerDev* __restrict__ sp,
                                                        SampWork* __restrict__ w) {
    samp_hist_body(logits, V, sp, w);
}

__device__ __forceinline__ void samp_gather_body(const float* __restrict__ logits, int V, const SamplerDev* __restrict__ sp,
                                                 SampWork* __restrict__ w) {
    __shared__ unsigned wtot[4];
    __shared__ unsigned thr_bin;
    const int k = samp_k(sp, V);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    // The bin that holds the k-th largest value: the highest bin b with count(bins >= b) >= k, found as "group of 8 bins, then bin"
    // from the top.  Thread t owns bins 8 t .. 8 t + 7; S[t] = count of the bins of threads >= t is a suffix scan over the 256
    // threads (shuffles inside a wave + four wave totals), and the one thread whose group crosses k finishes inside its own
    // registers.  (One thread walking the 256 group sums and then 8 bins -- dependent LDS and global reads in a loop with an early
    // exit -- was ~7 of this kernel's 10 us.)  Unsigned integer sums: the same bin whatever the order.
    unsigned h8[8];
    {
        const uint4 a = *reinterpret_cast<const uint4*>(w->hist + tid * 8), b = *reinterpret_cast<const uint4*>(w->hist + tid * 8 + 4);
        h8[0] = a.x; h8[1] = a.y; h8[2] = a.z; h8[3] = a.w; h8[4] = b.x; h8[5] = b.y; h8[6] = b.z; h8[7] = b.w;
    }
    const unsigned s8 = ((h8[0] + h8[1]) + (h8[2] + h8[3])) + ((h8[4] + h8[5]) + (h8[6] + h8[7]));
    unsigned suf = s8;   // inclusive suffix sum over the lanes >= lane of this wave
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const unsigned o = __shfl_down(suf, off);
        if (lane + off < 64) suf += o;
    }
    if (lane == 0) wtot[wave] = suf;
    __syncthreads();
    unsigned S = suf;
    for (int q = wave + 1; q < 4; ++q) S += wtot[q];
    // group g = the highest t >= 1 with S[t] >= k, or 0; the counts above it: S[t + 1] = S[t] - s8
    const unsigned above = S - s8;
    const bool mine = tid >= 1 ? (S >= (unsigned)k && above < (unsigned)k) : (above < (unsigned)k);
    if (mine) {
        unsigned acc = above;
        int j = 7;
        for (; j > 0; --j) {
            if (acc + h8[j] >= (unsigned)k) break;
            acc += h8[j];
        }
        thr_bin = (unsigned)(tid * 8 + j);
    }
    __syncthreads();
    const unsigned tb = thr_bin;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < V; i += gridDim.x * 256) {
        const unsigned long long key = sample_key(samp_value(logits, sp, i), (unsigned)i);
        if ((unsigned)(key >> 53) >= tb) {
            const unsigned slot = atomicAdd(&w->ncand, 1u);
            if (slot < SAMP_CAND_CAP) w->cand[slot] = key;
            else w->overflow = 1u;
        }
    }
}

__global__ __launch_bounds__(256) void samp_gather_kernel(const float* __restrict__ logits, int V, const SamplerDev* __restrict__ sp,
                                                          SampWork* __restrict__ w) {
    samp_gather_body(logits, V, sp, w);
}

// Inside a frame graph samp_final_kernel's tail also does what a one-thread "next pair" launch and the next step's embedding launch
// did: record the token, advance the position, make [token, user id of this frame] the next pair and gather their embedding rows
// into x (two launches less per step of a frame).  (One launch for the WHOLE sampler -- histogram, last-arriver gather + selection --
// was built and measured: the single workgroup that then scans the 1 MB of logits for candidates is bound by one CU's memory pipe,
// 0.917 -> 0.996 ms per step: profiles/r03/experiments/one_launch_sampler.txt.)
struct SampTail {
    int frame_i;          // >= 0: step i of a frame graph (advance + next pair + embedding); -1: plain sample
    const void* table;    // embedding table
    int f32tab;
    float* x;
    int H;
};
// llama.cpp's locally typical sampler (llama_sampler_typical_apply) between top_k and top_p, restated in float32 over the cnt sorted
// candidates of the serial chain (tests/samp_ext_ref.py is the definition; parity with llama.cpp is not pinned).  With
// d_i = v_i - v_0, e_i = rca_expf(d_i), tot = e_0 + e_1 + ... (serial, in rank order) and L = rca_logf(tot):
//   -ln p_i = L - d_i (no logarithm of a small p),  p_i = e_i * (1 / tot),  H = sum of p_i * (L - d_i) (serial, in rank order),
//   s_i = |(L - d_i) - H|.  A candidate with e_i == 0 (a -inf logit, or d_i < -87) adds nothing to H and has s_i = +inf.
// Order by (s ascending, rank ascending) -- a counting rank -- and keep the shortest prefix whose serial sum of e exceeds
// typical_p * tot.  The survivors go on in logit order as a fresh candidate list: both exponentials are taken again relative to the
// survivors' maximum (llama.cpp's re-sort and softmax inside top_p), so top_p sees their total mass and min_p their best token.
// Called by every thread of the workgroup; returns the number of survivors (cnt when the cut is off).  No product feeds a sum inside
// one expression, and contraction is off, so that the restatement's single float32 operations are these.
__device__ __forceinline__ int samp_typical_cut(const SamplerDev* __restrict__ sp, int cnt, unsigned long long* cand, float* cval, float* e_plain,
                                                float* e_temp) {
#pragma clang fp contract(off)
    __shared__ float t_nl[SAMP_MAXK], t_term[SAMP_MAXK], t_s[SAMP_MAXK];
    __shared__ int t_order[SAMP_MAXK], t_keep[SAMP_MAXK];
    __shared__ float t_tot, t_H;
    __shared__ int t_cnt;
    const int tid = threadIdx.x;
    const float typ = sp->typical_p;
    if (!(sp->temp > 0.0f) || cnt <= 1 || !(typ > 0.0f && typ < 1.0f)) return cnt;
    if (tid == 0) {
        float tot = 0.0f;
        for (int i = 0; i < cnt; ++i) tot += e_plain[i];
        t_tot = tot;
    }
    __syncthreads();
    const float tot = t_tot, L = rca_logf(tot), inv = 1.0f / tot;
    if (tid < cnt) {
        const float e = e_plain[tid];
        const float nl = L - (cval[tid] - cval[0]);
        const float p = e * inv;
        t_nl[tid] = nl;
        t_term[tid] = e > 0.0f ? p * nl : 0.0f;
    }
    __syncthreads();
    if (tid == 0) {
        float H = 0.0f;
        for (int i = 0; i < cnt; ++i) H += t_term[i];
        t_H = H;
    }
    __syncthreads();
    if (tid < cnt) { t_s[tid] = e_plain[tid] > 0.0f ? fabsf(t_nl[tid] - t_H) : INFINITY; t_keep[tid] = 0; }
    __syncthreads();
    if (tid < cnt) {
        const float si = t_s[tid];
        int rank = 0;
        for (int j = 0; j < cnt; ++j) rank += (t_s[j] < si || (t_s[j] == si && j < tid)) ? 1 : 0;
        t_order[rank] = tid;
    }
    __syncthreads();
    if (tid == 0) {
        const float need = typ * tot;
        float cum = 0.0f;
        for (int r = 0; r < cnt; ++r) {
            const int i = t_order[r];
            cum += e_plain[i];
            t_keep[i] = 1;
            if (cum > need) break;
        }
        int m = 0;
        for (int i = 0; i < cnt; ++i)
            if (t_keep[i]) { cand[m] = cand[i]; cval[m] = cval[i]; ++m; }
        t_cnt = m;
    }
    __syncthreads();
    const int m = t_cnt;
    if (tid < m) {
        const float d = cval[tid] - cval[0];
        e_plain[tid] = rca_expf(d);
        e_temp[tid] = rca_expf(d * (1.0f / sp->temp));
    }
    __syncthreads();
    return m;
}
// TYP: the instance behind samp_final_typ_kernel, which a handle launches only with rca_lm_sampler_set_typical in force; the <false>
// instance holds no trace of the typical cut.
template <bool TYP>
__device__ __forceinline__ void samp_final_body(float* logits, int V, const SamplerDev* __restrict__ sp,
                                                LmDevState* __restrict__ stt, SampWork* __restrict__ w, const SampTail& tail) {
    __shared__ unsigned long long s_draw;
    __shared__ unsigned hist[256];
    __shared__ unsigned long long sel_prefix;
    __shared__ int sel_shift;      // bits already fixed (from the top)
    __shared__ unsigned need;      // how many more keys to take inside the current prefix bucket
    __shared__ unsigned long long cand[SAMP_MAXK];
    __shared__ unsigned ncand;
    __shared__ float cval[SAMP_MAXK];
    const int tid = threadIdx.x;
    const bool greedy = sp->temp <= 0.0f;
    const int k = samp_k(sp, V);
    // (requested together with the two counters it would otherwise wait for: slot tid exists whatever the count, SAMP_CAND_CAP >= 1024)
    const unsigned long long my_cand = w->cand[tid];
    const bool full = w->overflow != 0u;
    const int NN = full ? V : (int)min(w->ncand, (unsigned)SAMP_CAND_CAP);
    auto key_at = [&](int i) -> unsigned long long {
        return full ? sample_key(samp_value(logits, sp, i), (unsigned)i) : w->cand[i];
    };
    __shared__ unsigned long long ck[SAMP_FAST_CAP];
    __shared__ float e_plain[SAMP_MAXK], e_temp[SAMP_MAXK];
    __shared__ int s_tok;
    int n;
    if (!full && NN <= SAMP_FAST_CAP) {
        // the usual case, a few hundred candidates: every thread ranks its own key by counting the larger ones
        // (keys are unique), the k best land in sorted order -- two barriers instead of a radix select, a compaction
        // and a bitonic sort
        if (tid < NN) ck[tid] = my_cand;
        __syncthreads();
        if (tid < NN) {
            const unsigned long long key = ck[tid];
            int rank = 0;
#pragma unroll 8
            for (int j = 0; j < NN; ++j) rank += ck[j] > key ? 1 : 0;
            if (rank < SAMP_MAXK) cand[rank] = key;
        }
        __syncthreads();
        n = min(NN, SAMP_MAXK);
    } else {
        if (tid == 0) { sel_prefix = 0ull; sel_shift = 0; need = (unsigned)min(k, NN); ncand = 0; }
        __syncthreads();
        // radix select: afterwards the keys >= threshold are exactly the k largest
        for (int pass = 0; pass < 8; ++pass) {
            if (tid < 256) hist[tid] = 0;
            __syncthreads();
            const int shift = 56 - 8 * pass;
            const unsigned long long prefix = sel_prefix;
            const int fixed = sel_shift;
            for (int i = tid; i < NN; i += 1024) {
                const unsigned long long key = key_at(i);
                const bool match = fixed == 0 ? true : ((key >> (64 - fixed)) == (prefix >> (64 - fixed)));
                if (match) atomicAdd(&hist[(unsigned)(key >> shift) & 255u], 1u);
            }
            __syncthreads();
            if (tid == 0) {
                unsigned acc = 0;
                int d = 255;
                for (; d > 0; --d) {
                    if (acc + hist[d] >= need) break;
                    acc += hist[d];
                }
                need -= acc;  // keys in higher digits are all taken
                sel_prefix = prefix | ((unsigned long long)d << shift);
                sel_shift = fixed + 8;
                if (hist[d] == need) need = 0xFFFFFFFFu;  // whole bucket taken: threshold fixed, stop refining
            }
            __syncthreads();
            if (need == 0xFFFFFFFFu) break;
        }
        const unsigned long long thr = sel_prefix;  // unfixed low bits are zero
        for (int i = tid; i < NN; i += 1024) {
            const unsigned long long key = key_at(i);
            if (key >= thr) {
                const unsigned slot = atomicAdd(&ncand, 1u);
                if (slot < SAMP_MAXK) cand[slot] = key;
            }
        }
        __syncthreads();
        n = min((int)ncand, SAMP_MAXK);
        if (tid < SAMP_MAXK && tid >= n) cand[tid] = 0ull;
        __syncthreads();
        for (int size = 2; size <= SAMP_MAXK; size <<= 1) {  // bitonic sort, descending; padding (0) sinks
            for (int stride = size >> 1; stride > 0; stride >>= 1) {
                if (tid < SAMP_MAXK) {
                    const int j = tid ^ stride;
                    if (j > tid) {
                        const unsigned long long a = cand[tid], b = cand[j];
                        const bool desc = (tid & size) == 0;
                        if (desc ? (a < b) : (a > b)) { cand[tid] = b; cand[j] = a; }
                    }
                }
                __syncthreads();
            }
        }
    }
    if (tid < n) cval[tid] = sample_key_value(cand[tid]);   // the key's upper half IS the value (the bits samp_value read at gather time)
    __syncthreads();
    if (tid < n && !greedy) {   // the exponentials in parallel; the sums below stay serial (their order is the definition)
        const float mx = cval[0];
        e_plain[tid] = rca_expf(cval[tid] - mx);
        e_temp[tid] = rca_expf((cval[tid] - mx) * (1.0f / sp->temp));
    }
    __syncthreads();
    int typ_cnt = 0;
    if constexpr (TYP) typ_cnt = samp_typical_cut(sp, min(n, k), cand, cval, e_plain, e_temp);
    if (tid == 0) {
        int cnt = TYP ? typ_cnt : min(n, k);
        int pick = 0;
        if (!greedy && cnt > 1) {
            if (sp->top_p < 1.0f) {  // smallest prefix whose probability mass reaches top_p
                float tot = 0.0f;
                for (int i = 0; i < cnt; ++i) tot += e_plain[i];
                float cum = 0.0f;
                int keep = cnt;
                for (int i = 0; i < cnt; ++i) {
                    cum += e_plain[i];
                    if (cum >= sp->top_p * tot) { keep = i + 1; break; }
                }
                cnt = keep;
            }
            if (sp->min_p > 0.0f) {  // keep p_i >= min_p * p_max
                int keep = 1;
                for (int i = 1; i < cnt; ++i)
                    if (e_plain[i] >= sp->min_p) keep = i + 1; else break;
                cnt = keep;
            }
            float tot = 0.0f;
            for (int i = 0; i < cnt; ++i) tot += e_temp[i];
            const unsigned long long z = splitmix(sp->seed, stt->rng_counter);
            const float u = (float)(unsigned)(z >> 40) * 5.9604644775390625e-08f;  // 2^-24
            const float target = u * tot;
            float cum = 0.0f;
            pick = cnt - 1;
            for (int i = 0; i < cnt; ++i) {
                cum += e_temp[i];
                if (cum > target) { pick = i; break; }
            }
        }
        const int tok = (int)(0xFFFFFFFFu - (unsigned)(cand[pick] & 0xFFFFFFFFull));
        s_draw = stt->rng_counter;
        stt->rng_counter += 1ull;
        stt->out_token = tok;
        if (tail.frame_i >= 0) {   // the pair just evaluated is in the cache; the next pair is [token just sampled, user's token of this frame]
            stt->frame_out[tail.frame_i] = tok;
            stt->n_tokens += 2;
            stt->ids[0] = tok;
            stt->ids[1] = stt->ids[LM_FRAME_USER0 + tail.frame_i];
        }
        s_tok = tok;
    }
    // re-arm the shared work area for the next call
    __syncthreads();
    samp_accept_and_restore(logits, sp, w, s_draw, s_tok, tid);
    for (int b = tid; b < SAMP_BINS; b += 1024) w->hist[b] = 0u;
    if (tid == 0) { w->ncand = 0u; w->overflow = 0u; }
    if (tail.frame_i >= 0) {   // lm_embed_kernel for the next pair (m = 2)
        const int id1 = stt->ids[LM_FRAME_USER0 + tail.frame_i];
        for (int e = tid; e < 2 * tail.H; e += 1024) {
            const int m = e / tail.H, hh = e - m * tail.H;
            int id = m == 0 ? s_tok : id1;
            id = id < 0 ? 0 : (id >= V ? V - 1 : id);
            tail.x[e] = tail.f32tab ? reinterpret_cast<const float*>(tail.table)[(long)id * tail.H + hh]
                                    : __uint_as_float((unsigned)reinterpret_cast<const bf16_t*>(tail.table)[(long)id * tail.H + hh] << 16);
        }
    }
}
__global__ __launch_bounds__(1024) void samp_final_kernel(float* logits, int V, const SamplerDev* __restrict__ sp,
                                                          LmDevState* __restrict__ stt, SampWork* __restrict__ w, SampTail tail) {
    samp_final_body<false>(logits, V, sp, stt, w, tail);
}

// ---- top_k <= 0: llama.cpp's "whole vocabulary" (its top-k sampler is then a no-op; llamacpp_utils.py:39-77 passes top_k straight
// through).  With top_p >= 1 the chain is min_p -> temp -> softmax -> draw over every token, and that draw is made by the Gumbel-max
// rule: token = argmax_i (v_i - max) / temp + g_i over the tokens that pass min_p, g_i = -log(-log(u_i)), u_i from the counter RNG
// keyed by (seed, draw, token).  Same distribution, no sort of 259 k candidates, one pass; ties go to the lowest index.  Three launches
// like the top-k sampler: slice maxima, slice winners, merge + the sampler tail.  (top_k <= 0 with top_p < 1 is refused at init.)
#define SAMPF_SLICES 64
__global__ __launch_bounds__(1024) void samp_full_max_kernel(const float* __restrict__ logits, int V, const SamplerDev* __restrict__ sp,
                                                             SampWork* __restrict__ w) {
    __shared__ float red[16];
    const int per = (V + SAMPF_SLICES - 1) / SAMPF_SLICES;
    const int i0 = blockIdx.x * per, i1 = min(V, i0 + per);
    float mx = -INFINITY;
    for (int i = i0 + threadIdx.x; i < i1; i += 1024) mx = fmaxf(mx, samp_value(logits, sp, i));
    mx = wave_max(mx);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = mx;
    __syncthreads();
    if (threadIdx.x == 0) {
        float m = red[0];
        for (int k = 1; k < 16; ++k) m = fmaxf(m, red[k]);
        reinterpret_cast<float*>(w->hist)[blockIdx.x] = m;     // the histogram area is free in this mode (and re-zeroed by the merge)
    }
}
__global__ __launch_bounds__(1024) void samp_full_pick_kernel(const float* __restrict__ logits, int V, const SamplerDev* __restrict__ sp,
                                                              const LmDevState* __restrict__ stt, SampWork* __restrict__ w) {
    __shared__ unsigned long long red[16];
    const float* smax = reinterpret_cast<const float*>(w->hist);
    float mx = smax[0];
    for (int k = 1; k < SAMPF_SLICES; ++k) mx = fmaxf(mx, smax[k]);
    const float inv_t = 1.0f / sp->temp, min_p = sp->min_p;
    const unsigned long long draw = splitmix(sp->seed, stt->rng_counter);
    const int per = (V + SAMPF_SLICES - 1) / SAMPF_SLICES;
    const int i0 = blockIdx.x * per, i1 = min(V, i0 + per);
    unsigned long long best = 0ull;   // below every real key (a real key has bit 63 or bits of ~u set... see sample_key: never 0 with idx < 2^32 - 1)
    for (int i = i0 + threadIdx.x; i < i1; i += 1024) {
        const float d = samp_value(logits, sp, i) - mx;
        if (min_p > 0.0f && !(rca_expf(d) >= min_p)) continue;
        const unsigned long long z = splitmix(draw, (unsigned long long)i);
        const float u = (float)(unsigned)(((z >> 41) << 1) | 1ull) * 5.9604644775390625e-08f;
        const float g = -rca_logf(-rca_logf(u));
        const unsigned long long key = sample_key(__builtin_fmaf(d, inv_t, g), (unsigned)i);
        best = key > best ? key : best;
    }
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned long long o = __shfl_xor(best, off);
        best = o > best ? o : best;
    }
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = best;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long b = red[0];
        for (int k = 1; k < 16; ++k) b = red[k] > b ? red[k] : b;
        w->cand[blockIdx.x] = b;
    }
}
__global__ __launch_bounds__(1024) void samp_full_final_kernel(float* logits, int V, const SamplerDev* __restrict__ sp, LmDevState* __restrict__ stt,
                                                               SampWork* __restrict__ w, SampTail tail) {
    __shared__ int s_tok;
    __shared__ unsigned long long s_draw;
    const int tid = threadIdx.x;
    if (tid == 0) {
        unsigned long long b = w->cand[0];
        for (int k = 1; k < SAMPF_SLICES; ++k) b = w->cand[k] > b ? w->cand[k] : b;
        const int tok = (int)(0xFFFFFFFFu - (unsigned)(b & 0xFFFFFFFFull));
        s_draw = stt->rng_counter;
        stt->rng_counter += 1ull;
        stt->out_token = tok;
        if (tail.frame_i >= 0) {
            stt->frame_out[tail.frame_i] = tok;
            stt->n_tokens += 2;
            stt->ids[0] = tok;
            stt->ids[1] = stt->ids[LM_FRAME_USER0 + tail.frame_i];
        }
        s_tok = tok;
    }
    __syncthreads();
    samp_accept_and_restore(logits, sp, w, s_draw, s_tok, tid);
    for (int b = tid; b < SAMPF_SLICES; b += 1024) w->hist[b] = 0u;   // the top-k sampler expects a zeroed histogram
    if (tail.frame_i >= 0) {   // lm_embed_kernel for the next pair (m = 2), as in samp_final_kernel
        const int id1 = stt->ids[LM_FRAME_USER0 + tail.frame_i];
        for (int e = tid; e < 2 * tail.H; e += 1024) {
            const int m = e / tail.H, hh = e - m * tail.H;
            int id = m == 0 ? s_tok : id1;
            id = id < 0 ? 0 : (id >= V ? V - 1 : id);
            tail.x[e] = tail.f32tab ? reinterpret_cast<const float*>(tail.table)[(long)id * tail.H + hh]
                                    : __uint_as_float((unsigned)reinterpret_cast<const bf16_t*>(tail.table)[(long)id * tail.H + hh] << 16);
        }
    }
}

// ---- The "big" path (round 4): top_k > SAMP_MAXK (a rank cut anywhere up to the vocabulary) and / or top_p < 1 without a small top_k
// (llamacpp_utils.py:39-77 hands both straight to llama.cpp; realtime_agent_config.py:11-13).  llama.cpp sorts the candidates and
// walks the sorted list; here the two cuts are THRESHOLD KEYS found by radix selects over the 64-bit (value, ~index) keys of the whole
// vocabulary -- 11 + 11 + 11 + 11 + 11 + 9 bits, one pass per level, 2048-bin histograms:
//   rank cut:  the top_k-th largest key T_k (histograms of counts);
//   mass cut:  the key T_p at which the mass of the keys above it first reaches top_p of the candidates' total, walking down from
//              the top (histograms of mass; the candidates are the keys >= T_k).  Masses are 2^-40 fixed point,
//              w_i = trunc(exp(v_i - max) * 2^40), so every sum is an integer sum -- independent of the order the atomics land in,
//              and the C restatement's sorted loop (oracle/sampler_oracle.c) gets the same threshold bit for bit;
//              need = max(1, trunc(top_p * W)) in double.
// Every workgroup of pass l first takes level l - 1's decision from that level's histogram (redundantly: a parallel suffix scan by
// one wave); workgroup 0 records it.  The draw itself is the whole-vocabulary sampler's Gumbel-max pick restricted to keys >= the
// threshold (and to min_p).
__device__ __constant__ int samp_rshift[SAMP_LEVELS] = {53, 42, 31, 20, 9, 0};
__device__ __forceinline__ int samp_rbins(int level) { return level == SAMP_LEVELS - 1 ? 512 : 2048; }

// decision of one level: walking the bins from the top, the bin in which the running total first reaches `need`, and what is still
// needed inside it.  Called by all 256 threads of a workgroup; wave 0 decides.  total_out (optional): the sum of all bins.
__device__ void samp_radix_decide(const unsigned long long* __restrict__ hist, int nbins, unsigned long long need, bool need_from_total, float top_p,
                                  int* bin_out, unsigned long long* need_out) {
    __shared__ unsigned long long grp[256];
    __shared__ int s_bin;
    __shared__ unsigned long long s_need;
    const int tid = threadIdx.x, per = nbins / 256;      // 8 or 2 bins per thread
    unsigned long long g = 0;
    for (int j = 0; j < per; ++j) g += hist[tid * per + j];
    grp[tid] = g;
    __syncthreads();
    if (tid < 64) {
        unsigned long long s4 = grp[4 * tid] + grp[4 * tid + 1] + grp[4 * tid + 2] + grp[4 * tid + 3];
        // inclusive suffix sums over the lanes (lane 63 = the top bins)
        unsigned long long incl = s4;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const unsigned long long o = __shfl_down(incl, off);
            if (tid + off < 64) incl += o;
        }
        const unsigned long long total = __shfl(incl, 0);
        if (need_from_total) {   // mass cut: the target is a share of the candidates' total mass
            need = (unsigned long long)((double)top_p * (double)total);
            if (need < 1ull) need = 1ull;
        }
        const unsigned long long above = incl - s4;                   // total of the lanes above this one
        const bool here = above < need && incl >= need;
        const unsigned long long vote = __builtin_amdgcn_ballot_w64(here);
        if (vote == 0ull) {                                           // cannot happen while need <= total; keep the state defined
            if (tid == 0) { s_bin = 0; s_need = need; }
        } else if (here) {
            unsigned long long acc = above;
            int gi = 4 * tid + 3;
            for (; gi > 4 * tid; --gi) {
                if (acc + grp[gi] >= need) break;
                acc += grp[gi];
            }
            int b = gi * per + per - 1;
            for (; b > gi * per; --b) {
                if (acc + hist[b] >= need) break;
                acc += hist[b];
            }
            s_bin = b;
            s_need = need - acc;
        }
    }
    __syncthreads();
    *bin_out = s_bin;
    *need_out = s_need;
    __syncthreads();
}

// state after level `upto` (prefix of the key fixed so far, what is still needed inside it), for select m (0 rank, 1 mass);
// upto = -1: the start.  Workgroup 0 records each decision it takes.
__device__ void samp_radix_state(const SamplerDev* __restrict__ sp, SampWork* __restrict__ w, int m, int upto, unsigned long long* prefix,
                                 unsigned long long* need) {
    if (upto < 0) { *prefix = 0ull; *need = m == 0 ? (unsigned long long)sp->big_k : 0ull; return; }
    unsigned long long pfx = 0ull, nd = m == 0 ? (unsigned long long)sp->big_k : 0ull;
    if (upto >= 1) { pfx = w->rstate[m][upto - 1][0]; nd = w->rstate[m][upto - 1][1]; }
    int bin;
    unsigned long long nd2;
    samp_radix_decide(w->rhist[m][upto], samp_rbins(upto), nd, m == 1 && upto == 0, sp->top_p, &bin, &nd2);
    pfx |= (unsigned long long)bin << samp_rshift[upto];
    if (blockIdx.x == 0 && threadIdx.x == 0) { w->rstate[m][upto][0] = pfx; w->rstate[m][upto][1] = nd2; }
    *prefix = pfx;
    *need = nd2;
}
__device__ __forceinline__ unsigned long long samp_mass_fx(float d) {   // exp(v - max) in 2^-40 fixed point (d <= 0)
    return (unsigned long long)(rca_expf(d) * 1099511627776.0f);
}

// pass `level` of select m over the whole vocabulary
__global__ __launch_bounds__(256) void samp_radix_pass_kernel(const float* __restrict__ logits, int V, const SamplerDev* __restrict__ sp,
                                                              SampWork* __restrict__ w, int m, int level) {
    __shared__ unsigned long long hl[SAMP_BINS];
    unsigned long long prefix, need;
    samp_radix_state(sp, w, m, level - 1, &prefix, &need);
    const int nb = samp_rbins(level), shift = samp_rshift[level];
    for (int b = threadIdx.x; b < nb; b += 256) hl[b] = 0ull;
    __syncthreads();
    const int fixed = level == 0 ? 0 : 64 - samp_rshift[level - 1];       // key bits already decided (from the top)
    unsigned long long tk = 0ull;
    float mx = 0.0f;
    if (m == 1) {
        if (sp->big_k > 0) tk = w->rstate[0][SAMP_LEVELS - 1][0];          // candidates = keys >= T_k (the rank select is finished)
        const float* smax = reinterpret_cast<const float*>(w->hist);
        mx = smax[0];
        for (int k = 1; k < SAMPF_SLICES; ++k) mx = fmaxf(mx, smax[k]);
    }
    for (int i = blockIdx.x * 256 + threadIdx.x; i < V; i += gridDim.x * 256) {
        const float v = logits[i];
        const unsigned long long key = sample_key(v, (unsigned)i);
        if (fixed && (key >> (64 - fixed)) != (prefix >> (64 - fixed))) continue;
        if (m == 1 && key < tk) continue;
        const unsigned long long add = m == 0 ? 1ull : samp_mass_fx(v - mx);
        if (add) atomicAdd(&hl[(unsigned)(key >> shift) & (unsigned)(nb - 1)], add);
    }
    __syncthreads();
    for (int b = threadIdx.x; b < nb; b += 256)
        if (hl[b]) atomicAdd(&w->rhist[m][level][b], hl[b]);
}
// closes select m: the last level's decision fixes the threshold key, recorded in rstate[m][last][0]
__global__ __launch_bounds__(256) void samp_radix_finish_kernel(const SamplerDev* __restrict__ sp, SampWork* __restrict__ w, int m) {
    unsigned long long prefix, need;
    samp_radix_state(sp, w, m, SAMP_LEVELS - 1, &prefix, &need);
    unsigned long long* hz = &w->rhist[m][0][0];          // the select is done: its histograms are zero again for the next draw
    for (int b = threadIdx.x; b < SAMP_LEVELS * SAMP_BINS; b += 256) hz[b] = 0ull;
}
// the whole-vocabulary pick restricted to keys >= the threshold of the last select that ran
__global__ __launch_bounds__(1024) void samp_big_pick_kernel(const float* __restrict__ logits, int V, const SamplerDev* __restrict__ sp,
                                                             const LmDevState* __restrict__ stt, SampWork* __restrict__ w) {
    __shared__ unsigned long long red[16];
    const float* smax = reinterpret_cast<const float*>(w->hist);
    float mx = smax[0];
    for (int k = 1; k < SAMPF_SLICES; ++k) mx = fmaxf(mx, smax[k]);
    const unsigned long long thr = w->rstate[sp->big_p ? 1 : 0][SAMP_LEVELS - 1][0];
    const float inv_t = 1.0f / sp->temp, min_p = sp->min_p;
    const unsigned long long draw = splitmix(sp->seed, stt->rng_counter);
    const int per = (V + SAMPF_SLICES - 1) / SAMPF_SLICES;
    const int i0 = blockIdx.x * per, i1 = min(V, i0 + per);
    unsigned long long best = 0ull;
    for (int i = i0 + threadIdx.x; i < i1; i += 1024) {
        const float v = logits[i];
        if (sample_key(v, (unsigned)i) < thr) continue;
        const float d = v - mx;
        if (min_p > 0.0f && !(rca_expf(d) >= min_p)) continue;
        const unsigned long long z = splitmix(draw, (unsigned long long)i);
        const float u = (float)(unsigned)(((z >> 41) << 1) | 1ull) * 5.9604644775390625e-08f;
        const float g = -rca_logf(-rca_logf(u));
        const unsigned long long key = sample_key(__builtin_fmaf(d, inv_t, g), (unsigned)i);
        best = key > best ? key : best;
    }
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned long long o = __shfl_xor(best, off);
        best = o > best ? o : best;
    }
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = best;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long b = red[0];
        for (int k = 1; k < 16; ++k) b = red[k] > b ? red[k] : b;
        w->cand[blockIdx.x] = b;
    }
}

// probs[i] = softmax(logits)[ids[i]] : one workgroup, two sweeps (max, sum)
// softmax(logits)[ids] in two launches (the agent asks for P(<|end_audio|>) once per frame, realtime_agent_v2.py:448-452):
// 64 workgroups reduce a slice each to (max, sum of exp relative to it); one wave merges the slices in slice order.
#define PROBS_SLICES 64
// (bodies: shared with the table forms of rca_lm_batch_frame, which take the member's logits from grid y)
__device__ __forceinline__ void lm_softmax_slices_body(const float* __restrict__ logits, int V, float* __restrict__ part) {
    __shared__ float red[16];
    __shared__ float smax;
    const int per = (V + PROBS_SLICES - 1) / PROBS_SLICES;
    const int i0 = blockIdx.x * per, i1 = min(V, i0 + per);
    float mx = -INFINITY;
    for (int i = i0 + threadIdx.x; i < i1; i += 1024) mx = fmaxf(mx, logits[i]);
    mx = wave_max(mx);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = mx;
    __syncthreads();
    if (threadIdx.x == 0) { float m = red[0]; for (int w = 1; w < 16; ++w) m = fmaxf(m, red[w]); smax = m; }
    __syncthreads();
    mx = smax;
    float s = 0.0f;
    for (int i = i0 + threadIdx.x; i < i1; i += 1024) s += __expf(logits[i] - mx);
    s = wave_sum(s);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        float t = 0;
        for (int w = 0; w < 16; ++w) t += red[w];
        part[2 * blockIdx.x] = mx;
        part[2 * blockIdx.x + 1] = t;
    }
}
__global__ __launch_bounds__(1024) void lm_softmax_slices_kernel(const float* __restrict__ logits, int V, float* __restrict__ part) {
    lm_softmax_slices_body(logits, V, part);
}
__device__ __forceinline__ void lm_token_probs_body(const float* __restrict__ logits, int V, const float* __restrict__ part,
                                                    const int* __restrict__ ids, int n, float* __restrict__ probs) {
    const float pm = part[2 * threadIdx.x], ps = part[2 * threadIdx.x + 1];   // PROBS_SLICES == 64 lanes
    const float mx = wave_max(pm);
    const float contrib = (pm == -INFINITY) ? 0.0f : ps * __expf(pm - mx);
    float tot = 0.0f;
    for (int b = 0; b < PROBS_SLICES; ++b) tot += __shfl(contrib, b);   // slice order
    if ((int)threadIdx.x < n) {
        const int id = ids[threadIdx.x];
        probs[threadIdx.x] = (id >= 0 && id < V) ? __expf(logits[id] - mx) / tot : 0.0f;
    }
}
__global__ __launch_bounds__(64) void lm_token_probs_kernel(const float* __restrict__ logits, int V, const float* __restrict__ part,
                                                            const int* __restrict__ ids, int n, float* __restrict__ probs) {
    lm_token_probs_body(logits, V, part, ids, n, probs);
}

// ------------------------------------------------------------------------- random init (bench)
// value(tensor_id, i) = std * 1.7320508 * (sum of four 16-bit uniforms - 131070) / 65535 ~ N(0, std^2)
// (Irwin-Hall, integer arithmetic only, reproduced by oracle/lm_ref.py), rounded to bf16 (RNE).
__global__ __launch_bounds__(256) void lm_random_bf16_kernel(bf16_t* __restrict__ out, long n, unsigned long long seed,
                                                             unsigned long long tensor_id, float scale) {
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        const unsigned long long z = splitmix(seed ^ (tensor_id * 0xD6E8FEB86659FD93ull), (unsigned long long)i);
        const int sum = (int)(z & 0xFFFF) + (int)((z >> 16) & 0xFFFF) + (int)((z >> 32) & 0xFFFF) + (int)((z >> 48) & 0xFFFF);
        out[i] = f32_to_bf16_rne((float)(sum - 131070) * scale);
    }
}
__global__ __launch_bounds__(256) void lm_fill_f32_kernel(float* __restrict__ out, long n, float v) {
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) out[i] = v;
}
__global__ __launch_bounds__(256) void lm_rope_table_kernel(const float* __restrict__ inv_freq, float* __restrict__ cos_t,
                                                            float* __restrict__ sin_t, int n_ctx, int half) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long)n_ctx * half) return;
    const int pos = (int)(i / half), d = (int)(i - (long)pos * half);
    const float ang = (float)pos * inv_freq[d];
    cos_t[i] = cosf(ang);
    sin_t[i] = sinf(ang);
}
// interleave gate/up rows: dst row 2i = gate_i, 2i+1 = up_i
__global__ __launch_bounds__(256) void lm_interleave_rows_kernel(const bf16_t* __restrict__ gate, const bf16_t* __restrict__ up,
                                                                 bf16_t* __restrict__ dst, int F, int H) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long)2 * F * H) return;
    const long row = i / H;
    const int h = (int)(i - row * H);
    const long src = (row >> 1) * H + h;
    dst[i] = (row & 1) ? up[src] : gate[src];
}
__global__ __launch_bounds__(256) void lm_f32_to_bf16_kernel(const float* __restrict__ in, bf16_t* __restrict__ out, long n) {
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) out[i] = f32_to_bf16_rne(in[i]);
}

// ------------------------------------------------------------------------- weight formats at load
// GGUF block_q8_0 = { fp16 d; int8 qs[32] } (34 bytes), value = d * q.  "Plain" form on the device: q [N][K] int8 and
// d [N][K / 32] fp16; from there the pair-interleaved layout the GEMV streams (GemvQ8).  There is no second copy: the prefill tiles
// de-quantise the packed blocks while staging (lm_gemm128_kernel).
__global__ __launch_bounds__(256) void lm_q8_unblock_kernel(const unsigned char* __restrict__ blocks, long nblocks, signed char* __restrict__ q,
                                                            f16_t* __restrict__ d) {
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < nblocks * 32; i += (long)gridDim.x * blockDim.x) {
        const long blk = i >> 5;
        const int j = (int)(i & 31);
        const unsigned char* bp = blocks + blk * 34;
        q[i] = (signed char)bp[2 + j];
        if (j == 0) {
            const unsigned short bits = (unsigned short)bp[0] | ((unsigned short)bp[1] << 8);
            d[blk] = __builtin_bit_cast(f16_t, bits);
        }
    }
}
__device__ __forceinline__ float w16_to_f32(bf16_t bits, int is_f16) {
    return is_f16 ? (float)__builtin_bit_cast(f16_t, bits) : __uint_as_float((unsigned)bits << 16);
}
// llama.cpp's quantize_row_q8_0: d = amax / 127, q = round(x / d) (ties away from zero), d stored as fp16
__global__ __launch_bounds__(256) void lm_q8_quantize_kernel(const bf16_t* __restrict__ w, int is_f16, long nblocks, signed char* __restrict__ q,
                                                             f16_t* __restrict__ d) {
    for (long blk = (long)blockIdx.x * blockDim.x + threadIdx.x; blk < nblocks; blk += (long)gridDim.x * blockDim.x) {
        float v[32];
        float amax = 0.0f;
#pragma unroll
        for (int j = 0; j < 32; ++j) {
            v[j] = w16_to_f32(w[blk * 32 + j], is_f16);
            amax = fmaxf(amax, fabsf(v[j]));
        }
        const float dd = amax / 127.0f;
        const float id = dd != 0.0f ? 1.0f / dd : 0.0f;
#pragma unroll
        for (int j = 0; j < 32; ++j) q[blk * 32 + j] = (signed char)(int)roundf(v[j] * id);
        d[blk] = (f16_t)dd;
    }
}
__global__ __launch_bounds__(256) void lm_q8_dequant_f32_kernel(const signed char* __restrict__ q, const f16_t* __restrict__ d, float* __restrict__ out, long n) {
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x)
        out[i] = (float)d[i >> 5] * (float)q[i];
}
__global__ __launch_bounds__(256) void lm_bf16_to_f16_kernel(const bf16_t* __restrict__ in, f16_t* __restrict__ out, long n) {
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x)
        out[i] = (f16_t)__uint_as_float((unsigned)in[i] << 16);   // round to nearest even (values below the fp16 range go subnormal / to zero)
}
__global__ __launch_bounds__(256) void lm_f16_to_f32_kernel(const f16_t* __restrict__ in, float* __restrict__ out, long n) {
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) out[i] = (float)in[i];
}
// rows of two byte matrices interleaved: dst row 2i = a row i, 2i+1 = b row i (gate/up: 16-bit values, q8_0 q and d)
__global__ __launch_bounds__(256) void lm_interleave_rows_bytes_kernel(const unsigned char* __restrict__ a, const unsigned char* __restrict__ b,
                                                                       unsigned char* __restrict__ dst, long rows, long row_bytes) {
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < 2 * rows * row_bytes; i += (long)gridDim.x * blockDim.x) {
        const long row = i / row_bytes, o = i - row * row_bytes;
        dst[i] = (row & 1) ? b[(row >> 1) * row_bytes + o] : a[(row >> 1) * row_bytes + o];
    }
}
// ---- Q4_K.  Plain form on the device: q [N][K] one byte per 4-bit value, scm [N][K / 32] ushort (sc | m << 8), dd [N][K / 256]
// uint (d | dmin << 16).
__global__ __launch_bounds__(256) void lm_q4k_unblock_kernel(const unsigned char* __restrict__ blocks, long nblocks, unsigned char* __restrict__ q,
                                                             unsigned short* __restrict__ scm, unsigned* __restrict__ dd) {
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < nblocks * 256; i += (long)gridDim.x * blockDim.x) {
        const long blk = i >> 8;
        const int e = (int)(i & 255);
        const unsigned char* bp = blocks + blk * 144;
        const int t = e >> 6, l = e & 31, high = (e >> 5) & 1;   // weights 64 t + 32 high + l: low / high nibble of qs[32 t + l]
        const unsigned char byte = bp[16 + 32 * t + l];
        q[i] = high ? (byte >> 4) : (byte & 0xF);
        if ((e & 31) == 0) {   // sub-block j = e / 32: get_scale_min_k4
            const int j = e >> 5;
            const unsigned char* sc = bp + 4;
            unsigned scv, mv;
            if (j < 4) { scv = sc[j] & 63; mv = sc[j + 4] & 63; }
            else { scv = (sc[j + 4] & 0xF) | ((sc[j - 4] >> 6) << 4); mv = (sc[j + 4] >> 4) | ((sc[j] >> 6) << 4); }
            scm[blk * 8 + j] = (unsigned short)(scv | (mv << 8));
        }
        if (e == 0) dd[blk] = (unsigned)bp[0] | ((unsigned)bp[1] << 8) | ((unsigned)bp[2] << 16) | ((unsigned)bp[3] << 24);
    }
}
// ---- Q5_K (176-byte block_q5_K = { fp16 d; fp16 dmin; scales[12]; qh[32]; qs[128] }).  Plain form: the Q4_K one with the 5-bit value in
// the byte.  Weight 64 t + 32 high + l: low / high nibble of qs[32 t + l] and, as its bit 4, bit 2 t + high of qh[l].
__global__ __launch_bounds__(256) void lm_q5k_unblock_kernel(const unsigned char* __restrict__ blocks, long nblocks, unsigned char* __restrict__ q,
                                                             unsigned short* __restrict__ scm, unsigned* __restrict__ dd) {
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < nblocks * 256; i += (long)gridDim.x * blockDim.x) {
        const long blk = i >> 8;
        const int e = (int)(i & 255);
        const unsigned char* bp = blocks + blk * 176;
        const int t = e >> 6, l = e & 31, high = (e >> 5) & 1;
        const unsigned char byte = bp[48 + 32 * t + l];
        const unsigned b4 = (bp[16 + l] >> (2 * t + high)) & 1u;
        q[i] = (unsigned char)((high ? (byte >> 4) : (byte & 0xF)) | (b4 << 4));
        if ((e & 31) == 0) {   // sub-block j = e / 32: get_scale_min_k4, as for Q4_K
            const int j = e >> 5;
            const unsigned char* sc = bp + 4;
            unsigned scv, mv;
            if (j < 4) { scv = sc[j] & 63; mv = sc[j + 4] & 63; }
            else { scv = (sc[j + 4] & 0xF) | ((sc[j - 4] >> 6) << 4); mv = (sc[j + 4] >> 4) | ((sc[j] >> 6) << 4); }
            scm[blk * 8 + j] = (unsigned short)(scv | (mv << 8));
        }
        if (e == 0) dd[blk] = (unsigned)bp[0] | ((unsigned)bp[1] << 8) | ((unsigned)bp[2] << 16) | ((unsigned)bp[3] << 24);
    }
}
// ---- Q4_0 / Q4_1 (18-byte block_q4_0 = { fp16 d; qs[16] }, 20-byte block_q4_1 = { fp16 d; fp16 m; qs[16] }; value j of a block is the low
// nibble of qs[j], value j + 16 the high nibble).  Plain form on the device: q [N][K] one byte per 4-bit value, st [N][K / 32] uint
// (fp16 s | fp16 t << 16) with value = s q - t: Q4_0 s = d, t = 8 d (exact in fp16 unless it overflows: *bad is set then and the load
// fails), Q4_1 s = d, t = -m (the sign bit flipped).
__device__ __forceinline__ unsigned q40_factors(unsigned short dbits, int* __restrict__ bad) {
    const f16_t t = (f16_t)(8.0f * (float)__builtin_bit_cast(f16_t, dbits));
    const unsigned short tb = __builtin_bit_cast(unsigned short, t);
    if ((tb & 0x7c00u) == 0x7c00u) *bad = 1;   // inf or NaN
    return (unsigned)dbits | ((unsigned)tb << 16);
}
template <bool Q41>
__global__ __launch_bounds__(256) void lm_q40_unblock_kernel(const unsigned char* __restrict__ blocks, long nblocks, unsigned char* __restrict__ q,
                                                             unsigned* __restrict__ st, int* __restrict__ bad) {
    constexpr int BS = Q41 ? 20 : 18, Q0 = Q41 ? 4 : 2;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < nblocks * 32; i += (long)gridDim.x * blockDim.x) {
        const long blk = i >> 5;
        const int j = (int)(i & 31);
        const unsigned char* bp = blocks + blk * BS;
        const unsigned char byte = bp[Q0 + (j & 15)];
        q[i] = j < 16 ? (byte & 0xF) : (byte >> 4);
        if (j == 0) {
            const unsigned short dbits = (unsigned short)bp[0] | ((unsigned short)bp[1] << 8);
            if (Q41) st[blk] = (unsigned)dbits | (((unsigned)bp[2] | ((unsigned)bp[3] << 8)) ^ 0x8000u) << 16;
            else st[blk] = q40_factors(dbits, bad);
        }
    }
}
// ggml's quantize_row_q4_0_ref / quantize_row_q4_1_ref restated from the published algorithm (ggml is not part of this tree: parity with
// llama-quantize's own bits is not pinned).  Q4_0: max = the value of largest magnitude (the first on ties), d = max / -8,
// id = d != 0 ? 1 / d : 0, q = min(15, (int)(x * id + 8.5f)).  Q4_1: d = (max - min) / 15, q = min(15, (int)((x - min) * id + 0.5f)).
// Every operation is rounded to f32 on its own (the build runs with -ffp-contract=off); d and min are stored as fp16 (rne).
template <bool Q41>
__global__ __launch_bounds__(256) void lm_q40_quantize_kernel(const bf16_t* __restrict__ w, int is_f16, long nblocks, unsigned char* __restrict__ q,
                                                              unsigned* __restrict__ st, int* __restrict__ bad) {
    for (long blk = (long)blockIdx.x * blockDim.x + threadIdx.x; blk < nblocks; blk += (long)gridDim.x * blockDim.x) {
        float v[32];
        float amax = 0.0f, mx = 0.0f, lo = INFINITY, hi = -INFINITY;
#pragma unroll
        for (int j = 0; j < 32; ++j) {
            v[j] = w16_to_f32(w[blk * 32 + j], is_f16);
            if (amax < fabsf(v[j])) { amax = fabsf(v[j]); mx = v[j]; }
            lo = fminf(lo, v[j]);
            hi = fmaxf(hi, v[j]);
        }
        const float d = Q41 ? (hi - lo) / 15.0f : mx / -8.0f;
        const float id = d != 0.0f ? 1.0f / d : 0.0f;
#pragma unroll
        for (int j = 0; j < 32; ++j) {
            const float y = Q41 ? (v[j] - lo) * id + 0.5f : v[j] * id + 8.5f;
            q[blk * 32 + j] = (unsigned char)min(15, (int)y);
        }
        const unsigned short dbits = __builtin_bit_cast(unsigned short, (f16_t)d);
        if (Q41) st[blk] = (unsigned)dbits | ((unsigned)(__builtin_bit_cast(unsigned short, (f16_t)lo) ^ 0x8000u) << 16);
        else st[blk] = q40_factors(dbits, bad);
    }
}
// s q - t in f32: d q and 8 d are exact and so is their difference, d (q - 8) (dequantize_row_q4_0's value); for Q4_1 the subtraction of
// t = -m is dequantize_row_q4_1's one rounding on d q + m
__device__ __forceinline__ float q40_value(unsigned st, unsigned q) {
    const f16x2 f = __builtin_bit_cast(f16x2, st);
    return (float)f[0] * (float)q - (float)f[1];
}
__global__ __launch_bounds__(256) void lm_q40_dequant_f32_kernel(const unsigned char* __restrict__ q, const unsigned* __restrict__ st, float* __restrict__ out, long n) {
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) out[i] = q40_value(st[i >> 5], q[i]);
}
// ---- IQ4_NL / IQ4_XS (18-byte block_iq4_nl = { fp16 d; qs[16] } over 32 values, 136-byte block_iq4_xs = { fp16 d; uint16 scales_h;
// scales_l[4]; qs[128] } over 256; value j of a 32-value (sub-)block is the low nibble of its qs[j], value j + 16 the high nibble; the
// 6-bit scale of sub-block ib is ls = ((scales_l[ib / 2] >> 4 (ib % 2)) & 15) | (((scales_h >> 2 ib) & 3) << 4)).  Plain form on the
// device: q [N][K] one byte per 4-bit index, st [N][K / 32] the f32 factor s (bits) with value = s kv[q]: IQ4_NL s = d, IQ4_XS
// s = d (ls - 32), exact.  A d that is not finite sets *bad and the load fails.
template <bool XS>
__global__ __launch_bounds__(256) void lm_iq4_unblock_kernel(const unsigned char* __restrict__ blocks, long nblocks32, unsigned char* __restrict__ q,
                                                             unsigned* __restrict__ st, int* __restrict__ bad) {
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < nblocks32 * 32; i += (long)gridDim.x * blockDim.x) {
        const long blk = i >> 5;   // 32-value (sub-)block
        const int j = (int)(i & 31);
        const int ib = XS ? (int)(blk & 7) : 0;
        const unsigned char* bp = XS ? blocks + (blk >> 3) * 136 : blocks + blk * 18;
        const unsigned char byte = XS ? bp[8 + 16 * ib + (j & 15)] : bp[2 + (j & 15)];
        q[i] = j < 16 ? (byte & 0xF) : (byte >> 4);
        if (j == 0) {
            const unsigned short dbits = (unsigned short)bp[0] | ((unsigned short)bp[1] << 8);
            if ((dbits & 0x7c00u) == 0x7c00u) *bad = 1;   // inf or NaN
            float s = (float)__builtin_bit_cast(f16_t, dbits);
            if (XS) {
                const unsigned sh = (unsigned)bp[2] | ((unsigned)bp[3] << 8);
                const int ls = (int)(((unsigned)bp[4 + (ib >> 1)] >> (4 * (ib & 1))) & 15u) | (int)(((sh >> (2 * ib)) & 3u) << 4);
                s = s * (float)(ls - 32);
            }
            st[blk] = __float_as_uint(s);
        }
    }
}
// The load-time IQ4_NL rule of this build (NOT llama-quantize's, which is an iterative weighted search): max = the value of largest
// magnitude (the first on ties), d = fp16(max / -127); every value goes to the index whose d kv[i] is nearest (|v - d kv[i]| in f32,
// ties to the lower index); a block whose d is zero (all-zero blocks among them) gets index 8 everywhere.
__global__ __launch_bounds__(256) void lm_iq4nl_quantize_kernel(const bf16_t* __restrict__ w, int is_f16, long nblocks, unsigned char* __restrict__ q,
                                                                unsigned* __restrict__ st, int* __restrict__ bad) {
    for (long blk = (long)blockIdx.x * blockDim.x + threadIdx.x; blk < nblocks; blk += (long)gridDim.x * blockDim.x) {
        float amax = 0.0f, mx = 0.0f;
        for (int j = 0; j < 32; ++j) {
            const float v = w16_to_f32(w[blk * 32 + j], is_f16);
            if (amax < fabsf(v)) { amax = fabsf(v); mx = v; }
        }
        const f16_t dh = (f16_t)(mx / -127.0f);
        const unsigned short dbits = __builtin_bit_cast(unsigned short, dh);
        if ((dbits & 0x7c00u) == 0x7c00u) *bad = 1;
        const float d = (float)dh;
        for (int j = 0; j < 32; ++j) {
            const float v = w16_to_f32(w[blk * 32 + j], is_f16);
            int best = 8;
            if (d != 0.0f) {
                best = 0;
                float bd = fabsf(v - d * (float)iq4_kv(0));
                for (int i = 1; i < 16; ++i) {
                    const float e = fabsf(v - d * (float)iq4_kv(i));
                    if (e < bd) { bd = e; best = i; }
                }
            }
            q[blk * 32 + j] = (unsigned char)best;
        }
        st[blk] = __float_as_uint(d);
    }
}
// s kv[q] in f32: 17 x 7 bits, exact (dequantize_row_iq4_nl's / _xs's value)
__device__ __forceinline__ float iq4_value(unsigned st, unsigned q) { return __uint_as_float(st) * (float)iq4_kv(q); }
__global__ __launch_bounds__(256) void lm_iq4_dequant_f32_kernel(const unsigned char* __restrict__ q, const unsigned* __restrict__ st, float* __restrict__ out, long n) {
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) out[i] = iq4_value(st[i >> 5], q[i]);
}
// This build's Q4_K quantiser (oracle/q4k_ref.py::quantize_q4_k, operation for operation): per 32 values offset o = -min(0, min w)
// and step s = (max w + o) / 15; per 256 d = max s / 63, dmin = max o / 63 (fp16); sc = round(s / d), m = round(o / dmin);
// q = clamp(round((w + dmin m) / (d sc)), 0, 15).  llama-quantize searches for better scales; the FORMAT and its de-quantisation are GGUF's.
// QMAX = 31: the same rule with 31 steps, Q5_K (the plain form keeps the whole 5-bit value in its byte).
template <int QMAX>
__global__ __launch_bounds__(256) void lm_q4k_quantize_kernel(const bf16_t* __restrict__ w, int is_f16, long nblocks, unsigned char* __restrict__ q,
                                                              unsigned short* __restrict__ scm, unsigned* __restrict__ dd) {
    for (long blk = (long)blockIdx.x * blockDim.x + threadIdx.x; blk < nblocks; blk += (long)gridDim.x * blockDim.x) {
        float s[8], o[8];
        float smax = 0.0f, omax = 0.0f;
        for (int j = 0; j < 8; ++j) {
            float mn = 0.0f, mx = -INFINITY;
            for (int l = 0; l < 32; ++l) {
                const float v = w16_to_f32(w[blk * 256 + j * 32 + l], is_f16);
                mn = fminf(mn, v);
                mx = fmaxf(mx, v);
            }
            s[j] = (mx - mn) / (float)QMAX;
            o[j] = -mn;
            smax = fmaxf(smax, s[j]);
            omax = fmaxf(omax, o[j]);
        }
        const f16_t dh = (f16_t)(smax / 63.0f), dminh = (f16_t)(omax / 63.0f);
        const float df = (float)dh, dminf = (float)dminh;
        for (int j = 0; j < 8; ++j) {
            float sc = df > 0.0f ? floorf(s[j] / df + 0.5f) : 0.0f;
            float mm = dminf > 0.0f ? floorf(o[j] / dminf + 0.5f) : 0.0f;
            sc = fminf(fmaxf(sc, 0.0f), 63.0f);
            mm = fminf(fmaxf(mm, 0.0f), 63.0f);
            const float d1 = df * sc, m1 = dminf * mm;
            for (int l = 0; l < 32; ++l) {
                const float v = w16_to_f32(w[blk * 256 + j * 32 + l], is_f16);
                float qq = d1 > 0.0f ? floorf((v + m1) / d1 + 0.5f) : 0.0f;
                qq = fminf(fmaxf(qq, 0.0f), (float)QMAX);
                q[blk * 256 + j * 32 + l] = (unsigned char)qq;
            }
            scm[blk * 8 + j] = (unsigned short)((unsigned)sc | ((unsigned)mm << 8));
        }
        dd[blk] = (unsigned)__builtin_bit_cast(unsigned short, dh) | ((unsigned)__builtin_bit_cast(unsigned short, dminh) << 16);
    }
}
// dequantize_row_q4_K's arithmetic: (d * sc) * q - (dmin * m), two products and a subtraction in f32
__device__ __forceinline__ float q4k_value(unsigned dd, unsigned scm, unsigned q) {
    const f16x2 d2 = __builtin_bit_cast(f16x2, dd);
    const float d1 = (float)d2[0] * (float)(scm & 0xffu), m1 = (float)d2[1] * (float)(scm >> 8);
    return d1 * (float)q - m1;
}
__global__ __launch_bounds__(256) void lm_q4k_dequant_f32_kernel(const unsigned char* __restrict__ q, const unsigned short* __restrict__ scm,
                                                                 const unsigned* __restrict__ dd, float* __restrict__ out, long n) {
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) out[i] = q4k_value(dd[i >> 8], scm[i >> 5], q[i]);
}
// slot -> row of a packed matrix: plain, or (qkv_pairs) slots (2 s, 2 s + 1) = rows (d, d + 32) of one head
__host__ __device__ __forceinline__ long packed_slot_row(long slot, int qkv_pairs) {
    if (!qkv_pairs) return slot;
    const long pp = slot >> 1;
    return (pp >> 5) * 64 + (pp & 31) + 32 * (slot & 1);
}
// plain -> the quad-interleaved GEMV layout (GemvQ8 with dd).  WF_Q5K: the low nibbles as for Q4_K, bit 4 of every value into the
// plane qh[quad][k / 8] (q5k_hbit).  WF_Q40 (Q4_0 / Q4_1): the nibbles as for Q4_K; `dd` is the plain factor array st [N][K / 32] and
// `odd` its slot-grouped copy [ceil(N / 16)][K / 32][16] (scm / oscm unused).
template <int WF>
__global__ __launch_bounds__(256) void lm_q4k_pack_kernel(const unsigned char* __restrict__ q, const unsigned short* __restrict__ scm, const unsigned* __restrict__ dd,
                                                          int N, int K, int qkv_pairs, u32x4* __restrict__ qs, unsigned short* __restrict__ oscm, unsigned* __restrict__ odd,
                                                          unsigned* __restrict__ qh) {
    const long nchunk = K >> 3, nquad = (N + 3) >> 2, nkb = K >> 5, nk256 = K >> 8;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < nquad * nchunk; i += (long)gridDim.x * blockDim.x) {
        const long quad = i / nchunk;
        const int c = (int)(i - quad * nchunk);
        constexpr bool Q5 = WF == WF_Q5K, Q40 = WF == WF_Q40;
        unsigned dw[4], hb = 0;
#pragma unroll
        for (int sl = 0; sl < 4; ++sl) {
            const long slot = 4 * quad + sl, row = packed_slot_row(slot, qkv_pairs);
            unsigned v = 0;
            if (slot < N) {
                const uint2 b8 = *reinterpret_cast<const uint2*>(q + row * K + 8 * c);
                const unsigned bytes[2] = {b8.x, b8.y};
#pragma unroll
                for (int j = 0; j < 8; ++j) v |= ((bytes[j >> 2] >> (8 * (j & 3))) & 0xFu) << (4 * j);
                if (Q5) {
#pragma unroll
                    for (int j = 0; j < 8; ++j) hb |= ((bytes[j >> 2] >> (8 * (j & 3) + 4)) & 1u) << q5k_hbit(sl, j);
                }
                if (Q40) {
                    if ((c & 3) == 0) odd[q4k_scm_index(slot, c >> 2, nkb)] = dd[row * nkb + (c >> 2)];
                } else {
                    if ((c & 3) == 0) oscm[q4k_scm_index(slot, c >> 2, nkb)] = scm[row * nkb + (c >> 2)];
                    if ((c & 31) == 0) odd[q4k_scm_index(slot, c >> 5, nk256)] = dd[row * nk256 + (c >> 5)];
                }
            }
            dw[sl] = v;
        }
        qs[i] = u32x4{dw[0], dw[1], dw[2], dw[3]};
        if (Q5) qh[i] = hb;
    }
}
// ---- Q6_K.  Plain form on the device: q [N][K] int8 (the 6-bit value - 32), sc [N][K / 16] int8, d [N][K / 256] fp16.
__global__ __launch_bounds__(256) void lm_q6k_unblock_kernel(const unsigned char* __restrict__ blocks, long nblocks, signed char* __restrict__ q,
                                                             signed char* __restrict__ sc, f16_t* __restrict__ d) {
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < nblocks * 256; i += (long)gridDim.x * blockDim.x) {
        const long blk = i >> 8;
        const int e = (int)(i & 255);
        const unsigned char* bp = blocks + blk * 210;
        const int n = e >> 7, j = (e >> 5) & 3, l = e & 31;          // weight 128 n + 32 j + l (dequantize_row_q6_K's q1..q4 = j 0..3)
        const unsigned char lb = bp[64 * n + 32 * (j & 1) + l];
        const unsigned lo = (j >> 1) ? (lb >> 4) : (lb & 0xF);
        const unsigned hi = (bp[128 + 32 * n + l] >> (2 * j)) & 3u;
        q[i] = (signed char)((int)(lo | (hi << 4)) - 32);
        if ((e & 15) == 0) sc[blk * 16 + (e >> 4)] = (signed char)bp[192 + (e >> 4)];
        if (e == 0) {
            const unsigned short bits = (unsigned short)bp[208] | ((unsigned short)bp[209] << 8);
            d[blk] = __builtin_bit_cast(f16_t, bits);
        }
    }
}
__global__ __launch_bounds__(256) void lm_q6k_dequant_f32_kernel(const signed char* __restrict__ q, const signed char* __restrict__ sc, const f16_t* __restrict__ d,
                                                                 float* __restrict__ out, long n) {
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x)
        out[i] = ((float)d[i >> 8] * (float)sc[i >> 4]) * (float)q[i];
}
// plain -> the q8_0 pair layout for the values + (s_a, s_b) f32 scales per pair and group of 16
__global__ __launch_bounds__(256) void lm_q6k_pack_kernel(const signed char* __restrict__ q, const signed char* __restrict__ sc, const f16_t* __restrict__ d,
                                                          int N, int K, int qkv_pairs, u32x4* __restrict__ qs, float* __restrict__ osc) {
    const long nchunk = K >> 3, npairs = N >> 1, nk16 = K >> 4;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < npairs * nchunk; i += (long)gridDim.x * blockDim.x) {
        const long pp = i / nchunk;
        const int c = (int)(i - pp * nchunk);
        const long ra = qkv_pairs ? (pp >> 5) * 64 + (pp & 31) : 2 * pp;
        const long rb = qkv_pairs ? ra + 32 : ra + 1;
        const uint2 a = *reinterpret_cast<const uint2*>(q + ra * K + 8 * c);
        const uint2 b = *reinterpret_cast<const uint2*>(q + rb * K + 8 * c);
        qs[i] = u32x4{a.x, a.y, b.x, b.y};
        if ((c & 1) == 0) {
            const long k16 = c >> 1;
            float* o = osc + 2 * q8_sc_index(pp, k16, nk16);
            o[0] = (float)d[ra * (K >> 8) + (k16 >> 4)] * (float)sc[ra * nk16 + k16];
            o[1] = (float)d[rb * (K >> 8) + (k16 >> 4)] * (float)sc[rb * nk16 + k16];
        }
    }
}
// plain -> GemvQ8.  pair pp = rows (2pp, 2pp+1), or for the fused QKV matrix (qkv_pairs) rows (d, d+32) of one head.
__global__ __launch_bounds__(256) void lm_q8_pack_kernel(const signed char* __restrict__ q, const f16_t* __restrict__ d, int N, int K, int qkv_pairs,
                                                         u32x4* __restrict__ qs, unsigned* __restrict__ sc) {
    const long nchunk = K >> 3, npairs = N >> 1;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < npairs * nchunk; i += (long)gridDim.x * blockDim.x) {
        const long pp = i / nchunk;
        const int c = (int)(i - pp * nchunk);
        const long ra = qkv_pairs ? (pp >> 5) * 64 + (pp & 31) : 2 * pp;
        const long rb = qkv_pairs ? ra + 32 : ra + 1;
        const uint2 a = *reinterpret_cast<const uint2*>(q + ra * K + 8 * c);
        const uint2 b = *reinterpret_cast<const uint2*>(q + rb * K + 8 * c);
        qs[i] = u32x4{a.x, a.y, b.x, b.y};
        if ((c & 3) == 0) {
            const unsigned short da = __builtin_bit_cast(unsigned short, d[ra * (K >> 5) + (c >> 2)]);
            const unsigned short db = __builtin_bit_cast(unsigned short, d[rb * (K >> 5) + (c >> 2)]);
            sc[q8_sc_index(pp, c >> 2, K >> 5)] = (unsigned)da | ((unsigned)db << 16);
        }
    }
}

// =============================================================================================
// One projection matrix [N][K] as it is kept in HBM: ONE copy, in the format it arrived in (or was asked for through
// rca_lm_config_t::decode_weights).
struct WMat {
    int fmt = WF_BF16;
    int N = 0, K = 0;
    bf16_t* w = nullptr;        // WF_BF16 / WF_F16: row-major 16-bit values
    u32x4* qs = nullptr;        // WF_Q8 / WF_Q4K (GemvQ8)
    unsigned* sc = nullptr;     // WF_Q40 / WF_Q41: the (s | t << 16) factor dwords; WF_IQ4 / WF_IQ4XS: the f32 factors s
    unsigned* dd = nullptr;     // WF_Q4K / WF_Q5K
    unsigned* qh = nullptr;     // WF_Q5K: the plane of high bits [N / 4][K / 8]
    void release() {
        for (void* p : {(void*)w, (void*)qs, (void*)sc, (void*)dd, (void*)qh})
            if (p) (void)hipFree(p);
        w = nullptr; qs = nullptr; sc = nullptr; dd = nullptr; qh = nullptr;
    }
    // the kernels' 16-bit weight pointer: the packed formats do not use it, and Q5_K hands its plane over in that argument (the
    // argument list, and with it the 14 preloaded dwords, stays what it is for every format)
    const bf16_t* wptr() const { return fmt == WF_Q5K ? reinterpret_cast<const bf16_t*>(qh) : w; }
    long stream_bytes() const { return (long)N * K * WF_TABLE[fmt].stream64 / 64; }   // bytes one decode pass reads of it
    void** array(int arr) {   // the member a WA_* id of the table names
        return arr == WA_W16 ? (void**)&w : (arr == WA_QS ? (void**)&qs : (arr == WA_SC ? (void**)&sc : (arr == WA_DD ? (void**)&dd : (void**)&qh)));
    }
};
struct LmLayer {
    WMat qkv, o, gu, down;
    WMat vseg;              // split_v: qkv holds [q; k] only and the V projection is a matrix of its own (formats differ)
    bool split_v = false;
    float *attn_norm = nullptr, *ffn_norm = nullptr;
};

struct rca_lm {
    int n_cus = 256;            // compute units of the device (grid shapes that want one workgroup per CU)
    rca_lm_config_t cfg;
    int device = 0;
    hipStream_t stream = nullptr;
    void* embed = nullptr;      // [V][H] bf16 or f32 rows (embed_f32): the table keeps the precision it arrived in
    int embed_f32 = 0;
    WMat head;
    float* final_norm = nullptr;
    std::vector<LmLayer> layers;
    float *cos_t = nullptr, *sin_t = nullptr;
    f16_t *kc = nullptr, *vc = nullptr;  // [L][n_ctx_pad][nkv][hd]; kv_format 1: ONE allocation each of the int8 plane [L][n_ctx_pad][nkv][64] and,
                                         // behind it, the fp16 scales [L][n_ctx_pad][nkv][2] -- so whatever exchanges or keys caches by these two
                                         // pointers (rca_lm_swap_kv, the graph sets, rca_duplex_precapture) holds for either format
    int kv_format = 0;                   // 0 fp16, 1 q8_0 (rca_lm_set_kv_format)
    int kv_shift_requant = 0;            // q8_0 only: rca_lm_kv_remove may re-quantise the rotated keys (rca_lm_set_kv_shift_requant); a permission, no state
    f16_t *ring_k = nullptr, *ring_v = nullptr;   // q8_0: [LM_KV_RING][nkv][64] fp16 rows of the current pass and layer, what the QKV epilogues store
    f16_t* kv_stage = nullptr;           // rca_lm_kv_remove: two slabs of [K, V][L][ATT_KEYS][nkv][hd], allocated by the first call that moves rows
    f16_t* kv_stage_many = nullptr;      // rca_lm_kv_remove_many, on the weight OWNER only: RCA_LM_KV_REMOVE_GROUP such pairs of slabs, allocated by the first
                                         // call with a staged member, freed with the weights (lm_free_weights)
    long kv_layer_stride = 0;
    int n_ctx_pad = 0, n_splits = 0;
    // activations
    float *x = nullptr, *xn = nullptr, *qkv = nullptr, *attn = nullptr, *hbuf = nullptr,
          *att_part = nullptr, *logits = nullptr, *probs_dev = nullptr;
    int* probe_ids_dev = nullptr;
    int* att_arrive = nullptr;   // per kv head: workgroups of the current attention launch that have published their partial
    bf16_t *xh = nullptr, *xl = nullptr;   // prefill: bf16 hi / lo split of the current GEMM input [LM_MAXM][max K]
    float* gpart = nullptr;                // prefill: k-split partial sums of the narrow projections [8][LM_MAXM][hidden]
    long logits_rows_cap = 0;   // rows allocated in `logits` (1, or more when logits_all)
    int logits_rows = 0;        // rows valid from the last eval
    LmDevState* stt = nullptr;  // device
    SamplerDev* samp = nullptr; // device
    SampWork* swork = nullptr;  // device: sampler histogram + candidate list
    LmDevState* h_stt = nullptr;   // pinned host staging (ids, n_tokens, m in; out_token back)
    int* h_probe = nullptr;        // pinned: [0, 64) probe ids in, [64, 128) their probabilities back (rca_lm_step_probe)
    int n_tokens = 0;           // host mirror (llama_cpp.Llama.n_tokens)
    bool sampler_set = false;
    bool samp_full = false;     // top_k <= 0 or > SAMP_MAXK: the whole-vocabulary (Gumbel-max) sampler launches instead of the top-k ones
    bool samp_patch = false, samp_big_k = false, samp_big_p = false;   // which other sampler launches a captured step holds (rca_lm_sampler_init)
    bool samp_typ = false;      // rca_lm_sampler_set_typical in force on the serial chain: samp_final_typ_kernel closes it
    bool samp_miro = false;     // rca_lm_sampler_set_mirostat(2) in force (temp > 0): the samp_miro_* launches, whatever top_k says
    SamplerDev samp_host = {};  // what h->samp holds (rca_lm_sampler_init; the two calls above change single fields)
    // captured steady-state steps (n = 1, 2)
    // decode-step graphs per (tokens 1..2, context bucket): bucket b launches min(n_splits, 4 << b) attention splits
    // Two sets: the handle's KV cache can be exchanged with a twin's (rca_lm_swap_kv) and the cache address is baked into the
    // captured kernel nodes, so a set remembers the cache it was captured over (at most two caches ever rotate through a handle).
    struct GraphSet { const f16_t* kc = nullptr; hipGraphExec_t g[3][LM_GRAPH_BUCKETS] = {}; hipGraphExec_t fg[LM_FRAME_MAX + 1][LM_GRAPH_BUCKETS] = {};
                      hipGraphExec_t gp[3][LM_GRAPH_BUCKETS] = {}; int gp_nprobe[3][LM_GRAPH_BUCKETS] = {};   // step + token probabilities (rca_lm_step_probe)
                      // rca_lm_eval_async passes of ONE prefill tile (the shadow cache's background tiles): tokens of the pass -> graph.  The
                      // flash attention of the tile path takes the context from the device state, so one graph serves every position.
                      int tile_m[2] = {0, 0}; hipGraphExec_t tile_g[2] = {nullptr, nullptr}; int tile_seen[2] = {0, 0};
                      unsigned long long last_use = 0; };
    GraphSet gset[2];
    unsigned long long gset_clock = 0;
    bool async_pending = false;   // an rca_lm_eval_async pass may still be running on the stream
    // rca_lm_batch_eval: a pass on ANOTHER handle's stream (the call's workspace) may still be writing this handle's cache, state and
    // logits.  The call records be_event (this handle's own, made by its first call) behind its last pass; whatever waits for
    // async_pending waits for it too (lm_wait_batch_eval), so the event outlives the workspace and nothing points at it.
    bool be_pending = false;
    hipEvent_t be_event = nullptr;
    struct LmEvalStage* be_dev = nullptr;   // as the workspace of rca_lm_batch_eval: the pass's block on the device ...
    struct LmEvalStage* be_pin = nullptr;   // ... and its pinned staging copy (made by the first call)
    hipGraphExec_t be_g[LM_MAXM / 128][2] = {};   // ... and its captured passes, per (token blocks of the pass, KV format of the handles)
    int be_seen[LM_MAXM / 128][2] = {};           //     passes of that geometry so far: the first runs eagerly, the second is captured
    unsigned long long rng_host = 0;   // host mirror of the device's draw counter (restored when a frame graph is cut short)
    bool graphs_enabled = true;
    unsigned long long graph_epoch = 0;   // bumped by whatever invalidates graphs captured over this handle (lm_drop_graphs, rca_lm_swap_kv): a group
                                          // (rca_lm_group_step) holds graphs over SEVERAL handles and compares before it replays one
    unsigned long long drop_epoch = 0;    // bumped by lm_drop_graphs alone: a selection frame's graphs (rca_lm_batch_frame_sel) hold no cache pointer and
                                          // outlive rca_lm_swap_kv, but not a moved buffer or another sampler chain
    bool mfma_prefill = true;   // evals longer than LM_PREFILL_MIN tokens use the bf16 MFMA tiles
    bool fuse_attn = true;      // decode steps merge the attention splits inside the attention launch (rca_lm_set_attn_fuse)
    int act_format = 0;         // activations of the decode GEMVs over packed matrices: 0 f32, 1 q8_1 blocks + integer dots (rca_lm_set_act_format)
    int gemv_last[8] = {};      // tests only (rca_lm_gemv_tap_form): M, NIT, R, batches per workgroup, grid, format, ACT and N of the last launch_gemv_r
    // weight sharing (rca_lm_create_shared): a borrower points at the handle that owns the weights and the RoPE tables; an owner
    // destroyed while borrowers are alive keeps those allocations (and its struct) until the last borrower is gone
    rca_lm* weights_of = nullptr;
    int borrowers = 0;
    bool zombie = false;
    struct DuplexState* duplex = nullptr;   // rca_duplex_frame: buffers + graphs of the one-replay frame
    // rca_lm_score: allocated by the first call that needs them, freed with the handle
    float* sc_blk = nullptr;                 // the logits of one 128-token block [128][V]
    rca_score_row_t* sc_rows = nullptr;      // device rows of a call + its targets behind them
    int* sc_tgt = nullptr;
    long sc_rows_cap = 0;
    char* sc_pin = nullptr;                  // pinned: the (n_tokens, m, ids) block of EVERY pass of a call, so no pass waits for the one before
    size_t sc_pin_cap = 0;
    hipEvent_t sc_ready = nullptr, sc_free = nullptr;   // base: block logits written; scored handle: block logits consumed
    // rca_lm_imatrix_begin .. rca_lm_imatrix_end: the importance matrix's accumulators -- this handle's own, never a twin's
    double* imx_acc = nullptr;               // n_layers * (H + AO + H + F) + H column sums (lm_imx_slot); null: not collecting
    long imx_count = 0;                      // tokens summed
    int imx_tap_layer = -1, imx_tap_kind = -1;            // rca_lm_imatrix_chunk_tap: the planes of this (layer, kind) are copied to
    bf16_t *imx_tap_h = nullptr, *imx_tap_l = nullptr;    // these buffers right behind their collection launch
};
// an rca_lm_batch_eval pass over this handle may still be running on its workspace's stream: wait for it (every place that waits for
// the handle's own stream before it reads or changes the handle does)
static int lm_wait_batch_eval(rca_lm* h) {
    if (h->be_pending) {
        RCA_HIP(hipSetDevice(h->device));
        RCA_HIP(hipEventSynchronize(h->be_event));
        h->be_pending = false;
    }
    return RCA_OK;
}
// ---- the two KV formats behind one pair of pointers (kv_layer_stride: elements of a layer = bytes of a layer's int8 plane)
static bool lm_kv_q8(const rca_lm* h) { return h->kv_format == 1; }
static size_t lm_kv_plane_bytes(const rca_lm* h) {
    const size_t n = (size_t)h->cfg.n_layers * h->kv_layer_stride;
    return lm_kv_q8(h) ? n + n / 32 * sizeof(f16_t) : n * sizeof(f16_t);
}
static long lm_kv_sc_off(const rca_lm* h) { return (long)h->cfg.n_layers * h->kv_layer_stride; }   // q8_0: bytes from kc / vc to the scales
template <class T>
static T* lm_kv_layer(const rca_lm* h, T* base, int l) {   // layer l of kc / vc as the attention kernels take it
    return lm_kv_q8(h) ? reinterpret_cast<T*>((char*)base + (long)l * h->kv_layer_stride) : base + (long)l * h->kv_layer_stride;
}
static const f16_t* lm_kv_scales(const rca_lm* h, const f16_t* base, int l) {   // q8_0: the scales of layer l
    return reinterpret_cast<const f16_t*>((const char*)base + lm_kv_sc_off(h)) + (long)l * (h->kv_layer_stride >> 5);
}
static int lm_kv_bytes_per_pos(const rca_lm* h) {
    const int per_row = lm_kv_q8(h) ? 64 + 2 * (int)sizeof(f16_t) : 64 * (int)sizeof(f16_t);
    return 2 * h->cfg.n_layers * h->cfg.n_kv_heads * per_row;
}
// where the QKV epilogues of layer l store their fp16 rows: the cache itself, or the ring
static void lm_rope_target(const rca_lm* h, int l, GemvRope& rope) {
    if (lm_kv_q8(h)) { rope.kc = h->ring_k; rope.vc = h->ring_v; rope.pos_mask = LM_KV_RING - 1; }
    else { rope.kc = h->kc + (long)l * h->kv_layer_stride; rope.vc = h->vc + (long)l * h->kv_layer_stride; rope.pos_mask = -1; }
}
static LmGroupRow lm_group_row(const rca_lm* h, int j, int xrow) {
    if (lm_kv_q8(h)) return LmGroupRow{h->stt, h->ring_k, h->ring_v, h->logits, 0, j, xrow, h->cfg.n_ctx, LM_KV_RING - 1};
    return LmGroupRow{h->stt, h->kc, h->vc, h->logits, h->kv_layer_stride, j, xrow, h->cfg.n_ctx, -1};
}
static int lm_alloc(void** p, size_t bytes);
// (re)allocate the cache in the handle's format, zeroed
static int lm_kv_alloc(rca_lm* h) {
    int rc;
    for (f16_t** p : {&h->kc, &h->vc, &h->ring_k, &h->ring_v})
        if (*p) { (void)hipFree(*p); *p = nullptr; }
    const size_t kvb = lm_kv_plane_bytes(h);
    if (lm_kv_q8(h) && (kvb >> 35) != 0) return fail(RCA_ERR_ARG, "q8_0 KV cache: %zu bytes per tensor (the scale offset is passed in 16-byte units as an int)", kvb);
    if ((rc = lm_alloc((void**)&h->kc, kvb)) != RCA_OK) return rc;
    if ((rc = lm_alloc((void**)&h->vc, kvb)) != RCA_OK) return rc;
    RCA_HIP(hipMemsetAsync(h->kc, 0, kvb, h->stream));
    RCA_HIP(hipMemsetAsync(h->vc, 0, kvb, h->stream));
    if (lm_kv_q8(h)) {
        const size_t rb = (size_t)LM_KV_RING * h->cfg.n_kv_heads * 64 * sizeof(f16_t);
        if ((rc = lm_alloc((void**)&h->ring_k, rb)) != RCA_OK) return rc;
        if ((rc = lm_alloc((void**)&h->ring_v, rb)) != RCA_OK) return rc;
        RCA_HIP(hipMemsetAsync(h->ring_k, 0, rb, h->stream));
        RCA_HIP(hipMemsetAsync(h->ring_v, 0, rb, h->stream));
    }
    return RCA_OK;
}
struct DuplexState;
static void duplex_destroy(DuplexState* d);
static void duplex_drop_graphs(DuplexState* d);

static int lm_alloc(void** p, size_t bytes) {
    hipError_t e = hipMalloc(p, bytes);
    if (e != hipSuccess) return fail(RCA_ERR_HIP, "hipMalloc(%zu) -> %s", bytes, hipGetErrorString(e));
    return RCA_OK;
}

static void lm_free_weights(rca_lm* h) {
    for (auto& L : h->layers) {
        for (WMat* m : {&L.qkv, &L.o, &L.gu, &L.down, &L.vseg}) m->release();
        for (void* p : {(void*)L.attn_norm, (void*)L.ffn_norm})
            if (p) (void)hipFree(p);
    }
    h->head.release();
    for (void* p : {(void*)h->embed, (void*)h->final_norm, (void*)h->cos_t, (void*)h->sin_t, (void*)h->kv_stage_many})
        if (p) (void)hipFree(p);
    h->layers.clear();
    h->embed = nullptr;
    h->final_norm = h->cos_t = h->sin_t = nullptr;
    h->kv_stage_many = nullptr;
}

// The captured step graphs carry the addresses of the logits buffer, the KV cache and the workspace in their kernel nodes:
// whenever one of those is reallocated (or the handle goes away) every captured graph has to go with it.
static void lm_drop_graph_set(rca_lm::GraphSet& gs) {
    for (int i = 0; i < 3; ++i)
        for (int b = 0; b < LM_GRAPH_BUCKETS; ++b) {
            if (gs.g[i][b]) { (void)hipGraphExecDestroy(gs.g[i][b]); gs.g[i][b] = nullptr; }
            if (gs.gp[i][b]) { (void)hipGraphExecDestroy(gs.gp[i][b]); gs.gp[i][b] = nullptr; }
        }
    for (int i = 0; i <= LM_FRAME_MAX; ++i)
        for (int b = 0; b < LM_GRAPH_BUCKETS; ++b)
            if (gs.fg[i][b]) { (void)hipGraphExecDestroy(gs.fg[i][b]); gs.fg[i][b] = nullptr; }
    for (int i = 0; i < 2; ++i) {
        if (gs.tile_g[i]) { (void)hipGraphExecDestroy(gs.tile_g[i]); gs.tile_g[i] = nullptr; }
        gs.tile_m[i] = gs.tile_seen[i] = 0;
    }
    gs.kc = nullptr;
}
static void lm_drop_graphs(rca_lm* h) {
    h->graph_epoch++;
    h->drop_epoch++;
    for (auto& gs : h->gset) lm_drop_graph_set(gs);
    for (auto& per_tbz : h->be_g)
        for (hipGraphExec_t& e : per_tbz)
            if (e) { (void)hipGraphExecDestroy(e); e = nullptr; }
    memset(h->be_seen, 0, sizeof(h->be_seen));
    duplex_drop_graphs(h->duplex);
}
// the graph set captured over the KV cache that is installed now (evicting the older set if neither matches)
static rca_lm::GraphSet& lm_graph_set(rca_lm* h) {
    rca_lm::GraphSet* hit = nullptr;
    for (auto& gs : h->gset)
        if (gs.kc == h->kc) hit = &gs;
    if (!hit) {
        hit = h->gset[0].last_use <= h->gset[1].last_use ? &h->gset[0] : &h->gset[1];
        lm_drop_graph_set(*hit);
        hit->kc = h->kc;
    }
    hit->last_use = ++h->gset_clock;
    return *hit;
}
// Capture what `enqueue` (a callable returning an rca status) puts on `st` into *exec, in thread-local mode so that other threads'
// HIP calls do not break it.  The capture is ended whether or not `enqueue` failed; its failure is returned as it is.  *exec stays
// null unless the graph was instantiated; the upload makes the device-side copy now, not inside the first frame that replays it
// (pre-captured graphs: first trim frame, first frame of a bucket).  `tag` names the caller in the error text.
template <class F>
static int lm_capture(hipStream_t st, hipGraphExec_t* exec, const char* tag, F&& enqueue) {
    hipGraph_t g = nullptr;
    RCA_HIP(hipStreamSynchronize(st));
    RCA_HIP(hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal));
    const int rc = enqueue();
    hipError_t e = hipStreamEndCapture(st, &g);
    if (rc != RCA_OK) { if (g) (void)hipGraphDestroy(g); return rc; }
    if (e != hipSuccess) return fail(RCA_ERR_HIP, "%s capture: %s", tag, hipGetErrorString(e));
    e = hipGraphInstantiate(exec, g, nullptr, nullptr, 0);
    (void)hipGraphDestroy(g);
    if (e != hipSuccess) { *exec = nullptr; return fail(RCA_ERR_HIP, "%s graph instantiate: %s", tag, hipGetErrorString(e)); }
    (void)hipGraphUpload(*exec, st);
    return RCA_OK;
}

extern "C" int rca_lm_destroy(rca_lm_t* h) {
    if (!h) return RCA_OK;
    (void)hipSetDevice(h->device);
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    (void)lm_wait_batch_eval(h);
    if (h->be_event) { (void)hipEventDestroy(h->be_event); h->be_event = nullptr; }
    if (h->be_dev) { (void)hipFree(h->be_dev); h->be_dev = nullptr; }
    if (h->be_pin) { (void)hipHostFree(h->be_pin); h->be_pin = nullptr; }
    lm_drop_graphs(h);
    duplex_destroy(h->duplex);
    h->duplex = nullptr;
    for (void* p : {(void*)h->kc, (void*)h->vc, (void*)h->ring_k, (void*)h->ring_v, (void*)h->kv_stage, (void*)h->x, (void*)h->xn, (void*)h->qkv, (void*)h->attn, (void*)h->hbuf,
                    (void*)h->att_part, (void*)h->logits, (void*)h->probs_dev, (void*)h->probe_ids_dev, (void*)h->att_arrive, (void*)h->xh, (void*)h->xl,
                    (void*)h->gpart, (void*)h->stt, (void*)h->samp, (void*)h->swork})
        if (p) (void)hipFree(p);
    h->kc = h->vc = h->kv_stage = h->ring_k = h->ring_v = nullptr;
    h->x = h->xn = h->qkv = h->attn = h->hbuf = h->att_part = h->logits = h->probs_dev = h->gpart = nullptr;
    h->probe_ids_dev = nullptr; h->att_arrive = nullptr; h->xh = h->xl = nullptr; h->stt = nullptr; h->samp = nullptr; h->swork = nullptr;
    if (h->h_stt) { (void)hipHostFree(h->h_stt); h->h_stt = nullptr; }
    if (h->h_probe) { (void)hipHostFree(h->h_probe); h->h_probe = nullptr; }
    for (void* p : {(void*)h->sc_blk, (void*)h->sc_rows, (void*)h->sc_tgt})
        if (p) (void)hipFree(p);
    h->sc_blk = nullptr; h->sc_rows = nullptr; h->sc_tgt = nullptr;
    if (h->sc_pin) { (void)hipHostFree(h->sc_pin); h->sc_pin = nullptr; }
    if (h->imx_acc) { (void)hipFree(h->imx_acc); h->imx_acc = nullptr; }
    if (h->sc_ready) { (void)hipEventDestroy(h->sc_ready); h->sc_ready = nullptr; }
    if (h->sc_free) { (void)hipEventDestroy(h->sc_free); h->sc_free = nullptr; }
    if (h->stream) { (void)hipStreamDestroy(h->stream); h->stream = nullptr; }
    if (h->weights_of) {            // borrower: the weights belong to someone else
        rca_lm* owner = h->weights_of;
        h->layers.clear();
        if (--owner->borrowers == 0 && owner->zombie) { lm_free_weights(owner); delete owner; }
        delete h;
        return RCA_OK;
    }
    if (h->borrowers > 0) {         // owner with live borrowers: keep the weights until the last one goes
        h->zombie = true;
        return RCA_OK;
    }
    lm_free_weights(h);
    delete h;
    return RCA_OK;
}

static int lm_check_cfg(const rca_lm_config_t* c) {
    if (!c) return fail(RCA_ERR_ARG, "null config");
    if (c->head_dim != 64) return fail(RCA_ERR_ARG, "head_dim must be 64 (got %d)", c->head_dim);
    if (c->n_kv_heads < 1 || c->n_heads % c->n_kv_heads) return fail(RCA_ERR_ARG, "n_heads must be a multiple of n_kv_heads");
    const int G = c->n_heads / c->n_kv_heads;
    if (G != 1 && G != 2 && G != 4) return fail(RCA_ERR_ARG, "query group size %d unsupported (1, 2, 4)", G);
    if (c->hidden % 8 || c->ffn % 8 || (c->n_heads * c->head_dim) % 8) return fail(RCA_ERR_ARG, "hidden/ffn must be multiples of 8");
    if (c->hidden > LM_KSLICE || c->n_heads * c->head_dim > LM_KSLICE) return fail(RCA_ERR_ARG, "hidden > %d unsupported", LM_KSLICE);
    if (c->ffn > LM_KSLICE * LM_MAXSPLIT) return fail(RCA_ERR_ARG, "ffn > %d unsupported", LM_KSLICE * LM_MAXSPLIT);
    if (c->ffn > LM_KSLICE && c->ffn % LM_KSLICE) return fail(RCA_ERR_ARG, "ffn above %d must be a multiple of it", LM_KSLICE);
    if (c->vocab_size < 2 || c->n_layers < 1 || c->n_ctx < 2) return fail(RCA_ERR_ARG, "bad sizes");
    if (c->decode_weights < 0 || c->decode_weights >= DW_COUNT) return fail(RCA_ERR_ARG, "decode_weights %d (0 as supplied, 1 q8_0, 2 f16, 3 q4_k, 4 q5_k, 5 q4_0, 6 q4_1, 7 iq4_nl)", c->decode_weights);
    return RCA_OK;
}

// A source tensor on the device in its "plain" form (row-major, one array per component), before fusion (q;k;v rows, gate/up rows
// interleaved) and before the GEMV layout is built.
struct RawMat {
    int fmt = WF_BF16;
    long rows = 0, cols = 0;
    bf16_t* w16 = nullptr;      // WF_BF16 / WF_F16
    signed char* q = nullptr;   // WF_Q8: int8 [rows][cols]; WF_Q4K / WF_Q5K: one byte per 4-bit / 5-bit value (the rest as WF_Q4K)
    f16_t* d = nullptr;         // WF_Q8: fp16 [rows][cols / 32]; WF_Q4K / WF_Q5K: ushort (sc | m << 8) [rows][cols / 32]
    unsigned* dd = nullptr;     // WF_Q4K / WF_Q5K: (d | dmin << 16) [rows][cols / 256]; WF_Q40 / WF_Q41: (s | t << 16) [rows][cols / 32] (q as WF_Q4K, d unused);
                                // WF_IQ4 / WF_IQ4XS: the f32 factor s (bits) [rows][cols / 32] (q: table indices, d unused)
    RawMat() = default;
    RawMat(const RawMat&) = delete;
    RawMat& operator=(const RawMat&) = delete;
    RawMat(RawMat&& o) noexcept { *this = std::move(o); }
    RawMat& operator=(RawMat&& o) noexcept {
        if (this != &o) {
            release();
            fmt = o.fmt; rows = o.rows; cols = o.cols;
            w16 = o.w16; q = o.q; d = o.d; dd = o.dd;
            o.w16 = nullptr; o.q = nullptr; o.d = nullptr; o.dd = nullptr;
        }
        return *this;
    }
    ~RawMat() { release(); }
    void release() {
        for (void* p : {(void*)w16, (void*)q, (void*)d, (void*)dd})
            if (p) (void)hipFree(p);
        w16 = nullptr; q = nullptr; d = nullptr; dd = nullptr;
    }
    void** array(int arr) const {   // the member a WA_* id of the table names
        return arr == WA_W16 ? (void**)&w16 : (arr == WA_Q ? (void**)&q : (arr == WA_D ? (void**)&d : (void**)&dd));
    }
    // (array, bytes per row) of every component
    int parts(void** ptr, long* row_bytes) const {
        int n = 0;
        for (const WfPart& p : WF_TABLE[fmt].plain)
            if (p.arr != WA_NONE) { ptr[n] = *array(p.arr); row_bytes[n++] = cols / p.per * p.bytes; }
        return n;
    }
    int alloc(int f, long r, long c) {
        const WfInfo& info = WF_TABLE[f];
        fmt = f; rows = r; cols = c;
        if (c % info.row_mult) return fail(RCA_ERR_ARG, "%s needs rows of a multiple of %d values (got %ld)", info.name, info.row_mult, c);
        int rc;
        for (const WfPart& p : info.plain)
            if (p.arr != WA_NONE && (rc = lm_alloc(array(p.arr), (size_t)r * (c / p.per * p.bytes))) != RCA_OK) { release(); return rc; }
        return RCA_OK;
    }
};
// A device scratch buffer of the load path, freed when its scope ends.
struct DevScratch {
    void* p = nullptr;
    DevScratch() = default;
    DevScratch(const DevScratch&) = delete;
    DevScratch& operator=(const DevScratch&) = delete;
    ~DevScratch() { if (p) (void)hipFree(p); }
    int alloc(size_t bytes) { return lm_alloc(&p, bytes); }
    void* take() { void* r = p; p = nullptr; return r; }
};

static const WfInfo* wf_of_blocks(int dtype) {   // the format a tensor of file blocks arrives as
    for (const WfInfo& f : WF_TABLE)
        if (wf_packed(f.id) && f.dtype == dtype) return &f;
    return nullptr;
}
// The kernels of a verb keep their own signatures: one switch per verb picks the launch.
static void lm_launch_unblock(hipStream_t s, int fmt, const unsigned char* blocks, long numel, RawMat* out, int* bad) {
    switch (fmt) {
        case WF_Q8: lm_q8_unblock_kernel<<<4096, 256, 0, s>>>(blocks, numel / 32, out->q, out->d); break;
        case WF_Q6K: lm_q6k_unblock_kernel<<<4096, 256, 0, s>>>(blocks, numel / 256, out->q, (signed char*)out->d, (f16_t*)out->dd); break;
        case WF_Q5K: lm_q5k_unblock_kernel<<<4096, 256, 0, s>>>(blocks, numel / 256, (unsigned char*)out->q, (unsigned short*)out->d, out->dd); break;
        case WF_Q4K: lm_q4k_unblock_kernel<<<4096, 256, 0, s>>>(blocks, numel / 256, (unsigned char*)out->q, (unsigned short*)out->d, out->dd); break;
        case WF_Q40: lm_q40_unblock_kernel<false><<<4096, 256, 0, s>>>(blocks, numel / 32, (unsigned char*)out->q, out->dd, bad); break;
        case WF_Q41: lm_q40_unblock_kernel<true><<<4096, 256, 0, s>>>(blocks, numel / 32, (unsigned char*)out->q, out->dd, bad); break;
        case WF_IQ4: lm_iq4_unblock_kernel<false><<<4096, 256, 0, s>>>(blocks, numel / 32, (unsigned char*)out->q, out->dd, bad); break;
        case WF_IQ4XS: lm_iq4_unblock_kernel<true><<<4096, 256, 0, s>>>(blocks, numel / 32, (unsigned char*)out->q, out->dd, bad); break;   // counts 32-value sub-blocks too
    }
}
static void lm_launch_dequant_f32(hipStream_t s, const RawMat& m, float* out, long numel) {
    switch (WF_TABLE[m.fmt].device) {
        case WF_Q8: lm_q8_dequant_f32_kernel<<<4096, 256, 0, s>>>(m.q, m.d, out, numel); break;
        case WF_Q6K: lm_q6k_dequant_f32_kernel<<<4096, 256, 0, s>>>(m.q, (const signed char*)m.d, (const f16_t*)m.dd, out, numel); break;
        case WF_Q4K: case WF_Q5K:   // the plain byte holds the whole value, 4 or 5 bits
            lm_q4k_dequant_f32_kernel<<<4096, 256, 0, s>>>((const unsigned char*)m.q, (const unsigned short*)m.d, m.dd, out, numel); break;
        case WF_Q40: lm_q40_dequant_f32_kernel<<<4096, 256, 0, s>>>((const unsigned char*)m.q, m.dd, out, numel); break;
        case WF_IQ4: lm_iq4_dequant_f32_kernel<<<4096, 256, 0, s>>>((const unsigned char*)m.q, m.dd, out, numel); break;
    }
}
static void lm_launch_quantize(hipStream_t s, int fmt, const RawMat& m, RawMat* qd, int* bad) {
    const int f16 = m.fmt == WF_F16;
    const long n = m.rows * m.cols;
    switch (fmt) {
        case WF_Q8: lm_q8_quantize_kernel<<<4096, 256, 0, s>>>(m.w16, f16, n / 32, qd->q, qd->d); break;
        case WF_Q4K: lm_q4k_quantize_kernel<15><<<4096, 256, 0, s>>>(m.w16, f16, n / 256, (unsigned char*)qd->q, (unsigned short*)qd->d, qd->dd); break;
        case WF_Q5K: lm_q4k_quantize_kernel<31><<<4096, 256, 0, s>>>(m.w16, f16, n / 256, (unsigned char*)qd->q, (unsigned short*)qd->d, qd->dd); break;
        case WF_Q40: lm_q40_quantize_kernel<false><<<4096, 256, 0, s>>>(m.w16, f16, n / 32, (unsigned char*)qd->q, qd->dd, bad); break;
        case WF_Q41: lm_q40_quantize_kernel<true><<<4096, 256, 0, s>>>(m.w16, f16, n / 32, (unsigned char*)qd->q, qd->dd, bad); break;
        case WF_IQ4: lm_iq4nl_quantize_kernel<<<4096, 256, 0, s>>>(m.w16, f16, n / 32, (unsigned char*)qd->q, qd->dd, bad); break;
    }
}
static void lm_launch_pack(hipStream_t s, const RawMat& m, int qkv_pairs, WMat* out) {
    const int N = out->N, K = out->K;
    switch (WF_TABLE[m.fmt].device) {
        case WF_Q8: lm_q8_pack_kernel<<<4096, 256, 0, s>>>(m.q, m.d, N, K, qkv_pairs, out->qs, out->sc); break;
        case WF_Q6K: lm_q6k_pack_kernel<<<4096, 256, 0, s>>>(m.q, (const signed char*)m.d, (const f16_t*)m.dd, N, K, qkv_pairs, out->qs, (float*)out->sc); break;
        case WF_Q4K:
            lm_q4k_pack_kernel<WF_Q4K><<<4096, 256, 0, s>>>((const unsigned char*)m.q, (const unsigned short*)m.d, m.dd, N, K, qkv_pairs, out->qs, (unsigned short*)out->sc, out->dd, nullptr);
            break;
        case WF_Q5K:
            lm_q4k_pack_kernel<WF_Q5K><<<4096, 256, 0, s>>>((const unsigned char*)m.q, (const unsigned short*)m.d, m.dd, N, K, qkv_pairs, out->qs, (unsigned short*)out->sc, out->dd, out->qh);
            break;
        case WF_Q40: case WF_IQ4:   // IQ4: the same arrays, the factor dword is an f32
            lm_q4k_pack_kernel<WF_Q40><<<4096, 256, 0, s>>>((const unsigned char*)m.q, nullptr, m.dd, N, K, qkv_pairs, out->qs, nullptr, out->sc, nullptr); break;
    }
}

// A tensor of file blocks (the GGUF blocks as they sit in the file) is unblocked into its plain form.
static int lm_upload_blocks(rca_lm* h, const rca_tensor_t* t, const WfInfo& info, long rows, long cols, RawMat* out) {
    int rc;
    if ((rc = out->alloc(info.id, rows, cols)) != RCA_OK) return rc;
    const long numel = rows * cols;
    const size_t nbytes = (size_t)(numel / info.blk_vals) * info.blk_bytes;
    DevScratch raw;   // the blocks, then (bad_flag) the flag "a block's factor is not finite in the form the kernels keep it in"
    if ((rc = raw.alloc(info.bad_flag ? nbytes + 8 : nbytes)) != RCA_OK) return rc;
    int* bad = info.bad_flag ? reinterpret_cast<int*>((unsigned char*)raw.p + ((nbytes + 3) & ~(size_t)3)) : nullptr;
    int bad_h = 0;
    hipError_t e = hipMemcpy(raw.p, t->data, nbytes, hipMemcpyHostToDevice);
    if (e == hipSuccess && bad) e = hipMemsetAsync(bad, 0, 4, h->stream);
    if (e == hipSuccess) {
        lm_launch_unblock(h->stream, info.id, (const unsigned char*)raw.p, numel, out, bad);
        if (bad) e = hipMemcpyAsync(&bad_h, bad, 4, hipMemcpyDeviceToHost, h->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    }
    if (e != hipSuccess) return fail(RCA_ERR_HIP, "upload '%s': %s", t->name, hipGetErrorString(e));
    if (bad_h && info.device == WF_Q40) return fail(RCA_ERR_ARG, "tensor '%s': a Q4_0 block's 8 d is not finite in fp16", t->name);   // Q4_1 is refused in these words too
    if (bad_h) return fail(RCA_ERR_ARG, "tensor '%s': an %s block's d is not finite", t->name, info.name);
    return RCA_OK;
}
// Uploads a matrix.  RCA_BF16 / RCA_F16 stay what they are; RCA_F32 is rounded to bf16 (nearest even: this build's storage format
// for 32-bit checkpoints); the quantised types go through lm_upload_blocks.
static int lm_upload_raw(rca_lm* h, const rca_tensor_t* ts, int nt, const std::string& name, long rows, long cols, RawMat* out) {
    const rca_tensor_t* t = find_tensor(ts, nt, name);
    const long numel = rows * cols;
    if (!t) return fail(RCA_ERR_MISSING, "tensor '%s' missing", name.c_str());
    if (t->numel != numel) return fail(RCA_ERR_ARG, "tensor '%s': numel %ld, expected %ld", name.c_str(), (long)t->numel, numel);
    int rc;
    if (const WfInfo* info = wf_of_blocks(t->dtype)) return lm_upload_blocks(h, t, *info, rows, cols, out);
    if (t->dtype == RCA_BF16 || t->dtype == RCA_F16) {
        if ((rc = out->alloc(t->dtype == RCA_F16 ? WF_F16 : WF_BF16, rows, cols)) != RCA_OK) return rc;
        RCA_HIP(hipMemcpy(out->w16, t->data, (size_t)numel * 2, hipMemcpyHostToDevice));
        return RCA_OK;
    }
    if (t->dtype != RCA_F32) return fail(RCA_ERR_ARG, "tensor '%s': dtype %d is not supported for a projection matrix", name.c_str(), t->dtype);
    if ((rc = out->alloc(WF_BF16, rows, cols)) != RCA_OK) return rc;
    DevScratch tmp;
    if ((rc = tmp.alloc((size_t)numel * 4)) != RCA_OK) return rc;
    hipError_t e = hipMemcpy(tmp.p, t->data, (size_t)numel * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        lm_f32_to_bf16_kernel<<<2048, 256, 0, h->stream>>>((const float*)tmp.p, out->w16, numel);
        e = hipStreamSynchronize(h->stream);
    }
    if (e != hipSuccess) return fail(RCA_ERR_HIP, "upload '%s': %s", name.c_str(), hipGetErrorString(e));
    return RCA_OK;
}
// The embedding table: never streamed, so it is kept exact -- f32 rows for RCA_F32 / RCA_F16 / RCA_Q8_0 sources, bf16 rows for RCA_BF16.
static int lm_upload_embed(rca_lm* h, const rca_tensor_t* ts, int nt, const std::string& name, long rows, long cols) {
    const rca_tensor_t* t = find_tensor(ts, nt, name);
    const long numel = rows * cols;
    if (!t) return fail(RCA_ERR_MISSING, "tensor '%s' missing", name.c_str());
    if (t->numel != numel) return fail(RCA_ERR_ARG, "tensor '%s': numel %ld, expected %ld", name.c_str(), (long)t->numel, numel);
    int rc;
    if (t->dtype == RCA_BF16) {
        h->embed_f32 = 0;
        if ((rc = lm_alloc(&h->embed, (size_t)numel * 2)) != RCA_OK) return rc;
        RCA_HIP(hipMemcpy(h->embed, t->data, (size_t)numel * 2, hipMemcpyHostToDevice));
        return RCA_OK;
    }
    h->embed_f32 = 1;
    if ((rc = lm_alloc(&h->embed, (size_t)numel * 4)) != RCA_OK) return rc;
    if (t->dtype == RCA_F32) {
        RCA_HIP(hipMemcpy(h->embed, t->data, (size_t)numel * 4, hipMemcpyHostToDevice));
        return RCA_OK;
    }
    if (t->dtype == RCA_F16) {
        DevScratch tmp;
        if ((rc = tmp.alloc((size_t)numel * 2)) != RCA_OK) return rc;
        hipError_t e = hipMemcpy(tmp.p, t->data, (size_t)numel * 2, hipMemcpyHostToDevice);
        if (e == hipSuccess) {
            lm_f16_to_f32_kernel<<<4096, 256, 0, h->stream>>>((const f16_t*)tmp.p, (float*)h->embed, numel);
            e = hipStreamSynchronize(h->stream);
        }
        if (e != hipSuccess) return fail(RCA_ERR_HIP, "upload '%s': %s", name.c_str(), hipGetErrorString(e));
        return RCA_OK;
    }
    if (const WfInfo* info = wf_of_blocks(t->dtype)) {
        RawMat raw;
        if ((rc = lm_upload_blocks(h, t, *info, rows, cols, &raw)) != RCA_OK) return rc;
        lm_launch_dequant_f32(h->stream, raw, (float*)h->embed, numel);
        hipError_t e = hipStreamSynchronize(h->stream);
        if (e != hipSuccess) return fail(RCA_ERR_HIP, "upload '%s': %s", name.c_str(), hipGetErrorString(e));
        return RCA_OK;
    }
    return fail(RCA_ERR_ARG, "tensor '%s': dtype %d is not supported for the embedding table", name.c_str(), t->dtype);
}
static int lm_upload_f32(const rca_tensor_t* ts, int nt, const std::string& name, long numel, float** out) {
    const rca_tensor_t* t = find_tensor(ts, nt, name);
    if (!t) return fail(RCA_ERR_MISSING, "tensor '%s' missing", name.c_str());
    if (t->numel != numel) return fail(RCA_ERR_ARG, "tensor '%s': numel %ld, expected %ld", name.c_str(), (long)t->numel, numel);
    int rc;
    if ((rc = lm_alloc((void**)out, (size_t)numel * 4)) != RCA_OK) return rc;
    if (t->dtype == RCA_BF16) {  // small tensors (norm weights): widen on the host
        std::vector<float> tmp((size_t)numel);
        const bf16_t* src = (const bf16_t*)t->data;
        for (long i = 0; i < numel; ++i) {
            const unsigned u = (unsigned)src[i] << 16;
            memcpy(&tmp[i], &u, 4);
        }
        RCA_HIP(hipMemcpy(*out, tmp.data(), (size_t)numel * 4, hipMemcpyHostToDevice));
    } else if (t->dtype == RCA_F32) {
        RCA_HIP(hipMemcpy(*out, t->data, (size_t)numel * 4, hipMemcpyHostToDevice));
    } else {
        return fail(RCA_ERR_ARG, "tensor '%s': norm weights must be f32 or bf16", name.c_str());
    }
    return RCA_OK;
}

// rca_lm_config_t::decode_weights (DW_*) applied to one plain matrix: q8_0 is quantised the way llama-quantize does, Q4_K / Q5_K by this
// build's quantiser, Q4_0 / Q4_1 by ggml's reference rule, IQ4_NL by this build's rule; DW_F16 converts bf16 to fp16.
// A matrix that ARRIVED quantised stays what it is.
static int lm_raw_convert(rca_lm* h, RawMat* m, int want) {
    if (want == DW_AS_SUPPLIED || wf_packed(m->fmt)) return RCA_OK;
    int rc;
    if (want == DW_F16) {
        if (m->fmt != WF_BF16) return RCA_OK;
        DevScratch out;
        if ((rc = out.alloc((size_t)m->rows * m->cols * 2)) != RCA_OK) return rc;
        lm_bf16_to_f16_kernel<<<4096, 256, 0, h->stream>>>(m->w16, (f16_t*)out.p, m->rows * m->cols);
        hipError_t e = hipStreamSynchronize(h->stream);
        (void)hipFree(m->w16);
        m->w16 = reinterpret_cast<bf16_t*>(out.take());
        m->fmt = WF_F16;
        if (e != hipSuccess) return fail(RCA_ERR_HIP, "fp16 conversion: %s", hipGetErrorString(e));
        return RCA_OK;
    }
    const WfInfo& info = WF_TABLE[DW_FORMAT[want]];
    RawMat qd;
    if ((rc = qd.alloc(info.id, m->rows, m->cols)) != RCA_OK) return rc;
    DevScratch bad;   // (bad_flag) the flag "a block's factor is not finite in fp16"
    int bad_h = 0;
    hipError_t e = hipSuccess;
    if (info.bad_flag) {
        if ((rc = bad.alloc(4)) != RCA_OK) return rc;
        e = hipMemsetAsync(bad.p, 0, 4, h->stream);
    }
    if (e == hipSuccess) {
        lm_launch_quantize(h->stream, info.id, *m, &qd, (int*)bad.p);
        if (info.bad_flag) e = hipMemcpyAsync(&bad_h, bad.p, 4, hipMemcpyDeviceToHost, h->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    }
    if (e != hipSuccess) return fail(RCA_ERR_HIP, "%s quantise: %s", info.name, hipGetErrorString(e));
    // (worded after the device form: Q4_1 is refused as Q4_0 is)
    if (bad_h) return fail(RCA_ERR_ARG, "%s quantise: a block's %sd is not finite in fp16", WF_TABLE[info.device].name, info.device == WF_Q40 ? "8 " : "");
    *m = std::move(qd);
    return RCA_OK;
}
// rows of `parts` stacked (q; k; v).  Parts of different formats cannot be fused.
static int lm_raw_concat(rca_lm* h, std::vector<RawMat*> parts, RawMat* out, const char* what) {
    long rows = 0;
    for (RawMat* p : parts) {
        if (p->fmt != parts[0]->fmt || p->cols != parts[0]->cols) return fail(RCA_ERR_ARG, "%s: its parts arrived in different formats", what);
        rows += p->rows;
    }
    int rc;
    if ((rc = out->alloc(parts[0]->fmt, rows, parts[0]->cols)) != RCA_OK) return rc;
    void* dp[3]; long drb[3];
    const int np = out->parts(dp, drb);
    long r0 = 0;
    for (RawMat* p : parts) {
        void* sp[3]; long srb[3];
        p->parts(sp, srb);
        for (int i = 0; i < np; ++i)
            RCA_HIP(hipMemcpyAsync((char*)dp[i] + r0 * drb[i], sp[i], (size_t)p->rows * srb[i], hipMemcpyDeviceToDevice, h->stream));
        r0 += p->rows;
    }
    RCA_HIP(hipStreamSynchronize(h->stream));
    return RCA_OK;
}
// dst row 2i = a row i, 2i+1 = b row i (gate/up: SwiGLU becomes an epilogue)
static int lm_raw_interleave(rca_lm* h, RawMat* a, RawMat* b, RawMat* out, const char* what) {
    if (a->fmt != b->fmt || a->cols != b->cols || a->rows != b->rows) return fail(RCA_ERR_ARG, "%s: its parts arrived in different formats", what);
    int rc;
    if ((rc = out->alloc(a->fmt, 2 * a->rows, a->cols)) != RCA_OK) return rc;
    void *dp[3], *ap[3], *bp[3]; long rb[3];
    const int np = out->parts(dp, rb);
    a->parts(ap, rb);
    b->parts(bp, rb);
    for (int i = 0; i < np; ++i)
        lm_interleave_rows_bytes_kernel<<<4096, 256, 0, h->stream>>>((const unsigned char*)ap[i], (const unsigned char*)bp[i], (unsigned char*)dp[i], a->rows, rb[i]);
    RCA_HIP(hipStreamSynchronize(h->stream));
    return RCA_OK;
}
// plain -> the layout the decode GEMV streams.  Takes ownership of `raw` (released or moved into `out`).
static int lm_finish_mat(rca_lm* h, RawMat* src, int qkv_pairs, WMat* out, const char* what) {
    RawMat raw = std::move(*src);   // freed when this returns
    const WfInfo& info = WF_TABLE[raw.fmt];
    const int N = (int)raw.rows, K = (int)raw.cols;
    out->fmt = raw.fmt; out->N = N; out->K = K;
    if (!wf_packed(raw.fmt)) {
        out->w = raw.w16;
        raw.w16 = nullptr;
        return RCA_OK;
    }
    if ((K % info.k_mult) || (N % info.n_mult) || (qkv_pairs && (N % 64)))
        return fail(RCA_ERR_ARG, "%s weights: %s is %d x %d (K must be a multiple of %d, N %s)", info.name, what, N, K, info.k_mult, info.n_word);
    for (int zero = 0; zero < 2; ++zero)   // every array is allocated, then the factor arrays are zeroed
        for (const WfPart& p : info.packed) {
            if (p.arr == WA_NONE) continue;
            const bool padded = p.arr == WA_SC || p.arr == WA_DD;   // the factor arrays: whole groups of 16 rows, zero padded
            const size_t bytes = (size_t)(padded ? (N + 15) / 16 * 16 : N) * (K / p.per * p.bytes);
            int rc;
            if (!zero && (rc = lm_alloc(out->array(p.arr), bytes)) != RCA_OK) return rc;
            if (zero && padded) (void)hipMemsetAsync(*out->array(p.arr), 0, bytes, h->stream);
        }
    lm_launch_pack(h->stream, raw, qkv_pairs, out);
    hipError_t e = hipStreamSynchronize(h->stream);
    if (e != hipSuccess) return fail(RCA_ERR_HIP, "%s pack of %s: %s", info.name, what, hipGetErrorString(e));
    return RCA_OK;
}

static int g128_splits(int N, int K);
static bool lm_can_gemm128(const rca_lm* h);
// the split partials of a handle: {m, l, o[64]} per query row (LM_MAXM tokens x up to 4 q heads of a kv head), kv head and split
static size_t lm_att_part_bytes(const rca_lm* h) { return (size_t)(LM_MAXM / 2) * h->cfg.n_kv_heads * h->n_splits * 8 * 66 * 4; }
static int lm_common_init(rca_lm* h, const rca_tensor_t* ts, int nt, const rca_lm* rope_src = nullptr) {
    const rca_lm_config_t& c = h->cfg;
    int rc;
    const int half = c.head_dim / 2;
    h->n_ctx_pad = (c.n_ctx + ATT_KEYS - 1) / ATT_KEYS * ATT_KEYS;
    h->n_splits = h->n_ctx_pad / ATT_KEYS;
    if (rope_src) {   // borrower: the owner's tables cover at least this context (checked by the caller)
        h->cos_t = rope_src->cos_t;
        h->sin_t = rope_src->sin_t;
    } else {
    // RoPE tables from inv_freq (supplied by the host layer exactly as HF computes it, or derived here)
    std::vector<float> inv(half);
    const rca_tensor_t* tinv = find_tensor(ts, nt, "rope.inv_freq");
    if (tinv) {
        if (tinv->numel != half || tinv->dtype != RCA_F32) return fail(RCA_ERR_ARG, "rope.inv_freq must hold %d f32", half);
        memcpy(inv.data(), tinv->data, half * sizeof(float));
    } else {
        for (int i = 0; i < half; ++i) {
            double f = 1.0 / pow((double)c.rope_theta, (double)(2 * i) / (double)c.head_dim);
            if (c.rope_scaling == 1) {
                const double low_wl = (double)c.rope_orig_ctx / c.rope_low_freq_factor;
                const double high_wl = (double)c.rope_orig_ctx / c.rope_high_freq_factor;
                const double wl = 2.0 * M_PI / f;
                if (wl > low_wl) f = f / c.rope_factor;
                else if (wl >= high_wl) {
                    const double smooth = ((double)c.rope_orig_ctx / wl - c.rope_low_freq_factor) / (c.rope_high_freq_factor - c.rope_low_freq_factor);
                    f = (1.0 - smooth) * f / c.rope_factor + smooth * f;
                }
            }
            inv[i] = (float)f;
        }
    }
    float* inv_dev = nullptr;
    if ((rc = lm_alloc((void**)&inv_dev, half * 4)) != RCA_OK) return rc;
    RCA_HIP(hipMemcpy(inv_dev, inv.data(), half * 4, hipMemcpyHostToDevice));
    if ((rc = lm_alloc((void**)&h->cos_t, (size_t)h->n_ctx_pad * half * 4)) != RCA_OK) return rc;
    if ((rc = lm_alloc((void**)&h->sin_t, (size_t)h->n_ctx_pad * half * 4)) != RCA_OK) return rc;
    lm_rope_table_kernel<<<cdiv((long)h->n_ctx_pad * half, 256), 256, 0, h->stream>>>(inv_dev, h->cos_t, h->sin_t, h->n_ctx_pad, half);
    RCA_HIP(hipStreamSynchronize(h->stream));
    (void)hipFree(inv_dev);
    }
    // KV cache
    h->kv_layer_stride = (long)h->n_ctx_pad * c.n_kv_heads * c.head_dim;
    if ((rc = lm_kv_alloc(h)) != RCA_OK) return rc;
    // activations
    const int H = c.hidden, QKV = (c.n_heads + 2 * c.n_kv_heads) * c.head_dim, AO = c.n_heads * c.head_dim;
    if ((rc = lm_alloc((void**)&h->x, (size_t)LM_MAXM * H * 4)) != RCA_OK) return rc;
    if ((rc = lm_alloc((void**)&h->xn, (size_t)LM_MAXM * H * 4)) != RCA_OK) return rc;
    if ((rc = lm_alloc((void**)&h->qkv, (size_t)LM_MAXM * QKV * 4)) != RCA_OK) return rc;
    if ((rc = lm_alloc((void**)&h->attn, (size_t)LM_MAXM * AO * 4)) != RCA_OK) return rc;
    if ((rc = lm_alloc((void**)&h->hbuf, (size_t)LM_MAXM * c.ffn * 4)) != RCA_OK) return rc;
    if ((rc = lm_alloc((void**)&h->att_part, lm_att_part_bytes(h))) != RCA_OK) return rc;
    h->logits_rows_cap = c.logits_all ? 64 : 1;
    if ((rc = lm_alloc((void**)&h->logits, (size_t)h->logits_rows_cap * c.vocab_size * 4)) != RCA_OK) return rc;
    if ((rc = lm_alloc((void**)&h->probs_dev, (64 + 2 * PROBS_SLICES) * 4)) != RCA_OK) return rc;   // [64 probs][slice (max, sum) pairs]
    if ((rc = lm_alloc((void**)&h->probe_ids_dev, 64 * 4)) != RCA_OK) return rc;
    {   // in-launch attention merge: 64 launch counters (tags start at 1: the zeroed granules match nothing), then the granules
        const size_t gb = ATT_EPOCH_INTS * 4 + (size_t)c.n_kv_heads * h->n_splits * 8 * 66 * 8;
        if ((rc = lm_alloc((void**)&h->att_arrive, gb)) != RCA_OK) return rc;
        RCA_HIP(hipMemsetAsync(h->att_arrive, 0, gb, h->stream));
        int ones[ATT_EPOCH_INTS];
        for (int i = 0; i < ATT_EPOCH_INTS; ++i) ones[i] = 1;
        RCA_HIP(hipMemcpyAsync(h->att_arrive, ones, sizeof(ones), hipMemcpyHostToDevice, h->stream));
        RCA_HIP(hipStreamSynchronize(h->stream));
    }
    {
        const size_t kmax = (size_t)std::max(std::max(H, AO), c.ffn);
        if ((rc = lm_alloc((void**)&h->xh, (size_t)LM_MAXM * kmax * 2)) != RCA_OK) return rc;
        if ((rc = lm_alloc((void**)&h->xl, (size_t)LM_MAXM * kmax * 2)) != RCA_OK) return rc;
        RCA_HIP(hipMemsetAsync(h->xh, 0, (size_t)LM_MAXM * kmax * 2, h->stream));
        RCA_HIP(hipMemsetAsync(h->xl, 0, (size_t)LM_MAXM * kmax * 2, h->stream));
        // k-split partial sums [split][N][LM_MAXM] of the 128-row GEMMs (lm_enqueue_prefill_tile128); other models never touch the buffer
        size_t part_rows = 64;   // largest split count x N over the four projections
        if (lm_can_gemm128(h)) {
            const int Fq = c.ffn;
            const int nk[4][2] = {{QKV, H}, {H, AO}, {2 * Fq, H}, {H, Fq}};
            for (int i = 0; i < 4; ++i) {
                const int ns = g128_splits(nk[i][0], nk[i][1]);
                if (ns > 1) part_rows = std::max(part_rows, (size_t)ns * nk[i][0]);
            }
        }
        if ((rc = lm_alloc((void**)&h->gpart, part_rows * LM_MAXM * 4)) != RCA_OK) return rc;
    }
    if ((rc = lm_alloc((void**)&h->stt, sizeof(LmDevState))) != RCA_OK) return rc;
    if ((rc = lm_alloc((void**)&h->samp, sizeof(SamplerDev))) != RCA_OK) return rc;
    RCA_HIP(hipMemsetAsync(h->stt, 0, sizeof(LmDevState), h->stream));
    RCA_HIP(hipMemsetAsync(h->samp, 0, sizeof(SamplerDev), h->stream));
    if ((rc = lm_alloc((void**)&h->swork, sizeof(SampWork))) != RCA_OK) return rc;
    RCA_HIP(hipMemsetAsync(h->swork, 0, sizeof(SampWork), h->stream));
    RCA_HIP(hipHostMalloc((void**)&h->h_stt, sizeof(LmDevState), hipHostMallocDefault));
    memset(h->h_stt, 0, sizeof(LmDevState));
    RCA_HIP(hipHostMalloc((void**)&h->h_probe, 128 * 4, hipHostMallocDefault));   // at creation: a pinned allocation inside a frame costs milliseconds
    memset(h->h_probe, 0, 128 * 4);
    RCA_HIP(hipStreamSynchronize(h->stream));
    return RCA_OK;
}

static int lm_new(const rca_lm_config_t* cfg, int device, rca_lm** out) {
    int rc;
    if ((rc = lm_check_cfg(cfg)) != RCA_OK) return rc;
    RCA_HIP(hipSetDevice(device));
    rca_lm* h = new rca_lm();
    h->cfg = *cfg;
    h->device = device;
    if (hipDeviceGetAttribute(&h->n_cus, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || h->n_cus <= 0) h->n_cus = 256;
    h->layers.resize(cfg->n_layers);
    if (hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking) != hipSuccess) {
        delete h;
        return fail(RCA_ERR_HIP, "stream create");
    }
    *out = h;
    return RCA_OK;
}

// Fusions + GEMV layouts of one layer from its seven plain matrices (which are consumed).
static int lm_build_layer(rca_lm* h, LmLayer& L, RawMat& q, RawMat& k, RawMat& v, RawMat& o, RawMat& g, RawMat& u, RawMat& dn) {
    const int want = h->cfg.decode_weights;
    int rc = RCA_OK;
    RawMat qkv, gu;
    for (RawMat* m : {&q, &k, &v, &o, &g, &u, &dn})
        if ((rc = lm_raw_convert(h, m, want)) != RCA_OK) return rc;
    if (q.fmt == k.fmt && k.fmt != v.fmt) {   // llama-quantize Q4_K_M: attn_v is Q6_K in the layers use_more_bits() picks, attn_q / attn_k Q4_K
        if ((rc = lm_raw_concat(h, {&q, &k}, &qkv, "the fused QK projection")) != RCA_OK) return rc;
        if ((rc = lm_finish_mat(h, &v, 1, &L.vseg, "v_proj")) != RCA_OK) return rc;
        L.split_v = true;
    } else if ((rc = lm_raw_concat(h, {&q, &k, &v}, &qkv, "the fused QKV projection")) != RCA_OK) return rc;
    q.release(); k.release(); v.release();   // (before the next matrices are built: the peak of device memory at load)
    if ((rc = lm_raw_interleave(h, &g, &u, &gu, "the fused gate/up projection")) != RCA_OK) return rc;
    g.release(); u.release();
    if ((rc = lm_finish_mat(h, &qkv, 1, &L.qkv, "the fused QKV projection")) != RCA_OK) return rc;
    if ((rc = lm_finish_mat(h, &o, 0, &L.o, "o_proj")) != RCA_OK) return rc;
    if ((rc = lm_finish_mat(h, &gu, 0, &L.gu, "the fused gate/up projection")) != RCA_OK) return rc;
    return lm_finish_mat(h, &dn, 0, &L.down, "down_proj");
}

extern "C" int rca_lm_create(const rca_lm_config_t* cfg, const rca_tensor_t* ts, int32_t nt, int32_t device, rca_lm_t** out) {
    if (!ts || !out) return fail(RCA_ERR_ARG, "null argument");
    rca_lm* h = nullptr;
    int rc;
    if ((rc = lm_new(cfg, device, &h)) != RCA_OK) return rc;
    auto bail = [&](int code) { rca_lm_destroy(h); return code; };
    const rca_lm_config_t& c = h->cfg;
    const long H = c.hidden, V = c.vocab_size, F = c.ffn, Q = (long)c.n_heads * c.head_dim, KVD = (long)c.n_kv_heads * c.head_dim;
    if ((rc = lm_upload_embed(h, ts, nt, "model.embed_tokens.weight", V, H)) != RCA_OK) return bail(rc);
    {
        RawMat ph;
        if ((rc = lm_upload_raw(h, ts, nt, "lm_head.weight", V, H, &ph)) != RCA_OK) return bail(rc);
        if ((rc = lm_raw_convert(h, &ph, c.decode_weights)) != RCA_OK) return bail(rc);
        if ((rc = lm_finish_mat(h, &ph, 0, &h->head, "lm_head")) != RCA_OK) return bail(rc);
    }
    if ((rc = lm_upload_f32(ts, nt, "model.norm.weight", H, &h->final_norm)) != RCA_OK) return bail(rc);
    for (int l = 0; l < c.n_layers; ++l) {
        const std::string p = "model.layers." + std::to_string(l) + ".";
        LmLayer& L = h->layers[l];
        RawMat q, k, v, o, g, u, dn;
        if ((rc = lm_upload_raw(h, ts, nt, p + "self_attn.q_proj.weight", Q, H, &q)) != RCA_OK ||
            (rc = lm_upload_raw(h, ts, nt, p + "self_attn.k_proj.weight", KVD, H, &k)) != RCA_OK ||
            (rc = lm_upload_raw(h, ts, nt, p + "self_attn.v_proj.weight", KVD, H, &v)) != RCA_OK ||
            (rc = lm_upload_raw(h, ts, nt, p + "self_attn.o_proj.weight", H, Q, &o)) != RCA_OK ||
            (rc = lm_upload_raw(h, ts, nt, p + "mlp.gate_proj.weight", F, H, &g)) != RCA_OK ||
            (rc = lm_upload_raw(h, ts, nt, p + "mlp.up_proj.weight", F, H, &u)) != RCA_OK ||
            (rc = lm_upload_raw(h, ts, nt, p + "mlp.down_proj.weight", H, F, &dn)) != RCA_OK)
            return bail(rc);
        if ((rc = lm_build_layer(h, L, q, k, v, o, g, u, dn)) != RCA_OK) return bail(rc);
        if ((rc = lm_upload_f32(ts, nt, p + "input_layernorm.weight", H, &L.attn_norm)) != RCA_OK) return bail(rc);
        if ((rc = lm_upload_f32(ts, nt, p + "post_attention_layernorm.weight", H, &L.ffn_norm)) != RCA_OK) return bail(rc);
    }
    if ((rc = lm_common_init(h, ts, nt)) != RCA_OK) return bail(rc);
    *out = h;
    return RCA_OK;
}

extern "C" int rca_lm_create_random(const rca_lm_config_t* cfg, uint64_t seed, float init_std, int32_t device, rca_lm_t** out) {
    if (!out) return fail(RCA_ERR_ARG, "null argument");
    rca_lm* h = nullptr;
    int rc;
    if ((rc = lm_new(cfg, device, &h)) != RCA_OK) return rc;
    auto bail = [&](int code) { rca_lm_destroy(h); return code; };
    const rca_lm_config_t& c = h->cfg;
    const long H = c.hidden, V = c.vocab_size, F = c.ffn, Q = (long)c.n_heads * c.head_dim, KVD = (long)c.n_kv_heads * c.head_dim;
    const float scale = init_std * 1.7320508f / 65535.0f;
    unsigned long long tid = 1;
    // every matrix is generated as bf16 values (hash of (seed, tensor id, element)), then brought into the requested decode format
    // the way a converter would from a bf16 checkpoint
    auto rnd = [&](long rows, long cols, int qkv_pairs, WMat* dst, const char* what) -> int {
        RawMat m;
        int r = m.alloc(WF_BF16, rows, cols);
        if (r != RCA_OK) return r;
        lm_random_bf16_kernel<<<4096, 256, 0, h->stream>>>(m.w16, rows * cols, seed, tid++, scale);
        if ((r = lm_raw_convert(h, &m, c.decode_weights)) != RCA_OK) return r;
        return lm_finish_mat(h, &m, qkv_pairs, dst, what);
    };
    auto ones = [&](float** p, long n) -> int {
        int r = lm_alloc((void**)p, (size_t)n * 4);
        if (r != RCA_OK) return r;
        lm_fill_f32_kernel<<<cdiv(n, 256), 256, 0, h->stream>>>(*p, n, 1.0f);
        return RCA_OK;
    };
    // tensor ids: 1 embed, 2 head, then per layer 10*l + {3 qkv, 4 o, 5 gate/up(interleaved), 6 down}
    h->embed_f32 = 0;
    if ((rc = lm_alloc(&h->embed, (size_t)V * H * 2)) != RCA_OK) return bail(rc);
    lm_random_bf16_kernel<<<4096, 256, 0, h->stream>>>((bf16_t*)h->embed, V * H, seed, tid++, scale);
    if ((rc = rnd(V, H, 0, &h->head, "lm_head")) != RCA_OK || (rc = ones(&h->final_norm, H)) != RCA_OK) return bail(rc);
    for (int l = 0; l < c.n_layers; ++l) {
        LmLayer& L = h->layers[l];
        tid = 10ull * (l + 1) + 3;
        if ((rc = rnd(Q + 2 * KVD, H, 1, &L.qkv, "the fused QKV projection")) != RCA_OK || (rc = rnd(H, Q, 0, &L.o, "o_proj")) != RCA_OK ||
            (rc = rnd(2 * F, H, 0, &L.gu, "the fused gate/up projection")) != RCA_OK || (rc = rnd(H, F, 0, &L.down, "down_proj")) != RCA_OK ||
            (rc = ones(&L.attn_norm, H)) != RCA_OK || (rc = ones(&L.ffn_norm, H)) != RCA_OK)
            return bail(rc);
    }
    RCA_HIP(hipStreamSynchronize(h->stream));
    if ((rc = lm_common_init(h, nullptr, 0)) != RCA_OK) return bail(rc);
    *out = h;
    return RCA_OK;
}

// A second instance over the SAME weights (the reference keeps two llama.cpp models of one file: `llm` and the logits_all twin
// `aux_llm`, realtime_agent_resources.py:19-33): own KV cache, workspace, sampler, stream and graphs; weights and RoPE tables
// are the parent's.  Either handle may be destroyed first.  Calls that modify weights (rca_lm_mask_head_rows,
// rca_lm_persist_codec_embeddings) act on both.
extern "C" int rca_lm_create_shared(rca_lm_t* parent, int32_t n_ctx, int32_t logits_all, rca_lm_t** out) {
    if (!parent || !out) return fail(RCA_ERR_ARG, "null argument");
    rca_lm* owner = parent->weights_of ? parent->weights_of : parent;
    if (owner->zombie) return fail(RCA_ERR_STATE, "create_shared: the parent handle was destroyed");
    rca_lm_config_t cfg = parent->cfg;
    cfg.n_ctx = n_ctx;
    cfg.logits_all = logits_all;
    if (n_ctx < 2 || (n_ctx + ATT_KEYS - 1) / ATT_KEYS * ATT_KEYS > owner->n_ctx_pad)
        return fail(RCA_ERR_ARG, "create_shared: n_ctx %d exceeds the parent's RoPE tables (%d positions)", n_ctx, owner->n_ctx_pad);
    rca_lm* h = nullptr;
    int rc;
    if ((rc = lm_new(&cfg, parent->device, &h)) != RCA_OK) return rc;
    h->embed = owner->embed;
    h->embed_f32 = owner->embed_f32;
    h->head = owner->head;
    h->final_norm = owner->final_norm;
    h->layers = owner->layers;
    h->weights_of = owner;
    // the twin evaluates with the kernels its parent would use (the shadow cache must hold the bits recompute_kv_cache would leave)
    h->fuse_attn = parent->fuse_attn;
    h->mfma_prefill = parent->mfma_prefill;
    h->act_format = parent->act_format;
    h->kv_format = parent->kv_format;   // (lm_common_init below allocates the cache in it)
    h->kv_shift_requant = parent->kv_shift_requant;
    owner->borrowers++;
    if ((rc = lm_common_init(h, nullptr, 0, owner)) != RCA_OK) { rca_lm_destroy(h); return rc; }
    *out = h;
    return RCA_OK;
}

// ------------------------------------------------------------------------- forward pass (M tokens)
// The one place that turns a matrix's runtime format into a template argument: f(std::integral_constant<int, WF_...>{}).  A new
// format is added here (and to WF_FORMATS) and every launcher below sees it.
static constexpr int WF_FORMATS[] = {WF_BF16, WF_Q8, WF_F16, WF_Q4K, WF_Q6K, WF_Q5K, WF_Q40, WF_IQ4};
template <class F>
static void wf_dispatch(int fmt, F&& f) {
    switch (fmt) {
        case WF_Q6K: return f(std::integral_constant<int, WF_Q6K>{});
        case WF_Q4K: return f(std::integral_constant<int, WF_Q4K>{});
        case WF_Q5K: return f(std::integral_constant<int, WF_Q5K>{});
        case WF_Q40: case WF_Q41: return f(std::integral_constant<int, WF_Q40>{});   // one form on the device: the two differ only at load
        case WF_IQ4: case WF_IQ4XS: return f(std::integral_constant<int, WF_IQ4>{});   // likewise
        case WF_Q8: return f(std::integral_constant<int, WF_Q8>{});
        case WF_F16: return f(std::integral_constant<int, WF_F16>{});
        default: return f(std::integral_constant<int, WF_BF16>{});
    }
}
// Launch geometry of the decode GEMVs: R rows per batch (weights of a whole batch are in flight per wave before any is
// consumed) and batches per workgroup.  Defaults are sized for the 256 CUs (>= 2 workgroups each, all resident at once);
// RCA_GEMV_<QKV|O|GU|DOWN|HEAD>="R,batches" overrides one for tuning runs (scripts/lm_gemv_sweep.sh).  Results do not
// depend on the choice.
struct GemvGeom { int R, bpw; };
enum { GEMV_QKV = 0, GEMV_O, GEMV_GU, GEMV_DOWN, GEMV_HEAD, GEMV_KINDS };
static GemvGeom gemv_geom(int kind, int N, bool q8) {
    static GemvGeom tab[2][GEMV_KINDS];
    static bool init = false;
    if (!init) {
        // measured (scripts/lm_gemv_sweep.sh, profiles/r02): the same geometry serves both formats; a q8_0 batch of R rows is R / 2 loads
        const GemvGeom def[2][GEMV_KINDS] = {{{4, 1}, {4, 1}, {16, 2}, {4, 1}, {16, 8}}, {{4, 1}, {4, 1}, {16, 2}, {4, 1}, {16, 8}}};
        const char* names[2][GEMV_KINDS] = {{"RCA_GEMV_QKV", "RCA_GEMV_O", "RCA_GEMV_GU", "RCA_GEMV_DOWN", "RCA_GEMV_HEAD"},
                                           {"RCA_GEMVQ_QKV", "RCA_GEMVQ_O", "RCA_GEMVQ_GU", "RCA_GEMVQ_DOWN", "RCA_GEMVQ_HEAD"}};
        for (int f = 0; f < 2; ++f)
            for (int k = 0; k < GEMV_KINDS; ++k) {
                tab[f][k] = def[f][k];
                const char* e = getenv(names[f][k]);
                int r = 0, bw = 0;
                if (e && sscanf(e, "%d,%d", &r, &bw) == 2 && (r == 4 || r == 8 || r == 16) && bw >= 1) tab[f][k] = {r, bw};
            }
        init = true;
    }
    GemvGeom g = tab[q8 ? 1 : 0][kind];
    // small models: never fewer than ~64 workgroups while there are rows to hand out
    while (g.bpw > 1 && (N + g.R * g.bpw - 1) / (g.R * g.bpw) < 64) g.bpw >>= 1;
    return g;
}
// M = 4 (the group step's rows) costs registers per weight row in flight: 4 R sums and 32 NIT x values per lane.  gemv_group_r lowers R
// until R * NIT <= 16 (the 4-bit forms and Q6_K keep their minimum of 8), and the packed instances with four chunks per lane (the down
// projection of a wide FFN: 128 x values) ask the allocator for one wave per SIMD instead of two (gemv_min_waves).  With that every
// format has its M = 4 instances and none of them uses scratch: profiles/r13/gemv_m4_registers.txt.
constexpr bool gemv_built(int M, int NIT, int R, int Q) {
    // Q5_K / Q4_0 / IQ4 at NIT = 4: launch_gemv_q never leaves R = 16 (four quads x four chunks = 16 loads, twice its limit), and the
    // instance would not fit the register file (it spills): not built
    if ((Q == WF_Q5K || Q == WF_Q40 || Q == WF_IQ4) && NIT == 4 && R == 16) return false;
    if (M == 4) {   // what gemv_group_r never asks for is not built
        const bool min8 = Q == WF_Q4K || Q == WF_Q5K || Q == WF_Q40 || Q == WF_IQ4 || Q == WF_Q6K;
        if (min8 ? (R == 4 || (R == 16 && NIT > 1)) : R * NIT > 16) return false;
    }
    return true;
}
template <int M, int NIT, int PRO, int EPI, int Q, int ACT, int GRP = 0>
static void launch_gemv_r(const GemvGeom& g, rca_lm* h, const WMat& w, const float* x, float* y, int N, int K, int ldy, const GemvPro& pro,
                          const GemvRope& rope, hipStream_t st, const GemvGroup& grp = GemvGroup{nullptr, 0}) {
    const int grid = cdiv(cdiv(N, g.R), g.bpw);
    const GemvQ8 qa{w.qs, w.sc, w.dd};
    if (h) { const int rec[8] = {M, NIT, g.R, g.bpw, grid, w.fmt, ACT, N}; memcpy(h->gemv_last, rec, sizeof rec); }   // host side only: what rca_lm_gemv_tap_form reports
    auto go = [&](auto rr) {
        constexpr int R = decltype(rr)::value;
        if constexpr (gemv_built(M, NIT, R, Q)) {
            if constexpr (GRP != 0) lm_gemv_group_kernel<M, NIT, R, PRO, EPI, Q, ACT><<<grid, 256, 0, st>>>(nullptr, w.wptr(), qa, x, N, K, y, g.bpw, ldy, pro, rope, grp);
            else lm_gemv_kernel<M, NIT, R, PRO, EPI, Q, ACT><<<grid, 256, 0, st>>>(h->stt, w.wptr(), qa, x, N, K, y, g.bpw, ldy, pro, rope);
        }
    };
    switch (g.R) {
        case 4: go(std::integral_constant<int, 4>{}); break;
        case 8: go(std::integral_constant<int, 8>{}); break;
        default: go(std::integral_constant<int, 16>{}); break;
    }
}
// rows per batch of an M = 4 launch: the geometry of the M <= 2 launch, halved until R * NIT <= 16 (the packed 4-bit forms keep two
// quads).  Results do not depend on R.
static int gemv_group_r(int R, int nit_t, bool four_bit) {
    while (R > (four_bit ? 8 : 4) && R * nit_t > 16) R >>= 1;
    return R;
}
// M = 1, 2 or (group steps) 4 rows; GRP: the rows' sessions come from `grp` (QKV and head only, M = 2 or 4)
template <int PRO, int EPI, int Q, int ACT = 0, int GRP = 0>
static void launch_gemv_q(GemvGeom g, rca_lm* h, int M, const WMat& w, const float* x, float* y, int N, int K, int ldy, const GemvPro& pro,
                          const GemvRope& rope, hipStream_t st, const GemvGroup& grp = GemvGroup{nullptr, 0}) {
    const int nit = cdiv(cdiv(K >> 3, 4), 64);
    // 16-byte weight loads in flight per lane: at most 16 (registers); q8_0 needs one load per row PAIR
    constexpr bool four_bit = Q == WF_Q4K || Q == WF_Q5K || Q == WF_Q40 || Q == WF_IQ4;
    const int lpr = (Q == WF_Q8 || Q == WF_Q6K) ? 2 : (four_bit ? 4 : 1);
    const int max_loads = four_bit ? 8 : 16;   // Q4_K / Q5_K / Q4_0 / IQ4 also hold the factors of every quad in registers
    while (g.R > 4 && (g.R / lpr) * (nit == 3 ? 4 : nit) > max_loads) g.R >>= 1;
    if ((four_bit || Q == WF_Q6K) && g.R < 8) g.R = 8;   // a Q4_K batch is at least two quads (one per register half); Q6_K scale loads cover two pairs
    if (M == 4) g.R = gemv_group_r(g.R, nit == 3 ? 4 : nit, four_bit || Q == WF_Q6K);
    if (PRO == 0 && EPI == 3 && nit > 1) {
        if constexpr (GRP == 0) {
            if (nit == 2) {
                if (M == 1) launch_gemv_r<1, 2, 0, 3, Q, ACT>(g, h, w, x, y, N, K, ldy, pro, rope, st);
                else if (M == 2) launch_gemv_r<2, 2, 0, 3, Q, ACT>(g, h, w, x, y, N, K, ldy, pro, rope, st);
                else launch_gemv_r<4, 2, 0, 3, Q, ACT>(g, h, w, x, y, N, K, ldy, pro, rope, st);
            } else {
                if (M == 1) launch_gemv_r<1, 4, 0, 3, Q, ACT>(g, h, w, x, y, N, K, ldy, pro, rope, st);
                else if (M == 2) launch_gemv_r<2, 4, 0, 3, Q, ACT>(g, h, w, x, y, N, K, ldy, pro, rope, st);
                else launch_gemv_r<4, 4, 0, 3, Q, ACT>(g, h, w, x, y, N, K, ldy, pro, rope, st);
            }
        }
        return;
    }
    if constexpr (GRP != 0) {
        if (M == 2) launch_gemv_r<2, 1, PRO, EPI, Q, ACT, 1>(g, h, w, x, y, N, K, ldy, pro, rope, st, grp);
        else launch_gemv_r<4, 1, PRO, EPI, Q, ACT, 1>(g, h, w, x, y, N, K, ldy, pro, rope, st, grp);
    } else {
        if (M == 1) launch_gemv_r<1, 1, PRO, EPI, Q, ACT>(g, h, w, x, y, N, K, ldy, pro, rope, st);
        else if (M == 2) launch_gemv_r<2, 1, PRO, EPI, Q, ACT>(g, h, w, x, y, N, K, ldy, pro, rope, st);
        else if constexpr (!(PRO == 1 && (EPI == 0 || EPI == 2)))   // four rows of ONE session do not exist: QKV and head at M = 4 are grouped launches
            launch_gemv_r<4, 1, PRO, EPI, Q, ACT>(g, h, w, x, y, N, K, ldy, pro, rope, st);
    }
}
// M = 1 or 2 tokens of one session, or the 2 / 4 rows of a group step.  Only the down projection (K = ffn) needs more than one chunk per
// lane and wave.  The matrix is streamed in the format it is kept in.
template <int PRO, int EPI, int GRP = 0>
static void launch_gemv(int kind, rca_lm* h, int M, const WMat& w, const float* x, float* y, int N, int K, int ldy, const GemvPro& pro,
                        const GemvRope& rope, hipStream_t st, const GemvGroup& grp = GemvGroup{nullptr, 0}) {
    const GemvGeom g = gemv_geom(kind, N, wf_packed(w.fmt));
    wf_dispatch(w.fmt, [&](auto wf) {
        constexpr int Q = decltype(wf)::value;
        if constexpr (wf_packed(Q))   // q8_1 activations on the integer dot (rca_lm_set_act_format); 16-bit matrices keep f32 activations
            if (h->act_format == 1) return launch_gemv_q<PRO, EPI, Q, 1, GRP>(g, h, M, w, x, y, N, K, ldy, pro, rope, st, grp);
        launch_gemv_q<PRO, EPI, Q, 0, GRP>(g, h, M, w, x, y, N, K, ldy, pro, rope, st, grp);
    });
}

// Merge of the splits of one (token, head) row by ONE wave, lane <-> dim, in split order.  Latency code: every load it will ever
// need is issued in the first instructions -- the (m, l) pair of split `lane` and this lane's output element of up to CMB_PRE
// splits -- and none of them depends on the step state (the bound is the number of splits the attention kernel was LAUNCHED
// with; a split beyond the visible context carries m = -inf and weighs 0, its o is never used).  COHERENT: the partials were
// written by other workgroups of the SAME launch (fused path): every load is an agent-scope (sc1) load.
#define CMB_PRE 32
template <bool COHERENT>
__device__ __forceinline__ float attn_part_load(const float* p) {
    if (COHERENT) return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return *p;
}
template <bool COHERENT>
__device__ __forceinline__ float attn_merge_row(const float* __restrict__ base, int nsp, int d) {
    const long sstride = 32L * 66;
    float pv[CMB_PRE];
#pragma unroll
    for (int j = 0; j < CMB_PRE; ++j) pv[j] = attn_part_load<COHERENT>(base + (long)min(j, nsp - 1) * sstride + 2 + d);
    float mx, ml0, ll0;
    {
        const int sp = min(d, nsp - 1);
        ml0 = attn_part_load<COHERENT>(base + sp * sstride);
        ll0 = attn_part_load<COHERENT>(base + sp * sstride + 1);
        if (d >= nsp) { ml0 = -INFINITY; ll0 = 0.0f; }
        mx = ml0;
    }
    for (int s0 = 64; s0 < nsp; s0 += 64) {   // more than 64 splits (contexts beyond 16 k): the rare, slower tail
        const int sp = s0 + d;
        mx = fmaxf(mx, sp < nsp ? attn_part_load<COHERENT>(base + sp * sstride) : -INFINITY);
    }
    mx = wave_max(mx);
    float L = 0.0f, O = 0.0f;
    {
        const float fl = (ml0 == -INFINITY) ? 0.0f : __expf(ml0 - mx);
        const int cnt = min(64, nsp);
#pragma unroll
        for (int j = 0; j < CMB_PRE; ++j) {
            if (j < cnt) {
                const float f = __shfl(fl, j), l = __shfl(ll0, j);
                L = __builtin_fmaf(l, f, L);
                O = __builtin_fmaf(f == 0.0f ? 0.0f : pv[j], f, O);
            }
        }
        for (int j = CMB_PRE; j < cnt; ++j) {
            const float f = __shfl(fl, j), l = __shfl(ll0, j);
            const float p = attn_part_load<COHERENT>(base + (long)j * sstride + 2 + d);
            L = __builtin_fmaf(l, f, L);
            O = __builtin_fmaf(f == 0.0f ? 0.0f : p, f, O);
        }
    }
    for (int s0 = 64; s0 < nsp; s0 += 64) {
        const int spl = min(s0 + d, nsp - 1);
        const float ml = attn_part_load<COHERENT>(base + spl * sstride), ll = attn_part_load<COHERENT>(base + spl * sstride + 1);
        const float fl = (ml == -INFINITY) ? 0.0f : __expf(ml - mx);
        const int cnt = min(64, nsp - s0);
        for (int j = 0; j < cnt; ++j) {
            const float f = __shfl(fl, j), l = __shfl(ll, j);
            const float p = attn_part_load<COHERENT>(base + (long)(s0 + j) * sstride + 2 + d);
            L = __builtin_fmaf(l, f, L);
            O = __builtin_fmaf(f == 0.0f ? 0.0f : p, f, O);
        }
    }
    return O / L;
}
// ------------------------------------------------------------------ attention on MFMA (decode steps and prefill tiles)
// grid (kv head, 256-key split, block of 32 query rows); a query row is (token, q head of this kv head), 32 / G tokens
// per block; 8 waves, each ONE block of 32 keys (so there is no online rescaling inside a wave):
//   S^T = K (32 keys x 64 dims, fp16 straight from the cache) x Q^T  on v_mfma_f32_32x32x16_f16, Q split into fp16
//         hi + lo (two MFMAs per 16 dims).  The result has lane <-> query row, registers <-> keys, so the softmax
//         statistics are 16 in-lane values plus one cross-half exchange.
//   O   = P x V: P goes in as the A operand exactly as it sits in registers (hi + lo fp16); the order of the
//         contraction index is free as long as both operands agree, so V is read from an LDS-transposed copy
//         vt[dim][key] in the key order P's registers have.
// Then the 8 waves are merged and the split partial is written like the pairwise kernel does:
// part[((qblock * nkv + g) * n_splits + split) * 32 + row][66] = {m, l, o[64]}, row = token_in_block * G + q_head.
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));
typedef short flash_s16x4 __attribute__((__vector_size__(4 * sizeof(short))));
// Diagnostic build only (-DRCA_ATTN_TIMELINE, scripts/attn_timeline.py): thread 0 of every decode-attention workgroup stamps its phases
// with the 100 MHz wall clock into a buffer no other code reads.
#ifdef RCA_ATTN_TIMELINE
__device__ long* rca_attn_tl = nullptr;
#define ATL_STAMP(k) do { if (atl && threadIdx.x == 0) atl[k] = (long)wall_clock64(); } while (0)
#define ATL_STAMP_W7(k) do { if (atl && threadIdx.x == 448) atl[k] = (long)wall_clock64(); } while (0)   // the same phases seen by the last wave
#else
#define ATL_STAMP(k)
#define ATL_STAMP_W7(k)
#endif

#define ATTM_LDS (8 * 32 * 64 * 4 + 2 * 8 * 32 * 4)   // wo (aliases the K / V images) + wm + wl
// TAB = true (rca_lm_batch_step): the decode attention of EVERY member of a batch in one launch, grid (kv head, 256-key split, member).
// A member's n <= 2 query tokens are one query block; its state, cache, partials and its rows of the shared qkv buffer come from
// tab[member] (the pointer arguments are unused).  The grid covers the largest split count among the members: a split past a
// member's cache leaves at once (its att_part has no slot for it), one past its context takes the empty-split path below.  Partials
// always go through att_part and a separate merge launch: the in-launch merge and its polling loop are compiled out of this instance.
// The TAB = false instances are the kernel as it was before the table existed.
struct LmBatchMember {
    LmDevState* stt;          // the member's step state: n_tokens = its KV position, m = its tokens of the pass
    const f16_t* kc; const f16_t* vc;   // its cache (layer 0)
    long kv_stride;           // layer stride in elements
    float* part;              // its att_part
    float* logits;            // its logits buffer (the head's row copy)
    SamplerDev* samp;         // its sampler + work area (the table chain)
    SampWork* swork;
    int row0;                 // its first row in the batch's qkv / hi / lo buffers
    int n_splits, n_ctx;
    int serial;               // 1: its sampler is the serial top-k chain, run by the table kernels
    // q8_0 cache (every member of a batch has the same format): kc / vc are the int8 planes, kv_stride their layer stride in bytes; the
    // fp16 scales [L][n_ctx_pad][nkv][2] start sc_off bytes behind kc / vc; ring_k / ring_v: the member's staging ring (LmGroupRow::kc)
    long sc_off;
    const f16_t* ring_k; const f16_t* ring_v;
    int ring_mask, pad;
};
// ------------------------------------------------------------------ q8_0 KV cache (rca_lm_set_kv_format)
// A cached head row (64 values of K or of V) is two ggml q8_0 blocks: 32 int8 + one fp16 scale each, kept in two planes per tensor,
// q[L][n_ctx_pad][nkv][64] int8 and d[L][n_ctx_pad][nkv][2] fp16, so a head row is 64 contiguous, 64-byte-aligned bytes.
// Contract: cache row == Q8(the fp16 row the default cache would hold).  The QKV epilogues are untouched but for where they store:
// under q8_0 their fp16 rows go to a per-handle ring of LM_KV_RING positions (row pos & (LM_KV_RING - 1); one ring for all layers,
// a layer's rows are quantised before the next layer's projection runs), and lm_kv_quant_kernel, one small launch per layer between
// the projection and attention, turns the rows of the pass into blocks with the rule of the q8_1 activations:
//   d = amax / 127;  inv = d != 0 ? 1 / d : 0;  q_j = roundf(x_j * inv);  stored scale d16 = fp16_rne(d)
// Attention multiplies fp16_rne((float)d16 * q_j), formed while a row is staged into the LDS images (kvq8_deq16): behind the images
// nothing differs from the fp16 cache.
static_assert((LM_KV_RING & (LM_KV_RING - 1)) == 0, "ring positions are masked");
// 16 int8 of one block and the block's scale -> the 16 fp16 values as two 16-byte chunks ((float)d16 * q is exact in f32: 11 x 7 bits)
__device__ __forceinline__ void kvq8_deq16(const u32x4 q, const f16_t d16, u32x4& c0, u32x4& c1) {
    const float d = (float)d16;
    f16x8 a, b;
#pragma unroll
    for (int w = 0; w < 4; ++w)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float v = (float)(int)(signed char)(q[w] >> (8 * e)) * d;
            if (w < 2) a[4 * w + e] = (_Float16)v;
            else b[4 * (w - 2) + e] = (_Float16)v;
        }
    c0 = __builtin_bit_cast(u32x4, a);
    c1 = __builtin_bit_cast(u32x4, b);
}
// grid (blocks of 8 units, token of the pass, member): a unit is one q8_0 block = 32 lanes, lane <-> value; units of a position are
// ordered (tensor, kv head, block).  stt != nullptr: position and token count of the pass come from the device state (graph-safe);
// else from pos0_arg / m_arg (rca_lm_kv_write).  which: bit 0 K, bit 1 V.  TAB: everything per member from tab[blockIdx.z].
template <bool TAB>
__global__ __launch_bounds__(256) void lm_kv_quant_kernel(const LmDevState* __restrict__ stt, const f16_t* __restrict__ ring_k, const f16_t* __restrict__ ring_v,
                                                          int ring_mask, signed char* __restrict__ kq, signed char* __restrict__ vq,
                                                          f16_t* __restrict__ kd, f16_t* __restrict__ vd, int nkv, int n_ctx, int pos0_arg, int m_arg,
                                                          int which, const LmBatchMember* __restrict__ tab, int tab_layer) {
    if constexpr (TAB) {
        const LmBatchMember e = tab[blockIdx.z];
        if (!e.stt) return;   // a slot past the live count of a selection frame
        stt = e.stt;
        ring_k = e.ring_k; ring_v = e.ring_v; ring_mask = e.ring_mask;
        kq = reinterpret_cast<signed char*>(const_cast<f16_t*>(e.kc)) + (long)tab_layer * e.kv_stride;
        vq = reinterpret_cast<signed char*>(const_cast<f16_t*>(e.vc)) + (long)tab_layer * e.kv_stride;
        kd = reinterpret_cast<f16_t*>(reinterpret_cast<char*>(const_cast<f16_t*>(e.kc)) + e.sc_off) + (long)tab_layer * (e.kv_stride >> 5);
        vd = reinterpret_cast<f16_t*>(reinterpret_cast<char*>(const_cast<f16_t*>(e.vc)) + e.sc_off) + (long)tab_layer * (e.kv_stride >> 5);
        n_ctx = e.n_ctx;
    }
    const int M = stt ? stt->m : m_arg;
    const int tok = blockIdx.y;
    if (tok >= M) return;
    const int pos = (stt ? stt->n_tokens : pos0_arg) + tok;
    if (pos >= n_ctx) return;
    const int unit = blockIdx.x * 8 + (threadIdx.x >> 5);
    if (unit >= 4 * nkv) return;
    const int tensor = unit / (2 * nkv), hb = unit - tensor * 2 * nkv;   // hb = kv head * 2 + block
    if (!((which >> tensor) & 1)) return;
    const int j = threadIdx.x & 31;
    const float x = (float)(tensor ? ring_v : ring_k)[((long)(pos & ring_mask) * nkv) * 64 + hb * 32 + j];
    float amax = fabsf(x);
#pragma unroll
    for (int o = 16; o >= 1; o >>= 1) amax = fmaxf(amax, __shfl_xor(amax, o, 32));
    const float d = amax / 127.0f;
    const float inv = d != 0.0f ? 1.0f / d : 0.0f;
    (tensor ? vq : kq)[((long)pos * nkv) * 64 + hb * 32 + j] = (signed char)(int)roundf(x * inv);
    if (j == 0) (tensor ? vd : kd)[((long)pos * nkv) * 2 + hb] = (f16_t)d;
}
// rca_lm_batch_eval: grid (blocks of 8 units, row of the pass).  A row finds its segment through the pass's owner map (one entry per
// 32 rows) and takes ring, planes, scales, position and context bound from the segment's entry; pad rows leave.  One geometry for
// every packing of a pass of the same token blocks, so a captured pass holds no segment count.
__global__ __launch_bounds__(256) void lm_kv_quant_rows_kernel(const LmDevState* __restrict__ pstt, const LmBatchMember* __restrict__ tab,
                                                               const int* __restrict__ owner, int tab_layer, int nkv) {
    const int row = blockIdx.y;
    if (row >= pstt->m) return;
    const int seg = owner[row >> 5];
    if (seg < 0) return;
    const LmBatchMember e = tab[seg];
    const int tok = row - e.row0;
    if (tok >= e.stt->m) return;
    const int pos = e.stt->n_tokens + tok;
    if (pos >= e.n_ctx) return;
    // from here on: lm_kv_quant_kernel's arithmetic on the segment's ring, planes and scales
    const f16_t* ring_k = e.ring_k; const f16_t* ring_v = e.ring_v;
    const int ring_mask = e.ring_mask, which = 3;
    signed char* kq = reinterpret_cast<signed char*>(const_cast<f16_t*>(e.kc)) + (long)tab_layer * e.kv_stride;
    signed char* vq = reinterpret_cast<signed char*>(const_cast<f16_t*>(e.vc)) + (long)tab_layer * e.kv_stride;
    f16_t* kd = reinterpret_cast<f16_t*>(reinterpret_cast<char*>(const_cast<f16_t*>(e.kc)) + e.sc_off) + (long)tab_layer * (e.kv_stride >> 5);
    f16_t* vd = reinterpret_cast<f16_t*>(reinterpret_cast<char*>(const_cast<f16_t*>(e.vc)) + e.sc_off) + (long)tab_layer * (e.kv_stride >> 5);
    const int unit = blockIdx.x * 8 + (threadIdx.x >> 5);
    if (unit >= 4 * nkv) return;
    const int tensor = unit / (2 * nkv), hb = unit - tensor * 2 * nkv;   // hb = kv head * 2 + block
    if (!((which >> tensor) & 1)) return;
    const int j = threadIdx.x & 31;
    const float x = (float)(tensor ? ring_v : ring_k)[((long)(pos & ring_mask) * nkv) * 64 + hb * 32 + j];
    float amax = fabsf(x);
#pragma unroll
    for (int o = 16; o >= 1; o >>= 1) amax = fmaxf(amax, __shfl_xor(amax, o, 32));
    const float d = amax / 127.0f;
    const float inv = d != 0.0f ? 1.0f / d : 0.0f;
    (tensor ? vq : kq)[((long)pos * nkv) * 64 + hb * 32 + j] = (signed char)(int)roundf(x * inv);
    if (j == 0) (tensor ? vd : kd)[((long)pos * nkv) * 2 + hb] = (f16_t)d;
}
// rca_lm_kv_read / rca_lm_gemv_tap on a q8_0 cache: n16 pieces of 16 values, de-quantised by the code attention stages rows with
__global__ __launch_bounds__(256) void lm_kv_dequant_kernel(const signed char* __restrict__ q, const f16_t* __restrict__ d, f16_t* __restrict__ out, long n16) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n16) return;
    u32x4 c0, c1;
    kvq8_deq16(*reinterpret_cast<const u32x4*>(q + 16 * i), d[i >> 1], c0, c1);
    *reinterpret_cast<u32x4*>(out + 16 * i) = c0;
    *reinterpret_cast<u32x4*>(out + 16 * i + 8) = c1;
}
// KVQ = 1: the cache is q8_0 -- kc / vc are the int8 planes of the layer, kd / vd its scales; only the global loads and the image writes
// differ (a lane takes 16 int8 of a row and their block's scale: 16 rows per instruction, two chunks per lane and load)
template <int G, bool TAB = false, int KVQ = 0>
// (argument order: what the first loads need -- the cache pointers, the head counts, n_ctx -- sits inside the 14 dwords the
//  dispatcher preloads into SGPRs; `part` / `arrive` / `attn_out` are only needed at the end)
__global__ __launch_bounds__(512) void lm_attn_mfma_kernel(const LmDevState* __restrict__ stt, const float* __restrict__ qkv,
                                                           const f16_t* __restrict__ kc, const f16_t* __restrict__ vc,
                                                           int nh, int nkv, int n_splits, float scale, int n_ctx,
                                                           float* __restrict__ part, int* __restrict__ arrive, float* __restrict__ attn_out,
                                                           const LmBatchMember* __restrict__ tab = nullptr, int tab_layer = 0) {
    // q8_0 scales of the layer.  The argument list is the fp16 kernel's (its instances are what they were): without a table, tab_layer
    // carries the distance from the layer's int8 plane to its scales in units of 16 bytes -- the same for K and V, whose allocations
    // have one layout
    const f16_t *kd = nullptr, *vd = nullptr;
    if constexpr (KVQ && !TAB) {
        kd = reinterpret_cast<const f16_t*>(reinterpret_cast<const char*>(kc) + (long)tab_layer * 16);
        vd = reinterpret_cast<const f16_t*>(reinterpret_cast<const char*>(vc) + (long)tab_layer * 16);
    }
    if constexpr (TAB) {
        const LmBatchMember e = tab[blockIdx.z];
        if ((int)blockIdx.y >= e.n_splits) return;   // (also a slot past a selection's live count: an all-zero entry has no splits)
        stt = e.stt;
        qkv += (long)e.row0 * (nh + 2 * nkv) * 64;
        if constexpr (KVQ) {
            kd = reinterpret_cast<const f16_t*>(reinterpret_cast<const char*>(e.kc) + e.sc_off) + (long)tab_layer * (e.kv_stride >> 5);
            vd = reinterpret_cast<const f16_t*>(reinterpret_cast<const char*>(e.vc) + e.sc_off) + (long)tab_layer * (e.kv_stride >> 5);
            kc = reinterpret_cast<const f16_t*>(reinterpret_cast<const char*>(e.kc) + (long)tab_layer * e.kv_stride);
            vc = reinterpret_cast<const f16_t*>(reinterpret_cast<const char*>(e.vc) + (long)tab_layer * e.kv_stride);
        } else {
            kc = e.kc + (long)tab_layer * e.kv_stride;
            vc = e.vc + (long)tab_layer * e.kv_stride;
        }
        n_splits = e.n_splits;
        n_ctx = e.n_ctx;
        part = e.part;
    }
    // arrive != nullptr (decode steps: one query block, at most one workgroup per CU, at most 8 live query rows): the merge of the
    // splits happens HERE, by data-tagged granules (MI355X_MICROARCH.md, price list rows handoff-1to1 / allgather: "granule = one
    // naturally aligned 8-byte {data, tag} written by ONE sc1 store", polled with sc1 loads; R2: a granule needs no ordering).  Every
    // workgroup publishes its partial (m, l, o[64]) of the 8 live rows as 528 granules {f32 bits, tag} -- no drain, no barrier, no
    // ticket -- and leaves; the workgroups of the first splits then gather, one wave per (token, head) row and lane <-> dim, the
    // granules of every launched split, re-polling until each carries this launch's tag, and merge them in split order with the
    // arithmetic of the separate combine kernel (same bits).  The tag is the kv head's launch counter arrive[g]: read at entry by every workgroup of the
    // head, advanced by split 0's workgroup at its very end -- after it has seen every producer's granules, so no workgroup of this
    // launch can read the new value; the next launch (another layer, the same buffer) starts behind the kernel boundary.  Producers
    // never wait, so the merger's wait ends whatever the placement; its spin is bounded all the same (a NaN row would tell).
    // Round 3 did this with drained sc1 stores + an arrival ticket + a re-read by the last arriver: 4.2 us from the last partial's
    // stores to the merged row at 6.6 k context (profiles/r04/attn_decode_timeline.txt); the granules take the drain, the two
    // barriers and the ticket round trip out of the chain.
    const bool fused = !TAB && arrive != nullptr;
#ifdef RCA_ATTN_TIMELINE
    long* const atl = (rca_attn_tl && fused) ? rca_attn_tl + ((long)(blockIdx.y * gridDim.x + blockIdx.x) & 1023) * 16 : nullptr;
#endif
    ATL_STAMP(0);
    ATL_STAMP_W7(11);
    unsigned long long* const gran = reinterpret_cast<unsigned long long*>(arrive + ATT_EPOCH_INTS) +
                                     ((long)blockIdx.x * n_splits + blockIdx.y) * (8 * 66);     // this workgroup's 8 x 66 granules
    unsigned tag = 0;
    auto part_store = [&](float* p, float v) { *p = v; };
    auto gran_store = [&](int row, int e, float v) {
        __hip_atomic_store(gran + row * 66 + e, ((unsigned long long)tag << 32) | (unsigned long long)__float_as_uint(v), __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_AGENT);
    };
    auto tag_merge = [&](int M_) {
        // The rows of a kv head are merged by DIFFERENT workgroups -- row r by the workgroup of split r % nmerge, nmerge = min(8,
        // launched splits) -- one wave per row, lane <-> dim: a row's sweep is splits x 528 bytes, and eight rows gathered by ONE
        // workgroup (139 KB of 8-byte sc1 loads through one CU at 6.6 k context) took 2 us per sweep.
        const int d = threadIdx.x & 63;
        const int nsp = (int)gridDim.y;
        const int nmerge = min(nsp, 8);
        const int w = (int)blockIdx.y + nmerge * (int)(threadIdx.x >> 6);       // row (token_in_block * G + q head) of this wave
        if (w < M_ * G) {
            const unsigned long long* base = reinterpret_cast<const unsigned long long*>(arrive + ATT_EPOCH_INTS) + ((long)blockIdx.x * n_splits) * (8 * 66) + w * 66;
            auto gload = [&](const unsigned long long* q) { return __hip_atomic_load(q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); };
            int spins = 0;
            // ONE sweep asks for everything the row needs -- (m, l) of split d + 64 c in lane d and this lane's output element of the
            // first CMB_PRE splits -- and is repeated as a whole until every granule carries the tag: in the common case the merge
            // costs one memory round trip behind the last producer's stores (two sweeps in sequence, (m, l) first, cost two).
            unsigned long long gm[ATT_TAG_MAXSP / 64], gl[ATT_TAG_MAXSP / 64], pg[CMB_PRE];
            for (;;) {
                bool ok = true;
#pragma unroll
                for (int c = 0; c < ATT_TAG_MAXSP / 64; ++c) {
                    gm[c] = gl[c] = (unsigned long long)tag << 32;
                    if (64 * c < nsp) {
                        const int spj = min(64 * c + d, nsp - 1);
                        gm[c] = gload(base + (long)spj * (8 * 66));
                        gl[c] = gload(base + (long)spj * (8 * 66) + 1);
                    }
                }
#pragma unroll
                for (int j = 0; j < CMB_PRE; ++j) pg[j] = gload(base + (long)min(j, nsp - 1) * (8 * 66) + 2 + d);
#pragma unroll
                for (int c = 0; c < ATT_TAG_MAXSP / 64; ++c) ok = ok && (unsigned)(gm[c] >> 32) == tag && (unsigned)(gl[c] >> 32) == tag;
#pragma unroll
                for (int j = 0; j < CMB_PRE; ++j) ok = ok && (unsigned)(pg[j] >> 32) == tag;
                if (__builtin_amdgcn_ballot_w64(!ok) == 0ull || ++spins > ATT_TAG_SPINS) break;
                __builtin_amdgcn_s_sleep(1);
            }
            float ml[ATT_TAG_MAXSP / 64], ll[ATT_TAG_MAXSP / 64];
            float mx = -INFINITY;
#pragma unroll
            for (int c = 0; c < ATT_TAG_MAXSP / 64; ++c) {
                const bool live = 64 * c + d < nsp;
                ml[c] = live ? __uint_as_float((unsigned)gm[c]) : -INFINITY;
                ll[c] = live ? __uint_as_float((unsigned)gl[c]) : 0.0f;
                mx = fmaxf(mx, ml[c]);
            }
            mx = wave_max(mx);
            float L = 0.0f, O = 0.0f;
#pragma unroll
            for (int c = 0; c < ATT_TAG_MAXSP / 64; ++c) {
                if (64 * c >= nsp) break;
                const float fl = (ml[c] == -INFINITY) ? 0.0f : __expf(ml[c] - mx);
                for (int j0 = 64 * c; j0 < min(nsp, 64 * c + 64); j0 += CMB_PRE) {
                    const int cnt = min(CMB_PRE, nsp - j0);
                    if (j0 > 0) {   // later blocks of CMB_PRE splits (models with fewer kv heads): their granules are long there by now
                        for (;;) {
                            bool ok = true;
#pragma unroll
                            for (int j = 0; j < CMB_PRE; ++j) pg[j] = gload(base + (long)min(j0 + j, nsp - 1) * (8 * 66) + 2 + d);
#pragma unroll
                            for (int j = 0; j < CMB_PRE; ++j) ok = ok && (unsigned)(pg[j] >> 32) == tag;
                            if (__builtin_amdgcn_ballot_w64(!ok) == 0ull || ++spins > ATT_TAG_SPINS) break;
                            __builtin_amdgcn_s_sleep(1);
                        }
                    }
#pragma unroll
                    for (int j = 0; j < CMB_PRE; ++j) {
                        if (j < cnt) {
                            const float f = __shfl(fl, (j0 + j) & 63), l = __shfl(ll[c], (j0 + j) & 63);
                            const float pv = __uint_as_float((unsigned)pg[j]);
                            L = __builtin_fmaf(l, f, L);
                            O = __builtin_fmaf(f == 0.0f ? 0.0f : pv, f, O);
                        }
                    }
                }
            }
            const int m = w / G, head = blockIdx.x * G + w % G;
            attn_out[(long)m * nh * 64 + head * 64 + d] = spins > ATT_TAG_SPINS ? __builtin_nanf("") : O / L;
        }
        // the next launch's tag (never 0: a zeroed buffer matches nothing).  Written by split 0's workgroup once its row is merged:
        // by then every producer has stored -- so has read -- this launch's tag; the other rows' mergers compare with the tag they
        // hold in a register, not with this word.
        if (blockIdx.y == 0 && threadIdx.x == 0) arrive[blockIdx.x] = (int)(tag + 1u == 0u ? 1u : tag + 1u);
        ATL_STAMP(6);
    };
    constexpr int HD = 64;
    constexpr int TPB = 32 / G;   // tokens per query block
    extern __shared__ __attribute__((aligned(16))) float attm_lds[];
    float (*wo)[32][HD] = reinterpret_cast<float (*)[32][HD]>(attm_lds);                        // [8][32][64]
    // (the waves' K / V images, 8 KB each, alias wo: they are dead before wo is written)
    float (*wm)[32] = reinterpret_cast<float (*)[32]>(attm_lds + 8 * 32 * HD);
    float (*wl)[32] = wm + 8;
    const int g = blockIdx.x, sp = blockIdx.y, qb = TAB ? 0 : blockIdx.z;
    const int lane = threadIdx.x & 63;
    const int half = lane >> 5, col = lane & 31;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int kbase = sp * ATT_KEYS;
    const int kwb = kbase + wave * 32;
    const int t0 = qb * TPB;
    const int tl = col / G, hq = col % G;
    const int ld = (nh + 2 * nkv) * HD;
    // every load that does not depend on the step state goes out first (rows past the visible range: clamped, masked).
    // K / V of this wave's 32 keys are loaded in WHOLE ROWS -- lane l of load i takes 16-byte chunk l % 8 of key 8 i + l / 8: 8 cache
    // lines per instruction -- and reach the MFMA operand layouts through two wave-private 4 KB LDS images (the flash kernel's
    // swizzles).  Loading the A layout directly (lane <-> key: 16 bytes of each of 32 rows per instruction) made the CU's address
    // path the bottleneck of the whole launch: round-4 timeline, 1 k context, 32 workgroups: wave 0 had its keys 2.4 us after entry
    // and wave 7 1.55 us later (profiles/r04/attn_decode_timeline.txt).  K first, then q, then V: S^T starts while V is in flight.
    u32x4 kf[KVQ ? 2 : 4], vf[KVQ ? 2 : 4];
    f16_t ksc[2], vsc[2];   // q8_0: the scales of the two loads' blocks
    f32x4 qf[4][2];
    char* const kbytes = reinterpret_cast<char*>(attm_lds) + wave * 8192;   // K image [key][128 bytes], chunk c of key k at c ^ ((k >> 1) & 7)
    char* const vbytes = kbytes + 4096;                                     // V image, chunk c of key k at c ^ (k1 k2 k0)
    const int ld_key = KVQ ? lane >> 2 : lane >> 3, ld_chunk = KVQ ? 2 * (lane & 3) : lane & 7;   // q8_0: the first of the lane's two chunks
    {
        long roff[4];   // (q8_0: two loads, their offsets set below)
#pragma unroll
        for (int i = 0; i < 4; ++i) roff[i] = ((long)min(kwb + 8 * i + ld_key, n_ctx - 1) * nkv + g) * HD + 8 * ld_chunk;
        if constexpr (KVQ) {
#pragma unroll
            for (int i = 0; i < 2; ++i) {   // load i: keys 16 i .. 16 i + 15; byte offset == element offset, a block is 4 chunks
                roff[i] = ((long)min(kwb + 16 * i + ld_key, n_ctx - 1) * nkv + g) * HD + 8 * ld_chunk;
                kf[i] = *reinterpret_cast<const u32x4*>(reinterpret_cast<const char*>(kc) + roff[i]);
                ksc[i] = kd[roff[i] >> 5];
            }
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i) kf[i] = *reinterpret_cast<const u32x4*>(kc + roff[i]);
        }
        // a decode step (fused merge) has at most two tokens: the lanes of the 24 dead query rows load nothing (their scores are
        // masked whatever q they hold) -- the q loads were as many bytes through the CU's address path as K and V together
        const float* qp = qkv + (long)min(t0 + tl, LM_MAXM - 1) * ld + (g * G + hq) * HD + 8 * half;
#pragma unroll
        for (int sub = 0; sub < 4; ++sub) { qf[sub][0] = f32x4{0.0f, 0.0f, 0.0f, 0.0f}; qf[sub][1] = f32x4{0.0f, 0.0f, 0.0f, 0.0f}; }
        if (!fused || tl * G < 8) {   // the fused merge is only used while M * G <= 8
#pragma unroll
            for (int sub = 0; sub < 4; ++sub) {
                qf[sub][0] = *reinterpret_cast<const f32x4*>(qp + 16 * sub);
                qf[sub][1] = *reinterpret_cast<const f32x4*>(qp + 16 * sub + 4);
            }
        }
        if constexpr (KVQ) {
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                vf[i] = *reinterpret_cast<const u32x4*>(reinterpret_cast<const char*>(vc) + roff[i]);
                vsc[i] = vd[roff[i] >> 5];
            }
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i) vf[i] = *reinterpret_cast<const u32x4*>(vc + roff[i]);
        }
    }
    __builtin_amdgcn_sched_barrier(0);
    auto pin_loads = [&]() {
        if constexpr (KVQ) {
#pragma unroll
            for (int c = 0; c < 2; ++c) asm volatile("" ::"v"(kf[c]), "v"(vf[c]), "v"(ksc[c]), "v"(vsc[c]));
#pragma unroll
            for (int c = 0; c < 4; ++c) asm volatile("" ::"v"(qf[c][0]), "v"(qf[c][1]));
        } else {
#pragma unroll
            for (int c = 0; c < 4; ++c) asm volatile("" ::"v"(kf[c]), "v"(vf[c]), "v"(qf[c][0]), "v"(qf[c][1]));
        }
    };
    const int M = stt->m;
    if (t0 >= M) { pin_loads(); return; }
    const int pos0 = stt->n_tokens;
    const int ntok = min(TPB, M - t0);
    const int kmax = pos0 + t0 + ntok;   // keys [0, kmax) are visible to the last token of the block
    ATL_STAMP(12);
    float* pout = part + ((long)(qb * nkv + g) * n_splits + sp) * 32 * 66;
    if (fused) tag = (unsigned)arrive[blockIdx.x];
    if (kbase >= kmax) {   // nothing visible in this split
        if (fused) {   // all 8 x 66 granules, so that the merger has one rule: every granule of every launched split carries the tag
            for (int i = threadIdx.x; i < 8 * 66; i += 512) gran_store(i / 66, i % 66, (i % 66) == 0 ? -INFINITY : 0.0f);
        } else if (threadIdx.x < 32) { part_store(pout + threadIdx.x * 66, -INFINITY); part_store(pout + threadIdx.x * 66 + 1, 0.0f); }
        pin_loads();
        if (fused && sp < 8) tag_merge(M);   // a launched split beyond the context still merges the rows that fall to it
        return;
    }
    // ---- K image of this wave (written and read by this wave only: LDS operations of a wave complete in order)
    if constexpr (KVQ) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int k = 16 * i + ld_key;
            u32x4 c0, c1;
            kvq8_deq16(kf[i], ksc[i], c0, c1);
            *reinterpret_cast<u32x4*>(kbytes + k * 128 + ((ld_chunk ^ ((k >> 1) & 7)) << 4)) = c0;
            *reinterpret_cast<u32x4*>(kbytes + k * 128 + (((ld_chunk + 1) ^ ((k >> 1) & 7)) << 4)) = c1;
        }
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int k = 8 * i + ld_key;
            *reinterpret_cast<u32x4*>(kbytes + k * 128 + ((ld_chunk ^ ((k >> 1) & 7)) << 4)) = kf[i];
        }
    }
    ATL_STAMP(13);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    // ---- S^T = K Q^T (hi + lo): lane (key = col, half) reads chunk half + 2 sub (dims 8 half + 16 sub .. + 8) of its key
    f32x16 sacc;
#pragma unroll
    for (int r = 0; r < 16; ++r) sacc[r] = 0.0f;
#pragma unroll
    for (int sub = 0; sub < 4; ++sub) {
        f16x8 qh, ql;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const float q = j < 4 ? qf[sub][0][j] : qf[sub][1][j - 4];
            const _Float16 h16 = (_Float16)q;
            qh[j] = h16;
            ql[j] = (_Float16)(q - (float)h16);
        }
        const u32x4 kraw = *reinterpret_cast<const u32x4*>(kbytes + col * 128 + (((half | (sub << 1)) ^ ((col >> 1) & 7)) << 4));
        const f16x8 kfr = __builtin_bit_cast(f16x8, kraw);
        sacc = __builtin_amdgcn_mfma_f32_32x32x16_f16(kfr, qh, sacc, 0, 0, 0);
        sacc = __builtin_amdgcn_mfma_f32_32x32x16_f16(kfr, ql, sacc, 0, 0, 0);
    }
    // ---- V image (its loads were issued behind K and q)
    if constexpr (KVQ) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int k = 16 * i + ld_key;
            const int sw = (((k >> 1) & 1) << 2) | (((k >> 2) & 1) << 1) | (k & 1);
            u32x4 c0, c1;
            kvq8_deq16(vf[i], vsc[i], c0, c1);
            *reinterpret_cast<u32x4*>(vbytes + k * 128 + ((ld_chunk ^ sw) << 4)) = c0;
            *reinterpret_cast<u32x4*>(vbytes + k * 128 + (((ld_chunk + 1) ^ sw) << 4)) = c1;
        }
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int k = 8 * i + ld_key;
            *reinterpret_cast<u32x4*>(vbytes + k * 128 + ((ld_chunk ^ ((((k >> 1) & 1) << 2) | (((k >> 2) & 1) << 1) | (k & 1))) << 4)) = vf[i];
        }
    }
    ATL_STAMP(1);   // V of this wave is in registers (its image requested)
    ATL_STAMP_W7(9);
    // ---- softmax statistics of this wave's 32 keys for query row `col`: registers are keys
    const int qpos = pos0 + t0 + tl;
    const bool qvalid = tl < ntok;
    float mx = -INFINITY;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int key = kwb + (r & 3) + 8 * (r >> 2) + 4 * half;
        const float sv = (qvalid && key <= qpos) ? sacc[r] * scale : -INFINITY;
        sacc[r] = sv;
        mx = fmaxf(mx, sv);
    }
    {
        float a = mx, b = mx;
        asm volatile("s_nop 1\n\tv_permlane32_swap_b32 %0, %1\n\ts_nop 1" : "+v"(a), "+v"(b));
        mx = fmaxf(a, b);
    }
    float lsum = 0.0f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const float e = (mx == -INFINITY) ? 0.0f : __expf(sacc[r] - mx);
        sacc[r] = e;
        lsum += e;
    }
    {
        float a = lsum, b = lsum;
        asm volatile("s_nop 1\n\tv_permlane32_swap_b32 %0, %1\n\ts_nop 1" : "+v"(a), "+v"(b));
        lsum = a + b;
    }
    // P as the A operand of O = P V: registers 8i..8i+7 feed MFMA i (hi + lo fp16)
    f16x8 ph[2], pl[2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const float pv = sacc[8 * i + j];
            const _Float16 h16 = (_Float16)pv;
            ph[i][j] = h16;
            pl[i][j] = (_Float16)(pv - (float)h16);
        }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    // ---- O = P V: dims 32 * nt + col; slot j of MFMA i, half h is key 16 i + 4 h + 8 (j >> 2) + (j & 3).  Transposed reads:
    // lane 4 q + p of a 16-lane group supplies row (key) q, dims 4 p .. 4 p + 3 of the group's 16 dims
    f32x16 oacc[2];
    {
        const int l16 = lane & 15, q4 = l16 >> 2, pp = l16 & 3;
        const int sw = ((q4 >> 1) << 2) | (half << 1) | (q4 & 1);   // rows 16 i + 4 half + q4 (+ 8)
#pragma unroll
        for (int nt = 0; nt < 2; ++nt) {
            const int tr_off = (4 * half + q4) * 128 + (((4 * nt + 2 * (col >> 4) + (pp >> 1)) ^ sw) << 4) + 8 * (pp & 1);
#pragma unroll
            for (int r = 0; r < 16; ++r) oacc[nt][r] = 0.0f;
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const char* tp = vbytes + tr_off + 16 * i * 128;
                const flash_s16x4 t0v = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) flash_s16x4*)tp);
                const flash_s16x4 t1v = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) flash_s16x4*)(tp + 8 * 128));
                const f16x4 v0 = __builtin_bit_cast(f16x4, t0v), v1 = __builtin_bit_cast(f16x4, t1v);
                // keys past the visible range may hold anything (their p is 0): zero them
                f16x8 vb;
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const int key = kwb + 16 * i + 4 * half + 8 * (j >> 2) + (j & 3);
                    const _Float16 x = j < 4 ? v0[j] : v1[j - 4];
                    vb[j] = key < kmax ? x : (_Float16)0.0f;
                }
                oacc[nt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ph[i], vb, oacc[nt], 0, 0, 0);
                oacc[nt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(pl[i], vb, oacc[nt], 0, 0, 0);
            }
        }
    }
    ATL_STAMP(2);      // S, softmax, P V of this wave
    ATL_STAMP_W7(10);
    __syncthreads();   // every wave is done with vt: wo may overwrite it
    ATL_STAMP(7);
    if (half == 0) { wm[wave][col] = mx; wl[wave][col] = lsum; }
    // (a decode step has at most 8 live query rows -- registers 0..3 of the accumulators: the other 24 rows are never merged)
#pragma unroll
    for (int nt = 0; nt < 2; ++nt)
#pragma unroll
        for (int r = 0; r < 16; ++r)
            if (r < 4 || !fused) wo[wave][(r & 3) + 8 * (r >> 2) + 4 * half][32 * nt + col] = oacc[nt][r];
    __syncthreads();
    ATL_STAMP(8);
    // ---- merge the 8 waves, write the split partial (a decode step has M * G <= 8 live rows of the 32: the others are skipped)
    const int live_rows = fused ? M * G : 32;
    for (int i = threadIdx.x; i < live_rows * HD; i += 512) {
        const int r = i / HD, d = i - r * HD;
        float m2 = wm[0][r];
#pragma unroll
        for (int w = 1; w < 8; ++w) m2 = fmaxf(m2, wm[w][r]);
        float L = 0.0f, O = 0.0f;
#pragma unroll
        for (int w = 0; w < 8; ++w) {
            const float f = (wm[w][r] == -INFINITY) ? 0.0f : __expf(wm[w][r] - m2);
            L = __builtin_fmaf(wl[w][r], f, L);
            O = __builtin_fmaf(wo[w][r][d], f, O);
        }
        if (fused) {
            gran_store(r, 2 + d, O);
            if (d == 0) { gran_store(r, 0, m2); gran_store(r, 1, L); }
        } else {
            part_store(pout + r * 66 + 2 + d, O);
            if (d == 0) { part_store(pout + r * 66, m2); part_store(pout + r * 66 + 1, L); }
        }
    }
    ATL_STAMP(3);      // 8 waves merged, partial stores issued
    if (fused && sp < 8) tag_merge(M);
}
#ifdef RCA_ATTN_TIMELINE
extern "C" int rca_debug_attn_timeline(long* out_host, int enable) {   // enable: allocate + arm; else copy the 1024 x 8 stamps out
    static long* buf = nullptr;
    if (enable) {
        if (!buf) { if (hipMalloc((void**)&buf, 1024 * 16 * sizeof(long)) != hipSuccess) return 1; }
        (void)hipMemset(buf, 0, 1024 * 16 * sizeof(long));
        return hipMemcpyToSymbol(HIP_SYMBOL(rca_attn_tl), &buf, sizeof(buf)) == hipSuccess ? 0 : 1;
    }
    (void)hipDeviceSynchronize();
    return buf && hipMemcpy(out_host, buf, 1024 * 16 * sizeof(long), hipMemcpyDeviceToHost) == hipSuccess ? 0 : 1;
}
#endif
#ifdef RCA_ATTN_TIMELINE
// flash prefill attention: per wave [entry, loop start, loop end, exit] on the 100 MHz wall clock, then shader cycles summed over its
// blocks for [QK^T + mask/max, exp + sum, P split, PV], block count and the SIMD / CU it ran on (16 longs per wave)
__device__ long* rca_flash_tl = nullptr;
extern "C" int rca_debug_flash_timeline(long* out_host, int enable, int n_waves) {
    static long* buf = nullptr;
    static int cap = 0;
    if (enable) {
        if (!buf || cap < n_waves) { if (buf) (void)hipFree(buf); if (hipMalloc((void**)&buf, (size_t)n_waves * 16 * sizeof(long)) != hipSuccess) return 1; cap = n_waves; }
        (void)hipMemset(buf, 0, (size_t)cap * 16 * sizeof(long));
        return hipMemcpyToSymbol(HIP_SYMBOL(rca_flash_tl), &buf, sizeof(buf)) == hipSuccess ? 0 : 1;
    }
    (void)hipDeviceSynchronize();
    return buf && hipMemcpy(out_host, buf, (size_t)min(cap, n_waves) * 16 * sizeof(long), hipMemcpyDeviceToHost) == hipSuccess ? 0 : 1;
}
#define FTL_CLK() ((long)__builtin_readcyclecounter())
#define FTL_PHASE(k) do { const long t_now = FTL_CLK(); ftl_acc[k] += t_now - ftl_t; ftl_t = t_now; } while (0)
#else
#define FTL_PHASE(k)
#endif
// merges the splits of lm_attn_mfma_kernel as its own launch (prefill tiles, and decode steps whose grid exceeds one workgroup per
// CU): one wave per (token, head)
template <int G>
__global__ __launch_bounds__(64) void lm_attn_mfma_combine_kernel(const LmDevState* __restrict__ stt, const float* __restrict__ part,
                                                                  float* __restrict__ attn, int nh, int nkv, int n_splits, int nsp_launch,
                                                                  bf16_t* __restrict__ hi = nullptr, bf16_t* __restrict__ lo = nullptr) {
    constexpr int TPB = 32 / G;
    const int m = blockIdx.x / nh, head = blockIdx.x % nh;
    const int g = head / G, hq = head % G;
    const int qb = m / TPB, tl = m % TPB;
    const int r = tl * G + hq;
    const int d = threadIdx.x;
    const float* base = part + ((long)(qb * nkv + g) * n_splits) * 32 * 66 + r * 66;
    const float ov = attn_merge_row<false>(base, min(nsp_launch, n_splits), d);
    if (m >= stt->m) return;
    if (hi) {   // prefill tiles: the O-projection GEMM reads bf16 hi + lo
        const bf16_t hb = f32_to_bf16_rne(ov);
        hi[(long)m * nh * 64 + head * 64 + d] = hb;
        lo[(long)m * nh * 64 + head * 64 + d] = f32_to_bf16_rne(ov - __uint_as_float((unsigned)hb << 16));
    } else {
        attn[(long)m * nh * 64 + head * 64 + d] = ov;
    }
}
// the merge behind lm_attn_mfma_kernel<G, true>, grid (token of the member * head, member): the arithmetic and the bf16 hi / lo output of
// the kernel above, over the splits the member has, into the member's rows of the planes the O projection's tile GEMM reads
template <int G>
__global__ __launch_bounds__(64) void lm_attn_mfma_batch_combine_kernel(const LmBatchMember* __restrict__ tab, int nh, int nkv, int nsp_launch,
                                                                        bf16_t* __restrict__ hi, bf16_t* __restrict__ lo) {
    const LmBatchMember e = tab[blockIdx.y];
    if (!e.stt) return;   // a slot past the live count of a selection frame (rca_lm_batch_frame_sel): its table entry is all zero
    const int m = blockIdx.x / nh, head = blockIdx.x % nh;
    const int g = head / G, hq = head % G;
    const int r = m * G + hq;   // one query block per member
    const int d = threadIdx.x;
    const float* base = e.part + ((long)g * e.n_splits) * 32 * 66 + r * 66;
    const float ov = attn_merge_row<false>(base, min(nsp_launch, e.n_splits), d);
    if (m >= e.stt->m) return;
    const long o = (long)(e.row0 + m) * nh * 64 + head * 64 + d;
    const bf16_t hb = f32_to_bf16_rne(ov);
    hi[o] = hb;
    lo[o] = f32_to_bf16_rne(ov - __uint_as_float((unsigned)hb << 16));
}

// ------------------------------------------------------------------ prefill attention, flash shape
// The decode-shaped kernel above gives every block of 32 query rows one workgroup PER 256 keys and merges the partial results in a
// second launch: at 6 k tokens of context a 1024-token pass wrote and re-read 0.2 GB of partials per layer and spent 245 us in
// attention for ~50 us of MFMA work.  Prefill passes run this kernel instead: a TEAM of three waves owns a tile of 32 query rows
// (32 / G tokens x the G heads of one kv head); wave w takes the key blocks of 32 at ABSOLUTE positions 32 (3 i + w) up to the tile's
// last visible key, each wave with its own online softmax in registers, and the three (m, l, O) are merged through LDS once at the
// end -- no partials in HBM, no second launch, three waves per SIMD whose MFMA and VALU phases overlap.
// Per key block:
//   K, V:         global -> registers (one block ahead) -> the wave's two 4 KB LDS images, loaded 8 whole rows per instruction
//   S^T = K Q^T   (v_mfma_f32_32x32x16_f16; K fragments by ds_read_b128; Q scaled by scale * log2(e) and split into fp16 hi + lo
//                 once per wave) -> lane <-> query row, registers <-> keys: max / sum / rescale are per-lane scalars, p = 2^(s - m);
//                 only the blocks that reach past the tile's first row are masked (a second copy of the loop body)
//   O^T += V^T P^T: V^T fragments by ds_read_b64_tr_b16, which hands a lane 4 consecutive KEYS of its dim; B = P exactly as it sits
//                 in the S^T registers (fp16 hi + lo, hi rounded toward zero so lo is the rest, one v_fma_mix_f32 each) -> O^T has
//                 dims on registers and the query row on the lane.
//   The O^T rescale by 2^(m - m') is skipped when no lane's maximum moved (multiplying by 1.0 changes nothing).
// A query row's result depends only on its own position (every row sees the same key blocks on the same waves in the same order;
// blocks past its position contribute exact zeros behind alpha = 1, and the three partial results are merged in wave order), so the
// bits do not depend on how a prompt is cut into evals or passes -- the property the shadow KV cache rests on
// (test_mfma_prefill_is_tiling_invariant).
// Measured at 6.6 k context, per layer and 1024-token pass (profiles/r03/flash_attention_steps.txt): one wave per tile 148 us ->
// key blocks split over the waves of a workgroup 101 -> coalesced loads through LDS 90 (the direct A-layout loads took 16 bytes from
// each of 32 cache lines per instruction: 4100 of 4900 cycles per block were spent waiting on the L1) -> one workgroup per CU ~78.
#define FLASH_WAVES 3        // waves that split the key blocks of one query tile
#define FLASH_OPITCH 68      // f32 per query row of a wave's O in the merge buffer
// TEAMS query tiles per workgroup (a team = FLASH_WAVES waves = one tile).  With 4 teams a workgroup takes more than half of a CU's
// LDS, so every CU gets exactly one and the dispatcher cannot pile five tiles on one CU and three on another (measured with one tile
// per workgroup: 414 .. 730 key blocks per CU, the last CU done at 135 us against a median of 101); the four tiles of workgroup j
// are j, 2 n - 1 - j, 2 n + j and 4 n - 1 - j of the head's 4 n tiles, whose causal lengths add up to the same total for every j.
// KVQ = 1: q8_0 cache (see lm_attn_mfma_kernel): the block in flight is 2 x 16 int8 per lane and tensor plus the blocks' scales
// TAB = true (rca_lm_batch_eval): the rows of the pass are SEGMENTS of several sessions, every segment starting on a multiple of 32
// rows, so a tile (8 / 16 / 32 tokens) lies inside one segment.  `stt` is the pass's state (m = its padded row count); a tile finds
// its segment in owner[first row / 32] (-1: pad rows, the team idles as one past the pass does) and takes from tab[segment] what the
// other instances take from "the" handle: position and token count (the session's own step state), cache (+ layer, q8_0 scales),
// context bound, and its first row in qkv / hi / lo.  From there on a tile is the tile at the same LOCAL row of that session's own
// pass -- same keys on the same waves in the same order -- so its rows carry that pass's bits.  kc / vc / kd / vd / n_ctx are unused.
// The TAB = false instances are the kernel as it was before the table existed.
template <int G, int TEAMS, int KVQ = 0, bool TAB = false>
__global__ __launch_bounds__(64 * FLASH_WAVES * TEAMS, 3) void lm_attn_flash_kernel(const LmDevState* __restrict__ stt, const float* __restrict__ qkv,
                                                                        const f16_t* __restrict__ kc, const f16_t* __restrict__ vc,
                                                                        float* __restrict__ attn_out, bf16_t* __restrict__ hi, bf16_t* __restrict__ lo,
                                                                        int nh, int nkv, float scale, int n_ctx,
                                                                        const f16_t* __restrict__ kd = nullptr, const f16_t* __restrict__ vd = nullptr,
                                                                        const LmBatchMember* __restrict__ tab = nullptr, const int* __restrict__ owner = nullptr,
                                                                        int tab_layer = 0) {
    constexpr int HD = 64;
    constexpr int TPB = 32 / G;   // tokens per tile
    constexpr int NWAVES = FLASH_WAVES * TEAMS;
    // the K / V images of the key loop (8 KB per wave) and the merge buffer that follows it share one region (a barrier between the uses)
    __shared__ __attribute__((aligned(16))) float flash_lds[NWAVES * 32 * FLASH_OPITCH];
    __shared__ float mrg_m_all[NWAVES][32], mrg_l_all[NWAVES][32];
    static_assert(8192 <= sizeof(float) * 32 * FLASH_OPITCH, "K / V images fit the merge buffer");
    const int g = blockIdx.x;
    const int lane = threadIdx.x & 63;
    const int half = lane >> 5, col = lane & 31;
    const int wave_all = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int team = wave_all / FLASH_WAVES, wave = wave_all % FLASH_WAVES;
    float (*mrg_o)[32][FLASH_OPITCH] = reinterpret_cast<float (*)[32][FLASH_OPITCH]>(flash_lds) + team * FLASH_WAVES;
    float (*mrg_m)[32] = mrg_m_all + team * FLASH_WAVES;
    float (*mrg_l)[32] = mrg_l_all + team * FLASH_WAVES;
    char* const kbytes = reinterpret_cast<char*>(flash_lds) + wave_all * 8192;   // K image of the current key block: [key][128 bytes]
    char* const vbytes = kbytes + 4096;                                          // V image
    int M = stt->m;
    const int ntiles = (M + TPB - 1) / TPB;
    int tile = blockIdx.y;
    if (TEAMS == 4) {
        const int n4 = gridDim.y, j = blockIdx.y;
        tile = team == 0 ? j : team == 1 ? 2 * n4 - 1 - j : team == 2 ? 2 * n4 + j : 4 * n4 - 1 - j;
    } else if (TEAMS == 2) {
        tile = team == 0 ? (int)blockIdx.y : 2 * (int)gridDim.y - 1 - (int)blockIdx.y;
    }
    bool active = tile < ntiles;   // team-uniform; an idle team still takes part in the workgroup's barriers
    int t0, pos0 = 0;
    if constexpr (TAB) {
        // the tile's segment.  An idle team (a tile past the pass, pad rows, the unused tail of a segment) runs the prologue on the first
        // tile of segment 0 -- every address it forms is a valid one -- with no key blocks, and leaves before the merge.
        const int seg = active ? owner[(tile * TPB) >> 5] : -1;
        const LmBatchMember e = tab[max(seg, 0)];
        t0 = seg >= 0 ? tile * TPB - e.row0 : 0;   // from here on: the row inside the segment
        M = e.stt->m;
        active = seg >= 0 && t0 < M;
        if (!active) t0 = 0;
        if (TEAMS == 1 && !active) return;
        pos0 = e.stt->n_tokens;
        n_ctx = e.n_ctx;
        qkv += (long)e.row0 * (nh + 2 * nkv) * HD;
        hi += (long)e.row0 * nh * HD;
        lo += (long)e.row0 * nh * HD;
        if constexpr (KVQ) {   // int8 planes: kv_stride in bytes; the scales sc_off bytes behind them (LmBatchMember)
            kd = reinterpret_cast<const f16_t*>(reinterpret_cast<const char*>(e.kc) + e.sc_off) + (long)tab_layer * (e.kv_stride >> 5);
            vd = reinterpret_cast<const f16_t*>(reinterpret_cast<const char*>(e.vc) + e.sc_off) + (long)tab_layer * (e.kv_stride >> 5);
            kc = reinterpret_cast<const f16_t*>(reinterpret_cast<const char*>(e.kc) + (long)tab_layer * e.kv_stride);
            vc = reinterpret_cast<const f16_t*>(reinterpret_cast<const char*>(e.vc) + (long)tab_layer * e.kv_stride);
        } else {
            kc = e.kc + (long)tab_layer * e.kv_stride;
            vc = e.vc + (long)tab_layer * e.kv_stride;
        }
    } else {
        if (TEAMS == 1 && !active) return;
        t0 = min(tile, ntiles - 1) * TPB;
    }
#ifdef RCA_ATTN_TIMELINE
    long* const ftl = rca_flash_tl ? rca_flash_tl + ((long)(blockIdx.y * gridDim.x + blockIdx.x) * NWAVES + wave_all) * 16 : nullptr;
    long ftl_acc[4] = {0, 0, 0, 0}, ftl_t = 0, ftl_n = 0;
    const long ftl_entry = (long)wall_clock64();
#endif
    if constexpr (!TAB) pos0 = stt->n_tokens;
    const int ntok = min(TPB, M - t0);
    const int tl = min(col / G, ntok - 1), hq = col % G;   // rows past the pass repeat the last valid token's: they are never stored
    const int ld = (nh + 2 * nkv) * HD;
    const int qpos = pos0 + t0 + tl;
    const int kmax = min(pos0 + t0 + ntok, n_ctx);   // keys [0, kmax) are visible to the last token of this tile (and are all written)
    const int nblk = active ? (kmax + 31) >> 5 : 0;
    // ---- K / V of a key block, global -> registers -> LDS.  A load instruction covers 8 whole rows (lane l: key 8 i + l / 8, 16-byte
    // chunk l % 8 of its 128-byte row): 8 cache lines per instruction.  (Loading the MFMA A layout directly -- lane <-> key, 16 bytes of
    // each of 32 rows per instruction -- touched 32 lines for 1 KB and made the kernel wait on the L1: 4100 of 4900 cycles per block.)
    // Images: chunk c of key k sits at chunk c ^ sw(k); K: sw = (k >> 1) & 7, so the 16 lanes of a ds_read_b128 group (lane <-> key) tile
    // the 64 banks; V: sw = k1 k2 k0 (bits of k), so the 4 rows x 64 bytes of a transposed read do.  A store group is 8 lanes = one row.
    u32x4 kf[KVQ ? 2 : 4], vf[KVQ ? 2 : 4];
    f16_t ksc[2], vsc[2];
    const int ld_key = KVQ ? lane >> 2 : lane >> 3, ld_chunk = KVQ ? 2 * (lane & 3) : lane & 7;   // q8_0: 16 rows per load, the first of the lane's two chunks
    auto load_block = [&](int kb) {
        if constexpr (KVQ) {
#pragma unroll
            for (int i = 0; i < 2; ++i) {   // byte offset == element offset; a scale covers 32 of them
                const long off = ((long)min(32 * max(kb, 0) + 16 * i + ld_key, kmax - 1) * nkv + g) * HD + 8 * ld_chunk;
                kf[i] = *reinterpret_cast<const u32x4*>(reinterpret_cast<const char*>(kc) + off);
                vf[i] = *reinterpret_cast<const u32x4*>(reinterpret_cast<const char*>(vc) + off);
                ksc[i] = kd[off >> 5];
                vsc[i] = vd[off >> 5];
            }
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const long off = ((long)min(32 * max(kb, 0) + 8 * i + ld_key, kmax - 1) * nkv + g) * HD + 8 * ld_chunk;   // keys past kmax: a written row, p = 0
                kf[i] = *reinterpret_cast<const u32x4*>(kc + off);
                vf[i] = *reinterpret_cast<const u32x4*>(vc + off);
            }
        }
    };
    int kw_off[4], vw_off[4];   // q8_0: [2 i + j] = chunk ld_chunk + j of load i
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int k = KVQ ? 16 * (i >> 1) + ld_key : 8 * i + ld_key;
        const int ch = KVQ ? ld_chunk + (i & 1) : ld_chunk;
        kw_off[i] = k * 128 + ((ch ^ ((k >> 1) & 7)) << 4);
        vw_off[i] = k * 128 + ((ch ^ ((((k >> 1) & 1) << 2) | (((k >> 2) & 1) << 1) | (k & 1))) << 4);
    }
    auto stage_block = [&]() {   // the registers' block becomes the current images
        if constexpr (KVQ) {
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                u32x4 c0, c1;
                kvq8_deq16(kf[i], ksc[i], c0, c1);
                *reinterpret_cast<u32x4*>(kbytes + kw_off[2 * i]) = c0;
                *reinterpret_cast<u32x4*>(kbytes + kw_off[2 * i + 1]) = c1;
                kvq8_deq16(vf[i], vsc[i], c0, c1);
                *reinterpret_cast<u32x4*>(vbytes + vw_off[2 * i]) = c0;
                *reinterpret_cast<u32x4*>(vbytes + vw_off[2 * i + 1]) = c1;
            }
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                *reinterpret_cast<u32x4*>(kbytes + kw_off[i]) = kf[i];
                *reinterpret_cast<u32x4*>(vbytes + vw_off[i]) = vf[i];
            }
        }
    };
    load_block(min(wave, nblk - 1));
    // ---- Q of this lane's query row, times scale * log2(e), fp16 hi + lo
    f16x8 qh[4], ql[4];
    {
        const float qs = scale * 1.44269504088896340736f;
        const float* qp = qkv + (long)(t0 + tl) * ld + (g * G + hq) * HD + 8 * half;
#pragma unroll
        for (int sub = 0; sub < 4; ++sub) {
            const f32x4 a = *reinterpret_cast<const f32x4*>(qp + 16 * sub), b = *reinterpret_cast<const f32x4*>(qp + 16 * sub + 4);
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                float q = (j < 4 ? a[j] : b[j - 4]) * qs;
                // the product as ONE f32 value for both uses below.  Left to itself the compiler folds the multiply into the conversion
                // that feeds the subtraction (v_fma_mixlo_f16: the exact product rounded once) but not into the one that feeds the MFMA
                // operand (v_cvt_pk_f16_f32 of the f32 product: rounded twice); where the two differ -- a product next to the middle
                // of two fp16 values -- lo completed another hi than the one in use and the element was off by a whole fp16 ulp
                // (tests/test_attn_gpu.py: one row in a few hundred with weights off by 1e-3)
                asm("" : "+v"(q));
                const _Float16 h16 = (_Float16)q;
                qh[sub][j] = h16;
                ql[sub][j] = (_Float16)(q - (float)h16);
            }
        }
    }
    float m_run = -INFINITY, l_run = 0.0f;
    f32x16 oacc[2];
#pragma unroll
    for (int nt = 0; nt < 2; ++nt)
#pragma unroll
        for (int r = 0; r < 16; ++r) oacc[nt][r] = 0.0f;
    // K fragments: lane (key = col, half) reads chunk half + 2 sub (dims 8 half + 16 sub .. + 8) of its key
    int kr_off[4];
#pragma unroll
    for (int sub = 0; sub < 4; ++sub) kr_off[sub] = col * 128 + (((half | (sub << 1)) ^ ((col >> 1) & 7)) << 4);
    // transposed reads: lane 4 q + p of a 16-lane group supplies row (key) q, dims 4 p .. 4 p + 3 of the group's 16 dims
    int tr_off[2];
    {
        const int l16 = lane & 15, q = l16 >> 2, pp = l16 & 3;
        const int sw = ((q >> 1) << 2) | (half << 1) | (q & 1);   // rows 16 i + 4 half + q (+ 8)
#pragma unroll
        for (int nt = 0; nt < 2; ++nt) tr_off[nt] = (4 * half + q) * 128 + (((4 * nt + 2 * (col >> 4) + (pp >> 1)) ^ sw) << 4) + 8 * (pp & 1);
    }
    const int nfull = min((pos0 + t0 + 1) >> 5, nblk);   // blocks [0, nfull) are visible to every row of the tile: no mask
    auto block = [&](int kb, auto masked_t) {
        constexpr bool MASKED = decltype(masked_t)::value;
        u32x4 kcur[4];
#pragma unroll
        for (int sub = 0; sub < 4; ++sub) kcur[sub] = *reinterpret_cast<const u32x4*>(kbytes + kr_off[sub]);
        // ---- S^T = K Q^T (hi + lo), in log2 units
        f32x16 sacc;
#pragma unroll
        for (int r = 0; r < 16; ++r) sacc[r] = 0.0f;
#pragma unroll
        for (int sub = 0; sub < 4; ++sub) {
            const f16x8 kfr = __builtin_bit_cast(f16x8, kcur[sub]);
            sacc = __builtin_amdgcn_mfma_f32_32x32x16_f16(kfr, qh[sub], sacc, 0, 0, 0);
            sacc = __builtin_amdgcn_mfma_f32_32x32x16_f16(kfr, ql[sub], sacc, 0, 0, 0);
        }
        // ---- online softmax for query row `col`: register r is key 32 kb + 4 half + (r & 3) + 8 (r >> 2)
        float mx = -INFINITY;
        if (MASKED) {
            const int lim = qpos - 32 * kb - 4 * half;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float sv = ((r & 3) + 8 * (r >> 2) <= lim) ? sacc[r] : -INFINITY;
                sacc[r] = sv;
                mx = fmaxf(mx, sv);
            }
        } else {
#pragma unroll
            for (int r = 0; r < 16; ++r) mx = fmaxf(mx, sacc[r]);
        }
        {
            float a = mx, b = mx;
            asm volatile("s_nop 1\n\tv_permlane32_swap_b32 %0, %1\n\ts_nop 1" : "+v"(a), "+v"(b));
            mx = fmaxf(a, b);
        }
        FTL_PHASE(0);
        const float m_new = fmaxf(m_run, mx);
        const float m_ref = (m_new == -INFINITY) ? 0.0f : m_new;   // a row with nothing visible yet: 2^(-inf - 0) = 0 everywhere
        const float alpha = __builtin_amdgcn_exp2f(m_run - m_ref);
        float lsum = 0.0f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const float e = __builtin_amdgcn_exp2f(sacc[r] - m_ref);
            sacc[r] = e;
            lsum += e;
        }
        {
            float a = lsum, b = lsum;
            asm volatile("s_nop 1\n\tv_permlane32_swap_b32 %0, %1\n\ts_nop 1" : "+v"(a), "+v"(b));
            lsum = a + b;
        }
        l_run = l_run * alpha + lsum;
        m_run = m_new;
        if (__builtin_amdgcn_ballot_w64(alpha != 1.0f)) {   // wave-uniform
#pragma unroll
            for (int nt = 0; nt < 2; ++nt)
#pragma unroll
                for (int r = 0; r < 16; ++r) oacc[nt][r] *= alpha;
        }
        FTL_PHASE(1);
        // V^T fragments: all eight transposed reads go out before the P split below, which hides their latency.  The image was
        // written at the top of the block by this wave only (LDS operations of a wave complete in order).
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        flash_s16x4 vfr[2][2][2];   // [nt][i][key group]: lane <-> dim 32 nt + col; slot j <-> key 16 i + 4 half + 8 (j >> 2) + (j & 3)
#pragma unroll
        for (int nt = 0; nt < 2; ++nt)
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const char* tp = vbytes + tr_off[nt] + 16 * i * 128;
                vfr[nt][i][0] = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) flash_s16x4*)tp);
                vfr[nt][i][1] = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) flash_s16x4*)(tp + 8 * 128));
            }
        __builtin_amdgcn_sched_barrier(0);
        // P as the B operand of O^T += V^T P^T: registers 8 i .. 8 i + 7 feed MFMA i (fp16 hi toward zero + lo = the exact rest, rounded)
        u32x4 ph[2], pl[2];
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float p0 = sacc[8 * i + 2 * j], p1 = sacc[8 * i + 2 * j + 1];
                const unsigned h2 = __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_pkrtz(p0, p1));
                float r0, r1;   // p - (float)hi in one instruction each
                asm("v_fma_mix_f32 %0, %1, -1.0, %2 op_sel_hi:[1,0,0]" : "=v"(r0) : "v"(h2), "v"(p0));
                asm("v_fma_mix_f32 %0, %1, -1.0, %2 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "=v"(r1) : "v"(h2), "v"(p1));
                ph[i][j] = h2;
                pl[i][j] = __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_pkrtz(r0, r1));
            }
        FTL_PHASE(2);
#pragma unroll
        for (int nt = 0; nt < 2; ++nt) {
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                typedef short s16x8_t __attribute__((__vector_size__(8 * sizeof(short))));
                const s16x8_t v01 = __builtin_shufflevector(vfr[nt][i][0], vfr[nt][i][1], 0, 1, 2, 3, 4, 5, 6, 7);
                const f16x8 vb = __builtin_bit_cast(f16x8, v01);
                oacc[nt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(vb, __builtin_bit_cast(f16x8, ph[i]), oacc[nt], 0, 0, 0);
                oacc[nt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(vb, __builtin_bit_cast(f16x8, pl[i]), oacc[nt], 0, 0, 0);
            }
        }
        // the next block (in registers since the last iteration) replaces the images: this block's reads are done (one wave, LDS
        // operations complete in order); the block after it starts its way from the caches
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        stage_block();
        load_block(min(kb + 2 * FLASH_WAVES, nblk - 1));   // unconditional (the last iterations re-read a block): no merge of wait states
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    };
    stage_block();                                          // block `wave` (waits for its loads)
    load_block(min(wave + FLASH_WAVES, nblk - 1));
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    int kb = wave;
#ifdef RCA_ATTN_TIMELINE
    const long ftl_loop0 = (long)wall_clock64();
    ftl_t = FTL_CLK();
    for (; kb < nfull; kb += FLASH_WAVES) { block(kb, std::false_type{}); FTL_PHASE(3); ++ftl_n; }
    for (; kb < nblk; kb += FLASH_WAVES) { block(kb, std::true_type{}); FTL_PHASE(3); ++ftl_n; }
    const long ftl_loop1 = (long)wall_clock64();
#else
    for (; kb < nfull; kb += FLASH_WAVES) block(kb, std::false_type{});
    for (; kb < nblk; kb += FLASH_WAVES) block(kb, std::true_type{});
#endif
    // ---- the four waves' (m, l, O^T): this lane holds, for query row col, dims 32 nt + 8 (r >> 2) + 4 half + (r & 3)
    __syncthreads();   // every wave is done with its V image
    if (half == 0) { mrg_m[wave][col] = m_run; mrg_l[wave][col] = l_run; }
#pragma unroll
    for (int nt = 0; nt < 2; ++nt)
#pragma unroll
        for (int rq = 0; rq < 4; ++rq)
            *reinterpret_cast<f32x4*>(&mrg_o[wave][col][32 * nt + 8 * rq + 4 * half]) =
                f32x4{oacc[nt][4 * rq], oacc[nt][4 * rq + 1], oacc[nt][4 * rq + 2], oacc[nt][4 * rq + 3]};
    __syncthreads();
#ifdef RCA_ATTN_TIMELINE
    if (ftl && lane == 0) {
        unsigned hwid;
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hwid));
        ftl[0] = ftl_entry; ftl[1] = ftl_loop0; ftl[2] = ftl_loop1; ftl[3] = (long)wall_clock64();
        for (int k = 0; k < 4; ++k) ftl[4 + k] = ftl_acc[k];
        unsigned xcc;
        asm volatile("s_getreg_b32 %0, hwreg(20)" : "=s"(xcc));   // XCC_ID
        ftl[8] = ftl_n; ftl[9] = hwid; ftl[10] = nblk; ftl[11] = xcc & 15;
    }
#endif
    // ---- merge in wave order: thread of the team <-> (query row, 8 dims)
    if (!active) return;
    for (int idx = threadIdx.x - 64 * FLASH_WAVES * team; idx < 256; idx += 64 * FLASH_WAVES) {
        const int row = idx >> 3, d0 = 8 * (idx & 7);
        if (row / G >= ntok) break;
        float mm = mrg_m[0][row];   // wave 0 holds key 0, which every row sees: finite
#pragma unroll
        for (int w = 1; w < FLASH_WAVES; ++w) mm = fmaxf(mm, mrg_m[w][row]);
        float lsum = 0.0f, o[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) o[j] = 0.0f;
#pragma unroll
        for (int w = 0; w < FLASH_WAVES; ++w) {
            const float wgt = __builtin_amdgcn_exp2f(mrg_m[w][row] - mm);   // a wave that saw nothing: 2^-inf = 0
            lsum += mrg_l[w][row] * wgt;
            const f32x4 a = *reinterpret_cast<const f32x4*>(&mrg_o[w][row][d0]), b = *reinterpret_cast<const f32x4*>(&mrg_o[w][row][d0 + 4]);
#pragma unroll
            for (int j = 0; j < 4; ++j) { o[j] += a[j] * wgt; o[4 + j] += b[j] * wgt; }
        }
        const float inv = 1.0f / lsum;
#pragma unroll
        for (int j = 0; j < 8; ++j) o[j] *= inv;
        const long obase = (long)(t0 + row / G) * nh * HD + (long)(g * G + row % G) * HD + d0;
        if (hi) {   // prefill tiles: the O-projection GEMM reads bf16 hi + lo
            unsigned ph2[4], pl2[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const bf16_t h0 = f32_to_bf16_rne(o[2 * j]), h1 = f32_to_bf16_rne(o[2 * j + 1]);
                const bf16_t l0 = f32_to_bf16_rne(o[2 * j] - __uint_as_float((unsigned)h0 << 16));
                const bf16_t l1 = f32_to_bf16_rne(o[2 * j + 1] - __uint_as_float((unsigned)h1 << 16));
                ph2[j] = (unsigned)h0 | ((unsigned)h1 << 16);
                pl2[j] = (unsigned)l0 | ((unsigned)l1 << 16);
            }
            *reinterpret_cast<uint4*>(hi + obase) = make_uint4(ph2[0], ph2[1], ph2[2], ph2[3]);
            *reinterpret_cast<uint4*>(lo + obase) = make_uint4(pl2[0], pl2[1], pl2[2], pl2[3]);
        } else {
            *reinterpret_cast<float4*>(attn_out + obase) = make_float4(o[0], o[1], o[2], o[3]);
            *reinterpret_cast<float4*>(attn_out + obase + 4) = make_float4(o[4], o[5], o[6], o[7]);
        }
    }
}
// The one place that turns a head-group size or a team count (4, 2 or 1), or a yes / no, into a template argument (wf_dispatch's way)
template <class F>
static void lm_dispatch_421(int v, F&& f) {
    if (v == 4) f(std::integral_constant<int, 4>{});
    else if (v == 2) f(std::integral_constant<int, 2>{});
    else f(std::integral_constant<int, 1>{});
}
template <class F>
static void lm_dispatch_bool(bool v, F&& f) {
    if (v) f(std::true_type{});
    else f(std::false_type{});
}
// what a pass of rca_lm_batch_eval reads about its segments (device pointers into the block the pass uploaded)
struct LmEvalTables {
    const LmGroupRow* rows;      // [padded rows of the pass]: the QKV epilogue's row table; a pad row has n_ctx 0 and stores nothing
    const LmBatchMember* tab;    // [n_seg]
    const int* owner;            // [LM_MAXM / 32]: segment of every 32 rows, -1 = pad rows behind the last segment
    bool q8;
};
// Every flash launch.  The handle's own pass: M tokens on its cache (kc / vc of the layer, kd / vd its q8_0 scales or null).  With t, the
// table instance: one launch for every segment of a pass of M rows, cache and position per segment from the table (layer l), no
// cache argument.  Teams per workgroup, from the pass's total tile count: 4 (one workgroup per CU) once that still gives every CU of
// the device a workgroup, else 2, else 1.
static void launch_attention_flash(rca_lm* h, int M, const f16_t* kc, const f16_t* vc, hipStream_t st, bf16_t* hi, bf16_t* lo, const f16_t* kd, const f16_t* vd,
                                   const LmEvalTables* t = nullptr, int l = 0) {
    const rca_lm_config_t& c = h->cfg;
    const float scale = 1.0f / sqrtf((float)c.head_dim);
    const int G = c.n_heads / c.n_kv_heads;
    const int ntiles = cdiv(M * G, 32);
    int teams = 1;
    if (c.n_kv_heads * cdiv(ntiles, 4) >= h->n_cus) teams = 4;
    else if (c.n_kv_heads * cdiv(ntiles, 2) >= h->n_cus) teams = 2;
    lm_dispatch_421(G, [&](auto g) { lm_dispatch_421(teams, [&](auto tm) { lm_dispatch_bool(t ? t->q8 : kd != nullptr, [&](auto q) { lm_dispatch_bool(t != nullptr, [&](auto tb) {
        constexpr int TEAMS = decltype(tm)::value;
        lm_attn_flash_kernel<decltype(g)::value, TEAMS, decltype(q)::value ? 1 : 0, decltype(tb)::value><<<dim3(c.n_kv_heads, cdiv(ntiles, TEAMS)), 64 * FLASH_WAVES * TEAMS, 0, st>>>(
            h->stt, h->qkv, kc, vc, h->attn, hi, lo, c.n_heads, c.n_kv_heads, scale, t ? 0 : c.n_ctx, kd, vd, t ? t->tab : nullptr, t ? t->owner : nullptr, l);
    }); }); }); });
}
static void launch_attention_flash_tab(rca_lm* h, int rows, hipStream_t st, bf16_t* hi, bf16_t* lo, const LmEvalTables& t, int l) {
    launch_attention_flash(h, rows, nullptr, nullptr, st, hi, lo, nullptr, nullptr, &t, l);
}
// the q8_0 quantiser of layer l over the rows the pass has just stored into the ring (nothing to do for an fp16 cache).  m_max: the
// most tokens the pass can have (the grid); the live count and the position are read on the device
static void lm_launch_kv_quant(rca_lm* h, int l, int m_max, hipStream_t st) {
    if (!lm_kv_q8(h)) return;
    const rca_lm_config_t& c = h->cfg;
    lm_kv_quant_kernel<false><<<dim3(cdiv(4 * c.n_kv_heads, 8), m_max), 256, 0, st>>>(
        h->stt, h->ring_k, h->ring_v, LM_KV_RING - 1, reinterpret_cast<signed char*>(lm_kv_layer(h, h->kc, l)), reinterpret_cast<signed char*>(lm_kv_layer(h, h->vc, l)),
        const_cast<f16_t*>(lm_kv_scales(h, h->kc, l)), const_cast<f16_t*>(lm_kv_scales(h, h->vc, l)), c.n_kv_heads, c.n_ctx, 0, 0, 3, nullptr, 0);
}

// a member's entry of a batch table (either cache format)
static LmBatchMember lm_batch_member(const rca_lm* h, int row0, bool serial) {
    return LmBatchMember{h->stt, h->kc, h->vc, h->kv_layer_stride, h->att_part, h->logits, h->samp, h->swork, row0, h->n_splits, h->cfg.n_ctx, serial ? 1 : 0,
                         lm_kv_q8(h) ? lm_kv_sc_off(h) : 0, h->ring_k, h->ring_v, LM_KV_RING - 1, 0};
}
// RCA_LM_FLASH / RCA_LM_TILE_GRAPHS: unset or non-zero = on; read once per process
static bool lm_env_on(const char* name) {
    const char* v = getenv(name);
    return !(v && atoi(v) == 0);
}
static bool lm_env_flash() {   // 0: A/B runs against the split kernel
    static const bool v = lm_env_on("RCA_LM_FLASH");
    return v;
}
static bool lm_env_tile_graphs() {   // 0: every prefill tile pass is launched eagerly
    static const bool v = lm_env_on("RCA_LM_TILE_GRAPHS");
    return v;
}
// the dynamic LDS of every instance of the split kernel, once per process; called where a pass is about to launch one eagerly
static void lm_attn_split_attrs() {
    static bool done = false;
    if (done) return;
    for (int G : {4, 2, 1})
        lm_dispatch_421(G, [](auto g) {
            constexpr int GG = decltype(g)::value;
            (void)hipFuncSetAttribute((const void*)lm_attn_mfma_kernel<GG>, hipFuncAttributeMaxDynamicSharedMemorySize, ATTM_LDS);
            (void)hipFuncSetAttribute((const void*)lm_attn_mfma_kernel<GG, false, 1>, hipFuncAttributeMaxDynamicSharedMemorySize, ATTM_LDS);
            (void)hipFuncSetAttribute((const void*)lm_attn_mfma_kernel<GG, true>, hipFuncAttributeMaxDynamicSharedMemorySize, ATTM_LDS);
            (void)hipFuncSetAttribute((const void*)lm_attn_mfma_kernel<GG, true, 1>, hipFuncAttributeMaxDynamicSharedMemorySize, ATTM_LDS);
        });
    done = true;
}
// Every launch of the split kernel.  A handle's own pass (tab null): its state, the layer's cache, and for a q8_0 cache the distance
// to the scales in tab_layer.  A batch pass: a member per grid z from tab, layer tab_layer, everything else null / 0.  The merge of
// the splits (in-launch, combine kernel or batch combine kernel) is the caller's.
static void lm_launch_attn_split(const rca_lm_config_t& c, dim3 grid, bool q8, hipStream_t st, const LmDevState* stt, const float* qkv, const f16_t* kc, const f16_t* vc,
                                 int n_splits, int n_ctx, float* part, int* arrive, float* attn, const LmBatchMember* tab, int tab_layer) {
    const float scale = 1.0f / sqrtf((float)c.head_dim);
    lm_dispatch_421(c.n_heads / c.n_kv_heads, [&](auto g) { lm_dispatch_bool(tab != nullptr, [&](auto tb) { lm_dispatch_bool(q8, [&](auto q) {
        lm_attn_mfma_kernel<decltype(g)::value, decltype(tb)::value, decltype(q)::value ? 1 : 0><<<grid, 512, ATTM_LDS, st>>>(
            stt, qkv, kc, vc, c.n_heads, c.n_kv_heads, n_splits, scale, n_ctx, part, arrive, attn, tab, tab_layer);
    }); }); });
}
// split attention on MFMA + merge of the splits, for the M tokens of the current pass
// qkv / attn: the M query rows and where their outputs go -- the handle's own buffers for its own passes, the rows of ONE member inside the
// shared buffers of a group step (the flash route, prefill only, reads the handle's)
static void launch_attention_mfma(rca_lm* h, int M, int nsp_launch, const f16_t* kc, const f16_t* vc, const float* qkv, float* attn, hipStream_t st,
                                  bf16_t* hi = nullptr, bf16_t* lo = nullptr, bool prefill = false) {
    const rca_lm_config_t& c = h->cfg;
    // q8_0 cache: kc / vc are a layer of the int8 planes (lm_kv_layer); its scales sit at the same element offset / 32 of the scale plane
    const f16_t *kd = nullptr, *vd = nullptr;
    if (lm_kv_q8(h)) {
        kd = lm_kv_scales(h, h->kc, 0) + (((const char*)kc - (const char*)h->kc) >> 5);
        vd = lm_kv_scales(h, h->vc, 0) + (((const char*)vc - (const char*)h->vc) >> 5);
    }
    if (prefill && lm_env_flash()) {   // every pass of the prefill-tile path, whatever its size: pieces of one long eval must use ONE arithmetic
        launch_attention_flash(h, M, kc, vc, st, hi, lo, kd, vd);
        return;
    }
    const int G = c.n_heads / c.n_kv_heads;
    const int sc_units = kd ? (int)(((const char*)kd - (const char*)kc) >> 4) : 0;   // (lm_kv_alloc keeps a plane below 2^35 bytes)
    dim3 agm(c.n_kv_heads, nsp_launch, cdiv(M * G, 32));
    lm_attn_split_attrs();
    // decode steps: the merge of the splits is fused into the attention launch while the grid is at most one workgroup per CU (the
    // regime the sc1 hand-off is measured for); prefill tiles and longer contexts keep the separate combine launch
    const bool fuse = h->fuse_attn && !hi && agm.z == 1 && c.n_kv_heads * nsp_launch <= 256 && M * G <= 8 && nsp_launch <= ATT_TAG_MAXSP && c.n_kv_heads <= ATT_EPOCH_INTS;
    lm_launch_attn_split(c, agm, kd != nullptr, st, h->stt, qkv, kc, vc, h->n_splits, c.n_ctx, h->att_part, fuse ? h->att_arrive : nullptr, attn, nullptr, sc_units);
    if (!fuse)
        lm_dispatch_421(G, [&](auto g) {
            lm_attn_mfma_combine_kernel<decltype(g)::value><<<M * c.n_heads, 64, 0, st>>>(h->stt, h->att_part, attn, c.n_heads, c.n_kv_heads, h->n_splits, nsp_launch, hi, lo);
        });
}

// attention split blocks needed by a pass of m tokens on top of the current context
static int lm_splits_needed(const rca_lm* h, int m) { return std::min(h->n_splits, (h->n_tokens + m + ATT_KEYS - 1) / ATT_KEYS); }

// The five projections of a decode pass over M <= 2 tokens: each function owns the argument list of its launch, so whoever runs a
// stage (lm_enqueue_pass, the head behind a prefill, rca_lm_gemv_tap for the tests) runs the same launch.
static const GemvPro nopro{nullptr, nullptr, 0.0f, 0};
static const GemvRope norope{nullptr, nullptr, nullptr, nullptr, 0, 0, 0, 0};
static const GemvGroup nogroup{nullptr, 0};
static void lm_launch_qkv(rca_lm* h, int l, int M, hipStream_t st) {   // RMSNorm(x) -> [q; k; v] + RoPE -> qkv, KV cache of layer l
    const rca_lm_config_t& c = h->cfg;
    const LmLayer& L = h->layers[l];
    const int QKV = (c.n_heads + 2 * c.n_kv_heads) * c.head_dim;
    const GemvPro pro{h->x, L.attn_norm, c.rms_eps, 0};
    GemvRope rope{h->cos_t, h->sin_t, nullptr, nullptr, c.n_heads, c.n_kv_heads, c.n_ctx, 0};
    lm_rope_target(h, l, rope);
    launch_gemv<1, 2>(GEMV_QKV, h, M, L.qkv, nullptr, h->qkv, L.qkv.N, c.hidden, QKV, pro, rope, st);
    if (L.split_v) {   // the V projection of this layer is kept in another format than Q / K (a Q4_K_M file): its own launch
        rope.row_base = L.qkv.N;
        launch_gemv<1, 2>(GEMV_QKV, h, M, L.vseg, nullptr, h->qkv, L.vseg.N, c.hidden, QKV, pro, rope, st);
    }
    lm_launch_kv_quant(h, l, M, st);
}
static void lm_launch_o(rca_lm* h, int l, int M, hipStream_t st) {   // x += O attn
    const int AO = h->cfg.n_heads * h->cfg.head_dim;
    launch_gemv<0, 3>(GEMV_O, h, M, h->layers[l].o, h->attn, h->x, h->cfg.hidden, AO, h->cfg.hidden, nopro, norope, st);
}
static void lm_launch_gu(rca_lm* h, int l, int M, hipStream_t st) {   // RMSNorm(x) -> silu(gate) * up -> hbuf
    const rca_lm_config_t& c = h->cfg;
    const LmLayer& L = h->layers[l];
    launch_gemv<1, 1>(GEMV_GU, h, M, L.gu, nullptr, h->hbuf, 2 * c.ffn, c.hidden, c.ffn, GemvPro{h->x, L.ffn_norm, c.rms_eps, 0}, norope, st);
}
static void lm_launch_down(rca_lm* h, int l, int M, hipStream_t st) {   // x += down hbuf
    launch_gemv<0, 3>(GEMV_DOWN, h, M, h->layers[l].down, h->hbuf, h->x, h->cfg.hidden, h->cfg.ffn, h->cfg.hidden, nopro, norope, st);
}
// final RMSNorm + head over M rows of x -> out[M][vocab]; only_last (M = 1): the row is the pass's last token
static void lm_launch_head(rca_lm* h, int M, hipStream_t st, float* out, bool only_last) {
    const rca_lm_config_t& c = h->cfg;
    launch_gemv<1, 0>(GEMV_HEAD, h, M, h->head, nullptr, out, c.vocab_size, c.hidden, c.vocab_size, GemvPro{h->x, h->final_norm, c.rms_eps, only_last ? 1 : 0}, norope, st);
}

// Enqueue one decode pass over the M <= 2 tokens whose ids / position are already in h->stt (device).
// want_logits: 0 none, 1 last token only, 2 every token (logits_all).
// Per layer: [norm+QKV+RoPE/KV-write] -> [split attention] -> [combine] -> [O proj + residual] -> [norm+gate/up+SwiGLU] -> [down + residual]
// nsp_launch: attention split blocks to launch (>= ceil((n_tokens + M) / ATT_KEYS); later splits exit at once).
static int lm_enqueue_pass(rca_lm* h, int M, int want_logits, hipStream_t st, int nsp_launch, bool skip_embed = false) {
    const rca_lm_config_t& c = h->cfg;
    if (M < 1 || M > LM_GEMV_M) return fail(RCA_ERR_ARG, "decode pass of %d tokens", M);
    if (!skip_embed) lm_embed_kernel<<<M, 256, 0, st>>>(h->stt, h->embed, h->embed_f32, h->x, c.hidden, c.vocab_size);   // (inside a frame graph the previous step's sampler has gathered the rows)
    for (int l = 0; l < c.n_layers; ++l) {
        lm_launch_qkv(h, l, M, st);
        launch_attention_mfma(h, M, nsp_launch, lm_kv_layer(h, h->kc, l), lm_kv_layer(h, h->vc, l), h->qkv, h->attn, st);
        lm_launch_o(h, l, M, st);
        lm_launch_gu(h, l, M, st);
        lm_launch_down(h, l, M, st);
    }
    if (want_logits == 1) lm_launch_head(h, 1, st, h->logits, true);
    else if (want_logits) lm_launch_head(h, M, st, h->logits, false);
    RCA_LAUNCH_CHECK();
    return RCA_OK;
}

// One prefill tile (M <= 32 tokens already described by h->stt): projections on bf16 MFMA with hi/lo-split
// activations, attention through the same split-KV kernels.  Leaves the residual stream in h->x.
// ------------------------------------------------------------------ prefill GEMM, 128 weight rows x 128 tokens
// Y[tok][n] = sum_k W[n][k] * (xh + xl)[tok][k] on v_mfma_f32_32x32x16_bf16, LDS-staged and double-buffered.
// Workgroup = 4 waves in a 2 x 2 grid, each wave 64 rows x 64 tokens (2 x 2 MFMA tiles, hi and lo passes share the
// weight fragment).  A stage is 32 k: three 128 x 32 bf16 tiles (W, xh, xl) fetched with 16-byte loads one stage
// ahead and kept in LDS rows of 40 bf16 (80 B: the 16-byte fragment reads of 8 consecutive rows hit 8 distinct
// 4-bank groups).  Weights are read from HBM once per 128 tokens instead of once per 32.
// grid (N / 128, k splits): with one split the epilogue is fused (RoPE + KV write, SwiGLU + hi/lo split, residual
// add); with several (the narrow N = hidden projections, to put more than 16 workgroups on the chip) each split
// stores its partial sums and lm_gemm128_epilogue_kernel adds them in split order and runs the epilogue -- deterministic.
#define G128_PITCH 40
#define G128_LDS_T(NT) (2 * (NT) * 128 * G128_PITCH * 2)
#define G128_LDS G128_LDS_T(3)
// Weight formats other than bf16 (WF): the matrix is kept ONCE, in the format the decode GEMV streams, and de-quantised while it is
// staged -- a thread turns its 16 weights of the stage into f32 (fp16: widened; q8_0: d * q, exact in f32) and splits each into
// bf16 hi + bf16 lo (hi = RNE(w), lo = RNE(w - hi): exact for fp16 values, within 2^-17 for d * q), written to a fourth LDS tile.
// Three MFMAs per k step instead of two: w_hi x_hi + w_hi x_lo + w_lo x_hi (the dropped w_lo x_lo term is below the 16 bits the
// activation split keeps anyway).  So prefill and decode see the same weights to 2^-17, whatever the format.
typedef __bf16 bf16x2_t __attribute__((ext_vector_type(2)));
__device__ __forceinline__ unsigned pack_bf16x2(float a, float b) {   // v_cvt_pk_bf16_f32: round to nearest even
    const bf16x2_t v = {(__bf16)a, (__bf16)b};
    return __builtin_bit_cast(unsigned, v);
}
__device__ __forceinline__ void split_w8(const float (&w)[8], uint4& hi, uint4& lo) {
    unsigned ph[4], pl[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        ph[j] = pack_bf16x2(w[2 * j], w[2 * j + 1]);
        pl[j] = pack_bf16x2(w[2 * j] - bf16_lo(ph[j]), w[2 * j + 1] - bf16_hi(ph[j]));
    }
    hi = make_uint4(ph[0], ph[1], ph[2], ph[3]);
    lo = make_uint4(pl[0], pl[1], pl[2], pl[3]);
}
template <int EPI, int WF>
__global__ __launch_bounds__(256, 2) void lm_gemm128_kernel(const LmDevState* __restrict__ stt, const bf16_t* __restrict__ W, GemvQ8 q8,
                                                            const bf16_t* __restrict__ xh, const bf16_t* __restrict__ xl, int N, int K,
                                                            int kslice, float* __restrict__ y, int ldy, bf16_t* __restrict__ oh,
                                                            bf16_t* __restrict__ ol, float* __restrict__ part, GemvRope rope, int nseq,
                                                            GemvGroup grp) {
    constexpr bool ROPE = EPI == GEMM_EPI_ROPE || EPI == GEMM_EPI_ROPE_ROWS;   // the weight rows of the fused QKV matrix: pairs (d, d + 32) of one head
    // nseq > 1: this workgroup walks nseq consecutive k slices itself.  Each slice is summed into a fresh accumulator and that is
    // added to a running total -- exactly the additions, in exactly the order, of "every slice its own workgroup, then
    // lm_gemm128_epilogue_kernel adds the partial sums starting from 0" -- so the result does not depend on which of the two forms a
    // pass used, and the partial sums never travel through HBM.  Used where the token blocks alone fill the chip.
    constexpr int NT = WF == WF_BF16 ? 3 : 4;   // LDS tiles per buffer: W (hi), xh, xl [, W lo]
    extern __shared__ __attribute__((aligned(16))) bf16_t g128_lds[];   // [2 buffers][NT][128 rows][G128_PITCH]
    typedef bf16_t tile_t[NT][128 * G128_PITCH];
    tile_t* sm = reinterpret_cast<tile_t*>(g128_lds);
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int half = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wr = wave >> 1, wc = wave & 1;
    const int n0 = blockIdx.x * 128;
    const int ks = blockIdx.y * nseq * kslice;
    const int tb = blockIdx.z * 128;   // token block of this workgroup: a pass holds up to LM_MAXM / 128 of them, the weights are
                                       // fetched from HBM by the first and served from L2 / Infinity Cache to the others
    const int spf = kslice >> 5;          // stages per slice
    const int nstage = nseq * spf;
    // staging role: two 16-byte chunks per tile and thread: rows c >> 2, k offset (c & 3) * 8
    const int srow0 = tid >> 2, skc = (tid & 3) * 8;
    // GEMM_EPI_LOGITS: N (the vocabulary) is no multiple of 128, so the last row tile clamps every weight address to the last valid
    // row / pair / quad (the packed formats are loaded with N % 2 == 0 resp. N % 4 == 0) -- no read passes the end of the matrix or of
    // its scale arrays; the rows staged twice that way are masked at the store (n >= N).  The other epilogues see what they always saw.
    constexpr bool RAGGED = EPI == GEMM_EPI_LOGITS;
    const int wrow0 = RAGGED ? min(n0 + srow0, N - 1) : n0 + srow0;
    const bf16_t* gW = W + (long)wrow0 * K + ks + skc;
    const bf16_t* gH = xh + (long)(tb + srow0) * K + ks + skc;
    const bf16_t* gL = xl + (long)(tb + srow0) * K + ks + skc;
    const long rstep = 64L * K;     // second chunk: row + 64
    const long wstep = RAGGED ? (long)(min(n0 + srow0 + 64, N - 1) - wrow0) * K : rstep;
    const int soff0 = srow0 * G128_PITCH + skc, soff1 = soff0 + 64 * G128_PITCH;
    // q8_0: a thread's stage is ONE 16-byte unit of the packed layout = 8 k of the two rows of pair (n0 / 2 + tid / 4); the pair's
    // rows are (2p, 2p + 1), or (d, d + 32) of one head in the fused QKV matrix (the only matrix that runs the RoPE epilogue)
    const int qp = tid >> 2;
    const long q_nkb = K >> 5;
    const int gpair = RAGGED ? min((n0 >> 1) + qp, (N >> 1) - 1) : (n0 >> 1) + qp;
    const u32x4* gQ = (WF == WF_Q8 || WF == WF_Q6K) ? q8.qs + (long)gpair * (K >> 3) + (ks >> 3) + (tid & 3) : nullptr;
    const unsigned* gS = WF == WF_Q8 ? q8.sc + q8_sc_index(gpair, ks >> 5, q_nkb) : nullptr;   // next k block: + 8
    const float* gS6 = WF == WF_Q6K ? reinterpret_cast<const float*>(q8.sc) + 2 * q8_sc_index(gpair, (ks >> 4) + ((tid & 3) >> 1), K >> 4) : nullptr;   // next stage: + 2 groups of 16
    // Q4_K: a thread's stage is HALF a 16-byte unit = 8 k of two adjacent slots: quad tid / 8, chunk (tid / 2) % 4, slots 2 (tid % 2) + {0, 1}
    const int q4quad = tid >> 3, q4half = tid & 1;
    const int gquad = RAGGED ? min((n0 >> 2) + q4quad, (N >> 2) - 1) : (n0 >> 2) + q4quad;
    const int q4slot = 4 * gquad + 2 * q4half;
    constexpr bool WIQ = WF == WF_IQ4;                  // IQ4_NL / IQ4_XS: the same staging as Q4_0, the dword is the f32 factor s and the nibbles are table indices
    constexpr bool W40 = WF == WF_Q40 || WIQ;           // Q4_0 / Q4_1: the Q4_K staging with the (s | t << 16) dword of each slot and stage
    constexpr bool W4 = WF == WF_Q4K || WF == WF_Q5K || W40;   // Q5_K: the Q4_K staging + the quad's dword of high bits (arrives as W)
    const unsigned* gH5 = WF == WF_Q5K ? reinterpret_cast<const unsigned*>(W) + (long)gquad * (K >> 3) + (ks >> 3) + ((tid >> 1) & 3) : nullptr;
    const uint2* gQ4 = W4 ? reinterpret_cast<const uint2*>(q8.qs + (long)gquad * (K >> 3) + (ks >> 3) + ((tid >> 1) & 3)) + q4half : nullptr;
    const unsigned short* gS4 = (W4 && !W40) ? reinterpret_cast<const unsigned short*>(q8.sc) + q4k_scm_index(q4slot, ks >> 5, q_nkb) : nullptr;   // next sub-block: + 16
    const unsigned* gF40 = W40 ? q8.sc + q4k_scm_index(q4slot, ks >> 5, q_nkb) : nullptr;                                                      // next block: + 16
    const unsigned* gD4 = (W4 && !W40) ? q8.dd + q4k_scm_index(q4slot, 0, K >> 8) : nullptr;                                                     // super-block k / 256: + 16 each
    int q4row[2];   // LDS rows of the two slots
#pragma unroll
    for (int i = 0; i < 2; ++i) q4row[i] = (int)packed_slot_row(4 * q4quad + 2 * q4half + i, ROPE);
    const int q4soff0 = q4row[0] * G128_PITCH + ((tid >> 1) & 3) * 8, q4soff1 = q4row[1] * G128_PITCH + ((tid >> 1) & 3) * 8;
    const int qra = ROPE ? (qp >> 5) * 64 + (qp & 31) : 2 * qp;
    const int qsoff0 = qra * G128_PITCH + skc, qsoff1 = qsoff0 + (ROPE ? 32 : 1) * G128_PITCH;
    // Software pipeline.  A workgroup's stage needs 8 KB of weights straight from HBM (~2 us away) and 16 KB of
    // activations from L2 (~0.7 us): weight chunks are requested DW stages ahead, activation chunks DX stages ahead,
    // both held in registers until their LDS buffer is free.
    constexpr int DW = 1, DX = 1;   // measured: deeper register prefetch (4 / 2) is slower at 2 workgroups per CU
    uint4 rw[DW][2], rh[DX][2], rl[DX][2];
    unsigned rs[DW];
    uint2 rdd[DW];
    auto gload_w = [&](int slot, int s) {
        const int st = min(s, nstage - 1);
        if (W4) {
            const uint2 t = gQ4[(long)st * 8];                       // + 4 units of 16 bytes per stage
            rw[slot][0] = make_uint4(t.x, t.y, WF == WF_Q5K ? gH5[(long)st * 4] : 0u, 0u);
            if constexpr (W40) {
                rdd[slot] = *reinterpret_cast<const uint2*>(gF40 + (long)st * 16);       // (s | t << 16) of the two slots
            } else {
                rs[slot] = *reinterpret_cast<const unsigned*>(gS4 + (long)st * 16);          // (sc | m << 8) of the two slots
                rdd[slot] = *reinterpret_cast<const uint2*>(gD4 + (long)(((ks >> 5) + st) >> 3) * 16);   // (d | dmin << 16) of the two slots
            }
        } else if (WF == WF_Q6K) {
            const u32x4 t = gQ[st * 4];
            rw[slot][0] = make_uint4(t.x, t.y, t.z, t.w);
            rdd[slot] = *reinterpret_cast<const uint2*>(gS6 + (long)st * 2 * 16);   // (s_a, s_b): two groups of 16 per stage, 8 pairs x 2 floats per group
        } else if (WF == WF_Q8) {
            const u32x4 t = gQ[st * 4];
            rw[slot][0] = make_uint4(t.x, t.y, t.z, t.w);
            rs[slot] = gS[(long)st * 8];
        } else {
            const int k = st << 5;
            rw[slot][0] = *reinterpret_cast<const uint4*>(gW + k); rw[slot][1] = *reinterpret_cast<const uint4*>(gW + wstep + k);
        }
    };
    auto gload_x = [&](int slot, int s) {
        const int k = min(s, nstage - 1) << 5;
        rh[slot][0] = *reinterpret_cast<const uint4*>(gH + k); rh[slot][1] = *reinterpret_cast<const uint4*>(gH + rstep + k);
        rl[slot][0] = *reinterpret_cast<const uint4*>(gL + k); rl[slot][1] = *reinterpret_cast<const uint4*>(gL + rstep + k);
    };
    auto swrite = [&](int buf, int ws, int xs) {
        if (WF == WF_BF16) {
            *reinterpret_cast<uint4*>(&sm[buf][0][soff0]) = rw[ws][0]; *reinterpret_cast<uint4*>(&sm[buf][0][soff1]) = rw[ws][1];
        } else if (WF == WF_F16) {
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                const unsigned u[4] = {rw[ws][c].x, rw[ws][c].y, rw[ws][c].z, rw[ws][c].w};
                float wv[8];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const f16x2 h2 = __builtin_bit_cast(f16x2, u[j]);
                    wv[2 * j] = (float)h2[0];
                    wv[2 * j + 1] = (float)h2[1];
                }
                uint4 hi, lo;
                split_w8(wv, hi, lo);
                *reinterpret_cast<uint4*>(&sm[buf][0][c ? soff1 : soff0]) = hi;
                *reinterpret_cast<uint4*>(&sm[buf][3][c ? soff1 : soff0]) = lo;
            }
        } else if (W4) {   // .x / .y = 8 nibbles of the first / second slot (.z: Q5_K's high bits); the value is dequantize_row_q4_K's (d sc) q - (dmin m)
            const unsigned qw[2] = {rw[ws][0].x, rw[ws][0].y}, ddw[2] = {rdd[ws].x, rdd[ws].y};
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                const unsigned scm = W40 ? 0u : (rs[ws] >> (16 * c)) & 0xffffu;
                float wv[8];
                if constexpr (WIQ) {   // s kv[q], exact: the table stays in scalar registers (iq4_map4), four look-ups per permute triple
                    const unsigned klo = iq4_map4<0>(qw[c]), khi = iq4_map4<4>(qw[c]);
                    const float s1 = __uint_as_float(ddw[c]);
#pragma unroll
                    for (int b = 0; b < 4; ++b) {
                        wv[2 * b] = s1 * q8_byte_to_f32(klo, b);
                        wv[2 * b + 1] = s1 * q8_byte_to_f32(khi, b);
                    }
                } else {
#pragma unroll
                    for (int j = 0; j < 8; ++j) {
                        unsigned qv = (qw[c] >> (4 * j)) & 0xFu;
                        if (WF == WF_Q5K) qv |= ((rw[ws][0].z >> q5k_hbit(2 * q4half + c, j)) & 1u) << 4;
                        wv[j] = W40 ? q40_value(ddw[c], qv) : q4k_value(ddw[c], scm, qv);   // Q4_0 / Q4_1: s q - t
                    }
                }
                uint4 hi, lo;
                split_w8(wv, hi, lo);
                *reinterpret_cast<uint4*>(&sm[buf][0][c ? q4soff1 : q4soff0]) = hi;
                *reinterpret_cast<uint4*>(&sm[buf][3][c ? q4soff1 : q4soff0]) = lo;
            }
        } else {   // q8_0: .x .y = 8 int8 of the pair's first row, .z .w = of its second row; rs = (fp16 d_a, fp16 d_b); Q6_K: rdd = (f32 s_a, f32 s_b)
            const f16x2 d2 = __builtin_bit_cast(f16x2, rs[ws]);
            const unsigned u[4] = {rw[ws][0].x, rw[ws][0].y, rw[ws][0].z, rw[ws][0].w};
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                const float dd = WF == WF_Q6K ? __uint_as_float(c ? rdd[ws].y : rdd[ws].x) : (float)d2[c];
                float wv[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) wv[j] = dd * (float)(signed char)((u[2 * c + (j >> 2)] >> (8 * (j & 3))) & 0xffu);
                uint4 hi, lo;
                split_w8(wv, hi, lo);
                *reinterpret_cast<uint4*>(&sm[buf][0][c ? qsoff1 : qsoff0]) = hi;
                *reinterpret_cast<uint4*>(&sm[buf][3][c ? qsoff1 : qsoff0]) = lo;
            }
        }
        *reinterpret_cast<uint4*>(&sm[buf][1][soff0]) = rh[xs][0]; *reinterpret_cast<uint4*>(&sm[buf][1][soff1]) = rh[xs][1];
        *reinterpret_cast<uint4*>(&sm[buf][2][soff0]) = rl[xs][0]; *reinterpret_cast<uint4*>(&sm[buf][2][soff1]) = rl[xs][1];
    };
    f32x16 acc[2][2], tot[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) { acc[i][j][r] = 0.0f; tot[i][j][r] = 0.0f; }
    // fragment read offsets: row (lane & 31) of the 32-row tile, k offset 8 * half inside a 16-k substep
    const int fa = (wr * 64 + (lane & 31)) * G128_PITCH + 8 * half;
    const int fb = (wc * 64 + (lane & 31)) * G128_PITCH + 8 * half;
#pragma unroll
    for (int d = 0; d < DW; ++d) gload_w(d, d);
#pragma unroll
    for (int d = 0; d < DX; ++d) gload_x(d, d);
    swrite(0, 0, 0);
    __syncthreads();
    // stage s: weights in slot s % DW, activations in slot s % DX; the loop is unrolled by DW (a multiple of DX)
    for (int s0 = 0; s0 < nstage; s0 += DW) {
#pragma unroll
        for (int d = 0; d < DW; ++d) {
            const int s = s0 + d;
            if (s >= nstage) break;
            const int buf = s & 1;
            // slots of stage s are in LDS: refill them with the stages DW / DX ahead
            gload_w(d, s + DW);
            gload_x(d % DX, s + DX);
#pragma unroll
            for (int ksub = 0; ksub < 2; ++ksub) {
                bf16x8 a[2], al[2], bh[2], bl[2];
#pragma unroll
                for (int i = 0; i < 2; ++i) {
                    a[i] = *reinterpret_cast<const bf16x8*>(&sm[buf][0][fa + i * 32 * G128_PITCH + ksub * 16]);
                    if (WF != WF_BF16) al[i] = *reinterpret_cast<const bf16x8*>(&sm[buf][NT - 1][fa + i * 32 * G128_PITCH + ksub * 16]);
                    bh[i] = *reinterpret_cast<const bf16x8*>(&sm[buf][1][fb + i * 32 * G128_PITCH + ksub * 16]);
                    bl[i] = *reinterpret_cast<const bf16x8*>(&sm[buf][2][fb + i * 32 * G128_PITCH + ksub * 16]);
                }
#pragma unroll
                for (int i = 0; i < 2; ++i)
#pragma unroll
                    for (int j = 0; j < 2; ++j) {
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[i], bh[j], acc[i][j], 0, 0, 0);
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[i], bl[j], acc[i][j], 0, 0, 0);
                        if (WF != WF_BF16) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al[i], bh[j], acc[i][j], 0, 0, 0);
                    }
            }
            if (nseq > 1 && (s + 1) % spf == 0) {   // end of a slice: fold it into the running total (0 + p0, then + p1, ...)
#pragma unroll
                for (int i = 0; i < 2; ++i)
#pragma unroll
                    for (int j = 0; j < 2; ++j)
#pragma unroll
                        for (int r = 0; r < 16; ++r) {
                            tot[i][j][r] = tot[i][j][r] + acc[i][j][r];
                            acc[i][j][r] = 0.0f;
                        }
            }
            if (s + 1 < nstage) swrite(buf ^ 1, (d + 1) % DW, (d + 1) % DX);
            __syncthreads();
        }
    }
    if (nseq > 1) {
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j) acc[i][j] = tot[i][j];
    }
    // epilogue.  C layout: token = lane & 31, row = (r & 3) + 8 * (r >> 2) + 4 * half inside a 32 x 32 tile
    const int Mv = stt->m;
    const int nsplit = gridDim.y;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int tok = tb + wc * 64 + j * 32 + (lane & 31);
        if (EPI == GEMM_EPI_LOGITS) {   // y = the block's scratch [128][ldy], rope.row_base = first token of the block inside the pass
            if (rope.row_base + tok >= Mv) continue;
            float* yr = y + (long)tok * ldy;
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int q = 0; q < 4; ++q) {   // registers 4 q .. 4 q + 3 are four consecutive rows
                    const int n = n0 + wr * 64 + i * 32 + 8 * q + 4 * half;
                    if (n + 3 < N && (ldy & 3) == 0) {
                        *reinterpret_cast<float4*>(yr + n) = make_float4(acc[i][j][4 * q], acc[i][j][4 * q + 1], acc[i][j][4 * q + 2], acc[i][j][4 * q + 3]);
                    } else {
#pragma unroll
                        for (int e = 0; e < 4; ++e)
                            if (n + e < N) yr[n + e] = acc[i][j][4 * q + e];
                    }
                }
            continue;
        }
        if (tok >= Mv) continue;
        if (nsplit > 1) {   // partial sums of this k slice, token-contiguous [split][n][LM_MAXM]: lanes are tokens -> 128-byte runs
            float* p = part + ((long)blockIdx.y * N + n0 + wr * 64) * LM_MAXM + tok;
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int r = 0; r < 16; ++r) p[(long)(i * 32 + (r & 3) + 8 * (r >> 2) + 4 * half) * LM_MAXM] = acc[i][j][r];
        } else if (EPI == GEMM_EPI_RESID) {
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int n = n0 + wr * 64 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
                    y[(long)tok * ldy + n] = y[(long)tok * ldy + n] + acc[i][j][r];
                }
        } else if (ROPE) {
            // the wave's 64 rows are one head: rows d (tile 0) and d + 32 (tile 1) sit in the same register slot
            if (EPI == GEMM_EPI_ROPE_ROWS) {   // this token row's session: its position, its cache (the arithmetic below is shared)
                const LmGroupRow gr = grp.rows[tok];
                rope.kc = gr.kc + (long)grp.layer * gr.kv_stride;
                rope.vc = gr.vc + (long)grp.layer * gr.kv_stride;
                rope.n_ctx = gr.n_ctx;
                rope.pos_mask = gr.pos_mask;
            }
            const int pos = EPI == GEMM_EPI_ROPE_ROWS ? grp.rows[tok].stt->n_tokens + grp.rows[tok].j : stt->n_tokens + tok;
            if (pos >= rope.n_ctx) continue;
            const int head = (n0 + wr * 64 + rope.row_base) >> 6;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int d = (r & 3) + 8 * (r >> 2) + 4 * half;   // < 32
                const float x1 = acc[0][j][r], x2 = acc[1][j][r];
                if (head < rope.nh + rope.nkv) {
                    const float c = rope.cos_t[(long)pos * 32 + d], sn = rope.sin_t[(long)pos * 32 + d];
                    const float o1 = x1 * c + (-x2) * sn;
                    const float o2 = x2 * c + x1 * sn;
                    if (head < rope.nh) {
                        y[(long)tok * ldy + head * 64 + d] = o1;
                        y[(long)tok * ldy + head * 64 + d + 32] = o2;
                    } else {
                        f16_t* kp = rope.kc + ((long)(pos & rope.pos_mask) * rope.nkv + (head - rope.nh)) * 64;
                        kp[d] = (f16_t)o1;
                        kp[d + 32] = (f16_t)o2;
                    }
                } else {
                    f16_t* vp = rope.vc + ((long)(pos & rope.pos_mask) * rope.nkv + (head - rope.nh - rope.nkv)) * 64;
                    vp[d] = (f16_t)x1;
                    vp[d + 32] = (f16_t)x2;
                }
            }
        } else {   // SwiGLU: rows (2i, 2i+1) = (gate_i, up_i) sit in registers (2q, 2q+1)
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int q = 0; q < 8; ++q) {
                    const int rr = ((2 * q) & 3) + 8 * ((2 * q) >> 2) + 4 * half;
                    const int fi = (n0 + wr * 64 + i * 32 + rr) >> 1;
                    const float g = acc[i][j][2 * q], u = acc[i][j][2 * q + 1];
                    const float hv = (g / (1.0f + __expf(-g))) * u;
                    const bf16_t hb = f32_to_bf16_rne(hv);
                    oh[(long)tok * ldy + fi] = hb;
                    ol[(long)tok * ldy + fi] = f32_to_bf16_rne(hv - __uint_as_float((unsigned)hb << 16));
                }
        }
    }
}
// Epilogue over the k-split partial sums part[split][n][LM_MAXM] (added in split order, starting from 0).  A block
// takes 64 rows x 32 tokens: it sums the splits with token-contiguous reads, turns the tile through LDS and runs the
// fused epilogue with row-contiguous writes -- residual add, RoPE + KV write (the 64 rows are one head), or SwiGLU +
// hi/lo split (the 64 rows are 32 interleaved gate/up pairs).
template <int EPI>
__global__ __launch_bounds__(256) void lm_gemm128_epilogue_kernel(const LmDevState* __restrict__ stt, const float* __restrict__ part, int nsplit, int grp, int N,
                                                                  float* __restrict__ y, int ldy, bf16_t* __restrict__ oh, bf16_t* __restrict__ ol,
                                                                  GemvRope rope, GemvGroup rt) {
    __shared__ float tile[64][33];
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;   // ty 0..7
    const int n0 = blockIdx.x * 64, t0 = blockIdx.y * 32;
    const int Mv = stt->m;
    if (t0 >= Mv) return;
    {
        float v[8];
#pragma unroll
        for (int rr = 0; rr < 8; ++rr) v[rr] = 0.0f;
        const float* p0 = part + ((long)n0 + ty) * LM_MAXM + t0 + tx;
        // The sum over the k slices is DEFINED in two levels: groups of `grp` consecutive slices are folded first (each from 0), the
        // group sums are folded in group order (from 0).  A pass stores either every slice (grp > 1 here) or the group sums its
        // workgroups folded themselves while walking `grp` slices (grp == 1 here: 0 + G == G) -- the same additions either way.
        for (int s0 = 0; s0 < nsplit; s0 += grp) {
            float g[8];
#pragma unroll
            for (int rr = 0; rr < 8; ++rr) g[rr] = 0.0f;
#pragma unroll 4
            for (int s = s0; s < s0 + grp; ++s) {   // eight independent row sums per thread: eight loads in flight per slice
                const float* ps = p0 + (long)s * N * LM_MAXM;
#pragma unroll
                for (int rr = 0; rr < 8; ++rr) g[rr] += ps[(long)rr * 8 * LM_MAXM];
            }
#pragma unroll
            for (int rr = 0; rr < 8; ++rr) v[rr] += g[rr];
        }
#pragma unroll
        for (int rr = 0; rr < 8; ++rr) tile[rr * 8 + ty][tx] = v[rr];
    }
    __syncthreads();
#pragma unroll
    for (int tt = 0; tt < 4; ++tt) {
        const int tl = tt * 8 + ty;
        const int tok = t0 + tl;
        if (tok >= Mv) continue;
        if (EPI == GEMM_EPI_RESID) {
            float* yr = y + (long)tok * ldy + n0;
            yr[tx] = yr[tx] + tile[tx][tl];
            yr[tx + 32] = yr[tx + 32] + tile[tx + 32][tl];
        } else if (EPI == GEMM_EPI_ROPE || EPI == GEMM_EPI_ROPE_ROWS) {
            if (EPI == GEMM_EPI_ROPE_ROWS) {   // this token row's session: its position, its cache (the arithmetic below is shared)
                const LmGroupRow gr = rt.rows[tok];
                rope.kc = gr.kc + (long)rt.layer * gr.kv_stride;
                rope.vc = gr.vc + (long)rt.layer * gr.kv_stride;
                rope.n_ctx = gr.n_ctx;
                rope.pos_mask = gr.pos_mask;
            }
            const int pos = EPI == GEMM_EPI_ROPE_ROWS ? rt.rows[tok].stt->n_tokens + rt.rows[tok].j : stt->n_tokens + tok;
            if (pos >= rope.n_ctx) continue;
            const int head = (n0 + rope.row_base) >> 6, d = tx;
            const float x1 = tile[d][tl], x2 = tile[d + 32][tl];
            if (head < rope.nh + rope.nkv) {
                const float c = rope.cos_t[(long)pos * 32 + d], sn = rope.sin_t[(long)pos * 32 + d];
                const float o1 = x1 * c + (-x2) * sn;
                const float o2 = x2 * c + x1 * sn;
                if (head < rope.nh) {
                    y[(long)tok * ldy + head * 64 + d] = o1;
                    y[(long)tok * ldy + head * 64 + d + 32] = o2;
                } else {
                    f16_t* kp = rope.kc + ((long)(pos & rope.pos_mask) * rope.nkv + (head - rope.nh)) * 64;
                    kp[d] = (f16_t)o1;
                    kp[d + 32] = (f16_t)o2;
                }
            } else {
                f16_t* vp = rope.vc + ((long)(pos & rope.pos_mask) * rope.nkv + (head - rope.nh - rope.nkv)) * 64;
                vp[d] = (f16_t)x1;
                vp[d + 32] = (f16_t)x2;
            }
        } else {   // rows (2i, 2i+1) = (gate_i, up_i)
            const int F = N >> 1;
            const int fi = (n0 >> 1) + tx;
            const float g = tile[2 * tx][tl], u = tile[2 * tx + 1][tl];
            const float hv = (g / (1.0f + __expf(-g))) * u;
            const bf16_t hb = f32_to_bf16_rne(hv);
            oh[(long)tok * F + fi] = hb;
            ol[(long)tok * F + fi] = f32_to_bf16_rne(hv - __uint_as_float((unsigned)hb << 16));
        }
    }
}

static bool lm_all_bf16(const rca_lm* h) {
    for (const LmLayer& L : h->layers)
        for (const WMat* m : {&L.qkv, &L.o, &L.gu, &L.down})
            if (m->fmt != WF_BF16 || L.split_v) return false;
    return true;
}
static bool lm_can_gemm128(const rca_lm* h);
// the 32-token tiles read bf16 fragments straight from HBM: bf16 models only; the 128-token tiles de-quantise any format while staging
static bool lm_can_mfma_prefill(const rca_lm* h) {
    const rca_lm_config_t& c = h->cfg;
    const int AO = c.n_heads * c.head_dim;
    if (lm_can_gemm128(h)) return true;
    return lm_all_bf16(h) && c.hidden % 64 == 0 && AO % 64 == 0 && c.ffn % 64 == 0 && (2 * c.ffn) % 32 == 0;
}
static int lm_enqueue_prefill_tile(rca_lm* h, int M, hipStream_t st, int nsp_launch) {
    const rca_lm_config_t& c = h->cfg;
    const int H = c.hidden, QKV = (c.n_heads + 2 * c.n_kv_heads) * c.head_dim, AO = c.n_heads * c.head_dim, F = c.ffn;
    GemvRope rope{h->cos_t, h->sin_t, nullptr, nullptr, c.n_heads, c.n_kv_heads, c.n_ctx, 0};
    float* x = h->x;
    lm_embed_kernel<<<M, 256, 0, st>>>(h->stt, h->embed, h->embed_f32, x, H, c.vocab_size);
    for (int l = 0; l < c.n_layers; ++l) {
        const LmLayer& L = h->layers[l];
        f16_t* kc = lm_kv_layer(h, h->kc, l);
        f16_t* vc = lm_kv_layer(h, h->vc, l);
        lm_rope_target(h, l, rope);
        lm_add_rmsnorm_kernel<<<M, 64, 0, st>>>(h->stt, x, nullptr, nullptr, 0, 0, L.attn_norm, h->xn, H, c.rms_eps);
        lm_split_bf16_kernel<<<dim3(cdiv(H, 256), M), 256, 0, st>>>(h->stt, h->xn, h->xh, h->xl, H);
        lm_gemm_mfma_kernel<GEMM_EPI_ROPE><<<QKV / 32, 256, 0, st>>>(h->stt, L.qkv.w, h->xh, h->xl, QKV, H, h->qkv, QKV, nullptr, nullptr, rope);
        lm_launch_kv_quant(h, l, M, st);
        launch_attention_mfma(h, M, nsp_launch, kc, vc, h->qkv, h->attn, st, nullptr, nullptr, true);
        lm_split_bf16_kernel<<<dim3(cdiv(AO, 256), M), 256, 0, st>>>(h->stt, h->attn, h->xh, h->xl, AO);
        lm_gemm_mfma_kernel<GEMM_EPI_RESID><<<H / 32, 256, 0, st>>>(h->stt, L.o.w, h->xh, h->xl, H, AO, x, H, nullptr, nullptr, norope);
        lm_add_rmsnorm_kernel<<<M, 64, 0, st>>>(h->stt, x, nullptr, nullptr, 0, 0, L.ffn_norm, h->xn, H, c.rms_eps);
        lm_split_bf16_kernel<<<dim3(cdiv(H, 256), M), 256, 0, st>>>(h->stt, h->xn, h->xh, h->xl, H);
        // SwiGLU epilogue writes the hi/lo split of h straight into the (ffn-wide) split buffers of the down projection:
        // it reads xh/xl [M][H] and writes [M][F] -- distinct regions are needed, so h goes to the second half of hbuf
        bf16_t* hh = reinterpret_cast<bf16_t*>(h->hbuf);
        bf16_t* hl = hh + (long)LM_MAXM * F;
        lm_gemm_mfma_kernel<GEMM_EPI_SWIGLU><<<2 * F / 32, 256, 0, st>>>(h->stt, L.gu.w, h->xh, h->xl, 2 * F, H, nullptr, F, hh, hl, norope);
        lm_gemm_mfma_kernel<GEMM_EPI_RESID><<<H / 32, 256, 0, st>>>(h->stt, L.down.w, hh, hl, H, F, x, H, nullptr, nullptr, norope);
    }
    RCA_LAUNCH_CHECK();
    return RCA_OK;
}
// Every 128-row GEMM is cut along k until ~512 workgroups per token block are in flight (a workgroup's stage is one exposed
// HBM round trip: parallel slices are what hides it), slices of >= 256 k, powers of two so they divide K / 32.  The count
// depends on the matrix only -- never on the tokens of the pass -- so any tiling of a prompt adds the same partial sums.
static int g128_splits(int N, int K) {
    int ns = 1;
    while (ns * (N / 128) < 512 && K % (ns * 2 * 32) == 0 && K / (ns * 2) >= 256) ns *= 2;
    return ns;
}
// Two-level definition of the sum over the ns slices (lm_gemm128_epilogue_kernel): at most four groups, folded first.  A function of the
// matrix only, like ns.  It lets a LONG pass store four group sums per output instead of ns partial sums (the narrow projections wrote
// and re-read 0.9 GB of partials per layer and 1024-token pass: down had 32 slices) without changing a bit of what a short pass
// computes from all ns.
static int g128_group(int ns) { return ns / std::min(ns, 4); }
struct G128Form { int grid_y, nseq, ep_nsplit, ep_grp; };   // ep_nsplit == 0: the kernel's own (fused) epilogue
static G128Form g128_form(int N, int ns, int tbz, int seq_min) {
    const int grp = g128_group(ns), ng = ns / grp;
    if (ns == 1) return {1, 1, 0, 1};
    if (grp == 1 && seq_min > 0 && (N / 128) * tbz >= seq_min) return {1, ns, 0, 1};            // every workgroup walks all slices (gate/up)
    if (grp > 1 && seq_min > 0 && (N / 128) * tbz * ng >= seq_min) return {ng, grp, ng, 1};     // workgroups walk a group, group sums stored
    return {ns, 1, ns, grp};                                                                     // every slice stored
}
static int g128_seq_min() {   // one value per process: every pass of a token block takes the same form
    static const int v = getenv("RCA_LM_SEQ_MIN_WGS") ? atoi(getenv("RCA_LM_SEQ_MIN_WGS")) : 512;
    return v;
}
static bool lm_can_gemm128(const rca_lm* h) {
    const rca_lm_config_t& c = h->cfg;
    const int H = c.hidden, QKV = (c.n_heads + 2 * c.n_kv_heads) * c.head_dim, AO = c.n_heads * c.head_dim, F = c.ffn;
    const int G = c.n_heads / c.n_kv_heads;
    for (const LmLayer& L : h->layers)   // a V projection kept apart from [q; k] (formats differ): both parts are tiled by 128 rows
        if (L.split_v && ((L.qkv.N % 128) || (L.vseg.N % 128))) return false;
    return c.head_dim == 64 && (G == 1 || G == 2 || G == 4) && H % 128 == 0 && QKV % 128 == 0 && (2 * F) % 128 == 0 && AO % 32 == 0 && F % 32 == 0;
}
// one 128-row GEMM launch in the format the matrix is kept in
template <int EPI>
static void launch_gemm128(rca_lm* h, const WMat& w, dim3 grid, hipStream_t st, const bf16_t* xh, const bf16_t* xl, int N, int K, int kslice,
                           float* y, int ldy, bf16_t* oh, bf16_t* ol, GemvRope rope, int nseq, const LmDevState* stt,
                           const GemvGroup& grp = nogroup) {   // stt: the pass's device state (the handle's own, or a batch step's)
    static bool attr_done = false;
    if (!attr_done) {   // the four-tile variants need 80 KB of LDS
        for (int fmt : WF_FORMATS)
            wf_dispatch(fmt, [](auto wf) {
                if constexpr (decltype(wf)::value != WF_BF16)
                    (void)hipFuncSetAttribute((const void*)lm_gemm128_kernel<EPI, decltype(wf)::value>, hipFuncAttributeMaxDynamicSharedMemorySize, G128_LDS_T(4));
            });
        attr_done = true;
    }
    const GemvQ8 qa{w.qs, w.sc, w.dd};
    wf_dispatch(w.fmt, [&](auto wf) {   // bf16 fragments go to the MFMA as they are: three tiles per stage, not four
        constexpr int WF = decltype(wf)::value;
        lm_gemm128_kernel<EPI, WF><<<grid, 256, WF == WF_BF16 ? G128_LDS_T(3) : G128_LDS_T(4), st>>>(stt, w.wptr(), qa, xh, xl, N, K, kslice, y, ldy, oh, ol,
                                                                                                 h->gpart, rope, nseq, grp);
    });
}
// What differs between the callers of the 128-token-tile layer sequence (lm_enqueue_layers128)
struct LmTilePass {
    rca_lm* h;                 // whose buffers and weights the pass uses
    const LmDevState* stt;     // the state the row-wise kernels and the GEMMs read: h->stt, or a batch's own (m = the rows that exist)
    int rows;                  // sizes the row-wise grids and the k-split epilogues' token groups
    int tbz;                   // token blocks of the pass: the GEMMs' grid.z, and what their k-split form is chosen for
    const LmGroupRow* qrows;   // null: the QKV epilogue is GEMM_EPI_ROPE into h's own cache (lm_rope_target, n_ctx bound); else
                               // GEMM_EPI_ROPE_ROWS, position, cache and bound per row from this table
    int seq_min;               // workgroup threshold of g128_form: g128_seq_min() for every pass (rca_lm_gemm128_tap: the test's own)
    double* imx = nullptr;     // a collecting pass (rca_lm_imatrix_chunk): the accumulator base of h; null for every other caller, whose
                               // launch sequence then is what it was
};
// The importance matrix's accumulators of a handle: per layer the vectors of kind 0 (width H: the input of attn_q / attn_k / attn_v),
// 1 (AO: attn_output), 2 (H: ffn_gate / ffn_up), 3 (F: ffn_down), and behind the layers kind 4 (H: output.weight; `layer` is ignored).
// Returns the offset of (layer, kind) and its width in *K; -1 for a layer or kind that does not exist.
static long lm_imx_slot(const rca_lm_config_t& c, int layer, int kind, int* K) {
    const long H = c.hidden, AO = (long)c.n_heads * c.head_dim, F = c.ffn, per_layer = H + AO + H + F;
    if (kind == 4) { *K = (int)H; return per_layer * c.n_layers; }
    if (kind < 0 || kind > 4 || layer < 0 || layer >= c.n_layers) return -1;
    const long off[4] = {0, H, H + AO, H + AO + H};
    *K = (int)(kind == 1 ? AO : kind == 3 ? F : H);
    return per_layer * layer + off[kind];
}
static void lm_launch_imatrix(const bf16_t* xh, const bf16_t* xl, int K, int m, double* acc, hipStream_t st);
// Behind a launch of a collecting pass that wrote a projection's input planes xh / xl (row stride = the projection's K; the pass's
// p.rows rows are all live): their column sums into the slot of (l, kind); rca_lm_imatrix_chunk_tap's copy of the planes follows it.
static void lm_collect_planes(const LmTilePass& p, hipStream_t st, int l, int kind, const bf16_t* xh, const bf16_t* xl) {
    if (!p.imx) return;
    int K = 0;
    const long off = lm_imx_slot(p.h->cfg, l, kind, &K);
    lm_launch_imatrix(xh, xl, K, p.rows, p.imx + off, st);
    if (p.h->imx_tap_kind == kind && (kind == 4 || p.h->imx_tap_layer == l)) {
        (void)hipMemcpyAsync(p.h->imx_tap_h, xh, (size_t)p.rows * K * 2, hipMemcpyDeviceToDevice, st);
        (void)hipMemcpyAsync(p.h->imx_tap_l, xl, (size_t)p.rows * K * 2, hipMemcpyDeviceToDevice, st);
    }
}
// One projection of such a pass: the GEMM and, where its k slices went through HBM, the epilogue that sums them.  A projection whose
// token blocks alone put `seq_min` workgroups on the chip is run with every workgroup walking the k slices itself (same sums in the
// same order, no partial sums through HBM, no epilogue launch); RCA_LM_SEQ_MIN_WGS overrides the threshold (0 = never) for A/B runs.
template <int EPI>
static G128Form lm_launch_proj128(const LmTilePass& p, const WMat& w, hipStream_t st, const bf16_t* xh, const bf16_t* xl, int N, int K, float* y, int ldy,
                              bf16_t* oh, bf16_t* ol, const GemvRope& rope = norope, const GemvGroup& grp = nogroup) {
    const int ns = g128_splits(N, K);
    const G128Form f = g128_form(N, ns, p.tbz, p.seq_min);
    launch_gemm128<EPI>(p.h, w, dim3(N / 128, f.grid_y, p.tbz), st, xh, xl, N, K, K / ns, y, ldy, oh, ol, rope, f.nseq, p.stt, grp);
    if (f.ep_nsplit)   // (the SwiGLU epilogue has no y and is handed ldy 0, its GEMM the width of the planes)
        lm_gemm128_epilogue_kernel<EPI><<<dim3(N / 64, cdiv(p.rows, 32)), 256, 0, st>>>(p.stt, p.h->gpart, f.ep_nsplit, f.ep_grp, N, y, EPI == GEMM_EPI_SWIGLU ? 0 : ldy,
                                                                                         oh, ol, rope, grp);
    return f;   // (the form that ran: rca_lm_gemm128_tap reports it)
}
// The layers of a pass on the 128-token tiles, behind the caller's embedding launch and in front of its heads: every route that runs
// these tiles -- a handle's own pass, a pass of rca_lm_batch_eval, the batch step / frame / selection / duplex pass -- runs this one
// sequence, so a row's bits cannot depend on the route.  attention(l): the caller's q8_0 quantiser and attention launches of layer l,
// reading h->qkv and writing the hi / lo planes h->xh / h->xl (a template argument: a tile is ~230 eager launches).
template <class Attn>
static void lm_enqueue_layers128(const LmTilePass& p, hipStream_t st, Attn&& attention) {
    rca_lm* h = p.h;
    const rca_lm_config_t& c = h->cfg;
    const int H = c.hidden, QKV = (c.n_heads + 2 * c.n_kv_heads) * c.head_dim, AO = c.n_heads * c.head_dim, F = c.ffn;
    GemvRope rope{h->cos_t, h->sin_t, nullptr, nullptr, c.n_heads, c.n_kv_heads, p.qrows ? 0 : c.n_ctx, 0};
    float* x = h->x;
    // SwiGLU epilogue writes the hi/lo split of h straight into the (ffn-wide) split buffers of the down projection:
    // it reads xh/xl [M][H] and writes [M][F] -- distinct regions are needed, so h goes to the second half of hbuf
    bf16_t* hh = reinterpret_cast<bf16_t*>(h->hbuf);
    bf16_t* hl = hh + (long)LM_MAXM * F;
    for (int l = 0; l < c.n_layers; ++l) {
        const LmLayer& L = h->layers[l];
        const GemvGroup grp = p.qrows ? GemvGroup{p.qrows, l} : nogroup;
        if (!p.qrows) lm_rope_target(h, l, rope);
        lm_add_rmsnorm_kernel<<<p.rows, 64, 0, st>>>(p.stt, x, nullptr, nullptr, 0, 0, L.attn_norm, h->xn, H, c.rms_eps, h->xh, h->xl);
        lm_collect_planes(p, st, l, 0, h->xh, h->xl);
        for (int seg = 0; seg < (L.split_v ? 2 : 1); ++seg) {   // [q; k; v] as one matrix, or [q; k] and v when their formats differ
            const WMat& w = seg ? L.vseg : L.qkv;
            rope.row_base = seg ? L.qkv.N : 0;
            if (p.qrows) lm_launch_proj128<GEMM_EPI_ROPE_ROWS>(p, w, st, h->xh, h->xl, w.N, H, h->qkv, QKV, nullptr, nullptr, rope, grp);
            else lm_launch_proj128<GEMM_EPI_ROPE>(p, w, st, h->xh, h->xl, w.N, H, h->qkv, QKV, nullptr, nullptr, rope, grp);
        }
        attention(l);
        lm_collect_planes(p, st, l, 1, h->xh, h->xl);
        lm_launch_proj128<GEMM_EPI_RESID>(p, L.o, st, h->xh, h->xl, H, AO, x, H, nullptr, nullptr);
        lm_add_rmsnorm_kernel<<<p.rows, 64, 0, st>>>(p.stt, x, nullptr, nullptr, 0, 0, L.ffn_norm, h->xn, H, c.rms_eps, h->xh, h->xl);
        lm_collect_planes(p, st, l, 2, h->xh, h->xl);
        lm_launch_proj128<GEMM_EPI_SWIGLU>(p, L.gu, st, h->xh, h->xl, 2 * F, H, nullptr, F, hh, hl);
        lm_collect_planes(p, st, l, 3, hh, hl);
        lm_launch_proj128<GEMM_EPI_RESID>(p, L.down, st, hh, hl, H, F, x, H, nullptr, nullptr);
    }
}
// The logits head on the tiles (GEMM_EPI_LOGITS): the 128 normalised rows whose hi / lo planes start at xh / xl -> blk [128][V]; they
// are rows row_base .. of the pass stt describes.  Every workgroup walks all of K itself (one slice: no partial sums).
static void lm_launch_logits128(rca_lm* h, const LmDevState* stt, const bf16_t* xh, const bf16_t* xl, int row_base, float* blk, hipStream_t st) {
    const rca_lm_config_t& c = h->cfg;
    GemvRope rp = norope;
    rp.row_base = row_base;
    launch_gemm128<GEMM_EPI_LOGITS>(h, h->head, dim3(cdiv(c.vocab_size, 128), 1, 1), st, xh, xl, c.vocab_size, c.hidden, c.hidden, blk, c.vocab_size, nullptr, nullptr, rp, 1, stt);
}
// A handle's own pass of M tokens.  bt (rca_lm_batch_eval): the rows are segments of several sessions packed into h's buffers (h is the
// call's workspace, h->stt the pass's state; M is the pass's whole token blocks, the launch geometry, and h->stt->m the rows that
// exist); what is per session -- the QKV epilogue's position and cache, the q8_0 quantiser, attention -- takes it from the pass's tables.
// imx (rca_lm_imatrix_chunk alone; M = m, no bt): the pass collects into these accumulators.
static int lm_enqueue_prefill_tile128(rca_lm* h, int M, hipStream_t st, int nsp_launch, const LmEvalTables* bt = nullptr, double* imx = nullptr) {
    const rca_lm_config_t& c = h->cfg;
    const LmTilePass p{h, h->stt, M, (int)cdiv(M, 128), bt ? bt->rows : nullptr, g128_seq_min(), imx};
    lm_embed_kernel<<<M, 256, 0, st>>>(h->stt, h->embed, h->embed_f32, h->x, c.hidden, c.vocab_size);
    if (bt)
        lm_enqueue_layers128(p, st, [&](int l) {
            if (bt->q8)   // every segment's new rows, ring -> int8 planes, in one launch
                lm_kv_quant_rows_kernel<<<dim3(cdiv(4 * c.n_kv_heads, 8), M), 256, 0, st>>>(h->stt, bt->tab, bt->owner, l, c.n_kv_heads);
            launch_attention_flash_tab(h, M, st, h->xh, h->xl, *bt, l);
        });
    else
        lm_enqueue_layers128(p, st, [&](int l) {
            lm_launch_kv_quant(h, l, M, st);
            launch_attention_mfma(h, M, nsp_launch, lm_kv_layer(h, h->kc, l), lm_kv_layer(h, h->vc, l), h->qkv, h->attn, st, h->xh, h->xl, true);
        });
    RCA_LAUNCH_CHECK();
    return RCA_OK;
}

// The route of an eval of more than LM_PREFILL_MIN tokens (and of every rca_lm_eval_async piece) with the handle's current settings:
// the one place that decides it -- lm_eval_impl branches on it and rca_lm_prefill_route reports it to the tests.
enum { LM_ROUTE_GEMV = 0, LM_ROUTE_TILE32 = 1, LM_ROUTE_TILE128 = 2 };
static int lm_prefill_route(const rca_lm* h) {
    if (h->cfg.logits_all != 0 || !h->mfma_prefill || !lm_can_mfma_prefill(h)) return LM_ROUTE_GEMV;
    return lm_can_gemm128(h) ? LM_ROUTE_TILE128 : LM_ROUTE_TILE32;
}

// an rca_lm_eval_async pass may still own the pinned staging block and the activations: wait for it before anything else runs
static int lm_settle(rca_lm* h) {
    { const int rc = lm_wait_batch_eval(h); if (rc != RCA_OK) return rc; }
    if (h->async_pending) {
        RCA_HIP(hipSetDevice(h->device));
        RCA_HIP(hipStreamSynchronize(h->stream));
        h->async_pending = false;
    }
    return RCA_OK;
}
// The next pass as the device will read it, into the pinned staging block: KV position, m and the m ids.  The copy to the device is
// the caller's (a captured graph's first node, or lm_push_state); the rng counter / out_token stay device-owned.
static void lm_stage_state(rca_lm* h, const int32_t* ids, int m) {
    h->h_stt->n_tokens = h->n_tokens;
    h->h_stt->m = m;
    for (int i = 0; i < m; ++i) h->h_stt->ids[i] = ids[i];
}
static size_t lm_state_bytes(int m) { return 8 + 4 * (size_t)std::max(m, 16); }   // n_tokens, m and the m ids only
static int lm_push_state(rca_lm* h, const int32_t* ids, int m, hipStream_t st) {
    lm_stage_state(h, ids, m);
    RCA_HIP(hipMemcpyAsync(h->stt, h->h_stt, lm_state_bytes(m), hipMemcpyHostToDevice, st));
    return RCA_OK;
}

// Context buckets of the captured decode graphs: bucket b launches min(n_splits, 4 << b) attention splits, the last bucket all of
// them.  A call of m tokens takes the first bucket that covers the splits it needs (cap_bucket >= 0, rca_duplex_precapture: that one).
struct LmBucket { int bucket, nsp_launch; };
static LmBucket lm_bucket(const rca_lm* h, int m, int cap_bucket) {
    const int need = lm_splits_needed(h, m);
    int b = 0;
    while (b + 1 < LM_GRAPH_BUCKETS && (4 << b) < need) ++b;
    if (cap_bucket >= 0) b = cap_bucket;
    return {b, b + 1 == LM_GRAPH_BUCKETS ? h->n_splits : std::min(h->n_splits, 4 << b)};
}
// the rule above can choose bucket b on this handle: the bucket before it does not launch every split yet
static bool lm_bucket_reachable(const rca_lm* h, int b) { return b == 0 || (4 << (b - 1)) < h->n_splits; }

extern "C" int rca_lm_reset(rca_lm_t* h) {
    if (!h) return fail(RCA_ERR_ARG, "null");
    h->n_tokens = 0;
    h->logits_rows = 0;
    return RCA_OK;
}
extern "C" int rca_lm_get_n_tokens(const rca_lm_t* h, int32_t* n) {
    if (!h || !n) return fail(RCA_ERR_ARG, "null");
    *n = h->n_tokens;
    return RCA_OK;
}
extern "C" int rca_lm_set_n_tokens(rca_lm_t* h, int32_t n) {
    if (!h) return fail(RCA_ERR_ARG, "null");
    if (n < 0 || n > h->cfg.n_ctx) return fail(RCA_ERR_ARG, "n_tokens %d outside [0, %d]", n, h->cfg.n_ctx);
    h->n_tokens = n;
    return RCA_OK;
}
extern "C" int rca_lm_sync(rca_lm_t* h) {
    if (!h) return fail(RCA_ERR_ARG, "null");
    RCA_HIP(hipSetDevice(h->device));
    RCA_HIP(hipStreamSynchronize(h->stream));
    h->async_pending = false;
    { const int rc = lm_wait_batch_eval(h); if (rc != RCA_OK) return rc; }
    return RCA_OK;
}

// as_prefill: use the prefill tiles even for n <= LM_PREFILL_MIN (pieces of one long eval).
// wait_last = false: return as soon as the LAST pass / tile is enqueued (everything before it has completed, because the
// pinned staging block is reused per pass); the next call on the handle waits for it first.
static int lm_eval_impl(rca_lm_t* h, const int32_t* ids, int32_t n, bool wait_last, bool as_prefill) {
    if (!h || (!ids && n > 0) || n < 0) return fail(RCA_ERR_ARG, "eval: bad argument");
    if (n == 0) return RCA_OK;
    if (h->n_tokens + n > h->cfg.n_ctx) return fail(RCA_ERR_STATE, "context overflow: %d + %d > n_ctx %d", h->n_tokens, n, h->cfg.n_ctx);
    for (int i = 0; i < n; ++i)
        if (ids[i] < 0 || ids[i] >= h->cfg.vocab_size) return fail(RCA_ERR_ARG, "eval: token id %d at index %d is outside the vocabulary [0, %d)", ids[i], i, h->cfg.vocab_size);
    RCA_HIP(hipSetDevice(h->device));
    hipStream_t st = h->stream;
    int rc;
    if (h->async_pending) { RCA_HIP(hipStreamSynchronize(st)); h->async_pending = false; }
    if ((rc = lm_wait_batch_eval(h)) != RCA_OK) return rc;
    const bool all = h->cfg.logits_all != 0;
    if (all && n > h->logits_rows_cap) {
        RCA_HIP(hipStreamSynchronize(st));
        lm_drop_graphs(h);   // their head-GEMV and sampler nodes point at the buffer that is about to be freed
        (void)hipFree(h->logits);
        h->logits = nullptr;
        h->logits_rows_cap = n;
        if ((rc = lm_alloc((void**)&h->logits, (size_t)n * h->cfg.vocab_size * 4)) != RCA_OK) return rc;
    }
    float* logits_base = h->logits;
    const int route = lm_prefill_route(h);
    if ((n > LM_PREFILL_MIN || as_prefill) && route != LM_ROUTE_GEMV) {
        // long evals (session prefill, recompute_kv_cache): 32-token tiles on the bf16 MFMA path
        const bool big = route == LM_ROUTE_TILE128;
        const int tile = big ? LM_MAXM : LM_TILE32;
        // A background tile (rca_lm_eval_async of one pass: kv_shadow.py feeds one per few frames) is ~230 launches; issued eagerly
        // they cost the calling frame ~2 ms of host time before its own replay is even launched (tile frames 9.5 ms against a median
        // of 4.4).  The second pass of a size on this cache is captured and replayed from then on: one launch.  (First: eager --
        // the launchers' one-time attribute calls; the geometry of a pass depends on its token count only, the context is read
        // from the device state.)
        const bool tile_graphs = lm_env_tile_graphs() && lm_env_flash();   // (the split-attention A/B path launches per context)
        if (!wait_last && big && n <= tile && h->graphs_enabled && tile_graphs) {
            rca_lm::GraphSet& gs = lm_graph_set(h);
            int slot = -1;
            for (int i = 0; i < 2; ++i)
                if (gs.tile_m[i] == n) slot = i;
            if (slot < 0) {
                slot = gs.tile_seen[0] <= gs.tile_seen[1] ? 0 : 1;
                if (gs.tile_g[slot]) { (void)hipGraphExecDestroy(gs.tile_g[slot]); gs.tile_g[slot] = nullptr; }
                gs.tile_m[slot] = n; gs.tile_seen[slot] = 0;
            }
            if (++gs.tile_seen[slot] >= 2) {
                lm_stage_state(h, ids, n);
                if (!gs.tile_g[slot]) {
                    rc = lm_capture(st, &gs.tile_g[slot], "tile", [&]() -> int {
                        hipError_t e = hipMemcpyAsync(h->stt, h->h_stt, lm_state_bytes(n), hipMemcpyHostToDevice, st);
                        if (e != hipSuccess) return fail(RCA_ERR_HIP, "tile capture memcpy: %s", hipGetErrorString(e));
                        const int r = lm_enqueue_prefill_tile128(h, n, st, 1);
                        if (r == RCA_OK) lm_launch_head(h, 1, st, h->logits, true);
                        return r;
                    });
                    if (rc != RCA_OK) return rc;
                }
                RCA_HIP(hipGraphLaunch(gs.tile_g[slot], st));
                h->n_tokens += n;
                h->logits_rows = 1;
                h->async_pending = true;
                return RCA_OK;
            }
        }
        for (int off = 0; off < n; off += tile) {
            const int m = std::min(tile, n - off);
            const bool last = off + m >= n;
            if ((rc = lm_push_state(h, ids + off, m, st)) != RCA_OK) return rc;
            rc = big ? lm_enqueue_prefill_tile128(h, m, st, lm_splits_needed(h, m)) : lm_enqueue_prefill_tile(h, m, st, lm_splits_needed(h, m));
            if (rc != RCA_OK) return rc;
            if (last) {   // logits of the final token: final norm + head on the register GEMV path
                lm_launch_head(h, 1, st, h->logits, true);
                RCA_LAUNCH_CHECK();
            }
            h->n_tokens += m;
            if (!last) RCA_HIP(hipStreamSynchronize(st));
        }
    } else {
        for (int off = 0; off < n; off += LM_GEMV_M) {
            const int m = std::min(LM_GEMV_M, n - off);
            const bool last = off + m >= n;
            if ((rc = lm_push_state(h, ids + off, m, st)) != RCA_OK) return rc;
            if (all) h->logits = logits_base + (long)off * h->cfg.vocab_size;
            rc = lm_enqueue_pass(h, m, all ? 2 : (last ? 1 : 0), st, lm_splits_needed(h, m));
            h->logits = logits_base;
            if (rc != RCA_OK) return rc;
            h->n_tokens += m;
            // the pinned staging block is reused by the next chunk: wait until this one's copy has been consumed
            if (!last) RCA_HIP(hipStreamSynchronize(st));
        }
    }
    h->logits_rows = all ? n : 1;
    if (wait_last) RCA_HIP(hipStreamSynchronize(st));
    else h->async_pending = true;
    return RCA_OK;
}
extern "C" int rca_lm_eval(rca_lm_t* h, const int32_t* ids, int32_t n) { return lm_eval_impl(h, ids, n, true, false); }
// Asynchronous, and with the arithmetic of a LONG eval whatever n is: a cache built piecewise with this call holds the same bits
// as one rca_lm_eval of the whole sequence (short evals otherwise run as decode passes, which round differently from the tiles).
extern "C" int rca_lm_eval_async(rca_lm_t* h, const int32_t* ids, int32_t n) { return lm_eval_impl(h, ids, n, false, true); }

// ---- KV-cache plumbing between a handle and its weight-sharing twin (the shadow cache of the sliding-window trim)
static int lm_same_cache_shape(const rca_lm* a, const rca_lm* b) {
    return a->device == b->device && a->cfg.n_layers == b->cfg.n_layers && a->cfg.n_kv_heads == b->cfg.n_kv_heads &&
           a->cfg.head_dim == b->cfg.head_dim && a->n_ctx_pad == b->n_ctx_pad && a->cfg.n_ctx == b->cfg.n_ctx;
}
extern "C" int rca_lm_copy_kv(rca_lm_t* dst, rca_lm_t* src, int32_t n_pos) {
    if (!dst || !src || dst == src) return fail(RCA_ERR_ARG, "copy_kv: two different handles needed");
    if (!lm_same_cache_shape(dst, src)) return fail(RCA_ERR_ARG, "copy_kv: the two KV caches differ in shape");
    if (dst->kv_format != src->kv_format) return fail(RCA_ERR_ARG, "copy_kv: the two KV caches differ in format (%d and %d, rca_lm_set_kv_format)", dst->kv_format, src->kv_format);
    if (n_pos < 0 || n_pos > src->cfg.n_ctx) return fail(RCA_ERR_ARG, "copy_kv: %d positions outside [0, %d]", n_pos, src->cfg.n_ctx);
    RCA_HIP(hipSetDevice(dst->device));
    RCA_HIP(hipStreamSynchronize(src->stream));   // everything src has evaluated so far is in its cache
    src->async_pending = false;
    { int rc; if ((rc = lm_wait_batch_eval(src)) != RCA_OK || (rc = lm_wait_batch_eval(dst)) != RCA_OK) return rc; }
    if (dst->async_pending) { RCA_HIP(hipStreamSynchronize(dst->stream)); dst->async_pending = false; }
    const size_t rows = (size_t)n_pos * src->cfg.n_kv_heads;   // head rows per layer: 128 bytes of fp16, or 64 int8 + two fp16 scales
    const size_t bytes = rows * (lm_kv_q8(src) ? 64 : 64 * sizeof(f16_t));
    for (int l = 0; l < src->cfg.n_layers && bytes; ++l) {
        RCA_HIP(hipMemcpyAsync(lm_kv_layer(dst, dst->kc, l), lm_kv_layer(src, src->kc, l), bytes, hipMemcpyDeviceToDevice, dst->stream));
        RCA_HIP(hipMemcpyAsync(lm_kv_layer(dst, dst->vc, l), lm_kv_layer(src, src->vc, l), bytes, hipMemcpyDeviceToDevice, dst->stream));
        if (lm_kv_q8(src)) {   // the scale planes, same position range
            RCA_HIP(hipMemcpyAsync(const_cast<f16_t*>(lm_kv_scales(dst, dst->kc, l)), lm_kv_scales(src, src->kc, l), rows * 2 * sizeof(f16_t), hipMemcpyDeviceToDevice, dst->stream));
            RCA_HIP(hipMemcpyAsync(const_cast<f16_t*>(lm_kv_scales(dst, dst->vc, l)), lm_kv_scales(src, src->vc, l), rows * 2 * sizeof(f16_t), hipMemcpyDeviceToDevice, dst->stream));
        }
    }
    dst->async_pending = true;
    return RCA_OK;
}
extern "C" int rca_lm_swap_kv(rca_lm_t* a, rca_lm_t* b) {
    if (!a || !b || a == b) return fail(RCA_ERR_ARG, "swap_kv: two different handles needed");
    if (!lm_same_cache_shape(a, b)) return fail(RCA_ERR_ARG, "swap_kv: the two KV caches differ in shape");
    if (a->kv_format != b->kv_format) return fail(RCA_ERR_ARG, "swap_kv: the two KV caches differ in format (%d and %d, rca_lm_set_kv_format)", a->kv_format, b->kv_format);
    RCA_HIP(hipSetDevice(a->device));
    RCA_HIP(hipStreamSynchronize(a->stream));
    RCA_HIP(hipStreamSynchronize(b->stream));
    a->async_pending = b->async_pending = false;
    { int rc; if ((rc = lm_wait_batch_eval(a)) != RCA_OK || (rc = lm_wait_batch_eval(b)) != RCA_OK) return rc; }
    std::swap(a->kc, b->kc);
    std::swap(a->vc, b->vc);
    a->graph_epoch++;   // the handles' own graph sets are keyed by the cache; a group's graphs over either handle are not
    b->graph_epoch++;
    return RCA_OK;
}

// ---- context shift (rca_lm_kv_remove): cache positions [p1, n) of every layer move down to [p0, n - delta), delta = p1 - p0, and
// their keys are rotated by -delta positions.  Source and destination rows overlap whenever delta < n - p1, so nothing moves in
// place: the rows travel in slabs of at most ATT_KEYS positions, in ascending order, through two staging slabs.  Launch i rotates
// source slab i into stage[i % 2] (unit kind A) and copies stage[(i - 1) % 2], which launch i - 1 filled, to destination slab
// i - 1 (kind B).  Destination slab i - 1 ends at p0 + ATT_KEYS * i, below the start p1 + ATT_KEYS * i of source slab i for any
// delta >= 1, and the two staging slabs are different buffers: inside one launch no byte is both read and written, whatever order
// the workgroups run in; between launches the stream orders.
// One unit = one thread = (layer, row of the slab, kv head, quarter q): elements q * 8 .. q * 8 + 7 and their RoPE partners
// q * 8 + 32 .. q * 8 + 39 (the pairing the QKV epilogues store) of the K row and the same 2 x 16 bytes of the V row.
// The body of one unit, shared by the single-handle kernel and the table form (rca_lm_kv_remove_many) so that a row's bits cannot
// differ between them.  stage_w == nullptr is the direct route of the table form: the rotated rows go straight to cache rows
// dst_pos + r (the host has shown that they are disjoint from every source row of the launch) and there are no kind-B units.
// The rotation of one RoPE pair (x1 at element j, x2 at element j + 32) by -delta positions, c / s = cos / sin of the table row
// `delta`: the inverse of the epilogues' x1 c - x2 s, x2 c + x1 s.  ONE helper for the fp16 unit and the q8_0 unit, its four products
// and two sums spelled as separate f32 operations that may not be contracted, so that the two instantiations round alike: a q8_0
// cache shifts to Q8 of what an fp16 cache holding its de-quantised rows shifts to, bit for bit.
static __device__ __forceinline__ void lm_kv_unrotate(const float x1, const float x2, const float c, const float s, float& o1, float& o2) {
#pragma clang fp contract(off)
    const float x1c = x1 * c, x2s = x2 * s, x2c = x2 * c, x1s = x1 * s;
    o1 = x1c + x2s;
    o2 = x2c - x1s;
}
static __device__ __forceinline__ void lm_kv_shift_unit(f16_t* kc, f16_t* vc, f16_t* stage_w, const f16_t* stage_r,
                                                        const float* cos_d, const float* sin_d, long layer_stride, int n_layers, int nkv,
                                                        int src_pos, int n_src, int dst_pos, int n_dst, long u, long ua) {
    const long stage_v = (long)n_layers * ATT_KEYS * nkv * 64;     // a staging slab holds its K rows first, its V rows stage_v elements later
    const bool rot = u < ua;
    long t = rot ? u : u - ua;
    const int npos = rot ? n_src : n_dst;
    const int q = (int)(t & 3);
    t >>= 2;
    const int kvh = (int)(t % nkv);
    t /= nkv;
    const int r = (int)(t % npos), l = (int)(t / npos);
    const long so = (((long)l * ATT_KEYS + r) * nkv + kvh) * 64 + q * 8;
    const long co = (long)l * layer_stride + ((long)((rot ? src_pos : dst_pos) + r) * nkv + kvh) * 64 + q * 8;
    if (rot) {
        const f16x8 k1 = *reinterpret_cast<const f16x8*>(kc + co), k2 = *reinterpret_cast<const f16x8*>(kc + co + 32);
        const u32x4 v1 = *reinterpret_cast<const u32x4*>(vc + co), v2 = *reinterpret_cast<const u32x4*>(vc + co + 32);
        float c[8], s[8];
        *reinterpret_cast<f32x4*>(c) = *reinterpret_cast<const f32x4*>(cos_d + q * 8);
        *reinterpret_cast<f32x4*>(c + 4) = *reinterpret_cast<const f32x4*>(cos_d + q * 8 + 4);
        *reinterpret_cast<f32x4*>(s) = *reinterpret_cast<const f32x4*>(sin_d + q * 8);
        *reinterpret_cast<f32x4*>(s + 4) = *reinterpret_cast<const f32x4*>(sin_d + q * 8 + 4);
        f16x8 o1, o2;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            float r1, r2;
            lm_kv_unrotate((float)k1[j], (float)k2[j], c[j], s[j], r1, r2);
            o1[j] = (f16_t)r1;                            // f32, then fp16 nearest-even
            o2[j] = (f16_t)r2;
        }
        const long cd = (long)l * layer_stride + ((long)(dst_pos + r) * nkv + kvh) * 64 + q * 8;
        f16_t* kw = stage_w ? stage_w + so : kc + cd;
        f16_t* vw = stage_w ? stage_w + stage_v + so : vc + cd;
        *reinterpret_cast<f16x8*>(kw) = o1;
        *reinterpret_cast<f16x8*>(kw + 32) = o2;
        *reinterpret_cast<u32x4*>(vw) = v1;
        *reinterpret_cast<u32x4*>(vw + 32) = v2;
    } else {
        const u32x4 k1 = *reinterpret_cast<const u32x4*>(stage_r + so), k2 = *reinterpret_cast<const u32x4*>(stage_r + so + 32);
        const u32x4 v1 = *reinterpret_cast<const u32x4*>(stage_r + stage_v + so), v2 = *reinterpret_cast<const u32x4*>(stage_r + stage_v + so + 32);
        *reinterpret_cast<u32x4*>(kc + co) = k1;
        *reinterpret_cast<u32x4*>(kc + co + 32) = k2;
        *reinterpret_cast<u32x4*>(vc + co) = v1;
        *reinterpret_cast<u32x4*>(vc + co + 32) = v2;
    }
}
__global__ __launch_bounds__(256) void lm_kv_shift_kernel(f16_t* kc, f16_t* vc, f16_t* __restrict__ stage_w, const f16_t* __restrict__ stage_r,
                                                          const float* __restrict__ cos_d, const float* __restrict__ sin_d,   // rows `delta` of the RoPE tables
                                                          long layer_stride, int n_layers, int nkv, int src_pos, int n_src, int dst_pos, int n_dst) {
    const long ua = (long)n_layers * n_src * nkv * 4, ub = (long)n_layers * n_dst * nkv * 4;
    for (long u = (long)blockIdx.x * 256 + threadIdx.x; u < ua + ub; u += (long)gridDim.x * 256)
        lm_kv_shift_unit(kc, vc, stage_w, stage_r, cos_d, sin_d, layer_stride, n_layers, nkv, src_pos, n_src, dst_pos, n_dst, u, ua);
}
// The table form: blockIdx.y picks a handle's row, and the row carries everything that differs between handles -- its cache, its
// staging slabs, the RoPE rows of ITS delta and the positions of this step.  A row whose tail has ended has n_src = n_dst = 0.
// The table travels by value in the kernel arguments (RCA_LM_KV_REMOVE_GROUP rows of 72 bytes): composed on the host, uploaded with
// the launch, and nothing of it outlives the launch.
struct LmShiftRow {
    f16_t *kc, *vc;
    f16_t* stage_w;            // nullptr: the direct route (rotated rows to cache rows dst_pos + r, n_dst = 0)
    const f16_t* stage_r;
    const float *cos_d, *sin_d;
    long layer_stride;
    int src_pos, n_src, dst_pos, n_dst;
};
struct LmShiftTable { LmShiftRow row[RCA_LM_KV_REMOVE_GROUP]; };
__global__ __launch_bounds__(256) void lm_kv_shift_many_kernel(const LmShiftTable tab, int n_layers, int nkv) {
    const LmShiftRow& w = tab.row[blockIdx.y];
    const long ua = (long)n_layers * w.n_src * nkv * 4, ub = (long)n_layers * w.n_dst * nkv * 4;
    for (long u = (long)blockIdx.x * 256 + threadIdx.x; u < ua + ub; u += (long)gridDim.x * 256)
        lm_kv_shift_unit(w.kc, w.vc, w.stage_w, w.stage_r, w.cos_d, w.sin_d, w.layer_stride, n_layers, nkv, w.src_pos, w.n_src, w.dst_pos, w.n_dst, u, ua);
}
// ---- the context shift of a q8_0 cache (opt-in: rca_lm_set_kv_shift_requant).  Host schedule, slabs, unit numbering and the proofs
// that a launch reads no byte it writes are those of the fp16 shift above -- they speak of cache POSITIONS, and a position's int8
// rows and scale pairs move together; only the unit body and the addressing differ.
//   V: the 64 int8 and the two fp16 scales of every moved head row, bit for bit.
//   K: x = fp16_rne((float)d16 * q), the row attention stages (kvq8_deq16's arithmetic); y = fp16_rne(lm_kv_unrotate(x)), the row an
//      fp16 cache holding x would hold after its own shift; new blocks = Q8(y) by lm_kv_quant_kernel's arithmetic, operation for
//      operation.  So "cache row == Q8(an fp16 row)" survives any number of shifts, and each shift costs the surviving keys one fp16
//      rounding (as on the fp16 cache) plus one q8_0 quantisation.  Non-finite x or y: whatever lm_kv_quant_kernel makes of such a row.
// Unit = thread = (layer, row of the slab, kv head, quarter q) as above: bytes q * 8 .. q * 8 + 7 of block 0 and of block 1 (8-byte
// loads and stores; lane-per-value, the quantiser's own mapping, would move single bytes), which are each other's RoPE partners, so a
// thread needs both scales of the head and no value of another thread.  The four threads of a head row are four neighbouring lanes
// with neighbouring unit numbers (unit counts are multiples of 4): they leave the loop together and take the same branch, and the
// block maxima are reduced over them with two shuffles of width 4.  V: 16 bytes per thread; thread 0 of a row moves the K scale pair,
// thread 1 the V scale pair.
// kc / vc: the tensor's allocation (int8 planes [L][n_ctx_pad][nkv][64], the scale planes [L][n_ctx_pad][nkv][2] n_layers * layer_stride
// bytes behind).  A staging slab holds finished blocks: K int8 [L][ATT_KEYS][nkv][64], V int8, K scale pairs, V scale pairs -- 136
// bytes per head row inside the 256 the fp16 slab has.
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
static __device__ __forceinline__ void lm_kv_shift_unit_q8(char* kc, char* vc, char* stage_w, const char* stage_r,
                                                           const float* cos_d, const float* sin_d, long layer_stride, int n_layers, int nkv,
                                                           int src_pos, int n_src, int dst_pos, int n_dst, long u, long ua) {
    const long srows = (long)n_layers * ATT_KEYS * nkv;          // head rows of a staging slab
    const long sc_off = (long)n_layers * layer_stride;           // bytes from the int8 planes to the scale planes
    const long s_vq = srows * 64, s_kd = srows * 128, s_vd = srows * 132;
    const bool rot = u < ua;
    long t = rot ? u : u - ua;
    const int npos = rot ? n_src : n_dst;
    const int q = (int)(t & 3);
    t >>= 2;
    const int kvh = (int)(t % nkv);
    t /= nkv;
    const int r = (int)(t % npos), l = (int)(t / npos);
    const long sr = ((long)l * ATT_KEYS + r) * nkv + kvh;                                                       // head row in a slab
    const long cr = (long)l * (layer_stride >> 6) + (long)((rot ? src_pos : dst_pos) + r) * nkv + kvh;          // head row in the cache
    if (rot) {
        const u32x2 a = *reinterpret_cast<const u32x2*>(kc + cr * 64 + q * 8), b = *reinterpret_cast<const u32x2*>(kc + cr * 64 + 32 + q * 8);
        const f16x2 kd = *reinterpret_cast<const f16x2*>(kc + sc_off + cr * 4);
        const u32x4 v = *reinterpret_cast<const u32x4*>(vc + cr * 64 + q * 16);
        const unsigned vd = *reinterpret_cast<const unsigned*>(vc + sc_off + cr * 4);
        float c[8], s[8];
        *reinterpret_cast<f32x4*>(c) = *reinterpret_cast<const f32x4*>(cos_d + q * 8);
        *reinterpret_cast<f32x4*>(c + 4) = *reinterpret_cast<const f32x4*>(cos_d + q * 8 + 4);
        *reinterpret_cast<f32x4*>(s) = *reinterpret_cast<const f32x4*>(sin_d + q * 8);
        *reinterpret_cast<f32x4*>(s + 4) = *reinterpret_cast<const f32x4*>(sin_d + q * 8 + 4);
        const float d0 = (float)kd[0], d1 = (float)kd[1];
        float y1[8], y2[8], am0 = 0.0f, am1 = 0.0f;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const float x1 = (float)(_Float16)((float)(int)(signed char)(a[j >> 2] >> (8 * (j & 3))) * d0);      // kvq8_deq16
            const float x2 = (float)(_Float16)((float)(int)(signed char)(b[j >> 2] >> (8 * (j & 3))) * d1);
            float r1, r2;
            lm_kv_unrotate(x1, x2, c[j], s[j], r1, r2);
            y1[j] = (float)(f16_t)r1;                                                                           // the fp16 row, widened as the quantiser reads it
            y2[j] = (float)(f16_t)r2;
            am0 = j ? fmaxf(am0, fabsf(y1[j])) : fabsf(y1[j]);
            am1 = j ? fmaxf(am1, fabsf(y2[j])) : fabsf(y2[j]);
        }
#pragma unroll
        for (int o = 2; o >= 1; o >>= 1) {
            am0 = fmaxf(am0, __shfl_xor(am0, o, 4));
            am1 = fmaxf(am1, __shfl_xor(am1, o, 4));
        }
        // lm_kv_quant_kernel's arithmetic per block
        const float e0 = am0 / 127.0f, e1 = am1 / 127.0f;
        const float inv0 = e0 != 0.0f ? 1.0f / e0 : 0.0f, inv1 = e1 != 0.0f ? 1.0f / e1 : 0.0f;
        u32x2 oa = {0u, 0u}, ob = {0u, 0u};
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            oa[j >> 2] |= (unsigned)(unsigned char)(signed char)(int)roundf(y1[j] * inv0) << (8 * (j & 3));
            ob[j >> 2] |= (unsigned)(unsigned char)(signed char)(int)roundf(y2[j] * inv1) << (8 * (j & 3));
        }
        f16x2 od;
        od[0] = (f16_t)e0;
        od[1] = (f16_t)e1;
        const long cd = (long)l * (layer_stride >> 6) + (long)(dst_pos + r) * nkv + kvh;
        char* kqw = stage_w ? stage_w + sr * 64 : kc + cd * 64;
        char* vqw = stage_w ? stage_w + s_vq + sr * 64 : vc + cd * 64;
        char* kdw = stage_w ? stage_w + s_kd + sr * 4 : kc + sc_off + cd * 4;
        char* vdw = stage_w ? stage_w + s_vd + sr * 4 : vc + sc_off + cd * 4;
        *reinterpret_cast<u32x2*>(kqw + q * 8) = oa;
        *reinterpret_cast<u32x2*>(kqw + 32 + q * 8) = ob;
        *reinterpret_cast<u32x4*>(vqw + q * 16) = v;
        if (q == 0) *reinterpret_cast<f16x2*>(kdw) = od;
        if (q == 1) *reinterpret_cast<unsigned*>(vdw) = vd;
    } else {
        const u32x2 a = *reinterpret_cast<const u32x2*>(stage_r + sr * 64 + q * 8), b = *reinterpret_cast<const u32x2*>(stage_r + sr * 64 + 32 + q * 8);
        const u32x4 v = *reinterpret_cast<const u32x4*>(stage_r + s_vq + sr * 64 + q * 16);
        *reinterpret_cast<u32x2*>(kc + cr * 64 + q * 8) = a;
        *reinterpret_cast<u32x2*>(kc + cr * 64 + 32 + q * 8) = b;
        *reinterpret_cast<u32x4*>(vc + cr * 64 + q * 16) = v;
        if (q == 0) *reinterpret_cast<unsigned*>(kc + sc_off + cr * 4) = *reinterpret_cast<const unsigned*>(stage_r + s_kd + sr * 4);
        if (q == 1) *reinterpret_cast<unsigned*>(vc + sc_off + cr * 4) = *reinterpret_cast<const unsigned*>(stage_r + s_vd + sr * 4);
    }
}
__global__ __launch_bounds__(256) void lm_kv_shift_q8_kernel(char* kc, char* vc, char* __restrict__ stage_w, const char* __restrict__ stage_r,
                                                             const float* __restrict__ cos_d, const float* __restrict__ sin_d,
                                                             long layer_stride, int n_layers, int nkv, int src_pos, int n_src, int dst_pos, int n_dst) {
    const long ua = (long)n_layers * n_src * nkv * 4, ub = (long)n_layers * n_dst * nkv * 4;
    for (long u = (long)blockIdx.x * 256 + threadIdx.x; u < ua + ub; u += (long)gridDim.x * 256)
        lm_kv_shift_unit_q8(kc, vc, stage_w, stage_r, cos_d, sin_d, layer_stride, n_layers, nkv, src_pos, n_src, dst_pos, n_dst, u, ua);
}
// the table form over q8_0 handles: LmShiftRow's pointers are the allocations of the q8_0 cache and of the staging slabs, taken as bytes
__global__ __launch_bounds__(256) void lm_kv_shift_many_q8_kernel(const LmShiftTable tab, int n_layers, int nkv) {
    const LmShiftRow& w = tab.row[blockIdx.y];
    const long ua = (long)n_layers * w.n_src * nkv * 4, ub = (long)n_layers * w.n_dst * nkv * 4;
    for (long u = (long)blockIdx.x * 256 + threadIdx.x; u < ua + ub; u += (long)gridDim.x * 256)
        lm_kv_shift_unit_q8(reinterpret_cast<char*>(w.kc), reinterpret_cast<char*>(w.vc), reinterpret_cast<char*>(w.stage_w), reinterpret_cast<const char*>(w.stage_r),
                            w.cos_d, w.sin_d, w.layer_stride, n_layers, nkv, w.src_pos, w.n_src, w.dst_pos, w.n_dst, u, ua);
}
extern "C" int rca_lm_kv_remove(rca_lm_t* h, int32_t p0, int32_t p1) {
    if (!h) return fail(RCA_ERR_ARG, "null");
    if (lm_kv_q8(h) && !h->kv_shift_requant)
        return fail(RCA_ERR_STATE, "kv_remove: this handle keeps a q8_0 KV cache (rca_lm_set_kv_format); re-rotating quantised keys would quantise them a second time, "
                                   "which this version does not do -- use an fp16 cache for the context shift");
    { const int rc = lm_settle(h); if (rc != RCA_OK) return rc; }
    const int n = h->n_tokens;
    if (p0 < 0 || p0 > p1 || p1 > n) return fail(RCA_ERR_ARG, "kv_remove: [%d, %d) is not a span of the %d cached positions", p0, p1, n);
    const int delta = p1 - p0, tail = n - p1;
    if (delta > 0 && tail > 0) {
        const rca_lm_config_t& c = h->cfg;
        RCA_HIP(hipSetDevice(h->device));
        const long slab = 2L * c.n_layers * ATT_KEYS * c.n_kv_heads * 64;      // elements: K rows, then V rows
        if (!h->kv_stage) {
            const int rc = lm_alloc((void**)&h->kv_stage, (size_t)slab * 2 * sizeof(f16_t));
            if (rc != RCA_OK) return rc;
        }
        const int nslab = (tail + ATT_KEYS - 1) / ATT_KEYS;
        const float* cos_d = h->cos_t + (long)delta * 32;      // delta < n <= n_ctx: inside the tables (a borrower reads its owner's)
        const float* sin_d = h->sin_t + (long)delta * 32;
        for (int i = 0; i <= nslab; ++i) {
            const int n_src = i < nslab ? std::min(ATT_KEYS, tail - ATT_KEYS * i) : 0;
            const int n_dst = i > 0 ? std::min(ATT_KEYS, tail - ATT_KEYS * (i - 1)) : 0;
            const long units = (long)c.n_layers * (n_src + n_dst) * c.n_kv_heads * 4;
            const int blocks = (int)std::min<long>((units + 255) / 256, 2048);
            f16_t* const sw = h->kv_stage + (long)(i & 1) * slab;
            const f16_t* const sr = h->kv_stage + (long)((i + 1) & 1) * slab;
            if (lm_kv_q8(h))   // the same steps over blocks (68 of a slab's 128 bytes per head row and tensor are used)
                lm_kv_shift_q8_kernel<<<blocks, 256, 0, h->stream>>>(reinterpret_cast<char*>(h->kc), reinterpret_cast<char*>(h->vc), reinterpret_cast<char*>(sw),
                                                                     reinterpret_cast<const char*>(sr), cos_d, sin_d, h->kv_layer_stride, c.n_layers, c.n_kv_heads,
                                                                     p1 + ATT_KEYS * i, n_src, p0 + ATT_KEYS * (i - 1), n_dst);
            else
                lm_kv_shift_kernel<<<blocks, 256, 0, h->stream>>>(h->kc, h->vc, sw, sr, cos_d, sin_d, h->kv_layer_stride, c.n_layers, c.n_kv_heads,
                                                                  p1 + ATT_KEYS * i, n_src, p0 + ATT_KEYS * (i - 1), n_dst);
            RCA_LAUNCH_CHECK();
        }
        RCA_HIP(hipStreamSynchronize(h->stream));
    }
    h->n_tokens = n - delta;
    return RCA_OK;
}
// ---- the context shift of several handles in one pass (rca_lm_kv_remove_many).  The handles that have rows to move are taken in
// launch groups of RCA_LM_KV_REMOVE_GROUP; step i of a group is ONE launch of the table form, whose row k holds member k's step i.
//   staged member (delta < ATT_KEYS): the steps of the single call, slab for slab, through its own two staging slabs (slot k of the
//     group's staging buffer, which lives on the weight owner and is reused by the next group: the stream orders them).
//   direct member (delta >= ATT_KEYS): slabs of R = delta rows, rotated from the cache straight into the cache.  Step i reads rows
//     [p1 + R i, p1 + R (i + 1)) and writes rows [p0 + R i, p0 + R (i + 1)); the write ends at p0 + R (i + 1) = p1 + R i, where the
//     read starts, so inside a launch no row is both read and written, and every later step reads above what this one wrote.  No
//     staging, half the traffic, ceil(tail / delta) steps.
// The values written are those of the single call on either route: the same unit body, the same RoPE rows.
static rca_lm* lm_weight_root(rca_lm* h) { return h->weights_of ? h->weights_of : h; }
static int lm_kv_remove_many(rca_lm_t* const* hs, int32_t n_h, const int32_t* p0, const int32_t* p1, bool allow_direct) {
    if (!hs || !p0 || !p1) return fail(RCA_ERR_ARG, "kv_remove_many: null argument");
    if (n_h < 1 || n_h > 64) return fail(RCA_ERR_ARG, "kv_remove_many: %d handles (1 to 64)", n_h);
    for (int k = 0; k < n_h; ++k) {
        rca_lm* h = hs[k];
        if (!h) return fail(RCA_ERR_ARG, "kv_remove_many: handle %d is null", k);
        for (int j = 0; j < k; ++j)
            if (hs[j] == h) return fail(RCA_ERR_ARG, "kv_remove_many: handle %d is handle %d again", k, j);
        if (h->device != hs[0]->device) return fail(RCA_ERR_ARG, "kv_remove_many: handle %d is on device %d, handle 0 on device %d", k, h->device, hs[0]->device);
        if (lm_weight_root(h) != lm_weight_root(hs[0]))
            return fail(RCA_ERR_ARG, "kv_remove_many: handle %d does not share handle 0's weights (rca_lm_create_shared): RoPE tables and dimensions must be the same", k);
    }
    for (int k = 0; k < n_h; ++k)
        if (lm_kv_q8(hs[k]) && !hs[k]->kv_shift_requant)
            return fail(RCA_ERR_STATE, "kv_remove_many: handle %d keeps a q8_0 KV cache (rca_lm_set_kv_format); re-rotating quantised keys would quantise them a second time, "
                                       "which this version does not do -- use an fp16 cache for the context shift", k);
    for (int k = 1; k < n_h; ++k)      // one launch runs one unit body
        if (hs[k]->kv_format != hs[0]->kv_format)
            return fail(RCA_ERR_ARG, "kv_remove_many: handle %d has KV format %d, handle 0 has %d (rca_lm_set_kv_format)", k, hs[k]->kv_format, hs[0]->kv_format);
    for (int k = 0; k < n_h; ++k) { const int rc = lm_settle(hs[k]); if (rc != RCA_OK) return rc; }
    for (int k = 0; k < n_h; ++k)
        if (p0[k] < 0 || p0[k] > p1[k] || p1[k] > hs[k]->n_tokens)
            return fail(RCA_ERR_ARG, "kv_remove_many: [%d, %d) of handle %d is not a span of its %d cached positions", p0[k], p1[k], k, hs[k]->n_tokens);
    int act[64], n_act = 0;
    bool any_staged = false;
    for (int k = 0; k < n_h; ++k)
        if (p1[k] > p0[k] && hs[k]->n_tokens > p1[k]) {
            act[n_act++] = k;
            any_staged = any_staged || !(allow_direct && p1[k] - p0[k] >= ATT_KEYS);
        }
    if (n_act) {
        rca_lm* const lead = hs[0];
        rca_lm* const root = lm_weight_root(lead);
        const rca_lm_config_t& c = lead->cfg;
        RCA_HIP(hipSetDevice(lead->device));
        const long slab = 2L * c.n_layers * ATT_KEYS * c.n_kv_heads * 64;      // elements: K rows, then V rows
        if (any_staged && !root->kv_stage_many) {
            const int rc = lm_alloc((void**)&root->kv_stage_many, (size_t)slab * 2 * RCA_LM_KV_REMOVE_GROUP * sizeof(f16_t));
            if (rc != RCA_OK) return rc;
        }
        for (int k = 0; k < n_h; ++k)      // whatever the other handles' streams still hold (a step's tail, a copy_kv) is in their caches first
            if (hs[k]->stream != lead->stream) RCA_HIP(hipStreamSynchronize(hs[k]->stream));
        for (int g0 = 0; g0 < n_act; g0 += RCA_LM_KV_REMOVE_GROUP) {
            const int gn = std::min(RCA_LM_KV_REMOVE_GROUP, n_act - g0);
            int R[RCA_LM_KV_REMOVE_GROUP], steps[RCA_LM_KV_REMOVE_GROUP], n_steps = 0;      // R 0: a staged member
            for (int j = 0; j < gn; ++j) {
                const int k = act[g0 + j], delta = p1[k] - p0[k], tail = hs[k]->n_tokens - p1[k];
                R[j] = allow_direct && delta >= ATT_KEYS ? delta : 0;
                steps[j] = R[j] ? (tail + R[j] - 1) / R[j] : (tail + ATT_KEYS - 1) / ATT_KEYS + 1;
                n_steps = std::max(n_steps, steps[j]);
            }
            for (int i = 0; i < n_steps; ++i) {
                LmShiftTable tab;
                long most = 0;
                for (int j = 0; j < gn; ++j) {
                    const int k = act[g0 + j], delta = p1[k] - p0[k], tail = hs[k]->n_tokens - p1[k];
                    rca_lm* h = hs[k];
                    LmShiftRow& w = tab.row[j];
                    w.kc = h->kc; w.vc = h->vc;
                    w.cos_d = h->cos_t + (long)delta * 32;      // delta < n_tokens <= n_ctx: inside the tables (the owner's, for a borrower)
                    w.sin_d = h->sin_t + (long)delta * 32;
                    w.layer_stride = h->kv_layer_stride;
                    if (R[j]) {
                        w.stage_w = nullptr; w.stage_r = nullptr;
                        w.src_pos = p1[k] + R[j] * i; w.dst_pos = p0[k] + R[j] * i;
                        w.n_src = i < steps[j] ? std::min(R[j], tail - R[j] * i) : 0;
                        w.n_dst = 0;
                    } else {
                        f16_t* st = root->kv_stage_many + (long)j * 2 * slab;
                        const int nslab = steps[j] - 1;
                        w.stage_w = st + (long)(i & 1) * slab; w.stage_r = st + (long)((i + 1) & 1) * slab;
                        w.src_pos = p1[k] + ATT_KEYS * i; w.dst_pos = p0[k] + ATT_KEYS * (i - 1);
                        w.n_src = i < nslab ? std::min(ATT_KEYS, tail - ATT_KEYS * i) : 0;
                        w.n_dst = i > 0 && i <= nslab ? std::min(ATT_KEYS, tail - ATT_KEYS * (i - 1)) : 0;
                    }
                    most = std::max(most, (long)c.n_layers * (w.n_src + w.n_dst) * c.n_kv_heads * 4);
                }
                for (int j = gn; j < RCA_LM_KV_REMOVE_GROUP; ++j) tab.row[j] = LmShiftRow{};
                const int blocks = (int)std::min<long>((most + 255) / 256, 1024);
                if (lm_kv_q8(lead)) lm_kv_shift_many_q8_kernel<<<dim3(blocks, gn), 256, 0, lead->stream>>>(tab, c.n_layers, c.n_kv_heads);
                else lm_kv_shift_many_kernel<<<dim3(blocks, gn), 256, 0, lead->stream>>>(tab, c.n_layers, c.n_kv_heads);
                RCA_LAUNCH_CHECK();
            }
        }
        RCA_HIP(hipStreamSynchronize(lead->stream));
    }
    for (int k = 0; k < n_h; ++k) hs[k]->n_tokens -= p1[k] - p0[k];
    return RCA_OK;
}
extern "C" int rca_lm_kv_remove_many(rca_lm_t* const* hs, int32_t n_h, const int32_t* p0, const int32_t* p1) { return lm_kv_remove_many(hs, n_h, p0, p1, true); }
extern "C" int rca_lm_kv_remove_many_staged(rca_lm_t* const* hs, int32_t n_h, const int32_t* p0, const int32_t* p1) { return lm_kv_remove_many(hs, n_h, p0, p1, false); }
// q8_0 cache: rows [pos0, pos0 + n_pos) of layer `layer` of one tensor (base = kc or vc), de-quantised into dst_host through a scratch buffer
static int lm_kv_read_deq(rca_lm* h, const f16_t* base, int layer, int pos0, int n_pos, uint16_t* dst_host) {
    const long n = (long)n_pos * h->cfg.n_kv_heads * 64, off = (long)pos0 * h->cfg.n_kv_heads * 64;
    f16_t* tmp = nullptr;
    int rc = lm_alloc((void**)&tmp, (size_t)n * sizeof(f16_t));
    if (rc != RCA_OK) return rc;
    lm_kv_dequant_kernel<<<cdiv(n / 16, 256), 256, 0, h->stream>>>(reinterpret_cast<const signed char*>(lm_kv_layer(h, base, layer)) + off,
                                                                   lm_kv_scales(h, base, layer) + (off >> 5), tmp, n / 16);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(dst_host, tmp, (size_t)n * sizeof(f16_t), hipMemcpyDeviceToHost, h->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    (void)hipFree(tmp);
    return e == hipSuccess ? RCA_OK : fail(RCA_ERR_HIP, "kv_read (q8_0): %s", hipGetErrorString(e));
}
// tests only: fp16 rows [n_pos][n_kv_heads][64] of one layer's K and / or V cache -- the raw rows of an fp16 cache, the de-quantised
// rows of a q8_0 cache (exactly the values attention stages)
extern "C" int rca_lm_kv_read(rca_lm_t* h, int32_t layer, int32_t pos0, int32_t n_pos, uint16_t* k_host, uint16_t* v_host) {
    if (!h) return fail(RCA_ERR_ARG, "null");
    const rca_lm_config_t& c = h->cfg;
    if (layer < 0 || layer >= c.n_layers) return fail(RCA_ERR_ARG, "kv_read: layer %d outside [0, %d)", layer, c.n_layers);
    if (pos0 < 0 || n_pos < 0 || pos0 > c.n_ctx - n_pos) return fail(RCA_ERR_ARG, "kv_read: positions [%d, %d + %d) outside the context of %d", pos0, pos0, n_pos, c.n_ctx);
    RCA_HIP(hipSetDevice(h->device));
    RCA_HIP(hipStreamSynchronize(h->stream));
    h->async_pending = false;
    { const int rc = lm_wait_batch_eval(h); if (rc != RCA_OK) return rc; }
    const long off = (long)layer * h->kv_layer_stride + (long)pos0 * c.n_kv_heads * 64;
    const size_t bytes = (size_t)n_pos * c.n_kv_heads * 64 * sizeof(f16_t);
    if (lm_kv_q8(h)) {
        int rc = RCA_OK;
        if (k_host && bytes) rc = lm_kv_read_deq(h, h->kc, layer, pos0, n_pos, k_host);
        if (rc == RCA_OK && v_host && bytes) rc = lm_kv_read_deq(h, h->vc, layer, pos0, n_pos, v_host);
        return rc;
    }
    if (k_host && bytes) RCA_HIP(hipMemcpy(k_host, h->kc + off, bytes, hipMemcpyDeviceToHost));
    if (v_host && bytes) RCA_HIP(hipMemcpy(v_host, h->vc + off, bytes, hipMemcpyDeviceToHost));
    return RCA_OK;
}
// tests only: the raw blocks of a q8_0 cache: int8 values [n_pos][n_kv_heads][64] and fp16 scales [n_pos][n_kv_heads][2] of K and / or V
extern "C" int rca_lm_kv_read_q8(rca_lm_t* h, int32_t layer, int32_t pos0, int32_t n_pos, int8_t* k_q, uint16_t* k_d, int8_t* v_q, uint16_t* v_d) {
    if (!h) return fail(RCA_ERR_ARG, "null");
    const rca_lm_config_t& c = h->cfg;
    if (!lm_kv_q8(h)) return fail(RCA_ERR_STATE, "kv_read_q8: this handle keeps an fp16 KV cache (rca_lm_set_kv_format)");
    if (layer < 0 || layer >= c.n_layers) return fail(RCA_ERR_ARG, "kv_read_q8: layer %d outside [0, %d)", layer, c.n_layers);
    if (pos0 < 0 || n_pos < 0 || pos0 > c.n_ctx - n_pos) return fail(RCA_ERR_ARG, "kv_read_q8: positions [%d, %d + %d) outside the context of %d", pos0, pos0, n_pos, c.n_ctx);
    RCA_HIP(hipSetDevice(h->device));
    RCA_HIP(hipStreamSynchronize(h->stream));
    h->async_pending = false;
    { const int rc = lm_wait_batch_eval(h); if (rc != RCA_OK) return rc; }
    const long off = (long)pos0 * c.n_kv_heads * 64;
    const size_t n = (size_t)n_pos * c.n_kv_heads * 64;
    if (!n) return RCA_OK;
    if (k_q) RCA_HIP(hipMemcpy(k_q, (const char*)lm_kv_layer(h, h->kc, layer) + off, n, hipMemcpyDeviceToHost));
    if (v_q) RCA_HIP(hipMemcpy(v_q, (const char*)lm_kv_layer(h, h->vc, layer) + off, n, hipMemcpyDeviceToHost));
    if (k_d) RCA_HIP(hipMemcpy(k_d, lm_kv_scales(h, h->kc, layer) + (off >> 5), n / 32 * sizeof(f16_t), hipMemcpyDeviceToHost));
    if (v_d) RCA_HIP(hipMemcpy(v_d, lm_kv_scales(h, h->vc, layer) + (off >> 5), n / 32 * sizeof(f16_t), hipMemcpyDeviceToHost));
    return RCA_OK;
}
// tests only: the inverse of rca_lm_kv_read (n_tokens stays as it is); a q8_0 cache quantises the rows with the kernel its passes use
extern "C" int rca_lm_kv_write(rca_lm_t* h, int32_t layer, int32_t pos0, int32_t n_pos, const uint16_t* k_host, const uint16_t* v_host) {
    if (!h) return fail(RCA_ERR_ARG, "null");
    const rca_lm_config_t& c = h->cfg;
    if (layer < 0 || layer >= c.n_layers) return fail(RCA_ERR_ARG, "kv_write: layer %d outside [0, %d)", layer, c.n_layers);
    if (pos0 < 0 || n_pos < 0 || pos0 > c.n_ctx - n_pos) return fail(RCA_ERR_ARG, "kv_write: positions [%d, %d + %d) outside the context of %d", pos0, pos0, n_pos, c.n_ctx);
    RCA_HIP(hipSetDevice(h->device));
    RCA_HIP(hipStreamSynchronize(h->stream));
    h->async_pending = false;
    { const int rc = lm_wait_batch_eval(h); if (rc != RCA_OK) return rc; }
    const long off = (long)layer * h->kv_layer_stride + (long)pos0 * c.n_kv_heads * 64;
    const size_t bytes = (size_t)n_pos * c.n_kv_heads * 64 * sizeof(f16_t);
    if (lm_kv_q8(h)) {   // through the ring, at most LM_KV_RING positions at a time, at the slots a pass would use
        const size_t prow = (size_t)c.n_kv_heads * 64;   // elements per position
        for (int p = 0; p < n_pos && bytes;) {
            const int slot = (pos0 + p) & (LM_KV_RING - 1);
            const int cnt = std::min(n_pos - p, LM_KV_RING - slot);   // up to the ring's end
            if (k_host) RCA_HIP(hipMemcpy(h->ring_k + slot * prow, k_host + p * prow, cnt * prow * sizeof(f16_t), hipMemcpyHostToDevice));
            if (v_host) RCA_HIP(hipMemcpy(h->ring_v + slot * prow, v_host + p * prow, cnt * prow * sizeof(f16_t), hipMemcpyHostToDevice));
            lm_kv_quant_kernel<false><<<dim3(cdiv(4 * c.n_kv_heads, 8), cnt), 256, 0, h->stream>>>(
                nullptr, h->ring_k, h->ring_v, LM_KV_RING - 1, reinterpret_cast<signed char*>(lm_kv_layer(h, h->kc, layer)), reinterpret_cast<signed char*>(lm_kv_layer(h, h->vc, layer)),
                const_cast<f16_t*>(lm_kv_scales(h, h->kc, layer)), const_cast<f16_t*>(lm_kv_scales(h, h->vc, layer)), c.n_kv_heads, c.n_ctx, pos0 + p, cnt,
                (k_host ? 1 : 0) | (v_host ? 2 : 0), nullptr, 0);
            RCA_LAUNCH_CHECK();
            RCA_HIP(hipStreamSynchronize(h->stream));
            p += cnt;
        }
        return RCA_OK;
    }
    if (k_host && bytes) RCA_HIP(hipMemcpy(h->kc + off, k_host, bytes, hipMemcpyHostToDevice));
    if (v_host && bytes) RCA_HIP(hipMemcpy(h->vc + off, v_host, bytes, hipMemcpyHostToDevice));
    return RCA_OK;
}
extern "C" int rca_lm_set_low_priority(rca_lm_t* h, int32_t enable) {
    if (!h) return fail(RCA_ERR_ARG, "null");
    RCA_HIP(hipSetDevice(h->device));
    int lo = 0, hi = 0;
    RCA_HIP(hipDeviceGetStreamPriorityRange(&lo, &hi));   // numerically lower = higher priority
    hipStream_t ns = nullptr;
    RCA_HIP(hipStreamCreateWithPriority(&ns, hipStreamNonBlocking, enable ? lo : hi));
    RCA_HIP(hipStreamSynchronize(h->stream));
    h->async_pending = false;
    { const int rc = lm_wait_batch_eval(h); if (rc != RCA_OK) return rc; }
    (void)hipStreamDestroy(h->stream);
    h->stream = ns;
    return RCA_OK;
}

extern "C" int rca_lm_logits_dev(rca_lm_t* h, const float** out) {
    if (!h || !out) return fail(RCA_ERR_ARG, "null");
    if (h->logits_rows < 1) return fail(RCA_ERR_STATE, "no logits: call eval first");
    *out = h->logits + (long)(h->logits_rows - 1) * h->cfg.vocab_size;
    return RCA_OK;
}
extern "C" int rca_lm_get_logits(rca_lm_t* h, float* out_host) {
    if (!h || !out_host) return fail(RCA_ERR_ARG, "null");
    { const int src = lm_settle(h); if (src != RCA_OK) return src; }
    const float* src;
    int rc;
    if ((rc = rca_lm_logits_dev(h, &src)) != RCA_OK) return rc;
    RCA_HIP(hipSetDevice(h->device));
    RCA_HIP(hipMemcpyAsync(out_host, src, (size_t)h->cfg.vocab_size * 4, hipMemcpyDeviceToHost, h->stream));
    RCA_HIP(hipStreamSynchronize(h->stream));
    return RCA_OK;
}
// Tests only: host-supplied values replace the last logits row, so that the sampler and rca_lm_token_probs can be driven with
// hand-made rows (caps, ties, infinities) that no model's head produces on demand
extern "C" int rca_lm_put_logits(rca_lm_t* h, const float* logits_host) {
    if (!h || !logits_host) return fail(RCA_ERR_ARG, "null");
    { const int src = lm_settle(h); if (src != RCA_OK) return src; }
    if (h->logits_rows < 1) return fail(RCA_ERR_STATE, "no logits: call eval first");
    RCA_HIP(hipSetDevice(h->device));
    RCA_HIP(hipMemcpyAsync(h->logits + (long)(h->logits_rows - 1) * h->cfg.vocab_size, logits_host, (size_t)h->cfg.vocab_size * 4,
                           hipMemcpyHostToDevice, h->stream));
    RCA_HIP(hipStreamSynchronize(h->stream));
    return RCA_OK;
}
extern "C" int rca_lm_get_logits_row(rca_lm_t* h, int32_t row, float* out_host) {
    if (!h || !out_host) return fail(RCA_ERR_ARG, "null");
    { const int src = lm_settle(h); if (src != RCA_OK) return src; }
    if (row < 0 || row >= h->logits_rows) return fail(RCA_ERR_ARG, "row %d outside the %d rows of the last eval", row, h->logits_rows);
    RCA_HIP(hipSetDevice(h->device));
    RCA_HIP(hipMemcpyAsync(out_host, h->logits + (long)row * h->cfg.vocab_size, (size_t)h->cfg.vocab_size * 4, hipMemcpyDeviceToHost, h->stream));
    RCA_HIP(hipStreamSynchronize(h->stream));
    return RCA_OK;
}

extern "C" int rca_lm_sampler_init(rca_lm_t* h, const rca_sampler_params_t* p) {
    if (!h || !p) return fail(RCA_ERR_ARG, "null");
    if (p->n_bias < 0 || p->n_bias > 8) return fail(RCA_ERR_ARG, "at most 8 logit-bias entries");
    // llama.cpp reads top_k <= 0 as "whole vocabulary" and honours any top_k up to it; penalties default to off.  Nothing is clamped:
    // 1..SAMP_MAXK ranked candidates take the serial chain (float sums, inverse-CDF draw), everything else the whole-vocabulary
    // sampler -- plain (top_p >= 1, no rank cut) or with the radix-select thresholds of the "big" path.
    const int V = h->cfg.vocab_size;
    if (!(p->repeat_penalty > 0.0f) && p->repeat_penalty != 0.0f) return fail(RCA_ERR_ARG, "sampler: repeat_penalty %g must be positive", (double)p->repeat_penalty);
    const float rep = p->repeat_penalty == 0.0f ? 1.0f : p->repeat_penalty;    // a zero-initialised struct (older callers) means "off"
    const bool stoch = p->temp > 0.0f;
    const bool full = stoch && (p->top_k <= 0 || p->top_k > SAMP_MAXK);
    const bool big_k = full && p->top_k > SAMP_MAXK && p->top_k < V;
    const bool big_p = full && p->top_p < 1.0f;
    const bool pen = rep != 1.0f || p->freq_penalty != 0.0f || p->presence_penalty != 0.0f;
    const bool patch = p->n_bias > 0 || pen;
    RCA_HIP(hipSetDevice(h->device));
    SamplerDev s;
    memset(&s, 0, sizeof(s));
    s.top_k = p->top_k; s.top_p = p->top_p; s.min_p = p->min_p; s.temp = p->temp; s.seed = p->seed; s.n_bias = p->n_bias;
    for (int i = 0; i < p->n_bias; ++i) { s.bias_ids[i] = p->bias_ids[i]; s.bias_vals[i] = p->bias_vals[i]; }
    s.repeat_penalty = rep; s.freq_penalty = p->freq_penalty; s.presence_penalty = p->presence_penalty;
    s.last_n = p->penalty_last_n > 0 ? std::min(p->penalty_last_n, 64) : (p->penalty_last_n == 0 ? 64 : 0);   // 0 = llama-cpp-python's default window, < 0 = off
    s.patch = patch ? 1 : 0; s.big_k = big_k ? p->top_k : 0; s.big_p = big_p ? 1 : 0;
    RCA_HIP(hipStreamSynchronize(h->stream));
    RCA_HIP(hipMemcpy(h->samp, &s, sizeof(s), hipMemcpyHostToDevice));
    // set_seed restarts the stream of draws (llamacpp_utils.py:58)
    const unsigned long long zero = 0;
    RCA_HIP(hipMemcpy(&h->stt->rng_counter, &zero, 8, hipMemcpyHostToDevice));
    h->rng_host = 0;
    h->sampler_set = true;
    if (full != h->samp_full || patch != h->samp_patch || big_k != h->samp_big_k || big_p != h->samp_big_p || h->samp_typ || h->samp_miro)
        lm_drop_graphs(h);   // the captured steps hold another set of sampler launches
    h->samp_full = full; h->samp_patch = patch; h->samp_big_k = big_k; h->samp_big_p = big_p;
    h->samp_typ = h->samp_miro = false;   // both options are off after every init (s.typical_p = 0, s.miro = 0)
    h->samp_host = s;
    return RCA_OK;
}

// typical_p and mirostat v2 ride on the sampler rca_lm_sampler_init set up: one field of SamplerDev each, and the choice of launches
static int lm_sampler_route(rca_lm* h, const SamplerDev& s) {
    const bool stoch = s.temp > 0.0f;
    const bool miro = stoch && s.miro == 2;
    const bool typ = stoch && !miro && s.typical_p > 0.0f && s.typical_p < 1.0f;
    if (typ && (s.top_k < 1 || s.top_k > SAMP_MAXK))
        return fail(RCA_ERR_ARG, "sampler: typical_p %g needs top_k in 1..%d (top_k is %d): the whole vocabulary is not sorted by typicality",
                    (double)s.typical_p, SAMP_MAXK, s.top_k);
    RCA_HIP(hipSetDevice(h->device));
    RCA_HIP(hipStreamSynchronize(h->stream));
    RCA_HIP(hipMemcpy(h->samp, &s, sizeof(s), hipMemcpyHostToDevice));
    if (typ != h->samp_typ || miro != h->samp_miro) lm_drop_graphs(h);
    h->samp_typ = typ; h->samp_miro = miro;
    h->samp_host = s;
    return RCA_OK;
}
extern "C" int rca_lm_sampler_set_typical(rca_lm_t* h, float typical_p) {
    if (!h) return fail(RCA_ERR_ARG, "null");
    { const int src = lm_settle(h); if (src != RCA_OK) return src; }
    if (!h->sampler_set) return fail(RCA_ERR_STATE, "sampler not initialised");
    if (!(typical_p >= 0.0f)) return fail(RCA_ERR_ARG, "sampler: typical_p %g must be 0 (unset) or positive", (double)typical_p);
    SamplerDev s = h->samp_host;
    s.typical_p = typical_p;
    return lm_sampler_route(h, s);
}
extern "C" int rca_lm_sampler_set_mirostat(rca_lm_t* h, int32_t mode, float tau, float eta) {
    if (!h) return fail(RCA_ERR_ARG, "null");
    { const int src = lm_settle(h); if (src != RCA_OK) return src; }
    if (!h->sampler_set) return fail(RCA_ERR_STATE, "sampler not initialised");
    if (mode == 1) return fail(RCA_ERR_ARG, "sampler: mirostat_mode 1 (v1) is not built: its k is computed per draw and can land on any route; use 0 or 2");
    if (mode != 0 && mode != 2) return fail(RCA_ERR_ARG, "sampler: mirostat_mode %d is none of 0 (off), 2 (v2)", mode);
    if (mode == 2 && !(tau >= 0.0f && tau <= 3.0e38f)) return fail(RCA_ERR_ARG, "sampler: mirostat_tau %g must be finite and not negative", (double)tau);
    if (mode == 2 && !(eta >= 0.0f && eta <= 3.0e38f)) return fail(RCA_ERR_ARG, "sampler: mirostat_eta %g must be finite and not negative", (double)eta);
    SamplerDev s = h->samp_host;
    s.miro = mode; s.miro_tau = mode == 2 ? tau : 0.0f; s.miro_eta = mode == 2 ? eta : 0.0f;
    const int rc = lm_sampler_route(h, s);
    if (rc != RCA_OK) return rc;
    if (mode == 2) {   // mu = 2 tau before the next draw, whichever it is (llamacpp_utils.py:60): every slot, so the counter need not be read
        std::vector<float> mu(SAMP_RING, 2.0f * tau);
        RCA_HIP(hipMemcpy(h->swork->mu_ring, mu.data(), sizeof(float) * SAMP_RING, hipMemcpyHostToDevice));
    }
    return RCA_OK;
}
extern "C" int rca_lm_sampler_get_mirostat_mu(rca_lm_t* h, float* mu) {
    if (!h || !mu) return fail(RCA_ERR_ARG, "null");
    { const int src = lm_settle(h); if (src != RCA_OK) return src; }
    if (!h->sampler_set || h->samp_host.miro != 2) return fail(RCA_ERR_STATE, "mirostat is off (rca_lm_sampler_set_mirostat)");
    RCA_HIP(hipSetDevice(h->device));
    RCA_HIP(hipStreamSynchronize(h->stream));
    unsigned long long c = 0;
    RCA_HIP(hipMemcpy(&c, &h->stt->rng_counter, 8, hipMemcpyDeviceToHost));
    RCA_HIP(hipMemcpy(mu, &h->swork->mu_ring[c % SAMP_RING], 4, hipMemcpyDeviceToHost));
    return RCA_OK;
}

// (the kernels of the two opt-in samplers are defined at the end of this file, behind every kernel that was here before them, so that
// the code object lays those out as it did)
__global__ void samp_final_typ_kernel(float* logits, int V, const SamplerDev* __restrict__ sp, LmDevState* __restrict__ stt, SampWork* __restrict__ w,
                                      SampTail tail);
__global__ void samp_miro_mass_kernel(const float* __restrict__ logits, int V, const SamplerDev* __restrict__ sp, SampWork* __restrict__ w);
__global__ void samp_miro_pick_kernel(const float* __restrict__ logits, int V, const SamplerDev* __restrict__ sp, const LmDevState* __restrict__ stt,
                                      SampWork* __restrict__ w);
__global__ void samp_miro_final_kernel(float* logits, int V, const SamplerDev* __restrict__ sp, LmDevState* __restrict__ stt, SampWork* __restrict__ w,
                                       SampTail tail);
// frame_i >= 0: step i of a frame graph -- the sampler's tail also advances the device state and gathers the next pair's embeddings
static void lm_enqueue_sample(rca_lm* h, float* lg, hipStream_t st, int frame_i = -1) {
    const int V = h->cfg.vocab_size;
    const SampTail tail{frame_i, h->embed, h->embed_f32, h->x, h->cfg.hidden};
    if (h->samp_patch) samp_prepare_kernel<<<1, 128, 0, st>>>(lg, V, h->samp, h->stt, h->swork);   // logit bias / penalties, in place
    if (h->samp_miro) {   // mirostat v2: the whole vocabulary cut at a surprise of mu, whatever top_k / top_p / min_p / typical_p say
        samp_full_max_kernel<<<SAMPF_SLICES, 1024, 0, st>>>(lg, V, h->samp, h->swork);
        samp_miro_mass_kernel<<<SAMPF_SLICES, 1024, 0, st>>>(lg, V, h->samp, h->swork);
        samp_miro_pick_kernel<<<SAMPF_SLICES, 1024, 0, st>>>(lg, V, h->samp, h->stt, h->swork);
        samp_miro_final_kernel<<<1, 1024, 0, st>>>(lg, V, h->samp, h->stt, h->swork, tail);
        return;
    }
    if (h->samp_full) {   // top_k <= 0 or > SAMP_MAXK: whole vocabulary (Gumbel-max), with a rank and / or mass threshold on the big path
        samp_full_max_kernel<<<SAMPF_SLICES, 1024, 0, st>>>(lg, V, h->samp, h->swork);
        if (h->samp_big_k || h->samp_big_p) {
            for (int m = 0; m < 2; ++m) {
                if (!(m == 0 ? h->samp_big_k : h->samp_big_p)) continue;
                for (int l = 0; l < SAMP_LEVELS; ++l) samp_radix_pass_kernel<<<128, 256, 0, st>>>(lg, V, h->samp, h->swork, m, l);
                samp_radix_finish_kernel<<<1, 256, 0, st>>>(h->samp, h->swork, m);
            }
            samp_big_pick_kernel<<<SAMPF_SLICES, 1024, 0, st>>>(lg, V, h->samp, h->stt, h->swork);
        } else {
            samp_full_pick_kernel<<<SAMPF_SLICES, 1024, 0, st>>>(lg, V, h->samp, h->stt, h->swork);
        }
        samp_full_final_kernel<<<1, 1024, 0, st>>>(lg, V, h->samp, h->stt, h->swork, tail);
        return;
    }
    samp_hist_kernel<<<128, 256, 0, st>>>(lg, V, h->samp, h->swork);
    samp_gather_kernel<<<128, 256, 0, st>>>(lg, V, h->samp, h->swork);
    if (h->samp_typ) samp_final_typ_kernel<<<1, 1024, 0, st>>>(lg, V, h->samp, h->stt, h->swork, tail);
    else samp_final_kernel<<<1, 1024, 0, st>>>(lg, V, h->samp, h->stt, h->swork, tail);
}
// a member of a batch whose sampler the table kernels do not run: its own launches follow the pass (lm_enqueue_sample)
static inline bool lm_samp_own_launches(const rca_lm* h) { return h->samp_full || h->samp_typ || h->samp_miro; }

static int lm_fetch_token(rca_lm* h, int32_t* token, hipStream_t st) {
    RCA_HIP(hipMemcpyAsync(&h->h_stt->out_token, &h->stt->out_token, 4, hipMemcpyDeviceToHost, st));
    RCA_HIP(hipStreamSynchronize(st));
    *token = h->h_stt->out_token;
    return RCA_OK;
}

extern "C" int rca_lm_sample(rca_lm_t* h, int32_t* token) {
    if (!h || !token) return fail(RCA_ERR_ARG, "null");
    { const int src = lm_settle(h); if (src != RCA_OK) return src; }
    if (!h->sampler_set) return fail(RCA_ERR_STATE, "sampler not initialised");
    if (h->logits_rows < 1) return fail(RCA_ERR_STATE, "no logits: call eval first");
    RCA_HIP(hipSetDevice(h->device));
    float* lg = h->logits + (long)(h->logits_rows - 1) * h->cfg.vocab_size;
    lm_enqueue_sample(h, lg, h->stream);
    RCA_LAUNCH_CHECK();
    h->rng_host += 1;
    return lm_fetch_token(h, token, h->stream);
}

// eval(ids[0..n)) + sample with no host round trip in between.  For n <= 2 and a plain (not
// logits_all) handle the whole step is one hipGraph replay.
// eval + sample (+ optionally softmax(logits)[probe ids] of the evaluated position) as one replay and one synchronisation
static int lm_step_impl(rca_lm_t* h, const int32_t* ids, int32_t n, const int32_t* probe_ids, int32_t n_probe, int32_t* token, float* probs_out,
                        int cap_bucket = -1) {
    if (!h || !ids || !token || n < 1) return fail(RCA_ERR_ARG, "step: bad argument");
    if (n_probe < 0 || n_probe > 8 || (n_probe > 0 && (!probe_ids || !probs_out))) return fail(RCA_ERR_ARG, "step: 0..8 probe ids");
    { const int src = lm_settle(h); if (src != RCA_OK) return src; }
    if (!h->sampler_set) return fail(RCA_ERR_STATE, "sampler not initialised");
    if (h->n_tokens + n > h->cfg.n_ctx) return fail(RCA_ERR_STATE, "context overflow: %d + %d > n_ctx %d", h->n_tokens, n, h->cfg.n_ctx);
    for (int i = 0; i < n; ++i)
        if (ids[i] < 0 || ids[i] >= h->cfg.vocab_size) return fail(RCA_ERR_ARG, "step: token id %d at index %d is outside the vocabulary [0, %d)", ids[i], i, h->cfg.vocab_size);
    for (int i = 0; i < n_probe; ++i)
        if (probe_ids[i] < 0 || probe_ids[i] >= h->cfg.vocab_size) return fail(RCA_ERR_ARG, "step: probe id %d is outside the vocabulary", probe_ids[i]);
    RCA_HIP(hipSetDevice(h->device));
    hipStream_t st = h->stream;
    int rc;
    if (n > 2 || h->cfg.logits_all || !h->graphs_enabled) {
        if ((rc = rca_lm_eval(h, ids, n)) != RCA_OK) return rc;
        if ((rc = rca_lm_sample(h, token)) != RCA_OK) return rc;
        return n_probe ? rca_lm_token_probs(h, probe_ids, n_probe, probs_out) : RCA_OK;
    }
    // stage inputs in pinned memory; the graph's first node copies them to the device
    lm_stage_state(h, ids, n);
    for (int i = 0; i < n_probe; ++i) h->h_probe[i] = probe_ids[i];
    const LmBucket bk = lm_bucket(h, n, cap_bucket);
    rca_lm::GraphSet& gs = lm_graph_set(h);
    hipGraphExec_t& gexec = n_probe ? gs.gp[n][bk.bucket] : gs.g[n][bk.bucket];
    if (n_probe && gexec && gs.gp_nprobe[n][bk.bucket] != n_probe) { (void)hipGraphExecDestroy(gexec); gexec = nullptr; }
    if (!gexec) {
        rc = lm_capture(st, &gexec, "step", [&]() -> int {
            hipError_t e = hipMemcpyAsync(h->stt, h->h_stt, LM_STATE_DECODE_BYTES, hipMemcpyHostToDevice, st);
            if (e == hipSuccess && n_probe) e = hipMemcpyAsync(h->probe_ids_dev, h->h_probe, n_probe * 4, hipMemcpyHostToDevice, st);
            if (e != hipSuccess) return fail(RCA_ERR_HIP, "capture memcpy: %s", hipGetErrorString(e));
            const int r = lm_enqueue_pass(h, n, 1, st, bk.nsp_launch);
            if (r != RCA_OK) return r;
            lm_enqueue_sample(h, h->logits, st);
            if (n_probe) {   // rca_lm_token_probs' two launches, over the logits this step just wrote
                lm_softmax_slices_kernel<<<PROBS_SLICES, 1024, 0, st>>>(h->logits, h->cfg.vocab_size, h->probs_dev + 64);
                lm_token_probs_kernel<<<1, 64, 0, st>>>(h->logits, h->cfg.vocab_size, h->probs_dev + 64, h->probe_ids_dev, n_probe, h->probs_dev);
            }
            e = hipMemcpyAsync(&h->h_stt->out_token, &h->stt->out_token, 4, hipMemcpyDeviceToHost, st);
            if (e == hipSuccess && n_probe) e = hipMemcpyAsync(h->h_probe + 64, h->probs_dev, n_probe * 4, hipMemcpyDeviceToHost, st);
            return e == hipSuccess ? RCA_OK : fail(RCA_ERR_HIP, "capture d2h: %s", hipGetErrorString(e));
        });
        if (rc != RCA_OK) return rc;
        if (n_probe) gs.gp_nprobe[n][bk.bucket] = n_probe;
    }
    if (cap_bucket >= 0) return RCA_OK;      // rca_duplex_precapture: the graph exists now, nothing is launched
    RCA_HIP(hipGraphLaunch(gexec, st));
    RCA_HIP(hipStreamSynchronize(st));
    h->n_tokens += n;
    h->logits_rows = 1;
    h->rng_host += 1;
    *token = h->h_stt->out_token;
    for (int i = 0; i < n_probe; ++i) probs_out[i] = reinterpret_cast<const float*>(h->h_probe + 64)[i];
    return RCA_OK;
}
static int lm_step_capture_only(rca_lm_t* h, int n, int n_probe, int bucket) {
    if (h->cfg.logits_all || !h->graphs_enabled || n > 2) return RCA_OK;
    const int32_t ids[2] = {0, 0}, probes[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    int32_t tok = 0;
    float pr[8];
    return lm_step_impl(h, ids, n, n_probe ? probes : nullptr, n_probe, &tok, n_probe ? pr : nullptr, bucket);
}
// eval(ids[0..n)) + sample with no host round trip in between.  For n <= 2 and a plain (not
// logits_all) handle the whole step is one hipGraph replay.
extern "C" int rca_lm_step(rca_lm_t* h, const int32_t* ids, int32_t n, int32_t* token) {
    return lm_step_impl(h, ids, n, nullptr, 0, token, nullptr);
}
// rca_lm_step + rca_lm_token_probs of the position just evaluated, as ONE replay and one synchronisation: the agent's speculative
// <|end_audio|> step (get_probable_event_speaker, realtime_agent_v2.py:455-466: eval, sample, softmax(logits)[agent / user speaker])
extern "C" int rca_lm_step_probe(rca_lm_t* h, const int32_t* ids, int32_t n, const int32_t* probe_ids, int32_t n_probe, int32_t* token, float* probs_out) {
    if (n_probe < 1) return fail(RCA_ERR_ARG, "step_probe: 1..8 probe ids");
    return lm_step_impl(h, ids, n, probe_ids, n_probe, token, probs_out);
}

// ------------------------------------------------------------------------------------ group step (rca_lm_group_step)
// Several sessions over ONE set of weights (rca_lm_create_shared twins) advance by n tokens each in one pass: every projection is one
// GEMV launch over the n_members * n rows, so a matrix is streamed once whatever the number of sessions (the reference's self-play
// loads the GGUF twice and streams it twice, inference_client_self_play.py:148-159).  Per-session work -- attention over the
// session's own cache, its sampler chain -- stays one launch (chain) per member.  The rows live in the FIRST member's activation
// buffers (x, qkv, attn, hbuf hold nothing between calls) and the pass runs on its stream, as one linear launch sequence.
#define LM_GROUP_MAX 4
struct LmGroupStage { int n_tokens[LM_GROUP_MAX]; int ids[LM_GROUP_MAX][LM_GEMV_M]; };
struct LmGroupPin { LmGroupStage in; int tokens[LM_GROUP_MAX]; };
struct rca_lm_group {
    int n_members = 0;
    rca_lm* m[LM_GROUP_MAX] = {};
    // row tables [n - 1][0 .. 3] = the QKV rows (member s, token j) -> row s * n + j, [n - 1][4 .. 7] = the head rows, one per member
    LmGroupRow* rows = nullptr;        // device, [LM_GEMV_M][2 * LM_GROUP_MAX]
    bool rows_valid = false;
    unsigned long long epoch[LM_GROUP_MAX] = {};   // the members' graph epochs the tables and graphs below were made under
    LmGroupStage* stage = nullptr;     // device copy of pin->in
    int* tokens = nullptr;             // device: the members' sampled tokens, gathered for one download
    LmGroupPin* pin = nullptr;         // pinned
    hipGraphExec_t g[LM_GEMV_M][LM_GRAPH_BUCKETS] = {};   // (n, largest context bucket among the members)
};
// the members' step states for this pass: what lm_push_state uploads for one handle, from one staging block
__global__ void lm_group_stage_kernel(const LmGroupStage* __restrict__ in, const LmGroupRow* __restrict__ head_rows, int n_members, int n) {
    const int s = threadIdx.x;
    if (s >= n_members) return;
    LmDevState* stt = head_rows[s].stt;
    stt->n_tokens = in->n_tokens[s];
    stt->m = n;
    for (int j = 0; j < n; ++j) stt->ids[j] = in->ids[s][j];
}
__global__ __launch_bounds__(256) void lm_embed_group_kernel(const LmGroupRow* __restrict__ rows, const void* __restrict__ table, int f32tab,
                                                             float* __restrict__ x, int H, int V) {
    const int m = blockIdx.x;
    int id = rows[m].stt->ids[rows[m].j];
    id = id < 0 ? 0 : (id >= V ? V - 1 : id);
    if (f32tab) {
        const float* row = reinterpret_cast<const float*>(table) + (long)id * H;
        for (int h = threadIdx.x; h < H; h += 256) x[(long)m * H + h] = row[h];
    } else {
        const bf16_t* row = reinterpret_cast<const bf16_t*>(table) + (long)id * H;
        for (int h = threadIdx.x; h < H; h += 256) x[(long)m * H + h] = __uint_as_float((unsigned)row[h] << 16);
    }
}
__global__ void lm_group_tokens_kernel(const LmGroupRow* __restrict__ head_rows, int n_members, int* __restrict__ out) {
    if ((int)threadIdx.x < n_members) out[threadIdx.x] = head_rows[threadIdx.x].stt->out_token;
}
static void lm_group_drop_graphs(rca_lm_group* g) {
    for (auto& per_n : g->g)
        for (hipGraphExec_t& e : per_n)
            if (e) { (void)hipGraphExecDestroy(e); e = nullptr; }
}
static const rca_lm* lm_weight_owner(const rca_lm* h) { return h->weights_of ? h->weights_of : h; }
extern "C" int rca_lm_group_create(rca_lm_t* const* members, int32_t n_members, rca_lm_group_t** out) {
    if (!members || !out) return fail(RCA_ERR_ARG, "group_create: null argument");
    if (n_members < 2 || n_members > LM_GROUP_MAX) return fail(RCA_ERR_ARG, "group_create: %d members, a group has 2 to %d", n_members, LM_GROUP_MAX);
    for (int s = 0; s < n_members; ++s) {
        const rca_lm* h = members[s];
        if (!h) return fail(RCA_ERR_ARG, "group_create: member %d is null", s);
        for (int t = 0; t < s; ++t)
            if (members[t] == h) return fail(RCA_ERR_ARG, "group_create: member %d is the same handle as member %d", s, t);
        if (h->device != members[0]->device) return fail(RCA_ERR_ARG, "group_create: member %d is on device %d, member 0 on device %d", s, h->device, members[0]->device);
        if (lm_weight_owner(h) != lm_weight_owner(members[0]))
            return fail(RCA_ERR_ARG, "group_create: member %d does not share member 0's weights (rca_lm_create_shared makes handles that do)", s);
        if (h->act_format != members[0]->act_format)
            return fail(RCA_ERR_ARG, "group_create: member %d has activation format %d, member 0 has %d", s, h->act_format, members[0]->act_format);
        if (h->kv_format != members[0]->kv_format)
            return fail(RCA_ERR_ARG, "group_create: member %d has KV format %d, member 0 has %d", s, h->kv_format, members[0]->kv_format);
        if (h->cfg.logits_all) return fail(RCA_ERR_ARG, "group_create: member %d is a logits_all handle (a group step keeps the last position's logits only)", s);
    }
    RCA_HIP(hipSetDevice(members[0]->device));
    rca_lm_group* g = new rca_lm_group();
    g->n_members = n_members;
    for (int s = 0; s < n_members; ++s) g->m[s] = members[s];
    int rc = lm_alloc((void**)&g->rows, sizeof(LmGroupRow) * LM_GEMV_M * 2 * LM_GROUP_MAX);
    if (rc == RCA_OK) rc = lm_alloc((void**)&g->stage, sizeof(LmGroupStage));
    if (rc == RCA_OK) rc = lm_alloc((void**)&g->tokens, sizeof(int) * LM_GROUP_MAX);
    if (rc == RCA_OK && hipHostMalloc((void**)&g->pin, sizeof(LmGroupPin), hipHostMallocDefault) != hipSuccess) rc = fail(RCA_ERR_HIP, "group_create: pinned staging");
    if (rc != RCA_OK) { rca_lm_group_destroy(g); return rc; }
    memset(g->pin, 0, sizeof(LmGroupPin));
    *out = g;
    return RCA_OK;
}
extern "C" int rca_lm_group_destroy(rca_lm_group_t* g) {
    if (!g) return RCA_OK;
    lm_group_drop_graphs(g);
    for (void* p : {(void*)g->rows, (void*)g->stage, (void*)g->tokens})
        if (p) (void)hipFree(p);
    if (g->pin) (void)hipHostFree(g->pin);
    delete g;
    return RCA_OK;
}
// tables + graphs follow the members: a swapped cache, a moved logits buffer or another sampler chain shows as a new epoch
static int lm_group_refresh(rca_lm_group* g) {
    bool same = g->rows_valid;
    for (int s = 0; s < g->n_members; ++s) same = same && g->epoch[s] == g->m[s]->graph_epoch;
    if (same) return RCA_OK;
    lm_group_drop_graphs(g);
    LmGroupRow tab[LM_GEMV_M][2 * LM_GROUP_MAX];
    memset(tab, 0, sizeof(tab));
    for (int n = 1; n <= LM_GEMV_M; ++n)
        for (int s = 0; s < g->n_members; ++s) {
            rca_lm* h = g->m[s];
            LmGroupRow r = lm_group_row(h, 0, 0);
            r.j = n - 1; r.xrow = s * n + n - 1;
            tab[n - 1][LM_GROUP_MAX + s] = r;
            for (int j = 0; j < n && s * n + j < LM_GROUP_MAX; ++j) {
                r.j = j; r.xrow = s * n + j;
                tab[n - 1][s * n + j] = r;
            }
        }
    RCA_HIP(hipMemcpy(g->rows, tab, sizeof(tab), hipMemcpyHostToDevice));
    for (int s = 0; s < g->n_members; ++s) g->epoch[s] = g->m[s]->graph_epoch;
    g->rows_valid = true;
    return RCA_OK;
}
// upload of the staged states -> embedding -> the layers -> head -> every member's sampler -> download of the tokens, all on `st`
static int lm_group_enqueue(rca_lm_group* g, int n, int nsp_launch, hipStream_t st) {
    rca_lm* ws = g->m[0];
    const rca_lm_config_t& c = ws->cfg;
    const int NM = g->n_members, MT = NM * n;
    const int QKV = (c.n_heads + 2 * c.n_kv_heads) * c.head_dim, AO = c.n_heads * c.head_dim;
    const LmGroupRow* qrows = g->rows + (size_t)(n - 1) * 2 * LM_GROUP_MAX;
    const LmGroupRow* hrows = qrows + LM_GROUP_MAX;
    hipError_t e = hipMemcpyAsync(g->stage, &g->pin->in, sizeof(LmGroupStage), hipMemcpyHostToDevice, st);
    if (e != hipSuccess) return fail(RCA_ERR_HIP, "group step upload: %s", hipGetErrorString(e));
    lm_group_stage_kernel<<<1, 64, 0, st>>>(g->stage, hrows, NM, n);
    lm_embed_group_kernel<<<MT, 256, 0, st>>>(qrows, ws->embed, ws->embed_f32, ws->x, c.hidden, c.vocab_size);
    for (int l = 0; l < c.n_layers; ++l) {
        const LmLayer& L = ws->layers[l];
        const GemvPro pro{ws->x, L.attn_norm, c.rms_eps, 0};
        GemvRope rope{ws->cos_t, ws->sin_t, nullptr, nullptr, c.n_heads, c.n_kv_heads, 0, 0};   // cache, position and context bound: per row, from the table
        const GemvGroup grp{qrows, l};
        launch_gemv<1, 2, 1>(GEMV_QKV, ws, MT, L.qkv, nullptr, ws->qkv, L.qkv.N, c.hidden, QKV, pro, rope, st, grp);
        if (L.split_v) {
            rope.row_base = L.qkv.N;
            launch_gemv<1, 2, 1>(GEMV_QKV, ws, MT, L.vseg, nullptr, ws->qkv, L.vseg.N, c.hidden, QKV, pro, rope, st, grp);
        }
        for (int s = 0; s < NM; ++s) {
            rca_lm* h = g->m[s];
            lm_launch_kv_quant(h, l, n, st);   // (q8_0 caches: the member's rows of the pass, as its own launches do)
            launch_attention_mfma(h, n, std::min(nsp_launch, h->n_splits), lm_kv_layer(h, h->kc, l), lm_kv_layer(h, h->vc, l),
                                  ws->qkv + (long)s * n * QKV, ws->attn + (long)s * n * AO, st);
        }
        lm_launch_o(ws, l, MT, st);
        lm_launch_gu(ws, l, MT, st);
        lm_launch_down(ws, l, MT, st);
    }
    // final RMSNorm + head over the last row of every member, each row's logits straight into its member's buffer
    launch_gemv<1, 0, 1>(GEMV_HEAD, ws, NM, ws->head, nullptr, nullptr, c.vocab_size, c.hidden, c.vocab_size, GemvPro{ws->x, ws->final_norm, c.rms_eps, 1}, norope, st,
                         GemvGroup{hrows, 0});
    for (int s = 0; s < NM; ++s) lm_enqueue_sample(g->m[s], g->m[s]->logits, st);
    lm_group_tokens_kernel<<<1, 64, 0, st>>>(hrows, NM, g->tokens);
    RCA_LAUNCH_CHECK();
    e = hipMemcpyAsync(g->pin->tokens, g->tokens, sizeof(int) * LM_GROUP_MAX, hipMemcpyDeviceToHost, st);
    return e == hipSuccess ? RCA_OK : fail(RCA_ERR_HIP, "group step download: %s", hipGetErrorString(e));
}
extern "C" int rca_lm_group_step(rca_lm_group_t* g, const int32_t* ids, int32_t n, int32_t* tokens) {
    if (!g || !ids || !tokens) return fail(RCA_ERR_ARG, "group_step: null argument");
    const int NM = g->n_members;
    if (n < 1 || n > LM_GEMV_M || (NM * n != 2 && NM * n != 4))
        return fail(RCA_ERR_ARG, "group_step: %d members x %d tokens = %d rows, a group pass has 2 or 4 (2 x 1, 2 x 2 or 4 x 1)", NM, n, NM * n);
    int rc;
    for (int s = 0; s < NM; ++s)
        if ((rc = lm_settle(g->m[s])) != RCA_OK) return rc;
    // every refusal before anything is staged or enqueued: no member changes
    for (int s = 0; s < NM; ++s) {
        const rca_lm* h = g->m[s];
        if (!h->sampler_set) return fail(RCA_ERR_STATE, "group_step: member %d has no sampler (rca_lm_sampler_init)", s);
        if (h->cfg.logits_all) return fail(RCA_ERR_STATE, "group_step: member %d was switched to logits_all after the group was made", s);
        if (h->kv_format != g->m[0]->kv_format) return fail(RCA_ERR_STATE, "group_step: member %d has KV format %d, member 0 has %d", s, h->kv_format, g->m[0]->kv_format);
        if (h->act_format != g->m[0]->act_format) return fail(RCA_ERR_STATE, "group_step: member %d has activation format %d, member 0 has %d", s, h->act_format, g->m[0]->act_format);
        if (h->n_tokens + n > h->cfg.n_ctx) return fail(RCA_ERR_STATE, "group_step: context overflow of member %d: %d + %d > n_ctx %d", s, h->n_tokens, n, h->cfg.n_ctx);
        for (int j = 0; j < n; ++j)
            if (ids[s * n + j] < 0 || ids[s * n + j] >= h->cfg.vocab_size)
                return fail(RCA_ERR_ARG, "group_step: token id %d of member %d at index %d is outside the vocabulary [0, %d)", ids[s * n + j], s, j, h->cfg.vocab_size);
    }
    RCA_HIP(hipSetDevice(g->m[0]->device));
    hipStream_t st = g->m[0]->stream;
    if ((rc = lm_group_refresh(g)) != RCA_OK) return rc;
    bool graphs = true;
    int bucket = 0, nsp = 1;
    for (int s = 0; s < NM; ++s) {
        const rca_lm* h = g->m[s];
        graphs = graphs && h->graphs_enabled;
        g->pin->in.n_tokens[s] = h->n_tokens;
        for (int j = 0; j < n; ++j) g->pin->in.ids[s][j] = ids[s * n + j];
        bucket = std::max(bucket, lm_bucket(h, n, -1).bucket);
        nsp = std::max(nsp, lm_splits_needed(h, n));
    }
    if (graphs) {
        // the split count of the largest bucket among the members (each member's launch is capped at its own cache below)
        const int nsp_bucket = bucket + 1 == LM_GRAPH_BUCKETS ? INT_MAX : 4 << bucket;
        hipGraphExec_t& gexec = g->g[n - 1][bucket];
        if (!gexec && (rc = lm_capture(st, &gexec, "group step", [&]() -> int { return lm_group_enqueue(g, n, nsp_bucket, st); })) != RCA_OK) return rc;
        RCA_HIP(hipGraphLaunch(gexec, st));
    } else if ((rc = lm_group_enqueue(g, n, nsp, st)) != RCA_OK) {
        return rc;
    }
    RCA_HIP(hipStreamSynchronize(st));
    for (int s = 0; s < NM; ++s) {
        rca_lm* h = g->m[s];
        h->n_tokens += n;
        h->logits_rows = 1;
        h->rng_host += 1;
        tokens[s] = g->pin->tokens[s];
    }
    return RCA_OK;
}

// ------------------------------------------------------------------------------------ batch eval (rca_lm_batch_eval)
// rca_lm_eval_async for several sessions over ONE set of weights in one pass of the 128-token tiles: the prompt tokens of up to 64
// handles are packed into the activation buffers of a WORKSPACE handle (one more rca_lm_create_shared twin, whose cache, n_tokens and
// logits the call never touches) and run on its stream, so every matrix is streamed once per pass, not once per handle.
// Packing: a handle's tokens of the pass are one SEGMENT, and every segment starts on a multiple of 32 rows: no flash tile (8 / 16 / 32
// tokens) and no 32-row group of the k-split epilogue spans two handles.  The rows between a segment's last token and the next
// multiple of 32 are pad rows: they run through the row-wise stages and the GEMMs like any row (a GEMM row depends on its own input
// row only), their table entry has a context bound of 0, so the QKV epilogue stores nothing for them, and no attention tile owns them.
// Why a handle ends with the bits of its own rca_lm_eval_async: the row-wise stages and the GEMMs do not know which pass a row is in
// (the k-split form changes no bit: g128_form), the QKV epilogue and the q8_0 quantiser take position and cache per row / segment, and
// a query row of the flash kernel depends on its own position only.  How the host cuts the work into passes is free for the same reason.
#define LM_EVAL_MAXH 64
#define LM_EVAL_SEGS (LM_MAXM / 32)
// the block one pass uploads (its head: everything in front of the row table, then one row entry per padded row of the pass)
struct LmEvalStage {
    int rows, n_seg;                              // padded rows of the pass; its segments
    int pos0[LM_EVAL_SEGS], cnt[LM_EVAL_SEGS];    // a segment's first KV position and token count
    int owner[LM_EVAL_SEGS];                      // rows 32 i .. 32 i + 31 -> segment, -1 behind the pass
    int ids[LM_MAXM];                             // a pad row carries id 0
    LmBatchMember tab[LM_EVAL_SEGS];
    LmGroupRow head[2 * LM_EVAL_SEGS];            // want_logits: the rows of the grouped head launches (2 or 4 entries per launch)
    LmGroupRow rowtab[LM_MAXM];
};
struct LmEvalSeg { int k, done, cnt, row0; };     // handle index, tokens of it evaluated before this pass, tokens in it, first row
// the pass's state (into the workspace's LmDevState) and every segment's own step state, as lm_push_state would leave it
__global__ __launch_bounds__(LM_MAXM) void lm_eval_stage_kernel(const LmEvalStage* __restrict__ in, LmDevState* __restrict__ pstt) {
    const int t = threadIdx.x, rows = in->rows;
    if (t == 0) { pstt->n_tokens = 0; pstt->m = rows; }
    if (t >= rows) return;
    pstt->ids[t] = in->ids[t];
    const int seg = in->owner[t >> 5];
    if (seg < 0) return;
    LmDevState* stt = in->tab[seg].stt;
    const int j = t - in->tab[seg].row0;
    if (j == 0) { stt->n_tokens = in->pos0[seg]; stt->m = in->cnt[seg]; }
    if (j < in->cnt[seg]) stt->ids[j] = in->ids[t];
}
// one pass: fill the pinned block, upload, stage, the layers, and the head of every handle whose last token is in this pass
static int lm_eval_pass(rca_lm* ws, rca_lm* const* hs, const int32_t* const* ids_of, const int32_t* counts, const LmEvalSeg* segs, int n_seg, int rows,
                        bool want_logits, hipStream_t st) {
    LmEvalStage& in = *ws->be_pin;
    memset(&in, 0, offsetof(LmEvalStage, rowtab));
    in.rows = rows;
    in.n_seg = n_seg;
    for (int i = 0; i < LM_EVAL_SEGS; ++i) in.owner[i] = -1;
    int n_fin = 0;
    LmGroupRow fin[LM_EVAL_SEGS];   // the last rows of the handles that end in this pass ...
    rca_lm* fin_h[LM_EVAL_SEGS];    // ... and those handles
    for (int s = 0; s < n_seg; ++s) {
        const LmEvalSeg& sg = segs[s];
        rca_lm* h = hs[sg.k];
        const int pad = (sg.cnt + 31) & ~31;
        in.pos0[s] = h->n_tokens + sg.done;
        in.cnt[s] = sg.cnt;
        in.tab[s] = lm_batch_member(h, sg.row0, false);
        for (int r = sg.row0; r < sg.row0 + pad; r += 32) in.owner[r >> 5] = s;
        for (int j = 0; j < pad; ++j) {
            const int r = sg.row0 + j;
            if (j < sg.cnt) {
                in.ids[r] = ids_of[sg.k][sg.done + j];
                in.rowtab[r] = lm_group_row(h, j, r);
            } else {   // a pad row: position 0 of a context of 0 -- the epilogue stores nothing
                in.rowtab[r] = LmGroupRow{ws->stt, nullptr, nullptr, nullptr, 0, 0, r, 0, 0};
            }
        }
        if (want_logits && sg.done + sg.cnt == counts[sg.k]) {   // its last token: row of x, its own logits buffer
            fin[n_fin] = lm_group_row(h, sg.cnt - 1, sg.row0 + sg.cnt - 1);
            fin_h[n_fin++] = h;
        }
    }
    // head launches of 2 or 4 rows: up to LM_GROUP_MAX consecutive handles of one activation format (the head GEMV of a handle's own eval
    // reads that handle's); a short launch repeats its last row -- same row of x, same destination, same values
    int n_head = 0, n_launch = 0, head_at[LM_EVAL_SEGS], head_m[LM_EVAL_SEGS];
    rca_lm* launch_h[LM_EVAL_SEGS];
    for (int i = 0; i < n_fin;) {
        int real = 1;
        while (real < LM_GROUP_MAX && i + real < n_fin && fin_h[i + real]->act_format == fin_h[i]->act_format) ++real;
        const int m = real <= 2 ? 2 : 4;
        head_at[n_launch] = n_head;
        head_m[n_launch] = m;
        launch_h[n_launch++] = fin_h[i];
        for (int j = 0; j < m; ++j) in.head[n_head++] = fin[i + std::min(j, real - 1)];
        i += real;
    }
    // upload -> stage -> the layers, launched at the geometry of the pass's whole token blocks (the kernels read the row count from the
    // state): one sequence for every packing of tbz blocks, captured when the geometry is seen a second time and replayed from then
    // on.  The upload sits inside it and everything per session comes from the uploaded block: the graph holds the workspace's
    // pointers only, and goes when the workspace drops its graphs (lm_drop_graphs).
    const int tbz = cdiv(rows, 128), q8 = lm_kv_q8(hs[segs[0].k]) ? 1 : 0;
    const size_t up = offsetof(LmEvalStage, rowtab) + (size_t)tbz * 128 * sizeof(LmGroupRow);
    const LmEvalTables bt{ws->be_dev->rowtab, ws->be_dev->tab, ws->be_dev->owner, q8 != 0};
    auto layers = [&]() -> int {
        hipError_t e = hipMemcpyAsync(ws->be_dev, ws->be_pin, up, hipMemcpyHostToDevice, st);
        if (e != hipSuccess) return fail(RCA_ERR_HIP, "batch_eval upload: %s", hipGetErrorString(e));
        lm_eval_stage_kernel<<<1, LM_MAXM, 0, st>>>(ws->be_dev, ws->stt);
        return lm_enqueue_prefill_tile128(ws, tbz * 128, st, 1, &bt);
    };
    int rc;
    if (ws->graphs_enabled && lm_env_tile_graphs() &&++ws->be_seen[tbz - 1][q8] >= 2) {
        hipGraphExec_t& g = ws->be_g[tbz - 1][q8];
        if (!g && (rc = lm_capture(st, &g, "batch eval", layers)) != RCA_OK) return rc;
        RCA_HIP(hipGraphLaunch(g, st));
    } else if ((rc = layers()) != RCA_OK) {
        return rc;
    }
    // the heads run behind it, eagerly: which handles end in a pass is not part of its geometry
    const rca_lm_config_t& c = ws->cfg;
    for (int i = 0; i < n_launch; ++i)   // final norm + head on the register GEMV, up to four handles per stream of the head matrix
        launch_gemv<1, 0, 1>(GEMV_HEAD, launch_h[i], head_m[i], ws->head, nullptr, nullptr, c.vocab_size, c.hidden, c.vocab_size,
                             GemvPro{ws->x, ws->final_norm, c.rms_eps, 1}, norope, st, GemvGroup{ws->be_dev->head + head_at[i], 0});
    RCA_LAUNCH_CHECK();
    return RCA_OK;
}
extern "C" int rca_lm_batch_eval(rca_lm_t* ws, rca_lm_t* const* hs, int32_t n_h, const int32_t* ids, const int32_t* counts, int32_t want_logits) {
    if (!ws || !hs || !ids || !counts) return fail(RCA_ERR_ARG, "batch_eval: null argument");
    if (n_h < 1 || n_h > LM_EVAL_MAXH) return fail(RCA_ERR_ARG, "batch_eval: %d handles (1..%d)", n_h, LM_EVAL_MAXH);
    if (!lm_env_flash()) return fail(RCA_ERR_STATE, "batch_eval: RCA_LM_FLASH=0 asks for the split-attention prefill, which has no table form; use rca_lm_eval_async");
    if (lm_prefill_route(ws) != LM_ROUTE_TILE128)
        return fail(RCA_ERR_ARG, "batch_eval: the workspace does not take the 128-token tiles (rca_lm_prefill_route %d, the call needs 2)", lm_prefill_route(ws));
    // every refusal before anything is staged or enqueued: no handle changes
    const int32_t* ids_of[LM_EVAL_MAXH];
    long off = 0;
    for (int k = 0; k < n_h; ++k) {
        const rca_lm* h = hs[k];
        if (!h) return fail(RCA_ERR_ARG, "batch_eval: handle %d is null", k);
        if (h == ws) return fail(RCA_ERR_ARG, "batch_eval: handle %d is the workspace", k);
        for (int t = 0; t < k; ++t)
            if (hs[t] == h) return fail(RCA_ERR_ARG, "batch_eval: handle %d is the same handle as handle %d", k, t);
        if (h->device != ws->device) return fail(RCA_ERR_ARG, "batch_eval: handle %d is on device %d, the workspace on device %d", k, h->device, ws->device);
        if (lm_weight_owner(h) != lm_weight_owner(ws))
            return fail(RCA_ERR_ARG, "batch_eval: handle %d does not share the workspace's weights (rca_lm_create_shared makes handles that do)", k);
        if (h->cfg.logits_all) return fail(RCA_ERR_ARG, "batch_eval: handle %d is a logits_all handle (the call keeps the last position's logits only)", k);
        if (lm_prefill_route(h) != LM_ROUTE_TILE128)
            return fail(RCA_ERR_ARG, "batch_eval: handle %d does not take the 128-token tiles (rca_lm_prefill_route %d, the call needs 2); such models keep rca_lm_eval_async",
                        k, lm_prefill_route(h));
        if (h->kv_format != hs[0]->kv_format) return fail(RCA_ERR_ARG, "batch_eval: handle %d has KV format %d, handle 0 has %d", k, h->kv_format, hs[0]->kv_format);
        if (counts[k] < 1) return fail(RCA_ERR_ARG, "batch_eval: handle %d has %d tokens (at least 1)", k, counts[k]);
        if (h->n_tokens + counts[k] > h->cfg.n_ctx)
            return fail(RCA_ERR_STATE, "batch_eval: context overflow of handle %d: %d + %d > n_ctx %d", k, h->n_tokens, counts[k], h->cfg.n_ctx);
        ids_of[k] = ids + off;
        for (int j = 0; j < counts[k]; ++j)
            if (ids_of[k][j] < 0 || ids_of[k][j] >= h->cfg.vocab_size)
                return fail(RCA_ERR_ARG, "batch_eval: token id %d of handle %d at index %d is outside the vocabulary [0, %d)", ids_of[k][j], k, j, h->cfg.vocab_size);
        off += counts[k];
    }
    int rc;
    if ((rc = lm_settle(ws)) != RCA_OK) return rc;
    for (int k = 0; k < n_h; ++k)
        if ((rc = lm_settle(hs[k])) != RCA_OK) return rc;
    RCA_HIP(hipSetDevice(ws->device));
    if (!ws->be_dev && (rc = lm_alloc((void**)&ws->be_dev, sizeof(LmEvalStage))) != RCA_OK) return rc;
    if (!ws->be_pin && hipHostMalloc((void**)&ws->be_pin, sizeof(LmEvalStage), hipHostMallocDefault) != hipSuccess) return fail(RCA_ERR_HIP, "batch_eval: pinned staging");
    for (int k = 0; k < n_h; ++k)
        if (!hs[k]->be_event) RCA_HIP(hipEventCreateWithFlags(&hs[k]->be_event, hipEventDisableTiming));
    hipStream_t st = ws->stream;
    // greedy cut into passes of up to LM_MAXM rows and LM_EVAL_SEGS segments; a handle's tokens may continue in the next pass
    LmEvalSeg segs[LM_EVAL_SEGS];
    int n_seg = 0, rows = 0, n_pass = 0;
    auto flush = [&]() -> int {
        if (n_pass++) RCA_HIP(hipStreamSynchronize(st));   // the pinned block is reused: the pass before has consumed its copy
        const int r = lm_eval_pass(ws, hs, ids_of, counts, segs, n_seg, rows, want_logits != 0, st);
        n_seg = rows = 0;
        return r;
    };
    for (int k = 0; k < n_h; ++k) {
        for (int done = 0; done < counts[k];) {
            if (rows == LM_MAXM || n_seg == LM_EVAL_SEGS) { if ((rc = flush()) != RCA_OK) return rc; }
            const int take = std::min(counts[k] - done, LM_MAXM - rows);
            segs[n_seg++] = LmEvalSeg{k, done, take, rows};
            rows += (take + 31) & ~31;
            done += take;
        }
    }
    if ((rc = flush()) != RCA_OK) return rc;
    for (int k = 0; k < n_h; ++k) {   // behind the last pass: what a later call on the handle waits for
        rca_lm* h = hs[k];
        RCA_HIP(hipEventRecord(h->be_event, st));
        h->be_pending = true;
        h->n_tokens += counts[k];
        h->logits_rows = want_logits ? 1 : 0;
    }
    ws->async_pending = true;
    return RCA_OK;
}

// ------------------------------------------------------------------------------------ batch step (rca_lm_batch_step)
// 2 to 64 sessions over ONE set of weights advance by n = 1 or 2 tokens each as ONE token block of the 128-token MFMA tiles: the
// n_members * n rows are a small GEMM, not a GEMV, so a matrix is staged (and de-quantised) once for all of them and the cost of a
// step grows slowly with the members.  The layers are lm_enqueue_layers128, the prefill tile's own -- RMSNorm +
// hi / lo split, O, gate / up + SwiGLU, down, with the same k-split forms (functions of the matrix only) -- driven by a batch-owned
// LmDevState whose m is the row count.  What is per session comes from tables: the QKV epilogue (GEMM_EPI_ROPE_ROWS) takes a row's
// position and cache from an LmGroupRow, the decode attention (split kernel + separate combine, never the in-launch merge) and the
// serial sampler chain take a member per grid z / y from an LmBatchMember.  The head is one tile GEMM over the members' last rows
// into a batch-owned block, then a row copy into every member's own logits buffer.  Arithmetic class: tile GEMMs (f32 activations
// as bf16 hi + lo) and decode attention, i.e. what a decode step on a tile-built cache sees -- not the GEMV steps' bits, so no
// bit-for-bit promise against rca_lm_step; a row's result does not depend on its slot or its companions.
#define LM_BATCH_MAX 64
#define LM_BATCH_ROWS 128   // one token block
// One staging block serves every call; each struct below is the head of the next, and a call uploads the head it needs.
// A step: the live count (the members of the pass, in slots 0 .. n_live - 1), their positions and their ids.
struct LmBatchStage { int n_live; int n_tokens[LM_BATCH_MAX]; int ids[LM_BATCH_ROWS]; };
// A frame: the step's block (the first pairs in ids), then the user's token of every step and the probe id of every member
struct LmBatchFrameStage : LmBatchStage { int user[LM_BATCH_MAX * LM_FRAME_MAX]; int probe[LM_BATCH_MAX]; };
struct LmBatchFrameOut { int tokens[LM_BATCH_MAX * LM_FRAME_MAX]; float probs[LM_BATCH_MAX]; };
// A selection (rca_lm_batch_frame_sel, rca_duplex_batch_frame): the frame's block over the SELECTED members, and the two tables of
// exactly those slots, composed on the host for every call and uploaded as one block inside the replay: a graph over them holds no
// member's pointer
#define LM_BATCH_CLASSES 4   // launch geometries: 8, 16, 32 or 64 slots
struct LmBatchSelStage : LmBatchFrameStage { LmBatchMember tab[LM_BATCH_MAX]; LmGroupRow rows[LM_BATCH_ROWS]; };
// rca_lm_batch_step_sel: the selection's block with the step's probe ids behind it (a frame uploads the LmBatchSelStage head only), and
// what a step gathers for its one download (rca_lm_batch_step: the tokens only)
#define LM_STEP_PROBES 8
struct LmBatchStepSelStage : LmBatchSelStage { int n_probe; int pad2; int probe_ids[LM_BATCH_MAX * LM_STEP_PROBES]; };   // probe_ids[k * n_probe + i]
struct LmBatchStepSelOut { int tokens[LM_BATCH_MAX]; float probs[LM_BATCH_MAX * LM_STEP_PROBES]; };                    // probs[k * n_probe + i]
// what a pass reads about its members: the batch's own tables, or a selection's
struct LmBatchView { const LmGroupRow* rows; const LmBatchMember* tab; int NM; bool any_serial, any_patch; rca_lm* const* hm; int n_hm; };
struct rca_lm_batch {
    int n_members = 0;
    rca_lm* m[LM_BATCH_MAX] = {};
    LmGroupRow* rows = nullptr;       // device, [LM_GEMV_M][LM_BATCH_ROWS]: (member s, token j) -> row s * n + j
    LmBatchMember* tab = nullptr;     // device, [LM_GEMV_M][LM_BATCH_MAX]
    bool tabs_valid = false;
    unsigned long long epoch[LM_BATCH_MAX] = {};   // the members' graph epochs the tables and graphs below were made under
    bool any_serial = false, any_patch = false;    // the table sampler chain has members / some of them patch their logits
    LmDevState* stt = nullptr;        // device: the pass over all rows (m = n_members * n, the rows' ids)
    LmDevState* stt_head = nullptr;   // device: the head's pass (m = n_members)
    float* head_blk = nullptr;        // device, [n_members][V]: the head GEMM's block
    LmBatchStepSelStage* sel_stage = nullptr;   // device copy of sel_pin (a call uploads the head it needs)
    LmBatchStepSelStage* sel_pin = nullptr;     // pinned: every call's staging block
    hipGraphExec_t g[LM_GEMV_M][LM_GRAPH_BUCKETS] = {};   // (n, largest context bucket among the members)
    // the frames
    LmBatchFrameOut* frame_out = nullptr;   // device: every step's tokens and the probes, gathered for one download
    LmBatchFrameOut* frame_pin = nullptr;   // pinned
    float* probe_part = nullptr;            // device, [n_members][PROBS_SLICES (max, sum) pairs]
    hipGraphExec_t fg[LM_FRAME_MAX][LM_GRAPH_BUCKETS][2] = {};   // (n_steps - 1, largest context bucket at the frame's end, probes)
    // rca_lm_batch_frame_sel
    int nsp_all = 1;                        // the largest split count among ALL members: a graph's attention grid
    unsigned long long sel_epoch = 0;       // sum of the members' drop_epoch the graphs below were captured under
    hipGraphExec_t sg[LM_BATCH_CLASSES][LM_FRAME_MAX][LM_GRAPH_BUCKETS][2][2] = {};   // (class, n_steps - 1, bucket, probes, a patching sampler among them)
    long long n_captures = 0;               // rca_lm_batch_captures
    struct LmBatchDuplex* dx = nullptr;     // rca_duplex_batch_frame: buffers, pinned staging and graphs (made by its first call)
    // the steps
    LmBatchStepSelOut* step_out = nullptr;      // device: the members' tokens and probe probabilities, gathered for one download
    LmBatchStepSelOut* step_out_pin = nullptr;  // pinned
    hipGraphExec_t ssg[LM_BATCH_CLASSES][LM_GEMV_M][LM_GRAPH_BUCKETS][2][2] = {};   // (class, n - 1, bucket, probes, a patching sampler among them)
};
// the pass's state and the members' step states from the staging block, for n tokens per member; `tab` is the table of the pass (the
// batch's own, or the block's).  The live count comes from the block, not the launch: a graph serves every selection of its class.
__global__ void lm_batch_stage_kernel(const LmBatchStage* __restrict__ in, const LmBatchMember* __restrict__ tab, LmDevState* __restrict__ bstt,
                                      LmDevState* __restrict__ hstt, int n) {
    const int t = threadIdx.x, n_members = in->n_live;
    if (t == 0) { bstt->n_tokens = 0; bstt->m = n_members * n; hstt->n_tokens = 0; hstt->m = n_members; }
    if (t < n_members * n) bstt->ids[t] = in->ids[t];
    if (t < n_members) {
        LmDevState* stt = tab[t].stt;
        stt->n_tokens = in->n_tokens[t];
        stt->m = n;
        for (int j = 0; j < n; ++j) stt->ids[j] = in->ids[t * n + j];
    }
}
// n = 2: the members' last rows of x, packed for the head's RMSNorm
__global__ __launch_bounds__(256) void lm_batch_last_rows_kernel(const float* __restrict__ x, float* __restrict__ out, int n, int H) {
    const float* src = x + ((long)blockIdx.x * n + n - 1) * H;
    for (int h = threadIdx.x; h < H; h += 256) out[(long)blockIdx.x * H + h] = src[h];
}
// the head block's rows -> the members' own logits buffers
__global__ __launch_bounds__(256) void lm_batch_logits_rows_kernel(const LmBatchMember* __restrict__ tab, const float* __restrict__ blk, int V) {
    float* dst = tab[blockIdx.y].logits;
    if (!dst) return;   // a slot past a selection's live count
    const float* src = blk + (long)blockIdx.y * V;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < V; i += gridDim.x * 256) dst[i] = src[i];
}
// the serial sampler chain with the member in grid y: the bodies of samp_prepare / hist / gather / final_kernel on the member's own
// {logits, SamplerDev, LmDevState, SampWork}.  Members on a whole-vocabulary sampler are skipped here (their own launches follow),
// and so is a slot past a selection's live count: its all-zero entry is not serial.
__global__ __launch_bounds__(128) void samp_prepare_batch_kernel(const LmBatchMember* __restrict__ tab, int V) {
    const LmBatchMember e = tab[blockIdx.y];
    if (!e.serial || !e.samp->patch) return;
    samp_prepare_body(e.logits, V, e.samp, e.stt, e.swork);
}
__global__ __launch_bounds__(256) void samp_hist_batch_kernel(const LmBatchMember* __restrict__ tab, int V) {
    const LmBatchMember e = tab[blockIdx.y];
    if (!e.serial) return;
    samp_hist_body(e.logits, V, e.samp, e.swork);
}
__global__ __launch_bounds__(256) void samp_gather_batch_kernel(const LmBatchMember* __restrict__ tab, int V) {
    const LmBatchMember e = tab[blockIdx.y];
    if (!e.serial) return;
    samp_gather_body(e.logits, V, e.samp, e.swork);
}
__global__ __launch_bounds__(1024) void samp_final_batch_kernel(const LmBatchMember* __restrict__ tab, int V) {
    const LmBatchMember e = tab[blockIdx.y];
    if (!e.serial) return;
    samp_final_body<false>(e.logits, V, e.samp, e.stt, e.swork, SampTail{-1, nullptr, 0, nullptr, 0});
}
__global__ void lm_batch_tokens_kernel(const LmBatchMember* __restrict__ tab, int n_members, int* __restrict__ out) {
    if ((int)threadIdx.x < n_members && tab[threadIdx.x].stt) out[threadIdx.x] = tab[threadIdx.x].stt->out_token;
}
// rca_lm_batch_frame, behind the samplers of step `step`: what the SampTail feedback does for one handle, for all members at once.
// Records the token, advances the member's position past the pair just evaluated and makes [token, user's token of this step] the
// next pair -- in the member's own step state (attention, RoPE rows and its sampler read it) and in the pass's id list (the
// embedding gather reads that one).
__global__ void lm_batch_feedback_kernel(const LmBatchFrameStage* __restrict__ in, const LmBatchMember* __restrict__ tab, LmDevState* __restrict__ bstt,
                                         LmBatchFrameOut* __restrict__ out, int n_members, int step) {
    const int t = threadIdx.x;
    if (t >= n_members) return;
    LmDevState* stt = tab[t].stt;
    if (!stt) return;   // a slot past a selection's live count
    const int tok = stt->out_token, user = in->user[t * LM_FRAME_MAX + step];
    out->tokens[t * LM_FRAME_MAX + step] = tok;
    stt->n_tokens += 2;
    stt->ids[0] = tok;
    stt->ids[1] = user;
    bstt->ids[2 * t] = tok;
    bstt->ids[2 * t + 1] = user;
}
// softmax(member's logits)[its probe id]: lm_softmax_slices_kernel / lm_token_probs_kernel with the member in grid y
__global__ __launch_bounds__(1024) void lm_softmax_slices_batch_kernel(const LmBatchMember* __restrict__ tab, int V, float* __restrict__ part) {
    if (!tab[blockIdx.y].logits) return;   // a slot past a selection's live count
    lm_softmax_slices_body(tab[blockIdx.y].logits, V, part + (long)blockIdx.y * 2 * PROBS_SLICES);
}
__global__ __launch_bounds__(64) void lm_token_probs_batch_kernel(const LmBatchMember* __restrict__ tab, int V, const float* __restrict__ part,
                                                                  const int* __restrict__ ids, float* __restrict__ probs) {
    const int s = blockIdx.y;
    if (!tab[s].logits) return;
    lm_token_probs_body(tab[s].logits, V, part + (long)s * 2 * PROBS_SLICES, ids + s, 1, probs + s);
}
// rca_lm_batch_step_sel: softmax(slot's logits)[its n_probe ids]; the count and the ids come from the uploaded block, not the launch
__global__ __launch_bounds__(64) void lm_token_probs_sel_kernel(const LmBatchMember* __restrict__ tab, int V, const float* __restrict__ part,
                                                                const LmBatchStepSelStage* __restrict__ in, float* __restrict__ probs) {
    const int s = blockIdx.y, np = in->n_probe;
    if (!tab[s].logits) return;   // a slot past the selection's live count
    lm_token_probs_body(tab[s].logits, V, part + (long)s * 2 * PROBS_SLICES, in->probe_ids + s * np, np, probs + s * np);
}
// a frame drew n_steps times for every member: the counters of the members it cut go back to where their accepted draws end
struct LmBatchCuts { int n; int member[LM_BATCH_MAX]; unsigned long long counter[LM_BATCH_MAX]; };
__global__ void lm_batch_counters_kernel(const LmBatchMember* __restrict__ tab, LmBatchCuts cuts) {
    if ((int)threadIdx.x < cuts.n) tab[cuts.member[threadIdx.x]].stt->rng_counter = cuts.counter[threadIdx.x];
}
static void lm_batch_drop_graphs(rca_lm_batch* b) {
    for (auto& per_n : b->g)
        for (hipGraphExec_t& e : per_n)
            if (e) { (void)hipGraphExecDestroy(e); e = nullptr; }
    for (auto& per_n : b->fg)
        for (auto& per_b : per_n)
            for (hipGraphExec_t& e : per_b)
                if (e) { (void)hipGraphExecDestroy(e); e = nullptr; }
}
static void lm_batch_drop_sel_graphs(rca_lm_batch* b) {
    hipGraphExec_t* e = &b->sg[0][0][0][0][0];
    for (size_t i = 0; i < sizeof(b->sg) / sizeof(hipGraphExec_t); ++i)
        if (e[i]) { (void)hipGraphExecDestroy(e[i]); e[i] = nullptr; }
    e = &b->ssg[0][0][0][0][0];   // rca_lm_batch_step_sel's
    for (size_t i = 0; i < sizeof(b->ssg) / sizeof(hipGraphExec_t); ++i)
        if (e[i]) { (void)hipGraphExecDestroy(e[i]); e[i] = nullptr; }
}
// the launch geometry of n slots: 8, 16, 32 or 64
static int lm_batch_class(int n) { return n <= 8 ? 0 : n <= 16 ? 1 : n <= 32 ? 2 : 3; }
static void lm_batch_duplex_destroy(struct LmBatchDuplex* d);
static void lm_batch_duplex_drop_graphs(struct LmBatchDuplex* d);
extern "C" int rca_lm_batch_destroy(rca_lm_batch_t* b);
extern "C" int rca_lm_batch_create(rca_lm_t* const* members, int32_t n_members, rca_lm_batch_t** out) {
    if (!members || !out) return fail(RCA_ERR_ARG, "batch_create: null argument");
    if (n_members < 2 || n_members > LM_BATCH_MAX) return fail(RCA_ERR_ARG, "batch_create: %d members, a batch has 2 to %d", n_members, LM_BATCH_MAX);
    for (int s = 0; s < n_members; ++s) {
        const rca_lm* h = members[s];
        if (!h) return fail(RCA_ERR_ARG, "batch_create: member %d is null", s);
        for (int t = 0; t < s; ++t)
            if (members[t] == h) return fail(RCA_ERR_ARG, "batch_create: member %d is the same handle as member %d", s, t);
        if (h->device != members[0]->device) return fail(RCA_ERR_ARG, "batch_create: member %d is on device %d, member 0 on device %d", s, h->device, members[0]->device);
        if (lm_weight_owner(h) != lm_weight_owner(members[0]))
            return fail(RCA_ERR_ARG, "batch_create: member %d does not share member 0's weights (rca_lm_create_shared makes handles that do)", s);
        if (h->kv_format != members[0]->kv_format)
            return fail(RCA_ERR_ARG, "batch_create: member %d has KV format %d, member 0 has %d", s, h->kv_format, members[0]->kv_format);
        if (h->cfg.logits_all) return fail(RCA_ERR_ARG, "batch_create: member %d is a logits_all handle (a batch step keeps the last position's logits only)", s);
        if (lm_prefill_route(h) != LM_ROUTE_TILE128)
            return fail(RCA_ERR_ARG, "batch_create: member %d does not take the 128-token tiles (rca_lm_prefill_route %d, a batch step needs 2); such models stay with rca_lm_group_step",
                        s, lm_prefill_route(h));
    }
    RCA_HIP(hipSetDevice(members[0]->device));
    rca_lm_batch* b = new rca_lm_batch();
    b->n_members = n_members;
    for (int s = 0; s < n_members; ++s) b->m[s] = members[s];
    int rc = lm_alloc((void**)&b->rows, sizeof(LmGroupRow) * LM_GEMV_M * LM_BATCH_ROWS);
    if (rc == RCA_OK) rc = lm_alloc((void**)&b->tab, sizeof(LmBatchMember) * LM_GEMV_M * LM_BATCH_MAX);
    if (rc == RCA_OK) rc = lm_alloc((void**)&b->stt, sizeof(LmDevState));
    if (rc == RCA_OK) rc = lm_alloc((void**)&b->stt_head, sizeof(LmDevState));
    const int n_slots = 8 << lm_batch_class(n_members);   // a selection frame launches at its class's slot count
    if (rc == RCA_OK) rc = lm_alloc((void**)&b->head_blk, (size_t)n_slots * members[0]->cfg.vocab_size * 4);
    if (rc == RCA_OK) rc = lm_alloc((void**)&b->frame_out, sizeof(LmBatchFrameOut));
    if (rc == RCA_OK && hipHostMalloc((void**)&b->frame_pin, sizeof(LmBatchFrameOut), hipHostMallocDefault) != hipSuccess) rc = fail(RCA_ERR_HIP, "batch_create: pinned staging");
    if (rc == RCA_OK) rc = lm_alloc((void**)&b->probe_part, sizeof(float) * 2 * PROBS_SLICES * n_slots);
    if (rc == RCA_OK) rc = lm_alloc((void**)&b->sel_stage, sizeof(LmBatchStepSelStage));
    if (rc == RCA_OK && hipHostMalloc((void**)&b->sel_pin, sizeof(LmBatchStepSelStage), hipHostMallocDefault) != hipSuccess) rc = fail(RCA_ERR_HIP, "batch_create: pinned staging");
    if (rc == RCA_OK) rc = lm_alloc((void**)&b->step_out, sizeof(LmBatchStepSelOut));
    if (rc == RCA_OK && hipHostMalloc((void**)&b->step_out_pin, sizeof(LmBatchStepSelOut), hipHostMallocDefault) != hipSuccess) rc = fail(RCA_ERR_HIP, "batch_create: pinned staging");
    if (rc == RCA_OK && (hipMemset(b->stt, 0, sizeof(LmDevState)) != hipSuccess || hipMemset(b->stt_head, 0, sizeof(LmDevState)) != hipSuccess))
        rc = fail(RCA_ERR_HIP, "batch_create: clearing the pass states");
    if (rc != RCA_OK) { rca_lm_batch_destroy(b); return rc; }
    memset(b->sel_pin, 0, sizeof(LmBatchStepSelStage));
    for (int s = 0; s < n_members; ++s) b->nsp_all = std::max(b->nsp_all, members[s]->n_splits);
    *out = b;
    return RCA_OK;
}
extern "C" int rca_lm_batch_destroy(rca_lm_batch_t* b) {
    if (!b) return RCA_OK;
    lm_batch_drop_graphs(b);
    lm_batch_drop_sel_graphs(b);
    lm_batch_duplex_destroy(b->dx);
    for (void* p : {(void*)b->rows, (void*)b->tab, (void*)b->stt, (void*)b->stt_head, (void*)b->head_blk, (void*)b->frame_out, (void*)b->probe_part,
                    (void*)b->sel_stage, (void*)b->step_out})
        if (p) (void)hipFree(p);
    if (b->frame_pin) (void)hipHostFree(b->frame_pin);
    if (b->sel_pin) (void)hipHostFree(b->sel_pin);
    if (b->step_out_pin) (void)hipHostFree(b->step_out_pin);
    delete b;
    return RCA_OK;
}
// tables + graphs follow the members: a swapped cache, a moved logits buffer or another sampler chain shows as a new epoch
static int lm_batch_refresh(rca_lm_batch* b) {
    bool same = b->tabs_valid;
    for (int s = 0; s < b->n_members; ++s) same = same && b->epoch[s] == b->m[s]->graph_epoch;
    if (same) return RCA_OK;
    lm_batch_drop_graphs(b);
    std::vector<LmGroupRow> rows((size_t)LM_GEMV_M * LM_BATCH_ROWS);
    std::vector<LmBatchMember> tab((size_t)LM_GEMV_M * LM_BATCH_MAX);
    memset(rows.data(), 0, rows.size() * sizeof(LmGroupRow));
    memset(tab.data(), 0, tab.size() * sizeof(LmBatchMember));
    b->any_serial = b->any_patch = false;
    for (int n = 1; n <= LM_GEMV_M; ++n)
        for (int s = 0; s < b->n_members; ++s) {
            rca_lm* h = b->m[s];
            if (s * n + n > LM_BATCH_ROWS) break;   // (more rows than a token block: refused by the step before anything reads the table)
            const bool serial = h->sampler_set && !lm_samp_own_launches(h);
            tab[(size_t)(n - 1) * LM_BATCH_MAX + s] = lm_batch_member(h, s * n, serial);
            b->any_serial = b->any_serial || serial;
            b->any_patch = b->any_patch || (serial && h->samp_patch);
            for (int j = 0; j < n; ++j) {
                LmGroupRow r = lm_group_row(h, j, s * n + j);
                rows[(size_t)(n - 1) * LM_BATCH_ROWS + s * n + j] = r;
            }
        }
    RCA_HIP(hipMemcpy(b->rows, rows.data(), rows.size() * sizeof(LmGroupRow), hipMemcpyHostToDevice));
    RCA_HIP(hipMemcpy(b->tab, tab.data(), tab.size() * sizeof(LmBatchMember), hipMemcpyHostToDevice));
    for (int s = 0; s < b->n_members; ++s) b->epoch[s] = b->m[s]->graph_epoch;
    b->tabs_valid = true;
    return RCA_OK;
}
// The decode attention of layer l for every slot of a pass's table: the split kernel with a member per grid z over the q rows in
// member 0's qkv, then the merge into the members' rows of the bf16 hi / lo planes.  The pass's launches and rca_lm_batch_attn_tap's.
static void lm_batch_launch_attn(rca_lm* ws, const LmBatchMember* tab, int NM, int n, int nsp_launch, bool q8kv, int l, hipStream_t st) {
    const rca_lm_config_t& c = ws->cfg;
    lm_launch_attn_split(c, dim3(c.n_kv_heads, nsp_launch, NM), q8kv, st, nullptr, ws->qkv, nullptr, nullptr, 0, 0, nullptr, nullptr, nullptr, tab, l);
    lm_dispatch_421(c.n_heads / c.n_kv_heads, [&](auto g) {
        lm_attn_mfma_batch_combine_kernel<decltype(g)::value><<<dim3(n * c.n_heads, NM), 64, 0, st>>>(tab, c.n_heads, c.n_kv_heads, nsp_launch, ws->xh, ws->xl);
    });
}
// embedding -> the layers -> head -> samplers over the device states as they stand (staged by lm_batch_stage_kernel, or left by
// lm_batch_feedback_kernel): the part a step and every step of a frame share
static void lm_batch_enqueue_pass(rca_lm_batch* b, const LmBatchView& vw, int n, int nsp_launch, hipStream_t st) {
    rca_lm* ws = b->m[0];
    const rca_lm_config_t& c = ws->cfg;
    const int NM = vw.NM, MT = NM * n;
    const int H = c.hidden, V = c.vocab_size;
    const LmBatchMember* tab = vw.tab;
    lm_attn_split_attrs();
    const bool q8kv = lm_kv_q8(ws);   // every member's format (rca_lm_batch_create, lm_batch_check)
    float* x = ws->x;
    lm_embed_kernel<<<MT, 256, 0, st>>>(b->stt, ws->embed, ws->embed_f32, x, H, V);
    // one token block: the k-split forms are what an rca_lm_eval_async pass of up to 128 tokens uses, so a row's sums are that pass's
    lm_enqueue_layers128(LmTilePass{ws, b->stt, MT, 1, vw.rows, g128_seq_min()}, st, [&](int l) {
        if (q8kv)   // every member's new rows, ring -> int8 planes, in one launch
            lm_kv_quant_kernel<true><<<dim3(cdiv(4 * c.n_kv_heads, 8), n, NM), 256, 0, st>>>(nullptr, nullptr, nullptr, 0, nullptr, nullptr, nullptr, nullptr, c.n_kv_heads, 0, 0, 0, 3, tab, l);
        lm_batch_launch_attn(ws, tab, NM, n, nsp_launch, q8kv, l, st);
    });
    // final RMSNorm + head over the last row of every member (one row per member: rows 0 .. NM - 1 of the hi / lo planes), every
    // workgroup walking all of K like rca_lm_score's head; the ragged last row tile of the vocabulary is the logits epilogue's
    if (n > 1) lm_batch_last_rows_kernel<<<NM, 256, 0, st>>>(x, ws->xn, n, H);
    lm_add_rmsnorm_kernel<<<NM, 64, 0, st>>>(b->stt_head, n > 1 ? ws->xn : x, nullptr, nullptr, 0, 0, ws->final_norm, ws->xn, H, c.rms_eps, ws->xh, ws->xl);
    lm_launch_logits128(ws, b->stt_head, ws->xh, ws->xl, 0, b->head_blk, st);
    lm_batch_logits_rows_kernel<<<dim3(std::min((int)cdiv(V, 256), 64), NM), 256, 0, st>>>(tab, b->head_blk, V);
    if (vw.any_serial) {
        if (vw.any_patch) samp_prepare_batch_kernel<<<dim3(1, NM), 128, 0, st>>>(tab, V);
        samp_hist_batch_kernel<<<dim3(128, NM), 256, 0, st>>>(tab, V);
        samp_gather_batch_kernel<<<dim3(128, NM), 256, 0, st>>>(tab, V);
        samp_final_batch_kernel<<<dim3(1, NM), 1024, 0, st>>>(tab, V);
    }
    for (int s = 0; s < vw.n_hm; ++s)
        if (lm_samp_own_launches(vw.hm[s])) lm_enqueue_sample(vw.hm[s], vw.hm[s]->logits, st);
}
// the batch's own tables for n tokens per member, every member in its slot
static LmBatchView lm_batch_view(rca_lm_batch* b, int n) {
    return LmBatchView{b->rows + (size_t)(n - 1) * LM_BATCH_ROWS, b->tab + (size_t)(n - 1) * LM_BATCH_MAX, b->n_members, b->any_serial, b->any_patch, b->m, b->n_members};
}

// ------------------------------------------------------------------------------------ the batch calls' host sequence
// rca_lm_batch_step, _frame, _frame_sel, _step_sel and rca_duplex_batch_frame are one sequence on the host: describe the call
// (LmBatchCall) -> refuse (lm_batch_check) -> fill the pinned block and plan the launches (lm_batch_stage) -> capture / replay or run
// eagerly (lm_batch_run over lm_batch_enqueue) -> settle.  Two things differ between them.  Where a pass's tables come from: the
// batch's resident ones, every member in its own slot at exact n_members geometry, refreshed under the members' graph_epoch -- or the
// call's own block, the selected members in slots 0 .. n_sel - 1 at the geometry of the selection's class, the live count in the block.
// And what runs between upload and download: one pass of n tokens per member, or n_steps pairs with feedback; the codec tails of a
// duplex call go around either.
// (grows a device buffer of rca_duplex_frame / rca_duplex_batch_frame; the old contents are not kept)
template <class T>
static int duplex_grow(T** p, size_t* cap, size_t n) {
    if (n <= *cap) return RCA_OK;
    if (*p) { (void)hipFree(*p); *p = nullptr; *cap = 0; }
    int rc = lm_alloc((void**)p, n * sizeof(T));
    if (rc == RCA_OK) *cap = n;
    return rc;
}
// What rca_duplex_batch_frame adds around the selection frame's passes: buffers, pinned staging and graphs, owned by the batch.
struct LmBatchDuplexDev { long long user_codes[LM_BATCH_MAX * LM_FRAME_MAX]; int flags[LM_BATCH_MAX]; };   // [slot][step of the call]; one download
struct LmBatchDuplexKey {
    int cls, T, F_ctx, n_steps, n_samples, probes, bucket, base, patch;
    unsigned long long codec_sig;
    const void* codec;
    bool operator==(const LmBatchDuplexKey& o) const {
        return cls == o.cls && T == o.T && F_ctx == o.F_ctx && n_steps == o.n_steps && n_samples == o.n_samples && probes == o.probes && bucket == o.bucket &&
               base == o.base && patch == o.patch && codec_sig == o.codec_sig && codec == o.codec;
    }
};
struct LmBatchDuplex {
    float* pcm_in = nullptr; size_t pcm_in_cap = 0;           // device [slots][T]
    long long* code_win = nullptr; size_t code_win_cap = 0;   // device [slots][F_ctx + n]
    float* pcm_out = nullptr; size_t pcm_out_cap = 0;         // device [slots][n_samples]
    LmBatchDuplexDev* dev = nullptr;
    char* pin = nullptr; size_t pin_cap = 0;                  // pinned: [LmBatchDuplexDev | pcm windows | code contexts | pcm out]
    struct Entry { LmBatchDuplexKey key; hipGraphExec_t exec = nullptr; };
    std::vector<Entry> graphs;
    struct Warm { int cls, T, F_ctx, n_steps, n_samples; const void* codec; unsigned long long codec_sig; };
    std::vector<Warm> warm;   // (class, shape)s whose codec workspace an eager call has sized: a capture must not allocate
};
// one call's geometry, handed to the enqueue
struct LmBatchDuplexCall {
    rca_codec_t* codec;
    int slots, T, F_ctx, n_samples, base, n_codes;
    size_t pin_pcm, pin_codes, pin_out;   // byte offsets in LmBatchDuplex::pin
};
// codes -> ids, table form over [slot][step]: the user's ids of the frame's block, where lm_batch_feedback_kernel reads them, written by
// the device instead of the upload; clears the slots' flags
__global__ void duplex_batch_codes_to_ids_kernel(const long long* __restrict__ codes, int n, int base, LmBatchSelStage* __restrict__ stage,
                                                 int* __restrict__ flags) {
    const int k = blockIdx.x, i = threadIdx.x;
    if (k >= stage->n_live) return;
    if (i == 0) flags[k] = 0;
    if (i < n) stage->user[k * LM_FRAME_MAX + i] = base + (int)codes[(long)k * n + i];
}
// ids -> codes, table form: every live slot's sampled tokens of the frame go behind its row's context codes; a token that is no codec
// token becomes code 0 and raises the slot's flag bit 0
__global__ void duplex_batch_tokens_to_codes_kernel(const LmBatchFrameOut* __restrict__ out, const LmBatchSelStage* __restrict__ stage, int n, int base,
                                                    int n_codes, long long* __restrict__ code_win, int F, int* __restrict__ flags) {
    const int k = blockIdx.x, i = threadIdx.x;
    if (k >= stage->n_live || i >= n) return;
    const int c = out->tokens[k * LM_FRAME_MAX + i] - base;
    const bool ok = c >= 0 && c < n_codes;
    code_win[(long)k * F + (F - n) + i] = ok ? c : 0;
    if (!ok) atomicOr(&flags[k], 1);
}
static void lm_batch_duplex_drop_graphs(LmBatchDuplex* d) {
    if (!d) return;
    for (auto& e : d->graphs)
        if (e.exec) (void)hipGraphExecDestroy(e.exec);
    d->graphs.clear();
}
static void lm_batch_duplex_destroy(LmBatchDuplex* d) {
    if (!d) return;
    lm_batch_duplex_drop_graphs(d);
    for (void* p : {(void*)d->pcm_in, (void*)d->code_win, (void*)d->pcm_out, (void*)d->dev})
        if (p) (void)hipFree(p);
    if (d->pin) (void)hipHostFree(d->pin);
    delete d;
}

// what an entry point was asked to do
struct LmBatchCall {
    const char* who;            // the API's name in messages
    const int32_t* sel;         // the selected members; null: every member in its own slot, the batch's resident tables
    int n_sel;                  // the members of the pass (lm_batch_check: n_members where sel is null)
    int n;                      // tokens per member of a pass
    bool frame;                 // n_steps pairs with feedback; else a step, one pass of n tokens
    int n_steps;                // 0: a step
    const int32_t* ids;         // a step's [n_sel][n], a frame's first pairs
    const int32_t* user_ids;    // a frame's [n_sel][n_steps]; null: the device makes them (rca_duplex_batch_frame)
    const int32_t* probe_ids;   // [n_sel][n_probe]; a frame has one per member, -1 for none
    int n_probe;
    rca_lm* hm[LM_BATCH_MAX];   // the handle of every slot (lm_batch_check)
};
// Every refusal of the five calls, before anything is staged or enqueued: no member changes.  Fills n_sel (without a selection) and
// hm[], and settles the members of the pass.
static int lm_batch_check(rca_lm_batch* b, LmBatchCall& c) {
    const int NM = b->n_members, n = c.n;
    if (c.sel && (c.n_sel < 1 || c.n_sel > NM)) return fail(RCA_ERR_ARG, "%s: %d selected members, the batch has %d (1..%d)", c.who, c.n_sel, NM, NM);
    if (c.frame && (c.n_steps < 1 || c.n_steps > LM_FRAME_MAX)) return fail(RCA_ERR_ARG, "%s: %d steps (1..%d)", c.who, c.n_steps, LM_FRAME_MAX);
    if (!c.sel) {
        if (NM * n > LM_BATCH_ROWS) return fail(RCA_ERR_ARG, "%s: %d members x %d tokens = %d rows, a batch pass is one token block of %d", c.who, NM, n, NM * n, LM_BATCH_ROWS);
        c.n_sel = NM;
        for (int s = 0; s < NM; ++s) c.hm[s] = b->m[s];
    } else {   // every index in range and selected once
        int first_k[LM_BATCH_MAX];
        for (int s = 0; s < NM; ++s) first_k[s] = -1;
        for (int k = 0; k < c.n_sel; ++k) {
            const int s = c.sel[k];
            if (s < 0 || s >= NM) return fail(RCA_ERR_ARG, "%s: sel[%d] = member %d is outside the batch's members [0, %d)", c.who, k, s, NM);
            if (first_k[s] >= 0) return fail(RCA_ERR_ARG, "%s: sel[%d] = member %d is selected twice (also sel[%d])", c.who, k, s, first_k[s]);
            first_k[s] = k;
            c.hm[k] = b->m[s];
        }
    }
    int rc;
    for (int k = 0; k < c.n_sel; ++k)
        if ((rc = lm_settle(c.hm[k])) != RCA_OK) return rc;
    const int adv = c.frame ? 2 * c.n_steps : n;   // the positions the call advances a member by
    for (int k = 0; k < c.n_sel; ++k) {
        const rca_lm* h = c.hm[k];
        const int V = h->cfg.vocab_size;
        char label[48];
        auto m = [&]() -> const char* {   // the member in messages, composed for a refusal only
            if (c.sel) snprintf(label, sizeof(label), "sel[%d] = member %d", k, c.sel[k]);
            else snprintf(label, sizeof(label), "member %d", k);
            return label;
        };
        if (!h->sampler_set) return fail(RCA_ERR_STATE, "%s: %s has no sampler (rca_lm_sampler_init)", c.who, m());
        if (h->cfg.logits_all) return fail(RCA_ERR_STATE, "%s: %s was switched to logits_all after the batch was made", c.who, m());
        if (h->kv_format != b->m[0]->kv_format) return fail(RCA_ERR_STATE, "%s: %s has KV format %d, member 0 has %d", c.who, m(), h->kv_format, b->m[0]->kv_format);
        if (lm_prefill_route(h) != LM_ROUTE_TILE128)
            return fail(RCA_ERR_STATE, "%s: %s no longer takes the 128-token tiles (rca_lm_prefill_route %d)", c.who, m(), lm_prefill_route(h));
        if (h->n_tokens + adv > h->cfg.n_ctx) return fail(RCA_ERR_STATE, "%s: context overflow of %s: %d + %d > n_ctx %d", c.who, m(), h->n_tokens, adv, h->cfg.n_ctx);
        for (int j = 0; j < n; ++j)
            if (c.ids[k * n + j] < 0 || c.ids[k * n + j] >= V)
                return fail(RCA_ERR_ARG, "%s: token id %d of %s at index %d%s is outside the vocabulary [0, %d)", c.who, c.ids[k * n + j], m(), j,
                            c.frame ? " of its first pair" : "", V);
        for (int i = 0; c.user_ids && i < c.n_steps; ++i)
            if (c.user_ids[k * c.n_steps + i] < 0 || c.user_ids[k * c.n_steps + i] >= V)
                return fail(RCA_ERR_ARG, "%s: user token id %d of %s at step %d is outside the vocabulary [0, %d)", c.who, c.user_ids[k * c.n_steps + i], m(), i, V);
        for (int i = 0; i < c.n_probe; ++i) {
            const int id = c.probe_ids[k * c.n_probe + i];
            if (c.frame && (id < -1 || id >= V)) return fail(RCA_ERR_ARG, "%s: probe id %d of %s is outside the vocabulary [0, %d) (-1: no probe)", c.who, id, m(), V);
            if (!c.frame && (id < 0 || id >= V)) return fail(RCA_ERR_ARG, "%s: probe id %d of %s at index %d is outside the vocabulary [0, %d)", c.who, id, m(), i, V);
        }
    }
    return RCA_OK;
}
// the selection graphs hold member 0's workspace and the sampler launches of the chain: they go when a member dropped its own graphs
static void lm_batch_sel_epoch(rca_lm_batch* b) {
    unsigned long long epoch = 0;
    for (int s = 0; s < b->n_members; ++s) epoch += b->m[s]->drop_epoch;
    if (epoch != b->sel_epoch) {
        lm_batch_drop_sel_graphs(b);
        lm_batch_duplex_drop_graphs(b->dx);
        b->sel_epoch = epoch;
    }
}
// The call's block in pinned memory and what the launches need to know about its members.  Without a selection the tables are the
// batch's resident ones (lm_batch_refresh), members with a whole-vocabulary sampler included: their own launches may sit in a graph
// that goes with their graph_epoch.  With one, the tables are composed here for slots 0 .. n_sel - 1, all-zero entries behind them.
struct LmBatchPlan { LmBatchView vw; bool graphs, any_patch; int cls, bucket, nsp, nsp_bucket; size_t up_bytes; };
static int lm_batch_stage(rca_lm_batch* b, const LmBatchCall& c, LmBatchPlan* plan) {
    RCA_HIP(hipSetDevice(b->m[0]->device));
    int rc;
    if (c.sel) lm_batch_sel_epoch(b);
    else if ((rc = lm_batch_refresh(b)) != RCA_OK) return rc;
    LmBatchPlan p{};
    const int n = c.n, adv = c.frame ? 2 * c.n_steps : n;
    p.cls = lm_batch_class(c.n_sel);
    p.graphs = true;
    p.nsp = 1;
    // the head of the block that the call uploads: a frame does not carry the tables without a selection, nor a step's probe ids
    p.up_bytes = c.sel ? (c.frame ? sizeof(LmBatchSelStage) : sizeof(LmBatchStepSelStage)) : (c.frame ? sizeof(LmBatchFrameStage) : sizeof(LmBatchStage));
    bool any_serial = false;
    LmBatchStepSelStage& in = *b->sel_pin;
    memset(&in, 0, p.up_bytes);   // slots past the selection: all-zero entries, the table kernels leave on them
    in.n_live = c.n_sel;
    if (p.up_bytes == sizeof(LmBatchStepSelStage)) in.n_probe = c.n_probe;
    for (int k = 0; k < c.n_sel; ++k) {
        rca_lm* h = c.hm[k];
        p.graphs = p.graphs && h->graphs_enabled;
        if (c.sel) {
            const bool serial = !lm_samp_own_launches(h);
            p.graphs = p.graphs && serial;   // a whole-vocabulary sampler has launches of its own with its own pointers: eager
            any_serial = any_serial || serial;
            p.any_patch = p.any_patch || (serial && h->samp_patch);
            in.tab[k] = lm_batch_member(h, k * n, serial);
            for (int j = 0; j < n; ++j) in.rows[k * n + j] = lm_group_row(h, j, k * n + j);
        }
        in.n_tokens[k] = h->n_tokens;
        for (int j = 0; j < n; ++j) in.ids[k * n + j] = c.ids[k * n + j];
        for (int i = 0; c.user_ids && i < c.n_steps; ++i) in.user[k * LM_FRAME_MAX + i] = c.user_ids[k * c.n_steps + i];
        if (c.frame) in.probe[k] = c.probe_ids ? c.probe_ids[k] : -1;
        else for (int i = 0; i < c.n_probe; ++i) in.probe_ids[k * c.n_probe + i] = c.probe_ids[k * c.n_probe + i];
        // the bucket and the splits of the call's END (as lm_frame_core): a frame that crosses a bucket or a 256-key split inside itself
        // has the splits its last step needs; its earlier steps leave the extra ones at once
        p.bucket = std::max(p.bucket, lm_bucket(h, adv, -1).bucket);
        p.nsp = std::max(p.nsp, lm_splits_needed(h, adv));
    }
    for (int k = c.n_sel; c.frame && k < LM_BATCH_MAX; ++k) in.probe[k] = -1;
    // a graph's split count is the bucket's over ALL members of the batch, so that the grid does not depend on who is selected (a
    // split past a member's cache leaves at once)
    p.nsp_bucket = p.bucket + 1 == LM_GRAPH_BUCKETS ? b->nsp_all : std::min(b->nsp_all, 4 << p.bucket);
    if (c.sel) p.vw = LmBatchView{b->sel_stage->rows, b->sel_stage->tab, 8 << p.cls, any_serial, p.any_patch, c.hm, c.n_sel};
    else p.vw = lm_batch_view(b, n);
    p.any_patch = p.vw.any_patch;
    *plan = p;
    return RCA_OK;
}
// upload -> stage -> [encode tails -> codes to ids] -> one pass of n tokens, or n_steps x (pass of pairs, feedback) -> [ids to codes ->
// decode tails] -> probes -> [a step's token gather] -> download, one linear sequence on `st`; the codec tails with a duplex call only.
// A captured sequence launches the bucket's splits, an eager one what the members need now.
static int lm_batch_enqueue(rca_lm_batch* b, const LmBatchCall& c, const LmBatchPlan& p, bool captured, hipStream_t st, const LmBatchDuplexCall* dc = nullptr) {
    const int V = b->m[0]->cfg.vocab_size, n_steps = c.n_steps, nsp_launch = captured ? p.nsp_bucket : p.nsp;
    const LmBatchView& vw = p.vw;
    LmBatchDuplex* d = b->dx;
    hipError_t e = hipMemcpyAsync(b->sel_stage, b->sel_pin, p.up_bytes, hipMemcpyHostToDevice, st);
    if (e == hipSuccess && dc) e = hipMemcpyAsync(d->pcm_in, d->pin + dc->pin_pcm, (size_t)dc->slots * dc->T * 4, hipMemcpyHostToDevice, st);
    if (e == hipSuccess && dc) e = hipMemcpyAsync(d->code_win, d->pin + dc->pin_codes, (size_t)dc->slots * (dc->F_ctx + n_steps) * 8, hipMemcpyHostToDevice, st);
    if (e != hipSuccess) return fail(RCA_ERR_HIP, "%s upload: %s", c.who, hipGetErrorString(e));
    lm_batch_stage_kernel<<<1, LM_BATCH_ROWS, 0, st>>>(b->sel_stage, vw.tab, b->stt, b->stt_head, c.n);
    if (dc) {
        const int r = rca_codec_encode_tail_dev(dc->codec, d->pcm_in, dc->slots, dc->T, n_steps, (int64_t*)d->dev->user_codes, st);
        if (r != RCA_OK) return r;
        duplex_batch_codes_to_ids_kernel<<<dc->slots, 64, 0, st>>>(d->dev->user_codes, n_steps, dc->base, b->sel_stage, d->dev->flags);
    }
    if (!c.frame) lm_batch_enqueue_pass(b, vw, c.n, nsp_launch, st);
    for (int i = 0; i < n_steps; ++i) {
        lm_batch_enqueue_pass(b, vw, 2, nsp_launch, st);
        lm_batch_feedback_kernel<<<1, LM_BATCH_MAX, 0, st>>>(b->sel_stage, vw.tab, b->stt, b->frame_out, vw.NM, i);
    }
    if (dc) {
        const int F = dc->F_ctx + n_steps;
        duplex_batch_tokens_to_codes_kernel<<<dc->slots, 64, 0, st>>>(b->frame_out, b->sel_stage, n_steps, dc->base, dc->n_codes, d->code_win, F, d->dev->flags);
        const int r = rca_codec_decode_tail_dev(dc->codec, (const int64_t*)d->code_win, dc->slots, F, dc->n_samples, d->pcm_out, st);
        if (r != RCA_OK) return r;
    }
    if (c.n_probe) {
        lm_softmax_slices_batch_kernel<<<dim3(PROBS_SLICES, vw.NM), 1024, 0, st>>>(vw.tab, V, b->probe_part);
        if (c.frame) lm_token_probs_batch_kernel<<<dim3(1, vw.NM), 64, 0, st>>>(vw.tab, V, b->probe_part, b->sel_stage->probe, b->frame_out->probs);
        else lm_token_probs_sel_kernel<<<dim3(1, vw.NM), 64, 0, st>>>(vw.tab, V, b->probe_part, b->sel_stage, b->step_out->probs);
    }
    if (!c.frame) lm_batch_tokens_kernel<<<1, LM_BATCH_MAX, 0, st>>>(vw.tab, vw.NM, b->step_out->tokens);
    RCA_LAUNCH_CHECK();
    // a frame's tokens and probes; a step's tokens, with the probabilities behind them where the call can have any (rca_lm_batch_step_sel)
    if (c.frame) e = hipMemcpyAsync(b->frame_pin, b->frame_out, sizeof(LmBatchFrameOut), hipMemcpyDeviceToHost, st);
    else e = hipMemcpyAsync(b->step_out_pin, b->step_out, c.sel ? sizeof(LmBatchStepSelOut) : sizeof(int) * LM_BATCH_MAX, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess && dc) e = hipMemcpyAsync(d->pin, d->dev, sizeof(LmBatchDuplexDev), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess && dc) e = hipMemcpyAsync(d->pin + dc->pin_out, d->pcm_out, (size_t)dc->slots * dc->n_samples * 4, hipMemcpyDeviceToHost, st);
    return e == hipSuccess ? RCA_OK : fail(RCA_ERR_HIP, "%s download: %s", c.who, hipGetErrorString(e));
}
// Replays the graph of `slot`, capturing it first if the slot is empty (counted: rca_lm_batch_captures), or with graphs off enqueues
// eagerly; then waits for the stream.  `enqueue(captured)` puts the call's sequence on `st`.
template <class F>
static int lm_batch_run(rca_lm_batch* b, hipStream_t st, hipGraphExec_t* slot, const char* tag, bool graphs, F&& enqueue) {
    int rc;
    if (graphs) {
        if (!*slot) {
            if ((rc = lm_capture(st, slot, tag, [&]() -> int { return enqueue(true); })) != RCA_OK) return rc;
            b->n_captures++;
        }
        RCA_HIP(hipGraphLaunch(*slot, st));
    } else if ((rc = enqueue(false)) != RCA_OK) {
        return rc;
    }
    RCA_HIP(hipStreamSynchronize(st));
    return RCA_OK;
}
// A step's settlement, after the synchronisation: every member of the pass took n tokens and drew once.
static void lm_batch_step_settle(rca_lm_batch* b, const LmBatchCall& c, int32_t* tokens) {
    for (int k = 0; k < c.n_sel; ++k) {
        rca_lm* h = c.hm[k];
        h->n_tokens += c.n;
        h->logits_rows = 1;
        h->rng_host += 1;
        tokens[k] = b->step_out_pin->tokens[k];
    }
}
// A frame's settlement, after the synchronisation: which steps of every member of the pass stand, as lm_frame_core settles one handle.
// `tab` is the table of the pass, where the slot of a cut member is addressed (the device tables still hold this call's members).
static int lm_batch_sel_settle(rca_lm_batch* b, const LmBatchCall& c, const LmBatchMember* tab, int audio_id_floor, int32_t* out_tokens, int out_stride,
                               int32_t* n_done, float* probe_probs, hipStream_t st) {
    const LmBatchFrameOut& out = *b->frame_pin;
    const int n_steps = c.n_steps;
    LmBatchCuts cuts;
    cuts.n = 0;
    for (int k = 0; k < c.n_sel; ++k) {
        rca_lm* h = c.hm[k];
        int done = n_steps;
        for (int i = 0; i < n_steps; ++i) {
            out_tokens[k * out_stride + i] = out.tokens[k * LM_FRAME_MAX + i];
            if (out_tokens[k * out_stride + i] <= audio_id_floor) { done = i + 1; break; }
        }
        for (int i = done; i < out_stride; ++i) out_tokens[k * out_stride + i] = -1;
        n_done[k] = done;
        h->n_tokens += 2 * done;
        // a member cut short holds the logits of a LATER step (evaluated on a wrong-guess pair): nothing may read them
        h->logits_rows = done < n_steps ? 0 : 1;
        h->rng_host += (unsigned long long)done;
        if (done < n_steps) {
            cuts.member[cuts.n] = k;
            cuts.counter[cuts.n++] = h->rng_host;
        }
        if (probe_probs) probe_probs[k] = done < n_steps || !c.probe_ids || c.probe_ids[k] < 0 ? -1.0f : out.probs[k];
    }
    if (cuts.n) {   // the device drew n_steps times for these: their counters go where the step-by-step loop would be, in one launch
        lm_batch_counters_kernel<<<1, LM_BATCH_MAX, 0, st>>>(tab, cuts);
        RCA_LAUNCH_CHECK();
        RCA_HIP(hipStreamSynchronize(st));
    }
    return RCA_OK;
}

// rca_lm_batch_step: every member advances by its n tokens in one pass over the batch's resident tables
extern "C" int rca_lm_batch_step(rca_lm_batch_t* b, const int32_t* ids, int32_t n, int32_t* tokens) {
    if (!b || !ids || !tokens) return fail(RCA_ERR_ARG, "batch_step: null argument");
    if (n < 1 || n > LM_GEMV_M) return fail(RCA_ERR_ARG, "batch_step: %d tokens per member (1..%d)", n, LM_GEMV_M);
    LmBatchCall c{"batch_step", nullptr, 0, n, false, 0, ids, nullptr, nullptr, 0};
    LmBatchPlan p;
    hipStream_t st = b->m[0]->stream;
    int rc;
    if ((rc = lm_batch_check(b, c)) != RCA_OK || (rc = lm_batch_stage(b, c, &p)) != RCA_OK) return rc;
    if ((rc = lm_batch_run(b, st, &b->g[n - 1][p.bucket], "batch step", p.graphs, [&](bool captured) -> int { return lm_batch_enqueue(b, c, p, captured, st); })) != RCA_OK) return rc;
    lm_batch_step_settle(b, c, tokens);
    return RCA_OK;
}

// ------------------------------------------------------------------------------------ batch frame (rca_lm_batch_frame)
// rca_lm_frame for every member of a batch in one launch sequence: n_steps times the batch pass over pairs (lm_batch_enqueue_pass, the
// launches of a 2-token batch step) with lm_batch_feedback_kernel between them, then the probes.  Every member runs every step -- a
// row cannot leave a captured graph -- and the host settles afterwards which steps of a member stand, as lm_frame_core does for one.
extern "C" int rca_lm_batch_frame(rca_lm_batch_t* b, const int32_t* first_pairs, const int32_t* user_ids, int32_t n_steps, int32_t audio_id_floor,
                                  const int32_t* probe_ids, int32_t* out_tokens, int32_t* n_done, float* probe_probs) {
    if (!b || !first_pairs || !user_ids || !out_tokens || !n_done) return fail(RCA_ERR_ARG, "batch_frame: null argument");
    if (probe_ids && !probe_probs) return fail(RCA_ERR_ARG, "batch_frame: probe_ids without probe_probs");
    LmBatchCall c{"batch_frame", nullptr, 0, 2, true, n_steps, first_pairs, user_ids, probe_ids, probe_ids ? 1 : 0};
    LmBatchPlan p;
    hipStream_t st = b->m[0]->stream;
    int rc;
    if ((rc = lm_batch_check(b, c)) != RCA_OK || (rc = lm_batch_stage(b, c, &p)) != RCA_OK) return rc;
    if ((rc = lm_batch_run(b, st, &b->fg[n_steps - 1][p.bucket][c.n_probe], "batch frame", p.graphs, [&](bool captured) -> int { return lm_batch_enqueue(b, c, p, captured, st); })) != RCA_OK)
        return rc;
    return lm_batch_sel_settle(b, c, p.vw.tab, audio_id_floor, out_tokens, n_steps, n_done, probe_ids ? probe_probs : nullptr, st);
}

// ------------------------------------------------------------------------------------ selection frame (rca_lm_batch_frame_sel)
// rca_lm_batch_frame over a SUBSET of the members: sessions sit ticks out (windows still filling, a forced branch, a trim between two
// steps, a chunk that has not arrived).  The selected members are compacted into slots 0 .. n_sel - 1 of tables composed on the host
// for THIS call (LmBatchSelStage) and uploaded with the frame's block inside the replay; the launches cover the selection's geometry
// class (8, 16, 32 or 64 slots).  The live count travels in the block: the row-wise kernels leave on the pass state's m, the table
// kernels on the all-zero entry of a slot past it.  So a graph holds no member's pointer -- only member 0's workspace and weights --
// and is keyed by (class, n_steps, bucket, probes, patching samplers): it serves every selection of its class and outlives a member's
// rca_lm_swap_kv.  An unselected member is not read on the device and not written anywhere.
extern "C" int rca_lm_batch_frame_sel(rca_lm_batch_t* b, const int32_t* sel, int32_t n_sel, const int32_t* first_pairs, const int32_t* user_ids, int32_t n_steps,
                                      int32_t audio_id_floor, const int32_t* probe_ids, int32_t* out_tokens, int32_t* n_done, float* probe_probs) {
    if (!b || !sel || !first_pairs || !user_ids || !out_tokens || !n_done) return fail(RCA_ERR_ARG, "batch_frame_sel: null argument");
    if (probe_ids && !probe_probs) return fail(RCA_ERR_ARG, "batch_frame_sel: probe_ids without probe_probs");
    LmBatchCall c{"batch_frame_sel", sel, n_sel, 2, true, n_steps, first_pairs, user_ids, probe_ids, probe_ids ? 1 : 0};
    LmBatchPlan p;
    hipStream_t st = b->m[0]->stream;
    int rc;
    if ((rc = lm_batch_check(b, c)) != RCA_OK || (rc = lm_batch_stage(b, c, &p)) != RCA_OK) return rc;
    hipGraphExec_t* slot = &b->sg[p.cls][n_steps - 1][p.bucket][c.n_probe][p.any_patch ? 1 : 0];
    if ((rc = lm_batch_run(b, st, slot, "batch frame_sel", p.graphs, [&](bool captured) -> int { return lm_batch_enqueue(b, c, p, captured, st); })) != RCA_OK) return rc;
    return lm_batch_sel_settle(b, c, p.vw.tab, audio_id_floor, out_tokens, n_steps, n_done, probe_ids ? probe_probs : nullptr, st);
}

// ------------------------------------------------------------------------------------ selection step (rca_lm_batch_step_sel)
// rca_lm_step_probe for a SUBSET of the members in one pass: the agents' speculative <|end_audio|> step for the members of a tick that
// owe it, or a server's step of the sessions that are in a text branch.  The selection machinery of the frame above with n = 1 or 2
// tokens per member: tables of slots 0 .. n_sel - 1 composed for this call, uploaded with the ids and the probe ids as one block inside
// the replay; the launches cover the class, the live count and the probe count travel in the block.  A selected member ends as
// rca_lm_batch_step(n) of a batch over the selected members alone leaves it; an unselected member is in no table of the call.
extern "C" int rca_lm_batch_step_sel(rca_lm_batch_t* b, const int32_t* sel, int32_t n_sel, const int32_t* ids, int32_t n, const int32_t* probe_ids, int32_t n_probe,
                                     int32_t* tokens, float* probs) {
    const char* who = "batch_step_sel";
    if (!b || !sel || !ids || !tokens) return fail(RCA_ERR_ARG, "%s: null argument", who);
    if (n < 1 || n > LM_GEMV_M) return fail(RCA_ERR_ARG, "%s: %d tokens per member (1..%d)", who, n, LM_GEMV_M);
    if (n_probe < 0 || n_probe > LM_STEP_PROBES) return fail(RCA_ERR_ARG, "%s: %d probe ids per member (0..%d)", who, n_probe, LM_STEP_PROBES);
    if ((n_probe > 0) != (probe_ids != nullptr)) return fail(RCA_ERR_ARG, "%s: probe_ids is null exactly when n_probe is 0 (n_probe %d)", who, n_probe);
    if (n_probe > 0 && !probs) return fail(RCA_ERR_ARG, "%s: probe_ids without probs", who);
    LmBatchCall c{who, sel, n_sel, n, false, 0, ids, nullptr, probe_ids, n_probe};
    LmBatchPlan p;
    hipStream_t st = b->m[0]->stream;
    int rc;
    if ((rc = lm_batch_check(b, c)) != RCA_OK || (rc = lm_batch_stage(b, c, &p)) != RCA_OK) return rc;
    hipGraphExec_t* slot = &b->ssg[p.cls][n - 1][p.bucket][n_probe ? 1 : 0][p.any_patch ? 1 : 0];
    if ((rc = lm_batch_run(b, st, slot, "batch step_sel", p.graphs, [&](bool captured) -> int { return lm_batch_enqueue(b, c, p, captured, st); })) != RCA_OK) return rc;
    lm_batch_step_settle(b, c, tokens);
    if (n_probe) memcpy(probs, b->step_out_pin->probs, sizeof(float) * (size_t)n_sel * n_probe);
    return RCA_OK;
}

// ------------------------------------------------------------------------------------ duplex batch frame (rca_duplex_batch_frame)
// rca_duplex_frame for every selected member of a batch in one call: upload -> encode tails over the class's rows -> codes to ids (into
// the frame block's user table, on the device) -> the selection frame -> ids to codes behind every row's context -> decode tails ->
// probes -> download, one linear sequence on member 0's stream with no side branch.  The host owns every rolling window and passes them
// whole, as for one session.  Rows past the selection hold code 0 and whatever finite PCM the block held: the codec runs over them
// (one codec shape per class) and nothing reads their results.
static int lm_batch_duplex_reserve(rca_lm_batch* b, int slots, int T, int F, int n_samples, size_t pin_total, hipStream_t st) {
    if (!b->dx) b->dx = new LmBatchDuplex();
    LmBatchDuplex* d = b->dx;
    const size_t np = (size_t)slots * T, nc = (size_t)slots * F, no = (size_t)slots * n_samples;
    if (np <= d->pcm_in_cap && nc <= d->code_win_cap && no <= d->pcm_out_cap && pin_total <= d->pin_cap && d->dev) return RCA_OK;
    RCA_HIP(hipStreamSynchronize(st));
    lm_batch_duplex_drop_graphs(d);   // a buffer is about to move
    int rc;
    if (np > d->pcm_in_cap) {
        if ((rc = duplex_grow(&d->pcm_in, &d->pcm_in_cap, np)) != RCA_OK) return rc;
        RCA_HIP(hipMemset(d->pcm_in, 0, np * 4));
    }
    if (nc > d->code_win_cap) {
        if ((rc = duplex_grow(&d->code_win, &d->code_win_cap, nc)) != RCA_OK) return rc;
        RCA_HIP(hipMemset(d->code_win, 0, nc * 8));
    }
    if (no > d->pcm_out_cap && (rc = duplex_grow(&d->pcm_out, &d->pcm_out_cap, no)) != RCA_OK) return rc;
    if (!d->dev) {
        if ((rc = lm_alloc((void**)&d->dev, sizeof(LmBatchDuplexDev))) != RCA_OK) return rc;
        RCA_HIP(hipMemset(d->dev, 0, sizeof(LmBatchDuplexDev)));
    }
    if (pin_total > d->pin_cap) {
        if (d->pin) (void)hipHostFree(d->pin);
        d->pin = nullptr; d->pin_cap = 0;
        RCA_HIP(hipHostMalloc((void**)&d->pin, pin_total, hipHostMallocDefault));
        d->pin_cap = pin_total;
        memset(d->pin, 0, pin_total);
    }
    return RCA_OK;
}
extern "C" int rca_duplex_batch_frame(rca_lm_batch_t* b, rca_codec_t* codec, const rca_duplex_batch_args_t* a, rca_duplex_batch_out_t* out, float* pcm_out_host) {
    if (!b || !codec || !a || !out || !pcm_out_host || !a->sel || !a->pcm_windows || !a->first_pairs || (a->F_ctx > 0 && !a->code_ctx) || !out->user_codes ||
        !out->tokens || !out->n_done || !out->flags || !out->probe_prob)
        return fail(RCA_ERR_ARG, "duplex_batch_frame: null argument");
    const int n = a->n_steps, n_sel = a->n_sel;
    if (a->T < 1 || a->F_ctx < 0 || a->n_samples < 1) return fail(RCA_ERR_ARG, "duplex_batch_frame: bad shape (T=%d F_ctx=%d n_samples=%d)", a->T, a->F_ctx, a->n_samples);
    LmBatchCall c{"duplex_batch_frame", a->sel, n_sel, 2, true, n, a->first_pairs, nullptr, a->probe_ids, a->probe_ids ? 1 : 0};
    LmBatchPlan p;
    int rc;
    if ((rc = lm_batch_check(b, c)) != RCA_OK) return rc;
    int32_t n_codes = 0, hop = 0;
    if ((rc = rca_codec_codebook_size(codec, &n_codes)) != RCA_OK || (rc = rca_codec_hop(codec, &hop)) != RCA_OK) return rc;
    const int V = b->m[0]->cfg.vocab_size, F = a->F_ctx + n;
    if (a->code_token_base < 0 || (long)a->code_token_base + n_codes > V)
        return fail(RCA_ERR_ARG, "duplex_batch_frame: codes [%d, %d + %d) fall outside the vocabulary", a->code_token_base, a->code_token_base, n_codes);
    if (((long)a->T + hop - 1) / hop < n) return fail(RCA_ERR_ARG, "duplex_batch_frame: %d codes wanted, a window of %d samples holds %ld", n, a->T, ((long)a->T + hop - 1) / hop);
    if ((long)a->n_samples > (long)F * hop) return fail(RCA_ERR_ARG, "duplex_batch_frame: %d samples wanted, %d codes give %ld", a->n_samples, F, (long)F * hop);
    for (int k = 0; k < n_sel; ++k)
        for (int i = 0; i < a->F_ctx; ++i) {
            const long long code = a->code_ctx[(long)k * a->F_ctx + i];
            if (code < 0 || code >= n_codes) return fail(RCA_ERR_ARG, "duplex_batch_frame: code %lld of sel[%d] = member %d at index %d of its context is out of range [0, %d)", code, k, a->sel[k], i, n_codes);
        }
    hipStream_t st = b->m[0]->stream;
    if ((rc = lm_batch_stage(b, c, &p)) != RCA_OK) return rc;
    const int slots = 8 << p.cls;
    auto up256 = [](size_t x) { return (x + 255) & ~(size_t)255; };
    LmBatchDuplexCall dc{codec, slots, a->T, a->F_ctx, a->n_samples, a->code_token_base, n_codes, 0, 0, 0};
    dc.pin_pcm = up256(sizeof(LmBatchDuplexDev));
    dc.pin_codes = dc.pin_pcm + up256((size_t)slots * a->T * 4);
    dc.pin_out = dc.pin_codes + up256((size_t)slots * F * 8);
    const size_t pin_total = dc.pin_out + (size_t)slots * a->n_samples * 4;
    if ((rc = lm_batch_duplex_reserve(b, slots, a->T, F, a->n_samples, pin_total, st)) != RCA_OK) return rc;
    LmBatchDuplex* d = b->dx;
    // The code rows past the selection are cleared for every call (at most 64 x F codes): whatever an earlier call of another shape or
    // another codec left at this place of the block must not reach the decoder as a code.  The PCM rows past the selection keep what
    // they hold -- zeros, or bytes of an earlier call's windows, codes or output, all finite floats -- and nothing reads their results.
    memset(d->pin + dc.pin_codes + (size_t)n_sel * F * 8, 0, (size_t)(slots - n_sel) * F * 8);
    // stage the windows: row k of the class's block is sel[k]'s (the new codes' places of a context row are written by the device)
    memcpy(d->pin + dc.pin_pcm, a->pcm_windows, (size_t)n_sel * a->T * 4);
    for (int k = 0; k < n_sel && a->F_ctx; ++k) memcpy(d->pin + dc.pin_codes + (size_t)k * F * 8, a->code_ctx + (long)k * a->F_ctx, (size_t)a->F_ctx * 8);
    uint64_t csig = 0;
    if ((rc = rca_codec_workspace_sig(codec, &csig)) != RCA_OK) return rc;
    bool warmed = false;
    for (auto& w : d->warm)
        warmed = warmed || (w.cls == p.cls && w.T == a->T && w.F_ctx == a->F_ctx && w.n_steps == n && w.n_samples == a->n_samples && w.codec == (const void*)codec && w.codec_sig == csig);
    // the codec's ordering moves to this stream (nothing of it is in flight elsewhere once this returns)
    if ((rc = rca_codec_stream_handoff(codec, st)) != RCA_OK) return rc;
    const bool graphs = p.graphs && warmed;
    hipGraphExec_t* slot = nullptr;   // the keyed entry's
    if (graphs) {
        const LmBatchDuplexKey key{p.cls, a->T, a->F_ctx, n, a->n_samples, c.n_probe, p.bucket, a->code_token_base, p.any_patch ? 1 : 0, csig, (const void*)codec};
        for (auto& e : d->graphs)
            if (e.key == key) slot = &e.exec;
        if (!slot) {
            if (d->graphs.size() >= 32) lm_batch_duplex_drop_graphs(d);   // stale shapes: start over (the stream is idle between calls)
            d->graphs.push_back(LmBatchDuplex::Entry{key, nullptr});
            slot = &d->graphs.back().exec;
        }
    }
    if ((rc = lm_batch_run(b, st, slot, "duplex batch", graphs, [&](bool captured) -> int { return lm_batch_enqueue(b, c, p, captured, st, &dc); })) != RCA_OK) return rc;
    if (!warmed) {   // the eager run sized the codec workspace of this (class, shape): graphs are keyed by the signature after it
        if ((rc = rca_codec_workspace_sig(codec, &csig)) != RCA_OK) return rc;
        if (d->warm.size() >= 32) d->warm.clear();
        d->warm.push_back(LmBatchDuplex::Warm{p.cls, a->T, a->F_ctx, n, a->n_samples, (const void*)codec, csig});
    }
    if ((rc = lm_batch_sel_settle(b, c, p.vw.tab, a->audio_id_floor, out->tokens, LM_FRAME_MAX, out->n_done, out->probe_prob, st)) != RCA_OK) return rc;
    const LmBatchDuplexDev* got = reinterpret_cast<const LmBatchDuplexDev*>(d->pin);
    for (int k = 0; k < n_sel; ++k) {
        for (int i = 0; i < LM_FRAME_MAX; ++i) out->user_codes[k * LM_FRAME_MAX + i] = i < n ? got->user_codes[k * n + i] : 0;
        out->flags[k] = got->flags[k] | (out->n_done[k] < n ? 2 : 0);
        if (out->flags[k] == 0) memcpy(pcm_out_host + (size_t)k * a->n_samples, d->pin + dc.pin_out + (size_t)k * a->n_samples * 4, (size_t)a->n_samples * 4);
    }
    return RCA_OK;
}
extern "C" int rca_lm_batch_captures(const rca_lm_batch_t* b, int64_t* n) {
    if (!b || !n) return fail(RCA_ERR_ARG, "batch_captures: null argument");
    *n = b->n_captures;
    return RCA_OK;
}

// One frame of the duplex loop as ONE graph (process_audio_input_ids, realtime_agent_v2.py:332-372, while every sampled token is an
// audio token): step i evaluates [agent_{i-1}, user_{i-1}] -- for i = 0 the pair the caller passes -- and samples agent_i, which
// goes back into step i + 1 on the device together with the user's token of frame i.  One host synchronisation per frame instead
// of one per step.  If step j samples a token <= audio_id_floor (the loop leaves audio mode there), steps after j have run on a
// wrong guess: n_done = j + 1, the KV position and the draw counter are put back to what the step-by-step loop would have (their
// cache slots are stale and get overwritten, exactly like a rollback), and the caller carries on step by step.
static int lm_frame_core(rca_lm_t* h, const int32_t* first_pair, const int32_t* user_ids, int32_t n_steps, int32_t audio_id_floor,
                         int32_t* out_tokens, int32_t* n_done, int cap_bucket) {
    if (!h || !first_pair || !user_ids || !out_tokens || !n_done) return fail(RCA_ERR_ARG, "frame: null argument");
    if (n_steps < 1 || n_steps > LM_FRAME_MAX) return fail(RCA_ERR_ARG, "frame: %d steps (1..%d)", n_steps, LM_FRAME_MAX);
    if (!h->sampler_set) return fail(RCA_ERR_STATE, "sampler not initialised");
    if (h->cfg.logits_all) return fail(RCA_ERR_STATE, "frame: not on a logits_all handle");
    if (cap_bucket < 0 && h->n_tokens + 2 * n_steps > h->cfg.n_ctx) return fail(RCA_ERR_STATE, "context overflow: %d + %d > n_ctx %d", h->n_tokens, 2 * n_steps, h->cfg.n_ctx);
    for (int i = 0; i < 2; ++i)
        if (first_pair[i] < 0 || first_pair[i] >= h->cfg.vocab_size) return fail(RCA_ERR_ARG, "frame: token id %d outside the vocabulary", first_pair[i]);
    for (int i = 0; i < n_steps; ++i)
        if (user_ids[i] < 0 || user_ids[i] >= h->cfg.vocab_size) return fail(RCA_ERR_ARG, "frame: token id %d outside the vocabulary", user_ids[i]);
    { const int src = lm_settle(h); if (src != RCA_OK) return src; }
    RCA_HIP(hipSetDevice(h->device));
    hipStream_t st = h->stream;
    int rc = RCA_OK;
    lm_stage_state(h, first_pair, 2);
    for (int i = 0; i < n_steps; ++i) h->h_stt->ids[LM_FRAME_USER0 + i] = user_ids[i];
    const LmBucket bk = lm_bucket(h, 2 * n_steps, cap_bucket);
    hipGraphExec_t& gexec = lm_graph_set(h).fg[n_steps][bk.bucket];
    if (cap_bucket >= 0 && (gexec || !h->graphs_enabled)) return RCA_OK;
    auto enqueue = [&]() -> int {
        hipError_t e = hipMemcpyAsync(h->stt, h->h_stt, LM_STATE_DECODE_BYTES, hipMemcpyHostToDevice, st);
        if (e != hipSuccess) return fail(RCA_ERR_HIP, "frame memcpy: %s", hipGetErrorString(e));
        for (int i = 0; i < n_steps; ++i) {
            const int r = lm_enqueue_pass(h, 2, 1, st, bk.nsp_launch, i > 0);
            if (r != RCA_OK) return r;
            lm_enqueue_sample(h, h->logits, st, i);
        }
        e = hipMemcpyAsync(h->h_stt->frame_out, h->stt->frame_out, sizeof(int) * LM_FRAME_MAX, hipMemcpyDeviceToHost, st);
        return e == hipSuccess ? RCA_OK : fail(RCA_ERR_HIP, "frame d2h: %s", hipGetErrorString(e));
    };
    if (!h->graphs_enabled) {   // tests: the same launches, eagerly
        RCA_HIP(hipStreamSynchronize(st));
        if ((rc = enqueue()) != RCA_OK) return rc;
    } else if (!gexec && (rc = lm_capture(st, &gexec, "frame", enqueue)) != RCA_OK) {
        return rc;
    }
    if (cap_bucket >= 0) return RCA_OK;      // rca_duplex_precapture: the graph exists now, nothing is launched
    if (h->graphs_enabled) RCA_HIP(hipGraphLaunch(gexec, st));
    RCA_HIP(hipStreamSynchronize(st));
    int done = n_steps;
    for (int i = 0; i < n_steps; ++i) {
        out_tokens[i] = h->h_stt->frame_out[i];
        if (out_tokens[i] <= audio_id_floor) { done = i + 1; break; }
    }
    *n_done = done;
    h->n_tokens += 2 * done;
    // a frame cut short leaves the logits of a LATER step (evaluated on a wrong-guess pair, rolled back above) in the buffer: nothing
    // may read them -- get_logits / token_probs / sample fail with "no logits" until the next eval
    h->logits_rows = done < n_steps ? 0 : 1;
    h->rng_host += (unsigned long long)done;
    if (done < n_steps) {   // the device drew n_steps times: put its counter where the step-by-step loop would be
        RCA_HIP(hipMemcpy(&h->stt->rng_counter, &h->rng_host, 8, hipMemcpyHostToDevice));
    }
    return RCA_OK;
}

extern "C" int rca_lm_frame(rca_lm_t* h, const int32_t* first_pair, const int32_t* user_ids, int32_t n_steps, int32_t audio_id_floor,
                            int32_t* out_tokens, int32_t* n_done) {
    return lm_frame_core(h, first_pair, user_ids, n_steps, audio_id_floor, out_tokens, n_done, -1);
}

// ---- one duplex frame as ONE graph (process_audio, realtime_agent_v2.py:504-554): encode tail of the user's PCM window -> code ->
// token id (affine: the codec tokens were added to the vocabulary in code order, train_vanilla_latest.py:587-589) -> the chunk's
// n_steps LM steps with device-side feedback (rca_lm_frame) -> token id -> code, appended to the detokenizer's code context ->
// decode tail -> softmax(last logits)[probe] (measure_event_prob, :448-452).  One upload, one replay, one synchronisation.  The host
// stays the owner of both rolling windows (it passes them in whole), so a frame that cannot take this path -- or is cut short --
// simply goes through the separate calls with nothing to repair on the device.
struct DuplexDev {            // device-side scratch of the duplex frame (one allocation)
    long long user_codes[LM_FRAME_MAX];
    float probe_prob;
    int flags;
    int probe_id;
    int pad;
};
struct DuplexPin {            // pinned mirror: inputs first (uploaded), outputs behind
    int probe_id;
    int pad0[3];
    long long user_codes[LM_FRAME_MAX];   // user_codes, probe_prob, flags: one copy of DuplexDev's head
    float probe_prob;
    int flags;
    int frame_out[LM_FRAME_MAX];
};
__global__ void duplex_codes_to_ids_kernel(const long long* __restrict__ codes, int n, int base, LmDevState* stt, int* flags) {
    if (threadIdx.x == 0) *flags = 0;
    if ((int)threadIdx.x < n) stt->ids[LM_FRAME_USER0 + threadIdx.x] = base + (int)codes[threadIdx.x];
}
// frame_out -> codes behind the context codes; a token that is not a codec token (the frame left audio mode, or a padding row of the
// vocabulary was drawn) becomes code 0 and raises flag bit 0: the PCM of this replay is then not used
__global__ void duplex_tokens_to_codes_kernel(const LmDevState* __restrict__ stt, int n, int base, int n_codes, long long* __restrict__ dst,
                                              int* flags) {
    if ((int)threadIdx.x < n) {
        const int c = stt->frame_out[threadIdx.x] - base;
        const bool ok = c >= 0 && c < n_codes;
        dst[threadIdx.x] = ok ? c : 0;
        if (!ok) atomicOr(flags, 1);
    }
}
struct DuplexGraphKey {
    int T, F_ctx, n_steps, n_samples, probe, bucket, base;
    const void* kc;
    unsigned long long codec_sig;
    const void* codec;
    bool operator==(const DuplexGraphKey& o) const {
        return T == o.T && F_ctx == o.F_ctx && n_steps == o.n_steps && n_samples == o.n_samples && probe == o.probe && bucket == o.bucket &&
               base == o.base && kc == o.kc && codec_sig == o.codec_sig && codec == o.codec;
    }
};
struct DuplexState {
    float* pcm_in = nullptr; size_t pcm_in_cap = 0;       // device: the PCM window
    long long* code_win = nullptr; size_t code_win_cap = 0;   // device: context codes + this frame's
    float* pcm_out = nullptr; size_t pcm_out_cap = 0;     // device: decode tail
    DuplexDev* dev = nullptr;
    char* pin = nullptr; size_t pin_cap = 0;              // pinned: [DuplexPin | pcm window | code ctx | pcm out]
    struct Entry { DuplexGraphKey key; hipGraphExec_t exec = nullptr; };
    std::vector<Entry> graphs;
    // call shapes whose codec workspace an eager frame has already sized (a capture must not allocate): one eager frame per SHAPE,
    // not per context bucket
    struct Warm { int T, F_ctx, n_steps, n_samples; const void* codec; unsigned long long codec_sig; };
    std::vector<Warm> warm;
    const void* logits_at_capture = nullptr;
    hipStream_t side = nullptr;      // the encode tail runs beside the first LM step (which does not need this chunk's codes)
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    bool fork = true;
};
static void duplex_drop_graphs(DuplexState* d) {
    if (!d) return;
    for (auto& e : d->graphs)
        if (e.exec) (void)hipGraphExecDestroy(e.exec);
    d->graphs.clear();
}
static void duplex_destroy(DuplexState* d) {
    if (!d) return;
    duplex_drop_graphs(d);
    for (void* p : {(void*)d->pcm_in, (void*)d->code_win, (void*)d->pcm_out, (void*)d->dev})
        if (p) (void)hipFree(p);
    if (d->pin) (void)hipHostFree(d->pin);
    if (d->side) (void)hipStreamDestroy(d->side);
    if (d->ev_fork) (void)hipEventDestroy(d->ev_fork);
    if (d->ev_join) (void)hipEventDestroy(d->ev_join);
    delete d;
}

// byte offsets of the variable parts of DuplexState::pin behind the DuplexPin header, each part on a 256-byte boundary
struct DuplexPinLayout {
    size_t pcm, codes, out, total;
    DuplexPinLayout(int T, int F_ctx, int n_samples)
        : pcm(sizeof(DuplexPin)), codes(pcm + (((size_t)T * 4 + 255) & ~(size_t)255)), out(codes + (((size_t)F_ctx * 8 + 255) & ~(size_t)255)),
          total(out + (size_t)n_samples * 4) {}
};
// buffers, side stream and events of the duplex frame for a call shape (growing a buffer invalidates the graphs captured over it)
static int duplex_reserve(rca_lm* h, int T, int F_ctx, int n, int n_samples) {
    int rc;
    hipStream_t st = h->stream;
    if (!h->duplex) {
        h->duplex = new DuplexState();
        const char* nf = getenv("RCA_DUPLEX_FORK");
        h->duplex->fork = !(nf && nf[0] == '0');
        RCA_HIP(hipStreamCreateWithFlags(&h->duplex->side, hipStreamNonBlocking));
        RCA_HIP(hipEventCreateWithFlags(&h->duplex->ev_fork, hipEventDisableTiming));
        RCA_HIP(hipEventCreateWithFlags(&h->duplex->ev_join, hipEventDisableTiming));
    }
    DuplexState* d = h->duplex;
    const int F = F_ctx + n;
    const size_t pin_total = DuplexPinLayout(T, F_ctx, n_samples).total;
    if ((size_t)T > d->pcm_in_cap || (size_t)F > d->code_win_cap || (size_t)n_samples > d->pcm_out_cap || pin_total > d->pin_cap || !d->dev) {
        RCA_HIP(hipStreamSynchronize(st));
        duplex_drop_graphs(d);
        if ((rc = duplex_grow(&d->pcm_in, &d->pcm_in_cap, (size_t)T)) != RCA_OK) return rc;
        if ((rc = duplex_grow(&d->code_win, &d->code_win_cap, (size_t)F + 8)) != RCA_OK) return rc;
        if ((rc = duplex_grow(&d->pcm_out, &d->pcm_out_cap, (size_t)n_samples)) != RCA_OK) return rc;
        if (!d->dev && (rc = lm_alloc((void**)&d->dev, sizeof(DuplexDev))) != RCA_OK) return rc;
        if (pin_total > d->pin_cap) {
            if (d->pin) (void)hipHostFree(d->pin);
            d->pin = nullptr; d->pin_cap = 0;
            RCA_HIP(hipHostMalloc((void**)&d->pin, pin_total + (pin_total >> 2), hipHostMallocDefault));
            d->pin_cap = pin_total + (pin_total >> 2);
        }
    }
    return RCA_OK;
}
// The one-time allocations of rca_duplex_frame for a call shape (pinned staging, device buffers, side stream), so that a session can make
// them at reset() instead of inside its first one-replay frame (a pinned allocation costs milliseconds).  Optional.
extern "C" int rca_duplex_prepare(rca_lm_t* h, int32_t T, int32_t F_ctx, int32_t n_steps, int32_t n_samples) {
    if (!h || T < 1 || F_ctx < 0 || n_steps < 1 || n_steps > LM_FRAME_MAX || n_samples < 1) return fail(RCA_ERR_ARG, "duplex_prepare: bad shape");
    { const int src = lm_settle(h); if (src != RCA_OK) return src; }
    RCA_HIP(hipSetDevice(h->device));
    return duplex_reserve(h, T, F_ctx, n_steps, n_samples);
}

// An eager run (or the precapture's two tail calls) has sized the codec workspace of this call shape: record the shape as warmed under
// the signature the workspace has now, and key the shape's graph by it.
static int duplex_mark_warm(DuplexState* d, DuplexState::Entry* ent, const rca_duplex_frame_args_t* a, rca_codec_t* codec) {
    uint64_t sig = 0;
    const int rc = rca_codec_workspace_sig(codec, &sig);
    if (rc != RCA_OK) return rc;
    if (d->warm.size() >= 16) d->warm.clear();
    d->warm.push_back(DuplexState::Warm{a->T, a->F_ctx, a->n_steps, a->n_samples, (const void*)codec, sig});
    ent->key.codec_sig = sig;
    return RCA_OK;
}

// cap_bucket < 0: run the frame.  cap_bucket >= 0 (rca_duplex_precapture): make sure the graph of this call shape exists for that
// context bucket on the KV cache currently installed -- nothing is launched except, once per shape, the codec's two tail calls on
// scratch buffers (they size its workspace; a capture must not allocate) -- and return.
static int duplex_frame_core(rca_lm_t* h, rca_codec_t* codec, const rca_duplex_frame_args_t* a, rca_duplex_frame_out_t* out,
                             float* pcm_out_host, int cap_bucket) {
    const bool cap_only = cap_bucket >= 0;
    if (!h || !codec || !a || (!cap_only && (!out || !pcm_out_host || !a->pcm_window || (a->F_ctx > 0 && !a->code_ctx)))) return fail(RCA_ERR_ARG, "duplex_frame: null argument");
    const int n = a->n_steps;
    if (n < 1 || n > LM_FRAME_MAX) return fail(RCA_ERR_ARG, "duplex_frame: %d steps (1..%d)", n, LM_FRAME_MAX);
    if (a->T < 1 || a->F_ctx < 0 || a->n_samples < 1) return fail(RCA_ERR_ARG, "duplex_frame: bad shape (T=%d F_ctx=%d n_samples=%d)", a->T, a->F_ctx, a->n_samples);
    if (!h->sampler_set) return fail(RCA_ERR_STATE, "sampler not initialised");
    if (h->cfg.logits_all) return fail(RCA_ERR_STATE, "duplex_frame: not on a logits_all handle");
    if (!cap_only && h->n_tokens + 2 * n > h->cfg.n_ctx) return fail(RCA_ERR_STATE, "context overflow: %d + %d > n_ctx %d", h->n_tokens, 2 * n, h->cfg.n_ctx);
    int32_t n_codes = 0;
    int rc;
    if ((rc = rca_codec_codebook_size(codec, &n_codes)) != RCA_OK) return rc;
    if (a->code_token_base < 0 || (long)a->code_token_base + n_codes > h->cfg.vocab_size) return fail(RCA_ERR_ARG, "duplex_frame: codes [%d, %d + %d) fall outside the vocabulary", a->code_token_base, a->code_token_base, n_codes);
    for (int i = 0; i < 2; ++i)
        if (a->first_pair[i] < 0 || a->first_pair[i] >= h->cfg.vocab_size) return fail(RCA_ERR_ARG, "duplex_frame: token id %d outside the vocabulary", a->first_pair[i]);
    if (a->probe_id >= h->cfg.vocab_size) return fail(RCA_ERR_ARG, "duplex_frame: probe id %d outside the vocabulary", a->probe_id);
    for (int i = 0; !cap_only && i < a->F_ctx; ++i)
        if (a->code_ctx[i] < 0 || a->code_ctx[i] >= n_codes) return fail(RCA_ERR_ARG, "decode: code out of range [0, %d)", n_codes);
    { const int src = lm_settle(h); if (src != RCA_OK) return src; }
    RCA_HIP(hipSetDevice(h->device));
    hipStream_t st = h->stream;
    if ((rc = duplex_reserve(h, a->T, a->F_ctx, n, a->n_samples)) != RCA_OK) return rc;
    DuplexState* d = h->duplex;
    const int F = a->F_ctx + n;
    const DuplexPinLayout lay(a->T, a->F_ctx, a->n_samples);
    if (d->logits_at_capture != (const void*)h->logits) { duplex_drop_graphs(d); d->logits_at_capture = h->logits; }
    DuplexPin* pin = reinterpret_cast<DuplexPin*>(d->pin);
    // stage the inputs
    lm_stage_state(h, a->first_pair, 2);
    for (int i = 0; i < n; ++i) h->h_stt->ids[LM_FRAME_USER0 + i] = 0;
    pin->probe_id = a->probe_id >= 0 ? a->probe_id : 0;
    if (!cap_only) {
        memcpy(d->pin + lay.pcm, a->pcm_window, (size_t)a->T * 4);
        if (a->F_ctx) memcpy(d->pin + lay.codes, a->code_ctx, (size_t)a->F_ctx * 8);
    }
    const LmBucket bk = lm_bucket(h, 2 * n, cap_bucket);
    uint64_t csig = 0;
    if ((rc = rca_codec_workspace_sig(codec, &csig)) != RCA_OK) return rc;
    DuplexGraphKey key{a->T, a->F_ctx, n, a->n_samples, a->probe_id >= 0 ? 1 : 0, bk.bucket, a->code_token_base, (const void*)h->kc, csig, (const void*)codec};
    DuplexState::Entry* ent = nullptr;
    for (auto& e : d->graphs)
        if (e.key == key) ent = &e;
    if (!ent) {
        if (d->graphs.size() >= 32) { RCA_HIP(hipStreamSynchronize(st)); duplex_drop_graphs(d); }   // stale shapes / caches: start over
        d->graphs.push_back(DuplexState::Entry{key, nullptr});
        ent = &d->graphs.back();
    }
    bool warmed = false;
    for (auto& w : d->warm)
        warmed = warmed || (w.T == a->T && w.F_ctx == a->F_ctx && w.n_steps == n && w.n_samples == a->n_samples && w.codec == (const void*)codec && w.codec_sig == csig);
    auto enqueue = [&]() -> int {
        hipError_t e = hipMemcpyAsync(h->stt, h->h_stt, LM_STATE_DECODE_BYTES, hipMemcpyHostToDevice, st);
        if (e == hipSuccess) e = hipMemcpyAsync(d->pcm_in, d->pin + lay.pcm, (size_t)a->T * 4, hipMemcpyHostToDevice, st);
        if (e == hipSuccess && a->F_ctx) e = hipMemcpyAsync(d->code_win, d->pin + lay.codes, (size_t)a->F_ctx * 8, hipMemcpyHostToDevice, st);
        if (e == hipSuccess) e = hipMemcpyAsync(&d->dev->probe_id, &pin->probe_id, 4, hipMemcpyHostToDevice, st);
        if (e != hipSuccess) return fail(RCA_ERR_HIP, "duplex h2d: %s", hipGetErrorString(e));
        // Step 0 evaluates the PREVIOUS frame's pair: this chunk's codes are first needed by the sampler tail of step 0, which makes
        // [token just sampled, user's code 0] the next pair.  The encode tail therefore runs on a side branch beside step 0's layers
        // (a dozen latency-bound launches of a few workgroups each) and joins in front of step 0's sampler.
        hipStream_t se = d->fork ? d->side : st;
        if (d->fork) {
            e = hipEventRecord(d->ev_fork, st);
            if (e == hipSuccess) e = hipStreamWaitEvent(se, d->ev_fork, 0);
            if (e != hipSuccess) return fail(RCA_ERR_HIP, "duplex fork: %s", hipGetErrorString(e));
        }
        int r = rca_codec_encode_tail_dev(codec, d->pcm_in, 1, a->T, n, (int64_t*)d->dev->user_codes, se);
        if (r != RCA_OK) return r;
        duplex_codes_to_ids_kernel<<<1, 64, 0, se>>>(d->dev->user_codes, n, a->code_token_base, h->stt, &d->dev->flags);
        if (d->fork) {
            e = hipEventRecord(d->ev_join, se);
            if (e != hipSuccess) return fail(RCA_ERR_HIP, "duplex join: %s", hipGetErrorString(e));
        }
        for (int i = 0; i < n; ++i) {
            if ((r = lm_enqueue_pass(h, 2, 1, st, bk.nsp_launch, i > 0)) != RCA_OK) return r;
            if (i == 0 && d->fork) {
                e = hipStreamWaitEvent(st, d->ev_join, 0);
                if (e != hipSuccess) return fail(RCA_ERR_HIP, "duplex join: %s", hipGetErrorString(e));
            }
            lm_enqueue_sample(h, h->logits, st, i);
        }
        duplex_tokens_to_codes_kernel<<<1, 64, 0, st>>>(h->stt, n, a->code_token_base, n_codes, d->code_win + a->F_ctx, &d->dev->flags);
        if ((r = rca_codec_decode_tail_dev(codec, (const int64_t*)d->code_win, 1, F, a->n_samples, d->pcm_out, st)) != RCA_OK) return r;
        if (a->probe_id >= 0) {
            lm_softmax_slices_kernel<<<PROBS_SLICES, 1024, 0, st>>>(h->logits, h->cfg.vocab_size, h->probs_dev + 64);
            lm_token_probs_kernel<<<1, 64, 0, st>>>(h->logits, h->cfg.vocab_size, h->probs_dev + 64, &d->dev->probe_id, 1, &d->dev->probe_prob);
        }
        RCA_LAUNCH_CHECK();
        e = hipMemcpyAsync(pin->frame_out, h->stt->frame_out, sizeof(int) * LM_FRAME_MAX, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipMemcpyAsync(pin->user_codes, d->dev->user_codes, sizeof(long long) * LM_FRAME_MAX + 8, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipMemcpyAsync(d->pin + lay.out, d->pcm_out, (size_t)a->n_samples * 4, hipMemcpyDeviceToHost, st);
        if (e != hipSuccess) return fail(RCA_ERR_HIP, "duplex d2h: %s", hipGetErrorString(e));
        return RCA_OK;
    };
    // the codec's ordering moves to this stream (nothing of it is in flight elsewhere once this returns)
    if ((rc = rca_codec_stream_handoff(codec, d->fork ? d->side : st)) != RCA_OK) return rc;
    if (cap_only && !warmed) {
        // size the codec workspace of this shape without touching the LM: the two tail calls on zeroed scratch input
        hipStream_t se = d->fork ? d->side : st;
        RCA_HIP(hipMemsetAsync(d->pcm_in, 0, (size_t)a->T * 4, se));
        RCA_HIP(hipMemsetAsync(d->code_win, 0, (size_t)F * 8, se));
        if ((rc = rca_codec_encode_tail_dev(codec, d->pcm_in, 1, a->T, n, (int64_t*)d->dev->user_codes, se)) != RCA_OK) return rc;
        if ((rc = rca_codec_decode_tail_dev(codec, (const int64_t*)d->code_win, 1, F, a->n_samples, d->pcm_out, se)) != RCA_OK) return rc;
        RCA_HIP(hipStreamSynchronize(se));
        if ((rc = duplex_mark_warm(d, ent, a, codec)) != RCA_OK) return rc;
        warmed = true;
    }
    const bool want_graph = h->graphs_enabled && warmed;
    // the eager frame before this one sized every workspace buffer of this shape: nothing allocates under capture (a workspace that
    // moved under the eager run, the first call of a shape, would have changed the signature: checked by the key)
    if (want_graph && !ent->exec && (rc = lm_capture(st, &ent->exec, "duplex", enqueue)) != RCA_OK) return rc;
    if (cap_only) return RCA_OK;
    if (want_graph) {
        RCA_HIP(hipGraphLaunch(ent->exec, st));
    } else if ((rc = enqueue()) != RCA_OK) {
        return rc;
    }
    RCA_HIP(hipStreamSynchronize(st));
    // the eager run may have (re)allocated codec workspace: graphs are keyed by the signature after it
    if (!warmed && (rc = duplex_mark_warm(d, ent, a, codec)) != RCA_OK) return rc;
    int done = n;
    for (int i = 0; i < n; ++i) {
        out->tokens[i] = pin->frame_out[i];
        out->user_codes[i] = pin->user_codes[i];
        if (out->tokens[i] <= a->audio_id_floor) { done = i + 1; break; }
    }
    for (int i = done; i < n; ++i) { out->tokens[i] = -1; out->user_codes[i] = pin->user_codes[i]; }
    out->n_done = done;
    out->flags = pin->flags | (done < n ? 2 : 0);
    out->probe_prob = (a->probe_id >= 0 && done == n) ? pin->probe_prob : -1.0f;
    if (out->flags == 0) memcpy(pcm_out_host, d->pin + lay.out, (size_t)a->n_samples * 4);
    h->n_tokens += 2 * done;
    h->logits_rows = done < n ? 0 : 1;
    h->rng_host += (unsigned long long)done;
    if (done < n) RCA_HIP(hipMemcpy(&h->stt->rng_counter, &h->rng_host, 8, hipMemcpyHostToDevice));
    return RCA_OK;
}

extern "C" int rca_duplex_frame(rca_lm_t* h, rca_codec_t* codec, const rca_duplex_frame_args_t* a, rca_duplex_frame_out_t* out,
                                float* pcm_out_host) {
    return duplex_frame_core(h, codec, a, out, pcm_out_host, -1);
}

static int lm_step_capture_only(rca_lm_t* h, int n, int n_probe, int bucket);

// Captures, ahead of the first frame, every graph the one-replay frame of this call shape can need: one per context bucket the
// handle's n_ctx can reach, on the KV cache installed in `h` and -- when the session trims through a shadow cache (kv_shadow.py:
// the two caches trade places at every trim) -- on `twin`'s as well; plus, with n_probe > 0, the one-token step + n_probe
// probabilities of the agent's speculative <|end_audio|> step (rca_lm_step_probe).  Called at session start (reset()): no frame of
// the session then pays a capture (in round 3 the first frame of every bucket and the first trim frame did: 10-14 ms against a
// median of 4.7).  a->pcm_window / code_ctx / first_pair are not read.
extern "C" int rca_duplex_precapture(rca_lm_t* h, rca_lm_t* twin, rca_codec_t* codec, const rca_duplex_frame_args_t* a, int32_t n_probe) {
    if (!h || !codec || !a) return fail(RCA_ERR_ARG, "duplex_precapture: null argument");
    if (!h->sampler_set) return fail(RCA_ERR_STATE, "sampler not initialised");
    if (!h->graphs_enabled) return RCA_OK;
    if (twin && (twin == h || twin->cfg.n_ctx != h->cfg.n_ctx || twin->n_splits != h->n_splits)) return fail(RCA_ERR_ARG, "duplex_precapture: the twin must be another handle of the same n_ctx");
    { const int src = lm_settle(h); if (src != RCA_OK) return src; }
    if (twin) { const int src = lm_settle(twin); if (src != RCA_OK) return src; }
    int rc = RCA_OK;
    for (int pass = 0; pass < (twin ? 2 : 1) && rc == RCA_OK; ++pass) {
        if (pass == 1) { std::swap(h->kc, twin->kc); std::swap(h->vc, twin->vc); }      // host pointers only: nothing runs under capture
        for (int b = 0; b < LM_GRAPH_BUCKETS && rc == RCA_OK; ++b) {
            if (!lm_bucket_reachable(h, b)) break;
            rc = duplex_frame_core(h, codec, a, nullptr, nullptr, b);
            if (rc == RCA_OK && n_probe > 0) rc = lm_step_capture_only(h, 1, n_probe, b);
            // the frames that cannot take the one-replay path (a trim, a text branch) replay the LM chunk or single steps
            if (rc == RCA_OK) {
                const int32_t pair[2] = {0, 0}, users[LM_FRAME_MAX] = {0, 0, 0, 0, 0, 0, 0, 0};
                int32_t toks[LM_FRAME_MAX], done = 0;
                rc = lm_frame_core(h, pair, users, a->n_steps, -1, toks, &done, b);
            }
            if (rc == RCA_OK) rc = lm_step_capture_only(h, 2, 0, b);
        }
        if (pass == 1) { std::swap(h->kc, twin->kc); std::swap(h->vc, twin->vc); }
    }
    return rc;
}

extern "C" int rca_lm_token_probs(rca_lm_t* h, const int32_t* token_ids, int32_t n, float* probs_out) {
    if (!h || !token_ids || !probs_out || n < 1 || n > 64) return fail(RCA_ERR_ARG, "token_probs: 1..64 ids");
    { const int src = lm_settle(h); if (src != RCA_OK) return src; }
    if (h->logits_rows < 1) return fail(RCA_ERR_STATE, "no logits: call eval first");
    RCA_HIP(hipSetDevice(h->device));
    hipStream_t st = h->stream;
    RCA_HIP(hipMemcpyAsync(h->probe_ids_dev, token_ids, n * 4, hipMemcpyHostToDevice, st));
    const float* lg = h->logits + (long)(h->logits_rows - 1) * h->cfg.vocab_size;
    lm_softmax_slices_kernel<<<PROBS_SLICES, 1024, 0, st>>>(lg, h->cfg.vocab_size, h->probs_dev + 64);
    lm_token_probs_kernel<<<1, 64, 0, st>>>(lg, h->cfg.vocab_size, h->probs_dev + 64, h->probe_ids_dev, n, h->probs_dev);
    RCA_LAUNCH_CHECK();
    RCA_HIP(hipMemcpyAsync(probs_out, h->probs_dev, n * 4, hipMemcpyDeviceToHost, st));
    RCA_HIP(hipStreamSynchronize(st));
    return RCA_OK;
}

// switch between "logits of every evaluated position" (llama_cpp's logits_all) and "last position only"
extern "C" int rca_lm_set_logits_all(rca_lm_t* h, int32_t enable) {
    if (!h) return fail(RCA_ERR_ARG, "null");
    if ((h->cfg.logits_all != 0) != (enable != 0)) {
        RCA_HIP(hipSetDevice(h->device));
        RCA_HIP(hipStreamSynchronize(h->stream));
        { const int rc = lm_wait_batch_eval(h); if (rc != RCA_OK) return rc; }
        lm_drop_graphs(h);   // a later eval may move the logits buffer; nothing captured before the switch is replayed after it
    }
    h->cfg.logits_all = enable != 0;
    return RCA_OK;
}

// test / bench knob: disable graph replay (eager launches) to compare
extern "C" int rca_lm_set_graphs(rca_lm_t* h, int32_t enable) {
    if (!h) return fail(RCA_ERR_ARG, "null");
    h->graphs_enabled = enable != 0;
    return RCA_OK;
}

__global__ __launch_bounds__(256) void lm_q8_zero_row_scales_kernel(unsigned* __restrict__ sc, int nblk, int row_begin, int row_end) {
    const long total = (long)(row_end - row_begin) * nblk;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int row = row_begin + (int)(i / nblk), j = (int)(i % nblk);
        unsigned short* half = reinterpret_cast<unsigned short*>(sc + q8_sc_index(row >> 1, j, nblk)) + (row & 1);
        *half = 0;
    }
}
__global__ __launch_bounds__(256) void lm_q6k_zero_row_scales_kernel(float* __restrict__ sc, int nk16, int row_begin, int row_end) {
    const long total = (long)(row_end - row_begin) * nk16;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int row = row_begin + (int)(i / nk16), j = (int)(i % nk16);
        sc[2 * q8_sc_index(row >> 1, j, nk16) + (row & 1)] = 0.0f;
    }
}
__global__ __launch_bounds__(256) void lm_q4k_zero_row_factors_kernel(unsigned* __restrict__ dd, int nk256, int row_begin, int row_end) {
    const long total = (long)(row_end - row_begin) * nk256;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int row = row_begin + (int)(i / nk256), j = (int)(i % nk256);
        dd[q4k_scm_index(row, j, nk256)] = 0u;   // lm_head is packed with plain slots: slot == row
    }
}
__global__ __launch_bounds__(256) void lm_zero_rows_kernel(bf16_t* __restrict__ w, long n) {
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) w[i] = 0;
}
// zero lm_head rows [row_begin, row_end): used with random-init weights so that, like a trained codec LM in
// audio mode, the sampler's top-k only ever holds codec tokens (text rows get logit 0)
extern "C" int rca_lm_mask_head_rows(rca_lm_t* h, int32_t row_begin, int32_t row_end) {
    if (!h || row_begin < 0 || row_end > h->cfg.vocab_size || row_begin > row_end) return fail(RCA_ERR_ARG, "mask_head_rows: bad range");
    RCA_HIP(hipSetDevice(h->device));
    const long n = (long)(row_end - row_begin) * h->cfg.hidden;
    // a row of a packed head is zero when its factors are: the table names their array and how many values share one
    const WfInfo& info = WF_TABLE[h->head.fmt];
    void* arr = *h->head.array(info.mask.arr);
    const int per_row = h->cfg.hidden / info.mask.per;
    if (n > 0) switch (info.device) {
        case WF_BF16: case WF_F16: lm_zero_rows_kernel<<<2048, 256, 0, h->stream>>>(h->head.w + (long)row_begin * h->cfg.hidden, n); break;   // zero bits
        case WF_Q8: lm_q8_zero_row_scales_kernel<<<256, 256, 0, h->stream>>>((unsigned*)arr, per_row, row_begin, row_end); break;   // the block scales
        case WF_Q6K: lm_q6k_zero_row_scales_kernel<<<256, 256, 0, h->stream>>>((float*)arr, per_row, row_begin, row_end); break;   // the row's f32 scales
        // Q4_K / Q5_K: d = dmin = 0 makes every value of the row (0 * sc) * q - (0 * m) = 0.  Q4_0 / Q4_1: s = t = 0 gives 0 * q - 0 = 0, IQ4: s = 0
        // (the f32's zero bits) gives 0 * kv[q] = 0 (the same slot-grouped index, per 32 values)
        default: lm_q4k_zero_row_factors_kernel<<<256, 256, 0, h->stream>>>((unsigned*)arr, per_row, row_begin, row_end); break;
    }
    RCA_LAUNCH_CHECK();
    RCA_HIP(hipStreamSynchronize(h->stream));
    return RCA_OK;
}

// ------------------------------------------------------------------------------------- persist_codec_embeddings
// The reference's deployment step (codec_llama.py:178-206): every codec token's input embedding is the projector output
// linear_2(gelu(linear_1(codec_embed[code]))) (codec_llama.py:32-44, exact erf GELU) and is baked into the plain embedding
// table so the deployed model is a vanilla Llama.  Done here on the device for a checkpoint that still carries the frozen
// codec embedding + projector: a small elementwise kernel for the 16 -> H layer, then an H x H f32 GEMM on
// v_mfma_f32_32x32x2_f32 (code rows x features; one 32 x 32 tile per wave, operands straight from L2 -- a load-time
// operation, 1.1 TFLOP for the 1B model), bias added and rounded to bf16 (nearest even) into the table rows.
__global__ __launch_bounds__(256) void lm_codec_proj1_kernel(const float* __restrict__ e, const float* __restrict__ w1, const float* __restrict__ b1,
                                                             float* __restrict__ h1, int rows, int dim, int H) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long)rows * H) return;
    const int r = (int)(i / H), j = (int)(i - (long)r * H);
    float acc = 0.0f;
    for (int d = 0; d < dim; ++d) acc = __builtin_fmaf(w1[(long)j * dim + d], e[(long)r * dim + d], acc);
    const float x = acc + b1[j];
    h1[i] = 0.5f * x * (1.0f + erff(x * 0.70710678118654752440f));
}

__global__ __launch_bounds__(256) void lm_codec_proj2_kernel(const float* __restrict__ h1, const float* __restrict__ w2, const float* __restrict__ b2,
                                                             void* __restrict__ table_rows, int f32tab, float* __restrict__ out_f32, int rows, int H) {
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int r32 = lane & 31, hs = lane >> 5;
    const int n0 = blockIdx.y * 32, f0 = (blockIdx.x * 4 + wave) * 32;
    if (f0 >= H) return;
    // A = h1 (code rows), B = w2 (feature rows), both contiguous along k; a lane takes 4 consecutive k of its row per 8-block
    // (k half `hs`), so MFMA step s of a block multiplies k0+s (half 0) and k0+4+s (half 1): same pairing on both operands.
    const float* ap = h1 + (long)min(n0 + r32, rows - 1) * H + hs * 4;
    const float* bp = w2 + (long)min(f0 + r32, H - 1) * H + hs * 4;
    f32x16 acc;
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = 0.0f;
    for (int k0 = 0; k0 < H; k0 += 8) {
        const f32x4 a = *reinterpret_cast<const f32x4*>(ap + k0);
        const f32x4 b = *reinterpret_cast<const f32x4*>(bp + k0);
#pragma unroll
        for (int s = 0; s < 4; ++s) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[s], b[s], acc, 0, 0, 0);
    }
    const int f = f0 + r32;   // accumulator i of lane: code row 8*(i/4) + 4*hs + i%4, feature r32
    if (f >= H) return;
    const float bias = b2[f];
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int n = n0 + 8 * (i / 4) + 4 * hs + (i & 3);
        if (n < rows) {
            const float v = acc[i] + bias;
            if (f32tab) reinterpret_cast<float*>(table_rows)[(long)n * H + f] = v;   // an f32 table keeps the projector output as it is
            else reinterpret_cast<bf16_t*>(table_rows)[(long)n * H + f] = f32_to_bf16_rne(v);
            if (out_f32) out_f32[(long)n * H + f] = v;
        }
    }
}

extern "C" int rca_lm_persist_codec_embeddings(rca_lm_t* h, const float* codec_embed, int32_t n_codes, int32_t dim, const float* w1,
                                               const float* b1, const float* w2, const float* b2, int32_t codec_vocab_start, float* out_f32) {
    if (!h || !codec_embed || !w1 || !b1 || !w2 || !b2) return fail(RCA_ERR_ARG, "persist_codec_embeddings: null argument");
    const int H = h->cfg.hidden;
    if (n_codes <= 0 || dim <= 0 || codec_vocab_start < 0 || (long)codec_vocab_start + n_codes > h->cfg.vocab_size)
        return fail(RCA_ERR_ARG, "persist_codec_embeddings: rows [%d, %ld) are outside the vocabulary of %d", codec_vocab_start,
                    (long)codec_vocab_start + n_codes, h->cfg.vocab_size);
    if (H % 8) return fail(RCA_ERR_ARG, "persist_codec_embeddings: hidden size must be a multiple of 8");
    RCA_HIP(hipSetDevice(h->device));
    const int chunk = std::min<int>(n_codes, 8192);
    float *de = nullptr, *dw1 = nullptr, *db1 = nullptr, *dw2 = nullptr, *db2 = nullptr, *dh1 = nullptr, *dout = nullptr;
    auto free_all = [&]() { for (float* p : {de, dw1, db1, dw2, db2, dh1, dout}) if (p) (void)hipFree(p); };
    auto up = [&](float** d, const float* src, size_t n) {
        if (hipMalloc((void**)d, n * 4) != hipSuccess) return false;
        return hipMemcpy(*d, src, n * 4, hipMemcpyHostToDevice) == hipSuccess;
    };
    if (!up(&de, codec_embed, (size_t)n_codes * dim) || !up(&dw1, w1, (size_t)H * dim) || !up(&db1, b1, H) || !up(&dw2, w2, (size_t)H * H) ||
        !up(&db2, b2, H) || hipMalloc((void**)&dh1, (size_t)chunk * H * 4) != hipSuccess ||
        (out_f32 && hipMalloc((void**)&dout, (size_t)chunk * H * 4) != hipSuccess)) {
        free_all();
        return fail(RCA_ERR_HIP, "persist_codec_embeddings: device allocation / upload failed");
    }
    for (int r0 = 0; r0 < n_codes; r0 += chunk) {
        const int rows = std::min(chunk, n_codes - r0);
        lm_codec_proj1_kernel<<<(unsigned)(((long)rows * H + 255) / 256), 256, 0, h->stream>>>(de + (long)r0 * dim, dw1, db1, dh1, rows, dim, H);
        lm_codec_proj2_kernel<<<dim3((H + 127) / 128, (rows + 31) / 32), 256, 0, h->stream>>>(
            dh1, dw2, db2, (char*)h->embed + ((long)codec_vocab_start + r0) * H * (h->embed_f32 ? 4 : 2), h->embed_f32, dout, rows, H);
        hipError_t e = hipGetLastError();
        if (e == hipSuccess && out_f32) e = hipMemcpyAsync(out_f32 + (long)r0 * H, dout, (size_t)rows * H * 4, hipMemcpyDeviceToHost, h->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
        if (e != hipSuccess) { free_all(); return fail(RCA_ERR_HIP, "persist_codec_embeddings: %s", hipGetErrorString(e)); }
    }
    free_all();
    return RCA_OK;
}

// test / bench knob: merge the attention splits inside the attention launch (1, default) or in a launch of its own (0)
extern "C" int rca_lm_set_attn_fuse(rca_lm_t* h, int32_t enable) {
    if (!h) return fail(RCA_ERR_ARG, "null");
    { const int src = lm_settle(h); if (src != RCA_OK) return src; }
    RCA_HIP(hipSetDevice(h->device));
    RCA_HIP(hipStreamSynchronize(h->stream));
    if (h->fuse_attn != (enable != 0)) lm_drop_graphs(h);
    h->fuse_attn = enable != 0;
    return RCA_OK;
}
// Activation format of the decode GEMVs over packed (q8_0 / Q4_K / Q5_K / Q6_K) matrices: 0 = f32, 1 = q8_1 blocks + integer dot products
// (lm_gemv_kernel<..., ACT = 1>).  The exact prefill route is made of the same launches and follows; the MFMA tiles do not.
static bool lm_has_packed_matrix(const rca_lm* h) {
    auto packed = [](const WMat& m) { return wf_packed(m.fmt); };
    bool any = packed(h->head);
    for (const LmLayer& L : h->layers) any = any || packed(L.qkv) || packed(L.o) || packed(L.gu) || packed(L.down) || (L.split_v && packed(L.vseg));
    return any;
}
extern "C" int rca_lm_set_act_format(rca_lm_t* h, int32_t fmt) {
    if (!h) return fail(RCA_ERR_ARG, "null");
    if (fmt != 0 && fmt != 1) return fail(RCA_ERR_ARG, "set_act_format: %d is neither 0 (f32) nor 1 (q8_1)", fmt);
    if (fmt == 1 && !lm_has_packed_matrix(h))
        return fail(RCA_ERR_ARG, "set_act_format: q8_1 activations need a q8_0 / Q4_K / Q6_K, Q5_K, Q4_0 / Q4_1 or IQ4_NL / IQ4_XS projection matrix, and this handle keeps all of its matrices in 16-bit floats");
    { const int src = lm_settle(h); if (src != RCA_OK) return src; }
    if (h->act_format != fmt) {
        RCA_HIP(hipSetDevice(h->device));
        RCA_HIP(hipStreamSynchronize(h->stream));
        lm_drop_graphs(h);   // the captured steps hold the other instances
    }
    h->act_format = fmt;
    return RCA_OK;
}
extern "C" int rca_lm_get_act_format(const rca_lm_t* h, int32_t* fmt) {
    if (!h || !fmt) return fail(RCA_ERR_ARG, "null");
    *fmt = h->act_format;
    return RCA_OK;
}
// Format of the KV cache: 0 = fp16 (default), 1 = q8_0 blocks (the comment above lm_kv_quant_kernel).  Only an empty handle (n_tokens == 0)
// can change it: the cache is re-allocated (zeroed) in the new format and every captured graph goes.
extern "C" int rca_lm_set_kv_format(rca_lm_t* h, int32_t fmt) {
    if (!h) return fail(RCA_ERR_ARG, "null");
    if (fmt != 0 && fmt != 1) return fail(RCA_ERR_ARG, "set_kv_format: %d is neither 0 (f16) nor 1 (q8_0)", fmt);
    if (h->cfg.head_dim != 64) return fail(RCA_ERR_ARG, "set_kv_format: head_dim %d (the cache kernels take 64)", h->cfg.head_dim);
    if (h->n_tokens != 0) return fail(RCA_ERR_STATE, "set_kv_format: the cache holds %d positions; the format changes on an empty handle only (rca_lm_reset)", h->n_tokens);
    { const int src = lm_settle(h); if (src != RCA_OK) return src; }
    if (h->kv_format == fmt) return RCA_OK;
    RCA_HIP(hipSetDevice(h->device));
    RCA_HIP(hipStreamSynchronize(h->stream));
    lm_drop_graphs(h);   // the captured passes hold the old cache and the other kernel instances
    const int old = h->kv_format;
    h->kv_format = fmt;
    const int rc = lm_kv_alloc(h);
    if (rc != RCA_OK) { h->kv_format = old; (void)lm_kv_alloc(h); return rc; }
    if (fmt == 0) h->kv_shift_requant = 0;   // the permission belongs to the q8_0 cache that has just gone
    RCA_HIP(hipStreamSynchronize(h->stream));
    return RCA_OK;
}
// q8_0 handles only: 1 lets rca_lm_kv_remove / rca_lm_kv_remove_many de-quantise, rotate and RE-QUANTISE the keys they move (the comment
// above lm_kv_shift_unit_q8); 0 (default) keeps their refusal.  A permission and nothing else: allowed at any n_tokens, no cache is
// touched, no graph is dropped.
extern "C" int rca_lm_set_kv_shift_requant(rca_lm_t* h, int32_t on) {
    if (!h) return fail(RCA_ERR_ARG, "null");
    if (on != 0 && on != 1) return fail(RCA_ERR_ARG, "set_kv_shift_requant: %d is neither 0 nor 1", on);
    if (!lm_kv_q8(h)) return fail(RCA_ERR_STATE, "set_kv_shift_requant: this handle keeps an fp16 KV cache, whose context shift quantises nothing (rca_lm_set_kv_format)");
    h->kv_shift_requant = on;
    return RCA_OK;
}
extern "C" int rca_lm_get_kv_shift_requant(const rca_lm_t* h, int32_t* on) {
    if (!h || !on) return fail(RCA_ERR_ARG, "null");
    *on = h->kv_shift_requant;
    return RCA_OK;
}
extern "C" int rca_lm_get_kv_format(const rca_lm_t* h, int32_t* fmt) {
    if (!h || !fmt) return fail(RCA_ERR_ARG, "null");
    *fmt = h->kv_format;
    return RCA_OK;
}
// bytes one cached position takes in the handle's format (all layers, K and V); ring_positions (may be null): positions of the fp16
// staging ring of a q8_0 cache, 0 for an fp16 cache
extern "C" int rca_lm_kv_bytes_per_position(const rca_lm_t* h, int64_t* bytes, int32_t* ring_positions) {
    if (!h || !bytes) return fail(RCA_ERR_ARG, "null");
    *bytes = lm_kv_bytes_per_pos(h);
    if (ring_positions) *ring_positions = lm_kv_q8(h) ? LM_KV_RING : 0;
    return RCA_OK;
}
// tests only: one decode GEMV stage, launched by the very call lm_enqueue_pass makes for it, on a host-supplied input
extern "C" int rca_lm_gemv_tap(rca_lm_t* h, int32_t layer, int32_t kind, const float* x_host, int32_t M, float* y_host, int64_t y_numel,
                               uint16_t* kv_host) {
    if (!h || !x_host || !y_host) return fail(RCA_ERR_ARG, "null");
    const rca_lm_config_t& c = h->cfg;
    const int H = c.hidden, QKV = (c.n_heads + 2 * c.n_kv_heads) * c.head_dim, AO = c.n_heads * c.head_dim, F = c.ffn, V = c.vocab_size;
    if (kind < 0 || kind > 4) return fail(RCA_ERR_ARG, "gemv_tap: kind %d outside [0, 4]", kind);
    if (M < 1 || M > LM_GEMV_M) return fail(RCA_ERR_ARG, "gemv_tap: M = %d, a decode pass has 1 or %d tokens", M, LM_GEMV_M);
    if (kind != 4 && (layer < 0 || layer >= c.n_layers)) return fail(RCA_ERR_ARG, "gemv_tap: layer %d outside [0, %d)", layer, c.n_layers);
    if (h->n_tokens + M > c.n_ctx) return fail(RCA_ERR_STATE, "gemv_tap: positions %d .. %d are outside the context of %d", h->n_tokens, h->n_tokens + M - 1, c.n_ctx);
    const int in_w[5] = {H, AO, H, F, H}, out_w[5] = {AO, H, F, H, V};
    if (y_numel != (int64_t)M * out_w[kind]) return fail(RCA_ERR_ARG, "gemv_tap: y_numel %ld, kind %d writes %d x %d values", (long)y_numel, kind, M, out_w[kind]);
    { const int src = lm_settle(h); if (src != RCA_OK) return src; }
    RCA_HIP(hipSetDevice(h->device));
    hipStream_t st = h->stream;
    RCA_HIP(hipStreamSynchronize(st));
    const int32_t ids[LM_GEMV_M] = {};
    int rc;
    if ((rc = lm_push_state(h, ids, M, st)) != RCA_OK) return rc;
    float* xin = kind == 1 ? h->attn : (kind == 3 ? h->hbuf : h->x);
    RCA_HIP(hipMemcpyAsync(xin, x_host, (size_t)M * in_w[kind] * 4, hipMemcpyHostToDevice, st));
    const float* yd = nullptr;
    int ldy = out_w[kind];
    float* head_out = nullptr;
    // The region read back is filled with NaN (all bits set) before the launch: an element the stage does not write comes back as NaN.
    // Kinds 1 and 3 add to a residual that must be zero, so they cannot be pre-filled: there the caller uses data whose every output
    // is non-zero.  The head's temporary buffer carries a guard of GEMV_TAP_GUARD floats of another pattern behind row M - 1.
    constexpr int GEMV_TAP_GUARD = 64;
    constexpr unsigned GEMV_TAP_SENTINEL = 0x7fa5a5a5u;   // a NaN with a payload no kernel produces
    memset(h->gemv_last, 0, sizeof h->gemv_last);
    if (kind == 0) {
        RCA_HIP(hipMemsetAsync(h->qkv, 0xff, (size_t)M * QKV * 4, st));
        lm_launch_qkv(h, layer, M, st);
        yd = h->qkv; ldy = QKV;
    } else if (kind == 1) {
        RCA_HIP(hipMemsetAsync(h->x, 0, (size_t)M * H * 4, st));
        lm_launch_o(h, layer, M, st);
        yd = h->x;
    } else if (kind == 2) {
        RCA_HIP(hipMemsetAsync(h->hbuf, 0xff, (size_t)M * F * 4, st));
        lm_launch_gu(h, layer, M, st);
        yd = h->hbuf;
    } else if (kind == 3) {
        RCA_HIP(hipMemsetAsync(h->x, 0, (size_t)M * H * 4, st));
        lm_launch_down(h, layer, M, st);
        yd = h->x;
    } else {
        if ((rc = lm_alloc((void**)&head_out, ((size_t)M * V + GEMV_TAP_GUARD) * 4)) != RCA_OK) return rc;   // the handle's own logits buffer may hold one row only
        hipError_t eh = hipMemsetAsync(head_out, 0xff, (size_t)M * V * 4, st);
        if (eh == hipSuccess) eh = hipMemsetD32Async((hipDeviceptr_t)(head_out + (size_t)M * V), (int)GEMV_TAP_SENTINEL, GEMV_TAP_GUARD, st);
        if (eh != hipSuccess) { (void)hipFree(head_out); return fail(RCA_ERR_HIP, "gemv_tap: %s", hipGetErrorString(eh)); }
        lm_launch_head(h, M, st, head_out, false);
        yd = head_out;
    }
    unsigned guard[GEMV_TAP_GUARD];
    hipError_t e = hipGetLastError();
    if (e == hipSuccess && head_out) e = hipMemcpyAsync(guard, head_out + (size_t)M * V, sizeof guard, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipMemcpy2DAsync(y_host, (size_t)out_w[kind] * 4, yd, (size_t)ldy * 4, (size_t)out_w[kind] * 4, M, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess && kind == 0 && kv_host && lm_kv_q8(h)) {   // the de-quantised rows, as rca_lm_kv_read gives them
        const size_t n = (size_t)M * c.n_kv_heads * 64;
        rc = lm_kv_read_deq(h, h->kc, layer, h->n_tokens, M, kv_host);
        if (rc == RCA_OK) rc = lm_kv_read_deq(h, h->vc, layer, h->n_tokens, M, kv_host + n);
        if (rc != RCA_OK) { if (head_out) (void)hipFree(head_out); return rc; }
    } else if (e == hipSuccess && kind == 0 && kv_host) {
        const size_t n = (size_t)M * c.n_kv_heads * 64;
        const long off = (long)layer * h->kv_layer_stride + (long)h->n_tokens * c.n_kv_heads * 64;
        e = hipMemcpyAsync(kv_host, h->kc + off, n * 2, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipMemcpyAsync(kv_host + n, h->vc + off, n * 2, hipMemcpyDeviceToHost, st);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (head_out) (void)hipFree(head_out);
    if (e != hipSuccess) return fail(RCA_ERR_HIP, "gemv_tap: %s", hipGetErrorString(e));
    if (kind == 4)
        for (int i = 0; i < GEMV_TAP_GUARD; ++i)
            if (guard[i] != GEMV_TAP_SENTINEL) return fail(RCA_ERR_STATE, "gemv_tap: the head wrote behind row %d of its output: guard float %d holds 0x%08x", M - 1, i, guard[i]);
    return RCA_OK;
}
// tests only: the instance and grid of the last decode GEMV the handle launched (rca_lm_gemv_tap sets the record to zeros before its
// launch): M, NIT, R, batches per workgroup, grid, format id (WF_*), ACT, N.  A stage of two launches (a layer that keeps V apart)
// leaves the second one's.
extern "C" int rca_lm_gemv_tap_form(const rca_lm_t* h, int32_t* form) {
    if (!h || !form) return fail(RCA_ERR_ARG, "null");
    for (int i = 0; i < 8; ++i) form[i] = h->gemv_last[i];
    return RCA_OK;
}
// tests only: the attention of one layer alone, launched by the very call the passes make for it (launch_attention_mfma), for M host-supplied
// post-RoPE query rows at positions n_tokens .. n_tokens + M - 1 over whatever the cache holds (rca_lm_kv_write)
extern "C" int rca_lm_attn_tap(rca_lm_t* h, int32_t layer, int32_t route, int32_t nsp_launch, const float* q_host, int32_t M, float* out_host,
                               int32_t out_rows) {
    if (!h || !q_host || !out_host) return fail(RCA_ERR_ARG, "null");
    const rca_lm_config_t& c = h->cfg;
    const int QKV = (c.n_heads + 2 * c.n_kv_heads) * c.head_dim, AO = c.n_heads * c.head_dim;
    if (layer < 0 || layer >= c.n_layers) return fail(RCA_ERR_ARG, "attn_tap: layer %d outside [0, %d)", layer, c.n_layers);
    if (route < 0 || route > 2) return fail(RCA_ERR_ARG, "attn_tap: route %d outside [0, 2]", route);
    const int m_max = route == 0 ? LM_GEMV_M : LM_MAXM;
    if (M < 1 || M > m_max) return fail(RCA_ERR_ARG, "attn_tap: M = %d, route %d takes 1 .. %d query tokens", M, route, m_max);
    if (route == 2 && lm_prefill_route(h) != LM_ROUTE_TILE128)
        return fail(RCA_ERR_ARG, "attn_tap: route 2 is the attention of the gemm128 prefill route, which this handle does not take");
    if (h->n_tokens + M > c.n_ctx) return fail(RCA_ERR_STATE, "attn_tap: positions %d .. %d are outside the context of %d", h->n_tokens, h->n_tokens + M - 1, c.n_ctx);
    if (out_rows < M || out_rows > LM_MAXM) return fail(RCA_ERR_ARG, "attn_tap: out_rows %d outside [M = %d, %d]", out_rows, M, LM_MAXM);
    const int need = lm_splits_needed(h, M);
    if (nsp_launch == 0) nsp_launch = need;
    if (nsp_launch < need || nsp_launch > h->n_splits)
        return fail(RCA_ERR_ARG, "attn_tap: nsp_launch %d outside [%d needed, %d splits]", nsp_launch, need, h->n_splits);
    { const int src = lm_settle(h); if (src != RCA_OK) return src; }
    RCA_HIP(hipSetDevice(h->device));
    hipStream_t st = h->stream;
    RCA_HIP(hipStreamSynchronize(st));
    const std::vector<int32_t> ids((size_t)M, 0);
    int rc;
    if ((rc = lm_push_state(h, ids.data(), M, st)) != RCA_OK) return rc;
    RCA_HIP(hipMemcpy2DAsync(h->qkv, (size_t)QKV * 4, q_host, (size_t)AO * 4, (size_t)AO * 4, M, hipMemcpyHostToDevice, st));
    // NaN sentinel (all bits set, as f32 and as bf16) in the rows a caller may look at: rows >= M must come back untouched
    const size_t n_out = (size_t)out_rows * AO;
    if (route == 2) {
        RCA_HIP(hipMemsetAsync(h->xh, 0xFF, n_out * 2, st));
        RCA_HIP(hipMemsetAsync(h->xl, 0xFF, n_out * 2, st));
    } else {
        RCA_HIP(hipMemsetAsync(h->attn, 0xFF, n_out * 4, st));
    }
    const f16_t* kc = lm_kv_layer(h, h->kc, layer);
    const f16_t* vc = lm_kv_layer(h, h->vc, layer);
    if (route == 0) launch_attention_mfma(h, M, nsp_launch, kc, vc, h->qkv, h->attn, st);
    else if (route == 1) launch_attention_mfma(h, M, nsp_launch, kc, vc, h->qkv, h->attn, st, nullptr, nullptr, true);
    else launch_attention_mfma(h, M, nsp_launch, kc, vc, h->qkv, h->attn, st, h->xh, h->xl, true);
    hipError_t e = hipGetLastError();
    std::vector<uint16_t> hb;
    if (route == 2) {
        hb.resize(2 * n_out);
        if (e == hipSuccess) e = hipMemcpyAsync(hb.data(), h->xh, n_out * 2, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipMemcpyAsync(hb.data() + n_out, h->xl, n_out * 2, hipMemcpyDeviceToHost, st);
        // later passes read the split buffers in blocks of 128 rows: leave no NaN behind in them
        if (e == hipSuccess) e = hipMemsetAsync(h->xh, 0, n_out * 2, st);
        if (e == hipSuccess) e = hipMemsetAsync(h->xl, 0, n_out * 2, st);
    } else {
        if (e == hipSuccess) e = hipMemcpyAsync(out_host, h->attn, n_out * 4, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipMemsetAsync(h->attn, 0, n_out * 4, st);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) return fail(RCA_ERR_HIP, "attn_tap: %s", hipGetErrorString(e));
    if (route == 2) {
        auto widen = [](uint16_t b) { const uint32_t u = (uint32_t)b << 16; float f; memcpy(&f, &u, 4); return f; };
        for (size_t i = 0; i < n_out; ++i) out_host[i] = widen(hb[i]) + widen(hb[n_out + i]);
    }
    return RCA_OK;
}

// tests only: the decode attention of one layer for the members of a batch pass, launched by the very call the pass makes for it
// (lm_batch_launch_attn) over tables staged the way the five batch calls stage theirs (lm_batch_check / lm_batch_stage), for
// host-supplied post-RoPE query rows over whatever the members' caches hold (rca_lm_kv_write)
extern "C" int rca_lm_batch_attn_tap(rca_lm_batch_t* b, int32_t layer, int32_t n, int32_t nsp_launch, const int32_t* sel, int32_t n_sel, const float* q_host,
                                     float* out_host, int32_t out_rows) {
    if (!b || !q_host || !out_host) return fail(RCA_ERR_ARG, "batch_attn_tap: null argument");
    rca_lm* ws = b->m[0];
    const rca_lm_config_t& c = ws->cfg;
    const int QKV = (c.n_heads + 2 * c.n_kv_heads) * c.head_dim, AO = c.n_heads * c.head_dim;
    if (layer < 0 || layer >= c.n_layers) return fail(RCA_ERR_ARG, "batch_attn_tap: layer %d outside [0, %d)", layer, c.n_layers);
    if (n < 1 || n > LM_GEMV_M) return fail(RCA_ERR_ARG, "batch_attn_tap: %d tokens per member (1..%d)", n, LM_GEMV_M);
    const int32_t ids[LM_BATCH_ROWS] = {};
    LmBatchCall call{"batch_attn_tap", sel, sel ? n_sel : 0, n, false, 0, ids, nullptr, nullptr, 0};
    int rc;
    if ((rc = lm_batch_check(b, call)) != RCA_OK) return rc;
    const int MT = call.n_sel * n;
    if (out_rows < MT || out_rows > LM_BATCH_ROWS) return fail(RCA_ERR_ARG, "batch_attn_tap: out_rows %d outside [%d rows of the pass, %d]", out_rows, MT, LM_BATCH_ROWS);
    int need = 1;
    for (int k = 0; k < call.n_sel; ++k) need = std::max(need, lm_splits_needed(call.hm[k], n));
    if (nsp_launch == 0) nsp_launch = need;
    if (nsp_launch < need || nsp_launch > b->nsp_all)
        return fail(RCA_ERR_ARG, "batch_attn_tap: nsp_launch %d outside [%d needed, %d splits of the batch]", nsp_launch, need, b->nsp_all);
    LmBatchPlan p;
    if ((rc = lm_batch_stage(b, call, &p)) != RCA_OK) return rc;
    hipStream_t st = ws->stream;
    RCA_HIP(hipStreamSynchronize(st));
    RCA_HIP(hipMemcpyAsync(b->sel_stage, b->sel_pin, p.up_bytes, hipMemcpyHostToDevice, st));
    lm_batch_stage_kernel<<<1, LM_BATCH_ROWS, 0, st>>>(b->sel_stage, p.vw.tab, b->stt, b->stt_head, n);
    // member k's rows are rows k * n + j of the pass (its table entry's row0 = k * n): the q columns of member 0's qkv
    RCA_HIP(hipMemcpy2DAsync(ws->qkv, (size_t)QKV * 4, q_host, (size_t)AO * 4, (size_t)AO * 4, MT, hipMemcpyHostToDevice, st));
    // NaN sentinel (all bits set) in the output rows a caller may look at, and in every partial a live member owns: a partial that the
    // merge uses although no workgroup of this launch wrote it shows as NaN
    const size_t n_out = (size_t)out_rows * AO;
    RCA_HIP(hipMemsetAsync(ws->xh, 0xFF, n_out * 2, st));
    RCA_HIP(hipMemsetAsync(ws->xl, 0xFF, n_out * 2, st));
    for (int k = 0; k < call.n_sel; ++k) RCA_HIP(hipMemsetAsync(call.hm[k]->att_part, 0xFF, lm_att_part_bytes(call.hm[k]), st));
    lm_attn_split_attrs();
    lm_batch_launch_attn(ws, p.vw.tab, p.vw.NM, n, nsp_launch, lm_kv_q8(ws), layer, st);
    hipError_t e = hipGetLastError();
    std::vector<uint16_t> hb(2 * n_out);
    if (e == hipSuccess) e = hipMemcpyAsync(hb.data(), ws->xh, n_out * 2, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipMemcpyAsync(hb.data() + n_out, ws->xl, n_out * 2, hipMemcpyDeviceToHost, st);
    // later passes read the split buffers in blocks of 128 rows: leave no NaN behind in them
    if (e == hipSuccess) e = hipMemsetAsync(ws->xh, 0, n_out * 2, st);
    if (e == hipSuccess) e = hipMemsetAsync(ws->xl, 0, n_out * 2, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) return fail(RCA_ERR_HIP, "batch_attn_tap: %s", hipGetErrorString(e));
    auto widen = [](uint16_t v) { const uint32_t u = (uint32_t)v << 16; float f; memcpy(&f, &u, 4); return f; };
    for (size_t i = 0; i < n_out; ++i) out_host[i] = widen(hb[i]) + widen(hb[n_out + i]);
    return RCA_OK;
}

// tests only: ONE projection of a 128-token-tile pass, launched by the very calls lm_enqueue_layers128 / rca_lm_score / the batch head make
// for it (lm_launch_proj128<EPI>, lm_launch_logits128), on host-supplied bf16 hi / lo planes
extern "C" int rca_lm_gemm128_tap(rca_lm_t* h, int32_t layer, int32_t kind, const uint16_t* xh_host, const uint16_t* xl_host, int32_t M, int32_t rows,
                                  int32_t row_base, int32_t seq_min, float* y_host, int32_t out_rows, uint16_t* kv_host, int32_t* form) {
    if (!h || !xh_host || !xl_host || !y_host) return fail(RCA_ERR_ARG, "null");
    const rca_lm_config_t& c = h->cfg;
    const int H = c.hidden, QKV = (c.n_heads + 2 * c.n_kv_heads) * c.head_dim, AO = c.n_heads * c.head_dim, F = c.ffn, V = c.vocab_size;
    if (lm_prefill_route(h) != LM_ROUTE_TILE128)
        return fail(RCA_ERR_ARG, "gemm128_tap: the handle does not take the 128-token tiles (rca_lm_prefill_route %d, the call needs 2)", lm_prefill_route(h));
    if (kind < 0 || kind > 4) return fail(RCA_ERR_ARG, "gemm128_tap: kind %d outside [0, 4]", kind);
    if (kind != 4 && (layer < 0 || layer >= c.n_layers)) return fail(RCA_ERR_ARG, "gemm128_tap: layer %d outside [0, %d)", layer, c.n_layers);
    const bool head = kind == 4;
    if (head) rows = 128;   // the head takes one token block: rows row_base .. row_base + 127 of a pass of row_base + M tokens
    if (M < 1 || M > (head ? 128 : LM_MAXM)) return fail(RCA_ERR_ARG, "gemm128_tap: M = %d, kind %d takes 1 .. %d rows", M, kind, head ? 128 : LM_MAXM);
    if (rows < M || rows > LM_MAXM) return fail(RCA_ERR_ARG, "gemm128_tap: rows %d outside [M = %d, %d]", rows, M, LM_MAXM);
    if (out_rows < M || out_rows > (head ? 128 : LM_MAXM)) return fail(RCA_ERR_ARG, "gemm128_tap: out_rows %d outside [M = %d, %d]", out_rows, M, head ? 128 : LM_MAXM);
    if (row_base < 0 || row_base % 128 || row_base + 128 > LM_MAXM || (!head && row_base))
        return fail(RCA_ERR_ARG, "gemm128_tap: row_base %d (a multiple of 128 below %d; 0 for every kind but the head)", row_base, LM_MAXM);
    if (kind == 0 && lm_kv_q8(h)) return fail(RCA_ERR_ARG, "gemm128_tap: kind 0 writes an fp16 cache; this handle's is q8_0");
    if (kind == 0 && h->n_tokens + M > c.n_ctx)
        return fail(RCA_ERR_ARG, "gemm128_tap: positions %d .. %d are outside the context of %d", h->n_tokens, h->n_tokens + M - 1, c.n_ctx);
    { const int src = lm_settle(h); if (src != RCA_OK) return src; }
    RCA_HIP(hipSetDevice(h->device));
    hipStream_t st = h->stream;
    RCA_HIP(hipStreamSynchronize(st));
    const int tbz = (int)cdiv(rows, 128), in_rows = 128 * tbz;
    const int in_w[5] = {H, AO, H, F, H}, out_w[5] = {AO, H, F, H, V};
    const int K = in_w[kind], OW = out_w[kind];
    const std::vector<int32_t> ids((size_t)row_base + M, 0);
    int rc;
    if ((rc = lm_push_state(h, ids.data(), row_base + M, st)) != RCA_OK) return rc;   // m = the rows that exist: the GEMMs' row mask
    // the planes the projection reads: kind 3 takes the SwiGLU planes in hbuf, the others the split buffers; rows M .. 128 tbz - 1 are bf16 NaN
    bf16_t* hh = reinterpret_cast<bf16_t*>(h->hbuf);
    bf16_t* hl = hh + (long)LM_MAXM * F;
    bf16_t* ih = (kind == 3 ? hh : h->xh) + (long)row_base * K;
    bf16_t* il = (kind == 3 ? hl : h->xl) + (long)row_base * K;
    RCA_HIP(hipMemsetAsync(ih, 0xFF, (size_t)in_rows * K * 2, st));
    RCA_HIP(hipMemsetAsync(il, 0xFF, (size_t)in_rows * K * 2, st));
    RCA_HIP(hipMemcpyAsync(ih, xh_host, (size_t)M * K * 2, hipMemcpyHostToDevice, st));
    RCA_HIP(hipMemcpyAsync(il, xl_host, (size_t)M * K * 2, hipMemcpyHostToDevice, st));
    // NaN sentinel (all bits set) in the output rows a caller may look at, zeros in the residual rows that exist
    float* blk = nullptr;
    const size_t head_n = (size_t)128 * V + 128;   // one row tile behind the block: nothing may be written past column V of the last row
    if (kind == 0) {
        RCA_HIP(hipMemsetAsync(h->qkv, 0xFF, (size_t)out_rows * QKV * 4, st));
    } else if (kind == 1 || kind == 3) {
        RCA_HIP(hipMemsetAsync(h->x, 0xFF, (size_t)out_rows * H * 4, st));
        RCA_HIP(hipMemsetAsync(h->x, 0, (size_t)M * H * 4, st));
    } else if (kind == 2) {
        RCA_HIP(hipMemsetAsync(hh, 0xFF, (size_t)out_rows * F * 2, st));
        RCA_HIP(hipMemsetAsync(hl, 0xFF, (size_t)out_rows * F * 2, st));
    } else {
        if ((rc = lm_alloc((void**)&blk, head_n * 4)) != RCA_OK) return rc;
        if (hipMemsetAsync(blk, 0xFF, head_n * 4, st) != hipSuccess) { (void)hipFree(blk); return fail(RCA_ERR_HIP, "gemm128_tap: memset"); }
    }
    const LmTilePass p{h, h->stt, rows, tbz, nullptr, seq_min < 0 ? g128_seq_min() : seq_min};
    G128Form f{1, 1, 0, 1};
    if (kind == 0) {
        const LmLayer& L = h->layers[layer];
        GemvRope rope{h->cos_t, h->sin_t, nullptr, nullptr, c.n_heads, c.n_kv_heads, c.n_ctx, 0};
        lm_rope_target(h, layer, rope);
        for (int seg = 0; seg < (L.split_v ? 2 : 1); ++seg) {   // as lm_enqueue_layers128 runs them; the form reported is the first segment's
            const WMat& w = seg ? L.vseg : L.qkv;
            rope.row_base = seg ? L.qkv.N : 0;
            const G128Form fs = lm_launch_proj128<GEMM_EPI_ROPE>(p, w, st, h->xh, h->xl, w.N, H, h->qkv, QKV, nullptr, nullptr, rope, nogroup);
            if (!seg) f = fs;
        }
    } else if (kind == 1) {
        f = lm_launch_proj128<GEMM_EPI_RESID>(p, h->layers[layer].o, st, h->xh, h->xl, H, AO, h->x, H, nullptr, nullptr);
    } else if (kind == 2) {
        f = lm_launch_proj128<GEMM_EPI_SWIGLU>(p, h->layers[layer].gu, st, h->xh, h->xl, 2 * F, H, nullptr, F, hh, hl);
    } else if (kind == 3) {
        f = lm_launch_proj128<GEMM_EPI_RESID>(p, h->layers[layer].down, st, hh, hl, H, F, h->x, H, nullptr, nullptr);
    } else {
        lm_launch_logits128(h, h->stt, ih, il, row_base, blk, st);
    }
    hipError_t e = hipGetLastError();
    const size_t n_out = (size_t)out_rows * OW;
    std::vector<uint16_t> hb;
    if (kind == 0) {
        if (e == hipSuccess) e = hipMemcpy2DAsync(y_host, (size_t)AO * 4, h->qkv, (size_t)QKV * 4, (size_t)AO * 4, out_rows, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess && kv_host) {
            const size_t n = (size_t)M * c.n_kv_heads * 64;
            const long off = (long)layer * h->kv_layer_stride + (long)h->n_tokens * c.n_kv_heads * 64;
            e = hipMemcpyAsync(kv_host, h->kc + off, n * 2, hipMemcpyDeviceToHost, st);
            if (e == hipSuccess) e = hipMemcpyAsync(kv_host + n, h->vc + off, n * 2, hipMemcpyDeviceToHost, st);
        }
        if (e == hipSuccess) e = hipMemsetAsync(h->qkv, 0, (size_t)out_rows * QKV * 4, st);
    } else if (kind == 1 || kind == 3) {
        if (e == hipSuccess) e = hipMemcpyAsync(y_host, h->x, n_out * 4, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipMemsetAsync(h->x, 0, n_out * 4, st);
    } else if (kind == 2) {
        hb.resize(2 * n_out);
        if (e == hipSuccess) e = hipMemcpyAsync(hb.data(), hh, n_out * 2, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipMemcpyAsync(hb.data() + n_out, hl, n_out * 2, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipMemsetAsync(hh, 0, n_out * 2, st);
        if (e == hipSuccess) e = hipMemsetAsync(hl, 0, n_out * 2, st);
    } else {   // out_rows rows of the block, then the 128 values behind its last row
        if (e == hipSuccess) e = hipMemcpyAsync(y_host, blk, n_out * 4, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipMemcpyAsync(y_host + n_out, blk + (size_t)128 * V, 128 * 4, hipMemcpyDeviceToHost, st);
    }
    // later passes read the planes in blocks of 128 rows: leave no NaN behind in them
    if (e == hipSuccess) e = hipMemsetAsync(ih, 0, (size_t)in_rows * K * 2, st);
    if (e == hipSuccess) e = hipMemsetAsync(il, 0, (size_t)in_rows * K * 2, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (blk) (void)hipFree(blk);
    if (e != hipSuccess) return fail(RCA_ERR_HIP, "gemm128_tap: %s", hipGetErrorString(e));
    if (kind == 2) {
        auto widen = [](uint16_t b) { const uint32_t u = (uint32_t)b << 16; float v; memcpy(&v, &u, 4); return v; };
        for (size_t i = 0; i < n_out; ++i) y_host[i] = widen(hb[i]) + widen(hb[n_out + i]);
    }
    if (form) { form[0] = f.grid_y; form[1] = f.nseq; form[2] = f.ep_nsplit; form[3] = f.ep_grp; }
    return RCA_OK;
}

// the format the projection matrices are kept (and streamed) in: 0 bf16, 1 q8_0, 2 f16, 3 q4_k, 5 q5_k, 6 q4_0, 7 q4_1, 8 iq4_nl, 9 iq4_xs (4 = Q6_K,
// which only ever appears next to Q4_K / Q5_K / Q4_0 / IQ4 tensors); bytes = weight bytes one decode step reads
extern "C" int rca_lm_weight_format(const rca_lm_t* h, int32_t* fmt, int64_t* bytes_per_step) {
    if (!h || !fmt) return fail(RCA_ERR_ARG, "null");
    *fmt = h->layers.empty() ? h->head.fmt : h->layers[0].gu.fmt;
    if (bytes_per_step) {
        long b = h->head.stream_bytes();
        for (const LmLayer& L : h->layers) b += L.qkv.stream_bytes() + L.o.stream_bytes() + L.gu.stream_bytes() + L.down.stream_bytes() + (L.split_v ? L.vseg.stream_bytes() : 0);
        *bytes_per_step = b;
    }
    return RCA_OK;
}

// tests only: which of the three prefill routes a long eval takes right now (lm_prefill_route, the predicate lm_eval_impl branches on)
extern "C" int rca_lm_prefill_route(const rca_lm_t* h, int32_t* route) {
    if (!h || !route) return fail(RCA_ERR_ARG, "null");
    *route = lm_prefill_route(h);
    return RCA_OK;
}

// test / bench knob: route long evals through the exact GEMV chunks (0) or the bf16 MFMA prefill tiles (1, default)
extern "C" int rca_lm_set_mfma_prefill(rca_lm_t* h, int32_t enable) {
    if (!h) return fail(RCA_ERR_ARG, "null");
    h->mfma_prefill = enable != 0;
    return RCA_OK;
}

// ------------------------------------------------------------------------------------ scoring (rca_lm_score)
// One workgroup per token row, ONE pass over the row's V logits (and over the same row of the base's block) with an online softmax:
// a thread keeps (m, s, t, arg) = running maximum, sum of exp(x - m), [base only] sum of exp(b - m_b) (b - a), index of the maximum.
// It takes 16-byte chunks tid, tid + 256, ...; per chunk the maximum is raised first (s and t scaled by exp(m_old - m_new), once per
// chunk), then the four terms are added in index order.  The <= 3 values in front of the first aligned chunk (V need not be a multiple
// of 4, so a row need not start on 16 bytes) go to thread 0 before its chunks, the <= 3 behind the last one to thread 255 after its
// chunks.  The 256 states are merged by a 6-step xor butterfly inside each wave (offsets 32 .. 1), then wave 1, 2, 3 are merged into
// wave 0 in that order: merge((m1, s1), (m2, s2)) = (M, s1 exp(m1 - M) + s2 exp(m2 - M)) with M = max, exp(0) taken as exactly 1.
// The longest chain of f32 additions is 4 ceil(chunks / 256) + 3 + 6 + 3 (tests/score_ref.py derives the error bound from it).
// Ties of the maximum go to the lowest index: strict > inside a thread (ascending indices), (value, lower index) between threads.
// -inf logits contribute exactly 0 (never exp(-inf - -inf)); NaN never wins a maximum, is flagged and turns the row's outputs NaN.
struct ScoreAcc { float m, s, t; int arg; };
__device__ __forceinline__ float score_scale(float from, float to) { return from == to ? 1.0f : expf(from - to); }
__device__ __forceinline__ void score_merge(ScoreAcc& a, const ScoreAcc& b) {
    const float M = fmaxf(a.m, b.m);
    const float fa = score_scale(a.m, M), fb = score_scale(b.m, M);
    if (b.m > a.m || (b.m == a.m && b.arg < a.arg)) a.arg = b.arg;
    a.s = a.s * fa + b.s * fb;
    a.t = a.t * fa + b.t * fb;
    a.m = M;
}
__device__ __forceinline__ void score_raise(ScoreAcc& A, const float* v, int idx0, int cnt) {
    float nm = A.m;
    for (int j = 0; j < cnt; ++j)
        if (v[j] > nm) { nm = v[j]; A.arg = idx0 + j; }
    if (nm != A.m) {
        const float f = expf(A.m - nm);
        A.s = A.s * f;
        A.t = A.t * f;
        A.m = nm;
    }
}
template <bool BASE>
__device__ __forceinline__ void score_take(ScoreAcc& A, ScoreAcc& B, int& fl, const float* a, const float* b, int idx0, int cnt) {
    score_raise(A, a, idx0, cnt);
    if (BASE) score_raise(B, b, idx0, cnt);
    for (int j = 0; j < cnt; ++j) {
        if (a[j] != a[j]) fl |= 1;
        A.s = A.s + (a[j] == -INFINITY ? 0.0f : expf(a[j] - A.m));
        if (BASE) {
            if (b[j] != b[j]) fl |= 2;
            const float e = b[j] == -INFINITY ? 0.0f : expf(b[j] - B.m);
            B.s = B.s + e;
            if (b[j] > -INFINITY) {   // p_base = 0: the term counts as 0 whatever a is
                if (a[j] == -INFINITY) fl |= 4;   // P gives no mass where the base does: kl = +inf
                else B.t = B.t + e * (b[j] - a[j]);
            }
        }
    }
}
__device__ __forceinline__ void score_wave_merge(ScoreAcc& A) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        ScoreAcc o;
        o.m = __shfl_xor(A.m, off); o.s = __shfl_xor(A.s, off); o.t = __shfl_xor(A.t, off); o.arg = __shfl_xor(A.arg, off);
        score_merge(A, o);
    }
}
#define SCORE_THREADS 256
template <bool BASE>
__global__ __launch_bounds__(SCORE_THREADS) void lm_score_rows_kernel(const float* __restrict__ logits, const float* __restrict__ base, int V,
                                                                      const int* __restrict__ targets, rca_score_row_t* __restrict__ out) {
    __shared__ ScoreAcc smA[SCORE_THREADS / 64], smB[SCORE_THREADS / 64];
    __shared__ int smf[SCORE_THREADS / 64];
    const int row = blockIdx.x, tid = threadIdx.x;
    const float* pa = logits + (long)row * V;
    const float* pb = BASE ? base + (long)row * V : nullptr;
    const int pre = min(V, (4 - (int)(((long)row * V) & 3)) & 3);   // values in front of the row's first 16-byte boundary
    const int nb4 = (V - pre) >> 2, tail0 = pre + 4 * nb4;
    ScoreAcc A{-INFINITY, 0.0f, 0.0f, INT_MAX}, B{-INFINITY, 0.0f, 0.0f, INT_MAX};
    int fl = 0;
    float a[4], b[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    if (tid == 0 && pre > 0) {
        for (int j = 0; j < pre; ++j) { a[j] = pa[j]; if (BASE) b[j] = pb[j]; }
        score_take<BASE>(A, B, fl, a, b, 0, pre);
    }
    for (int c = tid; c < nb4; c += SCORE_THREADS) {
        const float4 va = *reinterpret_cast<const float4*>(pa + pre + 4 * c);
        a[0] = va.x; a[1] = va.y; a[2] = va.z; a[3] = va.w;
        if (BASE) {
            const float4 vb = *reinterpret_cast<const float4*>(pb + pre + 4 * c);
            b[0] = vb.x; b[1] = vb.y; b[2] = vb.z; b[3] = vb.w;
        }
        score_take<BASE>(A, B, fl, a, b, pre + 4 * c, 4);
    }
    if (tid == SCORE_THREADS - 1 && tail0 < V) {
        for (int j = 0; j < V - tail0; ++j) { a[j] = pa[tail0 + j]; if (BASE) b[j] = pb[tail0 + j]; }
        score_take<BASE>(A, B, fl, a, b, tail0, V - tail0);
    }
    score_wave_merge(A);
    if (BASE) score_wave_merge(B);
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) fl |= __shfl_xor(fl, off);
    if ((tid & 63) == 0) { smA[tid >> 6] = A; smB[tid >> 6] = B; smf[tid >> 6] = fl; }
    __syncthreads();
    if (tid != 0) return;
    for (int w = 1; w < SCORE_THREADS / 64; ++w) {
        score_merge(A, smA[w]);
        if (BASE) score_merge(B, smB[w]);
        fl |= smf[w];
    }
    const float nanv = __uint_as_float(0x7fc00000u);
    const int tgt = targets[row];
    rca_score_row_t r;
    r.flags = fl;
    r.argmax = A.arg == INT_MAX ? 0 : A.arg;
    r.max_logit = A.m;
    r.lse = A.m + logf(A.s);
    r.logprob = tgt >= 0 ? pa[tgt] - r.lse : nanv;
    r.kl = nanv; r.base_logprob = nanv; r.base_argmax = -1;
    if (BASE) {
        const float lse_b = B.m + logf(B.s);
        r.base_argmax = B.arg == INT_MAX ? 0 : B.arg;
        r.base_logprob = tgt >= 0 ? pb[tgt] - lse_b : nanv;
        r.kl = (fl & 4) ? INFINITY : (B.t / B.s - lse_b) + r.lse;
        if (fl & 2) r.base_logprob = nanv;
        if (fl & 3) r.kl = nanv;
    }
    if (fl & 1) { r.lse = nanv; r.max_logit = nanv; r.logprob = nanv; }
    out[row] = r;
}
static void lm_launch_score_rows(const float* blk, const float* base_blk, int V, const int* tgt, rca_score_row_t* rows, int M, hipStream_t st) {
    if (base_blk) lm_score_rows_kernel<true><<<M, SCORE_THREADS, 0, st>>>(blk, base_blk, V, tgt, rows);
    else lm_score_rows_kernel<false><<<M, SCORE_THREADS, 0, st>>>(blk, nullptr, V, tgt, rows);
}

// the route rca_lm_score takes: the 128-token tiles wherever a long eval of the handle could take them (logits_all is ignored: the
// logits never leave the device), else the exact decode passes
static int lm_score_route(const rca_lm* h) { return h->mfma_prefill && lm_can_gemm128(h) ? LM_ROUTE_TILE128 : LM_ROUTE_GEMV; }
static size_t lm_score_pin_bytes(int n, int step) {   // every pass's state block, 16-byte aligned
    size_t b = 0;
    for (int off = 0; off < n; off += step) b += (lm_state_bytes(std::min(step, n - off)) + 15) / 16 * 16;
    return b;
}
static int lm_score_reserve_pin(rca_lm* h, size_t pin_bytes) {   // the pinned block alone (rca_lm_imatrix_chunk scores nothing)
    if (pin_bytes > h->sc_pin_cap) {
        if (h->sc_pin) { (void)hipHostFree(h->sc_pin); h->sc_pin = nullptr; h->sc_pin_cap = 0; }
        RCA_HIP(hipHostMalloc((void**)&h->sc_pin, pin_bytes, hipHostMallocDefault));
        h->sc_pin_cap = pin_bytes;
    }
    return RCA_OK;
}
static int lm_score_reserve(rca_lm* h, long n_rows, size_t pin_bytes) {
    int rc;
    if (!h->sc_blk && (rc = lm_alloc((void**)&h->sc_blk, (size_t)128 * h->cfg.vocab_size * 4)) != RCA_OK) return rc;
    if (!h->sc_ready) RCA_HIP(hipEventCreateWithFlags(&h->sc_ready, hipEventDisableTiming));
    if (!h->sc_free) RCA_HIP(hipEventCreateWithFlags(&h->sc_free, hipEventDisableTiming));
    if (n_rows > h->sc_rows_cap) {
        for (void* p : {(void*)h->sc_rows, (void*)h->sc_tgt})
            if (p) (void)hipFree(p);
        h->sc_rows = nullptr; h->sc_tgt = nullptr; h->sc_rows_cap = 0;
        if ((rc = lm_alloc((void**)&h->sc_rows, (size_t)n_rows * sizeof(rca_score_row_t))) != RCA_OK) return rc;
        if ((rc = lm_alloc((void**)&h->sc_tgt, (size_t)n_rows * 4)) != RCA_OK) return rc;
        h->sc_rows_cap = n_rows;
    }
    return lm_score_reserve_pin(h, pin_bytes);
}
// the next pass of a scoring call as the device will read it, from this pass's OWN pinned block (lm_push_state reuses one)
static int lm_score_push(rca_lm* x, size_t* pin_off, const int32_t* ids, int m, hipStream_t st) {
    int* p = reinterpret_cast<int*>(x->sc_pin + *pin_off);
    const size_t nb = lm_state_bytes(m);
    memset(p, 0, nb);
    p[0] = x->n_tokens;
    p[1] = m;
    memcpy(p + 2, ids, (size_t)m * 4);
    *pin_off += (nb + 15) / 16 * 16;
    RCA_HIP(hipMemcpyAsync(x->stt, p, nb, hipMemcpyHostToDevice, st));
    return RCA_OK;
}
// final RMSNorm + head of tokens [tb, tb + 128) of the pass in x->x on the 128-row tiles -> x->sc_blk.  The caller has written the
// hi / lo split of the normalised rows to x->xh / x->xl.  Every workgroup walks all of K itself (one slice: no partial sums).
static void lm_launch_head128(rca_lm* x, int tb, hipStream_t st) {
    lm_launch_logits128(x, x->stt, x->xh + (long)tb * x->cfg.hidden, x->xl + (long)tb * x->cfg.hidden, tb, x->sc_blk, st);
}

extern "C" int rca_lm_score(rca_lm_t* h, rca_lm_t* base, const int32_t* ids, int32_t n, const int32_t* targets, rca_score_row_t* rows_host) {
    if (!h || n < 0 || (n > 0 && (!ids || !rows_host))) return fail(RCA_ERR_ARG, "score: bad argument");
    if (n == 0) return RCA_OK;
    const rca_lm_config_t& c = h->cfg;
    const int V = c.vocab_size;
    if (h->n_tokens + n > c.n_ctx) return fail(RCA_ERR_STATE, "score: context overflow: %d + %d > n_ctx %d", h->n_tokens, n, c.n_ctx);
    for (int i = 0; i < n; ++i)
        if (ids[i] < 0 || ids[i] >= V) return fail(RCA_ERR_ARG, "score: token id %d at index %d is outside the vocabulary [0, %d)", ids[i], i, V);
    if (targets)
        for (int i = 0; i < n; ++i)
            if (targets[i] < -1 || targets[i] >= V) return fail(RCA_ERR_ARG, "score: target %d at index %d is neither -1 nor inside the vocabulary [0, %d)", targets[i], i, V);
    if (base) {
        if (base == h) return fail(RCA_ERR_ARG, "score: the base is the scored handle itself");
        if (base->device != h->device) return fail(RCA_ERR_ARG, "score: the base sits on device %d, the scored handle on %d", base->device, h->device);
        if (base->cfg.vocab_size != V) return fail(RCA_ERR_ARG, "score: the base has a vocabulary of %d, the scored handle one of %d", base->cfg.vocab_size, V);
        if (base->n_tokens != h->n_tokens) return fail(RCA_ERR_ARG, "score: the base is at n_tokens %d, the scored handle at %d", base->n_tokens, h->n_tokens);
        if (base->n_tokens + n > base->cfg.n_ctx) return fail(RCA_ERR_STATE, "score: context overflow of the base: %d + %d > n_ctx %d", base->n_tokens, n, base->cfg.n_ctx);
    }
    int rc;
    if ((rc = lm_settle(h)) != RCA_OK) return rc;
    if (base && (rc = lm_settle(base)) != RCA_OK) return rc;
    RCA_HIP(hipSetDevice(h->device));
    const bool tiles = lm_score_route(h) == LM_ROUTE_TILE128 && (!base || lm_score_route(base) == LM_ROUTE_TILE128);
    const int step = tiles ? LM_MAXM : LM_GEMV_M;
    const size_t pin_states = lm_score_pin_bytes(n, step);
    if ((rc = lm_score_reserve(h, n, pin_states + (size_t)n * 4)) != RCA_OK) return rc;
    if (base && (rc = lm_score_reserve(base, 0, pin_states)) != RCA_OK) return rc;
    hipStream_t st = h->stream, sb = base ? base->stream : nullptr;
    int* tgt_pin = reinterpret_cast<int*>(h->sc_pin + pin_states);
    for (int i = 0; i < n; ++i) tgt_pin[i] = targets ? targets[i] : (i + 1 < n ? ids[i + 1] : -1);
    RCA_HIP(hipMemcpyAsync(h->sc_tgt, tgt_pin, (size_t)n * 4, hipMemcpyHostToDevice, st));
    rca_lm* xs[2] = {h, base};
    hipStream_t ss[2] = {st, sb};
    size_t pin_off[2] = {0, 0};
    const int nx = base ? 2 : 1;
    bool base_blk_used = false;   // the scored handle's stream has read the base's block: the base waits before it overwrites it
    // one block of logits: both handles write theirs (the base on its own stream), the scored handle's stream waits for the base's
    // event, reduces the rows and records that the base's block is free again
    auto score_block = [&](int row0, int mb) -> int {
        if (base) {
            RCA_HIP(hipEventRecord(base->sc_ready, sb));
            RCA_HIP(hipStreamWaitEvent(st, base->sc_ready, 0));
        }
        lm_launch_score_rows(h->sc_blk, base ? base->sc_blk : nullptr, V, h->sc_tgt + row0, h->sc_rows + row0, mb, st);
        if (base) {
            RCA_HIP(hipEventRecord(h->sc_free, st));
            base_blk_used = true;
        }
        return RCA_OK;
    };
    for (int off = 0; off < n; off += step) {
        const int m = std::min(step, n - off);
        const bool last = off + m >= n;
        for (int k = 0; k < nx; ++k) {
            rca_lm* x = xs[k];
            if ((rc = lm_score_push(x, &pin_off[k], ids + off, m, ss[k])) != RCA_OK) return rc;
            if (tiles) {
                if ((rc = lm_enqueue_prefill_tile128(x, m, ss[k], lm_splits_needed(x, m))) != RCA_OK) return rc;
                if (last) lm_launch_head(x, 1, ss[k], x->logits, true);   // the last position's logits, as rca_lm_eval computes them
                lm_add_rmsnorm_kernel<<<m, 64, 0, ss[k]>>>(x->stt, x->x, nullptr, nullptr, 0, 0, x->final_norm, x->xn, x->cfg.hidden, x->cfg.rms_eps, x->xh, x->xl);
            } else {
                if ((rc = lm_enqueue_pass(x, m, 0, ss[k], lm_splits_needed(x, m))) != RCA_OK) return rc;
                if (last) lm_launch_head(x, 1, ss[k], x->logits, true);
            }
        }
        for (int tb = 0; tb < m; tb += 128) {
            const int mb = std::min(128, m - tb);
            if (base && base_blk_used) RCA_HIP(hipStreamWaitEvent(sb, h->sc_free, 0));
            for (int k = 0; k < nx; ++k) {
                if (tiles) lm_launch_head128(xs[k], tb, ss[k]);
                else lm_launch_head(xs[k], mb, ss[k], xs[k]->sc_blk, false);
            }
            if ((rc = score_block(off + tb, mb)) != RCA_OK) return rc;
        }
        RCA_LAUNCH_CHECK();
        for (int k = 0; k < nx; ++k) xs[k]->n_tokens += m;
    }
    for (int k = 0; k < nx; ++k) xs[k]->logits_rows = 1;
    if (base) base->async_pending = true;   // its stream may still run; everything the scored rows need has been waited for through the events
    RCA_HIP(hipMemcpyAsync(rows_host, h->sc_rows, (size_t)n * sizeof(rca_score_row_t), hipMemcpyDeviceToHost, st));
    RCA_HIP(hipStreamSynchronize(st));
    return RCA_OK;
}

extern "C" int rca_lm_score_rows_tap(rca_lm_t* h, const float* logits_host, const float* base_logits_host, const int32_t* targets, int32_t M,
                                     rca_score_row_t* rows_host) {
    if (!h || !logits_host || !targets || !rows_host) return fail(RCA_ERR_ARG, "null");
    const int V = h->cfg.vocab_size;
    if (M < 1 || M > 4096) return fail(RCA_ERR_ARG, "score_rows_tap: M = %d outside [1, 4096]", M);
    for (int i = 0; i < M; ++i)
        if (targets[i] < -1 || targets[i] >= V) return fail(RCA_ERR_ARG, "score_rows_tap: target %d at index %d is neither -1 nor inside the vocabulary [0, %d)", targets[i], i, V);
    int rc;
    if ((rc = lm_settle(h)) != RCA_OK) return rc;
    RCA_HIP(hipSetDevice(h->device));
    hipStream_t st = h->stream;
    const size_t nb = (size_t)M * V * 4;
    float *la = nullptr, *lb = nullptr;
    int* tg = nullptr;
    rca_score_row_t* rows = nullptr;
    hipError_t e = hipSuccess;
    if ((rc = lm_alloc((void**)&la, nb)) == RCA_OK && (!base_logits_host || (rc = lm_alloc((void**)&lb, nb)) == RCA_OK) &&
        (rc = lm_alloc((void**)&tg, (size_t)M * 4)) == RCA_OK && (rc = lm_alloc((void**)&rows, (size_t)M * sizeof(rca_score_row_t))) == RCA_OK) {
        e = hipMemcpyAsync(la, logits_host, nb, hipMemcpyHostToDevice, st);
        if (e == hipSuccess && lb) e = hipMemcpyAsync(lb, base_logits_host, nb, hipMemcpyHostToDevice, st);
        if (e == hipSuccess) e = hipMemcpyAsync(tg, targets, (size_t)M * 4, hipMemcpyHostToDevice, st);
        if (e == hipSuccess) {
            lm_launch_score_rows(la, lb, V, tg, rows, M, st);
            e = hipGetLastError();
        }
        if (e == hipSuccess) e = hipMemcpyAsync(rows_host, rows, (size_t)M * sizeof(rca_score_row_t), hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
    }
    for (void* p : {(void*)la, (void*)lb, (void*)tg, (void*)rows})
        if (p) (void)hipFree(p);
    if (rc != RCA_OK) return rc;
    if (e != hipSuccess) return fail(RCA_ERR_HIP, "score_rows_tap: %s", hipGetErrorString(e));
    return RCA_OK;
}

// ------------------------------------------------------------------------- importance matrix: the column sums (rca_lm_imatrix_rows_tap)
// Per input column of a projection, the sum over tokens of the squared activation, over the bf16 hi / lo planes the 128-token tile route
// stages a GEMM input as.  Definition (tests/imatrix_ref.py restates it): planes hi, lo [rows][K] with m live rows, v_r = f32(hi[r][j]) +
// f32(lo[r][j]), s_r = v_r * v_r (one multiply, no fma), the partial of token block b is p_b = ((0.0f + s_r0) + s_r1) + ... over rows
// 128 b .. min(128 b + 127, m - 1) in ascending order, and acc[j] += (double)p_b for b ascending.  Rows >= m are never read.  No
// atomics: one lane owns a (column pair, token block), the partials of a column meet in LDS, and one lane per column folds them in order.
// The adds of a column are a serial chain, so what a lane can do is keep loads in flight: it takes both columns of a pair with one
// 32-bit load per plane and row, and requests IMX_ROWS rows (clamped to its last live row) before the ordered adds of those rows.
// An odd K has no aligned pairs: its lanes load their two columns 2 bytes at a time.  Every collecting pass launches it
// (lm_collect_planes, rca_lm_imatrix_chunk) and the tap runs it alone (DESIGN.md "Importance matrix").
#define IMX_COLS 64    // columns per workgroup: 32 lanes of column pairs x 8 token blocks = 4 waves
#define IMX_ROWS 32    // rows requested before their adds
__global__ __launch_bounds__(IMX_COLS / 2 * (LM_MAXM / 128)) void lm_imatrix_kernel(const bf16_t* __restrict__ xh, const bf16_t* __restrict__ xl, int K, int m,
                                                                                      double* __restrict__ acc) {
    __shared__ float part[LM_MAXM / 128][IMX_COLS];
    const int j = blockIdx.x * IMX_COLS + 2 * threadIdx.x, b = threadIdx.y;
    const int r0 = 128 * b, r1 = min(r0 + 128, m);
    float p0 = 0.0f, p1 = 0.0f;
    if (!(K & 1)) {
        if (j < K)   // (K even, j even: column j + 1 exists and the pair is 4-byte aligned in every row)
            for (int r = r0; r < r1; r += IMX_ROWS) {
                unsigned a[IMX_ROWS], c[IMX_ROWS];
#pragma unroll
                for (int u = 0; u < IMX_ROWS; ++u) {
                    const long at = (long)min(r + u, r1 - 1) * K + j;
                    a[u] = *reinterpret_cast<const unsigned*>(xh + at);
                    c[u] = *reinterpret_cast<const unsigned*>(xl + at);
                }
#pragma unroll
                for (int u = 0; u < IMX_ROWS; ++u)
                    if (r + u < r1) {
                        const float v0 = __fadd_rn(__uint_as_float(a[u] << 16), __uint_as_float(c[u] << 16));
                        const float v1 = __fadd_rn(__uint_as_float(a[u] & 0xFFFF0000u), __uint_as_float(c[u] & 0xFFFF0000u));
                        p0 = __fadd_rn(p0, __fmul_rn(v0, v0));
                        p1 = __fadd_rn(p1, __fmul_rn(v1, v1));
                    }
            }
    } else {
        for (int r = r0; r < r1; ++r) {
            if (j < K) {
                const float v = __fadd_rn(__uint_as_float((unsigned)xh[(long)r * K + j] << 16), __uint_as_float((unsigned)xl[(long)r * K + j] << 16));
                p0 = __fadd_rn(p0, __fmul_rn(v, v));
            }
            if (j + 1 < K) {
                const float v = __fadd_rn(__uint_as_float((unsigned)xh[(long)r * K + j + 1] << 16), __uint_as_float((unsigned)xl[(long)r * K + j + 1] << 16));
                p1 = __fadd_rn(p1, __fmul_rn(v, v));
            }
        }
    }
    part[b][2 * threadIdx.x] = p0;
    part[b][2 * threadIdx.x + 1] = p1;
    __syncthreads();
    const int t = threadIdx.y * (IMX_COLS / 2) + threadIdx.x, jc = blockIdx.x * IMX_COLS + t;   // the first wave: one lane per column
    if (t < IMX_COLS && jc < K) {
        double s = acc[jc];
        for (int bb = 0; 128 * bb < m; ++bb) s += (double)part[bb][t];
        acc[jc] = s;
    }
}
static void lm_launch_imatrix(const bf16_t* xh, const bf16_t* xl, int K, int m, double* acc, hipStream_t st) {   // 1 <= m <= LM_MAXM
    lm_imatrix_kernel<<<cdiv(K, IMX_COLS), dim3(IMX_COLS / 2, LM_MAXM / 128), 0, st>>>(xh, xl, K, m, acc);
}
// tests only: the collector alone on host-supplied planes [M][K] of which m_live rows are live, adding into the caller's double[K]
extern "C" int rca_lm_imatrix_rows_tap(rca_lm_t* h, const uint16_t* xh_host, const uint16_t* xl_host, int32_t M, int32_t K, int32_t m_live,
                                       double* acc_inout_host) {
    if (!h || !xh_host || !xl_host || !acc_inout_host) return fail(RCA_ERR_ARG, "imatrix_rows_tap: null pointer");
    if (M < 1 || M > LM_MAXM || K < 1 || K > (1 << 20)) return fail(RCA_ERR_ARG, "imatrix_rows_tap: planes of %d x %d (1 .. %d rows, 1 .. %d columns)", M, K, LM_MAXM, 1 << 20);
    if (m_live < 1 || m_live > M) return fail(RCA_ERR_ARG, "imatrix_rows_tap: m_live = %d outside [1, M = %d]", m_live, M);
    int rc;
    if ((rc = lm_settle(h)) != RCA_OK) return rc;
    RCA_HIP(hipSetDevice(h->device));
    hipStream_t st = h->stream;
    const size_t nb = (size_t)M * K * 2;
    bf16_t *ph = nullptr, *pl = nullptr;
    double* acc = nullptr;
    hipError_t e = hipSuccess;
    if ((rc = lm_alloc((void**)&ph, nb)) == RCA_OK && (rc = lm_alloc((void**)&pl, nb)) == RCA_OK && (rc = lm_alloc((void**)&acc, (size_t)K * 8)) == RCA_OK) {
        e = hipMemcpyAsync(ph, xh_host, nb, hipMemcpyHostToDevice, st);
        if (e == hipSuccess) e = hipMemcpyAsync(pl, xl_host, nb, hipMemcpyHostToDevice, st);
        if (e == hipSuccess) e = hipMemcpyAsync(acc, acc_inout_host, (size_t)K * 8, hipMemcpyHostToDevice, st);
        if (e == hipSuccess) {
            lm_launch_imatrix(ph, pl, K, m_live, acc, st);
            e = hipGetLastError();
        }
        if (e == hipSuccess) e = hipMemcpyAsync(acc_inout_host, acc, (size_t)K * 8, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
    }
    for (void* p : {(void*)ph, (void*)pl, (void*)acc})
        if (p) (void)hipFree(p);
    if (rc != RCA_OK) return rc;
    if (e != hipSuccess) return fail(RCA_ERR_HIP, "imatrix_rows_tap: %s", hipGetErrorString(e));
    return RCA_OK;
}

// ------------------------------------------------------------------------- importance matrix: the collector (rca_lm_imatrix_begin .. _end)
// A handle between begin and end holds n_layers * (H + AO + H + F) + H double accumulators (lm_imx_slot) and a token count.  Only
// rca_lm_imatrix_chunk adds to them: it walks its tokens as rca_lm_score does -- passes of up to LM_MAXM rows on the 128-token tiles,
// enqueued eagerly, the last position's logits behind the last pass -- with the pass's LmTilePass::imx set, so lm_enqueue_layers128
// sums every projection's input planes right behind the launch that wrote them, and sums the final norm's planes of all live rows for
// output.weight.  No per-block head GEMM runs.  Every other call builds its passes with imx null and leaves sums and count alone.
static long lm_imx_values(const rca_lm_config_t& c) { int K; return lm_imx_slot(c, 0, 4, &K) + K; }
extern "C" int rca_lm_imatrix_begin(rca_lm_t* h) {
    if (!h) return fail(RCA_ERR_ARG, "imatrix_begin: null handle");
    if (h->imx_acc) return fail(RCA_ERR_STATE, "imatrix_begin: the handle is already collecting (rca_lm_imatrix_end ends a collection)");
    if (lm_score_route(h) != LM_ROUTE_TILE128)
        return fail(RCA_ERR_STATE, "imatrix_begin: the handle's long evals do not take the 128-token tiles (%s): the collector sums the tiles' input planes",
                    h->mfma_prefill ? "its weights or dimensions are off them" : "rca_lm_set_mfma_prefill is off");
    int rc;
    if ((rc = lm_settle(h)) != RCA_OK) return rc;
    RCA_HIP(hipSetDevice(h->device));
    const size_t nb = (size_t)lm_imx_values(h->cfg) * 8;
    double* acc = nullptr;
    if ((rc = lm_alloc((void**)&acc, nb)) != RCA_OK) return rc;
    hipError_t e = hipMemsetAsync(acc, 0, nb, h->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    if (e != hipSuccess) { (void)hipFree(acc); return fail(RCA_ERR_HIP, "imatrix_begin: %s", hipGetErrorString(e)); }
    h->imx_acc = acc;
    h->imx_count = 0;
    h->imx_tap_layer = h->imx_tap_kind = -1;
    return RCA_OK;
}
extern "C" int rca_lm_imatrix_end(rca_lm_t* h) {
    if (!h) return fail(RCA_ERR_ARG, "imatrix_end: null handle");
    if (!h->imx_acc) return RCA_OK;
    (void)hipSetDevice(h->device);
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    (void)hipFree(h->imx_acc);
    h->imx_acc = nullptr;
    h->imx_count = 0;
    return RCA_OK;
}
static int lm_imatrix_chunk_impl(rca_lm* h, const char* who, const int32_t* ids, int n) {
    if (n < 1 || !ids) return fail(RCA_ERR_ARG, "%s: bad argument (n = %d tokens)", who, n);
    if (!h->imx_acc) return fail(RCA_ERR_STATE, "%s: the handle is not collecting (rca_lm_imatrix_begin starts a collection)", who);
    const rca_lm_config_t& c = h->cfg;
    if (h->n_tokens + n > c.n_ctx) return fail(RCA_ERR_STATE, "%s: context overflow: %d + %d > n_ctx %d", who, h->n_tokens, n, c.n_ctx);
    for (int i = 0; i < n; ++i)
        if (ids[i] < 0 || ids[i] >= c.vocab_size)
            return fail(RCA_ERR_ARG, "%s: token id %d at index %d is outside the vocabulary [0, %d)", who, ids[i], i, c.vocab_size);
    if (lm_score_route(h) != LM_ROUTE_TILE128)
        return fail(RCA_ERR_STATE, "%s: the handle's long evals no longer take the 128-token tiles (rca_lm_set_mfma_prefill is off)", who);
    int rc;
    if ((rc = lm_settle(h)) != RCA_OK) return rc;
    RCA_HIP(hipSetDevice(h->device));
    if ((rc = lm_score_reserve_pin(h, lm_score_pin_bytes(n, LM_MAXM))) != RCA_OK) return rc;
    hipStream_t st = h->stream;
    size_t pin_off = 0;
    for (int off = 0; off < n; off += LM_MAXM) {
        const int m = std::min((int)LM_MAXM, n - off);
        if ((rc = lm_score_push(h, &pin_off, ids + off, m, st)) != RCA_OK) return rc;
        if ((rc = lm_enqueue_prefill_tile128(h, m, st, lm_splits_needed(h, m), nullptr, h->imx_acc)) != RCA_OK) return rc;
        if (off + m >= n) lm_launch_head(h, 1, st, h->logits, true);   // the last position's logits, as rca_lm_score leaves them
        lm_add_rmsnorm_kernel<<<m, 64, 0, st>>>(h->stt, h->x, nullptr, nullptr, 0, 0, h->final_norm, h->xn, c.hidden, c.rms_eps, h->xh, h->xl);
        lm_collect_planes(LmTilePass{h, h->stt, m, (int)cdiv(m, 128), nullptr, g128_seq_min(), h->imx_acc}, st, 0, 4, h->xh, h->xl);
        RCA_LAUNCH_CHECK();
        h->n_tokens += m;
    }
    h->logits_rows = 1;
    RCA_HIP(hipStreamSynchronize(st));
    h->imx_count += n;
    return RCA_OK;
}
extern "C" int rca_lm_imatrix_chunk(rca_lm_t* h, const int32_t* ids, int32_t n) {
    if (!h) return fail(RCA_ERR_ARG, "imatrix_chunk: null handle");
    return lm_imatrix_chunk_impl(h, "imatrix_chunk", ids, n);
}
// tests only: one pass of the call above with the planes of (layer, kind) copied right behind their collection launch
extern "C" int rca_lm_imatrix_chunk_tap(rca_lm_t* h, const int32_t* ids, int32_t n, int32_t layer, int32_t kind, uint16_t* xh_out, uint16_t* xl_out) {
    if (!h || !xh_out || !xl_out) return fail(RCA_ERR_ARG, "imatrix_chunk_tap: null pointer");
    if (n > LM_MAXM) return fail(RCA_ERR_ARG, "imatrix_chunk_tap: %d tokens are more than one pass of %d", n, LM_MAXM);
    int K = 0;
    if (lm_imx_slot(h->cfg, layer, kind, &K) < 0) return fail(RCA_ERR_ARG, "imatrix_chunk_tap: no layer %d / kind %d (%d layers, kinds 0 .. 4)", layer, kind, h->cfg.n_layers);
    if (n < 1) return fail(RCA_ERR_ARG, "imatrix_chunk_tap: bad argument (n = %d tokens)", n);
    RCA_HIP(hipSetDevice(h->device));
    const size_t nb = (size_t)n * K * 2;
    int rc;
    if ((rc = lm_alloc((void**)&h->imx_tap_h, nb)) == RCA_OK && (rc = lm_alloc((void**)&h->imx_tap_l, nb)) == RCA_OK) {
        h->imx_tap_layer = layer;
        h->imx_tap_kind = kind;
        rc = lm_imatrix_chunk_impl(h, "imatrix_chunk_tap", ids, n);
        h->imx_tap_layer = h->imx_tap_kind = -1;
        if (rc == RCA_OK) {   // (the call has waited for the stream)
            hipError_t e = hipMemcpy(xh_out, h->imx_tap_h, nb, hipMemcpyDeviceToHost);
            if (e == hipSuccess) e = hipMemcpy(xl_out, h->imx_tap_l, nb, hipMemcpyDeviceToHost);
            if (e != hipSuccess) rc = fail(RCA_ERR_HIP, "imatrix_chunk_tap: %s", hipGetErrorString(e));
        }
    }
    for (bf16_t** p : {&h->imx_tap_h, &h->imx_tap_l}) {
        if (*p) (void)hipFree(*p);
        *p = nullptr;
    }
    return rc;
}
extern "C" int rca_lm_imatrix_get(rca_lm_t* h, int32_t layer, int32_t kind, double* sums_out, int32_t K, int64_t* count_out) {
    if (!h || !sums_out) return fail(RCA_ERR_ARG, "imatrix_get: null pointer");
    if (!h->imx_acc) return fail(RCA_ERR_STATE, "imatrix_get: the handle is not collecting (rca_lm_imatrix_begin starts a collection)");
    int want = 0;
    const long off = lm_imx_slot(h->cfg, layer, kind, &want);
    if (off < 0) return fail(RCA_ERR_ARG, "imatrix_get: no layer %d / kind %d (%d layers, kinds 0 .. 4)", layer, kind, h->cfg.n_layers);
    if (K != want) return fail(RCA_ERR_ARG, "imatrix_get: K = %d, but kind %d has a width of %d", K, kind, want);
    int rc;
    if ((rc = lm_settle(h)) != RCA_OK) return rc;
    RCA_HIP(hipSetDevice(h->device));
    RCA_HIP(hipStreamSynchronize(h->stream));
    RCA_HIP(hipMemcpy(sums_out, h->imx_acc + off, (size_t)K * 8, hipMemcpyDeviceToHost));
    if (count_out) *count_out = h->imx_count;
    return RCA_OK;
}

// ------------------------------------------------------------------------- quantising rows to GGUF blocks (rca_quantize_rows)
// One lane per super-block of 256 values (Q8_0: per block of 32): the lane runs the whole rule of rca_quant_rows.h over its block, so
// every sum has the one order the numpy restatement has and no step depends on another lane.  Not a serving path: a 1B model is 8 M
// super-blocks, enough lanes to fill the chip without splitting a block.  A block that holds a non-finite value, or whose d is not
// finite in fp16, lowers bad[0] / bad[1] to its row (vector atomicMin); the host refuses the call after its one synchronisation.
#include "rca_quant_rows.h"
template <int TYPE, typename T>
__global__ __launch_bounds__(128) void lm_quant_rows_kernel(const T* __restrict__ src, long nblocks, long blocks_per_row, long row0, int rule,
                                                            unsigned char* __restrict__ out, int* __restrict__ bad, const float* __restrict__ col_weights) {
    constexpr int NV = TYPE == RCA_Q8_0 ? 32 : 256;
    constexpr int BS = TYPE == RCA_Q8_0 ? 34 : (TYPE == RCA_Q4_K ? 144 : (TYPE == RCA_Q5_K ? 176 : 210));
    for (long blk = (long)blockIdx.x * blockDim.x + threadIdx.x; blk < nblocks; blk += (long)gridDim.x * blockDim.x) {
        int status;
        // rca_quantize_rows_w: a slab starts at a row, so block blk of it covers columns (blk % blocks_per_row) * 256 .. + 255
        const float* qw = TYPE != RCA_Q8_0 && col_weights ? col_weights + (blk % blocks_per_row) * 256 : nullptr;
        if (TYPE == RCA_Q4_K) status = rca_quant::quantize_block_qk<15>(src + blk * NV, rule, reinterpret_cast<unsigned*>(out + blk * BS), qw);
        else if (TYPE == RCA_Q5_K) status = rca_quant::quantize_block_qk<31>(src + blk * NV, rule, reinterpret_cast<unsigned*>(out + blk * BS), qw);
        else if (TYPE == RCA_Q6_K) status = rca_quant::quantize_block_q6k(src + blk * NV, rule, reinterpret_cast<unsigned short*>(out + blk * BS), qw);
        else status = rca_quant::quantize_block_q8_0(src + blk * NV, reinterpret_cast<unsigned short*>(out + blk * BS));
        if (status) {
            const int row = (int)min((long)INT_MAX - 1, row0 + blk / blocks_per_row);
            if (status & rca_quant::QS_BAD_INPUT) atomicMin(&bad[0], row);
            if (status & rca_quant::QS_BAD_D) atomicMin(&bad[1], row);
        }
    }
}
template <typename T>
static void lm_launch_quant_rows(int type, const void* src, long nblocks, long blocks_per_row, long row0, int rule, unsigned char* out, int* bad,
                                 const float* qw, hipStream_t st) {
    const unsigned grid = (unsigned)std::min<long>((nblocks + 127) / 128, 1 << 20);
    const T* s = (const T*)src;
    if (type == RCA_Q4_K) lm_quant_rows_kernel<RCA_Q4_K, T><<<grid, 128, 0, st>>>(s, nblocks, blocks_per_row, row0, rule, out, bad, qw);
    else if (type == RCA_Q5_K) lm_quant_rows_kernel<RCA_Q5_K, T><<<grid, 128, 0, st>>>(s, nblocks, blocks_per_row, row0, rule, out, bad, qw);
    else if (type == RCA_Q6_K) lm_quant_rows_kernel<RCA_Q6_K, T><<<grid, 128, 0, st>>>(s, nblocks, blocks_per_row, row0, rule, out, bad, qw);
    else lm_quant_rows_kernel<RCA_Q8_0, T><<<grid, 128, 0, st>>>(s, nblocks, blocks_per_row, row0, rule, out, bad, qw);
}

#define LM_QUANT_SLAB_BYTES (64l << 20)   // source bytes uploaded per slab (at least one row)
static int lm_quantize_rows(int32_t device, const void* src_host, int32_t src_dtype, int64_t rows, int64_t K, int32_t type, int32_t rule,
                            const float* col_weights, void* blocks_host, int64_t blocks_bytes) {
    if (!src_host || !blocks_host) return fail(RCA_ERR_ARG, "quantize_rows: null pointer");
    if (src_dtype != RCA_F32 && src_dtype != RCA_BF16 && src_dtype != RCA_F16) return fail(RCA_ERR_ARG, "quantize_rows: source dtype %d (RCA_F32, RCA_BF16 or RCA_F16)", src_dtype);
    if (type != RCA_Q8_0 && type != RCA_Q4_K && type != RCA_Q5_K && type != RCA_Q6_K) return fail(RCA_ERR_ARG, "quantize_rows: unknown type %d (RCA_Q8_0, RCA_Q4_K, RCA_Q5_K or RCA_Q6_K)", type);
    if (rule != 0 && rule != 1) return fail(RCA_ERR_ARG, "quantize_rows: unknown rule %d (0 min / max, 1 search)", rule);
    if (rows < 1 || K < 1 || rows > (1l << 40) / K) return fail(RCA_ERR_ARG, "quantize_rows: %ld rows of %ld values", (long)rows, (long)K);
    if (K % 256) return fail(RCA_ERR_ARG, "quantize_rows: K = %ld is not a multiple of 256", (long)K);
    const long nv = type == RCA_Q8_0 ? 32 : 256, bs = type == RCA_Q8_0 ? 34 : (type == RCA_Q4_K ? 144 : (type == RCA_Q5_K ? 176 : 210));
    const long bpr = K / nv, row_out = bpr * bs, esz = src_dtype == RCA_F32 ? 4 : 2, row_in = K * esz;
    if (blocks_bytes != rows * row_out) return fail(RCA_ERR_ARG, "quantize_rows: blocks_bytes = %ld, %ld rows of %ld values take %ld", (long)blocks_bytes, (long)rows, (long)K, rows * row_out);
    if (col_weights) {   // (Q8_0 has one rule and no use for weights: they are checked and not uploaded)
        if (rule != 1) return fail(RCA_ERR_ARG, "quantize_rows: column weights need rule 1 (the search), not rule %d", rule);
        for (long j = 0; j < K; ++j)
            if (!(col_weights[j] >= 0.0f) || !rca_quant::finite32(col_weights[j]))
                return fail(RCA_ERR_ARG, "quantize_rows: the weight of column %ld is negative or not finite", j);
    }
    const bool weighted = col_weights && type != RCA_Q8_0;
    RCA_HIP(hipSetDevice(device));
    const long slab_rows = std::min<long>(rows, std::max<long>(1, LM_QUANT_SLAB_BYTES / row_in));
    hipStream_t st = nullptr;
    void* src_d = nullptr;
    unsigned char* out_d = nullptr;
    int* bad_d = nullptr;
    float* qw_d = nullptr;
    int bad_h[2] = {INT_MAX, INT_MAX};
    hipError_t e = hipStreamCreateWithFlags(&st, hipStreamNonBlocking);
    if (e == hipSuccess && weighted) e = hipMalloc((void**)&qw_d, (size_t)K * 4);
    if (e == hipSuccess && weighted) e = hipMemcpyAsync(qw_d, col_weights, (size_t)K * 4, hipMemcpyHostToDevice, st);   // once per call
    if (e == hipSuccess) e = hipMalloc(&src_d, (size_t)(slab_rows * row_in));
    if (e == hipSuccess) e = hipMalloc((void**)&out_d, (size_t)(slab_rows * row_out));
    if (e == hipSuccess) e = hipMalloc((void**)&bad_d, 8);
    if (e == hipSuccess) e = hipMemcpyAsync(bad_d, bad_h, 8, hipMemcpyHostToDevice, st);
    for (long r0 = 0; e == hipSuccess && r0 < rows; r0 += slab_rows) {   // stream order makes the one pair of slab buffers safe to reuse
        const long nr = std::min(slab_rows, rows - r0);
        e = hipMemcpyAsync(src_d, (const char*)src_host + r0 * row_in, (size_t)(nr * row_in), hipMemcpyHostToDevice, st);
        if (e != hipSuccess) break;
        if (src_dtype == RCA_F32) lm_launch_quant_rows<float>(type, src_d, nr * bpr, bpr, r0, rule, out_d, bad_d, qw_d, st);
        else if (src_dtype == RCA_BF16) lm_launch_quant_rows<rca_quant::bf16_src>(type, src_d, nr * bpr, bpr, r0, rule, out_d, bad_d, qw_d, st);
        else lm_launch_quant_rows<rca_quant::f16_src>(type, src_d, nr * bpr, bpr, r0, rule, out_d, bad_d, qw_d, st);
        e = hipGetLastError();
        if (e == hipSuccess) e = hipMemcpyAsync((char*)blocks_host + r0 * row_out, out_d, (size_t)(nr * row_out), hipMemcpyDeviceToHost, st);
    }
    if (e == hipSuccess) e = hipMemcpyAsync(bad_h, bad_d, 8, hipMemcpyDeviceToHost, st);
    if (st) {
        const hipError_t es = hipStreamSynchronize(st);
        if (e == hipSuccess) e = es;
    }
    for (void* p : {src_d, (void*)out_d, (void*)bad_d, (void*)qw_d})
        if (p) (void)hipFree(p);
    if (st) (void)hipStreamDestroy(st);
    if (e != hipSuccess) return fail(RCA_ERR_HIP, "quantize_rows: %s", hipGetErrorString(e));
    if (bad_h[0] != INT_MAX) return fail(RCA_ERR_ARG, "quantize_rows: row %d holds a value that is not finite", bad_h[0]);
    if (bad_h[1] != INT_MAX) return fail(RCA_ERR_ARG, "quantize_rows: row %d: a block's d or dmin is not finite in fp16", bad_h[1]);
    return RCA_OK;
}
extern "C" int rca_quantize_rows(int32_t device, const void* src_host, int32_t src_dtype, int64_t rows, int64_t K, int32_t type, int32_t rule,
                                 void* blocks_host, int64_t blocks_bytes) {
    return lm_quantize_rows(device, src_host, src_dtype, rows, K, type, rule, nullptr, blocks_host, blocks_bytes);
}
extern "C" int rca_quantize_rows_w(int32_t device, const void* src_host, int32_t src_dtype, int64_t rows, int64_t K, int32_t type, int32_t rule,
                                   const float* col_weights, void* blocks_host, int64_t blocks_bytes) {
    return lm_quantize_rows(device, src_host, src_dtype, rows, K, type, rule, col_weights, blocks_host, blocks_bytes);
}

// ------------------------------------------------------------------------------------ the opt-in samplers' kernels (declared in front of lm_enqueue_sample)
__global__ __launch_bounds__(1024) void samp_final_typ_kernel(float* logits, int V, const SamplerDev* __restrict__ sp,
                                                              LmDevState* __restrict__ stt, SampWork* __restrict__ w, SampTail tail) {
    samp_final_body<true>(logits, V, sp, stt, w, tail);
}

// ---- mirostat v2 (llama_sampler_mirostat_v2_apply; llama-cpp-python's chain is then logit bias -> penalties -> temp -> mirostat:
// top_k, typical, top_p and min_p are left out).  tests/samp_ext_ref.py is the definition.  Per draw c, with mx the row's maximum,
// x_i = (v_i - mx) * (1 / temp), e_i = rca_expf(x_i) and masses w_i = trunc(e_i * 2^40):
//   S   = sum of w_i over the vocabulary (integer: the same whatever the slices), lnS = rca_logf((float)S * 2^-40);
//   kept: surprise_i = (lnS - x_i) * log2(e) <= mu, mu = SampWork::mu_ring[c % SAMP_RING].  When not even the top token passes, the
//         lowest index among the maxima alone is kept (and drawn);
//   draw: the whole-vocabulary sampler's Gumbel-max pick over the kept tokens, same keyed RNG;
//   S'  = sum of w_i over the kept tokens, observed = (rca_logf((float)S' * 2^-40) - x_tok) * log2(e),
//   mu_ring[(c + 1) % SAMP_RING] = mu - eta * (observed - tau).
// Four launches: slice maxima (samp_full_max_kernel), slice masses, slice picks + kept masses, one-workgroup merge + the common tail.
// Contraction is off in all of them: every product and sum above is one float32 operation, as in the restatement.
#define SAMP_LOG2E 1.44269504f
#define SAMP_FX_INV 9.094947017729282e-13f   // 2^-40
__device__ __forceinline__ float samp_slices_max(const SampWork* __restrict__ w) {
    const float* smax = reinterpret_cast<const float*>(w->hist);
    float mx = smax[0];
    for (int k = 1; k < SAMPF_SLICES; ++k) mx = fmaxf(mx, smax[k]);
    return mx;
}
__device__ __forceinline__ unsigned long long samp_block_sum_u64(unsigned long long v, unsigned long long* red) {   // valid in thread 0
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    unsigned long long s = 0ull;
    if (threadIdx.x == 0)
        for (int k = 0; k < 16; ++k) s += red[k];
    return s;
}
__device__ __forceinline__ unsigned long long samp_miro_total(const SampWork* __restrict__ w, int which) {
    unsigned long long s = 0ull;
    for (int k = 0; k < SAMPF_SLICES; ++k) s += w->miro_part[which][k];
    return s;
}
__global__ __launch_bounds__(1024) void samp_miro_mass_kernel(const float* __restrict__ logits, int V, const SamplerDev* __restrict__ sp,
                                                              SampWork* __restrict__ w) {
#pragma clang fp contract(off)
    __shared__ unsigned long long red[16];
    const float mx = samp_slices_max(w), inv_t = 1.0f / sp->temp;
    const int per = (V + SAMPF_SLICES - 1) / SAMPF_SLICES;
    const int i0 = blockIdx.x * per, i1 = min(V, i0 + per);
    unsigned long long acc = 0ull;
    for (int i = i0 + threadIdx.x; i < i1; i += 1024) {
        const float x = (samp_value(logits, sp, i) - mx) * inv_t;
        acc += samp_mass_fx(x);
    }
    acc = samp_block_sum_u64(acc, red);
    if (threadIdx.x == 0) w->miro_part[0][blockIdx.x] = acc;
}
__global__ __launch_bounds__(1024) void samp_miro_pick_kernel(const float* __restrict__ logits, int V, const SamplerDev* __restrict__ sp,
                                                              const LmDevState* __restrict__ stt, SampWork* __restrict__ w) {
#pragma clang fp contract(off)
    __shared__ unsigned long long red[16], redm[16];
    const float mx = samp_slices_max(w), inv_t = 1.0f / sp->temp;
    const unsigned long long c = stt->rng_counter;
    const float mu = w->mu_ring[c % SAMP_RING];
    const float lnS = rca_logf((float)samp_miro_total(w, 0) * SAMP_FX_INV);
    const bool top_only = !(lnS * SAMP_LOG2E <= mu);
    const unsigned long long draw = splitmix(sp->seed, c);
    const int per = (V + SAMPF_SLICES - 1) / SAMPF_SLICES;
    const int i0 = blockIdx.x * per, i1 = min(V, i0 + per);
    unsigned long long best = 0ull, mass = 0ull;
    for (int i = i0 + threadIdx.x; i < i1; i += 1024) {
        const float v = samp_value(logits, sp, i);
        const float d = v - mx;
        unsigned long long key;
        if (top_only) {
            if (!(v == mx)) continue;
            key = sample_key(0.0f, (unsigned)i);
        } else {
            const float x = d * inv_t;
            const float surprise = (lnS - x) * SAMP_LOG2E;
            if (!(surprise <= mu)) continue;
            mass += samp_mass_fx(x);
            const unsigned long long z = splitmix(draw, (unsigned long long)i);
            const float u = (float)(unsigned)(((z >> 41) << 1) | 1ull) * 5.9604644775390625e-08f;
            const float g = -rca_logf(-rca_logf(u));
            key = sample_key(__builtin_fmaf(d, inv_t, g), (unsigned)i);
        }
        best = key > best ? key : best;
    }
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned long long o = __shfl_xor(best, off);
        best = o > best ? o : best;
    }
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = best;
    mass = samp_block_sum_u64(mass, redm);   // (its barrier also publishes red)
    if (threadIdx.x == 0) {
        unsigned long long b = red[0];
        for (int k = 1; k < 16; ++k) b = red[k] > b ? red[k] : b;
        w->cand[blockIdx.x] = b;
        w->miro_part[1][blockIdx.x] = mass;
    }
}
__global__ __launch_bounds__(1024) void samp_miro_final_kernel(float* logits, int V, const SamplerDev* __restrict__ sp, LmDevState* __restrict__ stt,
                                                               SampWork* __restrict__ w, SampTail tail) {
#pragma clang fp contract(off)
    __shared__ int s_tok;
    __shared__ unsigned long long s_draw;
    const int tid = threadIdx.x;
    if (tid == 0) {
        unsigned long long b = w->cand[0];
        for (int k = 1; k < SAMPF_SLICES; ++k) b = w->cand[k] > b ? w->cand[k] : b;
        const int tok = (int)(0xFFFFFFFFu - (unsigned)(b & 0xFFFFFFFFull));
        const unsigned long long c = stt->rng_counter;
        const float mx = samp_slices_max(w), inv_t = 1.0f / sp->temp;
        const float mu = w->mu_ring[c % SAMP_RING];
        const float lnS = rca_logf((float)samp_miro_total(w, 0) * SAMP_FX_INV);
        const bool top_only = !(lnS * SAMP_LOG2E <= mu);
        const unsigned long long kept = top_only ? (1ull << 40) : samp_miro_total(w, 1);
        const float x_tok = (logits[tok < 0 ? 0 : (tok >= V ? V - 1 : tok)] - mx) * inv_t;   // (the row is still patched: the value the passes saw)
        const float observed = (rca_logf((float)kept * SAMP_FX_INV) - x_tok) * SAMP_LOG2E;
        const float err = observed - sp->miro_tau;
        const float step = sp->miro_eta * err;
        w->mu_ring[(c + 1ull) % SAMP_RING] = mu - step;
        s_draw = c;
        stt->rng_counter = c + 1ull;
        stt->out_token = tok;
        if (tail.frame_i >= 0) {
            stt->frame_out[tail.frame_i] = tok;
            stt->n_tokens += 2;
            stt->ids[0] = tok;
            stt->ids[1] = stt->ids[LM_FRAME_USER0 + tail.frame_i];
        }
        s_tok = tok;
    }
    __syncthreads();
    samp_accept_and_restore(logits, sp, w, s_draw, s_tok, tid);
    for (int b = tid; b < SAMPF_SLICES; b += 1024) w->hist[b] = 0u;   // the top-k sampler expects a zeroed histogram
    if (tail.frame_i >= 0) {   // lm_embed_kernel for the next pair (m = 2), as in samp_final_kernel
        const int id1 = stt->ids[LM_FRAME_USER0 + tail.frame_i];
        for (int e = tid; e < 2 * tail.H; e += 1024) {
            const int m = e / tail.H, hh = e - m * tail.H;
            int id = m == 0 ? s_tok : id1;
            id = id < 0 ? 0 : (id >= V ? V - 1 : id);
            tail.x[e] = tail.f32tab ? reinterpret_cast<const float*>(tail.table)[(long)id * tail.H + hh]
                                    : __uint_as_float((unsigned)reinterpret_cast<const bf16_t*>(tail.table)[(long)id * tail.H + hh] << 16);
        }
    }
}
