/*
 * rca.h -- C ABI of the MI355X-native duplex codec-LM hot path.
 *
 * The reference (AbrahamSanders/realtime-codec-agent) has no FFI of its own: its
 * seams are two duck-typed Python objects held by RealtimeAgentResources
 * (realtime_agent_resources.py:19-39).  This header is the C boundary that sits
 * *behind* Python classes with those surfaces.  Each entry
 * point cites the reference call it replaces.
 *
 * Conventions
 *   - every function returns int: 0 = RCA_OK, <0 = error (rca_last_error() has text);
 *     no exception crosses the boundary
 *   - plain pointers and sizes only; no torch / C++ types
 *   - the caller owns every I/O buffer; the library owns weights, KV cache, workspace
 *   - one handle per stream, handles are not re-entrant (matches the reference:
 *     AudioTokenizer and llama_cpp.Llama are single-threaded objects)
 *   - "_dev" variants take device (HBM) pointers and a hipStream_t passed as void*;
 *     the plain variants take host pointers and do the H2D/D2H copies themselves
 */
#ifndef RCA_H
#define RCA_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RCA_OK 0
#define RCA_ERR_ARG -1      /* bad argument / shape */
#define RCA_ERR_HIP -2      /* a HIP runtime call failed */
#define RCA_ERR_STATE -3    /* wrong call order / context overflow */
#define RCA_ERR_MISSING -4  /* a named tensor was not supplied */

#define RCA_MAX_STAGES 8

typedef struct rca_codec rca_codec_t;
typedef struct rca_lm rca_lm_t;

/* dtype tags for rca_tensor_t */
#define RCA_F32 0
#define RCA_BF16 1
#define RCA_Q8_0 2   /* GGUF block_q8_0 as stored in the file: per 32 values one fp16 scale then 32 int8 (34 bytes); numel = values */
#define RCA_F16 3    /* IEEE half (the reference's default model file is an F16 GGUF, realtime_agent_resources.py:12) */
#define RCA_Q6_K 5   /* GGUF block_q6_K as stored in the file (210 bytes per 256 values: low nibbles, high bit pairs, 16 int8 scales, fp16 d): the
                        format llama-quantize Q4_K_M gives output.weight and some attn_v / ffn_down tensors */
#define RCA_Q4_K 4   /* GGUF block_q4_K as stored in the file: per 256 values fp16 d, fp16 dmin, 12 bytes of 6-bit scales / minima, 128 bytes
                        of nibbles (144 bytes); numel = values.  What llama-quantize Q4_K_M writes for most tensors (prep_test_model.sh:31) */
/* Q5_K carries three numbers, each in a numbering of its own that existed before it: the tensor dtype RCA_Q5_K = 6 (next free dtype),
   rca_lm_config_t::decode_weights = 4 (next free load-time conversion) and the id 5 that rca_lm_weight_format reports (the library's
   format ids: 0 bf16, 1 q8_0, 2 f16, 3 q4_k, 4 q6_k, 5 q5_k). */
#define RCA_Q5_K 6   /* GGUF block_q5_K as stored in the file: per 256 values fp16 d, fp16 dmin, 12 bytes of 6-bit scales / minima (packed as in
                        Q4_K), 32 bytes of high bits, 128 bytes of nibbles (176 bytes); numel = values.  The bulk of a llama-quantize Q5_K_S /
                        Q5_K_M file (the rest of such a file is Q6_K) */
/* Q4_0 / Q4_1 likewise carry three numbers each: the tensor dtypes RCA_Q4_0 = 7 and RCA_Q4_1 = 8 (next free dtypes),
   rca_lm_config_t::decode_weights = 5 / 6 (next free load-time conversions) and the ids 6 / 7 that rca_lm_weight_format reports
   (the library's format ids: 0 bf16, 1 q8_0, 2 f16, 3 q4_k, 4 q6_k, 5 q5_k, 6 q4_0, 7 q4_1). */
#define RCA_Q4_0 7   /* GGUF block_q4_0 as stored in the file: per 32 values fp16 d then 16 bytes of nibbles (18 bytes; value j of the block in the
                        low nibble of byte j, value j + 16 in the high nibble); value = d (q - 8); numel = values.  What llama-quantize Q4_0
                        writes for most tensors.  A block whose 8 d is not finite in fp16 is refused at load (RCA_ERR_ARG, with the tensor's name) */
#define RCA_Q4_1 8   /* GGUF block_q4_1: fp16 d, fp16 m, 16 bytes of nibbles (20 bytes); value = d q + m.  What llama-quantize Q4_0 gives some
                        ffn_down tensors when an importance matrix is supplied */
/* IQ4_NL / IQ4_XS likewise carry three numberings: the tensor dtypes RCA_IQ4_NL = 9 and RCA_IQ4_XS = 10 (next free dtypes),
   rca_lm_config_t::decode_weights = 7 for IQ4_NL (next free load-time conversion; there is no load-time IQ4_XS) and the ids 8 / 9 that
   rca_lm_weight_format reports (the library's format ids: 0 bf16, 1 q8_0, 2 f16, 3 q4_k, 4 q6_k, 5 q5_k, 6 q4_0, 7 q4_1, 8 iq4_nl,
   9 iq4_xs).  Both types index the 16-entry int8 table kvalues_iq4nl = { -127, -104, -83, -65, -49, -35, -22, -10, 1, 13, 25, 38,
   53, 69, 89, 113 } (restated from the published ggml definitions; ggml is not part of this tree: parity with llama-quantize's own
   bits is not pinned). */
#define RCA_IQ4_NL 9  /* GGUF block_iq4_nl as stored in the file: per 32 values fp16 d then 16 bytes of nibbles (18 bytes; Q4_0's nibble order);
                         value = d kv[q]; numel = values.  A block whose d is not finite is refused at load (RCA_ERR_ARG, with the tensor's name) */
#define RCA_IQ4_XS 10 /* GGUF block_iq4_xs: per 256 values fp16 d, uint16 scales_h, 4 bytes scales_l, 128 bytes of nibbles (136 bytes).  Sub-block
                         ib = 0..7 of 32 values has the 6-bit scale ls = ((scales_l[ib / 2] >> 4 (ib % 2)) & 15) | (((scales_h >> 2 ib) & 3) << 4)
                         and value = d (ls - 32) kv[q], nibbles of qs[16 ib ..] in Q4_0's order.  The bulk of a llama-quantize IQ4_XS file */

/* A named host tensor handed to a create() call (weights). */
typedef struct {
    const char* name;
    const void* data;  /* host pointer */
    int64_t numel;
    int32_t dtype;     /* RCA_F32, RCA_BF16, RCA_F16, RCA_Q8_0, RCA_Q4_K, RCA_Q5_K, RCA_Q6_K, RCA_Q4_0, RCA_Q4_1, RCA_IQ4_NL or RCA_IQ4_XS (the last eight: LM matrices and embedding table only) */
} rca_tensor_t;

const char* rca_last_error(void);
int rca_device_count(int* n);
/* hipDeviceSynchronize on `device`: the duplex profiler's fence before every timestamp (the reference's
 * realtime_agent_profiler.py:30-38 takes its timestamps without one) */
int rca_device_sync(int32_t device);
const char* rca_version(void);

/* ------------------------------------------------------------------ codec --
 * MagiCodec-style model object.  Architecture is described by
 * rca_codec_config_t; tensors are named as in oracle/codec_ref.py:
 *   enc.conv_in.{weight,bias}            [C0,1,k_in]
 *   enc.down.{i}.{weight,bias}           [C(i+1),C(i),2*s_i]
 *   enc.conv_out.{weight,bias}           [D,C_last,k_latent]
 *   quantizer.in_proj.{weight,bias}      [cd,D]
 *   quantizer.codebook.weight            [N,raw]
 *   quantizer.codebook_proj.{weight,bias}[cd,raw]
 *   dec.conv_in.{weight,bias}            [C_last,cd,k_latent]
 *   dec.up.{i}.{weight,bias}             [C(n-i),C(n-i-1),2*s]  (ConvTranspose1d layout [Cin,Cout,k])
 *   dec.conv_out.{weight,bias}           [1,C0,k_in]
 */
typedef struct {
    int32_t sample_rate;                  /* 16000 */
    int32_t n_stages;                     /* 4 */
    int32_t strides[RCA_MAX_STAGES];      /* 2,4,5,8 -> hop 320 (50 Hz) */
    int32_t channels[RCA_MAX_STAGES + 1]; /* 32,64,128,256,512 */
    int32_t k_in;                         /* 7 */
    int32_t k_latent;                     /* 3 */
    int32_t latent_dim;                   /* 256 */
    int32_t codebook_size;                /* 131072 */
    int32_t codebook_raw_dim;             /* 32 */
    int32_t codebook_dim;                 /* 16 */
    float leaky_slope;                    /* 0.1 */
} rca_codec_config_t;

/* replaces codec_bpe.tools.codec_utils.load_magicodec_model + .eval().to(device)
 * (audio_tokenizer.py:26-28).  The projected codebook and its half-norms are
 * computed once here instead of on every decode (audio_tokenizer.py:198). */
int rca_codec_create(const rca_codec_config_t* cfg, const rca_tensor_t* tensors, int32_t n_tensors,
                     int32_t device, rca_codec_t** out);
int rca_codec_destroy(rca_codec_t* h);
/* total stride of the encoder (samples per frame) */
int rca_codec_hop(const rca_codec_t* h, int32_t* hop);
/* frames produced for T samples: ceil(T / hop) (pad_audio right-pads to a hop multiple) */
int rca_codec_num_frames(const rca_codec_t* h, int32_t T, int32_t* F);

/* AudioTokenizer._magicodec_encode (audio_tokenizer.py:189-194):
 * pad_audio -> encoder -> quantizer.inference.  pcm [B,T] f32 -> codes [B,F] int64. */
int rca_codec_encode(rca_codec_t* h, const float* pcm_host, int32_t B, int32_t T, int64_t* codes_host);
int rca_codec_encode_dev(rca_codec_t* h, const float* pcm_dev, int32_t B, int32_t T, int64_t* codes_dev,
                         void* stream);

/* codec_bpe.audio_to_codes as driven by encode_audio_gpu_*.sh (--chunk_size_secs,
 * --context_secs, --batch_size): every `hop_samples` chunk of a long signal is
 * encoded with `ctx_samples` of left context and only the chunk's own codes are
 * kept (same rule as AudioTokenizer.tokenize_audio, audio_tokenizer.py:72-101).
 * audio [C,N] f32 resident in HBM -> codes [C, n_chunks*frames_per_chunk] int64.
 * Windows are cut on the device; `batch_windows` windows are encoded per pass. */
int rca_codec_encode_windows_dev(rca_codec_t* h, const float* audio_dev, int32_t C, int64_t N,
                                 int32_t chunk_samples, int32_t ctx_samples, int32_t batch_windows,
                                 int64_t* codes_dev, int64_t codes_per_channel, void* stream);

/* Same, restricted to chunks [chunk_begin, chunk_end) of the signal (left context is read from
 * the signal itself): the unit of work a batch shard / one bench step encodes.  Codes of chunk i
 * land at codes_dev[c * codes_per_channel + (i - chunk_begin) * frames_per_chunk ...]. */
int rca_codec_encode_chunk_range_dev(rca_codec_t* h, const float* audio_dev, int32_t C, int64_t N,
                                     int32_t chunk_samples, int32_t ctx_samples, int32_t batch_windows,
                                     int64_t chunk_begin, int64_t chunk_end, int64_t* codes_dev,
                                     int64_t codes_per_channel, void* stream);

/* The same per-window arithmetic for B windows of T samples taken ANYWHERE in one device buffer -- window b starts at
 * audio_dev + src_off_dev[b] (elements), its last n_keep codes go to codes_dev + dst_off_dev[b]; `span` = largest offset + T.
 * codec_bpe.audio_to_codes fills its --batch_size windows from one file at a time (encode_audio_gpu_1.sh:2-8 over corpora of
 * short utterances); with this call a pass holds windows of many files, including every file's short warm-up windows
 * (the rolling context is still shorter than context_secs, audio_tokenizer.py:72-74), grouped by length. */
int rca_codec_encode_rows_dev(rca_codec_t* h, const float* audio_dev, const int64_t* src_off_dev, int32_t B, int32_t T, int32_t n_keep,
                              int64_t* codes_dev, const int64_t* dst_off_dev, int64_t span, void* stream);

/* Device ingest for the batch CLI: PCM as the file holds it (int16 or f32, interleaved or planar, at the file's rate) -> the f32
 * rows at the codec rate that rca_codec_encode_rows_dev reads.  One launch converts, de-interleaves, downmixes and resamples.
 * Row r takes n_in frames; frame k is the mean of the n_mix elements src[src_off + k * src_stride + c], c < n_mix (int16: v * 2^-15,
 * exact; f32 as it is; the sum in ascending c in f32, then one IEEE division by n_mix; n_mix == 1 takes the element unchanged).
 * With t = n * down + (n_taps - 1) / 2 the row's n_out = ceil(n_in * up / down) outputs are
 *     y[n] = sum over k in [0, n_in) with 0 <= t - k * up < n_taps of taps[t - k * up] * m[k]      (zero beyond both ends)
 * -- scipy.signal.resample_poly's definition -- stored at dst_dev[dst_off + n].  The sum is an f32 fma chain over k descending from
 * floor(t / up), ceil(n_taps / up) terms (taps past the table and frames past the row enter as zeros): the bits depend on
 * (n, up, down, taps, the row's frames) only, never on where the row lies, on the grid or on the other rows of the call.
 * up == down == 1 is the pure conversion / de-interleave / downmix: exact, the taps are not consulted.
 * Every row of a call shares (src_fmt, up, down, taps).  rows_host is the host copy of rows_dev: the grid and every check come from
 * it, nothing is read back.  RCA_ERR_ARG before anything is enqueued for: an even n_taps, up / down / n_mix / src_stride < 1,
 * n_mix > src_stride (a planar row has one channel), a row reaching outside [0, src_span) elements of src_dev or
 * [0, dst_span) of dst_dev, and a ratio whose phase table and input tile do not fit the kernel's LDS budget (64 KiB; every ratio
 * from 8000 / 11025 / 12000 / 22050 / 24000 / 32000 / 44100 / 48000 Hz to 16000 Hz fits) -- rca_codec_ingest_supported asks that
 * last question alone.  The phase table of a (up, down, taps) is uploaded on its first call (a blocking copy: not inside a stream
 * capture) and kept on the handle; later calls only enqueue on `stream`. */
#define RCA_PCM_F32 0
#define RCA_PCM_S16 1
typedef struct {
    int64_t src_off;    /* element offset (in elements of the source format) of channel 0 of the row's first frame */
    int64_t n_in;       /* frames; 0 writes nothing */
    int64_t dst_off;    /* element offset of the row's first output sample in dst_dev */
    int32_t src_stride; /* elements between consecutive frames: the interleaved channel count, 1 for planar rows */
    int32_t n_mix;      /* channels averaged into the row */
} rca_ingest_row_t;
int rca_codec_ingest_rows_dev(rca_codec_t* h, const void* src_dev, int64_t src_span, int32_t src_fmt, const rca_ingest_row_t* rows_dev,
                              const rca_ingest_row_t* rows_host, int32_t n_rows, int32_t up, int32_t down, const float* taps_host,
                              int32_t n_taps, float* dst_dev, int64_t dst_span, void* stream);
int rca_codec_ingest_supported(const rca_codec_t* h, int32_t up, int32_t down, int32_t n_taps);

/* Streaming tail of the encoder.  AudioTokenizer.tokenize_audio re-encodes the whole rolling
 * window for every chunk and keeps only the last int(secs*framerate) codes (audio_tokenizer.py:72-74,98-101).
 * This returns exactly those codes -- bit-identical to the last n_keep columns of rca_codec_encode_dev(pcm, B, T) --
 * but runs the encoder only over the frames whose receptive field reaches them (n_keep + enc_left_frames whole
 * frames; the frame grid and the right edge of the window are unchanged).  Valid because this build's codec is a
 * finite-receptive-field conv stack; rca_codec_receptive_field reports the margins derived from the geometry.
 * pcm [B,T] f32 (row stride T) -> codes [B,n_keep] int64. */
int rca_codec_encode_tail_dev(rca_codec_t* h, const float* pcm_dev, int32_t B, int32_t T, int32_t n_keep,
                              int64_t* codes_dev, void* stream);
/* Streaming tail of the decoder: the last n_samples of rca_codec_decode_dev(codes, B, F), bit-identical
 * (AudioTokenizer.detokenize_audio keeps int(secs*sr)+preroll samples of a 100-code window,
 * audio_tokenizer.py:113,141-145).  codes [B,F] int64 (row stride F) -> pcm [B,n_samples] f32. */
int rca_codec_decode_tail_dev(rca_codec_t* h, const int64_t* codes_dev, int32_t B, int32_t F, int32_t n_samples,
                              float* pcm_dev, void* stream);
/* The decode mirror of rca_codec_encode_rows_dev: B rows of F codes taken ANYWHERE in one device buffer -- row b is the F codes at
 * codes_dev + src_off_dev[b] (elements; rows may overlap, as consecutive windows of one stream do) and the last n_samples of its decode
 * go to pcm_dev + dst_off_dev[b].  Each row is bit-identical to row b of rca_codec_decode_tail_dev on the same codes, the receptive-field
 * trim included (the decoder runs over frames j = max(0, f0 - dec_left_frames) onwards, f0 the first frame a kept sample belongs to).
 * Replaces one AudioTokenizer.detokenize_audio call per 0.1 s chunk and per file (audio_tokenizer.py:106-149 as driven by the loop of
 * run_stream_codes.py:60-68): a pass holds the windows of many chunks of many streams.  code_span / pcm_span = largest offset + F /
 * + n_samples.  Destination rows must not overlap: that is the caller's contract, nothing checks it.
 * RCA_ERR_ARG before anything is enqueued for B < 1, F < 1, n_samples < 1, n_samples > F * hop, a null pointer or a span that holds no
 * row.  The offset tables live on the device, so a row outside its span is caught by the kernels: it is not read / not written and
 * raises the handle's decode error flag, as a code outside [0, codebook_size) does (rca_codec_decode_error). */
int rca_codec_decode_rows_dev(rca_codec_t* h, const int64_t* codes_dev, const int64_t* src_off_dev, int32_t B, int32_t F, int32_t n_samples,
                              float* pcm_dev, const int64_t* dst_off_dev, int64_t code_span, int64_t pcm_span, void* stream);
/* The error flag the decode kernels raise on the device (code out of range, row outside its span): synchronises `stream`, returns
 * the flag in *raised and clears it.  The host-buffer decode calls read it themselves; the _dev calls leave it to the caller. */
int rca_codec_decode_error(rca_codec_t* h, void* stream, int32_t* raised);

/* smooth_join (utils/audio_utils.py:22-30) for many streams in ONE launch: the loop of run_stream_codes.py:60-68 joins every
 * decoded chunk to the audio so far, `audio = smooth_join(audio, chunk, L, fade_in, fade_out)`, on the host.  Here seg_dev holds
 * decoded segments (each the preroll + chunk that detokenize_audio returned), segment s being the n samples at seg_off that land at
 * out_off in out_dev.  The descriptors of one stream are consecutive; flags bit 0 marks the head of a stream (nothing to blend
 * into), bit 1 its tail (no successor).  Inside a stream out_off[s + 1] == out_off[s] + n[s] - n_fade: the last n_fade samples of
 * segment s meet the first n_fade of segment s + 1, and there the output is
 *     prev * fade_out[k] + cur * fade_in[k],   fade_out[k] = fade_in[n_fade - 1 - k]
 * evaluated as numpy does: two f32 products, each rounded, then one f32 sum (never a fused multiply-add).  Every other sample is a
 * copy; every output sample is written by exactly one thread; n_fade == 0 is pure concatenation.  fade_in_dev: n_fade floats on the
 * device (create_crossfade_ramps, utils/audio_utils.py:14-19).  segs_host is the host copy of segs_dev: every check comes from it,
 * nothing is read back.  RCA_ERR_ARG before anything is enqueued for: a first segment that is no head, a head inside an open stream,
 * a last segment that is no tail, a broken out_off chain, a segment with a predecessor or with a successor shorter than n_fade, one
 * with both shorter than 2 * n_fade, a negative length, and anything reaching outside [0, seg_span) / [0, out_span).  The outputs of
 * different streams must not overlap (the caller's contract). */
#define RCA_JOIN_HEAD 1
#define RCA_JOIN_TAIL 2
typedef struct {
    int64_t seg_off;   /* element offset of the segment's first sample in seg_dev */
    int64_t n;         /* samples, preroll included */
    int64_t out_off;   /* element offset in out_dev of the segment's first sample */
    int32_t flags;     /* RCA_JOIN_HEAD | RCA_JOIN_TAIL */
    int32_t reserved;  /* 0 */
} rca_join_seg_t;
int rca_codec_crossfade_join_dev(rca_codec_t* h, const float* seg_dev, int64_t seg_span, const rca_join_seg_t* segs_dev,
                                 const rca_join_seg_t* segs_host, int32_t n_segs, const float* fade_in_dev, int32_t n_fade, float* out_dev,
                                 int64_t out_span, void* stream);

/* The same two calls with host buffers, as the streaming tokenizer makes them once per frame: H2D of the window,
 * the tail kernels, D2H of the result, one synchronisation.  Shapes repeat frame after frame, so from the second
 * call of a shape on the whole sequence replays as one hipGraph over pinned staging buffers
 * (rca_codec_set_stream_graphs(h, 0) switches the replay off).  Error behaviour as rca_codec_encode / _decode. */
int rca_codec_encode_tail(rca_codec_t* h, const float* pcm_host, int32_t B, int32_t T, int32_t n_keep, int64_t* codes_host);
int rca_codec_decode_tail(rca_codec_t* h, const int64_t* codes_host, int32_t B, int32_t F, int32_t n_samples, float* pcm_host);
int rca_codec_set_stream_graphs(rca_codec_t* h, int32_t enable);
/* Opt-in arithmetic of the encoder's MFMA conv layers (never the default; the default, 0, is the f32 matrix instruction whose
 * results equal the oracle's fma chains bit for bit).  3: bf16 matrix instruction on operands split into bf16 hi + lo (three
 * products per step, ~2^-16 relative); 1: operands rounded to bf16, one product -- the arithmetic class of the reference's own GPU
 * path, bf16 autocast (audio_tokenizer.py:24,78-82).  Neither is bit-exact: ids can differ from mode 0 near ties (bench.py reports
 * the measured fraction).  Decoder and streaming-tail kernels are not affected. */
int rca_codec_set_mfma_mode(rca_codec_t* h, int32_t mode);
/* whole frames a kept code / a kept sample can see to its left */
int rca_codec_receptive_field(const rca_codec_t* h, int32_t* enc_left_frames, int32_t* dec_left_frames);
/* Batch windows (rca_codec_encode_windows_dev / _chunk_range_dev): when enabled, each window is cut down to the
 * frames its kept codes can see -- same codes for any ctx_samples >= the receptive field, ~10x less work at
 * 2.0 s context.  Off by default: the default path computes every window in full, as the reference does. */
int rca_codec_set_window_trim(rca_codec_t* h, int32_t enable);

/* AudioTokenizer._magicodec_decode (audio_tokenizer.py:196-201):
 * embedding(codes, codebook_proj(codebook.weight)) -> decoder -> f32 PCM.
 * codes [B,F] int64 -> pcm [B,F*hop] f32. */
int rca_codec_decode(rca_codec_t* h, const int64_t* codes_host, int32_t B, int32_t F, float* pcm_host);
int rca_codec_decode_dev(rca_codec_t* h, const int64_t* codes_dev, int32_t B, int32_t F, float* pcm_dev,
                         void* stream);

/* The three sub-steps of the model object, for callers that drive them separately the way
 * the reference does (audio_tokenizer.py:190-192,198-200):
 *   codec_model.encoder(pad_audio(x))      pcm [B,T] -> z_e [B,F,D] f32
 *   codec_model.quantizer.inference(z_e)   z_e [R,D] -> idx [R] int64 (R = B*F rows)
 *   codec_model.decoder(z_q)               z_q [B,F,cd] -> pcm [B,F*hop] f32 */
int rca_codec_encoder_dev(rca_codec_t* h, const float* pcm_dev, int32_t B, int32_t T, float* ze_dev, void* stream);
int rca_codec_quantize_dev(rca_codec_t* h, const float* ze_dev, int64_t rows, int64_t* codes_dev, void* stream);
int rca_codec_decoder_dev(rca_codec_t* h, const float* zq_dev, int32_t B, int32_t F, float* pcm_dev, void* stream);
/* device pointer of the projected codebook [codebook_size, codebook_dim] f32 (owned by the handle) */
int rca_codec_codebook_dev(rca_codec_t* h, const float** out_dev);

/* AudioTokenizer.get_codec_embeddings (audio_tokenizer.py:151-159): projected
 * codebook [codebook_size, codebook_dim] f32, copied to the host. */
int rca_codec_codebook(rca_codec_t* h, float* out_host);

/* Debug/parity taps (tests only): run the encoder and copy the activation after
 * layer `layer` (0=conv_in, 1..n=down, n+1=conv_out, n+2=in_proj z) to the host.
 * A tapped pass (layer <= n+1) is NOT the pass encode() runs: it runs without the LeakyReLU
 * hand-off between layers (no layer stores an activated output, none reads one), without the
 * kept-frames view of conv_out and, for layer 0, without the fusion of conv_in into the first
 * strided layer.  Those launches are reached by rca_codec_encoder_layer_tap below. */
int rca_codec_encode_tap(rca_codec_t* h, const float* pcm_host, int32_t B, int32_t T, int32_t layer,
                         float* out_host, int64_t out_numel);

/* Tests only: run encode()'s bf16 blocked pipeline (mfma mode 1 / 3) through encoder layer `layer`
 * and copy the bf16 planes it stored for the next layer: hi and, in mode 3, lo, as raw bf16 bits.
 * RCA_ERR_ARG when encode() would not take the blocked pipeline for this mode / shape, or the
 * layer is not materialised (layer 0 while conv_in is fused, or the last layer, which is f32).
 * Same launches and instantiations as encode() for layers 0..layer; nothing after them runs.
 * Layout as stored, channel-blocked: [B][C / 16][L][C % 16], numel = B * C * L of that layer.
 * The stored values are the layer's f32 accumulator after LeakyReLU (max(v, slope * v), in f32:
 * every layer this pipeline materialises feeds a pre-activated layer), then rounded to nearest
 * even (mode 1: hi only; lo_host may be NULL and is not written) or split (mode 3: hi = rne(v),
 * lo = rne(v - hi)).  tests/test_codec_bf16_gpu.py checks them against oracle/codec_bf16_ref.py. */
int rca_codec_encode_tap_bf16(rca_codec_t* h, const float* pcm_host, int32_t B, int32_t T, int32_t layer,
                              uint16_t* hi_host, uint16_t* lo_host, int64_t numel);

/* Tests only: ONE decoder layer exactly as a decode pass launches it (run_conv with run_decoder's arguments) on a host-supplied input.
 * layer: 0 = dec.conv_in, 1..n = dec.up.{0..n-1}, n + 1 = dec.conv_out with its clamp.  x_host [B][Cin][Lin], y_host [B][Cout][Lout]
 * (Lout = Lin * stride for the transposed layers, Lin otherwise), y_numel = B * Cout * Lout.
 * route 0: the throughput launch of rca_codec_decode_dev (lat_mode off).  route 1: what rca_codec_decode_tail_dev launches under
 * lat_mode, accepted only for shapes that call can produce: variant >= 1, Lin = F * (product of the strides applied before this
 * layer) for an integer F >= 1, and B * F <= 64 (RCA_LAT_MAX_FRAMES).  Where the latency launcher declines the shape the tap falls
 * through as the decode pass does and reports the class that ran.  The handle's current variant and mfma mode apply.
 * The device output has 256 guard floats on each side; output and guards are filled with NaN before the launch, so an element the
 * kernel did not write comes back NaN, and *guards_ok is 0 when a guard changed.  The input has the same margins, filled with 1e30.
 * *kernel_class: the kernel family and tile that ran (the launch helpers record it in the handle):
 *   1      scalar chain (conv1d_chain_kernel / convtr1d_chain_kernel)
 *   2..5   f32 MFMA, wave tile (channels x columns) 32 x 32, 64 x 32, 32 x 64, 64 x 64
 *   6      warp-specialised kernel (variant 2)
 *   7      bf16 MFMA (mfma mode 1 / 3)
 *   8      f32 MFMA, any other wave tile (the fused first encoder layer; never a decoder layer)
 *   9      conv_first_mfma_kernel: the fused first encoder layer with conv_in on the matrix pipe (never a decoder layer)
 *   16+NW  LDS latency kernel with NW waves per workgroup: 17, 18 or 20
 *   +32    the launch was conv1d_mfma_mixed_kernel: whole rounds on the tile the low bits name (4 or 5), the remaining columns on
 *          finer tiles of the same grid.  Only the strided encoder layers with k >= 8 have it; never a decoder layer.
 * conv_in_kernel (the encoder's first layer alone) reports 1.
 * RCA_ERR_ARG before any HIP call for a null pointer, a layer or route out of range, B or Lin < 1, a route-1 shape as above, more
 * than 2^30 input or output elements, or a y_numel other than B * Cout * Lout. */
#define RCA_KCLASS_CHAIN 1
#define RCA_KCLASS_MFMA_32x32 2
#define RCA_KCLASS_MFMA_64x32 3
#define RCA_KCLASS_MFMA_32x64 4
#define RCA_KCLASS_MFMA_64x64 5
#define RCA_KCLASS_WS 6
#define RCA_KCLASS_BF16 7
#define RCA_KCLASS_MFMA_OTHER 8
#define RCA_KCLASS_FIRST_MFMA 9
#define RCA_KCLASS_LDS 16   /* + NW */
#define RCA_KCLASS_MIXED 32 /* ORed onto 4 or 5 */
int rca_codec_decoder_layer_tap(rca_codec_t* h, int32_t layer, int32_t route, const float* x_host, int32_t B, int32_t Lin,
                                float* y_host, int64_t y_numel, int32_t* kernel_class, int32_t* guards_ok);

/* Tests only: ONE encoder layer through the code an encode pass runs it with, on a host-supplied input.
 * layer: 0 = enc.conv_in, 1..n = enc.down.{0..n-1}, n + 1 = enc.conv_out.
 * route 0: the throughput launch of encode() and the batch entry points.  route 1: what rca_codec_encode_tail_dev launches under
 * lat_mode: variant >= 1, at most 64 (RCA_LAT_MAX_FRAMES) frames in all rows together, no flag, no view.
 * flags: 1 = x_host already holds LeakyReLU(x) and the launch must not apply it again; 2 = store LeakyReLU(y); 4 (layer 1 only) =
 * x_host is PCM and the launch is conv_in fused into the first strided layer.  view: 0, or the trailing columns per row the last
 * layer computes and stores compact.  Each is accepted only where the pass itself decides so for this shape, by the same code:
 * 1 needs the hand-off into `layer` (layer >= 2: neither conv_in nor the fusion's own conv_in stores an activated output), 2 the
 * hand-off into layer + 1, 4 the fusion predicate, a view (halo < view < Lout, layer n + 1) the kept-frames rule with
 * keep = view - halo.  RCA_CONV_BALANCE, RCA_CONV_BALANCE_PLAN, RCA_FUSE_MFMA_IN and RCA_HEAD_KEEP are read per call as in a pass;
 * the handle's variant and mfma mode apply.
 * Layer 0 and flag 4 take PCM x_host [B][Lin] for any Lin >= 1 and pad to whole frames as a pass does (L = frames * hop; on route 1
 * Lin is the kernel's Lvalid).  Other layers take x_host [B][Cin][Lin] with Lin a whole number of frames times the strides still to
 * come.  y_host [B][Cout][Lout] (Lout = L / stride), or [B][Cout][view]; y_numel is its element count.
 * Guards and fills as in rca_codec_decoder_layer_tap: 256 guard floats around the device output, NaN in output and guards before the
 * launch, 1e30 in the input margins.  *kernel_class as documented there, *post_done = 1 when the launch stored LeakyReLU(y).
 * RCA_ERR_ARG before any HIP call for a null pointer, a layer, route or flag out of range, a flag or view the pass would not use, a
 * bad shape, more than 2^30 elements or a wrong y_numel. */
int rca_codec_encoder_layer_tap(rca_codec_t* h, int32_t layer, int32_t route, int32_t flags, int32_t view, const float* x_host,
                                int32_t B, int32_t Lin, float* y_host, int64_t y_numel, int32_t* kernel_class, int32_t* post_done,
                                int32_t* guards_ok);

/* Kernel-variant switch (parity tests compare variants): 0 = scalar-chain kernels,
 * 1 = MFMA/LDS kernels (default when available). */
int rca_codec_set_variant(rca_codec_t* h, int32_t variant);

/* Per-kernel HIP-event timing for bench.py's roofline object: when enabled, every launch of a
 * profiled kernel class is bracketed by hipEventRecord on the stream it is launched on.
 * classes: 0 = implicit-GEMM conv (MFMA), 1 = codebook search, 2 = conv_in, 3 = everything else.
 * _read synchronises, returns the summed device time, the launch count and the summed ALGORITHMIC
 * FLOPs (2 per multiply-add over the real, unpadded K) and bytes since the last _read. */
int rca_codec_profile(rca_codec_t* h, int32_t enable);
int rca_codec_profile_read(rca_codec_t* h, int32_t kclass, double* total_ms, int64_t* launches, double* flops,
                           double* bytes);

/* --------------------------------------------------------------------- LM --
 * Llama-architecture decoder with a llama_cpp.Llama-like control surface
 * (SURVEY.md 8b-3): the deployed model is codec_llama.py after
 * persist_codec_embeddings (codec_llama.py:178-206), i.e. a vanilla Llama with
 * an untied lm_head.  Tensor names follow the HF state dict:
 *   model.embed_tokens.weight [V,H]; model.layers.{i}.self_attn.{q,k,v,o}_proj.weight;
 *   model.layers.{i}.mlp.{gate,up,down}_proj.weight; model.layers.{i}.input_layernorm.weight;
 *   model.layers.{i}.post_attention_layernorm.weight; model.norm.weight; lm_head.weight [V,H]
 */
typedef struct {
    int32_t vocab_size;
    int32_t hidden;
    int32_t n_layers;
    int32_t n_heads;
    int32_t n_kv_heads;
    int32_t head_dim;
    int32_t ffn;
    int32_t n_ctx;            /* KV slots allocated (llm_n_ctx, realtime_agent_resources.py:13) */
    float rms_eps;
    float rope_theta;
    int32_t rope_scaling;     /* 0 = none, 1 = llama3 */
    float rope_factor;        /* 32 */
    float rope_low_freq_factor;   /* 1 */
    float rope_high_freq_factor;  /* 4 */
    int32_t rope_orig_ctx;    /* 8192 */
    int32_t logits_all;       /* keep logits of every evaluated position (aux_llm) */
    int32_t decode_weights;   /* Every projection matrix and lm_head is kept ONCE, in the format it is streamed in by the decode step and
                                 de-quantised from by the prefill tiles.  0 = as supplied: RCA_BF16 / RCA_F16 / RCA_Q8_0 tensors keep their
                                 format (RCA_F32 is rounded to bf16); 1 = quantise to q8_0 at load the way llama-quantize writes the Q8_0 file
                                 the reference deploys (prep_test_model.sh:29; 8.5 bits per weight streamed); 2 = convert bf16 to fp16 (what
                                 convert_hf_to_gguf.py --outtype f16 writes, prep_test_model.sh:28); 3 = quantise to GGUF Q4_K blocks (4.6 bits per weight streamed;
                                 this build's own min / max rule picks the scales, the format and its de-quantisation are llama.cpp's); 4 = the same rule into GGUF
                                 Q5_K blocks (31 steps per sub-block instead of 15; 5.6 bits per weight streamed); 5 / 6 = quantise to GGUF Q4_0 /
                                 Q4_1 blocks by ggml's reference rule restated from the published algorithm (Q4_0: d = max / -8 with max the value of
                                 largest magnitude, q = min(15, (int)(x / d + 8.5)); Q4_1: d = (max - min) / 15, q = min(15, (int)((x - min) / d + 0.5));
                                 5.0 bits per weight streamed; ggml is not part of this tree: parity with llama-quantize's own bits is not pinned);
                                 7 = quantise to GGUF IQ4_NL blocks by this build's plain rule, which is NOT llama-quantize's result (that is an
                                 iterative weighted search): per 32 values max = the value of largest magnitude (the first on ties),
                                 d = fp16(max / -127), every value to the index whose d kv[i] is nearest (ties to the lower index), a block
                                 whose d is 0 to index 8 (5.0 bits per weight streamed).
                                 Tensors that arrive quantised stay as
                                 they are.  The embedding table is gathered, not streamed, and keeps full precision: f32 rows for RCA_F32 /
                                 RCA_F16 / RCA_Q8_0 / RCA_Q4_K / RCA_Q5_K / RCA_Q6_K / RCA_Q4_0 / RCA_Q4_1 / RCA_IQ4_NL / RCA_IQ4_XS sources, bf16 rows for RCA_BF16. */
} rca_lm_config_t;

typedef struct {
    int32_t top_k;   /* llama.cpp semantics (llamacpp_utils.py:39-77 passes it straight through): 1..256 = that many ranked candidates on the
                        serial chain (float sums, inverse-CDF draw); <= 0 or >= vocabulary = the whole vocabulary; 257..vocabulary - 1 = a rank
                        cut found by a radix select, then the whole-vocabulary draw (Gumbel-max).  Never clamped.  temp <= 0 is greedy.
                        Tokens rank by (value descending, index ascending) on every path: equal logits -- -0.0 and +0.0 are equal -- go to
                        the lowest index, at the rank cut, at the mass cut and in the greedy pick */
    float top_p;     /* 1.0 = off.  With top_k outside 1..256 the cut is a mass threshold over the sorted vocabulary in 2^-40 fixed point */
    float min_p;     /* 0.0 = off */
    float temp;      /* <=0: greedy */
    uint32_t seed;
    int32_t n_bias;          /* logit bias entries (llamacpp_utils.py:8-24) */
    const int32_t* bias_ids;
    const float* bias_vals;
    /* llama.cpp's penalties sampler, in front of top_k (realtime_agent_v2.py:172-185 forwards repeat_penalty / presence_penalty /
       frequency_penalty of realtime_agent_config.py:18-20): over the last `penalty_last_n` tokens this sampler accepted.
       repeat_penalty 1.0 (or 0 = unset) with 0 / 0 = off */
    float repeat_penalty;
    float freq_penalty;
    float presence_penalty;
    int32_t penalty_last_n;  /* 0 = llama-cpp-python's default window (last_n_tokens_size = 64), 1..64, < 0 = no window */
} rca_sampler_params_t;

/* llama_cpp.Llama(model_path=..., n_ctx=..., n_gpu_layers=-1) (realtime_agent_resources.py:19-33) */
int rca_lm_create(const rca_lm_config_t* cfg, const rca_tensor_t* tensors, int32_t n_tensors,
                  int32_t device, rca_lm_t** out);
/* random-init weights generated on the device from a counter hash (bench configs 3/4:
 * there are no checkpoints offline).  oracle/lm_ref.py regenerates the same values. */
int rca_lm_create_random(const rca_lm_config_t* cfg, uint64_t seed, float init_std, int32_t device,
                         rca_lm_t** out);
/* A second instance over the same weights: what the reference obtains by loading one GGUF twice (`llm` and its logits_all twin
 * `aux_llm`, realtime_agent_resources.py:19-33).  Own KV cache / workspace / sampler / stream; n_ctx may not exceed the
 * parent's.  Either handle may be destroyed first; weight-modifying calls act on both. */
int rca_lm_create_shared(rca_lm_t* parent, int32_t n_ctx, int32_t logits_all, rca_lm_t** out);
int rca_lm_destroy(rca_lm_t* h);

/* Llama.reset(): n_tokens = 0 (realtime_agent_v2.py:68) */
int rca_lm_reset(rca_lm_t* h);
/* Llama.eval(tokens): append n ids at position n_tokens, run the forward, keep the
 * last position's logits (every position's when logits_all) (llamacpp_utils.py:150) */
int rca_lm_eval(rca_lm_t* h, const int32_t* ids, int32_t n);
/* Llama.eval that returns once its LAST pass (a 128-token prefill tile, or a 1-2 token decode pass) is enqueued instead of
 * finished; any later call on the handle waits for it first.  The pieces are evaluated with the arithmetic of ONE long eval
 * (prefill tiles even for a handful of tokens), so a cache built piecewise equals the cache of a single rca_lm_eval.  Used to build the post-trim KV cache ahead of the sliding-window
 * trim (realtime_agent_v2.py:187-190,725-733) on a weight-sharing twin while the live handle keeps stepping. */
int rca_lm_eval_async(rca_lm_t* h, const int32_t* ids, int32_t n);
/* llama.cpp: one llama_decode over a llama_batch that holds prompt tokens of several sequences (llama-server -np N).
 * rca_lm_eval_async for hs[0..n_h), 1 to 64 distinct handles over one set of weights (a parent and its rca_lm_create_shared twins),
 * in shared passes of the 128-token tiles: handle k appends counts[k] >= 1 tokens, taken from `ids` concatenated in handle order, at
 * its own n_tokens.  `ws` is one more handle over the same weights and NOT among hs: the call uses its activation buffers and its
 * stream (with its priority) only -- its cache, n_tokens and logits are not touched; make it once with rca_lm_create_shared(parent,
 * a small n_ctx, 0, ...).
 *   Packing: a pass holds up to 1024 rows; a handle's tokens of a pass start on a multiple of 32 rows (the rows up to the next
 *   multiple are pad rows: nothing is stored for them), so eight handles x 128 tokens are exactly one pass.  The host cuts longer
 *   work greedily into passes; a handle's tokens may continue in the next pass.
 *   Graphs: upload, staging and the layers of a pass whose geometry (its 128-token blocks, the handles' KV format) ws has seen once
 *   before are captured and replayed; the upload of the pass's block sits inside the graph and everything per handle comes from that
 *   block, so the graph holds no handle's pointer and lives and dies with ws's other graphs.  The heads (want_logits) follow it as
 *   plain launches: which handles end in a pass is not part of its geometry.  With rca_lm_set_graphs(ws, 0) or
 *   RCA_LM_TILE_GRAPHS=0 every pass runs eagerly.
 *   Contract: the call returns once its last pass is enqueued.  Every hs[k] ends in exactly the state rca_lm_eval_async(hs[k], its
 *   ids, counts[k]) leaves: n_tokens, and the K / V rows of every layer bit for bit (fp16 and q8_0 caches); with want_logits != 0
 *   the logits of its last token, bit for bit, too.  want_logits == 0: no head runs and the handles have no logits afterwards, as
 *   after rca_lm_reset.  Rows above n_tokens and every other handle are untouched.  Any later call on ws or on an hs[k] first waits
 *   for the pass (rca_lm_sync, rca_lm_destroy and the batch calls included).
 *   Refused before anything is staged, with NO handle changed and the handle's index in the message: n_h outside 1..64, a null or
 *   repeated handle, ws among hs, other weights or another device than ws, a logits_all handle, a handle (or ws) whose
 *   rca_lm_prefill_route is not 2 (such models keep rca_lm_eval_async), mixed KV formats, a count < 1, context overflow
 *   (RCA_ERR_STATE), an id outside the vocabulary; and the whole call under RCA_LM_FLASH=0 (the split-attention prefill has no
 *   table form). */
int rca_lm_batch_eval(rca_lm_t* ws, rca_lm_t* const* hs, int32_t n_h, const int32_t* ids, const int32_t* counts, int32_t want_logits);
/* The reference recomputes the KV cache of the surviving context inside the frame that trims (realtime_agent_v2.py:725-733:
 * n_tokens = header, eval(suffix)).  Here a twin handle (rca_lm_create_shared, same n_ctx) can be given the header's KV
 * (rca_lm_copy_kv: positions [0, n_pos) of every layer, device to device), be fed the suffix over the preceding frames, and
 * trade caches with the live handle at the trim (rca_lm_swap_kv: O(1), both streams are drained first; captured step graphs
 * are kept per cache).  n_tokens is not exchanged: the caller sets it, as the reference does. */
int rca_lm_copy_kv(rca_lm_t* dst, rca_lm_t* src, int32_t n_pos);
int rca_lm_swap_kv(rca_lm_t* a, rca_lm_t* b);
/* llama.cpp's context shift (kv_cache_seq_rm(p0, p1) followed by kv_cache_seq_add(p1, -1, p0 - p1)), restated from its published
 * behaviour (ggml is not in this tree: parity with its bits is not pinned).  Needs 0 <= p0 <= p1 <= n_tokens (RCA_ERR_ARG otherwise,
 * nothing touched).  With delta = p1 - p0: in every layer the K and V rows of positions [p1, n_tokens) move to [p0, n_tokens - delta),
 * V bit for bit, every K row rotated by -delta positions -- per head and d < 32, x1 = k[d], x2 = k[d + 32] widened to f32,
 * c / s = the handle's RoPE table entries cos / sin(delta * inv_freq[d]): k'[d] = x1 c + x2 s, k'[d + 32] = x2 c - x1 s in f32,
 * stored as fp16 (nearest even).  Angles add, under llama3 frequency scaling too, so the row becomes the key of its new position up
 * to that one extra fp16 rounding -- but the K / V of layers above the first were computed while attending to the removed tokens:
 * logits after the call are those of a SHIFTED cache, not of a recompute (opt-in, never on the default path).  n_tokens becomes
 * n_tokens - delta; rows at and above it are stale, the last logits stay readable, as after rca_lm_set_n_tokens.  delta == 0 and
 * p1 == n_tokens (pure truncation) launch nothing.  Runs on the handle's stream and returns after one synchronisation; captured step /
 * frame / duplex graphs stay valid (the cache does not move and positions come from the device state).  The first call that moves
 * rows allocates a staging buffer of 2 x 2 x n_layers x 256 cache rows, freed with the handle.
 * A q8_0 handle (rca_lm_set_kv_format) refuses the call (RCA_ERR_STATE, nothing touched) unless rca_lm_set_kv_shift_requant(h, 1)
 * has allowed it; then everything above holds with the rows as blocks, under the contract stated at rca_lm_set_kv_shift_requant. */
int rca_lm_kv_remove(rca_lm_t* h, int32_t p0, int32_t p1);
/* The context shift of several handles in one pass: every hs[k] ends exactly as rca_lm_kv_remove(hs[k], p0[k], p1[k]) would leave it,
 * bit for bit -- n_tokens, the K / V rows [0, n_tokens) of every layer, the last logits still readable, captured step / frame / duplex /
 * batch graphs still valid, rows at and above the new n_tokens stale.  No byte of a handle outside hs is touched.  Pending
 * rca_lm_eval_async / rca_lm_batch_eval work of every hs[k] is settled first and the other handles' streams are drained (as
 * rca_lm_swap_kv does); the launches run on hs[0]'s stream and the call returns after ONE synchronisation.  One launch covers one slab
 * step of up to RCA_LM_KV_REMOVE_GROUP handles, each with the RoPE rows of its own delta; handles with delta == 0 or p1 == n_tokens
 * launch nothing.  A handle with delta >= 256 moves its rows cache to cache in slabs of delta rows (source and destination slabs are
 * disjoint then), without staging; the others take the single call's 256-row slabs through two staging slabs each.  That staging
 * belongs to the weight owner, is allocated by the first call with such a handle and freed with the weights, and is bounded:
 * RCA_LM_KV_REMOVE_GROUP x 2 x 2 x n_layers x 256 cache rows (134 MB at 16 layers x 8 KV heads), however many handles a call names --
 * they are processed in launch groups of RCA_LM_KV_REMOVE_GROUP.  Takes handles, not a batch: it does not need the 128-token tile route.
 * Refused before anything is enqueued, no handle changed, the message naming k: RCA_ERR_ARG for n_h outside 1..64, a null or repeated
 * handle, a handle on another device than hs[0], a handle that does not share hs[0]'s weights (the parent and its
 * rca_lm_create_shared twins do), a span with p0 < 0, p0 > p1 or p1 > n_tokens; RCA_ERR_STATE for a handle with a q8_0 KV cache that
 * rca_lm_set_kv_shift_requant has not allowed to shift; then RCA_ERR_ARG for a handle whose KV format differs from hs[0]'s (one
 * launch runs one unit body).  Over q8_0 handles with the permission the call is the same schedule over blocks: each handle ends with
 * the bits of its own rca_lm_kv_remove, and the staging buffers are the ones described above (a block row needs 68 of their 128 bytes). */
#define RCA_LM_KV_REMOVE_GROUP 8
int rca_lm_kv_remove_many(rca_lm_t* const* hs, int32_t n_h, const int32_t* p0, const int32_t* p1);
/* Tests and measurements: rca_lm_kv_remove_many with every handle on the staged route, whatever its delta.  Same contract, same bits. */
int rca_lm_kv_remove_many_staged(rca_lm_t* const* hs, int32_t n_h, const int32_t* p0, const int32_t* p1);
/* Tests only: raw fp16 rows [n_pos][n_kv_heads][64] of positions [pos0, pos0 + n_pos) (inside n_ctx) of one layer's K and V cache,
 * after draining the handle's stream.  Either pointer may be NULL. */
int rca_lm_kv_read(rca_lm_t* h, int32_t layer, int32_t pos0, int32_t n_pos, uint16_t* k_host, uint16_t* v_host);
/* Tests only: the inverse of rca_lm_kv_read: the raw fp16 rows [n_pos][n_kv_heads][64] replace positions [pos0, pos0 + n_pos) (inside
 * n_ctx) of one layer's K and V cache, after draining the handle's stream.  Either pointer may be NULL.  n_tokens is left as it was. */
int rca_lm_kv_write(rca_lm_t* h, int32_t layer, int32_t pos0, int32_t n_pos, const uint16_t* k_host, const uint16_t* v_host);
/* run the handle's stream at the device's lowest (1) / highest (0) stream priority: background prefill next to a live session */
int rca_lm_set_low_priority(rca_lm_t* h, int32_t enable);
/* read / write Llama.n_tokens: the agent rolls the KV cache back by writing it
 * (realtime_agent_v2.py:208,219,261,465,730); stale slots are overwritten by the next eval */
int rca_lm_get_n_tokens(const rca_lm_t* h, int32_t* n);
int rca_lm_set_n_tokens(rca_lm_t* h, int32_t n);
/* llm._ctx.get_logits(): V floats of the last evaluated position (realtime_agent_v2.py:449,461) */
int rca_lm_get_logits(rca_lm_t* h, float* out_host);
/* llm._scores[row] for logits_all handles: row counts back from the last eval'd position */
int rca_lm_get_logits_row(rca_lm_t* h, int32_t pos, float* out_host);
/* device pointer of the last logits (V floats); valid until the next eval */
int rca_lm_logits_dev(rca_lm_t* h, const float** out_dev);

/* init_sampler_for_generate (llamacpp_utils.py:39-77) */
int rca_lm_sampler_init(rca_lm_t* h, const rca_sampler_params_t* p);
/* The two members of llama-cpp-python's chain that rca_sampler_params_t does not carry (llamacpp_utils.py:39-77 forwards typical_p,
 * mirostat_mode, mirostat_tau, mirostat_eta).  Valid after rca_lm_sampler_init, which resets both to off; each settles the stream,
 * and a change of the sampler's launches drops the captured graphs.  Restated from the published definitions: tests/samp_ext_ref.py is
 * the definition, parity with llama.cpp is not pinned ("typical_p and mirostat v2").
 * rca_lm_sampler_set_typical: llama.cpp's locally typical cut between top_k and top_p on the serial chain (temp > 0, top_k 1..256):
 *   over the top_k candidates, keep the shortest prefix in order of |-ln p - H| (ties to the better rank) whose mass exceeds
 *   typical_p, at least one token; the survivors go on to top_p / min_p / temp as a fresh candidate list.  typical_p >= 1 or 0 = off;
 *   temp <= 0 (greedy) and mirostat v2 ignore it.  RCA_ERR_ARG, naming the value: negative or NaN; typical_p < 1 with temp > 0 and
 *   top_k outside 1..256 (the whole vocabulary is not sorted by typicality).
 * rca_lm_sampler_set_mirostat: mode 0 = off, 2 = mirostat v2 -- the chain is then logit bias -> penalties -> temp -> mirostat, and
 *   top_k, top_p, min_p and typical_p are IGNORED, as llama-cpp-python leaves them out.  Per draw: the whole vocabulary cut at a
 *   surprise (-log2 p) of mu, the top token always kept; the draw by the Gumbel-max rule of the whole-vocabulary sampler with the same
 *   keyed RNG; mu <- mu - eta (observed surprise - tau).  Sums over the vocabulary are 2^-40 fixed point.  mu = 2 tau after this call.
 *   mu is a function of the draw counter: whatever rewinds the counter (a cut rca_lm_frame, a cut batch frame) rewinds mu.
 *   temp <= 0 stays greedy.  RCA_ERR_ARG: mode 1 (v1 is not built), any other mode, tau or eta negative, NaN or infinite.
 * rca_lm_sampler_get_mirostat_mu: settles the stream; the mu the next draw will read.  RCA_ERR_STATE when mirostat is off. */
int rca_lm_sampler_set_typical(rca_lm_t* h, float typical_p);
int rca_lm_sampler_set_mirostat(rca_lm_t* h, int32_t mode, float tau, float eta);
int rca_lm_sampler_get_mirostat_mu(rca_lm_t* h, float* mu);
/* sample() (llamacpp_utils.py:79-95): draw from the last logits */
int rca_lm_sample(rca_lm_t* h, int32_t* token);
/* next(generate(tokens, reset=False)) (llamacpp_utils.py:145-161; realtime_agent_v2.py:355):
 * eval + sample with no host round trip in between; hipGraph-replayed for n<=2 */
int rca_lm_step(rca_lm_t* h, const int32_t* ids, int32_t n, int32_t* token);
/* Group step: several sessions over ONE set of weights advance together, every weight matrix streamed once for all of them.  The
 * reference's self-play runs two agents on one card by loading the GGUF twice and stepping each model on its own
 * (inference_client_self_play.py:148-159: two weight streams per frame); llama.cpp knows the capability as parallel sequences
 * (n_seq_max, llama-server -np: several sequences in one llama_decode).
 * rca_lm_group_create: a group over 2 to 4 existing handles.  RCA_ERR_ARG, with a message naming the member, when two members are
 *   the same handle, a member is on another device than member 0, does not share member 0's weights (the parent and its
 *   rca_lm_create_shared twins do), has another activation format (rca_lm_set_act_format), or is a logits_all handle.  Every weight format
 *   and both activation formats of the single step have their four-row GEMV instances.  The group holds no state of its members beyond pointers: the members live
 *   on, and the group is destroyed BEFORE any of them.
 * rca_lm_group_step: ids [n_members][n], tokens [n_members].  Member s evaluates ids[s * n .. s * n + n) at ITS n_tokens and samples
 *   with ITS sampler; n_members * n is 2 or 4 (2 x 1, 2 x 2 -- the duplex pair step of two sessions -- or 4 x 1).  Afterwards every
 *   member is in exactly the state rca_lm_step(member, its ids, n, &tokens[s]) would have left, bit for bit: n_tokens += n, its KV
 *   rows written, its last logits where rca_lm_get_logits / rca_lm_token_probs / rca_lm_sample / rca_lm_logits_dev find them, its
 *   draw counter, penalty window and sampled token advanced.  Single-handle calls and group steps may be interleaved freely.
 *   Pending rca_lm_eval_async work of a member is waited for first.  Refused before anything is enqueued, with NO member changed:
 *   another row count (RCA_ERR_ARG), an id outside the vocabulary (RCA_ERR_ARG), a member without a sampler, a member switched to
 *   logits_all or to another activation format since the group was made, and a context overflow of ANY member (all RCA_ERR_STATE).
 *   The pass runs on member 0's stream, in member 0's activation workspace, and ends with one synchronisation and one download of
 *   the tokens; with graphs enabled on every member it is one replay, captured per (n, largest context bucket among the members)
 *   and re-captured when a member's captured state changes (rca_lm_swap_kv, a sampler of another kind, rca_lm_set_act_format, ...);
 *   rca_lm_set_graphs(member, 0) on any member makes it eager. */
typedef struct rca_lm_group rca_lm_group_t;
int rca_lm_group_create(rca_lm_t* const* members, int32_t n_members, rca_lm_group_t** out);
int rca_lm_group_destroy(rca_lm_group_t* g);
int rca_lm_group_step(rca_lm_group_t* g, const int32_t* ids, int32_t n, int32_t* tokens);
/* Batch step: 2 to 64 sessions over ONE set of weights advance together as one token block of the 128-token MFMA tiles (llama.cpp:
 * -np N with N above 4).  Where the group step runs the decode GEMVs over 2 or 4 rows, the batch step runs every projection as one
 * tile GEMM over all n_members * n rows, the decode attention of every member in one launch (+ one merge) per layer, the head as
 * one tile GEMM over one row per member and the top-k sampler chain (top_k 1..256) once for all members.
 * rca_lm_batch_create: a batch over 2 to 64 existing handles.  RCA_ERR_ARG, with a message naming the member, for the refusals of
 *   rca_lm_group_create (a null or duplicate member, another device, other weights, a logits_all member) and for a member whose
 *   long evals do not take the 128-token tiles (rca_lm_prefill_route != 2): such models stay with the group step.  Members MAY
 *   differ in activation format: the tiles always run f32 activations split into bf16 hi + lo, exactly as rca_lm_eval_async and
 *   rca_lm_score do, so rca_lm_set_act_format does not apply to a batch step.  The batch holds pointers to its members only and is
 *   destroyed BEFORE any of them.
 * rca_lm_batch_step: ids [n_members][n], tokens [n_members]; n is 1 or 2 and n_members * n <= 128.  Member s evaluates
 *   ids[s * n .. s * n + n) at ITS n_tokens and samples with ITS sampler.  Afterwards every member has n_tokens += n, its K / V rows
 *   written in its own cache, its last row's logits where rca_lm_get_logits / rca_lm_token_probs / rca_lm_sample /
 *   rca_lm_logits_dev find them, its draw counter and penalty window advanced and its sampled token in tokens[s].
 *   Contract (NOT the group step's bit-for-bit promise against rca_lm_step: the tiles round differently from the GEMVs):
 *     - the arithmetic class is that of a decode step on a tile-built cache: tile GEMMs + the split decode attention;
 *     - a K / V row is, bit for bit, the row rca_lm_eval_async writes for the same token at the same position over the same
 *       earlier rows;
 *     - a member's logits and K / V rows do not depend on its slot, on the other members, or on graphs being on or off;
 *     - the token is the one rca_lm_sample would draw from the member's logits at its draw counter.
 *   Pending rca_lm_eval_async work of a member is waited for first.  Refused before anything is staged, with NO member changed: n
 *   outside 1..2, more than 128 rows, an id outside the vocabulary (RCA_ERR_ARG); a member without a sampler, a member switched to
 *   logits_all or off the tile route since the batch was made, a context overflow of ANY member (RCA_ERR_STATE).  Messages name
 *   the member.  The pass runs on member 0's stream, in member 0's activation workspace: one upload, one synchronisation, one
 *   download.  With graphs enabled on every member it is one replay, captured per (n, largest context bucket among the members) as
 *   one linear launch sequence and re-captured when a member's captured state changes; rca_lm_set_graphs(member, 0) on any member
 *   makes it eager.  Single-handle calls, group steps and batch steps may be interleaved freely on the same handles. */
typedef struct rca_lm_batch rca_lm_batch_t;
int rca_lm_batch_create(rca_lm_t* const* members, int32_t n_members, rca_lm_batch_t** out);
int rca_lm_batch_destroy(rca_lm_batch_t* b);
int rca_lm_batch_step(rca_lm_batch_t* b, const int32_t* ids, int32_t n, int32_t* tokens);
/* Batch frame: rca_lm_frame (below) for every member of a batch in ONE call -- the unit of work of N duplex sessions on a card.
 * first_pairs [n_members][2], user_ids [n_members][n_steps], probe_ids [n_members] or NULL (-1: no probe for that member),
 * out_tokens [n_members][n_steps], n_done [n_members], probe_probs [n_members] or NULL.  n_steps is 1..8, n_members * 2 <= 128.
 *   Step i of member s evaluates its current pair -- first_pairs[s] for i = 0, then [token it sampled at step i - 1,
 *   user_ids[s][i - 1]] -- at ITS position through the batch pass of rca_lm_batch_step and samples with ITS sampler; the feedback
 *   happens on the device.  The whole frame is one linear launch sequence on member 0's stream: one upload, one synchronisation,
 *   one download.  With graphs enabled on every member it is one replay, captured per (n_steps, largest context bucket among the
 *   members at the frame's END, probes on / off) and re-captured under the rule of the batch step's graphs; with graphs off on any
 *   member it is eager.  Every step is a batch step's launches with a batch step's arguments, so member s ends the frame, bit for
 *   bit, as n_done[s] rca_lm_batch_step calls of n = 2 with the tokens fed back by the caller would have left it.
 *   Every member runs all n_steps steps; what stands is settled per member, with rca_lm_frame's semantics:
 *     - n_done[s] = n_steps, or j + 1 for the first step j whose token is <= audio_id_floor; out_tokens[s][i] = -1 for i >= n_done[s];
 *     - the member ends with n_tokens += 2 * n_done[s] and its draw counter at + n_done[s], on the host mirror and on the device
 *       (one small launch over the cut members); the cache slots and penalty-window entries of the discarded steps are stale and get
 *       overwritten, exactly as after a cut rca_lm_frame;
 *     - a member with n_done[s] < n_steps has NO logits: get_logits / sample / token_probs fail with "no logits" until its next
 *       eval or step; a complete member has its last step's logits in its own buffer.
 *   With probe_ids, probe_probs[s] = softmax(last logits of member s)[probe_ids[s]], computed inside the same replay with
 *   rca_lm_token_probs' arithmetic; -1 where the member was cut or its probe id is -1.
 *   Refused before anything is staged, with NO member changed: what rca_lm_batch_step refuses, n_steps outside 1..8, an id of a first
 *   pair, a user id or a probe id outside the vocabulary, probe_probs NULL while probe_ids is not (RCA_ERR_ARG); a context overflow
 *   of ANY member counted with 2 * n_steps (RCA_ERR_STATE).  Messages name the member.  Single-handle calls, group steps, batch
 *   steps and batch frames may be interleaved freely on the same handles. */
int rca_lm_batch_frame(rca_lm_batch_t* b, const int32_t* first_pairs, const int32_t* user_ids, int32_t n_steps, int32_t audio_id_floor,
                       const int32_t* probe_ids, int32_t* out_tokens, int32_t* n_done, float* probe_probs);
/* Selection frame: rca_lm_batch_frame over a SUBSET of the members -- a session sits a tick out while its codec windows fill, on a
 * forced transcription or response, when a trim falls between two steps, after it left audio mode, or when its chunk has not arrived.
 * sel [n_sel]: distinct member indices of the batch in any order, n_sel in 1..n_members.  Every per-member array is indexed by k, the
 * position in sel, NOT by member: first_pairs [n_sel][2], user_ids [n_sel][n_steps], probe_ids [n_sel] or NULL, out_tokens
 * [n_sel][n_steps], n_done [n_sel], probe_probs [n_sel] or NULL.  Per selected member the semantics are rca_lm_batch_frame's: cut,
 * roll-back, probes, "no logits" after a cut.
 *   Contract, bit for bit: a selected member ends as rca_lm_batch_frame on a batch created over ONLY the selected members would leave
 *   it (a member does not depend on slot or companions).  An unselected member is not touched at all: no byte of its K / V cache (rows
 *   at and past its n_tokens included), not its n_tokens, logits buffer or logits_rows, not its draw counter, penalty window or device
 *   state; pending rca_lm_eval_async work of an unselected member is not waited for.  An unselected member with a full cache or
 *   without a sampler is no reason to refuse.  (The pass runs on member 0's stream in member 0's activation workspace, selected or not.)
 *   Refused before anything is staged, with NO member changed, in a message that names k and the member: n_sel outside 1..n_members,
 *   an index outside the batch, an index selected twice (RCA_ERR_ARG), and everything rca_lm_batch_frame refuses, checked on the
 *   selected members only.
 *   The selected members are compacted into slots 0 .. n_sel - 1 of device tables composed on the host for this call and uploaded with
 *   the frame's block inside the replay; the launches cover the selection's geometry class -- n_sel rounded up to 8, 16, 32 or 64
 *   slots -- and every kernel leaves at once for a slot past the live count, which travels in the uploaded block.  A graph therefore
 *   holds no member's pointer: it is captured per (class, n_steps, largest context bucket among the SELECTED members at the frame's
 *   end, probes on / off, a logit-patching sampler among the selected) and serves every selection of its class, also after a member's
 *   rca_lm_swap_kv.  It is re-captured when a member's own graphs are dropped (a sampler of another kind, rca_lm_set_act_format, ...).
 *   A selection that holds a member on a whole-vocabulary sampler (top_k 0 or above 256: its own launches with its own pointers), or a
 *   member with graphs off, runs the same launches eagerly: same results. */
int rca_lm_batch_frame_sel(rca_lm_batch_t* b, const int32_t* sel, int32_t n_sel, const int32_t* first_pairs, const int32_t* user_ids,
                           int32_t n_steps, int32_t audio_id_floor, const int32_t* probe_ids, int32_t* out_tokens, int32_t* n_done,
                           float* probe_probs);
/* Selection step: rca_lm_step_probe for a SUBSET of the members in one pass -- the agents' speculative <|end_audio|> step for the
 * sessions of a tick that owe it, or a server's step of the sessions that are in a text branch.  sel [n_sel] as for the selection
 * frame; every per-member array is indexed by k, the position in sel: ids [n_sel][n] with n 1 or 2, probe_ids [n_sel][n_probe] with
 * n_probe 0..8 (NULL exactly when n_probe is 0), tokens [n_sel], probs [n_sel][n_probe] (may be NULL when n_probe is 0).  Member
 * sel[k] evaluates ids[k * n .. k * n + n) at ITS n_tokens, samples with ITS sampler (draw counter + 1, the token joins its penalty
 * window) and probs[k][i] = softmax(logits of the evaluated position)[probe_ids[k][i]].
 *   Contract, bit for bit: a selected member ends as rca_lm_batch_step(n) on a batch created over ONLY the selected members would
 *   leave it -- token, logits, K / V rows, n_tokens, draw counter, penalty window -- and its probabilities are the bytes
 *   rca_lm_token_probs returns on it right after that step.  An unselected member is in no table of the call: nothing reads or writes
 *   it, it is neither settled nor checked, and its full cache or missing sampler refuses nothing.  The caller that only wanted the
 *   probabilities rolls back with rca_lm_set_n_tokens(n_tokens - n): the next evaluation overwrites the speculative rows.
 *   Refused before anything is staged, with NO member changed, in a message that names k and the member: a null argument, n outside
 *   1..2, n_probe outside 0..8, probe_ids or probs NULL while n_probe > 0, n_sel outside 1..n_members, an index outside the batch or
 *   selected twice, a token or probe id outside the vocabulary (RCA_ERR_ARG); a selected member without a sampler, switched to
 *   logits_all, off the 128-token tile route, in another KV format than member 0, or with n_tokens + n > n_ctx (RCA_ERR_STATE).
 *   The launches are the selection frame's machinery with n tokens per member: tables of slots 0 .. n_sel - 1, the ids and the probe
 *   ids uploaded as one block inside the replay, the class's launch geometry, one linear sequence on member 0's stream, tokens and
 *   probabilities gathered for one download.  A graph is captured per (class, n, largest context bucket among the SELECTED members
 *   after the step, probes present or not, a logit-patching sampler among the selected); n_probe and the ids come from the block, so
 *   one graph serves every selection of its class, also after a member's rca_lm_swap_kv, and is dropped with the selection frame's
 *   graphs.  A selection that holds a member on a whole-vocabulary sampler, or a member with graphs off, runs the same launches
 *   eagerly: same results. */
int rca_lm_batch_step_sel(rca_lm_batch_t* b, const int32_t* sel, int32_t n_sel, const int32_t* ids, int32_t n, const int32_t* probe_ids,
                          int32_t n_probe, int32_t* tokens, float* probs);
/* graph captures made by this batch so far (batch steps, batch frames, selection frames and selection steps) */
int rca_lm_batch_captures(const rca_lm_batch_t* b, int64_t* n);
/* One whole frame of process_audio_input_ids (realtime_agent_v2.py:332-372) as ONE hipGraph: n_steps (<= 8) S=2 steps, the
 * agent token sampled by step i fed back on the device together with user_ids[i] as step i+1's input pair; first_pair is the
 * pair step 0 evaluates (the last two ids of the sequence).  out_tokens[i] = token sampled by step i.  *n_done = number of steps
 * whose result stands: n_steps, or j + 1 when step j sampled a token <= audio_id_floor (the loop leaves audio mode there,
 * realtime_agent_v2.py:361-371); the KV position and the sampler's draw counter are then exactly what j + 1 single steps would
 * have left, and the caller continues step by step.  After a complete frame the logits are those of its last step; after a frame
 * cut short (n_done < n_steps) NO logits are available (the buffer holds a rolled-back step's): get_logits / token_probs / sample
 * fail with "no logits" until the next eval or step. */
int rca_lm_frame(rca_lm_t* h, const int32_t* first_pair, const int32_t* user_ids, int32_t n_steps, int32_t audio_id_floor,
                 int32_t* out_tokens, int32_t* n_done);
/* ONE duplex frame-step as ONE graph replay (north_star: "the per-frame encode -> LM-step -> decode loop is hipGraph-captured";
 * the loop is RealtimeAgent.process_audio, realtime_agent_v2.py:504-554): encode tail of the user's rolling PCM window
 * (audio_tokenizer.py:67-103) -> code -> token id (code_token_base + code: the codec tokens sit in the vocabulary in code order,
 * train_vanilla_latest.py:587-589) -> the chunk's n_steps LM steps exactly as rca_lm_frame runs them (process_audio_input_ids,
 * :332-372) -> token id -> code appended to the detokenizer's rolling code context (audio_tokenizer.py:113) -> decode tail
 * (:141-145) -> softmax(last logits)[probe_id] (measure_event_prob, :448-452).  One upload, one replay, one synchronisation.
 * The host owns both rolling windows and passes them whole; nothing rolls on the device, so a frame that takes the separate
 * calls instead (warm-up shapes, forced transcription / response, a trim between two steps) needs no repair.
 * The first frame of a shape runs the same launches eagerly (it sizes the codec workspace); the second captures. */
typedef struct rca_duplex_frame_args {
    const float* pcm_window;    /* host [T]: mono PCM window INCLUDING this frame's chunk */
    const int64_t* code_ctx;    /* host [F_ctx]: the code context BEFORE this frame's codes (may be NULL when F_ctx = 0) */
    int32_t T;
    int32_t F_ctx;
    int32_t n_steps;            /* codes per frame == LM steps (1..8) */
    int32_t n_samples;          /* PCM samples wanted from the end of decode(code_ctx + this frame's codes) */
    int32_t code_token_base;    /* token id of code 0 */
    int32_t audio_id_floor;     /* a sampled token <= this leaves audio mode (<|end_header|>) */
    int32_t probe_id;           /* token whose probability under the last step's logits is wanted, or -1 */
    int32_t first_pair[2];      /* [agent, user] pair of the previous frame (the first step's input) */
} rca_duplex_frame_args_t;
typedef struct rca_duplex_frame_out {
    int64_t user_codes[8];      /* the n_steps codes of the user's chunk (always valid) */
    int32_t tokens[8];          /* sampled agent tokens; entries >= n_done are -1 */
    int32_t n_done;             /* as rca_lm_frame: < n_steps when step n_done - 1 left audio mode (KV position / draws put back) */
    int32_t flags;              /* 0: pcm_out_host holds the decode tail.  bit 0: a sampled token is no codec token, bit 1: frame
                                   cut short -- in both cases pcm_out_host is untouched and the caller decodes on its own path */
    float probe_prob;           /* -1 when not asked for or the frame was cut short */
} rca_duplex_frame_out_t;
int rca_duplex_frame(rca_lm_t* lm, rca_codec_t* codec, const rca_duplex_frame_args_t* args, rca_duplex_frame_out_t* out,
                     float* pcm_out_host);
/* Duplex batch frame: rca_duplex_frame for every selected member of a batch in ONE call -- encode tails -> ids -> the selection frame
 * (rca_lm_batch_frame_sel) -> codes -> decode tails -> probes for N sessions.  All members of one call share one call shape, the
 * steady-state shape AudioTokenizer.duplex_plan produces.  One upload, ONE linear launch sequence on member 0's stream (no side-stream
 * fork: at these sizes the encode tails are a fraction of a batch pass, and a captured graph without parallel branches is the plainer
 * shape), one download, one synchronisation.  The user's ids of the frame's block are written on the device by the table form of the
 * codes -> ids kernel; the sampled tokens go behind each row's context codes through the table form of the ids -> codes kernel, which
 * raises a flag per member.  The codec tails run over the row count of the selection's geometry class (8, 16, 32 or 64): the rows past
 * the selection hold code 0 and stale finite PCM and their results are not read, which keeps one codec shape per class.
 * Per member k, bit for bit what rca_duplex_frame gives one handle: user_codes = the encode tail of that window alone (B = 1); tokens,
 * n_done, the member's state and probe_prob = rca_lm_batch_frame_sel with code_token_base + code as user ids (so the batch's
 * arithmetic class: a session inside a batch samples other tokens than the same session alone); flags bit 0 when a sampled token is no
 * codec token (its code is 0 for the decode), bit 1 when the member was cut; the PCM row pcm_out_host + k * n_samples = the decode tail of
 * (code_ctx[k] + the new codes) alone, copied only when flags[k] == 0 -- otherwise the row is untouched and the caller decodes on its own path.
 * The first call of a (class, shape) runs eagerly and sizes the codec workspace; later calls replay a graph keyed by class, shape, base,
 * probes on / off, context bucket, rca_codec_workspace_sig and the codec (a selection with a whole-vocabulary sampler or graphs off
 * stays eager).  Refused before anything is staged, with NO member changed: what rca_lm_batch_frame_sel refuses, a bad shape, n_steps
 * codes not inside the window, n_samples > (F_ctx + n_steps) * hop, a base that puts codes outside the vocabulary, a context code outside
 * the codebook.  Buffers, pinned staging and graphs belong to the batch: rca_lm_batch_destroy frees them. */
typedef struct rca_duplex_batch_args {
    const int32_t* sel;         /* members taking part this tick */
    int32_t n_sel;
    const float* pcm_windows;   /* host [n_sel][T] */
    const int64_t* code_ctx;    /* host [n_sel][F_ctx], NULL when F_ctx = 0 */
    const int32_t* first_pairs; /* [n_sel][2] */
    const int32_t* probe_ids;   /* [n_sel] (-1: none) or NULL */
    int32_t T, F_ctx, n_steps, n_samples, code_token_base, audio_id_floor;
} rca_duplex_batch_args_t;
typedef struct rca_duplex_batch_out {   /* caller-allocated arrays, indexed by k */
    int64_t* user_codes;        /* [n_sel][8] */
    int32_t* tokens;            /* [n_sel][8], -1 from n_done on */
    int32_t* n_done;            /* [n_sel] */
    int32_t* flags;             /* [n_sel], rca_duplex_frame's bits */
    float* probe_prob;          /* [n_sel], -1 as rca_duplex_frame */
} rca_duplex_batch_out_t;
int rca_duplex_batch_frame(rca_lm_batch_t* b, rca_codec_t* codec, const rca_duplex_batch_args_t* a, rca_duplex_batch_out_t* out,
                           float* pcm_out_host /* [n_sel][n_samples] */);
/* Optional: make rca_duplex_frame's one-time allocations for a call shape (pinned staging, device buffers, side stream) ahead of the
 * first frame -- a session calls it at reset() (realtime_agent_v2.py:127-161) so that no frame pays for a pinned allocation. */
int rca_duplex_prepare(rca_lm_t* lm, int32_t T, int32_t F_ctx, int32_t n_steps, int32_t n_samples);
/* Optional, after rca_duplex_prepare and rca_lm_sampler_init: capture every graph the session's frames can replay BEFORE the first
 * frame -- the one-replay frame of the call shape in `args` (T, F_ctx, n_steps, n_samples, code_token_base, probe_id >= 0 or not; the
 * data pointers and first_pair are not read) for every context bucket n_ctx reaches, on the KV cache of `lm` and, when the session
 * trims through a shadow cache, on `twin`'s too (may be NULL), and with n_probe > 0 the speculative one-token step + n_probe
 * probabilities (rca_lm_step_probe; realtime_agent_v2.py:455-466).  A session calls it at reset() (realtime_agent_v2.py:127-161): no
 * frame then pays a graph capture. */
int rca_duplex_precapture(rca_lm_t* lm, rca_lm_t* twin, rca_codec_t* codec, const rca_duplex_frame_args_t* args, int32_t n_probe);
/* what rca_duplex_frame needs from a codec handle whose tail calls it captures: a signature of every address a captured tail
 * call bakes in, a hand-over of the handle's stream ordering to the capturing stream, the codebook size */
int rca_codec_workspace_sig(rca_codec_t* h, uint64_t* sig);
int rca_codec_stream_handoff(rca_codec_t* h, void* stream);
int rca_codec_codebook_size(const rca_codec_t* h, int32_t* n);
/* rca_lm_step + rca_lm_token_probs of the position it evaluated, as ONE replay and one synchronisation: the agent's speculative
 * <|end_audio|> step (get_probable_event_speaker, realtime_agent_v2.py:455-466: eval, sample, softmax(logits)[agent speaker, user
 * speaker], then n_tokens -= 1).  Same token and the same probabilities as the two separate calls. */
int rca_lm_step_probe(rca_lm_t* h, const int32_t* ids, int32_t n, const int32_t* probe_ids, int32_t n_probe, int32_t* token, float* probs_out);
/* softmax(logits)[token] of the last position, reduced on the device
 * (measure_event_prob, realtime_agent_v2.py:448-452) */
int rca_lm_token_probs(rca_lm_t* h, const int32_t* token_ids, int32_t n, float* probs_out);
/* zero lm_head rows [row_begin, row_end) (random-init bench models: keeps the sampler on codec tokens,
 * as a trained model in audio mode does; the bytes streamed per step are unchanged) */
int rca_lm_mask_head_rows(rca_lm_t* h, int32_t row_begin, int32_t row_end);
/* The reference's deployment step CodecLlamaForCausalLM.persist_codec_embeddings (codec_llama.py:178-206) for a checkpoint
 * that still carries the frozen codec embedding and its projector (codec_llama.py:32-69): table row
 * codec_vocab_start + i  <-  linear_2(gelu(linear_1(codec_embed[i]))), fp32 arithmetic, stored as bf16 (nearest even).
 * Host pointers: codec_embed [n_codes, dim], w1 [hidden, dim], b1 [hidden], w2 [hidden, hidden], b2 [hidden];
 * out_f32 (optional, [n_codes, hidden]) receives the rows before the 16-bit rounding.  One call per codebook. */
int rca_lm_persist_codec_embeddings(rca_lm_t* h, const float* codec_embed, int32_t n_codes, int32_t dim,
                                    const float* w1, const float* b1, const float* w2, const float* b2,
                                    int32_t codec_vocab_start, float* out_f32);
/* llama_cpp's logits_all after creation: 1 = keep the logits of every evaluated position (rca_lm_get_logits_row), 0 = last
 * position only.  get_logprobs (llamacpp_utils.py:30-37) evaluates its long context with 0 and the scored tokens with 1. */
int rca_lm_set_logits_all(rca_lm_t* h, int32_t enable);
/* enable / disable hipGraph replay of the steady-state step (eager launches otherwise); tests and
 * bench compare the two */
int rca_lm_set_graphs(rca_lm_t* h, int32_t enable);
/* evals longer than 8 tokens (session prefill llamacpp_utils.py:145-161 via realtime_agent_v2.py:100, KV recompute
 * :725-733) run as 128-token tiles on bf16 MFMA with hi/lo-split activations (default; logits within ~1e-3 of the
 * decode path); 0 routes them through the 8-token GEMV chunks, which are bit-identical to decode */
int rca_lm_set_mfma_prefill(rca_lm_t* h, int32_t enable);
/* Tests only: the route rca_lm_eval takes for an eval of more than LM_PREFILL_MIN tokens with the
 * current settings: 0 = 8-token GEMV chunks, 1 = 32-token tiles, 2 = 128-token tiles. */
int rca_lm_prefill_route(const rca_lm_t* h, int32_t* route);
/* the format the projection matrices are kept and streamed in (0 bf16, 1 q8_0, 2 f16, 3 q4_k, 5 q5_k, 6 q4_0, 7 q4_1, 8 iq4_nl, 9 iq4_xs) and, optionally, the weight bytes one decode
 * step reads (llama.cpp prints the same two facts at load: file type and model size) */
int rca_lm_weight_format(const rca_lm_t* h, int32_t* fmt, int64_t* bytes_per_step);
/* decode steps merge the attention splits inside the attention launch (1, default: the workgroup that publishes its partial last
 * merges them; bit-identical to the separate merge launch) or in a launch of its own (0); tests compare the two */
int rca_lm_set_attn_fuse(rca_lm_t* h, int32_t enable);
/* activation format of the decode GEMVs over quantised matrices: 0 = f32 (default), 1 = q8_1 blocks + integer dot products
 * (llama.cpp's GPU mat-vec class).  RCA_ERR_ARG for another value or when no projection matrix of the handle is q8_0 / Q4_K / Q5_K / Q6_K / Q4_0 / Q4_1 / IQ4_NL / IQ4_XS.
 * Drops captured graphs when the value changes.  Per handle; rca_lm_create_shared copies the parent's value.
 * q8_1: a row of K activations is cut into blocks of 32 consecutive values; per block d = amax / 127, inv = d != 0 ? 1 / d : 0 (IEEE
 * division), q_j = roundf(x_j * inv) (ties away from zero) as int8, scale used d_x = (float)(fp16 rne of d); an all-zero block is
 * q = 0, d = 0.  This is ggml's quantize_row_q8_1 restated from the published algorithm (ggml is not part of this tree: parity with
 * llama.cpp's own bits is not pinned).  Per block a weight row contributes
 *   q8_0: (d_w d_x) sum q_w q_x      Q6_K: d_x (s_w0 sum_first16 q_w q_x + s_w1 sum_second16 q_w q_x)
 *   Q4_K: d_x ((d sc_b) sum q_w q_x - (dmin m_b) sum q_x)           Q5_K: the same with the 5-bit q_w
 *   Q4_0 / Q4_1: d_x (s sum q_w q_x - t sum q_x) with (s, t) = (d, 8 d) / (d, -m) as formed at load
 *   IQ4_NL / IQ4_XS: (s d_x) sum kv[q_w] q_x with s = d / d (ls - 32) as formed at load (|sum| <= 8 * 127 * 127 per chunk)
 * with exact integer sums (v_dot4c_i32_i8 over a lane's 8 values); scaling and the sums across chunks, lanes and waves are f32 in
 * the order of the f32 path.  Matrices kept in bf16 / f16 and the MFMA prefill tiles keep f32 activations; the exact prefill
 * route (rca_lm_set_mfma_prefill(0), evals of up to 8 tokens) is made of decode GEMV passes and follows the mode. */
int rca_lm_set_act_format(rca_lm_t* h, int32_t fmt);
int rca_lm_get_act_format(const rca_lm_t* h, int32_t* fmt);
/* Format of the handle's KV cache: 0 = fp16 (default; bit for bit the cache of earlier versions), 1 = q8_0 (llama.cpp's
 * --cache-type-k q8_0 --cache-type-v q8_0).  RCA_ERR_ARG for another value, RCA_ERR_STATE unless n_tokens == 0 (nothing is touched).
 * When the value changes the cache is re-allocated, zeroed, and every captured graph is dropped.  Per handle; rca_lm_create_shared
 * copies the parent's value, so shadow and aux twins follow.  rca_lm_config_t is not extended.
 * FORMAT.  Per layer, position and kv head the 64 values of K and of V are two ggml q8_0 blocks (32 int8 + one fp16 scale each),
 * kept in separate planes per tensor: q[n_layers][n_ctx_pad][n_kv_heads][64] int8 and d[n_layers][n_ctx_pad][n_kv_heads][2] fp16 --
 * a head row is 64 contiguous, 64-byte-aligned bytes.  A cached position takes n_layers * n_kv_heads * 2 * 68 bytes instead of
 * n_layers * n_kv_heads * 2 * 128 (rca_lm_kv_bytes_per_position).
 * RULE.  The quantiser's input is the fp16 row the default cache would hold: cache row == Q8(fp16 row of the default path).  It is the
 * q8_1 rule of rca_lm_set_act_format: per block d = amax / 127 (IEEE f32 division), inv = d != 0 ? 1 / d : 0, q_j = roundf(x_j * inv)
 * (ties away from zero) as int8, stored scale d16 = fp16 rne of d; an all-zero block is q = 0, d16 = 0, and a block whose d rounds to
 * fp16 zero de-quantises to zeros, and a block whose amax is 65504 de-quantises its extreme element to infinity (d16 rounds up to 516;
 * 516 * 127 is beyond fp16) -- the rule, not an error.  Attention multiplies fp16_rne((float)d16 * q_j), formed while a row is
 * staged into the LDS images of the attention kernels; everything behind the images (MFMA, softmax, merge, combine) is the code of
 * the fp16 cache.  The QKV epilogues store their fp16 rows into a per-handle ring of 1024 positions (row = position & 1023, one ring
 * for all layers, about 2 MB at 8 kv heads) and one small launch per layer quantises the rows of the pass before attention runs.
 * Every eval / step / frame / score / duplex / group / batch call works on a q8_0 handle.  rca_lm_copy_kv / rca_lm_swap_kv between
 * handles of different formats, and groups or batches whose members differ in format, are refused.  rca_lm_kv_remove on a q8_0 handle
 * is refused (RCA_ERR_STATE, n_tokens unchanged): re-rotating quantised keys would quantise them a second time -- unless that has been
 * asked for by name (rca_lm_set_kv_shift_requant below).  rca_lm_set_kv_format(h, 0) clears that permission.
 * Tests-only calls on a q8_0 handle: rca_lm_kv_write quantises the given fp16 rows with the kernel the passes use; rca_lm_kv_read and
 * rca_lm_gemv_tap's kv_host return the de-quantised fp16 rows, exactly the values attention stages; rca_lm_kv_read_q8 the raw blocks. */
int rca_lm_set_kv_format(rca_lm_t* h, int32_t fmt);
int rca_lm_get_kv_format(const rca_lm_t* h, int32_t* fmt);
/* Opt-in: the context shift (rca_lm_kv_remove, rca_lm_kv_remove_many, rca_lm_kv_remove_many_staged) on a q8_0 KV cache, what llama.cpp's
 * K-shift does on a quantised cache: de-quantise, rotate, re-quantise.  on = 1 allows it, 0 (default) keeps the refusal.  A permission
 * only: allowed at any n_tokens, no cache is touched, no graph is dropped.  RCA_ERR_ARG for another value, RCA_ERR_STATE on an fp16
 * handle.  rca_lm_create_shared copies the parent's value; rca_lm_set_kv_format(h, 0) clears it.
 * CONTRACT of a shifted q8_0 cache (positions, n_tokens, stale rows, logits, graphs, the one synchronisation: as rca_lm_kv_remove):
 *   V rows: the two blocks of every moved head row (64 int8 + 2 fp16 scales) are copied bit for bit.
 *   K rows: x = fp16_rne((float)d16 * q) is the de-quantised row, the one attention stages.  The new row is Q8(fp16_rne(R(x))) with R the
 *     rotation of rca_lm_kv_remove (the pair at elements j and j + 32, in f32, rows `delta` of the handle's cos / sin tables, the same
 *     sequence of f32 operations as on an fp16 cache) and Q8 the RULE above: per block of 32, d = amax / 127, inv = d != 0 ? 1 / d : 0,
 *     q = roundf(y * inv), d16 = fp16_rne(d).
 *   So a shifted q8_0 cache holds exactly what an fp16 cache holding the de-quantised rows would hold after its own rca_lm_kv_remove,
 *   quantised; "cache row == Q8(an fp16 row)" survives any number of shifts, and every shift costs the surviving keys one fp16
 *   rounding, as on the fp16 cache, PLUS one q8_0 quantisation (about 2^-8 of the block's largest value) -- the price this switch names.
 *   A row whose de-quantised values or rotation are not finite is treated as the quantiser treats such an fp16 row. */
int rca_lm_set_kv_shift_requant(rca_lm_t* h, int32_t on);
int rca_lm_get_kv_shift_requant(const rca_lm_t* h, int32_t* on);
/* bytes one cached position takes in the handle's KV format (all layers, K and V); ring_positions (may be NULL): positions of the
 * fp16 staging ring of a q8_0 cache, 0 for an fp16 cache */
int rca_lm_kv_bytes_per_position(const rca_lm_t* h, int64_t* bytes, int32_t* ring_positions);
/* Tests only, q8_0 handles (RCA_ERR_STATE otherwise): the raw blocks of positions [pos0, pos0 + n_pos) of one layer: int8 values
 * [n_pos][n_kv_heads][64] and fp16 scales [n_pos][n_kv_heads][2] of K and of V.  Any pointer may be NULL. */
int rca_lm_kv_read_q8(rca_lm_t* h, int32_t layer, int32_t pos0, int32_t n_pos, int8_t* k_q, uint16_t* k_d, int8_t* v_q, uint16_t* v_d);
/* Tests only: ONE decode GEMV stage exactly as the step launches it (same instance, geometry and current activation format) on a
 * host-supplied input.  kind 0 QKV (x = residual rows [M][hidden]; y = the q rows after RoPE [M][n_heads*64]; kv_host, if not NULL,
 * receives the M new K rows then the M new V rows of `layer`'s cache as raw fp16), 1 O (x [M][AO]), 2 gate/up (y = silu(g)*u [M][ffn]),
 * 3 down (x [M][ffn]), 4 head (layer ignored; y [M][V]).  For the residual-add stages (1, 3) the residual is zeroed first, so y is
 * the product alone.  Positions are n_tokens .. n_tokens+M-1; n_tokens is left as it was.  M is 1 or 2.  The handle's activation
 * buffers and the cache rows at those positions are overwritten.  For kinds 0, 2 and 4 the device region that is read back is filled
 * with NaN before the launch, so an element the stage does not write comes back NaN (kinds 1 and 3 add to the zeroed residual: a
 * skipped element comes back 0).  The head's temporary output carries a guard of 64 floats behind row M - 1: RCA_ERR_STATE when the
 * launch changed it. */
int rca_lm_gemv_tap(rca_lm_t* h, int32_t layer, int32_t kind, const float* x_host, int32_t M, float* y_host, int64_t y_numel,
                    uint16_t* kv_host);
/* Tests only: the instance and grid of the last decode GEMV launch of the handle, recorded on the host (rca_lm_gemv_tap clears the
 * record before its launch): form[0..7] = M, NIT (16-byte chunks per lane and wave), R (rows per batch), batches per workgroup, grid,
 * format id of the matrix (rca_lm_weight_format's numbering, 4 = q6_k), ACT (0 f32 / 1 q8_1 activations), N (rows of the launch).  A
 * stage of two launches (a layer that keeps V in a format of its own) leaves the second launch's record. */
int rca_lm_gemv_tap_form(const rca_lm_t* h, int32_t* form);
/* Tests only: the attention of ONE layer exactly as a pass launches it (the same launcher picks the kernel, the grid and the merge), for
 * M query tokens at positions n_tokens .. n_tokens+M-1 over whatever the layer's cache holds (rca_lm_kv_write).  q_host [M][n_heads*64]
 * f32 are the query rows after RoPE.  route 0: the decode launch (M 1..2, follows rca_lm_set_attn_fuse); 1: the prefill launch with f32
 * output (the 32-token-tile route's, M 1..1024); 2: the prefill launch with bf16 hi / lo output (the 128-token-tile route's; hi + lo is
 * returned as f32), refused on a handle whose prefill route is not that one.  nsp_launch: 256-key splits the decode launch covers, 0 =
 * the splits the positions need, else a value from there up to the handle's split count (the bucketed launches of the captured graphs).
 * out_host [out_rows][n_heads*64], M <= out_rows <= 1024: the device rows are filled with NaN before the launch, so rows >= M come back
 * NaN unless the kernel wrote them.  n_tokens is left as it was; the handle's activation buffers are overwritten.  A bad layer, route, M,
 * nsp_launch or out_rows, or positions past n_ctx, are refused before anything is touched. */
int rca_lm_attn_tap(rca_lm_t* h, int32_t layer, int32_t route, int32_t nsp_launch, const float* q_host, int32_t M, float* out_host,
                    int32_t out_rows);
/* Tests only: the decode attention of ONE layer for the members of a batch pass, exactly as rca_lm_batch_step / _frame / their _sel forms
 * and rca_duplex_batch_frame launch it (one helper makes the split launch over the member table and the merge for the pass and for
 * this call), for n = 1 or 2 query tokens per member at positions n_tokens .. n_tokens+n-1 of each member, over whatever the members'
 * caches hold at `layer` (rca_lm_kv_write).  sel NULL: the batch's own table, every member in its slot (n_sel ignored); else the
 * selection table of rca_lm_batch_frame_sel, the n_sel members sel[0..n_sel-1] in slots 0 .. n_sel-1 at the slot count of the
 * selection's class (8 / 16 / 32 / 64), the slots behind them all zero.  With NM the members of the pass, q_host [NM*n][n_heads*64] f32
 * are the query rows after RoPE, member k's token j in row k*n + j; out_host [out_rows][n_heads*64], NM*n <= out_rows <= 128, is the
 * f32 value bf16 hi + lo of the planes the O projection reads (route 2 of rca_lm_attn_tap).  The members are checked and staged as a
 * step's are (every member needs a sampler; the ids are dummies).  nsp_launch: the 256-key splits the launch covers, 0 = the most any
 * member of the pass needs, else a value from there up to the largest split count among ALL members of the batch (the graphs' buckets).
 * Before the launch the first out_rows rows of the planes are filled with NaN (all bits set), so the rows of dead slots and rows >=
 * NM*n come back NaN unless a kernel wrote them, and every partial buffer of a member of the pass is filled with NaN as a whole: a
 * partial the merge uses although no workgroup of this launch wrote it shows as NaN.  The planes are zeroed afterwards.  Every
 * member's n_tokens is left as it was; member 0's activation buffers are overwritten.  A bad layer, n, nsp_launch, out_rows or
 * selection, a member a step would refuse, or positions past a member's n_ctx are refused before anything is touched. */
int rca_lm_batch_attn_tap(rca_lm_batch_t* b, int32_t layer, int32_t n, int32_t nsp_launch, const int32_t* sel, int32_t n_sel,
                          const float* q_host, float* out_host, int32_t out_rows);
/* Tests only: ONE projection of a 128-token-tile pass exactly as the layer sequence, rca_lm_score and the batch head launch it (the same
 * launcher picks the k-slice form, the grids and the epilogue), on host-supplied activations.  Refused (RCA_ERR_ARG) on a handle whose
 * rca_lm_prefill_route is not 2.  xh_host / xl_host [M][K] are the bf16 hi / lo planes themselves (K = hidden; n_heads*64 for kind 1;
 * ffn for kind 3).  kind 0 QKV (both segments where the layer keeps V apart; y = the q rows after RoPE [out_rows][n_heads*64]; kv_host,
 * if not NULL, receives the M new K rows then the M new V rows of `layer`'s fp16 cache, raw; refused on a q8_0 cache), 1 O, 2 gate/up
 * (y = the hi + lo planes of silu(g)*u as f32 [out_rows][ffn]), 3 down, 4 head (layer and rows ignored; M <= 128 rows that are rows
 * row_base .. of a pass of row_base + M tokens, row_base a multiple of 128; y [out_rows][V] followed by the 128 values behind the
 * block's last row, out_rows <= 128).  For kinds 1 and 3 the residual rows are zeroed first, so y is the product alone.  rows is the
 * pass's launch geometry (M <= rows <= 1024: ceil(rows / 128) token blocks); input rows M .. of those blocks are bf16 NaN.  Output rows
 * M .. out_rows-1 (M <= out_rows <= 1024) are filled with NaN before the launch and come back NaN unless a kernel wrote them.  seq_min:
 * the workgroup threshold that picks the k-slice form for this call, -1 = the process value (RCA_LM_SEQ_MIN_WGS).  form, if not NULL,
 * receives the form that ran: grid.y, slices a workgroup walks, slices the epilogue launch adds (0: none, the GEMM's own epilogue), its
 * group size.  Positions (kind 0) are n_tokens .. n_tokens+M-1; n_tokens is left as it was; the handle's activation buffers are
 * overwritten.  A bad layer, kind, M, rows, out_rows or row_base, or positions past n_ctx, are refused before anything is touched. */
int rca_lm_gemm128_tap(rca_lm_t* h, int32_t layer, int32_t kind, const uint16_t* xh_host, const uint16_t* xl_host, int32_t M, int32_t rows,
                       int32_t row_base, int32_t seq_min, float* y_host, int32_t out_rows, uint16_t* kv_host, int32_t* form);
/* One scored position (rca_lm_score): what llama-perplexity and its --kl-divergence mode reduce a row of logits to, reduced on the
 * device so that the logits never leave it.  With P = softmax(logits) of the scored handle and P_base of the base handle:
 * lse = log sum_j exp(logit_j), max_logit / argmax = the largest logit and its LOWEST index, logprob = logit[target] - lse,
 * base_logprob = the same under the base, kl = KL(P_base || P) = sum_j p_base,j (b_j - a_j) - lse_base + lse.
 * A -inf logit has probability 0; a 0 * inf term of the KL sum counts as 0; a -inf in P where the base has mass gives kl = +inf.
 * flags: bit 0 = the row holds a NaN (logprob, lse, max_logit and kl are NaN), bit 1 = the base row holds one (base_logprob and kl
 * are NaN), bit 2 = kl is +inf.  target -1 ("not scored"): logprob and base_logprob are NaN.  Without a base: kl and base_logprob are
 * NaN and base_argmax is -1. */
typedef struct rca_score_row {
    float logprob, lse, max_logit, kl, base_logprob;
    int32_t argmax, base_argmax, flags;
} rca_score_row_t;
/* llama-perplexity (and --kl-divergence against `base`): llama_decode of a chunk with logits for every position, then
 * log_softmax / the KL sums per row on the host (llama.cpp tools/perplexity; the reference deploys through llama.cpp,
 * realtime_agent_resources.py:19-33, and scores with Llama.eval + log-softmax of _scores, llamacpp_utils.py:30-37).  Appends the n ids at
 * n_tokens exactly as a long rca_lm_eval_async does -- on the 128-token-tile route the same launches, so the KV cache holds the same
 * bits -- advances n_tokens and leaves the LAST position's logits where rca_lm_eval leaves them (sample / get_logits follow as after
 * an eval).  Every 128-token block gets its logits from the head on the same tiles into a scratch block and one row reduction;
 * rows_host[i] scores position i against targets[i] (-1 = skip; targets == NULL: ids shifted by one, the last -1).  Handles whose long
 * evals do not take the 128-token tiles (shape, or rca_lm_set_mfma_prefill(0)) are scored on the exact 2-token decode passes: slower,
 * same results within the routes' rounding.  logits_all is ignored.  base (may be NULL; any weight format, may be a
 * rca_lm_create_shared twin): advanced over the same ids in lock-step on its own stream, ordered by events; it must be another
 * handle on the same device with the same vocabulary, the same n_tokens and room for n more (both handles run the decode passes
 * unless both take the tiles).  One download of n rows and one synchronisation per call; the base handle is left pending like after
 * rca_lm_eval_async.  Refused, with nothing changed: context overflow (RCA_ERR_STATE), an id or target outside the vocabulary, a
 * mismatched base (RCA_ERR_ARG).  The scratch (128 x V floats per handle) is allocated by the first call; captured graphs stay valid. */
int rca_lm_score(rca_lm_t* h, rca_lm_t* base, const int32_t* ids, int32_t n, const int32_t* targets, rca_score_row_t* rows_host);
/* Tests only: the row reduction of rca_lm_score alone on M rows of host-supplied logits [M][V] (V = the handle's vocabulary;
 * base_logits_host may be NULL), targets [M] in [-1, V).  The handle's state is untouched. */
int rca_lm_score_rows_tap(rca_lm_t* h, const float* logits_host, const float* base_logits_host, const int32_t* targets, int32_t M,
                          rca_score_row_t* rows_host);
/* Tests only: logits_host [V] replaces the last logits row of the handle (RCA_ERR_STATE "no logits: call eval first" while there is
 * none); rca_lm_sample, rca_lm_token_probs and rca_lm_get_logits then behave as after an eval that had produced this row.  Nothing
 * else changes: the sampler's kernels can be driven with hand-made rows at their caps, ties and infinities. */
int rca_lm_put_logits(rca_lm_t* h, const float* logits_host);
/* Quantise a host matrix [rows][K] (src_dtype RCA_F32 / RCA_BF16 / RCA_F16, K % 256 == 0) on `device` into raw GGUF blocks, byte for byte
 * in the file layout: type RCA_Q8_0 (34 bytes per 32 values), RCA_Q4_K (144 per 256), RCA_Q5_K (176) or RCA_Q6_K (210); blocks_host takes
 * rows * K / values * bytes, which blocks_bytes must equal.  Stand-alone: no LM handle.  rule 1 = the scale searches of ggml's published
 * reference quantisers (make_qkx2_quants for Q4_K / Q5_K, make_qx_quants for Q6_K) as DESIGN.md "Quantising on the card" restates them
 * (ggml is not part of this tree: parity with llama-quantize's own bits is not pinned); rule 0 = this build's min / max rules: for
 * Q4_K / Q5_K the blocks rca_lm_config_t::decode_weights = 3 / 4 keeps, for Q6_K max |x| / 31 per group of 16.  Q8_0 has one rule
 * (d = amax / 127, ties away from zero: what decode_weights = 1 keeps) under either value.  The source goes up in slabs of at most 64 MiB
 * (one row at least) on a stream of the call's own; one synchronisation.  RCA_ERR_ARG with a message, before any HIP call, for a null
 * pointer, an unknown dtype, type or rule, K % 256 != 0, a wrong blocks_bytes; after the run, naming the first such row, for a source
 * value that is not finite and for a block whose d or dmin is not finite in fp16 (blocks_host then holds no usable result). */
int rca_quantize_rows(int32_t device, const void* src_host, int32_t src_dtype, int64_t rows, int64_t K, int32_t type, int32_t rule,
                      void* blocks_host, int64_t blocks_bytes);
/* rca_quantize_rows under importance weights: col_weights [K] (or NULL), one non-negative finite f32 per input COLUMN, the same for every
 * row -- an importance matrix's in_sum2 / count.  NULL gives rca_quantize_rows' bytes.  With weights, rule must be
 * 1, and Q4_K / Q5_K / Q6_K follow ggml's published quantize_row_q{4,5,6}_K_impl with quant_weights as DESIGN.md "Weighted K-quant
 * search" restates them (tests/quant_weighted_ref.py is the definition; parity with llama-quantize's own bits is not pinned): the
 * sub-block search under w = qw sqrt(sigma2 + x^2) on a finer grid, d and dmin from a weighted search over the eight scales / minima,
 * Q6_K's group search under w = qw.  A group of 32 (Q6_K: 16) columns whose weights are all 0 takes 1.0 for them.  Uniform weights do
 * NOT reproduce the unweighted bytes (the rules' parameters differ).  Q8_0 ignores the weights.  The block of a row that starts at
 * column c reads col_weights + c; the weights go up once per call.  RCA_ERR_ARG before any HIP call, beside rca_quantize_rows' own
 * refusals: weights with rule 0; a weight that is negative or not finite, naming its column. */
int rca_quantize_rows_w(int32_t device, const void* src_host, int32_t src_dtype, int64_t rows, int64_t K, int32_t type, int32_t rule,
                        const float* col_weights, void* blocks_host, int64_t blocks_bytes);
/* Tests only: the column sums an importance matrix is made of (what llama-imatrix collects: per input column of a projection, the sum
 * over the tokens of the squared activation), by the kernel meant to follow every launch that writes a projection's bf16 hi / lo input
 * planes on the 128-token tiles of a collecting pass (rca_lm_imatrix_chunk).  This call runs it alone on host-supplied
 * planes xh / xl [M][K] (bf16 bits) of which the first m_live rows are live, adding into the caller's double[K].  Per column j:
 * v_r = f32(hi[r][j]) + f32(lo[r][j]), s_r = v_r * v_r (no fma), the partial of token block b is p_b = ((0.0f + s_r0) + s_r1) + ...
 * over rows 128 b .. min(128 b + 127, m_live - 1) ascending, acc[j] += (double)p_b for b ascending; rows >= m_live are never read; no
 * atomics.  1 <= m_live <= M <= 1024.  The handle's state is untouched. */
int rca_lm_imatrix_rows_tap(rca_lm_t* h, const uint16_t* xh_host, const uint16_t* xl_host, int32_t M, int32_t K, int32_t m_live,
                            double* acc_inout_host);
/* Collecting an importance matrix (what llama-imatrix does), on handles whose long evals take the 128-token tiles.
 * rca_lm_imatrix_begin allocates and zeroes the handle's own accumulators (never shared with a twin): double, per layer the vectors of
 * kind 0 (width hidden: the input of attn_q / attn_k / attn_v), 1 (n_heads * head_dim: attn_output), 2 (hidden: ffn_gate / ffn_up) and
 * 3 (ffn: ffn_down), and one of kind 4 (hidden: output.weight) -- plus a token count.  RCA_ERR_STATE: the handle's long evals do not
 * take the 128-token tiles (rca_lm_set_mfma_prefill off, or weights / dimensions off them); the handle is already collecting.
 * rca_lm_imatrix_chunk appends n >= 1 tokens at n_tokens exactly as rca_lm_score walks them (passes of up to 1024 rows on the tiles, any
 * n), each pass summing every projection's bf16 hi / lo input planes right behind the launch that wrote them, by the definition at
 * rca_lm_imatrix_rows_tap (m_live = the pass's rows), and the final norm's planes of all its rows for kind 4; no logits but the last
 * position's are computed.  n_tokens, the K / V rows and the last logits are left bit for bit as rca_lm_score leaves them; the count
 * grows by n.  Refusals as rca_lm_score's (context overflow: RCA_ERR_STATE; an id outside the vocabulary: RCA_ERR_ARG), RCA_ERR_STATE
 * when the handle is not collecting; a refused call leaves sums and count untouched.  NO OTHER CALL COLLECTS: eval, eval_async, step,
 * score and the batch calls on a collecting handle leave sums and count as they are.
 * rca_lm_imatrix_get downloads the K sums of (layer, kind) (layer is ignored for kind 4) and, where count_out is not NULL, the count.
 * RCA_ERR_ARG for a layer or kind that does not exist, or a K that is not the kind's width (the message names it).
 * rca_lm_imatrix_end frees the accumulators (no-op when not collecting); so does rca_lm_destroy. */
int rca_lm_imatrix_begin(rca_lm_t* h);
int rca_lm_imatrix_chunk(rca_lm_t* h, const int32_t* ids, int32_t n);
int rca_lm_imatrix_get(rca_lm_t* h, int32_t layer, int32_t kind, double* sums_out, int32_t K, int64_t* count_out);
int rca_lm_imatrix_end(rca_lm_t* h);
/* Tests only: rca_lm_imatrix_chunk for ONE pass (1 <= n <= 1024) that also copies the planes of (layer, kind), device to device, right
 * behind their collection launch, and downloads their first n rows to xh_out / xl_out [n][K] (bf16 bits, K = the kind's width). */
int rca_lm_imatrix_chunk_tap(rca_lm_t* h, const int32_t* ids, int32_t n, int32_t layer, int32_t kind, uint16_t* xh_out, uint16_t* xl_out);
/* synchronise the handle's stream (timing) */
int rca_lm_sync(rca_lm_t* h);
int rca_codec_sync(rca_codec_t* h);

#ifdef __cplusplus
}
#endif
#endif /* RCA_H */
