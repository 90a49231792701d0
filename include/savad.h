/*
 * savad.h -- C ABI of libsavad.so: the MI355X (gfx950) self-attentive-VAD forward pass.
 *
 * This is the drop-in boundary for ONE path of voithru/voice-activity-detection: the call
 *     model_outputs = self.model(features=batch_inputs["feature"])        vad/predictor.py:224
 * i.e. SelfAttentiveVAD.forward (vad/models/self_attention.py:23-28, blocks in
 * vad/modeling/transformer.py), plus the two host loops either side of it in
 * VADFromScratchPredictor.predict_probabilities: the window gather (vad/predictor.py:180-220)
 * and the boosted-prediction scatter/softmax/mean (vad/predictor.py:238-258 and :95).
 *
 * The reference has no FFI (it is pure Python + torch.nn); the reference-side binding a
 * maintainer would add is the ctypes stub shown in INTEGRATION.md -- in this repo it is
 * voice_activity_detection_amd/_lib.py + model.py (an nn.Module with the reference's
 * constructor signature and state_dict keys whose forward() calls savad_forward).
 *
 * Conventions: plain pointers and sizes only; all tensor pointers are DEVICE pointers unless
 * stated; row-major contiguous; fp32.  Every call returns 0 on success or a negative
 * SAVAD_E_* code, with a thread-local message in savad_last_error().  Handles share nothing: use one handle per stream that has a forward in
 * flight (two or three batches in flight on as many streams fill the CU slots a single forward leaves idle: +25 % batches per second at
 * [32,800,80] fp32 -- voice_activity_detection_amd/pipeline.py does exactly that), never one handle from two streams at once.  Kernels are enqueued
 * on the caller's HIP stream (`stream` is a hipStream_t passed as void*; NULL = default
 * stream).  savad_forward allocates no device memory and never synchronises (the caller supplies the
 * workspace) for every T covered by an earlier savad_reserve(h, T_max); a longer T first grows the
 * library's positional-encoding table on that call (one hipMalloc + one stream synchronisation, the
 * counterpart of the reference's cache growth: vad/modeling/transformer.py:392-397), and the first
 * forward after savad_set_param enqueues the weight re-packing kernels on `stream`.
 */
#ifndef SAVAD_H
#define SAVAD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SAVAD_OK 0
#define SAVAD_E_INVALID (-1)     /* bad argument / shape */
#define SAVAD_E_UNSUPPORTED (-2) /* configuration outside what the gfx950 kernels implement */
#define SAVAD_E_HIP (-3)         /* HIP runtime error (message carries hipGetErrorString) */
#define SAVAD_E_STATE (-4)       /* e.g. forward before every parameter was set */
#define SAVAD_E_NOKEY (-5)       /* unknown state_dict key */

typedef struct savad_model* savad_handle;

/* Mirrors SelfAttentiveVAD.__init__(feature_size, num_layers, d_model, dropout)
 * (vad/models/self_attention.py:7-21; d_ff = 4*d_model :10, n_heads = 1 :18).  dropout is an
 * inference no-op and is not part of the ABI.  Any even d_model in [2, 4096] (the reference's positional encoding pairs
 * sin / cos columns) and any feature_size (rows are zero-padded to a multiple of 16 internally when needed).
 * d_model = 128 -- the only value the reference ships (tests/configs/vad/train_config.yaml:7-10) -- runs the tuned MFMA
 * kernels in fp32 or bf16; every other width runs plain fp32 kernels (csrc/savad_generic.h: same results to the fp32
 * tolerance, several times slower per FLOP, savad_set_precision(h, 1) is refused with SAVAD_E_UNSUPPORTED, and
 * savad_set_attention_splits(h, n > 1) there means "n query tiles per sequence"). */
typedef struct savad_config {
    int32_t feature_size;
    int32_t num_layers;
    int32_t d_model;
} savad_config;

/* Replaces SelfAttentiveVAD(...) construction + .to(device) (vad/predictor.py:277-279).
 * Allocates the library-owned packed weights on the CURRENT HIP device. */
int savad_create(const savad_config* cfg, savad_handle* out);
void savad_destroy(savad_handle h);

/* Replaces load_state_dict(checkpoint["state_dict"]) (vad/predictor.py:278), one tensor per call.
 * `key` is the reference state_dict key (e.g. "encoder.layers.0.self_attention.query_projection.weight");
 * `data` may be a host or a device pointer (hipMemcpyDefault); `numel` must match the key's shape.
 * The copy is enqueued on `stream`; the library keeps its own packed copy (LayerNorm affine
 * parameters are folded into the following Linear at the next forward). */
int savad_set_param(savad_handle h, const char* key, const float* data, size_t numel, void* stream);
/* state_dict introspection: number of keys, i-th key, its element count. */
int savad_num_params(savad_handle h);
const char* savad_param_key(savad_handle h, int i);
size_t savad_param_numel(savad_handle h, int i);

/* Pre-sizes the positional-encoding table (vad/modeling/transformer.py:392-397: the reference grows its cache
 * when T exceeds it) for sequences of up to T_max frames, so that savad_forward with T <= T_max neither
 * allocates nor synchronises.  May allocate and synchronise `stream` itself.  Once every parameter has been set
 * (savad_set_param) it also folds / packs the weights for the precision selected by savad_set_precision, so that the
 * FIRST forward after it enqueues nothing but its own kernels (HIP-graph capturable). */
int savad_reserve(savad_handle h, int T_max, void* stream);

/* Bytes of scratch savad_forward needs for a [B,T,F] batch (activations + attention partials). */
int savad_workspace_bytes(savad_handle h, int B, int T, size_t* bytes);

/* Replaces self.model(features=x) (vad/predictor.py:224): x [B,T,F] fp32 -> out [B,T,2] fp32
 * log-probabilities (LogSoftmax(dim=2), vad/models/self_attention.py:26-27).  Asynchronous on
 * `stream`.  B == 0 or T == 0 is a no-op.  Masks do not exist on this path (always None in the
 * reference: vad/modeling/transformer.py:24). */
int savad_forward(savad_handle h, const float* x, int B, int T, float* out, void* workspace, size_t workspace_bytes,
                  void* stream);

/* Arithmetic of the forward pass: 0 = fp32 operands on the exact-fp32 MFMA (default; log-probs within
 * 1e-4 of the reference), 1 = bf16 operands (weights, Q/K/V, probabilities, FFN activations) with fp32
 * accumulation, fp32 softmax / LayerNorm statistics, residual stream fp32 in registers / fp16 in memory (BASELINE.json
 * configs[2..3]; judged on AUC, not on 1e-4), 2 = "fp32s": the fp32 arithmetic of vad/modeling/transformer.py:281-284,
 * 347,351-363,370-375 on the bf16 matrix pipe -- every GEMM operand kept as three bf16 pieces (hi + mid + lo = the fp32 value,
 * exactly), six bf16 MFMA products per K-step into one fp32 accumulator, everything else fp32 (softmax, LayerNorm, residual
 * stream): the same 1e-4 bar as precision 0, at 6/16 of its matrix time (gfx950 has no TF32; csrc/savad_kernels_f32s.h). */
int savad_set_precision(savad_handle h, int precision);
/* bf16 precision only: the residual stream lives in HBM as fp16 between kernels and saturates at +-65504 where the
 * reference's fp32 stream (vad/modeling/transformer.py:234-238) would not.  Saturation is counted, not silent: this
 * returns the number of residual elements clamped (or non-finite) since the previous call and clears the counter;
 * it synchronises `stream`.  0 on every parity workload; a model that reports > 0 needs precision 0 (fp32). */
int savad_residual_saturations(savad_handle h, unsigned long long* count, void* stream);
/* savad_forward with an explicit feature dtype: x_dtype 0 = fp32 [B,T,F], 1 = bf16 [B,T,F] (bf16
 * precision only).  Output is always fp32 log-probabilities. */
int savad_forward_ex(savad_handle h, const void* x, int x_dtype, int B, int T, float* out, void* workspace,
                     size_t workspace_bytes, void* stream);
/* The same with sequences that OVERLAP in memory: sequence b starts x_batch_stride elements behind sequence b-1
 * (x_batch_stride = T * feature_size is savad_forward_ex).  The streaming mode reads its windows [hop w, hop w + T) in place out of
 * the feature matrix with x_batch_stride = hop * feature_size -- no window copies (T > 32, feature_size a multiple of 16). */
int savad_forward_strided(savad_handle h, const void* x, int x_dtype, int B, int T, long x_batch_stride, float* out,
                          void* workspace, size_t workspace_bytes, void* stream);

/* Tuning knob: number of key-range splits of the attention stage (0 = automatic). */
int savad_set_attention_splits(savad_handle h, int splits);
/* Tuning knob: the launch schedule (results differ only in summation order; default 0 = automatic).
 *   fp32 operands
 *     1  row-wise stages on 32-row tiles, output features split over the workgroup's 4 waves; attention is its own
 *        launch (what automatic picks for small T > 32 batches)
 *     4  T <= 32: the whole forward in ONE launch, a workgroup per packed tile of floor(32/T) sequences (what
 *        automatic picks up to 1024 tiles unless the dense 32-row tiles of mode 1 fit fewer rounds of the CUs);
 *        T > 32: as 0
 *     2  row-wise stages on 128-row tiles, weight stream shared through LDS; attention and row stages are
 *        separate launches
 *     3  as 2, with attention and row chain of a query-block group fused into one launch per layer whenever
 *        T > 32 and the key range is not split (what automatic picks for large batches)
 *   bf16 operands
 *     1  separate attention / row launches, 4-wave workgroups      2  the same with 8-wave workgroups
 *     3  fused launches (T > 32)                                    0  fused up to ~4 workgroups per CU
 *     5  separate launches with the attention stage as ONE persistent launch (4 waves x 64 query rows per CU walking
 *        (sequence, 8 query blocks) items; csrc/savad_attn_pw_bf16.h).  Same bits as 1 except for the frames of a sequence's
 *        tail group of one or two query blocks (ceil(T / 32) mod 8 in {1, 2}), whose keys are summed as four partial softmaxes
 *        (key-split item): those agree with 1 to the bf16 rounding of the context.  Automatic picks it where a cost model of
 *        both attention kernels (savad.hip, pw_pays) has it ahead: large batches of long sequences ([160+,800], [256,1000] ...)
 *     0, 4 and 5 run the input stage, from one 32-row block per CU up, as ONE persistent launch with its weights resident in LDS
 *        (input_qkv_kernel_bf16_p; the same bits as the ring kernel 1 - 3 keep)
 *   bf16 operands, T <= 32 (the reference pipeline's 7-frame windows): 0 and 4 run the WHOLE forward in one launch (a wave per
 *        packed block for all layers, csrc/savad_packed_bf16.h; same bits as the per-layer launches of 1 - 3) in the variant
 *        the number of blocks suggests; 5 / 6 / 7 / 8 pin a variant (8-wave workgroups / 4 waves + 4 that move the weight stream
 *        through a 4-slot ring / 4 waves with a 2-slot ring / ONE block per workgroup, its four waves splitting every GEMM's
 *        output features: the latency variant, picked up to one block per CU)
 *   fp32s (split-bf16 operands), T <= 32: 0 and 4 run the WHOLE forward in one launch (csrc/savad_kernels_f32s.h) -- the latency
 *        variant (ONE packed block per workgroup, its four waves splitting every GEMM's output features, weights straight from L2
 *        into registers) up to two blocks per CU, a wave per block with the weight stream shared through the LDS ring beyond;
 *        8 pins the latency variant, 5 - 7 the wave-per-block one, 1 - 3 keep the per-layer launches.  The two variants agree to
 *        fp32 rounding (one fp32 sum is taken in another order), each is deterministic and independent of the batch. */
int savad_set_row_mode(savad_handle h, int mode);
/* bf16 operands: results that do not depend on the batch a sequence is evaluated in (0 = off, the default; 1 = on).  Every bf16 launch
 * schedule computes a frame with the same arithmetic, bit for bit -- with one exception: the persistent attention kernel that automatic
 * picks for large batches of long sequences sums the keys of a sequence's tail group of one or two query blocks as four partial
 * softmaxes (row_mode 5 above), so the same window can differ in the bf16 rounding of the context (<= 3e-3 in the log-probs) between a
 * 256-sequence batch and a 100-sequence remainder.  On: that kernel runs its tail groups as ordinary items (a second generated
 * instruction stream, csrc/savad_attn_pw_bf16_nosplit.inc) and every schedule -- hence every batching, chunk size and shard size --
 * gives the same bits, at about 9 % of that launch (3 - 4 % of a [256,800,80] forward).  fp32 operands: no effect (there a sequence's
 * result depends on its batch only through the automatic key-split count, <= 2e-6; savad_set_attention_splits(h, 1) pins that).
 * The reference itself (BLAS blocking) is not batch-invariant at the bit level. */
int savad_set_batch_invariant(savad_handle h, int on);
/* Per-kernel timing (bench.py's roofline block).  savad_set_profiling(h, capacity): the next `capacity` calls of
 * savad_forward bracket every launch with hipEvents on `stream` (capacity 0 switches profiling off and frees the
 * events); savad_profiling_skip(h, n): the next n forwards run un-recorded first (event creation idles the GPU for
 * a moment and the first ~15 ms of kernels afterwards run at lower clocks: 230 -> 207 us measured);
 * savad_last_kernel_times: after the caller has synchronised the stream, the launch names and their average duration
 * (ms) over the recorded forwards; returns the number of kernels written (<= max) and starts a new recording. */
int savad_set_profiling(savad_handle h, int capacity);
int savad_profiling_skip(savad_handle h, int forwards);
int savad_last_kernel_times(savad_handle h, const char** names, float* ms, int max);

/* Window geometry of the predictor: offsets = arange(-half,0,jump) ++ [0] ++ arange(1,half+1,jump) (vad/predictor.py:186-212).
 * Returns W = the NUMBER OF OFFSETS = 2*ceil(half/jump) + 1 (half >= 0, jump >= 1; any other value: SAVAD_E_INVALID); offsets (host
 * pointer, >= W ints) may be NULL.  Every entry below counts its window frames this way.  The reference sizes its result with
 * 2*(half-1)/jump + 3 (floor division, vad/predictor.py:57-59), which equals W exactly when 2*((half-1) mod jump) < jump (19/9, any
 * jump = 1 ...); where it does not (4/2, 9/3, 0/2) the reference itself fails, and the Python layer refuses the geometry.  The C ABI
 * serves every half / jump with W <= 64. */
int savad_window_offsets(int half, int jump, int32_t* offsets);

/* Replaces the per-window python gather loop (vad/predictor.py:182-220): for item i in
 * [first, first+count): windows[i-first][w][:] = feature[half+i+off[w]][:], positions[i-first][w] =
 * half+i+off[w].  feature [N,F] fp32, windows [count,W,F] fp32, positions [count,W] int64 (may be NULL).  With F a multiple of 4
 * the rows move in 16-byte pieces: feature and windows 16-byte aligned; any other F goes one float at a time. */
int savad_gather_windows(const float* feature, int N, int F, int half, int jump, int first, int count, float* windows,
                         int64_t* positions, void* stream);

/* The whole of VADFromScratchPredictor.predict_probabilities (vad/predictor.py:159-262) in one call: feature [N,F] fp32
 * (device) -> probs [N,W] (the boosted positive-class probabilities, unfilled slots exactly 0.5) and mean [N] (may be
 * NULL) = probs.mean(axis=1) (vad/predictor.py:95).  Windows are cut as savad_gather_windows does, `chunk` windows per
 * forward (the reference's chunk_size, :180); results are those of savad_gather_windows + savad_forward + savad_boost
 * (bit for bit when the forwards run the same launch schedule).  With fp32 arithmetic, W <= 32 and at most 1024 packed
 * tiles (4096 windows of 7 frames) the forward reads its windows straight out of the feature matrix (no window copies,
 * no positions, no scatter): two launches for the whole clip.  Asynchronous on `stream`, no allocation;
 * workspace from savad_predict_workspace_bytes (same N, half, jump, chunk and the handle's current precision). */
int savad_predict_workspace_bytes(savad_handle h, int N, int half, int jump, int chunk, size_t* bytes);
int savad_predict_probabilities(savad_handle h, const float* feature, int N, int half, int jump, int chunk, float* probs,
                                float* mean, void* workspace, size_t workspace_bytes, void* stream);

/* Replaces the boosted prediction (vad/predictor.py:238-258 and :95):
 *   boosted[N][W][2] = 0; boosted[positions[b][w]][w] = logp[b][w]  (scatter)
 *   probs[n][w] = softmax(boosted[n][w])[1]  (unfilled slots = exactly 0.5, and averaged in)
 *   mean[n] = mean_w probs[n][w]
 * logp [count,W,2] fp32, positions [count,W] int64, boosted_ws [N,W,2] fp32 scratch,
 * probs [N,W] fp32, mean [N] fp32 (may be NULL). */
int savad_boost(const float* logp, const int64_t* positions, int count, int N, int W, float* boosted_ws, float* probs,
                float* mean, void* stream);

/* MANY CLIPS IN ONE CALL.  The reference's windows are independent sequences, so the windows of several recordings can share
 * forwards without masks or padding -- as long as no window is cut across two recordings and every recording keeps its own
 * 0.5 placeholders.  A CLIP TABLE names the recordings inside one concatenated feature matrix [rows, F]:
 *   clip_first [C + 1] int32, non-decreasing, clip_first[0] = 0: clip c owns rows [clip_first[c], clip_first[c + 1]); rows =
 *   clip_first[C].  Clip c has n_c = max(0, its rows - 2 half) windows (vad/predictor.py:169); an empty clip and a clip too
 *   short for a window are legal.  The windows of all clips in clip order are the global ITEMS [0, sum n_c).
 * Every entry that launches takes the table twice: clip_first_host (HOST) is validated and planned from, clip_first (DEVICE, the same values)
 * is what the kernels read -- the library uploads nothing, allocates nothing and never synchronises; kernels go to `stream`.
 * Refused before anything is launched: C < 1, clip_first[0] != 0 or a decreasing table (SAVAD_E_INVALID); a window longer than
 * 64 frames, or sum n_c * W above 2^31 - 1 (SAVAD_E_UNSUPPORTED; the int32 table itself bounds rows by 2^31 - 1).
 *   savad_gather_windows_batch   savad_gather_windows for items [first, first + count): windows[i - first][w][:] =
 *       feature[clip_first[c] + half + local + off[w]][:] for item i = the local-th window of clip c; positions [count, W] int64
 *       (may be NULL) hold that row of the concatenated matrix.  items_first [C + 1] int32 (DEVICE) is written by the call: the
 *       exclusive prefix sum of n_c, which maps an item to its clip.  F a multiple of 4: 16-byte pieces, feature and windows
 *       16-byte aligned; any other F goes one float at a time.
 *   savad_boost_batch            the boosted prediction of every clip, read as a gather (no [rows, W, 2] scratch array, no
 *       positions): logp [sum n_c, W, 2] in item order -> probs [rows, W], mean [rows] (may be NULL); slot (n, w) of a clip is
 *       filled by the CLIP's window local - half - off[w] when that exists and is exactly 0.5 otherwise.  With one clip: the bits
 *       of savad_boost.  items_first as above (written by the call).
 *   savad_predict_probabilities_batch   savad_predict_probabilities for every clip of the table in one call: probs [rows, W] and
 *       mean [rows] (may be NULL) hold clip c's result in its rows.  The items run `chunk` (made even; at most sum n_c) per
 *       forward, whatever clips they belong to; the windows are always copied and each chunk is one savad_forward, in every
 *       precision and row mode: the bits of savad_gather_windows_batch + savad_forward per chunk + savad_boost_batch.  feature and
 *       workspace 16-byte aligned; workspace from savad_predict_batch_workspace_bytes (HOST arithmetic: it takes the host table
 *       only) for the same table, half, jump, chunk and the handle's current settings. */
int savad_gather_windows_batch(const float* feature, const int32_t* clip_first_host, const int32_t* clip_first, int C, int F, int half,
                               int jump, int first, int count, int32_t* items_first, float* windows, int64_t* positions, void* stream);
int savad_boost_batch(const float* logp, const int32_t* clip_first_host, const int32_t* clip_first, int C, int half, int jump,
                      int32_t* items_first, float* probs, float* mean, void* stream);
int savad_predict_batch_workspace_bytes(savad_handle h, const int32_t* clip_first_host, int C, int half, int jump, int chunk,
                                        size_t* bytes);
int savad_predict_probabilities_batch(savad_handle h, const float* feature, const int32_t* clip_first_host, const int32_t* clip_first,
                                      int C, int half, int jump, int chunk, float* probs, float* mean, void* workspace,
                                      size_t workspace_bytes, void* stream);

/* Streaming long-form mode (BASELINE.json configs[4]: sliding windows T=800, hop=400; NOT a mode of
 * the reference, whose predictor only cuts 7-frame windows -- the rule below is this build's):
 * window w covers frames [hop*w, hop*w+T) of feature[N,F], zero-padded past N; the number of windows
 * is savad_stream_window_count = N <= T ? 1 : ceil((N-T)/hop) + 1.  After savad_forward on the
 * windows, savad_overlap_merge gives probs[n] = mean over the windows covering frame n of
 * softmax(logp[w][n-hop*w])[1] (mirrors the averaging of vad/predictor.py:95).  savad_gather_strided copies the windows
 * [first, first + count) in 16-byte pieces (F a multiple of 4; feature and windows 16-byte aligned); logp is read as 8-byte
 * (log p0, log p1) pairs here and in savad_boost. */
int savad_stream_window_count(int N, int T, int hop);
int savad_gather_strided(const float* feature, int N, int F, int T, int hop, int first, int count, float* windows,
                         void* stream);
int savad_overlap_merge(const float* logp, int W, int N, int T, int hop, float* probs, void* stream);

/* Log-mel front-end (next-row 1 of the scope table): replaces, for the reference's only transform
 * configuration (n_fft 512, hop 160, window 400, 80 mels, 16 kHz: tests/configs/vad/train_config.yaml:
 * 18-26), FeatureExtractor.extract_with_postprocessing = librosa.feature.melspectrogram(...) ->
 * log(x + 1e-6) -> transpose (vad/acoustics/transforms/log_mel_spectrogram.py:19-32,
 * vad/acoustics/feature_extractor.py:71-80).  audio: n_samples fp32 mono 16 kHz (device);
 * features: [savad_logmel_frames(n_samples) = 1 + n_samples/160][80] fp32 (device), ready to be the
 * model's / predictor's feature matrix; workspace: savad_logmel_workspace_bytes(n_samples) bytes. */
int savad_logmel_frames(int n_samples);
size_t savad_logmel_workspace_bytes(int n_samples);
int savad_logmel(const float* audio, int n_samples, float* workspace, float* features, void* stream);
/* The same for a SPAN of the frames -- what one rank of a sharded run computes (each rank only the frames its
 * windows cover).  audio points at sample audio_first of a signal of n_samples samples and holds audio_count of them;
 * frames [frame_first, frame_first + frame_count) are written to features[frame_count][80].  The slice must hold the
 * samples savad_logmel_span_samples names for these frames (160 f - 208 .. 160 f + 207 of every frame, plus the
 * mirrored stretch when the span touches an end of the signal: centre=True, reflect padding); *first is a multiple of
 * 4, so that a slice cut there keeps the 16-byte alignment of the direct reads (any other slice is copied first).
 * workspace: savad_logmel_span_workspace_bytes(frame_count) bytes, 16-byte aligned. */
int savad_logmel_span_samples(long n_samples, int frame_first, int frame_count, long* first, long* count);
/* 16-bit PCM (device) -> float32 samples in [-1, 1): sample / 32768, exactly what the reference's AudioData.load obtains from
 * soundfile for a PCM16 source (vad/data_models/audio_data.py:21-24,32).  For uploads from the host: PCM16 is half the bytes
 * of the float signal the log-mel entry points take (StreamingPredictor.predict_audio_host).  pcm: 2-byte aligned (8-byte
 * aligned slices move four samples per load); audio: 16-byte aligned. */
int savad_pcm16_to_f32(const short* pcm, long n_samples, float* audio, void* stream);
size_t savad_logmel_span_workspace_bytes(int frame_count);
int savad_logmel_span(const float* audio, long audio_first, long audio_count, long n_samples, int frame_first,
                      int frame_count, float* workspace, float* features, void* stream);
/* Experiments and tests: algorithm 0 (default) = the STFT as a factored DFT (512 = 32 x 16, two small GEMMs with the
 * twiddles folded into the second), 1 = the DFT as one GEMM (rounds 1-4; whole-signal calls only).  Process-wide.
 * savad_logmel_tables_host copies the factored kernel's three A-operand tables (savad_logmel_table_floats(0..2)
 * floats each) to HOST memory: the CPU suite replays the kernel's data flow on them against the oracle. */
int savad_logmel_set_algorithm(int algorithm);
int savad_logmel_table_floats(int which);
int savad_logmel_tables_host(float* t1, float* t3, float* tm);

/* THE LOG-MEL FEATURES OF MANY CLIPS IN ONE CALL: three launches whatever the number of clips, in front of
 * savad_predict_probabilities_batch.  An AUDIO CLIP TABLE names the clips inside one float32 buffer of audio_count samples (device):
 *   clips [C] {first, count}: clip c is samples [first, first + count).  count = 0 is legal and gives a clip without frames,
 *   count >= 1 gives savad_logmel_frames(count) = 1 + count / 160 frames.  first is a multiple of 4: the kernel reads 16-byte chunks
 *   straight from the clip and the batch has no aligned-copy fall-back.  Clips may overlap or repeat (they are only read: the
 *   chunks of one recording are used in place).  No sample outside [first, first + count) is read for clip c.
 * The call takes the table twice: clips_host (HOST) is validated and planned from, clips (DEVICE, the same values) is what the
 * kernels read -- the library uploads nothing, allocates nothing and never synchronises; kernels go to `stream`.
 * Refused before anything is launched: C < 1, a negative first or count, a clip that leaves [0, audio_count), a first that is no
 * multiple of 4 (SAVAD_E_INVALID); a clip of more than 2 000 000 000 samples, more than 2^31 - 1 rows or tiles in all
 * (SAVAD_E_UNSUPPORTED).
 *   savad_logmel_batch_shape            rows = the frames of all clips, tiles = sum ceil(frames_c / 32) (a tile of 32 frames never spans
 *       two clips); either pointer may be NULL.  HOST arithmetic.
 *   savad_logmel_batch_workspace_bytes  HOST arithmetic: tiles_first [C + 1] int32, then a mirrored-head slot of 208 floats and a
 *       tail slot of 212 floats per clip, every piece 16-byte aligned.
 *   savad_logmel_batch                  features [rows][80] fp32: clip c's rows are [clip_first[c], clip_first[c + 1]), with the bits of
 *       savad_logmel on the clip alone (a frame depends on nothing but its own 400 samples).  clip_first [C + 1] int32 (DEVICE) is
 *       written by the call: the row table savad_predict_probabilities_batch takes, so that its caller uploads no second table.
 *       audio, workspace, features and clip_first 16-byte aligned.  Writes exactly rows * 80 floats and C + 1 ints and stays inside
 *       the reported workspace.  Only the factored DFT has a batch form: after savad_logmel_set_algorithm(1) the call returns
 *       SAVAD_E_UNSUPPORTED. */
typedef struct {
    int64_t first, count;
} savad_audio_clip;
int savad_logmel_batch_shape(const savad_audio_clip* clips_host, int n_clips, int64_t audio_count, int64_t* rows, int64_t* tiles);
int savad_logmel_batch_workspace_bytes(const savad_audio_clip* clips_host, int n_clips, int64_t audio_count, size_t* bytes);
int savad_logmel_batch(const float* audio, int64_t audio_count, const savad_audio_clip* clips_host, const savad_audio_clip* clips,
                       int n_clips, void* workspace, float* features, int32_t* clip_first, void* stream);

/* Feature front-end for every transform a reference config can name (vad/acoustics/transforms/transform_factory.py:13-59)
 * and the temporal differences of vad/acoustics/feature_extractor.py:135-145 (stack_differences false), at 16 kHz.
 * hop / win in samples (int(hop_ms / 1000 * 16000), int(window_ms / 1000 * 16000)); output [n_frames][n_features] fp32:
 *   SAVAD_FE_LOGMEL / _MEL : librosa 0.8 melspectrogram (stft center=True, reflect padding, periodic Hann(win) centred in
 *                            n_fft, power 2, Slaney filterbank fmin 0 fmax 8 kHz) -> log(x + 1e-6) / as it is; n_mels features
 *   SAVAD_FE_MFCC          : power_to_db(mel, ref 1, amin 1e-10, top_db 80 -- the maximum over the whole call) -> DCT-II ortho,
 *                            first n_mfcc rows; n_frames = 1 + (n_samples + 2 (n_fft / 2) - n_fft) / hop for these
 *                            three (1 + n_samples / hop for an even n_fft)
 *   SAVAD_FE_SPECTROGRAM   : |torch.stft(center=False, periodic Hamming(win) centred in n_fft, onesided)|; n_fft / 2 + 1
 *                            features, n_frames = 1 + (n_samples - n_fft) / hop
 *   deltas = 1             : [x, delta(x, 9, order 1), delta(x, 9, order 2)] along the features (3x), at least 9 frames.
 * Limits: win <= n_fft <= 2048, 1 <= n_mels <= 256, 1 <= n_mfcc <= n_mels, n_samples >= n_fft / 2 + 1 (centred) or n_fft
 * (spectrogram).  The tables of a config are built on the host and uploaded to the current device on first use, which
 * synchronises: call savad_frontend_prepare before a graph capture; savad_frontend itself then only launches kernels.
 * savad_frontend_tables_host (which = 0 DFT [rows][kr], 1 mel [n_mels][n_fft/2+1], 2 DCT [n_mfcc][n_mels], 3 Savitzky-Golay
 * [order 2][position 9][tap 9]; savad_frontend_table_floats floats each) copies them to HOST memory for the CPU tests.
 * The DFT table's columns are frame samples k0 .. k0 + kr - 1, k0 = ((n_fft - win) / 2) rounded down to a multiple of 4,
 * kr = that window's end - k0 rounded up to 8; its rows: re(bin 0), re(bin n_fft/2) (zero for an odd n_fft), then re / im of
 * bins 1 .. ceil(n_fft/2) - 1, padded with zero rows to a multiple of 128.  audio: device, any alignment; workspace
 * (savad_frontend_workspace_bytes) and features: device, 16-byte aligned. */
#define SAVAD_FE_SPECTROGRAM 0
#define SAVAD_FE_MEL 1
#define SAVAD_FE_LOGMEL 2
#define SAVAD_FE_MFCC 3
typedef struct {
    int transform; /* SAVAD_FE_* */
    int n_fft, hop, win, n_mels, n_mfcc, deltas;
} savad_frontend_config;
int savad_frontend_shape(const savad_frontend_config* config, long n_samples, int* n_frames, int* n_features);
int savad_frontend_workspace_bytes(const savad_frontend_config* config, long n_samples, size_t* bytes);
int savad_frontend_prepare(const savad_frontend_config* config);
int savad_frontend(const savad_frontend_config* config, const float* audio, long n_samples, float* workspace, float* features,
                   void* stream);
int savad_frontend_table_floats(const savad_frontend_config* config, int which);
int savad_frontend_tables_host(const savad_frontend_config* config, int which, float* out);

/* Audio ingest on the device: what AudioData.load does before the first feature (vad/data_models/audio_data.py:18-34) for a
 * recording that is not 16 kHz mono -- the channel average (:26) and librosa.resample(audio, sr, 16000,
 * res_type="kaiser_fast") (:27-30) = resampy 0.2.x's band-limited interpolation + librosa's fix_length.
 *
 * Resampler.  One lane per output sample walks the taps in resampy's order with resampy's arithmetic (weight and product in
 * float64, the accumulator rounded to float32 after every tap, no contraction), and the time register takes the values of
 * resampy's repeated float64 addition (from a table of (first output, time, exact step) segments, one per binade of the
 * register; k * increment is NOT that value).  An output sample therefore has the bits of resampy's loop.
 *   savad_resample_length       ceil(n_samples * 16000 / rate) (in float64, as librosa computes it); outputs at or past
 *                               int(n_samples * 16000 / rate) are zero (fix_length).  n_samples for a 16 kHz source.
 *   savad_resample_set_window   the filter: resampy's "kaiser_fast" half window, SAVAD_RESAMPLE_WINDOW float64 values (HOST) =
 *                               kaiser(2 n + 1, 8.555504641634386)[n:] * (0.85 * sinc(0.85 * linspace(0, 16, n + 1))), n = 8192.
 *                               It is an INPUT, once per process: the bits of numpy's exp differ between CPUs (its AVX-512
 *                               path against libm), so a table built inside the library could not equal the one numpy /
 *                               resampy hold on every host.  A second call must pass the same bits.
 *   savad_resample_prepare      builds a rate's tables (the window scaled by the ratio when downsampling, its first
 *                               differences, the time segments) and uploads them to the current device: it allocates and
 *                               synchronises, so call it before a graph capture.  The compute entry points do this on
 *                               first use of a (device, rate); afterwards they only launch on `stream`.
 *   savad_resample              the whole signal: audio [n_samples] float32 (device) -> out [savad_resample_length] float32.
 *   savad_resample_span         outputs [out_first, out_first + out_count) from a slice that starts at input sample
 *                               audio_first and holds audio_count samples: the same bits as the rows of the whole call.  The
 *                               slice must hold the samples savad_resample_span_samples names (it may start up to 3 samples
 *                               later: *first is rounded down to a multiple of 4 so that a slice cut there keeps the 16-byte
 *                               alignment of float data).
 *   savad_resample_span_samples HOST arithmetic: [*first, *first + *count) contains every input sample those outputs read
 *                               (a wing has at most 8193 / int(min(1, ratio) * 512) taps), clipped to the signal; the lowest
 *                               sample read lies within 1 + 3 (one tap, alignment) of *first, the highest within 1 of the
 *                               end, unless clipped.  A span of nothing but fix_length zeros reads nothing: count 0.
 *   savad_resample_table_host / _segments_host   HOST copies for the CPU tests: the rate's window and differences
 *                               (SAVAD_RESAMPLE_WINDOW each; delta may be NULL), and up to `max` time segments -- returns their
 *                               number; *covered = the number of outputs the segments cover (2^45 input samples).
 *   savad_resample_set_table_mode   experiments: 0 (default) = a workgroup keeps the table in LDS, 1 = reads it through the cache.
 * Limits: 1000 <= rate <= 100000 Hz (a block's input span must fit the 160 KiB of LDS next to the 128 KiB table; outside:
 * SAVAD_E_UNSUPPORTED), sample counts are long, 16000 Hz is a plain copy (no window needed).
 *
 * savad_ingest_downmix: interleaved [n_frames][channels] samples (device) -> float32 mono with the bits of the host loader:
 * sample / 32768 for SAVAD_PCM_INT16, then numpy's float32 .mean(axis=1) = the left-to-right float32 sum divided by
 * float32(channels).  int16: channels <= 256 (every partial sum is exact); float32: channels <= 7 (numpy sums a row of 8 or
 * more elements in another order: refused with SAVAD_E_UNSUPPORTED).  One channel is savad_pcm16_to_f32 / a copy. */
#define SAVAD_RESAMPLE_WINDOW 8193
#define SAVAD_PCM_INT16 0
#define SAVAD_PCM_FLOAT32 1
long savad_resample_length(long n_samples, int rate);
int savad_resample_set_window(const double* half_window);
int savad_resample_prepare(int rate);
int savad_resample(const float* audio, long n_samples, int rate, float* out, void* stream);
int savad_resample_span_samples(long n_samples, int rate, long out_first, long out_count, long* first, long* count);
int savad_resample_span(const float* audio, long audio_first, long audio_count, long n_samples, int rate, long out_first,
                        long out_count, float* out, void* stream);
int savad_resample_table_host(int rate, double* window, double* delta);
int savad_resample_segments_host(int rate, int max, long* first, double* time, double* step, long* covered);
int savad_resample_set_table_mode(int mode);
int savad_ingest_downmix(const void* raw, int dtype, int channels, long n_frames, float* mono, void* stream);

/* Post-processing of the predict path (next-row 3 of the scope table); HOST pointers.
 * savad_trim_voice_activity  : vad/postprocessing/trim.py:4-66 (valley fill, hill flatten, hang before/over; the
 *                              hang pass only runs when hang_before > 0, as in the reference)
 * savad_frames_to_samples    : vad/postprocessing/convert.py:6-24; returns int((n-1)*hop + window) samples
 *                              (out == NULL: size query)
 * savad_samples_to_segments  : vad/postprocessing/convert.py:27-61; returns the segment count, writes up to `cap`
 *                              (start, end) SAMPLE indices (the reference's times are index / sample_rate)
 * savad_optimal_split        : vad/postprocessing/split.py:26-109 */
int savad_trim_voice_activity(const uint8_t* pred, int n, int min_vally, int min_hill, int hang_before, int hang_over,
                              uint8_t* out);
long savad_frames_to_samples(const double* frames, int n, int sample_rate, double hop_ms, double window_ms, double* out);
int savad_samples_to_segments(const double* samples, long n, long* starts, long* ends, int cap);
int savad_optimal_split(const double* pred, const double* probs, long n, long max_samples, double* out);

/* The same post-processing ON THE DEVICE (csrc/savad_post_device.h): probs [N, W] float32 -> the segments the four host
 * functions above give, bit for bit; only a segment count and count x 2 sample indices return to the host.
 *   savad_post_supported        HOST arithmetic, 1 or 0: 1 <= W <= 128 (numpy's float32 row mean sums longer rows in another
 *                               order), and a geometry whose hop is a whole number of samples >= 1 with
 *                               (n_frames - 1) * hop + window < 2^52 (then the reference's repeated `start += hop` is exact).
 *   savad_post_workspace_bytes  one workspace size for _frames and _segments of n_frames frames at that geometry.
 *   savad_post_frames           DEVICE pointers.  boosted [N] = numpy's float32 mean(axis=1) of probs; trimmed [N] (0 / 1) =
 *                               savad_trim_voice_activity of (boosted > threshold).  Asynchronous on `stream`: launches only,
 *                               no allocation, no synchronisation.  Trim parameters must not be negative.
 *   savad_post_segments         trimmed, boosted: DEVICE; starts, ends: HOST.  The segments of savad_samples_to_segments over
 *                               savad_frames_to_samples of `trimmed`; with max_samples > 0 after savad_optimal_split against
 *                               savad_frames_to_samples of `boosted` (max_samples == 0: no split, boosted may be NULL).
 *                               Returns the segment count and writes up to `cap` pairs.  SYNCHRONISES `stream` (at least
 *                               once; with a split once more per range query of the recursion: a long segment needs on
 *                               the order of length / max_samples queries).
 *   savad_post_sample_probs     boosted [N] (device) -> out (device, float64, as many elements as the size query of
 *                               savad_frames_to_samples names) = savad_frames_to_samples of boosted.  Asynchronous.
 *   savad_post_frames_host / savad_post_sample_class_host   HOST twins for the CPU tests: the arithmetic the kernels run
 *                               (shared inline functions) in plain loops on host pointers; the second writes the classes
 *                               (0 = value 0.0, 1 = value 1.0, 2 = in between) of samples [first, first + count).
 *   savad_post_set_block        process-wide test knob: elements per workgroup block of the scans, 0 (default) or a power of
 *                               two from 64 to the default 2048, so that a small input runs three and more scan levels.
 * N == 0 is a no-op (0 segments).  Frame counts are int, sample indices long. */
int savad_post_supported(int W, int sample_rate, double hop_ms, double window_ms, int n_frames);
int savad_post_workspace_bytes(int n_frames, int W, int sample_rate, double hop_ms, double window_ms, size_t* bytes);
int savad_post_frames(const float* probs, int N, int W, float threshold, int min_vally, int min_hill, int hang_before, int hang_over,
                      float* boosted, uint8_t* trimmed, void* ws, size_t ws_bytes, void* stream);
int savad_post_segments(const uint8_t* trimmed, const float* boosted, int N, int sample_rate, double hop_ms, double window_ms,
                        long max_samples, long* starts, long* ends, int cap, void* ws, size_t ws_bytes, void* stream);
int savad_post_sample_probs(const float* boosted, int N, int sample_rate, double hop_ms, double window_ms, double* out, void* stream);
int savad_post_frames_host(const float* probs, int N, int W, float threshold, int min_vally, int min_hill, int hang_before,
                           int hang_over, float* boosted, uint8_t* trimmed);
int savad_post_sample_class_host(const uint8_t* frames, int n, int sample_rate, double hop_ms, double window_ms, long first,
                                 long count, uint8_t* cls);
int savad_post_set_block(int elems);

/* The device post-processing for EVERY CLIP OF A BATCH (csrc/savad_post_batch.h): probs [rows, W] of a clip table (clip_first
 * [C + 1] as above, passed as clip_first_host and clip_first) -> every clip's segments, each clip with the results of
 * savad_post_frames + savad_post_segments on its rows alone, integer for integer and bit for bit.  The number of launches and of
 * stream synchronisations does not depend on the number of clips.  Clip boundaries: an edge never exists at a clip's first row,
 * and the whole-matrix edge scans are clamped to the row's clip (a last edge before it, a first edge at or behind its end: none);
 * the clips' sample domains lie one after the other as SLOTS -- a clip of n > 0 frames owns its int((n - 1) * hop + window)
 * samples and one closing slot, a clip without rows owns nothing -- and "voice before this sample" restarts behind every
 * closing slot.  Sample indices are local to the clip.
 *   savad_post_batch_supported        HOST arithmetic, 1 or 0: a clip table whose every clip savad_post_supported takes.
 *   savad_post_batch_slot_table       HOST arithmetic: slot_first [C + 1] (host), the exclusive prefix sum of the clips' slots.
 *   savad_post_batch_workspace_bytes  HOST arithmetic from the table: one size for _frames and _segments.
 *   savad_post_batch_frames           DEVICE pointers; boosted [rows], trimmed [rows].  Asynchronous: launches only.
 *   savad_post_batch_segments         trimmed, boosted, clip_first, ws: DEVICE; everything else HOST.  Returns the segment count of
 *       the batch; seg_first_host [C + 1]: clip c's segments are [seg_first_host[c], seg_first_host[c + 1]) of starts / ends, of
 *       which the first `cap` pairs are written.  max_samples > 0: long_host [C] = 1 for the clips that hold a segment longer than
 *       max_samples (flagged on the device); those clips' pairs come from savad_post_segments (the optimal split) on the clip's
 *       rows and are spliced in.  max_samples == 0: no split, boosted may be NULL, long_host all 0.  SYNCHRONISES `stream`: at
 *       most twice when no clip is flagged (counts, then pairs); a flagged clip adds savad_post_segments' own.
 *   savad_post_batch_frames_host / savad_post_batch_slot_class_host   HOST twins for the CPU tests, running the clip rules the
 *       kernels run (shared inline functions) in plain loops; the second writes the classes of all slots (0, 1, 2 as
 *       savad_post_sample_class_host; 3 = a closing slot).
 * Refused before anything is launched or written: what is not a clip table, negative parameters, a NULL pointer, a workspace
 * that is short or not 8-byte aligned.  savad_post_set_block governs these scans too.  rows == 0 is a no-op (0 segments). */
int savad_post_batch_supported(const int32_t* clip_first_host, int C, int W, int sample_rate, double hop_ms, double window_ms);
int savad_post_batch_slot_table(const int32_t* clip_first_host, int C, int sample_rate, double hop_ms, double window_ms, long* slot_first);
int savad_post_batch_workspace_bytes(const int32_t* clip_first_host, int C, int W, int sample_rate, double hop_ms, double window_ms,
                                     size_t* bytes);
int savad_post_batch_frames(const float* probs, const int32_t* clip_first_host, const int32_t* clip_first, int C, int W, float threshold,
                            int min_vally, int min_hill, int hang_before, int hang_over, float* boosted, uint8_t* trimmed, void* ws,
                            size_t ws_bytes, void* stream);
int savad_post_batch_segments(const uint8_t* trimmed, const float* boosted, const int32_t* clip_first_host, const int32_t* clip_first, int C,
                              int sample_rate, double hop_ms, double window_ms, long max_samples, long* seg_first_host, uint8_t* long_host,
                              long* starts, long* ends, int cap, void* ws, size_t ws_bytes, void* stream);
int savad_post_batch_frames_host(const float* probs, const int32_t* clip_first_host, int C, int W, float threshold, int min_vally,
                                 int min_hill, int hang_before, int hang_over, float* boosted, uint8_t* trimmed);
int savad_post_batch_slot_class_host(const uint8_t* frames, const int32_t* clip_first_host, int C, int sample_rate, double hop_ms,
                                     double window_ms, uint8_t* cls);

/* The metrics of the evaluate command ON THE DEVICE (csrc/savad_eval_device.h).  Every one of the 18 values of a file
 * (vad/evaluate.py:56-80) is a float64 expression of integers -- confusion counts, edge counts, a rank sum and per-boundary hit
 * counts -- so only those integers are computed here and return to the host; metrics.metrics_from_counts turns them into the
 * values of the host path, bit for bit.  Everything works on n = min(N, n_labels) frames.
 *   counters [SAVAD_EVAL_COUNTERS] (int64): SAVAD_EVAL_N = n; _POS = labels that are 1; _TRUE = true segments (rising edges of the
 *       labels, a 1 at frame 0 included); _NAN = frames whose boosted or single score is NaN; _BAD_LABEL = labels above 1 (with
 *       either above zero the other values mean nothing: use the host path); _U2 = twice the Mann-Whitney U of the boosted
 *       scores (mean of a row, numpy's float32 bits) with mid-ranks for ties, -0.0 equal to +0.0; then for the single
 *       prediction (probs[i][W / 2] > threshold) at SAVAD_EVAL_PRED and for the boosted one (mean > threshold) at
 *       SAVAD_EVAL_PRED + SAVAD_EVAL_PRED_STRIDE: TP, FP, FN, TN and the prediction's rising edges.
 *   seg [count x 8] (uint8), in the order of the true segments: (num, den) of the start boundary and (num, den) of the end
 *       boundary for the single prediction, then the same four for the boosted one.  Start boundary b: den = the frames of
 *       [b, min(b + L, n)), num = those where prediction == label; end boundary e: the frames of [max(e - L, 0), e].
 *   savad_eval_supported        HOST arithmetic, 1 or 0: 1 <= W <= 128 and 1 <= n < 2^31.
 *   savad_eval_workspace_bytes  the workspace of savad_eval_counts for n_frames frames, and of savad_eval_sort for n_frames elements.
 *   savad_eval_counts           probs [N, W] float32, labels [n_labels] uint8, workspace: DEVICE; counters, seg: HOST.  1 <= L <= 254
 *                               (5 in the reference).  Returns the number of true segments (their records are written), or a
 *                               negative code; seg_cap below that number is SAVAD_E_INVALID.  SYNCHRONISES `stream` (twice when
 *                               there are segments).  No allocation.
 *   savad_eval_sort             DEVICE pointers; the stable sort alone, on the kernels and the key mapping of savad_eval_counts:
 *                               sorted_keys = keys in ascending order of value (a -0.0 comes back as +0.0), sorted_labels = their
 *                               payload bytes.  Asynchronous.
 *   savad_eval_counts_host      HOST twin for the CPU tests: the same outputs from host pointers by the same inline functions,
 *                               std::stable_sort in place of the radix passes.
 *   savad_eval_set_block        process-wide test knob: elements per workgroup block of the sort and its scans, 0 (default) or a
 *                               power of two from 64 to the default 2048. */
#define SAVAD_EVAL_COUNTERS 16
#define SAVAD_EVAL_N 0
#define SAVAD_EVAL_POS 1
#define SAVAD_EVAL_TRUE 2
#define SAVAD_EVAL_NAN 3
#define SAVAD_EVAL_BAD_LABEL 4
#define SAVAD_EVAL_U2 5
#define SAVAD_EVAL_PRED 6
#define SAVAD_EVAL_PRED_STRIDE 5 /* TP, FP, FN, TN, rising edges */
int savad_eval_supported(int W, long n_frames, long n_labels);
int savad_eval_workspace_bytes(int n_frames, int W, size_t* bytes);
long savad_eval_counts(const float* probs, int N, int W, const uint8_t* labels, long n_labels, float threshold, int L, long* counters,
                       uint8_t* seg, long seg_cap, void* ws, size_t ws_bytes, void* stream);
int savad_eval_sort(const float* keys, const uint8_t* labels, long n, float* sorted_keys, uint8_t* sorted_labels, void* ws,
                    size_t ws_bytes, void* stream);
long savad_eval_counts_host(const float* probs, int N, int W, const uint8_t* labels, long n_labels, float threshold, int L,
                            long* counters, uint8_t* seg, long seg_cap);
int savad_eval_set_block(int elems);

/* The same metrics for EVERY CLIP OF A BATCH in one call (csrc/savad_eval_batch.h).  probs [rows, W] with the row clip table
 * clip_first [C + 1] of the batched prediction; ONE concatenated labels array with a table of its own, label_first [C + 1] (a
 * file's label count is not its row count); both tables as HOST and DEVICE copies holding the same values.  Clip c works on
 * n_c = min(rows_c, labels_c) frames and gets what savad_eval_counts returns for that clip alone -- nothing looks across a clip
 * boundary: edges, boundary windows, tie groups, "negatives before", _NAN and _BAD_LABEL are the clip's own.
 *   counters [C][SAVAD_EVAL_COUNTERS] (int64, HOST): clip c's block, SAVAD_EVAL_N = n_c included.
 *   seg [count x 8] (uint8, HOST): the boundary records in clip order, then segment order; clip c's are records
 *       seg_first_host[c] .. seg_first_host[c + 1] (seg_first_host [C + 1], HOST, written by the call).
 *   A clip with n_c = 0 is legal: zero counters, no records.  C = 1 gives the results of savad_eval_counts.
 *   savad_eval_batch_supported        HOST arithmetic, 1 or 0: C >= 1, both tables start at 0 and do not decrease, 1 <= W <= 128,
 *                                     fewer than 2^31 frames in all.
 *   savad_eval_batch_workspace_bytes  HOST arithmetic from the two host tables; the same at every savad_eval_set_block.
 *   savad_eval_batch_counts           probs, labels, the device tables, workspace (8-byte aligned): DEVICE.  Returns the batch's
 *                                     true-segment count, or a negative code.  Refused before anything is launched or written:
 *                                     C < 1, a table that does not start at 0 or decreases, W outside 1 .. 128, L outside
 *                                     1 .. 254, 2^31 frames or more, a NULL pointer, a short or misaligned workspace.  seg_cap
 *                                     below the count is SAVAD_E_INVALID once the counters are known (they are returned).  The
 *                                     number of launches does not depend on C; SYNCHRONISES `stream` at most twice (counters,
 *                                     then records).  No allocation.
 *   savad_eval_batch_counts_host      HOST twin for the CPU tests: evaldev::counts_host on every clip's slice, in a plain loop.
 * savad_eval_set_block governs the scans and sort blocks of the batch too (a sort block never spans two clips). */
int savad_eval_batch_supported(const int32_t* clip_first_host, const int32_t* label_first_host, int C, int W);
int savad_eval_batch_workspace_bytes(const int32_t* clip_first_host, const int32_t* label_first_host, int C, int W, size_t* bytes);
long savad_eval_batch_counts(const float* probs, const int32_t* clip_first_host, const int32_t* clip_first, const uint8_t* labels,
                             const int32_t* label_first_host, const int32_t* label_first, int C, int W, float threshold, int L,
                             long* counters, uint8_t* seg, long seg_cap, long* seg_first_host, void* ws, size_t ws_bytes, void* stream);
long savad_eval_batch_counts_host(const float* probs, const int32_t* clip_first_host, const uint8_t* labels,
                                  const int32_t* label_first_host, int C, int W, float threshold, int L, long* counters, uint8_t* seg,
                                  long seg_cap, long* seg_first_host);

/* LIVE SESSIONS: audio fed as it arrives, many streams per tick (csrc/savad_live_plan.h, csrc/savad_live.h).  The rows a stream's
 * ticks and its finish emit, concatenated, are savad_logmel + savad_predict_probabilities of the finished recording, row for row,
 * however the recording was cut into pushes.  Shipped front-end only (16 kHz mono).  After n samples of an open stream
 *   K(n) = 0 for n < 257, else (n - 208) / 160 + 1 frames are ready (a frame reads samples 160 f - 208 .. 160 f + 207),
 *   E(n) = max(0, K(n) - 2 half) rows are final (row f needs the window centred at f + half);
 * finish computes the frames up to N = 1 + n / 160 with the right-hand reflection and emits rows E .. N - 1.  Latency: 2 half
 * frames + 208 samples (393 ms at half = 19).
 * A TICK is: savad_live_plan (HOST arithmetic) writes the tick's tables -- entries (one per stream in the tick), log-mel tiles,
 * window items, row offsets -- into the caller's host buffer; the caller copies that buffer to the device as it is (the library
 * uploads nothing, allocates nothing, never synchronises); savad_live_step launches the tick on `stream`: append, log-mel over the
 * tile table, window gather over the item table, savad_forward per `chunk` items, log-prob history + boost -- a fixed number of
 * launches whatever the number of streams -- and moves the slots on.  Every entry point that launches takes the table twice:
 * table_host is validated and counted from, table_dev (the same bytes) is what the kernels read.
 *   config      streams = slots of the state; max_push_samples = the largest push; half, jump = the window geometry; chunk = items
 *               per forward (rounded down to whole packed blocks).
 *   slots       HOST, streams x savad_live_slot, caller-owned, zeroed = all closed.  savad_live_open opens one.
 *   state       DEVICE, savad_live_state_bytes, 16-byte aligned, caller-owned; needs no initialisation.
 *   pushes      HOST; data = the DEVICE address the samples will have when the tick runs (float32: 4-byte aligned; int16 PCM,
 *               converted as savad_pcm16_to_f32 does: 2-byte aligned); n_samples = 0 is legal; finish != 0 ends the stream after
 *               the push (the slot is closed by the step and may be opened again: nothing of its state is read by the successor).
 *   rows        HOST, 2 x n_pushes int64 (may be NULL): first row index in the recording and row count of each push.
 *   probs/mean  DEVICE, [counts.rows, W] and [counts.rows] (mean may be NULL), the pushes' rows in push order.
 *   workspace   DEVICE, savad_live_workspace_bytes (the handle's current settings), 16-byte aligned; the device table likewise.
 * Refused before anything is launched: a window longer than 64 frames (SAVAD_E_UNSUPPORTED); a push above max_push_samples, a
 * closed slot (in the pushes, or in a table that no longer describes the slots), a finish below 257 samples, a slot twice in one
 * tick, null tables (SAVAD_E_INVALID).
 * Stage entries (tests hold each to bits): savad_live_append, savad_live_logmel, savad_live_gather (items [first, first + count) ->
 * windows [count, W, F]), savad_live_boost (logp [counts.items, W, 2] in item order), savad_live_commit (HOST: the slots move on);
 * savad_live_step = these in order around the forwards. */
typedef struct savad_live_config {
    int32_t streams, max_push_samples, half, jump, chunk;
} savad_live_config;
typedef struct savad_live_slot {
    int64_t n_samples; /* pushed so far */
    int64_t base;      /* library bookkeeping: first sample the state still holds */
    int32_t open;
    int32_t phase;     /* library bookkeeping */
} savad_live_slot;
typedef struct savad_live_push {
    int32_t slot, n_samples, dtype /* SAVAD_PCM_FLOAT32 or SAVAD_PCM_INT16 */, finish;
    const void* data;
} savad_live_push;
typedef struct savad_live_counts {
    int32_t entries, tiles, items, rows;
    int32_t table_bytes; /* bytes of the table the plan wrote */
    int32_t W;
} savad_live_counts;
long savad_live_ready_frames(long n_samples);
long savad_live_final_rows(long n_samples, int half);
int savad_live_state_bytes(const savad_live_config* config, size_t* bytes);
int savad_live_table_bytes(const savad_live_config* config, int max_pushes, size_t* bytes);
int savad_live_max_rows(const savad_live_config* config, int* rows_per_stream);
int savad_live_workspace_bytes(savad_handle h, const savad_live_config* config, int max_pushes, size_t* bytes);
int savad_live_open(const savad_live_config* config, savad_live_slot* slots, int slot);
int savad_live_plan(const savad_live_config* config, const savad_live_slot* slots, const savad_live_push* pushes, int n_pushes,
                    const void* state, void* table_host, size_t table_bytes, savad_live_counts* counts, int64_t* rows);
int savad_live_append(const savad_live_config* config, const void* table_host, const void* table_dev, void* stream);
int savad_live_logmel(const savad_live_config* config, const void* table_host, const void* table_dev, void* stream);
int savad_live_gather(const savad_live_config* config, const void* table_host, const void* table_dev, int first, int count,
                      float* windows, void* stream);
int savad_live_boost(const savad_live_config* config, const void* table_host, const void* table_dev, const float* logp, float* probs,
                     float* mean, void* stream);
int savad_live_commit(const savad_live_config* config, const void* table_host, savad_live_slot* slots);
int savad_live_step(savad_handle h, const savad_live_config* config, savad_live_slot* slots, const void* table_host,
                    const void* table_dev, float* probs, float* mean, void* workspace, size_t workspace_bytes, void* stream);

/* LIVE SESSIONS, EVENTS (csrc/savad_live_post.h): "speech started at sample s" / "speech ended at sample e" as soon as no
 * continuation of the recording can change them.  One more stage of a tick, called after savad_live_step (or savad_live_boost) with
 * the tick's tables and its compact probs [counts.rows, W]; two launches whatever the number of streams.  The events of a stream,
 * concatenated over its ticks, are the segments savad_post_frames + savad_post_segments (max_samples = 0) give for the finished
 * recording's probabilities, index for index: START = a segment's first sample, END = its last.
 *   post config W = the window geometry's; threshold and the trim parameters in frames, as predict() derives them (all >= 0).
 *   look-ahead  after R final rows of an open stream every event at a sample s with 160 (R - v - h - b) > s + 1 has been emitted
 *               (v, h, b = min_vally, min_hill, hang_before; hang_over needs none); a finish emits the rest.  Nothing is retracted.
 *               Worst-case latency behind the audio: the rows' 2 half frames + 208 samples, plus (v + h + b) frames.
 *   post state  DEVICE, savad_live_post_state_bytes (64 bytes per stream, whatever the parameters and however long the recording),
 *               16-byte aligned, caller-owned; needs no initialisation: an entry with row_first == 0 starts a recording.  An entry
 *               whose row_first is not the state's next row (the stage was skipped for a tick) gets count -1 and its state is left
 *               as it is.
 *   events      DEVICE, savad_live_post_event_bytes of the tick's table, 16-byte aligned, one contiguous buffer:
 *               int32 offsets[entries + 1] | int32 counts[entries] | padding to *events_offset | savad_live_event[offsets[entries]];
 *               the events of entry i (table order) are [offsets[i], offsets[i + 1]), in ascending sample order; counts[i] is their
 *               number, or -1.
 *   workspace   DEVICE, savad_live_post_workspace_bytes of the tick's table, 16-byte aligned.
 * savad_live_post is asynchronous on `stream`: no allocation, no synchronisation, no read-back.  Refused before anything is launched
 * (SAVAD_E_INVALID): W outside 1 .. 128 or not the geometry's, a negative parameter, null pointers, an event buffer or workspace
 * too small for the tick.
 * savad_live_post_host: HOST twin for the CPU tests -- the same inline functions in plain loops on a HOST state of
 * savad_live_post_state_bytes(post, 1, ..) bytes: one entry (rows row_first .. row_first + row_count - 1 of one stream, probs
 * [row_count, W], finish) -> up to `cap` events and *count (all events, also those beyond cap; -1 as above). */
#define SAVAD_LIVE_EVENT_START 0
#define SAVAD_LIVE_EVENT_END 1
typedef struct savad_live_event {
    int64_t sample;
    int32_t slot;
    int32_t kind; /* SAVAD_LIVE_EVENT_* */
} savad_live_event;
typedef struct savad_live_post_config {
    int32_t W;
    float threshold;
    int32_t min_vally, min_hill, hang_before, hang_over; /* frames */
} savad_live_post_config;
int savad_live_post_state_bytes(const savad_live_post_config* post, int streams, size_t* bytes);
int savad_live_post_event_bytes(const savad_live_config* config, const savad_live_post_config* post, const void* table_host, size_t* bytes,
                                size_t* events_offset);
int savad_live_post_workspace_bytes(const savad_live_config* config, const savad_live_post_config* post, const void* table_host,
                                    size_t* bytes);
int savad_live_post(const savad_live_config* config, const savad_live_post_config* post, const void* table_host, const void* table_dev,
                    const float* probs, void* post_state, void* events, size_t events_bytes, void* workspace, size_t workspace_bytes,
                    void* stream);
int savad_live_post_host(const savad_live_post_config* post, void* state, int slot, int64_t row_first, int row_count, int finish,
                         const float* probs, savad_live_event* events, int cap, int* count);

const char* savad_last_error(void);
const char* savad_version(void);

#ifdef __cplusplus
}
#endif
#endif /* SAVAD_H */
