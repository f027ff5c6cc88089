/* dimx.h -- C-ABI of libdimx_hip.so, the MI355X (gfx950) implementation of the DIM-Listener
 * hot path.  Plain pointers and sizes only; no torch types.  Every function returns 0 on
 * success and a negative dimx_status on failure (never throws); dimx_last_error() gives the
 * thread-local message.  All device work is enqueued asynchronously on the hipStream_t passed
 * in (as void*; NULL = the null stream).  A handle is bound to one device and is not
 * re-entrant across streams.  Two exceptions to "asynchronously": dimx_generate reads its chain kernels' fault word before it
 * returns (bf16 mode), and dimx_vq_encode / dimx_encode_ctx / dimx_vq_decode run batches of >= 16 384 rows as
 * clip groups on the handle's own side streams (fork / join events around them: every result is complete in stream order when
 * the call's stream reaches the join) -- if the call's stream still has work in flight when such a call is made, the call waits
 * for it on the host before it forks (DIMX_PREFILL_GROUPS=1 keeps one batch on the caller's stream and never waits).
 *
 * Each stage entry point replaces one method of the reference's Python operator surface
 * (paths relative to /root/reference):
 *
 *   dimx_vq_encode   <- SLMFT.forward_vq / VQAutoEncoder.encode
 *                       (code/seq2seq_pretrain.py:480-494, code/models/stage1_BIWI.py:22-27,307-317)
 *   dimx_vq_argmin   <- VectorQuantizer.forward, argmin part (code/models/lib/quantizer.py:35-47)
 *   dimx_vq_decode   <- SLMFT.forward_vq_decoder / VQAutoEncoder.decode
 *                       (code/seq2seq_pretrain.py:454-464, code/models/stage1_BIWI.py:29-37,376-393)
 *   dimx_encode_ctx  <- SLMFT.forward_encoder + the context concat of forward_decoder
 *                       (code/seq2seq_pretrain.py:431-446)
 *   dimx_decode_tf   <- AutoregressiveWrapper.forward via forward_decoder(mode='train')
 *                       (code/seq2seq_pretrain.py:448)
 *   dimx_generate    <- AutoregressiveWrapper.generate via forward_decoder(mode='val')
 *                       (code/seq2seq_pretrain.py:450)
 *
 * The dimx_op_* functions expose the individual HIP kernels for unit parity tests.
 */
#ifndef DIMX_H
#define DIMX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct dimx_ctx* dimx_handle;

typedef enum {
    DIMX_OK = 0,
    DIMX_ERR_ARG = -1,      /* bad argument (null pointer, shape out of range, misaligned) */
    DIMX_ERR_HIP = -2,      /* a HIP runtime call failed */
    DIMX_ERR_WEIGHT = -3,   /* unknown / missing / wrongly shaped weight tensor */
    DIMX_ERR_STATE = -4,    /* call order violated (e.g. decode before encode_ctx) */
    DIMX_ERR_WORKSPACE = -5 /* workspace too small */
} dimx_status;

/* numeric modes */
#define DIMX_MODE_PARITY_F32 0 /* f32 storage, f32-input MFMA: matches the CPU oracle to ~1e-5 */
#define DIMX_MODE_PERF_BF16 1  /* bf16 GEMM/attention operands, f32 accumulate + f32 residual stream */

/* element types for dimx_op_* */
#define DIMX_F32 0
#define DIMX_BF16 1

typedef struct {
    /* VQ-VAE (reference code/config.yaml:15-30) */
    int vq_in_dim, vq_hidden, vq_layers, vq_heads, vq_inter, vq_n_embed, vq_zdim;
    /* seq2seq (reference code/seq2seq_pretrain.py:369-418) */
    int dim_in, dim, dim_a, enc_depth, dec_depth, heads, dim_head, num_tokens, max_seq_len, ff_mult;
    /* 0 = DIM-Listener SLMFT (code/seq2seq_pretrain.py:325); 1 = legacy ListenerGenerator (code/seq2seq.py:138,
     * driven by code/x_engine.py): speaker VQ 824->768 with 8 codes per frame, x-tf encoder/decoder dim 512,
     * depth 6, heads 8, decoder with absolute positional embedding */
    int variant;
    /* speaker VQ-VAE geometry of variant 1 (reference code/config_speaker_old.yaml:15-30) */
    int spk_in_dim, spk_hidden, spk_heads, spk_inter, spk_face_quan_num;
    /* DIM-Speaker mesh head (EmocaConverter, reference code/seq2seq_pretrain.py:759-842): output width of vertice_map_reverse
     * (70110 in the reference); 0 = no head (dimx_default_dims / dimx_legacy_dims).  Needs variant 2. */
    int mesh_dim;
} dimx_dims;

typedef struct {
    const char* name;   /* state-dict key, e.g. "listener_vq.encoder.vertice_mapping.0.weight" */
    const float* data;  /* HOST pointer, float32, contiguous row-major; caller keeps ownership */
    int ndim;
    int64_t shape[4];
} dimx_weight_desc;

int dimx_version(void);
const char* dimx_last_error(void);
void dimx_default_dims(dimx_dims* d);
/* the legacy ListenerGenerator geometry (variant 1) */
void dimx_legacy_dims(dimx_dims* d);

int dimx_create(dimx_handle* h, int device_id, const dimx_dims* dims, int numeric_mode);
int dimx_destroy(dimx_handle h);
int dimx_numeric_mode(dimx_handle h);

/* Upload + pack weights (fused QKV, conv tap-major, bf16 copies, K padding).  May be called
 * several times; every key of the hot path must have been supplied before the first stage call
 * that needs it.  Unknown keys that belong to the reference surface but not to the path
 * (encoder_l.*, norm_l.*, norm.*, patch_embed_l, patch_embed_dec_l, *.project_out.weight / .bias) are
 * accepted and ignored.  OPTIONAL tensors (SURVEY A.2 [XT?]: details of x-transformers that differ between releases):
 * <encoder>.project_in.bias and <decoder>.to_logits.bias are applied when supplied and stay until dimx_begin_checkpoint (a call never
 * drops a tensor, so a chunked or key-sorted loader gives the same result in any order); a LayerNorm bias under *.attn_layers.* must
 * be all zero (DIMX_ERR_WEIGHT otherwise).  Any other unknown key is DIMX_ERR_WEIGHT.  Synchronous. */
int dimx_load_weights(dimx_handle h, const dimx_weight_desc* descs, int n);
/* A new checkpoint begins (what nn.Module.load_state_dict of another checkpoint means, code/finetune_s2s_pretrain.py:57): the
 * optional tensors of the previous one are forgotten; the required tensors stay until overwritten.  Synchronous. */
int dimx_begin_checkpoint(dimx_handle h);
/* number of hot-path tensors still missing (0 = ready) */
int dimx_missing_weights(dimx_handle h);

/* Bytes of caller-provided device workspace needed by any stage call at (B, T); 0 = shape not supported
 * (B < 1, T < 1 or T > max_seq_len). */
size_t dimx_workspace_bytes(dimx_handle h, int B, int T);
/* same, when dimx_generate will draw n_samples sequences per clip */
size_t dimx_workspace_bytes_samples(dimx_handle h, int B, int T, int n_samples);

/* Stream behaviour of the three prefill-sized stages (dimx_vq_encode, dimx_vq_decode(_latent), dimx_encode_ctx): from 16 384
 * rows (B x T) up they run as 2-4 clip groups, group 0 on `stream`, the others on side streams of the handle between a fork and a
 * join event (DIMX_PREFILL_GROUPS=1: never).  Consequences a pipelining caller must know: (1) when `stream` still has work in flight
 * the call WAITS FOR IT ON THE HOST before it forks (hipStreamSynchronize); (2) a `stream` that is being captured keeps one batch,
 * and the hipStreamQuery the fork uses must not run while ANOTHER thread captures in the global capture mode (use
 * hipStreamCaptureModeThreadLocal there, or DIMX_PREFILL_GROUPS=1); (3) on an error return the side streams have been joined:
 * nothing of the call still writes into `ws` once `stream` has drained.
 *
 * which: 0 = speaker VQ-VAE, 1 = listener VQ-VAE.
 * x: [B,T,56] f32, valid frames left-aligned; lens: [B] int32 device (NULL = all T).
 * pe_mode 0: every clip gets positional row 0 (the reference's batch-1 calls in forward_vq);
 * pe_mode 1: clip b gets row b + batch_row_offset (public batched VQAutoEncoder.encode).
 * idx: [B,T] int32, frames t >= lens[b] are set to pad_value.  z_out (optional) [B,T,128] f32. */
int dimx_vq_encode(dimx_handle h, int which, const float* x, const int32_t* lens, int B, int T,
                   int pe_mode, int batch_row_offset, int32_t pad_value, int32_t* idx, float* z_out,
                   void* ws, size_t ws_bytes, void* stream);

/* Nearest codebook entry, first index on ties.  z: [N,128] f32.  best_d / margin optional [N]. */
int dimx_vq_argmin(dimx_handle h, int which, const float* z, int N, int32_t* idx, float* best_d,
                   float* margin, void* stream);

/* idx: [B,L] int32 in [0,512).  Clip b is decoded with positional row b + batch_row_offset and
 * InstanceNorm / attention span the full L (reference behaviour on padded batches).
 * rows_per_clip S > 1 (multi-sample generation): rows b*S .. b*S+S-1 are samples of clip b and all use
 * positional row b + batch_row_offset, like S separate reference forwards would.  out: [B,L,56] f32. */
int dimx_vq_decode(dimx_handle h, int which, const int32_t* idx, int B, int L, int batch_row_offset,
                   int rows_per_clip, float* out, void* ws, size_t ws_bytes, void* stream);

/* VQAutoEncoder.decode on latents the caller supplies (reference code/models/stage1_BIWI.py:29-37: decode(quant)
 * applies the decoder to WHATEVER [B,128,L] tensor it is given, quantised or not): z [B,L,128] f32 (time-major,
 * i.e. quant.permute(0,2,1)), clip b decoded with positional row b + batch_row_offset.  out: [B,L,56] f32. */
int dimx_vq_decode_latent(dimx_handle h, int which, const float* z, int B, int L, int batch_row_offset,
                          float* out, void* ws, size_t ws_bytes, void* stream);

/* SLMFT.forward_encoder on its own (reference code/seq2seq_pretrain.py:431-442): x_s_out [B,T,384] f32 =
 * norm_s(encoder_joint(encoder_s(v_speaker + patch_embed_s))) with the causal attn_mask and the padding mask.
 * No audio, no context, no K/V projection; invalidates a context built earlier in the same workspace. */
int dimx_encode_speaker(dimx_handle h, const float* v_speaker, const uint8_t* mask, int B, int T,
                        float* x_s_out, void* ws, size_t ws_bytes, void* stream);

/* Multi-GPU sharding of one evaluation batch: this handle generates clips
 * [row_offset, row_offset + B) of a batch of rows_total clips.  Only the sampler's counter-based generator
 * depends on it (its counter is indexed by the GLOBAL sequence row, so the shards of a batch draw exactly what a
 * single process would draw for the same seed).  rows_total = 0 restores the default (the call's own B).
 *
 * The generator (csrc/sample_pick.hpp; the host definition the tests hold every route to is dimx.prng.sampler_noise).  A seeded
 * sampler call (exp_noise == NULL, seed != 0) at decode step `step` (the token column) divides the probability of code i of
 * global row g by
 *     ctr = (step * rows + g) * 512 + i                                     uint64, wraps
 *     z   = seed + (ctr + 1) * 0x9E3779B97F4A7C15                           uint64, wraps
 *     z   = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9;  z = (z ^ (z >> 27)) * 0x94D049BB133111EB;  r = z ^ (z >> 31)    (splitmix64)
 *     u   = (r >> 40) / 2^24                                                the top 24 bits, exact in f32
 *     q   = max(-log1p(-u), 2^-30)                                          Exp(1), f32 on the device
 * and takes token = argmax_i softmax(kept logits / temperature)_i / q_i, the lower index on a tie.  Nothing else is drawn: a forced
 * (prompted) column consumes no counter, and a prompted or streaming step t draws what dimx_generate draws at step t.
 * For a generation with S samples per clip, sample s of clip b of this handle is global row g = (row_offset + b) * S + s and
 * rows = rows_total * S (rows_total = 0: rows = B * S, row_offset = 0); clip groups do not enter (a group's rows keep their
 * numbers).  A guided generation has S = 1 and draws once per clip, for both branches.  The dimx_op_sample* launches on R rows have
 * g = the row and rows = R; a parameter block (dimx_op_sample_step, dimx_op_layer_chain_head) carries the window in words 6 / 7:
 * g = word 6 + row and rows = word 7 (0: the launch's rows_total). */
int dimx_set_shard(dimx_handle h, int row_offset, int rows_total);

/* Speaker encoder stack + context assembly + cross-attention K/V projection for all decoder
 * layers.  v_speaker [B,T,56] f32, v_audio [B,T,768] f32, mask [B,T] uint8 (1 = valid frame).
 * The result lives in the workspace (same ws must be passed to the decode call that follows).
 * x_s_out (optional): [B,T,384] f32 = norm_s(encoder_joint(encoder_s(.))).
 * for_generate: 0 -> cross K/V laid out for dimx_decode_tf, 1 -> for dimx_generate. */
int dimx_encode_ctx(dimx_handle h, const float* v_speaker, const float* v_audio, const uint8_t* mask,
                    int B, int T, int for_generate, float* x_s_out, void* ws, size_t ws_bytes,
                    void* stream);
/* Variant 1 (legacy ListenerGenerator, reference code/seq2seq.py:220-249) gives the same entry point this
 * meaning: v_speaker [B,T,824] f32 with the valid frames of each clip FIRST (the reference indexes
 * v_speaker[i][mask[i]]; the host compacts), v_audio ignored (may be NULL), mask [B,T] uint8 with
 * popcount(mask[b]) = number of valid frames; the speaker VQ-VAE encoder (batch-1 per clip, positional row 0),
 * the quantiser, the reference's channel-major re-view and the 6-layer bidirectional encoder run inside;
 * x_s_out (optional): [B,T,512] f32 encoder output.  dimx_decode_tf then takes kv_mask = NULL and
 * dimx_generate produces T (not T-1) tokens per sequence: tokens [B*S, T], logits_out [B*S, T, 512]. */

/* Variant 2 = the SLM pre-training model (reference code/seq2seq_pretrain.py:58-323; dims of the default
 * geometry with dimx_dims.variant = 2): bidirectional encoders incl. encoder_l, decoder with absolute positional
 * embedding.  dimx_slm_encode replaces SLM.forward_encoder (:200-221): v_speaker / v_listener [B,T,56] f32,
 * mask [B,T] uint8 (1 = valid), mask_speaker / mask_listener [B,T] uint8 (1 = frame masked out: its input row is
 * zeroed after the patch embedding was added; NULL = none); outputs f32 x_s, x_l [B,T,384], x_joint [B,2T,384]
 * (speaker half first).  2T must not exceed max_seq_len. */
int dimx_slm_encode(dimx_handle h, const float* v_speaker, const float* v_listener, const uint8_t* mask,
                    const uint8_t* mask_speaker, const uint8_t* mask_listener, int B, int T, float* x_s,
                    float* x_l, float* x_joint, void* ws, size_t ws_bytes, void* stream);

/* Cross-attention context from a given encoder output (SLM.forward_decoder :223-229, SLMFT :445-446):
 * context = cat(x + patch_embed_dec_{s (which_patch 0) | l (1, variant 2 only)}, v_audio) and the K/V projection
 * of every decoder layer.  x: f32 [B, ldx_rows, 384] of which the first T rows of every clip are used
 * (ldx_rows = T for a plain [B,T,384]; 2T to address a half of x_joint).  Then dimx_decode_tf / dimx_generate
 * as after dimx_encode_ctx. */
int dimx_set_context(dimx_handle h, const float* x, int ldx_rows, int which_patch, const float* v_audio, int B,
                     int T, int for_generate, void* ws, size_t ws_bytes, void* stream);

/* Test hook for variant 1: the x_speaker tensor of code/seq2seq.py:224-241 ([B,T,1024] f32, optional) and
 * the speaker code indices ([B,T*8] int32, -100 beyond the clip length, optional). */
int dimx_legacy_speaker_features(dimx_handle h, const float* v_speaker, const uint8_t* mask, int B, int T,
                                 float* x_speaker_out, int32_t* idx_out, void* ws, size_t ws_bytes,
                                 void* stream);

/* Teacher-forced decoder pass.  z_l [B,T] int32 (-100 = ignore), ctx_mask [B,T] uint8,
 * kv_mask [B,T-1] uint8 keep-mask for self-attention keys (NULL = keep all).
 * logits [B,T-1,512] f32; row_loss (optional) [B,T-1] f32 = per-position cross entropy (0 where the
 * target is -100); argmax_tok (optional) [B,T-1] int32.
 * dimx_set_cross_lookahead does not apply here: every position attends over the whole (masked) context. */
int dimx_decode_tf(dimx_handle h, const int32_t* z_l, const uint8_t* ctx_mask, const uint8_t* kv_mask,
                   int B, int T, float* logits, float* row_loss, int32_t* argmax_tok, void* ws,
                   size_t ws_bytes, void* stream);

/* The teacher-forced decoder pass under online visibility (the definition is dimx/online.py): dimx_decode_tf's stack with
 * every layer's cross attention bounded per query -- row t (it consumes position t and predicts position t+1) attends over the
 * context rows j < clamp(t + 2 + lookahead, 1, T) with ctx_mask[b][j] != 0, what decode step t of an online generation reads.  One
 * pass gives the logits a generation with every token forced gives step by step (other kernels: equal within the decode steps'
 * tolerance, not bit for bit).  The cross attention is csrc/win_attn.hip over the generation-layout K / V, so the context must
 * have been built with dimx_encode_ctx(for_generate = 1) in the same ws (DIMX_ERR_STATE otherwise).  No kv_mask: the random key
 * mask is a training device.  lookahead is this call's argument (any int; >= T-2 is the whole context) and independent of
 * dimx_set_cross_lookahead.  Variant 0 only; DIMX_ERR_STATE while a streaming session is open.  Outputs as dimx_decode_tf. */
int dimx_decode_tf_win(dimx_handle h, const int32_t* z_l, const uint8_t* ctx_mask, int B, int T, int lookahead, float* logits,
                       float* row_loss, int32_t* argmax_tok, void* ws, size_t ws_bytes, void* stream);

/* Autoregressive generation of T-1 tokens from start[B] with KV cache.
 * temperature <= 0 or exp_noise == NULL && seed == 0 -> greedy argmax.
 * exp_noise: [T-1,B,512] f32 Exp(1) samples (token = argmax softmax(top_k(logits)/temp)/noise);
 * if NULL and seed != 0 the noise is drawn on device from a counter-based generator (the formula is stated at dimx_set_shard:
 * row b*S+s of step t draws counter (t * B*S + b*S + s) * 512 + code, unsharded).
 * n_samples S (1, 2, 4, 5, 8, 10): S independent samples per clip in one pass -- rows b*S+s of tokens /
 * exp_noise / logits_out belong to clip b; the clip's context K/V is streamed once for all S samples (the
 * reference's best-of-10 protocol, code/x_engine_pt.py:257, as one batched generation).  The workspace must
 * come from dimx_workspace_bytes_samples(h, B, T, S).
 * tokens: [B*S,T-1] int32.  logits_out (optional): [B*S,T-1,512] f32 raw logits of every step. */
int dimx_generate(dimx_handle h, const int32_t* start, const uint8_t* ctx_mask, int B, int T, int n_samples,
                  float temperature, int top_k, const float* exp_noise, uint64_t seed, int32_t* tokens,
                  float* logits_out, void* ws, size_t ws_bytes, void* stream);

/* Prompted generation: continue a sequence whose first tokens are given (AutoregressiveWrapper.generate(prompts, seq_len, ...)
 * with a prompt of any length; dimx_generate is the one-token case and shares the implementation).  Variant 0 (SLMFT) only: a
 * handle of variant 1 or 2 returns DIMX_ERR_ARG.
 * Positions are 0 .. T-1; step t consumes the token at position t and produces position t+1.
 *   prompt      [B, ld_prompt] int32, the first Pmax columns are used, 1 <= Pmax <= T-1, one row per CLIP (also with n_samples > 1).
 *               A negative entry (the -100 padding of forward_vq) counts as token 0, as dimx_decode_tf treats it.
 *   prompt_len  [B] int32 device, or NULL = Pmax for every clip.  Clip b's effective length is
 *               plen[b] = clamp(prompt_len[b], P0, Pmax).
 *   P0          host integer, 1 <= P0 <= Pmax: the prefix every clip certainly has (it comes from the host so that no device value
 *               is read back).  Positions 0 .. P0-2 are PREFILLED: the teacher-forced decoder stack runs over them once and
 *               writes every layer's self-attention K/V into the generation cache (no logits are formed).  The first decode step
 *               is t = P0-1 with input prompt[:, P0-1]; from then on a step runs as in dimx_generate, except that while
 *               t+1 < plen[b] the sampler's result of row b is replaced by prompt[b][t+1] (this is what makes ragged prompt
 *               lengths work).  P0 is not part of what keys the captured step graph.
 *   tokens      [B*S, T-1] as in dimx_generate: column c is position c+1; columns < plen-1 hold the prompt's own tokens, the rest
 *               are generated.
 *   logits_out  (optional) [B*S, T-1, 512]: columns < P0-1 are zero-filled by the call (the prefill forms no logits), every later
 *               column holds that step's raw logits.
 *   exp_noise / seed stay indexed by (step, global row): a prompted call draws at step t what dimx_generate draws at step t.
 *   flags       bit 0 = no prefill: the call behaves as if P0 = 1 and forces the whole prompt through decode steps (for the tests
 *               and measurements, like dimx_mesh_head's bit 0; not a tuning knob).
 *               bit 1 = windowed prefill: read only while online generation is on (below) and bit 0 is clear.  Other bits are
 *               reserved.
 * Pmax = P0 = 1 is dimx_generate, bit for bit.  The context must have been built with dimx_encode_ctx(for_generate = 1) in the
 * same ws; dimx_workspace_bytes_prompt(h, B, T, S, P0) sizes ws for both calls (for P0 = 1 it equals
 * dimx_workspace_bytes_samples, and it does not shrink as P0 grows; 0 = shape not supported).  The prefill's teacher-forced scratch
 * is sized for the WHOLE batch, B x (P0-1) rows, behind the generation scratch (no clip chunks); a smaller workspace returns
 * DIMX_ERR_WORKSPACE before anything is launched.  Chain faults are answered as in dimx_generate (below); the regeneration keeps
 * the prefilled cache prefix.
 * Online generation (dimx_set_cross_lookahead, on): without flags bit 1 there is no prefill -- the call behaves as with flags bit 0
 * whatever P0 is, so that every prompt position's cross attention runs under its own key bound; the columns < P0-1 of logits_out
 * then hold logits.  With flags bit 1 the positions 0 .. P0-2 are prefilled as above by a teacher-forced pass whose cross attention
 * carries that bound per query (csrc/win_attn.hip): the same definition through other kernels, so tokens and logits
 * agree with the forced-step form within the decode steps' tolerance, not bit for bit; logits_out and the workspace are those of
 * the offline prefill (columns < P0-1 zero, dimx_workspace_bytes_prompt(h, B, T, S, P0)). */
size_t dimx_workspace_bytes_prompt(dimx_handle h, int B, int T, int n_samples, int P0);
int dimx_generate_prompted(dimx_handle h, const int32_t* prompt, int ld_prompt, const int32_t* prompt_len, int Pmax, int P0,
                           const uint8_t* ctx_mask, int B, int T, int n_samples, float temperature, int top_k,
                           const float* exp_noise, uint64_t seed, int32_t* tokens, float* logits_out, int flags, void* ws,
                           size_t ws_bytes, void* stream);

/* Beam search: the deterministic decoder.  W = beam_width hypotheses per clip (1, 2, 4, 5, 8, 10; 1 is greedy decoding, bit for
 * bit) are extended one position per step; of the W x 512 candidates cum[w] + log softmax(raw logits[w])[v] the W largest survive,
 * in descending order, ties to the smaller w * 512 + v (the definition is dimx/beam.py, float64; csrc/beam.hip).  There is no
 * temperature, filter, noise or seed, no end token and no length penalty.  Variant 0 (SLMFT) only: another variant, and a width
 * outside the set, return DIMX_ERR_ARG.
 * The call mirrors dimx_generate_prompted with beam_width in place of n_samples: rows b*W + w belong to clip b and share its
 * context K/V; prompt / prompt_len / Pmax / P0 / flags bit 0 as there (Pmax = P0 = 1, ld_prompt = 1: prompt is start[B]); the
 * prefill is broadcast to the W rows and ragged prompts finish by forced steps.  Per clip and column c (position c + 1):
 *   c < plen - 1              forced: every hypothesis takes the prompt's token, scores unchanged
 *   c >= lens[b] - 1          frozen: every hypothesis takes its own arg-max, scores unchanged (lens NULL: never) -- the columns
 *                             dimx_op_seq_logprob does not score (dimx.scoring.scored_columns)
 *   otherwise                 live: the selection above; the search starts from scores (0, -inf, ...), so the first live step
 *                             expands hypothesis 0 alone
 * After a live step the self-attention cache rows and the token rows of the clip are permuted by parent hypothesis, so
 *   tokens   [B*W, T-1] int32 holds whole hypotheses, row b*W the best;
 *   scores   [B*W] f64, descending within a clip: the sum of the live columns' log-probabilities;
 *   backptr  (optional) [B*W, T-1] int32: backptr[r][c] = the row (0 .. W-1 within the clip) that ran step c on hypothesis r's path,
 *            -1 in the prefilled columns < P0-1;
 *   logits_out (optional) [B*W, T-1, 512] f32: every step's raw logits in the row order the step ran in (it is NOT permuted: follow
 *            backptr), zero in the prefilled columns.
 *   lens     [B] int32 device or NULL.
 *   beam_state: device memory of at least DIMX_BEAM_STATE_BYTES(B, W) bytes, 8-byte aligned, owned by the call while it runs (running
 *            scores f64 [B*W], then parents int32 [B*W]).  It is the caller's so that the three workspace queries return what they
 *            returned before: ws comes from dimx_workspace_bytes_prompt(h, B, T, W, P0) as for W samples.
 * Chain faults (W = 1, bf16) are answered as in dimx_generate; the regeneration starts the search over. */
#define DIMX_BEAM_STATE_BYTES(B, W) ((size_t)16 * (size_t)(B) * (size_t)(W))
int dimx_generate_beam(dimx_handle h, const int32_t* prompt, int ld_prompt, const int32_t* prompt_len, int Pmax, int P0,
                       const uint8_t* ctx_mask, const int32_t* lens, int B, int T, int beam_width, int32_t* tokens, double* scores,
                       int32_t* backptr, float* logits_out, void* beam_state, size_t beam_state_bytes, int flags, void* ws, size_t ws_bytes,
                       void* stream);

/* Classifier-free guidance: every step samples from g = c + (scale - 1) * (c - u), c the step's raw logits under the clip's context and
 * u those of the same decoder WITHOUT a context (the definition is dimx/guidance.py).  Every cross-attention projection of
 * the decoder is bias-free, so a context of zero rows makes each cross sublayer add exactly 0: the unconditional model is the decoder
 * with its cross sublayers left out.  scale = 1 is dimx_generate's model (g is c bit for bit), scale > 1 makes the listener follow the
 * speaker more closely, scale = 0 samples the listener's prior.  The sampler filter, the temperature and the noise act on g as they act
 * on the raw logits elsewhere; the noise row and the generator counter are those of row b of a B-row generation.
 * One decode step runs 2B rows: rows [0, B) conditional, rows [B, 2B) unconditional and fed the same tokens.  Projections, self
 * attention, feed-forward and logits run at 2B rows, the cross sublayer on rows [0, B) only: the unconditional rows have no cross K/V
 * and no launch reads cross K/V for them.  The step takes the one-kernel-per-op route (no chain or layer kernels); with
 * dimx_set_cross_lookahead on, the conditional rows run under the window.  Call dimx_encode_ctx(for_generate = 1) first with the same
 * B, T and ws; dimx_workspace_bytes_guided(h, B, T) sizes ws for both calls (2B self-attention caches, B cross caches; 0 = shape
 * not supported).
 *   prompt / ld_prompt / prompt_len / Pmax as in dimx_generate_prompted; the whole prompt goes through forced decode steps (P0 = 1;
 *            Pmax = 1, ld_prompt = 1: prompt is start[B]).
 *   tokens   [B, T-1] int32;  logits_out (optional) [B, T-1, 512] f32: every step's GUIDED logits;
 *   branch_logits_out (optional) [2, B, T-1, 512] f32: every step's c, then every step's u.
 * The scale lives in device memory: a call with another scale replays the captured step graphs.  Variant 0 (SLMFT) only, one sample
 * per clip, no beam.  DIMX_ERR_ARG for a NaN or infinite scale, another variant or a bad prompt shape, DIMX_ERR_STATE while a streaming
 * session is open, DIMX_ERR_WORKSPACE for a ws below dimx_workspace_bytes_guided; nothing is enqueued then. */
size_t dimx_workspace_bytes_guided(dimx_handle h, int B, int T);
int dimx_generate_guided(dimx_handle h, const int32_t* prompt, int ld_prompt, const int32_t* prompt_len, int Pmax, const uint8_t* ctx_mask,
                         int B, int T, float scale, float temperature, int top_k, const float* exp_noise, uint64_t seed, int32_t* tokens,
                         float* logits_out, float* branch_logits_out, void* ws, size_t ws_bytes, void* stream);

/* In the bf16 mode dimx_generate runs part of the decode step as XCD-local chain kernels (B <= 256, one sample per clip,
 * 256-CU device) that rely on their 256 blocks being co-resident, one per CU.  They verify that and dimx_generate checks
 * their flags BEFORE it returns: with the chain path active the call therefore waits for its own generation to finish
 * (everything else stays asynchronous); on a fault it regenerates the same batch on the one-kernel-per-op step, keeps the
 * chain path off for this handle and counts the event here (0 = never happened).  The same check covers the deferred
 * LayerNorm's precision guard (a residual row whose |mean| exceeds 8 standard deviations: the batch is regenerated with the
 * row-phase LayerNorm, the deferred form stays off for the handle, the event is counted here too). */
int dimx_chain_faults(dimx_handle h);

/* Sampler filters of AutoregressiveWrapper.generate(filter_logits_fn, filter_kwargs).  All act on the raw logits of a row,
 * p = softmax(logits) over the 512 entries, temperature afterwards; the definition is dimx/sampling.py (float64):
 *   TOP_K  the call's top_k argument (the k-th largest logit and everything tied with it); the state after dimx_create
 *   TOP_P  a = thres: keep i iff the probability mass ranked strictly above i is <= thres (thres >= 1: everything)
 *   MIN_P  a = min_p: keep i iff p_i >= min_p * p_max (min_p = 0: everything)
 *   TOP_A  a = min_p_pow, b = min_p_ratio: keep i iff p_i >= p_max^a * b
 * Equal logits are kept or dropped together and the arg-max always stays. */
typedef enum {
    DIMX_FILTER_TOP_K = 0,
    DIMX_FILTER_TOP_P = 1,
    DIMX_FILTER_MIN_P = 2,
    DIMX_FILTER_TOP_A = 3
} dimx_filter_kind;
/* The filter of this handle's dimx_generate / dimx_generate_prompted calls, until it is set again.  Kind 0: the call's top_k
 * (a, b ignored); the other kinds ignore the call's top_k.  DIMX_ERR_ARG (setting unchanged) for an unknown kind, a NaN,
 * thres < 0, min_p outside [0, 1], min_p_pow or min_p_ratio < 0.  a and b reach the sampler through device memory: another
 * value replays the captured step graph, another kind captures a new one. */
int dimx_set_sampler_filter(dimx_handle h, int kind, float a, float b);

/* Online generation: decode steps see only the speaker frames that exist so far.  Handle state, like the sampler filter; variant
 * 0 (SLMFT) only, a handle of variant 1 or 2 returns DIMX_ERR_ARG.  With on != 0, step t of clip b (it consumes the token at
 * position t and produces position t+1, as in dimx_generate_prompted) attends in every layer's CROSS attention over the context rows
 *     j < vis(t) = clamp(t + 2 + lookahead, 1, T)        (and ctx_mask[b][j] != 0, as always)
 * lookahead = 0: the frame being produced and everything before it; < 0: a reaction delay of -lookahead frames; > 0: a buffer of
 * look-ahead frames; lookahead >= T-2 computes what on = 0 computes.  Row 0 is always visible.  Past positions are not
 * recomputed: the self-attention K/V a step cached under its own visibility stay, which is what a running system has (it equals a
 * decoder whose cross attention carries the per-query mask j < vis(i)).  The speaker encoder is causal already, so the context rows
 * below a frame do not depend on that frame: the tokens of dimx_generate / dimx_generate_prompted (any n_samples) are causal in the
 * speaker.  The definition is dimx/online.py.
 *   - on = 0 restores the offline behaviour bit for bit.  on and lookahead are part of what keys the captured step graph: a new
 *     value captures a new graph, never replays another one's.
 *   - With the window on the decode step runs the one-query attention kernels (csrc/decode_attn.hip) for every cross attention:
 *     not the decoder-layer kernel and not the matrix-core multi-sample route, which have no windowed form.
 *   - dimx_generate_prompted forces the whole prompt through decode steps, as its flags bit 0 does (the offline prefill's attention
 *     has no per-query key bound; dimx_workspace_bytes_prompt(h, B, T, S, 1) suffices), unless its flags bit 1 asks for the windowed
 *     prefill.
 *   - dimx_generate_beam returns DIMX_ERR_ARG while the window is on.
 *   - dimx_decode_tf is unaffected: the teacher-forced pass always sees the whole context (dimx_decode_tf_win is the bounded one). */
int dimx_set_cross_lookahead(dimx_handle h, int on, int lookahead);
/* The handle's current setting (either pointer may be NULL). */
int dimx_cross_lookahead(dimx_handle h, int* on, int* lookahead);
/* FP8 cross-attention K/V for generation (csrc/decode_attn_kv8.hip; the definition is dimx/kv8.py).  Opt-in handle state, like the
 * cross-attention window; variant 0 only (DIMX_ERR_ARG otherwise), either numeric mode; DIMX_ERR_STATE while a streaming session is
 * open (sessions neither read nor change the setting: dimx_stream_set_kv8 is theirs).  With a buffer set, dimx_generate / dimx_generate_prompted /
 * dimx_generate_guided quantise every layer's context K / V once, ahead of the first decode step, into OCP e4m3fn codes with one f32
 * scale per (clip, head, key), and every decode step's cross attention streams the codes instead of the caches: half the bytes of
 * the bf16 caches, a quarter of the f32 ones.
 *   - The buffer is the caller's: dimx_cross_kv8_bytes(h, B, T) bytes of device memory, 256-byte aligned; the workspace queries
 *     return what they returned before (the unquantised caches stay: a prompt's prefill, offline or windowed, reads them).
 *     Layout, with Tp = (T + 7) / 8 * 8, H and depth the decoder's heads and layers, every block rounded up to 256 bytes:
 *         layer 0: K codes [B, H, Tp, 64] uint8 | V codes [B, H, Tp, 64] uint8 | K scales [B, H, Tp] f32 | V scales [B, H, Tp] f32
 *         layer 1: the same, ... layer depth - 1.
 *     Rows t >= T of a (clip, head) are never written and never read.  0 = the shape is not supported.
 *   - buf = NULL turns it off: every call then launches what it launched before the setting existed, bit for bit.  The pointer is
 *     part of what keys the captured step graph.
 *   - The decoder-layer kernel is not taken (as under the window); the chain route and the per-op route stay.  With the window on
 *     the kv8 cross attention is the windowed one.  In a guided step it runs over the conditional rows only.  The regeneration after
 *     a chain fault keeps the setting and reuses the codes.
 *   - n_samples > 1 (without dimx_set_cross_kv8_samples) and dimx_generate_beam (without dimx_set_beam_kv8) return DIMX_ERR_ARG before any launch; a buffer below dimx_cross_kv8_bytes(h, B, T) for
 *     the call's shape returns DIMX_ERR_WORKSPACE. */
size_t dimx_cross_kv8_bytes(dimx_handle h, int B, int T);
int dimx_set_cross_kv8(dimx_handle h, void* buf, size_t bytes);
/* The handle's current setting (either pointer may be NULL). */
int dimx_cross_kv8(dimx_handle h, void** buf, size_t* bytes);
/* FP8 cross K/V for best-of-N generation (csrc/decode_attn_kv8.hip, decode_attn_mq_kv8_kernel; the definition is dimx/kv8.py
 * attention_rows).  A separate opt-in on top of dimx_set_cross_kv8: handle state of variant 0 (DIMX_ERR_ARG otherwise),
 * default off, DIMX_ERR_STATE while a streaming session is open, part of what keys the captured step graph.  With on != 0 and a cross
 * buffer set, dimx_generate / dimx_generate_prompted take n_samples in {2, 4, 5, 8, 10}: the quantiser pass is unchanged (one row per
 * clip; dimx_cross_kv8_bytes(h, B, T) is unchanged), and the cross attention of every layer is dimx_op_decode_attn_kv8_multi -- the S
 * queries of a clip against that clip's codes, read once for all S -- in its matrix-core form on a bf16 handle (q from a plain bf16
 * projection) and in its exact form on an f32 handle (q as f32 split-K slabs); windowed when the cross-attention window is on (q as
 * slabs in both modes).  Works with dimx_set_self_kv8, the sampler filters, prompts (the prefill reads the unquantised caches),
 * logits_out and the score dumps.  dimx_generate_beam and dimx_generate_guided stay DIMX_ERR_ARG.  With on = 0 every call launches
 * what it launched before the setting existed, refusals included. */
int dimx_set_cross_kv8_samples(dimx_handle h, int on);
/* The handle's current setting. */
int dimx_cross_kv8_samples(dimx_handle h, int* on);
/* FP8 self-attention K/V caches for generation (csrc/decode_attn_kv8.hip, decode_attn_self_kv8_kernel; the definition is dimx/kv8.py
 * self_step).  Opt-in handle state like dimx_set_cross_kv8: variant 0 only (DIMX_ERR_ARG otherwise), either numeric mode,
 * DIMX_ERR_STATE while a streaming session is open (sessions neither read nor change the setting: dimx_stream_set_kv8 is theirs).  With a buffer set, every decode
 * step of dimx_generate / dimx_generate_prompted quantises its k / v row -- the f32 sum of the projection's split-K slabs, never rounded
 * to the cache type -- into OCP e4m3fn codes with one f32 scale per (row, head, position), stores it at the step's position and
 * attends over the codes of the positions so far, its own included: one launch per layer and step.  The output of step t is a
 * function of the buffer's rows <= t alone.
 *   - The buffer is the caller's: dimx_self_kv8_bytes(h, R, T) bytes of device memory, 256-byte aligned, R = B * n_samples
 *     sequences; the layout is dimx_set_cross_kv8's with R in place of B.  The workspace queries return what they returned before
 *     (the unquantised self caches stay allocated: a prompt's prefill writes them).  Positions a generation has not reached are
 *     neither read nor written.  0 = the shape is not supported.
 *   - buf = NULL turns it off: every call then launches what it launched before the setting existed, bit for bit.  The pointer is
 *     part of what keys the captured step graph.
 *   - Any n_samples; rows are samples, and with n_samples > 1 the cross attention stays the unquantised multi-query launch.  The
 *     decoder-layer kernel is not taken.  The first layer keeps its table form where the route has it (that layer has no cache).
 *     Works with the cross-attention window, the sampler filters, logits_out and prompts; a prefilled prompt's rows 0 .. P0 - 2 are
 *     quantised from the caches the prefill wrote, one dimx_op_kv8_quantize launch per layer and operand, ahead of the first step.
 *     Combines with dimx_set_cross_kv8 at one sample per clip.
 *   - dimx_generate_beam (without dimx_set_beam_kv8) and dimx_generate_guided return DIMX_ERR_ARG before any launch; a buffer below
 *     dimx_self_kv8_bytes(h, B * n_samples, T) for the call's shape returns DIMX_ERR_WORKSPACE. */
size_t dimx_self_kv8_bytes(dimx_handle h, int R, int T);
int dimx_set_self_kv8(dimx_handle h, void* buf, size_t bytes);
/* The handle's current setting (either pointer may be NULL). */
int dimx_self_kv8(dimx_handle h, void** buf, size_t* bytes);
/* FP8 K/V caches for beam search (csrc/beam.hip, beam_reorder_kv8_kernel; the definition is dimx/kv8.py reorder on top of dimx/beam.py
 * and self_step).  A separate opt-in on top of dimx_set_cross_kv8 / dimx_set_self_kv8: handle state of variant 0
 * (DIMX_ERR_ARG otherwise), default off, DIMX_ERR_STATE while a streaming session is open (sessions do not read it).  With on = 0
 * dimx_generate_beam refuses a handle with either buffer set, exactly as before the setting existed.  With on != 0:
 *   - a self buffer of dimx_self_kv8_bytes(h, B * beam_width, T) bytes: every layer's self attention of every beam step appends to
 *     and reads the codes (beam search has no table form of layer 0), a prefilled prompt's rows are quantised once over the B * W
 *     rows, and the step ends in ONE launch that permutes, by parent hypothesis, positions 0 .. c of every layer's K codes, V
 *     codes, K scales and V scales (codes and scale of a position move together: a pure permutation, so the rows a hypothesis reads
 *     afterwards are its ancestor's, bit for bit) and the token / back-pointer columns < c.  The unquantised self caches are not
 *     reordered: nothing reads them after the prefill's quantisation.
 *   - a cross buffer of dimx_cross_kv8_bytes(h, B, T) bytes: the W hypotheses of a clip read that clip's codes through the
 *     multi-query launch of dimx_set_cross_kv8_samples (beam_width = 1: the one-query launch); the cross K/V is never reordered.
 *   - either buffer alone is valid; with neither the call is the plain one, launch for launch.  The workspace queries are unchanged.
 * dimx_generate / dimx_generate_prompted / dimx_generate_guided do not read the setting.  Part of what keys the captured step graph. */
int dimx_set_beam_kv8(dimx_handle h, int on);
/* The handle's current setting. */
int dimx_beam_kv8(dimx_handle h, int* on);
/* Streaming sessions (csrc/stream.hip; the schedule is dimx/stream.py): the speaker arrives in pieces, the listener's
 * tokens leave as soon as they are due.  A session fed a clip in pieces computes what dimx_encode_ctx + dimx_generate under
 * dimx_set_cross_lookahead(1, lookahead) compute on the whole clip: the speaker encoders are causal, so the context rows of the new
 * frames are computed from those frames and per-layer K / V caches alone (dimx_op_append_attn), and decode step t (it produces
 * listener position t + 1) runs as soon as the frames 0 .. t + 1 + max(lookahead, 0) exist.  Variant 0, one sample per clip, the B
 * clips in lockstep, every pushed frame valid.  One open session per handle.
 *   dimx_stream_workspace_bytes: bytes of the session's workspace (a dimx_generate workspace for (B, Tmax), the encoder caches, the
 *     token and logit rows of all Tmax - 1 steps, the scratch of a 16-row encoder increment); 0 for an unsupported shape
 *     (variant != 0, B < 1, Tmax outside [2, min(2048, max_seq_len)]).  The caller need not initialise it.
 *   dimx_stream_begin: start [B] int32 (device; copied), noise [Tmax-1, B, 512] or NULL and the sampler arguments as dimx_generate
 *     takes them (the handle's sampler filter applies; dimx_set_cross_lookahead's setting is neither read nor changed).  ws stays
 *     the session's until it closes.  DIMX_ERR_STATE when a session is open, DIMX_ERR_ARG for a handle of variant 1 / 2 or a shape
 *     outside the ranges above, DIMX_ERR_WORKSPACE for too small a workspace; nothing is launched in those cases.
 *   dimx_stream_push: c >= 1 new frames of every clip, v_speaker [B, c, 56], v_audio [B, c, 768] (device f32).  Runs the encoder
 *     increment (launches of at most 16 rows per clip), appends the cross K / V rows, runs the steps now due.  The new tokens land
 *     in columns [done, done + *n_new) of tokens_out [B, ld_tok] (done = the steps run before the call), their logits, when
 *     logits_out is given, in the same columns of logits_out [B, ld_tok, 512]; x_s_out, when given, receives the c new encoder
 *     rows [B, c, 384] (the rows dimx_encode_ctx returns).  DIMX_ERR_STATE without an open session (before begin, after end);
 *     DIMX_ERR_ARG for c < 1, frames past Tmax, a null argument or ld_tok below the columns written; nothing is launched then and
 *     the session stays as it was.
 *   dimx_stream_end: T := the frames pushed (>= 2, else DIMX_ERR_ARG and the session stays open); runs the remaining steps up to
 *     T - 1 with the key bound T and closes the session.
 *   dimx_stream_abort: closes the session, if any, without running anything.
 *   dimx_stream_state: frames pushed, steps run, open (0 / 1); any pointer may be NULL; zeros without a session.
 *   dimx_stream_begin_prompted: a session whose first F frames (v_speaker [B, F, 56], v_audio [B, F, 768]) and first P listener codes
 *     (prompt [B, ld_prompt] int32, copied) are given -- the state a session with lookahead L >= 0 is in after F frames with its
 *     F - L codes, so a conversation that outlasts Tmax carries the last K frames and their K - max(L, 0) codes into a new session.
 *     It runs the encoder increments and the K / V append of a push of F frames, one windowed prefill (dimx_generate_prompted's flags
 *     bit 1) over the positions 0 .. P - 2 and sets the step counter to P - 1; no token is produced by the call: steps the F frames
 *     make due beyond P - 1 run with the next push or end, whose token columns start at P - 1 (the columns below repeat the prompt
 *     for the caller to fill; their logits are not formed).  Needs 1 <= P, P + max(lookahead, 0) <= F <= Tmax and ld_prompt >= P --
 *     teacher-forced row P - 2 reads the keys below P + lookahead, and they must exist -- DIMX_ERR_ARG otherwise, the other
 *     refusals as dimx_stream_begin, nothing launched.  P = 1 is dimx_stream_begin followed by a push of F frames.  What the session
 *     emits is dimx_generate_prompted(prompt, Pmax = P0 = P, flags bit 1) under the lookahead on the clip of the frames given plus
 *     the frames pushed.  ws comes from dimx_stream_workspace_bytes_prompt (the session workspace with the prefill scratch for
 *     Tmax - 1 positions in its generate part); one P for all clips.
 * While a session is open dimx_encode_ctx, dimx_set_context, dimx_generate, dimx_generate_prompted, dimx_generate_beam, dimx_decode_tf
 * and dimx_set_cross_lookahead return DIMX_ERR_STATE; the VQ stages and the dimx_op_* calls stay usable.  The steps run on the
 * one-kernel-per-op route without the captured step graphs: the chain kernels answer a placement fault by regenerating the whole
 * call, which a session cannot offer.  All calls of a session go to one stream (or are ordered by the caller). */
size_t dimx_stream_workspace_bytes(dimx_handle h, int B, int Tmax);
int dimx_stream_begin(dimx_handle h, const int32_t* start, int B, int Tmax, int lookahead, float temperature, int top_k, const float* noise,
                      uint64_t seed, void* ws, size_t ws_bytes, void* stream);
size_t dimx_stream_workspace_bytes_prompt(dimx_handle h, int B, int Tmax);
int dimx_stream_begin_prompted(dimx_handle h, const int32_t* prompt, int ld_prompt, int P, const float* v_speaker, const float* v_audio, int F,
                               int B, int Tmax, int lookahead, float temperature, int top_k, const float* noise, uint64_t seed, void* ws,
                               size_t ws_bytes, void* stream);
int dimx_stream_push(dimx_handle h, const float* v_speaker, const float* v_audio, int c, int32_t* tokens_out, int ld_tok, float* logits_out,
                     float* x_s_out, int* n_new, void* stream);
int dimx_stream_end(dimx_handle h, int32_t* tokens_out, int ld_tok, float* logits_out, int* n_new, void* stream);
int dimx_stream_abort(dimx_handle h);
int dimx_stream_state(dimx_handle h, int* frames, int* steps, int* open);
/* Measurement (tools/bench_stream.py): four hipEvent_t of the caller's (any may be NULL) that every later push of the open session
 * records on its stream -- at its start, after the encoder increment, after the cross K / V append, after the decode steps and the
 * copy of their tokens.  A push of more than 16 frames interleaves the first two parts per launch group; the second event is then
 * the last group's.  The events must outlive the session or be replaced by NULL.  DIMX_ERR_STATE without an open session. */
int dimx_stream_set_events(dimx_handle h, void* ev_start, void* ev_encoded, void* ev_appended, void* ev_stepped);
/* FP8 K/V for streaming sessions (the definition is dimx/kv8.py, append and self_step).  Opt-in handle state that session
 * begins alone read: the next dimx_stream_begin / dimx_stream_begin_prompted takes cross_buf as the session's FP8 cross K/V buffer
 * and self_buf as its FP8 self K/V buffer; either may be NULL (that route off), both NULL is a plain session, which launches what
 * it launched before the setting existed.  Independent of dimx_set_cross_kv8 / dimx_set_self_kv8: sessions keep ignoring those two,
 * dimx_generate* ignores this one.  Variant 0 only and 256-byte aligned buffers (DIMX_ERR_ARG otherwise); DIMX_ERR_STATE while a
 * session is open.
 *   - The buffers are the caller's, of dimx_cross_kv8_bytes(h, B, Tmax) and dimx_self_kv8_bytes(h, B, Tmax) bytes, in
 *     dimx_set_cross_kv8's layout with Tp = (Tmax + 7) / 8 * 8.  A begin checks them against its (B, Tmax) before it launches
 *     anything: a shape the size query answers with 0 is DIMX_ERR_ARG, too small a buffer DIMX_ERR_WORKSPACE; no session opens.
 *     dimx_stream_workspace_bytes returns what it returned before (the unquantised caches stay: the windowed prefill reads them).
 *   - Cross: every push (and the F given frames of dimx_stream_begin_prompted) quantises the cross K / V rows it appended, K and V of
 *     all layers in one dimx_op_kv8_append launch ahead of the `ev_appended` event, and every decode step's cross attention is the
 *     windowed dimx_op_decode_attn_kv8.  A row's codes and scale are a function of that row alone, so the buffer's rows below the
 *     frames pushed are what dimx_op_kv8_quantize gives on the session's finished caches, whatever the chunking; rows at or past the
 *     frames pushed are neither read nor written.
 *   - Self: every decode step is dimx_op_decode_attn_self_kv8, as under dimx_set_self_kv8 (the first layer keeps its table form);
 *     the rows 0 .. P - 2 a prompted begin's prefill stored are quantised ahead of the first step.
 *   - dimx_stream_end / dimx_stream_abort leave the buffers and the setting as they are.
 * dimx_stream_kv8 reads the setting back (any pointer may be NULL). */
int dimx_stream_set_kv8(dimx_handle h, void* cross_buf, size_t cross_bytes, void* self_buf, size_t self_bytes);
int dimx_stream_kv8(dimx_handle h, void** cross_buf, size_t* cross_bytes, void** self_buf, size_t* self_bytes);
/* The open session's unquantised cross K / V caches of decoder layer `layer`: device pointers into its workspace, [B, H, Tp, 64] in
 * the operand type, rows below the frames pushed valid (tests compare the FP8 buffer with them).  Either pointer may be NULL;
 * DIMX_ERR_STATE without an open session. */
int dimx_stream_cross_kv(dimx_handle h, int layer, void** k, void** v);
/* Decoders without positional embedding (variant 0): the first layer's q/k/v depend on the input token alone, so dimx_generate
 * reads them from a table over the token ids instead of projecting them at every step.  The table is built with the decode
 * step's own kernels (bit-identical rows) on first use and whenever the rows per call, the numeric mode or the decoder weights
 * changed; this counts the builds of a handle (0 = the table is not in use: other variants, several generation groups, or
 * DIMX_NO_QKV0_TABLE=1 in the environment at dimx_create). */
int dimx_qkv0_table_builds(dimx_handle h);
/* The same fact makes that layer's K/V cache redundant: the cached K / V of a position are columns of the table row of the
 * position's input token.  With the table in use, generations without beam search and without a prompt read those rows through
 * a per-row token history instead of appending to and streaming the layer's cache (same bits); this counts the generations of a
 * handle that did (0 = the cache: see above, or DIMX_NO_KV0_TABLE=1 in the environment at dimx_create). */
int dimx_kv0_table_generations(dimx_handle h);
/* And the sampler a launch of its own: the consumer of a row's token is the CU that runs the row's first-layer attention.  On
 * the bf16 chain route -- the table form above in the decoder-layer kernel, the top-k filter, one sample per clip in one group,
 * no beam search, guidance or prompt, no to_logits.bias -- the first layer's launch samples the previous step's logits itself
 * (same tokens and logits), a step is one launch shorter and one plain sampler launch ends the call; this counts the
 * generations of a handle that ran so (0 = the sampler launch: see above, or DIMX_NO_SAMPLE_HEAD=1 at dimx_create). */
int dimx_sample_head_generations(dimx_handle h);
/* Test hook: the next n_calls dimx_generate calls launch their chain kernels with a deliberately non-bijective
 * (XCD, CU slot) placement (the blocks of every odd XCD claim the slots of its even neighbour). */
int dimx_debug_chain_fault(dimx_handle h, int n_calls);

/* ---- DIM-Speaker mesh head (handle of variant 2 created with dimx_dims.mesh_dim = V > 0) ---------------------------------------
 * SpeakerSLMFT (reference code/seq2seq_pretrain.py:516-757) is the variant-2 transformer (dimx_set_context(which_patch = 1) +
 * dimx_decode_tf(kv_mask = NULL) / dimx_generate) plus the converter head of EmocaConverter (:801-819, applied at :671-672 and
 * :834-836).  dimx_mesh_head runs that head: mesh_out [B,L,V] f32 =
 *   Linear(768 -> V)(LeakyReLU_0.2(Linear(768 -> 768)(LSTM_2layers_bidirectional(motion [B,L,56])))) + template[b]
 * with template [B,V] f32 or NULL (row b is added to every frame of clip b, in the last GEMM's epilogue; ldc = V, nothing is
 * written past mesh_out).  Like the reference the LSTM has NO per-clip lengths: it runs over all L frames of every clip, and
 * the reverse direction starts at the last (padded) frame.  The recurrence is f32 in both numeric modes (csrc/lstm.hip); the two
 * Linear layers use the mode's operands.  flags bit 0: run the LSTM layers on the safe path (one block per 4 clips and direction,
 * no communication between blocks).  Otherwise, on a 256-CU device, they run on the group path, whose 256 blocks wait for each
 * other: the call then WAITS for each LSTM layer on the host, reads its fault word, and after a fault (a bounded wait timed out)
 * reruns the layer on the safe path and counts the event (dimx_lstm_faults; 0 = never happened); because of that wait a stream
 * that is being captured must take flags bit 0.  Extra state-dict keys:
 * vertice_map_reverse_lstm.{weight_ih,weight_hh,bias_ih,bias_hh}_l{0,1}[_reverse] and vertice_map_reverse.{0,2}.{weight,bias}
 * are required by such a handle; vertice_mapping.*, squasher.*, vertice_map_reverse_lstm_2.*, vertice_map_reverse2.*, W and
 * speaker_embed.weight (never applied by the reference's forward, or applied on the host) are accepted and ignored by every handle. */
int dimx_mesh_head(dimx_handle h, const float* motion, const float* templ, int B, int L, float* mesh_out, int flags, void* ws,
                   size_t ws_bytes, void* stream);
int dimx_lstm_faults(dimx_handle h);

/* ---- training step: reference train_epoch, code/x_engine_pt.py:9-60 driven by
 * code/finetune_s2s_pretrain.py:105-143 (AdamW lr 1e-5, clip 1.0, VQ-VAEs frozen) --------------------------------------------
 * The reference differentiates SLMFT.forward(mode='train') with autograd; here forward AND backward of the teacher-forced stack
 * (encoder_s -> encoder_joint -> norm_s -> context -> decoder -> cross entropy, code/seq2seq_pretrain.py:431-450,496-514) are
 * hand-written HIP kernels (csrc/train.hip, train_kernels.hip; every Linear and both of its adjoints on the library's GEMM).
 * Parameters, gradients and the AdamW moments are FLAT f32 device arenas owned by the caller, laid out as reported by
 * dimx_train_param_info (the trainable tensors this path reaches; unused reference parameters -- encoder_l.*, norm_l.*,
 * project_out, ... -- get no gradient from autograd either and are not in the arena).  The handle must have been given the
 * full state dict (dimx_load_weights); its numeric mode selects the GEMM operands (f32-exact or bf16 with f32 accumulation). */
int dimx_train_num_params(dimx_handle h);
int64_t dimx_train_total(dimx_handle h);   /* floats in an arena (tensors are 16-byte aligned inside it) */
int dimx_train_param_info(dimx_handle h, int i, const char** name, int64_t* offset, int64_t* numel);
size_t dimx_train_workspace_bytes(dimx_handle h, int B, int T);
/* One forward + backward pass.  params / grads: arenas (grads is overwritten); v_speaker [B,T,56], v_audio [B,T,768] f32;
 * mask [B,T] uint8 (1 = valid frame); z_l [B,T] int32 listener codes, -100 on padding (from dimx_vq_encode); kv_mask [B,T-1]
 * uint8 keep-mask of AutoregressiveWrapper's mask_prob draw (NULL = keep all).  loss_out: 2 device floats {mean cross
 * entropy over the valid targets, 1 / number of valid targets}; logits_out optional [B,T-1,512] f32. */
int dimx_train_forward_backward(dimx_handle h, const float* params, float* grads, const float* v_speaker, const float* v_audio,
                                const uint8_t* mask, const int32_t* z_l, const uint8_t* kv_mask, int B, int T, float* loss_out,
                                float* logits_out, void* ws, size_t ws_bytes, void* stream);
/* How this handle's training steps were launched: out3 = {steps replayed from the captured hipGraph, steps launched kernel by
 * kernel, nodes of the captured graph}.  Below 4 096 rows (B x T) a call whose arguments (every pointer, B, T) equal the
 * previous call's is captured once and replayed afterwards; from 4 096 rows up the step is launched kernel by kernel with its
 * weight-gradient GEMMs on a side stream (the faster choice there: csrc/train.hip).  DIMX_TRAIN_GRAPH=0|1 / DIMX_TRAIN_SIDE=0|1
 * force either; results are bit-identical in every combination. */
int dimx_train_graph_stats(dimx_handle h, int64_t* out3);
/* Online fine-tuning: train under the visibility an online generation runs with (dimx_set_cross_lookahead; the definition is
 * dimx/online.py).  With on != 0, dimx_train_forward_backward masks the decoder's cross attention, in every layer, forward and
 * both adjoints, in both numeric modes and on both launch paths: query row i (it consumes token i and predicts token i + 1, so
 * it is generation step t = i) keeps context row j iff j < clamp(i + 2 + lookahead, 1, T) and mask keeps j.  loss_out /
 * logits_out are the windowed model's.
 *   - Row 0 is always inside the window; lookahead >= T - 2 is the offline form, bit for bit; any int is accepted.
 *   - A query whose every in-window row is dropped by mask is outside the contract.  The step never produces one for a clip with
 *     at least one valid frame (valid frames are a prefix, so row 0 is valid).
 *   - Handle state of variant 0 only (DIMX_ERR_ARG on a handle of variant 1 or 2); on = 0 resets lookahead to 0.  on and
 *     lookahead key the captured step graph: a step captured under one setting is never replayed under another.
 *   - Independent of dimx_set_cross_lookahead: generation and dimx_decode_tf do not read this setting, the step does not read
 *     that one.  The legacy, SLM, VQ-VAE, converter and speaker steps do not take it. */
int dimx_set_train_lookahead(dimx_handle h, int on, int lookahead);
/* The handle's current setting (either pointer may be NULL). */
int dimx_train_lookahead(dimx_handle h, int* on, int* lookahead);
/* Condition dropout (classifier-free guidance's training side; the definition is dimx/guidance.py): keep_dev [B] uint8 in device
 * memory, NULL = off.  With a vector set, dimx_train_forward_backward trains clip b under the null context where keep_dev[b] == 0:
 * its context rows are zeroed after the concat [x_s + patch_embed_dec_s | audio], before the cross K / V projections, and its rows
 * of the context gradient are zeroed before they reach patch_embed_dec_s and the encoders.  A kept clip is unchanged: there is no
 * rescaling, and a vector of ones gives the plain step bit for bit.
 *   - The pointer is handle state of variant 0 only (DIMX_ERR_ARG on a handle of variant 1 or 2) and keys the captured step graph;
 *     its CONTENTS are read on the device by the step, so a new draw in the same buffer replays the graph.  The buffer must hold B
 *     entries of the steps that follow and stay valid while it is set.
 *   - Both numeric modes and both launch paths.  The legacy, SLM, VQ-VAE, converter and speaker steps do not take it. */
int dimx_set_train_cond_keep(dimx_handle h, const uint8_t* keep_dev);
/* The handle's current vector (NULL while off). */
int dimx_train_cond_keep(dimx_handle h, const uint8_t** keep_dev);
/* The legacy generator's training step (reference loop code/x_engine.py:8-36 over ListenerGenerator.forward,
 * code/seq2seq.py:235-278): handle of variant 1.  The arenas follow dimx_train_param_info of that handle: generator.*, the
 * listener VQ-VAE's DECODER (listener_vq.decoder.*) and the listener-id conditioning (listener_embeddings.weight [100,256],
 * fc_listener.*) -- what the reference trains on this call (code/seq2seq.py:165-176; speaker_ids is None in the loop).
 * x_speaker [B,T,1024]: features of the frozen speaker VQ-VAE (dimx_legacy_speaker_features); z_l [B,T] listener codes, -100 on
 * padding; v_listener [B,T,56]; mask [B,T]; listener_ids [B] int32 or NULL; codebook [512,128] and pe [>=B rows of 384] are the
 * listener VQ-VAE's frozen codebook and its decoder's positional buffer (device pointers of the module's tensors).
 * loss_out: 4 device floats {cross entropy, 1 / valid targets, continuous loss, 1 / selected rows}; pred_out optional
 * [B,T-1,56]; logits_out optional [B,T (with ids) or T-1,512]. */
size_t dimx_train_legacy_workspace_bytes(dimx_handle h, int B, int T);
int dimx_train_legacy_forward_backward(dimx_handle h, const float* params, float* grads, const float* x_speaker, const int32_t* z_l,
                                       const float* v_listener, const uint8_t* mask, const int32_t* listener_ids, const float* codebook,
                                       const float* pe, int B, int T, float* loss_out, float* pred_out, float* logits_out, void* ws,
                                       size_t ws_bytes, void* stream);
/* The SLM pre-training step (reference loop code/train_s2s_pretrain.py:41-64 -> x_engine_pt.train_epoch over
 * SLM.forward, code/seq2seq_pretrain.py:300-323): handle of variant 2.  The arenas follow dimx_train_param_info of that handle:
 * everything the reference trains there (:98-113) -- the patch embeddings, norm / norm_s / norm_l, encoder_s / encoder_l /
 * encoder_joint, decoder_joint (with its absolute positional table) and BOTH VQ-VAE decoders; the VQ encoders and codebooks are
 * frozen.  v_speaker / v_listener [B,T,56], v_audio [B,T,768] f32; mask [B,T] uint8 (1 = valid frame); mask_speaker /
 * mask_listener [B,T] uint8 (1 = frame masked out: random_masking_unstructured, :170-183); z_s / z_l [B,T] int32 codes of the
 * frozen VQ encoders (dimx_vq_encode); codebook_* [512,128] and pe_* [>= B rows of 384]: the VQ-VAEs' frozen codebooks and their
 * decoders' positional buffers.  2T <= max_seq_len.  loss_out: 10 device floats {l_ce_s, 1 / targets, l_ce_l, 1 / targets,
 * l_cont_s, 1 / rows, l_cont_l, 1 / rows, nce, c_acc}; the reference's total is [0] + [2] + [4] + [6] + [8]. */
size_t dimx_train_slm_workspace_bytes(dimx_handle h, int B, int T);
int dimx_train_slm_forward_backward(dimx_handle h, const float* params, float* grads, const float* v_speaker, const float* v_listener,
                                    const float* v_audio, const uint8_t* mask, const uint8_t* mask_speaker, const uint8_t* mask_listener,
                                    const int32_t* z_s, const int32_t* z_l, const float* codebook_s, const float* codebook_l,
                                    const float* pe_s, const float* pe_l, int B, int T, float* loss_out, void* ws, size_t ws_bytes,
                                    void* stream);
/* The VQ-VAE's own training step (stage 1; reference loop code/train_vq.py:173-196 over VQAutoEncoder.forward,
 * code/models/stage1_BIWI.py:10-137, and calc_vq_loss, code/metrics/loss.py:6-11).  Slot `which` of the handle: 0 = speaker_vq.,
 * 1 = listener_vq. (VQAutoEncoder(which=...)); only the 56 / 384 / 8 x 48 / 128 geometry is built (anything else, e.g. the
 * legacy 824-d speaker VQ-VAE: DIMX_ERR_ARG).  The arenas follow dimx_train_vq_param_info: every parameter of the slot --
 * <prefix>encoder.*, <prefix>decoder.*, <prefix>quantize.embedding.weight (the pe buffers are not parameters; the step reads
 * them from the loaded weights).  AdamW: dimx_train_adamw over the same arenas. */
int dimx_train_vq_num_params(dimx_handle h, int which);
int64_t dimx_train_vq_total(dimx_handle h, int which);   /* floats in an arena (tensors are 16-byte aligned inside it) */
int dimx_train_vq_param_info(dimx_handle h, int which, int i, const char** name, int64_t* offset, int64_t* numel);
size_t dimx_train_vq_workspace_bytes(dimx_handle h, int B, int T);
/* One forward + backward pass over x [B,T,56] f32 (B clips of one length T, no padding): encoder -> z, idx = the inference argmin
 * (dimx_vq_encode's kernel and summation order, over the arena's codebook), straight-through latent z + sg(e - z), decoder, L1
 * reconstruction; loss = quant_loss_weight * quant_loss + rec, quant_loss = beta mean(sg(e) - z)^2 + mean(e - sg(z))^2.  grads
 * is overwritten.  dropout_p: the Dropout after each positional encoding (0.1 in the reference's train mode, 0 = none); its keep
 * mask is a counter-based function of (dropout_seed, step, site 0 = encoder / 1 = decoder, b, t, c), restated by
 * dimx.prng.dropout_keep.  loss_out: 4 device floats {loss, rec_loss, quant_loss, perplexity}; pred_out optional [B,T,56];
 * idx_out optional [B*T] int32.  Deterministic: a rerun is bit-identical. */
int dimx_train_vq_forward_backward(dimx_handle h, int which, const float* params, float* grads, const float* x, int B, int T, float beta,
                                   float quant_loss_weight, float dropout_p, uint64_t dropout_seed, int64_t step, float* loss_out,
                                   float* pred_out, int32_t* idx_out, void* ws, size_t ws_bytes, void* stream);
/* ---- DIM-Speaker converter training step: reference EmocaConverter (code/seq2seq_pretrain.py:759-842) under the loop of
 * code/train_converter.py:17-96.  What trains is the head of dimx_mesh_head -- the 2-layer bidirectional LSTM(384),
 * Linear(768,768), LeakyReLU(0.2), Linear(768,V) -- 20 tensors under their state-dict names
 * vertice_map_reverse_lstm.{weight_ih,weight_hh,bias_ih,bias_hh}_l{0,1}[_reverse] and vertice_map_reverse.{0,2}.{weight,bias}, in
 * flat f32 arenas (tensors 16-byte aligned) as for the other steps.  The handle must be a speaker handle with mesh_dim > 0
 * (DIMX_ERR_STATE otherwise).  The frozen speaker VQ-VAE is NOT part of the call: motion is its output (dimx_vq_encode /
 * dimx_vq_decode), as EmocaConverter.forward computes it. */
int dimx_train_conv_num_params(dimx_handle h);
int64_t dimx_train_conv_total(dimx_handle h);
int dimx_train_conv_param_info(dimx_handle h, int i, const char** name, int64_t* offset, int64_t* numel);
size_t dimx_train_conv_workspace_bytes(dimx_handle h, int B, int T);
/* One forward + loss + backward pass.  motion [B,T,56], templ [B,V] or NULL, target [B,T,V], all f32.
 *   mesh = head(motion) + templ;  loss = mse(mesh, target) + 5 mse over the mouth vertices
 * vert_w [V/3] f32 or NULL: entry v = how often vertex v occurs in the mouth map (duplicates count, as the reference's fancy
 * indexing counts them), n_mouth = the length of that map; NULL = no mouth term.  The mean runs over all B clips (the reference
 * is written for B = 1, where the two agree).  loss_out: 3 device floats {total, full-mesh mse, mouth mse}.  grads == NULL:
 * forward and loss only (the reference's evaluate_epoch).  mesh_out optional [B,T,V]; in the f32 mode it equals
 * dimx_mesh_head's result on the same path bit for bit.  flags bit 0 = the safe LSTM path (see dimx_mesh_head).  The LSTM
 * recurrences, forward and adjoint, are f32 in both numeric modes; the Linear layers and every weight-gradient product take the
 * handle's operand type.  Launched kernel by kernel, no captured graph; the forward group path WAITS on the host for its fault
 * word like dimx_mesh_head (reruns are counted in dimx_lstm_faults).  Deterministic: no float atomics, a rerun is bit-identical. */
int dimx_train_conv_forward_backward(dimx_handle h, const float* params, float* grads, const float* motion, const float* templ,
                                     const float* target, const float* vert_w, int n_mouth, int B, int T, int flags, float* loss_out,
                                     float* mesh_out, void* ws, size_t ws_bytes, void* stream);
/* ---- DIM-Speaker fine-tuning step: reference SpeakerSLMFT.forward(mode='train') (code/seq2seq_pretrain.py:708-757) under the
 * loop train_epoch_biwi (code/x_engine_pt.py:62-132; AdamW lr 1e-5, clip 1.0, batch size 1).  The handle must be a speaker handle
 * (variant 2 with mesh_dim > 0; DIMX_ERR_STATE otherwise) whose weights were loaded with speaker_embed.weight among them.  What
 * trains is what that forward leaves a gradient on, in flat f32 arenas (tensors 16-byte aligned) as for the other steps:
 * patch_embed_dec_l, decoder_joint.* (its absolute positional table included), speaker_vq.decoder.* and speaker_embed.weight
 * [rows, 384] (dense: rows no clip names get a zero gradient and are still decayed by AdamW).  The encoders, the norms, the
 * converter head and the frozen halves of the VQ-VAEs receive no gradient in the reference and are not in the arenas. */
int dimx_train_spk_num_params(dimx_handle h);
int64_t dimx_train_spk_total(dimx_handle h);   /* floats in an arena */
int dimx_train_spk_param_info(dimx_handle h, int i, const char** name, int64_t* offset, int64_t* numel);
size_t dimx_train_spk_workspace_bytes(dimx_handle h, int B, int T);
/* One forward + backward pass.  v_emoca [B,T,56], v_audio [B,T,768] f32; mask [B,T] uint8 (1 = valid frame: the cross-attention's
 * key mask); z [B,T] int32: the LISTENER VQ-VAE's codes of v_emoca, -100 on padding (dimx_vq_encode); speaker_ids [B] int32 on the
 * device or NULL (NULL: a zero embedding row, and speaker_embed.weight's gradient is zero); codebook_s [512,128] and pe_s [>= B
 * rows of 384]: the speaker VQ-VAE's frozen codebook and its decoder's positional buffer.
 *   ctx = cat(speaker_embed[ids] + patch_embed_dec_l, v_audio);  logits = decoder_joint(z[:, :-1], ctx, mask) (no key masking of
 *   the self-attention);  l_ce = cross entropy against z[:, 1:] (ignore -100);  idx = argmax(logits) (first index on ties);
 *   pred = speaker_vq.decode(codebook_s[idx]);  l_emoca = mean((pred - v_emoca[:, 1:])^2) over all B (T-1) 56 elements, padded
 *   frames included;  grads (overwritten) = d(l_ce + l_emoca): l_emoca reaches speaker_vq.decoder.* only, the arg-max cuts the rest.
 * loss_out: 4 device floats {l_ce, 1 / valid targets, l_emoca, 1 / elements}.  Optional outputs: logits_out [B,T-1,512], idx_out
 * [B (T-1)] int32, pred_out [B,T-1,56] (16-byte aligned).  The mesh head is not part of the call (it reports a metric and takes no
 * gradient): run dimx_mesh_head or dimx_train_conv_forward_backward(grads = NULL) on pred_out.  A speaker id outside [0, rows) is
 * DIMX_ERR_ARG: the ids are read back and checked on the host before the first launch (one stream synchronisation when ids are
 * given).  Launched kernel by kernel on `stream`, no captured graph.  Deterministic: no float atomics, every sum in a fixed order
 * (the embedding gradient adds its clips in ascending b per table row), a rerun is bit-identical. */
int dimx_train_spk_forward_backward(dimx_handle h, const float* params, float* grads, const float* v_emoca, const float* v_audio,
                                    const uint8_t* mask, const int32_t* z, const int32_t* speaker_ids, const float* codebook_s,
                                    const float* pe_s, int B, int T, float* loss_out, float* logits_out, int32_t* idx_out, float* pred_out,
                                    void* ws, size_t ws_bytes, void* stream);
/* The adjoint of one bidirectional LSTM layer alone (unit parity): x [B,T,In], the four weight sets as dimx_op_lstm_layer takes
 * them, dy [B,T,2H] -> dx [B,T,In] (optional), dw_ih[d] [4H,In], dw_hh[d] [4H,H], db[d] [4H] (= d bias_ih = d bias_hh).  f32
 * only.  It runs the training forward first.  Allocates its scratch and synchronises the stream. */
int dimx_op_lstm_layer_bwd(int dtype, const float* x, int B, int T, int In, int H, const float* const* w_ih, const float* const* w_hh,
                           const float* const* b_ih, const float* const* b_hh, const float* dy, float* dx, float* const* dw_ih,
                           float* const* dw_hh, float* const* db, int flags, int* faults_out, void* stream);
/* Gradient clipping (torch.nn.utils.clip_grad_norm_, max_norm <= 0: none) + one torch.optim.AdamW step over a flat arena.
 * step: 1-based step count (bias correction).  scratch: >= 1026 device floats; scratch[1024] = gradient norm before clipping,
 * scratch[1025] = the clip coefficient applied.  params, grads, exp_avg and exp_avg_sq must be 16-byte aligned (the kernels read
 * them as float4): DIMX_ERR_ARG before any launch otherwise. */
int dimx_train_adamw(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int64_t n, float lr, float beta1,
                     float beta2, float eps, float weight_decay, int step, float max_norm, float* scratch, void* stream);
/* The attention operator of the training step alone (unit parity): q [B,Lq,H*64], k / v [B,Lk,H*64] f32, head h at columns
 * 64 h; kmask / kmask2 [B,Lk] uint8 keep-masks (NULL = keep all), causal: key j > query i masked; masked scores are filled
 * with -FLT_MAX before the softmax (x-transformers' Attend).  Writes o [B,Lq,H*64] and lse [B,H,Lq]; with d_o also delta
 * [B,H,Lq], dq, dk, dv.  mfma = 1: the bf16 matrix-core kernels the perf mode trains with (csrc/train_attn.hip), 2: the same
 * kernels on exact-f32 MFMA (what the parity mode trains with), 0: the one-wave-per-row f32 VALU kernels (the plain form). */
int dimx_op_train_attention(int mfma, const float* q, const float* k, const float* v, const float* d_o, const uint8_t* kmask,
                            const uint8_t* kmask2, int B, int H, int Lq, int Lk, int causal, float scale, float* o, float* lse,
                            float* delta, float* dq, float* dk, float* dv, void* stream);
/* The same operator with the online window (dimx/online.py; what dimx_set_train_lookahead puts on the step's cross attention):
 * win != 0: query i keeps key j iff j < clamp(i + 2 + lookahead, 1, Lk) and the keep-masks keep j.  Key 0 is always inside the
 * window; lookahead >= Lk - 2 is the window off, bit for bit.  Any int is a valid lookahead (the diagonal is formed in 64 bits
 * and clamped on the host).  A masked key has probability exactly 0 and gets no gradient.  win and causal together are
 * DIMX_ERR_ARG; win = 0 is dimx_op_train_attention.  A query whose every in-window key is dropped by kmask / kmask2 is outside
 * the contract (its row is then a softmax over filled scores, as x-transformers' would be, but over the key tiles the kernels
 * did not skip only). */
int dimx_op_train_attention_win(int mfma, const float* q, const float* k, const float* v, const float* d_o, const uint8_t* kmask,
                                const uint8_t* kmask2, int B, int H, int Lq, int Lk, int causal, float scale, int win, int lookahead,
                                float* o, float* lse, float* delta, float* dq, float* dk, float* dv, void* stream);
/* The operators of the training step whose launch plan depends on the row count alone (unit parity).  Each runs the step's own
 * helper over caller scratch, so rows per block, slab counts, chunk widths and the deferred column-sum finish are the step's.
 * scratch: 256-byte aligned device floats for the partial rows; too little is DIMX_ERR_WORKSPACE before any launch.
 * dimx_op_train_layernorm_bwd: x, dy [M,C] f32, gamma [C], C in {384, 512, 768, 1152} -> dx [M,C] (accumulate: dx += ...), dgamma [C],
 *   dbeta [C] (optional).  roundup4(ceil(M / 600)) rows per block; scratch >= 2 * (600 * C + 64) floats is always enough.
 * dimx_op_train_colsum: dy [M,C] f32 -> out [C] = column sums (a bias gradient); 1 slab of rows below 256 rows, 32 from 256 up;
 *   scratch >= 32 * C + 64 floats.
 * dimx_op_train_prep: the operand copy in front of every training GEMM.  dtype: DIMX_F32 / DIMX_BF16 operand type; src [rows,cols]
 *   f32 with row stride lds; mode 0 copy, 1 erf-GELU(src), 2 LayerNorm(src) * gamma (+ beta), 3 src * erf-GELU'(src2), 4 / 5 = 1 / 3
 *   with tanh-GELU (src2 [rows,cols] with row stride lds2: modes 3 and 5).  Writes o [rows,Kp] and t [cols,Mp] (the transpose),
 *   Kp / Mp = cols / rows padded to the operand type's k-tile (64 bf16, 32 f32) with exact zeros, and (optional) colpart
 *   [n_part,cols] f32: row i = column sums of rows 32 i .. 32 i + 31 of what was cast.  dims3 (host) = {Kp, Mp, n_part}.  o_elems,
 *   t_elems, colpart_floats: what the buffers hold; too little is DIMX_ERR_WORKSPACE.  cols, lds, lds2 multiples of 4, 16-byte aligned.
 * dimx_op_train_cross_entropy: logits [R,512] f32, targets [R] int32 (outside [0, 512): ignored) -> row_loss [R], dlogits [R,512]
 *   = d loss / d logits, loss_out2 = {mean loss over the valid targets, 1 / max(count, 1)} (no valid target: loss 0, dlogits 0). */
int dimx_op_train_layernorm_bwd(const float* x, const float* gamma, const float* dy, float* dx, int accumulate, int M, int C, float* dgamma,
                                float* dbeta, float* scratch, size_t scratch_floats, void* stream);
int dimx_op_train_colsum(const float* dy, int M, int C, float* out, float* scratch, size_t scratch_floats, void* stream);
int dimx_op_train_prep(int dtype, int mode, const float* src, int lds, const float* src2, int lds2, const float* gamma, const float* beta,
                       int rows, int cols, void* o, size_t o_elems, void* t, size_t t_elems, float* colpart, size_t colpart_floats,
                       int* dims3, void* stream);
int dimx_op_train_cross_entropy(const float* logits, const int32_t* targets, int R, float* row_loss, float* dlogits, float* loss_out2,
                                void* stream);

/* ---- kernel-level entry points (unit parity tests) -------------------------------------- */

/* C = epilogue(A[M,K] . W[N,K]^T).  A/W element type `in_dtype`, C element type `out_dtype`.
 * W must be K-padded to a multiple of 64 (bf16) / 32 (f32) elements with zeros (ldw = padded K).
 * act: 0 none, 1 LeakyReLU(0.2), 2 GELU-tanh, 3 GELU-erf.  bias [N] f32 / residual [M,ldr] f32
 * optional.  conv_T > 0: A is [B*conv_T, C] and the GEMM is a k=5 replicate-padded temporal
 * convolution with K = 5*C, W tap-major [N][5][C]; conv_lens optional [B] int32.
 * flags: bit 0 = allow split-K with f32 atomics (only taken when residual == C, i.e. in-place accumulation
 * onto the residual stream, small M); bit 1 = force the register-staged (non LDS-DMA) kernel; bit 2 = C is [splits][M, ldc] f32
 * split-K slabs (count: dimx_op_gemm_slabs). */
int dimx_op_gemm(int in_dtype, int out_dtype, const void* A, int lda, const void* W, int ldw, void* C,
                 int ldc, int M, int N, int K, const float* bias, int act, const float* residual,
                 int ldr, int conv_T, const int32_t* conv_lens, int flags, void* stream);
/* The f32 parity mode's decode GEMM alone (csrc/gemm_x3.hip; reference arithmetic: the fp32 Linear layers of the decoder,
 * code/seq2seq_pretrain.py:413-418): an f32 number is the exact sum of three bf16 numbers, so C = A . W^T is computed on the bf16
 * matrix cores from the three planes of each operand with f32 accumulation -- an f32 GEMM at 6/16 of the f32-MFMA cost.
 * dimx_op_split_x3: w [n] f32 (device) -> planes [3][n] bf16 (device), plane0 + plane1 + plane2 == w exactly.
 * dimx_op_gemm_x3: A [M, lda] f32, planes of W [N, K] (K % 32 == 0, N a multiple of 36 / 64 / 72 / 96; planned for M = 256, any M runs), C [M, ldc] f32 or,
 * with flags bit 2, the split-K slabs [dimx_op_gemm_slabs(.., flags | 16)][M, ldc]; bias / act / residual as in dimx_op_gemm. */
int dimx_op_split_x3(const float* w, void* planes, long n, void* stream);
int dimx_op_gemm_x3(const float* A, int lda, const void* planes, float* C, int ldc, int M, int N, int K, const float* bias, int act,
                    const float* residual, int ldr, int flags, void* stream);
/* split-K slabs an out_slabs dimx_op_gemm call with these arguments writes (the f32 kernels plan the count from (N, K) themselves;
 * flags as in dimx_op_gemm: bit 0 allow split-K (without it one slab, the split-bf16 kernel included), bit 4 the split-bf16 kernel
 * of the f32 parity mode, bits 16..23 a forced count).  Every reported slab is written: a count that would leave a split without
 * k-tiles (k-tiles nk, per = ceil(nk / count), (count - 1) * per >= nk) -- forced or planned -- is CLAMPED to ceil(nk / per), the
 * count that covers the same partition, and this function reports the clamped value.  The split-bf16 kernel rejects an
 * activation together with more than one slab (an activation of a partial sum). */
int dimx_op_gemm_slabs(int in_dtype, int M, int N, int K, int flags);
/* The cross-attention K/V projection as dimx_encode_ctx(for_generate=1) launches it: [M = B*rowT, K] . W[N, K]^T, the
 * N columns being nlayers x (K | V) segments of H*64 columns; segment i goes to the i-th [B, H, Tp, 64] cache inside
 * `out`.  bf16 with nlayers = 4 is the fused all-layers launch of the 256 x 256 kernel; f32 supports nlayers = 1. */
int dimx_op_gemm_headmajor(int dtype, const void* A, int lda, const void* W, int ldw, void* out, int M, int N, int K,
                           int rowT, int Tp, int nlayers, void* stream);
/* dimx_op_gemm with an output map instead of a plain C (the epilogue's scatter as the model's projections use it; unit tests).  Rows
 * decompose as m = b * rowT + t (the last clip may be partial); the N columns are nseg (1..3) equal segments of N / nseg columns, and element
 * (m, n) of segment s, nn = n - s * (N / nseg), goes to seg_ptr[s] + b * sb + t * st + (nn / D) * sh + (nn % D) * sd (element strides;
 * seg_strides = [nseg][4] = {sb, sh, st, sd}, seg_D [nseg], D divides N / nseg).  sd == 1 is a row-contiguous segment, anything
 * else a transposed one (V^T: st == 1).  Row add (after the activation, before the residual): rowadd_mode 0 none, 1 table row t,
 * 2 table row b / rowadd_div + rowadd_off, 3 table row rowadd_off; the table is [rows, ld_rowadd] f32 and its row is scaled by
 * rowadd_scale.  flags: bit 1 and bits 8..15 as in dimx_op_gemm (no conv, no slabs).  DIMX_ERR_ARG for a null operand or segment,
 * segments that do not divide N, a mode outside 0..3 or a mode without a table, and whatever the launcher itself refuses (cfg 72
 * with a map, ...); nothing is launched then. */
int dimx_op_gemm_map(int in_dtype, int out_dtype, const void* A, int lda, const void* W, int ldw, int M, int N, int K, const float* bias,
                     int act, const float* residual, int ldr, int rowT, int nseg, void* const* seg_ptr, const int64_t* seg_strides,
                     const int32_t* seg_D, const float* rowadd, int ld_rowadd, int rowadd_mode, float rowadd_scale, int rowadd_off,
                     int rowadd_div, int flags, void* stream);
/* What a dimx_op_gemm_map call with these arguments would launch, answered by the launcher's own decision code; nothing is read,
 * written or launched (only the alignment of the pointers counts).  Returns a negative DIMX_ERR_* as the call would, else the route
 * word: bits 0..15 the kernel -- the LDS-DMA kernels' cfg id 1 / 3 / 4 / 14 / 34 / 35 / 72, 256 the 256 x 256 kernel, 1064 / 1128 the
 * register-staged kernel with its 64 x 64 / 128 x 128 tile --, bit 16 the staged (through-LDS) epilogue, bit 17 packed 4-row stores
 * of transposed segments. */
int dimx_op_gemm_route(int in_dtype, int out_dtype, const void* A, int lda, const void* W, int ldw, int M, int N, int K, const float* bias,
                       int act, const float* residual, int ldr, int rowT, int nseg, void* const* seg_ptr, const int64_t* seg_strides,
                       const int32_t* seg_D, const float* rowadd, int ld_rowadd, int rowadd_mode, float rowadd_scale, int rowadd_off,
                       int rowadd_div, int flags);
/* One bidirectional LSTM layer (csrc/lstm.hip; torch.nn.LSTM(batch_first=True, bidirectional=True), eval, zero initial state, gate
 * order i, f, g, o): x [B,T,In] f32 (In % 4 == 0), H = 384, w_ih[d] [4H,In], w_hh[d] [4H,H], b_ih[d] / b_hh[d] [4H] f32 device
 * pointers (d = 0 forward, 1 reverse), y [B,T,2H] f32, forward half first.  No lengths: every clip runs over all T frames.
 * dtype: DIMX_F32 (the bf16-operand recurrence is not built: DIMX_ERR_ARG).  flags bit 0 = safe path (see dimx_mesh_head).
 * *faults_out (optional) = 1 when the group path reported a fault and the layer was rerun on the safe path, else 0.
 * Allocates its scratch and synchronises the stream. */
int dimx_op_lstm_layer(int dtype, const float* x, int B, int T, int In, int H, const float* const* w_ih, const float* const* w_hh,
                       const float* const* b_ih, const float* const* b_hh, float* y, int flags, int* faults_out, void* stream);
/* y = LayerNorm(x) over the last dim (C in {384,1152}), eps 1e-5; beta optional. */
int dimx_op_layernorm(int out_dtype, const float* x, void* y, const float* gamma, const float* beta,
                      int M, int C, void* stream);
/* y[b,t,c] = (x - mean_bc) / sqrt(var_bc + 1e-5) with statistics over t < len_b (biased var). */
int dimx_op_instnorm(int out_dtype, const float* x, void* y, const int32_t* lens, int B, int T, int C,
                     void* stream);
/* Flash-style attention on packed [B,L,H*D] q/k and a transposed v [B,H,D,Lk_pad] (as the QKV GEMM
 * writes it).  D in {48,64}.  out [B,Lq,H*D]. */
int dimx_op_attention(int dtype, const void* q, const void* k, const void* vt, void* out, int B, int H,
                      int Lq, int Lk, int D, int ldq, int ldk, int ld_vt, int ldo, float scale,
                      int causal, const int32_t* lens, const uint8_t* kmask, void* stream);
/* The same attention with v row-major like k ([B,Lk,H*D] bf16; what the perf mode's fused q/k/v projection writes since round 3:
 * three row-contiguous destinations for the 256x256 GEMM, the transposition happens on the way into LDS).  bf16, D in {48,64}. */
int dimx_op_attention_rowv(const void* q, const void* k, const void* v, void* out, int B, int H, int Lq, int Lk, int D, int ldq,
                           int ldk, int ldv, int ldo, float scale, int causal, const int32_t* lens, const uint8_t* kmask,
                           void* stream);
/* Test entry: the row-major-v attention with every stride given.  q_str / k_str / v_str / o_str are host arrays of three element
 * strides (batch, row, head): element (b, i, h, d) of q at q + b q_str[0] + i q_str[1] + h q_str[2] + d, likewise k, v, out; all
 * multiples of 8.  kmask [B, kmask_ld], kmask_ld >= Lk.  prepacked != 0 packs the key validity words in a launch of its own ahead
 * of the attention (the decode loop's order) instead of inside the attention launch.  bf16, D in {48,64}. */
int dimx_op_attention_strided(const void* q, const void* k, const void* v, void* out, int B, int H, int Lq, int Lk, int D,
                              const long* q_str, const long* k_str, const long* v_str, const long* o_str, float scale, int causal,
                              const int32_t* lens, const uint8_t* kmask, int kmask_ld, int prepacked, void* stream);
/* One-query (autoregressive step) attention over a [B,H,Tmax,64] K/V cache, n_keys keys per (clip,head);
 * q/out are [B,H*64].  kmask optional [B,n_keys].  Cross-attention form (no cache append).
 * nsplit: waves per (clip, head) sharing the keys (1, 2, 4; 0 = automatic).  q_is_f32: q is a single f32 slab
 * (the form dimx_generate launches) instead of the cache's element type. */
int dimx_op_decode_attn(int dtype, const void* q, const void* kcache, const void* vcache, void* out, int B, int H,
                        int Tmax, int n_keys, float scale, const uint8_t* kmask, int nsplit, int q_is_f32,
                        void* stream);
/* Self-attention form of the step kernel, exactly as dimx_generate launches it: qkv [B, ld] holds this step's
 * q | k | v (H*64 each; f32 when q_is_f32, else the cache type), *step_dev keys are already cached; the kernel
 * appends k/v at position *step_dev and attends over *step_dev + 1 keys.  out [B, H*64] in the cache type. */
int dimx_op_decode_attn_self(int dtype, const void* qkv, int ld, void* kcache, void* vcache, void* out, int B, int H,
                             int Tmax, const int32_t* step_dev, float scale, int q_is_f32, void* stream);
/* Every form of the step kernel dimx_generate launches (tests), with all of its arguments:
 *   q [nslab][B*S, q_ld] (slab s at q + s*slab_stride elements): f32 split-K slabs summed in slab order when q_is_f32 (nslab 1..8),
 *     else one row array in the cache type (nslab 1); head h at column h*64.
 *   self_attn = 1: the self form of dimx_op_decode_attn_self -- this step's k / v are columns H*64 / 2*H*64 of the same rows
 *     (q_ld >= 3*H*64), appended at position *step_dev (< Tmax) of the caches, keys = *step_dev + 1; n_keys / kmask unused.
 *   self_attn = 0: the cross form over 1 <= n_keys <= Tmax keys, kmask optional [B, kmask_ld] (kmask_ld >= n_keys, 0 = masked;
 *     a row with every key masked averages V over the n_keys keys, as a softmax over -FLT_MAX scores does).
 *   rows_per_clip S in {2,4,5,8,10} (cross form only): rows b*S .. b*S+S-1 of q / out share clip b's caches and mask row;
 *     S x n_keys beyond the kernel's LDS score buffer is rejected.  0 / 1: one row per clip.
 *   out [B*S, o_ld] in the cache type.  nsplit: waves per (clip, head), 1 / 2 / 4, 0 = automatic. */
int dimx_op_decode_attn_ex(int dtype, const void* q, int q_ld, int q_is_f32, int nslab, long slab_stride, int self_attn, void* kcache,
                           void* vcache, void* out, int o_ld, int B, int H, int Tmax, const int32_t* step_dev, int n_keys,
                           const uint8_t* kmask, int kmask_ld, int rows_per_clip, float scale, int nsplit, void* stream);
/* The table form of the self attention (tests; what dimx_generate launches for the first decoder layer when its k / v come from the
 * table over the token ids): dimx_op_decode_attn_ex's self form (q must be f32 slabs) plus the table arguments.  The cached K / V
 * row of position j < *step_dev of row b is row hist[b][j] of tab [tab_rows, tab_ld] (cache type; K of head h at column
 * tab_koff + h*64, V at tab_voff + h*64; ids outside the table are clamped to its last row); hist [B, hist_ld] int32, hist_ld >= Tmax,
 * entries at or past *step_dev are not used.  Nothing is appended: kcache / vcache are not touched (they must be non-null).  The
 * result has the bits of the cache form run on caches gathered from the table. */
int dimx_op_decode_attn_tab(int dtype, const void* q, int q_ld, int q_is_f32, int nslab, long slab_stride, void* kcache, void* vcache,
                            void* out, int o_ld, int B, int H, int Tmax, const int32_t* step_dev, float scale, int nsplit, const void* tab,
                            int tab_ld, int tab_koff, int tab_voff, int tab_rows, const int32_t* hist, int hist_ld, void* stream);
/* The windowed cross form of an online generation (dimx_set_cross_lookahead): the arguments of dimx_op_decode_attn_ex's cross form
 * plus lookahead; step_dev is required and the keys are j < clamp(*step_dev + 2 + lookahead, 1, n_keys).  K / V rows at or past that
 * bound are never read, and the result has the bits of dimx_op_decode_attn_ex called with n_keys = that bound. */
int dimx_op_decode_attn_win(int dtype, const void* q, int q_ld, int q_is_f32, int nslab, long slab_stride, void* kcache, void* vcache,
                            void* out, int o_ld, int B, int H, int Tmax, const int32_t* step_dev, int n_keys, const uint8_t* kmask,
                            int kmask_ld, int rows_per_clip, float scale, int nsplit, int lookahead, void* stream);
/* FP8 cross K/V, the quantiser (csrc/decode_attn_kv8.hip; dimx/kv8.py quantize): cache [B, H, Tp, 64] of dtype (DIMX_F32 / DIMX_BF16),
 * as dimx_encode_ctx(for_generate = 1) writes a layer's K or V.  Rows 0 .. T - 1 of every (clip, head) become 64 OCP e4m3fn codes
 * (codes [B, H, Tp, 64] uint8) and one scale (scales [B, H, Tp] f32): scale = amax / 448 (a row with amax < 2^-60: scale 0, codes 0),
 * code = e4m3fn(clamp(x / scale, +-448)), round to nearest even, both divisions IEEE f32.  Rows at or past T are neither read nor
 * written.  DIMX_ERR_ARG (nothing launched) for a null or misaligned operand (cache / codes 16 bytes, scales 4) or T outside 1 .. Tp. */
int dimx_op_kv8_quantize(int dtype, const void* cache, int B, int H, int Tp, int T, uint8_t* codes, float* scales, void* stream);
/* ... the incremental form, as a streaming session's push launches it under dimx_stream_set_kv8 (dimx/kv8.py append): rows
 * [n0, n0 + c) of every (clip, head) of the K and V caches of `depth` layers in one launch, with the quantiser's arithmetic (the
 * bits dimx_op_kv8_quantize gives those rows).  caches, codes, scales: HOST arrays of 2 * depth device pointers -- K of layer 0,
 * V of layer 0, K of layer 1, ... -- to caches [B, H, Tc, 64] of dtype, code planes [B, H, Tp, 64] uint8 and scale planes
 * [B, H, Tp] f32.  Rows outside the range are neither read nor written.  DIMX_ERR_ARG (nothing launched) for another dtype, depth
 * outside 1 .. 8, c < 1, n0 < 0, n0 + c beyond Tc or Tp, Tp > 2048, a null pointer, caches or codes not 16-byte aligned, scales not
 * 4-byte aligned. */
int dimx_op_kv8_append(int dtype, const void* const* caches, uint8_t* const* codes, float* const* scales, int depth, int B, int H, int Tc, int Tp,
                       int n0, int c, void* stream);
/* ... and the one-query cross attention over such codes, as dimx_generate launches it with dimx_set_cross_kv8: the arguments of
 * dimx_op_decode_attn_win with kcodes / kscale / vcodes / vscale ([B, H, Tmax, 64] uint8, [B, H, Tmax] f32) in place of the caches,
 * out_dtype (DIMX_F32 / DIMX_BF16: the type of out [B, o_ld], the handle's operand type) in place of dtype, and win: 0 = the keys
 * j < n_keys (step_dev and lookahead unused), 1 = the keys j < clamp(*step_dev + 2 + lookahead, 1, n_keys).  q is f32 split-K slabs
 * (q_is_f32 must be 1; nslab 1..8, summed in slab order).  Scores are scale * q . (kscale[j] * codes[j]); a masked key scores
 * -FLT_MAX, a row with every key masked is the mean of the dequantised V over the keys.  Codes and scales at or past the key bound
 * are never read; the windowed form has the bits of the plain form called with n_keys = that bound; no atomics, repeats are
 * bit-identical; nsplit = 0 on out_dtype = DIMX_F32 depends on Tmax only.  DIMX_ERR_ARG (nothing launched) for a null or misaligned
 * operand (q / codes / out 16 bytes, scales 4; q_ld, slab_stride multiples of 4, o_ld of 4 (f32) / 8 (bf16)), n_keys outside
 * 1 .. min(Tmax, 2048), kmask_ld < n_keys, win without a step counter, or rows_per_clip > 1. */
int dimx_op_decode_attn_kv8(int out_dtype, const void* q, int q_ld, int q_is_f32, int nslab, long slab_stride, const uint8_t* kcodes,
                            const float* kscale, const uint8_t* vcodes, const float* vscale, void* out, int o_ld, int B, int H, int Tmax,
                            const int32_t* step_dev, int n_keys, const uint8_t* kmask, int kmask_ld, int rows_per_clip, float scale, int nsplit,
                            int lookahead, int win, void* stream);
/* The multi-query form (dimx/kv8.py attention_rows): the arguments of dimx_op_decode_attn_kv8 with B clips and
 * rows_per_clip = S in {2, 4, 5, 8, 10} -- rows b*S .. b*S+S-1 of q / out share clip b's codes, scales and mask row -- and exact.
 * q is f32 split-K slabs [nslab][B*S, q_ld] (q_is_f32 = 1; nslab 1..8, summed in slab order) or one bf16 row array [B*S, q_ld]
 * (q_is_f32 = 0, nslab = 1, q_ld a multiple of 8).  One wave per (clip, head) on v_mfma_f32_16x16x32_bf16, the codes converted to
 * bf16 exactly and read once for all S; nsplit is ignored, so a slice of clips returns the whole batch's bits.
 *   exact = 0, the matrix-core form: two roundings beyond f32 arithmetic, q -> bf16 (RNE of the slab sum) and (p * vscale) -> bf16;
 *              the K scale is applied to the f32 scores and the row sum is that of the unrounded p.
 *   exact = 1, the exact form: q and p * vscale enter as three bf16 planes each, so products are exact in f32 and the result is
 *              within the step kernels' f32 tolerance of the definition.
 * Conventions, bounds and refusals are dimx_op_decode_attn_kv8's (a masked key scores -FLT_MAX, nothing at or past the key bound is
 * read, the windowed form has the bits of the plain form at n_keys = the bound, repeats are bit-identical); any other rows_per_clip
 * is DIMX_ERR_ARG.  Query rows the operand is padded with are never stored. */
int dimx_op_decode_attn_kv8_multi(int out_dtype, const void* q, int q_ld, int q_is_f32, int nslab, long slab_stride, const uint8_t* kcodes,
                                  const float* kscale, const uint8_t* vcodes, const float* vscale, void* out, int o_ld, int B, int H, int Tmax,
                                  const int32_t* step_dev, int n_keys, const uint8_t* kmask, int kmask_ld, int rows_per_clip, float scale,
                                  int nsplit, int lookahead, int win, int exact, void* stream);
/* The self attention over FP8 self caches, as dimx_generate launches it with dimx_set_self_kv8 (dimx/kv8.py self_step): qkv is f32
 * split-K slabs [nslab][B, ld] (nslab 1..8, summed in slab order), row b holding q | k | v at columns 0, H*64, 2*H*64 (ld >= 3*H*64).
 * The k / v sums are quantised as dimx_op_kv8_quantize quantises a cache row and stored at position n of kcodes / vcodes
 * [B, H, Tmax, 64] uint8 and kscale / vscale [B, H, Tmax] f32; the output is the softmax attention (scores scale * q . k) over the
 * dequantised rows 0 .. n, row n from registers.  n is *step_dev clamped to 0 .. n, or n itself with step_dev = NULL, so no position
 * past the given n is addressed whatever the device word holds.  Rows past n are neither read nor written, every other row is left
 * as it is; no atomics, repeats are bit-identical; nsplit = 0 on out_dtype = DIMX_F32 depends on Tmax only.  DIMX_ERR_ARG (nothing
 * launched) for a null or misaligned operand (qkv / codes / out 16 bytes, scales 4; ld, slab_stride multiples of 4, o_ld of 4 (f32) /
 * 8 (bf16)), n outside 0 .. min(Tmax, 2048) - 1, nslab outside 1..8 or another out_dtype. */
int dimx_op_decode_attn_self_kv8(int out_dtype, const float* qkv, int ld, int nslab, long slab_stride, uint8_t* kcodes, float* kscale,
                                 uint8_t* vcodes, float* vscale, void* out, int o_ld, int B, int H, int Tmax, const int32_t* step_dev, int n,
                                 float scale, int nsplit, void* stream);
/* Append attention (csrc/stream_attn.hip; what a streaming session launches for every encoder layer): the self attention of the c
 * new rows of every clip over a growing K / V cache.  qkv [B*c, ld] f32 (row b*c + i; q | k | v at columns 0, H*64, 2*H*64, ld >= 3*H*64,
 * the layout the q/k/v projection writes), kcache / vcache [B, H, Tmax, 64] of dtype (DIMX_F32 / DIMX_BF16), n0 rows already cached,
 * 1 <= c <= 16, n0 + c <= Tmax <= 2048.  The k / v rows are rounded to dtype and stored as cache rows [n0, n0 + c); query i attends
 * over the cache rows 0 .. n0 + i -- the new ones as stored -- with scale * q.k, softmax in f32; out [B*c, H*64] in dtype.
 *   - The output row of a query has the same bits whether the row arrives alone (c = 1) or anywhere inside a chunk.
 *   - Cache rows at or past n0 + c are never read; rows outside [n0, n0 + c) are never written.
 * One launch, no atomics, fixed orders.  DIMX_ERR_ARG (nothing launched) for a null or misaligned (16 bytes) operand or a shape outside
 * the ranges above. */
int dimx_op_append_attn(int dtype, const float* qkv, int ld, void* kcache, void* vcache, void* out, int B, int H, int Tmax, int n0, int c,
                        float scale, void* stream);
/* Windowed cross attention for many queries (csrc/win_attn.hip; what dimx_decode_tf_win, the windowed prefill of
 * dimx_generate_prompted and dimx_stream_begin_prompted launch for every decoder layer).  q [B*Lq, ld] f32 (row b*Lq + i, head h at
 * column h*64, ld >= H*64, ld % 4 == 0); kcache / vcache [B, H, Tp, 64] of dtype (DIMX_F32 / DIMX_BF16), the layout
 * dimx_encode_ctx(for_generate = 1) writes, of which rows 0 .. n_keys - 1 are keys (1 <= n_keys <= min(Tp, 2048)); kmask [B, kmask_ld]
 * uint8 keep-mask (kmask_ld >= n_keys) or NULL.  Query row i of a clip has position t = t0 + i (t0 >= 0) and attends over the keys
 *     j < clamp(t + 2 + lookahead, 1, n_keys)   with kmask[b][j] != 0
 * (dimx/online.py; any int is a valid lookahead, the bound is formed in 64 bits) with scale * q.k, softmax in f32; out [B*Lq, o_ld]
 * in dtype (o_ld >= H*64, o_ld % 8 == 0).  Nothing is written to the caches.
 *   - The output row of a query has the same bits whatever Lq is, however t0 + i splits into t0 and i, and wherever the row lies
 *     in a launch.
 *   - K / V rows at or past the bound of the launch's last query are never read; nor are q rows outside [0, B*Lq).
 *   - A row whose visible keys are all masked is zero.
 * One launch, no atomics, fixed orders.  DIMX_ERR_ARG (nothing launched) for a null or misaligned (16 bytes) operand or a shape outside
 * the ranges above. */
int dimx_op_cross_attn_win(int dtype, const float* q, int ld, const void* kcache, const void* vcache, int Tp, void* out, int o_ld, int B, int H,
                           int Lq, int t0, int n_keys, int lookahead, const uint8_t* kmask, int kmask_ld, float scale, void* stream);
/* Decode-step residual + pre-norm: x[M,C] += sum_s slabs[s] (fixed order), y = LayerNorm(x) * gamma (no bias). */
/* The prefill's fused feed-forward sublayer alone (csrc/mlp_fused.hip; unit parity): x [M,C] f32 on the device is replaced by
 * x + W2 . gelu(W1 . LayerNorm(x) + b1) + b2 with bf16 operands and f32 accumulation.  w1 [F,C], b1 [F] (or NULL), w2 [C,F] are HOST
 * f32 arrays (packed into the kernel's chunk images by the call); b2 [C], ln_g [C], ln_b [C] (or NULL) are device f32.  C = 384,
 * F a multiple of 32; act 2 = tanh-GELU (VQ-VAE blocks, code/models/lib/base_models.py:56-68), 3 = erf-GELU (x-transformers
 * FeedForward).  Synchronises the stream. */
int dimx_op_mlp_fused(float* x, const float* w1_host, const float* b1_host, const float* w2_host, const float* b2, const float* ln_g,
                      const float* ln_b, int M, int C, int F, int act, void* stream);
/* The same in its parts (what dimx_load_weights / the forward do): the size of the packed weights, the host-side packing, and the
 * asynchronous launch on weights that already sit on the device (packed: dimx_mlp_fused_packed_bytes(C, F) bytes, 16-byte aligned). */
size_t dimx_mlp_fused_packed_bytes(int C, int F);
int dimx_mlp_fused_pack(const float* w1_host, const float* b1_host, const float* w2_host, int C, int F, void* out_host, size_t out_bytes);
int dimx_op_mlp_fused_packed(float* x, const void* packed, const float* b2, const float* ln_g, const float* ln_b, int M, int C, int F,
                             int act, void* stream);
int dimx_op_add_slabs_layernorm(int out_dtype, float* x, const float* slabs, int nslab, long slab_stride, void* y,
                                const float* gamma, int M, int C, void* stream);
/* One XCD-local chain launch of the decode step (csrc/chain.hip; bf16 only, B <= 256, 256-CU device):
 *   [W1 != NULL]  xr = A1[B,K1] . W1[C,K1]^T ;   x[B,C] += xr + sum_s slabs[s][B,C] ;   y = bf16(LayerNorm(x) * gamma) ;
 *   [W2 != NULL]  out2[B,N2] = y . W2[N2,C]^T   (f32).
 * A1 / W1 / W2 / y are bf16, x / slabs / gamma / out2 f32.  scratch: >= 2048 + B*C*4 bytes of device memory; on return
 * (after the stream has drained) ((uint32_t*)scratch)[129] holds the kernel's error flags (0 = ok, bit 0 = two blocks
 * claimed the same (XCD, CU slot), bit 1 = a group barrier timed out, bit 2 (deferred form only) = a row's |mean| exceeds 8
 * standard deviations, i.e. the deferred LayerNorm's bf16(x) operand is too coarse for it). */
int dimx_op_chain(const void* A1, int K1, const void* W1, float* x, const float* slabs, int nslab, const float* gamma,
                  void* y, const void* W2, int N2, float* out2, int B, int C, void* scratch, void* stream);
/* Deferred-LayerNorm form of the chain launch (what generate() runs in the bf16 mode):
 *   x[B,C] += A1[B,K1] . W1[C,K1]^T ;  y = bf16(x) (NOT normalised) ;  stats[8][32][32][2] = {sum x, sum (x - slice mean)^2} of
 *   the CU's column slice per (row group, CU, row), combined by the consumers with the parallel-variance formula ;  [W2s != NULL]  out2[B,N2] = rstd * (y . W2s^T - mean * colsum2), i.e. LayerNorm(x) * gamma . W2^T
 *   for W2s = gamma o W2 (columns scaled) and colsum2[n] = sum_k W2s[n][k].  scratch / error flags as dimx_op_chain. */
int dimx_op_chain_ln(const void* A1, int K1, const void* W1, float* x, void* y, float* stats, const void* W2s,
                     const float* colsum2, int N2, float* out2, int B, int C, void* scratch, void* stream);
/* C[M,N] = act(LayerNorm-corrected A . Ws^T + bias): the consumer side of dimx_op_chain_ln (decode-step ff1).  A = bf16(x)
 * un-normalised [M,K], Ws = gamma o W bf16 [N,K], stats as written by dimx_op_chain_ln over K columns, colsum[n] = sum_k
 * Ws[n][k]; out_dtype DIMX_BF16 / DIMX_F32; M <= 256. */
int dimx_op_gemm_ln(int out_dtype, const void* A, const void* Ws, void* C, int M, int N, int K, const float* bias, int act,
                    const float* stats, const float* colsum, void* stream);
/* The attention half of one decoder layer of the decode step as ONE XCD-local launch (csrc/chain.hip xcd_layer_kernel; what
 * dimx_generate runs per layer for 128 < B <= 256 clips in the bf16 mode; x-transformers Decoder layer, reference
 * code/seq2seq_pretrain.py:413-419, one step of AutoregressiveWrapper.generate :450):
 *   o = self-attention(q, k, v of this step summed from the nslab f32 slabs qkv[s][B, 3*768]; keys = *step cached rows of
 *       sk / sv [B,12,T,64] bf16, the new row is appended);   x += o . Wso^T;   y = bf16(x);   qc = LN(x) . Wq^T in its deferred
 *   form (w_cq = gamma o Wq, colsum_cq its row sums);   o = cross-attention(qc, ck / cv [B,12,Tp,64] bf16, n_keys, kmask [B,n_keys]);
 *   x += o . Wco^T;   y = bf16(x);   stats = the partial row sums of x for the consumer's deferred LayerNorm.
 * w_so / w_co [1152][768], w_cq [768][1152] bf16 row-major; x [B,1152] f32, y [B,1152] bf16, o [B,768] bf16, qc [B,768] f32,
 * stats [8][32][32][2] f32; *step = cached self-attention keys; scratch >= 4096 bytes, zeroed by the caller before the first call
 * (arrival counters, claim stamps, error flags at word 768: 0 = ok); call_index = 0, 1, 2, ... on the same scratch (the epoch
 * of its monotonic counters). */
int dimx_op_layer_chain(const float* qkv, int nslab, long slab_stride, void* sk, void* sv, int T, const void* ck, const void* cv,
                        int Tp, int n_keys, const uint8_t* kmask, const void* w_so, const void* w_cq, const float* colsum_cq,
                        const void* w_co, float* x, void* y, void* o, float* qc, float* stats, int B, const int32_t* step,
                        int call_index, float scale, void* scratch, void* prof, void* stream);
/* dimx_op_layer_chain with the self attention in its table form (tests; the first decoder layer's launch): the arguments of
 * dimx_op_layer_chain plus the table arguments of dimx_op_decode_attn_tab (bf16 table, hist [B, hist_ld >= T]); sk / sv are not
 * touched. */
int dimx_op_layer_chain_tab(const float* qkv, int nslab, long slab_stride, void* sk, void* sv, int T, const void* ck, const void* cv,
                            int Tp, int n_keys, const uint8_t* kmask, const void* w_so, const void* w_cq, const float* colsum_cq,
                            const void* w_co, float* x, void* y, void* o, float* qc, float* stats, int B, const int32_t* step,
                            int call_index, float scale, void* scratch, void* prof, const void* tab, int tab_ld, int tab_koff,
                            int tab_voff, int tab_rows, const int32_t* hist, int hist_ld, void* stream);
/* ... with the sampler of the previous step's logits as the launch's first stage (csrc/chain.hip, xcd_layer_kernel HEAD).  `params`
 * is a parameter block of 16 int32 words laid out as dimx_generate's: 0 the step word, 2 the temperature's bits, 4-5 the seed,
 * 6 / 7 the row offset and row count of the whole batch (generator window), 8 the arrival counter (0), 9 the chain epoch, 14 the
 * first-step flag.  Flag clear: row b's token is sampled from logits [>= B, 512] at step = word 0 (top-k filter, injected noise
 * [steps, rows_total, 512] or the seeded generator), written to tokens[b, step], hist[b, step + 1] and as emb_table [512][1152]
 * row into x; the self attention runs position step + 1 on q | k | v = row `token` of qkv0 [512][2304] f32, and the launch leaves
 * words 0 and 9 advanced by one.  Flag set: nothing is sampled, the token is hist[b, step], the words stay and the flag is
 * cleared.  The group counters' epoch is word 9 (+ 1 with the flag clear): a zeroed scratch wants -1 there (0 with the flag set). */
int dimx_op_layer_chain_head(const float* qkv0, const float* logits, int top_k, const float* exp_noise, int rows_total, int32_t* tokens,
                             int tok_ld, float* logits_out, const float* emb_table, int32_t* params, void* sk, void* sv, int T, const void* ck,
                             const void* cv, int Tp, int n_keys, const uint8_t* kmask, const void* w_so, const void* w_cq,
                             const float* colsum_cq, const void* w_co, float* x, void* y, void* o, float* qc, float* stats, int B, float scale,
                             void* scratch, void* prof, const void* tab, int tab_ld, int tab_koff, int tab_voff, int tab_rows, int32_t* hist,
                             int hist_ld, void* stream);
/* The sampler launch of a generation step on such a parameter block (what the head replaces): tokens[r, step], hist[r, step + 1],
 * x_next[r, :] = emb_table[token] (C floats), qkv0_out[r, :] = qkv0[token] (qkv0_N floats), words 0 and 9 advanced by one. */
int dimx_op_sample_step(const float* logits, int R, int top_k, const float* exp_noise, int rows_total, int32_t* tokens, int tok_ld,
                        float* logits_out, const float* emb_table, int C, float* x_next, const float* qkv0, float* qkv0_out, int qkv0_N,
                        int32_t* hist, int hist_ld, int32_t* params, void* stream);
/* Best-of-S selection by Frechet distance, the selection step of the test-time protocol (csrc/fd_select.hip; reference
 * code/x_engine_pt.py:255-270 around code/metrics/eval_utils.py:6-46).  All pointers are device memory.
 *   y_true f32 [B, L, .]: clip j, frame t starts at y_true + j*yt_clip_stride + t*yt_frame_stride (elements; feature stride 1)
 *   y_pred f32 [B, S, L, W]: clip j, try s, frame t starts at y_pred + j*yp_clip_stride + s*yp_sample_stride + t*yp_frame_stride
 *   lens int32 [B]: valid frames per clip (clamped to 0..L); frames t >= lens[j] are never read
 *   columns [c0, c0 + F) of the rows enter the distance, 1 <= F <= 64, c0 + F <= W
 *   fd f64 [B, S] = |mu1 - mu2|^2 + tr S1 + tr S2 - 2 tr sqrt(S1 S2), mean and unbiased covariance over the valid frames, float64
 *       throughout; NaN for every try of a clip with fewer than 2 valid frames
 *   win int32 [B]: first minimum of the row, NaN counting as +inf;  ok uint8 [B]: 0 when no try of the clip has a finite distance
 *   best f32 [B, L, W] or NULL: the winning try's full rows, zero for t >= lens[j] and for clips with ok = 0
 *   workspace: dimx_op_fd_select_ws_bytes(B, S, F) bytes, 8-byte aligned.  After the call its last (B + B*S) int32 hold the Jacobi
 *       sweeps of each clip's target factorisation and of each (clip, try) (diagnostic; the loop is bounded at 30).
 * Asynchronous on `stream`: no allocation, no host synchronisation, no atomics (bit-reproducible).  DIMX_ERR_ARG for F outside
 * 1..64, a window that leaves the row, a null pointer (best excepted), a short or misaligned workspace; nothing is enqueued then. */
size_t dimx_op_fd_select_ws_bytes(int B, int S, int F);
int dimx_op_fd_select(const float* y_true, long yt_clip_stride, long yt_frame_stride, const float* y_pred, long yp_clip_stride,
                      long yp_sample_stride, long yp_frame_stride, const int32_t* lens, int B, int S, int L, int W, int c0, int F,
                      double* fd, int32_t* win, uint8_t* ok, float* best, void* workspace, size_t workspace_bytes, void* stream);
/* The DIM-Speaker mesh metrics, Lip Vertex Error and upper-Face Dynamics Deviation (csrc/mesh_metrics.hip; reference
 * print_biwi_metrics, code/mymetrics.py:122-182), as the float64 value of the reference's formulas on f32 meshes.
 *   y_true / y_pred f32: clip b, frame t is a row of 3*n_vert floats (xyz per vertex, element stride 1) starting at
 *       y + b*clip_stride + t*frame_stride (elements, taken as long: views such as v_speaker[:, 1:] are passed as they are and a
 *       buffer may exceed 2^32 bytes).  A row needs 4-byte alignment only.
 *   templ f32 [B, 3*n_vert] (row b at templ + b*templ_clip_stride) or NULL = the zero template
 *   lens int32 [B] in HOST memory: valid frames per clip, 1..L.  They are checked here and copied into the workspace on `stream`
 *       (a pageable array is staged before the call returns).  Frames t >= lens[b] are never read.
 *   mouth int32 [n_mouth], upper int32 [n_upper] in device memory: vertex indices, in any order, duplicates count.  The result
 *       does not depend on the order beyond float64 rounding (the Python layer uploads sorted copies: neighbouring lanes then read
 *       neighbouring vertices).  An index outside [0, n_vert) is skipped and sets *status; n_mouth = 0 / n_upper = 0 skips that
 *       half and leaves its outputs 0.
 *   clip_out f64 [B, 4] = {sum_t max_m d(b,t,m), lens[b], sigma_gt(b), sigma_pred(b)} with d = |gt - pred|^2 of a vertex,
 *       s_x = |x - templ|^2, sigma_x = mean_u std_t s_x (population standard deviation, two-pass per chunk of 8 frames and Chan's
 *       merge over the chunks: no E[s^2] - E[s]^2).  LVE = sum_b clip_out[b][0] / sum_b clip_out[b][1], FDD = mean_b
 *       (clip_out[b][2] - clip_out[b][3]).
 *   frame_max f64 [B, L] or NULL: max_m d per valid frame, 0 for t >= lens[b]
 *   status int32, one device word: 0, or 1 when an index outside [0, n_vert) was met
 *   workspace: dimx_op_mesh_metrics_ws_bytes(B, L, n_mouth, n_upper) bytes, 8-byte aligned.
 * Asynchronous on `stream`: three launches, no allocation, no host synchronisation, no atomics (bit-reproducible).  DIMX_ERR_ARG
 * for B, L or n_vert < 1, a lens[b] outside 1..L, a null operand (templ and frame_max excepted), a short or misaligned workspace;
 * nothing is enqueued then. */
size_t dimx_op_mesh_metrics_ws_bytes(int B, int L, int n_mouth, int n_upper);
int dimx_op_mesh_metrics(const float* y_true, long yt_clip_stride, long yt_frame_stride, const float* y_pred, long yp_clip_stride,
                         long yp_frame_stride, const float* templ, long templ_clip_stride, const int32_t* lens, int B, int L, int n_vert,
                         const int32_t* mouth, int n_mouth, const int32_t* upper, int n_upper, double* clip_out, double* frame_max,
                         int32_t* status, void* workspace, size_t workspace_bytes, void* stream);
/* The listener evaluation metrics, print_metrics / print_metrics_full (csrc/listener_metrics.hip; reference code/mymetrics.py:7-120
 * around code/metrics/eval_utils.py:6-46,85-91): per clip the Frechet distances of up to 8 column windows and the moments every
 * other printed scalar is made of, as float64 values of the reference's formulas on the f32 inputs.
 *   y_true / y_pred f32 [B, L, Wy], x f32 [B, L, Wx] (the speaker motion), Wy, Wx >= 56: clip b, frame t of a tensor starts at
 *       base + b*clip_stride + t*frame_stride (elements, taken as long; feature stride 1: views such as tgt[:, 1:] are passed as
 *       they are)
 *   lens int32 [B] in device memory: valid frames per clip (clamped to 0..L); frames t >= lens[b] are never read
 *   windows int32 [n_win][4] in HOST memory, 1 <= n_win <= 8, rows (xc0, xF, yc0, yF): the operand rows of window w are
 *       [x[:, xc0:xc0+xF] | y[:, yc0:yc0+yF]] with y = y_true on the target side and y = y_pred on the candidate side;
 *       F = xF + yF, 1 <= F <= 112, xF = 0 is the plain distance, xc0 + xF <= Wx, yc0 + yF <= Wy.  The table is read before the
 *       call returns.
 *   fd f64 [B, n_win] = |mu1 - mu2|^2 + tr S1 + tr S2 - 2 tr sqrt(S1 S2), mean and unbiased covariance over the valid frames,
 *       float64 throughout, tr sqrt(S1 S2) = sum of the square roots of the r = min(F, n - 1) largest eigenvalues of A^T S2 A
 *       with S1 = A A^T (one-sided Jacobi, as dimx_op_fd_select); NaN for a clip with fewer than 2 valid frames
 *   moments f64 [B, DIMX_LM_ROW]: row b holds, with d = gt - pred and the groups g = 0 (pose, columns 0:6) and g = 1 (exp,
 *       columns 6:56), every sum running over the n * cols elements of the group's valid frames:
 *         [0]               n, the valid frames
 *         [1 + 10 g + 0]    sum d^2
 *         [1 + 10 g + 1, 2] mean of gt, sum (gt - mean)^2         [.. + 3, 4] the same of pred        [.. + 5, 6] the same of x
 *         [1 + 10 g + 7]    sum (gt - mean_gt)(x - mean_x)        [.. + 8]    sum (pred - mean_pred)(x - mean_x)
 *         [1 + 10 g + 9]    sum over t >= 1 of ((gt_t - gt_{t-1}) - (pred_t - pred_{t-1}))^2   (the STS sum inside the clip)
 *         [21 .. 77)        d of the first valid frame, 56 columns    [77 .. 133) d of the last valid frame
 *       Two passes (the means first, then the centred sums): no E[v^2] - E[v]^2.  A clip with n = 0 leaves a row of zeros.
 *   workspace: dimx_op_listener_metrics_ws_bytes(B, n_win, F) bytes with F the largest window, 8-byte aligned.  After the call
 *       its last 2 * B * n_win int32 hold the Jacobi sweeps of each (window, clip): the target factorisations [n_win][B], then
 *       the candidate problems [n_win][B] (diagnostic; the loop is bounded at 30).
 * Asynchronous on `stream`: two launches, no allocation, no host synchronisation, no atomics, a fixed summation order
 * (bit-reproducible).  DIMX_ERR_ARG for a null operand, B or L < 1, n_win outside 1..8, Wy or Wx < 56, an F outside 1..112, a
 * window that leaves its row, a negative stride, a short or misaligned workspace; nothing is enqueued then.  _ws_bytes returns 0
 * for B < 1, n_win outside 1..8 and F outside 1..112. */
#define DIMX_LM_ROW 133
size_t dimx_op_listener_metrics_ws_bytes(int B, int n_win, int F);
int dimx_op_listener_metrics(const float* y_true, long yt_clip_stride, long yt_frame_stride, const float* y_pred, long yp_clip_stride,
                             long yp_frame_stride, const float* x, long x_clip_stride, long x_frame_stride, const int32_t* lens, int B,
                             int L, int Wy, int Wx, const int32_t* windows, int n_win, double* fd, double* moments, void* workspace,
                             size_t workspace_bytes, void* stream);
/* The SID diversity metric, calcuate_sid (csrc/kmeans_sid.hip; reference code/metrics/eval_utils.py:51-83): a KMeans fit on the
 * ground-truth frames and the entropy of the histogram of frames over its centres, as the float64 value of scikit-learn's
 * KMeans(K, random_state, n_init='auto') (k-means++ init, lloyd) on float64 copies of the f32 inputs; the definition is
 * dimx.mymetrics.kmeans_fit_f64.  All pointers are device memory.
 *   frames f32: row i starts at frames + i*frame_stride (elements, taken as long); its columns [c0, c0 + F) enter, c0 + F <= W,
 *       W <= frame_stride, F <= 64, K * F <= 2048 (the centres lie in LDS).  Only rows 0 .. N - 1 (M - 1) are read.
 * dimx_op_kmeans_fit:
 *   first_index, U f64 [(K - 1), trials]: the random numbers of the initialisation, drawn on the host (they do not depend on the
 *       data): the first centre's row and per further centre `trials` uniforms (dimx.mymetrics.kmeans_draws), trials <= 16
 *   tol, max_iter: scikit-learn's (1e-4, 300); the threshold is tol * mean of the column variances
 *   centers f64 [K, F]; n_iter int32: Lloyd iterations run; status int32: 0, or the (1-based) iteration at which a cluster was left
 *       without a frame -- the fit stops there (scikit-learn relocates such a centre; that is not restated) and centers is not a
 *       result;  labels int32 [N] or NULL: the assignment the returned means were taken over
 *   workspace: dimx_op_kmeans_fit_ws_bytes(N, K, F) bytes, 256-byte aligned.
 *   The whole fit is enqueued at once: 5 + 4 (K - 1) + 3 max_iter launches; convergence is a device word and every launch after it
 *   is set returns at once.  No host synchronisation, no floating-point atomics, fixed summation orders (bit-reproducible).
 * dimx_op_sid_assign:
 *   hist int64 [K]: frames per nearest centre (the first index on ties);  sid f64: -sum h log2(h + 1e-6), h = hist / M;
 *   labels int32 [M] or NULL.  Two launches and a memset; integer atomics only.
 * DIMX_ERR_ARG for a null operand (labels excepted), N < K, F or K * F beyond the LDS plan, a window that leaves the row, a frame
 * stride below W, first_index outside [0, N), trials outside 1..16, a short or misaligned workspace; nothing is enqueued then.
 * _ws_bytes returns 0 for N < 1 and shapes beyond the LDS plan. */
size_t dimx_op_kmeans_fit_ws_bytes(int N, int K, int F);
int dimx_op_kmeans_fit(const float* frames, long frame_stride, int N, int W, int c0, int F, int K, int first_index, const double* U,
                       int trials, double tol, int max_iter, double* centers, int32_t* n_iter, int32_t* status, int32_t* labels,
                       void* workspace, size_t workspace_bytes, void* stream);
int dimx_op_sid_assign(const float* frames, long frame_stride, int M, int W, int c0, int F, const double* centers, int K, int64_t* hist,
                       double* sid, int32_t* labels, void* stream);
/* Sequence log-likelihoods over dumped logits and the best-of-S pick by them (csrc/seq_score.hip; the definition is
 * dimx/scoring.py): the model's own verdict on a sampled (or given) token sequence, the selection criterion that needs no ground
 * truth.  All pointers are device memory; the vocabulary is the sampler's 512 entries.
 * dimx_op_seq_logprob:
 *   logits f32: row r, column c holds 512 entries (element stride 1) starting at logits + r*row_stride + c*step_stride (elements,
 *       taken as long; step_stride >= 512): the logits_out dump of dimx_generate / dimx_generate_prompted, the logits of
 *       dimx_decode_tf, or a view of either
 *   tokens int32: row r, column c at tokens + r*tok_row_stride + c.  A token outside [0, 512) (the -100 padding of forward_vq) is
 *       skipped and not counted, as ce_argmax_kernel skips it; its column's logits are never read
 *   first / last int32 [R / rows_per_clip] or NULL (= 0 / n): row r belongs to clip r / rows_per_clip and sums the columns
 *       clamp(first[clip], 0, n) <= c < clamp(last[clip], 0, n); columns outside are never read
 *   score f64 [R] = sum over the summed columns of logits[tok] - logsumexp(logits), float64 throughout (exact f32 row maximum, exp of
 *       the double difference, double sums and log);  count int32 [R]: the columns summed.  An empty range gives (0.0, 0)
 *   tok_logprob f64 [R, n] or NULL: the per-column terms, 0 outside the range and for skipped tokens.  (f64, not f32: a term is the
 *       float64 value of the definition like the sums)
 * dimx_op_score_select:
 *   score f64 [B, S];  win int32 [B]: first maximum of the row, NaN counting as -inf;  ok uint8 [B]: 0 when no try of the clip has a
 *       finite score
 *   y_pred f32 [B, S, L, W], lens int32 [B], best f32 [B, L, W] or NULL: the winning try's rows with the clip / sample / frame strides
 *       and the lens clamp of dimx_op_fd_select, zero for t >= lens[b] and for clips with ok = 0.  y_pred and lens may be NULL when
 *       best is
 *   tokens int32 (row b*S + s at tokens + (b*S + s)*tok_row_stride), best_tokens int32 [B, n] or NULL: the winner's token row, -100
 *       for clips with ok = 0.  tokens may be NULL when best_tokens is
 * Asynchronous on `stream`: one launch each, no workspace, no allocation, no host synchronisation, no atomics, fixed summation
 * orders (bit-reproducible).  DIMX_ERR_ARG for a null required pointer, n, B, S or rows_per_clip below 1, a negative R or stride,
 * step_stride < 512, an R that is not a multiple of rows_per_clip, L or W below 1 with best; nothing is enqueued then.  R = 0 with
 * valid arguments is a no-op that returns 0. */
int dimx_op_seq_logprob(const float* logits, long row_stride, long step_stride, const int32_t* tokens, long tok_row_stride,
                        const int32_t* first, const int32_t* last, int rows_per_clip, int R, int n, double* tok_logprob, double* score,
                        int32_t* count, void* stream);
int dimx_op_score_select(const double* score, const float* y_pred, long yp_clip_stride, long yp_sample_stride, long yp_frame_stride,
                         const int32_t* lens, const int32_t* tokens, long tok_row_stride, int B, int S, int L, int W, int n,
                         int32_t* win, uint8_t* ok, float* best, int32_t* best_tokens, void* stream);
/* Consensus (minimum-Bayes-risk, medoid) best-of-S selection: per clip the try with the smallest total distance to the other
 * S - 1 tries (csrc/consensus.hip; the definition is dimx/consensus.py).  No ground truth enters.  All pointers are device memory.
 *   y_pred f32 [B, S, L, W], lens int32 [B], the window [c0, c0 + F): as dimx_op_fd_select (1 <= F <= 64, c0 + F <= W; frames
 *       t >= lens[b] are never read).  S is any value >= 1, not only a batched sample count.
 *   kind 0 (fd): dist[b, i, j] for i < j is the Frechet distance of dimx_op_fd_select with try i as its first operand (S_i = A A^T
 *       is factorised once per try, M = A^T S_j A per pair; the r = min(F, n - 1) largest eigenvalues are kept; no clamp at 0).
 *   kind 1 (l2): dist[b, i, j] for i < j is the mean over the valid frames and the window's columns of (x_i - x_j)^2, float64.
 *   dist f64 [B, S, S] or NULL: dist[b, j, i] = dist[b, i, j] (the same bits), dist[b, i, i] = 0; NaN off the diagonal for a clip
 *       with fewer than 2 valid frames
 *   risk f64 [B, S]: risk[b, i] = sum over j != i of dist[b, i, j], in ascending j from zero
 *   win int32 [B]: first minimum of the risks, NaN counting as +inf;  ok uint8 [B]: 0 when no risk of the clip is finite.  S = 1
 *       gives risk 0, win 0, ok 1
 *   best f32 [B, L, W] or NULL, tokens int32 (row b*S + s at tokens + (b*S + s)*tok_row_stride), best_tokens int32 [B, n_tok] or
 *       NULL: the winner's rows and token row as dimx_op_score_select leaves them (zero / -100 for clips with ok = 0).  tokens may
 *       be NULL when best_tokens is
 *   workspace: dimx_op_consensus_select_ws_bytes(B, S, F, kind) bytes, 8-byte aligned.  After a call of kind 0 its last
 *       (B*S + B*S*(S-1)/2) int32 hold the Jacobi sweeps of each try's factorisation [B, S] and of each pair [B, S*(S-1)/2] (pairs
 *       in the order (0,1), (0,2), .., (1,2), ..; diagnostic; the loop is bounded at 30).
 * Asynchronous on `stream`: three launches for kind 0 (try factorisations, pairs, pick), two for kind 1, no allocation, no host
 * synchronisation, no atomics, fixed summation orders: repeated calls and identical tries give identical bits.  DIMX_ERR_ARG for F
 * outside 1..64, a window that leaves the row, an unknown kind, B, S, L or W below 1, more than 2^31 - 1 pairs, a negative stride, a
 * null required pointer, a short or misaligned workspace; nothing is enqueued then.  _ws_bytes returns 0 for such shapes. */
size_t dimx_op_consensus_select_ws_bytes(int B, int S, int F, int kind);
int dimx_op_consensus_select(const float* y_pred, long yp_clip_stride, long yp_sample_stride, long yp_frame_stride,
                             const int32_t* lens, int B, int S, int L, int W, int c0, int F, int kind /* 0 = fd, 1 = l2 */,
                             double* dist /* [B,S,S] or NULL */, double* risk /* [B,S] */, int32_t* win, uint8_t* ok,
                             float* best /* [B,L,W] or NULL */, const int32_t* tokens, long tok_row_stride, int n_tok,
                             int32_t* best_tokens /* or NULL */, void* workspace, size_t workspace_bytes, void* stream);
/* Retrieval baselines (reference code/baselines.py:30-103: NN audio, NN motion, Random; csrc/retrieval.hip; the definition is
 * dimx/retrieval.py).  All pointers are device memory.
 * dimx_op_pool_desc: clip descriptors.
 *   x f32: frame t of clip i holds D entries (element stride 1) at x + i*clip_stride + t*frame_stride (elements); lens int32 [N],
 *       clamped to [0, T]: frames t >= lens[i] are never read
 *   kind 0 (max): desc[i, d] = the maximum over the valid frames of the f32 values, widened (exact);  kind 1 (mean): the float64 sum
 *       in frame order from zero, divided by the number of valid frames.  A clip without valid frames gets a zero descriptor
 *   desc f64 [N, D] dense, norm f64 [N] = sqrt(sum of squares), summed in an order that depends on D alone
 * dimx_op_nn_search: per query the K library entries of largest cosine similarity.
 *   q_desc f64 (row q at q_desc + q*q_row_stride), q_norm f64 [Q], x_desc / x_row_stride / x_norm [N] likewise; 1 <= D <= 960
 *   sim(q, i) = dot(q_desc[q], x_desc[i]) / (q_norm[q] * x_norm[i]) in float64; the dot product's summation order depends on D alone,
 *       so the value is a function of the two descriptors and norms only, not of Q, N or the pair's position: identical entries tie
 *       bit for bit and a search of a slice of the library returns the same bits for its entries.  A zero norm gives NaN (0 / 0)
 *   idx int32 [Q, K], sim f64 [Q, K]: the K best entries under the total order (similarity descending, index ascending); an entry is
 *       eligible only if its similarity is not NaN and is > -1 (the reference's strict '>' from best_sim = -1).  Unfilled slots hold
 *       -1 / NaN;  found int32 [Q]: the filled slots.  (The reference keeps index 0 where found is 0.)
 *   sim_out f64 [Q, N] or NULL: every similarity (tests and margins; the matrix is not materialised otherwise)
 *   workspace: dimx_op_nn_search_ws_bytes(Q, N, D, K) bytes, 8-byte aligned: the per-(query, chunk of 256 entries) partial lists
 *       [Q][chunks][K] f64 then [Q][chunks][K] int32.  _ws_bytes returns 0 for shapes the call refuses
 * dimx_op_nn_gather: the retrieved sequences.
 *   idx int32 [Q, K] (entries outside [0, N) = no entry), lib_seq f32: frame t of entry i holds W entries at lib_seq + i*clip_stride +
 *       t*frame_stride; lib_lens int32 [N] clamped to [0, Lmax], q_lens int32 [Q] clamped to [0, L]
 *   out f32 [Q, K, L, W], out_len int32 [Q, K]: out_len[q, s] = min(q_lens[q], lib_lens[idx[q, s]], L), the entry's first out_len
 *       frames, zero at and beyond; no entry gives zeros and length 0.  Frames t >= out_len and entries >= N are never read
 * Asynchronous on `stream`: one launch (pool, gather) or two (search: partial lists, merge), no allocation, no host synchronisation,
 * no atomics, fixed summation orders (bit-reproducible).  DIMX_ERR_ARG for K outside 1..16, D < 1 (search: D > 960), N, Q, T, L, Lmax
 * or W below 1, an unknown kind, a negative stride, a null operand (sim_out excepted), a misaligned workspace; DIMX_ERR_WORKSPACE for
 * a workspace that is too small; nothing is enqueued then. */
int dimx_op_pool_desc(const float* x, long clip_stride, long frame_stride, const int32_t* lens, int N, int T, int D,
                      int kind /* 0 = max, 1 = mean */, double* desc, double* norm, void* stream);
size_t dimx_op_nn_search_ws_bytes(int Q, int N, int D, int K);
int dimx_op_nn_search(const double* q_desc, long q_row_stride, const double* q_norm, const double* x_desc, long x_row_stride,
                      const double* x_norm, int Q, int N, int D, int K, int32_t* idx, double* sim, int32_t* found,
                      double* sim_out /* [Q,N] or NULL */, void* workspace, size_t workspace_bytes, void* stream);
int dimx_op_nn_gather(const int32_t* idx, const float* lib_seq, long clip_stride, long frame_stride, const int32_t* lib_lens,
                      const int32_t* q_lens, int Q, int K, int N, int Lmax, int L, int W, float* out, int32_t* out_len, void* stream);
/* The two kernels of dimx_generate_beam on their own (csrc/beam.hip).  All pointers are device memory.
 * dimx_op_beam_step: logits f32 [B*W, 512], cum f64 [B*W], mode int32 [B] (0 live, 2 frozen, anything else forced with
 *   forced_tok[B], clamped to [0, 512); forced_tok may be NULL = token 0) -> parent int32 [B*W], token int32 [B*W], cum_out f64 [B*W]
 *   (cum_out may be cum).  One launch of B blocks.
 * dimx_op_beam_reorder: cache [R, H, T, 64] of DIMX_F32 or DIMX_BF16 elements, 16-byte aligned, parent int32 [R] (entries 0 .. W-1,
 *   rows r = clip*W + w): cache[clip*W + w, :, 0..c, :] = old cache[clip*W + parent[w], :, 0..c, :] in place; positions > c and clips
 *   whose parents are the identity (or out of range) are not touched.  One launch; W = 1 launches nothing.
 * DIMX_ERR_ARG for a null operand, W outside {1,2,4,5,8,10}, B < 1, R not a positive multiple of W, c outside [0, T), a misaligned
 * cache; nothing is enqueued then. */
int dimx_op_beam_step(const float* logits, const double* cum, const int32_t* mode, const int32_t* forced_tok, int B, int W,
                      int32_t* parent, int32_t* token, double* cum_out, void* stream);
int dimx_op_beam_reorder(void* cache, int dtype, const int32_t* parent, int R, int W, int H, int T, int c, void* stream);
/* dimx_op_beam_reorder_kv8: the same permutation of one FP8 code plane kcodes [R, H, Tp, 64] uint8 (16-byte aligned) and its scale
 *   plane kscale [R, H, Tp] f32 (dimx/kv8.py reorder): codes and scale of the positions 0 .. c of row clip*W + w become those of row
 *   clip*W + parent[w], in place; positions > c and clips whose parents are the identity (or out of range) are not touched.  One
 *   launch; W = 1 launches nothing.  The same DIMX_ERR_ARG cases, with c outside [0, Tp). */
int dimx_op_beam_reorder_kv8(void* kcodes, void* kscale, const int32_t* parent, int R, int W, int H, int Tp, int c, void* stream);
/* tokens = sampler(logits[R,512]) -- see dimx_generate. */
int dimx_op_sample(const float* logits, int R, int top_k, float temperature, const float* exp_noise,
                   uint64_t seed, uint64_t step, int32_t* tokens, void* stream);
/* The same launch with a filter kind (dimx_set_sampler_filter; kind 0 uses top_k, the others a / b).  keep_out (optional,
 * [R,512] uint8): the kept set the kernel used, also for a greedy launch.  Invalid settings: DIMX_ERR_ARG. */
int dimx_op_sample_filtered(const float* logits, int R, int kind, int top_k, float a, float b, float temperature,
                            const float* exp_noise, uint64_t seed, uint64_t step, int32_t* tokens, uint8_t* keep_out,
                            void* stream);
/* The guided sampler (classifier-free guidance, dimx/guidance.py): row r is sampled from cond[r] + (scale - 1) * (cond[r] - uncond[r])
 * formed in f32 (scale = 1: cond[r] bit for bit); filter, temperature, noise and generator as dimx_op_sample_filtered on an R-row
 * launch.  cond / uncond: nslab slabs [R,512] each, slab_stride elements apart, added in slab order (nslab = 1: plain rows).
 * tokens [2R]: the token of row r at r and again at r + R, as the guided decode step feeds both halves.  guided_out (optional,
 * [R,512]): the guided rows.  DIMX_ERR_ARG for a NaN or infinite scale, invalid filter settings or slab arguments; nothing is
 * enqueued then. */
int dimx_op_sample_guided(const float* cond, const float* uncond, int R, int nslab, long slab_stride, float scale, int kind, int top_k,
                          float a, float b, float temperature, const float* exp_noise, uint64_t seed, uint64_t step, int32_t* tokens,
                          float* guided_out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DIMX_H */
