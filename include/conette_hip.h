/* conette_hip.h -- C ABI of the MI355X (gfx950) CoNeTTE inference library (libconette_hip.so).
 *
 * The reference (Labbeti/conette-audio-captioning v0.3.1) is pure Python and has NO FFI layer
 * (SURVEY.md section 8b): these entry points sit UNDER the Python operator API that the build's
 * host package (conette_amd) keeps, one per dense stage of the hot path.  Each declaration
 * names the reference interface it replaces (paths relative to /root/reference/src/conette/).
 *
 * Conventions
 *   - every pointer marked "dev" is a device pointer owned by the caller (PyTorch caching
 *     allocator); the library allocates only inside conette_create (packed weights + tables);
 *   - all entry points are asynchronous on `stream` (a hipStream_t passed as void*), never
 *     call hipDeviceSynchronize, and may be captured into a hipGraph;
 *   - return value: 0 = ok, non-zero = error code, text via conette_last_error();
 *     no C++ exception crosses the boundary;
 *   - one host thread per device/process.
 */
#ifndef CONETTE_HIP_H
#define CONETTE_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CONETTE_ABI_VERSION 3 /* 2: conette_encode_taps carries its size; CONETTE_PREC_F16X2 / _FP8 / _F16; conette_decode_graph_nodes
                                 3: conette_decode's `margins` output (the id certificate of the 16-bit precisions), beams up to 16,
                                    conette_encode_nonfinite */

/* precision of GEMM operands / intermediate activations.  Accumulation is always fp32 and the decoder's residual stream is
 * always fp32; the ENCODER's residual stream is IEEE fp16 in the two 16-bit precisions (BF16, F16) since round 5 -- 11
 * significant bits, |x| <= 65504 required: frame embeddings 4.43e-3 -> 4.48e-3 (BF16) and 5.4e-4 -> 8.5e-4 (F16) rel. rms off the
 * fp32 reference for 10 C instead of 16 C bytes moved per position and block -- and fp32 in the other precisions */
#define CONETTE_PREC_F32 0  /* v_mfma_f32_16x16x4_f32: exact-fp32 parity mode          */
#define CONETTE_PREC_BF16 1 /* v_mfma_f32_16x16x32_bf16: throughput mode (BASELINE cfg) */
#define CONETTE_PREC_F16X2 2 /* "exact": every GEMM operand an fp16 hi + lo pair (22 bits), products as three
                                v_mfma_f32_16x16x32_f16 (hi.hi + hi.lo + lo.hi): fp32-MFMA accuracy at MFMA-f16 rate,
                                exact-erf GELU; token ids equal the fp32 mode's / the reference's */

/* 3: the experimental fp8 precision of ABI 2 (pointwise convolutions of stages 0-2 on the non-scaled e4m3 MFMA) -- WITHDRAWN in
 * ABI 3, conette_create refuses it.  BASELINE.json configs[4]'s "fp8 MFMA pointwise GEMMs" is not offered: the block-scaled
 * v_mfma_scale_f32_16x16x128_f8f6f4 does sustain 4.0 PFLOP/s in register-fed loops (3.5x the bf16 16x16x32 loop's 1.13), but e4m3
 * operands -- per-tensor scaled or MX block-scaled alike -- move the frame embeddings by 4 % (MX in stage 2 alone: 3.7 %; the
 * bf16 mode: 0.44 %), an order of magnitude beyond what keeps captions: profiles/r06_notes.md section 3, oracle/mx_study.py */

#define CONETTE_PREC_F16 4 /* the bf16 mode's kernels instantiated for IEEE fp16 operands (v_mfma_f32_*_f16: the same cycles,
                              the same bytes): 11 significant bits instead of 8, i.e. an eighth of the bf16 mode's operand
                              rounding error at the bf16 mode's speed.  Conversions saturate at +-65504; weights below
                              6.1e-5 in magnitude are fp16 subnormals (absolute error <= 3e-8, kept by the MFMA) */

typedef struct conette_ctx conette_ctx; /* opaque: packed weights + constant tables */

/* Hyper-parameters; mirrors CoNeTTEConfig (huggingface/config.py:13-88) + tokenizer ids
 * (tokenization/constants.py:15). */
typedef struct conette_config {
  int32_t precision;    /* CONETTE_PREC_* */
  int32_t vocab_size;   /* rows of model.decoder.classifier.weight */
  int32_t d_model;      /* 256 */
  int32_t nhead;        /* 8   */
  int32_t n_layers;     /* 6   */
  int32_t d_ff;         /* 2048 */
  int32_t pad_id;       /* 0 */
  int32_t bos_id;       /* 1 */
  int32_t eos_id;       /* 2 */
  int32_t reserved[7];
} conette_config;

/* Optional per-stage outputs of conette_encode for parity tests: fp32, channels-last
 * (B, H, W, C) unless noted; any pointer may be NULL. */
typedef struct conette_encode_taps {
  size_t struct_bytes;  /* sizeof(conette_encode_taps) of the CALLER's header: members beyond it are never read, so a caller
                           built against an older (shorter) layout stays valid when members are appended */
  float* logmel;        /* (B, F, 224)  bn0 output (convnext.py:276-292) */
  float* stem;          /* (B, 252, 56, 96)  downsample_layers[0] output */
  float* stage_block0[4]; /* output of the first block of stage i */
  float* stage[4];      /* output of stage i */
  float* down[4];       /* output of downsample_layers[i], i = 1..3 ([0] unused) */
  float* block[18];     /* output of every ConvNeXt block in network order (stage 0 block 0 .. stage 3 block 2) */
} conette_encode_taps;

const char* conette_last_error(void);
int conette_abi_version(void);

/* Build a context from the reference state dict: `names[i]` is the
 * reference key (e.g. "preprocessor.encoder.stages.0.0.pwconv1.weight"), `tensors[i]` a dev
 * pointer to the contiguous fp32 tensor (bool tensors as uint8, int64 as int64), `numel[i]`
 * its element count.  Replaces module construction + load_state_dict of
 * huggingface/model.py:41-107,126-163.  Synchronous (runs once).
 * A list WITHOUT any "preprocessor.encoder." tensor creates a decoder-only context -- the reference's BaselinePLM family
 * (pl_modules/baseline.py:84-140: FrameIdentEncoder + projection + decoder over precomputed frame embeddings; the caller maps its
 * keys "projection.*" / "decoder.*" / "forbid_rep_mask" under "model."): conette_decode / conette_greedy / conette_forcing work,
 * conette_encode and conette_frontend_logmel return an error. */
int conette_create(const conette_config* cfg, int32_t n_tensors, const char* const* names,
                   const void* const* tensors, const int64_t* numel, conette_ctx** out);
void conette_destroy(conette_ctx* ctx);

/* Geometry helpers: STFT frames F = L/320 + 1; encoder frames T (convnext.py stem + 3 /2). */
int32_t conette_num_frames(int32_t n_samples);
int32_t conette_num_audio_frames(int32_t n_samples);

/* Bytes of caller-provided scratch needed by conette_encode / conette_decode. */
size_t conette_encode_workspace_bytes(const conette_ctx* ctx, int32_t batch, int32_t n_samples);
size_t conette_decode_workspace_bytes(const conette_ctx* ctx, int32_t batch, int32_t t_audio, int32_t beam,
                                      int32_t max_pred);

/* a2: log-mel frontend (convnext.py:270-292 + torchlibrosa Spectrogram/LogmelFilterBank + bn0).
 * wave: dev (B, L) fp32 mono @ 32 kHz, zero-padded to L.  out: dev (B, F, 224) fp32. */
int conette_frontend_logmel(conette_ctx* ctx, const float* wave, int32_t batch, int32_t n_samples, float* out,
                            void* stream);

/* a2-a7: ConvNeXt.forward (convnext.py:264-336) + the transpose of preprocessor.py:66.
 *   frame_embs : dev (B, T, 768) fp32      ("audio" of preprocessor.py:71-75)
 *   clip_probs : dev (B, 527) fp32         (sigmoid(head_audioset), convnext.py:324-334) */
int conette_encode(conette_ctx* ctx, const float* wave, int32_t batch, int32_t n_samples, float* frame_embs,
                   float* clip_probs, const conette_encode_taps* taps, void* workspace, size_t workspace_bytes,
                   void* stream);

/* The 16-bit precisions keep the encoder's residual stream in IEEE fp16 (|x| <= 65504).  A value beyond that is inf where the
 * fused MLP stored it and NaN after the next LayerNorm (convnext.py:61-66) -- and the saturating conversions further down the
 * encoder turn such NaNs back into finite garbage, so the frame embeddings do not reliably show it.  Every LayerNorm of
 * conette_encode that reads the stream (the next block's depthwise conv + LN, the downsample layers, the frame-mean head) counts
 * the positions whose statistics are not finite in one per-device counter.  This call waits for `stream`, returns the count
 * accumulated by the encodes of this process on the context's device since the previous call in *count and resets it.
 * Non-zero = some clip's embeddings are unusable in this precision: run it through a CONETTE_PREC_F16X2 / _F32 context (fp32
 * stream).  The ONE blocking entry point besides conette_create; a host that never calls it loses the diagnosis. */
int conette_encode_nonfinite(conette_ctx* ctx, void* stream, int32_t* count);

/* a9-a14: CoNeTTEPLM.encode_audio + decode_audio("generate") = nn/decoding/beam.py:22-227 with
 * the decoder of nn/decoders/aac_tfmer.py:71-118, KV-cached, whole search loop on device.
 *   frame_embs  : dev (B, T, 768) fp32           frame_lens : dev (B) int32 valid frames
 *   bos_ids     : dev (B) int32 task tokens      forbid_mask: dev (V) uint8 or NULL
 * Outputs (all dev, full width; trim on host with out_sizes):
 *   best_preds  (B, max_pred) int32   best_lprobs (B) fp32
 *   mult_preds  (B, beam, max_pred) int32   mult_lprobs (B, beam) fp32
 *   out_sizes   (2) int32: [0] = pred_size (beam.py:192-194,207-211), [1] = best_maxlen (:222-225)
 *   step0_logits: optional dev (B*beam, ld_v) fp32 copy of the step-0 logits (parity), or NULL
 *   trace_sel   : optional dev (max_pred, B, beam, 2) int32 = (parent row, token) picked by the
 *                 per-clip top-k of each step in descending order, -1 where unused; or NULL
 *   trace_val   : optional dev (max_pred, B, beam) fp32 running log-prob sums of those picks
 *   margins     : optional dev (B, 2, max_pred + 1) fp32, or NULL -- how far each decision of the search is from any other
 *                 outcome.  Plane [b][0] = MEMBERSHIP: [i], i < max_pred = last pick minus first rejected candidate of clip b's
 *                 top-k call of step i (_select_k_next_toks, beam.py:230-269) -- which candidates continue; [max_pred] = best
 *                 averaged log-prob minus the second best (the final choice, beam.py:214-217), +inf for beam 1.  Plane [b][1] =
 *                 ORDER: [i] = the smallest gap between consecutive picks of that call (their order assigns the slots,
 *                 beam.py:165-169: the order of mult_preds, never best_preds), +inf with one pick; [max_pred] unused (+inf).
 *                 +inf for steps the clip no longer takes; NaN = fewer finite candidates than picks.  A search whose margins
 *                 all exceed twice the precision's candidate error took the decisions an exact search takes: the certificate
 *                 behind the host's precision "certified" (conette_amd/engine.py), which re-runs only the other clips through a
 *                 CONETTE_PREC_F16X2 context; with plane 0 alone ("certified-best") best_preds / best_lprobs are certified and
 *                 mult_preds as a set of hypotheses.
 * beam <= 16 (1..8 on the register-resident step kernel, 9..16 -- BaselinePLM's default is 10, pl_modules/baseline.py:47 -- on
 * the generic one), max_pred <= 64.  With identical arguments (pointers included) the launch sequence is replayed from a cached
 * hipGraph from the third call on (see conette_set_option). */
int conette_decode(conette_ctx* ctx, const float* frame_embs, const int32_t* frame_lens, const int32_t* bos_ids,
                   const uint8_t* forbid_mask, int32_t batch, int32_t t_audio, int32_t beam,
                   int32_t min_pred, int32_t max_pred, int32_t* best_preds, float* best_lprobs,
                   int32_t* mult_preds, float* mult_lprobs, int32_t* out_sizes, float* step0_logits,
                   int32_t* trace_sel, float* trace_val, float* margins, void* workspace, size_t workspace_bytes,
                   void* stream);

/* teacher forcing (nn/decoding/forcing.py:12-71 as called by CoNeTTEPLM.decode_audio(..., "forcing",
 * caps_in=...), pl_modules/conette.py:392-417, after the projection of conette.py:457): the logits of every position of
 * given input captions under the causal mask, padded caption positions masked as keys
 * (tensor_to_pad_mask(caps_in, pad_value=pad_id)).
 *   caps_in : dev (B, cap_len) int32, column 0 = the task token that replaced <bos>, right-padded with pad_id
 *   logits  : dev (B, cap_len, vocab) fp32 -- the reference returns the same values permuted to (B, vocab, cap_len)
 * Runs the KV-cached step kernels of conette_decode with the next token taken from caps_in instead of the search. */
size_t conette_forcing_workspace_bytes(const conette_ctx* ctx, int32_t batch, int32_t t_audio, int32_t cap_len);
int conette_forcing(conette_ctx* ctx, const float* frame_embs, const int32_t* frame_lens, const int32_t* caps_in,
                    int32_t batch, int32_t t_audio, int32_t cap_len, float* logits, void* workspace,
                    size_t workspace_bytes, void* stream);

/* Scoring of given captions: what CoNeTTEPLM.validation_step / test_step compute from the forcing logits
 * (pl_modules/conette.py:233-256: decode_audio(..., "forcing") per reference caption, then CrossEntropyLossMean(ignore_index=pad_id,
 * dim=1), nn/loss/ce_mean.py:30-34) -- the log-probability of every target token, without the logits: the classifier GEMM, the
 * log-sum-exp over the vocabulary and the gather of the target's logit are one kernel, and no (rows, vocab) array exists
 * anywhere, the workspace included.  P = n_audio * caps_per_audio captions; caption p belongs to clip p / caps_per_audio, so the
 * projection and the cross-attention keys / values are computed once per CLIP however many captions are scored against it.
 *   caps_in    : dev (P, cap_len) int32, conette_forcing's contract (column 0 the task token, right-padded with pad_id, pads
 *                masked as keys); ids must lie in [0, vocab)
 *   targets    : dev (P, cap_len) int32, targets[p][t] = the token to be predicted at position t (the reference passes
 *                captions[:, 1:] for caps_in = captions[:, :-1])
 *   tok_lprobs : dev (P, cap_len) fp32 or NULL -- log_softmax(logits[p][t])[targets[p][t]]; exactly 0 where the target is pad_id,
 *                NaN where it lies outside [0, vocab) (the target is compared with column indices, never used as an address)
 *   sum_lprobs : dev (P) fp32, the sum over the caption's non-pad targets
 *   n_tokens   : dev (P) int32, their number -- the reference's per-caption loss is -sum_lprobs / n_tokens
 * cap_len <= 64, caps_per_audio >= 1.  Asynchronous on `stream`, capturable; results are bit-identical from run to run.  Works on
 * decoder-only contexts.  The workspace size depends on CONETTE_OPT_SCORE_VSPLIT as set when it is asked for. */
size_t conette_score_workspace_bytes(const conette_ctx* ctx, int32_t n_audio, int32_t t_audio, int32_t caps_per_audio,
                                     int32_t cap_len);
int conette_score(conette_ctx* ctx, const float* frame_embs, const int32_t* frame_lens, const int32_t* caps_in,
                  const int32_t* targets, int32_t n_audio, int32_t t_audio, int32_t caps_per_audio, int32_t cap_len,
                  float* tok_lprobs, float* sum_lprobs, int32_t* n_tokens, void* workspace, size_t workspace_bytes,
                  void* stream);

/* Word-to-audio alignment of given captions: conette_score's one causal pass with the decoder's cross-attention weights kept --
 * for every caption position a distribution over the clip's encoder frames (one frame = 32 STFT hops = 0.32 s at 32 kHz).
 * Row (p, t) belongs to the query at position t of caption p, the one that PREDICTS targets[p][t]; per layer the weights are the
 * mean over the 8 heads of softmax_frames(q_h . k_h / sqrt(32)), computed from the same scores, maxima and sums as the context
 * vector the layer goes on with (p_h = exp(s_h - m_h) * (1 / l_h), heads added in ascending order, times 1 / 8).
 *   caps_in, targets, P, cap_len, caps_per_audio : conette_score's contract; targets may be NULL: then the classifier is not run,
 *                and tok_lprobs, sum_lprobs and n_tokens must be NULL too (with targets, sum_lprobs and n_tokens are required and
 *                hold exactly conette_score's results)
 *   layer_mask  : bit l = decoder layer l takes part in `attn`; 0 = all layers; a bit at or above n_layers is an error
 *   attn        : dev (P, cap_len, t_audio) fp32, the mean over the selected layers in ascending order (sum, then times
 *                 1 / n_selected); no memset needed
 *   attn_layers : dev (n_layers, P, cap_len, t_audio) fp32 or NULL -- every layer's own weights, selected or not
 * Frames at or behind frame_lens[clip] are exactly 0, and so is every frame of a row whose caps_in token is pad_id, whatever the
 * buffers held; every other row sums to 1 up to rounding.  cap_len <= 64, caps_per_audio >= 1, t_audio unbounded.  Asynchronous on
 * `stream`, capturable; results are bit-identical from run to run.  Works on decoder-only contexts and in every precision.  The
 * workspace is conette_score's without the score partials unless `with_scores`; nothing of size rows x frames x heads exists. */
size_t conette_align_workspace_bytes(const conette_ctx* ctx, int32_t n_audio, int32_t t_audio, int32_t caps_per_audio,
                                     int32_t cap_len, int32_t with_scores);
int conette_align(conette_ctx* ctx, const float* frame_embs, const int32_t* frame_lens, const int32_t* caps_in,
                  const int32_t* targets, int32_t n_audio, int32_t t_audio, int32_t caps_per_audio, int32_t cap_len,
                  uint32_t layer_mask, float* attn, float* attn_layers, float* tok_lprobs, float* sum_lprobs, int32_t* n_tokens,
                  void* workspace, size_t workspace_bytes, void* stream);

/* greedy_search (nn/decoding/greedy.py:17-131; BaselinePLM's decoder, not reachable from
 * CoNeTTEPLM): the arg-max chain with the full masked logits of every step as output.
 *   logits : dev (B, max_pred, vocab) fp32 -- per step the logits of every unfinished clip with the EOS floor
 *            (greedy.py:96-97) and the forbid-repeat mask (:99-105) applied; finished clips hold (-inf, pad_id -> 0)
 *            (:64-69).  The reference returns the same values permuted to (B, vocab, pred_size).
 *   preds  : dev (B, max_pred) int32 arg-max tokens, pad_id after <eos>
 *   out_sizes[0] = pred_size (steps until every clip had finished), out_sizes[1] = longest caption incl. <eos> */
size_t conette_greedy_workspace_bytes(const conette_ctx* ctx, int32_t batch, int32_t t_audio, int32_t max_pred);
int conette_greedy(conette_ctx* ctx, const float* frame_embs, const int32_t* frame_lens, const int32_t* bos_ids,
                   const uint8_t* forbid_mask, int32_t batch, int32_t t_audio, int32_t min_pred, int32_t max_pred,
                   float* logits, int32_t* preds, int32_t* out_sizes, void* workspace, size_t workspace_bytes,
                   void* stream);

/* Sampling: n_samples stochastic captions per clip from the model's distribution, on the KV-cached step path of conette_decode
 * with a per-row sampling decision in place of the search step (csrc/dec_sample.h).  Rows r = clip * n_samples + sample never
 * change parents.  One decision, from the row's logits z, its prefix, the step and a uniform u in [0, 1):
 *   masks      z[eos] = -inf while step < min_pred; z[v] = -inf for every v with forbid_mask[v] set that occurs in the row's
 *              prefix, the task token at position 0 included -- as conette_decode applies them
 *   log-prob   log_softmax(masked z)[token], at temperature 1 and unfiltered: the quantity the beam search sums
 *   top-k      with y = z / temperature, v is kept iff fewer than top_k tokens have a strictly larger y (0 or >= vocab: off)
 *   top-p      with q = softmax(y over the top-k set), v is kept iff the total q of the tokens with strictly larger y is < top_p
 *              (1: off).  Both rules are tie-inclusive and always keep the arg-max.  "Larger y" is decided on z (temperature > 0: the
 *              same order in the reals), so two distinct logits never become a tie through the rounding of z / temperature.
 *   draw       q renormalised over the kept set, walked in ascending token id: the first token whose running sum exceeds u, or
 *              the largest kept id when rounding leaves the total <= u
 * A row finishes when it draws <eos>, or at step max_pred - 1 (the drawn token stays).  A row without a finite logit takes <eos>,
 * its log-prob becomes NaN, and it finishes.
 *   uniforms    : dev (max_pred, batch * n_samples) fp32 in [0, 1), step-major; entries of finished rows are ignored.  The
 *                 randomness is the caller's: the library holds no generator state
 *   preds       : dev (batch, n_samples, max_pred) int32, pad_id after the end
 *   sum_lprobs  : dev (batch, n_samples) fp32, the sum of the row's token log-probs in step order
 *   lens        : dev (batch, n_samples) int32, tokens including <eos>
 *   out_sizes   : dev (2) int32: [0] steps until every row had finished, [1] the longest caption
 *   tok_lprobs  : optional dev (batch, n_samples, max_pred) fp32, 0 after the end; or NULL
 *   step_logits : optional dev (batch * n_samples, max_pred, vocab) fp32, the RAW (unmasked) logits each decision saw; rows of
 *                 steps after the row finished are unspecified; or NULL
 * n_samples 1..16, max_pred <= 64, temperature finite and > 0, top_k >= 0, 0 < top_p <= 1, vocab <= 65536 (up to 8192 on the
 * register-resident kernel, beyond on the generic one).  Asynchronous on `stream`, capturable, never replayed from the decode graph
 * cache; results are bit-identical from run to run.  Works on decoder-only contexts and in every precision. */
size_t conette_sample_workspace_bytes(const conette_ctx* ctx, int32_t batch, int32_t t_audio, int32_t n_samples,
                                      int32_t max_pred);
int conette_sample(conette_ctx* ctx, const float* frame_embs, const int32_t* frame_lens, const int32_t* bos_ids,
                   const uint8_t* forbid_mask, const float* uniforms, int32_t batch, int32_t t_audio, int32_t n_samples,
                   int32_t min_pred, int32_t max_pred, float temperature, int32_t top_k, float top_p, int32_t* preds,
                   float* sum_lprobs, int32_t* lens, int32_t* out_sizes, float* tok_lprobs, float* step_logits,
                   void* workspace, size_t workspace_bytes, void* stream);

/* Diverse beam search (Vijayakumar et al. 2016; Hugging Face's num_beam_groups / diversity_penalty): n_groups * group_beam
 * deterministic, likely and DIFFERENT captions per clip, on the KV-cached step path of conette_decode with one search step per
 * decode step that goes through the clip's groups in sequence (csrc/dec_group.h; the CPU restatement of the rule is
 * conette_amd/group_search.py).  G = n_groups, W = group_beam, lambda = diversity_penalty.
 *   rows       clip b owns rows b * G * W ..; group g owns rows g * W .. g * W + W - 1 of the clip, its k_g live rows (W at the
 *              start) compacted to the front of its own range; a row's ancestors never leave its group
 *   one step i of a clip, groups g = 0 .. G - 1 in this order; a group with k_g == 0 takes no picks and adds nothing to the counts:
 *     candidates  the group's live rows (step 0: its first row only); logits masked as conette_decode masks them (EOS floor while
 *                 i < min_pred, forbid-repeat over the row's own prefix, position 0 included); lp = log_softmax of the masked
 *                 row, (z - max) - log(sum), in fp32
 *     model score m(p, v) = sum_lp[p] + lp[p][v] (step 0: lp)
 *     counts      c[v] = the number of picks made AT THIS STEP by groups 0 .. g - 1 of this clip whose token is v; every pick
 *                 counts, those that finish included
 *     key         s(p, v) = m if c[v] == 0, else m - lambda * c[v]: one rounded fp32 multiply, then one rounded fp32 subtract
 *     picks       the top k_g keys over the group's k_g * V candidates; ties go to the lowest flat index p_in_group * V + v
 *     carried     a pick carries its MODEL SCORE m, never its key: running sums and returned scores are the model's
 *                 log-probabilities of the caption
 *     bookkeeping conette_decode's, per group: a pick of <eos>, or any pick at step max_pred - 1, goes to output slot
 *                 g * W + (the slot of its row) with score m / (i + 1) and leaves; the others continue with a smaller k_g
 * Outputs as conette_decode's with beam = G * W: mult_preds (B, G * W, max_pred) / mult_lprobs (B, G * W) in slot order, group-major;
 * best_* = the first maximum of the averaged score over all G * W slots; out_sizes; no `margins` (no certificate is defined for
 * this search) and no step0_logits.
 *   trace_sel   : optional dev (max_pred, B, G * W, 2) int32 = (within-clip parent row, token) of the picks of group g at positions
 *                 g * W + pick, in descending key order, -1 where unused; or NULL
 *   trace_val   : optional dev (max_pred, B, G * W) fp32, the carried model sums of those picks
 *   step_logits : optional dev (max_pred, B * G * W, vocab) fp32, the RAW (unmasked) logits of the rows as they stood when that
 *                 step decided; the rows of a clip all of whose groups have finished are unspecified; or NULL
 * With n_groups == 1 the search is conette_decode at beam group_beam, bit for bit, for any lambda; group 0 is that search for any
 * G and lambda, and with lambda == 0 every group is (on equal logits: the decoder runs G * W rows per clip, not W).
 * n_groups >= 1, group_beam >= 1, n_groups * group_beam <= 16 (up to 8 with vocab <= 8192 on the register-resident kernel, beyond
 * on the generic one), diversity_penalty finite and >= 0, max_pred <= 64.  The workspace is conette_decode's at beam G * W plus the
 * groups' counters.  Asynchronous on `stream`, capturable, never replayed from the decode graph cache; results are bit-identical
 * from run to run.  Works on decoder-only contexts and in every precision. */
size_t conette_decode_groups_workspace_bytes(const conette_ctx* ctx, int32_t batch, int32_t t_audio, int32_t n_groups,
                                             int32_t group_beam, int32_t max_pred);
int conette_decode_groups(conette_ctx* ctx, const float* frame_embs, const int32_t* frame_lens, const int32_t* bos_ids,
                          const uint8_t* forbid_mask, int32_t batch, int32_t t_audio, int32_t n_groups, int32_t group_beam,
                          float diversity_penalty, int32_t min_pred, int32_t max_pred, int32_t* best_preds, float* best_lprobs,
                          int32_t* mult_preds, float* mult_lprobs, int32_t* out_sizes, int32_t* trace_sel, float* trace_val,
                          float* step_logits, void* workspace, size_t workspace_bytes, void* stream);

/* Ensemble beam search: conette_decode at beam `beam` whose candidates are scored by M = n_members (1..4) members -- several
 * checkpoints, or one checkpoint under several task tokens -- that decode ONE hypothesis tree in lockstep, the top-k running on the
 * combined scores inside the one search-step launch per decode step (csrc/dec_ensemble.h; the CPU restatement of the rule is
 * conette_amd/ensemble_search.py).
 *   members     : host array of n_members records.  ctx: the member's context (the same context may appear more than once);
 *                 frame_embs: dev (B, t_audio, 768) fp32, its audio memory; bos_ids: dev (B) int32, its task token per clip;
 *                 weight: finite and > 0 -- the caller normalises the weights to sum 1 (the library uses them as given);
 *                 workspace / workspace_bytes: its own, conette_decode_ensemble_workspace_bytes(ctx, ...) bytes; the members' ranges
 *                 must not overlap (refused)
 *   combine     : CONETTE_COMBINE_LOGPROB  c(p, v) = sum_m w_m * lp_m(p, v)            (product of experts; -inf where any member is)
 *                 CONETTE_COMBINE_PROB     c(p, v) = log sum_m w_m * exp(lp_m(p, v))   (mixture; -inf only where every member is;
 *                                          accumulated around a running maximum, so it never underflows where some lp_m is finite)
 *                 with one member c = lp_0 under either rule, no arithmetic
 *   lp_m(p, .)  = the log-softmax of member m's logits of candidate row p, masked as conette_decode masks them (EOS floor while
 *                 step < min_pred, forbid-repeat over the row's prefix WITH MEMBER m's OWN TASK TOKEN at position 0): bit for bit what
 *                 conette_decode's step computes for member m on that prefix
 *   score       sum_lp[p] + c(p, v) (step 0: c); top-k over the k * V candidates, ties to the lowest flat index, finished picks to their
 *               slot with score / (step + 1), the shortage rule: all conette_decode's.  The returned scores are the combined ones.
 * Shared by the members: frame_lens, t_audio, forbid_mask, beam (1..16), min_pred, max_pred, and the vocabulary size, eos and pad ids
 * and the precision of their contexts (a difference is an error).  Every decode step runs every member's forward on that member's
 * workspace, one after another on `stream`, against the search state in member 0's workspace; at step 0 a member embeds its own
 * task tokens, afterwards the shared current tokens.
 * Outputs as conette_decode's (best_*, mult_*, out_sizes, optional trace_sel / trace_val / margins), and
 *   step_logits : optional dev (max_pred, M, B * beam, ldv) fp32, ldv = vocab rounded up to a multiple of 8: the RAW (unmasked) logits
 *                 of every member as they stood when that step decided (rows that no longer search are unspecified); or NULL
 * With one member the result is conette_decode's bit for bit; so it is with 2 or 4 copies of one member (same context, same task
 * tokens, separate workspaces) at equal weights under CONETTE_COMBINE_LOGPROB.  A failing call names the argument, launches nothing
 * and leaves the outputs untouched.  Replayed from the decode graph cache of members[0].ctx (keyed on every member's context --
 * pointer, creation serial and decode-fusion option --, buffers, workspace, weight and the rule); asynchronous on `stream`; bit-identical from run to
 * run.  Works on decoder-only contexts and in every precision. */
#define CONETTE_COMBINE_LOGPROB 0
#define CONETTE_COMBINE_PROB 1
typedef struct conette_member {
  conette_ctx* ctx;
  const float* frame_embs;
  const int32_t* bos_ids;
  float weight;
  void* workspace;
  size_t workspace_bytes;
} conette_member;
size_t conette_decode_ensemble_workspace_bytes(const conette_ctx* ctx, int32_t batch, int32_t t_audio, int32_t beam,
                                               int32_t max_pred); /* per member */
int conette_decode_ensemble(const conette_member* members, int32_t n_members, int32_t combine, const int32_t* frame_lens,
                            const uint8_t* forbid_mask, int32_t batch, int32_t t_audio, int32_t beam, int32_t min_pred,
                            int32_t max_pred, int32_t* best_preds, float* best_lprobs, int32_t* mult_preds, float* mult_lprobs,
                            int32_t* out_sizes, int32_t* trace_sel, float* trace_val, float* margins, float* step_logits,
                            void* stream);

/* Constrained beam search: conette_decode at beam W = `beam` (1..16) whose caller steers the search -- a forced beginning per
 * clip, tokens that never appear, no n-gram twice -- inside the one search-step launch per decode step (csrc/dec_constrain.h; the
 * CPU restatement of the rule is conette_amd/constrained_search.py).
 *   prefix      : dev (B, prefix_width) int32; prefix_lens : dev (B) int32, 0 <= plen[b] <= prefix_width <= max_pred - 1 (values
 *                 outside are clamped).  With prefix_width == 0 both may be NULL.  The tokens prefix[b][:plen[b]] must lie in
 *                 [0, vocab) and be neither <eos> nor pad: the caller's contract (a token outside the vocabulary, or <eos>, is
 *                 treated as a token whose score is not finite, below)
 *   ban_mask    : dev (vocab) uint8 or NULL;  no_repeat_ngram : n, 0 (off) .. 64
 * A row's sequence at step i is s_0 (the task token), s_1 .. s_i; a candidate's token becomes s_{i+1}.
 *   masks on the raw logits z of a candidate row at step i:
 *     M1  conette_decode's: the EOS floor while i < min_pred, forbid-repeat over s_0 .. s_i
 *     M2  z[v] = -inf where ban_mask[v] != 0
 *     M3  (n >= 1) for every j with 0 <= j <= i - n + 1 for which s_j .. s_{j+n-2} equals s_{i-n+2} .. s_i (n - 1 tokens; with
 *         n = 1 the comparison is empty and always true): z[s_{j+n-1}] = -inf.  Position 0 takes part, as in forbid-repeat
 *     then lp = (z - max) - log(sum) in fp32, summed in the order of the kernel conette_decode runs at this (vocab, W)
 *   calls of clip b at step i; model score m = sum_lp[p] + lp[p][v] (i = 0: lp):
 *     forced   (i < plen[b]) the only candidate is (row 0, t = prefix[b][i]).  m finite: row 0 goes on with t and carries m, the
 *              clip keeps its W live rows, trace position 0 = (0, t), the others -1, trace_val = m.  m not finite: every one of
 *              the clip's W slots becomes void and the clip leaves the search
 *     fan-out  (i == plen[b]) candidates: the V tokens of row 0; k = W picks (plen 0: conette_decode's step 0)
 *     later    conette_decode's step over the k live rows
 *     picks    the top k FINITE m, ties to the lowest flat index p * V + v; with only f < k finite candidates there are f picks
 *              and the slots of row positions f .. k - 1 become void; no index is formed from a pick that does not exist
 *     void slot  mult_lprobs = -inf, length 0, pad_id throughout; best_* is the first maximum as ever (all slots void:
 *              best_lprobs = -inf, best_preds all pad)
 *     bookkeeping  conette_decode's: a finished hypothesis scores m / (i + 1), prefix tokens count in the sum and in the length
 * The result is the beam search restricted to captions that begin with the prefix; with no mask active its score is what
 * conette_score gives for the returned caption.  With prefix_width == 0, ban_mask == NULL and n == 0 it is conette_decode, bit for
 * bit.  Outputs as conette_decode_groups: best / mult / out_sizes, optional trace_sel (max_pred, B, W, 2) / trace_val (max_pred, B, W),
 * optional step_logits (max_pred, B * W, vocab), RAW; no `margins`, no step0_logits.  The workspace is conette_decode's at beam W.
 * Asynchronous on `stream`, capturable, never replayed from the decode graph cache; results are bit-identical from run to run.
 * Works on decoder-only contexts and in every precision. */
size_t conette_decode_constrained_workspace_bytes(const conette_ctx* ctx, int32_t batch, int32_t t_audio, int32_t beam,
                                                  int32_t max_pred);
int conette_decode_constrained(conette_ctx* ctx, const float* frame_embs, const int32_t* frame_lens, const int32_t* bos_ids,
                               const uint8_t* forbid_mask, const int32_t* prefix, const int32_t* prefix_lens, int32_t prefix_width,
                               const uint8_t* ban_mask, int32_t no_repeat_ngram, int32_t batch, int32_t t_audio, int32_t beam,
                               int32_t min_pred, int32_t max_pred, int32_t* best_preds, float* best_lprobs, int32_t* mult_preds,
                               float* mult_lprobs, int32_t* out_sizes, int32_t* trace_sel, float* trace_val, float* step_logits,
                               void* workspace, size_t workspace_bytes, void* stream);

/* Keyword-guided beam search: conette_decode_constrained whose every caption must hold a token of each of a clip's G <= 8
 * requirement groups (dynamic beam allocation) -- inside the same one search-step launch per decode step (csrc/dec_require.h; the
 * CPU restatement of the rule is conette_amd/required_search.py).  Arguments and outputs are conette_decode_constrained's, plus
 *   req_tokens  : dev (B, req_width) int32, the clip's required tokens;  req_groups : dev (B, req_width) int32, the group 0 .. 7 of
 *                 each, -1 = unused entry (any order, gaps allowed).  0 <= req_width <= 32; with req_width == 0 both may be NULL.
 *                 The caller's contract: no token in two groups of a clip, none is <eos>, pad, <bos>, the clip's task token or a
 *                 banned token, and the groups the prefix leaves unmet number at most max_pred - plen[b].  A group index outside
 *                 -1 .. 7 is an argument error: the table is read back for that check, so the call waits for `stream` (not while
 *                 the stream is capturing: there such an entry, like a token outside the vocabulary or one an earlier entry of the
 *                 clip holds, counts as unused)
 * Group g of a row is MET when one of its tokens occurs among s_1 .. s_i (prefix tokens count); unmet(p) = unmet groups of row p,
 * c(p) = G - unmet(p).  A row's state is derived from its own sequence: the search carries nothing new.
 *   masks, after M1 .. M3, on every call of a row, forced calls included:
 *     M4  while unmet(p) > 0: z[eos] = -inf
 *     M5  if unmet(p) >= max_pred - i: z[v] = -inf for every v that is no token of one of the row's unmet groups
 *   banks    candidate (p, v) is in bank c(p) + 1 if v belongs to an unmet group of row p, else in bank c(p)
 *   picks of a free call with k slots: per bank the candidates are ordered by descending finite m, ties to the lowest flat index
 *            p * V + v; the slots are dealt round-robin from the highest non-empty bank to the lowest, again and again, skipping
 *            exhausted banks, until k picks or until no finite candidate is left.  Pick order is deal order (trace_sel / trace_val,
 *            and which row goes on in which position).  Fewer finite candidates than k: void slots, as conette_decode_constrained
 *   forced calls are conette_decode_constrained's, under M4 / M5
 * Under the caller's contract every hypothesis that is not void holds a token of every group and ends in <eos> or at max_pred; M5
 * can leave a call fewer finite candidates than slots (a fan-out with fewer unmet-group tokens than W), which gives void slots, never
 * an indexed non-pick.  With req_width == 0, and
 * for every clip without a used entry, the result is conette_decode_constrained's, bit for bit.  The workspace is
 * conette_decode's at beam W.  Capturable, never replayed from the decode graph cache; results are bit-identical from run to run.
 * Works on decoder-only contexts and in every precision. */
size_t conette_decode_required_workspace_bytes(const conette_ctx* ctx, int32_t batch, int32_t t_audio, int32_t beam, int32_t max_pred);
int conette_decode_required(conette_ctx* ctx, const float* frame_embs, const int32_t* frame_lens, const int32_t* bos_ids,
                            const uint8_t* forbid_mask, const int32_t* prefix, const int32_t* prefix_lens, int32_t prefix_width,
                            const uint8_t* ban_mask, int32_t no_repeat_ngram, const int32_t* req_tokens, const int32_t* req_groups,
                            int32_t req_width, int32_t batch, int32_t t_audio, int32_t beam, int32_t min_pred, int32_t max_pred,
                            int32_t* best_preds, float* best_lprobs, int32_t* mult_preds, float* mult_lprobs, int32_t* out_sizes,
                            int32_t* trace_sel, float* trace_val, float* step_logits, void* workspace, size_t workspace_bytes,
                            void* stream);

/* Consensus (minimum-Bayes-risk) choice among candidate captions: per clip the candidate that agrees most with all the others, each
 * weighted by the evidence for it (csrc/dec_consensus.h; the CPU statement of the rule, its fp32 arithmetic included, is
 * conette_amd/consensus.py).  Takes no context and no workspace: one launch, one workgroup per clip.
 *   preds    : dev (B, n_cands, row_len) int32, any ids in 0 .. 2^31 - 1 (compared as whole words)
 *   lens     : dev (B, n_cands) int32 or NULL.  Given (conette_sample's `lens`, <eos> included; clamped to 0 .. row_len): the content
 *              of a candidate is row[:len] without its last token if that is eos_id.  NULL: the tokens in front of the first eos_id or
 *              pad_id of the row, the whole row if neither occurs.  A content may be empty
 *   weights  : dev (B, n_cands) fp32 or NULL -- finite, > 0, normalised to sum 1 per clip by the caller (used as given); NULL: every
 *              weight is fp32(1) / fp32(n_cands)
 *   utility  : CONETTE_UTILITY_NGRAM  u(i, j) = the mean over the orders n = 1 .. max_order that count of F_n = 2 m_n / (t_i + t_j),
 *                                     t_i = max(|c_i| - n + 1, 0), m_n = the clipped n-gram match (sum over distinct n-grams of the
 *                                     smaller count); an order with t_i + t_j = 0 does not count; u = 1 when none counts
 *              CONETTE_UTILITY_EDIT   u(i, j) = 1 - levenshtein(c_i, c_j) / max(|c_i|, |c_j|) at unit costs; 1 when both are empty
 *   max_order: 1 .. 4 (checked under either utility, read by CONETTE_UTILITY_NGRAM)
 *   expected : dev (B, n_cands) fp32, E_i = sum_j w_j u(i, j), j = 0 .. n_cands - 1 in this order, i included
 *   best     : dev (B) int32, the first index of the maximum E
 *   margin   : dev (B) fp32, E[best] minus the largest E at any other index: +inf with one candidate, 0 when a duplicate ties
 *   pairwise : dev (B, n_cands, n_cands) fp32 or NULL, u itself (symmetric, diagonal 1)
 * Counts and distances are exact integers and every fp32 operation is rounded on its own in the order consensus.py fixes (one
 * division per F_n, the orders added in ascending n, one division by their number; products w_j u(i, j) added from 0 in ascending j,
 * no fused multiply-add): the results equal consensus.select_fp32 bit for bit.  1 <= n_cands <= CONETTE_MAX_CANDS, 1 <= row_len <= 64.
 * A failing call names the argument and launches nothing.  Asynchronous on `stream`, allocates nothing, capturable; bit-identical from
 * run to run. */
#define CONETTE_UTILITY_NGRAM 0
#define CONETTE_UTILITY_EDIT 1
#define CONETTE_MAX_CANDS 64
int conette_consensus(const int32_t* preds, const int32_t* lens, const float* weights, int32_t batch, int32_t n_cands,
                      int32_t row_len, int32_t utility, int32_t max_order, int32_t eos_id, int32_t pad_id, float* expected,
                      int32_t* best, float* margin, float* pairwise, void* stream);

/* Tag timeline: WHEN each AudioSet tag is heard in a clip (csrc/enc_tags.h; the CPU statement of both rules is
 * conette_amd/tagging.py).  conette_tag_frames runs the clip head -- max over time + mean over time, LayerNorm, head_audioset,
 * sigmoid -- over a window of frames around every frame instead of over the whole clip:
 *   frame_embs : dev (B, t_audio, 768) fp32, conette_encode's output (0.32 s per frame)
 *   frame_lens : dev (B) int32, the valid frames of each clip (clamped to 0 .. t_audio).  Frames at or beyond it are never read
 *   window     : 1 .. CONETTE_TAG_MAX_WINDOW frames; frame t pools the frames max(0, t - (window - 1) / 2) ..
 *                min(len, t + window / 2 + 1) - 1, summed in ascending order in fp32.  A window of 2 t_audio - 1 covers the clip at
 *                every t: each row is then conette_encode's clip_probs
 *   frame_probs: dev (B, t_audio, 527) fp32; rows t >= frame_lens[b] are exact zeros.  Every element is written
 *   workspace  : conette_tag_frames_workspace_bytes(ctx, batch, t_audio) bytes (the head GEMM's operand rows)
 * The head's product runs in the context's precision, like conette_encode's.  A decoder-only context has no clip head: CN_ERR_ARG.
 * conette_tag_events turns probabilities into events per (clip, tag), with no context and no workspace, one thread per sequence:
 *   frame_probs  : dev (B, t_audio, n_tags) fp32 -- conette_tag_frames' output or any other table; compared in fp32, NaN below all
 *   on_threshold / off_threshold : finite, 0 < off <= on <= 1.  A run is a maximal stretch of frames t < len with p >= off that
 *                  holds a frame with p >= on (hysteresis; off = on: plain thresholding)
 *   max_gap      : >= 0; a run that starts at most max_gap frames after the (exclusive) end of the event before it joins that event
 *   min_frames   : >= 0; after merging, an event shorter than this (end - start) is dropped
 *   max_events   : 1 .. CONETTE_TAG_MAX_EVENTS slots per sequence, filled in time order
 *   spans        : dev (B, n_tags, max_events, 2) int32 (start, end), end exclusive; unused slots (-1, -1)
 *   peaks        : dev (B, n_tags, max_events) fp32, the largest p of the event (its bits); unused slots 0
 *   peak_frames  : dev (B, n_tags, max_events) int32, the first frame that holds the peak; unused slots -1
 *   counts       : dev (B, n_tags) int32, the true number of events, which may exceed max_events
 * Every element of the four outputs is written by every call.  A failing call names the argument (CN_ERR_ARG; a short workspace:
 * CN_ERR_WORKSPACE) and launches nothing.  Both calls are asynchronous on `stream`, allocate nothing, are capturable and
 * bit-identical from run to run. */
#define CONETTE_TAG_MAX_WINDOW 255
#define CONETTE_TAG_MAX_EVENTS 64
size_t conette_tag_frames_workspace_bytes(const conette_ctx* ctx, int32_t batch, int32_t t_audio);
int conette_tag_frames(conette_ctx* ctx, const float* frame_embs, const int32_t* frame_lens, int32_t batch, int32_t t_audio,
                       int32_t window, float* frame_probs /* (B, t_audio, 527) */, void* workspace, size_t workspace_bytes, void* stream);
int conette_tag_events(const float* frame_probs, const int32_t* frame_lens, int32_t batch, int32_t t_audio, int32_t n_tags,
                       float on_threshold, float off_threshold, int32_t min_frames, int32_t max_gap, int32_t max_events,
                       int32_t* spans /* (B, n_tags, max_events, 2) */, float* peaks, int32_t* peak_frames /* (B, n_tags, max_events) */,
                       int32_t* counts /* (B, n_tags) */, void* stream);

/* Caption timeline: captions of SPANS of long recordings that were encoded once, and the rule that merges the captions of a
 * window grid into segments (csrc/dec_spans.h, csrc/dec_segments.h; the CPU statement of the grid and the rule is
 * conette_amd/segments.py).  conette_decode_spans is conette_decode's beam search over n_spans clips, each a span of one of n_rec
 * recordings:
 *   frame_embs : dev (n_rec, t_rec, 768) fp32, conette_encode's output
 *   spans      : dev (n_spans, 3) int32 rows of (recording, start, len) in frames.  Read on the device by every call (a replayed
 *                graph follows a table whose contents changed behind the same address) and clamped there -- recording to
 *                0 .. n_rec - 1, start to 0 .. t_rec - 1, len to 1 .. min(t_span, t_rec - start) -- so that no table makes a kernel
 *                read out of bounds; checking that a span lies inside its recording's valid frames is the caller's job
 *   bos_ids    : dev (n_spans) int32       forbid_mask: dev (V) uint8 or NULL
 *   t_span     : the width of the span axis, at least the longest len
 *   best_preds (n_spans, max_pred), best_lprobs (n_spans), mult_preds (n_spans, beam, max_pred), mult_lprobs (n_spans, beam),
 *   out_sizes (2): as conette_decode's, over the n_spans clips.  No trace, margin or step-0 outputs.
 * Span s is searched exactly as conette_decode searches a clip whose valid frames are frame_embs[rec, start : start + len] with
 * t_audio = t_span; frames outside a span are never attended.  The precision conversion, the 768 -> 256 projection and the
 * cross-attention K/V of all layers are computed once per recording FRAME, however many spans hold it (the audio memory carries no
 * positional encoding), and gathered per span.  Limits as conette_decode's (beam <= 16, max_pred <= 64), n_spans <= 65535.  Works
 * on decoder-only contexts and in every precision; replayed from the context's decode graph cache like conette_decode.
 * conette_segments merges windows 0 .. n_windows[r] - 1 (in time order) of recording r into segments, with no context:
 *   preds      : dev (n_rec, w_max, row_len) int32, the windows' best captions; content = the tokens in front of the first eos_id / pad_id
 *   n_windows  : dev (n_rec) int32, clamped to 0 .. w_max; windows at or beyond it are never read
 *   win_spans  : dev (n_rec, w_max, 2) int32 (start, len) in frames      lprobs: dev (n_rec, w_max) fp32
 *   utility, max_order: conette_consensus's pair utility u; a_k = u(k, k + 1)
 *   threshold  : finite; window k + 1 joins the run of window k iff a_k >= threshold (fp32)
 *   max_run    : a run that has reached max_run windows closes anyway; 0: no cap
 *   max_segments: 1 .. CONETTE_SEG_MAX_SEGMENTS slots per recording, filled in time order
 *   adjacency  : dev (n_rec, w_max - 1) fp32 or NULL, a_k; exact zeros beyond n_windows - 2
 *   seg_windows: dev (n_rec, max_segments, 2) int32 (first, end) windows, end exclusive; unused slots (-1, -1)
 *   seg_frames : dev (n_rec, max_segments, 2) int32 (start, end) frames: the first segment starts at start_0, the last ends at
 *                start + len of the last window, and two neighbours meet at (start_{k+1} + start_k + len_k + 1) / 2 (floor), k the
 *                last window of the earlier one; unused slots (-1, -1)
 *   seg_rep    : dev (n_rec, max_segments) int32, the run's window with the largest lprob (the first on ties; a NaN never wins, the
 *                first window if all are NaN); unused slots -1
 *   seg_agree  : dev (n_rec, max_segments) fp32, the smallest a_k inside the run (its bits), 1 for a run of one window; unused slots 0
 *   counts     : dev (n_rec) int32, the true number of segments, which may exceed max_segments
 *   workspace  : NULL when `adjacency` is given; otherwise n_rec * (w_max - 1) * 4 bytes
 * Every element of every output is written by every call; the results equal segments.merge_batch bit for bit.  row_len <= 64,
 * w_max <= CONETTE_SEG_MAX_WINDOWS.  A failing call of either names the argument (CN_ERR_ARG; a short workspace: CN_ERR_WORKSPACE)
 * and launches nothing.  Both are asynchronous on `stream`, allocate nothing, are capturable and bit-identical from run to run. */
#define CONETTE_SEG_MAX_WINDOWS 4096
#define CONETTE_SEG_MAX_SEGMENTS 256
size_t conette_decode_spans_workspace_bytes(const conette_ctx* ctx, int32_t n_rec, int32_t t_rec, int32_t n_spans, int32_t t_span,
                                            int32_t beam, int32_t max_pred);
int conette_decode_spans(conette_ctx* ctx, const float* frame_embs, const int32_t* spans, const int32_t* bos_ids,
                         const uint8_t* forbid_mask, int32_t n_rec, int32_t t_rec, int32_t n_spans, int32_t t_span, int32_t beam,
                         int32_t min_pred, int32_t max_pred, int32_t* best_preds, float* best_lprobs, int32_t* mult_preds,
                         float* mult_lprobs, int32_t* out_sizes, void* workspace, size_t workspace_bytes, void* stream);
int conette_segments(const int32_t* preds, const int32_t* n_windows, const int32_t* win_spans, const float* lprobs, int32_t n_rec,
                     int32_t w_max, int32_t row_len, int32_t utility, int32_t max_order, float threshold, int32_t max_run,
                     int32_t max_segments, int32_t eos_id, int32_t pad_id, float* adjacency, int32_t* seg_windows,
                     int32_t* seg_frames, int32_t* seg_rep, float* seg_agree, int32_t* counts, void* workspace,
                     size_t workspace_bytes, void* stream);

/* a1: torchaudio.functional.resample (preprocessor.py:134-141), sinc_interpolation width 6,
 * rolloff 0.99.  in: dev (rows, n_in) fp32; out: dev (rows, n_out), n_out = ceil(n_in*new/orig). */
int conette_resample(const float* in, int32_t rows, int32_t n_in, int32_t orig_sr, int32_t new_sr, float* out,
                     void* stream);
int32_t conette_resample_len(int32_t n_in, int32_t orig_sr, int32_t new_sr);

/* CU-partitioned streams (hipExtStreamCreateWithCUMask).  The decode phase is a chain of ~10^3 tiny
 * dependent launches; sharing the whole chip with the encoder's big grids makes every one of them
 * queue behind resident encoder workgroups.  Giving the decode stream a private slice of CUs and
 * the encode stream the complement lets both phases of consecutive batches run side by side.
 * mask_words: 32-bit words, bit i = CU i enabled; returns a hipStream_t in *out_stream. */
int conette_stream_create_masked(const uint32_t* mask_words, int32_t n_words, void** out_stream);
int conette_stream_destroy(void* stream);

/* Runtime options. */
#define CONETTE_OPT_DECODE_GRAPH 1 /* 1 (default): replay conette_decode from a cached hipGraph */
#define CONETTE_OPT_DECODE_FUSION 2 /* 1 (default): fused decoder-layer kernels (bf16); 0: one launch per sub-layer */
#define CONETTE_OPT_ENCODE_RESERVED_CUS 3 /* default 0: compute units the encoder's persistent kernels leave free, so that
                                            the small dependent kernels of a conette_decode running on another stream are
                                            not queued behind them (0 .. n_cu / 2) */
#define CONETTE_OPT_FORCING_STEPWISE 4 /* default 0: conette_forcing is one causal pass over all caption positions
                                         (forcing.py:12-71); 1: the KV-cached step kernels fed with the caption */
#define CONETTE_OPT_SCORE_VSPLIT 5 /* default 0: conette_score picks the number of vocabulary slabs its fused kernel's grid is
                                     split into from the row count and the compute units (1 at large row counts); k >= 1:
                                     k slabs, clamped to the number of 128-column tiles of the vocabulary (tests, measurements) */
int conette_set_option(conette_ctx* ctx, int32_t option, int32_t value);

/* Kernel / copy nodes of the decode hipGraph that conette_decode launched (or captured) most recently on this context
 * (0: none yet): the launch count of that whole search, for bench.py's decode roofline entry. */
int32_t conette_decode_graph_nodes(const conette_ctx* ctx);
/* Decode graphs a context keeps (least recently used evicted beyond it; the evicting call waits for the evicted graph's own
 * last launch, outside the context's cache lock).  A caller that cycles through more (shape, buffer) keys than this replays nothing. */
#define CONETTE_MAX_DECODE_GRAPHS 64

/* Per-kernel-class timing with HIP events recorded on the caller's stream around each launch
 * of the selected classes (bench.py's roofline leg).  While a decoder class is selected, decode
 * graphs are bypassed.  conette_profile_read synchronises the recorded events, ADDS the elapsed
 * milliseconds / launch counts per class into ms[CONETTE_PROF_NCLASS] / counts[...] and
 * clears the recording. */
#define CONETTE_PROF_FRONTEND 0
#define CONETTE_PROF_STEM 1
#define CONETTE_PROF_DWCONV_LN 2
#define CONETTE_PROF_PW1_GEMM 3
#define CONETTE_PROF_PW2_GEMM 4
#define CONETTE_PROF_DOWNSAMPLE 5
#define CONETTE_PROF_HEADS 6
#define CONETTE_PROF_DEC_PREPARE 7
#define CONETTE_PROF_DEC_GEMM 8
#define CONETTE_PROF_DEC_ATTN 9
#define CONETTE_PROF_DEC_MISC 10
#define CONETTE_PROF_SEARCH 11
#define CONETTE_PROF_NCLASS 12
int conette_profile_enable(conette_ctx* ctx, uint32_t class_mask);
int conette_profile_read(conette_ctx* ctx, float* ms, int32_t* counts);

#ifdef __cplusplus
}
#endif
#endif /* CONETTE_HIP_H */
