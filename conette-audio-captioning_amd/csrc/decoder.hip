// Task-embedded Transformer decoder under beam search, KV-cached, whole loop on device
// (rows a9-a14 of SURVEY.md section 8a).
//
// Reference: pl_modules/conette.py:452-467 (projection + pad mask), nn/decoders/aac_tfmer.py:71-118
// (embedding * sqrt(d) + PE, 6 post-norm torch TransformerDecoderLayer, classifier),
// nn/decoding/beam.py:22-269 (search).  The reference re-decodes the whole prefix and
// re-projects the audio memory at every step, and replicates the memory per beam; here
//   * the cross-attention K/V of all layers are projected once per clip and shared by its beams,
//   * self-attention K/V are cached per (layer, step, row); beams are re-ordered through a
//     small ancestor table instead of moving the cache,
//   * EOS floor, forbid-repeat mask, log-softmax, running sums, per-clip top-k and the
//     finished / shrinking-k bookkeeping run in one kernel per step with no host sync.
// This file is the host side: workspace, launch sequences, the hipGraph cache and the entry points.  The device code is in
// dec_rows.h (row-wise kernels), dec_search.h (search step), dec_sample.h, dec_group.h, dec_constrain.h, dec_require.h, dec_ensemble.h, dec_block.h, dec_ffn.h, dec_score.h, dec_align.h and dec_spans.h.
#include "ctx.h"
#include <stdlib.h>

#include <type_traits>

#include "gemm2.h"
#include "dec_ffn.h"
#include "dec_score.h"
#include "dec_rows.h"
#include "dec_search.h"
#include "dec_sample.h"
#include "dec_group.h"
#include "dec_constrain.h"
#include "dec_require.h"
#include "dec_align.h"
#include "dec_ensemble.h"
#include "dec_spans.h"

#define FF2_SPLITS 8
static int ff2_splits_default() { return 4; }  // split-K slabs of the unfused FFN2 GEMM at small R

// ---------------------------------------------------------------------------------------------
// workspace + orchestration
// ---------------------------------------------------------------------------------------------

struct DecWs {
  void *fe_t, *mem, *kvc, *xt, *attn_t, *ffh, *kc, *vc;
  float *x, *x2, *qkv, *q, *tmp, *logits, *slabs;
  int *n_active, *slot, *prefix, *anc, *cur_tok, *out_len, *eos_idx;
  int* live;  // [CN_MAX_PRED + 2] rows still searching when step s starts (summed by the search step of s - 1)
  unsigned long long* kvalid;  // teacher forcing: bit s of row r = caption position s is not padding
  float* sum_lp;
  int ldv;
  size_t total;
};

// `lean` (conette_score): no logits, no KV cache -- the one-pass layer loop uses neither, and scoring must not hold an (R, V) array
static DecWs dec_ws(const conette_ctx* ctx, int B, int Ta, int beam, int maxp, char* base, bool lean = false) {
  const size_t es = ctx->esize;
  const int d = ctx->cfg.d_model, NL = ctx->cfg.n_layers, R = B * beam;
  DecWs w;
  size_t off = 0;
  auto take = [&](size_t bytes) {
    char* p = base ? base + off : nullptr;
    off += cn_align(bytes);
    return p;
  };
  w.ldv = (ctx->cfg.vocab_size + 7) / 8 * 8;
  w.fe_t = take((size_t)B * Ta * CN_FEAT * es);
  w.mem = take((size_t)B * Ta * d * es);
  w.kvc = take((size_t)B * Ta * NL * 2 * d * es);
  w.x = (float*)take((size_t)R * d * 4);
  w.x2 = (float*)take((size_t)R * d * 4);
  w.xt = take((size_t)R * d * es);
  w.qkv = (float*)take((size_t)R * 3 * d * 4);
  w.q = (float*)take((size_t)R * d * 4);
  w.attn_t = take((size_t)R * d * es);
  w.tmp = (float*)take((size_t)R * d * 4);
  w.slabs = (float*)take((size_t)FF2_SPLITS * R * d * 4);
  w.ffh = take((size_t)R * ctx->cfg.d_ff * es);
  w.logits = (float*)take(lean ? 0 : (size_t)R * w.ldv * 4);
  w.kc = take(lean ? 0 : (size_t)NL * maxp * R * d * es);
  w.vc = take(lean ? 0 : (size_t)NL * maxp * R * d * es);
  w.n_active = (int*)take((size_t)B * 4);
  w.live = (int*)take((size_t)(CN_MAX_PRED + 2) * 4);
  w.slot = (int*)take((size_t)R * 4);
  w.sum_lp = (float*)take((size_t)R * 4);
  w.prefix = (int*)take((size_t)R * (maxp + 1) * 4);
  w.anc = (int*)take((size_t)R * maxp * 4);
  w.cur_tok = (int*)take((size_t)R * 4);
  w.out_len = (int*)take((size_t)R * 4);
  w.eos_idx = (int*)take((size_t)B * 4);
  w.kvalid = (unsigned long long*)take((size_t)R * 8);
  w.total = off;
  return w;
}

extern "C" size_t conette_decode_workspace_bytes(const conette_ctx* ctx, int32_t batch, int32_t t_audio, int32_t beam,
                                                 int32_t max_pred) {
  return dec_ws(ctx, batch, t_audio, beam, max_pred, nullptr).total;
}

// Arguments of the step path (decode_impl): conette_decode, conette_forcing (stepwise) and conette_greedy fill them by name.
// Zeroed with memset, the record is also the key of conette_decode's graph cache, compared bytewise: the buffers and the shape
// identify a captured launch sequence.  The stream is no part of it, and the three pointers at the end are null on that path.
struct DecArgs {
  const float* frame_embs;
  const int32_t* frame_lens;
  const int32_t* bos_ids;
  const uint8_t* forbid;  // may be null
  int32_t* best_preds;
  float* best_lprobs;
  int32_t* mult_preds;
  float* mult_lprobs;
  int32_t* out_sizes;
  float* step0_logits;  // these four outputs are optional (null: not wanted)
  int32_t* trace_sel;
  float* trace_val;
  float* margins;
  char* ws;
  int B, Ta, beam, min_pred, maxp;
  const int32_t* force_caps;  // teacher forcing: beam == 1, maxp == caption length, no search
  float* force_logits;
  float* greedy_logits;  // conette_greedy: the masked logits of every step
  const float* uniforms;  // conette_sample: beam == samples per clip, mult_preds / mult_lprobs == preds / sum_lprobs (dec_sample.h)
  int32_t* sample_lens;
  float* sample_tok_lp;       // these two are optional
  float* sample_step_logits;
  float temperature, top_p;
  int top_k;
  int n_groups, group_beam;  // conette_decode_groups: beam == n_groups * group_beam rows per clip, searched in groups (dec_group.h)
  float diversity;
  float* group_step_logits;  // optional
  int constrained;           // conette_decode_constrained: the steered search at beam `beam` (dec_constrain.h)
  int prefix_width, no_repeat_ngram;
  const int32_t* prefix;       // these four are optional
  const int32_t* prefix_lens;
  const uint8_t* ban;
  float* constrain_step_logits;
  int req_width;               // conette_decode_required: the constrained search with per-clip requirements (dec_require.h); 0: none
  const int32_t* req_tokens;
  const int32_t* req_groups;
  // conette_decode_ensemble (dec_ensemble.h): every member, member 0 included (whose context runs the graph cache).  INVARIANT: a
  // key with n_members > 0 names other contexts' weights, which a cached graph's launches read.  A pointer alone does not identify
  // a context -- a later conette_create may be handed the address of a destroyed one -- so the key also holds every member's
  // process-unique serial number (conette_ctx::serial, never reused): a recycled address gives another key, and the stale graph,
  // whose launches would read freed weights, is never replayed (it ages out of the cache like any other entry).
  int n_members, combine;
  conette_ctx* ens_ctx[CN_MAX_MEMBERS];
  unsigned long long ens_serial[CN_MAX_MEMBERS];
  const float* ens_fe[CN_MAX_MEMBERS];
  const int32_t* ens_bos[CN_MAX_MEMBERS];
  char* ens_ws[CN_MAX_MEMBERS];
  float ens_w[CN_MAX_MEMBERS];
  // a member's launch sequence depends on its CONETTE_OPT_DECODE_FUSION, and only the context whose option changes flushes its
  // own cache: the flag of every member is part of the key, so a graph with the other sequence is never replayed
  int ens_unfused[CN_MAX_MEMBERS];
  float* ens_step_logits;  // optional
  // conette_decode_spans (dec_spans.h): B == n_spans clips of Ta == t_span frames, gathered on the device from n_rec recordings of
  // t_rec frames by the table `spans`; frame_lens is null (the gather writes the lengths).  All zero on every other path.
  const int32_t* spans;
  int n_rec, t_rec, n_spans;
  bool operator==(const DecArgs& o) const { return memcmp(this, &o, sizeof(DecArgs)) == 0; }
};

// ---- once per batch: projection (conette.py:457) and cross K/V of every layer ---------------
template <typename T>
static int dec_prepare(conette_ctx* ctx, const float* frame_embs, int B, int Ta, const DecWs& w, hipStream_t s) {
  CnProfScope ps(ctx, CONETTE_PROF_DEC_PREPARE, s);
  const int d = ctx->cfg.d_model, kv_ld = ctx->cfg.n_layers * 2 * d;
  T* fe_t = (T*)w.fe_t;
  T* mem = (T*)w.mem;
  const size_t n = (size_t)B * Ta * CN_FEAT;
  hipLaunchKernelGGL((cn_cvt_kernel<T>), dim3((unsigned)((n + 1023) / 1024 < 4096 ? (n + 1023) / 1024 : 4096)), dim3(256), 0, s,
                     frame_embs, fe_t, n);
  CN_LAUNCH_CHECK();
  EpiBiasAct<T, ACT_RELU> ep{ctx->proj_b, mem, d, ACT_RELU};
  CN_TRY(cn_mm(fe_t, CN_FEAT, (const T*)ctx->proj_w, CN_FEAT, B * Ta, d, CN_FEAT, ep, s));
  EpiBiasAct<T, ACT_NONE> ekv{ctx->kv_b, (T*)w.kvc, kv_ld, ACT_NONE};
  CN_TRY(cn_mm(mem, d, (const T*)ctx->kv_w, d, B * Ta, kv_ld, d, ekv, s));
  return CN_OK;
}

// ---- conette_decode_spans: dec_prepare once over the recordings, then the spans' K/V rows gathered into w.kvc ----------------
// Behind the search's workspace (w.total): the recordings' converted frames, projected memory and cross K/V, and the spans' lengths.
struct SpanWs {
  void *fe_t, *mem, *kvc;
  int32_t* lens;
  size_t total;
};
static SpanWs span_ws(const conette_ctx* ctx, int n_rec, int t_rec, int n_spans, char* base) {
  const size_t es = ctx->esize, rows = (size_t)n_rec * t_rec;
  const int d = ctx->cfg.d_model;
  SpanWs w;
  size_t off = 0;
  auto take = [&](size_t bytes) {
    char* p = base ? base + off : nullptr;
    off += cn_align(bytes);
    return p;
  };
  w.fe_t = take(rows * CN_FEAT * es);
  w.mem = take(rows * d * es);
  w.kvc = take(rows * ctx->cfg.n_layers * 2 * d * es);
  w.lens = (int32_t*)take((size_t)n_spans * 4);
  w.total = off;
  return w;
}
template <typename T>
static int dec_prepare_spans(conette_ctx* ctx, const DecArgs& a, const DecWs& w, const SpanWs& sw, hipStream_t s) {
  DecWs rec = w;  // (dec_prepare reads these three members only)
  rec.fe_t = sw.fe_t, rec.mem = sw.mem, rec.kvc = sw.kvc;
  CN_TRY(dec_prepare<T>(ctx, a.frame_embs, a.n_rec, a.t_rec, rec, s));
  CnProfScope ps(ctx, CONETTE_PROF_DEC_PREPARE, s);
  const int row_vecs = (int)((size_t)ctx->cfg.n_layers * 2 * ctx->cfg.d_model * ctx->esize / 16);
  hipLaunchKernelGGL(cn_span_gather_kernel, dim3((unsigned)a.Ta, (unsigned)a.n_spans), dim3(256), 0, s, (const uint4*)sw.kvc, a.spans,
                     a.n_rec, a.t_rec, a.Ta, row_vecs, (uint4*)w.kvc, sw.lens);
  CN_LAUNCH_CHECK();
  return CN_OK;
}

// ---- decoder layer l, one launch per sub-layer, on the R rows of w.x / w.xt ------------------------------------------------
// QKV GEMM, self-attention, out-proj + residual, LN1, cross-Q GEMM, cross-attention, out-proj + residual, LN2, FFN1, FFN2, LN3.
// The step path without the block kernel and the one-pass teacher forcing both run it; what they differ in:
//   self_attn(l)   launches the layer's self-attention from w.qkv into w.attn_t: the KV-cached step kernel, or the causal one
//   rows_per_clip  consecutive rows that attend to one clip's audio memory (the "beam" of the cross-attention kernel)
//   ffn2_split     FFN2 as split-K slabs summed by LN3 (16-bit and exact operands only: fp32 has no such GEMM) instead of one
//                  GEMM with bias + residual in its epilogue.  The two sum in different orders, so a caller never changes its choice.
//   cross_attn(l)  optional: launches the layer's cross-attention from w.q into w.attn_t in place of cn_cross_attn_kernel
//                  (conette_align: the kernel that also keeps the weights, dec_align.h)
struct CnCrossDefault {};
template <typename T, typename SelfAttn, typename CrossAttn = CnCrossDefault>
static int dec_sublayer_layer(conette_ctx* ctx, const DecWs& w, int l, const int32_t* frame_lens, int R, int Ta, int rows_per_clip,
                              bool ffn2_split, SelfAttn self_attn, hipStream_t s, CrossAttn cross_attn = CrossAttn()) {
  const CnLayerW& lw = ctx->layers[l];
  const int d = ctx->cfg.d_model, dff = ctx->cfg.d_ff, kv_ld = ctx->cfg.n_layers * 2 * d;
  const float scale = 1.0f / sqrtf((float)(d / ctx->cfg.nhead));
  const int rblocks = cn_cdiv(R, 4);
  T* xt = (T*)w.xt;
  T* attn_t = (T*)w.attn_t;
  T* ffh = (T*)w.ffh;
  auto ln_tmp = [&](const float* g, const float* b) -> int {  // LayerNorm of w.tmp, a GEMM output that holds bias + residual already
    CnProfScope ps(ctx, CONETTE_PROF_DEC_MISC, s);
    hipLaunchKernelGGL((cn_ln256_kernel<T>), dim3(rblocks), dim3(256), 0, s, w.tmp, 1, (size_t)0, (const float*)nullptr,
                       (const float*)nullptr, g, b, R, w.x, xt);
    CN_LAUNCH_CHECK();
    return CN_OK;
  };
  {
    CnProfScope ps(ctx, CONETTE_PROF_DEC_GEMM, s);
    EpiBiasAct<float, ACT_NONE> eq{lw.sa_in_b, w.qkv, 3 * d, ACT_NONE};
    CN_TRY(cn_mm(xt, d, (const T*)lw.sa_in_w, d, R, 3 * d, d, eq, s));
  }
  {
    CnProfScope ps(ctx, CONETTE_PROF_DEC_ATTN, s);
    self_attn(l);
    CN_LAUNCH_CHECK();
  }
  {
    CnProfScope ps(ctx, CONETTE_PROF_DEC_GEMM, s);
    EpiResid eo{lw.sa_out_b, nullptr, w.x, w.tmp, d};
    CN_TRY(cn_mm(attn_t, d, (const T*)lw.sa_out_w, d, R, d, d, eo, s));
  }
  CN_TRY(ln_tmp(lw.n1w, lw.n1b));
  {
    CnProfScope ps(ctx, CONETTE_PROF_DEC_GEMM, s);
    EpiBiasAct<float, ACT_NONE> ecq{lw.ca_q_b, w.q, d, ACT_NONE};
    CN_TRY(cn_mm(xt, d, (const T*)lw.ca_q_w, d, R, d, d, ecq, s));
  }
  {
    CnProfScope ps(ctx, CONETTE_PROF_DEC_ATTN, s);
    if constexpr (std::is_same<CrossAttn, CnCrossDefault>::value)
      hipLaunchKernelGGL((cn_cross_attn_kernel<T>), dim3(rblocks), dim3(256), 0, s, w.q, (T*)w.kvc, kv_ld, l * 2 * d, frame_lens, R,
                         rows_per_clip, Ta, scale, attn_t);
    else
      cross_attn(l);
    CN_LAUNCH_CHECK();
  }
  {
    CnProfScope ps(ctx, CONETTE_PROF_DEC_GEMM, s);
    EpiResid eco{lw.ca_out_b, nullptr, w.x, w.tmp, d};
    CN_TRY(cn_mm(attn_t, d, (const T*)lw.ca_out_w, d, R, d, d, eco, s));
  }
  CN_TRY(ln_tmp(lw.n2w, lw.n2b));
  {
    CnProfScope ps(ctx, CONETTE_PROF_DEC_GEMM, s);
    EpiBiasAct<T, CnGeluAct<T>::value> e1{lw.ff1_b, ffh, dff, CnGeluAct<T>::value};
    CN_TRY(cn_mm(xt, d, (const T*)lw.ff1_w, d, R, dff, d, e1, s));
  }
  int nslab = 0;  // slabs FFN2 wrote for LN3 to sum; 0: FFN2 finished its sum in w.tmp
  if (ffn2_split) {
    CnProfScope ps(ctx, CONETTE_PROF_DEC_GEMM, s);
    EpiSlab e2{w.slabs, d, (size_t)R * d};
    if constexpr (CnIsH16<T>::value) {
      // K = d_ff is long and M = R is small: split K over blockIdx.y into partial slabs, summed
      // (fixed order, with bias + residual) by the LayerNorm kernel that follows
      const int splits = (dff % (FF2_SPLITS * 64) == 0) ? FF2_SPLITS : 1;
      CN_TRY(cn_gemm2(ffh, dff, (const T*)lw.ff2_w, dff, R, d, dff, e2, s, splits));
      nslab = splits;
    } else if constexpr (std::is_same<T, sp16_t>::value) {
      // exact precision: the same split-K as bf16 (M = R rows, K = d_ff: 12 blocks looping over 64 k-tiles took 30 us,
      // a quarter of the whole decode) -- partial slabs, summed in a fixed order with bias + residual by the LayerNorm
      const int splits = (dff % (FF2_SPLITS * 32) == 0) ? FF2_SPLITS : 1;
      CN_TRY(cn_gemm2_sp((const sp16_t*)ffh, dff, (const sp16_t*)lw.ff2_w, dff, R, d, dff, e2, s, splits));
      nslab = splits;
    }
  }
  if (nslab == 0) {
    {
      CnProfScope ps(ctx, CONETTE_PROF_DEC_GEMM, s);
      EpiResid e2{lw.ff2_b, nullptr, w.x, w.tmp, d};
      CN_TRY(cn_mm(ffh, dff, (const T*)lw.ff2_w, dff, R, d, dff, e2, s));
    }
    return ln_tmp(lw.n3w, lw.n3b);
  }
  CnProfScope ps(ctx, CONETTE_PROF_DEC_MISC, s);
  hipLaunchKernelGGL((cn_ln256_kernel<T>), dim3(rblocks), dim3(256), 0, s, w.slabs, nslab, (size_t)R * d, lw.ff2_b, w.x, lw.n3w,
                     lw.n3b, R, w.x, xt);
  CN_LAUNCH_CHECK();
  return CN_OK;
}

// ---- one decode step's forward, embedding through classifier: the R rows' tokens `tok` at position `step` -> w.logits ----------
// The activations, the KV cache and the cross K/V are those of `w`; the search state the kernels read is passed beside it -- `tok`
// (R) the rows' current tokens, `anc` (R, maxp) their ancestor table, `gate` (null: none) the count of rows still searching --
// so that the members of an ensemble run on the state of member 0 (decode_ensemble_impl) while every other caller passes its own.
template <typename T>
static int dec_step_forward(conette_ctx* ctx, const DecWs& w, const int* tok, int* anc, const int* gate, const unsigned long long* kvalid,
                            const int32_t* frame_lens, int B, int Ta, int beam, int maxp, int step, int db_debug, hipStream_t s) {
  const conette_config& cfg = ctx->cfg;
  const int d = cfg.d_model, NL = cfg.n_layers, R = B * beam, V = cfg.vocab_size, dff = cfg.d_ff;
  T* kvc = (T*)w.kvc;
  T* xt = (T*)w.xt;
  T* ffh = (T*)w.ffh;
  const int kv_ld = NL * 2 * d;
  const float scale = 1.0f / sqrtf((float)(d / cfg.nhead));
  const int rblocks = cn_cdiv(R, 4);
  // fused path (dec_block.h + dec_ffn.h): 16-bit operands, and since round 4 the exact precision (hi / lo passes of the same
  // two kernels; needs both packed streams, i.e. d_ff % 256 == 0 and d_ff <= 2048)
  constexpr bool kBlockT = CnIsH16<T>::value || std::is_same<T, sp16_t>::value;
  const bool block_path = kBlockT && !ctx->dec_unfused && ctx->layers[0].blk_w != nullptr &&
                          (CnIsH16<T>::value || (ctx->layers[0].ffn_w != nullptr && dff / 256 <= FF2_SPLITS));
  if (!block_path) {  // (the block path embeds in the prologue of layer 0's block kernel)
    hipLaunchKernelGGL((cn_embed_kernel<T>), dim3(rblocks), dim3(256), 0, s, tok, ctx->emb, ctx->pe, step, 0, R,
                       sqrtf((float)d), w.x, xt);
    CN_LAUNCH_CHECK();
  }
  bool fused_done = false;
  if constexpr (kBlockT) if (block_path) {
    // default path: 3 launches per layer -- fused block (embedding | previous LN3, QKV, self-attention,
    // cross-attention: dec_block.h), FFN1 GEMM + GELU, FFN2 split-K slabs (summed by the next layer's block
    // prologue; the last layer's by the LN3 kernel in front of the classifier)
    fused_done = true;
    int splits = ff2_splits_default();
    if (splits < 1 || splits > FF2_SPLITS || splits > 8 || dff % (splits * 64) != 0) splits = 1;
    // fused FFN (dec_ffn.h): one launch per layer, one slab per 256-wide hidden chunk
    const bool ffn_fused = ctx->layers[0].ffn_w != nullptr && dff / 256 <= FF2_SPLITS;
    if (ffn_fused) splits = dff / 256;
    const size_t slab = (size_t)R * d;
    for (int l = 0; l < NL; ++l) {
      const CnLayerW& lw = ctx->layers[l];
      T* kc = (T*)w.kc + (size_t)l * maxp * R * d;
      T* vc = (T*)w.vc + (size_t)l * maxp * R * d;
      {
        CnProfScope ps(ctx, CONETTE_PROF_DEC_ATTN, s);
        DbPrologue pro;
        pro.tok = tok, pro.emb = ctx->emb, pro.pe_row = ctx->pe + (size_t)step * d, pro.emb_scale = sqrtf((float)d);
        pro.slabs = nullptr, pro.nslab = 0, pro.slab_stride = slab, pro.b2_prev = nullptr, pro.g3 = nullptr, pro.b3 = nullptr;
        if (l > 0) {
          const CnLayerW& pw = ctx->layers[l - 1];
          pro.slabs = w.slabs, pro.nslab = splits, pro.b2_prev = pw.ff2_b, pro.g3 = pw.n3w, pro.b3 = pw.n3b;
        }
        DbWeights wt;
        wt.stream = lw.blk_w;
        wt.params = lw.blk_p;
        // rows per block: DbOp<T>::ROWS (4: many small blocks spread a short search over the chip); a wide search -- R >= DB_WIDE_R
        // rows, the grouped search of four 64-clip batches -- runs 8 rows per block (two per row wave): half the blocks, half the
        // weight re-streaming from L2, +1.1 % end to end beside the encoder (profiles/r05_notes.md section 8).  Row-local arithmetic:
        // the same bits either way.
        auto launch_block = [&](auto nr_tag) -> int {
          constexpr int NR = decltype(nr_tag)::value;
          CN_TRY((cn_dec_block_setup<T, NR>()));
          hipLaunchKernelGGL((cn_dec_block_kernel<T, NR>), dim3(cn_cdiv(R, NR)), dim3((DbL<T, NR>::THREADS)), (DbL<T, NR>::BYTES), s,
                             pro, wt, kc, vc, anc, step, R, beam, maxp, (const T*)kvc, kv_ld, l * 2 * d, frame_lens, Ta, w.x,
                             xt, scale, kvalid, db_debug, gate);
          CN_LAUNCH_CHECK();
          return CN_OK;
        };
        constexpr int kWide = CnIsH16<T>::value ? DB_WIDE_ROWS : DB_WIDE_ROWS_SP;
        if (kWide != DbOp<T>::ROWS && R >= DB_WIDE_R) CN_TRY(launch_block(std::integral_constant<int, kWide>{}));
        else CN_TRY(launch_block(std::integral_constant<int, DbOp<T>::ROWS>{}));
      }
      if (ffn_fused) {
        CnProfScope ps(ctx, CONETTE_PROF_DEC_GEMM, s);
        CN_TRY(cn_dec_ffn_setup<T>());
        hipLaunchKernelGGL(cn_dec_ffn_kernel<T>, dim3(dff / 256, cn_cdiv(R, DF_ROWS)), dim3(256), DF_LDS_BYTES_T(DbOp<T>::NPH), s, (const T*)xt, R,
                           lw.ffn_w, lw.ff1_b, w.slabs, slab, gate);
        CN_LAUNCH_CHECK();
      } else if constexpr (CnIsH16<T>::value) {
        {
          CnProfScope ps(ctx, CONETTE_PROF_DEC_GEMM, s);
          EpiBiasAct<T, ACT_GELU_FAST> e1{lw.ff1_b, ffh, dff, ACT_GELU_FAST};
          CN_TRY(cn_gemm2(xt, d, (const T*)lw.ff1_w, d, R, dff, d, e1, s));
        }
        {
          CnProfScope ps(ctx, CONETTE_PROF_DEC_GEMM, s);
          EpiSlab e2{w.slabs, d, slab};
          CN_TRY(cn_gemm2(ffh, dff, (const T*)lw.ff2_w, dff, R, d, dff, e2, s, splits));
        }
      }
    }
    {
      CnProfScope ps(ctx, CONETTE_PROF_DEC_MISC, s);
      const CnLayerW& lw = ctx->layers[NL - 1];
      hipLaunchKernelGGL((cn_ln256_kernel<T>), dim3(rblocks), dim3(256), 0, s, w.slabs, splits, slab, lw.ff2_b, w.x,
                         lw.n3w, lw.n3b, R, w.x, xt);
      CN_LAUNCH_CHECK();
    }
    {
      CnProfScope ps(ctx, CONETTE_PROF_DEC_GEMM, s);
      EpiBiasAct<float, ACT_NONE> ec{ctx->cls_b, w.logits, w.ldv, ACT_NONE};
      CN_TRY(cn_mm(xt, d, (const T*)ctx->cls_w, d, R, V, d, ec, s));
    }
  }
  if (!fused_done) {
    auto self_attn = [&](int l) {
      T* kc = (T*)w.kc + (size_t)l * maxp * R * d;
      T* vc = (T*)w.vc + (size_t)l * maxp * R * d;
      hipLaunchKernelGGL((cn_self_attn_kernel<T>), dim3(rblocks), dim3(256), 0, s, w.qkv, kc, vc, anc, step, R, beam, maxp,
                         scale, (T*)w.attn_t, kvalid);
    };
    for (int l = 0; l < NL; ++l) CN_TRY((dec_sublayer_layer<T>(ctx, w, l, frame_lens, R, Ta, beam, kBlockT, self_attn, s)));
    {
      CnProfScope ps(ctx, CONETTE_PROF_DEC_GEMM, s);
      EpiBiasAct<float, ACT_NONE> ec{ctx->cls_b, w.logits, w.ldv, ACT_NONE};
      CN_TRY(cn_mm(xt, d, (const T*)ctx->cls_w, d, R, V, d, ec, s));
    }
  }
  return CN_OK;
}

template <typename T>
static int decode_impl(conette_ctx* ctx, const DecArgs& a, hipStream_t s) {
  const conette_config& cfg = ctx->cfg;
  const int B = a.B, Ta = a.Ta, beam = a.beam, min_pred = a.min_pred, maxp = a.maxp;
  const int R = B * beam, V = cfg.vocab_size;
  DecWs w = dec_ws(ctx, B, Ta, beam, maxp, a.ws);
  const bool forcing = a.force_caps != nullptr;
  const bool sampling = a.uniforms != nullptr;
  const unsigned long long* kvalid = forcing ? w.kvalid : nullptr;

  const int32_t* frame_lens = a.frame_lens;
  if (a.spans) {  // conette_decode_spans: the clips are spans of recordings; their lengths come from the gather
    const SpanWs sw = span_ws(ctx, a.n_rec, a.t_rec, a.n_spans, a.ws + w.total);
    CN_TRY(dec_prepare_spans<T>(ctx, a, w, sw, s));
    frame_lens = sw.lens;
  } else {
    CN_TRY(dec_prepare<T>(ctx, a.frame_embs, B, Ta, w, s));
  }
  hipLaunchKernelGGL(cn_init_state_kernel, dim3(64), dim3(256), 0, s, B, beam, maxp, a.bos_ids, w.n_active, w.slot,
                     w.sum_lp, w.prefix, w.anc, w.cur_tok, a.mult_preds, a.mult_lprobs, w.out_len, a.out_sizes, cfg.pad_id,
                     a.trace_sel, a.trace_val, w.live, a.margins);
  CN_LAUNCH_CHECK();
  if (forcing) {
    hipLaunchKernelGGL(cn_force_init_kernel, dim3(cn_cdiv(B, 64)), dim3(64), 0, s, a.force_caps, B, maxp, cfg.pad_id,
                       w.kvalid, w.anc);
    CN_LAUNCH_CHECK();
  }
  const bool grouped = a.n_groups > 0;
  int* group_k = (int*)(a.ws + w.total);  // (B, n_groups) live rows of every group: behind the plain search's workspace
  if (grouped) {
    hipLaunchKernelGGL(cn_group_init_kernel, dim3(cn_cdiv(B * a.n_groups, 256)), dim3(256), 0, s, B * a.n_groups, a.group_beam, group_k);
    CN_LAUNCH_CHECK();
  }
  if (sampling) {  // rows never change parents: every row is its own ancestor; w.slot holds the per-row finished flag
    hipLaunchKernelGGL(cn_sample_init_kernel, dim3(64), dim3(256), 0, s, R, beam, maxp, w.anc, w.slot, a.sample_lens,
                       a.sample_tok_lp);
    CN_LAUNCH_CHECK();
  }
#ifdef CN_G2_PROF  // profiling build: phase stamps of the block kernel and the search step (tools/dbprof.py)
  static const int db_debug = getenv("CN_DB_DEBUG") ? atoi(getenv("CN_DB_DEBUG")) : 0;
#else
  constexpr int db_debug = 0;
#endif
  SsArgs ss;  // the search step's arguments (dec_search.h): the same at every step
  ss.logits = w.logits, ss.forbid = a.forbid, ss.n_active = w.n_active, ss.slot = w.slot, ss.sum_lp = w.sum_lp;
  ss.prefix = w.prefix, ss.anc = w.anc, ss.cur_tok = w.cur_tok, ss.out_preds = a.mult_preds, ss.out_avg = a.mult_lprobs;
  ss.out_len = w.out_len, ss.trace_sel = a.trace_sel, ss.trace_val = a.trace_val, ss.live = w.live, ss.margins = a.margins;
  ss.ldv = w.ldv, ss.V = V, ss.beam = beam, ss.maxp = maxp, ss.min_pred = min_pred, ss.eos_id = cfg.eos_id, ss.dbg = db_debug;
  GsArgs gs;  // the diverse search's own arguments: its step kernels read the groups' live rows through ss.n_active
  gs.step_logits = a.group_step_logits, gs.G = a.n_groups, gs.W = a.group_beam, gs.lambda = a.diversity;
  if (grouped) ss.n_active = group_k;
  CsArgs cs;  // the constrained search's own arguments
  cs.prefix = a.prefix, cs.prefix_lens = a.prefix_lens, cs.ban = a.ban, cs.step_logits = a.constrain_step_logits;
  cs.P = a.prefix_width, cs.ngram = a.no_repeat_ngram;
  RqArgs rq;  // the keyword-guided search's own arguments
  rq.tokens = a.req_tokens, rq.groups = a.req_groups, rq.width = a.req_width;

  for (int step = 0; step < maxp; ++step) {
    if (forcing) {
      hipLaunchKernelGGL(cn_force_tok_kernel, dim3(cn_cdiv(B, 64)), dim3(64), 0, s, a.force_caps, B, maxp, step, w.cur_tok);
      CN_LAUNCH_CHECK();
    }
    // device-side early exit: once every hypothesis of every clip has finished the reference leaves its loop
    // (beam.py:192-194); the launch sequence is static (hipGraph), so the heavy kernels of the remaining steps read the
    // number of rows still searching and return at once
    const int* gate = (!forcing && step > 0) ? w.live + step : nullptr;
    CN_TRY(dec_step_forward<T>(ctx, w, w.cur_tok, w.anc, gate, kvalid, frame_lens, B, Ta, beam, maxp, step, db_debug, s));
    if (step == 0 && a.step0_logits)
      CN_HIP(hipMemcpyAsync(a.step0_logits, w.logits, (size_t)R * w.ldv * 4, hipMemcpyDeviceToDevice, s));
    if (forcing) {
      hipLaunchKernelGGL(cn_force_store_kernel, dim3(cn_cdiv(V, 1024), R), dim3(256), 0, s, w.logits, w.ldv, V, maxp, step,
                         a.force_logits);
      CN_LAUNCH_CHECK();
      continue;
    }
    if (a.greedy_logits) {  // beam == 1: rows == clips; before the search step updates prefix / n_active
      hipLaunchKernelGGL(cn_greedy_logits_kernel, dim3(cn_cdiv(V, 1024), B), dim3(256), 0, s, ss, step, cfg.pad_id, a.greedy_logits);
      CN_LAUNCH_CHECK();
    }
    CnProfScope ps_search(ctx, CONETTE_PROF_SEARCH, s);
    if (sampling) {  // the per-row sampling step instead of the search step (dec_sample.h)
      SmArgs sa;
      sa.logits = w.logits, sa.forbid = a.forbid, sa.uniforms = a.uniforms, sa.prefix = w.prefix, sa.cur_tok = w.cur_tok;
      sa.sum_lp = w.sum_lp, sa.fin = w.slot, sa.live = w.live, sa.preds = a.mult_preds, sa.sum_out = a.mult_lprobs;
      sa.lens = a.sample_lens, sa.sizes = a.out_sizes, sa.tok_lp = a.sample_tok_lp, sa.step_logits = a.sample_step_logits;
      sa.ldv = w.ldv, sa.V = V, sa.R = R, sa.maxp = maxp, sa.min_pred = min_pred, sa.eos_id = cfg.eos_id, sa.top_k = a.top_k;
      sa.temperature = a.temperature, sa.top_p = a.top_p;
      const int vpt = cn_cdiv(V, SM_T);
#define SM_LAUNCH(VPT_) hipLaunchKernelGGL((cn_sample_step_kernel<VPT_>), dim3(R), dim3(SM_T), 0, s, sa, step)
      if (vpt <= 2) SM_LAUNCH(2);
      else if (vpt <= 4) SM_LAUNCH(4);
      else if (vpt <= 6) SM_LAUNCH(6);
      else if (vpt <= SM_VPT) SM_LAUNCH(8);
      else SM_LAUNCH(0);  // vocabularies beyond 8192 entries: the logits are re-read from global memory
#undef SM_LAUNCH
      CN_LAUNCH_CHECK();
      continue;
    }
    if (grouped) {  // the groups of a clip in sequence, one launch per step (dec_group.h)
      cn_group_step_launch(ss, gs, B, step, s);
      CN_LAUNCH_CHECK();
      continue;
    }
    if (a.constrained) {  // the steered step, one launch per step (dec_constrain.h)
      if (a.req_width > 0) cn_require_step_launch(ss, cs, rq, B, step, s);  // (no table: no requirement, the constrained step)
      else cn_constrain_step_launch(ss, cs, B, step, s);
      CN_LAUNCH_CHECK();
      continue;
    }
    if (V <= S3_T * S3_VPT && beam <= 8) {  // register-resident step (one block of 1024 threads per clip)
#define S3_LAUNCH(NR_, VPT_) hipLaunchKernelGGL((cn_search_step3_kernel<NR_, VPT_>), dim3(B), dim3(S3_T), 0, s, ss, step)
      const int vpt = cn_cdiv(V, S3_T);
      if (beam <= 4) {
        if (vpt <= 2) S3_LAUNCH(4, 2);
        else if (vpt <= 4) S3_LAUNCH(4, 4);
        else if (vpt <= 6) S3_LAUNCH(4, 6);
        else S3_LAUNCH(4, 8);
      } else {
        if (vpt <= 4) S3_LAUNCH(8, 4);
        else S3_LAUNCH(8, 8);
      }
#undef S3_LAUNCH
    } else {  // vocabularies beyond 8192 entries, beams beyond 8: the generic step (masking in place, top-k over global memory)
      hipLaunchKernelGGL(cn_search_step_kernel, dim3(B), dim3(256), 0, s, ss, step);
    }
    CN_LAUNCH_CHECK();
  }
  if (forcing || sampling) return CN_OK;
  hipLaunchKernelGGL(cn_finalize_kernel, dim3(cn_cdiv(B, 64)), dim3(64), 0, s, B, beam, maxp, cfg.eos_id, a.mult_preds,
                     a.mult_lprobs, w.out_len, a.best_preds, a.best_lprobs, w.eos_idx, a.out_sizes, a.margins);
  CN_LAUNCH_CHECK();
  hipLaunchKernelGGL(cn_finalize2_kernel, dim3(1), dim3(256), 0, s, B, w.eos_idx, a.out_sizes);
  CN_LAUNCH_CHECK();
  return CN_OK;
}

// ---- hipGraph replay of the (static) decode launch sequence ---------------------------------------
struct DecGraph {
  DecArgs key;
  hipGraphExec_t exec;
  hipGraph_t graph;
  hipEvent_t last;  // recorded behind every launch of `exec`: what an eviction waits for (never the whole device)
  int seen;         // 1: seen once (ran eagerly); 2: being captured by some thread (others run eagerly meanwhile)
  int nodes;        // kernel nodes of `graph`
};
static void dec_graph_release(DecGraph& g) {
  if (!g.exec) return;
  // the graph may still be executing on another stream: wait for ITS last launch.  (Not hipDeviceSynchronize: that is illegal
  // while any stream of the process is being captured -- e.g. another thread's first capture -- and would invalidate it.)
  if (g.last) {
    if (hipEventSynchronize(g.last) != hipSuccess) (void)hipGetLastError();
    (void)hipEventDestroy(g.last);
  }
  (void)hipGraphExecDestroy(g.exec);
  (void)hipGraphDestroy(g.graph);
  g.exec = nullptr, g.graph = nullptr, g.last = nullptr;
}
#define CN_MAX_DEC_GRAPHS 64  // (bucket, pipeline slot) keys: conette_amd.engine sizes its buffer cache from the same number
// The cache is shared by every host thread that decodes on this context (the pipelines run two or three decode streams,
// usually from one thread, but nothing in the ABI says so).  Its lock is PER CONTEXT and covers only the table itself --
// lookup, LRU order, insertion, the hand-over of an evicted entry: the ~300 eager launches of a first sighting, stream
// capture + instantiation and the blocking wait for an evicted graph's last launch all run outside it, so threads that
// drive other contexts (other GPUs) never meet, and an eviction stalls nobody but the caller that caused it.
struct DecGraphCache {
  std::mutex mu;
  DecGraph g[CN_MAX_DEC_GRAPHS] = {};
  int n = 0;
  int enabled = 1;
  int last_nodes = 0;  // nodes of the graph most recently launched or captured (conette_decode_graph_nodes)
};
static std::mutex g_dec_cache_create_mu;   // only the creation / destruction of a context's cache object
static DecGraphCache* graph_cache(conette_ctx* ctx, bool create) {
  std::lock_guard<std::mutex> lock(g_dec_cache_create_mu);
  if (ctx->dec_graphs == nullptr && create) ctx->dec_graphs = new DecGraphCache();
  return (DecGraphCache*)ctx->dec_graphs;
}
void cn_decode_graphs_free(conette_ctx* ctx) {
  DecGraphCache* c = graph_cache(ctx, false);
  if (!c) return;
  {
    std::lock_guard<std::mutex> lock(c->mu);
    for (int i = 0; i < c->n; ++i) dec_graph_release(c->g[i]);
    c->n = 0;
  }
  std::lock_guard<std::mutex> lock(g_dec_cache_create_mu);
  delete c;
  ctx->dec_graphs = nullptr;
}
extern "C" int conette_set_option(conette_ctx* ctx, int32_t option, int32_t value) {
  if (!ctx) return CN_ERR_ARG;
  if (option == CONETTE_OPT_DECODE_GRAPH) {
    DecGraphCache* c = graph_cache(ctx, true);
    if (c) {
      std::lock_guard<std::mutex> lock(c->mu);
      c->enabled = value ? 1 : 0;
    }
    return CN_OK;
  }
  if (option == CONETTE_OPT_DECODE_FUSION) {
    ctx->dec_unfused = value ? 0 : 1;
    DecGraphCache* c = graph_cache(ctx, false);
    if (c) {  // cached graphs hold the other launch sequence
      std::lock_guard<std::mutex> lock(c->mu);
      for (int i = 0; i < c->n; ++i) dec_graph_release(c->g[i]);
      c->n = 0;
    }
    return CN_OK;
  }
  if (option == CONETTE_OPT_FORCING_STEPWISE) {
    ctx->forcing_stepwise = value ? 1 : 0;
    return CN_OK;
  }
  if (option == CONETTE_OPT_SCORE_VSPLIT) {
    if (value < 0) {
      cn_set_error("set_option: score vocabulary split %d < 0", value);
      return CN_ERR_ARG;
    }
    ctx->score_vsplit = value;
    return CN_OK;
  }
  if (option == CONETTE_OPT_ENCODE_RESERVED_CUS) {
    if (value < 0 || value > ctx->n_cu / 2) {
      cn_set_error("set_option: reserved CUs %d outside 0 .. %d", value, ctx->n_cu / 2);
      return CN_ERR_ARG;
    }
    ctx->enc_reserved_cus = value;
    return CN_OK;
  }
  cn_set_error("set_option: unknown option %d", option);
  return CN_ERR_ARG;
}

// The shared refusals of the decoder entry points, `who` being the prefix of their messages.  dec_check_model: the length (caption
// length or max_pred, with the entry point's own message: `len_fmt` and its arguments) and the architecture the kernels are
// specialised for; dec_check_workspace: the workspace.  conette_score has a check of its own between the two.
template <typename... A>
static int dec_check_model(const conette_ctx* ctx, const char* who, int len, int min_pred, const char* len_fmt, A... len_args) {
  if (len < 1 || len > CN_MAX_PRED || len > ctx->pe_len || min_pred < 0) {
    cn_set_error(len_fmt, len_args...);
    return CN_ERR_ARG;
  }
  if (ctx->cfg.d_model != 256 || ctx->cfg.nhead != 8) {
    cn_set_error("%s: kernels are specialised for d_model=256, nhead=8", who);
    return CN_ERR_ARG;
  }
  return CN_OK;
}
static int dec_check_workspace(const char* who, size_t workspace_bytes, size_t need) {
  if (workspace_bytes < need) {
    cn_set_error("%s: workspace %zu < %zu", who, workspace_bytes, need);
    return CN_ERR_WORKSPACE;
  }
  return CN_OK;
}

// conette_decode and conette_decode_ensemble share their checks.  dec_check_search: the arguments every member of a search shares;
// dec_check_member: what a context and its workspace must satisfy (one call per member).
static int dec_check_search(const char* who, const int32_t* frame_lens, int batch, int t_audio, int beam, int min_pred, int max_pred,
                            const int32_t* best_preds, const float* best_lprobs, const int32_t* mult_preds, const float* mult_lprobs,
                            const int32_t* out_sizes) {
  if (!frame_lens || !best_preds || !best_lprobs || !mult_preds || !mult_lprobs || !out_sizes || batch <= 0 || t_audio <= 0) {
    cn_set_error("%s: bad argument", who);
    return CN_ERR_ARG;
  }
  if (beam < 1 || beam > CN_MAX_BEAM || max_pred < 1 || max_pred > CN_MAX_PRED || min_pred < 0) {
    cn_set_error("%s: beam=%d (1..%d) max_pred=%d (1..%d) min_pred=%d unsupported", who, beam, CN_MAX_BEAM, max_pred, CN_MAX_PRED,
                 min_pred);
    return CN_ERR_ARG;
  }
  return CN_OK;
}
static int dec_check_member(const char* who, const conette_ctx* ctx, int min_pred, int max_pred, size_t workspace_bytes, size_t need) {
  CN_TRY(dec_check_model(ctx, who, max_pred, min_pred, "%s: max_pred exceeds positional table", who));
  return dec_check_workspace(who, workspace_bytes, need);
}

// `run` (the launch sequence of the decode that `key` identifies) through the context's graph cache: eagerly at the first sighting
// of a key, captured at the second, replayed from then on.
template <typename Run>
static int dec_graph_run(conette_ctx* ctx, const DecArgs& key, hipStream_t s, Run run) {
  DecGraphCache* cache = graph_cache(ctx, true);
  const uint32_t dec_classes = (1u << CONETTE_PROF_DEC_PREPARE) | (1u << CONETTE_PROF_DEC_GEMM) |
                               (1u << CONETTE_PROF_DEC_ATTN) | (1u << CONETTE_PROF_DEC_MISC) |
                               (1u << CONETTE_PROF_SEARCH);
  if (!cache || (ctx->prof_mask & dec_classes) != 0) return run();

  auto find = [&]() -> DecGraph* {  // (under the lock) least recently used first: a hit moves to the back
    for (int i = 0; i < cache->n; ++i)
      if (cache->g[i].key == key) {
        const DecGraph hit = cache->g[i];
        memmove(&cache->g[i], &cache->g[i + 1], sizeof(DecGraph) * (cache->n - 1 - i));
        cache->g[cache->n - 1] = hit;
        return &cache->g[cache->n - 1];
      }
    return nullptr;
  };
  enum { EAGER, CAPTURE } todo = EAGER;
  DecGraph evicted;
  memset(&evicted, 0, sizeof(evicted));
  {
    std::lock_guard<std::mutex> lock(cache->mu);
    if (!cache->enabled) {
      todo = EAGER;
    } else if (DecGraph* e = find()) {
      if (e->exec) {  // replay (the launch and the event record stay under the lock: an eviction must see this launch's event)
        CN_HIP(hipGraphLaunch(e->exec, s));
        CN_HIP(hipEventRecord(e->last, s));
        cache->last_nodes = e->nodes;
        return CN_OK;
      }
      if (e->seen == 1) {  // second sighting: this call captures; the same key from another thread meanwhile runs eagerly
        e->seen = 2;
        todo = CAPTURE;
      }
    } else {  // first sighting: run eagerly (also performs the one-time kernel attribute setup)
      if (cache->n == CN_MAX_DEC_GRAPHS) {
        // Evict the least recently used entry.  Its graph may still be executing on another stream (two or three decode
        // streams replay graphs side by side), and destroying an executable graph under a running launch is undefined: its
        // own last launch is waited for (an event per graph) -- below, after the lock has been dropped.  This is the one
        // place an entry point blocks, and it is off the steady state (more than CN_MAX_DEC_GRAPHS distinct (shape, buffer)
        // keys alive at once); conette_set_option(DECODE_GRAPH, 0) avoids it.
        evicted = cache->g[0];
        memmove(&cache->g[0], &cache->g[1], sizeof(DecGraph) * (CN_MAX_DEC_GRAPHS - 1));
        cache->n--;
      }
      DecGraph* fresh = &cache->g[cache->n++];
      memset(fresh, 0, sizeof(*fresh));
      memcpy(&fresh->key, &key, sizeof(key));  // (every byte: the keys are compared bytewise)
      fresh->seen = 1;
    }
  }
  dec_graph_release(evicted);
  if (todo == EAGER) return run();

  // capture, instantiate, launch -- outside the lock; the entry is found again by its key when the graph exists
  hipGraph_t graph = nullptr;
  hipGraphExec_t exec = nullptr;
  hipEvent_t last = nullptr;
  auto capture = [&]() -> bool {
    if (hipStreamBeginCapture(s, hipStreamCaptureModeRelaxed) != hipSuccess) return false;
    const int rc = run();
    if (hipStreamEndCapture(s, &graph) != hipSuccess || rc != CN_OK || graph == nullptr) return false;
    if (hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0) != hipSuccess || exec == nullptr) return false;
    return hipEventCreateWithFlags(&last, hipEventDisableTiming) == hipSuccess;
  };
  if (!capture()) {  // capture is not available here: every later call runs eagerly, and so does this one
    (void)hipGetLastError();
    if (exec) (void)hipGraphExecDestroy(exec);
    if (graph) (void)hipGraphDestroy(graph);
    {
      std::lock_guard<std::mutex> lock(cache->mu);
      cache->enabled = 0;
    }
    return run();
  }
  size_t n_nodes = 0;
  if (hipGraphGetNodes(graph, nullptr, &n_nodes) != hipSuccess) (void)hipGetLastError();
  {
    std::lock_guard<std::mutex> lock(cache->mu);
    DecGraph* e = find();
    if (e && !e->exec) {
      e->exec = exec, e->graph = graph, e->last = last, e->nodes = (int)n_nodes;
      cache->last_nodes = e->nodes;
      CN_HIP(hipGraphLaunch(exec, s));
      CN_HIP(hipEventRecord(last, s));
      return CN_OK;
    }
  }
  // (the entry was evicted, or the cache reset, while this call captured: launch once and drop the graph)
  CN_HIP(hipGraphLaunch(exec, s));
  CN_HIP(hipEventRecord(last, s));
  DecGraph tmp;
  memset(&tmp, 0, sizeof(tmp));
  tmp.exec = exec, tmp.graph = graph, tmp.last = last;
  dec_graph_release(tmp);
  return CN_OK;
}

extern "C" int conette_decode(conette_ctx* ctx, const float* frame_embs, const int32_t* frame_lens,
                              const int32_t* bos_ids, const uint8_t* forbid_mask, int32_t batch, int32_t t_audio,
                              int32_t beam, int32_t min_pred, int32_t max_pred, int32_t* best_preds,
                              float* best_lprobs, int32_t* mult_preds, float* mult_lprobs, int32_t* out_sizes,
                              float* step0_logits, int32_t* trace_sel, float* trace_val, float* margins,
                              void* workspace, size_t workspace_bytes, void* stream) {
  if (!ctx || !frame_embs || !bos_ids || !workspace) {
    cn_set_error("decode: bad argument");
    return CN_ERR_ARG;
  }
  CN_TRY(dec_check_search("decode", frame_lens, batch, t_audio, beam, min_pred, max_pred, best_preds, best_lprobs, mult_preds, mult_lprobs,
                          out_sizes));
  CN_TRY(dec_check_member("decode", ctx, min_pred, max_pred, workspace_bytes, conette_decode_workspace_bytes(ctx, batch, t_audio, beam, max_pred)));
  DecArgs a;
  memset(&a, 0, sizeof(a));  // (padding included: the record is the graph key)
  a.frame_embs = frame_embs, a.frame_lens = frame_lens, a.bos_ids = bos_ids, a.forbid = forbid_mask;
  a.best_preds = best_preds, a.best_lprobs = best_lprobs, a.mult_preds = mult_preds, a.mult_lprobs = mult_lprobs;
  a.out_sizes = out_sizes, a.step0_logits = step0_logits, a.trace_sel = trace_sel, a.trace_val = trace_val;
  a.margins = margins, a.ws = (char*)workspace;
  a.B = batch, a.Ta = t_audio, a.beam = beam, a.min_pred = min_pred, a.maxp = max_pred;
  hipStream_t s = (hipStream_t)stream;
  auto run = [&]() -> int { CN_BY_PRECISION(ctx, decode_impl<OT>(ctx, a, s)); };
  // the caller captures: the launches go into the caller's graph and the context's cache is left alone (no entry, no sighting
  // counted, no replay, no event record -- a begin-capture on a capturing stream would switch the cache off for good, and a
  // replay's event would only be captured, never recorded, for a later eviction to wait on)
  hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
  CN_HIP(hipStreamIsCapturing(s, &cap));
  if (cap != hipStreamCaptureStatusNone) return run();
  return dec_graph_run(ctx, a, s, run);
}

// ---- ensemble beam search (dec_ensemble.h): M members decode one hypothesis tree in lockstep ----------------------------------
// Every member has its own workspace (dec_ws: activations, KV cache, cross K/V, logits); the search state lives in member 0's, and
// the other members' block / attention kernels read it from there.  Per step: every member's forward, one after another on the
// caller's stream, then ONE search step over the M logits arrays.  With one member the launch sequence is conette_decode's but for
// the step kernel.
__global__ void cn_ens_tok0_kernel(int R, int beam, const int* __restrict__ bos, int* __restrict__ tok) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < R) tok[i] = bos[i / beam];
}

template <typename T>
static int decode_ensemble_impl(const DecArgs& a, hipStream_t s) {
  const int M = a.n_members, B = a.B, Ta = a.Ta, beam = a.beam, maxp = a.maxp, R = B * beam;
  conette_ctx* c0 = a.ens_ctx[0];
  const conette_config& cfg = c0->cfg;
  DecWs w[CN_MAX_MEMBERS];
  for (int m = 0; m < M; ++m) {
    w[m] = dec_ws(a.ens_ctx[m], B, Ta, beam, maxp, a.ens_ws[m]);
    CN_TRY(dec_prepare<T>(a.ens_ctx[m], a.ens_fe[m], B, Ta, w[m], s));
  }
  hipLaunchKernelGGL(cn_init_state_kernel, dim3(64), dim3(256), 0, s, B, beam, maxp, a.ens_bos[0], w[0].n_active, w[0].slot,
                     w[0].sum_lp, w[0].prefix, w[0].anc, w[0].cur_tok, a.mult_preds, a.mult_lprobs, w[0].out_len, a.out_sizes, cfg.pad_id,
                     a.trace_sel, a.trace_val, w[0].live, a.margins);
  CN_LAUNCH_CHECK();
  for (int m = 1; m < M; ++m) {  // step 0: a member embeds its own task tokens (kept in its own workspace)
    hipLaunchKernelGGL(cn_ens_tok0_kernel, dim3(cn_cdiv(R, 256)), dim3(256), 0, s, R, beam, a.ens_bos[m], w[m].cur_tok);
    CN_LAUNCH_CHECK();
  }
  SsArgs ss;
  ss.logits = nullptr, ss.forbid = a.forbid, ss.n_active = w[0].n_active, ss.slot = w[0].slot, ss.sum_lp = w[0].sum_lp;
  ss.prefix = w[0].prefix, ss.anc = w[0].anc, ss.cur_tok = w[0].cur_tok, ss.out_preds = a.mult_preds, ss.out_avg = a.mult_lprobs;
  ss.out_len = w[0].out_len, ss.trace_sel = a.trace_sel, ss.trace_val = a.trace_val, ss.live = w[0].live, ss.margins = a.margins;
  ss.ldv = w[0].ldv, ss.V = cfg.vocab_size, ss.beam = beam, ss.maxp = maxp, ss.min_pred = a.min_pred, ss.eos_id = cfg.eos_id, ss.dbg = 0;
  EsArgs es;
  memset(&es, 0, sizeof(es));
  for (int m = 0; m < M; ++m) {
    es.logits[m] = w[m].logits, es.bos[m] = a.ens_bos[m], es.w[m] = a.ens_w[m];
    es.logw[m] = (float)log((double)a.ens_w[m]);
  }
  es.comb = (float*)(a.ens_ws[0] + w[0].total);  // behind the plain search's workspace
  es.M = M, es.rule = a.combine;
  const size_t lbytes = (size_t)R * w[0].ldv * 4;
  for (int step = 0; step < maxp; ++step) {
    const int* gate = step > 0 ? w[0].live + step : nullptr;
    for (int m = 0; m < M; ++m) {
      const int* tok = (step == 0 && m > 0) ? w[m].cur_tok : w[0].cur_tok;
      CN_TRY(dec_step_forward<T>(a.ens_ctx[m], w[m], tok, w[0].anc, gate, nullptr, a.frame_lens, B, Ta, beam, maxp, step, 0, s));
      if (a.ens_step_logits)
        CN_HIP(hipMemcpyAsync((char*)a.ens_step_logits + ((size_t)step * M + m) * lbytes, w[m].logits, lbytes, hipMemcpyDeviceToDevice, s));
    }
    CnProfScope ps_search(c0, CONETTE_PROF_SEARCH, s);
    cn_ens_step_launch(ss, es, B, step, s);
    CN_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(cn_finalize_kernel, dim3(cn_cdiv(B, 64)), dim3(64), 0, s, B, beam, maxp, cfg.eos_id, a.mult_preds,
                     a.mult_lprobs, w[0].out_len, a.best_preds, a.best_lprobs, w[0].eos_idx, a.out_sizes, a.margins);
  CN_LAUNCH_CHECK();
  hipLaunchKernelGGL(cn_finalize2_kernel, dim3(1), dim3(256), 0, s, B, w[0].eos_idx, a.out_sizes);
  CN_LAUNCH_CHECK();
  return CN_OK;
}

extern "C" size_t conette_decode_ensemble_workspace_bytes(const conette_ctx* ctx, int32_t batch, int32_t t_audio, int32_t beam,
                                                          int32_t max_pred) {
  if (!ctx || batch <= 0 || t_audio <= 0 || max_pred <= 0 || beam < 1 || beam > CN_MAX_BEAM) return 0;
  const DecWs w = dec_ws(ctx, batch, t_audio, beam, max_pred, nullptr);
  return w.total + cn_align((size_t)batch * beam * w.ldv * 4);  // (+ the combined scores of the generic step: used in member 0's)
}

extern "C" int conette_decode_ensemble(const conette_member* members, int32_t n_members, int32_t combine, const int32_t* frame_lens,
                                       const uint8_t* forbid_mask, int32_t batch, int32_t t_audio, int32_t beam, int32_t min_pred,
                                       int32_t max_pred, int32_t* best_preds, float* best_lprobs, int32_t* mult_preds,
                                       float* mult_lprobs, int32_t* out_sizes, int32_t* trace_sel, float* trace_val, float* margins,
                                       float* step_logits, void* stream) {
  const char* who = "decode_ensemble";
  if (!members || n_members < 1 || n_members > CN_MAX_MEMBERS) {
    cn_set_error("%s: n_members=%d unsupported (1..%d, members given)", who, n_members, CN_MAX_MEMBERS);
    return CN_ERR_ARG;
  }
  if (combine != CONETTE_COMBINE_LOGPROB && combine != CONETTE_COMBINE_PROB) {
    cn_set_error("%s: combine=%d unknown (0: logprob, 1: prob)", who, combine);
    return CN_ERR_ARG;
  }
  for (int m = 0; m < n_members; ++m) {
    const conette_member& mb = members[m];
    const char* missing = !mb.ctx ? "ctx" : (!mb.frame_embs ? "frame_embs" : (!mb.bos_ids ? "bos_ids" : (!mb.workspace ? "workspace" : nullptr)));
    if (missing) {
      cn_set_error("%s: members[%d].%s is NULL", who, m, missing);
      return CN_ERR_ARG;
    }
    if (!(mb.weight > 0.f) || !(mb.weight < INFINITY)) {
      cn_set_error("%s: members[%d].weight=%g must be finite and > 0", who, m, (double)mb.weight);
      return CN_ERR_ARG;
    }
  }
  CN_TRY(dec_check_search(who, frame_lens, batch, t_audio, beam, min_pred, max_pred, best_preds, best_lprobs, mult_preds, mult_lprobs,
                          out_sizes));
  const conette_config& c0 = members[0].ctx->cfg;
  for (int m = 0; m < n_members; ++m) {
    const conette_config& c = members[m].ctx->cfg;
    if (c.vocab_size != c0.vocab_size || c.eos_id != c0.eos_id || c.pad_id != c0.pad_id) {
      cn_set_error("%s: members[%d].ctx has vocab_size=%d eos_id=%d pad_id=%d, members[0].ctx %d / %d / %d (one vocabulary per ensemble)", who,
                   m, c.vocab_size, c.eos_id, c.pad_id, c0.vocab_size, c0.eos_id, c0.pad_id);
      return CN_ERR_ARG;
    }
    if (c.precision != c0.precision) {
      cn_set_error("%s: members[%d].ctx has precision %d, members[0].ctx %d (one precision per ensemble)", who, m, c.precision, c0.precision);
      return CN_ERR_ARG;
    }
    CN_TRY(dec_check_member(who, members[m].ctx, min_pred, max_pred, members[m].workspace_bytes,
                            conette_decode_ensemble_workspace_bytes(members[m].ctx, batch, t_audio, beam, max_pred)));
    // a member keeps its KV cache, activations and logits in its workspace: two members on one range would overwrite each other's
    const char* lo = (const char*)members[m].workspace;
    const char* hi = lo + conette_decode_ensemble_workspace_bytes(members[m].ctx, batch, t_audio, beam, max_pred);
    for (int o = 0; o < m; ++o) {
      const char* olo = (const char*)members[o].workspace;
      const char* ohi = olo + conette_decode_ensemble_workspace_bytes(members[o].ctx, batch, t_audio, beam, max_pred);
      if (lo < ohi && olo < hi) {
        cn_set_error("%s: members[%d].workspace overlaps members[%d].workspace (every member needs its own)", who, m, o);
        return CN_ERR_ARG;
      }
    }
  }
  DecArgs a;
  memset(&a, 0, sizeof(a));  // (padding included: the record is the graph key)
  a.frame_lens = frame_lens, a.forbid = forbid_mask;
  a.best_preds = best_preds, a.best_lprobs = best_lprobs, a.mult_preds = mult_preds, a.mult_lprobs = mult_lprobs;
  a.out_sizes = out_sizes, a.trace_sel = trace_sel, a.trace_val = trace_val, a.margins = margins;
  a.B = batch, a.Ta = t_audio, a.beam = beam, a.min_pred = min_pred, a.maxp = max_pred;
  a.n_members = n_members, a.combine = combine, a.ens_step_logits = step_logits;
  bool profiled = false;
  for (int m = 0; m < n_members; ++m) {
    a.ens_ctx[m] = members[m].ctx, a.ens_serial[m] = members[m].ctx->serial, a.ens_fe[m] = members[m].frame_embs;
    a.ens_bos[m] = members[m].bos_ids, a.ens_ws[m] = (char*)members[m].workspace, a.ens_w[m] = members[m].weight;
    a.ens_unfused[m] = members[m].ctx->dec_unfused;
    profiled |= members[m].ctx->prof_mask != 0;
  }
  hipStream_t s = (hipStream_t)stream;
  auto run = [&]() -> int { CN_BY_PRECISION(a.ens_ctx[0], decode_ensemble_impl<OT>(a, s)); };
  if (profiled) return run();  // (a profiled member's event pairs do not go into a captured graph)
  hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
  CN_HIP(hipStreamIsCapturing(s, &cap));
  if (cap != hipStreamCaptureStatusNone) return run();  // the caller captures: the launches go into the caller's graph
  return dec_graph_run(a.ens_ctx[0], a, s, run);
}

extern "C" int32_t conette_decode_graph_nodes(const conette_ctx* ctx) {
  DecGraphCache* c = ctx ? (DecGraphCache*)ctx->dec_graphs : nullptr;
  if (!c) return 0;
  std::lock_guard<std::mutex> lock(c->mu);
  return c->last_nodes;
}

// ---- beam search over spans of recordings encoded once (dec_spans.h) ----
// The limits of one call: the GEMM epilogues and the attention kernels index rows * kv_ld elements in 32 bits, and the gather's grid
// has one y-block per span.
static bool spans_shape_ok(const conette_ctx* ctx, long n_rec, long t_rec, long n_spans, long t_span) {
  const long kv_ld = (long)ctx->cfg.n_layers * 2 * ctx->cfg.d_model;
  const long wide = kv_ld > CN_FEAT ? kv_ld : CN_FEAT;
  return n_rec * t_rec <= 0x7fffffffL / wide && n_spans * t_span <= 0x7fffffffL / wide && n_spans <= 65535;
}
extern "C" size_t conette_decode_spans_workspace_bytes(const conette_ctx* ctx, int32_t n_rec, int32_t t_rec, int32_t n_spans,
                                                       int32_t t_span, int32_t beam, int32_t max_pred) {
  if (!ctx || n_rec <= 0 || t_rec <= 0 || n_spans <= 0 || t_span <= 0 || max_pred <= 0 || beam < 1 || beam > CN_MAX_BEAM) return 0;
  if (!spans_shape_ok(ctx, n_rec, t_rec, n_spans, t_span)) return 0;
  return dec_ws(ctx, n_spans, t_span, beam, max_pred, nullptr).total + span_ws(ctx, n_rec, t_rec, n_spans, nullptr).total;
}

extern "C" int conette_decode_spans(conette_ctx* ctx, const float* frame_embs, const int32_t* spans, const int32_t* bos_ids,
                                    const uint8_t* forbid_mask, int32_t n_rec, int32_t t_rec, int32_t n_spans, int32_t t_span,
                                    int32_t beam, int32_t min_pred, int32_t max_pred, int32_t* best_preds, float* best_lprobs,
                                    int32_t* mult_preds, float* mult_lprobs, int32_t* out_sizes, void* workspace,
                                    size_t workspace_bytes, void* stream) {
  const char* who = "decode_spans";
  const char* missing = !ctx ? "ctx" : !frame_embs ? "frame_embs" : !spans ? "spans" : !bos_ids ? "bos_ids" : !best_preds ? "best_preds"
                      : !best_lprobs ? "best_lprobs" : !mult_preds ? "mult_preds" : !mult_lprobs ? "mult_lprobs"
                      : !out_sizes ? "out_sizes" : !workspace ? "workspace" : nullptr;
  if (missing) {
    cn_set_error("%s: %s is NULL", who, missing);
    return CN_ERR_ARG;
  }
  if (n_rec < 1 || t_rec < 1) {
    cn_set_error("%s: n_rec=%d t_rec=%d (both at least 1)", who, n_rec, t_rec);
    return CN_ERR_ARG;
  }
  if (n_spans < 1) {
    cn_set_error("%s: n_spans=%d (expected at least 1)", who, n_spans);
    return CN_ERR_ARG;
  }
  if (t_span < 1) {
    cn_set_error("%s: t_span=%d (expected at least 1)", who, t_span);
    return CN_ERR_ARG;
  }
  if (beam < 1 || beam > CN_MAX_BEAM) {
    cn_set_error("%s: beam=%d unsupported (1..%d)", who, beam, CN_MAX_BEAM);
    return CN_ERR_ARG;
  }
  CN_TRY(dec_check_model(ctx, who, max_pred, min_pred, "%s: max_pred=%d (1..%d) min_pred=%d unsupported", who, max_pred, CN_MAX_PRED,
                         min_pred));
  if (!spans_shape_ok(ctx, n_rec, t_rec, n_spans, t_span)) {
    cn_set_error("%s: n_rec=%d x t_rec=%d frames or n_spans=%d x t_span=%d frames in one call are too many (split the call)", who, n_rec,
                 t_rec, n_spans, t_span);
    return CN_ERR_ARG;
  }
  CN_TRY(dec_check_workspace(who, workspace_bytes, conette_decode_spans_workspace_bytes(ctx, n_rec, t_rec, n_spans, t_span, beam, max_pred)));
  DecArgs a;
  memset(&a, 0, sizeof(a));  // (padding included: the record is the graph key)
  a.frame_embs = frame_embs, a.bos_ids = bos_ids, a.forbid = forbid_mask;
  a.best_preds = best_preds, a.best_lprobs = best_lprobs, a.mult_preds = mult_preds, a.mult_lprobs = mult_lprobs;
  a.out_sizes = out_sizes, a.ws = (char*)workspace;
  a.B = n_spans, a.Ta = t_span, a.beam = beam, a.min_pred = min_pred, a.maxp = max_pred;
  a.spans = spans, a.n_rec = n_rec, a.t_rec = t_rec, a.n_spans = n_spans;
  hipStream_t s = (hipStream_t)stream;
  auto run = [&]() -> int { CN_BY_PRECISION(ctx, decode_impl<OT>(ctx, a, s)); };
  hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;  // (the caller captures: as conette_decode)
  CN_HIP(hipStreamIsCapturing(s, &cap));
  if (cap != hipStreamCaptureStatusNone) return run();
  return dec_graph_run(ctx, a, s, run);
}

// ---- teacher forcing as ONE causal pass (nn/decoding/forcing.py:12-71 is a single decoder forward over the caption) ----
// Rows r = clip * cap_len + position: every GEMM of the layer runs once on all B * cap_len rows (the unfused per-sub-layer
// kernels of the step path with M = B * cap_len), the cross-attention kernel is reused with "beam" = cap_len, and the
// self-attention reads the K / V of the clip's earlier positions from this pass's own QKV output -- at cache precision
// (rounded to the operand type exactly as the step path stores and re-reads them), masked to valid (non-pad) keys <= t.
// conette_score runs the same pass over `cpa` captions per clip (rows r = (clip * cpa + caption) * cap_len + position; the
// projection and the cross-attention K / V once per CLIP, the cross-attention's "beam" = cpa * cap_len) and ends in the fused
// classifier + log-soft-max + gather of dec_score.h instead of the classifier GEMM.
// conette_align is conette_score's pass with the cross-attention kernel of dec_align.h, which also stores the attention weights.
struct CnScoreOut {  // conette_score's tail of the pass
  const int32_t* targets;
  float* tok_lprobs;  // may be null
  float* sum_lprobs;
  int32_t* n_tokens;
};
template <typename T>
static int forcing_prefill_impl(conette_ctx* ctx, const float* frame_embs, const int32_t* frame_lens, const int32_t* caps,
                                int B, int Ta, int cpa, int cap_len, float* logits, const CnScoreOut* score, char* wsp,
                                hipStream_t s, const CnAlignOut* align = nullptr) {
  const conette_config& cfg = ctx->cfg;
  const int d = cfg.d_model, NL = cfg.n_layers, R = B * cpa * cap_len, V = cfg.vocab_size;
  DecWs w = dec_ws(ctx, B, Ta, cpa * cap_len, 1, wsp, score || align);  // rows = B * cpa * cap_len ("beam" = cpa * cap_len, one step)
  T* xt = (T*)w.xt;
  const float scale = 1.0f / sqrtf((float)(d / cfg.nhead));
  const int rblocks = cn_cdiv(R, 4);
  CN_TRY(dec_prepare<T>(ctx, frame_embs, B, Ta, w, s));
  hipLaunchKernelGGL((cn_embed_kernel<T>), dim3(rblocks), dim3(256), 0, s, caps, ctx->emb, ctx->pe, 0, cap_len, R,
                     sqrtf((float)d), w.x, xt);
  CN_LAUNCH_CHECK();
  auto self_attn = [&](int) {
    hipLaunchKernelGGL((cn_self_attn_causal_kernel<T>), dim3(rblocks), dim3(256), 0, s, w.qkv, caps, cap_len, R, cfg.pad_id,
                       scale, (T*)w.attn_t);
  };
  // (ffn2_split = false at every precision: FFN2 as one GEMM is the summation order the outputs of this pass are defined by)
  if (align) {  // conette_align: the cross-attention that keeps its weights (dec_align.h); the plain kernel where a layer has no output
    const uint32_t sel = align->layer_mask;
    const int first = __builtin_ctz(sel), last = 31 - __builtin_clz(sel);
    const float inv_sel = 1.0f / (float)__builtin_popcount(sel);
    const int kv_ld = NL * 2 * d;
    auto cross_attn = [&](int l) {
      const int mode = !((sel >> l) & 1) ? 0 : ((l == first ? AL_FIRST : AL_ADD) | (l == last ? AL_LAST : 0));
      float* plane = align->attn_layers ? align->attn_layers + (size_t)l * R * Ta : nullptr;
      if (mode == 0 && !plane)
        hipLaunchKernelGGL((cn_cross_attn_kernel<T>), dim3(rblocks), dim3(256), 0, s, w.q, (T*)w.kvc, kv_ld, l * 2 * d, frame_lens, R,
                           cpa * cap_len, Ta, scale, (T*)w.attn_t);
      else
        hipLaunchKernelGGL((cn_cross_attn_align_kernel<T>), dim3(rblocks), dim3(256), 0, s, w.q, (T*)w.kvc, kv_ld, l * 2 * d,
                           frame_lens, caps, cfg.pad_id, R, cpa * cap_len, Ta, scale, (T*)w.attn_t, plane, align->attn, mode, inv_sel);
    };
    for (int l = 0; l < NL; ++l)
      CN_TRY((dec_sublayer_layer<T>(ctx, w, l, frame_lens, R, Ta, cpa * cap_len, false, self_attn, s, cross_attn)));
    if (!score) return CN_OK;  // no targets: the classifier is not run
  } else {
    for (int l = 0; l < NL; ++l) CN_TRY((dec_sublayer_layer<T>(ctx, w, l, frame_lens, R, Ta, cpa * cap_len, false, self_attn, s)));
  }
  CnProfScope ps(ctx, CONETTE_PROF_DEC_GEMM, s);
  if (score) {  // no logits: every row's log-probability of its target, summed per caption (dec_score.h)
    const int S = cn_score_slabs(R, V, ctx->n_cu, ctx->score_vsplit);
    return cn_score_launch<T>(xt, (const T*)ctx->cls_w, ctx->cls_b, score->targets, B * cpa, cap_len, V, S, cfg.pad_id,
                              (float*)(wsp + w.total), score->tok_lprobs, score->sum_lprobs, score->n_tokens, s);
  }
  EpiBiasAct<float, ACT_NONE> ec{ctx->cls_b, logits, V, ACT_NONE};  // (B, cap_len, V) written in place
  CN_TRY(cn_mm(xt, d, (const T*)ctx->cls_w, d, R, V, d, ec, s));
  return CN_OK;
}

extern "C" size_t conette_forcing_workspace_bytes(const conette_ctx* ctx, int32_t batch, int32_t t_audio,
                                                  int32_t cap_len) {
  if (!ctx || batch <= 0 || t_audio <= 0 || cap_len <= 0) return 0;
  // step path: decode workspace at beam 1 + the int32 scratch the search bookkeeping of a normal decode writes into;
  // one-pass path: the same buffers laid out for B * cap_len rows
  const size_t stepwise = conette_decode_workspace_bytes(ctx, batch, t_audio, 1, cap_len) + cn_align((size_t)batch * cap_len * 8) +
                          cn_align((size_t)batch * 16);
  const size_t onepass = dec_ws(ctx, batch, t_audio, cap_len, 1, nullptr).total;
  return stepwise > onepass ? stepwise : onepass;
}

extern "C" int conette_forcing(conette_ctx* ctx, const float* frame_embs, const int32_t* frame_lens,
                               const int32_t* caps_in, int32_t batch, int32_t t_audio, int32_t cap_len, float* logits,
                               void* workspace, size_t workspace_bytes, void* stream) {
  if (!ctx || !frame_embs || !frame_lens || !caps_in || !logits || !workspace || batch <= 0 || t_audio <= 0) {
    cn_set_error("forcing: bad argument");
    return CN_ERR_ARG;
  }
  CN_TRY(dec_check_model(ctx, "forcing", cap_len, 0, "forcing: cap_len=%d unsupported (1..%d)", cap_len, CN_MAX_PRED));
  CN_TRY(dec_check_workspace("forcing", workspace_bytes, conette_forcing_workspace_bytes(ctx, batch, t_audio, cap_len)));
  hipStream_t s = (hipStream_t)stream;
  if (!ctx->forcing_stepwise) {  // default: one causal pass over all caption positions
    CN_BY_PRECISION(ctx, forcing_prefill_impl<OT>(ctx, frame_embs, frame_lens, caps_in, batch, t_audio, 1, cap_len, logits,
                                          nullptr, (char*)workspace, s));
  }
  // CONETTE_OPT_FORCING_STEPWISE: the KV-cached step kernels fed with the caption (cross-check of the pass above)
  // outputs of the search bookkeeping that a forced pass does not produce: parked in the workspace tail
  char* tail = (char*)workspace + conette_decode_workspace_bytes(ctx, batch, t_audio, 1, cap_len);
  DecArgs a = {};
  a.frame_embs = frame_embs, a.frame_lens = frame_lens, a.ws = (char*)workspace;
  a.bos_ids = caps_in;  // init kernel input; any valid ids
  a.B = batch, a.Ta = t_audio, a.beam = 1, a.min_pred = 0, a.maxp = cap_len;
  a.mult_preds = a.best_preds = (int32_t*)tail;
  a.mult_lprobs = a.best_lprobs = (float*)(tail + cn_align((size_t)batch * cap_len * 4));
  a.out_sizes = (int32_t*)(tail + cn_align((size_t)batch * cap_len * 8));
  a.force_caps = caps_in, a.force_logits = logits;
  CN_BY_PRECISION(ctx, decode_impl<OT>(ctx, a, s));
}

extern "C" size_t conette_score_workspace_bytes(const conette_ctx* ctx, int32_t n_audio, int32_t t_audio,
                                                int32_t caps_per_audio, int32_t cap_len) {
  if (!ctx || n_audio <= 0 || t_audio <= 0 || caps_per_audio <= 0 || cap_len <= 0) return 0;
  const long rows = (long)n_audio * caps_per_audio * cap_len;
  if (rows > 0x7fffffffL / 4096) return 0;  // (row * 768 floats of the QKV buffer is indexed in 32 bits by the GEMM epilogues)
  const int R = (int)rows;
  const int S = cn_score_slabs(R, ctx->cfg.vocab_size, ctx->n_cu, ctx->score_vsplit);
  return dec_ws(ctx, n_audio, t_audio, caps_per_audio * cap_len, 1, nullptr, true).total + cn_score_part_bytes(R, S);
}

extern "C" int conette_score(conette_ctx* ctx, const float* frame_embs, const int32_t* frame_lens, const int32_t* caps_in,
                             const int32_t* targets, int32_t n_audio, int32_t t_audio, int32_t caps_per_audio,
                             int32_t cap_len, float* tok_lprobs, float* sum_lprobs, int32_t* n_tokens, void* workspace,
                             size_t workspace_bytes, void* stream) {
  if (!ctx || !frame_embs || !frame_lens || !caps_in || !targets || !sum_lprobs || !n_tokens || !workspace || n_audio <= 0 ||
      t_audio <= 0) {
    cn_set_error("score: bad argument");
    return CN_ERR_ARG;
  }
  CN_TRY(dec_check_model(ctx, "score", cap_len, 0, "score: cap_len=%d unsupported (1..%d)", cap_len, CN_MAX_PRED));
  if (caps_per_audio < 1) {
    cn_set_error("score: caps_per_audio=%d < 1", caps_per_audio);
    return CN_ERR_ARG;
  }
  const size_t need = conette_score_workspace_bytes(ctx, n_audio, t_audio, caps_per_audio, cap_len);
  if (need == 0) {
    cn_set_error("score: %d x %d x %d rows in one call are too many (split the call)", n_audio, caps_per_audio, cap_len);
    return CN_ERR_ARG;
  }
  CN_TRY(dec_check_workspace("score", workspace_bytes, need));
  const CnScoreOut out{targets, tok_lprobs, sum_lprobs, n_tokens};
  CN_BY_PRECISION(ctx, forcing_prefill_impl<OT>(ctx, frame_embs, frame_lens, caps_in, n_audio, t_audio, caps_per_audio, cap_len,
                                                nullptr, &out, (char*)workspace, (hipStream_t)stream));
}

// ---- alignment (dec_align.h): conette_score's pass with the cross-attention weights kept ----
extern "C" size_t conette_align_workspace_bytes(const conette_ctx* ctx, int32_t n_audio, int32_t t_audio, int32_t caps_per_audio,
                                                int32_t cap_len, int32_t with_scores) {
  if (!ctx || n_audio <= 0 || t_audio <= 0 || caps_per_audio <= 0 || cap_len <= 0) return 0;
  const long rows = (long)n_audio * caps_per_audio * cap_len;
  if (rows > 0x7fffffffL / 4096) return 0;  // (as conette_score)
  const int R = (int)rows;
  const size_t lean = dec_ws(ctx, n_audio, t_audio, caps_per_audio * cap_len, 1, nullptr, true).total;
  if (!with_scores) return lean;
  return lean + cn_score_part_bytes(R, cn_score_slabs(R, ctx->cfg.vocab_size, ctx->n_cu, ctx->score_vsplit));
}

extern "C" int conette_align(conette_ctx* ctx, const float* frame_embs, const int32_t* frame_lens, const int32_t* caps_in,
                             const int32_t* targets, int32_t n_audio, int32_t t_audio, int32_t caps_per_audio, int32_t cap_len,
                             uint32_t layer_mask, float* attn, float* attn_layers, float* tok_lprobs, float* sum_lprobs,
                             int32_t* n_tokens, void* workspace, size_t workspace_bytes, void* stream) {
  if (!ctx || !frame_embs || !frame_lens || !caps_in || !attn || !workspace || n_audio <= 0 || t_audio <= 0) {
    cn_set_error("align: bad argument");
    return CN_ERR_ARG;
  }
  if (targets ? (!sum_lprobs || !n_tokens) : (tok_lprobs || sum_lprobs || n_tokens)) {
    cn_set_error("align: sum_lprobs and n_tokens go with targets (all given, or all NULL together with tok_lprobs)");
    return CN_ERR_ARG;
  }
  CN_TRY(dec_check_model(ctx, "align", cap_len, 0, "align: cap_len=%d unsupported (1..%d)", cap_len, CN_MAX_PRED));
  if (caps_per_audio < 1) {
    cn_set_error("align: caps_per_audio=%d < 1", caps_per_audio);
    return CN_ERR_ARG;
  }
  const int NL = ctx->cfg.n_layers;
  const uint32_t all = NL >= 32 ? ~0u : ((1u << NL) - 1u);
  if (layer_mask & ~all) {
    cn_set_error("align: layer_mask=0x%x selects a layer at or above n_layers=%d", layer_mask, NL);
    return CN_ERR_ARG;
  }
  const size_t need = conette_align_workspace_bytes(ctx, n_audio, t_audio, caps_per_audio, cap_len, targets != nullptr);
  if (need == 0) {
    cn_set_error("align: %d x %d x %d rows in one call are too many (split the call)", n_audio, caps_per_audio, cap_len);
    return CN_ERR_ARG;
  }
  CN_TRY(dec_check_workspace("align", workspace_bytes, need));
  const CnScoreOut out{targets, tok_lprobs, sum_lprobs, n_tokens};
  const CnAlignOut al{attn, attn_layers, layer_mask ? layer_mask : all};
  CN_BY_PRECISION(ctx, forcing_prefill_impl<OT>(ctx, frame_embs, frame_lens, caps_in, n_audio, t_audio, caps_per_audio, cap_len,
                                                nullptr, targets ? &out : nullptr, (char*)workspace, (hipStream_t)stream, &al));
}

extern "C" int conette_greedy(conette_ctx* ctx, const float* frame_embs, const int32_t* frame_lens, const int32_t* bos_ids,
                              const uint8_t* forbid_mask, int32_t batch, int32_t t_audio, int32_t min_pred,
                              int32_t max_pred, float* logits, int32_t* preds, int32_t* out_sizes, void* workspace,
                              size_t workspace_bytes, void* stream) {
  if (!ctx || !frame_embs || !frame_lens || !bos_ids || !logits || !preds || !out_sizes || !workspace || batch <= 0 ||
      t_audio <= 0) {
    cn_set_error("greedy: bad argument");
    return CN_ERR_ARG;
  }
  CN_TRY(dec_check_model(ctx, "greedy", max_pred, min_pred, "greedy: max_pred=%d (1..%d) min_pred=%d unsupported", max_pred, CN_MAX_PRED,
                         min_pred));
  CN_TRY(dec_check_workspace("greedy", workspace_bytes, conette_greedy_workspace_bytes(ctx, batch, t_audio, max_pred)));
  char* tail = (char*)workspace + conette_decode_workspace_bytes(ctx, batch, t_audio, 1, max_pred);
  DecArgs a = {};
  a.frame_embs = frame_embs, a.frame_lens = frame_lens, a.bos_ids = bos_ids, a.forbid = forbid_mask, a.ws = (char*)workspace;
  a.B = batch, a.Ta = t_audio, a.beam = 1, a.min_pred = min_pred, a.maxp = max_pred;
  a.best_preds = preds, a.out_sizes = out_sizes, a.greedy_logits = logits;
  a.mult_preds = (int32_t*)tail;  // beam 1: the single hypothesis of every clip
  a.mult_lprobs = (float*)(tail + cn_align((size_t)batch * max_pred * 4));
  a.best_lprobs = (float*)(tail + cn_align((size_t)batch * max_pred * 4) + cn_align((size_t)batch * 4));
  CN_BY_PRECISION(ctx, decode_impl<OT>(ctx, a, (hipStream_t)stream));
}

// ---- sampling (dec_sample.h): the step path with the per-row sampling decision in place of the search step ----
extern "C" size_t conette_sample_workspace_bytes(const conette_ctx* ctx, int32_t batch, int32_t t_audio, int32_t n_samples,
                                                 int32_t max_pred) {
  if (!ctx || batch <= 0 || t_audio <= 0 || n_samples <= 0 || max_pred <= 0) return 0;
  return conette_decode_workspace_bytes(ctx, batch, t_audio, n_samples, max_pred);
}

extern "C" int conette_sample(conette_ctx* ctx, const float* frame_embs, const int32_t* frame_lens, const int32_t* bos_ids,
                              const uint8_t* forbid_mask, const float* uniforms, int32_t batch, int32_t t_audio,
                              int32_t n_samples, int32_t min_pred, int32_t max_pred, float temperature, int32_t top_k,
                              float top_p, int32_t* preds, float* sum_lprobs, int32_t* lens, int32_t* out_sizes,
                              float* tok_lprobs, float* step_logits, void* workspace, size_t workspace_bytes, void* stream) {
  if (!ctx || !frame_embs || !frame_lens || !bos_ids || !uniforms || !preds || !sum_lprobs || !lens || !out_sizes || !workspace ||
      batch <= 0 || t_audio <= 0) {
    cn_set_error("sample: bad argument");
    return CN_ERR_ARG;
  }
  if (n_samples < 1 || n_samples > CN_MAX_BEAM) {
    cn_set_error("sample: n_samples=%d unsupported (1..%d)", n_samples, CN_MAX_BEAM);
    return CN_ERR_ARG;
  }
  if (!(temperature > 0.f) || !(temperature < INFINITY)) {
    cn_set_error("sample: temperature=%g must be finite and > 0", (double)temperature);
    return CN_ERR_ARG;
  }
  if (top_k < 0) {
    cn_set_error("sample: top_k=%d < 0", top_k);
    return CN_ERR_ARG;
  }
  if (!(top_p > 0.f) || !(top_p <= 1.f)) {
    cn_set_error("sample: top_p=%g outside (0, 1]", (double)top_p);
    return CN_ERR_ARG;
  }
  CN_TRY(dec_check_model(ctx, "sample", max_pred, min_pred, "sample: max_pred=%d (1..%d) min_pred=%d unsupported", max_pred,
                         CN_MAX_PRED, min_pred));
  if (ctx->cfg.vocab_size > SM_T * SM_MAX_SLABS) {
    cn_set_error("sample: vocab_size=%d unsupported (at most %d)", ctx->cfg.vocab_size, SM_T * SM_MAX_SLABS);
    return CN_ERR_ARG;
  }
  CN_TRY(dec_check_workspace("sample", workspace_bytes, conette_sample_workspace_bytes(ctx, batch, t_audio, n_samples, max_pred)));
  DecArgs a;
  memset(&a, 0, sizeof(a));
  a.frame_embs = frame_embs, a.frame_lens = frame_lens, a.bos_ids = bos_ids, a.forbid = forbid_mask, a.ws = (char*)workspace;
  a.B = batch, a.Ta = t_audio, a.beam = n_samples, a.min_pred = min_pred, a.maxp = max_pred;
  a.mult_preds = preds, a.mult_lprobs = sum_lprobs, a.out_sizes = out_sizes;
  a.uniforms = uniforms, a.sample_lens = lens, a.sample_tok_lp = tok_lprobs, a.sample_step_logits = step_logits;
  a.temperature = temperature, a.top_p = top_p, a.top_k = top_k;
  // (eager: the caller's output buffers usually change from call to call, which a graph cache keyed on them would only churn
  //  through; the launch sequence is static and holds no host state, so the caller may capture it)
  CN_BY_PRECISION(ctx, decode_impl<OT>(ctx, a, (hipStream_t)stream));
}

// ---- diverse beam search (dec_group.h): the step path with the groups' sequential top-k in place of the search step ----
static bool groups_shape_ok(int32_t n_groups, int32_t group_beam) {
  return n_groups >= 1 && group_beam >= 1 && n_groups <= CN_MAX_BEAM && group_beam <= CN_MAX_BEAM && n_groups * group_beam <= CN_MAX_BEAM;
}
extern "C" size_t conette_decode_groups_workspace_bytes(const conette_ctx* ctx, int32_t batch, int32_t t_audio, int32_t n_groups,
                                                        int32_t group_beam, int32_t max_pred) {
  if (!ctx || batch <= 0 || t_audio <= 0 || max_pred <= 0 || !groups_shape_ok(n_groups, group_beam)) return 0;
  return conette_decode_workspace_bytes(ctx, batch, t_audio, n_groups * group_beam, max_pred) + cn_align((size_t)batch * n_groups * 4);
}

extern "C" int conette_decode_groups(conette_ctx* ctx, const float* frame_embs, const int32_t* frame_lens, const int32_t* bos_ids,
                                     const uint8_t* forbid_mask, int32_t batch, int32_t t_audio, int32_t n_groups,
                                     int32_t group_beam, float diversity_penalty, int32_t min_pred, int32_t max_pred,
                                     int32_t* best_preds, float* best_lprobs, int32_t* mult_preds, float* mult_lprobs,
                                     int32_t* out_sizes, int32_t* trace_sel, float* trace_val, float* step_logits, void* workspace,
                                     size_t workspace_bytes, void* stream) {
  if (!ctx || !frame_embs || !frame_lens || !bos_ids || !best_preds || !best_lprobs || !mult_preds || !mult_lprobs ||
      !out_sizes || !workspace || batch <= 0 || t_audio <= 0) {
    cn_set_error("decode_groups: bad argument");
    return CN_ERR_ARG;
  }
  if (!groups_shape_ok(n_groups, group_beam)) {
    cn_set_error("decode_groups: n_groups=%d x group_beam=%d unsupported (both >= 1, product <= %d)", n_groups, group_beam, CN_MAX_BEAM);
    return CN_ERR_ARG;
  }
  if (!(diversity_penalty >= 0.f) || !(diversity_penalty < INFINITY)) {
    cn_set_error("decode_groups: diversity_penalty=%g must be finite and >= 0", (double)diversity_penalty);
    return CN_ERR_ARG;
  }
  CN_TRY(dec_check_model(ctx, "decode_groups", max_pred, min_pred, "decode_groups: max_pred=%d (1..%d) min_pred=%d unsupported", max_pred,
                         CN_MAX_PRED, min_pred));
  CN_TRY(dec_check_workspace("decode_groups", workspace_bytes,
                             conette_decode_groups_workspace_bytes(ctx, batch, t_audio, n_groups, group_beam, max_pred)));
  DecArgs a;
  memset(&a, 0, sizeof(a));
  a.frame_embs = frame_embs, a.frame_lens = frame_lens, a.bos_ids = bos_ids, a.forbid = forbid_mask, a.ws = (char*)workspace;
  a.best_preds = best_preds, a.best_lprobs = best_lprobs, a.mult_preds = mult_preds, a.mult_lprobs = mult_lprobs;
  a.out_sizes = out_sizes, a.trace_sel = trace_sel, a.trace_val = trace_val;
  a.B = batch, a.Ta = t_audio, a.beam = n_groups * group_beam, a.min_pred = min_pred, a.maxp = max_pred;
  a.n_groups = n_groups, a.group_beam = group_beam, a.diversity = diversity_penalty, a.group_step_logits = step_logits;
  // (eager, as conette_sample: the launch sequence is static and holds no host state, so the caller may capture it)
  CN_BY_PRECISION(ctx, decode_impl<OT>(ctx, a, (hipStream_t)stream));
}

// ---- constrained beam search (dec_constrain.h): the step path with the steered step in place of the search step ----
extern "C" size_t conette_decode_constrained_workspace_bytes(const conette_ctx* ctx, int32_t batch, int32_t t_audio, int32_t beam,
                                                             int32_t max_pred) {
  if (!ctx || batch <= 0 || t_audio <= 0 || max_pred <= 0 || beam < 1 || beam > CN_MAX_BEAM) return 0;
  return conette_decode_workspace_bytes(ctx, batch, t_audio, beam, max_pred);  // (the step keeps nothing of its own between launches)
}

// The checks and the launch of conette_decode_constrained and conette_decode_required (`who`); req_width 0: no requirements.
static int decode_steered(const char* who, conette_ctx* ctx, const float* frame_embs, const int32_t* frame_lens, const int32_t* bos_ids,
                          const uint8_t* forbid_mask, const int32_t* prefix, const int32_t* prefix_lens, int32_t prefix_width,
                          const uint8_t* ban_mask, int32_t no_repeat_ngram, const int32_t* req_tokens, const int32_t* req_groups,
                          int32_t req_width, int32_t batch, int32_t t_audio, int32_t beam, int32_t min_pred, int32_t max_pred,
                          int32_t* best_preds, float* best_lprobs, int32_t* mult_preds, float* mult_lprobs, int32_t* out_sizes,
                          int32_t* trace_sel, float* trace_val, float* step_logits, void* workspace, size_t workspace_bytes,
                          void* stream) {
  if (!ctx || !frame_embs || !frame_lens || !bos_ids || !best_preds || !best_lprobs || !mult_preds || !mult_lprobs ||
      !out_sizes || !workspace || batch <= 0 || t_audio <= 0) {
    cn_set_error("%s: bad argument", who);
    return CN_ERR_ARG;
  }
  if (beam < 1 || beam > CN_MAX_BEAM) {
    cn_set_error("%s: beam=%d unsupported (1..%d)", who, beam, CN_MAX_BEAM);
    return CN_ERR_ARG;
  }
  CN_TRY(dec_check_model(ctx, who, max_pred, min_pred, "%s: max_pred=%d (1..%d) min_pred=%d unsupported", who, max_pred, CN_MAX_PRED,
                         min_pred));
  if (prefix_width < 0 || prefix_width > max_pred - 1) {
    cn_set_error("%s: prefix_width=%d outside 0 .. max_pred - 1 = %d", who, prefix_width, max_pred - 1);
    return CN_ERR_ARG;
  }
  if (prefix_width > 0 && (!prefix || !prefix_lens)) {
    cn_set_error("%s: prefix and prefix_lens must be given with prefix_width=%d > 0", who, prefix_width);
    return CN_ERR_ARG;
  }
  if (no_repeat_ngram < 0 || no_repeat_ngram > CN_MAX_NGRAM) {
    cn_set_error("%s: no_repeat_ngram=%d outside 0 .. %d", who, no_repeat_ngram, CN_MAX_NGRAM);
    return CN_ERR_ARG;
  }
  if (req_width < 0 || req_width > RQ_MAX_TOKENS) {
    cn_set_error("%s: req_width=%d outside 0 .. %d", who, req_width, RQ_MAX_TOKENS);
    return CN_ERR_ARG;
  }
  if (req_width > 0 && (!req_tokens || !req_groups)) {
    cn_set_error("%s: req_tokens and req_groups must be given with req_width=%d > 0", who, req_width);
    return CN_ERR_ARG;
  }
  CN_TRY(dec_check_workspace(who, workspace_bytes, conette_decode_workspace_bytes(ctx, batch, t_audio, beam, max_pred)));
  if (req_width > 0) {  // the group indices, read back unless the stream is capturing (then a bad entry counts as unused)
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    CN_HIP(hipStreamIsCapturing((hipStream_t)stream, &cap));
    if (cap == hipStreamCaptureStatusNone) {
      const size_t n = (size_t)batch * req_width;
      int32_t* host = (int32_t*)malloc(n * sizeof(int32_t));
      if (!host) {
        cn_set_error("%s: out of host memory", who);
        return CN_ERR_ARG;
      }
      hipError_t e = hipMemcpyAsync(host, req_groups, n * sizeof(int32_t), hipMemcpyDeviceToHost, (hipStream_t)stream);
      if (e == hipSuccess) e = hipStreamSynchronize((hipStream_t)stream);
      size_t bad = n;
      if (e == hipSuccess)
        for (size_t i = 0; i < n && bad == n; ++i)
          if (host[i] < -1 || host[i] >= RQ_MAX_GROUPS) bad = i;
      const int32_t bad_value = bad < n ? host[bad] : 0;
      free(host);
      CN_HIP(e);
      if (bad < n) {
        cn_set_error("%s: req_groups[%d][%d]=%d outside -1 .. %d", who, (int)(bad / req_width), (int)(bad % req_width), bad_value,
                     RQ_MAX_GROUPS - 1);
        return CN_ERR_ARG;
      }
    }
  }
  DecArgs a;
  memset(&a, 0, sizeof(a));
  a.frame_embs = frame_embs, a.frame_lens = frame_lens, a.bos_ids = bos_ids, a.forbid = forbid_mask, a.ws = (char*)workspace;
  a.best_preds = best_preds, a.best_lprobs = best_lprobs, a.mult_preds = mult_preds, a.mult_lprobs = mult_lprobs;
  a.out_sizes = out_sizes, a.trace_sel = trace_sel, a.trace_val = trace_val;
  a.B = batch, a.Ta = t_audio, a.beam = beam, a.min_pred = min_pred, a.maxp = max_pred;
  a.constrained = 1, a.prefix_width = prefix_width, a.no_repeat_ngram = no_repeat_ngram;
  if (prefix_width > 0) a.prefix = prefix, a.prefix_lens = prefix_lens;
  a.ban = ban_mask, a.constrain_step_logits = step_logits;
  if (req_width > 0) a.req_width = req_width, a.req_tokens = req_tokens, a.req_groups = req_groups;
  // (eager, as conette_sample: the launch sequence is static and holds no host state, so the caller may capture it)
  CN_BY_PRECISION(ctx, decode_impl<OT>(ctx, a, (hipStream_t)stream));
}

extern "C" int conette_decode_constrained(conette_ctx* ctx, const float* frame_embs, const int32_t* frame_lens, const int32_t* bos_ids,
                                          const uint8_t* forbid_mask, const int32_t* prefix, const int32_t* prefix_lens,
                                          int32_t prefix_width, const uint8_t* ban_mask, int32_t no_repeat_ngram, int32_t batch,
                                          int32_t t_audio, int32_t beam, int32_t min_pred, int32_t max_pred, int32_t* best_preds,
                                          float* best_lprobs, int32_t* mult_preds, float* mult_lprobs, int32_t* out_sizes,
                                          int32_t* trace_sel, float* trace_val, float* step_logits, void* workspace,
                                          size_t workspace_bytes, void* stream) {
  return decode_steered("decode_constrained", ctx, frame_embs, frame_lens, bos_ids, forbid_mask, prefix, prefix_lens, prefix_width,
                        ban_mask, no_repeat_ngram, nullptr, nullptr, 0, batch, t_audio, beam, min_pred, max_pred, best_preds, best_lprobs,
                        mult_preds, mult_lprobs, out_sizes, trace_sel, trace_val, step_logits, workspace, workspace_bytes, stream);
}

// ---- keyword-guided beam search (dec_require.h): the constrained search with per-clip requirements ----
extern "C" size_t conette_decode_required_workspace_bytes(const conette_ctx* ctx, int32_t batch, int32_t t_audio, int32_t beam,
                                                          int32_t max_pred) {
  return conette_decode_constrained_workspace_bytes(ctx, batch, t_audio, beam, max_pred);  // (a row's requirement state is its sequence)
}

extern "C" int conette_decode_required(conette_ctx* ctx, const float* frame_embs, const int32_t* frame_lens, const int32_t* bos_ids,
                                       const uint8_t* forbid_mask, const int32_t* prefix, const int32_t* prefix_lens,
                                       int32_t prefix_width, const uint8_t* ban_mask, int32_t no_repeat_ngram, const int32_t* req_tokens,
                                       const int32_t* req_groups, int32_t req_width, int32_t batch, int32_t t_audio, int32_t beam,
                                       int32_t min_pred, int32_t max_pred, int32_t* best_preds, float* best_lprobs, int32_t* mult_preds,
                                       float* mult_lprobs, int32_t* out_sizes, int32_t* trace_sel, float* trace_val, float* step_logits,
                                       void* workspace, size_t workspace_bytes, void* stream) {
  return decode_steered("decode_required", ctx, frame_embs, frame_lens, bos_ids, forbid_mask, prefix, prefix_lens, prefix_width, ban_mask,
                        no_repeat_ngram, req_tokens, req_groups, req_width, batch, t_audio, beam, min_pred, max_pred, best_preds,
                        best_lprobs, mult_preds, mult_lprobs, out_sizes, trace_sel, trace_val, step_logits, workspace, workspace_bytes,
                        stream);
}

extern "C" size_t conette_greedy_workspace_bytes(const conette_ctx* ctx, int32_t batch, int32_t t_audio, int32_t max_pred) {
  if (!ctx || batch <= 0 || t_audio <= 0 || max_pred <= 0) return 0;
  return conette_decode_workspace_bytes(ctx, batch, t_audio, 1, max_pred) + cn_align((size_t)batch * max_pred * 4) +
         2 * cn_align((size_t)batch * 4);
}

extern "C" int conette_debug_dbprof(unsigned long long* out16, int reset) {
  if (out16) {
    CN_HIP(hipMemcpyFromSymbol(out16, HIP_SYMBOL(g_db_prof), 128));
    CN_HIP(hipMemcpyFromSymbol(out16 + 16, HIP_SYMBOL(g_s3_prof), 128));
  }
  if (reset) {
    unsigned long long z[16] = {0};
    CN_HIP(hipMemcpyToSymbol(HIP_SYMBOL(g_db_prof), z, 128));
    CN_HIP(hipMemcpyToSymbol(HIP_SYMBOL(g_s3_prof), z, 128));
  }
  return CN_OK;
}
