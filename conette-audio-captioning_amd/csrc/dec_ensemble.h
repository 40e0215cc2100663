// Ensemble beam search (conette_decode_ensemble, include/conette_hip.h; the CPU restatement of the rule is
// conette_amd/ensemble_search.py): one search step of one clip whose candidates are scored by M <= 4 members -- checkpoints, or
// one checkpoint under several task tokens -- that decode ONE hypothesis tree in lockstep.
//
// Shared.  prefix / anc / slot / sum_lp / cur_tok / n_active / live are the plain search's (SsArgs), in member 0's workspace; every
// member's block, attention and FFN kernels read them.  A member owns its weights, cross K/V, KV cache, activations and logits.
// One step.  Per member m and candidate row p, lp_m(p, .) = the log-softmax of member m's logits masked as the plain search masks
// them -- EOS floor while step < min_pred, forbid-repeat over the row's prefix with member m's OWN task token at position 0 -- in
// the expressions and the summation order of the plain step kernels, so lp_m is bit for bit conette_decode's.  Combination:
//   M == 1              c = lp_0, no arithmetic
//   rule 0 ("logprob")  c = sum_m w_m * lp_m                      (product of experts: -inf where any member is -inf)
//   rule 1 ("prob")     c = log sum_m w_m * exp(lp_m)             (mixture: -inf only where every member is -inf), accumulated as
//                       a running log-add-exp of lp_m + log w_m, so it never underflows where some lp_m is finite
// accumulated in the order M - 1, 0, 1, .., M - 2 (the member whose statistics were taken last is still in registers).  The score
// is sum_lp[p] + c (step 0: c); top-k, ties, margins and the bookkeeping (cn_search_commit) are the plain search's.
//
// Two kernels, as for the plain search.  Register-resident (V <= 8192 and beam <= 4, or V <= 6144 and beam <= 8; 1024 threads): the members are STREAMED through
// the one register array val[NR][VPT] -- a pass per member takes the log-softmax statistics of all rows (the array holds that
// member's masked logits), the last member's values are turned into its term in place, and the other members' terms are added row
// by row from logits that are L2-resident by then (VPT values in flight).  Generic (256 threads): the members' logits are never
// masked in place -- every read applies the masks on the fly -- and the combined scores of the clip's rows go through a
// (R, ldv) array in member 0's workspace, over which the k rounds of block arg-max run as the plain generic step's do.
#pragma once

#include "dec_search.h"

#define CN_MAX_MEMBERS 4

// What the ensemble step reads beside SsArgs (whose `logits` is unused here), passed by value.
struct EsArgs {
  const float* logits[CN_MAX_MEMBERS];  // (R, ldv) per member, never written by the step
  const int* bos[CN_MAX_MEMBERS];       // (B) per member: the token at position 0 of every row of the clip
  float w[CN_MAX_MEMBERS];              // weights, normalised to sum 1 by the host
  float logw[CN_MAX_MEMBERS];           // their logarithms (rule 1)
  float* comb;                          // (R, ldv): the generic kernel's combined scores
  int M, rule;
};

// (selects on a wave-uniform index: a by-value array indexed at run time would go through scratch memory)
__device__ __forceinline__ const float* es_logits(const EsArgs& e, int m) {
  return m == 0 ? e.logits[0] : (m == 1 ? e.logits[1] : (m == 2 ? e.logits[2] : e.logits[3]));
}
__device__ __forceinline__ float es_w(const EsArgs& e, int m) { return m == 0 ? e.w[0] : (m == 1 ? e.w[1] : (m == 2 ? e.w[2] : e.w[3])); }
__device__ __forceinline__ float es_logw(const EsArgs& e, int m) {
  return m == 0 ? e.logw[0] : (m == 1 ? e.logw[1] : (m == 2 ? e.logw[2] : e.logw[3]));
}

// acc (+)= member's term.  Rule 0: acc + w * lp; rule 1: log(exp(acc) + exp(lp + log w)) around the larger of the two.
__device__ __forceinline__ float es_first(float lp, int rule, float w, float logw) { return rule == 0 ? w * lp : lp + logw; }
__device__ __forceinline__ float es_add(float acc, float lp, int rule, float w, float logw) {
  if (rule == 0) return acc + w * lp;
  const float x = lp + logw;
  const float hi = fmaxf(acc, x), lo = fminf(acc, x);
  return hi == -INFINITY ? -INFINITY : hi + __logf(1.0f + __expf(lo - hi));  // (log of a number in [1, 2]: 1e-7 absolute)
}

// cn_mask_registers with `tok0` at position 0 of the prefix (a member's own task token); bit sl of `fbm` = the thread's token of slab sl
// is forbidden to repeat (one register in place of VPT flags: the kernel is at the register limit of a 1024-thread block)
template <int THREADS, int VPT>
__device__ __forceinline__ void cn_ens_mask_registers(float (&val)[VPT], unsigned fbm, const int* s_prefix, int tok0, int step, int min_pred,
                                                      int eos_id, int tid, int wv) {
  static_assert(THREADS == 1024, "a token's slab is tok >> 10");
  for (int j = 0; j <= step; ++j) {
    const int tok = j == 0 ? tok0 : s_prefix[j];
    if ((((unsigned)tok & (THREADS - 1)) >> 6) == (unsigned)wv) {
      if ((tok & (THREADS - 1)) == tid && ((fbm >> (tok >> 10)) & 1u)) {
#pragma unroll
        for (int sl = 0; sl < VPT; ++sl) val[sl] = sl == (tok >> 10) ? -INFINITY : val[sl];
      }
    }
  }
  if (step < min_pred && (eos_id & (THREADS - 1)) == tid) {
#pragma unroll
    for (int sl = 0; sl < VPT; ++sl) val[sl] = sl == (eos_id >> 10) ? -INFINITY : val[sl];
  }
}
// cn_masked_logit with `tok0` at position 0 of the prefix
__device__ __forceinline__ float cn_ens_masked_logit(const float* lg, int v, int step, int min_pred, int eos_id, const uint8_t* forbid,
                                                     const int* s_prefix, int tok0) {
  float x = lg[v];
  if (step < min_pred && v == eos_id) x = -INFINITY;
  if (forbid != nullptr && forbid[v] != 0) {
    bool seen = tok0 == v;
    for (int j = 1; j <= step; ++j) seen |= s_prefix[j] == v;
    if (seen) x = -INFINITY;
  }
  return x;
}

// Register-resident step: cn_search_step3_kernel with the members streamed through val.
template <int NR, int VPT>
__global__ __launch_bounds__(S3_T) void cn_ens_step3_kernel(const SsArgs a, const EsArgs e, const int step) {
  __shared__ float s_redm[NR][16], s_reds[NR][16];
  __shared__ float s_mx[CN_MAX_MEMBERS][NR], s_lg[CN_MAX_MEMBERS][NR];
  __shared__ float s_ru[16];
  __shared__ ValIdx s_cand[16][CN_MAX_BEAM];
  __shared__ float s_base[CN_MAX_BEAM];
  __shared__ float s_selv[CN_MAX_BEAM];
  __shared__ int s_self[CN_MAX_BEAM];
  __shared__ int s_prefix[CN_MAX_BEAM][CN_MAX_PRED + 1];
  __shared__ int s_anc[CN_MAX_BEAM][CN_MAX_PRED];
  __shared__ int s_slot[CN_MAX_BEAM];
  __shared__ int s_newpos[CN_MAX_BEAM];
  __shared__ int s_bos[CN_MAX_MEMBERS];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int ldv = a.ldv, V = a.V, beam = a.beam, maxp = a.maxp, M = e.M, rule = e.rule;
  const int rb = b * beam;
  // every global read that does not depend on another is issued up front (as cn_search_step3_kernel): the state, the masks and
  // member 0's logits; the later members' logits are read when the array is free again
  const int k_ld = a.n_active[b];
  const int rows_ld = step == 0 ? 1 : beam;
  float val[NR][VPT];
  unsigned fbm = 0;
#pragma unroll
  for (int sl = 0; sl < VPT; ++sl) {
    const int v = sl * S3_T + tid;
    if (a.forbid != nullptr && v < V && a.forbid[v] != 0) fbm |= 1u << sl;
  }
#pragma unroll
  for (int p = 0; p < NR; ++p) {
    const float* row = e.logits[0] + (size_t)(rb + p) * ldv;  // (a scalar base and a 32-bit lane offset)
#pragma unroll
    for (int sl = 0; sl < VPT; ++sl) {
      const int v = sl * S3_T + tid;
      val[p][sl] = (p < rows_ld && v < V) ? row[v] : -INFINITY;
    }
  }
  for (int i = tid; i < beam * (maxp + 1); i += S3_T) s_prefix[i / (maxp + 1)][i % (maxp + 1)] = a.prefix[(size_t)rb * (maxp + 1) + i];
  for (int i = tid; i < beam * maxp; i += S3_T) s_anc[i / maxp][i % maxp] = a.anc[(size_t)rb * maxp + i];
  if (tid < beam) {
    s_slot[tid] = a.slot[rb + tid];
    s_base[tid] = step == 0 ? 0.f : a.sum_lp[rb + tid];
  }
  if (tid < CN_MAX_MEMBERS) s_bos[tid] = tid < M ? (tid == 0 ? e.bos[0] : (tid == 1 ? e.bos[1] : (tid == 2 ? e.bos[2] : e.bos[3])))[b] : 0;
  const int k = k_ld;
  if (k == 0) return;
  const int nrows = step == 0 ? 1 : k;
  __syncthreads();
  // pass 1, per member: masks and log-softmax statistics of every live row (the expressions and the summation order of
  // cn_search_step3_kernel); the last member's masked logits stay in the registers
#pragma unroll 1
  for (int m = 0; m < M; ++m) {
    float rmx[NR];
    if (m > 0) {
      const float* lg = es_logits(e, m);
#pragma unroll
      for (int p = 0; p < NR; ++p) {
        const float* row = lg + (size_t)(rb + p) * ldv;
#pragma unroll
        for (int sl = 0; sl < VPT; ++sl) {
          const int v = sl * S3_T + tid;
          val[p][sl] = (p < rows_ld && v < V) ? row[v] : -INFINITY;
        }
      }
    }
    const int tok0 = s_bos[m];
#pragma unroll
    for (int p = 0; p < NR; ++p)
      if (p < nrows) cn_ens_mask_registers<S3_T>(val[p], fbm, s_prefix[p], tok0, step, a.min_pred, a.eos_id, tid, wv);
#pragma unroll
    for (int p = 0; p < NR; ++p)
      if (p < nrows) {
        float mx = val[p][0];
#pragma unroll
        for (int sl = 1; sl < VPT; ++sl) mx = fmaxf(mx, val[p][sl]);
        mx = cn_wave_max_dpp(mx);
        if (lane == 0) s_redm[p][wv] = mx;
      }
    __syncthreads();
#pragma unroll
    for (int p = 0; p < NR; ++p)
      if (p < nrows) {
        float mx = s_redm[p][0];
#pragma unroll
        for (int w = 1; w < 16; ++w) mx = fmaxf(mx, s_redm[p][w]);
        rmx[p] = mx;
        float sm = 0.f;
#pragma unroll
        for (int sl = 0; sl < VPT; ++sl) sm += __expf(val[p][sl] - mx);
        sm = cn_wave_sum_dpp(sm);
        if (lane == 0) s_reds[p][wv] = sm;
      }
    __syncthreads();
#pragma unroll
    for (int p = 0; p < NR; ++p)
      if (p < nrows) {
        float sm = s_reds[p][0];
#pragma unroll
        for (int w = 1; w < 16; ++w) sm += s_reds[p][w];
        if (tid == 0) {
          s_mx[m][p] = rmx[p];
          s_lg[m][p] = logf(sm);
        }
      }
  }
  __syncthreads();  // s_mx / s_lg of every member
  // the last member's log-probabilities, in place; with more members its term of the combination
#pragma unroll
  for (int p = 0; p < NR; ++p)
    if (p < nrows) {
      const float mx = s_mx[M - 1][p], lgs = s_lg[M - 1][p];
#pragma unroll
      for (int sl = 0; sl < VPT; ++sl) val[p][sl] = (val[p][sl] - mx) - lgs;
    }
  if (M > 1) {
    {
      const float w = es_w(e, M - 1), logw = es_logw(e, M - 1);
#pragma unroll
      for (int p = 0; p < NR; ++p)
        if (p < nrows) {
#pragma unroll
          for (int sl = 0; sl < VPT; ++sl) val[p][sl] = es_first(val[p][sl], rule, w, logw);
        }
    }
    // pass 2: the other members' terms, a row at a time
#pragma unroll 1
    for (int m = 0; m < M - 1; ++m) {
      const float* lg = es_logits(e, m);
      const float w = es_w(e, m), logw = es_logw(e, m);
      const int tok0 = s_bos[m];
#pragma unroll
      for (int p = 0; p < NR; ++p)
        if (p < nrows) {
          const float* row = lg + (size_t)(rb + p) * ldv;
          float x[VPT];
#pragma unroll
          for (int sl = 0; sl < VPT; ++sl) {
            const int v = sl * S3_T + tid;
            x[sl] = v < V ? row[v] : -INFINITY;
          }
          cn_ens_mask_registers<S3_T>(x, fbm, s_prefix[p], tok0, step, a.min_pred, a.eos_id, tid, wv);
          const float mx = s_mx[m][p], lgs = s_lg[m][p];
#pragma unroll
          for (int sl = 0; sl < VPT; ++sl) val[p][sl] = es_add(val[p][sl], (x[sl] - mx) - lgs, rule, w, logw);
        }
    }
  }
  // per-thread sorted top-k (strict > keeps the earlier = lower flat index first on ties)
  float bv[NR];
  int bi[NR];
#pragma unroll
  for (int j = 0; j < NR; ++j) {
    bv[j] = -INFINITY;
    bi[j] = 0x7fffffff;
  }
#pragma unroll
  for (int p = 0; p < NR; ++p)
    if (p < nrows) {
      const float base = s_base[p];
#pragma unroll
      for (int sl = 0; sl < VPT; ++sl) {
        const int v = sl * S3_T + tid;
        float cand = val[p][sl];
        if (step != 0) cand = base + cand;
        if (v < V && cand > bv[NR - 1]) {
          bv[NR - 1] = cand;
          bi[NR - 1] = p * V + v;
#pragma unroll
          for (int j = NR - 1; j > 0; --j) {
            if (bv[j] > bv[j - 1]) {
              const float tv = bv[j];
              bv[j] = bv[j - 1];
              bv[j - 1] = tv;
              const int ti = bi[j];
              bi[j] = bi[j - 1];
              bi[j - 1] = ti;
            }
          }
        }
      }
    }
  // level 1: the wave's k best
  {
    int head = 0;
#pragma unroll
    for (int c = 0; c < NR; ++c)
      if (c < k) {
        ValIdx mine{-INFINITY, 0x7fffffff};
#pragma unroll
        for (int j = 0; j < NR; ++j)
          if (head == j) mine = ValIdx{bv[j], bi[j]};
        const ValIdx best = vi_wave_dpp(mine);
        if (mine.i == best.i && mine.i != 0x7fffffff) ++head;
        if (lane == 0) s_cand[wv][c] = best;
      }
  }
  __syncthreads();
  // level 2: merge the 16 x k wave winners (every wave computes the same result)
  {
    const int nc = 16 * k;  // <= 128: two entries per lane
    ValIdx t0{-INFINITY, 0x7fffffff}, t1{-INFINITY, 0x7fffffff};
    if (lane < nc) t0 = s_cand[lane / k][lane % k];
    if (lane + 64 < nc) t1 = s_cand[(lane + 64) / k][(lane + 64) % k];
#pragma unroll
    for (int c = 0; c < NR; ++c)
      if (c < k) {
        const ValIdx best = vi_wave_dpp(vi_better(t0, t1));
        if (best.i != 0x7fffffff) {
          if (t0.i == best.i) t0 = ValIdx{-INFINITY, 0x7fffffff};
          else if (t1.i == best.i) t1 = ValIdx{-INFINITY, 0x7fffffff};
        }
        if (tid == 0) {
          s_selv[c] = best.v;
          s_self[c] = best.i;
        }
      }
  }
  __syncthreads();
  if (a.margins != nullptr) {  // the first rejected candidate: the best of everything the k picks left (same expression, same bits)
    float ru = -INFINITY;
#pragma unroll
    for (int p = 0; p < NR; ++p)
      if (p < nrows) {
        const float base = s_base[p];
#pragma unroll
        for (int sl = 0; sl < VPT; ++sl) {
          const int v = sl * S3_T + tid;
          float cand = val[p][sl];
          if (step != 0) cand = base + cand;
          const int flat = p * V + v;
          bool taken = v >= V;
          for (int c = 0; c < k; ++c) taken |= (s_self[c] == flat);
          if (!taken) ru = fmaxf(ru, cand);
        }
      }
    ru = cn_wave_max_dpp(ru);
    if (lane == 0) s_ru[wv] = ru;
    __syncthreads();
    if (tid == 0) {
      ru = s_ru[0];
#pragma unroll
      for (int w = 1; w < 16; ++w) ru = fmaxf(ru, s_ru[w]);
      cn_step_margin(a.margins, b, maxp, step, s_selv, k, ru);
    }
  }
  cn_search_commit<S3_T>(a, b, k, step, s_selv, s_self, s_prefix, s_anc, s_slot, s_newpos);
}

// Generic step: any beam <= CN_MAX_BEAM and any V.  The statistics are cn_search_step_kernel's (expressions and summation order);
// with `reg_sums` the log-sum-exp is summed as cn_search_step3_kernel sums it (as dec_group.h's generic kernel does): the searches
// that conette_decode runs on its register kernel and this file runs here -- beams 5 .. 8 with 6144 < V <= 8192 -- keep its bits.
__global__ __launch_bounds__(256) void cn_ens_step_kernel(const SsArgs a, const EsArgs e, const int step, const int reg_sums) {
  __shared__ float s_red[8];
  __shared__ float s_reds[16];
  __shared__ ValIdx s_vi[4];
  __shared__ float s_mx[CN_MAX_MEMBERS][CN_MAX_BEAM], s_lg[CN_MAX_MEMBERS][CN_MAX_BEAM], s_base[CN_MAX_BEAM];
  __shared__ float s_selv[CN_MAX_BEAM + 1];
  __shared__ int s_self[CN_MAX_BEAM + 1];
  __shared__ int s_prefix[CN_MAX_BEAM][CN_MAX_PRED + 1];
  __shared__ int s_anc[CN_MAX_BEAM][CN_MAX_PRED];
  __shared__ int s_slot[CN_MAX_BEAM];
  __shared__ int s_newpos[CN_MAX_BEAM];
  __shared__ int s_bos[CN_MAX_MEMBERS];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int ldv = a.ldv, V = a.V, maxp = a.maxp, M = e.M, rule = e.rule;
  const int k = a.n_active[b];
  if (k == 0) return;
  const int rb = b * a.beam;
  const int nrows = step == 0 ? 1 : k;

  for (int i = tid; i < k * (maxp + 1); i += 256) s_prefix[i / (maxp + 1)][i % (maxp + 1)] = a.prefix[(size_t)rb * (maxp + 1) + i];
  for (int i = tid; i < k * maxp; i += 256) s_anc[i / maxp][i % maxp] = a.anc[(size_t)rb * maxp + i];
  if (tid < k) {
    s_slot[tid] = a.slot[rb + tid];
    s_base[tid] = step == 0 ? 0.f : a.sum_lp[rb + tid];
  }
  if (tid < CN_MAX_MEMBERS) s_bos[tid] = tid < M ? (tid == 0 ? e.bos[0] : (tid == 1 ? e.bos[1] : (tid == 2 ? e.bos[2] : e.bos[3])))[b] : 0;
  __syncthreads();
  // log-softmax statistics per member and row; the masks are applied to what is read, never to the members' arrays
  for (int m = 0; m < M; ++m) {
    const float* lgm = es_logits(e, m);
    const int tok0 = s_bos[m];
    for (int p = 0; p < nrows; ++p) {
      const float* lg = lgm + (size_t)(rb + p) * ldv;
      float mx = -INFINITY;
      for (int v = tid; v < V; v += 256) mx = fmaxf(mx, cn_ens_masked_logit(lg, v, step, a.min_pred, a.eos_id, a.forbid, s_prefix[p], tok0));
      mx = cn_wave_max(mx);
      if (lane == 0) s_red[wv] = mx;
      __syncthreads();
      mx = fmaxf(fmaxf(s_red[0], s_red[1]), fmaxf(s_red[2], s_red[3]));
      if (reg_sums) {
        // thread t of 1024 adds its logits t, t + 1024, .. in order, a wave adds its 64 threads by cn_wave_sum_dpp, the 16 wave sums
        // are added in sequence.  This thread plays threads tid + 256 j (waves wv + 4 j).
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          float sm = 0.f;
          for (int v = tid + 256 * j; v < V; v += S3_T)
            sm += __expf(cn_ens_masked_logit(lg, v, step, a.min_pred, a.eos_id, a.forbid, s_prefix[p], tok0) - mx);
          sm = cn_wave_sum_dpp(sm);
          if (lane == 0) s_reds[wv + 4 * j] = sm;
        }
        __syncthreads();
        if (tid == 0) {
          float sm = s_reds[0];
          for (int w = 1; w < 16; ++w) sm += s_reds[w];
          s_mx[m][p] = mx;
          s_lg[m][p] = logf(sm);
        }
      } else {
        float sm = 0.f;
        for (int v = tid; v < V; v += 256) sm += expf(cn_ens_masked_logit(lg, v, step, a.min_pred, a.eos_id, a.forbid, s_prefix[p], tok0) - mx);
        sm = cn_wave_sum(sm);
        if (lane == 0) s_red[4 + wv] = sm;
        __syncthreads();
        if (tid == 0) {
          s_mx[m][p] = mx;
          s_lg[m][p] = logf(s_red[4] + s_red[5] + s_red[6] + s_red[7]);
        }
      }
      __syncthreads();
    }
  }
  // the combined scores of the clip's candidate rows
  for (int p = 0; p < nrows; ++p) {
    float* out = e.comb + (size_t)(rb + p) * ldv;
    for (int v = tid; v < V; v += 256) {
      const int last = M - 1;
      float c = (cn_ens_masked_logit(es_logits(e, last) + (size_t)(rb + p) * ldv, v, step, a.min_pred, a.eos_id, a.forbid, s_prefix[p],
                                     s_bos[last]) - s_mx[last][p]) - s_lg[last][p];
      if (M > 1) {
        c = es_first(c, rule, es_w(e, last), es_logw(e, last));
        for (int m = 0; m < last; ++m) {
          const float lp = (cn_ens_masked_logit(es_logits(e, m) + (size_t)(rb + p) * ldv, v, step, a.min_pred, a.eos_id, a.forbid,
                                                s_prefix[p], s_bos[m]) - s_mx[m][p]) - s_lg[m][p];
          c = es_add(c, lp, rule, es_w(e, m), es_logw(e, m));
        }
      }
      out[v] = c;
    }
  }
  __syncthreads();
  // top-k over the nrows * V candidates, k rounds of block arg-max (ties -> lowest flat index); with a margin output one
  // more round finds the first rejected candidate
  for (int c = 0; c < k + (a.margins != nullptr ? 1 : 0); ++c) {
    ValIdx best{-INFINITY, 0x7fffffff};
    for (int p = 0; p < nrows; ++p) {
      const float* cb = e.comb + (size_t)(rb + p) * ldv;
      const float base = s_base[p];
      for (int v = tid; v < V; v += 256) {
        const int flat = p * V + v;
        bool taken = false;
        for (int d = 0; d < c; ++d) taken |= (s_self[d] == flat);
        if (taken) continue;
        float cand = cb[v];
        if (step != 0) cand = base + cand;
        best = vi_better(best, ValIdx{cand, flat});
      }
    }
    best = vi_wave(best);
    if (lane == 0) s_vi[wv] = best;
    __syncthreads();
    if (tid == 0) {
      ValIdx r0 = vi_better(vi_better(s_vi[0], s_vi[1]), vi_better(s_vi[2], s_vi[3]));
      s_selv[c] = r0.v;
      s_self[c] = r0.i;
    }
    __syncthreads();
  }
  if (a.margins != nullptr && tid == 0) cn_step_margin(a.margins, b, maxp, step, s_selv, k, s_selv[k]);
  cn_search_commit<256>(a, b, k, step, s_selv, s_self, s_prefix, s_anc, s_slot, s_newpos);
}

// The step launch of the ensemble loop: the kernel choice of the plain search (decode_impl) and its instantiations, but for
// <NR 8, VPT 8>, which does not fit the 128 registers of a 1024-thread block beside the streamed member (26 registers would go to
// scratch memory; <8, 7> still 5).  Beams 5 .. 8 run <8, 6> up to 6144 tokens -- bit for bit the plain <8, 8>: the two slabs it
// lacks hold -inf there and add +0 to a sum -- and the generic kernel, with the register kernel's sums, above.
static inline void cn_ens_step_launch(const SsArgs& ss, const EsArgs& es, int B, int step, hipStream_t s) {
  const bool plain_in_registers = ss.V <= S3_T * S3_VPT && ss.beam <= 8;  // conette_decode's own choice
  const int vpt = cn_cdiv(ss.V, S3_T);
  if (plain_in_registers && (ss.beam <= 4 || vpt <= 6)) {
#define ES_LAUNCH(NR_, VPT_) hipLaunchKernelGGL((cn_ens_step3_kernel<NR_, VPT_>), dim3(B), dim3(S3_T), 0, s, ss, es, step)
    if (ss.beam <= 4) {
      if (vpt <= 2) ES_LAUNCH(4, 2);
      else if (vpt <= 4) ES_LAUNCH(4, 4);
      else if (vpt <= 6) ES_LAUNCH(4, 6);
      else ES_LAUNCH(4, 8);
    } else {
      if (vpt <= 4) ES_LAUNCH(8, 4);
      else ES_LAUNCH(8, 6);
    }
#undef ES_LAUNCH
  } else {
    hipLaunchKernelGGL(cn_ens_step_kernel, dim3(B), dim3(256), 0, s, ss, es, step, plain_in_registers ? 1 : 0);
  }
}
