// Keyword-guided beam search (conette_decode_required, include/conette_hip.h; the CPU restatement of the rule is
// conette_amd/required_search.py): the constrained search's step (dec_constrain.h) for a clip whose every caption must hold a token
// of each of G <= 8 groups of tokens -- dynamic beam allocation.
//
// A row's requirement state is derived from its own sequence: group g is MET when one of its tokens occurs among s_1 .. s_i,
// c(p) = met groups of row p.  After the constrained search's masks, on every call of a row (forced calls included):
//   M4  while a group is unmet, z[eos] = -inf;
//   M5  if unmet(p) >= max_pred - i, z[v] = -inf for every v that is no token of one of the row's unmet groups.
// Candidate (p, v) is in bank c(p) + 1 if v belongs to an unmet group of row p, else in bank c(p).  Per bank the candidates are
// ordered by descending finite model score, ties to the lowest flat index; the k slots are dealt round-robin from the highest
// non-empty bank to the lowest, skipping exhausted banks, until k picks or until no finite candidate is left.  Pick order is deal
// order; the missing picks are CN_NO_PICK behind the others and cn_constrain_commit, unchanged, turns them into void slots.
//
// Structure of a step, both kernels: the clip's (token, group) table, at most 32 entries, is staged in LDS (an entry with a group
// outside 0 .. 7, a token outside the vocabulary or a token an earlier entry holds counts as unused; the register kernel also
// notes per thread which entries are tokens of its registers, so that no thread walks the table); one thread per (row,
// position) ORs the row's met bits; M4 / M5 are wave-uniform per row and go onto the logits beside the ban mask; the log-softmax
// statistics are the constrained kernel's, expression for expression; then the scores of the tokens of a row's unmet groups are
// moved out of the logits into LDS (k x 32 floats), so that the ordinary top-k, which runs once per distinct c(p) among the live
// rows as a filter on rows, never sees them; wave 0 merges each bank's ordinary list with its moved-out candidates and lane 0
// deals the slots.  A clip none of whose rows has an unmet group left takes its one bank's list as it is: the constrained step.
#pragma once

#include "dec_constrain.h"

#define RQ_MAX_TOKENS 32
#define RQ_MAX_GROUPS 8
#define RQ_BANKS (RQ_MAX_GROUPS + 1)

struct RqArgs {
  const int* tokens;  // (B, width)
  const int* groups;  // (B, width): 0 .. 7, -1 = unused entry
  int width;          // 1 .. RQ_MAX_TOKENS (width 0 runs the constrained step)
};

// Entry e of clip b's table into LDS, by thread e < RQ_MAX_TOKENS: the token, and the group or -1 for an entry out of range.
__device__ __forceinline__ void rq_stage(const RqArgs& ra, int b, int V, int e, int* s_rt, int* s_rg0) {
  int tok = 0, g = -1;
  if (e < ra.width) {
    tok = ra.tokens[(size_t)b * ra.width + e];
    g = ra.groups[(size_t)b * ra.width + e];
    if (g < 0 || g >= RQ_MAX_GROUPS || tok < 0 || tok >= V) g = -1;
  }
  s_rt[e] = tok;
  s_rg0[e] = g;
}
// After a barrier, by thread e < RQ_MAX_TOKENS: the entry's final group -- -1 too where an earlier entry holds its token.
__device__ __forceinline__ int rq_dedupe(int e, const int* s_rt, const int* s_rg0) {
  int g = s_rg0[e];
  for (int q = 0; q < e; ++q)
    if (s_rg0[q] >= 0 && s_rt[q] == s_rt[e]) g = -1;
  return g;
}

// The met bits of the rows' sequences s_1 .. s_step (one thread per (row, position)) and the clip's group mask, by atomic OR.
template <int THREADS>
__device__ __forceinline__ void rq_find_met(const int (*s_prefix)[CN_MAX_PRED + 1], int nrows, int step, const int* s_rt, const int* s_rg,
                                            unsigned* s_met, unsigned* s_gmask) {
  const int tid = threadIdx.x;
  for (int i = tid; i < nrows * step; i += THREADS) {
    const int p = i / step, tok = s_prefix[p][1 + i % step];
    unsigned bits = 0;
    for (int e = 0; e < RQ_MAX_TOKENS; ++e) bits |= (s_rg[e] >= 0 && s_rt[e] == tok) ? (1u << s_rg[e]) : 0u;
    if (bits) atomicOr(&s_met[p], bits);
  }
  if (tid < RQ_MAX_TOKENS && s_rg[tid] >= 0) atomicOr(s_gmask, 1u << s_rg[tid]);
}

// The deal, by wave 0 (all 64 lanes).  s_ord[c]: the ordinary top-k list of the rows with c(p) == c (sorted, CN_NO_PICK from its
// end on), for every c of cmask; s_rq[p][e]: the model score of entry e's token as a candidate of row p, -inf unless the entry's
// group is unmet in row p and the score finite (its bank is s_c[p] + 1).  Leaves the picks in s_selv / s_self.
template <int MAXR>
__device__ __forceinline__ void rq_deal(int k, int nrows, int V, unsigned cmask, const int* s_c, const ValIdx (*s_ord)[MAXR],
                                        float (*s_rq)[RQ_MAX_TOKENS], const int* s_rt, ValIdx (*s_fin)[MAXR], int* s_nfin,
                                        float* s_selv, int* s_self) {
  const int lane = threadIdx.x & 63;
  for (int j = RQ_MAX_GROUPS; j >= 0; --j) {  // the bank's own order: its ordinary list merged with its moved-out candidates
    const bool has_ord = (cmask >> j) & 1u;
    const bool has_req = j > 0 && ((cmask >> (j - 1)) & 1u);
    int nf = 0;
    if (has_ord || has_req) {
      int head = 0;
      for (int r = 0; r < k; ++r) {
        ValIdx best{-INFINITY, CN_NO_PICK};
        if (has_req)
          for (int i = lane; i < nrows * RQ_MAX_TOKENS; i += 64) {
            const int p = i / RQ_MAX_TOKENS, e = i % RQ_MAX_TOKENS;
            const float m = s_rq[p][e];
            if (s_c[p] == j - 1 && m > -INFINITY) best = vi_better(best, ValIdx{m, p * V + s_rt[e]});
          }
        best = vi_wave(best);
        ValIdx o{-INFINITY, CN_NO_PICK};
        if (has_ord && head < k) o = s_ord[j][head];
        const ValIdx win = vi_better(best, o);
        if (win.i == CN_NO_PICK) break;  // (wave-uniform: the bank is exhausted)
        if (win.i == o.i) {
          ++head;
        } else {  // the lane that holds the winner takes it out
          for (int i = lane; i < nrows * RQ_MAX_TOKENS; i += 64) {
            const int p = i / RQ_MAX_TOKENS, e = i % RQ_MAX_TOKENS;
            if (s_c[p] == j - 1 && s_rq[p][e] > -INFINITY && p * V + s_rt[e] == win.i) s_rq[p][e] = -INFINITY;
          }
        }
        if (lane == 0) s_fin[j][nf] = win;
        ++nf;
      }
    }
    if (lane == 0) s_nfin[j] = nf;
  }
  if (lane == 0) {  // round r takes every bank's pick r, highest bank first
    int n = 0;
    for (int r = 0; r < k && n < k; ++r)
      for (int j = RQ_MAX_GROUPS; j >= 0 && n < k; --j)
        if (r < s_nfin[j]) {
          s_selv[n] = s_fin[j][r].v;
          s_self[n] = s_fin[j][r].i;
          ++n;
        }
    for (; n < k; ++n) {
      s_selv[n] = -INFINITY;
      s_self[n] = CN_NO_PICK;
    }
  }
}

// Register-resident step: the layout, the masks and the statistics of cn_constrain_step3_kernel.
template <int NR, int VPT>
__global__ __launch_bounds__(S3_T) void cn_require_step3_kernel(const SsArgs a, const CsArgs ca, const RqArgs ra, const int step) {
  __shared__ float s_redm[NR][16], s_reds[NR][16];
  __shared__ ValIdx s_cand[16][NR];
  __shared__ float s_base[NR];
  __shared__ float s_selv[NR];
  __shared__ int s_self[NR];
  __shared__ int s_prefix[NR][CN_MAX_PRED + 1];
  __shared__ int s_anc[NR][CN_MAX_PRED];
  __shared__ int s_ng[NR][CN_MAX_PRED];
  __shared__ int s_slot[NR];
  __shared__ int s_newpos[NR];
  __shared__ int s_rt[RQ_MAX_TOKENS], s_rg0[RQ_MAX_TOKENS], s_rg[RQ_MAX_TOKENS];
  __shared__ unsigned s_own[S3_T];  // bit e: table entry e is a token of this thread's (tok & 1023 == tid)
  __shared__ unsigned s_met[NR], s_gmask;
  __shared__ int s_c[NR];
  __shared__ float s_rq[NR][RQ_MAX_TOKENS];
  __shared__ ValIdx s_ord[RQ_BANKS][NR], s_fin[RQ_BANKS][NR];
  __shared__ int s_nfin[RQ_BANKS];
  __shared__ float s_rmx[NR], s_rlg[NR];  // the rows' statistics: in LDS, the registers go to the bank loop
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int ldv = a.ldv, V = a.V, beam = a.beam, maxp = a.maxp, n = ca.ngram;
  const int rb = b * beam;
  // every global read is issued up front and none depends on another (as cn_search_step3_kernel)
  const int k = a.n_active[b];
  const int plen = cn_prefix_len(ca, b);
  const int ftok = cn_prefix_tok(ca, b, step);
  float val[NR][VPT];
  bool fb[VPT];
  unsigned bb = 0;  // bit sl: this thread's token of slab sl is in the ban mask
#pragma unroll
  for (int sl = 0; sl < VPT; ++sl) {
    const int v = sl * S3_T + tid;
    fb[sl] = a.forbid != nullptr && v < V && a.forbid[v] != 0;
    bb |= (ca.ban != nullptr && v < V && ca.ban[v] != 0) ? (1u << sl) : 0u;
  }
#pragma unroll
  for (int p = 0; p < NR; ++p)
#pragma unroll
    for (int sl = 0; sl < VPT; ++sl) {
      const int v = sl * S3_T + tid;
      val[p][sl] = (p < beam && v < V) ? a.logits[(size_t)(rb + p) * ldv + v] : -INFINITY;
    }
  for (int i = tid; i < beam * (maxp + 1); i += S3_T) s_prefix[i / (maxp + 1)][i % (maxp + 1)] = a.prefix[(size_t)rb * (maxp + 1) + i];
  for (int i = tid; i < beam * maxp; i += S3_T) s_anc[i / maxp][i % maxp] = a.anc[(size_t)rb * maxp + i];
  if (tid < beam) {
    s_slot[tid] = a.slot[rb + tid];
    s_base[tid] = step == 0 ? 0.f : a.sum_lp[rb + tid];
  }
  if (tid == 0) s_self[0] = CN_NO_PICK;  // (a forced call: until the token's owner finds its score finite)
  if (tid < RQ_MAX_TOKENS) rq_stage(ra, b, V, tid, s_rt, s_rg0);
  s_own[tid] = 0u;
  if (tid >= 64 && tid < 64 + NR) s_met[tid - 64] = 0u;
  if (tid == 128) s_gmask = 0u;
  if (tid < NR * RQ_MAX_TOKENS) s_rq[tid / RQ_MAX_TOKENS][tid % RQ_MAX_TOKENS] = -INFINITY;
  if (k == 0) return;
  const bool forced = step < plen;
  const int nrows = step <= plen ? 1 : k;
  if (ca.step_logits) {  // the RAW logits this step's decisions see
    float* o = ca.step_logits + ((size_t)step * gridDim.x * beam + rb) * V;
#pragma unroll
    for (int p = 0; p < NR; ++p)
      if (p < beam) {
#pragma unroll
        for (int sl = 0; sl < VPT; ++sl)
          if (sl * S3_T + tid < V) o[(size_t)p * V + sl * S3_T + tid] = val[p][sl];
      }
  }
  __syncthreads();
  if (tid < RQ_MAX_TOKENS) {
    const int g = rq_dedupe(tid, s_rt, s_rg0);
    s_rg[tid] = g;
    if (g >= 0) atomicOr(&s_own[s_rt[tid] & (S3_T - 1)], 1u << tid);
  }
  __syncthreads();
  const unsigned own = s_own[tid];
  rq_find_met<S3_T>(s_prefix, nrows, step, s_rt, s_rg, s_met, &s_gmask);
  // the plain search's masks, then the ban mask, on the owner's registers
#pragma unroll
  for (int p = 0; p < NR; ++p)
    if (p < nrows) {
      cn_mask_registers<S3_T>(val[p], fb, s_prefix[p], step, a.min_pred, a.eos_id, tid, wv);
#pragma unroll
      for (int sl = 0; sl < VPT; ++sl) val[p][sl] = ((bb >> sl) & 1u) ? -INFINITY : val[p][sl];
    }
  if (n > 0) {  // the n-gram rule: one thread per (row, start position) finds the token, its owner masks it
    const int starts = max(step - n + 2, 0);
    for (int i = tid; i < nrows * CN_MAX_PRED; i += S3_T) {
      const int p = i / CN_MAX_PRED, j = i % CN_MAX_PRED;
      s_ng[p][j] = j < starts ? cn_ngram_banned(s_prefix[p], step, n, j) : -1;
    }
    __syncthreads();
#pragma unroll
    for (int p = 0; p < NR; ++p)
      if (p < nrows) cn_ban_registers<S3_T>(val[p], s_ng[p], starts, tid, wv);
  }
  __syncthreads();  // the met bits are complete
  const unsigned gmask = s_gmask;
  unsigned cmask = 0;  // bit c: a candidate row has c met groups
  bool open = false;   // a candidate row has an unmet group
  for (int p = 0; p < nrows; ++p) {
    cmask |= 1u << __popc(s_met[p] & gmask);
    open |= (gmask & ~s_met[p]) != 0u;
  }
  if (tid < nrows) s_c[tid] = __popc(s_met[tid] & gmask);
  if (open) {  // M4 and M5, wave-uniform per row
#pragma unroll
    for (int p = 0; p < NR; ++p)
      if (p < nrows) {
        const unsigned left = gmask & ~s_met[p];
        if (left != 0u) {
          if ((a.eos_id & (S3_T - 1)) == tid) {
#pragma unroll
            for (int sl = 0; sl < VPT; ++sl) val[p][sl] = sl == (a.eos_id >> 10) ? -INFINITY : val[p][sl];
          }
          if (__popc(left) >= maxp - step) {  // only the tokens of the unmet groups stay
            unsigned keep = 0;
            for (unsigned m = own; m != 0u; m &= m - 1u) {
              const int e = __ffs((int)m) - 1;
              if ((left >> s_rg[e]) & 1u) keep |= 1u << (s_rt[e] >> 10);
            }
#pragma unroll
            for (int sl = 0; sl < VPT; ++sl) val[p][sl] = ((keep >> sl) & 1u) ? val[p][sl] : -INFINITY;
          }
        }
      }
  }
  // log-softmax statistics of every candidate row (the expressions and the summation order of cn_search_step3_kernel)
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
      if (tid == 0) s_rmx[p] = mx;
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
      if (tid == 0) s_rlg[p] = logf(sm);
    }
  __syncthreads();
  if (forced) {  // no top-k: the owner of the token forms its model score
    if (ftok >= 0 && ftok < V && ftok != a.eos_id && (ftok & (S3_T - 1)) == tid) {
      float z = -INFINITY;
#pragma unroll
      for (int sl = 0; sl < VPT; ++sl) z = sl == (ftok >> 10) ? val[0][sl] : z;
      float m = (z - s_rmx[0]) - s_rlg[0];
      if (step != 0) m = s_base[0] + m;
      if (m > -INFINITY && m < INFINITY) {
        s_selv[0] = m;
        s_self[0] = ftok;
      }
    }
    __syncthreads();
    cn_constrain_commit<S3_T>(a, b, k, step, true, s_selv, s_self, s_prefix, s_anc, s_slot, s_newpos);
    return;
  }
  if (open) {  // the candidates of the unmet groups leave the registers for LDS: the owner forms their model score
#pragma unroll
    for (int p = 0; p < NR; ++p)
      if (p < nrows) {
        const unsigned left = gmask & ~s_met[p];
        if (left != 0u) {
          const float base = s_base[p];
          for (unsigned m = own; m != 0u; m &= m - 1u) {
            const int e = __ffs((int)m) - 1, tok = s_rt[e];
            if ((left >> s_rg[e]) & 1u) {
              float z = -INFINITY;
#pragma unroll
              for (int sl = 0; sl < VPT; ++sl) z = sl == (tok >> 10) ? val[p][sl] : z;
              float cand = (z - s_rmx[p]) - s_rlg[p];
              if (step != 0) cand = base + cand;
              s_rq[p][e] = (cand > -INFINITY && cand < INFINITY) ? cand : -INFINITY;
#pragma unroll
              for (int sl = 0; sl < VPT; ++sl) val[p][sl] = sl == (tok >> 10) ? -INFINITY : val[p][sl];
            }
          }
        }
      }
  }
  // the logits have served: the registers now hold the model scores (the constrained kernel's expression), so that the bank
  // loop reads no statistics
#pragma unroll
  for (int p = 0; p < NR; ++p)
    if (p < nrows) {
      const float base = s_base[p], mx = s_rmx[p], lg = s_rlg[p];
#pragma unroll
      for (int sl = 0; sl < VPT; ++sl) {
        float cand = (val[p][sl] - mx) - lg;
        if (step != 0) cand = base + cand;
        val[p][sl] = cand;
      }
    }
  // the ordinary top-k, once per distinct c(p): the constrained kernel's, over the rows with that c
  for (int c = RQ_MAX_GROUPS; c >= 0; --c) {
    if (!((cmask >> c) & 1u)) continue;
    // per-thread sorted top-k (strict > keeps the earlier = lower flat index first on ties; -inf and NaN never enter)
    float bv[NR];
    int bi[NR];
#pragma unroll
    for (int j = 0; j < NR; ++j) {
      bv[j] = -INFINITY;
      bi[j] = CN_NO_PICK;
    }
#pragma unroll
    for (int p = 0; p < NR; ++p)
      if (p < nrows && s_c[p] == c) {
#pragma unroll
        for (int sl = 0; sl < VPT; ++sl) {
          const int v = sl * S3_T + tid;
          const float cand = val[p][sl];
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
      for (int r = 0; r < NR; ++r)
        if (r < k) {
          ValIdx mine{-INFINITY, CN_NO_PICK};
#pragma unroll
          for (int j = 0; j < NR; ++j)
            if (head == j) mine = ValIdx{bv[j], bi[j]};
          const ValIdx best = vi_wave_dpp(mine);
          if (mine.i == best.i && mine.i != CN_NO_PICK) ++head;
          if (lane == 0) s_cand[wv][r] = best;
        }
    }
    __syncthreads();
    // level 2: merge the 16 x k wave winners (every wave computes the same result)
    {
      const int nc = 16 * k;  // <= 128: two entries per lane
      ValIdx t0{-INFINITY, CN_NO_PICK}, t1{-INFINITY, CN_NO_PICK};
      if (lane < nc) t0 = s_cand[lane / k][lane % k];
      if (lane + 64 < nc) t1 = s_cand[(lane + 64) / k][(lane + 64) % k];
#pragma unroll
      for (int r = 0; r < NR; ++r)
        if (r < k) {
          const ValIdx best = vi_wave_dpp(vi_better(t0, t1));
          if (best.i != CN_NO_PICK) {
            if (t0.i == best.i) t0 = ValIdx{-INFINITY, CN_NO_PICK};
            else if (t1.i == best.i) t1 = ValIdx{-INFINITY, CN_NO_PICK};
          }
          if (tid == 0) s_ord[c][r] = best;
        }
    }
    __syncthreads();
  }
  if (!open) {  // one bank, nothing moved out: its list is the call's picks
    const int c0 = 31 - __clz((int)cmask);
    if (tid < k) {
      s_selv[tid] = s_ord[c0][tid].v;
      s_self[tid] = s_ord[c0][tid].i;
    }
  } else if (wv == 0) {
    rq_deal<NR>(k, nrows, V, cmask, s_c, s_ord, s_rq, s_rt, s_fin, s_nfin, s_selv, s_self);
  }
  __syncthreads();
  cn_constrain_commit<S3_T>(a, b, k, step, false, s_selv, s_self, s_prefix, s_anc, s_slot, s_newpos);
}

// Generic step: any W <= CN_MAX_BEAM and any V (the layout, the masks and the sums of cn_constrain_step_kernel).
__global__ __launch_bounds__(256) void cn_require_step_kernel(const SsArgs a, const CsArgs ca, const RqArgs ra, const int step) {
  __shared__ float s_red[8];
  __shared__ ValIdx s_vi[4];
  __shared__ float s_mx[CN_MAX_BEAM], s_lg[CN_MAX_BEAM], s_base[CN_MAX_BEAM];
  __shared__ float s_selv[CN_MAX_BEAM];
  __shared__ int s_self[CN_MAX_BEAM];
  __shared__ int s_prefix[CN_MAX_BEAM][CN_MAX_PRED + 1];
  __shared__ int s_anc[CN_MAX_BEAM][CN_MAX_PRED];
  __shared__ int s_slot[CN_MAX_BEAM];
  __shared__ int s_newpos[CN_MAX_BEAM];
  __shared__ int s_rt[RQ_MAX_TOKENS], s_rg0[RQ_MAX_TOKENS], s_rg[RQ_MAX_TOKENS];
  __shared__ unsigned s_met[CN_MAX_BEAM], s_gmask;
  __shared__ int s_c[CN_MAX_BEAM];
  __shared__ float s_rq[CN_MAX_BEAM][RQ_MAX_TOKENS];
  __shared__ ValIdx s_ord[RQ_BANKS][CN_MAX_BEAM], s_fin[RQ_BANKS][CN_MAX_BEAM];
  __shared__ int s_nfin[RQ_BANKS];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int ldv = a.ldv, V = a.V, beam = a.beam, maxp = a.maxp, n = ca.ngram;
  const int k = a.n_active[b];
  if (k == 0) return;
  const int rb = b * beam;
  const int plen = cn_prefix_len(ca, b);
  const int ftok = cn_prefix_tok(ca, b, step);
  const bool forced = step < plen;
  const int nrows = step <= plen ? 1 : k;

  for (int i = tid; i < k * (maxp + 1); i += 256) s_prefix[i / (maxp + 1)][i % (maxp + 1)] = a.prefix[(size_t)rb * (maxp + 1) + i];
  for (int i = tid; i < k * maxp; i += 256) s_anc[i / maxp][i % maxp] = a.anc[(size_t)rb * maxp + i];
  if (tid < k) {
    s_slot[tid] = a.slot[rb + tid];
    s_base[tid] = step == 0 ? 0.f : a.sum_lp[rb + tid];
  }
  if (tid < RQ_MAX_TOKENS) rq_stage(ra, b, V, tid, s_rt, s_rg0);
  if (tid >= 64 && tid < 64 + CN_MAX_BEAM) s_met[tid - 64] = 0u;
  if (tid == 128) s_gmask = 0u;
  for (int i = tid; i < CN_MAX_BEAM * RQ_MAX_TOKENS; i += 256) s_rq[i / RQ_MAX_TOKENS][i % RQ_MAX_TOKENS] = -INFINITY;
  if (ca.step_logits) {  // the RAW logits, before the masks go into them
    float* o = ca.step_logits + ((size_t)step * gridDim.x * beam + rb) * V;
    for (int p = 0; p < beam; ++p)
      for (int v = tid; v < V; v += 256) o[(size_t)p * V + v] = a.logits[(size_t)(rb + p) * ldv + v];
  }
  __syncthreads();
  if (tid < RQ_MAX_TOKENS) s_rg[tid] = rq_dedupe(tid, s_rt, s_rg0);
  __syncthreads();
  rq_find_met<256>(s_prefix, nrows, step, s_rt, s_rg, s_met, &s_gmask);
  // EOS floor + forbid-repeat, the ban mask and the n-gram rule, in place, once per candidate row
  for (int i = tid; i < nrows * (step + 2); i += 256) {
    const int p = i / (step + 2), j = i % (step + 2);
    float* lg = a.logits + (size_t)(rb + p) * ldv;
    if (j == step + 1) {
      if (step < a.min_pred) lg[a.eos_id] = -INFINITY;
    } else {
      const int tok = s_prefix[p][j];
      if (a.forbid != nullptr && a.forbid[tok]) lg[tok] = -INFINITY;
      if (n > 0 && j <= step - n + 1) {
        const int t = cn_ngram_banned(s_prefix[p], step, n, j);
        if (t >= 0) lg[t] = -INFINITY;
      }
    }
  }
  if (ca.ban != nullptr)
    for (int v = tid; v < V; v += 256)
      if (ca.ban[v] != 0)
        for (int p = 0; p < nrows; ++p) a.logits[(size_t)(rb + p) * ldv + v] = -INFINITY;
  __syncthreads();  // the met bits are complete
  const unsigned gmask = s_gmask;
  unsigned cmask = 0;  // bit c: a candidate row has c met groups
  bool open = false;   // a candidate row has an unmet group
  for (int p = 0; p < nrows; ++p) {
    cmask |= 1u << __popc(s_met[p] & gmask);
    open |= (gmask & ~s_met[p]) != 0u;
  }
  if (tid < nrows) s_c[tid] = __popc(s_met[tid] & gmask);
  if (open) {  // M4 and M5, in place
    for (int p = 0; p < nrows; ++p) {
      const unsigned left = gmask & ~s_met[p];
      if (left == 0u) continue;
      float* lg = a.logits + (size_t)(rb + p) * ldv;
      if (tid == 0) lg[a.eos_id] = -INFINITY;
      if (__popc(left) >= maxp - step)  // only the tokens of the unmet groups stay
        for (int v = tid; v < V; v += 256) {
          bool keep = false;
          for (int e = 0; e < RQ_MAX_TOKENS; ++e) keep |= s_rg[e] >= 0 && ((left >> s_rg[e]) & 1u) && s_rt[e] == v;
          if (!keep) lg[v] = -INFINITY;
        }
    }
  }
  __syncthreads();
  // log-softmax statistics per row
  for (int p = 0; p < nrows; ++p) {
    const float* lg = a.logits + (size_t)(rb + p) * ldv;
    float mx = -INFINITY;
    for (int v = tid; v < V; v += 256) mx = fmaxf(mx, lg[v]);
    mx = cn_wave_max(mx);
    if (lane == 0) s_red[wv] = mx;
    __syncthreads();
    mx = fmaxf(fmaxf(s_red[0], s_red[1]), fmaxf(s_red[2], s_red[3]));
    float sm = 0.f;
    for (int v = tid; v < V; v += 256) sm += expf(lg[v] - mx);
    sm = cn_wave_sum(sm);
    if (lane == 0) s_red[4 + wv] = sm;
    __syncthreads();
    if (tid == 0) {
      s_mx[p] = mx;
      s_lg[p] = logf(s_red[4] + s_red[5] + s_red[6] + s_red[7]);
    }
    __syncthreads();
  }
  if (forced) {
    if (tid == 0) {
      s_self[0] = CN_NO_PICK;
      if (ftok >= 0 && ftok < V && ftok != a.eos_id) {
        float m = (a.logits[(size_t)rb * ldv + ftok] - s_mx[0]) - s_lg[0];
        if (step != 0) m = s_base[0] + m;
        if (m > -INFINITY && m < INFINITY) {
          s_selv[0] = m;
          s_self[0] = ftok;
        }
      }
    }
    __syncthreads();
    cn_constrain_commit<256>(a, b, k, step, true, s_selv, s_self, s_prefix, s_anc, s_slot, s_newpos);
    return;
  }
  if (open) {  // the candidates of the unmet groups leave the logits for LDS (a token is in the table once: no two threads meet)
    for (int i = tid; i < nrows * RQ_MAX_TOKENS; i += 256) {
      const int p = i / RQ_MAX_TOKENS, e = i % RQ_MAX_TOKENS;
      const unsigned left = gmask & ~s_met[p];
      if (s_rg[e] >= 0 && ((left >> s_rg[e]) & 1u)) {
        float* lg = a.logits + (size_t)(rb + p) * ldv;
        float cand = (lg[s_rt[e]] - s_mx[p]) - s_lg[p];
        if (step != 0) cand = s_base[p] + cand;
        s_rq[p][e] = (cand > -INFINITY && cand < INFINITY) ? cand : -INFINITY;
        lg[s_rt[e]] = -INFINITY;
      }
    }
    __syncthreads();
  }
  // the ordinary top-k, once per distinct c(p): k rounds of block arg-max over the rows with that c (ties -> lowest flat index);
  // a round that finds no finite candidate takes no pick
  for (int c = RQ_MAX_GROUPS; c >= 0; --c) {
    if (!((cmask >> c) & 1u)) continue;
    for (int r = 0; r < k; ++r) {
      ValIdx best{-INFINITY, CN_NO_PICK};
      for (int p = 0; p < nrows; ++p) {
        if (s_c[p] != c) continue;
        const float* lg = a.logits + (size_t)(rb + p) * ldv;
        const float mx = s_mx[p], lgs = s_lg[p], base = s_base[p];
        for (int v = tid; v < V; v += 256) {
          const int flat = p * V + v;
          bool taken = false;
          for (int d = 0; d < r; ++d) taken |= (s_ord[c][d].i == flat);
          if (taken) continue;
          float cand = (lg[v] - mx) - lgs;
          if (step != 0) cand = base + cand;
          best = vi_better(best, ValIdx{cand, flat});
        }
      }
      best = vi_wave(best);
      if (lane == 0) s_vi[wv] = best;
      __syncthreads();
      if (tid == 0) {
        const ValIdx r0 = vi_better(vi_better(s_vi[0], s_vi[1]), vi_better(s_vi[2], s_vi[3]));
        s_ord[c][r] = ValIdx{r0.v, r0.v > -INFINITY ? r0.i : CN_NO_PICK};
      }
      __syncthreads();
    }
  }
  if (!open) {  // one bank, nothing moved out: its list is the call's picks
    const int c0 = 31 - __clz((int)cmask);
    if (tid < k) {
      s_selv[tid] = s_ord[c0][tid].v;
      s_self[tid] = s_ord[c0][tid].i;
    }
  } else if (wv == 0) {
    rq_deal<CN_MAX_BEAM>(k, nrows, V, cmask, s_c, s_ord, s_rq, s_rt, s_fin, s_nfin, s_selv, s_self);
  }
  __syncthreads();
  cn_constrain_commit<256>(a, b, k, step, false, s_selv, s_self, s_prefix, s_anc, s_slot, s_newpos);
}

// The step launch of decode_impl: the kernel the plain search runs at this (V, W), instantiated as the plain search's.
static inline void cn_require_step_launch(const SsArgs& ss, const CsArgs& cs, const RqArgs& rq, int B, int step, hipStream_t s) {
  if (ss.V <= S3_T * S3_VPT && ss.beam <= 8) {
#define RQ_LAUNCH(NR_, VPT_) hipLaunchKernelGGL((cn_require_step3_kernel<NR_, VPT_>), dim3(B), dim3(S3_T), 0, s, ss, cs, rq, step)
    const int slabs = cn_cdiv(ss.V, S3_T);
    if (ss.beam <= 4) {
      if (slabs <= 2) RQ_LAUNCH(4, 2);
      else if (slabs <= 4) RQ_LAUNCH(4, 4);
      else if (slabs <= 6) RQ_LAUNCH(4, 6);
      else RQ_LAUNCH(4, 8);
    } else {
      if (slabs <= 4) RQ_LAUNCH(8, 4);
      else RQ_LAUNCH(8, 8);
    }
#undef RQ_LAUNCH
  } else {
    hipLaunchKernelGGL(cn_require_step_kernel, dim3(B), dim3(256), 0, s, ss, cs, rq, step);
  }
}
