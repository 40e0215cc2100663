// Constrained beam search (conette_decode_constrained, include/conette_hip.h; the CPU restatement of the rule is
// conette_amd/constrained_search.py): one search step of one clip at beam W whose caller steers the search with a forced beginning
// (a prefix per clip), a mask of tokens that never appear, and a ban on repeating any n-gram.
//
// Masks of a candidate row at step i, on its raw logits: the plain search's (EOS floor while i < min_pred, forbid-repeat over the
// row's sequence s_0 .. s_i), then -inf for every token of the ban mask, then -inf for the token behind every earlier occurrence
// of the row's last n - 1 tokens (cn_ngram_banned; n = 1: every token of the sequence).  The log-softmax of the masked row is
// summed in the order of the plain kernel that runs at this (V, W): cn_search_step3_kernel's in the register kernel,
// cn_search_step_kernel's in the generic one, which are dispatched on the same condition.
// Calls of clip b with prefix length plen: steps i < plen are FORCED -- the only candidate is (row 0, prefix[b][i]); its model
// score m = sum_lp[0] + lp[0][t] goes on in row 0, the clip keeps its W live rows, and a token whose m is not finite (masked, or
// no token of the vocabulary, or <eos>) voids the whole clip.  Step plen is the FAN-OUT: W picks over row 0's V candidates (the
// plain search's step 0 when plen = 0); later steps are the plain search's step over the k live rows.
// Picks are the top k FINITE scores, ties to the lowest flat index; with f < k finite candidates there are f picks, the output
// slots of row positions f .. k - 1 become void (score -inf, length 0, pad_id throughout) and nothing is indexed by a pick
// that does not exist.  The bookkeeping is cn_search_commit's.
//
// Two kernels, as for the plain search.  Register-resident (W <= 8, V <= 8192; 1024 threads): the ban mask is one bit per slab in
// one register beside the forbid flags; the n-gram tokens of every candidate row are found once, one thread per start position,
// into LDS and applied by the token's owner thread as selects (cn_ban_registers: the wave-uniform early-out of cn_mask_registers);
// a forced call takes no top-k, the token's owner thread forms m from the block's statistics.  Generic (256 threads, logits in
// global memory): the three masks go into the logits in place, once per candidate row.
#pragma once

#include "dec_search.h"

#define CN_MAX_NGRAM 64
#define CN_NO_PICK 0x7fffffff  // the flat index of a pick that does not exist (no finite candidate was left)

struct CsArgs {
  const int* prefix;       // (B, P) or null
  const int* prefix_lens;  // (B) or null
  const uint8_t* ban;      // (V) or null
  float* step_logits;      // (maxp, R, V) or null: the raw logits of every row of a clip that still searches, per step
  int P, ngram;
};

// The token the n-gram rule takes from a row whose sequence is seq[0 .. step], for the start position 0 <= j <= step - n + 1
// (n >= 1): seq[j + n - 1] if seq[j .. j + n - 2] equals the sequence's last n - 1 tokens, else -1.
__device__ __forceinline__ int cn_ngram_banned(const int* seq, int step, int n, int j) {
  bool same = true;
  for (int q = 0; q + 1 < n; ++q) same &= seq[j + q] == seq[step - n + 2 + q];
  return same ? seq[j + n - 1] : -1;
}

// -inf into the registers that hold the tokens of list[0 .. n) (entries < 0: none); the layout and the owner-wave test are
// cn_mask_registers'.
template <int THREADS, int VPT>
__device__ __forceinline__ void cn_ban_registers(float (&val)[VPT], const int* list, int n, int tid, int wv) {
  static_assert(THREADS == 1024, "a token's slab is tok >> 10");
  for (int j = 0; j < n; ++j) {
    const int tok = list[j];
    if (tok >= 0 && (((unsigned)tok & (THREADS - 1)) >> 6) == (unsigned)wv) {
      if ((tok & (THREADS - 1)) == tid) {
#pragma unroll
        for (int sl = 0; sl < VPT; ++sl) val[sl] = sl == (tok >> 10) ? -INFINITY : val[sl];
      }
    }
  }
}

// The prefix length of clip b (clamped to the table's width) and the token a forced call of `step` takes (-1: none in the table).
__device__ __forceinline__ int cn_prefix_len(const CsArgs& ca, int b) {
  return (ca.prefix != nullptr && ca.prefix_lens != nullptr) ? min(max(ca.prefix_lens[b], 0), ca.P) : 0;
}
__device__ __forceinline__ int cn_prefix_tok(const CsArgs& ca, int b, int step) {
  return (ca.prefix != nullptr && step < ca.P) ? ca.prefix[(size_t)b * ca.P + step] : -1;
}

// The bookkeeping of a call whose picks are in s_selv / s_self, the missing ones (CN_NO_PICK) behind the others: `forced` -- one
// pick that goes on in row 0 while the clip keeps its k live rows, or none and the clip is void; else cn_search_commit on the f
// picks there are, and the slots of the row positions f .. k - 1 become void.
template <int THREADS>
__device__ __forceinline__ void cn_constrain_commit(const SsArgs& a, int b, int k, int step, bool forced, const float* s_selv,
                                                    const int* s_self, const int (*s_prefix)[CN_MAX_PRED + 1],
                                                    const int (*s_anc)[CN_MAX_PRED], const int* s_slot, int* s_newpos) {
  const int tid = threadIdx.x, rb = b * a.beam;
  if (forced) {
    if (s_self[0] == CN_NO_PICK) {  // the clip leaves the search: every slot void (their tokens are pad_id since the initialisation)
      if (tid < a.beam) {
        a.out_avg[rb + tid] = -INFINITY;
        a.out_len[rb + tid] = 0;
      }
      if (tid == 0) a.n_active[b] = 0;
      return;
    }
    // (a forced token is never <eos> and a forced step never the last one: the pick continues, live[step + 1] becomes positive)
    cn_search_commit<THREADS>(a, b, 1, step, s_selv, s_self, s_prefix, s_anc, s_slot, s_newpos);
    if (tid == 0) a.n_active[b] = k;
    return;
  }
  int f = 0;
  for (int c = 0; c < k; ++c) f += s_self[c] != CN_NO_PICK;
  cn_search_commit<THREADS>(a, b, f, step, s_selv, s_self, s_prefix, s_anc, s_slot, s_newpos);
  if (tid >= f && tid < k) {
    const int sl = rb + s_slot[tid];
    a.out_avg[sl] = -INFINITY;
    a.out_len[sl] = 0;
  }
}

// Register-resident step: NR >= W rows, VPT logits per thread and row (the layout of cn_search_step3_kernel).
template <int NR, int VPT>
__global__ __launch_bounds__(S3_T) void cn_constrain_step3_kernel(const SsArgs a, const CsArgs ca, const int step) {
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
  float rmx[NR], rlg[NR];
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
      rlg[p] = logf(sm);
    }
  if (forced) {  // no top-k: the owner of the token forms its model score
    if (ftok >= 0 && ftok < V && ftok != a.eos_id && (ftok & (S3_T - 1)) == tid) {
      float z = -INFINITY;
#pragma unroll
      for (int sl = 0; sl < VPT; ++sl) z = sl == (ftok >> 10) ? val[0][sl] : z;
      float m = (z - rmx[0]) - rlg[0];
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
    if (p < nrows) {
      const float base = s_base[p];
#pragma unroll
      for (int sl = 0; sl < VPT; ++sl) {
        const int v = sl * S3_T + tid;
        float cand = (val[p][sl] - rmx[p]) - rlg[p];
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
        ValIdx mine{-INFINITY, CN_NO_PICK};
#pragma unroll
        for (int j = 0; j < NR; ++j)
          if (head == j) mine = ValIdx{bv[j], bi[j]};
        const ValIdx best = vi_wave_dpp(mine);
        if (mine.i == best.i && mine.i != CN_NO_PICK) ++head;
        if (lane == 0) s_cand[wv][c] = best;
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
    for (int c = 0; c < NR; ++c)
      if (c < k) {
        const ValIdx best = vi_wave_dpp(vi_better(t0, t1));
        if (best.i != CN_NO_PICK) {
          if (t0.i == best.i) t0 = ValIdx{-INFINITY, CN_NO_PICK};
          else if (t1.i == best.i) t1 = ValIdx{-INFINITY, CN_NO_PICK};
        }
        if (tid == 0) {
          s_selv[c] = best.v;
          s_self[c] = best.i;
        }
      }
  }
  __syncthreads();
  cn_constrain_commit<S3_T>(a, b, k, step, false, s_selv, s_self, s_prefix, s_anc, s_slot, s_newpos);
}

// Generic step: any W <= CN_MAX_BEAM and any V (the layout and the sums of cn_search_step_kernel).
__global__ __launch_bounds__(256) void cn_constrain_step_kernel(const SsArgs a, const CsArgs ca, const int step) {
  __shared__ float s_red[8];
  __shared__ ValIdx s_vi[4];
  __shared__ float s_mx[CN_MAX_BEAM], s_lg[CN_MAX_BEAM], s_base[CN_MAX_BEAM];
  __shared__ float s_selv[CN_MAX_BEAM];
  __shared__ int s_self[CN_MAX_BEAM];
  __shared__ int s_prefix[CN_MAX_BEAM][CN_MAX_PRED + 1];
  __shared__ int s_anc[CN_MAX_BEAM][CN_MAX_PRED];
  __shared__ int s_slot[CN_MAX_BEAM];
  __shared__ int s_newpos[CN_MAX_BEAM];
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
  if (ca.step_logits) {  // the RAW logits, before the masks go into them
    float* o = ca.step_logits + ((size_t)step * gridDim.x * beam + rb) * V;
    for (int p = 0; p < beam; ++p)
      for (int v = tid; v < V; v += 256) o[(size_t)p * V + v] = a.logits[(size_t)(rb + p) * ldv + v];
  }
  __syncthreads();
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
  // top-k over the nrows * V candidates, k rounds of block arg-max (ties -> lowest flat index); a round that finds no finite
  // candidate takes no pick
  for (int c = 0; c < k; ++c) {
    ValIdx best{-INFINITY, CN_NO_PICK};
    for (int p = 0; p < nrows; ++p) {
      const float* lg = a.logits + (size_t)(rb + p) * ldv;
      const float mx = s_mx[p], lgs = s_lg[p], base = s_base[p];
      for (int v = tid; v < V; v += 256) {
        const int flat = p * V + v;
        bool taken = false;
        for (int d = 0; d < c; ++d) taken |= (s_self[d] == flat);
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
      s_selv[c] = r0.v;
      s_self[c] = r0.v > -INFINITY ? r0.i : CN_NO_PICK;
    }
    __syncthreads();
  }
  cn_constrain_commit<256>(a, b, k, step, false, s_selv, s_self, s_prefix, s_anc, s_slot, s_newpos);
}

// The step launch of decode_impl: the kernel the plain search runs at this (V, W), instantiated as the plain search's.
static inline void cn_constrain_step_launch(const SsArgs& ss, const CsArgs& cs, int B, int step, hipStream_t s) {
  if (ss.V <= S3_T * S3_VPT && ss.beam <= 8) {
#define CS_LAUNCH(NR_, VPT_) hipLaunchKernelGGL((cn_constrain_step3_kernel<NR_, VPT_>), dim3(B), dim3(S3_T), 0, s, ss, cs, step)
    const int slabs = cn_cdiv(ss.V, S3_T);
    if (ss.beam <= 4) {
      if (slabs <= 2) CS_LAUNCH(4, 2);
      else if (slabs <= 4) CS_LAUNCH(4, 4);
      else if (slabs <= 6) CS_LAUNCH(4, 6);
      else CS_LAUNCH(4, 8);
    } else {
      if (slabs <= 4) CS_LAUNCH(8, 4);
      else CS_LAUNCH(8, 8);
    }
#undef CS_LAUNCH
  } else {
    hipLaunchKernelGGL(cn_constrain_step_kernel, dim3(B), dim3(256), 0, s, ss, cs, step);
  }
}
