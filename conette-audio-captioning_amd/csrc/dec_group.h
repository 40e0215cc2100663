// Diverse beam search (Vijayakumar et al. 2016; conette_decode_groups, include/conette_hip.h; the CPU restatement of the rule is
// conette_amd/group_search.py): one search step of one clip whose beam = G * W rows are split into G groups of W beams.
//
// Rows.  Clip b owns rows b * G * W ..; group g owns rows g * W .. g * W + W - 1 of the clip, its k_g live rows compacted to the
// front of its own range; anc entries are within-clip rows (g * W + parent), so a row's ancestors never leave its group and the
// block / FFN / classifier kernels run on the rows as they run on a plain search of beam G * W.
// One step.  Masks and log-softmax of every live row as the plain searches compute them (dec_search.h), then the groups IN ORDER:
// model score m(p, v) = sum_lp[p] + lp[p][v]; c[v] = picks of this step by the earlier groups of the clip whose token is v (every
// pick counts, finishing ones included); key = m if c[v] == 0, else m - lambda * c[v] as one rounded multiply and one rounded
// subtract (cn_group_key); the picks are the top k_g keys over the group's k_g * V candidates (step 0: its first row), ties to the
// lowest flat index p * V + v; a pick CARRIES m, never its key; the bookkeeping is cn_search_commit on the group's rows.
// The G top-k calls of a clip depend on one another and a decode step is bound by launch latency: they are one launch per step.
//
// Two kernels, as for the plain search.  Register-resident (G * W <= 8, V <= 8192; 1024 threads): the logits of all G * W rows read
// up front in one coalesced pass, the statistics of all rows together, then per group a per-thread sorted top list with the penalty
// applied, the two-level wave merge and the commit.  The counts live with the token's owner thread (tid = v & 1023), four bits per
// slab v >> 10 packed in one register (a count is at most 7 here).  Generic (256 threads, logits in global memory, masked in place
// once per row): k rounds of block arg-max per group; the tokens picked so far at this step sit in LDS (<= 15), and only the
// threads that own one of them (v & 255) look at the list.
// Bits.  With one group, for group 0 of any search, and with lambda = 0 for every group, the picks and the carried sums are those of
// the plain search at beam W on the same logits.  The log-sum-exp is therefore summed in the order of the kernel conette_decode
// runs at beam W: the generic kernel sums as cn_search_step3_kernel does (its 1024 threads' partial sums, 16 wave sums, in
// sequence) when W <= 8 and V <= 8192, and as cn_search_step_kernel does otherwise.
#pragma once

#include "dec_search.h"

struct GsArgs {
  float* step_logits;  // (maxp, R, V) or null: the raw logits of every row of a clip that still searches, per step
  int G, W;
  float lambda;
};

// the selection key of a candidate with model score m whose token the earlier groups picked c times at this step
__device__ __forceinline__ float cn_group_key(float m, float lambda, int c) {
#pragma clang fp contract(off)
  const float pen = lambda * (float)c;
  const float key = m - pen;
  return c == 0 ? m : key;
}

__global__ void cn_group_init_kernel(int n, int W, int* __restrict__ group_k) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) group_k[i] = W;
}

// Register-resident step: NR >= G * W rows, VPT logits per thread and row.  a.n_active is (B, G): the live rows of every group.
template <int NR, int VPT>
__global__ __launch_bounds__(S3_T) void cn_group_step3_kernel(const SsArgs a, const GsArgs ga, const int step) {
  __shared__ float s_redm[NR][16], s_reds[NR][16];
  __shared__ ValIdx s_cand[16][NR];
  __shared__ float s_base[NR];
  __shared__ float s_selv[NR];
  __shared__ int s_self[NR];
  __shared__ int s_prefix[NR][CN_MAX_PRED + 1];
  __shared__ int s_anc[NR][CN_MAX_PRED];
  __shared__ int s_slot[NR];
  __shared__ int s_newpos[NR];
  __shared__ int s_k[NR];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int ldv = a.ldv, V = a.V, beam = a.beam, maxp = a.maxp, G = ga.G, W = ga.W;
  const int rb = b * beam;
  // every global read is issued up front and none depends on another (as cn_search_step3_kernel)
  float val[NR][VPT];
  bool fb[VPT];
#pragma unroll
  for (int sl = 0; sl < VPT; ++sl) {
    const int v = sl * S3_T + tid;
    fb[sl] = a.forbid != nullptr && v < V && a.forbid[v] != 0;
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
  if (tid < G) s_k[tid] = a.n_active[b * G + tid];
  __syncthreads();
  // bit p of `rows`: row p of the clip is a candidate row of its group at this step
  unsigned rows = 0;
  for (int g = 0; g < G; ++g) {
    const int k = s_k[g];
    rows |= ((1u << (step == 0 ? (k > 0 ? 1 : 0) : k)) - 1u) << (g * W);
  }
  if (rows == 0) return;  // every group of the clip has finished
  if (ga.step_logits) {   // the RAW logits this step's decisions see
    float* o = ga.step_logits + ((size_t)step * gridDim.x * beam + rb) * V;
#pragma unroll
    for (int p = 0; p < NR; ++p)
      if (p < beam) {
#pragma unroll
        for (int sl = 0; sl < VPT; ++sl)
          if (sl * S3_T + tid < V) o[(size_t)p * V + sl * S3_T + tid] = val[p][sl];
      }
  }
#pragma unroll
  for (int p = 0; p < NR; ++p)
    if ((rows >> p) & 1) cn_mask_registers<S3_T>(val[p], fb, s_prefix[p], step, a.min_pred, a.eos_id, tid, wv);
  // log-softmax statistics of every candidate row (the expressions and the summation order of cn_search_step3_kernel)
#pragma unroll
  for (int p = 0; p < NR; ++p)
    if ((rows >> p) & 1) {
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
    if ((rows >> p) & 1) {
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
    if ((rows >> p) & 1) {
      float sm = s_reds[p][0];
#pragma unroll
      for (int w = 1; w < 16; ++w) sm += s_reds[p][w];
      rlg[p] = logf(sm);
    }
  unsigned cnt = 0;  // 4 bits per slab: picks of this step, by the groups so far, of this thread's token of the slab
  for (int g = 0; g < G; ++g) {
    const int k = s_k[g];
    if (k == 0) continue;  // takes no picks, adds nothing to the counts
    const int p0 = g * W, nrows = step == 0 ? 1 : k;
    // per-thread sorted top list by key (strict > keeps the lower flat index first on ties); bm = the model score of the entry
    float bv[NR], bm[NR];
    int bi[NR];
#pragma unroll
    for (int j = 0; j < NR; ++j) {
      bv[j] = -INFINITY;
      bm[j] = -INFINITY;
      bi[j] = 0x7fffffff;
    }
#pragma unroll
    for (int p = 0; p < NR; ++p)
      if (p >= p0 && p < p0 + nrows) {
        const float base = s_base[p];
#pragma unroll
        for (int sl = 0; sl < VPT; ++sl) {
          const int v = sl * S3_T + tid;
          float m = (val[p][sl] - rmx[p]) - rlg[p];
          if (step != 0) m = base + m;
          const float key = cn_group_key(m, ga.lambda, (int)((cnt >> (4 * sl)) & 15u));
          if (v < V && key > bv[NR - 1]) {
            bv[NR - 1] = key;
            bm[NR - 1] = m;
            bi[NR - 1] = (p - p0) * V + v;
#pragma unroll
            for (int j = NR - 1; j > 0; --j) {
              if (bv[j] > bv[j - 1]) {
                const float tv = bv[j];
                bv[j] = bv[j - 1];
                bv[j - 1] = tv;
                const float tm = bm[j];
                bm[j] = bm[j - 1];
                bm[j - 1] = tm;
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
            s_selv[c] = best.v;  // (the key: only a pick no thread owns -- fewer finite candidates than picks -- keeps it)
            s_self[c] = best.i;
          }
        }
    }
    __syncthreads();
    // what a pick carries is its model score: written by the thread whose list holds the pick; the owner of its token counts it
    for (int c = 0; c < k; ++c) {
      const int flat = s_self[c];
      if (flat == 0x7fffffff) continue;
#pragma unroll
      for (int j = 0; j < NR; ++j)
        if (bi[j] == flat) s_selv[c] = bm[j];
      const int tok = flat % V;
      if ((tok & (S3_T - 1)) == tid) cnt += 1u << (4 * (tok >> 10));
    }
    __syncthreads();
    cn_search_commit<S3_T>(a, b, k, step, s_selv, s_self, s_prefix + p0, s_anc + p0, s_slot + p0, s_newpos, p0, b * G + g);
  }
}

// Generic step: any G * W <= CN_MAX_BEAM and any V.  `reg_sums`: the log-sum-exp in the summation order of the register kernels.
__global__ __launch_bounds__(256) void cn_group_step_kernel(const SsArgs a, const GsArgs ga, const int step, const int reg_sums) {
  __shared__ float s_red[8];
  __shared__ float s_reds[16];
  __shared__ ValIdx s_vi[4];
  __shared__ float s_mx[CN_MAX_BEAM], s_lg[CN_MAX_BEAM], s_base[CN_MAX_BEAM];
  __shared__ float s_selv[CN_MAX_BEAM];
  __shared__ int s_self[CN_MAX_BEAM];
  __shared__ int s_prefix[CN_MAX_BEAM][CN_MAX_PRED + 1];
  __shared__ int s_anc[CN_MAX_BEAM][CN_MAX_PRED];
  __shared__ int s_slot[CN_MAX_BEAM];
  __shared__ int s_newpos[CN_MAX_BEAM];
  __shared__ int s_k[CN_MAX_BEAM];
  __shared__ int s_ptok[CN_MAX_BEAM];  // tokens picked at this step by the groups so far
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int ldv = a.ldv, V = a.V, beam = a.beam, maxp = a.maxp, G = ga.G, W = ga.W;
  const int rb = b * beam;
  if (tid < G) s_k[tid] = a.n_active[b * G + tid];
  for (int i = tid; i < beam * (maxp + 1); i += 256) s_prefix[i / (maxp + 1)][i % (maxp + 1)] = a.prefix[(size_t)rb * (maxp + 1) + i];
  for (int i = tid; i < beam * maxp; i += 256) s_anc[i / maxp][i % maxp] = a.anc[(size_t)rb * maxp + i];
  if (tid < beam) {
    s_slot[tid] = a.slot[rb + tid];
    s_base[tid] = step == 0 ? 0.f : a.sum_lp[rb + tid];
  }
  __syncthreads();
  unsigned rows = 0;  // bit p: row p of the clip is a candidate row of its group at this step
  for (int g = 0; g < G; ++g) {
    const int k = s_k[g];
    rows |= ((1u << (step == 0 ? (k > 0 ? 1 : 0) : k)) - 1u) << (g * W);
  }
  if (rows == 0) return;
  if (ga.step_logits) {  // the RAW logits, before the masks go into them
    float* o = ga.step_logits + ((size_t)step * gridDim.x * beam + rb) * V;
    for (int p = 0; p < beam; ++p)
      for (int v = tid; v < V; v += 256) o[(size_t)p * V + v] = a.logits[(size_t)(rb + p) * ldv + v];
    __syncthreads();
  }
  // EOS floor + forbid-repeat, in place, once per candidate row
  for (int i = tid; i < beam * (step + 2); i += 256) {
    const int p = i / (step + 2), j = i % (step + 2);
    if (!((rows >> p) & 1)) continue;
    float* lg = a.logits + (size_t)(rb + p) * ldv;
    if (j == step + 1) {
      if (step < a.min_pred) lg[a.eos_id] = -INFINITY;
    } else if (a.forbid != nullptr) {
      const int tok = s_prefix[p][j];
      if (a.forbid[tok]) lg[tok] = -INFINITY;
    }
  }
  __syncthreads();
  for (int p = 0; p < beam; ++p) {
    if (!((rows >> p) & 1)) continue;  // (block-uniform)
    const float* lg = a.logits + (size_t)(rb + p) * ldv;
    float mx = -INFINITY;
    for (int v = tid; v < V; v += 256) mx = fmaxf(mx, lg[v]);
    mx = cn_wave_max(mx);
    if (lane == 0) s_red[wv] = mx;
    __syncthreads();
    mx = fmaxf(fmaxf(s_red[0], s_red[1]), fmaxf(s_red[2], s_red[3]));
    if (reg_sums) {
      // cn_search_step3_kernel's sum: thread t of 1024 adds its logits t, t + 1024, .. in order, a wave adds its 64 threads by
      // cn_wave_sum_dpp, the 16 wave sums are added in sequence.  This thread plays threads tid + 256 j (waves wv + 4 j).
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        float sm = 0.f;
        for (int v = tid + 256 * j; v < V; v += S3_T) sm += __expf(lg[v] - mx);
        sm = cn_wave_sum_dpp(sm);
        if (lane == 0) s_reds[wv + 4 * j] = sm;
      }
      __syncthreads();
      if (tid == 0) {
        float sm = s_reds[0];
        for (int w = 1; w < 16; ++w) sm += s_reds[w];
        s_mx[p] = mx;
        s_lg[p] = logf(sm);
      }
    } else {  // cn_search_step_kernel's sum
      float sm = 0.f;
      for (int v = tid; v < V; v += 256) sm += expf(lg[v] - mx);
      sm = cn_wave_sum(sm);
      if (lane == 0) s_red[4 + wv] = sm;
      __syncthreads();
      if (tid == 0) {
        s_mx[p] = mx;
        s_lg[p] = logf(s_red[4] + s_red[5] + s_red[6] + s_red[7]);
      }
    }
    __syncthreads();
  }
  int np = 0;  // entries of s_ptok
  for (int g = 0; g < G; ++g) {
    const int k = s_k[g];
    if (k == 0) continue;
    const int p0 = g * W, nrows = step == 0 ? 1 : k;
    bool owner = false;  // this thread's tokens (v & 255 == tid) hold one that was picked at this step
    for (int i = 0; i < np; ++i) owner |= (s_ptok[i] & 255) == tid;
    // k rounds of block arg-max over the group's nrows * V keys (ties -> lowest flat index)
    for (int c = 0; c < k; ++c) {
      ValIdx best{-INFINITY, 0x7fffffff};
      for (int p = 0; p < nrows; ++p) {
        const float* lg = a.logits + (size_t)(rb + p0 + p) * ldv;
        const float mx = s_mx[p0 + p], lgs = s_lg[p0 + p], base = s_base[p0 + p];
        for (int v = tid; v < V; v += 256) {
          const int flat = p * V + v;
          bool taken = false;
          for (int d = 0; d < c; ++d) taken |= (s_self[d] == flat);
          if (taken) continue;
          float m = (lg[v] - mx) - lgs;
          if (step != 0) m = base + m;
          int cn = 0;
          if (owner)
            for (int i = 0; i < np; ++i) cn += s_ptok[i] == v;
          best = vi_better(best, ValIdx{cn_group_key(m, ga.lambda, cn), flat});
        }
      }
      best = vi_wave(best);
      if (lane == 0) s_vi[wv] = best;
      __syncthreads();
      if (tid == 0) {
        const ValIdx r0 = vi_better(vi_better(s_vi[0], s_vi[1]), vi_better(s_vi[2], s_vi[3]));
        float m = r0.v;
        if (r0.i != 0x7fffffff) {  // the pick carries its model score: the same expression on the same operands
          const int p = r0.i / V, v = r0.i % V;
          m = (a.logits[(size_t)(rb + p0 + p) * ldv + v] - s_mx[p0 + p]) - s_lg[p0 + p];
          if (step != 0) m = s_base[p0 + p] + m;
        }
        s_selv[c] = m;
        s_self[c] = r0.i;
      }
      __syncthreads();
    }
    if (tid == 0)
      for (int c = 0; c < k; ++c) s_ptok[np + c] = s_self[c] == 0x7fffffff ? -1 : s_self[c] % V;
    np += k;
    // (cn_search_commit's barrier orders the s_ptok writes before the next group reads them)
    cn_search_commit<256>(a, b, k, step, s_selv, s_self, s_prefix + p0, s_anc + p0, s_slot + p0, s_newpos, p0, b * G + g);
  }
}

// The step launch of decode_impl: the register kernel where the clip's G * W rows and the vocabulary fit it, instantiated as the
// plain search's (NR 4 / 8 rows, 2 .. 8 logits per thread), else the generic one.
static inline void cn_group_step_launch(const SsArgs& ss, const GsArgs& gs, int B, int step, hipStream_t s) {
  const bool fits_registers = ss.V <= S3_T * S3_VPT;
  if (fits_registers && ss.beam <= 8) {
#define GS_LAUNCH(NR_, VPT_) hipLaunchKernelGGL((cn_group_step3_kernel<NR_, VPT_>), dim3(B), dim3(S3_T), 0, s, ss, gs, step)
    const int slabs = cn_cdiv(ss.V, S3_T);
    if (ss.beam <= 4) {
      if (slabs <= 2) GS_LAUNCH(4, 2);
      else if (slabs <= 4) GS_LAUNCH(4, 4);
      else if (slabs <= 6) GS_LAUNCH(4, 6);
      else GS_LAUNCH(4, 8);
    } else {
      if (slabs <= 4) GS_LAUNCH(8, 4);
      else GS_LAUNCH(8, 8);
    }
#undef GS_LAUNCH
  } else {  // the log-sum-exp as the plain search of beam W sums it
    hipLaunchKernelGGL(cn_group_step_kernel, dim3(B), dim3(256), 0, s, ss, gs, step, (fits_registers && gs.W <= 8) ? 1 : 0);
  }
}
