// The beam search's device code: one search step for one clip (beam.py:125-203, _select_k_next_toks :230-269) in two kernels --
// the generic step (256 threads, masking in place, top-k over global memory) and the register-resident step (1024 threads,
// V <= 8192, beam <= 8) -- which share their bookkeeping tail (cn_search_commit) and their argument record (SsArgs); the state
// initialisation, the choice of the best beam, greedy_search's masked-logit output, and the masking rule of the searches and of
// the sampling step (dec_sample.h): EOS floor while step < min_pred, forbid-repeat over the row's prefix.
// decode_impl (decoder.hip) fills the record once per decode and picks the kernel.
#pragma once

#define CN_MAX_BEAM 16  // beams 1..8: the register-resident step kernel; 9..16 (BaselinePLM's default is 10, baseline.py:47): the generic one
#define CN_MAX_PRED 64

// What a search step reads and writes, passed by value; `step` is the kernels' other argument.
struct SsArgs {
  float* logits;          // (R, ldv); the generic step masks them in place
  const uint8_t* forbid;  // (V) or null
  int* n_active;          // (B) rows of the clip still searching
  int* slot;              // (R) the output slot a row's hypothesis will land in
  float* sum_lp;          // (R) running sums
  int* prefix;            // (R, maxp + 1)
  int* anc;               // (R, maxp) ancestor row (within the clip) of every cached step
  int* cur_tok;           // (R)
  int* out_preds;         // (R, maxp)
  float* out_avg;         // (R)
  int* out_len;           // (R)
  int* trace_sel;         // (maxp, R, 2) or null
  float* trace_val;       // (maxp, R) or null
  int* live;              // [step + 1] += rows that search on
  float* margins;         // (B, 2, maxp + 1) or null
  int ldv, V, beam, maxp, min_pred, eos_id;
  int dbg;                // phase stamps of the register-resident step (0 outside a CN_G2_PROF build)
};

// ---- the masking rule ---------------------------------------------------------------------------------------------------------
// Global-memory form: logit v of a row whose prefix (positions 0..step) is in s_prefix, EOS floor (beam.py:129-130) and
// forbid-repeat (beam.py:146-156) applied.
__device__ __forceinline__ float cn_masked_logit(const float* lg, int v, int step, int min_pred, int eos_id, const uint8_t* forbid,
                                                 const int* s_prefix) {
  float x = lg[v];
  if (step < min_pred && v == eos_id) x = -INFINITY;
  if (forbid != nullptr && forbid[v] != 0) {
    bool seen = false;
    for (int j = 0; j <= step; ++j) seen |= s_prefix[j] == v;
    if (seen) x = -INFINITY;
  }
  return x;
}
// Register form: thread tid of THREADS owns logit sl * THREADS + tid in val[sl], fb[sl] = that token is forbidden to repeat.
// The test on the token's wave is a wave-uniform early-out: only the owner wave looks closer.  The slabs are written as
// selects, not as stores under a condition: through the array references the compiler merges conditional stores into one store
// to a computed slab, which puts the caller's registers into scratch memory.
template <int THREADS, int VPT>
__device__ __forceinline__ void cn_mask_registers(float (&val)[VPT], const bool (&fb)[VPT], const int* s_prefix, int step,
                                                  int min_pred, int eos_id, int tid, int wv) {
  static_assert(THREADS == 1024, "a token's slab is tok >> 10");
  for (int j = 0; j <= step; ++j) {
    const int tok = s_prefix[j];
    if ((((unsigned)tok & (THREADS - 1)) >> 6) == (unsigned)wv) {
      if ((tok & (THREADS - 1)) == tid) {
#pragma unroll
        for (int sl = 0; sl < VPT; ++sl) val[sl] = (sl == (tok >> 10) && fb[sl]) ? -INFINITY : val[sl];
      }
    }
  }
  if (step < min_pred && (eos_id & (THREADS - 1)) == tid) {
#pragma unroll
    for (int sl = 0; sl < VPT; ++sl) val[sl] = sl == (eos_id >> 10) ? -INFINITY : val[sl];
  }
}

__global__ void cn_init_state_kernel(int B, int beam, int maxp, const int* __restrict__ bos, int* n_active, int* slot,
                                     float* sum_lp, int* prefix, int* anc, int* cur_tok, int* out_preds,
                                     float* out_avg, int* out_len, int* sizes, int pad_id, int* trace_sel,
                                     float* trace_val, int* live, float* margins) {
  const int R = B * beam;
  const int gid = blockIdx.x * blockDim.x + threadIdx.x, gsz = gridDim.x * blockDim.x;
  for (int i = gid; i < CN_MAX_PRED + 2; i += gsz) live[i] = 0;
  for (int i = gid; i < B; i += gsz) n_active[i] = beam;
  for (int i = gid; i < R; i += gsz) {
    slot[i] = i % beam;
    sum_lp[i] = 0.f;
    cur_tok[i] = bos[i / beam];
    out_avg[i] = 0.f;
    out_len[i] = 0;
  }
  for (int i = gid; i < R * (maxp + 1); i += gsz) prefix[i] = (i % (maxp + 1)) == 0 ? bos[i / ((maxp + 1) * beam)] : pad_id;
  for (int i = gid; i < R * maxp; i += gsz) {
    anc[i] = 0;
    out_preds[i] = pad_id;
  }
  if (gid < 2) sizes[gid] = 0;
  if (trace_sel)
    for (int i = gid; i < maxp * R * 2; i += gsz) trace_sel[i] = -1;
  if (trace_val)
    for (int i = gid; i < maxp * R; i += gsz) trace_val[i] = 0.f;
  if (margins)  // a step a clip does not take (it has finished) decides nothing: +inf
    for (int i = gid; i < B * 2 * (maxp + 1); i += gsz) margins[i] = INFINITY;
}

struct ValIdx {
  float v;
  int i;
};
__device__ __forceinline__ ValIdx vi_better(ValIdx a, ValIdx b) {  // larger value, then lower flat index
  return (b.v > a.v || (b.v == a.v && b.i < a.i)) ? b : a;
}
template <int CTRL> __device__ __forceinline__ ValIdx vi_dpp_step(ValIdx x) {
  return vi_better(x, ValIdx{cn_dpp<CTRL>(x.v), cn_dpp<CTRL>(x.i)});
}
// same result as vi_wave (the order relation is total), 4 of the 6 exchange steps on DPP
__device__ __forceinline__ ValIdx vi_wave_dpp(ValIdx x) {
  x = vi_dpp_step<0xB1>(x);
  x = vi_dpp_step<0x4E>(x);
  x = vi_dpp_step<0x141>(x);
  x = vi_dpp_step<0x140>(x);
#pragma unroll
  for (int o = 16; o <= 32; o <<= 1) {
    ValIdx y;
    y.v = __shfl_xor(x.v, o);
    y.i = __shfl_xor(x.i, o);
    x = vi_better(x, y);
  }
  return x;
}
__device__ __forceinline__ ValIdx vi_wave(ValIdx x) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    ValIdx y;
    y.v = __shfl_xor(x.v, o);
    y.i = __shfl_xor(x.i, o);
    x = vi_better(x, y);
  }
  return x;
}

// The effective margin of one top-k call (round 6, precision "certified"): how far the call is from ANY other outcome -- the gap
// between the last pick and the first rejected candidate, and the gaps between consecutive picks (their order decides which
// hypothesis lands in which slot: beam.py:165-169).  A 16-bit search whose every call (and whose final best-beam choice) has a
// margin above twice the precision's worst candidate error has taken the decisions an exact search takes.
// Two planes per clip, (B, 2, max_pred + 1): plane 0 = MEMBERSHIP, the gap that decides WHICH candidates continue (and, in its last
// column, which hypothesis is returned as the best); plane 1 = ORDER, the smallest gap between consecutive picks, which only decides
// which slot a hypothesis lands in -- the order of mult_preds, never best_preds.
__device__ __forceinline__ void cn_step_margin(float* margins, int b, int maxp, int step, const float* selv, int k, float runner_up) {
  float* row = margins + (size_t)b * 2 * (maxp + 1);
  row[step] = selv[k - 1] - runner_up;   // NaN (-inf - -inf: fewer finite candidates than picks) reads as "not certified" on the host
  float m = INFINITY;
  for (int c = 0; c + 1 < k; ++c) m = fminf(m, selv[c] - selv[c + 1]);
  row[(maxp + 1) + step] = m;
}

// The bookkeeping of a step (beam.py:164-203), by a block of THREADS threads that has the clip's k picks in s_selv / s_self
// (value, flat index parent * V + token) and its old state in s_prefix / s_anc / s_slot: the trace, the rows that search on
// (n_active, live), finished hypotheses to their slot, continuing rows' prefix / anc / sum_lp / slot / cur_tok.
// The diverse search (dec_group.h) commits one beam group at a time: the group's rows start at row `row0` of the clip (the LDS
// arrays are passed from there, parents in s_self count from there, slots are within-clip indices) and its live-row count is
// n_active[na]; the plain searches commit the whole clip (row0 = 0, n_active[b]).
template <int THREADS>
__device__ __forceinline__ void cn_search_commit(const SsArgs& a, int b, int k, int step, const float* s_selv, const int* s_self,
                                                 const int (*s_prefix)[CN_MAX_PRED + 1], const int (*s_anc)[CN_MAX_PRED],
                                                 const int* s_slot, int* s_newpos, const int row0 = 0, const int na = -1) {
  const int tid = threadIdx.x, V = a.V, maxp = a.maxp, rb = b * a.beam + row0;
  if (tid < k) {
    const size_t ti = ((size_t)step * gridDim.x + b) * a.beam + row0 + tid;
    if (a.trace_sel) {
      a.trace_sel[2 * ti] = row0 + s_self[tid] / V;
      a.trace_sel[2 * ti + 1] = s_self[tid] % V;
    }
    if (a.trace_val) a.trace_val[ti] = s_selv[tid];
  }
  if (tid == 0) {
    int cnt = 0;
    for (int c = 0; c < k; ++c) {
      const int token = s_self[c] % V;
      const bool fin = (token == a.eos_id) || (step == maxp - 1);
      s_newpos[c] = fin ? -1 : cnt++;
    }
    a.n_active[na < 0 ? b : na] = cnt;
    if (cnt > 0) atomicAdd(&a.live[step + 1], cnt);  // rows that search on: gates the next step's kernels
  }
  __syncthreads();
  for (int c = 0; c < k; ++c) {
    const int flat = s_self[c];
    const int parent = flat / V, token = flat % V;
    const int np = s_newpos[c];
    if (np < 0) {  // finished: write to the slot of this row position
      const int sl = b * a.beam + s_slot[c];
      for (int j = tid; j <= step; j += THREADS) a.out_preds[(size_t)sl * maxp + j] = (j == step) ? token : s_prefix[parent][j + 1];
      if (tid == 0) {
        a.out_avg[sl] = s_selv[c] / (float)(step + 1);
        a.out_len[sl] = step + 1;
      }
    } else {
      const int dst = rb + np;
      for (int j = tid; j <= step + 1; j += THREADS) a.prefix[(size_t)dst * (maxp + 1) + j] = (j == step + 1) ? token : s_prefix[parent][j];
      for (int j = tid; j <= step; j += THREADS) a.anc[(size_t)dst * maxp + j] = (j == step) ? row0 + parent : s_anc[parent][j];
      if (tid == 0) {
        a.sum_lp[dst] = s_selv[c];
        a.slot[dst] = s_slot[c];
        a.cur_tok[dst] = token;
      }
    }
  }
}

__global__ __launch_bounds__(256) void cn_search_step_kernel(const SsArgs a, const int step) {
  __shared__ float s_red[8];
  __shared__ ValIdx s_vi[4];
  __shared__ float s_mx[CN_MAX_BEAM], s_lg[CN_MAX_BEAM], s_base[CN_MAX_BEAM];
  __shared__ float s_selv[CN_MAX_BEAM + 1];
  __shared__ int s_self[CN_MAX_BEAM + 1];
  __shared__ int s_prefix[CN_MAX_BEAM][CN_MAX_PRED + 1];
  __shared__ int s_anc[CN_MAX_BEAM][CN_MAX_PRED];
  __shared__ int s_slot[CN_MAX_BEAM];
  __shared__ int s_newpos[CN_MAX_BEAM];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int ldv = a.ldv, V = a.V, maxp = a.maxp;
  const int k = a.n_active[b];
  if (k == 0) return;
  const int rb = b * a.beam;
  const int nrows = step == 0 ? 1 : k;

  // old state -> LDS
  for (int i = tid; i < k * (maxp + 1); i += 256) s_prefix[i / (maxp + 1)][i % (maxp + 1)] = a.prefix[(size_t)rb * (maxp + 1) + i];
  for (int i = tid; i < k * maxp; i += 256) s_anc[i / maxp][i % maxp] = a.anc[(size_t)rb * maxp + i];
  if (tid < k) {
    s_slot[tid] = a.slot[rb + tid];
    s_base[tid] = step == 0 ? 0.f : a.sum_lp[rb + tid];
  }
  __syncthreads();
  // EOS floor (beam.py:129-130) + forbid-repeat (beam.py:146-156), in place: a loop over prefix positions, not over the vocabulary
  for (int i = tid; i < nrows * (step + 2); i += 256) {
    const int p = i / (step + 2), j = i % (step + 2);
    float* lg = a.logits + (size_t)(rb + p) * ldv;
    if (j == step + 1) {
      if (step < a.min_pred) lg[a.eos_id] = -INFINITY;
    } else if (a.forbid != nullptr) {
      const int tok = s_prefix[p][j];
      if (a.forbid[tok]) lg[tok] = -INFINITY;
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
  // top-k over the nrows * V candidates, k rounds of block arg-max (ties -> lowest flat index); with a margin output one
  // more round finds the first rejected candidate
  for (int c = 0; c < k + (a.margins != nullptr ? 1 : 0); ++c) {
    ValIdx best{-INFINITY, 0x7fffffff};
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
      ValIdx r0 = vi_better(vi_better(s_vi[0], s_vi[1]), vi_better(s_vi[2], s_vi[3]));
      s_selv[c] = r0.v;
      s_self[c] = r0.i;
    }
    __syncthreads();
  }
  if (a.margins != nullptr && tid == 0) cn_step_margin(a.margins, b, maxp, step, s_selv, k, s_selv[k]);
  cn_search_commit<256>(a, b, k, step, s_selv, s_self, s_prefix, s_anc, s_slot, s_newpos);
}

// Same step, register path (V <= 8192): 1024 threads per clip, every thread keeps its <= 8 logits of each live row
// in registers (one coalesced pass over the logits, nothing staged in LDS: the kernel starts on any CU with a free
// workgroup slot while the encoder's blocks hold the LDS), block reductions for the log-softmax, per-thread sorted
// top-k, then a two-level merge: k rounds of wave arg-max inside each wave, and the 16 x k wave winners merged
// redundantly by every wave.  Ties resolve to the lowest flat index exactly like the kernels above.
#define S3_T 1024
#define S3_VPT 8  // most logits per thread: V <= 8192
__device__ unsigned long long g_s3_prof[16];
#define S3_STAMP(i)                                            \
  if (dbg) {                                                   \
    const unsigned long long t_ = wall_clock64();              \
    if (tid == 0 && b == 0) atomicAdd(&g_s3_prof[i], t_ - t_prev); \
    t_prev = t_;                                               \
  }
template <int NR, int VPT>
__global__ __launch_bounds__(S3_T) void cn_search_step3_kernel(const SsArgs a, const int step) {
  __shared__ float s_redm[NR][16], s_reds[NR][16];
  __shared__ float s_ru[16];
  __shared__ ValIdx s_cand[16][CN_MAX_BEAM];
  __shared__ float s_base[CN_MAX_BEAM];
  __shared__ float s_selv[CN_MAX_BEAM];
  __shared__ int s_self[CN_MAX_BEAM];
  __shared__ int s_prefix[CN_MAX_BEAM][CN_MAX_PRED + 1];
  __shared__ int s_anc[CN_MAX_BEAM][CN_MAX_PRED];
  __shared__ int s_slot[CN_MAX_BEAM];
  __shared__ int s_newpos[CN_MAX_BEAM];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int ldv = a.ldv, V = a.V, beam = a.beam, maxp = a.maxp, dbg = a.dbg;
  unsigned long long t_prev = dbg ? wall_clock64() : 0ull;
  const int rb = b * beam;
  // every global read is issued up front and none depends on another (rows that turn out to be dead are read
  // and ignored): the step is a chain of dependent launches, a second round trip costs more than the bytes
  const int k_ld = a.n_active[b];
  const int rows_ld = step == 0 ? 1 : beam;
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
      val[p][sl] = (p < rows_ld && v < V) ? a.logits[(size_t)(rb + p) * ldv + v] : -INFINITY;
    }
  for (int i = tid; i < beam * (maxp + 1); i += S3_T) s_prefix[i / (maxp + 1)][i % (maxp + 1)] = a.prefix[(size_t)rb * (maxp + 1) + i];
  for (int i = tid; i < beam * maxp; i += S3_T) s_anc[i / maxp][i % maxp] = a.anc[(size_t)rb * maxp + i];
  if (tid < beam) {
    s_slot[tid] = a.slot[rb + tid];
    s_base[tid] = step == 0 ? 0.f : a.sum_lp[rb + tid];
  }
  const int k = k_ld;
  if (k == 0) return;
  S3_STAMP(0)
  const int nrows = step == 0 ? 1 : k;
  __syncthreads();
  S3_STAMP(1)
  // forbid-repeat over the row's prefix and EOS floor, on the owner's registers
#pragma unroll
  for (int p = 0; p < NR; ++p)
    if (p < nrows) cn_mask_registers<S3_T>(val[p], fb, s_prefix[p], step, a.min_pred, a.eos_id, tid, wv);
  S3_STAMP(2)
  // log-softmax statistics of every live row
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
  S3_STAMP(3)
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
  S3_STAMP(4)
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
  S3_STAMP(5)
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
  S3_STAMP(6)
  if (a.margins != nullptr) {  // the first rejected candidate: the best of everything the k picks left (same expression, same bits)
    float ru = -INFINITY;
#pragma unroll
    for (int p = 0; p < NR; ++p)
      if (p < nrows) {
        const float base = s_base[p];
#pragma unroll
        for (int sl = 0; sl < VPT; ++sl) {
          const int v = sl * S3_T + tid;
          float cand = (val[p][sl] - rmx[p]) - rlg[p];
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
  S3_STAMP(7)
  if (dbg && tid == 0 && b == 0) atomicAdd(&g_s3_prof[9], 1ull);
}

// best beam per clip (beam.py:205-220): first max of the averaged log-prob; pred_size via atomicMax
__global__ void cn_finalize_kernel(int B, int beam, int maxp, int eos_id, const int* __restrict__ out_preds,
                                   const float* __restrict__ out_avg, const int* __restrict__ out_len,
                                   int* __restrict__ best_preds, float* __restrict__ best_lp,
                                   int* __restrict__ eos_idx, int* sizes, float* __restrict__ margins) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  int best = 0, mlen = 0;
  float bv = out_avg[b * beam];
  for (int s = 0; s < beam; ++s) {
    if (out_avg[b * beam + s] > bv) {
      bv = out_avg[b * beam + s];
      best = s;
    }
    mlen = max(mlen, out_len[b * beam + s]);
  }
  atomicMax(&sizes[0], mlen);
  best_lp[b] = bv;
  if (margins) {  // how far the best hypothesis is from the second best (beam.py:214-217 takes the first maximum)
    float second = -INFINITY;
    for (int s = 0; s < beam; ++s)
      if (s != best) second = fmaxf(second, out_avg[b * beam + s]);
    margins[(size_t)b * 2 * (maxp + 1) + maxp] = bv - second;
  }
  int e = -1;
  for (int j = 0; j < maxp; ++j) {
    const int t = out_preds[((size_t)b * beam + best) * maxp + j];
    best_preds[(size_t)b * maxp + j] = t;
    if (e < 0 && t == eos_id) e = j;
  }
  eos_idx[b] = e;
}
// best_maxlen = max_b(first EOS index, or pred_size when absent) + 1 (beam.py:222-225)
__global__ void cn_finalize2_kernel(int B, const int* __restrict__ eos_idx, int* sizes) {
  __shared__ int s_m;
  if (threadIdx.x == 0) s_m = 0;
  __syncthreads();
  const int ps = sizes[0];
  int m = 0;
  for (int b = threadIdx.x; b < B; b += blockDim.x) {
    const int e = eos_idx[b];
    m = max(m, (e >= 0 && e < ps) ? e : ps);
  }
  atomicMax(&s_m, m);
  __syncthreads();
  if (threadIdx.x == 0) sizes[1] = min(s_m + 1, ps);
}

// ---- greedy_search's full-logit output (nn/decoding/greedy.py:17-131): the step's logits of every unfinished clip
// with the EOS floor (:96-97) and the forbid-repeat mask (:99-105) applied, (-inf, pad_id -> 0) for finished clips (:64-69).
// beam == 1: rows == clips; runs before the search step updates prefix / n_active.
__global__ __launch_bounds__(256) void cn_greedy_logits_kernel(const SsArgs a, const int step, int pad_id, float* __restrict__ out) {
  __shared__ int s_tok[CN_MAX_PRED + 1];
  const int b = blockIdx.y, V = a.V, maxp = a.maxp;
  const bool active = a.n_active[b] > 0;
  for (int j = threadIdx.x; j <= step; j += 256) s_tok[j] = a.prefix[(size_t)b * (maxp + 1) + j];
  __syncthreads();
  float* o = out + ((size_t)b * maxp + step) * V;
  for (int v = blockIdx.x * 256 + threadIdx.x; v < V; v += gridDim.x * 256)
    o[v] = active ? cn_masked_logit(a.logits + (size_t)b * a.ldv, v, step, a.min_pred, a.eos_id, a.forbid, s_tok)
                  : (v == pad_id ? 0.f : -INFINITY);
}
