// One sampling decision per row per step: temperature, top-k and nucleus (top-p) sampling over the fp32 logits the classifier
// GEMM leaves in the workspace (conette_sample, include/conette_hip.h; the CPU restatement of the rule is conette_amd/sampling.py).
//
// Rows = clips x samples.  A row never changes its parent, so the step is row-local: one block of 1024 threads per row.
//   masks      EOS floor while step < min_pred, forbid-repeat over the row's prefix -- the searches' rule (dec_search.h)
//   log-prob   log_softmax(masked z)[token] at temperature 1, unfiltered: (z_t - max) - log(sum exp(z - max))
//   top-k      v kept iff fewer than k tokens have a strictly larger logit      = key(v) >= the k-th largest key
//   top-p      v kept iff the mass of the strictly larger logits is < p         = key(v) >= the largest t with mass(key >= t) >= p * S
//   draw       the first kept token, in ascending id, whose running sum of e = exp((z - max) / T) exceeds u * (sum over the kept)
// Both thresholds are selections by VALUE, found by a bitwise search over the order-preserving integer image of the floats (32
// block-wide counts / sums each; skipped when the filter is off).  The order is taken on z, not on z / T: division by T > 0 keeps
// the order of the reals, and two logits one ulp apart must not become a tie.  Every block-wide sum has a fixed order -- wave DPP
// reduction, then the 16 wave partials added in sequence -- and a subset sum of non-negative terms in a fixed order is monotone in
// the subset, which is what the bitwise search of top-p needs.  No float atomics: results are bit-identical from run to run.
//
// Register variant (V <= 8192): one coalesced pass, every thread keeps its <= 8 logits; all global reads are issued up front; LDS
// holds reduction scratch only.  Generic variant (VPT = 0, V <= 65536): the same code re-reading (and re-masking) the logits from
// global memory in every phase.
#pragma once

#include "dec_search.h"

#define SM_T 1024
#define SM_VPT 8          // most logits per thread of the register variant: V <= 8192
#define SM_MAX_SLABS 64   // generic variant: slabs of 1024 ids

struct SmArgs {
  const float* logits;  // (R, ldv)
  const uint8_t* forbid;  // (V) or null
  const float* uniforms;  // (maxp, R) step-major
  int* prefix;            // (R, maxp + 1)
  int* cur_tok;           // (R)
  float* sum_lp;          // (R) running sums (workspace)
  int* fin;               // (R) 1 = the row has finished
  int* live;              // [step + 1] += rows that sample on
  int32_t* preds;         // (R, maxp)
  float* sum_out;         // (R)
  int32_t* lens;          // (R)
  int32_t* sizes;         // (2)
  float* tok_lp;          // (R, maxp) or null
  float* step_logits;     // (R, maxp, V) or null
  int ldv, V, R, maxp, min_pred, eos_id, top_k;
  float temperature, top_p;
};

// every row is its own ancestor; nothing has finished; per-token outputs are 0 after the end
__global__ void cn_sample_init_kernel(int R, int n, int maxp, int* __restrict__ anc, int* __restrict__ fin,
                                      int32_t* __restrict__ lens, float* __restrict__ tok_lp) {
  const int gid = blockIdx.x * blockDim.x + threadIdx.x, gsz = gridDim.x * blockDim.x;
  for (int i = gid; i < R * maxp; i += gsz) {
    anc[i] = (i / maxp) % n;
    if (tok_lp) tok_lp[i] = 0.f;
  }
  for (int i = gid; i < R; i += gsz) {
    fin[i] = 0;
    lens[i] = 0;
  }
}

// order-preserving image of a float: a < b (as floats, -0 folded into +0 by the caller) <=> key(a) < key(b)
__device__ __forceinline__ unsigned sm_key(float x) {
  const unsigned u = __float_as_uint(x);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ int sm_wave_sum_i(int v) {
  v += cn_dpp<0xB1>(v);
  v += cn_dpp<0x4E>(v);
  v += cn_dpp<0x141>(v);
  v += cn_dpp<0x140>(v);
  v += __shfl_xor(v, 16);
  v += __shfl_xor(v, 32);
  return v;
}
// Block reductions over 16 waves through a double-buffered LDS line: call i uses line i & 1, which was last read before the
// barrier of call i - 1, so one barrier per call is enough.  The 16 partials are combined in sequence by every thread.
struct SmRed {
  unsigned (*buf)[16];
  int it, lane, wv;
  __device__ __forceinline__ float sum(float x) {
    x = cn_wave_sum_dpp(x);
    unsigned* b = buf[it++ & 1];
    if (lane == 0) b[wv] = __float_as_uint(x);
    __syncthreads();
    float s = __uint_as_float(b[0]);
#pragma unroll
    for (int w = 1; w < 16; ++w) s += __uint_as_float(b[w]);
    return s;
  }
  __device__ __forceinline__ float max(float x) {
    x = cn_wave_max_dpp(x);
    unsigned* b = buf[it++ & 1];
    if (lane == 0) b[wv] = __float_as_uint(x);
    __syncthreads();
    float s = __uint_as_float(b[0]);
#pragma unroll
    for (int w = 1; w < 16; ++w) s = fmaxf(s, __uint_as_float(b[w]));
    return s;
  }
  __device__ __forceinline__ int sum(int x) {
    x = sm_wave_sum_i(x);
    unsigned* b = buf[it++ & 1];
    if (lane == 0) b[wv] = (unsigned)x;
    __syncthreads();
    int s = (int)b[0];
#pragma unroll
    for (int w = 1; w < 16; ++w) s += (int)b[w];
    return s;
  }
  __device__ __forceinline__ int max(int x) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x = ::max(x, __shfl_xor(x, o));
    unsigned* b = buf[it++ & 1];
    if (lane == 0) b[wv] = (unsigned)x;
    __syncthreads();
    int s = (int)b[0];
#pragma unroll
    for (int w = 1; w < 16; ++w) s = ::max(s, (int)b[w]);
    return s;
  }
};

template <int VPT>
__global__ __launch_bounds__(SM_T) void cn_sample_step_kernel(const SmArgs a, const int step) {
  constexpr bool REG = VPT > 0;
  constexpr int NV = REG ? VPT : 1;
  constexpr int NSL = REG ? VPT : SM_MAX_SLABS;
  __shared__ unsigned s_red[2][16];
  __shared__ float s_wt[NSL][16];    // draw: total of e per (slab of 1024 ids, wave)
  __shared__ float s_wb[NSL][16];    //       exclusive running sum of the waves inside their slab
  __shared__ float s_st[NSL];        //       slab totals
  __shared__ int s_prefix[CN_MAX_PRED + 1];
  const int r = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int V = a.V, maxp = a.maxp, eos = a.eos_id;
  const int nsl = REG ? VPT : (V + SM_T - 1) / SM_T;
  const float* lg = a.logits + (size_t)r * a.ldv;
  SmRed red{s_red, 0, lane, wv};

  // every global read is issued up front, none depends on another
  float val[NV];
  bool fb[NV];
  if constexpr (REG) {
#pragma unroll
    for (int sl = 0; sl < VPT; ++sl) {
      const int v = sl * SM_T + tid;
      fb[sl] = a.forbid != nullptr && v < V && a.forbid[v] != 0;
      val[sl] = v < V ? lg[v] : -INFINITY;
    }
  }
  const float u = a.uniforms[(size_t)step * a.R + r];
  const int fin = a.fin[r];
  const float sum_prev = step == 0 ? 0.f : a.sum_lp[r];
  if (tid <= step) s_prefix[tid] = a.prefix[(size_t)r * (maxp + 1) + tid];
  if (fin) return;  // (block-uniform)
  if (a.step_logits) {  // the RAW logits this decision sees
    float* o = a.step_logits + ((size_t)r * maxp + step) * V;
    if constexpr (REG) {
#pragma unroll
      for (int sl = 0; sl < VPT; ++sl)
        if (sl * SM_T + tid < V) o[sl * SM_T + tid] = val[sl];
    } else {
      for (int v = tid; v < V; v += SM_T) o[v] = lg[v];
    }
  }
  __syncthreads();
  if constexpr (REG) {  // forbid-repeat over the prefix (position 0 included) and the EOS floor, on the owner's registers
    cn_mask_registers<SM_T>(val, fb, s_prefix, step, a.min_pred, eos, tid, wv);
#pragma unroll
    for (int sl = 0; sl < VPT; ++sl) val[sl] += 0.f;  // -0 -> +0: equal floats, equal keys
  }
  // the masked logit of this thread's token of slab sl
  auto Z = [&](int sl) -> float {
    if constexpr (REG) {
      return val[sl];
    } else {
      const int v = sl * SM_T + tid;
      if (v >= V) return -INFINITY;
      return cn_masked_logit(lg, v, step, a.min_pred, eos, a.forbid, s_prefix) + 0.f;
    }
  };
#define SM_FOR(sl) _Pragma("unroll") for (int sl = 0; sl < (REG ? VPT : nsl); ++sl)

  // log-soft-max statistics at temperature 1
  float mx = -INFINITY;
  SM_FOR(sl) mx = fmaxf(mx, Z(sl));
  mx = red.max(mx);
  int tok;
  float lp;
  bool owner;
  // No finite logit, or a +inf in the row: <eos>, NaN, finished.  (fmaxf drops NaN: a NaN beside finite logits takes the normal path,
  // where it is never kept -- its comparisons are false -- so the token is a valid id and the log-prob NaN through the log-sum-exp.)
  if (!(mx > -INFINITY) || !(mx < INFINITY)) {
    tok = eos;
    lp = __uint_as_float(0x7fc00000u);
    owner = tid == 0;
  } else {
    float sm = 0.f;
    SM_FOR(sl) sm += __expf(Z(sl) - mx);
    const float lse = logf(red.sum(sm));

    // top-k: the k-th largest key (with multiplicity) = the largest t that at least k keys reach
    unsigned thr = 0u;
    if (a.top_k > 0 && a.top_k < V) {
      for (int bit = 31; bit >= 0; --bit) {
        const unsigned cand = thr | (1u << bit);
        int c = 0;
        SM_FOR(sl) c += sm_key(Z(sl)) >= cand ? 1 : 0;
        if (red.sum(c) >= a.top_k) thr = cand;
      }
    }
    // e = exp(y - max y) over the kept set, y = z / T
    const float T = a.temperature;
    auto E = [&](int sl, unsigned t) -> float {
      const float z = Z(sl);
      return (z > -INFINITY && sm_key(z) >= t) ? __expf((z - mx) / T) : 0.f;
    };
    if (a.top_p < 1.f) {  // top-p: the largest t whose upper mass reaches p * S
      float s = 0.f;
      SM_FOR(sl) s += E(sl, thr);
      const float need = a.top_p * red.sum(s);
      unsigned t = 0u;
      for (int bit = 31; bit >= 0; --bit) {
        const unsigned cand = t | (1u << bit);
        float f = 0.f;
        SM_FOR(sl) f += E(sl, cand > thr ? cand : thr);
        if (red.sum(f) >= need) t = cand;
      }
      thr = t > thr ? t : thr;
    }
    // draw: running sum in ascending id = slab base + wave base + inclusive lane scan
    SM_FOR(sl) {
      const float w = cn_wave_sum_dpp(E(sl, thr));
      if (lane == 0) s_wt[sl][wv] = w;
    }
    __syncthreads();
    if (tid < nsl) {
      float acc = 0.f;
#pragma unroll
      for (int w = 0; w < 16; ++w) {
        s_wb[tid][w] = acc;
        acc += s_wt[tid][w];
      }
      s_st[tid] = acc;
    }
    __syncthreads();
    float total = 0.f;
    for (int sl = 0; sl < nsl; ++sl) total += s_st[sl];
    const float target = u * total;
    int first = 0x7fffffff, last = -1;
    float sb = 0.f;
    SM_FOR(sl) {
      const float e = E(sl, thr);
      const float z = Z(sl);
      const int v = sl * SM_T + tid;
      if (z > -INFINITY && sm_key(z) >= thr) last = v;  // (ids ascend with sl)
      float c = e;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const float t = __shfl_up(c, o);
        if (lane >= o) c += t;
      }
      c = (sb + s_wb[sl][wv]) + c;
      if (e > 0.f && c > target && first == 0x7fffffff) first = v;
      sb += s_st[sl];
    }
    first = -red.max(-first);
    last = red.max(last);
    tok = first != 0x7fffffff ? first : (last >= 0 ? last : eos);  // rounding left the total <= u * total: the largest kept id
    owner = (tok & (SM_T - 1)) == tid;
    lp = 0.f;
    if (owner) {
      float zt = -INFINITY;
      if constexpr (REG) {
#pragma unroll
        for (int sl = 0; sl < VPT; ++sl)
          if (sl == (tok >> 10)) zt = val[sl];
      } else {
        zt = Z(tok >> 10);
      }
      lp = (zt - mx) - lse;
    }
  }
#undef SM_FOR
  if (owner) {  // bookkeeping of the row, by one thread
    const bool done = tok == eos || step == maxp - 1;
    a.preds[(size_t)r * maxp + step] = tok;
    if (a.tok_lp) a.tok_lp[(size_t)r * maxp + step] = lp;
    const float s = step == 0 ? lp : sum_prev + lp;
    a.sum_lp[r] = s;
    a.sum_out[r] = s;
    a.prefix[(size_t)r * (maxp + 1) + step + 1] = tok;
    a.cur_tok[r] = tok;
    if (done) {
      a.fin[r] = 1;
      a.lens[r] = step + 1;
      atomicMax(&a.sizes[0], step + 1);
      atomicMax(&a.sizes[1], step + 1);
    } else {
      atomicAdd(&a.live[step + 1], 1);  // rows that sample on: gates the next step's kernels
    }
  }
}
