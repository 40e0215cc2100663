// Caption scoring: classifier GEMM + log-sum-exp + target gather in one kernel (conette_score, decoder.hip).
//
//   lp[r] = logit[r][targets[r]] - logsumexp_v logit[r][:],    logit[r][v] = xt[r][:] . cls_w[v][:] + cls_b[v]
//
// The (R, V) logits never exist: a block owns SC_BM = 64 rows of xt, keeps them in LDS for its whole life (K is always 256:
// 32 KB of 16-bit operands, 64 KB of fp32 / sp16 ones) and walks the vocabulary in N-tiles of SC_BN = 128 columns itself;
// only cls_w streams through, in k-tiles of 128 bytes per row, register-staged and double buffered as in cn_gemm_nt_kernel
// (gemm.h), one barrier per k-tile.  The accumulators have that kernel's layout -- a lane holds one row m = lane & 15 of
// a 16 x 16 tile and four consecutive columns 4 * (lane >> 4) -- so after the last k-tile of an N-tile every lane folds its
// own 16 columns per row into a LANE-PRIVATE running state (max, sum of exp(z - max), target logit; fp32, online rescale),
// and the state is combined only once, when the block has walked its slab: lanes l, l + 16, l + 32, l + 48 by two
// exchanges, the two `wn` waves through LDS.
//   * the target is found by comparing the column index with targets[r] -- it is never an address;
//   * columns n >= V of the last N-tile are masked BY INDEX (the loader clamps their row of cls_w to V - 1);
//   * blockIdx.y = vocabulary slab: with few rows one row-tile per block would leave the chip empty, so the N-tiles are
//     dealt to S slabs and the (R, S, 3) partial states go to the workspace; cn_score_merge_kernel combines them in slab
//     order (bit-identical from run to run), turns them into log-probabilities and sums each caption's.
#pragma once
#include "gemm2.h"

#define SC_BM 64
#define SC_BN 128
#define SC_MAX_AUTO_SLABS 21  // automatic split: at most 21 slabs of 12 bytes = 252 bytes of partials per row

// gemm.h's pieces for the other operand types.  A staged k-tile is 128 bytes of a row for every type (pitch 128 + 16):
// 32 fp32 or sp16 elements, 64 bf16 / fp16 ones; a "fragment" is what one lane feeds the MFMAs of one k-tile.
template <> struct GemmTraits<bf16_t> { static constexpr int ROW_BYTES = 128 + 16; static constexpr int CPR = 8; };
template <> struct GemmTraits<half_t> { static constexpr int ROW_BYTES = 128 + 16; static constexpr int CPR = 8; };
template <> struct GemmTraits<sp16_t> { static constexpr int ROW_BYTES = 128 + 16; static constexpr int CPR = 8; };
template <> struct Frag8<bf16_t> { struct type { cn_h8<bf16_t> lo, hi; }; };  // k-steps 0 and 1 (32 elements each)
template <> struct Frag8<half_t> { struct type { cn_h8<half_t> lo, hi; }; };
template <> struct Frag8<sp16_t> { struct type { f16x8 hi, lo; }; };          // the hi and lo halves of 8 elements
template <> __device__ __forceinline__ Frag8<bf16_t>::type cn_lds_frag<bf16_t>(const char* p) {
  Frag8<bf16_t>::type f;
  f.lo = *(const cn_h8<bf16_t>*)p;
  f.hi = *(const cn_h8<bf16_t>*)(p + 64);
  return f;
}
template <> __device__ __forceinline__ Frag8<half_t>::type cn_lds_frag<half_t>(const char* p) {
  Frag8<half_t>::type f;
  f.lo = *(const cn_h8<half_t>*)p;
  f.hi = *(const cn_h8<half_t>*)(p + 64);
  return f;
}
template <> __device__ __forceinline__ Frag8<sp16_t>::type cn_lds_frag<sp16_t>(const char* p) {
  Frag8<sp16_t>::type f;
  cn_sp_split(*(const u32x4*)p, *(const u32x4*)(p + 16), f.hi, f.lo);
  return f;
}
__device__ __forceinline__ f32x4 cn_mma(const Frag8<bf16_t>::type& a, const Frag8<bf16_t>::type& b, f32x4 c) {
  return cn_mma16(a.hi, b.hi, cn_mma16(a.lo, b.lo, c));
}
__device__ __forceinline__ f32x4 cn_mma(const Frag8<half_t>::type& a, const Frag8<half_t>::type& b, f32x4 c) {
  return cn_mma16(a.hi, b.hi, cn_mma16(a.lo, b.lo, c));
}
// sp16: lo.hi + hi.lo + hi.hi, smallest terms first (cn_g2_compute_sp)
__device__ __forceinline__ f32x4 cn_mma(const Frag8<sp16_t>::type& w, const Frag8<sp16_t>::type& a, f32x4 c) {
  c = __builtin_amdgcn_mfma_f32_16x16x32_f16(w.lo, a.hi, c, 0, 0, 0);
  c = __builtin_amdgcn_mfma_f32_16x16x32_f16(w.hi, a.lo, c, 0, 0, 0);
  return __builtin_amdgcn_mfma_f32_16x16x32_f16(w.hi, a.hi, c, 0, 0, 0);
}

template <typename T> struct ScoreGeom {
  static constexpr int K = 256;
  static constexpr int KE = 128 / (int)sizeof(T);          // elements per staged k-tile
  static constexpr int KT = K / KE;                        // k-tiles per N-tile
  static constexpr int FRAG_BYTES = CnIsH16<T>::value ? 16 : 32;  // lane group g reads its fragment at g * FRAG_BYTES
  static constexpr int A_PITCH = K * (int)sizeof(T) + 16;  // resident rows: pitch = 4 banks mod 64, 16 rows conflict-free
  static constexpr int A_BYTES = SC_BM * A_PITCH;
  static constexpr int W_BUF = SC_BN * GemmTraits<T>::ROW_BYTES;
  static constexpr int SMEM = A_BYTES + 2 * W_BUF;         // 69 KB (16-bit: two blocks per CU) / 101 KB
};

// running state of one row's soft-max: (m, s) = (max, sum exp(z - max)); (-inf, 0) is the empty state
__device__ __forceinline__ void cn_lse_merge(float& m, float& s, float m2, float s2) {
  const float nm = fmaxf(m, m2);
  const float a = (m == -INFINITY) ? 0.f : s * __expf(m - nm);
  const float b = (m2 == -INFINITY) ? 0.f : s2 * __expf(m2 - nm);
  m = nm;
  s = a + b;
}

// grid (row tiles, S slabs).  part[(r * S + slab) * 3 + {0, 1, 2}] = max, sum, target logit of row r over the slab's columns
template <typename T>
__global__ __launch_bounds__(256) void cn_score_kernel(const T* __restrict__ xt, const T* __restrict__ W,
                                                       const float* __restrict__ bias, const int32_t* __restrict__ targets,
                                                       int R, int V, float* __restrict__ part) {
  typedef ScoreGeom<T> G;
  constexpr int RB = GemmTraits<T>::ROW_BYTES, CPR = GemmTraits<T>::CPR;
  constexpr int EPC = 16 / (int)sizeof(T);
  constexpr int TM = SC_BM / 32, TN = SC_BN / 32;
  constexpr int W_IT = SC_BN * CPR / 256;
  constexpr int A_CPR = G::K / EPC;  // 16-byte chunks per resident row
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* sA = smem;
  char* sWb = smem + G::A_BYTES;

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int m0 = blockIdx.x * SC_BM;
  const int S = gridDim.y, slab = blockIdx.y;
  const int n_tiles = (V + SC_BN - 1) / SC_BN;
  const int t_begin = (int)((long)slab * n_tiles / S), t_end = (int)((long)(slab + 1) * n_tiles / S);  // S <= n_tiles: never empty
  const int steps = (t_end - t_begin) * G::KT;

  // the block's rows, whole K, once
  for (int idx = tid; idx < SC_BM * A_CPR; idx += 256) {
    const int row = idx / A_CPR, ch = idx % A_CPR;
    const int gm = min(m0 + row, R - 1);
    *(uint4*)(sA + row * G::A_PITCH + ch * 16) = *(const uint4*)(xt + (size_t)gm * G::K + ch * EPC);
  }

  u32x4 rw[W_IT];
  auto gload = [&](int step) {
    const int n0 = (t_begin + step / G::KT) * SC_BN, k0 = (step % G::KT) * G::KE;
#pragma unroll
    for (int i = 0; i < W_IT; ++i) {
      const int idx = tid + i * 256;
      const int row = idx / CPR, ch = idx % CPR;
      const int gn = min(n0 + row, V - 1);
      rw[i] = *(const u32x4*)(W + (size_t)gn * G::K + k0 + ch * EPC);
    }
  };
  auto swrite = [&](int buf) {
    char* sW = sWb + buf * G::W_BUF;
#pragma unroll
    for (int i = 0; i < W_IT; ++i) {
      const int idx = tid + i * 256;
      *(u32x4*)(sW + (idx / CPR) * RB + (idx % CPR) * 16) = rw[i];
    }
  };

  // lane-private running state of the TM rows this lane sees
  float rm[TM], rs[TM], rt[TM];
  int tg[TM];
#pragma unroll
  for (int b = 0; b < TM; ++b) {
    rm[b] = -INFINITY, rs[b] = 0.f, rt[b] = 0.f;
    tg[b] = targets[min(m0 + wm * (SC_BM / 2) + b * 16 + (lane & 15), R - 1)];
  }
  f32x4 acc[TN][TM];
#pragma unroll
  for (int a = 0; a < TN; ++a)
#pragma unroll
    for (int b = 0; b < TM; ++b) acc[a][b] = f32x4{0.f, 0.f, 0.f, 0.f};

  gload(0);
  swrite(0);
  __syncthreads();
  int buf = 0;
  const int w_off = (lane & 15) * RB + (lane >> 4) * G::FRAG_BYTES;
  const int a_off = (lane & 15) * G::A_PITCH + (lane >> 4) * G::FRAG_BYTES;
  for (int step = 0; step < steps; ++step) {
    if (step + 1 < steps) gload(step + 1);
    const int kt = step % G::KT;
    const char* sW = sWb + buf * G::W_BUF;
    typename Frag8<T>::type fw[TN], fa[TM];
#pragma unroll
    for (int a = 0; a < TN; ++a) fw[a] = cn_lds_frag<T>(sW + (wn * (SC_BN / 2) + a * 16) * RB + w_off);
#pragma unroll
    for (int b = 0; b < TM; ++b) fa[b] = cn_lds_frag<T>(sA + (wm * (SC_BM / 2) + b * 16) * G::A_PITCH + kt * 128 + a_off);
#pragma unroll
    for (int a = 0; a < TN; ++a)
#pragma unroll
      for (int b = 0; b < TM; ++b) acc[a][b] = cn_mma(fw[a], fa[b], acc[a][b]);
    if (step + 1 < steps) swrite(buf ^ 1);
    __syncthreads();
    buf ^= 1;
    if (kt == G::KT - 1) {  // an N-tile is complete: fold it into the running state (registers only)
      const int nb = (t_begin + step / G::KT) * SC_BN + wn * (SC_BN / 2) + 4 * (lane >> 4);
      float bz[TN][4];
#pragma unroll
      for (int a = 0; a < TN; ++a)
#pragma unroll
        for (int i = 0; i < 4; ++i) bz[a][i] = bias[min(nb + a * 16 + i, V - 1)];
#pragma unroll
      for (int b = 0; b < TM; ++b) {
        float z[TN][4], tmax = -INFINITY;
#pragma unroll
        for (int a = 0; a < TN; ++a)
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const int n = nb + a * 16 + i;
            z[a][i] = acc[a][b][i] + bz[a][i];
            if (n < V) {
              tmax = fmaxf(tmax, z[a][i]);
              if (n == tg[b]) rt[b] += z[a][i];  // at most one column of the vocabulary matches: 0 + z
            }
            acc[a][b][i] = 0.f;
          }
        if (tmax != -INFINITY) {
          const float nm = fmaxf(rm[b], tmax);
          float sum = rs[b] * __expf(rm[b] - nm);  // (rm = -inf: rs = 0 and exp(-inf) = 0)
#pragma unroll
          for (int a = 0; a < TN; ++a)
#pragma unroll
            for (int i = 0; i < 4; ++i)
              if (nb + a * 16 + i < V) sum += __expf(z[a][i] - nm);
          rm[b] = nm, rs[b] = sum;
        }
      }
    }
  }

  // lanes l, l + 16, l + 32, l + 48 hold the same rows: two exchanges; then the two wn waves through LDS (the loop's
  // last barrier has passed: nobody reads the tiles any more)
  float* sx = (float*)smem;  // [SC_BM][3] of the wn = 1 waves
#pragma unroll
  for (int b = 0; b < TM; ++b) {
#pragma unroll
    for (int o = 16; o <= 32; o <<= 1) {
      const float m2 = __shfl_xor(rm[b], o), s2 = __shfl_xor(rs[b], o), t2 = __shfl_xor(rt[b], o);
      cn_lse_merge(rm[b], rs[b], m2, s2);
      rt[b] += t2;
    }
    if (wn == 1 && lane < 16) {
      float* p = sx + (wm * (SC_BM / 2) + b * 16 + lane) * 3;
      p[0] = rm[b], p[1] = rs[b], p[2] = rt[b];
    }
  }
  __syncthreads();
  if (wn == 0 && lane < 16) {
#pragma unroll
    for (int b = 0; b < TM; ++b) {
      const int ml = wm * (SC_BM / 2) + b * 16 + lane;
      const float* p = sx + ml * 3;
      cn_lse_merge(rm[b], rs[b], p[0], p[1]);
      rt[b] += p[2];
      if (m0 + ml < R) {
        float* o = part + ((size_t)(m0 + ml) * S + slab) * 3;
        o[0] = rm[b], o[1] = rs[b], o[2] = rt[b];
      }
    }
  }
}

// One wave per caption: lane t combines the S partial states of position t in slab order, lp = target logit - (max + log sum);
// a pad target gives exactly 0 and is not counted, a target outside [0, V) gives NaN.  The caption's sum and count are a
// butterfly over the wave (fixed order).
__global__ __launch_bounds__(256) void cn_score_merge_kernel(const float* __restrict__ part, const int32_t* __restrict__ targets,
                                                             int P, int cap_len, int S, int V, int pad_id,
                                                             float* __restrict__ tok_lprobs, float* __restrict__ sum_lprobs,
                                                             int32_t* __restrict__ n_tokens) {
  const int p = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (p >= P) return;
  float sum = 0.f;
  int cnt = 0;
  for (int t = lane; t < cap_len; t += 64) {
    const size_t r = (size_t)p * cap_len + t;
    const int tg = targets[r];
    float lp = 0.f;
    if (tg != pad_id) {
      float m = -INFINITY, s = 0.f, z = 0.f;
      for (int k = 0; k < S; ++k) {
        const float* q = part + (r * S + k) * 3;
        const float m2 = q[0], nm = fmaxf(m, m2);
        s = (m == -INFINITY ? 0.f : s * expf(m - nm)) + q[1] * expf(m2 - nm);  // a slab is never empty: m2 is finite
        m = nm;
        z += q[2];
      }
      lp = (tg < 0 || tg >= V) ? __builtin_nanf("") : z - (m + logf(s));
      ++cnt;
    }
    if (tok_lprobs) tok_lprobs[r] = lp;
    sum += lp;
  }
  sum = cn_wave_sum(sum);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o);
  if (lane == 0) {
    sum_lprobs[p] = sum;
    n_tokens[p] = cnt;
  }
}

// slabs of a launch: `forced` >= 1 (CONETTE_OPT_SCORE_VSPLIT) or chosen so that about two blocks per compute unit exist
static inline int cn_score_slabs(int R, int V, int n_cu, int forced) {
  const int n_tiles = cn_cdiv(V, SC_BN), row_tiles = cn_cdiv(R, SC_BM);
  if (forced >= 1) return forced < n_tiles ? forced : n_tiles;
  int s = (2 * n_cu) / row_tiles;
  if (s > SC_MAX_AUTO_SLABS) s = SC_MAX_AUTO_SLABS;
  if (s > n_tiles) s = n_tiles;
  return s < 1 ? 1 : s;
}
static inline size_t cn_score_part_bytes(int R, int S) { return cn_align((size_t)R * S * 3 * sizeof(float)); }

template <typename T>
static int cn_score_launch(const T* xt, const T* W, const float* bias, const int32_t* targets, int P, int cap_len, int V, int S,
                           int pad_id, float* part, float* tok_lprobs, float* sum_lprobs, int32_t* n_tokens, hipStream_t s) {
  const int R = P * cap_len;
  CN_TRY(cn_configure_lds((const void*)cn_score_kernel<T>, ScoreGeom<T>::SMEM));
  hipLaunchKernelGGL((cn_score_kernel<T>), dim3((unsigned)cn_cdiv(R, SC_BM), (unsigned)S), dim3(256), ScoreGeom<T>::SMEM, s, xt, W, bias,
                     targets, R, V, part);
  CN_LAUNCH_CHECK();
  hipLaunchKernelGGL(cn_score_merge_kernel, dim3((unsigned)cn_cdiv(P, 4)), dim3(256), 0, s, part, targets, P, cap_len, S, V, pad_id,
                     tok_lprobs, sum_lprobs, n_tokens);
  CN_LAUNCH_CHECK();
  return CN_OK;
}
