// Consensus (minimum-Bayes-risk) choice among candidate captions: conette_consensus (include/conette_hip.h).  The rule, its
// arithmetic included, is stated in conette_amd/consensus.py; select_fp32 there is what this kernel equals bit for bit.
//
// One workgroup per clip, everything in LDS:
//   phase 0  the clip's ids (N x L) and weights come in; one wave per candidate finds its content length
//   phase 1  one wave per candidate, a lane per position a: for each order n = 1..4 the occurrence RANK of the n-gram at a -- how
//            many earlier positions of the same candidate hold the same n-gram (4 bytes packed in one word)
//   phase 2  one wave per pair i < j.  "ngram": lane a walks c_j once with a sliding 4-token window and counts, per order, the
//            positions of c_j that hold its n-gram; the clipped match is popc(ballot(count > rank)): of the p positions of c_i
//            with an n-gram that c_j holds q times, those of rank 0 .. q - 1 count, min(p, q) in all.  Tokens are compared as whole
//            32-bit words: nothing is hashed.  "edit": the anti-diagonal wavefront, DP row a + 1 in lane a, the row above through
//            one __shfl_up per diagonal.  u goes to LDS in both triangles
//   phase 3  thread i sums E_i over j = 0 .. N - 1 in order; the pairwise table goes out
//   phase 4  wave 0 takes the first maximum and the runner-up
// Integer counts are exact; every fp32 operation is one of cs_add / cs_sub / cs_mul / cs_div below, each rounded on its own.
#pragma once
#include "common.h"

#define CN_CS_MAX_CANDS 64
#define CN_CS_MAX_LEN 64
#define CN_CS_MAX_WAVES 16
#define CN_CS_USTRIDE (CN_CS_MAX_CANDS + 1)   // (phase 3 reads a column per lane: the odd stride keeps the lanes on separate banks)

// One rounded fp32 operation each.  HIP's __fmul_rn / __fadd_rn are the plain operators, which the build's default contraction
// turns into FMAs (seen in this kernel's ISA: the sum of E became a v_fmac chain); operators written under `fp contract(off)` are
// left alone.  Nothing is reassociated (no fast-math) and fp32 division is the correctly rounded expansion.
__device__ __forceinline__ float cs_add(float a, float b) {
#pragma clang fp contract(off)
  return a + b;
}
__device__ __forceinline__ float cs_sub(float a, float b) {
#pragma clang fp contract(off)
  return a - b;
}
__device__ __forceinline__ float cs_mul(float a, float b) {
#pragma clang fp contract(off)
  return a * b;
}
__device__ __forceinline__ float cs_div(float a, float b) {
#pragma clang fp contract(off)
  return a / b;
}

struct CnConsensusArgs {
  const int32_t* preds;    // (B, N, L)
  const int32_t* lens;     // (B, N) or null
  const float* weights;    // (B, N) or null
  float uniform_w;         // fp32(1) / fp32(N): every weight when `weights` is null
  int n, l, utility, max_order, eos_id, pad_id;
  float* expected;         // (B, N)
  int32_t* best;           // (B)
  float* margin;           // (B)
  float* pairwise;         // (B, N, N) or null
};

// per order n = 1..4: does the n-gram at c_x[a] equal the n-gram at c_y[b]?  xa / yb hold the four tokens from a / b on (anything
// behind the content's end: `ok` masks those orders), returned as 4 flags in the low bytes of one word so that four counters add at once
__device__ __forceinline__ uint32_t cs_match4(const int (&xa)[4], const int (&yb)[4], int room_y) {
  const bool e1 = xa[0] == yb[0], e2 = e1 && xa[1] == yb[1], e3 = e2 && xa[2] == yb[2], e4 = e3 && xa[3] == yb[3];
  return (uint32_t)(e1 && room_y >= 1) | ((uint32_t)(e2 && room_y >= 2) << 8) | ((uint32_t)(e3 && room_y >= 3) << 16) |
         ((uint32_t)(e4 && room_y >= 4) << 24);
}

// lane a's packed counts, per order, of the positions b < stop of content y (length len_y, in LDS) whose n-gram equals the one in xa
__device__ __forceinline__ uint32_t cs_count4(const int (&xa)[4], const int* y, int len_y, int stop) {
  int yb[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) yb[k] = k < len_y ? y[k] : 0;
  uint32_t cnt = 0;
  for (int b = 0; b < stop; ++b) {   // (stop <= len_y <= 64: a byte never overflows)
    cnt += cs_match4(xa, yb, len_y - b);
    yb[0] = yb[1];
    yb[1] = yb[2];
    yb[2] = yb[3];
    yb[3] = b + 4 < len_y ? y[b + 4] : 0;
  }
  return cnt;
}

// ---- the per-wave routines of the rule, shared with the caption timeline's adjacency kernel (dec_segments.h).  `lane` is the
// caller's lane; rows live in LDS; every routine is called by all 64 lanes of a wave.

// content length of a row without given lengths: the tokens in front of the first eos_id or pad_id (the whole row if neither occurs)
__device__ __forceinline__ int cs_content_len(const int* row, int L, int lane, int eos_id, int pad_id) {
  const bool stop = lane < L && (row[lane] == eos_id || row[lane] == pad_id);
  const unsigned long long m = __ballot(stop);
  return m ? __ffsll((long long)m) - 1 : L;
}

// lane a's occurrence ranks, packed per order: how many positions b < a of the same content hold the n-gram at a
__device__ __forceinline__ uint32_t cs_ranks(const int* row, int len, int lane) {
  int xa[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) xa[k] = lane + k < len ? row[lane + k] : 0;
  // (positions b < lane: the loop runs to the wave's longest need and each lane masks its own tail)
  int yb[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) yb[k] = k < len ? row[k] : 0;
  uint32_t rank = 0;
  for (int b = 0; b + 1 < len; ++b) {
    const uint32_t hit = cs_match4(xa, yb, len - b);
    rank += b < lane ? hit : 0u;
    yb[0] = yb[1];
    yb[1] = yb[2];
    yb[2] = yb[3];
    yb[3] = b + 4 < len ? row[b + 4] : 0;
  }
  return rank;
}

// u(i, j) of the n-gram utility; `rank` is lane's cs_ranks of c_i
__device__ __forceinline__ float cs_pair_ngram(const int* ci, int li, const int* cj, int lj, uint32_t rank, int lane, int max_order) {
  int xa[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) xa[k] = lane + k < li ? ci[lane + k] : 0;
  const uint32_t cnt = cs_count4(xa, cj, lj, lj);
  float sum = 0.0f;
  int counted = 0;
  for (int n = 1; n <= max_order; ++n) {
    const int ti = max(li - n + 1, 0), tj = max(lj - n + 1, 0);
    const int sh = 8 * (n - 1);
    const bool in = lane < ti && ((cnt >> sh) & 0xffu) > ((rank >> sh) & 0xffu);
    const int m = __popcll(__ballot(in));
    if (ti + tj > 0) {
      sum = cs_add(sum, cs_div((float)(2 * m), (float)(ti + tj)));
      ++counted;
    }
  }
  return counted ? cs_div(sum, (float)counted) : 1.0f;
}

// u(i, j) of the edit utility.  Lane a owns DP row a + 1 (token ci[a]); on diagonal d it fills column col = d - (a + 1) when
// 1 <= col <= lj.  `cur` is the row's newest cell (column 0 at the start: a + 1), `up` the newest cell of the row above (one diagonal
// behind), `diag` the `up` of the diagonal before.  Row 0 is the column index itself.
__device__ __forceinline__ float cs_pair_edit(const int* ci, int li, const int* cj, int lj, int lane) {
  const int row = lane + 1;
  const int x = lane < li ? ci[lane] : 0;
  int cur = row, diag = lane;
  for (int d = 2; d <= li + lj; ++d) {
    const int col = d - row;
    int up = __shfl_up(cur, 1);
    if (lane == 0) up = col;
    if (lane < li && col >= 1 && col <= lj) {
      const int sub = diag + (x != cj[col - 1]);
      cur = min(min(up, cur) + 1, sub);
    }
    diag = lane == 0 ? col : up;
  }
  const int lev = li == 0 ? lj : __shfl(cur, li - 1);
  const int big = max(li, lj);
  return big ? cs_sub(1.0f, cs_div((float)lev, (float)big)) : 1.0f;
}

__global__ __launch_bounds__(CN_CS_MAX_WAVES * 64) void cn_consensus_kernel(CnConsensusArgs A) {
  __shared__ int s_ids[CN_CS_MAX_CANDS * CN_CS_MAX_LEN];
  __shared__ uint32_t s_rank[CN_CS_MAX_CANDS * CN_CS_MAX_LEN];
  __shared__ float s_u[CN_CS_MAX_CANDS * CN_CS_USTRIDE];
  __shared__ int s_len[CN_CS_MAX_CANDS];
  __shared__ float s_w[CN_CS_MAX_CANDS];
  __shared__ float s_e[CN_CS_MAX_CANDS];

  const int N = A.n, L = A.l;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nwaves = blockDim.x >> 6;
  const size_t clip = blockIdx.x;

  // ---- phase 0: ids, weights, content lengths
  const int32_t* src = A.preds + clip * (size_t)N * L;
  for (int t = tid; t < N * L; t += blockDim.x) s_ids[t] = src[t];
  if (tid < N) s_w[tid] = A.weights ? A.weights[clip * N + tid] : A.uniform_w;
  __syncthreads();
  for (int c = wave; c < N; c += nwaves) {
    const int* row = s_ids + c * L;
    int len;
    if (A.lens) {
      len = min(max(A.lens[clip * N + c], 0), L);
      if (len > 0 && row[len - 1] == A.eos_id) --len;
    } else {
      len = cs_content_len(row, L, lane, A.eos_id, A.pad_id);
    }
    if (lane == 0) s_len[c] = len;
  }
  __syncthreads();

  // ---- phase 1: occurrence ranks (only the n-gram utility reads them)
  if (A.utility == 0) {
    for (int c = wave; c < N; c += nwaves) {
      const int* row = s_ids + c * L;
      const uint32_t rank = cs_ranks(row, s_len[c], lane);
      if (lane < L) s_rank[c * L + lane] = rank;
    }
  }
  if (tid < N) s_u[tid * CN_CS_USTRIDE + tid] = 1.0f;
  __syncthreads();

  // ---- phase 2: one wave per pair i < j, pairs in row-major order of the upper triangle
  const int npairs = N * (N - 1) / 2;
  for (int p = wave; p < npairs; p += nwaves) {
    int i = 0, rest = p;
    while (rest >= N - 1 - i) {
      rest -= N - 1 - i;
      ++i;
    }
    const int j = i + 1 + rest;
    const int* ci = s_ids + i * L;
    const int* cj = s_ids + j * L;
    const int li = s_len[i], lj = s_len[j];
    float u;
    if (A.utility == 0)
      u = cs_pair_ngram(ci, li, cj, lj, lane < L ? s_rank[i * L + lane] : 0u, lane, A.max_order);
    else
      u = cs_pair_edit(ci, li, cj, lj, lane);
    if (lane == 0) {
      s_u[i * CN_CS_USTRIDE + j] = u;
      s_u[j * CN_CS_USTRIDE + i] = u;
    }
  }
  __syncthreads();

  // ---- phase 3: expected utilities, in the order the rule fixes
  if (tid < N) {
    float acc = 0.0f;
    for (int j = 0; j < N; ++j) acc = cs_add(acc, cs_mul(s_w[j], s_u[tid * CN_CS_USTRIDE + j]));
    s_e[tid] = acc;
    A.expected[clip * N + tid] = acc;
  }
  if (A.pairwise) {
    float* dst = A.pairwise + clip * (size_t)N * N;
    for (int t = tid; t < N * N; t += blockDim.x) dst[t] = s_u[(t / N) * CN_CS_USTRIDE + t % N];
  }
  __syncthreads();

  // ---- phase 4: first maximum and runner-up
  if (wave == 0) {
    const float ninf = -__builtin_inff();
    const float e = lane < N ? s_e[lane] : ninf;
    float top = e;
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) top = fmaxf(top, __shfl_xor(top, s));
    const unsigned long long at = __ballot(lane < N && e == top);
    const int best = at ? __ffsll((long long)at) - 1 : 0;   // (no lane equals the maximum only when every E is NaN: index 0)
    float second = lane == best ? ninf : e;
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) second = fmaxf(second, __shfl_xor(second, s));
    if (lane == 0) {
      A.best[clip] = best;
      A.margin[clip] = N == 1 ? __builtin_inff() : cs_sub(top, second);
    }
  }
}
