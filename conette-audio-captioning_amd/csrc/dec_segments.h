// Caption timeline, the merge rule: conette_segments (include/conette_hip.h).  The rule, its arithmetic included, is stated in
// conette_amd/segments.py; merge_batch there is what these two kernels equal bit for bit.
//
//   cn_seg_adjacency_kernel  one wave per adjacent pair (recording r, windows k and k + 1): both rows come into LDS, their content
//                            lengths and the occurrence ranks of row k are found, and u(k, k + 1) is computed by the pair routines of
//                            dec_consensus.h (cs_pair_ngram / cs_pair_edit: exact integer counts, one rounded fp32 operation at a
//                            time).  Pairs at or beyond n_windows[r] - 1 write exact zeros, so every element is written.
//   cn_seg_runs_kernel       one thread per recording walks its windows in time order, as cn_tag_events_kernel walks frames: the
//                            current run's first window, representative and smallest adjacency live in registers; a segment goes out
//                            when window k + 1 does not join.  Unused slots are written with (-1, -1), -1, 0 and (-1, -1).
#pragma once
#include "dec_consensus.h"

#define CN_SEG_WAVES 4  // pairs per block of the adjacency kernel

struct CnSegArgs {
  const int32_t* preds;      // (N, Wmax, L)
  const int32_t* n_windows;  // (N), clamped to 0 .. Wmax
  const int32_t* win_spans;  // (N, Wmax, 2) (start, len)
  const float* lprobs;       // (N, Wmax)
  int n_rec, w_max, l, utility, max_order, max_run, max_segments, eos_id, pad_id;
  float threshold;
  float* adj;                // (N, Wmax - 1): the caller's `adjacency`, or the workspace
  int32_t* seg_windows;      // (N, max_segments, 2)
  int32_t* seg_frames;       // (N, max_segments, 2)
  int32_t* seg_rep;          // (N, max_segments)
  float* seg_agree;          // (N, max_segments)
  int32_t* counts;           // (N)
};

__global__ __launch_bounds__(CN_SEG_WAVES * 64) void cn_seg_adjacency_kernel(CnSegArgs A) {
  __shared__ int s_ids[CN_SEG_WAVES][2][CN_CS_MAX_LEN];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int per_rec = A.w_max - 1;
  const long pair = (long)blockIdx.x * CN_SEG_WAVES + wave;
  const bool in_grid = pair < (long)A.n_rec * per_rec;
  const int r = in_grid ? (int)(pair / per_rec) : 0, k = in_grid ? (int)(pair - (long)r * per_rec) : 0;
  const int w = in_grid ? min(max(A.n_windows[r], 0), A.w_max) : 0;
  const bool live = in_grid && k + 1 < w;  // (wave-uniform)
  const int L = A.l;
  int* ci = s_ids[wave][0];
  int* cj = s_ids[wave][1];
  if (live && lane < L) {
    const int32_t* src = A.preds + ((size_t)r * A.w_max + k) * L;  // rows k and k + 1 are contiguous
    ci[lane] = src[lane];
    cj[lane] = src[L + lane];
  }
  __syncthreads();
  float u = 0.0f;
  if (live) {
    const int li = cs_content_len(ci, L, lane, A.eos_id, A.pad_id);
    const int lj = cs_content_len(cj, L, lane, A.eos_id, A.pad_id);
    if (A.utility == 0)
      u = cs_pair_ngram(ci, li, cj, lj, cs_ranks(ci, li, lane), lane, A.max_order);
    else
      u = cs_pair_edit(ci, li, cj, lj, lane);
  }
  if (in_grid && lane == 0) A.adj[pair] = u;
}

__global__ __launch_bounds__(64) void cn_seg_runs_kernel(CnSegArgs A) {
  const int r = blockIdx.x * 64 + threadIdx.x;
  if (r >= A.n_rec) return;
  const int w = min(max(A.n_windows[r], 0), A.w_max);
  const int MS = A.max_segments;
  const float* adj = A.adj + (size_t)r * (A.w_max - 1);
  const float* lp = A.lprobs + (size_t)r * A.w_max;
  const int32_t* sp = A.win_spans + (size_t)r * A.w_max * 2;
  int32_t* seg_w = A.seg_windows + (size_t)r * MS * 2;
  int32_t* seg_f = A.seg_frames + (size_t)r * MS * 2;
  int32_t* seg_rep = A.seg_rep + (size_t)r * MS;
  float* seg_agree = A.seg_agree + (size_t)r * MS;
  int count = 0;
  if (w > 0) {
    int first = 0, rep = 0;
    float rep_lp = lp[0], agree = 1.0f;
    int start = sp[0], len = sp[1];  // window k's span
    int f0 = start;                  // the current segment's first frame
    for (int k = 0; k < w; ++k) {
      const bool last = k + 1 == w;
      float a = 0.0f;
      int nstart = 0, nlen = 0;
      bool joins = false;
      if (!last) {
        a = adj[k];
        nstart = sp[2 * (k + 1)];
        nlen = sp[2 * (k + 1) + 1];
        joins = a >= A.threshold && !(A.max_run > 0 && k + 1 - first >= A.max_run);
      }
      if (joins) {
        if (k == first || a < agree) agree = a;  // (the first link of a run replaces the 1 of a single window)
        const float v = lp[k + 1];
        if (v > rep_lp || (rep_lp != rep_lp && v == v)) {
          rep = k + 1;
          rep_lp = v;
        }
      } else {
        const int f1 = last ? start + len : (int)(((long)nstart + start + len + 1) >> 1);
        if (count < MS) {
          seg_w[2 * count] = first;
          seg_w[2 * count + 1] = k + 1;
          seg_f[2 * count] = f0;
          seg_f[2 * count + 1] = f1;
          seg_rep[count] = rep;
          seg_agree[count] = agree;
        }
        ++count;
        if (!last) {
          first = k + 1;
          rep = k + 1;
          rep_lp = lp[k + 1];
          agree = 1.0f;
          f0 = f1;
        }
      }
      start = nstart;
      len = nlen;
    }
  }
  A.counts[r] = count;
  for (int k = min(count, MS); k < MS; ++k) {
    seg_w[2 * k] = -1;
    seg_w[2 * k + 1] = -1;
    seg_f[2 * k] = -1;
    seg_f[2 * k + 1] = -1;
    seg_rep[k] = -1;
    seg_agree[k] = 0.0f;
  }
}
