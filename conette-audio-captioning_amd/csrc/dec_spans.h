// Beam search over spans of recordings that were encoded once: conette_decode_spans (include/conette_hip.h).
//
// The decoder's audio memory carries no positional encoding, so a frame's cross-attention K/V are the same in whichever span the
// frame sits: the conversion, the projection and the all-layer K/V GEMM of dec_prepare run once over the N * t_rec recording frames,
// and the kernel below lays the spans' rows out as the (S, t_span, kv_ld) array the step kernels read, together with the (S) lengths
// they take as frame_lens.  From there the step loop of decode_impl runs as it does for conette_decode.
//
// The table (S, 3) of (recording, start, len) is read HERE, on the device, at every launch: a replayed graph follows a table whose
// contents changed behind the same address.  What is read is clamped -- recording to 0 .. N - 1, start to 0 .. t_rec - 1, len to
// 1 .. min(t_span, t_rec - start) -- so that no table can make the kernel read outside `src`; validation proper is the host's.
#pragma once
#include "common.h"

// One block per (frame t of the span, span s); a K/V row of all layers is row_vecs 16-byte words in every precision.  Rows at or
// beyond the span's length are exact zeros.  src: (N * t_rec) rows, dst: (S * t_span) rows.
__global__ __launch_bounds__(256) void cn_span_gather_kernel(const uint4* __restrict__ src, const int32_t* __restrict__ spans, int n_rec,
                                                             int t_rec, int t_span, int row_vecs, uint4* __restrict__ dst,
                                                             int32_t* __restrict__ span_lens) {
  const int t = blockIdx.x, s = blockIdx.y;
  const int rec = min(max(spans[3 * s], 0), n_rec - 1);
  const int start = min(max(spans[3 * s + 1], 0), t_rec - 1);
  const int len = min(max(spans[3 * s + 2], 1), min(t_span, t_rec - start));
  uint4* out = dst + ((size_t)s * t_span + t) * row_vecs;
  if (t < len) {
    const uint4* in = src + ((size_t)rec * t_rec + start + t) * row_vecs;
    for (int i = threadIdx.x; i < row_vecs; i += 256) out[i] = in[i];
  } else {
    const uint4 zero = make_uint4(0u, 0u, 0u, 0u);
    for (int i = threadIdx.x; i < row_vecs; i += 256) out[i] = zero;
  }
  if (t == 0 && threadIdx.x == 0) span_lens[s] = len;
}
