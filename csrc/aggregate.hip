// Fused k-way weighted sum over flat parameter arenas: the FedAvg hot op.
//
// Replaces the reference's per-layer, per-model torch loop
// (reference p2pfl/learning/aggregators/fedavg.py:49-58: accum[layer] += m*w,
// then /= total) with ONE memory-bound pass: each lane streams float4 from up
// to kMaxInputs arenas, accumulates in fp32 registers with the normalised
// weights, and writes once.  Bytes moved = (k + 1) * 4 * n; at k = 8 and the
// 6.5 M-parameter MNIST CNN that is 234 MB, ~40 us at the ~6 TB/s HBM3E rate.
#include "arena_io.h"

namespace p2 {

struct WSumArgs : ArenaSrcs {
  float w[kMaxInputs];
};

// bf16_mask bit k: input k is bf16 (else fp32).  The mask is uniform across
// the grid, so the per-input dtype test never diverges.  acc_in (may alias
// out, may be null) seeds the fp32 accumulator: a running FedAvg sum folds the
// models in as they arrive and only the last call applies the 1/sum(w) scale.
template <int K>
__global__ __launch_bounds__(256) void wsum_kernel(WSumArgs a, uint32_t bf16_mask, const float* acc_in, float scale,
                                                   void* out, int out_bf16, int64_t n4) {
  const int64_t stride = int64_t(gridDim.x) * blockDim.x;
  for (int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; i < n4; i += stride) {
    f32x4 acc = acc_in ? reinterpret_cast<const f32x4*>(acc_in)[i] : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int k = 0; k < K; ++k) acc += a.w[k] * load4(a.src[k], i, (bf16_mask >> k) & 1u);
    acc *= scale;
    store4(out, i, acc, out_bf16);
  }
}

__global__ void wsum_tail(WSumArgs a, uint32_t bf16_mask, int k, const float* acc_in, float scale, void* out,
                          int out_bf16, int64_t start, int64_t n) {
  int64_t i = start + blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  float acc = acc_in ? acc_in[i] : 0.f;
  for (int j = 0; j < k; ++j) {
    acc = fmaf(a.w[j], load1(a.src[j], i, (bf16_mask >> j) & 1u), acc);
  }
  acc *= scale;
  store1(out, i, acc, out_bf16);
}

template <int K>
static void launch_k(const WSumArgs& a, uint32_t mask, const float* acc_in, float scale, void* out, int out_bf16,
                     int64_t n4, hipStream_t s) {
  hipLaunchKernelGGL(wsum_kernel<K>, dim3(stream_grid(n4, 256)), dim3(256), 0, s, a, mask, acc_in, scale, out,
                     out_bf16, n4);
}

void weighted_sum(const void* const* srcs, const int* src_bf16, const float* weights, int k, const float* acc_in,
                  float scale, void* out, int out_bf16, int64_t n, hipStream_t stream) {
  int done = 0;
  do {
    const int kk = (k - done) < kMaxInputs ? (k - done) : kMaxInputs;
    WSumArgs a{};
    uint32_t mask = 0;
    for (int j = 0; j < kk; ++j) {
      a.src[j] = srcs[done + j];
      a.w[j] = weights[done + j];
      if (src_bf16[done + j]) mask |= 1u << j;
    }
    // chunks after the first accumulate into out (fp32 output only; checked by
    // the caller); only the last chunk applies the scale
    const float* acc = done > 0 ? static_cast<const float*>(out) : acc_in;
    const bool last = done + kk >= k;
    const float sc = last ? scale : 1.f;
    const int ob = last ? out_bf16 : 0;
    const int64_t n4 = n / 4;
    switch (kk) {
      case 0: launch_k<0>(a, mask, acc, sc, out, ob, n4, stream); break;
      case 1: launch_k<1>(a, mask, acc, sc, out, ob, n4, stream); break;
      case 2: launch_k<2>(a, mask, acc, sc, out, ob, n4, stream); break;
      case 3: launch_k<3>(a, mask, acc, sc, out, ob, n4, stream); break;
      case 4: launch_k<4>(a, mask, acc, sc, out, ob, n4, stream); break;
      case 5: launch_k<5>(a, mask, acc, sc, out, ob, n4, stream); break;
      case 6: launch_k<6>(a, mask, acc, sc, out, ob, n4, stream); break;
      case 7: launch_k<7>(a, mask, acc, sc, out, ob, n4, stream); break;
      case 8: launch_k<8>(a, mask, acc, sc, out, ob, n4, stream); break;
      case 9: launch_k<9>(a, mask, acc, sc, out, ob, n4, stream); break;
      case 10: launch_k<10>(a, mask, acc, sc, out, ob, n4, stream); break;
      case 11: launch_k<11>(a, mask, acc, sc, out, ob, n4, stream); break;
      case 12: launch_k<12>(a, mask, acc, sc, out, ob, n4, stream); break;
      case 13: launch_k<13>(a, mask, acc, sc, out, ob, n4, stream); break;
      case 14: launch_k<14>(a, mask, acc, sc, out, ob, n4, stream); break;
      case 15: launch_k<15>(a, mask, acc, sc, out, ob, n4, stream); break;
      default: launch_k<16>(a, mask, acc, sc, out, ob, n4, stream); break;
    }
    const int64_t tail = n - n4 * 4;
    if (tail > 0)
      hipLaunchKernelGGL(wsum_tail, dim3(1), dim3(64), 0, stream, a, mask, kk, acc, sc, out, ob, n4 * 4, n);
    done += kk;
  } while (done < k);
}

}  // namespace p2
