// Byzantine-robust aggregation over flat parameter arenas: the two streaming
// passes behind FedMedian / TrimmedMean (order_stat_kernel) and (Multi-)Krum
// (pairwise_sqdist_kernel).  Same shape as aggregate.hip's weighted sum: up to
// kMaxInputs fp32/bf16 arenas read once with 16-byte nontemporal loads in a
// grid-stride loop, everything per element held in registers.
#include <utility>

#include "arena_io.h"

namespace p2 {

// ---------------------------------------------------------------------------
// Sorting network: Batcher's odd-even merge sort on the next power of two,
// without the comparators that touch a wire >= K (those wires would hold +inf
// and never move).  63 compare-exchanges at K = 16, 19 at K = 8, 5 at K = 4.
// Built at compile time so every register index in the kernel is a constant.
// ---------------------------------------------------------------------------
template <int K>
struct SortNet {
  int a[64], b[64];
  int n;
  constexpr SortNet() : a{}, b{}, n(0) {
    int P = 1;
    while (P < K) P *= 2;
    for (int p = 1; p < P; p *= 2)
      for (int k = p; k >= 1; k /= 2)
        for (int j = k % p; j + k < P; j += 2 * k)
          for (int i = 0; i < k && i + j + k < P; ++i)
            if ((i + j) / (2 * p) == (i + j + k) / (2 * p) && i + j + k < K) {
              a[n] = i + j;
              b[n] = i + j + k;
              ++n;
            }
  }
};
template <int K>
inline constexpr SortNet<K> kSortNet{};

// V = f32x4 (four independent coordinates per lane) or float (the tail)
template <int A, int B, int K, typename V>
P2_DEVICE void compare_exchange(V (&v)[K]) {
  const V lo = __builtin_elementwise_min(v[A], v[B]);
  const V hi = __builtin_elementwise_max(v[A], v[B]);
  v[A] = lo;
  v[B] = hi;
}

template <int K, typename V, size_t... I>
P2_DEVICE void sort_network(V (&v)[K], std::index_sequence<I...>) {
  (compare_exchange<kSortNet<K>.a[I], kSortNet<K>.b[I]>(v), ...);
}

// mean of sorted[b .. K-1-b], added in ascending order
template <int K, typename V>
P2_DEVICE V trimmed_mean_of(V (&v)[K], int b) {
  sort_network<K>(v, std::make_index_sequence<kSortNet<K>.n>{});
  V acc = V(0.f);
#pragma unroll
  for (int j = 0; j < K; ++j)
    if (j >= b && j < K - b) acc = (j == b) ? v[j] : acc + v[j];
  return acc / float(K - 2 * b);
}

// Coordinate-wise trimmed mean of K arenas; b (uniform) values dropped at each
// end.  The kept values are summed in sorted order, so the result does not
// depend on the order of the arenas.  The n % 4 tail runs the same network on
// scalars in the first lanes of block 0.
template <int K>
__global__ __launch_bounds__(256) void order_stat_kernel(ArenaSrcs a, uint32_t bf16_mask, int b, void* out,
                                                         int out_bf16, int64_t n4, int64_t n) {
  const int64_t stride = int64_t(gridDim.x) * blockDim.x;
  for (int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; i < n4; i += stride) {
    f32x4 v[K];
#pragma unroll
    for (int k = 0; k < K; ++k) v[k] = load4(a.src[k], i, (bf16_mask >> k) & 1u);
    store4(out, i, trimmed_mean_of<K>(v, b), out_bf16);
  }
  const int64_t t = n4 * 4 + threadIdx.x;
  if (blockIdx.x == 0 && t < n) {
    float v[K];
#pragma unroll
    for (int k = 0; k < K; ++k) v[k] = load1(a.src[k], t, (bf16_mask >> k) & 1u);
    store1(out, t, trimmed_mean_of<K>(v, b), out_bf16);
  }
}

// ---------------------------------------------------------------------------
// All K (K - 1) / 2 squared L2 distances in one pass: one fp32 accumulator per
// pair per lane, reduced lane -> wave (DPP, fixed order) -> block (LDS, wave
// order) into partials[pair][block].  sqdist_finish_kernel adds the blocks in a
// fixed order.  No atomics anywhere: the matrix is a function of the inputs,
// their order and n alone.
// ---------------------------------------------------------------------------
constexpr int pair_count(int k) { return k * (k - 1) / 2; }
// row-major index of pair (i < j) in the strict upper triangle
constexpr int pair_index(int i, int j, int k) { return i * k - i * (i + 1) / 2 + (j - i - 1); }

template <int K>
__global__ __launch_bounds__(256) void pairwise_sqdist_kernel(ArenaSrcs a, uint32_t bf16_mask, float* partials,
                                                              int64_t n4, int64_t n) {
  constexpr int P = pair_count(K);
  float acc[P];
#pragma unroll
  for (int p = 0; p < P; ++p) acc[p] = 0.f;

  const int64_t stride = int64_t(gridDim.x) * blockDim.x;
  for (int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; i < n4; i += stride) {
    f32x4 v[K];
#pragma unroll
    for (int k = 0; k < K; ++k) v[k] = load4(a.src[k], i, (bf16_mask >> k) & 1u);
#pragma unroll
    for (int x = 0; x < K; ++x)
#pragma unroll
      for (int y = x + 1; y < K; ++y) {
        const f32x4 d = v[x] - v[y];
        float s = acc[pair_index(x, y, K)];
        s = fmaf(d[0], d[0], s);
        s = fmaf(d[1], d[1], s);
        s = fmaf(d[2], d[2], s);
        s = fmaf(d[3], d[3], s);
        acc[pair_index(x, y, K)] = s;
      }
  }
  const int64_t t = n4 * 4 + threadIdx.x;  // the n % 4 tail: first lanes of block 0
  if (blockIdx.x == 0 && t < n) {
    float v[K];
#pragma unroll
    for (int k = 0; k < K; ++k) v[k] = load1(a.src[k], t, (bf16_mask >> k) & 1u);
#pragma unroll
    for (int x = 0; x < K; ++x)
#pragma unroll
      for (int y = x + 1; y < K; ++y) {
        const float d = v[x] - v[y];
        acc[pair_index(x, y, K)] = fmaf(d, d, acc[pair_index(x, y, K)]);
      }
  }

  __shared__ float red[4][P];
  const int wave = threadIdx.x / kWave, lane = threadIdx.x % kWave;
#pragma unroll
  for (int p = 0; p < P; ++p) {
    const float s = wave_sum(acc[p]);
    if (lane == 0) red[wave][p] = s;
  }
  __syncthreads();
  if (threadIdx.x < P)
    partials[int64_t(threadIdx.x) * gridDim.x + blockIdx.x] =
        (red[0][threadIdx.x] + red[1][threadIdx.x]) + (red[2][threadIdx.x] + red[3][threadIdx.x]);
}

// One block per pair: lane t adds partials[pair][t], [t + 256], ... in index
// order, then wave and block reductions as above; writes both triangle entries
// (and block 0 the zero diagonal).
__global__ __launch_bounds__(256) void sqdist_finish_kernel(const float* partials, int nblocks, int k, float* out) {
  const int p = blockIdx.x;
  float s = 0.f;
  for (int b = threadIdx.x; b < nblocks; b += blockDim.x) s += partials[int64_t(p) * nblocks + b];
  s = wave_sum(s);
  __shared__ float red[4];
  if (threadIdx.x % kWave == 0) red[threadIdx.x / kWave] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    int i = 0, first = 0;  // first = pair_index(i, i + 1, k)
    while (first + (k - 1 - i) <= p) first += k - 1 - i, ++i;
    const int j = i + 1 + (p - first);
    const float d = (red[0] + red[1]) + (red[2] + red[3]);
    out[i * k + j] = d;
    out[j * k + i] = d;
  }
  if (p == 0 && threadIdx.x < k) out[threadIdx.x * k + threadIdx.x] = 0.f;
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
static uint32_t fill_srcs(ArenaSrcs& a, const void* const* srcs, const int* src_bf16, int k) {
  uint32_t mask = 0;
  for (int j = 0; j < k; ++j) {
    a.src[j] = srcs[j];
    if (src_bf16[j]) mask |= 1u << j;
  }
  return mask;
}

template <int K>
static void launch_order_stat(const ArenaSrcs& a, uint32_t mask, int b, void* out, int out_bf16, int64_t n,
                              hipStream_t s) {
  const int64_t n4 = n / 4;
  hipLaunchKernelGGL(order_stat_kernel<K>, dim3(stream_grid(n4, 256)), dim3(256), 0, s, a, mask, b, out, out_bf16, n4,
                     n);
}

template <int K>
static void launch_sqdist(const ArenaSrcs& a, uint32_t mask, float* partials, int64_t n, hipStream_t s) {
  const int64_t n4 = n / 4;
  hipLaunchKernelGGL(pairwise_sqdist_kernel<K>, dim3(stream_grid(n4, 256)), dim3(256), 0, s, a, mask, partials, n4, n);
}

#define P2_FOR_K(M) \
  M(2) M(3) M(4) M(5) M(6) M(7) M(8) M(9) M(10) M(11) M(12) M(13) M(14) M(15) M(16)

void trimmed_mean(const void* const* srcs, const int* src_bf16, int k, int trim, void* out, int out_bf16, int64_t n,
                  hipStream_t stream) {
  if (k < 1 || k > kMaxInputs) throw std::invalid_argument("trimmed_mean: k must be in [1, kMaxInputs]");
  if (trim < 0 || trim > (k - 1) / 2) throw std::invalid_argument("trimmed_mean: trim must be in [0, (k - 1) / 2]");
  ArenaSrcs a{};
  const uint32_t mask = fill_srcs(a, srcs, src_bf16, k);
  switch (k) {
    case 1: launch_order_stat<1>(a, mask, trim, out, out_bf16, n, stream); break;
#define P2_CASE(K) \
  case K: launch_order_stat<K>(a, mask, trim, out, out_bf16, n, stream); break;
      P2_FOR_K(P2_CASE)
#undef P2_CASE
  }
}

int pairwise_sqdist_blocks(int64_t n) { return stream_grid(n / 4, 256); }

void pairwise_sqdist(const void* const* srcs, const int* src_bf16, int k, float* partials, float* out, int64_t n,
                     hipStream_t stream) {
  if (k < 2 || k > kMaxInputs) throw std::invalid_argument("pairwise_sqdist: k must be in [2, kMaxInputs]");
  ArenaSrcs a{};
  const uint32_t mask = fill_srcs(a, srcs, src_bf16, k);
  switch (k) {
#define P2_CASE(K) \
  case K: launch_sqdist<K>(a, mask, partials, n, stream); break;
    P2_FOR_K(P2_CASE)
#undef P2_CASE
  }
  hipLaunchKernelGGL(sqdist_finish_kernel, dim3(pair_count(k)), dim3(256), 0, stream, partials,
                     pairwise_sqdist_blocks(n), k, out);
}

}  // namespace p2
