// Fused BatchNorm (+ residual add) (+ ReLU) for MI355X (gfx950, wave64), on
// channels-last activations viewed as [M, C] (M = N*H*W rows of C channels).
//
// What it replaces in a ResNet block (PyTorch-ROCm, NHWC bf16):
//   forward   MIOpen BN training kernel(s) + residual add + ReLU     (3+ passes)
//   backward  ReLU threshold_backward + MIOpen BN backward           (3+ passes)
// Here, per BN:
//   forward   stats (1 read of x)  -> finalize (C threads) -> apply (read x [+res], write y)
//   backward  stats (read dy, y, x) -> finalize              -> apply (read dy, y, x, write dx [+dres])
//
// Column statistics: every thread owns 8 consecutive channels (one 16-B bf16
// load per row), a 256-thread block covers `tpr` threads per row x `rp` row
// phases, row splits go over gridDim.y.  Per-block sums are combined across
// row phases in LDS in fixed order and written as [S, C] partials; the
// finalize kernel reduces the S partials in fixed order (for small bf16
// activations both run as one launch, bn_stats_fin_kernel / bn_bwd_stats_fin_
// kernel, the last block to arrive doing the finalize).  No float atomics:
// results are bitwise reproducible run to run.  Forward statistics use sums
// shifted by the first row's value (x - x[0][c]) so the variance does not
// cancel for activations with a large mean.  The limit of that shift: the
// variance's error is relative to var + (x[0][c] - mean)^2, so a first row that
// is an outlier of its channel costs accuracy (about 6e-3 relative at 1e5
// standard deviations over 32768 rows).  ReLU and the variance clamp are
// comparisons, not fmaxf: a NaN or Inf activation gives a NaN channel (mean,
// rstd, y, running statistics) rather than a finite one.
#include <type_traits>

#include "batchnorm.h"
#include "common.h"

namespace p2bn {
using namespace p2;

P2_DEVICE void ld8f(const float* p, float (&v)[8]) { Vec8<float>::load(p, v); }

constexpr int kThreads = 256;
constexpr int kRedCols = kThreads * 8;  // LDS columns of one phase-reduction slab
constexpr int kInFlight = 4;             // rows per thread in flight in the statistics passes

// ---------------------------------------------------------------------------
// Block-level fixed-order reduction of two per-thread [8] accumulators over
// the rp row phases, written as row blockIdx.y of the [S, C] partials a / b:
// st(i, v) stores element i of the [2, S, C] partials.
// ---------------------------------------------------------------------------
struct PlainStore {
  float* __restrict__ part;
  P2_DEVICE void operator()(size_t i, float v) const { part[i] = v; }
};

template <class Store>
P2_DEVICE void phase_reduce_store(const float (&s1)[8], const float (&s2)[8], bool active, int tg, int ph, int tpr,
                                  int rp, int C, const Store& st) {
  __shared__ float red[2][kRedCols];
  const int width = tpr * 8;  // columns of this block
  if (active) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      red[0][ph * width + tg * 8 + j] = s1[j];
      red[1][ph * width + tg * 8 + j] = s2[j];
    }
  }
  __syncthreads();
  const int S = gridDim.y;
  for (int i = threadIdx.x; i < width; i += kThreads) {
    const int c = blockIdx.x * width + i;
    if (c >= C) continue;
    float a = 0.f, b = 0.f;
    for (int p = 0; p < rp; ++p) {
      a += red[0][p * width + i];
      b += red[1][p * width + i];
    }
    st(size_t(blockIdx.y) * C + c, a);
    st(size_t(S + blockIdx.y) * C + c, b);
  }
}

// One row's share of the forward sums, d = x - x0 (a row past M counts zero).
P2_DEVICE void acc_fwd(const float (&v)[8], const float (&sh)[8], bool in, float (&s1)[8], float (&s2)[8]) {
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const float d = in ? v[j] - sh[j] : 0.f;
    s1[j] += d;
    s2[j] = fmaf(d, d, s2[j]);
  }
}

// One row's share of the backward sums, dz = g behind the ReLU mask y > 0 (yv is read only with RELU).
template <bool RELU>
P2_DEVICE void acc_bwd(const float (&g)[8], const float (&xv)[8], const float (&yv)[8], const float (&mu)[8], bool in,
                       float (&s1)[8], float (&s2)[8]) {
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const float gg = in && (!RELU || yv[j] > 0.f) ? g[j] : 0.f;
    s1[j] += gg;
    s2[j] = fmaf(gg, xv[j] - mu[j], s2[j]);
  }
}

// forward statistics: sum (x - x0) and sum (x - x0)^2 per channel
template <typename T>
__global__ __launch_bounds__(kThreads) void bn_stats_kernel(const T* __restrict__ x, float* __restrict__ part, int M,
                                                            int C, int tpr, int rp) {
  const int tg = threadIdx.x % tpr, ph = threadIdx.x / tpr;
  const int c = (blockIdx.x * tpr + tg) * 8;
  const bool active = ph < rp && c < C;
  float s1[8], s2[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) s1[j] = s2[j] = 0.f;
  if (active) {
    float sh[8];
    Vec8<T>::load(x + c, sh);
    const int step = rp * gridDim.y;
    // kInFlight rows per iteration, loaded unconditionally (rows past M re-read
    // row 0 and count zero): a load under a branch gets its own vmcnt(0), which
    // serialised the rows one memory round trip at a time
    for (int r = blockIdx.y * rp + ph; r < M; r += kInFlight * step) {
      float v[kInFlight][8];
#pragma unroll
      for (int u = 0; u < kInFlight; ++u) {
        const int ru = r + u * step;
        Vec8<T>::load(x + size_t(ru < M ? ru : 0) * C + c, v[u]);
      }
#pragma unroll
      for (int u = 0; u < kInFlight; ++u) acc_fwd(v[u], sh, r + u * step < M, s1, s2);
    }
  }
  phase_reduce_store(s1, s2, active, tg, ph, tpr, rp, C, PlainStore{part});
}

// backward statistics: sum dz and sum dz * (x - mean) per channel.  dy2 (or null):
// a second gradient of the same output, summed on load -- a residual block's
// input feeds two branches, and the two gradients never need an add pass
template <typename T, bool RELU>
__global__ __launch_bounds__(kThreads) void bn_bwd_stats_kernel(const T* __restrict__ dy, const T* __restrict__ dy2,
                                                                const T* __restrict__ y,
                                                                const T* __restrict__ x,
                                                                const float* __restrict__ mean,
                                                                float* __restrict__ part, int M, int C, int tpr,
                                                                int rp) {
  const int tg = threadIdx.x % tpr, ph = threadIdx.x / tpr;
  const int c = (blockIdx.x * tpr + tg) * 8;
  const bool active = ph < rp && c < C;
  float s1[8], s2[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) s1[j] = s2[j] = 0.f;
  if (active) {
    float mu[8];
    ld8f(mean + c, mu);
    const int step = rp * gridDim.y;
    // kInFlight rows per iteration, loads unconditional (see bn_stats_kernel)
    for (int r = blockIdx.y * rp + ph; r < M; r += kInFlight * step) {
      float g[kInFlight][8], xv[kInFlight][8], yv[kInFlight][8];
#pragma unroll
      for (int u = 0; u < kInFlight; ++u) {
        const int ru = r + u * step;
        const size_t e = size_t(ru < M ? ru : 0) * C + c;
        Vec8<T>::load(dy + e, g[u]);
        Vec8<T>::load(x + e, xv[u]);
        if (RELU) Vec8<T>::load(y + e, yv[u]);
      }
      if (dy2) {
#pragma unroll
        for (int u = 0; u < kInFlight; ++u) {
          const int ru = r + u * step;
          float g2[8];
          Vec8<T>::load(dy2 + size_t(ru < M ? ru : 0) * C + c, g2);
#pragma unroll
          for (int j = 0; j < 8; ++j) g[u][j] += g2[j];
        }
      }
#pragma unroll
      for (int u = 0; u < kInFlight; ++u) acc_bwd<RELU>(g[u], xv[u], yv[u], mu, r + u * step < M, s1, s2);
    }
  }
  phase_reduce_store(s1, s2, active, tg, ph, tpr, rp, C, PlainStore{part});
}

// ---------------------------------------------------------------------------
// Finalize: block = 16 channels x 16 partial-row phases, 8 rows in flight per
// thread (two arrays), then a fixed-order sum over the phases in LDS.  The
// S <= 256 partial rows are read in <= 2 rounds of memory latency (the
// earlier 64 x 4 split needed up to 16 dependent rounds: 5.5 us per call).
// Not merged with fused_reduce_parts below (4 columns per thread x pq phases):
// the two sum the partial rows in different orders, so sharing one would
// change the bits of the other.
// ---------------------------------------------------------------------------
constexpr int kFinCols = 16, kFinPh = kThreads / kFinCols;

P2_DEVICE void reduce_parts(const float* __restrict__ part, int S, int C, int c, float& a, float& b) {
  __shared__ float red[2][kFinPh][kFinCols];
  const int cl = threadIdx.x % kFinCols, q = threadIdx.x / kFinCols;
  float sa = 0.f, sb = 0.f;
  if (c < C) {
    for (int r0 = q; r0 < S; r0 += kFinPh * 8) {
      float ta[8], tb[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int r = r0 + kFinPh * u;
        ta[u] = r < S ? part[size_t(r) * C + c] : 0.f;
        tb[u] = r < S ? part[size_t(S + r) * C + c] : 0.f;
      }
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        sa += ta[u];
        sb += tb[u];
      }
    }
  }
  red[0][q][cl] = sa;
  red[1][q][cl] = sb;
  __syncthreads();
  a = 0.f;
  b = 0.f;
  if (q == 0) {
#pragma unroll
    for (int p = 0; p < kFinPh; ++p) {
      a += red[0][p][cl];
      b += red[1][p][cl];
    }
  }
}

// Forward finalize of channel c from its shifted sums s1 = sum (x - x0), s2 = sum (x - x0)^2:
// mean, rstd, coef = [mean | w rstd | b], running statistics (unbiased variance).
P2_DEVICE void fin_fwd(int c, float s1, float s2, float x0, const float* w, const float* b, float* run_mean,
                       float* run_var, float momentum, float eps, float* mean_out, float* rstd_out, float* coef, int M,
                       int C) {
  const float inv_m = 1.f / float(M);
  const float ms = s1 * inv_m;
  const float v0 = s2 * inv_m - ms * ms;
  const float var = v0 < 0.f ? 0.f : v0;  // a NaN (an Inf or NaN activation) stays a NaN
  const float mu = x0 + ms;
  const float rs = rsqrtf(var + eps);
  mean_out[c] = mu;
  rstd_out[c] = rs;
  coef[c] = mu;
  coef[C + c] = w[c] * rs;
  coef[2 * C + c] = b[c];
  if (run_mean) {
    const float unb = M > 1 ? var * (float(M) / float(M - 1)) : var;
    run_mean[c] = (1.f - momentum) * run_mean[c] + momentum * mu;
    run_var[c] = (1.f - momentum) * run_var[c] + momentum * unb;
  }
}

// Backward finalize of channel c from s1 = sum dz, s2 = sum dz (x - mean):
// db = s1, dw = rstd s2, coef = [A | B | D] with dx = A dz + B (x - mean) + D
P2_DEVICE void fin_bwd(int c, float s1, float s2, const float* w, const float* rstd, float* dw, float* db, float* coef,
                       int M, int C) {
  const float rs = rstd[c], inv_m = 1.f / float(M);
  const float A = w[c] * rs;
  db[c] = s1;
  dw[c] = s2 * rs;
  coef[c] = A;
  coef[C + c] = -A * rs * rs * s2 * inv_m;
  coef[2 * C + c] = -A * s1 * inv_m;
}

template <typename T>
__global__ __launch_bounds__(kThreads) void bn_finalize_fwd_kernel(
    const float* __restrict__ part, int S, const T* __restrict__ x, const float* __restrict__ w,
    const float* __restrict__ b, float* __restrict__ run_mean, float* __restrict__ run_var, int64_t* __restrict__ nbt,
    float momentum, float eps, float* __restrict__ mean_out, float* __restrict__ rstd_out, float* __restrict__ coef,
    int M, int C) {
  const int c = blockIdx.x * kFinCols + (threadIdx.x % kFinCols);
  float s1, s2;
  reduce_parts(part, S, C, c, s1, s2);
  if (threadIdx.x >= kFinCols || c >= C) return;
  fin_fwd(c, s1, s2, Vec8<T>::one(x + c), w, b, run_mean, run_var, momentum, eps, mean_out, rstd_out, coef, M, C);
  if (nbt && c == 0) nbt[0] += 1;
}

__global__ __launch_bounds__(kThreads) void bn_finalize_bwd_kernel(const float* __restrict__ part, int S,
                                                                   const float* __restrict__ w,
                                                                   const float* __restrict__ rstd,
                                                                   float* __restrict__ dw, float* __restrict__ db,
                                                                   float* __restrict__ coef, int M, int C) {
  const int c = blockIdx.x * kFinCols + (threadIdx.x % kFinCols);
  float s1, s2;
  reduce_parts(part, S, C, c, s1, s2);
  if (threadIdx.x >= kFinCols || c >= C) return;
  fin_bwd(c, s1, s2, w, rstd, dw, db, coef, M, C);
}

// ---------------------------------------------------------------------------
// Apply passes: 8 channels per thread, grid-stride over the [M, C] matrix.
// ---------------------------------------------------------------------------
template <typename T, bool RELU, bool RES>
__global__ __launch_bounds__(kThreads) void bn_apply_fwd_kernel(const T* __restrict__ x, const T* __restrict__ res,
                                                                const float* __restrict__ c_mean,
                                                                const float* __restrict__ c_scale,
                                                                const float* __restrict__ c_bias,
                                                                const float* __restrict__ run_var, float eps,
                                                                T* __restrict__ y, int64_t n8, int C) {
  // training: (mean, scale, bias) = the finalize kernel's coefficients;
  // inference (run_var != null): (running_mean, weight, bias), scale = w * rsqrt(running_var + eps)
  for (int64_t i = blockIdx.x * int64_t(kThreads) + threadIdx.x; i < n8; i += int64_t(gridDim.x) * kThreads) {
    const int64_t e = i * 8;
    const int c = int(e % C);
    float v[8], mu[8], sc[8], bb[8];
    Vec8<T>::load(x + e, v);
    ld8f(c_mean + c, mu);
    ld8f(c_scale + c, sc);
    ld8f(c_bias + c, bb);
    if (run_var) {
      float rv[8];
      ld8f(run_var + c, rv);
#pragma unroll
      for (int j = 0; j < 8; ++j) sc[j] *= rsqrtf(rv[j] + eps);
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = fmaf(v[j] - mu[j], sc[j], bb[j]);
    if (RES) {
      float r[8];
      Vec8<T>::load(res + e, r);
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] += r[j];
    }
    if (RELU) {
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = v[j] < 0.f ? 0.f : v[j];  // not fmaxf: a NaN stays a NaN
    }
    Vec8<T>::store(y + e, v);
  }
}

template <typename T, bool RELU, bool RES>
__global__ __launch_bounds__(kThreads) void bn_apply_bwd_kernel(const T* __restrict__ dy, const T* __restrict__ dy2,
                                                                const T* __restrict__ y,
                                                                const T* __restrict__ x,
                                                                const float* __restrict__ mean,
                                                                const float* __restrict__ coef, T* __restrict__ dx,
                                                                T* __restrict__ dres, int64_t n8, int C) {
  for (int64_t i = blockIdx.x * int64_t(kThreads) + threadIdx.x; i < n8; i += int64_t(gridDim.x) * kThreads) {
    const int64_t e = i * 8;
    const int c = int(e % C);
    float g[8], xv[8], mu[8], A[8], B[8], D[8];
    Vec8<T>::load(dy + e, g);
    Vec8<T>::load(x + e, xv);
    if (dy2) {
      float g2[8];
      Vec8<T>::load(dy2 + e, g2);
#pragma unroll
      for (int j = 0; j < 8; ++j) g[j] += g2[j];
    }
    if (RELU) {
      float yv[8];
      Vec8<T>::load(y + e, yv);
#pragma unroll
      for (int j = 0; j < 8; ++j) g[j] = yv[j] > 0.f ? g[j] : 0.f;
    }
    ld8f(mean + c, mu);
    ld8f(coef + c, A);
    ld8f(coef + C + c, B);
    ld8f(coef + 2 * C + c, D);
    if (RES) Vec8<T>::store(dres + e, g);
    float o[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) o[j] = fmaf(A[j], g[j], fmaf(B[j], xv[j] - mu[j], D[j]));
    Vec8<T>::store(dx + e, o);
  }
}

// ---------------------------------------------------------------------------
// Statistics + finalize in ONE launch (bf16, C <= 2048, small activations).
// On the ResNet CIFAR shapes each BN pass above is a few us of latency (a
// handful of dependent memory rounds, ~5 us per launch in
// profiles/r3_resnet18_native_steady_state.md), not of bandwidth, so the
// separate finalize launch costs as much as the statistics pass itself.  Here
// every thread loads all kFuseRows of its rows at once, the block writes its
// partial-sum row with sc1 (write-through) stores, and the LAST block to
// arrive (relaxed agent-scope ticket, the split-K hand-off of gemm_core.h: no
// fences) reduces the [S, C] partials in fixed order (sc1 loads) and writes
// the statistics and the apply coefficients.  No block ever waits for
// another (no grid barrier, nothing to deadlock against concurrent streams);
// the apply pass stays its own launch.  Counter: 1 int, zero on entry and on
// exit (ops/splitk.py ring).
// ---------------------------------------------------------------------------
constexpr int kFuseRows = 8;          // rows per thread, all in flight
constexpr int kFuseMaxPart = 16384;   // S * C: the last block reads <= 128 KB of partials

P2_DEVICE __amdgpu_buffer_rsrc_t f32_rsrc(const float* p, int n) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p), 0, n * 4, 0x00020000);
}

// phase_reduce_store's store for these kernels: sc1 (write-through) buffer stores
struct Sc1Store {
  __amdgpu_buffer_rsrc_t rs;
  P2_DEVICE void operator()(size_t i, float v) const {
    __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v), rs, int(i) * 4, 0, 16);
  }
};

// Ticket: true in the one block that arrived last (every block drained its
// sc1 partial stores before taking its ticket); it resets the counter.
P2_DEVICE bool fused_arrive(int* ctr, int total) {
  __shared__ int last;
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (threadIdx.x == 0) {
    const int old = __hip_atomic_fetch_add(ctr, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    last = old == total - 1;
    if (last) __hip_atomic_store(ctr, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  __syncthreads();
  return last;
}

// Fixed-order sum of the S partial rows of (a, b), 4 consecutive columns per
// thread and pq row phases, 8 rows per phase in flight; calls fn(c0, a, b)
// once per 4-column group.
template <class Fn>
P2_DEVICE void fused_reduce_parts(const float* part, int S, int C, Fn&& fn) {
  __shared__ f32x4 red[2][kThreads];
  const auto rs = f32_rsrc(part, 2 * S * C);
  const int nc4 = C / 4;
  const bool narrow = nc4 <= kThreads;
  const int pq = narrow ? kThreads / nc4 : 1;
  const int cl = narrow ? threadIdx.x % nc4 : threadIdx.x, q = narrow ? threadIdx.x / nc4 : 0;
  for (int base = 0; base < nc4; base += kThreads) {  // a second round only when C > 1024
    const int c4 = base + cl;
    const bool on = q < pq && c4 < nc4;
    f32x4 a = {0.f, 0.f, 0.f, 0.f}, b = a;
    if (on) {
      for (int r0 = q; r0 < S; r0 += 8 * pq) {
        f32x4 ta[8], tb[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          const int r = r0 + u * pq;
          const bool in = r < S;
          ta[u] = in ? __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rs, (r * C + 4 * c4) * 4, 0, 16))
                     : f32x4{0.f, 0.f, 0.f, 0.f};
          tb[u] = in ? __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rs, ((S + r) * C + 4 * c4) * 4, 0, 16))
                     : f32x4{0.f, 0.f, 0.f, 0.f};
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          a += ta[u];
          b += tb[u];
        }
      }
    }
    __syncthreads();
    red[0][threadIdx.x] = a;
    red[1][threadIdx.x] = b;
    __syncthreads();
    if (on && q == 0) {
      f32x4 sa = {0.f, 0.f, 0.f, 0.f}, sb = sa;
      for (int p = 0; p < pq; ++p) {
        sa += red[0][p * nc4 + cl];
        sb += red[1][p * nc4 + cl];
      }
      fn(4 * c4, sa, sb);
    }
  }
}

// forward: statistics + finalize (coef / mean / rstd / running stats as bn_finalize_fwd_kernel)
__global__ __launch_bounds__(kThreads) void bn_stats_fin_kernel(
    const uint16_t* __restrict__ x, const float* __restrict__ w, const float* __restrict__ b,
    float* __restrict__ run_mean, float* __restrict__ run_var, int64_t* __restrict__ nbt, float momentum, float eps,
    float* __restrict__ mean_out, float* __restrict__ rstd_out, float* __restrict__ coef, float* part, int* ctr, int M,
    int C, int tpr, int rp) {
  const int tg = threadIdx.x % tpr, ph = threadIdx.x / tpr, c = tg * 8, S = gridDim.y;
  const bool active = ph < rp;
  const int r0 = blockIdx.y * rp * kFuseRows + ph;
  float s1[8], s2[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) s1[j] = s2[j] = 0.f;
  if (active) {
    float sh[8];
    Vec8<uint16_t>::load(x + c, sh);
    uint4 xv[kFuseRows];
#pragma unroll
    for (int k = 0; k < kFuseRows; ++k) {
      const int r = r0 + k * rp;
      xv[k] = r < M ? *reinterpret_cast<const uint4*>(x + size_t(r) * C + c) : uint4{0, 0, 0, 0};
    }
#pragma unroll
    for (int k = 0; k < kFuseRows; ++k) {
      float v[8];
      Vec8<uint16_t>::unpack(xv[k], v);
      acc_fwd(v, sh, r0 + k * rp < M, s1, s2);
    }
  }
  phase_reduce_store(s1, s2, active, tg, ph, tpr, rp, C, Sc1Store{f32_rsrc(part, 2 * S * C)});
  if (!fused_arrive(ctr, S)) return;
  fused_reduce_parts(part, S, C, [&](int c0, const f32x4& sa, const f32x4& sb) {
#pragma unroll
    for (int e = 0; e < 4; ++e)
      fin_fwd(c0 + e, sa[e], sb[e], Vec8<uint16_t>::one(x + c0 + e), w, b, run_mean, run_var, momentum, eps, mean_out,
              rstd_out, coef, M, C);
  });
  if (nbt && threadIdx.x == 0) nbt[0] += 1;
}

// backward: statistics + finalize (dw / db / coef as bn_finalize_bwd_kernel)
template <bool RELU>
__global__ __launch_bounds__(kThreads) void bn_bwd_stats_fin_kernel(
    const uint16_t* __restrict__ dy, const uint16_t* __restrict__ y, const uint16_t* __restrict__ x,
    const float* __restrict__ w, const float* __restrict__ mean, const float* __restrict__ rstd,
    float* __restrict__ dw, float* __restrict__ db, float* __restrict__ coef, float* part, int* ctr, int M, int C,
    int tpr, int rp) {
  const int tg = threadIdx.x % tpr, ph = threadIdx.x / tpr, c = tg * 8, S = gridDim.y;
  const bool active = ph < rp;
  const int r0 = blockIdx.y * rp * kFuseRows + ph;
  float s1[8], s2[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) s1[j] = s2[j] = 0.f;
  if (active) {
    float mu[8];
    ld8f(mean + c, mu);
    uint4 gv[kFuseRows], xv[kFuseRows], yv[kFuseRows];
#pragma unroll
    for (int k = 0; k < kFuseRows; ++k) {
      const int r = r0 + k * rp;
      const bool in = r < M;
      gv[k] = in ? *reinterpret_cast<const uint4*>(dy + size_t(r) * C + c) : uint4{0, 0, 0, 0};
      xv[k] = in ? *reinterpret_cast<const uint4*>(x + size_t(r) * C + c) : uint4{0, 0, 0, 0};
      if (RELU) yv[k] = in ? *reinterpret_cast<const uint4*>(y + size_t(r) * C + c) : uint4{0, 0, 0, 0};
    }
#pragma unroll
    for (int k = 0; k < kFuseRows; ++k) {
      float g[8], xf[8], yf[8];
      Vec8<uint16_t>::unpack(gv[k], g);
      Vec8<uint16_t>::unpack(xv[k], xf);
      if (RELU) Vec8<uint16_t>::unpack(yv[k], yf);
      acc_bwd<RELU>(g, xf, yf, mu, r0 + k * rp < M, s1, s2);
    }
  }
  phase_reduce_store(s1, s2, active, tg, ph, tpr, rp, C, Sc1Store{f32_rsrc(part, 2 * S * C)});
  if (!fused_arrive(ctr, S)) return;
  fused_reduce_parts(part, S, C, [&](int c0, const f32x4& sa, const f32x4& sb) {
#pragma unroll
    for (int e = 0; e < 4; ++e) fin_bwd(c0 + e, sa[e], sb[e], w, rstd, dw, db, coef, M, C);
  });
}

// ---------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------
BnPlan bn_fused_plan(int M, int C) {
  BnPlan p{};
  const int groups = C / 8;
  if (C % 8 || groups > kThreads) return p;  // S = 0: not eligible
  p.tpr = groups;
  p.rp = kThreads / groups;
  p.gx = 1;
  const int64_t S = (int64_t(M) + int64_t(p.rp) * kFuseRows - 1) / (int64_t(p.rp) * kFuseRows);
  if (S < 1 || S * C > kFuseMaxPart) return p;
  p.S = int(S);
  return p;
}

BnPlan bn_plan(int M, int C) {
  BnPlan p{};
  const int groups = C / 8;
  p.tpr = groups < kThreads ? groups : kThreads;
  p.rp = kThreads / p.tpr;
  p.gx = (groups + p.tpr - 1) / p.tpr;
  // >= 4 rows per thread, <= 256 row splits, <= ~1024 blocks in total
  int S = (M + 4 * p.rp - 1) / (4 * p.rp);
  const int cap = 1024 / p.gx > 256 ? 256 : (1024 / p.gx < 1 ? 1 : 1024 / p.gx);
  if (S > cap) S = cap;
  p.S = S < 1 ? 1 : S;
  return p;
}

// Runtime flags as template booleans: fn receives std::true_type / std::false_type values.
template <class Fn>
static void with_flag(bool a, Fn&& fn) {
  a ? fn(std::true_type{}) : fn(std::false_type{});
}
template <class Fn>
static void with_flags(bool a, bool b, Fn&& fn) {
  with_flag(a, [&](auto A) { with_flag(b, [&](auto B) { fn(A, B); }); });
}
// fn receives a value of the activation's element type
template <class Fn>
static void with_dtype(bool bf16, Fn&& fn) {
  bf16 ? fn(uint16_t{}) : fn(float{});
}

constexpr dim3 kBlock(kThreads);
static dim3 fin_grid(int C) { return dim3((C + kFinCols - 1) / kFinCols); }

// training: (mean, scale, bias) = the finalize kernel's coefficient rows, run_var null;
// inference: (running_mean, weight, bias) and run_var
template <typename T>
static void apply_fwd(const T* x, const T* r, const float* mean, const float* scale, const float* bias,
                      const float* run_var, float eps, T* y, int M, int C, bool relu, hipStream_t s) {
  const int64_t n8 = int64_t(M) * C / 8;
  with_flags(relu, r != nullptr, [&](auto RELU, auto RES) {
    hipLaunchKernelGGL((bn_apply_fwd_kernel<T, RELU.value, RES.value>), dim3(stream_grid(n8, kThreads)), kBlock, 0, s, x, r,
                       mean, scale, bias, run_var, eps, y, n8, C);
  });
}

template <typename T>
static void apply_bwd(const T* dy, const T* dy2, const T* y, const T* x, const float* mean, const float* coef, T* dx,
                      T* dres, int M, int C, bool relu, hipStream_t s) {
  const int64_t n8 = int64_t(M) * C / 8;
  with_flags(relu, dres != nullptr, [&](auto RELU, auto RES) {
    hipLaunchKernelGGL((bn_apply_bwd_kernel<T, RELU.value, RES.value>), dim3(stream_grid(n8, kThreads)), kBlock, 0, s, dy,
                       dy2, y, x, mean, coef, dx, dres, n8, C);
  });
}

void bn_fwd_train(bool bf16, const void* xv, const void* res, const float* w, const float* b, float* run_mean,
                  float* run_var, int64_t* nbt, float momentum, float eps, void* yv, float* mean, float* rstd,
                  float* coef, float* part, int* ctr, int M, int C, bool relu, hipStream_t s) {
  with_dtype(bf16, [&](auto t) {
    using T = decltype(t);
    const T* x = static_cast<const T*>(xv);
    bool one_launch = false;
    if constexpr (sizeof(T) == 2) {
      const BnPlan f = bn_fused_plan(M, C);
      one_launch = ctr && f.S > 0;
      if (one_launch)
        hipLaunchKernelGGL(bn_stats_fin_kernel, dim3(1, f.S), kBlock, 0, s, x, w, b, run_mean, run_var, nbt, momentum, eps,
                           mean, rstd, coef, part, ctr, M, C, f.tpr, f.rp);
    }
    if (!one_launch) {
      const BnPlan p = bn_plan(M, C);
      hipLaunchKernelGGL(bn_stats_kernel<T>, dim3(p.gx, p.S), kBlock, 0, s, x, part, M, C, p.tpr, p.rp);
      hipLaunchKernelGGL(bn_finalize_fwd_kernel<T>, fin_grid(C), kBlock, 0, s, part, p.S, x, w, b, run_mean, run_var, nbt,
                         momentum, eps, mean, rstd, coef, M, C);
    }
    apply_fwd(x, static_cast<const T*>(res), coef, coef + C, coef + 2 * C, nullptr, 0.f, static_cast<T*>(yv), M, C, relu, s);
  });
}

void bn_apply_train(bool bf16, const void* x, const void* res, const float* coef, void* y, int M, int C, bool relu,
                    hipStream_t s) {
  with_dtype(bf16, [&](auto t) {
    using T = decltype(t);
    apply_fwd(static_cast<const T*>(x), static_cast<const T*>(res), coef, coef + C, coef + 2 * C, nullptr, 0.f,
              static_cast<T*>(y), M, C, relu, s);
  });
}

void bn_fwd_eval(bool bf16, const void* x, const void* res, const float* w, const float* b, const float* run_mean,
                 const float* run_var, float eps, void* y, int M, int C, bool relu, hipStream_t s) {
  with_dtype(bf16, [&](auto t) {
    using T = decltype(t);
    apply_fwd(static_cast<const T*>(x), static_cast<const T*>(res), run_mean, w, b, run_var, eps, static_cast<T*>(y), M, C,
              relu, s);
  });
}

void bn_apply_bwd_only(const void* dy, const void* y, const void* x, const float* mean, const float* coef, void* dx,
                       int M, int C, bool relu, hipStream_t s) {
  using T = uint16_t;
  apply_bwd<T>(static_cast<const T*>(dy), nullptr, static_cast<const T*>(y), static_cast<const T*>(x), mean, coef,
               static_cast<T*>(dx), nullptr, M, C, relu, s);
}

void bn_bwd(bool bf16, const void* dyv, const void* dy2v, const void* yv, const void* xv, const float* w,
            const float* mean, const float* rstd, void* dx, void* dres, float* dw, float* db, float* coef, float* part,
            int* ctr, int M, int C, bool relu, hipStream_t s) {
  with_dtype(bf16, [&](auto t) {
    using T = decltype(t);
    const T *dy = static_cast<const T*>(dyv), *dy2 = static_cast<const T*>(dy2v);
    const T *y = static_cast<const T*>(yv), *x = static_cast<const T*>(xv);
    bool one_launch = false;
    if constexpr (sizeof(T) == 2) {
      const BnPlan f = bn_fused_plan(M, C);
      one_launch = ctr && f.S > 0 && !dy2;
      if (one_launch)
        with_flag(relu, [&](auto RELU) {
          hipLaunchKernelGGL(bn_bwd_stats_fin_kernel<RELU.value>, dim3(1, f.S), kBlock, 0, s, dy, y, x, w, mean, rstd, dw,
                             db, coef, part, ctr, M, C, f.tpr, f.rp);
        });
    }
    if (!one_launch) {
      const BnPlan p = bn_plan(M, C);
      with_flag(relu, [&](auto RELU) {
        hipLaunchKernelGGL((bn_bwd_stats_kernel<T, RELU.value>), dim3(p.gx, p.S), kBlock, 0, s, dy, dy2, y, x, mean, part,
                           M, C, p.tpr, p.rp);
      });
      hipLaunchKernelGGL(bn_finalize_bwd_kernel, fin_grid(C), kBlock, 0, s, part, p.S, w, rstd, dw, db, coef, M, C);
    }
    apply_bwd(dy, dy2, y, x, mean, coef, static_cast<T*>(dx), static_cast<T*>(dres), M, C, relu, s);
  });
}

}  // namespace p2bn
