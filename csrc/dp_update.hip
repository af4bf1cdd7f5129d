// Differentially private model updates: the Gaussian mechanism on the update
// delta = w - w0 of a flat fp32 arena (w: the trained weights, w0: the weights
// the round started from), as two streaming passes.
//
//   dp_delta_sqnorm   ss = sum (w[i] - w0[i])^2 over the privatised elements
//   dp_apply          out[i] = base[i] + sigma * g[i]         (privatised)
//                     out[i] = w[i]                           (everything else)
//     base = w                         if ss <= C^2   (no clipping: bitwise w)
//     base = w0 + s * (w - w0)         else, s = C / sqrt(ss)
//
// Which elements are privatised comes from a block table, one byte per
// 64-element block: byte c = the first c elements of the block (0: none, an
// exempt block; 64: all; 1..63: the last block of a tensor, whose padding is
// copied through).  Any byte >= 64 means the whole block: the table is only
// compared against, never used as an index.  One DPP row of 16 lanes owns one
// block (4 elements per lane, one 16-byte access), as in quant_wire.hip.
//
// Arithmetic of the apply pass, so that an fp32 reference reproduces `base`
// bit for bit: C^2 is one fp32 multiply, sqrt and the division are correctly
// rounded, and every multiply and add below is a separate, singly rounded
// operation.  __fmul_rn / __fadd_rn are plain `*` / `+` in this toolchain's
// headers, which a -ffp-contract=fast build would still fuse into an fma:
// setup.py compiles this one file with -ffp-contract=on, which contracts only
// inside one source expression and so never across these calls.
//
// Noise g is a function of (seed, round, element index) alone -- not of the
// grid, the stream or the launch: Philox4x32-10 with key (seed low, seed high)
// and counter (q low, q high, round, 0) for the element group q = i / 4; its
// four words r0..r3 give g[4q .. 4q+3] as the Box-Muller pairs (r0, r1) and
// (r2, r3):
//   u = ((ra >> 8) + 1) * 2^-24   in (0, 1], exact in fp32
//   t = (rb >> 8) * 2^-24         in [0, 1)
//   rad = sqrtf(-2 logf(u)),  pair = (rad cospif(2t), rad sinpif(2t))
// with the accurate library functions (the guarantee rests on the tail of the
// distribution, which the fast intrinsics bend).  The smallest u is 2^-24, so
// |g| <= sqrt(48 ln 2) ~= 5.77: the sampled Gaussian is truncated there.
//
// Traffic: 8n bytes for the norm pass (exempt blocks are not read), 12n + n/64
// for the apply pass.  The norm is reduced lane -> wave (DPP) -> block (LDS) ->
// grid (partials + a one-block finish launch) in a fixed order without
// atomics, on a grid that is a function of n alone: the same inputs give the
// bitwise-same ss on every node and every stream.
#include <string>

#include "arena_io.h"

namespace p2 {

namespace {

constexpr int kDpBlock = 64;

P2_DEVICE f32x4 ld4(const float* p, int64_t q) {
  return __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(p) + q);
}

// ---------------------------------------------------------------------------
// norm pass
// ---------------------------------------------------------------------------
// nq = n / 4 lane slots, a multiple of 16; slot q holds elements 4q .. 4q+3 of
// block q / 16.  The loop bound may split a wave, so the reductions come after
// the loop, where every lane is active again.
__global__ __launch_bounds__(256) void dp_sqnorm_kernel(const float* __restrict__ w, const float* __restrict__ w0,
                                                        const uint8_t* __restrict__ table, int64_t nq,
                                                        float* __restrict__ partials) {
  float acc = 0.f;
  const int64_t stride = int64_t(gridDim.x) * blockDim.x;
  for (int64_t q = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; q < nq; q += stride) {
    const int c = table[q >> 4];          // uniform over the row
    const int first = int(q & 15) * 4;    // this lane's first element inside the block
    if (c > first) {
      const f32x4 a = ld4(w, q), b = ld4(w0, q);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float d = a[j] - b[j];
        if (first + j < c) acc = fmaf(d, d, acc);
      }
    }
  }
  __shared__ float red[4];
  const float s = wave_sum(acc);
  if (threadIdx.x % kWave == 0) red[threadIdx.x / kWave] = s;
  __syncthreads();
  if (threadIdx.x == 0) partials[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

// one block: lane t adds partials[t], [t + 256], ... in index order, then the
// wave and block reductions as above
__global__ __launch_bounds__(256) void dp_sqnorm_finish_kernel(const float* __restrict__ partials, int nblocks,
                                                               float* __restrict__ out) {
  float s = 0.f;
  for (int b = threadIdx.x; b < nblocks; b += blockDim.x) s += partials[b];
  s = wave_sum(s);
  __shared__ float red[4];
  if (threadIdx.x % kWave == 0) red[threadIdx.x / kWave] = s;
  __syncthreads();
  if (threadIdx.x == 0) out[0] = (red[0] + red[1]) + (red[2] + red[3]);
}

// ---------------------------------------------------------------------------
// noise
// ---------------------------------------------------------------------------
struct Philox4 {
  uint32_t r[4];
};

// Philox4x32-10 (Salmon et al., SC'11; the Random123 constants)
P2_DEVICE Philox4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
  constexpr uint32_t kM0 = 0xD2511F53u, kM1 = 0xCD9E8D57u, kW0 = 0x9E3779B9u, kW1 = 0xBB67AE85u;
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    // one 32 x 32 -> 64-bit multiply per product (v_mad_u64_u32), not a low and a high half
    const uint64_t p0 = uint64_t(kM0) * c0, p1 = uint64_t(kM1) * c2;
    c0 = uint32_t(p1 >> 32) ^ c1 ^ k0;
    c1 = uint32_t(p1);
    c2 = uint32_t(p0 >> 32) ^ c3 ^ k1;
    c3 = uint32_t(p0);
    k0 += kW0;
    k1 += kW1;
  }
  return Philox4{{c0, c1, c2, c3}};
}

P2_DEVICE void box_muller(uint32_t ra, uint32_t rb, float& g0, float& g1) {
  const float u = float((ra >> 8) + 1u) * 0x1p-24f;  // both exact: 24-bit integers
  const float t2 = float(rb >> 8) * 0x1p-23f;        // 2 t, exact
  const float rad = sqrtf(-2.f * logf(u));
  float sn, cs;
  sincospif(t2, &sn, &cs);
  g0 = __fmul_rn(rad, cs);
  g1 = __fmul_rn(rad, sn);
}

// ---------------------------------------------------------------------------
// apply pass
// ---------------------------------------------------------------------------
template <bool NOISE>
__global__ __launch_bounds__(256) void dp_apply_kernel(const float* __restrict__ w, const float* __restrict__ w0,
                                                       const uint8_t* __restrict__ table,
                                                       const float* __restrict__ ss_ptr, float clip, float sigma,
                                                       uint32_t k0, uint32_t k1, uint32_t round, int64_t nq,
                                                       float* __restrict__ out) {
  const float ss = ss_ptr[0];
  const bool clipped = !(ss <= __fmul_rn(clip, clip));  // grid-uniform; a NaN norm clips (and gives NaN)
  const float s = clipped ? __fdiv_rn(clip, sqrtf(ss)) : 1.f;
  const int64_t stride = int64_t(gridDim.x) * blockDim.x;
  for (int64_t q = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; q < nq; q += stride) {
    const int c = table[q >> 4];
    const int first = int(q & 15) * 4;
    const f32x4 a = ld4(w, q);
    f32x4 y = a;
    if (c > first) {
      if (clipped) {
        const f32x4 b = ld4(w0, q);
#pragma unroll
        for (int j = 0; j < 4; ++j) y[j] = __fadd_rn(b[j], __fmul_rn(s, __fadd_rn(a[j], -b[j])));
      }
      if (NOISE) {
        const Philox4 p = philox4x32_10(uint32_t(q), uint32_t(uint64_t(q) >> 32), round, 0u, k0, k1);
        float g[4];
        box_muller(p.r[0], p.r[1], g[0], g[1]);
        box_muller(p.r[2], p.r[3], g[2], g[3]);
#pragma unroll
        for (int j = 0; j < 4; ++j) y[j] = __fadd_rn(y[j], __fmul_rn(sigma, g[j]));
      }
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (first + j >= c) y[j] = a[j];  // a tensor's padding: copied through
    }
    reinterpret_cast<f32x4*>(out)[q] = y;
  }
}

void check_n(int64_t n, const char* op) {
  if (n < kDpBlock || n % kDpBlock) throw std::invalid_argument(std::string(op) + ": n must be a positive multiple of 64");
}

}  // namespace

int dp_sqnorm_blocks(int64_t n) { return stream_grid(n / 4, 256); }

void dp_delta_sqnorm(const float* w, const float* w0, const uint8_t* table, int64_t n, float* partials, float* out,
                     hipStream_t s) {
  check_n(n, "dp_delta_sqnorm");
  const int blocks = dp_sqnorm_blocks(n);
  hipLaunchKernelGGL(dp_sqnorm_kernel, dim3(blocks), dim3(256), 0, s, w, w0, table, n / 4, partials);
  hipLaunchKernelGGL(dp_sqnorm_finish_kernel, dim3(1), dim3(256), 0, s, partials, blocks, out);
}

void dp_apply(const float* w, const float* w0, const uint8_t* table, const float* sqnorm, float clip, float sigma,
              uint64_t seed, uint32_t round, float* out, int64_t n, hipStream_t s) {
  check_n(n, "dp_apply");
  if (!(clip > 0.f) || !(sigma >= 0.f)) throw std::invalid_argument("dp_apply: clip must be > 0 and sigma >= 0");
  const dim3 grid(stream_grid(n / 4, 256)), block(256);
  const uint32_t k0 = uint32_t(seed), k1 = uint32_t(seed >> 32);
  if (sigma > 0.f)
    hipLaunchKernelGGL(dp_apply_kernel<true>, grid, block, 0, s, w, w0, table, sqnorm, clip, sigma, k0, k1, round,
                       n / 4, out);
  else
    hipLaunchKernelGGL(dp_apply_kernel<false>, grid, block, 0, s, w, w0, table, sqnorm, clip, sigma, k0, k1, round,
                       n / 4, out);
}

}  // namespace p2
