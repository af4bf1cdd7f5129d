// Host-side launch API of the p2pfl_amd HIP kernels (raw pointers + stream;
// no torch headers, so kernel files compile fast and stay reusable from C++).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace p2 {

constexpr int kMaxInputs = 16;

// out[i] = scale * (acc_in[i] + sum_j weights[j] * srcs[j][i]), fp32
// accumulation in input order (acc_in: fp32 running sum or null = 0; it may
// alias out).  Each src fp32 or bf16 (src_bf16[j]); out fp32 or bf16; k may be
// 0 (just scale acc_in) and may exceed kMaxInputs (fp32 out only).  Folding a
// set of inputs in several calls (running sum, scale on the last) gives the
// bitwise-same result as one call over all of them.
void weighted_sum(const void* const* srcs, const int* src_bf16, const float* weights, int k, const float* acc_in,
                  float scale, void* out, int out_bf16, int64_t n, hipStream_t s);

// Robust aggregation (robust_agg.hip).  Both take up to kMaxInputs arenas of n
// elements (trimmed_mean at least 1, pairwise_sqdist at least 2), each fp32 or
// bf16, and throw std::invalid_argument outside that range.
//
// out[i] = mean of the values {srcs[j][i]} left after dropping the trim lowest
// and trim highest, 0 <= trim <= (k - 1) / 2, added in ascending order in fp32
// (independent of the order of srcs).  trim = (k - 1) / 2 is the median (mean
// of the two middle values for even k), trim = 0 the plain mean.
void trimmed_mean(const void* const* srcs, const int* src_bf16, int k, int trim, void* out, int out_bf16, int64_t n,
                  hipStream_t s);
// out[k][k] (fp32, symmetric, zero diagonal) = squared L2 distances between
// the arenas, each arena read once.  partials: k (k - 1) / 2 *
// pairwise_sqdist_blocks(n) floats of workspace.  Reductions run in a fixed
// order (no atomics): the same inputs give the bitwise-same matrix.
int pairwise_sqdist_blocks(int64_t n);
void pairwise_sqdist(const void* const* srcs, const int* src_bf16, int k, float* partials, float* out, int64_t n,
                     hipStream_t s);

// Block-quantised int8 wire (quant_wire.hip).  packed: 64 nb int8 codes, then
// the 256 R bytes of the R raw blocks as fp32, then nb fp32 scales, nb =
// ceil(n / 64); 16-byte aligned.  raw_ids: device table of R sorted, unique
// block indices below nb (may be null when R = 0).  Encode: per block scale =
// amax / 127, code = clamp(rint(x / scale), -127, 127); a block holding NaN or
// Inf gets a NaN scale, one below 127 FLT_MIN a zero scale (codes 0 in both).
// Decode: float(code) * scale, then the raw blocks exactly.  Any n >= 1; src /
// out fp32 or bf16.  Both throw std::invalid_argument for n < 1 or R < 0.
void q8_encode(const void* src, int src_bf16, int64_t n, const int32_t* raw_ids, int R, uint8_t* packed,
               hipStream_t s);
void q8_decode(const uint8_t* packed, int64_t n, const int32_t* raw_ids, int R, void* out, int out_bf16,
               hipStream_t s);

// Differentially private updates (dp_update.hip): the Gaussian mechanism on
// delta = w - w0.  w, w0, out: fp32 arenas of n elements, n a positive multiple
// of 64, 16-byte aligned; table: n / 64 bytes, byte c = the first c elements of
// that 64-element block are privatised, the rest copied through (0: an exempt
// block).  Both throw std::invalid_argument for any other n.
//
// out[0] = sum (w[i] - w0[i])^2 over the privatised elements, fp32.  partials:
// dp_sqnorm_blocks(n) floats of workspace.  Fixed-order reductions, no atomics,
// a grid that depends on n alone: the same inputs give the bitwise-same sum.
int dp_sqnorm_blocks(int64_t n);
void dp_delta_sqnorm(const float* w, const float* w0, const uint8_t* table, int64_t n, float* partials, float* out,
                     hipStream_t s);
// Privatised elements: out = base + sigma * g, base = w if *sqnorm <= clip^2
// (bitwise) else w0 + (clip / sqrt(*sqnorm)) * (w - w0), every operation singly
// rounded; g: Philox4x32-10 (key = seed, counter = (i / 4, round)) through
// Box-Muller, |g| <= 5.77, a function of (seed, round, i) alone.  sigma = 0
// launches a kernel without any noise code.  Everything else: out = w bitwise.
// out must not overlap w or w0.  Throws unless clip > 0 and sigma >= 0.
void dp_apply(const float* w, const float* w0, const uint8_t* table, const float* sqnorm, float clip, float sigma,
              uint64_t seed, uint32_t round, float* out, int64_t n, hipStream_t s);

struct AdamParams {
  float lr, beta1, beta2, eps, weight_decay;
  // both from the float32 lr / beta1 / beta2 above (the values m and v accumulate with),
  // evaluated in double and rounded once
  float step_size;     // lr / (1 - beta1^t)
  float inv_sqrt_bc2;  // 1 / sqrt(1 - beta2^t)
  int decoupled;
  // multi-tensor kernel only: when set, t = *t_dev and the two bias
  // corrections above are computed on the device (graph-replayable steps)
  const int* t_dev;
};
void adam_step(float* p, const float* g, float* m, float* v, uint16_t* p_bf16, int64_t n, const AdamParams& h,
               hipStream_t s);

struct SgdParams {
  float lr, momentum, dampening, weight_decay;
  int nesterov, first_step;
};
void sgd_step(float* p, const float* g, float* buf, uint16_t* p_bf16, int64_t n, const SgdParams& h, hipStream_t s);

// Multi-tensor optimizer steps (mixed-precision learners, optim.hip).
constexpr int kMTChunk = 4096;  // elements per block (dense tensors)
constexpr int kMTMaxCL = 4608;  // elements per block of a channels-last tensor staged through LDS
                                // (whole output-channel slabs: the largest ResNet slab is 512 x 3 x 3)
constexpr int kMTGradBf16 = 1;  // gradient tensor is bf16 (else fp32)
constexpr int kMTShadow = 2;    // also write the bf16 shadow of the weight
constexpr int kMTPermCL = 4;    // grad + shadow in channels-last (O, kh, kw, I) order; fp32 state OIHW.
                                // flags bits 8..31 = I, bits 32..55 = kh * kw
// Tables built by p2pfl_amd/learning/optim.py mt_tables(): chunks are int32
// (tensor, first element) pairs; a block covers [first, first + min(chunk, n - first)).
struct MTTensor {
  int64_t off;    // element offset in the flat arenas
  int64_t n;      // elements
  int64_t flags;
  int64_t chunk;  // elements per block (kMTChunk, or whole (I, kh, kw) slabs for the LDS-staged path)
};
void adam_mt_step(float* p, float* m, float* v, uint16_t* p_bf16, const MTTensor* tens, const int2* chunks,
                  int n_chunks, const uint64_t* grad_ptrs, const AdamParams& h, hipStream_t s);
void sgd_mt_step(float* p, float* buf, uint16_t* p_bf16, const MTTensor* tens, const int2* chunks, int n_chunks,
                 const uint64_t* grad_ptrs, const SgdParams& h, hipStream_t s);

}  // namespace p2
