// Block-quantised int8 model wire ("q8"): int8 codes with one fp32 scale per
// 64-element block of a flat parameter arena, plus an exact fp32 copy of the
// blocks listed as raw (biases, norm parameters and statistics).
//
// Packed buffer (uint8, 16-byte aligned), nb = ceil(n / 64) blocks, R raw blocks:
//   codes   [0, 64 nb)                     int8, element i at byte i, padding 0
//   raw     [64 nb, 64 nb + 256 R)         fp32, the 64 values of each raw block
//   scales  [64 nb + 256 R, .. + 4 nb)     fp32, one per block
//
// Encode, per block (IEEE binary32; bf16 input widened exactly):
//   any NaN / Inf      -> scale = quiet NaN, codes 0 (the block decodes to NaN)
//   amax < 127 FLT_MIN -> scale = 0, codes 0 (so a scale is never subnormal, and a block
//                         of subnormals encodes the same whether or not they are flushed)
//   else                  scale = amax / 127, code = clamp(rint(x / scale), -127, 127)
// Subnormals are kept (hipcc's default float mode; setup.py sets no flush flag):
// a subnormal element of a quantised block counts, e.g. 0.75 FLT_MIN under scale
// FLT_MIN has code 1.  A build that flushed them would give 0 there and no longer
// match the reference; tests/test_gpu_wire_q8.py holds such a block.
// Decode: y = float(code) * scale; raw blocks are then overwritten exactly.
//
// One row of 16 lanes holds one block (4 elements per lane), so the block
// reduction is four DPP steps inside the row: no LDS, no atomics, no traffic
// between workgroups.  Memory-bound: encode moves (4 or 2) n + 1.06 n bytes,
// decode 1.06 n + (4 or 2) n.
#include <cfloat>

#include "arena_io.h"

namespace p2 {

namespace {

constexpr int kQ8Block = 64;
constexpr uint32_t kQ8NaN = 0x7FC00000u;
constexpr uint32_t kQ8Inf = 0x7F800000u;

template <int CTRL>
P2_DEVICE uint32_t dpp_mov_u32(uint32_t v) {
  return uint32_t(__builtin_amdgcn_update_dpp(0, int(v), CTRL, 0xF, 0xF, false));
}
// max over the 16 lanes of a DPP row, every lane of the row gets it (the row
// part of wave_max; the rows stay separate: one row = one block)
P2_DEVICE uint32_t row_umax(uint32_t v) {
  v = max(v, dpp_mov_u32<0xB1>(v));   // quad_perm [1,0,3,2]
  v = max(v, dpp_mov_u32<0x4E>(v));   // quad_perm [2,3,0,1]
  v = max(v, dpp_mov_u32<0x141>(v));  // row_half_mirror
  v = max(v, dpp_mov_u32<0x140>(v));  // row_mirror
  return v;
}

// four elements from e (a multiple of 4), zeros past n
P2_DEVICE f32x4 load4_guarded(const void* src, int64_t e, int64_t n, bool bf16) {
  if (e + 4 <= n) return load4(src, e >> 2, bf16);
  f32x4 x = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int j = 0; j < 4; ++j)
    if (e + j < n) x[j] = load1(src, e + j, bf16);
  return x;
}

P2_DEVICE void store4_guarded(void* out, int64_t e, int64_t n, f32x4 y, bool bf16) {
  if (e + 4 <= n) {
    store4(out, e >> 2, y, bf16);
    return;
  }
#pragma unroll
  for (int j = 0; j < 4; ++j)
    if (e + j < n) store1(out, e + j, y[j], bf16);
}

P2_DEVICE int q8_code(float x, float scale) {
  const float q = rintf(__fdiv_rn(x, scale));  // correctly rounded quotient, ties to even
  return int(fminf(fmaxf(q, -127.f), 127.f));
}

// nq = 16 nb lane slots of four elements; the loop bound is uniform over a
// wave (nq is a multiple of 16 and the row bound is tested per row), so every
// lane of a row that reduces is active.
__global__ __launch_bounds__(256) void q8_encode_kernel(const void* __restrict__ src, int src_bf16, int64_t n,
                                                        int64_t nb, uint8_t* __restrict__ codes,
                                                        float* __restrict__ scales) {
  const int64_t stride = int64_t(gridDim.x) * blockDim.x;
  const int64_t nq_wave = (nb * 16 + kWave - 1) / kWave * kWave;  // whole waves
  for (int64_t q = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; q < nq_wave; q += stride) {
    const int64_t b = q >> 4;
    const bool live = b < nb;  // uniform over the row
    const int64_t e = q * 4;
    f32x4 x = {0.f, 0.f, 0.f, 0.f};
    if (live) x = load4_guarded(src, e, n, src_bf16);
    // unsigned order of |x| bit patterns = numeric order, and every Inf / NaN
    // pattern is >= 0x7F800000: absmax and the finite test from one reduction
    uint32_t m = __float_as_uint(x[0]) & 0x7FFFFFFFu;
    m = max(m, __float_as_uint(x[1]) & 0x7FFFFFFFu);
    m = max(m, __float_as_uint(x[2]) & 0x7FFFFFFFu);
    m = max(m, __float_as_uint(x[3]) & 0x7FFFFFFFu);
    m = row_umax(m);
    const float amax = __uint_as_float(m);
    float scale;
    uint32_t packed = 0;
    if (m >= kQ8Inf) {
      scale = __uint_as_float(kQ8NaN);
    } else if (amax < 127.f * FLT_MIN) {
      scale = 0.f;
    } else {
      scale = __fdiv_rn(amax, 127.f);
      packed = uint32_t(q8_code(x[0], scale) & 0xFF) | (uint32_t(q8_code(x[1], scale) & 0xFF) << 8) |
               (uint32_t(q8_code(x[2], scale) & 0xFF) << 16) | (uint32_t(q8_code(x[3], scale) & 0xFF) << 24);
    }
    if (live) {
      reinterpret_cast<uint32_t*>(codes)[q] = packed;  // a row writes 64 contiguous bytes
      if ((q & 15) == 0) scales[b] = scale;
    }
  }
}

__global__ __launch_bounds__(256) void q8_decode_kernel(const uint8_t* __restrict__ codes,
                                                        const float* __restrict__ scales, int64_t n, int64_t nb,
                                                        void* __restrict__ out, int out_bf16) {
  const int64_t stride = int64_t(gridDim.x) * blockDim.x;
  const int64_t nq = nb * 16;
  for (int64_t q = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; q < nq; q += stride) {
    const uint32_t w = __builtin_nontemporal_load(reinterpret_cast<const uint32_t*>(codes) + q);
    const float scale = scales[q >> 4];
    const f32x4 y = {float(int(int8_t(w & 0xFF))) * scale, float(int(int8_t((w >> 8) & 0xFF))) * scale,
                     float(int(int8_t((w >> 16) & 0xFF))) * scale, float(int(int8_t(w >> 24))) * scale};
    store4_guarded(out, q * 4, n, y, out_bf16);
  }
}

// Raw blocks: one row of 16 lanes moves one block (slot r of the raw section
// <-> block raw_ids[r] of the arena).  An id outside [0, nb) is skipped (the
// bindings refuse such a table before any launch).
__global__ __launch_bounds__(256) void q8_raw_gather(const void* __restrict__ src, int src_bf16, int64_t n, int64_t nb,
                                                     const int32_t* __restrict__ raw_ids, int R,
                                                     float* __restrict__ raw) {
  const int64_t stride = int64_t(gridDim.x) * blockDim.x;
  for (int64_t t = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; t < int64_t(R) * 16; t += stride) {
    const int64_t b = raw_ids[t >> 4];
    if (b < 0 || b >= nb) continue;
    reinterpret_cast<f32x4*>(raw)[t] = load4_guarded(src, b * kQ8Block + (t & 15) * 4, n, src_bf16);
  }
}

__global__ __launch_bounds__(256) void q8_raw_scatter(const float* __restrict__ raw, int64_t n, int64_t nb,
                                                      const int32_t* __restrict__ raw_ids, int R,
                                                      void* __restrict__ out, int out_bf16) {
  const int64_t stride = int64_t(gridDim.x) * blockDim.x;
  for (int64_t t = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; t < int64_t(R) * 16; t += stride) {
    const int64_t b = raw_ids[t >> 4];
    if (b < 0 || b >= nb) continue;
    store4_guarded(out, b * kQ8Block + (t & 15) * 4, n, reinterpret_cast<const f32x4*>(raw)[t], out_bf16);
  }
}

}  // namespace

void q8_encode(const void* src, int src_bf16, int64_t n, const int32_t* raw_ids, int R, uint8_t* packed,
               hipStream_t s) {
  if (n < 1 || R < 0) throw std::invalid_argument("q8_encode: n must be >= 1 and R >= 0");
  const int64_t nb = (n + kQ8Block - 1) / kQ8Block;
  float* raw = reinterpret_cast<float*>(packed + 64 * nb);
  float* scales = reinterpret_cast<float*>(packed + 64 * nb + 256 * int64_t(R));
  hipLaunchKernelGGL(q8_encode_kernel, dim3(stream_grid(nb * 16, 256)), dim3(256), 0, s, src, src_bf16, n, nb, packed,
                     scales);
  if (R > 0)
    hipLaunchKernelGGL(q8_raw_gather, dim3(stream_grid(int64_t(R) * 16, 256)), dim3(256), 0, s, src, src_bf16, n, nb,
                       raw_ids, R, raw);
}

void q8_decode(const uint8_t* packed, int64_t n, const int32_t* raw_ids, int R, void* out, int out_bf16,
               hipStream_t s) {
  if (n < 1 || R < 0) throw std::invalid_argument("q8_decode: n must be >= 1 and R >= 0");
  const int64_t nb = (n + kQ8Block - 1) / kQ8Block;
  const float* raw = reinterpret_cast<const float*>(packed + 64 * nb);
  const float* scales = reinterpret_cast<const float*>(packed + 64 * nb + 256 * int64_t(R));
  hipLaunchKernelGGL(q8_decode_kernel, dim3(stream_grid(nb * 16, 256)), dim3(256), 0, s, packed, scales, n, nb, out,
                     out_bf16);
  // same stream, after the main pass: the exact values overwrite the decoded ones
  if (R > 0)
    hipLaunchKernelGGL(q8_raw_scatter, dim3(stream_grid(int64_t(R) * 16, 256)), dim3(256), 0, s, raw, n, nb, raw_ids,
                       R, out, out_bf16);
}

}  // namespace p2
