// Element access shared by the kernels that stream k flat parameter arenas
// (aggregate.hip: weighted sum; robust_agg.hip: order statistics, pairwise
// distances): the pointer table passed by value, vector and scalar loads of an
// fp32-or-bf16 arena widened to fp32, and the matching stores.
#pragma once
#include "common.h"
#include "kernels.h"

namespace p2 {

struct ArenaSrcs {
  const void* src[kMaxInputs];
};

// Four consecutive elements of an arena as fp32: a 16-byte fp32 load or an
// 8-byte bf16 load widened in registers (a bf16 arena costs half the bytes).
P2_DEVICE f32x4 load4(const void* base, int64_t i, bool bf16) {
  if (bf16) {
    const uint2 r = __builtin_bit_cast(uint2, __builtin_nontemporal_load(reinterpret_cast<const u32x2*>(base) + i));
    return f32x4{__uint_as_float(r.x << 16), __uint_as_float(r.x & 0xffff0000u), __uint_as_float(r.y << 16),
                 __uint_as_float(r.y & 0xffff0000u)};
  }
  return __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(base) + i);
}

// One element (the n % 4 tail).
P2_DEVICE float load1(const void* base, int64_t i, bool bf16) {
  return bf16 ? bf16_to_f32(reinterpret_cast<const uint16_t*>(base)[i]) : reinterpret_cast<const float*>(base)[i];
}

P2_DEVICE void store4(void* out, int64_t i, f32x4 v, bool bf16) {
  if (bf16)
    reinterpret_cast<uint2*>(out)[i] = uint2{pack_bf16x2(v[0], v[1]), pack_bf16x2(v[2], v[3])};
  else
    reinterpret_cast<f32x4*>(out)[i] = v;
}

P2_DEVICE void store1(void* out, int64_t i, float v, bool bf16) {
  if (bf16)
    reinterpret_cast<uint16_t*>(out)[i] = f32_to_bf16(v);
  else
    reinterpret_cast<float*>(out)[i] = v;
}

}  // namespace p2
