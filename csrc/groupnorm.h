// Fused GroupNorm (+ residual add) (+ ReLU) for channels-last activations
// (groupnorm.hip).  An NHWC activation is N row-major matrices [HW, C]; bf16
// selects uint16 bf16 activations, else fp32.  Parameters and statistics are
// fp32.  G groups of cpg = C / G contiguous channels, cpg a multiple of 8.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace p2gn {

// LDS a workgroup may use on gfx950 (static + dynamic): the 160 KB of a CU.
// Above 64 KB the launchers ask for it per kernel (hipFuncSetAttribute); a
// kernel whose request is refused keeps the 64 KB default.  Found on the
// MI355X: the full 163840 bytes are granted and a 163776-byte dynamic slab
// launches and runs (profiles/groupnorm.md).
constexpr int kLdsLimit = 160 * 1024;
constexpr int kLdsDefault = 64 * 1024;

// Work split.  A unit is one sample times a slab of cs channels (whole groups,
// the last slab of a sample may be narrower); a team of wpu waves owns a unit,
// 4 / wpu units share a 256-thread workgroup.
struct GnPlan {
  int cs;      // channels per slab
  int ns;      // slabs per sample
  int wpu;     // waves per unit: 1 (four packed units per workgroup) or 4; 0: shape not supported
  int units;   // N * ns
  int blocks;  // workgroups
  int64_t unit_bytes;  // one unit's activations: HW * cs * sizeof(element)
};
GnPlan gn_plan(bool bf16, int N, int HW, int C, int G);

// What the launchers do with the plan on the current device.  fwd_resident:
// the slab stays in LDS between the statistics and the apply.  bwd_keep: 2 the
// masked gradient and x stay in LDS, 1 the masked gradient only (x is read
// again), 0 neither (the streamed variant).  lds: the per-workgroup LDS the
// kernels were granted.
struct GnResidency {
  int fwd_resident, bwd_keep, lds;
};
GnResidency gn_residency(bool bf16, int N, int HW, int C, int G);

// y = act((x - mean) * rstd * w + b [+ res]) per (sample, group); biased
// two-pass variance; mean / rstd: [N, G] (saved for the backward).
void gn_fwd(bool bf16, const void* x, const void* res, const float* w, const float* b, float eps, void* y, float* mean,
            float* rstd, int N, int HW, int C, int G, bool relu, hipStream_t s);

// Backward of the above given dy and the saved output y (ReLU mask; read only with relu):
//   dz = relu ? dy * (y > 0) : dy
//   db = sum_{n,hw} dz, dw = sum_{n,hw} dz * xhat
//   dx = rstd * (w dz - mean_group(w dz) - xhat mean_group(w dz xhat)); dres = dz (if dres != null)
// part: [2, N, C] fp32 scratch (per-sample db / dw rows, added in sample order).
void gn_bwd(bool bf16, const void* dy, const void* y, const void* x, const float* w, const float* mean,
            const float* rstd, void* dx, void* dres, float* dw, float* db, float* part, int N, int HW, int C, int G,
            bool relu, hipStream_t s);

}  // namespace p2gn
