// Host launch API of the hand-written MFMA GEMM (csrc/gemm.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace p2 {

// C[M][N] = sum_k A(m, k) * B(n, k) over bf16 operands, fp32 accumulation.
//   A(m, k) = a[m * lda + k] when a_kmajor, else a[k * lda + m]
//   B(n, k) = b[n * ldb + k] when b_kmajor, else b[k * ldb + n]
// (nn.Linear forward: A = x [M][K], B = W [N][K], both k-major; dgrad:
//  B = W read n-major; wgrad: both operands m/n-major.)
// Epilogue, in order: + bias[n] (fp32 or bf16), GELU (writes the
// pre-activation to `z` if given), + residual[m][n] (bf16); C is bf16 or
// fp32.  With splits > 1 every K-slice writes its raw fp32 partial to
// c + slice * M * N instead (no epilogue; reduce afterwards) -- or, when
// `counters` is given, to the workspace `ws` ([splits][M][N] fp32), and the
// last slice to finish a tile reduces the tile in the same launch and runs
// the epilogue into c.  `counters` holds one int per output tile, zero
// before the launch; the kernel leaves it zero again.
// BatchNorm training statistics emitted by a GEMM / convolution epilogue (bf16 C
// only): every output tile writes per-column (mean, M2) of its bf16-rounded
// values as a partial; the last tile of a group of 16 tile-rows combines its
// group (Chan's parallel formula, fixed order), the last group finalizes the
// column: batch mean / rstd, the apply coefficients [mean | w * rstd | b] of
// csrc/batchnorm.hip, running statistics (momentum, unbiased variance) and
// num_batches_tracked.  `part` holds (tiles_m + groups) * 2 * N floats; `cnt`
// tiles_n * (groups + 1) ints, zero before the launch and left zero.
struct BnEpi {
  float* part;
  int* cnt;
  const float* w;
  const float* b;
  float* run_mean;  // optional (no running statistics when null)
  float* run_var;
  int64_t* nbt;     // optional
  float* mean;      // [N] out
  float* rstd;      // [N] out
  float* coef;      // [3N] out
  float eps, momentum;
  // Backward mode (bx != null): C is dz, the gradient w.r.t. the output of an
  // act(bn(x)) whose input x = bx and output (for the ReLU mask) = by (null: no
  // ReLU) are bf16 [M][N]; the launch reduces s1 = sum dz', s2 = sum dz' (x -
  // bmean) with dz' = dz * (by > 0), and the finalize writes dw = rstd * s2,
  // db = s1 and coef = [A | B | D] of csrc/batchnorm.hip's apply_bwd
  // (dx = A dz' + B (x - mean) + D) instead of the forward outputs.
  const uint16_t* bx;
  const uint16_t* by;
  const float* bmean;
  const float* brstd;
  float* dw;
  float* db;
  // measurement knob (P2_BN_EPI_MODE, read once by the conv launcher): 0 = full
  // epilogue; 1 = per-tile statistics only (no cross-tile reduction: outputs are
  // not finalized); 2 = statistics + partial stores + first-level ticket only
  int mode;
};

struct GemmParams {
  const uint16_t* a;
  const uint16_t* b;
  void* c;
  int64_t lda, ldb, ldc;
  int M, N, K;
  int a_kmajor, b_kmajor;
  int c_bf16;
  const void* bias;
  int bias_bf16;
  int gelu;
  uint16_t* z;  // GELU pre-activation output (bf16, ldc), optional
  const uint16_t* residual;  // bf16 [M][ldc], optional
  int splits;
  float* ws;      // split-K workspace for the in-launch reduction
  int* counters;  // per-tile arrival counters (see above), or null
  BnEpi bn;       // BatchNorm statistics epilogue when bn.part != null
  int variant;    // kernel selection and tuning bits: the kVar* constants below
};

// GemmParams::variant bits.  The values are part of the tuner's choice names
// ("native:2048:6"), of P2PFL_GEMM_VARIANT and of the committed profiles.
constexpr int kVarSetprio = 1;            // s_setprio around the core kernel's MFMA clusters
constexpr int kVarAPanel = 2;             // consecutive tiles share an A panel (default: a B panel)
constexpr int kVarNoXcdRemap = 4;         // workgroup ids as dispatched, no per-XCD tile runs
constexpr int kVarSingleBuf = 8;          // 128 x 128 tile on one LDS buffer, 4 workgroups per CU
constexpr int kVarProbeNoStore = 16;      // core kernel timing probe (wrong results): no C stores
constexpr int kVarProbeNoKLoop = 32;      // core kernel timing probe (wrong results): no K loop
constexpr int kVarTile256 = 64;           // 256 x 256 tile, 8 waves, on the core pipeline
constexpr int kVarProbeNoDma = 128;       // core kernel timing probe (wrong results): no DMA after the prologue
constexpr int kVarLegacyOrder = 256;      // plain panel tile order instead of grouped (kVarAPanel picks the panel)
constexpr int kVarPrefetchShift = 9;      // bits 9-10: where the double buffer's prefetch is issued (0 before the
constexpr int kVarPrefetchMask = 3 << 9;  //   K-tile's fragment reads, 1 after the first ones, 2 a chunk per k-substep)
constexpr int kVarPP = 2048;              // the ping-pong pipeline of gemm_pp.hip (256 x 256 tile)
constexpr int kVarRing = 4096;            // 128 x 128 tile on a 4-stage LDS ring, one workgroup per CU
constexpr int kConvT64 = 1 << 14;         // conv.hip only: 64 x 64 tiles (gemm_core.h Tile64) and their split-K slabs
constexpr int kVarPPM16 = 1 << 16;        // with kVarPP: v_mfma_f32_16x16x32_bf16 instead of 32x32x16
constexpr int kVarPPStreamK = 1 << 17;    // with kVarPP: stream-K schedule, GemmParams::splits = grid size
constexpr int kVarPPN128 = 1 << 21;       // with kVarPP: the 256 x 128 tile (gemm_pp128_kernel)
// with kVarPP, bits 12-15 and 18-20 select nothing: the binding refuses them, so a stale
// or forced value fails instead of reaching what bits 12 and 14 mean to the core kernels
constexpr int kVarPPRefused = (15 << 12) | (7 << 18);

void gemm_bf16(const GemmParams& p, hipStream_t s);
// out[M][ldc] = sum of the `splits` fragment-native split-K slabs (gemm_core.h SlabGeom)
// that a launch without counters wrote to `ws`; `variant` = that launch's (tile shape, order)
void tile_slab_reduce(const float* ws, int splits, int M, int N, int64_t ldc, void* out, int out_bf16, int variant,
                      hipStream_t s);
// the ping-pong pipeline (gemm_pp.hip); gemm_bf16 routes kVarPP here
bool gemm_pp_supported(const GemmParams& p);
void gemm_bf16_pp(const GemmParams& p, hipStream_t s);

}  // namespace p2
