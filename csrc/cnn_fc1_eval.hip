// FC1 of the MNIST-CNN evaluation passes on the tiled MFMA GEMM core (gemm_core.h).
//
//   slabs[s][m][n] = sum_{k in slice s} A[m][k] * W1bf[n][k]     (bf16 operands, fp32)
//
// with m < mrows (a multiple of 128 up to 512), n < 2048, k < 3136 and S = 1..4 K-slices:
// the slab layout head_kernel reduces.  gemm_skinny streams the 12.8 MB W1 shadow once
// per 128 rows through per-lane register loads; an evaluation pass of 300 or 500 samples
// is one launch here, W1 read once: 128 x 128 tiles on the double-buffered
// global_load_lds pipeline, 4 x 16 tiles x 4 slices = 256 workgroups at 512 rows, one per
// CU.  The 49 K-tiles of 64 split as 13 + 13 + 13 + 10 (gemm_body rounds a slice up to
// whole K-tiles and clips the last).  Workgroup ids are remapped per XCD (xcd_remap), and
// tiles run row-tile fastest, so an XCD's 32 workgroups share 8 column panels of one
// slice: every W1 byte is fetched by one XCD only.  Each slice writes its own slab with
// plain stores (epilogue 3) -- no tickets, no atomics, a fixed summation order.
#include "cnn.h"
#include "gemm_core.h"

namespace p2cnn {

using p2gemm::PlainK;
using p2gemm::Tile128;

__global__ __launch_bounds__(p2gemm::NT, 2) void fc1_eval_kernel(p2::GemmParams p, PlainK la, PlainK lb, int tiles_m,
                                                                 int tiles_n) {
  __shared__ __attribute__((aligned(16))) char smem[p2gemm::smem_bytes<Tile128, 2>()];
  p2gemm::gemm_body<Tile128, 2, PlainK, PlainK, 0, 3>(p, la, lb, tiles_m, tiles_n, smem);
}

void fc1_eval(const uint16_t* A, const uint16_t* W1bf, float* slabs, int mrows, int S, hipStream_t s) {
  p2::GemmParams p{};
  p.a = A;
  p.b = W1bf;
  p.c = slabs;
  p.lda = p.ldb = kFeat;
  p.ldc = kHid;
  p.M = mrows;
  p.N = kHid;
  p.K = kFeat;
  p.a_kmajor = p.b_kmajor = 1;
  p.splits = S;
  int tm, tn;
  const int grid = p2gemm::gemm_grid<Tile128>(p, tm, tn);
  hipLaunchKernelGGL(fc1_eval_kernel, dim3(grid), dim3(p2gemm::NT), 0, s, p, PlainK{A, kFeat, mrows, kFeat},
                     PlainK{W1bf, kFeat, kHid, kFeat}, tm, tn);
}

}  // namespace p2cnn
