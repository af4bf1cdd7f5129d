// Fused MLP training / evaluation step (csrc/mlp.hip): three launches.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace p2 {

constexpr int kMlpMaxH1 = 256, kMlpMaxH2 = 128, kMlpMaxC = 32;

// B samples (Bpad = B rounded up to 32), K0 inputs (% 16), H1 <= 256 and H2 <= 128
// hidden units (% 32), C <= 32 classes
struct MlpDims {
  int B, Bpad, K0, H1, H2, C;
};

// rows of the batch-contiguous workspace `acts` (bf16 [2 H1 + 2 H2 + 32][Bpad]):
// h1^T, h2^T, dlogits^T (32 rows, C used), dh2^T, dh1^T
inline int mlp_acts_rows(const MlpDims& d) { return 2 * d.H1 + 2 * d.H2 + kMlpMaxC; }

// h1 = relu(x W1^T + b1) as bf16 hi and lo planes, [2][B][H1]
void mlp_l1(const void* x, int x_bf16, const uint16_t* w1, const float* b1, uint16_t* h1, MlpDims d, hipStream_t s);
// layers 2 and 3, loss, accuracy and (train) the activation gradients
void mlp_tail(const uint16_t* h1, const uint16_t* w2, const float* b2, const uint16_t* w3, const float* b3,
              const int64_t* y, float* logits, float* parts, float* loss, float* acc, int* ctr, uint16_t* acts,
              int train, MlpDims d, hipStream_t s);
// all six parameter gradients, scaled by gloss[0]
void mlp_wgrad(const float* gloss, const void* x, int x_bf16, const uint16_t* acts, uint16_t* dw1, float* db1,
               uint16_t* dw2, float* db2, uint16_t* dw3, float* db3, MlpDims d, hipStream_t s);

}  // namespace p2
