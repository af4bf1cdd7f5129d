// Fused MLP step (gfx950): x -> Linear+ReLU -> Linear+ReLU -> Linear -> softmax
// cross-entropy, forward and backward, in three launches (two for evaluation).
// On PyTorch-ROCm the same step is two GEMM launches with bias epilogues, two
// ReLUs, a hipBLASLt GEMM for the 10-class layer, two log-softmaxes, an nll and
// autograd's mirror of all of it: launch overhead around 470 KB of weights.
//
// All products are v_mfma_f32_32x32x16_bf16 with fp32 accumulation.  Lane l
// (r = l & 31, h = l >> 5) supplies A[row r][k = 8h + j] and B[k = 8h + j][col r],
// j = 0..7 -- both operands as 16 B of a k-contiguous row; accumulator register i
// of lane l holds C[row (i & 3) + 8 (i >> 2) + 4h][col r].
//
//   1. mlp_l1    grid (ceil(B/32), H1/32), 4 waves.  h1 = relu(x W1^T + b1).  Both
//                operands are k-contiguous in global memory, so fragments are read
//                straight from L2 (fp32 x converted in registers); the K0 loop is
//                dealt round-robin to the four waves, whose partial tiles are added
//                through LDS in wave order.  Rows >= B read row B - 1 and are never
//                stored.
//                h1 and h2 are kept as bf16 hi + lo pairs for the forward products (two
//                MFMAs per k-step), so loss and logits carry the weights' and x's
//                rounding only; the gradients take the hi parts.
//   2. mlp_tail  grid ceil(B/32), 4 waves.  The h1 tile is staged in LDS; h2 (one
//                32-unit tile per wave) and the logits (one tile, classes >= C read
//                as zero weights) never leave the chip.  One lane per sample does
//                the row max, log-sum-exp, loss, hit and dlogits = (softmax -
//                onehot) / B.  Training continues in the same launch: dh2 =
//                (dlogits W3) . [h2 > 0] and dh1 = (dh2 W2) . [h1 > 0] sum over the
//                weights' row index, so W3 and W2 are read from transposed LDS
//                images (W2^T: 68 KB at 128 x 256).  h1, h2, dlogits, dh2 and dh1
//                are written batch-contiguous ([units][Bpad], rows B.. zero) for
//                launch 3.  Loss and accuracy: per-tile sums, added in tile order
//                by the last workgroup to arrive (relaxed ticket, sc1 partials).
//   3. mlp_wgrad one wave per 32 x 32 tile of dW1 = dh1^T x, dW2 = dh2^T h1, dW3 =
//                dlogits^T h2 (block index -> layer and tile from the counts in the
//                kernel arguments), K over the batch in steps of 16; x tiles are
//                transposed (and converted) through LDS.  Further waves sum the
//                rows of dlogits^T, dh2^T, dh1^T into the bias gradients, one thread
//                per unit in batch order.  Everything is scaled by the incoming
//                loss gradient (a device scalar).  One owner per element: no
//                atomics anywhere, results are bitwise reproducible.
//
// The reference's model: mnist_examples/models/mlp.py (784-256-128-10).
#include "common.h"
#include "mlp.h"

namespace p2mlp {
using namespace p2;

typedef __bf16 bf16x8_t __attribute__((ext_vector_type(8)));

constexpr int kLd1 = kMlpMaxH1 + 8;  // LDS row strides in bf16 elements (16-B multiples,
constexpr int kLd2 = kMlpMaxH2 + 8;  // the + 8 staggers rows over the banks)
constexpr int kLdc = kMlpMaxC + 8;
constexpr int kLgLd = kMlpMaxC + 1;

// dynamic LDS of mlp_tail (bytes)
constexpr int kOffH1 = 0;                                  // h1 tile   [32][kLd1] bf16
constexpr int kOffH1l = kOffH1 + 32 * kLd1 * 2;            // its low parts
constexpr int kOffH2 = kOffH1l + 32 * kLd1 * 2;            // h2 tile   [32][kLd2]
constexpr int kOffH2l = kOffH2 + 32 * kLd2 * 2;            // its low parts
constexpr int kOffDh2 = kOffH2l + 32 * kLd2 * 2;           // dh2 tile  [32][kLd2]
constexpr int kOffDl = kOffDh2 + 32 * kLd2 * 2;            // dlogits   [32][kLdc]
constexpr int kOffW3t = kOffDl + 32 * kLdc * 2;            // W3^T      [H2][kLdc]
constexpr int kOffLg = kOffW3t + kMlpMaxH2 * kLdc * 2;     // logits    [32][kLgLd] fp32
constexpr int kOffRow = kOffLg + 32 * kLgLd * 4;           // loss / hit per row [2][32] fp32
constexpr int kTailEvalLds = kOffRow + 64 * 4;
constexpr int kOffW2t = (kTailEvalLds + 15) / 16 * 16;     // W2^T      [H1][kLd2] (training)
constexpr int kTailTrainLds = kOffW2t + kMlpMaxH1 * kLd2 * 2;
static_assert(kTailTrainLds <= 160 * 1024, "mlp_tail exceeds gfx950's LDS");

P2_DEVICE f32x16 mfma(uint4 a, uint4 b, f32x16 c) {
  return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8_t, a), __builtin_bit_cast(bf16x8_t, b), c,
                                                  0, 0, 0);
}
P2_DEVICE int acc_row(int i, int h) { return (i & 3) + 8 * (i >> 2) + 4 * h; }
P2_DEVICE f32x16 zero16() {
  f32x16 z;
#pragma unroll
  for (int i = 0; i < 16; ++i) z[i] = 0.f;
  return z;
}
P2_DEVICE uint4 ld16(const uint16_t* p) { return *reinterpret_cast<const uint4*>(p); }

// 8 consecutive inputs as bf16
P2_DEVICE uint4 ldx8(const float* p) {
  const float4 a = reinterpret_cast<const float4*>(p)[0], b = reinterpret_cast<const float4*>(p)[1];
  return make_uint4(pack_bf16x2(a.x, a.y), pack_bf16x2(a.z, a.w), pack_bf16x2(b.x, b.y), pack_bf16x2(b.z, b.w));
}
P2_DEVICE uint4 ldx8(const uint16_t* p) { return ld16(p); }

P2_DEVICE void st_sc1f(float* p, float v) {
  const auto rs = __builtin_amdgcn_make_buffer_rsrc(p, 0, 4, 0x00020000);
  __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v), rs, 0, 0, 16);
}
P2_DEVICE float ld_sc1f(const float* p) {
  const auto rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p), 0, 4, 0x00020000);
  return __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rs, 0, 0, 16));
}

// ---------------------------------------------------------------------------
// 1. h1 = relu(x W1^T + b1)
// ---------------------------------------------------------------------------
template <typename TX>
__global__ __launch_bounds__(256) void mlp_l1_kernel(const TX* __restrict__ x, const uint16_t* __restrict__ w1,
                                                     const float* __restrict__ b1, uint16_t* __restrict__ h1, int B,
                                                     int K0, int H1) {
  __shared__ float red[4][16][64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, h = lane >> 5;
  const int m0 = blockIdx.x * 32, n0 = blockIdx.y * 32;
  const TX* xp = x + int64_t(min(m0 + r, B - 1)) * K0 + 8 * h;
  const uint16_t* wp = w1 + int64_t(n0 + r) * K0 + 8 * h;
  const int nks = K0 / 16;
  f32x16 acc = zero16();
  // k-step ks belongs to wave ks & 3; four steps of a wave are loaded together
  for (int base = 0; base < nks; base += 16) {
    uint4 a[4], b[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int ks = base + 4 * u + wave;
      a[u] = b[u] = make_uint4(0, 0, 0, 0);
      if (ks < nks) {
        a[u] = ldx8(xp + 16 * ks);
        b[u] = ld16(wp + 16 * ks);
      }
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) acc = mfma(a[u], b[u], acc);
  }
#pragma unroll
  for (int i = 0; i < 16; ++i) red[wave][i][lane] = acc[i];
  __syncthreads();
  // thread -> sample m, units nq..nq+3; the four wave partials in wave order
  const int m = tid >> 3, nq = (tid & 7) * 4;
  if (m0 + m >= B) return;
  const int i = (m & 3) + 4 * (m >> 3), lb = 32 * ((m >> 2) & 1) + nq;
  float v[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const float s = ((red[0][i][lb + q] + red[1][i][lb + q]) + red[2][i][lb + q]) + red[3][i][lb + q];
    v[q] = fmaxf(s + b1[n0 + nq + q], 0.f);
  }
  // h1 as two bf16 planes, hi + lo (16 mantissa bits): the forward products after it take both
  const uint2 hi = make_uint2(pack_bf16x2(v[0], v[1]), pack_bf16x2(v[2], v[3]));
  const float l0 = v[0] - __uint_as_float(hi.x << 16), l1 = v[1] - __uint_as_float(hi.x & 0xffff0000u);
  const float l2 = v[2] - __uint_as_float(hi.y << 16), l3 = v[3] - __uint_as_float(hi.y & 0xffff0000u);
  const int64_t o = int64_t(m0 + m) * H1 + n0 + nq;
  *reinterpret_cast<uint2*>(h1 + o) = hi;
  *reinterpret_cast<uint2*>(h1 + int64_t(B) * H1 + o) = make_uint2(pack_bf16x2(l0, l1), pack_bf16x2(l2, l3));
}

// ---------------------------------------------------------------------------
// 2. everything after h1
// ---------------------------------------------------------------------------
// the accumulator's 16 rows of column `col` -> out[col][m0 + row] (bf16, 4 samples per store)
P2_DEVICE void store_cols(uint16_t* out, int Bpad, int col, int m0, int h, const float (&v)[16]) {
#pragma unroll
  for (int q = 0; q < 4; ++q)
    *reinterpret_cast<uint2*>(out + int64_t(col) * Bpad + m0 + 8 * q + 4 * h) =
        make_uint2(pack_bf16x2(v[4 * q], v[4 * q + 1]), pack_bf16x2(v[4 * q + 2], v[4 * q + 3]));
}

__global__ __launch_bounds__(256) void mlp_tail_kernel(const uint16_t* __restrict__ h1g, const uint16_t* __restrict__ w2,
                                                       const float* __restrict__ b2, const uint16_t* __restrict__ w3,
                                                       const float* __restrict__ b3, const int64_t* __restrict__ y,
                                                       float* __restrict__ logits, float* __restrict__ parts,
                                                       float* __restrict__ loss_out, float* __restrict__ acc_out,
                                                       int* __restrict__ ctr, uint16_t* __restrict__ acts, int train,
                                                       MlpDims d) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  uint16_t* h1s = reinterpret_cast<uint16_t*>(smem + kOffH1);
  uint16_t* h1l = reinterpret_cast<uint16_t*>(smem + kOffH1l);
  uint16_t* h2s = reinterpret_cast<uint16_t*>(smem + kOffH2);
  uint16_t* h2l = reinterpret_cast<uint16_t*>(smem + kOffH2l);
  uint16_t* dh2s = reinterpret_cast<uint16_t*>(smem + kOffDh2);
  uint16_t* dls = reinterpret_cast<uint16_t*>(smem + kOffDl);
  uint16_t* w3t = reinterpret_cast<uint16_t*>(smem + kOffW3t);
  float* lg = reinterpret_cast<float*>(smem + kOffLg);
  float* rowv = reinterpret_cast<float*>(smem + kOffRow);
  uint16_t* w2t = reinterpret_cast<uint16_t*>(smem + kOffW2t);  // only touched when train
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, h = lane >> 5;
  const int B = d.B, Bpad = d.Bpad, H1 = d.H1, H2 = d.H2, C = d.C;
  const int m0 = blockIdx.x * 32;
  uint16_t* h1t = acts;
  uint16_t* h2t = h1t + int64_t(H1) * Bpad;
  uint16_t* dlt = h2t + int64_t(H2) * Bpad;
  uint16_t* dh2t = dlt + int64_t(kMlpMaxC) * Bpad;
  uint16_t* dh1t = dh2t + int64_t(H2) * Bpad;

  if (train) {
    // W2^T image: a task moves rows j, j + 1 of 8 columns as 8 packed words.  Lanes: 4
    // neighbouring column chunks (64 B of a row) x 16 row pairs.
    const int icg = H1 / 32, ntask = 64 * icg * (H2 / 32);
    for (int t = tid; t < ntask; t += 256) {
      const int rest = t >> 6;
      const int i0 = 8 * ((rest % icg) * 4 + (t & 3)), j = 2 * ((rest / icg) * 16 + ((t >> 2) & 15));
      const uint4 u0 = ld16(w2 + int64_t(j) * H1 + i0), u1 = ld16(w2 + int64_t(j + 1) * H1 + i0);
      const uint32_t a[4] = {u0.x, u0.y, u0.z, u0.w}, b[4] = {u1.x, u1.y, u1.z, u1.w};
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        *reinterpret_cast<uint32_t*>(w2t + (i0 + 2 * e) * kLd2 + j) = (a[e] & 0xffffu) | (b[e] << 16);
        *reinterpret_cast<uint32_t*>(w2t + (i0 + 2 * e + 1) * kLd2 + j) = (a[e] >> 16) | (b[e] & 0xffff0000u);
      }
    }
    // W3^T image, classes C..31 zero
    for (int t = tid; t < H2 * kMlpMaxC; t += 256) {
      const int j = t % H2, c = t / H2;
      w3t[j * kLdc + c] = c < C ? w3[int64_t(c) * H2 + j] : uint16_t(0);
    }
  }
  // h1 tile, rows >= B zero
  for (int t = tid; t < 32 * (H1 / 8); t += 256) {
    const int row = t / (H1 / 8), c8 = 8 * (t % (H1 / 8));
    uint4 v = make_uint4(0, 0, 0, 0), vl = v;
    if (m0 + row < B) {
      v = ld16(h1g + int64_t(m0 + row) * H1 + c8);
      vl = ld16(h1g + int64_t(B + m0 + row) * H1 + c8);
    }
    *reinterpret_cast<uint4*>(h1s + row * kLd1 + c8) = v;
    *reinterpret_cast<uint4*>(h1l + row * kLd1 + c8) = vl;
  }
  __syncthreads();

  // h2 = relu(h1 W2^T + b2): wave w owns units 32w..32w+31
  if (32 * wave < H2) {
    const int n0 = 32 * wave;
    const uint16_t* wp = w2 + int64_t(n0 + r) * H1 + 8 * h;
    f32x16 acc = zero16();
#pragma unroll 4
    for (int ks = 0; ks < H1 / 16; ++ks) {
      const uint4 b = ld16(wp + 16 * ks);
      acc = mfma(*reinterpret_cast<const uint4*>(h1l + r * kLd1 + 16 * ks + 8 * h), b, acc);
      acc = mfma(*reinterpret_cast<const uint4*>(h1s + r * kLd1 + 16 * ks + 8 * h), b, acc);
    }
    const float bias = b2[n0 + r];
    float v[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int row = acc_row(i, h);
      const float z = fmaxf(acc[i] + bias, 0.f);
      const uint16_t q = f32_to_bf16(z);
      h2s[row * kLd2 + n0 + r] = q;
      h2l[row * kLd2 + n0 + r] = f32_to_bf16(z - bf16_to_f32(q));
      v[i] = m0 + row < B ? bf16_to_f32(q) : 0.f;
    }
    if (train) store_cols(h2t, Bpad, n0 + r, m0, h, v);
  }
  __syncthreads();

  // logits = h2 W3^T + b3: one tile, wave 0
  if (wave == 0) {
    const uint16_t* wp = w3 + int64_t(min(r, C - 1)) * H2 + 8 * h;
    f32x16 acc = zero16();
#pragma unroll 4
    for (int ks = 0; ks < H2 / 16; ++ks) {
      const uint4 b = r < C ? ld16(wp + 16 * ks) : make_uint4(0, 0, 0, 0);
      acc = mfma(*reinterpret_cast<const uint4*>(h2l + r * kLd2 + 16 * ks + 8 * h), b, acc);
      acc = mfma(*reinterpret_cast<const uint4*>(h2s + r * kLd2 + 16 * ks + 8 * h), b, acc);
    }
    const float bias = r < C ? b3[r] : 0.f;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int row = acc_row(i, h);
      const float z = acc[i] + bias;
      lg[row * kLgLd + r] = z;
      if (r < C && m0 + row < B) logits[int64_t(m0 + row) * C + r] = z;
    }
  }
  __syncthreads();

  // one lane per sample: loss, hit, dlogits
  if (tid < 32) {
    const int s = tid, row = m0 + s;
    float lv = 0.f, hit = 0.f;
    uint16_t* dl = dls + s * kLdc;
    if (row < B) {
      const float* l = lg + s * kLgLd;
      float mx = l[0];
      int arg = 0;
      for (int c = 1; c < C; ++c)
        if (l[c] > mx) {
          mx = l[c];
          arg = c;
        }
      float se = 0.f;
      for (int c = 0; c < C; ++c) se += __expf(l[c] - mx);
      // a label outside [0, C) gives a NaN loss and NaN gradients, never a clamped one
      const int64_t yl = y[row];
      const bool ok = yl >= 0 && yl < C;
      const int yy = ok ? int(yl) : 0;
      lv = ok ? (logf(se) + mx) - l[yy] : __builtin_nanf("");
      hit = arg == yy ? 1.f : 0.f;
      const float rs = 1.f / se, ib = 1.f / float(B);
      for (int c = 0; c < C; ++c)
        dl[c] = f32_to_bf16(ok ? (__expf(l[c] - mx) * rs - (c == yy ? 1.f : 0.f)) * ib : __builtin_nanf(""));
      for (int c = C; c < kMlpMaxC; ++c) dl[c] = 0;
    } else {
      for (int c = 0; c < kMlpMaxC; ++c) dl[c] = 0;
    }
    rowv[s] = lv;
    rowv[32 + s] = hit;
    if (train)
      for (int c = 0; c < kMlpMaxC; ++c) dlt[int64_t(c) * Bpad + row] = dl[c];
  }
  __syncthreads();

  if (train) {
    // dh2 = (dlogits W3) . [h2 > 0]
    if (32 * wave < H2) {
      const int n0 = 32 * wave;
      f32x16 acc = zero16();
#pragma unroll
      for (int ks = 0; ks < kMlpMaxC / 16; ++ks)
        acc = mfma(*reinterpret_cast<const uint4*>(dls + r * kLdc + 16 * ks + 8 * h),
                   *reinterpret_cast<const uint4*>(w3t + (n0 + r) * kLdc + 16 * ks + 8 * h), acc);
      float v[16];
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int row = acc_row(i, h);
        const uint16_t q = (h2s[row * kLd2 + n0 + r] & 0x7fff) != 0 ? f32_to_bf16(acc[i]) : uint16_t(0);
        dh2s[row * kLd2 + n0 + r] = q;
        v[i] = bf16_to_f32(q);
      }
      store_cols(dh2t, Bpad, n0 + r, m0, h, v);
    }
    __syncthreads();
    // dh1 = (dh2 W2) . [h1 > 0]: H1 / 32 tiles dealt to the four waves
    for (int n0 = 32 * wave; n0 < H1; n0 += 128) {
      f32x16 acc = zero16();
#pragma unroll 4
      for (int ks = 0; ks < H2 / 16; ++ks)
        acc = mfma(*reinterpret_cast<const uint4*>(dh2s + r * kLd2 + 16 * ks + 8 * h),
                   *reinterpret_cast<const uint4*>(w2t + (n0 + r) * kLd2 + 16 * ks + 8 * h), acc);
      float v[16];
#pragma unroll
      for (int i = 0; i < 16; ++i) v[i] = (h1s[acc_row(i, h) * kLd1 + n0 + r] & 0x7fff) != 0 ? acc[i] : 0.f;
      store_cols(dh1t, Bpad, n0 + r, m0, h, v);
    }
    // h1^T for dW2
    for (int u = tid; u < H1; u += 256) {
      uint32_t p[16];
#pragma unroll
      for (int s = 0; s < 16; ++s)
        p[s] = uint32_t(h1s[(2 * s) * kLd1 + u]) | (uint32_t(h1s[(2 * s + 1) * kLd1 + u]) << 16);
      uint4* o = reinterpret_cast<uint4*>(h1t + int64_t(u) * Bpad + m0);
#pragma unroll
      for (int s = 0; s < 4; ++s) o[s] = make_uint4(p[4 * s], p[4 * s + 1], p[4 * s + 2], p[4 * s + 3]);
    }
  }

  // tile sums, then the last tile to arrive adds all of them in tile order
  if (tid != 0) return;
  const int T = gridDim.x;
  float sl = 0.f, sa = 0.f;
  for (int s = 0; s < 32; ++s) {
    sl += rowv[s];
    sa += rowv[32 + s];
  }
  st_sc1f(parts + blockIdx.x, sl);
  st_sc1f(parts + T + blockIdx.x, sa);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  const int old = __hip_atomic_fetch_add(ctr, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (old != T - 1) return;
  __hip_atomic_store(ctr, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  sl = sa = 0.f;
  for (int t = 0; t < T; ++t) {
    sl += ld_sc1f(parts + t);
    sa += ld_sc1f(parts + T + t);
  }
  loss_out[0] = sl / float(B);
  acc_out[0] = sa / float(B);
}

// ---------------------------------------------------------------------------
// 3. the six parameter gradients
// ---------------------------------------------------------------------------
struct WgradJobs {  // blocks [0, n1): dW1 tiles, then dW2, dW3, db1, db2, db3 (one block)
  int n1, n2, n3, nb1, nb2;
};

// out[u0 + row][v0 + r] = g * acc, rows < ulim, columns < vlim
P2_DEVICE void store_tile(uint16_t* out, int ld, int u0, int v0, int ulim, int vlim, int r, int h, float g,
                          const f32x16& acc) {
  if (v0 + r >= vlim) return;
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const int u = u0 + acc_row(i, h);
    if (u < ulim) out[int64_t(u) * ld + v0 + r] = f32_to_bf16(acc[i] * g);
  }
}

// out[u][v] = sum_b gt[u][b] at[v][b]: both batch-contiguous
P2_DEVICE f32x16 tile_tt(const uint16_t* gt, const uint16_t* at, int Bpad, int u0, int v0, int r, int h) {
  const uint16_t* ap = gt + int64_t(u0 + r) * Bpad + 8 * h;
  const uint16_t* bp = at + int64_t(v0 + r) * Bpad + 8 * h;
  f32x16 acc = zero16();
#pragma unroll 2
  for (int ks = 0; ks < Bpad / 16; ++ks) acc = mfma(ld16(ap + 16 * ks), ld16(bp + 16 * ks), acc);
  return acc;
}

template <typename TX>
__global__ __launch_bounds__(64) void mlp_wgrad_kernel(const float* __restrict__ gloss, const TX* __restrict__ x,
                                                       const uint16_t* __restrict__ acts, uint16_t* __restrict__ dw1,
                                                       float* __restrict__ db1, uint16_t* __restrict__ dw2,
                                                       float* __restrict__ db2, uint16_t* __restrict__ dw3,
                                                       float* __restrict__ db3, MlpDims d, WgradJobs jobs) {
  __shared__ __attribute__((aligned(16))) uint16_t xt[32 * kLdc];  // x tile transposed: [column][sample]
  const int lane = threadIdx.x, r = lane & 31, h = lane >> 5;
  const int B = d.B, Bpad = d.Bpad, K0 = d.K0, H1 = d.H1, H2 = d.H2, C = d.C;
  const uint16_t* h1t = acts;
  const uint16_t* h2t = h1t + int64_t(H1) * Bpad;
  const uint16_t* dlt = h2t + int64_t(H2) * Bpad;
  const uint16_t* dh2t = dlt + int64_t(kMlpMaxC) * Bpad;
  const uint16_t* dh1t = dh2t + int64_t(H2) * Bpad;
  const float g = gloss[0];
  int blk = blockIdx.x;
  if (blk < jobs.n1) {  // dW1 = dh1^T x
    const int tv = (K0 + 31) / 32, u0 = (blk / tv) * 32, v0 = (blk % tv) * 32;
    const uint16_t* ap = dh1t + int64_t(u0 + r) * Bpad + 8 * h;
    const int col0 = v0 + 16 * h;  // this lane stages 16 columns of sample b0 + r
    f32x16 acc = zero16();
    for (int b0 = 0; b0 < Bpad; b0 += 32) {
      uint4 lo = make_uint4(0, 0, 0, 0), hi = lo;
      if (b0 + r < B && col0 < K0) {
        const TX* xp = x + int64_t(b0 + r) * K0 + col0;
        lo = ldx8(xp);
        hi = ldx8(xp + 8);
      }
      const uint32_t w[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
      __syncthreads();  // the previous chunk's fragments have been read
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        xt[(16 * h + 2 * e) * kLdc + r] = uint16_t(w[e] & 0xffffu);
        xt[(16 * h + 2 * e + 1) * kLdc + r] = uint16_t(w[e] >> 16);
      }
      __syncthreads();
#pragma unroll
      for (int ks = 0; ks < 2; ++ks)
        acc = mfma(ld16(ap + b0 + 16 * ks), *reinterpret_cast<const uint4*>(xt + r * kLdc + 16 * ks + 8 * h), acc);
    }
    store_tile(dw1, K0, u0, v0, H1, K0, r, h, g, acc);
    return;
  }
  blk -= jobs.n1;
  if (blk < jobs.n2) {  // dW2 = dh2^T h1
    const int tv = H1 / 32, u0 = (blk / tv) * 32, v0 = (blk % tv) * 32;
    store_tile(dw2, H1, u0, v0, H2, H1, r, h, g, tile_tt(dh2t, h1t, Bpad, u0, v0, r, h));
    return;
  }
  blk -= jobs.n2;
  if (blk < jobs.n3) {  // dW3 = dlogits^T h2, rows < C
    store_tile(dw3, H2, 0, blk * 32, C, H2, r, h, g, tile_tt(dlt, h2t, Bpad, 0, blk * 32, r, h));
    return;
  }
  blk -= jobs.n3;
  // bias gradients: one thread per unit, the batch in order
  const uint16_t* src;
  float* dst;
  int n, u;
  if (blk < jobs.nb1) {
    src = dh1t, dst = db1, n = H1, u = blk * 64 + lane;
  } else if (blk < jobs.nb1 + jobs.nb2) {
    src = dh2t, dst = db2, n = H2, u = (blk - jobs.nb1) * 64 + lane;
  } else {
    src = dlt, dst = db3, n = C, u = lane;
  }
  if (u >= n) return;
  float s = 0.f;
  for (int b0 = 0; b0 < Bpad; b0 += 8) {
    float v[8];
    Vec8<uint16_t>::load(src + int64_t(u) * Bpad + b0, v);
#pragma unroll
    for (int j = 0; j < 8; ++j) s += v[j];
  }
  dst[u] = s * g;
}

}  // namespace p2mlp

namespace p2 {

void mlp_l1(const void* x, int x_bf16, const uint16_t* w1, const float* b1, uint16_t* h1, MlpDims d, hipStream_t s) {
  using namespace p2mlp;
  const dim3 grid(d.Bpad / 32, d.H1 / 32);
  if (x_bf16)
    hipLaunchKernelGGL(mlp_l1_kernel<uint16_t>, grid, dim3(256), 0, s, static_cast<const uint16_t*>(x), w1, b1, h1, d.B,
                       d.K0, d.H1);
  else
    hipLaunchKernelGGL(mlp_l1_kernel<float>, grid, dim3(256), 0, s, static_cast<const float*>(x), w1, b1, h1, d.B, d.K0,
                       d.H1);
}

void mlp_tail(const uint16_t* h1, const uint16_t* w2, const float* b2, const uint16_t* w3, const float* b3,
              const int64_t* y, float* logits, float* parts, float* loss, float* acc, int* ctr, uint16_t* acts,
              int train, MlpDims d, hipStream_t s) {
  using namespace p2mlp;
  // the training launch needs more than the default 64 KB of LDS: asked for once per device
  constexpr int kMaxDevices = 64;
  static bool asked[kMaxDevices] = {};
  int dev = 0;
  P2_CHECK(hipGetDevice(&dev));
  if (dev < 0 || dev >= kMaxDevices) throw std::runtime_error("mlp: device index out of range");
  if (!asked[dev]) {
    P2_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(mlp_tail_kernel),
                                 hipFuncAttributeMaxDynamicSharedMemorySize, kTailTrainLds));
    asked[dev] = true;
  }
  hipLaunchKernelGGL(mlp_tail_kernel, dim3(d.Bpad / 32), dim3(256), train ? kTailTrainLds : kTailEvalLds, s, h1, w2, b2,
                     w3, b3, y, logits, parts, loss, acc, ctr, acts, train, d);
}

void mlp_wgrad(const float* gloss, const void* x, int x_bf16, const uint16_t* acts, uint16_t* dw1, float* db1,
               uint16_t* dw2, float* db2, uint16_t* dw3, float* db3, MlpDims d, hipStream_t s) {
  using namespace p2mlp;
  WgradJobs j;
  j.n1 = (d.H1 / 32) * ((d.K0 + 31) / 32);
  j.n2 = (d.H2 / 32) * (d.H1 / 32);
  j.n3 = d.H2 / 32;
  j.nb1 = (d.H1 + 63) / 64;
  j.nb2 = (d.H2 + 63) / 64;
  const dim3 grid(j.n1 + j.n2 + j.n3 + j.nb1 + j.nb2 + 1);
  if (x_bf16)
    hipLaunchKernelGGL(mlp_wgrad_kernel<uint16_t>, grid, dim3(64), 0, s, gloss, static_cast<const uint16_t*>(x), acts,
                       dw1, db1, dw2, db2, dw3, db3, d, j);
  else
    hipLaunchKernelGGL(mlp_wgrad_kernel<float>, grid, dim3(64), 0, s, gloss, static_cast<const float*>(x), acts, dw1,
                       db1, dw2, db2, dw3, db3, d, j);
}

}  // namespace p2
