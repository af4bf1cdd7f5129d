// Fused optimizer steps (Adam / AdamW / SGD-momentum) over flat arenas.
//
// torch.optim (and the reference's Lightning loop, cnn.py:89-91) update each
// parameter tensor with its own kernel(s).  With parameters, gradients and
// optimizer state laid out as flat arenas the full update is one streaming
// pass: float4 loads of p, g, m, v; fp32 math; float4 stores; optional bf16
// shadow copy of p for bf16 MFMA consumers (saves a separate cast kernel).
//
// Each piece exists once: an update rule per optimizer (AdamRule, SgdRule), the
// element helpers that move a rule's state between memory and registers, one
// whole-arena traversal and one multi-tensor traversal.  The __global__ kernels
// are wrappers that pick a rule and a traversal.
#include <cstdlib>
#include "common.h"
#include "kernels.h"

namespace p2 {

// ---- update rules ----------------------------------------------------------
// A rule holds its hyperparameters and the bases of its kStates fp32 state
// arenas (indexed like p), says whether a state array is there at all, and
// updates one element held in registers: p and its state s[kStates], given g.
struct AdamRule {
  static constexpr int kStates = 2;  // m, v
  AdamParams h;
  float* s[kStates];
  P2_DEVICE bool has(int) const { return true; }
  P2_DEVICE void apply(float& p, float g, float (&ms)[kStates]) const {
    float &m = ms[0], &v = ms[1];
    if (h.weight_decay != 0.f) {
      if (h.decoupled)
        p *= (1.f - h.lr * h.weight_decay);
      else
        g = fmaf(h.weight_decay, p, g);
    }
    m = fmaf(h.beta1, m, (1.f - h.beta1) * g);
    v = fmaf(h.beta2, v, (1.f - h.beta2) * g * g);
    p = p - h.step_size * (m / (sqrtf(v) * h.inv_sqrt_bc2 + h.eps));
  }
};

struct SgdRule {
  static constexpr int kStates = 1;  // momentum buffer; null without momentum
  SgdParams h;
  float* s[kStates];
  P2_DEVICE bool has(int) const { return s[0] != nullptr; }
  P2_DEVICE void apply(float& p, float g, float (&bs)[kStates]) const {
    float& b = bs[0];
    if (h.weight_decay != 0.f) g = fmaf(h.weight_decay, p, g);
    if (has(0)) {
      b = h.first_step ? g : fmaf(h.momentum, b, (1.f - h.dampening) * g);
      g = h.nesterov ? fmaf(h.momentum, b, g) : b;
    }
    p = fmaf(-h.lr, g, p);
  }
};

// ---- element helpers ---------------------------------------------------------
// Everything stays in registers: the arrays are indexed by unrolled constants
// only (a pointer to a local would put the state on the stack).
P2_DEVICE void load_grad4(const void* g, bool bf, int64_t i, float (&o)[4]) {
  if (bf) {
    const uint2 u = *reinterpret_cast<const uint2*>(static_cast<const uint16_t*>(g) + i);
    o[0] = __uint_as_float(u.x << 16);
    o[1] = __uint_as_float(u.x & 0xffff0000u);
    o[2] = __uint_as_float(u.y << 16);
    o[3] = __uint_as_float(u.y & 0xffff0000u);
  } else {
    const float4 f = *reinterpret_cast<const float4*>(static_cast<const float*>(g) + i);
    o[0] = f.x; o[1] = f.y; o[2] = f.z; o[3] = f.w;
  }
}
P2_DEVICE float load_grad1(const void* g, bool bf, int64_t i) {
  return bf ? bf16_to_f32(static_cast<const uint16_t*>(g)[i]) : static_cast<const float*>(g)[i];
}
P2_DEVICE void store_bf16x4(uint16_t* q, const float (&v)[4]) {
  uint2 o;
  o.x = pack_bf16x2(v[0], v[1]);
  o.y = pack_bf16x2(v[2], v[3]);
  *reinterpret_cast<uint2*>(q) = o;
}

// Element i of the arenas: p and the rule's state into registers / back.
template <class Rule>
P2_DEVICE void load1(const Rule& r, const float* p, int64_t i, float& pv, float (&sv)[Rule::kStates]) {
  pv = p[i];
#pragma unroll
  for (int k = 0; k < Rule::kStates; ++k) sv[k] = r.has(k) ? r.s[k][i] : 0.f;
}
template <class Rule>
P2_DEVICE void store1(const Rule& r, float* p, int64_t i, float pv, const float (&sv)[Rule::kStates]) {
  p[i] = pv;
#pragma unroll
  for (int k = 0; k < Rule::kStates; ++k)
    if (r.has(k)) r.s[k][i] = sv[k];
}
// One step of element i; returns the new p.
template <class Rule>
P2_DEVICE float step1(const Rule& r, float* p, int64_t i, float g) {
  float pv, sv[Rule::kStates];
  load1(r, p, i, pv, sv);
  r.apply(pv, g, sv);
  store1(r, p, i, pv, sv);
  return pv;
}
// Elements i .. i + 3 (16-byte aligned) as float4 accesses.
template <class Rule>
P2_DEVICE void load4(const Rule& r, const float* p, int64_t i, float (&pv)[4], float (&sv)[4][Rule::kStates]) {
  const float4 pp = *reinterpret_cast<const float4*>(p + i);
  pv[0] = pp.x; pv[1] = pp.y; pv[2] = pp.z; pv[3] = pp.w;
#pragma unroll
  for (int k = 0; k < Rule::kStates; ++k) {
    const float4 t = r.has(k) ? *reinterpret_cast<const float4*>(r.s[k] + i) : make_float4(0.f, 0.f, 0.f, 0.f);
    sv[0][k] = t.x; sv[1][k] = t.y; sv[2][k] = t.z; sv[3][k] = t.w;
  }
}
// The step on the 4 elements load4 left in registers, and their new p and state back to memory.
template <class Rule>
P2_DEVICE void step4(const Rule& r, float* p, int64_t i, const float (&g)[4], float (&pv)[4],
                     float (&sv)[4][Rule::kStates]) {
#pragma unroll
  for (int e = 0; e < 4; ++e) r.apply(pv[e], g[e], sv[e]);
  *reinterpret_cast<float4*>(p + i) = make_float4(pv[0], pv[1], pv[2], pv[3]);
#pragma unroll
  for (int k = 0; k < Rule::kStates; ++k)
    if (r.has(k)) *reinterpret_cast<float4*>(r.s[k] + i) = make_float4(sv[0][k], sv[1][k], sv[2][k], sv[3][k]);
}

// ---- whole-arena traversal ------------------------------------------------------
template <class Rule>
P2_DEVICE void arena_body(const Rule& r, float* p, const float* g, uint16_t* pbf, int64_t n4) {
  const int64_t stride = int64_t(gridDim.x) * blockDim.x;
  for (int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; i < n4; i += stride) {
    float gg[4], pv[4], sv[4][Rule::kStates];
    load_grad4(g, false, 4 * i, gg);
    load4(r, p, 4 * i, pv, sv);
    step4(r, p, 4 * i, gg, pv, sv);
    if (pbf) store_bf16x4(pbf + 4 * i, pv);
  }
}

__global__ __launch_bounds__(256) void adam_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                   float* __restrict__ m, float* __restrict__ v,
                                                   uint16_t* __restrict__ pbf, int64_t n4, AdamParams h) {
  arena_body(AdamRule{h, {m, v}}, p, g, pbf, n4);
}

__global__ __launch_bounds__(256) void sgd_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                  float* __restrict__ buf, uint16_t* __restrict__ pbf,
                                                  int64_t n4, SgdParams h) {
  arena_body(SgdRule{h, {buf}}, p, g, pbf, n4);
}

void adam_step(float* p, const float* g, float* m, float* v, uint16_t* pbf, int64_t n, const AdamParams& h,
               hipStream_t s) {
  const int64_t n4 = n / 4;  // arenas are padded to 64 elements
  hipLaunchKernelGGL(adam_kernel, dim3(stream_grid(n4, 256)), dim3(256), 0, s, p, g, m, v, pbf, n4, h);
}

void sgd_step(float* p, const float* g, float* buf, uint16_t* pbf, int64_t n, const SgdParams& h, hipStream_t s) {
  const int64_t n4 = n / 4;
  hipLaunchKernelGGL(sgd_kernel, dim3(stream_grid(n4, 256)), dim3(256), 0, s, p, g, buf, pbf, n4, h);
}

// ---------------------------------------------------------------------------
// Multi-tensor variants for mixed-precision learners.  The module's matrix
// weights are bf16 views of a shadow arena (the GEMMs read them directly, no
// per-step cast kernels) and autograd leaves each gradient in its own tensor
// (bf16 for bf16 weights, fp32 for the rest): no per-parameter grad
// accumulate / zero-fill launches.  One launch updates every tensor: a static
// chunk table maps each block to (tensor, start); the per-step table holds
// the gradient pointers (null = no grad this step: the tensor is skipped, as
// torch.optim does).  Master weights and state stay fp32 flat arenas, so
// FedAvg / gossip / checkpoints are unchanged.
// ---------------------------------------------------------------------------

// Memory position, in a channels-last (O, kh, kw, I) tensor, of logical
// OIHW element ``i``.  32-bit math: one tensor stays below 2^31 elements.
P2_DEVICE uint32_t cl_index(uint32_t i, uint32_t C, uint32_t HW) {
  const uint32_t per_o = C * HW, o = i / per_o, r = i - o * per_o, c = r / HW, s = r - c * HW;
  return o * per_o + s * C + c;
}
// n / d by multiply-high (n < 2^31): the magic numbers are computed once per block
// (uniform), so the per-element channels-last index costs two v_mul_hi instead of
// two ~25-instruction integer divisions
struct FastDivU {
  uint32_t d, mul, shift;
};
P2_DEVICE FastDivU make_fastdiv_u(uint32_t d) {
  const uint32_t l = d <= 1 ? 0u : 32u - __clz(d - 1);
  const uint64_t mul = ((uint64_t(1) << 32) * ((uint64_t(1) << l) - d)) / d + 1;
  return FastDivU{d, uint32_t(mul), l};
}
P2_DEVICE uint32_t fdivu(uint32_t n, const FastDivU& f) { return (__umulhi(n, f.mul) + n) >> f.shift; }
P2_DEVICE uint32_t cl_index_fast(uint32_t i, uint32_t C, const FastDivU& per_o, const FastDivU& hw) {
  const uint32_t o = fdivu(i, per_o), r = i - o * per_o.d, c = fdivu(r, hw), s = r - c * hw.d;
  return o * per_o.d + s * C + c;
}
P2_DEVICE uint32_t cl_c(int64_t flags) { return uint32_t((flags >> 8) & 0xFFFFFF); }
P2_DEVICE uint32_t cl_hw(int64_t flags) { return uint32_t((flags >> 32) & 0xFFFFFF); }

// ---- channels-last chunks staged through LDS ---------------------------------
// A chunk of whole output-channel slabs covers the SAME element range in the
// OIHW state and in the (O, kh, kw, I) gradient / shadow, only permuted inside
// each slab (cl_index_fast of a chunk-local element is its chunk-local
// channels-last position).  So every global access can be contiguous: the
// gradient is read as 8 / 16-byte vectors into LDS (one pad word after every
// I-run, so the OIHW-order reads that follow hit distinct banks), the
// fp32 state is streamed in OIHW order as 16-byte vectors, and the new bf16
// weights go back through LDS to 8-byte stores.  The per-element gather /
// scatter of the fallback path below (2-byte gradient loads and shadow stores
// at channels-last positions) ran sgd_mt at 50-65 % of HBM roofline on
// ResNet-18 (profiles/r4_resnet18_steady_state.md).
constexpr int kMTClPad = kMTMaxCL + kMTMaxCL / 4;  // gradient words incl. pads (I >= 4)
struct ClStage {
  float g[kMTClPad];
  uint16_t sh[kMTMaxCL];
};
// Staged only when the chunk is whole slabs: ops.optim's layout gives whole-slab chunks
// only to tensors whose slab C x HW fits kMTMaxCL; a larger slab is cut into plain
// chunks that start mid-slab, which the slab-local permutation cannot map (gather path).
P2_DEVICE bool cl_staged(uint32_t C, uint32_t HW, int64_t len) {
  return HW > 1 && C % 4 == 0 && len <= kMTMaxCL && C * HW <= uint32_t(kMTMaxCL);
}
// LDS word of channels-last element j (one pad word per I-run of C elements)
P2_DEVICE uint32_t cl_pad(uint32_t j, const FastDivU& fc) { return j + fdivu(j, fc); }
P2_DEVICE void cl_load_grad(ClStage& st, const void* g, bool gbf, int64_t first, int len, const FastDivU& fc) {
  for (int j = threadIdx.x * 4; j < len; j += 1024) {
    float v[4];
    load_grad4(g, gbf, first + j, v);
    const uint32_t q = cl_pad(uint32_t(j), fc);  // the 4 share one I-run (I % 4 == 0)
#pragma unroll
    for (int e = 0; e < 4; ++e) st.g[q + e] = v[e];
  }
}
P2_DEVICE void cl_store_shadow(const ClStage& st, uint16_t* __restrict__ sb, int len) {
  for (int j = threadIdx.x * 4; j < len; j += 1024)
    *reinterpret_cast<uint2*>(sb + j) = *reinterpret_cast<const uint2*>(st.sh + j);
}

// ---- multi-tensor traversal: one block per chunk-table entry -------------------
template <bool FD, class Rule>
P2_DEVICE void mt_body(const Rule& r, float* p, uint16_t* pbf, const MTTensor* tens, const int2* chunks,
                       const uint64_t* gptr) {
  __shared__ ClStage st;
  const int2 ch = chunks[blockIdx.x];
  const void* g = reinterpret_cast<const void*>(gptr[ch.x]);
  if (g == nullptr) return;
  const MTTensor T = tens[ch.x];
  const bool gbf = T.flags & kMTGradBf16, shadow = (T.flags & kMTShadow) && pbf;
  const int64_t start = ch.y;
  const int64_t len = T.n - start < T.chunk ? T.n - start : T.chunk;
  const int64_t base = T.off + start;  // the chunk's first element in p, the state arenas and a plain shadow
  uint16_t* PB = shadow ? pbf + base : nullptr;
  if ((T.flags & kMTPermCL) && cl_staged(cl_c(T.flags), cl_hw(T.flags), len)) {
    const uint32_t C = cl_c(T.flags), HW = cl_hw(T.flags);
    const FastDivU fpo = make_fastdiv_u(C * HW), fhw = make_fastdiv_u(HW), fc = make_fastdiv_u(C);
    cl_load_grad(st, g, gbf, start, int(len), fc);
    __syncthreads();
    for (int i = threadIdx.x * 4; i < len; i += 1024) {
      uint32_t j[4];
      float gg[4], pv[4], sv[4][Rule::kStates];
      load4(r, p, base + i, pv, sv);  // in flight under the index math
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        j[e] = cl_index_fast(uint32_t(i + e), C, fpo, fhw);
        gg[e] = st.g[cl_pad(j[e], fc)];
      }
      step4(r, p, base + i, gg, pv, sv);
      if (PB) {
#pragma unroll
        for (int e = 0; e < 4; ++e) st.sh[j[e]] = f32_to_bf16(pv[e]);
      }
    }
    if (PB) {
      __syncthreads();
      cl_store_shadow(st, PB, int(len));
    }
    return;
  }
  if (T.flags & kMTPermCL) {
    // fp32 state in logical (coalesced) order; the bf16 gradient and shadow
    // are gathered / scattered at their channels-last positions (the whole
    // slab of an output channel is L2-resident while its block runs)
    const uint32_t C = cl_c(T.flags), HW = cl_hw(T.flags);
    FastDivU fpo{}, fhw{};
    if (FD) fpo = make_fastdiv_u(C * HW), fhw = make_fastdiv_u(HW);
    uint16_t* SB = shadow ? pbf + T.off : nullptr;
    // 4 elements per thread in flight (state loads + gradient gathers issued
    // together): one dependent round trip per element made this loop latency-bound
    for (int64_t i0 = threadIdx.x; i0 < len; i0 += 4 * 256) {
      float pv[4], gv[4], sv[4][Rule::kStates];
      uint32_t j[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int64_t i = i0 + u * 256;
        if (i < len) {
          j[u] = FD ? cl_index_fast(uint32_t(start + i), C, fpo, fhw) : cl_index(uint32_t(start + i), C, HW);
          load1(r, p, base + i, pv[u], sv[u]);
          gv[u] = load_grad1(g, gbf, j[u]);
        }
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int64_t i = i0 + u * 256;
        if (i < len) {
          r.apply(pv[u], gv[u], sv[u]);
          store1(r, p, base + i, pv[u], sv[u]);
          if (SB) SB[j[u]] = f32_to_bf16(pv[u]);
        }
      }
    }
    return;
  }
  // contiguous tensors: 16-byte vectors where the chunk starts on one (always, for arenas laid
  // out by learning/optim.py: offsets are multiples of 64, chunks of kMTChunk), then a scalar tail
  const int64_t len4 = (reinterpret_cast<uintptr_t>(p + base) & 15) == 0 ? (len & ~int64_t(3)) : 0;
  for (int64_t i = int64_t(threadIdx.x) * 4; i < len4; i += 256 * 4) {
    float gg[4], pv[4], sv[4][Rule::kStates];
    load_grad4(g, gbf, start + i, gg);
    load4(r, p, base + i, pv, sv);
    step4(r, p, base + i, gg, pv, sv);
    if (PB) store_bf16x4(PB + i, pv);
  }
  for (int64_t i = len4 + threadIdx.x; i < len; i += 256) {
    const float np = step1(r, p, base + i, load_grad1(g, gbf, start + i));
    if (PB) PB[i] = f32_to_bf16(np);
  }
}

template <bool FD>
__global__ __launch_bounds__(256) void adam_mt_kernel(float* __restrict__ p, float* __restrict__ m,
                                                      float* __restrict__ v, uint16_t* __restrict__ pbf,
                                                      const MTTensor* __restrict__ tens, const int2* __restrict__ chunks,
                                                      const uint64_t* __restrict__ gptr, AdamParams h) {
  if (h.t_dev) {  // graph-replayable steps: the bias corrections of step *t_dev, from the fp32 betas
    const float t = float(*h.t_dev);
    h.step_size = h.lr / (1.f - powf(h.beta1, t));
    h.inv_sqrt_bc2 = rsqrtf(1.f - powf(h.beta2, t));
  }
  mt_body<FD>(AdamRule{h, {m, v}}, p, pbf, tens, chunks, gptr);
}

template <bool FD>
__global__ __launch_bounds__(256) void sgd_mt_kernel(float* __restrict__ p, float* __restrict__ buf,
                                                     uint16_t* __restrict__ pbf, const MTTensor* __restrict__ tens,
                                                     const int2* __restrict__ chunks, const uint64_t* __restrict__ gptr,
                                                     SgdParams h) {
  mt_body<FD>(SgdRule{h, {buf}}, p, pbf, tens, chunks, gptr);
}

// channels-last index by multiply-high (default) or by integer division (P2_MT_FASTDIV=0; A/B knob, read once)
static bool mt_fastdiv() {
  static const bool on = [] {
    const char* e = getenv("P2_MT_FASTDIV");
    return !e || atoi(e) != 0;
  }();
  return on;
}

void adam_mt_step(float* p, float* m, float* v, uint16_t* pbf, const MTTensor* tens, const int2* chunks,
                  int n_chunks, const uint64_t* gptr, const AdamParams& h, hipStream_t s) {
  if (n_chunks <= 0) return;
  if (mt_fastdiv())
    hipLaunchKernelGGL(adam_mt_kernel<true>, dim3(n_chunks), dim3(256), 0, s, p, m, v, pbf, tens, chunks, gptr, h);
  else
    hipLaunchKernelGGL(adam_mt_kernel<false>, dim3(n_chunks), dim3(256), 0, s, p, m, v, pbf, tens, chunks, gptr, h);
}

void sgd_mt_step(float* p, float* buf, uint16_t* pbf, const MTTensor* tens, const int2* chunks, int n_chunks,
                 const uint64_t* gptr, const SgdParams& h, hipStream_t s) {
  if (n_chunks <= 0) return;
  if (mt_fastdiv())
    hipLaunchKernelGGL(sgd_mt_kernel<true>, dim3(n_chunks), dim3(256), 0, s, p, buf, pbf, tens, chunks, gptr, h);
  else
    hipLaunchKernelGGL(sgd_mt_kernel<false>, dim3(n_chunks), dim3(256), 0, s, p, buf, pbf, tens, chunks, gptr, h);
}

}  // namespace p2
