// PyTorch bindings of the p2pfl_amd HIP kernels (module p2pfl_amd._C).
// Every entry validates shapes/dtypes/devices on the host BEFORE launching,
// so a mismatched call fails with a Python exception instead of a GPU fault.
#include <torch/extension.h>
#include <c10/hip/HIPStream.h>
#include <c10/core/DeviceGuard.h>

#include <cmath>
#include <cstdint>
#include <vector>

#include "kernels.h"
#include "cnn.h"

namespace {

hipStream_t stream() { return c10::hip::getCurrentHIPStream().stream(); }

void check_f32(const torch::Tensor& t, const char* name) {
  TORCH_CHECK(t.is_cuda(), name, " must be a GPU tensor");
  TORCH_CHECK(t.scalar_type() == torch::kFloat32, name, " must be float32");
  TORCH_CHECK(t.is_contiguous(), name, " must be contiguous");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0, name, " must be 16-byte aligned");
}

void check_arena(const torch::Tensor& t, const char* name) {
  TORCH_CHECK(t.is_cuda(), name, " must be a GPU tensor");
  TORCH_CHECK(t.scalar_type() == torch::kFloat32 || t.scalar_type() == torch::kBFloat16, name, " must be float32 or bfloat16");
  TORCH_CHECK(t.is_contiguous(), name, " must be contiguous");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0, name, " must be 16-byte aligned");
}

void weighted_sum(std::vector<torch::Tensor> srcs, std::vector<double> weights, torch::Tensor out,
                  c10::optional<torch::Tensor> acc_in, double scale) {
  TORCH_CHECK(srcs.size() == weights.size(), "weighted_sum: bad inputs");
  check_arena(out, "out");
  const bool out_bf16 = out.scalar_type() == torch::kBFloat16;
  TORCH_CHECK(!out_bf16 || srcs.size() <= size_t(p2::kMaxInputs), "weighted_sum: bf16 output supports at most ",
              p2::kMaxInputs, " inputs");
  const c10::DeviceGuard guard(out.device());
  const int64_t n = out.numel();
  const float* acc = nullptr;
  if (acc_in.has_value() && acc_in->defined()) {
    check_arena(*acc_in, "acc_in");
    TORCH_CHECK(acc_in->scalar_type() == torch::kFloat32 && acc_in->numel() == n && acc_in->device() == out.device(),
                "weighted_sum: acc_in must be an fp32 arena of the output's size and device");
    acc = acc_in->data_ptr<float>();
  }
  TORCH_CHECK(!srcs.empty() || acc != nullptr, "weighted_sum: no inputs");
  std::vector<const void*> ptrs;
  std::vector<int> bf;
  std::vector<float> w;
  for (size_t i = 0; i < srcs.size(); ++i) {
    check_arena(srcs[i], "src");
    TORCH_CHECK(srcs[i].numel() == n, "weighted_sum: size mismatch");
    TORCH_CHECK(srcs[i].device() == out.device(), "weighted_sum: device mismatch");
    ptrs.push_back(srcs[i].data_ptr());
    bf.push_back(srcs[i].scalar_type() == torch::kBFloat16 ? 1 : 0);
    w.push_back(float(weights[i]));
  }
  p2::weighted_sum(ptrs.data(), bf.data(), w.data(), int(ptrs.size()), acc, float(scale), out.data_ptr(),
                   out_bf16 ? 1 : 0, n, stream());
}

// pointer / dtype tables of 1..kMaxInputs arenas of one size on one device
struct ArenaList {
  std::vector<const void*> ptrs;
  std::vector<int> bf;
  int64_t n;
};
ArenaList check_arenas(const std::vector<torch::Tensor>& srcs, size_t min_k, const char* op) {
  TORCH_CHECK(srcs.size() >= min_k && srcs.size() <= size_t(p2::kMaxInputs), op, ": takes ", min_k, " to ",
              p2::kMaxInputs, " arenas, got ", srcs.size());
  ArenaList a;
  a.n = srcs[0].numel();
  for (const auto& t : srcs) {
    check_arena(t, "src");
    TORCH_CHECK(t.numel() == a.n, op, ": size mismatch");
    TORCH_CHECK(t.device() == srcs[0].device(), op, ": device mismatch");
    a.ptrs.push_back(t.data_ptr());
    a.bf.push_back(t.scalar_type() == torch::kBFloat16 ? 1 : 0);
  }
  return a;
}

void trimmed_mean(std::vector<torch::Tensor> srcs, int64_t trim, torch::Tensor out) {
  const ArenaList a = check_arenas(srcs, 1, "trimmed_mean");
  const int k = int(srcs.size());
  TORCH_CHECK(trim >= 0 && trim <= (k - 1) / 2, "trimmed_mean: trim must be in [0, ", (k - 1) / 2, "], got ", trim);
  check_arena(out, "out");
  TORCH_CHECK(out.numel() == a.n && out.device() == srcs[0].device(),
              "trimmed_mean: out must have the inputs' size and device");
  const c10::DeviceGuard guard(out.device());
  p2::trimmed_mean(a.ptrs.data(), a.bf.data(), k, int(trim), out.data_ptr(),
                   out.scalar_type() == torch::kBFloat16 ? 1 : 0, a.n, stream());
}

torch::Tensor pairwise_sqdist(std::vector<torch::Tensor> srcs) {
  const ArenaList a = check_arenas(srcs, 2, "pairwise_sqdist");
  const int k = int(srcs.size());
  const c10::DeviceGuard guard(srcs[0].device());
  const auto opts = torch::TensorOptions().dtype(torch::kFloat32).device(srcs[0].device());
  torch::Tensor partials = torch::empty({int64_t(k) * (k - 1) / 2, int64_t(p2::pairwise_sqdist_blocks(a.n))}, opts);
  torch::Tensor out = torch::empty({k, k}, opts);
  p2::pairwise_sqdist(a.ptrs.data(), a.bf.data(), k, partials.data_ptr<float>(), out.data_ptr<float>(), a.n, stream());
  return out;
}

// ---- block-quantised int8 wire (quant_wire.hip) ------------------------------
int64_t q8_packed_nbytes(int64_t n, int64_t n_raw) {
  TORCH_CHECK(n >= 1 && n_raw >= 0, "q8: n must be >= 1 and n_raw >= 0");
  const int64_t nb = (n + 63) / 64;
  return 64 * nb + 256 * n_raw + 4 * nb;
}

// The raw-block table: int32, on the arena's device, sorted, unique, below nb.
// The kernels index the arena with these values, so they are checked on the
// host before anything is launched.  Two forms:
//  * Q8RawTable: built from host integers, checked once where it is built, then
//    copied to the device and never handed out again except as a copy -- what
//    the kernels read is what was checked, and a call costs no read-back
//    (p2pfl_amd.learning.arena.q8_raw_table makes these);
//  * any int32 device tensor: read back and checked on every call, which waits
//    for the work queued on the current stream.
struct Q8RawTable {
  torch::Tensor ids;  // int32 [R] on the device
  int64_t last;       // largest index: good for every nb above it
};
Q8RawTable make_raw_table(const std::vector<int64_t>& blocks, int64_t device) {
  TORCH_CHECK(!blocks.empty(), "Q8RawTable: no blocks");
  torch::Tensor host = torch::empty({int64_t(blocks.size())}, torch::dtype(torch::kInt32));
  int32_t* h = host.data_ptr<int32_t>();
  int64_t prev = -1;
  for (size_t i = 0; i < blocks.size(); ++i) {
    TORCH_CHECK(blocks[i] >= 0 && blocks[i] <= INT32_MAX, "Q8RawTable: block index ", blocks[i], " is out of range");
    TORCH_CHECK(blocks[i] > prev, "Q8RawTable: blocks must be sorted and unique");
    prev = blocks[i];
    h[i] = int32_t(prev);
  }
  return Q8RawTable{host.to(torch::Device(torch::kCUDA, c10::DeviceIndex(device))), prev};
}

struct RawIds {
  const int32_t* ptr = nullptr;
  int R = 0;
};
RawIds check_raw_ids(const pybind11::object& raw_obj, int64_t nb, const torch::Device& dev, const char* op) {
  RawIds r;
  if (raw_obj.is_none()) return r;
  if (pybind11::isinstance<Q8RawTable>(raw_obj)) {
    const Q8RawTable& t = raw_obj.cast<const Q8RawTable&>();  // lives as long as the caller's argument
    TORCH_CHECK(t.ids.device() == dev, op, ": raw_blocks must be on the arena's device");
    TORCH_CHECK(t.last < nb, op, ": raw block index ", t.last, " is outside [0, ", nb, ")");
    r.ptr = t.ids.data_ptr<int32_t>();
    r.R = int(t.ids.numel());
    return r;
  }
  const torch::Tensor raw_t = raw_obj.cast<torch::Tensor>();
  const torch::Tensor* raw = &raw_t;
  if (!raw->defined() || raw->numel() == 0) return r;
  TORCH_CHECK(raw->scalar_type() == torch::kInt32 && raw->dim() == 1 && raw->is_contiguous(), op,
              ": raw_blocks must be a contiguous 1-D int32 tensor");
  TORCH_CHECK(raw->device() == dev, op, ": raw_blocks must be on the arena's device");
  TORCH_CHECK(raw->numel() <= nb, op, ": more raw blocks than blocks");
  // (this read waits for the work queued on the current stream: the price of
  // checking the indices a kernel is about to use, every time)
  const torch::Tensor host = raw->cpu();
  const int32_t* h = host.data_ptr<int32_t>();
  int64_t prev = -1;
  for (int64_t i = 0; i < host.numel(); ++i) {
    TORCH_CHECK(h[i] >= 0 && h[i] < nb, op, ": raw block index ", h[i], " is outside [0, ", nb, ")");
    TORCH_CHECK(h[i] > prev, op, ": raw_blocks must be sorted and unique");
    prev = h[i];
  }
  r.ptr = raw->data_ptr<int32_t>();
  r.R = int(raw->numel());
  return r;
}

void check_packed(const torch::Tensor& packed, int64_t n, int R, const torch::Device& dev, const char* op) {
  TORCH_CHECK(packed.is_cuda() && packed.device() == dev, op, ": packed must be a GPU tensor on the arena's device");
  TORCH_CHECK(packed.scalar_type() == torch::kUInt8 && packed.dim() == 1 && packed.is_contiguous(), op,
              ": packed must be a contiguous 1-D uint8 tensor");
  TORCH_CHECK(packed.numel() == q8_packed_nbytes(n, R), op, ": packed holds ", packed.numel(), " bytes, expected ",
              q8_packed_nbytes(n, R), " for ", n, " elements and ", R, " raw blocks");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(packed.data_ptr()) % 16 == 0, op, ": packed must be 16-byte aligned");
}

torch::Tensor q8_encode(torch::Tensor src, pybind11::object raw_blocks, c10::optional<torch::Tensor> out) {
  check_arena(src, "src");
  TORCH_CHECK(src.dim() == 1 && src.numel() >= 1, "q8_encode: src must be a 1-D arena of at least one element");
  const int64_t n = src.numel();
  const RawIds raw = check_raw_ids(raw_blocks, (n + 63) / 64, src.device(), "q8_encode");
  const c10::DeviceGuard guard(src.device());
  torch::Tensor packed = (out.has_value() && out->defined())
                             ? *out
                             : torch::empty({q8_packed_nbytes(n, raw.R)},
                                            torch::TensorOptions().dtype(torch::kUInt8).device(src.device()));
  check_packed(packed, n, raw.R, src.device(), "q8_encode");
  p2::q8_encode(src.data_ptr(), src.scalar_type() == torch::kBFloat16 ? 1 : 0, n, raw.ptr, raw.R,
                packed.data_ptr<uint8_t>(), stream());
  return packed;
}

void q8_decode(torch::Tensor packed, int64_t n, pybind11::object raw_blocks, torch::Tensor out) {
  check_arena(out, "out");
  TORCH_CHECK(n >= 1 && out.dim() == 1 && out.numel() == n, "q8_decode: out must be a 1-D arena of n elements");
  const RawIds raw = check_raw_ids(raw_blocks, (n + 63) / 64, out.device(), "q8_decode");
  check_packed(packed, n, raw.R, out.device(), "q8_decode");
  const c10::DeviceGuard guard(out.device());
  p2::q8_decode(packed.data_ptr<uint8_t>(), n, raw.ptr, raw.R, out.data_ptr(),
                out.scalar_type() == torch::kBFloat16 ? 1 : 0, stream());
}

// ---- differentially private updates (dp_update.hip) --------------------------
// w / w0 / out: fp32 arenas of one size (a multiple of 64) on one device; table:
// uint8 [n / 64] on that device (its values are only compared against, so they
// need no check).
int64_t check_dp(const torch::Tensor& w, const torch::Tensor& w0, const torch::Tensor& table, const char* op) {
  check_f32(w, "w");
  check_f32(w0, "w0");
  const int64_t n = w.numel();
  TORCH_CHECK(w.dim() == 1 && n >= 64 && n % 64 == 0, op, ": w must be a 1-D arena of a positive multiple of 64 elements");
  TORCH_CHECK(w0.dim() == 1 && w0.numel() == n && w0.device() == w.device(), op, ": w0 must have w's size and device");
  TORCH_CHECK(table.is_cuda() && table.device() == w.device() && table.scalar_type() == torch::kUInt8 &&
                  table.dim() == 1 && table.is_contiguous() && table.numel() == n / 64,
              op, ": table must be a contiguous uint8 [n / 64] tensor on the arena's device");
  return n;
}

bool overlaps(const torch::Tensor& a, const torch::Tensor& b) {
  const auto a0 = reinterpret_cast<uintptr_t>(a.data_ptr()), b0 = reinterpret_cast<uintptr_t>(b.data_ptr());
  return a0 < b0 + b.nbytes() && b0 < a0 + a.nbytes();
}

torch::Tensor dp_delta_sqnorm(torch::Tensor w, torch::Tensor w0, torch::Tensor table) {
  const int64_t n = check_dp(w, w0, table, "dp_delta_sqnorm");
  const c10::DeviceGuard guard(w.device());
  const auto opts = torch::TensorOptions().dtype(torch::kFloat32).device(w.device());
  torch::Tensor partials = torch::empty({int64_t(p2::dp_sqnorm_blocks(n))}, opts);
  torch::Tensor out = torch::empty({1}, opts);
  p2::dp_delta_sqnorm(w.data_ptr<float>(), w0.data_ptr<float>(), table.data_ptr<uint8_t>(), n,
                      partials.data_ptr<float>(), out.data_ptr<float>(), stream());
  return out;
}

torch::Tensor dp_apply(torch::Tensor w, torch::Tensor w0, torch::Tensor table, torch::Tensor sqnorm, double clip,
                       double noise_multiplier, uint64_t seed, int64_t round, c10::optional<torch::Tensor> out) {
  const int64_t n = check_dp(w, w0, table, "dp_apply");
  TORCH_CHECK(sqnorm.is_cuda() && sqnorm.device() == w.device() && sqnorm.scalar_type() == torch::kFloat32 &&
                  sqnorm.numel() == 1,
              "dp_apply: sqnorm must be a 1-element float32 tensor on the arena's device");
  const float c = float(clip), sigma = float(noise_multiplier * clip);  // the product rounded once
  TORCH_CHECK(std::isfinite(c) && c > 0.f, "dp_apply: clip must be finite and > 0");
  TORCH_CHECK(std::isfinite(sigma) && noise_multiplier >= 0.0, "dp_apply: noise_multiplier must be finite and >= 0");
  TORCH_CHECK(noise_multiplier == 0.0 || sigma > 0.f, "dp_apply: noise_multiplier * clip underflows float32");
  TORCH_CHECK(round >= 0 && round <= int64_t(UINT32_MAX), "dp_apply: round must be in [0, 2^32)");
  const c10::DeviceGuard guard(w.device());
  torch::Tensor o = (out.has_value() && out->defined()) ? *out : torch::empty_like(w);
  check_f32(o, "out");
  TORCH_CHECK(o.dim() == 1 && o.numel() == n && o.device() == w.device(), "dp_apply: out must have w's size and device");
  TORCH_CHECK(!overlaps(o, w) && !overlaps(o, w0), "dp_apply: out must not overlap w or w0");
  p2::dp_apply(w.data_ptr<float>(), w0.data_ptr<float>(), table.data_ptr<uint8_t>(), sqnorm.data_ptr<float>(), c,
               sigma, seed, uint32_t(round), o.data_ptr<float>(), n, stream());
  return o;
}

uint16_t* opt_bf16(const c10::optional<torch::Tensor>& t, int64_t n) {
  if (!t.has_value() || !t->defined()) return nullptr;
  TORCH_CHECK(t->is_cuda() && t->scalar_type() == torch::kBFloat16 && t->is_contiguous() && t->numel() >= n,
              "bf16 shadow must be a contiguous bf16 GPU tensor of the arena size");
  return reinterpret_cast<uint16_t*>(t->data_ptr());
}

// Bias corrections of step t from the float32 hyperparameters already in h: the kernels
// accumulate m and v with those (1.f - h.beta2 is not 1 - 0.999), and corrections from the
// unrounded doubles describe a slightly different optimizer (v_hat = g^2 (1 - 1.3e-5) at
// t = 1, ~20x the rounding error of the whole update).  The device-side t_dev path of
// adam_mt_kernel uses the same float32 values.
void adam_bias_corrections(p2::AdamParams& h, int64_t step) {
  const double lr = double(h.lr), b1 = double(h.beta1), b2 = double(h.beta2);
  h.step_size = float(lr / (1.0 - std::pow(b1, double(step))));
  h.inv_sqrt_bc2 = float(1.0 / std::sqrt(1.0 - std::pow(b2, double(step))));
}

p2::AdamParams adam_params(double lr, double b1, double b2, double eps, double wd, int64_t step, bool decoupled) {
  p2::AdamParams h{};
  h.lr = float(lr);
  h.beta1 = float(b1);
  h.beta2 = float(b2);
  h.eps = float(eps);
  h.weight_decay = float(wd);
  adam_bias_corrections(h, step);
  h.decoupled = decoupled ? 1 : 0;
  return h;
}

// SGD's optional momentum buffer: null when absent, else an fp32 arena of n elements
float* opt_buf(c10::optional<torch::Tensor>& buf, int64_t n) {
  if (!buf.has_value() || !buf->defined()) return nullptr;
  check_f32(*buf, "buf");
  TORCH_CHECK(buf->numel() == n, "sgd: buf size mismatch");
  return buf->data_ptr<float>();
}

void adam_step(torch::Tensor p, torch::Tensor g, torch::Tensor m, torch::Tensor v, c10::optional<torch::Tensor> pbf,
               double lr, double b1, double b2, double eps, double wd, int64_t step, bool decoupled) {
  for (auto* t : {&p, &g, &m, &v}) check_f32(*t, "adam operand");
  const int64_t n = p.numel();
  TORCH_CHECK(g.numel() == n && m.numel() == n && v.numel() == n, "adam: size mismatch");
  TORCH_CHECK(n % 4 == 0, "adam: arena length must be a multiple of 4");
  const c10::DeviceGuard guard(p.device());
  const p2::AdamParams h = adam_params(lr, b1, b2, eps, wd, step, decoupled);
  p2::adam_step(p.data_ptr<float>(), g.data_ptr<float>(), m.data_ptr<float>(), v.data_ptr<float>(), opt_bf16(pbf, n),
                n, h, stream());
}

void sgd_step(torch::Tensor p, torch::Tensor g, c10::optional<torch::Tensor> buf, c10::optional<torch::Tensor> pbf,
              double lr, double momentum, double dampening, double wd, bool nesterov, bool first_step) {
  check_f32(p, "p");
  check_f32(g, "g");
  const int64_t n = p.numel();
  TORCH_CHECK(g.numel() == n && n % 4 == 0, "sgd: size mismatch");
  float* b = opt_buf(buf, n);
  const c10::DeviceGuard guard(p.device());
  p2::SgdParams h{float(lr), float(momentum), float(dampening), float(wd), nesterov ? 1 : 0, first_step ? 1 : 0};
  p2::sgd_step(p.data_ptr<float>(), g.data_ptr<float>(), b, opt_bf16(pbf, n), n, h, stream());
}

// ---- multi-tensor optimizer steps (mixed-precision learners) ----------------
// tens: int64 [T, 4] (offset, numel, flags, chunk) on the GPU; chunks: int32 [C, 2]
// (tensor, first element) on the GPU; grads: one entry per tensor (None = skip).
torch::Tensor grad_table(const std::vector<c10::optional<torch::Tensor>>& grads, const std::vector<int64_t>& numels,
                         const std::vector<bool>& grad_bf16, const std::vector<bool>& grad_cl, const torch::Device& dev) {
  const size_t T = grads.size();
  TORCH_CHECK(numels.size() == T && grad_bf16.size() == T && grad_cl.size() == T,
              "multi-tensor step: table size mismatch");
  auto host = torch::empty({int64_t(T)}, torch::dtype(torch::kInt64)).pin_memory();
  auto* hp = host.data_ptr<int64_t>();
  for (size_t t = 0; t < T; ++t) {
    hp[t] = 0;
    if (!grads[t].has_value() || !grads[t]->defined()) continue;
    const auto& g = *grads[t];
    // channels-last tensors (flag bit 2): the gradient arrives in the
    // weight's (O, kh, kw, I) memory order
    const bool dense = grad_cl[t] ? (g.dim() == 4 && g.is_contiguous(at::MemoryFormat::ChannelsLast)) : g.is_contiguous();
    TORCH_CHECK(g.device() == dev && dense && g.numel() == numels[t], "grad ", t,
                " must be a dense GPU tensor of the parameter's size and layout");
    TORCH_CHECK(g.scalar_type() == (grad_bf16[t] ? torch::kBFloat16 : torch::kFloat32), "grad ", t,
                " has an unexpected dtype");
    TORCH_CHECK(reinterpret_cast<uintptr_t>(g.data_ptr()) % 16 == 0, "grad ", t, " must be 16-byte aligned");
    hp[t] = int64_t(reinterpret_cast<uintptr_t>(g.data_ptr()));
  }
  return host.to(dev, /*non_blocking=*/true);
}

void check_tables(const torch::Tensor& tens, const torch::Tensor& chunks, const torch::Device& dev) {
  TORCH_CHECK(tens.device() == dev && tens.scalar_type() == torch::kInt64 && tens.dim() == 2 && tens.size(1) == 4 &&
                  tens.is_contiguous(),
              "tensor table must be int64 [T, 4] on the arena's device");
  TORCH_CHECK(chunks.device() == dev && chunks.scalar_type() == torch::kInt32 && chunks.dim() == 2 &&
                  chunks.size(1) == 2 && chunks.is_contiguous(),
              "chunk table must be int32 [C, 2] on the arena's device");
}

// gtab (optional): a persistent device table of gradient addresses (int64 [T])
// used instead of `grads` -- for steps captured in a HIP graph, whose gradient
// buffers have fixed addresses filled in after capture.
torch::Tensor grad_ptrs(const c10::optional<torch::Tensor>& gtab, const std::vector<c10::optional<torch::Tensor>>& grads,
                        const std::vector<int64_t>& numels, const std::vector<bool>& grad_bf16,
                        const std::vector<bool>& grad_cl, const torch::Tensor& tens, const torch::Device& dev) {
  if (gtab.has_value() && gtab->defined()) {
    TORCH_CHECK(gtab->device() == dev && gtab->scalar_type() == torch::kInt64 && gtab->is_contiguous() &&
                    gtab->numel() == tens.size(0),
                "gtab must be a contiguous int64 [T] tensor on the arena's device");
    return *gtab;
  }
  TORCH_CHECK(tens.size(0) == int64_t(grads.size()), "multi-tensor step: one gradient per tensor");
  return grad_table(grads, numels, grad_bf16, grad_cl, dev);
}

void adam_mt_step(torch::Tensor p, torch::Tensor m, torch::Tensor v, c10::optional<torch::Tensor> pbf,
                  torch::Tensor tens, torch::Tensor chunks, std::vector<c10::optional<torch::Tensor>> grads,
                  std::vector<int64_t> numels, std::vector<bool> grad_bf16, std::vector<bool> grad_cl, double lr,
                  double b1, double b2, double eps,
                  double wd, int64_t step, bool decoupled, c10::optional<torch::Tensor> gtab,
                  c10::optional<torch::Tensor> t_dev) {
  for (auto* t : {&p, &m, &v}) check_f32(*t, "adam operand");
  const int64_t n = p.numel();
  TORCH_CHECK(m.numel() == n && v.numel() == n, "adam: size mismatch");
  check_tables(tens, chunks, p.device());
  const c10::DeviceGuard guard(p.device());
  auto gp = grad_ptrs(gtab, grads, numels, grad_bf16, grad_cl, tens, p.device());
  p2::AdamParams h = adam_params(lr, b1, b2, eps, wd, step, decoupled);
  if (t_dev.has_value() && t_dev->defined()) {
    TORCH_CHECK(t_dev->device() == p.device() && t_dev->scalar_type() == torch::kInt32 && t_dev->numel() == 1,
                "t_dev must be an int32 [1] tensor on the arena's device");
    h.t_dev = t_dev->data_ptr<int32_t>();
  }
  p2::adam_mt_step(p.data_ptr<float>(), m.data_ptr<float>(), v.data_ptr<float>(), opt_bf16(pbf, n),
                   reinterpret_cast<const p2::MTTensor*>(tens.data_ptr<int64_t>()),
                   reinterpret_cast<const int2*>(chunks.data_ptr<int32_t>()), int(chunks.size(0)),
                   reinterpret_cast<const uint64_t*>(gp.data_ptr<int64_t>()), h, stream());
}

void sgd_mt_step(torch::Tensor p, c10::optional<torch::Tensor> buf, c10::optional<torch::Tensor> pbf,
                 torch::Tensor tens, torch::Tensor chunks, std::vector<c10::optional<torch::Tensor>> grads,
                 std::vector<int64_t> numels, std::vector<bool> grad_bf16, std::vector<bool> grad_cl, double lr,
                 double momentum,
                 double dampening, double wd, bool nesterov, bool first_step, c10::optional<torch::Tensor> gtab) {
  check_f32(p, "p");
  const int64_t n = p.numel();
  float* b = opt_buf(buf, n);
  check_tables(tens, chunks, p.device());
  const c10::DeviceGuard guard(p.device());
  auto gp = grad_ptrs(gtab, grads, numels, grad_bf16, grad_cl, tens, p.device());
  p2::SgdParams h{float(lr), float(momentum), float(dampening), float(wd), nesterov ? 1 : 0, first_step ? 1 : 0};
  p2::sgd_mt_step(p.data_ptr<float>(), b, opt_bf16(pbf, n), reinterpret_cast<const p2::MTTensor*>(tens.data_ptr<int64_t>()),
                  reinterpret_cast<const int2*>(chunks.data_ptr<int32_t>()), int(chunks.size(0)),
                  reinterpret_cast<const uint64_t*>(gp.data_ptr<int64_t>()), h, stream());
}

// A stream owned by its caller.  torch.cuda.Stream() hands out streams from a
// fixed pool of 32 per device, round robin: two learners (virtual peers) can
// then share one HIP stream, and an event one records on it while the other
// captures a graph on it becomes part of that capture (hipErrorCapturedEvent).
// priority: 0 the default queue priority, > 0 the device's lowest, < 0 its highest
int64_t new_stream(int64_t device, int64_t priority) {
  const c10::DeviceGuard guard(c10::Device(c10::DeviceType::CUDA, c10::DeviceIndex(device)));
  hipStream_t s = nullptr;
  int least = 0, greatest = 0;
  hipError_t e = hipDeviceGetStreamPriorityRange(&least, &greatest);
  TORCH_CHECK(e == hipSuccess, "new_stream: ", hipGetErrorString(e));
  const int prio = priority > 0 ? least : (priority < 0 ? greatest : 0);
  e = prio == 0 ? hipStreamCreateWithFlags(&s, hipStreamNonBlocking) : hipStreamCreateWithPriority(&s, hipStreamNonBlocking, prio);
  TORCH_CHECK(e == hipSuccess, "new_stream: ", hipGetErrorString(e));
  return reinterpret_cast<int64_t>(s);
}
void destroy_stream(int64_t s) { (void)hipStreamDestroy(reinterpret_cast<hipStream_t>(s)); }

}  // namespace

void register_cnn(pybind11::module& m);
void register_fused(pybind11::module& m);
void register_bn(pybind11::module& m);
void register_rccl(pybind11::module& m);
void register_gemm(pybind11::module& m);
void register_conv(pybind11::module& m);
void register_head(pybind11::module& m);

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.doc() = "p2pfl_amd native HIP/CDNA4 kernels (gfx950)";
  m.def("weighted_sum", &weighted_sum,
        "out = scale * (acc_in + sum_i w_i * src_i) (flat arenas, fp32/bf16 in, fp32/bf16 out, fp32 running sum)",
        pybind11::arg("srcs"), pybind11::arg("weights"), pybind11::arg("out"), pybind11::arg("acc_in") = pybind11::none(),
        pybind11::arg("scale") = 1.0);
  m.def("trimmed_mean", &trimmed_mean,
        "out = coordinate-wise mean of up to 16 arenas after dropping the trim lowest and highest values "
        "(trim = (k-1)/2: median)",
        pybind11::arg("srcs"), pybind11::arg("trim"), pybind11::arg("out"));
  m.def("pairwise_sqdist", &pairwise_sqdist,
        "k x k fp32 matrix of squared L2 distances between 2..16 arenas, one pass, deterministic",
        pybind11::arg("srcs"));
  m.def("q8_packed_nbytes", &q8_packed_nbytes, "bytes of the q8 packed buffer of n elements with n_raw raw blocks",
        pybind11::arg("n"), pybind11::arg("n_raw") = 0);
  pybind11::class_<Q8RawTable>(m, "Q8RawTable", "a q8 raw-block table checked where it is built (sorted, unique)")
      .def(pybind11::init(&make_raw_table), pybind11::arg("blocks"), pybind11::arg("device") = 0)
      .def("__len__", [](const Q8RawTable& t) { return t.ids.numel(); })
      .def("tensor", [](const Q8RawTable& t) { return t.ids.clone(); }, "a copy of the device table");
  m.def("q8_encode", &q8_encode,
        "block-quantise a flat fp32/bf16 arena: int8 codes + one fp32 scale per 64 elements, raw blocks kept in fp32",
        pybind11::arg("src"), pybind11::arg("raw_blocks") = pybind11::none(), pybind11::arg("out") = pybind11::none());
  m.def("q8_decode", &q8_decode, "decode a q8 packed buffer of n elements into a flat fp32/bf16 arena",
        pybind11::arg("packed"), pybind11::arg("n"), pybind11::arg("raw_blocks"), pybind11::arg("out"));
  m.def("dp_delta_sqnorm", &dp_delta_sqnorm,
        "1-element fp32 tensor: sum (w - w0)^2 over the elements the block table privatises, deterministic",
        pybind11::arg("w"), pybind11::arg("w0"), pybind11::arg("table"));
  m.def("dp_apply", &dp_apply,
        "clip the update w - w0 to L2 norm clip (given its squared norm) and add N(0, (noise_multiplier clip)^2) "
        "to the privatised elements; a fresh arena, everything else copied from w",
        pybind11::arg("w"), pybind11::arg("w0"), pybind11::arg("table"), pybind11::arg("sqnorm"), pybind11::arg("clip"),
        pybind11::arg("noise_multiplier"), pybind11::arg("seed"), pybind11::arg("round"),
        pybind11::arg("out") = pybind11::none());
  m.def("adam_step", &adam_step, "fused whole-arena Adam/AdamW step");
  m.def("sgd_step", &sgd_step, "fused whole-arena SGD(+momentum/nesterov) step");
  m.def("adam_mt_step", &adam_mt_step, "multi-tensor Adam/AdamW over per-tensor grads into flat fp32 state",
        pybind11::arg("p"), pybind11::arg("m"), pybind11::arg("v"), pybind11::arg("pbf"), pybind11::arg("tens"),
        pybind11::arg("chunks"), pybind11::arg("grads"), pybind11::arg("numels"), pybind11::arg("grad_bf16"), pybind11::arg("grad_cl"),
        pybind11::arg("lr"), pybind11::arg("beta1"), pybind11::arg("beta2"), pybind11::arg("eps"),
        pybind11::arg("weight_decay"), pybind11::arg("step"), pybind11::arg("decoupled"),
        pybind11::arg("gtab") = pybind11::none(), pybind11::arg("t_dev") = pybind11::none());
  m.def("sgd_mt_step", &sgd_mt_step, "multi-tensor SGD over per-tensor grads into flat fp32 state", pybind11::arg("p"),
        pybind11::arg("buf"), pybind11::arg("pbf"), pybind11::arg("tens"), pybind11::arg("chunks"),
        pybind11::arg("grads"), pybind11::arg("numels"), pybind11::arg("grad_bf16"), pybind11::arg("grad_cl"), pybind11::arg("lr"),
        pybind11::arg("momentum"), pybind11::arg("dampening"), pybind11::arg("weight_decay"),
        pybind11::arg("nesterov"), pybind11::arg("first_step"), pybind11::arg("gtab") = pybind11::none());
  m.def("new_stream", &new_stream, "create a private non-blocking HIP stream on a device (returns its handle)",
        pybind11::arg("device"), pybind11::arg("priority") = 0);
  m.def("destroy_stream", &destroy_stream, "destroy a stream made by new_stream");
  register_cnn(m);
  register_fused(m);
  register_bn(m);
  register_rccl(m);
  register_gemm(m);
  register_conv(m);
  register_head(m);
}
