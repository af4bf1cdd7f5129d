// PyTorch bindings of the fused MLP step (csrc/mlp.hip): Linear+ReLU, Linear+ReLU,
// Linear, softmax cross-entropy -- two launches forward (the second also
// produces the activation gradients when training), one for all six parameter
// gradients.  Every shape / dtype / device / alignment assumption of the
// kernels is checked here.
#include <c10/core/DeviceGuard.h>
#include <c10/hip/HIPStream.h>
#include <torch/extension.h>

#include "mlp.h"

namespace {

hipStream_t stream() { return c10::hip::getCurrentHIPStream().stream(); }

bool aligned16(const torch::Tensor& t) { return reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0; }

const uint16_t* bf(const torch::Tensor& t) { return reinterpret_cast<const uint16_t*>(t.data_ptr()); }
uint16_t* bf_mut(torch::Tensor& t) { return reinterpret_cast<uint16_t*>(t.data_ptr()); }

void check_x(const torch::Tensor& x) {
  TORCH_CHECK(x.is_cuda() && x.dim() == 2 && x.is_contiguous() && aligned16(x) &&
                  (x.scalar_type() == torch::kFloat32 || x.scalar_type() == torch::kBFloat16),
              "mlp: x must be a contiguous, 16-byte aligned fp32/bf16 [B, K0] GPU tensor");
  TORCH_CHECK(x.size(0) >= 1 && x.size(1) >= 16 && x.size(1) % 16 == 0 && x.numel() < (int64_t(1) << 31),
              "mlp: B >= 1, K0 a positive multiple of 16, B * K0 < 2^31");
}

void check_layer(const torch::Tensor& w, const torch::Tensor& b, const torch::Tensor& x, int64_t in, const char* name) {
  TORCH_CHECK(w.is_cuda() && w.device() == x.device() && w.scalar_type() == torch::kBFloat16 && w.dim() == 2 &&
                  w.is_contiguous() && w.size(1) == in && aligned16(w),
              "mlp: ", name, ".weight must be a contiguous, 16-byte aligned bf16 [out, ", in, "] tensor on x's device");
  TORCH_CHECK(b.device() == x.device() && b.scalar_type() == torch::kFloat32 && b.dim() == 1 && b.is_contiguous() &&
                  b.size(0) == w.size(0),
              "mlp: ", name, ".bias must be a contiguous fp32 [out] tensor on x's device");
}

p2::MlpDims dims_of(int64_t B, int64_t K0, int64_t H1, int64_t H2, int64_t C) {
  TORCH_CHECK(H1 >= 32 && H1 % 32 == 0 && H1 <= p2::kMlpMaxH1, "mlp: H1 must be a multiple of 32, at most ", p2::kMlpMaxH1);
  TORCH_CHECK(H2 >= 32 && H2 % 32 == 0 && H2 <= p2::kMlpMaxH2, "mlp: H2 must be a multiple of 32, at most ", p2::kMlpMaxH2);
  TORCH_CHECK(C >= 1 && C <= p2::kMlpMaxC, "mlp: 1 <= C <= ", p2::kMlpMaxC, " classes");
  const int64_t Bpad = (B + 31) / 32 * 32;
  TORCH_CHECK(Bpad * (2 * H1 + 2 * H2 + p2::kMlpMaxC) < (int64_t(1) << 31), "mlp: batch too large");
  return p2::MlpDims{int(B), int(Bpad), int(K0), int(H1), int(H2), int(C)};
}

// -> {mean loss (), logits [B, C] fp32, accuracy (), acts}: acts is the bf16
// [2 H1 + 2 H2 + 32, Bpad] workspace mlp.bwd consumes (empty unless train)
std::vector<torch::Tensor> mlp_fwd(torch::Tensor x, torch::Tensor w1, torch::Tensor b1, torch::Tensor w2,
                                   torch::Tensor b2, torch::Tensor w3, torch::Tensor b3, torch::Tensor y,
                                   torch::Tensor counter, bool train) {
  check_x(x);
  const int64_t B = x.size(0), K0 = x.size(1);
  check_layer(w1, b1, x, K0, "l1");
  check_layer(w2, b2, x, w1.size(0), "l2");
  check_layer(w3, b3, x, w2.size(0), "l3");
  const p2::MlpDims d = dims_of(B, K0, w1.size(0), w2.size(0), w3.size(0));
  TORCH_CHECK(y.device() == x.device() && y.scalar_type() == torch::kInt64 && y.dim() == 1 && y.is_contiguous() &&
                  y.size(0) == B,
              "mlp: y must be a contiguous int64 [B] tensor on x's device");
  TORCH_CHECK(counter.device() == x.device() && counter.scalar_type() == torch::kInt32 && counter.numel() >= 1 &&
                  counter.is_contiguous(),
              "mlp: the loss needs a zeroed int32 counter on x's device");
  const c10::DeviceGuard g(x.device());
  auto f32 = x.options().dtype(torch::kFloat32), b16 = x.options().dtype(torch::kBFloat16);
  auto h1 = torch::empty({2, B, int64_t(d.H1)}, b16);  // hi and lo planes
  auto logits = torch::empty({B, int64_t(d.C)}, f32);
  auto parts = torch::empty({2 * int64_t(d.Bpad / 32)}, f32);
  auto loss = torch::empty({}, f32), acc = torch::empty({}, f32);
  auto acts = torch::empty({train ? int64_t(p2::mlp_acts_rows(d)) : 0, int64_t(d.Bpad)}, b16);
  const bool xb = x.scalar_type() == torch::kBFloat16;
  p2::mlp_l1(x.data_ptr(), xb, bf(w1), b1.data_ptr<float>(), bf_mut(h1), d, stream());
  p2::mlp_tail(bf(h1), bf(w2), b2.data_ptr<float>(), bf(w3), b3.data_ptr<float>(), y.data_ptr<int64_t>(),
               logits.data_ptr<float>(), parts.data_ptr<float>(), loss.data_ptr<float>(), acc.data_ptr<float>(),
               counter.data_ptr<int>(), train ? bf_mut(acts) : nullptr, train ? 1 : 0, d, stream());
  return {loss, logits, acc, acts};
}

// -> {dW1, db1, dW2, db2, dW3, db3}: weights' gradients bf16, biases' fp32
std::vector<torch::Tensor> mlp_bwd(torch::Tensor gloss, torch::Tensor x, torch::Tensor acts, int64_t H1, int64_t H2,
                                   int64_t C) {
  check_x(x);
  const int64_t B = x.size(0), K0 = x.size(1);
  const p2::MlpDims d = dims_of(B, K0, H1, H2, C);
  TORCH_CHECK(acts.device() == x.device() && acts.scalar_type() == torch::kBFloat16 && acts.dim() == 2 &&
                  acts.is_contiguous() && acts.size(0) == p2::mlp_acts_rows(d) && acts.size(1) == d.Bpad &&
                  aligned16(acts),
              "mlp_bwd: acts must be the workspace of a training mlp.fwd on the same x");
  TORCH_CHECK(gloss.device() == x.device() && gloss.scalar_type() == torch::kFloat32 && gloss.numel() == 1,
              "mlp_bwd: gloss must be an fp32 scalar tensor on x's device");
  auto gl = gloss.contiguous();
  const c10::DeviceGuard g(x.device());
  auto f32 = x.options().dtype(torch::kFloat32), b16 = x.options().dtype(torch::kBFloat16);
  auto dw1 = torch::empty({H1, K0}, b16), dw2 = torch::empty({H2, H1}, b16), dw3 = torch::empty({C, H2}, b16);
  auto db1 = torch::empty({H1}, f32), db2 = torch::empty({H2}, f32), db3 = torch::empty({C}, f32);
  p2::mlp_wgrad(gl.data_ptr<float>(), x.data_ptr(), x.scalar_type() == torch::kBFloat16, bf(acts), bf_mut(dw1),
                db1.data_ptr<float>(), bf_mut(dw2), db2.data_ptr<float>(), bf_mut(dw3), db3.data_ptr<float>(), d, stream());
  return {dw1, db1, dw2, db2, dw3, db3};
}

}  // namespace

void register_mlp(pybind11::module& m) {
  namespace py = pybind11;
  auto h = m.def_submodule("mlp", "fused MLP step: Linear+ReLU x 2, Linear, softmax cross-entropy (three launches)");
  h.def("fwd", &mlp_fwd, py::arg("x"), py::arg("w1"), py::arg("b1"), py::arg("w2"), py::arg("b2"), py::arg("w3"),
        py::arg("b3"), py::arg("y"), py::arg("counter"), py::arg("train"));
  h.def("bwd", &mlp_bwd, py::arg("gloss"), py::arg("x"), py::arg("acts"), py::arg("H1"), py::arg("H2"), py::arg("C"));
}
