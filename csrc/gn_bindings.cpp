// PyTorch bindings of the fused GroupNorm kernels (groupnorm.hip).
// Activations are [N, HW, C] views of channels-last NHWC tensors.
#include <c10/core/DeviceGuard.h>
#include <c10/hip/HIPStream.h>
#include <torch/extension.h>

#include "groupnorm.h"

namespace {

hipStream_t stream() { return c10::hip::getCurrentHIPStream().stream(); }

bool act(const torch::Tensor& t, const torch::Tensor& like, const char* name) {
  TORCH_CHECK(t.is_cuda() && t.is_contiguous() && t.dim() == 3, name, " must be a contiguous [N, HW, C] GPU tensor");
  TORCH_CHECK(t.scalar_type() == torch::kBFloat16 || t.scalar_type() == torch::kFloat32, name, " must be bf16 or fp32");
  TORCH_CHECK(t.sizes() == like.sizes() && t.scalar_type() == like.scalar_type() && t.device() == like.device(), name,
              " must match x");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0, name, " must be 16-byte aligned");
  return t.scalar_type() == torch::kBFloat16;
}

// fp32 [n] on x's device; aligned: 16-byte vector loads (scale and shift)
float* f32(const torch::Tensor& t, int64_t n, const torch::Tensor& x, const char* name, bool aligned = false) {
  TORCH_CHECK(t.device() == x.device() && t.is_contiguous() && t.scalar_type() == torch::kFloat32 && t.numel() == n,
              name, " must be a contiguous fp32 tensor of ", n, " elements on x's device");
  TORCH_CHECK(!aligned || reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0, name, " must be 16-byte aligned");
  return t.data_ptr<float>();
}

// the kernels index with these: checked here, before any launch
void check_shape(const torch::Tensor& x, int64_t G) {
  TORCH_CHECK(x.dim() == 3, "x must be [N, HW, C]");
  const int64_t N = x.size(0), HW = x.size(1), C = x.size(2);
  TORCH_CHECK(N > 0 && HW > 0 && C > 0 && G > 0 && C % G == 0 && (C / G) % 8 == 0,
              "C / G must be a positive multiple of 8");
  TORCH_CHECK(HW <= (int64_t(1) << 22) && N < (int64_t(1) << 24) && C < (int64_t(1) << 24) &&
                  N * C < (int64_t(1) << 31) && N * HW * C < (int64_t(1) << 40),
              "shape out of range");
  TORCH_CHECK(p2gn::gn_plan(true, int(N), int(HW), int(C), int(G)).wpu != 0, "C / G must be at most 512");
}

// returns {y, mean, rstd}
std::vector<torch::Tensor> gn_fwd(torch::Tensor x, torch::Tensor w, torch::Tensor b, int64_t G,
                                  c10::optional<torch::Tensor> residual, double eps, bool relu) {
  const c10::DeviceGuard g(x.device());
  check_shape(x, G);
  const int64_t N = x.size(0), HW = x.size(1), C = x.size(2);
  const bool bf = act(x, x, "x");
  const void* rp = nullptr;
  if (residual.has_value() && residual->defined()) {
    act(*residual, x, "residual");
    rp = residual->data_ptr();
  }
  auto y = torch::empty_like(x);
  auto opt = x.options().dtype(torch::kFloat32);
  auto mean = torch::empty({N, G}, opt), rstd = torch::empty({N, G}, opt);
  p2gn::gn_fwd(bf, x.data_ptr(), rp, f32(w, C, x, "weight", true), f32(b, C, x, "bias", true), float(eps), y.data_ptr(),
               mean.data_ptr<float>(), rstd.data_ptr<float>(), int(N), int(HW), int(C), int(G), relu, stream());
  return {y, mean, rstd};
}

// returns {dx, dw, db} or {dx, dw, db, dres}; y is read only with relu
std::vector<torch::Tensor> gn_bwd(torch::Tensor dy, torch::Tensor y, torch::Tensor x, torch::Tensor w,
                                  torch::Tensor mean, torch::Tensor rstd, bool relu, bool need_dres) {
  const c10::DeviceGuard g(x.device());
  TORCH_CHECK(mean.dim() == 2, "mean must be [N, G]");
  const int64_t G = mean.size(1);
  check_shape(x, G);
  const int64_t N = x.size(0), HW = x.size(1), C = x.size(2);
  const bool bf = act(x, x, "x");
  act(dy, x, "dy");
  if (relu) act(y, x, "y");
  auto dx = torch::empty_like(x);
  auto dres = need_dres ? torch::empty_like(x) : torch::Tensor();
  auto opt = x.options().dtype(torch::kFloat32);
  auto dw = torch::empty({C}, opt), db = torch::empty({C}, opt), part = torch::empty({2, N, C}, opt);
  p2gn::gn_bwd(bf, dy.data_ptr(), relu ? y.data_ptr() : nullptr, x.data_ptr(), f32(w, C, x, "weight", true),
               f32(mean, N * G, x, "mean"), f32(rstd, N * G, x, "rstd"), dx.data_ptr(),
               need_dres ? dres.data_ptr() : nullptr, dw.data_ptr<float>(), db.data_ptr<float>(),
               part.data_ptr<float>(), int(N), int(HW), int(C), int(G), relu, stream());
  if (need_dres) return {dx, dw, db, dres};
  return {dx, dw, db};
}

}  // namespace

void register_gn(pybind11::module& m) {
  namespace py = pybind11;
  auto f = m.def_submodule("gn", "fused GroupNorm (+ residual) (+ ReLU) on channels-last [N, HW, C] activations");
  f.def("fwd", &gn_fwd, py::arg("x"), py::arg("w"), py::arg("b"), py::arg("groups"), py::arg("residual") = py::none(),
        py::arg("eps") = 1e-5, py::arg("relu") = true);
  f.def("bwd", &gn_bwd, py::arg("dy"), py::arg("y"), py::arg("x"), py::arg("w"), py::arg("mean"), py::arg("rstd"),
        py::arg("relu"), py::arg("need_dres"));
  f.def("plan", [](bool bf16, int64_t N, int64_t HW, int64_t C, int64_t G) {
          const auto p = p2gn::gn_plan(bf16, int(N), int(HW), int(C), int(G));
          return std::make_tuple(p.cs, p.ns, p.wpu, p.units, p.blocks);
        },
        "(cs, ns, wpu, units, blocks): slab width, slabs per sample, waves per unit (0: unsupported), units, workgroups",
        py::arg("bf16"), py::arg("N"), py::arg("HW"), py::arg("C"), py::arg("G"));
  f.def("residency", [](bool bf16, int64_t N, int64_t HW, int64_t C, int64_t G) {
          const auto r = p2gn::gn_residency(bf16, int(N), int(HW), int(C), int(G));
          return std::make_tuple(r.fwd_resident, r.bwd_keep, r.lds);
        },
        "(forward resident, backward slabs kept in LDS: 2 / 1 / 0, per-workgroup LDS granted) on the current device",
        py::arg("bf16"), py::arg("N"), py::arg("HW"), py::arg("C"), py::arg("G"));
}
