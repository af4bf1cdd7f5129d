// PyTorch bindings of the fused transformer / classifier ops (fused_ops.hip).
#include <c10/core/DeviceGuard.h>
#include <c10/hip/HIPStream.h>
#include <torch/extension.h>

#include <cmath>

#include "attention.h"
#include "fused_ops.h"

namespace {

hipStream_t stream() { return c10::hip::getCurrentHIPStream().stream(); }

// what every kernel's 16-byte vector accesses need of a tensor
void check_vec16(const torch::Tensor& t, const char* name) {
  TORCH_CHECK(t.is_cuda() && t.is_contiguous(), name, " must be a contiguous GPU tensor");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0, name, " must be 16-byte aligned");
}

bool act_dtype(const torch::Tensor& t, const char* name) {
  check_vec16(t, name);
  TORCH_CHECK(t.scalar_type() == torch::kBFloat16 || t.scalar_type() == torch::kFloat32, name, " must be bf16 or fp32");
  return t.scalar_type() == torch::kBFloat16;
}

void check_bf16(const torch::Tensor& t, const char* name) {
  check_vec16(t, name);
  TORCH_CHECK(t.scalar_type() == torch::kBFloat16, name, " must be bf16");
}

uint16_t* bf16_ptr(const torch::Tensor& t) { return reinterpret_cast<uint16_t*>(t.data_ptr()); }

void check_f32(const torch::Tensor& t, int64_t n, const char* name) {
  TORCH_CHECK(t.is_cuda() && t.is_contiguous() && t.scalar_type() == torch::kFloat32, name, " must be contiguous fp32 on GPU");
  TORCH_CHECK(t.numel() >= n, name, " too small");
}

// a second activation of an op (dy, residual, gsum): x's shape, dtype and device, and as accessible
void check_like(const torch::Tensor& t, const torch::Tensor& x, const char* name) {
  act_dtype(t, name);
  TORCH_CHECK(t.sizes() == x.sizes() && t.scalar_type() == x.scalar_type() && t.device() == x.device(), name,
              " must match x");
}

bool present(const c10::optional<torch::Tensor>& t) { return t.has_value() && t->defined(); }

// uint8 [B, C, H, W] -> bf16 [B, (H/P)(W/P), C P P] / 255
torch::Tensor patchify_u8(torch::Tensor x, int64_t P) {
  const c10::DeviceGuard g(x.device());
  TORCH_CHECK(x.is_cuda() && x.is_contiguous() && x.scalar_type() == torch::kUInt8 && x.dim() == 4,
              "patchify_u8: x must be a contiguous uint8 [B, C, H, W] GPU tensor");
  const int64_t B = x.size(0), C = x.size(1), H = x.size(2), W = x.size(3);
  TORCH_CHECK(P > 0 && P % 8 == 0 && H % P == 0 && W % P == 0, "patchify_u8: P % 8 == 0 and P | H, W");
  auto out = torch::empty({B, (H / P) * (W / P), C * P * P}, x.options().dtype(torch::kBFloat16));
  if (out.numel() > 0)
    p2fused::patchify_u8(x.data_ptr<uint8_t>(), bf16_ptr(out), int(B), int(C), int(H), int(W), int(P), stream());
  return out;
}

// y [B, N, D], cls [D], pos [N + 1, D] (bf16) -> h [B, N + 1, D]
torch::Tensor embed_tokens_fwd(torch::Tensor y, torch::Tensor cls, torch::Tensor pos) {
  const c10::DeviceGuard g(y.device());
  check_bf16(y, "y");
  check_bf16(cls, "cls");
  check_bf16(pos, "pos");
  TORCH_CHECK(y.dim() == 3, "embed_tokens: y must be [B, N, D]");
  const int64_t B = y.size(0), N = y.size(1), D = y.size(2);
  TORCH_CHECK(D % 8 == 0 && cls.numel() == D && pos.numel() == (N + 1) * D, "embed_tokens: shapes");
  TORCH_CHECK(cls.device() == y.device() && pos.device() == y.device(), "embed_tokens: devices");
  auto h = torch::empty({B, N + 1, D}, y.options());
  if (h.numel() > 0)
    p2fused::embed_tokens_fwd(bf16_ptr(y), bf16_ptr(cls), bf16_ptr(pos), bf16_ptr(h), int(B), int(N), int(D), stream());
  return h;
}

// dh [B, N + 1, D] -> (dy [B, N, D], dpos [N + 1, D], dcls [D])
std::vector<torch::Tensor> embed_tokens_bwd(torch::Tensor dh) {
  const c10::DeviceGuard g(dh.device());
  check_bf16(dh, "dh");
  TORCH_CHECK(dh.dim() == 3 && dh.size(1) >= 1 && dh.size(2) % 8 == 0, "embed_tokens_bwd: dh must be [B, N + 1, D]");
  const int64_t B = dh.size(0), N = dh.size(1) - 1, D = dh.size(2);
  auto dy = torch::empty({B, N, D}, dh.options());
  auto dpos = torch::empty({N + 1, D}, dh.options());
  auto dcls = torch::empty({D}, dh.options());
  if (dpos.numel() > 0)
    p2fused::embed_tokens_bwd(bf16_ptr(dh), bf16_ptr(dy), bf16_ptr(dpos), bf16_ptr(dcls), int(B), int(N), int(D), stream());
  return {dy, dpos, dcls};
}

// ---- LayerNorm ------------------------------------------------------------------
// x [N, C] as the kernels take it and its fp32 weight; the forward and both backward bindings
bool ln_check(const torch::Tensor& x, const torch::Tensor& w) {
  TORCH_CHECK(x.dim() == 2, "x must be [N, C]");
  const int64_t C = x.size(1);
  TORCH_CHECK(C % 8 == 0 && C <= p2fused::kMaxLnCols, "C must be a multiple of 8 and <= ", p2fused::kMaxLnCols);
  check_f32(w, C, "weight");
  return act_dtype(x, "x");
}

std::vector<torch::Tensor> ln_fwd(torch::Tensor x, torch::Tensor w, torch::Tensor b, double eps,
                                  c10::optional<torch::Tensor> residual) {
  const c10::DeviceGuard g(x.device());
  const bool bf = ln_check(x, w);
  const int64_t N = x.size(0), C = x.size(1);
  check_f32(b, C, "bias");
  const bool has_res = present(residual);
  if (has_res) check_like(*residual, x, "residual");
  auto y = torch::empty_like(x);
  auto sum = has_res ? torch::empty_like(x) : torch::Tensor();
  auto opt = x.options().dtype(torch::kFloat32);
  auto mean = torch::empty({N}, opt), rstd = torch::empty({N}, opt);
  if (N > 0)
    p2fused::layer_norm_fwd(bf, x.data_ptr(), has_res ? residual->data_ptr() : nullptr, w.data_ptr<float>(),
                            b.data_ptr<float>(), y.data_ptr(), has_res ? sum.data_ptr() : nullptr,
                            mean.data_ptr<float>(), rstd.data_ptr<float>(), int(N), int(C), float(eps), stream());
  if (has_res) return {y, mean, rstd, sum};
  return {y, mean, rstd};
}

// reduce: (dx, dgamma, dbeta); else (dx and the [G, C] partials), their column reduction left to
// col_reduce_multi (a training step's deferred parameter-gradient reductions, ops/fused.py
// deferred_param_grads).  The same holds for the bias+GELU backward and the column sums below.
std::vector<torch::Tensor> ln_bwd_any(const torch::Tensor& dy, const torch::Tensor& x, const torch::Tensor& w,
                                      const torch::Tensor& mean, const torch::Tensor& rstd,
                                      const c10::optional<torch::Tensor>& gsum, bool reduce) {
  const c10::DeviceGuard g(x.device());
  const bool bf = ln_check(x, w);
  const int64_t N = x.size(0), C = x.size(1);
  TORCH_CHECK(reduce || N > 0, "ln_bwd_parts: empty input");
  check_like(dy, x, "dy");
  check_f32(mean, N, "mean");
  check_f32(rstd, N, "rstd");
  const bool has_gs = present(gsum);
  if (has_gs) check_like(*gsum, x, "gsum");
  auto dx = torch::empty_like(x);
  auto opt = x.options().dtype(torch::kFloat32);
  torch::Tensor pdw, pdb, dw, db;
  if (reduce) dw = torch::empty({C}, opt), db = torch::empty({C}, opt);  // col_reduce writes every column
  if (N > 0) {
    const int G = p2fused::layer_norm_bwd_blocks(int(N));
    pdw = torch::empty({G, C}, opt), pdb = torch::empty({G, C}, opt);
    p2fused::layer_norm_bwd(bf, dy.data_ptr(), x.data_ptr(), w.data_ptr<float>(), mean.data_ptr<float>(),
                            rstd.data_ptr<float>(), has_gs ? gsum->data_ptr() : nullptr, dx.data_ptr(),
                            pdw.data_ptr<float>(), pdb.data_ptr<float>(), reduce ? dw.data_ptr<float>() : nullptr,
                            reduce ? db.data_ptr<float>() : nullptr, int(N), int(C), stream());
  } else {
    dw.zero_();
    db.zero_();
  }
  if (reduce) return {dx, dw, db};
  return {dx, pdw, pdb};
}

std::vector<torch::Tensor> ln_bwd(torch::Tensor dy, torch::Tensor x, torch::Tensor w, torch::Tensor mean,
                                  torch::Tensor rstd, c10::optional<torch::Tensor> gsum) {
  return ln_bwd_any(dy, x, w, mean, rstd, gsum, true);
}

std::vector<torch::Tensor> ln_bwd_parts(torch::Tensor dy, torch::Tensor x, torch::Tensor w, torch::Tensor mean,
                                        torch::Tensor rstd, c10::optional<torch::Tensor> gsum) {
  return ln_bwd_any(dy, x, w, mean, rstd, gsum, false);
}

// ---- bias + GELU ----------------------------------------------------------------
// x [..., H] and its fp32 bias; the forward and both backward bindings
bool gelu_check(const torch::Tensor& x, const torch::Tensor& b) {
  const int64_t H = x.size(-1);
  TORCH_CHECK(H % 8 == 0, "last dim must be a multiple of 8");
  check_f32(b, H, "bias");
  return act_dtype(x, "x");
}

torch::Tensor bias_gelu_fwd(torch::Tensor x, torch::Tensor b) {
  const c10::DeviceGuard g(x.device());
  const bool bf = gelu_check(x, b);
  auto y = torch::empty_like(x);
  if (x.numel() > 0)
    p2fused::bias_gelu_fwd(bf, x.data_ptr(), b.data_ptr<float>(), y.data_ptr(), x.numel(), int(x.size(-1)), stream());
  return y;
}

std::vector<torch::Tensor> bias_gelu_bwd_any(const torch::Tensor& dy, const torch::Tensor& x, const torch::Tensor& b,
                                             bool reduce) {
  const c10::DeviceGuard g(x.device());
  const bool bf = gelu_check(x, b);
  const int64_t H = x.size(-1), N = x.numel() / std::max<int64_t>(H, 1);
  TORCH_CHECK(reduce || N > 0, "bias_gelu_bwd_parts: empty input");
  check_like(dy, x, "dy");
  auto dx = torch::empty_like(x);
  auto opt = x.options().dtype(torch::kFloat32);
  torch::Tensor pdb, db;
  if (reduce) db = torch::empty({H}, opt);  // col_reduce writes every column
  if (N > 0) {
    pdb = torch::empty({p2fused::bias_gelu_bwd_splits(int(N)), H}, opt);
    p2fused::bias_gelu_bwd(bf, dy.data_ptr(), x.data_ptr(), b.data_ptr<float>(), dx.data_ptr(), pdb.data_ptr<float>(),
                           reduce ? db.data_ptr<float>() : nullptr, int(N), int(H), stream());
  } else {
    db.zero_();
  }
  if (reduce) return {dx, db};
  return {dx, pdb};
}

std::vector<torch::Tensor> bias_gelu_bwd(torch::Tensor dy, torch::Tensor x, torch::Tensor b) {
  return bias_gelu_bwd_any(dy, x, b, true);
}

std::vector<torch::Tensor> bias_gelu_bwd_parts(torch::Tensor dy, torch::Tensor x, torch::Tensor b) {
  return bias_gelu_bwd_any(dy, x, b, false);
}

// ---- column sums ----------------------------------------------------------------
// reduce: the [H] sums (fp32, or bf16 with bf16_out); else the [S, H] partials of a non-empty x
torch::Tensor column_sum_any(const torch::Tensor& x, bool bf16_out, bool reduce) {
  const c10::DeviceGuard g(x.device());
  TORCH_CHECK(x.dim() == 2 && (reduce || x.size(0) > 0), reduce ? "x must be [N, H]" : "x must be a non-empty [N, H]");
  const int64_t N = x.size(0), H = x.size(1);
  TORCH_CHECK(H % 8 == 0, "H must be a multiple of 8");
  const bool bf = act_dtype(x, "x");
  auto opt = x.options().dtype(torch::kFloat32);
  torch::Tensor part, out;
  if (reduce) out = torch::empty({H}, bf16_out ? x.options().dtype(torch::kBFloat16) : opt);
  if (N > 0) {
    part = torch::empty({p2fused::bias_gelu_bwd_splits(int(N)), H}, opt);
    p2fused::column_sum(bf, x.data_ptr(), part.data_ptr<float>(), reduce && !bf16_out ? out.data_ptr<float>() : nullptr,
                        reduce && bf16_out ? bf16_ptr(out) : nullptr, int(N), int(H), stream());
  } else {
    out.zero_();
  }
  return reduce ? out : part;
}

torch::Tensor column_sum(torch::Tensor x, bool bf16_out) { return column_sum_any(x, bf16_out, true); }

torch::Tensor column_sum_parts(torch::Tensor x) { return column_sum_any(x, false, false); }

// parts[i] = the [S, H] column partials of xs[i] (bf16 [N, H], N > 0), many per launch
void column_sum_parts_multi(std::vector<torch::Tensor> xs, std::vector<torch::Tensor> parts) {
  TORCH_CHECK(xs.size() == parts.size(), "column_sum_parts_multi: xs / parts length mismatch");
  if (xs.empty()) return;
  const c10::DeviceGuard g(xs[0].device());
  p2fused::CsJobs jobs{};
  for (size_t i = 0; i < xs.size(); ++i) {
    const auto& x = xs[i];
    const auto& pt = parts[i];
    check_bf16(x, "column_sum_parts_multi: xs[i]");
    TORCH_CHECK(x.dim() == 2 && x.size(0) > 0 && x.size(1) % 8 == 0,
                "column_sum_parts_multi: xs must be non-empty [N, H] (H % 8 == 0)");
    const int N = int(x.size(0)), H = int(x.size(1)), S = p2fused::bias_gelu_bwd_splits(N);
    TORCH_CHECK(pt.is_cuda() && pt.scalar_type() == torch::kFloat32 && pt.is_contiguous() && pt.dim() == 2 &&
                    pt.size(0) == S && pt.size(1) == H && pt.device() == x.device() && x.device() == xs[0].device(),
                "column_sum_parts_multi: parts[i] must be contiguous fp32 [bias_gelu_bwd_splits(N), H] on xs' device");
    jobs.j[jobs.n++] = p2fused::CsJob{bf16_ptr(x), pt.data_ptr<float>(), N, H, S, 0};
    if (jobs.n == p2fused::kCsMaxJobs || i + 1 == xs.size()) {
      p2fused::colsum_multi(jobs, stream());
      jobs.n = 0;
    }
  }
}

int64_t colsum_splits(int64_t N) { return p2fused::bias_gelu_bwd_splits(int(N)); }

// outs[i] (fp32 or bf16 [C]) = column sums of parts[i] (fp32 [R, C]), up to kCrMaxJobs per launch
void col_reduce_multi(std::vector<torch::Tensor> parts, std::vector<torch::Tensor> outs) {
  TORCH_CHECK(parts.size() == outs.size(), "col_reduce_multi: parts / outs length mismatch");
  if (parts.empty()) return;
  const c10::DeviceGuard g(parts[0].device());
  p2fused::CrJobs jobs{};
  for (size_t i = 0; i < parts.size(); ++i) {
    const auto& a = parts[i];
    const auto& o = outs[i];
    TORCH_CHECK(a.is_cuda() && a.scalar_type() == torch::kFloat32 && a.dim() == 2 && a.is_contiguous() && a.size(0) > 0,
                "col_reduce_multi: parts must be non-empty contiguous fp32 [R, C] GPU tensors");
    TORCH_CHECK(a.device() == parts[0].device() && o.device() == a.device(), "col_reduce_multi: one device");
    TORCH_CHECK(o.is_contiguous() && o.numel() == a.size(1) &&
                    (o.scalar_type() == torch::kFloat32 || o.scalar_type() == torch::kBFloat16),
                "col_reduce_multi: outs must be contiguous fp32 / bf16 [C] matching their partials");
    const bool bf = o.scalar_type() == torch::kBFloat16;
    jobs.j[jobs.n++] = p2fused::CrJob{a.data_ptr<float>(), bf ? nullptr : o.data_ptr<float>(), nullptr, nullptr,
                                      bf ? bf16_ptr(o) : nullptr, int(a.size(0)), int(a.size(1)), 0, 0};
    if (jobs.n == p2fused::kCrMaxJobs || i + 1 == parts.size()) {
      p2fused::col_reduce_multi(jobs, stream());
      jobs.n = 0;
    }
  }
}

torch::Tensor split_sum_bf16(torch::Tensor parts) {
  const c10::DeviceGuard g(parts.device());
  check_bf16(parts, "parts");
  TORCH_CHECK(parts.dim() >= 2, "parts must be [S, ...]");
  const int64_t S = parts.size(0), n = parts.numel() / std::max<int64_t>(S, 1);
  TORCH_CHECK(S >= 1 && n % 8 == 0, "split_sum_bf16: S >= 1 and a multiple-of-8 slice required");
  auto out = torch::empty(parts.sizes().slice(1), parts.options());
  if (n > 0) p2fused::split_sum_bf16(bf16_ptr(parts), bf16_ptr(out), n, int(S), stream());
  return out;
}

// ---- softmax cross-entropy --------------------------------------------------------
// logits [N, K] and their int64 labels [N]; the forward and the backward binding
bool xent_check(const torch::Tensor& z, const torch::Tensor& y) {
  TORCH_CHECK(z.dim() == 2, "logits must be [N, K]");
  TORCH_CHECK(y.is_cuda() && y.scalar_type() == torch::kInt64 && y.is_contiguous() && y.numel() == z.size(0) &&
                  y.device() == z.device(),
              "labels must be int64 [N] on the logits' GPU");
  return act_dtype(z, "logits");
}

std::vector<torch::Tensor> xent_fwd(torch::Tensor z, torch::Tensor y) {
  const c10::DeviceGuard g(z.device());
  const bool bf = xent_check(z, y);
  const int64_t N = z.size(0), K = z.size(1);
  auto opt = z.options().dtype(torch::kFloat32);
  auto loss = torch::empty({N}, opt), lse = torch::empty({N}, opt);
  if (N > 0) p2fused::xent_fwd(bf, z.data_ptr(), y.data_ptr<int64_t>(), loss.data_ptr<float>(), lse.data_ptr<float>(), int(N), int(K), stream());
  return {loss, lse};
}

torch::Tensor xent_bwd(torch::Tensor z, torch::Tensor y, torch::Tensor lse, torch::Tensor gscale) {
  const c10::DeviceGuard g(z.device());
  const bool bf = xent_check(z, y);
  const int64_t N = z.size(0), K = z.size(1);
  check_f32(lse, N, "lse");
  check_f32(gscale, 1, "grad");
  auto dz = torch::empty_like(z);
  if (N > 0)
    p2fused::xent_bwd(bf, z.data_ptr(), y.data_ptr<int64_t>(), lse.data_ptr<float>(), gscale.data_ptr<float>(),
                      dz.data_ptr(), int(N), int(K), stream());
  return dz;
}

// ---- fused attention over the QKV projection output --------------------------
p2attn::AttnShape attn_shape(const torch::Tensor& qkv, int64_t heads) {
  check_bf16(qkv, "qkv");
  TORCH_CHECK(qkv.dim() == 3, "qkv must be [B, T, 3C]");
  const int64_t B = qkv.size(0), T = qkv.size(1), C3 = qkv.size(2);
  TORCH_CHECK(C3 % 3 == 0 && heads > 0 && (C3 / 3) == heads * p2attn::kHeadDim, "qkv last dim must be 3 * heads * 64");
  TORCH_CHECK(T >= 1 && T <= p2attn::kMaxT, "attention kernel supports 1..256 tokens");
  TORCH_CHECK(B <= 65535 && heads <= 65535, "grid limits");
  p2attn::AttnShape sh{};
  sh.B = int(B);
  sh.H = int(heads);
  sh.T = int(T);
  sh.C = int(C3 / 3);
  sh.qkv_row = C3;
  sh.qkv_batch = T * C3;
  sh.o_row = sh.C;
  sh.o_batch = T * sh.C;
  sh.scale = float(1.0 / std::sqrt(double(p2attn::kHeadDim)));
  return sh;
}

std::vector<torch::Tensor> attn_fwd(torch::Tensor qkv, int64_t heads) {
  const c10::DeviceGuard g(qkv.device());
  const auto sh = attn_shape(qkv, heads);
  auto o = torch::empty({qkv.size(0), qkv.size(1), int64_t(sh.C)}, qkv.options());
  auto lse = torch::empty({qkv.size(0), heads, qkv.size(1)}, qkv.options().dtype(torch::kFloat32));
  if (sh.B > 0) p2attn::attention_fwd(bf16_ptr(qkv), bf16_ptr(o), lse.data_ptr<float>(), sh, stream());
  return {o, lse};
}

torch::Tensor attn_bwd(torch::Tensor qkv, torch::Tensor o, torch::Tensor dout, torch::Tensor lse, int64_t heads) {
  const c10::DeviceGuard g(qkv.device());
  const auto sh = attn_shape(qkv, heads);
  for (auto* t : {&o, &dout}) {
    check_bf16(*t, "o / dout");
    TORCH_CHECK(t->dim() == 3 && t->size(0) == sh.B && t->size(1) == sh.T && t->size(2) == sh.C,
                "o / dout must be [B, T, C]");
  }
  TORCH_CHECK(lse.is_cuda() && lse.is_contiguous() && lse.scalar_type() == torch::kFloat32 &&
                  lse.numel() == int64_t(sh.B) * sh.H * sh.T,
              "lse must be the forward's fp32 [B, H, T]");
  auto dqkv = torch::empty_like(qkv);
  if (sh.B > 0)
    p2attn::attention_bwd(bf16_ptr(qkv), bf16_ptr(o), bf16_ptr(dout), lse.data_ptr<float>(), bf16_ptr(dqkv), sh, stream());
  return dqkv;
}

// dsts[i] <- srcs[i] for every pair, one launch (same byte size per pair, any dtype)
void multi_copy(std::vector<torch::Tensor> dsts, std::vector<torch::Tensor> srcs) {
  TORCH_CHECK(dsts.size() == srcs.size() && !dsts.empty() && int(dsts.size()) <= p2fused::kMaxCopies,
              "multi_copy: 1..", p2fused::kMaxCopies, " (dst, src) pairs");
  const c10::DeviceGuard g(dsts[0].device());
  p2fused::CopyList cl{};
  cl.n = int(dsts.size());
  for (int i = 0; i < cl.n; ++i) {
    const auto &d = dsts[i], &s = srcs[i];
    TORCH_CHECK(d.is_cuda() && s.is_cuda() && d.device() == s.device() && d.device() == dsts[0].device(),
                "multi_copy: tensors must be on one GPU");
    TORCH_CHECK(d.is_contiguous() && s.is_contiguous(), "multi_copy: tensors must be contiguous");
    const int64_t nb = d.numel() * d.element_size();
    TORCH_CHECK(nb == s.numel() * s.element_size() && nb % 4 == 0, "multi_copy: pair ", i, " byte sizes differ or not % 4");
    TORCH_CHECK(reinterpret_cast<uintptr_t>(d.data_ptr()) % 16 == 0 && reinterpret_cast<uintptr_t>(s.data_ptr()) % 16 == 0,
                "multi_copy: pair ", i, " not 16-byte aligned");
    cl.dst[i] = d.data_ptr();
    cl.src[i] = s.data_ptr();
    cl.bytes[i] = nb;
  }
  p2fused::multi_copy(cl, stream());
}

}  // namespace

void register_fused(pybind11::module& m) {
  auto f = m.def_submodule("fused", "fused LayerNorm / bias+GELU / softmax cross-entropy kernels");
  f.def("patchify_u8", &patchify_u8, "uint8 images -> bf16 ViT patch rows / 255", pybind11::arg("x"), pybind11::arg("P"));
  f.def("embed_tokens_fwd", &embed_tokens_fwd, "cat(cls, y) + pos in one pass (bf16)");
  f.def("embed_tokens_bwd", &embed_tokens_bwd, "dy = dh[:, 1:], dpos = sum_b dh, dcls = dpos[0]");
  f.def("ln_fwd", &ln_fwd, pybind11::arg("x"), pybind11::arg("w"), pybind11::arg("b"), pybind11::arg("eps"),
        pybind11::arg("residual") = pybind11::none());
  f.def("ln_bwd", &ln_bwd, pybind11::arg("dy"), pybind11::arg("x"), pybind11::arg("w"), pybind11::arg("mean"),
        pybind11::arg("rstd"), pybind11::arg("gsum") = pybind11::none());
  f.def("column_sum", &column_sum, "column sums of a [N, H] bf16/fp32 activation (linear bias gradient), fp32 or bf16 out",
        pybind11::arg("x"), pybind11::arg("bf16_out") = false);
  f.def("ln_bwd_parts", &ln_bwd_parts, "LayerNorm backward: dx and the [G, C] dgamma / dbeta partials");
  f.def("bias_gelu_bwd_parts", &bias_gelu_bwd_parts, "bias+GELU backward: dx and the [S, H] dbias partials");
  f.def("column_sum_parts", &column_sum_parts, "[S, H] partial column sums of a [N, H] activation");
  f.def("col_reduce_multi", &col_reduce_multi, "outs[i] = column sums of parts[i], many per launch");
  f.def("column_sum_parts_multi", &column_sum_parts_multi, "parts[i] = column_sum partials of xs[i], many per launch");
  f.def("colsum_splits", &colsum_splits, "row splits S of column_sum's [S, H] partials for N rows");
  f.def("multi_copy", &multi_copy, "dsts[i] <- srcs[i] for up to 12 pairs in one launch");
  f.def("split_sum_bf16", &split_sum_bf16, "bf16 sum over dim 0 of [S, ...] bf16 partials, fp32 accumulation");
  f.def("bias_gelu_fwd", &bias_gelu_fwd);
  f.def("bias_gelu_bwd", &bias_gelu_bwd);
  f.def("xent_fwd", &xent_fwd);
  f.def("xent_bwd", &xent_bwd);
  f.def("attn_fwd", &attn_fwd, "fused MHSA forward over [B, T, 3C] qkv (head dim 64, T <= 256) -> (o, lse)");
  f.def("attn_bwd", &attn_bwd, "fused MHSA backward -> dqkv [B, T, 3C]");
}
