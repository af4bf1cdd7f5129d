// Adam's per-step scalars of the fused MNIST-CNN step, shared by the head launch
// (cnn_fwd.hip), which computes them once per training step, and the Adam roles of
// the backward launches (cnn_bwd.hip), which read them.
#pragma once
#include "cnn.h"
#include "common.h"

namespace p2cnn {

struct AdamScal {
  float step_size, inv_sqrt_bc2;
};
// The scalars at step (*t + t_off): two powf, a correctly rounded square root and two
// correctly rounded divisions, on values uniform across a launch.
P2_DEVICE AdamScal adam_scal_compute(const AdamCfg& c, const int* t, int t_off) {
  const float tt = float(*t + t_off);
  AdamScal s;
  s.step_size = c.lr / (1.f - powf(c.beta1, tt));
  s.inv_sqrt_bc2 = 1.f / sqrtf(1.f - powf(c.beta2, tt));
  return s;
}
// What an Adam role uses: the step's scalars as its head launch left them in c.scal
// (a wave-uniform address), or, without that buffer, computed by every thread.  Both
// come from adam_scal_compute on the same inputs, so they are the same bits.
P2_DEVICE AdamScal adam_scal(const AdamCfg& c, const int* t, int t_off) {
  if (c.scal) return AdamScal{c.scal[0], c.scal[1]};
  return adam_scal_compute(c, t, t_off);
}

}  // namespace p2cnn
