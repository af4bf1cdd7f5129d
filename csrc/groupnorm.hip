// Fused GroupNorm (+ residual add) (+ ReLU) for MI355X (gfx950, wave64), on
// channels-last activations read as N matrices [HW, C].
//
// GroupNorm statistics are per sample, so the unit of work is (sample, slab of
// whole groups) and a unit small enough stays in LDS between its statistics
// and its apply: every tensor crosses HBM once.
//   forward   x (and res) read once, y written once            (BatchNorm: statistics + apply)
//   backward  dy, y, x read once, dx (and dres) written once   (BatchNorm: statistics + apply)
//
// Work unit.  A slab is cs channels: the smallest multiple of cpg whose row
// segment is at least 64 bytes (32 bf16 / 16 fp32 channels), at most C; the
// last slab of a sample may be narrower.  64-byte segments rather than wider
// ones because the CIFAR ResNet layers have few samples and many CUs: a
// narrower slab means more units.  Within a unit a thread owns one 8-channel
// octet (16 bytes of bf16): oct = width / 8 threads per row, rp = team / oct
// row phases, threads past rp * oct idle.  A thread's octet lies inside one
// group, so its scale, shift, mean and rstd are loop invariants.
//
// Unit -> wave / workgroup map.  A unit of at most 128 octet vectors (two per
// lane; HW = 16 at every slab width) is owned by one wave and four units share
// a 256-thread workgroup; anything larger is owned by the four waves of a
// workgroup.  The last packed workgroup may be partly filled.
//
// Resident forward.  Pass 1 streams the slab from global memory into LDS with
// 16-byte loads (4 rows per thread in flight) and sums x on the way; pass 2
// sums (x - mean)^2 from LDS -- a true two-pass variance, no shift and no
// cancellation for activations with a large mean, and never negative, so there
// is no clamp; pass 3 applies, adds the residual, applies the ReLU (a
// comparison: a NaN stays a NaN) and stores.  A thread reads back from LDS
// exactly the vectors it wrote (consecutive lanes, consecutive 16 bytes: no
// bank conflicts), so the slab needs no barrier; only the reductions do.
// One NaN or Inf in a group gives a NaN mean or variance: the whole group of
// y and its rstd are NaN.
//
// Resident backward.  Pass 1 reads dy, y, x once, keeps dz = dy * (y > 0) and
// x in LDS and forms the per-channel sums of dz and dz * xhat over the rows;
// the group's two means follow from those: mean_group(w dz) = sum_c w_c
// sum_rows dz / (HW cpg), and the same with xhat.  Pass 2 writes dx (and dres)
// from LDS.  If dz and x do not both fit, dz stays (it replaces two reads, dy
// and y) and x is read again.
//
// Streamed variant (template flag, same body): a unit that does not fit takes
// its passes 2 and 3 from global memory instead of LDS.  It keeps the two-pass
// variance -- so it needs neither shifted sums nor pairwise merges -- at the
// price of a third read of x in the forward (from L2 when the unit fits
// there).  It makes any HW correct; it is not tuned.
//
// LDS.  gfx950 has 160 KB per CU and the compiler accepts a workgroup of that
// size (kLdsLimit).  Slabs are dynamic shared memory; above 64 KB the launcher
// asks once per kernel and device (hipFuncSetAttribute, MaxDynamicSharedMemory
// Size) and, if refused, the kernel keeps the 64 KB default and larger units
// are streamed.
//
// Reductions: fixed order, no float atomics.  Within a group: thread (rows in
// order, the 8 channels of a row as a balanced tree) -> wave (wave_sum over
// the lanes of the group, the other lanes contributing exact zeros) -> block
// (LDS, wave order).  Per channel in the backward: thread -> row phases in
// order (LDS); the group's means add the group's channels in index order.
// dgamma / dbeta: every unit writes its slice of a [2, N, C] partial, a second
// kernel adds the N rows in index order.  Nothing depends on which other
// samples are in the batch, and two runs are bitwise equal.
#include <type_traits>

#include "common.h"
#include "groupnorm.h"

namespace p2gn {
using namespace p2;

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / kWave;
constexpr int kInFlight = 4;    // rows per thread in flight
constexpr int kRowBytes = 64;   // least row segment of a slab
constexpr int kMaxOct = 64;     // octets per slab row: one wave covers a row
constexpr int kMaxGroups = kRowBytes / 2 / 8;  // groups per slab: cpg = 8 in bf16
constexpr int kWaveVecs = 128;  // a unit of at most this many octet vectors is owned by one wave
constexpr int kMaxDevices = 64;

struct Geom {
  int HW, C, G, cpg, cs, units, ns;
  float inv_cnt;  // 1 / (HW * cpg)
};

// 8 consecutive channels as they lie in memory: one 16-byte part in bf16, two in fp32.
// LDS slot i of a slab of nv vectors: part p at uint4 index p * nv + i.
template <typename T>
struct Raw8;
template <>
struct Raw8<uint16_t> {
  static constexpr int kParts = 1;
  uint4 a;
  P2_DEVICE void load(const uint16_t* p) { a = *reinterpret_cast<const uint4*>(p); }
  P2_DEVICE void unpack(float (&v)[8]) const { Vec8<uint16_t>::unpack(a, v); }
  P2_DEVICE void pack(const float (&v)[8]) {
    a.x = pack_bf16x2(v[0], v[1]);
    a.y = pack_bf16x2(v[2], v[3]);
    a.z = pack_bf16x2(v[4], v[5]);
    a.w = pack_bf16x2(v[6], v[7]);
  }
  P2_DEVICE void put(uint4* lds, int i, int) const { lds[i] = a; }
  P2_DEVICE void get(const uint4* lds, int i, int) { a = lds[i]; }
};
template <>
struct Raw8<float> {
  static constexpr int kParts = 2;
  uint4 a, b;
  P2_DEVICE void load(const float* p) {
    a = reinterpret_cast<const uint4*>(p)[0];
    b = reinterpret_cast<const uint4*>(p)[1];
  }
  P2_DEVICE void unpack(float (&v)[8]) const {
    v[0] = __uint_as_float(a.x); v[1] = __uint_as_float(a.y); v[2] = __uint_as_float(a.z); v[3] = __uint_as_float(a.w);
    v[4] = __uint_as_float(b.x); v[5] = __uint_as_float(b.y); v[6] = __uint_as_float(b.z); v[7] = __uint_as_float(b.w);
  }
  P2_DEVICE void pack(const float (&v)[8]) {
    a = make_uint4(__float_as_uint(v[0]), __float_as_uint(v[1]), __float_as_uint(v[2]), __float_as_uint(v[3]));
    b = make_uint4(__float_as_uint(v[4]), __float_as_uint(v[5]), __float_as_uint(v[6]), __float_as_uint(v[7]));
  }
  P2_DEVICE void put(uint4* lds, int i, int nv) const {
    lds[i] = a;
    lds[nv + i] = b;
  }
  P2_DEVICE void get(const uint4* lds, int i, int nv) {
    a = lds[i];
    b = lds[nv + i];
  }
};

// Where a thread stands: its team's unit (wave-uniform) and its octet and row phase in it.
struct Coord {
  int team, tt;        // team in the workgroup, thread in the team
  int n, c0, w;        // sample, first channel and width of the slab
  int oct, rp, ph, tg; // octets per row, row phases, this thread's phase and octet
  int gl, ngl, g0;     // this thread's group in the slab, groups in the slab, first group of the slab
  bool live, active;   // the team has a unit; the thread has an octet column in it
};

template <int WPU>
P2_DEVICE Coord coord(const Geom& g) {
  constexpr int TT = kWave * WPU;
  Coord k;
  k.team = threadIdx.x / TT;
  k.tt = threadIdx.x % TT;
  const int unit = __builtin_amdgcn_readfirstlane(int(blockIdx.x) * (kWaves / WPU) + k.team);
  k.live = unit < g.units;
  k.n = k.live ? unit / g.ns : 0;
  k.c0 = k.live ? (unit % g.ns) * g.cs : 0;
  k.w = g.C - k.c0 < g.cs ? g.C - k.c0 : g.cs;
  k.oct = k.w / 8;
  k.rp = TT / k.oct;
  k.ph = k.tt / k.oct;
  k.tg = k.tt % k.oct;
  k.gl = (k.tg * 8) / g.cpg;
  k.ngl = k.w / g.cpg;
  k.g0 = k.c0 / g.cpg;
  k.active = k.live && k.ph < k.rp;
  return k;
}

// The 8 channels of a row as a balanced tree.
P2_DEVICE float sum8(const float (&v)[8]) { return ((v[0] + v[1]) + (v[2] + v[3])) + ((v[4] + v[5]) + (v[6] + v[7])); }

// Sum of v over the active threads of this thread's group: per wave over the
// group's lanes (the others add exact zeros), then the waves in order.  Call
// with every thread of the workgroup (WPU == 4) or of the wave (WPU == 1).
template <int WPU>
P2_DEVICE float group_sum(const Coord& k, float v, float (*wred)[kWaves]) {
  const float in = k.active ? v : 0.f;
  float mine = 0.f;
  for (int q = 0; q < k.ngl; ++q) {
    const float sq = wave_sum(k.gl == q ? in : 0.f);
    if (WPU == 1) {
      if (k.gl == q) mine = sq;
    } else if (threadIdx.x % kWave == 0) {
      wred[q][threadIdx.x / kWave] = sq;
    }
  }
  if (WPU != 1) {
    __syncthreads();
    mine = ((wred[k.gl][0] + wred[k.gl][1]) + wred[k.gl][2]) + wred[k.gl][3];
    __syncthreads();
  }
  return mine;
}

// f(r, v) for each of this thread's rows r, v from the LDS slab or from global
// memory (gp: row 0 of the thread's octet column).  kInFlight rows per
// iteration are loaded unconditionally (a row past HW re-reads the iteration's
// first row and is dropped): a load under a branch waits for itself.
template <typename T, bool FROM_LDS, class F>
P2_DEVICE void for_rows(const Coord& k, int HW, int C, const T* gp, const uint4* slab, int nv, F&& f) {
  for (int r0 = k.ph; r0 < HW; r0 += kInFlight * k.rp) {
    Raw8<T> v[kInFlight];
#pragma unroll
    for (int u = 0; u < kInFlight; ++u) {
      const int r = r0 + u * k.rp, rc = r < HW ? r : r0;
      if (FROM_LDS) v[u].get(slab, rc * k.oct + k.tg, nv);
      else v[u].load(gp + size_t(rc) * C);
    }
#pragma unroll
    for (int u = 0; u < kInFlight; ++u) {
      const int r = r0 + u * k.rp;
      if (r < HW) f(r, v[u]);
    }
  }
}

// ---------------------------------------------------------------------------
// forward
// ---------------------------------------------------------------------------
template <typename T, int WPU, bool RESIDENT>
__global__ __launch_bounds__(kThreads) void gn_fwd_kernel(const T* __restrict__ x, const T* __restrict__ res,
                                                          const float* __restrict__ gamma,
                                                          const float* __restrict__ beta, float eps,
                                                          T* __restrict__ y, float* __restrict__ mean,
                                                          float* __restrict__ rstd, Geom g, int relu) {
  extern __shared__ uint4 dyn[];
  __shared__ float wred[kMaxGroups][kWaves];
  const Coord k = coord<WPU>(g);
  if (WPU == 1 && !k.live) return;  // a packed team runs without barriers
  const int nv = g.HW * (g.cs / 8);
  uint4* slab = dyn + size_t(k.team) * nv * Raw8<T>::kParts;
  const size_t col = (size_t(k.n) * g.HW) * g.C + k.c0 + k.tg * 8;

  float s = 0.f;
  if (k.active)
    for_rows<T, false>(k, g.HW, g.C, x + col, slab, nv, [&](int r, const Raw8<T>& v) {
      if (RESIDENT) v.put(slab, r * k.oct + k.tg, nv);
      float f[8];
      v.unpack(f);
      s += sum8(f);
    });
  const float mu = group_sum<WPU>(k, s, wred) * g.inv_cnt;

  float q = 0.f;
  if (k.active)
    for_rows<T, RESIDENT>(k, g.HW, g.C, x + col, slab, nv, [&](int, const Raw8<T>& v) {
      float f[8];
      v.unpack(f);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        f[j] -= mu;
        f[j] *= f[j];
      }
      q += sum8(f);
    });
  const float rs = rsqrtf(group_sum<WPU>(k, q, wred) * g.inv_cnt + eps);

  if (!k.active) return;
  if (k.ph == 0 && (k.tg * 8) % g.cpg == 0) {
    mean[size_t(k.n) * g.G + k.g0 + k.gl] = mu;
    rstd[size_t(k.n) * g.G + k.g0 + k.gl] = rs;
  }
  float sc[8], sh[8];
  Vec8<float>::load(gamma + k.c0 + k.tg * 8, sc);
  Vec8<float>::load(beta + k.c0 + k.tg * 8, sh);
#pragma unroll
  for (int j = 0; j < 8; ++j) sc[j] *= rs;
  for_rows<T, RESIDENT>(k, g.HW, g.C, x + col, slab, nv, [&](int r, const Raw8<T>& v) {
    float f[8];
    v.unpack(f);
#pragma unroll
    for (int j = 0; j < 8; ++j) f[j] = fmaf(f[j] - mu, sc[j], sh[j]);
    const size_t e = col + size_t(r) * g.C;
    if (res) {
      float rr[8];
      Vec8<T>::load(res + e, rr);
#pragma unroll
      for (int j = 0; j < 8; ++j) f[j] += rr[j];
    }
    if (relu) {
#pragma unroll
      for (int j = 0; j < 8; ++j) f[j] = f[j] < 0.f ? 0.f : f[j];  // not fmaxf: a NaN stays a NaN
    }
    Vec8<T>::store(y + e, f);
  });
}

// ---------------------------------------------------------------------------
// backward.  KEEP: 2 dz and x stay in LDS, 1 dz only, 0 neither (streamed).
// Dynamic LDS: [teams][2][cs] floats (w_c times the channel's two sums), then
// [teams][KEEP] slabs.
// ---------------------------------------------------------------------------
template <typename T>
P2_DEVICE void masked(const Raw8<T>& dyv, const Raw8<T>& yv, bool relu, float (&dz)[8]) {
  dyv.unpack(dz);
  if (relu) {
    float yf[8];
    yv.unpack(yf);
#pragma unroll
    for (int j = 0; j < 8; ++j) dz[j] = yf[j] > 0.f ? dz[j] : 0.f;
  }
}

template <typename T, int WPU, int KEEP>
__global__ __launch_bounds__(kThreads) void gn_bwd_kernel(const T* __restrict__ dy, const T* __restrict__ y,
                                                          const T* __restrict__ x, const float* __restrict__ gamma,
                                                          const float* __restrict__ mean,
                                                          const float* __restrict__ rstd, T* __restrict__ dx,
                                                          T* __restrict__ dres, float* __restrict__ part, Geom g,
                                                          int N, int relu) {
  extern __shared__ uint4 dyn[];
  __shared__ float red[2][kThreads * 8];
  constexpr int TT = kWave * WPU, UPW = kWaves / WPU;
  const Coord k = coord<WPU>(g);
  const int nv = g.HW * (g.cs / 8);
  float* csum = reinterpret_cast<float*>(dyn) + k.team * 2 * g.cs;
  uint4* slab_dz = dyn + (UPW * 2 * g.cs) / 4 + size_t(k.team) * KEEP * nv * Raw8<T>::kParts;
  uint4* slab_x = slab_dz + size_t(nv) * Raw8<T>::kParts;  // KEEP == 2 only
  float* red0 = red[0] + k.team * TT * 8;
  float* red1 = red[1] + k.team * TT * 8;
  const size_t col = (size_t(k.n) * g.HW) * g.C + k.c0 + k.tg * 8;
  const float mu = k.live ? mean[size_t(k.n) * g.G + k.g0 + k.gl] : 0.f;
  const float rs = k.live ? rstd[size_t(k.n) * g.G + k.g0 + k.gl] : 0.f;

  // pass 1: per-thread channel sums of dz and dz * xhat over the thread's rows
  float s1[8], s2[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) s1[j] = s2[j] = 0.f;
  if (k.active) {
    for (int r0 = k.ph; r0 < g.HW; r0 += kInFlight * k.rp) {
      Raw8<T> gv[kInFlight], yv[kInFlight], xv[kInFlight];
#pragma unroll
      for (int u = 0; u < kInFlight; ++u) {
        const int r = r0 + u * k.rp;
        const size_t e = col + size_t(r < g.HW ? r : r0) * g.C;
        gv[u].load(dy + e);
        xv[u].load(x + e);
        if (relu) yv[u].load(y + e);
        else yv[u] = gv[u];
      }
#pragma unroll
      for (int u = 0; u < kInFlight; ++u) {
        const int r = r0 + u * k.rp;
        if (r >= g.HW) continue;
        float dz[8], xf[8];
        masked(gv[u], yv[u], relu, dz);
        xv[u].unpack(xf);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          s1[j] += dz[j];
          s2[j] = fmaf(dz[j], (xf[j] - mu) * rs, s2[j]);
        }
        if (KEEP >= 1) {
          Raw8<T> z;
          z.pack(dz);  // dy or 0: exact in the activation type
          z.put(slab_dz, r * k.oct + k.tg, nv);
        }
        if (KEEP == 2) xv[u].put(slab_x, r * k.oct + k.tg, nv);
      }
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      red0[k.ph * k.w + k.tg * 8 + j] = s1[j];
      red1[k.ph * k.w + k.tg * 8 + j] = s2[j];
    }
  }
  __syncthreads();
  // the row phases in order: this sample's row of the dbeta / dgamma partials, and w_c times each
  if (k.live)
    for (int i = k.tt; i < k.w; i += TT) {
      float a = 0.f, b = 0.f;
      for (int p = 0; p < k.rp; ++p) {
        a += red0[p * k.w + i];
        b += red1[p * k.w + i];
      }
      const int c = k.c0 + i;
      part[size_t(k.n) * g.C + c] = a;
      part[(size_t(N) + k.n) * g.C + c] = b;
      const float wc = gamma[c];
      csum[i] = wc * a;
      csum[g.cs + i] = wc * b;
    }
  __syncthreads();
  if (!k.active) return;
  // the group's means of w dz and w dz xhat: its channels in index order
  float ma = 0.f, mb = 0.f;
  for (int c = k.gl * g.cpg; c < (k.gl + 1) * g.cpg; ++c) {
    ma += csum[c];
    mb += csum[g.cs + c];
  }
  ma *= g.inv_cnt;
  mb *= g.inv_cnt;
  float wv[8];
  Vec8<float>::load(gamma + k.c0 + k.tg * 8, wv);

  // pass 2: dx = rstd (w dz - ma - xhat mb), dres = dz
  for (int r0 = k.ph; r0 < g.HW; r0 += kInFlight * k.rp) {
    Raw8<T> gv[kInFlight], yv[kInFlight], xv[kInFlight];
#pragma unroll
    for (int u = 0; u < kInFlight; ++u) {
      const int r = r0 + u * k.rp, rc = r < g.HW ? r : r0;
      const size_t e = col + size_t(rc) * g.C;
      if (KEEP >= 1) {
        gv[u].get(slab_dz, rc * k.oct + k.tg, nv);
      } else {
        gv[u].load(dy + e);
        if (relu) yv[u].load(y + e);
        else yv[u] = gv[u];
      }
      if (KEEP == 2) xv[u].get(slab_x, rc * k.oct + k.tg, nv);
      else xv[u].load(x + e);
    }
#pragma unroll
    for (int u = 0; u < kInFlight; ++u) {
      const int r = r0 + u * k.rp;
      if (r >= g.HW) continue;
      float dz[8], xf[8], o[8];
      if (KEEP >= 1) gv[u].unpack(dz);
      else masked(gv[u], yv[u], relu, dz);
      xv[u].unpack(xf);
#pragma unroll
      for (int j = 0; j < 8; ++j) o[j] = rs * ((wv[j] * dz[j] - ma) - (xf[j] - mu) * rs * mb);
      const size_t e = col + size_t(r) * g.C;
      Vec8<T>::store(dx + e, o);
      if (dres) Vec8<T>::store(dres + e, dz);
    }
  }
}

// dbeta / dgamma: the N rows of the [2, N, C] partials in index order
__global__ __launch_bounds__(kThreads) void gn_param_reduce_kernel(const float* __restrict__ part,
                                                                   float* __restrict__ dw, float* __restrict__ db,
                                                                   int N, int C) {
  const int c = blockIdx.x * kThreads + threadIdx.x;
  if (c >= C) return;
  float a = 0.f, b = 0.f;
  for (int n = 0; n < N; ++n) {
    a += part[size_t(n) * C + c];
    b += part[(size_t(N) + n) * C + c];
  }
  db[c] = a;
  dw[c] = b;
}

// ---------------------------------------------------------------------------
// plans and launchers
// ---------------------------------------------------------------------------
GnPlan gn_plan(bool bf16, int N, int HW, int C, int G) {
  GnPlan p{};
  if (N < 1 || HW < 1 || C < 8 || G < 1 || C % G || (C / G) % 8) return p;
  const int elt = bf16 ? 2 : 4, cpg = C / G, target = kRowBytes / elt;
  int cs = cpg * ((target + cpg - 1) / cpg);
  if (cs > C) cs = C;
  if (cs / 8 > kMaxOct) return p;
  p.cs = cs;
  p.ns = (C + cs - 1) / cs;
  p.wpu = int64_t(HW) * (cs / 8) <= kWaveVecs ? 1 : kWaves;
  p.units = N * p.ns;
  p.blocks = (p.units + kWaves / p.wpu - 1) / (kWaves / p.wpu);
  p.unit_bytes = int64_t(HW) * cs * elt;
  return p;
}

static Geom geom(const GnPlan& p, int HW, int C, int G) {
  Geom g{};
  g.HW = HW;
  g.C = C;
  g.G = G;
  g.cpg = C / G;
  g.cs = p.cs;
  g.units = p.units;
  g.ns = p.ns;
  g.inv_cnt = 1.f / (float(HW) * float(C / G));
  return g;
}

// Dynamic LDS a kernel may be launched with on the current device, and the
// per-workgroup total that is: asked for once per kernel and device.
struct Budget {
  int dyn, total;
};
template <class K>
static Budget lds_budget(K kernel, Budget (&cache)[kMaxDevices]) {
  int dev = 0;
  P2_CHECK(hipGetDevice(&dev));
  if (dev < 0 || dev >= kMaxDevices) throw std::runtime_error("groupnorm: device index out of range");
  if (cache[dev].total == 0) {
    hipFuncAttributes at{};
    P2_CHECK(hipFuncGetAttributes(&at, reinterpret_cast<const void*>(kernel)));
    const int stat = int(at.sharedSizeBytes);
    int total = kLdsLimit;
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                            kLdsLimit - stat) != hipSuccess) {
      (void)hipGetLastError();  // refused: the default holds, larger units are streamed
      total = kLdsDefault;
    }
    cache[dev] = Budget{total - stat, total};
  }
  return cache[dev];
}
template <typename T, int WPU>
static Budget fwd_budget() {
  static Budget cache[kMaxDevices];
  return lds_budget(gn_fwd_kernel<T, WPU, true>, cache);
}
template <typename T, int WPU, int KEEP>
static Budget bwd_budget() {
  static Budget cache[kMaxDevices];
  return lds_budget(gn_bwd_kernel<T, WPU, KEEP>, cache);
}

// dynamic LDS of the backward with `keep` slabs per unit
static int64_t bwd_dyn(const GnPlan& p, int keep) {
  const int upw = kWaves / p.wpu;
  return int64_t(upw) * 2 * p.cs * 4 + int64_t(upw) * keep * p.unit_bytes;
}

template <typename T, int WPU>
static GnResidency residency(const GnPlan& p) {
  GnResidency r{};
  const Budget f = fwd_budget<T, WPU>();
  r.lds = f.total;
  r.fwd_resident = int64_t(kWaves / WPU) * p.unit_bytes <= f.dyn;
  r.bwd_keep = bwd_dyn(p, 2) <= bwd_budget<T, WPU, 2>().dyn ? 2 : (bwd_dyn(p, 1) <= bwd_budget<T, WPU, 1>().dyn ? 1 : 0);
  return r;
}

// fn receives (element value, std::integral_constant<int, WPU>)
template <class Fn>
static void with_kind(bool bf16, int wpu, Fn&& fn) {
  auto w = [&](auto t) { wpu == 1 ? fn(t, std::integral_constant<int, 1>{}) : fn(t, std::integral_constant<int, kWaves>{}); };
  bf16 ? w(uint16_t{}) : w(float{});
}

static GnPlan checked_plan(bool bf16, int N, int HW, int C, int G) {
  const GnPlan p = gn_plan(bf16, N, HW, C, G);
  if (p.wpu == 0) throw std::runtime_error("groupnorm: unsupported shape (C / G must be a multiple of 8, at most 512)");
  return p;
}

GnResidency gn_residency(bool bf16, int N, int HW, int C, int G) {
  const GnPlan p = checked_plan(bf16, N, HW, C, G);
  GnResidency r{};
  with_kind(bf16, p.wpu, [&](auto t, auto W) { r = residency<decltype(t), decltype(W)::value>(p); });
  return r;
}

void gn_fwd(bool bf16, const void* xv, const void* resv, const float* w, const float* b, float eps, void* yv,
            float* mean, float* rstd, int N, int HW, int C, int G, bool relu, hipStream_t s) {
  const GnPlan p = checked_plan(bf16, N, HW, C, G);
  const Geom g = geom(p, HW, C, G);
  with_kind(bf16, p.wpu, [&](auto t, auto W) {
    using T = decltype(t);
    constexpr int WPU = decltype(W)::value;
    const T *x = static_cast<const T*>(xv), *res = static_cast<const T*>(resv);
    T* y = static_cast<T*>(yv);
    if (residency<T, WPU>(p).fwd_resident)
      hipLaunchKernelGGL((gn_fwd_kernel<T, WPU, true>), dim3(p.blocks), dim3(kThreads),
                         size_t(kWaves / WPU) * p.unit_bytes, s, x, res, w, b, eps, y, mean, rstd, g, int(relu));
    else
      hipLaunchKernelGGL((gn_fwd_kernel<T, WPU, false>), dim3(p.blocks), dim3(kThreads), 0, s, x, res, w, b, eps, y,
                         mean, rstd, g, int(relu));
  });
  P2_CHECK(hipGetLastError());
}

void gn_bwd(bool bf16, const void* dyv, const void* yv, const void* xv, const float* w, const float* mean,
            const float* rstd, void* dxv, void* dresv, float* dw, float* db, float* part, int N, int HW, int C, int G,
            bool relu, hipStream_t s) {
  const GnPlan p = checked_plan(bf16, N, HW, C, G);
  const Geom g = geom(p, HW, C, G);
  with_kind(bf16, p.wpu, [&](auto t, auto W) {
    using T = decltype(t);
    constexpr int WPU = decltype(W)::value;
    const T *dy = static_cast<const T*>(dyv), *y = static_cast<const T*>(yv), *x = static_cast<const T*>(xv);
    T *dx = static_cast<T*>(dxv), *dres = static_cast<T*>(dresv);
    const int keep = residency<T, WPU>(p).bwd_keep;
    const dim3 grid(p.blocks), block(kThreads);
    if (keep == 2)
      hipLaunchKernelGGL((gn_bwd_kernel<T, WPU, 2>), grid, block, size_t(bwd_dyn(p, 2)), s, dy, y, x, w, mean, rstd, dx,
                         dres, part, g, N, int(relu));
    else if (keep == 1)
      hipLaunchKernelGGL((gn_bwd_kernel<T, WPU, 1>), grid, block, size_t(bwd_dyn(p, 1)), s, dy, y, x, w, mean, rstd, dx,
                         dres, part, g, N, int(relu));
    else
      hipLaunchKernelGGL((gn_bwd_kernel<T, WPU, 0>), grid, block, size_t(bwd_dyn(p, 0)), s, dy, y, x, w, mean, rstd, dx,
                         dres, part, g, N, int(relu));
  });
  hipLaunchKernelGGL(gn_param_reduce_kernel, dim3((C + kThreads - 1) / kThreads), dim3(kThreads), 0, s, part, dw, db, N,
                     C);
  P2_CHECK(hipGetLastError());
}

}  // namespace p2gn
