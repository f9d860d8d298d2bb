// tiresias_amd — fused optimizer steps over a job's *flat* parameter arena.
//
// Every job keeps its parameters in one contiguous fp32 master buffer with a
// bf16 shadow (the compute copy the kernels read), one fp32 gradient buffer
// (what the bucketed RCCL all-reduce reduces in place) and its optimizer
// state. One launch updates the whole model: read grad + master + state,
// write master + state + bf16 shadow, and zero the gradient for the next
// iteration (saves the separate memset pass). 16 B per lane.
//
// ``guard`` (nullable): a device word that, when non-zero, turns the step
// into a gradient reset only -- no master / state / shadow update. The
// trainer of a GNMT job passes ITS OWN persistent-LSTM timeout word
// (models/gnmt.py GNMT.err[0], bumped by a timed-out grid barrier of that
// job only): a step whose recurrence read h / dG that had not arrived must
// not reach the weights. lstm_guard_step then moves the word into the job's
// skipped-step count (err[1]), which the worker subtracts from the round's
// progress and uses to switch the job to the per-step recurrence.
//
// ``clip`` (nullable): the 16-B device record grad_clip_finalize writes from
// the step's global gradient norm (grad_sumsq). clip[0] is the clip scale,
// folded into gscale once per thread; a negative clip[0] (non-finite norm)
// takes the guard path. The scale never visits the host.
#include <cmath>
#include <cstdlib>

#include "tam/common.h"
#include "tam/kernels.h"
#include "tam/philox.h"

namespace tam {

__global__ void __launch_bounds__(256) sgd_kernel(float* __restrict__ w, float* __restrict__ g,
                                                   float* __restrict__ mom,
                                                   bf16_t* __restrict__ wb, long n4, float lr,
                                                   float momentum, float wd0, float gscale,
                                                   int nesterov, int zero_grad, const unsigned* guard,
                                                   long zero_from4, long wd_until4, const float* clip) {
  if ((guard != nullptr && *guard != 0u) || (clip != nullptr && clip[0] < 0.f)) {
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n4; i += (long)gridDim.x * blockDim.x)
      if (i >= zero_from4) ((float4*)g)[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    return;
  }
  if (clip != nullptr) gscale *= clip[0];
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n4;
       i += (long)gridDim.x * blockDim.x) {
    float4 wv = ((float4*)w)[i];
    float4 gv = ((float4*)g)[i];
    float4 mv = ((float4*)mom)[i];
    float* wp = (float*)&wv; float* gp = (float*)&gv; float* mp = (float*)&mv;
    const float wd = i < wd_until4 ? wd0 : 0.f;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      float d = __builtin_fmaf(wd, wp[k], gp[k] * gscale);
      mp[k] = __builtin_fmaf(momentum, mp[k], d);
      d = nesterov ? __builtin_fmaf(momentum, mp[k], d) : mp[k];
      wp[k] = __builtin_fmaf(-lr, d, wp[k]);
    }
    ((float4*)w)[i] = wv;
    ((float4*)mom)[i] = mv;
    if (zero_grad && i >= zero_from4) ((float4*)g)[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    ((uint2*)wb)[i] = make_uint2(pack_bf2(wp[0], wp[1]), pack_bf2(wp[2], wp[3]));
  }
}

__global__ void __launch_bounds__(256) adam_kernel(float* __restrict__ w, float* __restrict__ g,
                                                    float* __restrict__ m, float* __restrict__ v,
                                                    bf16_t* __restrict__ wb, long n4, float lr,
                                                    float b1, float b2, float eps, float wd0,
                                                    float bc1, float bc2, float gscale,
                                                    int zero_grad, const unsigned* guard, long zero_from4,
                                                    long wd_until4, const float* clip) {
  if ((guard != nullptr && *guard != 0u) || (clip != nullptr && clip[0] < 0.f)) {
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n4; i += (long)gridDim.x * blockDim.x)
      if (i >= zero_from4) ((float4*)g)[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    return;
  }
  if (clip != nullptr) gscale *= clip[0];
  const float ib1 = 1.f / bc1, ib2 = 1.f / bc2;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n4;
       i += (long)gridDim.x * blockDim.x) {
    float4 wv = ((float4*)w)[i], gv = ((float4*)g)[i], mv = ((float4*)m)[i], vv = ((float4*)v)[i];
    float* wp = (float*)&wv; float* gp = (float*)&gv; float* mp = (float*)&mv; float* vp = (float*)&vv;
    const float wd = i < wd_until4 ? wd0 : 0.f;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float gr = gp[k] * gscale;
      mp[k] = __builtin_fmaf(b1, mp[k], (1.f - b1) * gr);
      vp[k] = __builtin_fmaf(b2, vp[k], (1.f - b2) * gr * gr);
      const float mh = mp[k] * ib1, vh = vp[k] * ib2;
      const float u = __builtin_fmaf(wd, wp[k], mh / (sqrtf(vh) + eps));   // decoupled (AdamW)
      wp[k] = __builtin_fmaf(-lr, u, wp[k]);
    }
    ((float4*)w)[i] = wv; ((float4*)m)[i] = mv; ((float4*)v)[i] = vv;
    if (zero_grad && i >= zero_from4) ((float4*)g)[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    ((uint2*)wb)[i] = make_uint2(pack_bf2(wp[0], wp[1]), pack_bf2(wp[2], wp[3]));
  }
}

// Every form spells its arithmetic as explicit FMAs: the element update is
// then one fixed rounding sequence whichever path (kernel, unrolled group or
// tail) covers the element, so a step is bitwise independent of the grid,
// the variant and how an arena is split into launches (contraction was left
// to the compiler before and differed between the unrolled and tail bodies).
// Streaming variants (optim_variant): U float4 groups per thread per
// iteration, all loads issued before any math (U x 4 x 16 B in flight per
// lane), NT: non-temporal loads / stores (every byte is touched once per
// step; keeps the step from evicting the next forward's L2 / MALL working
// set). Tail groups (n4 % U) are handled with the same body at U = 1.
typedef unsigned u32x2_t __attribute__((ext_vector_type(2)));
template <int U, bool NT>
__device__ __forceinline__ float4 ld4(const float* p, long i) {
  if constexpr (NT) {
    const f32x4_t r = __builtin_nontemporal_load((const f32x4_t*)p + i);
    return make_float4(r[0], r[1], r[2], r[3]);
  } else {
    return ((const float4*)p)[i];
  }
}
template <bool NT>
__device__ __forceinline__ void st4(float* p, long i, float4 v) {
  if constexpr (NT) __builtin_nontemporal_store(f32x4_t{v.x, v.y, v.z, v.w}, (f32x4_t*)p + i);
  else ((float4*)p)[i] = v;
}
template <bool NT>
__device__ __forceinline__ void st2(bf16_t* p, long i, uint2 v) {
  if constexpr (NT) __builtin_nontemporal_store(u32x2_t{v.x, v.y}, (u32x2_t*)p + i);
  else ((uint2*)p)[i] = v;
}

template <int U, bool NT>
__global__ void __launch_bounds__(256) adam_stream_kernel(float* __restrict__ w, float* __restrict__ g,
                                                           float* __restrict__ m, float* __restrict__ v,
                                                           bf16_t* __restrict__ wb, long n4, float lr, float b1,
                                                           float b2, float eps, float wd0, float bc1, float bc2,
                                                           float gscale, int zero_grad, const unsigned* guard,
                                                           long zero_from4, long wd_until4, const float* clip) {
  const long stride = (long)gridDim.x * blockDim.x;
  if ((guard != nullptr && *guard != 0u) || (clip != nullptr && clip[0] < 0.f)) {
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n4; i += stride)
      if (i >= zero_from4) st4<NT>(g, i, make_float4(0.f, 0.f, 0.f, 0.f));
    return;
  }
  if (clip != nullptr) gscale *= clip[0];
  const float ib1 = 1.f / bc1, ib2 = 1.f / bc2;
  auto body = [&](long i, float4 wv, float4 gv, float4 mv, float4 vv) {
    float* wp = (float*)&wv; float* gp = (float*)&gv; float* mp = (float*)&mv; float* vp = (float*)&vv;
    const float wd = i < wd_until4 ? wd0 : 0.f;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float gr = gp[k] * gscale;
      mp[k] = __builtin_fmaf(b1, mp[k], (1.f - b1) * gr);
      vp[k] = __builtin_fmaf(b2, vp[k], (1.f - b2) * gr * gr);
      const float mh = mp[k] * ib1, vh = vp[k] * ib2;
      const float u = __builtin_fmaf(wd, wp[k], mh / (sqrtf(vh) + eps));   // decoupled (AdamW)
      wp[k] = __builtin_fmaf(-lr, u, wp[k]);
    }
    st4<NT>(w, i, wv); st4<NT>(m, i, mv); st4<NT>(v, i, vv);
    if (zero_grad && i >= zero_from4) st4<NT>(g, i, make_float4(0.f, 0.f, 0.f, 0.f));
    st2<NT>(wb, i, make_uint2(pack_bf2(wp[0], wp[1]), pack_bf2(wp[2], wp[3])));
  };
  const long t = blockIdx.x * (long)blockDim.x + threadIdx.x;
  const long full = n4 / (U * stride) * (U * stride);
  for (long base = t; base < full; base += U * stride) {
    float4 wv[U], gv[U], mv[U], vv[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const long i = base + u * stride;
      wv[u] = ld4<U, NT>(w, i); gv[u] = ld4<U, NT>(g, i); mv[u] = ld4<U, NT>(m, i); vv[u] = ld4<U, NT>(v, i);
    }
#pragma unroll
    for (int u = 0; u < U; ++u) body(base + u * stride, wv[u], gv[u], mv[u], vv[u]);
  }
  for (long i = full + t; i < n4; i += stride)
    body(i, ld4<1, NT>(w, i), ld4<1, NT>(g, i), ld4<1, NT>(m, i), ld4<1, NT>(v, i));
}

template <int U, bool NT>
__global__ void __launch_bounds__(256) sgd_stream_kernel(float* __restrict__ w, float* __restrict__ g,
                                                          float* __restrict__ mom, bf16_t* __restrict__ wb, long n4,
                                                          float lr, float momentum, float wd0, float gscale,
                                                          int nesterov, int zero_grad, const unsigned* guard,
                                                          long zero_from4, long wd_until4, const float* clip) {
  const long stride = (long)gridDim.x * blockDim.x;
  if ((guard != nullptr && *guard != 0u) || (clip != nullptr && clip[0] < 0.f)) {
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n4; i += stride)
      if (i >= zero_from4) st4<NT>(g, i, make_float4(0.f, 0.f, 0.f, 0.f));
    return;
  }
  if (clip != nullptr) gscale *= clip[0];
  auto body = [&](long i, float4 wv, float4 gv, float4 mv) {
    float* wp = (float*)&wv; float* gp = (float*)&gv; float* mp = (float*)&mv;
    const float wd = i < wd_until4 ? wd0 : 0.f;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      float d = __builtin_fmaf(wd, wp[k], gp[k] * gscale);
      mp[k] = __builtin_fmaf(momentum, mp[k], d);
      d = nesterov ? __builtin_fmaf(momentum, mp[k], d) : mp[k];
      wp[k] = __builtin_fmaf(-lr, d, wp[k]);
    }
    st4<NT>(w, i, wv); st4<NT>(mom, i, mv);
    if (zero_grad && i >= zero_from4) st4<NT>(g, i, make_float4(0.f, 0.f, 0.f, 0.f));
    st2<NT>(wb, i, make_uint2(pack_bf2(wp[0], wp[1]), pack_bf2(wp[2], wp[3])));
  };
  const long t = blockIdx.x * (long)blockDim.x + threadIdx.x;
  const long full = n4 / (U * stride) * (U * stride);
  for (long base = t; base < full; base += U * stride) {
    float4 wv[U], gv[U], mv[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const long i = base + u * stride;
      wv[u] = ld4<U, NT>(w, i); gv[u] = ld4<U, NT>(g, i); mv[u] = ld4<U, NT>(mom, i);
    }
#pragma unroll
    for (int u = 0; u < U; ++u) body(base + u * stride, wv[u], gv[u], mv[u]);
  }
  for (long i = full + t; i < n4; i += stride) body(i, ld4<1, NT>(w, i), ld4<1, NT>(g, i), ld4<1, NT>(mom, i));
}

// ------------------------------------------------------ bf16 optimizer state
// Siblings of the two streaming kernels above for a job that keeps its
// moments in bf16 (Trainer opt_dtype="bf16"): m / v / mom are bf16, 8 B per
// float4 group, widened by a shift; the element update is the same explicit
// FMA sequence on fp32 values, and the weight and the shadow come from the
// fresh UNROUNDED moments, so for state that is exact in bf16 a step writes
// the weights the fp32-state kernel writes. Only the stored moments are
// rounded, stochastically (tam/philox.h "Optimizer-state rounding
// contract"): one Philox call per group, keyed by the job's seed and the
// optimizer step, indexed by the group's position in the WHOLE arena (q0 =
// arena index of this launch's element 0, / 4), so a launch over [lo, hi)
// draws what one launch over the arena draws. Nothing random is stored. The
// draws of an unrolled pass are computed after its loads are issued and
// depend on none of them: the integer work runs under the load latency.
// The guard / non-finite-clip path writes no state and draws nothing.
template <bool NT>
__device__ __forceinline__ uint2 ld2(const bf16_t* p, long i) {
  if constexpr (NT) {
    const u32x2_t r = __builtin_nontemporal_load((const u32x2_t*)p + i);
    return make_uint2(r[0], r[1]);
  } else {
    return ((const uint2*)p)[i];
  }
}
__device__ __forceinline__ float4 widen4(uint2 s) {
  return make_float4(__uint_as_float(s.x << 16), __uint_as_float(s.x & 0xffff0000u), __uint_as_float(s.y << 16),
                     __uint_as_float(s.y & 0xffff0000u));
}
struct Draw4 {
  uint32_t r[4];
};
__device__ __forceinline__ Draw4 draw4(long q, uint32_t seed, uint32_t step) {
  Draw4 d;
  opt_state_draw4((uint64_t)q, seed, step, d.r);
  return d;
}
// HI = false: the low halves of the draw words (first moment / momentum),
// true: the high halves (second moment)
template <bool HI>
__device__ __forceinline__ uint2 round4(float4 f, const Draw4& d) {
  const float* fp = (const float*)&f;
  uint32_t o[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) o[j] = sr_bf16(__float_as_uint(fp[j]), HI ? d.r[j] >> 16 : d.r[j] & 0xffffu);
  return make_uint2(o[0] | (o[1] << 16), o[2] | (o[3] << 16));
}

template <int U, bool NT>
__global__ void __launch_bounds__(256) adam_stream_bf16s_kernel(
    float* __restrict__ w, float* __restrict__ g, bf16_t* __restrict__ m, bf16_t* __restrict__ v,
    bf16_t* __restrict__ wb, long n4, float lr, float b1, float b2, float eps, float wd0, float bc1, float bc2,
    float gscale, int zero_grad, const unsigned* guard, long zero_from4, long wd_until4, const float* clip,
    uint32_t seed, uint32_t step, long q0) {
  const long stride = (long)gridDim.x * blockDim.x;
  if ((guard != nullptr && *guard != 0u) || (clip != nullptr && clip[0] < 0.f)) {
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n4; i += stride)
      if (i >= zero_from4) st4<NT>(g, i, make_float4(0.f, 0.f, 0.f, 0.f));
    return;
  }
  if (clip != nullptr) gscale *= clip[0];
  const float ib1 = 1.f / bc1, ib2 = 1.f / bc2;
  auto body = [&](long i, float4 wv, float4 gv, uint2 ms, uint2 vs, const Draw4& d) {
    float4 mv = widen4(ms), vv = widen4(vs);
    float* wp = (float*)&wv; float* gp = (float*)&gv; float* mp = (float*)&mv; float* vp = (float*)&vv;
    const float wd = i < wd_until4 ? wd0 : 0.f;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float gr = gp[k] * gscale;
      mp[k] = __builtin_fmaf(b1, mp[k], (1.f - b1) * gr);
      vp[k] = __builtin_fmaf(b2, vp[k], (1.f - b2) * gr * gr);
      const float mh = mp[k] * ib1, vh = vp[k] * ib2;
      const float u = __builtin_fmaf(wd, wp[k], mh / (sqrtf(vh) + eps));   // decoupled (AdamW)
      wp[k] = __builtin_fmaf(-lr, u, wp[k]);
    }
    st4<NT>(w, i, wv); st2<NT>(m, i, round4<false>(mv, d)); st2<NT>(v, i, round4<true>(vv, d));
    if (zero_grad && i >= zero_from4) st4<NT>(g, i, make_float4(0.f, 0.f, 0.f, 0.f));
    st2<NT>(wb, i, make_uint2(pack_bf2(wp[0], wp[1]), pack_bf2(wp[2], wp[3])));
  };
  const long t = blockIdx.x * (long)blockDim.x + threadIdx.x;
  const long full = n4 / (U * stride) * (U * stride);
  for (long base = t; base < full; base += U * stride) {
    float4 wv[U], gv[U];
    uint2 ms[U], vs[U];
    Draw4 d[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const long i = base + u * stride;
      wv[u] = ld4<U, NT>(w, i); gv[u] = ld4<U, NT>(g, i); ms[u] = ld2<NT>(m, i); vs[u] = ld2<NT>(v, i);
    }
#pragma unroll
    for (int u = 0; u < U; ++u) d[u] = draw4(q0 + base + u * stride, seed, step);
#pragma unroll
    for (int u = 0; u < U; ++u) body(base + u * stride, wv[u], gv[u], ms[u], vs[u], d[u]);
  }
  for (long i = full + t; i < n4; i += stride) {
    const float4 wv = ld4<1, NT>(w, i), gv = ld4<1, NT>(g, i);
    const uint2 ms = ld2<NT>(m, i), vs = ld2<NT>(v, i);
    body(i, wv, gv, ms, vs, draw4(q0 + i, seed, step));
  }
}

template <int U, bool NT>
__global__ void __launch_bounds__(256) sgd_stream_bf16s_kernel(
    float* __restrict__ w, float* __restrict__ g, bf16_t* __restrict__ mom, bf16_t* __restrict__ wb, long n4,
    float lr, float momentum, float wd0, float gscale, int nesterov, int zero_grad, const unsigned* guard,
    long zero_from4, long wd_until4, const float* clip, uint32_t seed, uint32_t step, long q0) {
  const long stride = (long)gridDim.x * blockDim.x;
  if ((guard != nullptr && *guard != 0u) || (clip != nullptr && clip[0] < 0.f)) {
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n4; i += stride)
      if (i >= zero_from4) st4<NT>(g, i, make_float4(0.f, 0.f, 0.f, 0.f));
    return;
  }
  if (clip != nullptr) gscale *= clip[0];
  auto body = [&](long i, float4 wv, float4 gv, uint2 ms, const Draw4& dr) {
    float4 mv = widen4(ms);
    float* wp = (float*)&wv; float* gp = (float*)&gv; float* mp = (float*)&mv;
    const float wd = i < wd_until4 ? wd0 : 0.f;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      float d = __builtin_fmaf(wd, wp[k], gp[k] * gscale);
      mp[k] = __builtin_fmaf(momentum, mp[k], d);
      d = nesterov ? __builtin_fmaf(momentum, mp[k], d) : mp[k];
      wp[k] = __builtin_fmaf(-lr, d, wp[k]);
    }
    st4<NT>(w, i, wv); st2<NT>(mom, i, round4<false>(mv, dr));
    if (zero_grad && i >= zero_from4) st4<NT>(g, i, make_float4(0.f, 0.f, 0.f, 0.f));
    st2<NT>(wb, i, make_uint2(pack_bf2(wp[0], wp[1]), pack_bf2(wp[2], wp[3])));
  };
  const long t = blockIdx.x * (long)blockDim.x + threadIdx.x;
  const long full = n4 / (U * stride) * (U * stride);
  for (long base = t; base < full; base += U * stride) {
    float4 wv[U], gv[U];
    uint2 ms[U];
    Draw4 d[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const long i = base + u * stride;
      wv[u] = ld4<U, NT>(w, i); gv[u] = ld4<U, NT>(g, i); ms[u] = ld2<NT>(mom, i);
    }
#pragma unroll
    for (int u = 0; u < U; ++u) d[u] = draw4(q0 + base + u * stride, seed, step);
#pragma unroll
    for (int u = 0; u < U; ++u) body(base + u * stride, wv[u], gv[u], ms[u], d[u]);
  }
  for (long i = full + t; i < n4; i += stride) {
    const float4 wv = ld4<1, NT>(w, i), gv = ld4<1, NT>(g, i);
    const uint2 ms = ld2<NT>(mom, i);
    body(i, wv, gv, ms, draw4(q0 + i, seed, step));
  }
}

// 0: adam_kernel / sgd_kernel (one group per thread per iteration); 3: U=4
// + NT (1 / 2, U=2 with / without NT, measured between the two and were
// dropped). -1 (default): optim_pick.
static int g_optim_variant = [] {
  const char* e = getenv("TAM_OPTIM_VARIANT");   // A/B runs
  return e ? atoi(e) : -1;
}();
TAM_KNOB(g_optim_variant)
void optim_variant(int v) { g_optim_variant = v; }
// auto: the streaming form for every arena, launched at ONE block per CU
// (ogrid). Rounds 4-5 ran it on a 4096-block grid, where its isolated gain
// on Adam did not survive inside the graph step; at one block per CU each
// CU keeps 4 waves x 16 float4 loads in flight on a single arena stream
// (fewer open DRAM pages than 16 blocks interleaving), and it wins both
// isolated and in the step. Same box (tools/bench_optim.py,
// profiles/r6/optim_grid.md):
//   isolated, us (v0 @4096 -> v3 @256): GNMT Adam 1593 -> 1393,
//   Transformer Adam 382 -> 327, VGG-16 SGD 795 -> 627, ResNet-50 SGD 120 -> 108;
//   graph step, ms: GNMT 9.73-9.75 -> 9.41-9.48, Transformer 4.95-4.96 ->
//   4.90-4.91, VGG-16 6.57-6.60 -> 6.47, ResNet-50 equal.
static int optim_pick(long, bool) {
  return g_optim_variant >= 0 ? g_optim_variant : 3;
}

// grid cap of the optimizer launches (blocks of 256; each thread strides
// over the arena); 0 (default): one block per CU. TAM_OPTIM_GRID /
// optim_grid(): A/B of the cap. Partial waves of blocks (1.5 per CU) measured
// 10-15 % slower than whole multiples.
static int g_optim_grid = [] {
  const char* e = getenv("TAM_OPTIM_GRID");
  return e ? atoi(e) : 0;
}();
TAM_KNOB(g_optim_grid)
void optim_grid(int blocks) { g_optim_grid = blocks > 0 ? blocks : 0; }

static int ogrid(long n4) {
  static int cus = 0;
  if (!cus) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess ||
        hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus < 1)
      cus = 256;
  }
  const long cap = g_optim_grid > 0 ? g_optim_grid : cus;
  long b = (n4 + 255) / 256;
  if (b > cap) b = cap;
  return (int)(b < 1 ? 1 : b);
}

// zero_from / wd_until (elements, multiples of 4): the gradient is reset only
// from zero_from on (store-first gradients before it, Fx.grad_mode), weight
// decay applies only below wd_until -- one launch over a whole arena's
// store / decay / no-decay regions (was three launches through round 5)
void sgd_step(float* w, float* g, float* mom, bf16_t* wb, long n, float lr, float momentum,
              float wd, float gscale, int nesterov, int zero_grad, hipStream_t s, const unsigned* guard,
              long zero_from, long wd_until, const float* clip) {
  // n % 4 == 0 (arena segments are padded to 64 elements)
  const dim3 grid(ogrid(n / 4));
  const long zf4 = zero_from / 4, wu4 = wd_until < 0 ? n / 4 : wd_until / 4;
  switch (optim_pick(n / 4, false)) {
    case 3:
      hipLaunchKernelGGL((sgd_stream_kernel<4, true>), grid, dim3(256), 0, s, w, g, mom, wb, n / 4, lr, momentum, wd,
                         gscale, nesterov, zero_grad, guard, zf4, wu4, clip);
      break;
    default:
      hipLaunchKernelGGL(sgd_kernel, grid, dim3(256), 0, s, w, g, mom, wb, n / 4, lr, momentum, wd, gscale, nesterov,
                         zero_grad, guard, zf4, wu4, clip);
  }
}

void adam_step(float* w, float* g, float* m, float* v, bf16_t* wb, long n, float lr, float b1,
               float b2, float eps, float wd, int step, float gscale, int zero_grad,
               hipStream_t s, const unsigned* guard, long zero_from, long wd_until, const float* clip) {
  const float bc1 = 1.f - powf(b1, (float)step), bc2 = 1.f - powf(b2, (float)step);
  const dim3 grid(ogrid(n / 4));
  const long zf4 = zero_from / 4, wu4 = wd_until < 0 ? n / 4 : wd_until / 4;
  switch (optim_pick(n / 4, true)) {
    case 3:
      hipLaunchKernelGGL((adam_stream_kernel<4, true>), grid, dim3(256), 0, s, w, g, m, v, wb, n / 4, lr, b1, b2, eps,
                         wd, bc1, bc2, gscale, zero_grad, guard, zf4, wu4, clip);
      break;
    default:
      hipLaunchKernelGGL(adam_kernel, grid, dim3(256), 0, s, w, g, m, v, wb, n / 4, lr, b1, b2, eps, wd, bc1, bc2,
                         gscale, zero_grad, guard, zf4, wu4, clip);
  }
}

// bf16-state steps: the streaming form only (TAM_OPTIM_VARIANT selects among
// the fp32-state kernels). base (elements, % 4 == 0): arena index of element 0
// of this launch; step: the 1-based optimizer step, for SGD too (it indexes
// the rounding draws).
void sgd_step_bf16s(float* w, float* g, bf16_t* mom, bf16_t* wb, long n, float lr, float momentum, float wd,
                    float gscale, int nesterov, int zero_grad, unsigned seed, unsigned step, long base,
                    hipStream_t s, const unsigned* guard, long zero_from, long wd_until, const float* clip) {
  const dim3 grid(ogrid(n / 4));
  const long zf4 = zero_from / 4, wu4 = wd_until < 0 ? n / 4 : wd_until / 4;
  hipLaunchKernelGGL((sgd_stream_bf16s_kernel<4, true>), grid, dim3(256), 0, s, w, g, mom, wb, n / 4, lr, momentum,
                     wd, gscale, nesterov, zero_grad, guard, zf4, wu4, clip, seed, step, base / 4);
}

void adam_step_bf16s(float* w, float* g, bf16_t* m, bf16_t* v, bf16_t* wb, long n, float lr, float b1, float b2,
                     float eps, float wd, int step, float gscale, int zero_grad, unsigned seed, long base,
                     hipStream_t s, const unsigned* guard, long zero_from, long wd_until, const float* clip) {
  const float bc1 = 1.f - powf(b1, (float)step), bc2 = 1.f - powf(b2, (float)step);
  const dim3 grid(ogrid(n / 4));
  const long zf4 = zero_from / 4, wu4 = wd_until < 0 ? n / 4 : wd_until / 4;
  hipLaunchKernelGGL((adam_stream_bf16s_kernel<4, true>), grid, dim3(256), 0, s, w, g, m, v, wb, n / 4, lr, b1, b2,
                     eps, wd, bc1, bc2, gscale, zero_grad, guard, zf4, wu4, clip, seed, (unsigned)step, base / 4);
}

// ------------------------------------------------- global-norm gradient clip
// Pass 1, grad_sumsq: one streaming read of the gradient arena on the
// optimizer's grid (ogrid), U float4 loads in flight per lane. The loads are
// ordinary, not NT: the optimizer reads the same bytes next, so an arena that
// fits stays in L2 / MALL. Squares accumulate in fp64 per thread (the pass is
// memory-bound, vector fp64 FMA is full rate), then wave shuffles + LDS; each
// block stores ONE fp64 partial into its own slot and the slots past the grid
// are zeroed, so pass 2 sums a fixed count in a fixed order. No float
// atomics: for a fixed grid the norm is bitwise reproducible, as the slab
// split-K and BN reductions are.
template <int U>
__global__ void __launch_bounds__(256) grad_sumsq_kernel(const float* __restrict__ g, long n4,
                                                          double* __restrict__ partials, int slots) {
  const long stride = (long)gridDim.x * blockDim.x;
  const long t = blockIdx.x * (long)blockDim.x + threadIdx.x;
  const long full = n4 / (U * stride) * (U * stride);
  double a0 = 0., a1 = 0., a2 = 0., a3 = 0.;
  auto acc = [&](float4 v) {
    a0 = fma((double)v.x, (double)v.x, a0); a1 = fma((double)v.y, (double)v.y, a1);
    a2 = fma((double)v.z, (double)v.z, a2); a3 = fma((double)v.w, (double)v.w, a3);
  };
  for (long base = t; base < full; base += U * stride) {
    float4 gv[U];
#pragma unroll
    for (int u = 0; u < U; ++u) gv[u] = ((const float4*)g)[base + u * stride];
#pragma unroll
    for (int u = 0; u < U; ++u) acc(gv[u]);
  }
  for (long i = full + t; i < n4; i += stride) acc(((const float4*)g)[i]);
  double r = (a0 + a1) + (a2 + a3);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) r += __shfl_down(r, o, 64);
  __shared__ double wsum[4];
  if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = r;
  __syncthreads();
  if (threadIdx.x == 0) partials[blockIdx.x] = (wsum[0] + wsum[1]) + (wsum[2] + wsum[3]);
  for (long s = gridDim.x + t; s < slots; s += stride) partials[s] = 0.;
}

// Pass 2, one block: sumsq = partials[0..P) in a fixed order, then the clip
// record (4 words, 16 B): [0] float scale, [1] float norm of this step,
// [2] uint32 non-finite steps, [3] uint32 steps that clipped.
//   norm = gscale * sqrt(sumsq)
//   finite:     scale = min(1, max_norm / (norm + 1e-6))   (clip_grad_norm_)
//   non-finite: scale = -1 -> the optimizer only resets the gradient
__global__ void __launch_bounds__(256) grad_clip_finalize_kernel(const double* __restrict__ partials, int P,
                                                                  float max_norm, float gscale, float* clip) {
  __shared__ double red[256];
  double a = 0.;
  for (int i = threadIdx.x; i < P; i += 256) a += partials[i];
  red[threadIdx.x] = a;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const float norm = (float)((double)gscale * sqrt(red[0]));
    unsigned* cnt = (unsigned*)clip;
    float scale = -1.f;
    if (isfinite(norm)) {
      // the quotient in fp64: one rounding into the fp32 scale
      scale = fminf(1.f, (float)((double)max_norm / ((double)norm + 1e-6)));
      if (scale < 1.f) cnt[3] += 1u;
    } else {
      cnt[2] += 1u;
    }
    clip[0] = scale;
    clip[1] = norm;
  }
}

int grad_sumsq_blocks(long n) { return ogrid(n / 4); }

void grad_sumsq(const float* g, long n, double* partials, int slots, hipStream_t s) {
  // n % 4 == 0, slots >= grad_sumsq_blocks(n)
  hipLaunchKernelGGL((grad_sumsq_kernel<8>), dim3(ogrid(n / 4)), dim3(256), 0, s, g, n / 4, partials, slots);
}

void grad_clip_finalize(const double* partials, int slots, float max_norm, float gscale, float* clip,
                        hipStream_t s) {
  hipLaunchKernelGGL(grad_clip_finalize_kernel, dim3(1), dim3(256), 0, s, partials, slots, max_norm, gscale, clip);
}

// ---------------------------------------------------- layer-wise trust ratio
// LARS (over SGD momentum) and LAMB (over AdamW) for the decayed region
// [0, n_decay) of an arena; the no-decay tail runs sgd_step / adam_step on
// its slice (ratio 1, wd 0). A segment is one parameter's padded extent; the
// host cuts every segment into tiles of at most kTrustTile elements (a
// multiple of 64, a segment's last tile may be short) and passes
//   tiles     int4 [ntiles]   {start, length, segment, 0}, elements
//   seg_first int  [nseg + 1] first tile of every segment, then ntiles
// Contract (||.|| = L2 norm over the segment, fp64 sums; g^ = g * gscale,
// gscale including the clip scale):
//   LARS  r = eta |w| / (|g^| + wd |w|);  d = r (g^ + wd w);
//         mom = momentum mom + d;  w -= lr mom
//   LAMB  m, v, m^, v^ as adam_stream_kernel;  u = m^ / (sqrt(v^) + eps) + wd w;
//         r = eta |w| / |u|;  w -= (lr r) u       (r = 1: the Adam step, bitwise)
//   r = 1 unless both norms are finite and > 0. The quotient is formed in
//   fp64 and rounded once to fp32, as grad_clip_finalize's scale is.
// Pass 1 (blocks stride over TILES on the optimizer's grid): one block reduces
//   a tile's w^2 and g^^2 / u^2 in fp64 -- lane-local sums over a fixed
//   element -> thread map, wave shuffles, four wave sums through LDS -- and
//   stores the pair into the TILE's slot: the order depends on the tile
//   alone, so the norms do not depend on the grid. No atomics. The LAMB form
//   also stores the new m / v (pass 3 reads them back; the gradient is not
//   read again) and resets the gradient.
// Pass 2 (one wave per segment): lane l sums the segment's tiles l, l + 64,
//   ... in tile order, the 64 lane sums fold by shuffles; writes
//   ratios[seg] = {r, |w|, |g^| or |u|}.
// Pass 3 (blocks stride over tiles): the streaming update with the tile's
//   ratio, NT 16-B accesses as the streaming kernels above.
// A tile record that does not lie inside [0, n_decay) / [0, nseg) is skipped
// by every pass (nothing is read or written through it).
// Skipped step (guard word / negative clip scale): passes 1 and 2 return,
// pass 3 resets the gradient from zero_from on; nothing else is written.
constexpr int kTrustTile = 8192;   // elements: 256 threads x 8 float4 groups
int trust_tile() { return kTrustTile; }

__device__ __forceinline__ bool step_skipped(const unsigned* guard, const float* clip) {
  return (guard != nullptr && *guard != 0u) || (clip != nullptr && clip[0] < 0.f);
}
__device__ __forceinline__ bool trust_tile_ok(int4 t, long n_decay, int nseg) {
  return t.x >= 0 && t.y > 0 && t.y <= kTrustTile && ((t.x | t.y) & 63) == 0 && (long)t.x + t.y <= n_decay &&
         t.z >= 0 && t.z < nseg;
}
// the LAMB update direction; passes 1 and 3 both call it on the same values
__device__ __forceinline__ float lamb_u(float w, float m, float v, float ib1, float ib2, float eps, float wd) {
  const float mh = m * ib1, vh = v * ib2;
  return __builtin_fmaf(wd, w, mh / (sqrtf(vh) + eps));
}
struct Sq4 {
  double a0 = 0., a1 = 0., a2 = 0., a3 = 0.;
  __device__ __forceinline__ void add(float x, float y, float z, float w) {
    a0 = fma((double)x, (double)x, a0); a1 = fma((double)y, (double)y, a1);
    a2 = fma((double)z, (double)z, a2); a3 = fma((double)w, (double)w, a3);
  }
  __device__ __forceinline__ double sum() const { return (a0 + a1) + (a2 + a3); }
};
// block sum of (a, b) into partials[slot]; red: this tile's LDS buffer. One
// barrier: the caller alternates between two buffers
__device__ __forceinline__ void tile_store2(double a, double b, double (*red)[2], double* __restrict__ partials,
                                            int slot) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    a += __shfl_down(a, o, 64);
    b += __shfl_down(b, o, 64);
  }
  if ((threadIdx.x & 63) == 0) {
    red[threadIdx.x >> 6][0] = a;
    red[threadIdx.x >> 6][1] = b;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    partials[2 * (long)slot] = (red[0][0] + red[1][0]) + (red[2][0] + red[3][0]);
    partials[2 * (long)slot + 1] = (red[0][1] + red[1][1]) + (red[2][1] + red[3][1]);
  }
}

__global__ void __launch_bounds__(256) lars_norm_kernel(const float* __restrict__ w, const float* __restrict__ g,
                                                         const int4* __restrict__ tiles, int ntiles, long n_decay,
                                                         int nseg, float gscale, double* __restrict__ partials,
                                                         const unsigned* guard, const float* clip) {
  if (step_skipped(guard, clip)) return;
  if (clip != nullptr) gscale *= clip[0];
  __shared__ double red[2][4][2];
  constexpr int U = kTrustTile / 4 / 256;
  int par = 0;
  for (int t = blockIdx.x; t < ntiles; t += gridDim.x, par ^= 1) {
    const int4 tl = tiles[t];
    Sq4 sw, sg;
    if (trust_tile_ok(tl, n_decay, nseg)) {
      const long b4 = tl.x / 4;
      const int len4 = tl.y / 4;
      // ordinary loads: pass 3 reads the same bytes next
      float4 wv[U], gv[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int i = threadIdx.x + u * 256;
        wv[u] = gv[u] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (i < len4) {
          wv[u] = ((const float4*)w)[b4 + i];
          gv[u] = ((const float4*)g)[b4 + i];
        }
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        sw.add(wv[u].x, wv[u].y, wv[u].z, wv[u].w);
        sg.add(gv[u].x * gscale, gv[u].y * gscale, gv[u].z * gscale, gv[u].w * gscale);
      }
    }
    tile_store2(sw.sum(), sg.sum(), red[par], partials, t);
  }
}

__global__ void __launch_bounds__(256) lamb_moments_kernel(
    const float* __restrict__ w, float* __restrict__ g, float* __restrict__ m, float* __restrict__ v,
    const int4* __restrict__ tiles, int ntiles, long n_decay, int nseg, float b1, float b2, float eps, float wd,
    float bc1, float bc2, float gscale, long zero_from4, double* __restrict__ partials, const unsigned* guard,
    const float* clip) {
  if (step_skipped(guard, clip)) return;
  if (clip != nullptr) gscale *= clip[0];
  const float ib1 = 1.f / bc1, ib2 = 1.f / bc2;
  __shared__ double red[2][4][2];
  constexpr int U = 4;
  int par = 0;
  for (int t = blockIdx.x; t < ntiles; t += gridDim.x, par ^= 1) {
    const int4 tl = tiles[t];
    Sq4 sw, su;
    if (trust_tile_ok(tl, n_decay, nseg)) {
      const long b4 = tl.x / 4;
      const int len4 = tl.y / 4;
      for (int base = threadIdx.x; base < len4; base += U * 256) {
        float4 wv[U], gv[U], mv[U], vv[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const int i = base + u * 256;
          wv[u] = gv[u] = mv[u] = vv[u] = make_float4(0.f, 0.f, 0.f, 0.f);
          if (i < len4) {
            wv[u] = ((const float4*)w)[b4 + i];
            gv[u] = ld4<U, true>(g, b4 + i);
            mv[u] = ((const float4*)m)[b4 + i];
            vv[u] = ((const float4*)v)[b4 + i];
          }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const int i = base + u * 256;
          if (i >= len4) continue;
          const float* wp = (const float*)&wv[u]; const float* gp = (const float*)&gv[u];
          float* mp = (float*)&mv[u]; float* vp = (float*)&vv[u];
          float us[4];
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            const float gr = gp[k] * gscale;
            mp[k] = __builtin_fmaf(b1, mp[k], (1.f - b1) * gr);
            vp[k] = __builtin_fmaf(b2, vp[k], (1.f - b2) * gr * gr);
            us[k] = lamb_u(wp[k], mp[k], vp[k], ib1, ib2, eps, wd);
          }
          sw.add(wp[0], wp[1], wp[2], wp[3]);
          su.add(us[0], us[1], us[2], us[3]);
          ((float4*)m)[b4 + i] = mv[u];
          ((float4*)v)[b4 + i] = vv[u];
          if (b4 + i >= zero_from4) st4<true>(g, b4 + i, make_float4(0.f, 0.f, 0.f, 0.f));
        }
      }
    }
    tile_store2(sw.sum(), su.sum(), red[par], partials, t);
  }
}

__global__ void __launch_bounds__(64) trust_finalize_kernel(const double* __restrict__ partials,
                                                             const int* __restrict__ seg_first, int ntiles, int nseg,
                                                             float eta, float wd, int lamb,
                                                             float* __restrict__ ratios, const unsigned* guard,
                                                             const float* clip) {
  if (step_skipped(guard, clip)) return;
  const int s = blockIdx.x;
  if (s >= nseg) return;
  int a = seg_first[s], b = seg_first[s + 1];
  if (a < 0) a = 0;
  if (b > ntiles) b = ntiles;
  double sw = 0., sx = 0.;
  for (int t = a + (int)threadIdx.x; t < b; t += 64) {
    sw += partials[2 * (long)t];
    sx += partials[2 * (long)t + 1];
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    sw += __shfl_down(sw, o, 64);
    sx += __shfl_down(sx, o, 64);
  }
  if (threadIdx.x == 0) {
    const double wn = sqrt(sw), xn = sqrt(sx);
    double r = 1.;
    // the quotient in fp64: one rounding into the fp32 ratio
    if (isfinite(wn) && wn > 0. && isfinite(xn) && xn > 0.)
      r = lamb ? (double)eta * wn / xn : (double)eta * wn / (xn + (double)wd * wn);
    ratios[3 * s] = (float)r;
    ratios[3 * s + 1] = (float)wn;
    ratios[3 * s + 2] = (float)xn;
  }
}

__global__ void __launch_bounds__(256) lars_apply_kernel(float* __restrict__ w, float* __restrict__ g,
                                                          float* __restrict__ mom, bf16_t* __restrict__ wb,
                                                          const int4* __restrict__ tiles, int ntiles, long n_decay,
                                                          int nseg, const float* __restrict__ ratios, float lr,
                                                          float momentum, float wd, float gscale, long zero_from4,
                                                          const unsigned* guard, const float* clip) {
  if (step_skipped(guard, clip)) {
    const long n4 = n_decay / 4;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n4; i += (long)gridDim.x * blockDim.x)
      if (i >= zero_from4) st4<true>(g, i, make_float4(0.f, 0.f, 0.f, 0.f));
    return;
  }
  if (clip != nullptr) gscale *= clip[0];
  constexpr int U = 4;
  for (int t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const int4 tl = tiles[t];
    if (!trust_tile_ok(tl, n_decay, nseg)) continue;
    const float r = ratios[3 * tl.z];
    const long b4 = tl.x / 4;
    const int len4 = tl.y / 4;
    for (int base = threadIdx.x; base < len4; base += U * 256) {
      float4 wv[U], gv[U], mv[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int i = base + u * 256;
        wv[u] = gv[u] = mv[u] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (i < len4) {
          wv[u] = ld4<U, true>(w, b4 + i); gv[u] = ld4<U, true>(g, b4 + i); mv[u] = ld4<U, true>(mom, b4 + i);
        }
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int i = base + u * 256;
        if (i >= len4) continue;
        float* wp = (float*)&wv[u]; const float* gp = (const float*)&gv[u]; float* mp = (float*)&mv[u];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const float d = r * __builtin_fmaf(wd, wp[k], gp[k] * gscale);
          mp[k] = __builtin_fmaf(momentum, mp[k], d);
          wp[k] = __builtin_fmaf(-lr, mp[k], wp[k]);
        }
        st4<true>(w, b4 + i, wv[u]); st4<true>(mom, b4 + i, mv[u]);
        if (b4 + i >= zero_from4) st4<true>(g, b4 + i, make_float4(0.f, 0.f, 0.f, 0.f));
        st2<true>(wb, b4 + i, make_uint2(pack_bf2(wp[0], wp[1]), pack_bf2(wp[2], wp[3])));
      }
    }
  }
}

__global__ void __launch_bounds__(256) lamb_apply_kernel(float* __restrict__ w, float* __restrict__ g,
                                                          const float* __restrict__ m, const float* __restrict__ v,
                                                          bf16_t* __restrict__ wb, const int4* __restrict__ tiles,
                                                          int ntiles, long n_decay, int nseg,
                                                          const float* __restrict__ ratios, float lr, float eps,
                                                          float wd, float bc1, float bc2, long zero_from4,
                                                          const unsigned* guard, const float* clip) {
  if (step_skipped(guard, clip)) {
    const long n4 = n_decay / 4;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n4; i += (long)gridDim.x * blockDim.x)
      if (i >= zero_from4) st4<true>(g, i, make_float4(0.f, 0.f, 0.f, 0.f));
    return;
  }
  const float ib1 = 1.f / bc1, ib2 = 1.f / bc2;
  constexpr int U = 4;
  for (int t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const int4 tl = tiles[t];
    if (!trust_tile_ok(tl, n_decay, nseg)) continue;
    const float lrr = lr * ratios[3 * tl.z];
    const long b4 = tl.x / 4;
    const int len4 = tl.y / 4;
    for (int base = threadIdx.x; base < len4; base += U * 256) {
      float4 wv[U], mv[U], vv[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int i = base + u * 256;
        wv[u] = mv[u] = vv[u] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (i < len4) {
          wv[u] = ld4<U, true>(w, b4 + i); mv[u] = ld4<U, true>(m, b4 + i); vv[u] = ld4<U, true>(v, b4 + i);
        }
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int i = base + u * 256;
        if (i >= len4) continue;
        float* wp = (float*)&wv[u]; const float* mp = (const float*)&mv[u]; const float* vp = (const float*)&vv[u];
#pragma unroll
        for (int k = 0; k < 4; ++k)
          wp[k] = __builtin_fmaf(-lrr, lamb_u(wp[k], mp[k], vp[k], ib1, ib2, eps, wd), wp[k]);
        st4<true>(w, b4 + i, wv[u]);
        st2<true>(wb, b4 + i, make_uint2(pack_bf2(wp[0], wp[1]), pack_bf2(wp[2], wp[3])));
      }
    }
  }
}

// blocks of a tile-strided pass: the optimizer's grid cap, at most one block per tile
static int tgrid(int ntiles) {
  const int cap = ogrid(1L << 40);
  return ntiles < cap ? (ntiles < 1 ? 1 : ntiles) : cap;
}

void lars_step(float* w, float* g, float* mom, bf16_t* wb, long n, float lr, float momentum, float wd, float eta,
               float gscale, const int* tiles, int ntiles, const int* seg_first, int nseg, double* partials,
               float* ratios, hipStream_t s, const unsigned* guard, long zero_from, long wd_until,
               const float* clip) {
  const long nd = wd_until < 0 ? n : wd_until;
  if (nd > 0 && ntiles > 0 && nseg > 0) {
    const dim3 grid(tgrid(ntiles));
    hipLaunchKernelGGL(lars_norm_kernel, grid, dim3(256), 0, s, w, g, (const int4*)tiles, ntiles, nd, nseg, gscale,
                       partials, guard, clip);
    hipLaunchKernelGGL(trust_finalize_kernel, dim3(nseg), dim3(64), 0, s, partials, seg_first, ntiles, nseg, eta, wd,
                       0, ratios, guard, clip);
    hipLaunchKernelGGL(lars_apply_kernel, grid, dim3(256), 0, s, w, g, mom, wb, (const int4*)tiles, ntiles, nd, nseg,
                       ratios, lr, momentum, wd, gscale, zero_from / 4, guard, clip);
  }
  if (nd < n)
    sgd_step(w + nd, g + nd, mom + nd, wb + nd, n - nd, lr, momentum, 0.f, gscale, 0, 1, s, guard,
             zero_from > nd ? zero_from - nd : 0, -1, clip);
}

void lamb_step(float* w, float* g, float* m, float* v, bf16_t* wb, long n, float lr, float b1, float b2, float eps,
               float wd, int step, float eta, float gscale, const int* tiles, int ntiles, const int* seg_first,
               int nseg, double* partials, float* ratios, hipStream_t s, const unsigned* guard, long zero_from,
               long wd_until, const float* clip) {
  const float bc1 = 1.f - powf(b1, (float)step), bc2 = 1.f - powf(b2, (float)step);
  const long nd = wd_until < 0 ? n : wd_until;
  if (nd > 0 && ntiles > 0 && nseg > 0) {
    const dim3 grid(tgrid(ntiles));
    hipLaunchKernelGGL(lamb_moments_kernel, grid, dim3(256), 0, s, w, g, m, v, (const int4*)tiles, ntiles, nd, nseg,
                       b1, b2, eps, wd, bc1, bc2, gscale, zero_from / 4, partials, guard, clip);
    hipLaunchKernelGGL(trust_finalize_kernel, dim3(nseg), dim3(64), 0, s, partials, seg_first, ntiles, nseg, eta, wd,
                       1, ratios, guard, clip);
    hipLaunchKernelGGL(lamb_apply_kernel, grid, dim3(256), 0, s, w, g, m, v, wb, (const int4*)tiles, ntiles, nd, nseg,
                       ratios, lr, eps, wd, bc1, bc2, zero_from / 4, guard, clip);
  }
  if (nd < n)
    adam_step(w + nd, g + nd, m + nd, v + nd, wb + nd, n - nd, lr, b1, b2, eps, 0.f, step, gscale, 1, s, guard,
              zero_from > nd ? zero_from - nd : 0, -1, clip);
}

__global__ void lstm_guard_step_kernel(unsigned* err) {
  if (threadIdx.x == 0 && err[0] != 0u) {
    err[1] += 1u;
    err[0] = 0u;
  }
}

void lstm_guard_step(unsigned* err, hipStream_t s) {
  hipLaunchKernelGGL(lstm_guard_step_kernel, dim3(1), dim3(64), 0, s, err);
}

}  // namespace tam
