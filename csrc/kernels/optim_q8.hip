// tiresias_amd — fused optimizer steps over a flat arena whose moments are kept
// as 8-bit block-scaled codes (Trainer opt_dtype="q8"; block-wise 8-bit
// optimizer state, Dettmers et al. 2021, with companded codes).
//
// Format (README "8-bit optimizer state"; Fx.q8_tables holds the tables):
// the arena is cut into quantisation blocks of 256 consecutive elements,
// block b = arena [256 b, 256 b + 256); the last one may be partial, a missing
// element counts as 0 and is never loaded or stored in w / g / wb. Per block
// and per moment the state is one fp32 scale (the block's max |value|) and
// one code byte per element:
//   first moment / SGD momentum  int8  q in [-127, 127]: sign(q) TM[|q|] scale,
//                                TM[k] = (k / 127)^2
//   Adam second moment           uint8 q in [0, 255]:    TV[q] scale,
//                                TV[k] = (k / 255)^4
// Both tables are formed in fp64 (d = k / N, d2 = d * d, TM = d2, TV = d2 * d2)
// and rounded to fp32 once; a decoded value is one fp32 multiply.
//
// Encoding a new moment x of a block with scale s: s == 0 -> code 0; s not
// finite -> code 0 as well and s is stored, so the block decodes non-finite
// (0 * inf) and the poison stays visible. Otherwise y = |x| / s in [0, 1]
// (formed as |x| * (1 / s), clamped to 1, and exactly 1 for |x| == s), k with
// T[k] <= y <= T[k + 1] from a hardware sqrt guess fixed up against the table,
// and the code is k + 1 with probability (y - T[k]) / (T[k + 1] - T[k]), else
// k: rounding is stochastic in the VALUE domain, the stored value's
// expectation is x. The draw is the element's 16-bit draw of the
// optimizer-state contract (tam/philox.h): u_m for the first moment /
// momentum, u_v for the second moment, up iff u < p * 65536 (compared as
// u (T[k+1] - T[k]) < (y - T[k]) 65536: no division). The block's max element
// encodes to exactly +-127 / 255; a nonzero second moment is never stored as
// code 0 (floored at 1: a zero v under a live m would turn the next step's
// m / (sqrt(v) + eps) into a jump, rounding up errs toward a smaller step).
//
// Work split: a quantisation block is ONE wave64 times one float4 per lane.
// Lane l holds elements 4l .. 4l+3: w and g are one 16-B load each, each
// moment's codes one 4-B load (the wave reads one coalesced 256-B line per
// moment), the scales one wave-uniform load each. The block max of a new
// moment is a wave reduction (xor shuffles, 6 steps) over the |x| bit
// patterns as unsigned integers -- for non-negative floats that is the float
// order with NaN above inf, so a poisoned element wins the max -- with no LDS
// and no barrier in the loop. LDS holds only the two tables (1.5 KB), filled
// once per workgroup. Grid: three 256-thread blocks per CU (per unit of the
// optimizer's grid cap, optim_grid): further resident waves run under a
// block's decode / reduce / encode chain. Each of a workgroup's 4 waves
// strides over blocks, U blocks' loads in flight before the first is consumed
// (U = 1 is what measured best); the Philox draws are issued after the
// loads and depend on none of them. Non-temporal loads and stores throughout.
//
// The element update is the fp32-state kernels' exact FMA sequence (optim.hip)
// on the decoded moments, and the weight and the shadow come from the fresh
// UNROUNDED moments; only what is stored is quantised. A block's result
// depends on nothing outside it: state and weights are bitwise independent of
// the grid and of U. No atomics. The guard / non-finite-clip path writes no
// state and draws nothing; it resets the gradient from zero_from on.
#include <cmath>

#include "tam/common.h"
#include "tam/kernels.h"
#include "tam/philox.h"

namespace tam {
namespace {

typedef unsigned u32x2_t __attribute__((ext_vector_type(2)));

__device__ __forceinline__ float4 q8_ld4(const float* p, long i) {
  const f32x4_t r = __builtin_nontemporal_load((const f32x4_t*)p + i);
  return make_float4(r[0], r[1], r[2], r[3]);
}
__device__ __forceinline__ void q8_st4(float* p, long i, float4 v) {
  __builtin_nontemporal_store(f32x4_t{v.x, v.y, v.z, v.w}, (f32x4_t*)p + i);
}
__device__ __forceinline__ uint32_t q8_ld1(const void* p, long i) {
  return __builtin_nontemporal_load((const uint32_t*)p + i);
}
__device__ __forceinline__ void q8_st1(void* p, long i, uint32_t v) {
  __builtin_nontemporal_store(v, (uint32_t*)p + i);
}
__device__ __forceinline__ void q8_st_shadow(bf16_t* p, long i, const float* w) {
  __builtin_nontemporal_store(u32x2_t{pack_bf2(w[0], w[1]), pack_bf2(w[2], w[3])}, (u32x2_t*)p + i);
}

struct Q8Tables {
  float tm[128];
  float tv[256];
};

// 256 threads fill both tables; ends in the workgroup's one barrier
__device__ __forceinline__ void q8_fill(Q8Tables& t) {
  const int k = threadIdx.x;
  const double a = (double)k / 255.0, a2 = a * a;
  t.tv[k] = (float)(a2 * a2);
  if (k < 128) {
    const double b = (double)k / 127.0;
    t.tm[k] = (float)(b * b);
  }
  __syncthreads();
}

__device__ __forceinline__ void q8_decode_m(uint32_t codes, float scale, const Q8Tables& t, float* m) {
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int q = (int)(int8_t)(codes >> (8 * j));
    const float a = t.tm[(q < 0 ? -q : q) & 127] * scale;
    m[j] = q < 0 ? -a : a;
  }
}
__device__ __forceinline__ void q8_decode_v(uint32_t codes, float scale, const Q8Tables& t, float* v) {
#pragma unroll
  for (int j = 0; j < 4; ++j) v[j] = t.tv[(codes >> (8 * j)) & 255u] * scale;
}

// bits of the wave's max |x[j]|: NaN > inf > every finite value
__device__ __forceinline__ uint32_t q8_wave_absmax(const float* x) {
  uint32_t a = 0u;
#pragma unroll
  for (int j = 0; j < 4; ++j) a = max(a, __float_as_uint(x[j]) & 0x7fffffffu);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) a = max(a, (uint32_t)__shfl_xor((int)a, o, 64));
  return a;
}

// 1 / s would overflow for a subnormal scale: such a block is scaled up by
// 2^64 first (exact, and * 1 for every normal scale: the same bits as without)
struct Q8Scale {
  float s, pre, rs;
  __device__ __forceinline__ explicit Q8Scale(uint32_t sb) {
    s = __uint_as_float(sb);
    pre = sb < 0x00800000u ? 0x1p64f : 1.f;
    rs = 1.f / (s * pre);
  }
};

// code in [0, N] of ax = |x| under scale sc.s (finite, > 0), table T of N + 1
// entries, T[k] = (k / N)^2 (ROOT4 false) or (k / N)^4 (true), rounded with
// the 16-bit draw u
template <int N, bool ROOT4>
__device__ __forceinline__ int q8_code(float ax, const Q8Scale& sc, uint32_t u, const float* T) {
  const float y = ax == sc.s ? 1.f : fminf(ax * sc.pre * sc.rs, 1.f);
  float r = __builtin_amdgcn_sqrtf(y);
  if constexpr (ROOT4) r = __builtin_amdgcn_sqrtf(r);
  int k = min((int)(r * (float)N), N - 1);
  float lo = T[k], hi = T[k + 1];
  if (y < lo) {              // (T[0] = 0 <= y: k >= 1 here)
    k = max(k - 1, 0);
    hi = lo;
    lo = T[k];
  } else if (y > hi) {       // (y <= 1 = T[N]: k + 1 < N here)
    k = min(k + 1, N - 1);
    lo = hi;
    hi = T[k + 1];
  }
  return k + ((float)u * (hi - lo) < (y - lo) * 65536.f ? 1 : 0);
}

// the four int8 codes of a lane's first moments / momenta under block max
// bits sb, rounded with the low halves of the draw words
__device__ __forceinline__ uint32_t q8_encode_m(const float* m, uint32_t sb, const uint32_t* draw,
                                                const Q8Tables& t) {
  if (sb == 0u || sb >= 0x7f800000u) return 0u;
  const Q8Scale sc(sb);
  uint32_t out = 0u;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int c = q8_code<127, false>(fabsf(m[j]), sc, draw[j] & 0xffffu, t.tm);
    out |= (uint32_t)((m[j] < 0.f ? -c : c) & 0xff) << (8 * j);
  }
  return out;
}
// the four uint8 codes of a lane's second moments: the high halves of the
// draw words; a nonzero value never gets code 0
__device__ __forceinline__ uint32_t q8_encode_v(const float* v, uint32_t sb, const uint32_t* draw,
                                                const Q8Tables& t) {
  if (sb == 0u || sb >= 0x7f800000u) return 0u;
  const Q8Scale sc(sb);
  uint32_t out = 0u;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    int c = q8_code<255, true>(fabsf(v[j]), sc, draw[j] >> 16, t.tv);
    if (c == 0 && v[j] != 0.f) c = 1;
    out |= (uint32_t)c << (8 * j);
  }
  return out;
}

struct Q8Draw {
  uint32_t r[4];
};

__device__ __forceinline__ bool q8_skipped(const unsigned* guard, const float* clip) {
  return (guard != nullptr && *guard != 0u) || (clip != nullptr && clip[0] < 0.f);
}
__device__ __forceinline__ void q8_reset_grad(float* g, long n4, long zero_from4) {
  const long stride = (long)gridDim.x * blockDim.x;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n4; i += stride)
    if (i >= zero_from4) q8_st4(g, i, make_float4(0.f, 0.f, 0.f, 0.f));
}

// what a lane loads of one quantisation block
struct Q8SgdIn {
  float4 w, g;
  uint32_t mc;
  float sm;
};
struct Q8AdamIn {
  float4 w, g;
  uint32_t mc, vc;
  float sm, sv;
};

}  // namespace

// nb: quantisation blocks = ceil(n4 / 64); sm / sv: the scale rows [nb]
template <int U>
__global__ void __launch_bounds__(256) adam_stream_q8_kernel(
    float* __restrict__ w, float* __restrict__ g, int8_t* __restrict__ mq, uint8_t* __restrict__ vq,
    float* __restrict__ sm, float* __restrict__ sv, bf16_t* __restrict__ wb, long n4, long nb, float lr, float b1,
    float b2, float eps, float wd0, float bc1, float bc2, float gscale, int zero_grad, const unsigned* guard,
    long zero_from4, long wd_until4, const float* clip, uint32_t seed, uint32_t step) {
  if (q8_skipped(guard, clip)) {
    q8_reset_grad(g, n4, zero_from4);
    return;
  }
  __shared__ Q8Tables tab;
  q8_fill(tab);
  if (clip != nullptr) gscale *= clip[0];
  const float ib1 = 1.f / bc1, ib2 = 1.f / bc2;
  const int lane = threadIdx.x & 63;
  auto load = [&](long b, Q8AdamIn& in) {
    const long i = b * 64 + lane;
    in.w = in.g = make_float4(0.f, 0.f, 0.f, 0.f);
    in.mc = in.vc = 0u;
    if (i < n4) {
      in.w = q8_ld4(w, i); in.g = q8_ld4(g, i); in.mc = q8_ld1(mq, i); in.vc = q8_ld1(vq, i);
    }
    in.sm = sm[b]; in.sv = sv[b];
  };
  auto body = [&](long b, Q8AdamIn& in, const Q8Draw& d) {
    const long i = b * 64 + lane;
    const bool live = i < n4;
    float mp[4], vp[4];
    q8_decode_m(in.mc, in.sm, tab, mp);
    q8_decode_v(in.vc, in.sv, tab, vp);
    float* wp = (float*)&in.w; const float* gp = (const float*)&in.g;
    const float wd = i < wd_until4 ? wd0 : 0.f;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float gr = gp[k] * gscale;
      mp[k] = __builtin_fmaf(b1, mp[k], (1.f - b1) * gr);
      vp[k] = __builtin_fmaf(b2, vp[k], (1.f - b2) * gr * gr);
      const float mh = mp[k] * ib1, vh = vp[k] * ib2;
      const float u = __builtin_fmaf(wd, wp[k], mh / (sqrtf(vh) + eps));   // decoupled (AdamW)
      wp[k] = __builtin_fmaf(-lr, u, wp[k]);
      if (!live) mp[k] = vp[k] = 0.f;     // a missing element counts as 0
    }
    if (live) {
      q8_st4(w, i, in.w);
      if (zero_grad && i >= zero_from4) q8_st4(g, i, make_float4(0.f, 0.f, 0.f, 0.f));
      q8_st_shadow(wb, i, wp);
    }
    const uint32_t bm = q8_wave_absmax(mp), bv = q8_wave_absmax(vp);
    const uint32_t mc = q8_encode_m(mp, bm, d.r, tab), vc = q8_encode_v(vp, bv, d.r, tab);
    if (live) {
      q8_st1(mq, i, mc); q8_st1(vq, i, vc);
    }
    if (lane == 0) {
      sm[b] = __uint_as_float(bm); sv[b] = __uint_as_float(bv);
    }
  };
  const long wave = blockIdx.x * 4L + (threadIdx.x >> 6), nw = gridDim.x * 4L;
  const long full = nb / (U * nw) * (U * nw);
  for (long base = wave; base < full; base += U * nw) {
    Q8AdamIn in[U];
    Q8Draw d[U];
#pragma unroll
    for (int u = 0; u < U; ++u) load(base + u * nw, in[u]);
#pragma unroll
    for (int u = 0; u < U; ++u) opt_state_draw4((uint64_t)((base + u * nw) * 64 + lane), seed, step, d[u].r);
#pragma unroll
    for (int u = 0; u < U; ++u) body(base + u * nw, in[u], d[u]);
  }
  for (long b = full + wave; b < nb; b += nw) {
    Q8AdamIn in;
    Q8Draw d;
    load(b, in);
    opt_state_draw4((uint64_t)(b * 64 + lane), seed, step, d.r);
    body(b, in, d);
  }
}

template <int U>
__global__ void __launch_bounds__(256) sgd_stream_q8_kernel(
    float* __restrict__ w, float* __restrict__ g, int8_t* __restrict__ mq, float* __restrict__ sm,
    bf16_t* __restrict__ wb, long n4, long nb, float lr, float momentum, float wd0, float gscale, int nesterov,
    int zero_grad, const unsigned* guard, long zero_from4, long wd_until4, const float* clip, uint32_t seed,
    uint32_t step) {
  if (q8_skipped(guard, clip)) {
    q8_reset_grad(g, n4, zero_from4);
    return;
  }
  __shared__ Q8Tables tab;
  q8_fill(tab);
  if (clip != nullptr) gscale *= clip[0];
  const int lane = threadIdx.x & 63;
  auto load = [&](long b, Q8SgdIn& in) {
    const long i = b * 64 + lane;
    in.w = in.g = make_float4(0.f, 0.f, 0.f, 0.f);
    in.mc = 0u;
    if (i < n4) {
      in.w = q8_ld4(w, i); in.g = q8_ld4(g, i); in.mc = q8_ld1(mq, i);
    }
    in.sm = sm[b];
  };
  auto body = [&](long b, Q8SgdIn& in, const Q8Draw& dr) {
    const long i = b * 64 + lane;
    const bool live = i < n4;
    float mp[4];
    q8_decode_m(in.mc, in.sm, tab, mp);
    float* wp = (float*)&in.w; const float* gp = (const float*)&in.g;
    const float wd = i < wd_until4 ? wd0 : 0.f;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      float d = __builtin_fmaf(wd, wp[k], gp[k] * gscale);
      mp[k] = __builtin_fmaf(momentum, mp[k], d);
      d = nesterov ? __builtin_fmaf(momentum, mp[k], d) : mp[k];
      wp[k] = __builtin_fmaf(-lr, d, wp[k]);
      if (!live) mp[k] = 0.f;             // a missing element counts as 0
    }
    if (live) {
      q8_st4(w, i, in.w);
      if (zero_grad && i >= zero_from4) q8_st4(g, i, make_float4(0.f, 0.f, 0.f, 0.f));
      q8_st_shadow(wb, i, wp);
    }
    const uint32_t bm = q8_wave_absmax(mp);
    const uint32_t mc = q8_encode_m(mp, bm, dr.r, tab);
    if (live) q8_st1(mq, i, mc);
    if (lane == 0) sm[b] = __uint_as_float(bm);
  };
  const long wave = blockIdx.x * 4L + (threadIdx.x >> 6), nw = gridDim.x * 4L;
  const long full = nb / (U * nw) * (U * nw);
  for (long base = wave; base < full; base += U * nw) {
    Q8SgdIn in[U];
    Q8Draw d[U];
#pragma unroll
    for (int u = 0; u < U; ++u) load(base + u * nw, in[u]);
#pragma unroll
    for (int u = 0; u < U; ++u) opt_state_draw4((uint64_t)((base + u * nw) * 64 + lane), seed, step, d[u].r);
#pragma unroll
    for (int u = 0; u < U; ++u) body(base + u * nw, in[u], d[u]);
  }
  for (long b = full + wave; b < nb; b += nw) {
    Q8SgdIn in;
    Q8Draw d;
    load(b, in);
    opt_state_draw4((uint64_t)(b * 64 + lane), seed, step, d.r);
    body(b, in, d);
  }
}

// Measured on live data (profiles/r7/opt_q8.md): the step is bound by a
// block's decode / reduce / encode chain, not by bytes, so what pays is
// resident waves, not loads in flight per wave. Three workgroups per CU (per
// unit of optim_grid's cap) with one block per wave per pass was the best of
// 1-6 workgroups x U = 1, 2, 4; at the fp32 / bf16-state kernels' one
// workgroup per CU and U = 4 the Adam step took 1.85x as long. The result
// does not depend on either.
constexpr int kQ8Unroll = 1, kQ8WgsPerCu = 3;

// a workgroup's 4 waves take 4 quantisation blocks = 1024 elements per pass,
// the extent a 256-thread block of the float4 kernels covers
static int q8_grid(long n) {
  const long cap = (long)optim_tile_grid(1 << 30) * kQ8WgsPerCu, want = (n + 1023) / 1024;
  return (int)(want < 1 ? 1 : (want < cap ? want : cap));
}

void sgd_step_q8(float* w, float* g, int8_t* mq, float* sm, bf16_t* wb, long n, float lr, float momentum, float wd,
                 float gscale, int nesterov, int zero_grad, unsigned seed, unsigned step, hipStream_t s,
                 const unsigned* guard, long zero_from, long wd_until, const float* clip) {
  const dim3 grid(q8_grid(n));
  const long n4 = n / 4, nb = (n4 + 63) / 64;
  const long zf4 = zero_from / 4, wu4 = wd_until < 0 ? n4 : wd_until / 4;
  hipLaunchKernelGGL((sgd_stream_q8_kernel<kQ8Unroll>), grid, dim3(256), 0, s, w, g, mq, sm, wb, n4, nb, lr, momentum,
                     wd, gscale, nesterov, zero_grad, guard, zf4, wu4, clip, seed, step);
}

void adam_step_q8(float* w, float* g, int8_t* mq, uint8_t* vq, float* sm, float* sv, bf16_t* wb, long n, float lr,
                  float b1, float b2, float eps, float wd, int step, float gscale, int zero_grad, unsigned seed,
                  hipStream_t s, const unsigned* guard, long zero_from, long wd_until, const float* clip) {
  const float bc1 = 1.f - powf(b1, (float)step), bc2 = 1.f - powf(b2, (float)step);
  const dim3 grid(q8_grid(n));
  const long n4 = n / 4, nb = (n4 + 63) / 64;
  const long zf4 = zero_from / 4, wu4 = wd_until < 0 ? n4 : wd_until / 4;
  hipLaunchKernelGGL((adam_stream_q8_kernel<kQ8Unroll>), grid, dim3(256), 0, s, w, g, mq, vq, sm, sv, wb, n4, nb, lr,
                     b1, b2, eps, wd, bc1, bc2, gscale, zero_grad, guard, zf4, wu4, clip, seed, (unsigned)step);
}

}  // namespace tam
