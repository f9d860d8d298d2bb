// tiresias_amd — GroupNorm (NHWC, training) kernels.
//
// x [N][P = H*W][C] bf16, G groups of Cg = C / G channels (Cg a power of two
// in [2, 256]). The statistics of a (sample, group) run over a strided slab:
// P rows of Cg contiguous channels. Two routes, chosen on the host per call
// from (P, C, Cg) only, never from N:
//   * resident: ONE launch, x read once. A block owns one sample and one
//     channel slab of whole groups (max(64, Cg) channels; all of C when C <=
//     64), stages its P x slab tile in LDS (16-B loads; 128 contiguous bytes
//     per pixel at a 64-channel slab), takes the mean, then the centred sum of
//     squares from LDS (two passes: nothing cancels), then applies from LDS.
//     The backward stages x and the masked gradient dy' (2 tiles). Valid while
//     the tile(s) fit the LDS the device grants one block;
//   * tiled: any shape. Pass 1 cuts a sample into tiles of GN_TILE pixels and
//     writes per-(sample, tile, group) partials, shifted by a per-group pilot
//     value (the group's first element) so that |mean| >> std does not cancel
//     in fp32; a small finalize sums a group's tiles in tile order in fp64;
//     the apply pass streams with non-temporal accesses.
// Thread layout of every block: thread = (row lane, 16-B column vector), the
// column vectors of a row adjacent in a wave. Group fold (gn_group_sums):
// Cg < 8 -> 8 / Cg groups inside a lane's vector; Cg >= 8 -> Cg / 8 adjacent
// lanes fold by xor-shuffles; row lanes and waves fold through LDS in a fixed
// order. No atomics: a sample's results never depend on its batch-mates or on
// the grid. dgamma / dbeta leave as per-block partial rows [rows][2C] that
// col_reduce_acc (norm.hip) finishes.
#include "tam/common.h"
#include "tam/kernels.h"

namespace tam {
namespace {

constexpr int GN_THREADS = 256;
constexpr int GN_RED = GN_THREADS * 16;     // floats of block-reduce scratch
constexpr int GN_MAX_SLAB = 256;            // channels of the widest slab (Cg <= 256)
// static LDS of the widest kernel here (red + channel sums + group sums),
// rounded up: what the resident tile cannot have
constexpr int GN_STATIC_LDS = 24 * 1024;

typedef uint32_t gn_u32x4_t __attribute__((ext_vector_type(4)));

__device__ __forceinline__ void gn_unpack8(const uint4 v, float (&f)[8]) {
  const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    f[2 * i] = __uint_as_float(w[i] << 16);
    f[2 * i + 1] = __uint_as_float(w[i] & 0xffff0000u);
  }
}
__device__ __forceinline__ uint4 gn_pack8(const float (&f)[8]) {
  return make_uint4(pack_bf2(f[0], f[1]), pack_bf2(f[2], f[3]), pack_bf2(f[4], f[5]), pack_bf2(f[6], f[7]));
}
__device__ __forceinline__ uint4 gn_ld_nt(const bf16_t* p) {
  const gn_u32x4_t r = __builtin_nontemporal_load((const gn_u32x4_t*)p);
  return make_uint4(r.x, r.y, r.z, r.w);
}
__device__ __forceinline__ void gn_st_nt(bf16_t* p, const uint4 v) {
  __builtin_nontemporal_store(gn_u32x4_t{v.x, v.y, v.z, v.w}, (gn_u32x4_t*)p);
}

// a thread's place in its block: slab blockIdx.y of sw channels (the last one
// may be narrower), column vector v of the slab's tpr, row lane rl of rpp
struct GnLane {
  int c0, cs, tpr, rpp, v, rl, col;
  bool on;
};
__device__ __forceinline__ GnLane gn_lane(int C, int sw) {
  GnLane L;
  L.c0 = blockIdx.y * sw;
  L.cs = min(sw, C - L.c0);
  L.tpr = L.cs / 8;
  L.rpp = GN_THREADS / L.tpr;
  L.v = threadIdx.x % L.tpr;
  L.rl = threadIdx.x / L.tpr;
  L.col = L.c0 + L.v * 8;
  L.on = L.rl < L.rpp;
  return L;
}

// Two per-lane 8-channel sums (a, b; zeros in idle lanes) -> the slab's
// per-group sums over the whole block: out[g] = sum a, out[ngs + g] = sum b
// for g < ngs = cs / Cg. Every thread of the block calls it. red: GN_RED
// floats, free on entry after the leading barrier; out: 2 * ngs floats,
// readable on return.
__device__ __forceinline__ void gn_group_sums(const float (&a)[8], const float (&b)[8], const GnLane& L, int Cg,
                                              float* red, float* out) {
  const int ngs = L.cs / Cg;
  float ga[4], gb[4];
  int ng, g0;
  bool owner = true;
  if (Cg == 2) {
    ng = 4; g0 = L.v * 4;
#pragma unroll
    for (int i = 0; i < 4; ++i) { ga[i] = a[2 * i] + a[2 * i + 1]; gb[i] = b[2 * i] + b[2 * i + 1]; }
  } else if (Cg == 4) {
    ng = 2; g0 = L.v * 2;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      ga[i] = (a[4 * i] + a[4 * i + 1]) + (a[4 * i + 2] + a[4 * i + 3]);
      gb[i] = (b[4 * i] + b[4 * i + 1]) + (b[4 * i + 2] + b[4 * i + 3]);
    }
  } else {
    // the group's Cg / 8 vectors sit in adjacent lanes of one row, aligned to
    // their count (tpr is a multiple of it), so the xor partners are its own
    const int lw = Cg / 8;
    float ta = ((a[0] + a[1]) + (a[2] + a[3])) + ((a[4] + a[5]) + (a[6] + a[7]));
    float tb = ((b[0] + b[1]) + (b[2] + b[3])) + ((b[4] + b[5]) + (b[6] + b[7]));
    for (int o = 1; o < lw; o <<= 1) {
      ta += __shfl_xor(ta, o, 64);
      tb += __shfl_xor(tb, o, 64);
    }
    ng = 1; g0 = L.v / lw; owner = (L.v % lw) == 0;
    ga[0] = ta; gb[0] = tb;
  }
  __syncthreads();
  if (L.on && owner) {
    for (int i = 0; i < ng; ++i) {
      red[L.rl * ngs + g0 + i] = ga[i];
      red[GN_RED / 2 + L.rl * ngs + g0 + i] = gb[i];
    }
  }
  __syncthreads();
  for (int e = threadIdx.x; e < 2 * ngs; e += GN_THREADS) {
    const int q = e >= ngs, g = e - q * ngs;
    float t = 0.f;
    for (int j = 0; j < L.rpp; ++j) t += red[q * (GN_RED / 2) + j * ngs + g];
    out[e] = t;
  }
  __syncthreads();
}

// The same two sums per CHANNEL of the slab: out[c] = sum a, out[cs + c] = sum b
__device__ __forceinline__ void gn_channel_sums(const float (&a)[8], const float (&b)[8], const GnLane& L, float* red,
                                                float* out) {
  __syncthreads();
#pragma unroll
  for (int i = 0; i < 8; ++i) { red[threadIdx.x * 16 + i] = a[i]; red[threadIdx.x * 16 + 8 + i] = b[i]; }
  __syncthreads();
  for (int e = threadIdx.x; e < 2 * L.cs; e += GN_THREADS) {
    const int q = e >= L.cs, c = e - q * L.cs;
    float t = 0.f;
    for (int j = 0; j < L.rpp; ++j) t += red[(j * L.tpr + (c >> 3)) * 16 + q * 8 + (c & 7)];
    out[e] = t;
  }
  __syncthreads();
}

// dy' of one 8-channel vector: (dy + addend), zero where the stored y <= 0
__device__ __forceinline__ void gn_dyr(const uint4 vd, const uint4 va, const uint4 vy, bool add, bool relu,
                                       float (&fd)[8]) {
  gn_unpack8(vd, fd);
  if (add) {
    float fa[8];
    gn_unpack8(va, fa);
#pragma unroll
    for (int i = 0; i < 8; ++i) fd[i] += fa[i];
  }
  if (relu) {
    float fy[8];
    gn_unpack8(vy, fy);
#pragma unroll
    for (int i = 0; i < 8; ++i) fd[i] = fy[i] <= 0.f ? 0.f : fd[i];
  }
}

// ---------------------------------------------------------------- tiled forward
// grid (tiles, slabs, N). part[n][tile][g] = {sum (x - pilot_g), sum (x - pilot_g)^2}
__global__ void __launch_bounds__(GN_THREADS) gn_stats_kernel(const bf16_t* __restrict__ x, int P, int C, int Cg,
                                                              int sw, float2* __restrict__ part) {
  __shared__ float red[GN_RED / 2 + GN_RED / 4];
  __shared__ float out[GN_MAX_SLAB];
  const GnLane L = gn_lane(C, sw);
  const int n = blockIdx.z, tile = blockIdx.x, T = gridDim.x, G = C / Cg;
  const bf16_t* xn = x + (long)n * P * C;
  float pl[8], s[8], q[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    pl[j] = bf2f(xn[(L.col + j) & ~(Cg - 1)]);       // pixel 0, first channel of the group
    s[j] = q[j] = 0.f;
  }
  const int r1 = min(P, (tile + 1) * GN_TILE);
  if (L.on) {
    int r = tile * GN_TILE + L.rl;
    auto acc = [&](const uint4 v) {
      float f[8];
      gn_unpack8(v, f);
#pragma unroll
      for (int j = 0; j < 8; ++j) { const float d = f[j] - pl[j]; s[j] += d; q[j] += d * d; }
    };
    for (; r + 3 * L.rpp < r1; r += 4 * L.rpp) {
      uint4 v[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) v[u] = *(const uint4*)(xn + (long)(r + u * L.rpp) * C + L.col);
#pragma unroll
      for (int u = 0; u < 4; ++u) acc(v[u]);
    }
    for (; r < r1; r += L.rpp) acc(*(const uint4*)(xn + (long)r * C + L.col));
  }
  // (the group sums use the lower half of a GN_RED scratch: rpp * ngs <= 1024)
  gn_group_sums(s, q, L, Cg, red, out);
  const int ngs = L.cs / Cg;
  for (int e = threadIdx.x; e < ngs; e += GN_THREADS)
    part[((long)n * T + tile) * G + L.c0 / Cg + e] = make_float2(out[e], out[ngs + e]);
}

// one thread per (n, g): the group's tiles in tile order, fp64
__global__ void __launch_bounds__(GN_THREADS) gn_finalize_kernel(const bf16_t* __restrict__ x,
                                                                 const float2* __restrict__ part, int P, int C, int Cg,
                                                                 int T, int NG, float eps, float* __restrict__ mean,
                                                                 float* __restrict__ rstd) {
  const int i = blockIdx.x * GN_THREADS + threadIdx.x;
  if (i >= NG) return;
  const int G = C / Cg, n = i / G, g = i % G;
  const double pilot = (double)bf2f(x[(long)n * P * C + g * Cg]);
  double S = 0.0, Q = 0.0;
  for (int t = 0; t < T; ++t) {
    const float2 p = part[((long)n * T + t) * G + g];
    S += (double)p.x;
    Q += (double)p.y;
  }
  const double cnt = (double)P * Cg, m = S / cnt;
  double var = Q / cnt - m * m;
  if (var < 0) var = 0;
  mean[i] = (float)(pilot + m);
  rstd[i] = (float)(1.0 / sqrt(var + (double)eps));
}

// grid (tiles, slabs, N): y = relu?((x - mean) * rstd * gamma + beta (+ res))
__global__ void __launch_bounds__(GN_THREADS) gn_apply_kernel(
    const bf16_t* __restrict__ x, const bf16_t* __restrict__ res, bf16_t* __restrict__ y, int P, int C, int Cg, int sw,
    const float* __restrict__ mean, const float* __restrict__ rstd, const float* __restrict__ gamma,
    const float* __restrict__ beta, int relu) {
  const GnLane L = gn_lane(C, sw);
  if (!L.on) return;
  const int n = blockIdx.z, tile = blockIdx.x, G = C / Cg;
  float mu[8], sc[8], be[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int c = L.col + j, g = n * G + c / Cg;
    mu[j] = mean[g];
    sc[j] = rstd[g] * gamma[c];
    be[j] = beta[c];
  }
  auto one = [&](const long off, const uint4 vx, const uint4 vr) {
    float f[8], rr[8];
    gn_unpack8(vx, f);
    if (res) gn_unpack8(vr, rr);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      float o = (f[j] - mu[j]) * sc[j] + be[j];
      if (res) o += rr[j];
      if (relu) o = fmaxf(o, 0.f);
      f[j] = o;
    }
    gn_st_nt(y + off, gn_pack8(f));
  };
  const uint4 z = make_uint4(0, 0, 0, 0);
  const long base = (long)n * P * C + L.col;
  const int r1 = min(P, (tile + 1) * GN_TILE);
  int r = tile * GN_TILE + L.rl;
  for (; r + L.rpp < r1; r += 2 * L.rpp) {
    const long o0 = base + (long)r * C, o1 = base + (long)(r + L.rpp) * C;
    const uint4 x0 = gn_ld_nt(x + o0), x1 = gn_ld_nt(x + o1);
    const uint4 q0 = res ? gn_ld_nt(res + o0) : z, q1 = res ? gn_ld_nt(res + o1) : z;
    one(o0, x0, q0);
    one(o1, x1, q1);
  }
  if (r < r1) {
    const long o0 = base + (long)r * C;
    one(o0, gn_ld_nt(x + o0), res ? gn_ld_nt(res + o0) : z);
  }
}

// ---------------------------------------------------------------- resident forward
// grid (1, slabs, N); dynamic LDS: the P x cs tile, [P][tpr] 16-B vectors.
// Every thread reads back only the vectors it staged itself.
__global__ void __launch_bounds__(GN_THREADS) gn_fwd_resident_kernel(
    const bf16_t* __restrict__ x, const bf16_t* __restrict__ res, bf16_t* __restrict__ y, int P, int C, int Cg, int sw,
    const float* __restrict__ gamma, const float* __restrict__ beta, float eps, int relu, float* __restrict__ mean,
    float* __restrict__ rstd) {
  extern __shared__ uint4 gn_tile[];
  __shared__ float red[GN_RED / 2 + GN_RED / 4];
  __shared__ float out[GN_MAX_SLAB];
  __shared__ float s_mean[GN_MAX_SLAB / 2];
  const GnLane L = gn_lane(C, sw);
  const int n = blockIdx.z, G = C / Cg, ngs = L.cs / Cg;
  const long base = (long)n * P * C + L.col;
  const float inv = 1.f / ((float)P * (float)Cg);
  float s[8], zero[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) s[j] = zero[j] = 0.f;
  if (L.on) {
    auto stage = [&](const int r, const uint4 v) {
      gn_tile[r * L.tpr + L.v] = v;
      float f[8];
      gn_unpack8(v, f);
#pragma unroll
      for (int j = 0; j < 8; ++j) s[j] += f[j];
    };
    int r = L.rl;
    for (; r + 3 * L.rpp < P; r += 4 * L.rpp) {
      uint4 v[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) v[u] = *(const uint4*)(x + base + (long)(r + u * L.rpp) * C);
#pragma unroll
      for (int u = 0; u < 4; ++u) stage(r + u * L.rpp, v[u]);
    }
    for (; r < P; r += L.rpp) stage(r, *(const uint4*)(x + base + (long)r * C));
  }
  gn_group_sums(s, zero, L, Cg, red, out);
  float mu[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) mu[j] = out[(L.v * 8 + j) / Cg] * inv;
  for (int e = threadIdx.x; e < ngs; e += GN_THREADS) s_mean[e] = out[e] * inv;
  // centred second moment from LDS
#pragma unroll
  for (int j = 0; j < 8; ++j) s[j] = 0.f;
  if (L.on) {
    for (int r = L.rl; r < P; r += L.rpp) {
      float f[8];
      gn_unpack8(gn_tile[r * L.tpr + L.v], f);
#pragma unroll
      for (int j = 0; j < 8; ++j) { const float d = f[j] - mu[j]; s[j] += d * d; }
    }
  }
  gn_group_sums(s, zero, L, Cg, red, out);
  for (int e = threadIdx.x; e < ngs; e += GN_THREADS) {
    const int g = n * G + L.c0 / Cg + e;
    mean[g] = s_mean[e];
    rstd[g] = 1.f / sqrtf(out[e] * inv + eps);
  }
  if (!L.on) return;
  float sc[8], be[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    sc[j] = gamma[L.col + j] / sqrtf(out[(L.v * 8 + j) / Cg] * inv + eps);
    be[j] = beta[L.col + j];
  }
  const uint4 z = make_uint4(0, 0, 0, 0);
  for (int r = L.rl; r < P; r += L.rpp) {
    const long off = base + (long)r * C;
    const uint4 vr = res ? gn_ld_nt(res + off) : z;
    float f[8], rr[8];
    gn_unpack8(gn_tile[r * L.tpr + L.v], f);
    if (res) gn_unpack8(vr, rr);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      float o = (f[j] - mu[j]) * sc[j] + be[j];
      if (res) o += rr[j];
      if (relu) o = fmaxf(o, 0.f);
      f[j] = o;
    }
    gn_st_nt(y + off, gn_pack8(f));
  }
}

// ---------------------------------------------------------------- backward
// per-thread constants of a column vector: mean, rstd of each channel's group, gamma
struct GnCoef {
  float mu[8], rs[8], gm[8];
};
__device__ __forceinline__ GnCoef gn_coef(const GnLane& L, int n, int C, int Cg, const float* __restrict__ mean,
                                          const float* __restrict__ rstd, const float* __restrict__ gamma) {
  GnCoef k;
  const int G = C / Cg;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int c = L.col + j, g = n * G + c / Cg;
    k.mu[j] = mean[g];
    k.rs[j] = rstd[g];
    k.gm[j] = gamma[c];
  }
  return k;
}

// Tiled pass 1, grid (tiles, slabs, N): dy' (stored into dres when given,
// and then summed as stored); per-channel partial row n * T + tile of cpart
// [rows][2C] (sum dy' x^ | sum dy'); gpart[n][tile][g] = {sum gamma dy', sum gamma dy' x^}
__global__ void __launch_bounds__(GN_THREADS) gn_bwd_stats_kernel(
    const bf16_t* __restrict__ dy, const bf16_t* __restrict__ addend, const bf16_t* __restrict__ y,
    const bf16_t* __restrict__ x, const float* __restrict__ mean, const float* __restrict__ rstd,
    const float* __restrict__ gamma, int P, int C, int Cg, int sw, int relu, bf16_t* __restrict__ dres,
    float* __restrict__ cpart, float2* __restrict__ gpart) {
  __shared__ float red[GN_RED];
  __shared__ float outc[2 * GN_MAX_SLAB];
  __shared__ float outg[GN_MAX_SLAB];
  const GnLane L = gn_lane(C, sw);
  const int n = blockIdx.z, tile = blockIdx.x, T = gridDim.x, G = C / Cg;
  const GnCoef k = gn_coef(L, n, C, Cg, mean, rstd, gamma);
  float a[8], b[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) a[j] = b[j] = 0.f;
  const long base = (long)n * P * C + L.col;
  const int r1 = min(P, (tile + 1) * GN_TILE);
  if (L.on) {
    const uint4 z = make_uint4(0, 0, 0, 0);
    auto row = [&](const long off, const uint4 vd, const uint4 vx, const uint4 vy, const uint4 va) {
      float fd[8], fx[8];
      gn_dyr(vd, va, vy, addend != nullptr, relu != 0, fd);
      if (dres) {
        const uint4 pk = gn_pack8(fd);
        *(uint4*)(dres + off) = pk;
        gn_unpack8(pk, fd);
      }
      gn_unpack8(vx, fx);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        a[j] += fd[j];
        b[j] += fd[j] * ((fx[j] - k.mu[j]) * k.rs[j]);
      }
    };
    int r = tile * GN_TILE + L.rl;
    for (; r + L.rpp < r1; r += 2 * L.rpp) {
      uint4 vd[2], vx[2], vy[2], va[2];
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const long off = base + (long)(r + u * L.rpp) * C;
        vd[u] = *(const uint4*)(dy + off);
        vx[u] = *(const uint4*)(x + off);
        vy[u] = relu ? *(const uint4*)(y + off) : z;
        va[u] = addend ? *(const uint4*)(addend + off) : z;
      }
#pragma unroll
      for (int u = 0; u < 2; ++u) row(base + (long)(r + u * L.rpp) * C, vd[u], vx[u], vy[u], va[u]);
    }
    if (r < r1) {
      const long off = base + (long)r * C;
      row(off, *(const uint4*)(dy + off), *(const uint4*)(x + off), relu ? *(const uint4*)(y + off) : z,
          addend ? *(const uint4*)(addend + off) : z);
    }
  }
  gn_channel_sums(b, a, L, red, outc);
  float* crow = cpart + ((long)n * T + tile) * 2 * C;
  for (int e = threadIdx.x; e < 2 * L.cs; e += GN_THREADS) {
    const int q = e >= L.cs, c = e - q * L.cs;
    crow[q * C + L.c0 + c] = outc[e];
  }
  float ga[8], gb[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) { ga[j] = k.gm[j] * a[j]; gb[j] = k.gm[j] * b[j]; }
  gn_group_sums(ga, gb, L, Cg, red, outg);
  const int ngs = L.cs / Cg;
  for (int e = threadIdx.x; e < ngs; e += GN_THREADS)
    gpart[((long)n * T + tile) * G + L.c0 / Cg + e] = make_float2(outg[e], outg[ngs + e]);
}

// one thread per (n, g): m12 = {mean_g(gamma dy'), mean_g(gamma dy' x^)}, tiles in order, fp64
__global__ void __launch_bounds__(GN_THREADS) gn_bwd_finalize_kernel(const float2* __restrict__ gpart, int P, int C,
                                                                     int Cg, int T, int NG,
                                                                     float2* __restrict__ m12) {
  const int i = blockIdx.x * GN_THREADS + threadIdx.x;
  if (i >= NG) return;
  const int G = C / Cg, n = i / G, g = i % G;
  double A = 0.0, B = 0.0;
  for (int t = 0; t < T; ++t) {
    const float2 p = gpart[((long)n * T + t) * G + g];
    A += (double)p.x;
    B += (double)p.y;
  }
  const double cnt = (double)P * Cg;
  m12[i] = make_float2((float)(A / cnt), (float)(B / cnt));
}

// Tiled pass 2, grid (tiles, slabs, N): dx = rstd (gamma dy' - m1 - x^ m2);
// dres (when pass 1 did not store it): dy'
__global__ void __launch_bounds__(GN_THREADS) gn_bwd_apply_kernel(
    const bf16_t* __restrict__ dy, const bf16_t* __restrict__ addend, const bf16_t* __restrict__ y,
    const bf16_t* __restrict__ x, const float* __restrict__ mean, const float* __restrict__ rstd,
    const float* __restrict__ gamma, const float2* __restrict__ m12, int P, int C, int Cg, int sw, int relu,
    bf16_t* __restrict__ dx) {
  const GnLane L = gn_lane(C, sw);
  if (!L.on) return;
  const int n = blockIdx.z, tile = blockIdx.x, G = C / Cg;
  const GnCoef k = gn_coef(L, n, C, Cg, mean, rstd, gamma);
  float m1[8], m2[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const float2 m = m12[n * G + (L.col + j) / Cg];
    m1[j] = m.x;
    m2[j] = m.y;
  }
  const uint4 z = make_uint4(0, 0, 0, 0);
  const long base = (long)n * P * C + L.col;
  const int r1 = min(P, (tile + 1) * GN_TILE);
  auto one = [&](const long off, const uint4 vd, const uint4 vx, const uint4 vy, const uint4 va) {
    float fd[8], fx[8], o[8];
    gn_dyr(vd, va, vy, addend != nullptr, relu != 0, fd);
    gn_unpack8(vx, fx);
#pragma unroll
    for (int j = 0; j < 8; ++j)
      o[j] = k.rs[j] * (k.gm[j] * fd[j] - m1[j] - ((fx[j] - k.mu[j]) * k.rs[j]) * m2[j]);
    gn_st_nt(dx + off, gn_pack8(o));
  };
  int r = tile * GN_TILE + L.rl;
  for (; r + L.rpp < r1; r += 2 * L.rpp) {
    uint4 vd[2], vx[2], vy[2], va[2];
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const long off = base + (long)(r + u * L.rpp) * C;
      vd[u] = gn_ld_nt(dy + off);
      vx[u] = gn_ld_nt(x + off);
      vy[u] = relu ? gn_ld_nt(y + off) : z;
      va[u] = addend ? gn_ld_nt(addend + off) : z;
    }
#pragma unroll
    for (int u = 0; u < 2; ++u) one(base + (long)(r + u * L.rpp) * C, vd[u], vx[u], vy[u], va[u]);
  }
  if (r < r1) {
    const long off = base + (long)r * C;
    one(off, gn_ld_nt(dy + off), gn_ld_nt(x + off), relu ? gn_ld_nt(y + off) : z,
        addend ? gn_ld_nt(addend + off) : z);
  }
}

// Resident backward, grid (1, slabs, N); dynamic LDS: [2][P][tpr] vectors,
// x then dy' (bf16, as dres stores it). cpart row n.
__global__ void __launch_bounds__(GN_THREADS) gn_bwd_resident_kernel(
    const bf16_t* __restrict__ dy, const bf16_t* __restrict__ addend, const bf16_t* __restrict__ y,
    const bf16_t* __restrict__ x, const float* __restrict__ mean, const float* __restrict__ rstd,
    const float* __restrict__ gamma, int P, int C, int Cg, int sw, int relu, bf16_t* __restrict__ dx,
    bf16_t* __restrict__ dres, float* __restrict__ cpart) {
  extern __shared__ uint4 gn_tile[];
  __shared__ float red[GN_RED];
  __shared__ float outc[2 * GN_MAX_SLAB];
  __shared__ float outg[GN_MAX_SLAB];
  const GnLane L = gn_lane(C, sw);
  const int n = blockIdx.z;
  const GnCoef k = gn_coef(L, n, C, Cg, mean, rstd, gamma);
  uint4* tx = gn_tile;
  uint4* td = gn_tile + P * L.tpr;
  float a[8], b[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) a[j] = b[j] = 0.f;
  const long base = (long)n * P * C + L.col;
  if (L.on) {
    const uint4 z = make_uint4(0, 0, 0, 0);
    auto row = [&](const int r, const uint4 vd, const uint4 vx, const uint4 vy, const uint4 va) {
      float fd[8], fx[8];
      gn_dyr(vd, va, vy, addend != nullptr, relu != 0, fd);
      const uint4 pk = gn_pack8(fd);
      if (dres) gn_st_nt(dres + base + (long)r * C, pk);
      gn_unpack8(pk, fd);
      tx[r * L.tpr + L.v] = vx;
      td[r * L.tpr + L.v] = pk;
      gn_unpack8(vx, fx);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        a[j] += fd[j];
        b[j] += fd[j] * ((fx[j] - k.mu[j]) * k.rs[j]);
      }
    };
    int r = L.rl;
    for (; r + L.rpp < P; r += 2 * L.rpp) {
      uint4 vd[2], vx[2], vy[2], va[2];
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const long off = base + (long)(r + u * L.rpp) * C;
        vd[u] = gn_ld_nt(dy + off);
        vx[u] = gn_ld_nt(x + off);
        vy[u] = relu ? gn_ld_nt(y + off) : z;
        va[u] = addend ? gn_ld_nt(addend + off) : z;
      }
#pragma unroll
      for (int u = 0; u < 2; ++u) row(r + u * L.rpp, vd[u], vx[u], vy[u], va[u]);
    }
    if (r < P) {
      const long off = base + (long)r * C;
      row(r, gn_ld_nt(dy + off), gn_ld_nt(x + off), relu ? gn_ld_nt(y + off) : z,
          addend ? gn_ld_nt(addend + off) : z);
    }
  }
  gn_channel_sums(b, a, L, red, outc);
  float* crow = cpart + (long)n * 2 * C;
  for (int e = threadIdx.x; e < 2 * L.cs; e += GN_THREADS) {
    const int q = e >= L.cs, c = e - q * L.cs;
    crow[q * C + L.c0 + c] = outc[e];
  }
  float ga[8], gb[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) { ga[j] = k.gm[j] * a[j]; gb[j] = k.gm[j] * b[j]; }
  gn_group_sums(ga, gb, L, Cg, red, outg);
  if (!L.on) return;
  const int ngs = L.cs / Cg;
  const float inv = 1.f / ((float)P * (float)Cg);
  float m1[8], m2[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int g = (L.v * 8 + j) / Cg;
    m1[j] = outg[g] * inv;
    m2[j] = outg[ngs + g] * inv;
  }
  for (int r = L.rl; r < P; r += L.rpp) {
    float fd[8], fx[8], o[8];
    gn_unpack8(td[r * L.tpr + L.v], fd);
    gn_unpack8(tx[r * L.tpr + L.v], fx);
#pragma unroll
    for (int j = 0; j < 8; ++j)
      o[j] = k.rs[j] * (k.gm[j] * fd[j] - m1[j] - ((fx[j] - k.mu[j]) * k.rs[j]) * m2[j]);
    gn_st_nt(dx + base + (long)r * C, gn_pack8(o));
  }
}

// ---------------------------------------------------------------- host
// 0 auto, 1 tiled, 2 resident wherever its tile fits (A/B runs and tests)
int g_gn_policy = 0;
TAM_KNOB(g_gn_policy)

int gn_slab(int C, int Cg) { return C <= 64 ? C : (Cg > 64 ? Cg : 64); }

// dynamic LDS one block of the current device may have next to this file's static arrays
long gn_lds_budget() {
  static long cached[64];
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return 0;
  if (cached[dev] == 0) {
    int v = 0;
    if (hipDeviceGetAttribute(&v, hipDeviceAttributeMaxSharedMemoryPerBlock, dev) != hipSuccess) v = 0;
    cached[dev] = v > GN_STATIC_LDS ? v - GN_STATIC_LDS : -1;
  }
  return cached[dev] > 0 ? cached[dev] : 0;
}

long gn_tile_bytes(int P, int C, int Cg, int backward) {
  return (long)P * gn_slab(C, Cg) * 2 * (backward ? 2 : 1);
}

// a kernel that asks for more than 64 KB of dynamic LDS opts in first (once per device)
template <class K>
void gn_opt_in(K kernel, long bytes, bool (&done)[64]) {
  if (bytes <= 64 * 1024) return;
  int dev = 0;
  TAM_HIP_CHECK(hipGetDevice(&dev));
  if (done[dev & 63]) return;
  TAM_HIP_CHECK(hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                    (int)gn_lds_budget()));
  done[dev & 63] = true;
}

// Auto policy, from tools/bench_gn.py at ResNet-50's batch-64 shapes
// (profiles/r7/groupnorm.md): the resident route won every shape whose staged
// tiles take <= 50 KB (forward 14x14 and 7x7: 6-25 KB, 1.2-1.6x; backward
// 14x14 / 7x7: 12-50 KB, 1.1-1.5x) and lost the 28x28 forward class (100 KB,
// one 4-wave block per CU: 404 us against 353 us over that class's layers).
// Nothing was measured between 50 and 100 KB; the line sits at 64 KB, where
// a CU still holds two blocks.
bool gn_auto_resident(int P, int C, int Cg, int backward) {
  return gn_tile_bytes(P, C, Cg, backward) <= 64 * 1024;
}

bool gn_use_resident(int P, int C, int G, int backward) {
  if (g_gn_policy == 1 || !gn_resident_fits(P, C, G, backward)) return false;
  return g_gn_policy == 2 || gn_auto_resident(P, C, C / G, backward);
}

}  // namespace

void gn_policy(int p) { g_gn_policy = p; }

bool gn_resident_fits(int P, int C, int G, int backward) {
  const long need = gn_tile_bytes(P, C, C / G, backward);
  return need <= gn_lds_budget();
}

void gn_forward(const bf16_t* x, const bf16_t* res, bf16_t* y, int N, int P, int C, int G, float eps,
                const float* gamma, const float* beta, float* mean, float* rstd, int relu, float* ws,
                hipStream_t s) {
  const int Cg = C / G, sw = gn_slab(C, Cg), slabs = (C + sw - 1) / sw;
  if (gn_use_resident(P, C, G, 0)) {
    static bool opted[64];
    const long bytes = gn_tile_bytes(P, C, Cg, 0);
    gn_opt_in(gn_fwd_resident_kernel, bytes, opted);
    hipLaunchKernelGGL(gn_fwd_resident_kernel, dim3(1, slabs, N), dim3(GN_THREADS), (size_t)bytes, s, x, res, y, P, C,
                       Cg, sw, gamma, beta, eps, relu, mean, rstd);
    return;
  }
  const int T = gn_tiles(P);
  float2* part = (float2*)ws;
  hipLaunchKernelGGL(gn_stats_kernel, dim3(T, slabs, N), dim3(GN_THREADS), 0, s, x, P, C, Cg, sw, part);
  hipLaunchKernelGGL(gn_finalize_kernel, dim3((N * G + GN_THREADS - 1) / GN_THREADS), dim3(GN_THREADS), 0, s, x,
                     (const float2*)part, P, C, Cg, T, N * G, eps, mean, rstd);
  hipLaunchKernelGGL(gn_apply_kernel, dim3(T, slabs, N), dim3(GN_THREADS), 0, s, x, res, y, P, C, Cg, sw,
                     (const float*)mean, (const float*)rstd, gamma, beta, relu);
}

int gn_backward(const bf16_t* dy, const bf16_t* addend, const bf16_t* y, const bf16_t* x, const float* mean,
                const float* rstd, const float* gamma, int N, int P, int C, int G, int relu, bf16_t* dx,
                bf16_t* dres, float* cpart, float* ws, hipStream_t s) {
  const int Cg = C / G, sw = gn_slab(C, Cg), slabs = (C + sw - 1) / sw;
  if (gn_use_resident(P, C, G, 1)) {
    static bool opted[64];
    const long bytes = gn_tile_bytes(P, C, Cg, 1);
    gn_opt_in(gn_bwd_resident_kernel, bytes, opted);
    hipLaunchKernelGGL(gn_bwd_resident_kernel, dim3(1, slabs, N), dim3(GN_THREADS), (size_t)bytes, s, dy, addend, y, x,
                       mean, rstd, gamma, P, C, Cg, sw, relu, dx, dres, cpart);
    return N;
  }
  const int T = gn_tiles(P);
  float2* gpart = (float2*)ws;
  float2* m12 = gpart + (long)N * T * G;
  hipLaunchKernelGGL(gn_bwd_stats_kernel, dim3(T, slabs, N), dim3(GN_THREADS), 0, s, dy, addend, y, x, mean, rstd,
                     gamma, P, C, Cg, sw, relu, dres, cpart, gpart);
  hipLaunchKernelGGL(gn_bwd_finalize_kernel, dim3((N * G + GN_THREADS - 1) / GN_THREADS), dim3(GN_THREADS), 0, s,
                     (const float2*)gpart, P, C, Cg, T, N * G, m12);
  if (dres) {
    // pass 1 stored dy' into dres: pass 2 is a plain backward over (dres, x)
    dy = dres;
    addend = nullptr;
    y = nullptr;
    relu = 0;
  }
  hipLaunchKernelGGL(gn_bwd_apply_kernel, dim3(T, slabs, N), dim3(GN_THREADS), 0, s, dy, addend, y, x, mean, rstd,
                     gamma, (const float2*)m12, P, C, Cg, sw, relu, dx);
  return N * T;
}

}  // namespace tam
