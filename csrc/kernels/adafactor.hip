// tiresias_amd — Adafactor over a job's flat parameter arena: the second
// moment of an R x C parameter is kept as R row means and C column means
// (Shazeer & Stern 2018, Algorithm 4 with beta1 = 0, the job's fixed lr, no
// relative step, no parameter scaling), so the optimizer state is O(R + C) per
// weight matrix. Trainer opt_dtype="factored".
//
// Contract (g^ = g * gscale, gscale including the clip scale; t the 1-based
// step, b2 = 1 - t^-0.8 formed on the host in double; e1 = 1e-30):
//   Rv_i = b2 Rv_i + (1 - b2) mean_j(g^_ij^2 + e1)
//   Cv_j = b2 Cv_j + (1 - b2) mean_i(g^_ij^2 + e1)
//   rfac_i = rsqrt(Rv_i / mean_i Rv_i),  cfac_j = rsqrt(Cv_j)
//   u_ij = g^_ij rfac_i cfac_j;  s = 1 / max(1, RMS(u)) per parameter
//   w -= lr (s u + wd w)         (wd = 0 from wd_until on)
// A parameter the host does not factor is the 1 x numel case of the same
// formulas (rfac = 1 exactly, Cv the plain second moment): one code path.
//
// Tables (host-built once, ops/arena.py adafactor_tables; every record is
// bound-checked on the device and a record that does not fit is skipped by
// every pass, nothing is read or written through it):
//   params int32 [nparam][8]  {offset, R, C, state offset, partial offset,
//                              first tile, tile count, 0}
//   tiles  int32 [ntiles][4]  {element offset, rows <= 32, cols <= 256, param}
//   tasks  int32 [ntasks][4]  {param, 0 rows / 1 columns, start, count <= 256}
// A parameter's state slice is [Rv (R) | Cv (C)] at its state offset; ``fac``
// has the same layout and holds rfac / cfac of the step. Its partials are
// row sums [column block][row] followed by column sums [row block][col].
//
// Six launches, no atomics, no host read; every sum has an order fixed by the
// tables alone, so a step is bitwise independent of the grid:
//   1 stats     blocks stride over tiles. A lane owns one 16-B column group,
//               a wave the rows w, w + 4, ... of the tile (8 loads in flight
//               per lane). Column sums are lane-local over the wave's rows,
//               then the four waves fold through LDS; row sums fold by wave
//               shuffles. fp32 partials per tile.
//   2 moments   one thread per row / column (task table): the partials across
//               tiles in fp64, in tile order, the EMA, Rv / Cv stored in fp32.
//   3 factors   one block per parameter: mean(Rv) in fp64, then rfac / cfac.
//   4 update^2  blocks stride over tiles: cfac of the lane's columns stays in
//               registers, rfac is read per row; the tile's sum of u^2 in
//               fp64 into the tile's slot.
//   5 clip      one wave per parameter: its slots in order -> {RMS(u), s}.
//   6 apply     blocks stride over tiles, u as in pass 4, non-temporal 16-B
//               accesses, bf16 shadow, gradient reset from zero_from on.
// g is read three times; only the last read is non-temporal.
// Skipped step (guard word / negative clip scale): passes 1-5 return, pass 6
// resets the gradient from zero_from on; nothing else is written.
#include <cmath>

#include "tam/common.h"
#include "tam/kernels.h"

namespace tam {

constexpr int kAfRows = 32, kAfCols = 256;   // 8192 elements, as kTrustTile
constexpr float kAfEps1 = 1e-30f;
int adafactor_tile_rows() { return kAfRows; }
int adafactor_tile_cols() { return kAfCols; }

namespace {

typedef unsigned af_u32x2_t __attribute__((ext_vector_type(2)));

struct AfDims {
  long n, nstate, npart;
  int nparam, ntiles;
};
struct AfParam {
  int off, R, C, soff, poff, first, ntiles;
  __device__ __forceinline__ long ntr() const { return ((long)R + kAfRows - 1) / kAfRows; }
  __device__ __forceinline__ long ntc() const { return ((long)C + kAfCols - 1) / kAfCols; }
};
struct AfTile {
  AfParam P;
  long base;   // arena index of the tile's first element (% 4 == 0)
  int r0, c0, rows, cols, param;
};

__device__ __forceinline__ bool af_skipped(const unsigned* guard, const float* clip) {
  return (guard != nullptr && *guard != 0u) || (clip != nullptr && clip[0] < 0.f);
}

__device__ __forceinline__ bool af_param(const int4* __restrict__ params, int p, const AfDims& d, AfParam& P) {
  if (p < 0 || p >= d.nparam) return false;
  const int4 a = params[2 * p], b = params[2 * p + 1];
  P.off = a.x; P.R = a.y; P.C = a.z; P.soff = a.w; P.poff = b.x; P.first = b.y; P.ntiles = b.z;
  if (P.off < 0 || (P.off & 63) || P.R < 1 || P.C < 1 || (P.R > 1 && (P.C & 3))) return false;
  const long numel = (long)P.R * P.C;
  if ((long)P.off + ((numel + 63) & ~63L) > d.n) return false;
  if (P.soff < 0 || (long)P.soff + P.R + P.C > d.nstate) return false;
  if (P.poff < 0 || (long)P.poff + P.ntc() * P.R + P.ntr() * P.C > d.npart) return false;
  return P.first >= 0 && (long)P.ntiles == P.ntr() * P.ntc() && (long)P.first + P.ntiles <= d.ntiles;
}

__device__ __forceinline__ bool af_tile(const int4* __restrict__ tiles, int t, const int4* __restrict__ params,
                                        const AfDims& d, AfTile& T) {
  const int4 tl = tiles[t];
  if (!af_param(params, tl.w, d, T.P)) return false;
  const AfParam& P = T.P;
  if (t < P.first || t >= P.first + P.ntiles || tl.x < P.off) return false;
  const int rel = tl.x - P.off;
  T.base = tl.x; T.r0 = rel / P.C; T.c0 = rel % P.C; T.rows = tl.y; T.cols = tl.z; T.param = tl.w;
  return (T.r0 % kAfRows) == 0 && (T.c0 % kAfCols) == 0 && T.rows >= 1 && T.rows <= kAfRows && T.cols >= 1 &&
         T.cols <= kAfCols && T.r0 + T.rows <= P.R && T.c0 + T.cols <= P.C;
}

// the update direction; passes 4 and 6 both call it on the same values
__device__ __forceinline__ float af_u(float g, float gscale, float rf, float cf) { return ((g * gscale) * rf) * cf; }

// this lane's rows of a tile: row r = wave + 4 u, column group 4 lane .. + 3.
// Groups past the tile's columns and rows past its rows read nothing (0). A
// ragged last group (1 x n parameters only) reads into the parameter's padding
template <bool NT>
__device__ __forceinline__ void af_load(const float* __restrict__ p, const AfTile& T, int wv, int lane,
                                        float4 (&v)[kAfRows / 4]) {
#pragma unroll
  for (int u = 0; u < kAfRows / 4; ++u) {
    const int r = wv + 4 * u;
    v[u] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (r < T.rows && 4 * lane < T.cols) {
      const f32x4_t* a = (const f32x4_t*)(p + T.base + (long)r * T.P.C + 4 * lane);
      const f32x4_t x = NT ? __builtin_nontemporal_load(a) : *a;
      v[u] = make_float4(x[0], x[1], x[2], x[3]);
    }
  }
}

__device__ __forceinline__ void af_cfac(const float* __restrict__ fac, const AfTile& T, int lane, float (&cf)[4]) {
#pragma unroll
  for (int k = 0; k < 4; ++k)
    cf[k] = 4 * lane + k < T.cols ? fac[(long)T.P.soff + T.P.R + T.c0 + 4 * lane + k] : 0.f;
}

__global__ void __launch_bounds__(256) af_stats_kernel(const float* __restrict__ g, const int4* __restrict__ tiles,
                                                        const int4* __restrict__ params, AfDims d, float gscale,
                                                        float* __restrict__ partials, const unsigned* guard,
                                                        const float* clip) {
  if (af_skipped(guard, clip)) return;
  if (clip != nullptr) gscale *= clip[0];
  __shared__ __align__(16) float csum[2][4][kAfCols];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  int par = 0;
  for (int t = blockIdx.x; t < d.ntiles; t += gridDim.x) {
    AfTile T;
    if (!af_tile(tiles, t, params, d, T)) continue;   // (uniform over the block)
    const AfParam& P = T.P;
    float4 gv[kAfRows / 4];
    af_load<false>(g, T, wv, lane, gv);   // ordinary loads: passes 4 and 6 read the same bytes
    float ca[4] = {0.f, 0.f, 0.f, 0.f};
    float* rowp = partials + (long)P.poff + (long)(T.c0 / kAfCols) * P.R + T.r0;
#pragma unroll
    for (int u = 0; u < kAfRows / 4; ++u) {
      const int r = wv + 4 * u;
      if (r >= T.rows) continue;   // (uniform over the wave)
      const float* gp = (const float*)&gv[u];
      float rs = 0.f;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        if (4 * lane + k >= T.cols) continue;
        const float gh = gp[k] * gscale;
        const float v = __builtin_fmaf(gh, gh, kAfEps1);
        ca[k] += v;
        rs += v;
      }
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) rs += __shfl_down(rs, o, 64);
      if (lane == 0) rowp[r] = rs;
    }
    *(float4*)&csum[par][wv][4 * lane] = make_float4(ca[0], ca[1], ca[2], ca[3]);
    __syncthreads();
    const int c = threadIdx.x;
    if (c < T.cols)
      partials[(long)P.poff + P.ntc() * P.R + (long)(T.r0 / kAfRows) * P.C + T.c0 + c] =
          (csum[par][0][c] + csum[par][1][c]) + (csum[par][2][c] + csum[par][3][c]);
    par ^= 1;   // the next tile fills the other buffer: one barrier per tile
  }
}

__global__ void __launch_bounds__(256) af_moments_kernel(const float* __restrict__ partials,
                                                          const int4* __restrict__ tasks, int ntasks,
                                                          const int4* __restrict__ params, AfDims d, float b2,
                                                          float* __restrict__ state, const unsigned* guard,
                                                          const float* clip) {
  if (af_skipped(guard, clip)) return;
  for (int k = blockIdx.x; k < ntasks; k += gridDim.x) {
    const int4 tk = tasks[k];   // {param, rows / columns, start, count}
    AfParam P;
    if (!af_param(params, tk.x, d, P)) continue;
    const bool col = tk.y != 0;
    if ((tk.y != 0 && tk.y != 1) || tk.z < 0 || tk.w < 1 || tk.w > 256 || (long)tk.z + tk.w > (col ? P.C : P.R))
      continue;
    if ((int)threadIdx.x >= tk.w) continue;
    const int i = tk.z + threadIdx.x;
    const long nb = col ? P.ntr() : P.ntc(), stride = col ? P.C : P.R;
    const float* src = partials + (long)P.poff + (col ? P.ntc() * P.R : 0) + i;
    // 16 loads in flight (an embedding has ~1000 row blocks), added in tile order
    double s = 0.;
    for (long b0 = 0; b0 < nb; b0 += 16) {
      float x[16];
#pragma unroll
      for (int q = 0; q < 16; ++q) x[q] = b0 + q < nb ? src[(b0 + q) * stride] : 0.f;
#pragma unroll
      for (int q = 0; q < 16; ++q) s += (double)x[q];
    }
    const float mean = (float)(s / (double)(col ? P.R : P.C));
    float* dst = state + (long)P.soff + (col ? P.R : 0) + i;
    *dst = __builtin_fmaf(b2, *dst, (1.f - b2) * mean);
  }
}

__global__ void __launch_bounds__(256) af_factors_kernel(const float* __restrict__ state,
                                                          const int4* __restrict__ params, AfDims d,
                                                          float* __restrict__ fac, const unsigned* guard,
                                                          const float* clip) {
  if (af_skipped(guard, clip)) return;
  AfParam P;
  if (!af_param(params, blockIdx.x, d, P)) return;
  const float* rv = state + P.soff;
  double a = 0.;
  for (int i = threadIdx.x; i < P.R; i += 256) a += (double)rv[i];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) a += __shfl_down(a, o, 64);
  __shared__ double red[4];
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = a;
  __syncthreads();
  const double mean = ((red[0] + red[1]) + (red[2] + red[3])) / (double)P.R;
  for (int i = threadIdx.x; i < P.R; i += 256) fac[P.soff + i] = (float)(1. / sqrt((double)rv[i] / mean));
  for (int j = threadIdx.x; j < P.C; j += 256)
    fac[(long)P.soff + P.R + j] = (float)(1. / sqrt((double)rv[(long)P.R + j]));
}

__global__ void __launch_bounds__(256) af_usq_kernel(const float* __restrict__ g, const float* __restrict__ fac,
                                                      const int4* __restrict__ tiles,
                                                      const int4* __restrict__ params, AfDims d, float gscale,
                                                      double* __restrict__ tslots, const unsigned* guard,
                                                      const float* clip) {
  if (af_skipped(guard, clip)) return;
  if (clip != nullptr) gscale *= clip[0];
  __shared__ double red[2][4];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  int par = 0;
  for (int t = blockIdx.x; t < d.ntiles; t += gridDim.x, par ^= 1) {
    AfTile T;
    double acc = 0.;
    if (af_tile(tiles, t, params, d, T)) {
      float cf[4];
      af_cfac(fac, T, lane, cf);
      float4 gv[kAfRows / 4];
      af_load<false>(g, T, wv, lane, gv);
#pragma unroll
      for (int u = 0; u < kAfRows / 4; ++u) {
        const int r = wv + 4 * u;
        if (r >= T.rows) continue;
        const float rf = fac[T.P.soff + T.r0 + r];
        const float* gp = (const float*)&gv[u];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const float uu = af_u(gp[k], gscale, rf, cf[k]);   // (0 past the tile's columns: g = cfac = 0)
          acc = fma((double)uu, (double)uu, acc);
        }
      }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_down(acc, o, 64);
    if (lane == 0) red[par][wv] = acc;
    __syncthreads();
    if (threadIdx.x == 0) tslots[t] = (red[par][0] + red[par][1]) + (red[par][2] + red[par][3]);
  }
}

__global__ void __launch_bounds__(64) af_clip_kernel(const double* __restrict__ tslots,
                                                      const int4* __restrict__ params, AfDims d,
                                                      float* __restrict__ urms, const unsigned* guard,
                                                      const float* clip) {
  if (af_skipped(guard, clip)) return;
  AfParam P;
  if (!af_param(params, blockIdx.x, d, P)) return;
  double a = 0.;
  for (int t = P.first + (int)threadIdx.x; t < P.first + P.ntiles; t += 64) a += tslots[t];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) a += __shfl_down(a, o, 64);
  if (threadIdx.x == 0) {
    const double rms = sqrt(a / ((double)P.R * (double)P.C));
    urms[2 * blockIdx.x] = (float)rms;
    urms[2 * blockIdx.x + 1] = (float)(1. / fmax(1., rms));
  }
}

__global__ void __launch_bounds__(256) af_apply_kernel(float* __restrict__ w, float* __restrict__ g,
                                                        bf16_t* __restrict__ wb, const float* __restrict__ fac,
                                                        const float* __restrict__ urms,
                                                        const int4* __restrict__ tiles,
                                                        const int4* __restrict__ params, AfDims d, float lr,
                                                        float wd0, float gscale, long zero_from4, long wd_until,
                                                        const unsigned* guard, const float* clip) {
  const f32x4_t zero = {0.f, 0.f, 0.f, 0.f};
  if (af_skipped(guard, clip)) {
    const long n4 = d.n / 4;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n4; i += (long)gridDim.x * blockDim.x)
      if (i >= zero_from4) __builtin_nontemporal_store(zero, (f32x4_t*)g + i);
    return;
  }
  if (clip != nullptr) gscale *= clip[0];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  for (int t = blockIdx.x; t < d.ntiles; t += gridDim.x) {
    AfTile T;
    if (!af_tile(tiles, t, params, d, T)) continue;
    const float s = urms[2 * T.param + 1];
    const float wd = T.base < wd_until ? wd0 : 0.f;
    float cf[4];
    af_cfac(fac, T, lane, cf);
    float4 wv4[kAfRows / 4], gv[kAfRows / 4];
    af_load<true>(w, T, wv, lane, wv4);
    af_load<true>(g, T, wv, lane, gv);
    if (4 * lane >= T.cols) continue;
#pragma unroll
    for (int u = 0; u < kAfRows / 4; ++u) {
      const int r = wv + 4 * u;
      if (r >= T.rows) continue;
      const float rf = fac[T.P.soff + T.r0 + r];
      float* wp = (float*)&wv4[u];
      const float* gp = (const float*)&gv[u];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const float upd = __builtin_fmaf(wd, wp[k], s * af_u(gp[k], gscale, rf, cf[k]));
        wp[k] = __builtin_fmaf(-lr, upd, wp[k]);
      }
      const long i4 = (T.base + (long)r * T.P.C + 4 * lane) / 4;
      __builtin_nontemporal_store(f32x4_t{wp[0], wp[1], wp[2], wp[3]}, (f32x4_t*)w + i4);
      if (i4 >= zero_from4) __builtin_nontemporal_store(zero, (f32x4_t*)g + i4);
      __builtin_nontemporal_store(af_u32x2_t{pack_bf2(wp[0], wp[1]), pack_bf2(wp[2], wp[3])}, (af_u32x2_t*)wb + i4);
    }
  }
}

}  // namespace

void adafactor_step(float* w, float* g, float* state, float* fac, bf16_t* wb, long n, long nstate, float lr,
                    float wd, int step, float gscale, const int* params, int nparam, const int* tiles, int ntiles,
                    const int* tasks, int ntasks, float* partials, long npart, double* tslots, float* urms,
                    hipStream_t s, const unsigned* guard, long zero_from, long wd_until, const float* clip) {
  if (n <= 0) return;
  const float b2 = (float)(1.0 - pow((double)step, -0.8));
  const AfDims d{n, nstate, npart, nparam, ntiles};
  const int4* pr = (const int4*)params;
  const int4* tl = (const int4*)tiles;
  // tiled passes: 8 blocks per block of the optimizer's cap. A block has one
  // tile (8 loads per lane) in flight between barriers, so one block per CU
  // leaves the passes latency-bound (measured, profiles/r7/adafactor.md)
  const long cap = 8L * optim_tile_grid(1 << 30);
  const dim3 grid((unsigned)(ntiles < cap ? (ntiles < 1 ? 1 : ntiles) : cap)), pgrid(nparam < 1 ? 1 : nparam);
  hipLaunchKernelGGL(af_stats_kernel, grid, dim3(256), 0, s, g, tl, pr, d, gscale, partials, guard, clip);
  hipLaunchKernelGGL(af_moments_kernel, dim3(optim_tile_grid(ntasks)), dim3(256), 0, s, partials, (const int4*)tasks,
                     ntasks, pr, d, b2, state, guard, clip);
  hipLaunchKernelGGL(af_factors_kernel, pgrid, dim3(256), 0, s, state, pr, d, fac, guard, clip);
  hipLaunchKernelGGL(af_usq_kernel, grid, dim3(256), 0, s, g, fac, tl, pr, d, gscale, tslots, guard, clip);
  hipLaunchKernelGGL(af_clip_kernel, pgrid, dim3(64), 0, s, tslots, pr, d, urms, guard, clip);
  hipLaunchKernelGGL(af_apply_kernel, grid, dim3(256), 0, s, w, g, wb, fac, urms, tl, pr, d, lr, wd, gscale,
                     zero_from / 4, wd_until < 0 ? n : wd_until, guard, clip);
}

}  // namespace tam
