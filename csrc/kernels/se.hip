// tiresias_amd — Squeeze-and-Excitation (Hu et al. 2018) kernels, NHWC training.
//
// u [N][P = H*W][C] bf16 is a bottleneck's last norm output; the block computes
//   z = mean_p u            [N][C]   se_squeeze
//   h = relu(z W1^T + b1)   [N][Cr]  se_excite_fwd
//   s = sigmoid(h W2^T + b2)[N][C]
//   y = relu(s u + idn)              se_gate_fwd
// and backward, with g = (dy + addend) (y > 0):
//   ds = sum_p g u, didn = g         se_gate_bwd_reduce
//   dW1, db1, dW2, db2 (+=), dz      se_excite_bwd
//   du = s g + dz / P                se_gate_bwd_apply
// C % 8 == 0, C <= 2048, Cr % 8 == 0, 8 <= Cr <= 512 (checked by the caller).
//
// Streaming kernels (squeeze, gate reduce, the two gates): thread = (row lane,
// 16-B channel vector) of a channel slab, the vectors of a pixel adjacent in a
// wave, as in group_norm.hip. The reductions run over 64-channel slabs (128
// contiguous bytes per pixel) on two routes picked per kernel from P only,
// never from N:
//   * single pass: a block owns one (sample, slab) and all P pixels;
//   * tiled: SE_TILE-pixel tiles leave fp32 partials [N][tiles][C] that a
//     finalize sums in tile order.
// Row lanes fold through LDS in row-lane order. The gates run over 256-channel
// slabs (512 contiguous bytes per pixel); a thread keeps its 8 gate values in
// registers for all its pixels, so a block reads its s row once.
//
// The FCs and their gradients are six small GEMMs out[m][n] = sum_k A(m,k)
// B(n,k) on v_mfma_f32_16x16x32_bf16, one kernel (se_mma_kernel): a wave owns
// a 16 x 16 output tile and builds its fragments in registers from global
// memory -- fp32 operands (z, h, ds, dh) are rounded to bf16 there, dt = ds s
// (1 - s) is formed there, rows and k beyond the matrix are zeros there (no
// padded copies in memory). K runs over channels (FC1, dh: the block's 16
// waves split K and fold through LDS in wave order) or over the batch (dW1,
// dW2: a wave's own MFMA chain, samples in order). A launch carries up to
// three GEMMs and two fp32 column sums (db1, db2) as block ranges.
// No atomics anywhere: every output element has one owner, every sum a fixed
// order, and a sample's z, s, y never depend on its batch-mates.
#include "tam/common.h"
#include "tam/kernels.h"

namespace tam {
namespace {

constexpr int SE_THREADS = 256;
constexpr int SE_RED_SLAB = 64;      // channels of a reduction block
constexpr int SE_GATE_SLAB = 256;    // channels of a gate block
constexpr int SE_GATE_ROWS = 128;    // pixels of a gate block

typedef uint32_t se_u32x4_t __attribute__((ext_vector_type(4)));

__device__ __forceinline__ void se_unpack8(const uint4 v, float (&f)[8]) {
  const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    f[2 * i] = __uint_as_float(w[i] << 16);
    f[2 * i + 1] = __uint_as_float(w[i] & 0xffff0000u);
  }
}
__device__ __forceinline__ uint4 se_pack8(const float (&f)[8]) {
  return make_uint4(pack_bf2(f[0], f[1]), pack_bf2(f[2], f[3]), pack_bf2(f[4], f[5]), pack_bf2(f[6], f[7]));
}
__device__ __forceinline__ void se_st_nt(bf16_t* p, const uint4 v) {
  __builtin_nontemporal_store(se_u32x4_t{v.x, v.y, v.z, v.w}, (se_u32x4_t*)p);
}
__device__ __forceinline__ void se_ld8f(const float* p, float (&f)[8]) {
  const float4 a = *(const float4*)p, b = *(const float4*)(p + 4);
  f[0] = a.x; f[1] = a.y; f[2] = a.z; f[3] = a.w; f[4] = b.x; f[5] = b.y; f[6] = b.z; f[7] = b.w;
}

// a thread's place in its block: slab blockIdx.y of sw channels (the last one
// may be narrower), column vector v of the slab's tpr, row lane rl of rpp
struct SeLane {
  int c0, cs, tpr, rpp, v, rl, col;
  bool on;
};
__device__ __forceinline__ SeLane se_lane(int C, int sw) {
  SeLane L;
  L.c0 = blockIdx.y * sw;
  L.cs = min(sw, C - L.c0);
  L.tpr = L.cs / 8;
  L.rpp = SE_THREADS / L.tpr;
  L.v = threadIdx.x % L.tpr;
  L.rl = threadIdx.x / L.tpr;
  L.col = L.c0 + L.v * 8;
  L.on = L.rl < L.rpp;
  return L;
}

// ------------------------------------------------- squeeze / gate-backward reduce
// grid (tiles, slabs, N); a block sums rows [tile * tile_len, ...) of its slab.
// BWD = false: acc = sum u. BWD = true: g = (dy + addend) where y > 0, stored as
// bf16; acc = sum g u (the fp32 g). direct: out[n][c] = acc * scale (single
// pass), else out[n][tile][c] = acc (se_finalize_kernel sums the tiles).
template <bool BWD>
__global__ void __launch_bounds__(SE_THREADS) se_reduce_kernel(const bf16_t* __restrict__ u,
                                                               const bf16_t* __restrict__ dy,
                                                               const bf16_t* __restrict__ addend,
                                                               const bf16_t* __restrict__ y, bf16_t* __restrict__ g,
                                                               int P, int C, int tile_len, float scale, int direct,
                                                               float* __restrict__ out) {
  __shared__ float red[SE_THREADS * 8];
  const SeLane L = se_lane(C, SE_RED_SLAB);
  const int n = blockIdx.z, tile = blockIdx.x, T = gridDim.x;
  const long base = (long)n * P * C + L.col;
  float acc[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) acc[j] = 0.f;
  const int r1 = min(P, (tile + 1) * tile_len);
  if (L.on) {
    int r = tile * tile_len + L.rl;
    if constexpr (!BWD) {
      auto add = [&](const uint4 v) {
        float f[8];
        se_unpack8(v, f);
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[j] += f[j];
      };
      for (; r + 3 * L.rpp < r1; r += 4 * L.rpp) {
        uint4 v[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) v[q] = *(const uint4*)(u + base + (long)(r + q * L.rpp) * C);
#pragma unroll
        for (int q = 0; q < 4; ++q) add(v[q]);
      }
      for (; r < r1; r += L.rpp) add(*(const uint4*)(u + base + (long)r * C));
    } else {
      for (; r < r1; r += L.rpp) {
        const long o = base + (long)r * C;
        const uint4 vd = *(const uint4*)(dy + o), vy = *(const uint4*)(y + o), vu = *(const uint4*)(u + o);
        float fd[8], fy[8], fu[8];
        se_unpack8(vd, fd); se_unpack8(vy, fy); se_unpack8(vu, fu);
        if (addend) {
          float fa[8];
          se_unpack8(*(const uint4*)(addend + o), fa);
#pragma unroll
          for (int j = 0; j < 8; ++j) fd[j] += fa[j];
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          fd[j] = fy[j] > 0.f ? fd[j] : 0.f;
          acc[j] += fd[j] * fu[j];
        }
        *(uint4*)(g + o) = se_pack8(fd);
      }
    }
  }
  // row lanes fold through LDS, in row-lane order
  *(float4*)(red + threadIdx.x * 8) = make_float4(acc[0], acc[1], acc[2], acc[3]);
  *(float4*)(red + threadIdx.x * 8 + 4) = make_float4(acc[4], acc[5], acc[6], acc[7]);
  __syncthreads();
  for (int c = threadIdx.x; c < L.cs; c += SE_THREADS) {
    float t = 0.f;
    for (int j = 0; j < L.rpp; ++j) t += red[(j * L.tpr + (c >> 3)) * 8 + (c & 7)];
    if (direct) out[(long)n * C + L.c0 + c] = t * scale;
    else out[((long)n * T + tile) * C + L.c0 + c] = t;
  }
}

// out[n][c] = scale * sum_t part[n][t][c], tiles in order
__global__ void __launch_bounds__(SE_THREADS) se_finalize_kernel(const float* __restrict__ part, int T, int C,
                                                                 long total, float scale, float* __restrict__ out) {
  const long i = (long)blockIdx.x * SE_THREADS + threadIdx.x;
  if (i >= total) return;
  const long n = i / C;
  const int c = (int)(i - n * C);
  float t = 0.f;
  for (int k = 0; k < T; ++k) t += part[(n * T + k) * C + c];
  out[i] = t * scale;
}

// ------------------------------------------------------------------- the two gates
// grid (pixel chunks, slabs, N): out = s[n][c] * a (+ b) (+ cadd[n][c] * cscale),
// ReLU and a non-temporal store for the forward (a = u, b = idn, out = y); the
// backward apply is a = g, cadd = dz, cscale = 1 / P, out = du
__global__ void __launch_bounds__(SE_THREADS) se_gate_kernel(const bf16_t* __restrict__ a,
                                                             const bf16_t* __restrict__ b,
                                                             const float* __restrict__ s,
                                                             const float* __restrict__ cadd, float cscale, int fwd,
                                                             int P, int C, bf16_t* __restrict__ out) {
  const SeLane L = se_lane(C, SE_GATE_SLAB);
  if (!L.on) return;
  const int n = blockIdx.z;
  float sv[8], cv[8];
  se_ld8f(s + (long)n * C + L.col, sv);
#pragma unroll
  for (int j = 0; j < 8; ++j) cv[j] = 0.f;
  if (cadd) {
    se_ld8f(cadd + (long)n * C + L.col, cv);
#pragma unroll
    for (int j = 0; j < 8; ++j) cv[j] *= cscale;
  }
  const long base = (long)n * P * C + L.col;
  const int r1 = min(P, (int)(blockIdx.x + 1) * SE_GATE_ROWS);
  auto one = [&](int r, const uint4 va, const uint4 vb) {
    float fa[8], fb[8];
    se_unpack8(va, fa);
    se_unpack8(vb, fb);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      fa[j] = sv[j] * fa[j] + fb[j] + cv[j];
      if (fwd) fa[j] = fmaxf(fa[j], 0.f);
    }
    bf16_t* o = out + base + (long)r * C;
    if (fwd) se_st_nt(o, se_pack8(fa));
    else *(uint4*)o = se_pack8(fa);
  };
  const uint4 zero = make_uint4(0, 0, 0, 0);
  int r = blockIdx.x * SE_GATE_ROWS + L.rl;
  for (; r + L.rpp < r1; r += 2 * L.rpp) {
    const long o0 = base + (long)r * C, o1 = o0 + (long)L.rpp * C;
    const uint4 a0 = *(const uint4*)(a + o0), a1 = *(const uint4*)(a + o1);
    const uint4 b0 = b ? *(const uint4*)(b + o0) : zero, b1 = b ? *(const uint4*)(b + o1) : zero;
    one(r, a0, b0);
    one(r + L.rpp, a1, b1);
  }
  if (r < r1) {
    const long o0 = base + (long)r * C;
    one(r, *(const uint4*)(a + o0), b ? *(const uint4*)(b + o0) : zero);
  }
}

// --------------------------------------------------------- the excitation GEMMs
// Element (row, k) of an operand at row * sr + k * sk: bf16 (b), fp32 (f), or
// dt = f * f2 * (1 - f2) (ds and s, fp32). Rows >= rows and k >= K read as zero.
struct SeOperand {
  const float* f;
  const float* f2;
  const bf16_t* b;
  long sr, sk;
  int rows;
};
enum { SE_EPI_RELU = 0, SE_EPI_SIGMOID, SE_EPI_MASK, SE_EPI_STORE, SE_EPI_ACC };
// out[m][n] (row pitch ldo) from acc = sum_k A(m,k) B(n,k): relu / sigmoid(acc +
// bias[n]), acc where mask[m][n] > 0, acc, or out += acc
struct SeGemm {
  SeOperand A, B;
  int M, Nn, K, epi, ldo;
  const bf16_t* bias;
  const float* mask;
  float* out;
  int nt, ntiles, blk0;     // n tiles, all tiles, first block of the launch
};
// out[c] += sum_r v[r][c] in row order, v = f or dt as above (db1, db2)
struct SeColsum {
  const float* f;
  const float* f2;
  float* out;
  int rows, cols, blk0;
};
struct SeBatch {
  int ng, nc;
  SeGemm g[3];
  SeColsum c[2];
};

// 8 consecutive k of one operand row as a bf16 MFMA fragment. The loads are
// unconditional at clamped addresses and zeroed afterwards: no divergent branch
// between the loads of a K step
__device__ __forceinline__ bf16x8_t se_frag(const SeOperand& o, int row, int k, int K) {
  const bool ok = row < o.rows && k < K;
  const int kk = ok ? k : 0;
  const long at = (long)(ok ? row : 0) * o.sr + (long)kk * o.sk;
  float f[8], t[8];
  if (o.sk == 1) {                           // K % 8 == 0 on the contiguous routes
    if (o.b) {
      se_unpack8(*(const uint4*)(o.b + at), f);
    } else {
      se_ld8f(o.f + at, f);
      if (o.f2) se_ld8f(o.f2 + at, t);
    }
  } else {
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const long e = at + (long)(min(kk + i, K - 1) - kk) * o.sk;
      f[i] = o.b ? bf2f(o.b[e]) : o.f[e];
      if (o.f2) t[i] = o.f2[e];
    }
  }
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    if (o.f2) f[i] = f[i] * t[i] * (1.f - t[i]);
    f[i] = (ok && kk + i < K) ? f[i] : 0.f;
  }
  const uint4 p = se_pack8(f);
  return __builtin_bit_cast(bf16x8_t, p);
}

// KS = SE_KSPLIT: one tile per block of KS waves that split K; KS = 1: a tile
// per wave of a 4-wave block
constexpr int SE_KSPLIT = 16;
template <int KS>
__global__ void __launch_bounds__(KS > 1 ? 64 * KS : SE_THREADS) se_mma_kernel(const SeBatch bt) {
  __shared__ float red[KS > 1 ? 64 * KS * 4 : 4];
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int bid = blockIdx.x;
  for (int i = 0; i < bt.nc; ++i) {
    const SeColsum& cs = bt.c[i];
    const int nb = (cs.cols + SE_THREADS - 1) / SE_THREADS;
    if (bid < cs.blk0 || bid >= cs.blk0 + nb) continue;
    const int c = (bid - cs.blk0) * SE_THREADS + threadIdx.x;
    if (c < cs.cols) {
      float t = 0.f;
#pragma unroll 8
      for (int r = 0; r < cs.rows; ++r) {
        float v = cs.f[(long)r * cs.cols + c];
        if (cs.f2) {
          const float sg = cs.f2[(long)r * cs.cols + c];
          v = v * sg * (1.f - sg);
        }
        t += v;
      }
      cs.out[c] += t;
    }
    return;
  }
  int gi = 0;
  for (int i = 1; i < bt.ng; ++i)
    if (bid >= bt.g[i].blk0) gi = i;
  const SeGemm& p = bt.g[gi];
  constexpr int TN = KS > 1 ? 1 : 4;               // tiles per block
  const int tile = (bid - p.blk0) * TN + (KS > 1 ? 0 : wid);
  if (tile >= p.ntiles) return;                    // (whole block when KS > 1)
  const int m0 = (tile / p.nt) * 16, n0 = (tile % p.nt) * 16;
  const int ksteps = (p.K + 31) / 32, per = (ksteps + KS - 1) / KS;
  const int kb = (KS > 1 ? wid : 0) * per * 32, ke = min(p.K, kb + per * 32);
  // A / B fragment of 16x16x32: row = lane & 15, k = 8 * (lane >> 4) .. + 7
  const int fr = lane & 15, fk = 8 * (lane >> 4);
  f32x4_t acc = {0.f, 0.f, 0.f, 0.f};
  for (int k = kb; k < ke; k += 32)
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(se_frag(p.A, m0 + fr, k + fk, ke),
                                                  se_frag(p.B, n0 + fr, k + fk, ke), acc, 0, 0, 0);
  if constexpr (KS > 1) {
    *(f32x4_t*)(red + threadIdx.x * 4) = acc;
    __syncthreads();
    if (wid != 0) return;
    for (int w = 1; w < KS; ++w) acc += *(const f32x4_t*)(red + (w * 64 + lane) * 4);
  }
  // C map of 16x16x32: col = lane & 15 (n), row = 4 * (lane >> 4) + r (m)
  const int n = n0 + (lane & 15);
  if (n >= p.Nn) return;
  const float bv = p.bias ? bf2f(p.bias[n]) : 0.f;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int m = m0 + 4 * (lane >> 4) + r;
    if (m >= p.M) continue;
    float* o = p.out + (long)m * p.ldo + n;
    const float v = acc[r] + bv;
    switch (p.epi) {
      case SE_EPI_RELU: *o = fmaxf(v, 0.f); break;
      case SE_EPI_SIGMOID: *o = sigmoidf_(v); break;
      case SE_EPI_MASK: *o = p.mask[(long)m * p.ldo + n] > 0.f ? v : 0.f; break;
      case SE_EPI_STORE: *o = v; break;
      default: *o += v; break;
    }
  }
}

SeOperand se_f32(const float* f, const float* f2, long sr, long sk, int rows) {
  return SeOperand{f, f2, nullptr, sr, sk, rows};
}
SeOperand se_b16(const bf16_t* b, long sr, long sk, int rows) { return SeOperand{nullptr, nullptr, b, sr, sk, rows}; }

// appends a GEMM to the launch; returns the launch's block count so far
template <int KS>
int se_add_gemm(SeBatch& bt, int blocks, SeOperand A, SeOperand B, int M, int Nn, int K, int epi, float* out,
                const bf16_t* bias = nullptr, const float* mask = nullptr) {
  SeGemm& g = bt.g[bt.ng++];
  g.A = A; g.B = B; g.M = M; g.Nn = Nn; g.K = K; g.epi = epi; g.ldo = Nn;
  g.bias = bias; g.mask = mask; g.out = out;
  g.nt = (Nn + 15) / 16;
  g.ntiles = ((M + 15) / 16) * g.nt;
  g.blk0 = blocks;
  return KS > 1 ? blocks + g.ntiles : blocks + (g.ntiles + 3) / 4;
}
int se_add_colsum(SeBatch& bt, int blocks, const float* f, const float* f2, int rows, int cols, float* out) {
  bt.c[bt.nc++] = SeColsum{f, f2, out, rows, cols, blocks};
  return blocks + (cols + SE_THREADS - 1) / SE_THREADS;
}

int g_se_policy = 0;
TAM_KNOB(g_se_policy)
// measured (profiles/r7/se.md, batch 64): the squeeze is faster single-pass at
// every ResNet-50 shape (up to 3136 pixels); the backward reduce, with four
// streams per pixel, is faster single-pass at 784 pixels and tiled at 3136
constexpr int SE_SINGLE_MAX_P_FWD = 4096, SE_SINGLE_MAX_P_BWD = 1024;

bool se_single(int P, bool bwd) {
  if (g_se_policy == 1) return false;
  if (g_se_policy == 2) return true;
  return P <= (bwd ? SE_SINGLE_MAX_P_BWD : SE_SINGLE_MAX_P_FWD);
}

template <bool BWD>
void se_reduce(const bf16_t* u, const bf16_t* dy, const bf16_t* addend, const bf16_t* y, bf16_t* g, float* out,
               float* ws, int N, int P, int C, float scale, hipStream_t s) {
  const int slabs = (C + SE_RED_SLAB - 1) / SE_RED_SLAB;
  if (se_single(P, BWD)) {
    hipLaunchKernelGGL(se_reduce_kernel<BWD>, dim3(1, slabs, N), dim3(SE_THREADS), 0, s, u, dy, addend, y, g, P, C, P,
                       scale, 1, out);
    return;
  }
  const int T = se_tiles(P);
  hipLaunchKernelGGL(se_reduce_kernel<BWD>, dim3(T, slabs, N), dim3(SE_THREADS), 0, s, u, dy, addend, y, g, P, C,
                     SE_TILE, 1.f, 0, ws);
  const long total = (long)N * C;
  hipLaunchKernelGGL(se_finalize_kernel, dim3((unsigned)((total + SE_THREADS - 1) / SE_THREADS)), dim3(SE_THREADS), 0,
                     s, ws, T, C, total, scale, out);
}

void se_gate(const bf16_t* a, const bf16_t* b, const float* sg, const float* cadd, float cscale, int fwd, int N, int P,
             int C, bf16_t* out, hipStream_t s) {
  const dim3 grid((P + SE_GATE_ROWS - 1) / SE_GATE_ROWS, (C + SE_GATE_SLAB - 1) / SE_GATE_SLAB, N);
  hipLaunchKernelGGL(se_gate_kernel, grid, dim3(SE_THREADS), 0, s, a, b, sg, cadd, cscale, fwd, P, C, out);
}

}  // namespace

void se_policy(int p) { g_se_policy = (p == 1 || p == 2) ? p : 0; }
long se_reduce_ws(int N, int P, int C, int bwd) { return se_single(P, bwd != 0) ? 0 : (long)N * se_tiles(P) * C; }

void se_squeeze(const bf16_t* u, float* z, float* ws, int N, int P, int C, hipStream_t s) {
  se_reduce<false>(u, nullptr, nullptr, nullptr, nullptr, z, ws, N, P, C, 1.f / (float)P, s);
}

void se_excite_fwd(const float* z, const bf16_t* w1, const bf16_t* b1, const bf16_t* w2, const bf16_t* b2, float* h,
                   float* sg, int N, int C, int Cr, hipStream_t s) {
  // FC1: few output tiles over a long K = C: the block's waves split K.
  // FC2: many output tiles over K = Cr: a tile per wave
  SeBatch f1{}, f2{};
  const int nb1 = se_add_gemm<SE_KSPLIT>(f1, 0, se_f32(z, nullptr, C, 1, N), se_b16(w1, C, 1, Cr), N, Cr, C, SE_EPI_RELU, h, b1);
  hipLaunchKernelGGL(se_mma_kernel<SE_KSPLIT>, dim3(nb1), dim3(64 * SE_KSPLIT), 0, s, f1);
  const int nb2 =
      se_add_gemm<1>(f2, 0, se_f32(h, nullptr, Cr, 1, N), se_b16(w2, Cr, 1, C), N, C, Cr, SE_EPI_SIGMOID, sg, b2);
  hipLaunchKernelGGL(se_mma_kernel<1>, dim3(nb2), dim3(SE_THREADS), 0, s, f2);
}

void se_gate_fwd(const bf16_t* u, const float* sg, const bf16_t* idn, bf16_t* y, int N, int P, int C, hipStream_t s) {
  se_gate(u, idn, sg, nullptr, 0.f, 1, N, P, C, y, s);
}

void se_gate_bwd_reduce(const bf16_t* dy, const bf16_t* addend, const bf16_t* y, const bf16_t* u, bf16_t* g,
                        float* ds, float* ws, int N, int P, int C, hipStream_t s) {
  se_reduce<true>(u, dy, addend, y, g, ds, ws, N, P, C, 1.f, s);
}

void se_excite_bwd(const float* ds, const float* sg, const float* h, const float* z, const bf16_t* w1,
                   const bf16_t* w2, float* dh, float* dw1, float* db1, float* dw2, float* db2, float* dz, int N,
                   int C, int Cr, hipStream_t s) {
  // launch 1: dh[n][j] = (sum_c dt[n][c] W2[c][j]) (h > 0), K = C split over the waves
  SeBatch a{}, b{};
  const int nba = se_add_gemm<SE_KSPLIT>(a, 0, se_f32(ds, sg, C, 1, N), se_b16(w2, 1, Cr, Cr), N, Cr, C, SE_EPI_MASK, dh,
                                 nullptr, h);
  hipLaunchKernelGGL(se_mma_kernel<SE_KSPLIT>, dim3(nba), dim3(64 * SE_KSPLIT), 0, s, a);
  // launch 2: dz = dh W1 (K = Cr); dW1 += dh^T z and dW2 += dt^T h (K = the
  // batch, samples in order); db1 += colsum dh, db2 += colsum dt
  int nb = se_add_gemm<1>(b, 0, se_f32(dh, nullptr, Cr, 1, N), se_b16(w1, 1, C, C), N, C, Cr, SE_EPI_STORE, dz);
  nb = se_add_gemm<1>(b, nb, se_f32(dh, nullptr, 1, Cr, Cr), se_f32(z, nullptr, 1, C, C), Cr, C, N, SE_EPI_ACC, dw1);
  nb = se_add_gemm<1>(b, nb, se_f32(ds, sg, 1, C, C), se_f32(h, nullptr, 1, Cr, Cr), C, Cr, N, SE_EPI_ACC, dw2);
  nb = se_add_colsum(b, nb, dh, nullptr, N, Cr, db1);
  nb = se_add_colsum(b, nb, ds, sg, N, C, db2);
  hipLaunchKernelGGL(se_mma_kernel<1>, dim3(nb), dim3(SE_THREADS), 0, s, b);
}

void se_gate_bwd_apply(const bf16_t* g, const float* sg, const float* dz, bf16_t* du, int N, int P, int C,
                       hipStream_t s) {
  se_gate(g, nullptr, sg, dz, 1.f / (float)P, 0, N, P, C, du, s);
}

}  // namespace tam
