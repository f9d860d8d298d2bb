// Grouped 3x3 convolution (ResNeXt bottlenecks): bf16 NHWC, pad 1, stride 1 or
// 2, K == C, weights [C][3][3][Cg] with Cg = C / groups in {4, 8, 16, 32}.
//
// A slab of Wd = max(16, Cg) consecutive channels holds whole groups and reads
// only itself, so the layer is C / Wd independent dense Wd -> Wd 3x3 convs. With
// a block-diagonal Wd x Wd weight per tap these are v_mfma_f32_16x16x32_bf16
// shaped: at Wd = 16 one MFMA covers two taps (K = 2 x 16 channels), at Wd = 32
// one tap. At Cg = 4 / 8 the MFMA multiplies zeros 4x / 2x over: the pass is
// bound by how the activations move, not by the MFMA rate.
//
// Forward / data gradient (gconv_kernel): a block owns a spatial tile of output
// pixels x a chunk of up to 64 channels (128 B per pixel: full lines), stages
// the input patch with its halo in LDS once, and each wave takes a slab of the
// chunk. The slab's packed weights sit in registers as MFMA A fragments (M =
// output channel), the B fragments (N = 16 pixels of one tile row) are 16-B
// reads of the patch at the tap offsets: no im2col. A lane ends up with four
// consecutive channels of one pixel. Three geometries:
//   S1   stride 1 (the stride-1 data gradient is this one on the mirrored,
//        transposed weight image),
//   S2   stride-2 forward: patch columns stored split by parity, so the 16
//        pixels of a row tile are consecutive LDS rows at every tap,
//   DG2  stride-2 data gradient: the dx pixels of a row tile share their (h & 1,
//        w & 1) parity, hence their valid taps (1 / 2 / 2 / 4 of the nine): a
//        dense read of the dy patch, no zero-dilated math.
// Weight gradient (gconv_wgrad_kernel): the reduction runs over pixels, so dy
// and x fragments are transposed LDS reads (ds_read_b64_tr_b16) of the dy tile
// and the x patch; a slab's nine Wd x Wd fp32 tiles stay in registers while a
// persistent block walks its fixed list of spatial tiles, then leave as one
// partial. gconv_wgrad_reduce_kernel sums the partials in order, keeps the
// diagonal blocks and accumulates into dw. No atomics anywhere.
#include "tam/common.h"
#include "tam/igemm.h"
#include "tam/launch.h"

namespace tam {
namespace {

enum { GC_S1 = 0, GC_S2 = 1, GC_DG2 = 2 };

// LDS images: 128-B pixel rows; 16-B granule c of row L sits at c ^ swz(L), the
// MN-major image's swizzle (igemm.h), so the transposed reads below apply
__device__ __forceinline__ int gc_off(int L, int c16) {
  return L * 128 + ((c16 ^ (mnmaj_swz<64>(L) >> 1)) << 4);
}

// Tile geometry. TH x 16 MFMA row tiles per block; the staged patch is PR x PC
// input pixels from origin org(tile row) / org(tile col); lmap is a patch
// pixel's LDS row, base(r) + j the LDS row of row tile r's pixel j at tap
// offset 0, tapoff(t) what tap t = dh * 3 + dw (forward sense) adds to it.
template <int MODE>
struct GcGeo;
template <>
struct GcGeo<GC_S1> {
  static constexpr int TH = 8, PR = 10, PC = 18, NPX = 180, NCLS = 1;
  __device__ static int org(int t0) { return t0 - 1; }
  __device__ static int lmap(int pr, int pc) { return pr * 18 + pc; }
  __device__ static int base(int r) { return r * 18; }
  __device__ static constexpr int tapoff(int t) { return (t / 3) * 18 + t % 3; }
};
template <>
struct GcGeo<GC_S2> {
  // columns split by parity: even columns 0, 2, .., 32 at 0..16, odd at 17..32
  static constexpr int TH = 4, PR = 9, PC = 33, NPX = 9 * 34, NCLS = 1;
  __device__ static int org(int t0) { return 2 * t0 - 1; }
  __device__ static int lmap(int pr, int pc) { return pr * 34 + (pc & 1) * 17 + (pc >> 1); }
  __device__ static int base(int r) { return 2 * r * 34; }
  __device__ static constexpr int tapoff(int t) { return (t / 3) * 34 + ((t % 3) & 1) * 17 + ((t % 3) >> 1); }
};
template <>
struct GcGeo<GC_DG2> {
  // dx tile 8 x 32 = TH x 16 quads; dy patch rows a0 .. a0 + 4, columns b0 .. b0 + 16.
  // dx row 2a + ph takes dy row a at dh = 1 (ph = 0), a + 1 at dh = 0 and a at dh = 2 (ph = 1)
  static constexpr int TH = 4, PR = 5, PC = 17, NPX = 85, NCLS = 4;
  __device__ static int org(int t0) { return t0; }
  __device__ static int lmap(int pr, int pc) { return pr * 17 + pc; }
  __device__ static int base(int r) { return r * 17; }
  __device__ static constexpr int tapoff(int t) { return (t / 3 == 0 ? 17 : 0) + (t % 3 == 0 ? 1 : 0); }
};

// The ten K slots of a pass (two per Wd = 16 MFMA, one per Wd = 32 MFMA): the
// tap in slot i (-1: none, a zero fragment) and the parity class that slot
// pair i >> 1 serves. DG2: class ph * 2 + pw has taps dh = 1 - ph (mod 2), dw alike
template <int MODE>
__device__ __forceinline__ constexpr int gc_tap(int i) {
  if (MODE != GC_DG2) return i < 9 ? i : -1;
  switch (i) {
    case 0: return 4;
    case 2: return 3;
    case 3: return 5;
    case 4: return 1;
    case 5: return 7;
    case 6: return 0;
    case 7: return 2;
    case 8: return 6;
    case 9: return 8;
    default: return -1;
  }
}
template <int MODE>
__device__ __forceinline__ constexpr int gc_cls(int i) {
  return MODE != GC_DG2 ? 0 : (i < 8 ? i >> 1 : 3);
}

struct GcArgs {
  const bf16_t* in;    // [N][Hi][Wi][C]
  bf16_t* out;         // [N][Ho][Wo][C]
  const bf16_t* wpk;   // [C / Wd][9][Wd][Wd] packed image of the pass
  const bf16_t* mask;  // optional, out's shape: store only where mask > 0
  int N, Hi, Wi, Ho, Wo, C, th, tw;
};

// stage the PR x PC patch of `in` around tile (thi, twi) of sample n, channels
// cb .. cb + cw, zero outside the image and past the chunk
template <class G>
__device__ __forceinline__ void gc_stage(char* patch, const bf16_t* in, int n, int Hi, int Wi, int C, int ih0, int iw0,
                                         int cb, int cw, int tid) {
  for (int idx = tid; idx < G::PR * G::PC * 8; idx += 256) {
    const int e = idx >> 3, c = idx & 7;
    const int pr = e / G::PC, pc = e % G::PC;
    const int ih = ih0 + pr, iw = iw0 + pc;
    uint4 v = make_uint4(0u, 0u, 0u, 0u);
    if ((unsigned)ih < (unsigned)Hi && (unsigned)iw < (unsigned)Wi && 8 * c < cw)
      v = *(const uint4*)(in + (((long)n * Hi + ih) * Wi + iw) * C + cb + 8 * c);
    *(uint4*)(patch + gc_off(G::lmap(pr, pc), c)) = v;
  }
}

template <int WD, int MODE>
__global__ void __launch_bounds__(256) gconv_kernel(GcArgs a) {
  using G = GcGeo<MODE>;
  constexpr int SL = 64 / WD, RP = 4 / SL, MT = WD / 16;
  constexpr int NSTEP = WD == 16 ? 5 : 10;
  __shared__ __attribute__((aligned(128))) char patch[G::NPX * 128];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, g = lane >> 4, j = lane & 15;
  int tile = blockIdx.x;
  const int twi = tile % a.tw;
  tile /= a.tw;
  const int thi = tile % a.th, n = tile / a.th;
  const int cb = blockIdx.y * 64;
  const int cw = a.C - cb < 64 ? a.C - cb : 64;
  gc_stage<G>(patch, a.in, n, a.Hi, a.Wi, a.C, G::org(thi * G::TH), G::org(twi * 16), cb, cw, tid);

  // this wave's slab of the chunk, and its share of the row tiles
  const int slot = w % SL, part = w / SL;
  const bool active = slot * WD < cw;
  const s16x8_t zero8 = {0, 0, 0, 0, 0, 0, 0, 0};
  s16x8_t wf[NSTEP][MT];
  if (active) {
    const bf16_t* wp = a.wpk + (long)(cb / WD + slot) * 9 * WD * WD;
#pragma unroll
    for (int s = 0; s < NSTEP; ++s) {
      int tap, kin;
      if (WD == 16) {
        tap = (g >> 1) ? gc_tap<MODE>(2 * s + 1) : gc_tap<MODE>(2 * s);
        kin = 8 * (g & 1);
      } else {
        tap = gc_tap<MODE>(s);
        kin = 8 * g;
      }
      // (the data-gradient image is tap-mirrored: DG2 names taps in the forward sense)
      const int ti = tap < 0 ? 0 : (MODE == GC_DG2 ? 8 - tap : tap);
#pragma unroll
      for (int mt = 0; mt < MT; ++mt)
        wf[s][mt] = tap < 0 ? zero8 : *(const s16x8_t*)(wp + ((long)ti * WD + 16 * mt + j) * WD + kin);
    }
  }
  __syncthreads();
  if (!active) return;
  const int c16 = slot * (WD / 8) + (WD == 16 ? (g & 1) : g);

  for (int r = part; r < G::TH; r += RP) {
#pragma unroll
    for (int cls = 0; cls < G::NCLS; ++cls) {
      f32x4_t acc[MT];
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) acc[mt] = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int s = 0; s < NSTEP; ++s) {
        const int i0 = WD == 16 ? 2 * s : s;
        if (gc_cls<MODE>(i0) != cls || gc_tap<MODE>(i0) < 0) continue;
        int off = G::tapoff(gc_tap<MODE>(i0));
        bool live = true;
        if (WD == 16 && (g >> 1)) {
          if (gc_tap<MODE>(i0 + 1) < 0) live = false;
          else off = G::tapoff(gc_tap<MODE>(i0 + 1));
        }
        s16x8_t xb = *(const s16x8_t*)(patch + gc_off(G::base(r) + j + off, c16));
        if (!live) xb = zero8;
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
          acc[mt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, wf[s][mt]),
                                                            __builtin_bit_cast(bf16x8_t, xb), acc[mt], 0, 0, 0);
      }
      // lane (g, j): channels 4g .. 4g + 3 of M tile mt, pixel j of the row tile
      int oh = thi * G::TH + r, ow = twi * 16 + j;
      if (MODE == GC_DG2) {
        oh = 2 * oh + (cls >> 1);
        ow = 2 * ow + (cls & 1);
      }
      if (oh < a.Ho && ow < a.Wo) {
        const long o = (((long)n * a.Ho + oh) * a.Wo + ow) * a.C + cb + slot * WD + 4 * g;
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
          float v0 = acc[mt][0], v1 = acc[mt][1], v2 = acc[mt][2], v3 = acc[mt][3];
          if (a.mask != nullptr) {
            const uint2 m = *(const uint2*)(a.mask + o + 16 * mt);
            v0 = bf2f((bf16_t)(m.x & 0xffffu)) > 0.f ? v0 : 0.f;
            v1 = bf2f((bf16_t)(m.x >> 16)) > 0.f ? v1 : 0.f;
            v2 = bf2f((bf16_t)(m.y & 0xffffu)) > 0.f ? v2 : 0.f;
            v3 = bf2f((bf16_t)(m.y >> 16)) > 0.f ? v3 : 0.f;
          }
          *(uint2*)(a.out + o + 16 * mt) = make_uint2(pack_bf2(v0, v1), pack_bf2(v2, v3));
        }
      }
    }
  }
}

// transposed fragment of a 128-B-row LDS image: this lane group's 8 rows start
// at rbase; the lane receives column colbase + (lane & 15), element e = row
// rbase + e (conv_dma.h wc_frag's form)
__device__ __forceinline__ s16x8_t gc_frag_tr(const char* img, int lane, int rbase, int colbase) {
  const int t = lane & 15, q = t >> 2, p = t & 3;
  const int c8 = (colbase >> 2) + p;
  s16x4_t lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(img + mnmaj_off<64>(rbase + q, c8)));
  s16x4_t hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(img + mnmaj_off<64>(rbase + q + 4, c8)));
  s16x8_t r;
  r[0] = lo[0]; r[1] = lo[1]; r[2] = lo[2]; r[3] = lo[3];
  r[4] = hi[0]; r[5] = hi[1]; r[6] = hi[2]; r[7] = hi[3];
  return r;
}

struct GwArgs {
  const bf16_t* dy;   // [N][P][Q][C]
  const bf16_t* x;    // [N][H][W][C]
  float* ws;          // [chunks][gridDim.x * RP][64 / Wd][9][Wd][Wd] partials
  int N, H, W, P, Q, C, th, tw, ntiles;
};

template <int WD, int STRIDE>
__global__ void __launch_bounds__(256, 1) gconv_wgrad_kernel(GwArgs a) {
  using G = GcGeo<STRIDE == 1 ? GC_S1 : GC_S2>;
  constexpr int SL = 64 / WD, RP = 4 / SL, MT = WD / 16;
  constexpr int RUNS = G::TH * 16 / 32;       // 32-pixel reduction runs (two tile rows) per tile
  __shared__ __attribute__((aligned(128))) char patch[G::NPX * 128];
  __shared__ __attribute__((aligned(128))) char dyt[G::TH * 16 * 128];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, g = lane >> 4, j = lane & 15;
  const int cb = blockIdx.y * 64;
  const int cw = a.C - cb < 64 ? a.C - cb : 64;
  const int slot = w % SL, part = w / SL;
  const bool active = slot * WD < cw;
  f32x4_t acc[9][MT][MT];
#pragma unroll
  for (int t = 0; t < 9; ++t)
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
      for (int nt = 0; nt < MT; ++nt) acc[t][mt][nt] = f32x4_t{0.f, 0.f, 0.f, 0.f};

  // this block's tiles: blockIdx.x, + gridDim.x, ... -- fixed by the shape alone
  for (int tile = blockIdx.x; tile < a.ntiles; tile += gridDim.x) {
    const int twi = tile % a.tw, rest = tile / a.tw;
    const int thi = rest % a.th, n = rest / a.th;
    __syncthreads();                 // every wave is done with the last tile's images
    gc_stage<G>(patch, a.x, n, a.H, a.W, a.C, G::org(thi * G::TH), G::org(twi * 16), cb, cw, tid);
    for (int idx = tid; idx < G::TH * 16 * 8; idx += 256) {
      const int e = idx >> 3, c = idx & 7;
      const int oh = thi * G::TH + (e >> 4), ow = twi * 16 + (e & 15);
      uint4 v = make_uint4(0u, 0u, 0u, 0u);
      if (oh < a.P && ow < a.Q && 8 * c < cw)
        v = *(const uint4*)(a.dy + (((long)n * a.P + oh) * a.Q + ow) * a.C + cb + 8 * c);
      *(uint4*)(dyt + gc_off(e, c)) = v;
    }
    __syncthreads();
    if (!active) continue;
    for (int run = part; run < RUNS; run += RP) {
      // lane group g reduces tile pixels i0 .. i0 + 7: one row, columns j0 .. j0 + 7
      const int i0 = 32 * run + 8 * g, r = i0 >> 4, j0 = i0 & 15;
      s16x8_t fa[MT];
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) fa[mt] = gc_frag_tr(dyt, lane, i0, slot * WD + 16 * mt);
#pragma unroll
      for (int t = 0; t < 9; ++t) {
        const int rb = G::base(r) + j0 + G::tapoff(t);
#pragma unroll
        for (int nt = 0; nt < MT; ++nt) {
          const s16x8_t fb = gc_frag_tr(patch, lane, rb, slot * WD + 16 * nt);
#pragma unroll
          for (int mt = 0; mt < MT; ++mt)
            acc[t][mt][nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                __builtin_bit_cast(bf16x8_t, fa[mt]), __builtin_bit_cast(bf16x8_t, fb), acc[t][mt][nt], 0, 0, 0);
        }
      }
    }
  }
  if (!active) return;
  // partial [tap][out channel 16mt + 4g + r][in channel 16nt + j] of this (block, part, slab)
  const long np = (long)gridDim.x * RP, q = (long)blockIdx.x * RP + part;
  float* o = a.ws + ((blockIdx.y * np + q) * SL + slot) * (9 * WD * WD);
#pragma unroll
  for (int t = 0; t < 9; ++t)
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
      for (int nt = 0; nt < MT; ++nt)
#pragma unroll
        for (int r = 0; r < 4; ++r)
          o[(t * WD + 16 * mt + 4 * g + r) * WD + 16 * nt + j] = acc[t][mt][nt][r];
}

// dw[ko][tap][ci in group] += sum over the NP partials, in order, of the
// diagonal-block element; the off-diagonal products are dropped here
__global__ void __launch_bounds__(256) gconv_wgrad_reduce_kernel(const float* ws, float* dw, int C, int Cg, int WD,
                                                                 int NP) {
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (long)C * 9 * Cg) return;
  const int cig = (int)(idx % Cg), tap = (int)((idx / Cg) % 9), ko = (int)(idx / (9 * Cg));
  const int SL = 64 / WD, chunk = ko >> 6, slot = (ko & 63) / WD, o = ko % WD;
  const int i = (ko / Cg) * Cg + cig - (ko / WD) * WD;
  const long tile = 9L * WD * WD;
  const float* p = ws + ((long)chunk * NP * SL + slot) * tile + (tap * WD + o) * WD + i;
  float s = 0.f;
  for (int q = 0; q < NP; ++q) s += p[(long)q * SL * tile];
  dw[idx] += s;
}

// images of every grouped weight of a model, one launch: [0] forward
// [C / Wd][tap][Wd out][Wd in], [1] data gradient: in / out swapped, taps
// mirrored; zero off the diagonal blocks
__global__ void __launch_bounds__(256) gconv_pack_kernel(GPBatch b) {
  int e = 0;
  while (e + 1 < b.n && (int)blockIdx.x >= b.e[e + 1].blk0) ++e;
  const GPEntry& en = b.e[e];
  const int WD = en.Cg < 16 ? 16 : en.Cg;
  const long per = 9L * en.C * WD;
  const long idx = (long)(blockIdx.x - en.blk0) * 256 + threadIdx.x;
  if (idx >= 2 * per) return;
  const int which = idx >= per;
  const long rem = idx - which * per;
  const int i = (int)(rem % WD), o = (int)((rem / WD) % WD), tap = (int)((rem / (WD * WD)) % 9);
  const int s = (int)(rem / (9L * WD * WD));
  const int ko = s * WD + (which ? i : o), ci = s * WD + (which ? o : i), t = which ? 8 - tap : tap;
  bf16_t v = 0;
  if (ko / en.Cg == ci / en.Cg) v = en.w[((long)ko * 9 + t) * en.Cg + ci % en.Cg];
  en.img[idx] = v;
}

inline int gc_wd(int Cg) { return Cg < 16 ? 16 : Cg; }
inline int cdiv(int a, int b) { return (a + b - 1) / b; }

template <int WD>
void gc_launch(int mode, const GcArgs& a, dim3 grid, hipStream_t s) {
  if (mode == GC_S1) hipLaunchKernelGGL((gconv_kernel<WD, GC_S1>), grid, dim3(256), 0, s, a);
  else if (mode == GC_S2) hipLaunchKernelGGL((gconv_kernel<WD, GC_S2>), grid, dim3(256), 0, s, a);
  else hipLaunchKernelGGL((gconv_kernel<WD, GC_DG2>), grid, dim3(256), 0, s, a);
}

void gc_run(int mode, GcArgs a, int Cg, hipStream_t s) {
  // tiles of `out`: 8 x 16 (S1), 4 x 16 (S2), 8 x 32 (DG2) pixels
  a.th = cdiv(a.Ho, 8 >> (mode == GC_S2));
  a.tw = cdiv(a.Wo, 16 << (mode == GC_DG2));
  const dim3 grid((unsigned)(a.N * a.th * a.tw), (unsigned)cdiv(a.C, 64));
  if (gc_wd(Cg) == 16) gc_launch<16>(mode, a, grid, s);
  else gc_launch<32>(mode, a, grid, s);
}

// persistent wgrad blocks per chunk: about one per CU over all chunks
inline int gw_blocks(int ntiles, int chunks) {
  int b = 256 / chunks;
  if (b < 1) b = 1;
  return b < ntiles ? b : ntiles;
}
inline int gw_tiles(int N, int P, int Q, int stride) { return N * cdiv(P, stride == 1 ? 8 : 4) * cdiv(Q, 16); }

}  // namespace

long gconv_image_elems(int C, int Cg) { return 2L * 9 * C * gc_wd(Cg); }

void gconv_pack_batch(GPBatch& b, hipStream_t s) {
  int blocks = 0;
  for (int i = 0; i < b.n; ++i) {
    b.e[i].blk0 = blocks;
    blocks += (int)((gconv_image_elems(b.e[i].C, b.e[i].Cg) + 255) / 256);
  }
  if (blocks > 0) hipLaunchKernelGGL(gconv_pack_kernel, dim3(blocks), dim3(256), 0, s, b);
}

void gconv_fwd(const bf16_t* x, const bf16_t* img, bf16_t* y, int N, int H, int W, int C, int Cg, int stride,
               hipStream_t s) {
  const int P = (H - 1) / stride + 1, Q = (W - 1) / stride + 1;
  gc_run(stride == 1 ? GC_S1 : GC_S2, GcArgs{x, y, img, nullptr, N, H, W, P, Q, C, 0, 0}, Cg, s);
}

void gconv_dgrad(const bf16_t* dy, const bf16_t* img, bf16_t* dx, const bf16_t* mask, int N, int H, int W, int C,
                 int Cg, int stride, hipStream_t s) {
  const int P = (H - 1) / stride + 1, Q = (W - 1) / stride + 1;
  const bf16_t* dimg = img + gconv_image_elems(C, Cg) / 2;
  gc_run(stride == 1 ? GC_S1 : GC_DG2, GcArgs{dy, dx, dimg, mask, N, P, Q, H, W, C, 0, 0}, Cg, s);
}

long gconv_wgrad_ws(int N, int H, int W, int C, int Cg, int stride) {
  const int P = (H - 1) / stride + 1, Q = (W - 1) / stride + 1, chunks = cdiv(C, 64);
  return (long)chunks * gw_blocks(gw_tiles(N, P, Q, stride), chunks) * 4 * 9 * gc_wd(Cg) * gc_wd(Cg);
}

void gconv_wgrad(const bf16_t* dy, const bf16_t* x, float* dw, float* ws, int N, int H, int W, int C, int Cg,
                 int stride, hipStream_t s) {
  const int P = (H - 1) / stride + 1, Q = (W - 1) / stride + 1, chunks = cdiv(C, 64), WD = gc_wd(Cg);
  GwArgs a{dy, x, ws, N, H, W, P, Q, C, cdiv(P, stride == 1 ? 8 : 4), cdiv(Q, 16), gw_tiles(N, P, Q, stride)};
  const int nb = gw_blocks(a.ntiles, chunks);
  const dim3 grid((unsigned)nb, (unsigned)chunks);
  if (WD == 16) {
    if (stride == 1) hipLaunchKernelGGL((gconv_wgrad_kernel<16, 1>), grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL((gconv_wgrad_kernel<16, 2>), grid, dim3(256), 0, s, a);
  } else {
    if (stride == 1) hipLaunchKernelGGL((gconv_wgrad_kernel<32, 1>), grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL((gconv_wgrad_kernel<32, 2>), grid, dim3(256), 0, s, a);
  }
  const long n = (long)C * 9 * Cg;
  hipLaunchKernelGGL(gconv_wgrad_reduce_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, ws, dw, C, Cg, WD,
                     nb * (4 / (64 / WD)));
}

}  // namespace tam
