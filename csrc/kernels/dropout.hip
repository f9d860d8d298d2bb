// tiresias_amd — training dropout (standalone form) and the per-step advance
// of a trainer's dropout record.
//
// The mask is never stored: it is a pure function of (record, site, element
// index) through Philox4x32-10 (tam/philox.h), so the backward is this same
// kernel applied to dy. One Philox call covers the 8 bf16 of a 16-byte load.
// The Transformer's residual sites do not run this kernel: they are applied
// inside the LayerNorm kernels (norm.hip).
#include "tam/common.h"
#include "tam/kernels.h"
#include "tam/philox.h"

namespace tam {

// y = keep ? bf16(fp32(x) * scale) : +0; y == x (in place) is allowed: every
// thread reads its own 16 bytes before it writes them
// (so x and y carry no __restrict__)
__global__ void __launch_bounds__(256) dropout_kernel(const bf16_t* x, bf16_t* y, long n, uint32_t thr, float scale,
                                                       const int* __restrict__ rec, uint32_t site) {
  const DropRec r{(uint32_t)rec[0], (uint32_t)rec[1], (uint32_t)rec[2]};
  const long n8 = n >> 3;
  for (long q = blockIdx.x * (long)blockDim.x + threadIdx.x; q < n8; q += (long)gridDim.x * blockDim.x) {
    const uint4 v = ((const uint4*)x)[q];
    const uint32_t keep = drop_keep8((uint64_t)q, site, r, thr);
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
    uint32_t o[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const float lo = __uint_as_float(w[i] << 16) * scale;
      const float hi = __uint_as_float(w[i] & 0xffff0000u) * scale;
      const uint32_t pk = pack_bf2(lo, hi);
      o[i] = ((keep >> (2 * i)) & 1u ? pk & 0xffffu : 0u) | ((keep >> (2 * i + 1)) & 1u ? pk & 0xffff0000u : 0u);
    }
    ((uint4*)y)[q] = make_uint4(o[0], o[1], o[2], o[3]);
  }
  // scalar tail: the n % 8 elements of the last (partial) group
  const int tail = (int)(n & 7);
  if (tail && blockIdx.x == 0 && (int)threadIdx.x < tail) {
    const uint32_t keep = drop_keep8((uint64_t)n8, site, r, thr);
    const long i = n8 * 8 + threadIdx.x;
    y[i] = (keep >> threadIdx.x) & 1u ? f2bf(bf2f(x[i]) * scale) : (bf16_t)0;
  }
}

// streaming, grid-strided on the optimizer's pattern: one block per CU
static int dgrid(long n8) {
  static int cus = 0;
  if (!cus) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess ||
        hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus < 1)
      cus = 256;
  }
  long b = (n8 + 255) / 256;
  if (b > cus) b = cus;
  return (int)(b < 1 ? 1 : b);
}

void dropout_apply(const bf16_t* x, bf16_t* y, long n, unsigned thr, float scale, const int* rec, int site,
                   hipStream_t s) {
  if (n <= 0) return;
  hipLaunchKernelGGL(dropout_kernel, dim3(dgrid(n >> 3)), dim3(256), 0, s, x, y, n, (uint32_t)thr, scale, rec,
                     (uint32_t)site);
}

// the step word advances ON the device, as the last launch of a captured
// forward + backward: a graph replay draws fresh masks with no host write
__global__ void dropout_advance_kernel(int* __restrict__ rec) {
  if (blockIdx.x == 0 && threadIdx.x == 0) rec[2] = (int)((uint32_t)rec[2] + 1u);
}

void dropout_advance(int* rec, hipStream_t s) {
  hipLaunchKernelGGL(dropout_advance_kernel, dim3(1), dim3(1), 0, s, rec);
}

}  // namespace tam
