// tiresias_amd — Philox4x32-10 counter-based generator and the dropout mask
// built on it (device and host, plain C++: a 32x32->64 multiply is all it
// needs).
//
// Mask contract (README "Training dropout"; tests rebuild it on the host):
// one Philox call per group of 8 consecutive elements of a contiguous tensor.
// For flat element index i: q = i >> 3, j = i & 7,
//   counter = (q & 0xffffffff, q >> 32, site, step), key = (seed, stream),
//   u = (out[j >> 1] >> (16 * (j & 1))) & 0xffff, kept iff u >= thr,
// thr = round(p * 65536) in (0, 65536). Kept elements are scaled by
// fp32(65536) / fp32(65536 - thr), dropped ones become +0. Nothing is stored:
// the backward regenerates the mask from the same (record, site).
//
// Attention-probability mask contract (README "Training dropout"; tests
// rebuild it on the host): a pure function of the logical position
// (b, h, q, kv) in the [B,H,Sq,Sk] probability tensor, (b, q) indexing the
// [B,S,H,64] views the attention kernels take. One Philox call covers a block
// of 4 queries x 4 keys, block (Q, K) = (q >> 2, kv >> 2):
//   counter = (K | (Q << 16), b*H + h, 0x80000000 | a, step), key = (seed, stream),
//   u = (out[q & 3] >> (8 * (kv & 3))) & 0xff, kept iff u >= thr,
// thr = round(p * 256) in (0, 256), so p is quantised to 1/256. a is the
// attention call's ordinal within the forward, from a counter of its own: the
// elementwise sites above keep their ordinals whether or not attention dropout
// is on, and the top bit of the site word keeps the two spaces apart. Kept
// probabilities are scaled by fp32(256) / fp32(256 - thr). Sq, Sk <= 262144
// (Q, K fit 16 bits) and B*H <= 2^32.
// Why 4 x 4: the forward kernel's lane holds 4 consecutive keys of one query
// (one output word), both backward kernels' lane holds 4 consecutive queries
// of one key (one byte of each of the four words), so either direction eats
// whole Philox outputs. The running max, row sum and LSE come from the
// undropped scores: O = (keep * P) V * scale, LSE unchanged.
//
// Optimizer-state rounding contract (README "bf16 optimizer state"; tests
// rebuild it on the host): bf16 moments are stored with stochastic rounding.
// One Philox call covers 4 consecutive arena elements, the float4 group the
// optimizer kernels work in. For arena element index e (within the whole
// arena, not within the launch): q = e >> 2, j = e & 3,
//   counter = (q & 0xffffffff, q >> 32, 0x40000000, step), key = (seed, 0),
//   u_m = out[j] & 0xffff   (first moment / SGD momentum),
//   u_v = out[j] >> 16      (Adam second moment).
// step is the 1-based optimizer step (the integer Adam takes). The site word
// 0x40000000 keeps this counter space apart from elementwise dropout (small
// ordinals) and attention dropout (top bit set). The key holds no gang
// position: every member of a non-sharded gang writes identical state.
// Rounding fp32 bits b with a 16-bit draw u (sr_bf16): exponent field not all
// ones -> (b + u) >> 16, which rounds the magnitude up with probability
// (b & 0xffff) / 65536 -- unbiased, and a carry into the exponent (up to inf
// from the largest finite values) is the correct result; inf passes through;
// NaN stays NaN (quiet bit forced). A value that is exact in bf16 (low 16
// bits zero) comes back unchanged for every draw.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define TAM_HD __host__ __device__ __forceinline__
#else
#define TAM_HD inline
#endif

namespace tam {

constexpr uint32_t kPhiloxM0 = 0xD2511F53u, kPhiloxM1 = 0xCD9E8D57u;
constexpr uint32_t kPhiloxW0 = 0x9E3779B9u, kPhiloxW1 = 0xBB67AE85u;

TAM_HD void philox4x32_10(const uint32_t (&ctr)[4], const uint32_t (&key)[2], uint32_t (&out)[4]) {
  uint32_t c0 = ctr[0], c1 = ctr[1], c2 = ctr[2], c3 = ctr[3];
  uint32_t k0 = key[0], k1 = key[1];
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint64_t p0 = (uint64_t)kPhiloxM0 * c0;
    const uint64_t p1 = (uint64_t)kPhiloxM1 * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0;
    const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
    c1 = (uint32_t)p1;
    c3 = (uint32_t)p0;
    c0 = n0;
    c2 = n2;
    k0 += kPhiloxW0;
    k1 += kPhiloxW1;
  }
  out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

// the dropout record a trainer keeps on the device: int32[4] {seed, stream,
// step, 0}; dropout_advance bumps step once per training step
struct DropRec {
  uint32_t seed, stream, step;
};

// keep bits of group q (elements 8q .. 8q+7): bit j set = element 8q+j is kept
TAM_HD uint32_t drop_keep8(uint64_t q, uint32_t site, const DropRec& r, uint32_t thr) {
  const uint32_t ctr[4] = {(uint32_t)q, (uint32_t)(q >> 32), site, r.step};
  const uint32_t key[2] = {r.seed, r.stream};
  uint32_t o[4];
  philox4x32_10(ctr, key, o);
  uint32_t bits = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    bits |= ((o[i] & 0xffffu) >= thr ? 1u : 0u) << (2 * i);
    bits |= ((o[i] >> 16) >= thr ? 1u : 0u) << (2 * i + 1);
  }
  return bits;
}

// site word of the optimizer-state rounding draws
constexpr uint32_t kOptStateSite = 0x40000000u;

// fp32 bits b -> bf16 bits, stochastically rounded with the 16-bit draw u
TAM_HD uint32_t sr_bf16(uint32_t b, uint32_t u) {
  if ((b & 0x7f800000u) == 0x7f800000u)   // inf passes, NaN keeps its sign and turns quiet
    return (b >> 16) | ((b & 0x007fffffu) ? 0x40u : 0u);
  return (b + u) >> 16;
}

// the four words of group q (arena elements 4q .. 4q+3) at optimizer step
// `step`: element j rounds its first moment with out[j] & 0xffff and its
// second moment with out[j] >> 16
TAM_HD void opt_state_draw4(uint64_t q, uint32_t seed, uint32_t step, uint32_t (&out)[4]) {
  const uint32_t ctr[4] = {(uint32_t)q, (uint32_t)(q >> 32), kOptStateSite, step};
  const uint32_t key[2] = {seed, 0u};
  philox4x32_10(ctr, key, out);
}

// the four words of attention-mask block (Q, K) = (q >> 2, kv >> 2) of head
// bh = b*H + h at attention call ordinal a: word q & 3, byte kv & 3
TAM_HD void attn_drop_block(uint32_t Q, uint32_t K, uint32_t bh, uint32_t a, const DropRec& r,
                            uint32_t (&out)[4]) {
  const uint32_t ctr[4] = {K | (Q << 16), bh, 0x80000000u | a, r.step};
  const uint32_t key[2] = {r.seed, r.stream};
  philox4x32_10(ctr, key, out);
}

}  // namespace tam
