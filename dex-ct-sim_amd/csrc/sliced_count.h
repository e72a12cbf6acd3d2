// Bit-sliced counters of rows16_kernel (siddon_packed.hip): 32 counters of 11 bits, one per bit position of the words
// added, held as 11 bit planes (Harley-Seal).  The one copy; plain C++ apart from the two-instruction adder, so that a
// host program can include it and count the same words (tests/test_sliced_count_host.py).
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define DEXCT_SLICED_FN __host__ __device__ __forceinline__
#else
#define DEXCT_SLICED_FN inline
#endif

namespace dexct {

// carry-save adder on 32 one-bit lanes: (h, l) = a + b + c.  gfx950 has v_bitop3_b32 (any function of three inputs, the
// truth table as an immediate): carry = majority = 0xE8, sum = parity = 0x96, TWO instructions.  They are written as the
// builtin because the compiler, given the and / or / xor form, re-associates the parity chains across adders and ends
// up with more instructions than the three per adder that the source spells.
DEXCT_SLICED_FN void csa(uint32_t& h, uint32_t& l, uint32_t a, uint32_t b, uint32_t c) {
#if defined(__HIP_DEVICE_COMPILE__) && defined(__gfx950__)
  h = __builtin_amdgcn_bitop3_b32(a, b, c, 0xE8);
  l = __builtin_amdgcn_bitop3_b32(a, b, c, 0x96);
#else
  const uint32_t u = a ^ b;
  h = (a & b) | (u & c);
  l = u ^ c;
#endif
}

// two stages of a ripple in three instructions: the carry out of the second stage and its sum, straight from the first
// stage's inputs (a = the second plane, b = the first plane, c = the carry into the first)
DEXCT_SLICED_FN uint32_t and3(uint32_t a, uint32_t b, uint32_t c) {
#if defined(__HIP_DEVICE_COMPILE__) && defined(__gfx950__)
  return __builtin_amdgcn_bitop3_b32(a, b, c, 0x80);
#else
  return a & b & c;
#endif
}
DEXCT_SLICED_FN uint32_t xor_and(uint32_t a, uint32_t b, uint32_t c) {        // a ^ (b & c)
#if defined(__HIP_DEVICE_COMPILE__) && defined(__gfx950__)
  return __builtin_amdgcn_bitop3_b32(a, b, c, 0x78);
#else
  return a ^ (b & c);
#endif
}

struct Sliced {
  uint32_t ones = 0, twos = 0, fours = 0, eights = 0;
  uint32_t hi[7] = {0, 0, 0, 0, 0, 0, 0};         // bits 4..10 of the 32 counters
  // a word of weight 16 ripples through the high planes, two planes per step and every plane updated in place (10
  // instructions, no copies).  Counters stay below 2048: no carry leaves hi[6].
  DEXCT_SLICED_FN void add_sixteens(uint32_t carry) {
#pragma unroll
    for (int k = 0; k < 6; k += 2) {
      const uint32_t c2 = and3(hi[k + 1], hi[k], carry);
      hi[k + 1] = xor_and(hi[k + 1], hi[k], carry);
      hi[k] ^= carry;
      carry = c2;
    }
    hi[6] ^= carry;
  }
  DEXCT_SLICED_FN void add_eights(uint32_t e) {
    const uint32_t c = eights & e;
    eights ^= e;
    add_sixteens(c);
  }
  // sixteen words: 8 + 4 + 2 + 1 = 15 adders (30 instructions) and ONE ripple (10): 2.5 instructions per word
  DEXCT_SLICED_FN void add16(const uint32_t (&x)[16]) {
    uint32_t ta, tb, fa, fb, ea, eb, c;
    csa(ta, ones, ones, x[0], x[1]);
    csa(tb, ones, ones, x[2], x[3]);
    csa(fa, twos, twos, ta, tb);
    csa(ta, ones, ones, x[4], x[5]);
    csa(tb, ones, ones, x[6], x[7]);
    csa(fb, twos, twos, ta, tb);
    csa(ea, fours, fours, fa, fb);
    csa(ta, ones, ones, x[8], x[9]);
    csa(tb, ones, ones, x[10], x[11]);
    csa(fa, twos, twos, ta, tb);
    csa(ta, ones, ones, x[12], x[13]);
    csa(tb, ones, ones, x[14], x[15]);
    csa(fb, twos, twos, ta, tb);
    csa(eb, fours, fours, fa, fb);
    csa(c, eights, eights, ea, eb);
    add_sixteens(c);
  }
  // eight words: 7 adders, a half adder into eights and the ripple (26 instructions)
  DEXCT_SLICED_FN void add8(const uint32_t (&x)[8]) {
    uint32_t ta, tb, fa, fb, e;
    csa(ta, ones, ones, x[0], x[1]);
    csa(tb, ones, ones, x[2], x[3]);
    csa(fa, twos, twos, ta, tb);
    csa(ta, ones, ones, x[4], x[5]);
    csa(tb, ones, ones, x[6], x[7]);
    csa(fb, twos, twos, ta, tb);
    csa(e, fours, fours, fa, fb);
    add_eights(e);
  }
  // four words (no sweep of the kernel uses it: the lists are padded to whole trips; the host test mixes it in)
  DEXCT_SLICED_FN void add4(const uint32_t (&x)[4]) {
    uint32_t ta, tb, fa;
    csa(ta, ones, ones, x[0], x[1]);
    csa(tb, ones, ones, x[2], x[3]);
    csa(fa, twos, twos, ta, tb);
    const uint32_t e = fours & fa;
    fours ^= fa;
    add_eights(e);
  }
  // all 32 counters at once: out[p] = counter of bit position p.  A 32 x 32 bit-matrix transpose (five rounds of
  // masked swaps) of the 11 planes; the 21 zero rows fold away at compile time: about a third of extracting every bit
  // of every counter on its own.
  DEXCT_SLICED_FN void unslice(uint32_t (&out)[32]) const {
    out[0] = ones; out[1] = twos; out[2] = fours; out[3] = eights;
#pragma unroll
    for (int k = 0; k < 7; ++k) out[4 + k] = hi[k];
#pragma unroll
    for (int k = 11; k < 32; ++k) out[k] = 0u;
    uint32_t m = 0x0000FFFFu;
#pragma unroll
    for (int j = 16; j != 0; j >>= 1) {
#pragma unroll
      for (int k = 0; k < 32; k = (k + j + 1) & ~j) {
        const uint32_t t = ((out[k] >> j) ^ out[k + j]) & m;
        out[k] ^= t << j;
        out[k + j] ^= t;
      }
      m ^= m << (j >> 1);
    }
  }
};

}  // namespace dexct
