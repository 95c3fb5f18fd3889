// Attention-dropout keep mask: the ONE definition every kernel regenerates.
//
// The decision for probability element (b, hq, i, j) (i = query position,
// j = key position) is a pure function of (seed, offset, b * HQ + hq, i, j,
// t). It does not depend on SQ, SKV, B, the tile shape, the grid,
// flash_block_rows, the XCD remap or the kernel that asks.
//
// Probabilities have 8 bits: t = round(256 * p), an element is DROPPED iff
// its random byte is < t, kept elements are scaled by 256 / (256 - t).
//
// Random bytes come from Philox4x32-7 (Salmon et al., "Parallel Random
// Numbers: As Easy as 1, 2, 3", SC'11: seven rounds are the fewest that
// pass BigCrush), keyed on the seed, one call per
//   (offset, bh, i >> 2, kg),   kg = (j >> 6) * 16 + (j & 15).
// The call's four 32-bit words are keys c, c + 16, c + 32, c + 48 of the
// 64-aligned key block (c = j & 15): word (j >> 4) & 3. The four bytes of a
// word are queries (i & ~3) + 0..3: byte i & 3. That is the footprint of one
// f32x4 score accumulator (four consecutive queries at one key) in the
// forward, dQ and pipelined dK/dV kernels, so a lane generates exactly the
// words it consumes: the forward and dQ lanes use all four words of a call
// (one 64-key tile), a dK/dV lane two (its 32-key strip).
//
// The 64-bit offset enters as counter word 3 (low half) and key word 1 (high
// half, XORed with the seed's): streams of all offsets below 2^32 with one
// seed are disjoint.
#pragma once
#include "common.h"

struct DropWords {
  uint w[4];
};

// a * b as (hi, lo)
DEVINL void philox_mulhilo(uint a, uint b, uint& hi, uint& lo) {
  lo = a * b;
  hi = __umulhi(a, b);
}

// The four words of call (bh, qg = i >> 2, kg) of stream (seed, offset).
DEVINL DropWords dropout_words(unsigned long long seed,
                               unsigned long long offset, uint bh, uint qg,
                               uint kg) {
  uint k0 = (uint)seed;
  uint k1 = (uint)(seed >> 32) ^ (uint)(offset >> 32);
  uint c0 = kg, c1 = qg, c2 = bh, c3 = (uint)offset;
#pragma unroll
  for (int round = 0; round < 7; ++round) {
    uint hi0, lo0, hi1, lo1;
    philox_mulhilo(0xD2511F53u, c0, hi0, lo0);
    philox_mulhilo(0xCD9E8D57u, c2, hi1, lo1);
    c0 = hi1 ^ c1 ^ k0;
    c1 = lo1;
    c2 = hi0 ^ c3 ^ k1;
    c3 = lo0;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  return DropWords{{c0, c1, c2, c3}};
}

// key-group index of key j: which call of a (bh, i >> 2) row holds it
DEVINL uint dropout_key_group(int j) {
  return ((uint)j >> 6) * 16u + ((uint)j & 15u);
}

// keep decision of byte r (query (i & ~3) + r) of one word; t in 1..255
DEVINL bool dropout_keep_byte(uint word, int r, int t) {
  return (int)((word >> (8 * r)) & 0xffu) >= t;
}

// The definition, element by element (the mask kernel calls this; the
// attention kernels call the three pieces above on their own footprint).
DEVINL bool dropout_keep(unsigned long long seed, unsigned long long offset,
                         int b, int hq, int HQ, int i, int j, int t) {
  const DropWords d = dropout_words(seed, offset, (uint)(b * HQ + hq),
                                    (uint)i >> 2, dropout_key_group(j));
  const int wi = (j >> 4) & 3;  // selects, not a dynamic index (scratch)
  const uint word = wi == 0 ? d.w[0] : wi == 1 ? d.w[1]
                  : wi == 2 ? d.w[2] : d.w[3];
  return dropout_keep_byte(word, i & 3, t);
}

// 256 / (256 - t): the factor on kept probabilities
DEVINL float dropout_keep_scale(int t) { return 256.f / (float)(256 - t); }
