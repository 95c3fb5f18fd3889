// Flash attention BACKWARD dK/dV for MI355X (gfx950) — pipelined tile loop.
//
// Computes exactly what flash_bwd_dkv_kernel (flash_attn_bwd.hip) computes:
// same grid and xcd_remap, BN = 256 keys per block (32 per wave), BM = 64
// query tile, same MFMA shapes, same accumulation order into dvacc / dkacc,
// same fp32 partial-slab output. Only the data movement differs, so the two
// kernels are held bit-equal by tests/test_gpu_flash_dkv_pipe.py:
//
//   1. One global read per element: a thread owns a row pair x 8 columns of
//      Q and of dO and writes the row-major and the transposed LDS image
//      from the same registers (the parent reads every element twice).
//   2. Issue early, write late: the loads of tile i+1 are issued right after
//      the barrier that publishes tile i, stay in flight under tile i's
//      MFMAs and are first waited for after the barrier that frees the
//      images. No load is issued for a tile index >= nqb, so a block with an
//      empty tile loop issues none.
//   3. LSE, delta and (SEGMENTED) q_start travel with the tile: waves 0..2
//      fetch 64 values each and publish them through a small LDS strip. No
//      global load sits between a tile's first and last MFMA.
//   4. Loop invariants are kept few and narrow (32-bit element offsets from
//      a wave-uniform tile base; swizzled addresses recomputed per tile) so
//      that the prefetch registers fit without scratch.
//   5. S and dP are computed with Q / dO as the A operand and K / V as the B
//      operand. The 16x16x32 A and B lane maps are identical, so no register
//      or LDS read changes, but a lane now holds one key and four
//      consecutive queries: P^T / dS^T go to LDS as one 8-byte store per
//      16-key strip instead of four 2-byte stores.
//
// The q / dout sequence stride must satisfy 64 * stride * 2 B < 4 GiB (the
// binding checks it).
//
// DROPOUT (DENSE mask only; no counterpart in the parent kernel):
// dV = (P . M * keep_scale)^T dO and dS = P . (M * keep_scale . dP - delta)
// * scale with the keep mask M of attn_dropout.h. By point 5 a lane holds
// four consecutive queries at key l15 of both 16-key strips, i.e. two of the
// four words of one call (the wave's 32 keys are half a 64-key block). The
// words are generated per 16-query sub-tile, after the MFMAs, and are dead
// before the next one.
#include "attn_common.h"
#include "attn_dropout.h"
#include "flash_dispatch.h"

template <int D, bool CAUSAL, bool RANGED = false, bool SEGMENTED = false,
          bool DROPOUT = false>
__global__ __launch_bounds__(512) void flash_bwd_dkv_pipe_kernel(
    const bf16* __restrict__ dO, const bf16* __restrict__ Q,
    const bf16* __restrict__ K, const bf16* __restrict__ V,
    const float* __restrict__ LSE, const float* __restrict__ DELTA,
    float* __restrict__ dK,  // [group, s, b, hkv, d] fp32 partials, as the
    float* __restrict__ dV,  // parent kernel writes them
    int SQ, int SKV, int Bb, int HQ, int HKV, float scale,
    int window, long sQs, long sQb, long sQh, long sKs, long sKb, long sKh,
    long sVs, long sVb, long sVh, long sDs, long sDb, long sDh,
    const int* __restrict__ kv_lo = nullptr,  // [B] int32 (RANGED), or
    const int* __restrict__ kv_hi = nullptr,  // [B, S] (SEGMENTED)
    int drop_t = 0,  // DROPOUT: threshold 1..255 and the random stream
    unsigned long long drop_seed = 0, unsigned long long drop_off = 0) {
  static_assert(!(RANGED && SEGMENTED), "one mask mode at a time");
  static_assert(!SEGMENTED || CAUSAL, "segments are causal");
  static_assert(!DROPOUT || !(RANGED || SEGMENTED), "dropout: DENSE only");
  constexpr int BN = 256;  // keys per block
  constexpr int BM = 64;   // q tile
  const int coff = SKV - SQ;  // bottom-right causal alignment
  constexpr int KP = D + 8;
  constexpr int VP = BM + 8;
  // The parent's six images with the parent's layouts, paired into three
  // arrays so that one address register and immediate offsets reach both
  // members of a pair.
  __shared__ __attribute__((aligned(16))) __bf16 qdo_lds[2 * BM * KP];
  __shared__ __attribute__((aligned(16))) __bf16 tr_lds[2 * D * VP];
  __shared__ __attribute__((aligned(16))) __bf16 pds_lds[2 * 8 * 32 * VP];
  __bf16* const q_lds = qdo_lds;            // Q   [BM][KP] row-major
  __bf16* const do_lds = qdo_lds + BM * KP;  // dO  [BM][KP] row-major
  __bf16* const dot_lds = tr_lds;            // dO^T [D][VP], tr_swz
  __bf16* const qt_lds = tr_lds + D * VP;    // Q^T  [D][VP], tr_swz
  __bf16* const pT_lds = pds_lds;            // P^T  [256 keys][VP]
  __bf16* const dsT_lds = pds_lds + 8 * 32 * VP;  // dS^T
  // D = 128: the register file cannot hold both accumulator sets (128),
  // the K / V fragments (64), the prefetched tile (17) and the S / dP
  // working set. PARK of the 16 V fragments live in LDS instead, one 16-byte
  // slot per thread each (lane-linear, conflict-free), written once and
  // read back by the same thread in every 16-query sub-tile.
  constexpr int PARK = (D == 128) ? 2 : 0;
  __shared__ __attribute__((aligned(16))) __bf16 park_lds[PARK * 512 * 8 + 8];
  // per-tile row constants: [0] LSE, [1] delta, [2] q_start (as int bits)
  __shared__ __attribute__((aligned(16))) float row_lds[3 * BM];

  const int lane = threadIdx.x & 63;
  // scalar wave id: keeps krow_w and every wave-level test (wave skip,
  // full_patch) in SGPRs and their branches scalar
  const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int group = HQ / HKV;
  int kblock, bhg;  // (b * HKV + hkv) * group + g
  xcd_remap(kblock, bhg);
  const int g = bhg % group;
  const int hkv = (bhg / group) % HKV;
  const int b = bhg / (group * HKV);
  // wave-uniform visible key range of this batch row
  int lo = 0, hi = SKV;
  if constexpr (RANGED) {
    lo = kv_lo[b];
    hi = kv_hi[b];
  }

  const bf16* Kp = K + b * sKb + hkv * sKh;
  const bf16* Vp = V + b * sVb + hkv * sVh;
  const int kbase = kblock * BN;
  const int krow_w = kbase + wid * 32;  // 2 sub-blocks of 16 keys

  constexpr int DK = D / 32;
  bf16x8_t kfrag[2][DK], vfrag[2][DK];
#pragma unroll
  for (int sb = 0; sb < 2; ++sb) {
    const int r = krow_w + sb * 16 + (lane & 15);
    const long row = (r < SKV) ? r : (SKV - 1);
#pragma unroll
    for (int kk = 0; kk < DK; ++kk) {
      *(int4*)&kfrag[sb][kk] =
          *(const int4*)(Kp + row * sKs + kk * 32 + (lane >> 4) * 8);
      *(int4*)&vfrag[sb][kk] =
          *(const int4*)(Vp + row * sVs + kk * 32 + (lane >> 4) * 8);
      // fold the softmax scale into K once
#pragma unroll
      for (int j = 0; j < 8; ++j)
        kfrag[sb][kk][j] = (__bf16)((float)kfrag[sb][kk][j] * scale);
    }
  }

#pragma unroll
  for (int i = 0; i < PARK; ++i)
    *(bf16x8_t*)&park_lds[(i * 512 + threadIdx.x) * 8] =
        vfrag[1][DK - PARK + i];

  constexpr int DN2 = D / 32;
  f32x16_t dvacc[DN2], dkacc[DN2];
#pragma unroll
  for (int nj = 0; nj < DN2; ++nj) {
    dvacc[nj] = f32x16_t{};
    dkacc[nj] = f32x16_t{};
  }

  {
    const int hq = hkv * group + g;
    const bf16* Qp = Q + b * sQb + hq * sQh;
    const bf16* dOp = dO + b * sDb + hq * sDh;
    const float* Lp = LSE + ((long)b * HQ + hq) * SQ;
    const float* Dp = DELTA + ((long)b * HQ + hq) * SQ;

    // tile range, exactly as the parent kernel derives it
    const int klo = RANGED ? max(kbase, lo) : kbase;
    const int khi = RANGED ? min(kbase + BN, hi) : kbase + BN;
    const int ib0 = CAUSAL ? max(0, (klo - coff) / BM) : 0;
    int nqb = (SQ + BM - 1) / BM;
    if (CAUSAL && window > 0)
      nqb = min(nqb, (khi - 1 + window - coff + BM - 1) / BM);
    if (RANGED && klo >= khi) nqb = 0;
    const int* Sp = kv_lo + (long)b * SQ;  // q_start row (SEGMENTED only)
    if constexpr (SEGMENTED)
      nqb = min(nqb,
                (kv_hi[(long)b * SQ + min(kbase + BN, SKV) - 1] + BM - 1) / BM);

    // staging task of a thread: rows (srow, srow + 1) x 8 columns of the
    // tile; D = 128 gives every thread one task, D = 64 the first 256.
    // Both lambdas re-derive the task from the thread id behind an opaque
    // copy: hoisted out of the tile loop, the row / column / offsets and the
    // eight swizzled write addresses would stay live across the MFMAs.
    constexpr int C8 = D / 8;
    const uint qrs = (uint)sQs * 2, dors = (uint)sDs * 2;  // row strides, B
    // which row constant this wave fetches: 0 LSE, 1 delta, 2 q_start
    constexpr int NROWC = SEGMENTED ? 3 : 2;
    const float* rowp = wid == 0 ? Lp : wid == 1 ? Dp : (const float*)Sp;

    // prefetch registers of the next tile
    typedef int i32x4_t __attribute__((ext_vector_type(4)));
    i32x4_t q0 = {0, 0, 0, 0}, q1 = q0, d0 = q0, d1 = q0;  // whole 128-bit
    float rowc = 0.f;  // registers: 32- or 16-bit views get split and copied
    // The loads are unconditional: a row at or past SQ reads row SQ - 1
    // instead (no row >= SQ is ever read) and is zeroed in write_tile. A
    // conditional load would copy its result into the loop-carried register
    // behind a wait placed right where the load is issued.
    auto issue_tile = [&](int ib) {
      const int qbase = ib * BM;
      int t = threadIdx.x;
      asm volatile("" : "+v"(t));
      const int last = SQ - 1 - qbase;  // >= 0: the tile has a row
      if ((D == 128) || wid < 4) {  // D = 64: waves 0..3 stage
        const int srow = (t / C8) * 2, scol = (t % C8) * 8;
        const int r0 = min(srow, last), r1 = min(srow + 1, last);
        // wave-uniform 64-bit tile bases + 32-bit per-thread byte offsets
        const char* qt = (const char*)(Qp + (long)qbase * sQs);
        const char* dt = (const char*)(dOp + (long)qbase * sDs);
        q0 = *(const i32x4_t*)(qt + ((uint)r0 * qrs + scol * 2));
        d0 = *(const i32x4_t*)(dt + ((uint)r0 * dors + scol * 2));
        q1 = *(const i32x4_t*)(qt + ((uint)r1 * qrs + scol * 2));
        d1 = *(const i32x4_t*)(dt + ((uint)r1 * dors + scol * 2));
      }
      if (wid < NROWC)
        rowc = *(const float*)((const char*)(rowp + qbase) +
                               (uint)min(t & 63, last) * 4);
    };
    auto write_tile = [&](int ib) {
      // nothing computed from the loaded values may move above this point
      // (it would wait for the loads right where they are issued)
      asm volatile("" : "+v"(q0), "+v"(q1), "+v"(d0), "+v"(d1));
      asm volatile("" : "+v"(rowc));
      const int last = SQ - 1 - ib * BM;
      int t = threadIdx.x;
      asm volatile("" : "+v"(t));
      if ((D == 128) || wid < 4) {
        const int sr = (t / C8) * 2, sc = (t % C8) * 8;
        if (sr > last) q0 = d0 = i32x4_t{0, 0, 0, 0};  // rows past SQ:
        if (sr + 1 > last) q1 = d1 = i32x4_t{0, 0, 0, 0};  // zero, as the parent
        *(i32x4_t*)&q_lds[sr * KP + sc] = q0;
        *(i32x4_t*)&q_lds[(sr + 1) * KP + sc] = q1;
        *(i32x4_t*)&do_lds[sr * KP + sc] = d0;
        *(i32x4_t*)&do_lds[(sr + 1) * KP + sc] = d1;
        // transposed images: columns sc + 2m, sc + 2m + 1 of the row pair,
        // packed from the 32-bit words (no 16-bit views of the prefetch
        // registers: they would be carried across the loop as halves)
        const uint qw0[4] = {(uint)q0.x, (uint)q0.y, (uint)q0.z, (uint)q0.w};
        const uint qw1[4] = {(uint)q1.x, (uint)q1.y, (uint)q1.z, (uint)q1.w};
        const uint rw0[4] = {(uint)d0.x, (uint)d0.y, (uint)d0.z, (uint)d0.w};
        const uint rw1[4] = {(uint)d1.x, (uint)d1.y, (uint)d1.z, (uint)d1.w};
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const int m = j >> 1;
          const uint qp = (j & 1) ? (qw0[m] >> 16) | (qw1[m] & 0xffff0000u)
                                  : (qw0[m] & 0xffffu) | (qw1[m] << 16);
          const uint dp = (j & 1) ? (rw0[m] >> 16) | (rw1[m] & 0xffff0000u)
                                  : (rw0[m] & 0xffffu) | (rw1[m] << 16);
          const int r = sc + j;
          const uint byte = tr_swz((uint)(r * VP + sr) * 2, r);
          *(uint*)((char*)qt_lds + byte) = qp;
          *(uint*)((char*)dot_lds + byte) = dp;
        }
      }
      // rows past SQ get the parent's fill values (1e30 / 0 / 0)
      if (wid < NROWC)
        row_lds[wid * BM + (t & 63)] =
            (t & 63) > last ? (wid == 0 ? 1e30f : 0.f) : rowc;
    };

    if (ib0 < nqb) issue_tile(ib0);
    for (int ib = ib0; ib < nqb; ++ib) {
      const int qbase = ib * BM;
      write_tile(ib);  // first wait for the tile's loads
      __syncthreads();
      if (ib + 1 < nqb) issue_tile(ib + 1);  // in flight under the MFMAs

      int qs_tile = 0;  // q_start of the tile's first query
      if constexpr (SEGMENTED)
        qs_tile = __builtin_amdgcn_readfirstlane(
            __float_as_int(row_lds[2 * BM]));
      // causal: skip waves whose keys are all above this q tile
      if ((!CAUSAL || krow_w <= qbase + BM - 1 + coff) &&
          (!RANGED || (krow_w < hi && krow_w + 32 > lo)) &&
          // SEGMENTED: the wave's keys all lie below the segment of the
          // tile's first (hence every) query
          (!SEGMENTED || krow_w + 32 > qs_tile)) {
        __bf16* pw = &pT_lds[wid * 32 * VP];
        __bf16* dw = &dsT_lds[wid * 32 * VP];
        // lane-derived values are re-derived per tile (a few VALU ops) so
        // that none of them, nor anything computed from them, is carried
        // across the tile loop in a register
        int ln = threadIdx.x;
        asm volatile("" : "+v"(ln));
        ln &= 63;
        const int l15 = ln & 15;       // key within a 16-key strip
        const int lq = (ln >> 4) * 4;  // first of the lane's 4 queries
        const int dl = lq - l15;
#pragma unroll
        for (int nq = 0; nq < BM / 16; ++nq) {
          // Q / dO as A, K / V as B: the lane holds key l15 of each 16-key
          // strip and queries nq * 16 + lq + r
          f32x4_t st[2], dpt[2];
          st[0] = st[1] = f32x4_t{0.f, 0.f, 0.f, 0.f};
          dpt[0] = dpt[1] = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
          for (int kk = 0; kk < DK; ++kk) {
            bf16x8_t qa = load_frag_a(&q_lds[nq * 16 * KP], KP, kk * 32, ln);
            st[0] = MFMA_16x16x32(qa, kfrag[0][kk], st[0]);
            st[1] = MFMA_16x16x32(qa, kfrag[1][kk], st[1]);
            bf16x8_t da = load_frag_a(&do_lds[nq * 16 * KP], KP, kk * 32, ln);
            dpt[0] = MFMA_16x16x32(da, vfrag[0][kk], dpt[0]);
            bf16x8_t vf1;
            if (kk < DK - PARK)
              vf1 = vfrag[1][kk];
            else
              vf1 = *(const bf16x8_t*)&park_lds[((kk - (DK - PARK)) * 512 +
                                                 wid * 64 + ln) * 8];
            dpt[1] = MFMA_16x16x32(da, vf1, dpt[1]);
          }
          __builtin_amdgcn_sched_barrier(0);
          const f32x4_t lse = *(const f32x4_t*)&row_lds[nq * 16 + lq];
          const f32x4_t delta = *(const f32x4_t*)&row_lds[BM + nq * 16 + lq];
          // DROPOUT: the lane's word of each 16-key strip (byte r = query
          // lq + r); strip sb of wave wid is word (wid & 1) * 2 + sb of the
          // block's call, a scalar choice
          uint rw0 = 0u, rw1 = 0u;
          float kscale = 1.f;
          if constexpr (DROPOUT) {
            const DropWords w4 = dropout_words(
                drop_seed, drop_off, (uint)(b * HQ + hq),
                (uint)(qbase + nq * 16 + lq) >> 2,
                dropout_key_group(krow_w + l15));
            const bool upper = (wid & 1) != 0;
            rw0 = upper ? w4.w[2] : w4.w[0];
            rw1 = upper ? w4.w[3] : w4.w[1];
            kscale = dropout_keep_scale(drop_t);
          }
          // interior fast path: every (q, key) of this 16-query x 32-key
          // patch in bounds and alive — no compare/selects
          bool full_patch =
              (!RANGED || (krow_w >= lo && krow_w + 31 < hi)) &&
              (qbase + nq * 16 + 15 < SQ) && (krow_w + 31 < SKV) &&
              (!CAUSAL || (qbase + nq * 16 + coff >= krow_w + 31)) &&
              (window <= 0 ||
               (qbase + nq * 16 + 15 + coff < krow_w + window));
          if constexpr (SEGMENTED)  // the patch's last query starts latest
            full_patch = full_patch &&
                         krow_w >= __builtin_amdgcn_readfirstlane(
                                       __float_as_int(
                                           row_lds[2 * BM + nq * 16 + 15]));
          // one 8-byte store per 16-key strip: 4 consecutive queries
          typedef __bf16 bf16x4_t __attribute__((ext_vector_type(4)));
          if (full_patch) {
#pragma unroll
            for (int sb = 0; sb < 2; ++sb) {
              bf16x4_t p4, ds4;
#pragma unroll
              for (int r = 0; r < 4; ++r) {
                const float p = __expf(st[sb][r] - lse[r]);
                if constexpr (DROPOUT) {
                  // M * keep_scale
                  const float mk =
                      dropout_keep_byte(sb ? rw1 : rw0, r, drop_t) ? kscale : 0.f;
                  const float ds = p * (dpt[sb][r] * mk - delta[r]) * scale;
                  p4[r] = (__bf16)(p * mk);
                  ds4[r] = (__bf16)ds;
                } else {
                  const float ds = p * (dpt[sb][r] - delta[r]) * scale;
                  p4[r] = (__bf16)p;
                  ds4[r] = (__bf16)ds;
                }
              }
              const int at = (sb * 16 + l15) * VP + nq * 16 + lq;
              *(bf16x4_t*)&pw[at] = p4;
              *(bf16x4_t*)&dw[at] = ds4;
            }
          } else {
            // the parent's tests with key = k0 + l15 and query = q0 + lq + r,
            // the wave-uniform terms gathered on one side of each compare
            const int q0 = qbase + nq * 16;
            int qs[4] = {0, 0, 0, 0};  // first key visible to each query
            if constexpr (SEGMENTED) {
              const int4 t = *(const int4*)&row_lds[2 * BM + nq * 16 + lq];
              qs[0] = t.x, qs[1] = t.y, qs[2] = t.z, qs[3] = t.w;
            }
#pragma unroll
            for (int sb = 0; sb < 2; ++sb) {
              bf16x4_t p4, ds4;
              const int k0 = krow_w + sb * 16;
              const int kd = k0 - q0 - coff;  // key above query: dl + r < kd
              bool kdead = l15 >= SKV - k0;
              if constexpr (RANGED) kdead |= (l15 < lo - k0) || (l15 >= hi - k0);
#pragma unroll
              for (int r = 0; r < 4; ++r) {
                bool dead = kdead || (lq >= SQ - q0 - r) ||
                            (CAUSAL && dl < kd - r);
                if (CAUSAL && window > 0) dead |= (dl >= kd + window - r);
                if constexpr (SEGMENTED) dead |= (l15 < qs[r] - k0);
                const float p = dead ? 0.f : __expf(st[sb][r] - lse[r]);
                if constexpr (DROPOUT) {
                  // M * keep_scale
                  const float mk =
                      dropout_keep_byte(sb ? rw1 : rw0, r, drop_t) ? kscale : 0.f;
                  const float ds = p * (dpt[sb][r] * mk - delta[r]) * scale;
                  p4[r] = (__bf16)(p * mk);
                  ds4[r] = (__bf16)ds;
                } else {
                  const float ds = p * (dpt[sb][r] - delta[r]) * scale;
                  p4[r] = (__bf16)p;
                  ds4[r] = (__bf16)ds;
                }
              }
              const int at = (sb * 16 + l15) * VP + nq * 16 + lq;
              *(bf16x4_t*)&pw[at] = p4;
              *(bf16x4_t*)&dw[at] = ds4;
            }
          }
          __builtin_amdgcn_sched_barrier(0);
        }
        // dV += P^T dO ; dK += dS^T Q — 32x32x16, contraction in 16-q
        // chunks; A = the wave's own P^T/dS^T strip, loaded once per kq
        // The B reads are load_frag_b32_trT_swz(img, VP, nj * 32, kq * 16):
        // with r = nj * 32 + (lane & 31) the swizzle term splits into a
        // per-lane part (bits 4-5) and bit 6 = nj & 1, and nj * 32 rows are a
        // multiple of 512 B, so two addresses per kq plus immediates serve
        // all nj — recomputed here instead of sixteen kept live
        const int l31 = ln & 31;
        const uint tra = (uint)(l31 * VP + (ln >> 5) * 8) * 2;
        const uint trs = ((uint)(l31 >> 3) & 3u) << 4;
#pragma unroll
        for (int kq = 0; kq < BM / 16; ++kq) {
          bf16x8_t pa = load_frag_a32(pw, VP, kq * 16, ln);
          bf16x8_t da = load_frag_a32(dw, VP, kq * 16, ln);
          const uint tr0 = (tra + kq * 32) ^ trs;  // even nj
          const uint tr1 = tr0 ^ 64u;              // odd nj
#pragma unroll
          for (int nj = 0; nj < DN2; ++nj) {
            const uint byte = ((nj & 1) ? tr1 : tr0) + nj * 32 * VP * 2;
            bf16x8_t dob, qb2;
            *(int4*)&dob = *(const int4*)((const char*)dot_lds + byte);
            dvacc[nj] = MFMA_32x32x16(pa, dob, dvacc[nj]);
            *(int4*)&qb2 = *(const int4*)((const char*)qt_lds + byte);
            dkacc[nj] = MFMA_32x32x16(da, qb2, dkacc[nj]);
          }
        }
      }
      __syncthreads();  // frees the images for the next tile's writes
    }
  }

  // ---- store fp32 partials: [group][s][b][hkv][d] (32x32 C layout) ----
  const long sOs = (long)Bb * HKV * D;
  const long slab = (long)g * SKV * sOs + ((long)b * HKV + hkv) * D;
  float* dKp = dK + slab;
  float* dVp = dV + slab;
#pragma unroll
  for (int nj = 0; nj < DN2; ++nj) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int krow = krow_w + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
      if (krow < SKV) {
        const int dcol = nj * 32 + (lane & 31);
        dKp[(long)krow * sOs + dcol] = dkacc[nj][r];
        dVp[(long)krow * sOs + dcol] = dvacc[nj][r];
      }
    }
  }
}

// dK/dV only, same grid as the parent's launch in launch_flash_bwd
extern "C" void launch_flash_dkv_pipe(const FlashArgs& a, hipStream_t stream) {
  // one block per (kblock, b, hkv, g)
  const dim3 gkv((a.SKV + 255) / 256, a.B * a.HQ), blk(512);
  dispatch_flash_drop(a, [&](auto d, auto c, auto r, auto s, auto p) {
    flash_bwd_dkv_pipe_kernel<decltype(d)::value, decltype(c)::value,
                              decltype(r)::value, decltype(s)::value,
                              decltype(p)::value>
        <<<gkv, blk, 0, stream>>>(
            (const bf16*)a.dout, (const bf16*)a.q, (const bf16*)a.k,
            (const bf16*)a.v, (const float*)a.lse, (const float*)a.delta,
            (float*)a.dk, (float*)a.dv, a.SQ, a.SKV, a.B, a.HQ, a.HKV,
            a.scale, a.window, a.qs[0], a.qs[1], a.qs[2], a.ks[0], a.ks[1],
            a.ks[2], a.vs[0], a.vs[1], a.vs[2], a.ds[0], a.ds[1], a.ds[2],
            a.bound_a, a.bound_b, a.drop_t, a.drop_seed, a.drop_offset);
  });
}
