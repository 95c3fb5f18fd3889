// Causal flash attention BACKWARD for MI355X (gfx950) — v2.
// FlashAttention-2 recompute, two kernels, no atomics:
//   dkv: grid over 256-key blocks — recompute P^T, accumulate dV, dK
//   dq : grid over 256-query blocks — recompute P, accumulate dQ
// GQA: dkv sums over the q-head group of each kv head in-kernel.
// delta = rowsum(dO ∘ O) is computed by the caller.
//
// v2: strided [s, b, h, d] IO (no permutes), 8 waves with 2 sub-blocks per
// wave (every staged LDS B-fragment feeds 2 MFMAs), paired transpose
// writes. dkv: BN=256 keys (32/wave), q-tile 64. dq: BM=256 (32/wave),
// key tile 64.
#include "attn_common.h"
#include "attn_dropout.h"
#include "flash_dispatch.h"

// RANGED (both kernels): per-batch-row visible key range
// [kv_lo[b], kv_hi[b]) on top of the causal / window mask, matching
// flash_fwd_dbuf_kernel<.., RANGED>. Keys outside the range get dK = dV = 0
// (their slabs are still written); query rows with no alive key get dQ = 0
// and contribute nothing. RANGED=false compiles exactly as before and
// never reads kv_lo / kv_hi.
//
// SEGMENTED (both kernels): packed sequences, block-diagonal causal mask
// (S_q == S_kv), matching flash_fwd_dbuf_kernel<.., SEGMENTED>. The same
// two pointers then carry per-token int32 [B, S] bounds: kv_lo = q_start
// (first key query i may see) decides every mask bit; kv_hi = k_end (one
// past the last query that sees key j) only bounds the dkv q-tile loop.
// Both are non-decreasing along a row.
// ============================ dK / dV ============================
template <int D, bool CAUSAL, bool RANGED = false, bool SEGMENTED = false>
__global__ __launch_bounds__(512) void flash_bwd_dkv_kernel(
    const bf16* __restrict__ dO, const bf16* __restrict__ Q,
    const bf16* __restrict__ K, const bf16* __restrict__ V,
    const float* __restrict__ LSE, const float* __restrict__ DELTA,
    float* __restrict__ dK,  // [group, s, b, hkv, d] fp32 PARTIALS (one
    float* __restrict__ dV,  // slab per q-head of the GQA group; the
                             // binding sums over dim 0) — one block per
                             // (key-block, b, hkv, g) keeps the grid full
                             // even at TP=8 where HKV_local = 1
    int SQ, int SKV, int Bb, int HQ, int HKV, float scale,
    int window, long sQs, long sQb, long sQh, long sKs, long sKb, long sKh,
    long sVs, long sVb, long sVh, long sDs, long sDb, long sDh,
    const int* __restrict__ kv_lo = nullptr,  // [B] int32 (RANGED), or
    const int* __restrict__ kv_hi = nullptr) {  // [B, S] (SEGMENTED)
  static_assert(!(RANGED && SEGMENTED), "one mask mode at a time");
  static_assert(!SEGMENTED || CAUSAL, "segments are causal");
  constexpr int BN = 256;  // keys per block
  // q tile 64 at 145 KB LDS = 1 block/CU. A BM=32 variant (79 KB, 2
  // blocks/CU) measured SLOWER (14.7 vs 12.0 ms): halving the tile
  // doubles per-tile staging/barrier overhead. This kernel is NOT
  // MFMA-bound: about a fifth of a tile's cycles are MFMA issue; it reads
  // Q/dO twice per tile with both fetches exposed after the closing
  // barrier, and D = 128 spills (27 VGPRs, 112 B/lane scratch). It is kept
  // verbatim as the A/B arm (*_sbuf bindings) of the pipelined kernel in
  // flash_attn_bwd_dkv_pipe.hip, which does the same arithmetic and takes
  // the whole backward call at the bench shape from 7.21 to 5.27 ms
  // (profiles/README_dkv_pipeline.md).
  constexpr int BM = 64;
  // bottom-right causal alignment for S_q != S_kv (see flash_attn_fwd.hip)
  const int coff = SKV - SQ;
  constexpr int KP = D + 8;
  constexpr int VP = BM + 8;
  __shared__ __bf16 q_lds[BM * KP];
  __shared__ __bf16 do_lds[BM * KP];
  __shared__ __bf16 dot_lds[D * VP];
  __shared__ __bf16 qt_lds[D * VP];
  __shared__ __bf16 pT_lds[8 * 32 * VP];
  __shared__ __bf16 dsT_lds[8 * 32 * VP];

  const int lane = threadIdx.x & 63;
  const int wid = threadIdx.x >> 6;
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
      // fold the softmax scale into K once (VALU-bound kernel)
#pragma unroll
      for (int j = 0; j < 8; ++j)
        kfrag[sb][kk][j] = (__bf16)((float)kfrag[sb][kk][j] * scale);
    }
  }

  // dV/dK accumulate on 32x32x16 MFMAs (the wave's 32 keys = one C-row
  // block): 25% more FLOP per issue-cycle than 16x16x32 on these pure
  // GEMM chains. kq-outer loop order: per kq the A-frags load once and
  // the 8 MFMAs hit 8 DISTINCT accumulators (no dependent-accumulator
  // back-to-back issue).
  constexpr int DN2 = D / 32;
  f32x16_t dvacc[DN2], dkacc[DN2];
#pragma unroll
  for (int nj = 0; nj < DN2; ++nj) {
    dvacc[nj] = f32x16_t{};
    dkacc[nj] = f32x16_t{};
  }

  const int wkey_min = krow_w;  // first key of this wave

  {
    const int hq = hkv * group + g;
    const bf16* Qp = Q + b * sQb + hq * sQh;
    const bf16* dOp = dO + b * sDb + hq * sDh;
    const float* Lp = LSE + ((long)b * HQ + hq) * SQ;
    const float* Dp = DELTA + ((long)b * HQ + hq) * SQ;

    // causal: first q tile containing a row with qcol + coff >= kbase
    // RANGED: the block's alive keys are [klo, khi); none -> no q tile
    // (the zero accumulators are still stored below)
    const int klo = RANGED ? max(kbase, lo) : kbase;
    const int khi = RANGED ? min(kbase + BN, hi) : kbase + BN;
    const int ib0 = CAUSAL ? max(0, (klo - coff) / BM) : 0;
    int nqb = (SQ + BM - 1) / BM;
    if (CAUSAL && window > 0)
      nqb = min(nqb, (khi - 1 + window - coff + BM - 1) / BM);
    if (RANGED && klo >= khi) nqb = 0;
    // SEGMENTED: no query at or past the end of the block's last key's
    // segment sees any key of the block
    const int* Sp = kv_lo + (long)b * SQ;  // q_start row (SEGMENTED only)
    if constexpr (SEGMENTED)
      nqb = min(nqb,
                (kv_hi[(long)b * SQ + min(kbase + BN, SKV) - 1] + BM - 1) / BM);
    // q_start of the tile's first query, fetched one tile ahead so the
    // wave-skip test below never waits for the load
    int qs_tile_next = 0;
    if constexpr (SEGMENTED)
      if (ib0 < nqb) qs_tile_next = Sp[ib0 * BM];
    for (int ib = ib0; ib < nqb; ++ib) {
      const int qbase = ib * BM;
      const int qs_tile = qs_tile_next;
      if constexpr (SEGMENTED)
        if (ib + 1 < nqb) qs_tile_next = Sp[qbase + BM];
      {  // stage Q, dO row-major (16B) + transposed (paired b32)
        constexpr int KVECS = BM * D / 8;
        for (int t = threadIdx.x; t < KVECS; t += 512) {
          const int row = t / (D / 8);
          const int col8 = (t % (D / 8)) * 8;
          const int gr = qbase + row;
          int4 qv = (gr < SQ) ? *(const int4*)(Qp + (long)gr * sQs + col8)
                              : int4{0, 0, 0, 0};
          int4 dv = (gr < SQ) ? *(const int4*)(dOp + (long)gr * sDs + col8)
                              : int4{0, 0, 0, 0};
          *(int4*)&q_lds[row * KP + col8] = qv;
          *(int4*)&do_lds[row * KP + col8] = dv;
        }
        constexpr int TVECS = BM * D / 16;  // row pairs
        for (int t = threadIdx.x; t < TVECS; t += 512) {
          const int row = (t / (D / 8)) * 2;
          const int col8 = (t % (D / 8)) * 8;
          const int g0 = qbase + row, g1 = g0 + 1;
          int4 q0 = (g0 < SQ) ? *(const int4*)(Qp + (long)g0 * sQs + col8)
                              : int4{0, 0, 0, 0};
          int4 q1 = (g1 < SQ) ? *(const int4*)(Qp + (long)g1 * sQs + col8)
                              : int4{0, 0, 0, 0};
          int4 d0 = (g0 < SQ) ? *(const int4*)(dOp + (long)g0 * sDs + col8)
                              : int4{0, 0, 0, 0};
          int4 d1 = (g1 < SQ) ? *(const int4*)(dOp + (long)g1 * sDs + col8)
                              : int4{0, 0, 0, 0};
          const __bf16 *qe0 = (const __bf16*)&q0, *qe1 = (const __bf16*)&q1;
          const __bf16 *de0 = (const __bf16*)&d0, *de1 = (const __bf16*)&d1;
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            __bf16 qp[2] = {qe0[j], qe1[j]};
            __bf16 dp[2] = {de0[j], de1[j]};
            const int r = col8 + j;
            const uint byte = tr_swz((uint)(r * VP + row) * 2, r);
            *(uint*)((char*)qt_lds + byte) = *(uint*)qp;
            *(uint*)((char*)dot_lds + byte) = *(uint*)dp;
          }
        }
      }
      __syncthreads();

      // causal: skip waves whose keys are all above this q tile
      if ((!CAUSAL || wkey_min <= qbase + BM - 1 + coff) &&
          (!RANGED || (krow_w < hi && krow_w + 32 > lo)) &&
          // SEGMENTED: the wave's keys all lie below the segment of the
          // tile's first (hence every) query
          (!SEGMENTED || krow_w + 32 > qs_tile)) {
        __bf16* pw = &pT_lds[wid * 32 * VP];
        __bf16* dw = &dsT_lds[wid * 32 * VP];
#pragma unroll
        for (int nq = 0; nq < BM / 16; ++nq) {
          f32x4_t st[2], dpt[2];
          st[0] = st[1] = f32x4_t{0.f, 0.f, 0.f, 0.f};
          dpt[0] = dpt[1] = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
          for (int kk = 0; kk < DK; ++kk) {
            bf16x8_t qb =
                load_frag_b_rowmajorT(&q_lds[nq * 16 * KP], KP, kk * 32, lane);
            st[0] = MFMA_16x16x32(kfrag[0][kk], qb, st[0]);
            st[1] = MFMA_16x16x32(kfrag[1][kk], qb, st[1]);
            bf16x8_t db =
                load_frag_b_rowmajorT(&do_lds[nq * 16 * KP], KP, kk * 32, lane);
            dpt[0] = MFMA_16x16x32(vfrag[0][kk], db, dpt[0]);
            dpt[1] = MFMA_16x16x32(vfrag[1][kk], db, dpt[1]);
          }
          const int qcol = qbase + nq * 16 + (lane & 15);
          const float lse = (qcol < SQ) ? Lp[qcol] : 1e30f;
          const float delta = (qcol < SQ) ? Dp[qcol] : 0.f;
          int qs = 0;  // first key visible to qcol
          if constexpr (SEGMENTED) qs = (qcol < SQ) ? Sp[qcol] : 0;
          // interior fast path (the fwd kernel's full_tile analog): every
          // (q, key) of this 16-col x 32-key patch in bounds and causally
          // alive — skip the 3 compare/selects per element (VALU-bound
          // kernel)
          const bool full_patch =
              (!RANGED || (krow_w >= lo && krow_w + 31 < hi)) &&
              // lane 15 holds the patch's last query (largest q_start)
              (!SEGMENTED || krow_w >= __builtin_amdgcn_readlane(qs, 15)) &&
              (qbase + nq * 16 + 15 < SQ) && (krow_w + 31 < SKV) &&
              (!CAUSAL || (qbase + nq * 16 + coff >= krow_w + 31)) &&
              (window <= 0 ||
               (qbase + nq * 16 + 15 + coff < krow_w + window));
          if (full_patch) {
#pragma unroll
            for (int sb = 0; sb < 2; ++sb) {
#pragma unroll
              for (int r = 0; r < 4; ++r) {
                const float p = __expf(st[sb][r] - lse);
                const float ds = p * (dpt[sb][r] - delta) * scale;
                const int lrow = sb * 16 + (lane >> 4) * 4 + r;
                pw[lrow * VP + nq * 16 + (lane & 15)] = (__bf16)p;
                dw[lrow * VP + nq * 16 + (lane & 15)] = (__bf16)ds;
              }
            }
          } else {
#pragma unroll
            for (int sb = 0; sb < 2; ++sb) {
#pragma unroll
              for (int r = 0; r < 4; ++r) {
                const int krow = krow_w + sb * 16 + (lane >> 4) * 4 + r;
                bool dead = (qcol >= SQ) || (krow >= SKV) ||
                            (CAUSAL && qcol + coff < krow);
                if (CAUSAL && window > 0)
                  dead |= (qcol + coff >= krow + window);
                if constexpr (RANGED) dead |= (krow < lo) || (krow >= hi);
                if constexpr (SEGMENTED) dead |= (krow < qs);
                const float p = dead ? 0.f : __expf(st[sb][r] - lse);
                const float ds = p * (dpt[sb][r] - delta) * scale;
                const int lrow = sb * 16 + (lane >> 4) * 4 + r;
                pw[lrow * VP + nq * 16 + (lane & 15)] = (__bf16)p;
                dw[lrow * VP + nq * 16 + (lane & 15)] = (__bf16)ds;
              }
            }
          }
        }
        // dV += P^T dO ; dK += dS^T Q — 32x32x16, contraction in 16-q
        // chunks; A = the wave's own P^T/dS^T strip, loaded once per kq
#pragma unroll
        for (int kq = 0; kq < BM / 16; ++kq) {
          bf16x8_t pa = load_frag_a32(pw, VP, kq * 16, lane);
          bf16x8_t da = load_frag_a32(dw, VP, kq * 16, lane);
#pragma unroll
          for (int nj = 0; nj < DN2; ++nj) {
            bf16x8_t dob =
                load_frag_b32_trT_swz(dot_lds, VP, nj * 32, kq * 16, lane);
            dvacc[nj] = MFMA_32x32x16(pa, dob, dvacc[nj]);
            bf16x8_t qb2 =
                load_frag_b32_trT_swz(qt_lds, VP, nj * 32, kq * 16, lane);
            dkacc[nj] = MFMA_32x32x16(da, qb2, dkacc[nj]);
          }
        }
      }
      __syncthreads();
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

// ============================ dQ ============================
// NSB: 16-row sub-blocks per wave (see flash_fwd_kernel) — NSB=1 keeps
// the chip full at TP=8's HQ_local=4
//
// DROPOUT (DENSE mask only): dS = P . (M * keep_scale . dP - delta) * scale
// with the keep mask M of attn_dropout.h the forward used; LSE and delta
// come from that forward. A lane's four words of a 64-key tile (one per
// 16-key chunk) are generated once per tile and sub-block.
template <int D, bool CAUSAL, int NSB, bool RANGED = false,
          bool SEGMENTED = false, bool DROPOUT = false>
__global__ __launch_bounds__(512) void flash_bwd_dq_kernel(
    const bf16* __restrict__ dO, const bf16* __restrict__ Q,
    const bf16* __restrict__ K, const bf16* __restrict__ V,
    const float* __restrict__ LSE, const float* __restrict__ DELTA,
    bf16* __restrict__ dQ,  // [s, b, hq, d] contiguous
    int SQ, int SKV, int Bb, int HQ, int HKV, float scale, int window,
    long sQs, long sQb, long sQh, long sKs, long sKb, long sKh, long sVs,
    long sVb, long sVh, long sDs, long sDb, long sDh,
    const int* __restrict__ kv_lo = nullptr,  // [B] int32 (RANGED), or
    const int* __restrict__ kv_hi = nullptr,  // [B, S] (SEGMENTED)
    int drop_t = 0,  // DROPOUT: threshold 1..255 and the random stream
    unsigned long long drop_seed = 0, unsigned long long drop_off = 0) {
  static_assert(!(RANGED && SEGMENTED), "one mask mode at a time");
  static_assert(!SEGMENTED || CAUSAL, "segments are causal");
  static_assert(!DROPOUT || !(RANGED || SEGMENTED), "dropout: DENSE only");
  constexpr int BM = NSB * 128, BN = 64;  // BN=32 (2 blk/CU) was slower
  const int coff = SKV - SQ;  // bottom-right causal alignment
  constexpr int KP = D + 8;
  constexpr int VP = BN + 8;
  // double-buffered K/V/K^T staging: tile jb+1 streams global->LDS into
  // the other buffer set DURING tile jb's MFMAs, and each tile needs one
  // barrier instead of two (the kernel was already 1 block/CU at 90 KB,
  // so the extra LDS costs no occupancy)
  __shared__ __bf16 k_lds[2][BN * KP];
  __shared__ __bf16 v_lds[2][BN * KP];
  __shared__ __bf16 kt_lds[2][D * VP];
  __shared__ __bf16 ds_lds[8 * NSB * 16 * VP];

  const int lane = threadIdx.x & 63;
  const int wid = threadIdx.x >> 6;
  int qblock, bh;  // b * HQ + hq
  xcd_remap(qblock, bh);
  const int hq = bh % HQ;
  const int b = bh / HQ;
  const int hkv = hq / (HQ / HKV);
  // wave-uniform visible key range of this batch row
  int lo = 0, hi = SKV;
  if constexpr (RANGED) {
    lo = kv_lo[b];
    hi = kv_hi[b];
  }

  const bf16* Qp = Q + b * sQb + hq * sQh;
  const bf16* dOp = dO + b * sDb + hq * sDh;
  const bf16* Kp = K + b * sKb + hkv * sKh;
  const bf16* Vp = V + b * sVb + hkv * sVh;
  const float* Lp = LSE + ((long)b * HQ + hq) * SQ;
  const float* Dp = DELTA + ((long)b * HQ + hq) * SQ;

  const int q0 = qblock * BM;
  const int qrow_w = q0 + wid * NSB * 16;

  constexpr int DK = D / 32;
  bf16x8_t qfrag[NSB][DK], dofrag[NSB][DK];
  float lse[NSB][4], delta[NSB][4];
  // SEGMENTED: first visible key of each of the lane's 4*NSB rows, of the
  // wave's last row (full_patch) and of its first row (tile skip)
  int qs[NSB][4], qs_last = 0, qs_wave = 0;
  if constexpr (SEGMENTED) {
    const int* Sp = kv_lo + (long)b * SQ;
    qs_wave = Sp[min(qrow_w, SQ - 1)];
    qs_last = Sp[min(qrow_w + NSB * 16 - 1, SQ - 1)];
#pragma unroll
    for (int sb = 0; sb < NSB; ++sb)
#pragma unroll
      for (int rr = 0; rr < 4; ++rr)
        qs[sb][rr] = Sp[min(qrow_w + sb * 16 + (lane >> 4) * 4 + rr, SQ - 1)];
  }
#pragma unroll
  for (int sb = 0; sb < NSB; ++sb) {
    const int r = qrow_w + sb * 16 + (lane & 15);
    const long row = (r < SQ) ? r : (SQ - 1);
#pragma unroll
    for (int kk = 0; kk < DK; ++kk) {
      *(int4*)&qfrag[sb][kk] =
          *(const int4*)(Qp + row * sQs + kk * 32 + (lane >> 4) * 8);
      *(int4*)&dofrag[sb][kk] =
          *(const int4*)(dOp + row * sDs + kk * 32 + (lane >> 4) * 8);
      // fold the softmax scale into Q once (VALU-bound kernel)
#pragma unroll
      for (int j = 0; j < 8; ++j)
        qfrag[sb][kk][j] = (__bf16)((float)qfrag[sb][kk][j] * scale);
    }
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) {
      const int qrow = qrow_w + sb * 16 + (lane >> 4) * 4 + rr;
      lse[sb][rr] = (qrow < SQ) ? Lp[qrow] : 1e30f;
      delta[sb][rr] = (qrow < SQ) ? Dp[qrow] : 0.f;
    }
  }

  // NSB==2: dQ accumulates on 32x32x16 MFMAs (wave's 32 q-rows = one
  // C block, distinct accumulators back-to-back); NSB==1 waves hold
  // only 16 rows and stay on 16x16x32.
  constexpr int DN = D / 16;
  constexpr int DN2 = D / 32;
  f32x4_t dqacc[NSB == 1 ? NSB : 1][NSB == 1 ? DN : 1];
  f32x16_t dqacc32[NSB == 2 ? DN2 : 1];
  if constexpr (NSB == 1) {
#pragma unroll
    for (int sb = 0; sb < NSB; ++sb)
#pragma unroll
      for (int nj = 0; nj < DN; ++nj)
        dqacc[sb][nj] = f32x4_t{0.f, 0.f, 0.f, 0.f};
  } else {
#pragma unroll
    for (int nj = 0; nj < DN2; ++nj) dqacc32[nj] = f32x16_t{};
  }

  int kend = CAUSAL ? min(SKV, q0 + BM + coff) : SKV;
  if constexpr (RANGED) kend = min(kend, hi);
  const int nkb = (kend + BN - 1) / BN;
  int jb0 =
      (CAUSAL && window > 0) ? max(0, (q0 + coff - window + 1) / BN) : 0;
  // tiles wholly below lo are skipped; jb0 >= nkb leaves the loop empty
  // and the zero dQ accumulators are stored
  if constexpr (RANGED) jb0 = max(jb0, lo / BN);
  // SEGMENTED: no row of the tile sees a key below its first row's segment
  if constexpr (SEGMENTED) jb0 = max(jb0, kv_lo[(long)b * SQ + q0] / BN);
  const int wrow_max = qrow_w + NSB * 16 - 1;

  auto stage_kv = [&](int jb, int buf) {
    const int kbase = jb * BN;
    constexpr int KVECS = BN * D / 8;
    for (int t = threadIdx.x; t < KVECS; t += 512) {
      const int row = t / (D / 8);
      const int col8 = (t % (D / 8)) * 8;
      const int gr = kbase + row;
      int4 kv = (gr < SKV) ? *(const int4*)(Kp + (long)gr * sKs + col8)
                           : int4{0, 0, 0, 0};
      int4 vv = (gr < SKV) ? *(const int4*)(Vp + (long)gr * sVs + col8)
                           : int4{0, 0, 0, 0};
      *(int4*)&k_lds[buf][row * KP + col8] = kv;
      *(int4*)&v_lds[buf][row * KP + col8] = vv;
    }
    constexpr int TVECS = BN * D / 16;
    for (int t = threadIdx.x; t < TVECS; t += 512) {
      const int row = (t / (D / 8)) * 2;
      const int col8 = (t % (D / 8)) * 8;
      const int g0 = kbase + row, g1 = g0 + 1;
      int4 k0 = (g0 < SKV) ? *(const int4*)(Kp + (long)g0 * sKs + col8)
                           : int4{0, 0, 0, 0};
      int4 k1 = (g1 < SKV) ? *(const int4*)(Kp + (long)g1 * sKs + col8)
                           : int4{0, 0, 0, 0};
      const __bf16 *e0 = (const __bf16*)&k0, *e1 = (const __bf16*)&k1;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        __bf16 pr[2] = {e0[j], e1[j]};
        const int r = col8 + j;
        *(uint*)((char*)kt_lds[buf] + tr_swz((uint)(r * VP + row) * 2, r)) =
            *(uint*)pr;
      }
    }
  };

  stage_kv(jb0, jb0 & 1);
  __syncthreads();

  for (int jb = jb0; jb < nkb; ++jb) {
    const int kbase = jb * BN;
    const int cur = jb & 1;
    // stream tile jb+1 into the other buffer set (last read before the
    // barrier that ended tile jb-1) while this tile's MFMAs run
    if (jb + 1 < nkb) stage_kv(jb + 1, cur ^ 1);

    if ((!CAUSAL || kbase <= wrow_max + coff) &&
        (!SEGMENTED || kbase + BN > qs_wave)) {
      __bf16* dsw = &ds_lds[wid * NSB * 16 * VP];
      // DROPOUT: word nk of a call is key kbase + nk * 16 + (lane & 15)
      DropWords dw[NSB];
      float kscale = 1.f;
      if constexpr (DROPOUT) {
        kscale = dropout_keep_scale(drop_t);
#pragma unroll
        for (int sb = 0; sb < NSB; ++sb)
          dw[sb] = dropout_words(
              drop_seed, drop_off, (uint)bh,
              (uint)(qrow_w + sb * 16 + (lane >> 4) * 4) >> 2,
              dropout_key_group(kbase + (lane & 15)));
      }
#pragma unroll
      for (int nk = 0; nk < BN / 16; ++nk) {
        f32x4_t st[NSB], dpt[NSB];
#pragma unroll
        for (int sb = 0; sb < NSB; ++sb) {
          st[sb] = f32x4_t{0.f, 0.f, 0.f, 0.f};
          dpt[sb] = f32x4_t{0.f, 0.f, 0.f, 0.f};
        }
#pragma unroll
        for (int kk = 0; kk < DK; ++kk) {
          bf16x8_t kb = load_frag_b_rowmajorT(&k_lds[cur][nk * 16 * KP],
                                              KP, kk * 32, lane);
#pragma unroll
          for (int sb = 0; sb < NSB; ++sb)
            st[sb] = MFMA_16x16x32(qfrag[sb][kk], kb, st[sb]);
          bf16x8_t vb = load_frag_b_rowmajorT(&v_lds[cur][nk * 16 * KP],
                                              KP, kk * 32, lane);
#pragma unroll
          for (int sb = 0; sb < NSB; ++sb)
            dpt[sb] = MFMA_16x16x32(dofrag[sb][kk], vb, dpt[sb]);
        }
        const int kcol = kbase + nk * 16 + (lane & 15);
        // interior fast path: whole 32-row x 16-key patch alive (see dkv)
        const bool full_patch =
            (!RANGED ||
             (kbase + nk * 16 >= lo && kbase + nk * 16 + 15 < hi)) &&
            (!SEGMENTED || kbase + nk * 16 >= qs_last) &&
            (kbase + nk * 16 + 15 < SKV) &&
            (!CAUSAL || (kbase + nk * 16 + 15 <= qrow_w + coff)) &&
            (window <= 0 || (kbase + nk * 16 > qrow_w + 31 + coff - window));
        if (full_patch) {
#pragma unroll
          for (int sb = 0; sb < NSB; ++sb) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              const float p = __expf(st[sb][r] - lse[sb][r]);
              float dp = dpt[sb][r];
              if constexpr (DROPOUT)
                dp = dropout_keep_byte(dw[sb].w[nk], r, drop_t) ? dp * kscale
                                                                : 0.f;
              const float ds = p * (dp - delta[sb][r]) * scale;
              dsw[(sb * 16 + (lane >> 4) * 4 + r) * VP + nk * 16 +
                  (lane & 15)] = (__bf16)ds;
            }
          }
        } else {
#pragma unroll
          for (int sb = 0; sb < NSB; ++sb) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              const int qrow = qrow_w + sb * 16 + (lane >> 4) * 4 + r;
              bool dead = (kcol >= SKV) || (CAUSAL && kcol > qrow + coff);
              if (CAUSAL && window > 0)
                dead |= (kcol <= qrow + coff - window);
              if constexpr (RANGED) dead |= (kcol < lo) || (kcol >= hi);
              if constexpr (SEGMENTED) dead |= (kcol < qs[sb][r]);
              const float p = dead ? 0.f : __expf(st[sb][r] - lse[sb][r]);
              float dp = dpt[sb][r];
              if constexpr (DROPOUT)
                dp = dropout_keep_byte(dw[sb].w[nk], r, drop_t) ? dp * kscale
                                                                : 0.f;
              const float ds = p * (dp - delta[sb][r]) * scale;
              dsw[(sb * 16 + (lane >> 4) * 4 + r) * VP + nk * 16 +
                  (lane & 15)] = (__bf16)ds;
            }
          }
        }
      }
      if constexpr (NSB == 1) {
#pragma unroll
        for (int nj = 0; nj < DN; ++nj) {
#pragma unroll
          for (int kk = 0; kk < BN / 32; ++kk) {
            bf16x8_t kb2 =
                load_frag_b_trT_swz(kt_lds[cur], VP, nj * 16, kk * 32, lane);
            bf16x8_t da = load_frag_a(dsw, VP, kk * 32, lane);
            dqacc[0][nj] = MFMA_16x16x32(da, kb2, dqacc[0][nj]);
          }
        }
      } else {
#pragma unroll
        for (int kq = 0; kq < BN / 16; ++kq) {
          bf16x8_t da = load_frag_a32(dsw, VP, kq * 16, lane);
#pragma unroll
          for (int nj = 0; nj < DN2; ++nj) {
            bf16x8_t kb2 = load_frag_b32_trT_swz(kt_lds[cur], VP, nj * 32,
                                                 kq * 16, lane);
            dqacc32[nj] = MFMA_32x32x16(da, kb2, dqacc32[nj]);
          }
        }
      }
    }
    __syncthreads();  // tile jb reads done AND tile jb+1 stage visible
  }

  const long sOs = (long)Bb * HQ * D;
  bf16* dQp = dQ + ((long)b * HQ + hq) * D;
  if constexpr (NSB == 1) {
#pragma unroll
    for (int nj = 0; nj < DN; ++nj)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int qrow = qrow_w + (lane >> 4) * 4 + r;
        if (qrow < SQ)
          dQp[(long)qrow * sOs + nj * 16 + (lane & 15)] =
              f2bf(dqacc[0][nj][r]);
      }
  } else {
#pragma unroll
    for (int nj = 0; nj < DN2; ++nj)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int qrow = qrow_w + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
        if (qrow < SQ)
          dQp[(long)qrow * sOs + nj * 32 + (lane & 31)] =
              f2bf(dqacc32[nj][r]);
      }
  }
}

// ===================== delta = rowsum(dO . O) =====================
// One wave per (b, h, s) row: fused bf16 reads, fp32 dot, no fp32
// materialization of dO/O (the torch expression cast+mul+sum moved
// ~3.5 GB per call at the bench shape).
template <int D>
__global__ __launch_bounds__(256) void attn_delta_kernel(
    const bf16* __restrict__ dO, const bf16* __restrict__ O,
    float* __restrict__ DELTA, int SQ, int Bb, int HQ, long sDs, long sDb,
    long sDh, long sOs, long sOb, long sOh) {
  const int lane = threadIdx.x & 63;
  const long row = ((long)blockIdx.x * 4 + (threadIdx.x >> 6));
  const long total = (long)SQ * Bb * HQ;
  if (row >= total) return;
  // row order matches DELTA [b][h][s]
  const int s = (int)(row % SQ);
  const int h = (int)((row / SQ) % HQ);
  const int b = (int)(row / ((long)SQ * HQ));
  const bf16* dp = dO + b * sDb + h * sDh + s * sDs;
  const bf16* op = O + b * sOb + h * sOh + s * sOs;
  float acc = 0.f;
#pragma unroll
  for (int j = 0; j < D / 64; ++j) {
    const int c = lane + j * 64;
    acc += bf2f(dp[c]) * bf2f(op[c]);
  }
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) acc += __shfl_xor(acc, off, 64);
  if (lane == 0) DELTA[row] = acc;
}

extern "C" {
void launch_attn_delta(const void* dout, const void* o, void* delta, int SQ,
                       int B, int HQ, int D, const long* dstr,
                       const long* ostr, hipStream_t stream) {
  long total = (long)SQ * B * HQ;
  dim3 grid((unsigned)((total + 3) / 4));
  dim3 blk(256);
  if (D == 128)
    attn_delta_kernel<128><<<grid, blk, 0, stream>>>(
        (const bf16*)dout, (const bf16*)o, (float*)delta, SQ, B, HQ, dstr[0],
        dstr[1], dstr[2], ostr[0], ostr[1], ostr[2]);
  else if (D == 64)
    attn_delta_kernel<64><<<grid, blk, 0, stream>>>(
        (const bf16*)dout, (const bf16*)o, (float*)delta, SQ, B, HQ, dstr[0],
        dstr[1], dstr[2], ostr[0], ostr[1], ostr[2]);
}

// dK/dV by one of the two kernels (pipe = true: the pipelined kernel of
// flash_attn_bwd_dkv_pipe.hip, the default; false: flash_bwd_dkv_kernel
// above, the A/B arm, bit-equal), then dQ, the same kernel in both.
void launch_flash_bwd(const FlashArgs& a, bool pipe, hipStream_t stream) {
  const dim3 blk(512);
  // the single-buffered dK/dV kernel has no dropout instantiation (its lanes
  // hold one query x four keys, the transpose of the random words' footprint)
  if (pipe || a.drop_t > 0) {
    launch_flash_dkv_pipe(a, stream);
  } else {
    // one block per (kblock, b, hkv, g)
    const dim3 gkv((a.SKV + 255) / 256, a.B * a.HQ);
    dispatch_flash(a, [&](auto d, auto c, auto r, auto s) {
      flash_bwd_dkv_kernel<decltype(d)::value, decltype(c)::value,
                           decltype(r)::value, decltype(s)::value>
          <<<gkv, blk, 0, stream>>>(
              (const bf16*)a.dout, (const bf16*)a.q, (const bf16*)a.k,
              (const bf16*)a.v, (const float*)a.lse, (const float*)a.delta,
              (float*)a.dk, (float*)a.dv, a.SQ, a.SKV, a.B, a.HQ, a.HKV,
              a.scale, a.window, a.qs[0], a.qs[1], a.qs[2], a.ks[0], a.ks[1],
              a.ks[2], a.vs[0], a.vs[1], a.vs[2], a.ds[0], a.ds[1], a.ds[2],
              a.bound_a, a.bound_b);
    });
  }
  const int bm = flash_block_rows(a.SQ, a.B * a.HQ);
  const dim3 gq((a.SQ + bm - 1) / bm, a.B * a.HQ);
  dispatch_flash_drop(a, [&](auto d, auto c, auto r, auto s, auto p) {
    constexpr int D = decltype(d)::value;
    constexpr bool C = decltype(c)::value, R = decltype(r)::value,
                   S = decltype(s)::value, P = decltype(p)::value;
    auto kern = bm == 128 ? flash_bwd_dq_kernel<D, C, 1, R, S, P>
                          : flash_bwd_dq_kernel<D, C, 2, R, S, P>;
    kern<<<gq, blk, 0, stream>>>(
        (const bf16*)a.dout, (const bf16*)a.q, (const bf16*)a.k,
        (const bf16*)a.v, (const float*)a.lse, (const float*)a.delta,
        (bf16*)a.dq, a.SQ, a.SKV, a.B, a.HQ, a.HKV, a.scale, a.window,
        a.qs[0], a.qs[1], a.qs[2], a.ks[0], a.ks[1], a.ks[2], a.vs[0],
        a.vs[1], a.vs[2], a.ds[0], a.ds[1], a.ds[2], a.bound_a, a.bound_b,
        a.drop_t, a.drop_seed, a.drop_offset);
  });
}
}
