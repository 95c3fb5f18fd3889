// DOUBLE-BUFFERED variant of flash_fwd_kernel, the default forward (the
// single-buffered kernel stays reachable for A/B as the flash_attn_fwd_sbuf
// binding; bit-identical output): two K/V LDS buffer sets -> ONE barrier
// per tile and the staging writes overlap the previous tile's MFMAs.
// LDS 108.5 KB -> 1 block/CU (8 waves) vs the single-buffered kernel's 2
// blocks; measured +3.0% (bench shape) / +1.8% (TP=8 shape).
#include "attn_common.h"
#include "attn_dropout.h"
#include "flash_dispatch.h"

// NSB = 16-row sub-blocks per wave: 2 -> BM 256 (the TP<=4 shape), 1 ->
// BM 128 for small B*HQ launches (TP=8 has HQ_local=4: BM=256 gives 256
// blocks = 1/CU on the bench shape — half the chip idles).
//
// RANGED: per-batch-row visible key range [kv_lo[b], kv_hi[b]) on top of
// the causal / window mask (padded batches: one contiguous run of real
// tokens per row). Key-side only; a query row with no alive key stores
// O = 0 and a finite LSE. The dense instantiations (RANGED=false) compile
// exactly as before and never read kv_lo / kv_hi.
//
// SEGMENTED: packed sequences, block-diagonal causal mask (S_q == S_kv).
// The same two pointers then carry per-token int32 [B, S] bounds instead:
// kv_lo = q_start (first key query i may see = start of its segment) and
// kv_hi = k_end (unused here; the dK/dV kernel bounds its q loop with it).
// q_start is non-decreasing along a row, so a tile's bounds come from its
// first / last row. Every query sees itself: no empty rows.

// DROPOUT (DENSE mask only): O = ((P . M) V) * keep_scale / l with the keep
// mask M of attn_dropout.h; l and LSE are those of the undropped softmax.
// The dropped P goes to p_lds, so the ones-fragment MFMA over p_lds would
// sum the wrong thing: these instantiations instead add the fp32 p into a
// per-lane partial of l (alpha is uniform over the 16 lanes that share a
// row, so the partials rescale like l itself) and reduce it across those
// lanes once, in the epilogue. The other instantiations compile as before.

// LDS home of the q_start values of a block's N query rows. The buffer
// exists only in kernels that call this (the SEGMENTED ones), so the other
// instantiations keep their LDS size.
template <int N>
__device__ __forceinline__ int* seg_bounds_lds() {
  __shared__ __attribute__((aligned(16))) int buf[N];
  return buf;
}

template <int D, bool CAUSAL, int NSB, bool RANGED = false,
          bool SEGMENTED = false, bool DROPOUT = false>
__global__ __launch_bounds__(512) void flash_fwd_dbuf_kernel(
    const bf16* __restrict__ Q, const bf16* __restrict__ K,
    const bf16* __restrict__ V, bf16* __restrict__ O,
    float* __restrict__ LSE,  // [B, HQ, SQ] f32
    int SQ, int SKV, int Bb, int HQ, int HKV, float scale,
    int window,                     // sliding window (<=0: disabled)
    long sQs, long sQb, long sQh,   // Q element strides (seq, batch, head)
    long sKs, long sKb, long sKh,   // K strides
    long sVs, long sVb, long sVh,   // V strides
    const int* __restrict__ kv_lo = nullptr,   // [B] int32 (RANGED), or
    const int* __restrict__ kv_hi = nullptr,   // [B, S] (SEGMENTED)
    int drop_t = 0,  // DROPOUT: threshold 1..255 and the random stream
    unsigned long long drop_seed = 0, unsigned long long drop_off = 0) {
  static_assert(!(RANGED && SEGMENTED), "one mask mode at a time");
  static_assert(!SEGMENTED || CAUSAL, "segments are causal");
  static_assert(!DROPOUT || !(RANGED || SEGMENTED), "dropout: DENSE only");
  constexpr int BM = NSB * 128, BN = 64;
  constexpr int KP = D + 8;
  constexpr int VP = BN + 8;
  __shared__ __bf16 k_lds[2][BN * KP];
  __shared__ __bf16 vt_lds[2][D * VP];
  __shared__ __bf16 p_lds[8 * NSB * 16 * VP];

  const int lane = threadIdx.x & 63;
  const int wid = threadIdx.x >> 6;
  int qblock, bh;  // b * HQ + hq
  xcd_remap(qblock, bh);
  const int hq = bh % HQ;
  const int b = bh / HQ;
  const int hkv = hq / (HQ / HKV);
  // S_q != S_kv: causal is BOTTOM-RIGHT aligned (query i sees keys
  // j <= i + SKV - SQ) — the KV-cache decode / ring half-block convention
  const int coff = SKV - SQ;
  // wave-uniform visible key range of this batch row
  int lo = 0, hi = SKV;
  if constexpr (RANGED) {
    lo = kv_lo[b];
    hi = kv_hi[b];
  }

  const bf16* Qp = Q + b * sQb + hq * sQh;
  const bf16* Kp = K + b * sKb + hkv * sKh;
  const bf16* Vp = V + b * sVb + hkv * sVh;

  const int q0 = qblock * BM;
  const int qrow_w = q0 + wid * NSB * 16;  // first row of this wave

  constexpr int DK = D / 32;
  bf16x8_t qfrag[NSB][DK];
#pragma unroll
  for (int sb = 0; sb < NSB; ++sb) {
    const int r = qrow_w + sb * 16 + (lane & 15);
    const long row = (r < SQ) ? r : (SQ - 1);
#pragma unroll
    for (int kk = 0; kk < DK; ++kk) {
      const bf16* p = Qp + row * sQs + kk * 32 + (lane >> 4) * 8;
      *(int4*)&qfrag[sb][kk] = *(const int4*)p;
      // fold the softmax scale into Q once (saves a VALU mul per score
      // per tile; PMC: these kernels are VALU-bound at ~8 VALU/MFMA)
#pragma unroll
      for (int j = 0; j < 8; ++j)
        qfrag[sb][kk][j] = (__bf16)((float)qfrag[sb][kk][j] * scale);
    }
  }

  // SEGMENTED: first visible key of the last row of each sub-block
  // (full_tile) and of the wave's first row (tiles wholly below it are
  // skipped by the whole wave), wave-uniform. The per-row bounds of the
  // block's BM rows sit in LDS and are read by masked tiles only: held in
  // 4*NSB VGPRs per lane they pushed the D=128 / BM=256 instantiation to
  // its 256-VGPR budget and cost the one-segment forward 11% over dense.
  int qs_last[NSB], qs_wave = 0;
  int* qs_lds = nullptr;
  if constexpr (SEGMENTED) {
    const int* Sp = kv_lo + (long)b * SQ;
    qs_wave = Sp[min(qrow_w, SQ - 1)];
#pragma unroll
    for (int sb = 0; sb < NSB; ++sb)
      qs_last[sb] = Sp[min(qrow_w + sb * 16 + 15, SQ - 1)];
    qs_lds = seg_bounds_lds<BM>();
    // visible after the barrier that follows the first K/V stage
    if (threadIdx.x < BM)
      qs_lds[threadIdx.x] = Sp[min(q0 + (int)threadIdx.x, SQ - 1)];
  }

  float m_i[NSB][4], l_i[NSB][4];
  float alpha_s[NSB][4];
  // all-ones B fragment: one MFMA per 32-key chunk computes the P row-sums
  // into every lane's accumulator (replaces 16 adds + 16 shuffles per
  // sub-block of VALU reduction)
  bf16x8_t ones_frag;
#pragma unroll
  for (int j = 0; j < 8; ++j) ones_frag[j] = (__bf16)1.0f;
  constexpr int DN = D / 16;
  f32x4_t oacc[NSB][DN];
#pragma unroll
  for (int sb = 0; sb < NSB; ++sb) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      m_i[sb][r] = -1e30f;
      l_i[sb][r] = 0.f;
    }
#pragma unroll
    for (int nj = 0; nj < DN; ++nj) oacc[sb][nj] = f32x4_t{0.f, 0.f, 0.f, 0.f};
  }

  int kend = CAUSAL ? min(SKV, q0 + BM + coff) : SKV;
  if constexpr (RANGED) kend = min(kend, hi);
  const int nkb = (kend + BN - 1) / BN;
  int jb0 =
      (CAUSAL && window > 0) ? max(0, (q0 + coff - window + 1) / BN) : 0;
  // tiles wholly below lo are skipped; jb0 >= nkb (no alive tile) leaves
  // the loop empty and the epilogue stores O = 0 / LSE = -1e30
  if constexpr (RANGED) jb0 = max(jb0, lo / BN);
  // SEGMENTED: no row of the tile sees a key below its first row's segment
  if constexpr (SEGMENTED) jb0 = max(jb0, kv_lo[(long)b * SQ + q0] / BN);
  const int wrow_max = qrow_w + NSB * 16 - 1;

  // T5 static form: the younger dispatch half gets priority so it is not
  // starved of VALU issue at segment starts (guide §5.5 T5).
  if (__builtin_amdgcn_readfirstlane(threadIdx.x) >= 256)
    __builtin_amdgcn_s_setprio(1);

  // T14 async-stage split: issue tile t+1's global loads into registers
  // BEFORE computing tile t (HBM latency hides under the MFMAs) and write
  // them to LDS only after the end-of-tile barrier (guide §5.5 T14/G15).
  // Per-thread staging registers: K = 2 int4 rows-slices, V = 1 row-pair.
  constexpr int KV_PER_THR = BN * D / 8 / 512;  // int4 K vectors / thread
  int4 kreg[KV_PER_THR];
  int4 vreg0, vreg1;
  // V stages as BN*D/16 row-pair slices, one per thread: all 512 threads
  // at D=128, only the first 256 at D=64 (the rest would fetch rows past
  // the tile and write them over the V^T image)
  constexpr int V_SLICES = BN * D / 16;
  static_assert(V_SLICES <= 512, "one V row-pair slice per thread");
  const bool v_stager = (V_SLICES == 512) || (threadIdx.x < V_SLICES);

  auto issue_loads = [&](int kbase) {
#pragma unroll
    for (int u = 0; u < KV_PER_THR; ++u) {
      const int t = threadIdx.x + u * 512;
      const int row = t / (D / 8);
      const int col8 = (t % (D / 8)) * 8;
      const int gr = kbase + row;
      kreg[u] = (gr < SKV) ? *(const int4*)(Kp + (long)gr * sKs + col8)
                           : int4{0, 0, 0, 0};
    }
    if (v_stager) {
      const int t = threadIdx.x;
      const int row = (t / (D / 8)) * 2;
      const int col8 = (t % (D / 8)) * 8;
      const int g0 = kbase + row, g1 = g0 + 1;
      vreg0 = (g0 < SKV) ? *(const int4*)(Vp + (long)g0 * sVs + col8)
                         : int4{0, 0, 0, 0};
      vreg1 = (g1 < SKV) ? *(const int4*)(Vp + (long)g1 * sVs + col8)
                         : int4{0, 0, 0, 0};
    }
  };

  auto write_lds = [&](int buf) {
#pragma unroll
    for (int u = 0; u < KV_PER_THR; ++u) {
      const int t = threadIdx.x + u * 512;
      const int row = t / (D / 8);
      const int col8 = (t % (D / 8)) * 8;
      *(int4*)&k_lds[buf][row * KP + col8] = kreg[u];
    }
    if (v_stager) {
      const int t = threadIdx.x;
      const int row = (t / (D / 8)) * 2;
      const int col8 = (t % (D / 8)) * 8;
      const __bf16* e0 = (const __bf16*)&vreg0;
      const __bf16* e1 = (const __bf16*)&vreg1;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        __bf16 pair[2] = {e0[j], e1[j]};
        const int r = col8 + j;
        *(uint*)((char*)vt_lds[buf] + tr_swz((uint)(r * VP + row) * 2, r)) =
            *(uint*)pair;
      }
    }
  };

  issue_loads(jb0 * BN);
  write_lds(jb0 & 1);
  __syncthreads();

  for (int jb = jb0; jb < nkb; ++jb) {
    const int kbase = jb * BN;
    const int cur = jb & 1;
    if (jb + 1 < nkb) issue_loads((jb + 1) * BN);

    if ((!CAUSAL || kbase <= wrow_max + coff) &&
        (!SEGMENTED || kbase + BN > qs_wave)) {
      // ---- S = Q K^T for both sub-blocks (B-frags loaded once) ----
      f32x4_t sacc[NSB][4];
#pragma unroll
      for (int nk = 0; nk < 4; ++nk) {
#pragma unroll
        for (int sb = 0; sb < NSB; ++sb)
          sacc[sb][nk] = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int kk = 0; kk < DK; ++kk) {
          bf16x8_t bfrag =
              load_frag_b_rowmajorT(&k_lds[cur][nk * 16 * KP], KP, kk * 32, lane);
#pragma unroll
          for (int sb = 0; sb < NSB; ++sb)
            sacc[sb][nk] = MFMA_16x16x32(qfrag[sb][kk], bfrag, sacc[sb][nk]);
        }
      }
      // ---- mask + online softmax + P→LDS, per sub-block ----
      __bf16* pw = &p_lds[wid * NSB * 16 * VP];
#pragma unroll
      for (int sb = 0; sb < NSB; ++sb) {
        // interior tiles (every key visible to every row) skip the mask
        const bool full_tile =
            (!RANGED || (kbase >= lo && kbase + BN <= hi)) &&
            (!SEGMENTED || kbase >= qs_last[sb]) &&
            (kbase + BN <= SKV) &&
            (!CAUSAL || (kbase + BN - 1 <= qrow_w + sb * 16 + coff)) &&
            (window <= 0 || kbase >= qrow_w + sb * 16 + coff + 15 - window + 1);
        float tile_max[4] = {-1e30f, -1e30f, -1e30f, -1e30f};
        float sv[4][4];
        if (full_tile) {
#pragma unroll
          for (int nk = 0; nk < 4; ++nk) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              const float s = sacc[sb][nk][r];  // scale folded into Q
              sv[nk][r] = s;
              tile_max[r] = fmaxf(tile_max[r], s);
            }
          }
        } else {
          int qs[4] = {0, 0, 0, 0};  // first visible key of the lane's rows
          if constexpr (SEGMENTED)
            *(int4*)qs = *(const int4*)&qs_lds[(wid * NSB + sb) * 16 +
                                               (lane >> 4) * 4];
#pragma unroll
          for (int nk = 0; nk < 4; ++nk) {
            const int kcol = kbase + nk * 16 + (lane & 15);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              const int qrow = qrow_w + sb * 16 + (lane >> 4) * 4 + r;
              float s = sacc[sb][nk][r];  // scale folded into Q
              bool dead = (kcol >= SKV) || (CAUSAL && kcol > qrow + coff);
              if (CAUSAL && window > 0) dead |= (kcol <= qrow + coff - window);
              if constexpr (RANGED) dead |= (kcol < lo) || (kcol >= hi);
              if constexpr (SEGMENTED) dead |= (kcol < qs[r]);
              // SEGMENTED: a row whose segment starts above the first tile
              // its wave visits sees fully dead tiles while m_i is still
              // -1e30, and exp(-1e30 - m_i) would be 1. Dead scores are
              // -inf there instead: m_i stays finite (tile_max starts at
              // -1e30), so p = exp(-inf) = 0 exactly with no select in the
              // exp loop, which runs on every tile (a select there cost
              // the one-segment forward 17% over dense).
              s = dead ? (SEGMENTED ? -__builtin_inff() : -1e30f) : s;
              sv[nk][r] = s;
              tile_max[r] = fmaxf(tile_max[r], s);
            }
          }
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
#pragma unroll
          for (int off = 1; off < 16; off <<= 1)
            tile_max[r] = fmaxf(tile_max[r], __shfl_xor(tile_max[r], off, 64));
        }
        // rescale is EXACTLY the identity when no row's max grew — skip
        // the alpha exps and the O/l rescale entirely then (wave-uniform
        // vote; most interior tiles after the first few don't move m).
        bool grew = false;
#pragma unroll
        for (int r = 0; r < 4; ++r) grew |= tile_max[r] > m_i[sb][r];
        if (__builtin_amdgcn_ballot_w64(grew) != 0ull) {
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const float mn = fmaxf(m_i[sb][r], tile_max[r]);
            alpha_s[sb][r] = __expf(m_i[sb][r] - mn);
            m_i[sb][r] = mn;
          }
#pragma unroll
          for (int nj = 0; nj < DN; ++nj) {
#pragma unroll
            for (int r = 0; r < 4; ++r) oacc[sb][nj][r] *= alpha_s[sb][r];
          }
        } else {
#pragma unroll
          for (int r = 0; r < 4; ++r) alpha_s[sb][r] = 1.0f;
        }
        // DROPOUT: this lane's four keys of the tile (kbase + nk * 16 +
        // (lane & 15)) x its four queries are the four words of one call;
        // generated here, per sub-block, and dead after the loop below
        DropWords dw;
        if constexpr (DROPOUT) {
          dw = dropout_words(
              drop_seed, drop_off, (uint)bh,
              (uint)(qrow_w + sb * 16 + (lane >> 4) * 4) >> 2,
              dropout_key_group(kbase + (lane & 15)));
#pragma unroll
          for (int r = 0; r < 4; ++r) l_i[sb][r] *= alpha_s[sb][r];
        }
#pragma unroll
        for (int nk = 0; nk < 4; ++nk) {
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            float p = __expf(sv[nk][r] - m_i[sb][r]);
            if constexpr (DROPOUT) {
              l_i[sb][r] += p;  // lane partial of the undropped row sum
              p = dropout_keep_byte(dw.w[nk], r, drop_t) ? p : 0.f;
            }
            // a row with no alive key yet still has m_i = -1e30, so its
            // dead entries would get exp(0) = 1 (dense causal rows always
            // see themselves; rows below lo do not) — force them to 0.
            // (SEGMENTED meets the same trap and avoids it with s = -inf
            // on dead entries, see above.)
            if constexpr (RANGED) p = (sv[nk][r] < -1e29f) ? 0.f : p;
            pw[(sb * 16 + (lane >> 4) * 4 + r) * VP + nk * 16 + (lane & 15)] =
                (__bf16)p;
          }
        }
      }
      // ---- O += P V (V^T B-frags loaded once per sub-block set) ----
      f32x4_t racc[NSB];
#pragma unroll
      for (int sb = 0; sb < NSB; ++sb) racc[sb] = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int nj = 0; nj < DN; ++nj) {
#pragma unroll
        for (int kk = 0; kk < BN / 32; ++kk) {
          bf16x8_t vb =
              load_frag_b_trT_swz(vt_lds[cur], VP, nj * 16, kk * 32, lane);
#pragma unroll
          for (int sb = 0; sb < NSB; ++sb) {
            bf16x8_t pa = load_frag_a(pw + sb * 16 * VP, VP, kk * 32, lane);
            oacc[sb][nj] = MFMA_16x16x32(pa, vb, oacc[sb][nj]);
            if constexpr (!DROPOUT)
              if (nj == 0) racc[sb] = MFMA_16x16x32(pa, ones_frag, racc[sb]);
          }
        }
      }
      if constexpr (!DROPOUT) {
#pragma unroll
        for (int sb = 0; sb < NSB; ++sb)
#pragma unroll
          for (int r = 0; r < 4; ++r)
            l_i[sb][r] = l_i[sb][r] * alpha_s[sb][r] + racc[sb][r];
      }
    }
    // stage tile jb+1 into the OTHER buffer (its previous contents —
    // tile jb-1 — were last read before the barrier that ended jb-1, so
    // no wave can still be reading it); T14: the global loads issued at
    // the top of this iteration have been landing under the MFMAs
    if (jb + 1 < nkb) write_lds(cur ^ 1);
    __syncthreads();  // tile jb reads done AND tile jb+1 writes visible
  }

  // ---- epilogue: O /= l (strided [s,b,h,d] store) + LSE ----
  bf16* Op = O + ((long)b * HQ + hq) * D;  // O contiguous [s, b, hq, d]
  const long sOs = (long)Bb * HQ * D;
  float* Lp = LSE + ((long)b * HQ + hq) * SQ;
#pragma unroll
  for (int sb = 0; sb < NSB; ++sb) {
    float inv_l[4];
    if constexpr (DROPOUT) {  // lane partials -> row sums
#pragma unroll
      for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int off = 1; off < 16; off <<= 1)
          l_i[sb][r] += __shfl_xor(l_i[sb][r], off, 64);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r)
      inv_l[r] = (l_i[sb][r] > 0.f) ? 1.f / l_i[sb][r] : 0.f;
    if constexpr (DROPOUT) {  // keep_scale folds into the normalisation
#pragma unroll
      for (int r = 0; r < 4; ++r) inv_l[r] *= dropout_keep_scale(drop_t);
    }
#pragma unroll
    for (int nj = 0; nj < DN; ++nj) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int qrow = qrow_w + sb * 16 + (lane >> 4) * 4 + r;
        if (qrow < SQ)
          Op[(long)qrow * sOs + nj * 16 + (lane & 15)] =
              f2bf(oacc[sb][nj][r] * inv_l[r]);
      }
    }
    if ((lane & 15) == 0) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int qrow = qrow_w + sb * 16 + (lane >> 4) * 4 + r;
        if (qrow < SQ)
          Lp[qrow] = m_i[sb][r] + __logf(fmaxf(l_i[sb][r], 1e-30f));
      }
    }
  }
}

extern "C" void launch_flash_fwd_dbuf(const FlashArgs& a, hipStream_t stream) {
  const int bm = flash_block_rows(a.SQ, a.B * a.HQ);
  const dim3 grid((a.SQ + bm - 1) / bm, a.B * a.HQ), blk(512);
  dispatch_flash_drop(a, [&](auto d, auto c, auto r, auto s, auto p) {
    constexpr int D = decltype(d)::value;
    constexpr bool C = decltype(c)::value, R = decltype(r)::value,
                   S = decltype(s)::value, P = decltype(p)::value;
    auto kern = bm == 128 ? flash_fwd_dbuf_kernel<D, C, 1, R, S, P>
                          : flash_fwd_dbuf_kernel<D, C, 2, R, S, P>;
    kern<<<grid, blk, 0, stream>>>(
        (const bf16*)a.q, (const bf16*)a.k, (const bf16*)a.v, (bf16*)a.o,
        (float*)a.lse, a.SQ, a.SKV, a.B, a.HQ, a.HKV, a.scale, a.window,
        a.qs[0], a.qs[1], a.qs[2], a.ks[0], a.ks[1], a.ks[2], a.vs[0],
        a.vs[1], a.vs[2], a.bound_a, a.bound_b, a.drop_t, a.drop_seed,
        a.drop_offset);
  });
}
