// Split-KV flash-decode: attention of a few query rows (S_q = 1 decode step,
// or a short speculative / chunked step) over a long, preallocated KV cache.
// Forward only, bf16, head_dim 64 / 128, two kernels.
//
// The training forward gives a block a 128/256-row query tile and walks the
// keys serially; at decode one row of that tile is alive, the grid is B*HQ
// blocks and every query head of a GQA group streams the same K/V again.
// Here the work is cut the other way round:
//
//   grid = (key split, kv head, batch row), 128 threads = 2 waves.
//
// * One block serves ALL G = HQ/HKV query heads of its kv head: the G*S_q
//   query rows are stacked (row m = g*S_q + i) as the M rows of MT 16-row
//   mfma_f32_16x16x32_bf16 tiles (G*S_q <= 64, MT = 1, 2 or 4), loaded once
//   and held in registers. K/V bytes are read once per kv head.
// * The block walks its slice of the keys in 64-key tiles. All 128 threads
//   stage a tile with 16-byte global loads: K row-major, V transposed
//   (tr_swz image, as in the training forward). Tile t+1's loads are issued
//   before tile t's MFMAs and land in the other LDS buffer after them: one
//   barrier per tile.
// * Inside a tile the two waves do not share rows, they share KEYS: wave w
//   owns keys [32w, 32w+32) of every tile and runs a private online softmax
//   (m, l, O) over them for all M rows. S = Q K^T is 2 x D/32 MFMAs per
//   M-tile, P goes through a wave-private LDS patch to become the A operand
//   of O += P V (D/16 MFMAs per M-tile, full k = 32 contraction), the row
//   sums come from one ones-fragment MFMA. No cross-wave traffic in the loop.
// * After the loop wave 1 hands its state to wave 0 through LDS (the K
//   buffers are free by then), wave 0 merges the two by log-sum-exp and
//   stores the split's NORMALISED partial O (fp32) and partial LSE.
//
// The combine kernel merges the partials of a row by log-sum-exp with
// reductions of a fixed shape, so for a given num_splits the result is
// bit-reproducible.
//
// Key range and garbage: row b sees keys kv_lo[b] <= j < kv_hi[b] (device
// int32, clamped to [0, max_kv] here, so no value of theirs can move a load
// out of the cache buffers). Everything outside is torch.empty garbage and
// may be NaN / Inf: what a load of a dead key returns is replaced by zeros
// with a select before it is staged, and a dead score is replaced by -inf
// with a select before the exp, so garbage reaches neither S nor P V and
// nothing is ever multiplied by a zero probability to get rid of it. Tiles
// with no alive key for the block are skipped; a split with none stores
// O = 0 / LSE = -1e30.
//
// Mask: query i of row b sits at position p = kv_hi[b] - S_q + i and sees
// j <= p, and j > p - window with a sliding window.
#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>

#include "launch.h"

// Scalar fp32 VALU only in this file: the packed-fp32 forms are kept out of
// the new kernels (same effect as -target-feature -packed-fp32-ops, limited
// to this translation unit so the other kernels compile as before).
#pragma clang attribute push(__attribute__((target("no-packed-fp32-ops"))), \
                             apply_to = function)
#include "attn_common.h"

namespace {

typedef int i32x4_t __attribute__((ext_vector_type(4)));

constexpr float kEmptyLse = -1e30f;  // the project's "no alive key" sentinel

constexpr int DEC_BN = 64;        // keys per tile
constexpr int DEC_WN = 32;        // keys per wave per tile
constexpr int DEC_THREADS = 128;  // 2 waves
constexpr int DEC_PP = DEC_WN + 8;  // P patch row stride (elements)

template <int D, int MT>
__global__ __launch_bounds__(DEC_THREADS) void flash_decode_split_kernel(
    const bf16* __restrict__ Q, const bf16* __restrict__ K,
    const bf16* __restrict__ V,
    float* __restrict__ Opart,    // [NS, B, HQ, SQ, D] f32, normalised
    float* __restrict__ LSEpart,  // [NS, B, HQ, SQ] f32
    const int* __restrict__ kv_lo, const int* __restrict__ kv_hi, int max_kv,
    int keys_per_split, int Bb, int HQ, int HKV, int SQ, float scale,
    int window, long sQs, long sQb, long sQh, long sKs, long sKb, long sKh,
    long sVs, long sVb, long sVh) {
  constexpr int BN = DEC_BN, WN = DEC_WN, NT = DEC_THREADS, PP = DEC_PP;
  constexpr int KP = D + 8;   // K tile row stride
  constexpr int VP = BN + 8;  // V^T image row stride
  constexpr int DK = D / 32, DN = D / 16;
  __shared__ __attribute__((aligned(16))) __bf16 k_lds[2][BN * KP];
  __shared__ __attribute__((aligned(16))) __bf16 vt_lds[2][D * VP];
  __shared__ __attribute__((aligned(16))) __bf16 p_lds[2][MT * 16 * PP];
  // the hand-over of wave 1's state reuses the K and V^T buffers
  static_assert(sizeof(f32x4_t) * MT * DN * 64 <= sizeof(k_lds), "O hand-over");
  static_assert(sizeof(f32x4_t) * MT * 2 * 64 <= sizeof(vt_lds), "m/l hand-over");

  const int lane = threadIdx.x & 63;
  const int wid = threadIdx.x >> 6;
  const int split = blockIdx.x, hkv = blockIdx.y, b = blockIdx.z;
  const int G = HQ / HKV;
  const int M = G * SQ;  // stacked query rows, <= 16 * MT

  // block-uniform alive key range of this batch row, clamped so that no
  // device value can push a load outside [0, max_kv)
  const int hi = min(max(kv_hi[b], 0), max_kv);
  const int lo = min(max(kv_lo[b], 0), hi);
  // first key any query of the step can see (query 0 has the lowest window)
  int kmin = lo;
  if (window > 0) kmin = max(kmin, hi - SQ - window + 1);
  const int s0 = split * keys_per_split;
  const int s1 = min(s0 + keys_per_split, max_kv);
  const int a0 = max(s0, kmin), a1 = min(s1, hi);  // alive part of the slice
  // tiles are aligned to BN from key 0 (keys_per_split is a multiple of BN)
  const int t0 = a0 / BN;
  const int t1 = a0 < a1 ? (a1 + BN - 1) / BN : t0;  // empty: no tile

  const bf16* Kp = K + b * sKb + hkv * sKh;
  const bf16* Vp = V + b * sVb + hkv * sVh;

  // ---- Q: the group's stacked rows, once, into A fragments ----
  bf16x8_t qfrag[MT][DK];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) {
    int m = mt * 16 + (lane & 15);
    if (m >= M) m = 0;  // padding rows read row 0; they are never stored
    const int g = m / SQ, i = m - g * SQ;
    const bf16* qp = Q + b * sQb + (long)(hkv * G + g) * sQh + (long)i * sQs;
#pragma unroll
    for (int kk = 0; kk < DK; ++kk)
      *(i32x4_t*)&qfrag[mt][kk] =
          *(const i32x4_t*)(qp + kk * 32 + (lane >> 4) * 8);
  }

  // per C-layout row (mt, r): last and first visible key. Padding rows see
  // nothing (last = -1).
  int row_last[MT][4], row_first[MT][4];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int m = mt * 16 + (lane >> 4) * 4 + r;
      const int i = m % SQ;
      const int p = hi - SQ + i;
      row_last[mt][r] = (m < M) ? p : -1;
      row_first[mt][r] = (window > 0) ? max(lo, p - window + 1) : lo;
    }
  }

  float m_i[MT][4], l_i[MT][4];
  f32x4_t oacc[MT][DN];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      m_i[mt][r] = kEmptyLse;
      l_i[mt][r] = 0.f;
    }
#pragma unroll
    for (int nj = 0; nj < DN; ++nj) oacc[mt][nj] = f32x4_t{0.f, 0.f, 0.f, 0.f};
  }
  bf16x8_t ones_frag;
#pragma unroll
  for (int j = 0; j < 8; ++j) ones_frag[j] = (__bf16)1.0f;

  // ---- staging: BN x D of K and of V per tile, 16 B per load ----
  constexpr int K_PER_THR = BN * D / 8 / NT;   // int4 K vectors per thread
  constexpr int V_PER_THR = BN * D / 16 / NT;  // V row-pair slices per thread
  i32x4_t kreg[K_PER_THR], vreg0[V_PER_THR], vreg1[V_PER_THR];
  const i32x4_t zero4 = {0, 0, 0, 0};

  // One 16 B vector of cache row `gr`. The address is clamped into
  // [0, max_kv) so the load is always legal and needs no branch (a branch
  // per vector would put a wait between the loads); what a dead row
  // returned, garbage or not, is replaced by zeros with a select.
  auto load_row = [&](const bf16* base, long stride, int gr, int col8) {
    const int grc = min(max(gr, 0), max_kv - 1);
    const i32x4_t x = *(const i32x4_t*)(base + (long)grc * stride + col8);
    return (gr >= kmin && gr < hi) ? x : zero4;
  };

  auto issue_loads = [&](int kbase) {
#pragma unroll
    for (int u = 0; u < K_PER_THR; ++u) {
      const int t = threadIdx.x + u * NT;
      kreg[u] = load_row(Kp, sKs, kbase + t / (D / 8), (t % (D / 8)) * 8);
    }
#pragma unroll
    for (int u = 0; u < V_PER_THR; ++u) {
      const int t = threadIdx.x + u * NT;
      const int g0 = kbase + (t / (D / 8)) * 2;
      const int col8 = (t % (D / 8)) * 8;
      vreg0[u] = load_row(Vp, sVs, g0, col8);
      vreg1[u] = load_row(Vp, sVs, g0 + 1, col8);
    }
  };

  auto write_lds = [&](int buf) {
#pragma unroll
    for (int u = 0; u < K_PER_THR; ++u) {
      const int t = threadIdx.x + u * NT;
      *(i32x4_t*)&k_lds[buf][(t / (D / 8)) * KP + (t % (D / 8)) * 8] = kreg[u];
    }
#pragma unroll
    for (int u = 0; u < V_PER_THR; ++u) {
      const int t = threadIdx.x + u * NT;
      const int row = (t / (D / 8)) * 2;  // key pair inside the tile
      const int col8 = (t % (D / 8)) * 8;
      // word w of a row holds columns 2w (low half) and 2w + 1 (high half);
      // pure register arithmetic, so the staging arrays stay in VGPRs
      const uint w0[4] = {(uint)vreg0[u].x, (uint)vreg0[u].y,
                          (uint)vreg0[u].z, (uint)vreg0[u].w};
      const uint w1[4] = {(uint)vreg1[u].x, (uint)vreg1[u].y,
                          (uint)vreg1[u].z, (uint)vreg1[u].w};
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const uint pair = (j & 1)
                              ? (w0[j >> 1] >> 16) | (w1[j >> 1] & 0xffff0000u)
                              : (w0[j >> 1] & 0xffffu) | (w1[j >> 1] << 16);
        const int r = col8 + j;  // image row = head-dim column
        *(uint*)((char*)vt_lds[buf] + tr_swz((uint)(r * VP + row) * 2, r)) =
            pair;
      }
    }
  };

  if (t0 < t1) {
    issue_loads(t0 * BN);
    write_lds(t0 & 1);
  }
  __syncthreads();

  __bf16* pw = p_lds[wid];
  for (int t = t0; t < t1; ++t) {
    const int cur = t & 1;
    const int kbase_w = t * BN + wid * WN;  // first key of this wave
    if (t + 1 < t1) issue_loads((t + 1) * BN);

    // ---- S = Q K^T over the wave's 32 keys (K fragments loaded once) ----
    f32x4_t sacc[MT][2];
#pragma unroll
    for (int nk = 0; nk < 2; ++nk) {
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) sacc[mt][nk] = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int kk = 0; kk < DK; ++kk) {
        const bf16x8_t kb = load_frag_b_rowmajorT(
            &k_lds[cur][(wid * WN + nk * 16) * KP], KP, kk * 32, lane);
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
          sacc[mt][nk] = MFMA_16x16x32(qfrag[mt][kk], kb, sacc[mt][nk]);
      }
    }

    // ---- mask (select), online softmax, P -> wave-private LDS patch ----
    float alpha[MT][4];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
      float sv[2][4];
      float tile_max[4] = {kEmptyLse, kEmptyLse, kEmptyLse, kEmptyLse};
#pragma unroll
      for (int nk = 0; nk < 2; ++nk) {
        const int kcol = kbase_w + nk * 16 + (lane & 15);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const bool dead =
              kcol > row_last[mt][r] || kcol < row_first[mt][r];
          // -inf, not -1e30: with m_i finite (>= -1e30) exp gives exactly 0
          // even for a row that has met no alive key yet
          const float s =
              dead ? -__builtin_inff() : sacc[mt][nk][r] * scale;
          sv[nk][r] = s;
          tile_max[r] = fmaxf(tile_max[r], s);
        }
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) {
#pragma unroll
        for (int off = 1; off < 16; off <<= 1)
          tile_max[r] = fmaxf(tile_max[r], __shfl_xor(tile_max[r], off, 64));
        const float mn = fmaxf(m_i[mt][r], tile_max[r]);
        alpha[mt][r] = __expf(m_i[mt][r] - mn);
        m_i[mt][r] = mn;
      }
#pragma unroll
      for (int nk = 0; nk < 2; ++nk) {
#pragma unroll
        for (int r = 0; r < 4; ++r)
          pw[(mt * 16 + (lane >> 4) * 4 + r) * PP + nk * 16 + (lane & 15)] =
              (__bf16)__expf(sv[nk][r] - m_i[mt][r]);
      }
#pragma unroll
      for (int nj = 0; nj < DN; ++nj) {
#pragma unroll
        for (int r = 0; r < 4; ++r) oacc[mt][nj][r] *= alpha[mt][r];
      }
    }

    // ---- O += P V, l += rowsum(P) (V^T fragments loaded once) ----
    bf16x8_t pa[MT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
      pa[mt] = load_frag_a(pw + mt * 16 * PP, PP, 0, lane);
      const f32x4_t rs =
          MFMA_16x16x32(pa[mt], ones_frag, (f32x4_t{0.f, 0.f, 0.f, 0.f}));
#pragma unroll
      for (int r = 0; r < 4; ++r)
        l_i[mt][r] = l_i[mt][r] * alpha[mt][r] + rs[r];
    }
#pragma unroll
    for (int nj = 0; nj < DN; ++nj) {
      const bf16x8_t vb =
          load_frag_b_trT_swz(vt_lds[cur], VP, nj * 16, wid * WN, lane);
#pragma unroll
      for (int mt = 0; mt < MT; ++mt)
        oacc[mt][nj] = MFMA_16x16x32(pa[mt], vb, oacc[mt][nj]);
    }

    // tile t+1 goes to the other buffer: tile t-1, its previous content,
    // was last read before the barrier that ended iteration t-1
    if (t + 1 < t1) write_lds(cur ^ 1);
    __syncthreads();  // tile t reads done, tile t+1 visible
  }

  // ---- merge the two waves' (m, l, O) by log-sum-exp in wave 0 ----
  f32x4_t* o_x = (f32x4_t*)&k_lds[0][0];    // [MT * DN][64]
  f32x4_t* ml_x = (f32x4_t*)&vt_lds[0][0];  // [MT * 2][64]
  if (wid == 1) {
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
      ml_x[(mt * 2 + 0) * 64 + lane] =
          f32x4_t{m_i[mt][0], m_i[mt][1], m_i[mt][2], m_i[mt][3]};
      ml_x[(mt * 2 + 1) * 64 + lane] =
          f32x4_t{l_i[mt][0], l_i[mt][1], l_i[mt][2], l_i[mt][3]};
#pragma unroll
      for (int nj = 0; nj < DN; ++nj)
        o_x[(mt * DN + nj) * 64 + lane] = oacc[mt][nj];
    }
  }
  __syncthreads();
  if (wid != 0) return;

  const long row_stride = (long)SQ * D;  // partials: [NS, B, HQ, SQ, D]
  float* Op = Opart + (((long)split * Bb + b) * HQ + (long)hkv * G) * row_stride;
  float* Lp = LSEpart + (((long)split * Bb + b) * HQ + (long)hkv * G) * SQ;
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) {
    const f32x4_t m1 = ml_x[(mt * 2 + 0) * 64 + lane];
    const f32x4_t l1 = ml_x[(mt * 2 + 1) * 64 + lane];
    float w0[4], w1[4], lse[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float mn = fmaxf(m_i[mt][r], m1[r]);
      const float c0 = __expf(m_i[mt][r] - mn), c1 = __expf(m1[r] - mn);
      const float l = l_i[mt][r] * c0 + l1[r] * c1;
      // no alive key in the slice: l == 0 -> O = 0, sentinel LSE
      const float inv = l > 0.f ? 1.f / l : 0.f;
      w0[r] = c0 * inv;
      w1[r] = c1 * inv;
      lse[r] = l > 0.f ? mn + __logf(l) : kEmptyLse;
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      // stacked row m = g * SQ + i is row (hkv * G + g, i) of [HQ, SQ]: the
      // group's rows are contiguous, so m indexes them directly
      const int m = mt * 16 + (lane >> 4) * 4 + r;
      if (m < M) {
#pragma unroll
        for (int nj = 0; nj < DN; ++nj) {
          const f32x4_t o1 = o_x[(mt * DN + nj) * 64 + lane];
          Op[(long)m * D + nj * 16 + (lane & 15)] =
              oacc[mt][nj][r] * w0[r] + o1[r] * w1[r];
        }
        if ((lane & 15) == 0) Lp[m] = lse[r];
      }
    }
  }
}

// One 256-thread block per output row (b, hq, i). The row's NS partials are
// independent loads: a serial walk over them would pay one memory latency
// per split (64 splits at batch 1), so the block spreads them out.
//   1. thread t reads the LSEs of splits t, t + 256, ..; block max; the
//      weights w_s = exp(LSE_s - max) go to LDS, their sum is reduced;
//   2. D / 4 threads cover a row as float4s, so 256 / (D / 4) groups walk
//      the splits side by side (group g takes s = g, g + NG, ..) into
//      partial sums, which the first D / 4 threads add in group order.
// Every reduction has a fixed shape, so a given num_splits is
// bit-reproducible. An empty split (sentinel LSE) gets weight 0 by select.
constexpr int CMB_THREADS = 256;
constexpr int CMB_MAX_SPLITS = 1024;

DEVINL float block_all_reduce(float x, bool is_max, float* red) {
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const float y = __shfl_xor(x, off, 64);
    x = is_max ? fmaxf(x, y) : x + y;
  }
  __syncthreads();  // red may still be read from the previous call
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = x;
  __syncthreads();
  x = red[0];
#pragma unroll
  for (int w = 1; w < CMB_THREADS / 64; ++w)
    x = is_max ? fmaxf(x, red[w]) : x + red[w];
  return x;
}

template <int D>
__global__ __launch_bounds__(CMB_THREADS) void flash_decode_combine_kernel(
    const float* __restrict__ Opart, const float* __restrict__ LSEpart,
    bf16* __restrict__ O, float* __restrict__ LSE, int num_splits,
    long rows) {
  constexpr int L = D / 4;             // threads per row
  constexpr int NG = CMB_THREADS / L;  // split groups
  __shared__ float w_lds[CMB_MAX_SPLITS];
  __shared__ f32x4_t acc_lds[NG * L];
  __shared__ float red[CMB_THREADS / 64];
  const long row = blockIdx.x;
  const int t = threadIdx.x;

  float mx = kEmptyLse;
  for (int s = t; s < num_splits; s += CMB_THREADS) {
    const float lse = LSEpart[s * rows + row];
    w_lds[s] = lse;
    mx = fmaxf(mx, lse);
  }
  mx = block_all_reduce(mx, true, red);
  float wsum = 0.f;
  for (int s = t; s < num_splits; s += CMB_THREADS) {
    const float lse = w_lds[s];  // written by this thread
    const float w = lse > kEmptyLse ? __expf(lse - mx) : 0.f;
    w_lds[s] = w;
    wsum += w;
  }
  wsum = block_all_reduce(wsum, false, red);  // its barriers publish w_lds

  const int g = t / L, c = t % L;
  f32x4_t acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
  for (int s = g; s < num_splits; s += NG) {
    const f32x4_t o =
        *(const f32x4_t*)(Opart + (s * rows + row) * D + c * 4);
    const float w = w_lds[s];
#pragma unroll
    for (int e = 0; e < 4; ++e) acc[e] += w * o[e];
  }
  acc_lds[g * L + c] = acc;
  __syncthreads();
  if (t >= L) return;
  acc = acc_lds[t];
#pragma unroll
  for (int gg = 1; gg < NG; ++gg) {
    const f32x4_t x = acc_lds[gg * L + t];
#pragma unroll
    for (int e = 0; e < 4; ++e) acc[e] += x[e];
  }
  // no alive key in any split: wsum == 0 -> O = 0, sentinel LSE
  const float inv = wsum > 0.f ? 1.f / wsum : 0.f;
  __attribute__((aligned(8))) bf16 out[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) out[e] = f2bf(acc[e] * inv);
  *(uint2*)(O + row * D + t * 4) = *(const uint2*)out;
  if (t == 0) LSE[row] = wsum > 0.f ? mx + __logf(wsum) : kEmptyLse;
}

}  // namespace
#pragma clang attribute pop

template <int D, int MT>
static void launch_split(const FlashDecodeArgs& a, int keys_per_split,
                         hipStream_t stream) {
  const dim3 grid(a.num_splits, a.HKV, a.B), blk(DEC_THREADS);
  flash_decode_split_kernel<D, MT><<<grid, blk, 0, stream>>>(
      (const bf16*)a.q, (const bf16*)a.k, (const bf16*)a.v, (float*)a.o_part,
      (float*)a.lse_part, a.kv_lo, a.kv_hi, a.max_kv, keys_per_split, a.B,
      a.HQ, a.HKV, a.SQ, a.scale, a.window, a.qs[0], a.qs[1], a.qs[2],
      a.ks[0], a.ks[1], a.ks[2], a.vs[0], a.vs[1], a.vs[2]);
  HIP_CHECK_LAST();
}

template <int D>
static void launch_decode_d(const FlashDecodeArgs& a, hipStream_t stream) {
  const int tiles = (a.max_kv + DEC_BN - 1) / DEC_BN;
  const int keys_per_split =
      (tiles + a.num_splits - 1) / a.num_splits * DEC_BN;
  const int m_tiles = (a.HQ / a.HKV * a.SQ + 15) / 16;  // 1..4
  if (m_tiles == 1)
    launch_split<D, 1>(a, keys_per_split, stream);
  else if (m_tiles == 2)
    launch_split<D, 2>(a, keys_per_split, stream);
  else
    launch_split<D, 4>(a, keys_per_split, stream);
  const long rows = (long)a.B * a.HQ * a.SQ;
  flash_decode_combine_kernel<D>
      <<<dim3((unsigned)rows), dim3(CMB_THREADS), 0, stream>>>(
      (const float*)a.o_part, (const float*)a.lse_part, (bf16*)a.o,
      (float*)a.lse, a.num_splits, rows);
  HIP_CHECK_LAST();
}

// The binding has checked: D in {64, 128}, HQ % HKV == 0, G * SQ <= 64,
// 1 <= max_kv <= CAP, 1 <= num_splits <= 1024, B, HKV, SQ >= 1.
extern "C" void launch_flash_decode(const FlashDecodeArgs& a,
                                    hipStream_t stream) {
  if (a.num_splits < 1 || a.num_splits > CMB_MAX_SPLITS)  // w_lds
    throw std::runtime_error("flash decode: num_splits out of [1, 1024]");
  if (a.D == 128)
    launch_decode_d<128>(a, stream);
  else
    launch_decode_d<64>(a, stream);
}
