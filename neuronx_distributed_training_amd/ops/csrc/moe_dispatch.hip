// Token path of the dropless / capacity MoE layer around the grouped GEMMs
// (moe_gemm.hip): from the router's topi [T, k] to the 256-row-aligned padded
// layout and back, with no sort, no index op and no token-sorted intermediate.
//
// Plan: a deterministic counting sort of the P = T * k (token, choice) pairs
// by expert, in three launches.
//   hist   one block per chunk of MOE_PLAN_CHUNK consecutive pairs counts the
//          chunk's pairs per expert in LDS (integer adds: order-free) and
//          writes row `chunk` of a [chunks, E] table;
//   scan   one block: lane e of wave 0 walks column e of the table, leaving
//          each chunk's exclusive base, clamps the total to the capacity,
//          rounds it up to 256 and prefix-sums the E padded sizes across the
//          wave (pad_off, total); all 256 threads then fill tile_expert;
//   place  one block per chunk re-reads it 256 pairs at a time, thread order =
//          pair order. A lane finds the lanes of its wave that hold the same
//          expert from six ballots (one per bit of the id); the popcount of
//          the lower ones is its rank in the wave, a [4][64] LDS table of
//          per-wave counts gives the waves before it, a running LDS base the
//          rounds and chunks before that. rank < cap keeps the pair:
//          slot[p] = pad_off[e] + rank, row_src[slot] = p; else slot[p] = -1.
// No global atomic decides a position, so the plan is a pure function of topi:
// inside an expert pairs stay in ascending pair order, the order of a stable
// argsort. An id outside [0, E) is treated as a dropped pair.
//
// Row kernels (permute, combine, combine backward): a row of H bf16 is held
// by a group of G = moe_row_lanes(H) adjacent lanes, 256 / G rows per block;
// lane `sub` of the group moves the 16-byte vectors sub, sub + G, ... so a
// group's accesses are contiguous. A padded row r is past the end
// (r >= total: never touched), padding (r - pad_off[e] >= counts[e] with e =
// tile_expert[r / 256]: zero-filled) or valid (holds pair row_src[r]).
//   permute       x_pad[r] = x[row_src[r] / k]
//   combine       y[t] = bf16(sum_j w[t, j] * y_pad[slot[t, j]]), fp32 in
//                 registers, j ascending, dropped pairs skipped, every token
//                 row written; w == null: unit weights (permute's backward)
//   combine bwd   dy_pad[r] = bf16(w[pair] * dy[tok]) and dw[pair] =
//                 dot(dy[tok], y_pad[r]) from one read of both rows; the dot is
//                 reduced over the group in a fixed order. Extra blocks behind
//                 the row blocks sweep `slot` and write dw = 0 for dropped
//                 pairs, so no fill launch is needed.
// Every index read from a plan tensor is range-checked before it addresses
// memory: a plan that does not belong to the other arguments yields zeros.
#include "common.h"
#include "launch.h"

namespace {

constexpr int MAXE = MOE_PLAN_MAX_E;
static_assert(MAXE == 64, "one wave lane per expert, six id bits per ballot");
static_assert(MOE_PLAN_CHUNK % 256 == 0, "place walks a chunk 256 pairs a round");

// expert of pair p, -1 for a pair past the end or an id outside [0, E)
DEVINL int pair_expert(const long* __restrict__ topi, int p, int P, int E) {
  if (p >= P) return -1;
  const long v = topi[p];
  return (v >= 0 && v < E) ? (int)v : -1;
}

__global__ __launch_bounds__(256) void moe_plan_hist_kernel(
    const long* __restrict__ topi, int* __restrict__ table, int P, int E) {
  __shared__ int hist[MAXE];
  if (threadIdx.x < MAXE) hist[threadIdx.x] = 0;
  __syncthreads();
  const int base = blockIdx.x * MOE_PLAN_CHUNK;
  for (int i = threadIdx.x; i < MOE_PLAN_CHUNK; i += 256) {
    const int e = pair_expert(topi, base + i, P, E);
    if (e >= 0) atomicAdd(&hist[e], 1);
  }
  __syncthreads();
  if (threadIdx.x < E) table[(long)blockIdx.x * E + threadIdx.x] = hist[threadIdx.x];
}

__global__ __launch_bounds__(256) void moe_plan_scan_kernel(
    int* __restrict__ table, long* __restrict__ counts,
    int* __restrict__ pad_off, int* __restrict__ total,
    int* __restrict__ tile_expert, int chunks, int E, int cap, int n_tiles) {
  __shared__ int off[MAXE + 1];
  const int e = threadIdx.x;
  if (e < 64) {
    int run = 0;
    if (e < E) {
      for (int c = 0; c < chunks; ++c) {
        int* t = table + (long)c * E + e;
        const int v = *t;
        *t = run;
        run += v;
      }
    }
    const int cnt = (cap > 0 && run > cap) ? cap : run;
    int incl = e < E ? (cnt + 255) / 256 * 256 : 0;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const int up = __shfl_up(incl, d, 64);
      if (e >= d) incl += up;
    }
    if (e == 0) off[0] = pad_off[0] = 0;
    if (e < E) {
      counts[e] = cnt;
      off[e + 1] = pad_off[e + 1] = incl;
    }
    if (e == E - 1) total[0] = incl;
  }
  __syncthreads();
  // searchsorted(pad_off[1:], 256 * t, right = True), clamped to E - 1
  for (int t = threadIdx.x; t < n_tiles; t += 256) {
    const int row = t * 256;
    int n = 0;
    for (int j = 1; j <= E; ++j) n += off[j] <= row;
    tile_expert[t] = n < E - 1 ? n : E - 1;
  }
}

__global__ __launch_bounds__(256) void moe_plan_place_kernel(
    const long* __restrict__ topi, const int* __restrict__ table,
    const int* __restrict__ pad_off, int* __restrict__ slot,
    int* __restrict__ row_src, int P, int E, int cap, int Tp) {
  __shared__ int base[MAXE];      // pairs of expert e before this round
  __shared__ int wcnt[4][MAXE];   // this round's pairs of expert e per wave
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  if (tid < MAXE) base[tid] = tid < E ? table[(long)blockIdx.x * E + tid] : 0;
  wcnt[w][lane] = 0;
  __syncthreads();
  for (int r = 0; r < MOE_PLAN_CHUNK / 256; ++r) {
    const int p = blockIdx.x * MOE_PLAN_CHUNK + r * 256 + tid;
    const int e = pair_expert(topi, p, P, E);
    // lanes of this wave with the same expert
    unsigned long long peers = __ballot(e >= 0);
#pragma unroll
    for (int b = 0; b < 6; ++b) {
      const int bit = (e >> b) & 1;
      const unsigned long long set = __ballot(bit);
      peers &= bit ? set : ~set;
    }
    const unsigned long long lower = peers & ((1ull << lane) - 1ull);
    if (e >= 0 && lower == 0) wcnt[w][e] = __popcll(peers);
    __syncthreads();
    if (e >= 0) {
      int rank = base[e] + __popcll(lower);
      for (int w2 = 0; w2 < w; ++w2) rank += wcnt[w2][e];
      int s = (cap <= 0 || rank < cap) ? pad_off[e] + rank : -1;
      if (s >= Tp) s = -1;
      slot[p] = s;
      if (s >= 0) row_src[s] = p;
    } else if (p < P) {
      slot[p] = -1;
    }
    __syncthreads();
    if (tid < MAXE) {
      int add = 0;
#pragma unroll
      for (int w2 = 0; w2 < 4; ++w2) {
        add += wcnt[w2][tid];
        wcnt[w2][tid] = 0;
      }
      base[tid] += add;
    }
    __syncthreads();
  }
}

// ------------------------------------------------------------- row kernels

enum RowState { ROW_PAST_END, ROW_PADDING, ROW_VALID };
DEVINL RowState row_state(const MoePlan& pl, long r) {
  if (r >= *pl.total) return ROW_PAST_END;
  const int e = pl.tile_expert[r >> 8];
  return r - pl.pad_off[e] < pl.counts[e] ? ROW_VALID : ROW_PADDING;
}

struct F8 {
  float f[8];
};
DEVINL F8 load8(const bf16* p, int vec) {
  Pack16B q;
  q.i4 = ((const int4*)p)[vec];
  F8 r;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    bf16x2 h = (&q.h8.a)[j];
    r.f[2 * j] = bf2f(h.x);
    r.f[2 * j + 1] = bf2f(h.y);
  }
  return r;
}
DEVINL void store8(bf16* p, int vec, const F8& v) {
  Pack16B o;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    bf16x2 h;
    h.x = f2bf(v.f[2 * j]);
    h.y = f2bf(v.f[2 * j + 1]);
    (&o.h8.a)[j] = h;
  }
  ((int4*)p)[vec] = o.i4;
}

DEVINL float w2f(float v) { return v; }
DEVINL float w2f(bf16 v) { return bf2f(v); }
DEVINL void f2w(float* p, float v) { *p = v; }
DEVINL void f2w(bf16* p, float v) { *p = f2bf(v); }

// sum over the G lanes of a row group, in a fixed order; lane 0 of the group
// (every lane for G = 256) holds it
template <int G>
DEVINL float group_sum(float v, float* lds) {
  if constexpr (G == 256) {
    return block_reduce_sum<256>(v, lds);
  } else {
#pragma unroll
    for (int off = G / 2; off > 0; off >>= 1) v += __shfl_down(v, off, G);
    return v;
  }
}

template <int G>
__global__ __launch_bounds__(256) void moe_permute_kernel(
    const bf16* __restrict__ x, bf16* __restrict__ x_pad, MoePlan pl, int T,
    int topk, int H) {
  const long r = blockIdx.x * (long)(256 / G) + threadIdx.x / G;
  const int sub = threadIdx.x % G;
  const RowState st = row_state(pl, r);
  if (st == ROW_PAST_END) return;
  const int nvec = H >> 3;
  int4* dst = (int4*)(x_pad + r * H);
  const int tok = st == ROW_VALID ? pl.row_src[r] / topk : -1;
  if ((unsigned)tok < (unsigned)T) {
    const int4* src = (const int4*)(x + (long)tok * H);
#pragma unroll 4
    for (int v = sub; v < nvec; v += G) dst[v] = src[v];
  } else {
    for (int v = sub; v < nvec; v += G) dst[v] = make_int4(0, 0, 0, 0);
  }
}

template <int G, typename WT>
__global__ __launch_bounds__(256) void moe_combine_kernel(
    const bf16* __restrict__ y_pad, const int* __restrict__ slot,
    const WT* __restrict__ w, bf16* __restrict__ y, int T, int topk, int H,
    int Tp) {
  const long t = blockIdx.x * (long)(256 / G) + threadIdx.x / G;
  const int sub = threadIdx.x % G;
  if (t >= T) return;
  int s[MOE_MAX_TOPK];
  float wt[MOE_MAX_TOPK];
#pragma unroll
  for (int j = 0; j < MOE_MAX_TOPK; ++j) {
    s[j] = -1;
    wt[j] = 1.f;
    if (j < topk) {
      const int v = slot[t * topk + j];
      if ((unsigned)v < (unsigned)Tp) s[j] = v;
      if (w) wt[j] = w2f(w[t * topk + j]);
    }
  }
  const int nvec = H >> 3;
  for (int v = sub; v < nvec; v += G) {
    F8 acc;
#pragma unroll
    for (int i = 0; i < 8; ++i) acc.f[i] = 0.f;
#pragma unroll
    for (int j = 0; j < MOE_MAX_TOPK; ++j) {
      if (s[j] >= 0) {
        const F8 a = load8(y_pad + (long)s[j] * H, v);
#pragma unroll
        for (int i = 0; i < 8; ++i) acc.f[i] = fmaf(wt[j], a.f[i], acc.f[i]);
      }
    }
    store8(y + t * H, v, acc);
  }
}

template <int G, typename WT>
__global__ __launch_bounds__(256) void moe_combine_bwd_kernel(
    const bf16* __restrict__ dy, const bf16* __restrict__ y_pad,
    const WT* __restrict__ w, const int* __restrict__ slot,
    bf16* __restrict__ dy_pad, WT* __restrict__ dw, MoePlan pl, int T,
    int topk, int H, int row_blocks) {
  __shared__ float red[4];
  const int P = T * topk;
  if ((int)blockIdx.x >= row_blocks) {   // pair side: dw of the dropped pairs
    const long p = (blockIdx.x - row_blocks) * 256L + threadIdx.x;
    if (p < P && slot[p] < 0) f2w(dw + p, 0.f);
    return;
  }
  const long r = blockIdx.x * (long)(256 / G) + threadIdx.x / G;
  const int sub = threadIdx.x % G;
  const RowState st = row_state(pl, r);
  int pair = st == ROW_VALID ? pl.row_src[r] : -1;
  if ((unsigned)pair >= (unsigned)P) pair = -1;
  const int nvec = H >> 3;
  float dot = 0.f;
  if (pair >= 0) {
    const float wt = w2f(w[pair]);
    const bf16* drow = dy + (long)(pair / topk) * H;
    for (int v = sub; v < nvec; v += G) {
      const F8 d = load8(drow, v);
      const F8 yv = load8(y_pad + r * H, v);
      F8 o;
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        o.f[i] = wt * d.f[i];
        dot = fmaf(d.f[i], yv.f[i], dot);
      }
      store8(dy_pad + r * H, v, o);
    }
  } else if (st != ROW_PAST_END) {
    int4* dst = (int4*)(dy_pad + r * H);
    for (int v = sub; v < nvec; v += G) dst[v] = make_int4(0, 0, 0, 0);
  }
  dot = group_sum<G>(dot, red);
  if (pair >= 0 && sub == 0) f2w(dw + pair, dot);
}

template <int G>
void permute_g(const void* x, void* x_pad, const MoePlan& plan, int T, int topk,
               int H, long Tp, hipStream_t stream) {
  moe_permute_kernel<G>
      <<<dim3((unsigned)(Tp / (256 / G))), dim3(256), 0, stream>>>(
          (const bf16*)x, (bf16*)x_pad, plan, T, topk, H);
}

template <int G, typename WT>
void combine_g(const void* y_pad, const void* slot, const void* w, void* y,
               int T, int topk, int H, long Tp, hipStream_t stream) {
  const unsigned blocks = (unsigned)((T + 256 / G - 1) / (256 / G));
  moe_combine_kernel<G, WT><<<dim3(blocks), dim3(256), 0, stream>>>(
      (const bf16*)y_pad, (const int*)slot, (const WT*)w, (bf16*)y, T, topk, H,
      (int)Tp);
}

template <int G, typename WT>
void combine_bwd_g(const void* dy, const void* y_pad, const void* w,
                   const void* slot, void* dy_pad, void* dw,
                   const MoePlan& plan, int T, int topk, int H, long Tp,
                   hipStream_t stream) {
  const int row_blocks = (int)(Tp / (256 / G));
  const int pair_blocks = (int)(((long)T * topk + 255) / 256);
  if (row_blocks + pair_blocks == 0) return;
  moe_combine_bwd_kernel<G, WT>
      <<<dim3((unsigned)(row_blocks + pair_blocks)), dim3(256), 0, stream>>>(
          (const bf16*)dy, (const bf16*)y_pad, (const WT*)w, (const int*)slot,
          (bf16*)dy_pad, (WT*)dw, plan, T, topk, H, row_blocks);
}

}  // namespace

// CALL with G = moe_row_lanes(H): one instantiation per row-group width
#define MOE_ROW_SWITCH(H, ...)                                   \
  switch (moe_row_lanes(H)) {                                    \
    case 16: { constexpr int G = 16; __VA_ARGS__; } break;       \
    case 64: { constexpr int G = 64; __VA_ARGS__; } break;       \
    default: { constexpr int G = 256; __VA_ARGS__; } break;      \
  }

extern "C" {
void launch_moe_plan(const void* topi, void* table, void* counts, void* pad_off,
                     void* total, void* tile_expert, void* slot, void* row_src,
                     int P, int E, int cap, long Tp, hipStream_t stream) {
  const int chunks = moe_plan_chunks(P);
  if (chunks > 0) {
    moe_plan_hist_kernel<<<dim3(chunks), dim3(256), 0, stream>>>(
        (const long*)topi, (int*)table, P, E);
    HIP_CHECK_LAST();
  }
  // with no pair at all it still writes zero counts, offsets and total
  moe_plan_scan_kernel<<<dim3(1), dim3(256), 0, stream>>>(
      (int*)table, (long*)counts, (int*)pad_off, (int*)total,
      (int*)tile_expert, chunks, E, cap, (int)(Tp / 256));
  HIP_CHECK_LAST();
  if (chunks > 0) {
    moe_plan_place_kernel<<<dim3(chunks), dim3(256), 0, stream>>>(
        (const long*)topi, (const int*)table, (const int*)pad_off, (int*)slot,
        (int*)row_src, P, E, cap, (int)Tp);
    HIP_CHECK_LAST();
  }
}

void launch_moe_permute(const void* x, void* x_pad, const MoePlan& plan, int T,
                        int topk, int H, long Tp, hipStream_t stream) {
  if (Tp <= 0) return;  // a grid of zero blocks is an invalid launch
  MOE_ROW_SWITCH(H, permute_g<G>(x, x_pad, plan, T, topk, H, Tp, stream));
  HIP_CHECK_LAST();
}

void launch_moe_combine(const void* y_pad, const void* slot, const void* w,
                        bool w_f32, void* y, int T, int topk, int H, long Tp,
                        hipStream_t stream) {
  if (T <= 0) return;
  if (w_f32) {
    MOE_ROW_SWITCH(H, combine_g<G, float>(y_pad, slot, w, y, T, topk, H, Tp,
                                          stream));
  } else {
    MOE_ROW_SWITCH(H, combine_g<G, bf16>(y_pad, slot, w, y, T, topk, H, Tp,
                                         stream));
  }
  HIP_CHECK_LAST();
}

void launch_moe_combine_bwd(const void* dy, const void* y_pad, const void* w,
                            bool w_f32, const void* slot, void* dy_pad,
                            void* dw, const MoePlan& plan, int T, int topk,
                            int H, long Tp, hipStream_t stream) {
  if (w_f32) {
    MOE_ROW_SWITCH(H, combine_bwd_g<G, float>(dy, y_pad, w, slot, dy_pad, dw,
                                              plan, T, topk, H, Tp, stream));
  } else {
    MOE_ROW_SWITCH(H, combine_bwd_g<G, bf16>(dy, y_pad, w, slot, dy_pad, dw,
                                             plan, T, topk, H, Tp, stream));
  }
  HIP_CHECK_LAST();
}
}

