// Fused LM-head + cross-entropy for MI355X (gfx950): the loss and its logit
// gradient straight from hidden[N, H] and weight[V, H] (the lm_head layout, V
// = local vocab shard), without the [N, V] logits tensor. bf16 in, fp32
// accumulation.
//
//   lmhead_ce_fwd     : per (token tile x vocab tile) block, the logits tile
//                       in fp32 accumulators -> one (max, sum-exp at that max)
//                       pair per (row, vocab tile) and the target logit
//   lmhead_ce_merge   : per row, the pairs combined in tile order into
//                       row_max / row_sumexp (the outputs of ce_fwd)
//   lmhead_ce_dlogits : the same main loop over a chunk of rows, epilogue
//                       dS = (exp(s - gmax) / gsum - onehot) * gout as bf16
//
// The product is "NT": both operands are contiguous along the contraction H,
// so both tiles are staged with 16-byte loads along H and both MFMA
// fragments are 16-byte LDS reads, with no transposed image.
//
// Block = 128 tokens x 128 vocab columns, 4 waves as 2 x 2, each 64 x 64 =
// 4 x 4 MFMA tiles (64 accumulator VGPRs). K loop in steps of 64 through two
// LDS buffers: the next step's global loads are issued into registers before
// this step's MFMAs and stored to the other buffer after them, one barrier
// per step. LDS rows are 64 + 8 elements (144 bytes): sixteen rows start at
// sixteen different 16-byte slots of the 256-byte bank span, so a fragment
// read (16 rows x 16 bytes per k group) is conflict-free.
//
// Swapped operands: MFMA(A = weight rows, B = hidden rows) gives C[vocab,
// token], so a lane holds ONE token (lane & 15) and four consecutive vocab
// columns per MFMA. The weight tile is stored to LDS with its rows permuted
// inside each 64-column block (wperm) such that MFMA j's row m stands for
// column (m >> 2) * 16 + j * 4 + (m & 3): the sixteen values of a lane over
// j = 0..3 are then the consecutive columns g * 16 .. g * 16 + 15 (g = lane >>
// 4). The row statistics need only two shuffles (the four g lanes of a token),
// and dS leaves as two 16-byte stores per lane and token.
//
// Rows past N and columns past V are never loaded (zeros go to LDS), masked
// out of the statistics and never stored. No atomics: every sum has one fixed
// order, so two runs are bit-equal, and the forward and the dlogits kernel
// run the same main loop and see bit-identical logits.
#include "attn_common.h"
#include "launch.h"

namespace {

constexpr int BM = LMHEAD_BM, BN = LMHEAD_BN, BK = LMHEAD_BK;
constexpr int LP = BK + 8;       // LDS row pitch in elements
constexpr int NT = 256;          // 4 waves
constexpr int VPT = BM * BK / 8 / NT;  // 16-byte vectors per thread and tile
constexpr int GROUP_M = 8;       // token tiles per grid group
static_assert(BM == 128 && BN == 128 && BK % 32 == 0, "2 x 2 waves of 64 x 64");

constexpr float NEG = -1e30f;  // max of an empty set; its sum-exp is 0

// (m, s) <- the pair of the union of two column sets
DEVINL void combine(float& m, float& s, float mo, float so) {
  const float mn = fmaxf(m, mo);
  s = s * __expf(m - mn) + so * __expf(mo - mn);
  m = mn;
}

// LDS row of weight-tile row r: inside each 64-row block, column
// c = q * 16 + j * 4 + lo goes to row j * 16 + q * 4 + lo.
DEVINL int wperm(int r) {
  return (r & 64) | (((r >> 2) & 3) << 4) | (((r >> 4) & 3) << 2) | (r & 3);
}

// Block -> (token tile, vocab tile). Workgroups are dealt round-robin to the 8
// XCDs, each with its own L2. XCD x takes the x-th eighth of the tile list (as
// xcd_remap does for attention heads), and the list runs over groups of
// GROUP_M token tiles, token tile fastest: the blocks resident on one XCD at
// the same time (about 64) form an 8 x 8 patch that shares 8 hidden and 8
// weight tiles while it walks H in step.
DEVINL void tile_of_block(int n_mt, int n_vt, int& mt, int& vt) {
  const long total = (long)n_mt * n_vt;
  long id = blockIdx.x;
  if ((total & 7) == 0) id = (id & 7) * (total >> 3) + (id >> 3);
  const long per_group = (long)GROUP_M * n_vt;
  const int first = (int)(id / per_group) * GROUP_M;
  const int gsz = n_mt - first < GROUP_M ? n_mt - first : GROUP_M;
  const long rem = id % per_group;
  mt = first + (int)(rem % gsz);
  vt = (int)(rem / gsz);
}

struct Stage {
  int4 h[VPT], w[VPT];
};

// One K step of both tiles into registers: thread t takes vectors t, t + 256,
// ... of the [128 rows x 8 vectors] tile, so 8 consecutive threads read 128
// contiguous bytes of one row.
DEVINL void load_stage(Stage& st, const bf16* __restrict__ hid,
                       const bf16* __restrict__ wt, long row0, long n_rows,
                       int col0, int V, int H, int k0) {
#pragma unroll
  for (int q = 0; q < VPT; ++q) {
    const int v = threadIdx.x + q * NT;
    const int r = v >> 3, c8 = (v & 7) * 8;
    st.h[q] = int4{0, 0, 0, 0};
    st.w[q] = int4{0, 0, 0, 0};
    if (row0 + r < n_rows)
      st.h[q] = *(const int4*)(hid + (row0 + r) * H + k0 + c8);
    if (col0 + r < V)
      st.w[q] = *(const int4*)(wt + (long)(col0 + r) * H + k0 + c8);
  }
}

DEVINL void store_stage(const Stage& st, __bf16* h_lds, __bf16* w_lds) {
#pragma unroll
  for (int q = 0; q < VPT; ++q) {
    const int v = threadIdx.x + q * NT;
    const int r = v >> 3, c8 = (v & 7) * 8;
    *(int4*)&h_lds[r * LP + c8] = st.h[q];
    *(int4*)&w_lds[wperm(r) * LP + c8] = st.w[q];
  }
}

enum Epilogue { STATS, DLOGITS };

// n_rows rows of hid / targets / gmax / gsum / gout / ds (the caller offsets
// them to its row chunk). STATS writes part and tgt, DLOGITS writes ds.
template <Epilogue EPI>
__global__ __launch_bounds__(NT) void lmhead_ce_kernel(
    const bf16* __restrict__ hid,      // [n_rows, H]
    const bf16* __restrict__ wt,       // [V, H]
    const long* __restrict__ targets,  // [n_rows] global ids
    float2* __restrict__ part,         // [n_rows, n_vt] (max, sum-exp)
    float* __restrict__ tgt,           // [n_rows], zero on entry
    const float* __restrict__ gmax, const float* __restrict__ gsum,
    const float* __restrict__ gout,    // [n_rows] each
    bf16* __restrict__ ds,             // [n_rows, V]
    long n_rows, int H, int V, long vocab_start, int n_mt, int n_vt) {
  __shared__ __bf16 h_lds[2][BM * LP];
  __shared__ __bf16 w_lds[2][BN * LP];
  __shared__ float red_m[BM], red_s[BM];

  const int lane = threadIdx.x & 63;
  const int wid = threadIdx.x >> 6;
  const int wm = wid >> 1, wn = wid & 1;
  const int g = lane >> 4;
  int mt, vt;
  tile_of_block(n_mt, n_vt, mt, vt);
  const long row0 = (long)mt * BM;
  const int col0 = vt * BN;

  f32x4_t acc[4][4];  // [token sub-block i][MFMA j]
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4_t{0.f, 0.f, 0.f, 0.f};

  Stage st;
  load_stage(st, hid, wt, row0, n_rows, col0, V, H, 0);
  store_stage(st, h_lds[0], w_lds[0]);
  __syncthreads();
  const int nkb = H / BK;
  for (int kb = 0; kb < nkb; ++kb) {
    const int cur = kb & 1;
    const bool more = kb + 1 < nkb;
    if (more) load_stage(st, hid, wt, row0, n_rows, col0, V, H, (kb + 1) * BK);
#pragma unroll
    for (int kk = 0; kk < BK / 32; ++kk) {
      bf16x8_t wf[4], hf[4];
#pragma unroll
      for (int j = 0; j < 4; ++j)
        wf[j] = load_frag_a(&w_lds[cur][(wn * 64 + j * 16) * LP], LP, kk * 32,
                            lane);
#pragma unroll
      for (int i = 0; i < 4; ++i)
        hf[i] = load_frag_b_rowmajorT(&h_lds[cur][(wm * 64 + i * 16) * LP], LP,
                                      kk * 32, lane);
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
          acc[i][j] = MFMA_16x16x32(wf[j], hf[i], acc[i][j]);
    }
    // the other buffer was last read in step kb - 1, before its barrier
    if (more) store_stage(st, h_lds[cur ^ 1], w_lds[cur ^ 1]);
    __syncthreads();
  }

  // acc[i][j][r] = logit of token row0 + wm * 64 + i * 16 + (lane & 15) and
  // column cbase + j * 4 + r
  const int cbase = col0 + wn * 64 + g * 16;
  if constexpr (EPI == STATS) {
    float m[4], s[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int lrow = wm * 64 + i * 16 + (lane & 15);
      const long row = row0 + lrow;
      const long t = row < n_rows ? targets[row] - vocab_start : -1;
      m[i] = NEG;
      s[i] = 0.f;
#pragma unroll
      for (int e = 0; e < 16; ++e)
        if (cbase + e < V) m[i] = fmaxf(m[i], acc[i][e >> 2][e & 3]);
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const float v = acc[i][e >> 2][e & 3];
        if (cbase + e < V) s[i] += __expf(v - m[i]);
        // t < V: a column past V is never a target, whatever the id
        if (t >= 0 && t < V && cbase + e == t) tgt[row] = v;
      }
      // the four lanes of a token; the two waves of its row meet in LDS
      combine(m[i], s[i], __shfl_xor(m[i], 16, 64), __shfl_xor(s[i], 16, 64));
      combine(m[i], s[i], __shfl_xor(m[i], 32, 64), __shfl_xor(s[i], 32, 64));
      if (wn == 1 && g == 0) {
        red_m[lrow] = m[i];
        red_s[lrow] = s[i];
      }
    }
    __syncthreads();
    if (wn == 0 && g == 0) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int lrow = wm * 64 + i * 16 + (lane & 15);
        if (row0 + lrow >= n_rows) continue;
        combine(m[i], s[i], red_m[lrow], red_s[lrow]);
        part[(row0 + lrow) * n_vt + vt] = float2{m[i], s[i]};
      }
    }
  } else {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const long row = row0 + wm * 64 + i * 16 + (lane & 15);
      if (row >= n_rows) continue;
      const float M = gmax[row];
      const float inv_s = 1.f / gsum[row];
      const float go = gout[row];
      const long t = targets[row] - vocab_start;
#pragma unroll
      for (int half = 0; half < 2; ++half) {
        const int col = cbase + half * 8;
        if (col >= V) continue;  // V % 8 == 0: the vector is in or out whole
        Pack16B o;
        bf16* ov = (bf16*)&o;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const float v = acc[i][half * 2 + (e >> 2)][e & 3];
          const float p = __expf(v - M) * inv_s - (col + e == t ? 1.f : 0.f);
          ov[e] = f2bf(p * go);  // the only rounding
        }
        *(int4*)(ds + row * V + col) = o.i4;
      }
    }
  }
}

__global__ __launch_bounds__(256) void lmhead_ce_merge_kernel(
    const float2* __restrict__ part, float* __restrict__ row_max,
    float* __restrict__ row_sumexp, long N, int n_vt) {
  const long row = (long)blockIdx.x * 256 + threadIdx.x;
  if (row >= N) return;
  const float2* p = part + row * n_vt;
  float m = p[0].x, s = p[0].y;
  for (int t = 1; t < n_vt; ++t) combine(m, s, p[t].x, p[t].y);
  row_max[row] = m;
  row_sumexp[row] = s;
}

}  // namespace

extern "C" {
void launch_lmhead_ce_fwd(const void* hidden, const void* weight,
                          const void* targets, void* part, void* tgt, long N,
                          int H, int V, long vocab_start, hipStream_t stream) {
  if (N <= 0) return;
  const int n_mt = (int)lmhead_tiles(N, LMHEAD_BM), n_vt = lmhead_vtiles(V);
  lmhead_ce_kernel<STATS><<<dim3((unsigned)(n_mt * n_vt)), NT, 0, stream>>>(
      (const bf16*)hidden, (const bf16*)weight, (const long*)targets,
      (float2*)part, (float*)tgt, nullptr, nullptr, nullptr, nullptr, N, H, V,
      vocab_start, n_mt, n_vt);
  HIP_CHECK_LAST();
}

void launch_lmhead_ce_merge(const void* part, void* row_max, void* row_sumexp,
                            long N, int n_vt, hipStream_t stream) {
  if (N <= 0) return;
  lmhead_ce_merge_kernel<<<dim3((unsigned)((N + 255) / 256)), 256, 0,
                           stream>>>((const float2*)part, (float*)row_max,
                                     (float*)row_sumexp, N, n_vt);
  HIP_CHECK_LAST();
}

void launch_lmhead_ce_dlogits(const void* hidden, const void* weight,
                              const void* targets, const void* gmax,
                              const void* gsum, const void* gout, void* ds,
                              long rows, int H, int V, long vocab_start,
                              hipStream_t stream) {
  if (rows <= 0) return;
  const int n_mt = (int)lmhead_tiles(rows, LMHEAD_BM), n_vt = lmhead_vtiles(V);
  lmhead_ce_kernel<DLOGITS><<<dim3((unsigned)(n_mt * n_vt)), NT, 0, stream>>>(
      (const bf16*)hidden, (const bf16*)weight, (const long*)targets, nullptr,
      nullptr, (const float*)gmax, (const float*)gsum, (const float*)gout,
      (bf16*)ds, rows, H, V, vocab_start, n_mt, n_vt);
  HIP_CHECK_LAST();
}
}
