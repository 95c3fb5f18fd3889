// LoRA adapter products on MI355X (gfx950): the three skinny GEMMs of
//   out = base + scaling * (x A^T) B^T
// and of its backward, each with one dimension of only r = 8..64. bf16 in,
// fp32 accumulation, one rounding per output.
//
//   lora_shrink : h[T, r]   = scale * X[T, W] M[r, W]^T   (contract the wide W)
//   lora_expand : out[T, N] = (base +) scale * h[T, r] M[N, r]^T   (contract r)
//   lora_wgrad  : G = scale * Y[T, W]^T Z[T, r]           (contract T)
//
// forward:  h = shrink(x, A);  out = expand(h, B, base_out, scaling)
// backward: dh = shrink(dout, B^T, scaling);  dx = expand(dh, A^T)
//           dB[N, r] = wgrad(dout, h, scaling);  dA[r, K] = wgrad(x, dh)
//
// Rows past T and columns past W / N / r are fed to the MFMA as zeros on
// BOTH operands (never loaded), and never stored. No atomics anywhere: every
// sum has one fixed order, so two runs are bit-equal.
//
// XCD remap (attn_common.h) is not used: the only operands that blocks share
// are M (<= 512 KB) and the [T, r] tensors, which stay resident in every
// XCD's 4 MB L2; the wide tensors are each read exactly once.
#include "attn_common.h"
#include "launch.h"

typedef short s16x4_t __attribute__((ext_vector_type(4)));
// K = 16 MFMA, four bf16 per lane: row / col = lane & 15 and
// k = (lane >> 4) * 4 + j on both operands; C / D as the 16x16x32 map.
#define MFMA_16x16x16(A, B, C) \
  __builtin_amdgcn_mfma_f32_16x16x16bf16_1k((A), (B), (C), 0, 0, 0)

namespace {

constexpr int SHRINK_WAVES = 8;   // waves that split one row tile's contraction
constexpr int SHRINK_ROWS = 16;   // rows of h per block
constexpr int EXPAND_TILE = 64;   // rows and columns of out per block
constexpr int WGRAD_BW = 64;      // columns of Y per block
constexpr int WGRAD_BT = 32;      // rows staged per step (one MFMA K)

DEVINL bf16x8_t zero8() {
  bf16x8_t z;
  *(int4*)&z = int4{0, 0, 0, 0};
  return z;
}

// ============================== shrink ==============================
// Block = 16 rows of X, 8 waves. Both MFMA operands are contiguous along the
// contraction, so each lane's fragment is one 16-byte global load (X: row
// lane & 15; M: row nj * 16 + (lane & 15); k = 8 * (lane >> 4) + j). M is read
// from global memory by every block and stays L2-resident. The W / 32
// k-windows are dealt to the waves in eight contiguous runs; the eight fp32
// partial tiles meet in LDS and are summed in wave order 0..7.
template <int R>
__global__ __launch_bounds__(512) void lora_shrink_kernel(
    const bf16* __restrict__ X,  // [T, W]
    const bf16* __restrict__ M,  // [R, W]
    bf16* __restrict__ H,        // [T, R]
    int T, int W, float scale) {
  constexpr int NJ = (R + 15) / 16, RP = NJ * 16;
  __shared__ float part[SHRINK_WAVES][SHRINK_ROWS][RP];

  const int lane = threadIdx.x & 63;
  const int wid = threadIdx.x >> 6;
  const long row0 = (long)blockIdx.x * SHRINK_ROWS;
  const long trow = row0 + (lane & 15);
  const bool row_ok = trow < T;
  const bf16* xp = X + (row_ok ? trow : 0) * W;

  const int nwin = (W + 31) / 32;
  const int per = (nwin + SHRINK_WAVES - 1) / SHRINK_WAVES;
  const int wbeg = wid * per;
  const int wend = wbeg + per < nwin ? wbeg + per : nwin;

  f32x4_t acc[NJ];
#pragma unroll
  for (int nj = 0; nj < NJ; ++nj) acc[nj] = f32x4_t{0.f, 0.f, 0.f, 0.f};

  for (int win = wbeg; win < wend; ++win) {
    const int k = win * 32 + (lane >> 4) * 8;
    const bool k_ok = k < W;  // W % 8 == 0: a lane's 8 k's are in or out together
    bf16x8_t a = zero8();
    if (row_ok && k_ok) *(int4*)&a = *(const int4*)(xp + k);
#pragma unroll
    for (int nj = 0; nj < NJ; ++nj) {
      const int c = nj * 16 + (lane & 15);
      bf16x8_t b = zero8();
      if (c < R && k_ok) *(int4*)&b = *(const int4*)(M + (long)c * W + k);
      acc[nj] = MFMA_16x16x32(a, b, acc[nj]);
    }
  }

#pragma unroll
  for (int nj = 0; nj < NJ; ++nj)
#pragma unroll
    for (int i = 0; i < 4; ++i)
      part[wid][(lane >> 4) * 4 + i][nj * 16 + (lane & 15)] = acc[nj][i];
  __syncthreads();

  for (int e = threadIdx.x; e < SHRINK_ROWS * R; e += 512) {
    const int row = e / R, c = e % R;
    float s = 0.f;
#pragma unroll
    for (int w = 0; w < SHRINK_WAVES; ++w) s += part[w][row][c];
    if (row0 + row < T) H[(row0 + row) * R + c] = f2bf(s * scale);
  }
}

// ============================== expand ==============================
// Block = 64 rows x 64 columns of out, one wave per 16 rows. Swapped operands:
// MFMA(A = M rows, B = h rows) gives C[n, t], so a lane holds four
// consecutive columns of ONE row t = lane & 15. MFMA j's row m stands for
// column (m >> 2) * 16 + j * 4 + (m & 3), which makes the sixteen values of a
// lane over j = 0..3 consecutive columns g * 16 .. g * 16 + 15 (g = lane >> 4):
// base is read and out written as two 16-byte vectors per lane, 128
// contiguous bytes per row. r <= 16 takes the K = 16 instruction (r = 8:
// upper k lanes zero), r = 32 / 64 one / two 16x16x32.
template <int R, bool HAS_BASE>
__global__ __launch_bounds__(256) void lora_expand_kernel(
    const bf16* __restrict__ Hh,    // [T, R]
    const bf16* __restrict__ M,     // [N, R]
    const bf16* __restrict__ base,  // [T, N] or null
    bf16* __restrict__ out,         // [T, N]
    int T, int N, float scale) {
  const int lane = threadIdx.x & 63;
  const int wid = threadIdx.x >> 6;
  const int g = lane >> 4, m = lane & 15;
  const long t = (long)blockIdx.x * EXPAND_TILE + wid * 16 + m;
  const int c0 = blockIdx.y * EXPAND_TILE;
  const bool t_ok = t < T;

  f32x4_t acc[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) acc[j] = f32x4_t{0.f, 0.f, 0.f, 0.f};

  if constexpr (R <= 16) {
    const int k = g * 4;
    const bool k_ok = k < R;
    s16x4_t hb = {0, 0, 0, 0};
    if (t_ok && k_ok) *(int2*)&hb = *(const int2*)(Hh + t * R + k);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int n = c0 + (m >> 2) * 16 + j * 4 + (m & 3);
      s16x4_t a = {0, 0, 0, 0};
      if (n < N && k_ok) *(int2*)&a = *(const int2*)(M + (long)n * R + k);
      acc[j] = MFMA_16x16x16(a, hb, acc[j]);
    }
  } else {
#pragma unroll
    for (int kk = 0; kk < R / 32; ++kk) {
      const int k = kk * 32 + g * 8;
      bf16x8_t hb = zero8();
      if (t_ok) *(int4*)&hb = *(const int4*)(Hh + t * R + k);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int n = c0 + (m >> 2) * 16 + j * 4 + (m & 3);
        bf16x8_t a = zero8();
        if (n < N) *(int4*)&a = *(const int4*)(M + (long)n * R + k);
        acc[j] = MFMA_16x16x32(a, hb, acc[j]);
      }
    }
  }

  if (!t_ok) return;
#pragma unroll
  for (int half = 0; half < 2; ++half) {
    const int n = c0 + g * 16 + half * 8;
    if (n >= N) continue;  // N % 8 == 0: the vector is in or out as a whole
    Pack16B b, o;
    if (HAS_BASE) b.i4 = *(const int4*)(base + t * N + n);
    bf16* ov = (bf16*)&o;
    const bf16* bv = (const bf16*)&b;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      float v = scale * acc[half * 2 + (e >> 2)][e & 3];
      if (HAS_BASE) v += bf2f(bv[e]);
      ov[e] = f2bf(v);  // the only rounding
    }
    *(int4*)(out + t * N + n) = o.i4;
  }
}

// ============================== wgrad ==============================
// Stage 1. Block = 64 columns of Y (one wave per 16) x all r columns of Z, over
// one chunk of LORA_WGRAD_CHUNK rows of T. Both operands need the contraction
// (t) contiguous per lane, so each 32-row step is staged through LDS as
// transposed images [column][t] with the tr_swz slot swizzle (row pairs
// written as one 4-byte store, read back as 16-byte fragments), as in
// moe_wgrad_kernel. The next step's global loads are issued before this
// step's MFMAs. Each block stores its fp32 partial [W, r] slab.
struct WgradRegs {
  int4 v0, v1;
};

template <int R>
DEVINL WgradRegs wgrad_load(const bf16* __restrict__ Y,
                            const bf16* __restrict__ Z, long tb, int T, int W,
                            int w0) {
  // threads 0..127: Y [32 t x 64 w] as 16 row pairs x 8 column groups;
  // threads 128..128 + 2R: Z [32 t x R] as 16 row pairs x R / 8 groups
  WgradRegs r{int4{0, 0, 0, 0}, int4{0, 0, 0, 0}};
  const int tid = threadIdx.x;
  if (tid < 128) {
    const long g0 = tb + (tid / 8) * 2;
    const int col = w0 + (tid % 8) * 8;
    if (col < W) {
      if (g0 < T) r.v0 = *(const int4*)(Y + g0 * W + col);
      if (g0 + 1 < T) r.v1 = *(const int4*)(Y + (g0 + 1) * W + col);
    }
  } else if (tid - 128 < 2 * R) {
    const int task = tid - 128;
    const long g0 = tb + (task / (R / 8)) * 2;
    const int col = (task % (R / 8)) * 8;
    if (g0 < T) r.v0 = *(const int4*)(Z + g0 * R + col);
    if (g0 + 1 < T) r.v1 = *(const int4*)(Z + (g0 + 1) * R + col);
  }
  return r;
}

template <int R, int IP>
DEVINL void wgrad_stage(const WgradRegs& r, __bf16* y_img, __bf16* z_img) {
  const int tid = threadIdx.x;
  __bf16* img;
  int trow, col8;
  if (tid < 128) {
    img = y_img;
    trow = (tid / 8) * 2;
    col8 = (tid % 8) * 8;
  } else if (tid - 128 < 2 * R) {
    img = z_img;
    trow = ((tid - 128) / (R / 8)) * 2;
    col8 = ((tid - 128) % (R / 8)) * 8;
  } else {
    return;
  }
  const __bf16* e0 = (const __bf16*)&r.v0;
  const __bf16* e1 = (const __bf16*)&r.v1;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    __bf16 pr[2] = {e0[j], e1[j]};
    const int row = col8 + j;  // image row = column of Y / Z
    *(uint*)((char*)img + tr_swz((uint)(row * IP + trow) * 2, row)) =
        *(uint*)pr;
  }
}

template <int R>
__global__ __launch_bounds__(256) void lora_wgrad_kernel(
    const bf16* __restrict__ Y,  // [T, W]
    const bf16* __restrict__ Z,  // [T, R]
    float* __restrict__ part,    // [chunks, W, R]
    int T, int W) {
  constexpr int IP = WGRAD_BT + 8;  // 80-byte image rows
  constexpr int NJ = (R + 15) / 16;
  // both images are whole multiples of 128 bytes, the span tr_swz permutes
  __shared__ __bf16 y_img[WGRAD_BW * IP];
  __shared__ __bf16 z_img[64 * IP];

  const int lane = threadIdx.x & 63;
  const int wid = threadIdx.x >> 6;
  const int w0 = blockIdx.x * WGRAD_BW;
  const long tbeg = (long)blockIdx.y * LORA_WGRAD_CHUNK;
  const long tend = tbeg + LORA_WGRAD_CHUNK < T ? tbeg + LORA_WGRAD_CHUNK : T;

  f32x4_t acc[NJ];
#pragma unroll
  for (int nj = 0; nj < NJ; ++nj) acc[nj] = f32x4_t{0.f, 0.f, 0.f, 0.f};

  WgradRegs regs = wgrad_load<R>(Y, Z, tbeg, T, W, w0);
  for (long tb = tbeg; tb < tend; tb += WGRAD_BT) {
    wgrad_stage<R, IP>(regs, y_img, z_img);
    __syncthreads();
    if (tb + WGRAD_BT < tend)
      regs = wgrad_load<R>(Y, Z, tb + WGRAD_BT, T, W, w0);
    // A: rows = columns of Y, B: columns = columns of Z, k = t
    bf16x8_t a = load_frag_b_trT_swz(y_img, IP, wid * 16, 0, lane);
#pragma unroll
    for (int nj = 0; nj < NJ; ++nj) {
      bf16x8_t b = zero8();  // r = 8: image rows 8..15 are never written
      if (nj * 16 + (lane & 15) < R)
        b = load_frag_b_trT_swz(z_img, IP, nj * 16, 0, lane);
      acc[nj] = MFMA_16x16x32(a, b, acc[nj]);
    }
    __syncthreads();
  }

  float* pp = part + (long)blockIdx.y * W * R;
#pragma unroll
  for (int nj = 0; nj < NJ; ++nj)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int w = w0 + wid * 16 + (lane >> 4) * 4 + i;
      const int c = nj * 16 + (lane & 15);
      if (w < W && c < R) pp[(long)w * R + c] = acc[nj][i];
    }
}

// Stage 2: the chunk partials summed in chunk order, scaled, rounded once and
// written in the parameter's layout: [W, r] (lora_B) or [r, W] (lora_A).
__global__ __launch_bounds__(256) void lora_wgrad_reduce_kernel(
    const float* __restrict__ part, bf16* __restrict__ G, int chunks, int W,
    int R, float scale, bool out_rw) {
  const long o = (long)blockIdx.x * 256 + threadIdx.x;
  if (o >= (long)W * R) return;
  const long w = out_rw ? o % W : o / R;
  const long c = out_rw ? o / W : o % R;
  float s = 0.f;
  for (int ch = 0; ch < chunks; ++ch) s += part[((long)ch * W + w) * R + c];
  G[o] = f2bf(s * scale);
}

template <int R>
void shrink_rank(const void* x, const void* m, void* h, int T, int W,
                 float scale, hipStream_t stream) {
  dim3 grid((T + SHRINK_ROWS - 1) / SHRINK_ROWS);
  lora_shrink_kernel<R><<<grid, 512, 0, stream>>>(
      (const bf16*)x, (const bf16*)m, (bf16*)h, T, W, scale);
}

template <int R>
void expand_rank(const void* h, const void* m, const void* base, void* out,
                 int T, int N, float scale, hipStream_t stream) {
  dim3 grid((T + EXPAND_TILE - 1) / EXPAND_TILE,
            (N + EXPAND_TILE - 1) / EXPAND_TILE);
  if (base)
    lora_expand_kernel<R, true><<<grid, 256, 0, stream>>>(
        (const bf16*)h, (const bf16*)m, (const bf16*)base, (bf16*)out, T, N,
        scale);
  else
    lora_expand_kernel<R, false><<<grid, 256, 0, stream>>>(
        (const bf16*)h, (const bf16*)m, nullptr, (bf16*)out, T, N, scale);
}

template <int R>
void wgrad_rank(const void* y, const void* z, void* part, int T, int W,
                hipStream_t stream) {
  dim3 grid((W + WGRAD_BW - 1) / WGRAD_BW, lora_wgrad_chunks(T));
  lora_wgrad_kernel<R><<<grid, 256, 0, stream>>>(
      (const bf16*)y, (const bf16*)z, (float*)part, T, W);
}

}  // namespace

// one instantiation per supported rank; the bindings admit no other
#define LORA_BY_RANK(R, FN, ...)                   \
  switch (R) {                                     \
    case 8: FN<8>(__VA_ARGS__); break;             \
    case 16: FN<16>(__VA_ARGS__); break;           \
    case 32: FN<32>(__VA_ARGS__); break;           \
    case 64: FN<64>(__VA_ARGS__); break;           \
    default:                                       \
      throw std::runtime_error("lora: rank must be 8, 16, 32 or 64"); \
  }

extern "C" {
void launch_lora_shrink(const void* x, const void* m, void* h, int T, int W,
                        int R, float scale, hipStream_t stream) {
  if (T == 0) return;
  LORA_BY_RANK(R, shrink_rank, x, m, h, T, W, scale, stream);
  HIP_CHECK_LAST();
}

void launch_lora_expand(const void* h, const void* m, const void* base,
                        void* out, int T, int N, int R, float scale,
                        hipStream_t stream) {
  if (T == 0) return;
  LORA_BY_RANK(R, expand_rank, h, m, base, out, T, N, scale, stream);
  HIP_CHECK_LAST();
}

void launch_lora_wgrad(const void* y, const void* z, void* part, void* g,
                       int T, int W, int R, float scale, bool out_rw,
                       hipStream_t stream) {
  const int chunks = lora_wgrad_chunks(T);  // 0 when T == 0: G = 0
  if (chunks > 0) {
    LORA_BY_RANK(R, wgrad_rank, y, z, part, T, W, stream);
    HIP_CHECK_LAST();
  }
  const long n = (long)W * R;
  lora_wgrad_reduce_kernel<<<(unsigned)((n + 255) / 256), 256, 0, stream>>>(
      (const float*)part, (bf16*)g, chunks, W, R, scale, out_rw);
  HIP_CHECK_LAST();
}
}
