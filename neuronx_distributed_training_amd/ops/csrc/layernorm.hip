// LayerNorm forward/backward for MI355X: y = (x - mean) * rstd * w + b with
// the biased variance (torch's definition). bf16 IO in 16-byte vectors, fp32
// arithmetic; mean / rstd [N] fp32 travel from the forward to the backward.
//
// Three forms, chosen by the launcher from H (layernorm_form in launch.h):
//   wave   H <= 2048: one 64-lane wave owns a row, its H / 64 elements live in
//          registers (VPL 16-byte vectors per lane), every row reduction is a
//          cross-lane butterfly: no LDS, no barrier in the row loop. A block
//          is 4 waves = 4 rows at a time, striding over the rows.
//   block  2048 < H <= 8192: the row is register-resident across 256 threads
//          (VPT vectors per thread), reductions through LDS.
//   looped longer rows: the row is read twice.
// Statistics: the mean first, then the squared deviations of the held values;
// the first mean's own rounding error is measured by the same pass (sum of
// the deviations) and taken out, so neither the mean nor the variance carries
// the cancellation of E[x^2] - mean^2. The looped form merges per-vector
// (count, mean, M2) triples (Chan et al.) instead.
// Backward: g = dy * w, xh = (x - mean) * rstd,
//   dx = rstd * (g - mean(g) - xh * mean(g * xh)),
// the two row sums reduced as a pair. dw = sum_rows dy * xh and db = sum_rows
// dy in two stages without atomics: a lane (thread) owns the same columns in
// every row it sees, so it accumulates them in registers over the block's
// whole row loop; the block stores one fp32 partial [2, H] into part[grid, 2,
// H] (the wave form after combining its 4 waves once through LDS, in wave
// order), and layernorm_dwdb_kernel sums the partials over the grid in a
// fixed order. Two runs are bit-equal.
#include "common.h"
#include "launch.h"

namespace {

constexpr int NT = 256;      // threads per block
constexpr int NW = NT / 64;  // waves per block

DEVINL void unpack8(const int4& v, float* f) {
  Pack16B p;
  p.i4 = v;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    bf16x2 h = (&p.h8.a)[j];
    f[2 * j] = bf2f(h.x);
    f[2 * j + 1] = bf2f(h.y);
  }
}

DEVINL int4 pack8(const float* f) {
  Pack16B o;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    bf16x2 h;
    h.x = f2bf(f[2 * j]);
    h.y = f2bf(f[2 * j + 1]);
    (&o.h8.a)[j] = h;
  }
  return o.i4;
}

// butterfly all-reduce: every lane ends with the same bits (a + b == b + a)
DEVINL float wave_allsum(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}
DEVINL void wave_allsum2(float& a, float& b) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    a += __shfl_xor(a, off, 64);
    b += __shfl_xor(b, off, 64);
  }
}

// block all-reduce of a pair; red holds 2 * NW floats and is free again on
// return
DEVINL void block_allsum2(float& a, float& b, float* red) {
  wave_allsum2(a, b);
  if ((threadIdx.x & 63) == 0) {
    red[threadIdx.x >> 6] = a;
    red[NW + (threadIdx.x >> 6)] = b;
  }
  __syncthreads();
  a = 0.f;
  b = 0.f;
#pragma unroll
  for (int k = 0; k < NW; ++k) {
    a += red[k];
    b += red[NW + k];
  }
  __syncthreads();
}

DEVINL float rstd_of(float var, float eps) {
  // once per row: rounded once from fp64
  return (float)(1.0 / sqrt((double)var + (double)eps));
}

// One row held as VN vectors per owner (a lane of a wave, or a thread of a
// block): owner `own` of `stride` holds vectors own + v * stride < nvec.
// Leaves xf = x - m0 and returns the correction c (mean = m0 + c) and rstd.
template <int VN, bool WAVE>
DEVINL void row_stats(float (&xf)[VN][8], int own, int stride, int nvec,
                      int H, float eps, float* red, float& m0, float& c,
                      float& r) {
  float s = 0.f, z = 0.f;
#pragma unroll
  for (int v = 0; v < VN; ++v)
    if (own + v * stride < nvec) {
#pragma unroll
      for (int j = 0; j < 8; ++j) s += xf[v][j];
    }
  if constexpr (WAVE) s = wave_allsum(s); else block_allsum2(s, z, red);
  m0 = s / (float)H;
  float sd = 0.f, sq = 0.f;
#pragma unroll
  for (int v = 0; v < VN; ++v)
    if (own + v * stride < nvec) {
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float d = xf[v][j] - m0;
        xf[v][j] = d;
        sd += d;
        sq += d * d;
      }
    }
  if constexpr (WAVE) wave_allsum2(sd, sq); else block_allsum2(sd, sq, red);
  c = sd / (float)H;
  // sum (x - mean)^2 = sum d^2 - H c^2: c is m0's rounding error, tiny
  r = rstd_of(fmaxf(sq / (float)H - c * c, 0.f), eps);
}

template <int VN>
DEVINL void store_y(const float (&xf)[VN][8], int own, int stride, int nvec,
                    const int4* __restrict__ w, const int4* __restrict__ b,
                    int4* __restrict__ yr, float c, float r) {
#pragma unroll
  for (int v = 0; v < VN; ++v) {
    const int i = own + v * stride;
    if (i < nvec) {
      float wf[8], bf[8], o[8];
      unpack8(w[i], wf);
      unpack8(b[i], bf);
#pragma unroll
      for (int j = 0; j < 8; ++j) o[j] = (xf[v][j] - c) * r * wf[j] + bf[j];
      yr[i] = pack8(o);
    }
  }
}

// ---------------- forward ----------------
template <int VPL>
__global__ void __launch_bounds__(NT)
layernorm_fwd_wave_kernel(const bf16* __restrict__ x,
                          const bf16* __restrict__ w,
                          const bf16* __restrict__ b, bf16* __restrict__ y,
                          float* __restrict__ mean, float* __restrict__ rstd,
                          long N, int H, float eps) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int nvec = H >> 3;  // H % 8 == 0
  for (long row = blockIdx.x * (long)NW + wid; row < N;
       row += (long)gridDim.x * NW) {
    const int4* xr = (const int4*)(x + row * H);
    float xf[VPL][8];
#pragma unroll
    for (int v = 0; v < VPL; ++v)
      if (lane + v * 64 < nvec) unpack8(xr[lane + v * 64], xf[v]);
    float m0, c, r;
    row_stats<VPL, true>(xf, lane, 64, nvec, H, eps, nullptr, m0, c, r);
    if (lane == 0) {
      mean[row] = m0 + c;
      rstd[row] = r;
    }
    store_y<VPL>(xf, lane, 64, nvec, (const int4*)w, (const int4*)b,
                 (int4*)(y + row * H), c, r);
  }
}

template <int VPT>
__global__ void __launch_bounds__(NT)
layernorm_fwd_block_kernel(const bf16* __restrict__ x,
                           const bf16* __restrict__ w,
                           const bf16* __restrict__ b, bf16* __restrict__ y,
                           float* __restrict__ mean, float* __restrict__ rstd,
                           int H, float eps) {
  __shared__ float red[2 * NW];
  const long row = blockIdx.x;
  const int tid = threadIdx.x, nvec = H >> 3;
  const int4* xr = (const int4*)(x + row * H);
  float xf[VPT][8];
#pragma unroll
  for (int v = 0; v < VPT; ++v)
    if (tid + v * NT < nvec) unpack8(xr[tid + v * NT], xf[v]);
  float m0, c, r;
  row_stats<VPT, false>(xf, tid, NT, nvec, H, eps, red, m0, c, r);
  if (tid == 0) {
    mean[row] = m0 + c;
    rstd[row] = r;
  }
  store_y<VPT>(xf, tid, NT, nvec, (const int4*)w, (const int4*)b,
               (int4*)(y + row * H), c, r);
}

// (count, mean, M2) of b merged into a. The mean moves by a fraction of the
// difference, so its error scales with the spread, not with the offset.
DEVINL void chan_merge(float& n, float& mu, float& m2, float on, float omu,
                       float om2) {
  const float nn = n + on;
  if (nn > 0.f) {
    const float dl = omu - mu;
    mu += dl * (on / nn);
    m2 = (m2 + om2) + dl * dl * (n * on / nn);
  }
  n = nn;
}

__global__ void __launch_bounds__(NT)
layernorm_fwd_looped_kernel(const bf16* __restrict__ x,
                            const bf16* __restrict__ w,
                            const bf16* __restrict__ b, bf16* __restrict__ y,
                            float* __restrict__ mean,
                            float* __restrict__ rstd, int H, float eps) {
  __shared__ float red[3 * NW];
  const long row = blockIdx.x;
  const int tid = threadIdx.x, nvec = H >> 3;
  const int4* xr = (const int4*)(x + row * H);
  float n = 0.f, mu = 0.f, m2 = 0.f;
  for (int i = tid; i < nvec; i += NT) {
    float f[8];
    unpack8(xr[i], f);
    float vs = 0.f, vq = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) vs += f[j];
    const float vm = vs * 0.125f;
#pragma unroll
    for (int j = 0; j < 8; ++j) vq += (f[j] - vm) * (f[j] - vm);
    chan_merge(n, mu, m2, 8.f, vm, vq);
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1)
    chan_merge(n, mu, m2, __shfl_xor(n, off, 64), __shfl_xor(mu, off, 64),
               __shfl_xor(m2, off, 64));
  if ((tid & 63) == 0) {
    red[tid >> 6] = n;
    red[NW + (tid >> 6)] = mu;
    red[2 * NW + (tid >> 6)] = m2;
  }
  __syncthreads();
  n = 0.f, mu = 0.f, m2 = 0.f;
#pragma unroll
  for (int k = 0; k < NW; ++k)
    chan_merge(n, mu, m2, red[k], red[NW + k], red[2 * NW + k]);
  const float r = rstd_of(m2 / (float)H, eps);
  if (tid == 0) {
    mean[row] = mu;
    rstd[row] = r;
  }
  int4* yr = (int4*)(y + row * H);
  for (int i = tid; i < nvec; i += NT) {
    float f[8], wf[8], bf[8], o[8];
    unpack8(xr[i], f);
    unpack8(((const int4*)w)[i], wf);
    unpack8(((const int4*)b)[i], bf);
#pragma unroll
    for (int j = 0; j < 8; ++j) o[j] = (f[j] - mu) * r * wf[j] + bf[j];
    yr[i] = pack8(o);
  }
}

// ---------------- backward ----------------
// One vector of a row: g and xh for the dx pass, the row sums s1 = sum g and
// s2 = sum g * xh, and (ACC) the owner's column sums aw += dy * xh, ab += dy.
template <bool ACC = true>
DEVINL void bwd_vec(const int4& vdy, const int4& vx, const int4& vw, float m,
                    float r, float* g, float* xh, float& s1, float& s2,
                    float* aw, float* ab) {
  float d[8], wf[8];
  unpack8(vdy, d);
  unpack8(vx, xh);
  unpack8(vw, wf);
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    xh[j] = (xh[j] - m) * r;
    if (ACC) {
      aw[j] += d[j] * xh[j];
      ab[j] += d[j];
    }
    g[j] = d[j] * wf[j];
    s1 += g[j];
    s2 += g[j] * xh[j];
  }
}

DEVINL int4 dx_vec(const float* g, const float* xh, float r, float c1,
                   float c2) {
  float o[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) o[j] = r * (g[j] - c1 - xh[j] * c2);
  return pack8(o);
}

DEVINL void store_cols(float* dst, const float* a) {
  ((float4*)dst)[0] = make_float4(a[0], a[1], a[2], a[3]);
  ((float4*)dst)[1] = make_float4(a[4], a[5], a[6], a[7]);
}

DEVINL void load_cols(const float* src, float* a) {
  const float4 lo = ((const float4*)src)[0], hi = ((const float4*)src)[1];
  a[0] = lo.x, a[1] = lo.y, a[2] = lo.z, a[3] = lo.w;
  a[4] = hi.x, a[5] = hi.y, a[6] = hi.z, a[7] = hi.w;
}

template <int VPL>
__global__ void __launch_bounds__(NT)
layernorm_bwd_wave_kernel(const bf16* __restrict__ dy,
                          const bf16* __restrict__ x,
                          const bf16* __restrict__ w,
                          const float* __restrict__ mean,
                          const float* __restrict__ rstd,
                          bf16* __restrict__ dx,
                          float* __restrict__ part /* [grid, 2, H] */, long N,
                          int H) {
  // [VPL][2][8][64]: a lane's column sums, lane-contiguous (no bank conflict)
  __shared__ float lds[VPL * 2 * 8 * 64];
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int nvec = H >> 3;
  const float invH = 1.f / (float)H;
  float aw[VPL][8], ab[VPL][8];
#pragma unroll
  for (int v = 0; v < VPL; ++v)
#pragma unroll
    for (int j = 0; j < 8; ++j) aw[v][j] = ab[v][j] = 0.f;

  for (long row = blockIdx.x * (long)NW + wid; row < N;
       row += (long)gridDim.x * NW) {
    const int4* dyr = (const int4*)(dy + row * H);
    const int4* xr = (const int4*)(x + row * H);
    const float m = mean[row], r = rstd[row];
    float g[VPL][8], xh[VPL][8];
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int v = 0; v < VPL; ++v) {
      const int i = lane + v * 64;
      if (i < nvec)
        bwd_vec(dyr[i], xr[i], ((const int4*)w)[i], m, r, g[v], xh[v], s1, s2,
                aw[v], ab[v]);
    }
    wave_allsum2(s1, s2);
    const float c1 = s1 * invH, c2 = s2 * invH;
    int4* dxr = (int4*)(dx + row * H);
#pragma unroll
    for (int v = 0; v < VPL; ++v) {
      const int i = lane + v * 64;
      if (i < nvec) dxr[i] = dx_vec(g[v], xh[v], r, c1, c2);
    }
  }

  // the block's 4 waves, once, in wave order: ((w0 + w1) + w2) + w3
  for (int k = 0; k < NW; ++k) {
    if (wid == k) {
#pragma unroll
      for (int v = 0; v < VPL; ++v)
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          float* pw = lds + ((v * 2 + 0) * 8 + j) * 64 + lane;
          float* pb = lds + ((v * 2 + 1) * 8 + j) * 64 + lane;
          if (k == 0) {
            *pw = aw[v][j];
            *pb = ab[v][j];
          } else if (k < NW - 1) {
            *pw += aw[v][j];
            *pb += ab[v][j];
          } else {
            aw[v][j] += *pw;
            ab[v][j] += *pb;
          }
        }
    }
    __syncthreads();
  }
  if (wid == NW - 1) {
    float* slab = part + (long)blockIdx.x * 2 * H;
#pragma unroll
    for (int v = 0; v < VPL; ++v) {
      const int i = lane + v * 64;
      if (i < nvec) {
        store_cols(slab + (i << 3), aw[v]);
        store_cols(slab + H + (i << 3), ab[v]);
      }
    }
  }
}

template <int VPT>
__global__ void __launch_bounds__(NT)
layernorm_bwd_block_kernel(const bf16* __restrict__ dy,
                           const bf16* __restrict__ x,
                           const bf16* __restrict__ w,
                           const float* __restrict__ mean,
                           const float* __restrict__ rstd,
                           bf16* __restrict__ dx, float* __restrict__ part,
                           long N, int H) {
  __shared__ float red[2 * NW];
  const int tid = threadIdx.x, nvec = H >> 3;
  const float invH = 1.f / (float)H;
  float aw[VPT][8], ab[VPT][8];
#pragma unroll
  for (int v = 0; v < VPT; ++v)
#pragma unroll
    for (int j = 0; j < 8; ++j) aw[v][j] = ab[v][j] = 0.f;

  for (long row = blockIdx.x; row < N; row += gridDim.x) {
    const int4* dyr = (const int4*)(dy + row * H);
    const int4* xr = (const int4*)(x + row * H);
    const float m = mean[row], r = rstd[row];
    float g[VPT][8], xh[VPT][8];
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int v = 0; v < VPT; ++v) {
      const int i = tid + v * NT;
      if (i < nvec)
        bwd_vec(dyr[i], xr[i], ((const int4*)w)[i], m, r, g[v], xh[v], s1, s2,
                aw[v], ab[v]);
    }
    block_allsum2(s1, s2, red);
    const float c1 = s1 * invH, c2 = s2 * invH;
    int4* dxr = (int4*)(dx + row * H);
#pragma unroll
    for (int v = 0; v < VPT; ++v) {
      const int i = tid + v * NT;
      if (i < nvec) dxr[i] = dx_vec(g[v], xh[v], r, c1, c2);
    }
  }
  // every thread owns its columns alone: no combine inside the block
  float* slab = part + (long)blockIdx.x * 2 * H;
#pragma unroll
  for (int v = 0; v < VPT; ++v) {
    const int i = tid + v * NT;
    if (i < nvec) {
      store_cols(slab + (i << 3), aw[v]);
      store_cols(slab + H + (i << 3), ab[v]);
    }
  }
}

// Rows too long for registers: dy and x are read twice, and the column sums
// live in the block's own slab of part, which only the owning thread of a
// column reads and writes (plain loads and stores, no atomics).
__global__ void __launch_bounds__(NT)
layernorm_bwd_looped_kernel(const bf16* __restrict__ dy,
                            const bf16* __restrict__ x,
                            const bf16* __restrict__ w,
                            const float* __restrict__ mean,
                            const float* __restrict__ rstd,
                            bf16* __restrict__ dx, float* part, long N,
                            int H) {
  __shared__ float red[2 * NW];
  const int tid = threadIdx.x, nvec = H >> 3;
  const float invH = 1.f / (float)H;
  float* slab = part + (long)blockIdx.x * 2 * H;
  const float zero[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  for (int i = tid; i < nvec; i += NT) {
    store_cols(slab + (i << 3), zero);
    store_cols(slab + H + (i << 3), zero);
  }
  for (long row = blockIdx.x; row < N; row += gridDim.x) {
    const int4* dyr = (const int4*)(dy + row * H);
    const int4* xr = (const int4*)(x + row * H);
    const float m = mean[row], r = rstd[row];
    float s1 = 0.f, s2 = 0.f;
    for (int i = tid; i < nvec; i += NT) {
      float g[8], xh[8];
      bwd_vec<false>(dyr[i], xr[i], ((const int4*)w)[i], m, r, g, xh, s1, s2,
                     nullptr, nullptr);
    }
    block_allsum2(s1, s2, red);
    const float c1 = s1 * invH, c2 = s2 * invH;
    int4* dxr = (int4*)(dx + row * H);
    for (int i = tid; i < nvec; i += NT) {
      float g[8], xh[8], aw[8], ab[8], t1 = 0.f, t2 = 0.f;
      load_cols(slab + (i << 3), aw);
      load_cols(slab + H + (i << 3), ab);
      bwd_vec(dyr[i], xr[i], ((const int4*)w)[i], m, r, g, xh, t1, t2, aw, ab);
      dxr[i] = dx_vec(g, xh, r, c1, c2);
      store_cols(slab + (i << 3), aw);
      store_cols(slab + H + (i << 3), ab);
    }
  }
}

// out[c] = sum over g of part[g, c], c over the 2 * H columns of [dw | db]:
// 64 columns a block, the grid dimension split over 8 waves, each summing
// its share in order (in fp64: exact enough that the order of the 8 is the
// only one that matters), wave 0 adds the 8 in order.
__global__ void __launch_bounds__(512)
layernorm_dwdb_kernel(const float* __restrict__ part, float* __restrict__ out,
                      int G, int C) {
  __shared__ double lds[8][64];
  const int lane = threadIdx.x & 63, sl = threadIdx.x >> 6;
  const int col = blockIdx.x * 64 + lane;
  double a = 0.0;
  if (col < C)
    for (int g = sl; g < G; g += 8) a += (double)part[(long)g * C + col];
  lds[sl][lane] = a;
  __syncthreads();
  if (sl == 0 && col < C) {
    double t = 0.0;
#pragma unroll
    for (int s = 0; s < 8; ++s) t += lds[s][lane];
    out[col] = (float)t;
  }
}

}  // namespace

extern "C" {
void launch_layernorm_fwd(const void* x, const void* w, const void* b, void* y,
                          void* mean, void* rstd, long N, int H, float eps,
                          int num_cu, hipStream_t stream) {
  if (N <= 0 || H <= 0) return;  // a grid of zero blocks is an invalid launch
  const bf16 *xp = (const bf16*)x, *wp = (const bf16*)w, *bp = (const bf16*)b;
  bf16* yp = (bf16*)y;
  float *mp = (float*)mean, *rp = (float*)rstd;
  const int vn = layernorm_vecs(H);
  if (layernorm_form(H) == LN_WAVE) {
    const long want = (N + NW - 1) / NW, cap = 8L * num_cu;
    const dim3 grid((unsigned)(want < cap ? want : cap)), block(NT);
    switch (vn) {
      case 1:
        layernorm_fwd_wave_kernel<1><<<grid, block, 0, stream>>>(
            xp, wp, bp, yp, mp, rp, N, H, eps);
        break;
      case 2:
        layernorm_fwd_wave_kernel<2><<<grid, block, 0, stream>>>(
            xp, wp, bp, yp, mp, rp, N, H, eps);
        break;
      default:
        layernorm_fwd_wave_kernel<4><<<grid, block, 0, stream>>>(
            xp, wp, bp, yp, mp, rp, N, H, eps);
    }
  } else {
    const dim3 grid((unsigned)N), block(NT);
    switch (vn) {
      case 2:
        layernorm_fwd_block_kernel<2><<<grid, block, 0, stream>>>(
            xp, wp, bp, yp, mp, rp, H, eps);
        break;
      case 4:
        layernorm_fwd_block_kernel<4><<<grid, block, 0, stream>>>(
            xp, wp, bp, yp, mp, rp, H, eps);
        break;
      default:
        layernorm_fwd_looped_kernel<<<grid, block, 0, stream>>>(
            xp, wp, bp, yp, mp, rp, H, eps);
    }
  }
  HIP_CHECK_LAST();
}

void launch_layernorm_bwd(const void* dy, const void* x, const void* w,
                          const void* mean, const void* rstd, void* dx,
                          void* part, void* dwdb, long N, int H, int grid_n,
                          hipStream_t stream) {
  if (N <= 0 || H <= 0) return;
  const bf16 *dp = (const bf16*)dy, *xp = (const bf16*)x,
             *wp = (const bf16*)w;
  const float *mp = (const float*)mean, *rp = (const float*)rstd;
  bf16* dxp = (bf16*)dx;
  float* pp = (float*)part;
  const dim3 grid((unsigned)grid_n), block(NT);
  const int vn = layernorm_vecs(H);
  if (layernorm_form(H) == LN_WAVE) {
    switch (vn) {
      case 1:
        layernorm_bwd_wave_kernel<1><<<grid, block, 0, stream>>>(
            dp, xp, wp, mp, rp, dxp, pp, N, H);
        break;
      case 2:
        layernorm_bwd_wave_kernel<2><<<grid, block, 0, stream>>>(
            dp, xp, wp, mp, rp, dxp, pp, N, H);
        break;
      default:
        layernorm_bwd_wave_kernel<4><<<grid, block, 0, stream>>>(
            dp, xp, wp, mp, rp, dxp, pp, N, H);
    }
  } else {
    switch (vn) {
      case 2:
        layernorm_bwd_block_kernel<2><<<grid, block, 0, stream>>>(
            dp, xp, wp, mp, rp, dxp, pp, N, H);
        break;
      case 4:
        layernorm_bwd_block_kernel<4><<<grid, block, 0, stream>>>(
            dp, xp, wp, mp, rp, dxp, pp, N, H);
        break;
      default:
        layernorm_bwd_looped_kernel<<<grid, block, 0, stream>>>(
            dp, xp, wp, mp, rp, dxp, pp, N, H);
    }
  }
  HIP_CHECK_LAST();
  const int C = 2 * H;
  layernorm_dwdb_kernel<<<dim3((C + 63) / 64), dim3(512), 0, stream>>>(
      pp, (float*)dwdb, grid_n, C);
  HIP_CHECK_LAST();
}
}
