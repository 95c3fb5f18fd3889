// RMSNorm forward/backward for MI355X — one HBM pass each way.
// Replaces the reference's apex/NxD RMSNorm.
// bf16 IO, fp32 accumulate; vectorized 8×bf16 (16 B) loads per lane
// (guide: scalar bf16 loads are a 2× loss on this op).
#include "common.h"
#include "launch.h"

// ---------------- forward ----------------
// x: [N, H] bf16, w: [H] bf16 -> y: [N, H] bf16, invrms: [N] f32.
// One block of 256 threads per row.
template <int NT>
__global__ void rmsnorm_fwd_kernel(const bf16* __restrict__ x,
                                   const bf16* __restrict__ w,
                                   bf16* __restrict__ y,
                                   float* __restrict__ invrms,
                                   int H, float eps) {
  __shared__ float lds[NT / 64];
  const int row = blockIdx.x;
  const bf16* xr = x + (long)row * H;
  bf16* yr = y + (long)row * H;
  float ss = 0.f;
  const int nvec = H >> 3;  // H % 8 == 0
  for (int i = threadIdx.x; i < nvec; i += NT) {
    Pack16B p;
    p.i4 = ((const int4*)xr)[i];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      bf16x2 h = (&p.h8.a)[j];
      float lo = bf2f(h.x), hi = bf2f(h.y);
      ss += lo * lo + hi * hi;
    }
  }
  ss = block_reduce_sum<NT>(ss, lds);
  float r = rsqrtf(ss / (float)H + eps);
  if (threadIdx.x == 0) invrms[row] = r;
  for (int i = threadIdx.x; i < nvec; i += NT) {
    Pack16B p, pw, o;
    p.i4 = ((const int4*)xr)[i];
    pw.i4 = ((const int4*)w)[i];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      bf16x2 h = (&p.h8.a)[j];
      bf16x2 hw = (&pw.h8.a)[j];
      bf16x2 res;
      res.x = f2bf(bf2f(h.x) * r * bf2f(hw.x));
      res.y = f2bf(bf2f(h.y) * r * bf2f(hw.y));
      (&o.h8.a)[j] = res;
    }
    ((int4*)yr)[i] = o.i4;
  }
}

// ---------------- backward ----------------
// dx = r*(w*dy - xhat * mean(w*dy*xhat));  dw = sum_rows(dy * xhat)
// Grid-stride over rows; per-block dw accumulated in LDS fp32 then one
// atomicAdd pass (contention = gridDim, not N).
template <int NT>
__global__ void rmsnorm_bwd_kernel(const bf16* __restrict__ dy,
                                   const bf16* __restrict__ x,
                                   const bf16* __restrict__ w,
                                   const float* __restrict__ invrms,
                                   bf16* __restrict__ dx,
                                   float* __restrict__ dw /* [H] f32, zeroed */,
                                   int N, int H) {
  extern __shared__ float smem[];          // [H] dw accum + [NT/64] reduce
  float* dw_lds = smem;
  float* red = smem + H;
  for (int i = threadIdx.x; i < H; i += NT) dw_lds[i] = 0.f;
  __syncthreads();

  const int nvec = H >> 3;
  for (int row = blockIdx.x; row < N; row += gridDim.x) {
    const bf16* dyr = dy + (long)row * H;
    const bf16* xr = x + (long)row * H;
    bf16* dxr = dx + (long)row * H;
    const float r = invrms[row];
    // pass 1: c = mean(w*dy*xhat)
    float c = 0.f;
    for (int i = threadIdx.x; i < nvec; i += NT) {
      Pack16B pd, px, pw;
      pd.i4 = ((const int4*)dyr)[i];
      px.i4 = ((const int4*)xr)[i];
      pw.i4 = ((const int4*)w)[i];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        bf16x2 hd = (&pd.h8.a)[j], hx = (&px.h8.a)[j], hw = (&pw.h8.a)[j];
        c += bf2f(hw.x) * bf2f(hd.x) * bf2f(hx.x) * r;
        c += bf2f(hw.y) * bf2f(hd.y) * bf2f(hx.y) * r;
      }
    }
    c = block_reduce_sum<NT>(c, red) / (float)H;
    // pass 2: dx store + dw partial accumulation (LDS).
    // Each thread owns fixed columns (i strided by NT) so the dw_lds adds
    // are conflict-free plain adds, no atomics needed within a block.
    for (int i = threadIdx.x; i < nvec; i += NT) {
      Pack16B pd, px, pw, o;
      pd.i4 = ((const int4*)dyr)[i];
      px.i4 = ((const int4*)xr)[i];
      pw.i4 = ((const int4*)w)[i];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        bf16x2 hd = (&pd.h8.a)[j], hx = (&px.h8.a)[j], hw = (&pw.h8.a)[j];
        float xh0 = bf2f(hx.x) * r, xh1 = bf2f(hx.y) * r;
        float d0 = bf2f(hd.x), d1 = bf2f(hd.y);
        bf16x2 res;
        res.x = f2bf((bf2f(hw.x) * d0 - xh0 * c) * r);
        res.y = f2bf((bf2f(hw.y) * d1 - xh1 * c) * r);
        (&o.h8.a)[j] = res;
        const int col = (i << 3) + (j << 1);
        dw_lds[col] += d0 * xh0;
        dw_lds[col + 1] += d1 * xh1;
      }
      ((int4*)dxr)[i] = o.i4;
    }
  }
  __syncthreads();
  // flush dw partials
  for (int i = threadIdx.x; i < H; i += NT) atomicAdd(&dw[i], dw_lds[i]);
}

// ---------------- fused residual add + RMSNorm ----------------
// h = bf16(x + delta), then the norm of the ROUNDED h: every output is
// bit-equal to torch's bf16 add followed by the kernels above. Their fp32
// arithmetic is pinned here to what the compiler made of it there (read from
// the ISA): contraction is off in the helpers below and each fused
// multiply-add is written out.
//   sum of squares  ss += fma(lo, lo, hi * hi) per bf16 pair
//   c               c  += ((w * dy) * x) * r
//   dx              fma(dy, w, -((x * r) * c)) * r
//   dw              dw = fma(dy, x * r, dw)
// A row of up to VPT * NT vectors stays in registers between the reduction
// and the pass that needs it again (H = 4096: 2 vectors per thread);
// VPT = 0 is the looped form for longer rows, which reads the row twice.

// (Pack16B has no copy constructor: vectors travel as int4.)
DEVINL int4 add8(const int4& xa, const int4& xb) {
  Pack16B a, b, o;
  a.i4 = xa;
  b.i4 = xb;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    bf16x2 ha = (&a.h8.a)[j], hb = (&b.h8.a)[j], res;
    res.x = f2bf(bf2f(ha.x) + bf2f(hb.x));
    res.y = f2bf(bf2f(ha.y) + bf2f(hb.y));
    (&o.h8.a)[j] = res;
  }
  return o.i4;
}

DEVINL float sumsq8(const int4& xp, float ss) {
#pragma clang fp contract(off)
  Pack16B p;
  p.i4 = xp;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    bf16x2 h = (&p.h8.a)[j];
    float lo = bf2f(h.x), hi = bf2f(h.y);
    ss = ss + fmaf(lo, lo, hi * hi);
  }
  return ss;
}

DEVINL int4 scale8(const int4& xp, const int4& xw, float r) {
#pragma clang fp contract(off)
  Pack16B p, pw, o;
  p.i4 = xp;
  pw.i4 = xw;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    bf16x2 h = (&p.h8.a)[j], hw = (&pw.h8.a)[j], res;
    res.x = f2bf(bf2f(h.x) * r * bf2f(hw.x));
    res.y = f2bf(bf2f(h.y) * r * bf2f(hw.y));
    (&o.h8.a)[j] = res;
  }
  return o.i4;
}

template <int NT, int VPT>
__global__ void add_rmsnorm_fwd_kernel(const bf16* __restrict__ x,
                                       const bf16* __restrict__ delta,
                                       const bf16* __restrict__ w,
                                       bf16* h, bf16* __restrict__ y,
                                       float* __restrict__ invrms, int H,
                                       float eps) {
#pragma clang fp contract(off)
  __shared__ float lds[NT / 64];
  const int row = blockIdx.x;
  const int4* xr = (const int4*)(x + (long)row * H);
  const int4* dr = (const int4*)(delta + (long)row * H);
  int4* hr = (int4*)(h + (long)row * H);
  int4* yr = (int4*)(y + (long)row * H);
  const int nvec = H >> 3;  // H % 8 == 0
  int4 hv[VPT > 0 ? VPT : 1];
  float ss = 0.f;
  if (VPT > 0) {
#pragma unroll
    for (int v = 0; v < VPT; ++v) {
      const int i = threadIdx.x + v * NT;
      if (i < nvec) {
        hv[v] = add8(xr[i], dr[i]);
        hr[i] = hv[v];
        ss = sumsq8(hv[v], ss);
      }
    }
  } else {
    for (int i = threadIdx.x; i < nvec; i += NT) {
      const int4 ph = add8(xr[i], dr[i]);
      hr[i] = ph;
      ss = sumsq8(ph, ss);
    }
  }
  ss = block_reduce_sum<NT>(ss, lds);
  float r = rsqrtf(ss / (float)H + eps);
  if (threadIdx.x == 0) invrms[row] = r;
  if (VPT > 0) {
#pragma unroll
    for (int v = 0; v < VPT; ++v) {
      const int i = threadIdx.x + v * NT;
      if (i < nvec) yr[i] = scale8(hv[v], ((const int4*)w)[i], r);
    }
  } else {
    // each thread reads back the vectors it stored itself
    for (int i = threadIdx.x; i < nvec; i += NT)
      yr[i] = scale8(hr[i], ((const int4*)w)[i], r);
  }
}

DEVINL float csum8(const int4& xd, const int4& xx, const int4& xw, float r,
                   float c) {
#pragma clang fp contract(off)
  Pack16B pd, px, pw;
  pd.i4 = xd;
  px.i4 = xx;
  pw.i4 = xw;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    bf16x2 hd = (&pd.h8.a)[j], hx = (&px.h8.a)[j], hw = (&pw.h8.a)[j];
    c = c + bf2f(hw.x) * bf2f(hd.x) * bf2f(hx.x) * r;
    c = c + bf2f(hw.y) * bf2f(hd.y) * bf2f(hx.y) * r;
  }
  return c;
}

// dx (+ dh) of one vector; adds the vector's dy * xhat into dw_lds[0 .. 8)
template <bool HAS_DH>
DEVINL int4 dx8(const int4& xd, const int4& xx, const int4& xw,
                const int4& xg, float r, float c, float* dw_lds) {
#pragma clang fp contract(off)
  Pack16B pd, px, pw, pg, o;
  pd.i4 = xd;
  px.i4 = xx;
  pw.i4 = xw;
  pg.i4 = xg;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    bf16x2 hd = (&pd.h8.a)[j], hx = (&px.h8.a)[j], hw = (&pw.h8.a)[j];
    float xh0 = bf2f(hx.x) * r, xh1 = bf2f(hx.y) * r;
    float d0 = bf2f(hd.x), d1 = bf2f(hd.y);
    bf16x2 res;
    res.x = f2bf(fmaf(d0, bf2f(hw.x), -(xh0 * c)) * r);
    res.y = f2bf(fmaf(d1, bf2f(hw.y), -(xh1 * c)) * r);
    if (HAS_DH) {
      bf16x2 hg = (&pg.h8.a)[j];
      res.x = f2bf(bf2f(hg.x) + bf2f(res.x));
      res.y = f2bf(bf2f(hg.y) + bf2f(res.y));
    }
    (&o.h8.a)[j] = res;
    dw_lds[2 * j] = fmaf(d0, xh0, dw_lds[2 * j]);
    dw_lds[2 * j + 1] = fmaf(d1, xh1, dw_lds[2 * j + 1]);
  }
  return o.i4;
}

// dx = bf16(dh + bf16(dxn)) with dxn the value rmsnorm_bwd_kernel stores; no
// add without dh. dy and h are read once (VPT > 0). dw as above: per-block
// LDS accumulation in fixed columns, one atomicAdd pass.
template <int NT, int VPT, bool HAS_DH>
__global__ void add_rmsnorm_bwd_kernel(const bf16* __restrict__ dy,
                                       const bf16* __restrict__ dh,
                                       const bf16* __restrict__ h,
                                       const bf16* __restrict__ w,
                                       const float* __restrict__ invrms,
                                       bf16* __restrict__ dx,
                                       float* __restrict__ dw /* zeroed */,
                                       int N, int H) {
#pragma clang fp contract(off)
  extern __shared__ float smem[];          // [H] dw accum + [NT/64] reduce
  float* dw_lds = smem;
  float* red = smem + H;
  for (int i = threadIdx.x; i < H; i += NT) dw_lds[i] = 0.f;
  __syncthreads();

  const int nvec = H >> 3;
  for (int row = blockIdx.x; row < N; row += gridDim.x) {
    const int4* dyr = (const int4*)(dy + (long)row * H);
    const int4* xr = (const int4*)(h + (long)row * H);
    const int4* dhr = (const int4*)(dh + (HAS_DH ? (long)row * H : 0));
    int4* dxr = (int4*)(dx + (long)row * H);
    const float r = invrms[row];
    const int4* wv = (const int4*)w;
    int4 vd[VPT > 0 ? VPT : 1], vx[VPT > 0 ? VPT : 1];
    float c = 0.f;
    if (VPT > 0) {
#pragma unroll
      for (int v = 0; v < VPT; ++v) {
        const int i = threadIdx.x + v * NT;
        if (i < nvec) {
          vd[v] = dyr[i];
          vx[v] = xr[i];
          c = csum8(vd[v], vx[v], wv[i], r, c);
        }
      }
    } else {
      for (int i = threadIdx.x; i < nvec; i += NT)
        c = csum8(dyr[i], xr[i], wv[i], r, c);
    }
    c = block_reduce_sum<NT>(c, red) / (float)H;
    // without dh, dhr is dy's row and dx8 ignores it
    if (VPT > 0) {
#pragma unroll
      for (int v = 0; v < VPT; ++v) {
        const int i = threadIdx.x + v * NT;
        if (i < nvec)
          dxr[i] = dx8<HAS_DH>(vd[v], vx[v], wv[i], HAS_DH ? dhr[i] : vd[v],
                               r, c, dw_lds + (i << 3));
      }
    } else {
      for (int i = threadIdx.x; i < nvec; i += NT) {
        const int4 pd = dyr[i];
        dxr[i] = dx8<HAS_DH>(pd, xr[i], wv[i], HAS_DH ? dhr[i] : pd, r, c,
                             dw_lds + (i << 3));
      }
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < H; i += NT) atomicAdd(&dw[i], dw_lds[i]);
}

// vectors per thread held in registers for a row of H elements; 0 = looped
static int add_rmsnorm_vpt(int H, int NT) {
  const int nvec = H >> 3;
  return nvec <= 2 * NT ? 2 : nvec <= 4 * NT ? 4 : 0;
}

template <int NT, int VPT>
static void add_rmsnorm_bwd_launch(const void* dy, const void* dh,
                                   const void* h, const void* w,
                                   const void* invrms, void* dx, void* dw,
                                   long N, int H, hipStream_t stream) {
  int blocks = (int)min((long)1024, N);
  size_t shmem = (H + NT / 64) * sizeof(float);
  if (dh)
    add_rmsnorm_bwd_kernel<NT, VPT, true>
        <<<dim3(blocks), dim3(NT), shmem, stream>>>(
            (const bf16*)dy, (const bf16*)dh, (const bf16*)h, (const bf16*)w,
            (const float*)invrms, (bf16*)dx, (float*)dw, (int)N, H);
  else
    add_rmsnorm_bwd_kernel<NT, VPT, false>
        <<<dim3(blocks), dim3(NT), shmem, stream>>>(
            (const bf16*)dy, (const bf16*)dy, (const bf16*)h, (const bf16*)w,
            (const float*)invrms, (bf16*)dx, (float*)dw, (int)N, H);
  HIP_CHECK_LAST();
}

extern "C" {
void launch_add_rmsnorm_fwd(const void* x, const void* delta, const void* w,
                            void* h, void* y, void* invrms, long N, int H,
                            float eps, hipStream_t stream) {
  constexpr int NT = 256;
  if (N <= 0) return;
  const bf16 *xp = (const bf16*)x, *dp = (const bf16*)delta,
             *wp = (const bf16*)w;
  const dim3 grid((unsigned)N), block(NT);
  switch (add_rmsnorm_vpt(H, NT)) {
    case 2:
      add_rmsnorm_fwd_kernel<NT, 2><<<grid, block, 0, stream>>>(
          xp, dp, wp, (bf16*)h, (bf16*)y, (float*)invrms, H, eps);
      break;
    case 4:
      add_rmsnorm_fwd_kernel<NT, 4><<<grid, block, 0, stream>>>(
          xp, dp, wp, (bf16*)h, (bf16*)y, (float*)invrms, H, eps);
      break;
    default:
      add_rmsnorm_fwd_kernel<NT, 0><<<grid, block, 0, stream>>>(
          xp, dp, wp, (bf16*)h, (bf16*)y, (float*)invrms, H, eps);
  }
  HIP_CHECK_LAST();
}

void launch_add_rmsnorm_bwd(const void* dy, const void* dh, const void* h,
                            const void* w, const void* invrms, void* dx,
                            void* dw, long N, int H, hipStream_t stream) {
  constexpr int NT = 256;
  if (N <= 0) return;
  switch (add_rmsnorm_vpt(H, NT)) {
    case 2:
      add_rmsnorm_bwd_launch<NT, 2>(dy, dh, h, w, invrms, dx, dw, N, H, stream);
      break;
    case 4:
      add_rmsnorm_bwd_launch<NT, 4>(dy, dh, h, w, invrms, dx, dw, N, H, stream);
      break;
    default:
      add_rmsnorm_bwd_launch<NT, 0>(dy, dh, h, w, invrms, dx, dw, N, H, stream);
  }
}

void launch_rmsnorm_fwd(const void* x, const void* w, void* y, void* invrms,
                        long N, int H, float eps, hipStream_t stream) {
  constexpr int NT = 256;
  if (N <= 0) return;  // a grid of zero blocks is an invalid launch
  rmsnorm_fwd_kernel<NT><<<dim3((unsigned)N), dim3(NT), 0, stream>>>(
      (const bf16*)x, (const bf16*)w, (bf16*)y, (float*)invrms, H, eps);
  HIP_CHECK_LAST();
}

void launch_rmsnorm_bwd(const void* dy, const void* x, const void* w,
                        const void* invrms, void* dx, void* dw, long N, int H,
                        hipStream_t stream) {
  constexpr int NT = 256;
  if (N <= 0) return;
  int blocks = (int)min((long)1024, N);
  size_t shmem = (H + NT / 64) * sizeof(float);
  rmsnorm_bwd_kernel<NT><<<dim3(blocks), dim3(NT), shmem, stream>>>(
      (const bf16*)dy, (const bf16*)x, (const bf16*)w, (const float*)invrms,
      (bf16*)dx, (float*)dw, (int)N, H);
  HIP_CHECK_LAST();
}
}
