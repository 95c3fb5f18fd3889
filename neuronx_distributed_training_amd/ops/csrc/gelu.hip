// Exact (erf) GELU and GEGLU, forward and backward, one HBM pass each.
//   gelu(x)  = x * Phi(x),  Phi(x) = (1 + erf(x / sqrt 2)) / 2
//   gelu'(x) = Phi(x) + x * phi(x),  phi(x) = exp(-x^2 / 2) / sqrt(2 pi)
// bf16 IO in 16-byte vectors, fp32 arithmetic, grid-stride. GEGLU reads
// gate_up packed [N, 2I] = [gate | up] (the fused ColumnParallel output) and
// splits it in the kernel; y = bf16(bf16(gelu(gate)) * up), the two rounding
// points of F.gelu(gate) * up on bf16 tensors; its backward writes
// [dgate | dup] in place of a concatenation.
#include "common.h"
#include "launch.h"

namespace {

DEVINL float phi_cdf(float x) { return 0.5f * (1.f + erff(x * 0.70710678f)); }
DEVINL float gelu_f(float x) { return x * phi_cdf(x); }
DEVINL float dgelu_f(float x) {
  return phi_cdf(x) + x * (0.39894228f * expf(-0.5f * x * x));
}

// 8 bf16 of one vector as fp32
struct F8 {
  float f[8];
};
DEVINL F8 load8(const bf16* p, long vec) {
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
DEVINL void store8(bf16* p, long vec, const F8& v) {
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

// total = number of 16-byte vectors of x
__global__ void gelu_fwd_kernel(const bf16* __restrict__ x,
                                bf16* __restrict__ y, long total) {
  for (long idx = blockIdx.x * (long)blockDim.x + threadIdx.x; idx < total;
       idx += (long)gridDim.x * blockDim.x) {
    F8 v = load8(x, idx);
#pragma unroll
    for (int j = 0; j < 8; ++j) v.f[j] = gelu_f(v.f[j]);
    store8(y, idx, v);
  }
}

__global__ void gelu_bwd_kernel(const bf16* __restrict__ dy,
                                const bf16* __restrict__ x,
                                bf16* __restrict__ dx, long total) {
  for (long idx = blockIdx.x * (long)blockDim.x + threadIdx.x; idx < total;
       idx += (long)gridDim.x * blockDim.x) {
    F8 v = load8(x, idx);
    const F8 d = load8(dy, idx);
#pragma unroll
    for (int j = 0; j < 8; ++j) v.f[j] = d.f[j] * dgelu_f(v.f[j]);
    store8(dx, idx, v);
  }
}

__global__ void geglu_fwd_kernel(const bf16* __restrict__ gu,
                                 bf16* __restrict__ y, long N, int I) {
  const int nvec = I >> 3;
  const long total = N * (long)nvec;
  for (long idx = blockIdx.x * (long)blockDim.x + threadIdx.x; idx < total;
       idx += (long)gridDim.x * blockDim.x) {
    const long row = idx / nvec;
    const int i = (int)(idx % nvec);
    const bf16* g = gu + row * 2 * (long)I;
    F8 v = load8(g, i);
    const F8 u = load8(g + I, i);
#pragma unroll
    for (int j = 0; j < 8; ++j) v.f[j] = bf2f(f2bf(gelu_f(v.f[j]))) * u.f[j];
    store8(y + row * (long)I, i, v);
  }
}

__global__ void geglu_bwd_kernel(const bf16* __restrict__ dy,
                                 const bf16* __restrict__ gu,
                                 bf16* __restrict__ dgu, long N, int I) {
  const int nvec = I >> 3;
  const long total = N * (long)nvec;
  for (long idx = blockIdx.x * (long)blockDim.x + threadIdx.x; idx < total;
       idx += (long)gridDim.x * blockDim.x) {
    const long row = idx / nvec;
    const int i = (int)(idx % nvec);
    const bf16* g = gu + row * 2 * (long)I;
    bf16* dg = dgu + row * 2 * (long)I;
    const F8 vg = load8(g, i), vu = load8(g + I, i);
    const F8 d = load8(dy + row * (long)I, i);
    F8 og, ou;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      og.f[j] = d.f[j] * vu.f[j] * dgelu_f(vg.f[j]);
      ou.f[j] = d.f[j] * gelu_f(vg.f[j]);
    }
    store8(dg, i, og);
    store8(dg + I, i, ou);
  }
}

int blocks_for(long total) {
  return (int)min((total + 255) / 256, (long)8192);
}

}  // namespace

extern "C" {
void launch_gelu_fwd(const void* x, void* y, long n, hipStream_t stream) {
  const long total = n >> 3;
  if (total <= 0) return;  // a grid of zero blocks is an invalid launch
  gelu_fwd_kernel<<<dim3(blocks_for(total)), dim3(256), 0, stream>>>(
      (const bf16*)x, (bf16*)y, total);
  HIP_CHECK_LAST();
}
void launch_gelu_bwd(const void* dy, const void* x, void* dx, long n,
                     hipStream_t stream) {
  const long total = n >> 3;
  if (total <= 0) return;
  gelu_bwd_kernel<<<dim3(blocks_for(total)), dim3(256), 0, stream>>>(
      (const bf16*)dy, (const bf16*)x, (bf16*)dx, total);
  HIP_CHECK_LAST();
}
void launch_geglu_fwd(const void* gu, void* y, long N, int I,
                      hipStream_t stream) {
  const long total = N * (long)(I >> 3);
  if (total <= 0) return;
  geglu_fwd_kernel<<<dim3(blocks_for(total)), dim3(256), 0, stream>>>(
      (const bf16*)gu, (bf16*)y, N, I);
  HIP_CHECK_LAST();
}
void launch_geglu_bwd(const void* dy, const void* gu, void* dgu, long N,
                      int I, hipStream_t stream) {
  const long total = N * (long)(I >> 3);
  if (total <= 0) return;
  geglu_bwd_kernel<<<dim3(blocks_for(total)), dim3(256), 0, stream>>>(
      (const bf16*)dy, (const bf16*)gu, (bf16*)dgu, N, I);
  HIP_CHECK_LAST();
}
}
