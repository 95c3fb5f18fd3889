// Rotary position embedding (rotate-half), strided input → contiguous
// [s, b, h, d] output. Input is typically a non-contiguous [b, h, s, d]
// view of the fused QKV GEMM output — the kernel reads it in place, so the
// attention path does zero permute/contiguous copies.
// cos/sin tables [Smax, D] fp32; backward = forward with -sin (orthogonal).
#include <cstdint>

#include "common.h"
#include "launch.h"

__global__ void rope_fwd_kernel(const bf16* __restrict__ x,
                                const float* __restrict__ cost,
                                const float* __restrict__ sint,
                                bf16* __restrict__ y, int S, int B, int H,
                                int D, long sxs, long sxb, long sxh,
                                int pos_offset, int pos_offset2,
                                float sin_sign) {
  // pos_offset2 >= 0: zigzag context-parallel layout — rows [S/2, S) are
  // the rank's SECOND global chunk and take positions pos_offset2 + i
  const int half = D >> 1;
  const int shalf = S >> 1;
  const long total = (long)S * B * H * half;
  for (long idx = blockIdx.x * (long)blockDim.x + threadIdx.x; idx < total;
       idx += (long)gridDim.x * blockDim.x) {
    const int d = (int)(idx % half);
    const long row = idx / half;  // output row in [s][b][h] order
    const int h = (int)(row % H);
    const int b = (int)((row / H) % B);
    const int s = (int)(row / ((long)H * B));
    const bf16* xr = x + s * sxs + b * sxb + h * sxh;
    bf16* yr = y + row * D;
    const int p = (pos_offset2 >= 0 && s >= shalf)
                      ? (s - shalf) + pos_offset2
                      : s + pos_offset;
    const float c0 = cost[(long)p * D + d];
    const float s0 = sint[(long)p * D + d] * sin_sign;
    const float c1 = cost[(long)p * D + d + half];
    const float s1 = sint[(long)p * D + d + half] * sin_sign;
    const float x0 = bf2f(xr[d]);
    const float x1 = bf2f(xr[d + half]);
    yr[d] = f2bf(x0 * c0 - x1 * s0);
    yr[d + half] = f2bf(x1 * c1 + x0 * s1);
  }
}

// ---------------- Q and K in one launch, 16-byte accesses ----------------
// One grid over the HQ + HKV head rows of every (s, b). A thread owns the
// column pair [8 l, 8 l + 8) and [D/2 + 8 l, D/2 + 8 l + 8) (l < D / 16) of
// ROPE_PAIR_HEADS consecutive head rows: it reads its 32 table values of the
// position once and then moves one 16 B vector per half and head row.
// Needs D % 16 == 0, 16 B-aligned bases and strides that are multiples of 8;
// 32-bit index arithmetic except for the final element offsets.
// The products are fused as the compiler fused them in rope_fwd_kernel (read
// from its ISA), so the results are bit-equal to it:
//   y0 = fma(x0, c0, -(x1 * s0)),  y1 = fma(x0, s1, x1 * c1).
constexpr int ROPE_PAIR_HEADS = 8;

struct RopePairArgs {
  const bf16 *q, *k;
  bf16 *yq, *yk;
  const float *cost, *sint;
  int S, B, HQ, HKV, D;
  long qs[3], ks[3];  // (seq, batch, head) strides, elements
  int pos_offset, pos_offset2;
  float sin_sign;
  int lanes, chunks, total;  // D / 16, head chunks per (s, b), threads
};

DEVINL void load8f(const float* p, float (&v)[8]) {
  const float4 a = ((const float4*)p)[0], b = ((const float4*)p)[1];
  v[0] = a.x, v[1] = a.y, v[2] = a.z, v[3] = a.w;
  v[4] = b.x, v[5] = b.y, v[6] = b.z, v[7] = b.w;
}

__global__ void rope_pair_kernel(const RopePairArgs a) {
#pragma clang fp contract(off)
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= a.total) return;
  const int l = t % a.lanes;
  const int u = t / a.lanes;
  const int chunk = u % a.chunks;
  const int sb = u / a.chunks;  // s * B + b
  const int b = sb % a.B;
  const int s = sb / a.B;
  const int half = a.D >> 1;
  const int shalf = a.S >> 1;
  const int p = (a.pos_offset2 >= 0 && s >= shalf)
                    ? (s - shalf) + a.pos_offset2
                    : s + a.pos_offset;
  float c0[8], c1[8], s0[8], s1[8];
  const long trow = (long)p * a.D + (l << 3);
  load8f(a.cost + trow, c0);
  load8f(a.cost + trow + half, c1);
  load8f(a.sint + trow, s0);
  load8f(a.sint + trow + half, s1);
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    s0[j] = s0[j] * a.sin_sign;
    s1[j] = s1[j] * a.sin_sign;
  }
  const int HT = a.HQ + a.HKV;
  const int g0 = chunk * ROPE_PAIR_HEADS;
  const int g1 = min(g0 + ROPE_PAIR_HEADS, HT);
  const long qrow = s * a.qs[0] + b * a.qs[1];
  const long krow = s * a.ks[0] + b * a.ks[1];
#pragma unroll 4
  for (int g = g0; g < g1; ++g) {
    const bool isq = g < a.HQ;
    const int hd = isq ? g : g - a.HQ;
    const bf16* xr = isq ? a.q + qrow + hd * a.qs[2]
                         : a.k + krow + hd * a.ks[2];
    bf16* yr = isq ? a.yq + ((long)sb * a.HQ + hd) * a.D
                   : a.yk + ((long)sb * a.HKV + hd) * a.D;
    Pack16B lo, hi, olo, ohi;
    lo.i4 = *(const int4*)(xr + (l << 3));
    hi.i4 = *(const int4*)(xr + half + (l << 3));
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const bf16x2 h0 = (&lo.h8.a)[j], h1 = (&hi.h8.a)[j];
      const float x0a = bf2f(h0.x), x0b = bf2f(h0.y);
      const float x1a = bf2f(h1.x), x1b = bf2f(h1.y);
      bf16x2 r0, r1;
      r0.x = f2bf(fmaf(x0a, c0[2 * j], -(x1a * s0[2 * j])));
      r0.y = f2bf(fmaf(x0b, c0[2 * j + 1], -(x1b * s0[2 * j + 1])));
      r1.x = f2bf(fmaf(x0a, s1[2 * j], x1a * c1[2 * j]));
      r1.y = f2bf(fmaf(x0b, s1[2 * j + 1], x1b * c1[2 * j + 1]));
      (&olo.h8.a)[j] = r0;
      (&ohi.h8.a)[j] = r1;
    }
    *(int4*)(yr + (l << 3)) = olo.i4;
    *(int4*)(yr + half + (l << 3)) = ohi.i4;
  }
}

static bool rope_pair_vec_ok(const void* q, const void* k, const void* cost,
                             const void* sint, long S, long B, long HT, int D,
                             const long* qstr, const long* kstr) {
  if (D % 16 != 0) return false;
  for (const void* p : {q, k, cost, sint})
    if ((uintptr_t)p % 16 != 0) return false;
  for (int i = 0; i < 3; ++i)
    if (qstr[i] % 8 != 0 || kstr[i] % 8 != 0) return false;
  // thread index and s * B + b in 32 bits
  const long chunks = (HT + ROPE_PAIR_HEADS - 1) / ROPE_PAIR_HEADS;
  return S * B * chunks * (D / 16) < (1L << 31) - 256;
}

extern "C" {
void launch_rope_fwd_pair(const void* q, const void* k, const void* cost,
                          const void* sint, void* yq, void* yk, int S, int B,
                          int HQ, int HKV, int D, const long* qstr,
                          const long* kstr, int pos_offset, int pos_offset2,
                          float sin_sign, hipStream_t stream) {
  if ((long)S * B * (HQ + HKV) * D <= 0) return;
  if (!rope_pair_vec_ok(q, k, cost, sint, S, B, HQ + HKV, D, qstr, kstr)) {
    // the scalar kernel, once per tensor (it returns at an empty one)
    launch_rope_fwd(q, cost, sint, yq, S, B, HQ, D, qstr, pos_offset,
                    pos_offset2, sin_sign, stream);
    launch_rope_fwd(k, cost, sint, yk, S, B, HKV, D, kstr, pos_offset,
                    pos_offset2, sin_sign, stream);
    return;
  }
  RopePairArgs a;
  a.q = (const bf16*)q, a.k = (const bf16*)k;
  a.yq = (bf16*)yq, a.yk = (bf16*)yk;
  a.cost = (const float*)cost, a.sint = (const float*)sint;
  a.S = S, a.B = B, a.HQ = HQ, a.HKV = HKV, a.D = D;
  for (int i = 0; i < 3; ++i) a.qs[i] = qstr[i], a.ks[i] = kstr[i];
  a.pos_offset = pos_offset, a.pos_offset2 = pos_offset2;
  a.sin_sign = sin_sign;
  a.lanes = D / 16;
  a.chunks = (HQ + HKV + ROPE_PAIR_HEADS - 1) / ROPE_PAIR_HEADS;
  a.total = S * B * a.chunks * a.lanes;
  rope_pair_kernel<<<dim3((a.total + 255) / 256), dim3(256), 0, stream>>>(a);
  HIP_CHECK_LAST();
}

void launch_rope_fwd(const void* x, const void* cost, const void* sint,
                     void* y, int S, int B, int H, int D, const long* xstr,
                     int pos_offset, int pos_offset2, float sin_sign,
                     hipStream_t stream) {
  long total = (long)S * B * H * (D >> 1);
  if (total <= 0) return;  // a grid of zero blocks is an invalid launch
  int blocks = (int)min((total + 255) / 256, (long)16384);
  rope_fwd_kernel<<<dim3(blocks), dim3(256), 0, stream>>>(
      (const bf16*)x, (const float*)cost, (const float*)sint, (bf16*)y, S, B,
      H, D, xstr[0], xstr[1], xstr[2], pos_offset, pos_offset2, sin_sign);
  HIP_CHECK_LAST();
}
}
