// The attention-dropout keep mask as a tensor: test and debug support, on no
// hot path. One thread per element calls dropout_keep (attn_dropout.h), the
// definition the DROPOUT instantiations of the attention kernels regenerate
// on their own footprint, so a comparison against this mask proves that they
// agree with it and with one another.
#include "attn_dropout.h"
#include "launch.h"

__global__ __launch_bounds__(256) void attn_dropout_mask_kernel(
    unsigned char* __restrict__ mask,  // [B, HQ, SQ, SKV], 1 = keep
    int HQ, int SQ, int SKV, long total, int drop_t, unsigned long long seed,
    unsigned long long offset) {
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  if (e >= total) return;
  const int j = (int)(e % SKV);
  const int i = (int)((e / SKV) % SQ);
  const long bh = e / ((long)SKV * SQ);
  const int hq = (int)(bh % HQ);
  const int b = (int)(bh / HQ);
  mask[e] = dropout_keep(seed, offset, b, hq, HQ, i, j, drop_t) ? 1 : 0;
}

extern "C" void launch_attn_dropout_mask(void* mask, int B, int HQ, int SQ,
                                         int SKV, int drop_t,
                                         unsigned long long seed,
                                         unsigned long long offset,
                                         hipStream_t stream) {
  const long total = (long)B * HQ * SQ * SKV;
  if (total == 0) return;
  const dim3 grid((unsigned)((total + 255) / 256)), blk(256);
  attn_dropout_mask_kernel<<<grid, blk, 0, stream>>>(
      (unsigned char*)mask, HQ, SQ, SKV, total, drop_t, seed, offset);
}
