// Host-side launch ABI of every HIP kernel file: the ONLY declaration of each
// launch_* function. bindings.cpp and every .hip file that defines a launcher
// include it, so each definition is compiled against its declaration and a
// parameter that differs between the two is a compile error (the functions
// have C linkage: there is no overloading to hide it).
#pragma once

#include <hip/hip_runtime.h>

// ---- flash attention: argument block and tiling rule ----

// Tensors are logical [b, h, s, d] bf16 with d contiguous; a stride triple is
// in (seq, batch, head) order, in elements. O and dQ are contiguous
// [s, b, hq, d]; LSE and delta are dense [B, HQ, SQ] fp32; dK / dV are fp32
// partial slabs [HQ / HKV, s, b, hkv, d] that the binding sums. The backward
// fields stay null in a forward call.
struct FlashArgs {
  // DENSE: bound_a / bound_b unused. RANGED: per-batch-row visible key range
  // [bound_a[b], bound_b[b]), int32 [B], 0 <= lo <= hi <= SKV. SEGMENTED:
  // packed sequences, always causal, SQ == SKV; bound_a = q_start and
  // bound_b = k_end, int32 [B, S], non-decreasing along each row with
  // 0 <= q_start[b,i] <= i < k_end[b,i] <= S.
  enum Mask { DENSE, RANGED, SEGMENTED };

  const void *q, *k, *v;
  void *o, *lse;  // lse: written by the forward, read by the backward
  const void *dout, *delta;
  void *dq, *dk, *dv;
  int B, HQ, HKV, SQ, SKV, D;
  bool causal;
  float scale;
  int window;  // sliding window (<= 0: disabled)
  long qs[3], ks[3], vs[3], ds[3];  // q, k, v, dout strides
  Mask mask;
  const int *bound_a, *bound_b;
  // Attention dropout (attn_dropout.h), DENSE only: drop_t = round(256 * p)
  // in 1..255 selects the DROPOUT instantiations of the double-buffered
  // forward, the dQ kernel and the pipelined dK/dV kernel; 0 = no dropout
  // (every other call). (drop_seed, drop_offset) name the random stream.
  int drop_t;
  unsigned long long drop_seed, drop_offset;
};

// Query rows per block of the forward and dQ grids: 128 when the 256-row grid
// would leave CUs idle (TP=8: HQ_local=4), else 256.
constexpr int flash_block_rows(int SQ, int BH) {
  return (long)((SQ + 255) / 256) * BH < 512 ? 128 : 256;
}
static_assert(flash_block_rows(300, 256) == 256, "512 blocks: 256-row tiles");
static_assert(flash_block_rows(256, 511) == 128, "511 blocks: 128-row tiles");
static_assert(flash_block_rows(300, 255) == 128, "510 blocks: 128-row tiles");

extern "C" {
// flash_attn_fwd.hip: single-buffered forward (A/B arm), DENSE only
void launch_flash_fwd(const FlashArgs& a, hipStream_t stream);
// flash_attn_fwd_dbuf.hip: double-buffered forward (default), every mask,
// dropout
void launch_flash_fwd_dbuf(const FlashArgs& a, hipStream_t stream);
// flash_attn_bwd.hip: dK/dV, then dQ. pipe = true: dK/dV by the pipelined
// kernel (default); false: by flash_bwd_dkv_kernel (A/B arm, bit-equal).
// A dropout call (drop_t > 0) always takes the pipelined kernel.
void launch_flash_bwd(const FlashArgs& a, bool pipe, hipStream_t stream);
// flash_attn_bwd_dkv_pipe.hip: dK/dV only; called by launch_flash_bwd
void launch_flash_dkv_pipe(const FlashArgs& a, hipStream_t stream);
// v3 kernels: DENSE only, SQ == SKV
void launch_flash_fwd_v3(const FlashArgs& a, hipStream_t stream);
void launch_flash_bwd_v3(const FlashArgs& a, hipStream_t stream);
// attn_dropout.hip: keep mask [B, HQ, SQ, SKV] uint8 (1 = keep), the mask the
// DROPOUT kernels regenerate; test and debug support
void launch_attn_dropout_mask(void* mask, int B, int HQ, int SQ, int SKV,
                              int drop_t, unsigned long long seed,
                              unsigned long long offset, hipStream_t stream);
void launch_attn_delta(const void* dout, const void* o, void* delta, int SQ,
                       int B, int HQ, int D, const long* dstr,
                       const long* ostr, hipStream_t stream);

void launch_rmsnorm_fwd(const void* x, const void* w, void* y, void* invrms,
                        long N, int H, float eps, hipStream_t stream);
void launch_rmsnorm_bwd(const void* dy, const void* x, const void* w,
                        const void* invrms, void* dx, void* dw, long N, int H,
                        hipStream_t stream);
void launch_swiglu_fwd(const void* gu, void* y, long N, int I,
                       hipStream_t stream);
void launch_swiglu_bwd(const void* dy, const void* gu, void* dgu, long N,
                       int I, hipStream_t stream);
void launch_rope_fwd(const void* x, const void* cost, const void* sint,
                     void* y, int S, int B, int H, int D, const long* xstr,
                     int pos_offset, int pos_offset2, float sin_sign,
                     hipStream_t stream);
void launch_adamw(void* p, const void* g, void* m, void* v,
                  const void* wd_mask, const void* grad_scale, void* p_bf16,
                  long n, float lr, float beta1, float beta2, float eps,
                  float wd, int step, hipStream_t stream);
void launch_ce_fwd(const void* logits, const void* targets, void* row_max,
                   void* row_sumexp, void* tgt_logit, long N, int V,
                   long vocab_start, hipStream_t stream);
void launch_ce_bwd(const void* logits, const void* targets, const void* gmax,
                   const void* gsum, const void* gout, void* dlogits, long N,
                   int V, long vocab_start, hipStream_t stream);
void launch_moe_gemm(const void* a, const void* w, void* c,
                     const int* tile_expert, const int* total_rows,
                     int row_tiles, int K, int Nc, long wstride, bool trans_b,
                     hipStream_t stream);
void launch_moe_wgrad(const void* dy, const void* x, void* dw,
                      const int* seg_start, int E, int N, int K,
                      hipStream_t stream);
void launch_mfma_probe(const void* a, const void* b, void* c,
                       hipStream_t stream);
void launch_mfma_probe32(const void* a, const void* b, void* c,
                         hipStream_t stream);
}
