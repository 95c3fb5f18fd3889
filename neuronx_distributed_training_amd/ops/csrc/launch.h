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
  // forward (the pipe forward has none and hands such calls to it), the dQ
  // kernel and the pipelined dK/dV kernel; 0 = no dropout
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

// ---- flash decode: argument block and split rule ----

// q is logical [B, HQ, SQ, D] bf16; k / v are the preallocated cache buffers,
// logical [B, HKV, CAP, D] bf16; d contiguous, stride triples in (seq, batch,
// head) order as in FlashArgs. Row b sees keys kv_lo[b] <= j < kv_hi[b]
// (device int32 [B]; the kernel clamps them to [0, max_kv]), bottom-right
// causal: query i sits at position kv_hi[b] - SQ + i. The grid covers keys
// [0, max_kv), max_kv <= CAP. o_part / lse_part are fp32 scratch
// [num_splits, B, HQ, SQ, D] / [num_splits, B, HQ, SQ]; o is bf16
// [B, HQ, SQ, D] and lse fp32 [B, HQ, SQ], both dense.
struct FlashDecodeArgs {
  const void *q, *k, *v;
  void *o, *lse, *o_part, *lse_part;
  const int *kv_lo, *kv_hi;
  int B, HQ, HKV, SQ, D;
  int max_kv, num_splits;
  float scale;
  int window;  // sliding window (<= 0: disabled)
  long qs[3], ks[3], vs[3];
};

// Key splits of a decode call, from host values only (never the device
// lengths: no sync): enough (split, kv head, batch row) blocks for two per
// CU, at least two 64-key tiles per split, at most 64 splits.
constexpr int flash_decode_splits(int B, int HKV, int max_kv, int num_cu) {
  const long base = (long)B * HKV;
  const long want = (2L * num_cu + base - 1) / base;
  const long tiles = (max_kv + 63) / 64;
  const long cap = tiles / 2 < 64 ? tiles / 2 : 64;
  return (int)(want < cap ? (want < 1 ? 1 : want) : (cap < 1 ? 1 : cap));
}
static_assert(flash_decode_splits(1, 8, 8192, 256) == 64, "long, batch 1");
static_assert(flash_decode_splits(8, 8, 512, 256) == 4, "tile-bound");
static_assert(flash_decode_splits(64, 8, 4096, 256) == 1, "grid already full");
static_assert(flash_decode_splits(1, 1, 1, 256) == 1, "one key");

// ---- LoRA adapter products (lora.hip) ----

// Rows of T that one block of the wgrad kernel contracts; the second stage
// sums the ceil(T / chunk) fp32 partial slabs in chunk order.
constexpr int LORA_WGRAD_CHUNK = 256;
constexpr int lora_wgrad_chunks(long T) {
  return (int)((T + LORA_WGRAD_CHUNK - 1) / LORA_WGRAD_CHUNK);
}
static_assert(lora_wgrad_chunks(0) == 0 && lora_wgrad_chunks(257) == 2,
              "no rows: no partial; a ragged last chunk counts");

// ---- fused LM-head + cross-entropy (lm_head_loss.hip) ----

// Token rows and vocab columns of one block's logits tile, and the step of
// its K loop over H.
constexpr int LMHEAD_BM = 128, LMHEAD_BN = 128, LMHEAD_BK = 64;
constexpr long lmhead_tiles(long n, int tile) { return (n + tile - 1) / tile; }
constexpr int lmhead_vtiles(long V) { return (int)lmhead_tiles(V, LMHEAD_BN); }
static_assert(lmhead_vtiles(128) == 1 && lmhead_vtiles(136) == 2,
              "one 8-column group past a tile is a tile of its own");

// ---- LayerNorm (layernorm.hip) ----

// How a row of H elements (H % 8 == 0) is held. LN_WAVE: H <= 2048, one
// 64-lane wave per row, layernorm_vecs(H) 16-byte vectors per lane.
// LN_BLOCK: H <= 8192, a 256-thread block per row, that many vectors per
// thread. LN_LOOPED: longer rows, read twice (layernorm_vecs == 0).
enum LayerNormForm { LN_WAVE, LN_BLOCK, LN_LOOPED };
constexpr LayerNormForm layernorm_form(int H) {
  return H <= 2048 ? LN_WAVE : H <= 8192 ? LN_BLOCK : LN_LOOPED;
}
constexpr int layernorm_vecs(int H) {
  const int nvec = H >> 3;
  return nvec <= 64 ? 1 : nvec <= 128 ? 2 : nvec <= 256 ? 4
         : nvec <= 512 ? 2 : nvec <= 1024 ? 4 : 0;
}
static_assert(layernorm_form(2048) == LN_WAVE && layernorm_vecs(2048) == 4 &&
                  layernorm_vecs(1032) == 4 && layernorm_vecs(8) == 1,
              "wave form: up to 4 vectors a lane, 3 rounded up");
static_assert(layernorm_form(2056) == LN_BLOCK && layernorm_vecs(2056) == 2 &&
                  layernorm_vecs(8192) == 4 && layernorm_vecs(8200) == 0,
              "block form up to 8192, looped beyond");
// Blocks of the backward, each of which writes one fp32 partial [2, H] of
// (dw, db): two per CU, fewer when the rows run out (a wave-form block takes
// 4 rows at a time).
constexpr int layernorm_bwd_grid(long N, int H, int num_cu) {
  const long want = layernorm_form(H) == LN_WAVE ? (N + 3) / 4 : N;
  const long cap = 2L * num_cu;
  return (int)(want < cap ? want : cap);
}
static_assert(layernorm_bwd_grid(3, 1032, 256) == 1 &&
                  layernorm_bwd_grid(1500, 256, 256) == 375 &&
                  layernorm_bwd_grid(16384, 2048, 256) == 512 &&
                  layernorm_bwd_grid(9, 4096, 256) == 9,
              "rows bound the grid before the CUs do");

// ---- MoE token path (moe_dispatch.hip) ----

// Consecutive (token, choice) pairs per block of the plan's histogram and
// placement kernels; most experts (one wave lane each) and choices per token.
constexpr int MOE_PLAN_CHUNK = 1024, MOE_PLAN_MAX_E = 64, MOE_MAX_TOPK = 8;
constexpr int moe_plan_chunks(long P) {
  return (int)((P + MOE_PLAN_CHUNK - 1) / MOE_PLAN_CHUNK);
}
// Rows of the padded layout for P pairs over E experts, from host values
// only: every segment rounded up to 256 rows (ops/moe_gemm.py _layout).
constexpr long moe_padded_rows(long P, int E) {
  return (P + E * 255L + 255) / 256 * 256;
}
static_assert(moe_plan_chunks(0) == 0 && moe_plan_chunks(1025) == 2 &&
                  moe_padded_rows(600, 4) == 1792 && moe_padded_rows(0, 1) == 256,
              "a ragged last chunk counts; _layout's Tp_max");
// Adjacent lanes that hold one row of H bf16 in the permute / combine
// kernels (256 / lanes rows per block).
constexpr int moe_row_lanes(int H) { return H <= 512 ? 16 : H <= 2048 ? 64 : 256; }
static_assert(moe_row_lanes(128) == 16 && moe_row_lanes(640) == 64 &&
                  moe_row_lanes(4096) == 256,
              "one 16-byte vector a lane at H = 128; a block a row from 2176");
// The plan's tensors as the row kernels read them. Padded row r is valid when
// r < total[0] and r - pad_off[e] < counts[e] with e = tile_expert[r / 256];
// row_src[r] is then its pair index.
struct MoePlan {
  const int *row_src, *tile_expert, *pad_off, *total;
  const long* counts;
};

extern "C" {
// moe_dispatch.hip. plan: topi int64 [P] -> counts int64 [E], pad_off int32
// [E + 1], total int32 [1], tile_expert int32 [Tp / 256], slot int32 [P] (-1:
// dropped), row_src int32 [Tp] (valid rows only); table is int32 scratch
// [moe_plan_chunks(P), E]; cap 0 = dropless; Tp = moe_padded_rows(P, E).
// permute: x [T, H] bf16 -> x_pad [Tp, H]. combine: y_pad [Tp, H], slot
// [T, topk], w [T, topk] bf16 or fp32 (w_f32), null = unit weights -> y
// [T, H]. combine_bwd: dy [T, H], y_pad -> dy_pad [Tp, H], dw [T, topk] in
// w's type. H % 8 == 0; rows at or past total are never written.
void launch_moe_plan(const void* topi, void* table, void* counts, void* pad_off,
                     void* total, void* tile_expert, void* slot, void* row_src,
                     int P, int E, int cap, long Tp, hipStream_t stream);
void launch_moe_permute(const void* x, void* x_pad, const MoePlan& plan, int T,
                        int topk, int H, long Tp, hipStream_t stream);
void launch_moe_combine(const void* y_pad, const void* slot, const void* w,
                        bool w_f32, void* y, int T, int topk, int H, long Tp,
                        hipStream_t stream);
void launch_moe_combine_bwd(const void* dy, const void* y_pad, const void* w,
                            bool w_f32, const void* slot, void* dy_pad,
                            void* dw, const MoePlan& plan, int T, int topk,
                            int H, long Tp, hipStream_t stream);
// lm_head_loss.hip: hidden [N, H] and weight [V, H] dense bf16, H % LMHEAD_BK
// == 0, V % 8 == 0; targets int64 global ids; the shard owns ids
// [vocab_start, vocab_start + V). fwd: part[N, lmhead_vtiles(V)] float2 (max,
// sum-exp at that max) per row and vocab tile, and tgt[N] fp32, ZERO on entry,
// the target logit of the rows whose target the shard owns. merge: part ->
// row_max / row_sumexp [N] fp32, the outputs of launch_ce_fwd. dlogits: for
// `rows` rows (all row pointers already offset to the chunk), ds[rows, V]
// bf16 = (exp(logit - gmax) / gsum - onehot) * gout.
void launch_lmhead_ce_fwd(const void* hidden, const void* weight,
                          const void* targets, void* part, void* tgt, long N,
                          int H, int V, long vocab_start, hipStream_t stream);
void launch_lmhead_ce_merge(const void* part, void* row_max, void* row_sumexp,
                            long N, int n_vt, hipStream_t stream);
void launch_lmhead_ce_dlogits(const void* hidden, const void* weight,
                              const void* targets, const void* gmax,
                              const void* gsum, const void* gout, void* ds,
                              long rows, int H, int V, long vocab_start,
                              hipStream_t stream);
// lora.hip: all tensors dense row-major bf16, R in {8, 16, 32, 64}, W and N
// multiples of 8. shrink: h[T, R] = scale * x[T, W] m[R, W]^T. expand:
// out[T, N] = (base[T, N] +) scale * h[T, R] m[N, R]^T, base may be null.
// wgrad: g = scale * y[T, W]^T z[T, R], written as [W, R], or as [R, W] when
// out_rw; part is fp32 scratch [lora_wgrad_chunks(T), W, R].
void launch_lora_shrink(const void* x, const void* m, void* h, int T, int W,
                        int R, float scale, hipStream_t stream);
void launch_lora_expand(const void* h, const void* m, const void* base,
                        void* out, int T, int N, int R, float scale,
                        hipStream_t stream);
void launch_lora_wgrad(const void* y, const void* z, void* part, void* g,
                       int T, int W, int R, float scale, bool out_rw,
                       hipStream_t stream);
// flash_attn_decode.hip: split-KV decode forward, then the combine of the
// per-split partials
void launch_flash_decode(const FlashDecodeArgs& a, hipStream_t stream);
// flash_attn_fwd.hip: single-buffered forward (A/B arm), DENSE only
void launch_flash_fwd(const FlashArgs& a, hipStream_t stream);
// flash_attn_fwd_dbuf.hip: double-buffered forward, every mask, dropout; the
// A/B arm of the pipe kernel and the forward of every dropout call
void launch_flash_fwd_dbuf(const FlashArgs& a, hipStream_t stream);
// flash_attn_fwd_pipe.hip: swapped-operand forward (default), every mask,
// bit-equal to the dbuf kernel; a dropout call (drop_t > 0) is handed to
// launch_flash_fwd_dbuf
void launch_flash_fwd_pipe(const FlashArgs& a, hipStream_t stream);
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
// rmsnorm.hip, fused residual add: h = bf16(x + delta), y / invrms = the
// norm of h; dx = bf16(dh + dxn) with dxn what launch_rmsnorm_bwd stores,
// dh may be null (dx = dxn). All outputs but dw bit-equal to the unfused
// calls; dw fp32 [H], zeroed by the caller.
void launch_add_rmsnorm_fwd(const void* x, const void* delta, const void* w,
                            void* h, void* y, void* invrms, long N, int H,
                            float eps, hipStream_t stream);
void launch_add_rmsnorm_bwd(const void* dy, const void* dh, const void* h,
                            const void* w, const void* invrms, void* dx,
                            void* dw, long N, int H, hipStream_t stream);
// layernorm.hip: x, dy [N, H] bf16 dense, w, b [H] bf16, mean / rstd [N]
// fp32. bwd: part is fp32 scratch [grid, 2, H] with grid =
// layernorm_bwd_grid(N, H, CUs), every element of which the kernel writes;
// dwdb [2, H] fp32 = (dw, db), written, not accumulated.
void launch_layernorm_fwd(const void* x, const void* w, const void* b, void* y,
                          void* mean, void* rstd, long N, int H, float eps,
                          int num_cu, hipStream_t stream);
void launch_layernorm_bwd(const void* dy, const void* x, const void* w,
                          const void* mean, const void* rstd, void* dx,
                          void* part, void* dwdb, long N, int H, int grid,
                          hipStream_t stream);
void launch_swiglu_fwd(const void* gu, void* y, long N, int I,
                       hipStream_t stream);
void launch_swiglu_bwd(const void* dy, const void* gu, void* dgu, long N,
                       int I, hipStream_t stream);
// gelu.hip: exact (erf) GELU over n = N * I bf16 elements (n % 8 == 0), and
// GEGLU over gate_up [N, 2I] = [gate | up] -> y [N, I], dgu [N, 2I]
void launch_gelu_fwd(const void* x, void* y, long n, hipStream_t stream);
void launch_gelu_bwd(const void* dy, const void* x, void* dx, long n,
                     hipStream_t stream);
void launch_geglu_fwd(const void* gu, void* y, long N, int I,
                      hipStream_t stream);
void launch_geglu_bwd(const void* dy, const void* gu, void* dgu, long N,
                      int I, hipStream_t stream);
void launch_rope_fwd(const void* x, const void* cost, const void* sint,
                     void* y, int S, int B, int H, int D, const long* xstr,
                     int pos_offset, int pos_offset2, float sin_sign,
                     hipStream_t stream);
// rope.hip: q [b, hq, s, d] and k [b, hkv, s, d] in one launch, each with
// its own (seq, batch, head) strides; yq / yk dense [s, b, h, d]. Bit-equal
// to launch_rope_fwd on each tensor. 16-byte accesses where D % 16 == 0,
// the bases are 16 B-aligned and the strides multiples of 8; otherwise the
// scalar kernel of launch_rope_fwd, once per tensor.
void launch_rope_fwd_pair(const void* q, const void* k, const void* cost,
                          const void* sint, void* yq, void* yk, int S, int B,
                          int HQ, int HKV, int D, const long* qstr,
                          const long* kstr, int pos_offset, int pos_offset2,
                          float sin_sign, hipStream_t stream);
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
