// PyTorch bindings for the MI355X HIP kernels (gfx950-only build).
#include <torch/extension.h>

#include <cmath>
#include <cstdint>

#include <hip/hip_runtime.h>

#include <c10/hip/HIPStream.h>

#include "launch.h"

namespace {

hipStream_t cur_stream() {
  return c10::hip::getCurrentHIPStream().stream();
}

#define CHECK_IN(t)                                             \
  TORCH_CHECK((t).is_cuda(), #t " must be on GPU");             \
  TORCH_CHECK((t).is_contiguous(), #t " must be contiguous")

// The elementwise kernels index their arguments as dense arrays of one fixed
// type with no strides, so every tensor they read is checked here, before
// the launch: a dense tensor of `type` on the GPU of `ref` (t itself when it
// is the first argument) ...
static void check_dense(const torch::Tensor& t, const torch::Tensor& ref,
                        c10::ScalarType type, const char* op,
                        const char* name) {
  TORCH_CHECK(t.is_cuda() && t.device() == ref.device(), op, ": ", name,
              " must be on the GPU of the first argument");
  TORCH_CHECK(t.scalar_type() == type, op, ": ", name, " must be ",
              c10::toString(type));
  TORCH_CHECK(t.is_contiguous(), op, ": ", name, " must be contiguous");
}

// ... and, for a per-row or per-column vector, of exactly n elements.
static void check_vec(const torch::Tensor& t, const torch::Tensor& ref,
                      c10::ScalarType type, long n, const char* op,
                      const char* name) {
  check_dense(t, ref, type, op, name);
  TORCH_CHECK(t.numel() == n, op, ": ", name, " must have ", n,
              " elements, got ", t.numel());
}

std::vector<torch::Tensor> rmsnorm_fwd(torch::Tensor x, torch::Tensor w,
                                       double eps) {
  CHECK_IN(x);
  CHECK_IN(w);
  TORCH_CHECK(x.scalar_type() == torch::kBFloat16, "rmsnorm: bf16 only");
  TORCH_CHECK(w.scalar_type() == torch::kBFloat16, "rmsnorm: w must be bf16");
  TORCH_CHECK(x.dim() == 2, "rmsnorm: x must be [N, H]");
  auto N = x.size(0);
  auto H = x.size(1);
  TORCH_CHECK(H % 8 == 0, "hidden must be divisible by 8");
  check_vec(w, x, torch::kBFloat16, H, "rmsnorm", "w");
  auto y = torch::empty_like(x);
  auto invrms = torch::empty({N}, x.options().dtype(torch::kFloat32));
  if (N == 0 || H == 0) return {y, invrms};
  launch_rmsnorm_fwd(x.data_ptr(), w.data_ptr(), y.data_ptr(),
                     invrms.data_ptr(), N, (int)H, (float)eps, cur_stream());
  return {y, invrms};
}

// Returns {dx bf16 [N, H], dw fp32 [H]}: dw is the kernel's fp32 sum itself;
// the caller casts it to the dtype of its weight.
std::vector<torch::Tensor> rmsnorm_bwd(torch::Tensor dy, torch::Tensor x,
                                       torch::Tensor w, torch::Tensor invrms) {
  CHECK_IN(dy);
  CHECK_IN(x);
  CHECK_IN(w);
  TORCH_CHECK(w.scalar_type() == torch::kBFloat16, "rmsnorm: w must be bf16");
  check_dense(x, x, torch::kBFloat16, "rmsnorm_bwd", "x");
  TORCH_CHECK(x.dim() == 2, "rmsnorm_bwd: x must be [N, H]");
  auto N = x.size(0);
  auto H = x.size(1);
  TORCH_CHECK(H % 8 == 0, "hidden must be divisible by 8");
  check_dense(dy, x, torch::kBFloat16, "rmsnorm_bwd", "dy");
  TORCH_CHECK(dy.sizes() == x.sizes(), "rmsnorm_bwd: dy must have x's shape");
  check_vec(w, x, torch::kBFloat16, H, "rmsnorm_bwd", "w");
  check_vec(invrms, x, torch::kFloat32, N, "rmsnorm_bwd", "invrms");
  auto dx = torch::empty_like(x);
  auto dw32 = torch::zeros({H}, x.options().dtype(torch::kFloat32));
  if (N == 0 || H == 0) return {dx, dw32};
  launch_rmsnorm_bwd(dy.data_ptr(), x.data_ptr(), w.data_ptr(),
                     invrms.data_ptr(), dx.data_ptr(), dw32.data_ptr(), N,
                     (int)H, cur_stream());
  return {dx, dw32};
}

torch::Tensor swiglu_fwd(torch::Tensor gu) {
  CHECK_IN(gu);
  check_dense(gu, gu, torch::kBFloat16, "swiglu_fwd", "gate_up");
  TORCH_CHECK(gu.dim() == 2 && gu.size(1) % 2 == 0,
              "swiglu_fwd: gate_up must be [N, 2 * I]");
  auto N = gu.size(0);
  auto I = gu.size(1) / 2;
  TORCH_CHECK(I % 8 == 0, "intermediate must be divisible by 8");
  auto y = torch::empty({N, I}, gu.options());
  if (N == 0 || I == 0) return y;
  launch_swiglu_fwd(gu.data_ptr(), y.data_ptr(), N, (int)I, cur_stream());
  return y;
}

torch::Tensor swiglu_bwd(torch::Tensor dy, torch::Tensor gu) {
  CHECK_IN(dy);
  CHECK_IN(gu);
  check_dense(gu, gu, torch::kBFloat16, "swiglu_bwd", "gate_up");
  TORCH_CHECK(gu.dim() == 2 && gu.size(1) % 2 == 0,
              "swiglu_bwd: gate_up must be [N, 2 * I]");
  auto N = gu.size(0);
  auto I = gu.size(1) / 2;
  TORCH_CHECK(I % 8 == 0, "intermediate must be divisible by 8");
  check_dense(dy, gu, torch::kBFloat16, "swiglu_bwd", "dy");
  TORCH_CHECK(dy.dim() == 2 && dy.size(0) == N && dy.size(1) == I,
              "swiglu_bwd: dy must be [N, I]");
  auto dgu = torch::empty_like(gu);
  if (N == 0 || I == 0) return dgu;
  launch_swiglu_bwd(dy.data_ptr(), gu.data_ptr(), dgu.data_ptr(), N, (int)I,
                    cur_stream());
  return dgu;
}

torch::Tensor rope_fwd(torch::Tensor x, torch::Tensor cost, torch::Tensor sint,
                       long pos_offset, long pos_offset2) {
  // x: logical [b, h, s, d], any strides with d contiguous (e.g. a view of
  // the fused QKV output). Returns a [s, b, h, d]-contiguous tensor exposed
  // as a [b, h, s, d] view — zero permute copies in the attention path.
  // pos_offset2 >= 0: zigzag CP layout — rows [s/2, s) take positions
  // pos_offset2 + i instead of pos_offset + s/2 + i.
  TORCH_CHECK(x.is_cuda() && x.dim() == 4 && x.stride(3) == 1,
              "rope: x must be [b, h, s, d] on GPU with d contiguous");
  TORCH_CHECK(x.scalar_type() == torch::kBFloat16, "rope: x must be bf16");
  int B = (int)x.size(0), H = (int)x.size(1), S = (int)x.size(2),
      D = (int)x.size(3);
  // the kernel pairs column d with d + D / 2
  TORCH_CHECK(D % 2 == 0, "rope: head_dim must be even, got ", D);
  TORCH_CHECK(pos_offset2 < 0 || S % 2 == 0, "zigzag rope needs even s");
  // Both tables are read as dense fp32 [rows, D] at rows pos_offset + i; in
  // the zigzag layout the first half reads pos_offset + [0, S / 2) and the
  // second pos_offset2 + [0, S / 2).
  const long first = pos_offset2 < 0 ? S : S / 2;
  long need = pos_offset + first;
  if (pos_offset2 >= 0 && pos_offset2 + S / 2 > need)
    need = pos_offset2 + S / 2;
  TORCH_CHECK(pos_offset >= 0, "rope: pos_offset must be >= 0");
  for (const torch::Tensor* t : {&cost, &sint}) {
    const char* name = t == &cost ? "cos" : "sin";
    TORCH_CHECK(t->is_cuda() && t->device() == x.device(), "rope: ", name,
                " table must be on x's GPU");
    TORCH_CHECK(t->scalar_type() == torch::kFloat32, "rope: ", name,
                " table must be f32");
    TORCH_CHECK(t->dim() == 2 && t->size(1) == D, "rope: ", name,
                " table must be [rows, head_dim]");
    TORCH_CHECK(S == 0 || t->size(0) >= need, "rope: ", name, " table has ",
                t->size(0), " rows, positions reach ", need);
  }
  auto cos_c = cost.contiguous();
  auto sin_c = sint.contiguous();
  auto y_mem = torch::empty({S, B, H, D}, x.options());
  if (y_mem.numel() == 0) return y_mem.permute({1, 2, 0, 3});
  long xstr[3] = {x.stride(2), x.stride(0), x.stride(1)};  // s, b, h
  launch_rope_fwd(x.data_ptr(), cos_c.data_ptr(), sin_c.data_ptr(),
                  y_mem.data_ptr(), S, B, H, D, xstr, (int)pos_offset,
                  (int)pos_offset2, 1.0f, cur_stream());
  return y_mem.permute({1, 2, 0, 3});
}

static void check_adamw_f32(const torch::Tensor& t, const torch::Tensor& p,
                            const char* name) {
  TORCH_CHECK(t.is_cuda() && t.device() == p.device(), "adamw: ", name,
              " must be on the same GPU as p");
  TORCH_CHECK(t.scalar_type() == torch::kFloat32, "adamw: ", name,
              " must be fp32");
  TORCH_CHECK(t.is_contiguous(), "adamw: ", name, " must be contiguous");
  TORCH_CHECK(t.numel() == p.numel(), "adamw: ", name,
              " must have p's numel");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0, "adamw: ",
              name, " must be 16-byte aligned");
}

void adamw_step(torch::Tensor p, torch::Tensor g, torch::Tensor m,
                torch::Tensor v, torch::Tensor wd_mask, double lr, double b1,
                double b2, double eps, double wd, long step,
                c10::optional<torch::Tensor> grad_scale,
                c10::optional<torch::Tensor> p_bf16) {
  // The kernel indexes all five arrays as dense [n] with no strides and
  // moves p/g/m/v as float4 and p_bf16 as int2, so everything it reads is
  // checked here, before the launch.
  check_adamw_f32(p, p, "p");
  check_adamw_f32(g, p, "g");
  check_adamw_f32(m, p, "m");
  check_adamw_f32(v, p, "v");
  TORCH_CHECK(wd_mask.is_cuda() && wd_mask.device() == p.device(),
              "adamw: wd_mask must be on the same GPU as p");
  TORCH_CHECK(wd_mask.scalar_type() == torch::kBool,
              "adamw: wd_mask must be bool");
  TORCH_CHECK(wd_mask.is_contiguous() && wd_mask.numel() == p.numel(),
              "adamw: wd_mask must be contiguous with p's numel");
  // bc1 = 1 - b1^step and bc2 = 1 - b2^step are both zero at step 0
  TORCH_CHECK(step >= 1, "adamw: step must be >= 1");
  void* gs = nullptr;
  if (grad_scale.has_value()) {
    TORCH_CHECK(grad_scale->scalar_type() == torch::kFloat32 &&
                    grad_scale->is_cuda() &&
                    grad_scale->device() == p.device(),
                "grad_scale must be a device fp32 scalar");
    TORCH_CHECK(grad_scale->numel() == 1,
                "grad_scale must have exactly one element");
    gs = grad_scale->data_ptr();
  }
  void* pb = nullptr;
  if (p_bf16.has_value()) {
    TORCH_CHECK(p_bf16->is_cuda() && p_bf16->device() == p.device(),
                "adamw: p_bf16 must be on the same GPU as p");
    TORCH_CHECK(p_bf16->scalar_type() == torch::kBFloat16 &&
                    p_bf16->is_contiguous() && p_bf16->numel() == p.numel(),
                "p_bf16 must be contiguous bf16 of the same numel");
    TORCH_CHECK(reinterpret_cast<uintptr_t>(p_bf16->data_ptr()) % 8 == 0,
                "adamw: p_bf16 must be 8-byte aligned");
    pb = p_bf16->data_ptr();
  }
  launch_adamw(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(),
               wd_mask.data_ptr(), gs, pb, p.numel(), (float)lr, (float)b1,
               (float)b2, (float)eps, (float)wd, (int)step, cur_stream());
}

static void check_bhsd(const torch::Tensor& t, const char* name) {
  TORCH_CHECK(t.is_cuda() && t.dim() == 4 && t.stride(3) == 1,
              name, " must be [b, h, s, d] on GPU with d contiguous");
  TORCH_CHECK(t.scalar_type() == torch::kBFloat16, name, " must be bf16");
}

// Shared argument contract of the three backward bindings. The kernels
// index LSE as a dense [B, HQ, SQ] fp32 array (no strides), so a view such
// as the ring's lse[:, :, half:] is copied (B*HQ*SQ floats); returns the
// LSE to hand to the kernel.
static torch::Tensor check_bwd_args(const torch::Tensor& q,
                                    const torch::Tensor& k,
                                    const torch::Tensor& v,
                                    const torch::Tensor& lse) {
  check_bhsd(k, "k");
  check_bhsd(v, "v");
  TORCH_CHECK(q.size(3) == 128 || q.size(3) == 64,
              "head_dim must be 64 or 128");
  TORCH_CHECK(k.size(1) > 0 && q.size(1) % k.size(1) == 0,
              "GQA head mismatch");
  TORCH_CHECK(lse.is_cuda() && lse.device() == q.device(),
              "lse must be on the same GPU as q");
  TORCH_CHECK(lse.scalar_type() == torch::kFloat32, "lse must be fp32");
  TORCH_CHECK(lse.dim() == 3 && lse.size(0) == q.size(0) &&
                  lse.size(1) == q.size(1) && lse.size(2) == q.size(2),
              "lse must have shape [B, HQ, SQ]");
  return lse.contiguous();
}

static void check_kv_range(const torch::Tensor& t, const torch::Tensor& q,
                           const char* name) {
  TORCH_CHECK(t.is_cuda() && t.device() == q.device(), name,
              " must be on the same GPU as q");
  TORCH_CHECK(t.scalar_type() == torch::kInt, name, " must be int32");
  TORCH_CHECK(t.dim() == 1 && t.size(0) == q.size(0), name,
              " must have shape [B]");
  TORCH_CHECK(t.is_contiguous(), name, " must be contiguous");
}

static void check_seg_bound(const torch::Tensor& t, const torch::Tensor& q,
                            const char* name) {
  TORCH_CHECK(t.is_cuda() && t.device() == q.device(), name,
              " must be on the same GPU as q");
  TORCH_CHECK(t.scalar_type() == torch::kInt, name, " must be int32");
  TORCH_CHECK(t.dim() == 2 && t.size(0) == q.size(0) &&
                  t.size(1) == q.size(2),
              name, " must have shape [B, S]");
  TORCH_CHECK(t.is_contiguous(), name, " must be contiguous");
}

// (seq, batch, head) element strides of a logical [b, h, s, d] tensor
static void sbh_strides(const torch::Tensor& t, long (&s)[3]) {
  s[0] = t.stride(2);
  s[1] = t.stride(0);
  s[2] = t.stride(1);
}

// The launch arguments that q / k / v and the scalars decide; q, k and v have
// passed check_bhsd. Outputs, the backward tensors and the mask bounds are
// null / DENSE until the caller sets them.
static FlashArgs flash_args(const torch::Tensor& q, const torch::Tensor& k,
                            const torch::Tensor& v, bool causal, double scale,
                            long window) {
  FlashArgs a{};
  a.q = q.data_ptr();
  a.k = k.data_ptr();
  a.v = v.data_ptr();
  a.B = (int)q.size(0);
  a.HQ = (int)q.size(1);
  a.SQ = (int)q.size(2);
  a.D = (int)q.size(3);
  a.HKV = (int)k.size(1);
  a.SKV = (int)k.size(2);
  a.causal = causal;
  a.scale = (float)scale;
  a.window = (int)window;
  sbh_strides(q, a.qs);
  sbh_strides(k, a.ks);
  sbh_strides(v, a.vs);
  return a;
}

static void set_mask(FlashArgs& a, FlashArgs::Mask mask,
                     const torch::Tensor* lo, const torch::Tensor* hi) {
  a.mask = mask;
  if (mask != FlashArgs::DENSE) {
    a.bound_a = lo->data_ptr<int>();
    a.bound_b = hi->data_ptr<int>();
  }
}

// Attention dropout: p_drop in [0, 1) -> 8-bit threshold t = round(256 * p)
// (an element is dropped iff its random byte is < t; 0 = no dropout). A p
// that rounds to 256 would drop everything and is rejected with the rest.
static int drop_threshold(double p_drop) {
  TORCH_CHECK(p_drop >= 0.0 && p_drop < 1.0,
              "p_drop must be in [0, 1), got ", p_drop);
  const long t = std::lround(256.0 * p_drop);
  TORCH_CHECK(t <= 255, "p_drop ", p_drop,
              " rounds to 256/256: the threshold has 8 bits");
  return (int)t;
}

static void set_dropout(FlashArgs& a, double p_drop, uint64_t seed,
                        uint64_t offset) {
  a.drop_t = drop_threshold(p_drop);
  a.drop_seed = seed;
  a.drop_offset = offset;
}

static torch::Tensor attn_delta(torch::Tensor dout, torch::Tensor o) {
  // fused rowsum(dO . O) -> [B, HQ, SQ] fp32 (no fp32 materialization)
  auto oc = o.stride(3) == 1 ? o : o.contiguous();
  int B = (int)dout.size(0), HQ = (int)dout.size(1), SQ = (int)dout.size(2),
      D = (int)dout.size(3);
  auto delta = torch::empty(
      {B, HQ, SQ}, dout.options().dtype(torch::kFloat32));
  long ds[3], os_[3];
  sbh_strides(dout, ds);
  sbh_strides(oc, os_);
  launch_attn_delta(dout.data_ptr(), oc.data_ptr(), delta.data_ptr(), SQ, B,
                    HQ, D, ds, os_, cur_stream());
  return delta;
}

// Allocates O and LSE, runs launch(a, stream) and returns O as a
// [b, h, s, d] view of its [s, b, h, d] storage, and LSE [B, HQ, SQ] fp32.
template <class Launch>
static std::vector<torch::Tensor> flash_fwd_run(FlashArgs a,
                                                const torch::Tensor& q,
                                                Launch launch) {
  auto o_mem = torch::empty({a.SQ, a.B, a.HQ, a.D}, q.options());
  auto lse =
      torch::empty({a.B, a.HQ, a.SQ}, q.options().dtype(torch::kFloat32));
  a.o = o_mem.data_ptr();
  a.lse = lse.data_ptr();
  launch(a, cur_stream());
  return {o_mem.permute({1, 2, 0, 3}), lse};
}

// delta, the outputs, launch(a, stream), and the sum over the GQA partial
// slabs; dout, q and lse are the tensors handed to the kernels.
template <class Launch>
static std::vector<torch::Tensor> flash_bwd_run(FlashArgs a,
                                                const torch::Tensor& dout,
                                                const torch::Tensor& q,
                                                const torch::Tensor& o,
                                                const torch::Tensor& lse,
                                                Launch launch) {
  auto delta = attn_delta(dout, o);  // [B, HQ, SQ] f32, fused
  // every q-block / key-block stores its whole slab (zeros where a range or
  // a segment leaves it no work), so torch::empty is safe
  auto dq_mem = torch::empty({a.SQ, a.B, a.HQ, a.D}, q.options());
  // dkv writes one fp32 partial slab per q-head of each GQA group (full
  // grid occupancy at high TP); sum + cast here
  int group = a.HQ / a.HKV;
  auto f32 = q.options().dtype(torch::kFloat32);
  auto dk_part = torch::empty({group, a.SKV, a.B, a.HKV, a.D}, f32);
  auto dv_part = torch::empty({group, a.SKV, a.B, a.HKV, a.D}, f32);
  a.dout = dout.data_ptr();
  sbh_strides(dout, a.ds);
  a.lse = lse.data_ptr();
  a.delta = delta.data_ptr();
  a.dq = dq_mem.data_ptr();
  a.dk = dk_part.data_ptr();
  a.dv = dv_part.data_ptr();
  launch(a, cur_stream());
  auto dk_mem = dk_part.sum(0).to(torch::kBFloat16);
  auto dv_mem = dv_part.sum(0).to(torch::kBFloat16);
  return {dq_mem.permute({1, 2, 0, 3}), dk_mem.permute({1, 2, 0, 3}),
          dv_mem.permute({1, 2, 0, 3})};
}

std::vector<torch::Tensor> flash_attn_fwd_v3(torch::Tensor q, torch::Tensor k,
                                             torch::Tensor v, bool causal,
                                             double scale, long window) {
  // T12 swapped-operand forward (ROADMAP §1); dark until HW-validated
  check_bhsd(q, "q");
  check_bhsd(k, "k");
  check_bhsd(v, "v");
  FlashArgs a = flash_args(q, k, v, causal, scale, window);
  TORCH_CHECK(a.D == 128 || a.D == 64, "head_dim must be 64 or 128");
  TORCH_CHECK(a.SKV == a.SQ, "v3 kernel requires S_q == S_kv (use v2)");
  return flash_fwd_run(a, q, launch_flash_fwd_v3);
}

std::vector<torch::Tensor> flash_attn_bwd_v3(torch::Tensor dout,
                                             torch::Tensor q, torch::Tensor k,
                                             torch::Tensor v, torch::Tensor o,
                                             torch::Tensor lse, bool causal,
                                             double scale, long window) {
  if (dout.stride(3) != 1) dout = dout.contiguous();
  check_bhsd(dout, "dout");
  check_bhsd(q, "q");
  lse = check_bwd_args(q, k, v, lse);
  FlashArgs a = flash_args(q, k, v, causal, scale, window);
  TORCH_CHECK(a.SKV == a.SQ, "v3 kernel requires S_q == S_kv (use v2)");
  return flash_bwd_run(a, dout, q, o, lse, launch_flash_bwd_v3);
}

// Shared body of the four forward bindings. q/k/v: logical [b, h, s, d],
// arbitrary strides (views of the QKV GEMM output). S_q != S_kv supported;
// causal is then bottom-right aligned (decode / ring-attention half-block
// convention, requires S_kv >= S_q). dbuf selects the kernel: true = the
// double-buffered staging kernel (the default: bit-identical output,
// measured +3.0% (bench shape) / +1.8% (TP=8 shape)), false = the
// single-buffered kernel it replaced (flash_attn_fwd_sbuf, kept for A/B;
// DENSE only).
// RANGED: per-batch-row visible key range [kv_lo[b], kv_hi[b]) (padded
// batches), lo = kv_lo, hi = kv_hi, int32 [B]. Values are trusted to satisfy
// 0 <= lo <= hi <= S_kv; the Python op clamps them.
// SEGMENTED: causal attention over packed sequences: query i of row b sees
// keys q_start[b,i] <= j <= i (block-diagonal mask); k_end[b,j] is one past
// the last query that sees key j. lo = q_start, hi = k_end, int32 [B, S].
// Values are trusted to be non-decreasing along each row with
// 0 <= q_start[b,i] <= i < k_end[b,i] <= S; the Python op derives them from
// segment ids.
// p_drop (non-null only from flash_attn_fwd_drop, DENSE): attention dropout
// on the probabilities with the keep mask of stream (seed, offset).
static std::vector<torch::Tensor> flash_fwd_common(
    bool dbuf, FlashArgs::Mask mask, torch::Tensor q, torch::Tensor k,
    torch::Tensor v, const torch::Tensor* lo, const torch::Tensor* hi,
    bool causal, double scale, long window, const double* p_drop = nullptr,
    uint64_t seed = 0, uint64_t offset = 0) {
  check_bhsd(q, "q");
  check_bhsd(k, "k");
  check_bhsd(v, "v");
  FlashArgs a = flash_args(q, k, v, causal, scale, window);
  if (mask == FlashArgs::RANGED) {
    check_kv_range(*lo, q, "kv_lo");
    check_kv_range(*hi, q, "kv_hi");
  }
  if (mask == FlashArgs::SEGMENTED) {
    TORCH_CHECK(a.SKV == a.SQ, "segmented attention needs S_q == S_kv");
    check_seg_bound(*lo, q, "q_start");
    check_seg_bound(*hi, q, "k_end");
  }
  TORCH_CHECK(a.D == 128 || a.D == 64, "head_dim must be 64 or 128");
  TORCH_CHECK(a.HQ % a.HKV == 0, "GQA head mismatch");
  if (mask != FlashArgs::SEGMENTED)
    TORCH_CHECK(!causal || a.SKV >= a.SQ, "causal needs S_kv >= S_q");
  set_mask(a, mask, lo, hi);
  if (p_drop) set_dropout(a, *p_drop, seed, offset);
  return flash_fwd_run(a, q,
                       dbuf ? launch_flash_fwd_dbuf : launch_flash_fwd);
}

std::vector<torch::Tensor> flash_attn_fwd(torch::Tensor q, torch::Tensor k,
                                          torch::Tensor v, bool causal,
                                          double scale, long window) {
  return flash_fwd_common(true, FlashArgs::DENSE, q, k, v, nullptr, nullptr,
                          causal, scale, window);
}

std::vector<torch::Tensor> flash_attn_fwd_sbuf(torch::Tensor q,
                                               torch::Tensor k,
                                               torch::Tensor v, bool causal,
                                               double scale, long window) {
  return flash_fwd_common(false, FlashArgs::DENSE, q, k, v, nullptr, nullptr,
                          causal, scale, window);
}

std::vector<torch::Tensor> flash_attn_fwd_range(
    torch::Tensor q, torch::Tensor k, torch::Tensor v, torch::Tensor kv_lo,
    torch::Tensor kv_hi, bool causal, double scale, long window) {
  return flash_fwd_common(true, FlashArgs::RANGED, q, k, v, &kv_lo, &kv_hi,
                          causal, scale, window);
}

std::vector<torch::Tensor> flash_attn_fwd_seg(
    torch::Tensor q, torch::Tensor k, torch::Tensor v, torch::Tensor q_start,
    torch::Tensor k_end, double scale, long window) {
  return flash_fwd_common(true, FlashArgs::SEGMENTED, q, k, v, &q_start,
                          &k_end, true, scale, window);
}

// Dense attention with dropout on the probabilities: O = ((P . M) V) *
// keep_scale with the keep mask M of flash_attn_dropout_mask(.., p_drop,
// seed, offset); LSE is that of the undropped softmax. t == 0 (p_drop below
// 1/512) is the dense kernel.
std::vector<torch::Tensor> flash_attn_fwd_drop(
    torch::Tensor q, torch::Tensor k, torch::Tensor v, bool causal,
    double scale, long window, double p_drop, uint64_t seed,
    uint64_t offset) {
  return flash_fwd_common(true, FlashArgs::DENSE, q, k, v, nullptr, nullptr,
                          causal, scale, window, &p_drop, seed, offset);
}

// The keep mask of (p_drop, seed, offset) as uint8 [B, HQ, SQ, SKV] on the
// current device, 1 = keep: test and debug support, on no hot path.
torch::Tensor flash_attn_dropout_mask(long B, long HQ, long SQ, long SKV,
                                      double p_drop, uint64_t seed,
                                      uint64_t offset) {
  const int t = drop_threshold(p_drop);
  TORCH_CHECK(B >= 0 && HQ >= 0 && SQ >= 0 && SKV >= 0,
              "dropout mask: negative size");
  TORCH_CHECK(B * HQ < (1L << 31) && SQ < (1L << 31) && SKV < (1L << 31),
              "dropout mask: B * HQ, SQ and SKV must be below 2^31");
  // one thread per element, 256 per block, grid.x < 2^31
  TORCH_CHECK((double)B * HQ * SQ * SKV < 256.0 * 2147483647.0,
              "dropout mask: too many elements");
  auto mask = torch::empty(
      {B, HQ, SQ, SKV},
      torch::TensorOptions().dtype(torch::kUInt8).device(
          torch::kCUDA, c10::hip::current_device()));
  launch_attn_dropout_mask(mask.data_ptr(), (int)B, (int)HQ, (int)SQ,
                           (int)SKV, t, seed, offset, cur_stream());
  return mask;
}

// Shared body of the six backward bindings; mask, lo and hi as in
// flash_fwd_common. pipe selects the dK/dV kernel: true = the pipelined
// kernel (flash_attn_bwd_dkv_pipe.hip, the default), false = the
// single-buffered kernel it replaced (the *_sbuf bindings, kept for A/B;
// bit-identical). dQ, delta and every check are shared.
static std::vector<torch::Tensor> flash_bwd_common(
    FlashArgs::Mask mask, bool pipe, torch::Tensor dout, torch::Tensor q,
    torch::Tensor k, torch::Tensor v, torch::Tensor o, torch::Tensor lse,
    const torch::Tensor* lo, const torch::Tensor* hi, bool causal,
    double scale, long window, const double* p_drop = nullptr,
    uint64_t seed = 0, uint64_t offset = 0) {
  if (dout.stride(3) != 1) dout = dout.contiguous();
  check_bhsd(dout, "dout");
  check_bhsd(q, "q");
  lse = check_bwd_args(q, k, v, lse);
  FlashArgs a = flash_args(q, k, v, causal, scale, window);
  if (mask == FlashArgs::RANGED) {
    check_kv_range(*lo, q, "kv_lo");
    check_kv_range(*hi, q, "kv_hi");
  }
  if (mask == FlashArgs::SEGMENTED) {
    TORCH_CHECK(a.SKV == a.SQ, "segmented attention needs S_q == S_kv");
    check_seg_bound(*lo, q, "q_start");
    check_seg_bound(*hi, q, "k_end");
  } else {
    TORCH_CHECK(!causal || a.SKV >= a.SQ, "causal needs S_kv >= S_q");
  }
  // the pipelined kernel addresses a 64-row tile with 32-bit byte offsets
  TORCH_CHECK(!pipe || (q.stride(2) >= 0 && q.stride(2) < (1L << 24) &&
                        dout.stride(2) >= 0 && dout.stride(2) < (1L << 24)),
              "q / dout sequence stride must be below 2^24 elements");
  set_mask(a, mask, lo, hi);
  if (p_drop) set_dropout(a, *p_drop, seed, offset);
  return flash_bwd_run(a, dout, q, o, lse,
                       [pipe](const FlashArgs& f, hipStream_t stream) {
                         launch_flash_bwd(f, pipe, stream);
                       });
}

#define BWD_BINDINGS(SUFFIX, PIPE)                                            \
  std::vector<torch::Tensor> flash_attn_bwd##SUFFIX(                          \
      torch::Tensor dout, torch::Tensor q, torch::Tensor k, torch::Tensor v,  \
      torch::Tensor o, torch::Tensor lse, bool causal, double scale,          \
      long window) {                                                          \
    return flash_bwd_common(FlashArgs::DENSE, PIPE, dout, q, k, v, o, lse,    \
                            nullptr, nullptr, causal, scale, window);         \
  }                                                                           \
  std::vector<torch::Tensor> flash_attn_bwd_range##SUFFIX(                    \
      torch::Tensor dout, torch::Tensor q, torch::Tensor k, torch::Tensor v,  \
      torch::Tensor o, torch::Tensor lse, torch::Tensor kv_lo,                \
      torch::Tensor kv_hi, bool causal, double scale, long window) {          \
    return flash_bwd_common(FlashArgs::RANGED, PIPE, dout, q, k, v, o, lse,   \
                            &kv_lo, &kv_hi, causal, scale, window);           \
  }                                                                           \
  std::vector<torch::Tensor> flash_attn_bwd_seg##SUFFIX(                      \
      torch::Tensor dout, torch::Tensor q, torch::Tensor k, torch::Tensor v,  \
      torch::Tensor o, torch::Tensor lse, torch::Tensor q_start,              \
      torch::Tensor k_end, double scale, long window) {                       \
    return flash_bwd_common(FlashArgs::SEGMENTED, PIPE, dout, q, k, v, o,     \
                            lse, &q_start, &k_end, true, scale, window);      \
  }
BWD_BINDINGS(, true)        // pipelined dK/dV (default)
BWD_BINDINGS(_sbuf, false)  // the kernel it replaced, for A/B
#undef BWD_BINDINGS

// Backward of flash_attn_fwd_drop: o and lse are its outputs, and (p_drop,
// seed, offset) the values it was given; the kernels regenerate the mask.
// dK/dV always come from the pipelined kernel.
std::vector<torch::Tensor> flash_attn_bwd_drop(
    torch::Tensor dout, torch::Tensor q, torch::Tensor k, torch::Tensor v,
    torch::Tensor o, torch::Tensor lse, bool causal, double scale,
    long window, double p_drop, uint64_t seed, uint64_t offset) {
  return flash_bwd_common(FlashArgs::DENSE, true, dout, q, k, v, o, lse,
                          nullptr, nullptr, causal, scale, window, &p_drop,
                          seed, offset);
}

torch::Tensor moe_gemm(torch::Tensor a, torch::Tensor w,
                       torch::Tensor tile_expert, torch::Tensor total_rows,
                       bool trans_b) {
  // a: [Tp, K] bf16 padded/sorted tokens; w: [E, N, Kw] bf16 expert slabs.
  // trans_b=false: C = a @ w[e]^T ([Tp, N]); true: C = a @ w[e] ([Tp, Kw]).
  CHECK_IN(a);
  CHECK_IN(w);
  CHECK_IN(tile_expert);
  CHECK_IN(total_rows);
  TORCH_CHECK(a.dim() == 2, "moe_gemm: a must be [Tp, K]");
  TORCH_CHECK(w.dim() == 3, "moe_gemm: w must be [E, N, Kw]");
  TORCH_CHECK(a.scalar_type() == torch::kBFloat16 &&
                  w.scalar_type() == torch::kBFloat16,
              "moe_gemm: bf16 only");
  TORCH_CHECK(tile_expert.scalar_type() == torch::kInt &&
                  total_rows.scalar_type() == torch::kInt,
              "moe_gemm: int32 maps");
  TORCH_CHECK(w.device() == a.device() && tile_expert.device() == a.device() &&
                  total_rows.device() == a.device(),
              "moe_gemm: w and the int32 maps must be on a's device");
  TORCH_CHECK(total_rows.numel() == 1, "moe_gemm: total_rows must be [1]");
  long Tp = a.size(0);
  int K = (int)a.size(1);
  int N = (int)w.size(1), Kw = (int)w.size(2);
  TORCH_CHECK(Tp % 256 == 0, "padded rows must be a multiple of 256");
  int row_tiles = (int)(Tp / 256);
  int contraction = trans_b ? N : Kw;
  int out_cols = trans_b ? Kw : N;
  TORCH_CHECK(K == contraction, "moe_gemm: contraction mismatch");
  // 16-byte row loads of a and w need every row start 16-byte aligned
  TORCH_CHECK(K % 8 == 0, "moe_gemm: contraction % 8");
  TORCH_CHECK(out_cols % 128 == 0, "moe_gemm: out cols % 128");
  TORCH_CHECK(tile_expert.numel() >= row_tiles,
              "moe_gemm: tile_expert shorter than Tp / 256");
  auto c = torch::empty({Tp, out_cols}, a.options());
  launch_moe_gemm(a.data_ptr(), w.data_ptr(), c.data_ptr(),
                  tile_expert.data_ptr<int>(), total_rows.data_ptr<int>(),
                  row_tiles, K, out_cols, (long)N * Kw, trans_b,
                  cur_stream());
  return c;
}

torch::Tensor moe_wgrad(torch::Tensor dy, torch::Tensor x,
                        torch::Tensor seg_start, long E) {
  // dW[e] = dy[seg_e]^T @ x[seg_e] -> [E, N, K] fp32
  CHECK_IN(dy);
  CHECK_IN(x);
  CHECK_IN(seg_start);
  TORCH_CHECK(dy.dim() == 2 && x.dim() == 2,
              "moe_wgrad: dy must be [Tp, N] and x [Tp, K]");
  TORCH_CHECK(dy.scalar_type() == torch::kBFloat16 &&
                  x.scalar_type() == torch::kBFloat16,
              "moe_wgrad: bf16 only");
  TORCH_CHECK(seg_start.scalar_type() == torch::kInt, "int32 seg bounds");
  TORCH_CHECK(x.device() == dy.device() && seg_start.device() == dy.device(),
              "moe_wgrad: x and seg_start must be on dy's device");
  TORCH_CHECK(dy.size(0) == x.size(0), "moe_wgrad: dy and x row counts differ");
  // the kernel walks each segment in 32-row chunks
  TORCH_CHECK(dy.size(0) % 32 == 0, "moe_wgrad: rows % 32");
  TORCH_CHECK(E >= 1 && seg_start.numel() == E + 1,
              "moe_wgrad: seg_start must have E + 1 entries");
  int N = (int)dy.size(1), K = (int)x.size(1);
  TORCH_CHECK(N % 128 == 0 && K % 128 == 0, "moe_wgrad: dims % 128");
  auto dw = torch::empty({E, N, K}, dy.options().dtype(torch::kFloat32));
  launch_moe_wgrad(dy.data_ptr(), x.data_ptr(), dw.data_ptr(),
                   seg_start.data_ptr<int>(), (int)E, N, K, cur_stream());
  return dw;
}

torch::Tensor mfma_probe(torch::Tensor a, torch::Tensor b) {
  CHECK_IN(a);
  CHECK_IN(b);
  auto c = torch::empty({16, 16}, a.options().dtype(torch::kFloat32));
  launch_mfma_probe(a.data_ptr(), b.data_ptr(), c.data_ptr(), cur_stream());
  return c;
}

torch::Tensor mfma_probe32(torch::Tensor a, torch::Tensor b) {
  CHECK_IN(a);
  CHECK_IN(b);
  auto c = torch::empty({32, 32}, a.options().dtype(torch::kFloat32));
  launch_mfma_probe32(a.data_ptr(), b.data_ptr(), c.data_ptr(), cur_stream());
  return c;
}

std::vector<torch::Tensor> ce_fwd(torch::Tensor logits, torch::Tensor targets,
                                  long vocab_start) {
  CHECK_IN(logits);
  TORCH_CHECK(logits.scalar_type() == torch::kBFloat16, "ce: bf16 logits");
  TORCH_CHECK(targets.scalar_type() == torch::kLong, "ce: int64 targets");
  TORCH_CHECK(logits.dim() == 2, "ce: logits must be [N, V]");
  long N = logits.size(0);
  int V = (int)logits.size(1);
  TORCH_CHECK(targets.is_cuda() && targets.device() == logits.device(),
              "ce: targets must be on the GPU of logits");
  TORCH_CHECK(targets.numel() == N, "ce: targets must have N elements");
  auto opt = logits.options().dtype(torch::kFloat32);
  auto row_max = torch::empty({N}, opt);
  auto row_sumexp = torch::empty({N}, opt);
  auto tgt = torch::empty({N}, opt);
  if (N == 0) return {row_max, row_sumexp, tgt};
  launch_ce_fwd(logits.data_ptr(), targets.contiguous().data_ptr(),
                row_max.data_ptr(), row_sumexp.data_ptr(), tgt.data_ptr(), N,
                V, vocab_start, cur_stream());
  return {row_max, row_sumexp, tgt};
}

torch::Tensor ce_bwd(torch::Tensor logits, torch::Tensor targets,
                     torch::Tensor gmax, torch::Tensor gsum,
                     torch::Tensor gout, long vocab_start) {
  CHECK_IN(logits);
  TORCH_CHECK(logits.scalar_type() == torch::kBFloat16, "ce: bf16 logits");
  TORCH_CHECK(logits.dim() == 2, "ce: logits must be [N, V]");
  long N = logits.size(0);
  int V = (int)logits.size(1);
  // per-row vectors the kernel indexes by row; a strided one is copied below
  const struct {
    const torch::Tensor& t;
    c10::ScalarType type;
    const char* name;
  } rows[] = {{targets, torch::kLong, "targets"},
              {gmax, torch::kFloat32, "gmax"},
              {gsum, torch::kFloat32, "gsum"},
              {gout, torch::kFloat32, "gout"}};
  for (const auto& r : rows) {
    TORCH_CHECK(r.t.is_cuda() && r.t.device() == logits.device(), "ce_bwd: ",
                r.name, " must be on the GPU of logits");
    TORCH_CHECK(r.t.scalar_type() == r.type, "ce_bwd: ", r.name, " must be ",
                c10::toString(r.type));
    TORCH_CHECK(r.t.numel() == N, "ce_bwd: ", r.name,
                " must have N elements");
  }
  auto dl = torch::empty_like(logits);
  if (dl.numel() == 0) return dl;
  launch_ce_bwd(logits.data_ptr(), targets.contiguous().data_ptr(),
                gmax.contiguous().data_ptr(), gsum.contiguous().data_ptr(),
                gout.contiguous().data_ptr(), dl.data_ptr(), N, V,
                vocab_start, cur_stream());
  return dl;
}

}  // namespace

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.def("rmsnorm_fwd", &rmsnorm_fwd);
  m.def("rmsnorm_bwd", &rmsnorm_bwd);
  m.def("swiglu_fwd", &swiglu_fwd);
  m.def("swiglu_bwd", &swiglu_bwd);
  m.def("rope_fwd", &rope_fwd, py::arg("x"), py::arg("cost"), py::arg("sint"),
        py::arg("pos_offset"), py::arg("pos_offset2") = -1);
  m.def("adamw_step", &adamw_step, py::arg("p"), py::arg("g"), py::arg("m"),
        py::arg("v"), py::arg("wd_mask"), py::arg("lr"), py::arg("b1"),
        py::arg("b2"), py::arg("eps"), py::arg("wd"), py::arg("step"),
        py::arg("grad_scale") = py::none(), py::arg("p_bf16") = py::none());
  m.def("flash_attn_fwd_sbuf", &flash_attn_fwd_sbuf, pybind11::arg("q"),
        pybind11::arg("k"), pybind11::arg("v"), pybind11::arg("causal"),
        pybind11::arg("scale"), pybind11::arg("window") = 0);
  m.def("flash_attn_fwd", &flash_attn_fwd, pybind11::arg("q"),
        pybind11::arg("k"), pybind11::arg("v"), pybind11::arg("causal"),
        pybind11::arg("scale"), pybind11::arg("window") = 0);
  m.def("flash_attn_bwd", &flash_attn_bwd, pybind11::arg("dout"),
        pybind11::arg("q"), pybind11::arg("k"), pybind11::arg("v"),
        pybind11::arg("o"), pybind11::arg("lse"), pybind11::arg("causal"),
        pybind11::arg("scale"), pybind11::arg("window") = 0);
  m.def("flash_attn_fwd_range", &flash_attn_fwd_range, pybind11::arg("q"),
        pybind11::arg("k"), pybind11::arg("v"), pybind11::arg("kv_lo"),
        pybind11::arg("kv_hi"), pybind11::arg("causal"),
        pybind11::arg("scale"), pybind11::arg("window") = 0);
  m.def("flash_attn_bwd_range", &flash_attn_bwd_range, pybind11::arg("dout"),
        pybind11::arg("q"), pybind11::arg("k"), pybind11::arg("v"),
        pybind11::arg("o"), pybind11::arg("lse"), pybind11::arg("kv_lo"),
        pybind11::arg("kv_hi"), pybind11::arg("causal"),
        pybind11::arg("scale"), pybind11::arg("window") = 0);
  m.def("flash_attn_fwd_seg", &flash_attn_fwd_seg, pybind11::arg("q"),
        pybind11::arg("k"), pybind11::arg("v"), pybind11::arg("q_start"),
        pybind11::arg("k_end"), pybind11::arg("scale"),
        pybind11::arg("window") = 0);
  m.def("flash_attn_bwd_seg", &flash_attn_bwd_seg, pybind11::arg("dout"),
        pybind11::arg("q"), pybind11::arg("k"), pybind11::arg("v"),
        pybind11::arg("o"), pybind11::arg("lse"), pybind11::arg("q_start"),
        pybind11::arg("k_end"), pybind11::arg("scale"),
        pybind11::arg("window") = 0);
  m.def("flash_attn_fwd_drop", &flash_attn_fwd_drop, pybind11::arg("q"),
        pybind11::arg("k"), pybind11::arg("v"), pybind11::arg("causal"),
        pybind11::arg("scale"), pybind11::arg("window"),
        pybind11::arg("p_drop"), pybind11::arg("seed"),
        pybind11::arg("offset"));
  m.def("flash_attn_bwd_drop", &flash_attn_bwd_drop, pybind11::arg("dout"),
        pybind11::arg("q"), pybind11::arg("k"), pybind11::arg("v"),
        pybind11::arg("o"), pybind11::arg("lse"), pybind11::arg("causal"),
        pybind11::arg("scale"), pybind11::arg("window"),
        pybind11::arg("p_drop"), pybind11::arg("seed"),
        pybind11::arg("offset"));
  m.def("flash_attn_dropout_mask", &flash_attn_dropout_mask,
        pybind11::arg("B"), pybind11::arg("HQ"), pybind11::arg("SQ"),
        pybind11::arg("SKV"), pybind11::arg("p_drop"), pybind11::arg("seed"),
        pybind11::arg("offset"));
  m.def("flash_attn_bwd_sbuf", &flash_attn_bwd_sbuf, pybind11::arg("dout"),
        pybind11::arg("q"), pybind11::arg("k"), pybind11::arg("v"),
        pybind11::arg("o"), pybind11::arg("lse"), pybind11::arg("causal"),
        pybind11::arg("scale"), pybind11::arg("window") = 0);
  m.def("flash_attn_bwd_range_sbuf", &flash_attn_bwd_range_sbuf,
        pybind11::arg("dout"), pybind11::arg("q"), pybind11::arg("k"),
        pybind11::arg("v"), pybind11::arg("o"), pybind11::arg("lse"),
        pybind11::arg("kv_lo"), pybind11::arg("kv_hi"),
        pybind11::arg("causal"), pybind11::arg("scale"),
        pybind11::arg("window") = 0);
  m.def("flash_attn_bwd_seg_sbuf", &flash_attn_bwd_seg_sbuf,
        pybind11::arg("dout"), pybind11::arg("q"), pybind11::arg("k"),
        pybind11::arg("v"), pybind11::arg("o"), pybind11::arg("lse"),
        pybind11::arg("q_start"), pybind11::arg("k_end"),
        pybind11::arg("scale"), pybind11::arg("window") = 0);
  m.def("mfma_probe", &mfma_probe);
  m.def("mfma_probe32", &mfma_probe32);
  m.def("flash_attn_fwd_v3", &flash_attn_fwd_v3, pybind11::arg("q"),
        pybind11::arg("k"), pybind11::arg("v"), pybind11::arg("causal"),
        pybind11::arg("scale"), pybind11::arg("window") = 0);
  m.def("flash_attn_bwd_v3", &flash_attn_bwd_v3, pybind11::arg("dout"),
        pybind11::arg("q"), pybind11::arg("k"), pybind11::arg("v"),
        pybind11::arg("o"), pybind11::arg("lse"), pybind11::arg("causal"),
        pybind11::arg("scale"), pybind11::arg("window") = 0);
  m.def("ce_fwd", &ce_fwd);
  m.def("ce_bwd", &ce_bwd);
  m.def("moe_gemm", &moe_gemm);
  m.def("moe_wgrad", &moe_wgrad);
}
