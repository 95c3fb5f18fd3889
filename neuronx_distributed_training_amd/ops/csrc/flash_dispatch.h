// Runtime (D, causal, mask, dropout) -> compile-time constants for the flash-attention
// launchers (.hip files only). Each helper calls a generic lambda with
// std::integral_constant arguments; the lambda reads them back with
// decltype(x)::value and names its kernel once. The combinations enumerated
// here are exactly the kernel instantiations that exist: a new head dim,
// mask mode or template flag is added here and nowhere else.
#pragma once

#include <type_traits>

#include "launch.h"

template <int N>
using int_c = std::integral_constant<int, N>;

// f(int_c<D>) for D in {64, 128}; the bindings reject every other D
template <class F>
void dispatch_head_dim(int D, F&& f) {
  if (D == 128) f(int_c<128>{});
  else if (D == 64) f(int_c<64>{});
}

// f(int_c<D>, bool_constant<CAUSAL>): the kernels without mask modes
template <class F>
void dispatch_dense(const FlashArgs& a, F&& f) {
  dispatch_head_dim(a.D, [&](auto d) {
    if (a.causal) f(d, std::true_type{});
    else f(d, std::false_type{});
  });
}

// f(int_c<D>, bool_constant<CAUSAL>, bool_constant<RANGED>,
// bool_constant<SEGMENTED>): D x {dense, ranged} x {causal, non-causal},
// plus segmented, which is causal whatever a.causal says (the kernels
// static_assert against SEGMENTED && !CAUSAL, so it is never instantiated)
template <class F>
void dispatch_flash(const FlashArgs& a, F&& f) {
  if (a.mask == FlashArgs::SEGMENTED)
    dispatch_head_dim(a.D, [&](auto d) {
      f(d, std::true_type{}, std::false_type{}, std::true_type{});
    });
  else
    dispatch_dense(a, [&](auto d, auto c) {
      if (a.mask == FlashArgs::RANGED)
        f(d, c, std::true_type{}, std::false_type{});
      else
        f(d, c, std::false_type{}, std::false_type{});
    });
}

// dispatch_flash plus a fifth argument bool_constant<DROPOUT>, for the three
// kernels with a DROPOUT flag: a.drop_t > 0 adds D x {causal, non-causal}
// with DROPOUT set, DENSE only (the bindings never set drop_t with another
// mask mode, and the kernels static_assert against it)
template <class F>
void dispatch_flash_drop(const FlashArgs& a, F&& f) {
  if (a.drop_t > 0)
    dispatch_dense(a, [&](auto d, auto c) {
      f(d, c, std::false_type{}, std::false_type{}, std::true_type{});
    });
  else
    dispatch_flash(a, [&](auto d, auto c, auto r, auto s) {
      f(d, c, r, s, std::false_type{});
    });
}
