// Error reporting shared by the C-ABI entry points (thread-local last error).
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>

int stif_fail(int code, const char* msg);
int stif_check_launch(const char* where);
// compute units of the current device (cached; 256 if the query fails) -- persistent-grid sizing
int stif_num_cus();

// A runtime bool as a template argument: f(std::true_type{}) or f(std::false_type{})
template <class F>
void with_bool(bool v, F&& f) {
  if (v) f(std::true_type{});
  else f(std::false_type{});
}
// A runtime int as a template argument, over the values it may take: f(std::integral_constant<int, V>{}) for
// the V that equals v; false (f not called) if none does
template <int... Vs, class F>
bool with_int(int v, F&& f) {
  return ((v == Vs && (f(std::integral_constant<int, Vs>{}), true)) || ...);
}
