// Error reporting shared by the C-ABI entry points (thread-local last error).
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>

int stif_fail(int code, const char* msg);
int stif_check_launch(const char* where);
// compute units of the current device (cached; 256 if the query fails) -- persistent-grid sizing
int stif_num_cus();

// The per-set item table of a launch (stif.h STIF_MAX_GROUPS), checked and put into the form the kernels scan
// (set_item_of), in place in the launcher's copy of the arguments: tab[g] = first item of set g, tab[ngroups] = the
// launch's items, every entry past it INT_MAX.  An all-zero table is filled with the uniform `nitems` per set.
// *total = items of the launch, *most = the largest set.  STIF_E_INVALID (message prefixed by `who`): ngroups
// outside [1, STIF_MAX_GROUPS], a table that does not start at 0 or does not increase, nitems < 1 in the uniform
// form, more than INT_MAX items.
int stif_item_table(const char* who, int ngroups, int nitems, int* tab, long long* total, int* most);

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
