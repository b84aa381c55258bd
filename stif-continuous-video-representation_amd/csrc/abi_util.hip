#include <stdio.h>
#include <string.h>

#include "abi_util.h"
#include "stif.h"

static thread_local char g_err[512] = "";

int stif_fail(int code, const char* msg) {
  snprintf(g_err, sizeof(g_err), "%s", msg);
  return code;
}

int stif_check_launch(const char* where) {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    snprintf(g_err, sizeof(g_err), "%s: %s", where, hipGetErrorString(e));
    return STIF_E_LAUNCH;
  }
  return STIF_OK;
}

extern "C" const char* stif_last_error(void) { return g_err; }
extern "C" const char* stif_version(void) { return "stif_hip 0.1 gfx950"; }

int stif_item_table(const char* who, int ngroups, int nitems, int* tab, long long* total, int* most) {
  char msg[160];
  auto bad = [&](const char* why) {
    snprintf(msg, sizeof(msg), "%s: %s", who, why);
    return stif_fail(STIF_E_INVALID, msg);
  };
  if (ngroups < 1 || ngroups > STIF_MAX_GROUPS) return bad("bad ngroups (1 .. STIF_MAX_GROUPS weight sets)");
  bool uniform = true;
  for (int i = 0; i <= STIF_MAX_GROUPS; ++i) uniform &= tab[i] == 0;
  if (uniform) {
    if (nitems < 1) return bad("bad nitems");
    if ((long long)ngroups * nitems > 0x7fffffffLL) return bad("too many items");
    for (int g = 0; g <= ngroups; ++g) tab[g] = g * nitems;
  } else {
    if (tab[0] != 0) return bad("item_base must start at 0");
    for (int g = 0; g < ngroups; ++g)
      if (tab[g + 1] <= tab[g]) return bad("item_base must increase (no empty set)");
  }
  *most = 0;
  for (int g = 0; g < ngroups; ++g) *most = tab[g + 1] - tab[g] > *most ? tab[g + 1] - tab[g] : *most;
  *total = tab[ngroups];
  for (int i = ngroups + 1; i <= STIF_MAX_GROUPS; ++i) tab[i] = 0x7fffffff;
  return STIF_OK;
}

int stif_num_cus() {
  static int n = 0;
  if (!n) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0)
      n = 256;
  }
  return n;
}
