// What the knob table (knobs.h) generates: the constructor that reads
// UMAMD_TUNING, umamd::knobs() and the C-ABI setter.
#include "common.h"

#include <stdlib.h>

#include "knobs.h"

namespace umamd {

// the value of `key` in UMAMD_TUNING="key=value,key=value", else dflt
static int tuning_env(const char* key, int dflt) {
  const char* v = getenv("UMAMD_TUNING");
  if (v == nullptr) return dflt;
  const size_t n = strlen(key);
  for (const char* p = v; *p;) {
    if (!strncmp(p, key, n) && p[n] == '=') return (int)atol(p + n + 1);
    p = strchr(p, ',');
    if (p == nullptr) break;
    ++p;
  }
  return dflt;
}

Knobs::Knobs() {
#define UM_KNOB_READ(name, dflt) name = tuning_env(#name, dflt);
  UM_KNOBS(UM_KNOB_READ)
#undef UM_KNOB_READ
}

Knobs& knobs() {
  static Knobs k;
  return k;
}

}  // namespace umamd

// tuning keys at run time (tests force code paths; sweeps): returns the old
// value, or -1 for an unknown key
extern "C" int um_set_tuning(const char* key, int value) {
  static const struct {
    const char* name;
    int umamd::Knobs::*field;
  } table[] = {
#define UM_KNOB_ROW(name, dflt) {#name, &umamd::Knobs::name},
      UM_KNOBS(UM_KNOB_ROW)
#undef UM_KNOB_ROW
  };
  for (const auto& row : table)
    if (!strcmp(key, row.name)) {
      int& f = umamd::knobs().*row.field;
      const int old = f;
      f = value;
      return old;
    }
  return -1;
}
