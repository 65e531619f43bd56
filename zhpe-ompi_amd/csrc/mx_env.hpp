// mx_env.hpp -- the two forms of on/off environment switch (MX_*).  Each
// reads the variable when called; a switch function caches its own value
// once per process (`static const bool v = env_default_on("MX_...")`).
#pragma once
#include <stdlib.h>

namespace mx {
// default on: a value whose first character is '0' turns it off
inline bool env_default_on(const char *name) {
  const char *e = getenv(name);
  return !(e && *e == '0');
}
// default off: a value whose first character is '1' turns it on
inline bool env_default_off(const char *name) {
  const char *e = getenv(name);
  return e && *e == '1';
}
}  // namespace mx
