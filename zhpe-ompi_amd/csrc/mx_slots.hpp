// mx_slots.hpp -- the (op, type) slots the data path serves (host only, no
// HIP).  The public mx_op_supported / mx_type_size answer for the reference
// configuration the table variants name; the two binary16 slots
// (MX_TABLE_SHORT_FLOAT) are outside variants 0 and 1, so the library's own
// gates and element sizes go through these instead.
#pragma once
#include <stddef.h>

#include "../../include/mx_kernels.h"

namespace mx {

// element size of a slot, the binary16 slots included; 0 if none
inline size_t type_size(int t) {
  return t == MX_TYPE_SHORT_FLOAT ? 2 : t == MX_TYPE_C_SHORT_FLOAT_COMPLEX ? 4 : mx_type_size(t);
}

// (op, type) has a kernel in the widest table this library builds
inline bool op_has_kernel(int op, int type) {
  return mx_op_supported(op, type, MX_TABLE_WITH_FORTRAN | MX_TABLE_SHORT_FLOAT) != 0;
}

}  // namespace mx
