// Error reporting of the C-ABI translation units that call HIP: the thread's
// message (error.h) and the check of a HIP call.
#pragma once

#include <hip/hip_runtime.h>

#include <string>

#include "../../include/isim.h"
#include "error.h"

// returns ISIM_EHIP from the calling function when a HIP call fails
#define ISIM_HIPCHK(expr)                                                                          \
  do {                                                                                             \
    hipError_t e_ = (expr);                                                                        \
    if (e_ != hipSuccess) return isim::set_error(ISIM_EHIP, std::string(#expr) + ": " + hipGetErrorString(e_)); \
  } while (0)
