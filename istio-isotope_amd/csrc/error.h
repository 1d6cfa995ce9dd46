// The thread's error slot (isim_last_error): every C-ABI translation unit
// reports through it.  No HIP header: host-only sources include this alone.
#pragma once

#include <string>

namespace isim {
int set_error(int code, const std::string &msg);  // api.hip; returns code
}
