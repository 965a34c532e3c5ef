// error.h — the exception every host unit throws; capi.cpp turns it into a DAC_E* code +
// dac_last_error(). No HIP header, so host-only units (profiler.h) can use it;
// HIP_OK is for the units that do include the HIP runtime.
#pragma once
#include <stdexcept>
#include <string>

#include "../../include/daclip_hip.h"

namespace dac {

struct Error : std::runtime_error {
  int code;
  Error(int c, const std::string& m) : std::runtime_error(m), code(c) {}
};

}  // namespace dac

#define HIP_OK(expr)                                                                      \
  do {                                                                                    \
    hipError_t e_ = (expr);                                                               \
    if (e_ != hipSuccess)                                                                 \
      throw ::dac::Error(DAC_E_HIP, std::string(#expr) + ": " + hipGetErrorString(e_));   \
  } while (0)
