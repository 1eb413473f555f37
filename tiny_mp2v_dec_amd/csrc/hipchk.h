// hipchk.h — HIPCHK: a failed HIP call becomes MP2VG_E_HIP with the call's text in mp2vg_last_error
#pragma once
#include <hip/hip_runtime.h>

#include <string>

#include "syntax.h"

#define HIPCHK(expr)                                                                       \
    do {                                                                                   \
        hipError_t e_ = (expr);                                                            \
        if (e_ != hipSuccess) {                                                            \
            mp2vg::set_error(std::string(#expr) + ": " + hipGetErrorString(e_));           \
            return MP2VG_E_HIP;                                                            \
        }                                                                                  \
    } while (0)
