// Host stand-in for <hip/hip_runtime.h>: lets tests/host/onevar_selftest.cpp compile the device headers of the one-variable solver
// (csrc/onevar.h, philox.h, cd_phase1_sep.h) as plain C++.  Empty qualifiers and the two standard headers, nothing else.
#pragma once
#include <cmath>
#include <cstdint>
#define __device__
#define __host__
#define __global__
