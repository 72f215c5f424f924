// Test-only stand-in for <hip/hip_runtime.h>: lets the host/device core headers that include it
// unconditionally compile as plain C++ (tests/cpp/initializer_core_main.cpp, -Itests/cpp/hipstub).
#pragma once
#define __host__
#define __device__
#define __forceinline__ inline
