// hip/hip_runtime.h for tests/hostcheck/adam_hostcheck.cpp ONLY (g++ -Itests/hostcheck/hip_host): just what csrc/shems_adam.h needs to
// compile on the host -- the function qualifiers as nothing, and the hardware's Float64 reciprocal estimate.
#pragma once
#include <cmath>

#define __device__
#define __host__
#define __forceinline__ inline __attribute__((always_inline))

// v_rcp_f64 returns an ESTIMATE that adam_math refines (two Newton steps and a residual correction).  The host stands in with a worse
// one, good to fp32 only, so that the refinement is what the check exercises: 2^-24 -> 2^-48 -> 2^-96 relative.
static inline double shems_hostcheck_rcp(double x) { return (double)(1.0f / (float)x); }
#define __builtin_amdgcn_rcp(x) shems_hostcheck_rcp(x)
