// Host stand-in for <hip/hip_runtime.h>: lets tools/check_geom_edges.cpp compile the device headers that include it
// (folddisco_amd/csrc/fd_device.h, fd_geom_other.h, and with -D__HIPCC__ the speculative section of fd_geom.h) with a plain C++ compiler,
// so that their __device__ functions run on the CPU.  The few device instructions they use are emulated: v_alignbit and v_med3 exactly,
// v_rsq_f32 / v_sqrt_f32 (1 ulp on the device) by the correctly rounded value — one of the values the error bounds of fd_geom.h admit.
#pragma once
#include <math.h>
#include <stdint.h>
#define __device__
#define __host__
#define __forceinline__ inline
#define __builtin_amdgcn_fence(order, scope) ((void)0)
#define __builtin_amdgcn_wave_barrier() ((void)0)
#define __builtin_amdgcn_mbcnt_lo(mask, v) (0u)
#define __builtin_amdgcn_mbcnt_hi(mask, v) (0u)
static inline uint32_t fd_host_alignbit(uint32_t hi, uint32_t lo, uint32_t s) { return (uint32_t)((((uint64_t)hi << 32) | lo) >> (s & 31u)); }
static inline float fd_host_rsq(float x) { return (float)(1.0 / sqrt((double)x)); }
static inline float fd_host_med3(float a, float b, float c) { return fmaxf(fminf(a, b), fminf(fmaxf(a, b), c)); }
#define __builtin_amdgcn_alignbit(hi, lo, s) fd_host_alignbit(hi, lo, s)
#define __builtin_amdgcn_rsqf(x) fd_host_rsq(x)
#define __builtin_amdgcn_sqrtf(x) sqrtf(x)
#define __builtin_amdgcn_fmed3f(a, b, c) fd_host_med3(a, b, c)
