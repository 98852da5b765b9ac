// Host/device qualifiers + the kernel-launch macro shared by every source of libark355.
//
// Product builds are hipcc for gfx950 only.  ARK_EMUL is a *test-only* configuration
// (tests/emul/, g++): it swaps the HIP runtime for a single-threaded emulator so that kernel and
// orchestration logic can be exercised on a machine without a GPU; it is never shipped or loaded by
// the snark_amd package.
#pragma once
#if defined(ARK_EMUL)
#include "hip_emul.h"
#define ARK_HD inline
#define ARK_HD_NOINLINE __attribute__((noinline))
#define ARK_D inline
#define ARK_LAUNCH(kernel, grid, block, smem, stream, ...) \
  emu::launch((grid), (block), (smem), [&]() { kernel(__VA_ARGS__); })
#define ARK_DYN_SMEM(T, name) T* name = reinterpret_cast<T*>(emu::g_dyn_smem)
// value held by the other lane of this lane's pair (lane ^ 1)
static inline uint32_t ark_pair_xchg(uint32_t v) { return __emu_pair_xchg(v); }
// value held by the even / by the odd lane of this lane's pair, on both lanes.  Built on the exchange: BOTH lanes take part, as
// both lanes of a pair execute the one DPP move on the hardware.
static inline uint32_t __emu_pair_bcast0(uint32_t v) {
  const uint32_t other = __emu_pair_xchg(v);
  return (threadIdx.x & 1u) ? other : v;
}
static inline uint32_t __emu_pair_bcast1(uint32_t v) {
  const uint32_t other = __emu_pair_xchg(v);
  return (threadIdx.x & 1u) ? v : other;
}
static inline uint32_t ark_pair_bcast0(uint32_t v) { return __emu_pair_bcast0(v); }
static inline uint32_t ark_pair_bcast1(uint32_t v) { return __emu_pair_bcast1(v); }
// The two lanes of a pair meet here.  The emulator's lanes are coroutines that run ahead of each other between exchanges; a
// lane that reads its partner's LDS column directly brackets the read with this.
static inline void ark_pair_sync() { (void)__emu_pair_xchg(0u); }
#elif defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define ARK_HD __host__ __device__ __forceinline__
#define ARK_HD_NOINLINE __host__ __device__ __noinline__
#define ARK_D __device__ __forceinline__
#define ARK_LAUNCH(kernel, grid, block, smem, stream, ...) \
  hipLaunchKernelGGL(kernel, (grid), (block), (smem), (stream), __VA_ARGS__)
#define ARK_DYN_SMEM(T, name)                                  \
  extern __shared__ __align__(16) unsigned char _ark_smem[];   \
  T* name = reinterpret_cast<T*>(_ark_smem)
// value held by the other lane of this lane's pair (lane ^ 1): one v_mov_b32_dpp quad_perm:[1,0,3,2]
__device__ __forceinline__ uint32_t ark_pair_xchg(uint32_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
  return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0xB1, 0xF, 0xF, true);   // bound_ctrl: no lane of this pattern reads out of bounds, and with it hipcc needs no v_mov to initialise the destination
#else
  return v;   // never executed on the host pass
#endif
}
// value held by the even (bcast0) / by the odd (bcast1) lane of this lane's pair, on both lanes: one v_mov_b32_dpp
// quad_perm:[0,0,2,2] / quad_perm:[1,1,3,3]
__device__ __forceinline__ uint32_t ark_pair_bcast0(uint32_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
  return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0xA0, 0xF, 0xF, true);
#else
  return v;
#endif
}
__device__ __forceinline__ uint32_t ark_pair_bcast1(uint32_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
  return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0xF5, 0xF, 0xF, true);
#else
  return v;
#endif
}
// the two lanes of a pair are lanes of one wave and execute in lockstep: nothing to do (see the emulator's version above)
__device__ __forceinline__ void ark_pair_sync() {}
#else
// plain host translation unit (no kernels): arithmetic headers only
#define ARK_HD inline
#define ARK_HD_NOINLINE __attribute__((noinline))
#define ARK_D inline
#endif
