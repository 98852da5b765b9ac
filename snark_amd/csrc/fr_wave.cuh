// An Fr across the lanes of a wave (wave64) and the waves of a workgroup: what poly_impl.cuh, evals_impl.cuh, sumcheck_impl.cuh
// and colgather_impl.cuh share, and the dispatch on the elements a lane owns.
#pragma once
#include "hd.h"

namespace ark355 {

template <class Fr>
ARK_D Fr fr_shfl_down(const Fr& v, uint32_t delta) {
  Fr o;
#pragma unroll
  for (int i = 0; i < Fr::N; i++) o.l[i] = (uint32_t)__shfl_down((int)v.l[i], delta, 64);
  return o;
}
template <class Fr>
ARK_D Fr fr_shfl_xor(const Fr& v, uint32_t mask) {
  Fr o;
#pragma unroll
  for (int i = 0; i < Fr::N; i++) o.l[i] = (uint32_t)__shfl_xor((int)v.l[i], (int)mask, 64);
  return o;
}

// the sum over the wave, in every lane: a butterfly of six exchanges
template <class Fr>
ARK_D Fr fr_wave_sum(Fr v) {
  for (uint32_t mask = 32; mask >= 1; mask >>= 1) v = Fr::add(v, fr_shfl_xor(v, mask));
  return v;
}

// lane value -> the sum over the `waves` waves of the workgroup in out[0], stored by thread 0: six shuffle steps, the wave values
// through buf (LDS; a caller that comes back before every lane has left passes another buffer in turn), one barrier
template <class Fr>
ARK_D void fr_group_sum(Fr v, uint32_t (*buf)[Fr::N], uint32_t waves, Fr* out) {
  const uint32_t tid = threadIdx.x;
#pragma unroll
  for (uint32_t s = 0; s < 6; s++) v = Fr::add(v, fr_shfl_down(v, 1u << s));
  if ((tid & 63u) == 0) {
#pragma unroll
    for (int i = 0; i < Fr::N; i++) buf[tid >> 6][i] = v.l[i];
  }
  __syncthreads();
  if (tid == 0) {
    for (uint32_t w = 1; w < waves; w++) {
      Fr o;
#pragma unroll
      for (int i = 0; i < Fr::N; i++) o.l[i] = buf[w][i];
      v = Fr::add(v, o);
    }
    *out = v;
  }
}

// CALL with PE = the E (1 .. 8) elements a lane owns as a compile-time constant
#define ARK_BY_E(E_, CALL)                          \
  switch (E_) {                                     \
    case 1: { constexpr int PE = 1; CALL; } break;  \
    case 2: { constexpr int PE = 2; CALL; } break;  \
    case 3: { constexpr int PE = 3; CALL; } break;  \
    case 4: { constexpr int PE = 4; CALL; } break;  \
    case 5: { constexpr int PE = 5; CALL; } break;  \
    case 6: { constexpr int PE = 6; CALL; } break;  \
    case 7: { constexpr int PE = 7; CALL; } break;  \
    default: { constexpr int PE = 8; CALL; } break; \
  }

}  // namespace ark355
