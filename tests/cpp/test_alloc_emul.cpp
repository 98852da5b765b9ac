// CPU tier: the emulator's allocator (tests/emul/hip_emul.h) on its own -- poison on allocation and on free, guard bands on both
// sides, a damaged band as a pending error that is handed out once and names the allocation, never an abort.  Plain host program:
// built with an address sanitizer by tests/test_emul_alloc.py when the compiler has one.
#include <stdio.h>
#include <string.h>
#include "hip_emul.h"

static int g_fail = 0;
#define EXPECT(cond)                                                   \
  do {                                                                 \
    if (!(cond)) {                                                     \
      printf("FAILED line %d: %s\n", __LINE__, #cond);                 \
      g_fail++;                                                        \
    }                                                                  \
  } while (0)

static bool all_bytes(const unsigned char* p, size_t n, unsigned char v) {
  for (size_t i = 0; i < n; i++)
    if (p[i] != v) return false;
  return true;
}

static void store_kernel(unsigned char* p, long at, unsigned char v) {
  if (threadIdx.x == 0 && blockIdx.x == 0) p[at] = v;
}

int main() {
  // fresh memory is poisoned, aligned, and sits between two bands; sizes around the word loop of the band check
  for (size_t n : {(size_t)1, (size_t)7, (size_t)64, (size_t)1000, (size_t)(1 << 20) + 3}) {
    unsigned char* p = nullptr;
    EXPECT(hipMalloc(&p, n) == hipSuccess && p);
    EXPECT(((uintptr_t)p & 255) == 0);
    EXPECT(all_bytes(p, n, emu::POISON_FRESH));
    EXPECT(all_bytes(p - emu::GUARD_FRONT, emu::GUARD_FRONT, emu::POISON_GUARD));
    EXPECT(all_bytes(p + n, emu::GUARD_BACK, emu::POISON_GUARD));
    memset(p, 0, n);                                   // the whole body is the caller's
    EXPECT(hipDeviceSynchronize() == hipSuccess);
    EXPECT(hipFree(p) == hipSuccess);
    EXPECT(hipGetLastError() == hipSuccess);
  }
  unsigned char* h = nullptr;
  EXPECT(hipHostMalloc((void**)&h, 100, hipHostMallocDefault) == hipSuccess && all_bytes(h, 100, emu::POISON_FRESH));
  EXPECT(hipHostFree(h) == hipSuccess);
  EXPECT(hipFree(nullptr) == hipSuccess);

  unsigned char *a = nullptr, *b = nullptr;
  EXPECT(hipMalloc(&a, 1000) == hipSuccess && hipMalloc(&b, 48) == hipSuccess);
  // a kernel stores one byte past the end of `a`: the launch check that follows reports it, once, and names the size
  emu::launch(dim3(2), dim3(64), 0, [&]() { store_kernel(a, 1000, 0); });
  EXPECT(hipPeekAtLastError() == hipErrorEmuGuardBand);
  EXPECT(hipGetLastError() == hipErrorEmuGuardBand);
  EXPECT(strstr(hipGetErrorString(hipErrorEmuGuardBand), "AFTER an allocation of 1000 bytes") != nullptr);
  EXPECT(strstr(hipGetErrorString(hipErrorEmuGuardBand), "byte 0 past") != nullptr);
  EXPECT(hipGetLastError() == hipSuccess);             // handed out once; the band was repaired
  EXPECT(hipDeviceSynchronize() == hipSuccess);
  // the last byte of the back band, by an asynchronous fill that overruns: pending until a synchronisation
  EXPECT(hipMemsetAsync(b + 40, 0, 8 + emu::GUARD_BACK, nullptr) == hipSuccess);
  EXPECT(hipStreamSynchronize(nullptr) == hipErrorEmuGuardBand);
  EXPECT(strstr(hipGetErrorString(hipErrorEmuGuardBand), "AFTER an allocation of 48 bytes") != nullptr);
  EXPECT(hipStreamSynchronize(nullptr) == hipSuccess);
  // one byte before the start
  emu::launch(dim3(1), dim3(1), 0, [&]() { store_kernel(b, -1, 7); });
  EXPECT(hipGetLastError() == hipErrorEmuGuardBand);
  EXPECT(strstr(hipGetErrorString(hipErrorEmuGuardBand), "BEFORE an allocation of 48 bytes") != nullptr);
  EXPECT(strstr(hipGetErrorString(hipErrorEmuGuardBand), "byte 1 before") != nullptr);
  // the far end of the front band
  emu::launch(dim3(1), dim3(1), 0, [&]() { store_kernel(b, -(long)emu::GUARD_FRONT, 7); });
  EXPECT(hipGetLastError() == hipErrorEmuGuardBand);
  // damage found only by hipFree (a plain host store, no launch after it) stays pending for the next check: the library's
  // destructors ignore what hipFree returns
  a[1000 + emu::GUARD_BACK - 1] = 1;
  EXPECT(hipFree(a) == hipErrorEmuGuardBand);
  EXPECT(hipGetLastError() == hipErrorEmuGuardBand);
  EXPECT(hipGetLastError() == hipSuccess);
  // a synchronous copy reports its own overrun
  unsigned char src[64] = {0};
  EXPECT(hipMemcpy(b, src, 49, hipMemcpyHostToDevice) == hipErrorEmuGuardBand);
  EXPECT(hipMemcpy(b, src, 48, hipMemcpyHostToDevice) == hipSuccess);
  EXPECT(hipFree(b) == hipSuccess);
  EXPECT(hipFree(b) == hipErrorInvalidValue);          // not live any more: refused, nothing is freed twice
  if (g_fail) return 1;
  printf("emulator allocator: all cases agree\n");
  return 0;
}
