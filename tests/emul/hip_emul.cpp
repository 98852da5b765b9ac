// TEST INFRASTRUCTURE ONLY -- scheduler of the HIP emulator (see hip_emul.h).
#include "hip_emul.h"
#include <map>
#include <mutex>

namespace emu {
dim3 g_threadIdx, g_blockIdx, g_blockDim, g_gridDim;
Thread* g_cur = nullptr;
void* g_sched_sp = nullptr;
uint64_t g_xchg[64];
unsigned char* g_dyn_smem = nullptr;
PairBox g_pairbox[1024];

static const std::function<void()>* g_body = nullptr;
static const size_t STACK = 1 << 20;
static std::vector<char*> g_stacks;

// Register-only context switch (System V x86-64): push the callee-saved registers, swap stack pointers, pop, return.
// No signal mask, no floating-point environment: the coroutines are plain integer / SSE code of one thread.
#if !defined(__x86_64__)
#error "the HIP emulator's context switch is written for x86-64"
#endif
extern "C" void emu_switch(void** save_sp, void* load_sp);
asm(R"(
    .text
    .globl emu_switch
    .type emu_switch, @function
emu_switch:
    pushq %rbp
    pushq %rbx
    pushq %r12
    pushq %r13
    pushq %r14
    pushq %r15
    movq %rsp, (%rdi)
    movq %rsi, %rsp
    popq %r15
    popq %r14
    popq %r13
    popq %r12
    popq %rbx
    popq %rbp
    ret
    .size emu_switch, .-emu_switch
)");

void yield(int st) {
  Thread* me = g_cur;
  me->state = st;
  emu_switch(&me->sp, g_sched_sp);
}

static void trampoline() {
  (*g_body)();
  g_cur->state = DONE;
  emu_switch(&g_cur->sp, g_sched_sp);
  abort();                               // a finished coroutine is never resumed
}

static void resume(Thread& t) {
  g_cur = &t;
  g_threadIdx = t.tid;
  emu_switch(&g_sched_sp, t.sp);
}

// a fresh coroutine: six zeroed callee-saved registers, then the address emu_switch "returns" to; the slot above it is where a
// caller's return address would sit, so that the entry sees the stack alignment the ABI promises (rsp = 16 k + 8)
static void* fresh_stack(char* stack, size_t size) {
  uintptr_t top = ((uintptr_t)stack + size) & ~(uintptr_t)15;
  void** sp = reinterpret_cast<void**>(top);
  *--sp = nullptr;                                  // (fake return address of the trampoline)
  *--sp = reinterpret_cast<void*>(&trampoline);
  for (int i = 0; i < 6; i++) *--sp = nullptr;      // rbp rbx r12 r13 r14 r15
  return sp;
}

void launch(dim3 grid, dim3 block, size_t smem, const std::function<void()>& body) {
  const unsigned nthreads = block.x * block.y * block.z;
  if (nthreads == 0 || grid.x * grid.y * grid.z == 0) return;
  g_body = &body;
  g_blockDim = block;
  g_gridDim = grid;
  while (g_stacks.size() < nthreads) g_stacks.push_back((char*)malloc(STACK));
  std::vector<Thread> th(nthreads);
  std::vector<unsigned char> dyn(smem + 64);
  g_dyn_smem = dyn.data();
  for (unsigned bz = 0; bz < grid.z; bz++)
    for (unsigned by = 0; by < grid.y; by++)
      for (unsigned bx = 0; bx < grid.x; bx++) {
        g_blockIdx = dim3(bx, by, bz);
        unsigned k = 0;
        for (unsigned tz = 0; tz < block.z; tz++)
          for (unsigned ty = 0; ty < block.y; ty++)
            for (unsigned tx = 0; tx < block.x; tx++, k++) {
              Thread& t = th[k];
              t.sp = fresh_stack(g_stacks[k], STACK);
              t.state = RUN;
              t.tid = dim3(tx, ty, tz);
              g_pairbox[k % 1024] = PairBox();
            }
        const unsigned nwaves = (nthreads + 63) / 64;
        for (;;) {
          bool any_run = false;
          for (unsigned w = 0; w < nwaves; w++) {
            const unsigned lo = w * 64, hi = (lo + 64 < nthreads) ? lo + 64 : nthreads;
            for (;;) {
              bool ran = false;
              for (unsigned i = lo; i < hi; i++)
                if (th[i].state == RUN) {
                  resume(th[i]);
                  ran = true;
                }
              // lanes that yielded with RUN (pair exchange polling) are simply resumed on the next pass
              bool any_running = false, any_wave_wait = false;
              for (unsigned i = lo; i < hi; i++) {
                any_running |= (th[i].state == RUN);
                any_wave_wait |= (th[i].state == WAVE_WAIT);
              }
              if (any_running) {
                if (!ran) break;
                continue;
              }
              if (!any_wave_wait) break;
              for (unsigned i = lo; i < hi; i++)
                if (th[i].state == WAVE_WAIT) th[i].state = RUN;
            }
            for (unsigned i = lo; i < hi; i++) any_run |= (th[i].state == RUN);
          }
          if (any_run) continue;
          bool any_block_wait = false;
          for (unsigned i = 0; i < nthreads; i++) any_block_wait |= (th[i].state == BLOCK_WAIT);
          if (!any_block_wait) break;
          for (unsigned i = 0; i < nthreads; i++)
            if (th[i].state == BLOCK_WAIT) th[i].state = RUN;
        }
      }
  g_dyn_smem = nullptr;
  mem_check();                           // a kernel that stored past a buffer fails the launch check that follows it
}

// ---- allocator (see hip_emul.h) ---------------------------------------------------------------------------------------
// Layout of one block: [GUARD_FRONT bytes POISON_GUARD][body, n bytes][GUARD_BACK bytes POISON_GUARD]; the body is what the
// caller sees.  The registry is locked: the ranks of a multi-GPU test are threads of one process.
namespace {
std::mutex g_mem_mu;
std::map<char*, size_t> g_live;          // body -> size
hipError_t g_pending = hipSuccess;
char g_mem_msg[256] = "no guard-band error";

// first byte of [p, p + n) that is not `v`, or n
size_t first_not(const unsigned char* p, size_t n, unsigned char v) {
  uint64_t w;
  memset(&w, v, sizeof(w));
  size_t i = 0;
  for (; i + 8 <= n; i += 8) {
    uint64_t x;
    memcpy(&x, p + i, 8);
    if (x != w) break;
  }
  for (; i < n; i++)
    if (p[i] != v) return i;
  return n;
}

// locked.  Reports the first damaged band only while no error is pending, repairs every damaged band.
void check_block(char* body, size_t n) {
  unsigned char* front = reinterpret_cast<unsigned char*>(body) - GUARD_FRONT;
  unsigned char* back = reinterpret_cast<unsigned char*>(body) + n;
  const size_t f = first_not(front, GUARD_FRONT, POISON_GUARD), b = first_not(back, GUARD_BACK, POISON_GUARD);
  if (f == GUARD_FRONT && b == GUARD_BACK) return;
  if (g_pending == hipSuccess) {
    g_pending = hipErrorEmuGuardBand;
    if (b != GUARD_BACK)
      snprintf(g_mem_msg, sizeof(g_mem_msg), "emulator: guard band AFTER an allocation of %zu bytes damaged, first at byte %zu past its end",
               n, b);
    else {
      size_t last = GUARD_FRONT;         // the damaged byte nearest to the body says how far before it the store went
      while (last > 0 && front[last - 1] == POISON_GUARD) last--;
      snprintf(g_mem_msg, sizeof(g_mem_msg), "emulator: guard band BEFORE an allocation of %zu bytes damaged, nearest at byte %zu before its start",
               n, GUARD_FRONT - last + 1);
    }
  }
  memset(front, POISON_GUARD, GUARD_FRONT);
  memset(back, POISON_GUARD, GUARD_BACK);
}
}  // namespace

hipError_t mem_alloc(void** p, size_t n) {
  *p = nullptr;
  if (n == 0) n = 1;
  void* raw = nullptr;
  if (n > SIZE_MAX - GUARD_FRONT - GUARD_BACK || posix_memalign(&raw, 256, GUARD_FRONT + n + GUARD_BACK) != 0) return hipErrorOutOfMemory;
  char* body = static_cast<char*>(raw) + GUARD_FRONT;
  memset(raw, POISON_GUARD, GUARD_FRONT);
  memset(body, POISON_FRESH, n);
  memset(body + n, POISON_GUARD, GUARD_BACK);
  std::lock_guard<std::mutex> lk(g_mem_mu);
  g_live[body] = n;
  *p = body;
  return hipSuccess;
}

hipError_t mem_free(void* p) {
  if (!p) return hipSuccess;
  std::lock_guard<std::mutex> lk(g_mem_mu);
  auto it = g_live.find(static_cast<char*>(p));
  if (it == g_live.end()) return hipErrorInvalidValue;          // not ours, or freed twice: left alone
  check_block(it->first, it->second);
  memset(it->first, POISON_FREED, it->second);
  free(it->first - GUARD_FRONT);
  g_live.erase(it);
  return g_pending;                      // stays pending: the library's destructors ignore what hipFree returns
}

void mem_check() {
  std::lock_guard<std::mutex> lk(g_mem_mu);
  for (auto& kv : g_live) check_block(kv.first, kv.second);
}

hipError_t mem_report() {
  mem_check();
  std::lock_guard<std::mutex> lk(g_mem_mu);
  const hipError_t e = g_pending;
  g_pending = hipSuccess;
  return e;
}

hipError_t mem_peek() {
  mem_check();
  std::lock_guard<std::mutex> lk(g_mem_mu);
  return g_pending;
}

// the ranks of a multi-GPU test are threads: the caller gets its own copy, taken under the lock that guards the writer
const char* mem_error_string() {
  static thread_local char mine[sizeof(g_mem_msg)];
  std::lock_guard<std::mutex> lk(g_mem_mu);
  memcpy(mine, g_mem_msg, sizeof(mine));
  return mine;
}
}  // namespace emu
