// kernel_stamps.h -- cycle stamps of the diagnostic builds (-DEXABM4D_STAMPS: the stage kernels, tools/dbg/stamps.py;
// -DEXABM4D_BM_STAMPS: bm_tile16_kernel, tools/dbg/bm_stamps.py).  A kernel sums (b) - (a) into its own `st[]`; the
// counters, what their slots mean and the read-out functions are in the kernel's file.  A variant build passes its
// switches to every file, so a kernel's file defines KERNEL_STAMPS under its own switch before it includes this:
// one kernel's stamps stay off in the other's file, which declares no `st[]` then.  Empty in every other build.
#pragma once

#ifdef KERNEL_STAMPS
namespace exabm4d {
__device__ __forceinline__ unsigned long long stamp() {
    unsigned long long t;
    __builtin_amdgcn_sched_barrier(0);
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t)::"memory");
    __builtin_amdgcn_sched_barrier(0);
    return t;
}
}  // namespace exabm4d
#define STAMP(var) const unsigned long long var = stamp()
#define STAMP_ADD(i, a, b) st[i] += (b) - (a)
#define STAMP_MOVE(i, j, a, b) (st[i] += (b) - (a), st[j] -= (b) - (a))
#else
#define STAMP(var)
#define STAMP_ADD(i, a, b)
#define STAMP_MOVE(i, j, a, b) (void)0
#endif
