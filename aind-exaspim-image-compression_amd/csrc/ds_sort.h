// ds_sort.h -- the fixed compare-exchange networks the mode reductions of the pyramid kernels sort a window's 4 or 8
// values with, in registers.  T is an UNSIGNED integer type: uint32_t (the uint16 counts and the
// 32-bit ids) or uint64_t (the 64-bit ids, compared whole).
#pragma once
#include <cstdint>
#include <type_traits>

#include <hip/hip_runtime.h>

namespace exabm4d {

template <typename T, int N>
__device__ __forceinline__ void ds_sort(T (&v)[N]) {
    static_assert(std::is_unsigned<T>::value, "values compare as unsigned integers");
#define DS_CE(a, b)                                  \
    {                                                \
        const T lo = min(v[a], v[b]);                \
        v[b] = max(v[a], v[b]);                      \
        v[a] = lo;                                   \
    }
    if constexpr (N == 8) {                          // 19 compare-exchanges, 6 layers
        DS_CE(0, 2) DS_CE(1, 3) DS_CE(4, 6) DS_CE(5, 7)
        DS_CE(0, 4) DS_CE(1, 5) DS_CE(2, 6) DS_CE(3, 7)
        DS_CE(0, 1) DS_CE(2, 3) DS_CE(4, 5) DS_CE(6, 7)
        DS_CE(2, 4) DS_CE(3, 5)
        DS_CE(1, 4) DS_CE(3, 6)
        DS_CE(1, 2) DS_CE(3, 4) DS_CE(5, 6)
    } else {
        static_assert(N == 4, "windows of 4 or 8 values");
        DS_CE(0, 1) DS_CE(2, 3)
        DS_CE(0, 2) DS_CE(1, 3)
        DS_CE(1, 2)
    }
#undef DS_CE
}

}  // namespace exabm4d
