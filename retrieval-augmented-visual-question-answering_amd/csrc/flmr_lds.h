// One statement of a kernel's dynamic-LDS layout, read by the kernel (region offsets) and by its launcher (`bytes`).
// A layout is a struct next to its kernel: its parameters first, then `flmr_lds c;`, then one member per region, initialised in
// order by c.take<T>(count[, align]) -- default member initialisers run in declaration order, so the struct reads as the carve-up
// -- and `bytes` last.  A per-wave stride (`x_wave`) is a member too, in elements of its region's type (bytes for a char region).
// Two names at one offset are a deliberate alias (then bytes is the larger end).  Usable in constant
// expressions on host and device: layouts whose parameters are compile-time are pinned by static_asserts beside them.
#pragma once
#include <cstddef>

struct flmr_lds {
    size_t bytes = 0;
    // offset of the next region of `count` T's, aligned to `align` bytes; advances past it
    template <typename T>
    __host__ __device__ constexpr size_t take(size_t count, size_t align = alignof(T)) {
        const size_t off = (bytes + align - 1) / align * align;
        bytes = off + count * sizeof(T);
        return off;
    }
};

// The pointer of the region at offset `to` from the typed pointer of the region before it (at `from`): for layouts whose offsets are
// runtime values.  The element-typed step is the address chain a hand carve-up gives the compiler, and the dense stage-1 kernels'
// register allocation depends on it (as `smem + offset` s1_image_kernel's SGPR spill counts moved).
template <typename T, typename P>
__device__ __forceinline__ T* flmr_lds_next(P* prev, size_t from, size_t to) { return reinterpret_cast<T*>(prev + (to - from) / sizeof(P)); }

#define FLMR_LDS_CU_BYTES (160 * 1024)   // LDS of one gfx950 CU: `n` workgroups are co-resident only if n * (dynamic + static) fits
