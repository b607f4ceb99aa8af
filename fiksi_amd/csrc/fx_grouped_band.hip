// The one-structure build's two-column f64 kernel (fx_grouped_c.hip: lm_solve_grouped_c_kernel) with a band factor: the register
// Cholesky compiled for a row profile of half-band W plus B dense last rows (fx_grouped_rows.h: RBand), which leaves out the
// updates of the rows where L(i, K) is a structural zero and the loads of matrix elements no lane holds a non-zero of. Same
// operations on the same operands otherwise, so the same bits. The host picks the cheapest build whose band and
// border hold the structure's factor (fx_programs.cpp: build_gc_program; fx_device.h: GC_BANDS) — ring16 in its column order is
// a band of half-width 5 and four dense rows of the closing constraints.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fx_device.h"
#include "fx_grouped_c.h"

namespace fx {

template <int W, int B>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(2, 2))) void lm_solve_grouped_c_band_kernel(
    DeviceBatch b, LmParams prm, GcLayout L, uint32_t* __restrict__ next_system) {
    extern __shared__ __align__(16) unsigned char smem[];
    grouped_c_body<2, 2, double, W, B>(b, prm, L, next_system, smem);
}
// ... with the set-up staged before it and the closing check after it (fx_grouped_c.hip: gc_stage_kernel, gc_close_kernel)
template <int W, int B>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(2, 2))) void lm_solve_grouped_c_band_staged_kernel(
    DeviceBatch b, LmParams prm, GcLayout L, uint32_t* __restrict__ next_system) {
    extern __shared__ __align__(16) unsigned char smem[];
    grouped_c_body<2, 2, double, W, B, true>(b, prm, L, next_system, smem);
}

static_assert(GC_NBANDS == 3 && GC_BANDS[0].w == 5 && GC_BANDS[0].b == 0 && GC_BANDS[1].w == 5 && GC_BANDS[1].b == 4 &&
                  GC_BANDS[2].w == 5 && GC_BANDS[2].b == 6,
              "one kernel per GC_BANDS entry, in its order");

GcBuild gc_band_build(uint32_t band, bool staged) {
    static unsigned int r[2 * GC_NBANDS] = {0};
    if (staged) {
        switch (band) {
            case 1: return {&lm_solve_grouped_c_band_staged_kernel<5, 0>, &r[3], 8u};
            case 2: return {&lm_solve_grouped_c_band_staged_kernel<5, 4>, &r[4], 8u};
            case 3: return {&lm_solve_grouped_c_band_staged_kernel<5, 6>, &r[5], 8u};
            default: return {nullptr, nullptr, 0u};
        }
    }
    switch (band) {
        case 1: return {&lm_solve_grouped_c_band_kernel<5, 0>, &r[0], 8u};
        case 2: return {&lm_solve_grouped_c_band_kernel<5, 4>, &r[1], 8u};
        case 3: return {&lm_solve_grouped_c_band_kernel<5, 6>, &r[2], 8u};
        default: return {nullptr, nullptr, 0u};
    }
}

}  // namespace fx
