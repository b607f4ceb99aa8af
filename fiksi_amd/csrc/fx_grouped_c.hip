// Grouped fused solve, the build for batches of ONE structure (gfx950, wave64): four Systems per wavefront as in
// fx_grouped.hip — same algorithm, same arithmetic on the same operands, same order of every sum and of every addition
// into the normal equations, so the same bits (reference: fiksi/src/assemble/mod.rs:46-167, fiksi/src/solve/lm.rs:21-193) —
// cut down to what TWO wavefronts per SIMD leave: 256 registers and 20 KB of LDS per wavefront (fx_grouped.hip's 32-column
// build takes 392 and 40 KB and runs one wavefront per SIMD, with the VALU busy half of the time).
//
// What makes it fit is that nothing about the structure is per System any more. The host writes one PROGRAM for the batch
// (fx_programs.cpp: build_gc_program; every System has one component, at most 32 variables and 32 expressions — two matrix columns per
// lane; 16 / 16: one column, four wavefronts per SIMD; 48 / 48, the reference's own bench sketch: three columns, a wavefront on
// every SIMD; an over-constrained structure — up to twice the shape's rows — the same bodies with twice the row chunks), the
// wavefront copies it into LDS once, and the four Systems share it:
//   * the row lists (variables and kind of every expression), the free-variable map, the product lists of Jt J and Jt r —
//     4 KB once per wavefront instead of 2.4 KB per System (and no list building when a row takes a System);
//   * Jt J by its PATTERN: a slot per structural non-zero of the lower triangle (ring16: 144 of 528), addressed through the
//     program — the product lists name slots, and a lane's 64 matrix elements are loaded through a table of slot numbers
//     (64 bytes per lane; what is not in the pattern reads the zero slot). The factor's fill exists in registers only;
//   * Jacobian rows compact (an expression's own entries instead of eight).
// ring16: 3.5 KB per System, 18.2 KB per wavefront, eight wavefronts per CU. The f32 instantiation (cfg5) assembles by gather
// instead of LDS float atomics (ds_add_f32 runs at a fourteenth of ds_add_f64's rate on gfx950).
// A batch of SEVERAL structures brings a program per big structure class; one launch works through all of them (a wavefront
// loads the next class's program when its own class's queue is empty).
// The per-row state machine, the device-side queue, the lambda ladder, the hold passes are fx_grouped.hip's.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <utility>

#include "fx_device.h"
#include "fx_expr.h"
#include "fx_grouped_c.h"
#include "fx_grouped_rows.h"
#include "fx_wave.h"

namespace fx {

// 16 free variables and fewer (the reference's bench sketches of one to three triangles): one column per lane, four wavefronts
// per SIMD
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(4, 4))) void lm_solve_grouped_c1_kernel(
    DeviceBatch b, LmParams prm, GcLayout L, uint32_t* __restrict__ next_system) {
    extern __shared__ __align__(16) unsigned char smem[];
    grouped_c_body<1, 1, double>(b, prm, L, next_system, smem);
}
// 17 ... 32 free variables: two columns per lane, 256 registers, two wavefronts per SIMD
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(2, 2))) void lm_solve_grouped_c_kernel(
    DeviceBatch b, LmParams prm, GcLayout L, uint32_t* __restrict__ next_system) {
    extern __shared__ __align__(16) unsigned char smem[];
    grouped_c_body<2, 2, double>(b, prm, L, next_system, smem);
}
// ... in f32 (fx_lm_opts_default_f32): 178 registers (three wavefronts per SIMD — 168 registers, 24 bytes of scratch — measured
// the same: 2.79 against 2.77 ms on 125 000 inconsistent ring16 sketches)
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(2, 2))) void lm_solve_grouped_c_f32_kernel(
    DeviceBatch b, LmParams prm, GcLayout L, uint32_t* __restrict__ next_system) {
    extern __shared__ __align__(16) unsigned char smem[];
    grouped_c_body<2, 2, float>(b, prm, L, next_system, smem);
}
// 33 ... 48 free variables (the reference's own bench sketch, fiksi_bench.rs:15-40: 46): three columns per lane are 288
// registers of matrix alone — one wavefront per SIMD, but on every SIMD (the general build's 16 KB of LDS per System leave two
// wavefronts per CU)
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(1, 1))) void lm_solve_grouped_c3_kernel(
    DeviceBatch b, LmParams prm, GcLayout L, uint32_t* __restrict__ next_system) {
    extern __shared__ __align__(16) unsigned char smem[];
    grouped_c_body<3, 3, double>(b, prm, L, next_system, smem);
}

// Over-constrained structures — more expressions than the shape's 16 / 32 rows, up to twice as many: the same bodies with twice
// the row chunks (cfg5's theme: least squares over more constraints than unknowns)
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(4, 4))) void lm_solve_grouped_c1r_kernel(
    DeviceBatch b, LmParams prm, GcLayout L, uint32_t* __restrict__ next_system) {
    extern __shared__ __align__(16) unsigned char smem[];
    grouped_c_body<1, 2, double>(b, prm, L, next_system, smem);
}
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(2, 2))) void lm_solve_grouped_cr_kernel(
    DeviceBatch b, LmParams prm, GcLayout L, uint32_t* __restrict__ next_system) {
    extern __shared__ __align__(16) unsigned char smem[];
    grouped_c_body<2, 4, double>(b, prm, L, next_system, smem);
}
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(2, 2))) void lm_solve_grouped_cr_f32_kernel(
    DeviceBatch b, LmParams prm, GcLayout L, uint32_t* __restrict__ next_system) {
    extern __shared__ __align__(16) unsigned char smem[];
    grouped_c_body<2, 4, float>(b, prm, L, next_system, smem);
}

// ------------------------------------------------------------------------------------------
// launcher
// ------------------------------------------------------------------------------------------
// the factor a launch of the two-column f64 kernel takes: 1 + the GC_BANDS entry the program names (fx_programs.cpp: build_gc_program),
// 0 = dense — always for a launch over several structure classes and under FIKSI_AMD_GC_BAND=0
static uint32_t gc_band_of(const DeviceBatch& b, const LmParams& p) { return p.gc_band && !b.gc_nclasses && b.gc_band <= GC_NBANDS ? b.gc_band : 0u; }
// the instantiation for a program's shape (columns per lane, row chunks), the compute type and the factor; fn == nullptr: none
static GcBuild gc_build_for(uint32_t nc, uint32_t rc, bool f32, uint32_t band) {
    static unsigned int r1 = 0, r1r = 0, r2 = 0, r2r = 0, r3 = 0, rf = 0, rfr = 0;
    if (!f32 && nc == 2u && rc == 2u && band) return gc_band_build(band);
    if (f32) {
        if (nc == 2u && rc == 2u) return {&lm_solve_grouped_c_f32_kernel, &rf, 8u};
        if (nc == 2u && rc == 4u) return {&lm_solve_grouped_cr_f32_kernel, &rfr, 8u};
        return {nullptr, nullptr, 0u};
    }
    if (nc == 1u && rc == 1u) return {&lm_solve_grouped_c1_kernel, &r1, 16u};
    if (nc == 1u && rc == 2u) return {&lm_solve_grouped_c1r_kernel, &r1r, 16u};
    if (nc == 2u && rc == 2u) return {&lm_solve_grouped_c_kernel, &r2, 8u};
    if (nc == 2u && rc == 4u) return {&lm_solve_grouped_cr_kernel, &r2r, 8u};
    if (nc == 3u && rc == 3u) return {&lm_solve_grouped_c3_kernel, &r3, 4u};
    return {nullptr, nullptr, 0u};
}

// LDS bytes per wavefront, 0 when the batch has no program
size_t grouped_c_lds_bytes(const DeviceBatch& b, uint32_t es) {
    if (!b.gc_tab || !b.gc_words) return 0;
    const GcLayout L = make_gc_layout(b, es);
    return (size_t)L.tab_bytes + 4u * (size_t)L.stride;
}

bool grouped_c_applies(const DeviceBatch& b, const LmParams& p) {
    if (!p.grouped_one_structure) return false;  // (a context created under FIKSI_AMD_GROUPED_C=0: A / B measurements, tests)
    if (!b.gc_tab || !(b.uniform ? b.u_ncomp == 1u : b.gc_nclasses != 0u) || !b.work_counter || b.has_pose) return false;
    if (p.prof || p.lm.solver != FX_STEP_CHOLESKY || (p.mode & (MODE_UNITS | MODE_LBFGS))) return false;
    const bool f32 = p.lm.precision == 32;
    const GcBuild k = gc_build_for(b.gc_nc, b.gc_rc, f32, gc_band_of(b, p));
    if (!k.fn) return false;  // (f32: the 32-column instantiations only)
    // one column per lane: eight wavefronts per CU or more; two: six (a SIMD with two is what the build is for); three: one per SIMD
    const size_t lds = grouped_c_lds_bytes(b, f32 ? 4u : 8u);
    return lds != 0 && lds <= (160u * 1024u) / (b.gc_nc == 1u ? 8u : b.gc_nc == 2u ? 6u : 4u);
}

int grouped_c_band(const DeviceBatch& b, const LmParams& p) {
    if (!grouped_c_applies(b, p) || p.lm.precision == 32 || b.gc_nc != 2u || b.gc_rc != 2u) return -1;
    return (int)gc_band_of(b, p);
}

hipError_t launch_solve_grouped_c(const DeviceBatch& b, const LmParams& p, hipStream_t stream) {
    if (grouped_tiny_applies(b, p)) return launch_solve_tiny(b, p, stream);  // (at most eight variables and expressions: eight Systems per wavefront)
    const bool f32 = p.lm.precision == 32;
    const uint32_t band = f32 ? 0u : gc_band_of(b, p);
    const GcBuild k = gc_build_for(b.gc_nc, b.gc_rc, f32, band);
    if (!k.fn) return hipErrorInvalidValue;
    const GcLayout L = make_gc_layout(b, f32 ? 4u : 8u);
    const uint32_t per_wave = L.tab_bytes + 4u * L.stride;
    static const bool trace = getenv("FIKSI_AMD_TRACE") != nullptr;
    if (trace)
        fprintf(stderr, "[fiksi_amd] grouped kernel, one-structure build (%u columns per lane, %u row chunks, band factor %u, 0 = dense): %u B of LDS per wavefront (program %u, 4 x %u per System: %u slots of Jt J, %u Jacobian entries)\n",
                b.gc_nc, b.gc_rc, band, per_wave, L.tab_bytes, L.stride, b.gc_nslots, b.gc_ng);
    hipError_t e = raise_lds_limit_once(reinterpret_cast<const void*>(k.fn), k.raised);
    if (e != hipSuccess) return e;
    e = hipMemsetAsync(b.work_counter, 0, sizeof(uint32_t) * (b.gc_nclasses ? b.gc_nclasses : 1u), stream);  // the queue heads
    if (e != hipSuccess) return e;
    uint32_t waves = (b.n_systems + 3u) / 4u;
    if (waves > 256u * 16u) waves = 256u * 16u;
    LmParams pl = p;
    pl.spread = 0u;
    if (p.ladder) {
        int dev = 0, cus = 256;
        if (hipGetDevice(&dev) == hipSuccess) (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
        const uint32_t by_lds = (160u * 1024u) / per_wave;
        uint32_t resident = (uint32_t)cus * (by_lds < k.waves_per_cu ? by_lds : k.waves_per_cu);
        if (resident > waves) resident = waves;
        if (b.order && p.spread && !b.gc_nclasses) pl.spread = resident < b.n_systems / 4u ? resident : b.n_systems / 4u;
        if (p.ladder_tail == 0xFFFFFFFFu) pl.ladder_tail = 32u * resident / (b.gc_nclasses ? b.gc_nclasses : 1u);
    }
    hipLaunchKernelGGL(k.fn, dim3(waves), dim3(64), per_wave, stream, b, pl, L, b.work_counter);
    return hipGetLastError();
}

}  // namespace fx
