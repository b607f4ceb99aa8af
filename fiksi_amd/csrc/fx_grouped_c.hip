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
// ... with the set-up staged before it and the closing check after it (gc_stage_kernel, gc_close_kernel)
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(2, 2))) void lm_solve_grouped_c_staged_kernel(
    DeviceBatch b, LmParams prm, GcLayout L, uint32_t* __restrict__ next_system) {
    extern __shared__ __align__(16) unsigned char smem[];
    grouped_c_body<2, 2, double, RS * 2, 0, true>(b, prm, L, next_system, smem);
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
// the staged set-up and closing check of a resident f64 batch (DeviceBatch::st_x): work that is the same for every System and
// independent between them, streamed with every lane busy instead of run by one row of the solve while its wavefront's other
// rows wait. One row of 16 lanes per place j of the launch's hand-out list: entry j of b.order (the classes'
// member lists one after the other in a launch over structure classes), System j when there is no list.
// ------------------------------------------------------------------------------------------
struct GcEntry {
    const uint32_t* prog;  // the System's program (in global memory: the tables are read where they lie)
    uint32_t s, v0, e0, nvt, net;
};
__device__ __forceinline__ GcEntry gc_entry(const DeviceBatch& b, uint32_t j) {
    GcEntry E;
    E.prog = b.gc_tab;
    E.s = b.order ? b.order[j] : j;
    if (b.gc_nclasses) {  // (the member lists lie class after class, list_off ascending)
        uint32_t c = 0;
        while (c + 1u < b.gc_nclasses && j >= b.gc_classes[c + 1u].list_off) ++c;
        E.prog = b.gc_tab + b.gc_classes[c].prog_off;
    }
    E.nvt = E.prog[1];
    E.net = E.prog[2];
    E.v0 = b.uniform ? E.s * E.nvt : b.var_off[E.s];
    E.e0 = b.uniform ? E.s * E.net : b.expr_off[E.s];
    return E;
}

// before the solve: gc_setup, the operations of the kernel's own NEXT, on the same operands, into place j; the kernel's write of the
// fixed variables' start values into b.vars moves here with it (the free ones are written back when the System is done)
template <int NC, int RC>
__global__ __launch_bounds__(256) void gc_stage_kernel(DeviceBatch b, uint32_t mode) {
    using TK = GcTable<NC, RC>;
    const int lane = (int)(threadIdx.x & 63u);
    const int hl = lane & (RS - 1);
    uint32_t j = (blockIdx.x * 256u + threadIdx.x) / RS;
    const bool live = j < b.n_systems;
    if (!live) j = b.n_systems - 1u;  // (a row past the end repeats the last entry and writes nothing)
    const GcEntry E = gc_entry(b, j);
    const int8_t* vcol = reinterpret_cast<const int8_t*>(E.prog) + TK::VCOL;
    const uint8_t* rtag = reinterpret_cast<const uint8_t*>(E.prog) + TK::RTAG;
    double c_var[NC], c_param[RC];
    int colk[NC], tagk[RC];
#pragma unroll
    for (int k = 0; k < NC; ++k) {
        const uint32_t i = (uint32_t)(RS * k + hl);
        c_var[k] = i < E.nvt ? b.vars0[E.v0 + i] : 0.0;
        colk[k] = i < E.nvt ? (int)vcol[i] : -1;
    }
#pragma unroll
    for (int k = 0; k < RC; ++k) {
        const uint32_t i = (uint32_t)(RS * k + hl);
        c_param[k] = i < E.net ? b.expr_param[E.e0 + i] : 0.0;
        tagk[k] = i < E.net ? (int)rtag[i] : 0;
    }
    double x[NC], pe[RC];
    const double scale = gc_setup<NC, RC>(mode, E.nvt, E.net, hl, lane & ~(RS - 1), c_var, colk, c_param, tagk, x, pe);
    if (!live) return;
#pragma unroll
    for (int k = 0; k < NC; ++k) {
        const uint32_t i = (uint32_t)(RS * k + hl);
        if (i < E.nvt) {
            b.st_x[(uint32_t)(RS * NC) * j + i] = x[k];
            if (colk[k] < 0) b.vars[E.v0 + i] = c_var[k];  // (fixed variables stay bit-identical)
        }
    }
#pragma unroll
    for (int k = 0; k < RC; ++k)
        if ((uint32_t)(RS * k + hl) < E.net) b.st_p[(uint32_t)(RS * RC) * j + (uint32_t)(RS * k + hl)] = pe[k];
    if (hl == 0) {
        b.st_scale[j] = scale;
        b.st_sys[j] = E.s;
    }
}

// after the solve: the closing check (constraints/mod.rs:96-109) on the written-back values, what the kernel's FINISH computed —
// the same expressions on the same operands, summed in the same order — into the result records the kernel wrote
template <int NC, int RC>
__global__ __launch_bounds__(256) void gc_close_kernel(DeviceBatch b) {
    using TK = GcTable<NC, RC>;
    __shared__ double vv[256 / RS][RS * NC];  // the System's unscaled values, a row's own
    const int hl = (int)(threadIdx.x & (RS - 1));
    const uint32_t row = threadIdx.x / RS;
    uint32_t j = (blockIdx.x * 256u + threadIdx.x) / RS;
    const bool live = j < b.n_systems;
    if (!live) j = b.n_systems - 1u;
    const GcEntry E = gc_entry(b, j);
    const uint8_t* rtag = reinterpret_cast<const uint8_t*>(E.prog) + TK::RTAG;
    const uint2* gvar = reinterpret_cast<const uint2*>(reinterpret_cast<const unsigned char*>(E.prog) + TK::GVAR);
#pragma unroll
    for (int k = 0; k < NC; ++k) {
        const uint32_t i = (uint32_t)(RS * k + hl);
        vv[row][i] = i < E.nvt ? b.vars[E.v0 + i] : 0.0;
    }
    __syncthreads();
    double part[RC];
#pragma unroll
    for (int k = 0; k < RC; ++k) {
        const uint32_t i = (uint32_t)(hl + RS * k);
        part[k] = 0.0;
        if (i < E.net) {
            double v[8], g[8];
            const uint2 gv = gvar[i];
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = vv[row][(gv.x >> (8 * e)) & 0xFFu];  // (the program's variable numbers are < nvt)
#pragma unroll
            for (int e = 0; e < 4; ++e) v[4 + e] = vv[row][(gv.y >> (8 * e)) & 0xFFu];
            const double r = eval_expression<double, false, false>((int)rtag[i], v, b.expr_param[E.e0 + i], g);
            part[k] = r * r;
        }
    }
    const double sse_u = gc_rows_sum<RC>(part);
    if (live && hl == 0) {
        b.results[E.s].sse_unscaled = sse_u;
        if (b.results_out) b.results_out[E.s].sse_unscaled = sse_u;
    }
}

// ------------------------------------------------------------------------------------------
// launcher
// ------------------------------------------------------------------------------------------
// the factor a launch of the two-column f64 kernel takes: 1 + the GC_BANDS entry the program names (fx_programs.cpp: build_gc_program),
// 0 = dense — always for a launch over several structure classes and under FIKSI_AMD_GC_BAND=0
static uint32_t gc_band_of(const DeviceBatch& b, const LmParams& p) { return p.gc_band && !b.gc_nclasses && b.gc_band <= GC_NBANDS ? b.gc_band : 0u; }
// whether a launch takes the staged set-up and closing check: the two-column f64 shape on a batch with a staging area, the
// Systems' values on the device (not the caller's arrays: vars_in / param_in) and no hand-over queue (queue_len)
static bool gc_staged_of(const DeviceBatch& b, const LmParams& p) {
    return p.gc_staged && b.st_x && b.gc_nc == 2u && b.gc_rc == 2u && p.lm.precision != 32 && !b.vars_in && !b.param_in && !b.queue_len;
}
// the instantiation for a program's shape (columns per lane, row chunks), the compute type, the factor and the staging; fn == nullptr: none
static GcBuild gc_build_for(uint32_t nc, uint32_t rc, bool f32, uint32_t band, bool staged = false) {
    static unsigned int r1 = 0, r1r = 0, r2 = 0, r2s = 0, r2r = 0, r3 = 0, rf = 0, rfr = 0;
    if (!f32 && nc == 2u && rc == 2u && band) return gc_band_build(band, staged);
    if (!f32 && nc == 2u && rc == 2u && staged) return {&lm_solve_grouped_c_staged_kernel, &r2s, 8u};
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

int grouped_c_staged(const DeviceBatch& b, const LmParams& p) {
    if (!grouped_c_applies(b, p) || grouped_tiny_applies(b, p)) return -1;
    return gc_staged_of(b, p) ? 1 : 0;
}

hipError_t launch_solve_grouped_c(const DeviceBatch& b, const LmParams& p, hipStream_t stream) {
    if (grouped_tiny_applies(b, p)) return launch_solve_tiny(b, p, stream);  // (at most eight variables and expressions: eight Systems per wavefront)
    const bool f32 = p.lm.precision == 32;
    const uint32_t band = f32 ? 0u : gc_band_of(b, p);
    const bool staged = gc_staged_of(b, p);
    const GcBuild k = gc_build_for(b.gc_nc, b.gc_rc, f32, band, staged);
    if (!k.fn) return hipErrorInvalidValue;
    const GcLayout L = make_gc_layout(b, f32 ? 4u : 8u, staged);
    const uint32_t per_wave = L.tab_bytes + 4u * L.stride;
    static const bool trace = getenv("FIKSI_AMD_TRACE") != nullptr;
    if (trace)
        fprintf(stderr, "[fiksi_amd] grouped kernel, one-structure build (%u columns per lane, %u row chunks, band factor %u, 0 = dense, staged %d): %u B of LDS per wavefront (program %u, 4 x %u per System: %u slots of Jt J, %u Jacobian entries)\n",
                b.gc_nc, b.gc_rc, band, (int)staged, per_wave, L.tab_bytes, L.stride, b.gc_nslots, b.gc_ng);
    hipError_t e = raise_lds_limit_once(reinterpret_cast<const void*>(k.fn), k.raised);
    if (e != hipSuccess) return e;
    e = hipMemsetAsync(b.work_counter, 0, sizeof(uint32_t) * (b.gc_nclasses ? b.gc_nclasses : 1u), stream);  // the queue heads
    if (e != hipSuccess) return e;
    uint32_t waves = (b.n_systems + 3u) / 4u;
    if (waves > 256u * 16u) waves = 256u * 16u;
    LmParams pl = p;
    pl.spread = 0u;
    // (a staged launch's FINISH is a few stores and its NEXT one round trip: waiting for company costs more than it saves —
    // 100 000 ring16 sketches, hold 0 / 1 / 2 / 3 / 4: 1.487 / 1.508 / 1.518 / 1.523 / 1.537 ms; the inline set-up keeps 2)
    if (staged && !p.hold_set) pl.hold_passes = 0u;
    if (p.ladder) {
        int dev = 0, cus = 256;
        if (hipGetDevice(&dev) == hipSuccess) (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
        const uint32_t by_lds = (160u * 1024u) / per_wave;
        uint32_t resident = (uint32_t)cus * (by_lds < k.waves_per_cu ? by_lds : k.waves_per_cu);
        if (resident > waves) resident = waves;
        if (b.order && p.spread && !b.gc_nclasses) pl.spread = resident < b.n_systems / 4u ? resident : b.n_systems / 4u;
        if (p.ladder_tail == 0xFFFFFFFFu) pl.ladder_tail = 32u * resident / (b.gc_nclasses ? b.gc_nclasses : 1u);
    }
    const uint32_t st_blocks = (b.n_systems + 256u / RS - 1u) / (256u / RS);  // (a row of 16 lanes per System)
    if (staged && b.n_systems) hipLaunchKernelGGL((gc_stage_kernel<2, 2>), dim3(st_blocks), dim3(256), 0, stream, b, p.mode);
    hipLaunchKernelGGL(k.fn, dim3(waves), dim3(64), per_wave, stream, b, pl, L, b.work_counter);
    if (staged && b.n_systems) hipLaunchKernelGGL((gc_close_kernel<2, 2>), dim3(st_blocks), dim3(256), 0, stream, b);
    return hipGetLastError();
}

}  // namespace fx
