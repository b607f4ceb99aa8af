// Diagnostic only (fx_debug_dense_solve): the register Cholesky of every build that solves the LM step, run on matrices the caller
// gives, so that tests can hold the factor and the solves against a high-precision reference and check the verdict on singular
// pivots. Each variant is one instantiation a kernel really uses, and runs its call site's sequence: invd = 1, the right-hand side
// in acc before or after the factor as that site sets it, invd2 = invd * invd, x = acc * invd2. x is written whatever the verdict.
//
// Matrices: the host (fx_entry.cpp) pads each to the variant's size N with the identity, right-hand sides with 0, and the count to
// a multiple of four with identity matrices; the kernels read N x N blocks without a test. Row variants (fx_grouped_rows.h) put
// four matrices in a wavefront, one per DPP row: lane r of row g holds column r + 16 q in a[q][.]. The one-column variants
// (fx_chol.h) take one matrix per wavefront, lane j column j, lanes >= N zero as in fx_kernels.hip. f32 variants round their
// inputs to float.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fx_chol.h"
#include "fx_grouped_rows.h"

namespace fx {

namespace {

enum RowSite : int {
    SITE_GENERAL = 0,  // fx_grouped.hip: RBlock<NC, T, 0, UNITS>::factor<false>, acc = rhs after the factor, forward, backward
    SITE_ONE = 1       // fx_grouped_c.h: acc = rhs before RBlock<NC, T, 0, false, W, B>::factor<FWD>, forward unless FWD, backward
};

template <int NC, typename T, bool BOUNDED, int W, int B, bool FWD, int SITE>
__global__ __launch_bounds__(64) void debug_rows_kernel(uint32_t count, uint32_t n, const double* __restrict__ A,
                                                        const double* __restrict__ bv, uint32_t kmax_in, double* __restrict__ x,
                                                        int32_t* __restrict__ bad_out) {
    constexpr int N = RS * NC;
    const int lane = (int)threadIdx.x;
    const int hl = lane & (RS - 1);
    const uint32_t g = blockIdx.x * 4u + (uint32_t)(lane / RS);  // < count, a multiple of 4
    const int kmax = BOUNDED ? (int)kmax_in : N;
    const double* Ag = A + (size_t)g * N * N + hl;
    T a[NC][N];
#pragma unroll
    for (int q = 0; q < NC; ++q) {
#pragma unroll
        for (int i = 0; i < N; ++i) {
            // (the one-structure build loads a structural zero of the band as 0, fx_grouped_c.h)
            if (SITE == SITE_ONE && RBand<NC, W, B>::zero_row(q, i)) a[q][i] = T(0);
            else a[q][i] = (T)Ag[i * N + RS * q];
        }
    }
    T rhs[NC];
#pragma unroll
    for (int q = 0; q < NC; ++q) rhs[q] = (T)bv[(size_t)g * N + hl + RS * q];
    T invd[NC];
#pragma unroll
    for (int q = 0; q < NC; ++q) invd[q] = T(1);
    bool bad = false;
    T acc[NC];
    if constexpr (SITE == SITE_GENERAL) {
#pragma unroll
        for (int q = 0; q < NC; ++q) acc[q] = T(0);
        RBlock<NC, T, 0, BOUNDED>::template factor<false>(a, invd, acc, bad, hl, kmax);
        T invd2[NC];
#pragma unroll
        for (int q = 0; q < NC; ++q) {
            acc[q] = rhs[q];
            invd2[q] = invd[q] * invd[q];
        }
        RBlock<NC, T, 0, BOUNDED>::forward(a, invd, acc, hl, kmax);
        RBlock<NC, T, N / 8 - 1, BOUNDED>::backward(a, invd2, acc, hl, kmax);
#pragma unroll
        for (int q = 0; q < NC; ++q) acc[q] = acc[q] * invd2[q];
    } else {
#pragma unroll
        for (int q = 0; q < NC; ++q) acc[q] = rhs[q];
        RBlock<NC, T, 0, false, W, B>::template factor<FWD>(a, invd, acc, bad, hl, N);
        T invd2[NC];
#pragma unroll
        for (int q = 0; q < NC; ++q) invd2[q] = invd[q] * invd[q];
        if constexpr (!FWD) RBlock<NC, T, 0, false>::forward(a, invd, acc, hl, N);
        RBlock<NC, T, N / 8 - 1, false>::backward(a, invd2, acc, hl, N);
#pragma unroll
        for (int q = 0; q < NC; ++q) acc[q] = acc[q] * invd2[q];
    }
#pragma unroll
    for (int q = 0; q < NC; ++q) x[(size_t)g * N + hl + RS * q] = (double)acc[q];
    if (hl == 0) bad_out[g] = bad ? 1 : 0;
}

// fx_kernels.hip: chol_factor<N, T> + chol_solve<N, T>, one matrix per wavefront
template <int N, typename T>
__global__ __launch_bounds__(64) void debug_chol_kernel(uint32_t count, uint32_t n, const double* __restrict__ A,
                                                        const double* __restrict__ bv, double* __restrict__ x,
                                                        int32_t* __restrict__ bad_out) {
    const int lane = (int)threadIdx.x;
    const uint32_t g = blockIdx.x;
    T a[N];
    const double* Ag = A + (size_t)g * N * N + (lane < N ? lane : 0);
#pragma unroll
    for (int i = 0; i < N; ++i) a[i] = lane < N ? (T)Ag[i * N] : T(0);
    const T rhs_l = lane < N ? (T)bv[(size_t)g * N + lane] : T(0);
    T invd = T(1);
    const bool solved = chol_factor<N, T>(a, invd, lane);
    const T delta = chol_solve<N, T>(a, invd, rhs_l, lane);
    if (lane < N) x[(size_t)g * N + lane] = (double)delta;
    if (lane == 0) bad_out[g] = solved ? 0 : 1;
}

// fx_wide.hip: a diagonal block of the blocked factorization, chol_factor<64, double> with nb = n, written back to the plain lower
// triangle and reloaded (reload_factor: invd = 1 / d, column entries L_ik * d_k) before the solves. SECOND: the second block's
// chol_solve with nb; otherwise the first block's chol_forward then chol_backward.
template <bool SECOND>
__global__ __launch_bounds__(64) void debug_wide_kernel(uint32_t count, uint32_t n, const double* __restrict__ A,
                                                        const double* __restrict__ bv, double* __restrict__ x,
                                                        int32_t* __restrict__ bad_out) {
    __shared__ double Lm[64 * 65 / 2];
    const int lane = (int)threadIdx.x;
    const uint32_t g = blockIdx.x;
    const uint32_t nb = n;
    auto tri = [](uint32_t r, uint32_t c) { return r * (r + 1u) / 2u + c; };
    double a[64], invd = 1.0;
    const double* Ag = A + (size_t)g * 64 * 64 + lane;
#pragma unroll
    for (int i = 0; i < 64; ++i) a[i] = Ag[i * 64];  // (the identity past nb: load_block's padding)
    const bool ok = chol_factor<64, double>(a, invd, lane, (int)nb);
    if ((uint32_t)lane < nb) {
        const uint32_t c = (uint32_t)lane;
#pragma unroll
        for (int p = 0; p < 64; ++p)
            if (p <= lane) Lm[tri(c, (uint32_t)p)] = a[p];
    }
    __syncthreads();
    {
        const uint32_t c = (uint32_t)lane;
        const bool lane_real = c < nb;
        const double d = lane_real ? Lm[tri(c, c)] : 1.0;
        invd = 1.0 / d;
#pragma unroll
        for (int i = 0; i < 64; ++i) {
            const uint32_t r = (uint32_t)i;
            const bool real = lane_real && r < nb;
            const uint32_t hi = real ? max(r, c) : 0u, lo = real ? min(r, c) : 0u;
            const double v = Lm[tri(hi, lo)];
            a[i] = real ? ((i > lane) ? v * d : v) : ((i == lane) ? 1.0 : 0.0);
        }
    }
    const double rhs = bv[(size_t)g * 64 + lane];
    double xl;
    if constexpr (SECOND) {
        xl = chol_solve<64, double>(a, invd, rhs, lane, (int)nb);
    } else {
        const double y = chol_forward<64, double>(a, invd, rhs, lane);
        xl = chol_backward<64, double>(a, invd, y, lane);
    }
    x[(size_t)g * 64 + lane] = xl;
    if (lane == 0) bad_out[g] = ok ? 0 : 1;
}

template <int NC, typename T, bool BOUNDED, int W, int B, bool FWD, int SITE>
hipError_t rows(uint32_t count, uint32_t n, const double* A, const double* b, uint32_t kmax, double* x, int32_t* bad, hipStream_t s) {
    if (n > (uint32_t)(RS * NC) || count % 4u || (BOUNDED && (kmax > (uint32_t)(RS * NC) || kmax < n))) return hipErrorInvalidValue;
    hipLaunchKernelGGL((debug_rows_kernel<NC, T, BOUNDED, W, B, FWD, SITE>), dim3(count / 4u), dim3(64), 0, s, count, n, A, b, kmax, x, bad);
    return hipGetLastError();
}
template <int N, typename T>
hipError_t chol(uint32_t count, uint32_t n, const double* A, const double* b, double* x, int32_t* bad, hipStream_t s) {
    if (n > (uint32_t)N) return hipErrorInvalidValue;
    hipLaunchKernelGGL((debug_chol_kernel<N, T>), dim3(count), dim3(64), 0, s, count, n, A, b, x, bad);
    return hipGetLastError();
}
template <bool SECOND>
hipError_t wide(uint32_t count, uint32_t n, const double* A, const double* b, double* x, int32_t* bad, hipStream_t s) {
    if (n == 0u || n > 64u) return hipErrorInvalidValue;
    hipLaunchKernelGGL((debug_wide_kernel<SECOND>), dim3(count), dim3(64), 0, s, count, n, A, b, x, bad);
    return hipGetLastError();
}

}  // namespace

// The variant table (fiksi_amd/abi.py: DENSE_VARIANTS holds the same list by name; tests/test_dense_variants.py checks both
// against the call sites). rows<NC, T, BOUNDED, W, B, FWD, SITE>, chol<N, T>, wide<SECOND>.
// the size N each variant factors (the host pads the caller's matrices to it), 0 for no such variant
uint32_t debug_dense_size(int variant) {
    static const uint8_t n[] = {16, 32, 48, 16, 32, 48, 16, 32, 48, 16, 32, 48, 16, 32, 32, 48, 32, 32, 32,
                                8, 16, 24, 32, 40, 48, 56, 64, 8, 16, 24, 32, 40, 48, 56, 64, 64, 64};
    return (variant >= 0 && variant < (int)sizeof(n)) ? n[variant] : 0u;
}

hipError_t launch_debug_dense_solve(int variant, uint32_t count, uint32_t n, const double* A, const double* b, uint32_t kmax, double* x,
                                    int32_t* bad, hipStream_t s) {
    if (count == 0u) return hipSuccess;
    switch (variant) {
        // fx_grouped.hip, the general build: NC = 1, 2, 3 in f64 and f32, UNITS (SinglePass blocks: BOUNDED) or not
        case 0: return rows<1, double, false, 16, 0, false, SITE_GENERAL>(count, n, A, b, kmax, x, bad, s);
        case 1: return rows<2, double, false, 32, 0, false, SITE_GENERAL>(count, n, A, b, kmax, x, bad, s);
        case 2: return rows<3, double, false, 48, 0, false, SITE_GENERAL>(count, n, A, b, kmax, x, bad, s);
        case 3: return rows<1, float, false, 16, 0, false, SITE_GENERAL>(count, n, A, b, kmax, x, bad, s);
        case 4: return rows<2, float, false, 32, 0, false, SITE_GENERAL>(count, n, A, b, kmax, x, bad, s);
        case 5: return rows<3, float, false, 48, 0, false, SITE_GENERAL>(count, n, A, b, kmax, x, bad, s);
        case 6: return rows<1, double, true, 16, 0, false, SITE_GENERAL>(count, n, A, b, kmax, x, bad, s);
        case 7: return rows<2, double, true, 32, 0, false, SITE_GENERAL>(count, n, A, b, kmax, x, bad, s);
        case 8: return rows<3, double, true, 48, 0, false, SITE_GENERAL>(count, n, A, b, kmax, x, bad, s);
        case 9: return rows<1, float, true, 16, 0, false, SITE_GENERAL>(count, n, A, b, kmax, x, bad, s);
        case 10: return rows<2, float, true, 32, 0, false, SITE_GENERAL>(count, n, A, b, kmax, x, bad, s);
        case 11: return rows<3, float, true, 48, 0, false, SITE_GENERAL>(count, n, A, b, kmax, x, bad, s);
        // fx_grouped_c.hip / fx_grouped_band.hip, the one-structure build: FWD = (NC == 2)
        case 12: return rows<1, double, false, 16, 0, false, SITE_ONE>(count, n, A, b, kmax, x, bad, s);
        case 13: return rows<2, double, false, 32, 0, true, SITE_ONE>(count, n, A, b, kmax, x, bad, s);
        case 14: return rows<2, float, false, 32, 0, true, SITE_ONE>(count, n, A, b, kmax, x, bad, s);
        case 15: return rows<3, double, false, 48, 0, false, SITE_ONE>(count, n, A, b, kmax, x, bad, s);
        case 16: return rows<2, double, false, 5, 0, true, SITE_ONE>(count, n, A, b, kmax, x, bad, s);
        case 17: return rows<2, double, false, 5, 4, true, SITE_ONE>(count, n, A, b, kmax, x, bad, s);
        case 18: return rows<2, double, false, 5, 6, true, SITE_ONE>(count, n, A, b, kmax, x, bad, s);
        // fx_kernels.hip: chol_factor<N, T> + chol_solve<N, T>
        case 19: return chol<8, double>(count, n, A, b, x, bad, s);
        case 20: return chol<16, double>(count, n, A, b, x, bad, s);
        case 21: return chol<24, double>(count, n, A, b, x, bad, s);
        case 22: return chol<32, double>(count, n, A, b, x, bad, s);
        case 23: return chol<40, double>(count, n, A, b, x, bad, s);
        case 24: return chol<48, double>(count, n, A, b, x, bad, s);
        case 25: return chol<56, double>(count, n, A, b, x, bad, s);
        case 26: return chol<64, double>(count, n, A, b, x, bad, s);
        case 27: return chol<8, float>(count, n, A, b, x, bad, s);
        case 28: return chol<16, float>(count, n, A, b, x, bad, s);
        case 29: return chol<24, float>(count, n, A, b, x, bad, s);
        case 30: return chol<32, float>(count, n, A, b, x, bad, s);
        case 31: return chol<40, float>(count, n, A, b, x, bad, s);
        case 32: return chol<48, float>(count, n, A, b, x, bad, s);
        case 33: return chol<56, float>(count, n, A, b, x, bad, s);
        case 34: return chol<64, float>(count, n, A, b, x, bad, s);
        // fx_wide.hip: chol_factor<64, double> with nb, then the first block's forward / backward or the second block's solve
        case 35: return wide<false>(count, n, A, b, x, bad, s);
        case 36: return wide<true>(count, n, A, b, x, bad, s);
        default: return hipErrorInvalidValue;
    }
}

}  // namespace fx
