// The one-structure build's body (fx_grouped_c.hip): shared by its instantiations there and by the band-factor instantiations
// of fx_grouped_band.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <utility>

#include "fx_device.h"
#include "fx_expr.h"
#include "fx_grouped_rows.h"
#include "fx_wave.h"

namespace fx {

// A System's block, bytes: everything of fixed size first, at offsets the instructions carry as immediates (one base register per
// row), then Jt J's slots and behind them the compact Jacobian rows
// (NV = 16 NC: the most variables of a System in the build with NC columns per lane; NR = 16 RC: the most expressions — an
// over-constrained structure takes the instantiation with twice the rows; ES: bytes of the compute type; VO: 1 = the closing check's
// unscaled values have a place, 0 = a staged build, whose closing check is a pass of its own)
template <int NV, int NR, int ES, int VO = 1> struct GcBlock {
    static constexpr uint32_t XS = 0, RHS = ES * NV, R = 2 * ES * NV, P = R + ES * NR, VOUT = P + ES * NR, STASH = VOUT + 8 * NV * VO, A = STASH + 16;
};
struct GcLayout {
    uint32_t tab_bytes, off_g, stride;
};

static GcLayout make_gc_layout(const DeviceBatch& b, uint32_t es, bool staged = false) {
    GcLayout L;
    L.tab_bytes = ((es == 4u ? b.gc_words_all : b.gc_words) * 4u + 15u) & ~15u;
    L.off_g = (2u * es + (staged ? 0u : 8u)) * 16u * b.gc_nc + 2u * es * 16u * b.gc_rc + 16u + b.gc_nslots * es;  // (slots are a multiple of four: 16-byte aligned)
    L.stride = L.off_g + b.gc_ng * es;
    return L;
}

__device__ __forceinline__ uint32_t rfl(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }

// sum over the expressions' chunks of a row's System, as wave_sum adds its blocks: (b0 + b1) + (b2 + b3)
template <int RC, typename U>
__device__ __forceinline__ U gc_rows_sum(const U (&part)[RC]) {
    U s01 = row_sum(part[0]);
    if constexpr (RC >= 2) s01 = s01 + row_sum(part[1]);
    if constexpr (RC == 3) s01 = s01 + row_sum(part[2]);
    if constexpr (RC == 4) s01 = s01 + (row_sum(part[2]) + row_sum(part[3]));
    return s01;
}

// K0 of the System of a row of 16 lanes (assemble/mod.rs:32-44, 91-111): from its start values (c_var[k]: variable RS k + hl; colk:
// its free column or -1) and its parameters (c_param[k], tagk[k]: expression RS k + hl), its scale — summed strictly in reference
// order (utils.rs:11-33) — and, in f64, its scaled and perturbed start point x and its scaled parameters pe. Past nvt / net: zeros.
// The kernel's own set-up and the staged one (gc_stage_kernel) both run this: the same operations in the same order.
template <int NC, int RC>
__device__ __forceinline__ double gc_setup(uint32_t mode, uint32_t nvt, uint32_t net, int hl, int gbase, const double (&c_var)[NC],
                                           const int (&colk)[NC], const double (&c_param)[RC], const int (&tagk)[RC], double (&x)[NC],
                                           double (&pe)[RC]) {
    double scale = 1.0, scale_recip = 1.0;
    if (mode & 1u) {
        double sum = 0.0;
        uint32_t count = nvt;
#pragma unroll
        for (int k = 0; k < NC; ++k)
            if ((uint32_t)(RS * k) < nvt) seq_add(sum, c_var[k] * c_var[k]);  // (past the end: + 0.0, exact)
#pragma unroll
        for (int k = 0; k < RC; ++k) {
            if ((uint32_t)(RS * k) < net) {
                const bool isd = (uint32_t)(RS * k + hl) < net && (tagk[k] == FX_TAG_PPD || tagk[k] == FX_TAG_PLD);
                count += (uint32_t)__popc((uint32_t)(__ballot(isd) >> gbase) & 0xFFFFu);
                seq_add(sum, isd ? c_param[k] * c_param[k] : 0.0);
            }
        }
        scale = ::sqrt(sum / (double)count);
        scale_recip = 1.0 / scale;
    }
#pragma unroll
    for (int k = 0; k < NC; ++k) {
        x[k] = 0.0;
        if ((uint32_t)(RS * k + hl) < nvt) {
            double xx = (mode & 1u) ? c_var[k] * scale_recip : c_var[k];
            if (colk[k] >= 0 && (mode & 2u)) {  // K0b: two draws of the LCG per free variable, in column order
                uint32_t st = lcg_jump(42u, 2u * (uint32_t)colk[k]);
                st = st * 1664525u + 1013904223u;
                const double f1 = (1.0 / 4294967295.0) * (double)st;
                st = st * 1664525u + 1013904223u;
                const double f2 = (1.0 / 4294967295.0) * (double)st;
                xx += xx * (1.0 / 8196.0) * f1 + (1.0 / 65568.0) * f2;
            }
            x[k] = xx;
        }
    }
#pragma unroll
    for (int k = 0; k < RC; ++k) {
        pe[k] = c_param[k];
        if ((mode & 1u) && (tagk[k] == FX_TAG_PPD || tagk[k] == FX_TAG_PLD)) pe[k] = scale_recip * c_param[k];
    }
    return scale;
}

// W, B: the factor's band and border (fx_grouped_rows.h: RBand; the dense factor by default). STAGED: every System's set-up comes
// from b.st_x / st_p / st_scale and its closing check is left to gc_close_kernel (resident f64 batches; fx_grouped_c.hip: the launcher)
template <int NC, int RC, typename T, int W = RS * NC, int B = 0, bool STAGED = false>
__device__ __forceinline__ void grouped_c_body(const DeviceBatch& b, const LmParams& prm, const GcLayout& L, uint32_t* __restrict__ next_system,
                                               unsigned char* smem) {
    static_assert(!STAGED || (sizeof(T) == 8 && NC == 2 && RC == 2), "the staged set-up: f64, 32 + 32 values per place (fx_solve.cpp)");
    constexpr int N = RS * NC;
    using BK = GcBlock<N, RS * RC, (int)sizeof(T), STAGED ? 0 : 1>;
    using V16 = typename Vec16<T>::type;
    using TK = GcTable<NC, RC>;
    const int lane = threadIdx.x;
    const int hl = lane & (RS - 1);
    const int gbase = lane & ~(RS - 1);
    const int myrow = lane / RS;
    // The program and the queue at hand. A batch of one structure has one of each; a batch of several structures brings a
    // program, a member list and a queue head per structure CLASS (b.gc_classes; fx_solve.cpp: launch_class_solves): a wavefront
    // starts on the class its place in the grid falls into — the grid is dealt in proportion to the classes' sizes — and, when
    // that queue is empty and its Systems are done, loads the next class's program and goes on there: one launch, every
    // wavefront busy until every queue is empty.
    const uint32_t* TB = reinterpret_cast<const uint32_t*>(smem);
    uint32_t nvt = 0, net = 0, nfree = 0, n_pw = 0, n_pe = 0, nslots = 0;
    uint32_t qn = 0;                  // Systems in the queue
    const uint32_t* qlist = nullptr;  // ... their numbers (null: the ticket is the number)
    uint32_t* qhead = next_system;    // ... its head
    uint32_t qbase = 0;               // ... where its list starts in b.order (the staged data of ticket t lie at place qbase + t)
    // (the tables of fixed size sit at fixed places: fx_device.h, GcTable)
    const int8_t* vcol = reinterpret_cast<const int8_t*>(smem + TK::VCOL);         // [N] variable -> free column or -1
    const uint8_t* fidx = smem + TK::FIDX;                                         // [N] free column -> variable
    const uint8_t* rtag = smem + TK::RTAG;                                         // [N] kind of expression i
    const uint16_t* gbaseT = reinterpret_cast<const uint16_t*>(smem + TK::GBASE);  // [N] first compact Jacobian entry of row i
    const uint2* gvar = reinterpret_cast<const uint2*>(smem + TK::GVAR);           // [N] eight variable numbers, a byte each
    const uint4* LT = reinterpret_cast<const uint4*>(smem + TK::LT + (uint32_t)hl * (uint32_t)(NC * N));  // this lane's NC x N slot numbers
    const uint32_t* PE = reinterpret_cast<const uint32_t*>(smem + TK::PE);         // right-hand side: entry | row << 8 | column << 16
    const uint32_t* PW = PE;                                                       // products: entry a | entry b << 8 | slot << 16 (behind PE)

    unsigned char* const rows0 = smem + L.tab_bytes;
    unsigned char* base = rows0 + (uint32_t)myrow * L.stride;
    T* XS = reinterpret_cast<T*>(base + BK::XS);          // [N] working variables: trial point on the free ones
    T* At = reinterpret_cast<T*>(base + BK::A);           // Jt J by slots (+ lambda on the diagonal per trial)
    T* rhsv = reinterpret_cast<T*>(base + BK::RHS);       // [N] -Jt r
    T* G = At;                                            // compact Jacobian rows of the last evaluated point (behind the slots)
    T* R = reinterpret_cast<T*>(base + BK::R);            // [N]
    T* P = reinterpret_cast<T*>(base + BK::P);            // [N] scaled parameters
    double* VOUT = reinterpret_cast<double*>(base + BK::VOUT);    // [N] unscaled values as written back
    double* STASH = reinterpret_cast<double*>(base + BK::STASH);  // [2] the System's scale, the SSE of its start point

    const fx_lm_opts o = prm.lm;

    // per lane, fixed for a program: the variables of its columns and the slots of their diagonal entries
    uint32_t my_vi[NC], dslot[NC];
#pragma unroll
    for (int q = 0; q < NC; ++q) my_vi[q] = dslot[q] = 0u;

    // per-row state (identical in every lane of the row unless noted)
    int phase = GP_NEXT;
    uint32_t s = 0;
    T xc[NC], diag[NC], rhs_l[NC];
#pragma unroll
    for (int q = 0; q < NC; ++q) {
        xc[q] = rhs_l[q] = T(0);
        diag[q] = T(1);
    }
    T sse = T(0);
    double lambda = 0.0;
    uint32_t accepted = 0, trials = 0, outer = 0, exit_code = FX_EXIT_MAX_OUTER;
    bool fresh = false;
    uint32_t held = 0;
    // the lambda ladder (fx_grouped.hip)
    int lad_rank = 0, lad_width = 1, lad_lead = myrow;
    uint32_t lad_members = (uint32_t)myrow * 0x55u;
    int win_row = myrow;
    bool qdone = false;
    uint32_t last_tk = 0;

    auto row_vars = [&](uint32_t row, const T* from, T (&v)[8]) {
        const uint2 gv = gvar[row];
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = from[(gv.x >> (8 * e)) & 0xFFu];
#pragma unroll
        for (int e = 0; e < 4; ++e) v[4 + e] = from[(gv.y >> (8 * e)) & 0xFFu];
    };
    // sum over a vector laid out 16 entries per accumulator, as wave_sum adds its blocks: (b0 + b1) + (b2 + b3) with the blocks
    // past the end left out (+ 0.0 of a sum of squares: exact)
    auto chunk_sum = [&](const auto (&part)[NC]) {
        auto s01 = row_sum(part[0]);
        if constexpr (NC >= 2) s01 = s01 + row_sum(part[1]);
        if constexpr (NC >= 3) s01 = s01 + row_sum(part[2]);
        return s01;
    };
    // ... over the expressions' chunks: (b0 + b1) + (b2 + b3)
    auto rows_sum = [&](const auto (&part)[RC]) { return gc_rows_sum<RC>(part); };
    // residuals and Jacobian rows of the point in XS
    auto eval_rows = [&]() -> T {
        T part[RC];
#pragma unroll
        for (int k = 0; k < RC; ++k) part[k] = T(0);
#pragma unroll
        for (int k = 0; k < RC; ++k) {
            const uint32_t row = (uint32_t)(hl + RS * k);
            if (row < net) {
                T v[8], g[8] = {0, 0, 0, 0, 0, 0, 0, 0};
                row_vars(row, XS, v);
                const int tag = (int)rtag[row];
                const T r = eval_expression<T, true, false>(tag, v, P[row], g);
                R[row] = r;
                const uint32_t gb = gbaseT[row];
                const int kk = tag_nvars(tag);
#pragma unroll
                for (int e = 0; e < 8; ++e)
                    if (e < kk) G[gb + (uint32_t)e] = g[e];
                part[k] = r * r;
            }
        }
        group_sync();
        return rows_sum(part);
    };
    // K3: Jt J into its slots and -Jt r from the program's lists (ds_add_f64; entry t is lane t % 16's, 16 consecutive entries
    // per instruction, in list order — fx_grouped.hip's order)
    auto form_normal = [&]() {
        if constexpr (sizeof(T) == 4) {
            // f32: every slot's and every column's sum by a gather, in list order — the order the atomics below arrive in — instead
            // of ds_add_f32, which gfx950 executes at a fourteenth of ds_add_f64's rate (tools/probes/lds_atomic_f32_probe.hip)
            const uint16_t* sptr = reinterpret_cast<const uint16_t*>(smem + rfl(TB[9]));
            const uint16_t* SPW = reinterpret_cast<const uint16_t*>(smem + rfl(TB[10]));
            const uint16_t* cptr = reinterpret_cast<const uint16_t*>(smem + rfl(TB[11]));
            const uint16_t* CPE = reinterpret_cast<const uint16_t*>(smem + rfl(TB[12]));
            for (uint32_t sl = hl; sl < nslots; sl += RS) {
                const uint32_t t0 = sptr[sl], t1 = sptr[sl + 1];
                T acc = T(0);
                for (uint32_t t = t0; t < t1; ++t) {
                    const uint32_t w = SPW[t];
                    acc += G[w & 0xFFu] * G[w >> 8];
                }
                At[sl] = acc;
            }
#pragma unroll
            for (int q = 0; q < NC; ++q) {
                const uint32_t j = (uint32_t)(hl + RS * q);
                const uint32_t t0 = cptr[j], t1 = cptr[j + 1];
                T acc = T(0);
                for (uint32_t t = t0; t < t1; ++t) {
                    const uint32_t w = CPE[t];
                    acc += G[w & 0xFFu] * -R[w >> 8];
                }
                rhsv[j] = acc;
            }
            group_sync();
#pragma unroll
            for (int q = 0; q < NC; ++q)
                if ((uint32_t)(hl + RS * q) >= nfree) At[dslot[q]] = T(1);  // identity padding
            group_sync();
#pragma unroll
            for (int q = 0; q < NC; ++q) {
                diag[q] = At[dslot[q]];
                rhs_l[q] = rhsv[hl + RS * q];
            }
            return;
        }
        {
            V16 z;
            for (int q = 0; q < Vec16<T>::n; ++q) reinterpret_cast<T*>(&z)[q] = T(0);
            for (uint32_t i = hl; i < nslots / (uint32_t)Vec16<T>::n; i += RS) reinterpret_cast<V16*>(At)[i] = z;
        }
#pragma unroll
        for (int q = 0; q < NC; ++q) rhsv[hl + RS * q] = T(0);
        group_sync();
        constexpr int U = 4;
        for (uint32_t t0 = 0; t0 < n_pw; t0 += RS * U) {
            uint32_t w[U];
            T g1[U], g2[U];
#pragma unroll
            for (int u = 0; u < U; ++u) w[u] = PW[t0 + (uint32_t)(u * RS + hl)];  // (padded to a multiple of 64 with 0xFFFFFFFF)
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const uint32_t ww = (w[u] == 0xFFFFFFFFu) ? 0u : w[u];
                g1[u] = G[ww & 0xFFu];
                g2[u] = G[(ww >> 8) & 0xFFu];
            }
#pragma unroll
            for (int u = 0; u < U; ++u)
                if (w[u] != 0xFFFFFFFFu) lds_add(&At[w[u] >> 16], g1[u] * g2[u]);
        }
        for (uint32_t t0 = 0; t0 < n_pe; t0 += RS * U) {
            uint32_t w[U];
            T g1[U], rr[U];
#pragma unroll
            for (int u = 0; u < U; ++u) w[u] = PE[t0 + (uint32_t)(u * RS + hl)];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const uint32_t ww = (w[u] == 0xFFFFFFFFu) ? 0u : w[u];
                g1[u] = G[ww & 0xFFu];
                rr[u] = -R[(ww >> 8) & 0xFFu];
            }
#pragma unroll
            for (int u = 0; u < U; ++u)
                if (w[u] != 0xFFFFFFFFu) lds_add(&rhsv[w[u] >> 16], g1[u] * rr[u]);
        }
        group_sync();
#pragma unroll
        for (int q = 0; q < NC; ++q)
            if ((uint32_t)(hl + RS * q) >= nfree) At[dslot[q]] = T(1);  // identity padding
        group_sync();
#pragma unroll
        for (int q = 0; q < NC; ++q) {
            diag[q] = At[dslot[q]];
            rhs_l[q] = rhsv[hl + RS * q];
        }
    };

    // a launch over what the tiny build handed over (DeviceBatch::queue_len): mostly nothing, or a few dozen stragglers — a wavefront
    // whose first four tickets would lie past the end of that queue leaves before it has copied the program
    if (b.queue_len && !b.gc_nclasses && blockIdx.x * 4u >= rfl(*b.queue_len)) return;
    const uint32_t ncls = b.gc_nclasses ? b.gc_nclasses : 1u;
    uint32_t home = 0;
    if (b.gc_nclasses > 1u) {  // the class this wavefront's place in the grid falls into
        const unsigned long long at = (unsigned long long)blockIdx.x * b.n_systems;  // (b.n_systems: the classes' Systems in all)
        unsigned long long acc = 0;
        for (uint32_t c = 0; c < b.gc_nclasses; ++c) {
            acc += b.gc_classes[c].count;
            if (at < acc * gridDim.x) break;
            home = c + 1u < b.gc_nclasses ? c + 1u : c;
        }
    }
    for (uint32_t ci = 0; ci < ncls; ++ci) {
    {
        const uint32_t c = home + ci < ncls ? home + ci : home + ci - ncls;
        const uint32_t* prog = b.gc_tab;
        uint32_t words = sizeof(T) == 4 ? b.gc_words_all : b.gc_words;
        qn = b.n_systems;
        qlist = b.order;
        qhead = next_system;
        if (b.queue_len && !b.gc_nclasses) qn = rfl(*b.queue_len);  // (what the tiny build handed over)
        if (b.gc_nclasses) {
            const GcClass k = b.gc_classes[c];
            prog = b.gc_tab + k.prog_off;
            words = sizeof(T) == 4 ? k.words_all : k.words;
            qn = k.count;
            qlist = b.order + k.list_off;
            qbase = k.list_off;
            qhead = next_system + c;
        }
        group_sync();
        const uint4* src = reinterpret_cast<const uint4*>(prog);
        uint4* dst = reinterpret_cast<uint4*>(smem);
        for (uint32_t i = lane; i < words / 4u; i += 64) dst[i] = src[i];
        group_sync();
        nvt = rfl(TB[1]);
        net = rfl(TB[2]);
        nfree = rfl(TB[3]);
        n_pw = rfl(TB[4]);
        n_pe = rfl(TB[5]);
        nslots = rfl(TB[6]);
        PW = PE + n_pe;
        G = At + nslots;
#pragma unroll
        for (int q = 0; q < NC; ++q) {
            const uint32_t j = (uint32_t)(hl + RS * q);
            my_vi[q] = j < nfree ? (uint32_t)fidx[j] : 0u;
            dslot[q] = (uint32_t)reinterpret_cast<const uint8_t*>(LT)[(uint32_t)(N * q) + j];
        }
        phase = GP_NEXT;
        fresh = false;
        held = 0;
        lad_rank = 0;
        lad_width = 1;
        lad_lead = myrow;
        lad_members = (uint32_t)myrow * 0x55u;
        qdone = false;
        last_tk = 0;
    }
    for (;;) {
        // near the end of the queue a wavefront that holds a straggler stops taking Systems (fx_grouped.hip)
        bool park = false;
        if (prm.ladder && prm.ladder_tail != 0u) {
            const bool straggler = __ballot(phase == GP_RUN && lad_rank == 0 && !fresh && trials >= prm.ladder_k) != 0ull;
            if (phase == GP_EXIT && !qdone && !straggler) phase = GP_NEXT;
            park = straggler && last_tk < qn && qn - last_tk <= prm.ladder_tail;
        }
        // ================= NEXT: take a System, scale and perturb it (assemble/mod.rs:32-44, 91-111) =================
        if (phase == GP_NEXT && park) phase = GP_EXIT;
        if (phase == GP_NEXT) {
            uint32_t tk = 0;
            if (hl == 0) {
                tk = atomicAdd(qhead, 1u);
                last_tk = tk;
                if (tk >= qn) {
                    tk = 0xFFFFFFFFu;  // the queue is empty (a list — a schedule, or the members of a structure class — may hold
                                       // System numbers beyond the queue's length)
                } else if (STAGED) {  // the place in the list (prm.spread is 0 without one): the staged data are there
                    if (tk < 4u * prm.spread) tk = (tk & 3u) * prm.spread + (tk >> 2);
                } else if (qlist) {
                    uint32_t pos = tk;
                    if (tk < 4u * prm.spread) pos = (tk & 3u) * prm.spread + (tk >> 2);
                    tk = qlist[pos];
                }
            }
            const uint32_t nxt = (uint32_t)__shfl((int)tk, 0, RS);
            last_tk = (uint32_t)__shfl((int)last_tk, 0, RS);
            if (nxt == 0xFFFFFFFFu) {
                phase = GP_EXIT;
                qdone = true;
            } else {
                s = nxt;
                if constexpr (STAGED) {  // set up by gc_stage_kernel at the System's place in the list: one round trip for all of it
                    const uint32_t j = qbase + nxt;
                    s = b.st_sys[j];
#pragma unroll
                    for (int k = 0; k < NC; ++k)
                        if ((uint32_t)(RS * k + hl) < nvt) XS[RS * k + hl] = b.st_x[(uint32_t)N * j + (uint32_t)(RS * k + hl)];
#pragma unroll
                    for (int k = 0; k < RC; ++k)
                        if ((uint32_t)(RS * k + hl) < net) P[RS * k + hl] = b.st_p[(uint32_t)(RS * RC) * j + (uint32_t)(RS * k + hl)];
                    if (hl == 0) STASH[0] = b.st_scale[j];
                } else {
                // (a launch over ONE structure class of a batch of several — b.uniform == 0 — reads the System's offsets)
                const uint32_t v0 = b.uniform ? s * nvt : b.var_off[s], e0 = b.uniform ? s * net : b.expr_off[s];
                double c_var[NC], c_param[RC];
                int tagk[RC], colk[NC];
#pragma unroll
                for (int k = 0; k < NC; ++k) {
                    const uint32_t i = (uint32_t)(RS * k + hl);
                    c_var[k] = i < nvt ? (b.vars_in ? b.vars_in : b.vars0)[v0 + i] : 0.0;
                    colk[k] = i < nvt ? (int)vcol[i] : -1;
                }
#pragma unroll
                for (int k = 0; k < RC; ++k) {
                    const uint32_t i = (uint32_t)(RS * k + hl);
                    c_param[k] = i < net ? (b.param_in ? b.param_in : b.expr_param)[e0 + i] : 0.0;
                    tagk[k] = i < net ? (int)rtag[i] : 0;
                }
                if (b.param_in) {  // (the closing check reads them again: from the device's copy, not over the link)
#pragma unroll
                    for (int k = 0; k < RC; ++k)
                        if ((uint32_t)(RS * k + hl) < net) b.expr_param[e0 + (uint32_t)(RS * k + hl)] = c_param[k];
                }
                if (b.vars_in) {  // (start values stay on the device: a refused hint puts them back, fx_solve.cpp)
#pragma unroll
                    for (int k = 0; k < NC; ++k)
                        if ((uint32_t)(RS * k + hl) < nvt) b.vars0[v0 + (uint32_t)(RS * k + hl)] = c_var[k];
                }
                __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0)
                // K0a: system scale; K0b: the perturbation (gc_setup)
                double x[NC], pe[RC];
                const double scale = gc_setup<NC, RC>(prm.mode, nvt, net, hl, gbase, c_var, colk, c_param, tagk, x, pe);
#pragma unroll
                for (int k = 0; k < NC; ++k) {
                    const uint32_t i = (uint32_t)(RS * k + hl);
                    if (i < nvt) {
                        XS[i] = (T)x[k];  // (perturbed from the f64 input: the f64 start point is bit-identical to the reference)
                        VOUT[i] = c_var[k];
                        b.vars[v0 + i] = c_var[k];  // fixed variables stay bit-identical
                    }
                }
#pragma unroll
                for (int k = 0; k < RC; ++k)
                    if ((uint32_t)(RS * k + hl) < net) P[RS * k + hl] = (T)pe[k];
                if (hl == 0) STASH[0] = scale;
                }
                group_sync();
#pragma unroll
                for (int q = 0; q < NC; ++q) xc[q] = ((uint32_t)(hl + RS * q) < nfree) ? XS[my_vi[q]] : T(0);
                lambda = o.lambda0;
                accepted = 0;
                trials = 0;
                outer = 0;
                exit_code = FX_EXIT_MAX_OUTER;
                fresh = true;
                phase = GP_RUN;
            }
        }

        // ================= LADDER: idle rows join a running row of their wavefront (fx_grouped.hip) =================
        if (prm.ladder) {
            const unsigned long long bcand = __ballot(phase == GP_RUN && !fresh && lad_rank == 0);
            const unsigned long long bidle = __ballot(phase == GP_EXIT);
            if (bcand != 0ull && bidle != 0ull) {
                uint32_t wid = 0, mem = 0, newlead = 0xFFFFu, newrank = 0;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    wid |= ((uint32_t)__builtin_amdgcn_readlane(lad_width, RS * r) & 15u) << (4 * r);
                    mem |= ((uint32_t)__builtin_amdgcn_readlane((int)lad_members, RS * r) & 255u) << (8 * r);
                }
                bool anyjoin = false;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    if (!((bidle >> (RS * r)) & 1ull)) continue;
                    uint32_t best = 15u, bw = 4u;
#pragma unroll
                    for (int l = 0; l < 4; ++l) {
                        const uint32_t w = (wid >> (4 * l)) & 15u;
                        if (((bcand >> (RS * l)) & 1ull) && w < bw) {
                            best = (uint32_t)l;
                            bw = w;
                        }
                    }
                    if (best != 15u) {
                        newlead = (newlead & ~(15u << (4 * r))) | (best << (4 * r));
                        newrank |= bw << (4 * r);
                        const uint32_t at = 8u * best + 2u * bw;
                        mem = (mem & ~(3u << at)) | ((uint32_t)r << at);
                        wid += 1u << (4u * best);
                        anyjoin = true;
                    }
                }
                if (anyjoin) {
                    const uint32_t nl = (newlead >> (4 * myrow)) & 15u;
                    const bool joining = nl != 15u;
                    const int grp = joining ? (int)nl : lad_lead;
                    const int srcl = grp * RS + hl;
                    auto cp = [&](auto& v) {
                        const auto t = lane_get(v, srcl);
                        if (joining) v = t;
                    };
                    cp(trials); cp(accepted); cp(outer); cp(exit_code);
                    cp(sse); cp(lambda);
#pragma unroll
                    for (int q = 0; q < NC; ++q) {
                        cp(xc[q]); cp(diag[q]); cp(rhs_l[q]);
                    }
                    lad_width = (int)((wid >> (4 * grp)) & 15u);
                    lad_members = (mem >> (8 * grp)) & 255u;
                    if (joining) {
                        lad_lead = (int)nl;
                        lad_rank = (int)((newrank >> (4 * myrow)) & 15u);
                        const uint4* lb = reinterpret_cast<const uint4*>(rows0 + (uint32_t)nl * L.stride);
                        uint4* mine = reinterpret_cast<uint4*>(base);
                        for (uint32_t i = hl; i < L.stride / 16u; i += RS) mine[i] = lb[i];
                        fresh = false;
                        phase = GP_RUN;
                    }
                    group_sync();
                }
            }
        }

        // ================= RUN: one lambda trial (lm.rs:115-191) =================
        if (phase == GP_RUN) {
            int code = LC_FRESH;
            bool go = true;
            T delta[NC];
#pragma unroll
            for (int q = 0; q < NC; ++q) delta[q] = T(0);
            if (!fresh) {
                code = LC_REJECT;
                double lam_k = lambda;
                if (lad_rank > 0)
                    for (int k = 0; k < lad_rank; ++k) lam_k *= o.reject_factor;
                if (trials + (uint32_t)lad_rank >= o.max_trials) {
                    code = LC_CAP;
                    go = false;
                }
                if (go) {
                    // K4: factor (Jt J + lambda I) and solve for delta; columns hl and hl + 16 of the symmetric matrix through
                    // the lane's table of slots
#pragma unroll
                    for (int q = 0; q < NC; ++q) At[dslot[q]] = diag[q] + (T)lam_k;
                    group_sync();
                    T a[NC][N];
#pragma unroll
                    for (int cch = 0; cch < NC * N / 16; ++cch) {
                        const uint4 w4 = LT[cch];
                        const uint32_t ws[4] = {w4.x, w4.y, w4.z, w4.w};
#pragma unroll
                        for (int e = 0; e < 16; ++e) {
                            const int el = 16 * cch + e;
                            // (a band factor: an element that lies outside the envelope in every lane is a structural zero, and
                            // its slot would be the zero slot)
                            if (RBand<NC, W, B>::zero_row(el / N, el % N)) a[el / N][el % N] = T(0);
                            else a[el / N][el % N] = At[(ws[e / 4] >> (8 * (e % 4))) & 0xFFu];
                        }
                    }
                    T invd[NC];
#pragma unroll
                    for (int q = 0; q < NC; ++q) invd[q] = T(1);
                    bool bad = false;
                    // (two columns per lane: the forward substitution runs inside the factorization, a step behind each pivot;
                    // the one-column build keeps its own pass, where the fused form cost it scratch)
                    constexpr bool FWD = NC == 2;
                    T acc[NC];
#pragma unroll
                    for (int q = 0; q < NC; ++q) acc[q] = rhs_l[q];
                    RBlock<NC, T, 0, false, W, B>::template factor<FWD>(a, invd, acc, bad, hl, N);
                    if (bad) {  // lm.rs:134-137
                        code = LC_SINGULAR;
                        go = false;
                    } else {
                        T invd2[NC];
#pragma unroll
                        for (int q = 0; q < NC; ++q) invd2[q] = invd[q] * invd[q];
                        if constexpr (!FWD) RBlock<NC, T, 0, false>::forward(a, invd, acc, hl, N);
                        RBlock<NC, T, N / 8 - 1, false>::backward(a, invd2, acc, hl, N);
#pragma unroll
                        for (int q = 0; q < NC; ++q) delta[q] = ((uint32_t)(hl + RS * q) < nfree) ? acc[q] * invd2[q] : T(0);
                    }
                }
                if (go) {
                    T dsq[NC];
#pragma unroll
                    for (int q = 0; q < NC; ++q) dsq[q] = delta[q] * delta[q];
                    const T dn2 = chunk_sum(dsq);
                    if (!(dn2 == dn2)) {
                        code = LC_NAN;
                        go = false;
                    } else if (dn2 < (T)o.step_tol) {  // lm.rs:139-142
                        code = LC_STEP;
                        go = false;
                    }
                }
                if (go) {
#pragma unroll
                    for (int q = 0; q < NC; ++q)
                        if ((uint32_t)(hl + RS * q) < nfree) XS[my_vi[q]] = xc[q] + delta[q];
                    group_sync();
                }
            }
            T sse_t = T(0);
            if (go) {
                sse_t = eval_rows();
                if (!fresh) {
                    if (sse_t < sse) {
                        code = LC_ACCEPT;  // lm.rs:151-186
                    } else {               // lm.rs:187-190
                        double lam_k = lambda * o.reject_factor;
                        if (lad_rank > 0)
                            for (int k = 0; k < lad_rank; ++k) lam_k *= o.reject_factor;
                        if (!(sse_t == sse_t) && !(lam_k < 1.0e300)) code = LC_REJ_NAN;  // the reference would double lambda forever
                        else if (sizeof(T) == 4 && sse_t - sse <= (T)o.ftol * sse) code = LC_REJ_FTOL;  // f32: stagnated at round-off (fx_grouped.hip)
                    }
                }
            }
            // --- the verdicts of a ladder group in rank order: the first that is not a plain reject decides
            int kw = (code != LC_REJECT) ? 0 : 1;
            int code_w = code;
            T sse_w = sse_t;
            T delta_w[NC];
#pragma unroll
            for (int q = 0; q < NC; ++q) delta_w[q] = delta[q];
            win_row = myrow;
            if (__ballot(lad_width > 1) != 0ull) {
                int ck[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) ck[k] = lane_get(code, (int)((lad_members >> (2 * k)) & 3u) * RS + hl);
                kw = lad_width;
                code_w = LC_REJECT;
#pragma unroll
                for (int k = 3; k >= 0; --k) {
                    if (k < lad_width && ck[k] != LC_REJECT) {
                        kw = k;
                        code_w = ck[k];
                    }
                }
                const int wrow = (int)((lad_members >> (2 * (kw < lad_width ? kw : 0))) & 3u);
                const int wl = wrow * RS + hl;
                sse_w = lane_get(sse_t, wl);
#pragma unroll
                for (int q = 0; q < NC; ++q) delta_w[q] = lane_get(delta[q], wl);
                win_row = wrow;
            }
            bool assemble = false, fin = false;
            if (fresh) {  // the start point
                sse = sse_t;
                if (hl == 0) STASH[1] = (double)sse_t;
                assemble = true;
            } else {
                if (kw > 0) {  // the plain rejects in front (lm.rs:189)
                    lambda *= o.reject_factor;
                    for (int k = 1; k < kw; ++k) lambda *= o.reject_factor;
                }
                if (kw == lad_width) {
                    trials += (uint32_t)kw;
                } else {
                    trials += (uint32_t)kw + (code_w != LC_CAP ? 1u : 0u);
                    if (code_w == LC_CAP) {
                        exit_code = FX_EXIT_TRIAL_CAP;
                        fin = true;
                    } else if (code_w == LC_SINGULAR) {  // lm.rs:134-137
                        lambda *= o.singular_factor;
                    } else if (code_w == LC_NAN) {
                        exit_code = FX_EXIT_NAN;
                        fin = true;
                    } else if (code_w == LC_STEP) {  // lm.rs:139-142
                        exit_code = FX_EXIT_STEP;
                        fin = true;
                    } else if (code_w == LC_ACCEPT) {  // lm.rs:151-186
                        lambda *= o.accept_factor;
                        if (lambda < o.lambda_min) lambda = o.lambda_min;
#pragma unroll
                        for (int q = 0; q < NC; ++q)
                            if ((uint32_t)(hl + RS * q) < nfree) xc[q] = xc[q] + delta_w[q];
                        accepted += 1;
                        const T rel = (sse - sse_w) / sse;
                        sse = sse_w;
                        if (rel <= (T)o.ftol) {
                            exit_code = FX_EXIT_FTOL;
                            fin = true;
                        } else {
                            assemble = true;
                            outer += 1;
                        }
                    } else {  // a reject that ends the solve
                        lambda *= o.reject_factor;
                        exit_code = (code_w == LC_REJ_NAN) ? FX_EXIT_NAN : FX_EXIT_FTOL;
                        fin = true;
                    }
                }
            }
            if (assemble) {
                if (win_row != myrow) {  // the accepted point's Jacobian rows and residuals are another row's
                    const unsigned char* wb = rows0 + (uint32_t)win_row * L.stride;
                    const uint32_t off_g = BK::A + nslots * (uint32_t)sizeof(T);
                    const uint4* gs = reinterpret_cast<const uint4*>(wb + off_g);
                    uint4* gd = reinterpret_cast<uint4*>(G);
                    const uint32_t ng2 = (L.stride - off_g) / 16u;
                    for (uint32_t i = hl; i < ng2; i += RS) gd[i] = gs[i];
                    const T* rs = reinterpret_cast<const T*>(wb + BK::R);
#pragma unroll
                    for (int k = 0; k < RC; ++k) R[hl + RS * k] = rs[hl + RS * k];
                    group_sync();
                }
                form_normal();
                // top of the next outer iteration (lm.rs:108-112)
                if (fresh && (!(sse == sse) || !(sse < Lim<T>::huge()))) {
                    exit_code = FX_EXIT_NAN;
                    fin = true;
                } else if (outer >= o.max_outer) {
                    fin = true;  // exit_code is still FX_EXIT_MAX_OUTER
                } else if (sse < (T)o.sse_tol) {
                    exit_code = FX_EXIT_SSE;
                    fin = true;
                }
            }
            fresh = false;
            if (fin) {
                phase = GP_FINISH;
                if (lad_rank > 0) phase = GP_EXIT;  // a helper goes back to being an idle row; the leader writes the System back
                lad_rank = 0;
                lad_width = 1;
                lad_lead = myrow;
                lad_members = (uint32_t)myrow * 0x55u;
            }
        }

        // a row that is done waits up to prm.hold_passes passes for company (fx_grouped.hip)
        bool finish_now = phase == GP_FINISH;
        if (prm.hold_passes) {
            const int n_done = __popcll(__ballot(phase == GP_FINISH)) / RS;
            const bool any_running = __ballot(phase == GP_RUN) != 0ull;
            if (phase == GP_FINISH) {
                if (n_done >= 2 || !any_running || held >= prm.hold_passes) {
                    held = 0;
                } else {
                    held += 1;
                    finish_now = false;
                }
            }
        }
        // ================= FINISH: write back scale * x (assemble/mod.rs:161-166), the closing check
        // (constraints/mod.rs:96-109), the result record =================
        if (finish_now) {
            const uint32_t v0 = b.uniform ? s * nvt : b.var_off[s], e0 = b.uniform ? s * net : b.expr_off[s];
            const double scale = STASH[0];
            double sse_u = 0.0;  // (a staged build: gc_close_kernel fills it in)
            if constexpr (STAGED) {
#pragma unroll
                for (int q = 0; q < NC; ++q) {
                    if ((uint32_t)(hl + RS * q) < nfree) {
                        const double x = (double)xc[q];
                        const double xo = (prm.mode & 1u) ? scale * x : x;
                        b.vars[v0 + my_vi[q]] = xo;
                        if (b.vars_out) b.vars_out[v0 + my_vi[q]] = xo;
                    }
                }
            } else {
            double c_param[RC];  // the unscaled parameters of expressions hl, hl + 16, ...
#pragma unroll
            for (int k = 0; k < RC; ++k) c_param[k] = (uint32_t)(RS * k + hl) < net ? b.expr_param[e0 + (uint32_t)(RS * k + hl)] : 0.0;
#pragma unroll
            for (int q = 0; q < NC; ++q) {
                if ((uint32_t)(hl + RS * q) < nfree) {
                    const double x = (double)xc[q];
                    const double xo = (prm.mode & 1u) ? scale * x : x;
                    b.vars[v0 + my_vi[q]] = xo;
                    if (b.vars_out) b.vars_out[v0 + my_vi[q]] = xo;
                    VOUT[my_vi[q]] = xo;
                }
            }
            group_sync();
            double part[RC];
#pragma unroll
            for (int k = 0; k < RC; ++k) {
                const uint32_t i = (uint32_t)(hl + RS * k);
                part[k] = 0.0;
                if (i < net) {
                    double v[8], g[8];
                    const uint2 gv = gvar[i];
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[e] = VOUT[(gv.x >> (8 * e)) & 0xFFu];
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[4 + e] = VOUT[(gv.y >> (8 * e)) & 0xFFu];
                    const double r = eval_expression<double, false, false>((int)rtag[i], v, c_param[k], g);
                    part[k] = r * r;
                }
            }
            sse_u = rows_sum(part);
            }
            if (hl == 0) {
                fx_result res;
                res.accepted = accepted;
                res.trials = trials;
                res.exit = exit_code;
                res.ncomp = 1;
                res.scale = scale;
                res.sse0 = STASH[1];
                res.sse = (double)sse;
                res.sse_unscaled = sse_u;
                b.results[s] = res;
                if (b.results_out) b.results_out[s] = res;
            }
            group_sync();
            phase = GP_NEXT;
        }

        if (__ballot(phase != GP_EXIT || (prm.ladder && !qdone)) == 0ull) break;
    }
    }  // the next class's queue
}

typedef void (*GcKernel)(DeviceBatch, LmParams, GcLayout, uint32_t*);
struct GcBuild {
    GcKernel fn;
    unsigned int* raised;   // (raise_lds_limit_once's per-device bits)
    uint32_t waves_per_cu;  // by registers
};
// fx_grouped_band.hip: the two-column f64 kernel with the factor of GC_BANDS[band - 1] (staged: its build for a staged set-up and
// closing check); fn == nullptr: no such build
GcBuild gc_band_build(uint32_t band, bool staged);

}  // namespace fx
