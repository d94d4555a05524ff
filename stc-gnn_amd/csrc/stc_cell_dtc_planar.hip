// The gradient of the category graph's Chebyshev stack T_c from the PLANAR cells of the cell-graph executor (graph_mode 'csr-category-learned':
// a fixed sparse spatial graph, a learned category graph; ABI v43).  Order 2, hidden 16, fp32 planes (rows, C, w), C in {32, 64}; T_0 = I is a
// constant, so only dT_c[1] is formed:
//     gates      V[r][c][:] = [X|H][r][c][:] . Wg[block (0, 1)] + [SX|SH][r][c][:] . Wg[block (1, 1)]                        32 columns
//                dG[r][d][:] = [ dHnew (Cand - H) U (1 - U) | dRH H R (1 - R) ]                                              re-formed, never stored
//                partial[c][d] += sum_o V[r][c][o] dG[r][d][o]
//     candidate  V[r][c][:] = [ [X|RH][r][c][:] . Wc[block (0, 1)] | [X|RH][r][c][:] . Wc[block (1, 1)] ]                   16 + 16 columns
//                partial[c][d] += sum_o V[r][c][o] [dY | dBm][r][d][o]            (dBm = S^T dY: the aggregated slab S.[X|RH] is not needed)
// with block (n, kc) = the L = cin + 16 rows of W from (2 n + kc) L, input columns first.  Both forms are one kernel: NZ input rows per
// category (2 / 1), a table of NZ x LP x 32 weights in LDS, 32 gradient columns per category.
//
// A workgroup owns DTC_RUN consecutive rows (the grid is sized from the row count; no stride loop) and walks them in order.  Per row:
// stage the input row(s) and the 32 gradient columns in LDS; V = Z . W as fp32 fmaf chains (one category and C / 8 columns per thread);
// the C x C outer product over the 32 columns as fp32 fmaf chains (a (C/16) x (C/16) tile per thread), each finished dot product added to the
// thread's FLOAT64 accumulator.  The next row's planes are requested before the current row's products.  After its last row the workgroup ADDS
// its accumulators to its own slot of `partials` (slots, C, C): no atomics, one fixed order -- bitwise reproducible; the caller zeroes the
// buffer once, every launch of a backward pass adds, one sum over the slots finishes dT_c[1].
#include "stc_cell_dtc_gate.h"

namespace {

using stc_dtc::v4f;
constexpr int DTC_RUN = 256;               // consecutive rows of one workgroup = rows per slot of `partials`
constexpr int DTC_THREADS = 256;
constexpr int DTC_H = stc_dtc::H, DTC_COLS = stc_dtc::COLS;   // hidden width; gradient columns per category (gates: update | reset; candidate: dY | dBm)
constexpr int DTC_GS = stc_dtc::GS;        // LDS row stride of the V and gradient tiles (16 rows land on 16 different banks of four)

struct DtcPlanes {
    const float* x[2];        // input planes (rows, C, cin): X, SX (candidate: X)
    const float* h[2];        // state planes (rows, C, 16): H, SH (candidate: R*H)
    const float* g[5];        // gates: dHnew, Cand, U, dRH, R; candidate: dY, dBm
};

template <int C, int XW, bool GATES>       // XW: columns the input plane takes in LDS (16: a wide plane, 4: cin in 1..4, zero-filled)
__global__ __launch_bounds__(DTC_THREADS) void dtc_planar_kernel(DtcPlanes p, const float* __restrict__ W, double* __restrict__ part, int cin, long long rows) {
    constexpr int NZ = GATES ? 2 : 1, LP = XW + DTC_H, ZS = XW == 16 ? LP + 4 : LP;
    constexpr int HP = NZ * C * 4, HK = (HP + DTC_THREADS - 1) / DTC_THREADS;            // 16-byte pieces of the state planes of one row, per thread
    constexpr int XP = XW == 16 ? HP : 0, XK = (XP + DTC_THREADS - 1) / DTC_THREADS;     // ... of wide input planes
    constexpr int GK = C * 8 / DTC_THREADS;                                              // ... of the 32 gradient columns
    constexpr int OPT = C / 8, T = C / 16;                                               // V columns per thread; side of a thread's tile of the outer product
    __shared__ __attribute__((aligned(16))) float ws[NZ][LP][DTC_COLS];
    __shared__ __attribute__((aligned(16))) float zs[NZ][C][ZS];
    __shared__ __attribute__((aligned(16))) float gs[2][C][DTC_GS];
    __shared__ __attribute__((aligned(16))) float vs[C][DTC_GS];
    const int tid = threadIdx.x;
    const long long r0 = (long long)blockIdx.x * DTC_RUN, r1 = r0 + DTC_RUN < rows ? r0 + DTC_RUN : rows;
    if (r0 >= r1) return;
    const int L = cin + DTC_H;

    // the weight table: rows of the input columns first (beyond cin: zero), then the 16 state rows
    for (int i = tid; i < NZ * LP * DTC_COLS; i += DTC_THREADS) {
        const int n = i / (LP * DTC_COLS), l = i / DTC_COLS % LP, o = i % DTC_COLS;
        const bool live = l >= XW || l < cin;
        const int lrow = l < XW ? l : cin + l - XW;
        float w = 0.f;
        if (live) w = GATES ? W[(size_t)((2 * n + 1) * L + lrow) * DTC_COLS + o] : W[(size_t)((2 * (o / DTC_H) + 1) * L + lrow) * DTC_H + o % DTC_H];
        ws[n][l][o] = w;
    }

    v4f hr[HK], xr[XK > 0 ? XK : 1], ga[GK], gb[GK], gc[GK], gd[GK];
    float xn[4];
    const v4f zero = {0.f, 0.f, 0.f, 0.f};
    const stc_dtc::GatePlanes gp{p.g[0], p.g[1], p.g[2], p.g[3], p.g[4], p.h[0]};     // (gates: the planes the gate gradient is re-formed from)
    auto request = [&](long long r) {                                  // one row's planes into registers
        const size_t row16 = (size_t)r * C * DTC_H;
#pragma unroll
        for (int k = 0; k < HK; ++k) {
            const int q = tid + DTC_THREADS * k;                       // piece (n, c, part)
            hr[k] = q < HP ? *reinterpret_cast<const v4f*>(p.h[q / (C * 4)] + row16 + (size_t)(q % (C * 4)) * 4) : zero;
        }
        if constexpr (XW == 16) {
#pragma unroll
            for (int k = 0; k < XK; ++k) {
                const int q = tid + DTC_THREADS * k;
                xr[k] = q < XP ? *reinterpret_cast<const v4f*>(p.x[q / (C * 4)] + row16 + (size_t)(q % (C * 4)) * 4) : zero;
            }
        } else {
            const float* src = p.x[tid < NZ * C ? tid / C : 0] + ((size_t)r * C + tid % C) * cin;
#pragma unroll
            for (int j = 0; j < 4; ++j) xn[j] = (tid < NZ * C && j < cin) ? src[j] : 0.f;
        }
#pragma unroll
        for (int k = 0; k < GK; ++k) {
            const int q = tid + DTC_THREADS * k;                       // piece (d, part): columns 4 part .. 4 part + 3 of category d
            const size_t at = row16 + (size_t)(q >> 3) * DTC_H + (size_t)(q & 3) * 4;
            const bool second = (q & 7) >= 4;
            if constexpr (GATES) {
                const stc_dtc::GatePiece g = stc_dtc::gate_request(gp, at, second);               // dRH : dHnew | H | R : U | Cand
                ga[k] = g.a, gb[k] = g.b, gc[k] = g.c, gd[k] = g.d;
            } else {
                ga[k] = *reinterpret_cast<const v4f*>((second ? p.g[1] : p.g[0]) + at);           // dBm : dY
            }
        }
    };
    auto stage = [&](int buf) {                                        // registers -> LDS; the gate gradient is formed here
#pragma unroll
        for (int k = 0; k < HK; ++k) {
            const int q = tid + DTC_THREADS * k;
            if (q < HP) *reinterpret_cast<v4f*>(&zs[q / (C * 4)][q / 4 % C][XW + 4 * (q & 3)]) = hr[k];
        }
        if constexpr (XW == 16) {
#pragma unroll
            for (int k = 0; k < XK; ++k) {
                const int q = tid + DTC_THREADS * k;
                if (q < XP) *reinterpret_cast<v4f*>(&zs[q / (C * 4)][q / 4 % C][4 * (q & 3)]) = xr[k];
            }
        } else if (tid < NZ * C) {
            const v4f x4 = {xn[0], xn[1], xn[2], xn[3]};
            *reinterpret_cast<v4f*>(&zs[tid / C][tid % C][0]) = x4;
        }
#pragma unroll
        for (int k = 0; k < GK; ++k) {
            const int q = tid + DTC_THREADS * k;
            v4f g;
            if constexpr (GATES) {
                g = stc_dtc::gate_form(stc_dtc::GatePiece{ga[k], gb[k], gc[k], gd[k]}, (q & 7) >= 4);
            } else {
                g = ga[k];
            }
            *reinterpret_cast<v4f*>(&gs[buf][q >> 3][4 * (q & 7)]) = g;
        }
    };

    double acc[T][T];
#pragma unroll
    for (int a = 0; a < T; ++a)
#pragma unroll
        for (int b = 0; b < T; ++b) acc[a][b] = 0.0;
    const int vc = tid % C, vo = tid / C * OPT;                        // V: category, first column
    const int ci = tid & 15, di = tid >> 4;                            // outer product: categories ci + 16 a, di + 16 b

    request(r0);
    for (long long r = r0; r < r1; ++r) {
        const int buf = (int)(r - r0) & 1;
        stage(buf);
        if (r + 1 < r1) request(r + 1);
        __syncthreads();
        float v[OPT];
#pragma unroll
        for (int j = 0; j < OPT; ++j) v[j] = 0.f;
#pragma unroll
        for (int n = 0; n < NZ; ++n)
#pragma unroll
            for (int l4 = 0; l4 < LP / 4; ++l4) {
                const v4f z = *reinterpret_cast<const v4f*>(&zs[n][vc][4 * l4]);
#pragma unroll
                for (int e = 0; e < 4; ++e)
#pragma unroll
                    for (int j4 = 0; j4 < OPT / 4; ++j4) {
                        const v4f w = *reinterpret_cast<const v4f*>(&ws[n][4 * l4 + e][vo + 4 * j4]);
#pragma unroll
                        for (int i = 0; i < 4; ++i) v[4 * j4 + i] = fmaf(z[e], w[i], v[4 * j4 + i]);
                    }
            }
#pragma unroll
        for (int j4 = 0; j4 < OPT / 4; ++j4) {
            const v4f o4 = {v[4 * j4], v[4 * j4 + 1], v[4 * j4 + 2], v[4 * j4 + 3]};
            *reinterpret_cast<v4f*>(&vs[vc][vo + 4 * j4]) = o4;
        }
        __syncthreads();
        float s[T][T];
#pragma unroll
        for (int a = 0; a < T; ++a)
#pragma unroll
            for (int b = 0; b < T; ++b) s[a][b] = 0.f;
#pragma unroll
        for (int o4 = 0; o4 < DTC_COLS / 4; ++o4) {
            v4f va[T], gv[T];
#pragma unroll
            for (int a = 0; a < T; ++a) va[a] = *reinterpret_cast<const v4f*>(&vs[ci + 16 * a][4 * o4]);
#pragma unroll
            for (int b = 0; b < T; ++b) gv[b] = *reinterpret_cast<const v4f*>(&gs[buf][di + 16 * b][4 * o4]);
#pragma unroll
            for (int a = 0; a < T; ++a)
#pragma unroll
                for (int b = 0; b < T; ++b)
#pragma unroll
                    for (int e = 0; e < 4; ++e) s[a][b] = fmaf(va[a][e], gv[b][e], s[a][b]);
        }
#pragma unroll
        for (int a = 0; a < T; ++a)
#pragma unroll
            for (int b = 0; b < T; ++b) acc[a][b] += (double)s[a][b];
    }
    double* out = part + (size_t)blockIdx.x * C * C;
#pragma unroll
    for (int a = 0; a < T; ++a)
#pragma unroll
        for (int b = 0; b < T; ++b) out[(ci + 16 * a) * C + di + 16 * b] += acc[a][b];
}

template <bool GATES>
void dtc_launch(const DtcPlanes& p, const float* W, double* partials, int cin, long long rows, int C, hipStream_t stream) {
    const dim3 grid((unsigned)((rows + DTC_RUN - 1) / DTC_RUN)), block(DTC_THREADS);
    if (C == 32 && cin == 16) hipLaunchKernelGGL((dtc_planar_kernel<32, 16, GATES>), grid, block, 0, stream, p, W, partials, cin, rows);
    else if (C == 32) hipLaunchKernelGGL((dtc_planar_kernel<32, 4, GATES>), grid, block, 0, stream, p, W, partials, cin, rows);
    else if (cin == 16) hipLaunchKernelGGL((dtc_planar_kernel<64, 16, GATES>), grid, block, 0, stream, p, W, partials, cin, rows);
    else hipLaunchKernelGGL((dtc_planar_kernel<64, 4, GATES>), grid, block, 0, stream, p, W, partials, cin, rows);
}

// what both entry points check before any HIP call
int dtc_checked(const char* who, int32_t cin, int64_t rows, int32_t C) {
    STC_REQUIRE(stc_cell_dtc_planar_supported(C, cin, DTC_H), STC_EINVAL, "%s: C in (32, 64), cin = 16 or 1..4; got C=%d cin=%d", who, C, cin);
    STC_REQUIRE(rows >= 0 && rows < (1ll << 31), STC_EINVAL, "%s: rows=%lld outside [0, 2^31)", who, (long long)rows);
    return STC_OK;
}

}  // namespace

extern "C" int stc_cell_dtc_planar_supported(int32_t C, int32_t cin, int32_t h) {
    return (C == 32 || C == 64) && h == DTC_H && (cin == DTC_H || (cin >= 1 && cin <= 4));
}

extern "C" size_t stc_cell_dtc_planar_slots(int64_t rows) { return rows <= 0 ? 0 : (size_t)((rows + DTC_RUN - 1) / DTC_RUN); }

extern "C" int stc_cell_dtc_gates_planar_f32(const float* X, int32_t cin, const float* H, const float* SX, const float* SH, const float* Wg, const float* U,
                                             const float* R, const float* Cand, const float* dHnew, const float* dRH, double* partials, int64_t rows,
                                             int32_t C, void* stream) {
    const char* who = "stc_cell_dtc_gates_planar_f32";
    if (int rc = dtc_checked(who, cin, rows, C)) return rc;
    if (rows == 0) return STC_OK;
    STC_REQUIRE(X && H && SX && SH && Wg && U && R && Cand && dHnew && dRH && partials, STC_EINVAL, "%s: null operand", who);
    const uintptr_t xa = cin == DTC_H ? 16 : 4;                          // a narrow input plane is read by the float
    for (const float* q : {H, SH, U, R, Cand, dHnew, dRH})
        STC_REQUIRE(stc::aligned16(q), STC_EALIGN, "%s: state-sized planes must be 16-byte aligned", who);
    STC_REQUIRE(stc::aligned(X, xa) && stc::aligned(SX, xa) && stc::aligned(Wg, 4) && stc::aligned(partials, 8), STC_EALIGN,
                "%s: unaligned operand (input planes %d-byte, Wg 4-byte, partials 8-byte)", who, (int)xa);
    const DtcPlanes p{{X, SX}, {H, SH}, {dHnew, Cand, U, dRH, R}};
    dtc_launch<true>(p, Wg, partials, cin, rows, C, static_cast<hipStream_t>(stream));
    STC_LAUNCH_CHECK("stc_cell_dtc_gates_planar_f32 launch");
    return STC_OK;
}

extern "C" int stc_cell_dtc_cand_planar_f32(const float* X, int32_t cin, const float* RH, const float* Wc, const float* dY, const float* dBm, double* partials,
                                            int64_t rows, int32_t C, void* stream) {
    const char* who = "stc_cell_dtc_cand_planar_f32";
    if (int rc = dtc_checked(who, cin, rows, C)) return rc;
    if (rows == 0) return STC_OK;
    STC_REQUIRE(X && RH && Wc && dY && dBm && partials, STC_EINVAL, "%s: null operand", who);
    const uintptr_t xa = cin == DTC_H ? 16 : 4;
    for (const float* q : {RH, dY, dBm})
        STC_REQUIRE(stc::aligned16(q), STC_EALIGN, "%s: state-sized planes must be 16-byte aligned", who);
    STC_REQUIRE(stc::aligned(X, xa) && stc::aligned(Wc, 4) && stc::aligned(partials, 8), STC_EALIGN,
                "%s: unaligned operand (input plane %d-byte, Wc 4-byte, partials 8-byte)", who, (int)xa);
    const DtcPlanes p{{X, X}, {RH, RH}, {dY, dBm, nullptr, nullptr, nullptr}};
    dtc_launch<false>(p, Wc, partials, cin, rows, C, static_cast<hipStream_t>(stream));
    STC_LAUNCH_CHECK("stc_cell_dtc_cand_planar_f32 launch");
    return STC_OK;
}
