// The d(S.x) plane of a PLANAR cell with a NARROW input (layer 0: cin = 1..4 columns), which the planar gates backward does not form because the
// input itself needs no gradient -- but the value gradient of a LEARNED spatial graph does (graph_mode 'csr-learned' inside the cell-graph
// executor, ABI v44: dval[e] takes < d(S.x)[i(e)], x[colidx[e]] >).  Order 2, hidden 16, fp32 planes, C in {32, 64}:
//     dSx[r][c][l] = sum_o dG[r][c][o] Wg[block (1, 0)][l][o] + sum_d Tc[1][c][d] sum_o dG[r][d][o] Wg[block (1, 1)][l][o]          l < cin
// with dG the gate gradient of stc_cell_dtc_gate.h (re-formed in registers, as stc_cell_dtc_gates_planar_f32 forms it) and block (n, kc) the
// L = cin + 16 rows of Wg from (2 n + kc) L, input columns first.  The plane is WRITTEN.
//
// A workgroup owns DSX_RUN consecutive rows (the grid is sized from the row count; no stride loop), DSX_THREADS / (4 C) of them per step: thread
// (row, category c, column l) forms Q = dG[c] . W10[l] and P = dG[c] . W11[l] as fp32 fmaf chains over the 32 gradient columns, leaves P in
// LDS and then mixes the categories: Q + sum_d Tc[1][c][d] P[d][l], one more fmaf chain.  The next step's planes are requested before the
// current step's products.  No atomics, no scratch; every element of the plane has one owner.
#include "stc_cell_dtc_gate.h"

namespace {

using stc_dtc::v4f;
constexpr int DSX_RUN = 256;               // consecutive rows of one workgroup (that of the dT_c kernels)
constexpr int DSX_THREADS = 256;
constexpr int DSX_H = stc_dtc::H, DSX_COLS = stc_dtc::COLS, DSX_GS = stc_dtc::GS;

template <int C>
__global__ __launch_bounds__(DSX_THREADS) void dsx_narrow_kernel(stc_dtc::GatePlanes gp, const float* __restrict__ Wg, const float* __restrict__ Tc1,
                                                                 float* __restrict__ dSx, int cin, long long rows) {
    constexpr int RI = DSX_THREADS / (4 * C);                  // rows per step: 2 (C = 32), 1 (C = 64)
    constexpr int GK = RI * C * 8 / DSX_THREADS;               // 16-byte pieces of the gradient columns of one step, per thread (= 2)
    __shared__ __attribute__((aligned(16))) float ws[2][4][DSX_COLS];      // Wg[block (1, kc)][l][:], rows beyond cin: zero
    __shared__ float tc[C][C + 1];
    __shared__ __attribute__((aligned(16))) float gs[RI][C][DSX_GS];
    __shared__ __attribute__((aligned(16))) float ps[RI][C][4];
    const int tid = threadIdx.x;
    const long long r0 = (long long)blockIdx.x * DSX_RUN, r1 = r0 + DSX_RUN < rows ? r0 + DSX_RUN : rows;
    if (r0 >= r1) return;
    const int L = cin + DSX_H;
    {
        const int kc = tid >> 7, l = (tid >> 5) & 3, o = tid & 31;          // 2 x 4 x 32 = one weight per thread
        ws[kc][l][o] = l < cin ? Wg[(size_t)((2 + kc) * L + l) * DSX_COLS + o] : 0.f;
    }
    for (int i = tid; i < C * C; i += DSX_THREADS) tc[i / C][i % C] = Tc1[i];

    stc_dtc::GatePiece piece[GK];
    const stc_dtc::GatePiece none = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
    auto request = [&](long long r) {                          // the step whose first row is r
#pragma unroll
        for (int k = 0; k < GK; ++k) {
            const int q = tid + DSX_THREADS * k;               // piece (row of the step, d, part)
            const long long row = r + q / (C * 8);
            const size_t at = ((size_t)row * C + (size_t)((q >> 3) % C)) * DSX_H + (size_t)(q & 3) * 4;
            piece[k] = row < r1 ? stc_dtc::gate_request(gp, at, (q & 7) >= 4) : none;
        }
    };
    const int l = tid & 3, c = (tid >> 2) % C, rs = tid / (4 * C);

    request(r0);
    for (long long r = r0; r < r1; r += RI) {
#pragma unroll
        for (int k = 0; k < GK; ++k) {
            const int q = tid + DSX_THREADS * k;
            *reinterpret_cast<v4f*>(&gs[q / (C * 8)][(q >> 3) % C][4 * (q & 7)]) = stc_dtc::gate_form(piece[k], (q & 7) >= 4);
        }
        if (r + RI < r1) request(r + RI);
        __syncthreads();                                       // (the first step: the tables as well)
        float Q = 0.f, P = 0.f;
#pragma unroll
        for (int o4 = 0; o4 < DSX_COLS / 4; ++o4) {
            const v4f g = *reinterpret_cast<const v4f*>(&gs[rs][c][4 * o4]);
            const v4f w0 = *reinterpret_cast<const v4f*>(&ws[0][l][4 * o4]), w1 = *reinterpret_cast<const v4f*>(&ws[1][l][4 * o4]);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                Q = fmaf(g[e], w0[e], Q);
                P = fmaf(g[e], w1[e], P);
            }
        }
        ps[rs][c][l] = P;
        __syncthreads();
        float s = Q;
#pragma unroll 8
        for (int d = 0; d < C; ++d) s = fmaf(tc[c][d], ps[rs][d][l], s);
        if (l < cin && r + rs < r1) dSx[((size_t)(r + rs) * C + c) * cin + l] = s;
        __syncthreads();                                       // gs and ps are rewritten by the next step
    }
}

}  // namespace

extern "C" int stc_cell_dsx_narrow_planar_f32(const float* H, const float* Wg, const float* Tc, const float* U, const float* R, const float* Cand,
                                              const float* dHnew, const float* dRH, float* dSx, int32_t cin, int64_t rows, int32_t C, void* stream) {
    const char* who = "stc_cell_dsx_narrow_planar_f32";
    STC_REQUIRE(C == 32 || C == 64, STC_EINVAL, "%s: C in (32, 64); got C=%d", who, C);
    STC_REQUIRE(cin >= 1 && cin <= 4, STC_EINVAL, "%s: a narrow input plane, cin = 1..4; got cin=%d", who, cin);
    STC_REQUIRE(rows >= 0 && rows < (1ll << 31), STC_EINVAL, "%s: rows=%lld outside [0, 2^31)", who, (long long)rows);
    if (rows == 0) return STC_OK;
    STC_REQUIRE(H && Wg && Tc && U && R && Cand && dHnew && dRH && dSx, STC_EINVAL, "%s: null operand", who);
    for (const float* q : {H, U, R, Cand, dHnew, dRH})
        STC_REQUIRE(stc::aligned16(q), STC_EALIGN, "%s: state-sized planes must be 16-byte aligned", who);
    STC_REQUIRE(stc::aligned(Wg, 4) && stc::aligned(Tc, 4) && stc::aligned(dSx, 4), STC_EALIGN, "%s: unaligned operand (Wg, Tc and dSx 4-byte)", who);
    const stc_dtc::GatePlanes gp{dHnew, Cand, U, dRH, R, H};
    const dim3 grid((unsigned)((rows + DSX_RUN - 1) / DSX_RUN)), block(DSX_THREADS);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (C == 32) hipLaunchKernelGGL(dsx_narrow_kernel<32>, grid, block, 0, s, gp, Wg, Tc + 32 * 32, dSx, (int)cin, (long long)rows);
    else hipLaunchKernelGGL(dsx_narrow_kernel<64>, grid, block, 0, s, gp, Wg, Tc + 64 * 64, dSx, (int)cin, (long long)rows);
    STC_LAUNCH_CHECK("stc_cell_dsx_narrow_planar_f32 launch");
    return STC_OK;
}
