// The value gradient of a LEARNED spatial graph on a SPARSE pattern from the PLANAR cells of the cell-graph executor (graph_mode 'csr-learned'
// with csr_cells = 'fused' at C in {32, 64}; ABI v44): the sampled product of stc_graph_grad_csr.hip over up to three PAIRS of planes of one cell,
//     acc[e] += sum_{p < n_pairs} sum_{b < batch} sum_{f < F_p} A_p[b][i(e)][f] * B_p[b][colidx[e]][f]          e: the entries of row i(e)
// A planar cell applies S three times -- S.X, S.H and the candidate's A + S.Bm -- so one launch per cell takes the pairs (dSX, X), (dSH, H),
// (dY, Bm), each of its own width F_p (a narrow input plane: C * cin floats per node; a state plane: C * 16, up to 1024).  The pattern is the CSR
// of Gs^T (row = destination node): the result is in the order of the operand's forward values.  acc (nnz float64) is ADDED TO: the caller zeroes
// it once per backward pass and every cell's launch adds.
//
// One wave per row, GP_WAVES consecutive rows per workgroup, the workgroups dealt to the XCDs in bands of consecutive rows (stc_xcd_tile) so
// that rows which share neighbours sit in one L2.  Lane l holds the 16-byte pieces l, l + 64, .. of a row (1, 2 or 4 per lane: F <= 256, 512,
// 1024).  The row's entries are walked in tiles of TILE (8; 4 where some pair has four pieces per lane -- the neighbour rows of a whole tile are
// requested before the first product, and with four pieces eight of them do not fit the register file): per pair, sample and entry the lane
// forms ITS share of the dot product as an fp32 fmaf chain (piece l first, elements 0..3, then piece l + 64, ..) and adds it to the entry's
// FLOAT64 accumulator, which runs over the samples and the pairs in order; then the 64 accumulators are added over the wave in float64 and one
// lane adds the sum to acc[e].  Every entry belongs to exactly one wave: no atomics, one fixed order -- bitwise reproducible.  A row of any
// length takes ceil(length / TILE) passes; a row without entries does nothing.
#include "stc_common.h"

namespace {

using v4f = __attribute__((ext_vector_type(4))) float;
constexpr int GP_WAVES = 4, GP_THREADS = GP_WAVES * stc::kWave;
constexpr int GP_MAX_PAIRS = 3;
constexpr int GP_MAX_F = 1024;             // four 16-byte pieces per lane

struct Pairs {
    const float* a[GP_MAX_PAIRS];
    const float* b[GP_MAX_PAIRS];
    int F[GP_MAX_PAIRS];
    int n;
};

// one pair's share of a tile: acc[t] += sum over the samples of the lane's part of < A[b][row], B[b][col[t]] >
template <int PIECES, int TILE>
__device__ __forceinline__ void pair_share(const float* __restrict__ A, const float* __restrict__ B, int F, int row, const int (&col)[TILE], int n_rows, int batch,
                                           int lane, double (&acc)[TILE]) {
    bool has[PIECES];
    int at[PIECES];                                                   // the lane's pieces, as float offsets inside a row (a piece past F: none, reads nothing)
#pragma unroll
    for (int p = 0; p < PIECES; ++p) {
        has[p] = lane + 64 * p < (F >> 2);
        at[p] = has[p] ? 4 * (lane + 64 * p) : 0;
    }
    const size_t plane_floats = (size_t)n_rows * F;
    const v4f zero = {0.f, 0.f, 0.f, 0.f};
    for (int s = 0; s < batch; ++s) {
        const float* a_row = A + (size_t)s * plane_floats + (size_t)row * F;
        const float* b_plane = B + (size_t)s * plane_floats;
        v4f a[PIECES], b[TILE][PIECES];
#pragma unroll
        for (int p = 0; p < PIECES; ++p) a[p] = has[p] ? *reinterpret_cast<const v4f*>(a_row + at[p]) : zero;
#pragma unroll
        for (int t = 0; t < TILE; ++t)                                // every neighbour row of the tile requested before the first product
#pragma unroll
            for (int p = 0; p < PIECES; ++p) b[t][p] = has[p] ? *reinterpret_cast<const v4f*>(b_plane + (size_t)col[t] * F + at[p]) : zero;
#pragma unroll
        for (int t = 0; t < TILE; ++t) {
            float sh = 0.f;
#pragma unroll
            for (int p = 0; p < PIECES; ++p)
#pragma unroll
                for (int c = 0; c < 4; ++c) sh = fmaf(a[p][c], b[t][p][c], sh);
            acc[t] += (double)sh;
        }
    }
}

template <int MAXP>        // the most 16-byte pieces per lane any pair of the launch has: 1, 2 or 4
__global__ __launch_bounds__(GP_THREADS) void graph_grad_csr_pairs_kernel(const int* __restrict__ rowptr, const int* __restrict__ colidx, Pairs pr,
                                                                          double* __restrict__ out, int n_rows, int batch) {
    constexpr int TILE = MAXP == 4 ? 4 : 8;                           // entries whose B rows are in flight together = float64 accumulators per lane
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int groups = (n_rows + GP_WAVES - 1) / GP_WAVES, group = stc_xcd_tile(blockIdx.x, groups);
    if (group < 0) return;
    const int row = group * GP_WAVES + wave;
    if (row >= n_rows) return;
    const int e0 = __builtin_amdgcn_readfirstlane(rowptr[row]), e1 = __builtin_amdgcn_readfirstlane(rowptr[row + 1]);
    if (e0 >= e1) return;
    for (int t0 = e0; t0 < e1; t0 += TILE) {
        int col[TILE];                                                // (wave-uniform; a slot past the row repeats its last entry and is not stored)
#pragma unroll
        for (int t = 0; t < TILE; ++t) col[t] = __builtin_amdgcn_readfirstlane(colidx[min(t0 + t, e1 - 1)]);
        double acc[TILE];
#pragma unroll
        for (int t = 0; t < TILE; ++t) acc[t] = 0.0;
#pragma unroll                                                        // (unrolled: the pair table stays in kernel-argument registers)
        for (int p = 0; p < GP_MAX_PAIRS; ++p) {
            if (p >= pr.n) break;
            const int F = pr.F[p];                                    // (wave-uniform: each pair runs at its own piece count)
            if (MAXP >= 4 && F > 512) pair_share<4, TILE>(pr.a[p], pr.b[p], F, row, col, n_rows, batch, lane, acc);
            else if (MAXP >= 2 && F > 256) pair_share<2, TILE>(pr.a[p], pr.b[p], F, row, col, n_rows, batch, lane, acc);
            else pair_share<1, TILE>(pr.a[p], pr.b[p], F, row, col, n_rows, batch, lane, acc);
        }
#pragma unroll
        for (int t = 0; t < TILE; ++t) {
            const double s = stc_wave_sum(acc[t]);
            if (lane == t && t0 + t < e1) out[t0 + t] += s;           // the entry's one owner: a plain read-modify-write
        }
    }
}

}  // namespace

extern "C" int stc_graph_grad_csr_pairs_f32(const int32_t* rowptr, const int32_t* colidx, int32_t n_rows, int32_t nnz, const float* const* A,
                                            const float* const* B, const int32_t* F, int32_t n_pairs, int32_t batch, double* acc, void* stream) {
    const char* who = "stc_graph_grad_csr_pairs_f32";
    STC_REQUIRE(n_rows >= 0 && nnz >= 0 && batch >= 0, STC_EINVAL, "%s: negative size (n_rows=%d nnz=%d batch=%d)", who, n_rows, nnz, batch);
    STC_REQUIRE(n_pairs >= 1 && n_pairs <= GP_MAX_PAIRS, STC_EINVAL, "%s: n_pairs=%d outside [1, %d]", who, n_pairs, GP_MAX_PAIRS);
    STC_REQUIRE(A && B && F, STC_EINVAL, "%s: null operand (the host arrays A, B, F)", who);
    int max_f = 0;
    for (int p = 0; p < n_pairs; ++p) {
        STC_REQUIRE(F[p] >= 4 && F[p] % 4 == 0 && F[p] <= GP_MAX_F, STC_EINVAL, "%s: F[%d]=%d must be a multiple of 4 in [4, %d] (16-byte pieces, four per lane)",
                    who, p, F[p], GP_MAX_F);
        max_f = F[p] > max_f ? F[p] : max_f;
    }
    if (nnz == 0 || batch == 0 || n_rows == 0) return STC_OK;
    STC_REQUIRE(rowptr && colidx && acc, STC_EINVAL, "%s: null operand", who);
    Pairs pr{};
    pr.n = n_pairs;
    for (int p = 0; p < n_pairs; ++p) {
        STC_REQUIRE(A[p] && B[p], STC_EINVAL, "%s: null operand (plane of pair %d)", who, p);
        STC_REQUIRE(stc::aligned16(A[p]) && stc::aligned16(B[p]), STC_EALIGN, "%s: unaligned operand (planes of pair %d: 16-byte)", who, p);
        pr.a[p] = A[p], pr.b[p] = B[p], pr.F[p] = F[p];
    }
    STC_REQUIRE(stc::aligned(acc, 8) && stc::aligned(rowptr, 4) && stc::aligned(colidx, 4), STC_EALIGN,
                "%s: unaligned operand (acc 8-byte, rowptr and colidx 4-byte)", who);
    const int groups = (n_rows + GP_WAVES - 1) / GP_WAVES, padded = (groups + stc::kNumXcd - 1) / stc::kNumXcd * stc::kNumXcd;
    const dim3 grid((unsigned)padded), block(GP_THREADS);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (max_f <= 256) hipLaunchKernelGGL(graph_grad_csr_pairs_kernel<1>, grid, block, 0, s, rowptr, colidx, pr, acc, (int)n_rows, (int)batch);
    else if (max_f <= 512) hipLaunchKernelGGL(graph_grad_csr_pairs_kernel<2>, grid, block, 0, s, rowptr, colidx, pr, acc, (int)n_rows, (int)batch);
    else hipLaunchKernelGGL(graph_grad_csr_pairs_kernel<4>, grid, block, 0, s, rowptr, colidx, pr, acc, (int)n_rows, (int)batch);
    STC_LAUNCH_CHECK("stc_graph_grad_csr_pairs_f32 launch");
    return STC_OK;
}
