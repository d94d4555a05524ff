// The gradient of a LEARNED spatial graph on a SPARSE pattern (graph_mode 'csr-learned' on the few-category cell kernels): the product of
// stc_graph_grad_f32 (stc_graph_grad.hip) sampled at the stored entries of a CSR pattern,
//     partials[chunk][e] = sum_{planes g of the chunk} sum_f A[g][i(e)][f] * B[g][colidx[e]][f]          e: the entries of row i(e)
// with the same operands -- planes (cells * batch, N, F) that the cell launches left: A = gradient of an aggregated slab, B = its source slab --
// the same cell selector and the same cut of the planes into chunks (g = chunk, chunk + n_chunks, ...).  The pattern is the CSR of Gs^T (row =
// destination node), so the result is in the order of the operand's forward values.  A dense (N, N) product is never formed: at 90 x 90 nodes it
// would be 525 MB of float64 per chunk, the pattern has 6 x 10^4 entries.
//
// One wave per (row, chunk), GC_WAVES consecutive rows per workgroup.  Lane l holds the 16-byte pieces l (and l + 64: F > 256) of the row of A;
// the row's entries are walked in tiles of GC_TILE: per plane and entry the lane forms ITS share of the dot product as an fp32 fmaf chain over
// its <= 8 floats (piece l first, element 0..3, then piece l + 64) and adds it to the entry's FLOAT64 accumulator, which runs over the planes of
// the chunk; after the last plane the 64 accumulators are added over the wave in float64 and one lane writes the entry.  No atomics, one fixed
// order: bitwise reproducible.  The neighbour rows of B come through L2: the workgroups of a chunk are dealt to the XCDs in bands of
// consecutive rows (stc_xcd_tile), so rows that share neighbours -- a lattice's rows one grid line apart -- sit in one L2.  A row of any length
// takes ceil(length / GC_TILE) passes over the chunk's planes (the hub row of N - 1 entries included); a row without entries does nothing.
#include "stc_common.h"

namespace {

using v4f = __attribute__((ext_vector_type(4))) float;
constexpr int GC_WAVES = 4, GC_THREADS = GC_WAVES * stc::kWave;
constexpr int GC_TILE = 8;                 // entries whose B rows are in flight together = float64 accumulators per lane
constexpr int GC_MAX_F = 512;              // two 16-byte pieces per lane

// the cell selector of stc_graph_grad.hip: g = sel * batch + sample -> plane (cell0 + sel * cell_step) * batch + sample
struct Sel {
    int cell0, cell_step, n_sel, batch;
};
__device__ __forceinline__ size_t plane_of(const Sel& s, int g) { return (size_t)(s.cell0 + (g / s.batch) * s.cell_step) * s.batch + g % s.batch; }

template <int PIECES>      // 16-byte pieces per lane: 1 (F <= 256) or 2
__global__ __launch_bounds__(GC_THREADS) void graph_grad_csr_kernel(const int* __restrict__ rowptr, const int* __restrict__ colidx, const float* __restrict__ A,
                                                                    const float* __restrict__ B, double* __restrict__ part, Sel sel, int n_rows, int F,
                                                                    long long chunk_stride) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int groups = (n_rows + GC_WAVES - 1) / GC_WAVES, group = stc_xcd_tile(blockIdx.x, groups);
    if (group < 0) return;
    const int row = group * GC_WAVES + wave;
    if (row >= n_rows) return;
    const int e0 = __builtin_amdgcn_readfirstlane(rowptr[row]), e1 = __builtin_amdgcn_readfirstlane(rowptr[row + 1]);
    if (e0 >= e1) return;
    const int P4 = F >> 2, G = sel.n_sel * sel.batch, chunk = blockIdx.y, chunks = gridDim.y;
    bool has[PIECES];
    int at[PIECES];                                                   // the lane's pieces, as float offsets inside a row (a piece past F: none, reads nothing)
#pragma unroll
    for (int p = 0; p < PIECES; ++p) {
        has[p] = lane + 64 * p < P4;
        at[p] = has[p] ? 4 * (lane + 64 * p) : 0;
    }
    double* out = part + (size_t)chunk * chunk_stride;
    const size_t plane_floats = (size_t)n_rows * F;
    for (int t0 = e0; t0 < e1; t0 += GC_TILE) {
        size_t col[GC_TILE];                                          // (wave-uniform; a slot past the row repeats its last entry and is not stored)
#pragma unroll
        for (int t = 0; t < GC_TILE; ++t) col[t] = (size_t)__builtin_amdgcn_readfirstlane(colidx[min(t0 + t, e1 - 1)]) * F;
        double acc[GC_TILE];
#pragma unroll
        for (int t = 0; t < GC_TILE; ++t) acc[t] = 0.0;
        for (int g = chunk; g < G; g += chunks) {
            const size_t plane = plane_of(sel, g) * plane_floats;
            const float* a_row = A + plane + (size_t)row * F;
            const float* b_plane = B + plane;
            v4f a[PIECES], b[GC_TILE][PIECES];
            const v4f zero = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int p = 0; p < PIECES; ++p) a[p] = has[p] ? *reinterpret_cast<const v4f*>(a_row + at[p]) : zero;
#pragma unroll
            for (int t = 0; t < GC_TILE; ++t)                         // every neighbour row of the tile requested before the first product
#pragma unroll
                for (int p = 0; p < PIECES; ++p) b[t][p] = has[p] ? *reinterpret_cast<const v4f*>(b_plane + col[t] + at[p]) : zero;
#pragma unroll
            for (int t = 0; t < GC_TILE; ++t) {
                float s = 0.f;
#pragma unroll
                for (int p = 0; p < PIECES; ++p)
#pragma unroll
                    for (int c = 0; c < 4; ++c) s = fmaf(a[p][c], b[t][p][c], s);
                acc[t] += (double)s;
            }
        }
#pragma unroll
        for (int t = 0; t < GC_TILE; ++t) {
            const double s = stc_wave_sum(acc[t]);
            if (lane == t && t0 + t < e1) out[t0 + t] = s;            // (a chunk without a plane writes its zeros)
        }
    }
}

int check_sel(const char* what, int32_t cell0, int32_t cell_step, int32_t n_sel, int32_t batch, int32_t n_chunks) {
    STC_REQUIRE(cell0 >= 0 && cell_step >= 1 && n_sel >= 0 && batch >= 1 && n_chunks >= 1 && n_chunks <= 65535, STC_EINVAL,
                "%s: cell0=%d cell_step=%d n_sel=%d batch=%d n_chunks=%d", what, cell0, cell_step, n_sel, batch, n_chunks);
    return STC_OK;
}

}  // namespace

extern "C" int stc_graph_grad_csr_f32(const int32_t* rowptr, const int32_t* colidx, int32_t n_rows, int32_t nnz, const float* A, const float* B, double* partials,
                                      int32_t n_chunks, int32_t cell0, int32_t cell_step, int32_t n_sel, int32_t batch, int32_t F, int64_t chunk_stride,
                                      void* stream) {
    const char* who = "stc_graph_grad_csr_f32";
    STC_REQUIRE(n_rows >= 0 && nnz >= 0 && F >= 0, STC_EINVAL, "%s: negative size (n_rows=%d nnz=%d F=%d)", who, n_rows, nnz, F);
    if (int rc = check_sel(who, cell0, cell_step, n_sel, batch, n_chunks)) return rc;
    STC_REQUIRE(F >= 4 && F % 4 == 0 && F <= GC_MAX_F, STC_EINVAL, "%s: F=%d must be a multiple of 4 in [4, %d] (16-byte pieces, two per lane)", who, F, GC_MAX_F);
    STC_REQUIRE(chunk_stride == 0 || chunk_stride >= (int64_t)nnz, STC_EINVAL, "%s: chunk stride %lld below the block of %d entries", who, (long long)chunk_stride, nnz);
    if (nnz == 0 || n_sel == 0 || n_rows == 0) return STC_OK;
    STC_REQUIRE(rowptr && colidx && A && B && partials, STC_EINVAL, "%s: null operand", who);
    STC_REQUIRE(stc::aligned16(A) && stc::aligned16(B) && stc::aligned(partials, 8) && stc::aligned(rowptr, 4) && stc::aligned(colidx, 4), STC_EALIGN,
                "%s: unaligned operand (A and B 16-byte, partials 8-byte, rowptr and colidx 4-byte)", who);
    const int groups = (n_rows + GC_WAVES - 1) / GC_WAVES, padded = (groups + stc::kNumXcd - 1) / stc::kNumXcd * stc::kNumXcd;
    const dim3 grid((unsigned)padded, (unsigned)n_chunks);
    const long long stride = chunk_stride ? chunk_stride : (long long)nnz;
    const Sel sel{cell0, cell_step, n_sel, batch};
    if (F <= 256)
        hipLaunchKernelGGL(graph_grad_csr_kernel<1>, grid, dim3(GC_THREADS), 0, static_cast<hipStream_t>(stream), rowptr, colidx, A, B, partials, sel, (int)n_rows, (int)F, stride);
    else
        hipLaunchKernelGGL(graph_grad_csr_kernel<2>, grid, dim3(GC_THREADS), 0, static_cast<hipStream_t>(stream), rowptr, colidx, A, B, partials, sel, (int)n_rows, (int)F, stride);
    STC_LAUNCH_CHECK("stc_graph_grad_csr_f32 launch");
    return STC_OK;
}
