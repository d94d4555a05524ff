// Internal: the CSR (one wave per row) and row-blocked (BCSR 4x1) gather kernels of the spatial aggregation and their launch ladder, written
// once for fp32 rows (stc_spmm.hip) and bf16 rows (stc_spmm_bf16.hip).
//
// Layout of one launch (both kernels):
//   workgroup  = a run of consecutive output rows of one batch element
//   CSR stage  = row-pointer slice + the (col,val) segment of those rows -> LDS, one coalesced pass
//   wave       = one output row (CSR) or one block of 4 rows (BCSR) at a time; (col,val) read from LDS are
//                wave-uniform and moved to SGPRs (readfirstlane) so the neighbour-row base address is scalar
//   lane       = VPT 16-byte pieces of the row (stc_spmm_piece.h), 4 neighbour rows in flight (16 loads per lane)
//   blocks     = remapped so each XCD walks a contiguous band of rows: the rows a band gathers (its own +-
//                the graph bandwidth) stay in that XCD's 4 MiB L2
//   output     = the format's epilogue on the fp32 sums of each piece
//
// A format is a small struct Fmt.  What the two formats share is here; where they differ, the kernels call a member of Fmt by name:
//   Fmt::Acc                          the fp32 sums of a piece: zero(), fma(s, raw piece), elements v[i]
//   Fmt::Epi                          the epilogue's kernel argument (Y, Y0, X2 and whatever its modes read and write)
//   Fmt::Operand<TWO>, gather<TWO>,   what a lane holds of one neighbour row and how it enters the sums: with the second gathered operand of
//   accumulate                        EP_SUM2, fp32 rows add the X2 piece to the X piece and do one fma, bf16 rows do two fmas (either order of
//                                     roundings is pinned by its CPU twin, oracle/kernel_emul.py)
//   Fmt::BLEND_AHEAD_WAVE_ROW         whether the wave-per-row kernel requests the blend's A, U, H pieces before the gather (the row-block
//                                     kernel always does) or loads them in the epilogue
//   Fmt::blend_operands,              the epilogues: EP_BLEND on a piece (ROW_BLOCK: called by the row-block kernel), every other mode on a
//   blend<ROW_BLOCK>,                 piece, and what a wave does after its last
//   finish<MODE>, wave_done<MODE>     piece (fp32 rows: publishes the launch's max |Y|)
//   Fmt::MAX_VPT, ONE_WAVE_BLOCKS,    the arms of the launch ladder that are instantiated for the format
//   PIPELINED
#pragma once
#include "stc_spmm_host.h"
#include "stc_spmm_piece.h"

namespace {

using stc::GraphArgs;

constexpr int SPMM_THREADS = 256;
constexpr int SPMM_WAVES = SPMM_THREADS / 64;
constexpr int SPMM_ROWS = 8;         // CSR kernel: output rows per workgroup
constexpr int SPMM_SEG_CAP = 1024;   // CSR entries staged in LDS per workgroup

// one numbering of the epilogue modes for both formats (EP_PLAIN stays 0: profiles name the plain launch by it)
enum { EP_PLAIN = 0, EP_BLEND = 1, EP_SUM = 2, EP_SUM2 = 3 };

__device__ __forceinline__ float uniform_f(float v) {
    return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(v)));
}
__device__ __forceinline__ float tanh_fast(float v) { return stc_tanh(v); }      // hardware exp2 / rcp, polynomial below 1/4 (stc_common.h)

// EP_BLEND: the epilogue's own operands (A, U, H pieces of an output piece)
struct BlendIn { Raw a, u, h; };

// piece `at` of the gathered operand (of both in EP_SUM2: X2 is null otherwise); zeros for a piece past the row's end
template <class Fmt, int MODE>
__device__ __forceinline__ typename Fmt::template Operand<MODE == EP_SUM2> fetch(const Raw* X, const Raw* X2, size_t at, bool inside) {
    using Op = typename Fmt::template Operand<MODE == EP_SUM2>;
    Op x{};
    if (inside) x = Fmt::template gather<MODE == EP_SUM2>(X, X2, at);
    return x;
}

// ---- CSR: one wave per output row (learned dense graphs, graphs without a row-block plan) ------------------------
// FP: 16-byte pieces per row
template <int VPT, int MODE, class Fmt>
__global__ __launch_bounds__(SPMM_THREADS) void spmm_wave_row_kernel(
    const int* __restrict__ rowptr, const int* __restrict__ colidx, const float* __restrict__ val,
    int n_rows, int n_cols, const Raw* __restrict__ X, int FP, int n_tiles, typename Fmt::Epi ep) {
    using Acc = typename Fmt::Acc;
    using Op = typename Fmt::template Operand<MODE == EP_SUM2>;
    __shared__ int s_rp[SPMM_ROWS + 1];
    __shared__ int s_col[SPMM_SEG_CAP];
    __shared__ float s_val[SPMM_SEG_CAP];

    const int tile = stc_xcd_tile(blockIdx.x, n_tiles);
    if (tile < 0) return;                       // whole workgroup leaves together
    float wmax = 0.f;                           // for Fmt::wave_done
    const int b = blockIdx.y;
    const int row0 = tile * SPMM_ROWS;
    const int nr = min(SPMM_ROWS, n_rows - row0);

    if ((int)threadIdx.x <= nr) s_rp[threadIdx.x] = rowptr[row0 + threadIdx.x];
    __syncthreads();
    const int seg0 = s_rp[0];
    const int seg_n = min(s_rp[nr] - seg0, SPMM_SEG_CAP);
    for (int t = threadIdx.x; t < seg_n; t += SPMM_THREADS) {
        s_col[t] = colidx[seg0 + t];
        s_val[t] = val[seg0 + t];
    }
    __syncthreads();

    const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    const Raw* Xb = X + (size_t)b * n_cols * FP;
    const Raw* X2b = MODE == EP_SUM2 ? ep.X2 + (size_t)b * n_cols * FP : nullptr;

    for (int r = wave; r < nr; r += SPMM_WAVES) {
        const int js = s_rp[r] - seg0;
        const int je = s_rp[r + 1] - seg0;
        const size_t rowg = (size_t)b * n_rows + row0 + r;
        for (int cb = 0; cb < FP; cb += 64 * VPT) {
            Acc acc[VPT];
#pragma unroll
            for (int p = 0; p < VPT; ++p) acc[p].zero();
            constexpr bool AHEAD = MODE == EP_BLEND && Fmt::BLEND_AHEAD_WAVE_ROW;      // requested here, they arrive under the gather
            BlendIn bin[AHEAD ? VPT : 1];
            if (AHEAD) {
#pragma unroll
                for (int p = 0; p < VPT; ++p) {
                    const int ch = cb + lane + 64 * p;
                    if (ch < FP) bin[AHEAD ? p : 0] = Fmt::blend_operands(ep, rowg * FP + ch);
                }
            }

            auto entry = [&](int j, int& c, float& v) {
                if (j < SPMM_SEG_CAP) {
                    c = s_col[j];
                    v = s_val[j];
                } else {                       // rows longer than the staged segment (dense graphs)
                    c = colidx[seg0 + j];
                    v = val[seg0 + j];
                }
                c = __builtin_amdgcn_readfirstlane(c);
                v = uniform_f(v);
            };

            int j = js;
            for (; j + 4 <= je; j += 4) {
                int c[4];
                float v[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) entry(j + u, c[u], v[u]);
                Op x[4][VPT];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
#pragma unroll
                    for (int p = 0; p < VPT; ++p) {
                        const int ch = cb + lane + 64 * p;
                        x[u][p] = fetch<Fmt, MODE>(Xb, X2b, (size_t)c[u] * FP + ch, ch < FP);
                    }
                }
#pragma unroll
                for (int u = 0; u < 4; ++u)
#pragma unroll
                    for (int p = 0; p < VPT; ++p) Fmt::accumulate(acc[p], v[u], x[u][p]);
            }
            for (; j < je; ++j) {
                int c;
                float v;
                entry(j, c, v);
#pragma unroll
                for (int p = 0; p < VPT; ++p) {
                    const int ch = cb + lane + 64 * p;
                    if (ch < FP) Fmt::accumulate(acc[p], v, fetch<Fmt, MODE>(Xb, X2b, (size_t)c * FP + ch, true));
                }
            }
#pragma unroll
            for (int p = 0; p < VPT; ++p) {
                const int ch = cb + lane + 64 * p;
                if (ch < FP) {
                    if (MODE == EP_BLEND) Fmt::template blend<false>(ep, rowg, FP, ch, acc[p], AHEAD ? bin[AHEAD ? p : 0] : Fmt::blend_operands(ep, rowg * FP + ch));
                    else Fmt::template finish<MODE>(ep, rowg, FP, ch, acc[p], wmax);
                }
            }
        }
    }
    Fmt::template wave_done<MODE>(ep, wmax);
}

// ---- row-blocked (BCSR 4x1): one wave produces 4 consecutive output rows -----------------------------------------
// Same skeleton, but every fetched neighbour row is accumulated into the 4 rows of the block with its 4
// wave-uniform values: a row shared by several rows of the block is fetched once (18 instead of 36 fetches per 4
// rows of the 8-neighbour grid; the CSR kernel is bound by exactly that L2 -> CU gather traffic).  (An LDS-staged
// tile variant -- distinct rows of 8 output rows copied to LDS per 1 KiB column block -- measured 234 us vs 128 us
// for the CSR kernel: three dependent memory latencies per workgroup, too few bytes in flight; dropped.)
// BC_BLOCKS row blocks per workgroup: 4 (one per wave) or 2 (two waves share a block and split its column blocks
// of 64*VPT pieces).  Fewer rows per workgroup keep the set of rows all resident workgroups of an XCD are gathering
// (their "window") small enough for that XCD's 4 MiB L2: at 32 rows per workgroup the window is ~12 MB and
// FETCH_SIZE shows every X row fetched 1.8 times from beyond L2.
constexpr int BR = STC_SPMM_BLOCK_ROWS;
constexpr int BC_CAP = 512;           // block entries staged in LDS per workgroup

// PIPE = 1: the gather is software-pipelined -- batches of PU = 6 neighbour rows (the 8-neighbour grid's interior blocks list
// 18 rows: three full batches, no remainder; graph.py pads every block's list to a multiple of 6 with zero-weight repeats
// of its last column), the NEXT batch's row loads issued before the current batch is accumulated, so that a wave always
// has 6 KiB in flight instead of alternating between "4 loads outstanding" and "none while it multiplies"; the old form
// also walked a remainder (18 = 4 x 4 + 2) one exposed round trip per row.
constexpr int PU = 6;

template <int VPT, int MODE, int BC_BLOCKS, int PIPE, int FULL, class Fmt>      // FULL: FP is a multiple of the columns the waves of a row block cover
__global__ __launch_bounds__(SPMM_THREADS) void spmm_bcsr_kernel(
    const int* __restrict__ blk_ptr, const int* __restrict__ blk_cols, const float* __restrict__ blk_vals,
    int n_rows, int n_cols, const Raw* __restrict__ X, int FP, int n_blocks, int n_tiles, typename Fmt::Epi ep) {
    static_assert(BR == 4, "the pipelined gather reads one float4 of values per entry");
    static_assert(SPMM_WAVES % BC_BLOCKS == 0, "whole waves per row block");
    using Acc = typename Fmt::Acc;
    using Op = typename Fmt::template Operand<MODE == EP_SUM2>;
    __shared__ int s_bp[BC_BLOCKS + 1];
    __shared__ __attribute__((aligned(16))) int s_col[BC_CAP];
    __shared__ __attribute__((aligned(16))) float s_val[BC_CAP * BR];

    const int tile = stc_xcd_tile(blockIdx.x, n_tiles);
    if (tile < 0) return;
    float wmax = 0.f;                           // for Fmt::wave_done
    const int b = blockIdx.y;
    const int blk0 = tile * BC_BLOCKS;
    const int nb = min(BC_BLOCKS, n_blocks - blk0);
    if ((int)threadIdx.x <= nb) s_bp[threadIdx.x] = blk_ptr[blk0 + threadIdx.x];
    __syncthreads();
    const int seg0 = s_bp[0];
    const int seg_n = min(s_bp[nb] - seg0, BC_CAP);
    for (int t = threadIdx.x; t < seg_n; t += SPMM_THREADS) s_col[t] = blk_cols[seg0 + t];
    for (int t = threadIdx.x; t < seg_n * BR; t += SPMM_THREADS) s_val[t] = blk_vals[(size_t)seg0 * BR + t];
    __syncthreads();

    constexpr int WPB = SPMM_WAVES / BC_BLOCKS;      // waves sharing one row block
    const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    const Raw* Xb = X + (size_t)b * n_cols * FP;
    const Raw* X2b = MODE == EP_SUM2 ? ep.X2 + (size_t)b * n_cols * FP : nullptr;

    for (int bi = wave / WPB; bi < nb; bi += SPMM_WAVES / WPB) {
        const int js = s_bp[bi] - seg0, je = s_bp[bi + 1] - seg0;
        const int row_base = (blk0 + bi) * BR;
        const int rows_here = min(BR, n_rows - row_base);
        for (int cb = (wave % WPB) * 64 * VPT; cb < FP; cb += WPB * 64 * VPT) {
            Acc acc[BR][VPT];
#pragma unroll
            for (int r = 0; r < BR; ++r)
#pragma unroll
                for (int p = 0; p < VPT; ++p) acc[r][p].zero();
            // EP_BLEND: the epilogue's own operands (A, U, H pieces of the block's rows) are requested BEFORE the gather so
            // that they arrive under it instead of as a second exposed round trip at the end
            constexpr int PR = MODE == EP_BLEND ? BR : 1;
            BlendIn bin[PR][VPT];
            if (MODE == EP_BLEND) {
#pragma unroll
                for (int r = 0; r < PR; ++r)
#pragma unroll
                    for (int p = 0; p < VPT; ++p) {
                        const int ch = cb + lane + 64 * p;
                        if (r < rows_here && ch < FP) bin[r][p] = Fmt::blend_operands(ep, ((size_t)b * n_rows + row_base + r) * FP + ch);
                    }
            }

            auto entry = [&](int j, int& c, float (&v)[BR]) {
                if (j < BC_CAP) {
                    c = s_col[j];
#pragma unroll
                    for (int r = 0; r < BR; ++r) v[r] = s_val[j * BR + r];
                } else {                       // block lists longer than the staged segment
                    c = blk_cols[seg0 + j];
#pragma unroll
                    for (int r = 0; r < BR; ++r) v[r] = blk_vals[(size_t)(seg0 + j) * BR + r];
                }
                c = __builtin_amdgcn_readfirstlane(c);
#pragma unroll
                for (int r = 0; r < BR; ++r) v[r] = uniform_f(v[r]);
            };

            int j = js;
            if constexpr (PIPE) {
                // rows of one batch: PU neighbour rows, this lane's VPT pieces of each (second gathered operand included).
                // The six column indices come out of LDS in three 8-byte reads issued together (one wait, not six).
                constexpr bool full_cols = FULL != 0;                     // every lane's pieces exist: no per-load column guard
                auto issue = [&](int j0, Op (&x)[PU][VPT]) {
                    const int2* cp = reinterpret_cast<const int2*>(s_col + j0);
                    const int2 c01 = cp[0], c23 = cp[1], c45 = cp[2];
                    const int cc[PU] = {c01.x, c01.y, c23.x, c23.y, c45.x, c45.y};
#pragma unroll
                    for (int u = 0; u < PU; ++u) {
                        const int c = __builtin_amdgcn_readfirstlane(cc[u]);
#pragma unroll
                        for (int p = 0; p < VPT; ++p) {
                            const int ch = cb + lane + 64 * p;
                            x[u][p] = fetch<Fmt, MODE>(Xb, X2b, (size_t)c * FP + ch, full_cols || ch < FP);
                        }
                    }
                };
                auto consume = [&](int j0, const Op (&x)[PU][VPT]) {
                    const float4* vp = reinterpret_cast<const float4*>(s_val + (size_t)j0 * BR);      // BR = 4 values per entry: one 16-byte read each
                    float4 vv[PU];
#pragma unroll
                    for (int u = 0; u < PU; ++u) vv[u] = vp[u];
#pragma unroll
                    for (int u = 0; u < PU; ++u) {
                        const float v[BR] = {vv[u].x, vv[u].y, vv[u].z, vv[u].w};
#pragma unroll
                        for (int r = 0; r < BR; ++r)
#pragma unroll
                            for (int p = 0; p < VPT; ++p) Fmt::accumulate(acc[r][p], v[r], x[u][p]);
                    }
                };
                // (a workgroup whose lists outgrow the staged segment -- not a sparse graph any more -- or whose list starts at an
                // odd entry -- an unpadded plan: the 8-byte LDS reads want an even index -- takes the remainder loop)
                const int jfull = (je <= BC_CAP && (js & 1) == 0) ? js + (je - js) / PU * PU : js;
                if (j < jfull) {
                    Op xa[PU][VPT], xb[PU][VPT];
                    issue(j, xa);
                    while (true) {
                        if (j + PU < jfull) issue(j + PU, xb);
                        consume(j, xa);
                        j += PU;
                        if (j >= jfull) break;
                        if (j + PU < jfull) issue(j + PU, xa);
                        consume(j, xb);
                        j += PU;
                        if (j >= jfull) break;
                    }
                }
            } else
            for (; j + 4 <= je; j += 4) {
                int c[4];
                float v[4][BR];
#pragma unroll
                for (int u = 0; u < 4; ++u) entry(j + u, c[u], v[u]);
                Op x[4][VPT];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
#pragma unroll
                    for (int p = 0; p < VPT; ++p) {
                        const int ch = cb + lane + 64 * p;
                        x[u][p] = fetch<Fmt, MODE>(Xb, X2b, (size_t)c[u] * FP + ch, ch < FP);
                    }
                }
#pragma unroll
                for (int u = 0; u < 4; ++u)
#pragma unroll
                    for (int r = 0; r < BR; ++r)
#pragma unroll
                        for (int p = 0; p < VPT; ++p) Fmt::accumulate(acc[r][p], v[u][r], x[u][p]);
            }
            for (; j < je; ++j) {                 // remainder (PIPE: lists that are not a multiple of PU, i.e. unpadded plans)
                int c;
                float v[BR];
                entry(j, c, v);
#pragma unroll
                for (int p = 0; p < VPT; ++p) {
                    const int ch = cb + lane + 64 * p;
                    if (ch < FP) {
                        const Op xv = fetch<Fmt, MODE>(Xb, X2b, (size_t)c * FP + ch, true);
#pragma unroll
                        for (int r = 0; r < BR; ++r) Fmt::accumulate(acc[r][p], v[r], xv);
                    }
                }
            }
#pragma unroll
            for (int r = 0; r < BR; ++r) {
                if (r < rows_here) {
                    const size_t rowg = (size_t)b * n_rows + row_base + r;
#pragma unroll
                    for (int p = 0; p < VPT; ++p) {
                        const int ch = cb + lane + 64 * p;
                        if (ch < FP) {
                            if (MODE == EP_BLEND) Fmt::template blend<true>(ep, rowg, FP, ch, acc[r][p], bin[MODE == EP_BLEND ? r : 0][p]);
                            else Fmt::template finish<MODE>(ep, rowg, FP, ch, acc[r][p], wmax);
                        }
                    }
                }
            }
        }
    }
    Fmt::template wave_done<MODE>(ep, wmax);
}

// ---- the launch ladder of both graph forms.  FP: 16-byte pieces per row.  A format without an arm (Fmt::MAX_VPT, ONE_WAVE_BLOCKS, PIPELINED)
// names the neighbouring arm's instantiation there: no kernel is built that no launch selects.
template <int VPT, int MODE, int BLOCKS, class Fmt>      // BLOCKS row blocks per workgroup
void launch_row_blocks(const GraphArgs& g, int n_rows, int n_cols, const Raw* X, int batch, int FP, const typename Fmt::Epi& ep, hipStream_t s) {
    const int n_blocks = (n_rows + BR - 1) / BR;
    const int n_tiles = (n_blocks + BLOCKS - 1) / BLOCKS;
    const int per = (n_tiles + stc::kNumXcd - 1) / stc::kNumXcd;
    const dim3 grid(per * stc::kNumXcd, batch), block(SPMM_THREADS);
    // The pipelined gather is used where it measured faster on MI355X (profiles/r02/c_kbench_spmm.txt, fp32 rows): the plain product
    // Y = alpha S.X with full column blocks (F=1024, B=1: 99 -> 86 us; F=512, B=5: 218 -> 210 us).  With a Y0 operand or an
    // epilogue (sum / blend forms) the extra live registers cost what the pipelining gains (equal or slower): old loop.
    // (measured again for the state-gradient sum with ONE gathered operand, which is what the cell graph launches now: 27.1 vs 27.3 ms)
    constexpr int PIPE = Fmt::PIPELINED && MODE == EP_PLAIN;
    if (PIPE && (ep.Y0 == nullptr || ep.beta == 0.f) && FP % (128 * VPT) == 0)
        hipLaunchKernelGGL((spmm_bcsr_kernel<VPT, MODE, BLOCKS, PIPE, PIPE, Fmt>), grid, block, 0, s, g.blk_ptr, g.blk_cols, g.blk_vals, n_rows, n_cols, X, FP, n_blocks, n_tiles, ep);
    else
        hipLaunchKernelGGL((spmm_bcsr_kernel<VPT, MODE, BLOCKS, 0, 0, Fmt>), grid, block, 0, s, g.blk_ptr, g.blk_cols, g.blk_vals, n_rows, n_cols, X, FP, n_blocks, n_tiles, ep);
}

template <int VPT, int MODE, class Fmt>
void launch_wave_rows(const GraphArgs& g, int n_rows, int n_cols, const Raw* X, int batch, int FP, const typename Fmt::Epi& ep, hipStream_t s) {
    const int n_tiles = (n_rows + SPMM_ROWS - 1) / SPMM_ROWS;
    const int per = (n_tiles + stc::kNumXcd - 1) / stc::kNumXcd;
    hipLaunchKernelGGL((spmm_wave_row_kernel<VPT, MODE, Fmt>), dim3(per * stc::kNumXcd, batch), dim3(SPMM_THREADS), 0, s, g.rowptr, g.colidx, g.val, n_rows, n_cols, X, FP,
                       n_tiles, ep);
}

template <int MODE, class Fmt>
int launch_gather(const char* who, const GraphArgs& g, int n_rows, int n_cols, const void* X, int batch, int FP, const typename Fmt::Epi& ep, hipStream_t s) {
    const Raw* Xp = static_cast<const Raw*>(X);
    if (g.blk_ptr) {
        // two waves share a row block, each covers every other column block of 64*VPT pieces (fp32 rows: 4 and 8 blocks per workgroup measured
        // slower); bf16 rows of at most 64 pieces (state planes at C = 32: 1 KiB) take one wave per block -- otherwise half the waves would idle
        if (Fmt::ONE_WAVE_BLOCKS && FP <= 64) launch_row_blocks<1, MODE, Fmt::ONE_WAVE_BLOCKS ? 4 : 2, Fmt>(g, n_rows, n_cols, Xp, batch, FP, ep, s);
        else if (FP <= 128) launch_row_blocks<1, MODE, 2, Fmt>(g, n_rows, n_cols, Xp, batch, FP, ep, s);
        else if (FP <= 256 || Fmt::MAX_VPT == 2) launch_row_blocks<2, MODE, 2, Fmt>(g, n_rows, n_cols, Xp, batch, FP, ep, s);
        else launch_row_blocks<Fmt::MAX_VPT, MODE, 2, Fmt>(g, n_rows, n_cols, Xp, batch, FP, ep, s);
    } else {
        if (FP <= 64) launch_wave_rows<1, MODE, Fmt>(g, n_rows, n_cols, Xp, batch, FP, ep, s);
        else if (FP <= 128 || Fmt::MAX_VPT == 2) launch_wave_rows<2, MODE, Fmt>(g, n_rows, n_cols, Xp, batch, FP, ep, s);
        else launch_wave_rows<Fmt::MAX_VPT, MODE, Fmt>(g, n_rows, n_cols, Xp, batch, FP, ep, s);
    }
    return stc::launched(who);
}

}  // namespace
