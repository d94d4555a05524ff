// CSR / row-blocked CSR SpMM and SDDMM for the spatial (1-mode) aggregation of STC-GNN on gfx950.
//
//   Y[b,i,:] = alpha * sum_j val[j] * X[b, col[j], :] + beta * Y0[b,i,:]
//
// Replaces torch.einsum('bncl,nm->bmcl', X, T_n(Gs)) (reference STC_GNN.py:37) and, with (alpha,beta) = (2,-1),
// one step of the Chebyshev recurrence of STC_GNN.py:28 applied on the feature side.  HBM-bound: a feature row
// is F = C*L contiguous floats (4 KiB at C=32, L=32), streamed with one 16-byte load per lane, 1 KiB per wave
// instruction.
//
// The vector path -- rows of whole 16-byte pieces -- runs on the gather kernels of stc_spmm_gather.h (their layout is described there) with the
// fp32 format below: a lane's piece is a float4.  Output pieces are written with non-temporal stores (written once; keeps the output stream
// from evicting the X rows the neighbours still need from L2); Y0 is read non-temporally for the same reason.
//
// Epilogues: the GRU blend of the forward (EP_BLEND: Cand = tanh(A + S.Bm), Hnew = (1-U) H + U Cand, reference STC_GNN.py:76-78) and the
// state-gradient sums of the backward (EP_SUM / EP_SUM2: Y = sum of addend planes + alpha S.(X [+ X2]), optionally with the blend backward
// dY = Y U (1 - Cand^2) and the launch's max |Y| on the way) run on the accumulators, so neither intermediate is written to HBM.
#include "stc_spmm_gather.h"

namespace {

__device__ __forceinline__ void fma4(float4& acc, float s, const float4& x) {      // (the narrow-row kernel below)
    acc.x = fmaf(s, x.x, acc.x);
    acc.y = fmaf(s, x.y, acc.y);
    acc.z = fmaf(s, x.z, acc.z);
    acc.w = fmaf(s, x.w, acc.w);
}

struct EpiArgs {
    const Raw* Y0;                          // base term (PLAIN: optional, scaled by beta; BLEND: A)
    Raw* Y;                                 // PLAIN / SUM output
    float alpha, beta;                      // PLAIN (SUM: alpha)
    int C, h;                               // row geometry: rows of C categories x h = 16 floats
    const float *H, *U;                     // BLEND inputs, (rows*C, h)
    // BLEND (forward, post-aggregation candidate convolution): Y0 = A (bias included), rows of C*h floats;
    // Cand = tanh(A + S.Bm), Hnew = (1-U)*H + U*Cand, plus the state copies of stc_cell_blend_fwd_f32
    float *Cand, *Hnew;                     // (rows*C, h)
    float* copy[2]; int copy_ld[2], copy_off[2];
    const float* side_src; int side_cin;    // belongs to copy[0]
    // SUM / SUM2 (gradient of a state from its consumers' pieces): Y = sum_i add[i] + S.(X [+ X2]), rows of C*h floats;
    // add[i] = columns [off, off+h) of rows of ld floats (a contiguous plane: ld = h, off = 0)
    const Raw* X2;                          // SUM2: second gathered operand (same batch stride as X)
    const float* add[STC_SPMM_SUM_MAX_ADD]; int add_ld[STC_SPMM_SUM_MAX_ADD], add_off[STC_SPMM_SUM_MAX_ADD], n_add;
    float add_scale[STC_SPMM_SUM_MAX_ADD];   // SUM: Y = sum_i add_scale[i] add[i] + alpha S.(X [+ X2])
    const float *gU, *gCand; float* dYout;  // SUM, optional: also dY = Y * U * (1 - Cand^2), the blend backward of the cell that owns the state
    unsigned* amax; int n_amax;             // SUM, optional: max |Y| of the launch as float bits, spread over n_amax slots (zero before the launch)
};

__device__ __forceinline__ const Raw* raw(const float* p) { return reinterpret_cast<const Raw*>(p); }
__device__ __forceinline__ Raw* raw(float* p) { return reinterpret_cast<Raw*>(p); }

// The sums of a float4 piece for the gather kernels: Piece<false>'s fmaf chain on four scalars.  As ONE vector value -- which the patch kernel
// needs -- the sums are carried round the gather loops in aligned register quads, and the pipelined row-block kernels then take 108 / 184 / 432
// registers where they take 96 / 160 / 366 with scalars (assembly of this file, VPT = 1 / 2 / 4).
struct Sums4 {
    float v[4];
    __device__ __forceinline__ void zero() { v[0] = v[1] = v[2] = v[3] = 0.f; }
    __device__ __forceinline__ void fma(float s, const Raw x) {
#pragma unroll
        for (int c = 0; c < 4; ++c) v[c] = fmaf(s, x[c], v[c]);
    }
};

// fp32 rows on the gather kernels (stc_spmm_gather.h names the members).  rowg = b*n_rows + row; ch = piece inside the row of F4 pieces;
// acc = sum_j val_j X[col_j] for that piece.  State rows (BLEND, SUM) are (category, h) with h = 16: piece ch = 4 * category + quarter.
struct RowsF32 {
    using Acc = Sums4;
    using Epi = EpiArgs;
    static constexpr int MAX_VPT = 4;
    static constexpr bool ONE_WAVE_BLOCKS = false, PIPELINED = true, BLEND_AHEAD_WAVE_ROW = false;

    template <bool TWO>
    struct Operand { Raw x; };              // X, or X + X2: summed as they arrive, one fma for both
    template <bool TWO>
    static __device__ __forceinline__ Operand<TWO> gather(const Raw* X, const Raw* X2, size_t at) {
        Operand<TWO> o{X[at]};
        if (TWO) o.x += X2[at];
        return o;
    }
    template <bool TWO>
    static __device__ __forceinline__ void accumulate(Acc& acc, float s, const Operand<TWO>& o) { acc.fma(s, o.x); }

    static __device__ __forceinline__ BlendIn blend_operands(const Epi& ep, size_t o) {
        return BlendIn{stc_ld_once(ep.Y0 + o), stc_ld_once(raw(ep.U + 4 * o)), stc_ld_once(raw(ep.H + 4 * o))};
    }
    // the GRU blend on one piece of a (row, category) state row, plus its copies.
    // Hnew = (1-U) H + U Cand has one rounding fewer than its written form, and WHICH product is fused into the sum was the compiler's choice for
    // as long as it was written that way: fma(1-u, h, u c), except on elements 2 and 3 of a piece in the row-block kernel, fma(u, c, (1-u) h).
    // Spelled out here so that the bits every earlier build produced do not move with the next change of the surrounding code.
    template <bool ROW_BLOCK>
    static __device__ __forceinline__ void blend(const Epi& a, size_t rowg, int F4, int ch, const Acc& acc, const BlendIn& in) {
        const size_t o = rowg * F4 + ch;
        const Raw u = in.u, hh = in.h;
        Raw c, hn;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            c[i] = tanh_fast(acc.v[i] + in.a[i]);
            hn[i] = ROW_BLOCK && i >= 2 ? fmaf(u[i], c[i], (1.f - u[i]) * hh[i]) : fmaf(1.f - u[i], hh[i], u[i] * c[i]);
        }
        if (a.Cand) stc_st_once(raw(a.Cand + 4 * o), c);     // (optional: only a backward reads the candidate)
        stc_st_once(raw(a.Hnew + 4 * o), hn);
        const int q4 = ch & 3;
        const size_t e = rowg * a.C + (ch >> 2);
#pragma unroll
        for (int k = 0; k < 2; ++k)
            if (a.copy[k]) {
                float* dst = a.copy[k] + e * a.copy_ld[k] + a.copy_off[k] + 4 * q4;
                if (((a.copy_ld[k] | a.copy_off[k]) & 3) == 0) {
                    *raw(dst) = hn;
                } else {
                    dst[0] = hn[0]; dst[1] = hn[1]; dst[2] = hn[2]; dst[3] = hn[3];
                }
            }
        if (a.side_src) {                   // complete the consumer's row: its input columns and its zero padding
            float* drow = a.copy[0] + e * a.copy_ld[0];
            if (q4 == 0)
                for (int col = 0; col < a.side_cin; ++col) drow[col] = a.side_src[e * a.side_cin + col];
            if (q4 == 3)
                for (int col = a.side_cin + a.h; col < a.copy_ld[0]; ++col) drow[col] = 0.f;
        }
    }

    template <int MODE>      // EP_PLAIN, EP_SUM, EP_SUM2
    static __device__ __forceinline__ void finish(const Epi& a, size_t rowg, int F4, int ch, const Acc& acc, float& amax) {     // amax: running max |Y| (SUM forms)
        const size_t o = rowg * F4 + ch;
        Raw y;
#pragma unroll
        for (int i = 0; i < 4; ++i) y[i] = a.alpha * acc.v[i];
        if (MODE == EP_PLAIN) {
            if (a.beta != 0.f) {
                const Raw y0 = stc_ld_once(a.Y0 + o);
#pragma unroll
                for (int i = 0; i < 4; ++i) y[i] = fmaf(a.beta, y0[i], y[i]);
            }
            stc_st_once(a.Y + o, y);
            return;
        }
        const size_t e = rowg * a.C + (ch >> 2);
        const int q4 = ch & 3;
        for (int k = 0; k < a.n_add; ++k) {
            const Raw t = stc_ld_once(raw(a.add[k] + e * a.add_ld[k] + a.add_off[k] + 4 * q4));
            const float sc = a.add_scale[k];
#pragma unroll
            for (int i = 0; i < 4; ++i) y[i] = fmaf(sc, t[i], y[i]);
        }
        stc_st_once(a.Y + o, y);
        amax = fmaxf(fmaxf(amax, fmaxf(fabsf(y[0]), fabsf(y[1]))), fmaxf(fabsf(y[2]), fabsf(y[3])));
        if (a.dYout) {
            const Raw u = stc_ld_once(raw(a.gU + 4 * o)), c = stc_ld_once(raw(a.gCand + 4 * o));
            Raw d;
#pragma unroll
            for (int i = 0; i < 4; ++i) d[i] = y[i] * u[i] * (1.f - c[i] * c[i]);
            stc_st_once(raw(a.dYout) + o, d);
        }
    }

    // SUM / SUM2 with ep.amax: every wave leaves the largest |Y| it produced in one of the slots (atomic max on the bits of a non-negative
    // float, which order like the values) -- the consumer of Y (stc_cell_bwd_planar_f32, fp16 x 2 operand format) takes the maximum over the
    // slots as the launch's gradient scale, without another pass over Y and without a host round trip.  Slots spread the atomics over lines.
    template <int MODE>
    static __device__ __forceinline__ void wave_done(const Epi& ep, float m) {
        if (!((MODE == EP_SUM || MODE == EP_SUM2) && ep.amax)) return;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) m = fmaxf(m, __shfl_xor(m, off, 64));
        if ((threadIdx.x & 63) == 0 && m > 0.f) {
            const unsigned slot = (blockIdx.x + blockIdx.y * gridDim.x + (threadIdx.x >> 6) * 7u) % (unsigned)ep.n_amax;
            atomicMax(ep.amax + slot, __float_as_uint(m));
        }
    }
};

// ---- row-blocked, NARROW rows (F4 = F/4 in {1, 2, 4, 8, 16} float4 per row: the layer-0 input plane, C = 32 floats = 128 bytes) --------
// A 64-lane wave would leave all but F4 lanes idle on such rows, so it is split into G = 64 / F4 lane groups and each group
// produces its OWN block of 4 rows: 4 G rows per wave.  Block lists differ per group, so column / values are per-lane loads
// (identical within a group: one L1 transaction each) and the loop runs to the longest list with the finished groups masked.
// Same arithmetic order per row as spmm_bcsr_kernel (block list order, fmaf chain), plain epilogue Y = alpha S.X + beta Y0.
template <int F4>
__global__ __launch_bounds__(SPMM_THREADS) void spmm_bcsr_narrow_kernel(
    const int* __restrict__ blk_ptr, const int* __restrict__ blk_cols, const float4* __restrict__ blk_vals,
    int n_rows, int n_cols, const float4* __restrict__ X, const float4* __restrict__ Y0, float4* __restrict__ Y,
    int n_blocks, float alpha, float beta) {
    constexpr int G = 64 / F4;                       // row blocks per wave
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int grp = lane / F4, ch = lane % F4;
    const int blk = (blockIdx.x * SPMM_WAVES + wave) * G + grp;
    const int b = blockIdx.y;
    if (blk >= n_blocks) return;                     // (no barriers in this kernel)
    const int js = blk_ptr[blk], je = blk_ptr[blk + 1];
    const float4* Xb = X + (size_t)b * n_cols * F4 + ch;
    float4 acc[BR];
#pragma unroll
    for (int r = 0; r < BR; ++r) acc[r] = make_float4(0.f, 0.f, 0.f, 0.f);
    int j = js;
    for (; j + 3 <= je; j += 3) {                    // three neighbour rows in flight per lane
        int c[3]; float4 v[3], x[3];
#pragma unroll
        for (int u = 0; u < 3; ++u) { c[u] = blk_cols[j + u]; v[u] = blk_vals[j + u]; }
#pragma unroll
        for (int u = 0; u < 3; ++u) x[u] = Xb[(size_t)c[u] * F4];
#pragma unroll
        for (int u = 0; u < 3; ++u) { fma4(acc[0], v[u].x, x[u]); fma4(acc[1], v[u].y, x[u]); fma4(acc[2], v[u].z, x[u]); fma4(acc[3], v[u].w, x[u]); }
    }
    for (; j < je; ++j) {
        const int c = blk_cols[j];
        const float4 v = blk_vals[j], x = Xb[(size_t)c * F4];
        fma4(acc[0], v.x, x); fma4(acc[1], v.y, x); fma4(acc[2], v.z, x); fma4(acc[3], v.w, x);
    }
#pragma unroll
    for (int r = 0; r < BR; ++r) {
        const int row = blk * BR + r;
        if (row < n_rows) {
            const size_t o = ((size_t)b * n_rows + row) * F4 + ch;
            float4 y = make_float4(alpha * acc[r].x, alpha * acc[r].y, alpha * acc[r].z, alpha * acc[r].w);
            if (beta != 0.f) {
                const float4 y0 = Y0[o];
                y.x = fmaf(beta, y0.x, y.x); y.y = fmaf(beta, y0.y, y.y); y.z = fmaf(beta, y0.z, y.z); y.w = fmaf(beta, y0.w, y.w);
            }
            Y[o] = y;
        }
    }
}

// Any F, any alignment (SF shape: F = C*L = 85): lanes_per_row threads share a row.
__global__ __launch_bounds__(SPMM_THREADS) void spmm_generic_kernel(
    const int* __restrict__ rowptr, const int* __restrict__ colidx, const float* __restrict__ val,
    int n_rows, int n_cols, const float* __restrict__ X, const float* Y0, float* Y,
    int F, float alpha, float beta, int lanes_per_row) {
    const int rows_per_block = SPMM_THREADS / lanes_per_row;
    const int r = threadIdx.x / lanes_per_row;
    const int lr = threadIdx.x % lanes_per_row;
    const int i = blockIdx.x * rows_per_block + r;
    if (i >= n_rows) return;
    const int b = blockIdx.y;
    const int js = rowptr[i], je = rowptr[i + 1];
    const float* Xb = X + (size_t)b * n_cols * F;
    const size_t orow = ((size_t)b * n_rows + i) * F;
    for (int f = lr; f < F; f += lanes_per_row) {
        float acc = 0.f;
        for (int j = js; j < je; ++j) acc = fmaf(val[j], Xb[(size_t)colidx[j] * F + f], acc);
        float o = alpha * acc;
        if (beta != 0.f) o = fmaf(beta, Y0[orow + f], o);
        Y[orow + f] = o;
    }
}

// out[j] (+)= alpha * sum_b <A[b,i,:], Bm[b,col[j],:]> ; one wave per stored entry.
__global__ __launch_bounds__(SPMM_THREADS) void sddmm_kernel(
    const int* __restrict__ rowptr, const int* __restrict__ colidx, int n_rows, int n_cols,
    const float* __restrict__ A, const float* __restrict__ Bm, float* out,
    int batch, int F, float alpha, int accumulate) {
    const int i = blockIdx.x;
    const int wave = threadIdx.x >> 6;
    const int lane = threadIdx.x & 63;
    const int js = rowptr[i], je = rowptr[i + 1];
    for (int j = js + wave; j < je; j += SPMM_WAVES) {
        const int c = colidx[j];
        float s = 0.f;
        for (int b = 0; b < batch; ++b) {
            const float* a = A + ((size_t)b * n_rows + i) * F;
            const float* bm = Bm + ((size_t)b * n_cols + c) * F;
            for (int f = lane; f < F; f += 64) s = fmaf(a[f], bm[f], s);
        }
        s = stc_wave_sum(s);
        if (lane == 0) out[j] = accumulate ? fmaf(alpha, s, out[j]) : alpha * s;
    }
}

int next_pow2(int v) {
    int p = 1;
    while (p < v) p <<= 1;
    return p;
}

EpiArgs plain_epi(const float* Y0, float* Y, float alpha, float beta) {      // Y = alpha S.X + beta Y0
    EpiArgs ep{};
    ep.Y0 = reinterpret_cast<const Raw*>(Y0); ep.Y = reinterpret_cast<Raw*>(Y); ep.alpha = alpha; ep.beta = beta;
    return ep;
}

// state rows on the fp32 vector kernels: X the gathered operand, Y0 the other plane of the same shape (A, or the result of a sum)
int check_fused(const char* who, const GraphArgs& g, int n_rows, int n_cols, const float* X, const float* Y0, int batch, int C, int h) {
    // the column / value arrays may be null for a graph without edges (pointer arrays all zero: they are never read)
    if (int rc = stc::check_state_rows(who, n_rows, batch, C, h, g.blk_ptr || g.rowptr)) return rc;
    STC_REQUIRE(n_cols >= 0, STC_EINVAL, "%s: bad sizes", who);
    STC_REQUIRE((long long)C * h >= 64, STC_ELIMIT, "%s: node row of %d floats is too narrow for the vector kernels", who, C * h);
    if (n_rows == 0 || batch == 0) return STC_OK;
    STC_REQUIRE(X && Y0 && n_cols > 0, STC_EINVAL, "%s: null X / Y0", who);
    STC_REQUIRE(stc::aligned16(X) && stc::aligned16(Y0), STC_EALIGN, "%s: X / Y0 must be 16-byte aligned", who);
    return STC_OK;
}

}  // namespace

extern "C" int stc_csr_spmm_f32(const int32_t* rowptr, const int32_t* colidx, const float* val,
                                int32_t n_rows, int32_t n_cols,
                                const float* X, const float* Y0, float* Y,
                                int32_t batch, int32_t F, float alpha, float beta, void* stream) {
    const stc::Plain p{n_rows, n_cols, batch, F, X, Y0, Y, beta};
    // colidx/val may be null for a graph without edges (rowptr all zero): they are then never read.  Any F at any alignment: the generic kernel below
    if (int rc = stc::check_plain("stc_csr_spmm_f32", p, rowptr && X && Y && n_cols > 0, 0, 0, 0)) return rc;
    if (p.empty()) return STC_OK;
    if (int rc = stc::check_batch("stc_csr_spmm_f32", batch)) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);

    const bool vec = (F % 4 == 0) && stc::aligned16(X) && stc::aligned16(Y) && (Y0 == nullptr || stc::aligned16(Y0)) && F >= 64;
    if (vec) {
        const GraphArgs g{rowptr, colidx, val, nullptr, nullptr, nullptr};
        return launch_gather<EP_PLAIN, RowsF32>("stc_csr_spmm_f32 launch", g, n_rows, n_cols, X, batch, F / 4, plain_epi(Y0, Y, alpha, beta), s);
    }
    const int lanes = next_pow2(F) < SPMM_THREADS ? next_pow2(F) : SPMM_THREADS;
    const int rows_per_block = SPMM_THREADS / lanes;
    dim3 grid((n_rows + rows_per_block - 1) / rows_per_block, batch), block(SPMM_THREADS);
    hipLaunchKernelGGL(spmm_generic_kernel, grid, block, 0, s, rowptr, colidx, val, n_rows, n_cols, X, Y0, Y, F, alpha, beta, lanes);
    return stc::launched("stc_csr_spmm_f32 launch");
}

extern "C" int stc_bcsr_spmm_f32(const int32_t* blk_ptr, const int32_t* blk_cols, const float* blk_vals,
                                 int32_t n_rows, int32_t n_cols,
                                 const float* X, const float* Y0, float* Y,
                                 int32_t batch, int32_t F, float alpha, float beta, void* stream) {
    const stc::Plain p{n_rows, n_cols, batch, F, X, Y0, Y, beta};
    if (int rc = stc::check_plain("stc_bcsr_spmm_f32", p, blk_ptr && X && Y, 4, 4, STC_EINVAL)) return rc;
    if (p.empty()) return STC_OK;
    if (int rc = stc::check_batch("stc_bcsr_spmm_f32", batch)) return rc;
    const int F4 = F / 4;
    if (F4 <= 16 && (F4 & (F4 - 1)) == 0) {            // narrow rows (<= 256 bytes): several row blocks per wave
        const int n_blocks = (n_rows + BR - 1) / BR;
        hipStream_t s = static_cast<hipStream_t>(stream);
#define STC_NARROW_GO(F4_) hipLaunchKernelGGL((spmm_bcsr_narrow_kernel<F4_>), dim3((n_blocks + SPMM_WAVES * (64 / F4_) - 1) / (SPMM_WAVES * (64 / F4_)), batch), \
                                              dim3(SPMM_THREADS), 0, s, blk_ptr, blk_cols, reinterpret_cast<const float4*>(blk_vals), n_rows, n_cols, \
                                              reinterpret_cast<const float4*>(X), reinterpret_cast<const float4*>(Y0), reinterpret_cast<float4*>(Y), n_blocks, alpha, beta)
        switch (F4) { case 1: STC_NARROW_GO(1); break; case 2: STC_NARROW_GO(2); break; case 4: STC_NARROW_GO(4); break;
                      case 8: STC_NARROW_GO(8); break; default: STC_NARROW_GO(16); break; }
#undef STC_NARROW_GO
        return stc::launched("stc_bcsr_spmm_f32 (narrow rows) launch");
    }
    const GraphArgs g{nullptr, nullptr, nullptr, blk_ptr, blk_cols, blk_vals};
    return launch_gather<EP_PLAIN, RowsF32>("stc_bcsr_spmm_f32 launch", g, n_rows, n_cols, X, batch, F / 4, plain_epi(Y0, Y, alpha, beta), static_cast<hipStream_t>(stream));
}

extern "C" int stc_spmm_blend_fwd_f32(const int32_t* rowptr, const int32_t* colidx, const float* val,
                                      const int32_t* blk_ptr, const int32_t* blk_cols, const float* blk_vals,
                                      int32_t n_rows, int32_t n_cols, const float* Bm, const float* A,
                                      const float* U, const float* H, float* Cand, float* Hnew,
                                      float* copy0, int32_t copy0_ld, int32_t copy0_off, const float* side_src, int32_t side_cin,
                                      float* copy1, int32_t copy1_ld, int32_t copy1_off,
                                      int32_t batch, int32_t C, int32_t h, void* stream) {
    const GraphArgs g{rowptr, colidx, val, blk_ptr, blk_cols, blk_vals};
    if (int rc = check_fused("stc_spmm_blend_fwd_f32", g, n_rows, n_cols, Bm, A, batch, C, h)) return rc;
    if (n_rows == 0 || batch == 0) return STC_OK;
    STC_REQUIRE(U && H && Hnew, STC_EINVAL, "stc_spmm_blend_fwd_f32: null pointer");      // (Cand may be null: not stored)
    STC_REQUIRE(stc::aligned16(U) && stc::aligned16(H) && (!Cand || stc::aligned16(Cand)) && stc::aligned16(Hnew), STC_EALIGN,
                "stc_spmm_blend_fwd_f32: operands must be 16-byte aligned");
    STC_REQUIRE(Bm != Cand && Bm != Hnew, STC_EINVAL, "stc_spmm_blend_fwd_f32: outputs must not alias Bm (its rows are gathered by other rows)");
    STC_REQUIRE((!copy0 || (copy0_off >= 0 && copy0_off + h <= copy0_ld)) && (!copy1 || (copy1_off >= 0 && copy1_off + h <= copy1_ld)),
                STC_EINVAL, "stc_spmm_blend_fwd_f32: state copy columns [off, off+%d) do not fit the row width", h);
    STC_REQUIRE(!side_src || (copy0 && side_cin >= 0 && side_cin == copy0_off), STC_EINVAL,
                "stc_spmm_blend_fwd_f32: side_src needs copy0 with copy0_off == side_cin");
    STC_REQUIRE((!copy0 || (reinterpret_cast<uintptr_t>(copy0) & 3u) == 0) && (!copy1 || (reinterpret_cast<uintptr_t>(copy1) & 3u) == 0),
                STC_EALIGN, "stc_spmm_blend_fwd_f32: misaligned copy destination");
    if (copy0 && ((copy0_ld | copy0_off) & 3) == 0) STC_REQUIRE(stc::aligned16(copy0), STC_EALIGN, "stc_spmm_blend_fwd_f32: copy0 not 16-byte aligned");
    if (copy1 && ((copy1_ld | copy1_off) & 3) == 0) STC_REQUIRE(stc::aligned16(copy1), STC_EALIGN, "stc_spmm_blend_fwd_f32: copy1 not 16-byte aligned");
    EpiArgs ep{};
    ep.Y0 = reinterpret_cast<const Raw*>(A);
    ep.C = C; ep.h = h;
    ep.U = U; ep.H = H; ep.Cand = Cand; ep.Hnew = Hnew;
    ep.copy[0] = copy0; ep.copy_ld[0] = copy0_ld; ep.copy_off[0] = copy0_off;
    ep.copy[1] = copy1; ep.copy_ld[1] = copy1_ld; ep.copy_off[1] = copy1_off;
    ep.side_src = copy0 ? side_src : nullptr; ep.side_cin = side_cin;
    return launch_gather<EP_BLEND, RowsF32>("stc_spmm_blend_fwd_f32 launch", g, n_rows, n_cols, Bm, batch, C * h / 4, ep, static_cast<hipStream_t>(stream));
}

extern "C" int stc_spmm_sum_f32(const int32_t* rowptr, const int32_t* colidx, const float* val,
                                const int32_t* blk_ptr, const int32_t* blk_cols, const float* blk_vals,
                                int32_t n_rows, int32_t n_cols, const float* X, const float* X2, float alpha,
                                int32_t n_add, const float* const* add, const int32_t* add_ld, const int32_t* add_off, const float* add_scale,
                                float* Y, const float* U, const float* Cand, float* dY,
                                float* amax, int32_t n_amax,
                                int32_t batch, int32_t C, int32_t h, void* stream) {
    const GraphArgs g{rowptr, colidx, val, blk_ptr, blk_cols, blk_vals};
    STC_REQUIRE(h == 16, STC_EUNSUPPORTED, "stc_spmm_sum_f32: hidden width %d (built for 16)", h);
    STC_REQUIRE(!amax || n_amax >= 1, STC_EINVAL, "stc_spmm_sum_f32: amax with %d slots", n_amax);
    if (int rc = stc::check_addend_count("stc_spmm_sum_f32", "addend", n_add, 0, STC_SPMM_SUM_MAX_ADD, STC_EINVAL)) return rc;
    STC_REQUIRE(n_add == 0 || (add && add_ld && add_off), STC_EINVAL, "stc_spmm_sum_f32: null list of addends, ld or off");
    if (int rc = check_fused("stc_spmm_sum_f32", g, n_rows, n_cols, X, Y, batch, C, h)) return rc;      // (Y checked as the aligned "Y0" operand)
    if (n_rows == 0 || batch == 0) return STC_OK;
    STC_REQUIRE(X != Y && X2 != Y, STC_EINVAL, "stc_spmm_sum_f32: Y must not alias a gathered operand");
    STC_REQUIRE(!X2 || stc::aligned16(X2), STC_EALIGN, "stc_spmm_sum_f32: X2 not 16-byte aligned");
    EpiArgs ep{};
    ep.Y = reinterpret_cast<Raw*>(Y);
    ep.C = C; ep.h = h;
    ep.X2 = reinterpret_cast<const Raw*>(X2);
    if (int rc = stc::check_dy("stc_spmm_sum_f32", dY, U, Cand, Y)) return rc;
    ep.gU = U; ep.gCand = Cand; ep.dYout = dY;
    ep.amax = reinterpret_cast<unsigned*>(amax); ep.n_amax = n_amax;
    ep.alpha = alpha;
    ep.n_add = n_add;
    if (int rc = stc::check_addends("stc_spmm_sum_f32", "addend", add, n_add, Y, nullptr)) return rc;
    for (int i = 0; i < n_add; ++i) {
        STC_REQUIRE(add_off[i] >= 0 && add_off[i] + h <= add_ld[i] && ((add_ld[i] | add_off[i]) & 3) == 0, STC_EINVAL,
                    "stc_spmm_sum_f32: addend %d (ld %d, off %d): columns [off, off+%d) of rows of ld floats, ld and off multiples of 4", i, add_ld[i], add_off[i], h);
        ep.add[i] = add[i]; ep.add_ld[i] = add_ld[i]; ep.add_off[i] = add_off[i]; ep.add_scale[i] = add_scale ? add_scale[i] : 1.f;
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    return X2 ? launch_gather<EP_SUM2, RowsF32>("stc_spmm_sum_f32 launch", g, n_rows, n_cols, X, batch, C * h / 4, ep, s)
              : launch_gather<EP_SUM, RowsF32>("stc_spmm_sum_f32 launch", g, n_rows, n_cols, X, batch, C * h / 4, ep, s);
}

extern "C" int stc_csr_sddmm_f32(const int32_t* rowptr, const int32_t* colidx,
                                 int32_t n_rows, int32_t n_cols,
                                 const float* A, const float* Bm, float* out,
                                 int32_t batch, int32_t F, float alpha, int32_t accumulate, void* stream) {
    STC_REQUIRE(n_rows >= 0 && n_cols >= 0 && batch >= 0 && F >= 0, STC_EINVAL, "stc_csr_sddmm_f32: negative size");
    if (n_rows == 0) return STC_OK;
    STC_REQUIRE(rowptr && colidx && out, STC_EINVAL, "stc_csr_sddmm_f32: null rowptr/colidx/out");
    STC_REQUIRE((batch == 0 || F == 0) || (A && Bm), STC_EINVAL, "stc_csr_sddmm_f32: null A/Bm");
    hipLaunchKernelGGL(sddmm_kernel, dim3(n_rows), dim3(SPMM_THREADS), 0, static_cast<hipStream_t>(stream),
                       rowptr, colidx, n_rows, n_cols, A, Bm, out, batch, F, alpha, accumulate);
    return stc::launched("stc_csr_sddmm_f32 launch");
}
