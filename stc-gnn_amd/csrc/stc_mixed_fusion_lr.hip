// Rank-r MixedFusion (STC_GNN.py FactorisedLinear / MixedFusion(n, rank=r); not in the reference, whose two Linear(n^2, n^2) layers do not fit
// one GPU beyond n ~ 200):
//
//     t_A = V_A^T a,  t_P = V_P^T p                                   U_A, V_A, U_P, V_P (D, r) row-major, D = n^2, a = vec(A), p = vec(P)
//     gate = sigmoid(U_A t_A + b_A + U_P t_P + b_P),   G = gate * A + (1 - gate) * P
//     dpre = dG (A - P) gate (1 - gate) = db_A = db_P;   dU_A = dpre (x) t_A;   s_A = U_A^T dpre;   dV_A = a (x) s_A;   dA = dG gate + V_A s_A
//     (and the same with P; dP = dG (1 - gate) + V_P s_P)
//
// The factors are a few MB: the work is launch-bound, so each direction is two launches.  The first leaves, per chunk of STC_FUSION_LR_CHUNK
// rows, the chunk's share of the 2r column sums (t forward, s backward) as doubles in the workspace -- fp32 per thread, float64 from the wave
// up, no atomics, as in stc_loss.hip; the backward's first launch also forms dpre and writes db and the dU rows.  The second launch has
// every workgroup fold the partials itself in one fixed order (bitwise reproducible) and then works row by row.
//
// Two forms of every kernel:
//   vector  r in {4, 8, 16, 32, 64}: r/4 lanes hold one matrix row as 16-byte pieces, so a wave reads 1 KiB of consecutive rows; a lane keeps
//           the same four columns over all its rows, and column sums are reduced across the lanes r/4 apart
//   plain   every other rank (and what the vector form is measured against): column sums with one wave per column, row products with one
//           thread per row, outer products element by element
// Default cache policy throughout: the backward re-reads what the forward read.
#include "stc_common.h"

namespace {

using v4f = __attribute__((ext_vector_type(4))) float;
constexpr int LR_THREADS = 256, LR_WAVES = LR_THREADS / stc::kWave, LR_MAX_RANK = 64;
static_assert(STC_FUSION_LR_CHUNK % LR_THREADS == 0, "a chunk is whole passes of a workgroup in every form (256 >> lg rows per pass)");

// sum over the lanes `from`, 2 `from`, ... 32 apart: the partial sum that leaves one total per group of `from` neighbouring lanes
__device__ __forceinline__ double lr_strided_lane_sum(double v, int from) {
    for (int off = 32; off >= from; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// vector form: the chunk's column sums out of the lanes' registers -> part[0 .. 2r)
__device__ __forceinline__ void lr_store_partials(const v4f sa, const v4f sp, int lg, int r, double* __restrict__ part) {
    __shared__ double red[LR_WAVES][2 * LR_MAX_RANK];
    const int R4 = 1 << lg, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const double a = lr_strided_lane_sum((double)sa[c], R4), p = lr_strided_lane_sum((double)sp[c], R4);
        if (lane < R4) {                                     // lane = its column group q here
            red[wave][4 * lane + c] = a;
            red[wave][r + 4 * lane + c] = p;
        }
    }
    __syncthreads();
    if ((int)threadIdx.x < 2 * r) {
        double tot = red[0][threadIdx.x];
#pragma unroll
        for (int w = 1; w < LR_WAVES; ++w) tot += red[w][threadIdx.x];
        part[threadIdx.x] = tot;
    }
}

// plain form: wave w takes the columns w, w + 4, ... of [M_A | M_P] (rows of this chunk: `MA`, `MP` point at its first row), lane l the rows
// l, l + 64, ...; wa / wp: the row weights, indexed by the row within the chunk.  A side that is not needed gives zeros.
__device__ __forceinline__ void lr_plain_colsums(const float* __restrict__ MA, const float* __restrict__ MP, const float* wa, const float* wp, int rows,
                                                 int r, bool need_a, bool need_p, double* __restrict__ part) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int j = wave; j < 2 * r; j += LR_WAVES) {
        const bool is_p = j >= r;
        float acc = 0.f;
        if (is_p ? need_p : need_a) {
            const float* M = (is_p ? MP + (j - r) : MA + j);
            const float* w = is_p ? wp : wa;
            for (int i = lane; i < rows; i += 64) acc = fmaf(M[(size_t)i * r], w[i], acc);
        }
        const double tot = stc_wave_sum((double)acc);
        if (lane == 0) part[j] = tot;
    }
}

// every workgroup of a second launch: out[j] = (float) sum over chunks of part[chunk][j], j < W = 2r.  256 / W groups of threads take the
// chunks g, g + groups, ... in order, thread j then adds the groups in order: one fixed order for a given (chunks, r).
__device__ __forceinline__ void lr_fold(const double* __restrict__ part, int chunks, int W, float* out) {
    __shared__ double fold[LR_THREADS];
    const int groups = LR_THREADS / W, j = threadIdx.x % W, g = threadIdx.x / W;
    if (g < groups) {
        double acc = 0.0;
        for (int c = g; c < chunks; c += groups) acc += part[(size_t)c * W + j];
        fold[g * W + j] = acc;
    }
    __syncthreads();
    if ((int)threadIdx.x < W) {
        double tot = fold[threadIdx.x];
        for (int k = 1; k < groups; ++k) tot += fold[k * W + threadIdx.x];
        out[threadIdx.x] = (float)tot;
    }
    __syncthreads();
}

__device__ __forceinline__ v4f lr_load4(const float* p) { return v4f{p[0], p[1], p[2], p[3]}; }
__device__ __forceinline__ float lr_dot4(const v4f a, const v4f b) { return fmaf(a[3], b[3], fmaf(a[2], b[2], fmaf(a[1], b[1], a[0] * b[0]))); }
// sum over the R4 neighbouring lanes that hold one row
__device__ __forceinline__ float lr_row_sum(float v, int R4) {
    for (int off = 1; off < R4; off <<= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// ---- forward, first launch: part[chunk] = (V_A^T a | V_P^T p) over the chunk's rows.  lg >= 0: vector form with r = 4 << lg
__global__ __launch_bounds__(LR_THREADS) void lr_t_partials_kernel(const float* __restrict__ VA, const float* __restrict__ VP, const float* __restrict__ A,
                                                                   const float* __restrict__ P, double* __restrict__ part, int D, int r, int lg) {
    const int row0 = blockIdx.x * STC_FUSION_LR_CHUNK, row1 = min(D, row0 + STC_FUSION_LR_CHUNK);
    double* out = part + (size_t)blockIdx.x * 2 * r;
    if (lg < 0) {
        lr_plain_colsums(VA + (size_t)row0 * r, VP + (size_t)row0 * r, A + row0, P + row0, row1 - row0, r, true, true, out);
        return;
    }
    const int R4 = 1 << lg, q = threadIdx.x & (R4 - 1), step = LR_THREADS >> lg;
    v4f sa = {0.f, 0.f, 0.f, 0.f}, sp = {0.f, 0.f, 0.f, 0.f};
    for (int row = row0 + ((int)threadIdx.x >> lg); row < row1; row += step) {
        const size_t piece = (size_t)row * R4 + q;
        const v4f va = reinterpret_cast<const v4f*>(VA)[piece], vp = reinterpret_cast<const v4f*>(VP)[piece];
        const float a = A[row], p = P[row];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            sa[c] = fmaf(va[c], a, sa[c]);
            sp[c] = fmaf(vp[c], p, sp[c]);
        }
    }
    lr_store_partials(sa, sp, lg, r, out);
}

// ---- forward, second launch: t = fold(part) (workgroup 0 stores it), then gate and G for the chunk's rows
__global__ __launch_bounds__(LR_THREADS) void lr_gate_kernel(const float* __restrict__ UA, const float* __restrict__ bA, const float* __restrict__ UP,
                                                             const float* __restrict__ bP, const float* __restrict__ A, const float* __restrict__ P,
                                                             const double* __restrict__ part, int chunks, float* __restrict__ gate, float* __restrict__ G,
                                                             float* __restrict__ t_out, int D, int r, int lg) {
    __shared__ float t[2 * LR_MAX_RANK];
    lr_fold(part, chunks, 2 * r, t);
    if (blockIdx.x == 0 && (int)threadIdx.x < 2 * r) t_out[threadIdx.x] = t[threadIdx.x];
    const int row0 = blockIdx.x * STC_FUSION_LR_CHUNK, row1 = min(D, row0 + STC_FUSION_LR_CHUNK);
    auto finish = [&](int row, float sa, float sp) {
        const float g = stc_sigmoid((sa + bA[row]) + (sp + bP[row]));         // lin_A(a) + lin_P(p), as MixedFusion.forward adds them
        gate[row] = g;
        G[row] = g * A[row] + (1.f - g) * P[row];
    };
    if (lg < 0) {
        for (int row = row0 + threadIdx.x; row < row1; row += LR_THREADS) {
            const float* ua = UA + (size_t)row * r;
            const float* up = UP + (size_t)row * r;
            float sa = 0.f, sp = 0.f;
            for (int j = 0; j < r; ++j) {
                sa = fmaf(ua[j], t[j], sa);
                sp = fmaf(up[j], t[r + j], sp);
            }
            finish(row, sa, sp);
        }
        return;
    }
    const int R4 = 1 << lg, q = threadIdx.x & (R4 - 1), step = LR_THREADS >> lg;
    const v4f ta = lr_load4(t + 4 * q), tp = lr_load4(t + r + 4 * q);
    for (int base = row0; base < row1; base += step) {                        // (uniform trip count: every lane takes part in the row sums)
        const int row = base + ((int)threadIdx.x >> lg);
        const bool live = row < row1;
        float sa = 0.f, sp = 0.f;
        if (live) {
            const size_t piece = (size_t)row * R4 + q;
            sa = lr_dot4(reinterpret_cast<const v4f*>(UA)[piece], ta);
            sp = lr_dot4(reinterpret_cast<const v4f*>(UP)[piece], tp);
        }
        sa = lr_row_sum(sa, R4);
        sp = lr_row_sum(sp, R4);
        if (live && q == 0) finish(row, sa, sp);
    }
}

// ---- backward, first launch: dpre -> db, the dU rows, part[chunk] = (U_A^T dpre | U_P^T dpre) over the chunk's rows (a side nobody wants: zeros)
__global__ __launch_bounds__(LR_THREADS) void lr_bwd_cols_kernel(const float* __restrict__ UA, const float* __restrict__ UP, const float* __restrict__ A,
                                                                 const float* __restrict__ P, const float* __restrict__ gate, const float* __restrict__ t,
                                                                 const float* __restrict__ dG, float* __restrict__ dUA, float* __restrict__ dUP,
                                                                 float* __restrict__ db, double* __restrict__ part, int need_sa, int need_sp, int D, int r,
                                                                 int lg) {
    const int row0 = blockIdx.x * STC_FUSION_LR_CHUNK, row1 = min(D, row0 + STC_FUSION_LR_CHUNK);
    double* out = part + (size_t)blockIdx.x * 2 * r;
    auto dpre_of = [&](int row) {
        const float g = gate[row];
        return dG[row] * (A[row] - P[row]) * g * (1.f - g);
    };
    if (lg < 0) {
        __shared__ float dpre[STC_FUSION_LR_CHUNK];
        __shared__ float ts[2 * LR_MAX_RANK];
        const int rows = row1 - row0;
        for (int i = threadIdx.x; i < rows; i += LR_THREADS) {
            const float d = dpre_of(row0 + i);
            dpre[i] = d;
            db[row0 + i] = d;
        }
        if ((int)threadIdx.x < 2 * r) ts[threadIdx.x] = t[threadIdx.x];
        __syncthreads();
        if (dUA || dUP) {
            for (int e = threadIdx.x; e < rows * r; e += LR_THREADS) {
                const int i = e / r, j = e - i * r;
                if (dUA) dUA[(size_t)row0 * r + e] = dpre[i] * ts[j];
                if (dUP) dUP[(size_t)row0 * r + e] = dpre[i] * ts[r + j];
            }
        }
        lr_plain_colsums(UA + (size_t)row0 * r, UP + (size_t)row0 * r, dpre, dpre, rows, r, need_sa, need_sp, out);
        return;
    }
    const int R4 = 1 << lg, q = threadIdx.x & (R4 - 1), step = LR_THREADS >> lg;
    const v4f ta = lr_load4(t + 4 * q), tp = lr_load4(t + r + 4 * q);
    v4f sa = {0.f, 0.f, 0.f, 0.f}, sp = {0.f, 0.f, 0.f, 0.f};
    for (int row = row0 + ((int)threadIdx.x >> lg); row < row1; row += step) {
        const size_t piece = (size_t)row * R4 + q;
        const float d = dpre_of(row);                                        // (the r/4 lanes of a row form it alike)
        if (q == 0) db[row] = d;
        if (dUA) reinterpret_cast<v4f*>(dUA)[piece] = d * ta;
        if (dUP) reinterpret_cast<v4f*>(dUP)[piece] = d * tp;
        if (need_sa) {
            const v4f ua = reinterpret_cast<const v4f*>(UA)[piece];
#pragma unroll
            for (int c = 0; c < 4; ++c) sa[c] = fmaf(ua[c], d, sa[c]);
        }
        if (need_sp) {
            const v4f up = reinterpret_cast<const v4f*>(UP)[piece];
#pragma unroll
            for (int c = 0; c < 4; ++c) sp[c] = fmaf(up[c], d, sp[c]);
        }
    }
    lr_store_partials(sa, sp, lg, r, out);
}

// ---- backward, second launch: s = fold(part), then the dV rows, dA and dP for the chunk's rows (each where wanted)
__global__ __launch_bounds__(LR_THREADS) void lr_bwd_rows_kernel(const float* __restrict__ VA, const float* __restrict__ VP, const float* __restrict__ A,
                                                                 const float* __restrict__ P, const float* __restrict__ gate, const float* __restrict__ dG,
                                                                 const double* __restrict__ part, int chunks, float* __restrict__ dVA,
                                                                 float* __restrict__ dVP, float* __restrict__ dA, float* __restrict__ dP, int D, int r, int lg) {
    __shared__ float s[2 * LR_MAX_RANK];
    lr_fold(part, chunks, 2 * r, s);
    const int row0 = blockIdx.x * STC_FUSION_LR_CHUNK, row1 = min(D, row0 + STC_FUSION_LR_CHUNK);
    auto finish = [&](int row, float da, float dp) {
        const float g = gate[row], d = dG[row];
        if (dA) dA[row] = d * g + da;
        if (dP) dP[row] = d * (1.f - g) + dp;
    };
    if (lg < 0) {
        const int rows = row1 - row0;
        if (dVA || dVP) {
            for (int e = threadIdx.x; e < rows * r; e += LR_THREADS) {
                const int i = e / r, j = e - i * r;
                if (dVA) dVA[(size_t)row0 * r + e] = A[row0 + i] * s[j];
                if (dVP) dVP[(size_t)row0 * r + e] = P[row0 + i] * s[r + j];
            }
        }
        if (dA || dP) {
            for (int row = row0 + threadIdx.x; row < row1; row += LR_THREADS) {
                float da = 0.f, dp = 0.f;
                if (dA)
                    for (int j = 0; j < r; ++j) da = fmaf(VA[(size_t)row * r + j], s[j], da);
                if (dP)
                    for (int j = 0; j < r; ++j) dp = fmaf(VP[(size_t)row * r + j], s[r + j], dp);
                finish(row, da, dp);
            }
        }
        return;
    }
    const int R4 = 1 << lg, q = threadIdx.x & (R4 - 1), step = LR_THREADS >> lg;
    const v4f sa = lr_load4(s + 4 * q), sp = lr_load4(s + r + 4 * q);
    for (int base = row0; base < row1; base += step) {
        const int row = base + ((int)threadIdx.x >> lg);
        const bool live = row < row1;
        float da = 0.f, dp = 0.f;
        if (live) {
            const size_t piece = (size_t)row * R4 + q;
            if (dVA) reinterpret_cast<v4f*>(dVA)[piece] = A[row] * sa;
            if (dVP) reinterpret_cast<v4f*>(dVP)[piece] = P[row] * sp;
            if (dA) da = lr_dot4(reinterpret_cast<const v4f*>(VA)[piece], sa);
            if (dP) dp = lr_dot4(reinterpret_cast<const v4f*>(VP)[piece], sp);
        }
        if (dA) da = lr_row_sum(da, R4);
        if (dP) dp = lr_row_sum(dp, R4);
        if (live && q == 0) finish(row, da, dp);
    }
}

// log2(r / 4) where the vector form takes the rank, -1 for the plain form
inline int lr_form(int32_t r) {
    for (int lg = 0; lg <= 4; ++lg)
        if (r == (4 << lg)) return lg;
    return -1;
}

inline long long lr_chunks(int32_t D) { return ((long long)D + STC_FUSION_LR_CHUNK - 1) / STC_FUSION_LR_CHUNK; }

// the size checks both directions share
int lr_checked(const char* what, int32_t D, int32_t r) {
    STC_REQUIRE(D >= 1, STC_EINVAL, "%s: D = n^2 = %d must be positive", what, D);
    STC_REQUIRE(r >= 1 && r <= LR_MAX_RANK, STC_EUNSUPPORTED, "%s: rank %d outside [1, %d] (use the unfused products)", what, r, LR_MAX_RANK);
    STC_REQUIRE((long long)D * r < (1ll << 31), STC_ELIMIT, "%s: D r = %lld must be below 2^31", what, (long long)D * r);
    return STC_OK;
}

}  // namespace

extern "C" int stc_mixed_fusion_lr_supported(int32_t D, int32_t r) {
    return D >= 1 && r >= 1 && r <= LR_MAX_RANK && (long long)D * r < (1ll << 31);
}

extern "C" size_t stc_mixed_fusion_lr_workspace_bytes(int32_t D, int32_t r) {
    return stc_mixed_fusion_lr_supported(D, r) ? (size_t)lr_chunks(D) * 2 * (size_t)r * sizeof(double) : 0;
}

extern "C" int stc_mixed_fusion_lr_fwd_f32(const float* UA, const float* VA, const float* bA, const float* UP, const float* VP, const float* bP,
                                           const float* A, const float* P, float* gate, float* G, float* t, void* workspace, size_t workspace_bytes,
                                           int32_t D, int32_t r, void* stream) {
    if (int rc = lr_checked("stc_mixed_fusion_lr_fwd_f32", D, r)) return rc;
    STC_REQUIRE(UA && VA && bA && UP && VP && bP && A && P && gate && G && t && workspace, STC_EINVAL, "stc_mixed_fusion_lr_fwd_f32: null pointer");
    STC_REQUIRE(stc::aligned16(UA) && stc::aligned16(VA) && stc::aligned16(UP) && stc::aligned16(VP), STC_EALIGN,
                "stc_mixed_fusion_lr_fwd_f32: U_A / V_A / U_P / V_P must be 16-byte aligned");
    STC_REQUIRE(stc::aligned(bA, 4) && stc::aligned(bP, 4) && stc::aligned(A, 4) && stc::aligned(P, 4) && stc::aligned(gate, 4) && stc::aligned(G, 4) && stc::aligned(t, 4),
                STC_EALIGN, "stc_mixed_fusion_lr_fwd_f32: vectors must be 4-byte aligned");
    STC_REQUIRE(stc::aligned(workspace, 8), STC_EALIGN, "stc_mixed_fusion_lr_fwd_f32: workspace must be 8-byte aligned");
    const size_t need = stc_mixed_fusion_lr_workspace_bytes(D, r);
    STC_REQUIRE(workspace_bytes >= need, STC_EINVAL, "stc_mixed_fusion_lr_fwd_f32: workspace of %zu bytes, %zu needed", workspace_bytes, need);
    STC_REQUIRE(gate != A && gate != P && G != A && G != P && G != gate, STC_EINVAL, "stc_mixed_fusion_lr_fwd_f32: gate and G must not alias A, P or each other");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int chunks = (int)lr_chunks(D), lg = lr_form(r);
    double* part = static_cast<double*>(workspace);
    const dim3 grid((unsigned)chunks), block(LR_THREADS);
    hipLaunchKernelGGL(lr_t_partials_kernel, grid, block, 0, s, VA, VP, A, P, part, (int)D, (int)r, lg);
    STC_LAUNCH_CHECK("stc_mixed_fusion_lr_fwd_f32 partials launch");
    hipLaunchKernelGGL(lr_gate_kernel, grid, block, 0, s, UA, bA, UP, bP, A, P, part, chunks, gate, G, t, (int)D, (int)r, lg);
    STC_LAUNCH_CHECK("stc_mixed_fusion_lr_fwd_f32 gate launch");
    return STC_OK;
}

extern "C" int stc_mixed_fusion_lr_bwd_f32(const float* UA, const float* VA, const float* UP, const float* VP, const float* A, const float* P,
                                           const float* gate, const float* t, const float* dG, float* dUA, float* dVA, float* dUP, float* dVP, float* db,
                                           float* dA, float* dP, void* workspace, size_t workspace_bytes, int32_t D, int32_t r, void* stream) {
    if (int rc = lr_checked("stc_mixed_fusion_lr_bwd_f32", D, r)) return rc;
    STC_REQUIRE(UA && VA && UP && VP && A && P && gate && t && dG && db && workspace, STC_EINVAL,
                "stc_mixed_fusion_lr_bwd_f32: null pointer (only dU_A, dV_A, dU_P, dV_P, dA and dP may be NULL: not wanted)");
    STC_REQUIRE(stc::aligned16(UA) && stc::aligned16(VA) && stc::aligned16(UP) && stc::aligned16(VP) && stc::aligned16(dUA) && stc::aligned16(dVA) &&
                    stc::aligned16(dUP) && stc::aligned16(dVP),
                STC_EALIGN, "stc_mixed_fusion_lr_bwd_f32: the factors and their gradients must be 16-byte aligned");
    STC_REQUIRE(stc::aligned(A, 4) && stc::aligned(P, 4) && stc::aligned(gate, 4) && stc::aligned(t, 4) && stc::aligned(dG, 4) && stc::aligned(db, 4) && stc::aligned(dA, 4) &&
                    stc::aligned(dP, 4),
                STC_EALIGN, "stc_mixed_fusion_lr_bwd_f32: vectors must be 4-byte aligned");
    STC_REQUIRE(stc::aligned(workspace, 8), STC_EALIGN, "stc_mixed_fusion_lr_bwd_f32: workspace must be 8-byte aligned");
    const size_t need = stc_mixed_fusion_lr_workspace_bytes(D, r);
    STC_REQUIRE(workspace_bytes >= need, STC_EINVAL, "stc_mixed_fusion_lr_bwd_f32: workspace of %zu bytes, %zu needed", workspace_bytes, need);
    for (const float* out : {(const float*)dUA, (const float*)dVA, (const float*)dUP, (const float*)dVP, (const float*)db, (const float*)dA, (const float*)dP})
        STC_REQUIRE(!out || (out != UA && out != VA && out != UP && out != VP && out != A && out != P && out != gate && out != dG && out != t), STC_EINVAL,
                    "stc_mixed_fusion_lr_bwd_f32: a gradient must not alias an input");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int chunks = (int)lr_chunks(D), lg = lr_form(r);
    double* part = static_cast<double*>(workspace);
    const dim3 grid((unsigned)chunks), block(LR_THREADS);
    const int need_sa = dVA || dA, need_sp = dVP || dP;                       // s_A = U_A^T dpre feeds dV_A and dA only
    hipLaunchKernelGGL(lr_bwd_cols_kernel, grid, block, 0, s, UA, UP, A, P, gate, t, dG, dUA, dUP, db, part, need_sa, need_sp, (int)D, (int)r, lg);
    STC_LAUNCH_CHECK("stc_mixed_fusion_lr_bwd_f32 column launch");
    if (need_sa || need_sp) {
        hipLaunchKernelGGL(lr_bwd_rows_kernel, grid, block, 0, s, VA, VP, A, P, gate, dG, part, chunks, dVA, dVP, dA, dP, (int)D, (int)r, lg);
        STC_LAUNCH_CHECK("stc_mixed_fusion_lr_bwd_f32 row launch");
    }
    return STC_OK;
}
