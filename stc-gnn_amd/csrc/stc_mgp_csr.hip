// The learned spatial graph of MGP_Gen (reference STC_GNN.py:229-232) restricted to a sparsity pattern -- that of the prior graph, CSR of Gs
// itself (entry e = (i, j) sits in row i) -- and its autograd.  U, V (R, KH) are what stc_mgp_uv_fwd_f32 writes: one contiguous row of
// KH = K h floats per node.
//
//     score_e = <u_i, v_j> - <v_i, u_j>                                   the einsum pair of :231, sampled at e
//     Ps_e    = softmax over the STORED entries of row i of relu(score)   an entry whose relu is 0 still adds exp(0 - m_i) to the denominator
//     ds_e    = [score_e > 0] Ps_e (dPs_e - sum_{row i} Ps dPs)           a NaN score passes the mask, as in stc_mgp_softmax_bwd_f32
//     dU_i    = sum_{e=(i,j)} ds_e v_j - sum_{e=(j,i)} ds_e v_j           dV_i = -sum_{e=(i,j)} ds_e u_j + sum_{e=(j,i)} ds_e u_j
//
// One launch each, one wave per row, MC_WAVES rows per workgroup.  A dense (R, R) score matrix is never formed: at the flagship shape
// (R = 50 176) it would be 10 GB, the pattern has 4 x 10^5 entries.
//
//   score      lane l holds the 16-byte pieces l, l + 64, ... of the row's own u_i and v_i in a lane-private strip of LDS (read from memory once
//              per row, not once per entry; no lane reads what another wrote, so no barrier), then walks the row's entries: two fp32
//              accumulator sets per lane, acc1 = sum u_i v_j and acc2 = sum v_i u_j, formed by the SAME chain of fmaf calls and reduced over the
//              wave in the same order (in float64 from the wave up).  Two nodes with identical rows (real incident windows are full of all-zero rows) and a diagonal entry
//              therefore score exactly 0.0 -- a product commutes bit for bit -- and relu's mask, which is decided at 0, does not hang on rounding.
//   softmax    lanes stride over the row's entries (rows of 0, 1 or more than 64 entries alike); relu and max as torch has them (NaN stays NaN)
//   score bwd  gathered per destination row over both orientations of the pattern (CSR of Gs for the first sums, CSR of Gs^T plus the map
//              from its entries to those of Gs for the second): every dU / dV element is written once by one lane in one fixed order --
//              no float atomics, bitwise reproducible.
#include "stc_common.h"

namespace {

using v4f = __attribute__((ext_vector_type(4))) float;
constexpr int MC_WAVES = 4, MC_THREADS = MC_WAVES * stc::kWave;
static_assert((size_t)MC_WAVES * 2 * STC_MGP_CSR_MAX_KH * sizeof(float) <= stc::kMaxLdsBytes, "the rows' own u, v strips fit the LDS");

// as in stc_mgp_front.hip: a NaN operand comes out as NaN
__device__ __forceinline__ float mc_relu(float d) { return d <= 0.f ? 0.f : d; }
__device__ __forceinline__ float mc_max(float a, float b) { return (a != a || a > b) ? a : b; }

__global__ __launch_bounds__(MC_THREADS) void mgp_csr_score_kernel(const float* __restrict__ U, const float* __restrict__ V, const int* __restrict__ rowptr,
                                                                   const int* __restrict__ colidx, float* __restrict__ score, int R, int KH) {
    extern __shared__ v4f mc_own[];                                   // [wave][u | v][KH / 4]
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, row = blockIdx.x * MC_WAVES + wave, P4 = KH >> 2;
    if (row >= R) return;
    const int e0 = rowptr[row], e1 = rowptr[row + 1];
    if (e0 >= e1) return;
    v4f* ou = mc_own + (size_t)wave * 2 * P4;
    v4f* ov = ou + P4;
    const v4f* ui = reinterpret_cast<const v4f*>(U + (size_t)row * KH);
    const v4f* vi = reinterpret_cast<const v4f*>(V + (size_t)row * KH);
    for (int p = lane; p < P4; p += 64) {
        ou[p] = ui[p];
        ov[p] = vi[p];
    }
    for (int e = e0; e < e1; ++e) {
        const int col = colidx[e];
        const v4f* uj = reinterpret_cast<const v4f*>(U + (size_t)col * KH);
        const v4f* vj = reinterpret_cast<const v4f*>(V + (size_t)col * KH);
        v4f a1 = {0.f, 0.f, 0.f, 0.f}, a2 = {0.f, 0.f, 0.f, 0.f};
        for (int p = lane; p < P4; p += 64) {
            const v4f u = ou[p], v = ov[p], x = vj[p], y = uj[p];
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                a1[c] = fmaf(u[c], x[c], a1[c]);                      // u_i v_j
                a2[c] = fmaf(v[c], y[c], a2[c]);                      // v_i u_j: the same chain on the other pair
            }
        }
        // fp32 per lane, float64 from the wave up (as stc_loss.hip, stc_mixed_fusion_lr.hip): the two sums are tens of times the score they leave
        const double s1 = stc_wave_sum(((double)a1[0] + (double)a1[1]) + ((double)a1[2] + (double)a1[3]));
        const double s2 = stc_wave_sum(((double)a2[0] + (double)a2[1]) + ((double)a2[2] + (double)a2[3]));
        if (lane == 0) score[e] = (float)(s1 - s2);
    }
}

__global__ __launch_bounds__(MC_THREADS) void mgp_csr_softmax_fwd_kernel(const float* __restrict__ score, const int* __restrict__ rowptr, float* __restrict__ Ps, int R) {
    const int lane = threadIdx.x & 63, row = blockIdx.x * MC_WAVES + (threadIdx.x >> 6);
    if (row >= R) return;
    const int e0 = rowptr[row], e1 = rowptr[row + 1];
    if (e0 >= e1) return;
    float mx = 0.f;                                                   // relu: every entry >= 0
    for (int e = e0 + lane; e < e1; e += 64) mx = mc_max(mx, score[e]);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) mx = mc_max(mx, __shfl_xor(mx, off, 64));
    float sum = 0.f;
    for (int e = e0 + lane; e < e1; e += 64) sum += expf(mc_relu(score[e]) - mx);
    sum = stc_wave_sum(sum);
    const float inv = 1.f / sum;
    for (int e = e0 + lane; e < e1; e += 64) Ps[e] = expf(mc_relu(score[e]) - mx) * inv;
}

__global__ __launch_bounds__(MC_THREADS) void mgp_csr_softmax_bwd_kernel(const float* __restrict__ score, const float* __restrict__ Ps, const float* __restrict__ dPs,
                                                                         const int* __restrict__ rowptr, float* __restrict__ ds, int R) {
    const int lane = threadIdx.x & 63, row = blockIdx.x * MC_WAVES + (threadIdx.x >> 6);
    if (row >= R) return;
    const int e0 = rowptr[row], e1 = rowptr[row + 1];
    if (e0 >= e1) return;
    float dot = 0.f;
    for (int e = e0 + lane; e < e1; e += 64) dot = fmaf(dPs[e], Ps[e], dot);
    dot = stc_wave_sum(dot);
    for (int e = e0 + lane; e < e1; e += 64) ds[e] = !(score[e] <= 0.f) ? Ps[e] * (dPs[e] - dot) : 0.f;
}

// row i of dU, dV: the entries (i, j) of Gs (rowptr / colidx, ds in place), then the entries (j, i) (t_rowptr / t_colidx = CSR of Gs^T, whose
// entry f is entry t_entry[f] of Gs)
__global__ __launch_bounds__(MC_THREADS) void mgp_csr_score_bwd_kernel(const float* __restrict__ U, const float* __restrict__ V, const float* __restrict__ ds,
                                                                       const int* __restrict__ rowptr, const int* __restrict__ colidx,
                                                                       const int* __restrict__ t_rowptr, const int* __restrict__ t_colidx,
                                                                       const int* __restrict__ t_entry, float* __restrict__ dU, float* __restrict__ dV, int R, int KH) {
    const int lane = threadIdx.x & 63, row = blockIdx.x * MC_WAVES + (threadIdx.x >> 6), P4 = KH >> 2;
    if (row >= R) return;
    const int e0 = rowptr[row], e1 = rowptr[row + 1], f0 = t_rowptr[row], f1 = t_rowptr[row + 1];
    v4f* du = reinterpret_cast<v4f*>(dU + (size_t)row * KH);
    v4f* dv = reinterpret_cast<v4f*>(dV + (size_t)row * KH);
    for (int p = lane; p < P4; p += 64) {
        v4f au = {0.f, 0.f, 0.f, 0.f}, av = {0.f, 0.f, 0.f, 0.f};
        for (int e = e0; e < e1; ++e) {
            const float d = ds[e];
            const size_t at = (size_t)colidx[e] * KH;
            const v4f vj = reinterpret_cast<const v4f*>(V + at)[p], uj = reinterpret_cast<const v4f*>(U + at)[p];
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                au[c] = fmaf(d, vj[c], au[c]);
                av[c] = fmaf(-d, uj[c], av[c]);
            }
        }
        for (int f = f0; f < f1; ++f) {
            const float d = ds[t_entry[f]];
            const size_t at = (size_t)t_colidx[f] * KH;
            const v4f vj = reinterpret_cast<const v4f*>(V + at)[p], uj = reinterpret_cast<const v4f*>(U + at)[p];
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                au[c] = fmaf(-d, vj[c], au[c]);
                av[c] = fmaf(d, uj[c], av[c]);
            }
        }
        du[p] = au;
        dv[p] = av;
    }
}

// Sizes every entry point shares.  Offsets are formed in 64 bits, but rows, entries and the elements of U / V are counted in int32 on both
// sides of the ABI: R, nnz and R KH must stay below 2^31 (R KH is 1.2 x 10^8 at the flagship shape: 50 176 rows of 2 304 floats).
int mc_sizes(const char* who, int32_t R, int32_t KH, int32_t nnz, bool rows) {
    STC_REQUIRE(R >= 0 && nnz >= 0 && KH >= 0, STC_EINVAL, "%s: negative size (R=%d KH=%d nnz=%d)", who, R, KH, nnz);
    if (!rows) return STC_OK;
    STC_REQUIRE(KH >= 4 && KH % 4 == 0 && KH <= STC_MGP_CSR_MAX_KH, STC_EUNSUPPORTED, "%s: KH = %d must be a multiple of 4 in [4, %d] (16-byte pieces; use torch operations)",
                who, KH, STC_MGP_CSR_MAX_KH);
    STC_REQUIRE((long long)R * KH < (1ll << 31), STC_ELIMIT, "%s: R KH = %lld must be below 2^31", who, (long long)R * KH);
    return STC_OK;
}

inline dim3 mc_grid(int32_t R) { return dim3((unsigned)(((long long)R + MC_WAVES - 1) / MC_WAVES)); }

stc::Grants mc_score_grants;

}  // namespace

extern "C" int stc_mgp_csr_supported(int32_t R, int32_t KH, int32_t nnz) {
    return R >= 1 && nnz >= 0 && KH >= 4 && KH % 4 == 0 && KH <= STC_MGP_CSR_MAX_KH && (long long)R * KH < (1ll << 31);
}

extern "C" int stc_mgp_csr_score_f32(const float* U, const float* V, const int32_t* rowptr, const int32_t* colidx, float* score, int32_t R, int32_t KH,
                                     int32_t nnz, void* stream) {
    if (int rc = mc_sizes("stc_mgp_csr_score_f32", R, KH, nnz, true)) return rc;
    if (R == 0 || nnz == 0) return STC_OK;
    STC_REQUIRE(U && V && rowptr && colidx && score, STC_EINVAL, "stc_mgp_csr_score_f32: null pointer");
    STC_REQUIRE(stc::aligned16(U) && stc::aligned16(V), STC_EALIGN, "stc_mgp_csr_score_f32: U and V must be 16-byte aligned");
    STC_REQUIRE(stc::aligned(rowptr, 4) && stc::aligned(colidx, 4) && stc::aligned(score, 4), STC_EALIGN, "stc_mgp_csr_score_f32: rowptr, colidx and score must be 4-byte aligned");
    STC_REQUIRE(score != U && score != V, STC_EINVAL, "stc_mgp_csr_score_f32: score must not alias U or V");
    const size_t lds = (size_t)MC_WAVES * 2 * KH * sizeof(float);
    if (int rc = stc::hip_status(stc::allow_lds_once(mgp_csr_score_kernel, lds, mc_score_grants), "stc_mgp_csr_score_f32 (LDS size)")) return rc;
    hipLaunchKernelGGL(mgp_csr_score_kernel, mc_grid(R), dim3(MC_THREADS), lds, static_cast<hipStream_t>(stream), U, V, rowptr, colidx, score, (int)R, (int)KH);
    STC_LAUNCH_CHECK("stc_mgp_csr_score_f32 launch");
    return STC_OK;
}

extern "C" int stc_mgp_csr_softmax_fwd_f32(const float* score, const int32_t* rowptr, float* Ps, int32_t R, int32_t nnz, void* stream) {
    if (int rc = mc_sizes("stc_mgp_csr_softmax_fwd_f32", R, 0, nnz, false)) return rc;
    if (R == 0 || nnz == 0) return STC_OK;
    STC_REQUIRE(score && rowptr && Ps, STC_EINVAL, "stc_mgp_csr_softmax_fwd_f32: null pointer");
    STC_REQUIRE(stc::aligned(score, 4) && stc::aligned(rowptr, 4) && stc::aligned(Ps, 4), STC_EALIGN, "stc_mgp_csr_softmax_fwd_f32: operands must be 4-byte aligned");
    STC_REQUIRE(Ps != score, STC_EINVAL, "stc_mgp_csr_softmax_fwd_f32: Ps must not alias score (a row is read three times)");
    hipLaunchKernelGGL(mgp_csr_softmax_fwd_kernel, mc_grid(R), dim3(MC_THREADS), 0, static_cast<hipStream_t>(stream), score, rowptr, Ps, (int)R);
    STC_LAUNCH_CHECK("stc_mgp_csr_softmax_fwd_f32 launch");
    return STC_OK;
}

extern "C" int stc_mgp_csr_softmax_bwd_f32(const float* score, const float* Ps, const float* dPs, const int32_t* rowptr, float* ds, int32_t R, int32_t nnz,
                                           void* stream) {
    if (int rc = mc_sizes("stc_mgp_csr_softmax_bwd_f32", R, 0, nnz, false)) return rc;
    if (R == 0 || nnz == 0) return STC_OK;
    STC_REQUIRE(score && Ps && dPs && rowptr && ds, STC_EINVAL, "stc_mgp_csr_softmax_bwd_f32: null pointer");
    STC_REQUIRE(stc::aligned(score, 4) && stc::aligned(Ps, 4) && stc::aligned(dPs, 4) && stc::aligned(rowptr, 4) && stc::aligned(ds, 4), STC_EALIGN,
                "stc_mgp_csr_softmax_bwd_f32: operands must be 4-byte aligned");
    STC_REQUIRE(ds != score && ds != Ps && ds != dPs, STC_EINVAL, "stc_mgp_csr_softmax_bwd_f32: ds must not alias an input");
    hipLaunchKernelGGL(mgp_csr_softmax_bwd_kernel, mc_grid(R), dim3(MC_THREADS), 0, static_cast<hipStream_t>(stream), score, Ps, dPs, rowptr, ds, (int)R);
    STC_LAUNCH_CHECK("stc_mgp_csr_softmax_bwd_f32 launch");
    return STC_OK;
}

extern "C" int stc_mgp_csr_score_bwd_f32(const float* U, const float* V, const float* ds, const int32_t* rowptr, const int32_t* colidx, const int32_t* t_rowptr,
                                         const int32_t* t_colidx, const int32_t* t_entry, float* dU, float* dV, int32_t R, int32_t KH, int32_t nnz, void* stream) {
    if (int rc = mc_sizes("stc_mgp_csr_score_bwd_f32", R, KH, nnz, true)) return rc;
    if (R == 0) return STC_OK;
    STC_REQUIRE(U && V && rowptr && t_rowptr && dU && dV && (nnz == 0 || (ds && colidx && t_colidx && t_entry)), STC_EINVAL, "stc_mgp_csr_score_bwd_f32: null pointer");
    STC_REQUIRE(stc::aligned16(U) && stc::aligned16(V) && stc::aligned16(dU) && stc::aligned16(dV), STC_EALIGN,
                "stc_mgp_csr_score_bwd_f32: U, V, dU and dV must be 16-byte aligned");
    STC_REQUIRE(stc::aligned(ds, 4) && stc::aligned(rowptr, 4) && stc::aligned(colidx, 4) && stc::aligned(t_rowptr, 4) && stc::aligned(t_colidx, 4) && stc::aligned(t_entry, 4),
                STC_EALIGN, "stc_mgp_csr_score_bwd_f32: ds and the index arrays must be 4-byte aligned");
    STC_REQUIRE(dU != dV && dU != U && dU != V && dV != U && dV != V && (const float*)dU != ds && (const float*)dV != ds, STC_EINVAL,
                "stc_mgp_csr_score_bwd_f32: dU and dV must not alias an input or each other (every row gathers its neighbours' rows)");
    hipLaunchKernelGGL(mgp_csr_score_bwd_kernel, mc_grid(R), dim3(MC_THREADS), 0, static_cast<hipStream_t>(stream), U, V, ds, rowptr, colidx, t_rowptr, t_colidx,
                       t_entry, dU, dV, (int)R, (int)KH);
    STC_LAUNCH_CHECK("stc_mgp_csr_score_bwd_f32 launch");
    return STC_OK;
}
