// bf16-storage CSR / row-blocked CSR SpMM for the spatial (1-mode) aggregation of STC-GNN on gfx950.
//
//   Y[b,i,:] = bf16( alpha * sum_j val[j] * X[b, col[j], :] + beta * Y0[b,i,:] )        X, Y0, Y: bf16; val, sums: fp32
//
// Same product as stc_spmm.hip (reference STC_GNN.py:37 and, with (alpha, beta) = (2, -1), the feature-side Chebyshev
// step of STC_GNN.py:28) for BASELINE.json's bf16 configuration (N = 50 176, C = 64): feature rows are stored in
// bf16, every product and the whole row sum are fp32 (a bf16 value widens to fp32 exactly: 16-bit shift), and the
// result is rounded to bf16 once (round to nearest even, v_cvt_pk_bf16_f32).  The reference has no bf16 behaviour
// (its identity matrix is fp32-only); the contract here is "the fp32 kernel on the same bf16-valued inputs,
// rounded once", which the parity tests check to one bf16 ulp.
//
// The kernels are the gather kernels of stc_spmm_gather.h (skeleton described there) with the bf16 format below: each lane streams 16-byte
// pieces of 8 bf16 (1 KiB per wave instruction), output / Y0 / addend pieces are non-temporal.  HBM-bound: a node row of C*L = 2048 bf16 is the
// same 4 KiB as the fp32 row of the C = 32 configuration.
#include "stc_spmm_gather.h"

namespace {

struct Epi {
    const Raw* Y0;                   // PLAIN: optional base term (scaled by beta); BLEND: A (bias included)
    Raw* Y;                          // PLAIN / SUM output
    float alpha, beta;               // PLAIN
    // BLEND (forward of the candidate convolution in post-aggregation form, STC_GNN.py:76-78): rows are state rows,
    // Cand = tanh(A + S.Bm), Hnew = (1-U)*H + U*Cand
    const Raw *U, *H;
    Raw *Cand, *Hnew;
    // SUM / SUM2 (gradient of a state from its consumers' pieces): Y = sum_i add[i] + S.(X [+ X2]); optional
    // dY = Y * U * (1 - Cand^2), the blend backward of the cell that owns the state (U, gCand: that cell's saved gates)
    const Raw* X2;
    const Raw* add[5]; int n_add;
    const Raw* gCand; Raw* dY;
};
static_assert(sizeof(Epi::add) / sizeof(const Raw*) == STC_SPMM_SUM_BF16_MAX_ADD, "the addend slots of the kernel argument are the ABI's limit");

// bf16 rows on the gather kernels (stc_spmm_gather.h names the members): whole-plane operands, piece o = rowg * F8 + ch of every plane
struct RowsBf16 {
    using Acc = Piece<true>;
    using Epi = ::Epi;
    static constexpr int MAX_VPT = 2;
    static constexpr bool ONE_WAVE_BLOCKS = true, PIPELINED = false, BLEND_AHEAD_WAVE_ROW = true;

    template <bool TWO>
    struct Operand { Raw x[TWO ? 2 : 1]; };      // X and X2 side by side: each product is rounded into the sum on its own, two fmas
    template <bool TWO>
    static __device__ __forceinline__ Operand<TWO> gather(const Raw* X, const Raw* X2, size_t at) {
        Operand<TWO> o;
        o.x[0] = X[at];
        if (TWO) o.x[TWO ? 1 : 0] = X2[at];
        return o;
    }
    template <bool TWO>
    static __device__ __forceinline__ void accumulate(Acc& acc, float s, const Operand<TWO>& o) {
        acc.fma(s, o.x[0]);
        if (TWO) acc.fma(s, o.x[TWO ? 1 : 0]);
    }

    static __device__ __forceinline__ BlendIn blend_operands(const Epi& ep, size_t o) {
        return BlendIn{stc_ld_once(ep.Y0 + o), stc_ld_once(ep.U + o), stc_ld_once(ep.H + o)};
    }
    template <bool ROW_BLOCK>
    static __device__ __forceinline__ void blend(const Epi& ep, size_t rowg, int F8, int ch, const Acc& acc, const BlendIn& in) {
        const size_t o = rowg * F8 + ch;
        float a[8], u[8], h[8], c[8], hn[8];
        unpack8(in.a, a); unpack8(in.u, u); unpack8(in.h, h);
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            c[i] = tanh_fast(acc.v[i] + a[i]);
            hn[i] = (1.f - u[i]) * h[i] + u[i] * c[i];
        }
        stc_st_once(ep.Cand + o, pack8_raw(c));
        stc_st_once(ep.Hnew + o, pack8_raw(hn));
    }

    template <int MODE>      // EP_PLAIN, EP_SUM, EP_SUM2
    static __device__ __forceinline__ void finish(const Epi& ep, size_t rowg, int F8, int ch, const Acc& acc, float&) {
        const size_t o = rowg * F8 + ch;
        float r[8];
        if (MODE == EP_PLAIN) {
#pragma unroll
            for (int i = 0; i < 8; ++i) r[i] = ep.alpha * acc.v[i];
            if (ep.beta != 0.f) {
                float y0[8];
                unpack8(stc_ld_once(ep.Y0 + o), y0);
#pragma unroll
                for (int i = 0; i < 8; ++i) r[i] = fmaf(ep.beta, y0[i], r[i]);
            }
            stc_st_once(ep.Y + o, pack8_raw(r));
            return;
        }
#pragma unroll
        for (int i = 0; i < 8; ++i) r[i] = acc.v[i];
        for (int k = 0; k < ep.n_add; ++k) {
            float t[8];
            unpack8(stc_ld_once(ep.add[k] + o), t);
#pragma unroll
            for (int i = 0; i < 8; ++i) r[i] += t[i];
        }
        stc_st_once(ep.Y + o, pack8_raw(r));
        if (ep.dY) {
            float u[8], c[8];
            unpack8(stc_ld_once(ep.U + o), u); unpack8(stc_ld_once(ep.gCand + o), c);
#pragma unroll
            for (int i = 0; i < 8; ++i) r[i] = r[i] * u[i] * (1.f - c[i] * c[i]);
            stc_st_once(ep.dY + o, pack8_raw(r));
        }
    }
    template <int MODE>
    static __device__ __forceinline__ void wave_done(const Epi&, float) {}      // nothing is reduced over a launch
};

// the plain product on bf16 rows (16-byte pieces of 8 elements) on either graph form; its pointer array is checked last
int plain_bf16(const char* who, const char* launch_who, const GraphArgs& g, const stc::Plain& p, float alpha, void* Y, void* stream) {
    if (int rc = stc::check_plain(who, p, p.X && p.Y && p.n_cols > 0, 8, 8, STC_EINVAL)) return rc;
    if (p.empty()) return STC_OK;
    if (int rc = stc::check_batch(who, p.batch)) return rc;
    STC_REQUIRE(g.rowptr || g.blk_ptr, STC_EINVAL, "%s: null rowptr / blk_ptr", who);      // colidx / val may be null for a graph without edges
    Epi ep{};
    ep.Y0 = reinterpret_cast<const Raw*>(p.Y0); ep.Y = reinterpret_cast<Raw*>(Y); ep.alpha = alpha; ep.beta = p.beta;
    return launch_gather<EP_PLAIN, RowsBf16>(launch_who, g, p.n_rows, p.n_cols, p.X, p.batch, p.F / 8, ep, static_cast<hipStream_t>(stream));
}

}  // namespace

extern "C" int stc_csr_spmm_bf16(const int32_t* rowptr, const int32_t* colidx, const float* val,
                                 int32_t n_rows, int32_t n_cols,
                                 const void* X, const void* Y0, void* Y,
                                 int32_t batch, int32_t F, float alpha, float beta, void* stream) {
    return plain_bf16("stc_csr_spmm_bf16", "stc_csr_spmm_bf16 launch", GraphArgs{rowptr, colidx, val, nullptr, nullptr, nullptr},
                      stc::Plain{n_rows, n_cols, batch, F, X, Y0, Y, beta}, alpha, Y, stream);
}

extern "C" int stc_bcsr_spmm_bf16(const int32_t* blk_ptr, const int32_t* blk_cols, const float* blk_vals,
                                  int32_t n_rows, int32_t n_cols,
                                  const void* X, const void* Y0, void* Y,
                                  int32_t batch, int32_t F, float alpha, float beta, void* stream) {
    return plain_bf16("stc_bcsr_spmm_bf16", "stc_bcsr_spmm_bf16 launch", GraphArgs{nullptr, nullptr, nullptr, blk_ptr, blk_cols, blk_vals},
                      stc::Plain{n_rows, n_cols, batch, F, X, Y0, Y, beta}, alpha, Y, stream);
}

extern "C" int stc_spmm_blend_fwd_bf16(const int32_t* rowptr, const int32_t* colidx, const float* val,
                                       const int32_t* blk_ptr, const int32_t* blk_cols, const float* blk_vals,
                                       int32_t n_rows, int32_t n_cols, const void* Bm, const void* A,
                                       const void* U, const void* H, void* Cand, void* Hnew,
                                       int32_t batch, int32_t C, int32_t h, void* stream) {
    const GraphArgs g{rowptr, colidx, val, blk_ptr, blk_cols, blk_vals};
    if (int rc = stc::check_state_rows("stc_spmm_blend_fwd_bf16", n_rows, batch, C, h, g.blk_ptr || g.rowptr)) return rc;
    if (n_rows == 0 || batch == 0) return STC_OK;
    STC_REQUIRE(Bm && A && U && H && Cand && Hnew && n_cols > 0, STC_EINVAL, "stc_spmm_blend_fwd_bf16: null pointer");
    STC_REQUIRE(stc::aligned16(Bm) && stc::aligned16(A) && stc::aligned16(U) && stc::aligned16(H) && stc::aligned16(Cand) && stc::aligned16(Hnew),
                STC_EALIGN, "stc_spmm_blend_fwd_bf16: operands must be 16-byte aligned");
    STC_REQUIRE(Bm != Cand && Bm != Hnew, STC_EINVAL, "stc_spmm_blend_fwd_bf16: outputs must not alias Bm (its rows are gathered by other rows)");
    Epi ep{};
    ep.Y0 = reinterpret_cast<const Raw*>(A);
    ep.U = reinterpret_cast<const Raw*>(U); ep.H = reinterpret_cast<const Raw*>(H);
    ep.Cand = reinterpret_cast<Raw*>(Cand); ep.Hnew = reinterpret_cast<Raw*>(Hnew);
    return launch_gather<EP_BLEND, RowsBf16>("stc_spmm_blend_fwd_bf16 launch", g, n_rows, n_cols, Bm, batch, C * h / 8, ep, static_cast<hipStream_t>(stream));
}

extern "C" int stc_spmm_sum_bf16(const int32_t* rowptr, const int32_t* colidx, const float* val,
                                 const int32_t* blk_ptr, const int32_t* blk_cols, const float* blk_vals,
                                 int32_t n_rows, int32_t n_cols, const void* X, const void* X2,
                                 int32_t n_add, const void* const* add,
                                 void* Y, const void* U, const void* Cand, void* dY,
                                 int32_t batch, int32_t C, int32_t h, void* stream) {
    const GraphArgs g{rowptr, colidx, val, blk_ptr, blk_cols, blk_vals};
    if (int rc = stc::check_state_rows("stc_spmm_sum_bf16", n_rows, batch, C, h, g.blk_ptr || g.rowptr)) return rc;
    if (int rc = stc::check_addend_count("stc_spmm_sum_bf16", "addend", n_add, 0, STC_SPMM_SUM_BF16_MAX_ADD, STC_EINVAL)) return rc;
    STC_REQUIRE(n_add == 0 || add, STC_EINVAL, "stc_spmm_sum_bf16: null list of addends");
    if (n_rows == 0 || batch == 0) return STC_OK;
    STC_REQUIRE(X && Y && n_cols > 0, STC_EINVAL, "stc_spmm_sum_bf16: null pointer");
    STC_REQUIRE(stc::aligned16(X) && stc::aligned16(Y) && (!X2 || stc::aligned16(X2)), STC_EALIGN, "stc_spmm_sum_bf16: operands must be 16-byte aligned");
    STC_REQUIRE(X != Y && X2 != Y, STC_EINVAL, "stc_spmm_sum_bf16: Y must not alias a gathered operand");
    if (int rc = stc::check_dy("stc_spmm_sum_bf16", dY, U, Cand, Y)) return rc;
    if (int rc = stc::check_addends("stc_spmm_sum_bf16", "addend", add, n_add, Y, nullptr)) return rc;
    Epi ep{};
    ep.Y = reinterpret_cast<Raw*>(Y);
    ep.X2 = reinterpret_cast<const Raw*>(X2);
    ep.U = reinterpret_cast<const Raw*>(U); ep.gCand = reinterpret_cast<const Raw*>(Cand); ep.dY = reinterpret_cast<Raw*>(dY);
    ep.n_add = n_add;
    for (int i = 0; i < n_add; ++i) ep.add[i] = reinterpret_cast<const Raw*>(add[i]);
    hipStream_t s = static_cast<hipStream_t>(stream);
    return X2 ? launch_gather<EP_SUM2, RowsBf16>("stc_spmm_sum_bf16 launch", g, n_rows, n_cols, X, batch, C * h / 8, ep, s)
              : launch_gather<EP_SUM, RowsBf16>("stc_spmm_sum_bf16 launch", g, n_rows, n_cols, X, batch, C * h / 8, ep, s);
}
