// Internal: the host-side blocks that the C entry points of the spatial aggregation share (stc_spmm.hip and stc_spmm_bf16.hip: the CSR / row-blocked
// kernels of stc_spmm_gather.h on fp32 and bf16 rows; stc_spmm_patch.hip; stc_spmm_ring2.hip; stc_dense.hip).  Where fronts differ -- an element size, a divisibility
// rule, a status code, which pointers must be given -- the difference is an argument: it shows at the call site.  Plain checks on the
// arguments, no allocation: a launch-bound step makes several hundred of these calls.
#pragma once
#include "stc_common.h"

namespace stc {

struct GraphArgs {      // either form of the same matrix; BCSR is used when blk_ptr is given
    const int32_t *rowptr, *colidx; const float* val;
    const int32_t *blk_ptr, *blk_cols; const float* blk_vals;
};

// batch is grid.y
inline int check_batch(const char* who, int batch) {
    STC_REQUIRE(batch <= 65535, STC_ELIMIT, "%s: batch %d > 65535 (grid.y)", who, batch);
    return STC_OK;
}

// ---- the plain product  Y = alpha S.X + beta Y0  on rows of F elements
struct Plain {
    int n_rows, n_cols, batch, F;
    const void *X, *Y0, *Y;
    float beta;
    bool empty() const { return n_rows == 0 || batch == 0 || F == 0; }      // nothing to produce: STC_OK without a launch
};

// given: every pointer this front cannot do without (its graph arrays, X, Y; n_cols > 0 where it asks for that).
// piece: elements of a 16-byte piece -- X / Y0 / Y must be 16-byte aligned and F a multiple of `multiple` (a piece, or the 64 pieces of a 1 KiB
// chunk), else multiple_code; piece 0: a front whose kernel takes any F at any alignment.
inline int check_plain(const char* who, const Plain& p, bool given, int piece, int multiple, int multiple_code) {
    STC_REQUIRE(p.n_rows >= 0 && p.n_cols >= 0 && p.batch >= 0 && p.F >= 0, STC_EINVAL, "%s: negative size (n_rows=%d n_cols=%d batch=%d F=%d)", who,
                p.n_rows, p.n_cols, p.batch, p.F);
    if (p.empty()) return STC_OK;
    STC_REQUIRE(given, STC_EINVAL, "%s: null graph array / X / Y (or n_cols == 0 with rows to produce)", who);
    STC_REQUIRE(p.beta == 0.f || p.Y0, STC_EINVAL, "%s: beta != 0 needs Y0", who);
    STC_REQUIRE(p.X != p.Y, STC_EINVAL, "%s: X must not alias Y", who);
    if (piece == 0) return STC_OK;
    STC_REQUIRE(p.F % multiple == 0, multiple_code, "%s: F=%d must be a positive multiple of %d (rows in whole %s)", who, p.F, multiple,
                multiple == piece ? "16-byte pieces" : "1 KiB chunks");
    STC_REQUIRE(aligned16(p.X) && aligned16(p.Y) && (!p.Y0 || aligned16(p.Y0)), STC_EALIGN, "%s: X / Y / Y0 must be 16-byte aligned", who);
    return STC_OK;
}

// ---- state rows: (batch, n_rows) rows of C state vectors of h = 16 floats (the blend and sum epilogues, the two-ring launches).
// graph: one of the two graph forms is given (looked at only when there are rows to produce)
inline int check_state_rows(const char* who, int n_rows, int batch, int C, int h, bool graph) {
    STC_REQUIRE(h == 16, STC_EUNSUPPORTED, "%s: hidden width %d (built for 16)", who, h);
    STC_REQUIRE(n_rows >= 0 && batch >= 0 && C >= 1, STC_EINVAL, "%s: bad sizes", who);
    if (int rc = check_batch(who, batch)) return rc;
    STC_REQUIRE(n_rows == 0 || batch == 0 || graph, STC_EINVAL, "%s: neither graph form given", who);
    return STC_OK;
}

// ---- addend planes.  The count first (before anything is copied into a kernel's fixed arrays); limit_code: STC_EINVAL on stc_spmm_sum_*,
// STC_ELIMIT on stc_ring2_*.  what: "addend", "first-ring addend", ...
inline int check_addend_count(const char* who, const char* what, int n, int lo, int hi, int limit_code) {
    STC_REQUIRE(n >= lo && n <= hi, limit_code, "%s: %d..%d %ss, got %d", who, lo, hi, what, n);
    return STC_OK;
}

// ... then the list: every addend non-null, 16-byte aligned, and none of the launch's results r0 / r1 (r1 may be null)
template <class T>
inline int check_addends(const char* who, const char* what, const T* const* add, int n, const void* r0, const void* r1) {
    for (int i = 0; i < n; ++i)
        STC_REQUIRE(add[i] && aligned16(add[i]) && add[i] != r0 && (!r1 || add[i] != r1), STC_EINVAL, "%s: %s %d null, misaligned or aliasing a result", who, what, i);
    return STC_OK;
}

// ---- the optional blend backward of a sum: dY = Y U (1 - Cand^2) needs both gate planes
inline int check_dy(const char* who, const void* dY, const void* U, const void* Cand, const void* Y) {
    STC_REQUIRE(!dY || (U && Cand && aligned16(U) && aligned16(Cand) && aligned16(dY) && dY != Y), STC_EINVAL,
                "%s: dY needs U and Cand (16-byte aligned, not aliasing Y)", who);
    return STC_OK;
}

}  // namespace stc
