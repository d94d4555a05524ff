// Internal: the host-side blocks that the node / cell C entry points (stc_node.hip on fp32 rows and planes, stc_node_bf16.hip on bf16 planes)
// and the launch helpers of their kernels (stc_node_mfma.hip, stc_node_x3.hip, stc_cell_bwd_x3.hip, stc_node_bf16.hip) share.  Where the two
// fronts answer one fault with different status codes, the code is an argument of the helper: the difference shows at the call site.
#pragma once
#include <climits>

#include "stc_common.h"
#include "stc_node_mfma.h"

namespace stc {

// ---- planar cell rows [X | H]: the state plane is h columns wide; the input plane is h columns too (rows of two whole planes), or 1..4 columns
// (a model's first layer), which the fp32 kernels and every workspace take as padded rows of 20 columns
struct PlanarRow {
    int L, cin, h;      // row width the fp32 kernels and the workspace are sized for; columns of the input plane; hidden width
    bool narrow;
    PlanarRow(int Lw, int h_) : L(Lw == 2 * h_ ? 2 * h_ : 20), cin(Lw - h_), h(h_), narrow(Lw != 2 * h_) {}
    // code: STC_EINVAL on the fp32 front, STC_EUNSUPPORTED on the bf16 one
    int check_width(const char* who, int code) const {
        STC_REQUIRE(cin == h || (cin >= 1 && cin <= 4), code, "%s: input width %d (Lw - h) must be h or 1..4", who, cin);
        return STC_OK;
    }
};

inline int check_operand_format(const char* who, int fmt) {
    STC_REQUIRE(fmt == STC_FMT_BF16X3 || fmt == STC_FMT_F16X2, STC_EINVAL, "%s: operand_format %d (STC_FMT_BF16X3 or STC_FMT_F16X2)", who, fmt);
    return STC_OK;
}

// ---- the end of a dispatch ladder: no kernel took the operands
inline int dispatched(const char* who, int rc, const char* why = "alignment") {
    return rc == STC_NOT_HANDLED ? fail(STC_EUNSUPPORTED, "%s: operands not usable (%s)", who, why) : rc;
}

// ---- the parameter-gradient tail of a backward entry point.  The kernels leave per-workgroup partial rows [dW (nW) | db (Ho)] in the caller's
// workspace; one (dW, db) pair per convolution, two for the one-launch cell backward, each with its share of the workspace.
struct ParamGrad {
    float* dW; float* db;       // db may be null
    int nW, Ho;
    size_t bytes;               // this pair's share: stc_bdg_node_bwd_workspace_bytes(...)
    float* partial;             // set by grad_tail_begin
};

// Before the dispatch.  nodes == 0: the gradients of an empty batch are zero -- fills them and sets *done.  Otherwise checks the workspace and
// points every pair at its share.  align_code: what a null or misaligned workspace returns (STC_EALIGN on the fp32 front and the bf16 node
// kernel, STC_EINVAL on the bf16 planar front); a short one is STC_EINVAL everywhere.
inline int grad_tail_begin(const char* who, ParamGrad* g, int n, long long nodes, void* workspace, size_t workspace_bytes, int align_code,
                           hipStream_t s, bool* done) {
    *done = nodes == 0;
    if (*done) {
        for (int i = 0; i < n; ++i) {
            if (int rc = hip_status(hipMemsetAsync(g[i].dW, 0, (size_t)g[i].nW * sizeof(float), s), "memset dW")) return rc;
            if (g[i].db) if (int rc = hip_status(hipMemsetAsync(g[i].db, 0, (size_t)g[i].Ho * sizeof(float), s), "memset db")) return rc;
        }
        return STC_OK;
    }
    size_t need = 0;
    for (int i = 0; i < n; ++i) need += g[i].bytes;
    STC_REQUIRE(workspace && aligned16(workspace), align_code, "%s: workspace (%zu B) null or not 16-byte aligned", who, workspace_bytes);
    STC_REQUIRE(workspace_bytes >= need, STC_EINVAL, "%s: workspace of %zu B is too small (%zu B needed)", who, workspace_bytes, need);
    unsigned char* share = static_cast<unsigned char*>(workspace);
    for (int i = 0; i < n; ++i) {
        g[i].partial = reinterpret_cast<float*>(share);
        share += g[i].bytes;
    }
    return STC_OK;
}

// After the dispatch: the fixed-order sum of the n_parts partial rows of every pair.
inline int grad_tail_reduce(const ParamGrad* g, int n, int n_parts, hipStream_t s) {
    for (int i = 0; i < n; ++i)
        if (int rc = stc_node_reduce_partials(g[i].partial, n_parts, g[i].nW, g[i].Ho, g[i].dW, g[i].db, s)) return rc;
    return STC_OK;
}

// ---- grid of a persistent kernel: raises its dynamic-LDS cap, then min(workgroups resident at once, one workgroup per `waves` nodes, cap).
// The occupancy query runs once per kernel instantiation per process (the static of this instantiation): the few-category path is launch-bound.
// cap: MF_BWD_MAX_GRID for the backward forms (the partial rows the workspace holds), INT_MAX for the forward ones.
template <auto Kern>
int persistent_grid(const char* what, int threads, size_t lds, int fallback_per_cu, long long nodes, int waves, int cap, int* grid) {
    if (int rc = hip_status(allow_lds(Kern, lds), what)) return rc;
    static const int resident = resident_blocks(Kern, threads, lds, fallback_per_cu);
    const long long want = (nodes + waves - 1) / waves;
    *grid = resident < cap ? resident : cap;
    if (want < *grid) *grid = (int)want;
    return STC_OK;
}

}  // namespace stc
