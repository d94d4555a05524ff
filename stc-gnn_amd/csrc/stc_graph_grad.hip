// Gradients of LEARNED graphs (the reference's MGP_Gen output: dense Gs, and Gc through its Chebyshev stack; STC_GNN.py:185-261 via autograd)
// from what the few-category cell kernels leave behind (stc_cell_small.hip): both are sums over EVERY cell step and sample of a training
// step, of small products whose operands are planes (cells * batch, N, F):
//     stc_graph_grad_f32   out[n][m]   = sum_g sum_f A[g][n][f] B[g][m][f]      dGs^T pieces: A = gradient of an aggregated slab, B = its source slab
//     stc_mix_grad_f32     out[fa][fb] = sum_g sum_n A[g][n][fa] B[g][n][fb]    Q = Z^T . dY, from which dT_c = < W_(ks, c), Q[c, :, d, :] >
// As library GEMMs these cost 2.5 ms of the 8 ms learned SF step (permuted copies of every operand so that the contraction over (g, f) becomes
// one GEMM dimension; a batched product plus a sum is slower still), and dT_c needs more than fp32 over 10^5 cancelling terms (fp32: the SF
// golden's dGc at 1.1e-5).  Here: one workgroup per chunk of g, a wave per few 16 x 16 output tiles, v_mfma_f32_16x16x4_f32 per g (<= 160 terms,
// exact fp32 products, fp32 sums), and the per-g results added into FLOAT64 running sums in registers; every workgroup writes its float64 partial
// (deterministic: no atomics), the caller adds the partials.  `cell0 / cell_step / n_sel`: the cells of one parameter set inside a buffer that holds
// every cell of a width (g = sel * batch + sample -> plane (cell0 + sel * cell_step) * batch + sample).
#include "stc_common.h"

namespace {

using f32x4 = __attribute__((ext_vector_type(4))) float;
#ifndef STC_GG_THREADS                 // (probe builds override these: tools/probes/graph_grad_ab.sh)
#define STC_GG_THREADS 256              // round 6, same-box A/B on the reference's full model at the SF shape (threads, graph tiles per wave, mix tiles per wave,
#define STC_GG_NT_TPW 1                 // steps in flight): (1024, 4, 4, 4) mix 42 us / graph 62 us per launch -> (256, 1, 2, 8) 27 / 48: these launches are
#define STC_GG_TN_TPW 2                 // chains of L2 round trips, and four waves of 80 registers hide each other's better than sixteen of 128
#define STC_GG_TN_STEPS 8
#endif
constexpr int GG_THREADS = STC_GG_THREADS, GG_WAVES = GG_THREADS / 64;
constexpr int GG_NT_TPW = STC_GG_NT_TPW;          // output tiles per wave and tile group (blockIdx.y), graph product
constexpr int GG_TN_TPW = STC_GG_TN_TPW;          // output tiles per wave and tile group, mix product
constexpr int GG_TN_STEPS = STC_GG_TN_STEPS;      // contraction steps (of 4 rows) whose operands are in flight together

__device__ __forceinline__ f32x4 mfma4(float a, float b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }

struct Sel {
    int cell0, cell_step, n_sel, batch;
};
__device__ __forceinline__ size_t plane_of(const Sel& s, int g) { return (size_t)(s.cell0 + (g / s.batch) * s.cell_step) * s.batch + g % s.batch; }

__global__ __launch_bounds__(GG_THREADS) void graph_grad_kernel(const float* __restrict__ A, const float* __restrict__ B, double* __restrict__ part, Sel sel,
                                                                int N, int F, long long chunk_stride) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, j = lane & 15, kq = lane >> 4;
    const int T = (N + 15) >> 4, tiles = T * T, G = sel.n_sel * sel.batch;
    // the wave's output tiles (blockIdx.y: groups of GG_NT_TPW * GG_WAVES tiles); a tile past the end recomputes tile 0 and is not stored
    int it[GG_NT_TPW], jt[GG_NT_TPW];
    bool live[GG_NT_TPW];
#pragma unroll
    for (int t = 0; t < GG_NT_TPW; ++t) {
        const int tile = (blockIdx.y * GG_NT_TPW + t) * GG_WAVES + wave;
        live[t] = tile < tiles;
        it[t] = live[t] ? tile / T : 0;
        jt[t] = live[t] ? tile - it[t] * T : 0;
    }
    double sum[GG_NT_TPW][4];
#pragma unroll
    for (int t = 0; t < GG_NT_TPW; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) sum[t][r] = 0.0;
    for (int g = blockIdx.x; g < G; g += gridDim.x) {
        const float* Ag = A + plane_of(sel, g) * N * F;
        const float* Bg = B + plane_of(sel, g) * N * F;
        f32x4 acc[GG_NT_TPW];
        const float *ar[GG_NT_TPW], *br[GG_NT_TPW];
#pragma unroll
        for (int t = 0; t < GG_NT_TPW; ++t) {
            acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
            // rows beyond N read the last row: they only reach output rows / columns that are not stored
            ar[t] = Ag + (size_t)min(16 * it[t] + j, N - 1) * F;
            br[t] = Bg + (size_t)min(16 * jt[t] + j, N - 1) * F;
        }
        for (int kb = 0; kb < (F + 15) / 16; ++kb) {                // (the same count of steps on every lane; quads past F contribute zeros)
            const int k0 = 16 * kb + 4 * kq;
            const bool ok = k0 < F;
            f32x4 a[GG_NT_TPW], b[GG_NT_TPW];
#pragma unroll
            for (int t = 0; t < GG_NT_TPW; ++t) {                   // every operand of the step requested before the first product
                a[t] = *reinterpret_cast<const f32x4*>(ar[t] + (ok ? k0 : 0));
                b[t] = *reinterpret_cast<const f32x4*>(br[t] + (ok ? k0 : 0));
            }
#pragma unroll
            for (int s = 0; s < 4; ++s)
#pragma unroll
                for (int t = 0; t < GG_NT_TPW; ++t) acc[t] = mfma4(ok ? a[t][s] : 0.f, b[t][s], acc[t]);
        }
#pragma unroll
        for (int t = 0; t < GG_NT_TPW; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) sum[t][r] += (double)acc[t][r];
    }
    double* out = part + (size_t)blockIdx.x * chunk_stride;
#pragma unroll
    for (int t = 0; t < GG_NT_TPW; ++t)
        if (live[t]) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int n = 16 * it[t] + 4 * kq + r, m = 16 * jt[t] + j;
                if (n < N && m < N) out[(size_t)n * N + m] = sum[t][r];
            }
        }
}

// The same product for LARGER N, blocked: a workgroup (4 waves) owns 64 x 64 of the output = 4 x 4 tiles, a wave 2 x 2 of them, and the 64 A rows
// and 64 B rows of every plane go through LDS in pieces of GB_KC columns, double-buffered (the next piece is in registers while this one is
// multiplied; one barrier per piece): every operand row piece leaves L2 once per workgroup and plane and feeds four tiles -- tile per wave
// above fetches both row strips of a plane once per TILE, T = N / 16 times over (13 x at N = 196).
// Same bits as graph_grad_kernel on finite operands: per plane and tile an fp32 accumulator from zero takes the same chain of products (kb
// ascending, s = 0..3, lane quarter kq supplying column 16 kb + 4 kq + s; a quad past F supplies zeros), is folded into the tile's float64
// running sum once per plane, and the planes come in the order g = chunk, chunk + chunks, ...
// LDS rows: GB_KC floats + TWO 16-byte slots.  A ds_read_b128 is served in four groups of 16 lanes ({0-3, 12-15, 20-27}, {4-11, 16-19, 28-31}
// and the same + 32), i.e. of an operand fragment (lane = 16 kq + j: row j, slot kq) the rows {0-3, 12-15} at slot kq with the rows 4-11 at
// slot kq + 1: with a row stride of 10 slots these are the 16 distinct slots of a bank row (10 j mod 16 takes the even values once on either
// row set); a stride of 9 slots (one slot of padding) collides two ways on ten of them.  2 x 128 rows x 160 B = 40 KiB: three workgroups per CU.
constexpr int GB_THREADS = 256, GB_EDGE = 64, GB_KC = 32, GB_LD = GB_KC + 8, GB_ROWS = 2 * GB_EDGE, GB_PASSES = GB_ROWS * (GB_KC / 4) / GB_THREADS;
static_assert(GB_PASSES * GB_THREADS == GB_ROWS * (GB_KC / 4) && GB_PASSES % 2 == 0 && GB_KC % 16 == 0, "staging: whole passes, A rows then B rows");

__global__ __launch_bounds__(GB_THREADS) void graph_grad_blocked_kernel(const float* __restrict__ A, const float* __restrict__ B, double* __restrict__ part, Sel sel,
                                                                        int N, int F, long long chunk_stride) {
    __shared__ __attribute__((aligned(16))) float stage[2][GB_ROWS * GB_LD];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, j = lane & 15, kq = lane >> 4;
    const int NB = (N + GB_EDGE - 1) / GB_EDGE, bi = blockIdx.y / NB, bj = blockIdx.y - bi * NB, G = sel.n_sel * sel.batch;
    const int ti0 = 2 * (wave >> 1), tj0 = 2 * (wave & 1);          // the wave's 2 x 2 tiles inside the block
    bool live_i[2], live_j[2];                                      // (wave-uniform) a tile wholly past N is neither formed nor stored
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        live_i[u] = GB_EDGE * bi + 16 * (ti0 + u) < N;
        live_j[u] = GB_EDGE * bj + 16 * (tj0 + u) < N;
    }
    // staging: thread -> column quad sq of the rows sr + 32 p; staged rows 0..63 are the block's A rows, 64..127 its B rows.  Rows past N
    // are staged from row N - 1: they only reach outputs that are not stored
    const int sq = threadIdx.x % (GB_KC / 4), sr = threadIdx.x / (GB_KC / 4);
    constexpr int ROWS_PER_PASS = GB_THREADS / (GB_KC / 4);
    size_t row_off[GB_PASSES];
#pragma unroll
    for (int p = 0; p < GB_PASSES; ++p) {
        const int r = sr + ROWS_PER_PASS * p;
        row_off[p] = (size_t)min(r < GB_EDGE ? GB_EDGE * bi + r : GB_EDGE * bj + r - GB_EDGE, N - 1) * F;
    }
    const int pieces = (F + GB_KC - 1) / GB_KC;
    const int planes = (int)blockIdx.x < G ? (G - (int)blockIdx.x + (int)gridDim.x - 1) / (int)gridDim.x : 0;
    f32x4 held[GB_PASSES];
    auto fetch = [&](int g, int piece) {                            // one piece of one plane: global -> registers (column quads past F: zeros)
        const size_t plane = plane_of(sel, g) * N * F;
        const int col = GB_KC * piece + 4 * sq;
#pragma unroll
        for (int p = 0; p < GB_PASSES; ++p)
            held[p] = col < F ? *reinterpret_cast<const f32x4*>((p < GB_PASSES / 2 ? A : B) + plane + row_off[p] + col) : f32x4{0.f, 0.f, 0.f, 0.f};
    };
    auto stash = [&](int buf) {                                     // registers -> LDS
#pragma unroll
        for (int p = 0; p < GB_PASSES; ++p) *reinterpret_cast<f32x4*>(&stage[buf][(sr + ROWS_PER_PASS * p) * GB_LD + 4 * sq]) = held[p];
    };
    double sum[2][2][4];
    f32x4 acc[2][2];
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
        for (int v = 0; v < 2; ++v) {
            acc[u][v] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int r = 0; r < 4; ++r) sum[u][v][r] = 0.0;
        }
    if (planes) {
        fetch(blockIdx.x, 0);
        stash(0);
    }
    __syncthreads();
    int g = blockIdx.x, piece = 0;
    for (int step = 0, steps = planes * pieces; step < steps; ++step) {
        const int buf = step & 1;
        int g_next = g, piece_next = piece + 1;
        if (piece_next == pieces) {
            piece_next = 0;
            g_next = g + gridDim.x;
        }
        const bool more = step + 1 < steps;
        if (more) fetch(g_next, piece_next);                        // in flight across this piece's products
        const float* a_rows = &stage[buf][(16 * ti0 + j) * GB_LD + 4 * kq];
        const float* b_rows = &stage[buf][(GB_EDGE + 16 * tj0 + j) * GB_LD + 4 * kq];
#pragma unroll
        for (int kbl = 0; kbl < GB_KC / 16; ++kbl) {
            if (GB_KC * piece + 16 * kbl >= F) break;               // (the steps of graph_grad_kernel: kb < ceil(F / 16), no more)
            f32x4 a[2], b[2];
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                a[u] = *reinterpret_cast<const f32x4*>(a_rows + 16 * u * GB_LD + 16 * kbl);
                b[u] = *reinterpret_cast<const f32x4*>(b_rows + 16 * u * GB_LD + 16 * kbl);
            }
#pragma unroll
            for (int s = 0; s < 4; ++s)
#pragma unroll
                for (int u = 0; u < 2; ++u)
#pragma unroll
                    for (int v = 0; v < 2; ++v)
                        if (live_i[u] && live_j[v]) acc[u][v] = mfma4(a[u][s], b[v][s], acc[u][v]);
        }
        if (piece_next == 0) {                                      // the plane is complete: fold it
#pragma unroll
            for (int u = 0; u < 2; ++u)
#pragma unroll
                for (int v = 0; v < 2; ++v) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) sum[u][v][r] += (double)acc[u][v][r];
                    acc[u][v] = f32x4{0.f, 0.f, 0.f, 0.f};
                }
        }
        if (more) stash(buf ^ 1);                                   // (its last readers passed the barrier that ended the previous step)
        __syncthreads();
        g = g_next;
        piece = piece_next;
    }
    double* out = part + (size_t)blockIdx.x * chunk_stride;         // (a chunk without a plane writes its zeros)
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
        for (int v = 0; v < 2; ++v)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int n = GB_EDGE * bi + 16 * (ti0 + u) + 4 * kq + r, m = GB_EDGE * bj + 16 * (tj0 + v) + j;
                if (n < N && m < N) out[(size_t)n * N + m] = sum[u][v][r];
            }
}

// Which kernel stc_graph_grad_f32 launches (stc_set_graph_grad_form): 0 = by rule, 1 = tile per wave, 2 = blocked.  The two agree bit for bit,
// so the rule is a matter of time alone: blocked from GG_BLOCKED_MIN_N nodes on (measured: profiles/r10/INDEX.md).
std::atomic<int> g_graph_grad_form{0};
constexpr int GG_BLOCKED_MIN_N = 64;
bool graph_grad_blocked(int N) {
    const int form = g_graph_grad_form.load(std::memory_order_relaxed);
    return form == 2 || (form == 0 && N >= GG_BLOCKED_MIN_N);
}

__global__ __launch_bounds__(GG_THREADS) void mix_grad_kernel(const float* __restrict__ A, const float* __restrict__ B, double* __restrict__ part, Sel sel, int N,
                                                              int Fa, int Fb, long long chunk_stride) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, j = lane & 15, kq = lane >> 4;
    const int Ta = (Fa + 15) >> 4, Tb = (Fb + 15) >> 4, tiles = Ta * Tb, G = sel.n_sel * sel.batch;
    int it[GG_TN_TPW], jt[GG_TN_TPW];
    bool live[GG_TN_TPW];
#pragma unroll
    for (int t = 0; t < GG_TN_TPW; ++t) {
        const int tile = (blockIdx.y * GG_TN_TPW + t) * GG_WAVES + wave;
        live[t] = tile < tiles;
        it[t] = live[t] ? tile / Tb : 0;
        jt[t] = live[t] ? tile - it[t] * Tb : 0;
    }
    double sum[GG_TN_TPW][4];
#pragma unroll
    for (int t = 0; t < GG_TN_TPW; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) sum[t][r] = 0.0;
    for (int g = blockIdx.x; g < G; g += gridDim.x) {
        const float* Ag = A + plane_of(sel, g) * N * Fa;
        const float* Bg = B + plane_of(sel, g) * N * Fb;
        f32x4 acc[GG_TN_TPW];
        const float *ac[GG_TN_TPW], *bc[GG_TN_TPW];
#pragma unroll
        for (int t = 0; t < GG_TN_TPW; ++t) {
            acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
            ac[t] = Ag + min(16 * it[t] + j, Fa - 1);                  // columns beyond Fa / Fb: clamped, not stored
            bc[t] = Bg + min(16 * jt[t] + j, Fb - 1);
        }
        for (int n0 = 0; n0 < N; n0 += 4 * GG_TN_STEPS) {          // GG_TN_STEPS steps of 4 rows per pass: every operand of the pass is requested
            float a[GG_TN_STEPS][GG_TN_TPW], b[GG_TN_STEPS][GG_TN_TPW];     // before its first product (one load -> product at a time is an L2 round trip each)
            bool ok[GG_TN_STEPS];
#pragma unroll
            for (int u = 0; u < GG_TN_STEPS; ++u) {
                const int n = n0 + 4 * u + kq;
                ok[u] = n < N;                                          // the rows ARE the contraction: rows past N must contribute zero
                const size_t ra = (size_t)(ok[u] ? n : 0) * Fa, rb = (size_t)(ok[u] ? n : 0) * Fb;
#pragma unroll
                for (int t = 0; t < GG_TN_TPW; ++t) {
                    a[u][t] = ac[t][ra];
                    b[u][t] = bc[t][rb];
                }
            }
#pragma unroll
            for (int u = 0; u < GG_TN_STEPS; ++u)
#pragma unroll
                for (int t = 0; t < GG_TN_TPW; ++t) acc[t] = mfma4(ok[u] ? a[u][t] : 0.f, b[u][t], acc[t]);
        }
#pragma unroll
        for (int t = 0; t < GG_TN_TPW; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) sum[t][r] += (double)acc[t][r];
    }
    double* out = part + (size_t)blockIdx.x * chunk_stride;
#pragma unroll
    for (int t = 0; t < GG_TN_TPW; ++t)
        if (live[t]) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int fa = 16 * it[t] + 4 * kq + r, fb = 16 * jt[t] + j;
                if (fa < Fa && fb < Fb) out[(size_t)fa * Fb + fb] = sum[t][r];
            }
        }
}

int check_sel(const char* what, int32_t cell0, int32_t cell_step, int32_t n_sel, int32_t batch, int32_t n_chunks) {
    STC_REQUIRE(cell0 >= 0 && cell_step >= 1 && n_sel >= 0 && batch >= 1 && n_chunks >= 1 && n_chunks <= 65535, STC_EINVAL,
                "%s: cell0=%d cell_step=%d n_sel=%d batch=%d n_chunks=%d", what, cell0, cell_step, n_sel, batch, n_chunks);
    return STC_OK;
}

}  // namespace

extern "C" int stc_graph_grad_f32(const float* A, const float* B, double* partials, int32_t n_chunks, int32_t cell0, int32_t cell_step, int32_t n_sel,
                                  int32_t batch, int32_t N, int32_t F, int64_t chunk_stride, void* stream) {
    if (int rc = check_sel("stc_graph_grad_f32", cell0, cell_step, n_sel, batch, n_chunks)) return rc;
    STC_REQUIRE(N >= 1 && N <= 4096 && F >= 4 && F % 4 == 0, STC_EINVAL, "stc_graph_grad_f32: N=%d (1..4096), F=%d (a multiple of 4)", N, F);
    STC_REQUIRE(A && B && partials && stc::aligned16(A) && stc::aligned16(B), STC_EINVAL, "stc_graph_grad_f32: null or unaligned operand");
    STC_REQUIRE(chunk_stride == 0 || chunk_stride >= (int64_t)N * N, STC_EINVAL, "stc_graph_grad_f32: chunk stride %lld below the block of %d x %d", (long long)chunk_stride, N, N);
    const long long stride = chunk_stride ? chunk_stride : (int64_t)N * N;
    if (graph_grad_blocked(N)) {
        const int NB = (N + GB_EDGE - 1) / GB_EDGE;
        hipLaunchKernelGGL(graph_grad_blocked_kernel, dim3((unsigned)n_chunks, (unsigned)(NB * NB)), dim3(GB_THREADS), 0, static_cast<hipStream_t>(stream), A, B,
                           partials, Sel{cell0, cell_step, n_sel, batch}, N, F, stride);
    } else {
        const int T = (N + 15) / 16, groups = (T * T + GG_NT_TPW * GG_WAVES - 1) / (GG_NT_TPW * GG_WAVES);
        hipLaunchKernelGGL(graph_grad_kernel, dim3((unsigned)n_chunks, (unsigned)groups), dim3(GG_THREADS), 0, static_cast<hipStream_t>(stream), A, B, partials,
                           Sel{cell0, cell_step, n_sel, batch}, N, F, stride);
    }
    STC_LAUNCH_CHECK("stc_graph_grad_f32 launch");
    return STC_OK;
}

extern "C" int stc_set_graph_grad_form(int32_t form) {
    STC_REQUIRE(form >= 0 && form <= 2, STC_EINVAL, "stc_set_graph_grad_form: form %d (0 = by rule, 1 = tile per wave, 2 = blocked)", form);
    g_graph_grad_form.store(form, std::memory_order_relaxed);
    return STC_OK;
}

extern "C" int stc_mix_grad_f32(const float* A, const float* B, double* partials, int32_t n_chunks, int32_t cell0, int32_t cell_step, int32_t n_sel,
                                int32_t batch, int32_t N, int32_t Fa, int32_t Fb, int64_t chunk_stride, void* stream) {
    if (int rc = check_sel("stc_mix_grad_f32", cell0, cell_step, n_sel, batch, n_chunks)) return rc;
    STC_REQUIRE(N >= 1 && Fa >= 1 && Fb >= 1 && Fa <= 4096 && Fb <= 4096, STC_EINVAL, "stc_mix_grad_f32: N=%d Fa=%d Fb=%d", N, Fa, Fb);
    STC_REQUIRE(A && B && partials, STC_EINVAL, "stc_mix_grad_f32: null operand");
    STC_REQUIRE(chunk_stride == 0 || chunk_stride >= (int64_t)Fa * Fb, STC_EINVAL, "stc_mix_grad_f32: chunk stride %lld below the block of %d x %d", (long long)chunk_stride, Fa, Fb);
    const int tiles = ((Fa + 15) / 16) * ((Fb + 15) / 16), groups = (tiles + GG_TN_TPW * GG_WAVES - 1) / (GG_TN_TPW * GG_WAVES);
    hipLaunchKernelGGL(mix_grad_kernel, dim3((unsigned)n_chunks, (unsigned)groups), dim3(GG_THREADS), 0, static_cast<hipStream_t>(stream), A, B, partials,
                       Sel{cell0, cell_step, n_sel, batch}, N, Fa, Fb, (long long)(chunk_stride ? chunk_stride : (int64_t)Fa * Fb));
    STC_LAUNCH_CHECK("stc_mix_grad_f32 launch");
    return STC_OK;
}
