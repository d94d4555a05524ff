// ComboLoss of the reference trainer (Model_Trainer.py:9-23: mean binary cross-entropy + per-sample Dice, averaged over the batch), forward and
// backward, on strided (batch, segments, seg) operands: sample b is `segments` contiguous runs of `seg` floats, run (b, s) at b sb + s ss.
//
// Forward, two launches: per-chunk partial sums (three per chunk: the BCE terms, p y, p + y; fp32 per thread, float64 from the wave up; no
// atomics), then one workgroup that folds them in a fixed order -> bitwise reproducible.  Backward, one launch, one pass.
// fp32, memory-bound, streaming: 16-byte accesses where bases and strides allow, a scalar path of the same kernels otherwise.
//
// Arithmetic: torch's nn.BCELoss -- log clamped at -100 in the forward, the denominator p (1 - p) at 1e-12 in the backward.  Both clamps are
// written `v < lo ? lo : v`: a NaN fails the comparison and is handed on (fmaxf would drop it).  No device asserts: a prediction outside
// [0, 1] or non-finite gives a NaN loss through the logarithms.
#include "stc_common.h"

namespace {

constexpr int LOSS_THREADS = 256;
constexpr int LOSS_WAVES = LOSS_THREADS / stc::kWave;

__device__ __forceinline__ float clamp_below(float v, float lo) { return v < lo ? lo : v; }      // NaN stays NaN

struct Sums3 {
    float bce, py, sum;
    __device__ __forceinline__ void add(float p, float y) {
        const float lp = clamp_below(logf(p), -100.f), lq = clamp_below(logf(1.f - p), -100.f);
        bce -= y * lp + (1.f - y) * lq;
        py += p * y;
        sum += p + y;
    }
};

// (b, s, chunk) of a workgroup and the chunk's length; the grid is batch * segments * chunks workgroups
struct Chunk {
    long long b;
    long long p_off, y_off;
    int len;
};

__device__ __forceinline__ Chunk chunk_of(unsigned blk, long long segments, long long seg, long long chunks, long long p_sb, long long p_ss,
                                          long long y_sb, long long y_ss) {
    const long long c = blk % chunks, run = blk / chunks;
    const long long s = run % segments, b = run / segments;
    const long long e0 = c * STC_LOSS_CHUNK, left = seg - e0;
    return {b, b * p_sb + s * p_ss + e0, b * y_sb + s * y_ss + e0, (int)(left < STC_LOSS_CHUNK ? left : STC_LOSS_CHUNK)};
}

template <bool VEC>
__global__ __launch_bounds__(LOSS_THREADS) void loss_partials_kernel(const float* __restrict__ p, const float* __restrict__ y, long long segments,
                                                                     long long seg, long long chunks, long long p_sb, long long p_ss,
                                                                     long long y_sb, long long y_ss, double* __restrict__ part) {
    const Chunk ck = chunk_of(blockIdx.x, segments, seg, chunks, p_sb, p_ss, y_sb, y_ss);
    const float* pp = p + ck.p_off;
    const float* yy = y + ck.y_off;
    Sums3 acc = {0.f, 0.f, 0.f};
    if (VEC) {                                                   // len is a multiple of 4, both runs 16-byte aligned
#pragma unroll 4
        for (int i = threadIdx.x * 4; i < ck.len; i += LOSS_THREADS * 4) {
            const float4 a = *reinterpret_cast<const float4*>(pp + i), t = *reinterpret_cast<const float4*>(yy + i);
            acc.add(a.x, t.x);
            acc.add(a.y, t.y);
            acc.add(a.z, t.z);
            acc.add(a.w, t.w);
        }
    } else {
        for (int i = threadIdx.x; i < ck.len; i += LOSS_THREADS) acc.add(pp[i], yy[i]);
    }
    __shared__ double red[LOSS_WAVES][3];
    const double v0 = stc_wave_sum((double)acc.bce), v1 = stc_wave_sum((double)acc.py), v2 = stc_wave_sum((double)acc.sum);
    const int lane = threadIdx.x % stc::kWave, wave = threadIdx.x / stc::kWave;
    if (lane == 0) {
        red[wave][0] = v0;
        red[wave][1] = v1;
        red[wave][2] = v2;
    }
    __syncthreads();
    if (threadIdx.x < 3) {
        double t = red[0][threadIdx.x];
#pragma unroll
        for (int w = 1; w < LOSS_WAVES; ++w) t += red[w][threadIdx.x];
        part[(size_t)blockIdx.x * 3 + threadIdx.x] = t;
    }
}

// One workgroup.  Each wave folds whole samples (lane l takes partials l, l + 64, ... in order, then the butterfly: one fixed order), leaves
// sums[b] = (I_b, D_b) and the sample's BCE sum in `bce_b` (batch doubles of the workspace); the samples are then folded the same way.
// A sample whose BCE sum is NaN (a prediction outside [0, 1] or non-finite) gets NaN sums: 0 * NaN is added to both, so that the backward
// marks the WHOLE sample and not only the elements a NaN happens to reach; finite sums are unchanged by the + 0.
__global__ __launch_bounds__(LOSS_THREADS) void loss_finish_kernel(const double* __restrict__ part, long long batch, long long per_sample,
                                                                   double inv_count, double* __restrict__ bce_b, double* __restrict__ sums,
                                                                   float* __restrict__ loss) {
    const int lane = threadIdx.x % stc::kWave, wave = threadIdx.x / stc::kWave;
    for (long long b = wave; b < batch; b += LOSS_WAVES) {
        const double* pb = part + (size_t)b * per_sample * 3;
        double bce = 0, I = 0, D = 0;
        for (long long i = lane; i < per_sample; i += stc::kWave) {
            bce += pb[i * 3];
            I += pb[i * 3 + 1];
            D += pb[i * 3 + 2];
        }
        bce = stc_wave_sum(bce);
        I = stc_wave_sum(I);
        D = stc_wave_sum(D);
        const double flag = 0.0 * bce;
        if (lane == 0) {
            bce_b[b] = bce;
            sums[b * 2] = I + flag;
            sums[b * 2 + 1] = D + flag;
        }
    }
    __syncthreads();                                             // one workgroup: its own global writes are visible after the barrier
    double bce = 0, dice = 0;
    for (long long b = threadIdx.x; b < batch; b += LOSS_THREADS) {
        bce += bce_b[b];
        dice += 1.0 - 2.0 * sums[b * 2] / sums[b * 2 + 1];
    }
    __shared__ double red[LOSS_WAVES][2];
    bce = stc_wave_sum(bce);
    dice = stc_wave_sum(dice);
    if (lane == 0) {
        red[wave][0] = bce;
        red[wave][1] = dice;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < LOSS_WAVES; ++w) {
            bce += red[w][0];
            dice += red[w][1];
        }
        *loss = (float)(bce * inv_count + dice / (double)batch);
    }
}

//   dp = g [ (p - y) / max(p (1 - p), 1e-12) / M  -  (2 / batch) (y D_b - I_b) / D_b^2 ]  =  g [ bce' inv_m + y a_b + c_b ]
// a_b = -(2 / batch) / D_b and c_b = (2 / batch) I_b / D_b^2 are formed in float64 once per thread.
template <bool VEC>
__global__ __launch_bounds__(LOSS_THREADS) void loss_bwd_kernel(const float* __restrict__ p, const float* __restrict__ y,
                                                                const double* __restrict__ sums, const float* __restrict__ grad_out,
                                                                float* __restrict__ dp, long long batch, long long segments, long long seg,
                                                                long long chunks, long long p_sb, long long p_ss, long long y_sb, long long y_ss,
                                                                float inv_m) {
    const Chunk ck = chunk_of(blockIdx.x, segments, seg, chunks, p_sb, p_ss, y_sb, y_ss);
    const float* pp = p + ck.p_off;
    const float* yy = y + ck.y_off;
    float* dd = dp + ck.p_off;
    const double I = sums[ck.b * 2], D = sums[ck.b * 2 + 1], two_b = 2.0 / (double)batch;
    const float g = grad_out[0], a = (float)(-two_b / D), c = (float)(two_b * I / (D * D));
    auto grad = [&](float pv, float yv) {
        const float den = clamp_below(pv * (1.f - pv), 1e-12f);
        return g * ((pv - yv) / den * inv_m + (yv * a + c));
    };
    if (VEC) {
#pragma unroll 4
        for (int i = threadIdx.x * 4; i < ck.len; i += LOSS_THREADS * 4) {
            const float4 pv = *reinterpret_cast<const float4*>(pp + i), yv = *reinterpret_cast<const float4*>(yy + i);
            *reinterpret_cast<float4*>(dd + i) = make_float4(grad(pv.x, yv.x), grad(pv.y, yv.y), grad(pv.z, yv.z), grad(pv.w, yv.w));
        }
    } else {
        for (int i = threadIdx.x; i < ck.len; i += LOSS_THREADS) dd[i] = grad(pp[i], yy[i]);
    }
}

// chunks per run and workgroups of a launch; -1 for negative sizes, -2 beyond the grid limit
inline long long loss_grid(int64_t batch, int64_t segments, int64_t seg, long long* chunks) {
    if (batch < 0 || segments < 0 || seg < 0) return -1;
    *chunks = (seg + STC_LOSS_CHUNK - 1) / STC_LOSS_CHUNK;
    const unsigned __int128 blocks = (unsigned __int128)batch * (unsigned __int128)segments * (unsigned __int128)*chunks;
    if (blocks >= ((unsigned __int128)1 << 31)) return -2;
    return (long long)blocks;
}

// the checks both directions share; returns the workgroup count through *blocks (0: nothing to launch)
int loss_checked(const char* what, int64_t batch, int64_t segments, int64_t seg, int64_t p_sb, int64_t p_ss, int64_t y_sb, int64_t y_ss,
                 long long* chunks, long long* blocks) {
    STC_REQUIRE(batch >= 0 && segments >= 0 && seg >= 0 && p_sb >= 0 && p_ss >= 0 && y_sb >= 0 && y_ss >= 0, STC_EINVAL,
                "%s: negative size or stride (batch %lld, segments %lld, seg %lld, strides %lld %lld %lld %lld)", what, (long long)batch,
                (long long)segments, (long long)seg, (long long)p_sb, (long long)p_ss, (long long)y_sb, (long long)y_ss);
    *blocks = loss_grid(batch, segments, seg, chunks);
    STC_REQUIRE(*blocks >= 0, STC_ELIMIT, "%s: (%lld, %lld, %lld) gives 2^31 or more chunks of %d elements", what, (long long)batch,
                (long long)segments, (long long)seg, STC_LOSS_CHUNK);
    return STC_OK;
}

inline bool loss_vec(const void* a, const void* b, const void* c, int64_t seg, int64_t p_sb, int64_t p_ss, int64_t y_sb, int64_t y_ss) {
    return stc::aligned16(a) && stc::aligned16(b) && (c == nullptr || stc::aligned16(c)) && ((seg | p_sb | p_ss | y_sb | y_ss) & 3) == 0;
}

}  // namespace

extern "C" size_t stc_combo_loss_workspace_bytes(int64_t batch, int64_t segments, int64_t seg) {
    long long chunks = 0;
    const long long blocks = loss_grid(batch, segments, seg, &chunks);
    return blocks <= 0 ? 0 : ((size_t)blocks * 3 + (size_t)batch) * sizeof(double);      // (blocks > 0: batch < 2^31 as well)
}

extern "C" int stc_combo_loss_fwd_f32(const float* p, const float* y, int64_t batch, int64_t segments, int64_t seg, int64_t p_sb, int64_t p_ss,
                                      int64_t y_sb, int64_t y_ss, float* loss, double* sums, void* workspace, size_t workspace_bytes,
                                      void* stream) {
    long long chunks = 0, blocks = 0;
    if (int rc = loss_checked("stc_combo_loss_fwd_f32", batch, segments, seg, p_sb, p_ss, y_sb, y_ss, &chunks, &blocks)) return rc;
    if (blocks == 0) return STC_OK;
    STC_REQUIRE(p && y && loss && sums && workspace, STC_EINVAL, "stc_combo_loss_fwd_f32: null pointer");
    STC_REQUIRE(stc::aligned(p, 4) && stc::aligned(y, 4) && stc::aligned(loss, 4), STC_EALIGN, "stc_combo_loss_fwd_f32: p, y and loss must be 4-byte aligned");
    STC_REQUIRE(stc::aligned(sums, 8) && stc::aligned(workspace, 8), STC_EALIGN, "stc_combo_loss_fwd_f32: sums and workspace must be 8-byte aligned");
    const size_t need = stc_combo_loss_workspace_bytes(batch, segments, seg);
    STC_REQUIRE(workspace_bytes >= need, STC_EINVAL, "stc_combo_loss_fwd_f32: workspace of %zu bytes, %zu needed", workspace_bytes, need);
    hipStream_t s = static_cast<hipStream_t>(stream);
    double* part = static_cast<double*>(workspace);
    double* bce_b = part + (size_t)blocks * 3;
    const dim3 grid((unsigned)blocks), block(LOSS_THREADS);
    if (loss_vec(p, y, nullptr, seg, p_sb, p_ss, y_sb, y_ss))
        hipLaunchKernelGGL(loss_partials_kernel<true>, grid, block, 0, s, p, y, (long long)segments, (long long)seg, chunks, (long long)p_sb,
                           (long long)p_ss, (long long)y_sb, (long long)y_ss, part);
    else
        hipLaunchKernelGGL(loss_partials_kernel<false>, grid, block, 0, s, p, y, (long long)segments, (long long)seg, chunks, (long long)p_sb,
                           (long long)p_ss, (long long)y_sb, (long long)y_ss, part);
    STC_LAUNCH_CHECK("stc_combo_loss_fwd_f32 partials launch");
    const double inv_count = 1.0 / ((double)batch * (double)segments * (double)seg);
    hipLaunchKernelGGL(loss_finish_kernel, dim3(1), block, 0, s, part, (long long)batch, (long long)(segments * chunks), inv_count, bce_b, sums, loss);
    STC_LAUNCH_CHECK("stc_combo_loss_fwd_f32 finish launch");
    return STC_OK;
}

extern "C" int stc_combo_loss_bwd_f32(const float* p, const float* y, const double* sums, const float* grad_out, float* dp, int64_t batch,
                                      int64_t segments, int64_t seg, int64_t p_sb, int64_t p_ss, int64_t y_sb, int64_t y_ss, void* stream) {
    long long chunks = 0, blocks = 0;
    if (int rc = loss_checked("stc_combo_loss_bwd_f32", batch, segments, seg, p_sb, p_ss, y_sb, y_ss, &chunks, &blocks)) return rc;
    if (blocks == 0) return STC_OK;
    STC_REQUIRE(p && y && sums && grad_out && dp, STC_EINVAL, "stc_combo_loss_bwd_f32: null pointer");
    STC_REQUIRE(stc::aligned(p, 4) && stc::aligned(y, 4) && stc::aligned(grad_out, 4) && stc::aligned(dp, 4), STC_EALIGN,
                "stc_combo_loss_bwd_f32: p, y, grad_out and dp must be 4-byte aligned");
    STC_REQUIRE(stc::aligned(sums, 8), STC_EALIGN, "stc_combo_loss_bwd_f32: sums must be 8-byte aligned");
    STC_REQUIRE(dp != p && dp != y, STC_EINVAL, "stc_combo_loss_bwd_f32: dp must not alias p or y");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)blocks), block(LOSS_THREADS);
    const float inv_m = (float)(1.0 / ((double)batch * (double)segments * (double)seg));
    if (loss_vec(p, y, dp, seg, p_sb, p_ss, y_sb, y_ss))
        hipLaunchKernelGGL(loss_bwd_kernel<true>, grid, block, 0, s, p, y, sums, grad_out, dp, (long long)batch, (long long)segments, (long long)seg,
                           chunks, (long long)p_sb, (long long)p_ss, (long long)y_sb, (long long)y_ss, inv_m);
    else
        hipLaunchKernelGGL(loss_bwd_kernel<false>, grid, block, 0, s, p, y, sums, grad_out, dp, (long long)batch, (long long)segments, (long long)seg,
                           chunks, (long long)p_sb, (long long)p_ss, (long long)y_sb, (long long)y_ss, inv_m);
    STC_LAUNCH_CHECK("stc_combo_loss_bwd_f32 launch");
    return STC_OK;
}
