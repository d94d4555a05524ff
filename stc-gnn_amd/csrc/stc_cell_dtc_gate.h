// The gate gradient of a PLANAR cell, re-formed in registers from the planes the two-launch backward holds (never stored):
//     dG[r][d][0..15]  = dHnew (Cand - H) U (1 - U)          update gate
//     dG[r][d][16..31] = dRH H R (1 - R)                     reset gate
// in 16-byte pieces: piece `part` in 0..7 of category d holds columns 4 part .. 4 part + 3 of the 32.  What stc_cell_dtc_planar.hip (dT_c) and
// stc_cell_dsx_narrow.hip (the d(S.x) plane of a narrow input) share, so that both see the same dG bit for bit.
#pragma once
#include "stc_common.h"

namespace stc_dtc {

using v4f = __attribute__((ext_vector_type(4))) float;
constexpr int H = 16, COLS = 32;           // hidden width; gradient columns per category (update | reset)
constexpr int GS = COLS + 4;               // LDS row stride of a tile of gradient columns (16 rows land on 16 different banks of four)

struct GatePlanes {
    const float *dHnew, *Cand, *U, *dRH, *R, *H;      // (rows, C, 16) each
};

struct GatePiece {
    v4f a, b, c, d;                        // dRH : dHnew | H | R : U | Cand (update gate only)
};

// the four operands of one piece; `at`: float offset of (row, category, 4 (part & 3)) in a state-sized plane
__device__ __forceinline__ GatePiece gate_request(const GatePlanes& p, size_t at, bool second) {
    const v4f zero = {0.f, 0.f, 0.f, 0.f};
    GatePiece g;
    g.a = *reinterpret_cast<const v4f*>((second ? p.dRH : p.dHnew) + at);
    g.b = *reinterpret_cast<const v4f*>(p.H + at);
    g.c = *reinterpret_cast<const v4f*>((second ? p.R : p.U) + at);
    g.d = second ? zero : *reinterpret_cast<const v4f*>(p.Cand + at);
    return g;
}

__device__ __forceinline__ v4f gate_form(const GatePiece& g, bool second) {
    v4f out;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const float f = second ? g.b[e] : g.d[e] - g.b[e];                                    // H : Cand - H
        out[e] = g.a[e] * f * g.c[e] * (1.f - g.c[e]);
    }
    return out;
}

}  // namespace stc_dtc
