// query_common.h -- what the query kNN's select (query.hip query_select_kernel) and the re-rank of
// caller-supplied candidates (rerank.hip rerank_kernel) share: a wave's candidate lists in LDS, the
// exact distances of gll_knn_query's contract and the rank-and-keep, so a pair (q, j) gets the same
// bits on either route.
#pragma once

#include <limits.h>

#include "gll_internal.h"

namespace gll {

constexpr int kQCap = 512;             // candidate slots of a wave: k <= 256 kept + 256 new

struct QLists {
    double cd[kQCap];   // float64 d^2 (non-finite: +inf), the ranking key with cj
    int cj[kQCap];      // database row
    float cf[kQCap];    // fp32 d^2, the value returned
};

// Exact distances of the candidates in slots lo .. hi - 1: 8 lanes a candidate, lane `sub`
// features 4 sub + 32 u + (0..3), one fmaf chain a lane (fp32) and one fma chain (float64) over
// the same loads, then the xor butterfly over the 8 lanes.  Features past d add exact zeros, so
// the scalar path gives the vector path's bits.
template <bool VEC>
__device__ inline void q_exact(const float* __restrict__ Xdb, const float* __restrict__ xq, int d,
                               QLists& w, int lo, int hi) {
    const int lane = lane_id(), grp = lane >> 3, sub = lane & 7;
    for (int p0 = lo; p0 < hi; p0 += 8) {
        const int s = p0 + grp;
        const bool live = s < hi;
        const float* xj = Xdb + size_t(live ? w.cj[s] : 0) * d;
        float pf = 0.f;
        double pd = 0.0;
        for (int k = 4 * sub; k < d; k += 32) {
            const f32x4 a = load4<VEC>(xq, k, d), b = load4<VEC>(xj, k, d);
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const float df = a[t] - b[t];
                pf = __builtin_fmaf(df, df, pf);
                const double dd = double(a[t]) - double(b[t]);
                pd = __builtin_fma(dd, dd, pd);
            }
        }
#pragma unroll
        for (int off = 1; off < 8; off <<= 1) {
            pf += __shfl_xor(pf, off);
            pd += __shfl_xor(pd, off);
        }
        if (live && sub == 0) {
            w.cf[s] = pf;
            w.cd[s] = pd == pd ? pd : __builtin_inf();
        }
    }
    __builtin_amdgcn_wave_barrier();
    asm volatile("" ::: "memory");
}

// Ranks slots 0 .. cnt - 1 by (cd, cj) and leaves the first `keep` of that order in slots
// 0 .. keep - 1, sorted.  Every entry is read into registers before any slot is rewritten.
__device__ inline int q_rank_keep(QLists& w, int cnt, int keep) {
    constexpr int S = kQCap / kWave;
    const int lane = lane_id();
    double dv[S];
    float fv[S];
    int jv[S], rk[S];
#pragma unroll
    for (int s = 0; s < S; ++s) {
        const int e = lane + kWave * s;
        const bool in = e < cnt;
        dv[s] = in ? w.cd[e] : __builtin_inf();
        fv[s] = in ? w.cf[e] : 0.f;
        jv[s] = in ? w.cj[e] : INT_MAX;
        rk[s] = 0;
    }
    for (int u = 0; u < cnt; ++u) {
        const double du = w.cd[u];
        const int ju = w.cj[u];
#pragma unroll
        for (int s = 0; s < S; ++s)
            if (s * kWave < cnt) rk[s] += (du < dv[s] || (du == dv[s] && ju < jv[s])) ? 1 : 0;
    }
    __builtin_amdgcn_wave_barrier();
    asm volatile("" ::: "memory");
#pragma unroll
    for (int s = 0; s < S; ++s) {
        if (lane + kWave * s < cnt && rk[s] < keep) {
            w.cd[rk[s]] = dv[s];
            w.cf[rk[s]] = fv[s];
            w.cj[rk[s]] = jv[s];
        }
    }
    __builtin_amdgcn_wave_barrier();
    asm volatile("" ::: "memory");
    return cnt < keep ? cnt : keep;
}

// 16-B loads where both arrays allow them; scalar loads of the same elements otherwise
inline bool q_vec(const float* a, const float* b, int d) {
    return d % 4 == 0 && reinterpret_cast<uintptr_t>(a) % 16 == 0 &&
           reinterpret_cast<uintptr_t>(b) % 16 == 0;
}

// Counts a launch for gll_query_launches and returns its status (query.hip).
hipError_t q_launched(const char* what);

}  // namespace gll
