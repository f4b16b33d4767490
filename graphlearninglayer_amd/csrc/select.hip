// select.hip -- the exact half of the brute-force kNN for the GLL graph: from the nominating
// distances D2 of gram.hip (K1a) to the K - 1 nearest of every row.
//
//  K1b knn_select_kernel one wave per row:
//                       1. per-lane sorted candidate lists over the D2 row (16-B loads);
//                       2. a threshold merge to kc = K-1+margin candidates (exact 64-bit
//                          merge when a lane's list overflowed);
//                       3. exact re-ranking with d^2 = sum_k (x_ik - x_jk)^2 in float64,
//                          eight candidates at a time (8-lane groups, DPP group sums) --
//                          bitwise symmetric in (i, j) because both orders run the same lane
//                          mapping;
//                       4. the K-1 nearest by (exact d^2, index); self forced to rank 0 with
//                          distance 0 (the stand-in contract of SURVEY.md §8c);
//                       5. a certificate that no column left out of the candidates can beat
//                          the (K-1)-th exact distance given the Gram's error bound, else an
//                          exact re-rank of every column under the bound (rare; counted in
//                          GLL_ST_KNN_RESCAN) -- the result is the exact kNN for any input;
//                       6. every valid pair (i -> j) is pushed onto j's reverse list (or the
//                          overflow list), which is how the symmetric union of GLL.py:197 is
//                          built without an n x n structure or a prefix sum.
// Which instantiation a problem runs: select_route (knn_route.h) and the table above
// launch_select.
#include <limits.h>
#include <stdio.h>

#include <type_traits>

#include "knn_route.h"

namespace gll {

GLL_TRACE_UNIT(select)

// --------------------------------------------------------------------------------------
// K1b: per-row selection + exact re-rank + reverse scatter
// --------------------------------------------------------------------------------------
// A row of D2 as the select reads it: fp32, or fp16 x s decoded x 1/s (H, the pre-split route;
// 1/s is a power of two, so decoding adds no rounding).  Element offsets, 4-aligned for ld4.
template <bool H>
struct D2Row {
    const char* base;
    float inv;
    __device__ __forceinline__ f32x4 ld4(size_t e) const {
        if constexpr (H) {
            const h16x4 v = *reinterpret_cast<const h16x4*>(base + 2 * e);
            return f32x4{float(v.x) * inv, float(v.y) * inv, float(v.z) * inv, float(v.w) * inv};
        } else {   // streamed once per select: nontemporal (stress select 171 -> 153 us,
                   // profiles/r04s_ab_nt.txt)
            return __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(base + 4 * e));
        }
    }
    __device__ __forceinline__ float ld1(size_t e) const {
        if constexpr (H) return float(*reinterpret_cast<const _Float16*>(base + 2 * e)) * inv;
        else return *reinterpret_cast<const float*>(base + 4 * e);
    }
};

// Wave64 minimum of a 32-bit unsigned key through DPP (broadcast result).
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ uint32_t dpp_min_u32(uint32_t v) {
    const uint32_t o = __builtin_amdgcn_update_dpp(0xFFFFFFFFu, v, CTRL, ROW_MASK, 0xf, false);
    return o < v ? o : v;
}
__device__ __forceinline__ uint32_t wave_min_u32(uint32_t v) {
    v = dpp_min_u32<0xB1, 0xf>(v);
    v = dpp_min_u32<0x4E, 0xf>(v);
    v = dpp_min_u32<0x141, 0xf>(v);
    v = dpp_min_u32<0x140, 0xf>(v);
    v = dpp_min_u32<0x142, 0xa>(v);
    v = dpp_min_u32<0x143, 0xc>(v);
    return __builtin_amdgcn_readlane(v, 63);
}

template <int CTRL, int ROW_MASK>
__device__ __forceinline__ uint32_t dpp_max_u32(uint32_t v) {
    const uint32_t o = __builtin_amdgcn_update_dpp(0u, v, CTRL, ROW_MASK, 0xf, false);
    return o > v ? o : v;
}
__device__ __forceinline__ uint32_t wave_max_u32(uint32_t v) {
    v = dpp_max_u32<0xB1, 0xf>(v);
    v = dpp_max_u32<0x4E, 0xf>(v);
    v = dpp_max_u32<0x141, 0xf>(v);
    v = dpp_max_u32<0x140, 0xf>(v);
    v = dpp_max_u32<0x142, 0xa>(v);
    v = dpp_max_u32<0x143, 0xc>(v);
    return __builtin_amdgcn_readlane(v, 63);
}

// Threshold scan: each lane keeps only its TOP smallest D2 bits (min/max network, ~2 VALU per
// slot, against the ~35 of the sorted 64-bit list insert it replaced -- that select was VALU-issue
// bound), T = the kc-th smallest of the 64 x TOP lane entries by bisection -- at least kc distinct
// columns are <= T, so the kc-th smallest D2 is too -- and every column with D2 bits <= T is
// compacted into the wave's LDS slots.  Simulated at kc = 13 / n = 1,000 (TOP = 2) the set
// averages 13.2 columns, at kc = 32 / n = 1,500 (TOP = 3) 32.4; kc = 37 / n = 8,192 (stress,
// TOP = 5) holds ~0.6 of the kc nearest per lane -- five slots, not four, leave fewer rows
// with a full lane list and so a second read (stress select 151 -> 145 us,
// profiles/r04f8_ab_top5.txt).  CH > 0: the row (n <= 1024 CH) stays in
// registers between the two passes; CH = 0 re-reads it (L2 / MALL-hot).  Returns true when more
// than 64 columns tie in (the caller runs select_fallback, tb = T on return).  tb: D2 bits every
// left-out column is >= to (+inf when every valid column is a candidate).
constexpr int kSelNB = 4;   // float4 per lane per 1024-column chunk of a D2 row

// Loads of CH 1024-column chunks of D2 row `row` (sum of NP planes), clamped past ld.
template <int NP, int CH, bool H = false>
__device__ __forceinline__ void load_d2_row(const D2Row<H>& row, size_t plane, int ld,
                                            f32x4 (&v)[CH * kSelNB]) {
    const int lane = lane_id();
#pragma unroll
    for (int c = 0; c < CH; ++c)
#pragma unroll
        for (int b = 0; b < kSelNB; ++b) {
            const int j0 = c * 4 * kWave * kSelNB + 4 * (b * kWave + lane);
            const int jc = j0 < ld ? j0 : 0;
            v[c * kSelNB + b] = row.ld4(jc);
#pragma unroll
            for (int p = 1; p < NP; ++p)
                v[c * kSelNB + b] += row.ld4(p * plane + jc);
        }
}

template <int TOP, int NP, int CH, bool H = false>
__device__ __forceinline__ bool select_threshold(const D2Row<H>& row, size_t plane,
                                                 int n, int ld, int i, int kc,
                                                 int* __restrict__ cand,
                                                 uint32_t* __restrict__ cgd, int& ci, int& kce,
                                                 uint32_t& tb, uint32_t& gbits,
                                                 const f32x4 (&vin)[CH > 0 ? CH * kSelNB : 1]) {
    constexpr int NB = kSelNB;
    constexpr int HV = CH > 0 ? CH * NB * 4 : 1;
    const int lane = lane_id();
    uint32_t m[TOP];
    int mj[CH > 0 ? 1 : TOP];   // CH = 0: the columns of the lane's TOP smallest
#pragma unroll
    for (int t = 0; t < TOP; ++t) m[t] = 0xFFFFFFFFu;
#pragma unroll
    for (int t = 0; t < (CH > 0 ? 1 : TOP); ++t) mj[t] = -1;
    uint32_t hv[HV];
    auto load_chunk = [&](int jb, f32x4 (&v)[NB]) {
#pragma unroll
        for (int b = 0; b < NB; ++b) {
            const int j0 = jb + 4 * (b * kWave + lane);
            const int jc = j0 < ld ? j0 : 0;
            v[b] = row.ld4(jc);
#pragma unroll
            for (int p = 1; p < NP; ++p) v[b] += row.ld4(p * plane + jc);
        }
    };
    auto bits_of = [&](float x, int j) -> uint32_t {   // invalid: 0xFFFFFFFF (> any T)
        return (j < n && j != i && x == x) ? __float_as_uint(x > 0.f ? x : 0.f) : 0xFFFFFFFFu;
    };
    int nvalid = 0;
    // pass 1: per-lane TOP smallest
    auto absorb = [&](uint32_t u) {
        nvalid += u != 0xFFFFFFFFu ? 1 : 0;
#pragma unroll
        for (int t = 0; t < TOP; ++t) {
            const uint32_t lo = m[t] < u ? m[t] : u;
            u = m[t] < u ? u : m[t];
            m[t] = lo;
        }
    };
    auto absorb_j = [&](uint32_t u, int j) {   // the same network carrying the column
        nvalid += u != 0xFFFFFFFFu ? 1 : 0;
#pragma unroll
        for (int t = 0; t < (CH > 0 ? 1 : TOP); ++t) {
            const bool sw = u < m[t];
            const uint32_t mt = m[t];
            const int jt = mj[t];
            m[t] = sw ? u : mt;
            mj[t] = sw ? j : jt;
            u = sw ? mt : u;
            j = sw ? jt : j;
        }
    };
    if constexpr (CH > 0) {   // the row was loaded by the caller (prefetched under the last row)
#pragma unroll
        for (int c = 0; c < CH; ++c) {
#pragma unroll
            for (int b = 0; b < NB; ++b)
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    const uint32_t u = bits_of(vin[c * NB + b][t], c * 4 * kWave * NB + 4 * (b * kWave + lane) + t);
                    hv[(c * NB + b) * 4 + t] = u;
                    absorb(u);
                }
        }
    } else {
        for (int jb = 0; jb < n; jb += 4 * kWave * NB) {
            f32x4 v[NB];
            load_chunk(jb, v);
#pragma unroll
            for (int b = 0; b < NB; ++b)
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    const int j = jb + 4 * (b * kWave + lane) + t;
                    absorb_j(bits_of(v[b][t], j), j);
                }
        }
    }
    GLL_TRACE_PT(16);
    auto count_le = [&](uint32_t t) {
        int c = 0;
#pragma unroll
        for (int s = 0; s < TOP; ++s) c += __popcll(__ballot(m[s] <= t));
        return c;
    };
    uint32_t T = 0xFFFFFFFEu;   // fewer than kc valid entries: every valid column
    if (count_le(T) >= kc) {
        // between the smallest entry and the largest valid one
        uint32_t top = 0;
#pragma unroll
        for (int s = 0; s < TOP; ++s) top = m[s] != 0xFFFFFFFFu ? m[s] : top;
        uint32_t lo = wave_min_u32(m[0]), up = wave_max_u32(top);
        // a T with count_le(T) >= kc (wave-uniform, <= 32 steps); one holding exactly kc list
        // entries ends the search early -- any such T leaves the same list entries in the set
        // (left-out columns stay covered by tb = T + 1, and the kNN is exact either way)
        while (lo < up) {
            const uint32_t mid = lo + ((up - lo) >> 1);
            const int c = count_le(mid);
            if (c == kc) {
                up = mid;
                break;
            }
            if (c > kc) up = mid;
            else lo = mid + 1u;
        }
        T = up;
    }
    // pass 2: compact every column <= T.  CH = 0 (rows re-read from memory): when no lane may
    // hold more columns <= T than its TOP list (a lane whose whole list is <= T while it saw
    // more columns), the lists ARE that set and the row is not read again -- stress: the second
    // read was 22 of a wave's 81 us (profiles/r04p_trace_stress.txt)
    int base = 0, mine = 0;
    auto emit = [&](uint32_t u, int j) {
        const bool p = u <= T;
        const uint64_t mk = __ballot(p);
        const int pos = base + lanes_below(mk);
        if (p && pos < kWave) {
            cand[pos] = j;
            cgd[pos] = u;
        }
        mine += p ? 1 : 0;
        base += __popcll(mk);
    };
    if constexpr (CH > 0) {
#pragma unroll
        for (int c = 0; c < CH; ++c)
#pragma unroll
            for (int b = 0; b < NB; ++b)
#pragma unroll
                for (int t = 0; t < 4; ++t)
                    emit(hv[(c * NB + b) * 4 + t], c * 4 * kWave * NB + 4 * (b * kWave + lane) + t);
    } else if (__ballot(m[TOP - 1] <= T && nvalid > TOP) == 0ull) {
#pragma unroll
        for (int t = 0; t < (CH > 0 ? 1 : TOP); ++t) emit(m[t], mj[t]);
    } else {
        for (int jb = 0; jb < n; jb += 4 * kWave * NB) {
            f32x4 v[NB];
            load_chunk(jb, v);
#pragma unroll
            for (int b = 0; b < NB; ++b)
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    const int j = jb + 4 * (b * kWave + lane) + t;
                    emit(bits_of(v[b][t], j), j);
                }
        }
    }
    const bool redo = base > kWave;
    tb = redo ? T : (__ballot(mine != nvalid) == 0 ? 0x7F800000u : T + 1u);
    __builtin_amdgcn_wave_barrier();   // a wave's LDS ops run in order: the reads see the stores
    asm volatile("" ::: "memory");
    kce = base;
    ci = (!redo && lane < base) ? cand[lane] : -1;
    gbits = (!redo && lane < base) ? cgd[lane] : 0xFFFFFFFFu;
    return redo;
}

// Fallback of the threshold scan when more than 64 columns have D2 bits <= T (ties: duplicate
// points): T' = the kc-th smallest D2 bits of the whole row, by bisection on full-row counts in
// [0, T] (the scan's T already has >= kc columns at or below it; <= 31 passes over the hot row,
// rare), then every column below T' -- fewer than kc -- and columns at T' in index order up to
// 64 slots.  Every column left out is >= T' (tb).  Registers: the scan's, no per-lane key lists
// (the 64-key exact merge it replaces held 128 VGPRs and set the select's occupancy).
template <int NP, bool H = false>
__device__ __forceinline__ void select_fallback(const D2Row<H>& row, size_t plane, int n, int ld,
                                                int i, int kc, int* __restrict__ cand,
                                                uint32_t* __restrict__ cgd, int& ci, int& kce,
                                                uint32_t& tb, uint32_t& gbits) {
    constexpr int NB = kSelNB;
    const int lane = lane_id();
    auto bits_of = [&](float x, int j) -> uint32_t {
        return (j < n && j != i && x == x) ? __float_as_uint(x > 0.f ? x : 0.f) : 0xFFFFFFFFu;
    };
    auto wave_count_le = [&](uint32_t thr) {   // wave-uniform
        int c = 0;
        for (int jb = 0; jb < n; jb += 4 * kWave * NB) {
            f32x4 v[NB];
#pragma unroll
            for (int b = 0; b < NB; ++b) {
                const int j0 = jb + 4 * (b * kWave + lane);
                const int jc = j0 < ld ? j0 : 0;
                v[b] = row.ld4(jc);
#pragma unroll
                for (int p = 1; p < NP; ++p) v[b] += row.ld4(p * plane + jc);
            }
#pragma unroll
            for (int b = 0; b < NB; ++b)
#pragma unroll
                for (int t = 0; t < 4; ++t)
                    c += __popcll(__ballot(bits_of(v[b][t], jb + 4 * (b * kWave + lane) + t) <= thr));
        }
        return c;
    };
    uint32_t lo = 0u, up = tb;   // count_le(tb) >= kc (select_threshold's T)
    while (lo < up) {   // smallest T' with count_le(T') >= kc (wave-uniform)
        const uint32_t mid = lo + ((up - lo) >> 1);
        if (wave_count_le(mid) >= kc) up = mid;
        else lo = mid + 1u;
    }
    const uint32_t T = up;
    // columns below T' (any order), then ties at T' in index order: lane-contiguous columns
    int base = 0;
    auto emit = [&](bool p, uint32_t u, int j) {
        const uint64_t mk = __ballot(p);
        const int pos = base + lanes_below(mk);
        if (p && pos < kWave) {
            cand[pos] = j;
            cgd[pos] = u;
        }
        base += __popcll(mk);
    };
    for (int j0 = 0; j0 < n; j0 += kWave) {
        const int j = j0 + lane;
        float x = 0.f;
        if (j < n) {
            x = row.ld1(j);
#pragma unroll
            for (int p = 1; p < NP; ++p) x += row.ld1(p * plane + j);
        }
        const uint32_t u = bits_of(x, j);
        emit(u < T, u, j);
    }
    for (int j0 = 0; j0 < n && base < kWave; j0 += kWave) {
        const int j = j0 + lane;
        float x = 0.f;
        if (j < n) {
            x = row.ld1(j);
#pragma unroll
            for (int p = 1; p < NP; ++p) x += row.ld1(p * plane + j);
        }
        const uint32_t u = bits_of(x, j);
        emit(u == T, u, j);
    }
    tb = T;
    __builtin_amdgcn_wave_barrier();
    asm volatile("" ::: "memory");
    kce = base < kWave ? base : kWave;
    ci = lane < kce ? cand[lane] : -1;
    gbits = lane < kce ? cgd[lane] : 0xFFFFFFFFu;
}

// 64-bit DPP add of the 8-lane group butterfly (two 32-bit moves per stage).
template <int CTRL>
__device__ __forceinline__ double dpp_add_d(double v) {
    const uint64_t b = __builtin_bit_cast(uint64_t, v);
    const uint32_t lo = __builtin_amdgcn_update_dpp(0, uint32_t(b), CTRL, 0xf, 0xf, false);
    const uint32_t hi = __builtin_amdgcn_update_dpp(0, uint32_t(b >> 32), CTRL, 0xf, 0xf, false);
    return v + __builtin_bit_cast(double, (uint64_t(hi) << 32) | lo);
}
__device__ __forceinline__ double group8_sum_d(double v) {
    v = dpp_add_d<0xB1>(v);
    v = dpp_add_d<0x4E>(v);
    v = dpp_add_d<0x141>(v);
    return v;
}
__device__ __forceinline__ double shfl_d(double v, int src) {
    const uint64_t b = __builtin_bit_cast(uint64_t, v);
    const uint32_t lo = uint32_t(__shfl(int(uint32_t(b)), src));
    const uint32_t hi = uint32_t(__shfl(int(uint32_t(b >> 32)), src));
    return __builtin_bit_cast(double, (uint64_t(hi) << 32) | lo);
}
__device__ __forceinline__ double readlane_d(double v, int l) {
    const uint64_t b = __builtin_bit_cast(uint64_t, v);
    const uint32_t lo = __builtin_amdgcn_readlane(uint32_t(b), l);
    const uint32_t hi = __builtin_amdgcn_readlane(uint32_t(b >> 32), l);
    return __builtin_bit_cast(double, (uint64_t(hi) << 32) | lo);
}

// Exact squared distances d(i, c_L)^2 = sum_k (x_ik - x_jk)^2 for the candidates c_L held by
// lanes L in [lo, hi) (ci = -1: no candidate), 8 lanes per candidate across d, PG groups of 8
// candidates per sweep with every load in flight.  ACC = float: fp32 differences and sums
// (the fast path); ACC = double: float64 differences and sums -- the reference's stand-in
// ranks in float64 -- used where fp32 cannot separate two candidates.  Either
// way the (i, j) and (j, i) sums run the same lane mapping on negated differences: bitwise
// symmetric for the same ACC.  Lanes outside [lo, hi) keep `ce`.
// FULL: d is a multiple of 32 NU, so every feature step is in range -- no clamped addresses and
// no masks (the masked form adds exact zeros there: the same sums bit for bit).  Single-graph
// selects: NS 12.4 -> 11.7-12.1 us, FullySup 22.0 -> 21.3-21.5 us, stress unchanged
// (profiles/r05zx_ab_select_unmasked_gated.txt).
template <bool VEC, int PG, typename ACC, int NU, bool XL, bool FULL, bool SPLIT = false>
__device__ __forceinline__ ACC exact_d2_body(const float* __restrict__ X,
                                             const float* __restrict__ xi, int i, int d, int ci,
                                             int lo, int hi, ACC ce, const float* xs) {
    constexpr bool F64 = std::is_same<ACC, double>::value;
    const int lane = lane_id();
    const int grp = lane >> 3, sub = lane & 7;
    for (int p0 = lo; p0 < hi; p0 += 8 * PG) {
        const float* xj[PG];
#pragma unroll
        for (int g2 = 0; g2 < PG; ++g2) {
            const int idx = p0 + 8 * g2 + grp;
            const int j = __shfl(ci, idx < hi ? idx : lo);
            const bool live = idx < hi && j >= 0;
            xj[g2] = X + size_t(live ? j : i) * d;
        }
        ACC part[PG];
#pragma unroll
        for (int g2 = 0; g2 < PG; ++g2) part[g2] = ACC(0);
        // one step of NU x 32 features, every load in flight; F: no masks (in range)
        auto step = [&](const int kb, auto full) {
            constexpr bool F = decltype(full)::value;
            f32x4 va[NU], vb[PG][NU];
#pragma unroll
            for (int u = 0; u < NU; ++u) {   // straight-line: every load issued before use
                const int k = kb + 32 * u + 4 * sub;
                if constexpr (F) {
                    if constexpr (!XL) va[u] = *reinterpret_cast<const f32x4*>(xi + k);
#pragma unroll
                    for (int g2 = 0; g2 < PG; ++g2)
                        vb[g2][u] = *reinterpret_cast<const f32x4*>(xj[g2] + k);
                } else {
                    if constexpr (!XL) va[u] = load4_raw<VEC>(xi, k, d);
#pragma unroll
                    for (int g2 = 0; g2 < PG; ++g2) vb[g2][u] = load4_raw<VEC>(xj[g2], k, d);
                }

            }
#pragma unroll
            for (int g2 = 0; g2 < PG; ++g2) {
#pragma unroll
                for (int u = 0; u < NU; ++u) {   // same order from either end: symmetric
                    const int k = kb + 32 * u + 4 * sub;
                    if constexpr (XL)   // x_i from the wave's LDS copy, read at use
                        va[u] = *reinterpret_cast<const f32x4*>(xs + k);
                    if constexpr (F64) {
                        const f32x4 a = F ? va[u] : mask4<VEC>(va[u], k, d);
                        const f32x4 b = F ? vb[g2][u] : mask4<VEC>(vb[g2][u], k, d);
                        const double d0 = double(a.x) - double(b.x), d1 = double(a.y) - double(b.y);
                        const double d2 = double(a.z) - double(b.z), d3 = double(a.w) - double(b.w);
                        part[g2] = __builtin_fma(d0, d0, part[g2]);
                        part[g2] = __builtin_fma(d1, d1, part[g2]);
                        part[g2] = __builtin_fma(d2, d2, part[g2]);
                        part[g2] = __builtin_fma(d3, d3, part[g2]);
                    } else {
                        // explicit fma chain: contraction left to the compiler differed
                        // between instantiations (packed multiplies, then adds), and with it
                        // the last bit of d^2 between the select's two forms
                        const f32x4 df = F ? va[u] - vb[g2][u] : mask4<VEC>(va[u] - vb[g2][u], k, d);
                        part[g2] = __builtin_fmaf(df.x, df.x, part[g2]);
                        part[g2] = __builtin_fmaf(df.y, df.y, part[g2]);
                        part[g2] = __builtin_fmaf(df.z, df.z, part[g2]);
                        part[g2] = __builtin_fmaf(df.w, df.w, part[g2]);
                    }
                }
            }
        };
        if constexpr (FULL) {
            for (int kb = 0; kb < d; kb += 32 * NU) step(kb, std::true_type{});
        } else if constexpr (SPLIT) {
            // the whole steps unmasked, then at most one masked step
            const int df = d - d % (32 * NU);
            int kb = 0;
            for (; kb < df; kb += 32 * NU) step(kb, std::true_type{});
            if (kb < d) step(kb, std::false_type{});
        } else {
            for (int kb = 0; kb < d; kb += 32 * NU) step(kb, std::false_type{});
        }
#pragma unroll
        for (int g2 = 0; g2 < PG; ++g2) {
            ACC tot;
            if constexpr (F64) tot = group8_sum_d(part[g2]);
            else tot = group8_sum(part[g2]);
#pragma unroll
            for (int g = 0; g < 8; ++g) {
                ACC v;
                if constexpr (F64) v = readlane_d(tot, 8 * g);
                else v = readlane_f(tot, 8 * g);
                if (lane == p0 + 8 * g2 + g) ce = v;
            }
        }
    }
    return ce;
}

template <bool VEC, int PG, typename ACC, int NU = 16, bool XL = false>
__device__ __forceinline__ ACC exact_d2(const float* __restrict__ X, const float* __restrict__ xi,
                                        int i, int d, int ci, int lo, int hi, ACC ce,
                                        const float* xs = nullptr) {
    // only the single-graph sweep (NU = 16): in the occupancy forms (x_i in LDS, <= 64 / 80
    // VGPRs, NU = 4) a second body -- theirs or the rescan's / refinement's -- spilled (B = 64 NS
    // select 159 -> 186 us, profiles/r05zw_ab_select_unmasked.txt).  Those take SPLIT instead:
    // one body, whole steps unmasked and at most one masked step (B = 64 NS select 161 -> 148 us,
    // FullySup 332 -> 315 us, profiles/r05zy_ab_select_split_b64.txt)
    if constexpr (VEC && !XL && NU >= 16)
        if (d % (32 * NU) == 0)
            return exact_d2_body<VEC, PG, ACC, NU, XL, true>(X, xi, i, d, ci, lo, hi, ce, xs);
    return exact_d2_body<VEC, PG, ACC, NU, XL, false, VEC && XL>(X, xi, i, d, ci, lo, hi, ce, xs);
}

// Rank of this lane's (exact d^2, index) key among lanes [0, cnt); lanes without a candidate
// (ci < 0) sort last.
__device__ __forceinline__ int key_rank(double ce, int ci, int cnt) {
    const int me = ci < 0 ? INT_MAX : ci;
    int rank = 0;
    for (int u = 0; u < cnt; ++u) {
        const double du = readlane_d(ce, u);
        const int iu0 = __builtin_amdgcn_readlane(ci, u);
        const int iu = iu0 < 0 ? INT_MAX : iu0;
        rank += (du < ce || (du == ce && iu < me)) ? 1 : 0;
    }
    return rank;
}

// Conservative bound on |D2_gram(i, j) - d(i, j)^2| for the split-bf16 Gram over centred rows
// a = x - x_0: the dropped lo*lo terms and the bf16 rounding of lo (<= 3 * 2^-18 |a_k b_k|,
// doubled by the -2<a, b> term: 2^-15.4 |a||b|), plus fp32 accumulation at the kernels'
// depth (<= 3d/16 MFMA steps: 2^-24 * 3d/16 * 2 |a||b|, 1.1e-5 |a||b| at d = 1024) and the
// rounding of the centring and of the norms -- all below 2^-13 (|a| + |b|)^2 >= 2^-11 |a||b|
// for d <= 8192 (gll.h caps d at 4096).
constexpr double kGramErr = 1.0 / 8192.0;

// Float64 re-rank of the candidate list (rare: fp32 cannot separate the boundary pair); a
// shallow load pipeline (4 steps in flight) keeps its registers under the common path's.
template <bool VEC>
__device__ __forceinline__ double refine_d2(const float* __restrict__ X, const float* __restrict__ xi,
                                            int i, int d, int ci, int kce) {
    return exact_d2<VEC, 1, double, 4>(X, xi, i, d, ci, 0, kce, __builtin_inf());
}

struct KnnPick {
    double d;   // exact d^2 (float64)
    int j;      // column, -1: none
};

// Exact rescan of every column with D2_gram <= thr (the certificate failed): candidates in
// chunks of up to 64 - (K-1) lanes, float64 distances, the K-1 best (by d^2, index) carried
// in lanes 0..K-2 across chunks (rare path, shallow load pipeline).
template <bool VEC, int NP, bool H = false>
__device__ __forceinline__ KnnPick knn_rescan(const D2Row<H>& row, size_t plane, int n,
                                           int i, const float* __restrict__ X,
                                           const float* __restrict__ xi, int d, int K,
                                           double thr, int* s_cand) {
    const int lane = lane_id();
    const int F = kWave - (K - 1);          // free lanes per chunk (launch: K-1 <= 56)
    int bi = -1;                             // running best: lanes 0..K-2
    double bd = __builtin_inf();
    for (int jb = 0; jb < n; jb += kWave) {
        const int j = jb + lane;
        float v = 0.f;
        if (j < n) {
            v = row.ld1(j);
#pragma unroll
            for (int p = 1; p < NP; ++p) v += row.ld1(p * plane + j);
        }
        bool take = j < n && j != i && v == v && double(v) <= thr;
        uint64_t mask = __ballot(take);
        while (mask) {
            const int pos = lanes_below(mask);
            const bool sel = take && pos < F;
            if (sel) s_cand[pos] = j;
            const int cnt = __popcll(__ballot(sel));
            mask &= ~__ballot(sel);
            take = take && !sel;
            __builtin_amdgcn_wave_barrier();
            asm volatile("" ::: "memory");
            const int off = lane - (K - 1);
            const int cc = lane < K - 1 ? bi : (off < cnt ? s_cand[off] : -1);
            double cd = lane < K - 1 ? bd : __builtin_inf();
            cd = exact_d2<VEC, 1, double, 4>(X, xi, i, d, cc, K - 1, K - 1 + cnt, cd);
            if (cc < 0) cd = __builtin_inf();
            const int rk = key_rank(cd, cc, K - 1 + cnt);
            __builtin_amdgcn_wave_barrier();
            asm volatile("" ::: "memory");
            // keep the K-1 best in rank order: the lane holding rank L goes to LDS slot L
            const uint64_t live = __ballot(lane < K - 1 + cnt && rk < K - 1 && cc >= 0);
            if (((live >> lane) & 1ull) != 0) s_cand[rk] = lane;
            __builtin_amdgcn_wave_barrier();
            asm volatile("" ::: "memory");
            const int nl = __popcll(live);
            const int src = lane < nl ? s_cand[lane] : lane;
            const int nbi = __shfl(cc, src);
            const double nbd = shfl_d(cd, src);
            bi = lane < nl ? nbi : -1;
            bd = lane < nl ? nbd : __builtin_inf();
            __builtin_amdgcn_wave_barrier();
            asm volatile("" ::: "memory");
        }
    }
    return KnnPick{bd, bi};
}

// XQ > 0: x_i staged in LDS, d <= 256 XQ.  CH > 0 (KC <= 32): n <= 1024 CH, the D2 row held in
// registers by the threshold scan.
template <int KC, bool VEC, int NP, int PG, int NU, int XQ = 0, bool R = false, int CH = 0,
          bool H = false>
// Occupancy forms (x_i in LDS): NU = 8 load steps at 6 waves per SIMD (<= 80 VGPRs), NU = 4 at
// 8 waves per SIMD (<= 64 VGPRs).
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(XQ > 0 ? (NU <= 4 ? 8 : (NU <= 8 ? 6 : 1)) : 1)))
void knn_select_kernel(
    const float* __restrict__ D2, int ld, size_t plane, const float* __restrict__ X, int n, int d, int K,
    int kc, float eps_fixed, int auto_eps, int RCAP, int32_t* __restrict__ knn_idx,
    float* __restrict__ knn_d2, float* __restrict__ eps, int32_t* __restrict__ rev_cnt,
    int32_t* __restrict__ rev_idx, float* __restrict__ rev_d2, int32_t* __restrict__ ovf,
    int32_t* __restrict__ status, int32_t* __restrict__ status_pub, size_t xs, size_t wss,
    size_t sts, int r0, int r1, const float* __restrict__ d2s, const int32_t* __restrict__ perm) {
    GLL_TRACE_SCOPE(1);
    GLL_TRACE_PT(20);
    const int2 gxy = batch_xy<R>();   // once (per pointer it re-reads gridDim and divides)
    D2 = gshift_at(D2, wss, gxy.y);
    X = gshift_at(X, xs, gxy.y);
    knn_idx = gshift_at(knn_idx, wss, gxy.y);
    knn_d2 = gshift_at(knn_d2, wss, gxy.y);
    eps = gshift_at(eps, wss, gxy.y);
    rev_cnt = gshift_at(rev_cnt, wss, gxy.y);
    rev_idx = gshift_at(rev_idx, wss, gxy.y);
    rev_d2 = gshift_at(rev_d2, wss, gxy.y);
    ovf = gshift_at(ovf, wss, gxy.y);
    status = gshift_at(status, wss, gxy.y);
    status_pub = gshift_at(status_pub, sts, gxy.y);
    d2s = gshift_at(d2s, wss, gxy.y);
    __shared__ int s_cand[4][kWave];
    __shared__ uint32_t s_cgd[4][kWave];
    constexpr bool XL = XQ > 0;
    __shared__ float s_xi[XL ? 4 : 1][XL ? 256 * XQ : 1];
    const int lane = lane_id();
    const int wv = threadIdx.x >> 6;
    // rows r0 .. r1 - 1: all, or a panel (D2 row i - r0); with a locality order (one large graph,
    // no panels) block b takes positions of the order dealt XCD-contiguously (xcd_tile): each
    // XCD works through a run of rows whose neighbours mostly lie in that same run
    int i;
    if (perm) {
        const int sl = xcd_tile(int(blockIdx.x), int(gridDim.x)) * 4 + wv;
        if (sl >= r1) return;  // whole wave
        i = perm[sl];
    } else {
        i = r0 + gxy.x * 4 + wv;
        if (i >= r1) return;  // whole wave
    }
    // XL: x_i is staged once in LDS by LDS-DMA (global_load_lds: no registers held across the
    // D2 scan -- round 3 staged it through 4 XQ VGPRs that stayed live until the scan ended), so
    // the exact distances hold only the candidates' rows in registers (occupancy) and do not
    // re-load x_i per sweep.  Lanes past d re-read the row's first 16 B (in bounds; the features
    // past d are masked at use).
    if constexpr (XL) {
        const float* xg = X + size_t(i) * d;
#pragma unroll
        for (int q = 0; q < XQ; ++q) {
            const int k = 4 * lane + 256 * q;
            __builtin_amdgcn_global_load_lds(xg + (k < d ? k : 0), (lds_void*)&s_xi[wv][256 * q],
                                             16, 0, 0);
        }
    }

    // 1-2) candidates: short per-lane lists + threshold merge, exact re-run when inexact.
    //      tb: D2 bits every non-candidate column is >= to (+inf: all valid columns taken)
    // fp16 storage (H): decoded x 1/s; its rounding widens every Gram error bound below by
    // rho (relative, half an fp16 ulp) plus sub (absolute, half the smallest subnormal step)
    const float dsc = H ? *d2s : 1.f;   // written by every tile of the GEMM (the same value)
    const D2Row<H> row{reinterpret_cast<const char*>(D2) + size_t(i - r0) * ld * (H ? 2 : 4),
                       1.f / dsc};
    const double rho = H ? 1.0 / 2048.0 : 0.0;
    const double sub = H ? 0x1p-25 / double(dsc) : 0.0;
    // bounds between a true Gram value v and its stored decoding t: |t - v| <= rho |v| + sub
    auto up = [&](double t) { return H ? t + 2.0 * rho * fabs(t) + sub : t; };   // >= v
    auto lo = [&](double t) { return H ? t - 2.0 * rho * fabs(t) - sub : t; };   // <= v
    int ci, kce;
    uint32_t tb, gb;   // gb: this lane's candidate's Gram D2 bits
    {
        f32x4 vrow[CH > 0 ? CH * kSelNB : 1];
        if constexpr (CH > 0) load_d2_row<NP, CH, H>(row, plane, ld, vrow);
        constexpr int TOP = KC == 16 ? 2 : (KC == 32 ? 3 : 5);
        const bool redo = select_threshold<TOP, NP, CH, H>(row, plane, n, ld, i, kc, s_cand[wv],
                                                           s_cgd[wv], ci, kce, tb, gb, vrow);
        GLL_TRACE_PT(17);
        if (redo) {
            if (lane == 0) atomicAdd(&status_pub[GLL_ST_KNN_MERGE], 1);
            select_fallback<NP, H>(row, plane, n, ld, i, kc, s_cand[wv], s_cgd[wv], ci, kce, tb, gb);
        }
    }
    // 2b) drop the candidates the Gram's error bound already rules out, before their exact
    //     distances are computed (each is a d-float row gather): with G = the (K-1)-th smallest
    //     Gram D2 among the candidates and B its error bound (kGramErr, below), the exact
    //     (K-1)-th distance is <= G + B, and a column whose exact d^2 is below that has Gram
    //     D2 < G + 2B; candidates above G + 2B join the left-out columns (tb) that the
    //     certificate of step 5 covers.  NS: 16 candidates -> ~9-10 re-ranked.
    if (K >= 2 && kce > K - 1) {
        const float g = ci >= 0 && lane < kce ? __uint_as_float(gb) : __builtin_inff();
        int grk = 0;   // rank of (g, index) among the candidates
        for (int u = 0; u < kce; ++u) {
            const float gu = readlane_f(g, u);
            const int cu = __builtin_amdgcn_readlane(ci, u);
            grk += (gu < g || (gu == g && cu < ci)) ? 1 : 0;
        }
        const uint64_t kb = __ballot(lane < kce && ci >= 0 && grk == K - 2);
        if (kb) {
            const double G = up(double(readlane_f(g, int(__builtin_ctzll(kb)))));
            float a2 = row.ld1(0);
#pragma unroll
            for (int p = 1; p < NP; ++p) a2 += row.ld1(p * plane);
            const double ai = sqrt(up(double(a2 > 0.f ? a2 : 0.f)));
            const double gp = G > 0.0 ? G : 0.0;
            const double b0 = kGramErr * (2.0 * ai + sqrt(gp)) * (2.0 * ai + sqrt(gp));
            const double r1 = 2.0 * ai + sqrt(gp + b0);
            const double thr = up(G + 2.0 * kGramErr * r1 * r1);   // in stored units
            const bool need = lane < kce && ci >= 0 && (grk < K - 1 || double(g) <= thr);
            const bool drop = lane < kce && ci >= 0 && !need;
            // the smallest dropped Gram D2 joins the left-out bound
            const uint32_t dmin = wave_min_u32(drop ? gb : 0xFFFFFFFFu);
            if (dmin < tb) tb = dmin;
            const uint64_t nm = __ballot(need);
            if (need) s_cand[wv][lanes_below(nm)] = ci;
            __builtin_amdgcn_wave_barrier();
            asm volatile("" ::: "memory");
            kce = __popcll(nm);
            ci = lane < kce ? s_cand[wv][lane] : -1;
        }
    }
    // 3) exact squared distances of the candidates, fp32.  PG passes per sweep for single
    //    graphs (one wave per SIMD anyway); batches keep PG = 1 (register pressure).
    const float* xi = X + size_t(i) * d;
    // the LDS-DMA copy of x_i (issued at entry) has landed: DMA writes count in vmcnt, which
    // the compiler does not track for them
    if constexpr (XL) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_wave_barrier();
    asm volatile("" ::: "memory");
    double ce = double(exact_d2<VEC, PG, float, NU, XL>(X, xi, i, d, ci, 0, kce,
                                                        __builtin_inff(), &s_xi[wv][0]));
    GLL_TRACE_PT(18);
    if (ci < 0) ce = __builtin_inf();
    // 4) rank the candidates by (exact d^2, index); keep the K-1 nearest
    int rank = key_rank(ce, ci, kce);
    //    fp32 sums of d terms carry <= (d/8 + 3) 2^-24 relative error: where the pair at the
    //    set boundary (ranks K-2 | K-1) -- or, for auto eps, the pair that decides the kth
    //    neighbour (K-3 | K-2) -- is closer than 4x that, rank again in float64
    {
        const double tol = double(d / 8 + 16) * (1.0 / 4194304.0);
        auto at_rank = [&](int r) -> double {
            const uint64_t b = __ballot(lane < kce && ci >= 0 && rank == r);
            return b ? readlane_d(ce, int(__builtin_ctzll(b))) : __builtin_inf();
        };
        bool tie = false;
        if (K >= 2 && kce > K - 1) {
            const double a = at_rank(K - 2), b = at_rank(K - 1);
            tie |= b - a <= tol * b;
        }
        if (auto_eps && K >= 3) {
            const double a = at_rank(K - 3), b = at_rank(K - 2);
            tie |= b - a <= tol * b;
        }
        if (tie) {
            ce = refine_d2<VEC>(X, xi, i, d, ci, kce);
            if (ci < 0) ce = __builtin_inf();
            rank = key_rank(ce, ci, kce);
        }
    }
    bool keep = lane < kce && ci >= 0 && rank < K - 1;
    int nkeep = __popcll(__ballot(keep));

    // 5) certificate: every column left out has D2_gram >= tb; a left-out j that belongs in
    //    the K-1 nearest has d_ij^2 <= dK (the (K-1)-th exact distance found) and so
    //    |a_j| <= |a_i| + sqrt(dK), D2_gram <= dK + B with B = kGramErr (2|a_i| + sqrt(dK))^2.
    //    tb > dK + B rules that out.  |a_i|^2 = D2[i][0] (row 0 is the Gram's centre, a_0 = 0).
    //    Otherwise (rare: features far from row 0 relative to the neighbour gaps) every
    //    column with D2_gram <= dK + B is re-ranked exactly (knn_rescan).
    if (K >= 2 && nkeep == K - 1 && tb < 0x7F800000u) {
        const uint64_t kb = __ballot(keep && rank == K - 2);
        const double dK = readlane_d(ce, int(__builtin_ctzll(kb)));
        float a2 = row.ld1(0);
#pragma unroll
        for (int p = 1; p < NP; ++p) a2 += row.ld1(p * plane);
        const double ai = sqrt(up(double(a2 > 0.f ? a2 : 0.f)));
        const double r = 2.0 * ai + sqrt(dK);
        const double thr = dK + kGramErr * r * r;
        if (!(lo(double(__uint_as_float(tb))) > thr)) {
            if (lane == 0) atomicAdd(&status_pub[GLL_ST_KNN_RESCAN], 1);
            const KnnPick pk = knn_rescan<VEC, NP, H>(row, plane, n, i, X, xi, d, K, up(thr),
                                                      s_cand[wv]);
            ci = pk.j;
            ce = pk.d;
            kce = K - 1;
            rank = key_rank(ce, ci, kce);
            keep = lane < kce && ci >= 0 && rank < K - 1;
            nkeep = __popcll(__ballot(keep));
        }
    }
    int32_t* oi = knn_idx + size_t(i) * K;
    float* od = knn_d2 + size_t(i) * K;
    const float cef = float(ce);   // correctly rounded exact d^2
    if (lane == 0) {
        oi[0] = i;
        od[0] = 0.f;
    }
    if (keep) {
        oi[1 + rank] = ci;
        od[1 + rank] = cef;
    }
    // rows with fewer valid candidates (non-finite input) fall back to self at distance 0,
    // i.e. dropped edges (sparse.find drops zeros, GLL.py:198)
    if (lane >= nkeep && lane < K - 1) {
        oi[1 + lane] = i;
        od[1 + lane] = 0.f;
    }
    GLL_TRACE_PT(19);
    float ei = eps_fixed;
    if (auto_eps) {
        // eps_i = d(i, knn_ind[i, K-1])  (GLL.py:205)
        const float e = (keep && rank == K - 2) ? sqrtf(cef) : 0.f;
        ei = wave_sum_dpp(e);
    }
    if (lane == 0) {
        eps[i] = ei;
        if (!(ei >= 1e-10f)) atomicOr(&status_pub[GLL_ST_TINY_EPS], 1);  // GLL.py:240-241
    }
    // 5) reverse entry (ci, i) for every valid pair; zero distances never enter the graph
    if (keep && cef > 0.f) {
        const int pos = atomicAdd(&rev_cnt[ci], 1);
        if (pos < RCAP) {
            rev_idx[size_t(ci) * RCAP + pos] = i;
            rev_d2[size_t(ci) * RCAP + pos] = cef;
        } else {
            const int q = atomicAdd(&status[kStOvfCount], 1);
            ovf[3 * q + 0] = ci;
            ovf[3 * q + 1] = i;
            ovf[3 * q + 2] = __float_as_int(cef);
        }
    }
}

// --------------------------------------------------------------------------------------
// Wide kNN select (kMaxKm1 < K - 1 <= kMaxKm1Huge: k up to 257 incl. self, e.g. utils.laplace
// with knn_num = 64, 100 or 200, utils.py:574).  knn_select_kernel holds one candidate per lane, so
// its list (K - 1 plus a re-rank margin) and the rescan's lanes cap K - 1 at 56.  Here a wave
// keeps its row's candidates in LDS (kWideCap slots) and its running K - 1 nearest as a sorted
// list in LDS, and ranks in float64 throughout:
//   1. the same threshold scan (per-lane TOP = 4 smallest Gram D2 bits, bisection for T with at
//      least kc = K - 1 + 8 list entries <= T, then every column <= T compacted into LDS; more
//      than kWideCap ties: T' = the kc-th smallest of the whole row by bisection on full-row
//      counts, ties at T' in index order);
//   2. trimming by the Gram error bound (knn_select_kernel step 2b): G = the (K-1)-th smallest
//      candidate Gram D2, candidates above G + 2B join the left-out bound tb;
//   3. exact float64 difference-form distances of the kept candidates, 64 per chunk, merged into
//      the sorted list by (d^2, index) -- the reference's stand-in ranks in float64;
//   4. the certificate of knn_select_kernel step 5; if it fails, every column with Gram D2 under
//      the bound is streamed through the same merge (GLL_ST_KNN_RESCAN).
// Exact for any input like the narrow kernel; distances are the float64 sums rounded once.
// --------------------------------------------------------------------------------------
// Two tiers share the kernel: K - 1 <= 128 (kMaxKm1Wide) with 256 candidate slots and per-lane
// lists of 4, and K - 1 <= 256 (kMaxKm1Huge, round 6) with 512 slots and lists of 5 (64 x 5 >=
// kc = K - 1 + 8); the LDS lists of a wave are 5.5 / 10.5 KiB.
template <int CAP, int KMX>
struct WideListsT {
    int cj[CAP];               // candidates: column
    uint32_t cg[CAP];          // candidates: Gram D2 bits
    double cd[kWave];          // a chunk's float64 distances
    int bj[2][KMX];            // sorted K - 1 nearest (double-buffered merge)
    double bd[2][KMX];
};

template <bool VEC, typename WL>
__device__ __forceinline__ int wide_absorb(const float* __restrict__ X, const float* __restrict__ xi,
                                           int i, int d, int Km1, int cj, int cnt, WL& w,
                                           int& cur, int nb) {
    const int lane = lane_id();
    double dv = exact_d2<VEC, 1, double, 4>(X, xi, i, d, lane < cnt ? cj : -1, 0, cnt,
                                            __builtin_inf());
    if (!(dv == dv) || lane >= cnt || cj < 0) dv = __builtin_inf();   // NaN rows rank last
    const int jj = lane < cnt ? cj : INT_MAX;
    w.cd[lane] = dv;
    w.cj[lane] = jj;   // the chunk's candidates were read out of cj[] before this call
    __builtin_amdgcn_wave_barrier();
    asm volatile("" ::: "memory");
    const int nxt = cur ^ 1;
    auto less = [](double da, int ja, double db, int jb) {
        return da < db || (da == db && ja < jb);
    };
    // chunk entry `lane`: its rank among the chunk and among the list
    int rk = 0;
    for (int u = 0; u < cnt; ++u) rk += less(w.cd[u], w.cj[u], dv, jj) ? 1 : 0;
    for (int e = 0; e < nb; ++e) rk += less(w.bd[cur][e], w.bj[cur][e], dv, jj) ? 1 : 0;
    // list entries: rank = own position + chunk entries before it
    for (int e0 = 0; e0 < nb; e0 += kWave) {
        const int e = e0 + lane;
        if (e < nb) {
            const double de = w.bd[cur][e];
            const int je = w.bj[cur][e];
            int r = e;
            for (int u = 0; u < cnt; ++u) r += less(w.cd[u], w.cj[u], de, je) ? 1 : 0;
            if (r < Km1) {
                w.bd[nxt][r] = de;
                w.bj[nxt][r] = je;
            }
        }
    }
    if (lane < cnt && rk < Km1 && dv < __builtin_inf()) {
        w.bd[nxt][rk] = dv;
        w.bj[nxt][rk] = jj;
    }
    int valid = __popcll(__ballot(lane < cnt && dv < __builtin_inf()));
    __builtin_amdgcn_wave_barrier();
    asm volatile("" ::: "memory");
    cur = nxt;
    return min(nb + valid, Km1);
}

template <bool VEC, int NP, int CAP, int KMX, int TOP>
__global__ __launch_bounds__(256) void knn_select_wide_kernel(
    const float* __restrict__ D2, int ld, size_t plane, const float* __restrict__ X, int n, int d,
    int K, int kc, float eps_fixed, int auto_eps, int RCAP, int32_t* __restrict__ knn_idx,
    float* __restrict__ knn_d2, float* __restrict__ eps, int32_t* __restrict__ rev_cnt,
    int32_t* __restrict__ rev_idx, float* __restrict__ rev_d2, int32_t* __restrict__ ovf,
    int32_t* __restrict__ status, int32_t* __restrict__ status_pub, size_t xs, size_t wss,
    size_t sts, int r0, int r1, const int32_t* __restrict__ perm) {
    const int2 gxy = batch_xy<false>();
    D2 = gshift_at(D2, wss, gxy.y);
    X = gshift_at(X, xs, gxy.y);
    knn_idx = gshift_at(knn_idx, wss, gxy.y);
    knn_d2 = gshift_at(knn_d2, wss, gxy.y);
    eps = gshift_at(eps, wss, gxy.y);
    rev_cnt = gshift_at(rev_cnt, wss, gxy.y);
    rev_idx = gshift_at(rev_idx, wss, gxy.y);
    rev_d2 = gshift_at(rev_d2, wss, gxy.y);
    ovf = gshift_at(ovf, wss, gxy.y);
    status = gshift_at(status, wss, gxy.y);
    status_pub = gshift_at(status_pub, sts, gxy.y);
    constexpr int kWideCap = CAP;
    constexpr int kWideTop = TOP;
    __shared__ WideListsT<CAP, KMX> s_w[4];
    const int lane = lane_id();
    const int wv = threadIdx.x >> 6;
    int i;
    if (perm) {
        const int sl = xcd_tile(int(blockIdx.x), int(gridDim.x)) * 4 + wv;
        if (sl >= r1) return;   // whole wave
        i = perm[sl];
    } else {
        i = r0 + gxy.x * 4 + wv;
        if (i >= r1) return;    // whole wave
    }
    WideListsT<CAP, KMX>& w = s_w[wv];
    const int Km1 = K - 1;
    const D2Row<false> row{reinterpret_cast<const char*>(D2) + size_t(i - r0) * ld * 4, 1.f};
    auto bits_of = [&](float x, int j) -> uint32_t {   // invalid: 0xFFFFFFFF (> any T)
        return (j < n && j != i && x == x) ? __float_as_uint(x > 0.f ? x : 0.f) : 0xFFFFFFFFu;
    };
    auto load4 = [&](int jb) {   // columns jb + 4 lane .. + 3 (sum of NP planes), clamped
        const int j0 = jb + 4 * lane;
        const int jc = j0 < ld ? j0 : 0;
        f32x4 v = row.ld4(jc);
#pragma unroll
        for (int p = 1; p < NP; ++p) v += row.ld4(p * plane + jc);
        return v;
    };
    auto ld1 = [&](int j) {
        float x = row.ld1(j);
#pragma unroll
        for (int p = 1; p < NP; ++p) x += row.ld1(p * plane + j);
        return x;
    };
    // ---- 1. threshold scan: per-lane TOP smallest bits
    uint32_t m[kWideTop];
#pragma unroll
    for (int t = 0; t < kWideTop; ++t) m[t] = 0xFFFFFFFFu;
    int nvalid = 0;
    for (int jb = 0; jb < n; jb += 4 * kWave) {
        const f32x4 v = load4(jb);
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            uint32_t u = bits_of(v[t], jb + 4 * lane + t);
            nvalid += u != 0xFFFFFFFFu ? 1 : 0;
#pragma unroll
            for (int s = 0; s < kWideTop; ++s) {
                const uint32_t lo = m[s] < u ? m[s] : u;
                u = m[s] < u ? u : m[s];
                m[s] = lo;
            }
        }
    }
    auto count_le = [&](uint32_t t) {
        int c = 0;
#pragma unroll
        for (int s = 0; s < kWideTop; ++s) c += __popcll(__ballot(m[s] <= t));
        return c;
    };
    uint32_t T = 0xFFFFFFFEu;   // fewer than kc valid entries: every valid column
    if (count_le(T) >= kc) {
        uint32_t lo = wave_min_u32(m[0]), up = 0;
        uint32_t top = 0;
#pragma unroll
        for (int s = 0; s < kWideTop; ++s) top = m[s] != 0xFFFFFFFFu ? m[s] : top;
        up = wave_max_u32(top);
        while (lo < up) {
            const uint32_t mid = lo + ((up - lo) >> 1);
            const int c = count_le(mid);
            if (c == kc) {
                up = mid;
                break;
            }
            if (c > kc) up = mid;
            else lo = mid + 1u;
        }
        T = up;
    }
    // compaction of every column <= T
    int base = 0, mine = 0;
    for (int jb = 0; jb < n; jb += 4 * kWave) {
        const f32x4 v = load4(jb);
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int j = jb + 4 * lane + t;
            const uint32_t u = bits_of(v[t], j);
            const bool p = u <= T;
            const uint64_t mk = __ballot(p);
            const int pos = base + lanes_below(mk);
            if (p && pos < kWideCap) {
                w.cj[pos] = j;
                w.cg[pos] = u;
            }
            mine += p ? 1 : 0;
            base += __popcll(mk);
        }
    }
    uint32_t tb;   // Gram D2 bits every left-out column is >= to
    int N;
    if (base > kWideCap) {   // ties: T' = the kc-th smallest of the row, ties in index order
        if (lane == 0) atomicAdd(&status_pub[GLL_ST_KNN_MERGE], 1);
        auto count_full = [&](uint32_t thr) {
            int c = 0;
            for (int jb = 0; jb < n; jb += 4 * kWave) {
                const f32x4 v = load4(jb);
#pragma unroll
                for (int t = 0; t < 4; ++t)
                    c += __popcll(__ballot(bits_of(v[t], jb + 4 * lane + t) <= thr));
            }
            return c;
        };
        uint32_t lo = 0u, up = T;
        while (lo < up) {
            const uint32_t mid = lo + ((up - lo) >> 1);
            if (count_full(mid) >= kc) up = mid;
            else lo = mid + 1u;
        }
        const uint32_t T2 = up;
        base = 0;
        for (int pass = 0; pass < 2; ++pass) {   // below T2 (< kc of them), then ties in order
            for (int j0 = 0; j0 < n && base < kWideCap; j0 += kWave) {
                const int j = j0 + lane;
                const uint32_t u = bits_of(j < n ? ld1(j) : 0.f, j);
                const bool p = pass == 0 ? u < T2 : u == T2;
                const uint64_t mk = __ballot(p);
                const int pos = base + lanes_below(mk);
                if (p && pos < kWideCap) {
                    w.cj[pos] = j;
                    w.cg[pos] = u;
                }
                base += __popcll(mk);
            }
        }
        N = min(base, kWideCap);
        tb = T2;
    } else {
        N = base;
        tb = __ballot(mine != nvalid) == 0 ? 0x7F800000u : T + 1u;
    }
    __builtin_amdgcn_wave_barrier();
    asm volatile("" ::: "memory");
    const float* xi = X + size_t(i) * d;
    float a2 = ld1(0);   // |a_i|^2: column 0 is the Gram's centre row (a_0 = 0)
    const double ai = sqrt(double(a2 > 0.f ? a2 : 0.f));
    // ---- 2. trimming: G = the (K-1)-th smallest candidate Gram D2
    if (N > Km1) {
        uint32_t g[kWideCap / kWave];
#pragma unroll
        for (int t = 0; t < kWideCap / kWave; ++t) {
            const int e = t * kWave + lane;
            g[t] = e < N ? w.cg[e] : 0xFFFFFFFFu;
        }
        auto cnt_le = [&](uint32_t thr) {
            int c = 0;
#pragma unroll
            for (int t = 0; t < kWideCap / kWave; ++t) c += __popcll(__ballot(g[t] <= thr));
            return c;
        };
        uint32_t lo = 0u, up = 0xFFFFFFFEu;
        while (lo < up) {
            const uint32_t mid = lo + ((up - lo) >> 1);
            if (cnt_le(mid) >= Km1) up = mid;
            else lo = mid + 1u;
        }
        const double G = double(__uint_as_float(up));
        const double b0 = kGramErr * (2.0 * ai + sqrt(G)) * (2.0 * ai + sqrt(G));
        const double rr = 2.0 * ai + sqrt(G + b0);
        const double thr = G + 2.0 * kGramErr * rr * rr;
        int keep = 0;
        uint32_t dmin = 0xFFFFFFFFu;
#pragma unroll
        for (int t = 0; t < kWideCap / kWave; ++t) {   // in place: chunk t is read before written
            const int e = t * kWave + lane;
            const int j = e < N ? w.cj[e] : -1;
            const bool live = e < N;
            const bool need = live && double(__uint_as_float(g[t])) <= thr;
            if (live && !need) dmin = dmin < g[t] ? dmin : g[t];
            const uint64_t mk = __ballot(need);
            if (need) {
                w.cj[keep + lanes_below(mk)] = j;
                w.cg[keep + lanes_below(mk)] = g[t];
            }
            keep += __popcll(mk);
            __builtin_amdgcn_wave_barrier();
            asm volatile("" ::: "memory");
        }
        dmin = wave_min_u32(dmin);
        if (dmin < tb) tb = dmin;
        N = keep;
    }
    // ---- 3. float64 distances, merged into the sorted list
    int cur = 0, nb = 0;
    for (int c0 = 0; c0 < N; c0 += kWave) {
        const int cnt = min(kWave, N - c0);
        const int cj = lane < cnt ? w.cj[c0 + lane] : -1;
        __builtin_amdgcn_wave_barrier();
        asm volatile("" ::: "memory");
        nb = wide_absorb<VEC>(X, xi, i, d, Km1, cj, cnt, w, cur, nb);
    }
    // ---- 4. certificate (knn_select_kernel step 5), else a rescan under the bound
    if (Km1 >= 1 && nb == Km1 && tb < 0x7F800000u) {
        const double dK = w.bd[cur][Km1 - 1];
        const double r = 2.0 * ai + sqrt(dK);
        const double thr = dK + kGramErr * r * r;
        if (!(double(__uint_as_float(tb)) > thr)) {
            if (lane == 0) atomicAdd(&status_pub[GLL_ST_KNN_RESCAN], 1);
            nb = 0;
            for (int j0 = 0; j0 < n; j0 += kWave) {
                const int j = j0 + lane;
                const float v = j < n ? ld1(j) : 0.f;
                const bool take = j < n && j != i && v == v && double(v) <= thr;
                const uint64_t mk = __ballot(take);
                if (mk == 0ull) continue;
                if (take) w.cj[lanes_below(mk)] = j;
                __builtin_amdgcn_wave_barrier();
                asm volatile("" ::: "memory");
                const int cnt = __popcll(mk);
                const int cj = lane < cnt ? w.cj[lane] : -1;
                __builtin_amdgcn_wave_barrier();
                asm volatile("" ::: "memory");
                nb = wide_absorb<VEC>(X, xi, i, d, Km1, cj, cnt, w, cur, nb);
            }
        }
    }
    // ---- outputs (knn_select_kernel's)
    int32_t* oi = knn_idx + size_t(i) * K;
    float* od = knn_d2 + size_t(i) * K;
    if (lane == 0) {
        oi[0] = i;
        od[0] = 0.f;
    }
    for (int r = lane; r < Km1; r += kWave) {
        const bool live = r < nb;
        oi[1 + r] = live ? w.bj[cur][r] : i;   // fewer valid: self at 0 (dropped edges)
        od[1 + r] = live ? float(w.bd[cur][r]) : 0.f;
    }
    float ei = eps_fixed;
    if (auto_eps) ei = nb == Km1 ? sqrtf(float(w.bd[cur][Km1 - 1])) : 0.f;   // GLL.py:205
    if (lane == 0) {
        eps[i] = ei;
        if (!(ei >= 1e-10f)) atomicOr(&status_pub[GLL_ST_TINY_EPS], 1);   // GLL.py:240-241
    }
    for (int r = lane; r < nb; r += kWave) {   // reverse entries (ci, i); zero distances dropped
        const int ci = w.bj[cur][r];
        const float cef = float(w.bd[cur][r]);
        if (cef > 0.f) {
            const int pos = atomicAdd(&rev_cnt[ci], 1);
            if (pos < RCAP) {
                rev_idx[size_t(ci) * RCAP + pos] = i;
                rev_d2[size_t(ci) * RCAP + pos] = cef;
            } else {
                const int q = atomicAdd(&status[kStOvfCount], 1);
                ovf[3 * q + 0] = ci;
                ovf[3 * q + 1] = i;
                ovf[3 * q + 2] = __float_as_int(cef);
            }
        }
    }
}

// --------------------------------------------------------------------------------------
// The instantiated variants.  One list: a row of X is a table row AND the instantiation of its
// kernel, so neither exists without the other.  Columns: KC, V, NP, PG, NU, XQ, R, CH, H
// (knn_route.h SelVariant).  The list is every variant select_route can return, and nothing
// else (tests/test_lib_cpu.py sweeps gll_select_route over it):
//   - latency rows (PG 2, XQ 0, R 0) need bt.B == 1, and H needs d2_half, which needs bt.B > 1:
//     no latency row has H;
//   - NP = 2 needs gram_planes == 2: one graph of n <= 1024 rows with the whole matrix
//     (panel_rows == n, so rows == n), which d2_half excludes and which puts a KC <= 32, V row
//     at CH = 1: the NP = 2 rows have H = 0, and CH = 1 exactly when KC <= 32 and V;
//   - CH > 0 needs KC <= 32 and V; without V the occupancy form has XQ = 0;
//   - everything else is reachable: the d ladder sets (NU, XQ), n and rows set CH (CH = 0 at
//     KC <= 32 through n > 2048 or a row panel), presplit_route holds for any n at a large
//     enough batch (H), and the occupancy rows with H = 0 -- NP = 2 among them -- run for one
//     graph under GLL_KNOB_SEL_FORM = 2 or GLL_FLAG_D2_F32.
// --------------------------------------------------------------------------------------
#define GLL_SEL_VARIANTS(X)                                                                      \
    X(16, 1, 2, 2, 16, 0, 0, 1, 0) X(16, 1, 1, 2,  4, 0, 0, 1, 0) X(16, 1, 1, 2,  4, 0, 0, 2, 0) \
    X(16, 1, 1, 2,  4, 0, 0, 0, 0) X(16, 1, 1, 2, 16, 0, 0, 1, 0) X(16, 1, 1, 2, 16, 0, 0, 2, 0) \
    X(16, 1, 1, 2, 16, 0, 0, 0, 0) X(16, 0, 2, 2, 16, 0, 0, 0, 0) X(16, 0, 1, 2,  4, 0, 0, 0, 0) \
    X(16, 0, 1, 2, 16, 0, 0, 0, 0) X(32, 1, 2, 2, 16, 0, 0, 1, 0) X(32, 1, 1, 2,  4, 0, 0, 1, 0) \
    X(32, 1, 1, 2,  4, 0, 0, 2, 0) X(32, 1, 1, 2,  4, 0, 0, 0, 0) X(32, 1, 1, 2, 16, 0, 0, 1, 0) \
    X(32, 1, 1, 2, 16, 0, 0, 2, 0) X(32, 1, 1, 2, 16, 0, 0, 0, 0) X(32, 0, 2, 2, 16, 0, 0, 0, 0) \
    X(32, 0, 1, 2,  4, 0, 0, 0, 0) X(32, 0, 1, 2, 16, 0, 0, 0, 0) X(64, 1, 2, 2, 16, 0, 0, 0, 0) \
    X(64, 1, 1, 2,  4, 0, 0, 0, 0) X(64, 1, 1, 2, 16, 0, 0, 0, 0) X(64, 0, 2, 2, 16, 0, 0, 0, 0) \
    X(64, 0, 1, 2,  4, 0, 0, 0, 0) X(64, 0, 1, 2, 16, 0, 0, 0, 0) X(16, 1, 2, 1, 16, 0, 1, 1, 0) \
    X(16, 1, 1, 1,  4, 1, 1, 1, 0) X(16, 1, 1, 1,  4, 1, 1, 1, 1) X(16, 1, 1, 1,  4, 1, 1, 2, 0) \
    X(16, 1, 1, 1,  4, 1, 1, 2, 1) X(16, 1, 1, 1,  4, 1, 1, 0, 0) X(16, 1, 1, 1,  4, 1, 1, 0, 1) \
    X(16, 1, 1, 1,  4, 2, 1, 1, 0) X(16, 1, 1, 1,  4, 2, 1, 1, 1) X(16, 1, 1, 1,  4, 2, 1, 2, 0) \
    X(16, 1, 1, 1,  4, 2, 1, 2, 1) X(16, 1, 1, 1,  4, 2, 1, 0, 0) X(16, 1, 1, 1,  4, 2, 1, 0, 1) \
    X(16, 1, 1, 1,  4, 4, 1, 1, 0) X(16, 1, 1, 1,  4, 4, 1, 1, 1) X(16, 1, 1, 1,  4, 4, 1, 2, 0) \
    X(16, 1, 1, 1,  4, 4, 1, 2, 1) X(16, 1, 1, 1,  4, 4, 1, 0, 0) X(16, 1, 1, 1,  4, 4, 1, 0, 1) \
    X(16, 1, 1, 1, 16, 0, 1, 1, 0) X(16, 1, 1, 1, 16, 0, 1, 1, 1) X(16, 1, 1, 1, 16, 0, 1, 2, 0) \
    X(16, 1, 1, 1, 16, 0, 1, 2, 1) X(16, 1, 1, 1, 16, 0, 1, 0, 0) X(16, 1, 1, 1, 16, 0, 1, 0, 1) \
    X(16, 0, 2, 1, 16, 0, 1, 0, 0) X(16, 0, 1, 1,  4, 0, 1, 0, 0) X(16, 0, 1, 1,  4, 0, 1, 0, 1) \
    X(16, 0, 1, 1, 16, 0, 1, 0, 0) X(16, 0, 1, 1, 16, 0, 1, 0, 1) X(32, 1, 2, 1, 16, 0, 1, 1, 0) \
    X(32, 1, 1, 1,  4, 1, 1, 1, 0) X(32, 1, 1, 1,  4, 1, 1, 1, 1) X(32, 1, 1, 1,  4, 1, 1, 2, 0) \
    X(32, 1, 1, 1,  4, 1, 1, 2, 1) X(32, 1, 1, 1,  4, 1, 1, 0, 0) X(32, 1, 1, 1,  4, 1, 1, 0, 1) \
    X(32, 1, 1, 1,  4, 2, 1, 1, 0) X(32, 1, 1, 1,  4, 2, 1, 1, 1) X(32, 1, 1, 1,  4, 2, 1, 2, 0) \
    X(32, 1, 1, 1,  4, 2, 1, 2, 1) X(32, 1, 1, 1,  4, 2, 1, 0, 0) X(32, 1, 1, 1,  4, 2, 1, 0, 1) \
    X(32, 1, 1, 1,  4, 4, 1, 1, 0) X(32, 1, 1, 1,  4, 4, 1, 1, 1) X(32, 1, 1, 1,  4, 4, 1, 2, 0) \
    X(32, 1, 1, 1,  4, 4, 1, 2, 1) X(32, 1, 1, 1,  4, 4, 1, 0, 0) X(32, 1, 1, 1,  4, 4, 1, 0, 1) \
    X(32, 1, 1, 1, 16, 0, 1, 1, 0) X(32, 1, 1, 1, 16, 0, 1, 1, 1) X(32, 1, 1, 1, 16, 0, 1, 2, 0) \
    X(32, 1, 1, 1, 16, 0, 1, 2, 1) X(32, 1, 1, 1, 16, 0, 1, 0, 0) X(32, 1, 1, 1, 16, 0, 1, 0, 1) \
    X(32, 0, 2, 1, 16, 0, 1, 0, 0) X(32, 0, 1, 1,  4, 0, 1, 0, 0) X(32, 0, 1, 1,  4, 0, 1, 0, 1) \
    X(32, 0, 1, 1, 16, 0, 1, 0, 0) X(32, 0, 1, 1, 16, 0, 1, 0, 1) X(64, 1, 2, 1, 16, 0, 1, 0, 0) \
    X(64, 1, 1, 1,  4, 1, 1, 0, 0) X(64, 1, 1, 1,  4, 1, 1, 0, 1) X(64, 1, 1, 1,  4, 2, 1, 0, 0) \
    X(64, 1, 1, 1,  4, 2, 1, 0, 1) X(64, 1, 1, 1,  4, 4, 1, 0, 0) X(64, 1, 1, 1,  4, 4, 1, 0, 1) \
    X(64, 1, 1, 1, 16, 0, 1, 0, 0) X(64, 1, 1, 1, 16, 0, 1, 0, 1) X(64, 0, 2, 1, 16, 0, 1, 0, 0) \
    X(64, 0, 1, 1,  4, 0, 1, 0, 0) X(64, 0, 1, 1,  4, 0, 1, 0, 1) X(64, 0, 1, 1, 16, 0, 1, 0, 0) \
    X(64, 0, 1, 1, 16, 0, 1, 0, 1)
// The wide kernel: V, NP, CAP, KMX, TOP -- both tiers, each with either load width and plane
// count (one graph of n <= 1024 and 256 < d <= 512 has two planes at any k).
#define GLL_SELW_VARIANTS(X)                                                                     \
    X(1, 1, 256, kMaxKm1Wide, 4) X(1, 2, 256, kMaxKm1Wide, 4) X(0, 1, 256, kMaxKm1Wide, 4)       \
    X(0, 2, 256, kMaxKm1Wide, 4) X(1, 1, 512, kMaxKm1Huge, 5) X(1, 2, 512, kMaxKm1Huge, 5)       \
    X(0, 1, 512, kMaxKm1Huge, 5) X(0, 2, 512, kMaxKm1Huge, 5)

using SelFn = decltype(&knn_select_kernel<16, true, 1, 2, 16>);
using SelWideFn = decltype(&knn_select_wide_kernel<true, 1, 256, kMaxKm1Wide, 4>);
struct SelRow {
    SelVariant v;
    SelFn fn;
};
struct SelWideRow {
    SelWideVariant w;
    SelWideFn fn;
};
#define GLL_SEL_ROW(KC, V, NP, PG, NU, XQ, R, CH, H)                                             \
    {{KC, V, NP, PG, NU, XQ, R, CH, H},                                                          \
     knn_select_kernel<KC, V != 0, NP, PG, NU, XQ, R != 0, CH, H != 0>},
#define GLL_SELW_ROW(V, NP, CAP, KMX, TOP)                                                       \
    {{V, NP, CAP, KMX, TOP}, knn_select_wide_kernel<V != 0, NP, CAP, KMX, TOP>},
static constexpr SelRow kSelTable[] = {GLL_SEL_VARIANTS(GLL_SEL_ROW)};
static constexpr SelWideRow kSelWideTable[] = {GLL_SELW_VARIANTS(GLL_SELW_ROW)};
#undef GLL_SEL_ROW
#undef GLL_SELW_ROW
constexpr int kSelRows = int(sizeof(kSelTable) / sizeof(kSelTable[0]));
constexpr int kSelWideRows = int(sizeof(kSelWideTable) / sizeof(kSelWideTable[0]));

int select_table_rows() { return kSelRows + kSelWideRows; }

int select_table_index(const SelRoute& rt) {
    if (rt.wide) {
        for (int q = 0; q < kSelWideRows; ++q)
            if (kSelWideTable[q].w == rt.w) return kSelRows + q;
    } else {
        for (int q = 0; q < kSelRows; ++q)
            if (kSelTable[q].v == rt.v) return q;
    }
    return -1;
}

hipError_t launch_select(const Layout& L, const Batch& bt, void* ws, const float* X,
                         float eps_fixed, bool auto_eps, bool vec, int32_t* status_pub,
                         hipStream_t s, int r0, int rows) {
    if (rows < 0) rows = L.n - r0;
    const int n = L.n, K = L.K;
    if (K - 1 > kMaxKm1Huge) return hipErrorInvalidValue;
    const SelRoute rt = select_route(L, bt, vec, r0, rows);
    if (rt.wide && d2_half(L, bt)) return hipErrorInvalidValue;   // d2_half keeps fp32 rows for it
    const int row = select_table_index(rt);
    if (row < 0) {
        if (debug_log())
            fprintf(stderr, "gll: select.hip:launch_select: variant not instantiated (n %d d %d K %d "
                            "B %d rows %d vec %d)\n", n, L.d, K, bt.B, rows, int(vec));
        return hipErrorInvalidValue;
    }
    const size_t plane = size_t(n) * L.ldD;
    dim3 grid((rows + 3) / 4, bt.B);
    const int32_t* perm = (locality_order(L, bt) && r0 == 0 && rows == n)
                              ? L.at<int32_t>(ws, L.perm) : nullptr;
    if (rt.wide) {   // k past one candidate per lane: LDS lists (knn_select_wide_kernel)
        const int kcw = min(K - 1 + 8, n - 1);
        prof_begin(GLL_K_SELECT, s);
        launch_k(kSelWideTable[row - kSelRows].fn, grid, 256, 0, s, L.at<float>(ws, L.D2), L.ldD,
                 plane, X, n, L.d, K, kcw, eps_fixed, auto_eps ? 1 : 0, L.RCAP,
                 L.at<int32_t>(ws, L.knn_idx), L.at<float>(ws, L.knn_d2), L.at<float>(ws, L.eps),
                 L.at<int32_t>(ws, L.rev_cnt), L.at<int32_t>(ws, L.rev_idx),
                 L.at<float>(ws, L.rev_d2), L.at<int32_t>(ws, L.ovf), L.at<int32_t>(ws, L.status),
                 status_pub, bt.x, bt.ws, bt.st, r0, r0 + rows, perm);
        prof_end(GLL_K_SELECT, s);
        return launch_status("select.hip:launch_select(wide)");
    }
    // re-rank margin of the candidate list: up to 8 past the K - 1 kept
    int margin = rt.v.KC - (K - 1);
    if (margin > 8) margin = 8;
    int kc = K - 1 + margin;
    if (kc > n - 1) kc = n - 1;
    const float* d2s = L.at<float>(ws, L.d2s);
    prof_begin(GLL_K_SELECT, s);
    launch_k(kSelTable[row].fn, grid, 256, 0, s, L.at<float>(ws, L.D2), L.ldD, plane, X, n, L.d, K,
             kc, eps_fixed, auto_eps ? 1 : 0, L.RCAP, L.at<int32_t>(ws, L.knn_idx),
             L.at<float>(ws, L.knn_d2), L.at<float>(ws, L.eps), L.at<int32_t>(ws, L.rev_cnt),
             L.at<int32_t>(ws, L.rev_idx), L.at<float>(ws, L.rev_d2), L.at<int32_t>(ws, L.ovf),
             L.at<int32_t>(ws, L.status), status_pub, bt.x, bt.ws, bt.st, r0, r0 + rows, d2s,
             perm);
    prof_end(GLL_K_SELECT, s);
    return launch_status("select.hip:launch_select");
}

}  // namespace gll
