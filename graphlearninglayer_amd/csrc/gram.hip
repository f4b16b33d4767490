// gram.hip -- the nominating distances of the exact brute-force kNN for the GLL graph (which
// replaces the annoy search of graphlearning.weightmatrix.knnsearch, /root/reference/GLL.py:183).
//
//  K1a gram_bf3*_kernel D2 = |a_i|^2 + |a_j|^2 - 2 <a_i, a_j> on split-bf16 MFMA over the
//                       rows centred on row 0 (a = x - x_0: distance-invariant, and it keeps
//                       the product error proportional to the spread of the rows, not to
//                       their offset), upper-triangle tiles only (mirrored writes).  D2 only
//                       NOMINATES candidates; select.hip (K1b) re-ranks them exactly.
// Which kernel a problem takes: launch_gram below and the predicates of knn_route.h.
#include "knn_route.h"

namespace gll {

GLL_TRACE_UNIT(knn)

// --------------------------------------------------------------------------------------
// K1a (default): split-bf16 Gram on v_mfma_f32_32x32x16_bf16.  Each fp32 feature is split as
// x = hi + lo with hi = bf16(x), lo = bf16(x - hi), and x.y ~ hi.hi + hi.lo + lo.hi: three
// bf16 MFMAs at 16x the fp32 MFMA rate (5.3x fewer MFMA cycles than v_mfma_f32_32x32x2_f32).
// The dropped terms are <= 2^-16 |x_k y_k| each (~1e-6 on the d^2 of unit rows at d = 512,
// against ~1e-7 for fp32); D2 only nominates the K-1+margin candidates that the select
// kernel re-ranks with exact fp32 difference-form distances, so the kNN result keeps the
// fp32 exactness contract.  Row norms come from the fp32 values.
//
// 64 x 64 tile per workgroup (upper triangle, mirrored writes), 16 waves.  What bounds a
// tile at small n is how fast one CU pulls its 2 x 64 rows (256 KiB at d = 512) out of L2,
// which needs many loads in flight: tools/csrc/load_probe.hip measured 6.9 us for the tile
// loads with 4 waves x 2 chunks in flight and 4.0 us with 16 waves x 1 chunk.  So:
//   - features go in phases of 256; in a phase wave w loads rows 16s + w (s = 0..7) of the
//     128 tile rows (0..63 = rows bi*64.., 64..127 = rows bj*64..), one 1 KiB row segment
//     per wave instruction (whole lines); two phases of loads are in flight per wave;
//   - each phase is split into hi / lo bf16 planes in LDS (2 x 128 x 256, row stride 264
//     bf16: conflict-free ds_read_b128 fragment reads), one barrier, then wave (qd, kq)
//     multiplies quadrant qd of the tile over feature quarter kq of the phase (4 k-steps x 3
//     MFMAs into one 32 x 32 accumulator);
//   - the 4 feature-quarter partials of each quadrant are summed in LDS in a fixed order.
// --------------------------------------------------------------------------------------
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));

// ---- blocks the inline-split kernels (gram_bf3, bf3h, bf3s, bf3w) share ----
// Graph g's X, D2 and counters (the branching shift: gll_internal.h gshift_br).
__device__ __forceinline__ void shift_to_graph(const float* __restrict__& X, float* __restrict__& D2,
                                               int32_t* __restrict__& status,
                                               int32_t* __restrict__& rev_cnt, size_t xs,
                                               size_t wss) {
    X = gshift_br(X, xs);
    D2 = gshift_br(D2, wss);
    status = gshift_br(status, wss);
    rev_cnt = gshift_br(rev_cnt, wss);
}

// Per-call reset of the counters the select kernel accumulates into, by the first kernel of a
// graph build (NT threads a workgroup).
template <int NT>
__device__ __forceinline__ void reset_call_counters(int32_t* __restrict__ status,
                                                    int32_t* __restrict__ rev_cnt, int n) {
    const int g = bx() * NT + threadIdx.x;
    if (g < kStWords) status[g] = 0;
    for (int q = g; q < n; q += gridDim.x * NT) rev_cnt[q] = 0;
}

// One k-step of 16 features: a.b ~ lo_a.hi_b + hi_a.lo_b + hi_a.hi_b, operands at bf16 offsets
// oa / ob of the hi plane (smem_h) and of the lo plane (smem_h + plane).
__device__ __forceinline__ void mfma3(f32x16& acc, const __bf16* smem_h, int plane, int oa, int ob) {
    const bf16x8 ha = *reinterpret_cast<const bf16x8*>(smem_h + oa);
    const bf16x8 la = *reinterpret_cast<const bf16x8*>(smem_h + plane + oa);
    const bf16x8 hb = *reinterpret_cast<const bf16x8*>(smem_h + ob);
    const bf16x8 lb = *reinterpret_cast<const bf16x8*>(smem_h + plane + ob);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(la, hb, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ha, lb, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ha, hb, acc, 0, 0, 0);
}

// D2 storage of the pre-split path (round 3): fp16 of D2 x s, s = 2^e per graph with every
// D2 <= 4 max|a|^2 mapped below 2^14 (d2_scale), or fp32 (H = false).  D2 only nominates
// candidates; the select decodes x 1/s (exact) and widens its error bounds by the fp16 rounding.
template <bool H>
__device__ __forceinline__ void dput(float* D2, size_t o, float v, float s) {
    if constexpr (H) reinterpret_cast<_Float16*>(D2)[o] = static_cast<_Float16>(v * s);
    else D2[o] = v;
}
template <bool H>
__device__ __forceinline__ void dput4(float* D2, size_t o, f32x4 v, float s) {
    if constexpr (H) {
        const h16x4 hv = {static_cast<_Float16>(v.x * s), static_cast<_Float16>(v.y * s),
                          static_cast<_Float16>(v.z * s), static_cast<_Float16>(v.w * s)};
        *reinterpret_cast<h16x4*>(reinterpret_cast<_Float16*>(D2) + o) = hv;
    } else {
        *reinterpret_cast<f32x4*>(D2 + o) = v;
    }
}
constexpr int kBP = 256;            // features per phase
constexpr int kMaxCen = 4096;       // LDS copy of the centre row: d <= 4096 (gll.h limit)
constexpr int kBS = kBP + 8;        // LDS plane row stride (bf16)

// Epilogue of the 64-tile split-bf16 Gram: row norms (wave sums of the per-slot squares),
// the 4 feature-quarter partials of each quadrant summed in LDS in a fixed order,
// D2 = |a_i|^2 + |b_j|^2 - 2 <a_i, b_j> staged as a [64][65] tile, then the direct and mirrored
// stores (a diagonal tile takes the upper triangle for both halves: D2 bitwise symmetric).
// nrm_of(t) reads norm t (0..63 rows bi, 64..127 rows bj) out of sqp[slot][wave]; Dz, when
// set, receives zeros at the direct positions (the unused plane of a split diagonal tile).
// The full-width stores are non-temporal: D2 is read once, by the select kernel on other XCDs,
// and streaming it out leaves less for the end-of-kernel L2 write-back (NS call 71.4 -> 70.5 us
// over 300 calls, alternating builds, tools/ab_flags.py --lib; on the 128-tile kernel the same
// change measured +0.6% at stress and -1.3% at B = 64, so that one keeps ordinary stores).
// NT = 512 is the half tile (gram_bf3h_kernel): 2 feature halves instead of 4 quarters, and
// 8 tile elements per thread; slot s of wave w holds rows 16 s + 2 w (lanes 0..31) and
// 16 s + 2 w + 1 (lanes 32..63), reduced per half wave.
template <int NT = 1024, typename NF>
__device__ __forceinline__ void bf3_epilogue(const f32x16& acc, const float (&sq)[8], float* smem,
                                             float (*sqp)[16], float* nrm, NF nrm_of, int bi,
                                             int bj, int n, float* __restrict__ D2, int ld,
                                             float* __restrict__ Dz) {
    static_assert(NT == 1024 || NT == 512, "bf3_epilogue: 1024- or 512-thread tiles");
    constexpr int KQ = NT / 256;     // feature groups per quadrant
    constexpr int EP = 4096 / NT;    // tile elements per thread
    constexpr int CPR = 64 / EP;     // threads per tile row
    const int tid = threadIdx.x;
    const int lane = lane_id();
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 31, h = lane >> 5;
    const int qd = w & 3, kq = w >> 2;
    if constexpr (NT == 1024) {
        // row norms: slot s of wave w is tile row 16 s + w, its features spread over the wave
#pragma unroll
        for (int s = 0; s < 8; ++s) {
            const float t = wave_sum_dpp(sq[s]);
            if (lane == 0) sqp[s][w] = t;
        }
    } else {
        // half-wave sums: row sums of 16 lanes, then row_bcast15 carries row 0 into row 1 and
        // row 2 into row 3 (lane 31: lanes 0..31, lane 63: lanes 32..63)
#pragma unroll
        for (int s = 0; s < 8; ++s) {
            float t = dpp_add<0xB1, 0xf>(sq[s]);
            t = dpp_add<0x4E, 0xf>(t);
            t = dpp_add<0x141, 0xf>(t);
            t = dpp_add<0x140, 0xf>(t);
            t = dpp_add<0x142, 0xa>(t);
            if ((lane & 31) == 31) sqp[s][2 * w + h] = t;
        }
    }
    __syncthreads();   // fragment reads done: the planes become partial / tile space
    // partial quadrant -> LDS part[kq][qd][32][33] (C layout: col = lane & 31,
    // row = (e&3) + 8(e>>2) + 4h)
    float* pw = smem + (kq * 4 + qd) * 32 * 33;
#pragma unroll
    for (int e = 0; e < 16; ++e) pw[((e & 3) + 8 * (e >> 2) + 4 * h) * 33 + r] = acc[e];
    if (tid < 128) nrm[tid] = nrm_of(tid);
    __syncthreads();
    // tile element (ti, tj..tj+EP-1): sum of the KQ feature groups, fixed order
    const int ti = tid / CPR, tj = EP * (tid % CPR);
    float v[EP];
    {
        const int q = 2 * (ti >> 5) + (tj >> 5), rr = ti & 31;
#pragma unroll
        for (int e = 0; e < EP; ++e) {
            const int cc = (tj & 31) + e;
            float t = 0.f;
#pragma unroll
            for (int k4 = 0; k4 < KQ; ++k4) t += smem[(k4 * 4 + q) * 32 * 33 + rr * 33 + cc];
            v[e] = t;
        }
    }
    __syncthreads();
    float* tile = smem + KQ * 4 * 32 * 33;   // [64][65], past the partials
#pragma unroll
    for (int e = 0; e < EP; ++e) tile[ti * 65 + tj + e] = nrm[ti] + nrm[64 + tj + e] - 2.f * v[e];
    __syncthreads();
    // direct orientation: row bi*64 + ti, columns bj*64 + tj .. +EP-1; a diagonal tile takes
    // the upper triangle for both halves so D2 stays bitwise symmetric
    const int i = bi * 64 + ti;
    if (i < n) {
#pragma unroll
        for (int c = 0; c < EP; c += 4) {
            float o[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int jj = tj + c + e;
                o[e] = (bi == bj && jj < ti) ? tile[jj * 65 + ti] : tile[ti * 65 + jj];
            }
            const int j0 = bj * 64 + tj + c;
            float* dst = D2 + size_t(i) * ld + j0;
            float* dz = Dz ? Dz + size_t(i) * ld + j0 : nullptr;
            if (j0 + 4 <= n) {
                __builtin_nontemporal_store(f32x4{o[0], o[1], o[2], o[3]}, reinterpret_cast<f32x4*>(dst));
                if (dz) __builtin_nontemporal_store(f32x4{0.f, 0.f, 0.f, 0.f}, reinterpret_cast<f32x4*>(dz));
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (j0 + e < n) {
                        dst[e] = o[e];
                        if (dz) dz[e] = 0.f;
                    }
            }
        }
    }
    // mirrored orientation: row bj*64 + ti, columns bi*64 + tj .. from the tile's column ti
    const int jr = bj * 64 + ti;
    if (bi != bj && jr < n) {
#pragma unroll
        for (int c = 0; c < EP; c += 4) {
            float o[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) o[e] = tile[(tj + c + e) * 65 + ti];
            const int j0 = bi * 64 + tj + c;
            float* dst = D2 + size_t(jr) * ld + j0;
            if (j0 + 4 <= n) {
                __builtin_nontemporal_store(f32x4{o[0], o[1], o[2], o[3]}, reinterpret_cast<f32x4*>(dst));
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (j0 + e < n) dst[e] = o[e];
            }
        }
    }
}

template <bool VEC>
__global__ __launch_bounds__(1024) void gram_bf3_kernel(const float* __restrict__ X, int n, int d,
                                                        int T, float* __restrict__ D2, int ld,
                                                        int32_t* __restrict__ status,
                                                        int32_t* __restrict__ rev_cnt,
                                                        size_t xs, size_t wss) {
    GLL_TRACE_SCOPE(4);
    GLL_TRACE_PT(10);
    shift_to_graph(X, D2, status, rev_cnt, xs, wss);
    // hi plane [128][kBS] then lo plane [128][kBS] (bf16); after the k loop the space holds
    // the partial quadrants [kq][qd][32][33] and then the finished tile [64][65] (floats)
    constexpr int kPlane = 128 * kBS;                                   // bf16 per plane
    __shared__ __attribute__((aligned(16))) __bf16 smem_h[2 * kPlane];
    __shared__ float sqp[8][16];                                        // [slot][wave]
    __shared__ float nrm[128];
    __shared__ __attribute__((aligned(16))) float cen[kMaxCen];          // centre row x_0
    float* smem = reinterpret_cast<float*>(smem_h);
    const int tid = threadIdx.x;
    const int lane = lane_id();
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);   // wave-uniform: scalar row bases
    const int r = lane & 31, h = lane >> 5;
    int bi = 0, rem = xcd_tile(bx(), gridDim.x);
    while (rem >= T - bi) {
        rem -= T - bi;
        ++bi;
    }
    const int bj = bi + rem;
    reset_call_counters<1024>(status, rev_cnt, n);
    const int fo = 4 * lane;   // this lane's 4 features inside a phase
    auto slot_row = [&](int s) {   // row 16 s + w of the 128 tile rows; rows past n clamped
        const int R = 16 * s + w;
        const int row = (R < 64 ? bi * 64 + R : bj * 64 + R - 64);
        return X + size_t(row < n ? row : n - 1) * d;
    };
    const int nph = (d + kBP - 1) / kBP;
    f32x16 acc;
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[e] = 0.f;
    float sq[8];
#pragma unroll
    for (int s = 0; s < 8; ++s) sq[s] = 0.f;
    const int qd = w & 3, kq = w >> 2;              // MFMA role: quadrant, feature quarter
    const int qa = qd >> 1, qb = qd & 1;

    auto gload = [&](int ph, f32x4 (&v)[8]) {
        const int k = ph * kBP + fo;
#pragma unroll
        for (int s = 0; s < 8; ++s) v[s] = load4_raw<VEC>(slot_row(s), k, d);
    };
    auto phase = [&](int ph, const f32x4 (&v)[8]) {
        const int k = ph * kBP + fo;
        __syncthreads();   // the previous phase's fragment reads are done (and cen is staged)
        const f32x4 c = *reinterpret_cast<const f32x4*>(cen + ph * kBP + fo);
#pragma unroll
        for (int s = 0; s < 8; ++s) {
            const f32x4 f = mask4<VEC>(v[s] - c, k, d);
            sq[s] += f.x * f.x + f.y * f.y + f.z * f.z + f.w * f.w;
            bf16x4 hv, lv;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const __bf16 hb = static_cast<__bf16>(f[e]);
                hv[e] = hb;
                lv[e] = static_cast<__bf16>(f[e] - static_cast<float>(hb));
            }
            const int o = (16 * s + w) * kBS + fo;
            *reinterpret_cast<bf16x4*>(smem_h + o) = hv;
            *reinterpret_cast<bf16x4*>(smem_h + kPlane + o) = lv;
        }
        __syncthreads();
#pragma unroll
        for (int st = 0; st < 4; ++st) {
            const int kk = 64 * kq + 16 * st + 8 * h;
            const int oa = (32 * qa + r) * kBS + kk, ob = (64 + 32 * qb + r) * kBS + kk;
            mfma3(acc, smem_h, kPlane, oa, ob);
        }
    };
    {
        // the centre row (row 0 of the graph) into LDS: issued first, so staging it waits for
        // that load only (loads return in order) while the first phase's rows stay in flight
        const f32x4 cv = load4_raw<VEC>(X, 4 * tid, d);
        f32x4 va[8], vb[8];
        gload(0, va);
        if (4 * tid < nph * kBP) *reinterpret_cast<f32x4*>(cen + 4 * tid) = mask4<VEC>(cv, 4 * tid, d);
        for (int ph = 0; ph < nph; ph += 2) {
            gload(ph + 1 < nph ? ph + 1 : ph, vb);   // unconditional: static vmcnt counts
#ifdef GLL_TRACE
            if (ph == 0) {
                asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
                GLL_TRACE_PT(15);
            }
#endif
            phase(ph, va);
            if (ph + 1 >= nph) break;
            gload(ph + 2 < nph ? ph + 2 : ph + 1, va);
            phase(ph + 1, vb);
        }
    }
    GLL_TRACE_PT(12);
    bf3_epilogue(acc, sq, smem, sqp, nrm, [&](int t) { return sqp[t >> 4][t & 15]; }, bi, bj, n,
                 D2, ld, nullptr);
    GLL_TRACE_PT(14);
}

// K1a'' (d <= 128, fewer than 512 64-tiles): the same tile at half the workgroup.  The
// 1024-thread tile stages kBP = 256 features per phase, so at d <= 128 half its loads and half
// its MFMAs run on zero features, and its 151 KiB of LDS holds one workgroup per CU: FullySup's
// 300 tiles (n = 1500) ran as two rounds over 256 CUs.  Here 8 waves (4 quadrants x 2 feature
// halves) stage 128 rows x 128 features in 70 KiB: two workgroups per CU, one round.  Lanes
// 0..31 and 32..63 of a wave hold two rows (512 contiguous bytes each), so the loads stay
// coalesced; the epilogue is bf3_epilogue<512>.
constexpr int kHS = kHP + 8;      // LDS plane row stride (bf16) of the half tile (kHP features)
template <bool VEC>
__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(4)))
void gram_bf3h_kernel(const float* __restrict__ X, int n, int d, int T, float* __restrict__ D2,
                      int ld, int32_t* __restrict__ status, int32_t* __restrict__ rev_cnt,
                      size_t xs, size_t wss) {
    shift_to_graph(X, D2, status, rev_cnt, xs, wss);
    constexpr int kPlane = 128 * kHS;
    static_assert(2 * kPlane * 2 >= (8 * 32 * 33 + 64 * 65) * 4, "half tile: epilogue space");
    __shared__ __attribute__((aligned(16))) __bf16 smem_h[2 * kPlane];
    __shared__ float sqp[8][16];
    __shared__ float nrm[128];
    float* smem = reinterpret_cast<float*>(smem_h);
    const int tid = threadIdx.x;
    const int lane = lane_id();
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 31, h = lane >> 5;
    int bi = 0, rem = xcd_tile(bx(), gridDim.x);
    while (rem >= T - bi) {
        rem -= T - bi;
        ++bi;
    }
    const int bj = bi + rem;
    reset_call_counters<512>(status, rev_cnt, n);
    const int fo = 4 * r;   // this lane's 4 features
    // slot s -> LDS row 16 s + 2 w + h (0..63 rows bi, 64..127 rows bj; rows past n clamped);
    // the centre row's load is issued first
    const f32x4 c = load4_raw<VEC>(X, fo, d);
    f32x4 v[8];
#pragma unroll
    for (int s = 0; s < 8; ++s) {
        const int R = 16 * s + 2 * w + h;
        const int row = R < 64 ? bi * 64 + R : bj * 64 + R - 64;
        v[s] = load4_raw<VEC>(X + size_t(row < n ? row : n - 1) * d, fo, d);
    }
    float sq[8];
#pragma unroll
    for (int s = 0; s < 8; ++s) {
        const f32x4 f = mask4<VEC>(v[s] - c, fo, d);
        sq[s] = f.x * f.x + f.y * f.y + f.z * f.z + f.w * f.w;
        bf16x4 hv, lv;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const __bf16 hb = static_cast<__bf16>(f[e]);
            hv[e] = hb;
            lv[e] = static_cast<__bf16>(f[e] - static_cast<float>(hb));
        }
        const int o = (16 * s + 2 * w + h) * kHS + fo;
        *reinterpret_cast<bf16x4*>(smem_h + o) = hv;
        *reinterpret_cast<bf16x4*>(smem_h + kPlane + o) = lv;
    }
    __syncthreads();
    f32x16 acc;
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[e] = 0.f;
    const int qd = w & 3, kq = w >> 2;   // quadrant, feature half
    const int qa = qd >> 1, qb = qd & 1;
#pragma unroll
    for (int st = 0; st < 4; ++st) {
        const int kk = 64 * kq + 16 * st + 8 * h;
        const int oa = (32 * qa + r) * kHS + kk, ob = (64 + 32 * qb + r) * kHS + kk;
        mfma3(acc, smem_h, kPlane, oa, ob);
    }
    bf3_epilogue<512>(acc, sq, smem, sqp, nrm, [&](int t) { return sqp[t >> 4][t & 15]; }, bi, bj,
                      n, D2, ld, nullptr);
}

// K1a' (one graph, n <= 1024, 256 < d <= 512): the same tile over HALF the features.  With
// T = ceil(n / 64) <= 16 the T (T + 1) / 2 upper-triangle tiles leave CUs idle (136 of 256 at
// NS) while each tile pulls 256 KiB through one CU, and that pull is what bounds the kernel
// (load_probe above).  Here each off-diagonal tile runs as two workgroups -- feature phase 0
// into plane 0, phase 1 into plane 1 -- and each diagonal tile as one workgroup that loads its
// 64 rows once for both phases (LDS rows 0..63: phase 0, rows 64..127: phase 1).  That is T^2
// workgroups with 128 KiB of loads each; the select kernel adds the two planes in a fixed order
// (NP = 2) and a diagonal tile writes zeros into plane 1.  Partial planes carry partial norms,
// |a|^2_s + |b|^2_s - 2 <a, b>_s, so the plane sum is D2.
template <bool VEC>
__global__ __launch_bounds__(1024) void gram_bf3s_kernel(const float* __restrict__ X, int n,
                                                         int d, int T, float* __restrict__ D2,
                                                         int ld, size_t plane,
                                                         int32_t* __restrict__ status,
                                                         int32_t* __restrict__ rev_cnt,
                                                         size_t xs, size_t wss) {
    shift_to_graph(X, D2, status, rev_cnt, xs, wss);
    constexpr int kPlane = 128 * kBS;
    __shared__ __attribute__((aligned(16))) __bf16 smem_h[2 * kPlane];
    __shared__ float sqp[8][16];
    __shared__ float nrm[128];
    float* smem = reinterpret_cast<float*>(smem_h);
    const int tid = threadIdx.x;
    const int lane = lane_id();
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 31, h = lane >> 5;
    const int b = xcd_tile(bx(), gridDim.x);
    const bool dg = b < T;   // block-uniform
    int bi = b, bj = b, half = 0;
    if (!dg) {   // strictly-upper tile (b - T) / 2, row-major; half = feature phase = plane
        int rem = (b - T) >> 1;
        half = (b - T) & 1;
        bi = 0;
        while (rem >= T - 1 - bi) {
            rem -= T - 1 - bi;
            ++bi;
        }
        bj = bi + 1 + rem;
    }
    reset_call_counters<1024>(status, rev_cnt, n);
    const int fo = 4 * lane;
    // slot s -> LDS row 16 s + w.  Off-diagonal: tile row 16 s + w (0..63 rows bi, 64..127
    // rows bj), features of phase `half`.  Diagonal: row bi*64 + 16 (s & 3) + w, phase s >> 2.
    f32x4 v[8];
#pragma unroll
    for (int s = 0; s < 8; ++s) {
        const int R = dg ? 16 * (s & 3) + w : 16 * s + w;
        const int row = R < 64 ? bi * 64 + R : bj * 64 + R - 64;
        const int k = (dg ? (s >> 2) : half) * kBP + fo;
        v[s] = load4_raw<VEC>(X + size_t(row < n ? row : n - 1) * d, k, d);
    }
    // centre row (row 0 of the graph) over the phase(s) this workgroup multiplies
    const f32x4 cen0 = load4_raw<VEC>(X, (dg ? 0 : half) * kBP + fo, d);
    const f32x4 cen1 = load4_raw<VEC>(X, (dg ? 1 : half) * kBP + fo, d);
    float sq[8];
#pragma unroll
    for (int s = 0; s < 8; ++s) {
        const int k = (dg ? (s >> 2) : half) * kBP + fo;
        const f32x4 f = mask4<VEC>(v[s] - (s >= 4 ? cen1 : cen0), k, d);
        sq[s] = f.x * f.x + f.y * f.y + f.z * f.z + f.w * f.w;
        bf16x4 hv, lv;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const __bf16 hb = static_cast<__bf16>(f[e]);
            hv[e] = hb;
            lv[e] = static_cast<__bf16>(f[e] - static_cast<float>(hb));
        }
        const int o = (16 * s + w) * kBS + fo;
        *reinterpret_cast<bf16x4*>(smem_h + o) = hv;
        *reinterpret_cast<bf16x4*>(smem_h + kPlane + o) = lv;
    }
    __syncthreads();
    f32x16 acc;
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[e] = 0.f;
    const int qd = w & 3, kq = w >> 2;
    const int qa = qd >> 1, qb = qd & 1;
#pragma unroll
    for (int st = 0; st < 4; ++st) {
        const int kk = 64 * kq + 16 * st + 8 * h;
        if (dg) {   // both operands from the tile's own rows, phase 0 then phase 1
            mfma3(acc, smem_h, kPlane, (32 * qa + r) * kBS + kk, (32 * qb + r) * kBS + kk);
            mfma3(acc, smem_h, kPlane, (64 + 32 * qa + r) * kBS + kk, (64 + 32 * qb + r) * kBS + kk);
        } else {
            mfma3(acc, smem_h, kPlane, (32 * qa + r) * kBS + kk, (64 + 32 * qb + r) * kBS + kk);
        }
    }
    if (dg)   // norm of row t: its phase-0 slot plus its phase-1 slot, both halves the same rows
        bf3_epilogue(acc, sq, smem, sqp, nrm,
                     [&](int t) {
                         const int u = t & 63;
                         return sqp[u >> 4][u & 15] + sqp[(u >> 4) + 4][u & 15];
                     },
                     bi, bj, n, D2, ld, D2 + plane);
    else
        bf3_epilogue(acc, sq, smem, sqp, nrm, [&](int t) { return sqp[t >> 4][t & 15]; }, bi, bj,
                     n, D2 + size_t(half) * plane, ld, nullptr);
}

// --------------------------------------------------------------------------------------
// K1a (large problems and batches): split-bf16 Gram on 128 x 128 tiles.  With many tiles the
// kernel is bound by the tile rows every CU pulls out of L2 (2 x 64 rows per 64-tile: 4.3 GB
// at stress); a 128-tile halves those bytes per output.  16 waves, wave w owns the 32 x 32
// sub-tile (w >> 2, w & 3) over the WHOLE feature range, so there is no cross-wave reduction.
// Features go in phases of 128: thread t loads 4 features of row 32 s + (t >> 5) of the 256
// tile rows (0..127 = rows bi*128.., 128..255 = rows bj*128..) for slot s = 0..7 -- half a
// wave per 512-B row segment -- and splits them into hi / lo bf16 planes in LDS (row stride
// 136 bf16: conflict-free ds_read_b128); one barrier, then 8 k-steps x 3 MFMAs per wave.
// Off-diagonal tiles store straight from the accumulators in both orientations; diagonal
// tiles go through LDS so D2 stays bitwise symmetric (upper triangle mirrored).
// --------------------------------------------------------------------------------------
constexpr int kWP = 128;            // features per phase
constexpr int kWS = kWP + 8;        // LDS plane row stride (bf16)

template <bool VEC>
__global__ __launch_bounds__(1024) void gram_bf3w_kernel(const float* __restrict__ X, int n,
                                                         int d, int T, float* __restrict__ D2,
                                                         int ld, int32_t* __restrict__ status,
                                                         int32_t* __restrict__ rev_cnt,
                                                         size_t xs, size_t wss, int r0,
                                                         int pt) {
    // pt > 0 (a row panel, build_graph): rectangular tiles of rows r0 .. r0 + 128 pt against
    // every column block, stored in the direct orientation only into the panel's rows of D2
    shift_to_graph(X, D2, status, rev_cnt, xs, wss);
    constexpr int kPlane = 256 * kWS;                                   // bf16 per plane
    __shared__ __attribute__((aligned(16))) __bf16 smem_h[2 * kPlane];  // 136 KiB
    __shared__ float nrm[256];
    __shared__ __attribute__((aligned(16))) float cen[kMaxCen];          // centre row x_0
    float* smem = reinterpret_cast<float*>(smem_h);
    const int tid = threadIdx.x;
    const int lane = lane_id();
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 31, h = lane >> 5;
    int bi = 0, rem = xcd_tile(bx(), gridDim.x), bj;
    if (pt > 0) {
        bi = (r0 >> 7) + rem / T;
        bj = rem % T;
    } else {
        while (rem >= T - bi) {
            rem -= T - bi;
            ++bi;
        }
        bj = bi + rem;
    }
    if (r0 == 0) reset_call_counters<1024>(status, rev_cnt, n);
    const int fo = 4 * (tid & 31);       // this thread's 4 features inside a phase
    const int rs = tid >> 5;             // its row inside a slot (0..31)
    auto slot_row = [&](int s) {         // tile row 32 s + rs; rows past n clamped
        const int R = 32 * s + rs;
        const int row = (R < 128 ? bi * 128 + R : bj * 128 + R - 128);
        return X + size_t(row < n ? row : n - 1) * d;
    };
    const int nph = (d + kWP - 1) / kWP;
    const int sa = w >> 2, sb = w & 3;   // this wave's 32 x 32 sub-tile
    f32x16 acc;
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[e] = 0.f;
    // row norms: slot q's half-wave sum is kept by lane q of that half-wave (one register)
    float sq = 0.f;

    auto gload = [&](int ph, f32x4 (&v)[8]) {
        const int k = ph * kWP + fo;
#pragma unroll
        for (int q = 0; q < 8; ++q) v[q] = load4_raw<VEC>(slot_row(q), k, d);
    };
    auto phase = [&](int ph, const f32x4 (&v)[8]) {
        const int k = ph * kWP + fo;
        __syncthreads();   // the previous phase's fragment reads are done (and cen is staged)
        const f32x4 c = *reinterpret_cast<const f32x4*>(cen + ph * kWP + fo);
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const f32x4 f = mask4<VEC>(v[q] - c, k, d);
            float t = f.x * f.x + f.y * f.y + f.z * f.z + f.w * f.w;
            t = dpp_add<0xB1, 0xf>(t);    // quad
            t = dpp_add<0x4E, 0xf>(t);
            t = dpp_add<0x141, 0xf>(t);   // half row (8)
            t = dpp_add<0x140, 0xf>(t);   // row (16)
            t += __shfl_xor(t, 16);       // the 32 lanes of the row segment
            sq += (lane & 31) == q ? t : 0.f;
            bf16x4 hv, lv;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const __bf16 hb = static_cast<__bf16>(f[e]);
                hv[e] = hb;
                lv[e] = static_cast<__bf16>(f[e] - static_cast<float>(hb));
            }
            const int o = (32 * q + rs) * kWS + fo;
            *reinterpret_cast<bf16x4*>(smem_h + o) = hv;
            *reinterpret_cast<bf16x4*>(smem_h + kPlane + o) = lv;
        }
        __syncthreads();
#pragma unroll
        for (int st = 0; st < kWP / 16; ++st) {
            const int kk = 16 * st + 8 * h;
            const int oa = (32 * sa + r) * kWS + kk, ob = (128 + 32 * sb + r) * kWS + kk;
            mfma3(acc, smem_h, kPlane, oa, ob);
        }
    };
    {
        const f32x4 cv = load4_raw<VEC>(X, 4 * tid, d);   // centre row x_0 -> LDS (see gram_bf3)
        f32x4 va[8], vb[8];
        gload(0, va);
        if (4 * tid < nph * kWP) *reinterpret_cast<f32x4*>(cen + 4 * tid) = mask4<VEC>(cv, 4 * tid, d);
        for (int ph = 0; ph < nph; ph += 2) {
            gload(ph + 1 < nph ? ph + 1 : ph, vb);   // unconditional: static vmcnt counts
            phase(ph, va);
            if (ph + 1 >= nph) break;
            gload(ph + 2 < nph ? ph + 2 : ph + 1, va);
            phase(ph + 1, vb);
        }
    }
    if ((lane & 31) < 8) nrm[32 * (lane & 31) + rs] = sq;   // tile row 32 q + rs, q = lane
    __syncthreads();   // norms visible; fragment reads done (the planes may be reused)
    // C layout of 32x32: col = lane & 31, row = (e&3) + 8(e>>2) + 4h
    const int i0 = bi * 128 + 32 * sa, j0 = bj * 128 + 32 * sb;
    float dv[16];
#pragma unroll
    for (int e = 0; e < 16; ++e) {
        const int rr = (e & 3) + 8 * (e >> 2) + 4 * h;
        dv[e] = nrm[32 * sa + rr] + nrm[128 + 32 * sb + r] - 2.f * acc[e];
    }
    if (pt > 0) {   // panel: every tile in the direct orientation, rows relative to r0
        const int j = j0 + r;
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int i = i0 + (e & 3) + 8 * (e >> 2) + 4 * h;
            if (i < n && j < n) D2[size_t(i - r0) * ld + j] = dv[e];
        }
    } else if (bi != bj) {
        // direct orientation: element e is (i0 + rr, j0 + r) -- 32 lanes per 128-B row piece
        const int j = j0 + r;
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int i = i0 + (e & 3) + 8 * (e >> 2) + 4 * h;
            if (i < n && j < n) D2[size_t(i) * ld + j] = dv[e];
        }
        // mirrored: row j0 + r, columns i0 + 8 g + 4 h .. +3 are registers 4 g .. 4 g + 3
        if (j < n) {
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int i = i0 + 8 * g + 4 * h;
                float* dst = D2 + size_t(j) * ld + i;
                if (i + 4 <= n) {
                    *reinterpret_cast<f32x4*>(dst) =
                        f32x4{dv[4 * g], dv[4 * g + 1], dv[4 * g + 2], dv[4 * g + 3]};
                } else {
#pragma unroll
                    for (int t = 0; t < 4; ++t)
                        if (i + t < n) dst[t] = dv[4 * g + t];
                }
            }
        }
    } else {
        // diagonal tile: stage [128][129] in LDS, store the upper triangle in both orientations
        float* tile = smem;
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int rr = 32 * sa + (e & 3) + 8 * (e >> 2) + 4 * h;
            tile[rr * 129 + 32 * sb + r] = dv[e];
        }
        __syncthreads();
        for (int q = tid; q < 128 * 128; q += 1024) {
            const int ti = q >> 7, tj = q & 127;
            const int i = bi * 128 + ti, j = bi * 128 + tj;
            if (i < n && j < n) D2[size_t(i) * ld + j] = tj >= ti ? tile[ti * 129 + tj] : tile[tj * 129 + ti];
        }
    }
}

// --------------------------------------------------------------------------------------
// K1a (large problems and batches, round 2): the split done once per row, then a bf16 GEMM.
//
// gram_split_kernel: a_i = x_i - x_0 (centred on row 0 as above), hi = bf16(a), lo = bf16(a -
// hi) into two [n][dp] bf16 planes (dp = d rounded up to 64, zero-padded) and |a_i|^2 (fp32)
// into nrm[n]: one pass over X.  gram_bf3w_kernel redid this split for every tile a row takes
// part in (T times), on the VALU between two barriers per 128-feature phase.
//
// gram_pk_kernel: 128 x 128 upper-triangle tiles (same tile list and XCD order as bf3w), 4
// waves of 64 x 64 (2 x 2 accumulators of 32 x 32), k-stages of 64 features: the four tile
// planes (A hi, A lo, B hi, B lo; 64 KiB) go global -> LDS by LDS-DMA
// (global_load_lds_dwordx4, no VGPR staging, no conversion), double-buffered so stage k+1's
// loads are in flight while stage k's 48 MFMAs per wave run.  Rows are 128 B in LDS with the
// 16-B segments XOR-swizzled by (row >> 1) & 7 -- on the SOURCE address, the DMA writes
// lane-linearly -- so the ds_read_b128 fragment reads of 16 consecutive rows hit 16 distinct
// bank groups.  One raw s_barrier per stage; the next stage's DMAs are issued between the
// current stage's MFMA groups.
// --------------------------------------------------------------------------------------
// fp16 D2 scale of a graph with M = max |a_i|^2: s = 2^(14 - e) with 4M < 2^e, so every
// stored D2 x s stays below 2^14 (fp16 max 65504); 1 for an all-zero or non-finite graph.
__device__ __forceinline__ float d2_scale(float M) {
    const float t = 4.f * M;
    if (!(t > 1e-30f) || !(t < 1e38f)) return 1.f;
    int e;
    (void)frexpf(t, &e);   // t = f 2^e, f in [0.5, 1)
    int k = 14 - e;
    k = k < -120 ? -120 : (k > 120 ? 120 : k);
    return ldexpf(1.f, k);
}

// Block-wide max of nrm[0 .. n) (the graph's |a_i|^2 from gram_split) -> the fp16 scale; every
// tile of the GEMM computes the same value from the same array, and each stores it to the
// graph's scale word for the select: identical plain stores, no atomics, nothing to reset.
template <int NT>
__device__ __forceinline__ float tile_d2_scale(const float* __restrict__ nrm, int n, float* red) {
    float mx = 0.f;
    for (int q = threadIdx.x; q < n; q += NT) mx = fmaxf(mx, nrm[q]);   // NaN: dropped
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) mx = fmaxf(mx, __shfl_xor(mx, off));
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = mx;
    __syncthreads();
    mx = 0.f;
#pragma unroll
    for (int w = 0; w < NT / 64; ++w) mx = fmaxf(mx, red[w]);
    return d2_scale(mx);
}

template <bool VEC>
__global__ __launch_bounds__(256) void gram_split_kernel(const float* __restrict__ X, int n, int d,
                                                         int dp, __bf16* __restrict__ Ph,
                                                         __bf16* __restrict__ Pl,
                                                         float* __restrict__ nrm,
                                                         int32_t* __restrict__ status,
                                                         int32_t* __restrict__ rev_cnt,
                                                         size_t xs, size_t wss) {
    X = gshift_br(X, xs);
    Ph = gshift_br(Ph, wss);
    Pl = gshift_br(Pl, wss);
    nrm = gshift_br(nrm, wss);
    status = gshift_br(status, wss);
    rev_cnt = gshift_br(rev_cnt, wss);
    reset_call_counters<256>(status, rev_cnt, n);
    const int lane = lane_id();
    const int i = bx() * 4 + (threadIdx.x >> 6);
    if (i >= n) return;
    const float* xi = X + size_t(i) * d;
    float sq = 0.f;
    for (int k = 4 * lane; k < dp; k += 4 * kWave) {
        const f32x4 c = load4<VEC>(X, k, d);
        const f32x4 f = load4<VEC>(xi, k, d) - c;   // zeros past d
        sq += f.x * f.x + f.y * f.y + f.z * f.z + f.w * f.w;
        bf16x4 hv, lv;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const __bf16 hb = static_cast<__bf16>(f[e]);
            hv[e] = hb;
            lv[e] = static_cast<__bf16>(f[e] - static_cast<float>(hb));
        }
        *reinterpret_cast<bf16x4*>(Ph + size_t(i) * dp + k) = hv;
        *reinterpret_cast<bf16x4*>(Pl + size_t(i) * dp + k) = lv;
    }
    sq = wave_sum_dpp(sq);
    if (lane == 0) nrm[i] = sq;
}

// Tile t of the upper triangle of T x T blocks in supertile order: supertiles of kSR x kSC
// blocks, row-major, each walked row-major.  With the XCD-contiguous deal of xcd_tile, the ~32
// tiles an XCD runs at once come from one or two supertiles, whose kSR + kSC row blocks
// (512 KB each at d = 1024) mostly stay in that XCD's 4 MB L2, instead of a row-major run whose
// 32 column blocks are streamed from the MALL once per tile.
constexpr int kSR = 4, kSC = 8;
__device__ __forceinline__ void supertile_tile(int t, int T, int& bi, int& bj) {
    for (int I = 0; I * kSR < T; ++I) {
        for (int J = (I * kSR) / kSC; J * kSC < T; ++J) {
            int cnt = 0;
#pragma unroll
            for (int a = 0; a < kSR; ++a) {
                const int r = I * kSR + a;
                const int lo = max(r, J * kSC), hi = min(T, J * kSC + kSC);
                cnt += r < T && hi > lo ? hi - lo : 0;
            }
            if (t < cnt) {
                for (int a = 0; a < kSR; ++a) {
                    const int r = I * kSR + a;
                    const int lo = max(r, J * kSC), hi = min(T, J * kSC + kSC);
                    const int c = r < T && hi > lo ? hi - lo : 0;
                    if (t < c) {
                        bi = r;
                        bj = lo + t;
                        return;
                    }
                    t -= c;
                }
            }
            t -= cnt;
        }
    }
    bi = bj = 0;   // not reached for t < T (T + 1) / 2
}

// One-dimensional grid over B graphs x T (T + 1) / 2 tiles: xcd_tile deals each XCD a
// contiguous run of the graph-major sequence, so a batch's graphs are XCD-local too.
// t0 >= 0 (the tail of a 256-tile launch, launch_gram): with Q = 256 / TS, block Q^2 j + s
// computes TS-subtile s of 256-tile t0 + j in gram_pk2_kernel's sequence (T2 = ceil(T / Q)
// blocks a side, T counted in TS-tiles); subtiles below a diagonal 256-tile's diagonal or past
// n return at once.  TS = 64 (round 6): the tail's 16 256-tiles at stress become 256 workgroups,
// one per CU, instead of 64 128-subtiles on a quarter of the chip; each wave then holds one
// 32 x 32 accumulator.  Every element still sums the same MFMA sequence over k: D2 is bitwise
// the same for any TS.
template <bool H, int TS>
__global__ __launch_bounds__(256) void gram_pk_kernel(const __bf16* __restrict__ Ph,
                                                      const __bf16* __restrict__ Pl,
                                                      const float* __restrict__ nrm, int n,
                                                      int dp, int T, float* __restrict__ D2,
                                                      int ld, size_t wss,
                                                      float* __restrict__ d2s, int t0) {
    const int nks = dp / kPK;
    int g, bi, bj;
    if (t0 < 0) {
        const int NT = T * (T + 1) / 2;
        const int idx = xcd_tile(blockIdx.x, gridDim.x);
        g = idx / NT;
        supertile_tile(idx - g * NT, T, bi, bj);
    } else {
        constexpr int Q = 256 / TS;
        const int T2 = (T + Q - 1) / Q, NT2 = T2 * (T2 + 1) / 2;
        const int idx2 = t0 + int(blockIdx.x) / (Q * Q), sub = int(blockIdx.x) % (Q * Q);
        int b2i, b2j;
        g = idx2 / NT2;
        supertile_tile(idx2 - g * NT2, T2, b2i, b2j);
        bi = Q * b2i + sub / Q;
        bj = Q * b2j + sub % Q;
        if (bi > bj || bj >= T) return;   // whole workgroup, before any barrier
    }
    {
        const size_t off = size_t(g) * wss;   // graph g's workspace block
        Ph = reinterpret_cast<const __bf16*>(reinterpret_cast<const char*>(Ph) + off);
        Pl = reinterpret_cast<const __bf16*>(reinterpret_cast<const char*>(Pl) + off);
        nrm = reinterpret_cast<const float*>(reinterpret_cast<const char*>(nrm) + off);
        D2 = reinterpret_cast<float*>(reinterpret_cast<char*>(D2) + off);
        d2s = reinterpret_cast<float*>(reinterpret_cast<char*>(d2s) + off);
    }
    static_assert(TS == 128 || TS == 64, "128- or 64-row tiles");
    constexpr int MA = TS / 64;                // 32 x 32 accumulators a side per wave
    constexpr int RG = TS / 32;                // 32-row DMA groups per plane
    constexpr int NQ = 4 * RG;                 // DMA pieces per stage (4 planes)
    constexpr int kTP = TS * kPK;                                   // bf16 per tile plane
    __shared__ __attribute__((aligned(16))) __bf16 sm[2 * 4 * kTP];  // TS KiB: [buf][plane]
    const int lane = lane_id();
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int r = lane & 31, h = lane >> 5;
    const int wr = w >> 1, wc = w & 1;
    // this lane's DMA sources: NQ per stage = plane q / RG, rows 8 c .. 8 c + 7 (c = (q % RG) 4
    // + w) as 1 KiB pieces; lane -> row 8 c + lane / 8, LDS segment lane % 8 <- source segment
    // (lane % 8) ^ ((row >> 1) & 7)
    const __bf16* src[16];   // NQ used (a dependent bound here drops the host-side kernel stub)
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
        const int pl = q / RG, c = (q % RG) * 4 + w;
        const int row = 8 * c + (lane >> 3);
        const int seg = (lane & 7) ^ ((row >> 1) & 7);
        int grow = (pl < 2 ? bi : bj) * TS + row;
        grow = grow < n ? grow : n - 1;
        src[q] = ((pl & 1) ? Pl : Ph) + size_t(grow) * dp + 8 * seg;
    }
    // DMAs of stage ks into buffer buf, pieces [q0, q0 + NQ / 4)
    auto issue4 = [&](int ks, int buf, int q0) {
#pragma unroll
        for (int q = q0; q < q0 + NQ / 4; ++q) {
            const int pl = q / RG, c = (q % RG) * 4 + w;
            __bf16* dst = sm + (buf * 4 + pl) * kTP + c * 8 * kPK;
            __builtin_amdgcn_global_load_lds(src[q] + ks * kPK, (lds_void*)dst, 16, 0, 0);
        }
    };
    f32x16 acc[MA][MA];
#pragma unroll
    for (int a = 0; a < MA; ++a)
#pragma unroll
        for (int b = 0; b < MA; ++b)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[a][b][e] = 0.f;
    auto frag = [&](int buf, int pl, int row, int kk) {
        const int pos = (2 * kk + h) ^ ((row >> 1) & 7);
        return *reinterpret_cast<const bf16x8*>(sm + (buf * 4 + pl) * kTP + row * kPK + 8 * pos);
    };
    // One wave per SIMD: the next stage's 16 DMAs are issued in four groups between this
    // stage's MFMA groups, so their issue overlaps the MFMA pipe.  One barrier per stage: it
    // orders stage ks's DMAs (each wave drained its own with vmcnt(0) first) before any
    // fragment read, and every wave's reads of the buffer the next DMAs overwrite (stage ks-1's)
    // before those DMAs are issued.
#pragma unroll
    for (int q0 = 0; q0 < NQ; q0 += NQ / 4) issue4(0, 0, q0);
    float dsc = 1.f;   // fp16 D2 scale (H), computed under the first stage's DMAs
    if constexpr (H) {
        __shared__ float red[4];
        dsc = tile_d2_scale<256>(nrm, n, red);
        if (threadIdx.x == 0) *d2s = dsc;
    }
    for (int ks = 0; ks < nks; ++ks) {
        const int buf = ks & 1;
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");       // this wave's stage-ks DMAs
        __builtin_amdgcn_s_barrier();                          // every wave's
        const bool more = ks + 1 < nks;
#pragma unroll
        for (int kk = 0; kk < kPK / 16; ++kk) {
            if (more) issue4(ks + 1, buf ^ 1, (NQ / 4) * kk);
            bf16x8 ah[MA], al[MA], bh[MA], bl[MA];
#pragma unroll
            for (int m = 0; m < MA; ++m) {
                ah[m] = frag(buf, 0, wr * (TS / 2) + m * 32 + r, kk);
                al[m] = frag(buf, 1, wr * (TS / 2) + m * 32 + r, kk);
                bh[m] = frag(buf, 2, wc * (TS / 2) + m * 32 + r, kk);
                bl[m] = frag(buf, 3, wc * (TS / 2) + m * 32 + r, kk);
            }
#pragma unroll
            for (int a = 0; a < MA; ++a)
#pragma unroll
                for (int b = 0; b < MA; ++b) {
                    acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al[a], bh[b], acc[a][b], 0, 0, 0);
                    acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[a], bl[b], acc[a][b], 0, 0, 0);
                    acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[a], bh[b], acc[a][b], 0, 0, 0);
                }
        }
    }
    __syncthreads();   // the last stage's reads are done before the diagonal epilogue reuses sm
    // epilogue: D2 = |a_i|^2 + |a_j|^2 - 2 <a_i, a_j>; C layout of 32x32: col = lane & 31,
    // row = (e & 3) + 8 (e >> 2) + 4 h
    float nj[MA];
#pragma unroll
    for (int b = 0; b < MA; ++b) {
        const int j = bj * TS + wc * (TS / 2) + b * 32 + r;
        nj[b] = nrm[j < n ? j : n - 1];
    }
    if (bi != bj) {
#pragma unroll
        for (int a = 0; a < MA; ++a) {
            const int i0 = bi * TS + wr * (TS / 2) + a * 32;
            float ni[16];
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int i = i0 + (e & 3) + 8 * (e >> 2) + 4 * h;
                ni[e] = nrm[i < n ? i : n - 1];
            }
#pragma unroll
            for (int b = 0; b < MA; ++b) {
                const int j = bj * TS + wc * (TS / 2) + b * 32 + r;
                float dv[16];
#pragma unroll
                for (int e = 0; e < 16; ++e) dv[e] = ni[e] + nj[b] - 2.f * acc[a][b][e];
#pragma unroll
                for (int e = 0; e < 16; ++e) {   // direct: 32 lanes per 128-B row piece
                    const int i = i0 + (e & 3) + 8 * (e >> 2) + 4 * h;
                    if (i < n && j < n) dput<H>(D2, size_t(i) * ld + j, dv[e], dsc);
                }
                if (j < n) {   // mirrored: row j, columns i0 + 8 g + 4 h .. +3
#pragma unroll
                    for (int g = 0; g < 4; ++g) {
                        const int i = i0 + 8 * g + 4 * h;
                        const size_t o = size_t(j) * ld + i;
                        if (i + 4 <= n) {
                            dput4<H>(D2, o, f32x4{dv[4 * g], dv[4 * g + 1], dv[4 * g + 2], dv[4 * g + 3]}, dsc);
                        } else {
#pragma unroll
                            for (int t = 0; t < 4; ++t)
                                if (i + t < n) dput<H>(D2, o + t, dv[4 * g + t], dsc);
                        }
                    }
                }
            }
        }
    } else {
        // diagonal tile: stage [TS][TS + 1] in LDS, store the upper triangle in both orientations
        float* tile = reinterpret_cast<float*>(sm);
        constexpr int LT = TS + 1;
#pragma unroll
        for (int a = 0; a < MA; ++a)
#pragma unroll
            for (int b = 0; b < MA; ++b)
#pragma unroll
                for (int e = 0; e < 16; ++e) {
                    const int ti = wr * (TS / 2) + a * 32 + (e & 3) + 8 * (e >> 2) + 4 * h;
                    const int tj = wc * (TS / 2) + b * 32 + r;
                    const int i = bi * TS + ti;
                    tile[ti * LT + tj] = nrm[i < n ? i : n - 1] + nj[b] - 2.f * acc[a][b][e];
                }
        __syncthreads();
        for (int q = threadIdx.x; q < TS * TS; q += 256) {
            const int ti = q / TS, tj = q % TS;
            const int i = bi * TS + ti, j = bi * TS + tj;
            if (i < n && j < n) dput<H>(D2, size_t(i) * ld + j, tj >= ti ? tile[ti * LT + tj] : tile[tj * LT + ti], dsc);
        }
    }
}

// --------------------------------------------------------------------------------------
// gram_pk2_kernel (round 3): the pre-split bf16 GEMM on 256 x 256 upper-triangle tiles with 8
// waves -- two per SIMD -- of 64 x 128 (2 x 4 accumulators of 32 x 32), k-stages of 32 features.
// gram_pk_kernel's 128-tile moves 64 KiB into the CU per 48 MFMAs per wave at one wave per
// SIMD (~96 flops per staged byte; MFMA busy 25-28%, profiles/r02f_mfma_*.json): the CU's
// L2 -> LDS rate, not the matrix pipe, set its pace.  Here a stage is the same 64 KiB (A hi /
// lo and B hi / lo, 256 rows x 64 B each, by LDS-DMA, double-buffered: 128 KiB) for 48 MFMAs
// on EACH of 8 waves -- twice the flops per byte -- and the second wave per SIMD covers the
// other's waits.  Rows are 64 B in LDS, the four 16-B segments XOR-swizzled by (row >> 2) & 3 on
// the source address, which keeps every ds_read_b128 lane group of a fragment read on 16
// distinct bank groups.  Same k order per element as gram_pk_kernel (16-feature chunks in
// ascending order, lo*hi, hi*lo, hi*hi), same epilogue formula, same upper-triangle values
// stored in both orientations: D2 is bitwise gram_pk_kernel's.
// --------------------------------------------------------------------------------------
template <bool H>
__global__ __launch_bounds__(512) void gram_pk2_kernel(const __bf16* __restrict__ Ph,
                                                       const __bf16* __restrict__ Pl,
                                                       const float* __restrict__ nrm, int n,
                                                       int dp, int T, float* __restrict__ D2,
                                                       int ld, size_t wss,
                                                       float* __restrict__ d2s) {
    const int NT = T * (T + 1) / 2;
    const int idx = xcd_tile(blockIdx.x, gridDim.x);
    const int g = idx / NT;
    {
        const size_t off = size_t(g) * wss;   // graph g's workspace block
        Ph = reinterpret_cast<const __bf16*>(reinterpret_cast<const char*>(Ph) + off);
        Pl = reinterpret_cast<const __bf16*>(reinterpret_cast<const char*>(Pl) + off);
        nrm = reinterpret_cast<const float*>(reinterpret_cast<const char*>(nrm) + off);
        D2 = reinterpret_cast<float*>(reinterpret_cast<char*>(D2) + off);
        d2s = reinterpret_cast<float*>(reinterpret_cast<char*>(d2s) + off);
    }
    constexpr int kTP = 256 * kPK2;                                 // bf16 per tile plane
    constexpr int kSS = 260;   // epilogue staging: 128 rows x 256 columns, row stride 260 floats
    constexpr int kSM = 2 * 4 * kTP > 2 * 128 * kSS ? 2 * 4 * kTP : 2 * 128 * kSS;
    __shared__ __attribute__((aligned(16))) __bf16 sm[kSM];   // 130 KiB: [buf][plane] k-stages
    const int lane = lane_id();
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int r = lane & 31, h = lane >> 5;
    int bi, bj;
    supertile_tile(idx - g * NT, T, bi, bj);
    const int wr = w >> 1, wc = w & 1;   // rows wr * 64 .., columns wc * 128 ..
    // DMA pieces of a stage: 4 planes x 16 chunks of 16 rows (1 KiB each); wave w issues pieces
    // q = 0..7: plane q >> 1, chunk (q & 1) * 8 + w; lane -> row 16 c + lane / 4, LDS segment
    // lane % 4 <- source segment (lane % 4) ^ ((row >> 2) & 3)
    const __bf16* src[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        const int pl = q >> 1, c = (q & 1) * 8 + w;
        const int row = 16 * c + (lane >> 2);
        const int seg = (lane & 3) ^ ((row >> 2) & 3);
        int grow = (pl < 2 ? bi : bj) * 256 + row;
        grow = grow < n ? grow : n - 1;
        src[q] = ((pl & 1) ? Pl : Ph) + size_t(grow) * dp + 8 * seg;
    }
    auto issue4 = [&](int ks, int buf, int q0) {
#pragma unroll
        for (int q = q0; q < q0 + 4; ++q) {
            const int pl = q >> 1, c = (q & 1) * 8 + w;
            __bf16* dst = sm + (buf * 4 + pl) * kTP + c * 16 * kPK2;
            __builtin_amdgcn_global_load_lds(src[q] + ks * kPK2, (lds_void*)dst, 16, 0, 0);
        }
    };
    f32x16 acc[2][4];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[a][b][e] = 0.f;
    auto frag = [&](int buf, int pl, int row, int kk) {
        const int pos = (2 * kk + h) ^ ((row >> 2) & 3);
        return *reinterpret_cast<const bf16x8*>(sm + (buf * 4 + pl) * kTP + row * kPK2 + 8 * pos);
    };
    const int nks = dp / kPK2;
    issue4(0, 0, 0);
    issue4(0, 0, 4);
    float dsc = 1.f;   // fp16 D2 scale (H), computed under the first stage's DMAs
    if constexpr (H) {
        __shared__ float red[8];
        dsc = tile_d2_scale<512>(nrm, n, red);
        if (threadIdx.x == 0) *d2s = dsc;
    }
    // (Measured and removed in round 4: requesting both k-steps' fragments of a stage at once,
    // two register sets, 250 VGPRs: B = 64 NS Gram 200 -> 205 us, stress 277 -> 285;
    // profiles/r03y_d2_fp16_ab.txt.)
    {
        for (int ks = 0; ks < nks; ++ks) {
            const int buf = ks & 1;
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");       // this wave's stage-ks DMAs
            __builtin_amdgcn_s_barrier();                          // every wave's
            const bool more = ks + 1 < nks;
#pragma unroll
            for (int kk = 0; kk < kPK2 / 16; ++kk) {
                if (more) issue4(ks + 1, buf ^ 1, 4 * kk);
                bf16x8 ah[2], al[2], bh[4], bl[4];
#pragma unroll
                for (int m = 0; m < 2; ++m) {
                    ah[m] = frag(buf, 0, wr * 64 + m * 32 + r, kk);
                    al[m] = frag(buf, 1, wr * 64 + m * 32 + r, kk);
                }
#pragma unroll
                for (int m = 0; m < 4; ++m) {
                    bh[m] = frag(buf, 2, wc * 128 + m * 32 + r, kk);
                    bl[m] = frag(buf, 3, wc * 128 + m * 32 + r, kk);
                }
#pragma unroll
                for (int a = 0; a < 2; ++a)
#pragma unroll
                    for (int b = 0; b < 4; ++b) {
                        acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al[a], bh[b], acc[a][b], 0, 0, 0);
                        acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[a], bl[b], acc[a][b], 0, 0, 0);
                        acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[a], bh[b], acc[a][b], 0, 0, 0);
                    }
            }
        }
    }
    // epilogue: D2 = |a_i|^2 + |a_j|^2 - 2 <a_i, a_j>; C layout of 32x32: col = lane & 31,
    // row = (e & 3) + 8 (e >> 2) + 4 h.  Diagonal tiles keep the upper triangle (tj >= ti, the
    // value gram_pk_kernel stores there) and write it in both orientations.
    const bool diag = bi == bj;
    if (!diag) {
        // Off-diagonal tiles (round 3): the mirrored orientation leaves the registers as one
        // 16-B store per lane (a lane holds 4 consecutive rows of its column), while the direct
        // one -- 128 four-byte stores per wave, 256 B each -- goes through LDS: each half of the
        // tile (128 rows) is staged row-major and leaves as 1-KiB row stores (16 per wave).
        // Same values, same positions: D2 is bitwise the per-element epilogue's.
#pragma unroll
        for (int a = 0; a < 2; ++a) {
            const int i0 = bi * 256 + wr * 64 + a * 32;
            float ni[16];
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int i = i0 + (e & 3) + 8 * (e >> 2) + 4 * h;
                ni[e] = nrm[i < n ? i : n - 1];
            }
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                const int j = bj * 256 + wc * 128 + b * 32 + r;
                const float nj = nrm[j < n ? j : n - 1];
#pragma unroll
                for (int e = 0; e < 16; ++e) acc[a][b][e] = ni[e] + nj - 2.f * acc[a][b][e];
                if (j < n) {   // mirrored: row j, columns i0 + 8 g + 4 h .. +3
#pragma unroll
                    for (int gq = 0; gq < 4; ++gq) {
                        const int i = i0 + 8 * gq + 4 * h;
                        const size_t o = size_t(j) * ld + i;
                        if (i + 4 <= n) {
                            dput4<H>(D2, o, f32x4{acc[a][b][4 * gq], acc[a][b][4 * gq + 1],
                                                  acc[a][b][4 * gq + 2], acc[a][b][4 * gq + 3]}, dsc);
                        } else {
#pragma unroll
                            for (int t = 0; t < 4; ++t)
                                if (i + t < n) dput<H>(D2, o + t, acc[a][b][4 * gq + t], dsc);
                        }
                    }
                }
            }
        }
        float* stg = reinterpret_cast<float*>(sm);
#pragma unroll
        for (int hh = 0; hh < 2; ++hh) {
            __syncthreads();   // the k-stage buffers (then the previous half) are no longer read
            if ((wr >> 1) == hh) {
#pragma unroll
                for (int a = 0; a < 2; ++a)
#pragma unroll
                    for (int b = 0; b < 4; ++b)
#pragma unroll
                        for (int e = 0; e < 16; ++e) {
                            const int row = (wr & 1) * 64 + a * 32 + (e & 3) + 8 * (e >> 2) + 4 * h;
                            stg[row * kSS + wc * 128 + b * 32 + r] = acc[a][b][e];
                        }
            }
            __syncthreads();
            const int j = bj * 256 + 4 * lane;
#pragma unroll 4
            for (int q = 0; q < 16; ++q) {
                const int row = w * 16 + q;
                const int i = bi * 256 + hh * 128 + row;
                const f32x4 v = *reinterpret_cast<const f32x4*>(stg + row * kSS + 4 * lane);
                if (i < n) {
                    const size_t o = size_t(i) * ld + j;
                    if (j + 4 <= n) {
                        dput4<H>(D2, o, v, dsc);
                    } else {
#pragma unroll
                        for (int t = 0; t < 4; ++t)
                            if (j + t < n) dput<H>(D2, o + t, v[t], dsc);
                    }
                }
            }
        }
        return;
    }
#pragma unroll
    for (int a = 0; a < 2; ++a) {
        const int ti0 = wr * 64 + a * 32;
        const int i0 = bi * 256 + ti0;
        float ni[16];
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int i = i0 + (e & 3) + 8 * (e >> 2) + 4 * h;
            ni[e] = nrm[i < n ? i : n - 1];
        }
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const int tj = wc * 128 + b * 32 + r;
            const int j = bj * 256 + tj;
            if (diag && wc * 128 + b * 32 + 31 < ti0) continue;   // sub-tile wholly below
            const float nj = nrm[j < n ? j : n - 1];
            float dv[16];
#pragma unroll
            for (int e = 0; e < 16; ++e) dv[e] = ni[e] + nj - 2.f * acc[a][b][e];
#pragma unroll
            for (int e = 0; e < 16; ++e) {   // direct: 32 lanes per 128-B row piece
                const int ti = ti0 + (e & 3) + 8 * (e >> 2) + 4 * h;
                const int i = bi * 256 + ti;
                if (i < n && j < n && (!diag || tj >= ti)) dput<H>(D2, size_t(i) * ld + j, dv[e], dsc);
            }
            if (j < n) {   // mirrored: row j, columns i0 + 8 g + 4 h .. +3
#pragma unroll
                for (int gq = 0; gq < 4; ++gq) {
                    const int ti = ti0 + 8 * gq + 4 * h;
                    const int i = bi * 256 + ti;
                    const size_t o = size_t(j) * ld + i;
                    if (i + 4 <= n && (!diag || tj >= ti + 3)) {
                        dput4<H>(D2, o, f32x4{dv[4 * gq], dv[4 * gq + 1], dv[4 * gq + 2], dv[4 * gq + 3]}, dsc);
                    } else {
#pragma unroll
                        for (int t = 0; t < 4; ++t)
                            if (i + t < n && (!diag || tj >= ti + t)) dput<H>(D2, o + t, dv[4 * gq + t], dsc);
                    }
                }
            }
        }
    }
}

// Every launch below follows gram_route (knn_route.h): the one place the kernels are chosen.
hipError_t launch_gram(const Layout& L, const Batch& bt, void* ws, const float* X, bool vec,
                       hipStream_t s) {
    float* D2 = L.at<float>(ws, L.D2);
    int32_t* st = L.at<int32_t>(ws, L.status);
    int32_t* rc = L.at<int32_t>(ws, L.rev_cnt);
    const GramRoute rt = gram_route(L, bt, vec, device_cus());
    if (rt.panels) return hipErrorInvalidValue;   // row panels: launch_gram_panel
    prof_begin(GLL_K_GRAM, s);
    switch (rt.family) {
    case kGramBf3s: {
        const int T = (L.n + 63) / 64;
        const dim3 grid(T * T, bt.B);
        const size_t plane = size_t(L.n) * L.ldD;
        launch_k(rt.vec ? gram_bf3s_kernel<true> : gram_bf3s_kernel<false>, grid, 1024, 0, s, X,
                 L.n, L.d, T, D2, L.ldD, plane, st, rc, bt.x, bt.ws);
        prof_end(GLL_K_GRAM, s);
        return launch_status("gram.hip:launch_gram(bf3s)");
    }
    // pre-split GEMM from 256 tiles (NS B = 8, 288 tiles: 58 -> 45 us; a single FullySup graph,
    // 78 tiles, stays on the 64-tile kernel: 17.5 against 21.6 us).  Not for single graphs with
    // d <= 128 (utils.laplace's 250 + 60,000 points: one K stage, nothing for the DMA pipeline to
    // hide, and the whole graph build took 166 ms with it against 19 ms with the inline 128-tile
    // kernel; 20,250 points 3.9 -> 2.1 ms; profiles/r02i_gram_inline_ab.txt).  Batches
    // and d = 1024 keep it (NS B = 64 322 -> 237 us, FullySup B = 64 272 -> 228, stress 485 -> 319).
    // Nor for single graphs past ~12k rows at any d: forward 5.2 vs 3.8 ms at 20,250 x 256, 16.3 vs
    // 8.7 ms at 30,250 x 512, 17.5 vs 11.4 ms at 30,250 x 1024 (tools/gram_route_probe.py,
    // profiles/r02j_gram_route.txt); the stress shape (8,192 x 1024) is the largest measured where
    // it wins, and the 12,288 cut between the two is not measured.
    case kGramPk:
    case kGramPk2: {
        // split once (one pass over X), then the LDS-DMA bf16 GEMM over 128- or 256-tiles
        __bf16* Ph = L.at<__bf16>(ws, L.xhi);
        __bf16* Pl = L.at<__bf16>(ws, L.xlo);
        float* nrm = L.at<float>(ws, L.xnrm);
        const bool H = rt.H;
        const int T = (L.n + 127) / 128, T2 = (L.n + 255) / 256;
        const int64_t nt2 = int64_t(bt.B) * T2 * (T2 + 1) / 2;
        const int64_t tail = rt.tail;
        prof_span(tail > 0 ? 3 : 2);
        const dim3 sgrid((L.n + 3) / 4, bt.B);
        float* d2s = L.at<float>(ws, L.d2s);
        launch_k(rt.vec ? gram_split_kernel<true> : gram_split_kernel<false>, sgrid, 256, 0, s, X,
                 L.n, L.d, L.dp, Ph, Pl, nrm, st, rc, bt.x, bt.ws);
        if (rt.t256) {
            launch_k(H ? gram_pk2_kernel<true> : gram_pk2_kernel<false>,
                     dim3(unsigned(nt2 - tail)), 512, 0, s, Ph, Pl, nrm, L.n, L.dp, T2, D2,
                     L.ldD, bt.ws, d2s);
            if (tail > 0 && rt.sub == 4)
                launch_k(H ? gram_pk_kernel<true, 128> : gram_pk_kernel<false, 128>,
                         dim3(unsigned(4 * tail)), 256, 0, s, Ph, Pl, nrm, L.n, L.dp, T, D2, L.ldD,
                         bt.ws, d2s, int(nt2 - tail));
            else if (tail > 0)
                launch_k(H ? gram_pk_kernel<true, 64> : gram_pk_kernel<false, 64>,
                         dim3(unsigned(16 * tail)), 256, 0, s, Ph, Pl, nrm, L.n, L.dp,
                         (L.n + 63) / 64, D2, L.ldD, bt.ws, d2s, int(nt2 - tail));
        } else {
            launch_k(H ? gram_pk_kernel<true, 128> : gram_pk_kernel<false, 128>,
                     dim3(unsigned(bt.B * T * (T + 1) / 2)), 256, 0, s, Ph, Pl, nrm, L.n, L.dp, T,
                     D2, L.ldD, bt.ws, d2s, -1);
        }
        prof_end(GLL_K_GRAM, s);
        return launch_status("gram.hip:launch_gram(pk)");
    }
    case kGramBf3w: {
        const int T = (L.n + 127) / 128;
        const dim3 grid(T * (T + 1) / 2, bt.B);
        launch_k(rt.vec ? gram_bf3w_kernel<true> : gram_bf3w_kernel<false>, grid, 1024, 0, s, X,
                 L.n, L.d, T, D2, L.ldD, st, rc, bt.x, bt.ws, 0, 0);
        prof_end(GLL_K_GRAM, s);
        return launch_status("gram.hip:launch_gram(bf3w)");
    }
    case kGramBf3h: {   // 1024-thread tile 17.4 -> 9.5 us at FullySup (profiles/r06v_ab_*.txt)
        const int T64 = (L.n + 63) / 64;
        const dim3 grid(T64 * (T64 + 1) / 2, bt.B);
        launch_k(rt.vec ? gram_bf3h_kernel<true> : gram_bf3h_kernel<false>, grid, 512, 0, s, X,
                 L.n, L.d, T64, D2, L.ldD, st, rc, bt.x, bt.ws);
        prof_end(GLL_K_GRAM, s);
        return launch_status("gram.hip:launch_gram(bf3h)");
    }
    default: {
        const int T64 = (L.n + 63) / 64;
        const dim3 grid(T64 * (T64 + 1) / 2, bt.B);
        launch_k(rt.vec ? gram_bf3_kernel<true> : gram_bf3_kernel<false>, grid, 1024, 0, s, X, L.n,
                 L.d, T64, D2, L.ldD, st, rc, bt.x, bt.ws);
        prof_end(GLL_K_GRAM, s);
        return launch_status("gram.hip:launch_gram(bf3)");
    }
    }
}

// One row panel of the Gram (build_graph's panel mode, single graphs): rows r0 .. r0 + rows - 1
// against every column on the inline-split 128-tile kernel (rectangular tiles: twice the flops
// of the triangle, for an O(panel x n) buffer).
hipError_t launch_gram_panel(const Layout& L, void* ws, const float* X, bool vec, int r0, int rows,
                             hipStream_t s) {
    float* D2 = L.at<float>(ws, L.D2);
    int32_t* st = L.at<int32_t>(ws, L.status);
    int32_t* rc = L.at<int32_t>(ws, L.rev_cnt);
    const GramRoute rt = gram_route(L, Batch{}, vec, 0);   // a panel route reads no CU count
    const int T = (L.n + 127) / 128, pt = (rows + 127) / 128;
    if (!rt.panels || rt.family != kGramBf3w || r0 % 128 || pt <= 0) return hipErrorInvalidValue;
    const dim3 grid(unsigned(int64_t(pt) * T));
    prof_begin(GLL_K_GRAM, s);
    launch_k(rt.vec ? gram_bf3w_kernel<true> : gram_bf3w_kernel<false>, grid, 1024, 0, s, X, L.n,
             L.d, T, D2, L.ldD, st, rc, size_t(0), size_t(0), r0, pt);
    prof_end(GLL_K_GRAM, s);
    return launch_status("gram.hip:launch_gram_panel");
}

}  // namespace gll
