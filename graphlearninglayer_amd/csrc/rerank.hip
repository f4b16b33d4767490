// rerank.hip -- gll_knn_query's lists from caller-supplied candidates (include/gll.h
// gll_knn_rerank): no Gram panel, no scan, no workspace.
//
//  rerank_kernel  one wave per query row, four rows a workgroup:
//                 pool mode (flags 0, k <= c)
//                 1. the row's c candidates into registers and the wave's LDS list; an entry is
//                    valid when it lies in [0, N) and no earlier entry of the row holds the same
//                    index; the valid ones are compacted in the caller's order;
//                 2. their exact distances (query_common.h q_exact: the fp32 value returned and
//                    the float64 value ranked, from the same loads -- step 2 of
//                    query_select_kernel);
//                 3. the k nearest by (float64 d^2, index) (q_rank_keep, its step 3);
//                 4. the kept ordered by (returned fp32 d^2, index), NaN as +inf (its step 5); a
//                    row with fewer than k valid candidates ends in (-1, +inf) and is counted in
//                    status[3];
//                 list mode (GLL_RR_KEEP_ORDER, c == k)
//                    idx = cand as it is; step 2 over the entries in [0, N) (a repeat is computed
//                    twice), +inf for the others, which are never followed.
//
// An ordinary launch: no inter-workgroup waiting, no spin loop; the only atomics are atomicAdd on
// the status words.  A row's result is a function of that row, its candidates and the database.
#include <cmath>

#include "query_common.h"

namespace gll {

template <bool VEC>
__global__ __launch_bounds__(256) void rerank_kernel(
    const float* __restrict__ Xq, const float* __restrict__ Xdb, const int32_t* __restrict__ cand,
    int64_t Q, int N, int d, int c, int k, int keep_order, int32_t* __restrict__ idx,
    float* __restrict__ d2o, int32_t* __restrict__ status) {
    constexpr int S = kQCap / kWave;
    __shared__ QLists sh[4];
    const int lane = lane_id(), wv = threadIdx.x >> 6;
    const int64_t r = int64_t(blockIdx.x) * 4 + wv;
    if (r >= Q) return;   // whole wave
    QLists& w = sh[wv];
    const float* xq = Xq + size_t(r) * d;
    const int32_t* cr = cand + size_t(r) * c;
    int32_t* oi = idx + size_t(r) * k;
    float* od = d2o + size_t(r) * k;
    bool bad = false;   // a non-finite returned distance

    if (keep_order) {   // c == k <= 256
        for (int e = lane; e < k; e += kWave) {
            const int j = cr[e];
            w.cj[e] = (j >= 0 && j < N) ? j : 0;   // row 0 stands in; its distance is not returned
        }
        __builtin_amdgcn_wave_barrier();
        asm volatile("" ::: "memory");
        q_exact<VEC>(Xdb, xq, d, w, 0, k);
        for (int e = lane; e < k; e += kWave) {
            const int j = cr[e];
            const float fe = (j >= 0 && j < N) ? w.cf[e] : __builtin_inff();
            bad |= !(fabsf(fe) < __builtin_inff());
            oi[e] = j;
            od[e] = fe;
        }
        if (__ballot(bad) != 0ull && lane == 0) atomicAdd(&status[1], 1);
        return;
    }

    // 1) validity: entry e = lane + 64 s in registers, every entry once through LDS
    int jv[S];
    bool ok[S];
#pragma unroll
    for (int s = 0; s < S; ++s) {
        const int e = lane + kWave * s;
        jv[s] = e < c ? cr[e] : -1;
        ok[s] = jv[s] >= 0 && jv[s] < N;
        if (e < c) w.cj[e] = jv[s];
    }
    __builtin_amdgcn_wave_barrier();
    asm volatile("" ::: "memory");
    for (int u = 0; u < c; ++u) {
        const int ju = w.cj[u];
#pragma unroll
        for (int s = 0; s < S; ++s)
            if (s * kWave < c) ok[s] = ok[s] && !(u < lane + kWave * s && ju == jv[s]);
    }
    __builtin_amdgcn_wave_barrier();
    asm volatile("" ::: "memory");
    int cnt = 0;   // valid entries, compacted in the caller's order
#pragma unroll
    for (int s = 0; s < S; ++s) {
        const uint64_t mk = __ballot(ok[s]);
        if (ok[s]) w.cj[cnt + lanes_below(mk)] = jv[s];
        cnt += __popcll(mk);
    }
    __builtin_amdgcn_wave_barrier();
    asm volatile("" ::: "memory");
    // 2-3) exact distances, the k nearest by (float64 d^2, index)
    q_exact<VEC>(Xdb, xq, d, w, 0, cnt);
    const int nb = q_rank_keep(w, cnt, k);
    // 4) the nb kept, by (returned fp32 d^2, index); NaN ranks as +inf
    for (int e = lane; e < nb; e += kWave) {
        const float fe = w.cf[e];
        const float ke = fe == fe ? fe : __builtin_inff();
        const int je = w.cj[e];
        bad |= !(fabsf(fe) < __builtin_inff());
        int rk = 0;
        for (int u = 0; u < nb; ++u) {
            const float fu = w.cf[u];
            const float ku = fu == fu ? fu : __builtin_inff();
            rk += (ku < ke || (ku == ke && w.cj[u] < je)) ? 1 : 0;
        }
        oi[rk] = je;
        od[rk] = fe;
    }
    for (int e = nb + lane; e < k; e += kWave) {   // a short row: no candidate left
        oi[e] = -1;
        od[e] = __builtin_inff();
    }
    bad = __ballot(bad) != 0ull;
    if (lane == 0) {
        if (bad) atomicAdd(&status[1], 1);
        if (nb < k) atomicAdd(&status[3], 1);
    }
}

static int check_rerank(int64_t Q, int64_t N, int32_t d, int32_t c, int32_t k, int flags) {
    if (Q < 1 || N < 1 || d < 1 || k < 1 || c < k) return GLL_ERR_INVALID_ARG;
    if (flags & ~GLL_RR_KEEP_ORDER) return GLL_ERR_INVALID_ARG;
    if ((flags & GLL_RR_KEEP_ORDER) && c != k) return GLL_ERR_INVALID_ARG;
    if (c > kQCap || k > 256 || d > 4096 || N > INT32_MAX / 2 || Q > INT32_MAX / 2)
        return GLL_ERR_UNSUPPORTED;
    return GLL_OK;
}

}  // namespace gll

using namespace gll;

extern "C" int gll_knn_rerank(int64_t Q, int64_t N, int32_t d, int32_t c, int32_t k, int flags,
                              const float* Xq, const float* Xdb, const int32_t* cand, int32_t* idx,
                              float* d2, int32_t* status, void* stream) {
    const int rc = check_rerank(Q, N, d, c, k, flags);
    if (rc != GLL_OK) return rc;
    if (!Xq || !Xdb || !cand || !idx || !d2 || !status) return GLL_ERR_INVALID_ARG;
    if (reinterpret_cast<uintptr_t>(Xq) % 4 || reinterpret_cast<uintptr_t>(Xdb) % 4)
        return GLL_ERR_INVALID_ARG;
    const dim3 grid(unsigned((Q + 3) / 4));
    const int keep = (flags & GLL_RR_KEEP_ORDER) ? 1 : 0;
    const hipStream_t s = static_cast<hipStream_t>(stream);
    if (q_vec(Xq, Xdb, d))
        launch_k(rerank_kernel<true>, grid, dim3(256), 0, s, Xq, Xdb, cand, Q, int(N), int(d),
                 int(c), int(k), keep, idx, d2, status);
    else
        launch_k(rerank_kernel<false>, grid, dim3(256), 0, s, Xq, Xdb, cand, Q, int(N), int(d),
                 int(c), int(k), keep, idx, d2, status);
    return q_launched("rerank.hip:rerank_kernel") == hipSuccess ? GLL_OK : GLL_ERR_HIP;
}
