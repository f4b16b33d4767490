// ingest.hip -- the graph build's first stage from caller-supplied neighbour lists (DESIGN.md
// §3.14): what gram.hip + select.hip leave in the workspace -- knn_idx, knn_d2, eps, the reverse
// lists and the overflow triples -- written from an n x (K - 1) int32 list per graph instead of a
// search.  The reference defines everything after the search on an arbitrary knn_ind
// (GLL.py:186-205); the row build, the solves and the gradients read only the workspace.
//
// Two launches: ingest_reset_kernel zeroes the per-call counters the Gram's first launch zeroes on
// the searched route (the internal status words, the perm-valid word among them, and rev_cnt);
// knn_ingest_kernel then runs one wave per row.
#include <climits>

#include "gll_internal.h"

namespace gll {

constexpr int kIngNT = 256;          // 4 waves a workgroup, one row each
constexpr int kIngParts = kMaxKm1Huge / kWave;   // 64-entry parts of a list (K - 1 <= 256)
constexpr int kIngStageD = 2048;     // x_i is staged in LDS up to this many features (8 KiB a wave)
constexpr int kIngPG = 2;            // groups of 8 candidates a sweep
constexpr int kIngNU = 8;            // steps of 32 features with their loads in flight together

__global__ __launch_bounds__(256) void ingest_reset_kernel(int32_t* __restrict__ status,
                                                            int32_t* __restrict__ rev_cnt, int n,
                                                            size_t wss) {
    const int g = int(blockIdx.y);
    status = gshift_at(status, wss, g);
    rev_cnt = gshift_at(rev_cnt, wss, g);
    const int q = int(blockIdx.x) * 256 + int(threadIdx.x);
    if (q < kStWords) status[q] = 0;
    if (q < n) rev_cnt[q] = 0;
}

// Sum over each aligned group of 8 lanes, float64 (a butterfly: every lane of the group ends with
// the same bits, and the (i, j) and (j, i) sums -- the same squares -- agree bitwise).
__device__ __forceinline__ double ingest_group8_sum(double v) {
    v += __shfl_xor(v, 1);
    v += __shfl_xor(v, 2);
    v += __shfl_xor(v, 4);
    return v;
}

// The select's reverse scatter (select.hip step 5): entry (cj, i, d2) into row cj's reverse list,
// past RCAP into the overflow triples.  Integer slot counters only.
__device__ __forceinline__ void ingest_push_reverse(int cj, int i, float d2f, int RCAP,
                                                    int32_t* __restrict__ rev_cnt,
                                                    int32_t* __restrict__ rev_idx,
                                                    float* __restrict__ rev_d2,
                                                    int32_t* __restrict__ ovf,
                                                    int32_t* __restrict__ status) {
    const int pos = atomicAdd(&rev_cnt[cj], 1);
    if (pos < RCAP) {
        rev_idx[size_t(cj) * RCAP + pos] = i;
        rev_d2[size_t(cj) * RCAP + pos] = d2f;
    } else {
        const int q = atomicAdd(&status[kStOvfCount], 1);
        ovf[3 * q + 0] = cj;
        ovf[3 * q + 1] = i;
        ovf[3 * q + 2] = __float_as_int(d2f);
    }
}

// One wave per row i of graph g = blockIdx.y.  Per 64-entry part of the list:
//   1. classify: outside [0, n) -> dropped, counted; the row itself -> dropped; equal to an
//      earlier entry of the row -> dropped, counted (the whole list sits in the wave's LDS);
//   2. exact d2 of the live entries in float64, 8 lanes a candidate over the features (lane `sub`
//      of a group takes features 4 sub + 32 u .. + 3: exact_d2's mapping in select.hip), rounded
//      once to fp32; d2 = 0 and non-finite d2 -> dropped;
//   3. the kept entries go behind those of the earlier parts, in the caller's order.
// Then the padding, eps and the reverse entries.  STAGE: x_i sits in the wave's LDS slice (read
// from memory once); past kIngStageD features it is re-read through the cache instead.
template <bool VEC>
__global__ __launch_bounds__(kIngNT) void knn_ingest_kernel(
    const float* __restrict__ X, const int32_t* __restrict__ nbr, int n, int d, int K,
    float eps_fixed, int auto_eps, int RCAP, int stage, int32_t* __restrict__ knn_idx,
    float* __restrict__ knn_d2, float* __restrict__ eps, int32_t* __restrict__ rev_cnt,
    int32_t* __restrict__ rev_idx, float* __restrict__ rev_d2, int32_t* __restrict__ ovf,
    int32_t* __restrict__ status, int32_t* __restrict__ status_pub, size_t xs, size_t ns,
    size_t wss, size_t sts) {
    const int2 gxy = batch_xy<false>();
    X = gshift_at(X, xs, gxy.y);
    nbr = gshift_at(nbr, ns, gxy.y);
    knn_idx = gshift_at(knn_idx, wss, gxy.y);
    knn_d2 = gshift_at(knn_d2, wss, gxy.y);
    eps = gshift_at(eps, wss, gxy.y);
    rev_cnt = gshift_at(rev_cnt, wss, gxy.y);
    rev_idx = gshift_at(rev_idx, wss, gxy.y);
    rev_d2 = gshift_at(rev_d2, wss, gxy.y);
    ovf = gshift_at(ovf, wss, gxy.y);
    status = gshift_at(status, wss, gxy.y);
    status_pub = gshift_at(status_pub, sts, gxy.y);
    __shared__ int s_list[kIngNT / kWave][kMaxKm1Huge];
    extern __shared__ __attribute__((aligned(16))) float s_x[];   // stage: 4 x dpad floats
    const int lane = lane_id();
    const int wv = threadIdx.x >> 6;
    const int i = gxy.x * (kIngNT / kWave) + wv;
    if (i >= n) return;   // whole wave
    const int Km1 = K - 1;
    const int grp = lane >> 3, sub = lane & 7;
    const float* xi = X + size_t(i) * d;
    const int dpad = (d + 3) & ~3;
    float* sx = s_x + size_t(wv) * dpad;
    if (stage) {
        for (int k = 4 * lane; k < dpad; k += 4 * kWave)
            *reinterpret_cast<f32x4*>(sx + k) = load4<VEC>(xi, k, d);
    }
    // the row's list, as given
    const int32_t* li = nbr + size_t(i) * Km1;
    int* sl = s_list[wv];
    for (int t = lane; t < Km1; t += kWave) sl[t] = li[t];
    __builtin_amdgcn_wave_barrier();   // a wave's LDS ops run in order
    asm volatile("" ::: "memory");

    int32_t* oi = knn_idx + size_t(i) * K;
    float* od = knn_d2 + size_t(i) * K;
    int nk = 0;          // entries kept so far
    int ndrop = 0;       // this lane's counted drops
    float last = 0.f;    // stored d2 of column K - 1, when a kept entry lands there
#pragma unroll 1
    for (int h = 0; h < kIngParts; ++h) {
        const int t0 = h * kWave;
        if (t0 >= Km1) break;   // wave-uniform
        const int t = t0 + lane;
        const int jt = t < Km1 ? sl[t] : -1;
        const bool in = t < Km1 && jt >= 0 && jt < n;
        ndrop += (t < Km1 && !in) ? 1 : 0;
        bool live = in && jt != i;
        // a repeat of an earlier entry of the row (entries 0 .. t - 1)
        bool rep = false;
        const int tmax = min(t0 + kWave, Km1);
        for (int u = 0; u < tmax; ++u) rep |= (u < t && sl[u] == jt);
        if (live && rep) {
            live = false;
            ++ndrop;
        }
        const int cj = live ? jt : -1;
        const int cnt = min(kWave, Km1 - t0);
        // float64 difference-form distances: kIngPG groups of 8 candidates a sweep, kIngNU steps
        // of 32 features a round with every load of the round issued before the first use (the
        // gathers are dependent round trips otherwise: a sweep of NS took 4 of them).  A step past
        // d re-reads the row's first 16 B and is masked to zero: the sums add exact zeros there.
        double dv = 0.0;
        for (int p0 = 0; p0 < cnt; p0 += 8 * kIngPG) {
            const float* xj[kIngPG];
#pragma unroll
            for (int g2 = 0; g2 < kIngPG; ++g2) {
                const int j = __shfl(cj, p0 + 8 * g2 + grp);   // p0 + 8 g2 + grp < 64
                xj[g2] = X + size_t(j >= 0 ? j : i) * d;
            }
            double part[kIngPG];
#pragma unroll
            for (int g2 = 0; g2 < kIngPG; ++g2) part[g2] = 0.0;
            for (int kb = 4 * sub; kb < d + 4 * sub; kb += 32 * kIngNU) {   // wave-uniform trip count
                f32x4 vb[kIngPG][kIngNU];
#pragma unroll
                for (int u = 0; u < kIngNU; ++u)
#pragma unroll
                    for (int g2 = 0; g2 < kIngPG; ++g2)
                        vb[g2][u] = load4_raw<VEC>(xj[g2], kb + 32 * u, d);
#pragma unroll
                for (int u = 0; u < kIngNU; ++u) {
                    const int k = kb + 32 * u;
                    f32x4 a;
                    if (stage) a = k < d ? *reinterpret_cast<const f32x4*>(sx + k)
                                         : f32x4{0.f, 0.f, 0.f, 0.f};
                    else a = mask4<VEC>(load4_raw<VEC>(xi, k, d), k, d);
#pragma unroll
                    for (int g2 = 0; g2 < kIngPG; ++g2) {
                        const f32x4 b = mask4<VEC>(vb[g2][u], k, d);
                        const double d0 = double(a.x) - double(b.x), d1 = double(a.y) - double(b.y);
                        const double d2 = double(a.z) - double(b.z), d3 = double(a.w) - double(b.w);
                        part[g2] = __builtin_fma(d0, d0, part[g2]);
                        part[g2] = __builtin_fma(d1, d1, part[g2]);
                        part[g2] = __builtin_fma(d2, d2, part[g2]);
                        part[g2] = __builtin_fma(d3, d3, part[g2]);
                    }
                }
            }
#pragma unroll
            for (int g2 = 0; g2 < kIngPG; ++g2) {
                const double tot = ingest_group8_sum(part[g2]);
#pragma unroll
                for (int g = 0; g < 8; ++g) {
                    const double v = __shfl(tot, 8 * g);
                    if (lane == p0 + 8 * g2 + g) dv = v;
                }
            }
        }
        const float d2f = float(dv);   // correctly rounded
        // zero (a duplicated point) and non-finite distances never enter the graph
        const bool keep = live && d2f > 0.f && d2f < __builtin_inff();
        const uint64_t mk = __ballot(keep);
        const int pos = nk + lanes_below(mk);   // < Km1
        if (keep) {
            oi[1 + pos] = cj;
            od[1 + pos] = d2f;
            ingest_push_reverse(cj, i, d2f, RCAP, rev_cnt, rev_idx, rev_d2, ovf, status);
        }
        const uint64_t lb = __ballot(keep && pos == Km1 - 1);
        if (lb) last = readlane_f(d2f, int(__builtin_ctzll(lb)));
        nk += __popcll(mk);
    }
    // short rows: self at distance 0, i.e. dropped edges, as the select pads (select.hip)
    for (int r = nk + lane; r < Km1; r += kWave) {
        oi[1 + r] = i;
        od[1 + r] = 0.f;
    }
    ndrop = wave_sum_i(ndrop);
    if (lane == 0) {
        oi[0] = i;
        od[0] = 0.f;
        // eps_i = d(i, knn_ind[i, K-1]) (GLL.py:205): the caller's last column
        const float ei = auto_eps ? sqrtf(last) : eps_fixed;
        eps[i] = ei;
        if (!(ei >= 1e-10f)) atomicOr(&status_pub[GLL_ST_TINY_EPS], 1);   // GLL.py:240-241
        if (ndrop > 0) atomicAdd(&status_pub[GLL_ST_LIST_DROPPED], ndrop);
    }
}

hipError_t launch_ingest(const Layout& L, const Batch& bt, void* ws, const float* X,
                         const int32_t* nbr, float eps_fixed, bool auto_eps, bool vec,
                         int32_t* status_pub, hipStream_t s) {
    const int n = L.n, K = L.K;
    if (K - 1 > kMaxKm1Huge || K < 2) return hipErrorInvalidValue;
    const int rmax = n > kStWords ? n : kStWords;
    launch_k(ingest_reset_kernel, dim3((rmax + 255) / 256, bt.B), dim3(256), 0, s,
             L.at<int32_t>(ws, L.status), L.at<int32_t>(ws, L.rev_cnt), n, bt.ws);
    hipError_t e = launch_status("ingest.hip:ingest_reset");
    if (e != hipSuccess) return e;
    const int stage = L.d <= kIngStageD ? 1 : 0;
    const size_t lds = stage ? size_t(kIngNT / kWave) * ((L.d + 3) & ~3) * sizeof(float) : 0;
    const dim3 grid((n + kIngNT / kWave - 1) / (kIngNT / kWave), bt.B);
    const size_t ns = size_t(n) * (K - 1) * sizeof(int32_t);
    prof_begin(GLL_K_SELECT, s);   // the stage it stands in for
    auto go = [&](auto fn) {
        launch_k(fn, grid, dim3(kIngNT), lds, s, X, nbr, n, L.d, K, eps_fixed, auto_eps ? 1 : 0,
                 L.RCAP, stage, L.at<int32_t>(ws, L.knn_idx), L.at<float>(ws, L.knn_d2),
                 L.at<float>(ws, L.eps), L.at<int32_t>(ws, L.rev_cnt),
                 L.at<int32_t>(ws, L.rev_idx), L.at<float>(ws, L.rev_d2),
                 L.at<int32_t>(ws, L.ovf), L.at<int32_t>(ws, L.status), status_pub, bt.x, ns,
                 bt.ws, bt.st);
    };
    if (vec) go(knn_ingest_kernel<true>);
    else go(knn_ingest_kernel<false>);
    prof_end(GLL_K_SELECT, s);
    return launch_status("ingest.hip:knn_ingest");
}

}  // namespace gll
