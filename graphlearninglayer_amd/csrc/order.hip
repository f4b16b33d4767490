// order.hip -- the locality order of a large graph's rows, between its Gram (gram.hip) and its
// select (select.hip, which walks the rows in this order).
#include "gll_internal.h"

namespace gll {

// --------------------------------------------------------------------------------------
// Locality order of the rows of one large graph (gll_internal.h locality_order).  Pivot j is
// row (j * 2654435761 + 12345) mod n -- a hash, so periodic row layouts (labels i % 10 in the
// callers' minibatches) do not alias -- and row i joins the pivot nearest to it under the Gram
// D2, read as the pivots' D2 rows (D2 is symmetric; coalesced across i).  Ties go to the lower
// pivot; a NaN distance never wins.  Speed only: no row's result depends on the order.
// --------------------------------------------------------------------------------------
__device__ __forceinline__ int pivot_row(int j, int n) {
    return int((uint32_t(j) * 2654435761u + 12345u) % uint32_t(n));
}

// 64 rows per workgroup, the pivots split over its 4 waves (16 each: every load of a lane
// issued together), the 4 partial minima combined in LDS in pivot order.  Wave 0 then ranks its
// rows within their pivot (lane order: pid = pivot | rank << 8) and writes the block's rows per
// pivot as one plain 64-int histogram row.  (The first version counted with one global atomic
// per row on 64 counters: 8,192 same-address atomics made this a 13.9 us kernel at stress,
// profiles/r04b_stress_kernel_stats.csv; order_perm then scattered through LDS cursor atomics.)
template <int NP>
__global__ __launch_bounds__(256) void order_pid_kernel(const float* __restrict__ D2, int ld,
                                                        size_t plane, int n,
                                                        int32_t* __restrict__ pid,
                                                        int32_t* __restrict__ hist) {
    constexpr int PPW = kPiv / 4;   // pivots per wave
    static_assert(kPiv == kWave, "one histogram bin per lane");
    __shared__ float s_best[4][kWave];
    __shared__ int s_arg[4][kWave];
    const int lane = lane_id(), wv = threadIdx.x >> 6;
    const int i = int(blockIdx.x) * kWave + lane;
    const int ic = i < n ? i : n - 1;
    float v[PPW];
#pragma unroll
    for (int j = 0; j < PPW; ++j) {   // every load issued before any is compared
        const size_t o = size_t(pivot_row(wv * PPW + j, n)) * ld + ic;
        v[j] = D2[o];
#pragma unroll
        for (int p = 1; p < NP; ++p) v[j] += D2[p * plane + o];
    }
    float best = __builtin_inff();
    int bp = wv * PPW;
#pragma unroll
    for (int j = 0; j < PPW; ++j)
        if (v[j] < best) {   // ties: the lower pivot; a NaN never wins
            best = v[j];
            bp = wv * PPW + j;
        }
    s_best[wv][lane] = best;
    s_arg[wv][lane] = bp;
    __syncthreads();
    if (wv != 0) return;
#pragma unroll
    for (int w = 1; w < 4; ++w)
        if (s_best[w][lane] < best) {
            best = s_best[w][lane];
            bp = s_arg[w][lane];
        }
    const bool valid = i < n;
    int rank = 0, cnt = 0;   // cnt: rows of this block at pivot `lane`
    uint64_t todo = __ballot(valid);
    while (todo) {   // one round per distinct pivot of the block (wave-uniform)
        const int v0 = __builtin_amdgcn_readlane(bp, int(__builtin_ctzll(todo)));
        const uint64_t mk = __ballot(valid && bp == v0);
        if (valid && bp == v0) rank = lanes_below(mk);
        if (lane == v0) cnt = __popcll(mk);
        todo &= ~mk;
    }
    if (valid) pid[i] = bp | (rank << 8);
    hist[size_t(blockIdx.x) * kPiv + lane] = cnt;
}

// One workgroup, no atomics: per pivot, the blocks' counts become exclusive offsets (16 block
// groups per pivot, group totals scanned in LDS, pivots scanned by one wave), written back over
// the histogram; then row i goes to offset[block i / 64][pivot] + its rank in the block.
__global__ __launch_bounds__(1024) void order_perm_kernel(int n, const int32_t* __restrict__ pid,
                                                          int32_t* __restrict__ hist,
                                                          int32_t* __restrict__ perm,
                                                          int32_t* __restrict__ status) {
    static_assert(kPiv == kWave, "one wave scans the pivot counts");
    constexpr int NGRP = 1024 / kPiv;   // block groups per pivot
    __shared__ int part[NGRP][kPiv];
    __shared__ int goff[NGRP][kPiv];
    const int tid = threadIdx.x;
    const int nb = (n + kWave - 1) / kWave;
    const int per = (nb + NGRP - 1) / NGRP;
    const int pv = tid & (kPiv - 1), grp = tid / kPiv;
    const int b0 = grp * per, b1 = min(nb, b0 + per);
    int run = 0;
#pragma unroll 8
    for (int b = b0; b < b1; ++b) run += hist[size_t(b) * kPiv + pv];
    part[grp][pv] = run;
    __syncthreads();
    if (tid < kWave) {
        int c = 0;
#pragma unroll
        for (int g = 0; g < NGRP; ++g) c += part[g][tid];
        int incl = c;
#pragma unroll
        for (int off = 1; off < kWave; off <<= 1) {
            const int t = __shfl_up(incl, off);
            if (tid >= off) incl += t;
        }
        int o = incl - c;
#pragma unroll
        for (int g = 0; g < NGRP; ++g) {
            goff[g][tid] = o;
            o += part[g][tid];
        }
    }
    __syncthreads();
    int o = goff[grp][pv];
#pragma unroll 8
    for (int b = b0; b < b1; ++b) {
        const size_t q = size_t(b) * kPiv + pv;
        const int h = hist[q];
        hist[q] = o;
        o += h;
    }
    __syncthreads();   // the offsets are visible to the whole workgroup
    constexpr int U = 8;   // rows per thread per batch: every load of a batch in flight together
    for (int i0 = 0; i0 < n; i0 += 1024 * U) {
        int v[U], h[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int i = i0 + u * 1024 + tid;
            v[u] = i < n ? pid[i] : 0;
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int i = i0 + u * 1024 + tid;
            h[u] = i < n ? hist[size_t(i >> 6) * kPiv + (v[u] & 0xFF)] : 0;
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int i = i0 + u * 1024 + tid;
            if (i < n) perm[h[u] + (v[u] >> 8)] = i;
        }
    }
    if (tid == 0) status[kStPermValid] = 1;   // read by the backward (grad.hip launch_backward_grad)
}

hipError_t launch_order(const Layout& L, void* ws, hipStream_t s) {
    const float* D2 = L.at<float>(ws, L.D2);
    int32_t* hist = L.at<int32_t>(ws, L.ohist);
    int32_t* pid = L.at<int32_t>(ws, L.pid);
    const size_t plane = size_t(L.n) * L.ldD;
    const dim3 grid(unsigned((L.n + kWave - 1) / kWave));
    if (gram_planes(L, 1) == 2)
        launch_k(order_pid_kernel<2>, grid, 256, 0, s, D2, L.ldD, plane, L.n, pid, hist);
    else
        launch_k(order_pid_kernel<1>, grid, 256, 0, s, D2, L.ldD, plane, L.n, pid, hist);
    launch_k(order_perm_kernel, dim3(1), 1024, 0, s, L.n, static_cast<const int32_t*>(pid), hist,
             L.at<int32_t>(ws, L.perm), L.at<int32_t>(ws, L.status));
    return launch_status("order.hip:launch_order");
}

}  // namespace gll
