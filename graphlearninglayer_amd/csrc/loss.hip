// loss.hip -- the cross-entropy head every caller of the layer puts behind it
// (custom_ce_loss, losses.py:128-136; FullySup.py:156-171 adds the argmax accuracy).
//
// After gll_forward the workspace holds the fp32 predictions U32 (Layout::P + base * C); the
// float64 U the forward returns is exactly double(U32) (solve.hip).  With t_i the int64 target of
// unlabeled row i and m = n - base, evaluated in float64:
//     p_i        = double(U32[i, t_i]) + 1e-8
//     row_loss_i = -log(p_i)                             (no clamp: p_i <= 0 gives NaN / inf)
//     loss       = (sum_i row_loss_i) / m
//     gbar[i, c] = float(-(1 / m) / p_i) at c == t_i, 0 elsewhere        = dloss / dU, fp32
//     pred_i     = lowest index among the maxima of row i;  correct = #{i : pred_i == t_i}
// A target outside [0, C) masks its row: row_loss 0, a zero gbar row, not counted as correct, U
// never addressed with it; the divisor stays m (custom_ce_loss divides by batch_size).
//
// Sums run in a fixed order that depends on (m, C) alone -- never on B, the grid or timing; no
// atomics -- so graph g of a batch is bitwise the single call.  While a graph's rows fit one
// workgroup's strided pass (m <= kCeOneWg) the head is ONE launch, grid = B: row group q takes rows
// q, q + G, ... in ascending order, then a fixed tree (wave butterflies, wave sums in order).
// Past that, a row-parallel pass (ce_rows_kernel) leaves one float64 loss and one hit flag per row
// in the caller's scratch and ce_reduce_kernel sums them, as param_grad_kernel /
// param_reduce_kernel do.
#include <climits>
#include <cmath>

#include "gll_internal.h"

namespace gll {

constexpr int kCeThreads = 1024;   // one workgroup of the single-launch form
constexpr int kCeOneWg = 4096;     // rows a graph may have for it: <= 4 strided rows a thread

struct CeArgs {
    const float* U32;         // m x C of graph 0
    const int64_t* targets;   // m of graph 0
    float* gbar;              // m x C, or NULL
    double* row_loss;         // m, or NULL
    int64_t* pred;            // m, or NULL
    int m, C;
    size_t ws;                // byte stride of U32 between graphs (the workspace block)
    double ginv;              // -(1 / m)
};

struct CeRow {
    double loss;   // row_loss_i (0 for a masked row)
    int hit;       // pred_i == t_i
};

// Row i as the LPR lanes of a group hold it: lane gl the classes gl, gl + LPR, ... -- at most NPL of
// them (LPR * NPL >= C), loaded by one unrolled, predicated batch, so a row costs one memory
// latency (U32 was written on other XCDs: the loads miss this XCD's L2), not one per class.
template <int NPL>
struct CeLoad {
    float v[NPL];
    int64_t t;
};

template <int LPR, int NPL>
__device__ __forceinline__ CeLoad<NPL> ce_load(const CeArgs& a, int i, int gl) {
    const float* u = a.U32 + size_t(i) * a.C;
    CeLoad<NPL> d;
    d.t = a.targets[i];
#pragma unroll
    for (int q = 0; q < NPL; ++q) {
        const int c = gl + q * LPR;
        d.v[q] = c < a.C ? u[c] : -INFINITY;
    }
    return d;
}

// The head of row i from its loaded classes (all LPR lanes of the group call this together).
// The row's outputs are written here; the result is the same on every lane of the group.  The
// target never forms an address: U[i, t_i] is picked from the registers that hold the row.
template <int LPR, int NPL>
__device__ __forceinline__ CeRow ce_row(const CeArgs& a, int i, int gl, const CeLoad<NPL>& d) {
    const int64_t t = d.t;
    const bool valid = t >= 0 && t < int64_t(a.C);
    float best = -INFINITY, mine = 1.f;
    int bc = INT_MAX;
#pragma unroll
    for (int q = 0; q < NPL; ++q) {   // ascending c: a strict > keeps the lowest maximum
        const int c = gl + q * LPR;
        if (c < a.C && (d.v[q] > best || (d.v[q] == best && c < bc))) {
            best = d.v[q];
            bc = c;
        }
        if (int64_t(c) == t) mine = d.v[q];
    }
#pragma unroll
    for (int o = LPR / 2; o > 0; o >>= 1) {
        const float ov = __shfl_xor(best, o, LPR);
        const int oc = __shfl_xor(bc, o, LPR);
        if (ov > best || (ov == best && oc < bc)) {
            best = ov;
            bc = oc;
        }
    }
    if (bc == INT_MAX) bc = 0;   // a row of NaN
    // the lane that holds class t_i hands U[i, t_i] to its group
    const float pt = LPR > 1 ? __shfl(mine, valid ? int(t % LPR) : 0, LPR) : mine;
    CeRow r{0.0, 0};
    float gv = 0.f;
    if (valid) {   // group-uniform
        const double p = double(pt) + 1e-8;
        r.loss = -log(p);
        gv = float(a.ginv / p);
        r.hit = int64_t(bc) == t;
    }
    if (a.gbar) {
        float* g = a.gbar + size_t(i) * a.C;
#pragma unroll
        for (int q = 0; q < NPL; ++q) {
            const int c = gl + q * LPR;
            if (c < a.C) g[c] = (valid && int64_t(c) == t) ? gv : 0.f;
        }
    }
    if (gl == 0) {
        if (a.row_loss) a.row_loss[i] = r.loss;
        if (a.pred) a.pred[i] = int64_t(bc);
    }
    return r;
}

__device__ __forceinline__ void ce_to_graph(CeArgs& a, int g) {
    a.U32 = gshift_at(a.U32, a.ws, g);
    a.targets += size_t(g) * a.m;
    a.gbar = gshift_at(a.gbar, size_t(a.m) * a.C * sizeof(float), g);
    a.row_loss = gshift_at(a.row_loss, size_t(a.m) * sizeof(double), g);
    a.pred = gshift_at(a.pred, size_t(a.m) * sizeof(int64_t), g);
}

// Fixed-order sum of the workgroup's NT partials: a butterfly inside each wave, then thread 0 adds
// the NT / 64 wave sums in ascending wave order and writes loss[g] and correct[g].
template <int NT>
__device__ __forceinline__ void ce_finish(double s, int hits, int m, int g,
                                          double* __restrict__ loss,
                                          int64_t* __restrict__ correct) {
    __shared__ double red[NT / kWave];
    __shared__ int cnt[NT / kWave];
#pragma unroll
    for (int o = kWave / 2; o > 0; o >>= 1) {
        s += __shfl_xor(s, o, kWave);
        hits += __shfl_xor(hits, o, kWave);
    }
    if (lane_id() == 0) {
        red[threadIdx.x / kWave] = s;
        cnt[threadIdx.x / kWave] = hits;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double tot = 0.0;
        int c = 0;
#pragma unroll
        for (int w = 0; w < NT / kWave; ++w) {
            tot += red[w];
            c += cnt[w];
        }
        loss[g] = tot / double(m);
        if (correct) correct[g] = int64_t(c);
    }
}

// The single-launch head: workgroup g is graph g.  Group q of LPR lanes takes the rows q, q + G,
// ... (G = kCeThreads / LPR) in ascending order; its lane 0 carries the group's sums into the tree
// (the other lanes add 0), so the order depends on (m, C) alone.
template <int LPR, int NPL>
__global__ __launch_bounds__(kCeThreads) void ce_head_kernel(CeArgs a, double* __restrict__ loss,
                                                             int64_t* __restrict__ correct) {
    const int g = blockIdx.x;
    ce_to_graph(a, g);
    constexpr int G = kCeThreads / LPR;
    const int q = threadIdx.x / LPR, gl = threadIdx.x % LPR;
    double s = 0.0;
    int hits = 0;
    for (int i = q; i < a.m; i += G) {   // group-uniform trip count
        const CeRow r = ce_row<LPR, NPL>(a, i, gl, ce_load<LPR, NPL>(a, i, gl));
        s += r.loss;
        hits += r.hit;
    }
    if (gl != 0) {
        s = 0.0;
        hits = 0;
    }
    ce_finish<kCeThreads>(s, hits, a.m, g, loss, correct);
}

// Past kCeOneWg rows: one row per group, 256 threads; parts: per graph m float64 row losses
// followed by m int32 hit flags (`pss` bytes a graph).
template <int LPR, int NPL>
__global__ __launch_bounds__(256) void ce_rows_kernel(CeArgs a, double* __restrict__ parts,
                                                      size_t pss) {
    const int g = blockIdx.y;
    ce_to_graph(a, g);
    parts = gshift_at(parts, pss, g);
    constexpr int G = 256 / LPR;
    const int gl = threadIdx.x % LPR;
    const int i = blockIdx.x * G + threadIdx.x / LPR;
    if (i >= a.m) return;   // group-uniform
    const CeRow r = ce_row<LPR, NPL>(a, i, gl, ce_load<LPR, NPL>(a, i, gl));
    if (gl == 0) {
        parts[i] = r.loss;
        reinterpret_cast<int*>(parts + a.m)[i] = r.hit;
    }
}

// Second stage: workgroup g sums graph g's m row partials -- thread t the rows t, t + 256, ... in
// ascending order, then the fixed tree.
__global__ __launch_bounds__(256) void ce_reduce_kernel(const double* __restrict__ parts,
                                                        size_t pss, int m,
                                                        double* __restrict__ loss,
                                                        int64_t* __restrict__ correct) {
    const int g = blockIdx.x;
    const double* src = gshift_at(parts, pss, g);
    const int* hit = reinterpret_cast<const int*>(src + m);
    double s = 0.0;
    int hits = 0;
    for (int r = threadIdx.x; r < m; r += 256) {
        s += src[r];
        hits += hit[r];
    }
    ce_finish<256>(s, hits, m, g, loss, correct);
}

__global__ void ce_zero_kernel(double* __restrict__ loss, int B) {
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g < B) loss[g] = 0.0;
}

static size_t ce_parts_stride(int m) {
    return (size_t(m) * (sizeof(double) + sizeof(int)) + 255) & ~size_t(255);
}

size_t ce_head_scratch_bytes(int m, int B) {
    return m > kCeOneWg ? size_t(B) * ce_parts_stride(m) : 0;
}

template <int LPR, int NPL>
static hipError_t launch_ce(const CeArgs& a, int B, double* loss, int64_t* correct, void* scratch,
                            hipStream_t s) {
    if (a.m <= kCeOneWg) {
        launch_k(ce_head_kernel<LPR, NPL>, dim3(B), kCeThreads, 0, s, a, loss, correct);
        return launch_status("loss.hip:ce_head_kernel");
    }
    const size_t pss = ce_parts_stride(a.m);
    double* parts = static_cast<double*>(scratch);
    constexpr unsigned G = 256 / LPR;
    prof_span(2);
    launch_k(ce_rows_kernel<LPR, NPL>, dim3((unsigned(a.m) + G - 1) / G, B), 256, 0, s, a, parts,
             pss);
    hipError_t e = launch_status("loss.hip:ce_rows_kernel");
    if (e != hipSuccess) return e;
    launch_k(ce_reduce_kernel, dim3(B), 256, 0, s, static_cast<const double*>(parts), pss, a.m,
             loss, correct);
    return launch_status("loss.hip:ce_reduce_kernel");
}

hipError_t launch_ce_head(const Layout& L, int B, void* ws, const int64_t* targets, double* loss,
                          float* gbar, double* row_loss, int64_t* pred_label, int64_t* correct,
                          void* scratch, hipStream_t s) {
    prof_begin(GLL_K_LOSS, s);
    hipError_t e;
    if (L.m == 0) {   // no unlabeled row: loss = 0, nothing else
        launch_k(ce_zero_kernel, dim3((unsigned(B) + 255) / 256), 256, 0, s, loss, B);
        e = launch_status("loss.hip:ce_zero_kernel");
    } else {
        CeArgs a;
        a.U32 = L.at<float>(ws, L.P) + size_t(L.base) * L.C;
        a.targets = targets;
        a.gbar = gbar;
        a.row_loss = row_loss;
        a.pred = pred_label;
        a.m = L.m;
        a.C = L.C;
        a.ws = L.total;
        a.ginv = -(1.0 / double(L.m));
        // lanes per row x classes per lane (param_grad.hip's LPR idiom): a thread holds a
        // narrow row alone, 16 or 64 lanes share a wide one (C <= 256, api.hip check)
        if (L.C <= 4) e = launch_ce<1, 4>(a, B, loss, correct, scratch, s);
        else if (L.C <= 16) e = launch_ce<1, 16>(a, B, loss, correct, scratch, s);
        else if (L.C <= 128) e = launch_ce<16, 8>(a, B, loss, correct, scratch, s);
        else e = launch_ce<64, 4>(a, B, loss, correct, scratch, s);
    }
    prof_end(GLL_K_LOSS, s);
    return e;
}

}  // namespace gll
