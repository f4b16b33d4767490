// loss.hip -- the heads callers of the layer put behind it: the cross-entropy head (custom_ce_loss,
// losses.py:128-136; FullySup.py:156-171 adds the argmax accuracy), then the Carlini-Wagner margin
// head (adversarial.py:688-751) and, last, the score/objective head (losses.py:100-101, :111-112
// and the score store of FullySup.py:165-175).
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
#include <algorithm>
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

// ------------------------------------------------------------------------------------------------
// The Carlini-Wagner margin head (adversarial.py:688-751): the two best classes of every row, the
// margin of the best over a class `other` the caller names, its mean and dloss/dU.  Same U32, same
// row-holding scheme, same sums as the cross-entropy head above.  In float64, o_i = other[i]:
//     a_i          = lowest index among the maxima of row i          (pred of the ce head)
//     s_i          = lowest index among the maxima of the row without entry a_i;  0 for C = 1
//     d_i          = double(U32[i, a_i]) - double(U32[i, o_i])
//     row_margin_i = d_i when d_i >= 0 or d_i is NaN, else 0         (torch.clamp(., min=0))
//     loss         = (sum_i row_margin_i) / m
//     gbar[i, c]   = float(1 / m) * ([c == a_i] - [c == o_i])        a zero row when a_i == o_i
//     moved        = #{i : a_i == o_i}
// An o_i outside [0, C) -- or other == NULL: every row -- masks the row: margin 0, a zero gbar row,
// not counted as moved, U never addressed with it; label and second are written all the same and
// the divisor stays m.  The classes of a row are ranked numbers first by value descending, then
// NaN, each by index ascending: a NaN entry is never a maximum while a number is left.
// ------------------------------------------------------------------------------------------------
struct MgArgs {
    const float* U32;         // m x C of graph 0
    const int64_t* other;     // m of graph 0, or NULL
    float* gbar;              // m x C, or NULL
    double* row_margin;       // m, or NULL
    int64_t* label;           // m, or NULL
    int64_t* second;          // m, or NULL
    int m, C;
    size_t ws;                // byte stride of U32 between graphs (the workspace block)
    float ginv;               // float(1 / m)
};

// ce_load with an `other` that may be absent (-1: masked)
template <int LPR, int NPL>
__device__ __forceinline__ CeLoad<NPL> mg_load(const MgArgs& a, int i, int gl) {
    const float* u = a.U32 + size_t(i) * a.C;
    CeLoad<NPL> d;
    d.t = a.other ? a.other[i] : int64_t(-1);
#pragma unroll
    for (int q = 0; q < NPL; ++q) {
        const int c = gl + q * LPR;
        d.v[q] = c < a.C ? u[c] : -INFINITY;
    }
    return d;
}

// (v1, c1) ranks before (v2, c2): value descending, NaN after every number, index ascending.
// A total order on distinct indices; the empty slot is (NaN, INT_MAX), after every class.
__device__ __forceinline__ bool mg_before(float v1, int c1, float v2, int c2) {
    return v1 > v2 || (v1 == v2 && c1 < c2) || (v2 != v2 && (v1 == v1 || c1 < c2));
}

struct MgTop {
    float v1, v2;
    int c1, c2;   // c1 ranks before c2
};

__device__ __forceinline__ void mg_insert(MgTop& t, float v, int c) {
    if (mg_before(v, c, t.v1, t.c1)) {
        t.v2 = t.v1;
        t.c2 = t.c1;
        t.v1 = v;
        t.c1 = c;
    } else if (mg_before(v, c, t.v2, t.c2)) {
        t.v2 = v;
        t.c2 = c;
    }
}

// The head of row i from its loaded classes (all LPR lanes of the group call this together); the
// row's outputs are written here and the result (margin in .loss, moved in .hit) is the same on
// every lane of the group.
template <int LPR, int NPL>
__device__ __forceinline__ CeRow mg_row(const MgArgs& a, int i, int gl, const CeLoad<NPL>& d) {
    const int64_t t = d.t;
    const bool valid = t >= 0 && t < int64_t(a.C);
    MgTop top{NAN, NAN, INT_MAX, INT_MAX};
    float mine = 0.f;
#pragma unroll
    for (int q = 0; q < NPL; ++q) {
        const int c = gl + q * LPR;
        if (c < a.C) mg_insert(top, d.v[q], c);
        if (int64_t(c) == t) mine = d.v[q];
    }
#pragma unroll
    for (int o = LPR / 2; o > 0; o >>= 1) {   // two sorted pairs of disjoint classes into one
        const float ov1 = __shfl_xor(top.v1, o, LPR), ov2 = __shfl_xor(top.v2, o, LPR);
        const int oc1 = __shfl_xor(top.c1, o, LPR), oc2 = __shfl_xor(top.c2, o, LPR);
        mg_insert(top, ov1, oc1);
        mg_insert(top, ov2, oc2);
    }
    const int bc = top.c1;                          // C >= 1: a class, never the empty slot
    const int sc = top.c2 == INT_MAX ? 0 : top.c2;  // C = 1
    // the lane that holds class o_i hands U[i, o_i] to its group
    const float po = LPR > 1 ? __shfl(mine, valid ? int(t % LPR) : 0, LPR) : mine;
    CeRow r{0.0, 0};
    if (valid) {   // group-uniform
        const double dd = double(top.v1) - double(po);
        r.loss = (dd >= 0.0 || dd != dd) ? dd : 0.0;
        r.hit = int64_t(bc) == t;
    }
    if (a.gbar) {
        float* g = a.gbar + size_t(i) * a.C;
        const bool live = valid && !r.hit;
#pragma unroll
        for (int q = 0; q < NPL; ++q) {
            const int c = gl + q * LPR;
            if (c < a.C) g[c] = !live ? 0.f : c == bc ? a.ginv : int64_t(c) == t ? -a.ginv : 0.f;
        }
    }
    if (gl == 0) {
        if (a.row_margin) a.row_margin[i] = r.loss;
        if (a.label) a.label[i] = int64_t(bc);
        if (a.second) a.second[i] = int64_t(sc);
    }
    return r;
}

__device__ __forceinline__ void mg_to_graph(MgArgs& a, int g) {
    a.U32 = gshift_at(a.U32, a.ws, g);
    a.other = gshift_at(a.other, size_t(a.m) * sizeof(int64_t), g);
    a.gbar = gshift_at(a.gbar, size_t(a.m) * a.C * sizeof(float), g);
    a.row_margin = gshift_at(a.row_margin, size_t(a.m) * sizeof(double), g);
    a.label = gshift_at(a.label, size_t(a.m) * sizeof(int64_t), g);
    a.second = gshift_at(a.second, size_t(a.m) * sizeof(int64_t), g);
}

// The single-launch form (ce_head_kernel's): workgroup g is graph g, group q the rows q, q + G, ...
template <int LPR, int NPL>
__global__ __launch_bounds__(kCeThreads) void margin_head_kernel(MgArgs a,
                                                                 double* __restrict__ loss,
                                                                 int64_t* __restrict__ moved) {
    const int g = blockIdx.x;
    mg_to_graph(a, g);
    constexpr int G = kCeThreads / LPR;
    const int q = threadIdx.x / LPR, gl = threadIdx.x % LPR;
    double s = 0.0;
    int hits = 0;
    for (int i = q; i < a.m; i += G) {   // group-uniform trip count
        const CeRow r = mg_row<LPR, NPL>(a, i, gl, mg_load<LPR, NPL>(a, i, gl));
        s += r.loss;
        hits += r.hit;
    }
    if (gl != 0) {
        s = 0.0;
        hits = 0;
    }
    ce_finish<kCeThreads>(s, hits, a.m, g, loss, moved);
}

// Past kCeOneWg rows: one row per group into ce_rows_kernel's parts layout (m float64 margins, then
// m int32 moved flags a graph); ce_reduce_kernel sums them.
template <int LPR, int NPL>
__global__ __launch_bounds__(256) void margin_rows_kernel(MgArgs a, double* __restrict__ parts,
                                                          size_t pss) {
    const int g = blockIdx.y;
    mg_to_graph(a, g);
    parts = gshift_at(parts, pss, g);
    constexpr int G = 256 / LPR;
    const int gl = threadIdx.x % LPR;
    const int i = blockIdx.x * G + threadIdx.x / LPR;
    if (i >= a.m) return;   // group-uniform
    const CeRow r = mg_row<LPR, NPL>(a, i, gl, mg_load<LPR, NPL>(a, i, gl));
    if (gl == 0) {
        parts[i] = r.loss;
        reinterpret_cast<int*>(parts + a.m)[i] = r.hit;
    }
}

__global__ void margin_zero_kernel(double* __restrict__ loss, int64_t* __restrict__ moved, int B) {
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g < B) {
        loss[g] = 0.0;
        if (moved) moved[g] = 0;
    }
}

template <int LPR, int NPL>
static hipError_t launch_mg(const MgArgs& a, int B, double* loss, int64_t* moved, void* scratch,
                            hipStream_t s) {
    if (a.m <= kCeOneWg) {
        launch_k(margin_head_kernel<LPR, NPL>, dim3(B), kCeThreads, 0, s, a, loss, moved);
        return launch_status("loss.hip:margin_head_kernel");
    }
    const size_t pss = ce_parts_stride(a.m);
    double* parts = static_cast<double*>(scratch);
    constexpr unsigned G = 256 / LPR;
    prof_span(2);
    launch_k(margin_rows_kernel<LPR, NPL>, dim3((unsigned(a.m) + G - 1) / G, B), 256, 0, s, a,
             parts, pss);
    hipError_t e = launch_status("loss.hip:margin_rows_kernel");
    if (e != hipSuccess) return e;
    launch_k(ce_reduce_kernel, dim3(B), 256, 0, s, static_cast<const double*>(parts), pss, a.m,
             loss, moved);
    return launch_status("loss.hip:ce_reduce_kernel");
}

hipError_t launch_margin_head(const Layout& L, int B, void* ws, const int64_t* other, double* loss,
                              float* gbar, double* row_margin, int64_t* label, int64_t* second,
                              int64_t* moved, void* scratch, hipStream_t s) {
    prof_begin(GLL_K_LOSS, s);
    hipError_t e;
    if (L.m == 0) {   // no unlabeled row: loss = 0, moved = 0, nothing else
        launch_k(margin_zero_kernel, dim3((unsigned(B) + 255) / 256), 256, 0, s, loss, moved, B);
        e = launch_status("loss.hip:margin_zero_kernel");
    } else {
        MgArgs a;
        a.U32 = L.at<float>(ws, L.P) + size_t(L.base) * L.C;
        a.other = other;
        a.gbar = gbar;
        a.row_margin = row_margin;
        a.label = label;
        a.second = second;
        a.m = L.m;
        a.C = L.C;
        a.ws = L.total;
        a.ginv = float(1.0 / double(L.m));
        // the ce head's lanes per row x classes per lane
        if (L.C <= 4) e = launch_mg<1, 4>(a, B, loss, moved, scratch, s);
        else if (L.C <= 16) e = launch_mg<1, 16>(a, B, loss, moved, scratch, s);
        else if (L.C <= 128) e = launch_mg<16, 8>(a, B, loss, moved, scratch, s);
        else e = launch_mg<64, 4>(a, B, loss, moved, scratch, s);
    }
    prof_end(GLL_K_LOSS, s);
    return e;
}

// ------------------------------------------------------------------------------------------------
// The score/objective head: the cross-entropy head plus the two regularisers the reference's
// callers take from the same predictions (losses.py:100-101 entropy, :111-112 l2), the per-row
// scores of FullySup.py:165-173 and their scatter into the caller's score store.  Same U32, same
// row-holding scheme, same sums as the heads above.  In float64, u_c = double(U32[i, c]):
//     p_i   = u_{t_i} + 1e-8;   ce_i = -log(p_i)         (target outside [0, C): masked, ce_i = 0)
//     ent_i = -sum_c u_c log(u_c + 1e-8);   sq_i = sum_c u_c^2;   row_l2_i = 1 - sq_i
//     r_i   = w_ce ce_i + w_ent ent_i - w_l2 sq_i        (a term of weight 0 is left out)
//     loss  = (sum_i r_i) / m
//     gbar[i, c] = float(-(1/m) (w_ce [c == t_i] / p_i + w_ent (log(u_c + 1e-8) + u_c / (u_c + 1e-8))
//                               + w_l2 2 u_c))
// The row sums over c run lane by lane in ascending c, then a butterfly over the row's lanes; the
// sum over rows is the cross-entropy head's, fed r_i: with w = (1, 0, 0) r_i is ce_i and every
// output is bitwise that head's.  Masking touches the ce term, row_ce and correct alone.
// Scatter (score_kind 1: ce_i, 2: row_l2_i): an unmasked row whose index lies in [0, score_len)
// stores float(score_i) at score_out[index]; the index forms an address only after that test.
// ------------------------------------------------------------------------------------------------
struct ObArgs {
    const float* U32;         // m x C of graph 0
    const int64_t* targets;   // m of graph 0, or NULL (every row masked)
    float* gbar;              // m x C, or NULL
    double* row_ce;           // m, or NULL
    double* row_ent;          // m, or NULL
    double* ent_aside;        // m: row_entropy when helper workgroups write it (then row_ent is NULL)
    double* row_l2;           // m, or NULL
    int64_t* pred;            // m, or NULL
    float* score_out;        // score_len, shared by the graphs of a batch; NULL when kind == 0
    const int64_t* indices;   // m of graph 0; NULL when kind == 0
    int64_t score_len;
    int m, C, kind;
    size_t ws;                // byte stride of U32 between graphs (the workspace block)
    double ginv;              // -(1 / m)
    double wce, went, wl2;
};

// mg_load for ObArgs: targets may be absent (-1: masked)
template <int LPR, int NPL>
__device__ __forceinline__ CeLoad<NPL> ob_load(const ObArgs& a, int i, int gl) {
    const float* u = a.U32 + size_t(i) * a.C;
    CeLoad<NPL> d;
    d.t = a.targets ? a.targets[i] : int64_t(-1);
#pragma unroll
    for (int q = 0; q < NPL; ++q) {
        const int c = gl + q * LPR;
        d.v[q] = c < a.C ? u[c] : -INFINITY;
    }
    return d;
}

// The head of row i from its loaded classes (all LPR lanes of the group call this together); the
// row's outputs are written here and the result (r_i in .loss) is the same on every lane of the
// group.  Label, target pick and the ce term are ce_row's, statement by statement.
template <int LPR, int NPL>
__device__ __forceinline__ CeRow ob_row(const ObArgs& a, int i, int gl, const CeLoad<NPL>& d) {
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
    const float pt = LPR > 1 ? __shfl(mine, valid ? int(t % LPR) : 0, LPR) : mine;
    // the row sums over the classes: what is neither weighted nor asked for is not evaluated
    const bool need_ent = a.went != 0.0 || a.row_ent != nullptr;
    const bool need_sq = a.wl2 != 0.0 || a.row_l2 != nullptr || a.kind == 2;
    const bool ent_grad = a.went != 0.0 && a.gbar != nullptr;
    double lg[NPL] = {};   // log(u_c + 1e-8), kept for gbar
    double ent = 0.0, sq = 0.0;
    if (need_ent || need_sq) {   // uniform over the launch
#pragma unroll
        for (int q = 0; q < NPL; ++q) {
            const int c = gl + q * LPR;
            if (c < a.C) {
                const double u = double(d.v[q]);
                if (need_ent) {
                    lg[q] = log(u + 1e-8);
                    ent -= u * lg[q];
                }
                if (need_sq) sq += u * u;
            }
        }
#pragma unroll
        for (int o = LPR / 2; o > 0; o >>= 1) {
            ent += __shfl_xor(ent, o, LPR);
            sq += __shfl_xor(sq, o, LPR);
        }
    }
    CeRow r{0.0, 0};
    double ce = 0.0, gv = 0.0;
    if (valid) {   // group-uniform
        const double p = double(pt) + 1e-8;
        ce = -log(p);
        if (a.wce != 0.0) {
            r.loss = a.wce * ce;
            gv = (a.wce * a.ginv) / p;
        }
        r.hit = int64_t(bc) == t;
    }
    if (a.went != 0.0) r.loss += a.went * ent;
    if (a.wl2 != 0.0) r.loss -= a.wl2 * sq;
    if (a.gbar) {
        float* g = a.gbar + size_t(i) * a.C;
        const double ge = a.went * a.ginv, g2 = a.wl2 * a.ginv;
#pragma unroll
        for (int q = 0; q < NPL; ++q) {
            const int c = gl + q * LPR;
            if (c < a.C) {
                const double u = double(d.v[q]);
                double gc = (valid && int64_t(c) == t) ? gv : 0.0;
                if (ent_grad) gc += ge * (lg[q] + u / (u + 1e-8));
                if (a.wl2 != 0.0) gc += g2 * (2.0 * u);
                g[c] = float(gc);
            }
        }
    }
    if (gl == 0) {
        if (a.row_ce) a.row_ce[i] = ce;
        if (a.row_ent) a.row_ent[i] = ent;
        if (a.row_l2) a.row_l2[i] = 1.0 - sq;
        if (a.pred) a.pred[i] = int64_t(bc);
        if (a.kind != 0 && valid) {
            const int64_t at = a.indices[i];
            if (at >= 0 && at < a.score_len)
                a.score_out[at] = float(a.kind == 1 ? ce : 1.0 - sq);
        }
    }
    return r;
}

__device__ __forceinline__ void ob_to_graph(ObArgs& a, int g) {
    a.U32 = gshift_at(a.U32, a.ws, g);
    a.targets = gshift_at(a.targets, size_t(a.m) * sizeof(int64_t), g);
    a.gbar = gshift_at(a.gbar, size_t(a.m) * a.C * sizeof(float), g);
    a.row_ce = gshift_at(a.row_ce, size_t(a.m) * sizeof(double), g);
    a.row_ent = gshift_at(a.row_ent, size_t(a.m) * sizeof(double), g);
    a.ent_aside = gshift_at(a.ent_aside, size_t(a.m) * sizeof(double), g);
    a.row_l2 =gshift_at(a.row_l2, size_t(a.m) * sizeof(double), g);
    a.pred = gshift_at(a.pred, size_t(a.m) * sizeof(int64_t), g);
    a.indices = gshift_at(a.indices, size_t(a.m) * sizeof(int64_t), g);
}

// row_entropy alone, by helper workgroup hb of H: group q takes the rows hb * G + q, + H * G, ...
// The C float64 logs of a row are the head's whole arithmetic cost (one workgroup spends as long
// on them as on everything else); when the entropy is an output but no term of the loss
// (w_ent == 0: the reference's score mode) they run on other CUs beside the head's workgroup.
// Per row the same sums in the same order as ob_row's.
template <int LPR, int NPL>
__device__ __forceinline__ void ob_entropy_rows(const ObArgs& a, int hb, int H) {
    constexpr int G = kCeThreads / LPR;
    const int q = threadIdx.x / LPR, gl = threadIdx.x % LPR;
    for (int i = hb * G + q; i < a.m; i += H * G) {   // group-uniform trip count
        const float* u = a.U32 + size_t(i) * a.C;
        float v[NPL];
#pragma unroll
        for (int k = 0; k < NPL; ++k) {
            const int c = gl + k * LPR;
            v[k] = c < a.C ? u[c] : 0.f;
        }
        double ent = 0.0;
#pragma unroll
        for (int k = 0; k < NPL; ++k) {
            if (gl + k * LPR < a.C) {
                const double x = double(v[k]);
                ent -= x * log(x + 1e-8);
            }
        }
#pragma unroll
        for (int o = LPR / 2; o > 0; o >>= 1) ent += __shfl_xor(ent, o, LPR);
        if (gl == 0) a.ent_aside[i] = ent;
    }
}

constexpr int kObHelpers = 32;   // helper workgroups a graph may get

// The single-launch form (ce_head_kernel's): workgroup (g, 0) is graph g, group q the rows q,
// q + G, ...; workgroups (g, 1 ..) are its entropy helpers, when the launcher asked for any.
template <int LPR, int NPL>
__global__ __launch_bounds__(kCeThreads) void objective_head_kernel(ObArgs a,
                                                                    double* __restrict__ loss,
                                                                    int64_t* __restrict__ correct) {
    const int g = blockIdx.x;
    ob_to_graph(a, g);
    if (blockIdx.y > 0) {   // workgroup-uniform
        ob_entropy_rows<LPR, NPL>(a, int(blockIdx.y) - 1, int(gridDim.y) - 1);
        return;
    }
    constexpr int G = kCeThreads / LPR;
    const int q = threadIdx.x / LPR, gl = threadIdx.x % LPR;
    double s = 0.0;
    int hits = 0;
    for (int i = q; i < a.m; i += G) {   // group-uniform trip count
        const CeRow r = ob_row<LPR, NPL>(a, i, gl, ob_load<LPR, NPL>(a, i, gl));
        s += r.loss;
        hits += r.hit;
    }
    if (gl != 0) {
        s = 0.0;
        hits = 0;
    }
    ce_finish<kCeThreads>(s, hits, a.m, g, loss, correct);
}

// Past kCeOneWg rows: one row per group into ce_rows_kernel's parts layout (m float64 r_i, then m
// int32 hit flags a graph); ce_reduce_kernel sums them.
template <int LPR, int NPL>
__global__ __launch_bounds__(256) void objective_rows_kernel(ObArgs a, double* __restrict__ parts,
                                                             size_t pss) {
    const int g = blockIdx.y;
    ob_to_graph(a, g);
    parts = gshift_at(parts, pss, g);
    constexpr int G = 256 / LPR;
    const int gl = threadIdx.x % LPR;
    const int i = blockIdx.x * G + threadIdx.x / LPR;
    if (i >= a.m) return;   // group-uniform
    const CeRow r = ob_row<LPR, NPL>(a, i, gl, ob_load<LPR, NPL>(a, i, gl));
    if (gl == 0) {
        parts[i] = r.loss;
        reinterpret_cast<int*>(parts + a.m)[i] = r.hit;
    }
}

template <int LPR, int NPL>
static hipError_t launch_ob(const ObArgs& a, int B, double* loss, int64_t* correct, void* scratch,
                            hipStream_t s) {
    if (a.m <= kCeOneWg) {
        ObArgs k = a;
        unsigned H = 0;
        if (a.went == 0.0 && a.row_ent) {   // the entropy is an output only: helpers write it
            constexpr int G = kCeThreads / LPR;
            H = unsigned(std::min(kObHelpers, (a.m + G - 1) / G));
            k.ent_aside = a.row_ent;
            k.row_ent = nullptr;
        }
        launch_k(objective_head_kernel<LPR, NPL>, dim3(B, 1 + H), kCeThreads, 0, s, k, loss,
                 correct);
        return launch_status("loss.hip:objective_head_kernel");
    }
    const size_t pss = ce_parts_stride(a.m);
    double* parts = static_cast<double*>(scratch);
    constexpr unsigned G = 256 / LPR;
    prof_span(2);
    launch_k(objective_rows_kernel<LPR, NPL>, dim3((unsigned(a.m) + G - 1) / G, B), 256, 0, s, a,
             parts, pss);
    hipError_t e = launch_status("loss.hip:objective_rows_kernel");
    if (e != hipSuccess) return e;
    launch_k(ce_reduce_kernel, dim3(B), 256, 0, s, static_cast<const double*>(parts), pss, a.m,
             loss, correct);
    return launch_status("loss.hip:ce_reduce_kernel");
}

hipError_t launch_objective_head(const Layout& L, int B, void* ws, const int64_t* targets,
                                 double w_ce, double w_ent, double w_l2, double* loss, float* gbar,
                                 double* row_ce, double* row_entropy, double* row_l2,
                                 int64_t* pred_label, int64_t* correct, int score_kind,
                                 float* score_out, int64_t score_len, const int64_t* indices,
                                 void* scratch, hipStream_t s) {
    prof_begin(GLL_K_LOSS, s);
    hipError_t e;
    if (L.m == 0) {   // no unlabeled row: loss = 0, nothing else
        launch_k(ce_zero_kernel, dim3((unsigned(B) + 255) / 256), 256, 0, s, loss, B);
        e = launch_status("loss.hip:ce_zero_kernel");
    } else {
        ObArgs a;
        a.U32 = L.at<float>(ws, L.P) + size_t(L.base) * L.C;
        a.targets = targets;
        a.gbar = gbar;
        a.row_ce = row_ce;
        a.row_ent = row_entropy;
        a.ent_aside = nullptr;
        a.row_l2 = row_l2;
        a.pred = pred_label;
        a.score_out = score_kind ? score_out : nullptr;
        a.indices = score_kind ? indices : nullptr;
        a.score_len = score_len;
        a.m = L.m;
        a.C = L.C;
        a.kind = score_kind;
        a.ws = L.total;
        a.ginv = -(1.0 / double(L.m));
        a.wce = w_ce;
        a.went = w_ent;
        a.wl2 = w_l2;
        // the ce head's lanes per row x classes per lane
        if (L.C <= 4) e = launch_ob<1, 4>(a, B, loss, correct, scratch, s);
        else if (L.C <= 16) e = launch_ob<1, 16>(a, B, loss, correct, scratch, s);
        else if (L.C <= 128) e = launch_ob<16, 8>(a, B, loss, correct, scratch, s);
        else e = launch_ob<64, 4>(a, B, loss, correct, scratch, s);
    }
    prof_end(GLL_K_LOSS, s);
    return e;
}

}  // namespace gll
