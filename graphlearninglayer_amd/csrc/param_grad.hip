// param_grad.hip -- gradients of the Laplace-learning layer with respect to label_matrix, tau
// and a fixed epsilon (the reference returns None for all three, GLL.py:177).
//
// After gll_backward the workspace holds P = [Y; U], w = [0; Luu^-1 gbar] (Layout::Wadj) and the
// symmetric rows, and for a frozen kNN graph
//     grad_Y[j, c] = sum_{i in N(j)} W_ji w_ic                      (rows j < base)
//     grad_tau     = - sum_{i >= base, c} w_ic U_ic
//     grad_eps     = 4 / eps^3 * sum_{directed edges e = (i, j)} G_e W_e d_e^2     (fixed eps)
// with G_ij = sum_c (w_ic - w_jc)(P_jc - P_ic) as in grad_common.h (every undirected edge is
// stored in both rows: half of 8 / eps^3).  One pass over the rows (param_grad_kernel) writes
// grad_Y and one float64 partial per row and scalar; param_reduce_kernel sums each graph's
// partials in a fixed order.  No atomics: the results are bitwise reproducible, and graph g of
// a batch equals the single call (a row's partial and the order of the second stage depend on
// the problem alone, never on B).
#include "gll_internal.h"
#include "grad_common.h"

namespace gll {

// G_ij alone, in the register form of edge_gv_r (same loads, same fma order)
template <int CV>
__device__ __forceinline__ float edge_g_r(const EdgeArgs& a, const RowWP<CV < 0 ? -CV : CV>& ri,
                                          int j) {
    constexpr int N = CV < 0 ? -CV : CV;
    float wv[N], pv[N];
    load_wp<CV>(a, j, wv, pv);
    float g = 0.f;
#pragma unroll
    for (int c = 0; c < N; ++c)
        if (CV < 0 || c < a.C) g = __builtin_fmaf(ri.w[c] - wv[c], pv[c] - ri.p[c], g);
    return g;
}

// LPR lanes per row, 64 / LPR rows per wave, four waves per workgroup (edge_coef_kernel's
// shape).  `what`: GLL_PG_* bits.  parts: per graph, n float64 row partials of the tau sum
// followed by n of the eps sum (`pss` bytes a graph); gradY: base x C fp32 (`gys` bytes a graph).
template <int CV, int LPR>
__global__ __launch_bounds__(256) void param_grad_kernel(EdgeArgs a, int what, int nrows,
                                                         float* __restrict__ gradY, size_t gys,
                                                         double* __restrict__ parts, size_t pss) {
    const int g = bg();
    a.to_graph_at(g);
    gradY = gshift_at(gradY, gys, g);
    parts = gshift_at(parts, pss, g);
    constexpr int RPW = kWave / LPR;
    const int lane = lane_id();
    const int gl = lane % LPR;
    const int i = bx() * (4 * RPW) + (threadIdx.x >> 6) * RPW + lane / LPR;
    const bool live = i < nrows;   // nrows <= n
    const int ic = live ? i : 0;
    const int beg = live ? a.row_start[ic] : 0;
    const int end = live ? beg + a.row_len[ic] : 0;   // hub rows: any length (bump region)

    // eps: sum_e G_e W_e d_e^2 of this row, float64 from the per-edge fp32 term on
    if (what & GLL_PG_EPS) {
        double part = 0.0;
        if constexpr (CV != 0) {
            const auto ri = row_wp<CV>(a, ic);
            for (int e = beg + gl; e < end; e += LPR)
                part += double(edge_g_r<CV>(a, ri, a.col[e]) * a.w[e] * a.d2[e]);
        } else {
            for (int e = beg + gl; e < end; e += LPR) {
                float gv;
                (void)edge_gv(a, ic, a.col[e], a.w[e], 1.f, gv);
                part += double(gv * a.w[e] * a.d2[e]);
            }
        }
#pragma unroll
        for (int o = LPR / 2; o > 0; o >>= 1) part += __shfl_xor(part, o, LPR);
        if (live && gl == 0) parts[size_t(a.n) + i] = part;
    }

    // tau: sum_c w_ic U_ic of an unlabeled row (0 for a labeled one)
    if (what & GLL_PG_TAU) {
        double part = 0.0;
        if (live && i >= a.base) {
            const float* wi = a.Wadj + size_t(i) * a.C;
            const float* pi = a.P + size_t(i) * a.C;
            for (int c = gl; c < a.C; c += LPR) part = __builtin_fma(double(wi[c]), double(pi[c]), part);
        }
#pragma unroll
        for (int o = LPR / 2; o > 0; o >>= 1) part += __shfl_xor(part, o, LPR);
        if (live && gl == 0) parts[i] = part;
    }

    // label_matrix: grad_Y[i, c] = sum_e W_e w[col_e, c] over the row's entries in ascending
    // entry order.  Lanes first own entries (col, W), then classes; an entry reaches the
    // group's lanes by a width-LPR shuffle (the group's lanes run the loops together: the trip
    // counts depend on the row and on C alone).
    if ((what & GLL_PG_Y) && a.base > 0) {
        const bool lab = live && i < a.base;
        const int lend = lab ? end : beg;   // unlabeled rows: no entries
        for (int c0 = 0; c0 < a.C; c0 += LPR) {
            const int c = c0 + gl;
            const int cc = c < a.C ? c : 0;
            float acc = 0.f;
            for (int e0 = beg; e0 < lend; e0 += LPR) {
                const int e = e0 + gl;
                const bool in = e < lend;
                const int cj = in ? a.col[e] : ic;
                const float cw = in ? a.w[e] : 0.f;
                const int cnt = min(LPR, lend - e0);
                for (int t = 0; t < cnt; ++t) {
                    const int j = __shfl(cj, t, LPR);
                    const float wv = __shfl(cw, t, LPR);
                    acc = __builtin_fmaf(wv, a.Wadj[size_t(j) * a.C + cc], acc);
                }
            }
            if (lab && c < a.C) gradY[size_t(i) * a.C + c] = acc;
        }
    }
}

// Second stage: workgroup (q, g) sums graph g's n row partials of scalar q (0 tau, 1 eps) --
// thread t the rows t, t + 256, ... in ascending order, then a fixed LDS tree -- and writes
// -sum (tau) or 4 / eps^3 * sum (eps).
__global__ __launch_bounds__(256) void param_reduce_kernel(const double* __restrict__ parts,
                                                           size_t pss, int n, int what,
                                                           double eps_scale,
                                                           double* __restrict__ grad_tau,
                                                           double* __restrict__ grad_eps) {
    __shared__ double red[256];
    const int q = blockIdx.x, g = blockIdx.y;
    if (!(what & (q == 0 ? GLL_PG_TAU : GLL_PG_EPS))) return;   // workgroup-uniform
    const double* src = gshift_at(parts, pss, g) + size_t(q) * n;
    double s = 0.0;
    for (int r = threadIdx.x; r < n; r += 256) s += src[r];
    red[threadIdx.x] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (int(threadIdx.x) < o) red[threadIdx.x] += red[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        if (q == 0) grad_tau[g] = -red[0];
        else grad_eps[g] = eps_scale * red[0];
    }
}

template <int CV>
static void launch_param(const EdgeArgs& a, int B, int lpr, int what, int nrows, float* gradY,
                         size_t gys, double* parts, size_t pss, hipStream_t s) {
    const unsigned rows = 4u * unsigned(kWave / lpr);
    const dim3 grid((unsigned(nrows) + rows - 1) / rows, B);
    if (lpr == 16)
        launch_k(param_grad_kernel<CV, 16>, grid, 256, 0, s, a, what, nrows, gradY, gys, parts, pss);
    else
        launch_k(param_grad_kernel<CV, 32>, grid, 256, 0, s, a, what, nrows, gradY, gys, parts, pss);
}

size_t param_grad_scratch_bytes(int n, int B) {
    return size_t(B) * ((size_t(2) * n * sizeof(double) + 255) & ~size_t(255));
}

hipError_t launch_param_grad(const Layout& L, int B, void* ws, float eps_fixed, int what,
                             float* gradY, double* grad_tau, double* grad_eps, void* scratch,
                             hipStream_t s) {
    const bool scalars = what & (GLL_PG_TAU | GLL_PG_EPS);
    // label gradients alone need only the labeled rows
    const int nrows = scalars ? L.n : L.base;
    if (nrows == 0) return hipSuccess;
    const EdgeArgs a = make_edge_args(L, L.total, ws, (what & GLL_PG_EPS) ? eps_fixed : 1.f);
    const size_t pss = param_grad_scratch_bytes(L.n, 1);
    const size_t gys = size_t(L.base) * L.C * sizeof(float);
    double* parts = static_cast<double*>(scratch);
    const int lpr = L.K <= 40 ? 16 : 32;   // as edge_coef_kernel (grad.hip)
    prof_begin(GLL_K_PARAM, s);
    prof_span(scalars ? 2 : 1);
    switch (L.C) {   // even C <= 16: exact count, paired loads; else a bound, or the loop
        case 2: launch_param<-2>(a, B, lpr, what, nrows, gradY, gys, parts, pss, s); break;
        case 4: launch_param<-4>(a, B, lpr, what, nrows, gradY, gys, parts, pss, s); break;
        case 6: launch_param<-6>(a, B, lpr, what, nrows, gradY, gys, parts, pss, s); break;
        case 8: launch_param<-8>(a, B, lpr, what, nrows, gradY, gys, parts, pss, s); break;
        case 10: launch_param<-10>(a, B, lpr, what, nrows, gradY, gys, parts, pss, s); break;
        case 12: launch_param<-12>(a, B, lpr, what, nrows, gradY, gys, parts, pss, s); break;
        case 14: launch_param<-14>(a, B, lpr, what, nrows, gradY, gys, parts, pss, s); break;
        case 16: launch_param<-16>(a, B, lpr, what, nrows, gradY, gys, parts, pss, s); break;
        default:
            if (L.C <= 4) launch_param<4>(a, B, lpr, what, nrows, gradY, gys, parts, pss, s);
            else if (L.C <= 8) launch_param<8>(a, B, lpr, what, nrows, gradY, gys, parts, pss, s);
            else if (L.C <= 16) launch_param<16>(a, B, lpr, what, nrows, gradY, gys, parts, pss, s);
            else launch_param<0>(a, B, lpr, what, nrows, gradY, gys, parts, pss, s);
    }
    hipError_t e = launch_status("param_grad.hip:param_grad_kernel");
    if (e == hipSuccess && scalars) {
        const double ed = double(eps_fixed);
        launch_k(param_reduce_kernel, dim3(2, B), 256, 0, s, static_cast<const double*>(parts), pss,
                 L.n, what, 4.0 / (ed * ed * ed), grad_tau, grad_eps);
        e = launch_status("param_grad.hip:param_reduce_kernel");
    }
    prof_end(GLL_K_PARAM, s);
    return e;
}

}  // namespace gll
