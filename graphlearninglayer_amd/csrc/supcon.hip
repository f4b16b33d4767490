// supcon.hip -- fused SupCon / SimCLR loss (include/gll.h gll_supcon_*).
//
// The R x R logits l_rj = (z_r . z_j) / T are consumed tile by tile and never stored.  A
// workgroup of kScWaves waves owns kScRows anchor rows (one 32-row tile per wave) and one chunk
// of 32-column tiles; each 32 x 32 logits tile is one chain of v_mfma_f32_32x32x2_f32 oriented
// as Z_j . Z_r^T, so a lane owns ONE anchor (its column, lane & 31) and holds 16 of the tile's
// columns j in its accumulator registers (j = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)).  The
// forward leaves per (chunk, row) the partial (max, sum exp, sum of positive logits, positive
// count) and a one-workgroup second stage combines them in ascending chunk order.  The backward
// recomputes the tile, forms h_rj = q_rj + q_jr in those same registers and feeds them as the A
// operand of a second fp32 MFMA (sum over the accumulator's register index: no LDS transpose)
// that accumulates gZ_r += sum_j h_rj z_j; chunk partials go to scratch and a second stage sums
// them in ascending chunk order (a single chunk writes gZ itself).  No atomics; every sum order depends on (R, V, d, mode) alone.
#include <atomic>

#include "gll_internal.h"

namespace gll {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int kScThreads = kScWaves * kWave;
constexpr int kScLd = kScKc + 4;   // LDS row stride (floats): 16-B aligned rows, banks staggered
constexpr int kScSlabs = kScKc / 32;
constexpr int kScReduceThreads = 1024;

static std::atomic<int64_t> g_sc_launches{0};

int64_t supcon_launches() { return g_sc_launches.load(std::memory_order_relaxed); }

ScPlan supcon_plan(int64_t rows, int d) {
    ScPlan p;
    p.ntiles = int((rows + kScTile - 1) / kScTile);
    p.rowblocks = int((rows + kScRows - 1) / kScRows);
    const int64_t per = rows * (int64_t(d) * 4 + kScPartBytes);   // scratch bytes of one chunk
    int64_t budget = 2 * rows * rows;
    if (budget < kScMinBudget) budget = kScMinBudget;
    int64_t nc = (kScTargetWg + p.rowblocks - 1) / p.rowblocks;
    if (nc > budget / per) nc = budget / per;
    if (nc > p.ntiles) nc = p.ntiles;
    if (nc < 1) nc = 1;
    p.tpc = int((p.ntiles + nc - 1) / nc);
    p.chunks = (p.ntiles + p.tpc - 1) / p.tpc;
    // the forward's partials are 32 B a row: finer chunks, several waves on every SIMD
    int64_t nf = (kScTargetWgFwd + p.rowblocks - 1) / p.rowblocks;
    if (nf > p.ntiles) nf = p.ntiles;
    p.ftpc = int((p.ntiles + nf - 1) / nf);
    p.fchunks = (p.ntiles + p.ftpc - 1) / p.ftpc;
    return p;
}

size_t supcon_scratch_bytes(int64_t rows, int d) {
    const ScPlan p = supcon_plan(rows, d);
    // one chunk: the backward writes gZ itself and keeps no partials
    return size_t(p.fchunks) * size_t(rows) * kScPartBytes +
           (p.chunks > 1 ? size_t(p.chunks) * size_t(rows) * size_t(d) * 4 : 0);
}

// Column (mode 'all') or anchor partial of one row: running maximum, sum of exp(l - m) over
// j != r, sum of the positives' logits, their count.  E and P are float64: the only fp32
// roundings of a row's statistics are those of the logits and of expf.
struct ScPart {
    float m;
    double E, P;
    int c;
};

__device__ inline double sc_term(float mi, double Ei, float m) {
    return mi == -INFINITY ? 0.0 : Ei * double(expf(mi - m));
}

// a then b, in that order
__device__ inline ScPart sc_combine(const ScPart& a, const ScPart& b) {
    ScPart o;
    o.m = fmaxf(a.m, b.m);
    o.E = sc_term(a.m, a.E, o.m) + sc_term(b.m, b.E, o.m);
    o.P = a.P + b.P;
    o.c = a.c + b.c;
    return o;
}

// rows row0 .. row0 + nrows - 1, features k0 .. k0 + kScKc - 1 of Z into dst[nrows][kScLd],
// zero past R and past d
template <bool VEC>
__device__ inline void sc_stage(float* dst, const float* __restrict__ Z, int64_t R, int d,
                                int64_t row0, int nrows, int k0) {
    if constexpr (VEC) {
        for (int e = threadIdx.x; e < nrows * (kScKc / 4); e += kScThreads) {
            const int rr = e / (kScKc / 4), k = (e % (kScKc / 4)) * 4;
            const int64_t row = row0 + rr;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (row < R && k0 + k < d)   // d % 4 == 0: a group is inside the row or past it
                v = *reinterpret_cast<const float4*>(Z + size_t(row) * d + k0 + k);
            *reinterpret_cast<float4*>(dst + rr * kScLd + k) = v;
        }
    } else {
        for (int e = threadIdx.x; e < nrows * kScKc; e += kScThreads) {
            const int rr = e / kScKc, k = e % kScKc;
            const int64_t row = row0 + rr;
            dst[rr * kScLd + k] = (row < R && k0 + k < d) ? Z[size_t(row) * d + k0 + k] : 0.f;
        }
    }
}

// The same 16-B groups of one column tile (features 0 .. kScKc - 1) into registers and, a
// barrier later, from them into LDS: the next tile's loads fly under this tile's arithmetic.
constexpr int kScPre = kScTile * (kScKc / 4) / kScThreads;

__device__ inline void sc_prefetch(float4 (&pre)[kScPre], const float* __restrict__ Z, int64_t R,
                                   int d, int64_t row0) {
#pragma unroll
    for (int n = 0; n < kScPre; ++n) {
        const int e = threadIdx.x + n * kScThreads;
        const int rr = e / (kScKc / 4), k = (e % (kScKc / 4)) * 4;
        const int64_t row = row0 + rr;
        pre[n] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (row < R && k < d) pre[n] = *reinterpret_cast<const float4*>(Z + size_t(row) * d + k);
    }
}

__device__ inline void sc_commit(float* dst, const float4 (&pre)[kScPre]) {
#pragma unroll
    for (int n = 0; n < kScPre; ++n) {
        const int e = threadIdx.x + n * kScThreads;
        *reinterpret_cast<float4*>(dst + (e / (kScKc / 4)) * kScLd + (e % (kScKc / 4)) * 4) = pre[n];
    }
}

// acc += Zj[32][k8] . Zr[32][k8]^T: rows j on the accumulator's register index, anchors r on
// the lane.  Lane (i, h) reads features 8 q + 4 h .. + 3 of its row of both tiles, so MFMA step
// (q, c) multiplies feature 8 q + c (lanes 0..31) and 8 q + 4 + c (lanes 32..63) of both.
__device__ inline void sc_dot(f32x16& acc, const float* zj, const float* zr, int k8, int i, int h) {
    const float* pa = zj + i * kScLd + 4 * h;
    const float* pb = zr + i * kScLd + 4 * h;
    for (int q = 0; q < k8; q += 8) {
        const float4 a = *reinterpret_cast<const float4*>(pa + q);
        const float4 b = *reinterpret_cast<const float4*>(pb + q);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, b.x, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, b.y, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, b.z, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, b.w, acc, 0, 0, 0);
    }
}

__device__ inline int sc_jloc(int t, int h) { return (t & 3) + 8 * (t >> 2) + 4 * h; }

struct alignas(16) ScShared {
    float zr[kScRows * kScLd];
    float zj[kScTile * kScLd];
    int64_t lab[kScTile];
    float mj[kScTile], iEj[kScTile], icj[kScTile];
    int anchj[kScTile];
};

// The logits tile of column tile jt against this wave's anchors (dot products, not yet / T).
// Leaves the tile's labels in sh.lab and, for d <= kScKc, its rows in sh.zj.  Ends after a
// barrier-free read phase: callers enter the next call through its leading __syncthreads.
// pf (16-B loads and d <= kScKc): the tile comes from `pre`, and the tile at jnext (< 0: none)
// is loaded into `pre` once the barrier has passed.
template <bool VEC, bool BWD>
__device__ inline f32x16 sc_logits(ScShared& sh, const float* __restrict__ Z,
                                   const int64_t* __restrict__ labels,
                                   const float* __restrict__ stats, int64_t R, int V, int d, int mode,
                                   int64_t r0, int64_t j0, int nk, int w, int i, int h,
                                   float4 (&pre)[kScPre], bool pf, int64_t jnext) {
    f32x16 acc;
#pragma unroll
    for (int t = 0; t < 16; ++t) acc[t] = 0.f;
    for (int kc = 0; kc < nk; ++kc) {
        __syncthreads();   // everyone is done with the buffers' previous contents
        const int k0 = kc * kScKc;
        if (nk > 1) sc_stage<VEC>(sh.zr, Z, R, d, r0, kScRows, k0);
        if (pf)
            sc_commit(sh.zj, pre);
        else
            sc_stage<VEC>(sh.zj, Z, R, d, j0, kScTile, k0);
        if (kc == 0 && threadIdx.x < kScTile) {
            const int64_t j = j0 + threadIdx.x;
            const bool in = j < R;
            sh.lab[threadIdx.x] = in ? (labels ? labels[j / V] : j / V) : 0;
            if constexpr (BWD) {
                sh.mj[threadIdx.x] = in ? stats[j * 4 + 0] : 0.f;
                sh.icj[threadIdx.x] = in ? 1.f / stats[j * 4 + 2] : 0.f;
                sh.iEj[threadIdx.x] = in ? stats[j * 4 + 3] : 0.f;
                sh.anchj[threadIdx.x] = in && (mode == GLL_SC_ALL || j % V == 0);
            }
        }
        __syncthreads();
        if (pf && jnext >= 0) sc_prefetch(pre, Z, R, d, jnext);
        const int rem = d - k0 < kScKc ? d - k0 : kScKc;
        sc_dot(acc, sh.zj, sh.zr + w * kScTile * kScLd, (rem + 7) & ~7, i, h);
    }
    return acc;
}

template <bool VEC>
__global__ __launch_bounds__(kScThreads) void supcon_fwd_kernel(
    const float* __restrict__ Z, const int64_t* __restrict__ labels, int64_t R, int V, int d,
    float T, int tpc, int ntiles, double* __restrict__ part) {
    __shared__ ScShared sh;
    const int w = threadIdx.x / kWave, l = threadIdx.x % kWave, i = l & 31, h = l >> 5;
    const int64_t r0 = int64_t(blockIdx.x) * kScRows;
    const int ch = blockIdx.y;
    const int nk = (d + kScKc - 1) / kScKc;
    const int64_t myr = r0 + w * kScTile + i;
    const int64_t mylab = myr < R ? (labels ? labels[myr / V] : myr / V) : 0;
    if (nk == 1) sc_stage<VEC>(sh.zr, Z, R, d, r0, kScRows, 0);

    ScPart p{-INFINITY, 0.0, 0.0, 0};
    const int jt1 = (ch + 1) * tpc < ntiles ? (ch + 1) * tpc : ntiles;
    const bool pf = VEC && nk == 1;
    float4 pre[kScPre];
    if (pf) sc_prefetch(pre, Z, R, d, int64_t(ch) * tpc * kScTile);
    for (int jt = ch * tpc; jt < jt1; ++jt) {
        const int64_t j0 = int64_t(jt) * kScTile;
        const f32x16 acc = sc_logits<VEC, false>(sh, Z, labels, nullptr, R, V, d, 0, r0, j0, nk, w, i, h,
                                                 pre, pf, jt + 1 < jt1 ? j0 + kScTile : -1);
        float lg[16];
        float tmax = -INFINITY;
#pragma unroll
        for (int t = 0; t < 16; ++t) {
            lg[t] = acc[t] / T;
            if (j0 + sc_jloc(t, h) < R) tmax = fmaxf(tmax, lg[t]);
        }
        if (tmax > p.m) {   // p.m = -inf: E is 0 and stays 0
            p.E *= double(expf(p.m - tmax));
            p.m = tmax;
        }
#pragma unroll
        for (int t = 0; t < 16; ++t) {
            const int jl = sc_jloc(t, h);
            const int64_t j = j0 + jl;
            if (j < R && j != myr) {
                p.E += double(expf(lg[t] - p.m));
                if (sh.lab[jl] == mylab) {
                    p.P += double(lg[t]);
                    ++p.c;
                }
            }
        }
    }
    // the two lane halves of an anchor, half 0 first
    ScPart o;
    o.m = __shfl_xor(p.m, 32);
    o.E = __shfl_xor(p.E, 32);
    o.P = __shfl_xor(p.P, 32);
    o.c = __shfl_xor(p.c, 32);
    const ScPart a = h == 0 ? sc_combine(p, o) : sc_combine(o, p);
    if (h == 0 && myr < R) {
        double* q = part + (size_t(ch) * size_t(R) + size_t(myr)) * 4;
        q[0] = double(a.m);
        q[1] = a.E;
        q[2] = a.P;
        q[3] = double(a.c);
    }
}

// Second stage of the forward, one workgroup: chunk partials in ascending order, the row's
// statistics and loss, and the anchors' losses summed in float64 (each thread its rows in
// ascending order, then a fixed tree over the threads).
__global__ __launch_bounds__(kScReduceThreads) void supcon_reduce_kernel(
    const double* __restrict__ part, int64_t R, int V, int chunks, int mode, double scale /* T/Tb */,
    double* __restrict__ loss, float* __restrict__ row_loss, float* __restrict__ stats) {
    __shared__ double red[kScReduceThreads];
    const int64_t bsz = R / V;
    double sum = 0.0;
    for (int64_t r = threadIdx.x; r < R; r += kScReduceThreads) {
        ScPart a{-INFINITY, 0.0, 0.0, 0};
        for (int ch = 0; ch < chunks; ++ch) {
            const double* q = part + (size_t(ch) * size_t(R) + size_t(r)) * 4;
            const ScPart b{float(q[0]), q[1], q[2], int(q[3])};
            a = sc_combine(a, b);
        }
        const double logE = log(a.E);
        const double rl = -scale * (a.P / double(a.c) - double(a.m) - logE);
        stats[r * 4 + 0] = a.m;
        stats[r * 4 + 1] = float(logE);
        stats[r * 4 + 2] = float(a.c);
        stats[r * 4 + 3] = float(1.0 / a.E);
        const int64_t b = r / V, v = r % V;
        if (mode == GLL_SC_ALL || v == 0) {
            sum += rl;
            if (row_loss) row_loss[mode == GLL_SC_ALL ? v * bsz + b : b] = float(rl);
        }
    }
    red[threadIdx.x] = sum;
    __syncthreads();
    for (int s = kScReduceThreads / 2; s > 0; s >>= 1) {
        if (int(threadIdx.x) < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) *loss = red[0] / double(mode == GLL_SC_ALL ? R : bsz);
}

template <bool VEC>
__global__ __launch_bounds__(kScThreads) void supcon_bwd_kernel(
    const float* __restrict__ Z, const int64_t* __restrict__ labels,
    const float* __restrict__ stats, int64_t R, int V, int d, int mode, float T, int tpc,
    int ntiles, float* __restrict__ gpart, double wgt, const double* __restrict__ grad_loss) {
    __shared__ ScShared sh;
    const int w = threadIdx.x / kWave, l = threadIdx.x % kWave, i = l & 31, h = l >> 5;
    const int64_t r0 = int64_t(blockIdx.x) * kScRows;
    const int ch = blockIdx.y;
    const int nk = (d + kScKc - 1) / kScKc;
    const int64_t myr = r0 + w * kScTile + i;
    const bool rin = myr < R;
    const int64_t mylab = rin ? (labels ? labels[myr / V] : myr / V) : 0;
    const float mr = rin ? stats[myr * 4 + 0] : 0.f;
    const float icr = rin ? 1.f / stats[myr * 4 + 2] : 0.f;
    const float iEr = rin ? stats[myr * 4 + 3] : 0.f;
    const bool anchr = rin && (mode == GLL_SC_ALL || myr % V == 0);
    if (nk == 1) sc_stage<VEC>(sh.zr, Z, R, d, r0, kScRows, 0);

    const int jt1 = (ch + 1) * tpc < ntiles ? (ch + 1) * tpc : ntiles;
    const bool pf = VEC && nk == 1;
    float4 pre[kScPre];
    if (pf) sc_prefetch(pre, Z, R, d, int64_t(ch) * tpc * kScTile);
    // feature groups of kScKc: the accumulators of one group live in registers over the chunk
    for (int g = 0; g < nk; ++g) {
        const int f0 = g * kScKc;
        const int nsl = ((d - f0 < kScKc ? d - f0 : kScKc) + 31) / 32;
        f32x16 gz[kScSlabs];
#pragma unroll
        for (int sl = 0; sl < kScSlabs; ++sl)
#pragma unroll
            for (int t = 0; t < 16; ++t) gz[sl][t] = 0.f;
        for (int jt = ch * tpc; jt < jt1; ++jt) {
            const int64_t j0 = int64_t(jt) * kScTile;
            const f32x16 acc = sc_logits<VEC, true>(sh, Z, labels, stats, R, V, d, mode, r0, j0, nk, w, i, h,
                                                    pre, pf, jt + 1 < jt1 ? j0 + kScTile : -1);
            float hv[16];
#pragma unroll
            for (int t = 0; t < 16; ++t) {
                const int jl = sc_jloc(t, h);
                const int64_t j = j0 + jl;
                const float lg = acc[t] / T;
                const float pos = sh.lab[jl] == mylab ? 1.f : 0.f;
                const float qr = expf(lg - mr) * iEr - pos * icr;
                const float qj = expf(lg - sh.mj[jl]) * sh.iEj[jl] - pos * sh.icj[jl];
                const float v = (anchr ? qr : 0.f) + (sh.anchj[jl] ? qj : 0.f);
                hv[t] = (rin && j < R && j != myr) ? v : 0.f;
            }
            // gz[r][f] += sum_j h[j][r] z_j[f]: A = the h tile (its row index j is the k of
            // this product: register t of lane half h is j = jloc(t, h)), B = rows j of Z
#pragma unroll
            for (int sl = 0; sl < kScSlabs; ++sl) {
                if (sl < nsl) {
#pragma unroll
                    for (int t = 0; t < 16; ++t) {
                        const int jl = sc_jloc(t, h);
                        float b;
                        if (nk == 1) {
                            b = sh.zj[jl * kScLd + sl * 32 + i];
                        } else {   // sh.zj holds the last feature chunk: read group g from memory
                            const int64_t j = j0 + jl;
                            const int f = f0 + sl * 32 + i;
                            b = (j < R && f < d) ? Z[size_t(j) * d + f] : 0.f;
                        }
                        gz[sl] = __builtin_amdgcn_mfma_f32_32x32x2f32(hv[t], b, gz[sl], 0, 0, 0);
                    }
                }
            }
        }
        // accumulator: feature on the lane, anchor row on the register index
#pragma unroll
        for (int sl = 0; sl < kScSlabs; ++sl) {
            const int f = f0 + sl * 32 + i;
            if (sl < nsl && f < d) {
#pragma unroll
                for (int t = 0; t < 16; ++t) {
                    const int64_t r = r0 + w * kScTile + sc_jloc(t, h);
                    if (r >= R) continue;
                    if (grad_loss)   // the only chunk: gpart is gZ
                        gpart[size_t(r) * d + f] = float(*grad_loss * wgt * double(gz[sl][t]));
                    else
                        gpart[(size_t(ch) * size_t(R) + size_t(r)) * d + f] = gz[sl][t];
                }
            }
        }
    }
}

// Second stage of the backward: chunk partials in ascending order (float64), times
// grad_loss / (A Tb), rounded once.
__global__ __launch_bounds__(256) void supcon_grad_reduce_kernel(
    const float* __restrict__ gpart, int64_t total /* R d */, int chunks, double w,
    const double* __restrict__ grad_loss, float* __restrict__ gZ) {
    const double gl = *grad_loss * w;
    for (int64_t e = int64_t(blockIdx.x) * 256 + threadIdx.x; e < total; e += int64_t(gridDim.x) * 256) {
        double s = 0.0;
        for (int ch = 0; ch < chunks; ++ch) s += double(gpart[size_t(ch) * size_t(total) + size_t(e)]);
        gZ[e] = float(gl * s);
    }
}

static bool sc_vec(const float* Z, int d) {
    return d % 4 == 0 && reinterpret_cast<uintptr_t>(Z) % 16 == 0;
}

static hipError_t sc_launched(const char* what) {
    g_sc_launches.fetch_add(1, std::memory_order_relaxed);
    return launch_status(what);
}

hipError_t launch_supcon_forward(int64_t R, int V, int d, const float* Z, const int64_t* labels,
                                 int mode, float T, float Tb, double* loss, float* row_loss,
                                 float* stats, void* scratch, hipStream_t s) {
    const ScPlan p = supcon_plan(R, d);
    double* part = static_cast<double*>(scratch);
    const dim3 grid(p.rowblocks, p.fchunks);
    if (sc_vec(Z, d))
        launch_k(supcon_fwd_kernel<true>, grid, dim3(kScThreads), 0, s, Z, labels, R, V, d, T, p.ftpc,
                 p.ntiles, part);
    else
        launch_k(supcon_fwd_kernel<false>, grid, dim3(kScThreads), 0, s, Z, labels, R, V, d, T, p.ftpc,
                 p.ntiles, part);
    hipError_t e = sc_launched("supcon.hip:supcon_fwd_kernel");
    if (e != hipSuccess) return e;
    launch_k(supcon_reduce_kernel, dim3(1), dim3(kScReduceThreads), 0, s,
             static_cast<const double*>(part), R, V, p.fchunks, mode, double(T) / double(Tb), loss,
             row_loss, stats);
    return sc_launched("supcon.hip:supcon_reduce_kernel");
}

hipError_t launch_supcon_backward(int64_t R, int V, int d, const float* Z, const int64_t* labels,
                                  int mode, float T, float Tb, const float* stats,
                                  const double* grad_loss, float* gZ, void* scratch, hipStream_t s) {
    const ScPlan p = supcon_plan(R, d);
    const bool direct = p.chunks == 1;
    float* gpart = direct ? gZ
                          : reinterpret_cast<float*>(static_cast<char*>(scratch) +
                                                     size_t(p.fchunks) * size_t(R) * kScPartBytes);
    const int64_t anchors = mode == GLL_SC_ALL ? R : R / V;
    const double wgt = 1.0 / (double(anchors) * double(Tb));
    const double* gl_direct = direct ? grad_loss : nullptr;
    const dim3 grid(p.rowblocks, p.chunks);
    if (sc_vec(Z, d))
        launch_k(supcon_bwd_kernel<true>, grid, dim3(kScThreads), 0, s, Z, labels, stats, R, V, d,
                 mode, T, p.tpc, p.ntiles, gpart, wgt, gl_direct);
    else
        launch_k(supcon_bwd_kernel<false>, grid, dim3(kScThreads), 0, s, Z, labels, stats, R, V, d,
                 mode, T, p.tpc, p.ntiles, gpart, wgt, gl_direct);
    hipError_t e = sc_launched("supcon.hip:supcon_bwd_kernel");
    if (e != hipSuccess || direct) return e;
    const int64_t total = R * d;
    int64_t wgs = (total + 255) / 256;
    if (wgs > 4096) wgs = 4096;
    launch_k(supcon_grad_reduce_kernel, dim3(unsigned(wgs)), dim3(256), 0, s,
             static_cast<const float*>(gpart), total, p.chunks, wgt, grad_loss, gZ);
    return sc_launched("supcon.hip:supcon_grad_reduce_kernel");
}

}  // namespace gll
