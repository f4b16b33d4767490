// extend_grad.hip -- backward of the out-of-sample extension (include/gll.h gll_extend_backward,
// DESIGN.md §3.13).  The neighbour lists (idx, d2) of gll_knn_query are frozen; with
//   t_i = 4 d2_i / (e_q e_j),  w_i = exp(-t_i),  S = sum_i w_i,  u = sum_i w_i P[j_i] / S
// and g = dL/du the gradients are
//   r_i = sum_c g_c (P[j_i, c] - u_c),  beta_i = w_i r_i / S,  a_i = w_i / S,
//   c_i = -4 beta_i / (e_q e_j)  (+ (sum_i beta_i t_i) / (2 d2_last) on the last entry for 'auto'),
//   gXq[q] = 2 sum_i c_i (x_q - x_j),  gXdb[j] = -2 sum_(q,i: j_i = j) c_i (x_q - x_j),
//   gP[j]  = sum_(q,i: j_i = j) a_i g[q],  grad_eps = sum_q sum_i 2 beta_i t_i / eps.
//
//  eg_row_kernel     one wave per query row: the weights, S and u exactly as extend_kernel forms
//                    them, r / beta / a / c with entry e on lane e % 64, c_i kept in LDS, then
//                    gXq[q] over chunks of 256 features (4 a lane), entries the inner loop.  Writes
//                    c and a (float64 Q x kn) and the row's grad_eps partial to the workspace when
//                    they are asked for, and zeroes the list counts for the launches behind it.
//  eg_count_kernel   entries per database row (integer atomics).
//  eg_scan_kernel    exclusive scan of the counts: one workgroup, tiles of 1,024 rows.
//  eg_fill_kernel    every entry's key (q << 8 | i) into a slot of its row's segment; the slot
//                    comes from an integer atomic, so the segment's order is arbitrary.
//  eg_db_kernel      one wave per database row: ranks its keys (distinct, so the ranks are a
//                    permutation: the list ordered by q), then gXdb[j] and gP[j] from the list in
//                    that order.  Up to `cap` keys are ranked and kept in LDS; a longer list is
//                    ranked in global memory and streamed through LDS `cap` ranks at a time.
//  eg_eps_kernel     the row partials of grad_eps summed in a fixed order: one workgroup.
//
// Every float64 product and sum is an explicit __dmul_rn / __dadd_rn in an order fixed by the
// lists alone: list order within a query row, ascending query within a database row.  No
// floating-point atomics, no inter-workgroup waiting.  IEEE as written: no clamps.
#include <limits.h>

#include <atomic>
#include <cmath>

#include "gll_internal.h"

namespace gll {

constexpr int kEgMaxList = 256;    // kn and C
constexpr int kEgCap = 512;        // keys of a database row ranked and held in LDS
constexpr int kEgCapSmall = 64;    // GLL_EGF_SMALL_LISTS
constexpr int kEgChunk = 4 * kWave;   // features a wave holds at a time
constexpr int kEgScanNT = 1024;
constexpr int kEgDbBits = GLL_EG_XDB | GLL_EG_P;

static std::atomic<int64_t> g_eg_launches{0};

static hipError_t eg_launched(const char* what) {
    g_eg_launches.fetch_add(1, std::memory_order_relaxed);
    return launch_status(what);
}

struct EgPlan {
    size_t cw, aw, ge, cnt, start, list, rank, total;
};

static EgPlan eg_plan(int64_t Q, int64_t N, int kn, int what) {
    EgPlan p;
    size_t off = 0;
    auto take = [&](size_t bytes) {
        const size_t at = off;
        off += (bytes + 255) & ~size_t(255);
        return at;
    };
    const bool db = (what & kEgDbBits) != 0;
    const size_t ent = size_t(Q) * size_t(kn);
    p.ge = take(size_t(Q) * 8);              // grad_eps row partials
    p.cw = take(db ? ent * 8 : 0);           // c_i
    p.aw = take(db ? ent * 8 : 0);           // a_i
    p.cnt = take(db ? size_t(N) * 4 : 0);    // entries per database row
    p.start = take(db ? size_t(N + 1) * 8 : 0);
    p.list = take(db ? ent * 8 : 0);         // keys, a segment per database row
    p.rank = take(db ? ent * 8 : 0);         // ranks of the keys of lists too long for LDS
    p.total = off;
    return p;
}

__device__ __forceinline__ void eg_wave_sync() {
    __builtin_amdgcn_wave_barrier();
    asm volatile("" ::: "memory");
}

// --------------------------------------------------------------------------------------
// Row kernel
// --------------------------------------------------------------------------------------
struct EgRow {
    double u[kEgMaxList];   // u_c; then beta_i t_i
    double g[kEgMaxList];   // g_c
    double c[kEgMaxList];   // c_i
    int j[kEgMaxList];      // database row of entry i (0 for an index out of range)
};

template <bool VEC>
__global__ __launch_bounds__(256) void eg_row_kernel(
    const float* __restrict__ Xq, const float* __restrict__ Xdb, const int32_t* __restrict__ idx,
    const float* __restrict__ d2, const float* __restrict__ P, const float* __restrict__ eps_db,
    float eps, const double* __restrict__ gU, int64_t Q, int64_t N, int kn, int d, int C, int what,
    float* __restrict__ gXq, double* __restrict__ cw, double* __restrict__ aw,
    double* __restrict__ ge, uint32_t* __restrict__ cnt, int32_t* __restrict__ status) {
    __shared__ EgRow sh[4];
    if (cnt) {   // the counts of eg_count_kernel, which runs behind this launch
        const int64_t nt = int64_t(gridDim.x) * 256;
        for (int64_t t = int64_t(blockIdx.x) * 256 + threadIdx.x; t < N; t += nt) cnt[t] = 0u;
    }
    const int lane = lane_id(), wv = threadIdx.x >> 6;
    const int64_t q = int64_t(blockIdx.x) * 4 + wv;
    if (q >= Q) return;   // whole wave
    EgRow& w = sh[wv];
    const int32_t* qi = idx + size_t(q) * kn;
    const float* qd = d2 + size_t(q) * kn;
    const bool fixed = eps > 0.f;
    const double eq = fixed ? double(eps) : double(sqrtf(qd[kn - 1]));

    // 1) weights, S and u: extend_kernel's operations in extend_kernel's order
    double wt[4], tt[4], den[4];
    int jj[4];
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    double sw = 0.0;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        const int b0 = kWave * s, e = b0 + lane;
        wt[s] = 0.0;
        tt[s] = 0.0;
        den[s] = 1.0;
        jj[s] = 0;
        if (b0 < kn) {   // wave-uniform
            if (e < kn) {
                int j = qi[e];
                const bool in = j >= 0 && int64_t(j) < N;
                j = in ? j : 0;
                const double ej = fixed ? double(eps) : double(eps_db[j]);
                den[s] = eq * ej;
                const double arg = -4.0 * double(qd[e]) / den[s];
                wt[s] = in ? exp(arg) : __builtin_nan("");
                tt[s] = -arg;
                jj[s] = j;
            }
            const int nn = kn - b0 < kWave ? kn - b0 : kWave;
            for (int u = 0; u < nn; ++u) {   // list order
                const double wu = __shfl(wt[s], u);
                const int ju = __shfl(jj[s], u);
                sw = __dadd_rn(sw, wu);
#pragma unroll
                for (int s2 = 0; s2 < 4; ++s2) {
                    const int c = lane + kWave * s2;
                    if (c < C)
                        acc[s2] = __dadd_rn(acc[s2], __dmul_rn(wu, double(P[size_t(ju) * C + c])));
                }
            }
        }
    }
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        const int c = lane + kWave * s;
        if (c < C) {
            w.u[c] = acc[s] / sw;
            w.g[c] = gU[size_t(q) * C + c];
        }
    }
    eg_wave_sync();

    // 2) entry e on lane e % 64: r over the classes in ascending order, then beta, a, c
    double rr[4];
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        const int e = lane + kWave * s;
        rr[s] = 0.0;
        if (e < kn) {
            const float* pj = P + size_t(jj[s]) * C;
            double r = 0.0;
            for (int c = 0; c < C; ++c)
                r = __dadd_rn(r, __dmul_rn(w.g[c], __dadd_rn(double(pj[c]), -w.u[c])));
            rr[s] = r;
        }
    }
    eg_wave_sync();   // u is read; its storage takes beta t from here
    double* bt = w.u;
    double av[4];
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        const int e = lane + kWave * s;
        av[s] = 0.0;
        if (e < kn) {
            const double beta = __dmul_rn(wt[s], rr[s]) / sw;
            av[s] = wt[s] / sw;
            w.c[e] = __dmul_rn(-4.0, beta) / den[s];
            bt[e] = __dmul_rn(beta, tt[s]);
            w.j[e] = jj[s];
        }
    }
    eg_wave_sync();
    double sbt = 0.0;   // sum_i beta_i t_i in list order, the same in every lane
    for (int i = 0; i < kn; ++i) sbt = __dadd_rn(sbt, bt[i]);
    if (!fixed) {   // e_q moves with the last distance of the list
        eg_wave_sync();
        if (lane == 0) w.c[kn - 1] = __dadd_rn(w.c[kn - 1], sbt / __dmul_rn(2.0, double(qd[kn - 1])));
        eg_wave_sync();
    }
    if (cw) {
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const int e = lane + kWave * s;
            if (e < kn) {
                cw[size_t(q) * kn + e] = w.c[e];
                aw[size_t(q) * kn + e] = av[s];
            }
        }
    }
    if (lane == 0) {
        if (ge) ge[q] = __dmul_rn(2.0, sbt) / double(eps);
        if (!(sw > 0.0)) atomicAdd(&status[2], 1);   // zero or NaN: the row's gradients are NaN
    }
    if (!(what & GLL_EG_XQ)) return;

    // 3) gXq[q] = 2 sum_i c_i (x_q - x_j): 4 features a lane, entries the inner loop
    const float* xq = Xq + size_t(q) * d;
    float* out = gXq + size_t(q) * d;
    for (int f0 = 0; f0 < d; f0 += kEgChunk) {
        const int k = f0 + 4 * lane;
        const f32x4 a = load4<VEC>(xq, k, d);
        double s4[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll 4
        for (int i = 0; i < kn; ++i) {
            const double ci = w.c[i];
            const f32x4 b = load4<VEC>(Xdb + size_t(w.j[i]) * d, k, d);
#pragma unroll
            for (int t = 0; t < 4; ++t)
                s4[t] = __dadd_rn(s4[t], __dmul_rn(ci, double(a[t]) - double(b[t])));
        }
#pragma unroll
        for (int t = 0; t < 4; ++t)
            if (k + t < d) out[k + t] = float(__dmul_rn(2.0, s4[t]));
    }
}

// --------------------------------------------------------------------------------------
// Transposed lists: count, scan, fill
// --------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void eg_count_kernel(const int32_t* __restrict__ idx,
                                                       int64_t total, int64_t N,
                                                       uint32_t* __restrict__ cnt) {
    const int64_t t = int64_t(blockIdx.x) * 256 + threadIdx.x;
    if (t >= total) return;
    const int j = idx[t];
    if (j >= 0 && int64_t(j) < N) atomicAdd(&cnt[j], 1u);
}

__global__ __launch_bounds__(kEgScanNT) void eg_scan_kernel(const uint32_t* __restrict__ cnt,
                                                            int64_t N, int64_t* __restrict__ start) {
    __shared__ uint32_t part[kEgScanNT / kWave];
    const int tid = threadIdx.x, lane = lane_id(), wv = tid >> 6;
    int64_t carry = 0;
    for (int64_t b0 = 0; b0 < N; b0 += kEgScanNT) {
        const int64_t t = b0 + tid;
        const uint32_t v = t < N ? cnt[t] : 0u;
        uint32_t inc = v;   // inclusive scan of the wave
#pragma unroll
        for (int off = 1; off < kWave; off <<= 1) {
            const uint32_t o = __shfl_up(inc, off);
            if (lane >= off) inc += o;
        }
        if (lane == kWave - 1) part[wv] = inc;
        __syncthreads();
        uint32_t before = 0u, all = 0u;
        for (int x = 0; x < kEgScanNT / kWave; ++x) {
            const uint32_t px = part[x];
            before += x < wv ? px : 0u;
            all += px;
        }
        if (t < N) start[t] = carry + int64_t(before + inc - v);
        carry += int64_t(all);
        __syncthreads();
    }
    if (tid == 0) start[N] = carry;
}

__global__ __launch_bounds__(256) void eg_fill_kernel(const int32_t* __restrict__ idx,
                                                      int64_t total, int64_t N, int kn,
                                                      uint32_t* __restrict__ cnt,
                                                      const int64_t* __restrict__ start,
                                                      int64_t* __restrict__ list) {
    const int64_t t = int64_t(blockIdx.x) * 256 + threadIdx.x;
    if (t >= total) return;
    const int j = idx[t];
    if (j < 0 || int64_t(j) >= N) return;
    const uint32_t left = atomicSub(&cnt[j], 1u);   // counts down from the row's length to 1
    const int64_t q = t / kn;
    list[start[j] + int64_t(left - 1u)] = (q << 8) | int64_t(t - q * kn);
}

// --------------------------------------------------------------------------------------
// Database kernel
// --------------------------------------------------------------------------------------
struct EgDb {
    int64_t kin[kEgCap];    // the segment as the fill left it
    int64_t kout[kEgCap];   // keys by rank
};

template <bool VEC>
__global__ __launch_bounds__(256) void eg_db_kernel(
    const float* __restrict__ Xq, const float* __restrict__ Xdb, const double* __restrict__ gU,
    const double* __restrict__ cw, const double* __restrict__ aw,
    const int64_t* __restrict__ start, const int64_t* __restrict__ list,
    int64_t* __restrict__ rank, int64_t N, int kn, int d, int C, int what, int cap,
    float* __restrict__ gXdb, float* __restrict__ gP, int32_t* __restrict__ status) {
    __shared__ EgDb sh[4];
    const int lane = lane_id(), wv = threadIdx.x >> 6;
    const int64_t j = int64_t(blockIdx.x) * 4 + wv;
    if (j >= N) return;   // whole wave
    EgDb& w = sh[wv];
    const int64_t s0 = start[j], L = start[j + 1] - s0;
    const int64_t* src = list + s0;
    int64_t* rk = rank + s0;
    const bool inlds = L <= cap;
    if (inlds) {
        for (int e = lane; e < int(L); e += kWave) w.kin[e] = src[e];
        eg_wave_sync();
        for (int e = lane; e < int(L); e += kWave) {
            const int64_t key = w.kin[e];
            int r = 0;
            for (int u = 0; u < int(L); ++u) r += w.kin[u] < key ? 1 : 0;
            w.kout[r] = key;
        }
        eg_wave_sync();
    } else {
        if (lane == 0) atomicAdd(&status[3], 1);
        for (int64_t e = lane; e < L; e += kWave) {   // each lane reads back only its own ranks
            const int64_t key = src[e];
            int64_t r = 0;
            for (int64_t u = 0; u < L; ++u) r += src[u] < key ? 1 : 0;
            rk[e] = r;
        }
    }
    // body(key) for every entry of the list in ascending key order
    auto for_entries = [&](auto&& body) {
        if (inlds) {
            for (int u = 0; u < int(L); ++u) body(w.kout[u]);
            return;
        }
        for (int64_t t0 = 0; t0 < L; t0 += cap) {
            eg_wave_sync();   // the last chunk is consumed
            for (int64_t e = lane; e < L; e += kWave) {
                const int64_t r = rk[e];
                if (r >= t0 && r < t0 + cap) w.kout[r - t0] = src[e];
            }
            eg_wave_sync();
            const int n = L - t0 < cap ? int(L - t0) : cap;
            for (int u = 0; u < n; ++u) body(w.kout[u]);
        }
    };

    if (what & GLL_EG_XDB) {   // gXdb[j] = 2 sum c (x_j - x_q): the differences negated exactly
        const float* xj = Xdb + size_t(j) * d;
        float* out = gXdb + size_t(j) * d;
        for (int f0 = 0; f0 < d; f0 += kEgChunk) {
            const int k = f0 + 4 * lane;
            const f32x4 b = load4<VEC>(xj, k, d);
            double s4[4] = {0.0, 0.0, 0.0, 0.0};
            for_entries([&](int64_t key) {
                const int64_t q = key >> 8;
                const double ci = cw[size_t(q) * kn + size_t(key & 255)];
                const f32x4 a = load4<VEC>(Xq + size_t(q) * d, k, d);
#pragma unroll
                for (int t = 0; t < 4; ++t)
                    s4[t] = __dadd_rn(s4[t], __dmul_rn(ci, double(b[t]) - double(a[t])));
            });
#pragma unroll
            for (int t = 0; t < 4; ++t)
                if (k + t < d) out[k + t] = float(__dmul_rn(2.0, s4[t]));
        }
    }
    if (what & GLL_EG_P) {   // gP[j, c] = sum a g[q, c], class c on lane c % 64
        double s4[4] = {0.0, 0.0, 0.0, 0.0};
        for_entries([&](int64_t key) {
            const int64_t q = key >> 8;
            const double ai = aw[size_t(q) * kn + size_t(key & 255)];
            const double* gq = gU + size_t(q) * C;
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                const int c = lane + kWave * s;
                if (c < C) s4[s] = __dadd_rn(s4[s], __dmul_rn(ai, gq[c]));
            }
        });
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const int c = lane + kWave * s;
            if (c < C) gP[size_t(j) * C + c] = float(s4[s]);
        }
    }
}

// grad_eps = sum_q ge[q]: thread t sums rows t, t + 256, .. in ascending order, then a tree
__global__ __launch_bounds__(256) void eg_eps_kernel(const double* __restrict__ ge, int64_t Q,
                                                     double* __restrict__ out) {
    __shared__ double part[256];
    double s = 0.0;
    for (int64_t q = threadIdx.x; q < Q; q += 256) s = __dadd_rn(s, ge[q]);
    part[threadIdx.x] = s;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if (int(threadIdx.x) < off)
            part[threadIdx.x] = __dadd_rn(part[threadIdx.x], part[threadIdx.x + off]);
        __syncthreads();
    }
    if (threadIdx.x == 0) out[0] = part[0];
}

static int check_eg(int64_t Q, int64_t N, int32_t kn, int32_t d, int32_t C, int what, int flags) {
    if (Q < 1 || N < 1 || kn < 1 || d < 1 || C < 1) return GLL_ERR_INVALID_ARG;
    if (what < 1 || (what & ~(GLL_EG_XQ | GLL_EG_XDB | GLL_EG_P | GLL_EG_EPS)))
        return GLL_ERR_INVALID_ARG;
    if (flags & ~GLL_EGF_SMALL_LISTS) return GLL_ERR_INVALID_ARG;
    if (kn > kEgMaxList || C > kEgMaxList || d > 4096 || N > INT32_MAX / 2)
        return GLL_ERR_UNSUPPORTED;
    if (Q > INT32_MAX / 2) return GLL_ERR_UNSUPPORTED;   // one thread per list entry in a 1-D grid
    return GLL_OK;
}

static bool eg_aligned16(const void* p) { return reinterpret_cast<uintptr_t>(p) % 16 == 0; }

static hipError_t launch_extend_grad(int64_t Q, int64_t N, int kn, int d, int C, const float* Xq,
                                     const float* Xdb, const int32_t* idx, const float* d2,
                                     const float* P, const float* eps_db, float eps,
                                     const double* gU, int what, int flags, float* gXq,
                                     float* gXdb, float* gP, double* grad_eps, int32_t* status,
                                     void* ws, hipStream_t s) {
    const EgPlan p = eg_plan(Q, N, kn, what);
    char* base = static_cast<char*>(ws);
    const bool db = (what & kEgDbBits) != 0;
    double* ge = (what & GLL_EG_EPS) ? reinterpret_cast<double*>(base + p.ge) : nullptr;
    double* cw = db ? reinterpret_cast<double*>(base + p.cw) : nullptr;
    double* aw = db ? reinterpret_cast<double*>(base + p.aw) : nullptr;
    uint32_t* cnt = db ? reinterpret_cast<uint32_t*>(base + p.cnt) : nullptr;
    int64_t* start = reinterpret_cast<int64_t*>(base + p.start);
    int64_t* list = reinterpret_cast<int64_t*>(base + p.list);
    int64_t* rank = reinterpret_cast<int64_t*>(base + p.rank);
    const bool vec = d % 4 == 0 && eg_aligned16(Xq) && eg_aligned16(Xdb);
    const dim3 rgrid(unsigned((Q + 3) / 4));
    if (vec)
        launch_k(eg_row_kernel<true>, rgrid, dim3(256), 0, s, Xq, Xdb, idx, d2, P, eps_db, eps, gU,
                 Q, N, kn, d, C, what, gXq, cw, aw, ge, cnt, status);
    else
        launch_k(eg_row_kernel<false>, rgrid, dim3(256), 0, s, Xq, Xdb, idx, d2, P, eps_db, eps,
                 gU, Q, N, kn, d, C, what, gXq, cw, aw, ge, cnt, status);
    hipError_t e = eg_launched("extend_grad.hip:eg_row_kernel");
    if (e != hipSuccess) return e;
    if (db) {
        const int64_t total = Q * int64_t(kn);
        const dim3 egrid(unsigned((total + 255) / 256));
        launch_k(eg_count_kernel, egrid, dim3(256), 0, s, idx, total, N, cnt);
        if ((e = eg_launched("extend_grad.hip:eg_count_kernel")) != hipSuccess) return e;
        launch_k(eg_scan_kernel, dim3(1), dim3(kEgScanNT), 0, s, static_cast<const uint32_t*>(cnt),
                 N, start);
        if ((e = eg_launched("extend_grad.hip:eg_scan_kernel")) != hipSuccess) return e;
        launch_k(eg_fill_kernel, egrid, dim3(256), 0, s, idx, total, N, kn, cnt,
                 static_cast<const int64_t*>(start), list);
        if ((e = eg_launched("extend_grad.hip:eg_fill_kernel")) != hipSuccess) return e;
        const int cap = (flags & GLL_EGF_SMALL_LISTS) ? kEgCapSmall : kEgCap;
        const dim3 dgrid(unsigned((N + 3) / 4));
        const int dwhat = what & kEgDbBits;
        if (vec)
            launch_k(eg_db_kernel<true>, dgrid, dim3(256), 0, s, Xq, Xdb, gU,
                     static_cast<const double*>(cw), static_cast<const double*>(aw),
                     static_cast<const int64_t*>(start), static_cast<const int64_t*>(list), rank, N,
                     kn, d, C, dwhat, cap, gXdb, gP, status);
        else
            launch_k(eg_db_kernel<false>, dgrid, dim3(256), 0, s, Xq, Xdb, gU,
                     static_cast<const double*>(cw), static_cast<const double*>(aw),
                     static_cast<const int64_t*>(start), static_cast<const int64_t*>(list), rank, N,
                     kn, d, C, dwhat, cap, gXdb, gP, status);
        if ((e = eg_launched("extend_grad.hip:eg_db_kernel")) != hipSuccess) return e;
    }
    if (what & GLL_EG_EPS) {
        launch_k(eg_eps_kernel, dim3(1), dim3(256), 0, s, static_cast<const double*>(ge), Q,
                 grad_eps);
        if ((e = eg_launched("extend_grad.hip:eg_eps_kernel")) != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace gll

using namespace gll;

extern "C" {

size_t gll_extend_grad_workspace_bytes(int64_t Q, int64_t N, int32_t kn, int32_t d, int32_t C,
                                       int what, int flags) {
    if (check_eg(Q, N, kn, d, C, what, flags) != GLL_OK) return 0;
    return eg_plan(Q, N, kn, what).total;
}

int gll_extend_backward(int64_t Q, int64_t N, int32_t kn, int32_t d, int32_t C, const float* Xq,
                        const float* Xdb, const int32_t* idx, const float* d2, const float* P,
                        const float* eps_db, float eps, const double* gU, int what, int flags,
                        float* gXq, float* gXdb, float* gP, double* grad_eps, int32_t* status,
                        void* workspace, void* stream) {
    const int rc = check_eg(Q, N, kn, d, C, what, flags);
    if (rc != GLL_OK) return rc;
    if (!Xq || !Xdb || !idx || !d2 || !P || !gU || !status || !workspace)
        return GLL_ERR_INVALID_ARG;
    if (!(eps > 0.f) && (!eps_db || (what & GLL_EG_EPS))) return GLL_ERR_INVALID_ARG;
    if (((what & GLL_EG_XQ) && !gXq) || ((what & GLL_EG_XDB) && !gXdb) ||
        ((what & GLL_EG_P) && !gP) || ((what & GLL_EG_EPS) && !grad_eps))
        return GLL_ERR_INVALID_ARG;
    const void* four[] = {Xq, Xdb, idx, d2, P, eps_db, gXq, gXdb, gP, status};
    for (const void* p : four)
        if (reinterpret_cast<uintptr_t>(p) % 4) return GLL_ERR_INVALID_ARG;
    if (reinterpret_cast<uintptr_t>(gU) % 8 || reinterpret_cast<uintptr_t>(grad_eps) % 8 ||
        reinterpret_cast<uintptr_t>(workspace) % 16)
        return GLL_ERR_INVALID_ARG;
    const hipError_t e = launch_extend_grad(
        Q, N, kn, d, C, Xq, Xdb, idx, d2, P, eps_db, eps > 0.f ? eps : 0.f, gU, what, flags, gXq,
        gXdb, gP, grad_eps, status, workspace, static_cast<hipStream_t>(stream));
    return e == hipSuccess ? GLL_OK : GLL_ERR_HIP;
}

int64_t gll_extend_grad_launches(void) { return g_eg_launches.load(std::memory_order_relaxed); }

}  // extern "C"
