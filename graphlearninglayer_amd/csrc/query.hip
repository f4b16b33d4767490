// query.hip -- exact query-vs-database kNN and the out-of-sample (Nadaraya-Watson) extension
// of a solved graph (include/gll.h gll_knn_query / gll_extend).
//
//  query_norm_kernel    |a|^2 of the centred rows a = x - c, c = row 0 of Xdb; one wave per row.
//  query_gram_kernel    a panel of nominating distances D2[q, j] = |a_q|^2 + |a_j|^2 - 2 a_q.a_j,
//                       one 32 x 32 tile per wave as one chain of v_mfma_f32_32x32x2_f32 over the
//                       features (fp32 inputs: no split, no dropped terms).  Error bound kQErr(d)
//                       below, counted from this code; tests/query_ref.py repeats the count.
//  query_select_kernel  one wave per query row:
//                       1. threshold scan of the D2 row: every lane keeps its kQTop smallest D2
//                          bits, T = the kc-th smallest of the 64 kQTop entries (kc = k + 8), and
//                          every column with D2 bits <= T is compacted into the wave's LDS list
//                          (kQCap slots);
//                       2. exact difference-form d^2 = sum_f (q_f - x_f)^2 of every candidate,
//                          8 lanes a candidate, in fp32 (the value returned) and in float64 (the
//                          value ranked) from the same loads;
//                       3. the k nearest by (float64 d^2, index);
//                       4. a certificate that no column left out can belong to them given
//                          kQErr; when it fails, or the list overflowed (more than kQCap columns
//                          at or under T: ties), an exact rescan of the row -- every column under
//                          the bound streamed through the same rank-and-keep in chunks -- counted
//                          in status[0];
//                       5. the k kept ordered by (returned fp32 d^2, index).
//  extend_kernel        one wave per query row: weights exp(-4 d^2 / (eps_q eps_j)) in float64
//                       from the returned fp32 d^2, sum_j w_j P_j and sum_j w_j in list order,
//                       the quotient and the argmax label.
//
// Ordinary launches: no inter-workgroup waiting, no grid barrier, no spin loop; the only atomics
// are atomicAdd on the status words.  Every sum runs in an order fixed by (d, k) alone and every
// row's result is a function of that row, the database and k: bitwise reproducible, and
// independent of the rows that share the call or the panel.
#include <limits.h>

#include <atomic>
#include <cmath>

#include "gll_internal.h"
#include "query_common.h"

namespace gll {

constexpr int kQTile = 32;             // MFMA tile
constexpr int kQBlk = 64;              // rows and columns of a workgroup's 2 x 2 tiles
constexpr int kQKc = 64;               // features staged per round
constexpr int kQLd = kQKc + 4;         // LDS row stride (floats): 16-B aligned rows, banks staggered
constexpr int kQTop = 5;               // per-lane list of the threshold scan: 64 x 5 >= 256 + 8
constexpr int kQMargin = 8;            // candidates asked for beyond k
constexpr int kQChunk = kQCap - 256 - kWave;   // rescan: flush once more than this many are new
constexpr size_t kQPanelBytes = size_t(128) << 20;   // cap of the D2 panel
constexpr int64_t kQMaxPanelRows = int64_t(1) << 20;

// |D2[q, j] - d(q, j)^2| <= kQErr(d) (|a_q| + |a_j|)^2 with u = 2^-24:
//   centring   a^ = fl(x - c), |a^ - a| <= u |a| per element: the distance between the rounded
//              rows differs from d by <= u (|a_q| + |a_j|), its square by <= 2 u (1 + u) (..)^2;
//   norms      d fmaf roundings and a 6-level tree over the lanes: <= (d + 6) u |a^|^2 each;
//   dot        d products accumulated two a step, <= d roundings: <= d u |a^_q| |a^_j|, twice;
//   assembly   fl(nq + nj), then one fmaf: 2 u (|a^_q| + |a^_j|)^2;
// together <= (d + 10) u (1 + 2^-10) (|a_q| + |a_j|)^2 <= (d + 16) u (..)^2 for d <= 4096.
__host__ __device__ inline double q_gram_err(int d) { return double(d + 16) * 0x1p-24; }

static std::atomic<int64_t> g_q_launches{0};

hipError_t q_launched(const char* what) {
    g_q_launches.fetch_add(1, std::memory_order_relaxed);
    return launch_status(what);
}

struct QPlan {
    int ld;          // leading dimension of the panel: N rounded up to 4
    int64_t rows;    // panel height: min(Q, cap)
    size_t ndb, nq, D2, total;
};

static QPlan query_plan(int64_t Q, int64_t N, int flags) {
    QPlan p;
    p.ld = int((N + 3) & ~int64_t(3));
    int64_t pr = int64_t(kQPanelBytes / (size_t(p.ld) * 4)) / kQBlk * kQBlk;
    if (pr > kQMaxPanelRows) pr = kQMaxPanelRows;
    if (pr < kQBlk || (flags & GLL_QF_SMALL_PANELS)) pr = kQBlk;
    p.rows = Q < pr ? Q : pr;
    size_t off = 0;
    auto take = [&](size_t bytes) {
        const size_t at = off;
        off += (bytes + 255) & ~size_t(255);
        return at;
    };
    p.ndb = take(size_t(N) * 4);
    p.nq = take(size_t(p.rows) * 4);
    p.D2 = take(size_t(p.rows) * size_t(p.ld) * 4);
    p.total = off;
    return p;
}

// --------------------------------------------------------------------------------------
// |x - c|^2 of rows 0 .. ndb - 1 of Xdb (ndb = 0: the database norms stand from the first panel)
// and of `rows` query rows; feature f on lane f % 64, fmaf chain, then the xor butterfly.
// --------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void query_norm_kernel(
    const float* __restrict__ Xdb, int64_t ndb, const float* __restrict__ Xq, int64_t rows, int d,
    float* __restrict__ out_db, float* __restrict__ out_q) {
    const int lane = lane_id();
    const int64_t g = int64_t(blockIdx.x) * 4 + (threadIdx.x >> 6);
    if (g >= ndb + rows) return;   // whole wave
    const float* src = g < ndb ? Xdb + size_t(g) * d : Xq + size_t(g - ndb) * d;
    float s = 0.f;
    for (int f = lane; f < d; f += kWave) {
        const float a = src[f] - Xdb[f];
        s = __builtin_fmaf(a, a, s);
    }
    s = wave_sum(s);
    if (lane == 0) {
        if (g < ndb) out_db[g] = s;
        else out_q[g - ndb] = s;
    }
}

// rows row0 .. row0 + 63 of X (zero past nrows and past d), features k0 .. k0 + kQKc - 1, minus
// the centre c, into dst[64][kQLd]
template <bool VEC>
__device__ inline void q_stage(float* dst, const float* __restrict__ X, const float* __restrict__ c,
                               int64_t nrows, int d, int64_t row0, int k0) {
    if constexpr (VEC) {
        for (int e = threadIdx.x; e < kQBlk * (kQKc / 4); e += 256) {
            const int rr = e / (kQKc / 4), k = (e % (kQKc / 4)) * 4;
            const int64_t row = row0 + rr;
            f32x4 v{0.f, 0.f, 0.f, 0.f};
            if (row < nrows && k0 + k < d)   // d % 4 == 0: a group is inside the row or past it
                v = *reinterpret_cast<const f32x4*>(X + size_t(row) * d + k0 + k) -
                    *reinterpret_cast<const f32x4*>(c + k0 + k);
            *reinterpret_cast<f32x4*>(dst + rr * kQLd + k) = v;
        }
    } else {
        for (int e = threadIdx.x; e < kQBlk * kQKc; e += 256) {
            const int rr = e / kQKc, k = e % kQKc;
            const int64_t row = row0 + rr;
            dst[rr * kQLd + k] =
                (row < nrows && k0 + k < d) ? X[size_t(row) * d + k0 + k] - c[k0 + k] : 0.f;
        }
    }
}

// Panel rows r (queries q0 + r of the call; Xq points at the panel's first row) against every
// database row.  Workgroup (bx, by) of a 1-D grid: columns 64 bx .., rows 64 by ..; wave w the
// tile (w >> 1, w & 1).  MFMA A = query tile (accumulator register index = query row), B =
// database tile (lane = column): a store instruction writes 32 consecutive columns of two rows.
template <bool VEC>
__global__ __launch_bounds__(256) void query_gram_kernel(
    const float* __restrict__ Xq, const float* __restrict__ Xdb, int64_t rows, int64_t N, int d,
    int ld, int tiles_n, const float* __restrict__ nq, const float* __restrict__ ndb,
    float* __restrict__ D2) {
    __shared__ __attribute__((aligned(16))) float sa[kQBlk * kQLd];
    __shared__ __attribute__((aligned(16))) float sb[kQBlk * kQLd];
    const int bx = blockIdx.x % tiles_n, by = blockIdx.x / tiles_n;
    const int w = threadIdx.x >> 6, l = lane_id(), i = l & 31, h = l >> 5;
    const int64_t r0 = int64_t(by) * kQBlk, j0 = int64_t(bx) * kQBlk;
    f32x16 acc;
#pragma unroll
    for (int t = 0; t < 16; ++t) acc[t] = 0.f;
    const float* pa = sa + ((w >> 1) * kQTile + i) * kQLd + 4 * h;
    const float* pb = sb + ((w & 1) * kQTile + i) * kQLd + 4 * h;
    for (int k0 = 0; k0 < d; k0 += kQKc) {
        __syncthreads();   // everyone is done with the last round's tiles
        q_stage<VEC>(sa, Xq, Xdb, rows, d, r0, k0);
        q_stage<VEC>(sb, Xdb, Xdb, N, d, j0, k0);
        __syncthreads();
        const int rem = d - k0 < kQKc ? d - k0 : kQKc;
        const int k8 = (rem + 7) & ~7;   // zeros past d add exact zeros
        for (int q = 0; q < k8; q += 8) {
            const f32x4 a = *reinterpret_cast<const f32x4*>(pa + q);
            const f32x4 b = *reinterpret_cast<const f32x4*>(pb + q);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, b.x, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, b.y, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, b.z, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, b.w, acc, 0, 0, 0);
        }
    }
    const int64_t j = j0 + (w & 1) * kQTile + i;
    if (j >= N) return;
    const float nj = ndb[j];
#pragma unroll
    for (int t = 0; t < 16; ++t) {
        const int64_t r = r0 + (w >> 1) * kQTile + (t & 3) + 8 * (t >> 2) + 4 * h;
        if (r < rows) D2[size_t(r) * ld + j] = __builtin_fmaf(-2.f, acc[t], nq[r] + nj);
    }
}

// --------------------------------------------------------------------------------------
// Selection
// --------------------------------------------------------------------------------------
// QLists, q_exact (step 2) and q_rank_keep (step 3): query_common.h, shared with rerank.hip

// D2 bits as an ordered key: negative values (rounding) count as 0, NaN as +inf.
__device__ __forceinline__ uint32_t q_key(float x) {
    return x == x ? __float_as_uint(x > 0.f ? x : 0.f) : 0x7F800000u;
}

template <bool VEC>
__global__ __launch_bounds__(256) void query_select_kernel(
    const float* __restrict__ D2, int ld, const float* __restrict__ Xq,
    const float* __restrict__ Xdb, int64_t rows, int N, int d, int k, double gerr,
    int32_t* __restrict__ idx, float* __restrict__ d2o, int32_t* __restrict__ status) {
    __shared__ QLists sh[4];
    const int lane = lane_id(), wv = threadIdx.x >> 6;
    const int64_t r = int64_t(blockIdx.x) * 4 + wv;
    if (r >= rows) return;   // whole wave
    QLists& w = sh[wv];
    const float* row = D2 + size_t(r) * ld;   // 16-B aligned: ld % 4 == 0, the panel 256-B aligned
    const float* xq = Xq + size_t(r) * d;
    const int kc = k + kQMargin;

    // 1) per-lane kQTop smallest keys of the row
    uint32_t m[kQTop];
#pragma unroll
    for (int t = 0; t < kQTop; ++t) m[t] = 0xFFFFFFFFu;
    bool bad = false;   // a non-finite D2 in the row
    for (int jb = 0; jb < N; jb += 4 * kWave) {
        const int jl = jb + 4 * lane;
        f32x4 v{0.f, 0.f, 0.f, 0.f};
        if (jl < N) v = *reinterpret_cast<const f32x4*>(row + jl);   // jl + 3 < ld
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const bool in = jl + t < N;
            bad |= in && !(fabsf(v[t]) < __builtin_inff());
            uint32_t u = in ? q_key(v[t]) : 0xFFFFFFFFu;
#pragma unroll
            for (int s = 0; s < kQTop; ++s) {
                const uint32_t lo = m[s] < u ? m[s] : u;
                u = m[s] < u ? u : m[s];
                m[s] = lo;
            }
        }
    }
    auto count_le = [&](uint32_t t) {
        int c = 0;
#pragma unroll
        for (int s = 0; s < kQTop; ++s) c += __popcll(__ballot(m[s] <= t));
        return c;
    };
    // T: at least min(kc, N) columns have keys <= T.  Fewer than kc list entries (only for
    // N < kQCap: some lane saw fewer than kQTop columns): every column
    uint32_t T = 0xFFFFFFFEu;
    if (count_le(T) >= kc) {
        uint32_t lo = 0u, up = 0x7F800000u;   // keys are at most +inf
        while (lo < up) {   // the smallest T with count_le(T) >= kc (wave-uniform, <= 31 steps)
            const uint32_t mid = lo + ((up - lo) >> 1);
            if (count_le(mid) >= kc) up = mid;
            else lo = mid + 1u;
        }
        T = up;
    }
    // compact every column with key <= T
    int total = 0;
    for (int jb = 0; jb < N; jb += 4 * kWave) {
        const int jl = jb + 4 * lane;
        f32x4 v{0.f, 0.f, 0.f, 0.f};
        if (jl < N) v = *reinterpret_cast<const f32x4*>(row + jl);
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const bool p = jl + t < N && q_key(v[t]) <= T;
            const uint64_t mk = __ballot(p);
            const int pos = total + lanes_below(mk);
            if (p && pos < kQCap) w.cj[pos] = jl + t;
            total += __popcll(mk);
        }
    }
    __builtin_amdgcn_wave_barrier();
    asm volatile("" ::: "memory");
    bad = __ballot(bad) != 0ull;
    const bool overflow = total > kQCap;
    bool rescan = overflow;
    double thr = __builtin_inf();
    if (!overflow) {
        // 2-3) exact distances, the k nearest by (float64 d^2, index)
        q_exact<VEC>(Xdb, xq, d, w, 0, total);
        q_rank_keep(w, total, k);   // total >= min(kc, N) >= k
        // 4) certificate.  A left-out column j has max(D2, 0) >= tb = the float of bits T + 1.
        //    If it belonged to the k nearest, d_qj^2 <= dK (the k-th distance found), so
        //    |a_j| <= |a_q| + sqrt(dK) and D2 <= dK + gerr (2 |a_q| + sqrt(dK))^2 = thr:
        //    tb > thr rules that out.  A row with non-finite distances is not certified (its
        //    values are unspecified; the indices are in range either way).
        const double dK = w.cd[k - 1];
        if (total < N && !bad && dK < __builtin_inf()) {
            double a2 = 0.0;
            for (int f = lane; f < d; f += kWave) {
                const double a = double(xq[f]) - double(Xdb[f]);
                a2 = __builtin_fma(a, a, a2);
            }
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) a2 += __shfl_xor(a2, off);
            const double ai = sqrt(a2) * (1.0 + 0x1p-40);
            const double rr = 2.0 * ai + sqrt(dK);
            thr = dK + gerr * rr * rr + 0x1p-100;   // + the fp32 MFMA's flushed subnormals
            const double tb = double(__uint_as_float(T + 1u));
            rescan = !(tb > thr);
        }
    }
    if (rescan) {
        // exact rescan: every column whose D2 is not above thr (all of them after an overflow),
        // in chunks behind the k best so far
        if (lane == 0) atomicAdd(&status[0], 1);
        int nb = 0, cnt = 0;
        for (int jb = 0; jb < N; jb += kWave) {
            const int j = jb + lane;
            const float v = j < N ? row[j] : 0.f;
            const bool take = j < N && !(double(v) > thr);
            const uint64_t mk = __ballot(take);
            if (take) w.cj[nb + cnt + lanes_below(mk)] = j;   // nb + cnt <= kQCap - 64 here
            cnt += __popcll(mk);
            if (cnt > kQChunk || jb + kWave >= N) {
                __builtin_amdgcn_wave_barrier();
                asm volatile("" ::: "memory");
                q_exact<VEC>(Xdb, xq, d, w, nb, nb + cnt);
                nb = q_rank_keep(w, nb + cnt, k);
                cnt = 0;
            }
        }
        // nb == k: the k nearest all lie under thr
        for (int e = nb + lane; e < k; e += kWave) {   // (unreachable for finite input)
            w.cj[e] = 0;
            w.cd[e] = __builtin_inf();
            w.cf[e] = __builtin_inff();
        }
        __builtin_amdgcn_wave_barrier();
        asm volatile("" ::: "memory");
    }
    // 5) the k kept, by (returned fp32 d^2, index); NaN ranks as +inf
    int32_t* oi = idx + size_t(r) * k;
    float* od = d2o + size_t(r) * k;
    for (int e = lane; e < k; e += kWave) {
        const float fe = w.cf[e];
        const float ke = fe == fe ? fe : __builtin_inff();
        const int je = w.cj[e];
        bad |= !(fabsf(fe) < __builtin_inff());
        int rk = 0;
        for (int u = 0; u < k; ++u) {
            const float fu = w.cf[u];
            const float ku = fu == fu ? fu : __builtin_inff();
            rk += (ku < ke || (ku == ke && w.cj[u] < je)) ? 1 : 0;
        }
        oi[rk] = je;
        od[rk] = fe;
    }
    if (__ballot(bad) != 0ull && lane == 0) atomicAdd(&status[1], 1);
}

// --------------------------------------------------------------------------------------
// Extension
// --------------------------------------------------------------------------------------
// (value, index) a ranks before b: numbers by value descending, NaN after every number, each by
// index ascending (the margin head's rule)
__device__ __forceinline__ bool q_better(double av, int ai, double bv, int bi) {
    const bool an = av != av, bn = bv != bv;
    if (an != bn) return bn;
    if (!an && av != bv) return av > bv;
    return ai < bi;
}

__global__ __launch_bounds__(256) void extend_kernel(
    const int32_t* __restrict__ idx, const float* __restrict__ d2, int64_t Q, int64_t N, int kn,
    int C, const float* __restrict__ P, const float* __restrict__ eps_db, float eps,
    double* __restrict__ Uq, int64_t* __restrict__ label, int32_t* __restrict__ status) {
    const int lane = lane_id();
    const int64_t q = int64_t(blockIdx.x) * 4 + (threadIdx.x >> 6);
    if (q >= Q) return;   // whole wave
    const int32_t* qi = idx + size_t(q) * kn;
    const float* qd = d2 + size_t(q) * kn;
    const bool fixed = eps > 0.f;
    // eps_q of 'auto': the distance to the last neighbour of the list, in fp32 as the graph
    // build stores its eps_i
    const double eq = fixed ? double(eps) : double(sqrtf(qd[kn - 1]));
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    double sw = 0.0;
    for (int b0 = 0; b0 < kn; b0 += kWave) {
        const int e = b0 + lane;
        int j = 0;
        double wt = 0.0;
        if (e < kn) {
            j = qi[e];
            const bool in = j >= 0 && int64_t(j) < N;
            j = in ? j : 0;
            const double ej = fixed ? double(eps) : double(eps_db[j]);
            wt = in ? exp(-4.0 * double(qd[e]) / (eq * ej)) : __builtin_nan("");
        }
        const int nn = kn - b0 < kWave ? kn - b0 : kWave;
        for (int u = 0; u < nn; ++u) {   // list order
            const double wu = __shfl(wt, u);
            const int ju = __shfl(j, u);
            sw = __dadd_rn(sw, wu);
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                const int c = lane + kWave * s;
                if (c < C) acc[s] = __dadd_rn(acc[s], __dmul_rn(wu, double(P[size_t(ju) * C + c])));
            }
        }
    }
    double bv = __builtin_nan("");
    int bi = INT_MAX;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        const int c = lane + kWave * s;
        if (c < C) {
            const double u = acc[s] / sw;
            Uq[size_t(q) * C + c] = u;
            if (q_better(u, c, bv, bi)) {
                bv = u;
                bi = c;
            }
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const double ov = __shfl_xor(bv, off);
        const int oi = __shfl_xor(bi, off);
        if (q_better(ov, oi, bv, bi)) {
            bv = ov;
            bi = oi;
        }
    }
    if (lane == 0) {
        label[q] = bi;
        if (!(sw > 0.0)) atomicAdd(&status[2], 1);   // zero or NaN: the row is NaN
    }
}

static hipError_t launch_knn_query(int64_t Q, int64_t N, int d, int k, int flags, const float* Xq,
                                   const float* Xdb, int32_t* idx, float* d2, int32_t* status,
                                   void* ws, hipStream_t s) {
    const QPlan p = query_plan(Q, N, flags);
    char* base = static_cast<char*>(ws);
    float* ndb = reinterpret_cast<float*>(base + p.ndb);
    float* nq = reinterpret_cast<float*>(base + p.nq);
    float* D2 = reinterpret_cast<float*>(base + p.D2);
    const bool vec = q_vec(Xq, Xdb, d);
    const int tiles_n = int((N + kQBlk - 1) / kQBlk);
    for (int64_t q0 = 0; q0 < Q; q0 += p.rows) {
        const int64_t rows = Q - q0 < p.rows ? Q - q0 : p.rows;
        const float* xq = Xq + size_t(q0) * d;
        const int64_t ndb_rows = q0 == 0 ? N : 0;
        launch_k(query_norm_kernel, dim3(unsigned((ndb_rows + rows + 3) / 4)), dim3(256), 0, s, Xdb,
                 ndb_rows, xq, rows, d, ndb, nq);
        hipError_t e = q_launched("query.hip:query_norm_kernel");
        if (e != hipSuccess) return e;
        const dim3 grid(unsigned(int64_t(tiles_n) * ((rows + kQBlk - 1) / kQBlk)));
        if (vec)
            launch_k(query_gram_kernel<true>, grid, dim3(256), 0, s, xq, Xdb, rows, N, d, p.ld,
                     tiles_n, static_cast<const float*>(nq), static_cast<const float*>(ndb), D2);
        else
            launch_k(query_gram_kernel<false>, grid, dim3(256), 0, s, xq, Xdb, rows, N, d, p.ld,
                     tiles_n, static_cast<const float*>(nq), static_cast<const float*>(ndb), D2);
        e = q_launched("query.hip:query_gram_kernel");
        if (e != hipSuccess) return e;
        const dim3 sgrid(unsigned((rows + 3) / 4));
        int32_t* oi = idx + size_t(q0) * k;
        float* od = d2 + size_t(q0) * k;
        if (vec)
            launch_k(query_select_kernel<true>, sgrid, dim3(256), 0, s, static_cast<const float*>(D2),
                     p.ld, xq, Xdb, rows, int(N), d, k, q_gram_err(d), oi, od, status);
        else
            launch_k(query_select_kernel<false>, sgrid, dim3(256), 0, s, static_cast<const float*>(D2),
                     p.ld, xq, Xdb, rows, int(N), d, k, q_gram_err(d), oi, od, status);
        e = q_launched("query.hip:query_select_kernel");
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

static int check_query(int64_t Q, int64_t N, int32_t d, int32_t k, int flags) {
    if (Q < 1 || N < 1 || d < 1 || k < 1 || k > N) return GLL_ERR_INVALID_ARG;
    if (flags & ~GLL_QF_SMALL_PANELS) return GLL_ERR_INVALID_ARG;
    if (k > 256 || d > 4096 || N > INT32_MAX / 2) return GLL_ERR_UNSUPPORTED;
    return GLL_OK;
}

}  // namespace gll

using namespace gll;

extern "C" {

size_t gll_query_workspace_bytes(int64_t Q, int64_t N, int32_t d, int32_t k, int flags) {
    if (check_query(Q, N, d, k, flags) != GLL_OK) return 0;
    return query_plan(Q, N, flags).total;
}

int gll_knn_query(int64_t Q, int64_t N, int32_t d, int32_t k, int flags, const float* Xq,
                  const float* Xdb, int32_t* idx, float* d2, int32_t* status, void* workspace,
                  void* stream) {
    const int rc = check_query(Q, N, d, k, flags);
    if (rc != GLL_OK) return rc;
    if (!Xq || !Xdb || !idx || !d2 || !status || !workspace) return GLL_ERR_INVALID_ARG;
    if (reinterpret_cast<uintptr_t>(Xq) % 4 || reinterpret_cast<uintptr_t>(Xdb) % 4 ||
        reinterpret_cast<uintptr_t>(workspace) % 16)
        return GLL_ERR_INVALID_ARG;
    const hipError_t e = launch_knn_query(Q, N, d, k, flags, Xq, Xdb, idx, d2, status, workspace,
                                          static_cast<hipStream_t>(stream));
    return e == hipSuccess ? GLL_OK : GLL_ERR_HIP;
}

int gll_extend(int64_t Q, int64_t N, int32_t kn, int32_t C, const int32_t* idx, const float* d2,
               const float* P, const float* eps_db, float eps, double* Uq, int64_t* label,
               int32_t* status, void* stream) {
    if (Q < 1 || N < 1 || kn < 1 || C < 1) return GLL_ERR_INVALID_ARG;
    if (kn > 256 || C > 256 || N > INT32_MAX / 2) return GLL_ERR_UNSUPPORTED;
    if (!idx || !d2 || !P || !Uq || !label || !status) return GLL_ERR_INVALID_ARG;
    if (!(eps > 0.f) && !eps_db) return GLL_ERR_INVALID_ARG;
    launch_k(extend_kernel, dim3(unsigned((Q + 3) / 4)), dim3(256), 0,
             static_cast<hipStream_t>(stream), idx, d2, Q, N, int(kn), int(C), P, eps_db,
             eps > 0.f ? eps : 0.f, Uq, label, status);
    return q_launched("query.hip:extend_kernel") == hipSuccess ? GLL_OK : GLL_ERR_HIP;
}

int64_t gll_query_launches(void) { return g_q_launches.load(std::memory_order_relaxed); }

}  // extern "C"
