// fused_bwd.hip -- the fused backward of one small graph: the adjoint CG solves and the feature
// gradient in one launch (cg_grad_fused_kernel), its launch plan (fused_plan, fused_plan_device:
// gll_fused_plan reaches them without a launch) and its launcher (launch_cg_grad_fused).  It is a
// gradient kernel: the solve it carries is cg_ell_body (cg_common.h), the rest is
// grad_spmm_kernel's register form (grad_common.h).
#include <cstdio>
#include <cstdlib>

#include "gll_internal.h"
#include "grad_common.h"

namespace gll {
GLL_TRACE_UNIT(fused)   // trace unit 6 (api.hip gll_trace_read)
}  // namespace gll

#include "cg_common.h"

namespace gll {

#ifdef GLL_TRACE
// fused backward, per gradient wave (a row, or a part of one): [0] release seen, [1] w loaded +
// first coefficients, [2] products done, [3] stored, [4] (row length) | (CU id << 16) |
// (XCC id << 40) | (row << 48) | (1 << 63: the entry is in use)
static __device__ unsigned long long g_fz[5 * 4096];
void trace_read_fz(unsigned long long* out) {
    (void)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_fz), sizeof(g_fz));
}
#define GLL_FZ(slot, wv, val)                                                                  \
    do {                                                                                       \
        if (lane_id() == 0 && (wv) < 4096) g_fz[(slot) * 4096 + (wv)] = (val);                 \
    } while (0)
#else
#define GLL_FZ(slot, wv, val) do {} while (0)
#endif

// ---------------------------------------------------------------------------------------
// Fused backward of one small graph (gll_backward, B = 1, fixed eps, C = 10, m <= 512: the
// north-star shape).  The adjoint solve occupies C workgroups of the GPU for ~15 us while the
// feature gradient waits behind a kernel boundary: dispatch, a gap and then cold loads of X
// rows, the CSR and P.  Here both run in ONE launch: blocks 0..C-1 are the per-column CG
// (cg_ell_body), blocks C.. the whole-row gradient (grad_spmm_kernel's register form, one wave
// per row).  A gradient wave loads everything that does not depend on the solve -- x_i, its
// edges, P_i and P_j, the first EB neighbour rows x_j -- then waits for the C columns (one
// counter, the columns' solution stored write-through), loads w_i, w_j with sc1 loads and
// finishes: the same fma order as grad_spmm_kernel, so the results agree bitwise.  All
// C + n / (NT / 64) workgroups are co-resident (checked against the occupancy at launch), so
// a waiting gradient wave never holds a CU a solve needs.  The last gradient workgroup
// re-arms the counters for the next backward on the same workspace.
//
// Row parts.  A row of more than EB edges had to gather its further neighbour rows after the
// release, EB at a time: dependent L2 gathers at the end of the launch, ~2.4 us of its tail at NS
// (profiles/rp01_fused_tail_parent.txt).  Such a row now runs as P = 2 or 4 waves ("parts"), each
// owning 1/P of the row's FEATURES (never of its edges): a part needs 1/P of the registers per
// neighbour, so it holds EB P neighbours in the same 128 VGPRs, all gathered before the release.
// Every output element is still summed over the row's edges in edge order by the same fma, so the
// gradient stays bitwise what one wave per row gives.  The launch carries spare gradient waves
// for the parts (fused_grid); the work-item plan is computed by every gradient workgroup in its
// LDS from row_len and the class order alone, so all agree on it without a message.
struct FusedPlan {
    int nt, nd;       // threads per workgroup, f32x4 vectors a lane holds of one feature row
    int grid;         // workgroups of the launch: C solves, then the gradient workgroups
    int base_grid;    // C + ceil(n / waves per workgroup): one wave per row
    int waves;        // gradient waves of the launch
    int split;        // 1: rows may run in parts
    size_t lds;       // dynamic LDS bytes per workgroup
    int64_t mat_cap;  // the solves' LDS overflow entries
};

// Parts of a row of `len` edges where a whole-row wave holds `eb` neighbour rows and a row may
// take up to `pmax` parts: the fewest of 1, 2, 4 whose slots hold the row (its first 64 edges:
// longer rows run the 64-edge loop in every part), the most allowed when none does.
__host__ __device__ inline int row_parts(int len, int eb, int pmax) {
    const int l = len < kWave ? len : kWave;
    int p = 1;
    while (p < pmax && l > eb * p) p *= 2;
    return p;
}
// Most parts a row may take: a part keeps at least one 8-byte vector per lane, and rows of one
// f32x4 per lane (d <= 256) stay whole.
__host__ __device__ constexpr int max_parts(int nd) { return nd >= 2 ? 4 : 1; }
__host__ __device__ constexpr int fused_eb(int nd) { return nd <= 2 ? 16 : 8; }

// A part's share of a feature row in a lane: NV vectors of W floats (W = 4: f32x4, W = 2: f32x2,
// the four-part form of rows of two f32x4 per lane), vector q at feature fo + W lane + 64 W q.
// Loads are load4_raw's: the address clamped into the row, never branched, and the lanes past d
// never stored.
template <int W> struct PartVec { typedef f32x4 type; };
template <> struct PartVec<2> { typedef f32x2 type; };
template <int W>
__device__ __forceinline__ typename PartVec<W>::type part_load(const float* __restrict__ p, int k,
                                                               int lim) {
    return *reinterpret_cast<const typename PartVec<W>::type*>(p + (k < lim ? k : 0));
}
template <int NV, int W>
__device__ __forceinline__ void part_load_row(typename PartVec<W>::type* r,
                                              const float* __restrict__ x, int fo, int lane, int d) {
#pragma unroll
    for (int q = 0; q < NV; ++q) r[q] = part_load<W>(x, fo + W * lane + W * kWave * q, d);
}

// Gather the feature parts of neighbours t0 .. t0 + S - 1 of the wave's current 64 edges (lane
// t holds edge t's column in cj) into v[S][NV]; slots past cnt repeat edge t0.
template <int S, int NV, int W>
__device__ __forceinline__ void part_gather(typename PartVec<W>::type* v,
                                            const float* __restrict__ X, int cj, int t0, int cnt,
                                            int fo, int lane, int d) {
#pragma unroll
    for (int u = 0; u < S; ++u) {
        const int t = t0 + u < cnt ? t0 + u : t0;
        part_load_row<NV, W>(v + u * NV, X + size_t(readlane_i(cj, t)) * d, fo, lane, d);
    }
}

// acc += cf_t (x_i - x_t) over those slots, in edge order (grad_spmm_kernel's fma per element).
// Lane t of cf holds edge t's coefficient, 0 past the row's end (edge_coef), so slots past cnt
// add 0 (x_i - x_t0) as grad_spmm_kernel's padding does; S divides 64, so t0 + u stays a lane.
// FIRST: t0 = 0 is a constant and every coefficient a readlane of a constant lane (a lane chosen
// at run time costs a scalar chain per slot: ~30 ns each on the waves' path after the release).
template <int S, int NV, int W, bool FIRST>
__device__ __forceinline__ void part_fma(typename PartVec<W>::type* acc,
                                         const typename PartVec<W>::type* xv,
                                         const typename PartVec<W>::type* v, float cf, int t0) {
    static_assert(kWave % S == 0, "slots divide the 64 edges of a pass");
    constexpr int SB = S < 16 ? S : 16;   // coefficients held as scalars at a time
#pragma unroll
    for (int u0 = 0; u0 < S; u0 += SB) {
        float sv[SB];
#pragma unroll
        for (int u = 0; u < SB; ++u) sv[u] = readlane_f(cf, FIRST ? u0 + u : t0 + u0 + u);
#pragma unroll
        for (int u = 0; u < SB; ++u) {
#pragma unroll
            for (int q = 0; q < NV; ++q) acc[q] += sv[u] * (xv[q] - v[(u0 + u) * NV + q]);
        }
    }
}

struct EllCgArgs {
    int m, C, base;
    const int32_t* row_start;
    const int32_t* row_len;
    const int32_t* ucnt;
    const int32_t* col;
    const float* wv;
    const float* diag;
    const void* b;
    float* out32;
    float rtol;
    int max_iter, mat_cap;
    int32_t* st_nonconv;
    int32_t* st_iters;
    const int4* ell;
};

template <int NT, int S, typename TB, int ND>
__global__ __launch_bounds__(NT) void cg_grad_fused_kernel(EllCgArgs c, EdgeArgs a,
                                                           const float* __restrict__ X,
                                                           float* __restrict__ out,
                                                           unsigned* fsync, int32_t* st_failed,
                                                           int32_t* st_split, int split) {
    const int C = c.C;
    if (int(blockIdx.x) < C) {
        cg_ell_body<NT, 1, S, TB, 3>(int2{int(blockIdx.x), 0}, fsync, c.m, C, c.base,
                                     c.row_start, c.row_len, c.ucnt, c.col, c.wv, c.diag,
                                     static_cast<const TB*>(c.b), nullptr, c.out32, c.rtol,
                                     c.max_iter, c.mat_cap, c.st_nonconv, c.st_iters, c.ell,
                                     0, 0, 0, 0);
        return;
    }
    // ---- gradient role: one wave per row (C = 10 classes, fixed eps)
    constexpr int NC = 10;
    constexpr int EB = ND <= 2 ? 16 : 8;   // grad_spmm_kernel's single-graph (WIDE) batch
    __shared__ int s_ok;
    const int lane = lane_id();
    // XCD-local rows (round 6).  A row's gradient gathers its neighbours' X rows, and ~86% of
    // kNN edges join rows of one class, so the rows are taken in class order --
    // argmax of P = [Y; U], the forward's output -- and each XCD's workgroups (block b runs on
    // XCD b % 8: dispatch order, §3.5, a speed assumption only) take a contiguous run of that
    // order: an XCD then gathers mostly the X rows of one or two classes, which its L2 holds,
    // instead of every XCD refilling all of X (16 MB of counter bytes for a 2 MB X at NS,
    // profiles/r05zzzz_pmc_ns.json).  Each gradient workgroup sorts the rows itself (a stable
    // counting sort in its LDS) while the adjoint solves run; a row's result does not depend on
    // which wave computes it, so the gradient is bitwise that of the row-index order.
    // A gradient workgroup's way out (thread 0): count it; the last re-arms the counters for the
    // next backward over this workspace, unless the workspace is poisoned (see the end).
    auto exit_count = [&]() {
        const unsigned ng = gridDim.x - unsigned(C);
        const unsigned old = __hip_atomic_fetch_add(fsync + 32, 1u, __ATOMIC_RELAXED,
                                                    __HIP_MEMORY_SCOPE_AGENT);
        if (old + 1u == ng &&
            __hip_atomic_load(fsync + 64, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0u) {
            __hip_atomic_store(fsync, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(fsync + 32, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(fsync + 96, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    };
    constexpr int PMAX = max_parts(ND);
    int i0, pos;
    int part = 0, nparts = 1;   // this wave's part of its row's features, of how many
    {
        extern __shared__ __attribute__((aligned(16))) float smem[];
        int* srt = reinterpret_cast<int*>(smem);   // [n] rows in class order
        int* crk = srt + a.n;                      // [n] class << 16 | rank in its 64-row chunk
        const int nch = (a.n + kWave - 1) / kWave;
        int* cnt = crk + a.n;                      // [nch][NC] rows per (chunk, class)
        constexpr int NW = NT / kWave;
        const int w = threadIdx.x >> 6;
        for (int q = w; q < nch; q += NW) {   // wave-uniform
            const int i = q * kWave + lane;
            int cls = -1;
            if (i < a.n) {
                float bv = -3.0e38f;
                cls = 0;
#pragma unroll
                for (int k = 0; k < NC; k += 2) {
                    const f32x2 v = *reinterpret_cast<const f32x2*>(a.P + size_t(i) * NC + k);
                    if (v.x > bv) bv = v.x, cls = k;
                    if (v.y > bv) bv = v.y, cls = k + 1;
                }
            }
            int rnk = 0;
#pragma unroll
            for (int k = 0; k < NC; ++k) {
                const uint64_t mk = __ballot(cls == k);
                if (cls == k) rnk = lanes_below(mk);
                if (lane == k) cnt[q * NC + k] = __popcll(mk);
            }
            if (i < a.n) crk[i] = (cls << 16) | rnk;
        }
        __syncthreads();
        if (threadIdx.x < NC) {   // each (chunk, class) run's first position, class-major
            const int k = threadIdx.x;
            int before = 0;
            for (int kk = 0; kk < k; ++kk)
                for (int q = 0; q < nch; ++q) before += cnt[q * NC + kk];
            for (int q = 0; q < nch; ++q) {
                const int c0 = cnt[q * NC + k];
                cnt[q * NC + k] = before;
                before += c0;
            }
        }
        __syncthreads();
        for (int i = threadIdx.x; i < a.n; i += NT) {
            const int v = crk[i];
            srt[cnt[(i / kWave) * NC + (v >> 16)] + (v & 0xffff)] = i;
        }
        __syncthreads();
        // this workgroup's rank in XCD-major order of the `act` gradient workgroups that take
        // work: each XCD's first act / 8 (+1) workgroups, so the items -- fewer than the launched
        // waves, the launch being sized for two parts a row -- spread over all 8 XCDs instead of
        // filling the first few; -1 for a workgroup left without work.  act = G (or a count the
        // XCDs' shares cannot cover) ranks every workgroup, the order before the row parts.
        const int G = int(gridDim.x) - C, b = int(blockIdx.x), x = b & 7;
        auto xcd_rank = [&](int act) -> int {
            const int j = (b - (C + ((x - C % 8 + 8) & 7))) >> 3;   // index on its XCD
            int ord = 0, all = 0, tot = 0, mine = 0;
#pragma unroll
            for (int xx = 0; xx < 8; ++xx) {
                const int f = C + ((xx - C % 8 + 8) & 7);   // first gradient block on XCD xx
                const int cx = f < C + G ? (C + G - 1 - f) / 8 + 1 : 0;
                const int ax = min(cx, act / 8 + (xx < act % 8 ? 1 : 0));
                if (xx < x) ord += ax, all += cx;
                if (xx == x) mine = ax;
                tot += ax;
            }
            if (tot < act) return all + j;
            return j < mine ? ord + j : -1;
        };
        pos = xcd_rank(G) * NW + w;
        i0 = pos < a.n ? srt[pos] : a.n;
        // ---- the work-item plan: row srt[r] takes row_parts() consecutive items, wave `pos`
        // takes item `pos` (a row's parts sit in one workgroup or the next: mostly one XCD)
        int nsplit = 0;
        int wrank = 0;   // < 0: no item for any wave of this workgroup
        if (PMAX > 1 && split) {
            int* ipre = crk;    // [n] (items before the row within its 64-row chunk) << 3 | parts
            int* coff = cnt;    // [nch] items before the chunk, [nch] split rows, total, splits
            for (int q = w; q < nch; q += NW) {   // wave-uniform
                const int r = q * kWave + lane;
                const int p = r < a.n ? row_parts(a.row_len[srt[r]], EB, PMAX) : 0;
                int inc = p;
#pragma unroll
                for (int off = 1; off < kWave; off <<= 1) {
                    const int t = __shfl_up(inc, off);
                    if (lane >= off) inc += t;
                }
                if (r < a.n) ipre[r] = ((inc - p) << 3) | p;
                const uint64_t ms = __ballot(p > 1);
                if (lane == kWave - 1) coff[q] = inc, coff[nch + q] = __popcll(ms);
            }
            __syncthreads();
            if (threadIdx.x == 0) {
                int items = 0, rows = 0;
                for (int q = 0; q < nch; ++q) {
                    const int c0 = coff[q];
                    coff[q] = items;
                    items += c0;
                    rows += coff[nch + q];
                }
                coff[2 * nch] = items;
                coff[2 * nch + 1] = rows;
            }
            __syncthreads();
            const int items = coff[2 * nch];
            // more items than gradient waves (the host sized the launch without the row lengths):
            // every workgroup sees the same count and keeps one wave per row
            if (items <= G * NW) {
                nsplit = coff[2 * nch + 1];
                i0 = a.n;
                wrank = xcd_rank((items + NW - 1) / NW);
                pos = wrank * NW + w;
                if (wrank >= 0 && pos < items) {
                    int cq = 0;   // chunks that begin at or before item pos
                    for (int q0 = 0; q0 < nch; q0 += kWave) {
                        const int q = q0 + lane;
                        cq += __popcll(__ballot(q < nch && coff[q] <= pos));
                    }
                    const int r = (cq - 1) * kWave + lane;
                    const int e = r < a.n ? ipre[r] : 0;
                    const int first = coff[cq - 1] + (e >> 3);
                    const uint64_t hit = __ballot((e & 7) != 0 && pos >= first && pos < first + (e & 7));
                    if (hit != 0) {   // exactly one lane: the prefix sums cover every item
                        const int l = __ffsll((unsigned long long)hit) - 1;
                        i0 = srt[(cq - 1) * kWave + l];
                        nparts = readlane_i(e & 7, l);
                        part = pos - readlane_i(first, l);
                    }
                }
            }
        }
        if (int(blockIdx.x) == C && threadIdx.x == 0 && st_split) *st_split = nsplit;
        if (wrank < 0) {
            // A workgroup without work leaves at once: it does not poll the release word beside
            // the solves.  It counts itself out like the others; the workgroup whose count is
            // last (one with work, unless it was held up) re-arms the counters.
            if (threadIdx.x == 0) exit_count();
            return;
        }
        // wave-uniform by construction; said so to the compiler, or the branches on the part's
        // shape below become lane masks that keep every shape's registers alive at once
        nparts = __builtin_amdgcn_readfirstlane(nparts);
        part = __builtin_amdgcn_readfirstlane(part);
        i0 = __builtin_amdgcn_readfirstlane(i0);
    }
    const bool live = i0 < a.n;
    const int i = live ? i0 : 0;
    const int d = a.d;
    const int beg = a.row_start[i];
    const int end = live ? beg + a.row_len[i] : beg;
    const float ei = a.eps_fixed;
    const float* xi = X + size_t(i) * d;
    // this wave's part of the row: features fo .. fo + 256 ND / nparts - 1.  by_part(f) runs f
    // with the part's shape (vectors per lane, floats per vector) as constants; nparts is
    // wave-uniform.
    const int fo = part * (4 * kWave * ND / nparts);
    auto by_part = [&](auto f) {
        if constexpr (PMAX > 1) {
            if (nparts == 2) return f(std::integral_constant<int, ND / 2>{}, std::integral_constant<int, 4>{});
            if (nparts == 4)
                return f(std::integral_constant<int, (ND >= 4 ? ND / 4 : 1)>{},
                         std::integral_constant<int, (ND >= 4 ? 4 : 2)>{});
        }
        return f(std::integral_constant<int, ND>{}, std::integral_constant<int, 4>{});
    };
    float pi[NC];
#pragma unroll
    for (int q = 0; q < NC; q += 2) {
        const f32x2 v = *reinterpret_cast<const f32x2*>(a.P + size_t(i) * NC + q);
        pi[q] = v.x, pi[q + 1] = v.y;
    }
    const __amdgpu_buffer_rsrc_t rw =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.Wadj), 0, a.n * NC * 4, 0x00020000);
    // edge e's neighbour, weight and P row (forward data: plain loads)
    auto edge_pre = [&](int e, int& cj, float& we, float* pj) {
        const bool el = e < end;
        cj = el ? a.col[e] : i;
        we = el ? a.w[e] : 0.f;
#pragma unroll
        for (int q = 0; q < NC; q += 2) {
            const f32x2 v = *reinterpret_cast<const f32x2*>(a.P + size_t(cj) * NC + q);
            pj[q] = v.x, pj[q + 1] = v.y;
        }
    };
    // its coefficient once w is complete (edge_gv_r's order)
    float wi[NC];
    auto edge_coef = [&](int e, int cj, float we, const float* pj) -> float {
        float wj[NC];
#pragma unroll
        for (int q = 0; q < NC; ++q)
            wj[q] = __builtin_bit_cast(
                float, __builtin_amdgcn_raw_buffer_load_b32(rw, (cj * NC + q) * 4, 0, kSc1W));
        float g = 0.f;
#pragma unroll
        for (int q = 0; q < NC; ++q) g = __builtin_fmaf(wi[q] - wj[q], pj[q] - pi[q], g);
        const float ej = a.eps_fixed;
        const float v = -8.f * we / (ei * ej);   // GLL.py:217/234
        return e < end ? g * v : 0.f;
    };
    int cj;
    float we, pj[NC];
    edge_pre(beg + lane, cj, we, pj);
    const int cnt0 = min(kWave, end - beg);
#ifdef GLL_TRACE
    const bool tr = int(blockIdx.x) == C && threadIdx.x == 0;   // the first gradient block
    if (tr) g_trace[16] = __builtin_amdgcn_s_memrealtime();
#endif
    // ---- wait for the C column solves (bounded: a lost solve surfaces as NaN + status)
    auto wait_release = [&]() -> bool {
        if (threadIdx.x == 0) {
            // a workspace whose previous fused backward lost a solve stays poisoned (its counter
            // may be stale) until the next forward rebuilds it: NaN again, never a stale hand-off
            int ok = __hip_atomic_load(fsync + 64, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0u;
            unsigned spins = 0;
            const unsigned long long t0 = wall_ticks();
            // the release word (fsync[96]) sits on a line no arrival adds to, so the pollers (one
            // thread per gradient workgroup) may poll it closely (round 4 polled the counter line
            // itself with ~1,000 cycles between polls, so as not to queue the columns' adds
            // behind the loads)
            while (ok && __hip_atomic_load(fsync + 96, __ATOMIC_RELAXED,
                                           __HIP_MEMORY_SCOPE_AGENT) == 0u) {
                __builtin_amdgcn_s_sleep(2);
                if ((++spins & 15u) == 0 && wall_ticks() - t0 > kWaitTicks) {   // 1 s of wall clock
                    ok = 0;
                    break;
                }
            }
            s_ok = ok;
        }
        __syncthreads();
        return s_ok != 0;
    };
    bool ok = false;
    // One straight path per shape, prefetch to store: the neighbour registers of the three shapes
    // never meet in one value (merged after the prefetch they took two register sets and
    // spilled).  A wave passes exactly one of the wait's barriers, so the workgroup's count holds.
    // A wave without an item loads nothing: it only keeps its workgroup's barrier and exit counts.
    if (!live) ok = wait_release();
    else by_part([&](auto nv, auto wd) {
        constexpr int NV = nv(), W = wd();
        constexpr int SL = EB * ND * 4 / (NV * W);   // neighbour slots of this part: EB nparts
        typedef typename PartVec<W>::type VT;
        VT xv[NV];
        part_load_row<NV, W>(xv, xi, fo, lane, d);
        VT v[SL * NV];   // 128 VGPRs whatever the shape
        part_gather<SL, NV, W>(v, X, cj, 0, cnt0, fo, lane, d);
        ok = wait_release();
#ifdef GLL_TRACE
        if (tr) g_trace[17] = __builtin_amdgcn_s_memrealtime();
        const int fzi = live ? pos : 4096;   // stamps by wave (item); the row goes in the info word
        GLL_FZ(0, fzi, __builtin_amdgcn_s_memrealtime());
#endif
#pragma unroll
        for (int q = 0; q < NC; ++q)
            wi[q] = __builtin_bit_cast(
                float, __builtin_amdgcn_raw_buffer_load_b32(rw, (i * NC + q) * 4, 0, kSc1W));
        VT acc[NV];
#pragma unroll
        for (int q = 0; q < NV; ++q) acc[q] = VT(0.f);
        for (int e0 = beg; e0 < end; e0 += kWave) {
            if (e0 != beg) edge_pre(e0 + lane, cj, we, pj);   // rows past 64 edges (hubs)
            const float cf = edge_coef(e0 + lane, cj, we, pj);
#ifdef GLL_TRACE
            if (e0 == beg) {
                float cfo = cf;
                asm volatile("s_waitcnt vmcnt(0)" : "+v"(cfo)::"memory");
                if (cfo == 12345.f) g_trace[9] = 0;
                GLL_FZ(1, fzi, __builtin_amdgcn_s_memrealtime());
            }
#endif
            const int cnt = min(kWave, end - e0);
            if (e0 != beg) part_gather<SL, NV, W>(v, X, cj, 0, cnt, fo, lane, d);
            part_fma<SL, NV, W, true>(acc, xv, v, cf, 0);
            for (int t0 = SL; t0 < cnt; t0 += SL) {
                // rows that overflow their slots fetch the rest here, after the release
                part_gather<SL, NV, W>(v, X, cj, t0, cnt, fo, lane, d);
                part_fma<SL, NV, W, false>(acc, xv, v, cf, t0);
            }
        }
#ifdef GLL_TRACE
        {
            VT ao = acc[0];
            asm volatile("" : "+v"(ao));
            if (ao.x == 12345.f) g_trace[9] = 0;
            GLL_FZ(2, fzi, __builtin_amdgcn_s_memrealtime());
        }
#endif
        if (live) {
            const float nanf_ = __builtin_nanf("");
            float* oi = out + size_t(i) * d;
#pragma unroll
            for (int q = 0; q < NV; ++q) {
                const int k = fo + W * lane + W * kWave * q;
                const VT r = ok ? acc[q] : VT(nanf_);
                if (k < d) __builtin_nontemporal_store(r, reinterpret_cast<VT*>(oi + k));
            }
        }
#ifdef GLL_TRACE
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        GLL_FZ(3, fzi, __builtin_amdgcn_s_memrealtime());
        {
            unsigned hw;
            asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw));
            unsigned xcc;
            asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
            GLL_FZ(4, fzi, (unsigned long long)(end - beg) | ((unsigned long long)((hw >> 8) & 0xffff) << 16) |
                               ((unsigned long long)(xcc & 0xff) << 40) |
                               ((unsigned long long)(i & 0xfff) << 48) | (1ull << 63));
        }
#endif
    });
    __syncthreads();
#ifdef GLL_TRACE
    if (tr) g_trace[18] = __builtin_amdgcn_s_memrealtime();
    if (threadIdx.x == 0) atomicMax(&g_trace[19], __builtin_amdgcn_s_memrealtime());
#endif
    if (threadIdx.x == 0) {
        // the last gradient workgroup re-arms the counters for a second backward over the same
        // workspace (retain_graph) -- unless some workgroup gave up on the solves: then CG
        // workgroups may still add to fsync[0] after a reset, so the workspace is poisoned
        // instead (fsync[64], cleared by the next forward's row build)
        // Relaxed agent-scope atomics throughout (all performed at the coherence point, §3.5):
        // an acquire-release count made every one of the 125 gradient workgroups write back and
        // invalidate its XCD's L2 (buffer_wbl2 / buffer_inv) on its way out.  The poison is
        // performed before this workgroup's count (the vmcnt wait on the returning atomic), so
        // the last workgroup, whose count follows every other, reads it.
        if (!ok) {
            __hip_atomic_fetch_or(fsync + 64, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (st_failed) atomicOr(st_failed, 1);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
        exit_count();
    }
}

// The fused launch's sizes, host side, without a HIP call (gll_fused_plan reaches them from a CPU
// test).  fused_lds: the dynamic LDS a workgroup asks for -- the occupancy query needs it first.
static bool fused_lds(const Layout& L, int nt, int nd, FusedPlan* pl) {
    size_t lds = 128 * 4 + size_t((L.m + 3) & ~3) * 4 * 2;   // MODE 3: P and y
    const int64_t eu_bound = int64_t(L.m + L.n) * (L.K - 1);
    int64_t cap = int64_t(kLdsDyn - lds) / 8;
    if (cap > eu_bound) cap = eu_bound;
    if (cap < 0) cap = 0;
    lds += size_t(cap) * 8;
    // the gradient workgroups' counting sort of the rows (class order): 2 n ints + the chunk
    // table; the work-item plan reuses the second n ints and the table
    const size_t sort_lds = size_t(L.n) * 8 + size_t((L.n + kWave - 1) / kWave) * 10 * 4;
    if (sort_lds > kLdsDyn) return false;
    if (lds < sort_lds) lds = sort_lds;
    pl->nt = nt;
    pl->nd = nd;
    pl->lds = lds;
    pl->mat_cap = cap;
    return true;
}
// fused_grid: the grid for `capacity` co-resident workgroups.  The route needs the base grid (one
// gradient wave per row) co-resident, as before; with row parts the launch grows towards two
// waves per row -- the host does not know the row lengths and does not wait to learn them -- but
// never past the capacity.  (NS: 145-158 of 1000 rows take 2 parts and 5-8 take 4, ~1.2 n items.)
// Should the items still exceed the waves, the kernel runs every row whole.
static bool fused_grid(const Layout& L, int64_t capacity, FusedPlan* pl) {
    const int nw = pl->nt / kWave;
    pl->base_grid = L.C + (L.n + nw - 1) / nw;
    if (capacity < pl->base_grid) return false;
    pl->split = max_parts(pl->nd) > 1 && knob(GLL_KNOB_GRAD_SPLIT) != 2;
    int64_t g = pl->base_grid;
    if (pl->split) g = std::min<int64_t>(capacity, L.C + (2 * int64_t(L.n) + nw - 1) / nw);
    pl->grid = int(g);
    pl->waves = (pl->grid - L.C) * nw;
    return true;
}
static bool fused_shape(const Layout& L, float eps_fixed, bool vec, int* nt, int* nd) {
    const int m = L.m;
    if (L.C != 10 || !(eps_fixed > 0.f) || !vec || m < 1 || m > 512 || L.RV != 0 ||
        ell_emit(L, 1) != 24 || L.d > 1024)
        return false;
    if (L.flags & (GLL_FLAG_BWD_UNFUSED | GLL_FLAG_CG_GRID | GLL_FLAG_GRAD_CHUNK)) return false;
    if (size_t(L.n) * L.d * 4 > (size_t(4) << 20)) return false;   // chunked
    *nd = L.d <= 256 ? 1 : (L.d <= 512 ? 2 : 4);
    *nt = m <= 64 ? 64 : (m <= 128 ? 128 : (m <= 256 ? 256 : 512));
    return true;
}
static void fused_plan_words(const Layout& L, const FusedPlan& pl, int32_t out[8]) {
    out[0] = pl.nt, out[1] = pl.nd, out[2] = pl.grid, out[3] = pl.base_grid, out[4] = pl.waves;
    out[5] = pl.waves - L.n, out[6] = pl.split, out[7] = int32_t(pl.lds);
}
// out: threads, vectors per lane, grid, base grid, gradient waves, spare waves (waves - n), 1 when
// rows may run in parts, LDS bytes; false when the shape does not take the fused route or the
// base grid does not fit `capacity` co-resident workgroups.
bool fused_plan(const Layout& L, float eps_fixed, bool vec, int64_t capacity, int32_t out[8]) {
    FusedPlan pl;
    int nt, nd;
    if (!fused_shape(L, eps_fixed, vec, &nt, &nd) || !fused_lds(L, nt, nd, &pl) ||
        !fused_grid(L, capacity, &pl))
        return false;
    fused_plan_words(L, pl, out);
    return true;
}

template <int NT, int ND, typename TB>
static hipError_t run_fused(const Layout& L, void* ws, const void* gbar, const float* X,
                            float eps_fixed, float* gradX, float rtol, int max_iter,
                            int32_t* st_nonconv, int32_t* st_iters, int32_t* st_failed,
                            int32_t* st_split, hipStream_t s) {
    constexpr int S = 24;
    FusedPlan pl;
    if (!fused_lds(L, NT, ND, &pl)) return hipErrorNotSupported;
    const size_t lds = pl.lds;
    const int64_t cap = pl.mat_cap;
    auto fn = cg_grad_fused_kernel<NT, S, TB, ND>;
    allow_full_lds(reinterpret_cast<const void*>(fn));
    // (cached per kernel and device: a HIP query per call is host time on the step's path)
    const int nb = occupancy_blocks(reinterpret_cast<const void*>(fn), NT, lds);
    if (!fused_grid(L, int64_t(nb) * device_cus(), &pl)) return hipErrorNotSupported;   // not co-resident: two launches
    const int G = pl.grid;
    EllCgArgs c;
    c.m = L.m;
    c.C = L.C;
    c.base = L.base;
    c.row_start = L.at<int32_t>(ws, L.row_start);
    c.row_len = L.at<int32_t>(ws, L.row_len);
    c.ucnt = L.at<int32_t>(ws, L.ucnt);
    c.col = L.at<int32_t>(ws, L.col);
    c.wv = L.at<float>(ws, L.w);
    c.diag = L.at<float>(ws, L.diag);
    c.b = gbar;
    c.out32 = L.at<float>(ws, L.Wadj) + size_t(L.base) * L.C;
    c.rtol = rtol;
    c.max_iter = max_iter;
    c.mat_cap = int(cap);
    c.st_nonconv = st_nonconv;
    c.st_iters = st_iters;
    c.ell = L.at<int4>(ws, L.ell);
    const EdgeArgs a = make_edge_args(L, 0, ws, eps_fixed);
    prof_begin(GLL_K_BWD, s);
    launch_k(fn, dim3(unsigned(G)), NT, lds, s, c, a, X, gradX, L.at<unsigned>(ws, L.fsync),
             st_failed, st_split, pl.split);
    prof_end(GLL_K_BWD, s);
    return launch_status("fused_bwd.hip:run_fused");
}

// The instantiated variants: (threads, vectors per lane) of fused_shape, each for both grad_output
// types.  One list feeds the kernel pointer fused_plan_device asks about and the runner
// launch_cg_grad_fused calls.
#define GLL_FUSED_VARIANTS(X)                                                                    \
    X(64, 1) X(64, 2) X(64, 4) X(128, 1) X(128, 2) X(128, 4) X(256, 1) X(256, 2) X(256, 4)       \
    X(512, 1) X(512, 2) X(512, 4)
struct FusedRow {
    int nt, nd, dtype;
    const void* fn;
    decltype(&run_fused<64, 1, float>) run;
};
#define GLL_FUSED_ROW(NT, ND)                                                                    \
    {NT, ND, GLL_DT_F32, reinterpret_cast<const void*>(cg_grad_fused_kernel<NT, 24, float, ND>), \
     run_fused<NT, ND, float>},                                                                  \
    {NT, ND, GLL_DT_F64, reinterpret_cast<const void*>(cg_grad_fused_kernel<NT, 24, double, ND>), \
     run_fused<NT, ND, double>},
static const FusedRow kFusedTable[] = {GLL_FUSED_VARIANTS(GLL_FUSED_ROW)};
#undef GLL_FUSED_ROW
static const FusedRow* fused_row(int nt, int nd, int dtype) {
    for (const FusedRow& r : kFusedTable)
        if (r.nt == nt && r.nd == nd && r.dtype == dtype) return &r;
    return nullptr;
}

// gll_fused_plan for the current device: the same sizing with the capacity from the occupancy of
// the kernel this shape and grad_output type run (no launch, no workspace).
bool fused_plan_device(const Layout& L, float eps_fixed, bool vec, int g_dtype, int32_t out[8]) {
    FusedPlan pl;
    int nt, nd;
    if (!fused_shape(L, eps_fixed, vec, &nt, &nd) || !fused_lds(L, nt, nd, &pl)) return false;
    const FusedRow* row = fused_row(nt, nd, g_dtype == GLL_DT_F32 ? GLL_DT_F32 : GLL_DT_F64);
    if (!row) return false;
    allow_full_lds(row->fn);
    if (!fused_grid(L, int64_t(occupancy_blocks(row->fn, nt, pl.lds)) * device_cus(), &pl))
        return false;
    fused_plan_words(L, pl, out);
    return true;
}

hipError_t launch_cg_grad_fused(const Layout& L, void* ws, const void* gbar, int g_dtype,
                                const float* X, float eps_fixed, float* gradX, float rtol,
                                int max_iter, int32_t* st_nonconv, int32_t* st_iters,
                                int32_t* st_failed, int32_t* st_split, bool vec, hipStream_t s) {
    int nt, nd;
    if (!fused_shape(L, eps_fixed, vec, &nt, &nd)) return hipErrorNotSupported;
    // (as before the table: any grad_output type other than float32 is read as float64)
    const FusedRow* row = fused_row(nt, nd, g_dtype == GLL_DT_F32 ? GLL_DT_F32 : GLL_DT_F64);
    if (!row) return hipErrorInvalidValue;
    return row->run(L, ws, gbar, X, eps_fixed, gradX, rtol, max_iter, st_nonconv, st_iters,
                    st_failed, st_split, s);
}

}  // namespace gll
