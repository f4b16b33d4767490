// cg_common.h -- what the CG units (solve.hip, fused_bwd.hip, gridcg.hip) share: the LDS limits
// (through cg_route.h), the block-wide sums and scan, the two row-access structs of the whole-GPU
// CG, and cg_ell_body -- the per-column ELL solve that both cg_ell_kernel (solve.hip) and
// cg_grad_fused_kernel (fused_bwd.hip) run.
//
// Include it after the unit's GLL_TRACE_UNIT: in a trace build cg_ell_body writes its checkpoints
// into the g_trace of the unit that instantiates it.
#pragma once

#include "cg_route.h"   // kLdsLimit, kLdsDyn: the route of cg_lds_kernel needs them on the host
#include "gll_internal.h"

namespace gll {

constexpr int kSc1W = 16;   // buffer aux bit sc1 (write-through / L2-coherent)

// Block-wide sum of two values; every thread gets the totals (fixed order -> deterministic).
template <int NT>
__device__ __forceinline__ void block_sum2(float& a, float& b, float* red, int& phase) {
    wave_sum2_dpp(a, b);
    if constexpr (NT > kWave) {
        constexpr int NW = NT / kWave;
        float* q = red + phase * 2 * NW;
        phase ^= 1;
        if (lane_id() == 0) {
            q[threadIdx.x >> 6] = a;
            q[NW + (threadIdx.x >> 6)] = b;
        }
        __syncthreads();
        a = 0.f;
        b = 0.f;
#pragma unroll
        for (int w = 0; w < NW; ++w) {
            a += q[w];
            b += q[NW + w];
        }
    }
}

// Block-wide sum of three values in two halves: post (DPP, partials to LDS, barrier) and read
// (totals from LDS); block_sum3 below is the two together.  Partials are laid out [value][wave]
// so each total is read with 16-B loads; fixed order everywhere.
template <int NT>
__device__ __forceinline__ const float* block_sum3_post(float& a, float& b, float& c, float* red,
                                                        int& phase) {
    a = dpp_add<0xB1, 0xf>(a); b = dpp_add<0xB1, 0xf>(b); c = dpp_add<0xB1, 0xf>(c);
    a = dpp_add<0x4E, 0xf>(a); b = dpp_add<0x4E, 0xf>(b); c = dpp_add<0x4E, 0xf>(c);
    a = dpp_add<0x141, 0xf>(a); b = dpp_add<0x141, 0xf>(b); c = dpp_add<0x141, 0xf>(c);
    a = dpp_add<0x140, 0xf>(a); b = dpp_add<0x140, 0xf>(b); c = dpp_add<0x140, 0xf>(c);
    a = dpp_add<0x142, 0xa>(a); b = dpp_add<0x142, 0xa>(b); c = dpp_add<0x142, 0xa>(c);
    a = dpp_add<0x143, 0xc>(a); b = dpp_add<0x143, 0xc>(b); c = dpp_add<0x143, 0xc>(c);
    if constexpr (NT == kWave) {
        a = readlane_f(a, 63);
        b = readlane_f(b, 63);
        c = readlane_f(c, 63);
        return red;
    } else {
        constexpr int NW = NT / kWave;
        constexpr int NQ = NW < 4 ? 4 : NW;
        float* q = red + phase * 3 * NQ;
        phase ^= 1;
        if (lane_id() == 63) {
            const int w = threadIdx.x >> 6;
            q[w] = a;
            q[NQ + w] = b;
            q[2 * NQ + w] = c;
        }
        __syncthreads();
        return q;
    }
}

template <int NT>
__device__ __forceinline__ void block_sum3_read(const float* q, float& a, float& b, float& c) {
    if constexpr (NT > kWave) {
        constexpr int NW = NT / kWave;
        constexpr int NQ = NW < 4 ? 4 : NW;
        a = b = c = 0.f;
        if constexpr (NW == 2 || NW == 4 || NW == 8 || NW == 16) {
            // one ds_read_b32 per lane (lane l < 3 NW: partial l % NW of value l / NW) and DPP
            // sums over aligned groups of NW lanes, instead of 3 NW / 4 ds_read_b128 that every
            // lane of every wave repeats (8 LDS cycles each, all waves right after the barrier)
            const int lane = lane_id();
            const int idx = (lane / NW) * NQ + lane % NW;
            const float t = q[lane < 3 * NW ? idx : 0];
            float v = lane < 3 * NW ? t : 0.f;
            v = dpp_add<0xB1, 0xf>(v);                              // pairs
            if constexpr (NW >= 4) v = dpp_add<0x4E, 0xf>(v);       // quads
            if constexpr (NW >= 8) v = dpp_add<0x141, 0xf>(v);      // half rows
            if constexpr (NW >= 16) v = dpp_add<0x140, 0xf>(v);     // rows
            a = readlane_f(v, 0);
            b = readlane_f(v, NW);
            c = readlane_f(v, 2 * NW);
        } else if constexpr (NW % 4 == 0) {
#pragma unroll
            for (int w = 0; w < NW; w += 4) {
                const f32x4 va = *reinterpret_cast<const f32x4*>(q + w);
                const f32x4 vb = *reinterpret_cast<const f32x4*>(q + NQ + w);
                const f32x4 vc = *reinterpret_cast<const f32x4*>(q + 2 * NQ + w);
                a += va.x; a += va.y; a += va.z; a += va.w;
                b += vb.x; b += vb.y; b += vb.z; b += vb.w;
                c += vc.x; c += vc.y; c += vc.z; c += vc.w;
            }
        } else {
#pragma unroll
            for (int w = 0; w < NW; ++w) {
                a += q[w];
                b += q[NQ + w];
                c += q[2 * NQ + w];
            }
        }
    }
}

// Block-wide sum of three values in one LDS exchange (the single-reduction CG).  Partials
// are laid out [value][wave] so each total is read with 16-B loads; fixed order everywhere.
template <int NT>
__device__ __forceinline__ void block_sum3(float& a, float& b, float& c, float* red, int& phase) {
    const float* q = block_sum3_post<NT>(a, b, c, red, phase);
    block_sum3_read<NT>(q, a, b, c);
}

// Wave-uniform maximum of a small non-negative int (setup only).
__device__ __forceinline__ int wave_max_int(int v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const int o = __shfl_xor(v, off);
        v = o > v ? o : v;
    }
    return __builtin_amdgcn_readfirstlane(v);
}

// Exclusive prefix sum of one int per thread over the block; `total` gets the block sum.
template <int NT>
__device__ __forceinline__ int block_excl_scan(int v, int* scratch, int& total) {
    const int lane = lane_id();
    int incl = v;
#pragma unroll
    for (int off = 1; off < kWave; off <<= 1) {
        const int t = __shfl_up(incl, off);
        if (lane >= off) incl += t;
    }
    if constexpr (NT == kWave) {
        total = __shfl(incl, kWave - 1);
        return incl - v;
    } else {
        constexpr int NW = NT / kWave;
        const int w = threadIdx.x >> 6;
        if (lane == kWave - 1) scratch[w] = incl;
        __syncthreads();
        int before = 0, all = 0;
#pragma unroll
        for (int q = 0; q < NW; ++q) {
            const int sw = scratch[q];
            before += q < w ? sw : 0;
            all += sw;
        }
        total = all;
        return before + incl - v;
    }
}

// Luu of the padded graph rows: row u is graph row base+u, its U block the sorted suffix of
// length ucnt[u]; off-diagonal values -W, the diagonal deg + tau kept separately.
struct LuuRows {
    const int32_t* row_start;
    const int32_t* row_len;
    const int32_t* ucnt;
    const int32_t* col;
    const float* w;
    const float* diag;
    int base;
    __device__ int begin(int u) const { return row_start[base + u] + row_len[base + u] - ucnt[u]; }
    __device__ int end(int u) const { return row_start[base + u] + row_len[base + u]; }
    __device__ int column(int e) const { return col[e] - base; }
    __device__ float value(int e) const { return -w[e]; }
    __device__ float diagonal(int u) const { return diag[u]; }
    static constexpr bool kSeparateDiag = true;
};

// General CSR with the diagonal among the entries.
struct CsrRows {
    const int32_t* rp;
    const int32_t* col;
    const float* val;
    __device__ int begin(int u) const { return rp[u]; }
    __device__ int end(int u) const { return rp[u + 1]; }
    __device__ int column(int e) const { return col[e]; }
    __device__ float value(int e) const { return val[e]; }
    __device__ float diagonal(int u) const {
        float dg = 0.f;
        for (int e = rp[u]; e < rp[u + 1]; ++e)
            if (col[e] == u) dg += val[e];
        return dg;
    }
    static constexpr bool kSeparateDiag = false;
};

// MODE: 3 Chronopoulos-Gear with a first-order Neumann preconditioner (below; the default where
// a thread owns one row), 1 Chronopoulos-Gear (one reduction, two barriers per iteration).
// (Measured and removed in round 4, DESIGN.md §3.2: the classic two-reduction form and the
// pipelined Ghysels-Vanroose form.)
// The kernel body: `gxy` = (column, graph); `fsync` (the fused backward, cg_grad_fused_kernel)
// non-null: the solution is stored write-through (sc1) and, once every wave has drained its
// stores, thread 0 adds 1 to fsync[0] -- the feature-gradient workgroups of the same launch
// wait for C arrivals (the hand-off protocol of DESIGN.md §3.5).
template <int NT, int R, int S, typename TB, int MODE>
__device__ __forceinline__ void cg_ell_body(
    int2 gxy, unsigned* fsync,
    int m, int C, int base, const int32_t* __restrict__ row_start,
    const int32_t* __restrict__ row_len, const int32_t* __restrict__ ucnt,
    const int32_t* __restrict__ col, const float* __restrict__ wv, const float* __restrict__ diag,
    const TB* __restrict__ bsrc, double* __restrict__ out64, float* __restrict__ out32,
    float rtol, int max_iter, int mat_cap, int32_t* __restrict__ st_nonconv,
    int32_t* __restrict__ st_iters, const int4* __restrict__ ell, size_t wss, size_t bs,
    size_t us, size_t sts) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    ell = gshift_at(ell, wss, gxy.y);
    row_start = gshift_br_at(row_start, wss, gxy.y);   // batched launches: graph blockIdx.y
    row_len = gshift_br_at(row_len, wss, gxy.y);
    ucnt = gshift_at(ucnt, wss, gxy.y);
    col = gshift_br_at(col, wss, gxy.y);
    wv = gshift_br_at(wv, wss, gxy.y);
    diag = gshift_at(diag, wss, gxy.y);
    bsrc = gshift_at(bsrc, bs, gxy.y);
    out64 = gshift_br_at(out64, us, gxy.y);
    out32 = gshift_br_at(out32, wss, gxy.y);
    st_nonconv = gshift_br_at(st_nonconv, sts, gxy.y);
    st_iters = gshift_br_at(st_iters, sts, gxy.y);
    const int c = gxy.x;
    const int tid = threadIdx.x;
    float* red = smem;                                  // 96 floats of reduction scratch
    int* scan = reinterpret_cast<int*>(smem + 96);      // 16 ints of scan scratch
    const int mp4 = (m + 3) & ~3;
    float* P_ = smem + 128;                             // gathered vector (x2 for MODE 3)
    int* lcol = reinterpret_cast<int*>(P_ + (MODE == 3 ? 2 : 1) * mp4);   // overflow, compacted
    float* lw = reinterpret_cast<float*>(lcol + mat_cap);
    // (Ordering rows by length so each wave's slot bound tracks its own rows was measured:
    // no gain per iteration at NS, +1.5 us of setup from the permuted ELL loads.)
    int urow[R];   // the row each thread slot handles
#pragma unroll
    for (int q = 0; q < R; ++q) urow[q] = tid + NT * q;
    int ec[R][S];
    float ew[R][S];
    int ost[R], olen[R];
    float x[R], r[R], p[R], ap[R], mi[R], dg[R];
    float rz = 0.f, bb = 0.f;
    int tov = 0;
    GLL_TRACE_SCOPE(0);
    GLL_TRACE_PT(0);
    // Every global load of the setup is issued before the first barrier (the U-block lengths,
    // the ELL slices, the diagonal and the right-hand side), so the prologue pays one memory
    // latency, not one per dependent step.
    int ulen[R];
    float bv[R];
#pragma unroll
    for (int q = 0; q < R; ++q) {
        const int u = urow[q];
        const int uc = u < m ? u : 0;
        ulen[q] = ucnt[uc];
        static_assert(S % 2 == 0, "two ELL slots per 16-B record");
#pragma unroll
        for (int s2 = 0; s2 < S / 2; ++s2) {   // column-major ELL records (row_build): coalesced
            const int4 v = ell[size_t(s2) * m + uc];
            ec[q][2 * s2] = v.x;
            ew[q][2 * s2] = __int_as_float(v.y);
            ec[q][2 * s2 + 1] = v.z;
            ew[q][2 * s2 + 1] = __int_as_float(v.w);
        }
        dg[q] = diag[uc];
        bv[q] = to_f32(bsrc[size_t(uc) * C + c]);
    }
    // entries past the S ELL slots exist only when some U block is longer than S: one
    // workgroup-wide OR (a single barrier) decides, so the usual case skips the overflow scan
    int longer = 0;
#pragma unroll
    for (int q = 0; q < R; ++q) {
        if (urow[q] >= m) ulen[q] = 0;
        longer |= ulen[q] > S ? 1 : 0;
    }
    const bool has_ovf = __syncthreads_or(longer) != 0;
#pragma unroll
    for (int q = 0; q < R; ++q) {
        const int u = urow[q];
        x[q] = r[q] = p[q] = ap[q] = mi[q] = 0.f;
        if (u >= m) {
#pragma unroll
            for (int s = 0; s < S; ++s) {
                ec[q][s] = 0;
                ew[q][s] = 0.f;
            }
            dg[q] = 0.f;
        }
        ost[q] = 0;
        olen[q] = 0;
        if (has_ovf && u < m) {
            const int len = ulen[q];   // U block = sorted suffix of graph row base + u
            ost[q] = row_start[base + u] + row_len[base + u] - len + S;
            olen[q] = len - S;
            tov += olen[q] > 0 ? olen[q] : 0;
        }
        if (u < m) {
            mi[q] = dg[q] > 0.f ? 1.f / dg[q] : 0.f;
            r[q] = mi[q] > 0.f ? bv[q] : 0.f;   // zero-diagonal rows are decoupled: x = 0
            p[q] = mi[q] * r[q];
            P_[u] = p[q];
            rz += r[q] * p[q];
            bb += r[q] * r[q];
        }
    }
    GLL_TRACE_PT(1);
    // entries beyond the ELL slices: compact them into LDS when they fit
    int ov_total = 0;
    int ooff = has_ovf ? block_excl_scan<NT>(tov, scan, ov_total) : 0;
    const bool matl = ov_total <= mat_cap;
    if (has_ovf && matl) {
#pragma unroll
        for (int q = 0; q < R; ++q) {
            for (int t = 0; t < olen[q]; ++t) {
                const int e = ost[q] + t;
                lcol[ooff + t] = col[e] - base;
                lw[ooff + t] = wv[e];
            }
            if (olen[q] > 0) {
                ost[q] = ooff;
                ooff += olen[q];
            }
        }
    }
    GLL_TRACE_PT(2);
    int phase = 0;
    if constexpr (NT > kWave) __syncthreads();
    int it = 0;
    bool conv;
    static_assert(MODE == 1 || MODE == 3, "MODE: 1 Chronopoulos-Gear, 3 with Neumann-1");
    {
        // Each wave gathers only the ELL slots some row of its own holds (wave-uniform bound
        // in groups of 4: rows average ~6 of the 24 slots at NS).
        int smax[R];
#pragma unroll
        for (int q = 0; q < R; ++q) smax[q] = wave_max_int(ulen[q] < S ? ulen[q] : S);
        auto spmv = [&](int q, float pq, const float* Pb) {
            float pv[S];
#pragma unroll
            for (int s0 = 0; s0 < S; s0 += 4) {
                if (s0 < smax[q]) {
#pragma unroll
                    for (int t = 0; t < 4 && s0 + t < S; ++t) pv[s0 + t] = Pb[ec[q][s0 + t]];
                } else {
#pragma unroll
                    for (int t = 0; t < 4 && s0 + t < S; ++t) pv[s0 + t] = 0.f;
                }
            }
            // slots past the wave's bound hold weight 0: their products are skipped, not summed
            float acc = 0.f;
#pragma unroll
            for (int s0 = 0; s0 < S; s0 += 4)
                if (s0 < smax[q]) {
#pragma unroll
                    for (int t = 0; t < 4 && s0 + t < S; ++t) acc += ew[q][s0 + t] * pv[s0 + t];
                }
            if (matl) {
                // four entries per step, every LDS read issued before use (same summation
                // order as one at a time); rows past the slots are long at K = 25
                const int e0 = ost[q], no = olen[q];
                int t = 0;
                for (; t + 4 <= no; t += 4) {
                    int c4[4];
                    float w4[4], p4[4];
#pragma unroll
                    for (int v = 0; v < 4; ++v) {
                        c4[v] = lcol[e0 + t + v];
                        w4[v] = lw[e0 + t + v];
                    }
#pragma unroll
                    for (int v = 0; v < 4; ++v) p4[v] = Pb[c4[v]];
#pragma unroll
                    for (int v = 0; v < 4; ++v) acc += w4[v] * p4[v];
                }
                for (; t < no; ++t) acc += lw[e0 + t] * Pb[lcol[e0 + t]];
            } else {   // from the CSR (L2), four entries in flight per step
                const int e0 = ost[q], no = olen[q];
                int t = 0;
                for (; t + 4 <= no; t += 4) {
                    int c4[4];
                    float w4[4], p4[4];
#pragma unroll
                    for (int v = 0; v < 4; ++v) {
                        c4[v] = col[e0 + t + v];
                        w4[v] = wv[e0 + t + v];
                    }
#pragma unroll
                    for (int v = 0; v < 4; ++v) p4[v] = Pb[c4[v] - base];
#pragma unroll
                    for (int v = 0; v < 4; ++v) acc += w4[v] * p4[v];
                }
                for (; t < no; ++t) acc += wv[e0 + t] * Pb[col[e0 + t] - base];
            }
            return dg[q] * pq - acc;   // (Luu u)_row = (deg + tau) u_row - sum_j W_rowj u_j
        };
        {
        // Chronopoulos-Gear single-reduction PCG: one fused (r.u, w.u, r.r) exchange and one
        // publish barrier per iteration (classic PCG: two exchanges + publish = 3 barriers).
        // s = A p by recurrence; u = M^-1 r is what is published and multiplied.
        // MODE 3: M^-1 = D^-1 + D^-1 N D^-1 (A = D - N, N the off-diagonal weights W_uj >= 0:
        // the first two terms of the Neumann series of A^-1), applied as y = D^-1 r published,
        // u = y + D^-1 (N y) -- one more gather and barrier per iteration.  It is SPD where
        // D^-1/2 A D^-1/2 has its spectrum in (0, 2), which diagonal dominance gives, and turns
        // that spectrum [l, h] into {x (2 - x)}: at NS [0.44, 1.32] -> [0.69, 1], 11 -> 6
        // iterations, so each iteration's fixed reduction and step-size latency is paid about
        // half as often (tools/ab_flags.py).
        constexpr bool NEU = MODE == 3;
        float* P2_ = P_ + mp4;   // y = D^-1 r (MODE 3)
        if constexpr (NEU) {
            // setup left y0 = D^-1 r0 in P_ (as p) and rz = (r0, y0): u0 = y0 + D^-1 N y0
            rz = 0.f;
#pragma unroll
            for (int q = 0; q < R; ++q) {
                const float t = -spmv(q, 0.f, P_);   // (N y0)_row
                p[q] = p[q] + mi[q] * t;
                rz += r[q] * p[q];
            }
            __syncthreads();   // every gather of y0 is done before u0 overwrites it
#pragma unroll
            for (int q = 0; q < R; ++q) {
                const int u = urow[q];
                if (u < m) P_[u] = p[q];
            }
            __syncthreads();
        }
        // pre-step: w0 = A u0 (u0 = p, already published), gamma0 = (r,u), delta0 = (w,u)
        float sv[R];
        float dl = 0.f;
#pragma unroll
        for (int q = 0; q < R; ++q) {
            sv[q] = spmv(q, p[q], P_);
            dl += p[q] * sv[q];
        }
        block_sum3<NT>(rz, bb, dl, red, phase);
        GLL_TRACE_PT(3);
        const float tol2 = rtol * rtol * bb;
        conv = !(bb > 0.f);
        float gam = rz;
        float alpha = dl > 0.f ? gam / dl : 0.f;
        if (!(dl > 0.f)) alpha = -1.f;   // breakdown before the first step
#ifdef GLL_TRACE
#define GLL_TRACE_CYC(i)                                                                       \
    do {                                                                                       \
        if (it == 3 && blockIdx.x == 0 && threadIdx.x == 0) g_trace[i] = __builtin_amdgcn_s_memtime(); \
    } while (0)
#else
#define GLL_TRACE_CYC(i) do {} while (0)
#endif
        while (!conv && alpha > 0.f && it < max_iter) {
            ++it;
            GLL_TRACE_CYC(10);
#pragma unroll
            for (int q = 0; q < R; ++q) {
                x[q] += alpha * p[q];
                r[q] -= alpha * sv[q];
                ap[q] = mi[q] * r[q];                       // u = M^-1 r (MODE 3: y)
                const int u = urow[q];
                if (u < m) (NEU ? P2_ : P_)[u] = ap[q];
            }
            if constexpr (NEU) {   // u = y + D^-1 (N y)
                __syncthreads();
#pragma unroll
                for (int q = 0; q < R; ++q) {
                    ap[q] += mi[q] * -spmv(q, 0.f, P2_);
                    const int u = urow[q];
                    if (u < m) P_[u] = ap[q];
                }
            }
            GLL_TRACE_CYC(11);
            if constexpr (NT > kWave) __syncthreads();
            if (it == 1) GLL_TRACE_PT(4);
            GLL_TRACE_CYC(12);
            float gn = 0.f, de = 0.f, rr = 0.f;
            float w[R];
#pragma unroll
            for (int q = 0; q < R; ++q) {
                w[q] = spmv(q, ap[q], P_);
                gn += r[q] * ap[q];
                de += w[q] * ap[q];
                rr += r[q] * r[q];
            }
#ifdef GLL_TRACE
            if (it == 3 && blockIdx.x == 0 && threadIdx.x == 0 && de == 12345.f) g_trace[9] = 0;
#endif
            GLL_TRACE_CYC(13);
            block_sum3<NT>(gn, de, rr, red, phase);
            GLL_TRACE_CYC(14);
            if (it == 1) GLL_TRACE_PT(6);
            if (rr <= tol2) {
                conv = true;
                break;
            }
            // one reciprocal on the critical path: alpha' = gn / (de - beta gn / alpha)
            //                                             = gn alpha / (alpha de - beta gn)
            const float beta = gn * __builtin_amdgcn_rcpf(gam);
            const float den = alpha * de - beta * gn;
            if (!(den > 0.f)) break;   // breakdown or NaN: reported as non-converged
            alpha = (gn * alpha) * __builtin_amdgcn_rcpf(den);
            gam = gn;
#pragma unroll
            for (int q = 0; q < R; ++q) {
                p[q] = ap[q] + beta * p[q];
                sv[q] = w[q] + beta * sv[q];
            }
            GLL_TRACE_CYC(15);
        }
        }
    }
    GLL_TRACE_PT(8);
#pragma unroll
    for (int q = 0; q < R; ++q) {
        const int u = urow[q];
        if (u < m) {
            if (out64) out64[size_t(u) * C + c] = double(x[q]);
            if (out32) {
                if (fsync)
                    __hip_atomic_store(out32 + size_t(u) * C + c, x[q], __ATOMIC_RELAXED,
                                       __HIP_MEMORY_SCOPE_AGENT);   // global_store ... sc1
                else
                    out32[size_t(u) * C + c] = x[q];
            }
        }
    }
    if (tid == 0) {
        if (st_iters && (sts != 0 || gxy.y == 0 || !conv)) atomicMax(st_iters, it);   // sink: see gll.h
        if (!conv && st_nonconv) atomicAdd(st_nonconv, 1);
    }
    if (fsync) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        // the column completing the count writes the release word the gradient blocks poll
        // (on its own line: the pollers never read the line the arrivals add to)
        if (tid == 0 &&
            __hip_atomic_fetch_add(fsync, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) + 1u ==
                unsigned(C))
            __hip_atomic_store(fsync + 96, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    GLL_TRACE_PT(9);
}

}  // namespace gll
