// solve.hip -- Jacobi-preconditioned conjugate gradients on Luu (and on a general CSR).
//
// Replaces the SuperLU `spsolve(Luu, -Lul Y)` of the forward (/root/reference/GLL.py:53)
// and `spsolve(Luu, grad_output)` of the backward (GLL.py:93); the algorithm is the
// per-column masked CG of stable_conjgrad (GLL.py:247-276) with a Jacobi preconditioner
// (the reference's commented-out variant, GLL.py:55-64), WITHOUT its `p = r` aliasing
// quirk.  Each right-hand-side column is an independent system, so
// one workgroup owns one column: no inter-workgroup traffic, no host synchronisation, the
// iteration loop and the convergence test live on the device.
//
// Luu is never materialised: row u (graph row i = base + u) is
//     diag[u] * p_u - sum_{e in row i, col_e >= base} w_e * p_{col_e - base}
// over the sorted CSR of the symmetric kNN graph (labeled columns first, so the U block of
// a row is a suffix of the row).
//
// Per-column kernels.  cg_route (cg_route.h) says which one solves a problem, cg_dispatch launches
// it from the table of instantiated variants below; single graphs with m > 2048 take the
// whole-GPU CG of gridcg.hip first.  cg_ell_body, which cg_ell_kernel shares with the fused
// backward (fused_bwd.hip), and the block-wide sums live in cg_common.h.
//   cg_ell_kernel (short U rows, m <= 4096): a thread owns R rows and keeps everything about
//     them in registers, including the first S entries of each U row as an ELL slice; entries
//     past S are compacted into LDS.  Single-reduction (Chronopoulos-Gear) PCG: one fused
//     three-value exchange and one publish barrier per iteration.
//   cg_vr_kernel (long U rows: K = 25, the FullySup shape): the U block cut into "virtual
//     rows" of 8 entries dealt out evenly to the threads (see its comment).
//   cg_lds_kernel: vectors in LDS or global memory, for systems larger than either.
#include <cstdio>
#include <cstdlib>
#include <mutex>
#include <unordered_set>

#include "gll_internal.h"

namespace gll {
GLL_TRACE_UNIT(solve)
}  // namespace gll

#include "cg_common.h"

namespace gll {

// Opt a kernel into all of the 160 KiB of LDS its static allocation leaves for dynamic use,
// once per kernel (host-side cost).  The attribute call's status is consumed here: a failure
// must not linger as the thread's last error and surface at an unrelated launch.
void allow_full_lds(const void* fn) {
    static std::mutex mu;
    static std::unordered_set<const void*> done;
    std::lock_guard<std::mutex> lk(mu);
    if (done.insert(fn).second) {
        hipFuncAttributes at{};
        size_t stat = 0;
        if (hipFuncGetAttributes(&at, fn) == hipSuccess) stat = at.sharedSizeBytes;
        (void)hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize,
                                  int(kLdsLimit - stat));
        (void)hipGetLastError();
    }
}

// The batched geometry (256 x 2, MODE 1: B x C > 256 column workgroups) must keep three
// workgroups per CU -- B = 64 NS is 640 of them, all resident at once -- so <= 168 VGPRs.
template <int NT, int R, int S, typename TB, int MODE>
__global__ __launch_bounds__(NT) __attribute__((amdgpu_waves_per_eu(NT == 256 && R == 2 && MODE == 1 ? 3 : 1)))
void cg_ell_kernel(
    int m, int C, int base, const int32_t* __restrict__ row_start,
    const int32_t* __restrict__ row_len, const int32_t* __restrict__ ucnt,
    const int32_t* __restrict__ col, const float* __restrict__ wv, const float* __restrict__ diag,
    const TB* __restrict__ bsrc, double* __restrict__ out64, float* __restrict__ out32,
    float rtol, int max_iter, int mat_cap, int32_t* __restrict__ st_nonconv,
    int32_t* __restrict__ st_iters, const int4* __restrict__ ell, size_t wss, size_t bs,
    size_t us, size_t sts) {
    // batch_xy once: per pointer it re-reads gridDim and divides
    cg_ell_body<NT, R, S, TB, MODE>(batch_xy<true>(), nullptr, m, C, base, row_start, row_len,
                                    ucnt, col, wv, diag, bsrc, out64, out32, rtol, max_iter,
                                    mat_cap, st_nonconv, st_iters, ell, wss, bs, us, sts);
}

// --------------------------------------------------------------------------------------
// Balanced per-column CG for long U rows (cg_vr_kernel).
//
// At K = 25 (the FullySup caller, FullySup.py:156) a U row of Luu holds 27 entries on average
// and up to ~75, so a thread-per-row SpMV loops every wave to its longest row, and past the
// register slots each entry costs three LDS operations (column, weight, gathered value).
// Here the U block is cut into "virtual rows" of kVS = 8 consecutive entries (a row of L
// entries gives ceil(L/8)), which row_build writes pre-packed (16-bit LDS byte offsets of the
// columns, then the weights; gll_internal.h kVrSlot).  The virtual rows -- not the rows -- are
// dealt out to the threads, v = j * NT + tid for j < RV, and held in registers for the whole
// solve.  An SpMV is then one LDS gather per entry, the same count for every thread, plus one
// partial sum per virtual row written to LDS.
//
// The row sums of A u are needed only after the iteration's reduction barrier (for the
// recurrence s = w + beta s), so they are read there from the partials -- no extra barrier.
// The (w, u) product the reduction needs before that barrier is formed per virtual row
// instead: (w, u) = sum_rows diag u^2 - sum_v u_row(v) part_v.
// Fixed partition and fixed summation order: deterministic.  Virtual rows past the register
// capacity NT x RV (an underestimated size) or past the VRM slots of a row (hubs) are summed
// by their row's thread from the CSR.
// --------------------------------------------------------------------------------------
template <int NT, int R, int RV, typename TB>
__global__ __launch_bounds__(NT) void cg_vr_kernel(
    int m, int C, int base, int VRM, const int32_t* __restrict__ row_start,
    const int32_t* __restrict__ row_len, const int32_t* __restrict__ ucnt,
    const int32_t* __restrict__ col, const float* __restrict__ wv, const float* __restrict__ diag,
    const char* __restrict__ vrs, const TB* __restrict__ bsrc, double* __restrict__ out64,
    float* __restrict__ out32, float rtol, int max_iter, int32_t* __restrict__ st_nonconv,
    int32_t* __restrict__ st_iters, size_t wss, size_t bs, size_t us, size_t sts) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int2 gxy = batch_xy<true>();   // once: per pointer it re-reads gridDim and divides
    row_start = gshift_at(row_start, wss, gxy.y);
    row_len = gshift_at(row_len, wss, gxy.y);
    ucnt = gshift_at(ucnt, wss, gxy.y);
    col = gshift_at(col, wss, gxy.y);
    wv = gshift_at(wv, wss, gxy.y);
    diag = gshift_at(diag, wss, gxy.y);
    vrs = gshift_at(vrs, wss, gxy.y);
    bsrc = gshift_at(bsrc, bs, gxy.y);
    out64 = gshift_br_at(out64, us, gxy.y);
    out32 = gshift_br_at(out32, wss, gxy.y);
    st_nonconv = gshift_br_at(st_nonconv, sts, gxy.y);
    st_iters = gshift_br_at(st_iters, sts, gxy.y);
    constexpr int VCAP = NT * RV;
    const int c = gxy.x;
    const int tid = threadIdx.x;
    const int mp4 = (m + 3) & ~3;
    float* red = smem;                                   // 96 floats of reduction scratch
    int* scan = reinterpret_cast<int*>(smem + 96);       // 16 ints of scan scratch
    float* P_ = smem + 128;                              // the published vector u
    // partial sums, row-padded: row u's at vpart[vpad_u ..), vpad_u 16-B aligned, so the row
    // sums read them four at a time
    float* vpart = P_ + mp4;                             // VCAP + 4 mp4
    int* vmap = reinterpret_cast<int*>(vpart + VCAP + 4 * mp4);   // VCAP: (row << 10) | (j << 4) | len
    int* vpad = vmap + VCAP;                             // mp4: row u's first partial
    GLL_TRACE_SCOPE(0);
    GLL_TRACE_PT(0);

    // ---- rows this thread owns (u = tid + NT q): setup loads all issued together
    int ulen[R], est[R], vs[R], nvc[R], sps[R], spe[R], vp[R];
    float dg[R], bv[R], mi[R], x[R], r[R], p[R], sv[R], uu[R];
#pragma unroll
    for (int q = 0; q < R; ++q) {
        const int u = tid + NT * q;
        const int uc = u < m ? u : 0;
        ulen[q] = ucnt[uc];
        est[q] = row_start[base + uc] + row_len[base + uc];
        dg[q] = diag[uc];
        bv[q] = to_f32(bsrc[size_t(uc) * C + c]);
    }
    int tv = 0, tp = 0;
#pragma unroll
    for (int q = 0; q < R; ++q) {
        if (tid + NT * q >= m) {
            ulen[q] = 0;
            dg[q] = 0.f;
        }
        est[q] -= ulen[q];   // the U block is the row's sorted suffix
        const int nv = min((ulen[q] + kVS - 1) / kVS, VRM);
        tv += nv;
        tp += (nv + 3) & ~3;
    }
    int V = 0, VP = 0;
    int v0 = block_excl_scan<NT>(tv, scan, V);
    __syncthreads();   // the scan scratch is reused
    int p0 = block_excl_scan<NT>(tp, scan, VP);
    float rz = 0.f, bb = 0.f;
#pragma unroll
    for (int q = 0; q < R; ++q) {
        const int u = tid + NT * q;
        const int nv = min((ulen[q] + kVS - 1) / kVS, VRM);
        vs[q] = v0;
        vp[q] = p0;
        if (u < m) vpad[u] = p0;
        p0 += (nv + 3) & ~3;
        for (int j = 0; j < nv && v0 + j < VCAP; ++j)
            vmap[v0 + j] = (u << 10) | (j << 4) | min(kVS, ulen[q] - kVS * j);
        nvc[q] = v0 + nv <= VCAP ? nv : (v0 < VCAP ? VCAP - v0 : 0);
        if (nvc[q] == 0) vp[q] = 0;   // no partials held (past the capacity): stay in bounds
        sps[q] = est[q] + kVS * nvc[q];   // entries past the held virtual rows: from the CSR
        spe[q] = est[q] + ulen[q];
        v0 += nv;
        mi[q] = dg[q] > 0.f ? 1.f / dg[q] : 0.f;
        r[q] = mi[q] > 0.f ? bv[q] : 0.f;   // zero-diagonal rows are decoupled: x = 0
        x[q] = sv[q] = 0.f;
        p[q] = uu[q] = mi[q] * r[q];
        if (u < m) P_[u] = uu[q];
        rz += r[q] * uu[q];
        bb += r[q] * r[q];
    }
    // wave-uniform bound of the partial sums each row reads after the reduction
    int nvmax[R];
#pragma unroll
    for (int q = 0; q < R; ++q) nvmax[q] = wave_max_int(nvc[q]);
    GLL_TRACE_PT(1);
    __syncthreads();
    // ---- this thread's virtual rows, packed by row_build: 3 x 16-B loads each, consecutive
    // threads on consecutive virtual rows
    uint32_t cpk[RV][kVS / 2];
    float ew[RV][kVS];
    int vrow[RV], vmax[RV], pidx[RV];
    const int Vlive = V < VCAP ? V : VCAP;
#pragma unroll
    for (int j = 0; j < RV; ++j) {
        const int v = j * NT + tid;
        const int info = vmap[v < Vlive ? v : 0];
        const int len = v < Vlive ? (info & 15) : 0;
        vrow[j] = v < Vlive ? (info >> 10) : 0;
        pidx[j] = v < Vlive ? vpad[info >> 10] + ((info >> 4) & 63) : VCAP + 4 * mp4 - 1;
        const int slot = v < Vlive ? (info >> 10) * VRM + ((info >> 4) & 63) : 0;
        const uint4 cw = *reinterpret_cast<const uint4*>(vrs + size_t(slot) * kVrSlot);
        const f32x4 w0 = *reinterpret_cast<const f32x4*>(vrs + size_t(slot) * kVrSlot + 16);
        const f32x4 w1 = *reinterpret_cast<const f32x4*>(vrs + size_t(slot) * kVrSlot + 32);
        // a dead slot loads virtual row 0: masked through an opaque mask (a select on the
        // loaded values would let the compiler sink the loads into a branch)
        uint32_t mk = v < Vlive ? 0xffffffffu : 0u;
        asm volatile("" : "+v"(mk));
        cpk[j][0] = cw.x & mk;
        cpk[j][1] = cw.y & mk;
        cpk[j][2] = cw.z & mk;
        cpk[j][3] = cw.w & mk;
        ew[j][0] = __uint_as_float(__float_as_uint(w0.x) & mk);
        ew[j][1] = __uint_as_float(__float_as_uint(w0.y) & mk);
        ew[j][2] = __uint_as_float(__float_as_uint(w0.z) & mk);
        ew[j][3] = __uint_as_float(__float_as_uint(w0.w) & mk);
        ew[j][4] = __uint_as_float(__float_as_uint(w1.x) & mk);
        ew[j][5] = __uint_as_float(__float_as_uint(w1.y) & mk);
        ew[j][6] = __uint_as_float(__float_as_uint(w1.z) & mk);
        ew[j][7] = __uint_as_float(__float_as_uint(w1.w) & mk);
        vmax[j] = wave_max_int(len);
    }
    GLL_TRACE_PT(3);
    const char* Pb = reinterpret_cast<const char*>(P_);
    // A u over this thread's virtual rows: partials to LDS, returns sum_v u_row(v) part_v
    auto spmv = [&]() {
        float dl = 0.f;
        // the packed offsets are "redefined" here so the compiler cannot hoist their unpacked
        // halves out of the iteration loop (that doubles the registers they take)
#pragma unroll
        for (int j = 0; j < RV; ++j)
#pragma unroll
            for (int h = 0; h < kVS / 2; ++h) asm volatile("" : "+v"(cpk[j][h]));
#pragma unroll
        for (int j = 0; j < RV; ++j) {
            if (vmax[j] > 0) {
                float pv[kVS];
#pragma unroll
                for (int k0 = 0; k0 < kVS; k0 += 4) {
                    if (k0 < vmax[j]) {
#pragma unroll
                        for (int k = k0; k < k0 + 4; ++k) {
                            const uint32_t off = (k & 1) ? (cpk[j][k >> 1] >> 16)
                                                         : (cpk[j][k >> 1] & 0xffffu);
                            pv[k] = *reinterpret_cast<const float*>(Pb + off);
                        }
                    } else {
#pragma unroll
                        for (int k = k0; k < k0 + 4; ++k) pv[k] = 0.f;
                    }
                }
                const float ur = P_[vrow[j]];
                float acc = 0.f;
#pragma unroll
                for (int k = 0; k < kVS; ++k) acc += ew[j][k] * pv[k];
                vpart[pidx[j]] = acc;
                dl += ur * acc;
            }
            // one virtual row's gathers in flight at a time: hoisting all RV x 8 spills
            __builtin_amdgcn_sched_barrier(0);
        }
        return dl;
    };
    // entries past the held virtual rows (rare): this row's thread sums them from the CSR
    auto spill = [&](int q) {
        float acc = 0.f;
        for (int e = sps[q]; e < spe[q]; ++e) acc += wv[e] * P_[col[e] - base];
        return acc;
    };
    // after the reduction barrier: (A u)_row = diag u - sum of the row's partials; the loads
    // of every row of the thread are issued together, four partials per row per step
    // the first 8 of a row's partials (rows up to 64 entries) come in two 16-B loads per row,
    // every row's issued before any is used; longer rows loop over the rest
    const int vplim = VCAP + 4 * mp4 - 4;
    auto rowsums = [&](float* wr, const float* spl) {
        f32x4 pv[R][2];
#pragma unroll
        for (int q = 0; q < R; ++q)
#pragma unroll
            for (int h = 0; h < 2; ++h)
                pv[q][h] = *reinterpret_cast<const f32x4*>(vpart + min(vp[q] + 4 * h, vplim));
#pragma unroll
        for (int q = 0; q < R; ++q) {
            float acc = 0.f;
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                acc += 4 * h + 0 < nvc[q] ? pv[q][h].x : 0.f;
                acc += 4 * h + 1 < nvc[q] ? pv[q][h].y : 0.f;
                acc += 4 * h + 2 < nvc[q] ? pv[q][h].z : 0.f;
                acc += 4 * h + 3 < nvc[q] ? pv[q][h].w : 0.f;
            }
            for (int t = 8; t < nvmax[q]; ++t) acc += t < nvc[q] ? vpart[vp[q] + t] : 0.f;
            wr[q] = dg[q] * uu[q] - (acc + spl[q]);
        }
    };

    int phase = 0;
    int it = 0;
    bool conv;
    // pre-step: w0 = A u0, gamma0 = (r,u), delta0 = (w,u)
    float spl[R];
    float dl = -spmv();
#pragma unroll
    for (int q = 0; q < R; ++q) {
        spl[q] = spill(q);
        dl += dg[q] * uu[q] * uu[q] - uu[q] * spl[q];
    }
    block_sum3<NT>(rz, bb, dl, red, phase);
    rowsums(sv, spl);
    GLL_TRACE_PT(4);
    const float tol2 = rtol * rtol * bb;
    conv = !(bb > 0.f);
    float gam = rz;
    float alpha = dl > 0.f ? gam / dl : 0.f;
    if (!(dl > 0.f)) alpha = -1.f;   // breakdown before the first step
    while (!conv && alpha > 0.f && it < max_iter) {
        ++it;
        GLL_TRACE_CYC(10);
#pragma unroll
        for (int q = 0; q < R; ++q) {
            x[q] += alpha * p[q];
            r[q] -= alpha * sv[q];
            uu[q] = mi[q] * r[q];                       // u = M^-1 r
            const int u = tid + NT * q;
            if (u < m) P_[u] = uu[q];
        }
        GLL_TRACE_CYC(11);
        __syncthreads();
        GLL_TRACE_CYC(12);
        float gn = 0.f, de = -spmv(), rr = 0.f;
#pragma unroll
        for (int q = 0; q < R; ++q) {
            spl[q] = spill(q);
            gn += r[q] * uu[q];
            de += dg[q] * uu[q] * uu[q] - uu[q] * spl[q];
            rr += r[q] * r[q];
        }
#ifdef GLL_TRACE
        if (it == 3 && blockIdx.x == 0 && threadIdx.x == 0 && de == 12345.f) g_trace[9] = 0;
#endif
        GLL_TRACE_CYC(13);
        block_sum3<NT>(gn, de, rr, red, phase);
        GLL_TRACE_CYC(14);
        float w[R];
        rowsums(w, spl);
        if (rr <= tol2) {
            conv = true;
            break;
        }
        const float beta = gn * __builtin_amdgcn_rcpf(gam);
        const float den = alpha * de - beta * gn;
        if (!(den > 0.f)) break;   // breakdown or NaN: reported as non-converged
        alpha = (gn * alpha) * __builtin_amdgcn_rcpf(den);
        gam = gn;
#pragma unroll
        for (int q = 0; q < R; ++q) {
            p[q] = uu[q] + beta * p[q];
            sv[q] = w[q] + beta * sv[q];
        }
        GLL_TRACE_CYC(15);
    }
    GLL_TRACE_PT(8);
#pragma unroll
    for (int q = 0; q < R; ++q) {
        const int u = tid + NT * q;
        if (u < m) {
            if (out64) out64[size_t(u) * C + c] = double(x[q]);
            if (out32) out32[size_t(u) * C + c] = x[q];
        }
    }
    if (tid == 0) {
        if (st_iters && (sts != 0 || gxy.y == 0 || !conv)) atomicMax(st_iters, it);   // sink: see gll.h
        if (!conv && st_nonconv) atomicAdd(st_nonconv, 1);
    }
}

// Large systems: vectors in LDS (<= 160 KiB) or in the workspace.
template <int NT, typename TB>
__global__ __launch_bounds__(NT) void cg_lds_kernel(
    int m, int C, int base, const int32_t* __restrict__ row_start,
    const int32_t* __restrict__ row_len, const int32_t* __restrict__ ucnt,
    const int32_t* __restrict__ col,
    const float* __restrict__ wv, const float* __restrict__ diag, const TB* __restrict__ bsrc,
    double* __restrict__ out64, float* __restrict__ out32, float rtol, int max_iter,
    float* __restrict__ gvec, int vec_in_lds, int32_t* __restrict__ st_nonconv,
    int32_t* __restrict__ st_iters, size_t wss, size_t bs, size_t us, size_t sts) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int2 gxy = batch_xy<true>();   // once: per pointer it re-reads gridDim and divides
    row_start = gshift_at(row_start, wss, gxy.y);
    row_len = gshift_at(row_len, wss, gxy.y);
    ucnt = gshift_at(ucnt, wss, gxy.y);
    col = gshift_at(col, wss, gxy.y);
    wv = gshift_at(wv, wss, gxy.y);
    diag = gshift_at(diag, wss, gxy.y);
    bsrc = gshift_at(bsrc, bs, gxy.y);
    out64 = gshift_at(out64, us, gxy.y);
    out32 = gshift_at(out32, wss, gxy.y);
    gvec = gshift_at(gvec, wss, gxy.y);
    st_nonconv = gshift_at(st_nonconv, sts, gxy.y);
    st_iters = gshift_at(st_iters, sts, gxy.y);
    const int c = gxy.x;
    const int tid = threadIdx.x;
    float* red = smem;
    float* vb = vec_in_lds ? smem + 64 : gvec + size_t(c) * 5 * m;
    float *X_ = vb, *R_ = vb + m, *P_ = vb + 2 * m, *A_ = vb + 3 * m, *M_ = vb + 4 * m;
    float rz = 0.f, bb = 0.f;
    for (int u = tid; u < m; u += NT) {
        const float dg = diag[u];
        const float mi = dg > 0.f ? 1.f / dg : 0.f;
        const float bu = to_f32(bsrc[size_t(u) * C + c]);
        const float rb = mi > 0.f ? bu : 0.f;
        X_[u] = 0.f;
        R_[u] = rb;
        M_[u] = mi;
        P_[u] = mi * rb;
        rz += rb * mi * rb;
        bb += rb * rb;
    }
    int phase = 0;
    __syncthreads();
    block_sum2<NT>(rz, bb, red, phase);
    const float tol2 = rtol * rtol * bb;
    int it = 0;
    bool conv = !(bb > 0.f);
    while (!conv && it < max_iter) {
        ++it;
        float pap = 0.f, unused = 0.f;
        for (int u = tid; u < m; u += NT) {
            const int i = base + u;
            const int end = row_start[i] + row_len[i];
            float acc = 0.f;
            for (int e = end - ucnt[u]; e < end; ++e) acc += wv[e] * P_[col[e] - base];
            const float ap = diag[u] * P_[u] - acc;
            A_[u] = ap;
            pap += P_[u] * ap;
        }
        block_sum2<NT>(pap, unused, red, phase);
        if (!(pap > 0.f)) break;
        const float alpha = rz / pap;
        float rr = 0.f, rzn = 0.f;
        for (int u = tid; u < m; u += NT) {
            X_[u] += alpha * P_[u];
            const float ru = R_[u] - alpha * A_[u];
            R_[u] = ru;
            rr += ru * ru;
            rzn += ru * M_[u] * ru;
        }
        block_sum2<NT>(rr, rzn, red, phase);
        if (rr <= tol2) {
            conv = true;
            break;
        }
        const float beta = rzn / rz;
        rz = rzn;
        for (int u = tid; u < m; u += NT) P_[u] = M_[u] * R_[u] + beta * P_[u];
        __syncthreads();
    }
    for (int u = tid; u < m; u += NT) {
        if (out64) out64[size_t(u) * C + c] = double(X_[u]);
        if (out32) out32[size_t(u) * C + c] = X_[u];
    }
    if (tid == 0) {
        if (st_iters && (sts != 0 || gxy.y == 0 || !conv)) atomicMax(st_iters, it);   // sink: see gll.h
        if (!conv && st_nonconv) atomicAdd(st_nonconv, 1);
    }
}

template <int NT, int R, int S, typename TB, int MODE>
static hipError_t run_ell(const Layout& L, const Batch& bt, void* ws, const TB* b, size_t bs,
                          double* out64, float* out32, float rtol, int max_iter,
                          int32_t* st_nonconv, int32_t* st_iters, hipStream_t s) {
    size_t lds = 128 * 4 + size_t((L.m + 3) & ~3) * 4 * (MODE == 3 ? 2 : 1);
    // entries past the ELL slices are compacted into LDS up to kOvfLds of them, the rest read
    // from the CSR; batched launches cap them so 4 workgroups still share a CU (a full-LDS
    // request would pin one per CU); a single graph's C workgroups take all the LDS there is
    // (K = 25 rows overflow 16 slots by ~14K entries at m = 1250)
    const int64_t kOvfLds = bt.B == 1 ? int64_t(1) << 30 : 2048;
    const int64_t eu_bound = int64_t(L.m + L.n) * (L.K - 1);
    int64_t cap = int64_t(kLdsDyn - lds) / 8;
    if (cap > eu_bound) cap = eu_bound;
    if (cap > kOvfLds) cap = kOvfLds;
    if (cap < 0) cap = 0;
    lds += size_t(cap) * 8;
    // the kernel holds the first S of the ell_emit(L, B) slots row_build wrote in registers
    // (entries past S come from the CSR through the LDS overflow)
    if (S > ell_emit(L, bt.B)) return hipErrorInvalidValue;
    auto fn = cg_ell_kernel<NT, R, S, TB, MODE>;
    allow_full_lds(reinterpret_cast<const void*>(fn));
    launch_k(fn, dim3(L.C, bt.B), NT, lds, s,
        L.m, L.C, L.base, L.at<int32_t>(ws, L.row_start), L.at<int32_t>(ws, L.row_len),
        L.at<int32_t>(ws, L.ucnt), L.at<int32_t>(ws, L.col), L.at<float>(ws, L.w),
        L.at<float>(ws, L.diag), b, out64, out32, rtol, max_iter, int(cap), st_nonconv, st_iters,
        L.at<int4>(ws, L.ell), bt.ws, bs, bt.u, bt.st);
    return launch_status("solve.hip:run_ell");
}

template <int NT, int R, int RV, typename TB>
static hipError_t run_vr(const Layout& L, const Batch& bt, void* ws, const TB* b, size_t bs,
                         double* out64, float* out32, float rtol, int max_iter,
                         int32_t* st_nonconv, int32_t* st_iters, hipStream_t s) {
    if (L.m > NT * R || L.RV != RV || L.VRM <= 0 || L.VRM > 63) {   // row_build's packing
        (void)hipGetLastError();
        return hipErrorInvalidValue;
    }
    const size_t mp4 = size_t((L.m + 3) & ~3);
    const size_t lds = 128 * 4 + mp4 * 4 + (size_t(NT) * RV + 4 * mp4) * 4 +
                       size_t(NT) * RV * 4 + mp4 * 4;
    auto fn = cg_vr_kernel<NT, R, RV, TB>;
    allow_full_lds(reinterpret_cast<const void*>(fn));
    launch_k(fn, dim3(L.C, bt.B), NT, lds, s,
        L.m, L.C, L.base, L.VRM, L.at<int32_t>(ws, L.row_start), L.at<int32_t>(ws, L.row_len),
        L.at<int32_t>(ws, L.ucnt), L.at<int32_t>(ws, L.col), L.at<float>(ws, L.w),
        L.at<float>(ws, L.diag), L.at<char>(ws, L.vr), b, out64, out32, rtol, max_iter,
        st_nonconv, st_iters, bt.ws, bs, bt.u, bt.st);
    return launch_status("solve.hip:run_vr");
}

template <int NT, typename TB>
static hipError_t run_lds(const Layout& L, const Batch& bt, void* ws, const TB* b, size_t bs,
                          double* out64, float* out32, float rtol, int max_iter,
                          int32_t* st_nonconv, int32_t* st_iters, hipStream_t s) {
    const int vec_lds = cg_vec_in_lds(L.m) ? 1 : 0;
    const size_t lds = 64 * 4 + (vec_lds ? size_t(5) * L.m * sizeof(float) : 0);
    auto fn = cg_lds_kernel<NT, TB>;
    allow_full_lds(reinterpret_cast<const void*>(fn));
    launch_k(fn, dim3(L.C, bt.B), NT, lds, s,
        L.m, L.C, L.base, L.at<int32_t>(ws, L.row_start), L.at<int32_t>(ws, L.row_len),
        L.at<int32_t>(ws, L.ucnt), L.at<int32_t>(ws, L.col), L.at<float>(ws, L.w),
        L.at<float>(ws, L.diag), b, out64, out32, rtol, max_iter, L.at<float>(ws, L.cgv),
        vec_lds, st_nonconv, st_iters, bt.ws, bs, bt.u, bt.st);
    return launch_status("solve.hip:run_lds");
}

// --------------------------------------------------------------------------------------
// The instantiated per-column variants.  One list: a row is a table row AND the instantiation of
// its kernel for both right-hand-side types, so neither exists without the other.  It is every
// variant cg_route (cg_route.h) can return and nothing else (tests/test_lib_cpu.py sweeps
// gll_cg_route over it).  ELL(NT, R, S, MODE), VR(NT, R, RV), LDS(NT).
// --------------------------------------------------------------------------------------
#define GLL_CG_VARIANTS(ELL, VR, LDS)                                                            \
    ELL(64, 1, 24, 3) ELL(128, 1, 24, 3) ELL(256, 1, 24, 3) ELL(512, 1, 24, 3) ELL(256, 2, 24, 1) \
    ELL(1024, 1, 16, 3) ELL(1024, 2, 16, 1) ELL(1024, 4, 4, 1)                                   \
    VR(512, 1, 4) VR(512, 1, 8) VR(512, 1, 10) VR(512, 2, 4) VR(512, 2, 8) VR(512, 2, 10)        \
    VR(512, 3, 4) VR(512, 3, 8) VR(512, 3, 10) VR(512, 4, 4) VR(512, 4, 8) VR(512, 4, 10)        \
    LDS(1024)

template <typename TB>
using CgRunFn = hipError_t (*)(const Layout&, const Batch&, void*, const TB*, size_t, double*,
                               float*, float, int, int32_t*, int32_t*, hipStream_t);
struct CgRow {
    CgRoute v;
    CgRunFn<float> f32;
    CgRunFn<double> f64;
};
#define GLL_CG_ELL_ROW(NT, R, S, MODE) \
    {{kCgEll, NT, R, S, MODE, 0, 0}, run_ell<NT, R, S, float, MODE>, run_ell<NT, R, S, double, MODE>},
#define GLL_CG_VR_ROW(NT, R, RV) \
    {{kCgVr, NT, R, RV, 1, 0, 0}, run_vr<NT, R, RV, float>, run_vr<NT, R, RV, double>},
#define GLL_CG_LDS_ROW(NT) {{kCgLds, NT, 0, 0, 0, 0, 0}, run_lds<NT, float>, run_lds<NT, double>},
static const CgRow kCgTable[] = {GLL_CG_VARIANTS(GLL_CG_ELL_ROW, GLL_CG_VR_ROW, GLL_CG_LDS_ROW)};
#undef GLL_CG_ELL_ROW
#undef GLL_CG_VR_ROW
#undef GLL_CG_LDS_ROW
constexpr int kCgRows = int(sizeof(kCgTable) / sizeof(kCgTable[0]));

int cg_table_rows() { return kCgRows; }

int cg_table_index(const CgRoute& rt) {
    for (int q = 0; q < kCgRows; ++q)
        if (same_variant(kCgTable[q].v, rt)) return q;
    return -1;
}

// The whole-GPU launcher (gridcg.hip) first where the route says so; hipErrorNotSupported from it
// means no grid configuration holds the system, and the route's per-column variant runs (any m).
static hipError_t cg_dispatch(const Layout& L, const Batch& bt, void* ws, const void* b, size_t bs,
                              int b_dtype, double* out64, float* out32, float rtol, int max_iter,
                              int32_t* st_nonconv, int32_t* st_iters, int32_t* st_failed,
                              hipStream_t s) {
    const CgRoute rt = cg_route(L, bt);
    if (rt.grid_first) {
        const hipError_t e = launch_cg_grid_luu(L, ws, b, b_dtype, out64, out32, rtol, 0.f,
                                                max_iter, st_nonconv, st_iters, st_failed, s);
        if (e != hipErrorNotSupported) return e;
    }
    const int row = cg_table_index(rt);
    if (row < 0) {
        if (debug_log())
            fprintf(stderr, "gll: solve.hip:cg_dispatch: variant not instantiated (family %d NT %d "
                            "R %d S %d MODE %d)\n", rt.family, rt.NT, rt.R, rt.S, rt.MODE);
        return hipErrorInvalidValue;
    }
    return b_dtype == GLL_DT_F32
               ? kCgTable[row].f32(L, bt, ws, static_cast<const float*>(b), bs, out64, out32, rtol,
                                   max_iter, st_nonconv, st_iters, s)
               : kCgTable[row].f64(L, bt, ws, static_cast<const double*>(b), bs, out64, out32, rtol,
                                   max_iter, st_nonconv, st_iters, s);
}

hipError_t launch_cg_luu(const Layout& L, const Batch& bt, void* ws, const void* b,
                         size_t b_stride, int b_dtype, double* out64, float* out32, float rtol,
                         int max_iter, int32_t* st_nonconv, int32_t* st_iters,
                         int32_t* st_failed, hipStream_t s) {
    if (L.m <= 0) return hipSuccess;
    if (b_dtype != GLL_DT_F32 && b_dtype != GLL_DT_F64) return hipErrorInvalidValue;
    prof_begin(GLL_K_CG, s);
    const hipError_t e = cg_dispatch(L, bt, ws, b, b_stride, b_dtype, out64, out32, rtol, max_iter,
                                     st_nonconv, st_iters, st_failed, s);
    prof_end(GLL_K_CG, s);
    return e;
}

// --------------------------------------------------------------------------------------
// General SPD CSR (stable_conjgrad replacement, absolute tolerance like GLL.py:259)
// --------------------------------------------------------------------------------------
template <int NT>
__global__ __launch_bounds__(NT) void cg_csr_kernel(int m, int C, const int32_t* __restrict__ rp,
                                                    const int32_t* __restrict__ col,
                                                    const float* __restrict__ val,
                                                    const float* __restrict__ b,
                                                    float* __restrict__ x, float atol,
                                                    int max_iter, float* __restrict__ gvec,
                                                    int vec_in_lds, int32_t* __restrict__ iters,
                                                    int32_t* __restrict__ nonconv) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int c = bx<true>();
    const int tid = threadIdx.x;
    float* red = smem;
    float* vb = vec_in_lds ? smem + 64 : gvec + size_t(c) * 5 * m;
    float *X_ = vb, *R_ = vb + m, *P_ = vb + 2 * m, *A_ = vb + 3 * m, *M_ = vb + 4 * m;
    float rz = 0.f, rr0 = 0.f;
    for (int u = tid; u < m; u += NT) {
        float dg = 0.f;
        for (int e = rp[u]; e < rp[u + 1]; ++e)
            if (col[e] == u) dg += val[e];
        const float mi = dg > 0.f ? 1.f / dg : 0.f;
        const float bu = b[size_t(u) * C + c];
        X_[u] = 0.f;
        R_[u] = bu;
        M_[u] = mi;
        P_[u] = mi * bu;
        rz += bu * mi * bu;
        rr0 += bu * bu;
    }
    int phase = 0;
    __syncthreads();
    block_sum2<NT>(rz, rr0, red, phase);
    const float tol2 = atol * atol;
    int it = 0;
    bool conv = rr0 <= tol2;
    // (the same loop as cg_lds_kernel's but for the row product; written as one inlined function
    // over a row-product callable it changed both kernels' code, so it stays written out)
    while (!conv && it < max_iter) {
        ++it;
        float pap = 0.f, unused = 0.f;
        for (int u = tid; u < m; u += NT) {
            float acc = 0.f;
            for (int e = rp[u]; e < rp[u + 1]; ++e) acc += val[e] * P_[col[e]];
            A_[u] = acc;
            pap += P_[u] * acc;
        }
        block_sum2<NT>(pap, unused, red, phase);
        if (!(pap > 0.f)) break;
        const float alpha = rz / pap;
        float rr = 0.f, rzn = 0.f;
        for (int u = tid; u < m; u += NT) {
            X_[u] += alpha * P_[u];
            const float ru = R_[u] - alpha * A_[u];
            R_[u] = ru;
            rr += ru * ru;
            rzn += ru * M_[u] * ru;
        }
        block_sum2<NT>(rr, rzn, red, phase);
        if (rr <= tol2) {
            conv = true;
            break;
        }
        const float beta = rzn / rz;
        rz = rzn;
        for (int u = tid; u < m; u += NT) P_[u] = M_[u] * R_[u] + beta * P_[u];
        __syncthreads();
    }
    for (int u = tid; u < m; u += NT) x[size_t(u) * C + c] = X_[u];
    if (tid == 0) {
        if (iters) atomicMax(iters, it);
        if (!conv && nonconv) atomicAdd(nonconv, 1);
    }
}

hipError_t launch_cg_csr(int m, int C, const int32_t* row_ptr, const int32_t* col,
                         const float* val, const float* b, float* x, float atol, int max_iter,
                         int32_t* iters, int32_t* nonconv, float* gvec, hipStream_t s) {
    const size_t vec_bytes = size_t(5) * m * sizeof(float);
    const bool vec_lds = cg_vec_in_lds(m);
    if (!vec_lds && gvec == nullptr) return hipErrorInvalidValue;
    const size_t lds = 64 * 4 + (vec_lds ? vec_bytes : 0);
    auto fn = cg_csr_kernel<256>;
    allow_full_lds(reinterpret_cast<const void*>(fn));
    prof_begin(GLL_K_CG, s);
    launch_k(fn, C, 256, lds, s, m, C, row_ptr, col, val, b, x, atol, max_iter, gvec, vec_lds ? 1 : 0,
                           iters, nonconv);
    prof_end(GLL_K_CG, s);
    return launch_status("solve.hip:launch_cg_csr");
}

}  // namespace gll
