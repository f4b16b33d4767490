// cg_route.h -- which kernel solves the Luu systems of a problem.  cg_route computes a CgRoute
// from the problem and the batch alone; solve.hip keeps the table of the per-column variants it
// instantiates and cg_dispatch launches from that table, and gll_cg_route (api.hip) reports the
// route without a GPU, so the report cannot drift from the launch.  Host code without a HIP call.
#pragma once

#include "gll_internal.h"

namespace gll {

// The LDS of a CU and the dynamic share the CG kernels ask for (allow_full_lds); here because the
// route of cg_lds_kernel depends on it.
static constexpr size_t kLdsLimit = 160 * 1024;
static constexpr size_t kLdsDyn = kLdsLimit - 1024;   // dynamic share, room for static LDS

// The Luu solves of this problem try the whole-GPU CG first (gridcg.hip): single graphs past the
// per-column kernels' sweet spot (m > 2048), or forced by GLL_FLAG_CG_GRID.  Measured at stress
// (m 4096, K 30): 209 us against 288 us per solve, while at the FullySup shape (m 1250, K 25) the
// per-column kernel with 16 slots and the LDS overflow wins.  Batches keep the per-column kernels
// (B x C workgroups already fill the GPU).
inline bool grid_cg_route(const Layout& L, const Batch& bt) {
    return bt.B == 1 && L.C <= 16 && !(L.flags & GLL_FLAG_CG_PERCOL) &&
           (L.m > 2048 || (L.flags & GLL_FLAG_CG_GRID));
}

enum CgFamily {
    kCgEll = 0,   // cg_ell_kernel<NT, R, S, TB, MODE>
    kCgVr = 1,    // cg_vr_kernel<NT, R, RV, TB>
    kCgLds = 2,   // cg_lds_kernel<NT, TB>
};
struct CgRoute {
    int family;       // CgFamily
    int NT, R;        // threads per workgroup, rows per thread (cg_lds: 0, it strides over the rows)
    int S;            // cg_ell: register ELL slots per row; cg_vr: RV, virtual rows per thread
    int MODE;         // cg_ell: 3 Neumann-1, 1 Jacobi (both Chronopoulos-Gear); cg_vr 1; cg_lds 0,
                      // the classic two-reduction PCG (Jacobi)
    int vec_in_lds;   // cg_lds: the five vectors fit the dynamic LDS (else the workspace's cgv)
    int grid_first;   // the whole-GPU launcher is tried first; the fields above are what runs when
                      // no grid configuration holds the system
};
// Two routes run the same kernel (vec_in_lds is an argument of it, grid_first precedes it).
inline bool same_variant(const CgRoute& a, const CgRoute& b) {
    return a.family == b.family && a.NT == b.NT && a.R == b.R && a.S == b.S && a.MODE == b.MODE;
}

// cg_lds_kernel and cg_csr_kernel: the five vectors of a column (and 64 floats of reduction
// scratch) fit the dynamic LDS; else they live in global memory.
inline bool cg_vec_in_lds(int m) { return 64 * 4 + size_t(5) * m * sizeof(float) <= kLdsDyn; }

// Reads GLL_KNOB_VR_RV through the Layout (vr_threads).
inline CgRoute cg_route(const Layout& L, const Batch& bt) {
    const int m = L.m;
    const int gf = grid_cg_route(L, bt) ? 1 : 0;
    if (L.RV > 0)   // the balanced kernel (row_build packed its virtual rows): 512 rows a round
        return {kCgVr, kVrNT, m <= 512 ? 1 : (m <= 1024 ? 2 : (m <= 1536 ? 3 : 4)), L.RV, 1, 0, gf};
    // The Neumann form (MODE 3) wherever a thread owns one row; with two or more rows per thread
    // one SpMV per iteration (MODE 3 at 256 x 2 takes 220 VGPRs, two waves per SIMD instead of
    // three: B = 64 NS CG 21.8 -> 34.2 us, profiles/r03l_cg_neumann_ab.txt; at 1024 x 2 it
    // spilled 144 B per lane: FullySup single graph forced onto this kernel 174 -> 135 us per
    // solve with MODE 1, profiles/r04p_ab_ell2.txt).
    auto ell = [&](int nt, int r, int s) { return CgRoute{kCgEll, nt, r, s, r > 1 ? 1 : 3, 0, gf}; };
    if (m <= 64) return ell(64, 1, 24);
    if (m <= 128) return ell(128, 1, 24);
    if (m <= 256) return ell(256, 1, 24);
    // m <= 512: one row per thread is the lower latency for a single graph; batches run more
    // workgroups per CU with 4 waves x 2 rows (B = 64: 44.7 -> 36.6 us per launch).  Batches of
    // at most one column workgroup per CU (B x C <= 256) run the single-graph geometry, 512 x 1
    // with the Neumann form: NS B = 8 18.6 -> 15.9 us per launch; with more workgroups than CUs
    // 256 x 2 (MODE 1) keeps the lead: B = 64 21.9 against 28.2 us
    // (profiles/r03t_cg_batched_geometry_ab.txt).  Round 4 swept nine batched geometries (128 /
    // 256 / 512 threads x 4 / 2 / 1 rows, 8-24 register ELL slots, MODE 1 and 3) at B = 64:
    // none beat 256 x 2 x 24 MODE 1 (21.9 us; the best Neumann form 28.2 us,
    // profiles/r04c_ab_geom.txt), and the variants were removed.  (Column pairs -- two right-hand
    // sides per workgroup -- measured slower at B = 64 and 8 and were removed in round 4:
    // profiles/r03s_cg_pairs_ab.txt.)
    if (m <= 512 && (bt.B == 1 || int64_t(bt.B) * L.C <= 256)) return ell(512, 1, 24);
    if (m <= 512) return ell(256, 2, 24);
    if (m <= 1024) return ell(1024, 1, 16);
    if (m <= 2048) return ell(1024, 2, 16);
    if (m <= 4096) return ell(1024, 4, 4);
    return {kCgLds, 1024, 0, 0, 0, cg_vec_in_lds(m) ? 1 : 0, gf};
}

// Rows of solve.hip's table of instantiated per-column variants, and the row of a route: -1 when
// the variant is not instantiated (cg_dispatch then fails).
int cg_table_rows();
int cg_table_index(const CgRoute& rt);

}  // namespace gll
