// knn_route.h -- what the kNN units (gram.hip, select.hip, order.hip) agree on: the route
// predicates both launchers and the workspace layout depend on, the select's variant and the
// function that picks it, and the few device declarations more than one of them needs.  The
// routing is host code without a HIP call: gll_select_route (api.hip) runs it without a GPU.
#pragma once

#include "gll_internal.h"

namespace gll {

typedef _Float16 h16x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) void lds_void;

// XCD-aware tile order: blocks are dealt round-robin over the 8 XCDs (block b runs on XCD
// b % 8), so block b takes tile (b % 8) * ceil-share + b / 8: each XCD
// works through a contiguous run of the row-major upper-triangle tile list -- a band of row
// blocks bi whose rows stay in that XCD's L2 -- instead of every XCD touching every row.
// (Measured neutral at NS, B = 64 and stress, tools/ab_flags.py: the tile loads are bound by
// per-CU issue, not by L2 misses.)  The select deals the positions of a locality order the
// same way.
__device__ __forceinline__ int xcd_tile(int b, int nt) {
    const int x = b & 7, q = b >> 3;
    const int per = nt >> 3, extra = nt & 7;   // the first `extra` XCDs take one tile more
    return x * per + (x < extra ? x : extra) + q;
}

constexpr int kPK = 64;    // features per k-stage of the 128-tile pre-split GEMM (gram_pk_kernel)
constexpr int kPK2 = 32;   // features per k-stage of the 256-tile kernel (gram_pk2_kernel)

// 256-tiles (gram_pk2_kernel) or 128-tiles (gram_pk_kernel) for the pre-split GEMM: the one
// with fewer waves of one-workgroup-per-CU rounds x k-stage bytes (a round of 256-tiles moves
// the same 64 KiB per stage as one of 128-tiles but does 4x the work, in twice the stages).
// The knob GLL_KNOB_GRAM_TILE = 128 / 256 forces one (tests).
inline bool gram_tile256(const Layout& L, const Batch& bt, int T, int T2, int cus) {
    if (knob(GLL_KNOB_GRAM_TILE) > 0) return knob(GLL_KNOB_GRAM_TILE) == 256 && L.dp % kPK2 == 0;
    // (d <= 128: a tile is 4 k-stages; the FullySup shape measured 225 -> 230 us at B = 64)
    if (L.dp % kPK2 || L.dp <= 128) return false;
    const int64_t t1 = int64_t(bt.B) * T * (T + 1) / 2, t2 = int64_t(bt.B) * T2 * (T2 + 1) / 2;
    const int64_t r1 = (t1 + cus - 1) / cus, r2 = (t2 + cus - 1) / cus;
    return r2 * 2 * (L.dp / kPK2) * kPK2 < r1 * (L.dp / kPK) * kPK;   // stage bytes equal
}

// The pre-split route (gram_split + gram_pk / gram_pk2): batches, and single graphs with d > 128
// and n <= 12,288 (see gram.hip launch_gram).  Its D2 is stored fp16 (dput) unless
// GLL_FLAG_D2_F32 (A/B).
inline bool presplit_route(const Layout& L, const Batch& bt) {
    const int T = (L.n + 127) / 128;
    return int64_t(bt.B) * T * (T + 1) / 2 >= 256 &&
           !(L.flags & GLL_FLAG_GRAM_INLINE) && (bt.B > 1 || (L.d > 128 && L.n <= 12288)) &&
           gram_planes(L, bt.B) == 1 && L.PR == L.n;
}
// Batches only (single graphs measured slower with it: at stress the wider candidate margin
// cost the select 274 -> 299 us; DESIGN.md §3.1, profiles/r03x_d2_fp16_ab.txt).
// (Not for the wide select, K - 1 > kMaxKm1: it reads fp32 rows.)
inline bool d2_half(const Layout& L, const Batch& bt) {
    return !(L.flags & GLL_FLAG_D2_F32) && bt.B > 1 && presplit_route(L, bt) &&
           L.K - 1 <= kMaxKm1;
}

// ---------------------------------------------------------------------------------------
// The Gram's route: which kernels of gram.hip a graph build launches.  gram_route computes it
// from the problem and the CU count alone; launch_gram and launch_gram_panel launch from it, and
// gll_gram_route (api.hip) reports it without a GPU, so the report cannot drift from the launch.
// ---------------------------------------------------------------------------------------
constexpr int kHP = 128;   // features of the half tile (gram_bf3h_kernel)
enum GramFamily {
    kGramBf3 = 0,    // gram_bf3_kernel<VEC>: 64-tiles, phases of 256 features
    kGramBf3h = 1,   // gram_bf3h_kernel<VEC>: the half tile, d <= kHP
    kGramBf3s = 2,   // gram_bf3s_kernel<VEC>: split-phase, two planes
    kGramBf3w = 3,   // gram_bf3w_kernel<VEC>: inline-split 128-tiles (and every row panel)
    kGramPk = 4,     // gram_split_kernel<VEC> + gram_pk_kernel<H, 128>
    kGramPk2 = 5,    // gram_split_kernel<VEC> + gram_pk2_kernel<H> (+ a tail of gram_pk_kernel)
};
struct GramRoute {
    int family;     // GramFamily
    int vec;        // VEC of the inline-split kernel or of gram_split_kernel
    int planes;     // D2 planes written (gram_planes)
    int presplit;   // gram_split_kernel runs first (xhi / xlo / xnrm are written)
    int H;          // D2 stored as fp16 x s (d2_half)
    int t256;       // 256-tiles (gram_pk2_kernel)
    int tail;       // 256-tiles of the last round that run as subtiles on gram_pk_kernel<H, TS>
    int sub;        // subtiles per such tile: 16 (TS = 64) or 4 (TS = 128); 0 without a tail
    int panels;     // row panels (launch_gram_panel once per panel); 0: the whole matrix
};
inline GramRoute gram_route(const Layout& L, const Batch& bt, bool vec, int cus) {
    GramRoute r{};
    r.vec = vec;
    r.planes = gram_planes(L, bt.B);
    if (L.PR < L.n) {   // row panels: rectangular tiles on the inline-split 128-tile kernel
        r.family = kGramBf3w;
        r.panels = (L.n + L.PR - 1) / L.PR;
        return r;
    }
    if (r.planes == 2) {
        r.family = kGramBf3s;
        return r;
    }
    // 128-tiles when there are enough of them to fill the chip twice (large graphs and batches;
    // a single NS graph has only 36); 64-tiles otherwise
    const int T = (L.n + 127) / 128;
    if (presplit_route(L, bt)) {
        const int T2 = (L.n + 255) / 256;
        r.presplit = 1;
        r.H = d2_half(L, bt);
        r.t256 = gram_tile256(L, bt, T, T2, cus);
        r.family = r.t256 ? kGramPk2 : kGramPk;
        // one 256-tile per CU at a time: a last round short of a full one (stress: 528 tiles, 16
        // in the third round, profiles/r04b_stress_kernel_stats.csv) runs as subtiles of those
        // tiles instead (gram_pk_kernel's D2 is bitwise the 256-tile kernel's), where they fit
        // one round.  Round 6: 64-row subtiles (16 per tile, two workgroups per CU at 64 KiB of
        // LDS) where they fit: stress 256 of them, one per CU, 18.8 us where 64 128-subtiles on a
        // quarter of the chip took 31.4 (profiles/r06i_ab_gram_tail.txt); otherwise 128-subtiles
        // (4 per tile).  More than one round of subtiles loses to a last round of 256-tiles: B =
        // 64 NS, 128 tail tiles, 2,048 64-subtiles 58 us against ~35 for the round, and two rounds
        // of 128-subtiles 224 -> 235 us (round 5).  GLL_KNOB_GRAM_TAIL: 1 no tail, 2 128-subtiles.
        const int64_t nt2 = int64_t(bt.B) * T2 * (T2 + 1) / 2;
        const int tk = knob(GLL_KNOB_GRAM_TAIL);
        int64_t tail = r.t256 && nt2 > cus ? nt2 % cus : 0;
        const int sub = (tk != 2 && tail * 16 <= 2 * int64_t(cus)) ? 16 : 4;   // subtiles per tile
        if ((sub == 4 && tail * 4 > cus) || tk == 1) tail = 0;
        // (Measured and dropped: the subtiles split further over 4 k-slices summed by a reduce
        // kernel, 256 workgroups instead of 64: 250 -> 260 us, profiles/r04u_ab_tail.txt.)
        r.tail = int(tail);
        r.sub = tail > 0 ? sub : 0;
        return r;
    }
    if (int64_t(bt.B) * T * (T + 1) / 2 >= 512) r.family = kGramBf3w;
    else r.family = L.d <= kHP ? kGramBf3h : kGramBf3;   // (profiles/r06v_ab_*.txt)
    return r;
}

// ---------------------------------------------------------------------------------------
// The select's variant: the template arguments of the kernel a launch runs.  select_route
// computes it from the problem; select.hip keeps the table of the variants it instantiates,
// and a launch is a lookup in that table.
// ---------------------------------------------------------------------------------------
struct SelVariant {       // knn_select_kernel<KC, V, NP, PG, NU, XQ, R, CH, H>
    int KC;   // candidate list capacity: 16, 32 or 64
    int V;    // 16-B feature loads (aligned X, d % 4 == 0)
    int NP;   // D2 planes the scan sums (gram_planes)
    int PG;   // candidate groups per exact-distance sweep: 2 latency form, 1 occupancy form
    int NU;   // 32-feature steps per exact-distance load batch
    int XQ;   // quarters of 256 features of x_i staged in LDS (0: from global)
    int R;    // blocks numbered XCD-contiguously over the batch (batch_xy<true>)
    int CH;   // 1024-column chunks of the D2 row the scan holds in registers (0: re-read)
    int H;    // D2 rows stored as fp16 x s (d2_half)
};
struct SelWideVariant {   // knn_select_wide_kernel<V, NP, CAP, KMX, TOP>
    int V, NP;
    int CAP;  // candidate slots per wave
    int KMX;  // capacity of the sorted list (K - 1 at most)
    int TOP;  // per-lane list length of the threshold scan
};
struct SelRoute {
    bool wide;   // K - 1 > kMaxKm1: knn_select_wide_kernel (w), else knn_select_kernel (v)
    SelVariant v;
    SelWideVariant w;
};
inline bool operator==(const SelVariant& a, const SelVariant& b) {
    return a.KC == b.KC && a.V == b.V && a.NP == b.NP && a.PG == b.PG && a.NU == b.NU &&
           a.XQ == b.XQ && a.R == b.R && a.CH == b.CH && a.H == b.H;
}
inline bool operator==(const SelWideVariant& a, const SelWideVariant& b) {
    return a.V == b.V && a.NP == b.NP && a.CAP == b.CAP && a.KMX == b.KMX && a.TOP == b.TOP;
}

// The variant of a select over rows r0 .. r0 + rows - 1 (a panel, or all n) of each of bt.B
// graphs; vec: X is 16-B aligned and d % 4 == 0.  Reads GLL_KNOB_SEL_FORM.
inline SelRoute select_route(const Layout& L, const Batch& bt, bool vec, int r0, int rows) {
    (void)r0;   // a panel's position changes the row order (perm), not the kernel
    const int n = L.n, K = L.K;
    const int planes = gram_planes(L, bt.B);
    SelRoute rt{};
    if (K - 1 > kMaxKm1) {   // k past one candidate per lane: LDS lists
        rt.wide = true;
        rt.w = K - 1 > kMaxKm1Wide ? SelWideVariant{vec, planes, 512, kMaxKm1Huge, 5}
                                   : SelWideVariant{vec, planes, 256, kMaxKm1Wide, 4};
        return rt;
    }
    SelVariant& v = rt.v;
    // candidate list capacity: smallest of {16, 32, 64} leaving a re-rank margin >= 4
    const int need = K - 1 + 4;
    v.KC = need <= 16 ? 16 : (need <= 32 ? 32 : 64);
    v.V = vec;
    v.NP = planes;
    v.H = planes == 1 && d2_half(L, bt);   // the Gram stored D2 as fp16 x s
    // the latency form (PG = 2 candidate groups in flight, NU = 16, ~200 VGPRs: 2 waves per SIMD)
    // for a single graph whose rows fill at most one such round of the chip; larger graphs (and
    // batches) run the occupancy form.  Stress (n = 8,192): 2,048 workgroups, four rounds of the
    // latency form (profiles/r04c_trace_stress.txt: the last workgroup starts at +200 of
    // 255 us).  GLL_KNOB_SEL_FORM 1 / 2 forces either (tests, A/B).
    const int form = knob(GLL_KNOB_SEL_FORM);
    const bool lat = bt.B == 1 && (form == 1 || (form == 0 && rows <= 2048));
    // Batched launches (PG = 1) stage x_i in LDS (XQ quarters of 256 features, d <= 1024): round 2
    // measured B = 64 NS select 259 -> 214 us at 6 waves per SIMD (XQ = 2, NU = 8; the NU = 16
    // batch of loads held 120 VGPRs, 4 waves).  Round 4 (x_i by LDS-DMA, no registers held for
    // it): NU = 4 at 8 waves per SIMD, B = 64 NS 183 -> 174 us, FullySup B = 64 349 -> 339, stress
    // 169 -> 168 (profiles/r04q_ab_sel.txt).  NU: 32-feature steps per exact-distance load batch
    // (16 for the latency form, whose two waves per SIMD have registers to spare); the loads of
    // steps past d are clamped to row 0 and masked.
    // The d ladder: {latency NU, occupancy NU, XQ} of each rung.
    int nus = 16, nub = 16, xq = 0;                                  // two planes, or d > 1024
    if (planes == 1 && L.d <= 128) nus = 4, nub = 4, xq = 1;
    else if (planes == 1 && L.d <= 256) nus = 16, nub = 4, xq = 1;
    else if (planes == 1 && L.d <= 512) nus = 16, nub = 4, xq = 2;
    else if (planes == 1 && L.d <= 1024) nus = 16, nub = 4, xq = 4;
    // Batched launches number blocks XCD-contiguously (R: each XCD works through a run of
    // graphs): NS B = 64 220 -> 213 us, FullySup B = 64 440 -> 429 us (profiles/r02h_xcd_ab.txt),
    // once the kernel took its graph index once instead of per pointer.  The occupancy form
    // always carries R; for a single graph the numbering is the identity.
    v.PG = lat ? 2 : 1;
    v.NU = lat ? nus : nub;
    v.XQ = lat || !vec ? 0 : xq;
    v.R = lat ? 0 : 1;
    // the threshold scan holds rows of <= 2048 columns in registers (KC <= 32, aligned d)
    v.CH = (v.KC <= 32 && vec && rows == n) ? (n <= 1024 ? 1 : (n <= 2048 ? 2 : 0)) : 0;
    return rt;
}

// Rows of select.hip's table of instantiated variants (narrow rows, then wide rows), and the
// row of a route: -1 when the variant is not instantiated (launch_select then fails).
int select_table_rows();
int select_table_index(const SelRoute& rt);

}  // namespace gll
