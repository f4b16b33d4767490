// features.hip -- the layer's front end: feature rows of any supported element type into the fp32
// rows the graph build reads, optionally normalised to unit length, and the way back.
//
// Every network of the reference ends in F.normalize(feat, dim=1) (networks/BuildNet.py:101,
// preact_resnet.py:101, customCNN.py:36, train_and_adversarial.py:420), so the layer always
// receives unit-norm rows; GLL.py:24 leaves the normalisation to the caller.  Two streaming
// kernels, each templated on the element type of Z (fp32, fp16, bf16), one wave per row:
//
//   unit_rows_kernel   a_k = float(z_k) (exact).  Flags 0: X = a.  GLL_UF_NORMALIZE:
//                      s = sum_k a_k^2, r = 1 / max(sqrtf(s), 1e-12f) (F.normalize's clamp; no
//                      rescaling against overflow of s, as torch has none), X = a r, rnorm = r.
//   unit_grad_kernel   fp32 gX (dloss/dX), X, rnorm -> gZ in Z's type.  GLL_UF_NORMALIZE:
//                      t = sum_k X_k gX_k, out_k = r (gX_k - X_k t); a clamped row (r >= 1e12f)
//                      takes out_k = r gX_k, the backward of torch's clamp_min.  Flags 0:
//                      out = gX.  out is rounded once (to nearest even; an fp16 overflow gives
//                      inf) to Z's type.
//
// Lane l holds, in step s, the E = 16 B / sizeof(element) consecutive elements
// (64 s + l) E .. + E - 1 of its row: one 16-B load where the row starts are 16-B aligned, E scalar
// loads of the same elements otherwise (odd d with half types, d % 4 != 0 with fp32).  The row stays
// in registers between the sum and the scale (d <= 4096: at most 64 floats a lane), so every input
// element is read from global memory once and LDS is not used.  A lane sums its elements in
// ascending order with fmaf and wave_sum_dpp combines the 64 partials in a fixed tree; elements
// past d add +0.  The order therefore depends on d and the element type alone -- not on rows, the
// grid, the row's place in the launch, or which of the two load forms ran -- so a batch's rows
// are bitwise the single call's.  No atomics; rows past `rows` and bytes outside the outputs are
// never written.
#include <atomic>

#include "gll_internal.h"

namespace gll {

struct bf16_t {   // storage only: the kernels widen and round by hand
    uint16_t bits;
};
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

constexpr int kUnitThreads = 256;                       // 4 waves = 4 rows a workgroup
constexpr int kUnitRowsPerWg = kUnitThreads / kWave;
constexpr int64_t kUnitMaxWg = int64_t(1) << 22;        // workgroups a launch (2^30 threads)

__device__ __forceinline__ float widen(float v) { return v; }
__device__ __forceinline__ float widen(_Float16 v) { return static_cast<float>(v); }
__device__ __forceinline__ float widen(bf16_t v) {
    return __builtin_bit_cast(float, uint32_t(v.bits) << 16);
}

template <typename T>
__device__ __forceinline__ T narrow(float v);
template <>
__device__ __forceinline__ float narrow<float>(float v) { return v; }
template <>
__device__ __forceinline__ _Float16 narrow<_Float16>(float v) { return static_cast<_Float16>(v); }
template <>
__device__ __forceinline__ bf16_t narrow<bf16_t>(float v) {   // round to nearest even
    const uint32_t b = __builtin_bit_cast(uint32_t, v);
    if (v != v) return bf16_t{uint16_t(0x7FC0)};
    return bf16_t{uint16_t((b + 0x7FFFu + ((b >> 16) & 1u)) >> 16)};
}

// The E elements p[k .. k + E - 1] of a row of d (zeros past d).  VEC: one 16-B load (d % E == 0
// and 16-B aligned rows, so k < d covers all E).  Branch-free like load4: a lane past the row
// loads p[0 ..] and selects zero.
template <typename T, bool VEC>
__device__ __forceinline__ void load_elems(const T* __restrict__ p, int k, int d,
                                           float (&a)[16 / sizeof(T)]) {
    constexpr int E = 16 / sizeof(T);
    if constexpr (VEC) {
        const bool in = k < d;
        const u32x4 v = *reinterpret_cast<const u32x4*>(p + (in ? k : 0));
        T e[E];
        __builtin_memcpy(e, &v, 16);
#pragma unroll
        for (int j = 0; j < E; ++j) a[j] = in ? widen(e[j]) : 0.f;
    } else {
#pragma unroll
        for (int j = 0; j < E; ++j) {
            const T e = p[k + j < d ? k + j : 0];
            a[j] = k + j < d ? widen(e) : 0.f;
        }
    }
}

template <typename T, bool VEC>
__device__ __forceinline__ void store_elems(T* __restrict__ p, int k, int d,
                                            const float (&a)[16 / sizeof(T)]) {
    constexpr int E = 16 / sizeof(T);
    if constexpr (VEC) {
        if (k < d) {
            T e[E];
#pragma unroll
            for (int j = 0; j < E; ++j) e[j] = narrow<T>(a[j]);
            u32x4 v;
            __builtin_memcpy(&v, e, 16);
            *reinterpret_cast<u32x4*>(p + k) = v;
        }
    } else {
#pragma unroll
        for (int j = 0; j < E; ++j)
            if (k + j < d) p[k + j] = narrow<T>(a[j]);
    }
}

// fp32 rows read or written E elements at a time beside a row of T (E = 8 for the half types:
// two 16-B accesses).  VEC needs d % E == 0, which makes the fp32 rows 16-B aligned as well.
template <int E, bool VEC>
__device__ __forceinline__ void load_f32(const float* __restrict__ p, int k, int d, float (&a)[E]) {
#pragma unroll
    for (int h = 0; h < E / 4; ++h) {
        float q[4];
        load_elems<float, VEC>(p, k + 4 * h, d, q);
#pragma unroll
        for (int j = 0; j < 4; ++j) a[4 * h + j] = q[j];
    }
}
template <int E, bool VEC>
__device__ __forceinline__ void store_f32(float* __restrict__ p, int k, int d, const float (&a)[E]) {
#pragma unroll
    for (int h = 0; h < E / 4; ++h) {
        float q[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) q[j] = a[4 * h + j];
        store_elems<float, VEC>(p, k + 4 * h, d, q);
    }
}

// Rows row0 .. rows - 1, one wave each; 64 E STEPS >= d.
template <typename T, int STEPS, bool VEC>
__global__ __launch_bounds__(kUnitThreads) void unit_rows_kernel(const T* __restrict__ Z,
                                                                 float* __restrict__ X,
                                                                 float* __restrict__ rnorm,
                                                                 int d, int normalize,
                                                                 int64_t row0, int64_t rows) {
    constexpr int E = 16 / sizeof(T);
    const int64_t row = row0 + int64_t(blockIdx.x) * kUnitRowsPerWg + threadIdx.x / kWave;
    if (row >= rows) return;   // wave-uniform
    const int l = lane_id();
    const T* z = Z + size_t(row) * d;
    float* x = X + size_t(row) * d;
    float a[STEPS][E];
#pragma unroll
    for (int s = 0; s < STEPS; ++s) load_elems<T, VEC>(z, (s * kWave + l) * E, d, a[s]);
    float r = 1.f;
    if (normalize) {   // launch-uniform
        float acc = 0.f;
#pragma unroll
        for (int s = 0; s < STEPS; ++s)
#pragma unroll
            for (int j = 0; j < E; ++j) acc = fmaf(a[s][j], a[s][j], acc);
        const float nrm = sqrtf(wave_sum_dpp(acc));
        r = 1.f / (nrm < 1e-12f ? 1e-12f : nrm);   // a NaN norm stays NaN, as clamp_min keeps it
        if (l == 0) rnorm[row] = r;
#pragma unroll
        for (int s = 0; s < STEPS; ++s)
#pragma unroll
            for (int j = 0; j < E; ++j) a[s][j] *= r;
    }
#pragma unroll
    for (int s = 0; s < STEPS; ++s) store_f32<E, VEC>(x, (s * kWave + l) * E, d, a[s]);
}

template <typename T, int STEPS, bool VEC>
__global__ __launch_bounds__(kUnitThreads) void unit_grad_kernel(const float* __restrict__ gX,
                                                                 const float* __restrict__ X,
                                                                 const float* __restrict__ rnorm,
                                                                 T* __restrict__ gZ, int d,
                                                                 int normalize, int64_t row0,
                                                                 int64_t rows) {
    constexpr int E = 16 / sizeof(T);
    const int64_t row = row0 + int64_t(blockIdx.x) * kUnitRowsPerWg + threadIdx.x / kWave;
    if (row >= rows) return;   // wave-uniform
    const int l = lane_id();
    const float* g = gX + size_t(row) * d;
    T* gz = gZ + size_t(row) * d;
    float o[STEPS][E];
#pragma unroll
    for (int s = 0; s < STEPS; ++s) load_f32<E, VEC>(g, (s * kWave + l) * E, d, o[s]);
    if (normalize) {   // launch-uniform
        const float* x = X + size_t(row) * d;
        float xv[STEPS][E];
#pragma unroll
        for (int s = 0; s < STEPS; ++s) load_f32<E, VEC>(x, (s * kWave + l) * E, d, xv[s]);
        const float r = rnorm[row];
        float acc = 0.f;
#pragma unroll
        for (int s = 0; s < STEPS; ++s)
#pragma unroll
            for (int j = 0; j < E; ++j) acc = fmaf(xv[s][j], o[s][j], acc);
        // a clamped row (|z| < 1e-12) is z * 1e12: no projection, as clamp_min's backward
        const float t = r >= 1e12f ? 0.f : wave_sum_dpp(acc);
#pragma unroll
        for (int s = 0; s < STEPS; ++s)
#pragma unroll
            for (int j = 0; j < E; ++j) o[s][j] = r * fmaf(-xv[s][j], t, o[s][j]);
    }
#pragma unroll
    for (int s = 0; s < STEPS; ++s) store_elems<T, VEC>(gz, (s * kWave + l) * E, d, o[s]);
}

static std::atomic<int64_t> g_unit_calls{0};

int64_t features_calls() { return g_unit_calls.load(std::memory_order_relaxed); }

static bool aligned16(const void* p) { return reinterpret_cast<uintptr_t>(p) % 16 == 0; }

// Launch `fn` over all rows: a launch holds at most kUnitMaxWg workgroups, more rows take several.
template <typename F, typename... Args>
static hipError_t unit_launch(const char* what, F fn, int64_t rows, hipStream_t s, Args... args) {
    const int64_t per = kUnitMaxWg * kUnitRowsPerWg;
    for (int64_t row0 = 0; row0 < rows; row0 += per) {
        const int64_t cnt = rows - row0 < per ? rows - row0 : per;
        const unsigned wgs = unsigned((cnt + kUnitRowsPerWg - 1) / kUnitRowsPerWg);
        launch_k(fn, dim3(wgs), dim3(kUnitThreads), 0, s, args..., row0, rows);
        g_unit_calls.fetch_add(1, std::memory_order_relaxed);
        const hipError_t e = launch_status(what);
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}


// 64 E STEPS >= d with STEPS a power of two (d <= 4096: at most 16 steps of fp32, 8 of a half type)
template <typename T, int STEPS>
static hipError_t rows_steps(int64_t rows, int d, const T* Z, int normalize, float* X, float* rnorm,
                             hipStream_t s) {
    constexpr int E = 16 / sizeof(T);
    if constexpr (STEPS * kWave * E > 4096) {
        return hipErrorInvalidValue;
    } else {
        if (d > STEPS * kWave * E) return rows_steps<T, STEPS * 2>(rows, d, Z, normalize, X, rnorm, s);
        if (d % E == 0 && aligned16(Z) && aligned16(X))
            return unit_launch("features.hip:unit_rows_kernel", unit_rows_kernel<T, STEPS, true>,
                               rows, s, Z, X, rnorm, d, normalize);
        return unit_launch("features.hip:unit_rows_kernel", unit_rows_kernel<T, STEPS, false>, rows,
                           s, Z, X, rnorm, d, normalize);
    }
}

template <typename T, int STEPS>
static hipError_t grad_steps(int64_t rows, int d, const float* gX, const float* X,
                             const float* rnorm, int normalize, T* gZ, hipStream_t s) {
    constexpr int E = 16 / sizeof(T);
    if constexpr (STEPS * kWave * E > 4096) {
        return hipErrorInvalidValue;
    } else {
        if (d > STEPS * kWave * E)
            return grad_steps<T, STEPS * 2>(rows, d, gX, X, rnorm, normalize, gZ, s);
        if (d % E == 0 && aligned16(gX) && aligned16(gZ) && (!normalize || aligned16(X)))
            return unit_launch("features.hip:unit_grad_kernel", unit_grad_kernel<T, STEPS, true>,
                               rows, s, gX, X, rnorm, gZ, d, normalize);
        return unit_launch("features.hip:unit_grad_kernel", unit_grad_kernel<T, STEPS, false>, rows,
                           s, gX, X, rnorm, gZ, d, normalize);
    }
}

hipError_t launch_unit_rows(int64_t rows, int d, const void* Z, int z_dtype, int flags, float* X,
                            float* rnorm, hipStream_t s) {
    const int nz = (flags & GLL_UF_NORMALIZE) != 0;
    switch (z_dtype) {
        case GLL_XT_F32:
            return rows_steps<float, 1>(rows, d, static_cast<const float*>(Z), nz, X, rnorm, s);
        case GLL_XT_F16:
            return rows_steps<_Float16, 1>(rows, d, static_cast<const _Float16*>(Z), nz, X, rnorm, s);
        default:
            return rows_steps<bf16_t, 1>(rows, d, static_cast<const bf16_t*>(Z), nz, X, rnorm, s);
    }
}

hipError_t launch_unit_grad(int64_t rows, int d, const float* gX, const float* X,
                            const float* rnorm, int flags, void* gZ, int z_dtype, hipStream_t s) {
    const int nz = (flags & GLL_UF_NORMALIZE) != 0;
    switch (z_dtype) {
        case GLL_XT_F32:
            return grad_steps<float, 1>(rows, d, gX, X, rnorm, nz, static_cast<float*>(gZ), s);
        case GLL_XT_F16:
            return grad_steps<_Float16, 1>(rows, d, gX, X, rnorm, nz, static_cast<_Float16*>(gZ), s);
        default:
            return grad_steps<bf16_t, 1>(rows, d, gX, X, rnorm, nz, static_cast<bf16_t*>(gZ), s);
    }
}

}  // namespace gll
