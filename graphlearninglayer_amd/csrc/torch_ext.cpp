// torch_ext.cpp -- LaplaceLearningSparseHard.apply as native code over the C ABI of include/gll.h.
//
// The reference's LaplaceLearningSparseHard is a Python torch.autograd.Function
// (/root/reference/GLL.py:10-177).  At ~10^4 calls/s the host side of a call is on the step's
// critical path, so everything `apply` does before and after its kernels lives here:
//   * `apply(X, label_matrix, tau=0, epsilon='auto', k=25, normalize=False)` is a METH_FASTCALL
//     CPython function
//     (no pybind dispatch, no Python frame): argument checks with the reference's error
//     behaviour, tensor marshalling, the workspace from torch's caching allocator, gll_forward on
//     the current HIP stream, and -- when X, label_matrix or a tensor tau / epsilon requires
//     grad -- one autograd Node with its saved state in plain members (no IValue map, no
//     torch::autograd::Function bookkeeping).  The node's backward is gll_backward_batched, plus
//     one gll_param_grad_batched call when a gradient of label_matrix, tau or epsilon is wanted
//     (the reference returns None for them, GLL.py:177);
//   * `ce_loss(X, label_matrix, targets, tau=0, epsilon='auto', k=25, normalize=False)` is the
//     same call followed
//     by the cross-entropy head (gll_ce_head_batched: custom_ce_loss of losses.py:128-136 and the
//     argmax accuracy of FullySup.py:156-171 in one kernel); its node is the same one, holding
//     the head's dloss/dU;
//   * `margin_loss(X, label_matrix, other, tau=0, epsilon='auto', k=25, normalize=False)` is the
//     same call followed by the Carlini-Wagner margin head (gll_margin_head_batched: the top-2
//     labels and the clamped margin of adversarial.py:688-751 in one kernel), on the same node;
//   * `objective(X, label_matrix, targets, ..., weights, score, score_out, indices)` is the same
//     call followed by the score/objective head (gll_objective_head_batched: the weighted
//     cross-entropy / entropy / l2 loss and the score store of FullySup.py:165-175 in one kernel),
//     on the same node;
//   * neighbors= (the last argument of all four): the caller's neighbour lists instead of the
//     search -- gll_forward_lists_batched with GLL_FLAG_KNN_GIVEN; the node, the
//     heads and the parameter gradients are the same;
//   * the front end: an fp32 X with normalize=False goes to the kernels as it is;
//     normalize=True, or an fp16 / bf16 X, takes one gll_features_forward launch into a fresh fp32
//     X^ (and rnorm), which the node saves instead of X, and one gll_features_backward launch that
//     writes the gradient in X's dtype;
//   * the device status words (tiny eps, CG non-convergence, grid-barrier failure) accumulate in
//     a sticky per-device sink that is copied to pinned memory every kFlushEvery calls and turned
//     into the reference's warnings (GLL.py:240-241, 273-274) at a later call, with no host sync.
// A leading batch dimension (X: B x n x d, label_matrix: B x base x C or shared base x C) runs
// B independent graphs through gll_forward_batched / gll_backward_batched.
// No numerics here.
#include <Python.h>
#include <torch/extension.h>
#include <torch/csrc/autograd/function.h>
#include <torch/csrc/autograd/functions/utils.h>
#include <torch/csrc/autograd/python_variable.h>
#include <torch/csrc/autograd/saved_variable.h>
#include <c10/hip/HIPFunctions.h>
#include <c10/hip/HIPStream.h>
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <deque>
#include <mutex>
#include <string>
#include <vector>

#include "gll.h"

namespace {

using torch::autograd::variable_list;

constexpr int64_t kDefaultK = 25;       // GLL.py:27
constexpr int64_t kMaxK = 257;          // include/gll.h: 2 <= K <= 257
constexpr int kMaxIter = 1000;
constexpr float kRtol = 1e-6f;
constexpr int kFlushEvery = 64;         // calls between status copies
constexpr int kRing = 8;                // status copies in flight per device

// ------------------------------------------------------------------------------------------
// Python-level errors raised from C++ (the functions below hold the GIL)
// ------------------------------------------------------------------------------------------
struct PyErrSet {};   // a Python exception is set: unwind to the CPython entry point

[[noreturn]] void raise_py(PyObject* type, const std::string& msg) {
    PyErr_SetString(type, msg.c_str());
    throw PyErrSet{};
}

void warn_py(PyObject* category, const std::string& msg) {
    if (PyErr_WarnEx(category, msg.c_str(), 1) < 0) throw PyErrSet{};   // -W error
}

// ------------------------------------------------------------------------------------------
// Status sink per device (GLL_ST_* words; include/gll.h gll_problem.status_sink)
// ------------------------------------------------------------------------------------------
struct StatusCopy {
    hipEvent_t ev = nullptr;
    int32_t* host = nullptr;   // pinned, GLL_ST_NWORDS
    bool busy = false;
};

struct DeviceStatus {
    at::Tensor sink;           // int32 [GLL_ST_NWORDS] on the device, sticky between flushes
    int calls = 0;
    StatusCopy ring[kRing];
    std::deque<int> order;     // ring slots in flight, oldest first
};

std::mutex g_status_mu;
std::vector<DeviceStatus*> g_status;   // by device index (never freed: process lifetime)

DeviceStatus& status_of(int dev) {
    std::lock_guard<std::mutex> lk(g_status_mu);
    if (int(g_status.size()) <= dev) g_status.resize(dev + 1, nullptr);
    DeviceStatus*& s = g_status[dev];
    if (!s) {
        s = new DeviceStatus;
        s->sink = at::zeros({GLL_ST_NWORDS},
                            at::TensorOptions().dtype(at::kInt).device(at::kCUDA, dev));
    }
    return *s;
}

// Turn one completed copy of the status words into the reference's warnings (GLL.py:240-241
// warns; a non-converged CG prints at GLL.py:273-274) or an error (a lost grid barrier).
void report(const int32_t* st) {
    if (st[GLL_ST_SOLVE_FAILED])
        raise_py(PyExc_RuntimeError,
                 "GLL: the fused backward's gradient gave up waiting for the adjoint solves; "
                 "its grad_X was written as NaN");
    if (st[GLL_ST_GRID_RESCUED])
        warn_py(PyExc_RuntimeWarning,
                "GLL: " + std::to_string(st[GLL_ST_GRID_RESCUED]) +
                    " whole-GPU CG solve(s) lost their grid barrier (other kernels held the "
                    "CUs) and were solved by one workgroup instead: correct, slower");
    if (st[GLL_ST_TINY_EPS]) warn_py(PyExc_UserWarning, "Epsilon in KNN is very close to zero.");
    if (st[GLL_ST_LIST_DROPPED])
        warn_py(PyExc_UserWarning,
                "GLL neighbors: " + std::to_string(st[GLL_ST_LIST_DROPPED]) +
                    " list entries were dropped (an index outside [0, n) or a repeat within a row)");
    if (st[GLL_ST_FWD_NONCONV])
        warn_py(PyExc_RuntimeWarning,
                "GLL forward CG: " + std::to_string(st[GLL_ST_FWD_NONCONV]) +
                    " column solve(s) reached max_iter (" + std::to_string(st[GLL_ST_FWD_ITERS]) +
                    " iterations)");
    if (st[GLL_ST_BWD_NONCONV])
        warn_py(PyExc_RuntimeWarning,
                "GLL adjoint CG: " + std::to_string(st[GLL_ST_BWD_NONCONV]) +
                    " column solve(s) reached max_iter (" + std::to_string(st[GLL_ST_BWD_ITERS]) +
                    " iterations)");
}

// Completed copies (all of them when `block`), oldest first.
void poll(DeviceStatus& s, bool block) {
    while (!s.order.empty()) {
        StatusCopy& c = s.ring[s.order.front()];
        if (block) {
            (void)hipEventSynchronize(c.ev);
        } else if (hipEventQuery(c.ev) != hipSuccess) {
            (void)hipGetLastError();   // hipErrorNotReady must not linger as the last error
            return;
        }
        s.order.pop_front();
        c.busy = false;
        int32_t st[GLL_ST_NWORDS];
        std::memcpy(st, c.host, sizeof(st));
        report(st);
    }
}

// Copy the sink to pinned memory behind this stream's work, then clear it.
void flush(DeviceStatus& s, int dev, hipStream_t stream) {
    int slot = -1;
    for (int q = 0; q < kRing; ++q)
        if (!s.ring[q].busy) {
            slot = q;
            break;
        }
    if (slot < 0) {   // every copy still in flight: wait for the oldest
        poll(s, false);
        if (s.order.size() == size_t(kRing)) {
            StatusCopy& c = s.ring[s.order.front()];
            (void)hipEventSynchronize(c.ev);
            poll(s, false);
        }
        for (int q = 0; q < kRing; ++q)
            if (!s.ring[q].busy) {
                slot = q;
                break;
            }
        if (slot < 0) return;
    }
    StatusCopy& c = s.ring[slot];
    if (!c.ev) {
        c10::DeviceGuard g(c10::Device(c10::kCUDA, dev));
        if (hipEventCreateWithFlags(&c.ev, hipEventDisableTiming) != hipSuccess ||
            hipHostMalloc(reinterpret_cast<void**>(&c.host), GLL_ST_NWORDS * sizeof(int32_t),
                          hipHostMallocDefault) != hipSuccess) {
            (void)hipGetLastError();
            raise_py(PyExc_RuntimeError, "GLL: cannot allocate the status copy buffers");
        }
    }
    void* sink = s.sink.data_ptr();
    if (hipMemcpyAsync(c.host, sink, GLL_ST_NWORDS * sizeof(int32_t), hipMemcpyDeviceToHost,
                       stream) != hipSuccess ||
        hipEventRecord(c.ev, stream) != hipSuccess ||
        hipMemsetAsync(sink, 0, GLL_ST_NWORDS * sizeof(int32_t), stream) != hipSuccess) {
        (void)hipGetLastError();
        raise_py(PyExc_RuntimeError, "GLL: status copy failed");
    }
    c.busy = true;
    s.order.push_back(slot);
    s.calls = 0;
}

hipStream_t current_stream(int dev) { return c10::hip::getCurrentHIPStream(dev).stream(); }

void after_call(DeviceStatus& s, int dev, hipStream_t stream) {
    if (++s.calls >= kFlushEvery) flush(s, dev, stream);
}

// ------------------------------------------------------------------------------------------
// Tensor marshalling
// ------------------------------------------------------------------------------------------
int dtype_code(at::Tensor& t) {
    switch (t.scalar_type()) {
        case at::kFloat: return GLL_DT_F32;
        case at::kDouble: return GLL_DT_F64;
        case at::kLong: return GLL_DT_I64;
        default: t = t.to(at::kFloat); return GLL_DT_F32;
    }
}

at::Tensor features(const at::Tensor& X, const c10::Device& dev) {
    // the common case (fp32, contiguous, aligned, on the device) needs no new tensor
    if (X.device() == dev && X.scalar_type() == at::kFloat && X.is_contiguous() &&
        reinterpret_cast<uintptr_t>(X.data_ptr()) % 16 == 0)
        return X;
    at::Tensor X32 = X.detach().to(dev, at::kFloat).contiguous();
    if (reinterpret_cast<uintptr_t>(X32.data_ptr()) % 16) X32 = X32.clone();  // 16-B vector path
    return X32;
}

// Element type of the front end (gll_features_*) for a feature dtype; < 0: none (torch casts)
int feature_code(at::ScalarType t) {
    switch (t) {
        case at::kFloat: return GLL_XT_F32;
        case at::kHalf: return GLL_XT_F16;
        case at::kBFloat16: return GLL_XT_BF16;
        default: return -1;
    }
}

void check_rc(int rc, const char* what) {
    TORCH_CHECK(rc == GLL_OK, what, " failed: ", gll_strerror(rc), " (code ", rc, ")");
}

gll_problem make_problem(int64_t n, int64_t d, int64_t base, int64_t C, int64_t k, double tau,
                         double eps, int32_t* sink) {
    gll_problem p;
    p.n = int32_t(n);
    p.d = int32_t(d);
    p.base = int32_t(base);
    p.C = int32_t(C);
    p.K = int32_t(std::min<int64_t>(k, n));
    p.max_iter = kMaxIter;
    p.tau = float(tau);
    p.eps = float(eps);
    p.rtol = kRtol;
    p.flags = 0;
    p.status_sink = sink;
    return p;
}

// Exploding-gradient report of the adversarial scripts' inline copy
// (train_and_adversarial.py:177-183): < 0 = off (the default).
double g_grad_diag = -1.0;

// ------------------------------------------------------------------------------------------
// The autograd node: gll_backward over the saved workspace (GLL.py:76-177)
// ------------------------------------------------------------------------------------------
// Metadata of an input whose gradient takes that input's dtype, device and shape.
struct GradLike {
    int slot = -1;   // index among the node's inputs (next edges); < 0: not a tensor input
    std::vector<int64_t> sizes;
    at::ScalarType dtype = at::kFloat;
    c10::Device device = c10::Device(c10::kCPU);

    void set(int s, const at::Tensor& t) {
        slot = s;
        sizes = t.sizes().vec();
        dtype = t.scalar_type();
        device = t.device();
    }
    at::Tensor like(const at::Tensor& v) const { return v.to(device, dtype).reshape(sizes); }
};

struct LaplaceBackward : public torch::autograd::Node {
    torch::autograd::SavedVariable X_;   // X, or on the front-end route the fp32 X^ made from it
    GradLike Xin_;                       // X as given: its gradient's dtype, device and shape
    bool front_ = false;                 // gll_features_forward made X^ (and rnorm_)
    int zcode_ = GLL_XT_F32, uflags_ = 0;
    at::Tensor rnorm_;
    at::Tensor ws_;
    gll_problem p_{};
    int64_t B_ = 1;
    double diag_ = -1.0;
    // inputs in edge order: X, label_matrix, then tau and epsilon where they are tensors
    int n_inputs_ = 1;
    GradLike Y_, tau_, eps_;
    bool Y_shared_ = false;   // 2-D label_matrix with batched X: the gradient sums over graphs
    at::Tensor gbar_;         // ce_loss / margin_loss: dloss/dU (fp32, U's shape); the node's
                              // output is the loss

    std::string name() const override { return "LaplaceLearningSparseHardBackward"; }

    void release_variables() override {
        std::lock_guard<std::mutex> lk(mutex_);
        X_.reset_data();
        rnorm_.reset();
        ws_.reset();
        gbar_.reset();
    }

    variable_list apply(variable_list&& grads) override {
        std::lock_guard<std::mutex> lk(mutex_);
        const at::Tensor X = X_.unpack(shared_from_this());   // raises on a second backward
        variable_list out(n_inputs_);
        if (!grads[0].defined()) return out;
        const c10::Device dev = ws_.device();
        c10::DeviceGuard guard(dev);
        at::Tensor X32 = front_ ? X : features(X, dev);
        at::Tensor g = grads[0].device() == dev ? grads[0] : grads[0].to(dev);
        if (gbar_.defined()) {   // ce_loss: dL/dU = gbar * dL/dloss, broadcast over the graphs
            const at::Tensor gl = gbar_.dim() == 3 ? g.reshape({-1, 1, 1}) : g.reshape({});
            g = at::empty_like(gbar_);
            at::mul_out(g, gbar_, gl);
        }
        if (g.scalar_type() != at::kFloat && g.scalar_type() != at::kDouble) g = g.to(at::kDouble);
        if (!g.is_contiguous()) g = g.contiguous();
        const int gcode = g.scalar_type() == at::kFloat ? GLL_DT_F32 : GLL_DT_F64;
        at::Tensor gradX = at::empty(X.sizes(), X32.options());
        check_rc(gll_backward_batched(&p_, int(B_), X32.data_ptr<float>(), ws_.data_ptr(),
                                      g.data_ptr(), gcode, gradX.data_ptr<float>(),
                                      current_stream(dev.index())),
                 "gll_backward");
        if (diag_ >= 0.0) report_gradient(g, gradX);
        int what = 0;
        if (Y_.slot >= 0 && at::isFloatingType(Y_.dtype) && task_should_compute_output(Y_.slot))
            what |= GLL_PG_Y;
        if (tau_.slot >= 0 && task_should_compute_output(tau_.slot)) what |= GLL_PG_TAU;
        if (eps_.slot >= 0 && p_.eps > 0.f && task_should_compute_output(eps_.slot))
            what |= GLL_PG_EPS;
        if (what) param_grads(what, X32, out);
        if (task_should_compute_output(0)) {
            if (front_) {   // through the normalisation, rounded once to the front end's dtype
                const at::ScalarType zt = zcode_ == GLL_XT_F16    ? at::kHalf
                                          : zcode_ == GLL_XT_BF16 ? at::kBFloat16
                                                                  : at::kFloat;
                at::Tensor gZ = at::empty(X.sizes(), X32.options().dtype(zt));
                check_rc(gll_features_backward(
                             B_ * int64_t(p_.n), p_.d, gradX.data_ptr<float>(), X32.data_ptr<float>(),
                             rnorm_.defined() ? rnorm_.data_ptr<float>() : nullptr, uflags_,
                             gZ.data_ptr(), zcode_, current_stream(dev.index())),
                         "gll_features_backward");
                gradX = gZ;
            }
            if (gradX.device() != Xin_.device || gradX.scalar_type() != Xin_.dtype)
                gradX = gradX.to(Xin_.device, Xin_.dtype);
            out[0] = gradX;
        }
        return out;
    }

    // label_matrix / tau / epsilon gradients: one gll_param_grad_batched over the workspace the
    // backward just completed.  Batched input: shared labels and the scalars sum over graphs
    // (float64).
    void param_grads(int what, const at::Tensor& X32, variable_list& out) {
        const c10::Device dev = ws_.device();
        const auto f64 = X32.options().dtype(at::kDouble);
        at::Tensor gY, gtau, geps, scratch;
        if (what & GLL_PG_Y) gY = at::empty({B_, int64_t(p_.base), int64_t(p_.C)}, X32.options());
        if (what & GLL_PG_TAU) gtau = at::empty({B_}, f64);
        if (what & GLL_PG_EPS) geps = at::empty({B_}, f64);
        if (what & (GLL_PG_TAU | GLL_PG_EPS))
            scratch = at::empty({int64_t(gll_param_grad_scratch_bytes(&p_, int(B_)))},
                                X32.options().dtype(at::kByte));
        check_rc(gll_param_grad_batched(&p_, int(B_), ws_.data_ptr(), what,
                                        gY.defined() ? gY.data_ptr<float>() : nullptr,
                                        gtau.defined() ? gtau.data_ptr<double>() : nullptr,
                                        geps.defined() ? geps.data_ptr<double>() : nullptr,
                                        scratch.defined() ? scratch.data_ptr() : nullptr,
                                        current_stream(dev.index())),
                 "gll_param_grad");
        if (what & GLL_PG_Y) out[Y_.slot] = Y_.like(Y_shared_ ? gY.to(at::kDouble).sum(0) : gY);
        if (what & GLL_PG_TAU) out[tau_.slot] = tau_.like(B_ > 1 ? gtau.sum() : gtau);
        if (what & GLL_PG_EPS) out[eps_.slot] = eps_.like(B_ > 1 ? geps.sum() : geps);
    }

    // train_and_adversarial.py:177-183 (synchronises: diagnostic mode only)
    void report_gradient(const at::Tensor& g, const at::Tensor& gradX) {
        const double out_norm = at::linalg_vector_norm(gradX).item<double>();
        if (!(out_norm > diag_)) return;
        gll_view v;
        check_rc(gll_workspace_view(&p_, ws_.data_ptr(), &v), "gll_workspace_view");
        const int64_t m = int64_t(p_.n) - p_.base;
        const int64_t off = reinterpret_cast<char*>(v.wadj) - static_cast<char*>(ws_.data_ptr());
        const at::Tensor wadj = ws_.narrow(0, off, 4 * m * p_.C).view(at::kFloat);
        const double gn = at::linalg_vector_norm(g.to(at::kDouble)).item<double>();
        const double wn = at::linalg_vector_norm(wadj.to(at::kDouble)).item<double>();
        pybind11::gil_scoped_acquire gil;
        pybind11::print("possible exploding gradient");
        pybind11::print("grad norm: ", gn);
        pybind11::print("w norm: ", wn);
        pybind11::print("out norm: ", out_norm);
    }
};

// ------------------------------------------------------------------------------------------
// apply(X, label_matrix, tau=0, epsilon='auto', k=25, normalize=False, neighbors=None)  GLL.py:14-73
// ------------------------------------------------------------------------------------------
double parse_float(PyObject* o, const char* what) {
    const double v = PyFloat_AsDouble(o);
    if (v == -1.0 && PyErr_Occurred()) {
        PyErr_Clear();
        raise_py(PyExc_TypeError, std::string(what) + " must be a number");
    }
    return v;
}

// tau / epsilon given as a tensor (0-dim or one element, any float dtype, any device): its value
// is read once here -- a host synchronisation when it lives on the GPU -- and it becomes an
// input of the autograd node.
bool scalar_tensor_arg(PyObject* o, const char* what, at::Tensor& t, double& v) {
    if (!THPVariable_Check(o)) return false;
    t = THPVariable_Unpack(o);
    if (t.numel() != 1 || !at::isFloatingType(t.scalar_type()))
        raise_py(PyExc_TypeError, std::string(what) + " as a tensor must hold one floating-point value");
    v = t.item<double>();
    return true;
}

// epsilon: a number > 0 (fixed, GLL.py:226) or 'auto' (GLL.py:200-205) -> <= 0 for the ABI
double parse_eps(PyObject* o, at::Tensor& t) {
    double e;
    if (scalar_tensor_arg(o, "epsilon", t, e)) {
        if (t.requires_grad() && !(e > 0.0))
            raise_py(PyExc_ValueError, "epsilon as a tensor that requires grad must be > 0");
    } else if (PyUnicode_Check(o)) {
        if (PyUnicode_CompareWithASCIIString(o, "auto") != 0) {
            const char* s = PyUnicode_AsUTF8(o);
            raise_py(PyExc_ValueError,
                     std::string("epsilon must be a number or 'auto', got '") + (s ? s : "?") + "'");
        }
        return 0.0;
    } else {
        e = parse_float(o, "epsilon");
    }
    if (!(e > 0.0)) {
        // GLL.py:240-241 warns for any eps < 1e-10.  The reference uses eps only as the product
        // eps[rows] * eps[cols] (GLL.py:233-234), so a negative eps builds the graph of |eps|;
        // eps = 0 (or NaN) divides by zero there, here it disconnects the graph (W = 0)
        warn_py(PyExc_UserWarning, "Epsilon in KNN is very close to zero.");
        return e < 0.0 ? -e : 1e-30;
    }
    return e;
}

const at::Tensor& tensor_arg(PyObject* o, const char* what) {
    if (!THPVariable_Check(o)) raise_py(PyExc_TypeError, std::string(what) + " must be a Tensor");
    return THPVariable_Unpack(o);
}

// Positional / keyword arguments of a METH_FASTCALL entry into `a` (one slot per name).
void collect_args(const char* fn, const char* const* names, int nn, PyObject* const* args,
                  Py_ssize_t nargs, PyObject* kwnames, PyObject** a) {
    if (nargs > nn)
        raise_py(PyExc_TypeError, std::string(fn) + "() takes at most " + std::to_string(nn) +
                                      " arguments");
    for (Py_ssize_t q = 0; q < nargs; ++q) a[q] = args[q];
    if (kwnames) {
        const Py_ssize_t nk = PyTuple_GET_SIZE(kwnames);
        for (Py_ssize_t q = 0; q < nk; ++q) {
            const char* kn = PyUnicode_AsUTF8(PyTuple_GET_ITEM(kwnames, q));
            int slot = -1;
            for (int t = 0; t < nn && kn; ++t)
                if (std::strcmp(kn, names[t]) == 0) slot = t;
            if (slot < 0 || a[slot])
                raise_py(PyExc_TypeError, std::string(fn) + "() got an unexpected or repeated "
                                              "keyword argument '" + (kn ? kn : "?") + "'");
            a[slot] = args[nargs + q];
        }
    }
}

// One forward of the layer, shared by apply and ce_loss: argument checks, marshalling, the
// workspace, gll_forward_batched on the current stream and the status bookkeeping.  The device
// guard lives as long as the call does.
struct LayerCall {
    at::Tensor X, Y, tau_t, eps_t;   // the inputs as given (tau_t / eps_t: defined where tensors)
    at::Tensor X32, ws, U;
    at::Tensor rnorm;                // front-end route with normalize: 1 / max(|z_i|, 1e-12)
    bool front = false;              // X32 is the X^ gll_features_forward made
    int zcode = GLL_XT_F32, uflags = 0;
    gll_problem p{};
    int64_t B = 1, n = 0, base = 0, C = 0;
    bool batched = false;
    int devi = 0;
    hipStream_t s = nullptr;
    c10::OptionalDeviceGuard guard;
};

void layer_forward(LayerCall& c, const char* fn, PyObject* aX, PyObject* aY, PyObject* atau,
                   PyObject* aeps, PyObject* ak, PyObject* anorm, PyObject* anbr) {
    if (!aX || !aY) raise_py(PyExc_TypeError, std::string(fn) + "() needs X and label_matrix");
    c.X = tensor_arg(aX, "X");
    c.Y = tensor_arg(aY, "label_matrix");
    const at::Tensor& X = c.X;
    const at::Tensor& Y = c.Y;
    double tau = 0.0;
    if (atau && !scalar_tensor_arg(atau, "tau", c.tau_t, tau)) tau = parse_float(atau, "tau");
    const double eps = aeps ? parse_eps(aeps, c.eps_t) : 0.0;
    int64_t k = kDefaultK;
    if (ak) {
        k = PyLong_AsLongLong(ak);
        if (k == -1 && PyErr_Occurred()) {
            PyErr_Clear();
            raise_py(PyExc_TypeError, "k must be an int");
        }
    }
    bool normalize = false;
    if (anorm) {
        if (!PyBool_Check(anorm)) raise_py(PyExc_TypeError, "normalize must be a bool");
        normalize = anorm == Py_True;
    }
    if ((X.dim() != 2 && X.dim() != 3) || (Y.dim() != 2 && Y.dim() != X.dim()))
        raise_py(PyExc_ValueError,
                 "X must be n x d (or B x n x d), label_matrix base x C (or B x base x C)");
    const int64_t n = X.size(-2), d = X.size(-1), base = Y.size(-2), C = Y.size(-1);
    const int64_t kk = std::min(k, n);
    if (kk < 2 || kk > kMaxK)
        raise_py(PyExc_ValueError, "k = " + std::to_string(k) + " (n = " + std::to_string(n) +
                                       "): the kNN count incl. self must satisfy 2 <= min(k, n) <= " +
                                       std::to_string(kMaxK));
    // neighbors: the caller's lists in place of the search: n x K (the
    // reference's knn_ind, column 0 = self, not read) or n x (K - 1), with X's leading B; checked
    // on metadata alone, before any GPU call
    at::Tensor nbr;
    if (anbr && anbr != Py_None) {
        nbr = tensor_arg(anbr, "neighbors");
        const int64_t w = nbr.dim() >= 1 ? nbr.size(-1) : -1;
        if (!at::isIntegralType(nbr.scalar_type(), false))
            raise_py(PyExc_ValueError, "neighbors must hold integers (int32 or int64)");
        if (nbr.dim() != X.dim() || nbr.size(-2) != n || (X.dim() == 3 && nbr.size(0) != X.size(0)) ||
            (w != kk && w != kk - 1))
            raise_py(PyExc_ValueError,
                     "neighbors must be " + std::string(X.dim() == 3 ? "B x " : "") + "n x k or n x (k - 1) = " +
                         std::to_string(n) + " x " + std::to_string(kk) + " or " + std::to_string(kk - 1));
    }
    // device: X's, or the current one for CPU input (the result goes back to the CPU)
    int devi;
    if (X.is_cuda()) {
        devi = X.device().index();
    } else {
        if (c10::hip::device_count() == 0)
            raise_py(PyExc_RuntimeError, "graphlearninglayer_amd needs a ROCm GPU (no CPU fallback)");
        devi = c10::hip::current_device();
    }
    const c10::Device dev(c10::kCUDA, devi);
    c.guard.reset_device(dev);
    DeviceStatus& st = status_of(devi);
    if (!st.order.empty()) poll(st, false);
    const bool batched = X.dim() == 3;
    const int64_t B = batched ? X.size(0) : 1;
    c.s = current_stream(devi);
    const bool half = X.scalar_type() == at::kHalf || X.scalar_type() == at::kBFloat16;
    if (normalize || half) {
        // the front end: one launch over all B n rows converts (and normalises) into a fresh X^
        if (d > 4096)
            raise_py(PyExc_ValueError, "normalize=True and fp16 / bf16 features need d <= 4096, got d = " +
                                           std::to_string(d));
        at::Tensor Z = X.detach();
        if (feature_code(Z.scalar_type()) < 0) Z = Z.to(at::kFloat);   // float64: fp32 as today
        Z = Z.to(dev).contiguous();
        c.front = true;
        c.zcode = feature_code(Z.scalar_type());
        c.uflags = normalize ? GLL_UF_NORMALIZE : 0;
        c.X32 = at::empty(X.sizes(), Z.options().dtype(at::kFloat));
        if (normalize) c.rnorm = at::empty({B * n}, c.X32.options());
        check_rc(gll_features_forward(B * n, int32_t(d), Z.data_ptr(), c.zcode, c.uflags,
                                      c.X32.data_ptr<float>(),
                                      normalize ? c.rnorm.data_ptr<float>() : nullptr, c.s),
                 "gll_features_forward");
    } else {
        c.X32 = features(X, dev);
    }
    at::Tensor Yd = Y.device() == dev ? Y : Y.detach().to(dev);
    const int ycode = dtype_code(Yd);
    if (batched && Y.dim() == 2) Yd = Yd.unsqueeze(0).expand({B, base, C});   // shared labels
    if (batched && Yd.size(0) != B)
        raise_py(PyExc_ValueError, "label_matrix batch " + std::to_string(Yd.size(0)) +
                                       " != " + std::to_string(B));
    if (!Yd.is_contiguous()) Yd = Yd.contiguous();
    c.p = make_problem(n, d, base, C, k, tau, eps, st.sink.data_ptr<int32_t>());
    if (nbr.defined()) {
        c.p.flags |= GLL_FLAG_KNN_GIVEN;   // no distance buffer in the workspace
        nbr = nbr.detach();
        if (nbr.size(-1) == kk) nbr = nbr.narrow(-1, 1, kk - 1);   // drop the self column
        nbr = nbr.to(dev, at::kInt).contiguous();
    }
    const size_t nb = gll_workspace_bytes(&c.p);
    if (nb == 0)
        raise_py(PyExc_ValueError, "unsupported GLL problem n=" + std::to_string(n) + " d=" +
                                       std::to_string(d) + " base=" + std::to_string(base) +
                                       " C=" + std::to_string(C) + " k=" + std::to_string(k));
    const auto opts = c.X32.options();
    c.ws = at::empty({int64_t(nb) * B}, opts.dtype(at::kByte));
    c.U = batched ? at::empty({B, n - base, C}, opts.dtype(at::kDouble))
                  : at::empty({n - base, C}, opts.dtype(at::kDouble));
    if (nbr.defined())
        check_rc(gll_forward_lists_batched(&c.p, int(B), c.X32.data_ptr<float>(),
                                           nbr.data_ptr<int32_t>(), Yd.data_ptr(), ycode,
                                           c.ws.data_ptr(), c.U.data_ptr<double>(), c.s),
                 "gll_forward_lists");
    else
        check_rc(gll_forward_batched(&c.p, int(B), c.X32.data_ptr<float>(), Yd.data_ptr(), ycode,
                                     c.ws.data_ptr(), c.U.data_ptr<double>(), c.s),
                 "gll_forward");
    after_call(st, devi, c.s);
    c.B = B;
    c.n = n;
    c.base = base;
    c.C = C;
    c.batched = batched;
    c.devi = devi;
}

std::vector<at::Tensor> grad_inputs(const LayerCall& c) {
    std::vector<at::Tensor> inputs{c.X, c.Y};
    if (c.tau_t.defined()) inputs.push_back(c.tau_t);
    if (c.eps_t.defined()) inputs.push_back(c.eps_t);
    return inputs;
}

// The autograd node of a completed forward (it takes the workspace over).
std::shared_ptr<LaplaceBackward> make_node(LayerCall& c, const std::vector<at::Tensor>& inputs) {
    auto node = std::shared_ptr<LaplaceBackward>(new LaplaceBackward(),
                                                 torch::autograd::deleteNode);
    node->set_next_edges(torch::autograd::collect_next_edges(inputs));
    node->n_inputs_ = int(inputs.size());
    node->Y_.set(1, c.Y);
    node->Y_shared_ = c.batched && c.Y.dim() == 2;
    if (c.tau_t.defined()) node->tau_.set(2, c.tau_t);
    if (c.eps_t.defined()) node->eps_.set(c.tau_t.defined() ? 3 : 2, c.eps_t);
    node->X_ = torch::autograd::SavedVariable(c.front ? c.X32 : c.X, false);
    node->Xin_.set(0, c.X);
    node->front_ = c.front;
    node->zcode_ = c.zcode;
    node->uflags_ = c.uflags;
    node->rnorm_ = c.rnorm;
    node->ws_ = std::move(c.ws);
    node->p_ = c.p;
    node->B_ = c.B;
    node->diag_ = g_grad_diag;
    return node;
}

PyObject* apply_impl(PyObject* const* args, Py_ssize_t nargs, PyObject* kwnames) {
    static const char* names[] = {"X", "label_matrix", "tau", "epsilon", "k", "normalize",
                                  "neighbors"};
    PyObject* a[7] = {};
    collect_args("apply", names, 7, args, nargs, kwnames, a);
    LayerCall c;
    layer_forward(c, "apply", a[0], a[1], a[2], a[3], a[4], a[5], a[6]);
    const std::vector<at::Tensor> inputs = grad_inputs(c);
    if (torch::autograd::compute_requires_grad(inputs))
        torch::autograd::set_history(c.U, make_node(c, inputs));
    return THPVariable_Wrap(c.X.is_cuda() ? std::move(c.U) : c.U.cpu());
}

// What the loss heads (ce_loss, margin_loss) share around their kernel.
// One int64 per unlabeled row on the device, from a tensor of integers of shape m (B x m with a
// batched X).
at::Tensor head_rows_arg(const LayerCall& c, const at::Tensor& T, const char* what) {
    const int64_t m = c.n - c.base;
    const bool shape_ok = c.batched ? (T.dim() == 2 && T.size(0) == c.B && T.size(1) == m)
                                    : (T.dim() == 1 && T.size(0) == m);
    if (!shape_ok)
        raise_py(PyExc_ValueError, std::string(what) + " must have shape " +
                                       (c.batched ? "B x m = " + std::to_string(c.B) + " x " : "m = ") +
                                       std::to_string(m));
    return T.detach().to(c10::Device(c10::kCUDA, c.devi), at::kLong).contiguous();
}

// The result tuple of a head; out[0] is the loss.  When a gradient is wanted (gbar defined) the
// loss takes the layer's node, which keeps the head's dloss/dU.
PyObject* head_result(LayerCall& c, const std::vector<at::Tensor>& inputs, at::Tensor gbar,
                      std::vector<at::Tensor> out) {
    if (gbar.defined()) {
        auto node = make_node(c, inputs);
        node->gbar_ = std::move(gbar);
        torch::autograd::set_history(out[0], node);
    }
    PyObject* tup = PyTuple_New(Py_ssize_t(out.size()));
    if (!tup) throw PyErrSet{};
    for (size_t q = 0; q < out.size(); ++q)
        PyTuple_SET_ITEM(tup, q, THPVariable_Wrap(c.X.is_cuda() ? out[q] : out[q].cpu()));
    return tup;
}

// ------------------------------------------------------------------------------------------
// ce_loss(X, label_matrix, targets, tau=0, epsilon='auto', k=25, normalize=False): the layer and the
// cross-entropy head its callers put behind it (losses.py:128-136, FullySup.py:156-171) in one
// call.  gll_ce_head_batched reads the predictions the forward left in the workspace and writes
// loss, row losses, predicted labels, the correct count and -- when a gradient is wanted --
// dloss/dU, which the node keeps: its backward is the layer's, fed gbar * grad_loss.
// ------------------------------------------------------------------------------------------
PyObject* ce_loss_impl(PyObject* const* args, Py_ssize_t nargs, PyObject* kwnames) {
    static const char* names[] = {"X", "label_matrix", "targets", "tau", "epsilon", "k", "normalize",
                                  "neighbors"};
    PyObject* a[8] = {};
    collect_args("ce_loss", names, 8, args, nargs, kwnames, a);
    if (!a[2]) raise_py(PyExc_TypeError, "ce_loss() needs targets");
    const at::Tensor& T = tensor_arg(a[2], "targets");
    if (!at::isIntegralType(T.scalar_type(), false))
        raise_py(PyExc_TypeError, "targets must hold integers");
    LayerCall c;
    layer_forward(c, "ce_loss", a[0], a[1], a[3], a[4], a[5], a[6], a[7]);
    const int64_t m = c.n - c.base;
    at::Tensor Td = head_rows_arg(c, T, "targets");
    const auto f64 = c.X32.options().dtype(at::kDouble);
    const auto i64 = c.X32.options().dtype(at::kLong);
    const std::vector<int64_t> one = c.batched ? std::vector<int64_t>{c.B} : std::vector<int64_t>{};
    const std::vector<int64_t> rows = c.batched ? std::vector<int64_t>{c.B, m} : std::vector<int64_t>{m};
    at::Tensor loss = at::empty(one, f64), correct = at::empty(one, i64);
    at::Tensor row_loss = at::empty(rows, f64), labels = at::empty(rows, i64);
    const std::vector<at::Tensor> inputs = grad_inputs(c);
    const bool need_grad = torch::autograd::compute_requires_grad(inputs);
    at::Tensor gbar, scratch;
    if (need_grad) gbar = at::empty(c.U.sizes(), c.X32.options());
    const size_t sb = gll_ce_head_scratch_bytes(&c.p, int(c.B));
    if (sb) scratch = at::empty({int64_t(sb)}, c.X32.options().dtype(at::kByte));
    check_rc(gll_ce_head_batched(&c.p, int(c.B), c.ws.data_ptr(), Td.data_ptr<int64_t>(),
                                 loss.data_ptr<double>(),
                                 need_grad ? gbar.data_ptr<float>() : nullptr,
                                 row_loss.data_ptr<double>(), labels.data_ptr<int64_t>(),
                                 correct.data_ptr<int64_t>(),
                                 sb ? scratch.data_ptr() : nullptr, c.s),
             "gll_ce_head");
    return head_result(c, inputs, gbar, {loss, c.U, labels, row_loss, correct});
}

// ------------------------------------------------------------------------------------------
// margin_loss(X, label_matrix, other, tau=0, epsilon='auto', k=25, normalize=False): the layer and
// the Carlini-Wagner margin its attack loop puts behind it (adversarial.py:688-751) in one call.
// gll_margin_head_batched writes the two best classes of every row, the margin of the best over
// `other`, its mean, the count of rows whose best class is `other` and -- when a gradient is
// wanted -- dloss/dU for the same node ce_loss uses.  other = None: the top-2 query alone.
// ------------------------------------------------------------------------------------------
PyObject* margin_loss_impl(PyObject* const* args, Py_ssize_t nargs, PyObject* kwnames) {
    static const char* names[] = {"X", "label_matrix", "other", "tau", "epsilon", "k", "normalize",
                                  "neighbors"};
    PyObject* a[8] = {};
    collect_args("margin_loss", names, 8, args, nargs, kwnames, a);
    if (!a[2]) raise_py(PyExc_TypeError, "margin_loss() needs other (a tensor of integers or None)");
    at::Tensor T;   // undefined: other = None
    if (a[2] != Py_None) {
        T = tensor_arg(a[2], "other");
        if (!at::isIntegralType(T.scalar_type(), false))
            raise_py(PyExc_TypeError, "other must hold integers (or be None)");
    }
    LayerCall c;
    layer_forward(c, "margin_loss", a[0], a[1], a[3], a[4], a[5], a[6], a[7]);
    const int64_t m = c.n - c.base;
    at::Tensor Td;
    if (T.defined()) Td = head_rows_arg(c, T, "other");
    const auto f64 = c.X32.options().dtype(at::kDouble);
    const auto i64 = c.X32.options().dtype(at::kLong);
    const std::vector<int64_t> one = c.batched ? std::vector<int64_t>{c.B} : std::vector<int64_t>{};
    const std::vector<int64_t> rows = c.batched ? std::vector<int64_t>{c.B, m} : std::vector<int64_t>{m};
    at::Tensor loss = at::empty(one, f64), moved = at::empty(one, i64);
    at::Tensor row_margin = at::empty(rows, f64);
    at::Tensor labels = at::empty(rows, i64), second = at::empty(rows, i64);
    const std::vector<at::Tensor> inputs = grad_inputs(c);
    const bool need_grad = torch::autograd::compute_requires_grad(inputs);
    at::Tensor gbar, scratch;
    if (need_grad) gbar = at::empty(c.U.sizes(), c.X32.options());
    const size_t sb = gll_margin_head_scratch_bytes(&c.p, int(c.B));
    if (sb) scratch = at::empty({int64_t(sb)}, c.X32.options().dtype(at::kByte));
    check_rc(gll_margin_head_batched(&c.p, int(c.B), c.ws.data_ptr(),
                                     Td.defined() ? Td.data_ptr<int64_t>() : nullptr,
                                     loss.data_ptr<double>(),
                                     need_grad ? gbar.data_ptr<float>() : nullptr,
                                     row_margin.data_ptr<double>(), labels.data_ptr<int64_t>(),
                                     second.data_ptr<int64_t>(), moved.data_ptr<int64_t>(),
                                     sb ? scratch.data_ptr() : nullptr, c.s),
             "gll_margin_head");
    return head_result(c, inputs, gbar, {loss, c.U, labels, second, row_margin, moved});
}

// ------------------------------------------------------------------------------------------
// objective(X, label_matrix, targets, tau=0, epsilon='auto', k=25, normalize=False,
//           weights=(1, 0, 0), score=None, score_out=None, indices=None): the layer and the
// score-driven training step's head (FullySup.py:156-175) in one call.
// gll_objective_head_batched writes the weighted cross-entropy / entropy / l2 loss, the per-row
// terms, labels, the correct count, the chosen score scattered into `score_out` at `indices`
// and -- when a gradient is wanted -- dloss/dU for the same node ce_loss uses.
// targets = None: every row masked (the regularisers alone).
// ------------------------------------------------------------------------------------------
PyObject* objective_impl(PyObject* const* args, Py_ssize_t nargs, PyObject* kwnames) {
    static const char* names[] = {"X", "label_matrix", "targets", "tau", "epsilon", "k",
                                  "normalize", "weights", "score", "score_out", "indices",
                                  "neighbors"};
    PyObject* a[12] = {};
    collect_args("objective", names, 12, args, nargs, kwnames, a);
    if (!a[2]) raise_py(PyExc_TypeError, "objective() needs targets (a tensor of integers or None)");
    at::Tensor T;   // undefined: targets = None
    if (a[2] != Py_None) {
        T = tensor_arg(a[2], "targets");
        if (!at::isIntegralType(T.scalar_type(), false))
            raise_py(PyExc_TypeError, "targets must hold integers (or be None)");
    }
    double w[3] = {1.0, 0.0, 0.0};
    if (a[7] && a[7] != Py_None) {
        PyObject* seq = PySequence_Fast(a[7], "weights must be three numbers (w_ce, w_ent, w_l2)");
        if (!seq) throw PyErrSet{};
        const bool three = PySequence_Fast_GET_SIZE(seq) == 3;
        for (int q = 0; three && q < 3; ++q) {
            w[q] = PyFloat_AsDouble(PySequence_Fast_GET_ITEM(seq, q));
            if (w[q] == -1.0 && PyErr_Occurred()) {
                Py_DECREF(seq);
                throw PyErrSet{};
            }
        }
        Py_DECREF(seq);
        if (!three) raise_py(PyExc_ValueError, "weights must be three numbers (w_ce, w_ent, w_l2)");
    }
    int kind = GLL_SCORE_NONE;
    if (a[8] && a[8] != Py_None) {
        const char* sk = PyUnicode_Check(a[8]) ? PyUnicode_AsUTF8(a[8]) : nullptr;
        if (sk && std::strcmp(sk, "entropy") == 0) kind = GLL_SCORE_ENTROPY;
        else if (sk && std::strcmp(sk, "l2") == 0) kind = GLL_SCORE_L2;
        else raise_py(PyExc_ValueError, "score must be None, 'entropy' or 'l2'");
    }
    const bool has_out = a[9] && a[9] != Py_None, has_idx = a[10] && a[10] != Py_None;
    if (has_out != has_idx)
        raise_py(PyExc_ValueError, "score_out and indices go together: give both or neither");
    if (has_out && kind == GLL_SCORE_NONE)
        raise_py(PyExc_ValueError, "score_out needs score='entropy' or score='l2'");
    at::Tensor S, I;
    if (has_out) {
        S = tensor_arg(a[9], "score_out");
        I = tensor_arg(a[10], "indices");
        if (S.scalar_type() != at::kFloat || S.dim() != 1 || !S.is_contiguous() || !S.is_cuda())
            raise_py(PyExc_ValueError,
                     "score_out must be a contiguous float32 tensor of shape N on the layer's device");
        if (!at::isIntegralType(I.scalar_type(), false))
            raise_py(PyExc_TypeError, "indices must hold integers");
    } else {
        kind = GLL_SCORE_NONE;   // a score without a store: nothing to scatter
    }
    LayerCall c;
    layer_forward(c, "objective", a[0], a[1], a[3], a[4], a[5], a[6], a[11]);
    if (has_out && S.device().index() != c.devi)
        raise_py(PyExc_ValueError,
                 "score_out must be a contiguous float32 tensor of shape N on the layer's device");
    const int64_t m = c.n - c.base;
    at::Tensor Td, Id;
    if (T.defined()) Td = head_rows_arg(c, T, "targets");
    if (has_out) Id = head_rows_arg(c, I, "indices");
    const auto f64 = c.X32.options().dtype(at::kDouble);
    const auto i64 = c.X32.options().dtype(at::kLong);
    const std::vector<int64_t> one = c.batched ? std::vector<int64_t>{c.B} : std::vector<int64_t>{};
    const std::vector<int64_t> rows = c.batched ? std::vector<int64_t>{c.B, m} : std::vector<int64_t>{m};
    at::Tensor loss = at::empty(one, f64), correct = at::empty(one, i64);
    at::Tensor row_loss = at::empty(rows, f64), row_ent = at::empty(rows, f64);
    at::Tensor row_l2 = at::empty(rows, f64), labels = at::empty(rows, i64);
    const std::vector<at::Tensor> inputs = grad_inputs(c);
    const bool need_grad = torch::autograd::compute_requires_grad(inputs);
    at::Tensor gbar, scratch;
    if (need_grad) gbar = at::empty(c.U.sizes(), c.X32.options());
    const size_t sb = gll_objective_head_scratch_bytes(&c.p, int(c.B));
    if (sb) scratch = at::empty({int64_t(sb)}, c.X32.options().dtype(at::kByte));
    check_rc(gll_objective_head_batched(
                 &c.p, int(c.B), c.ws.data_ptr(), Td.defined() ? Td.data_ptr<int64_t>() : nullptr,
                 w[0], w[1], w[2], loss.data_ptr<double>(),
                 need_grad ? gbar.data_ptr<float>() : nullptr, row_loss.data_ptr<double>(),
                 row_ent.data_ptr<double>(), row_l2.data_ptr<double>(),
                 labels.data_ptr<int64_t>(), correct.data_ptr<int64_t>(), kind,
                 has_out ? S.data_ptr<float>() : nullptr, has_out ? S.size(0) : 0,
                 has_out ? Id.data_ptr<int64_t>() : nullptr, sb ? scratch.data_ptr() : nullptr,
                 c.s),
             "gll_objective_head");
    return head_result(c, inputs, gbar, {loss, c.U, labels, row_loss, correct, row_ent, row_l2});
}

template <PyObject* (*Impl)(PyObject* const*, Py_ssize_t, PyObject*)>
PyObject* entry_py(PyObject*, PyObject* const* args, Py_ssize_t nargs, PyObject* kwnames) {
    try {
        return Impl(args, nargs, kwnames);
    } catch (const PyErrSet&) {
        return nullptr;
    } catch (const c10::Error& e) {
        PyErr_SetString(PyExc_RuntimeError, e.what_without_backtrace());
        return nullptr;
    } catch (const std::exception& e) {
        PyErr_SetString(PyExc_RuntimeError, e.what());
        return nullptr;
    }
}

PyMethodDef kApplyDef = {
    "apply", reinterpret_cast<PyCFunction>(reinterpret_cast<void (*)(void)>(entry_py<apply_impl>)),
    METH_FASTCALL | METH_KEYWORDS,
    "U = LaplaceLearningSparseHard.apply(X, label_matrix, tau=0, epsilon='auto', k=25,\n"
    "                                    normalize=False, neighbors=None)\n"
    "(GLL.py:14; k: neighbours incl. self, the reference hard-codes 25; normalize=True: the rows\n"
    "of X are scaled to unit length first, as F.normalize(X, dim=1) does).  X, a floating-point\n"
    "label_matrix and tau / a fixed epsilon given as one-element tensors are differentiable\n"
    "(a tensor's value is read once in the forward: a host sync when it lives on the GPU).\n"
    "neighbors: an integer tensor n x k (the reference's knn_ind, column 0 = self) or n x (k - 1)\n"
    "(B x ... for batched X): the graph is built from these lists in the caller's order instead of\n"
    "a search, with no n x n distance buffer; ce_loss, margin_loss and objective take it too"};

PyMethodDef kCeLossDef = {
    "ce_loss", reinterpret_cast<PyCFunction>(reinterpret_cast<void (*)(void)>(entry_py<ce_loss_impl>)),
    METH_FASTCALL | METH_KEYWORDS,
    "loss, pred, pred_labels, row_loss, correct =\n"
    "    LaplaceLearningSparseHard.ce_loss(X, label_matrix, targets, tau=0, epsilon='auto', k=25,\n"
    "                                      normalize=False)\n"
    "apply followed by custom_ce_loss (losses.py:128-136) and the argmax accuracy\n"
    "(FullySup.py:156-171) with one extra kernel.  Only loss is differentiable (with respect to\n"
    "the inputs apply differentiates); a target outside [0, C) leaves its row out"};

PyMethodDef kMarginLossDef = {
    "margin_loss",
    reinterpret_cast<PyCFunction>(reinterpret_cast<void (*)(void)>(entry_py<margin_loss_impl>)),
    METH_FASTCALL | METH_KEYWORDS,
    "loss, pred, labels, second, row_margin, moved =\n"
    "    LaplaceLearningSparseHard.margin_loss(X, label_matrix, other, tau=0, epsilon='auto', k=25,\n"
    "                                          normalize=False)\n"
    "apply followed by the Carlini-Wagner margin (adversarial.py:688-751) with one extra kernel:\n"
    "the best and second-best class of every row, row_margin = clamp(max - pred[i, other_i], 0),\n"
    "loss = row_margin.sum() / m and moved = #{labels == other}.  Only loss is differentiable (with\n"
    "respect to the inputs apply differentiates); an other_i outside [0, C) leaves its row out and\n"
    "other=None leaves every row out (the top-2 query alone)"};

PyMethodDef kObjectiveDef = {
    "objective",
    reinterpret_cast<PyCFunction>(reinterpret_cast<void (*)(void)>(entry_py<objective_impl>)),
    METH_FASTCALL | METH_KEYWORDS,
    "loss, pred, pred_labels, row_loss, correct, row_entropy, row_l2 =\n"
    "    LaplaceLearningSparseHard.objective(X, label_matrix, targets, tau=0, epsilon='auto', k=25,\n"
    "                                        normalize=False, weights=(1.0, 0.0, 0.0),\n"
    "                                        score=None, score_out=None, indices=None)\n"
    "apply followed by the head of a score-driven training step (FullySup.py:156-175) with one\n"
    "extra kernel: loss = (w_ce sum(ce) + w_ent sum(entropy) - w_l2 sum(pred^2)) / m for weights =\n"
    "(w_ce, w_ent, w_l2) (losses.py:128-136, :100-101, :111-112), row_l2 = 1 - sum(pred^2, 1), and\n"
    "score_out[indices] = row_loss ('entropy') or row_l2 ('l2') as float32, written in place.  Only\n"
    "loss is differentiable; a target outside [0, C) leaves its row out of the ce term, of correct\n"
    "and of the scatter, targets=None leaves every row out; an index outside score_out is skipped"};

// ------------------------------------------------------------------------------------------
// status API for the Python layer
// ------------------------------------------------------------------------------------------
template <typename F>
void with_py_errors(F f) {
    try {
        f();
    } catch (const PyErrSet&) {
        throw pybind11::error_already_set();
    }
}

}  // namespace

PYBIND11_MODULE(_gll_torch, m) {
    m.doc() = "LaplaceLearningSparseHard.apply over libgll.so (include/gll.h) and its status sink";
    m.add_object("apply", pybind11::reinterpret_steal<pybind11::object>(
                              PyCFunction_NewEx(&kApplyDef, nullptr, m.attr("__name__").ptr())));
    m.add_object("ce_loss", pybind11::reinterpret_steal<pybind11::object>(
                                PyCFunction_NewEx(&kCeLossDef, nullptr, m.attr("__name__").ptr())));
    m.add_object("margin_loss",
                 pybind11::reinterpret_steal<pybind11::object>(
                     PyCFunction_NewEx(&kMarginLossDef, nullptr, m.attr("__name__").ptr())));
    m.add_object("objective",
                 pybind11::reinterpret_steal<pybind11::object>(
                     PyCFunction_NewEx(&kObjectiveDef, nullptr, m.attr("__name__").ptr())));
    m.def("status_sink",[](int dev) { return int64_t(status_of(dev).sink.data_ptr()); },
          "device address of the sticky status words of device `dev` (gll_problem.status_sink)");
    m.def("note_call", [](int dev) {
              with_py_errors([&] {
                  DeviceStatus& s = status_of(dev);
                  c10::DeviceGuard g(c10::Device(c10::kCUDA, dev));
                  if (!s.order.empty()) poll(s, false);
                  after_call(s, dev, current_stream(dev));
              });
          },
          "count one call that used the sink (Python Function path)");
    m.def("poll_status", [](int dev) {
              with_py_errors([&] {
                  DeviceStatus& s = status_of(dev);
                  if (!s.order.empty()) poll(s, false);
              });
          },
          "raise the warnings of completed status copies of device `dev`");
    m.def("check_status", []() {
              with_py_errors([&] {
                  std::vector<int> devs;
                  {
                      std::lock_guard<std::mutex> lk(g_status_mu);
                      for (int q = 0; q < int(g_status.size()); ++q)
                          if (g_status[q]) devs.push_back(q);
                  }
                  for (int dv : devs) {
                      DeviceStatus& s = status_of(dv);
                      c10::DeviceGuard g(c10::Device(c10::kCUDA, dv));
                      flush(s, dv, current_stream(dv));
                      poll(s, true);
                  }
              });
          },
          "flush every device's status sink now and raise the pending warnings (synchronises)");
    m.def("set_grad_diagnostics", [](double thr) { g_grad_diag = thr; },
          "exploding-gradient report threshold for calls made from now on (< 0: off)");
}
