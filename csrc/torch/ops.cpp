// Torch op registrations: every MI355X kernel of libpcmx_hip.so is exposed as torch.ops.pcmx.<name>.
// GPU tensors dispatch here (DispatchKey "CUDA" is the HIP device on ROCm builds of PyTorch); kernels
// run on the current torch HIP stream so they compose with torch.distributed (RCCL) streams and hipGraph
// capture. Workspaces come from the torch caching allocator (no hipMalloc on the launch path).
#include <cmath>
#include <map>
#include <mutex>
#include <torch/extension.h>
#include <torch/library.h>
#include <c10/hip/HIPStream.h>
#include <c10/core/DeviceGuard.h>

#include "pcmx_hip.h"

namespace {

hipStream_t cur_stream(const at::Tensor& t) {
    return c10::hip::getCurrentHIPStream(t.device().index()).stream();
}

void check_rc(int rc, const char* what) {
    TORCH_CHECK(rc == 0, "pcmx::", what, " failed: ", pcmx_error_string(rc), " (", rc, ")");
}

void check_gpu(const at::Tensor& t, const char* name, at::ScalarType dt) {
    TORCH_CHECK(t.is_cuda(), name, " must be a GPU tensor");
    TORCH_CHECK(t.scalar_type() == dt, name, " has dtype ", t.scalar_type(), ", expected ", dt);
}

at::Tensor aligned_contig(const at::Tensor& t) {
    at::Tensor c = t.contiguous();
    if (reinterpret_cast<uintptr_t>(c.data_ptr()) & 15u) c = c.clone();
    return c;
}

at::Tensor workspace(const at::Tensor& like, long long bytes) {
    return at::empty({std::max<long long>(bytes, 16)}, like.options().dtype(at::kByte));
}

// ---------------------------------------------------------------- element-wise
at::Tensor vmul(const at::Tensor& a, const at::Tensor& b) {
    check_gpu(a, "a", at::kFloat), check_gpu(b, "b", at::kFloat);
    TORCH_CHECK(a.numel() == b.numel(), "vmul: size mismatch");
    const at::DeviceGuard g(a.device());
    auto ac = aligned_contig(a), bc = aligned_contig(b);
    auto r = at::empty_like(ac);
    check_rc(pcmx_vmul_f32(ac.data_ptr<float>(), bc.data_ptr<float>(), r.data_ptr<float>(), ac.numel(), cur_stream(a)), "vmul");
    return r;
}

at::Tensor vadd(const at::Tensor& a, const at::Tensor& b) {
    check_gpu(a, "a", at::kFloat), check_gpu(b, "b", at::kFloat);
    TORCH_CHECK(a.numel() == b.numel(), "vadd: size mismatch");
    const at::DeviceGuard g(a.device());
    auto ac = aligned_contig(a), bc = aligned_contig(b);
    auto r = at::empty_like(ac);
    check_rc(pcmx_vadd_f32(ac.data_ptr<float>(), bc.data_ptr<float>(), r.data_ptr<float>(), ac.numel(), cur_stream(a)), "vadd");
    return r;
}

at::Tensor gather_(const at::Tensor& src, const at::Tensor& idx, at::Tensor out) {
    check_gpu(src, "src", at::kFloat), check_gpu(idx, "idx", at::kInt), check_gpu(out, "out", at::kFloat);
    TORCH_CHECK(src.is_contiguous() && idx.is_contiguous() && out.is_contiguous() && idx.numel() == out.numel(),
                "gather_: contiguous src / idx / out, out.numel() == idx.numel()");
    TORCH_CHECK((reinterpret_cast<uintptr_t>(idx.data_ptr()) & 15u) == 0 && (reinterpret_cast<uintptr_t>(out.data_ptr()) & 15u) == 0,
                "gather_: idx and out must be 16-B aligned");
    const at::DeviceGuard g(src.device());
    check_rc(pcmx_gather_f32(src.data_ptr<float>(), src.numel(), idx.data_ptr<int>(), out.data_ptr<float>(), out.numel(),
                             cur_stream(src)),
             "gather_");
    return out;
}

// The streaming kernels take their tiles in any order: an input that PARTLY overlaps the output is copied out first
// (an input identical to the output, element for element, is fine: each element is read before it is written).
at::Tensor unaliased(const at::Tensor& in, const at::Tensor& out) {
    const auto i0 = reinterpret_cast<uintptr_t>(in.data_ptr()), o0 = reinterpret_cast<uintptr_t>(out.data_ptr());
    const uintptr_t ib = (uintptr_t)in.numel() * in.element_size(), ob = (uintptr_t)out.numel() * out.element_size();
    return (i0 != o0 && i0 < o0 + ob && o0 < i0 + ib) ? in.clone() : in;
}

at::Tensor axpy_(at::Tensor y, double alpha, const at::Tensor& x) {
    check_gpu(y, "y", at::kFloat), check_gpu(x, "x", at::kFloat);
    TORCH_CHECK(y.is_contiguous() && (reinterpret_cast<uintptr_t>(y.data_ptr()) & 15u) == 0, "axpy_: y must be contiguous, 16-B aligned");
    TORCH_CHECK(x.numel() == y.numel(), "axpy_: size mismatch");
    const at::DeviceGuard g(y.device());
    auto xc = unaliased(aligned_contig(x), y);
    check_rc(pcmx_axpy_f32((float)alpha, xc.data_ptr<float>(), y.data_ptr<float>(), y.numel(), cur_stream(y)), "axpy_");
    return y;
}

at::Tensor copy_(at::Tensor dst, const at::Tensor& src) {
    check_gpu(dst, "dst", at::kFloat), check_gpu(src, "src", at::kFloat);
    TORCH_CHECK(dst.is_contiguous() && (reinterpret_cast<uintptr_t>(dst.data_ptr()) & 15u) == 0, "copy_: dst must be contiguous, 16-B aligned");
    TORCH_CHECK(src.numel() == dst.numel() && src.device() == dst.device(), "copy_: size / device mismatch");
    const at::DeviceGuard g(dst.device());
    auto sc = unaliased(aligned_contig(src), dst);  // memmove semantics
    check_rc(pcmx_copy_f32(sc.data_ptr<float>(), dst.data_ptr<float>(), dst.numel(), cur_stream(dst)), "copy_");
    return dst;
}

at::Tensor fill_(at::Tensor x, double v) {
    check_gpu(x, "x", at::kFloat);
    TORCH_CHECK(x.is_contiguous() && (reinterpret_cast<uintptr_t>(x.data_ptr()) & 15u) == 0, "fill_: contiguous, aligned");
    const at::DeviceGuard g(x.device());
    check_rc(pcmx_fill_f32(x.data_ptr<float>(), (float)v, x.numel(), cur_stream(x)), "fill_");
    return x;
}

at::Tensor rand_uniform_(at::Tensor x, int64_t seed, double lo, double hi) {
    check_gpu(x, "x", at::kFloat);
    TORCH_CHECK(x.is_contiguous(), "rand_uniform_: contiguous");
    const at::DeviceGuard g(x.device());
    check_rc(pcmx_rand_uniform_f32(x.data_ptr<float>(), x.numel(), (unsigned long long)seed, (float)lo, (float)hi, cur_stream(x)),
             "rand_uniform_");
    return x;
}

// ---------------------------------------------------------------- reductions / scan
at::Tensor reduce(const at::Tensor& x, int64_t op) {
    TORCH_CHECK(x.is_cuda(), "reduce: GPU tensor expected");
    const at::DeviceGuard g(x.device());
    auto xc = aligned_contig(x);
    auto ws = workspace(x, pcmx_reduce_workspace_bytes(xc.numel()));
    if (x.scalar_type() == at::kFloat) {
        auto out = at::empty({}, x.options());
        check_rc(pcmx_reduce_f32(xc.data_ptr<float>(), xc.numel(), (int)op, out.data_ptr<float>(), ws.data_ptr(), cur_stream(x)), "reduce");
        return out;
    }
    TORCH_CHECK(x.scalar_type() == at::kInt, "reduce: float32 or int32 expected");
    auto out = at::empty({}, x.options());
    check_rc(pcmx_reduce_i32(xc.data_ptr<int32_t>(), xc.numel(), (int)op, out.data_ptr<int32_t>(), ws.data_ptr(), cur_stream(x)), "reduce");
    return out;
}

at::Tensor dot(const at::Tensor& a, const at::Tensor& b) {
    check_gpu(a, "a", at::kFloat), check_gpu(b, "b", at::kFloat);
    TORCH_CHECK(a.numel() == b.numel(), "dot: size mismatch");
    const at::DeviceGuard g(a.device());
    auto ac = aligned_contig(a), bc = aligned_contig(b);
    auto ws = workspace(a, pcmx_reduce_workspace_bytes(ac.numel()));
    auto out = at::empty({}, a.options());
    check_rc(pcmx_dot_f32(ac.data_ptr<float>(), bc.data_ptr<float>(), ac.numel(), out.data_ptr<float>(), ws.data_ptr(), cur_stream(a)), "dot");
    return out;
}

// Sticky look-back-timeout word per (device, stream) in host-mapped pinned memory: a scan kernel whose look-back
// gives up ORs 1 into it (system-scope atomic), so the host sees it without a copy. scan_check (and
// ops.scan(check=True)) synchronises THAT stream and raises; the next scan on the same stream raises too. One word
// per stream, so a failed scan on one stream is never reported (and cleared) by an unrelated call on another.
struct ScanErrWord {
    unsigned* host = nullptr;
    unsigned* dev = nullptr;
};

ScanErrWord& scan_err_word(int dev, hipStream_t stream) {
    static std::mutex mu;
    static std::map<std::pair<int, hipStream_t>, ScanErrWord> words;
    TORCH_CHECK(dev >= 0, "scan: device index");
    std::lock_guard<std::mutex> lock(mu);
    ScanErrWord& w = words[{dev, stream}];
    if (!w.host) {
        void* p = nullptr;
        TORCH_CHECK(hipHostMalloc(&p, 64, hipHostMallocMapped | hipHostMallocCoherent) == hipSuccess,
                    "scan: pinned error word");
        *static_cast<volatile unsigned*>(p) = 0u;
        void* d = nullptr;
        TORCH_CHECK(hipHostGetDevicePointer(&d, p, 0) == hipSuccess, "scan: mapped error word");
        w.host = static_cast<unsigned*>(p), w.dev = static_cast<unsigned*>(d);
    }
    return w;
}

void raise_pending_scan_error(int dev, hipStream_t stream) {
    volatile unsigned* w = scan_err_word(dev, stream).host;
    if (*w) {
        *w = 0u;
        TORCH_CHECK(false, "pcmx::scan: a scan on device ", dev, " (this stream) timed out in its decoupled look-back ",
                    "(a predecessor tile never published); that result is invalid");
    }
}

// Waits for the current stream of `device` and raises if any scan issued on it gave up a look-back.
void scan_check(int64_t device) {
    const at::Device d(at::kCUDA, (c10::DeviceIndex)device);
    const at::DeviceGuard g(d);
    hipStream_t s = c10::hip::getCurrentHIPStream(d.index()).stream();
    TORCH_CHECK(hipStreamSynchronize(s) == hipSuccess, "scan_check: stream synchronize");
    raise_pending_scan_error((int)device, s);
}

at::Tensor scan_out(const at::Tensor& x, at::Tensor out, bool exclusive, const c10::optional<at::Tensor>& init) {
    check_gpu(x, "x", at::kFloat), check_gpu(out, "out", at::kFloat);
    TORCH_CHECK(x.is_contiguous() && out.is_contiguous() && x.numel() == out.numel(), "scan: contiguous same-size tensors");
    TORCH_CHECK(out.device() == x.device(), "scan: out must be on x's device");
    const at::DeviceGuard g(x.device());
    hipStream_t stream = cur_stream(x);
    unsigned* err_dev = scan_err_word(x.device().index(), stream).dev;
    raise_pending_scan_error(x.device().index(), stream);
    const float* init_ptr = nullptr;
    at::Tensor init_c;
    if (init.has_value() && init->defined()) {
        check_gpu(*init, "init", at::kFloat);
        TORCH_CHECK(init->numel() >= 1 && init->device() == x.device(), "scan: init needs >= 1 element on x's device");
        init_c = init->contiguous();
        init_ptr = init_c.data_ptr<float>();
    }
    at::Tensor xc = x, oc = out;
    if ((reinterpret_cast<uintptr_t>(x.data_ptr()) & 15u) || (reinterpret_cast<uintptr_t>(out.data_ptr()) & 15u)) {
        xc = x.clone();
        oc = at::empty_like(xc);
    }
    auto ws = workspace(x, pcmx_scan_workspace_bytes(xc.numel()));
    check_rc(pcmx_scan_f32(xc.data_ptr<float>(), oc.data_ptr<float>(), xc.numel(), exclusive ? 1 : 0, init_ptr, ws.data_ptr(),
                           err_dev, stream),
             "scan");
    if (!oc.is_same(out)) out.copy_(oc);
    return out;
}

at::Tensor scan(const at::Tensor& x, bool exclusive, const c10::optional<at::Tensor>& init) {
    auto xc = aligned_contig(x).view(-1);
    auto out = at::empty_like(xc);
    return scan_out(xc, out, exclusive, init).view(x.sizes());
}

// ---------------------------------------------------------------- stream compaction (select / nonzero)
// The three select ops return (out, count): out has room for x.numel() elements (the count is not known on the host),
// count is a 0-d int64 tensor on the device; nothing synchronises. They share the scan's per-(device, stream) sticky
// error word, so scan_check() covers a select whose look-back gave up.
bool overlaps(const at::Tensor& a, const at::Tensor& b) {
    const auto a0 = reinterpret_cast<uintptr_t>(a.data_ptr()), b0 = reinterpret_cast<uintptr_t>(b.data_ptr());
    const uintptr_t ab = (uintptr_t)a.numel() * a.element_size(), bb = (uintptr_t)b.numel() * b.element_size();
    return a0 < b0 + bb && b0 < a0 + ab;
}

// The flag bytes of a bool / uint8 mask, contiguous and 4-B aligned.
at::Tensor mask_bytes(const at::Tensor& mask, int64_t n, const char* what) {
    TORCH_CHECK(mask.is_cuda(), what, ": mask must be a GPU tensor");
    TORCH_CHECK(mask.scalar_type() == at::kBool || mask.scalar_type() == at::kByte, what, ": mask has dtype ",
                mask.scalar_type(), ", expected bool or uint8");
    TORCH_CHECK(mask.numel() == n, what, ": mask has ", mask.numel(), " elements, expected ", n);
    at::Tensor m = mask.contiguous().view(-1);
    if (m.scalar_type() == at::kBool) m = m.view(at::kByte);
    if (reinterpret_cast<uintptr_t>(m.data_ptr()) & 3u) m = m.clone();
    return m;
}

// The tensor the kernel writes (16-B aligned): `out` itself, a copy of it (so what lies past the count survives the
// copy back) when it is misaligned, or a fresh one of n elements.
at::Tensor select_dest(const c10::optional<at::Tensor>& out, const at::Tensor& like, at::ScalarType dt, int64_t n,
                       const char* what) {
    if (!(out.has_value() && out->defined())) return at::empty({n}, like.options().dtype(dt));
    check_gpu(*out, "out", dt);
    TORCH_CHECK(out->device() == like.device() && out->is_contiguous() && out->numel() >= n, what,
                ": out must be contiguous, on the input's device, with room for all ", n, " elements");
    return (reinterpret_cast<uintptr_t>(out->data_ptr()) & 15u) ? out->clone() : *out;
}

std::tuple<at::Tensor, at::Tensor> select_finish(const c10::optional<at::Tensor>& out, const at::Tensor& dest,
                                                 const at::Tensor& count) {
    if (out.has_value() && out->defined()) {
        if (!dest.is_same(*out)) out->copy_(dest);
        return {*out, count};
    }
    return {dest, count};
}

std::tuple<at::Tensor, at::Tensor> select_b32(const at::Tensor& x, const at::Tensor& mask, const c10::optional<at::Tensor>& out) {
    TORCH_CHECK(x.is_cuda(), "select: x must be a GPU tensor");
    TORCH_CHECK(x.scalar_type() == at::kFloat || x.scalar_type() == at::kInt, "select: x has dtype ", x.scalar_type(),
                ", expected float32 or int32");
    TORCH_CHECK(mask.device() == x.device(), "select: mask must be on x's device");
    const at::DeviceGuard g(x.device());
    hipStream_t stream = cur_stream(x);
    unsigned* err_dev = scan_err_word(x.device().index(), stream).dev;
    raise_pending_scan_error(x.device().index(), stream);
    const int64_t n = x.numel();
    at::Tensor xc = aligned_contig(x).view(-1), mc = mask_bytes(mask, n, "select");
    at::Tensor dest = select_dest(out, x, x.scalar_type(), n, "select");
    if (overlaps(xc, dest)) xc = xc.clone();
    if (overlaps(mc, dest)) mc = mc.clone();
    at::Tensor count = at::empty({}, x.options().dtype(at::kLong));
    auto ws = workspace(x, pcmx_select_workspace_bytes(n));
    check_rc(pcmx_select_b32(xc.data_ptr(), mc.data_ptr<uint8_t>(), dest.data_ptr(), n, (long long*)count.data_ptr<int64_t>(),
                             ws.data_ptr(), err_dev, stream),
             "select");
    return select_finish(out, dest, count);
}

std::tuple<at::Tensor, at::Tensor> select_index(const at::Tensor& mask, const c10::optional<at::Tensor>& out) {
    const at::DeviceGuard g(mask.device());
    const int64_t n = mask.numel();
    at::Tensor mc = mask_bytes(mask, n, "select_index");
    hipStream_t stream = cur_stream(mask);
    unsigned* err_dev = scan_err_word(mask.device().index(), stream).dev;
    raise_pending_scan_error(mask.device().index(), stream);
    at::Tensor dest = select_dest(out, mask, at::kInt, n, "select_index");
    if (overlaps(mc, dest)) mc = mc.clone();
    at::Tensor count = at::empty({}, mask.options().dtype(at::kLong));
    auto ws = workspace(mask, pcmx_select_workspace_bytes(n));
    check_rc(pcmx_select_index(mc.data_ptr<uint8_t>(), dest.data_ptr<int>(), n, (long long*)count.data_ptr<int64_t>(),
                               ws.data_ptr(), err_dev, stream),
             "select_index");
    return select_finish(out, dest, count);
}

std::tuple<at::Tensor, at::Tensor> select_if(const at::Tensor& x, int64_t op, double threshold, bool indices,
                                             const c10::optional<at::Tensor>& out) {
    check_gpu(x, "x", at::kFloat);
    TORCH_CHECK(op >= PCMX_CMP_GT && op <= PCMX_CMP_NE, "select_if: op code ", op);
    const at::DeviceGuard g(x.device());
    hipStream_t stream = cur_stream(x);
    unsigned* err_dev = scan_err_word(x.device().index(), stream).dev;
    raise_pending_scan_error(x.device().index(), stream);
    const int64_t n = x.numel();
    at::Tensor xc = aligned_contig(x).view(-1);
    at::Tensor dest = select_dest(out, x, indices ? at::kInt : at::kFloat, n, "select_if");
    if (overlaps(xc, dest)) xc = xc.clone();
    at::Tensor count = at::empty({}, x.options().dtype(at::kLong));
    auto ws = workspace(x, pcmx_select_workspace_bytes(n));
    check_rc(pcmx_select_if_f32(xc.data_ptr<float>(), (int)op, (float)threshold, dest.data_ptr(), indices ? 1 : 0, n,
                                (long long*)count.data_ptr<int64_t>(), ws.data_ptr(), err_dev, stream),
             "select_if");
    return select_finish(out, dest, count);
}

// ---------------------------------------------------------------- radix sort (keys, pairs, argsort)
// Stable LSD radix sort of float32 / int32 keys by bits [begin_bit, end_bit) of the transformed key (pcmx_hip.h), sorted
// as flattened 1-D; fresh 1-D outputs, the inputs are never written. Like the select ops: contiguous 16-B aligned inputs
// (copied when they are not), workspace from the caching allocator, the per-(device, stream) sticky error word (so
// scan_check() covers a sort whose look-back gave up), no host synchronisation.
int sort_key_type(const at::Tensor& keys, const char* what) {
    TORCH_CHECK(keys.is_cuda(), what, ": keys must be a GPU tensor");
    TORCH_CHECK(keys.scalar_type() == at::kFloat || keys.scalar_type() == at::kInt, what, ": keys have dtype ",
                keys.scalar_type(), ", expected float32 or int32");
    return keys.scalar_type() == at::kFloat ? PCMX_KEY_F32 : PCMX_KEY_I32;
}

void sort_launch(const at::Tensor& keys, const at::Tensor* values, at::Tensor* keys_out, at::Tensor* vals_out, int mode,
                 bool descending, int64_t begin_bit, int64_t end_bit, const char* what) {
    const int key_type = sort_key_type(keys, what);
    TORCH_CHECK(0 <= begin_bit && begin_bit < end_bit && end_bit <= 32, what, ": bit range [", begin_bit, ", ", end_bit, ")");
    const int64_t n = keys.numel();
    TORCH_CHECK(n < (1LL << 30), what, ": indices and granule counts are 30-bit, the keys must have fewer than 2^30 elements");
    hipStream_t stream = cur_stream(keys);
    unsigned* err_dev = scan_err_word(keys.device().index(), stream).dev;
    raise_pending_scan_error(keys.device().index(), stream);
    if (n == 0) return;
    at::Tensor kc = aligned_contig(keys).view(-1), vc;
    if (values) vc = aligned_contig(*values).view(-1);
    auto ws = workspace(keys, pcmx_sort_workspace_bytes(n, mode));
    check_rc(pcmx_radix_sort(kc.data_ptr(), keys_out ? keys_out->data_ptr() : nullptr, values ? vc.data_ptr() : nullptr,
                             vals_out ? vals_out->data_ptr() : nullptr, n, key_type, mode, descending ? 1 : 0,
                             (int)begin_bit, (int)end_bit, ws.data_ptr(), err_dev, stream),
             what);
}

at::Tensor sort_keys(const at::Tensor& keys, bool descending, int64_t begin_bit, int64_t end_bit) {
    sort_key_type(keys, "sort_keys");
    const at::DeviceGuard g(keys.device());
    at::Tensor out = at::empty({keys.numel()}, keys.options());
    sort_launch(keys, nullptr, &out, nullptr, PCMX_SORT_KEYS, descending, begin_bit, end_bit, "sort_keys");
    return out;
}

std::tuple<at::Tensor, at::Tensor> sort_pairs(const at::Tensor& keys, const at::Tensor& values, bool descending,
                                              int64_t begin_bit, int64_t end_bit) {
    sort_key_type(keys, "sort_pairs");
    TORCH_CHECK(values.device() == keys.device(), "sort_pairs: values must be on the keys' device");
    TORCH_CHECK(values.scalar_type() == at::kFloat || values.scalar_type() == at::kInt, "sort_pairs: values have dtype ",
                values.scalar_type(), ", expected float32 or int32");
    TORCH_CHECK(values.numel() == keys.numel(), "sort_pairs: ", values.numel(), " values for ", keys.numel(), " keys");
    const at::DeviceGuard g(keys.device());
    at::Tensor ko = at::empty({keys.numel()}, keys.options()), vo = at::empty({keys.numel()}, values.options());
    sort_launch(keys, &values, &ko, &vo, PCMX_SORT_PAIRS, descending, begin_bit, end_bit, "sort_pairs");
    return {ko, vo};
}

// (sorted keys, int32 indices); with want_keys false the first tensor is empty and no sorted keys are written
std::tuple<at::Tensor, at::Tensor> sort_index(const at::Tensor& keys, bool descending, int64_t begin_bit, int64_t end_bit,
                                              bool want_keys) {
    sort_key_type(keys, "sort_index");
    const at::DeviceGuard g(keys.device());
    at::Tensor ko = at::empty({want_keys ? keys.numel() : 0}, keys.options());
    at::Tensor io = at::empty({keys.numel()}, keys.options().dtype(at::kInt));
    sort_launch(keys, nullptr, want_keys ? &ko : nullptr, &io, PCMX_SORT_INDEX, descending, begin_bit, end_bit, "sort_index");
    return {ko, io};
}

// ---------------------------------------------------------------- top-k / k-th value (radix select)
// The first k entries of the stable sort of the flattened keys (descending = largest) without sorting them: four
// histogram passes find the k-th key, one look-back pass gathers the k survivors, a pair sort orders them
// (csrc/kernels/topk.hip). Like sort_launch: contiguous 16-B aligned input (copied when it is not), workspace from the
// caching allocator, the per-(device, stream) sticky error word, no host synchronisation.
std::tuple<at::Tensor, at::Tensor> topk(const at::Tensor& x, int64_t k, bool largest, bool sorted) {
    const int key_type = sort_key_type(x, "topk");
    const int64_t n = x.numel();
    TORCH_CHECK(n < (1LL << 30), "topk: the keys must have fewer than 2^30 elements");
    TORCH_CHECK(0 <= k && k <= n, "topk: k = ", k, " for ", n, " elements");
    const at::DeviceGuard g(x.device());
    hipStream_t stream = cur_stream(x);
    unsigned* err_dev = scan_err_word(x.device().index(), stream).dev;
    raise_pending_scan_error(x.device().index(), stream);
    at::Tensor vals = at::empty({k}, x.options()), idx = at::empty({k}, x.options().dtype(at::kInt));
    if (k == 0) return {vals, idx};
    at::Tensor xc = aligned_contig(x).view(-1);
    auto ws = workspace(x, pcmx_topk_workspace_bytes(n, k, sorted ? 1 : 0));
    check_rc(pcmx_topk_b32(xc.data_ptr(), n, k, key_type, largest ? 1 : 0, sorted ? 1 : 0, vals.data_ptr(), idx.data_ptr(),
                           ws.data_ptr(), err_dev, stream),
             "topk");
    return {vals, idx};
}

// the k-th key (1-based) as a 0-d tensor: the histogram passes alone
at::Tensor kth_value(const at::Tensor& x, int64_t k, bool largest) {
    const int key_type = sort_key_type(x, "kth_value");
    const int64_t n = x.numel();
    TORCH_CHECK(n < (1LL << 30), "kth_value: the keys must have fewer than 2^30 elements");
    TORCH_CHECK(1 <= k && k <= n, "kth_value: k = ", k, " for ", n, " elements");
    const at::DeviceGuard g(x.device());
    hipStream_t stream = cur_stream(x);
    unsigned* err_dev = scan_err_word(x.device().index(), stream).dev;
    raise_pending_scan_error(x.device().index(), stream);
    at::Tensor out = at::empty({}, x.options());
    at::Tensor xc = aligned_contig(x).view(-1);
    auto ws = workspace(x, pcmx_topk_workspace_bytes(n, k, 0));
    check_rc(pcmx_kth_key_b32(xc.data_ptr(), n, k, key_type, largest ? 1 : 0, out.data_ptr(), ws.data_ptr(), err_dev, stream),
             "kth_value");
    return out;
}

// ---------------------------------------------------------------- row-wise sort / top-k / k-th value
// The same operations on every row of a 2-D [rows, cols] tensor, one wave or one block per row (csrc/kernels/
// rowsort.hip): no workspace, no error word, no host synchronisation. Sizes, modes and routes are checked by the C entry
// points (PCMX_ERR_ARG raises here); contiguous 16-B aligned inputs (copied when they are not), fresh outputs.
at::Tensor row_input(const at::Tensor& x, const char* what) {
    sort_key_type(x, what);
    TORCH_CHECK(x.dim() == 2, what, ": expected a 2-D [rows, cols] tensor, got ", x.dim(), " dimensions");
    return aligned_contig(x);
}

// (sorted keys [rows, keep], values or int32 positions [rows, keep]); mode: PCMX_SORT_* | PCMX_ROWSORT_* (a forced
// kernel); with want_keys false (INDEX mode) the first tensor is empty and no keys are written
std::tuple<at::Tensor, at::Tensor> row_sort(const at::Tensor& keys, const c10::optional<at::Tensor>& values, int64_t keep,
                                            int64_t mode, bool descending, int64_t begin_bit, int64_t end_bit,
                                            bool want_keys) {
    const int key_type = sort_key_type(keys, "row_sort");
    const at::DeviceGuard g(keys.device());
    at::Tensor kc = row_input(keys, "row_sort"), vc;
    const int64_t rows = kc.size(0), cols = kc.size(1), base_mode = mode & 0xff;
    TORCH_CHECK(keep >= 0, "row_sort: keep = ", keep);
    if (values.has_value()) {
        TORCH_CHECK(values->device() == keys.device(), "row_sort: values must be on the keys' device");
        TORCH_CHECK(values->scalar_type() == at::kFloat || values->scalar_type() == at::kInt, "row_sort: values have dtype ",
                    values->scalar_type(), ", expected float32 or int32");
        TORCH_CHECK(values->sizes() == keys.sizes(), "row_sort: values must have the shape of keys");
        vc = aligned_contig(*values);
    }
    TORCH_CHECK(values.has_value() == (base_mode == PCMX_SORT_PAIRS), "row_sort: values go with PCMX_SORT_PAIRS and only with it");
    at::Tensor ko = at::empty({want_keys ? rows : 0, want_keys ? keep : 0}, keys.options()), vo;
    if (base_mode == PCMX_SORT_PAIRS) vo = at::empty({rows, keep}, values->options());
    else if (base_mode == PCMX_SORT_INDEX) vo = at::empty({rows, keep}, keys.options().dtype(at::kInt));
    else vo = at::empty({0, 0}, keys.options().dtype(at::kInt));
    if (keep <= cols && (rows == 0 || cols == 0 || keep == 0)) return {ko, vo};  // empty tensors have no base pointer
    check_rc(pcmx_row_sort_b32(kc.data_ptr(), want_keys ? ko.data_ptr() : nullptr, values.has_value() ? vc.data_ptr() : nullptr,
                               base_mode == PCMX_SORT_KEYS ? nullptr : vo.data_ptr(), rows, cols, keep, key_type, (int)mode,
                               descending ? 1 : 0, (int)begin_bit, (int)end_bit, cur_stream(keys)),
             "row_sort");
    return {ko, vo};
}

// the k survivors of every row in ascending position: (canonical values [rows, k], int32 positions [rows, k])
std::tuple<at::Tensor, at::Tensor> row_topk(const at::Tensor& x, int64_t k, bool largest) {
    const int key_type = sort_key_type(x, "row_topk");
    const at::DeviceGuard g(x.device());
    at::Tensor xc = row_input(x, "row_topk");
    TORCH_CHECK(k >= 0, "row_topk: k = ", k);
    at::Tensor vals = at::empty({xc.size(0), k}, x.options()), idx = at::empty({xc.size(0), k}, x.options().dtype(at::kInt));
    if (k <= xc.size(1) && (xc.numel() == 0 || k == 0)) return {vals, idx};  // empty tensors have no base pointer
    check_rc(pcmx_row_topk_b32(xc.data_ptr(), xc.size(0), xc.size(1), k, key_type, largest ? 1 : 0, vals.data_ptr(),
                               idx.data_ptr(), cur_stream(x)),
             "row_topk");
    return {vals, idx};
}

// the k-th key (1-based) of every row, [rows]
at::Tensor row_kth(const at::Tensor& x, int64_t k, bool largest) {
    const int key_type = sort_key_type(x, "row_kth");
    const at::DeviceGuard g(x.device());
    at::Tensor xc = row_input(x, "row_kth");
    TORCH_CHECK(k >= 1, "row_kth: k = ", k);
    at::Tensor out = at::empty({xc.size(0)}, x.options());
    if (xc.size(0) == 0) return out;
    check_rc(pcmx_row_kth_key_b32(xc.data_ptr(), xc.size(0), xc.size(1), k, key_type, largest ? 1 : 0, out.data_ptr(),
                                  cur_stream(x)),
             "row_kth");
    return out;
}

// ---------------------------------------------------------------- reduce / scan along a dimension
// x is the contiguous [outer, n, inner] view of the caller's tensor (csrc/kernels/axis.hip). Shapes, op, route and chunk
// are checked by the C entry points (PCMX_ERR_ARG raises here); the workspace comes from torch's allocator on the
// current stream; no error word, no host synchronisation.
at::Tensor axis_input(const at::Tensor& x, const char* what) {
    TORCH_CHECK(x.is_cuda(), what, ": GPU tensor expected");
    TORCH_CHECK(x.scalar_type() == at::kFloat || x.scalar_type() == at::kInt, what, ": x has dtype ", x.scalar_type(),
                ", expected float32 or int32");
    TORCH_CHECK(x.dim() == 3, what, ": expected a 3-D [outer, n, inner] tensor, got ", x.dim(), " dimensions");
    return aligned_contig(x);
}

// [outer, inner]
at::Tensor axis_reduce(const at::Tensor& x, int64_t op, int64_t route, int64_t chunk) {
    const at::DeviceGuard g(x.device());
    at::Tensor xc = axis_input(x, "axis_reduce");
    const int64_t outer = xc.size(0), n = xc.size(1), inner = xc.size(2);
    TORCH_CHECK(n > 0 || op == PCMX_OP_SUM, "axis_reduce: min / max of an empty dimension");
    if (n == 0) return at::zeros({outer, inner}, x.options());  // (an empty input has no base pointer)
    at::Tensor out = at::empty({outer, inner}, x.options());
    if (out.numel() == 0) return out;
    auto ws = workspace(x, pcmx_axis_workspace_bytes(outer, n, inner));
    if (x.scalar_type() == at::kFloat)
        check_rc(pcmx_axis_reduce_f32(xc.data_ptr<float>(), out.data_ptr<float>(), outer, n, inner, (int)op, (int)route, chunk,
                                      ws.data_ptr(), cur_stream(x)),
                 "axis_reduce");
    else
        check_rc(pcmx_axis_reduce_i32(xc.data_ptr<int32_t>(), out.data_ptr<int32_t>(), outer, n, inner, (int)op, (int)route,
                                      chunk, ws.data_ptr(), cur_stream(x)),
                 "axis_reduce");
    return out;
}

// [outer, n, inner]; out (contiguous, same numel and dtype) may be x itself
at::Tensor axis_scan(const at::Tensor& x, int64_t op, bool exclusive, int64_t route, int64_t chunk,
                     const c10::optional<at::Tensor>& out) {
    const at::DeviceGuard g(x.device());
    at::Tensor xc = axis_input(x, "axis_scan");
    const int64_t outer = xc.size(0), n = xc.size(1), inner = xc.size(2), total = xc.numel();
    const bool has_out = out.has_value() && out->defined();
    if (has_out) {
        check_gpu(*out, "out", x.scalar_type());
        TORCH_CHECK(out->device() == x.device() && out->is_contiguous() && out->numel() == total,
                    "axis_scan: out must be contiguous, on x's device, with ", total, " elements");
    }
    if (total == 0) return has_out ? *out : at::empty_like(xc);
    at::Tensor dest = has_out && !(reinterpret_cast<uintptr_t>(out->data_ptr()) & 15u) ? out->view({outer, n, inner})
                                                                                      : at::empty({outer, n, inner}, x.options());
    if (overlaps(xc, dest) && xc.data_ptr() != dest.data_ptr()) xc = xc.clone();  // identical is fine: the call is in place
    auto ws = workspace(x, pcmx_axis_workspace_bytes(outer, n, inner));
    if (x.scalar_type() == at::kFloat)
        check_rc(pcmx_axis_scan_f32(xc.data_ptr<float>(), dest.data_ptr<float>(), outer, n, inner, (int)op, exclusive ? 1 : 0,
                                    (int)route, chunk, ws.data_ptr(), cur_stream(x)),
                 "axis_scan");
    else
        check_rc(pcmx_axis_scan_i32(xc.data_ptr<int32_t>(), dest.data_ptr<int32_t>(), outer, n, inner, (int)op,
                                    exclusive ? 1 : 0, (int)route, chunk, ws.data_ptr(), cur_stream(x)),
                 "axis_scan");
    if (has_out) {
        if (dest.data_ptr() != out->data_ptr()) out->view(-1).copy_(dest.view(-1));
        return *out;
    }
    return dest;
}

// ---------------------------------------------------------------- run-length encode / reduce by key
// Runs of equal neighbouring keys (compared as bit patterns) of the flattened input, one pass on the scan's look-back
// (csrc/kernels/segreduce.hip). Like the select ops: per-run outputs have room for keys.numel() entries, the run count
// is a 0-d int64 tensor on the device, nothing synchronises, optional caller outputs are left untouched past the
// count, and the per-(device, stream) sticky error word is shared, so scan_check() covers these ops too.
struct SegPrep {
    at::Tensor keys;
    hipStream_t stream;
    unsigned* err_dev;
    int64_t n;
};

SegPrep seg_prepare(const at::Tensor& keys, const char* what) {
    sort_key_type(keys, what);
    TORCH_CHECK(keys.numel() < (1LL << 31), what, ": offsets are int32, the keys must have fewer than 2^31 elements");
    SegPrep p;
    p.stream = cur_stream(keys);
    p.err_dev = scan_err_word(keys.device().index(), p.stream).dev;
    raise_pending_scan_error(keys.device().index(), p.stream);
    p.n = keys.numel();
    p.keys = aligned_contig(keys).view(-1);
    return p;
}

// (run_keys, counts, starts, num_runs); starts is an empty tensor unless want_starts
std::tuple<at::Tensor, at::Tensor, at::Tensor, at::Tensor> run_length_encode(
    const at::Tensor& keys, bool want_starts, const c10::optional<at::Tensor>& out_keys,
    const c10::optional<at::Tensor>& out_counts, const c10::optional<at::Tensor>& out_starts) {
    const at::DeviceGuard g(keys.device());
    SegPrep p = seg_prepare(keys, "run_length_encode");
    at::Tensor dk = select_dest(out_keys, keys, keys.scalar_type(), p.n, "run_length_encode");
    at::Tensor dc = select_dest(out_counts, keys, at::kInt, p.n, "run_length_encode");
    at::Tensor ds = want_starts ? select_dest(out_starts, keys, at::kInt, p.n, "run_length_encode")
                                : at::empty({0}, keys.options().dtype(at::kInt));
    if (overlaps(p.keys, dk) || overlaps(p.keys, dc) || (want_starts && overlaps(p.keys, ds))) p.keys = p.keys.clone();
    at::Tensor count = at::empty({}, keys.options().dtype(at::kLong));
    auto ws = workspace(keys, pcmx_segreduce_workspace_bytes(p.n));
    check_rc(pcmx_run_length_encode_b32(p.keys.data_ptr(), p.n, dk.data_ptr(), dc.data_ptr<int>(),
                                        want_starts ? ds.data_ptr<int>() : nullptr, (long long*)count.data_ptr<int64_t>(),
                                        ws.data_ptr(), p.err_dev, p.stream),
             "run_length_encode");
    at::Tensor rk = std::get<0>(select_finish(out_keys, dk, count));
    at::Tensor rc = std::get<0>(select_finish(out_counts, dc, count));
    at::Tensor rs = want_starts ? std::get<0>(select_finish(out_starts, ds, count)) : ds;
    return {rk, rc, rs, count};
}

// (run_keys, aggregates, num_runs)
std::tuple<at::Tensor, at::Tensor, at::Tensor> reduce_by_key(const at::Tensor& keys, const at::Tensor& values, int64_t op,
                                                             const c10::optional<at::Tensor>& out_keys,
                                                             const c10::optional<at::Tensor>& out) {
    const at::DeviceGuard g(keys.device());
    SegPrep p = seg_prepare(keys, "reduce_by_key");
    TORCH_CHECK(op >= PCMX_OP_SUM && op <= PCMX_OP_MAX, "reduce_by_key: op code ", op);
    TORCH_CHECK(values.device() == keys.device(), "reduce_by_key: values must be on the keys' device");
    TORCH_CHECK(values.scalar_type() == at::kFloat || values.scalar_type() == at::kInt, "reduce_by_key: values have dtype ",
                values.scalar_type(), ", expected float32 or int32");
    TORCH_CHECK(values.numel() == p.n, "reduce_by_key: ", values.numel(), " values for ", p.n, " keys");
    at::Tensor vc = aligned_contig(values).view(-1);
    at::Tensor dk = select_dest(out_keys, keys, keys.scalar_type(), p.n, "reduce_by_key");
    at::Tensor da = select_dest(out, values, values.scalar_type(), p.n, "reduce_by_key");
    if (overlaps(p.keys, dk) || overlaps(p.keys, da)) p.keys = p.keys.clone();
    if (overlaps(vc, dk) || overlaps(vc, da)) vc = vc.clone();
    at::Tensor count = at::empty({}, keys.options().dtype(at::kLong));
    auto ws = workspace(keys, pcmx_segreduce_workspace_bytes(p.n));
    if (values.scalar_type() == at::kFloat)
        check_rc(pcmx_reduce_by_key_f32(p.keys.data_ptr(), vc.data_ptr<float>(), p.n, (int)op, dk.data_ptr(),
                                        da.data_ptr<float>(), (long long*)count.data_ptr<int64_t>(), ws.data_ptr(),
                                        p.err_dev, p.stream),
                 "reduce_by_key");
    else
        check_rc(pcmx_reduce_by_key_i32(p.keys.data_ptr(), vc.data_ptr<int32_t>(), p.n, (int)op, dk.data_ptr(),
                                        da.data_ptr<int32_t>(), (long long*)count.data_ptr<int64_t>(), ws.data_ptr(),
                                        p.err_dev, p.stream),
                 "reduce_by_key");
    at::Tensor rk = std::get<0>(select_finish(out_keys, dk, count));
    at::Tensor ra = std::get<0>(select_finish(out, da, count));
    return {rk, ra, count};
}

// ---------------------------------------------------------------- scan by key (segmented prefix scan)
// The running aggregate inside every run (csrc/kernels/scanbykey.hip): the result has the values' dtype and shape, the
// optional caller tensor `out` (contiguous, values.numel() elements) may be the values themselves (in place). Keys or
// head flags that overlap the output are cloned first, as reduce_by_key does. No block of these kernels waits for
// another one, so there is no error word to share and nothing synchronises.
bool same_elements(const at::Tensor& a, const at::Tensor& b) {
    return a.data_ptr() == b.data_ptr() && a.numel() == b.numel() && a.element_size() == b.element_size();
}

// runs: the flat, contiguous, aligned keys (PCMX_HEADS_FROM_KEYS) or flag bytes (PCMX_HEADS_FROM_FLAGS)
at::Tensor scan_by_key_launch(at::Tensor runs, int head_mode, const at::Tensor& values, int64_t op, bool exclusive,
                              const c10::optional<at::Tensor>& out, const char* what) {
    TORCH_CHECK(op >= PCMX_OP_SUM && op <= PCMX_OP_MAX, what, ": op code ", op);
    TORCH_CHECK(values.is_cuda() && values.device() == runs.device(), what, ": values must be on the device of the keys or heads");
    TORCH_CHECK(values.scalar_type() == at::kFloat || values.scalar_type() == at::kInt, what, ": values have dtype ",
                values.scalar_type(), ", expected float32 or int32");
    const int64_t n = values.numel();
    TORCH_CHECK(n == runs.numel(), what, ": ", n, " values for ", runs.numel(), " keys or heads");
    TORCH_CHECK(n < (1LL << 31), what, ": the values must have fewer than 2^31 elements");
    const bool has_out = out.has_value() && out->defined();
    if (has_out) {
        check_gpu(*out, "out", values.scalar_type());
        TORCH_CHECK(out->device() == values.device() && out->is_contiguous() && out->numel() == n, what,
                    ": out must be contiguous, on the values' device, with ", n, " elements");
    }
    if (n == 0) return has_out ? *out : at::empty_like(values);
    at::Tensor vc = aligned_contig(values).view(-1);
    at::Tensor dest = has_out && !(reinterpret_cast<uintptr_t>(out->data_ptr()) & 15u) ? out->view(-1)
                                                                                      : at::empty({n}, values.options());
    if (overlaps(vc, dest) && !same_elements(vc, dest)) vc = vc.clone();  // identical is fine: the call is in place
    if (overlaps(runs, dest)) runs = runs.clone();
    hipStream_t stream = cur_stream(values);
    auto ws = workspace(values, pcmx_scanbykey_workspace_bytes(n));
    if (values.scalar_type() == at::kFloat)
        check_rc(pcmx_scan_by_key_f32(runs.data_ptr(), head_mode, vc.data_ptr<float>(), dest.data_ptr<float>(), n, (int)op,
                                      exclusive ? 1 : 0, ws.data_ptr(), stream),
                 what);
    else
        check_rc(pcmx_scan_by_key_i32(runs.data_ptr(), head_mode, vc.data_ptr<int32_t>(), dest.data_ptr<int32_t>(), n,
                                      (int)op, exclusive ? 1 : 0, ws.data_ptr(), stream),
                 what);
    if (has_out) {
        if (dest.data_ptr() != out->data_ptr()) out->view(-1).copy_(dest);
        return *out;
    }
    return dest.view(values.sizes());
}

at::Tensor scan_by_key(const at::Tensor& keys, const at::Tensor& values, int64_t op, bool exclusive,
                       const c10::optional<at::Tensor>& out) {
    sort_key_type(keys, "scan_by_key");
    const at::DeviceGuard g(keys.device());
    return scan_by_key_launch(aligned_contig(keys).view(-1), PCMX_HEADS_FROM_KEYS, values, op, exclusive, out, "scan_by_key");
}

at::Tensor segmented_scan(const at::Tensor& values, const at::Tensor& heads, int64_t op, bool exclusive,
                          const c10::optional<at::Tensor>& out) {
    TORCH_CHECK(values.is_cuda(), "segmented_scan: values must be a GPU tensor");
    const at::DeviceGuard g(values.device());
    TORCH_CHECK(heads.device() == values.device(), "segmented_scan: heads must be on the values' device");
    return scan_by_key_launch(mask_bytes(heads, values.numel(), "segmented_scan"), PCMX_HEADS_FROM_FLAGS, values, op,
                              exclusive, out, "segmented_scan");
}

at::Tensor run_positions(const at::Tensor& keys) {
    sort_key_type(keys, "run_positions");
    const at::DeviceGuard g(keys.device());
    const int64_t n = keys.numel();
    TORCH_CHECK(n < (1LL << 31), "run_positions: the keys must have fewer than 2^31 elements");
    at::Tensor pos = at::empty(keys.sizes(), keys.options().dtype(at::kInt));
    if (n == 0) return pos;
    at::Tensor kc = aligned_contig(keys).view(-1);
    auto ws = workspace(keys, pcmx_scanbykey_workspace_bytes(n));
    check_rc(pcmx_run_positions_b32(kc.data_ptr(), pos.data_ptr<int32_t>(), n, ws.data_ptr(), cur_stream(keys)),
             "run_positions");
    return pos;
}

// ---------------------------------------------------------------- histograms (bincount / even bins / explicit edges)
// int32 counts of the flattened samples (csrc/kernels/bincount.hip). The samples keep their element-aligned start (a
// view such as x[1:] is not copied; the kernel peels its ends); only a non-contiguous input is gathered first. `out`
// is a 1-D int32 tensor of num_bins entries; accumulate adds into it instead of zeroing it. No workspace, no sync.
struct HistDest {
    at::Tensor dest;  // contiguous int32 [num_bins]: the caller's out where it is contiguous
    bool copy_back;
};

HistDest hist_dest(const at::Tensor& x, int64_t num_bins, const c10::optional<at::Tensor>& out, bool accumulate,
                   const char* what) {
    TORCH_CHECK(num_bins >= 1 && num_bins < (1LL << 31), what, ": ", num_bins, " bins (1 to 2^31 - 1)");
    TORCH_CHECK(x.numel() < (1LL << 31), what, ": the samples must have fewer than 2^31 elements");
    const bool has_out = out.has_value() && out->defined();
    TORCH_CHECK(has_out || !accumulate, what, ": accumulate needs out");
    if (!has_out) return {at::empty({num_bins}, x.options().dtype(at::kInt)), false};
    check_gpu(*out, "out", at::kInt);
    TORCH_CHECK(out->device() == x.device() && out->dim() == 1 && out->numel() == num_bins, what,
                ": out must be 1-D, on the samples' device, with ", num_bins, " entries");
    if (out->is_contiguous()) return {*out, false};
    return {accumulate ? out->contiguous() : at::empty({num_bins}, out->options()), true};
}

at::Tensor hist_finish(const HistDest& d, const c10::optional<at::Tensor>& out) {
    if (!d.copy_back) return d.dest;
    out->copy_(d.dest);
    return *out;
}

at::Tensor bincount(const at::Tensor& x, int64_t num_bins, const c10::optional<at::Tensor>& weights,
                    const c10::optional<at::Tensor>& out, bool accumulate) {
    TORCH_CHECK(x.is_cuda(), "bincount: x must be a GPU tensor");
    TORCH_CHECK(x.scalar_type() == at::kInt || x.scalar_type() == at::kByte, "bincount: x has dtype ", x.scalar_type(),
                ", expected int32 or uint8");
    const at::DeviceGuard g(x.device());
    HistDest d = hist_dest(x, num_bins, out, accumulate, "bincount");
    const bool has_w = weights.has_value() && weights->defined();
    at::Tensor xc = x.contiguous().view(-1), wc;
    if (has_w) {
        check_gpu(*weights, "weights", at::kInt);
        TORCH_CHECK(weights->device() == x.device() && weights->numel() == x.numel(), "bincount: ", weights->numel(),
                    " weights for ", x.numel(), " samples on ", x.device());
        xc = aligned_contig(xc), wc = aligned_contig(*weights).view(-1);
        if (overlaps(wc, d.dest)) wc = wc.clone();
    }
    if (overlaps(xc, d.dest)) xc = xc.clone();
    const int32_t* w = has_w ? wc.data_ptr<int32_t>() : nullptr;
    const int acc = accumulate ? 1 : 0;
    if (x.scalar_type() == at::kInt)
        check_rc(pcmx_bincount_i32(xc.data_ptr<int32_t>(), w, xc.numel(), num_bins, d.dest.data_ptr<int32_t>(), acc,
                                   cur_stream(x)),
                 "bincount");
    else
        check_rc(pcmx_bincount_u8(xc.data_ptr<uint8_t>(), w, xc.numel(), num_bins, d.dest.data_ptr<int32_t>(), acc,
                                  cur_stream(x)),
                 "bincount");
    return hist_finish(d, out);
}

// scale = float32(bins) / (float32(hi) - float32(lo)), computed once by the caller
at::Tensor hist_even(const at::Tensor& x, int64_t bins, double lo, double hi, double scale,
                     const c10::optional<at::Tensor>& out, bool accumulate) {
    check_gpu(x, "x", at::kFloat);
    const at::DeviceGuard g(x.device());
    HistDest d = hist_dest(x, bins, out, accumulate, "hist_even");
    at::Tensor xc = x.contiguous().view(-1);
    if (overlaps(xc, d.dest)) xc = xc.clone();
    check_rc(pcmx_hist_even_f32(xc.data_ptr<float>(), xc.numel(), bins, (float)lo, (float)hi, (float)scale,
                                d.dest.data_ptr<int32_t>(), accumulate ? 1 : 0, cur_stream(x)),
             "hist_even");
    return hist_finish(d, out);
}

at::Tensor hist_range(const at::Tensor& x, const at::Tensor& edges, const c10::optional<at::Tensor>& out,
                      bool accumulate) {
    check_gpu(x, "x", at::kFloat), check_gpu(edges, "edges", at::kFloat);
    TORCH_CHECK(edges.device() == x.device() && edges.dim() == 1 && edges.numel() >= 2, "hist_range: edges must be 1-D, on the "
                "samples' device, with at least 2 values");
    const at::DeviceGuard g(x.device());
    const int64_t bins = edges.numel() - 1;
    HistDest d = hist_dest(x, bins, out, accumulate, "hist_range");
    at::Tensor xc = x.contiguous().view(-1), ec = edges.contiguous();
    if (overlaps(xc, d.dest)) xc = xc.clone();
    if (overlaps(ec, d.dest)) ec = ec.clone();
    check_rc(pcmx_hist_range_f32(xc.data_ptr<float>(), xc.numel(), ec.data_ptr<float>(), bins, d.dest.data_ptr<int32_t>(),
                                 accumulate ? 1 : 0, cur_stream(x)),
             "hist_range (at most 8192 bins)");
    return hist_finish(d, out);
}

// ---------------------------------------------------------------- merge of sorted sequences / sorted search
// Merge of two sorted float32 / int32 key sequences, flattened, and searchsorted (csrc/kernels/merge.hip). The inputs
// keep their element-aligned start (a view such as x[1:] is not copied; only a non-contiguous input is gathered
// first). Outputs are fresh 1-D tensors, or the caller's `out` tensors (contiguous, exact size, right dtype; one that is
// not 16-B aligned is written through a temporary). Workspace from the caching allocator, no host synchronisation, no
// error word: no block of these kernels waits for another.
at::Tensor merge_input(const at::Tensor& t, const at::Tensor& like, const char* what, const char* name) {
    TORCH_CHECK(t.device() == like.device(), what, ": ", name, " must be on ", like.device());
    TORCH_CHECK(t.scalar_type() == like.scalar_type(), what, ": ", name, " has dtype ", t.scalar_type(), ", expected ",
                like.scalar_type());
    return t.contiguous().view(-1);
}

at::Tensor merge_dest(const c10::optional<at::Tensor>& out, const at::Tensor& like, at::ScalarType dt, int64_t n,
                      const char* what) {
    if (!(out.has_value() && out->defined())) return at::empty({n}, like.options().dtype(dt));
    check_gpu(*out, "out", dt);
    TORCH_CHECK(out->device() == like.device() && out->is_contiguous() && out->numel() == n, what,
                ": out must be contiguous, on the input's device, with ", n, " elements");
    return (reinterpret_cast<uintptr_t>(out->data_ptr()) & 15u) ? at::empty({n}, out->options()) : out->view(-1);
}

at::Tensor merge_finish(const c10::optional<at::Tensor>& out, const at::Tensor& dest) {
    if (!(out.has_value() && out->defined())) return dest;
    if (dest.data_ptr() != out->data_ptr()) out->view(-1).copy_(dest);
    return *out;
}

// keys_out / aux_out: destinations or undefined tensors (no such output in this mode)
void merge_launch(const at::Tensor& a, const at::Tensor& b, const at::Tensor* va, const at::Tensor* vb,
                  at::Tensor keys_out, at::Tensor aux_out, int mode, bool descending, const char* what) {
    const int key_type = sort_key_type(a, what);
    const int64_t na = a.numel(), nb = b.numel();
    if (na + nb == 0) return;
    at::Tensor ac = a, bc = b, vac, vbc;
    for (const at::Tensor* o : {&keys_out, &aux_out}) {
        if (!o->defined()) continue;
        if (overlaps(ac, *o)) ac = ac.clone();
        if (overlaps(bc, *o)) bc = bc.clone();
    }
    if (va) {
        vac = *va, vbc = *vb;
        for (const at::Tensor* o : {&keys_out, &aux_out}) {
            if (overlaps(vac, *o)) vac = vac.clone();
            if (overlaps(vbc, *o)) vbc = vbc.clone();
        }
    }
    auto ws = workspace(a, pcmx_merge_workspace_bytes(na, nb));
    check_rc(pcmx_merge_b32(ac.data_ptr(), va ? vac.data_ptr() : nullptr, na, bc.data_ptr(), va ? vbc.data_ptr() : nullptr,
                            nb, keys_out.defined() ? keys_out.data_ptr() : nullptr,
                            aux_out.defined() ? aux_out.data_ptr() : nullptr, key_type, mode, descending ? 1 : 0,
                            ws.data_ptr(), cur_stream(a)),
             what);
}

int64_t merge_total(const at::Tensor& a, const at::Tensor& b, const char* what) {
    const int64_t n = a.numel() + b.numel();
    TORCH_CHECK(n < (1LL << 31), what, ": indices are int32, the two inputs together must have fewer than 2^31 elements");
    return n;
}

at::Tensor merge_keys(const at::Tensor& a, const at::Tensor& b, bool descending, const c10::optional<at::Tensor>& out) {
    sort_key_type(a, "merge_keys");
    const at::DeviceGuard g(a.device());
    at::Tensor ac = a.contiguous().view(-1), bc = merge_input(b, a, "merge_keys", "b");
    at::Tensor dest = merge_dest(out, a, a.scalar_type(), merge_total(a, b, "merge_keys"), "merge_keys");
    merge_launch(ac, bc, nullptr, nullptr, dest, at::Tensor(), PCMX_MERGE_KEYS, descending, "merge_keys");
    return merge_finish(out, dest);
}

// (merged keys, int32 indices into cat(a, b)); with want_keys false the first tensor is empty and no keys are written
std::tuple<at::Tensor, at::Tensor> merge_index(const at::Tensor& a, const at::Tensor& b, bool descending, bool want_keys,
                                               const c10::optional<at::Tensor>& out_keys,
                                               const c10::optional<at::Tensor>& out_idx) {
    sort_key_type(a, "merge_index");
    const at::DeviceGuard g(a.device());
    at::Tensor ac = a.contiguous().view(-1), bc = merge_input(b, a, "merge_index", "b");
    const int64_t n = merge_total(a, b, "merge_index");
    at::Tensor kd = want_keys ? merge_dest(out_keys, a, a.scalar_type(), n, "merge_index") : at::Tensor();
    at::Tensor id = merge_dest(out_idx, a, at::kInt, n, "merge_index");
    merge_launch(ac, bc, nullptr, nullptr, kd, id, PCMX_MERGE_INDEX, descending, "merge_index");
    return {want_keys ? merge_finish(out_keys, kd) : at::empty({0}, a.options()), merge_finish(out_idx, id)};
}

std::tuple<at::Tensor, at::Tensor> merge_pairs(const at::Tensor& ka, const at::Tensor& va, const at::Tensor& kb,
                                               const at::Tensor& vb, bool descending,
                                               const c10::optional<at::Tensor>& out_keys,
                                               const c10::optional<at::Tensor>& out_values) {
    sort_key_type(ka, "merge_pairs");
    TORCH_CHECK(va.scalar_type() == at::kFloat || va.scalar_type() == at::kInt, "merge_pairs: values have dtype ",
                va.scalar_type(), ", expected float32 or int32");
    TORCH_CHECK(va.numel() == ka.numel() && vb.numel() == kb.numel(), "merge_pairs: ", va.numel(), " / ", vb.numel(),
                " values for ", ka.numel(), " / ", kb.numel(), " keys");
    const at::DeviceGuard g(ka.device());
    at::Tensor kac = ka.contiguous().view(-1), kbc = merge_input(kb, ka, "merge_pairs", "keys_b");
    TORCH_CHECK(va.device() == ka.device(), "merge_pairs: values_a must be on ", ka.device());
    at::Tensor vac = va.contiguous().view(-1), vbc = merge_input(vb, va, "merge_pairs", "values_b");
    const int64_t n = merge_total(ka, kb, "merge_pairs");
    at::Tensor kd = merge_dest(out_keys, ka, ka.scalar_type(), n, "merge_pairs");
    at::Tensor vd = merge_dest(out_values, ka, va.scalar_type(), n, "merge_pairs");
    merge_launch(kac, kbc, &vac, &vbc, kd, vd, PCMX_MERGE_PAIRS, descending, "merge_pairs");
    return {merge_finish(out_keys, kd), merge_finish(out_values, vd)};
}

// int32 [values.shape]: how many keys of the sorted sequence precede (right: precede or equal) each value
at::Tensor searchsorted(const at::Tensor& sorted, const at::Tensor& values, bool right, bool descending,
                        bool values_sorted, const c10::optional<at::Tensor>& out) {
    const int key_type = sort_key_type(sorted, "searchsorted");
    const at::DeviceGuard g(sorted.device());
    at::Tensor sc = sorted.contiguous().view(-1), vc = merge_input(values, sorted, "searchsorted", "values");
    const int64_t n = sc.numel(), m = vc.numel();
    TORCH_CHECK(n < (1LL << 31) && m < (1LL << 31), "searchsorted: the sequence and the values must each have fewer than "
                "2^31 elements");
    const bool has_out = out.has_value() && out->defined();
    if (has_out) TORCH_CHECK(out->sizes() == values.sizes(), "searchsorted: out must have the shape of values");
    at::Tensor dest = merge_dest(out, sorted, at::kInt, m, "searchsorted");
    if (m != 0) {
        if (overlaps(sc, dest)) sc = sc.clone();
        if (overlaps(vc, dest)) vc = vc.clone();
        auto ws = workspace(sorted, pcmx_searchsorted_workspace_bytes(n, m, values_sorted ? 1 : 0));
        check_rc(pcmx_searchsorted_b32(sc.data_ptr(), n, vc.data_ptr(), m, dest.data_ptr<int32_t>(), key_type, right ? 1 : 0,
                                       descending ? 1 : 0, values_sorted ? 1 : 0, ws.data_ptr(), cur_stream(sorted)),
                 "searchsorted");
    }
    return has_out ? merge_finish(out, dest) : dest.view(values.sizes());
}

// ---------------------------------------------------------------- set operations on sorted sequences
// Intersection / union / difference / symmetric difference of two sorted float32 / int32 key sequences, flattened
// (csrc/kernels/setops.hip). Inputs as for the merge (read where they lie; a non-contiguous one is gathered first).
// The outputs follow the select ops: they have room for the op's capacity, only [0, count) is written, count is a
// 0-d int64 tensor on the device and nothing synchronises; a caller's buffer that is not 16-B aligned is written
// through a copy of itself, so what lies past the count survives. The look-back shares the scan's per-(device, stream)
// sticky error word, so scan_check() covers these ops.
int64_t set_capacity(int64_t op, int64_t na, int64_t nb, const char* what) {
    TORCH_CHECK(op >= PCMX_SET_INTERSECTION && op <= PCMX_SET_SYMDIFF, what, ": unknown op code ", op);
    return op == PCMX_SET_INTERSECTION ? std::min(na, nb) : (op == PCMX_SET_DIFFERENCE ? na : na + nb);
}

at::Tensor set_finish(const c10::optional<at::Tensor>& out, const at::Tensor& dest) {
    if (!(out.has_value() && out->defined())) return dest;
    if (!dest.is_same(*out)) out->copy_(dest);
    return *out;
}

// keys_out / aux_out: destinations or undefined tensors (no such output in this mode); returns the count
at::Tensor set_launch(const at::Tensor& a, const at::Tensor& b, const at::Tensor* va, const at::Tensor* vb,
                      at::Tensor keys_out, at::Tensor aux_out, int64_t op, int mode, bool descending, const char* what) {
    const int key_type = sort_key_type(a, what);
    hipStream_t stream = cur_stream(a);
    unsigned* err_dev = scan_err_word(a.device().index(), stream).dev;
    raise_pending_scan_error(a.device().index(), stream);
    const int64_t na = a.numel(), nb = b.numel();
    at::Tensor ac = a, bc = b, vac, vbc;
    for (const at::Tensor* o : {&keys_out, &aux_out}) {
        if (!o->defined()) continue;
        if (overlaps(ac, *o)) ac = ac.clone();
        if (overlaps(bc, *o)) bc = bc.clone();
    }
    if (va) {
        vac = *va, vbc = *vb;
        for (const at::Tensor* o : {&keys_out, &aux_out}) {
            if (overlaps(vac, *o)) vac = vac.clone();
            if (overlaps(vbc, *o)) vbc = vbc.clone();
        }
    }
    at::Tensor count = at::empty({}, a.options().dtype(at::kLong));
    auto ws = workspace(a, pcmx_set_op_workspace_bytes(na, nb));
    check_rc(pcmx_set_op_b32(ac.data_ptr(), va ? vac.data_ptr() : nullptr, na, bc.data_ptr(), va ? vbc.data_ptr() : nullptr,
                             nb, keys_out.defined() ? keys_out.data_ptr() : nullptr,
                             aux_out.defined() ? aux_out.data_ptr() : nullptr, (long long*)count.data_ptr<int64_t>(),
                             (int)op, mode, key_type, descending ? 1 : 0, ws.data_ptr(), ws.numel(), err_dev, stream),
             what);
    return count;
}

// (kept keys, int32 indices into cat(a, b) or an empty tensor, count)
std::tuple<at::Tensor, at::Tensor, at::Tensor> set_op(const at::Tensor& a, const at::Tensor& b, int64_t op, bool descending,
                                                      bool want_idx, const c10::optional<at::Tensor>& out_keys,
                                                      const c10::optional<at::Tensor>& out_idx) {
    sort_key_type(a, "set_op");
    const at::DeviceGuard g(a.device());
    at::Tensor ac = a.contiguous().view(-1), bc = merge_input(b, a, "set_op", "b");
    merge_total(a, b, "set_op");
    const int64_t cap = set_capacity(op, ac.numel(), bc.numel(), "set_op");
    at::Tensor kd = select_dest(out_keys, a, a.scalar_type(), cap, "set_op");
    at::Tensor id = want_idx ? select_dest(out_idx, a, at::kInt, cap, "set_op") : at::Tensor();
    at::Tensor count = set_launch(ac, bc, nullptr, nullptr, kd, id, op, want_idx ? PCMX_MERGE_INDEX : PCMX_MERGE_KEYS,
                                  descending, "set_op");
    return {set_finish(out_keys, kd), want_idx ? set_finish(out_idx, id) : at::empty({0}, a.options().dtype(at::kInt)),
            count};
}

// (kept keys, their values, count)
std::tuple<at::Tensor, at::Tensor, at::Tensor> set_op_pairs(const at::Tensor& ka, const at::Tensor& va, const at::Tensor& kb,
                                                            const at::Tensor& vb, int64_t op, bool descending) {
    sort_key_type(ka, "set_op_pairs");
    TORCH_CHECK(va.scalar_type() == at::kFloat || va.scalar_type() == at::kInt, "set_op_pairs: values have dtype ",
                va.scalar_type(), ", expected float32 or int32");
    TORCH_CHECK(va.numel() == ka.numel() && vb.numel() == kb.numel(), "set_op_pairs: ", va.numel(), " / ", vb.numel(),
                " values for ", ka.numel(), " / ", kb.numel(), " keys");
    const at::DeviceGuard g(ka.device());
    at::Tensor kac = ka.contiguous().view(-1), kbc = merge_input(kb, ka, "set_op_pairs", "keys_b");
    TORCH_CHECK(va.device() == ka.device(), "set_op_pairs: values_a must be on ", ka.device());
    at::Tensor vac = va.contiguous().view(-1), vbc = merge_input(vb, va, "set_op_pairs", "values_b");
    merge_total(ka, kb, "set_op_pairs");
    const int64_t cap = set_capacity(op, kac.numel(), kbc.numel(), "set_op_pairs");
    at::Tensor kd = at::empty({cap}, ka.options()), vd = at::empty({cap}, va.options());
    at::Tensor count = set_launch(kac, kbc, &vac, &vbc, kd, vd, op, PCMX_MERGE_PAIRS, descending, "set_op_pairs");
    return {kd, vd, count};
}

// ---------------------------------------------------------------- reduction over ragged segments (offsets)
// out[j] = op over x.flatten()[offsets[j] : offsets[j+1]] (csrc/kernels/ragged.hip). x and offsets are read where they
// lie (element alignment is enough). `out` (1-D, contiguous, at least S elements, x's dtype) is returned as out[:S]
// and never written past S; one that is not 16-B aligned is written through a temporary. The offsets are not looked
// at on the host: nothing synchronises, and there is no error word.
at::Tensor segment_offsets(const at::Tensor& offsets, const at::Tensor& x, const char* what) {
    check_gpu(offsets, "offsets", at::kInt);
    TORCH_CHECK(offsets.device() == x.device(), what, ": offsets must be on ", x.device());
    TORCH_CHECK(offsets.dim() == 1 && offsets.is_contiguous() && offsets.numel() >= 1, what,
                ": offsets must be 1-D and contiguous with at least one entry");
    return offsets;
}

at::Tensor segment_reduce(const at::Tensor& x, const at::Tensor& offsets, int64_t op, const c10::optional<at::Tensor>& out) {
    TORCH_CHECK(x.is_cuda(), "segment_reduce: x must be a GPU tensor");
    TORCH_CHECK(x.scalar_type() == at::kFloat || x.scalar_type() == at::kInt, "segment_reduce: x has dtype ", x.scalar_type(),
                ", expected float32 or int32");
    TORCH_CHECK(op >= PCMX_OP_SUM && op <= PCMX_OP_MAX, "segment_reduce: op code ", op);
    TORCH_CHECK(x.is_contiguous(), "segment_reduce: x must be contiguous");
    const at::DeviceGuard g(x.device());
    at::Tensor oc = segment_offsets(offsets, x, "segment_reduce");
    const int64_t n = x.numel(), S = oc.numel() - 1;
    TORCH_CHECK(n + S < (1LL << 31), "segment_reduce: elements and segments together must be fewer than 2^31");
    const bool has_out = out.has_value() && out->defined();
    if (has_out) {
        check_gpu(*out, "out", x.scalar_type());
        TORCH_CHECK(out->device() == x.device() && out->dim() == 1 && out->is_contiguous() && out->numel() >= S,
                    "segment_reduce: out must be 1-D, contiguous, on x's device, with at least ", S, " elements");
        TORCH_CHECK(!(S && overlaps(*out, x)) && !overlaps(*out, oc), "segment_reduce: out must not overlap an input");
    }
    at::Tensor xc = x.view(-1);
    at::Tensor dest = has_out && !(reinterpret_cast<uintptr_t>(out->data_ptr()) & 15u) ? out->narrow(0, 0, S)
                                                                                      : at::empty({S}, x.options());
    if (S != 0) {
        auto ws = workspace(x, pcmx_segment_workspace_bytes(n, S));
        hipStream_t stream = cur_stream(x);
        if (x.scalar_type() == at::kFloat)
            check_rc(pcmx_segment_reduce_f32(n ? xc.data_ptr<float>() : nullptr, n, oc.data_ptr<int32_t>(), S, (int)op,
                                             dest.data_ptr<float>(), ws.data_ptr(), stream),
                     "segment_reduce");
        else
            check_rc(pcmx_segment_reduce_i32(n ? xc.data_ptr<int32_t>() : nullptr, n, oc.data_ptr<int32_t>(), S, (int)op,
                                             dest.data_ptr<int32_t>(), ws.data_ptr(), stream),
                     "segment_reduce");
    }
    if (!has_out) return dest;
    at::Tensor head = out->narrow(0, 0, S);
    if (S != 0 && dest.data_ptr() != out->data_ptr()) head.copy_(dest);
    return head;
}

// ---------------------------------------------------------------- argmin / argmax (csrc/kernels/argreduce.hip)
// (values, indices) of op (PCMX_OP_MIN / PCMX_OP_MAX) for float32 / int32; an output that is not wanted is not written
// by the kernels and comes back as an empty tensor. Shapes, op, route and chunk are checked in Python and again by the C
// entry points; workspaces come from torch's allocator on the current stream; nothing synchronises.
int arg_key_type(const at::Tensor& x, const char* what) {
    TORCH_CHECK(x.is_cuda(), what, ": GPU tensor expected");
    TORCH_CHECK(x.scalar_type() == at::kFloat || x.scalar_type() == at::kInt, what, ": x has dtype ", x.scalar_type(),
                ", expected float32 or int32");
    return x.scalar_type() == at::kFloat ? PCMX_KEY_F32 : PCMX_KEY_I32;
}

// 0-d outputs; the index into the row-major flattened tensor
std::tuple<at::Tensor, at::Tensor> arg_reduce(const at::Tensor& x, int64_t op, bool want_values, bool want_indices) {
    const int kt = arg_key_type(x, "arg_reduce");
    TORCH_CHECK(x.numel() > 0, "arg_reduce: no extremum of an empty tensor");
    TORCH_CHECK(want_values || want_indices, "arg_reduce: nothing to compute");
    const at::DeviceGuard g(x.device());
    at::Tensor xc = aligned_contig(x);
    at::Tensor vals = want_values ? at::empty({}, x.options()) : at::empty({0}, x.options());
    at::Tensor idx = want_indices ? at::empty({}, x.options().dtype(at::kInt)) : at::empty({0}, x.options().dtype(at::kInt));
    auto ws = workspace(x, pcmx_arg_reduce_workspace_bytes(xc.numel()));
    check_rc(pcmx_arg_reduce_b32(xc.data_ptr(), xc.numel(), kt, (int)op, want_values ? vals.data_ptr() : nullptr,
                                 want_indices ? idx.data_ptr<int32_t>() : nullptr, ws.data_ptr(), cur_stream(x)),
             "arg_reduce");
    return {vals, idx};
}

// x is the [outer, n, inner] view; outputs [outer, inner], the position along n
std::tuple<at::Tensor, at::Tensor> axis_arg_reduce(const at::Tensor& x, int64_t op, int64_t route, int64_t chunk, bool want_values,
                                                   bool want_indices) {
    const int kt = arg_key_type(x, "axis_arg_reduce");
    TORCH_CHECK(x.dim() == 3, "axis_arg_reduce: expected a 3-D [outer, n, inner] tensor, got ", x.dim(), " dimensions");
    TORCH_CHECK(want_values || want_indices, "axis_arg_reduce: nothing to compute");
    const at::DeviceGuard g(x.device());
    at::Tensor xc = aligned_contig(x);
    const int64_t outer = xc.size(0), n = xc.size(1), inner = xc.size(2);
    TORCH_CHECK(n > 0, "axis_arg_reduce: no extremum along an empty dimension");
    at::Tensor vals = want_values ? at::empty({outer, inner}, x.options()) : at::empty({0}, x.options());
    at::Tensor idx = want_indices ? at::empty({outer, inner}, x.options().dtype(at::kInt)) : at::empty({0}, x.options().dtype(at::kInt));
    if (outer * inner == 0) return {vals, idx};
    auto ws = workspace(x, pcmx_axis_arg_workspace_bytes(outer, n, inner));
    check_rc(pcmx_axis_arg_reduce_b32(xc.data_ptr(), want_values ? vals.data_ptr() : nullptr,
                                      want_indices ? idx.data_ptr<int32_t>() : nullptr, outer, n, inner, kt, (int)op, (int)route,
                                      chunk, ws.data_ptr(), cur_stream(x)),
             "axis_arg_reduce");
    return {vals, idx};
}

// [S] outputs; the FLAT index into x.flatten(), -1 and the identity for an empty segment. out_values / out_indices
// (1-D, contiguous, at least S elements) are written in [:S] only and returned as their [:S].
std::tuple<at::Tensor, at::Tensor> segment_arg_reduce(const at::Tensor& x, const at::Tensor& offsets, int64_t op, bool want_values,
                                                      bool want_indices, const c10::optional<at::Tensor>& out_values,
                                                      const c10::optional<at::Tensor>& out_indices) {
    const int kt = arg_key_type(x, "segment_arg_reduce");
    TORCH_CHECK(x.is_contiguous(), "segment_arg_reduce: x must be contiguous");
    TORCH_CHECK(want_values || want_indices, "segment_arg_reduce: nothing to compute");
    const at::DeviceGuard g(x.device());
    at::Tensor oc = segment_offsets(offsets, x, "segment_arg_reduce");
    const int64_t n = x.numel(), S = oc.numel() - 1;
    TORCH_CHECK(n + S < (1LL << 31), "segment_arg_reduce: elements and segments together must be fewer than 2^31");
    auto dest = [&](const c10::optional<at::Tensor>& out, bool want, at::ScalarType dt, const char* name) {
        if (!want) return at::empty({0}, x.options().dtype(dt));
        if (!(out.has_value() && out->defined())) return at::empty({S}, x.options().dtype(dt));
        check_gpu(*out, name, dt);
        TORCH_CHECK(out->device() == x.device() && out->dim() == 1 && out->is_contiguous() && out->numel() >= S,
                    "segment_arg_reduce: ", name, " must be 1-D, contiguous, on x's device, with at least ", S, " elements");
        TORCH_CHECK(!(S && overlaps(*out, x)) && !overlaps(*out, oc), "segment_arg_reduce: ", name, " must not overlap an input");
        return out->narrow(0, 0, S);
    };
    at::Tensor vals = dest(out_values, want_values, x.scalar_type(), "out_values");
    at::Tensor idx = dest(out_indices, want_indices, at::kInt, "out_indices");
    if (S != 0) {
        at::Tensor xc = x.view(-1);
        auto ws = workspace(x, pcmx_segment_arg_workspace_bytes(n, S));
        check_rc(pcmx_segment_arg_reduce_b32(n ? xc.data_ptr() : nullptr, n, oc.data_ptr<int32_t>(), S, kt, (int)op,
                                             want_values ? vals.data_ptr() : nullptr,
                                             want_indices ? idx.data_ptr<int32_t>() : nullptr, ws.data_ptr(), cur_stream(x)),
                 "segment_arg_reduce");
    }
    return {vals, idx};
}

// uint8 [n]: 1 at every offsets[j] < n, 0 elsewhere: the head flags segmented_scan takes
at::Tensor segment_heads(const at::Tensor& offsets, int64_t n, const at::Tensor& like) {
    TORCH_CHECK(like.is_cuda(), "segment_heads: the values must be a GPU tensor");
    const at::DeviceGuard g(like.device());
    at::Tensor oc = segment_offsets(offsets, like, "segment_heads");
    TORCH_CHECK(n >= 0 && n < (1LL << 31) && oc.numel() < (1LL << 31), "segment_heads: fewer than 2^31 elements and offsets");
    at::Tensor heads = at::empty({n}, like.options().dtype(at::kByte));
    if (n != 0)
        check_rc(pcmx_segment_heads(oc.data_ptr<int32_t>(), oc.numel() - 1, n, heads.data_ptr<uint8_t>(), cur_stream(like)),
                 "segment_heads");
    return heads;
}

// ---------------------------------------------------------------- sort inside ragged segments (offsets)
// (sorted keys [n], values or flat int32 indices [n], the 4-word int32 summary) of the flattened keys with every segment
// sorted on its own (csrc/kernels/segsort.hip). mode: PCMX_SORT_* | PCMX_SEGSORT_GRID(m). With want_keys false (INDEX
// mode) the first tensor is empty and no keys are written. Segments longer than PCMX_SEGSORT_MAX_LEN are left UNWRITTEN
// in the outputs and counted in the summary, a view of the workspace the caller may read (16 bytes) or drop: nothing
// synchronises here. Contiguous 16-B aligned inputs (copied when they are not), fresh outputs.
std::tuple<at::Tensor, at::Tensor, at::Tensor> segment_sort(const at::Tensor& keys, const c10::optional<at::Tensor>& values,
                                                            const at::Tensor& offsets, int64_t mode, bool descending,
                                                            int64_t begin_bit, int64_t end_bit, bool want_keys) {
    const int key_type = sort_key_type(keys, "segment_sort");
    TORCH_CHECK(keys.is_contiguous(), "segment_sort: the keys must be contiguous");
    const at::DeviceGuard g(keys.device());
    at::Tensor oc = segment_offsets(offsets, keys, "segment_sort");
    const int64_t n = keys.numel(), S = oc.numel() - 1, base_mode = mode & 0xff;
    TORCH_CHECK(n < (1LL << 30) && S < (1LL << 30), "segment_sort: fewer than 2^30 keys and segments");
    at::Tensor kc = aligned_contig(keys).view(-1), vc;
    if (values.has_value()) {
        TORCH_CHECK(values->device() == keys.device(), "segment_sort: values must be on the keys' device");
        TORCH_CHECK(values->scalar_type() == at::kFloat || values->scalar_type() == at::kInt,
                    "segment_sort: values have dtype ", values->scalar_type(), ", expected float32 or int32");
        TORCH_CHECK(values->numel() == n && values->is_contiguous(), "segment_sort: values must be contiguous with one "
                    "entry per key");
        vc = aligned_contig(*values).view(-1);
    }
    TORCH_CHECK(values.has_value() == (base_mode == PCMX_SORT_PAIRS), "segment_sort: values go with PCMX_SORT_PAIRS and only with it");
    TORCH_CHECK(want_keys || base_mode == PCMX_SORT_INDEX, "segment_sort: only PCMX_SORT_INDEX can go without sorted keys");
    at::Tensor ko = at::empty({want_keys ? n : 0}, keys.options()), vo;
    if (base_mode == PCMX_SORT_PAIRS) vo = at::empty({n}, values->options());
    else vo = at::empty({base_mode == PCMX_SORT_INDEX ? n : 0}, keys.options().dtype(at::kInt));
    at::Tensor ws = workspace(keys, pcmx_segment_sort_workspace_bytes(n, S));
    at::Tensor summary = ws.narrow(0, PCMX_SEGSORT_SUMMARY_OFFSET, 16).view(at::kInt);
    if (n == 0) {  // empty tensors have no base pointer
        summary.zero_();
        return {ko, vo, summary};
    }
    check_rc(pcmx_segment_sort_b32(kc.data_ptr(), want_keys ? ko.data_ptr() : nullptr, values.has_value() ? vc.data_ptr() : nullptr,
                                   base_mode == PCMX_SORT_KEYS ? nullptr : vo.data_ptr(), n, oc.data_ptr<int32_t>(), S, key_type,
                                   (int)mode, descending ? 1 : 0, (int)begin_bit, (int)end_bit, ws.data_ptr(), cur_stream(keys)),
             "segment_sort");
    return {ko, vo, summary};
}

// ---------------------------------------------------------------- SGEMM
at::Tensor sgemm_out(const at::Tensor& a, const at::Tensor& b, at::Tensor c, double alpha, double beta, int64_t variant) {
    check_gpu(a, "a", at::kFloat), check_gpu(b, "b", at::kFloat), check_gpu(c, "c", at::kFloat);
    TORCH_CHECK(a.dim() == 2 && b.dim() == 2 && c.dim() == 2, "sgemm: 2-D tensors");
    TORCH_CHECK(a.size(1) == b.size(0) && c.size(0) == a.size(0) && c.size(1) == b.size(1), "sgemm: shape mismatch");
    TORCH_CHECK(a.stride(1) == 1 && b.stride(1) == 1 && c.stride(1) == 1, "sgemm: row-major operands");
    const at::DeviceGuard g(a.device());
    const int M = (int)a.size(0), N = (int)b.size(1), K = (int)a.size(1);
    int rc;
    if (variant < 0)
        rc = pcmx_sgemm_f32(a.data_ptr<float>(), b.data_ptr<float>(), c.data_ptr<float>(), M, N, K, (int)a.stride(0),
                            (int)b.stride(0), (int)c.stride(0), (float)alpha, (float)beta, cur_stream(a));
    else
        rc = pcmx_sgemm_f32_variant(a.data_ptr<float>(), b.data_ptr<float>(), c.data_ptr<float>(), M, N, K, (int)a.stride(0),
                                    (int)b.stride(0), (int)c.stride(0), (float)alpha, (float)beta, (int)variant, cur_stream(a));
    check_rc(rc, "sgemm (shape must be tile-aligned; use parallel_c_programs_amd.ops.sgemm for any shape)");
    return c;
}

at::Tensor sgemm(const at::Tensor& a, const at::Tensor& b, int64_t variant) {
    auto c = at::empty({a.size(0), b.size(1)}, a.options());
    return sgemm_out(a, b, c, 1.0, 0.0, variant);
}

at::Tensor sgemm_simt(const at::Tensor& a, const at::Tensor& b) {
    check_gpu(a, "a", at::kFloat), check_gpu(b, "b", at::kFloat);
    TORCH_CHECK(a.dim() == 2 && b.dim() == 2 && a.size(1) == b.size(0), "sgemm_simt: shape mismatch");
    const at::DeviceGuard g(a.device());
    auto ac = a.contiguous(), bc = b.contiguous();
    auto c = at::empty({a.size(0), b.size(1)}, a.options());
    check_rc(pcmx_sgemm_f32_simt(ac.data_ptr<float>(), bc.data_ptr<float>(), c.data_ptr<float>(), (int)a.size(0), (int)b.size(1),
                                 (int)a.size(1), cur_stream(a)),
             "sgemm_simt");
    return c;
}

void device_info(int64_t device) { pcmx_print_device_info((int)device); }

void check_u8_gpu(const at::Tensor& t, const char* name) {
    check_gpu(t, name, at::kByte);
    TORCH_CHECK(t.is_contiguous(), name, " must be contiguous");
}

// ---------------------------------------------------------------- histogram equalisation
// The multi-block histeq keeps its histogram + ticket in a workspace that every call leaves zeroed, so it is
// allocated (and zeroed) once per (device, stream): no memset launch per call, and calls on different streams
// never share one.
at::Tensor& histeq_workspace(const at::Tensor& like, hipStream_t s) {
    static std::mutex mu;
    static auto* cache = new std::map<std::pair<int, hipStream_t>, at::Tensor>();  // never destroyed: no frees at exit
    std::lock_guard<std::mutex> lock(mu);
    auto& ws = (*cache)[{like.device().index(), s}];
    if (!ws.defined()) ws = at::zeros({pcmx_histeq_workspace_bytes()}, like.options().dtype(at::kByte));
    return ws;
}

at::Tensor histeq(const at::Tensor& img) {
    check_u8_gpu(img, "img");
    const at::DeviceGuard g(img.device());
    auto ic = aligned_contig(img);
    auto out = at::empty_like(ic);
    const hipStream_t s = cur_stream(img);
    auto& ws = histeq_workspace(ic, s);
    const int rc = pcmx_histeq_u8(ic.data_ptr<uint8_t>(), out.data_ptr<uint8_t>(), ic.numel(), ws.data_ptr(), s);
    if (rc) ws.zero_();  // a failed call may leave the self-cleaning replicas/ticket dirty: re-arm before raising
    check_rc(rc, "histeq");
    return out;
}

// ---------------------------------------------------------------- region growing
int64_t region2d_grow_(at::Tensor region, const at::Tensor& img, int64_t thr, int64_t batch, int64_t max_launches) {
    check_u8_gpu(region, "region"), check_u8_gpu(img, "img");
    TORCH_CHECK(region.dim() == 2 && img.sizes() == region.sizes() && region.device() == img.device() &&
                    img.size(0) > 2 && img.size(1) > 2,
                "region2d: padded (H+2, W+2) uint8 tensors on one device");
    const at::DeviceGuard g(img.device());
    const int H = (int)img.size(0) - 2, W = (int)img.size(1) - 2;
    auto ws = workspace(img, pcmx_region2d_workspace_bytes(H, W));
    int launches = 0;
    check_rc(pcmx_region2d_grow(img.data_ptr<uint8_t>(), region.data_ptr<uint8_t>(), H, W, (int)img.size(1), (int)thr,
                                ws.data_ptr(), (int)batch, (int)max_launches, cur_stream(img), &launches),
             "region2d_grow_");
    return launches;
}

int64_t region3d_grow_(at::Tensor region, const at::Tensor& data, int64_t thr, bool tiled, int64_t batch,
                       int64_t max_launches) {
    check_u8_gpu(region, "region"), check_u8_gpu(data, "data");
    TORCH_CHECK(data.dim() == 3 && data.size(0) == data.size(1) && data.size(1) == data.size(2) &&
                    region.sizes() == data.sizes() && region.device() == data.device(),
                "region3d: cubic uint8 volumes on one device");
    const at::DeviceGuard g(data.device());
    const int dim = (int)data.size(0);
    int launches = 0;
    if (tiled) {
        auto ws = workspace(data, pcmx_region3d_workspace_bytes(dim));
        check_rc(pcmx_region3d_grow_tiled(data.data_ptr<uint8_t>(), region.data_ptr<uint8_t>(), dim, (int)thr, ws.data_ptr(),
                                          (int)batch, (int)max_launches, cur_stream(data), &launches),
                 "region3d_grow_ (tiled)");
    } else {
        auto flag = at::empty({4}, data.options().dtype(at::kInt));
        check_rc(pcmx_region3d_grow_naive(data.data_ptr<uint8_t>(), region.data_ptr<uint8_t>(), dim, (int)thr,
                                          flag.data_ptr<int>(), (int)max_launches, cur_stream(data), &launches),
                 "region3d_grow_ (naive)");
    }
    return launches;
}

// z-slab with its halo planes: (nz + 2, dim, dim) uint8 tensors; planes 1..nz are grown, plane 0 / nz + 1 are
// read-only halo seeds when halos bit 0 / bit 1 is set (neighbour ranks' boundary planes)
int64_t region3d_grow_slab_(at::Tensor region, const at::Tensor& data, int64_t halos, int64_t thr, int64_t batch,
                            int64_t max_launches) {
    check_u8_gpu(region, "region"), check_u8_gpu(data, "data");
    TORCH_CHECK(data.dim() == 3 && data.size(1) == data.size(2) && data.size(0) >= 3 && region.sizes() == data.sizes() &&
                    region.device() == data.device(),
                "region3d_grow_slab_: (nz + 2, dim, dim) uint8 slabs with halo planes, on one device");
    TORCH_CHECK(halos >= 0 && halos <= 3, "region3d_grow_slab_: halos in 0..3");
    const at::DeviceGuard g(data.device());
    const int dim = (int)data.size(1), nz = (int)data.size(0) - 2;
    const size_t plane = (size_t)dim * dim;
    auto ws = workspace(data, pcmx_region3d_slab_workspace_bytes(dim, nz));
    int launches = 0;
    check_rc(pcmx_region3d_grow_slab(data.data_ptr<uint8_t>() + plane, region.data_ptr<uint8_t>() + plane, dim, nz,
                                     (int)halos, (int)thr, ws.data_ptr(), (int)batch, (int)max_launches, cur_stream(data),
                                     &launches),
             "region3d_grow_slab_");
    return launches;
}

// ---------------------------------------------------------------- volume + ray casting
void check_cubic(const at::Tensor& v, const char* what) {
    TORCH_CHECK(v.dim() == 3 && v.size(0) == v.size(1) && v.size(1) == v.size(2) && v.size(0) > 1, what,
                ": a cubic (dim, dim, dim) volume with dim > 1");
}

at::Tensor volume_gen_(at::Tensor data, int64_t seed) {
    check_u8_gpu(data, "data");
    check_cubic(data, "volume_gen_");
    const at::DeviceGuard g(data.device());
    check_rc(pcmx_volume_gen_u8(data.data_ptr<uint8_t>(), (int)data.size(0), (unsigned)seed, cur_stream(data)), "volume_gen_");
    return data;
}

at::Tensor volume_gen_slab_(at::Tensor data, int64_t z_first, int64_t seed) {
    check_u8_gpu(data, "data");
    TORCH_CHECK(data.dim() == 3 && data.size(1) == data.size(2) && data.size(0) >= 1,
                "volume_gen_slab_: (nplanes, dim, dim) uint8");
    const at::DeviceGuard g(data.device());
    check_rc(pcmx_volume_gen_slab_u8(data.data_ptr<uint8_t>(), (int)data.size(1), (int)z_first, (int)data.size(0),
                                     (unsigned)seed, cur_stream(data)),
             "volume_gen_slab_");
    return data;
}

std::vector<float> cam_vec(at::ArrayRef<double> cam12) {
    TORCH_CHECK(cam12.size() == 12, "camera: 12 floats (camera, forward, right, up)");
    std::vector<float> c(12);
    for (int i = 0; i < 12; ++i) c[i] = (float)cam12[i];
    return c;
}

at::Tensor raycast_global(const at::Tensor& data, const at::Tensor& region, int64_t image_dim, at::ArrayRef<double> cam12,
                          double pixel_width, double step, int64_t max_steps, bool f64_color, int64_t variant) {
    check_u8_gpu(data, "data"), check_u8_gpu(region, "region");
    check_cubic(data, "raycast_global");
    TORCH_CHECK(region.sizes() == data.sizes() && region.device() == data.device(),
                "raycast_global: region must match data's shape and device");
    TORCH_CHECK(image_dim > 0, "raycast_global: image_dim > 0");
    const at::DeviceGuard g(data.device());
    auto img = at::empty({image_dim, image_dim}, data.options());
    auto c = cam_vec(cam12);
    if (variant < 0) {  // the production rule (pcmx_raycast_global): 16-lane groups, DR16 + 4-lane groups above 2^16 rays
        variant = (image_dim * image_dim > (1 << 16) && data.size(0) % 4 == 0) ? 11 : 6;
    }
    if (variant >= 9) {  // the DR16 layout (data and region interleaved per voxel), packed on this call
        const int dim = (int)data.size(0);
        TORCH_CHECK(dim % 4 == 0, "raycast_global: DR16 variants need dim % 4 == 0");
        auto dr = at::empty({pcmx_raycast_dr16_bytes(dim)}, data.options());
        check_rc(pcmx_raycast_dr16_pack(data.data_ptr<uint8_t>(), region.data_ptr<uint8_t>(), dim, dr.data_ptr(),
                                        cur_stream(data)),
                 "raycast_dr16_pack");
        check_rc(pcmx_raycast_global_dr(dr.data_ptr(), dim, img.data_ptr<uint8_t>(), (int)image_dim, c.data(),
                                        (float)pixel_width, (float)step, (int)max_steps, f64_color ? 1 : 0, (int)variant,
                                        cur_stream(data)),
                 "raycast_global_dr");
        return img;
    }
    check_rc(pcmx_raycast_global_variant(data.data_ptr<uint8_t>(), region.data_ptr<uint8_t>(), (int)data.size(0),
                                         img.data_ptr<uint8_t>(), (int)image_dim, c.data(), (float)pixel_width, (float)step,
                                         (int)max_steps, f64_color ? 1 : 0, (int)variant, cur_stream(data)),
             "raycast_global");
    return img;
}

// slab buffers (nz + 2, dim, dim) starting at global plane z0 - 1; state int32 [image_dim^2, 6]
at::Tensor raycast_slab_(const at::Tensor& data, const at::Tensor& region, int64_t z0, at::Tensor state, bool init,
                         bool bottom, int64_t image_dim, at::ArrayRef<double> cam12, double pixel_width, double step,
                         int64_t max_steps) {
    check_u8_gpu(data, "data"), check_u8_gpu(region, "region");
    check_gpu(state, "state", at::kInt);
    TORCH_CHECK(data.dim() == 3 && data.size(1) == data.size(2) && data.size(0) >= 3 && region.sizes() == data.sizes(),
                "raycast_slab_: (nz + 2, dim, dim) uint8 slabs");
    TORCH_CHECK(state.is_contiguous() && state.numel() == image_dim * image_dim * 6 && state.device() == data.device(),
                "raycast_slab_: state int32 [image_dim^2, 6] on data's device");
    const int dim = (int)data.size(1);
    TORCH_CHECK(z0 >= 0 && z0 + data.size(0) - 2 <= dim, "raycast_slab_: slab planes inside the volume");
    const at::DeviceGuard g(data.device());
    auto img = at::empty({bottom ? image_dim : 0, bottom ? image_dim : 0}, data.options());
    auto c = cam_vec(cam12);
    check_rc(pcmx_raycast_slab(data.data_ptr<uint8_t>(), region.data_ptr<uint8_t>(), dim, (int)z0, state.data_ptr<int>(),
                               init ? 1 : 0, bottom ? 1 : 0, bottom ? img.data_ptr<uint8_t>() : nullptr, (int)image_dim,
                               c.data(), (float)pixel_width, (float)step, (int)max_steps, cur_stream(data)),
             "raycast_slab_");
    return img;
}

at::Tensor brick_pack(const at::Tensor& data, const at::Tensor& region) {
    check_u8_gpu(data, "data"), check_u8_gpu(region, "region");
    const at::DeviceGuard g(data.device());
    TORCH_CHECK(data.dim() == 3 && data.sizes() == region.sizes() && data.size(0) == data.size(1) &&
                    data.size(0) == data.size(2) && data.size(0) <= 2048 && data.is_contiguous() && region.is_contiguous(),
                "brick_pack: contiguous cubic volumes, dim <= 2048");
    auto tex = at::empty({data.numel() * 2 + 2}, data.options().dtype(at::kLong));  // texels + format flag
    check_rc(pcmx_brick_pack(data.data_ptr<uint8_t>(), region.data_ptr<uint8_t>(), (int)data.size(0), tex.data_ptr(),
                             cur_stream(data)),
             "brick_pack");
    return tex;
}

at::Tensor raycast_bricked(const at::Tensor& tex, int64_t image_dim, at::ArrayRef<double> cam12, double pixel_width,
                           double step, int64_t max_steps, int64_t batch, int64_t segments) {
    check_gpu(tex, "tex", at::kLong);
    TORCH_CHECK(tex.dim() == 1 && tex.numel() >= 18 && tex.is_contiguous(), "raycast_bricked: tex from brick_pack");
    const int64_t nvox = (tex.numel() - 2) / 2;
    int64_t dim = (int64_t)std::llround(std::cbrt((double)nvox));
    TORCH_CHECK(dim * dim * dim == nvox, "raycast_bricked: tex from brick_pack of a cubic volume");
    const at::DeviceGuard g(tex.device());
    auto img = at::empty({image_dim, image_dim}, tex.options().dtype(at::kByte));
    auto c = cam_vec(cam12);
    check_rc(pcmx_raycast_bricked(tex.data_ptr(), (int)dim,
                                  img.data_ptr<uint8_t>(), (int)image_dim, c.data(), (float)pixel_width, (float)step,
                                  (int)max_steps, (int)batch, (int)segments, cur_stream(tex)),
             "raycast_bricked");
    return img;
}

// ---------------------------------------------------------------- stencil
void stencil5_(const at::Tensor& u, at::Tensor out, int64_t r0, int64_t r1, int64_t global_row0, int64_t global_rows,
               double k) {
    check_gpu(u, "u", at::kBFloat16), check_gpu(out, "out", at::kBFloat16);
    TORCH_CHECK(u.dim() == 2 && u.sizes() == out.sizes() && u.is_contiguous() && out.is_contiguous(),
                "stencil5: slabs of shape (rows+2, cols)");
    const at::DeviceGuard g(u.device());
    const int rows = (int)u.size(0) - 2, cols = (int)u.size(1);
    check_rc(pcmx_stencil5_bf16(u.data_ptr(), out.data_ptr(), rows, cols, cols, (int)r0, (int)r1, global_row0, global_rows,
                                (float)k, cur_stream(u)),
             "stencil5_");
}

void stencil5xT_(const at::Tensor& u, at::Tensor out, int64_t halo, int64_t steps, int64_t r0, int64_t r1,
                 int64_t global_row0, int64_t global_rows, double k, int64_t shape) {
    check_gpu(u, "u", at::kBFloat16), check_gpu(out, "out", at::kBFloat16);
    TORCH_CHECK(u.dim() == 2 && u.sizes() == out.sizes() && u.is_contiguous() && out.is_contiguous() && halo >= 1 &&
                    u.size(0) > 2 * halo,
                "stencil5xT: slabs of shape (rows + 2*halo, cols)");
    const at::DeviceGuard g(u.device());
    const int rows = (int)(u.size(0) - 2 * halo), cols = (int)u.size(1);
    check_rc(pcmx_stencil5xT_bf16_spans_shape(u.data_ptr(), out.data_ptr(), rows, cols, cols, (int)halo, (int)steps,
                                              (int)r0, (int)r1, 0, 0, global_row0, global_rows, (float)k, (int)shape,
                                              cur_stream(u)),
             "stencil5xT_");
}

void stencil5xT_spans_(const at::Tensor& u, at::Tensor out, int64_t halo, int64_t steps, int64_t r0a, int64_t r1a,
                       int64_t r0b, int64_t r1b, int64_t global_row0, int64_t global_rows, double k, int64_t shape) {
    check_gpu(u, "u", at::kBFloat16), check_gpu(out, "out", at::kBFloat16);
    TORCH_CHECK(u.dim() == 2 && u.sizes() == out.sizes() && u.is_contiguous() && out.is_contiguous() && halo >= 1 &&
                    u.size(0) > 2 * halo,
                "stencil5xT_spans: slabs of shape (rows + 2*halo, cols)");
    const at::DeviceGuard g(u.device());
    const int rows = (int)(u.size(0) - 2 * halo), cols = (int)u.size(1);
    check_rc(pcmx_stencil5xT_bf16_spans_shape(u.data_ptr(), out.data_ptr(), rows, cols, cols, (int)halo, (int)steps,
                                              (int)r0a, (int)r1a, (int)r0b, (int)r1b, global_row0, global_rows, (float)k,
                                              (int)shape, cur_stream(u)),
             "stencil5xT_spans_");
}

// ---------------------------------------------------------------- SpMV
at::Tensor spmv_csr(const at::Tensor& row_ptr, const at::Tensor& col, const at::Tensor& val, const at::Tensor& x,
                    const at::Tensor& items) {
    check_gpu(row_ptr, "row_ptr", at::kLong), check_gpu(col, "col", at::kInt), check_gpu(val, "val", at::kFloat);
    check_gpu(x, "x", at::kFloat), check_gpu(items, "items", at::kLong);
    const at::DeviceGuard g(val.device());
    const int n_rows = (int)row_ptr.numel() - 1;
    auto y = at::empty({n_rows}, val.options());
    check_rc(pcmx_spmv_csr((const long long*)row_ptr.data_ptr<int64_t>(), col.data_ptr<int>(), val.data_ptr<float>(), x.data_ptr<float>(),
                           y.data_ptr<float>(), n_rows, items.data_ptr(), items.size(0), cur_stream(val)),
             "spmv_csr");
    return y;
}

// out[n_rows, k] = A x[n_cols, k] (spmm.hip). x and out are 2-D f32 views with unit column stride, read and written
// where they lie; items / slot / split: the plan of spmm_csr_plan(row_ptr, item_nnz), n_pieces its workspace rows. The
// workspace comes from torch's allocator on the current stream.
at::Tensor spmm_csr(const at::Tensor& row_ptr, const at::Tensor& col, const at::Tensor& val, const at::Tensor& x,
                    const at::Tensor& items, const at::Tensor& slot, const at::Tensor& split, int64_t n_pieces,
                    int64_t item_nnz, at::Tensor out) {
    check_gpu(row_ptr, "row_ptr", at::kLong), check_gpu(col, "col", at::kInt), check_gpu(val, "val", at::kFloat);
    check_gpu(x, "x", at::kFloat), check_gpu(out, "out", at::kFloat), check_gpu(items, "items", at::kLong);
    check_gpu(slot, "slot", at::kInt), check_gpu(split, "split", at::kInt);
    const int64_t n_rows = row_ptr.numel() - 1;
    TORCH_CHECK(x.dim() == 2 && out.dim() == 2 && out.size(0) == n_rows && out.size(1) == x.size(1),
                "spmm_csr: x [n_cols, k] and out [n_rows, k]");
    const int64_t k = x.size(1);
    TORCH_CHECK((k <= 1 || (x.stride(1) == 1 && out.stride(1) == 1)), "spmm_csr: x and out need a unit column stride");
    TORCH_CHECK(row_ptr.is_contiguous() && col.is_contiguous() && val.is_contiguous() && items.is_contiguous() &&
                    slot.is_contiguous() && split.is_contiguous() && items.dim() == 2 && items.size(1) == 3 &&
                    slot.numel() == items.size(0) && (split.numel() == 0 || (split.dim() == 2 && split.size(1) == 3)),
                "spmm_csr: contiguous CSR arrays and plan (items [n, 3], slot [n], split [s, 3])");
    TORCH_CHECK(n_pieces >= 0 && n_rows < (1LL << 31) && k < (1LL << 31), "spmm_csr: sizes");
    const at::DeviceGuard g(val.device());
    // a dimension of size <= 1 carries an arbitrary stride
    const int64_t ldx = x.size(0) > 1 ? x.stride(0) : std::max<int64_t>(x.stride(0), k);
    const int64_t ldy = n_rows > 1 ? out.stride(0) : std::max<int64_t>(out.stride(0), k);
    const int64_t ws_floats = n_pieces * ((k + 3) & ~int64_t(3));
    auto ws = at::empty({ws_floats}, val.options());
    check_rc(pcmx_spmm_csr((const long long*)row_ptr.data_ptr<int64_t>(), col.data_ptr<int>(), val.data_ptr<float>(),
                           x.data_ptr<float>(), ldx, out.data_ptr<float>(), ldy, (int)n_rows, (int)k, items.data_ptr(),
                           items.size(0), slot.data_ptr<int>(), split.data_ptr<int>(),
                           split.numel() ? (int)split.size(0) : 0, n_pieces, (int)item_nnz,
                           ws_floats ? ws.data_ptr<float>() : nullptr, ws_floats, cur_stream(val)),
             "spmm_csr");
    return out;
}

namespace {
// the named launch options of the sliced ops, refused here before anything is launched or written
void check_sliced_options(const char* op, int64_t item_nnz, bool packed, int64_t blocks_per_cu) {
    TORCH_CHECK(item_nnz == 1024 || item_nnz == 512 || (packed && (item_nnz == 384 || item_nnz == 256)), op,
                ": item_nnz must be 512 or 1024 (256 or 384 with the packed layout), got ", item_nnz);
    TORCH_CHECK(blocks_per_cu >= 0 && blocks_per_cu <= 255, op, ": blocks_per_cu must be 0 (default) .. 255, got ",
                blocks_per_cu);
}
}  // namespace

// XCD-sliced CSR (see spmv.hip): meta is a CPU int64 tensor [nz0 (S) | item0 (S + 1) | out0 (S + 1)]; ypart (every
// compact partial) and extra [n_items] are caller-owned scratch. packed: col holds one word per nonzero (column offset
// + head flag + row offset; lrow unused) and meta ends with colbase (S). stage: 0 all, 1 products only, 2 combine +
// fix-up only (PCMX_SPMV_*); phase_n 0: all phases from phase_lo.
at::Tensor spmv_sliced(const at::Tensor& lrow, const at::Tensor& col, const at::Tensor& val, const at::Tensor& x,
                       const at::Tensor& items, const at::Tensor& row_mask, const at::Tensor& chunk_base,
                       const at::Tensor& fix, const at::Tensor& meta, at::Tensor ypart, at::Tensor extra, int64_t n_rows,
                       const c10::optional<at::Tensor>& out, bool packed, int64_t item_nnz, int64_t stage,
                       bool ballot_combine, int64_t blocks_per_cu, int64_t phase_lo, int64_t phase_n) {
    check_gpu(lrow, "lrow", at::kShort), check_gpu(col, "col", at::kInt), check_gpu(val, "val", at::kFloat);
    check_gpu(x, "x", at::kFloat), check_gpu(items, "items", at::kLong), check_gpu(fix, "fix", at::kInt);
    check_gpu(ypart, "ypart", at::kFloat), check_gpu(extra, "extra", at::kFloat);
    check_gpu(row_mask, "row_mask", at::kInt), check_gpu(chunk_base, "chunk_base", at::kInt);
    TORCH_CHECK(!meta.is_cuda() && meta.scalar_type() == at::kLong && meta.is_contiguous(), "spmv_sliced: CPU int64 meta");
    check_sliced_options("spmv_sliced", item_nnz, packed, blocks_per_cu);
    TORCH_CHECK(stage == PCMX_SPMV_ALL || stage == PCMX_SPMV_PRODUCTS || stage == PCMX_SPMV_COMBINE,
                "spmv_sliced: stage must be 0 (all), 1 (products) or 2 (combine), got ", stage);
    const int64_t S = (meta.numel() - 2) / (packed ? 4 : 3);
    TORCH_CHECK(meta.numel() == (packed ? 4 : 3) * S + 2 && S >= 8 && S % 8 == 0 && S <= PCMX_SPMV_MAX_SLICES,
                "spmv_sliced: 8, 16, 24 or 32 slices");
    const int64_t* m = meta.data_ptr<int64_t>();
    const int64_t* out0 = m + 2 * S + 1;
    TORCH_CHECK(phase_lo >= 0 && phase_n >= 0 && phase_lo + phase_n <= S / 8 && phase_lo < S / 8,
                "spmv_sliced: phases [", phase_lo, ", ", phase_lo + phase_n, ") outside the ", S / 8, " phases");
    TORCH_CHECK((packed || lrow.numel() == col.numel()) && val.numel() == col.numel(), "spmv_sliced: lrow / val shape");
    std::vector<int> colbase;
    if (packed) {
        for (int64_t k = 0; k < S; ++k) {
            TORCH_CHECK(m[3 * S + 2 + k] >= 0 && m[3 * S + 2 + k] < x.numel(), "spmv_sliced: packed column base");
            colbase.push_back((int)m[3 * S + 2 + k]);
        }
    }
    TORCH_CHECK(row_mask.numel() >= n_rows && chunk_base.numel() >= ((n_rows + 63) / 64) * S,
                "spmv_sliced: row_mask / chunk_base shape");
    TORCH_CHECK(out0[0] == 0 && ypart.numel() >= out0[S], "spmv_sliced: ypart must hold every compact partial");
    TORCH_CHECK(x.numel() < (int64_t(1) << 30), "spmv_sliced: x must be < 2^30 elements (32-bit buffer offsets)");
    TORCH_CHECK(m[S] >= 0 && m[2 * S] <= items.size(0) && extra.numel() >= items.size(0), "spmv_sliced: items/extra shape");
    TORCH_CHECK(fix.dim() == 2 && fix.size(1) == 2, "spmv_sliced: fix [k, 2]");
    for (int64_t k = 0; k < S; ++k)
        TORCH_CHECK(m[k] >= 0 && m[k] <= col.numel() && m[S + k] <= m[S + k + 1] && out0[k] <= out0[k + 1],
                    "spmv_sliced: meta");
    const at::DeviceGuard g(val.device());
    at::Tensor y;
    if (out.has_value()) {
        y = *out;
        check_gpu(y, "out", at::kFloat);
        TORCH_CHECK(y.is_contiguous() && y.numel() >= n_rows && y.device() == val.device(),
                    "spmv_sliced: out must be a contiguous float32 tensor of >= n_rows elements on val's device");
    } else {
        y = at::empty({n_rows}, val.options());
    }
    check_rc(pcmx_spmv_sliced(reinterpret_cast<const unsigned short*>(lrow.numel() ? lrow.data_ptr<int16_t>() : nullptr),
                              col.data_ptr<int>(),
                              val.data_ptr<float>(), x.data_ptr<float>(), ypart.data_ptr<float>(), extra.data_ptr<float>(),
                              y.data_ptr<float>(), (int)n_rows, (int)x.numel(), (int)S, (const long long*)m,
                              (const long long*)m + S, (const long long*)out0, items.data_ptr(),
                              reinterpret_cast<const unsigned*>(row_mask.data_ptr<int>()), chunk_base.data_ptr<int>(),
                              fix.data_ptr(), (int)fix.size(0), (int)item_nnz, (int)stage, (int)ballot_combine,
                              (int)blocks_per_cu, (int)phase_lo, (int)phase_n, packed ? colbase.data() : nullptr,
                              cur_stream(val)),
             "spmv_sliced");
    return y;
}

// Products only of phases [a_lo, a_lo + a_n) of sliced matrix A and [b_lo, b_lo + b_n) of B (same x), ONE launch
// (pcmx_spmv_sliced_pair). meta_*: the packed spmv_sliced meta (nz0 S | item0 S + 1 | out0 S + 1 | colbase S).
void spmv_sliced_pair(const at::Tensor& x, int64_t item_nnz, int64_t blocks_per_cu, const at::Tensor& col_a,
                      const at::Tensor& val_a, const at::Tensor& items_a, const at::Tensor& meta_a, at::Tensor ypart_a,
                      at::Tensor extra_a, int64_t s_a, int64_t a_lo, int64_t a_n, const at::Tensor& col_b,
                      const at::Tensor& val_b, const at::Tensor& items_b, const at::Tensor& meta_b, at::Tensor ypart_b,
                      at::Tensor extra_b, int64_t s_b, int64_t b_lo, int64_t b_n) {
    check_gpu(x, "x", at::kFloat);
    check_sliced_options("spmv_sliced_pair", item_nnz, true, blocks_per_cu);
    TORCH_CHECK(x.numel() < (int64_t(1) << 30), "spmv_sliced_pair: x must be < 2^30 elements");
    auto chk = [&](const at::Tensor& col, const at::Tensor& val, const at::Tensor& items, const at::Tensor& meta,
                   const at::Tensor& ypart, const at::Tensor& extra, int64_t S, int64_t lo, int64_t n) {
        check_gpu(col, "col", at::kInt), check_gpu(val, "val", at::kFloat), check_gpu(items, "items", at::kLong);
        check_gpu(ypart, "ypart", at::kFloat), check_gpu(extra, "extra", at::kFloat);
        TORCH_CHECK(col.device() == x.device() && val.numel() == col.numel(), "spmv_sliced_pair: col / val");
        TORCH_CHECK(S >= 8 && S % 8 == 0 && S <= PCMX_SPMV_MAX_SLICES && lo >= 0 && n >= 0 && 8 * (lo + n) <= S,
                    "spmv_sliced_pair: slices / phases");
        TORCH_CHECK(!meta.is_cuda() && meta.scalar_type() == at::kLong && meta.is_contiguous() && meta.numel() == 4 * S + 2,
                    "spmv_sliced_pair: packed CPU int64 meta");
        const int64_t* m = meta.data_ptr<int64_t>();
        const int64_t* out0 = m + 2 * S + 1;
        TORCH_CHECK(out0[0] == 0 && ypart.numel() >= out0[S] && m[2 * S] <= items.size(0) && extra.numel() >= items.size(0),
                    "spmv_sliced_pair: ypart / items / extra shape");
        for (int64_t k = 0; k < S; ++k)
            TORCH_CHECK(m[k] >= 0 && m[k] <= col.numel() && m[S + k] <= m[S + k + 1] && m[3 * S + 2 + k] >= 0 &&
                            m[3 * S + 2 + k] < x.numel(),
                        "spmv_sliced_pair: meta");
    };
    chk(col_a, val_a, items_a, meta_a, ypart_a, extra_a, s_a, a_lo, a_n);
    chk(col_b, val_b, items_b, meta_b, ypart_b, extra_b, s_b, b_lo, b_n);
    TORCH_CHECK(8 * (a_n + b_n) <= PCMX_SPMV_MAX_SLICES, "spmv_sliced_pair: at most 32 slices per launch");
    auto cb = [](const at::Tensor& meta, int64_t S) {
        std::vector<int> v(S);
        for (int64_t k = 0; k < S; ++k) v[k] = (int)meta.data_ptr<int64_t>()[3 * S + 2 + k];
        return v;
    };
    const auto cba = cb(meta_a, s_a), cbb = cb(meta_b, s_b);
    const int64_t *ma = meta_a.data_ptr<int64_t>(), *mb = meta_b.data_ptr<int64_t>();
    const at::DeviceGuard g(x.device());
    check_rc(pcmx_spmv_sliced_pair(x.data_ptr<float>(), (int)x.numel(), (int)item_nnz, (int)blocks_per_cu, col_a.data_ptr<int>(),
                                   val_a.data_ptr<float>(), items_a.data_ptr(), ypart_a.data_ptr<float>(),
                                   extra_a.data_ptr<float>(), (int)s_a, (const long long*)ma, (const long long*)ma + s_a,
                                   (const long long*)ma + 2 * s_a + 1, cba.data(), (int)a_lo, (int)a_n,
                                   col_b.data_ptr<int>(), val_b.data_ptr<float>(), items_b.data_ptr(),
                                   ypart_b.data_ptr<float>(), extra_b.data_ptr<float>(), (int)s_b, (const long long*)mb,
                                   (const long long*)mb + s_b, (const long long*)mb + 2 * s_b + 1, cbb.data(), (int)b_lo,
                                   (int)b_n, cur_stream(x)),
             "spmv_sliced_pair");
}

// The combine + fix-up (+ send-buffer pack) of the partials a products-only spmv_sliced call (stage 1) wrote, in one
// launch (pcmx_spmv_sliced_combine). meta: the spmv_sliced meta of the same matrix (out0 at [2S + 1, 3S + 2)).
void spmv_sliced_combine(const at::Tensor& ypart, const at::Tensor& row_mask, const at::Tensor& chunk_base,
                         const at::Tensor& meta, int64_t n_slices, const at::Tensor& extra, const at::Tensor& fix,
                         const c10::optional<at::Tensor>& fix_chunk0, at::Tensor out, int64_t n_rows,
                         const c10::optional<at::Tensor>& send_ptr, const c10::optional<at::Tensor>& send_slot,
                         const c10::optional<at::Tensor>& sendbuf) {
    check_gpu(ypart, "ypart", at::kFloat), check_gpu(extra, "extra", at::kFloat), check_gpu(fix, "fix", at::kInt);
    check_gpu(row_mask, "row_mask", at::kInt), check_gpu(chunk_base, "chunk_base", at::kInt);
    check_gpu(out, "out", at::kFloat);
    const int64_t S = n_slices;
    TORCH_CHECK(S >= 8 && S % 8 == 0 && S <= PCMX_SPMV_MAX_SLICES, "spmv_sliced_combine: 8, 16, 24 or 32 slices");
    TORCH_CHECK(!meta.is_cuda() && meta.scalar_type() == at::kLong && meta.is_contiguous() && meta.numel() >= 3 * S + 2,
                "spmv_sliced_combine: CPU int64 meta");
    const int64_t* out0 = meta.data_ptr<int64_t>() + 2 * S + 1;
    const int64_t chunks = (n_rows + 63) / 64;
    TORCH_CHECK(row_mask.numel() >= n_rows && chunk_base.numel() >= chunks * S, "spmv_sliced_combine: row_mask / chunk_base");
    TORCH_CHECK(out0[0] == 0 && ypart.numel() >= out0[S], "spmv_sliced_combine: ypart must hold every compact partial");
    TORCH_CHECK(out.is_contiguous() && out.numel() >= n_rows && out.device() == ypart.device(), "spmv_sliced_combine: out");
    TORCH_CHECK(fix.dim() == 2 && fix.size(1) == 2, "spmv_sliced_combine: fix [k, 2]");
    const int* fc = nullptr;
    if (fix_chunk0.has_value() && fix.size(0) > 0) {
        check_gpu(*fix_chunk0, "fix_chunk0", at::kInt);
        TORCH_CHECK(fix_chunk0->is_contiguous() && fix_chunk0->numel() >= chunks + 1, "spmv_sliced_combine: fix_chunk0");
        fc = fix_chunk0->data_ptr<int>();
    } else {
        TORCH_CHECK(fix.size(0) == 0, "spmv_sliced_combine: split rows need fix_chunk0");
    }
    const int *sp = nullptr, *ss = nullptr;
    float* sb = nullptr;
    if (send_ptr.has_value()) {
        // INTERNAL op: the list CONTENTS (send_ptr rising from 0 to send_slot.numel(), every slot inside sendbuf) are
        // device data; checking them here would sync every call, so SlicedCSR._check_send (the only caller,
        // ops/sparse.py) validates each set of lists once. Shapes and dtypes are checked here.
        TORCH_CHECK(send_slot.has_value() && sendbuf.has_value(), "spmv_sliced_combine: send_ptr needs send_slot and sendbuf");
        check_gpu(*send_ptr, "send_ptr", at::kInt), check_gpu(*send_slot, "send_slot", at::kInt);
        check_gpu(*sendbuf, "sendbuf", at::kFloat);
        TORCH_CHECK(send_ptr->is_contiguous() && send_ptr->numel() >= n_rows + 1 && send_slot->is_contiguous() &&
                        sendbuf->is_contiguous() && send_slot->numel() <= sendbuf->numel(),
                    "spmv_sliced_combine: send lists");
        if (send_slot->numel() > 0)  // (no peer references any row, e.g. one rank: nothing to pack)
            sp = send_ptr->data_ptr<int>(), ss = send_slot->data_ptr<int>(), sb = sendbuf->data_ptr<float>();
    }
    const at::DeviceGuard g(ypart.device());
    check_rc(pcmx_spmv_sliced_combine(ypart.data_ptr<float>(), reinterpret_cast<const unsigned*>(row_mask.data_ptr<int>()),
                                      chunk_base.data_ptr<int>(), (const long long*)out0, (int)S, out.data_ptr<float>(),
                                      (int)n_rows, extra.data_ptr<float>(), fix.data_ptr(), fc, sp, ss, sb,
                                      cur_stream(ypart)),
             "spmv_sliced_combine");
}

at::Tensor spmv_banded(const at::Tensor& vals, const at::Tensor& row_off, int64_t n, int64_t a, int64_t b, int64_t c,
                       int64_t d, int64_t e, const at::Tensor& x, int64_t variant) {
    check_gpu(vals, "vals", at::kFloat), check_gpu(row_off, "row_off", at::kLong), check_gpu(x, "x", at::kFloat);
    TORCH_CHECK(vals.is_contiguous() && row_off.is_contiguous() && x.is_contiguous(), "spmv_banded: contiguous tensors");
    TORCH_CHECK(row_off.numel() >= n && x.numel() >= n, "spmv_banded: row_off and x need n entries");
    const at::DeviceGuard g(vals.device());
    auto y = at::empty({n}, vals.options());
    check_rc(pcmx_spmv_banded_variant(vals.data_ptr<float>(), (const long long*)row_off.data_ptr<int64_t>(), (int)n, (int)a,
                                      (int)b, (int)c, (int)d, (int)e, x.data_ptr<float>(), y.data_ptr<float>(), (int)variant,
                                      cur_stream(vals)),
             "spmv_banded");
    return y;
}

// ---------------------------------------------------------------- halo pack/unpack
at::Tensor pack_edges(const at::Tensor& tile) {
    TORCH_CHECK(tile.is_cuda() && tile.dim() == 2 && tile.is_contiguous(), "pack_edges: contiguous padded 2-D GPU tile");
    const at::DeviceGuard g(tile.device());
    const int H = (int)tile.size(0) - 2, W = (int)tile.size(1) - 2;
    auto buf = at::empty({2 * W + 2 * H}, tile.options());
    check_rc(pcmx_pack_edges(tile.data_ptr(), (int)tile.element_size(), H, W, (int)tile.size(1), buf.data_ptr(), cur_stream(tile)),
             "pack_edges");
    return buf;
}

void unpack_halo_(at::Tensor tile, const at::Tensor& buf, int64_t mask, const c10::optional<at::Tensor>& changed) {
    TORCH_CHECK(tile.is_cuda() && tile.dim() == 2 && tile.is_contiguous() && buf.dtype() == tile.dtype(), "unpack_halo_");
    TORCH_CHECK(buf.is_cuda() && buf.is_contiguous() && buf.device() == tile.device(), "unpack_halo_: buf on tile's device");
    const at::DeviceGuard g(tile.device());
    const int H = (int)tile.size(0) - 2, W = (int)tile.size(1) - 2;
    TORCH_CHECK(buf.numel() == 2 * W + 2 * H, "unpack_halo_: buffer size");
    int* flag = nullptr;
    if (changed.has_value()) {
        check_gpu(*changed, "changed", at::kInt);
        TORCH_CHECK(changed->numel() >= 1 && changed->device() == tile.device(), "unpack_halo_: changed flag");
        flag = changed->data_ptr<int>();
    }
    check_rc(pcmx_unpack_halo_changed(tile.data_ptr(), (int)tile.element_size(), H, W, (int)tile.size(1), buf.data_ptr(),
                                      (int)mask, flag, cur_stream(tile)),
             "unpack_halo_");
}

// host-side CSR analysis (CPU int64 row_ptr -> int64 [n_items, 3] work items)
at::Tensor spmv_csr_plan(const at::Tensor& row_ptr, int64_t item_nnz) {
    TORCH_CHECK(!row_ptr.is_cuda() && row_ptr.scalar_type() == at::kLong, "spmv_csr_plan: CPU int64 row_ptr");
    auto rp = row_ptr.contiguous();
    const int n_rows = (int)rp.numel() - 1;
    const long long k = pcmx_spmv_csr_plan_nnz((const long long*)rp.data_ptr<int64_t>(), n_rows, nullptr, 0, (int)item_nnz);
    TORCH_CHECK(k >= 0, "spmv_csr_plan: item_nnz must be a multiple of 64 in [64, 1024]");
    auto items = at::empty({k, 3}, rp.options());
    pcmx_spmv_csr_plan_nnz((const long long*)rp.data_ptr<int64_t>(), n_rows, items.data_ptr(), k, (int)item_nnz);
    return items;
}

// the SpMM plan of a CPU int64 row_ptr: (items [n, 3] int64, slot [n] int32, split [s, 3] int32). A piece of a split
// row (a one-row item that is not the whole row) takes the next workspace slot, so the pieces of one row hold
// consecutive slots in piece order; split lists {row, first slot, pieces} per split row; every other item has slot -1.
std::tuple<at::Tensor, at::Tensor, at::Tensor> spmm_csr_plan(const at::Tensor& row_ptr, int64_t item_nnz) {
    auto items = spmv_csr_plan(row_ptr, item_nnz);
    auto rp = row_ptr.contiguous();
    const int64_t* p = rp.data_ptr<int64_t>();
    const int64_t n = items.size(0);
    const int64_t* it = items.data_ptr<int64_t>();
    auto slot = at::empty({n}, rp.options().dtype(at::kInt));
    int* sl = slot.data_ptr<int>();
    std::vector<int> split;
    int64_t pieces = 0;
    for (int64_t i = 0; i < n; ++i) {
        const int64_t row0 = it[3 * i] & 0xFFFFFFFFLL, row1 = it[3 * i] >> 32;
        const bool piece = row1 == row0 + 1 && (it[3 * i + 1] != p[row0] || it[3 * i + 2] != p[row0 + 1]);
        sl[i] = piece ? (int)pieces : -1;
        if (!piece) continue;
        TORCH_CHECK(pieces < (1LL << 31) - 1, "spmm_csr_plan: too many pieces");
        if (it[3 * i + 1] == p[row0])
            split.insert(split.end(), {(int)row0, (int)pieces, 1});
        else
            ++split.back();
        ++pieces;
    }
    auto sp = at::empty({(int64_t)split.size() / 3, 3}, slot.options());
    std::copy(split.begin(), split.end(), sp.data_ptr<int>());
    return {items, slot, sp};
}

}  // namespace

TORCH_LIBRARY(pcmx, m) {
    m.def("vmul(Tensor a, Tensor b) -> Tensor");
    m.def("vadd(Tensor a, Tensor b) -> Tensor");
    m.def("axpy_(Tensor(a!) y, float alpha, Tensor x) -> Tensor(a!)");
    m.def("gather_(Tensor src, Tensor idx, Tensor(a!) out) -> Tensor(a!)");
    m.def("fill_(Tensor(a!) x, float v) -> Tensor(a!)");
    m.def("copy_(Tensor(a!) dst, Tensor src) -> Tensor(a!)");
    m.def("rand_uniform_(Tensor(a!) x, int seed, float lo, float hi) -> Tensor(a!)");
    m.def("reduce(Tensor x, int op) -> Tensor");
    m.def("dot(Tensor a, Tensor b) -> Tensor");
    m.def("scan(Tensor x, bool exclusive=False, Tensor? init=None) -> Tensor");
    m.def("scan_out(Tensor x, Tensor(a!) out, bool exclusive=False, Tensor? init=None) -> Tensor(a!)");
    m.def("scan_check(int device=0) -> ()", scan_check);
    m.def("select(Tensor x, Tensor mask, Tensor(a!)? out=None) -> (Tensor, Tensor)");
    m.def("select_index(Tensor mask, Tensor(a!)? out=None) -> (Tensor, Tensor)");
    m.def("select_if(Tensor x, int op, float threshold, bool indices=False, Tensor(a!)? out=None) -> (Tensor, Tensor)");
    m.def("sort_keys(Tensor keys, bool descending=False, int begin_bit=0, int end_bit=32) -> Tensor");
    m.def("sort_pairs(Tensor keys, Tensor values, bool descending=False, int begin_bit=0, int end_bit=32) -> (Tensor, Tensor)");
    m.def("sort_index(Tensor keys, bool descending=False, int begin_bit=0, int end_bit=32, bool want_keys=True) -> (Tensor, Tensor)");
    m.def("topk(Tensor x, int k, bool largest=True, bool sorted=True) -> (Tensor, Tensor)");
    m.def("kth_value(Tensor x, int k, bool largest=False) -> Tensor");
    m.def("row_sort(Tensor keys, Tensor? values, int keep, int mode, bool descending=False, int begin_bit=0, int end_bit=32, bool want_keys=True) -> (Tensor, Tensor)");
    m.def("row_topk(Tensor x, int k, bool largest=True) -> (Tensor, Tensor)");
    m.def("row_kth(Tensor x, int k, bool largest=False) -> Tensor");
    m.def("axis_reduce(Tensor x, int op, int route=0, int chunk=0) -> Tensor");
    m.def("axis_scan(Tensor x, int op, bool exclusive=False, int route=0, int chunk=0, Tensor(a!)? out=None) -> Tensor");
    m.def("run_length_encode(Tensor keys, bool starts=False, Tensor(a!)? out_keys=None, Tensor(b!)? out_counts=None, Tensor(c!)? out_starts=None) -> (Tensor, Tensor, Tensor, Tensor)");
    m.def("reduce_by_key(Tensor keys, Tensor values, int op, Tensor(a!)? out_keys=None, Tensor(b!)? out=None) -> (Tensor, Tensor, Tensor)");
    m.def("scan_by_key(Tensor keys, Tensor values, int op, bool exclusive=False, Tensor(a!)? out=None) -> Tensor");
    m.def("segmented_scan(Tensor values, Tensor heads, int op, bool exclusive=False, Tensor(a!)? out=None) -> Tensor");
    m.def("run_positions(Tensor keys) -> Tensor");
    m.def("bincount(Tensor x, int num_bins, Tensor? weights=None, Tensor(a!)? out=None, bool accumulate=False) -> Tensor");
    m.def("hist_even(Tensor x, int bins, float lo, float hi, float scale, Tensor(a!)? out=None, bool accumulate=False) -> Tensor");
    m.def("hist_range(Tensor x, Tensor edges, Tensor(a!)? out=None, bool accumulate=False) -> Tensor");
    m.def("merge_keys(Tensor a, Tensor b, bool descending=False, Tensor(a!)? out=None) -> Tensor");
    m.def("merge_index(Tensor a, Tensor b, bool descending=False, bool want_keys=True, Tensor(a!)? out_keys=None, Tensor(b!)? out_idx=None) -> (Tensor, Tensor)");
    m.def("merge_pairs(Tensor keys_a, Tensor values_a, Tensor keys_b, Tensor values_b, bool descending=False, Tensor(a!)? out_keys=None, Tensor(b!)? out_values=None) -> (Tensor, Tensor)");
    m.def("set_op(Tensor a, Tensor b, int op, bool descending=False, bool want_idx=False, Tensor(a!)? out_keys=None, Tensor(b!)? out_idx=None) -> (Tensor, Tensor, Tensor)");
    m.def("set_op_pairs(Tensor keys_a, Tensor values_a, Tensor keys_b, Tensor values_b, int op, bool descending=False) -> (Tensor, Tensor, Tensor)");
    m.def("searchsorted(Tensor sorted_sequence, Tensor values, bool right=False, bool descending=False, bool values_sorted=False, Tensor(a!)? out=None) -> Tensor");
    m.def("segment_reduce(Tensor x, Tensor offsets, int op, Tensor(a!)? out=None) -> Tensor");
    m.def("segment_heads(Tensor offsets, int n, Tensor like) -> Tensor");
    m.def("arg_reduce(Tensor x, int op, bool want_values=True, bool want_indices=True) -> (Tensor, Tensor)");
    m.def("axis_arg_reduce(Tensor x, int op, int route=0, int chunk=0, bool want_values=True, bool want_indices=True) -> (Tensor, Tensor)");
    m.def("segment_arg_reduce(Tensor x, Tensor offsets, int op, bool want_values=True, bool want_indices=True, Tensor(a!)? out_values=None, Tensor(b!)? out_indices=None) -> (Tensor, Tensor)");
    m.def("segment_sort(Tensor keys, Tensor? values, Tensor offsets, int mode, bool descending=False, int begin_bit=0, int end_bit=32, bool want_keys=True) -> (Tensor, Tensor, Tensor)");
    m.def("sgemm(Tensor a, Tensor b, int variant=-1) -> Tensor");
    m.def("sgemm_out(Tensor a, Tensor b, Tensor(a!) c, float alpha=1., float beta=0., int variant=-1) -> Tensor(a!)");
    m.def("sgemm_simt(Tensor a, Tensor b) -> Tensor");
    m.def("device_info(int device=0) -> ()", device_info);
    m.def("histeq(Tensor img) -> Tensor");
    m.def("region2d_grow_(Tensor(a!) region, Tensor img, int thr, int batch=4, int max_launches=100000) -> int");
    m.def("region3d_grow_(Tensor(a!) region, Tensor data, int thr, bool tiled=True, int batch=8, int max_launches=1000000) -> int");
    m.def("region3d_grow_slab_(Tensor(a!) region, Tensor data, int halos, int thr, int batch=8, int max_launches=1000000) -> int");
    m.def("volume_gen_(Tensor(a!) data, int seed) -> Tensor(a!)");
    m.def("volume_gen_slab_(Tensor(a!) data, int z_first, int seed) -> Tensor(a!)");
    m.def("raycast_slab_(Tensor data, Tensor region, int z0, Tensor(a!) state, bool init, bool bottom, int image_dim, float[] cam12, float pixel_width, float step, int max_steps) -> Tensor");
    m.def("raycast_global(Tensor data, Tensor region, int image_dim, float[] cam12, float pixel_width, float step, int max_steps, bool f64_color=True, int variant=-1) -> Tensor");
    m.def("brick_pack(Tensor data, Tensor region) -> Tensor");
    m.def("raycast_bricked(Tensor tex, int image_dim, float[] cam12, float pixel_width, float step, int max_steps, int batch=0, int segments=0) -> Tensor");
    m.def("stencil5_(Tensor u, Tensor(a!) out, int r0, int r1, int global_row0, int global_rows, float k) -> ()");
    m.def("stencil5xT_(Tensor u, Tensor(a!) out, int halo, int steps, int r0, int r1, int global_row0, int global_rows, float k, int shape=0) -> ()");
    m.def("stencil5xT_spans_(Tensor u, Tensor(a!) out, int halo, int steps, int r0a, int r1a, int r0b, int r1b, int global_row0, int global_rows, float k, int shape=0) -> ()");
    m.def("spmv_csr(Tensor row_ptr, Tensor col, Tensor val, Tensor x, Tensor items) -> Tensor");
    m.def("spmm_csr(Tensor row_ptr, Tensor col, Tensor val, Tensor x, Tensor items, Tensor slot, Tensor split, int n_pieces, "
          "int item_nnz, Tensor(a!) out) -> Tensor(a!)");
    m.def("spmv_sliced(Tensor lrow, Tensor col, Tensor val, Tensor x, Tensor items, Tensor row_mask, Tensor chunk_base, Tensor fix, Tensor meta, Tensor(a!) ypart, Tensor(b!) extra, int n_rows, Tensor(c!)? out=None, bool packed=False, int item_nnz=1024, int stage=0, bool ballot_combine=False, int blocks_per_cu=0, int phase_lo=0, int phase_n=0) -> Tensor");
    m.def("spmv_sliced_pair(Tensor x, int item_nnz, int blocks_per_cu, Tensor col_a, Tensor val_a, Tensor items_a, Tensor meta_a, Tensor(a!) ypart_a, Tensor(b!) extra_a, int s_a, int a_lo, int a_n, Tensor col_b, Tensor val_b, Tensor items_b, Tensor meta_b, Tensor(c!) ypart_b, Tensor(d!) extra_b, int s_b, int b_lo, int b_n) -> ()");
    m.def("spmv_sliced_combine(Tensor ypart, Tensor row_mask, Tensor chunk_base, Tensor meta, int n_slices, Tensor extra, Tensor fix, Tensor? fix_chunk0, Tensor(a!) out, int n_rows, Tensor? send_ptr=None, Tensor? send_slot=None, Tensor(b!)? sendbuf=None) -> ()");
    m.def("spmv_banded(Tensor vals, Tensor row_off, int n, int a, int b, int c, int d, int e, Tensor x, int variant=8) -> Tensor");
    m.def("pack_edges(Tensor tile) -> Tensor");
    m.def("unpack_halo_(Tensor(a!) tile, Tensor buf, int mask, Tensor(b!)? changed=None) -> ()");
}

TORCH_LIBRARY_IMPL(pcmx, CUDA, m) {
    m.impl("vmul", vmul);
    m.impl("vadd", vadd);
    m.impl("axpy_", axpy_);
    m.impl("gather_", gather_);
    m.impl("fill_", fill_);
    m.impl("copy_", copy_);
    m.impl("rand_uniform_", rand_uniform_);
    m.impl("reduce", reduce);
    m.impl("dot", dot);
    m.impl("scan", scan);
    m.impl("scan_out", scan_out);
    m.impl("select", select_b32);  // (::select is the POSIX call)
    m.impl("select_index", select_index);
    m.impl("select_if", select_if);
    m.impl("sort_keys", sort_keys);
    m.impl("sort_pairs", sort_pairs);
    m.impl("sort_index", sort_index);
    m.impl("topk", topk);
    m.impl("kth_value", kth_value);
    m.impl("row_sort", row_sort);
    m.impl("row_topk", row_topk);
    m.impl("row_kth", row_kth);
    m.impl("axis_reduce", axis_reduce);
    m.impl("axis_scan", axis_scan);
    m.impl("run_length_encode", run_length_encode);
    m.impl("reduce_by_key", reduce_by_key);
    m.impl("scan_by_key", scan_by_key);
    m.impl("segmented_scan", segmented_scan);
    m.impl("run_positions", run_positions);
    m.impl("bincount", bincount);
    m.impl("hist_even", hist_even);
    m.impl("hist_range", hist_range);
    m.impl("merge_keys", merge_keys);
    m.impl("merge_index", merge_index);
    m.impl("merge_pairs", merge_pairs);
    m.impl("set_op", set_op);
    m.impl("set_op_pairs", set_op_pairs);
    m.impl("searchsorted", searchsorted);
    m.impl("segment_reduce", segment_reduce);
    m.impl("segment_heads", segment_heads);
    m.impl("arg_reduce", arg_reduce);
    m.impl("axis_arg_reduce", axis_arg_reduce);
    m.impl("segment_arg_reduce", segment_arg_reduce);
    m.impl("segment_sort", segment_sort);
    m.impl("sgemm", sgemm);
    m.impl("sgemm_out", sgemm_out);
    m.impl("sgemm_simt", sgemm_simt);
    m.impl("histeq", histeq);
    m.impl("region2d_grow_", region2d_grow_);
    m.impl("region3d_grow_", region3d_grow_);
    m.impl("volume_gen_", volume_gen_);
    m.impl("raycast_global", raycast_global);
    m.impl("brick_pack", brick_pack);
    m.impl("raycast_bricked", raycast_bricked);
    m.impl("region3d_grow_slab_", region3d_grow_slab_);
    m.impl("volume_gen_slab_", volume_gen_slab_);
    m.impl("raycast_slab_", raycast_slab_);
    m.impl("stencil5_", stencil5_);
    m.impl("stencil5xT_", stencil5xT_);
    m.impl("stencil5xT_spans_", stencil5xT_spans_);
    m.impl("spmv_csr", spmv_csr);
    m.impl("spmm_csr", spmm_csr);
    m.impl("spmv_sliced", spmv_sliced);
    m.impl("spmv_sliced_pair", spmv_sliced_pair);
    m.impl("spmv_sliced_combine", spmv_sliced_combine);
    m.impl("spmv_banded", spmv_banded);
    m.impl("pack_edges", pack_edges);
    m.impl("unpack_halo_", unpack_halo_);
}

// ---------------------------------------------------------------- grouped exchange (dedicated RCCL communicator)
// Plain pybind functions (no torch dispatcher on the per-step path): parallel/dist.py NativeExchange.
pybind11::bytes xcomm_unique_id() {
    std::string id((size_t)pcmx_xcomm_id_bytes(), '\0');
    check_rc(pcmx_xcomm_unique_id(id.data()), "xcomm_unique_id");
    return pybind11::bytes(id);
}

int64_t xcomm_create(const std::string& id, int64_t world, int64_t rank, int64_t device) {
    TORCH_CHECK((int)id.size() == pcmx_xcomm_id_bytes(), "xcomm_create: unique id of ", pcmx_xcomm_id_bytes(), " bytes");
    void* h = nullptr;
    check_rc(pcmx_xcomm_create(id.data(), (int)world, (int)rank, (int)device, &h), "xcomm_create");
    return reinterpret_cast<int64_t>(h);
}

void xcomm_exchange(int64_t h, int64_t slot, const at::Tensor& send, const std::vector<int64_t>& soff,
                    const std::vector<int64_t>& scnt, at::Tensor recv, const std::vector<int64_t>& roff,
                    const std::vector<int64_t>& rcnt) {
    TORCH_CHECK(send.is_cuda() && recv.is_cuda() && send.device() == recv.device(), "xcomm_exchange: GPU buffers, one device");
    TORCH_CHECK(send.is_contiguous() && recv.is_contiguous() && send.scalar_type() == recv.scalar_type(),
                "xcomm_exchange: contiguous buffers of one dtype");
    const size_t W = soff.size();
    TORCH_CHECK(W > 0 && scnt.size() == W && roff.size() == W && rcnt.size() == W, "xcomm_exchange: one entry per rank");
    const int64_t es = send.element_size();
    std::vector<int64_t> b(4 * W);  // the segments in bytes
    for (size_t q = 0; q < W; ++q) {  // every segment inside its buffer (host-side, no device data involved)
        TORCH_CHECK(scnt[q] >= 0 && soff[q] >= 0 && soff[q] + scnt[q] <= send.numel(), "xcomm_exchange: send segment ", q);
        TORCH_CHECK(rcnt[q] >= 0 && roff[q] >= 0 && roff[q] + rcnt[q] <= recv.numel(), "xcomm_exchange: recv segment ", q);
        b[q] = soff[q] * es, b[W + q] = scnt[q] * es, b[2 * W + q] = roff[q] * es, b[3 * W + q] = rcnt[q] * es;
    }
    const auto* bl = reinterpret_cast<const long long*>(b.data());
    check_rc(pcmx_xcomm_exchange(reinterpret_cast<void*>(h), (int)slot, send.data_ptr(), bl, bl + W, recv.data_ptr(),
                                 bl + 2 * W, bl + 3 * W, cur_stream(recv)),
             "xcomm_exchange");
}

void xcomm_wait(int64_t h, int64_t slot, int64_t device) {
    check_rc(pcmx_xcomm_wait(reinterpret_cast<void*>(h), (int)slot, c10::hip::getCurrentHIPStream((int)device).stream()),
             "xcomm_wait");
}

PYBIND11_MODULE(_C, mod) {
    mod.doc() = "pcmx MI355X kernels (ops live under torch.ops.pcmx)";
    mod.def("device_count", []() { return pcmx_device_count(); });
    mod.def("spmv_csr_plan", &spmv_csr_plan, "CSR-adaptive work items from a CPU int64 row_ptr",
            pybind11::arg("row_ptr"), pybind11::arg("item_nnz") = 1024);
    mod.def("spmm_csr_plan", &spmm_csr_plan, "SpMM plan from a CPU int64 row_ptr: (items, slot per item, split rows)",
            pybind11::arg("row_ptr"), pybind11::arg("item_nnz") = 1024);
    mod.def("xcomm_unique_id", &xcomm_unique_id, "ncclUniqueId of a new dedicated RCCL communicator (rank 0)");
    mod.def("xcomm_create", &xcomm_create, "join the dedicated RCCL communicator: handle");
    mod.def("xcomm_exchange", &xcomm_exchange, "grouped per-peer send/recv of float segments, ordered after the "
            "current stream (slot: one exchange in flight)");
    mod.def("xcomm_wait", &xcomm_wait, "the current stream of `device` waits for the slot's exchange");
    mod.def("xcomm_probe", [](int64_t h, int64_t timeout_ms) {
        pybind11::gil_scoped_release nogil;
        return pcmx_xcomm_probe(reinterpret_cast<void*>(h), (int)timeout_ms);
    }, "one float to / from every peer, host-waited with a timeout; aborts the communicator on failure (0: ok)");
    mod.def("xcomm_async_error", [](int64_t h) { return pcmx_xcomm_async_error(reinterpret_cast<void*>(h)); });
    mod.def("xcomm_destroy", [](int64_t h) { return pcmx_xcomm_destroy(reinterpret_cast<void*>(h)); });
}
