// Python bindings for the shared-tensor engine (replaces the reference's Lua
// C-API layer, /root/reference/src/sharedtensor.c:347-477).  The binding is
// torch-header-free: tensors cross the boundary as raw data_ptr() integers,
// so the extension builds with bare hipcc and works for CPU and GPU tensors
// alike.  All blocking entrypoints release the GIL; engine threads never
// touch Python.
#include <pybind11/pybind11.h>
#include <pybind11/stl.h>

#include <array>

#include "codec_cpu.h"
#include "engine.h"
#include "rccl_transport.h"

namespace py = pybind11;
using namespace shamd;

namespace {

// CPU codec entrypoints for tests (numerics parity vs ops/oracle.py).
py::tuple py_cpu_encode(int codec, uintptr_t delta, int64_t n, double scale_in,
                        uintptr_t payload_out) {
  Codec c = static_cast<Codec>(codec);
  float* d = reinterpret_cast<float*>(delta);
  float scale = scale_in < 0 ? cpu_compute_scale(c, d, n)
                             : static_cast<float>(scale_in);
  cpu_quantize(c, d, n, scale, reinterpret_cast<uint8_t*>(payload_out));
  return py::make_tuple(scale, payload_bytes(c, n));
}

void py_cpu_apply(int codec, uintptr_t payload, int64_t n, double scale,
                  std::vector<uintptr_t> dsts) {
  std::vector<float*> d;
  for (auto p : dsts) d.push_back(reinterpret_cast<float*>(p));
  cpu_apply(static_cast<Codec>(codec), reinterpret_cast<uint8_t*>(payload), n,
            static_cast<float>(scale), d.data(), static_cast<int>(d.size()));
}

double py_cpu_scale(int codec, uintptr_t delta, int64_t n, int stride) {
  return cpu_compute_scale(static_cast<Codec>(codec),
                           reinterpret_cast<float*>(delta), n, stride);
}

// Direct handle on the CDNA4 codec kernels, for numerics tests and ad-hoc
// use (tensors pass as data_ptr integers; caller owns all buffers).
struct DevCodec {
  DevTable tb{};
  Codec c;
  int device;
  bool dbf16;
  void* reduce = nullptr;

  DevCodec(int codec, std::vector<int64_t> sizes, int dev, bool delta_bf16)
      : c(static_cast<Codec>(codec)), device(dev), dbf16(delta_bf16) {
    std::vector<int64_t> offs(sizes.size() + 1), poffs(sizes.size() + 1);
    offs[0] = poffs[0] = 0;
    for (size_t t = 0; t < sizes.size(); ++t) {
      offs[t + 1] = offs[t] + sizes[t];
      poffs[t + 1] = poffs[t] + pad64(sizes[t]);
    }
    if (hipSetDevice(device) != hipSuccess)
      throw std::runtime_error("hipSetDevice failed");
    int T = static_cast<int>(sizes.size());
    if (hipMalloc(&tb.offs, sizeof(int64_t) * (T + 1) * 2) != hipSuccess)
      throw std::runtime_error("hipMalloc failed");
    tb.poffs = tb.offs + (T + 1);
    (void)hipMemcpy(tb.offs, offs.data(), sizeof(int64_t) * (T + 1),
              hipMemcpyHostToDevice);
    (void)hipMemcpy(tb.poffs, poffs.data(), sizeof(int64_t) * (T + 1),
              hipMemcpyHostToDevice);
    tb.T = T;
    tb.n = offs[T];
    tb.pe = poffs[T];
    if (hipMalloc(&reduce, 8 * T) != hipSuccess)
      throw std::runtime_error("hipMalloc failed");
  }
  ~DevCodec() {
    if (tb.offs) (void)hipFree(tb.offs);
    if (reduce) (void)hipFree(reduce);
  }
  void reduce_scales(uintptr_t delta, uintptr_t scales_dev, int stride,
                     uintptr_t stream) {
    hip_reduce_scales(c, reinterpret_cast<const void*>(delta), dbf16, tb,
                      reduce, reinterpret_cast<float*>(scales_dev), stride,
                      reinterpret_cast<hipStream_t>(stream));
  }
  void quantize(uintptr_t delta, uintptr_t scales_dev, uintptr_t payload,
                uintptr_t stream, uintptr_t stats = 0) {
    hip_quantize(c, reinterpret_cast<void*>(delta), dbf16, tb,
                 reinterpret_cast<const float*>(scales_dev),
                 reinterpret_cast<uint8_t*>(payload),
                 reinterpret_cast<hipStream_t>(stream),
                 reinterpret_cast<void*>(stats));
  }
  void finalize_scales(uintptr_t stats, uintptr_t scales_dev, uintptr_t stream) {
    hip_finalize_scales(c, tb, reinterpret_cast<const void*>(stats),
                        reinterpret_cast<float*>(scales_dev), 1,
                        reinterpret_cast<hipStream_t>(stream));
  }
  // dsts[0] = fp32 values (or 0); dsts[1..2] = delta-typed forwards
  void apply(uintptr_t payload, uintptr_t scales_dev,
             std::vector<uintptr_t> dsts, uintptr_t stream) {
    uintptr_t d[3] = {0, 0, 0};
    for (size_t i = 0; i < dsts.size() && i < 3; ++i) d[i] = dsts[i];
    hip_apply(c, reinterpret_cast<const uint8_t*>(payload), tb,
              reinterpret_cast<const float*>(scales_dev),
              reinterpret_cast<float*>(d[0]), reinterpret_cast<void*>(d[1]),
              reinterpret_cast<void*>(d[2]), dbf16,
              reinterpret_cast<hipStream_t>(stream));
  }
};

// dsts[0] = fp32 values (or 0); dsts[1..3] = delta-typed
void py_gpu_add_scatter(uintptr_t src, int64_t n, double alpha,
                        std::vector<uintptr_t> dsts, uintptr_t stream,
                        bool delta_bf16) {
  uintptr_t d[4] = {0, 0, 0, 0};
  for (size_t i = 0; i < dsts.size() && i < 4; ++i) d[i] = dsts[i];
  hip_add_scatter(reinterpret_cast<const float*>(src), n,
                  static_cast<float>(alpha), reinterpret_cast<float*>(d[0]),
                  reinterpret_cast<void*>(d[1]), reinterpret_cast<void*>(d[2]),
                  reinterpret_cast<void*>(d[3]), delta_bf16,
                  reinterpret_cast<hipStream_t>(stream));
}

// dsts[0] = fp32 values (or 0); dsts[1..3] = delta-typed
void py_gpu_fused_sgd(uintptr_t mom, uintptr_t grad, double lr, double mu,
                      int64_t n, std::vector<uintptr_t> dsts, uintptr_t stream,
                      bool delta_bf16, uintptr_t clip_state, uintptr_t groups) {
  uintptr_t d[4] = {0, 0, 0, 0};
  for (size_t i = 0; i < dsts.size() && i < 4; ++i) d[i] = dsts[i];
  if (groups) {
    hip_fused_sgd_grouped(
        reinterpret_cast<float*>(mom), reinterpret_cast<const float*>(grad),
        static_cast<float>(lr), static_cast<float>(mu), n,
        reinterpret_cast<float*>(d[0]), reinterpret_cast<void*>(d[1]),
        reinterpret_cast<void*>(d[2]), reinterpret_cast<void*>(d[3]),
        delta_bf16, reinterpret_cast<hipStream_t>(stream),
        reinterpret_cast<const ClipState*>(clip_state),
        reinterpret_cast<const void*>(groups));
    return;
  }
  hip_fused_sgd(reinterpret_cast<float*>(mom),
                reinterpret_cast<const float*>(grad), static_cast<float>(lr),
                static_cast<float>(mu), n, reinterpret_cast<float*>(d[0]),
                reinterpret_cast<void*>(d[1]), reinterpret_cast<void*>(d[2]),
                reinterpret_cast<void*>(d[3]), delta_bf16,
                reinterpret_cast<hipStream_t>(stream),
                reinterpret_cast<const ClipState*>(clip_state));
}

// dsts[0] = fp32 values (required: the kernel reads the pre-update weight);
// dsts[1..3] = delta-typed
void py_gpu_fused_sgd_bf16(uintptr_t mom, uintptr_t grad_bf16,
                           uintptr_t shadow_bf16, double lr, double mu,
                           int64_t n, std::vector<uintptr_t> dsts,
                           uintptr_t stream, bool delta_bf16,
                           uintptr_t clip_state, uintptr_t groups) {
  uintptr_t d[4] = {0, 0, 0, 0};
  for (size_t i = 0; i < dsts.size() && i < 4; ++i) d[i] = dsts[i];
  if (!d[0] || !shadow_bf16)
    throw std::runtime_error("gpu_fused_sgd_bf16: values and shadow required");
  if (groups) {
    hip_fused_sgd_bf16_grouped(
        reinterpret_cast<float*>(mom),
        reinterpret_cast<const uint16_t*>(grad_bf16),
        reinterpret_cast<uint16_t*>(shadow_bf16), static_cast<float>(lr),
        static_cast<float>(mu), n, reinterpret_cast<float*>(d[0]),
        reinterpret_cast<void*>(d[1]), reinterpret_cast<void*>(d[2]),
        reinterpret_cast<void*>(d[3]), delta_bf16,
        reinterpret_cast<hipStream_t>(stream),
        reinterpret_cast<const ClipState*>(clip_state),
        reinterpret_cast<const void*>(groups));
    return;
  }
  hip_fused_sgd_bf16(reinterpret_cast<float*>(mom),
                     reinterpret_cast<const uint16_t*>(grad_bf16),
                     reinterpret_cast<uint16_t*>(shadow_bf16),
                     static_cast<float>(lr), static_cast<float>(mu), n,
                     reinterpret_cast<float*>(d[0]),
                     reinterpret_cast<void*>(d[1]),
                     reinterpret_cast<void*>(d[2]),
                     reinterpret_cast<void*>(d[3]), delta_bf16,
                     reinterpret_cast<hipStream_t>(stream),
                     reinterpret_cast<const ClipState*>(clip_state));
}

// dsts[0] = fp32 values (required); dsts[1..3] = delta-typed.  shadow may be
// 0.  inv_bc1/2 = 1/(1-beta^t), rounded to fp32 here as Engine::fused_adamw
// hands them to the kernel.
void py_gpu_fused_adamw(uintptr_t mom, uintptr_t vel, uintptr_t grad,
                        bool grad_bf16, uintptr_t shadow_bf16, double lr,
                        double beta1, double beta2, double eps, double wd,
                        double inv_bc1, double inv_bc2, int64_t n,
                        std::vector<uintptr_t> dsts, uintptr_t stream,
                        bool delta_bf16, uintptr_t clip_state,
                        uintptr_t groups) {
  uintptr_t d[4] = {0, 0, 0, 0};
  for (size_t i = 0; i < dsts.size() && i < 4; ++i) d[i] = dsts[i];
  if (!d[0]) throw std::runtime_error("gpu_fused_adamw: values required");
  if (groups) {  // wd is unused: the table holds each group's decay
    hip_fused_adamw_grouped(
        reinterpret_cast<float*>(mom), reinterpret_cast<float*>(vel),
        reinterpret_cast<const void*>(grad), grad_bf16,
        reinterpret_cast<uint16_t*>(shadow_bf16), static_cast<float>(lr),
        static_cast<float>(beta1), static_cast<float>(beta2),
        static_cast<float>(eps), static_cast<float>(inv_bc1),
        static_cast<float>(inv_bc2), n, reinterpret_cast<float*>(d[0]),
        reinterpret_cast<void*>(d[1]), reinterpret_cast<void*>(d[2]),
        reinterpret_cast<void*>(d[3]), delta_bf16,
        reinterpret_cast<hipStream_t>(stream),
        reinterpret_cast<const ClipState*>(clip_state),
        reinterpret_cast<const void*>(groups));
    return;
  }
  hip_fused_adamw(reinterpret_cast<float*>(mom), reinterpret_cast<float*>(vel),
                  reinterpret_cast<const void*>(grad), grad_bf16,
                  reinterpret_cast<uint16_t*>(shadow_bf16),
                  static_cast<float>(lr), static_cast<float>(beta1),
                  static_cast<float>(beta2), static_cast<float>(eps),
                  static_cast<float>(wd), static_cast<float>(inv_bc1),
                  static_cast<float>(inv_bc2), n,
                  reinterpret_cast<float*>(d[0]),
                  reinterpret_cast<void*>(d[1]), reinterpret_cast<void*>(d[2]),
                  reinterpret_cast<void*>(d[3]), delta_bf16,
                  reinterpret_cast<hipStream_t>(stream),
                  reinterpret_cast<const ClipState*>(clip_state));
}

// Exactly one of grad (fp32) and grad_bf16 is non-zero.  scratch: device
// fp64[>= 2048]; state: 32 device bytes (common.h ClipState), zeroed once by
// the caller.  ValueError unless max_norm is finite and > 0.
void py_gpu_grad_clip_coef(uintptr_t grad, uintptr_t grad_bf16, int64_t n,
                           double max_norm, uintptr_t scratch, uintptr_t state,
                           uintptr_t stream) {
  if (!grad == !grad_bf16)
    throw std::invalid_argument(
        "gpu_grad_clip_coef: pass exactly one of grad and grad_bf16");
  hip_grad_clip_coef(reinterpret_cast<const void*>(grad ? grad : grad_bf16),
                     grad_bf16 != 0, n, max_norm,
                     reinterpret_cast<double*>(scratch),
                     reinterpret_cast<ClipState*>(state),
                     reinterpret_cast<hipStream_t>(stream));
}

// out := values (fp32), delta -= values (delta-typed)
void py_gpu_snapshot_capture(uintptr_t values, uintptr_t delta, uintptr_t out,
                             int64_t n, uintptr_t stream, bool delta_bf16) {
  hip_snapshot_capture(reinterpret_cast<const float*>(values),
                       reinterpret_cast<void*>(delta), delta_bf16,
                       reinterpret_cast<float*>(out), n,
                       reinterpret_cast<hipStream_t>(stream));
}

// src is delta-typed; dsts[0] = fp32 values (or 0); dsts[1..2] = delta-typed
void py_gpu_add_delta_scatter(uintptr_t src, int64_t n,
                              std::vector<uintptr_t> dsts, uintptr_t stream,
                              bool delta_bf16) {
  uintptr_t d[3] = {0, 0, 0};
  for (size_t i = 0; i < dsts.size() && i < 3; ++i) d[i] = dsts[i];
  hip_add_delta_scatter(reinterpret_cast<const void*>(src), delta_bf16, n,
                        reinterpret_cast<float*>(d[0]),
                        reinterpret_cast<void*>(d[1]),
                        reinterpret_cast<void*>(d[2]),
                        reinterpret_cast<hipStream_t>(stream));
}

}  // namespace

PYBIND11_MODULE(_core, m) {
  m.doc() = "MI355X-native shared-tensor engine (CDNA4 HIP + RCCL/TCP)";

  py::class_<Config>(m, "Config")
      .def(py::init<>())
      .def_readwrite("host", &Config::host)
      .def_readwrite("port", &Config::port)
      .def_readwrite("device", &Config::device)
      .def_property(
          "codec", [](const Config& c) { return static_cast<int>(c.codec); },
          [](Config& c, int v) { c.codec = static_cast<Codec>(v); })
      .def_readwrite("snapshot_join", &Config::snapshot_join)
      .def_readwrite("use_rccl", &Config::use_rccl)
      .def_readwrite("reconnect", &Config::reconnect)
      .def_readwrite("preserve_subtree", &Config::preserve_subtree)
      .def_readwrite("keepalive_s", &Config::keepalive_s)
      .def_readwrite("bw_limit", &Config::bw_limit)
      .def_readwrite("min_round_interval_s", &Config::min_round_interval_s)
      .def_readwrite("expected_children", &Config::expected_children)
      .def_readwrite("sizes", &Config::sizes)
      .def_readwrite("explicit_parent", &Config::explicit_parent)
      .def_readwrite("listen_port", &Config::listen_port)
      .def_readwrite("join_timeout_s", &Config::join_timeout_s)
      .def_readwrite("rms_sample_stride", &Config::rms_sample_stride)
      .def_readwrite("lagged_scale", &Config::lagged_scale)
      .def_readwrite("delta_bf16", &Config::delta_bf16)
      .def_readwrite("use_graphs", &Config::use_graphs);

  py::class_<Engine>(m, "Engine")
      .def(py::init<Config>())
      .def("set_values", &Engine::set_values)
      .def("set_link_buffers", &Engine::set_link_buffers)
      .def("start", &Engine::start, py::call_guard<py::gil_scoped_release>())
      .def("add_from", &Engine::add_from,
           py::call_guard<py::gil_scoped_release>())
      .def("copy_to", &Engine::copy_to,
           py::call_guard<py::gil_scoped_release>())
      .def("fused_sgd", &Engine::fused_sgd, py::arg("mom"), py::arg("grad"),
           py::arg("lr"), py::arg("momentum"), py::arg("stream"),
           py::arg("clip_state") = 0, py::arg("groups") = 0,
           py::call_guard<py::gil_scoped_release>())
      .def("fused_sgd_bf16", &Engine::fused_sgd_bf16, py::arg("mom"),
           py::arg("grad"), py::arg("shadow"), py::arg("lr"),
           py::arg("momentum"), py::arg("stream"), py::arg("clip_state") = 0, py::arg("groups") = 0,
           py::call_guard<py::gil_scoped_release>())
      .def("fused_adamw", &Engine::fused_adamw, py::arg("mom"),
           py::arg("vel"), py::arg("grad"), py::arg("grad_bf16"),
           py::arg("shadow"), py::arg("lr"), py::arg("beta1"),
           py::arg("beta2"), py::arg("eps"), py::arg("wd"), py::arg("step"),
           py::arg("stream"), py::arg("clip_state") = 0, py::arg("groups") = 0,
           py::call_guard<py::gil_scoped_release>())
      .def("grad_clip_coef", &Engine::grad_clip_coef, py::arg("grad"),
           py::arg("grad_bf16"), py::arg("n"), py::arg("max_norm"),
           py::arg("scratch"), py::arg("state"), py::arg("stream"),
           py::call_guard<py::gil_scoped_release>())
      .def("notify_dirty", &Engine::notify_dirty)
      .def("close", &Engine::close, py::call_guard<py::gil_scoped_release>())
      .def("is_master", &Engine::is_master)
      .def("listen_port", &Engine::listen_port)
      .def("last_error", &Engine::last_error)
      .def("reconnect_count", &Engine::reconnect_count)
      .def("recent_scales_sent", &Engine::recent_scales_sent)
      .def("recent_scales_recv", &Engine::recent_scales_recv)
      .def("link_stats", [](Engine& e) {
        py::list out;
        for (auto& s : e.link_stats()) {
          py::dict d;
          d["rounds_sent"] = s.rounds_sent;
          d["rounds_recv"] = s.rounds_recv;
          d["bytes_sent"] = s.bytes_sent;
          d["bytes_recv"] = s.bytes_recv;
          d["last_scale_sent"] = s.last_scale_sent;
          d["last_scale_recv"] = s.last_scale_recv;
          d["active"] = s.active;
          d["dead"] = s.dead;
          d["peer"] = s.peer;
          d["rccl"] = s.rccl;
          out.append(d);
        }
        return out;
      });

  py::class_<DevCodec>(m, "DevCodec")
      .def(py::init<int, std::vector<int64_t>, int, bool>(), py::arg("codec"),
           py::arg("sizes"), py::arg("device"), py::arg("delta_bf16") = false)
      .def("reduce_scales", &DevCodec::reduce_scales)
      .def("quantize", &DevCodec::quantize, py::arg("delta"),
           py::arg("scales"), py::arg("payload"), py::arg("stream"),
           py::arg("stats") = 0)
      .def("finalize_scales", &DevCodec::finalize_scales)
      .def("apply", &DevCodec::apply);
  m.def("gpu_add_scatter", &py_gpu_add_scatter, py::arg("src"), py::arg("n"),
        py::arg("alpha"), py::arg("dsts"), py::arg("stream"),
        py::arg("delta_bf16") = false);
  m.def("gpu_fused_sgd", &py_gpu_fused_sgd, py::arg("mom"), py::arg("grad"),
        py::arg("lr"), py::arg("mu"), py::arg("n"), py::arg("dsts"),
        py::arg("stream"), py::arg("delta_bf16") = false,
        py::arg("clip_state") = 0, py::arg("groups") = 0);
  m.def("gpu_fused_sgd_bf16", &py_gpu_fused_sgd_bf16, py::arg("mom"),
        py::arg("grad"), py::arg("shadow"), py::arg("lr"), py::arg("mu"),
        py::arg("n"), py::arg("dsts"), py::arg("stream"),
        py::arg("delta_bf16") = false, py::arg("clip_state") = 0, py::arg("groups") = 0);
  m.def("gpu_fused_adamw", &py_gpu_fused_adamw, py::arg("mom"),
        py::arg("vel"), py::arg("grad"), py::arg("grad_bf16"),
        py::arg("shadow"), py::arg("lr"), py::arg("beta1"), py::arg("beta2"),
        py::arg("eps"), py::arg("wd"), py::arg("inv_bc1"), py::arg("inv_bc2"),
        py::arg("n"), py::arg("dsts"), py::arg("stream"),
        py::arg("delta_bf16") = false, py::arg("clip_state") = 0, py::arg("groups") = 0);
  m.def("gpu_grad_clip_coef", &py_gpu_grad_clip_coef, py::arg("grad"),
        py::arg("grad_bf16"), py::arg("n"), py::arg("max_norm"),
        py::arg("scratch"), py::arg("state"), py::arg("stream"));
  m.attr("GRAD_CLIP_MAX_BLOCKS") = GRAD_CLIP_MAX_BLOCKS;
  // Parameter-group table (common.h): validated, coalesced, as int32 words.
  m.def("build_group_table", &build_group_table, py::arg("n"),
        py::arg("seg_end"), py::arg("seg_group"), py::arg("lr_scale"),
        py::arg("weight_decay"));
  m.attr("GROUP_MAX_SEGMENTS") = GROUP_MAX_SEGMENTS;
  m.attr("GROUP_TILE") = GROUP_TILE;
  m.attr("GROUP_GRID_BLOCKS") = GROUP_GRID_BLOCKS;
  m.def("gpu_snapshot_capture", &py_gpu_snapshot_capture, py::arg("values"),
        py::arg("delta"), py::arg("out"), py::arg("n"), py::arg("stream"),
        py::arg("delta_bf16") = false);
  m.def("gpu_add_delta_scatter", &py_gpu_add_delta_scatter, py::arg("src"),
        py::arg("n"), py::arg("dsts"), py::arg("stream"),
        py::arg("delta_bf16") = false);
  m.def("rccl_loopback_payload", &rccl_loopback_payload,
        "Self ncclSend/ncclRecv of a real payload on one device (1-rank "
        "comm): executes the non-blocking enqueue ordering + stream polling "
        "the 2-GPU xGMI links use and verifies the moved bytes.");
  m.def("rccl_self_test", &rccl_self_test,
        py::call_guard<py::gil_scoped_release>());

  // fused bf16 GELU
  m.def("gelu_fwd", [](uintptr_t x, uintptr_t y, int64_t n, uintptr_t stream) {
    hip_gelu_fwd(reinterpret_cast<const void*>(x), reinterpret_cast<void*>(y),
                 n, reinterpret_cast<hipStream_t>(stream));
  });
  m.def("gelu_bwd", [](uintptr_t dy, uintptr_t x, uintptr_t dx, int64_t n,
                       uintptr_t stream) {
    hip_gelu_bwd(reinterpret_cast<const void*>(dy),
                 reinterpret_cast<const void*>(x),
                 reinterpret_cast<void*>(dx), n,
                 reinterpret_cast<hipStream_t>(stream));
  });

  // bias gradients fused into GELU backward / the qkv gradient pack
  m.def("bias_grad_partial_floats", &hip_bias_grad_partial_floats);
  m.def("bias_grad_sweep_rows", &hip_bias_grad_sweep_rows);
  m.def("gelu_bwd_colsum", [](uintptr_t dy, uintptr_t x, uintptr_t dx,
                              uintptr_t db, uintptr_t partial, int64_t R,
                              int64_t C, uintptr_t stream) {
    hip_gelu_bwd_colsum(reinterpret_cast<const void*>(dy),
                        reinterpret_cast<const void*>(x),
                        reinterpret_cast<void*>(dx),
                        reinterpret_cast<void*>(db),
                        reinterpret_cast<float*>(partial), R, C,
                        reinterpret_cast<hipStream_t>(stream));
  });
  m.def("pack3_colsum", [](uintptr_t s0, uintptr_t s1, uintptr_t s2,
                           uintptr_t dst, uintptr_t db, uintptr_t partial,
                           int64_t R, int64_t C, uintptr_t stream) {
    hip_pack3_colsum(reinterpret_cast<const void*>(s0),
                     reinterpret_cast<const void*>(s1),
                     reinterpret_cast<const void*>(s2),
                     reinterpret_cast<void*>(dst),
                     reinterpret_cast<void*>(db),
                     reinterpret_cast<float*>(partial), R, C,
                     reinterpret_cast<hipStream_t>(stream));
  });

  // causal bf16 attention forward, head dim 64
  m.def("attn_fwd_causal_hd64",
        [](uintptr_t q, uintptr_t k, uintptr_t v, uintptr_t out, uintptr_t lse,
           int64_t B, int64_t H, int64_t T, std::array<int64_t, 3> q_strides,
           std::array<int64_t, 3> k_strides, std::array<int64_t, 3> v_strides,
           int64_t lse_stride, double scale, uintptr_t stream) {
          hip_attn_fwd_causal_hd64(
              reinterpret_cast<const void*>(q),
              reinterpret_cast<const void*>(k),
              reinterpret_cast<const void*>(v), reinterpret_cast<void*>(out),
              reinterpret_cast<float*>(lse), B, H, T, q_strides.data(),
              k_strides.data(), v_strides.data(), lse_stride,
              static_cast<float>(scale),
              reinterpret_cast<hipStream_t>(stream));
        },
        py::arg("q"), py::arg("k"), py::arg("v"), py::arg("out"),
        py::arg("lse"), py::arg("B"), py::arg("H"), py::arg("T"),
        py::arg("q_strides"), py::arg("k_strides"), py::arg("v_strides"),
        py::arg("lse_stride"), py::arg("scale"), py::arg("stream"));

  // split-K bf16 weight gradient dW = dY^T X
  m.def("wgrad_num_variants", &hip_wgrad_num_variants);
  m.def("wgrad_tile", [](int variant) {
    int tn = 0, tk = 0;
    hip_wgrad_tile(variant, &tn, &tk);
    return std::make_pair(tn, tk);
  });
  m.def("wgrad_bf16",
        [](uintptr_t dy, uintptr_t x, uintptr_t dw, uintptr_t ws,
           int64_t ws_floats, int64_t M, int64_t N, int64_t K, int64_t ldy,
           int64_t ldx, int64_t ldw, int64_t split, int variant,
           uintptr_t stream) {
          hip_wgrad_bf16(reinterpret_cast<const void*>(dy),
                         reinterpret_cast<const void*>(x),
                         reinterpret_cast<void*>(dw),
                         reinterpret_cast<float*>(ws), ws_floats, M, N, K, ldy,
                         ldx, ldw, split, variant,
                         reinterpret_cast<hipStream_t>(stream));
        },
        py::arg("dy"), py::arg("x"), py::arg("dw"), py::arg("ws"),
        py::arg("ws_floats"), py::arg("M"), py::arg("N"), py::arg("K"),
        py::arg("ldy"), py::arg("ldx"), py::arg("ldw"), py::arg("split"),
        py::arg("variant"), py::arg("stream"));

  // fused bf16 cross-entropy
  m.def("ce_fwd", [](uintptr_t logits, uintptr_t targets, uintptr_t loss,
                     uintptr_t row_m, uintptr_t row_lse, int64_t R, int64_t V,
                     uintptr_t stream) {
    hip_ce_fwd(reinterpret_cast<const void*>(logits),
               reinterpret_cast<const int32_t*>(targets),
               reinterpret_cast<float*>(loss), reinterpret_cast<float*>(row_m),
               reinterpret_cast<float*>(row_lse), R, V,
               reinterpret_cast<hipStream_t>(stream));
  });
  m.def("ce_bwd", [](uintptr_t logits, uintptr_t targets, uintptr_t row_lse,
                     uintptr_t dlogits, uintptr_t gscale_dev, double inv_r,
                     int64_t R, int64_t V, uintptr_t stream,
                     bool skip_if_unit) {
    hip_ce_bwd(reinterpret_cast<const void*>(logits),
               reinterpret_cast<const int32_t*>(targets),
               reinterpret_cast<const float*>(row_lse),
               reinterpret_cast<void*>(dlogits),
               reinterpret_cast<const float*>(gscale_dev),
               static_cast<float>(inv_r), R, V, skip_if_unit,
               reinterpret_cast<hipStream_t>(stream));
  }, py::arg("logits"), py::arg("targets"), py::arg("row_lse"),
     py::arg("dlogits"), py::arg("gscale_dev"), py::arg("inv_r"),
     py::arg("R"), py::arg("V"), py::arg("stream"),
     py::arg("skip_if_unit") = false);
  m.def("ce_fwd_grad", [](uintptr_t logits, uintptr_t targets, uintptr_t loss,
                          uintptr_t row_lse, uintptr_t dlogits, double inv_r,
                          int64_t R, int64_t V, uintptr_t stream) {
    hip_ce_fwd_grad(reinterpret_cast<const void*>(logits),
                    reinterpret_cast<const int32_t*>(targets),
                    reinterpret_cast<float*>(loss),
                    reinterpret_cast<float*>(row_lse),
                    reinterpret_cast<void*>(dlogits),
                    static_cast<float>(inv_r), R, V,
                    reinterpret_cast<hipStream_t>(stream));
  });
  m.def("ce_fwd_grad_max_v", &hip_ce_fwd_grad_max_v);

  // fused bf16 cross-entropy with ignore_index / label smoothing / z-loss
  // (ce_kernels.hip, the masked row policies).  state: 16 device bytes (hip_api.h CeOptState),
  // written by ce_opts_scan.  ValueError for options out of range.
  m.attr("CE_OPT_STATE_BYTES") = static_cast<int>(sizeof(CeOptState));
  m.def("ce_opts_scan", [](uintptr_t targets, int64_t R, int64_t V,
                           int32_t ignore_index, bool has_ignore,
                           uintptr_t state, uintptr_t stream) {
    hip_ce_opts_scan(reinterpret_cast<const int32_t*>(targets), R, V,
                     CeOpts{ignore_index, has_ignore, 0.f, 0.f},
                     reinterpret_cast<CeOptState*>(state),
                     reinterpret_cast<hipStream_t>(stream));
  }, py::arg("targets"), py::arg("R"), py::arg("V"), py::arg("ignore_index"),
     py::arg("has_ignore"), py::arg("state"), py::arg("stream"));
  m.def("ce_opts_fwd_grad", [](uintptr_t logits, uintptr_t targets,
                               uintptr_t loss, uintptr_t row_lse,
                               uintptr_t dlogits, uintptr_t state, int64_t R,
                               int64_t V, int32_t ignore_index,
                               bool has_ignore, double label_smoothing,
                               double z_loss, uintptr_t stream) {
    hip_ce_opts_fwd_grad(reinterpret_cast<const void*>(logits),
                         reinterpret_cast<const int32_t*>(targets),
                         reinterpret_cast<float*>(loss),
                         reinterpret_cast<float*>(row_lse),
                         reinterpret_cast<void*>(dlogits),
                         reinterpret_cast<const CeOptState*>(state),
                         CeOpts{ignore_index, has_ignore,
                                static_cast<float>(label_smoothing),
                                static_cast<float>(z_loss)},
                         R, V, reinterpret_cast<hipStream_t>(stream));
  }, py::arg("logits"), py::arg("targets"), py::arg("loss"),
     py::arg("row_lse"), py::arg("dlogits"), py::arg("state"), py::arg("R"),
     py::arg("V"), py::arg("ignore_index"), py::arg("has_ignore"),
     py::arg("label_smoothing"), py::arg("z_loss"), py::arg("stream"));
  m.def("ce_opts_fwd", [](uintptr_t logits, uintptr_t targets, uintptr_t loss,
                          uintptr_t row_lse, int64_t R, int64_t V,
                          int32_t ignore_index, bool has_ignore,
                          double label_smoothing, double z_loss,
                          uintptr_t stream) {
    hip_ce_opts_fwd(reinterpret_cast<const void*>(logits),
                    reinterpret_cast<const int32_t*>(targets),
                    reinterpret_cast<float*>(loss),
                    reinterpret_cast<float*>(row_lse),
                    CeOpts{ignore_index, has_ignore,
                           static_cast<float>(label_smoothing),
                           static_cast<float>(z_loss)},
                    R, V, reinterpret_cast<hipStream_t>(stream));
  }, py::arg("logits"), py::arg("targets"), py::arg("loss"),
     py::arg("row_lse"), py::arg("R"), py::arg("V"), py::arg("ignore_index"),
     py::arg("has_ignore"), py::arg("label_smoothing"), py::arg("z_loss"),
     py::arg("stream"));
  m.def("ce_opts_bwd", [](uintptr_t logits, uintptr_t targets,
                          uintptr_t row_lse, uintptr_t dlogits,
                          uintptr_t gscale_dev, uintptr_t state, int64_t R,
                          int64_t V, int32_t ignore_index, bool has_ignore,
                          double label_smoothing, double z_loss,
                          uintptr_t stream, bool skip_if_unit) {
    hip_ce_opts_bwd(reinterpret_cast<const void*>(logits),
                    reinterpret_cast<const int32_t*>(targets),
                    reinterpret_cast<const float*>(row_lse),
                    reinterpret_cast<void*>(dlogits),
                    reinterpret_cast<const float*>(gscale_dev),
                    reinterpret_cast<const CeOptState*>(state),
                    CeOpts{ignore_index, has_ignore,
                           static_cast<float>(label_smoothing),
                           static_cast<float>(z_loss)},
                    R, V, skip_if_unit, reinterpret_cast<hipStream_t>(stream));
  }, py::arg("logits"), py::arg("targets"), py::arg("row_lse"),
     py::arg("dlogits"), py::arg("gscale_dev"), py::arg("state"), py::arg("R"),
     py::arg("V"), py::arg("ignore_index"), py::arg("has_ignore"),
     py::arg("label_smoothing"), py::arg("z_loss"), py::arg("stream"),
     py::arg("skip_if_unit") = false);

  // fused bf16 LayerNorm (pointers are bf16 unless named mean/rstd/dgamma/
  // dbeta, which are fp32)
  m.def("ln_fwd", [](uintptr_t x, uintptr_t w, uintptr_t b, uintptr_t y,
                     uintptr_t mean, uintptr_t rstd, int64_t R, int C,
                     double eps, uintptr_t stream) {
    hip_ln_fwd(reinterpret_cast<const void*>(x),
               reinterpret_cast<const void*>(w),
               reinterpret_cast<const void*>(b), reinterpret_cast<void*>(y),
               reinterpret_cast<float*>(mean), reinterpret_cast<float*>(rstd),
               R, C, static_cast<float>(eps),
               reinterpret_cast<hipStream_t>(stream));
  });
  m.def("colsum_bf16", [](uintptr_t x, uintptr_t out, int64_t R, int C,
                          uintptr_t stream) {
    hip_colsum_bf16(reinterpret_cast<const void*>(x),
                    reinterpret_cast<float*>(out), R, C,
                    reinterpret_cast<hipStream_t>(stream));
  });
  m.def("swiglu_fwd", [](uintptr_t x1, uintptr_t x3, uintptr_t y, int64_t n,
                         uintptr_t stream) {
    hip_swiglu_fwd(reinterpret_cast<const void*>(x1),
                   reinterpret_cast<const void*>(x3),
                   reinterpret_cast<void*>(y), n,
                   reinterpret_cast<hipStream_t>(stream));
  });
  m.def("swiglu_bwd", [](uintptr_t dy, uintptr_t x1, uintptr_t x3,
                         uintptr_t dx1, uintptr_t dx3, int64_t n,
                         uintptr_t stream) {
    hip_swiglu_bwd(reinterpret_cast<const void*>(dy),
                   reinterpret_cast<const void*>(x1),
                   reinterpret_cast<const void*>(x3),
                   reinterpret_cast<void*>(dx1),
                   reinterpret_cast<void*>(dx3), n,
                   reinterpret_cast<hipStream_t>(stream));
  });
  // fused RoPE over q and k; strides are (B, H, T) element strides, k == 0
  // rotates q alone
  m.def("rope_qk", [](uintptr_t q, uintptr_t k, uintptr_t q_out,
                      uintptr_t k_out, uintptr_t cos, uintptr_t sin,
                      int64_t B, int64_t Hq, int64_t Hkv, int64_t T,
                      int64_t D, std::array<int64_t, 3> q_strides,
                      std::array<int64_t, 3> k_strides,
                      std::array<int64_t, 3> q_out_strides,
                      std::array<int64_t, 3> k_out_strides, bool inverse,
                      uintptr_t stream) {
    auto st = [](const std::array<int64_t, 3>& a) {
      return RopeStrides{a[0], a[1], a[2]};
    };
    hip_rope_qk(reinterpret_cast<const void*>(q),
                reinterpret_cast<const void*>(k),
                reinterpret_cast<void*>(q_out),
                reinterpret_cast<void*>(k_out),
                reinterpret_cast<const float*>(cos),
                reinterpret_cast<const float*>(sin), B, Hq, Hkv, T, D,
                st(q_strides), st(k_strides), st(q_out_strides),
                st(k_out_strides), inverse,
                reinterpret_cast<hipStream_t>(stream));
  }, py::arg("q"), py::arg("k"), py::arg("q_out"), py::arg("k_out"),
     py::arg("cos"), py::arg("sin"), py::arg("B"), py::arg("Hq"),
     py::arg("Hkv"), py::arg("T"), py::arg("D"), py::arg("q_strides"),
     py::arg("k_strides"), py::arg("q_out_strides"),
     py::arg("k_out_strides"), py::arg("inverse"), py::arg("stream"));
  m.def("rms_fwd", [](uintptr_t x, uintptr_t w, uintptr_t y, uintptr_t rstd,
                      int64_t R, int C, double eps, uintptr_t stream) {
    hip_rms_fwd(reinterpret_cast<const void*>(x),
                reinterpret_cast<const void*>(w), reinterpret_cast<void*>(y),
                reinterpret_cast<float*>(rstd), R, C, static_cast<float>(eps),
                reinterpret_cast<hipStream_t>(stream));
  });
  m.def("rms_bwd", [](uintptr_t dy, uintptr_t x, uintptr_t w, uintptr_t rstd,
                      uintptr_t dx, uintptr_t dgamma, int64_t R, int C,
                      uintptr_t stream) {
    hip_rms_bwd(reinterpret_cast<const void*>(dy),
                reinterpret_cast<const void*>(x),
                reinterpret_cast<const void*>(w),
                reinterpret_cast<const float*>(rstd),
                reinterpret_cast<void*>(dx), reinterpret_cast<float*>(dgamma),
                R, C, reinterpret_cast<hipStream_t>(stream));
  });
  m.def("ln_bwd", [](uintptr_t dy, uintptr_t x, uintptr_t w, uintptr_t mean,
                     uintptr_t rstd, uintptr_t dx, uintptr_t dgamma,
                     uintptr_t dbeta, int64_t R, int C, uintptr_t stream) {
    hip_ln_bwd(reinterpret_cast<const void*>(dy),
               reinterpret_cast<const void*>(x),
               reinterpret_cast<const void*>(w),
               reinterpret_cast<const float*>(mean),
               reinterpret_cast<const float*>(rstd),
               reinterpret_cast<void*>(dx), reinterpret_cast<float*>(dgamma),
               reinterpret_cast<float*>(dbeta), R, C,
               reinterpret_cast<hipStream_t>(stream));
  });

  // fused residual add + LayerNorm; 0 for an absent optional pointer
  m.def("add_ln_supported", &hip_add_ln_supported);
  m.def("add_ln_max_blocks", &hip_add_ln_max_blocks);
  m.def("add_ln_fwd", [](uintptr_t x, uintptr_t delta, uintptr_t dbias,
                         uintptr_t w, uintptr_t b, uintptr_t x_new,
                         uintptr_t y, uintptr_t mean, uintptr_t rstd,
                         int64_t R, int C, double eps, uintptr_t stream) {
    hip_add_ln_fwd(reinterpret_cast<const void*>(x),
                   reinterpret_cast<const void*>(delta),
                   reinterpret_cast<const void*>(dbias),
                   reinterpret_cast<const void*>(w),
                   reinterpret_cast<const void*>(b),
                   reinterpret_cast<void*>(x_new), reinterpret_cast<void*>(y),
                   reinterpret_cast<float*>(mean),
                   reinterpret_cast<float*>(rstd), R, C,
                   static_cast<float>(eps),
                   reinterpret_cast<hipStream_t>(stream));
  });
  m.def("add_ln_bwd", [](uintptr_t dy, uintptr_t x_new, uintptr_t w,
                         uintptr_t mean, uintptr_t rstd, uintptr_t d_x_new,
                         uintptr_t dx_total, uintptr_t dgamma, uintptr_t dbeta,
                         uintptr_t ddbias, uintptr_t partial, int64_t R, int C,
                         uintptr_t stream) {
    hip_add_ln_bwd(reinterpret_cast<const void*>(dy),
                   reinterpret_cast<const void*>(x_new),
                   reinterpret_cast<const void*>(w),
                   reinterpret_cast<const float*>(mean),
                   reinterpret_cast<const float*>(rstd),
                   reinterpret_cast<const void*>(d_x_new),
                   reinterpret_cast<void*>(dx_total),
                   reinterpret_cast<void*>(dgamma),
                   reinterpret_cast<void*>(dbeta),
                   reinterpret_cast<void*>(ddbias),
                   reinterpret_cast<float*>(partial), R, C,
                   reinterpret_cast<hipStream_t>(stream));
  });

  // fused residual add + RMSNorm; 0 for an absent optional pointer
  m.def("add_rms_supported", &hip_add_rms_supported);
  m.def("add_rms_max_blocks", &hip_add_rms_max_blocks);
  m.def("add_rms_fwd", [](uintptr_t x, uintptr_t delta, uintptr_t w,
                          uintptr_t x_new, uintptr_t y, uintptr_t rstd,
                          int64_t R, int C, double eps, uintptr_t stream) {
    hip_add_rms_fwd(reinterpret_cast<const void*>(x),
                    reinterpret_cast<const void*>(delta),
                    reinterpret_cast<const void*>(w),
                    reinterpret_cast<void*>(x_new),
                    reinterpret_cast<void*>(y),
                    reinterpret_cast<float*>(rstd), R, C,
                    static_cast<float>(eps),
                    reinterpret_cast<hipStream_t>(stream));
  });
  m.def("add_rms_bwd", [](uintptr_t dy, uintptr_t x_new, uintptr_t w,
                          uintptr_t rstd, uintptr_t d_x_new,
                          uintptr_t dx_total, uintptr_t dgamma,
                          uintptr_t partial, int64_t R, int C,
                          uintptr_t stream) {
    hip_add_rms_bwd(reinterpret_cast<const void*>(dy),
                    reinterpret_cast<const void*>(x_new),
                    reinterpret_cast<const void*>(w),
                    reinterpret_cast<const float*>(rstd),
                    reinterpret_cast<const void*>(d_x_new),
                    reinterpret_cast<void*>(dx_total),
                    reinterpret_cast<void*>(dgamma),
                    reinterpret_cast<float*>(partial), R, C,
                    reinterpret_cast<hipStream_t>(stream));
  });

  m.def("msg_bytes", &Engine::msg_bytes);
  m.def("scales_area", &Engine::scales_area);
  m.def("payload_bytes",
        [](int c, int64_t n) { return payload_bytes(static_cast<Codec>(c), n); });
  m.def("pad64", &pad64);
  m.def("cpu_encode", &py_cpu_encode);
  m.def("cpu_apply", &py_cpu_apply);
  m.def("cpu_scale", &py_cpu_scale);
  m.def("f32_to_e4m3", [](float x) { return static_cast<int>(f32_to_e4m3(x)); });
  m.def("e4m3_to_f32", [](int v) { return e4m3_to_f32(static_cast<uint8_t>(v)); });

#ifdef SHAMD_WITH_HIP
  m.attr("with_hip") = true;
#else
  m.attr("with_hip") = false;
#endif
}
