// Common types for the MI355X-native shared-tensor engine.
//
// This is a from-scratch re-engineering of the capability set of
// Hello1024/shared-tensor (/root/reference/src/sharedtensor.c): a distributed
// shared tensor with approximate, compressed, error-feedback delta gossip over
// a self-organizing binary tree.  The reference is a single-threaded CPU/Lua
// extension; this engine keeps the replica and all delta staging in HBM3E,
// runs the codec as CDNA4 HIP kernels, and moves intra-node packets over RCCL
// p2p (xGMI) with TCP retained as control plane / inter-node data plane.
#pragma once

#include <atomic>
#include <condition_variable>
#include <cstdint>
#include <cstring>
#include <deque>
#include <mutex>
#include <shared_mutex>
#include <string>
#include <thread>
#include <vector>

namespace shamd {

enum class Codec : uint32_t { OneBit = 0, Fp8 = 1, Int4 = 2 };

// Padded element count: every tensor's element space is padded to a multiple
// of 64 so that (a) a 64-lane wavefront never straddles a tensor boundary in
// the quantize kernel (__ballot packs one uint64 word per wave) and (b) all
// per-tensor payload regions are 8-byte aligned.
inline int64_t pad64(int64_t n) { return (n + 63) & ~int64_t(63); }

// Payload bytes for one tensor of n elements (matches ops/oracle.py).
inline int64_t payload_bytes(Codec c, int64_t n) {
  int64_t pe = pad64(n);
  switch (c) {
    case Codec::OneBit: return pe / 8;
    case Codec::Fp8: return pe;
    case Codec::Int4: return pe / 2;
  }
  return 0;
}

struct Config {
  std::string host;          // rendezvous host (master binds here)
  int port = 0;              // rendezvous port
  int device = -1;           // -1 = CPU, else HIP device ordinal
  Codec codec = Codec::OneBit;
  bool snapshot_join = true; // 'Y' is followed by a full state snapshot
  bool use_rccl = true;      // allow RCCL/xGMI upgrade for same-host GPU links
  bool reconnect = false;    // try to rejoin if the up-link dies
  bool preserve_subtree = false;  // on up-link death keep children attached
                             // and rejoin with the whole subtree: the
                             // reconciliation computes a correction delta
                             // (S + R - V_old) that drains to the children
                             // as ordinary gossip.  Acyclic by construction:
                             // the detached subtree is unreachable from the
                             // root's redirect walk.  Requires snapshot_join.
  double keepalive_s = 1.0;  // idle ping interval (reference: 1s, :161-164)
  double bw_limit = 0.0;     // bytes/sec cap per link, 0 = unlimited
                             // (reference TODO, README.md:31)
  double min_round_interval_s = 0.0;  // pace each link's send loop: the
                             // reference free-runs ("fills all bandwidth"),
                             // but on GPU the codec kernels share HBM with
                             // training compute — pacing trades (already
                             // tiny) staleness for compute bandwidth
  int expected_children = 2; // how many child links to provision buffers for
  std::vector<int64_t> sizes;  // per-tensor element counts (table mode;
                               // size 1 = classic flat tensor)
  std::string explicit_parent;  // "ip:port" — skip the discovery walk and
                                // connect straight to this node ("" = walk)
  int listen_port = 0;  // >0: bind the listener to this fixed port (explicit
                        // topologies); 0: reference behaviour — the local
                        // port of the up-connection
  double join_timeout_s = 60.0;
  int rms_sample_stride = 1;  // >1: subsample the RMS reduction (scale is a
                              // heuristic; stride k cuts its HBM traffic k×)
  bool lagged_scale = false;  // GPU: fold the scale statistic into the
                              // quantize kernel (next round's scale from this
                              // round's post-quantize residual) — removes the
                              // reduce pass from the steady state
  bool delta_bf16 = false;    // GPU: store per-link residual deltas in bf16
                              // (halves their HBM footprint; debit quanta
                              // are bf16-exact, only the remainder rounds)
  bool use_graphs = false;    // GPU: capture the per-round kernel+copy
                              // sequences into hipGraphs.  Measured NET
                              // NEGATIVE on MI355X/ROCm 7.2 (replay floor
                              // ~10-16us vs ~3.5us per plain launch; rounds
                              // are 2-4 ops) — kept as an option only.
};

struct LinkStatsSnap {
  uint64_t rounds_sent, rounds_recv, bytes_sent, bytes_recv;
  float last_scale_sent, last_scale_recv;
  bool active, dead;
  std::string peer;
  bool rccl;
};

// Gradient-clipping state: written by grad_clip_coef (device memory for GPU
// engines, host memory for CPU engines) and read by the fused optimizer
// steps.  The layout is public: python reads it back as 8 int32 words.
struct ClipState {
  double sumsq;            // sum of g*g in fp64
  float norm;              // (float)sqrt(sumsq); may be inf
  float coef;              // (float)min(1, max_norm / (sqrt(sumsq) + 1e-6));
                           // 0 when skip is set
  uint32_t skip;           // 1: sumsq is not finite, the step must not run
  uint32_t skipped_total;  // running count of skip == 1, never reset here
  uint32_t pad[2];
};
static_assert(sizeof(ClipState) == 32, "clip state layout is public");

// Partials of the sum-of-squares reduction: callers size the fp64 scratch
// for this many blocks.
constexpr int GRAD_CLIP_MAX_BLOCKS = 2048;

// Parameter-group table read by the fused optimizer steps: the flat buffer
// of n elements as S contiguous segments, each belonging to one of G groups
// with its own learning-rate scale and weight decay.  Device memory for GPU
// engines, host memory for CPU engines, 8-byte aligned.  The layout is
// public (python holds it as int32 words; docs/ARCHITECTURE.md):
//
//   byte  0            int64   n              (== seg_end[S-1])
//   byte  8            int32   S              1 <= S <= GROUP_MAX_SEGMENTS
//   byte 12            int32   G              1 <= G
//   byte 16            int64   seg_end[S]     exclusive ends, strictly ascending
//   byte 16 + 8*S      int32   seg_group[S]   in [0, G)
//   byte 16 + 12*S     float   lr_scale[G]    finite, >= 0
//   byte 16 + 12*S+4*G float   weight_decay[G]  finite, >= 0
//
// Adjacent segments never share a group (build_group_table merges them).
// A segment's effective rate is fl32(lr * lr_scale[g]): one fp32 multiply
// rounded on its own, then used wherever the ungrouped step uses lr.
constexpr int GROUP_MAX_SEGMENTS = 4096;  // Llama-3-8B has 291 tensors
// The grouped kernels walk the buffer in tiles of GROUP_TILE contiguous
// elements, one block per tile, at most GROUP_GRID_BLOCKS blocks (the
// launch geometry of the ungrouped kernels); a tile that holds a segment
// boundary stages at most GROUP_TILE segments in LDS.
constexpr int GROUP_TILE = 256;
constexpr int GROUP_GRID_BLOCKS = 32768;
constexpr int GROUP_HEADER_WORDS = 4;

inline int64_t group_table_words(int64_t S, int64_t G) {
  return GROUP_HEADER_WORDS + 3 * S + 2 * G;
}

struct GroupTableView {
  int64_t n;
  int32_t S, G;
  const int64_t* seg_end;
  const int32_t* seg_group;
  const float* lr_scale;
  const float* weight_decay;
};

// Host-side view of a table in host memory (CPU engines, tests).
inline GroupTableView group_table_view(const void* table) {
  const char* b = static_cast<const char*>(table);
  GroupTableView v;
  std::memcpy(&v.n, b, 8);
  std::memcpy(&v.S, b + 8, 4);
  std::memcpy(&v.G, b + 12, 4);
  v.seg_end = reinterpret_cast<const int64_t*>(b + 16);
  v.seg_group = reinterpret_cast<const int32_t*>(b + 16 + 8 * int64_t(v.S));
  v.lr_scale = reinterpret_cast<const float*>(b + 16 + 12 * int64_t(v.S));
  v.weight_decay = v.lr_scale + v.G;
  return v;
}

// Validates (std::invalid_argument otherwise), merges adjacent segments of
// one group and returns the table as int32 words.  Defined in engine.cpp.
std::vector<int32_t> build_group_table(int64_t n,
                                       const std::vector<int64_t>& seg_end,
                                       const std::vector<int64_t>& seg_group,
                                       const std::vector<double>& lr_scale,
                                       const std::vector<double>& weight_decay);

constexpr uint32_t MAGIC = 0x53544132;  // "STA2"
constexpr uint16_t PROTO_VERSION = 2;

// client hello flags
constexpr uint16_t HELLO_HAS_GPU = 1;
constexpr uint16_t HELLO_WANT_RCCL = 2;
// accept flags
constexpr uint16_t ACC_SNAPSHOT = 1;
constexpr uint16_t ACC_RCCL = 2;

#pragma pack(push, 1)
struct Hello {           // client -> server right after connect
  uint32_t magic;
  uint16_t version;
  uint16_t flags;
  uint64_t n;            // total (unpadded) element count
  uint32_t ntensors;
  uint32_t codec;
  uint64_t hostid;       // for same-host (xGMI) detection
  int32_t device;        // HIP device ordinal (-1 = CPU)
  uint32_t pad;
};
struct AcceptHello {     // server -> client after 'Y'
  uint16_t version;
  uint16_t flags;
  uint32_t codec;        // authoritative codec for this link
  uint64_t n;
  uint32_t ntensors;
  uint32_t reserved;
};
struct PacketHeader {    // every TCP data-plane message
  uint8_t type;          // 0 = DATA, 1 = PING, 2 = CLOSE
  uint8_t codec;
  uint16_t reserved;
  uint32_t ntensors;
  // DATA: followed by fp32 scales[ntensors] + payload
};
#pragma pack(pop)

constexpr uint8_t PKT_DATA = 0;
constexpr uint8_t PKT_PING = 1;
constexpr uint8_t PKT_CLOSE = 2;

}  // namespace shamd
