// The closed-loop client rule (include/isim.h isim_closed_loop*, DESIGN.md
// §18), one header for closed_loop.cpp (host) and closed_loop.hip (host and
// device): the schedule, the saturating add, a request as a map on the
// connection's state and the composition of such maps, in exact integers.
//
//   c = j mod C, k = j div C, s_j = o_c + k p, o_c = floor(c p / C) or 0
//   A_j = max(F_c, s_j),  F_c <- A_j + L_j        (every + saturates)
//
// Request j is x -> max(x + L_j, s_j + L_j) = Map{L_j, s_j + L_j}; maps
// compose associatively under saturation, so a connection's requests can be
// scanned in any grouping.
#pragma once

#include <cstdint>

#include "../../include/isim.h"
#include "host_device.h"

namespace isim {
namespace cl {

using Client = struct ::isim_closed_loop;  // the function isim_closed_loop hides the plain name

constexpr uint32_t kMaxConnections = ISIM_CL_MAX_CONNECTIONS;
constexpr uint64_t kMaxPeriod = 1ull << 40;
constexpr uint64_t kMaxFirst = 1ull << 40;
constexpr uint64_t kMaxN = 1ull << 32;
constexpr uint64_t kScheduleEnd = 1ull << 63;  // every scheduled start of a batch stays below this

__host__ __device__ inline uint64_t sat_add(uint64_t a, uint64_t b) {
  const uint64_t s = a + b;
  return s < a ? ~0ull : s;
}

// o_c: c < C <= 2^16 and p <= 2^40, the product fits 64 bits
__host__ __device__ inline uint64_t offset_of(uint32_t c, uint32_t C, uint64_t p, uint32_t flags) {
  return (flags & ISIM_CL_UNIFORM) ? (uint64_t)c * p / C : 0;
}

// s_j for connection c's k-th request; the caller has checked that it is below 2^63
__host__ __device__ inline uint64_t start_of(uint32_t c, uint64_t k, uint32_t C, uint64_t p, uint32_t flags) {
  return offset_of(c, C, p, flags) + k * p;
}

// x -> max(x + a, b); the identity is {0, 0} (x >= 0)
struct Map {
  uint64_t a, b;
};

__host__ __device__ inline Map request_map(uint64_t latency, uint64_t s) { return Map{latency, sat_add(s, latency)}; }
__host__ __device__ inline uint64_t apply(const Map &m, uint64_t x) {
  const uint64_t y = sat_add(x, m.a);
  return y > m.b ? y : m.b;
}
// `first`, then `second`
__host__ __device__ inline Map compose(const Map &first, const Map &second) {
  const uint64_t b = sat_add(first.b, second.a);
  return Map{sat_add(first.a, second.a), b > second.b ? b : second.b};
}

// ---- the device call's geometry (closed_loop.hip; host side, shared with the workspace size).
// The requests of a batch are a matrix of rows k by C columns in record order.  A workgroup of
// kThreads takes a block of R = G x M rows of a tile of Cw columns: thread (g, c) walks M rows of
// column c, the G sub-blocks of a column are scanned through LDS.  The workspace holds one Map
// per (row block, connection), overwritten by the state at the block's start.
constexpr uint32_t kThreads = 256;
constexpr uint32_t kStageBelow = 64;    // C below one wave: the block's records are staged in LDS
constexpr uint32_t kStageRows = 16;     // M of the staged regime: G x Cw x M <= 4096 latencies in LDS
constexpr uint32_t kTargetBlocks = 2048;  // row blocks x tiles aimed at (256 CUs x 8)
constexpr uint32_t kScanThreads = 1024;   // the composite scan of C < kScanThreads: one workgroup

struct Shape {
  uint32_t C, Cw, G, M, tiles;
  bool stage;
  uint64_t R, max_blocks;  // rows per block, and the row blocks a batch of n can need
};

// n >= 1; depends on n and C alone, so that isim_closed_loop_workspace_bytes bounds every first_index
inline Shape shape_of(uint64_t n, uint32_t C) {
  Shape s{};
  s.C = C;
  s.Cw = C < kThreads ? C : kThreads;
  s.G = kThreads / s.Cw;
  s.tiles = (C + s.Cw - 1) / s.Cw;
  s.stage = C < kStageBelow;
  const uint64_t max_rows = (n - 1) / C + 2;  // a batch that starts inside a row ends one row later
  if (s.stage) {
    s.M = kStageRows;
  } else {
    const uint64_t want_blocks = kTargetBlocks / s.tiles ? kTargetBlocks / s.tiles : 1;
    const uint64_t rows_per_block = (max_rows + want_blocks - 1) / want_blocks;
    const uint64_t m = (rows_per_block + s.G - 1) / s.G;
    s.M = (uint32_t)(m < kStageRows ? kStageRows : m);
  }
  s.R = s.stage ? (uint64_t)s.G * s.M : s.M;
  s.max_blocks = (max_rows + s.R - 1) / s.R;
  return s;
}

inline uint64_t workspace_bytes(uint64_t n, uint32_t C) {
  return n ? shape_of(n, C).max_blocks * C * sizeof(Map) : 0;
}

// ---- host side (closed_loop.cpp).  "" or why the client or the batch is refused
const char *client_error(const Client *cl);
const char *batch_error(const Client *cl, uint64_t n);

// ---- device side (closed_loop.hip): the launches of one checked batch; 0, or 1 (HIP error)
int launch(const Client &cl, const isim_trace_rec *d_records, uint64_t n, uint64_t *d_free_at,
           uint64_t *d_arrivals, uint64_t *d_info, void *d_workspace, void *stream);

}  // namespace cl
}  // namespace isim
