/*
 * isim.h — C ABI of the MI355X-native isotope trace simulator ("isim").
 *
 * This is the drop-in boundary for ONE hot path of adalrsjr1/istio-isotope:
 * executing isotope service-graph scripts (isotope/service/pkg/srv) for many
 * independent request traces, over graphs loaded with isotope's own
 * service-graph schema (isotope/convert/pkg/graph).  Plain C types only: a Go
 * host binds it through cgo, Python through ctypes.
 *
 * Reference interfaces replaced (file:line relative to the reference repo):
 *   isim_graph_unmarshal_json  <- (*graph.ServiceGraph).UnmarshalJSON
 *                                 isotope/convert/pkg/graph/unmarshal.go:30-48
 *                                 (reached through sigs.k8s.io/yaml.Unmarshal,
 *                                 isotope/service/pkg/srv/graph.go:82-94; the
 *                                 host does the YAML->JSON step)
 *   isim_handler_create        <- srv.HandlerFromServiceGraphYAML(path, name)
 *                                 isotope/service/pkg/srv/graph.go:34-60
 *                                 (extractService :97-109, extractServiceTypes :113-120)
 *   isim_serve / isim_serve_device
 *                              <- Handler.ServeHTTP  isotope/service/pkg/srv/handler.go:37-79
 *                                 + execute / executeRequestCommand /
 *                                 executeConcurrentCommand executable.go:43-179,
 *                                 run for n_traces independent client requests
 *                                 in virtual integer-nanosecond time
 *   stats words                <- prometheus.Record* isotope/service/pkg/srv/prometheus/handler.go:87-106
 *   isim_multi_* / isim_stats_allreduce_device / isim_stats_merge
 *                              <- the per-pod Prometheus scrape of those counters
 *                                 (prometheus/handler.go:37-69, one registry per
 *                                 pod): here one RCCL all-reduce over the ranks
 *                                 that each walked a shard of the traces
 *
 * Semantics: "isim semantics v1" (SURVEY.md Appendix A).
 * Errors: every function returns an isim_status; isim_last_error() gives a
 * thread-local message (the Go error text for graph-load errors).
 * Thread-safety: distinct handles may be used concurrently; a handle may be
 * served from several threads onto different devices.
 */
#ifndef ISIM_H
#define ISIM_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ISIM_ABI_VERSION 10

#if defined(__GNUC__)
#define ISIM_API __attribute__((visibility("default")))
#else
#define ISIM_API
#endif

typedef enum {
  ISIM_OK = 0,
  ISIM_EINVAL = 1,   /* bad argument, or no isEntrypoint service */
  ISIM_ENOMEM = 2,
  ISIM_EHIP = 3,     /* HIP runtime error */
  ISIM_EPARSE = 4,   /* graph load error: the Go error text is in isim_last_error() */
  ISIM_ECYCLE = 5,   /* call cycle reachable from the entry (would recurse forever) */
  ISIM_EDEPTH = 6,   /* call depth above isim_params.max_depth (<= 64) */
  ISIM_ERANGE = 7,   /* hop cost / latency bound overflows int64 */
  ISIM_ENOTFOUND = 8,/* service name not in graph */
  ISIM_ENODEV = 9,   /* no usable gfx950 device */
  ISIM_ECOMM = 10    /* RCCL error, or RCCL cannot be loaded (isim_multi_*) */
} isim_status;

/* Error propagation mode. */
#define ISIM_MODE_A 0u /* reference: a callee's 500 is swallowed (executable.go:131-143) */
#define ISIM_MODE_B 1u /* EXT: a callee's 500 fails the calling step and aborts the script */

typedef struct isim_graph isim_graph;
typedef struct isim_handler isim_handler;

/* Simulation parameters (the hop-cost model replaces the HTTP transport of
 * isotope/service/pkg/srv/request.go:30-64):
 *   H(call) = hop_base_ns + floor((size*req_ps_per_byte + responseSize(callee)*resp_ps_per_byte)/1000) */
typedef struct {
  uint64_t seed;             /* Philox4x32-10 key = (seed_lo, seed_hi) */
  uint64_t hop_base_ns;
  uint64_t req_ps_per_byte;
  uint64_t resp_ps_per_byte;
  uint32_t error_mode;       /* ISIM_MODE_A / ISIM_MODE_B */
  uint32_t max_depth;        /* 0 = 64; at most 64 */
  uint32_t flags;            /* ISIM_FLAG_* */
  uint32_t reserved;         /* must be 0 */
} isim_params;

/* isim_params.flags */
#define ISIM_FLAG_NO_STREAM 1u  /* run static walks on the interpreter kernel instead of the draw stream */
#define ISIM_FLAG_NO_SVC_DUR 2u /* dynamic walks: do not record per-service invocation durations */
#define ISIM_FLAG_WALK_ALL 4u   /* draw-free static walks: walk every trace (default: walk one, fill the rest) */
#define ISIM_FLAG_BIT_STACK 8u  /* mode B on the draw stream: the bit-stack kernel (kind 5, call depth <= 32;
                                   kind 4 deeper) instead of sparse ancestor marking (kind 8, the default) or
                                   the close-list kernel (kind 6) */
#define ISIM_FLAG_DYNAMIC 16u   /* treat every walk as dynamic: the general kernels with per-lane time and hop
                                   ids (kind 7, or 2/3) even when every trace executes the same invocations
                                   (parity tests of the general path on static graphs; no DES) */
#define ISIM_FLAG_WAVE_WALK 32u /* dynamic walks on the wave-walk interpreter (kinds 2/3: a wave walks the union
                                   of its 64 traces' call paths) instead of the lane tree walk (kind 7) */
#define ISIM_FLAG_CLOSE_LIST 64u /* mode B on the draw stream: the close-list kernel (kind 6) instead of sparse
                                    ancestor marking (kind 8, the default when its per-invocation mark table
                                    fits the LDS) */
/* Independent-check paths (the same results by a different algorithm; tests
 * compare them with the defaults at sizes the CPU oracle does not reach): */
#define ISIM_FLAG_TREE_WIDE 128u      /* dynamic walks: the wide lane-tree format (16-byte nodes, 32-bit frames)
                                         for any tree, not only past the 8-byte nodes' 16-bit fields */
#define ISIM_FLAG_DES_SCAN_BY_KEY 256u /* DES item engine: every queue by rocPRIM's scan by key over max-plus maps
                                         instead of the one-pass look-back scan (k_qscan) */
#define ISIM_FLAG_DES_SORT_ALL 512u   /* DES item engine, cyclic schedules: sort every queue round of every pass
                                         (no reuse of the previous pass's sorted order) */
#define ISIM_FLAG_DES_TWO_SORTS 1024u /* DES item engine: every sorted queue round by two stable sorts (replica |
                                         arrival, then service) instead of one combined key */
#define ISIM_FLAG_TREE_DAG 2048u      /* dynamic walks: the lane walk over the site graph (one node per call site)
                                         for any graph, not only where the unrolled tree would pass 2^24 positions */

/* One 16-byte record per simulated request trace. */
typedef struct {
  uint64_t latency_ns;       /* T(entry): virtual duration of the entry's ServeHTTP */
  uint32_t hops;             /* executed invocations (entry included) */
  uint32_t status_err;       /* bit31: entry responded 500; bits0-30: invocations that responded 500 */
} isim_trace_rec;

/* Layout of the u64 stats buffer filled by isim_serve*.  Offsets in words. */
#define ISIM_ST_N_TRACES 0
#define ISIM_ST_SUM_LATENCY 1
#define ISIM_ST_SUM_HOPS 2
#define ISIM_ST_SUM_ERR_HOPS 3
#define ISIM_ST_N_500 4
#define ISIM_ST_NOT_MIN_LATENCY 5 /* ~min latency (so min and max both merge with MAX) */
#define ISIM_ST_MAX_LATENCY 6
#define ISIM_ST_DES_RETRY 7       /* DES batches NOT accumulated: low 32 bits, a latency reached 2^31 ns in
                                     32-bit rows (rerun them with ISIM_DES_FLAG_WIDE; isim_serve_des does), or
                                     a cyclic schedule found no fixed point within 4096 passes; high 32 bits,
                                     batches FAILED by a device fault (a queue pass's decoupled look-back gave
                                     up waiting for an earlier tile: an error, never retried — isim_serve_des
                                     and the item engine return ISIM_EHIP; such a batch writes no record and
                                     counts no trace, and the item engine's per-site / DES-table words it may
                                     have added are undefined: discard the buffers) */
#define ISIM_ST_PROM 8            /* [2][33] latency histogram, Prometheus duration buckets
                                     (prometheus/handler.go:26-31), index [status500][bucket] */
#define ISIM_N_PROM 33
#define ISIM_ST_LOG2 (ISIM_ST_PROM + 2 * ISIM_N_PROM) /* [2][64] latency histogram by bit length */
#define ISIM_N_LOG2 64
#define ISIM_ST_SITES (ISIM_ST_LOG2 + 2 * ISIM_N_LOG2) /* [2][n_slots]: executed calls, then callee 500s,
                                                          per reachable call site slot */
/* Per-service duration table (service_request_duration_seconds and its _sum,
 * prometheus/handler.go:55-69,101-106), one row of ISIM_SVC_DUR_WORDS per
 * reachable service: [code 200|500][33] bucket counts, then the two duration
 * sums in ns.  Present in the stats buffer only when info.svc_dur_rows > 0
 * (dynamic walks); for static walks every invocation of a service lasts the
 * same T(s) and isim_stats_fold_durations derives the table from the
 * counters. */
#define ISIM_SVC_DUR_WORDS (2 * ISIM_N_PROM + 2)
#define ISIM_ST_SVC_DUR(n_slots) (ISIM_ST_SITES + 2 * (uint64_t)(n_slots))

/* Per-service row of the DES table filled by isim_serve_des* (config 5,
 * DESIGN.md §10): the service's invocation durations from request receipt to
 * response, queueing included, as ISIM_SVC_DUR_WORDS ([code][33] buckets on
 * the Prometheus duration edges, then the [code] sums in ns), followed by
 * the replica-queue figures.  Rows follow the duration-table row order
 * (reachable services in preorder; isim_des_fold maps them to services). */
#define ISIM_DES_COUNT ISIM_SVC_DUR_WORDS          /* invocations */
#define ISIM_DES_SUM_WAIT (ISIM_SVC_DUR_WORDS + 1) /* sum of queue waits, ns */
#define ISIM_DES_MAX_WAIT (ISIM_SVC_DUR_WORDS + 2) /* longest queue wait, ns */
#define ISIM_DES_SUM_HOLD (ISIM_SVC_DUR_WORDS + 3) /* worker busy time, ns */
#define ISIM_DES_ROW_WORDS (ISIM_SVC_DUR_WORDS + 4)

typedef struct {
  int32_t n_services;        /* services in the graph */
  int32_t n_sites;           /* call commands in the graph (document order) */
  int32_t n_slots;           /* call sites reachable from the entry (stats slots) */
  int32_t entry;             /* entry service index */
  int32_t max_depth;         /* deepest call chain from the entry (entry = 1) */
  int32_t static_walk;       /* 1: every invocation executes in every trace */
  int32_t time_bits;         /* 32 or 64: per-lane time width of the kernel */
  int32_t program_len;       /* instructions in the device program */
  uint64_t max_latency_ns;   /* static upper bound of any trace's latency */
  uint64_t hops_upper;       /* static upper bound of invocations per trace */
  uint64_t stats_words;      /* u64 words of the stats buffer */
  int32_t svc_dur_rows;      /* rows of the device duration table (0: derived on the host) */
  int32_t n_reachable;       /* services reachable from the entry */
  uint64_t draw_groups;      /* draw stream: groups of 4 invocations with an error draw (one Philox4x32-10
                                block per trace each); 0 for draw-free and dynamic walks */
} isim_handler_info;

/* Launch configuration chosen for a device (filled on first use of that device). */
typedef struct {
  int32_t wg_threads;        /* workgroup size (multiple of 64) */
  int32_t lds_bytes;         /* dynamic LDS per workgroup */
  int32_t lds_counters;      /* 1: per-site counters in LDS; 0: global atomics */
  int32_t blocks_per_cu;     /* resident workgroups per CU (occupancy query) */
  int32_t max_blocks;        /* resident workgroups on the device (grid cap) */
  int32_t kernel_kind;       /* 0/1 static interpreter u32/u64 time, 2/3 dynamic u32/u64, 4 draw stream,
                                5 draw stream with the mode-B bit stack (call depth <= 32),
                                6 draw stream with the mode-B close list (ISIM_FLAG_CLOSE_LIST, or a stream
                                too long for kind 8's LDS mark table),
                                7 lane tree walk (dynamic walks whose unrolled tree of potential
                                invocations has at most 2^24 positions, or the site graph, tree_wide 2;
                                every single figure of a position must stay below 2^32 ns — a call's
                                hop cost, a script's sleeps between two call steps or after the last,
                                the longest sleep of a concurrent step — though the latency bound may
                                pass it, and at most 65 calling invocations may nest; else 2/3),
                                8 draw stream with mode-B sparse ancestor marking (the default in mode B) */
  int32_t fill;              /* 1: a draw-free static walk: one trace walked, batches are a record fill
                                (isim_fill_const) + n x its statistics (off with ISIM_FLAG_WALK_ALL) */
  int32_t tree_wide;         /* kind 7 on a wide tree (more than 65,535 positions, call sites or rows, or
                                per-site counters past the LDS): 16-byte nodes, the hottest sites counted
                                in LDS, the rest by global atomics; 2: kind 7 on the site
                                graph (one node per call site: a DAG whose unrolled tree would pass 2^24
                                positions, or ISIM_FLAG_TREE_DAG), wide as 1; else 0 */
  uint64_t max_launch_traces; /* isim_serve_device splits a batch into launches of at most this many traces
                                 (per-workgroup u32 LDS counters must not wrap) */
} isim_launch_info;

ISIM_API const char *isim_last_error(void);
ISIM_API int isim_abi_version(void);

/* ---- graph (convert/pkg/graph) ---- */
ISIM_API int isim_graph_unmarshal_json(const char *json, size_t len, isim_graph **out);
ISIM_API void isim_graph_free(isim_graph *g);
ISIM_API int isim_graph_num_services(const isim_graph *g);
/* Exact implementation-neutral dump of the decoded graph.
 * Writes at most cap bytes (NUL-terminated when it fits); *len = bytes needed. */
ISIM_API int isim_graph_canonical_json(const isim_graph *g, char *buf, size_t cap, size_t *len);
/* json.Marshal(graph.ServiceGraph): svc/service.go:25-51 json tags + omitempty,
 * script.Script.MarshalJSON (script/script.go:24-31, command.go:30-53),
 * ByteSize/Percentage/ServiceType MarshalJSON (size/byte_size.go:31-34,
 * pct/percentage.go:32-35, svctype/service_type.go:45-48).  Same buffer
 * contract as isim_graph_canonical_json. */
ISIM_API int isim_graph_marshal_json(const isim_graph *g, char *buf, size_t cap, size_t *len);
/* graphviz.ServiceGraphToDotLanguage (convert/pkg/graphviz/graphviz.go:28-41):
 * the Graphviz DOT text of `isotope convert graphviz`. */
ISIM_API int isim_graph_to_dot(const isim_graph *g, char *buf, size_t cap, size_t *len);
/* extractService: first service with that name (graph.go:97-109); -1 if absent. */
/* ---- Kubernetes manifests (convert/pkg/kubernetes) ----
 * Replaces kubernetes.ServiceGraphToKubernetesManifests(serviceGraph,
 * serviceNodeSelector, serviceImage, serviceMaxIdleConnectionsPerHost,
 * clientNodeSelector, clientImage, environmentName)
 * (isotope/convert/pkg/kubernetes/kubernetes.go:56-63): Namespace, ConfigMap
 * (the graph as yaml.Marshal), per service a Deployment + Service (+ RBAC
 * rules under ISTIO), the Fortio client Deployment + Service, YAML documents
 * joined by "---\n" exactly as sigs.k8s.io/yaml v1.2.0 renders k8s.io/api
 * v0.18.0 objects.  Node selectors are n key/value pairs [k0, v0, k1, v1, ...]
 * (the CLI's "k=v" flag, cmd/kubernetes.go:96-108).  EXT: the reference stamps
 * time.Now() and names RBAC rules with uuid.New(); here every
 * creationTimestamp is creation_timestamp_s (UTC, RFC 3339) and the rule
 * names are v4 UUIDs from Philox4x32-10 keyed by rbac_seed. */
typedef struct {
  const char *service_image;                 /* "" / NULL: omitted, as Go's omitempty */
  const char *client_image;
  const char *environment_name;              /* "NONE" or "ISTIO" (strings.EqualFold); NULL = "NONE" */
  const char *const *service_node_selector;  /* 2 * n_service_node_selector strings */
  const char *const *client_node_selector;   /* 2 * n_client_node_selector strings */
  int32_t n_service_node_selector;
  int32_t n_client_node_selector;
  int32_t service_max_idle_connections_per_host;
  int32_t reserved;                          /* 0 */
  int64_t creation_timestamp_s;              /* unix seconds of every metadata.creationTimestamp */
  uint64_t rbac_seed;                        /* RBAC rule names (environment ISTIO, numRbacPolicies > 0) */
} isim_k8s_params;
/* Writes at most cap bytes (NUL-terminated when it fits); *len = bytes needed. */
ISIM_API int isim_graph_to_k8s_manifests(const isim_graph *g, const isim_k8s_params *p, char *buf, size_t cap,
                                         size_t *len);
/* yaml.Marshal(graph) (sigs.k8s.io/yaml: JSONToYAML of json.Marshal) — the ConfigMap payload. */
ISIM_API int isim_graph_marshal_yaml(const isim_graph *g, char *buf, size_t cap, size_t *len);
ISIM_API int isim_graph_service_index(const isim_graph *g, const char *name);

/* ---- units (convert/pkg/graph/size, pct, script/sleep_command.go) ---- */
ISIM_API int isim_size_from_string(const char *s, uint64_t *out);        /* size.FromString */
ISIM_API int isim_duration_parse(const char *s, int64_t *out_ns);        /* time.ParseDuration */
ISIM_API int isim_percentage_from_string(const char *s, double *out);    /* pct.FromString */

/* ---- handler (service/pkg/srv) ---- */
/* service_name NULL: the first service with isEntrypoint: true. */
ISIM_API int isim_handler_create(const isim_graph *g, const char *service_name, const isim_params *p,
                        isim_handler **out);
ISIM_API void isim_handler_free(isim_handler *h);
ISIM_API int isim_handler_info_get(const isim_handler *h, isim_handler_info *out);
/* Prepares `device` (uploads the program) and reports the launch configuration. */
ISIM_API int isim_handler_launch_info(isim_handler *h, int device, isim_launch_info *out);
/* Map of stats slots to the graph: slot -> call-site id (document order) and
 * callee service index.  Arrays of info.n_slots entries. */
ISIM_API int isim_handler_slots(const isim_handler *h, int32_t *slot_site, int32_t *slot_callee);

/* Serve n_traces requests (trace ids [trace_begin, trace_begin+n_traces)) on
 * the current HIP device, asynchronously on `hip_stream` (a hipStream_t, NULL =
 * default stream).  d_records: device array of n_traces records or NULL.
 * d_stats: device array of info.stats_words u64; ACCUMULATED into (zero it
 * first; ~min word starts at 0).  No host synchronisation, no allocation:
 * graph-capturable after the first call on a device.
 * Concurrency limit: the walk kernels claim batches from per-launch queue
 * sets (and draw-stream kernels stage their per-site 500 counts in per-launch
 * u32 rows, folded into d_stats by the launch's last kernel) that rotate
 * over 256 sets per (handler, device); at most 256 launches
 * of one handler may be in flight on one device at once (launches on ONE
 * stream are ordered and never collide; with more than 256 streams in
 * flight, order them with events or use one handler per stream).  A lane tree
 * walk deeper than its register frames (16 calling invocations on narrow
 * trees, fewer on wide ones) spills frames to one of up to 4 areas per
 * (handler, device), each allocated when a stream first needs it: each such
 * launch waits for the previous launch that used its area (an event recorded
 * after every spilling launch), so launches on different streams never share
 * frames.  A spilling walk cannot be graph-captured: on a capturing stream it
 * returns ISIM_EINVAL. */
ISIM_API int isim_serve_device(isim_handler *h, uint64_t trace_begin, uint64_t n_traces,
                      isim_trace_rec *d_records, uint64_t *d_stats, void *hip_stream);

/* Synchronous convenience: host buffers (either may be NULL), device `device`. */
ISIM_API int isim_serve(isim_handler *h, int device, uint64_t trace_begin, uint64_t n_traces,
               isim_trace_rec *h_records, uint64_t *h_stats);

/* Fold a stats buffer into per-service / per-call-site counters:
 * svc_calls[n_services] = incoming requests (RecordRequestReceived),
 * svc_errs[n_services]  = responses with code 500 (RecordResponseSent),
 * site_calls[n_sites]   = executed calls per call command (RecordRequestSent).
 * Any output may be NULL. */
ISIM_API int isim_stats_fold(const isim_handler *h, const uint64_t *stats, uint64_t *svc_calls,
                    uint64_t *svc_errs, uint64_t *site_calls);

/* Per-service invocation-duration histograms (RecordResponseSent's duration
 * observation, prometheus/handler.go:101-106, made at handler.go:56-58):
 * svc_dur[n_services][ISIM_SVC_DUR_WORDS] = per service [code][33] bucket
 * counts (non-cumulative; code 0 = 200, 1 = 500) then the [code] sums in ns.
 * ISIM_EINVAL when the handler was created with ISIM_FLAG_NO_SVC_DUR for a
 * dynamic walk. */
ISIM_API int isim_stats_fold_durations(const isim_handler *h, const uint64_t *stats, uint64_t *svc_dur);

/* ---- per-replica worker-pool DES (BASELINE config 5) ----
 * Open-loop Poisson arrivals of the client requests at the entry; every
 * replica of a service (svc.Service.NumReplicas, convert/pkg/graph/svc/
 * service.go:30-31) is a FIFO queue in front of ONE worker (or of W_s workers:
 * isim_des_workers_set below), held for the
 * invocation's sleep total; an invocation's script (Handler.ServeHTTP,
 * handler.go:37-79) starts when the worker takes it.  Statuses, hops and
 * call counters are those of the walk; latencies and the per-service
 * durations include queueing; in mode B a failed call step ends its script
 * there (the worker hold stays the sleep total).  Exact (bit-identical to the
 * sequential event-driven oracle) for the DES graph class of DESIGN.md
 * §10.1: static walks of at most 2^24 invocations and 65536 replicas per
 * service, and dynamic walks (probabilistic calls; in mode B, a step after
 * one that can fail) whose lane-tree-walk tree was built
 * (isim_des_info.items; isim_des_info_get returns ISIM_EINVAL with the
 * reason otherwise).  Times
 * are kept per trace relative to its arrival: in 32-bit rows by default;
 * a batch with a latency of 2^31 ns (2.1 s) or more is then not accumulated
 * (ISIM_ST_DES_RETRY counts it) and must be rerun with ISIM_DES_FLAG_WIDE
 * (64-bit rows).  A graph whose call-step
 * schedule is cyclic (a service with sleeps invoked both inside a caller's
 * call step and after it) runs as passes to a fixed point; its batches
 * synchronize hip_stream once per pass. */
#define ISIM_DES_FLAG_WIDE 1u    /* 64-bit rows: any latency */
typedef struct {
  uint64_t mean_interarrival_ns; /* 1 .. 2^34: mean gap of the exponential arrivals */
  uint32_t flags;                /* 0 or ISIM_DES_FLAG_WIDE */
  uint32_t reserved;             /* must be 0 */
} isim_des_params;

typedef struct {
  int32_t n_positions;           /* invocations per trace */
  int32_t n_levels;              /* depth of the invocation tree */
  int32_t max_width;             /* widest level */
  int32_t table_rows;            /* rows of the DES table (reachable services) */
  int32_t n_fused;               /* leaf positions finished in their queue pass (no up pass) */
  int32_t cyclic;                /* 1: the call-step schedule is cyclic (fixed-point passes) */
  int32_t row_reads;             /* rows one trace's batch reads (queue + finish passes, one pass), 4 or 8 B each */
  int32_t row_writes;            /* rows it writes (the algorithmic bytes of bench.py's roofline) */
  int32_t items;                 /* 1: a dynamic walk (probabilistic calls, mode-B aborts) on the item engine (DESIGN.md
                                    §10.9): positions are the tree's POTENTIAL invocations, a batch simulates the
                                    executed ones and synchronizes hip_stream at its item count and bucket sizes,
                                    once per sort round whose arrival range it reads back, and (a cyclic schedule)
                                    once per quiet pass — isim_des_last_batch reports the count */
} isim_des_info;

ISIM_API int isim_des_info_get(const isim_handler *h, isim_des_info *out);

/* The item engine's (isim_des_info.items) last batch served through this
 * handler, on any device, for reports: passes over the rounds (a cyclic
 * schedule's quiet passes and the recording pass; 1 otherwise), host
 * synchronisations of hip_stream (the item count, bucket sizes, each sort
 * round's arrival range, each quiet pass's change flag), executed
 * invocations.  Zero before the first item-engine batch. */
typedef struct {
  uint32_t passes;
  uint32_t syncs;
  uint64_t items;
} isim_des_batch_stats;
ISIM_API int isim_des_last_batch(const isim_handler *h, isim_des_batch_stats *out);
/* Worker pools (EXT): service s has W_s workers per
 * replica, 1 .. 65536, default 1, behind the replica's one FIFO queue.  Within
 * a replica the requests are ordered (arrival, trace, hop) as ever, and the
 * request of rank j (0-based, per replica, per batch) starts at
 *   S_j = max(a_j, S_{j - W_s} + P_s),   S_j = a_j for j < W_s,
 * P_s the service's worker hold; everything else of the DES is unchanged, and
 * with every W_s = 1 this is the one-worker rule.  workers[n_services], by
 * service index; NULL resets every service to 1.  Handler state: read at the
 * start of each DES batch of the handler (isim_serve_des*,
 * isim_serve_des_profile*, isim_serve_des_spans*, and through the spans the
 * DES critical path and the service timeline), not to be changed while one is
 * in flight.  A handler whose workers are all 1, set or never set, runs the
 * launches it always ran.  ISIM_EINVAL, before any HIP call: a count of 0 or
 * above 65536; n_services not the graph's; any count above 1 on a handler
 * whose DES runs on the static engine (isim_des_info.items == 0: create it
 * with ISIM_FLAG_DYNAMIC) or whose call-step schedule is cyclic
 * (isim_des_info.cyclic: not built). */
ISIM_API int isim_des_workers_set(isim_handler *h, const uint32_t *workers, uint32_t n_services);
/* host only, no GPU: the handler's workers per service, [n_services] (1 each until set) */
ISIM_API int isim_des_workers_get(const isim_handler *h, uint32_t *workers);
/* Device workspace a batch of n_traces needs (either row width: 8 B per invocation per trace + ~40 B per trace). */
ISIM_API int isim_des_workspace_bytes(const isim_handler *h, uint64_t n_traces, uint64_t *bytes);
/* One DES batch (trace ids [trace_begin, trace_begin+n_traces), arrivals from
 * time 0, all replicas idle) on the current device, asynchronously on
 * hip_stream.  d_records may be NULL; d_stats (info.stats_words) and
 * d_des_table (table_rows * ISIM_DES_ROW_WORDS) are ACCUMULATED into. */
ISIM_API int isim_serve_des_device(isim_handler *h, const isim_des_params *p, uint64_t trace_begin,
                          uint64_t n_traces, isim_trace_rec *d_records, uint64_t *d_stats,
                          uint64_t *d_des_table, void *d_workspace, uint64_t workspace_bytes,
                          void *hip_stream);
/* Synchronous convenience: host buffers (any may be NULL). */
ISIM_API int isim_serve_des(isim_handler *h, int device, const isim_des_params *p, uint64_t trace_begin,
                   uint64_t n_traces, isim_trace_rec *h_records, uint64_t *h_stats, uint64_t *h_des_table);
/* DES table rows -> svc_rows[n_services][ISIM_DES_ROW_WORDS] (zero for unreachable services). */
ISIM_API int isim_des_fold(const isim_handler *h, const uint64_t *des_table, uint64_t *svc_rows);
/* Test hook (no reference counterpart): the polls a DES queue pass's decoupled
 * look-back makes for an earlier tile before it fails the batch (device
 * fault flag; default 2^26, never reached in practice).  0 makes every
 * look-back fail at once, so tests can drive the error path.  Process-wide; read at each DES launch. */
ISIM_API void isim_debug_set_spin_limit(uint32_t polls);
ISIM_API uint32_t isim_debug_spin_limit(void);
/* Test hooks (no reference counterpart), host only.  The first is the pure
 * predicate a walk launch must meet to run the lean mode-A draw-stream kernel:
 * 1 for a group table, kernel kind 4, mode A and one high word for all of the
 * n_traces trace ids from trace_begin, else 0.  It does not know whether the
 * device has that kernel (ISIM_NO_LEAN_WALK=1 or ISIM_NO_GROUP_TABLE=1 at
 * device preparation leave it out).  The second counts the launches that did
 * run it, process-wide, at launch (or capture) time. */
ISIM_API int isim_debug_lean_walk_eligible(int has_table, uint32_t kernel_kind, int mode_b, uint64_t trace_begin,
                                           uint64_t n_traces);
ISIM_API uint64_t isim_debug_lean_walk_launches(void);

/* ---- multi-device: trace shards + one RCCL all-reduce ----
 * north_star: traces shard evenly across the GPUs of a node; the histograms
 * and counters merge with one RCCL all-reduce over xGMI.  An isim_multi is an
 * RCCL communicator with one or more LOCAL devices: one process per GPU
 * (isim_multi_init_rank, the id exchanged out of band, e.g. by the Go host)
 * or one process driving several GPUs (isim_multi_init_all).  Global rank r
 * walks the shard [trace_begin + r*n_per_rank, +n_per_rank); Philox keys use
 * the global trace id, so any rank count gives identical per-trace results.
 * The merge is SUM over every stats word except [~min, max], which merge by
 * MAX; DES tables (isim_des_table_allreduce_device) SUM except
 * ISIM_DES_MAX_WAIT (MAX).  RCCL is loaded at run time (dlopen of
 * librccl.so.1) on the first isim_multi_* call; ISIM_ECOMM if it cannot be. */
typedef struct isim_multi isim_multi;
typedef struct {
  char internal[128];            /* an ncclUniqueId */
} isim_multi_id;
/* New communicator id (on ONE process; send its 128 bytes to every rank). */
ISIM_API int isim_multi_get_id(isim_multi_id *id);
/* Local checks a rank makes BEFORE the collective creation, so that the
 * ranks can agree on them out of band first: RCCL loads and `device` can be
 * selected.  No communication. */
ISIM_API int isim_multi_precheck(int device);
/* This process is rank `rank` of n_ranks, on HIP device `device` (ncclCommInitRank; collective over the ranks).
 * Created non-blocking (ncclCommInitRankConfig, blocking = 0) when RCCL has it, and polled: if the
 * peers do not all arrive within ISIM_MULTI_TIMEOUT_S seconds (environment, default 120) the
 * communicator is aborted and ISIM_ECOMM returned.  Collectives and isim_serve_multi's wait are polled
 * the same way (hipStreamQuery + ncclCommGetAsyncError), so a rank whose peer aborted or never came
 * returns ISIM_ECOMM instead of waiting forever. */
ISIM_API int isim_multi_init_rank(const isim_multi_id *id, int n_ranks, int rank, int device, isim_multi **out);
/* One process, n_devices local devices = ranks 0..n-1 in the order given (ncclCommInitAll). */
ISIM_API int isim_multi_init_all(const int *devices, int n_devices, isim_multi **out);
ISIM_API void isim_multi_free(isim_multi *m);
/* Aborts the communicator (ncclCommAbort on every local comm): a rank that
 * fails before a collective calls it so that its peers' pending or next
 * collectives fail with ISIM_ECOMM instead of waiting forever.  The handle
 * is then only good for isim_multi_free; collectives on it return ECOMM. */
ISIM_API int isim_multi_abort(isim_multi *m);
ISIM_API int isim_multi_info(const isim_multi *m, int *n_ranks, int *n_local, int *first_rank);
/* In-place all-reduce of the stats buffers of the local devices (d_stats[i]
 * on local device i, enqueued on hip_streams[i]; hip_streams may be NULL =
 * default streams).  Asynchronous; collective over all ranks. */
ISIM_API int isim_stats_allreduce_device(const isim_handler *h, isim_multi *m, uint64_t *const *d_stats,
                                void *const *hip_streams);
/* The same for DES tables (n_reachable * ISIM_DES_ROW_WORDS words each). */
ISIM_API int isim_des_table_allreduce_device(const isim_handler *h, isim_multi *m, uint64_t *const *d_tables,
                                    void *const *hip_streams);
/* Synchronous sharded batch: every local device walks its rank's shard; the
 * merged stats (identical on every rank) go to h_stats, the local shards'
 * records (n_local * n_per_rank, local device order) to h_records; either may
 * be NULL.  Collective over all ranks.  A local HIP failure before the
 * all-reduce aborts the communicator when it has remote ranks
 * (isim_multi_abort), so the peers return ECOMM rather than hang. */
ISIM_API int isim_serve_multi(isim_handler *h, isim_multi *m, uint64_t trace_begin, uint64_t n_per_rank,
                     isim_trace_rec *h_records, uint64_t *h_stats);
/* Host-side merges (the same rules): dst += src. */
ISIM_API int isim_stats_merge(const isim_handler *h, uint64_t *dst, const uint64_t *src);
ISIM_API int isim_des_table_merge(const isim_handler *h, uint64_t *dst, const uint64_t *src);

/* ---- exact latency percentiles from per-trace records ----
 * The Fortio client's report (p50 / p75 / p90 / p99 / p99.9) as exact order
 * statistics of isim_trace_rec.latency_ns, computed on the device from the
 * records a walk or a DES batch just wrote: an MSD radix select, every class
 * and quantile in one sweep per 8-bit digit, at most 9 reads of the records.
 * Classes: every record, the 200s and the 500s (status_err bit 31).  For each
 * class c, out[c][0] is the count N_c of its records and out[c][1 + i] the
 * k-th smallest latency_ns among them, k = isim_quantile_rank(N_c, q_ppm[i])
 * (nearest rank); all 0 when N_c is 0.  The ranks are computed on the device
 * from the counts.  Any u64 latency is valid; q_ppm need not be sorted and may
 * repeat; n_records 0 gives all zeros.  ISIM_EINVAL: n_q 0 or above
 * ISIM_MAX_QUANTILES, a q_ppm above 1,000,000, n_records above 2^40, a
 * workspace below isim_quantiles_workspace_bytes(n_q), a null d_out or
 * d_workspace, a records pointer that is not 16-byte aligned. */
#define ISIM_MAX_QUANTILES 16
#define ISIM_Q_ALL 0   /* every record */
#define ISIM_Q_200 1   /* status_err bit31 clear */
#define ISIM_Q_500 2   /* status_err bit31 set  */
/* out: u64[3][1 + n_q]; per class: matching-record count, then the n_q values
   (all 0 when the count is 0) */
#define ISIM_Q_OUT_WORDS(n_q) (3 * (1 + (uint64_t)(n_q)))

/* nearest rank, 1-based: k = max(1, ceil(q_ppm * n / 1e6)); n in 1..2^40, q_ppm in 0..1000000 */
ISIM_API int isim_quantile_rank(uint64_t n, uint32_t q_ppm, uint64_t *k);       /* host only, no GPU */
ISIM_API int isim_quantiles_workspace_bytes(uint32_t n_q, uint64_t *bytes);     /* host only */
/* On the current device, asynchronously on hip_stream, like isim_serve_device:
 * no host synchronisation, no allocation, graph-capturable from the first
 * call.  q_ppm is a host array, copied at the call.  The call clears the
 * workspace state it needs: a dirty workspace may be reused (calls that share
 * one must be ordered, e.g. on one stream). */
ISIM_API int isim_latency_quantiles_device(const isim_trace_rec *d_records, uint64_t n_records,
                                           const uint32_t *q_ppm, uint32_t n_q,   /* host array, copied at the call */
                                           uint64_t *d_out, void *d_workspace, uint64_t workspace_bytes,
                                           void *hip_stream);
ISIM_API int isim_latency_quantiles(int device, const isim_trace_rec *h_records, uint64_t n_records,
                                    const uint32_t *q_ppm, uint32_t n_q, uint64_t *h_out);  /* synchronous convenience */

/* ---- the load-test timeline: arrival times and per-window latency ----
 * A DES batch's time axis.  isim_des_arrivals* exports the arrival times the
 * engine itself uses; isim_timeline* bins arrivals and records into windows of
 * simulated time.  Both run on the device, asynchronously on the caller's
 * stream: no host synchronisation, no allocation, graph-capturable from the
 * first call.
 *
 * A[i] = arrival (ns since batch start) of trace trace_begin + i, exactly the
 * value isim_serve_des* uses for the same handler seed, p->mean_interarrival_ns
 * and trace_begin (A_t = sum of X_i, i = trace_begin .. t; the
 * engine's own kernels).  Needs no DES plan: any handler, also one outside the
 * DES class.  The workspace may be dirty.  n_traces 0: ISIM_OK, nothing
 * written.  ISIM_EINVAL: a null h, p or arrivals buffer (n_traces > 0), a mean
 * outside 1..2^34, a nonzero p->reserved or unknown p->flags
 * (ISIM_DES_FLAG_WIDE is accepted and ignored), n_traces above 2^40, a
 * workspace below isim_des_arrivals_workspace_bytes(n_traces) or not 8-byte
 * aligned. */
ISIM_API int isim_des_arrivals_workspace_bytes(uint64_t n_traces, uint64_t *bytes);   /* host only */
ISIM_API int isim_des_arrivals_device(const isim_handler *h, const isim_des_params *p,
                                      uint64_t trace_begin, uint64_t n_traces, uint64_t *d_arrivals,
                                      void *d_workspace, uint64_t workspace_bytes, void *hip_stream);
ISIM_API int isim_des_arrivals(const isim_handler *h, int device, const isim_des_params *p,
                               uint64_t trace_begin, uint64_t n_traces, uint64_t *h_arrivals);

/* ---- load profiles: steps, spikes, pauses and paced arrivals ----
 * A time-varying offered load for the DES in place of the one mean of
 * isim_des_params.  A profile is 1 .. ISIM_LP_MAX_SEGMENTS segments; segment j
 * lasts duration_ns D_j (1 .. 2^48) at mean_interarrival_ns m_j (0 .. 2^34).
 * The last segment runs forever: its duration must be 0.  m_j = 0 is a pause
 * (no arrivals), not allowed as the last segment.  flags is 0 or ISIM_LP_PACED.
 *
 * The rule, exact integers (csrc/load_profile.h, one header for host and
 * device): arrivals are a time change of a unit-rate stream of work in Q24.
 *   compile  T_0 = C_0 = 0, W_j = floor(D_j 2^24 / m_j) (0 for a pause),
 *            T_{j+1} = T_j + D_j, C_{j+1} = min(C_j + W_j, 2^63)
 *   map      for u < 2^63: j = the largest index with C_j <= u,
 *            t(u) = T_j + floor((u - C_j) m_j / 2^24)   (128-bit product)
 *   work     of trace i (0-based) of a batch from trace_begin:
 *            u_i = sum of E(draw_k), k = trace_begin .. trace_begin + i, the
 *            draws and the Q24 exponential of DESIGN §10.1-§10.2 (no new
 *            randomness); with ISIM_LP_PACED, u_i = (i + 1) 2^24: evenly paced
 *            arrivals, one segment of mean m gives A_i = (i + 1) m exactly
 *   A_i = t(u_i), ns since the batch start, all replicas idle at 0.
 * t does not decrease in u.  A one-segment profile of mean m floors the sum
 * where the constant-mean entry points sum the floors:
 * A_const[i] <= A_profile[i] <= A_const[i] + i + 1; those entry points keep
 * their arithmetic bit for bit.
 *
 * The profile is a host structure, copied at the call.  Every ISIM_EINVAL
 * below is found before any HIP call: a null profile or segment pointer,
 * n_segments 0 or above the maximum, unknown flag bits, a duration or mean out
 * of range, a nonzero last duration, a pause as the last segment; n_traces
 * above 2^32 (arrivals) or 2^31 (DES); a batch whose horizon, t at the largest
 * work its traces can reach (n x 24 ln 2 x 2^24, paced n x 2^24), is at or
 * above 2^62; misaligned buffers; a workspace that is too small.
 *
 * isim_load_profile_time is the map on the host (no GPU): ISIM_ERANGE if
 * work_q24 >= 2^63 or t >= 2^63.
 *
 * isim_profile_arrivals* keep the contract of isim_des_arrivals*: any handler
 * (only its seed is read), n_traces 0 is ISIM_OK with nothing written, the
 * workspace may be dirty; asynchronous on hip_stream, no host synchronisation,
 * no allocation, graph-capturable from the first call (the segment table
 * travels in kernel arguments into the workspace).
 *
 * isim_serve_des_profile* keep every contract of isim_serve_des* (accumulation,
 * ISIM_ST_DES_RETRY, the same workspace of isim_des_workspace_bytes; the
 * synchronous call reruns with 64-bit rows) with A_i as above; des_flags is 0
 * or ISIM_DES_FLAG_WIDE.  The segment table lives in the handler's per-device
 * state: profile batches of one handler on one device must be ordered (one
 * stream, or events), as calls that share a workspace must.  The first
 * profile batch of a handler on a device allocates that table (hipMalloc),
 * so it cannot be captured in a graph under the default capture mode: run one
 * profile batch before capturing.  A call refused with ISIM_EINVAL has put
 * nothing on the stream and left the table as it was. */
#define ISIM_LP_MAX_SEGMENTS 1024u
#define ISIM_LP_PACED 1u
typedef struct {
  uint64_t duration_ns;           /* 1 .. 2^48; the last segment: 0 (forever) */
  uint64_t mean_interarrival_ns;  /* 0 (a pause) .. 2^34 */
} isim_load_segment;
typedef struct {
  const isim_load_segment *segments;
  uint32_t n_segments;            /* 1 .. ISIM_LP_MAX_SEGMENTS */
  uint32_t flags;                 /* 0 or ISIM_LP_PACED */
} isim_load_profile;

ISIM_API int isim_load_profile_time(const isim_load_profile *lp, uint64_t work_q24, uint64_t *t_ns);  /* host only */
ISIM_API int isim_profile_arrivals_workspace_bytes(uint64_t n_traces, uint64_t *bytes);                /* host only */
ISIM_API int isim_profile_arrivals_device(const isim_handler *h, const isim_load_profile *lp, uint64_t trace_begin,
                                          uint64_t n_traces, uint64_t *d_arrivals, void *d_workspace,
                                          uint64_t workspace_bytes, void *hip_stream);
ISIM_API int isim_profile_arrivals(const isim_handler *h, int device, const isim_load_profile *lp,
                                   uint64_t trace_begin, uint64_t n_traces, uint64_t *h_arrivals);
ISIM_API int isim_serve_des_profile_device(isim_handler *h, const isim_load_profile *lp, uint32_t des_flags,
                                           uint64_t trace_begin, uint64_t n_traces, isim_trace_rec *d_records,
                                           uint64_t *d_stats, uint64_t *d_des_table, void *d_workspace,
                                           uint64_t workspace_bytes, void *hip_stream);
ISIM_API int isim_serve_des_profile(isim_handler *h, int device, const isim_load_profile *lp, uint64_t trace_begin,
                                    uint64_t n_traces, isim_trace_rec *h_records, uint64_t *h_stats,
                                    uint64_t *h_des_table);

/* Record i arrives at a = arrivals[i] and completes at c = a + latency_ns,
 * saturating at 2^64 - 1.  A time x falls in row 0 ("before") if x < t0_ns;
 * otherwise, with w = floor((x - t0_ns) / window_ns), in row 1 + w if
 * w < n_windows, else in row n_windows + 1 ("after").  A time equal to a
 * window's start belongs to that window; t0_ns + n_windows * window_ns is
 * never formed.  The code is bit 31 of status_err, the histogram's bucket the
 * one of ISIM_ST_PROM.  Exact integer arithmetic for every u64 input; the
 * arrivals need not be sorted.  out is ACCUMULATED into, like d_stats (zero it
 * first): sums and counts by add, ISIM_TL_MAX_LAT by max; so batches, shards
 * and GPUs fold into one table, on the device by calling again and on the host
 * with isim_timeline_merge.  Requests in flight at the end of window w:
 * sum over rows r <= 1 + w (with "before") of ARRIVED - DONE[0] - DONE[1].
 * n 0: ISIM_OK, nothing touched.  ISIM_EINVAL: a null p or out, null arrivals
 * or records with n > 0, window_ns 0, n_windows 0 or above
 * ISIM_TL_MAX_WINDOWS, a nonzero reserved, n above 2^40, records not 16-byte
 * or arrivals / out not 8-byte aligned. */
#define ISIM_TL_MAX_WINDOWS 65536u
typedef struct {
  uint64_t t0_ns;       /* start of window 0 */
  uint64_t window_ns;   /* >= 1 */
  uint32_t n_windows;   /* 1 .. ISIM_TL_MAX_WINDOWS */
  uint32_t reserved;    /* 0 */
} isim_timeline_params;

/* Row words (u64), one row per window, preceded by row "before" (index 0) and
 * followed by row "after" (index n_windows + 1): out[(n_windows + 2)][ISIM_TL_ROW_WORDS] */
#define ISIM_TL_ARRIVED  0                       /* records whose ARRIVAL falls in the window */
#define ISIM_TL_DONE     1                       /* [2] records whose COMPLETION falls in it, by code 200|500 */
#define ISIM_TL_SUM_LAT  3                       /* [2] sum of latency_ns of those, by code */
#define ISIM_TL_MAX_LAT  5                       /* [2] max latency_ns of those, by code */
#define ISIM_TL_PROM     7                       /* [2][ISIM_N_PROM] latency histogram of those, the stats buffer's edges */
#define ISIM_TL_ROW_WORDS (7 + 2 * ISIM_N_PROM)  /* 73 */

ISIM_API int isim_timeline_device(const uint64_t *d_arrivals, const isim_trace_rec *d_records, uint64_t n,
                                  const isim_timeline_params *p, uint64_t *d_out, void *hip_stream);
/* Synchronous convenience: host buffers; h_out is accumulated into as well. */
ISIM_API int isim_timeline(int device, const uint64_t *h_arrivals, const isim_trace_rec *h_records, uint64_t n,
                           const isim_timeline_params *p, uint64_t *h_out);
ISIM_API int isim_timeline_merge(uint32_t n_windows, uint64_t *dst, const uint64_t *src);  /* host: SUM, MAX words by MAX */

/* ---- per-window exact latency percentiles: p99 over time ----
 * For every row of the timeline above (the same isim_timeline_params, the
 * same rules for them, the same rows), the exact order statistics of the
 * latencies that COMPLETE in it (c = arrivals[i] + latency_ns, saturating), by
 * the classes of isim_latency_quantiles (ISIM_Q_ALL / ISIM_Q_200 / ISIM_Q_500,
 * bit 31 of status_err).  out is u64[n_windows + 2][3][1 + n_q]: out[r][c][0]
 * is the count N of records of class c completing in row r, out[r][c][1 + i]
 * the k-th smallest latency_ns among them, k = isim_quantile_rank(N, q_ppm[i])
 * (nearest rank); all 0 where N is 0.  Unlike the timeline table, out is
 * WRITTEN, not accumulated (order statistics do not merge): every word is
 * written by the call, so out may be dirty; n 0 writes all zeros; to cover
 * several batches pass their concatenated arrivals and records.  Any u64
 * latency is valid, the arrivals need not be sorted; q_ppm is a host array
 * copied at the call, 1 .. ISIM_MAX_QUANTILES entries, each <= 1,000,000, in
 * any order, repeats allowed.
 * n is at most 2^32 - 1: the call needs 8 B of workspace per record (the
 * latencies, grouped by row) and its per-row counters, offsets and ranks are
 * 32-bit.  ISIM_EINVAL, before any HIP call: the parameter errors of
 * isim_timeline*, the quantile-list errors of isim_latency_quantiles*, n above
 * 2^32 - 1, a null out or workspace, null arrivals or records with n > 0,
 * records not 16-byte or arrivals / out / workspace not 8-byte aligned, a
 * workspace below isim_timeline_quantiles_workspace_bytes(n, n_windows, n_q).
 * The device entry keeps the contract of isim_latency_quantiles_device:
 * asynchronous on hip_stream, no host synchronisation, no allocation,
 * graph-capturable from the first call; the workspace may be dirty, and calls
 * that share one must be ordered (e.g. on one stream). */
#define ISIM_TLQ_OUT_WORDS(n_windows, n_q) (((uint64_t)(n_windows) + 2) * ISIM_Q_OUT_WORDS(n_q))
ISIM_API int isim_timeline_quantiles_workspace_bytes(uint64_t n, uint32_t n_windows, uint32_t n_q,
                                                     uint64_t *bytes);               /* host only */
ISIM_API int isim_timeline_quantiles_device(const uint64_t *d_arrivals, const isim_trace_rec *d_records, uint64_t n,
                                            const isim_timeline_params *p, const uint32_t *q_ppm, uint32_t n_q,
                                            uint64_t *d_out, void *d_workspace, uint64_t workspace_bytes,
                                            void *hip_stream);
ISIM_API int isim_timeline_quantiles(int device, const uint64_t *h_arrivals, const isim_trace_rec *h_records,
                                     uint64_t n, const isim_timeline_params *p, const uint32_t *q_ppm, uint32_t n_q,
                                     uint64_t *h_out);                               /* synchronous convenience */

/* ---- mergeable latency sketch: percentiles across batches, shards and GPUs ----
 * A log-linear histogram of latency_ns (the HdrHistogram / Fortio kind) whose
 * every word merges by addition, so that percentiles survive what the exact
 * selects above cannot: many batches, shards and GPUs, without keeping the
 * records.  s = sub_bits in 0 .. ISIM_SK_MAX_SUB_BITS refines the bit-length
 * histogram (s = 0 is ISIM_ST_LOG2 with a bin for 0) by s further bits.
 *
 * The bucket rule, exact integer arithmetic for every u64 v (csrc/sketch_bucket.h,
 * one header for host and device): if v < 2^(s+1), bin = v (the exact region);
 * otherwise shift = bitlen(v) - (s + 1) and bin = (shift << s) + (v >> shift).
 * The rule is continuous at 2^(s+1); the last bin, ISIM_SK_BINS(s) - 1, holds
 * 2^64 - 1.  Bounds of a bin: lo = hi = bin if bin < 2^(s+1); otherwise
 * shift = (bin >> s) - 1, lo = (2^s + (bin & (2^s - 1))) << shift and
 * hi = lo + 2^shift - 1, hence hi - lo < lo >> s strictly: at s = 7 a bracket
 * is narrower than 0.79 % of the value and every latency below 256 ns is exact.
 *
 * A table is u64[2][ISIM_SK_BINS(s)], indexed by code (0: a 200, 1: a 500, bit
 * 31 of status_err) and bin.  It is ACCUMULATED into, like d_stats (zero it
 * first), and holds counts only, no min or max word: batches fold on the
 * device by calling again, on the host with isim_sketch_merge, and across GPUs
 * by a SUM all-reduce of the raw words.
 *
 * isim_sketch_quantiles reads one table: out is u64[3][1 + 2 * n_q], by the
 * classes ISIM_Q_ALL / ISIM_Q_200 / ISIM_Q_500 (ALL is the sum of the two code
 * rows).  out[c][0] is the count N_c, out[c][1 + 2i] and out[c][2 + 2i] the lo
 * and hi of the bin in which the running count first reaches
 * k = isim_quantile_rank(N_c, q_ppm[i]): the bracket [lo, hi] contains the exact
 * order statistic.  All words are 0 where N_c is 0.  The quantile list follows
 * isim_latency_quantiles (1 .. ISIM_MAX_QUANTILES entries, each <= 1,000,000,
 * any order, repeats allowed); a class count above 2^40 is ISIM_EINVAL.
 *
 * isim_latency_sketch_device: one kernel launch on the current device,
 * asynchronous on hip_stream, no workspace, no host synchronisation, no
 * allocation, graph-capturable from the first call.  n 0: ISIM_OK, nothing
 * touched.  ISIM_EINVAL, before any HIP call: sub_bits above
 * ISIM_SK_MAX_SUB_BITS, a null table, null records with n > 0, n above 2^40,
 * records not 16-byte or the table not 8-byte aligned.
 *
 * isim_timeline_sketch*: one table per row of the timeline (the same
 * isim_timeline_params, rules and rows as isim_timeline_quantiles: by
 * COMPLETION, c = arrivals[i] + latency_ns, saturating): out is
 * u64[n_windows + 2][2][ISIM_SK_BINS(s)], accumulated into; exact for unsorted
 * arrivals.  The rows summed are the whole-batch table.  Errors: the parameter
 * errors of isim_timeline*, plus those above (arrivals 8-byte aligned). */
#define ISIM_SK_MAX_SUB_BITS 7
#define ISIM_SK_BINS(s) ((uint64_t)(65 - (s)) << (s))          /* 65 at s = 0, 496 at s = 3, 7424 at s = 7 */
#define ISIM_SK_WORDS(s) (2 * ISIM_SK_BINS(s))                 /* u64 words of one table */
#define ISIM_SKQ_OUT_WORDS(n_q) (3 * (1 + 2 * (uint64_t)(n_q)))   /* isim_sketch_quantiles' out */
#define ISIM_TLS_OUT_WORDS(n_windows, s) (((uint64_t)(n_windows) + 2) * ISIM_SK_WORDS(s))
/* host only, no GPU */
ISIM_API int isim_sketch_bucket(uint32_t sub_bits, uint64_t v, uint32_t *bin);
ISIM_API int isim_sketch_bounds(uint32_t sub_bits, uint32_t bin, uint64_t *lo, uint64_t *hi);
/* dst += src over n_rows tables (n_rows 1 for a whole-batch table, n_windows + 2 for a per-window one) */
ISIM_API int isim_sketch_merge(uint32_t sub_bits, uint64_t n_rows, uint64_t *dst, const uint64_t *src);
ISIM_API int isim_sketch_quantiles(uint32_t sub_bits, const uint64_t *table, const uint32_t *q_ppm, uint32_t n_q,
                                   uint64_t *out);
ISIM_API int isim_latency_sketch_device(const isim_trace_rec *d_records, uint64_t n, uint32_t sub_bits,
                                        uint64_t *d_table, void *hip_stream);
/* Synchronous convenience: host buffers; h_table is accumulated into as well. */
ISIM_API int isim_latency_sketch(int device, const isim_trace_rec *h_records, uint64_t n, uint32_t sub_bits,
                                 uint64_t *h_table);
ISIM_API int isim_timeline_sketch_device(const uint64_t *d_arrivals, const isim_trace_rec *d_records, uint64_t n,
                                         const isim_timeline_params *p, uint32_t sub_bits, uint64_t *d_out,
                                         void *hip_stream);
ISIM_API int isim_timeline_sketch(int device, const uint64_t *h_arrivals, const isim_trace_rec *h_records, uint64_t n,
                                  const isim_timeline_params *p, uint32_t sub_bits, uint64_t *h_out);

/* ---- closed-loop clients: connection-limited arrivals for every walk (EXT) ----
 * The reference's load client (Fortio: num_concurrent_connections, qps) is a
 * closed loop: each of C connections sends its next request only when the
 * previous response has arrived and, with a numeric qps, never before its paced
 * slot.  For a walk a trace's latency does not depend on when it starts, so the
 * arrival times of a batch of finished records are an exact integer recurrence
 * along each connection.  The result is a u64 arrivals[n], which isim_timeline*,
 * isim_timeline_quantiles* and isim_timeline_sketch* take as it is.
 *
 * A client has `connections` C (1 .. ISIM_CL_MAX_CONNECTIONS) and a period
 * p = period_ns per connection (0: "max", no pacing; else 1 .. 2^40).  flags is
 * 0 or ISIM_CL_UNIFORM (the connections' slots staggered, Fortio's -uniform).
 * A run is a sequence of requests j = 0, 1, 2, ...; a batch covers requests
 * first_index .. first_index + n - 1 (first_index <= 2^40, n <= 2^32); request
 * first_index + i is record i.  The rule (csrc/closed_loop.h, one header for
 * host and device):
 *   c = j mod C,  k = j div C                    connection and its k-th request
 *   o_c = floor(c p / C) with ISIM_CL_UNIFORM, else 0
 *   s_j = o_c + k p                              scheduled start
 *   A_j = max(F_c, s_j)                          actual start: arrivals[i]
 *   F_c <- A_j + latency_ns(record i)            connection c is free again
 * Every addition saturates at 2^64 - 1 (as the timeline's completion time), so
 * the rule is defined for every u64 latency.  F is the state u64 free_at[C]:
 * read at the call, overwritten with the state after the batch; a connection
 * with no request in the batch keeps its value; all zeros starts a run; a null
 * pointer means zeros in and nothing out.  Successive batches with consecutive
 * first_index that pass the state along equal one big batch, value for value.
 * Request j is the map x -> max(x + L_j, s_j + L_j); (a1, b1) followed by
 * (a2, b2) composes to (a1 + a2, max(b1 + a2, b2)), which is associative under
 * saturation, so the device's scan along each connection is exact.
 *
 * info is u64[ISIM_CL_INFO_WORDS], WRITTEN (not accumulated): the max and the
 * min of free_at over all C connections after the batch, the number of requests
 * of the batch with A_j > s_j and the sum of A_j - s_j mod 2^64 (coordinated
 * omission).  The achieved rate of a run is requests / makespan.
 *
 * ISIM_EINVAL, always before any HIP call: a null client, info or (n > 0)
 * records or arrivals pointer; connections 0 or above the maximum; unknown
 * flags; a period above 2^40; first_index above 2^40; n above 2^32; a batch
 * whose last scheduled start o_c + k_max p, k_max = (first_index + n - 1) div C,
 * would reach 2^63; records not 16-byte aligned, the other buffers not 8-byte
 * aligned; a null or too small workspace (n > 0).
 *
 * isim_closed_loop_device keeps the contract of isim_latency_quantiles_device:
 * asynchronous on hip_stream, no host synchronisation, no allocation,
 * graph-capturable from the first call; the workspace may be dirty (calls that
 * share one must be ordered).  n 0: ISIM_OK, info written from the incoming
 * state, everything else untouched (no workspace needed). */
#define ISIM_CL_MAX_CONNECTIONS 65536u
#define ISIM_CL_UNIFORM 1u
#define ISIM_CL_MAKESPAN 0   /* max of free_at after the batch */
#define ISIM_CL_MIN_FREE 1   /* min of free_at after the batch */
#define ISIM_CL_LATE     2   /* requests of the batch with A_j > s_j */
#define ISIM_CL_SUM_LATE 3   /* sum of A_j - s_j, mod 2^64 */
#define ISIM_CL_INFO_WORDS 4
/* a struct tag, not a typedef: the synchronous entry point bears the same name */
struct isim_closed_loop {
  uint32_t connections;   /* 1 .. ISIM_CL_MAX_CONNECTIONS */
  uint32_t flags;         /* 0 or ISIM_CL_UNIFORM */
  uint64_t period_ns;     /* 0 ("max") or 1 .. 2^40, per connection */
  uint64_t first_index;   /* the run's index of record 0, <= 2^40 */
};

/* host only, no GPU: request j's connection and scheduled start (first_index is not read) */
ISIM_API int isim_closed_loop_schedule(const struct isim_closed_loop *cl, uint64_t j, uint32_t *c, uint64_t *s_ns);
/* host only, no GPU: the rule as a plain sequential loop */
ISIM_API int isim_closed_loop_host(const struct isim_closed_loop *cl, const isim_trace_rec *h_records, uint64_t n,
                                   uint64_t *h_free_at, uint64_t *h_arrivals, uint64_t *h_info);
ISIM_API int isim_closed_loop_workspace_bytes(uint64_t n, uint32_t connections, uint64_t *bytes);  /* host only */
ISIM_API int isim_closed_loop_device(const struct isim_closed_loop *cl, const isim_trace_rec *d_records, uint64_t n,
                                     uint64_t *d_free_at, uint64_t *d_arrivals, uint64_t *d_info,
                                     void *d_workspace, uint64_t workspace_bytes, void *hip_stream);
/* Synchronous convenience: host buffers (h_free_at may be NULL). */
ISIM_API int isim_closed_loop(int device, const struct isim_closed_loop *cl, const isim_trace_rec *h_records, uint64_t n,
                              uint64_t *h_free_at, uint64_t *h_arrivals, uint64_t *h_info);

/* ---- trace spans: the executed invocations of chosen traces (EXT) ----
 * A dynamic walk keeps 16 bytes per trace.  A trace is a pure function of
 * (seed, trace id), so the invocations behind any record come from walking
 * that id again: the role of the reference's Jaeger spans (service/main.go).
 * Handlers with an unrolled tree of potential invocations only (a dynamic walk,
 * or any graph under ISIM_FLAG_DYNAMIC; not the site graph).
 *
 * The spans of one trace are contiguous and ordered by hop.  The entry's
 * duration_ns is the record's latency_ns, its status bit 0 the record's status,
 * the number of spans the record's hops, the spans with bit 0 set the record's
 * 500 count.
 *
 * start_ns replays the caller's script (handler.go:66-76) with a
 * clock that starts at the caller's own start_ns: a sleep adds max(d, 0); an
 * executed call starts at the clock and adds H + T, a skipped call adds 0; every
 * child of a concurrent step starts at the step's start, and the step adds the
 * largest of its children's H + T and its sleeps. */
typedef struct {
  uint64_t start_ns;     /* when the caller sends the request, from the trace's start; entry 0 */
  uint64_t duration_ns;  /* the callee's own duration T (§2.4): receipt to respond point, no hop cost */
  uint64_t hop_ns;       /* H of the call site (§2.2); entry 0.  The call occupies [start, start + H + T] */
  uint32_t hop;          /* preorder index among the trace's executed invocations (§2.3), entry 0 */
  uint32_t caller_hop;   /* 0xFFFFFFFF for the entry */
  uint32_t position;     /* position in the unrolled tree */
  uint32_t slot;         /* call-site slot (isim_handler_slots); 0xFFFFFFFF for the entry */
  uint32_t service;      /* callee service index; the entry service for hop 0 */
  uint32_t status;       /* bit 0: responded 500; bit 1: its own error draw (mode B: bit 0 without bit 1 = a failed step) */
} isim_span;             /* 48 bytes */

#define ISIM_SPAN_TOTAL   0   /* spans of every listed trace (what cap_spans must reach for all to fit) */
#define ISIM_SPAN_WRITTEN 1   /* traces written: the list entries before the first that did not fit */
#define ISIM_SPAN_N_IDS   2   /* n_ids */
#define ISIM_SPAN_FIRST_UNFIT 3 /* first list index whose spans did not fit cap_spans, or n_ids */
#define ISIM_SPAN_INFO_WORDS 4

/* host only, no GPU */
ISIM_API int isim_trace_spans_workspace_bytes(const isim_handler *h, uint64_t n_ids, uint64_t *bytes);
/* The spans of the traces d_trace_ids[0 .. n_ids) (any u64, unsorted, repeats
 * allowed; n_ids <= 2^32) on the current device, asynchronously on hip_stream:
 * d_off[n_ids + 1] the exclusive scan of the traces' hops, the spans of list
 * entry i at d_spans[d_off[i] + hop] when d_off[i + 1] <= cap_spans (a trace
 * that does not fit writes nothing), d_info[ISIM_SPAN_INFO_WORDS] written.
 * start_ns is left 0 (isim_trace_spans_place fills it on the host).  Three
 * steps ordered by the stream: a counting walk, a scan, an emitting walk.  No
 * host synchronisation, graph-capturable from the first call, the workspace may
 * be dirty (calls that share one must be ordered); the first call of a handler
 * on a device uploads the handler's tree tables.  n_ids 0 writes d_off[0] = 0
 * and d_info, nothing else.  ISIM_EINVAL, before any HIP call: a null argument,
 * a handler without an unrolled tree (a static walk: create the handler with
 * ISIM_FLAG_DYNAMIC) or on the site graph, n_ids above 2^32, buffers not 8-byte
 * aligned, a workspace below isim_trace_spans_workspace_bytes(h, n_ids). */
ISIM_API int isim_trace_spans_device(const isim_handler *h, const uint64_t *d_trace_ids, uint64_t n_ids,
                                     uint64_t *d_off, isim_span *d_spans, uint64_t cap_spans, uint64_t *d_info,
                                     void *d_workspace, uint64_t workspace_bytes, void *hip_stream);
/* Synchronous convenience: host buffers, start_ns filled. */
ISIM_API int isim_trace_spans(int device, const isim_handler *h, const uint64_t *h_trace_ids, uint64_t n_ids,
                              uint64_t *h_off, isim_span *h_spans, uint64_t cap_spans, uint64_t *h_info);
/* host only, no GPU: the same walk on the CPU, start_ns filled */
ISIM_API int isim_trace_spans_host(const isim_handler *h, const uint64_t *h_trace_ids, uint64_t n_ids,
                                   uint64_t *h_off, isim_span *h_spans, uint64_t cap_spans, uint64_t *h_info);
/* host only, no GPU: fills start_ns of the n_written traces whose spans lie at
 * h_spans[h_off[i] .. h_off[i + 1]), one pass per trace in hop order */
ISIM_API int isim_trace_spans_place(const isim_handler *h, const uint64_t *h_off, uint64_t n_written,
                                    isim_span *h_spans);

/* The ids trace_begin + i, in ascending i, of the records with
 * latency_ns >= min_latency_ns in class cls (ISIM_Q_ALL / ISIM_Q_200 /
 * ISIM_Q_500): the first max_ids of them at d_ids, d_info = {matches, written}.
 * Count per block, scan, scatter: the order is deterministic.  The contract of
 * isim_trace_spans_device; n <= 2^40, records 16-byte aligned. */
ISIM_API int isim_select_traces_workspace_bytes(uint64_t n, uint64_t *bytes);  /* host only */
ISIM_API int isim_select_traces_device(const isim_trace_rec *d_records, uint64_t n, uint64_t trace_begin,
                                       uint64_t min_latency_ns, uint32_t cls, uint64_t max_ids, uint64_t *d_ids,
                                       uint64_t *d_info, void *d_workspace, uint64_t workspace_bytes,
                                       void *hip_stream);
ISIM_API int isim_select_traces(int device, const isim_trace_rec *h_records, uint64_t n, uint64_t trace_begin,
                                uint64_t min_latency_ns, uint32_t cls, uint64_t max_ids, uint64_t *h_ids,
                                uint64_t *h_info);
ISIM_API int isim_select_traces_host(const isim_trace_rec *h_records, uint64_t n, uint64_t trace_begin,
                                     uint64_t min_latency_ns, uint32_t cls, uint64_t max_ids, uint64_t *h_ids,
                                     uint64_t *h_info);  /* no GPU */

/* ---- critical path of chosen traces: per-service time on it (EXT) ----
 * Across a list of traces (the tail of a batch, usually): which services hold
 * the latency?  The rule, over one trace's spans in hop order and the handler's
 * scripts.  Each caller's script is replayed as start_ns replays it (above):
 * the clock starts at the caller's start_ns, the caller's executed children are
 * taken in hop order, each matched to the call command whose index its
 * position's node carries.
 *
 * Local winners.  An executed child of a sequential call command is a local
 * winner.  In a concurrent step the members are scanned in listed order with
 * longest = 0; a member's value is hop_ns + duration_ns for an executed call, 0
 * for a skipped call, max(d, 0) for a sleep; a member takes the lead only when
 * its value is strictly greater than longest; the step's winner is the last
 * member that took the lead (it may be a sleep, and there may be none).  So ties
 * go to the first listed member and a zero-cost child never wins.  A child of a
 * concurrent step is a local winner iff it is its step's winner.
 *
 * Critical set.  The entry is critical; any other span is critical iff it is a
 * local winner and its caller is critical.
 *
 * Self time.  self_ns(v) = duration_ns(v) - the sum over v's local-winner
 * children c of (hop_ns(c) + duration_ns(c)): the time v spends in its own
 * sleeps, concurrent steps that a sleep won included.  It is never negative
 * for the spans of a walk (isim_critical_path_host returns ISIM_EINVAL if it
 * would be; its outputs are then unspecified).  Mode B needs no extra rule:
 * nothing follows a failed step, and the spans already say which children ran.
 *
 * Identity.  For every trace the sum over its critical spans of (self_ns +
 * hop_ns) equals the entry's duration_ns, the record's latency_ns.
 *
 * The table: (n_services + 1) rows of ISIM_CP_ROW_WORDS u64 words, every word a
 * sum mod 2^64, so tables merge by plain addition across calls, batches, shards
 * and GPUs.  Row s < n_services: the words below.  The last row is the header.
 * Per table the sum over s of (SELF_NS + HOP_NS) equals the header's
 * ISIM_CP_H_SUM_LATENCY. */
#define ISIM_SPAN_CRITICAL 4u    /* isim_span.status bit 2: on the critical path (set by isim_critical_path* only) */
#define ISIM_CP_INVOCATIONS  0   /* every executed invocation of s in the processed traces */
#define ISIM_CP_SUM_DURATION 1   /* the sum of duration_ns of those invocations */
#define ISIM_CP_CRITICAL     2   /* invocations of s on the path */
#define ISIM_CP_SELF_NS      3   /* the sum of self_ns of the critical invocations */
#define ISIM_CP_HOP_NS       4   /* the sum of hop_ns of the critical invocations: the network time of the calls into s */
#define ISIM_CP_CRITICAL_500 5   /* critical invocations that responded 500 */
#define ISIM_CP_ROW_WORDS    6
/* the header row (row n_services); its last word is 0 */
#define ISIM_CP_H_TRACES      0  /* traces processed */
#define ISIM_CP_H_SPANS       1  /* their spans */
#define ISIM_CP_H_CRITICAL    2  /* their critical spans */
#define ISIM_CP_H_SUM_LATENCY 3  /* the sum of their entries' duration_ns */
#define ISIM_CP_H_REFUSED     4  /* traces refused: not the spans of a walk; left untouched, counted nowhere else */

/* host only, no GPU: (n_services + 1) * ISIM_CP_ROW_WORDS */
ISIM_API int isim_critical_path_table_words(const isim_handler *h, uint64_t *words);
/* host only, no GPU: 8 bytes per span of the buffer plus 64 */
ISIM_API int isim_critical_path_workspace_bytes(const isim_handler *h, uint64_t cap_spans, uint64_t *bytes);
/* host only, no GPU: dst[w] += src[w] over the table's words */
ISIM_API int isim_critical_path_merge(const isim_handler *h, uint64_t *dst, const uint64_t *src);
/* The critical path of the d_info[ISIM_SPAN_WRITTEN] traces that a preceding
 * isim_trace_spans_device of n_ids list entries wrote to d_off / d_spans, on
 * the current device, asynchronously on hip_stream.  The number of traces is
 * read on the device (at most n_ids, which bounds the grid).  In place: start_ns
 * filled as isim_trace_spans_place fills it, ISIM_SPAN_CRITICAL ORed into the
 * status of the critical spans.  ADDS into d_table (the caller zeroes it).  One
 * trace per lane: the spans are checked as isim_trace_spans_place checks them
 * (hop == j, caller_hop < j or the entry's sentinel, position and service in
 * range; offsets ascending, the range inside cap_spans and inside the written
 * spans d_off[written], at most 2^32 - 1 spans), a trace that fails is left
 * untouched and counted in ISIM_CP_H_REFUSED; every index read from a span is
 * bounded before use.  No host synchronisation, graph-capturable from the first
 * call, the workspace may be dirty (calls that share one must be ordered); the
 * first call of a handler on a device uploads the handler's tables, as
 * isim_trace_spans_device does.  n_ids 0 does nothing.  ISIM_EINVAL, before any
 * HIP call: the handlers isim_trace_spans_device refuses, a null argument,
 * n_ids above 2^32, cap_spans above 2^40, buffers not 8-byte aligned, a
 * workspace below isim_critical_path_workspace_bytes(h, cap_spans). */
ISIM_API int isim_critical_path_device(const isim_handler *h, const uint64_t *d_off, isim_span *d_spans,
                                       uint64_t cap_spans, const uint64_t *d_info, uint64_t n_ids, uint64_t *d_table,
                                       void *d_workspace, uint64_t workspace_bytes, void *hip_stream);
/* host only, no GPU: the same fold on the CPU over the n_written traces at
 * h_spans[h_off[i] .. h_off[i + 1]); a trace that reaches past h_off[n_written]
 * is refused.  ADDS into h_table. */
ISIM_API int isim_critical_path_host(const isim_handler *h, const uint64_t *h_off, uint64_t n_written,
                                     isim_span *h_spans, uint64_t *h_table);
/* Synchronous convenience: host buffers, on GPU `device`. */
ISIM_API int isim_critical_path(int device, const isim_handler *h, const uint64_t *h_off, uint64_t n_written,
                                isim_span *h_spans, uint64_t *h_table);

/* ---- DES trace spans: where the slow traces of a contended batch waited (EXT) ----
 * Under the DES an invocation's queue wait depends on every other trace of the
 * batch, so a trace cannot be walked again later: its arrival, start and finish
 * exist only in the item engine's per-batch arrays.  A tap on a DES batch
 * writes them out for chosen traces before the batch ends, and folds their
 * waits into a per-service table.  Item engine only (isim_des_info.items == 1:
 * a dynamic walk, or any graph under ISIM_FLAG_DYNAMIC).
 *
 * The spans of one trace are contiguous and in hop order.  All three times are
 * on the batch clock of isim_des_arrivals* (time 0 = the batch start).  The
 * entry's arrival_ns is the trace's A_t, its finish_ns - arrival_ns the
 * record's latency_ns.  With duration = finish_ns - arrival_ns next to hop_ns,
 * the winner rule of isim_critical_path (hop_ns + duration) reads unchanged. */
typedef struct {
  uint64_t arrival_ns;   /* a: the request reaches the replica's queue */
  uint64_t start_ns;     /* S: the worker takes it; S - a is the queue wait */
  uint64_t finish_ns;    /* F: the respond point */
  uint64_t hop_ns;       /* H of the call site; entry 0 */
  uint32_t hop;          /* as isim_span; entry 0 */
  uint32_t caller_hop;   /* as isim_span; 0xFFFFFFFF for the entry */
  uint32_t position;     /* as isim_span */
  uint32_t slot;         /* as isim_span; 0xFFFFFFFF for the entry */
  uint32_t service;      /* as isim_span */
  uint32_t status;       /* as isim_span: bit 0 responded 500, bit 1 its own error draw; bit 2 (ISIM_SPAN_CRITICAL)
                          * set by isim_des_critical_path* only */
  uint32_t replica;      /* the replica the §10.1 draw chose; 0 when the service has one */
  uint32_t reserved;     /* 0 */
} isim_des_span;         /* 64 bytes */

/* d_info: the four words of isim_trace_spans_device (ISIM_SPAN_TOTAL, _WRITTEN,
 * _N_IDS, _FIRST_UNFIT over the chosen list) and the matches before max_traces cut it */
#define ISIM_DES_SPAN_MATCHES 4
#define ISIM_DES_SPAN_INFO_WORDS 5

/* The wait table: (n_services + 1) rows of ISIM_DW_ROW_WORDS u64 words, ADDED
 * into (the caller zeroes it).  Row s < n_services, over the emitted spans of
 * service s: the words below.  The last row is the header.  Tables merge by
 * addition, except ISIM_DW_MAX_WAIT, which merges by MAX (isim_des_wait_merge). */
#define ISIM_DW_INVOCATIONS  0   /* emitted spans of s */
#define ISIM_DW_WAITED       1   /* those with S > a */
#define ISIM_DW_SUM_WAIT     2   /* sum of S - a */
#define ISIM_DW_MAX_WAIT     3   /* largest S - a */
#define ISIM_DW_SUM_DURATION 4   /* sum of F - a */
#define ISIM_DW_RESP_500     5   /* those that responded 500 */
#define ISIM_DW_ROW_WORDS    6
/* the header row (row n_services); its last two words are 0 */
#define ISIM_DW_H_TRACES      0  /* traces emitted */
#define ISIM_DW_H_SPANS       1  /* their spans */
#define ISIM_DW_H_SUM_LATENCY 2  /* the sum of their entries' F - a (the records' latency_ns) */
#define ISIM_DW_H_SUM_WAIT    3  /* the sum of their entries' own S - a */

/* Which traces, and where their spans go.  Chosen: the batch's records with
 * latency_ns >= threshold in class cls, ids ascending, the first max_traces of
 * them.  The threshold is min_latency_ns when q_ppm is 0; otherwise the exact
 * order statistic isim_quantile_rank(N_cls, q_ppm) of this batch's records in
 * that class (isim_latency_quantiles_device on the same stream; the host reads
 * that one word).  A trace's span count is its record's hops; the counts are
 * scanned into d_off; a trace whose range ends past cap_spans writes nothing,
 * so the traces that fit are a prefix of the list.  Words of d_ids and d_off
 * past the chosen list, and spans past d_off[written], are left untouched. */
typedef struct {
  uint64_t min_latency_ns;   /* the threshold when q_ppm == 0 */
  uint32_t q_ppm;            /* 0, or 1 .. 1000000 */
  uint32_t cls;              /* ISIM_Q_ALL / ISIM_Q_200 / ISIM_Q_500 */
  uint64_t max_traces;       /* <= 2^32 */
  uint64_t cap_spans;        /* <= 2^40 */
  uint64_t *d_ids;           /* [max_traces] (may be NULL when max_traces is 0) */
  uint64_t *d_off;           /* [max_traces + 1] */
  isim_des_span *d_spans;    /* [cap_spans] (may be NULL when cap_spans is 0) */
  uint64_t *d_info;          /* [ISIM_DES_SPAN_INFO_WORDS], written */
  uint64_t *d_wait_table;    /* NULL, or (n_services + 1) * ISIM_DW_ROW_WORDS words, added into */
  uint64_t reserved[2];      /* 0 */
} isim_des_tap;

/* host only, no GPU: (n_services + 1) * ISIM_DW_ROW_WORDS */
ISIM_API int isim_des_wait_table_words(const isim_handler *h, uint64_t *words);
/* host only, no GPU: dst += src, ISIM_DW_MAX_WAIT of the service rows by MAX */
ISIM_API int isim_des_wait_merge(const isim_handler *h, uint64_t *dst, const uint64_t *src);
/* One DES batch as isim_serve_des_device runs it (lp NULL: the constant mean
 * of p) or as isim_serve_des_profile_device runs it (lp given: p->flags are the
 * des_flags, p's mean is not read), with the same workspace.  With a NULL tap
 * it IS that call: records, stats and table bit for bit.  With a tap,
 * d_records is required, and the tap's kernels follow the batch on hip_stream
 * while its item arrays are alive; they do not walk the tree again.  The call
 * synchronises with the host as every item-engine batch does.  A batch that is
 * not accumulated (a look-back fault, or ISIM_ST_DES_RETRY) writes d_off[0] = 0
 * and a d_info with no trace written, no span and nothing to the table.
 * n_traces 0 with a tap does the same.  ISIM_EINVAL, before any HIP call: what
 * the two calls above refuse; with a tap: a handler whose DES is not on the
 * item engine (create it with ISIM_FLAG_DYNAMIC), null records, null or
 * misaligned tap buffers (8 bytes; d_spans 16), max_traces above 2^32,
 * cap_spans above 2^40, a class out of range, q_ppm above 1000000, nonzero
 * reserved words. */
ISIM_API int isim_serve_des_spans_device(isim_handler *h, const isim_des_params *p, const isim_load_profile *lp,
                                         uint64_t trace_begin, uint64_t n_traces, isim_trace_rec *d_records,
                                         uint64_t *d_stats, uint64_t *d_des_table, void *d_workspace,
                                         uint64_t workspace_bytes, const isim_des_tap *tap, void *hip_stream);
/* Synchronous convenience: host buffers, the tap's five pointers included (its
 * wait table is added into as well); h_records, h_stats and h_des_table may be NULL. */
ISIM_API int isim_serve_des_spans(isim_handler *h, int device, const isim_des_params *p,
                                  const isim_load_profile *lp, uint64_t trace_begin, uint64_t n_traces,
                                  isim_trace_rec *h_records, uint64_t *h_stats, uint64_t *h_des_table,
                                  const isim_des_tap *tap);

/* ---- DES critical path: queue wait, self time and hop cost per service (EXT) ----
 * The wait table above folds every wait of the tapped traces; it cannot say
 * which waits mattered: a long queue in a branch of a concurrent step that lost
 * anyway costs the trace nothing.  This fold marks the critical path of each
 * trace of isim_des_span records and splits its latency per service into queue
 * wait, self time and hop cost.
 *
 * Per span v: dur(v) = finish_ns - arrival_ns, wait(v) = start_ns - arrival_ns,
 * run(v) = finish_ns - start_ns.
 *
 * Replay.  A caller's script is replayed with the clock starting at the caller's
 * start_ns.  Its executed children, in hop order, are matched to the call
 * commands by the call index of their positions, as isim_critical_path matches
 * them.  A sleep adds max(d, 0).  A sequential call whose child c executed must
 * satisfy arrival_ns(c) == clock + hop_ns(c) and adds hop_ns(c) + dur(c).  In a
 * concurrent step every executed member must satisfy that equation at the
 * step's begin; the clock advances by the largest member value.
 *
 * Local winners, critical set: the rules of isim_critical_path with
 * duration_ns read as dur(c).
 *
 * Parts of a critical span: wait(v), hop_ns(v) and self(v) = run(v) - the sum
 * over v's local-winner children c of (hop_ns(c) + dur(c)).
 *
 * Identity.  Per trace the sum over its critical spans of (wait + self + hop_ns)
 * equals the entry's finish_ns - arrival_ns, the record's latency_ns.
 *
 * Refused traces (left untouched, counted in ISIM_DCP_H_REFUSED, by the host
 * and the device alike): offsets not ascending, past cap_spans or past the
 * written spans, more than 2^32 - 1 spans; a span with hop != j, a caller_hop
 * that is not j - 1 or one of its callers (the entry: not the sentinel, or a
 * hop_ns other than 0), a position or a service out of range, or not
 * arrival_ns <= start_ns <= finish_ns; a child whose arrival equation fails or
 * that matches no call command of its caller; a self below 0.
 *
 * The table: (n_services + 1) rows of ISIM_DCP_ROW_WORDS u64 words, every word
 * a sum mod 2^64, so tables merge by plain addition.  Row s < n_services: the
 * words below.  The last row is the header.  Per table the sum over s of
 * (WAIT_NS + SELF_NS + HOP_NS) equals the header's ISIM_DCP_H_SUM_LATENCY.
 * ISIM_SPAN_CRITICAL (bit 2) is ORed into isim_des_span.status of the critical
 * spans; nothing else in a span is written. */
#define ISIM_DCP_INVOCATIONS     0   /* every executed invocation of s in the folded traces */
#define ISIM_DCP_SUM_DURATION    1   /* the sum of their finish_ns - arrival_ns */
#define ISIM_DCP_CRITICAL        2   /* invocations of s on the path */
#define ISIM_DCP_WAIT_NS         3   /* the sum of the queue waits of the critical invocations */
#define ISIM_DCP_SELF_NS         4   /* the sum of their self times */
#define ISIM_DCP_HOP_NS          5   /* the sum of their hop_ns: the network time of the calls into s */
#define ISIM_DCP_CRITICAL_500    6   /* critical invocations that responded 500 */
#define ISIM_DCP_CRITICAL_WAITED 7   /* critical invocations with start_ns > arrival_ns */
#define ISIM_DCP_ROW_WORDS       8
/* the header row (row n_services); its last three words are 0 */
#define ISIM_DCP_H_TRACES      0  /* traces folded */
#define ISIM_DCP_H_SPANS       1  /* their spans */
#define ISIM_DCP_H_CRITICAL    2  /* their critical spans */
#define ISIM_DCP_H_SUM_LATENCY 3  /* the sum of their entries' finish_ns - arrival_ns */
#define ISIM_DCP_H_REFUSED     4  /* traces refused; left untouched, counted nowhere else */

/* host only, no GPU: (n_services + 1) * ISIM_DCP_ROW_WORDS */
ISIM_API int isim_des_critical_path_table_words(const isim_handler *h, uint64_t *words);
/* host only, no GPU: 16 bytes per span of the buffer plus 64 */
ISIM_API int isim_des_critical_path_workspace_bytes(const isim_handler *h, uint64_t cap_spans, uint64_t *bytes);
/* host only, no GPU: dst[w] += src[w] over the table's words */
ISIM_API int isim_des_critical_path_merge(const isim_handler *h, uint64_t *dst, const uint64_t *src);
/* The fold of the d_info[ISIM_SPAN_WRITTEN] traces that a preceding
 * isim_serve_des_spans_device with a tap of n_ids = max_traces list entries
 * wrote to d_off / d_spans, on the current device, asynchronously on
 * hip_stream.  The number of traces is read on the device (at most n_ids, which
 * bounds the grid).  ADDS into d_table (the caller zeroes it).  d_trace_wait:
 * NULL, or u64[n_ids]; entry i gets the sum of wait over the critical spans of
 * list entry i, UINT64_MAX for a refused trace; entries past the written count
 * are untouched.  One trace per wave.  No host synchronisation,
 * graph-capturable from the first call, the workspace may be dirty (calls that
 * share one must be ordered).  n_ids 0 does nothing.  ISIM_EINVAL, before any
 * HIP call: a handler isim_serve_des_spans_device refuses with a tap, a null
 * argument, n_ids above 2^32, cap_spans above 2^40, buffers not 8-byte aligned
 * (d_spans 16), a workspace below isim_des_critical_path_workspace_bytes(h,
 * cap_spans). */
ISIM_API int isim_des_critical_path_device(const isim_handler *h, const uint64_t *d_off, isim_des_span *d_spans,
                                           uint64_t cap_spans, const uint64_t *d_info, uint64_t n_ids,
                                           uint64_t *d_table, uint64_t *d_trace_wait, void *d_workspace,
                                           uint64_t workspace_bytes, void *hip_stream);
/* host only, no GPU: the same fold on the CPU over the n_written traces at
 * h_spans[h_off[i] .. h_off[i + 1]); a trace that reaches past h_off[n_written]
 * is refused.  ADDS into h_table; h_trace_wait NULL or u64[n_written]. */
ISIM_API int isim_des_critical_path_host(const isim_handler *h, const uint64_t *h_off, uint64_t n_written,
                                         isim_des_span *h_spans, uint64_t *h_table, uint64_t *h_trace_wait);
/* Synchronous convenience: host buffers, on GPU `device`. */
ISIM_API int isim_des_critical_path(int device, const isim_handler *h, const uint64_t *h_off, uint64_t n_written,
                                    isim_des_span *h_spans, uint64_t *h_table, uint64_t *h_trace_wait);

/* ---- service timeline: per-service queue depth and utilisation over time (EXT) ----
 * The timeline of isim_timeline* is the client's side of a load test.  This
 * fold is the servers' side: the isim_des_span records of a tapped batch
 * (threshold 0: every executed invocation) folded into a (service x window)
 * table, the figures a Prometheus scrape of each pod gives a real run.
 *
 * Rows: the isim_timeline_params rules and rows of isim_timeline.  Row 0
 * ("before") covers [0, t0); row 1 + w covers [t0 + w W, t0 + (w + 1) W) for
 * w < n_windows; row n_windows + 1 ("after") covers everything from
 * t0 + n_windows W on.
 *
 * A span v of service s with a = arrival_ns, S = start_ns, F = finish_ns has
 * point events at a, S and F, the queue interval [a, S) and the busy interval
 * [S, S + P_s), S + P_s saturating at 2^64 - 1; P_s is the worker hold of s,
 * the sleep total of its script (isim_des_service_holds).
 *
 * The overlap of an interval with a row is the length of their intersection
 * on the mathematical integers.  A row that would begin at or past 2^64
 * receives nothing; t0 + n_windows W is never formed in u64; over all rows the
 * overlaps of [x, y) sum to y - x exactly.
 *
 * The table: u64 [n_services][n_windows + 2][ISIM_SVT_ROW_WORDS], then one
 * header block of ISIM_SVT_ROW_WORDS words.  ADDED into (the caller zeroes
 * it).  Every word is a sum mod 2^64 except ISIM_SVT_MAX_WAIT, which merges by
 * MAX: tables fold across batches, shards and GPUs, on the device by calling
 * again and on the host with isim_service_timeline_merge.
 *
 * A span is refused if its service >= n_services or if a <= S <= F does not
 * hold.  A refused span counts in ISIM_SVT_H_REFUSED and adds to nothing else;
 * the host and the device refuse the same spans.
 *
 * Derived: the mean queue length of a window is QUEUED_NS / window_ns, the
 * utilisation BUSY_NS / (window_ns x replicas x workers, isim_des_workers_get), the queue depth at the end of
 * row r the cumulative ARRIVED - STARTED over the rows <= r. */
#define ISIM_SVT_ARRIVED   0   /* spans of s whose a falls in the row */
#define ISIM_SVT_STARTED   1   /* spans whose S falls in it */
#define ISIM_SVT_FINISHED  2   /* [2] spans whose F falls in it, by code (status bit 0) */
#define ISIM_SVT_SUM_WAIT  4   /* the sum of S - a over the spans STARTED in the row */
#define ISIM_SVT_MAX_WAIT  5   /* the largest of those (merges by MAX) */
#define ISIM_SVT_QUEUED_NS 6   /* the sum of the overlaps of [a, S) with the row: the integral of the queue length */
#define ISIM_SVT_BUSY_NS   7   /* the sum of the overlaps of [S, S + P_s) with the row: worker-busy time, all replicas */
#define ISIM_SVT_ROW_WORDS 8
/* the header block (after the last service's rows); its other words are 0 */
#define ISIM_SVT_H_FOLDED  0   /* spans folded */
#define ISIM_SVT_H_REFUSED 1   /* spans refused */
#define ISIM_SVT_MAX_CELLS (1u << 24)   /* n_services * (n_windows + 2) at most */

/* Every call below returns ISIM_EINVAL, before any HIP call, for a handler
 * isim_serve_des_spans_device refuses with a tap, a null argument, parameters
 * isim_timeline refuses, or n_services * (n_windows + 2) above ISIM_SVT_MAX_CELLS. */
/* host only, no GPU: per service its worker hold P_s in ns and its replicas (at least 1); [n_services] each */
ISIM_API int isim_des_service_holds(const isim_handler *h, uint64_t *hold_ns, uint32_t *replicas);
/* host only, no GPU: (n_services * (n_windows + 2) + 1) * ISIM_SVT_ROW_WORDS */
ISIM_API int isim_service_timeline_table_words(const isim_handler *h, const isim_timeline_params *p, uint64_t *words);
/* host only, no GPU: 16 bytes per (service, row), at least 64 */
ISIM_API int isim_service_timeline_workspace_bytes(const isim_handler *h, const isim_timeline_params *p,
                                                   uint64_t *bytes);
/* host only, no GPU: dst[w] += src[w], ISIM_SVT_MAX_WAIT of the rows by MAX */
ISIM_API int isim_service_timeline_merge(const isim_handler *h, const isim_timeline_params *p, uint64_t *dst,
                                         const uint64_t *src);
/* The fold of the spans that a preceding isim_serve_des_spans_device wrote to
 * d_spans, on the current device, asynchronously on hip_stream.  The span
 * count is read on the device: d_off[d_info[ISIM_SPAN_WRITTEN]], bounded by
 * cap_spans (which sizes the grid); d_off and d_info are the tap's.  ADDS into
 * d_table.  No host synchronisation, graph-capturable from the first call,
 * the workspace may be dirty (calls that share one must be ordered).
 * cap_spans 0 does nothing.  Also ISIM_EINVAL: cap_spans above 2^40, buffers
 * not 8-byte aligned (d_spans 16), a workspace below
 * isim_service_timeline_workspace_bytes. */
ISIM_API int isim_service_timeline_device(const isim_handler *h, const isim_timeline_params *p, const uint64_t *d_off,
                                          const isim_des_span *d_spans, uint64_t cap_spans, const uint64_t *d_info,
                                          uint64_t *d_table, void *d_workspace, uint64_t workspace_bytes,
                                          void *hip_stream);
/* host only, no GPU: the same fold on the CPU over h_spans[0 .. n_spans); ADDS into h_table */
ISIM_API int isim_service_timeline_host(const isim_handler *h, const isim_timeline_params *p,
                                        const isim_des_span *h_spans, uint64_t n_spans, uint64_t *h_table);
/* Synchronous convenience: host buffers, on GPU `device`. */
ISIM_API int isim_service_timeline(int device, const isim_handler *h, const isim_timeline_params *p,
                                   const isim_des_span *h_spans, uint64_t n_spans, uint64_t *h_table);

/* ---- per-service exact percentiles of queue wait, service time and duration (EXT) ----
 * The per-service view of service_request_duration_seconds: for every service
 * the exact order statistics of three measures over the isim_des_span records
 * of a tapped batch (threshold 0: every executed invocation).
 *
 * A span is refused by the rule of isim_service_timeline: service >=
 * n_services, or a <= S <= F does not hold (a = arrival_ns, S = start_ns,
 * F = finish_ns).  A refused span counts in ISIM_SVQ_H_REFUSED and in nothing
 * else; the host and the device refuse the same spans.
 *
 * Measures, per span that is not refused: */
#define ISIM_SVQ_WAIT     0   /* S - a: the queue wait */
#define ISIM_SVQ_SERVICE  1   /* F - S: from the worker taking it to the respond point */
#define ISIM_SVQ_DURATION 2   /* F - a: what RecordResponseSent observes */
#define ISIM_SVQ_MEASURES 3
/* Classes: ISIM_Q_ALL, ISIM_Q_200, ISIM_Q_500, the code being status bit 0. */
#define ISIM_SVQ_CLASSES  3
/* The table: u64 [n_services][ISIM_SVQ_MEASURES][ISIM_SVQ_CLASSES][1 + n_q],
 * then a header of ISIM_SVQ_HEADER_WORDS words.  Word 0 of a cell is the count
 * N of that service and class (the same for the three measures); word 1 + i is
 * the k-th smallest value of the measure among them, k =
 * isim_quantile_rank(N, q_ppm[i]); every word of a cell is 0 where N is 0.
 * The table is WRITTEN, not added into (order statistics do not merge): every
 * word is written by the call, and the table may be dirty.  q_ppm: the rules of
 * isim_latency_quantiles (1 .. ISIM_MAX_QUANTILES entries, each <= 1,000,000,
 * copied at the call). */
#define ISIM_SVQ_H_FOLDED  0   /* spans folded */
#define ISIM_SVQ_H_REFUSED 1   /* spans refused */
#define ISIM_SVQ_HEADER_WORDS 2
#define ISIM_SVQ_MAX_SPANS 0xFFFFFFFFull   /* u32 counters, offsets and ranks */
/* The device call selects a service with at most ISIM_SVQ_STAGE spans in LDS,
 * one workgroup per service.  A longer segment is cut into chunks of
 * ISIM_SVQ_CHUNK elements that many workgroups histogram, digit by digit. */
#define ISIM_SVQ_STAGE 3584
#define ISIM_SVQ_CHUNK 4096
#define ISIM_SVQ_SLOT_BYTES 3584   /* workspace of a long segment besides its bins */

/* Every call below returns ISIM_EINVAL, before any HIP call, for a handler
 * isim_serve_des_spans_device refuses with a tap, a null argument, a quantile
 * list isim_latency_quantiles refuses, or more than ISIM_SVQ_MAX_SPANS spans. */
/* host only, no GPU: n_services * 9 * (1 + n_q) + ISIM_SVQ_HEADER_WORDS */
ISIM_API int isim_service_quantiles_table_words(const isim_handler *h, uint32_t n_q, uint64_t *words);
/* host only, no GPU.  With P(x) = x rounded up to a multiple of 256:
 *   256 + 3 * P(8 * n_services)                        per service: counts, offsets and cursors by (service, code)
 *   + 24 * cap_spans                                   per span: its three measures, scattered by service
 *   + L * (ISIM_SVQ_SLOT_BYTES + 9 * n_q * 1024)       per long segment: select states and u32 bins
 * where L = min(n_services, cap_spans / (ISIM_SVQ_STAGE + 1)) is the most long segments cap_spans spans can form. */
ISIM_API int isim_service_quantiles_workspace_bytes(const isim_handler *h, uint64_t cap_spans, uint32_t n_q,
                                                    uint64_t *bytes);
/* The table of the spans that a preceding isim_serve_des_spans_device wrote to
 * d_spans, on the current device, asynchronously on hip_stream.  The span
 * count is read on the device: d_off[d_info[ISIM_SPAN_WRITTEN]], bounded by
 * cap_spans (which sizes the grids and the workspace); d_off and d_info are the
 * tap's.  WRITES d_out.  A fixed sequence of kernels that does not depend on
 * the data: no host synchronisation, no allocation, graph-capturable from the
 * first call, the workspace may be dirty (calls that share one must be
 * ordered).  cap_spans 0 writes zeros and needs no workspace.  Also
 * ISIM_EINVAL: buffers not 8-byte aligned (d_spans 16), a workspace below
 * isim_service_quantiles_workspace_bytes. */
ISIM_API int isim_service_quantiles_device(const isim_handler *h, const uint32_t *q_ppm, uint32_t n_q,
                                           const uint64_t *d_off, const isim_des_span *d_spans, uint64_t cap_spans,
                                           const uint64_t *d_info, uint64_t *d_out, void *d_workspace,
                                           uint64_t workspace_bytes, void *hip_stream);
/* host only, no GPU: the same table on the CPU over h_spans[0 .. n_spans) (a sort per service, measure and class) */
ISIM_API int isim_service_quantiles_host(const isim_handler *h, const uint32_t *q_ppm, uint32_t n_q,
                                         const isim_des_span *h_spans, uint64_t n_spans, uint64_t *h_out);
/* Synchronous convenience: host buffers, on GPU `device`. */
ISIM_API int isim_service_quantiles(int device, const isim_handler *h, const uint32_t *q_ppm, uint32_t n_q,
                                    const isim_des_span *h_spans, uint64_t n_spans, uint64_t *h_out);

/* ---- per-service exact percentiles over time (EXT) ----
 * histogram_quantile(0.99, service_request_duration_seconds) by service, over
 * time: for every service and timeline row the exact order statistics of the
 * three measures of isim_service_quantiles over the isim_des_span records of a
 * tapped batch (threshold 0: every executed invocation).
 *
 * A span is refused by the rule of isim_service_timeline: service >=
 * n_services, or a <= S <= F does not hold (a = arrival_ns, S = start_ns,
 * F = finish_ns).  A refused span counts in ISIM_SVQ_H_REFUSED and in nothing
 * else; the host and the device refuse the same spans.
 *
 * Rows: those of isim_timeline under an isim_timeline_params (row 0 "before"
 * t0_ns, rows 1 .. n_windows the windows, row n_windows + 1 "after"), with the
 * parameter errors of isim_timeline.  A span belongs to the row in which its
 * finish F falls, the convention of ISIM_SVT_FINISHED and of
 * isim_timeline_quantiles (what completes in the row).  t0_ns + n_windows *
 * window_ns is never formed: any u64 parameters and times are exact.
 *
 * Measures ISIM_SVQ_WAIT / ISIM_SVQ_SERVICE / ISIM_SVQ_DURATION and classes
 * ISIM_Q_ALL / ISIM_Q_200 / ISIM_Q_500 (status bit 0): isim_service_quantiles'.
 *
 * The table: u64 [n_services][n_windows + 2][ISIM_SVQ_MEASURES][ISIM_SVQ_CLASSES]
 * [1 + n_q], then a header of ISIM_SVQ_HEADER_WORDS words (ISIM_SVQ_H_FOLDED,
 * ISIM_SVQ_H_REFUSED).  Word 0 of a cell is the count N of that service, row
 * and class (the same for the three measures); word 1 + i is the k-th smallest
 * value of the measure among them, k = isim_quantile_rank(N, q_ppm[i]); every
 * word of a cell is 0 where N is 0.  The table is WRITTEN, not added into:
 * every word is written by the call, and the table may be dirty.  q_ppm: the
 * rules of isim_latency_quantiles. */
#define ISIM_SWQ_MAX_CELLS (1u << 20)   /* n_services * (n_windows + 2); at 16 quantiles the table is 1.2 GiB */
/* The device call ranks a cell of at most ISIM_SWQ_WAVE spans in the registers
 * of one wave; a cell of up to ISIM_SVQ_STAGE spans is selected in LDS by one
 * workgroup; a longer one in chunks of ISIM_SVQ_CHUNK, as isim_service_quantiles
 * does. */
#define ISIM_SWQ_WAVE 256

/* Every call below returns ISIM_EINVAL, before any HIP call, for what
 * isim_service_quantiles refuses (the handler, a null argument, the quantile
 * list, more than ISIM_SVQ_MAX_SPANS spans), for parameters isim_timeline
 * refuses, and for more than ISIM_SWQ_MAX_CELLS cells. */
/* host only, no GPU: C * 9 * (1 + n_q) + ISIM_SVQ_HEADER_WORDS with C = n_services * (n_windows + 2) */
ISIM_API int isim_service_window_quantiles_table_words(const isim_handler *h, const isim_timeline_params *p,
                                                       uint32_t n_q, uint64_t *words);
/* host only, no GPU.  With P(x) = x rounded up to a multiple of 256 and C the cells:
 *   256 + 3 * P(8 * C)                                 per cell: counts, offsets and cursors by (cell, code)
 *   + P(4 * M)                                         the list of the cells selected in LDS
 *   + 24 * cap_spans                                   per span: its three measures, scattered by cell
 *   + L * (ISIM_SVQ_SLOT_BYTES + 9 * n_q * 1024)       per long segment: select states and u32 bins
 * where M = min(C, cap_spans / (ISIM_SWQ_WAVE + 1)) and L = min(C, cap_spans / (ISIM_SVQ_STAGE + 1)) are the
 * most cells of either kind cap_spans spans can form. */
ISIM_API int isim_service_window_quantiles_workspace_bytes(const isim_handler *h, const isim_timeline_params *p,
                                                           uint64_t cap_spans, uint32_t n_q, uint64_t *bytes);
/* The table of the spans that a preceding isim_serve_des_spans_device wrote to
 * d_spans, addressed as isim_service_quantiles_device addresses them (the span
 * count is read on the device and bounded by cap_spans), on the current
 * device, asynchronously on hip_stream.  WRITES d_out.  A fixed sequence of
 * kernels that does not depend on the data: no host synchronisation, no
 * allocation, graph-capturable from the first call, the workspace may be dirty
 * (calls that share one must be ordered).  cap_spans 0 writes zeros and needs
 * no workspace.  Also ISIM_EINVAL: buffers not 8-byte aligned (d_spans 16), a
 * workspace below isim_service_window_quantiles_workspace_bytes. */
ISIM_API int isim_service_window_quantiles_device(const isim_handler *h, const isim_timeline_params *p,
                                                  const uint32_t *q_ppm, uint32_t n_q, const uint64_t *d_off,
                                                  const isim_des_span *d_spans, uint64_t cap_spans,
                                                  const uint64_t *d_info, uint64_t *d_out, void *d_workspace,
                                                  uint64_t workspace_bytes, void *hip_stream);
/* host only, no GPU: the same table on the CPU over h_spans[0 .. n_spans) (a sort per cell, measure and class) */
ISIM_API int isim_service_window_quantiles_host(const isim_handler *h, const isim_timeline_params *p,
                                                const uint32_t *q_ppm, uint32_t n_q, const isim_des_span *h_spans,
                                                uint64_t n_spans, uint64_t *h_out);
/* Synchronous convenience: host buffers, on GPU `device`. */
ISIM_API int isim_service_window_quantiles(int device, const isim_handler *h, const isim_timeline_params *p,
                                           const uint32_t *q_ppm, uint32_t n_q, const isim_des_span *h_spans,
                                           uint64_t n_spans, uint64_t *h_out);

/* ---- per-service latency sketch: percentiles across batches and GPUs (EXT) ----
 * The mergeable counterpart of isim_service_quantiles: for every service one
 * isim_latency_sketch table per measure, filled from the isim_des_span records
 * of a tapped batch (threshold 0: every executed invocation).  Exact order
 * statistics need every span of the population in one buffer; these words are
 * counts, so tables of many batches and GPUs merge by addition, and a quantile
 * comes back as the bracket of isim_sketch_quantiles.
 *
 * A span is refused by the rule of isim_service_timeline: service >=
 * n_services, or a <= S <= F does not hold (a = arrival_ns, S = start_ns,
 * F = finish_ns).  A refused span counts in ISIM_SVQ_H_REFUSED and in nothing
 * else; the host and the device refuse the same spans.  Measures ISIM_SVQ_WAIT
 * / ISIM_SVQ_SERVICE / ISIM_SVQ_DURATION: isim_service_quantiles'.  The code is
 * status bit 0.
 *
 * The table: u64 [n_services][ISIM_SVQ_MEASURES][2][ISIM_SK_BINS(s)], then a
 * header of ISIM_SVQ_HEADER_WORDS words (ISIM_SVQ_H_FOLDED, ISIM_SVQ_H_REFUSED).
 * Each [2][ISIM_SK_BINS(s)] block is a table of isim_latency_sketch, indexed by
 * code then bin, s = sub_bits in 0 .. ISIM_SK_MAX_SUB_BITS: isim_sketch_bucket,
 * isim_sketch_bounds, isim_sketch_merge (n_rows = 3 * n_services, the header
 * apart) and isim_sketch_quantiles apply to it unchanged.  A span that is not
 * refused adds 1 to one word of each of its service's three blocks.
 *
 * The table is ACCUMULATED INTO, the header included: the caller zeroes it
 * once, and a call adds only to the words it hits.  A batch the engine did not
 * accumulate (d_off[0] = 0, nothing written) adds nothing.  Tables merge by
 * plain addition of every word (a SUM all-reduce of the raw words across GPUs;
 * no RCCL entry point, as for isim_latency_sketch). */
#define ISIM_SVS_MAX_WORDS (1ull << 32)   /* a table of this many words or more is refused: a word index fits the
                                             u32 the peel compares; 100,000 services at s = 3 are 297,600,002 */
/* The device call adds a service with at most ISIM_SVS_SHORT spans straight
 * into the table, whole services per wave; a longer one is cut into chunks of
 * ISIM_SVQ_CHUNK elements, each histogrammed in LDS by one workgroup. */
#define ISIM_SVS_SHORT 256

/* Every call below returns ISIM_EINVAL, before any HIP call, for a handler
 * isim_service_quantiles refuses and a null argument; those that take sub_bits
 * for sub_bits above ISIM_SK_MAX_SUB_BITS and for a table of ISIM_SVS_MAX_WORDS
 * words or more at that sub_bits; those that take a span count for more than
 * ISIM_SVQ_MAX_SPANS spans. */
/* host only, no GPU: n_services * 3 * 2 * ISIM_SK_BINS(sub_bits) + ISIM_SVQ_HEADER_WORDS */
ISIM_API int isim_service_sketch_table_words(const isim_handler *h, uint32_t sub_bits, uint64_t *words);
/* host only, no GPU.  With P(x) = x rounded up to a multiple of 256:
 *   256 + 3 * P(8 * n_services)                        per service: counts, offsets and cursors by (service, code)
 *   + 24 * cap_spans                                   per span: its three measures, scattered by service
 *   + L * ISIM_SVQ_SLOT_BYTES                          per long segment: its record
 * where L = min(n_services, cap_spans / (ISIM_SVS_SHORT + 1)) is the most long segments cap_spans spans can form.
 * It does not depend on sub_bits (the long segments' bins are in LDS), so the table's bound is not this call's. */
ISIM_API int isim_service_sketch_workspace_bytes(const isim_handler *h, uint64_t cap_spans, uint64_t *bytes);
/* host only, no GPU: dst[i] += src[i] for every word of the table, the header included */
ISIM_API int isim_service_sketch_merge(const isim_handler *h, uint32_t sub_bits, uint64_t *dst, const uint64_t *src);
/* host only, no GPU: out is u64 [n_services][ISIM_SVQ_MEASURES][ISIM_SKQ_OUT_WORDS(n_q)], isim_sketch_quantiles of
 * each (service, measure) block, with its errors (the quantile list, a class count above 2^40) */
ISIM_API int isim_service_sketch_quantiles(const isim_handler *h, uint32_t sub_bits, const uint64_t *table,
                                           const uint32_t *q_ppm, uint32_t n_q, uint64_t *out);
/* Adds the spans that a preceding isim_serve_des_spans_device wrote to d_spans
 * into d_table, on the current device, asynchronously on hip_stream.  The
 * spans are addressed as isim_service_quantiles_device addresses them: the
 * count is read on the device, d_off[d_info[ISIM_SPAN_WRITTEN]], bounded by
 * cap_spans (which sizes the grids and the workspace); d_off and d_info are the
 * tap's.  A fixed sequence of kernels that does not depend on the data: no
 * host synchronisation, no allocation, graph-capturable from the first call,
 * the workspace may be dirty (calls that share one, or one table, must be
 * ordered).  cap_spans 0 touches nothing and needs no workspace.  Also
 * ISIM_EINVAL: buffers not 8-byte aligned (d_spans 16), a workspace below
 * isim_service_sketch_workspace_bytes. */
ISIM_API int isim_service_sketch_device(const isim_handler *h, uint32_t sub_bits, const uint64_t *d_off,
                                        const isim_des_span *d_spans, uint64_t cap_spans, const uint64_t *d_info,
                                        uint64_t *d_table, void *d_workspace, uint64_t workspace_bytes,
                                        void *hip_stream);
/* host only, no GPU: the same fold on the CPU over h_spans[0 .. n_spans), a plain loop; ADDS into h_table */
ISIM_API int isim_service_sketch_host(const isim_handler *h, uint32_t sub_bits, const isim_des_span *h_spans,
                                      uint64_t n_spans, uint64_t *h_table);
/* Synchronous convenience: host buffers, on GPU `device`; ADDS into h_table. */
ISIM_API int isim_service_sketch(int device, const isim_handler *h, uint32_t sub_bits, const isim_des_span *h_spans,
                                 uint64_t n_spans, uint64_t *h_table);

#ifdef __cplusplus
}
#endif
#endif /* ISIM_H */
